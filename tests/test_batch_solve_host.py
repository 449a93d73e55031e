"""Host-only side of the batched solve with phase 1 in the kernel (include/lpx.h: lpx_batch_solve_lds_bytes, lpx_batch_solve,
lpx_batch_shape, lpx_solve_batch_all): the LDS formula and the argument checks that come before any device call, so
they answer on a machine without a GPU too."""
import ctypes as C

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lpxlib():
    import __graft_entry__ as g
    import os
    from linear_programming_solver_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    _lib.lib()
    return _lib


def ev(x):
    return (x + 1) & ~1


def test_solve_lds_bytes_formula(lpxlib):
    L = lpxlib.lib()
    for m, n in [(0, 0), (1, 1), (5, 63), (5, 64), (64, 64), (33, 130), (96, 200)]:
        want = L.lpx_batch_lds_bytes(m, n + 1) + 16 * ev(n)    # the auxiliary LP, c0[n], order and slots 2 x int32[n]
        assert L.lpx_batch_solve_lds_bytes(m, n) == want, (m, n)
        assert want % 16 == 0
    assert L.lpx_batch_solve_lds_bytes(64, 64) == 36896


def test_solve_lds_bytes_monotone_and_above_the_aux_lp(lpxlib):
    L = lpxlib.lib()
    for m in range(0, 70, 3):
        for n in range(0, 70, 3):
            here = L.lpx_batch_solve_lds_bytes(m, n)
            assert here >= L.lpx_batch_lds_bytes(m, n + 1), (m, n)
            assert L.lpx_batch_solve_lds_bytes(m + 1, n) >= here, (m, n)
            assert L.lpx_batch_solve_lds_bytes(m, n + 1) >= here, (m, n)
    assert L.lpx_batch_solve_lds_bytes(-1, 3) == -1
    assert L.lpx_batch_solve_lds_bytes(3, -1) == -1
    assert "negative" in lpxlib.last_error()
    # far beyond any LDS: still a number above the limit, no overflow
    assert L.lpx_batch_solve_lds_bytes(2 ** 31 - 1, 2 ** 31 - 2) > lpxlib.BATCH_LDS_BYTES


def largest_rows(L, fn, n, limit):
    m = 1
    while fn(m + 1, n) <= limit:
        m += 1
    return m


def test_largest_phase1_form_with_200_columns(lpxlib):
    L = lpxlib.lib()
    m1 = largest_rows(L, L.lpx_batch_solve_lds_bytes, 200, lpxlib.BATCH_LDS_BYTES)
    m0 = largest_rows(L, L.lpx_batch_lds_bytes, 200, lpxlib.BATCH_LDS_BYTES)
    assert m1 == 96 and m0 == 98     # what include/lpx.h quotes


def call_all(lpxlib, count, m_max, n_max, A, lda, b, c, results="own", opts=None, maximize=None):
    L = lpxlib.lib()
    res = (lpxlib.SolveResult * max(count, 1))() if results == "own" else results
    took = C.c_int32(-5)
    rc = L.lpx_solve_batch_all(count, m_max, n_max, None, None, A.ctypes.data_as(lpxlib.dp), lda, m_max * lda,
                               b.ctypes.data_as(lpxlib.dp), c.ctypes.data_as(lpxlib.dp),
                               None if maximize is None else maximize.ctypes.data_as(lpxlib.ip),
                               None if opts is None else C.byref(opts), res, None, None, C.byref(took))
    return rc, took.value


def test_solve_batch_all_refuses_bad_arguments_before_any_device_call(lpxlib):
    A, b, c = np.ones((2, 3, 4)), -np.ones((2, 3)), np.ones((2, 4))
    BAD = lpxlib.BAD_ARGUMENT
    rc, took = call_all(lpxlib, -1, 3, 4, A, 4, b, c)
    assert rc == BAD and took == 0 and "negative" in lpxlib.last_error()
    rc, _ = call_all(lpxlib, 2, 3, 4, A, 3, b, c)                                   # lda < n_max
    assert rc == BAD and "lda" in lpxlib.last_error()
    rc, _ = call_all(lpxlib, 2, 3, 4, A, 4, b, c, results=None)
    assert rc == BAD and "results" in lpxlib.last_error()
    x = np.zeros(4)
    opts = lpxlib.SolveOptions()
    opts.max_pivots = -1
    opts.x_out = x.ctypes.data_as(lpxlib.dp)
    rc, _ = call_all(lpxlib, 2, 3, 4, A, 4, b, c, opts=opts)
    assert rc == BAD and "x_out" in lpxlib.last_error()
    # too large even without phase 1 (b >= 0): 99 x 200 is one row past the LDS
    big_A, big_b, big_c = np.ones((1, 99, 200)), np.ones((1, 99)), np.ones((1, 200))
    rc, _ = call_all(lpxlib, 1, 99, 200, big_A, 200, big_b, big_c)
    assert rc == BAD and "LP 0" in lpxlib.last_error() and "99 x 200" in lpxlib.last_error()
    # a restore order that names a variable the form does not have
    order = np.array([0, 1, 2, 7], dtype=np.int32)
    opts = lpxlib.SolveOptions()
    opts.max_pivots = -1
    opts.restore_order = order.ctypes.data_as(lpxlib.ip)
    opts.restore_order_len = 4
    rc, _ = call_all(lpxlib, 2, 3, 4, A, 4, b, c, opts=opts)
    assert rc == BAD and "LP 0" in lpxlib.last_error() and "variable 7" in lpxlib.last_error()


def test_null_handles(lpxlib):
    L = lpxlib.lib()
    res = (lpxlib.SolveResult * 1)()
    assert L.lpx_batch_solve(None, None, -1, None, None, res) == lpxlib.BAD_ARGUMENT
    assert "NULL handle" in lpxlib.last_error()
    m, n = C.c_int32(), C.c_int32()
    assert L.lpx_batch_shape(None, 0, C.byref(m), C.byref(n)) == lpxlib.BAD_ARGUMENT


def test_solve_batch_rejects_an_unknown_phase1_mode(lpxlib):
    from linear_programming_solver_amd import LPSolver
    with pytest.raises(ValueError):
        LPSolver().solve_batch([], phase1="device")
