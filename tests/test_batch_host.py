"""Host side of the batched solve (lpx_batch, LPBatch): the LDS formula, the argument checks that must answer before any
device call, and the packing of heterogeneous shapes.  Runs without a GPU."""
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


def lds_formula(m, n):
    """include/lpx.h, lpx_batch_lds_bytes: the documented formula restated."""
    ev = lambda x: (x + 1) // 2 * 2
    ld = n | 1
    return 8 * (ev(m * ld + m + n + 1) + ev((n + m + 1) // 2) + ev(m)) + 512


def largest_rows(lpxlib, n):
    """Largest m such that an m x n LP fits one workgroup's LDS."""
    L = lpxlib.lib()
    m = 0
    while L.lpx_batch_lds_bytes(m + 1, n) <= lpxlib.BATCH_LDS_BYTES:
        m += 1
    return m


def test_lds_bytes_follows_the_documented_formula_and_is_monotone(lpxlib):
    L = lpxlib.lib()
    for m in (0, 1, 2, 3, 7, 8, 63, 64, 65, 98, 99, 200):
        for n in (0, 1, 2, 3, 12, 63, 64, 65, 200, 257):
            got = L.lpx_batch_lds_bytes(m, n)
            assert got == lds_formula(m, n), (m, n)
            assert got % 16 == 0
            assert L.lpx_batch_lds_bytes(m + 1, n) >= got, (m, n)
            assert L.lpx_batch_lds_bytes(m, n + 1) >= got, (m, n)
    assert L.lpx_batch_lds_bytes(-1, 3) == -1 and L.lpx_batch_lds_bytes(3, -1) == -1
    assert L.lpx_batch_lds_bytes(2**31 - 1, 2**31 - 1) > lpxlib.BATCH_LDS_BYTES


def test_four_64x64_lps_share_a_cu(lpxlib):
    assert lpxlib.lib().lpx_batch_lds_bytes(64, 64) * 4 <= lpxlib.BATCH_LDS_BYTES


def test_largest_fit_with_200_columns_and_one_past_it(lpxlib):
    """The shapes tests/test_gpu_batch.py solves (largest fit) and expects to be refused (one more row)."""
    L = lpxlib.lib()
    m = largest_rows(lpxlib, 200)
    assert m == 98
    assert L.lpx_batch_lds_bytes(m, 200) <= lpxlib.BATCH_LDS_BYTES < L.lpx_batch_lds_bytes(m + 1, 200)


def _create(lpxlib, count, m_max, n_max, m=None, n=None, lda=None, have_arrays=True):
    L = lpxlib.lib()
    lda = max(n_max, 1) if lda is None else lda
    A = np.ones((max(count, 1), max(m_max, 1), max(lda, 1)))
    b = np.ones((max(count, 1), max(m_max, 1)))
    c = np.ones((max(count, 1), max(n_max, 1)))
    mm = None if m is None else np.array(m, dtype=np.int32)
    nn = None if n is None else np.array(n, dtype=np.int32)
    h = C.c_void_p()
    rc = L.lpx_batch_create(count, m_max, n_max, None if mm is None else mm.ctypes.data_as(lpxlib.ip),
                            None if nn is None else nn.ctypes.data_as(lpxlib.ip),
                            A.ctypes.data_as(lpxlib.dp) if have_arrays else None, lda, max(m_max, 1) * max(lda, 1),
                            b.ctypes.data_as(lpxlib.dp) if have_arrays else None,
                            c.ctypes.data_as(lpxlib.dp) if have_arrays else None, None, None, 0, C.byref(h))
    if rc == 0:
        L.lpx_batch_destroy(h)
    return rc, lpxlib.last_error()


def test_batch_create_refuses_bad_arguments_before_any_device_call(lpxlib):
    BAD = lpxlib.BAD_ARGUMENT
    assert _create(lpxlib, -1, 4, 4)[0] == BAD                         # negative count
    assert _create(lpxlib, 2, -4, 4)[0] == BAD                         # negative dimension
    assert _create(lpxlib, 2, 4, 6, lda=5)[0] == BAD                   # lda < n_max
    assert _create(lpxlib, 2, 4, 4, have_arrays=False)[0] == BAD       # NULL where data is due
    assert _create(lpxlib, 2, 4, 4, m=[4, 5], n=[4, 4])[0] == BAD      # a shape outside m_max x n_max
    m_fit = largest_rows(lpxlib, 200)
    rc, msg = _create(lpxlib, 3, m_fit + 1, 200, m=[3, m_fit + 1, 3], n=[5, 200, 5])
    assert rc == BAD                                                   # LP 1 does not fit the LDS of a workgroup
    assert "LP 1" in msg and "%d x 200" % (m_fit + 1) in msg, msg


def _solve_batch(lpxlib, count, m_max, n_max, lda=None, x_out=False):
    L = lpxlib.lib()
    lda = max(n_max, 1) if lda is None else lda
    A = np.ones((max(count, 1), max(m_max, 1), max(lda, 1)))
    b = np.ones((max(count, 1), max(m_max, 1)))
    c = np.ones((max(count, 1), max(n_max, 1)))
    maxi = np.ones(max(count, 1), dtype=np.int32)
    res = (lpxlib.SolveResult * max(count, 1))()
    opts = lpxlib.SolveOptions()
    opts.max_pivots = -1
    x = np.zeros(max(n_max, 1))
    if x_out:
        opts.x_out = x.ctypes.data_as(lpxlib.dp)
    nin = C.c_int32(-7)
    rc = L.lpx_solve_batch(count, m_max, n_max, None, None, A.ctypes.data_as(lpxlib.dp), lda,
                           max(m_max, 1) * max(lda, 1), b.ctypes.data_as(lpxlib.dp), c.ctypes.data_as(lpxlib.dp),
                           maxi.ctypes.data_as(lpxlib.ip), C.byref(opts), res, C.byref(nin))
    return rc, nin.value


def test_solve_batch_refuses_bad_arguments_before_any_device_call(lpxlib):
    BAD = lpxlib.BAD_ARGUMENT
    assert _solve_batch(lpxlib, -1, 4, 4) == (BAD, 0)                  # negative count
    assert _solve_batch(lpxlib, 2, 4, 6, lda=5) == (BAD, 0)            # lda < n_max
    m_fit = largest_rows(lpxlib, 200)
    assert _solve_batch(lpxlib, 2, m_fit + 1, 200) == (BAD, 0)         # does not fit
    assert "%d x 200" % (m_fit + 1) in lpxlib.last_error()
    assert _solve_batch(lpxlib, 2, 4, 4, x_out=True) == (BAD, 0)       # x_out must be NULL


def test_batch_handle_calls_refuse_null_and_bad_options(lpxlib):
    L = lpxlib.lib()
    assert L.lpx_batch_count(None) == 0
    assert L.lpx_batch_set_option(None, lpxlib.OPTIONS["fused"], 1) == lpxlib.BAD_ARGUMENT
    assert L.lpx_batch_set_pricing(None, 0) == lpxlib.BAD_ARGUMENT
    assert L.lpx_batch_simplex_loop(None, -1, None, None, None) == lpxlib.BAD_ARGUMENT
    assert L.lpx_batch_read(None, 0, None, 1, None, None, None, None) == lpxlib.BAD_ARGUMENT


def test_exception_for_status_returns_what_raise_for_status_raises(lpxlib):
    from linear_programming_solver_amd import LPException, SolutionException
    from linear_programming_solver_amd.errors import exception_for_status, raise_for_status
    assert exception_for_status(lpxlib.OPTIMAL) is None
    for status, cls in ((lpxlib.UNBOUNDED, SolutionException), (lpxlib.INFEASIBLE, LPException),
                        (lpxlib.AUX_UNBOUNDED, SolutionException), (lpxlib.DIVIDE_BY_ZERO, ZeroDivisionError),
                        (lpxlib.PIVOT_LIMIT, RuntimeError), (lpxlib.RESTORE_INDEX_FAULT, IndexError)):
        exc = exception_for_status(status)
        assert type(exc) is cls
        with pytest.raises(cls) as ei:
            raise_for_status(status)
        assert str(ei.value) == str(exc)
    assert str(exception_for_status(lpxlib.UNBOUNDED)) == "This linear program is unbounded"


def test_pack_lps_puts_heterogeneous_shapes_at_the_documented_offsets():
    from linear_programming_solver_amd import pack_lps
    rng = np.random.default_rng(3)
    shapes = [(2, 3), (4, 1), (0, 3), (3, 0), (1, 5)]
    lps = []
    for k, (m, n) in enumerate(shapes):
        lp = (rng.random((m, n)) + 1.0, rng.random(m) + 1.0, rng.random(n) + 1.0)
        lps.append(lp + (float(k),) if k % 2 else lp)
    p = pack_lps(lps)
    assert (p["count"], p["m_max"], p["n_max"], p["lda"], p["strideA"]) == (5, 4, 5, 5, 20)
    assert p["m"].dtype == np.int32 and p["m"].tolist() == [2, 4, 0, 3, 1] and p["n"].tolist() == [3, 1, 3, 0, 5]
    flatA, flatb, flatc = p["A"].reshape(-1), p["b"].reshape(-1), p["c"].reshape(-1)
    assert p["A"].flags.c_contiguous and p["b"].flags.c_contiguous and p["c"].flags.c_contiguous
    used = np.zeros(flatA.size, dtype=bool)
    for k, (m, n) in enumerate(shapes):
        A, b, c = lps[k][:3]
        for i in range(m):
            for j in range(n):
                assert flatA[k * p["strideA"] + i * p["lda"] + j] == A[i, j]       # A + k*strideA, row-major, lda
                used[k * p["strideA"] + i * p["lda"] + j] = True
        assert np.array_equal(flatb[k * p["m_max"]: k * p["m_max"] + m], b)        # b + k*m_max
        assert np.array_equal(flatc[k * p["n_max"]: k * p["n_max"] + n], c)        # c + k*n_max
        assert not flatb[k * p["m_max"] + m: (k + 1) * p["m_max"]].any()
        assert not flatc[k * p["n_max"] + n: (k + 1) * p["n_max"]].any()
        assert p["v"][k] == (float(k) if k % 2 else 0.0)
    assert not flatA[~used].any()
    empty = pack_lps([])
    assert (empty["count"], empty["m_max"], empty["n_max"], empty["lda"]) == (0, 0, 0, 1)
    with pytest.raises(ValueError):
        pack_lps([(np.ones((2, 2)), np.ones(3), np.ones(2))])
