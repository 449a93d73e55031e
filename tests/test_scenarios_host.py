"""Host-only side of the scenario batches (include/lpx.h: lpx_scenarios_*, lpx_solve_scenarios; LPScenarios): the argument
checks that come before any device call -- so they answer LPX_BAD_ARGUMENT on a machine without a GPU too, never
LPX_DEVICE_ERROR -- the shape checks of the Python class, and the proof, from the CPU oracle, that the inputs of
tests/test_gpu_scenarios.py hold what that file says they hold."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import scenario_cases as sc

OPTIMAL, UNBOUNDED, INFEASIBLE = 0, 1, 2


@pytest.fixture(scope="module")
def lpxlib():
    import __graft_entry__ as g
    from linear_programming_solver_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    _lib.lib()
    return _lib


def dp(lpxlib, a):
    return None if a is None else a.ctypes.data_as(lpxlib.dp)


def one_shot(lpxlib, m, n, A, lda, count, b, ldb, c, ldc, results="own", opts=None, maximize=None):
    res = (lpxlib.SolveResult * max(count, 1))() if results == "own" else results
    return lpxlib.lib().lpx_solve_scenarios(m, n, dp(lpxlib, A), lda, count, dp(lpxlib, b), ldb, dp(lpxlib, c), ldc,
                                            None if maximize is None else maximize.ctypes.data_as(lpxlib.ip),
                                            None if opts is None else C.byref(opts), res, None, None)


def create(lpxlib, m, n, A, lda, device=0):
    h = C.c_void_p()
    rc = lpxlib.lib().lpx_scenarios_create(m, n, dp(lpxlib, A), lda, device, C.byref(h))
    assert rc != 0 or h.value
    if rc == 0:
        lpxlib.lib().lpx_scenarios_destroy(h)
    return rc


def bad(lpxlib, rc, *words):
    msg = lpxlib.last_error()
    assert rc == lpxlib.BAD_ARGUMENT, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_create_refuses_bad_arguments_before_any_device_call(lpxlib):
    A = np.ones((3, 4))
    who = "lpx_scenarios_create"
    bad(lpxlib, create(lpxlib, -1, 4, A, 4), who, "negative")
    bad(lpxlib, create(lpxlib, 3, -4, A, 4), who, "negative")
    bad(lpxlib, create(lpxlib, 3, 4, A, 3), who, "lda < n")
    bad(lpxlib, create(lpxlib, 3, 4, None, 4), who, "NULL", "A")
    bad(lpxlib, create(lpxlib, 3, 4, A, 4, device=-1), who, "device")
    bad(lpxlib, create(lpxlib, 99, 200, np.ones((99, 200)), 200), who, "99 x 200", "LDS")    # one row past the LDS
    assert lpxlib.lib().lpx_scenarios_create(3, 4, dp(lpxlib, A), 4, 0, None) == lpxlib.BAD_ARGUMENT


def test_one_shot_refuses_bad_arguments_before_any_device_call(lpxlib):
    A, b, c = np.ones((3, 4)), -np.ones((2, 3)), np.ones((2, 4))
    who = "lpx_solve_scenarios"
    bad(lpxlib, one_shot(lpxlib, 3, 4, A, 4, -1, b, 3, c, 4), who, "negative count")
    bad(lpxlib, one_shot(lpxlib, -3, 4, A, 4, 2, b, 3, c, 4), who, "negative")
    bad(lpxlib, one_shot(lpxlib, 3, -4, A, 4, 2, b, 3, c, 4), who, "negative")
    bad(lpxlib, one_shot(lpxlib, 3, 4, A, 3, 2, b, 3, c, 4), who, "lda < n")
    for ldb in (1, 2):
        bad(lpxlib, one_shot(lpxlib, 3, 4, A, 4, 2, b, ldb, c, 4), who, "ldb")
    for ldc in (1, 3):
        bad(lpxlib, one_shot(lpxlib, 3, 4, A, 4, 2, b, 3, c, ldc), who, "ldc")
    bad(lpxlib, one_shot(lpxlib, 3, 4, A, 4, 2, b, 3, c, 4, results=None), who, "results")
    bad(lpxlib, one_shot(lpxlib, 3, 4, None, 4, 2, b, 3, c, 4), who, "NULL", "A")
    bad(lpxlib, one_shot(lpxlib, 3, 4, A, 4, 2, None, 3, c, 4), who, "NULL", "b or c")
    bad(lpxlib, one_shot(lpxlib, 3, 4, A, 4, 2, b, 3, None, 4), who, "NULL", "b or c")
    bad(lpxlib, one_shot(lpxlib, 3, 4, A, 4, 2, None, 0, c, 4), who, "NULL", "b or c")       # a shared vector is data too
    # the LDS limits: 98 x 200 fits, but not with phase 1 -- scenario 1 of 2 has a negative b; 99 x 200 does not fit at all
    big_A, big_b, big_c = np.ones((98, 200)), np.ones((2, 98)), np.ones(200)
    big_b[1, 7] = -1.0
    bad(lpxlib, one_shot(lpxlib, 98, 200, big_A, 200, 2, big_b, 98, big_c, 0), who, "scenario 1", "98 x 200", "phase 1")
    bad(lpxlib, one_shot(lpxlib, 99, 200, np.ones((99, 200)), 200, 1, np.ones((1, 99)), 99, big_c, 0), who, "99 x 200", "LDS")
    # a restore order that names variable n
    order = np.array([0, 1, 2, 4], dtype=np.int32)
    opts = lpxlib.SolveOptions()
    opts.max_pivots = -1
    opts.restore_order = order.ctypes.data_as(lpxlib.ip)
    opts.restore_order_len = 4
    bad(lpxlib, one_shot(lpxlib, 3, 4, A, 4, 2, b, 3, c, 4, opts=opts), who, "variable 4")
    opts.restore_order_len = 5                                                               # more entries than variables
    bad(lpxlib, one_shot(lpxlib, 3, 4, A, 4, 2, b, 3, c, 4, opts=opts), who, "5 entries")
    # what a scenario batch cannot honour
    x = np.zeros(4)
    opts = lpxlib.SolveOptions()
    opts.max_pivots = -1
    opts.x_out = x.ctypes.data_as(lpxlib.dp)
    bad(lpxlib, one_shot(lpxlib, 3, 4, A, 4, 2, b, 3, c, 4, opts=opts), who, "x_out")
    opts = lpxlib.SolveOptions()
    opts.max_pivots = -1
    opts.pricing = 2
    bad(lpxlib, one_shot(lpxlib, 3, 4, A, 4, 2, b, 3, c, 4, opts=opts), who, "pricing")


def test_null_handles(lpxlib):
    L = lpxlib.lib()
    res = (lpxlib.SolveResult * 1)()
    b, c = np.ones(3), np.ones(4)
    bad(lpxlib, L.lpx_scenarios_solve(None, 1, dp(lpxlib, b), 0, dp(lpxlib, c), 0, None, -1, None, -1, res, None, None),
        "lpx_scenarios_solve", "NULL handle")
    bad(lpxlib, L.lpx_scenarios_set_option(None, 18, 1), "lpx_scenarios_set_option", "NULL handle")
    bad(lpxlib, L.lpx_scenarios_set_pricing(None, 0), "lpx_scenarios_set_pricing")
    L.lpx_scenarios_destroy(None)


def test_a_valid_call_without_a_gpu_is_a_device_error(lpxlib):
    if lpxlib.lib().lpx_device_count() > 0:
        pytest.skip("a GPU is visible")
    A, b, c = np.ones((3, 4)), np.ones((2, 3)), np.ones(4)
    assert create(lpxlib, 3, 4, A, 4) == lpxlib.DEVICE_ERROR
    assert one_shot(lpxlib, 3, 4, A, 4, 2, b, 3, c, 0) == lpxlib.DEVICE_ERROR
    from linear_programming_solver_amd import LPScenarios
    with pytest.raises(RuntimeError):
        LPScenarios(A)


def test_an_empty_call_needs_no_device(lpxlib):
    A = np.ones((3, 4))
    assert one_shot(lpxlib, 3, 4, A, 4, 0, None, 0, None, 0, results=None) == 0


def test_scenario_arrays_checks_shapes_without_a_library_call():
    from linear_programming_solver_amd.lp_scenarios import scenario_arrays
    m, n = 3, 4
    assert scenario_arrays(m, n, np.ones(3), np.ones(4))[::2] == (1, 0, 0)
    assert scenario_arrays(m, n, np.ones((5, 3)), np.ones(4))[::2] == (5, 3, 0)
    assert scenario_arrays(m, n, np.ones(3), np.ones((5, 4)))[::2] == (5, 0, 4)
    assert scenario_arrays(m, n, np.ones((5, 3)), np.ones((5, 4)))[::2] == (5, 3, 4)
    with pytest.raises(ValueError):
        scenario_arrays(m, n, np.ones((5, 3)), np.ones((6, 4)))       # counts differ
    with pytest.raises(ValueError):
        scenario_arrays(m, n, np.ones((5, 4)), np.ones((5, 4)))       # b's trailing dimension
    with pytest.raises(ValueError):
        scenario_arrays(m, n, np.ones(3), np.ones(3))                 # c's trailing dimension
    with pytest.raises(ValueError):
        scenario_arrays(m, n, np.ones((2, 5, 3)), np.ones(4))


def test_solve_raises_on_bad_shapes_without_a_library_call():
    """LPScenarios.solve on an object that has no handle and no library: the ValueError comes first."""
    from linear_programming_solver_amd import LPScenarios
    s = LPScenarios.__new__(LPScenarios)
    s.m, s.n, s._h, s._L = 3, 4, None, None
    with pytest.raises(ValueError):
        s.solve(np.ones((5, 3)), np.ones((6, 4)))
    with pytest.raises(ValueError):
        s.solve(np.ones((5, 2)), np.ones((5, 4)))
    with pytest.raises(ValueError):
        s.solve(np.ones(3), np.ones(5))
    with pytest.raises(ValueError):
        s.solve(np.ones((5, 3)), np.ones(4), maximize=[True] * 4)
    with pytest.raises(ValueError):
        s.solve(np.ones((5, 3)), np.ones(4), restore_order=[0, 1, 2, 3, 0])


# ---------------------------------------------------------------------------------------------------- the claims
@pytest.fixture(scope="module")
def verdicts(oracle):
    """{(launch name, kind, pricing): [result dict per scenario]}: every launch of the GPU tests through both binary
    instantiations of the oracle and both entering rules."""
    out = {}
    for name, L in sc.launches():
        for kind in (oracle.FP64, oracle.FP64_FUSED):
            for pricing in (0, 1):
                rs = []
                for k in range(len(L["b"])):
                    r, st = oracle.solve(L["A"], L["b"][k], L["c"][k], L["maximize"][k], kind=kind, want_trace=False,
                                         pricing=pricing)
                    r["final_n"] = st.n
                    st.close()
                    rs.append(r)
                out[(name, kind, pricing)] = rs
    return out


def test_the_gpu_inputs_hold_what_they_claim(verdicts):
    names = [name for name, _ in sc.launches()]
    assert len(names) == len(sc.SHAPES) + 6 and len(set(names)) == len(names)
    for (name, kind, pricing), rs in verdicts.items():
        what = (name, kind, pricing)
        L = dict(sc.launches())[name]
        m, n = L["A"].shape
        assert (3 if name.startswith("big") else 8) <= len(rs) <= 16, what
        assert all(bool(r["phase1_used"]) == bool(L["b"][k].min() < 0) for k, r in enumerate(rs)), what
        if name.startswith("mixed") and m >= 2:
            assert any(r["phase1_used"] and r["status"] == OPTIMAL and r["pivots2"] >= 1 for r in rs), what
            assert any(not r["phase1_used"] for r in rs), what
            assert any(r["status"] == INFEASIBLE and r["final_n"] == n + 1 for r in rs), what
        if name.startswith("column"):
            assert any(r["status"] == UNBOUNDED for r in rs) and any(r["status"] == OPTIMAL for r in rs), what
            assert all((r["status"] == UNBOUNDED) == (L["c"][k][n // 2] > 0) for k, r in enumerate(rs)), what
        if name.startswith("signed"):
            assert any(not L["maximize"][k] and r["pivots1"] + r["pivots2"] > 0 for k, r in enumerate(rs)), what
            assert any(not L["maximize"][k] and r["phase1_used"] for k, r in enumerate(rs)), what
            assert any(L["maximize"][k] for k in range(len(rs))), what
        if name.startswith("big"):
            assert any(r["phase1_used"] and r["status"] == OPTIMAL and r["pivots2"] >= 1 for r in rs), what


def test_the_big_launch_needs_more_than_64_kib_of_lds(lpxlib):
    m, n = sc.BIG_SHAPE
    L = lpxlib.lib()
    assert 65536 < L.lpx_batch_solve_lds_bytes(m, n) <= lpxlib.BATCH_LDS_BYTES < L.lpx_batch_solve_lds_bytes(m + 1, n)
