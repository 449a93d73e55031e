"""Host-only side of the re-solve from a shared basis (include/lpx.h: lpx_scenarios_set_basis, lpx_scenarios_resolve,
lpx_solve_scenarios_from_basis): the proof, from the CPU oracle, that the inputs of tests/test_gpu_resolve.py
(tests/resolve_cases.py) hold what that file says they hold; the model of tests/resolve_cases.py against SciPy's HiGHS on
every warm-routed scenario; and the argument checks that come before any device call."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import resolve_cases as rc

BUDGET_SHAPE, BUDGET = rc.BUDGET_SHAPE, rc.BUDGET


@pytest.fixture(scope="module")
def lpxlib():
    import __graft_entry__ as g
    from linear_programming_solver_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    _lib.lib()
    return _lib


@pytest.fixture(scope="module", params=["plain", "fused"])
def moded(request, oracle):
    from tests.conftest import ArithOracle
    return ArithOracle(oracle, request.param)


@pytest.fixture(scope="module")
def modelled(moded):
    """[(name, case, basis, model per scenario)] of every case, in one arithmetic mode."""
    out = []
    for name, case in rc.cases():
        basis = rc.base_basis(moded, case)
        out.append((name, case, basis, rc.model_case(moded, case, basis)))
    return out


# ---------------------------------------------------------------------------------------------------- 1. the claims
def test_the_gpu_inputs_hold_what_they_claim(modelled):
    names = [name for name, _, _, _ in modelled]
    assert len(names) == len(rc.SHAPES) + 2 and len(set(names)) == len(names)
    routes, dual_verdicts, primal_verdicts = set(), set(), set()
    for name, case, basis, want in modelled:
        m, n = case["A"].shape
        assert len(basis) == m and len(set(basis)) == m, name
        assert len(want) == (4 if name.startswith("column") else rc.count_of(m, n)), name
        for k, w in enumerate(want):
            routes.add(w["route"])
            if w["route"] == "dual":
                dual_verdicts.add(w["status"])
                assert w["b_basis"].min() < 0, (name, k)
            if w["route"] == "primal":
                primal_verdicts.add(w["status"])
                assert w["pivots1"] == 0 and not w["b_basis"].min() < 0, (name, k)
        if name.startswith("column"):
            assert all(w["route"] == "primal" and w["status"] == rc.UNBOUNDED and w["pivots2"] >= 1 for w in want), name
        elif m >= 2 and len(want) > 12:
            assert want[12]["route"] == "dual" and want[12]["status"] == rc.INFEASIBLE, name
        if (m, n) in ((1, 1), (1, 3)):   # an unbounded base: the slack basis, the empty eta file
            assert basis == list(range(n, n + m)) and want[0]["crash"] == 0, name
        if name in ("24x40", "33x130", "%dx%d" % rc.BIG_SHAPE):
            assert {w["route"] for w in want} == {"cold", "primal", "dual"}, name
            assert want[0]["crash"] >= 5, name
            assert any(w["route"] == "dual" and w["status"] == rc.OPTIMAL and w["pivots1"] >= 2 for w in want), name
    assert routes == {"cold", "primal", "dual"}
    assert {rc.OPTIMAL, rc.INFEASIBLE} <= dual_verdicts
    assert {rc.OPTIMAL, rc.UNBOUNDED} <= primal_verdicts
    assert any(not case["maximize"][k] and w["route"] != "cold" and w["pivots1"] + w["pivots2"] > 0
               for _, case, _, want in modelled for k, w in enumerate(want))


def test_the_budgeted_case_ends_inside_both_loops(moded):
    case = rc.case(*BUDGET_SHAPE)
    basis = rc.base_basis(moded, case)
    want = rc.model_case(moded, case, basis, budget=BUDGET)
    assert any(w["route"] == "dual" and w["status"] == rc.PIVOT_LIMIT and (w["pivots1"], w["pivots2"]) == (BUDGET, 0) for w in want)
    assert any(w["route"] == "primal" and w["status"] == rc.PIVOT_LIMIT and (w["pivots1"], w["pivots2"]) == (0, BUDGET) for w in want)
    assert any(w["route"] != "cold" and w["status"] == rc.OPTIMAL for w in want)


def test_the_singular_case_is_singular(moded):
    A, basis = rc.singular_case()
    st = moded.State(A, np.ones(5), np.ones(6), kind=moded.FP64)
    with pytest.raises(rc.SingularBasis) as exc:
        rc.crash(st, basis)
    st.close()
    assert exc.value.args[0] == 4
    assert abs(np.linalg.det(A[:2, [1, 4]])) < 1e-12


def test_the_big_shape_needs_more_than_64_kib_and_has_no_room_for_phase_1(lpxlib):
    m, n = rc.BIG_SHAPE
    L = lpxlib.lib()
    assert 65536 < L.lpx_batch_lds_bytes(m, n) <= lpxlib.BATCH_LDS_BYTES < L.lpx_batch_lds_bytes(m + 1, n)
    assert L.lpx_batch_solve_lds_bytes(m, n) > lpxlib.BATCH_LDS_BYTES


# ---------------------------------------------------------------------------------------------------- 2. against HiGHS
def test_the_model_agrees_with_highs_on_every_warm_scenario(modelled):
    """Same verdict, and the optimum within 1e-8 relative: the warm start changes the path, not the answer."""
    from scipy.optimize import linprog
    checked = 0
    for name, case, _, want in modelled:
        for k, w in enumerate(want):
            if w["route"] == "cold":
                continue
            sign = 1.0 if case["maximize"][k] else -1.0
            got = linprog(-sign * case["c"][k], A_ub=case["A"], b_ub=case["b"][k], bounds=(0, None), method="highs")
            what = (name, k, w["route"], w["status"], got.status, got.message)
            if w["status"] == rc.OPTIMAL:
                assert got.status == 0, what
                best = -got.fun                      # of the maximisation the solver runs
                assert abs(sign * w["objective"] - best) <= 1e-8 * max(1.0, abs(best)), what
            elif w["status"] == rc.INFEASIBLE:
                assert got.status == 2, what
            else:
                assert w["status"] == rc.UNBOUNDED and got.status in (3, 4), what   # HiGHS: unbounded, or "infeasible or unbounded"
            checked += 1
    assert checked >= 100


# ---------------------------------------------------------------------------------------------------- 3. argument checks
def dp(lpxlib, a):
    return None if a is None else a.ctypes.data_as(lpxlib.dp)


def from_basis(lpxlib, m, n, A, basis, count, b, c, results="own"):
    res = (lpxlib.SolveResult * max(count, 1))() if results == "own" else results
    bs = None if basis is None else np.asarray(basis, dtype=np.int32)
    return lpxlib.lib().lpx_solve_scenarios_from_basis(m, n, dp(lpxlib, A), n, None if bs is None else bs.ctypes.data_as(lpxlib.ip),
                                                       count, dp(lpxlib, b), m, dp(lpxlib, c), n, None, None, res, None, None,
                                                       None)


def bad(lpxlib, rc_, *words):
    msg = lpxlib.last_error()
    assert rc_ == lpxlib.BAD_ARGUMENT, (rc_, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_the_one_shot_refuses_bad_arguments_before_any_device_call(lpxlib):
    A, b, c = np.ones((3, 4)), np.ones((2, 3)), np.ones((2, 4))
    who = "lpx_solve_scenarios_from_basis"
    bad(lpxlib, from_basis(lpxlib, 3, 4, A, [0, 1, 7], 2, b, c), who, "entry 2", "variable id 7")      # ids end at n + m - 1 = 6
    bad(lpxlib, from_basis(lpxlib, 3, 4, A, [0, -1, 2], 2, b, c), who, "entry 1", "variable id -1")
    bad(lpxlib, from_basis(lpxlib, 3, 4, A, [5, 1, 5], 2, b, c), who, "entry 2", "repeats", "variable id 5")
    bad(lpxlib, from_basis(lpxlib, 3, 4, A, [4, 5, 6], 2, b, c, results=None), who, "results")
    bad(lpxlib, from_basis(lpxlib, 3, 4, A, None, 2, b, c), who, "basis is NULL")
    bad(lpxlib, from_basis(lpxlib, 3, 4, None, [4, 5, 6], 2, b, c), who, "NULL", "A")
    bad(lpxlib, from_basis(lpxlib, 3, 4, A, [4, 5, 6], -1, b, c), who, "negative count")
    bad(lpxlib, from_basis(lpxlib, 3, 4, A, [4, 5, 6], 2, None, c), who, "NULL", "b or c")


def test_null_handles(lpxlib):
    L = lpxlib.lib()
    res = (lpxlib.SolveResult * 1)()
    b, c = np.ones(3), np.ones(4)
    took = C.c_int32(5)
    bad(lpxlib, L.lpx_scenarios_set_basis(None, None, C.byref(took)), "lpx_scenarios_set_basis", "NULL handle")
    assert took.value == 0
    bad(lpxlib, L.lpx_scenarios_resolve(None, 1, dp(lpxlib, b), 0, dp(lpxlib, c), 0, None, -1, None, -1, res, None, None, None),
        "lpx_scenarios_resolve", "NULL handle")


def test_a_valid_one_shot_without_a_gpu_is_a_device_error(lpxlib):
    if lpxlib.lib().lpx_device_count() > 0:
        return   # a GPU is visible: tests/test_gpu_resolve.py covers the call
    A, b, c = np.ones((3, 4)), np.ones((2, 3)), np.ones((2, 4))
    assert from_basis(lpxlib, 3, 4, A, [4, 5, 6], 2, b, c) == lpxlib.DEVICE_ERROR


def test_set_basis_checks_its_length_without_a_library_call():
    from linear_programming_solver_amd import LPScenarios
    s = LPScenarios.__new__(LPScenarios)
    s.m, s.n, s._h, s._L = 3, 4, None, None
    with pytest.raises(ValueError):
        s.set_basis([4, 5])
    with pytest.raises(ValueError):
        s.resolve(np.ones((5, 3)), np.ones((6, 4)))
