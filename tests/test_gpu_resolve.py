"""GPU parity of the re-solve from a shared basis (k_scenarios_crash and k_batch_resolve through lpx_scenarios_set_basis /
lpx_scenarios_resolve / LPScenarios, lpx_solve_scenarios_from_basis and LPSolver.solve_scenarios(basis=...)) against the
CPU model of tests/resolve_cases.py, which is made of oracle calls only.

The bar, for EVERY scenario and in both arithmetic modes: the route, the status, both pivot counts, the objective bit for
bit and its text, perm, and x bit for bit; phase1_used = 0 and x0_slot = -1 on the warm routes.  A scenario routed cold is
compared byte for byte with what lpx_scenarios_solve returns for it on the same handle (and its verdict with the oracle's).

Every test runs the model first, on the CPU, and gives the GPU a FINITE budget of twice the model's largest pivot count
plus 100: a divergence ends as a mismatch, not as a long loop.  tests/test_resolve_host.py proves on the CPU that the
inputs hold the routes and verdicts these tests are about."""
import ctypes as C
from decimal import Decimal

import numpy as np
import pytest

from tests import resolve_cases as rc

pytestmark = pytest.mark.gpu

SENTINEL_X, SENTINEL_PERM = -7.0, -1
BUDGET_SHAPE, BUDGET = rc.BUDGET_SHAPE, rc.BUDGET
ROUTES = ("cold", "primal", "dual")


@pytest.fixture(scope="module")
def lps(arith):
    from tests.conftest import package_in_mode
    pkg = package_in_mode(arith)
    yield pkg
    pkg.set_default_arithmetic("auto")


@pytest.fixture(scope="module")
def oracle(arith):
    from oracle import pyoracle
    from tests.conftest import ArithOracle
    pyoracle.build()
    pyoracle.lib()
    return ArithOracle(pyoracle, arith)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_WANT = {}


def modelled(oracle, name, case, pricing="reference", budget=-1):
    """(basis, model per scenario) of a named case: computed once per (name, mode, pricing, budget) and shared."""
    key = (name, oracle.mode, pricing, budget)
    if key not in _WANT:
        basis = rc.base_basis(oracle, case, pricing)
        _WANT[key] = (basis, rc.model_case(oracle, case, basis, budget, pricing))
    return _WANT[key]


def raw(handle, fn_name, case, budget, rows=None, shared=(), pass_x=True, pass_perm=True):
    """lpx_scenarios_solve / lpx_scenarios_resolve through ctypes on the LPScenarios `handle` for the scenarios `rows` of
    `case` (None: all); a name in `shared` passes that vector of the first row at pitch 0.  Returns (results, x, perm,
    route) with x and perm pre-filled with the sentinels (route: None for lpx_scenarios_solve); an array that is not
    passed (x_out / perm_out NULL) comes back as filled."""
    from linear_programming_solver_amd import _lib
    m, n = handle.m, handle.n
    rows = list(range(len(case["maximize"]))) if rows is None else list(rows)
    count = len(rows)
    b = np.ascontiguousarray(case["b"][rows[0]] if "b" in shared else case["b"][rows], dtype=np.float64)
    c = np.ascontiguousarray(case["c"][rows[0]] if "c" in shared else case["c"][rows], dtype=np.float64)
    mx = np.array([1 if case["maximize"][k] else 0 for k in rows], dtype=np.int32)
    res = (_lib.SolveResult * count)()
    x = np.full((count, n), SENTINEL_X)
    perm = np.full((count, n + m), SENTINEL_PERM, dtype=np.int32)
    args = [handle._h, count, b.ctypes.data_as(_lib.dp), m if b.ndim == 2 else 0, c.ctypes.data_as(_lib.dp),
            n if c.ndim == 2 else 0, mx.ctypes.data_as(_lib.ip), budget, None, -1, res,
            x.ctypes.data_as(_lib.dp) if pass_x else None, perm.ctypes.data_as(_lib.ip) if pass_perm else None]
    route = None
    if fn_name == "lpx_scenarios_resolve":
        route = np.full(count, -9, dtype=np.int32)
        args.append(route.ctypes.data_as(_lib.ip))
    rc_ = getattr(handle._L, fn_name)(*args)
    assert rc_ == 0, _lib.last_error()
    return res, x, perm, route


def result_bytes(r):
    """One result with the times blanked."""
    keep = (r.seconds_total, r.seconds_pivots)
    r.seconds_total = r.seconds_pivots = 0.0
    out = bytes(r)
    r.seconds_total, r.seconds_pivots = keep
    return out


def compare_warm(res, x_row, perm_row, route, w, what):
    assert ROUTES[route] == w["route"], "route differs %s: %s vs %s" % (what, ROUTES[route], w["route"])
    assert res.status == w["status"], "status differs %s: %d vs %d" % (what, res.status, w["status"])
    assert (res.pivots_phase1, res.pivots_phase2) == (w["pivots1"], w["pivots2"]), \
        "pivot counts differ %s: %r vs %r" % (what, (res.pivots_phase1, res.pivots_phase2), (w["pivots1"], w["pivots2"]))
    assert res.phase1_used == 0 and res.x0_slot == -1, "phase 1 fields " + what
    assert bits(np.array([res.objective]))[0] == bits(np.array([w["objective"]]))[0], "objective bits differ " + what
    assert res.objective_text.decode() == w["objective_text"], "objective text differs " + what
    assert list(perm_row) == list(w["perm"]), "perm differs " + what
    assert np.array_equal(bits(x_row), bits(w["x"])), "x differs " + what


def compare_all(got, cold_ref, want, what, rows=None):
    """`got` of lpx_scenarios_resolve against the model `want`; the cold scenarios against `cold_ref`, the answer of
    lpx_scenarios_solve for the same scenarios on the same handle, and their verdict against the oracle."""
    res, x, perm, route = got
    rows = list(range(len(want))) if rows is None else list(rows)
    assert len(rows) == len(route)
    for t, k in enumerate(rows):
        w = want[k]
        where = "(%s, scenario %d)" % (what, k)
        if w["route"] != "cold":
            compare_warm(res[t], x[t], perm[t], route[t], w, where)
            continue
        assert route[t] == 0, "route differs %s: %s vs cold" % (where, ROUTES[route[t]])
        assert result_bytes(res[t]) == result_bytes(cold_ref[0][t]), "cold result differs " + where
        assert x[t].tobytes() == cold_ref[1][t].tobytes() and perm[t].tobytes() == cold_ref[2][t].tobytes(), "cold rows differ " + where
        cold = w["cold"]
        assert (res[t].status, res[t].pivots_phase1, res[t].pivots_phase2) == (cold["status"], cold["pivots1"], cold["pivots2"]), where
        assert bits(np.array([res[t].objective]))[0] == bits(np.array([cold["objective"]]))[0], where


# ------------------------------------------------------------------------------------ 1. every case against the model
@pytest.mark.parametrize("pricing", ["reference", "dantzig"])
def test_every_case_matches_the_model(lps, oracle, pricing):
    """All shapes, all three routes, OPTIMAL and INFEASIBLE out of the dual loop, UNBOUNDED on the primal route, `min`
    scenarios, the empty eta file and the 98 x 200 case with more than 64 KiB of dynamic LDS.  set_basis returns the
    model's crash pivots, and lpx_scenarios_solve on a handle with a basis returns the bytes it returned without one."""
    seen = set()
    for name, case in rc.cases():
        basis, want = modelled(oracle, name, case, pricing)
        budget = rc.budget_above(want)
        handle = lps.LPScenarios(case["A"], pricing=pricing)
        try:
            before = raw(handle, "lpx_scenarios_solve", case, budget)
            assert handle.set_basis(basis) == want[0]["crash"], name
            got = raw(handle, "lpx_scenarios_resolve", case, budget)
            after = raw(handle, "lpx_scenarios_solve", case, budget)
        finally:
            handle.close()
        compare_all(got, before, want, "%s, %s" % (name, pricing))
        assert [result_bytes(r) for r in before[0]] == [result_bytes(r) for r in after[0]], name
        assert before[1].tobytes() == after[1].tobytes() and before[2].tobytes() == after[2].tobytes(), name
        seen |= {(w["route"], w.get("status")) for w in want}
    assert {("cold", None), ("primal", rc.OPTIMAL), ("primal", rc.UNBOUNDED), ("dual", rc.OPTIMAL), ("dual", rc.INFEASIBLE)} <= seen


# ------------------------------------------------------------------------------------ 2. budgets
def test_a_budget_ends_inside_the_dual_loop_and_inside_the_primal_loop(lps, oracle):
    name = "%dx%d" % BUDGET_SHAPE
    case = rc.case(*BUDGET_SHAPE)
    basis, want = modelled(oracle, name, case, budget=BUDGET)
    assert any(w["route"] == "dual" and w["status"] == rc.PIVOT_LIMIT for w in want)
    assert any(w["route"] == "primal" and w["status"] == rc.PIVOT_LIMIT for w in want)
    handle = lps.LPScenarios(case["A"])
    try:
        handle.set_basis(basis)
        got = raw(handle, "lpx_scenarios_resolve", case, BUDGET)
        cold = raw(handle, "lpx_scenarios_solve", case, BUDGET)
    finally:
        handle.close()
    compare_all(got, cold, want, name + ", budget %d" % BUDGET)


@pytest.mark.parametrize("shape", [(24, 40), (65, 5), rc.BIG_SHAPE])
def test_the_replay_alone_gives_b_at_the_basis(lps, oracle, shape):
    """max_pivots = 0: no pivot but the crash's replay.  x is the model's b at the basis on the basic rows, bit for bit."""
    name = "%dx%d" % shape
    case = rc.case(*shape)
    basis, want = modelled(oracle, name, case, budget=0)
    warm = [k for k, w in enumerate(want) if w["route"] != "cold"]
    assert len(warm) >= 3 and want[0]["crash"] >= 3
    handle = lps.LPScenarios(case["A"])
    try:
        handle.set_basis(basis)
        res, x, perm, route = raw(handle, "lpx_scenarios_resolve", case, 0, rows=warm)
    finally:
        handle.close()
    n = shape[1]
    for t, k in enumerate(warm):
        w = want[k]
        compare_warm(res[t], x[t], perm[t], route[t], w, "(%s, replay, scenario %d)" % (name, k))
        assert (res[t].pivots_phase1, res[t].pivots_phase2) == (0, 0)
        expect = np.zeros(n)
        for i, var in enumerate(perm[t][n:]):
            if var < n:
                expect[var] = w["b_basis"][i]
        assert np.array_equal(bits(x[t]), bits(expect)), (name, k)


# ------------------------------------------------------------------------------------ 3. set_basis
def test_a_singular_basis_is_refused_and_clears_the_basis(lps, oracle):
    from linear_programming_solver_amd import _lib
    A, singular = rc.singular_case()
    m, n = A.shape
    case = {"A": A, "b": np.ones((2, m)), "c": np.ones((2, n)), "maximize": [True, True]}
    slack = list(range(n, n + m))
    good = [1] + slack[1:]
    handle = lps.LPScenarios(A)
    try:
        res = (_lib.SolveResult * 2)()

        def resolve_rc():
            return handle._L.lpx_scenarios_resolve(handle._h, 2, case["b"].ctypes.data_as(_lib.dp), m, case["c"].ctypes.data_as(_lib.dp),
                                                   n, None, 1000, None, -1, res, None, None, None)

        assert resolve_rc() == _lib.BAD_ARGUMENT and "no basis" in _lib.last_error()          # a fresh handle has none
        assert handle.set_basis(good) == 1
        assert resolve_rc() == 0, _lib.last_error()
        took = C.c_int32(-1)
        ids = np.asarray(singular, dtype=np.int32)
        assert handle._L.lpx_scenarios_set_basis(handle._h, ids.ctypes.data_as(_lib.ip), C.byref(took)) == _lib.BAD_ARGUMENT
        assert "basis is singular at variable id 4" in _lib.last_error()
        assert resolve_rc() == _lib.BAD_ARGUMENT and "no basis" in _lib.last_error()          # the earlier basis is gone too
        with pytest.raises(Exception):
            handle.set_basis(singular)
        assert handle.set_basis(slack) == 0                                                   # the empty eta file
        assert resolve_rc() == 0, _lib.last_error()
        assert handle.set_basis(None) == 0                                                    # NULL clears
        assert resolve_rc() == _lib.BAD_ARGUMENT and "no basis" in _lib.last_error()
        ids = np.asarray([1, 1] + slack[2:], dtype=np.int32)                                  # the host checks still come first
        assert handle._L.lpx_scenarios_set_basis(handle._h, ids.ctypes.data_as(_lib.ip), None) == _lib.BAD_ARGUMENT
        assert "repeats" in _lib.last_error()
    finally:
        handle.close()


def test_a_second_basis_replaces_the_first(lps, oracle):
    """The slack basis first (everything cold or primal from the start), then the base case's: the answers are those of
    the basis in force."""
    case = rc.case(24, 40)
    m, n = 24, 40
    basis, want = modelled(oracle, "24x40", case)
    slack = list(range(n, n + m))
    want_slack = rc.model_case(oracle, case, slack)
    assert all(w["route"] == "primal" and w["crash"] == 0 for w in want_slack[:12])
    handle = lps.LPScenarios(case["A"])
    try:
        for ids, w in ((slack, want_slack), (basis, want), (slack, want_slack)):
            handle.set_basis(ids)
            budget = rc.budget_above(w)
            compare_all(raw(handle, "lpx_scenarios_resolve", case, budget), raw(handle, "lpx_scenarios_solve", case, budget), w,
                        "24x40 after %d crash pivots" % w[0]["crash"])
    finally:
        handle.close()


# ------------------------------------------------------------------------------------ 4. other calls
def test_one_handle_resolved_twice(lps, oracle):
    """16 scenarios, then 5 others (smaller count, other rows) through LPScenarios.resolve, then the 16 again: every
    answer is the model's, whatever the call before left in the buffers."""
    case = rc.case(24, 40)
    basis, want = modelled(oracle, "24x40", case)
    second = [14, 3, 10, 12, 1]                       # cold, dual, cold, infeasible, primal
    assert {want[k]["route"] for k in second} == {"cold", "primal", "dual"}
    budget = rc.budget_above(want)
    handle = lps.LPScenarios(case["A"])
    try:
        assert handle.set_basis(basis) == want[0]["crash"]
        for rows in (range(16), second, range(16)):
            rows = list(rows)
            infos = handle.resolve(case["b"][rows], case["c"][rows], maximize=[case["maximize"][k] for k in rows], max_pivots=budget)
            plain = handle.solve(case["b"][rows], case["c"][rows], maximize=[case["maximize"][k] for k in rows], max_pivots=budget)
            assert len(infos) == len(rows)
            for t, k in enumerate(rows):
                w, info = want[k], infos[t]
                assert info.route == w["route"], (k, info.route)
                if w["route"] == "cold":
                    ref = plain[t]
                    assert (info.status, info.phase1_used, info.pivots_phase1, info.pivots_phase2, info.x0_slot) == \
                        (ref.status, ref.phase1_used, ref.pivots_phase1, ref.pivots_phase2, ref.x0_slot), k
                    assert bits(np.array([info.objective]))[0] == bits(np.array([ref.objective]))[0], k
                    assert list(info.perm) == list(ref.perm) and np.array_equal(bits(info.x), bits(ref.x)), k
                else:
                    assert (info.status, info.phase1_used, info.pivots_phase1, info.pivots_phase2, info.x0_slot) == \
                        (w["status"], False, w["pivots1"], w["pivots2"], -1), k
                    assert info.objective_text == w["objective_text"], k
                    assert bits(np.array([info.objective]))[0] == bits(np.array([w["objective"]]))[0], k
                    assert list(info.perm) == list(w["perm"]) and np.array_equal(bits(info.x), bits(w["x"])), k
    finally:
        handle.close()


def test_a_shared_b_or_c_is_the_replicated_one(lps, oracle):
    """ldb = 0 with varying c (rows 1, 5, 9, 13 share the base b), and ldc = 0 with varying b (rows 0, 3, 4, 7, 8 share the
    base c): each against the model of the full rows, and the cold ones against lpx_scenarios_solve called the same way."""
    case = rc.case(24, 40)
    basis, want = modelled(oracle, "24x40", case)
    budget = rc.budget_above(want)
    handle = lps.LPScenarios(case["A"])
    try:
        handle.set_basis(basis)
        for shared, rows in (("b", [1, 5, 9, 13]), ("c", [0, 3, 4, 7, 8])):
            for k in rows:
                assert np.array_equal(case[shared][k], case[shared][rows[0]])
            got = raw(handle, "lpx_scenarios_resolve", case, budget, rows=rows, shared=(shared,))
            cold = raw(handle, "lpx_scenarios_solve", case, budget, rows=rows, shared=(shared,))
            compare_all(got, cold, want, "24x40 shared " + shared, rows=rows)
    finally:
        handle.close()


@pytest.mark.parametrize("shape", [(24, 40), (5, 65)])
def test_the_one_shot_equals_handle_set_basis_resolve(lps, oracle, shape):
    from linear_programming_solver_amd import _lib
    m, n = shape
    name = "%dx%d" % shape
    case = rc.case(m, n)
    basis, want = modelled(oracle, name, case)
    budget = rc.budget_above(want)
    count = len(want)
    handle = lps.LPScenarios(case["A"])
    try:
        handle.set_basis(basis)
        via_handle = raw(handle, "lpx_scenarios_resolve", case, budget)
        cold = raw(handle, "lpx_scenarios_solve", case, budget)
    finally:
        handle.close()
    opts = lps.LPSolver(max_pivots=budget)._solve_options()
    opts.restore_order_len = -1
    A = np.ascontiguousarray(case["A"])
    ids = np.asarray(basis, dtype=np.int32)
    mx = np.array([1 if f else 0 for f in case["maximize"]], dtype=np.int32)
    res = (_lib.SolveResult * count)()
    x = np.full((count, n), SENTINEL_X)
    perm = np.full((count, n + m), SENTINEL_PERM, dtype=np.int32)
    route = np.full(count, -9, dtype=np.int32)
    rc_ = _lib.lib().lpx_solve_scenarios_from_basis(m, n, A.ctypes.data_as(_lib.dp), n, ids.ctypes.data_as(_lib.ip), count,
                                                    case["b"].ctypes.data_as(_lib.dp), m, case["c"].ctypes.data_as(_lib.dp), n,
                                                    mx.ctypes.data_as(_lib.ip), C.byref(opts), res, x.ctypes.data_as(_lib.dp),
                                                    perm.ctypes.data_as(_lib.ip), route.ctypes.data_as(_lib.ip))
    assert rc_ == 0, _lib.last_error()
    compare_all((res, x, perm, route), cold, want, name + " one shot")
    assert [result_bytes(r) for r in res] == [result_bytes(r) for r in via_handle[0]]
    assert x.tobytes() == via_handle[1].tobytes() and perm.tobytes() == via_handle[2].tobytes()
    assert list(route) == list(via_handle[3])


def test_solve_scenarios_with_a_basis(lps, oracle):
    """LPSolver.solve_scenarios(basis=...): the Decimal or the exception instance per scenario, .route on every info."""
    kinds = set()
    for name, case in (("24x40", rc.case(24, 40)), ("column 5x65", rc.column_case(5, 65))):
        basis, want = modelled(oracle, name, case)
        solver = lps.LPSolver(max_pivots=rc.budget_above(want))
        answers = solver.solve_scenarios(case["A"], case["b"], case["c"], maximize=case["maximize"], basis=basis)
        plain = lps.LPSolver(max_pivots=rc.budget_above(want))
        expect = plain.solve_scenarios(case["A"], case["b"], case["c"], maximize=case["maximize"])
        assert len(answers) == len(want) == len(solver.last_batch)
        for k, w in enumerate(want):
            info = solver.last_batch[k]
            assert info.route == w["route"] and plain.last_batch[k].route is None, (name, k)
            kinds.add(type(answers[k]).__name__)
            if w["route"] == "cold":
                assert type(answers[k]) is type(expect[k]) and str(answers[k]) == str(expect[k]), (name, k)
                continue
            assert (info.status, info.pivots_phase1, info.pivots_phase2) == (w["status"], w["pivots1"], w["pivots2"]), (name, k)
            assert np.array_equal(bits(solver.last_batch_x[k]), bits(w["x"])), (name, k)
            if w["status"] == rc.OPTIMAL:
                assert isinstance(answers[k], Decimal) and answers[k] == Decimal(w["objective_text"]), (name, k)
            else:   # the exception the cold solve of the same scenario gives: the verdicts agree
                assert isinstance(answers[k], Exception), (name, k)
                assert type(answers[k]) is type(expect[k]) and str(answers[k]) == str(expect[k]), (name, k)
    assert "Decimal" in kinds and len(kinds) >= 3, kinds      # optima, infeasible and unbounded scenarios


# ------------------------------------------------------------------------------------ 5. which arrays come back
def small_case():
    """rc.case(5, 4) and one more scenario, 16: the b of scenario 12 (b[1] = -1e6) under the cost of scenario 5 read as a
    `max`, which is the base's cost negated.  At the base's basis its b has a negative entry and its cost is improving:
    cold -- the route no scenario of rc.case(5, 4) takes from that basis -- and the cold solve is infeasible, so it ends
    inside phase 1 whatever the budget: no x, no perm."""
    case = rc.case(5, 4)
    case["b"] = np.vstack([case["b"], case["b"][12]])
    case["c"] = np.vstack([case["c"], case["c"][5]])
    case["maximize"] = case["maximize"] + [True]
    return case


# name: (basis (None: the base's), scenarios, their routes, which of them end inside phase 1, budget (None: above the model's))
OUTPUT_CALLS = {
    "cold, primal and dual": (None, [0, 12, 16, 1, 5], ["primal", "dual", "cold", "primal", "primal"], [16], None),
    "cold, primal and dual without a pivot": (None, [0, 12, 16, 1, 5], ["primal", "dual", "cold", "primal", "primal"], [16], 0),
    "no cold route": (None, [0, 12, 1, 5], ["primal", "dual", "primal", "primal"], [], None),
    "every route cold": ([3, 5, 6, 7, 8], [0, 12, 3], ["cold", "cold", "cold"], [12], None),   # a basis that is not the base's
}


def final_n_of_the_cold_solve(oracle, case, k, budget):
    _, st = oracle.solve(case["A"], case["b"][k], case["c"][k], case["maximize"][k], kind=oracle.FP64, max_pivots=budget,
                         want_trace=False)
    final_n = st.n
    st.close()
    return final_n


@pytest.mark.parametrize("call", sorted(OUTPUT_CALLS))
def test_each_choice_of_output_arrays_gets_the_same_rows(lps, oracle, call):
    """x_out and perm_out, x_out alone, perm_out alone, neither: every array that is passed holds what the call with both
    arrays put there, bit for bit; results (but for the times) and route_out are the same.  With and without a cold route
    in the call, and with cold solves that end inside phase 1 (their rows keep the sentinels) beside cold solves that end
    m x n.  The model says first that the inputs hold these routes and endings."""
    basis, rows, routes, inside_phase1, budget = OUTPUT_CALLS[call]
    case = small_case()
    m, n = case["A"].shape
    if basis is None:
        basis = rc.base_basis(oracle, case)
    want = rc.model_case(oracle, case, basis, -1 if budget is None else budget)
    if budget is None:
        budget = rc.budget_above(want)
    assert [want[k]["route"] for k in rows] == routes, call
    for k in rows:
        if want[k]["route"] == "cold":
            assert final_n_of_the_cold_solve(oracle, case, k, budget) == (n + 1 if k in inside_phase1 else n), (call, k)
    choices = [(True, False), (False, True), (False, False)]
    handle = lps.LPScenarios(case["A"])
    try:
        handle.set_basis(basis)
        cold = raw(handle, "lpx_scenarios_solve", case, budget, rows=rows)
        both = raw(handle, "lpx_scenarios_resolve", case, budget, rows=rows)
        others = [raw(handle, "lpx_scenarios_resolve", case, budget, rows=rows, pass_x=px, pass_perm=pp) for px, pp in choices]
    finally:
        handle.close()
    compare_all(both, cold, want, call, rows=rows)
    for t, k in enumerate(rows):
        if k in inside_phase1:
            assert np.all(both[1][t] == SENTINEL_X) and np.all(both[2][t] == SENTINEL_PERM), (call, k)
        else:
            assert sorted(both[2][t]) == list(range(n + m)), (call, k)
    untouched_x = np.full((len(rows), n), SENTINEL_X)
    untouched_perm = np.full((len(rows), n + m), SENTINEL_PERM, dtype=np.int32)
    for (px, pp), (res, x, perm, route) in zip(choices, others):
        what = "%s: x_out %s, perm_out %s" % (call, "passed" if px else "NULL", "passed" if pp else "NULL")
        assert [result_bytes(r) for r in res] == [result_bytes(r) for r in both[0]], what
        assert list(route) == list(both[3]), what
        assert x.tobytes() == (both[1] if px else untouched_x).tobytes(), what
        assert perm.tobytes() == (both[2] if pp else untouched_perm).tobytes(), what
