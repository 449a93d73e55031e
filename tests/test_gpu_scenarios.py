"""GPU parity of the scenario batches (k_batch_scenarios through lpx_scenarios_solve / LPScenarios, lpx_solve_scenarios and
LPSolver.solve_scenarios): ONE constraint matrix, many (b, c, max | min) in one launch, one workgroup per scenario,
against oracle.solve(A, b_k, c_k, max_k) scenario by scenario.

The bar, for EVERY scenario and in both arithmetic modes (oracle.FP64 is the instantiation of the mode the test runs in):
status, phase1_used, both pivot counts, x0's slot and the objective text equal, the objective bit for bit, perm equal, x
bit for bit the oracle's final state read the same way (a basic original variable takes b[row], every other 0) -- and the
rows of a scenario whose solve ended inside phase 1 still at the sentinels the test put there.

Every test runs the oracle first, on the CPU, and gives the GPU a FINITE budget well above the oracle's largest pivot
count: a divergence ends as a mismatch, not as a long loop.  tests/test_scenarios_host.py proves on the CPU that the
inputs (tests/scenario_cases.py) hold the verdicts these tests are about."""
import ctypes as C
from decimal import Decimal

import numpy as np
import pytest

from tests import scenario_cases as sc

pytestmark = pytest.mark.gpu

OPTIMAL, UNBOUNDED, INFEASIBLE, PIVOT_LIMIT = 0, 1, 2, 9
SENTINEL_X, SENTINEL_PERM = -7.0, -1


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


def rows_of(a, count, width):
    """`a` of shape (width,) or (count, width) as count rows."""
    a = np.asarray(a, dtype=np.float64)
    return np.broadcast_to(a, (count, width)) if a.ndim == 1 else a


_WANT = {}


def oracle_results(oracle, L, pricing, budget=-1, order=None, key=None):
    """Per scenario what the oracle says: its result dict plus final_n, perm and x (None where the final state is not
    m x n).  Computed once per (key, mode, pricing, budget) and shared."""
    full_key = None if key is None else (key, oracle.mode, pricing, budget, None if order is None else tuple(order))
    if full_key in _WANT:
        return _WANT[full_key]
    A = L["A"]
    m, n = A.shape
    count = len(L["maximize"])
    bs, cs = rows_of(L["b"], count, m), rows_of(L["c"], count, n)
    out = []
    for k in range(count):
        r, st = oracle.solve(A, bs[k], cs[k], L["maximize"][k], kind=oracle.FP64, restore_order=order, max_pivots=budget,
                             want_trace=False, pricing=1 if pricing == "dantzig" else 0)
        r["final_n"] = st.n
        r["perm"] = r["x"] = None
        if st.n == n:
            _, b, _, _, perm = st.read()
            x = np.zeros(n)
            for i in range(m):
                if perm[n + i] < n:
                    x[perm[n + i]] = b[i]
            r["perm"], r["x"] = np.asarray(perm, dtype=np.int32), x
        st.close()
        out.append(r)
    if full_key is not None:
        _WANT[full_key] = out
    return out


def budget_above(want):
    return 2 * max(r["pivots1"] + r["pivots2"] for r in want) + 100


def raw_solve(handle, L, budget, order=None, pass_x=True, pass_perm=True):
    """lpx_scenarios_solve through ctypes on the LPScenarios `handle`; b and c of L may be 1-D (pitch 0).  Returns
    (results, x, perm) with x and perm pre-filled with the sentinels; an array that is not passed (x_out / perm_out
    NULL) comes back as filled."""
    from linear_programming_solver_amd import _lib
    m, n = handle.m, handle.n
    count = len(L["maximize"])
    b = np.ascontiguousarray(L["b"], dtype=np.float64)
    c = np.ascontiguousarray(L["c"], dtype=np.float64)
    mx = np.array([1 if f else 0 for f in L["maximize"]], dtype=np.int32)
    res = (_lib.SolveResult * count)()
    x = np.full((count, n), SENTINEL_X)
    perm = np.full((count, n + m), SENTINEL_PERM, dtype=np.int32)
    o = None if order is None else np.ascontiguousarray(np.asarray(order, dtype=np.int32))
    keep = None if o is None else (o if o.size else np.zeros(1, dtype=np.int32))
    rc = handle._L.lpx_scenarios_solve(handle._h, count, b.ctypes.data_as(_lib.dp), m if b.ndim == 2 else 0,
                                       c.ctypes.data_as(_lib.dp), n if c.ndim == 2 else 0, mx.ctypes.data_as(_lib.ip),
                                       budget, None if keep is None else keep.ctypes.data_as(_lib.ip),
                                       -1 if o is None else int(o.size), res, x.ctypes.data_as(_lib.dp) if pass_x else None,
                                       perm.ctypes.data_as(_lib.ip) if pass_perm else None)
    assert rc == 0, _lib.last_error()
    return res, x, perm


def compare_scenario(res, x_row, perm_row, want, what):
    assert res.status == want["status"], "status differs %s: %d vs %d" % (what, res.status, want["status"])
    assert bool(res.phase1_used) == want["phase1_used"], "phase1_used differs " + what
    assert (res.pivots_phase1, res.pivots_phase2) == (want["pivots1"], want["pivots2"]), \
        "pivot counts differ %s: %r vs %r" % (what, (res.pivots_phase1, res.pivots_phase2), (want["pivots1"], want["pivots2"]))
    assert res.x0_slot == want["x0_slot"], "x0 slot differs " + what
    assert res.objective_text.decode() == want["objective_text"], "objective text differs " + what
    assert bits(np.array([res.objective]))[0] == bits(np.array([want["objective"]]))[0], "objective bits differ " + what
    if want["perm"] is not None:
        assert list(perm_row) == list(want["perm"]), "perm differs " + what
        assert np.array_equal(bits(x_row), bits(want["x"])), "x differs " + what
    else:   # ended inside phase 1: the caller's rows are left alone
        assert np.all(perm_row == SENTINEL_PERM) and np.all(x_row == SENTINEL_X), "rows written " + what


def solve_and_compare(lps, oracle, name, L, pricing="reference", budget=None, order=None, want=None):
    if want is None:
        want = oracle_results(oracle, L, pricing, -1 if budget is None else budget, order, key=name)
    handle = lps.LPScenarios(L["A"], pricing=pricing)
    try:
        res, x, perm = raw_solve(handle, L, budget_above(want) if budget is None else budget, order)
    finally:
        handle.close()
    for k, w in enumerate(want):
        compare_scenario(res[k], x[k], perm[k], w, "(%s, %s, scenario %d)" % (name, pricing, k))
    return want, (res, x, perm)


def result_bytes(res):
    """The results array with the times blanked."""
    out = []
    for r in res:
        keep = (r.seconds_total, r.seconds_pivots)
        r.seconds_total = r.seconds_pivots = 0.0
        out.append(bytes(r))
        r.seconds_total, r.seconds_pivots = keep
    return out


# ------------------------------------------------------------------------------------ 1. every launch against the oracle
@pytest.mark.parametrize("pricing", ["reference", "dantzig"])
def test_every_launch_matches_the_oracle(lps, oracle, pricing):
    """All shapes, all scenario kinds (no phase 1, feasible and infeasible phase 1, signed costs with `min`, unbounded
    columns) and the 96 x 200 launch with more than 64 KiB of dynamic LDS."""
    seen = set()
    for name, L in sc.launches():
        want, _ = solve_and_compare(lps, oracle, name, L, pricing=pricing)
        seen |= {(r["status"], bool(r["phase1_used"])) for r in want}
    assert {(OPTIMAL, False), (OPTIMAL, True), (INFEASIBLE, True), (UNBOUNDED, False)} <= seen


# ------------------------------------------------------------------------------------ 2. shared vectors
def test_a_shared_b_or_c_is_the_replicated_one(lps, oracle):
    """ldb = 0 with varying c, and ldc = 0 with varying b, each against the same call with the vector replicated."""
    L = sc.mixed_launch(24, 40)
    count = len(L["maximize"])
    for shared, k_shared in (("b", 1), ("b", 0), ("c", 3)):          # b[1] needs phase 1, b[0] does not
        one = dict(L)
        one[shared] = L[shared][k_shared].copy()
        rep = dict(L)
        rep[shared] = np.tile(L[shared][k_shared], (count, 1))
        want = oracle_results(oracle, rep, "reference")
        handle = lps.LPScenarios(L["A"])
        try:
            got_one = raw_solve(handle, one, budget_above(want))
            got_rep = raw_solve(handle, rep, budget_above(want))
        finally:
            handle.close()
        for k, w in enumerate(want):
            compare_scenario(got_rep[0][k], got_rep[1][k], got_rep[2][k], w, "(replicated %s, scenario %d)" % (shared, k))
        assert result_bytes(got_one[0]) == result_bytes(got_rep[0]), shared
        assert got_one[1].tobytes() == got_rep[1].tobytes() and got_one[2].tobytes() == got_rep[2].tobytes(), shared


# ------------------------------------------------------------------------------------ 3. one handle, many solves
def test_one_handle_solved_twice(lps, oracle):
    """First 12 scenarios, then 5 others on the same handle (smaller count, other data, other flags), through
    LPScenarios.solve: the second answer is the oracle's, whatever the first left in the buffers."""
    first = sc.mixed_launch(24, 40)
    L2 = sc.signed_cost_launch(24, 40)
    assert np.array_equal(first["A"], L2["A"])
    second = {"A": L2["A"], "b": L2["b"][3:8], "c": L2["c"][3:8], "maximize": L2["maximize"][3:8]}
    want1 = oracle_results(oracle, first, "reference", key="mixed 24x40")
    want2 = oracle_results(oracle, second, "reference")
    handle = lps.LPScenarios(first["A"])
    try:
        for L, want in ((first, want1), (second, want2), (first, want1)):
            infos = handle.solve(L["b"], L["c"], maximize=L["maximize"], max_pivots=budget_above(want))
            assert len(infos) == len(want)
            for k, (info, w) in enumerate(zip(infos, want)):
                what = "(scenario %d of %d)" % (k, len(want))
                assert (info.status, info.phase1_used, info.pivots_phase1, info.pivots_phase2, info.x0_slot) == \
                    (w["status"], w["phase1_used"], w["pivots1"], w["pivots2"], w["x0_slot"]), what
                assert info.objective_text == w["objective_text"], what
                assert bits(np.array([info.objective]))[0] == bits(np.array([w["objective"]]))[0], what
                if w["perm"] is None:
                    assert info.perm is None and info.x is None, what
                else:
                    assert list(info.perm) == list(w["perm"]) and np.array_equal(bits(info.x), bits(w["x"])), what
    finally:
        handle.close()


# ------------------------------------------------------------------------------------ 4. budget
def test_a_budget_ends_exactly_the_scenarios_it_ends_in_the_oracle(lps, oracle):
    L = sc.mixed_launch(24, 40)
    full = oracle_results(oracle, L, "reference", key="mixed 24x40")
    budget = 40
    assert min(r["pivots1"] + r["pivots2"] for r in full) < budget < max(r["pivots1"] for r in full)
    want, _ = solve_and_compare(lps, oracle, "mixed 24x40", L, budget=budget)
    limited = [r["status"] == PIVOT_LIMIT for r in want]
    assert any(limited) and not all(limited)
    assert any(r["status"] == PIVOT_LIMIT and r["final_n"] == 41 for r in want)       # inside phase 1
    assert any(r["status"] == PIVOT_LIMIT and r["final_n"] == 40 for r in want)       # inside phase 2


# ------------------------------------------------------------------------------------ 5. against lpx_solve_batch_all
@pytest.mark.parametrize("shape", [(24, 40), (5, 65)])
def test_one_shot_equals_solve_batch_all_on_the_replicated_forms(lps, oracle, shape):
    from linear_programming_solver_amd import _lib
    from linear_programming_solver_amd.lp_batch import pack_lps, solve_packed
    L = sc.mixed_launch(*shape)
    m, n = shape
    count = len(L["maximize"])
    want = oracle_results(oracle, L, "reference", key="mixed %dx%d" % shape)
    opts = lps.LPSolver(max_pivots=budget_above(want))._solve_options()
    opts.restore_order_len = -1
    mx = np.array([1 if f else 0 for f in L["maximize"]], dtype=np.int32)
    res_b, x_b, perm_b, took = solve_packed(pack_lps([(L["A"], L["b"][k], L["c"][k]) for k in range(count)]), mx, opts, True)
    assert took == count
    res_s = (_lib.SolveResult * count)()
    x_s = np.full((count, n), SENTINEL_X)
    perm_s = np.full((count, n + m), SENTINEL_PERM, dtype=np.int32)
    A = np.ascontiguousarray(L["A"])
    rc = _lib.lib().lpx_solve_scenarios(m, n, A.ctypes.data_as(_lib.dp), n, count, L["b"].ctypes.data_as(_lib.dp), m,
                                        L["c"].ctypes.data_as(_lib.dp), n, mx.ctypes.data_as(_lib.ip), C.byref(opts), res_s,
                                        x_s.ctypes.data_as(_lib.dp), perm_s.ctypes.data_as(_lib.ip))
    assert rc == 0, _lib.last_error()
    assert result_bytes(res_s) == result_bytes(res_b)
    ended_in_phase1 = 0
    for k in range(count):
        compare_scenario(res_s[k], x_s[k], perm_s[k], want[k], "(one shot, scenario %d)" % k)
        if perm_b[k, 0] < 0:     # lpx_solve_batch_all left the row alone
            ended_in_phase1 += 1
            assert np.all(perm_s[k] == SENTINEL_PERM) and np.all(x_s[k] == SENTINEL_X), k
        else:
            assert list(perm_s[k]) == list(perm_b[k, :n + m]) and np.array_equal(bits(x_s[k]), bits(x_b[k, :n])), k
    assert 0 < ended_in_phase1 < count


# ------------------------------------------------------------------------------------ 6. restore order
def test_custom_restore_orders(lps, oracle):
    """The ONE order of restoreInitialLP decides the rounding of c and v of every phase-1 scenario.  A reversed order
    against the oracle with that order.  An empty order substitutes nothing: c = 0 and v = 0 after the restore, phase 2
    ends at once.  The oracle's solve() always takes n entries, so the empty order is checked against the oracle on the
    same scenarios with c = 0: its restore accumulates 0 + coef * 0 (= +0.0 in round-to-nearest, fused or not) into every
    c[j] and into v, which is what no substitution leaves, and phase 1 never reads c."""
    for shape in [(24, 40), (5, 65)]:
        L = sc.mixed_launch(*shape)
        n = shape[1]
        rev = oracle.java_default_name_order(n)[::-1].copy()
        want, _ = solve_and_compare(lps, oracle, "mixed %dx%d reversed" % shape, L, order=rev)
        default = oracle_results(oracle, L, "reference", key="mixed %dx%d" % shape)
        assert any(r["phase1_used"] and r["status"] == OPTIMAL for r in want)
        if shape == (24, 40):   # the order matters: some phase-1 objective differs in its last bits
            assert any(bits(np.array([a["objective"]]))[0] != bits(np.array([d["objective"]]))[0]
                       for a, d in zip(want, default) if a["phase1_used"] and a["status"] == OPTIMAL)
        p1 = [k for k, r in enumerate(default) if r["phase1_used"]]
        empty = {"A": L["A"], "b": L["b"][p1], "c": L["c"][p1], "maximize": [True] * len(p1)}
        zero_c = dict(empty)
        zero_c["c"] = np.zeros_like(empty["c"])
        want0 = oracle_results(oracle, zero_c, "reference")
        solve_and_compare(lps, oracle, "mixed %dx%d empty order" % shape, empty, order=[], want=want0)
        assert any(r["status"] == OPTIMAL and r["pivots2"] == 0 and r["objective_text"] == "0.000000" for r in want0)


# ------------------------------------------------------------------------------------ 7. LPSolver.solve_scenarios
def test_solve_scenarios_matches_solve_form_by_form(lps, oracle):
    kinds = set()
    for L in (sc.mixed_launch(5, 65), sc.column_launch(5, 65)):
        count = len(L["maximize"])
        want = oracle_results(oracle, L, "reference")
        solver = lps.LPSolver(max_pivots=budget_above(want))
        answers = solver.solve_scenarios(L["A"], L["b"], L["c"], maximize=L["maximize"])
        assert len(answers) == count == len(solver.last_batch) == len(solver.last_batch_x)
        for k in range(count):
            alone = lps.LPSolver()
            try:
                expect = alone.solve(lps.LPStandardForm(L["A"], L["b"][k], L["c"][k], maximize=L["maximize"][k]))
            except Exception as exc:
                expect = exc
            got = answers[k]
            if isinstance(expect, Exception):
                assert type(got) is type(expect) and str(got) == str(expect), (k, got, expect)
            else:
                assert isinstance(got, Decimal) and got == expect, (k, got, expect)
            kinds.add(type(expect).__name__)
            info = solver.last_batch[k]
            assert (info.status, info.pivots_phase1, info.pivots_phase2) == \
                (alone.last.status, alone.last.pivots_phase1, alone.last.pivots_phase2), k
            if want[k]["perm"] is None:
                assert solver.last_batch_x[k] is None and info.perm is None, k
            else:
                assert np.array_equal(bits(solver.last_batch_x[k]), bits(alone.last.x)), k
                assert list(info.perm) == list(alone.last.perm), k
    assert "Decimal" in kinds and len(kinds) >= 2, kinds      # optima, and the infeasible and unbounded scenarios' exceptions


# ------------------------------------------------------------------------------------ 8. which arrays come back
@pytest.mark.parametrize("budget", [1, None])
def test_each_choice_of_output_arrays_gets_the_same_rows(lps, oracle, budget):
    """x_out and perm_out, x_out alone, perm_out alone, neither: every array that is passed holds what the call with both
    arrays put there, bit for bit, and the results are the same but for the times.  6 scenarios of a 4 x 4 matrix, two of
    which need phase 1: under a budget of 1 those two end inside phase 1 (their rows keep the sentinels) and the others
    m x n; without a budget (None: a finite one above the oracle's pivots) every scenario ends m x n."""
    L = sc.signed_cost_launch(4, 4, count=6)
    m, n = L["A"].shape
    count = len(L["maximize"])
    want = oracle_results(oracle, L, "reference", -1 if budget is None else budget, key="signed 4x4")
    ended = [r["final_n"] for r in want]
    if budget is None:
        assert ended == [n] * count and any(r["phase1_used"] for r in want)
        budget = budget_above(want)
    else:
        assert n + 1 in ended and n in ended
    choices = [(True, False), (False, True), (False, False)]
    handle = lps.LPScenarios(L["A"])
    try:
        both = raw_solve(handle, L, budget)
        others = [raw_solve(handle, L, budget, pass_x=px, pass_perm=pp) for px, pp in choices]
    finally:
        handle.close()
    for k, w in enumerate(want):
        compare_scenario(both[0][k], both[1][k], both[2][k], w, "(both arrays, scenario %d)" % k)
    untouched_x = np.full((count, n), SENTINEL_X)
    untouched_perm = np.full((count, n + m), SENTINEL_PERM, dtype=np.int32)
    for (px, pp), (res, x, perm) in zip(choices, others):
        what = "x_out %s, perm_out %s" % ("passed" if px else "NULL", "passed" if pp else "NULL")
        assert result_bytes(res) == result_bytes(both[0]), what
        assert x.tobytes() == (both[1] if px else untouched_x).tobytes(), what
        assert perm.tobytes() == (both[2] if pp else untouched_perm).tobytes(), what
