"""GPU parity of the batched solve with phase 1 inside the kernel (k_batch_solve through lpx_batch_solve / LPBatch.solve,
lpx_solve_batch_all and LPSolver.solve_batch(phase1="kernel")): LPSolver.solve for many small standard forms in one
launch, one workgroup per form, against oracle.solve on the same inputs.

The bar, for EVERY LP of a batch and in both arithmetic modes (oracle.FP64 is the instantiation of the mode the test runs
in): status, phase1_used, the two pivot counts, x0's slot, the objective text and the objective bits equal; the final
A, b, c, v, perm of LPBatch.read(k) bit for bit the oracle's final State, shape included (m x (n + 1) where the solve
ended inside phase 1).

Every test runs the oracle first, on the CPU, and gives the GPU a FINITE budget well above the oracle's pivot count: a
divergence ends as a mismatch, not as an endless loop.  test_unlimited_budget alone passes -1, on inputs the other
tests have already compared.  Each test asserts, from the oracle's own results, that its inputs hold what it claims."""
import ctypes as C
from decimal import Decimal

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPTIMAL, UNBOUNDED, INFEASIBLE, AUX_UNBOUNDED, NO_DEGENERATE_PIVOT, RESTORE_INDEX_FAULT, PIVOT_LIMIT = 0, 1, 2, 3, 4, 6, 9


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


def assert_state_bits_equal(got, want, what=""):
    gA, gb, gc, gv, gp = got
    wA, wb, wc, wv, wp = want
    assert gA.shape == wA.shape, "shape differs %s: %s vs %s" % (what, gA.shape, wA.shape)
    assert np.array_equal(bits(gA), bits(wA)), "A differs " + what
    assert np.array_equal(bits(gb), bits(wb)), "b differs " + what
    assert np.array_equal(bits(gc), bits(wc)), "c differs " + what
    assert bits(np.array([gv]))[0] == bits(np.array([wv]))[0], "v differs %s: %r vs %r" % (what, gv, wv)
    assert list(gp) == list(wp), "perm differs " + what


# ------------------------------------------------------------------------------------ input families
def dense_lp(m, n, seed):
    """SURVEY §8(d) synthetic input: A ~ U(0,1), b = (n/4) U(1,2), c ~ U(0,1)."""
    rng = np.random.default_rng(seed)
    return rng.random((m, n)), (n / 4.0) * (1.0 + rng.random(m)), rng.random(n)


def seed_of(m, n, s):
    return 1000 * m + n + 17 * s


def feasible_phase1_lp(m, n, s):
    """dense_lp with every third row turned into a >= row that x* = 0.5 U(0,1)^n satisfies: negative b, feasible."""
    seed = seed_of(m, n, s)
    A, b, c = dense_lp(m, n, seed)
    xs = 0.5 * np.random.default_rng(seed + 77777).random(n)
    for i in range(0, m, 3):
        b[i] = -0.5 * (A[i] @ xs)
        A[i] = -A[i]
    return A, b, c


def infeasible_lp(m, n, s):
    """Rows 0 and 1 contradict each other: A[0] x <= 1 and A[0] x >= 2."""
    A, b, c = dense_lp(m, n, seed_of(m, n, s))
    A[1] = -A[0]
    b[0], b[1] = 1.0, -2.0
    return A, b, c


def integer_lp(m, n, s):
    rng = np.random.default_rng(seed_of(m, n, s))
    A = rng.integers(-3, 4, size=(m, n)).astype(np.float64)
    b = rng.integers(-2, 6, size=m).astype(np.float64)
    c = rng.integers(-2, 4, size=n).astype(np.float64)
    return A, b, c


def degenerate_lp():
    """Hand-built (the integer family holds a degenerate pivot under some rules and arithmetic modes only): rows 1 and 2
    say x1 + 2 x2 <= 1 and x1 + 2 x2 >= 1, so phase 1 ends with x0 still basic at value 0 and performDegeneratePivot has
    to take it out.  Small integers: the same pivots in both arithmetic modes and under both entering rules."""
    return np.array([[2.0, 2.0], [1.0, 2.0], [-1.0, -2.0]]), np.array([1.0, 1.0, -1.0]), np.array([2.0, -1.0])


FEASIBLE_SHAPES = [(1, 1), (2, 1), (1, 3), (5, 63), (5, 64), (5, 65), (63, 5), (65, 5), (33, 130), (24, 40)]
INFEASIBLE_SHAPES = [(2, 1), (5, 63), (9, 7), (24, 40)]
INTEGER_SHAPES = [(4, 3), (6, 5), (8, 6), (12, 9)]


# ------------------------------------------------------------------------------------ the comparison
def needs_phase1(b):
    return len(b) > 0 and min(b) < 0


def took_degenerate_pivot(oracle, case, res):
    """Replays the auxiliary LP through all phase-1 pivots of the trace but the last: if nothing may enter there, the
    loop of solveAuxLP had ended and the last phase-1 pivot was performDegeneratePivot."""
    p1 = [r for r in res["trace"] if r[0] == 1]
    if len(p1) < 2 or res["status"] not in (OPTIMAL, UNBOUNDED, RESTORE_INDEX_FAULT):   # phase 1 did not get that far
        return False
    aux = oracle.convert_into_aux_lp(case[0], case[1], kind=oracle.FP64)
    for _, e, l in p1[:-1]:
        aux.pivot(int(e), int(l))
    ended = aux.get_entering() == -1
    aux.close()
    return ended


def oracle_solve(oracle, case, pricing, max_pivots=-1, want_trace=False):
    A, b, c, mx = case[:4]
    order = case[4] if len(case) > 4 else None
    res, st = oracle.solve(A, b, c, mx, kind=oracle.FP64, restore_order=order, max_pivots=max_pivots,
                           want_trace=want_trace, pricing=1 if pricing == "dantzig" else 0)
    res["final_n"] = st.n
    return res, st


def compare_info(info, res, what):
    assert info.status == res["status"], "status differs %s: %d vs %d" % (what, info.status, res["status"])
    assert info.phase1_used == res["phase1_used"], "phase1_used differs " + what
    assert (info.pivots_phase1, info.pivots_phase2) == (res["pivots1"], res["pivots2"]), \
        "pivot counts differ %s: %r vs %r" % (what, (info.pivots_phase1, info.pivots_phase2), (res["pivots1"], res["pivots2"]))
    assert info.x0_slot == res["x0_slot"], "x0 slot differs " + what
    assert info.objective_text == res["objective_text"], "objective text differs " + what
    assert bits(np.array([info.objective]))[0] == bits(np.array([res["objective"]]))[0], "objective bits differ " + what


def solve_and_compare(lps, oracle, cases, pricing="reference", max_pivots=None, want_trace=False, unlimited=False):
    """cases: (A, b, c, maximize[, restore_order]).  The oracle first; then ONE batch with a finite budget (max_pivots when
    given: the oracle then ran with the same one).  Returns the oracle's result dicts."""
    want = [oracle_solve(oracle, case, pricing, -1 if max_pivots is None else max_pivots, want_trace) for case in cases]
    budget = max_pivots
    if budget is None:
        budget = -1 if unlimited else 2 * max(r["pivots1"] + r["pivots2"] for r, _ in want) + 100
    batch = lps.LPBatch([case[:3] for case in cases], pricing=pricing)
    orders = None
    if any(len(case) > 4 for case in cases):
        orders = [case[4] if len(case) > 4 else None for case in cases]
    infos = batch.solve(maximize=[case[3] for case in cases], max_pivots=budget, restore_orders=orders)
    assert len(infos) == len(cases)
    for k, (case, (res, st)) in enumerate(zip(cases, want)):
        m, n = len(case[1]), len(case[2])
        what = "(LP %d, %d x %d, %s)" % (k, m, n, "max" if case[3] else "min")
        compare_info(infos[k], res, what)
        assert batch.shape(k) == (st.m, st.n), "shape differs " + what
        assert_state_bits_equal(batch.read(k), st.read(), what)
        if st.n == n:   # an m x n final state carries perm and the solution
            _, b, _, _, perm = st.read()
            x = np.zeros(n)
            for i in range(m):
                if perm[n + i] < n:
                    x[perm[n + i]] = b[i]
            assert list(infos[k].perm) == list(perm) and np.array_equal(bits(infos[k].x), bits(x)), "x differs " + what
        else:
            assert infos[k].perm is None and infos[k].x is None, what
        st.close()
    batch.close()
    return [r for r, _ in want]


# ------------------------------------------------------------------------------------ 1. feasible phase 1
@pytest.mark.parametrize("pricing", ["reference", "dantzig"])
def test_feasible_phase1_shapes_in_one_batch(lps, oracle, pricing):
    """n + 1 crosses the 64-column chunk and the workgroup-size boundaries; max and min; phase 2 is reached."""
    cases = [feasible_phase1_lp(m, n, s) + (mx,) for (m, n) in FEASIBLE_SHAPES for s in range(3) for mx in (True, False)]
    res = solve_and_compare(lps, oracle, cases, pricing=pricing)
    assert all(r["phase1_used"] for r in res)
    assert {r["status"] for r in res} == {OPTIMAL, UNBOUNDED}
    assert sum(r["status"] == OPTIMAL for r in res) > len(res) // 2
    assert all(r["pivots1"] >= 1 for r in res) and max(r["pivots2"] for r in res) >= 20
    if pricing == "reference":   # each shape alone: the LP then runs at the workgroup size of its own shape
        for (m, n) in FEASIBLE_SHAPES:
            solve_and_compare(lps, oracle, [feasible_phase1_lp(m, n, 0) + (True,)])


# ------------------------------------------------------------------------------------ 2. infeasible
@pytest.mark.parametrize("pricing", ["reference", "dantzig"])
def test_infeasible_forms(lps, oracle, pricing):
    cases = [infeasible_lp(m, n, s) + (mx,) for (m, n) in INFEASIBLE_SHAPES for s in range(3) for mx in (True, False)]
    res = solve_and_compare(lps, oracle, cases, pricing=pricing)
    assert all(r["status"] == INFEASIBLE and r["pivots1"] == 2 and r["pivots2"] == 0 for r in res)
    assert all(r["final_n"] == len(case[2]) + 1 for r, case in zip(res, cases))       # the auxiliary LP comes back


# ------------------------------------------------------------------------------------ 3. small integer LPs
def solve_launch_info(lps, batch):
    fn = batch._L.lpxi_batch_solve_launch_info
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    t, lds, per_cu = C.c_int32(), C.c_int32(), C.c_int32()
    assert fn(batch._h, C.byref(t), C.byref(lds), C.byref(per_cu)) == 0
    return t.value, lds.value, per_cu.value


@pytest.mark.parametrize("pricing", ["reference", "dantzig"])
def test_small_integer_lps_as_one_batch(lps, oracle, pricing):
    """Every status of LPSolver.solve that these inputs reach, phase-1 and plain forms side by side, the degenerate pivot,
    the reference's index fault in restoreInitialLP — and, with three 33 x 130 forms setting the launch's LDS and
    workgroup size, more workgroups than the chip holds at once and tiny LPs on a many-wave workgroup."""
    cases = [integer_lp(m, n, s) + (mx,) for (m, n) in INTEGER_SHAPES for s in range(150) for mx in (True, False)]
    cases.append(degenerate_lp() + (True,))
    cases += [feasible_phase1_lp(33, 130, s) + (True,) for s in range(3)]
    res = solve_and_compare(lps, oracle, cases, pricing=pricing, want_trace=True)
    assert {r["status"] for r in res} == {OPTIMAL, UNBOUNDED, INFEASIBLE, RESTORE_INDEX_FAULT}
    with_p1 = sum(bool(r["phase1_used"]) for r in res)
    assert 100 < with_p1 < len(res) - 100
    assert all(bool(r["phase1_used"]) == needs_phase1(case[1]) for r, case in zip(res, cases))
    degenerate = [k for k, (r, case) in enumerate(zip(res, cases)) if took_degenerate_pivot(oracle, case, r)]
    assert len(degenerate) >= 1
    assert took_degenerate_pivot(oracle, cases[1200], res[1200]) and res[1200]["status"] == OPTIMAL   # the hand-built one
    batch = lps.LPBatch([case[:3] for case in cases], pricing=pricing)
    threads, lds_bytes, per_cu = solve_launch_info(lps, batch)
    batch.close()
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert threads > 256 and 1 <= per_cu and per_cu * cus < len(cases), (threads, lds_bytes, per_cu, cus)


# ------------------------------------------------------------------------------------ 4. budgets
def test_budgets_inside_both_phases(lps, oracle):
    """Budgets 0, 1, pivots1, pivots1 + 1 and one inside phase 2: the forced pivot is made at budget 0, PIVOT_LIMIT falls
    inside phase 1 (the auxiliary LP comes back) and inside phase 2."""
    case = feasible_phase1_lp(24, 40, 0) + (True,)
    full, st = oracle_solve(oracle, case, "reference")
    st.close()
    p1, p2 = full["pivots1"], full["pivots2"]
    assert full["status"] == OPTIMAL and p1 >= 3 and p2 >= 3, (p1, p2)
    seen = {}
    for budget in (0, 1, p1 - 1, p1, p1 + 1, p1 + p2 - 1, p1 + p2):
        (r,) = solve_and_compare(lps, oracle, [case, ], max_pivots=budget)
        seen[budget] = r
    assert seen[0]["status"] == PIVOT_LIMIT and seen[0]["pivots1"] == 1 and seen[0]["final_n"] == 41
    assert seen[1]["status"] == PIVOT_LIMIT and seen[1]["pivots1"] == 1 and seen[1]["final_n"] == 41
    assert seen[p1 - 1]["status"] == PIVOT_LIMIT and seen[p1 - 1]["pivots2"] == 0
    assert seen[p1]["status"] == PIVOT_LIMIT and (seen[p1]["pivots1"], seen[p1]["pivots2"]) == (p1, 0)
    assert seen[p1]["final_n"] == 40                                                  # restored, then out of budget
    assert seen[p1 + 1]["status"] == PIVOT_LIMIT and seen[p1 + 1]["pivots2"] == 1
    assert seen[p1 + p2 - 1]["status"] == PIVOT_LIMIT and seen[p1 + p2]["status"] == OPTIMAL


# ------------------------------------------------------------------------------------ 5. largest fit
def test_largest_phase1_fit_and_one_past_it(lps, oracle):
    from linear_programming_solver_amd import _lib
    L = _lib.lib()
    m = 1
    while L.lpx_batch_solve_lds_bytes(m + 1, 200) <= _lib.BATCH_LDS_BYTES:
        m += 1
    assert L.lpx_batch_solve_lds_bytes(m, 200) <= _lib.BATCH_LDS_BYTES < L.lpx_batch_solve_lds_bytes(m + 1, 200)
    assert L.lpx_batch_lds_bytes(m + 1, 200) <= _lib.BATCH_LDS_BYTES                   # it is phase 1 that does not fit
    big = feasible_phase1_lp(m, 200, 0) + (True,)
    res = solve_and_compare(lps, oracle, [big, feasible_phase1_lp(3, 4, 0) + (False,)])
    assert res[0]["phase1_used"] and res[0]["status"] in (OPTIMAL, UNBOUNDED) and res[0]["pivots2"] >= 1
    batch = lps.LPBatch([feasible_phase1_lp(3, 4, 0), feasible_phase1_lp(m + 1, 200, 0)])   # creating it is fine
    with pytest.raises(ValueError) as ei:                                               # LPX_BAD_ARGUMENT
        batch.solve()
    batch.close()
    assert "LP 1" in str(ei.value) and "%d x 200" % (m + 1) in str(ei.value)


# ------------------------------------------------------------------------------------ 6. restore order per LP
def test_restore_order_per_lp(lps, oracle):
    """The order of restoreInitialLP decides the rounding of c and v: each LP of the batch takes its own."""
    m, n = 9, 7
    base = feasible_phase1_lp(m, n, 1)
    default = oracle.java_default_name_order(n)
    rev = default[::-1].copy()
    rot = np.roll(default, 3)
    cases = [base + (True, default), base + (True, rev), base + (True, rot), base + (False, rev), base + (True,)]
    res = solve_and_compare(lps, oracle, cases)
    assert all(r["status"] in (OPTIMAL, UNBOUNDED) and r["pivots1"] >= 2 for r in res)
    assert res[0]["objective"] == res[4]["objective"]        # no order given = the default-name order


def test_named_form_takes_its_key_set_order_in_the_kernel(lps, oracle):
    A, b, c = feasible_phase1_lp(9, 7, 2)
    names = ["w", "alpha", "x3", "beta", "q", "x1", "zz"]
    form = lps.LPStandardForm(A, b, c, maximize=True, variables={i: nm for i, nm in enumerate(names)},
                              coefficients={nm: i for i, nm in enumerate(names)})
    assert form.has_variable_names()
    order = lps.LPSolver._key_set_order(form)
    assert sorted(order.tolist()) == list(range(7)) and order.tolist() != oracle.java_default_name_order(7).tolist()
    res, st = oracle.solve(A, b, c, True, kind=oracle.FP64, restore_order=order, want_trace=False)
    st.close()
    solver = lps.LPSolver(max_pivots=2 * (res["pivots1"] + res["pivots2"]) + 100)
    (got,) = solver.solve_batch([form], phase1="kernel")
    assert solver.last_batch_in_kernel == 1
    compare_info(solver.last_batch[0], res, "(named form)")
    alone = lps.LPSolver()
    assert got == alone.solve(form)
    assert np.array_equal(bits(solver.last_batch_x[0]), bits(alone.last.x))


# ------------------------------------------------------------------------------------ 7. solve_batch / lpx_solve_batch_all
def test_solve_batch_in_kernel_matches_solve_form_by_form(lps, oracle, reference_vectors):
    cases = [(np.asarray(c["A"], dtype=np.float64), np.asarray(c["b"], dtype=np.float64),
              np.asarray(c["c"], dtype=np.float64), c["maximize"]) for c in reference_vectors["solve"]]
    cases += [dense_lp(32, 48, 300 + k) + (k % 2 == 0,) for k in range(4)]
    cases += [feasible_phase1_lp(24, 40, s) + (s % 2 == 0,) for s in range(4)]
    cases += [infeasible_lp(9, 7, 0) + (True,), integer_lp(8, 6, 5) + (True,), degenerate_lp() + (True,)]
    forms = [lps.LPStandardForm(A, b, c, maximize=mx) for A, b, c, mx in cases]
    want = [oracle_solve(oracle, case, "reference") for case in cases]
    budget = 2 * max(r["pivots1"] + r["pivots2"] for r, _ in want) + 100
    solver = lps.LPSolver(max_pivots=budget)
    answers = solver.solve_batch(forms, phase1="kernel")
    assert len(answers) == len(forms) == len(solver.last_batch) == len(solver.last_batch_x)
    assert solver.last_batch_in_kernel == len(forms)
    with_p1 = sum(needs_phase1(b) for _, b, _, _ in cases)
    assert 0 < with_p1 < len(forms)
    kinds = set()
    for k, (form, (res, st)) in enumerate(zip(forms, want)):
        alone = lps.LPSolver()
        try:
            expect = alone.solve(form)
        except Exception as exc:
            expect = exc
        got, info = answers[k], solver.last_batch[k]
        if isinstance(expect, Exception):
            assert type(got) is type(expect) and str(got) == str(expect), (k, got, expect)
        else:
            assert isinstance(got, Decimal) and got == expect, (k, got, expect)
        kinds.add(type(expect).__name__)
        for mine in (info, alone.last):
            compare_info(mine, res, "(form %d)" % k)
        if st.n == form.n:
            assert np.array_equal(bits(solver.last_batch_x[k]), bits(alone.last.x)), k
            assert list(info.perm) == list(alone.last.perm) == list(st.read()[4]), k
        else:
            assert solver.last_batch_x[k] is None and info.perm is None, k
        st.close()
    assert kinds == {"Decimal", "SolutionException", "LPException"}
    # the default stays what it was: only the forms without phase 1 ride in the kernel
    host = lps.LPSolver()
    again = host.solve_batch(forms)
    assert host.last_batch_in_kernel == len(forms) - with_p1
    assert [str(a) for a in again] == [str(a) for a in answers]


# ------------------------------------------------------------------------------------ 8. handle rules, unlimited budget
def test_solve_needs_a_fresh_handle(lps, oracle):
    batch = lps.LPBatch([dense_lp(3, 4, 1), feasible_phase1_lp(3, 4, 0)])
    batch.simplex_loop(0)
    with pytest.raises(ValueError):
        batch.solve(max_pivots=50)
    batch.close()
    batch = lps.LPBatch([feasible_phase1_lp(3, 4, 0)])
    batch.solve(max_pivots=50)
    with pytest.raises(ValueError):
        batch.solve(max_pivots=50)
    with pytest.raises(ValueError):
        batch.simplex_loop(0)
    batch.close()


def test_unlimited_budget(lps, oracle):
    """max_pivots = -1 on inputs the tests above have compared with a finite budget."""
    cases = [feasible_phase1_lp(24, 40, 0) + (True,), infeasible_lp(9, 7, 0) + (False,), integer_lp(8, 6, 5) + (True,),
             dense_lp(5, 6, 3) + (True,), degenerate_lp() + (True,)]
    res = solve_and_compare(lps, oracle, cases, unlimited=True)
    assert res[0]["status"] == OPTIMAL and res[1]["status"] == INFEASIBLE


# ------------------------------------------------------------------------------------ 9. the one-shot calls' index scatter
SENTINEL_X, SENTINEL_PERM = -7.25, -77


def scatter_cases():
    """Seven forms whose routes interleave under the padding of the largest (m_max x n_max = 97 x 200), `max` and `min`
    and b >= 0 and a negative b in alternation.  The seeds (the s of seed_of, or dense_lp's seed) were chosen with the oracle
    on the CPU: the 5 x 7 form (s = 0) and the 97 x 200 form (s = 0) are feasible and reach phase 2, the second 3 x 2 form
    is infeasible by construction; the test asserts all of that from the oracle's results.  97 x 200 is one row past what
    lpx_batch_solve_lds_bytes admits: lpx_solve_batch_all leaves it to lpx_solve."""
    return [dense_lp(3, 2, 11) + (True,),
            feasible_phase1_lp(5, 7, 0) + (False,),
            dense_lp(1, 1, 12) + (True,),
            feasible_phase1_lp(97, 200, 0) + (False,),
            (np.zeros((0, 3)), np.zeros(0), np.array([0.5, -1.0, 0.25]), True),
            infeasible_lp(3, 2, 0) + (False,),
            dense_lp(4, 9, 13) + (True,)]


def one_shot(lps, arith, cases, budget, all_in_kernel, maximize_given=True):
    """lpx_solve_batch or lpx_solve_batch_all through ctypes.  Returns (SolveInfos, n_in_batch, x, perm): x and perm are
    the rows handed to lpx_solve_batch_all, pre-filled with the sentinels, and None for lpx_solve_batch."""
    from linear_programming_solver_amd import _lib
    from linear_programming_solver_amd.lp_solver import SolveInfo
    L = _lib.lib()
    p = lps.pack_lps([case[:3] for case in cases])
    cnt = p["count"]
    maxi = np.array([1 if case[3] else 0 for case in cases], dtype=np.int32)
    opts = _lib.SolveOptions()
    opts.max_pivots = budget
    opts.fused = 1 if arith == "fused" else -1
    opts.restore_order_len = -1
    res = (_lib.SolveResult * cnt)()
    took = C.c_int32(-1)
    args = [cnt, p["m_max"], p["n_max"], p["m"].ctypes.data_as(_lib.ip), p["n"].ctypes.data_as(_lib.ip),
            p["A"].ctypes.data_as(_lib.dp), p["lda"], p["strideA"], p["b"].ctypes.data_as(_lib.dp),
            p["c"].ctypes.data_as(_lib.dp), maxi.ctypes.data_as(_lib.ip) if maximize_given else None, C.byref(opts), res]
    x = perm = None
    if all_in_kernel:
        x = np.full((cnt, p["n_max"]), SENTINEL_X)
        perm = np.full((cnt, p["n_max"] + p["m_max"]), SENTINEL_PERM, dtype=np.int32)
        rc = L.lpx_solve_batch_all(*args, x.ctypes.data_as(_lib.dp), perm.ctypes.data_as(_lib.ip), C.byref(took))
    else:
        rc = L.lpx_solve_batch(*args, C.byref(took))
    assert rc == 0, _lib.last_error()
    return [SolveInfo(res[k], None, None) for k in range(cnt)], took.value, x, perm


def test_one_shot_calls_scatter_interleaved_routes(lps, oracle, arith):
    from linear_programming_solver_amd import _lib
    L = _lib.lib()
    cases = scatter_cases()
    shapes = [(len(case[1]), len(case[2])) for case in cases]
    assert shapes == [(3, 2), (5, 7), (1, 1), (97, 200), (0, 3), (3, 2), (4, 9)]
    assert L.lpx_batch_solve_lds_bytes(96, 200) <= _lib.BATCH_LDS_BYTES < L.lpx_batch_solve_lds_bytes(97, 200)
    assert [needs_phase1(case[1]) for case in cases] == [False, True, False, True, False, True, False]
    assert [case[3] for case in cases] == [True, False, True, False, True, False, True]
    for maximize_given in (True, False):   # NULL flags: every form maximises
        asked = cases if maximize_given else [case[:3] + (True,) for case in cases]
        want = [oracle_solve(oracle, case, "reference") for case in asked]
        res = [r for r, _ in want]
        assert res[1]["phase1_used"] and res[1]["status"] in (OPTIMAL, UNBOUNDED) and res[1]["pivots1"] >= 2
        assert res[3]["phase1_used"] and res[3]["status"] in (OPTIMAL, UNBOUNDED) and res[3]["pivots2"] >= 1
        assert res[5]["status"] == INFEASIBLE and res[5]["final_n"] == 3
        budget = 2 * max(r["pivots1"] + r["pivots2"] for r in res) + 100
        if maximize_given:   # lpx_solve_batch refuses NULL flags: tests/test_batch_host.py
            infos, took, _, _ = one_shot(lps, arith, asked, budget, all_in_kernel=False)
            assert took == 4
            for k, info in enumerate(infos):
                compare_info(info, res[k], "(lpx_solve_batch, form %d)" % k)
        infos, took, x, perm = one_shot(lps, arith, asked, budget, all_in_kernel=True, maximize_given=maximize_given)
        assert took == 6
        for k, (info, (r, st)) in enumerate(zip(infos, want)):
            what = "(lpx_solve_batch_all, maximize %s, form %d)" % ("given" if maximize_given else "NULL", k)
            compare_info(info, r, what)
            m, n = shapes[k]
            if st.n == n:
                _, b, _, _, want_perm = st.read()
                want_x = np.zeros(n)
                for i in range(m):
                    if want_perm[n + i] < n:
                        want_x[want_perm[n + i]] = b[i]
                assert list(perm[k, :n + m]) == list(want_perm), "perm differs " + what
                assert np.array_equal(bits(x[k, :n]), bits(want_x)), "x differs " + what
            else:   # the auxiliary LP of a solve that ended inside phase 1: the caller's rows are left alone
                n = m = 0
            assert np.all(x[k, n:] == SENTINEL_X) and np.all(perm[k, n + m:] == SENTINEL_PERM), "padding written " + what
            st.close()
