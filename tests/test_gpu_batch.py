"""GPU parity of the batched solve (k_batch_simplex through lpx_batch / LPBatch / LPSolver.solve_batch): many small LPs
in one launch, one workgroup per LP, against the oracle on the same inputs.

The bar for every test: A, b, c, v, perm bit for bit, pivot count and status, for EVERY LP of the batch, in both
arithmetic modes (oracle.FP64 is the instantiation of the mode the test runs in).  Each test also asserts, from the
oracle's own results, that its inputs contain what it claims to cover."""
from decimal import Decimal

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPTIMAL, UNBOUNDED, PIVOT_LIMIT = 0, 1, 9


@pytest.fixture(scope="module")
def lps(arith):
    """The host package; every test of this module runs in both arithmetic modes (tests/conftest.py `arith`)."""
    from tests.conftest import package_in_mode
    pkg = package_in_mode(arith)
    yield pkg
    pkg.set_default_arithmetic("auto")


@pytest.fixture(scope="module")
def oracle(arith):
    """The checker of the current mode: oracle.FP64 is the fp64 instantiation ("plain") or the fused one ("fused")."""
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
    assert gA.shape == wA.shape, "shape differs " + what
    assert np.array_equal(bits(gA), bits(wA)), "A differs " + what
    assert np.array_equal(bits(gb), bits(wb)), "b differs " + what
    assert np.array_equal(bits(gc), bits(wc)), "c differs " + what
    assert bits(np.array([gv]))[0] == bits(np.array([wv]))[0], "v differs %s: %r vs %r" % (what, gv, wv)
    assert list(gp) == list(wp), "perm differs " + what


def dense_lp(m, n, seed):
    """SURVEY §8(d) synthetic input: A ~ U(0,1), b = (n/4) U(1,2), c ~ U(0,1), maximise."""
    rng = np.random.default_rng(seed)
    return rng.random((m, n)), (n / 4.0) * (1.0 + rng.random(m)), rng.random(n)


def oracle_loop(oracle, lp, kind=None, max_pivots=-1, pricing=0, want_trace=False):
    """(final oracle State, result dict of its simplex loop) for one (A, b, c)."""
    st = oracle.State(lp[0], lp[1], lp[2], kind=oracle.FP64 if kind is None else kind, pricing=pricing)
    return st, st.simplex_loop(max_pivots, want_trace=want_trace)


def run_and_compare(lps, oracle, lp_list, pricing="reference", options=None, kind=None):
    """Solve lp_list as ONE batch and compare every LP with the oracle.  Returns the oracle's (status, pivots) lists."""
    batch = lps.LPBatch(lp_list, pricing=pricing, options=options)
    status, pivots, _ = batch.simplex_loop()
    want_status, want_pivots = [], []
    for k, lp in enumerate(lp_list):
        ref, r = oracle_loop(oracle, lp, kind=kind, pricing=1 if pricing == "dantzig" else 0)
        what = "(LP %d, %d x %d)" % (k, ref.m, ref.n)
        assert status[k] == r["status"], "status differs " + what
        assert pivots[k] == r["pivots"], "pivot count differs " + what
        assert_state_bits_equal(batch.read(k), ref.read(), what)
        want_status.append(r["status"])
        want_pivots.append(r["pivots"])
        ref.close()
    batch.close()
    return want_status, want_pivots


# ------------------------------------------------------------------------------------ 1. edge shapes
def test_edge_shapes_in_one_batch(lps, oracle, reference_vectors):
    groups = [g for g in reference_vectors["pivot"] if (len(g["b"]), len(g["c"])) in ((4, 5), (7, 2))]
    assert sorted((len(g["b"]), len(g["c"])) for g in groups) == [(4, 5), (7, 2)]
    lp_list = [
        (np.zeros((0, 3)), [], [-1.0, 2.0, 0.5]),       # no rows, a positive c: unbounded at once
        (np.zeros((0, 3)), [], [-1.0, 0.0, 1e-10]),     # no rows, nothing above 1e-9: optimal, 0 pivots
        (np.zeros((3, 0)), [1.0, 2.0, 3.0], []),        # no columns
        ([[2.0]], [4.0], [3.0]),                        # 1 x 1
    ] + [(g["A"], g["b"], g["c"]) for g in groups]      # the reference's pivot-vector shapes, run as loops
    status, pivots = run_and_compare(lps, oracle, lp_list)
    assert (status[0], pivots[0]) == (UNBOUNDED, 0)
    assert (status[1], pivots[1]) == (OPTIMAL, 0)
    assert (status[2], pivots[2]) == (OPTIMAL, 0)
    assert (status[3], pivots[3]) == (OPTIMAL, 1)
    assert pivots[4] >= 1 and pivots[5] >= 1


# ------------------------------------------------------------------------------------ 2. thread-count boundaries
def test_thread_count_boundaries_in_one_batch(lps, oracle):
    shapes = [(5, 63), (5, 64), (5, 65), (63, 5), (65, 5), (70, 130), (33, 257)]
    lp_list = [dense_lp(m, n, 100 + k) for k, (m, n) in enumerate(shapes)]
    status, pivots = run_and_compare(lps, oracle, lp_list)
    assert all(s == OPTIMAL for s in status) and all(p >= 2 for p in pivots), (status, pivots)
    # the same shapes one by one: every LP then runs at the workgroup size of its own shape
    for lp in lp_list:
        run_and_compare(lps, oracle, [lp])


# ------------------------------------------------------------------------------------ 3. largest fit and one past it
def test_largest_fit_and_one_past_it(lps, oracle):
    from linear_programming_solver_amd import _lib
    L = _lib.lib()
    m = 1
    while L.lpx_batch_lds_bytes(m + 1, 200) <= _lib.BATCH_LDS_BYTES:
        m += 1
    assert L.lpx_batch_lds_bytes(m, 200) <= _lib.BATCH_LDS_BYTES < L.lpx_batch_lds_bytes(m + 1, 200)
    status, pivots = run_and_compare(lps, oracle, [dense_lp(m, 200, 31), dense_lp(3, 4, 32)])
    assert status == [OPTIMAL, OPTIMAL] and pivots[0] >= m // 2
    with pytest.raises(ValueError) as ei:                        # LPX_BAD_ARGUMENT
        lps.LPBatch([dense_lp(3, 4, 32), dense_lp(m + 1, 200, 33)])
    assert "LP 1" in str(ei.value) and "%d x 200" % (m + 1) in str(ei.value)


# ------------------------------------------------------------------------------------ 4. more LPs than are resident
def test_more_lps_than_are_resident(lps, oracle):
    lp_list = [dense_lp(8, 12, 1000 + k) for k in range(3000)]
    status, pivots = run_and_compare(lps, oracle, lp_list)
    assert all(s == OPTIMAL for s in status) and len(set(pivots)) > 3


def test_more_64x64_lps_than_the_lds_holds(lps, oracle):
    """Four 64 x 64 LPs fill the LDS of a CU, so 256 CUs hold 1024 at a time: 1100 need a second round of workgroups."""
    from linear_programming_solver_amd import _lib
    assert 5 * _lib.lib().lpx_batch_lds_bytes(64, 64) > _lib.BATCH_LDS_BYTES
    lp_list = [dense_lp(64, 64, 5000 + k) for k in range(1100)]
    status, pivots = run_and_compare(lps, oracle, lp_list)
    assert all(s == OPTIMAL for s in status) and min(pivots) >= 2


# ------------------------------------------------------------------------------------ 5. ties and statuses
def tie_lp(seed):
    """Integer-valued LP whose rows 6..11 repeat rows 0..5: every minimum ratio is shared by two rows."""
    rng = np.random.default_rng(seed)
    A = rng.integers(1, 6, size=(6, 9)).astype(np.float64)
    b = rng.integers(4, 9, size=6).astype(np.float64) * 4.0
    return np.vstack([A, A]), np.concatenate([b, b]), rng.integers(1, 5, size=9).astype(np.float64)


def unbounded_lp(seed):
    A, b, c = dense_lp(9, 7, seed)
    A[:, 2] = -A[:, 2]                                   # column 2 <= 0 under c[2] > 0
    return A, b, c


def shared_minimum_steps(oracle, lp, pricing):
    """Replays the oracle pivot by pivot; returns how many ratio tests had their minimum on several rows, asserting
    that the LOWEST of those rows left every time."""
    st = oracle.State(lp[0], lp[1], lp[2], kind=oracle.FP64, pricing=pricing)
    shared = 0
    while True:
        e = st.get_entering()
        if e == -1:
            break
        l = st.get_leaving(e)
        if l == -1:
            break
        A, b, _, _, _ = st.read()
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(A[:, e] < 1e-9, 1e50, b / A[:, e])
        rows = np.flatnonzero(ratio == ratio.min())
        assert l == rows[0]
        shared += len(rows) > 1
        st.pivot(e, l)
    st.close()
    return shared


@pytest.mark.parametrize("pricing", ["reference", "dantzig"])
def test_ties_and_statuses_inside_one_batch(lps, oracle, pricing):
    lp_list = [tie_lp(7), dense_lp(9, 7, 41), unbounded_lp(42), dense_lp(7, 9, 43), tie_lp(8)]
    assert shared_minimum_steps(oracle, lp_list[0], 1 if pricing == "dantzig" else 0) >= 1
    status, pivots = run_and_compare(lps, oracle, lp_list, pricing=pricing)
    assert status == [OPTIMAL, OPTIMAL, UNBOUNDED, OPTIMAL, OPTIMAL], status
    assert pivots[0] >= 1 and pivots[1] >= 1 and pivots[3] >= 1


def test_dantzig_leaves_the_reference_pivot_sequence(oracle):
    """The Dantzig case above is a different check from the reference-rule case: the two rules give different traces."""
    lp = dense_lp(7, 9, 43)
    _, a = oracle_loop(oracle, lp, pricing=0, want_trace=True)
    _, d = oracle_loop(oracle, lp, pricing=1, want_trace=True)
    assert a["trace"].tolist() != d["trace"].tolist()


# ------------------------------------------------------------------------------------ 6. budget and resume
def replay_tracking(trace, n, slot):
    for e, l in trace:                                   # the three-line rule of the loop (LPSolver.java:151-155)
        if e == slot:
            slot = l + n
        elif l + n == slot:
            slot = e
    return slot


def test_budget_and_resume(lps, oracle):
    m, n, budget = 24, 40, 7
    lp_list = []
    for k in range(16):
        A, b, c = dense_lp(m, n, 200 + k)
        if k % 4 == 1:
            c[2:] = -c[2:]                               # two improving columns only: a short solve
        lp_list.append((A, b, c))
    full = [oracle_loop(oracle, lp, want_trace=True) for lp in lp_list]
    assert all(r["status"] == OPTIMAL for _, r in full)
    need = [r["pivots"] for _, r in full]
    assert any(p > budget for p in need) and any(p <= budget for p in need), need
    assert any(replay_tracking(r["trace"], n, 0) != 0 for _, r in full)       # slot 0 does move somewhere

    batch = lps.LPBatch(lp_list)
    status, pivots, track = batch.simplex_loop(budget, track_slots=np.zeros(16, dtype=np.int32))
    for k, lp in enumerate(lp_list):
        assert status[k] == (PIVOT_LIMIT if need[k] > budget else OPTIMAL), k
        assert pivots[k] == min(need[k], budget), k
        assert track[k] == replay_tracking(full[k][1]["trace"][:budget], n, 0), k
        part, r = oracle_loop(oracle, lp, max_pivots=budget)
        assert r["status"] == status[k]
        assert_state_bits_equal(batch.read(k), part.read(), "(LP %d after %d pivots)" % (k, budget))
        part.close()
    status2, pivots2, track2 = batch.simplex_loop(-1, track_slots=track)
    for k in range(16):
        assert status2[k] == OPTIMAL and pivots[k] + pivots2[k] == need[k], k
        assert track2[k] == replay_tracking(full[k][1]["trace"], n, 0), k
        assert_state_bits_equal(batch.read(k), full[k][0].read(), "(LP %d resumed)" % k)
        full[k][0].close()
    batch.close()


# ------------------------------------------------------------------------------------ 7. solve_batch
def test_solve_batch_matches_solve_form_by_form(lps, oracle, reference_vectors):
    cases = [(c["A"], c["b"], c["c"], c["maximize"]) for c in reference_vectors["solve"]]
    assert {c["status"] for c in reference_vectors["solve"]} == {"OPTIMAL", "UNBOUNDED", "INFEASIBLE"}
    assert {c["maximize"] for c in reference_vectors["solve"]} == {True, False}
    cases += [dense_lp(32, 48, 300 + k) + (k % 2 == 0,) for k in range(8)]
    forms = [lps.LPStandardForm(A, b, c, maximize=mx) for A, b, c, mx in cases]
    solver = lps.LPSolver()
    answers = solver.solve_batch(forms)
    assert len(answers) == len(forms) == len(solver.last_batch)
    no_phase1 = sum(1 for _, b, _, _ in cases if min(b) >= 0)
    assert solver.last_batch_in_kernel == no_phase1 and 0 < no_phase1 < len(forms)
    kinds = set()
    for k, (form, (A, b, c, mx)) in enumerate(zip(forms, cases)):
        alone = lps.LPSolver()
        try:
            want = alone.solve(form)
        except Exception as exc:
            want = exc
        got, info = answers[k], solver.last_batch[k]
        if isinstance(want, Exception):
            assert type(got) is type(want) and str(got) == str(want), (k, got, want)
        else:
            assert isinstance(got, Decimal) and got == want, (k, got, want)
        kinds.add(type(want).__name__)
        res, st = oracle.solve(A, b, c, mx, kind=oracle.FP64, want_trace=False)
        st.close()
        for mine in (info, alone.last):
            assert mine.status == res["status"], k
            assert mine.phase1_used == res["phase1_used"], k
            assert (mine.pivots_phase1, mine.pivots_phase2) == (res["pivots1"], res["pivots2"]), k
            assert mine.x0_slot == res["x0_slot"], k
            assert mine.objective_text == res["objective_text"], k
            assert bits(np.array([mine.objective]))[0] == bits(np.array([res["objective"]]))[0], k
    assert kinds == {"Decimal", "SolutionException", "LPException"}


# ------------------------------------------------------------------------------------ 8. mode separation
def test_the_two_arithmetic_modes_stay_apart(lps, oracle):
    lp = dense_lp(48, 64, 77)
    from oracle import pyoracle
    plain, rp = oracle_loop(oracle, lp, kind=pyoracle.FP64)
    fused, rf = oracle_loop(oracle, lp, kind=pyoracle.FP64_FUSED)
    pA, fA = plain.read()[0], fused.read()[0]
    assert pA.shape != fA.shape or not np.array_equal(bits(pA), bits(fA)) or rp["pivots"] != rf["pivots"]
    plain.close()
    fused.close()
    run_and_compare(lps, oracle, [lp], options={"fused": 0}, kind=pyoracle.FP64)
    run_and_compare(lps, oracle, [lp], options={"fused": 1}, kind=pyoracle.FP64_FUSED)
