"""Inputs and CPU model of the re-solve tests (tests/test_resolve_host.py, tests/test_gpu_resolve.py): generators and the
model only, no test of its own.

A case is a dict: A (m x n), base (b0, c0) -- the base case whose final basis the scenarios start from --, and the
scenarios b (count x m), c (count x n), maximize (count bools).  The matrices are those of tests/scenario_cases.py; the
base case has b0 = positive_b and costs U(0,1); scenario k is the base with
  k % 4 = 0 or 3   b off by up to 5 %
  k % 4 = 1        c off by up to 5 %
  k % 4 = 2        both
  k = 12 (m >= 2)  b[1] = -1e6: row 1 is not negated, so nothing satisfies it -- infeasible, found by the dual loop
  k = 5, 10        a `min` with c negated (the same LP, through the other flag)
column_case uses column_launch's matrix: the base prices the negative column at -1000, the scenarios at 0.5 -- the basis
stays primal feasible, the cost is improving and nothing blocks the column: UNBOUNDED on the primal route.

model_resolve is lpx_scenarios_set_basis + lpx_scenarios_resolve for ONE scenario out of existing oracle calls: the crash
rule, the route and the dual loop are numpy decisions on State.read(), every pivot is State.pivot and the primal loop is
State.simplex_loop, so the arithmetic is the oracle's in the mode under test."""
import numpy as np

from tests import scenario_cases as sc

BIG_SHAPE = (98, 200)   # the largest shape that fits the LDS at all: more than 64 KiB of dynamic LDS, no room for phase 1
SHAPES = sc.SHAPES + [BIG_SHAPE]
OPTIMAL, UNBOUNDED, INFEASIBLE, PIVOT_LIMIT = 0, 1, 2, 9
EPS, INF = 1e-9, 1e50
BUDGET_SHAPE, BUDGET = (33, 130), 1   # the budgeted case: some dual loop and some primal loop need more than one pivot


def count_of(m, n):
    return 4 if (m, n) == BIG_SHAPE else 16


def perturbed(rng, base):
    return base * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, base.shape))


def case(m, n):
    A, _ = sc.matrix(m, n)
    rng = np.random.default_rng(sc.seed_of(m, n, 0) + 777)
    b0, c0 = sc.positive_b(rng, m, n), rng.random(n)
    count = count_of(m, n)
    b, c = np.tile(b0, (count, 1)), np.tile(c0, (count, 1))
    maximize = [True] * count
    for k in range(count):
        if k % 4 != 1:
            b[k] = perturbed(rng, b0)
        if k % 4 in (1, 2):
            c[k] = perturbed(rng, c0)
        if k == 12 and m >= 2:
            b[k, 1] = -1e6
        if k in (5, 10):
            c[k] = -c[k]
            maximize[k] = False
    return {"A": A, "base": (b0, c0), "b": b, "c": c, "maximize": maximize}


def column_case(m, n):
    L = sc.column_launch(m, n)
    assert L["c"][1, n // 2] == -1000.0 and L["c"][0, n // 2] == 0.5
    base_c = L["c"][1]
    c = np.tile(base_c, (4, 1))
    c[:, n // 2] = 0.5
    return {"A": L["A"], "base": (L["b"][1], base_c), "b": np.tile(L["b"][1], (4, 1)), "c": c, "maximize": [True] * 4}


def cases():
    """(name, case) of every case the GPU parity test solves."""
    out = [("%dx%d" % (m, n), case(m, n)) for (m, n) in SHAPES]
    out += [("column %dx%d" % (m, n), column_case(m, n)) for (m, n) in [(5, 65), (24, 40)]]
    return out


def singular_case():
    """5 x 6 with columns 1 and 4 equal, both wanted (with slacks 8, 9, 10): the second finds only zeros to pivot on."""
    A = np.random.default_rng(99).random((5, 6)) + 0.5
    A[:, 4] = A[:, 1]
    return A, [1, 4, 8, 9, 10]


def base_basis(oracle, C, pricing="reference"):
    """perm[n:] of the solved base case (always a max), in the oracle's mode."""
    b0, c0 = C["base"]
    n = C["A"].shape[1]
    _, st = oracle.solve(C["A"], b0, c0, True, kind=oracle.FP64, want_trace=False, pricing=1 if pricing == "dantzig" else 0)
    perm = st.read()[4]
    st.close()
    return [int(v) for v in perm[n:]]


def min_in_b(b):
    """LPSolver.minInB (LPSolver.java:375-386): the first index of the strict minimum from 1e50, -1 if none."""
    mn, idx = INF, -1
    for i, x in enumerate(b):
        if mn > x:
            mn, idx = x, i
    return idx


class SingularBasis(Exception):
    pass


def crash(st, basis):
    """The crash rule of k_scenarios_crash on the oracle state; returns the pivots it took."""
    m, n = st.m, st.n
    wanted = np.zeros(n + m, dtype=bool)
    wanted[list(basis)] = True
    took = 0
    for j in range(n):
        A, _, _, _, perm = st.read()
        if not wanted[perm[j]]:
            continue
        size = np.abs(A[:, j])
        ok = ~wanted[perm[n:]] & (size > EPS)          # a NaN compares false
        if not ok.any():
            raise SingularBasis(int(perm[j]))
        l = int(np.argmax(np.where(ok, size, -1.0)))   # the first maximum: the lowest row
        assert st.pivot(j, l) == 0
        took += 1
    return took


def solution_of(st):
    A, b, c, v, perm = st.read()
    n = st.n
    x = np.zeros(n)
    for i in range(st.m):
        if perm[n + i] < n:
            x[perm[n + i]] = b[i]
    return v, np.asarray(perm, dtype=np.int32), x


def model_resolve(oracle, A, b, c, maximize, basis, budget=-1, pricing="reference"):
    """What lpx_scenarios_resolve answers for ONE scenario from `basis`: a dict with route ("cold" | "primal" | "dual"),
    crash (pivots of the crash), b_basis (b at the basis) and, for a warm route, status, pivots1 (dual loop), pivots2
    (primal loop), objective, objective_text, perm and x; for "cold" the oracle's own solve under `cold`."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    dantzig = 1 if pricing == "dantzig" else 0
    st = oracle.State(A, b, np.asarray(c) if maximize else -np.asarray(c), kind=oracle.FP64, pricing=dantzig)
    try:
        out = {"crash": crash(st, basis)}
        _, bb, cc, _, _ = st.read()
        out["b_basis"] = bb.copy()
        mib = min_in_b(bb)
        needs_dual = mib != -1 and bb[mib] < 0.0
        if needs_dual and bool((cc > EPS).any()):
            out["route"] = "cold"
            r, cold = oracle.solve(A, b, c, maximize, kind=oracle.FP64, max_pivots=budget, want_trace=False, pricing=dantzig)
            cold.close()
            out["cold"] = r
            return out
        out["route"] = "dual" if needs_dual else "primal"
        status, p1, p2 = OPTIMAL, 0, 0
        while needs_dual:
            Ac, bc, ccur, _, _ = st.read()
            l = min_in_b(bc)
            if l == -1 or not bc[l] < -EPS:
                break
            e, best = -1, INF
            for j in np.flatnonzero(Ac[l] < -EPS):
                r = ccur[j] / Ac[l, j]          # numpy's fp64 division is the IEEE one
                if r < best:
                    e, best = int(j), r
            if e < 0:
                status = INFEASIBLE
                break
            if 0 <= budget <= p1:
                status = PIVOT_LIMIT
                break
            assert st.pivot(e, l) == 0
            p1 += 1
        if status == OPTIMAL:
            got = st.simplex_loop(max_pivots=-1 if budget < 0 else max(0, budget - p1))
            status, p2 = got["status"], got["pivots"]
        v, perm, x = solution_of(st)
        objective = v if maximize else -v
        out.update(status=status, pivots1=p1, pivots2=p2, objective=objective,
                   objective_text=oracle.round6_double(objective), perm=perm, x=x)
        return out
    finally:
        st.close()


def model_case(oracle, C, basis, budget=-1, pricing="reference"):
    return [model_resolve(oracle, C["A"], C["b"][k], C["c"][k], C["maximize"][k], basis, budget, pricing)
            for k in range(len(C["maximize"]))]


def pivots_of(w):
    return w["cold"]["pivots1"] + w["cold"]["pivots2"] if w["route"] == "cold" else w["pivots1"] + w["pivots2"]


def budget_above(want):
    return 2 * max(pivots_of(w) for w in want) + 100
