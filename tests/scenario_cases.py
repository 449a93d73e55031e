"""Inputs of the scenario-batch tests (tests/test_scenarios_host.py, tests/test_gpu_scenarios.py): generators only.

A launch is a dict: A (m x n), b (count x m), c (count x n), maximize (count bools).  Every launch shares ONE matrix: the
dense_lp matrix (A ~ U(0,1)) with every third row negated, as feasible_phase1_lp of tests/test_gpu_batch_solve.py builds
it; the scenarios differ in b, c and the max | min flag:
  (i)    b = (n/4)(1 + U) > 0: no phase 1
  (ii)   as (i), but on the negated rows b[i] = -0.5 (A_orig[i] . xs_k) with xs_k = 0.5 U^n per scenario: phase 1, feasible
  (iii)  as (i), but one negated row gets b = -1e6: phase 1, infeasible (for m >= 2: the rows left positive bound x)
  (iv)   c ~ U(-1, 1) and `min` flags mixed in
column_launch uses a second matrix, one column of which is -|U|: a positive cost there is unbounded."""
import numpy as np

# the smallest shapes that cross what the kernel can get wrong: the pitch change n -> n + 1, the 64-column chunk edges,
# the row groups, one-wave and many-wave workgroups
SHAPES = [(1, 1), (2, 1), (1, 3), (5, 63), (5, 64), (5, 65), (63, 5), (65, 5), (33, 130), (24, 40)]
BIG_SHAPE = (96, 200)   # the largest phase-1 fit with 200 columns: more than 64 KiB of dynamic LDS


def seed_of(m, n, s):
    return 1000 * m + n + 17 * s


def matrix(m, n, s=0):
    """(A, A_orig): U(0,1)^(m x n) and the same with rows 0, 3, 6, ... negated."""
    A_orig = np.random.default_rng(seed_of(m, n, s)).random((m, n))
    A = A_orig.copy()
    A[0::3] = -A[0::3]
    return A, A_orig


def positive_b(rng, m, n):
    return (n / 4.0) * (1.0 + rng.random(m))


def feasible_b(rng, A_orig):
    m, n = A_orig.shape
    b = positive_b(rng, m, n)
    xs = 0.5 * rng.random(n)
    for i in range(0, m, 3):
        b[i] = -0.5 * (A_orig[i] @ xs)
    return b


def infeasible_b(rng, A_orig, k):
    m, n = A_orig.shape
    b = positive_b(rng, m, n)
    negated = list(range(0, m, 3))
    b[negated[k % len(negated)]] = -1e6
    return b


def mixed_launch(m, n, count=12, s=0):
    """Kinds (i), (ii), (iii) in turn, costs U(0,1), all `max`."""
    A, A_orig = matrix(m, n, s)
    rng = np.random.default_rng(seed_of(m, n, s) + 4242)
    b = np.zeros((count, m))
    for k in range(count):
        b[k] = (positive_b(rng, m, n), feasible_b(rng, A_orig), infeasible_b(rng, A_orig, k))[k % 3]
    return {"A": A, "b": b, "c": rng.random((count, n)), "maximize": [True] * count}


def signed_cost_launch(m, n, count=12, s=0):
    """Kind (iv): c ~ U(-1, 1), every other scenario a `min`; b of kinds (i) and (ii) in turn (two of each flag)."""
    A, A_orig = matrix(m, n, s)
    rng = np.random.default_rng(seed_of(m, n, s) + 9191)
    b = np.zeros((count, m))
    for k in range(count):
        b[k] = feasible_b(rng, A_orig) if (k // 2) % 2 else positive_b(rng, m, n)
    return {"A": A, "b": b, "c": rng.uniform(-1.0, 1.0, (count, n)), "maximize": [k % 2 == 0 for k in range(count)]}


def column_launch(m, n, count=8, s=0):
    """A ~ U(0,1) but column n // 2 = -|U|, b > 0, c ~ U(0,1) except on that column: 0.5 for even k -- unbounded, nothing
    ever blocks the column -- and -1000 for odd k -- not unbounded: raising that variable relaxes every row, but any
    other variable would have to gain more than 1000 times what it lets through."""
    rng = np.random.default_rng(seed_of(m, n, s) + 555)
    A = rng.random((m, n))
    j0 = n // 2
    A[:, j0] = -np.abs(rng.random(m))
    b = np.stack([positive_b(rng, m, n) for _ in range(count)])
    c = rng.random((count, n))
    c[:, j0] = [0.5 if k % 2 == 0 else -1000.0 for k in range(count)]
    return {"A": A, "b": b, "c": c, "maximize": [True] * count}


def big_launch():
    """96 x 200 with 3 scenarios: kinds (i), (ii), (i)."""
    m, n = BIG_SHAPE
    A, A_orig = matrix(m, n)
    rng = np.random.default_rng(seed_of(m, n, 0) + 31)
    b = np.stack([positive_b(rng, m, n), feasible_b(rng, A_orig), positive_b(rng, m, n)])
    return {"A": A, "b": b, "c": rng.random((3, n)), "maximize": [True, True, True]}


def launches():
    """(name, launch) of every launch the GPU parity test solves."""
    out = []
    for (m, n) in SHAPES:
        out.append(("mixed %dx%d" % (m, n), mixed_launch(m, n)))
    for (m, n) in [(5, 65), (24, 40), (63, 5)]:
        out.append(("signed %dx%d" % (m, n), signed_cost_launch(m, n)))
    for (m, n) in [(5, 65), (24, 40)]:
        out.append(("column %dx%d" % (m, n), column_launch(m, n)))
    out.append(("big 96x200", big_launch()))
    return out
