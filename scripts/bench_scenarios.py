#!/usr/bin/env python3
"""Scenario batches against the replicated-matrix path: --count scenarios (4096) of ONE 32 x 32 constraint matrix, all of
which need phase 1, in both arithmetic modes, same GPU, same run.

The matrix is dense_lp's (A ~ U(0,1)) with every third row negated; scenario k has b = (n/4)(1 + U) on the rows left
alone and b[i] = -0.5 (A_orig[i] . xs_k), xs_k = 0.5 U^n, on the negated ones (feasible, phase 1), c ~ U(0,1), all `max`
(tests/scenario_cases.py, kind (ii)).  Timed with the host clock around calls that end in a stream synchronise:
  (a) one-shot   lpx_solve_scenarios end to end: the matrix up once, b and c as they are, k_batch_scenarios, x / perm / results back
  (b) handle     lpx_scenarios_solve on an existing handle (the matrix is already on the device), end to end
  (c) parent     lpx_solve_batch_all on the same forms with A replicated count times: gather, images, upload, k_batch_solve,
                 the images read back -- three repetitions, for its spread
and the launch times of k_batch_scenarios and k_batch_solve as the library stamps them (seconds_pivots: the host clock
around launch + synchronise).  Asserts that (a) and (c) agree scenario by scenario on status, objective text, both pivot
counts and the bits of x and perm, and that (a) is faster than (c).  Needs a GPU; there is no fallback.  Lines go to
stdout and to --out."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from linear_programming_solver_amd import LPScenarios, _lib   # noqa: E402


def scenarios(m, n, count):
    """(A, b[count, m], c[count, n]): one matrix, every scenario of kind (ii)."""
    seed = 1000 * m + n
    A_orig = np.random.default_rng(seed).random((m, n))
    A = A_orig.copy()
    A[0::3] = -A[0::3]
    rng = np.random.default_rng(seed + 4242)
    b = (n / 4.0) * (1.0 + rng.random((count, m)))
    xs = 0.5 * rng.random((count, n))
    b[:, 0::3] = -0.5 * (xs @ A_orig[0::3].T)
    return A, b, rng.random((count, n))


def options(fused):
    opts = _lib.SolveOptions()
    opts.max_pivots = -1
    opts.fused = 1 if fused else -1
    opts.restore_order_len = -1
    return opts


def outputs(count, m, n):
    return (_lib.SolveResult * count)(), np.zeros((count, n)), np.zeros((count, n + m), dtype=np.int32)


def one_shot(A, b, c, fused):
    """(a): (seconds, results, x, perm)"""
    (m, n), count = A.shape, b.shape[0]
    res, x, perm = outputs(count, m, n)
    opts = options(fused)
    t0 = time.perf_counter()
    rc = _lib.lib().lpx_solve_scenarios(m, n, A.ctypes.data_as(_lib.dp), n, count, b.ctypes.data_as(_lib.dp), m,
                                        c.ctypes.data_as(_lib.dp), n, None, C.byref(opts), res, x.ctypes.data_as(_lib.dp),
                                        perm.ctypes.data_as(_lib.ip))
    dt = time.perf_counter() - t0
    if rc:
        raise RuntimeError(_lib.last_error())
    return dt, res, x, perm


def on_handle(handle, b, c):
    """(b): (seconds, results, x, perm)"""
    m, n, count = handle.m, handle.n, b.shape[0]
    res, x, perm = outputs(count, m, n)
    t0 = time.perf_counter()
    rc = handle._L.lpx_scenarios_solve(handle._h, count, b.ctypes.data_as(_lib.dp), m, c.ctypes.data_as(_lib.dp), n, None, -1,
                                       None, -1, res, x.ctypes.data_as(_lib.dp), perm.ctypes.data_as(_lib.ip))
    dt = time.perf_counter() - t0
    if rc:
        raise RuntimeError(_lib.last_error())
    return dt, res, x, perm


def parent(A_rep, b, c, fused):
    """(c): (seconds, results, x, perm) of lpx_solve_batch_all on A replicated (A_rep[count, m, n], built outside the window)"""
    count, m, n = A_rep.shape
    res, x, perm = outputs(count, m, n)
    opts = options(fused)
    took = C.c_int32()
    t0 = time.perf_counter()
    rc = _lib.lib().lpx_solve_batch_all(count, m, n, None, None, A_rep.ctypes.data_as(_lib.dp), n, m * n,
                                        b.ctypes.data_as(_lib.dp), c.ctypes.data_as(_lib.dp), None, C.byref(opts), res,
                                        x.ctypes.data_as(_lib.dp), perm.ctypes.data_as(_lib.ip), C.byref(took))
    dt = time.perf_counter() - t0
    if rc:
        raise RuntimeError(_lib.last_error())
    assert took.value == count, "every form stays in the kernel"
    return dt, res, x, perm


def launch_info(handle):
    fn = handle._L.lpxi_scenarios_launch_info
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32, _lib.ip, _lib.ip, _lib.ip]
    t, lds, per_cu = C.c_int32(), C.c_int32(), C.c_int32()
    if fn(handle._h, 1, C.byref(t), C.byref(lds), C.byref(per_cu)):
        raise RuntimeError(_lib.last_error())
    return t.value, lds.value, per_cu.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=4096)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_scenarios.txt"))
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    m, n, count = args.m, args.n, args.count
    A, b, c = scenarios(m, n, count)
    assert (b.min(axis=1) < 0).all(), "every scenario needs phase 1"
    A_rep = np.ascontiguousarray(np.broadcast_to(A, (count, m, n)))
    say("scenario batch: %d scenarios of one %d x %d matrix, all with phase 1; per scenario %d B up and %d B down against "
        "%d B of image each way on the replicated path" % (count, m, n, 8 * (m + n) + 4, 8 * n + 4 * (n + m) + 40,
                                                           8 * (m * (n | 1) + m + n + 2) + 4 * (n + m)))
    worst = None
    for fused in (False, True):
        mode = "fused" if fused else "plain"
        one_shot(A, b[:8], c[:8], fused)                               # warm-up of both paths
        parent(A_rep[:8], b[:8], c[:8], fused)
        a_runs = [one_shot(A, b, c, fused) for _ in range(args.repeats)]
        handle = LPScenarios(A, options={"fused": int(fused)})
        threads, lds, per_cu = launch_info(handle)
        on_handle(handle, b[:8], c[:8])
        b_runs = [on_handle(handle, b, c) for _ in range(args.repeats)]
        handle.close()
        c_runs = [parent(A_rep, b, c, fused) for _ in range(3)]
        ta, res_a, x_a, perm_a = min(a_runs, key=lambda r: r[0])
        tb = min(r[0] for r in b_runs)
        tcs = sorted(r[0] for r in c_runs)
        _, res_c, x_c, perm_c = c_runs[0]
        for k in range(count):
            ra, rc_ = res_a[k], res_c[k]
            assert (ra.status, ra.objective_text, ra.pivots_phase1, ra.pivots_phase2) == \
                   (rc_.status, rc_.objective_text, rc_.pivots_phase1, rc_.pivots_phase2), "scenario %d: the two paths disagree" % k
        assert x_a.tobytes() == x_c.tobytes() and perm_a.tobytes() == perm_c.tobytes(), "x or perm differ"
        for _, res_b, x_b, perm_b in b_runs:
            assert x_b.tobytes() == x_a.tobytes() and perm_b.tobytes() == perm_a.tobytes(), "the handle's x or perm differ"
        piv = sum(res_a[k].pivots_phase1 + res_a[k].pivots_phase2 for k in range(count))
        optimal = sum(res_a[k].status == 0 for k in range(count))
        ka = sorted(r[1][0].seconds_pivots for r in a_runs + b_runs)
        kc = sorted(r[1][0].seconds_pivots for r in c_runs)
        ratio = tcs[0] / ta
        say("%s (a) lpx_solve_scenarios end to end %.3f ms = %.0f LPs/s (all %d runs: %s ms)"
            % (mode, ta * 1e3, count / ta, len(a_runs), ", ".join("%.3f" % (r[0] * 1e3) for r in a_runs)))
        say("%s (b) lpx_scenarios_solve on a handle end to end %.3f ms = %.0f LPs/s (all %d runs: %s ms)"
            % (mode, tb * 1e3, count / tb, len(b_runs), ", ".join("%.3f" % (r[0] * 1e3) for r in b_runs)))
        say("%s (c) lpx_solve_batch_all, A replicated, end to end %.3f ms = %.0f LPs/s (three runs: %s ms, spread %.3f ms)"
            % (mode, tcs[0] * 1e3, count / tcs[0], ", ".join("%.3f" % (t * 1e3) for t in tcs), (tcs[-1] - tcs[0]) * 1e3))
        say("%s launch: k_batch_scenarios %.3f ms (of %d: %s) | k_batch_solve %.3f ms (of 3: %s, spread %.3f ms) | %d pivots, "
            "%d of %d optimal | threads %d lds %d B resident %d per CU"
            % (mode, ka[0] * 1e3, len(ka), ", ".join("%.3f" % (t * 1e3) for t in ka), kc[0] * 1e3,
               ", ".join("%.3f" % (t * 1e3) for t in kc), (kc[-1] - kc[0]) * 1e3, piv, optimal, count, threads, lds, per_cu))
        say("%s (a) is %.1fx (c); (b) is %.1fx (c); bits of x and perm, statuses, objective texts and pivot counts agree" % (mode, ratio, tcs[0] / tb))
        worst = ratio if worst is None else min(worst, ratio)
    assert worst > 1.0, "lpx_solve_scenarios is not faster than lpx_solve_batch_all on the replicated forms: %.2fx" % worst
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
