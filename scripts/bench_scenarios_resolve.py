#!/usr/bin/env python3
"""Re-solve from a shared basis against the cold scenario solve: --count scenarios (4096) of ONE 32 x 32 constraint matrix,
each the base case with its right-hand side off by up to 5 %, in both arithmetic modes, same GPU, same process, same handle.

The matrix is dense_lp's (A ~ U(0,1)) with every third row negated; the base case has b0 = (n/4)(1 + U) > 0 and c0 ~ U(0,1),
scenario k has b = b0 (1 + 0.05 U(-1,1)) and c = c0, all `max`.  The basis is the perm[n:] of the base case as the handle
itself solves it.  Timed with the host clock around calls that end in a stream synchronise:
  (cold)     lpx_scenarios_solve on the handle: every scenario from the slack basis, k_batch_scenarios
  (resolve)  lpx_scenarios_resolve on the same handle and the same scenarios: k_batch_resolve from the basis, plus the cold
             launch for the scenarios it routes cold
and the launch times as the library stamps them (seconds_pivots: the host clock around launch + synchronise).  Asserts that
the two agree scenario by scenario on status and, where optimal, on the optimum to 1e-9 max(1, |objective|) -- the
project's objective criterion between arithmetic modes: the two paths take different pivot sequences, so bits differ --
and that the resolve launch is faster than the cold launch; no ratio is fixed in advance.  Needs a GPU; there is no
fallback.  Lines go to stdout and to --out."""
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
    """(A, b0, c0, b[count, m]): one matrix, the base case and its perturbed right-hand sides."""
    seed = 1000 * m + n
    A = np.random.default_rng(seed).random((m, n))
    A[0::3] = -A[0::3]
    rng = np.random.default_rng(seed + 777)
    b0 = (n / 4.0) * (1.0 + rng.random(m))
    c0 = rng.random(n)
    return A, b0, c0, b0 * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, (count, m)))


def call(handle, name, b, c0):
    """(seconds, results, x, perm, route) of lpx_scenarios_solve or lpx_scenarios_resolve; c0 is shared (pitch 0)"""
    m, n, count = handle.m, handle.n, b.shape[0]
    res = (_lib.SolveResult * count)()
    x, perm, route = np.zeros((count, n)), np.zeros((count, n + m), dtype=np.int32), np.zeros(count, dtype=np.int32)
    args = [handle._h, count, b.ctypes.data_as(_lib.dp), m, c0.ctypes.data_as(_lib.dp), 0, None, -1, None, -1, res,
            x.ctypes.data_as(_lib.dp), perm.ctypes.data_as(_lib.ip)]
    if name == "lpx_scenarios_resolve":
        args.append(route.ctypes.data_as(_lib.ip))
    t0 = time.perf_counter()
    rc = getattr(handle._L, name)(*args)
    dt = time.perf_counter() - t0
    if rc:
        raise RuntimeError(_lib.last_error())
    return dt, res, x, perm, route


def launch_info(handle):
    fn = handle._L.lpxi_scenarios_resolve_launch_info
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, _lib.ip, _lib.ip, _lib.ip, _lib.ip]
    t, lds, per_cu, etas = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    if fn(handle._h, C.byref(t), C.byref(lds), C.byref(per_cu), C.byref(etas)):
        raise RuntimeError(_lib.last_error())
    return t.value, lds.value, per_cu.value, etas.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=4096)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_scenarios_resolve.txt"))
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    m, n, count = args.m, args.n, args.count
    A, b0, c0, b = scenarios(m, n, count)
    say("re-solve from a shared basis: %d scenarios of one %d x %d matrix, b = base (1 +- 5 %%), c = base; basis = the base "
        "case's final perm[n:]" % (count, m, n))
    worst = None
    for fused in (False, True):
        mode = "fused" if fused else "plain"
        handle = LPScenarios(A, options={"fused": int(fused)})
        base = handle.solve(b0, c0)[0]
        assert base.status == 0, "the base case is not optimal"
        t0 = time.perf_counter()
        crash = handle.set_basis(base.perm[n:])
        t_crash = time.perf_counter() - t0
        threads, lds, per_cu, etas = launch_info(handle)
        for name in ("lpx_scenarios_solve", "lpx_scenarios_resolve"):      # warm-up of both paths, buffers at full size
            call(handle, name, b, c0)
        cold_runs = [call(handle, "lpx_scenarios_solve", b, c0) for _ in range(args.repeats)]
        warm_runs = [call(handle, "lpx_scenarios_resolve", b, c0) for _ in range(args.repeats)]
        handle.close()
        _, res_c, _, _, _ = cold_runs[0]
        _, res_w, _, _, route = warm_runs[0]
        for k in range(count):
            rc_, rw = res_c[k], res_w[k]
            assert rc_.status == rw.status, "scenario %d: status %d cold, %d from the basis" % (k, rc_.status, rw.status)
            if rc_.status == 0:
                assert abs(rc_.objective - rw.objective) <= 1e-9 * max(1.0, abs(rc_.objective)), \
                    "scenario %d: optimum %r cold, %r from the basis" % (k, rc_.objective, rw.objective)
        routes = [int((route == r).sum()) for r in (0, 1, 2)]
        piv_c = sum(res_c[k].pivots_phase1 + res_c[k].pivots_phase2 for k in range(count))
        piv_w = sum(res_w[k].pivots_phase1 + res_w[k].pivots_phase2 for k in range(count))
        piv_dual = sum(res_w[k].pivots_phase1 for k in range(count) if route[k] == 2)
        optimal = sum(res_c[k].status == 0 for k in range(count))
        kc = sorted(r[1][0].seconds_pivots for r in cold_runs)
        kw = sorted(r[1][0].seconds_pivots for r in warm_runs)
        tc = sorted(r[0] for r in cold_runs)
        tw = sorted(r[0] for r in warm_runs)
        say("%s basis: %d crash pivots = %d eta entries of %d B, set_basis %.3f ms | threads %d lds %d B resident %d per CU"
            % (mode, crash, etas, 8 * (m + n + 4), t_crash * 1e3, threads, lds, per_cu))
        say("%s routes: %d cold, %d primal, %d dual | pivots: %d cold solve, %d from the basis (%d of them in the dual loop; "
            "cold-routed scenarios counted with their cold pivots) | %d of %d optimal, statuses and optima agree"
            % (mode, routes[0], routes[1], routes[2], piv_c, piv_w, piv_dual, optimal, count))
        say("%s launch: cold %.3f ms (of %d: %s) | from the basis %.3f ms (of %d: %s)"
            % (mode, kc[0] * 1e3, len(kc), ", ".join("%.3f" % (t * 1e3) for t in kc), kw[0] * 1e3, len(kw),
               ", ".join("%.3f" % (t * 1e3) for t in kw)))
        say("%s end to end: lpx_scenarios_solve %.3f ms (of %d: %s) | lpx_scenarios_resolve %.3f ms (of %d: %s)"
            % (mode, tc[0] * 1e3, len(tc), ", ".join("%.3f" % (t * 1e3) for t in tc), tw[0] * 1e3, len(tw),
               ", ".join("%.3f" % (t * 1e3) for t in tw)))
        ratio = kc[0] / kw[0]
        say("%s the launch from the basis is %.2fx the cold launch; end to end %.2fx" % (mode, ratio, tc[0] / tw[0]))
        worst = ratio if worst is None else min(worst, ratio)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert worst > 1.0, "the launch from the basis is not faster than the cold launch: %.2fx" % worst


if __name__ == "__main__":
    main()
