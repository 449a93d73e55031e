#!/usr/bin/env python3
"""Batched solve against a loop of lpx_solve: B small LPs in one launch of k_batch_simplex (one workgroup per LP, state in
LDS) versus what a caller could do before — lpx_solve LP by LP — on the same LPs, same GPU, same run.

Shapes: B = 1024 and 8192 LPs of 64 x 64 and B = 1024 of 96 x 160 (dense_lp: A ~ U(0,1), b = (n/4) U(1,2), c ~ U(0,1)),
in both arithmetic modes.  Timed with the host clock around calls that end in a stream synchronise:
  loop         lpx_batch_simplex_loop alone (handle and upload outside the window); best and median of --repeats handles
  solve_batch  lpx_solve_batch end to end (packing into images, upload, launch, read-back, rounding)
  baseline     lpx_solve over the first --baseline-lps LPs one by one, scaled to B
and a sweep of the workgroup size (LPX_BATCH_THREADS) on the plain mode, which is where the by-size rule comes from.

--phase1 runs another measurement instead (default --out profiles/batch_phase1.txt): 4096 forms of 32 x 32 that all need
phase 1 (every third row a >= row with a negative right-hand side, feasible), in both arithmetic modes:
  new          lpx_solve_batch_all: phase 1 inside k_batch_solve, one launch for all forms
  parent       lpx_solve_batch on the first --parent-lps of the same forms: each goes through lpx_solve on its own
  no-phase-1   the dense 32 x 32 forms through k_batch_simplex (lpx_batch_simplex_loop) and through k_batch_solve
and asserts that the new path solves at least 10 times the parent's LPs per second.
Needs a GPU; there is no fallback.  Lines go to stdout and to --out."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from linear_programming_solver_amd import LPBatch, _lib, pack_lps   # noqa: E402

CUS = 256


def dense_lp(m, n, seed):
    rng = np.random.default_rng(seed)
    return rng.random((m, n)), (n / 4.0) * (1.0 + rng.random(m)), rng.random(n)


def launch_info(batch):
    L = _lib.lib()
    fn = L.lpxi_batch_launch_info
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, _lib.ip, _lib.ip, _lib.ip]
    t, lds, per_cu = C.c_int32(), C.c_int32(), C.c_int32()
    if fn(batch._h, C.byref(t), C.byref(lds), C.byref(per_cu)):
        raise RuntimeError(_lib.last_error())
    return t.value, lds.value, per_cu.value


def time_loop(lps, fused, repeats):
    """[(seconds, total pivots)] of lpx_batch_simplex_loop on fresh handles, and the launch's shape."""
    out, info = [], None
    for _ in range(repeats):
        batch = LPBatch(lps, options={"fused": int(fused)})
        info = launch_info(batch)
        t0 = time.perf_counter()
        status, pivots, _ = batch.simplex_loop()
        dt = time.perf_counter() - t0
        assert not status.any(), "every dense LP is optimal"
        out.append((dt, int(pivots.sum())))
        batch.close()
    return out, info


def solve_args(lps, fused):
    p = pack_lps(lps)
    opts = _lib.SolveOptions()
    opts.max_pivots = -1
    opts.fused = 1 if fused else -1
    return p, opts


def time_solve_batch(lps, fused):
    L = _lib.lib()
    p, opts = solve_args(lps, fused)
    res = (_lib.SolveResult * p["count"])()
    maxi = np.ones(p["count"], dtype=np.int32)
    nin = C.c_int32()
    t0 = time.perf_counter()
    rc = L.lpx_solve_batch(p["count"], p["m_max"], p["n_max"], p["m"].ctypes.data_as(_lib.ip), p["n"].ctypes.data_as(_lib.ip),
                           p["A"].ctypes.data_as(_lib.dp), p["lda"], p["strideA"], p["b"].ctypes.data_as(_lib.dp),
                           p["c"].ctypes.data_as(_lib.dp), maxi.ctypes.data_as(_lib.ip), C.byref(opts), res, C.byref(nin))
    dt = time.perf_counter() - t0
    if rc:
        raise RuntimeError(_lib.last_error())
    assert nin.value == p["count"]
    return dt, res


def time_baseline(lps, fused):
    """lpx_solve one by one: seconds, pivots and the objective texts."""
    L = _lib.lib()
    texts, pivots = [], 0
    t0 = time.perf_counter()
    for A, b, c in lps:
        opts = _lib.SolveOptions()
        opts.max_pivots = -1
        opts.fused = 1 if fused else -1
        res = _lib.SolveResult()
        rc = L.lpx_solve(b.size, c.size, A.ctypes.data_as(_lib.dp), c.size, b.ctypes.data_as(_lib.dp),
                         c.ctypes.data_as(_lib.dp), 1, C.byref(opts), C.byref(res))
        if rc:
            raise RuntimeError(_lib.last_error())
        texts.append(res.objective_text)
        pivots += res.pivots_phase2
    return time.perf_counter() - t0, pivots, texts


def feasible_phase1_lp(m, n, s):
    """dense_lp with every third row turned into a >= row that x* = 0.5 U(0,1)^n satisfies (tests/test_gpu_batch_solve.py)."""
    seed = 1000 * m + n + 17 * s
    A, b, c = dense_lp(m, n, seed)
    xs = 0.5 * np.random.default_rng(seed + 77777).random(n)
    for i in range(0, m, 3):
        b[i] = -0.5 * (A[i] @ xs)
        A[i] = -A[i]
    return A, b, c


def solve_launch_info(lps, fused):
    L = _lib.lib()
    fn = L.lpxi_batch_solve_launch_info
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, _lib.ip, _lib.ip, _lib.ip]
    batch = LPBatch(lps, options={"fused": int(fused)})
    t, lds, per_cu = C.c_int32(), C.c_int32(), C.c_int32()
    if fn(batch._h, C.byref(t), C.byref(lds), C.byref(per_cu)):
        raise RuntimeError(_lib.last_error())
    batch.close()
    return t.value, lds.value, per_cu.value


def time_solve_batch_all(lps, fused):
    """(seconds end to end, results, forms the kernel took) of lpx_solve_batch_all with x_out and perm_out."""
    L = _lib.lib()
    p, opts = solve_args(lps, fused)
    res = (_lib.SolveResult * p["count"])()
    maxi = np.ones(p["count"], dtype=np.int32)
    x = np.zeros((p["count"], p["n_max"]))
    perm = np.zeros((p["count"], p["n_max"] + p["m_max"]), dtype=np.int32)
    nin = C.c_int32()
    t0 = time.perf_counter()
    rc = L.lpx_solve_batch_all(p["count"], p["m_max"], p["n_max"], p["m"].ctypes.data_as(_lib.ip),
                               p["n"].ctypes.data_as(_lib.ip), p["A"].ctypes.data_as(_lib.dp), p["lda"], p["strideA"],
                               p["b"].ctypes.data_as(_lib.dp), p["c"].ctypes.data_as(_lib.dp), maxi.ctypes.data_as(_lib.ip),
                               C.byref(opts), res, x.ctypes.data_as(_lib.dp), perm.ctypes.data_as(_lib.ip), C.byref(nin))
    dt = time.perf_counter() - t0
    if rc:
        raise RuntimeError(_lib.last_error())
    return dt, res, nin.value


def time_parent(lps, fused):
    """lpx_solve_batch as it routes phase-1 forms: lpx_solve one by one."""
    L = _lib.lib()
    p, opts = solve_args(lps, fused)
    res = (_lib.SolveResult * p["count"])()
    maxi = np.ones(p["count"], dtype=np.int32)
    nin = C.c_int32()
    t0 = time.perf_counter()
    rc = L.lpx_solve_batch(p["count"], p["m_max"], p["n_max"], p["m"].ctypes.data_as(_lib.ip), p["n"].ctypes.data_as(_lib.ip),
                           p["A"].ctypes.data_as(_lib.dp), p["lda"], p["strideA"], p["b"].ctypes.data_as(_lib.dp),
                           p["c"].ctypes.data_as(_lib.dp), maxi.ctypes.data_as(_lib.ip), C.byref(opts), res, C.byref(nin))
    dt = time.perf_counter() - t0
    if rc:
        raise RuntimeError(_lib.last_error())
    return dt, res, nin.value


def phase1_leg(say, count, parent_lps, repeats, m=32, n=32):
    """Returns the smallest new-over-parent ratio of LPs per second over the arithmetic modes."""
    forms = [feasible_phase1_lp(m, n, s) for s in range(count)]
    dense = [dense_lp(m, n, 9000 + s) for s in range(count)]
    worst = None
    for fused in (False, True):
        mode = "fused" if fused else "plain"
        threads, lds, per_cu = solve_launch_info(forms, fused)
        resident = min(count, max(per_cu, 1) * CUS)
        time_solve_batch_all(forms[:8], fused)                      # warm-up
        runs = [time_solve_batch_all(forms, fused) for _ in range(repeats)]
        dt, res, took = min(runs, key=lambda r: r[0])
        assert took == count, "every form stays in the kernel"
        kern = min(r[1][0].seconds_pivots for r in runs)
        piv = sum(res[k].pivots_phase1 + res[k].pivots_phase2 for k in range(count))
        p1 = sum(res[k].pivots_phase1 for k in range(count))
        say("phase1 %dx%d B=%d %s new: lpx_solve_batch_all end to end %.3f ms = %.0f LPs/s | kernel %.3f ms, %d pivots "
            "(%d in phase 1) = %.3g pivots/s, %.2f us per pivot per workgroup | threads %d lds %d B resident %d per CU (%d at once)"
            % (m, n, count, mode, dt * 1e3, count / dt, kern * 1e3, piv, p1, piv / kern, kern * resident / piv * 1e6, threads,
               lds, per_cu, resident))
        time_parent(forms[:4], fused)                               # warm-up of the one-LP path
        pdt, pres, ptook = time_parent(forms[:parent_lps], fused)
        assert ptook == 0, "the parent takes every phase-1 form out of the batch"
        for k in range(parent_lps):
            assert (pres[k].status, pres[k].objective_text, pres[k].pivots_phase1, pres[k].pivots_phase2) == \
                   (res[k].status, res[k].objective_text, res[k].pivots_phase1, res[k].pivots_phase2), "new and parent disagree"
        ppiv = sum(pres[k].pivots_phase1 + pres[k].pivots_phase2 for k in range(parent_lps))
        ratio = (count / dt) / (parent_lps / pdt)
        say("phase1 %dx%d B=%d %s parent: lpx_solve_batch on the first %d forms %.1f ms = %.0f LPs/s | pivot loops %.1f ms, "
            "%d pivots = %.1f us per pivot | new path %.0fx the parent's LPs/s"
            % (m, n, count, mode, parent_lps, pdt * 1e3, parent_lps / pdt, pres[0].seconds_pivots * 1e3, ppiv,
               pres[0].seconds_pivots / ppiv * 1e6, ratio))
        worst = ratio if worst is None else min(worst, ratio)
        time_loop(dense[:8], fused, 1)
        loops, (t0_, lds0, per_cu0) = time_loop(dense, fused, repeats)
        best, dpiv = min(r[0] for r in loops), loops[0][1]
        res0 = min(count, max(per_cu0, 1) * CUS)
        t1_, lds1, per_cu1 = solve_launch_info(dense, fused)
        res1 = min(count, max(per_cu1, 1) * CUS)
        time_solve_batch_all(dense[:8], fused)
        druns = [time_solve_batch_all(dense, fused) for _ in range(repeats)]
        dkern = min(r[1][0].seconds_pivots for r in druns)
        assert sum(druns[0][1][k].pivots_phase2 for k in range(count)) == dpiv
        say("phase1 %dx%d B=%d %s no-phase-1 forms: k_batch_simplex %.3f ms, %d pivots = %.2f us per pivot per workgroup "
            "(threads %d lds %d B resident %d per CU) | k_batch_solve %.3f ms = %.2f us per pivot per workgroup (threads %d lds %d B "
            "resident %d per CU)"
            % (m, n, count, mode, best * 1e3, dpiv, best * res0 / dpiv * 1e6, t0_, lds0, per_cu0, dkern * 1e3,
               dkern * res1 / dpiv * 1e6, t1_, lds1, per_cu1))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase1", action="store_true", help="the phase-1-in-the-kernel measurement instead (see the docstring)")
    ap.add_argument("--phase1-lps", type=int, default=4096)
    ap.add_argument("--parent-lps", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_first.txt"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-lps", type=int, default=64)
    ap.add_argument("--quick", action="store_true", help="B = 256 of 64 x 64 only (a rehearsal or a profiler run)")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--sweep-only", action="store_true", help="the workgroup-size sweep alone (for a kernel-trace run)")
    args = ap.parse_args()
    L = _lib.lib()
    if L.lpx_device_count() < 1:
        raise SystemExit("bench_batch.py needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.phase1:
        if args.out == ap.get_default("out"):
            args.out = os.path.join(ROOT, "profiles", "batch_phase1.txt")
        ratio = phase1_leg(say, args.phase1_lps, min(args.parent_lps, args.phase1_lps), args.repeats)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        assert ratio >= 10.0, "the new path must solve at least 10x the parent's LPs per second, it solves %.1fx" % ratio
        return

    shapes = [(256, 64, 64)] if args.quick else [(1024, 64, 64), (8192, 64, 64), (1024, 96, 160)]
    if args.sweep_only:
        shapes = []
    cache = {}
    for B, m, n in shapes:
        key = (m, n)
        have = cache.setdefault(key, [])
        while len(have) < B:
            have.append(dense_lp(m, n, 9000 + len(have)))
        lps = have[:B]
        nb = min(args.baseline_lps, B)
        for fused in (False, True):
            mode = "fused" if fused else "plain"
            time_loop(lps[:8], fused, 1)                      # warm-up: code object, first launch of this shape
            runs, (threads, lds, per_cu) = time_loop(lps, fused, args.repeats)
            secs = sorted(r[0] for r in runs)
            best, med, pivots = secs[0], secs[len(secs) // 2], runs[0][1]
            resident = min(B, max(per_cu, 1) * CUS)
            say("batch %dx%d B=%d %s: loop best %.3f ms median %.3f ms | %.0f LPs/s %.3g pivots/s | %d pivots | "
                "%.2f us per pivot per workgroup | threads %d lds %d B resident %d per CU (%d at once)"
                % (m, n, B, mode, best * 1e3, med * 1e3, B / best, pivots / best, pivots, best * resident / pivots * 1e6,
                   threads, lds, per_cu, resident))
            time_solve_batch(lps[:8], fused)
            sb, res = time_solve_batch(lps, fused)
            base_s, base_piv, base_txt = time_baseline(lps[:nb], fused)   # its first solves warm the one-LP path up too:
            base_s, base_piv, base_txt = time_baseline(lps[:nb], fused)   # timed on the second pass
            assert [res[k].objective_text for k in range(nb)] == base_txt, "solve_batch and lpx_solve disagree"
            assert sum(res[k].pivots_phase2 for k in range(nb)) == base_piv
            scaled = base_s * B / nb
            say("batch %dx%d B=%d %s: lpx_solve_batch end to end %.3f ms (%.0f LPs/s) | loop of lpx_solve %.3f ms for %d LPs "
                "= %.1f ms scaled to B (%.0f LPs/s, %.1f us per pivot) | batch loop %.1fx, solve_batch %.1fx the per-LP loop"
                % (m, n, B, mode, sb * 1e3, B / sb, base_s * 1e3, nb, scaled * 1e3, nb / base_s, base_s / base_piv * 1e6,
                   scaled / best, scaled / sb))
    if not args.no_sweep and not args.quick:
        for B, m, n in [(1024, 64, 64), (1024, 96, 160), (4096, 16, 24)]:
            key = (m, n)
            have = cache.setdefault(key, [])
            while len(have) < B:
                have.append(dense_lp(m, n, 9000 + len(have)))
            for threads in (64, 128, 256, 512, 1024):
                os.environ["LPX_BATCH_THREADS"] = str(threads)
                time_loop(have[:8], False, 1)
                runs, (t, lds, per_cu) = time_loop(have[:B], False, args.repeats)
                best = min(r[0] for r in runs)
                say("sweep %dx%d B=%d plain threads %d: loop best %.3f ms | resident %d per CU | %.3g pivots/s"
                    % (m, n, B, t, best * 1e3, per_cu, runs[0][1] / best))
            del os.environ["LPX_BATCH_THREADS"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
