#!/usr/bin/env python3
"""The variable-coefficient V-cycle (mg3d_ctx_set_coefficient) against the constant one: python tools/coef_bench.py [c,L ...]
(default 9,6 and 9,7: 257^3 and 513^3, V(2,2), eps = 1 + 1/2 sin(2 pi x) cos(pi y), sigma = 0).

python tools/coef_bench.py --slabs [--ranks 2,4,8] [c,L ...]: ms per coefficient cycle on i-slabs (mg3d_dist_set_coefficient)
through the loopback transport -- the single domain, then P virtual ranks on this one GPU.  Loopback serialises every rank
on one device: the numbers measure the halo planes' extra work and the extra launches, not multi-GPU speed.

Per size: ms per cycle with and without the coefficient (mg3d_vcycles, best of three timed runs); the finest level's
colour pass and residual as single launches (mg3d_smooth / mg3d_residual, HIP events around them on the library's
stream); and inside the cycle, the finest level's kernel timers (MG3D_K_COLOUR_PASS, MG3D_K_RESIDUAL).  Bandwidth is
compulsory bytes over kernel time, at cache-line granularity: a colour pass reads v, eps and d and writes v's lines
(32 B per point), the residual reads v, eps and d (24 B per point) and writes r (+8 B) when it stores it."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_parallel_amd as M

TARGET_TBS = 3.8
CYCLES = int(os.environ.get("CYCLES", "20"))


def smooth_eps(N):
    x = np.linspace(0.0, 1.0, N)
    return np.ascontiguousarray(np.broadcast_to(1.0 + 0.5 * np.sin(2 * np.pi * x)[:, None, None] * np.cos(np.pi * x)[None, :, None],
                                                (N, N, N)))


def cycle_ms(s):
    s.vcycles(3)
    best = 1e9
    for _ in range(3):
        s.sync()
        t0 = time.perf_counter()
        s.vcycles(CYCLES)
        best = min(best, (time.perf_counter() - t0) / CYCLES)
    return best * 1e3


def per_launch(s, top, fn, kernel):
    """mean seconds of one launch of `kernel` on the finest level over the calls of fn (kernel timers, finest level)"""
    fn()
    s.timing_enable(3)
    s.timing_reset()
    for _ in range(10):
        fn()
    s.sync()
    calls, secs = s.kernel_times().get((top, kernel), (0, 0.0))
    s.timing_enable(0)
    return secs / calls if calls else float("nan"), calls


def tbs(bytes_, secs):
    return bytes_ / secs / 1e12


def slab_table(sizes, ranks):
    """ms per coefficient cycle: single domain, then loopback P ranks; the norms must agree with the single domain's"""
    print(f"{'size':>6s} {'single':>9s} " + " ".join(f"{'P=' + str(p):>9s}" for p in ranks) + "   (ms per V(2,2) cycle, eps set)")
    for c, L in sizes:
        N = (c - 1) * (1 << (L - 1)) + 1
        eps = smooth_eps(N)
        with M.Solver(c, L, 2) as s:
            s.set_coefficient(eps)
            s.setup_test_problem()
            row = [cycle_ms(s)]
            s.setup_test_problem()
            ref = s.vcycles(4)
        for P in ranks:
            with M.DistSolver(c, L, 2, nranks=P) as d:
                d.set_coefficient(eps)
                d.setup_test_problem()
                got = d.vcycles(4)
                assert np.allclose(got, ref, rtol=1e-11, atol=0), (P, got, ref)
                row.append(cycle_ms(d))
        print(f"{N:>4d}^3 " + " ".join(f"{t:9.3f}" for t in row), flush=True)


def main():
    argv = sys.argv[1:]
    if "--slabs" in argv:
        argv.remove("--slabs")
        ranks = [2, 4, 8]
        if "--ranks" in argv:
            i = argv.index("--ranks")
            ranks = [int(v) for v in argv[i + 1].split(",")]
            del argv[i:i + 2]
        slab_table([tuple(int(v) for v in a.split(",")) for a in argv] or [(9, 6), (9, 7)], ranks)
        return
    sizes = [tuple(int(v) for v in a.split(",")) for a in argv] or [(9, 6), (9, 7)]
    for c, L in sizes:
        with M.Solver(c, L, 2) as s:
            N, top = s.N, L - 1
            pts = float(N) ** 3
            s.setup_test_problem()
            plain = cycle_ms(s)
            s.set_coefficient(smooth_eps(N))
            s.setup_test_problem()
            coef = cycle_ms(s)
            t_col, _ = per_launch(s, top, lambda: s.smooth(top, 0, 1), "colour_pass")
            t_rs, _ = per_launch(s, top, lambda: s.residual(top, store=True, want_norm=False), "residual")
            t_rn, _ = per_launch(s, top, lambda: s.residual(top, store=False, want_norm=False), "residual")
            s.setup_test_problem()
            c_col, n_col = per_launch(s, top, lambda: s.vcycles(1), "colour_pass")
            c_res, n_res = per_launch(s, top, lambda: s.vcycles(1), "residual")
            print(f"{N}^3 V(2,2): {plain:.3f} ms per cycle constant, {coef:.3f} ms with the coefficient ({coef / plain:.2f}x)")
            print(f"  single launches on the finest level (target {TARGET_TBS} TB/s of compulsory bytes):")
            print(f"    colour pass          {t_col * 1e3:.4f} ms  {tbs(32 * pts, t_col):.2f} TB/s (32 B/point)")
            print(f"    residual, r stored   {t_rs * 1e3:.4f} ms  {tbs(32 * pts, t_rs):.2f} TB/s (32 B/point)")
            print(f"    residual, norm only  {t_rn * 1e3:.4f} ms  {tbs(24 * pts, t_rn):.2f} TB/s (24 B/point)")
            print(f"  inside the cycle (finest level, {n_col // 10} colour passes and {n_res // 10} residuals per cycle):")
            print(f"    colour pass          {c_col * 1e3:.4f} ms  {tbs(32 * pts, c_col):.2f} TB/s")
            print(f"    residual (mean)      {c_res * 1e3:.4f} ms  {tbs(28 * pts, c_res):.2f} TB/s (28 B/point: one stores r, one not)",
                  flush=True)


if __name__ == "__main__":
    main()
