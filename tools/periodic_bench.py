#!/usr/bin/env python3
"""Periodic boundaries (mg3d_ctx_set_periodic) against the Dirichlet kernels on the same box: python tools/periodic_bench.py
[c,L ...] (default 9,7: 513^3, V(2,2), sigma = 0, eps = 1 + 1/2 sin(2 pi x) cos(pi y) where a coefficient is set).

Four contexts per size: the constant operator run launch by launch (MG3D_NO_FUSE=1 at creation: k_smooth_color /
k_residual), the coefficient operator (the same launchers with eps), and the periodic kernels with all three axes
periodic, constant and with eps.  Per context: the finest level's colour pass and residual as single launches (mg3d_smooth / mg3d_residual, kernel
timers), ms per cycle (mg3d_vcycles, best of three timed runs), and -- periodic only -- the coarse direct solve inside the
cycle (kernel timers of level 0; at c = 9 the wide band takes lu_solve_block_kernel).  Bandwidth is compulsory bytes
over kernel time: a colour pass reads v and d (and eps) and writes v (24 / 32 B per point), the residual reads v and d
(and eps) (16 / 24 B) and writes r (+8 B) when it stores it; points are N^3."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U

CYCLES = int(os.environ.get("CYCLES", "10"))


def smooth_eps(N):
    x = np.linspace(0.0, 1.0, N)
    return np.ascontiguousarray(np.broadcast_to(1.0 + 0.5 * np.sin(2 * np.pi * x)[:, None, None] * np.cos(np.pi * x)[None, :, None],
                                                (N, N, N)))


def cycle_ms(s):
    s.vcycles(2)
    best = 1e9
    for _ in range(3):
        s.sync()
        t0 = time.perf_counter()
        s.vcycles(CYCLES)
        best = min(best, (time.perf_counter() - t0) / CYCLES)
    return best * 1e3


def per_launch(s, level, fn, kernel, mode=3):
    fn()
    s.timing_enable(mode)
    s.timing_reset()
    for _ in range(10):
        fn()
    s.sync()
    calls, secs = s.kernel_times().get((level, kernel), (0, 0.0))
    s.timing_enable(0)
    return secs / calls if calls else float("nan"), calls


def make(c, L, no_fuse):
    if no_fuse:
        os.environ["MG3D_NO_FUSE"] = "1"
    try:
        return M.Solver(c, L, 2)
    finally:
        os.environ.pop("MG3D_NO_FUSE", None)


def main():
    sizes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or [(9, 7)]
    for c, L in sizes:
        N = (c - 1) * (1 << (L - 1)) + 1
        top, pts = L - 1, float(N) ** 3
        eps = smooth_eps(N)
        rng = np.random.default_rng(1)
        u = rng.standard_normal((N, N, N)) * 1e-3
        d = np.zeros((N, N, N))  # zero mean: the singular all-periodic problem is consistent
        print(f"{N}^3 V(2,2), finest level single launches and cycle time", flush=True)
        for name, no_fuse, axes, coef in (("constant, MG3D_NO_FUSE=1", True, 0, False), ("coefficient", False, 0, True),
                                          ("periodic 7, constant", False, 7, False), ("periodic 7, coefficient", False, 7, True)):
            with make(c, L, no_fuse) as s:
                s.set_periodic(axes)
                if coef:
                    s.set_coefficient(eps)
                s.get_details()
                s.upload(MG3D_U, top, u)
                s.upload(MG3D_D, top, d)
                b_col, b_res = (32, 24) if coef else (24, 16)
                t_col, _ = per_launch(s, top, lambda: s.smooth(top, 0, 1), "colour_pass")
                t_rs, _ = per_launch(s, top, lambda: s.residual(top, store=True, want_norm=False), "residual")
                t_rn, _ = per_launch(s, top, lambda: s.residual(top, store=False, want_norm=False), "residual")
                ms = cycle_ms(s)
                line = (f"  {name:26s} colour {t_col * 1e3:.4f} ms {b_col * pts / t_col / 1e12:.2f} TB/s | residual+r "
                        f"{t_rs * 1e3:.4f} ms {(b_res + 8) * pts / t_rs / 1e12:.2f} TB/s | norm only {t_rn * 1e3:.4f} ms "
                        f"{b_res * pts / t_rn / 1e12:.2f} TB/s | cycle {ms:.3f} ms")
                if axes:
                    t_lu, n_lu = per_launch(s, 0, lambda: s.vcycles(1), "coarse_solve", mode=1)
                    line += f" | coarse solve {t_lu * 1e3:.3f} ms"
                print(line, flush=True)


if __name__ == "__main__":
    main()
