#!/usr/bin/env python3
"""Neumann faces (mg3d_ctx_set_neumann) against the Dirichlet kernels on the same box: python tools/neumann_bench.py
[c,L ...] (default 9,7: 513^3, V(2,2), sigma = 0, eps = 1 + 1/2 sin(2 pi x) cos(pi y) where a coefficient is set).

Contexts per size: the constant operator run launch by launch (MG3D_NO_FUSE=1 at creation: k_smooth_color / k_residual,
k_restrict, k_prolong), the coefficient operator (the same launchers with eps), the same two with all six faces Neumann,
and all three axes periodic (constant) for its cycle and coarse solve.  Per context: the finest level's colour pass and
residual as single launches (mg3d_smooth / mg3d_residual, kernel timers), the finest level's restriction and prolongation
and level 0's direct solve inside a cycle (kernel timers of every level), and ms per cycle (mg3d_vcycles, best of three
timed runs).  Bandwidth as in tools/periodic_bench.py: compulsory bytes over kernel time, points N^3.  A library without
mg3d_ctx_set_neumann (an older commit, for the same-box comparison) runs the Dirichlet contexts only."""
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
    return secs / calls if calls else float("nan")


def make(c, L, no_fuse):
    if no_fuse:
        os.environ["MG3D_NO_FUSE"] = "1"
    try:
        return M.Solver(c, L, 2)
    finally:
        os.environ.pop("MG3D_NO_FUSE", None)


def main():
    sizes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or [(9, 7)]
    have = hasattr(M.Solver, "set_neumann")
    for c, L in sizes:
        N = (c - 1) * (1 << (L - 1)) + 1
        top, pts = L - 1, float(N) ** 3
        eps = smooth_eps(N)
        rng = np.random.default_rng(1)
        u = rng.standard_normal((N, N, N)) * 1e-3
        d = np.zeros((N, N, N))  # compatible: the singular problems are consistent
        print(f"{N}^3 V(2,2), finest level single launches, transfers and cycle time", flush=True)
        contexts = [("constant, MG3D_NO_FUSE=1", True, 0, 0, False), ("coefficient", False, 0, 0, True)]
        if have:
            contexts += [("neumann 63, constant", False, 0, 63, False), ("neumann 63, coefficient", False, 0, 63, True),
                         ("periodic 7, constant", False, 7, 0, False)]
        for name, no_fuse, axes, faces, coef in contexts:
            with make(c, L, no_fuse) as s:
                s.set_periodic(axes)
                if faces:
                    s.set_neumann(faces)
                if coef:
                    s.set_coefficient(eps)
                s.get_details()
                s.upload(MG3D_U, top, u)
                s.upload(MG3D_D, top, d)
                b_col, b_res = (32, 24) if coef else (24, 16)
                t_col = per_launch(s, top, lambda: s.smooth(top, 0, 1), "colour_pass")
                t_rs = per_launch(s, top, lambda: s.residual(top, store=True, want_norm=False), "residual")
                t_rn = per_launch(s, top, lambda: s.residual(top, store=False, want_norm=False), "residual")
                t_rt = per_launch(s, top, lambda: s.vcycles(1), "restrict", mode=1)
                t_pr = per_launch(s, top, lambda: s.vcycles(1), "prolong", mode=1)
                t_lu = per_launch(s, 0, lambda: s.vcycles(1), "coarse_solve", mode=1)
                ms = cycle_ms(s)
                print(f"  {name:26s} colour {t_col * 1e3:.4f} ms {b_col * pts / t_col / 1e12:.2f} TB/s | residual+r "
                      f"{t_rs * 1e3:.4f} ms {(b_res + 8) * pts / t_rs / 1e12:.2f} TB/s | norm only {t_rn * 1e3:.4f} ms "
                      f"{b_res * pts / t_rn / 1e12:.2f} TB/s | restrict {t_rt * 1e3:.4f} ms | prolong {t_pr * 1e3:.4f} ms | "
                      f"coarse solve {t_lu * 1e3:.3f} ms | cycle {ms:.3f} ms", flush=True)


if __name__ == "__main__":
    main()
