#!/usr/bin/env python3
"""mg3d_pcg_solve against mg3d_vcycles: python tools/pcg_bench.py [c,L ...]   (default 9,7: 513^3, V(2,2), sigma = 0)

Per size, for eps = ball x100 (jump inside the ball of radius 1/4) and for the constant operator, from a smooth guess with
d = 0: ms per V-cycle of mg3d_vcycles and ms per PCG iteration (a solve of ITERS iterations, the initial residual and the
first cycle included, divided by ITERS), each as median and min .. max over RUNS timed runs after a warm-up; and how many
cycles / iterations the two need to bring the residual down by 1e-10, hence ms to that tolerance.

The three vector passes of an iteration have no entry point of their own: their times come from a kernel trace,
    rocprofv3 --kernel-trace --stats -- python tools/pcg_bench.py --trace 9,7
(a run of its own that only solves), set against their compulsory bytes per point: apply + dot 16 B (24 B with eps),
update + norm 48 B, dot 16 B, direction 24 B."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_U

RUNS = int(os.environ.get("RUNS", "5"))
ITERS = int(os.environ.get("ITERS", "10"))


def ball_eps(N, jump):
    x = np.linspace(0.0, 1.0, N)
    r2 = (x[:, None, None] - 0.5) ** 2 + (x[None, :, None] - 0.5) ** 2 + (x[None, None, :] - 0.5) ** 2
    return np.where(r2 < 0.0625, jump, 1.0)


def guess(N):
    x = np.sin(np.pi * np.linspace(0.0, 1.0, N))
    y = np.sin(3 * np.pi * np.linspace(0.0, 1.0, N))
    return np.ascontiguousarray(x[:, None, None] * y[None, :, None] * x[None, None, :])


def spread(ts):
    return f"{statistics.median(ts) * 1e3:8.3f} ms (min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f}, {len(ts)} runs)"


def timed(fn, per):
    fn()  # warm-up: first launches, work vectors, chunk tuning
    out = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) / per)
    return out


def main():
    argv = sys.argv[1:]
    trace = "--trace" in argv
    if trace:
        argv.remove("--trace")
    sizes = [tuple(int(v) for v in a.split(",")) for a in argv] or [(9, 7)]
    for c, L in sizes:
        for label, jump in (("eps = ball x100", 100.0), ("constant", None)):
            with M.Solver(c, L, 2) as s:
                N, top = s.N, L - 1
                if jump:
                    s.set_coefficient(ball_eps(N, jump))
                s.get_details()
                u0 = guess(N)

                def solve(iters=ITERS, rtol=0.0):
                    s.upload(MG3D_U, top, u0)
                    s.sync()
                    t0 = time.perf_counter()
                    out = s.pcg_solve(rtol=rtol, atol=1e-300, max_iters=iters)
                    solve.t = time.perf_counter() - t0
                    return out

                if trace:
                    solve()
                    solve()
                    continue

                def cycles(n=ITERS):
                    s.upload(MG3D_U, top, u0)
                    s.sync()
                    t0 = time.perf_counter()
                    out = s.vcycles(n)
                    cycles.t = time.perf_counter() - t0
                    return out

                cycles()
                t_cyc = []
                for _ in range(RUNS):
                    cycles()
                    t_cyc.append(cycles.t / ITERS)
                solve()
                t_it = []
                for _ in range(RUNS):
                    solve()
                    t_it.append(solve.t / ITERS)
                s.upload(MG3D_U, top, u0)
                r0 = s.residual(top, store=False)
                nc = cycles(60)
                below = np.nonzero(nc <= 1e-10 * r0)[0]
                n_cyc = int(below[0]) + 1 if below.size else None
                _, info = solve(60, 1e-10)
                mc, mi = statistics.median(t_cyc), statistics.median(t_it)
                print(f"{N}^3 V(2,2), {label}:")
                print(f"  V-cycle        {spread(t_cyc)}")
                print(f"  PCG iteration  {spread(t_it)}   {mi / mc:.2f} x the cycle")
                print(f"  to 1e-10 of the initial residual: {n_cyc} cycles = {n_cyc * mc * 1e3 if n_cyc else float('nan'):.1f} ms, "
                      f"{info['iterations']} iterations = {info['iterations'] * mi * 1e3:.1f} ms "
                      f"(converged {info['converged']})", flush=True)


if __name__ == "__main__":
    main()
