#!/usr/bin/env python3
"""mg3d_wpcg_solve against mg3d_vcycles with all six faces Neumann: python tools/wpcg_bench.py [c,L ...]
(default 9,5 and 9,7: 129^3 and 513^3, V(2,2), sigma = 0, eps = ball x100 -- the singular case)

Per size, from a random guess with d = 0: ms per V-cycle of mg3d_vcycles and ms per iteration (a solve of ITERS
iterations, the initial residual, its projection and the first cycle included, divided by ITERS), each as median and
min .. max over RUNS timed runs after a warm-up; the iterations to 1e-10 of the initial residual; and what 30 plain cycles
do to the residual from the same start.

The vector passes have no entry point of their own: their times come from a kernel trace,
    rocprofv3 --kernel-trace --stats -- python tools/wpcg_bench.py --trace 9,7
(a run of its own that only solves), set against their compulsory bytes per point: apply + dot 24 B with eps,
update + norm 48 B, dot 16 B, direction 24 B."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_U
from pcg_bench import ball_eps, spread

RUNS = int(os.environ.get("RUNS", "5"))
ITERS = int(os.environ.get("ITERS", "10"))


def main():
    argv = sys.argv[1:]
    trace = "--trace" in argv
    if trace:
        argv.remove("--trace")
    sizes = [tuple(int(v) for v in a.split(",")) for a in argv] or [(9, 5), (9, 7)]
    for c, L in sizes:
        with M.Solver(c, L, 2) as s:
            N, top = s.N, L - 1
            s.set_neumann(63)
            s.set_coefficient(ball_eps(N, 100.0))
            s.get_details()
            u0 = np.random.default_rng(5).uniform(-1, 1, N ** 3)

            def solve(iters=ITERS, rtol=0.0):
                s.upload(MG3D_U, top, u0)
                s.sync()
                t0 = time.perf_counter()
                out = s.wpcg_solve(rtol=rtol, atol=1e-300, max_iters=iters)
                solve.t = time.perf_counter() - t0
                return out

            def cycles(n=ITERS):
                s.upload(MG3D_U, top, u0)
                s.sync()
                t0 = time.perf_counter()
                out = s.vcycles(n)
                cycles.t = time.perf_counter() - t0
                return out

            if trace:
                solve()
                solve()
                continue
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
            nc = cycles(30)
            norms, info = solve(60, 1e-10)
            mc, mi = statistics.median(t_cyc), statistics.median(t_it)
            ratios = norms[1:] / norms[:-1]
            print(f"{N}^3 V(2,2), six Neumann faces, eps = ball x100:")
            print(f"  V-cycle         {spread(t_cyc)}")
            print(f"  wPCG iteration  {spread(t_it)}   {mi / mc:.2f} x the cycle")
            print(f"  to 1e-10 of the initial residual: {info['iterations']} iterations = {info['iterations'] * mi * 1e3:.1f} ms "
                  f"(converged {info['converged']}), ratio per iteration {ratios.min():.2f} .. {ratios.max():.2f}")
            print(f"  30 plain cycles: residual / r0 = {nc[-1] / r0:.3g}, last ratio per cycle {nc[-1] / nc[-2]:.3f}", flush=True)


if __name__ == "__main__":
    main()
