#!/usr/bin/env python3
"""mg3d_step_advance against the time loop a caller had to write before it: python tools/step_bench.py [c,L,eps ...]
(default 9,7,0 and 9,6,1: 513^3 with the constant operator and 257^3 with eps = ball x100, Dirichlet faces, V(2,2)).

Per case, dt = 1e-3, from a smooth u0, STEPS steps per timed run, RUNS runs after a warm-up, median (min .. max):
  new   ms per step of step_advance(STEPS, cycles=2), for theta = 1 (backward Euler) and theta = 0.5 (Crank-Nicolson)
  rhs   ms per launch of the right-hand-side kernel of either theta, and of mg3d_wpcg_solve's apply + dot (its fold
        included) at the same size, from the library's per-kernel event pairs (timing mode 3), in a run of their own: the
        markers cost idle queue time and stay out of the step timings
  old   the same backward-Euler steps through download / numpy (d = -u/dt at the unknowns) / upload / vcycles(2), in the
        same process
and old / new.  The theta < 1 kernel is the apply walk with one more operand: more than 1.5 x the apply launch is flagged."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U

RUNS = int(os.environ.get("RUNS", "5"))
STEPS = int(os.environ.get("STEPS", "20"))
DT = 1e-3


def ball_eps(N, jump):
    x = np.linspace(0.0, 1.0, N)
    r2 = (x[:, None, None] - 0.5) ** 2 + (x[None, :, None] - 0.5) ** 2 + (x[None, None, :] - 0.5) ** 2
    return np.where(r2 < 0.0625, jump, 1.0)


def guess(N):
    x = np.sin(np.pi * np.linspace(0.0, 1.0, N))
    return np.ascontiguousarray(x[:, None, None] * x[None, :, None] * x[None, None, :])


def spread(ts):
    return f"{statistics.median(ts) * 1e3:9.3f} ms (min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f}, {len(ts)} runs)"


def timed(fn, per):
    fn()  # warm-up: first launches, chunk tuning
    out = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) / per)
    return out


def kernel_ms(s, name):
    calls, secs = s.kernel_times().get((s.num_levels - 1, name), (0, 0.0))
    return secs / calls * 1e3 if calls else float("nan"), calls


def main():
    cases = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or [(9, 7, 0), (9, 6, 1)]
    for c, L, coef in cases:
        with M.Solver(c, L, 2) as s:
            N, top = s.N, L - 1
            if coef:
                s.set_coefficient(ball_eps(N, 100.0))
            s.get_details()
            u0 = guess(N)
            print(f"{N}^3 V(2,2), {'eps = ball x100' if coef else 'constant'}, Dirichlet faces, dt = {DT}, "
                  f"{STEPS} steps per run:")
            new = {}
            for theta in (1.0, 0.5):
                s.step_setup(DT, theta)
                s.upload(MG3D_U, top, u0)
                new[theta] = timed(lambda: (s.step_advance(STEPS, cycles=2), s.sync()), STEPS)
                print(f"  new  theta = {theta}: step_advance(cycles=2)     {spread(new[theta])} per step")
            # the kernels, under the event pairs
            rhs = {}
            for theta in (1.0, 0.5):
                s.step_setup(DT, theta)
                s.upload(MG3D_U, top, u0)
                s.step_advance(2, cycles=1)
                s.timing_enable(3)
                s.timing_reset()
                s.step_advance(10, cycles=1)
                rhs[theta], calls = kernel_ms(s, "step_rhs")
                s.timing_enable(0)
                print(f"  rhs  theta = {theta}: right-hand-side kernel     {rhs[theta]:9.4f} ms per launch ({calls} launches)")
            s.upload(MG3D_U, top, u0)
            s.wpcg_solve(rtol=0.0, atol=1e-300, max_iters=1)
            s.timing_enable(3)
            s.timing_reset()
            s.upload(MG3D_U, top, u0)
            s.wpcg_solve(rtol=0.0, atol=1e-300, max_iters=5)
            apply_ms, calls = kernel_ms(s, "pcg_apply")
            s.timing_enable(0)
            ratio = rhs[0.5] / apply_ms
            print(f"  rhs  wpcg_solve's apply + dot (+ fold)           {apply_ms:9.4f} ms per launch ({calls} launches); "
                  f"theta = 0.5 kernel / apply = {ratio:.2f}" + ("   ** above 1.5 **" if ratio > 1.5 else ""))
            # the loop a caller had before: backward Euler, d = -u/dt on the host
            s.step_setup(DT, 1.0)
            s.upload(MG3D_U, top, u0)
            inner = (slice(1, -1),) * 3
            d = np.zeros((N, N, N))

            def old():
                for _ in range(STEPS):
                    u = s.download(MG3D_U, top).reshape(N, N, N)
                    d[inner] = -(u[inner] / DT)
                    s.upload(MG3D_D, top, d)
                    s.vcycles(2)

            t_old = timed(old, STEPS)
            mo, mn = statistics.median(t_old), statistics.median(new[1.0])
            print(f"  old  download / numpy / upload / vcycles(2)      {spread(t_old)} per step")
            print(f"  old / new (theta = 1) = {mo / mn:.1f}", flush=True)


if __name__ == "__main__":
    main()
