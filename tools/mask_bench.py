#!/usr/bin/env python3
"""Embedded conductors (mg3d_ctx_set_mask) against the same context without them: python tools/mask_bench.py [c,L ...]
(default 9,7: 513^3, V(2,2), all-Dirichlet, the reference's test problem with a sphere of radius 0.2 held at 1).

Per operator (constant; eps = 1 + 1/2 sin(2 pi x) cos(pi y)): ms per cycle of mg3d_vcycles -- every one of REPEATS timed
runs is printed, so the run-to-run spread is on the page -- for
    fused      the context without a mask (constant operator only: its fused schedules)
    no mask    the unfused kernels without a mask (eps: the context as it is; constant: not reachable, see zero mask)
    zero mask  an all-zero mask: the MASK kernels, every byte read, nothing skipped -- the unfused twin of the next line
    sphere     the sphere fixed
and inside the cycle the finest level's kernel timers per launch (colour pass, residual, prolongation)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_U

CYCLES = int(os.environ.get("CYCLES", "10"))
REPEATS = int(os.environ.get("REPEATS", "5"))


def smooth_eps(N):
    x = np.linspace(0.0, 1.0, N)
    return np.ascontiguousarray(np.broadcast_to(1.0 + 0.5 * np.sin(2 * np.pi * x)[:, None, None] * np.cos(np.pi * x)[None, :, None],
                                                (N, N, N)))


def sphere(N, radius=0.2):
    x = np.linspace(0.0, 1.0, N)
    r2 = (x[:, None, None] - 0.5) ** 2 + (x[None, :, None] - 0.5) ** 2 + (x[None, None, :] - 0.5) ** 2
    return (r2 <= radius * radius).astype(np.uint8)


def measure(s, top, label):
    s.vcycles(3)
    runs = []
    for _ in range(REPEATS):
        s.sync()
        t0 = time.perf_counter()
        s.vcycles(CYCLES)
        runs.append((time.perf_counter() - t0) / CYCLES * 1e3)
    s.timing_enable(3)
    s.timing_reset()
    s.vcycles(CYCLES)
    s.sync()
    kt = s.kernel_times()
    s.timing_enable(0)
    per = {k: secs / calls * 1e3 for (l, k), (calls, secs) in kt.items() if l == top}
    print(f"  {label:10s} ms per cycle: " + " ".join(f"{r:7.3f}" for r in runs) + f"   min {min(runs):7.3f} max {max(runs):7.3f}")
    print("             finest level, ms per launch: " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(per.items())), flush=True)
    return min(runs)


def main():
    sizes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or [(9, 7)]
    for c, L in sizes:
        with M.Solver(c, L, 2) as s:
            N, top = s.N, L - 1
            ball = sphere(N)
            print(f"{N}^3 V(2,2), {int(ball.sum())} fixed points in the sphere, {CYCLES} cycles per timed run")
            for name, eps in (("constant", None), ("eps", smooth_eps(N))):
                print(f" {name} operator")
                s.set_mask(None)
                s.set_coefficient(eps)

                def start(with_body):
                    s.setup_test_problem()
                    if with_body:
                        u = np.zeros((N, N, N))
                        s.L.mg3d_fill_boundary_host(u.ctypes.data_as(M.binding.dp), N, s.h)
                        u[ball != 0] = 1.0
                        s.upload(MG3D_U, top, u)

                start(False)
                base = measure(s, top, "fused" if eps is None else "no mask")
                s.set_mask(np.zeros(N ** 3, dtype=np.uint8))
                start(False)
                zero = measure(s, top, "zero mask")
                s.set_mask(ball)
                start(True)
                body = measure(s, top, "sphere")
                print(f"  sphere / zero mask {body / zero:.3f}, zero mask / {'fused' if eps is None else 'no mask'} {zero / base:.3f}", flush=True)


if __name__ == "__main__":
    main()
