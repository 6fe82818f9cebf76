#!/usr/bin/env python3
"""mg3d_fmg_solve and its interpolation kernel: python tools/fmg_bench.py [c,L ...]   (default 9,7 and 9,6: 513^3, 257^3)

Per size, constant operator, V(2,2):
  - the interpolation into the finest level (mg3d_fmg_interpolate) next to the prolongation of the same level
    (mg3d_prolong: the launch a cycle runs when the prolongation is not folded into a sweep), each as BATCH calls enqueued
    back to back and one synchronisation, median and min .. max over RUNS batches after a warm-up; their ratio, and the
    interpolation's compulsory bytes (N^3 doubles written, (N+1)^3/8 read) over its time;
  - mg3d_fmg_solve(1) as a multiple of one cycle of mg3d_vcycles(ITERS), in the same process."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U

RUNS = int(os.environ.get("RUNS", "7"))
BATCH = int(os.environ.get("BATCH", "20"))
ITERS = int(os.environ.get("ITERS", "10"))


def spread(ts):
    return f"{statistics.median(ts) * 1e3:8.3f} ms (min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f}, {len(ts)} runs)"


def batches(s, call):
    out = []
    for r in range(RUNS + 1):
        s.sync()
        t0 = time.perf_counter()
        for _ in range(BATCH):
            call()
        s.sync()
        if r:  # (the first batch is the warm-up)
            out.append((time.perf_counter() - t0) / BATCH)
    return out


def main():
    sizes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or [(9, 7), (9, 6)]
    for c, L in sizes:
        with M.Solver(c, L, 2) as s:
            N, top = s.N, L - 1
            s.get_details()
            rng = np.random.default_rng(N)
            s.upload(MG3D_U, top - 1, rng.standard_normal(s.level_n(top - 1) ** 3))
            t_int = batches(s, lambda: s.fmg_interpolate(top))
            s.zero(MG3D_U, top)
            t_pro = batches(s, lambda: s.prolong(top))
            mi, mp = statistics.median(t_int), statistics.median(t_pro)
            gb = 8.0 * (N ** 3 + s.level_n(top - 1) ** 3) / 1e9
            print(f"{N}^3:")
            print(f"  fmg_interpolate {spread(t_int)}   {gb / mi:.0f} GB/s of compulsory traffic")
            print(f"  prolong         {spread(t_pro)}   interpolation / prolongation = {mi / mp:.2f}")
            x = np.sin(np.pi * np.linspace(0.0, 1.0, N))
            d = np.ascontiguousarray(x[:, None, None] * x[None, :, None] * x[None, None, :])
            u0 = np.zeros(N ** 3)
            s.upload(MG3D_D, top, d)

            def run(fn, per):
                ts = []
                for r in range(RUNS + 1):
                    s.upload(MG3D_U, top, u0)
                    s.sync()
                    t0 = time.perf_counter()
                    fn()
                    if r:
                        ts.append((time.perf_counter() - t0) / per)
                return ts

            t_cyc = run(lambda: s.vcycles(ITERS), ITERS)
            t_fmg = run(lambda: s.fmg_solve(1), 1)
            print(f"  V-cycle         {spread(t_cyc)}")
            print(f"  fmg_solve(1)    {spread(t_fmg)}   {statistics.median(t_fmg) / statistics.median(t_cyc):.2f} cycles", flush=True)


if __name__ == "__main__":
    main()
