#!/usr/bin/env python3
"""The field output against the unpack launch: python tools/field_bench.py [c,L ...]
(default 9,7 and 9,5: 513^3 and 129^3, constant operator, Dirichlet faces, random u).

Per size, in one process, RUNS runs after a warm-up, median (min .. max):
  (a) unpack    ms per launch of download_tensor into a contiguous float64 tensor (the unpack kernel)
  (b) gradient  ms per launch of gradient_tensor with three contiguous float64 components
  (c) gradient  the same with float32 components
      (a) - (c) from the library's "pack" kernel timer (timing mode 3, REPS launches per run, in runs of their own)
  (d) flux, energy   ms per call of field_flux(1) (a ball of radius 0.2 as the body) and field_energy(), wall clock: launch,
      fold, one host synchronisation
and the condition the gradient launch is held to: (b) <= 3 x (a) of the same run, with the GB/s (b) reaches on its
compulsory traffic -- four arrays: u read once, three components written."""
import os
import statistics
import sys
import time

import numpy as np
import torch  # first: the HIP runtime is torch's

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_U

RUNS = int(os.environ.get("RUNS", "5"))
REPS = int(os.environ.get("REPS", "10"))


def spread(ts, unit=1e3):
    return f"{statistics.median(ts) * unit:9.3f} ms (min {min(ts) * unit:.3f}, max {max(ts) * unit:.3f}, {len(ts)} runs)"


def pack_ms(s):
    calls, secs = s.kernel_times().get((s.num_levels - 1, "pack"), (0, 0.0))
    return secs / calls if calls else float("nan")


def kernel_runs(s, call):
    """RUNS x (REPS launches under the kernel timer) -> seconds per launch of each run"""
    call()
    s.sync()
    out = []
    for _ in range(RUNS):
        s.timing_enable(3)
        s.timing_reset()
        for _ in range(REPS):
            call()
        s.sync()
        out.append(pack_ms(s))
        s.timing_enable(0)
    return out


def wall_runs(call):
    call()
    out = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        for _ in range(REPS):
            call()
        out.append((time.perf_counter() - t0) / REPS)
    return out


def ball(N, radius=0.2):
    x = np.linspace(0.0, 1.0, N)
    r2 = (x[:, None, None] - 0.5) ** 2 + (x[None, :, None] - 0.5) ** 2 + (x[None, None, :] - 0.5) ** 2
    return (r2 <= radius * radius).astype(np.uint8)


def main():
    cases = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or [(9, 7), (9, 5)]
    for c, L in cases:
        with M.Solver(c, L, 2) as s:
            N, top = s.N, L - 1
            s.upload_tensor(MG3D_U, top, torch.rand(N, N, N, dtype=torch.float64, device="cuda") * 2 - 1)
            print(f"{N}^3, constant operator, Dirichlet faces, random u, {REPS} launches per run:")
            out = torch.empty(N, N, N, dtype=torch.float64, device="cuda")
            g64 = torch.empty(3, N, N, N, dtype=torch.float64, device="cuda")
            g32 = torch.empty(3, N, N, N, dtype=torch.float32, device="cuda")
            a = kernel_runs(s, lambda: s.download_tensor(MG3D_U, top, out=out))
            b = kernel_runs(s, lambda: s.gradient_tensor(out=g64, scale=-1.0))
            cc = kernel_runs(s, lambda: s.gradient_tensor(out=g32, scale=-1.0))
            print(f"  (a) unpack   {'contiguous float64':36s}{spread(a)} per launch")
            print(f"  (b) gradient {'3 x contiguous float64':36s}{spread(b)} per launch")
            print(f"  (c) gradient {'3 x contiguous float32':36s}{spread(cc)} per launch")
            s.set_mask(ball(N))
            f = wall_runs(lambda: s.field_flux(1))
            e = wall_runs(lambda: s.field_energy())
            print(f"  (d) flux     {'label 1: a ball of radius 0.2':36s}{spread(f)} per call")
            print(f"  (d) energy   {'':36s}{spread(e)} per call")
            ma, mb, mc = (statistics.median(v) * 1e3 for v in (a, b, cc))
            pts = float(N) ** 3
            print(f"  (b) / (a) = {mb / ma:.2f} (held to <= 3: {'met' if mb <= 3 * ma else 'MISSED'}); compulsory traffic: "
                  f"(b) 4 arrays of float64 = {4 * 8 * pts / 1e9:.3f} GB at {4 * 8 * pts / mb / 1e6:.0f} GB/s, "
                  f"(c) {(8 + 12) * pts / 1e9:.3f} GB at {(8 + 12) * pts / mc / 1e6:.0f} GB/s, "
                  f"(a) 2 arrays = {2 * 8 * pts / 1e9:.3f} GB at {2 * 8 * pts / ma / 1e6:.0f} GB/s", flush=True)


if __name__ == "__main__":
    main()
