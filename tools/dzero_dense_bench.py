#!/usr/bin/env python3
"""The case the zero map of d can only lose: the flagship problem (513^3, V(2,2), one launch per leg) with a DENSE right-hand
side -- no plane of d is empty, the scan finds nothing and every launch runs the kernels without the map.  Same-box A/B against
a build without the map: ms per cycle must agree within the run-to-run spread.  Also runs on a build that has no map.
Usage (on the GPU box): python3 tools/dzero_dense_bench.py [--coarse 9 --levels 7 --steps 20 --warmup 3 --reps 5]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # first: the HIP runtime is torch's, as in bench.py

import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U

ap = argparse.ArgumentParser()
ap.add_argument("--coarse", type=int, default=9)
ap.add_argument("--levels", type=int, default=7)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()

with M.Solver(args.coarse, args.levels, 2) as s:
    N, top = s.N, args.levels - 1
    s.setup_test_problem()
    g = torch.Generator(device="cuda").manual_seed(1)
    d = torch.rand((N, N, N), dtype=torch.float64, device="cuda", generator=g) - 0.5
    s.upload_tensor(MG3D_D, top, d)
    s.vcycles(3)  # priming, as bench.py: first-use chunk measurement, the scan of the new d
    ms = []
    for _ in range(args.reps):
        s.zero(MG3D_U, top)
        s.setup_boundary_conditions(MG3D_U)
        s.vcycles(args.warmup)
        s.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.vcycles(args.steps)
        s.sync()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) / args.steps * 1e3)
    planes = s.dzero_planes() if hasattr(s, "dzero_planes") else None
print(json.dumps({"what": f"{N}^3 V(2,2), dense d", "ms_per_cycle": [round(x, 4) for x in ms],
                  "median": round(sorted(ms)[len(ms) // 2], 4), "zero_map": planes}))
