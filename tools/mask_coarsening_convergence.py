#!/usr/bin/env python3
"""Convergence of plain V(2,2) cycles with embedded conductors (mg3d_ctx_set_mask) under the two rules a coarser level can
take the mask by (mg3d_ctx_set_mask_coarsening) -- injection, the default, and KEEP --, measured with the numpy restatements
tests/_mask_ref.py and tests/_mask_keep_ref.py: the library's arithmetic, no GPU.  A Dirichlet box, c = 5, sigma = 0, no
eps, the body held at 1, a random right-hand side (seed 1).  Per body and rule: the residual factor per cycle, the geometric
mean over cycles 4 .. 10, and (--pcg) the wpcg iterations to rtol 1e-8.  --fmg: the residual norm after fmg_solve(1) under
KEEP on the plate held at 1 with d = 0, and how many plain KEEP cycles from the zero guess reach it.
Usage: tools/mask_coarsening_convergence.py [--pcg] [--fmg] [N ...]     (default 33 65)"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _mask_keep_ref as MK  # noqa: E402
import _mask_ref as MR  # noqa: E402

RULES = (("injection", MK.INJECT), ("KEEP", MK.KEEP))


def bodies(N):
    return {"plate, odd plane": MR.plate(N, (N // 2) | 1), "needle, odd j, k": MR.needle(N), "random 10 %": MR.random_mask(N),
            "gpu_test_mask": MR.gpu_test_mask(N), "sphere r=0.2": MR.sphere(N)}


def levels(N):
    L = int(round(math.log2((N - 1) // 4))) + 1
    assert 4 * (1 << (L - 1)) + 1 == N, "N = 4 * 2^k + 1"
    return L


def start(prob, mask, d):
    prob.u[-1][...] = 0.
    prob.u[-1][mask != 0] = 1.0
    prob.d[-1][...] = d
    return prob.u[-1].copy()


def cycle_table(N, pcg):
    L = levels(N)
    d = np.random.default_rng(1).standard_normal((N, N, N))
    for name, mask in bodies(N).items():
        out = []
        for _, rule in RULES:
            prob = MK.Hierarchy(5, L, 2, 0.0, None, 0, 0, mask, rule=rule)
            u0 = start(prob, mask, d)
            with np.errstate(all="ignore"):
                n = prob.vcycles(10)
            ok = n[3] > 0 and np.isfinite(n[9])
            its = ""
            if pcg:
                _, norms, conv, _, _ = MR.wpcg(prob, u0, d, 1e-8, 0.0, 80)
                its = f" (wpcg {len(norms) - 1}{'' if conv else ', not converged'})"
            out.append(f"{(n[9] / n[3]) ** (1.0 / 6) if ok else float('nan'):7.3f}{its}")
        print(f"{N:3d}^3  {name:18s} injection {out[0]}   KEEP {out[1]}", flush=True)


def fmg_quality(N):
    L = levels(N)
    mask = MR.plate(N, (N // 2) | 1)
    zero = np.zeros((N, N, N))
    prob = MK.Hierarchy(5, L, 2, 0.0, None, 0, 0, mask)
    start(prob, mask, zero)
    fmg = MK.fmg_solve(prob, 1)
    prob = MK.Hierarchy(5, L, 2, 0.0, None, 0, 0, mask)
    start(prob, mask, zero)
    norms = []
    while len(norms) < 30 and (not norms or norms[-1] > fmg):
        norms.append(prob.vcycle())
    print(f"{N:3d}^3  plate at 1, d = 0: residual norm after fmg_solve(1) under KEEP {fmg:.3e}; plain KEEP cycles from the zero "
          f"guess: {norms[0]:.3e} after one, {len(norms)} cycles to reach FMG's norm ({norms[-1]:.3e})", flush=True)


args = sys.argv[1:]
sizes = [int(a) for a in args if not a.startswith("--")] or [33, 65]
for N in sizes:
    if "--fmg" in args:
        fmg_quality(N)
    else:
        cycle_table(N, "--pcg" in args)
