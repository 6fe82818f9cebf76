#!/usr/bin/env python3
"""The GPU figures of the mask's coarsening rules (mg3d_ctx_set_mask_coarsening) that INTEGRATION.md, "Embedded
conductors", records: python tools/mask_coarsening_bench.py [--fmg] [c,L]     (default 9,7: 513^3)

Without --fmg: the time of mg3d_ctx_set_mask from a pageable host array under MG3D_MASK_INJECT and MG3D_MASK_KEEP,
alternating -- a host clock around the call, which ends in a host synchronisation; REPEATS timed calls per rule behind two
warm-up calls, every one printed so the spread is on the page; no coarse factor; the body is a ball, a one-point plate on an
odd plane and a needle on odd j, k.  Then the time of a change of the rule under the installed mask (no copy, no pack).
A library without the call (MG3D_LIB_PATH pointing at an older build, for an A/B in one session) is timed as it is.

With --fmg: the plate of tests/_mask_ref.py held at 1 in a grounded box, d = 0, at 33^3 and 65^3 under KEEP -- the residual
norm after fmg_solve(1), after one plain cycle from the zero guess, and how many plain cycles get below FMG's norm (the CPU
twin of these figures: tools/mask_coarsening_convergence.py --fmg)."""
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (the HIP runtime is torch's, as in bench.py)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multigrid_parallel_amd as M  # noqa: E402
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U  # noqa: E402

REPEATS = int(os.environ.get("REPEATS", "7"))


def body(N):
    x = np.linspace(0.0, 1.0, N)
    m = ((x[:, None, None] - .5) ** 2 + (x[None, :, None] - .5) ** 2 + (x[None, None, :] - .3) ** 2 <= 0.15 ** 2).astype(np.uint8)
    g, c = N // 4, (N // 2) | 1
    m[c, g:N - g, g:N - g] = 1            # a one-point plate on an odd plane
    m[g:N - g, c, c + 2 * (N // 8)] = 1   # a needle on odd j, k
    return m


def set_mask_times(c, L):
    with M.Solver(c, L, 2) as s:
        N = s.N
        mask = body(N)
        has_rule = hasattr(s.L, "mg3d_ctx_set_mask_coarsening")
        rules = ("inject", "keep") if has_rule else ("inject",)
        runs = {r: [] for r in rules}
        for rep in range(REPEATS + 2):
            for r in rules:
                s.set_mask(None)
                if has_rule:
                    s.set_mask_coarsening(r)
                s.sync()
                t0 = time.perf_counter()
                s.set_mask(mask)
                if rep >= 2:
                    runs[r].append((time.perf_counter() - t0) * 1e3)
        print(f"{N}^3, {int(mask.sum())} fixed points" + ("" if has_rule else " (a library without mg3d_ctx_set_mask_coarsening)"))
        for r in rules:
            v = runs[r]
            print(f"  set_mask under {r:6s} ms: " + " ".join(f"{t:7.2f}" for t in v) +
                  f"   min {min(v):7.2f} median {sorted(v)[len(v) // 2]:7.2f} max {max(v):7.2f}", flush=True)
        if not has_rule:
            return
        print(f"  nonzero bytes per level under keep (coarsest first): {[int((s.get_mask(l) != 0).sum()) for l in range(L)]}")
        for r in ("inject", "keep", "inject", "keep"):
            s.sync()
            t0 = time.perf_counter()
            s.set_mask_coarsening(r)
            print(f"  set_mask_coarsening({r}) under the mask: {(time.perf_counter() - t0) * 1e3:7.2f} ms", flush=True)


def fmg_quality():
    import _mask_ref as MR
    for c, L in ((5, 4), (5, 5)):
        N = (c - 1) * (1 << (L - 1)) + 1
        mask = MR.plate(N, (N // 2) | 1)
        u0 = np.zeros((N, N, N))
        u0[mask != 0] = 1.0
        with M.Solver(c, L, 2) as s:
            s.set_mask_coarsening("keep")
            s.set_mask(mask)
            s.get_details()
            s.upload(MG3D_D, L - 1, np.zeros(N ** 3))
            s.upload(MG3D_U, L - 1, u0)
            fmg = s.fmg_solve(1)
            s.upload(MG3D_U, L - 1, u0)
            norms = []
            while len(norms) < 30 and (not norms or norms[-1] > fmg):
                norms.append(s.vcycles(1)[0])
        print(f"{N}^3 plate at 1, d = 0: fmg_solve(1) {fmg:.6e}; plain KEEP cycles from the zero guess: {norms[0]:.6e} after "
              f"one, {len(norms)} to get below FMG's norm ({norms[-1]:.6e})", flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--fmg" in args:
        fmg_quality()
    else:
        sizes = [tuple(int(v) for v in a.split(",")) for a in args if not a.startswith("--")] or [(9, 7)]
        for c, L in sizes:
            set_mask_times(c, L)
