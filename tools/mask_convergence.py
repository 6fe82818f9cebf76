#!/usr/bin/env python3
"""Convergence of plain V(2,2) cycles and of PCG with embedded conductors (mg3d_ctx_set_mask), measured with the numpy
restatement tests/_mask_ref.py -- the library's arithmetic, no GPU.  A grounded Dirichlet box, the body held at 1, d = 0,
c = 5.  Per body: the residual factor per cycle (geometric mean over cycles 5 .. 12) and the PCG iterations to 1e-8.
Usage: tools/mask_convergence.py [N ...]     (default 33 65)"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _mask_ref as MR  # noqa: E402


def bodies(N):
    even = (N // 2) & ~1
    return {"sphere r=0.2": MR.sphere(N), "plate, even plane": MR.plate(N, even), "plate, odd plane": MR.plate(N, even + 1),
            "needle, odd indices": MR.needle(N), "random 10 %": MR.random_mask(N)}


for N in [int(a) for a in sys.argv[1:]] or [33, 65]:
    L = int(round(math.log2((N - 1) // 4))) + 1
    assert 4 * (1 << (L - 1)) + 1 == N, "N = 4 * 2^k + 1"
    for name, mask in bodies(N).items():
        prob = MR.Hierarchy(5, L, 2, 0.0, None, 0, 0, mask)
        u0 = np.zeros((N, N, N))
        u0[mask != 0] = 1.0
        prob.u[-1][...] = u0
        prob.d[-1][...] = 0.
        with np.errstate(all="ignore"):
            n = prob.vcycles(12)
        factor = (n[11] / n[3]) ** (1.0 / 8) if n[3] > 0 and np.isfinite(n[11]) else float("nan")
        _, norms, ok, _, _ = MR.wpcg(prob, u0, np.zeros_like(u0), 1e-8, 0.0, 80)
        coarse = [int(MR.fixed(m, 0, 0).sum()) for m in prob.mask]
        print(f"{N:3d}^3  {name:22s} fixed per level {coarse}  cycle factor {factor:6.3f}  "
              f"PCG iterations to 1e-8: {len(norms) - 1}{'' if ok else ' (not converged)'}", flush=True)
