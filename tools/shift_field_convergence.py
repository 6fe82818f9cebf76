#!/usr/bin/env python3
"""Convergence of plain V(2,2) cycles with a screening field (mg3d_ctx_set_shift_field) under the two rules a coarser level
could take the field by -- the library's full weighting (the context's own restriction) and injection --, measured with the
numpy restatement tests/_shift_field_ref.py: the library's arithmetic, no GPU.  A Dirichlet box, c = 5, sigma = 0, no eps,
a zero guess and a random right-hand side.  Per field: the residual factor per cycle, the geometric mean over cycles 4 .. 10.
Usage: tools/shift_field_convergence.py [N ...]     (default 33 65)"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _shift_field_ref as SF  # noqa: E402


def fields(N):
    h = 1.0 / (N - 1)
    x = np.linspace(0.0, 1.0, N)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    rng = np.random.default_rng(1)
    plane = np.zeros((N, N, N))
    plane[(N // 2) | 1] = 1e8
    return {"smooth 1e3 cosh": 1e3 * np.cosh(X + Y - Z),
            "random in [0, 1/h^2]": rng.uniform(0.0, 1.0 / (h * h), (N, N, N)),
            "10/h^2 on a random 10 %": np.where(rng.uniform(size=(N, N, N)) < 0.1, 10.0 / (h * h), 0.0),
            "1e8 on one odd plane": plane,
            "1e6 in a ball r=0.2": np.where((X - 0.5) ** 2 + (Y - 0.5) ** 2 + (Z - 0.5) ** 2 <= 0.04, 1e6, 0.0)}


for N in [int(a) for a in sys.argv[1:]] or [33, 65]:
    L = int(round(math.log2((N - 1) // 4))) + 1
    assert 4 * (1 << (L - 1)) + 1 == N, "N = 4 * 2^k + 1"
    d = np.random.default_rng(2).standard_normal((N, N, N))
    for name, s in fields(N).items():
        out = []
        for rule in ("inject", "restrict"):
            prob = SF.Hierarchy(5, L, 2, 0.0, None, 0, 0, None, s, rule=rule)
            prob.d[-1][...] = d
            with np.errstate(all="ignore"):
                n = prob.vcycles(10)
            ok = n[3] > 0 and np.isfinite(n[9])
            out.append((n[9] / n[3]) ** (1.0 / 6) if ok else float("nan"))
        print(f"{N:3d}^3  {name:26s} injection {out[0]:7.3f}   full weighting {out[1]:7.3f}", flush=True)
