#!/usr/bin/env python3
"""The particle gather and scatter against a plain torch restatement: python tools/particle_bench.py [c,L ...]
(default 9,7 and 9,6: 513^3 and 257^3, constant operator, Dirichlet faces, random u; POINTS=1000000,10000000).

Per size and number of points, for points uniformly random in the box and for the same points sorted by cell, in one
process, the median (min .. max) of RUNS runs after a warm-up, each run one call between two events on the current stream:
  sample   sample_tensor(pos): u and the three components of the gradient, float64, one launch
  deposit  deposit_tensor(pos, q): scan, accumulate, apply (the clearing of the accumulator included)
  torch    the same in torch on the same GPU: index arithmetic, then for the sample eight gathers of u and of a
           gradient_tensor() made beforehand (its launch is NOT in the time), for the deposit eight index_add_ -- floating
           point atomics, so neither reproducible nor independent of the order of the points
Nothing is gated; the numbers go into INTEGRATION.md ("Particles")."""
import os
import statistics
import sys

import torch  # first: the HIP runtime is torch's

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U

RUNS = int(os.environ.get("RUNS", "5"))
POINTS = [int(v) for v in os.environ.get("POINTS", "1000000,10000000").split(",")]


def timed(call):
    """RUNS x (one call between two events) after a warm-up -> milliseconds"""
    call()
    torch.cuda.synchronize()
    out = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def spread(ts):
    return f"{statistics.median(ts):9.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})"


def cells(pos, h, N):
    t = pos / h
    c = torch.floor(t).clamp_(max=N - 2)
    return c.long(), t - c


def torch_sample(u, g, pos, h, N):
    c, f = cells(pos, h, N)
    base = (c[:, 0] * N + c[:, 1]) * N + c[:, 2]
    uf, gf = u.view(-1), g.view(3, -1)
    su = torch.zeros(pos.shape[0], dtype=torch.float64, device=pos.device)
    sg = torch.zeros(3, pos.shape[0], dtype=torch.float64, device=pos.device)
    for a in range(2):
        for b in range(2):
            for cc in range(2):
                w = (f[:, 0] if a else 1 - f[:, 0]) * (f[:, 1] if b else 1 - f[:, 1]) * (f[:, 2] if cc else 1 - f[:, 2])
                idx = base + ((a * N + b) * N + cc)
                su += w * uf[idx]
                sg += w * gf[:, idx]
    return su, sg


def torch_deposit(d, pos, q, h, N, scale):
    c, f = cells(pos, h, N)
    base = (c[:, 0] * N + c[:, 1]) * N + c[:, 2]
    df = d.view(-1)
    qs = q * (scale / h ** 3)
    for a in range(2):
        for b in range(2):
            for cc in range(2):
                w = (f[:, 0] if a else 1 - f[:, 0]) * (f[:, 1] if b else 1 - f[:, 1]) * (f[:, 2] if cc else 1 - f[:, 2])
                df.index_add_(0, base + ((a * N + b) * N + cc), qs * w)


def main():
    cases = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or [(9, 7), (9, 6)]
    dev = dict(dtype=torch.float64, device="cuda")
    for c, L in cases:
        with M.Solver(c, L, 2) as s:
            N, top, h = s.N, L - 1, s.h
            gen = torch.Generator(device="cuda").manual_seed(N)
            u = torch.rand(N, N, N, generator=gen, **dev) * 2 - 1
            s.upload_tensor(MG3D_U, top, u)
            g = s.gradient_tensor(scale=-1.0)
            d = torch.zeros(N, N, N, **dev)
            for count in POINTS:
                pos = torch.rand(count, 3, generator=gen, **dev) * ((N - 1) * h)
                q = torch.rand(count, generator=gen, **dev) * 2 - 1
                cell, _ = cells(pos, h, N)
                order = torch.argsort((cell[:, 0] * N + cell[:, 1]) * N + cell[:, 2])
                del cell
                ou, og = torch.empty(count, **dev), torch.empty(count, 3, **dev)
                print(f"{N}^3, {count} points, Dirichlet faces, float64, median of {RUNS} runs:")
                for name, p, qq in (("random", pos, q), ("sorted by cell", pos[order].contiguous(), q[order].contiguous())):
                    ts = timed(lambda: s.sample_tensor(p, scale=-1.0, out_u=ou, out_grad=og))
                    tt = timed(lambda: torch_sample(u, g, p, h, N))
                    ds = timed(lambda: s.deposit_tensor(p, qq, scale=-1.0))
                    dt = timed(lambda: torch_deposit(d, p, qq, h, N, -1.0))
                    ms, mt = statistics.median(ts), statistics.median(tt)
                    md, mdt = statistics.median(ds), statistics.median(dt)
                    print(f"  {name:15s} sample   library {spread(ts)}   torch {spread(tt)}   library / torch = {ms / mt:.2f}")
                    print(f"  {name:15s} deposit  library {spread(ds)}   torch {spread(dt)}   library / torch = {md / mdt:.2f}",
                          flush=True)
                s.zero(MG3D_D, top)
                d.zero_()
                del pos, q, order, ou, og
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
