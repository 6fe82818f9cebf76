#!/usr/bin/env python3
"""The particle gather, scatter and push against a plain torch restatement: python tools/particle_bench.py [c,L ...]
(default 9,7 and 9,6: 513^3 and 257^3, constant operator, Dirichlet faces, random u; POINTS=1000000,10000000;
ROWS=sample,deposit,push; ROWS=sort for the reorder alone, see below).

Per size and number of points, for points uniformly random in the box and for the same points sorted by cell, in one
process, the median (min .. max) of RUNS runs after a warm-up, each run one call between two events on the current stream:
  sample   sample_tensor(pos): u and the three components of the gradient, float64, one launch
  deposit  deposit_tensor(pos, q): scan, accumulate, apply (the clearing of the accumulator included)
  torch    the same in torch on the same GPU: index arithmetic, then for the sample eight gathers of u and of a
           gradient_tensor() made beforehand (its launch is NOT in the time), for the deposit eight index_add_ -- floating
           point atomics, so neither reproducible nor independent of the order of the points
  push     push_tensor(pos, vel, qm, dt, fate): one launch; speeds up to half a spacing per step, kicks up to a hundredth.
           Its torch column is the composition it replaces: sample_tensor(want_u=False), then the kick, the drift and the
           fates of Dirichlet faces in torch (the first exit in axis order, INVALID for what is not finite; no table)
  sort     (ROWS=sort) points that start sorted by cell and then drift: DRIFT (50) pushes at up to half a spacing per step.
           (a) the cost of one reorder: sort_tensor(pos, fate) plus one permute_tensors of pos, vel, q, qm and fate (nine
           vectors, 1 + 3 passes + 1 launches) against what it replaces in torch on the same GPU: the keys of cells()
           above (no periodic wrap; the dead put last), torch.sort(stable=True), one index_select per tensor.  The two
           sides alternate run by run.  (b) the gain: push_tensor plus deposit_tensor on the drifted points against the same
           on the re-sorted points, alternating, and how many steps repay one reorder.
Nothing is gated; the numbers go into INTEGRATION.md ("Particles")."""
import os
import statistics
import sys

import torch  # first: the HIP runtime is torch's

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U

RUNS = int(os.environ.get("RUNS", "5"))
ROWS = os.environ.get("ROWS", "sample,deposit,push").split(",")
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


def timed_pair(first, second):
    """timed() for two calls that alternate run by run: (milliseconds of first, of second)"""
    first()
    second()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(RUNS):
        for call, ts in zip((first, second), out):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
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


def torch_push(s, pos, vel, qm, fate, dt, h, N, og):
    s.sample_tensor(pos, want_u=False, scale=-1.0, out_grad=og)  # (NaN for a point outside)
    alive = fate == 0
    v1 = vel + (qm * dt)[:, None] * og
    x1 = pos + dt * v1
    t = x1 / h
    face = 2 * torch.arange(3, device=pos.device)
    code = torch.where(t < 0, 256 + face, torch.where(t > N - 1, 257 + face, torch.zeros_like(face)))
    first = torch.where(code[:, 0] != 0, code[:, 0], torch.where(code[:, 1] != 0, code[:, 1], code[:, 2]))
    f = torch.where(torch.isfinite(x1).all(dim=1), first, torch.full_like(first, 262)).to(torch.int32)
    moved = (alive & (f != 262))[:, None]
    pos.copy_(torch.where(moved, x1, pos))
    vel.copy_(torch.where(moved, v1, vel))
    fate.copy_(torch.where(alive, f, fate))


def torch_reorder(tensors, pos, fate, h, N):
    """what the library's reorder replaces: the tool's own keys, a stable sort, one index_select per tensor"""
    cell, _ = cells(pos, h, N)
    key = (cell[:, 0] * N + cell[:, 1]) * N + cell[:, 2]
    key = torch.where(fate != 0, torch.full_like(key, N ** 3), key)
    order = torch.sort(key, stable=True)[1]
    return [t.index_select(0, order) for t in tensors]


def sort_rows(s, gen, count, N, h):
    dev = dict(dtype=torch.float64, device="cuda")
    drift, step = int(os.environ.get("DRIFT", "50")), 1.0
    pos = torch.rand(count, 3, generator=gen, **dev) * ((N - 1) * h)
    cell, _ = cells(pos, h, N)
    pos = pos[torch.argsort((cell[:, 0] * N + cell[:, 1]) * N + cell[:, 2])].contiguous()
    del cell
    vel = (torch.rand(count, 3, generator=gen, **dev) * 2 - 1) * (0.5 * h / step)
    q = torch.rand(count, generator=gen, **dev) * 2 - 1
    qm = q * (0.01 * h * h / (step * step))
    fate = torch.zeros(count, dtype=torch.int32, device="cuda")
    for _ in range(drift):
        s.push_tensor(pos, vel, qm, step, fate)
    tensors = [pos, vel, q, qm, fate]

    def library():
        perm, _ = s.sort_tensor(pos, fate)
        return s.permute_tensors(perm, *tensors)

    tl, tt = timed_pair(library, lambda: torch_reorder(tensors, pos, fate, h, N))
    ts = timed(lambda: s.sort_tensor(pos, fate))
    ml, mt = statistics.median(tl), statistics.median(tt)
    verdict = "faster" if max(tl) < min(tt) else ("slower" if min(tl) > max(tt) else "the ranges overlap")
    alive = int((fate == 0).sum())
    print(f"  after {drift} pushes ({alive} alive)")
    print(f"  reorder  library {spread(tl)}   torch {spread(tt)}   library / torch = {ml / mt:.2f} ({verdict})")
    print(f"           of which sort_tensor {spread(ts)}")
    # the gain: one step on the drifted points and on the re-sorted ones (clones: a step moves them)
    a = [t.clone() for t in tensors]
    b = [t.clone() for t in library()]
    del tensors, pos, vel, q, qm, fate

    def one_step(t):
        s.push_tensor(t[0], t[1], t[3], step, t[4])
        s.deposit_tensor(t[0], t[2], scale=-1.0)

    td, tr = timed_pair(lambda: one_step(a), lambda: one_step(b))
    md, mr = statistics.median(td), statistics.median(tr)
    even = f"{ml / (md - mr):.1f} steps repay one reorder" if md > mr else "a reorder is not repaid"
    print(f"  push + deposit  drifted {spread(td)}   re-sorted {spread(tr)}   gain {md - mr:.3f} ms a step: {even}")
    sys.stdout.flush()


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
                if "sort" in ROWS:
                    print(f"{N}^3, {count} points that drift away from cell order, Dirichlet faces, float64, median of {RUNS} runs:")
                    sort_rows(s, gen, count, N, h)
                    s.zero(MG3D_D, top)
                    torch.cuda.empty_cache()
                if not set(ROWS) & {"sample", "deposit", "push"}:
                    continue
                pos = torch.rand(count, 3, generator=gen, **dev) * ((N - 1) * h)
                q = torch.rand(count, generator=gen, **dev) * 2 - 1
                cell, _ = cells(pos, h, N)
                order = torch.argsort((cell[:, 0] * N + cell[:, 1]) * N + cell[:, 2])
                del cell
                ou, og = torch.empty(count, **dev), torch.empty(count, 3, **dev)
                print(f"{N}^3, {count} points, Dirichlet faces, float64, median of {RUNS} runs:")
                for name, p, qq in (("random", pos, q), ("sorted by cell", pos[order].contiguous(), q[order].contiguous())):
                    if "sample" in ROWS:
                        ts = timed(lambda: s.sample_tensor(p, scale=-1.0, out_u=ou, out_grad=og))
                        tt = timed(lambda: torch_sample(u, g, p, h, N))
                        ms, mt = statistics.median(ts), statistics.median(tt)
                        print(f"  {name:15s} sample   library {spread(ts)}   torch {spread(tt)}   library / torch = {ms / mt:.2f}")
                    if "deposit" in ROWS:
                        ds = timed(lambda: s.deposit_tensor(p, qq, scale=-1.0))
                        dt = timed(lambda: torch_deposit(d, p, qq, h, N, -1.0))
                        md, mdt = statistics.median(ds), statistics.median(dt)
                        print(f"  {name:15s} deposit  library {spread(ds)}   torch {spread(dt)}   library / torch = {md / mdt:.2f}")
                    if "push" in ROWS:
                        step = 1.0
                        vel = (torch.rand(count, 3, generator=gen, **dev) * 2 - 1) * (0.5 * h / step)
                        qm = qq * (0.01 * h * h / (step * step))
                        pa, va, fa = p.clone(), vel.clone(), torch.zeros(count, dtype=torch.int32, device="cuda")
                        pb, vb, fb = p.clone(), vel.clone(), torch.zeros(count, dtype=torch.int32, device="cuda")
                        ps = timed(lambda: s.push_tensor(pa, va, qm, step, fa))
                        pt = timed(lambda: torch_push(s, pb, vb, qm, fb, step, h, N, og))
                        mp, mpt = statistics.median(ps), statistics.median(pt)
                        print(f"  {name:15s} push     library {spread(ps)}   torch {spread(pt)}   library / torch = {mp / mpt:.2f}"
                              f"   (alive after {RUNS + 1} steps: {int((fa == 0).sum())} / {int((fb == 0).sum())})")
                        del vel, qm, pa, va, fa, pb, vb, fb
                    sys.stdout.flush()
                s.zero(MG3D_D, top)
                d.zero_()
                del pos, q, order, ou, og
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
