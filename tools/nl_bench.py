#!/usr/bin/env python3
"""One Newton iteration of Poisson-Boltzmann inside the library against the torch loop of INTEGRATION.md, "Screening field",
on the same GPU: python tools/nl_bench.py [c,L ...]   (default 9,6 and 9,7: 257^3 and 513^3; kappa^2 = 4, the manufactured
problem of tests/_shift_field_ref.py, constant operator, Dirichlet faces, V(2,2)).

Both sides take ONE Newton step from the same u (the Dirichlet values, zero inside) with the same linear work, two V-cycles of
the linearised operator:
  library  nl_solve(max_newton=1, cycles=2): evaluation, install, two cycles, trial, evaluation, install of s(x_1), u and d
           put back
  torch    the loop's body: set_shift_field_tensor(kappa2*cosh u), upload_tensor(d = f + kappa2*(sinh u - u cosh u)),
           upload_tensor(u), vcycles(2) in place of the loop's pcg_solve, download_tensor, the step size read on the host
The two alternate run by run (library, torch, library, ...), RUNS runs each after one warm-up of each; median and range.
Then, in a run of its own with the finest level's kernel timers on (they cost idle queue time: not part of the timing above),
one line per kernel timer of the library's iteration: launches and ms per launch.  The result goes to stdout and to
profiles/nl_bench.txt."""
import os
import statistics
import sys
import time

import numpy as np
import torch  # first: the HIP runtime is torch's

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U

RUNS = int(os.environ.get("RUNS", "5"))
KAPPA2 = 4.0


def problem(N):
    x = np.linspace(0.0, 1.0, N)
    sx = np.sin(np.pi * x)
    w = sx[:, None, None] * sx[None, :, None] * sx[None, None, :]
    ustar = w + 0.5 * x[:, None, None]
    f = -3.0 * np.pi ** 2 * w - KAPPA2 * np.sinh(ustar)
    u0 = ustar.copy()
    u0[1:-1, 1:-1, 1:-1] = 0.
    return np.ascontiguousarray(u0), np.ascontiguousarray(f)


def spread(ts):
    return f"{statistics.median(ts) * 1e3:9.3f} ms (min {min(ts) * 1e3:.3f}, max {max(ts) * 1e3:.3f}, {len(ts)} runs)"


def bench(c, L, out):
    N = (c - 1) * (1 << (L - 1)) + 1
    q = L - 1
    dev = torch.device("cuda:0")
    u0, f = problem(N)
    u0_t, f_t = torch.from_numpy(u0).to(dev), torch.from_numpy(f).to(dev)
    with M.Solver(c, L, 2) as lib, M.Solver(c, L, 2) as loop:
        for s in (lib, loop):
            s.get_details()
        lib.nl_setup("sinh", KAPPA2)
        lib.upload_tensor(MG3D_D, q, f_t)

        def library():
            lib.upload_tensor(MG3D_U, q, u0_t)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            norms, info = lib.nl_solve(max_newton=1, cycles=2)
            lib.sync()
            dt = time.perf_counter() - t0
            assert info["iterations"] == 1 and info["halvings"] == 0, info
            return dt, norms

        def torch_loop():
            u = u0_t.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop.set_shift_field_tensor(KAPPA2 * torch.cosh(u))
            loop.upload_tensor(MG3D_D, q, f_t + KAPPA2 * (torch.sinh(u) - u * torch.cosh(u)))
            loop.upload_tensor(MG3D_U, q, u)
            loop.vcycles(2)
            new = loop.download_tensor(MG3D_U, q)
            step = float((new - u).abs().max())
            dt = time.perf_counter() - t0
            return dt, step

        library()
        torch_loop()
        t_lib, t_loop = [], []
        for _ in range(RUNS):
            t_lib.append(library()[0])
            t_loop.append(torch_loop()[0])
        _, norms = library()
        out.append(f"{N}^3   ||F|| {norms[0]:.6e} -> {norms[1]:.6e}")
        out.append(f"  library  nl_solve(max_newton=1, cycles=2)         {spread(t_lib)}")
        out.append(f"  torch    the loop's body with vcycles(2)          {spread(t_loop)}")
        out.append(f"  ratio of the medians, torch / library: {statistics.median(t_loop) / statistics.median(t_lib):.3f}")
        lib.timing_enable(3)
        lib.timing_reset()
        library()
        out.append("  the library's iteration by kernel timer (finest level; a run of its own): launches, ms per launch, ms")
        for (level, name), (calls, secs) in sorted(lib.kernel_times().items()):
            if level == q:
                out.append(f"    MG3D_K_{name.upper():16s} {calls:4d}  {secs / calls * 1e3:9.4f}  {secs * 1e3:9.3f}")
        lib.timing_enable(0)


def main():
    sizes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or [(9, 6), (9, 7)]
    out = ["One Newton iteration of Poisson-Boltzmann (kappa^2 = 4): mg3d_nl_solve against the torch loop of INTEGRATION.md,",
           f"\"Screening field\", alternating run by run on {torch.cuda.get_device_name(0)} (tools/nl_bench.py)."]
    for c, L in sizes:
        bench(c, L, out)
    text = "\n".join(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.environ.get("NL_BENCH_OUT", os.path.join(ROOT, "profiles", "nl_bench.txt")), "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
