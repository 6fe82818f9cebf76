#!/usr/bin/env python3
"""The screening field (mg3d_ctx_set_shift_field) against the same context without it: python tools/shift_field_bench.py
[c,L ...]  (default 9,7: 513^3, V(2,2), all-Dirichlet, the reference's test problem).

Per operator (eps = 1 + 1/2 sin(2 pi x) cos(pi y); constant): ms per cycle of mg3d_vcycles -- every one of REPEATS timed
runs is printed, so the run-to-run spread is on the page -- for
    no field    the context as it is (eps: the unfused eps kernels; constant: the fused schedules)
    zero field  an all-zero field: the SFIELD kernels, every double read, the arithmetic of no field
    random      a random field in [0, 1/h^2]
and inside the cycle the finest level's kernel timers per launch.  A library without the field (the parent of the change
that added it) prints the "no field" lines only: the same script measures both.  BC=axes,faces in the environment sets
periodic axes and Neumann faces first (the wrap and reflect forms of the kernels; the constant operator is then unfused too)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_parallel_amd as M

CYCLES = int(os.environ.get("CYCLES", "10"))
REPEATS = int(os.environ.get("REPEATS", "5"))
AXES, FACES = (int(v) for v in os.environ.get("BC", "0,0").split(","))


def smooth_eps(N):
    x = np.linspace(0.0, 1.0, N)
    return np.ascontiguousarray(np.broadcast_to(1.0 + 0.5 * np.sin(2 * np.pi * x)[:, None, None] * np.cos(np.pi * x)[None, :, None],
                                                (N, N, N)))


def measure(s, top, label):
    if AXES or FACES:  # (the test problem fills Dirichlet values into all six faces)
        from multigrid_parallel_amd.binding import MG3D_D, MG3D_U
        s.get_details()
        s.zero(MG3D_U, top)
        s.upload(MG3D_D, top, np.random.default_rng(2).standard_normal(s.N ** 3))
    else:
        s.setup_test_problem()
    s.vcycles(3)
    runs = []
    for _ in range(REPEATS):
        s.sync()
        t0 = time.perf_counter()
        s.vcycles(CYCLES)
        runs.append((time.perf_counter() - t0) / CYCLES * 1e3)
    s.timing_enable(3)
    s.timing_reset()
    s.vcycles(CYCLES)
    s.sync()
    kt = s.kernel_times()
    s.timing_enable(0)
    per = {k: secs / calls * 1e3 for (l, k), (calls, secs) in kt.items() if l == top}
    print(f"  {label:10s} ms per cycle: " + " ".join(f"{r:7.3f}" for r in runs) + f"   min {min(runs):7.3f} max {max(runs):7.3f}")
    print("             finest level, ms per launch: " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(per.items())), flush=True)
    return min(runs)


def main():
    sizes = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or [(9, 7)]
    for c, L in sizes:
        with M.Solver(c, L, 2) as s:
            N, top = s.N, L - 1
            has_field = hasattr(s, "set_shift_field")
            print(f"{N}^3 V(2,2), periodic axes {AXES}, Neumann faces {FACES}, {CYCLES} cycles per timed run, "
                  f"library {'with' if has_field else 'without'} the field")
            s.set_periodic(AXES)
            s.set_neumann(FACES)
            for name, eps in (("eps", smooth_eps(N)), ("constant", None)):
                print(f" {name} operator")
                if has_field:
                    s.set_shift_field(None)
                s.set_coefficient(eps)
                base = measure(s, top, "no field")
                if not has_field:
                    continue
                s.set_shift_field(np.zeros(N ** 3))
                zero = measure(s, top, "zero field")
                s.set_shift_field(np.random.default_rng(1).uniform(0.0, 1.0 / (s.h * s.h), N ** 3))
                rnd = measure(s, top, "random")
                print(f"  zero field / no field {zero / base:.3f}, random / zero field {rnd / zero:.3f}", flush=True)


if __name__ == "__main__":
    main()
