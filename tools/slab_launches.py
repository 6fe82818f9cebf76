#!/usr/bin/env python3
"""One loopback run of the slab driver for a launch-order comparison of two builds of the library (MG3D_LIB_PATH selects
the other one): rocprofv3 --kernel-trace --output-format csv -- python tools/slab_launches.py <configuration>, then the
trace's rows in the order of Dispatch_Id (profiles/slab_driver_launches.txt).
c = 9, L = 5 (129^3), P = 4 (16 in the thin_* configurations), MG3D_SLAB_MIN_PLANES=8, vcycles(4); vcycles(1); vcycles(2)."""
import os
import sys

CONFIGS = {
    "plain": {"MG3D_LEGS": "0", "MG3D_NO_CARRY": "1"},
    "carried": {"MG3D_CARRY_MIN": "66", "MG3D_LEGS": "0"},
    "legs_overlap": {"MG3D_LEGS_MIN": "66", "MG3D_LEGS": "1", "MG3D_NO_CARRY": "1", "MG3D_NO_OVERLAP": "0"},
    "legs_no_overlap": {"MG3D_LEGS_MIN": "66", "MG3D_LEGS": "1", "MG3D_NO_CARRY": "1", "MG3D_NO_OVERLAP": "1"},
    "coef": {},
    # beyond the five: the launches that cannot go edges first (thin slabs: 8 owned planes; no communication stream)
    "thin_plain": {"MG3D_LEGS": "0", "MG3D_NO_CARRY": "1", "P": "16"},
    "thin_legs": {"MG3D_LEGS_MIN": "66", "MG3D_LEGS": "1", "MG3D_NO_CARRY": "1", "P": "16"},
    "carried_no_overlap": {"MG3D_CARRY_MIN": "66", "MG3D_LEGS": "0", "MG3D_NO_OVERLAP": "1"},
}
cfg = sys.argv[1]
os.environ["MG3D_SLAB_MIN_PLANES"] = "8"
os.environ["MG3D_SWEEP_TUNE"] = "0"  # the first-use chunk-length measurement picks grids by timing: not comparable between runs
os.environ.update(CONFIGS[cfg])
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import multigrid_parallel_amd as M  # noqa: E402

c, L, nu, P = 9, 5, 2, int(CONFIGS[cfg].get("P", 4))
N = (c - 1) * (1 << (L - 1)) + 1
with M.DistSolver(c, L, nu, nranks=P) as d:
    if cfg == "coef":
        x = np.linspace(0.0, 1.0, N)
        d.set_coefficient(np.ascontiguousarray(np.broadcast_to(
            1.0 + 0.5 * np.sin(2 * np.pi * x)[:, None, None] * np.cos(np.pi * x)[None, :, None], (N, N, N))))
    d.setup_test_problem()
    n = list(d.vcycles(4)) + list(d.vcycles(1)) + list(d.vcycles(2))
    print(cfg, "lib", os.environ.get("MG3D_LIB_PATH", "tree"), "first level", d.first_level, "halo", d.halo,
          "carried", d.carried_cycles(), "legs", d.legs_cycles(), "overlap", d.comm_info()[1])
    print(cfg, "norms", " ".join(f"{v!r}" for v in n))
