#!/usr/bin/env python3
"""The launches behind the setters of the operator fields (eps, mask, screening field, periodic and Neumann masks), for a
launch-order comparison of two builds of the library (MG3D_LIB_PATH selects the other one; profiles/operator_fields_launches.txt):

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o t -- python tools/operator_launches.py run
    python tools/operator_launches.py list <dir>/.../t_kernel_trace.csv

run:  the walk of tests/test_gpu_operator_fields.py at 17^3 -- both starts, the host forms and the tensor forms, two cycles
      behind every step -- and the six setter forms (host and tensor; eps, mask, s) once each on a context at 33^3 with a
      built factor, two cycles behind each.
list: the trace's rows in the order of Dispatch_Id (the order the host enqueued them), one line per launch -- "kernel
      grid x,y,z  workgroup x,y,z", template arguments kept, parameter list dropped --: how many, the sha256 of the list, the
      launches per kernel.
time: wall time of the six setter forms at 257^3 (c = 5, L = 7) with a built factor, each call between two sync(), REPEATS
      calls each: min / median / max in ms (profiles/operator_fields_ab.txt)."""
import collections
import csv
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run():
    os.environ["MG3D_SWEEP_TUNE"] = "0"  # the first-use chunk-length measurement picks grids by timing: not comparable
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import torch  # noqa: F401  (before the package, as bench.py does)
    import multigrid_parallel_amd as M
    import test_gpu_operator_fields as T
    from multigrid_parallel_amd.binding import MG3D_D, MG3D_U
    import _coef_ref as CR
    import _mask_ref as MR
    import _shift_field_ref as SF

    def cycles(s, u, d):
        s.upload(MG3D_U, s.num_levels - 1, u)
        s.upload(MG3D_D, s.num_levels - 1, d)
        return list(s.vcycles(2))

    c, L, N = 5, 3, 17
    rng = np.random.default_rng(17)
    u, d = rng.standard_normal(N ** 3), rng.standard_normal(N ** 3)
    for name in sorted(T.RUNS):
        (axes, faces), _, sigma = T.RUNS[name]
        for form in ("host", "tensor"):
            with M.Solver(c, L, 2) as s:
                s.set_shift(sigma)
                s.set_periodic(axes)
                s.set_neumann(faces)
                s.get_details()
                norms = [cycles(s, u, d)[-1] for _ in T._walk(s, form, name, N)]
            print("walk", name, form, " ".join(f"{v!r}" for v in norms))
    c, L, N = 5, 4, 33
    u, d = rng.standard_normal(N ** 3), rng.standard_normal(N ** 3)
    arrays = {"eps": CR.FIELDS["exp"](N), "mask": MR.gpu_test_mask(N), "field": SF.random_field(N, 1.0 / (N - 1), 1)}
    with M.Solver(c, L, 2) as s:
        s.get_details()
        for what in ("eps", "mask", "field"):
            for form in ("host", "tensor"):
                T._set(s, form, what, arrays[what])
                print("setter", what, form, repr(cycles(s, u, d)[-1]))


REPEATS = 9


def time_setters():
    import statistics
    import time
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import torch
    import multigrid_parallel_amd as M
    c, L, N = 5, 7, 257
    rng = np.random.default_rng(257)
    dev = torch.device("cuda:0")
    eps = 1.0 + rng.random((N, N, N))
    field = rng.random((N, N, N)) * (N - 1) ** 2
    mask = (rng.random((N, N, N)) < 0.1).astype(np.uint8)
    with M.Solver(c, L, 2) as s:
        s.get_details()
        forms = [("eps host", s.set_coefficient, eps), ("eps tensor", s.set_coefficient_tensor, torch.from_numpy(eps).to(dev)),
                 ("mask host", s.set_mask, mask), ("mask tensor", s.set_mask_tensor, torch.from_numpy(mask).to(dev)),
                 ("s host", s.set_shift_field, field), ("s tensor", s.set_shift_field_tensor, torch.from_numpy(field).to(dev))]
        for name, call, a in forms:
            call(a)  # the first call allocates: not timed
            ms = []
            for _ in range(REPEATS):
                torch.cuda.synchronize()
                s.sync()
                t0 = time.perf_counter()
                call(a)
                s.sync()
                ms.append(1e3 * (time.perf_counter() - t0))
            print(f"{name:12s} min {min(ms):9.3f}  median {statistics.median(ms):9.3f}  max {max(ms):9.3f} ms")
            call(None)


def launches(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    out = []
    for r in rows:
        kernel = r["Kernel_Name"].split("(")[0].replace(" [clone .kd]", "").replace(".kd", "")
        grid = ",".join(r.get(f"Grid_Size_{a}", "?") for a in "XYZ")
        wg = ",".join(r.get(f"Workgroup_Size_{a}", "?") for a in "XYZ")
        out.append(f"{kernel}  grid {grid}  workgroup {wg}")
    return out


def summary(path):
    lines = launches(path)
    print(f"{len(lines)} launches, sha256 of the list {hashlib.sha256(chr(10).join(lines).encode()).hexdigest()[:16]}")
    names = collections.Counter(line.split("  grid")[0] for line in lines)
    for kernel, n in sorted(names.items(), key=lambda kv: (-kv[1], kv[0])):
        print(f"{n:8d}  {kernel}")
    if len(sys.argv) > 3:  # list <trace.csv> <file>: the list itself, for diff
        with open(sys.argv[3], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run()
    elif sys.argv[1:2] == ["time"]:
        time_setters()
    elif sys.argv[1:2] == ["list"] and len(sys.argv) >= 3:
        summary(sys.argv[2])
    else:
        sys.exit(__doc__)
