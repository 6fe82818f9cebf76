#!/usr/bin/env python3
"""Records tests/golden/schedule_launches.json: the launch table and stage counts of every case of
tests/test_gpu_schedule.py, from the library the binding loads (MG3D_LIB_PATH=<build of another commit> for one that is not
the tree's).  Run it on a build of the commit BEFORE a change to the launch schedule and name that commit:
    MG3D_LIB_PATH=/path/to/parent/libmg3d.so python tools/record_schedule.py <commit> [output.json]
The test then holds the changed code to what that commit launched."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

lib_path = os.environ.get("MG3D_LIB_PATH")  # run_case() clears MG3D_* around every context: pin the library first
import torch  # noqa: E402,F401  (loads the HIP runtime first, as bench.py does)
import multigrid_parallel_amd.binding as B  # noqa: E402
B.lib()
import test_gpu_schedule as T  # noqa: E402

commit = sys.argv[1]
out = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN
doc = {"commit": commit, "library": "MG3D_LIB_PATH" if lib_path else "tree", "cases": {c: T.run_case(c) for c in sorted(T.CASES)}}
with open(out, "w") as f:
    json.dump(doc, f, indent=1, sort_keys=True)
    f.write("\n")
print(f"{len(doc['cases'])} cases from commit {commit} -> {out}")
