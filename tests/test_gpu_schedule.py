"""The launches a context makes, pinned: for each configuration a fixed call sequence runs under timing_enable(1) and the
whole table {(level, kernel name): launches} of Solver.kernel_times() plus the per-stage call counts of Solver.timing() must
equal tests/golden/schedule_launches.json.  One launch added, dropped or renamed on any level fails the case.  The file is
recorded by tools/record_schedule.py from a build of the commit BEFORE a change to the host side that decides which launch
runs when (the file names that commit), never from the code under test.  What the launches compute is held bit for bit
elsewhere (test_gpu_parity, test_gpu_legs, ...); this file holds which ones run.

All cases use c = 9, so that level 1 is 17^3 (the single-workgroup level) and L = 3 / L = 5 give 33^3 / 129^3: the smallest
sizes at which each branch of the cycle driver exists."""
import json
import os

import numpy as np
import pytest

import multigrid_parallel_amd as M

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "schedule_launches.json")

_LEGS_ON = {"legs_min": 66, "legs": 1, "carry": 0}  # as tests/test_gpu_legs.py forces the legs on at 129^3
_LEGS_OFF = {"legs_min": 66, "legs": 0, "carry": 0}

# id -> (L, nu, options, environment at creation, keep_residual, boundary / operator variant)
CASES = {
    "plain_nu1": (3, 1, {}, {}, False, None),
    "plain_nu2": (3, 2, {}, {}, False, None),
    "plain_nu3": (3, 3, {}, {}, False, None),
    "tiny_cycle_off": (3, 2, {"tiny_cycle": 0}, {}, False, None),
    "tiny_off": (3, 2, {"tiny": 0}, {}, False, None),
    "lu_reduced_off": (3, 2, {"lu_reduced": 0}, {}, False, None),
    "keep_residual": (3, 2, {}, {}, True, None),
    "no_fuse": (3, 2, {}, {"MG3D_NO_FUSE": "1"}, False, None),
    "legs_on": (5, 2, _LEGS_ON, {}, False, None),
    "legs_off": (5, 2, _LEGS_OFF, {}, False, None),
    "carried": (5, 2, {"legs": 0, "carry": 1, "carry_min": 66}, {}, False, None),
    "fuse_rst2_0_nu1": (5, 1, {"fuse_rst2": 0}, {}, False, None),
    "fuse_rst2_1_nu1": (5, 1, {"fuse_rst2": 1}, {}, False, None),
    "fuse_leg_max_129": (5, 2, {"fuse_leg_max": 129}, {}, False, None),
    "fuse_up_max_0": (5, 2, {"fuse_up_max": 0}, {}, False, None),
    "periodic": (3, 2, {}, {}, False, "periodic"),
    "neumann": (3, 2, {}, {}, False, "neumann"),
    "eps": (3, 2, {}, {}, False, "eps"),
}


def run_case(case):
    """the call sequence of one case; returns {"kernels": {"level:name": launches}, "stages": {"level:stage": calls}}"""
    L, nu, options, env, keep_r, variant = CASES[case]
    saved = {k: os.environ.get(k) for k in os.environ if k.startswith("MG3D_") and k != "MG3D_LIB_PATH"}
    saved.update({k: os.environ.get(k) for k in env})
    try:
        for k in saved:  # a context reads the environment once, at creation: nothing of the caller's may leak in
            os.environ.pop(k, None)
        os.environ.update(env)
        with M.Solver(9, L, nu) as s:
            for k, v in options.items():
                s.set_option(k, v)
            if keep_r:
                s.set_keep_residual(True)
            if variant == "periodic":
                s.set_periodic(1)
            elif variant == "neumann":
                s.set_neumann(1)
            elif variant == "eps":
                x = np.linspace(0., 1., s.N)
                s.set_coefficient(1. + 0.5 * x[:, None, None] * x[None, :, None] + 0.25 * x[None, None, :])
            s.setup_test_problem()
            s.timing_enable(1)
            s.vcycles(4)
            for _ in range(3):
                s.vcycle()
            s.smooth_restrict(L - 1, nu)
            s.smooth_residual(L - 1, 1, nu)
            s.sync()
            kernels = {f"{l}:{name}": calls for (l, name), (calls, _) in s.kernel_times().items()}
            stages = {f"{l}:{name}": calls for (l, name), (calls, _) in s.timing().items() if calls}
    finally:
        for k in env:
            os.environ.pop(k, None)
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v
    return {"kernels": kernels, "stages": stages}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_covers_exactly_these_cases(golden):
    assert sorted(golden["cases"]) == sorted(CASES)
    assert golden["commit"]


@pytest.mark.parametrize("case", sorted(CASES))
def test_launches_and_stage_counts_are_the_recorded_ones(case, golden):
    got, want = run_case(case), golden["cases"][case]
    print(case, json.dumps(got, sort_keys=True))
    assert got["kernels"] == want["kernels"]
    assert got["stages"] == want["stages"]
