"""The restricting down-leg without d (csrc/mg3d_sweep_kernel.h, ND with RES == 2): under ND the r pairs a step hands to the
next step's restriction and the diff a row keeps for one step stay in registers (rlag / rkeep; the kernels with a d window
park them in LDS), and the "this column is updatable" test of the update is a lane mask formed once a step.  Neither runs with
d_zero_skip = 0, so every case is option 1 against option 0, bitwise, signed zeros included: the norms, u of every level and
-- the restriction's own output -- d of every level below the finest.

Sizes, by where r pairs and masks can go wrong: 81^3 one k-tile, four j-tiles, the last one mostly outside the grid; 97^3
several j-tiles (the coarse rows are centred on a thread's odd rows, the pair of the last one comes from the wave below);
129^3 two k-tiles and several i-chunks on 256 CUs, chunk starts on an odd and on an even plane; 161^3 a second k-tile that is
partly empty and eight j-tiles.  Each with the benchmark's problem and with a seeded random u in the interior (faces kept, d
+0 inside): there neighbouring r values do not nearly cancel, and a swapped pair or column shows in the coarse d."""
import numpy as np
import pytest
import torch  # noqa: F401  before the package, as bench.py does: the HIP runtime is torch's

import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U
from test_gpu_dnone import _cycles, _same

pytestmark = pytest.mark.gpu

SIZES = {81: (6, 5), 97: (7, 5), 129: (9, 5), 161: (11, 5)}


def _solver(N, skip):
    c, L = SIZES[N]
    s = M.Solver(c, L, 2)
    assert s.N == N
    s.set_option("legs_min", 66)  # as tests/test_gpu_dnone.py: the legs schedule at these sizes
    s.set_option("carry_min", 66)
    s.set_option("legs", 1)
    s.set_option("carry", 0)
    s.set_option("d_zero_skip", skip)
    return s


def _three(s):
    """one call of three cycles: the four-pass launch, then tapped legs only"""
    return list(s.vcycles(3))


def _setup_benchmark(N):
    return lambda s: s.setup_test_problem()


def _setup_random_u(N):
    top = SIZES[N][1] - 1

    def setup(s):
        s.setup_test_problem()
        u = s.download(MG3D_U, top).reshape(N, N, N).copy()
        u[1:-1, 1:-1, 1:-1] = np.random.default_rng(4000 + N).uniform(-1., 1., (N - 2,) * 3)
        s.upload(MG3D_U, top, u)
        d = s.download(MG3D_D, top).reshape(N, N, N)
        assert np.all(d[1:-1, 1:-1, 1:-1] == 0.) and not np.signbit(d[1:-1, 1:-1, 1:-1]).any()
    return setup


PROBLEMS = {"benchmark": _setup_benchmark, "random_u": _setup_random_u}
PATTERNS = {"calls": _cycles, "three": _three}


def _run(N, problem, pattern, skip):
    """norms, u of every level, d of every level below the finest, launches that took a kernel without d"""
    with _solver(N, skip) as s:
        s.get_details()
        PROBLEMS[problem](N)(s)
        norms = np.array(PATTERNS[pattern](s))
        top = s.num_levels - 1
        return (norms, [s.download(MG3D_U, l) for l in range(top + 1)], [s.download(MG3D_D, l) for l in range(top)],
                s.dnone_launches())


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("problem", sorted(PROBLEMS))
@pytest.mark.parametrize("N", sorted(SIZES))
def test_option_one_against_zero(N, problem, pattern):
    one, off = _run(N, problem, pattern, 1), _run(N, problem, pattern, 0)
    assert one[3] > 0, "option 1 took no kernel without d"
    assert off[3] == 0, "option 0 took a kernel without d"
    _same(one[0], off[0], "norms")
    assert np.all(np.isfinite(off[0])) and np.all(off[0] > 0.)
    assert len(one[1]) == len(off[1]) == SIZES[N][1] and len(one[2]) == len(off[2]) == SIZES[N][1] - 1
    for l, (x, y) in enumerate(zip(one[1], off[1])):
        _same(x, y, f"u of level {l}")
    for l, (x, y) in enumerate(zip(one[2], off[2])):
        _same(x, y, f"d of level {l}")
    # the restriction's output is not trivially equal: the first coarse level's d holds non-zero values
    assert np.count_nonzero(off[2][-1]) > off[2][-1].size // 4
