"""The leg kernels without d (csrc/mg3d_sweep_kernel.h ND, option d_zero_skip = 1): when the zero map of the finest level's d is
full -- +0.0 at every interior point -- the two leg launches run kernels that hold no d window and never look at d or its map.
The bar: u of EVERY level and every norm are bitwise equal, signed zeros included, to the same run with d_zero_skip = 2 (the map
only: the kernels that form the +0.0 planes in registers) and with d_zero_skip = 0 (every plane read); neither runs the new
code.  The counter mg3d_ctx_dnone_launches says which runs took the new kernels: only option 1, and only while the map is
full.  h^2 * (+0.0) = +0.0 and x - (+0.0) = x for every x; the residual stays 0. - (...), so a zero residual is +0."""
import numpy as np
import pytest
import torch  # before the package, as bench.py does: the HIP runtime is torch's

import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U

pytestmark = pytest.mark.gpu

VALID = 2  # mg3d_ctx_dzero_planes' state
# 97^3: one k-tile, several j-tiles; 129^3: two k-tiles and more than one i-chunk on a 256-CU part
SIZES = {97: (7, 5), 129: (9, 5)}


def _solver(N, skip, nu=2):
    c, L = SIZES[N]
    s = M.Solver(c, L, nu)
    assert s.N == N
    s.set_option("legs_min", 66)  # as tests/test_gpu_legs.py: the legs schedule at these sizes
    s.set_option("carry_min", 66)
    s.set_option("legs", 1)
    s.set_option("carry", 0)
    s.set_option("d_zero_skip", skip)
    return s


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b, what=""):
    """bitwise: signed zeros and NaN payloads included"""
    assert np.array_equal(_bits(a), _bits(b)), what


def _same_runs(a, b, what):
    _same(a[0], b[0], f"{what}: norms")
    assert len(a[1]) == len(b[1])
    for l, (x, y) in enumerate(zip(a[1], b[1])):
        _same(x, y, f"{what}: u of level {l}")


def _cycles(s):
    """three mg3d_vcycles calls and one mg3d_vcycle: the first cycle behind nothing (four-pass launch), the tapped and the
    untapped legs, the first cycle of a call behind a red pass (red_tail), the down-leg that runs ahead behind mg3d_vcycle and
    the call that picks it up"""
    norms = list(s.vcycles(2)) + list(s.vcycles(1))
    norms.append(s.vcycle())
    norms += list(s.vcycles(2))
    return norms


def _run(N, skip, setup, nu=2, cycles=_cycles):
    """norms, u of every level, launches that took a kernel without d"""
    with _solver(N, skip, nu) as s:
        s.get_details()
        setup(s)
        norms = cycles(s)
        return np.array(norms), [s.download(MG3D_U, l) for l in range(s.num_levels)], s.dnone_launches()


_LAPLACE = {}


def laplace_d(N):
    """the benchmark's right-hand side: +0 inside, the reference's boundary function on the faces"""
    if N not in _LAPLACE:
        with _solver(N, 0) as s:
            s.setup_test_problem()
            _LAPLACE[N] = s.download(MG3D_D, s.num_levels - 1).reshape(N, N, N)
    return _LAPLACE[N].copy()


def _faces_mask(N):
    m = np.zeros((N, N, N), dtype=bool)
    m[0] = m[-1] = True
    m[:, 0] = m[:, -1] = True
    m[:, :, 0] = m[:, :, -1] = True
    return m


# ------------------------------------------------------------------------------------------------ 1. the benchmark's problem
@pytest.mark.parametrize("N", [97, 129])
def test_benchmark_problem_three_options(N):
    def setup(s):
        s.setup_test_problem()
    one, two, off = (_run(N, k, setup) for k in (1, 2, 0))
    _same_runs(one, off, "option 1 against 0")
    _same_runs(two, off, "option 2 against 0")
    assert one[2] > 0
    assert two[2] == 0 and off[2] == 0


# ------------------------------------------------------------------------------------------- 2. faces of d that nobody may use
@pytest.mark.parametrize("N", [97, 129])
def test_random_faces_of_d_are_not_used(N):
    """every face entry of d, planes 0 and N - 1 included, is a seeded random finite value or -0.0; the interior is +0.0.  The
    kernel without d never reads them, the yardsticks read them and must not use them"""
    rng = np.random.default_rng(1000 + N)
    faces = _faces_mask(N)
    d = np.zeros((N, N, N))
    vals = rng.uniform(-1e3, 1e3, int(faces.sum()))
    vals[rng.random(vals.size) < 0.2] = -0.0
    d[faces] = vals
    assert np.signbit(d[faces]).any() and not np.signbit(d[~faces]).any() and np.all(d[~faces] == 0.)
    top = SIZES[N][1] - 1

    def setup(s):
        s.setup_test_problem()
        s.upload(MG3D_D, top, d)
    one, two, off = (_run(N, k, setup) for k in (1, 2, 0))
    _same_runs(one, off, "option 1 against 0")
    _same_runs(two, off, "option 2 against 0")
    assert one[2] > 0 and two[2] == 0 and off[2] == 0


# ---------------------------------------------------------------------------------------------- 3. a map that is not full
@pytest.mark.parametrize("N", [97, 129])
@pytest.mark.parametrize("value", [0.75, -0.0])
def test_one_point_keeps_the_d_kernels(N, value):
    """one non-zero interior point, one interior -0.0: the map misses a plane, no launch takes a kernel without d"""
    top = SIZES[N][1] - 1
    d = laplace_d(N)
    d[N // 2, N // 3, N - 2] = value

    def setup(s):
        s.setup_test_problem()
        s.upload(MG3D_D, top, d)
    one, off = _run(N, 1, setup), _run(N, 0, setup)
    _same_runs(one, off, "option 1 against 0")
    assert one[2] == 0 and off[2] == 0


# ------------------------------------------------------------------------------------------------ 4. one solver, d changing
@pytest.mark.parametrize("N", [97, 129])
def test_the_counter_follows_d(N):
    """full-zero d, then a d with one non-zero point, then mg3d_zero + mg3d_fill_boundary: the counter rises, stands still,
    rises again; the bits are those of the same sequence with the option off"""
    top = SIZES[N][1] - 1
    d1 = laplace_d(N)
    d1[3, N - 2, 5] = -2.5
    res = []
    for skip in (1, 0):
        with _solver(N, skip) as s:
            out, counts = [], []
            s.setup_test_problem()
            out += [s.vcycles(2), s.vcycle()]
            counts.append(s.dnone_launches())
            s.upload(MG3D_D, top, d1)
            out += [s.vcycles(2), s.vcycle()]
            counts.append(s.dnone_launches())
            s.zero(MG3D_D, top)
            s.fill_boundary(MG3D_D, top)
            out += [s.vcycles(2), s.vcycle(), s.vcycles(1)]
            counts.append(s.dnone_launches())
            out += [s.download(MG3D_U, l) for l in range(top + 1)]
            res.append((out, counts))
    for n, (a, b) in enumerate(zip(res[0][0], res[1][0])):
        _same(a, b, f"item {n}")
    c = res[0][1]
    assert 0 < c[0] == c[1] < c[2], c
    assert res[1][1] == [0, 0, 0]


# ------------------------------------------------------------------------------------------------------- 5. a screened solve
@pytest.mark.parametrize("N", [97, 129])
def test_screened_solve(N):
    """sigma > 0: dg != 6 in the residual"""
    def setup(s):
        s.set_shift(37.5)
        s.setup_test_problem()
    one, off = _run(N, 1, setup), _run(N, 0, setup)
    _same_runs(one, off, "option 1 against 0")
    assert one[2] > 0 and off[2] == 0


# ------------------------------------------------------------------------------------------------ 6. other iteration counts
@pytest.mark.parametrize("nu", [1, 3])
def test_other_iteration_counts(nu):
    """V(1,1) and V(3,3) at 129^3: the same bits whichever kernels those schedules take"""
    def setup(s):
        s.setup_test_problem()
    one, off = _run(129, 1, setup, nu=nu), _run(129, 0, setup, nu=nu)
    _same_runs(one, off, "option 1 against 0")
    assert off[2] == 0
