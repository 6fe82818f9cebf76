"""The zero front (csrc/mg3d_sweep_kernel.h ZF, option zero_front): the launch that starts a coarse level's pre-smoother from the
zero guess runs a THREE-pass kernel on an input it forms from d as a plane arrives -- sixth * (0 - hSq * d) at every updatable
red point, +0.0 everywhere else -- instead of the four-pass kernel on an input that is not read.  zero_front = 0 runs none of
the front's code (from the zero guess it takes the sixteen-wave four-pass kernel, the one four-pass shape whose plane load still
tests for an absent input), so every case is option 1 against option 0, bitwise, signed zeros included: the norms, u of every level and d of
every level below the finest.  mg3d_ctx_sweep_taken says which ran: the front's record is of kind PASSES with S = 3, which no
other launch has; with option 1 there is one for every level that has a zero-guess sweep launch -- the levels that run the four-pass kernel from
the zero guess under option 0: levels 2 .. L - 2 (the finest has an input) and level 1 where it is too large for the
single-workgroup kernel (21^3 below 161^3) --, with option 0 none.  All with sweep_tune = 0.

Sizes (c, L), by where the front can go wrong: 65^3 the zero guess on 33^3, two j-tiles of which the second is mostly outside;
81^3 on 21^3 and 41^3, off the 2^k+1 ladder, odd and even face parities; 193^3 on 25^3, 49^3 and 97^3, the 16-wave shape with
four j-tiles and one k-tile; 161^3 on 41^3 and 81^3; 257^3 on 33^3, 65^3 and 129^3, the 16-wave shape with two k-tiles and
several chunks on 256 CUs.  One case per size also holds u of the finest level and the norms to the oracle.
Variations at 81^3 and 193^3: the chunk length (chunk starts on odd and on even planes: the front's colour depends on the
plane), the three compiled tile shapes on every level, a random right-hand side, values planted on the faces of r of every
level (the face injection carries them to the faces of the coarser d: a front that forgets its masks shows in u), the screened
operator, nu = 3 (more launches behind the front) and nu = 1 (no four-pass launch: the option changes nothing, no record).
One case on two loopback slabs at 129^3 (the slab path keeps no records: the bits alone)."""
import numpy as np
import pytest
import torch  # noqa: F401  before the package, as bench.py does: the HIP runtime is torch's

import _oracle as O
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U
from test_gpu_dnone import _same
from test_gpu_parity import norm_rtol

pytestmark = pytest.mark.gpu

SIZES = {65: (9, 4), 81: (6, 5), 161: (11, 5), 193: (7, 6), 257: (9, 6)}
VARIED = (81, 193)
SHAPES = ((2, 8, 2), (2, 16, 1), (4, 8, 1))


def _benchmark(s, N):
    s.setup_test_problem()


def _random_rhs(s, N):
    s.setup_test_problem()
    top = s.num_levels - 1
    d = s.download(MG3D_D, top).reshape(N, N, N).copy()
    d[1:-1, 1:-1, 1:-1] = np.random.default_rng(9100 + N).uniform(-50., 50., (N - 2,) * 3)
    s.upload(MG3D_D, top, d)


def _faces_of_r(s, N):
    """the random right-hand side, and r of every level above the coarsest +0 inside with non-zero faces: the restriction
    injects them into the faces of the next coarser d"""
    _random_rhs(s, N)
    for l in range(1, s.num_levels):
        n = s.level_n(l)
        r = np.random.default_rng(9200 + 10 * N + l).uniform(1., 2., (n, n, n))
        r[1:-1, 1:-1, 1:-1] = 0.
        s.upload(MG3D_R, l, r)


PROBLEMS = {"benchmark": _benchmark, "rhs": _random_rhs, "faces": _faces_of_r}


def run(N, front, problem="benchmark", nu=2, sigma=0., options=None, cycles=2):
    """norms, u of every level, d of every level below the finest, the records of kind PASSES"""
    c, L = SIZES[N]
    with M.Solver(c, L, nu) as s:
        assert s.N == N
        for k, v in dict(options or {}, sweep_tune=0, zero_front=front).items():
            s.set_option(k, v)
        if sigma:
            s.set_shift(sigma)
        PROBLEMS[problem](s, N)  # (builds the coarse factor of the context's sigma)
        norms = np.array(s.vcycles(cycles))
        assert np.all(np.isfinite(norms)) and np.all(norms > 0.)
        return (norms, [s.download(MG3D_U, l) for l in range(L)], [s.download(MG3D_D, l) for l in range(L - 1)],
                s.sweep_taken("passes")[1])


def front_levels(N):
    """points per side of the levels whose pre-smoother starts with a sweep launch from the zero guess"""
    c, L = SIZES[N]
    return {(c - 1) * (1 << l) + 1 for l in range(2, L - 1)}


def fronts(recs):
    return [r for r in recs if r["S"] == 3]


def assert_one_against_zero(N, nu=2, shape=None, **kw):
    one, off = run(N, 1, nu=nu, **kw), run(N, 0, nu=nu, **kw)
    L = SIZES[N][1]
    assert not fronts(off[3]), "option 0 ran the front"
    if nu == 1:
        assert not fronts(one[3]), "no four-pass launch from the zero guess in a V(1,1) cycle"
    else:
        # the levels that start from the zero guess with a sweep launch: with option 0 they take the four-pass kernel (the
        # only launch of kind PASSES below the finest level that has four passes and no prolongation)
        zero_guess = {r["N"] for r in off[3] if r["S"] == 4 and r["PRO"] == 0 and r["N"] < N}
        assert zero_guess >= front_levels(N), (zero_guess, front_levels(N))
        assert {r["N"] for r in fronts(one[3])} == zero_guess, fronts(one[3])
        if nu == 2:
            assert not [r for r in one[3] if r["S"] == 4 and r["PRO"] == 0 and r["N"] < N], "a four-pass launch from the zero guess is left"
        for r in fronts(one[3]):
            assert (r["RES"], r["PRO"], r["ND"], r["DZ"], r["TAP"]) == (0, 0, 0, 0, -1), r
            dflt = (2, 8, 2) if r["N"] <= 65 else (2, 16, 1) if r["N"] <= 300 else (4, 8, 1)
            assert (r["RJ"], r["NW"], r["PF"]) == (shape or dflt), r
            vj = r["RJ"] * r["NW"] - 6  # a halo of three rows on either side
            assert r["ntj"] == -(-r["N"] // vj) and r["blocks"] == r["ntj"] * r["ntk"] * -(-r["N"] // r["CI"]), r
    _same(one[0], off[0], "norms")
    assert len(one[1]) == len(off[1]) == L and len(one[2]) == len(off[2]) == L - 1
    for l, (x, y) in enumerate(zip(one[1], off[1])):
        _same(x, y, f"u of level {l}")
    for l, (x, y) in enumerate(zip(one[2], off[2])):
        _same(x, y, f"d of level {l}")
    # not trivially equal: the levels the front ran on hold a correction
    for l in range(2, L - 1):
        assert np.count_nonzero(off[1][l]) > off[1][l].size // 4
    return one


@pytest.mark.parametrize("N", sorted(SIZES))
def test_front_against_four_passes_and_the_oracle(N):
    cycles = 2
    one = assert_one_against_zero(N, cycles=cycles)
    c, L = SIZES[N]
    lib = O.lib()
    lib.orc_set_threads(8)
    try:
        want_norms, want_u, _, _ = O.run_problem(c, L, 2, cycles)
    finally:
        lib.orc_set_threads(1)
    _same(one[1][-1], want_u, "u of the finest level against the oracle")
    np.testing.assert_allclose(one[0], want_norms, rtol=norm_rtol(N))


@pytest.mark.parametrize("ci", [1, 2, 3, 5])
@pytest.mark.parametrize("N", VARIED)
def test_chunk_lengths(N, ci):
    one = assert_one_against_zero(N, problem="rhs", options=dict(sweep_ci=ci))
    assert all(r["CI"] == ci for r in fronts(one[3]))


@pytest.mark.parametrize("shape", SHAPES, ids=["%d.%d.%d" % sh for sh in SHAPES])
@pytest.mark.parametrize("N", VARIED)
def test_every_compiled_front_shape_on_every_level(N, shape):
    rj, nw, pf = shape
    assert_one_against_zero(N, problem="rhs", shape=shape, options=dict(sweep_rj=rj, sweep_nw=nw, sweep_pf=pf))


@pytest.mark.parametrize("N", VARIED)
def test_a_shape_without_a_front_runs_the_default_front(N):
    assert_one_against_zero(N, options=dict(sweep_rj=2, sweep_nw=8, sweep_pf=4))


@pytest.mark.parametrize("problem", ["rhs", "faces"])
@pytest.mark.parametrize("N", VARIED)
def test_problems(N, problem):
    one = assert_one_against_zero(N, problem=problem)
    if problem == "faces":  # the planted values arrived on the faces of every coarser d
        for d in one[2][1:]:
            n = round(d.size ** (1. / 3.))
            assert np.all(d.reshape(n, n, n)[0] >= 1.) and np.all(d.reshape(n, n, n)[:, :, -1] >= 1.)


@pytest.mark.parametrize("N", VARIED)
def test_screened_operator(N):
    assert_one_against_zero(N, problem="faces", sigma=37.5)


@pytest.mark.parametrize("nu", [1, 3])
@pytest.mark.parametrize("N", VARIED)
def test_other_cycles(N, nu):
    assert_one_against_zero(N, nu=nu, problem="faces")


def test_two_slabs(monkeypatch):
    monkeypatch.setenv("MG3D_SLAB_MIN_PLANES", "8")
    c, L, nu = 9, 5, 2
    got = []
    for front in (1, 0):
        with M.DistSolver(c, L, nu, nranks=2) as d:
            assert d.first_level <= 2  # a distributed level starts from the zero guess
            d.set_option("sweep_tune", 0)
            d.set_option("zero_front", front)
            d.setup_test_problem()
            norms = np.array(d.vcycles(3))
            got.append((norms, [d.download(MG3D_U, l) for l in range(L)], [d.download(MG3D_D, l) for l in range(L - 1)]))
    one, off = got
    _same(one[0], off[0], "norms")
    for l in range(L):
        _same(one[1][l], off[1][l], f"u of level {l}")
    for l in range(L - 1):
        _same(one[2][l], off[2][l], f"d of level {l}")
    with M.Solver(c, L, nu) as s:
        s.set_option("sweep_tune", 0)
        s.setup_test_problem()
        s.vcycles(3)
        _same(one[1][-1], s.download(MG3D_U, L - 1), "u of the finest level against the single domain")
