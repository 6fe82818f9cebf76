"""The zero-guess down-leg in one launch (csrc/mg3d_sweep_kernel.h ZF with RES = 2, option fuse_down_min): a coarse level's
V(2,2) pre-smoother from the zero guess, its residual and the restriction of it run as ONE launch -- the zero front, black,
red, black, the residual stage, full weighting into the coarse right-hand side -- instead of the front's three-pass launch
followed by residual + restriction.  fuse_down_min = 0 runs none of it, so every case is the option forced low (17: every level
that starts from the zero guess with a sweep launch) against option 0, bitwise, signed zeros included: the norms of two cycles,
u of every level and d of every level below the finest.  mg3d_ctx_sweep_taken says which ran: the fused launch's record is of
kind PASSES_RES with S = 3 and RES = 2, which no other launch has; with the option on there is one for every zero-guess sweep
level and the front's own record (kind PASSES, S = 3) is gone from those levels, with option 0 there is none.  All with
sweep_tune = 0.

Sizes (c, L) as tests/test_gpu_zero_front.py, by where the launch can go wrong: 65^3 the zero guess on 33^3, one k-tile, two
j-tiles of which the second is mostly outside; 81^3 on 21^3 and 41^3, off the 2^k+1 ladder, both face parities; 161^3 on 41^3
and 81^3; 193^3 on 25^3, 49^3 and 97^3; 257^3 on 33^3, 65^3 and 129^3, two k-tiles -- the restriction crosses a tile seam --
and several chunks.  One case per size also holds u of the finest level and the norms to the oracle.
Variations at 81^3 and 193^3: the chunk length (chunks start on odd and on even planes: the front's colour and the coarse plane
a chunk owns both depend on it), the three compiled shapes on every level, a random right-hand side, values planted on the
faces of r of every level (the face injection carries them to the faces of every coarser d), the screened operator, nu = 1
and nu = 3 (no four-pass pre-smoother: the option changes nothing, no record).
The default (130): none at 257^3, whose largest zero-guess level is 129^3; at 273^3 = (18, 5) -- levels 18, 35, 69, 137, 273,
the smallest top level whose first coarse level exceeds 129; 35 > 17, so level 1 runs sweep launches too -- only on 137^3."""
import numpy as np
import pytest
import torch  # noqa: F401  before the package, as bench.py does: the HIP runtime is torch's

import _oracle as O
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U
from test_gpu_dnone import _same
from test_gpu_parity import norm_rtol
from test_gpu_zero_front import PROBLEMS, SIZES, VARIED

pytestmark = pytest.mark.gpu

LOW = 17  # fuse_down_min forced below every level that runs sweep launches
SHAPES = ((2, 8, 2), (4, 8, 1), (4, 8, 2))
DEFAULT_BIG = (4, 8, 1)  # levels above small_max (129)
BIG = {273: (18, 5)}
ALL_SIZES = {**SIZES, **BIG}


def run(N, down, problem="benchmark", nu=2, sigma=0., options=None, cycles=2):
    """norms, u of every level, d of every level below the finest, the records of kind PASSES and of kind PASSES_RES;
    down None: the option's default"""
    c, L = ALL_SIZES[N]
    with M.Solver(c, L, nu) as s:
        assert s.N == N
        opts = dict(options or {}, sweep_tune=0)
        if down is not None:
            opts["fuse_down_min"] = down
        for k, v in opts.items():
            s.set_option(k, v)
        if sigma:
            s.set_shift(sigma)
        PROBLEMS[problem](s, N)
        norms = np.array(s.vcycles(cycles))
        assert np.all(np.isfinite(norms)) and np.all(norms > 0.)
        return (norms, [s.download(MG3D_U, l) for l in range(L)], [s.download(MG3D_D, l) for l in range(L - 1)],
                s.sweep_taken("passes")[1], s.sweep_taken("passes_res")[1])


def fused(recs):
    return [r for r in recs if r["S"] == 3 and r["RES"] == 2]


def fronts(recs):
    return [r for r in recs if r["S"] == 3]


def assert_same_bits(N, on, off):
    L = ALL_SIZES[N][1]
    _same(on[0], off[0], "norms")
    assert len(on[1]) == len(off[1]) == L and len(on[2]) == len(off[2]) == L - 1
    for l, (x, y) in enumerate(zip(on[1], off[1])):
        _same(x, y, f"u of level {l}")
    for l, (x, y) in enumerate(zip(on[2], off[2])):
        _same(x, y, f"d of level {l}")


def assert_record(r, shape):
    assert (r["PRO"], r["ND"], r["DZ"], r["TAP"], r["DP"]) == (0, 0, 0, -1, 0), r
    assert (r["RJ"], r["NW"], r["PF"]) == shape, r
    vj = r["RJ"] * r["NW"] - 10  # a halo of five rows on either side
    assert r["ntj"] == -(-r["N"] // vj) and r["blocks"] == r["ntj"] * r["ntk"] * -(-r["N"] // r["CI"]), r
    assert r["ntk"] == (1 if r["N"] <= 128 else 2), r


def assert_on_against_off(N, nu=2, shape=None, **kw):
    on, off = run(N, LOW, nu=nu, **kw), run(N, 0, nu=nu, **kw)
    assert not fused(off[4]), "option 0 ran the fused launch"
    if nu != 2:
        assert not fused(on[4]), "no four-pass pre-smoother in this cycle: nothing to fuse"
        assert [(r["N"], r["S"]) for r in on[3]] == [(r["N"], r["S"]) for r in off[3]]
    else:
        # the zero-guess sweep levels: where option 0 runs the front's own launch
        zero_guess = {r["N"] for r in fronts(off[3])}
        c, L = SIZES[N]
        assert zero_guess >= {(c - 1) * (1 << l) + 1 for l in range(2, L - 1)}, zero_guess
        assert sorted(r["N"] for r in fused(on[4])) == sorted(zero_guess), fused(on[4])
        assert not [r for r in fronts(on[3]) if r["N"] in zero_guess], "the front's own launch is left on a fused level"
        for r in fused(on[4]):
            assert_record(r, shape or ((2, 8, 2) if r["N"] <= 129 else DEFAULT_BIG))
            assert r["count"] == 2, r  # one launch a cycle
    assert_same_bits(N, on, off)
    # not trivially equal: the levels the launch ran on hold a correction and a restricted residual below them
    L = SIZES[N][1]
    for l in range(2, L - 1):
        assert np.count_nonzero(off[1][l]) > off[1][l].size // 4
        assert np.count_nonzero(off[2][l - 1]) > off[2][l - 1].size // 4
    return on


_oracle = {}


def oracle(N, cycles):
    if (N, cycles) not in _oracle:
        c, L = SIZES[N]
        lib = O.lib()
        lib.orc_set_threads(8)
        try:
            norms, u, _, _ = O.run_problem(c, L, 2, cycles)
        finally:
            lib.orc_set_threads(1)
        _oracle[(N, cycles)] = (norms, u)
    return _oracle[(N, cycles)]


@pytest.mark.parametrize("N", sorted(SIZES))
def test_fused_against_two_launches_and_the_oracle(N):
    on = assert_on_against_off(N)
    want_norms, want_u = oracle(N, 2)
    _same(on[1][-1], want_u, "u of the finest level against the oracle")
    np.testing.assert_allclose(on[0], want_norms, rtol=norm_rtol(N))


@pytest.mark.parametrize("ci", [1, 2, 3, 5])
@pytest.mark.parametrize("N", VARIED)
def test_chunk_lengths(N, ci):
    on = assert_on_against_off(N, problem="rhs", options=dict(sweep_ci=ci))
    assert all(r["CI"] == ci for r in fused(on[4]))


@pytest.mark.parametrize("shape", SHAPES, ids=["%d.%d.%d" % sh for sh in SHAPES])
@pytest.mark.parametrize("N", VARIED)
def test_every_compiled_shape_on_every_level(N, shape):
    rj, nw, pf = shape
    assert_on_against_off(N, problem="rhs", shape=shape, options=dict(sweep_rj=rj, sweep_nw=nw, sweep_pf=pf))


@pytest.mark.parametrize("problem", ["rhs", "faces"])
@pytest.mark.parametrize("N", VARIED)
def test_problems(N, problem):
    on = assert_on_against_off(N, problem=problem)
    if problem == "faces":  # the planted values arrived on the faces of every coarser d
        for d in on[2][1:]:
            n = round(d.size ** (1. / 3.))
            assert np.all(d.reshape(n, n, n)[0] >= 1.) and np.all(d.reshape(n, n, n)[:, :, -1] >= 1.)


@pytest.mark.parametrize("N", VARIED)
def test_screened_operator(N):
    assert_on_against_off(N, problem="faces", sigma=37.5)


@pytest.mark.parametrize("nu", [1, 3])
@pytest.mark.parametrize("N", VARIED)
def test_other_cycles(N, nu):
    assert_on_against_off(N, nu=nu, problem="faces")


def test_the_default_leaves_129_alone():
    dflt = run(257, None)
    assert not fused(dflt[4]), "129^3 is below the default of 130"
    assert {r["N"] for r in fronts(dflt[3])} >= {33, 65, 129}


def test_the_default_takes_137():
    N = 273
    with M.Solver(*BIG[N], 2) as s:
        assert s.get_option("fuse_down_min") == 130 and [s.level_n(l) for l in range(5)] == [18, 35, 69, 137, 273]
    dflt, off = run(N, None), run(N, 0)
    assert not fused(off[4])
    assert {r["N"] for r in fronts(off[3])} == {35, 69, 137}  # (level 1 is too large for the single-workgroup kernel)
    assert [r["N"] for r in fused(dflt[4])] == [137], fused(dflt[4])
    assert_record(fused(dflt[4])[0], DEFAULT_BIG)
    assert {r["N"] for r in fronts(dflt[3])} == {35, 69}
    assert_same_bits(N, dflt, off)
    assert np.count_nonzero(off[1][3]) > off[1][3].size // 4 and np.count_nonzero(off[2][2]) > off[2][2].size // 4
