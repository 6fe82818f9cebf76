"""The fused launches of the binary32 / damped-Jacobi variant on seeded random u, d AND r, off the 2^k + 1 ladder and
across the k-tile seam at column 248, against V-cycles of the CPU restatement (tests/_f32_ref.py): every grid value bit
for bit, every norm to the summation order (rel 1e-12 of the exactly rounded sum), and the launches a call is meant to
reach counted from the top level's kernel timers.

Random r matters: the fused down-leg never stores r, and the face injection of the restriction reads the faces of the
level's r array, which nothing but an upload ever writes.

    (c, L) ->  N   what it reaches
    (10,3)    37   smallest paired level off the ladder; a 12-row j-tile tail of 1 row
    (6,4)     41   a 10-row tail of 1 row
    (7,4)     49   a 12-row tail of 1 row, a 10-row tail of 9 rows
    (11,5)   161   one k-tile, 41 vectors in its last wave
    (9,6)    257   two k-tiles, the second 9 columns wide; second k-block of the 64 x 4 kernels with one column
    (10,6)   289   two k-tiles, the second 41 wide; every level from 37 up is paired"""
import numpy as np
import pytest

import _f32_ref as R
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U

pytestmark = pytest.mark.gpu
SEED = 20
ALL_SHAPES = [(10, 3), (6, 4), (7, 4), (11, 5), (9, 6), (10, 6)]
KERNELS = ("pair", "pair+tap", "prolong+pair", "prolong+pair+norm", "pair+norm", "residual+restrict", "residual",
           "prolong", "sweep1")


def faces(a, N):
    m = np.ones((N, N, N), dtype=bool)
    m[1:-1, 1:-1, 1:-1] = False
    return a.reshape(N, N, N)[m]


def launches(s):
    """launches of the top level per kernel name, zeros included"""
    kt = s.kernel_times()
    assert set(kt) <= set(KERNELS), kt
    return {k: kt.get(k, (0, 0.0))[0] for k in KERNELS}


def expected_launches(nu, cycles, pairs=True, fuse=True, carry=True):
    """The top level's launches of `cycles` V-cycles in one call, read off e32_vcycle / e32_jacobi / e32_can_carry
    (csrc/mg3d_f32.hip) for a top level of at least 33 points:
      down-leg   nu sweeps as nu // 2 pairs (when pairs are on and nu >= 2) and nu % 2 (else nu) single sweeps; a carried
                 cycle's first pair is `pair+tap`; then `residual+restrict`, or with fuse off `residual` (r stored; the
                 stand-alone restriction has no timer);
      up-leg     with pairs and fuse on and nu >= 2 the prolongation rides the first pair (`prolong+pair`), else it is the
                 stand-alone `prolong`; the norm rides the last pair (`pair+norm`, or `prolong+pair+norm` when that pair
                 is also the first) unless fuse is off, single sweeps follow it, or the cycle leaves it to the next one's
                 tap; a norm nobody delivered is a `residual` launch.
    Cycles are carried (norm of cycle n tapped by cycle n + 1; the last cycle forms its own) only for nu = 2 with all
    three options on."""
    n = dict.fromkeys(KERNELS, 0)
    paired = pairs and nu >= 2
    npairs, nsingle = (nu // 2, nu % 2) if paired else (0, nu)
    carried = carry and nu == 2 and pairs and fuse
    for cyc in range(cycles):
        # down-leg
        tap = carried and cyc > 0
        n["pair+tap"] += 1 if tap else 0
        n["pair"] += npairs - (1 if tap else 0)
        n["sweep1"] += nsingle
        n["residual+restrict" if fuse else "residual"] += 1
        # up-leg
        carry_out = carried and cyc + 1 < cycles
        ride = paired and fuse  # the first pair takes the prolongation along
        if not ride:
            n["prolong"] += 1
        normed = False
        for p in range(npairs):
            with_norm = fuse and not carry_out and p == npairs - 1 and nsingle == 0
            with_pro = ride and p == 0
            n["prolong+pair+norm" if with_norm and with_pro else "pair+norm" if with_norm else "prolong+pair" if with_pro else "pair"] += 1
            normed = with_norm
        n["sweep1"] += nsingle
        if not normed and not carry_out:
            n["residual"] += 1
    return n


def test_expected_launches_of_the_documented_cases():
    """the counts the V(2,2) x 3 default is known to make, and the ones each other sweep count must reach"""
    e = expected_launches(2, 3)
    assert (e["pair"], e["pair+tap"], e["prolong+pair"], e["prolong+pair+norm"], e["residual+restrict"]) == (1, 2, 2, 1, 3)
    assert sum(e.values()) == 9
    assert expected_launches(4, 3)["pair+norm"] == 3
    e = expected_launches(3, 3)
    assert e["sweep1"] == 6 and e["residual"] == 3 and e["pair"] == 3 and e["prolong+pair"] == 3
    e = expected_launches(0, 3)
    assert e["prolong"] == 3 and e["residual"] == 3 and e["residual+restrict"] == 3
    assert expected_launches(2, 3, fuse=False)["residual+restrict"] == 0
    assert expected_launches(2, 3, carry=False)["pair+tap"] == 0


def upload_start(s, c, L, start):
    top = L - 1
    for f, a in zip((MG3D_U, MG3D_D, MG3D_R), start):
        s.upload(f, top, a)


def check_norms(what, got, cycles):
    want = np.array([cyc.norm for cyc in cycles])
    print(f"{what}: norm / exactly rounded - 1 =", " ".join(f"{x:+.3e}" for x in got / want - 1))
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


def check_levels(s, c, L, cyc, what):
    """top u, and u and d of every level below it, against one recorded cycle"""
    sizes = R.O.level_sizes(c, L)
    R.assert_same_bits(s.download(MG3D_U, L - 1), cyc.u_top, sizes[-1], L - 1, f"{what}: u")
    for l in range(L - 2, -1, -1):  # d first, from the top down: the order the cycle forms them in
        R.assert_same_bits(s.download(MG3D_D, l), cyc.d_low[l], sizes[l], l, f"{what}: d")
    for l in range(L - 1):  # u from the bottom up
        R.assert_same_bits(s.download(MG3D_U, l), cyc.u_low[l], sizes[l], l, f"{what}: u")


@pytest.mark.parametrize("point", [(5, 11, 23), (23, 5, 11)])
def test_one_point_tells_the_axes_apart(point):
    """(e) 37^3, d = r = 0, u = 1 at one interior point whose three indices differ: one V(2,2) cycle bit for bit.  A
    transposed parent, a swapped j/k offset or a mixed-up axis moves the image of the point; where it lands says which."""
    c, L, nu = 10, 3, 2
    N = R.O.level_sizes(c, L)[-1]
    u0 = np.zeros((N, N, N), dtype=np.float32)
    u0[point] = 1.0
    start = (u0.reshape(-1), np.zeros(N ** 3, dtype=np.float32), np.zeros(N ** 3, dtype=np.float32))
    ref = R.run_cycles(c, L, nu, 1, *start)
    assert np.count_nonzero(ref[0].u_top) > 100 and np.count_nonzero(ref[0].d_low[L - 2]) > 20  # the point spreads
    with M.Solver32(c, L, nu, R.OMEGA) as s:
        upload_start(s, c, L, start)
        norms = s.vcycles(1)
        check_levels(s, c, L, ref[0], f"point {point}")
    check_norms(f"point {point}", norms, ref)


@pytest.mark.parametrize("c,L", ALL_SHAPES)
def test_one_cycle_every_level(c, L):
    """(a) one V(2,2) cycle from random u, d and r: `pair`, `residual+restrict` with the faces of r, `prolong+pair+norm`
    on the top level; `prolong+pair` on the levels below down to 33 points, the unpaired kernels under that."""
    nu = 2
    N = R.O.level_sizes(c, L)[-1]
    start = R.random_start(c, L, SEED)
    ref = R.random_cycles(c, L, nu, 1, SEED)
    assert np.isfinite(ref[0].u_top).all()
    with M.Solver32(c, L, nu, R.OMEGA) as s:
        upload_start(s, c, L, start)
        s.timing_enable()
        norms = s.vcycles(1)
        check_levels(s, c, L, ref[0], f"({c},{L}) {N}^3")
        r_after = s.download(MG3D_R, L - 1)
        assert R.same_bits(faces(r_after, N), faces(start[2], N)), "the faces of r changed"
        assert launches(s) == expected_launches(nu, 1)
    check_norms(f"one cycle ({c},{L}) {N}^3", norms, ref)


# shape by shape, V(2,2) last: the knob variants below share its CPU run
@pytest.mark.parametrize("c,L,nu", [(c, L, nu) for c, L in [(10, 3), (10, 6), (9, 6)] for nu in (0, 1, 3, 4, 2)])
def test_every_launch_combination(c, L, nu):
    """(b) three cycles in one call.  nu = 0: `prolong` alone and `residual`; 1: `sweep1`, stand-alone `prolong`; 2: the
    carried cycles (`pair+tap` twice, ending on `prolong+pair` twice); 3: pair + single sweep, so `residual` forms the
    norm; 4: two pairs a leg, `pair+norm`."""
    cycles = 3
    N = R.O.level_sizes(c, L)[-1]
    ref = R.random_cycles(c, L, nu, cycles, SEED)
    assert all(np.isfinite(cyc.u_top).all() for cyc in ref)
    with M.Solver32(c, L, nu, R.OMEGA) as s:
        upload_start(s, c, L, R.random_start(c, L, SEED))
        s.timing_enable()
        norms = s.vcycles(cycles)
        R.assert_same_bits(s.download(MG3D_U, L - 1), ref[-1].u_top, N, L - 1, f"({c},{L}) nu = {nu}: u")
        got, want = launches(s), expected_launches(nu, cycles)
    print(f"({c},{L}) nu = {nu} launches:", {k: v for k, v in got.items() if v})
    assert got == want
    named = {0: ("prolong", "residual"), 1: ("sweep1", "prolong"), 2: ("pair+tap", "prolong+pair", "prolong+pair+norm", "residual+restrict"),
             3: ("pair", "prolong+pair", "sweep1", "residual"), 4: ("pair", "prolong+pair", "pair+norm")}[nu]
    assert all(got[k] >= 1 for k in named), got
    check_norms(f"({c},{L}) {N}^3 nu = {nu}", norms, ref)


@pytest.mark.parametrize("knob", ["pairs", "fuse", "carry"])
def test_launch_knobs_on_random_data(knob):
    """(c) 257^3, V(2,2) x 3 with one launch option off: the same bits as the restatement (not merely as each other), and
    the timers show that the launches did change."""
    c, L, nu, cycles = 9, 6, 2, 3
    N = R.O.level_sizes(c, L)[-1]
    ref = R.random_cycles(c, L, nu, cycles, SEED)
    with M.Solver32(c, L, nu, R.OMEGA) as s:
        s.set_option(knob, 0)
        upload_start(s, c, L, R.random_start(c, L, SEED))
        s.timing_enable()
        norms = s.vcycles(cycles)
        check_levels(s, c, L, ref[-1], f"{knob} off")
        got = launches(s)
    print(f"{knob} off launches:", {k: v for k, v in got.items() if v})
    assert got == expected_launches(nu, cycles, **{knob: False})
    assert got != expected_launches(nu, cycles)
    if knob == "fuse":
        assert got["residual+restrict"] == 0 and got["residual"] == 2 * cycles
    if knob == "carry":
        assert got["pair+tap"] == 0 and got["prolong+pair+norm"] == cycles
    if knob == "pairs":
        assert got["sweep1"] == 4 * cycles and got["pair"] == 0
    check_norms(f"{knob} off", norms, ref)


@pytest.mark.parametrize("c,L", [(4, 2), (10, 2), (10, 3), (7, 4), (9, 6), (10, 6)])
def test_operators_past_one_block(c, L):
    """(d) the stand-alone operators (tests/test_gpu_f32.py holds them up to 33^3) at 7^3, at 19^3 (N mod 4 = 3, which
    only two levels give), off the ladder, and at 257^3 / 289^3 with a second block in k; one to four sweeps."""
    R.check_operators(c, L, sweeps=(1, 2, 3, 4), sequential_norm=False)
