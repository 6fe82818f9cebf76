"""The screened operator  Delta_h u - sigma u = d  on every kernel variant of the single-domain context, against the numpy
reference of tests/_screened_ref.py bit for bit.  At sigma = 0 every level shares dg = 6 and sixth = 1/6, so the constant
tests cannot see a launch that drops its LevelOp, takes a coarser level's or reads sigma from another context: here every
variant, schedule and option runs with sigma > 0 (1e-12 too, where dg == 6 on the finest levels only), on the test problem
and on random data, split over several calls, and shows that it ran.  Also the single operators, the FMG start, state
changes between calls, and 513^3 against the C oracle's screened twin (orc_run_problem_shift)."""
import os

import numpy as np
import pytest

import _oracle as O
import _screened_ref as S
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U

from test_gpu_parity import EXACT_NORM_RTOL, norm_rtol

pytestmark = pytest.mark.gpu

CALLS = (1, 2, 3)


def _same_bits(a, b):
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def start_data(c, L, data):
    """finest-level u0 and d of the case, flat: the test problem's boundary values and, for "random", a seeded random
    interior in both (no x <-> z symmetry left); "dirty" adds random values on the faces of r on level 1"""
    N = O.level_sizes(c, L)[-1]
    h = 1.0 / (N - 1)
    u = np.zeros(N ** 3)
    O.lib().orc_fill_boundary(O.P(u), N, h)
    d = u.copy()
    r1 = None
    rng = np.random.default_rng(1000 * c + 10 * L)
    if data == "random":
        u3, d3 = u.reshape(N, N, N), d.reshape(N, N, N)
        u3[1:-1, 1:-1, 1:-1] = rng.uniform(-1, 1, (N - 2,) * 3)
        d3[1:-1, 1:-1, 1:-1] = rng.uniform(-50, 50, (N - 2,) * 3)
    elif data == "dirty":
        N1 = 2 * c - 1
        r1 = rng.uniform(-1, 1, (N1, N1, N1))
        r1[1:-1, 1:-1, 1:-1] = 0.0
    return u, d, r1


# Every case's reference is computed once per session: the module holds every level of u, d and r of each (about 2 GB in
# all at the 129^3 cases), and the 513^3 oracle solution below (1 GB).  The cost is memory, against recomputing a reference
# that takes seconds on the host for each variant.
_refs = {}


def reference(c, L, nu, sigma, data, cycles):
    """norms and every level's u, d, r after `cycles` cycles of the reference; computed once per case"""
    key = (c, L, nu, sigma, data, cycles)
    if key not in _refs:
        ref = S.Problem(c, L, nu, sigma)
        u, d, r1 = start_data(c, L, data)
        N = ref.N[-1]
        ref.u[-1][...] = u.reshape(N, N, N)
        ref.d[-1][...] = d.reshape(N, N, N)
        if r1 is not None:
            ref.r[1][...] = r1
        norms = ref.vcycles(cycles)
        _refs[key] = {"norms": norms, "N": N,
                      **{(f, l): ref.flat(f, l) for f in ("u", "d", "r") for l in range(L)}}
    return _refs[key]


def load(s, c, L, data):
    """the case's start on a Solver (coarse factor of the context's sigma, as the reference's)"""
    u, d, r1 = start_data(c, L, data)
    s.get_details()
    s.upload(MG3D_U, L - 1, u)
    s.upload(MG3D_D, L - 1, d)
    if r1 is not None:
        s.upload(MG3D_R, 1, r1.reshape(-1))


def assert_levels(s, want, L, keep_r=False):
    for l in range(L):
        assert _same_bits(s.download(MG3D_U, l), want[("u", l)]), f"u level {l}"
    for l in range(L - 1):
        assert _same_bits(s.download(MG3D_D, l), want[("d", l)]), f"d level {l}"
    if keep_r:
        for l in range(1, L):
            assert _same_bits(s.download(MG3D_R, l), want[("r", l)]), f"r level {l}"


def assert_exact_norm(s, L, sigma, got):
    u, d = s.download(MG3D_U, L - 1), s.download(MG3D_D, L - 1)
    want = S.exact_residual_norm(u, d, s.level_n(L - 1), s.level_h(L - 1), sigma)
    assert got == pytest.approx(want, rel=EXACT_NORM_RTOL), (got, want)


# ------------------------------------------------------------------------------------------------ the variant matrix
# name -> (environment at creation, options after creation, keep_residual, start data override)
VARIANTS = {
    "plain": ({}, {"carry": 0, "legs": 0}, False, None),
    "carried": ({}, {"carry": 1, "carry_min": 66, "legs": 0}, False, None),
    "legs": ({}, {"carry": 0, "legs": 1, "legs_min": 66}, False, None),
    "no_fuse": ({"MG3D_NO_FUSE": "1"}, {}, False, None),
    "fuse_up_0": ({}, {"fuse_up_max": 0}, False, None),
    "fuse_up_big": ({}, {"fuse_up_max": 1 << 20}, False, None),
    "no_tiny": ({}, {"tiny": 0}, False, None),
    "no_tiny_cycle": ({}, {"tiny_cycle": 0}, False, None),
    "tiny_cycle_dirty_r": ({}, {"tiny_cycle": 1}, False, "dirty"),
    "lu_reduced_0": ({}, {"lu_reduced": 0}, False, None),
    "lu_reduced_1": ({}, {"lu_reduced": 1}, False, None),
    "fuse_rst2_0": ({}, {"fuse_rst2": 0}, False, None),
    "fuse_rst2_1": ({}, {"fuse_rst2": 1}, False, None),
    "small_0": ({}, {"small_max": 0, "fuse_leg_max": 0}, False, None),
    "small_65": ({}, {"small_max": 65, "fuse_leg_max": 65}, False, None),
    "small_1000": ({}, {"small_max": 1000, "fuse_leg_max": 1000}, False, None),
    "sweep_ci": ({}, {"sweep_tune": 0, "sweep_ci": 5}, False, None),
    "keep_residual": ({}, {}, True, None),
}

# (c, L, nu, sigma, data): every variant meets nu = 1, 2 and 3; 81^3 and 97^3 are not 2^k + 1
SHAPES = {
    1: [(9, 5, 1, 1e4, "random"), (5, 5, 1, 1.0, "test"), (11, 4, 1, 10.0, "random"), (7, 4, 1, 1.0, "random")],
    2: [(9, 5, 2, 1e-12, "test"), (6, 5, 2, 10.0, "random"), (3, 7, 2, 1e4, "random"), (17, 4, 2, 1.0, "test")],
    3: [(6, 5, 3, 1e4, "test"), (7, 5, 3, 1.0, "random"), (9, 4, 3, 10.0, "random")],
}
# variants whose launches exist only where level 1 fits one workgroup (at most 17^3: c <= 9, mg3d_tiny.hip k_tiny_fits) and
# the coarse factor has a reduced form (not at c = 3: one interior row, whose padded vectors do not fit beside the full ones, mg3d_ctx.hip install_lu)
TINY_VARIANTS = ("no_tiny", "no_tiny_cycle", "tiny_cycle_dirty_r", "lu_reduced_0", "lu_reduced_1")


def _cases():
    out = []
    for i, name in enumerate(VARIANTS):
        for nu in (1, 2, 3):
            shapes = [sh for sh in SHAPES[nu] if name not in TINY_VARIANTS or 5 <= sh[0] <= 9]
            picks = [shapes[i % len(shapes)]]
            if name in ("carried", "legs") and nu == 2:  # the schedules these names select: every shape
                picks = shapes
            for shape in picks:
                out.append(pytest.param(name, *shape, id=f"{name}-{shape[0]}_{shape[1]}_{shape[2]}-{shape[3]:g}-{shape[4]}"))
    return out


def _top_kernels(s, level):
    return {kn: n for (lvl, kn), (n, _) in s.kernel_times().items() if lvl == level}


def _assert_variant_ran(name, s, c, L, nu, kt_all, cycles):
    """The option selected its launches, as far as the kernel timers can tell (a variant that silently falls back fails
    here).  sweep_ci and small_max choose tile shapes and chunk lengths only, which the timers do not name, and an option
    that does not apply to a case's nu (fuse_rst2 at nu = 2, fuse_leg_max and fuse_up_max at nu != 2) is only compared
    for bits."""
    top = L - 1
    N = s.level_n(top)
    kt = {kn: n for (lvl, kn), n in kt_all.items() if lvl == top}
    lvl1 = {kn: n for (lvl, kn), n in kt_all.items() if lvl == 1}
    mid = range(2, top)  # below the top (no norm is formed) and above the single-workgroup level
    assert name == "no_fuse" or "colour_pass" not in kt, kt  # the fused kernels ran
    if name == "carried":
        if nu == 2 and N > 65:
            assert kt.get("sweep4+norm", 0) > 0 and kt.get("sweep1+restrict", 0) > 0, kt
        else:
            assert "sweep4+norm" not in kt and "sweep1+restrict" not in kt, kt
    elif name == "legs":
        if nu == 2 and N > 65:
            assert kt.get("leg_up", 0) > 0 and kt.get("leg_down", 0) > 0, kt
        else:
            assert "leg_up" not in kt and "leg_down" not in kt, kt
    elif name == "plain":
        assert not any(kn in kt for kn in ("sweep4+norm", "sweep1+restrict", "leg_up", "leg_down")), kt
    elif name == "no_fuse":
        assert kt.get("colour_pass", 0) > 0, kt
        assert not any(kn.startswith("sweep") for (lvl, kn) in kt_all), kt_all
    elif name in ("tiny_cycle_dirty_r", "lu_reduced_1"):
        # level 1 down, the direct solve and level 1 up as one launch (timer slot sweep4 of level 1), no coarse_solve launch
        assert lvl1 == {"sweep4": cycles} and (0, "coarse_solve") not in kt_all, kt_all
    elif name in ("no_tiny_cycle", "lu_reduced_0"):
        # (lu_reduced = 0: no reduced factor, which the single-launch bottom needs) level 1 in one workgroup, two launches
        # per cycle, the direct solve on its own
        assert lvl1 == {"sweep4": 2 * cycles} and kt_all.get((0, "coarse_solve"), 0) == cycles, kt_all
    elif name == "no_tiny":
        assert set(lvl1) != {"sweep4"} and kt_all.get((0, "coarse_solve"), 0) == cycles, kt_all
    elif name == "fuse_up_0":
        assert all(kt_all.get((l, "prolong"), 0) == cycles for l in mid) and len(mid) > 0, kt_all
    elif name == "fuse_up_big" and nu == 2:
        assert not any(kn == "prolong" for (lvl, kn) in kt_all), kt_all
    elif name.startswith("fuse_rst2") and nu != 2:
        # two passes + residual + restriction: one launch (fuse_rst2 = 1) or the passes, then a residual launch (0)
        fused = name.endswith("1")
        assert all(((l, "residual") in kt_all) != fused for l in list(mid) + [top]), kt_all
    elif name.startswith("small") and nu == 2:
        # fuse_leg_max: the down-leg of a level of at most that many points per side is one launch, without a residual one
        leg_max = VARIANTS[name][1]["fuse_leg_max"]
        assert len(mid) > 0 and all(((l, "residual") in kt_all) == (s.level_n(l) > leg_max) for l in mid), kt_all


@pytest.mark.parametrize("name,c,L,nu,sigma,data", _cases())
def test_variant_equals_the_reference(monkeypatch, name, c, L, nu, sigma, data):
    """u of every level and d below the top bit for bit after calls of 1, 2 and 3 cycles (carried and run-ahead state
    crosses the calls); every norm to the summation tolerance, the last one to the exactly rounded sum"""
    env, opts, keep_r, data_override = VARIANTS[name]
    data = data_override or data
    for k in ("MG3D_NO_FUSE", "MG3D_KEEP_R"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want = reference(c, L, nu, sigma, data, sum(CALLS))
    with M.Solver(c, L, nu) as s:
        for k, v in opts.items():
            s.set_option(k, v)
        s.set_keep_residual(keep_r)
        s.set_shift(sigma)
        load(s, c, L, data)
        s.timing_enable(1)
        norms = []
        for k in CALLS:
            norms += list(s.vcycles(k))
        kt_all = {key: n for key, (n, _) in s.kernel_times().items()}
        s.timing_enable(0)
        _assert_variant_ran(name, s, c, L, nu, kt_all, sum(CALLS))
        assert_levels(s, want, L, keep_r)
        np.testing.assert_allclose(norms, want["norms"], rtol=norm_rtol(want["N"]))
        assert_exact_norm(s, L, sigma, norms[-1])


# ------------------------------------------------------------------------------------------------ single operators
def _random_levels(s, c, L, seed):
    rng = np.random.default_rng(seed)
    out = {}
    for l in range(L):
        n = s.level_n(l)
        out[("u", l)] = rng.uniform(-1, 1, n ** 3)
        out[("d", l)] = rng.uniform(-50, 50, n ** 3)
        s.upload(MG3D_U, l, out[("u", l)])
        s.upload(MG3D_D, l, out[("d", l)])
        s.upload(MG3D_R, l, np.full(n ** 3, 3.25))  # faces of r must survive a stored residual
    return out


def _cube(a, n):
    return a.copy().reshape(n, n, n)


OP_CASES = [(9, 3, 1.0), (5, 4, 1e4), (6, 3, 10.0)]


@pytest.mark.parametrize("c,L,sigma", OP_CASES)
@pytest.mark.parametrize("post,iters", [(0, 1), (1, 2), (0, 3), (1, 3)])
def test_smooth(c, L, sigma, post, iters):
    with M.Solver(c, L, 2) as s:
        s.set_shift(sigma)
        x = _random_levels(s, c, L, 11 * c + iters)
        for l in (L - 2, L - 1):
            n, h = s.level_n(l), s.level_h(l)
            u = _cube(x[("u", l)], n)
            (S.post_smooth if post else S.pre_smooth)(u, x[("d", l)].reshape(n, n, n), h, sigma, iters)
            s.smooth(l, post, iters)
            assert _same_bits(s.download(MG3D_U, l), u.reshape(-1)), l


@pytest.mark.parametrize("c,L,sigma", OP_CASES)
@pytest.mark.parametrize("store,want_norm", [(True, True), (False, True), (True, False)])
def test_residual(c, L, sigma, store, want_norm):
    with M.Solver(c, L, 2) as s:
        s.set_shift(sigma)
        x = _random_levels(s, c, L, 13 * c)
        for l in (L - 2, L - 1):
            n, h = s.level_n(l), s.level_h(l)
            r = np.full((n, n, n), 3.25)
            want_n = S.residual(x[("u", l)].reshape(n, n, n), x[("d", l)].reshape(n, n, n), h, sigma, r)
            got = s.residual(l, store, want_norm)
            assert _same_bits(s.download(MG3D_R, l), r.reshape(-1) if store else np.full(n ** 3, 3.25)), l
            assert _same_bits(s.download(MG3D_U, l), x[("u", l)])
            if want_norm:
                assert got == pytest.approx(want_n, rel=norm_rtol(n)), l
                assert_exact_norm_level(s, l, sigma, got)


def assert_exact_norm_level(s, l, sigma, got):
    u, d = s.download(MG3D_U, l), s.download(MG3D_D, l)
    want = S.exact_residual_norm(u, d, s.level_n(l), s.level_h(l), sigma)
    assert got == pytest.approx(want, rel=EXACT_NORM_RTOL), (got, want)


@pytest.mark.parametrize("c,L,sigma", OP_CASES)
@pytest.mark.parametrize("post,iters,store", [(0, 1, True), (1, 2, False), (0, 2, True), (1, 3, True)])
def test_smooth_residual(c, L, sigma, post, iters, store):
    with M.Solver(c, L, 2) as s:
        s.set_shift(sigma)
        x = _random_levels(s, c, L, 17 * c + iters)
        for l in (L - 2, L - 1):
            n, h = s.level_n(l), s.level_h(l)
            u = _cube(x[("u", l)], n)
            d = x[("d", l)].reshape(n, n, n)
            (S.post_smooth if post else S.pre_smooth)(u, d, h, sigma, iters)
            r = np.full((n, n, n), 3.25)
            want_n = S.residual(u, d, h, sigma, r)
            got = s.smooth_residual(l, post, iters, store, True)
            assert _same_bits(s.download(MG3D_U, l), u.reshape(-1)), l
            if store:
                assert _same_bits(s.download(MG3D_R, l), r.reshape(-1)), l
            assert got == pytest.approx(want_n, rel=norm_rtol(n)), l
            assert_exact_norm_level(s, l, sigma, got)


@pytest.mark.parametrize("c,L,sigma", OP_CASES)
@pytest.mark.parametrize("iters", [1, 2, 3])
def test_smooth_restrict(c, L, sigma, iters):
    """pre-smoothing, residual and its restriction into d of the level below; r's faces (here zero) are injected"""
    with M.Solver(c, L, 2) as s:
        s.set_shift(sigma)
        x = _random_levels(s, c, L, 19 * c + iters)
        for l in (L - 2, L - 1):
            n, h, nc = s.level_n(l), s.level_h(l), s.level_n(l - 1)
            s.zero(MG3D_R, l)
            s.zero(MG3D_D, l - 1)
            u = _cube(x[("u", l)], n)
            d = x[("d", l)].reshape(n, n, n)
            S.pre_smooth(u, d, h, sigma, iters)
            r = np.zeros((n, n, n))
            S.residual(u, d, h, sigma, r)
            dc = np.zeros(nc ** 3)
            O.lib().orc_restrict(O.P(r.reshape(-1)), n, O.P(dc), nc)
            s.smooth_restrict(l, iters)
            assert _same_bits(s.download(MG3D_U, l), u.reshape(-1)), l
            assert _same_bits(s.download(MG3D_D, l - 1), dc), l


@pytest.mark.parametrize("c,L,sigma", OP_CASES)
def test_prolong_and_coarse_solve(c, L, sigma):
    """prolongation adds into u (no operator in it: it must not pick one up), the direct solve uses sigma's factor"""
    with M.Solver(c, L, 2) as s:
        s.set_shift(sigma)
        s.get_details()
        x = _random_levels(s, c, L, 23 * c)
        for l in (L - 1, L - 2):
            n, nc = s.level_n(l), s.level_n(l - 1)
            uf = x[("u", l)].copy()
            O.lib().orc_prolong(O.P(s.download(MG3D_U, l - 1)), nc, O.P(uf), n)
            s.prolong(l)
            assert _same_bits(s.download(MG3D_U, l), uf), l
        ref = S.Problem(c, L, 2, sigma)
        want = np.zeros(c ** 3)
        O.lib().orc_lu_solve(O.P(ref.LU), c ** 3, O.P(x[("d", 0)]), O.P(want))
        s.coarse_solve()
        assert _same_bits(s.download(MG3D_U, 0), want)


@pytest.mark.parametrize("c,L,nu,sigma", [(3, 6, 1, 10.0), (9, 4, 3, 1e4), (3, 5, 3, 1.0), (9, 3, 1, 1e-12)])
def test_fmg_initialize(c, L, nu, sigma):
    ref = S.Problem(c, L, nu, sigma)
    ref.setup_test_problem()
    ref.fmg_initialize()
    with M.Solver(c, L, nu) as s:
        s.set_shift(sigma)
        s.setup_test_problem()
        s.fmg_initialize()
        for l in range(L):
            assert _same_bits(s.download(MG3D_U, l), ref.flat("u", l)), l
        got = s.vcycles(2)
        want = ref.vcycles(2)
        for l in range(L):
            assert _same_bits(s.download(MG3D_U, l), ref.flat("u", l)), l
        for l in range(L - 1):
            assert _same_bits(s.download(MG3D_D, l), ref.flat("d", l)), l
    np.testing.assert_allclose(got, want, rtol=norm_rtol(ref.N[-1]))


# ------------------------------------------------------------------------------------------------ state between calls
def _schedule(s, name):
    for k, v in VARIANTS[name][1].items():
        s.set_option(k, v)


@pytest.mark.parametrize("sched", ["carried", "legs", "plain"])
def test_shift_changed_between_calls(sched):
    """vcycle (the carried / legs schedules run the next cycle's start ahead), set_shift(sigma2), vcycles(3): the state run
    ahead belongs to the old operator and must be dropped"""
    c, L, s1, s2 = 9, 5, 10.0, 1.0
    ref = S.Problem(c, L, 2, s1)
    u, d, _ = start_data(c, L, "random")
    N = ref.N[-1]
    ref.u[-1][...] = u.reshape(N, N, N)
    ref.d[-1][...] = d.reshape(N, N, N)
    want = [ref.vcycle()]
    ref.set_shift(s2)
    want += list(ref.vcycles(3))
    with M.Solver(c, L, 2) as s:
        _schedule(s, sched)
        s.set_shift(s1)
        load(s, c, L, "random")
        s.timing_enable(1)
        got = [s.vcycle()]
        s.set_shift(s2)
        got += list(s.vcycles(3))
        kt = _top_kernels(s, L - 1)
        s.timing_enable(0)
        if sched == "plain":
            assert not any(kn in kt for kn in ("sweep4+norm", "sweep1+restrict", "leg_up", "leg_down")), kt
        else:  # the first call ran the next cycle's start ahead, and the later cycles took the schedule again
            assert kt.get("sweep4+norm" if sched == "carried" else "leg_up", 0) >= 3, kt
        for l in range(L):
            assert _same_bits(s.download(MG3D_U, l), ref.flat("u", l)), l
        for l in range(L - 1):
            assert _same_bits(s.download(MG3D_D, l), ref.flat("d", l)), l
        assert_exact_norm(s, L, s2, got[-1])
    np.testing.assert_allclose(got, want, rtol=norm_rtol(N))


@pytest.mark.parametrize("sched", ["carried", "legs"])
def test_same_shift_again_inside_a_run_ahead(sched):
    """set_shift to the sigma the context already has, between single-cycle calls that run ahead: the result is that of an
    uninterrupted run"""
    c, L, sigma = 9, 5, 1e4
    want = reference(c, L, 2, sigma, "test", 6)
    with M.Solver(c, L, 2) as s:
        _schedule(s, sched)
        s.set_shift(sigma)
        load(s, c, L, "test")
        s.timing_enable(1)
        norms = [s.vcycle()]
        s.set_shift(sigma)
        norms.append(s.vcycle())
        s.set_shift(sigma)
        norms += list(s.vcycles(4))
        kt = _top_kernels(s, L - 1)
        s.timing_enable(0)
        assert kt.get("sweep4+norm" if sched == "carried" else "leg_up", 0) > 0, kt
        assert_levels(s, want, L)
        np.testing.assert_allclose(norms, want["norms"], rtol=norm_rtol(want["N"]))
        assert_exact_norm(s, L, sigma, norms[-1])


def test_options_changed_between_calls():
    """set_option between calls with sigma > 0: every schedule and kernel choice continues the same screened solve"""
    c, L, nu, sigma = 9, 5, 2, 1.0
    want = reference(c, L, nu, sigma, "random", 8)
    with M.Solver(c, L, nu) as s:
        s.set_shift(sigma)
        s.set_option("legs_min", 66)
        s.set_option("carry_min", 66)
        load(s, c, L, "random")
        s.timing_enable(1)
        norms = [s.vcycle()]                       # legs: runs ahead
        s.set_option("legs", 0)
        norms += list(s.vcycles(2))                # carried
        s.set_option("carry", 0)
        s.set_option("fuse_up_max", 0)
        norms.append(s.vcycle())                   # plain, prolongation on its own
        s.set_option("small_max", 1000)
        s.set_option("fuse_leg_max", 1000)
        s.set_option("tiny_cycle", 0)
        norms += list(s.vcycles(2))
        s.set_option("legs", 1)
        s.set_option("fuse_up_max", 1 << 20)
        norms += list(s.vcycles(2))
        kt = _top_kernels(s, L - 1)
        s.timing_enable(0)
        assert kt.get("leg_up", 0) > 0 and kt.get("sweep4+norm", 0) > 0, kt
        assert_levels(s, want, L)
        np.testing.assert_allclose(norms, want["norms"], rtol=norm_rtol(want["N"]))
        assert_exact_norm(s, L, sigma, norms[-1])


# ------------------------------------------------------------------------------------------------ 513^3
SIGMA_513 = 10.0
_oracle_513 = {}


def oracle_513(cycles=2):
    """orc_run_problem_shift(9, 7, 2, sigma = 10): the whole 513^3 solution, on 16 OpenMP threads (its grid values do not
    depend on the thread count, tests/test_screened_oracle.py)"""
    if cycles not in _oracle_513:
        O.lib().orc_set_threads(min(16, os.cpu_count() or 1))
        try:
            norms, u, _, _ = O.run_problem_shift(9, 7, 2, SIGMA_513, cycles)
        finally:
            O.lib().orc_set_threads(1)
        _oracle_513[cycles] = (norms, u)
    return _oracle_513[cycles]


def exact_norm_513(u, d, N, h, sigma):
    """S.exact_residual_norm with the residual field from the C twin (one N^3 temporary instead of numpy's several)"""
    res = np.zeros(N ** 3)
    O.lib().orc_residual_shift(O.P(u), O.P(d), N, h, sigma, O.P(res))
    sq = res * res
    total = np.longdouble(0)
    step = 1 << 24
    for a in range(0, sq.size, step):
        total += np.sum(sq[a:a + step].astype(np.longdouble))
    return float(np.sqrt(total))


@pytest.mark.parametrize("sched", ["default", "carried", "plain"])
def test_513_cubed(sched):
    """`9 7 2`, sigma = 10, two cycles in each schedule (default at this size: one launch per leg): the whole solution
    vector against the oracle's, the launches that ran, the last norm against the exactly rounded sum"""
    want_norms, want_u = oracle_513(2)
    with M.Solver(9, 7, 2) as s:
        if sched != "default":
            s.set_option("legs", 0)
        if sched == "plain":
            s.set_option("carry", 0)
        s.set_shift(SIGMA_513)
        s.setup_test_problem()
        s.timing_enable(1)
        got = s.vcycles(2)
        kt = _top_kernels(s, 6)
        s.timing_enable(0)
        if sched == "default":
            assert kt.get("leg_up") == 2 and kt.get("leg_down") == 1 and "sweep4+norm" not in kt, kt
        elif sched == "carried":
            assert kt.get("sweep4+norm") == 1 and "leg_up" not in kt, kt
        else:
            assert not any(kn in kt for kn in ("sweep4+norm", "sweep1+restrict", "leg_up", "leg_down")), kt
        u = s.download(MG3D_U, 6)
        assert _same_bits(u, want_u)
        exact = exact_norm_513(u, s.download(MG3D_D, 6), 513, s.level_h(6), SIGMA_513)
        assert got[-1] == pytest.approx(exact, rel=EXACT_NORM_RTOL)
    np.testing.assert_allclose(got, want_norms, rtol=norm_rtol(513))
