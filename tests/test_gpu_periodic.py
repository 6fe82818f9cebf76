"""Periodic boundaries (mg3d_ctx_set_periodic) on the GPU, against the numpy reference of tests/_periodic_ref.py: every
grid value bit for bit on every level for all seven masks, the single operators, periodic-consistent downloads, garbage
at duplicates, the norm over the unique points, mask 0 after a periodic mask, run-ahead state across a change of
boundaries, the argument and state rules, and convergence on manufactured problems."""
import math

import numpy as np
import pytest

import _coef_ref as CR
import _periodic_ref as R
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U

from test_gpu_parity import norm_rtol

pytestmark = pytest.mark.gpu

MG3D_ERR_ARG, MG3D_ERR_STATE = 1, 5


def _same_bits(a, b):
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _n(c, L):
    return (c - 1) * (1 << (L - 1)) + 1


def _consistent(a, axes):
    b = np.array(a).reshape((round(np.asarray(a).size ** (1 / 3)),) * 3)
    c = b.copy()
    R.refresh(c, axes)
    return _same_bits(b, c)


def _random_problem(ref, rng):
    N = ref.N[-1]
    ref.u[-1][...] = rng.standard_normal((N, N, N))
    ref.d[-1][...] = rng.standard_normal((N, N, N))
    R.refresh(ref.u[-1], ref.axes)
    R.refresh(ref.d[-1], ref.axes)


def _solver(c, L, nu, sigma, eps, axes, ref):
    s = M.Solver(c, L, nu)
    s.set_shift(sigma)
    s.set_periodic(axes)
    if eps is not None:
        s.set_coefficient(eps)
    s.get_details()
    s.upload(MG3D_U, L - 1, ref.u[-1])
    s.upload(MG3D_D, L - 1, ref.d[-1])
    return s


def _assert_levels(s, ref, L, axes):
    for l in range(L):
        got = s.download(MG3D_U, l)
        assert _same_bits(got, ref.flat("u", l)), f"u level {l}"
        assert _consistent(got, axes), f"u level {l} duplicates"
    for l in range(L - 1):
        got = s.download(MG3D_D, l)
        assert _same_bits(got, ref.flat("d", l)), f"d level {l}"
        assert _consistent(got, axes), f"d level {l} duplicates"


_CASES = [(c, L, axes, sigma, f) for (c, L) in [(5, 4), (5, 5), (9, 4)] for axes in range(1, 8) for sigma in (0.0, 1e3)
          for f in (None, "smooth")]
_CASES += [(9, 5, axes, sigma, f) for axes in (6, 7) for sigma in (0.0, 1e3) for f in (None, "exp")]


@pytest.mark.parametrize("c,L,axes,sigma,field", _CASES)
def test_parity(c, L, axes, sigma, field):
    """u of every level and d below the top after vcycles(1) + vcycles(2), bit for bit; nu = 1..3 across the masks"""
    nu = 1 + axes % 3
    eps = None if field is None else CR.FIELDS[field](_n(c, L))
    ref = R.Problem(c, L, nu, sigma, eps, axes)
    _random_problem(ref, np.random.default_rng(axes))
    with _solver(c, L, nu, sigma, eps, axes, ref) as s:
        assert s.periodic == axes
        want = ref.vcycles(3)
        got = list(s.vcycles(1)) + list(s.vcycles(2))
        _assert_levels(s, ref, L, axes)
        N, h = s.level_n(L - 1), s.level_h(L - 1)
        exact = R.exact_residual_norm(s.download(MG3D_U, L - 1), s.download(MG3D_D, L - 1), ref.e(L - 1), N, h, sigma,
                                      axes)
        assert got[-1] == pytest.approx(exact, rel=1e-13), (got[-1], exact)
    np.testing.assert_allclose(got, want, rtol=norm_rtol(ref.N[-1]))


def test_full_size_257():
    c, L, axes, sigma = 9, 6, 6, 10.0
    ref = R.Problem(c, L, 1, sigma, None, axes)
    _random_problem(ref, np.random.default_rng(257))
    with _solver(c, L, 1, sigma, None, axes, ref) as s:
        want = ref.vcycles(2)
        got = s.vcycles(2)
        assert _same_bits(s.download(MG3D_U, L - 1), ref.flat("u", L - 1))
    np.testing.assert_allclose(got, want, rtol=norm_rtol(ref.N[-1]))


@pytest.mark.parametrize("axes", [1, 2, 4, 7])
@pytest.mark.parametrize("field", [None, "exp"])
def test_single_operators(axes, field):
    """smooth, residual (r stored), restrict, prolong, coarse_solve on random data, bit for bit and periodic-consistent"""
    c, L, sigma = 5, 3, 1.0 if axes != 7 else 0.0
    rng = np.random.default_rng(11 + axes)
    N = _n(c, L)
    eps = None if field is None else CR.FIELDS[field](N)
    ref = R.Problem(c, L, 2, sigma, eps, axes)
    with M.Solver(c, L, 2) as s:
        s.set_shift(sigma)
        s.set_periodic(axes)
        if eps is not None:
            s.set_coefficient(eps)
        s.get_details()
        for l in (L - 1, L - 2):
            n, h, e = s.level_n(l), s.level_h(l), ref.e(l)
            u, d = rng.standard_normal((n, n, n)), rng.standard_normal((n, n, n))
            s.upload(MG3D_U, l, u)
            s.upload(MG3D_D, l, d)
            s.smooth(l, 0, 2)
            R.pre_smooth(u, d, e, h, sigma, axes, 2)
            assert _same_bits(s.download(MG3D_U, l), u.reshape(-1)), f"pre-smoothing, level {l}"
            s.smooth(l, 1, 1)
            R.post_smooth(u, d, e, h, sigma, axes, 1)
            assert _same_bits(s.download(MG3D_U, l), u.reshape(-1)), f"post-smoothing, level {l}"
            r = np.zeros((n, n, n))
            s.zero(MG3D_R, l)
            got = s.residual(l, store=True)
            want = R.residual(u, d, e, h, sigma, axes, r)
            assert _same_bits(s.download(MG3D_R, l), r.reshape(-1)), f"residual, level {l}"
            assert _consistent(s.download(MG3D_R, l), axes)
            assert got == pytest.approx(want, rel=1e-13)
            nc = s.level_n(l - 1)
            dc = rng.standard_normal((nc, nc, nc))
            s.upload(MG3D_D, l - 1, dc)
            s.restrict(l)
            R.restrict(r, dc, axes)
            assert _same_bits(s.download(MG3D_D, l - 1), dc.reshape(-1)), f"restrict, level {l}"
            ec = rng.standard_normal((nc, nc, nc))
            R.refresh(ec, axes)
            s.upload(MG3D_U, l - 1, ec)
            s.prolong(l)
            R.prolong(ec, u, axes)
            assert _same_bits(s.download(MG3D_U, l), u.reshape(-1)), f"prolong, level {l}"
        n0 = s.level_n(0)
        d0 = rng.standard_normal((n0, n0, n0))
        s.upload(MG3D_D, 0, d0)
        s.coarse_solve()
        u0 = np.zeros((n0, n0, n0))
        R.coarse_solve(ref.LU, d0, u0, axes, sigma)
        got = s.download(MG3D_U, 0)
        assert _same_bits(got, u0.reshape(-1))
        assert _consistent(got, axes)


@pytest.mark.parametrize("axes", [3, 7])
def test_garbage_at_duplicates(axes):
    """NaN at every duplicate of the uploaded u, d and eps changes no unique value, and every download is consistent"""
    c, L, sigma = 5, 4, 2.0
    N = _n(c, L)
    rng = np.random.default_rng(3)
    eps = CR.smooth_eps(N)
    u, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    dup = R.is_dup(N, axes)
    outs = []
    for garbage in (False, True):
        uu, dd, ee = u.copy(), d.copy(), eps.copy()
        if garbage:
            for a in (uu, dd, ee):
                a[dup] = np.nan
        else:
            for a in (uu, dd, ee):
                R.refresh(a, axes)
        with M.Solver(c, L, 2) as s:
            s.set_keep_residual(True)
            s.set_shift(sigma)
            s.set_periodic(axes)
            s.set_coefficient(ee)
            s.get_details()
            s.upload(MG3D_U, L - 1, uu)
            s.upload(MG3D_D, L - 1, dd)
            norms = s.vcycles(2)
            assert np.isfinite(norms).all()
            outs.append([s.download(MG3D_U, l) for l in range(L)] + [s.download(MG3D_R, L - 1)])
    for a, b in zip(*outs):  # (a duplicate that is also a Dirichlet point is never written: it keeps its NaN)
        assert _same_bits(a.reshape(N, N, N)[~dup] if a.size == N ** 3 else a, b.reshape(N, N, N)[~dup] if b.size == N ** 3 else b)
        assert _consistent(a, axes)
        if axes == 7:
            assert _same_bits(a, b)


@pytest.mark.parametrize("axes", [1, 6, 7])
def test_norm_over_unique_points(axes):
    c, L, sigma = 9, 4, 0.0
    ref = R.Problem(c, L, 2, sigma, None, axes)
    _random_problem(ref, np.random.default_rng(5))
    with _solver(c, L, 2, sigma, None, axes, ref) as s:
        got = s.residual(L - 1, store=False)
        N, h = s.level_n(L - 1), s.level_h(L - 1)
        diff = R.residual_field(ref.u[-1], ref.d[-1], None, h, sigma, axes)
        want = math.sqrt(math.fsum((diff * diff).reshape(-1)))
        assert abs(got - want) <= 1e-13 * want, (got, want)
        assert diff.size == R.unique_mask(N, axes).sum()


def test_mask_0_after_a_periodic_mask_is_a_fresh_context():
    """bits of u, norms and the fused schedules of a fresh context (kernel timers: sweeps run again)"""
    c, L = 9, 5
    N = _n(c, L)
    rng = np.random.default_rng(9)
    u, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))

    def run(s):
        s.get_details()
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        s.timing_enable(True)
        s.timing_reset()
        norms = [s.vcycle()] + list(s.vcycles(3))
        kt = s.kernel_times()
        return norms, s.download(MG3D_U, L - 1), kt

    with M.Solver(c, L, 2) as s:
        s.set_periodic((0, 2))
        s.get_details()
        s.vcycles(1)
        s.set_periodic(())
        assert s.periodic == 0
        got = run(s)
    with M.Solver(c, L, 2) as f:
        want = run(f)
    assert got[0] == want[0]
    assert _same_bits(got[1], want[1])
    assert sorted(k for k, v in got[2].items() if v) == sorted(k for k, v in want[2].items() if v)


def test_run_ahead_state_across_a_change_of_boundaries():
    """legs at 129^3: vcycle (runs the next down-leg ahead), set_periodic, cycles -- the reference of one Dirichlet cycle
    followed by periodic cycles"""
    c, L, axes = 9, 5, 6
    N = _n(c, L)
    rng = np.random.default_rng(13)
    import _screened_ref as S
    dref = S.Problem(c, L, 2, 0.0)
    dref.u[-1][...] = rng.standard_normal((N, N, N))
    dref.d[-1][...] = rng.standard_normal((N, N, N))
    u0, d0 = dref.u[-1].copy(), dref.d[-1].copy()
    first = dref.vcycle()
    ref = R.Problem(c, L, 2, 0.0, None, axes)
    ref.u[-1][...] = dref.u[-1]
    ref.d[-1][...] = dref.d[-1]
    want = [first] + list(ref.vcycles(3))
    with M.Solver(c, L, 2) as s:
        s.set_option("legs", 1)
        s.set_option("legs_min", 66)
        s.get_details()
        s.upload(MG3D_U, L - 1, u0)
        s.upload(MG3D_D, L - 1, d0)
        got = [s.vcycle()]
        s.set_periodic(axes)
        got += list(s.vcycles(2)) + [s.vcycle()]
        assert _same_bits(s.download(MG3D_U, L - 1), ref.flat("u", L - 1))
    np.testing.assert_allclose(got, want, rtol=norm_rtol(N))


def test_argument_and_state_rules():
    with M.Solver(5, 3, 2) as s:
        s.get_details()
        for bad in (-1, 8, 100):
            with pytest.raises(M.Mg3dError) as e:
                s.set_periodic(bad)
            assert e.value.code == MG3D_ERR_ARG
            assert s.periodic == 0
        with pytest.raises(ValueError):
            s.set_periodic([3])
        s.set_periodic([1, 2])
        assert s.periodic == 6
        s.set_periodic(6)  # the same mask: nothing changes
        for call in (lambda: s.es_setup(), lambda: s.es_vcycles(1), lambda: s.fmg_initialize(),
                     lambda: s.fill_boundary(MG3D_D, 2)):
            with pytest.raises(M.Mg3dError) as e:
                call()
            assert e.value.code == MG3D_ERR_STATE
        s.set_periodic(0)
        s.fill_boundary(MG3D_D, 2)
    for c in (3, 4, 6):  # c - 1 odd or below 4
        with M.Solver(c, 3, 2) as s:
            with pytest.raises(M.Mg3dError) as e:
                s.set_periodic(7)
            assert e.value.code == MG3D_ERR_ARG
            assert s.periodic == 0
    with M.Solver(5, 3, 2) as s:  # a factor given to set_lu is dropped
        s.get_details()
        n0 = 125
        LU = np.zeros(n0 * n0)
        import _oracle as O
        O.lib().orc_coarse_matrix(O.P(LU), 5, s.level_h(0))
        O.lib().orc_lu_factor(O.P(LU), n0)
        s.set_lu(LU)
        s.set_periodic(7)
        with pytest.raises(M.Mg3dError) as e:
            s.vcycles(1)
        assert e.value.code == MG3D_ERR_STATE
        s.get_details()
        s.vcycles(1)


@pytest.mark.parametrize("axes,sigma", [(7, 0.0), (7, 1e3), (6, 0.0)])
def test_manufactured_convergence(axes, sigma):
    """129^3: the discretisation error of u* (means removed when singular) is below 4e-4 max|u*| after 20 cycles, and the
    residual factor per cycle stays under the bound of the numpy reference"""
    from test_periodic_host import FACTOR_BOUND
    c, L = 9, 5
    N = _n(c, L)
    ustar, f = R.manufactured(N, axes, sigma)
    u0 = ustar.copy()
    u0[R.unique_mask(N, axes)] = 0.
    R.refresh(u0, axes)
    with M.Solver(c, L, 2) as s:
        s.set_shift(sigma)
        s.set_periodic(axes)
        s.get_details()
        s.upload(MG3D_U, L - 1, u0)
        s.upload(MG3D_D, L - 1, f)
        init = s.residual(L - 1, store=False)
        norms = np.concatenate([[init], s.vcycles(20)])
        u = s.download(MG3D_U, L - 1).reshape(N, N, N)
    m = R.unique_mask(N, axes)
    err = u[m] - ustar[m]
    if R.pinned(axes, sigma):
        err = err - err.mean()
    assert np.abs(err).max() < 4e-4 * np.abs(ustar).max(), np.abs(err).max()
    above = norms[norms > 1e-10 * norms[0]]
    assert (above[1:] / above[:-1]).max() < FACTOR_BOUND, norms
    assert norms[-1] < 1e-10 * norms[0], norms
