"""The variable-coefficient operator  div(eps grad u) - sigma u = d  (mg3d_ctx_set_coefficient) on the GPU, against the
numpy reference of tests/_coef_ref.py: every grid value bit for bit, norms to the summation tolerance and the last one
against the exactly rounded sum; the injected coefficients; the bypassed fused schedules; run-ahead state across a change
of operator; a manufactured solution; and the argument and state rules."""
import numpy as np
import pytest

import _coef_ref as R
import _oracle as O
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U

from test_gpu_parity import EXACT_NORM_RTOL, norm_rtol

pytestmark = pytest.mark.gpu

MG3D_ERR_ARG, MG3D_ERR_STATE = 1, 5


def _same_bits(a, b):
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _assert_levels(s, ref, L):
    for l in range(L):
        assert _same_bits(s.download(MG3D_U, l), ref.flat("u", l)), f"u level {l}"
    for l in range(L - 1):
        assert _same_bits(s.download(MG3D_D, l), ref.flat("d", l)), f"d level {l}"


def _assert_exact_norm(s, L, eps, sigma, got):
    u, d = s.download(MG3D_U, L - 1), s.download(MG3D_D, L - 1)
    want = R.exact_residual_norm(u, d, eps, s.level_n(L - 1), s.level_h(L - 1), sigma)
    assert got == pytest.approx(want, rel=EXACT_NORM_RTOL), (got, want)


def _n(c, L):
    return (c - 1) * (1 << (L - 1)) + 1


# every (nu, sigma, eps) on the 33^3 and 65^3 problems; on the three 129^3 ones every sigma with nu and eps paired, which
# keeps the numpy side of the file to a few minutes
_CASES = [(c, L, nu, sigma, f) for (c, L) in [(3, 5), (5, 5)] for nu in (1, 2, 3) for sigma in (0.0, 1e3)
          for f in ("smooth", "exp", "ball")]
_CASES += [(c, L, nu, sigma, f) for (c, L) in [(9, 5), (17, 4), (3, 7)] for sigma in (0.0, 1e3)
           for nu, f in ((1, "smooth"), (2, "exp"), (3, "ball"))]


@pytest.mark.parametrize("c,L,nu,sigma,field", _CASES)
def test_parity(c, L, nu, sigma, field):
    """u of every level and d below the top after vcycles(1) + vcycles(2), bit for bit"""
    eps = R.FIELDS[field](_n(c, L))
    ref = R.Problem(c, L, nu, sigma, eps)
    ref.setup_test_problem()
    want = ref.vcycles(3)
    with M.Solver(c, L, nu) as s:
        s.set_shift(sigma)
        s.set_coefficient(eps)
        assert s.has_coefficient()
        s.setup_test_problem()
        got = list(s.vcycles(1)) + list(s.vcycles(2))
        _assert_levels(s, ref, L)
        _assert_exact_norm(s, L, eps, sigma, got[-1])
    np.testing.assert_allclose(got, want, rtol=norm_rtol(ref.N[-1]))


@pytest.mark.parametrize("sigma", [0.0, 1e3])
def test_single_operators(sigma):
    """smooth (pre and post), residual with r stored, smooth_restrict: one level, random u and d, bit for bit"""
    c, L = 5, 4
    rng = np.random.default_rng(7)
    N = _n(c, L)
    eps = R.exp_eps(N)
    with M.Solver(c, L, 2) as s:
        s.set_shift(sigma)
        s.set_coefficient(eps)
        es = R.inject(eps, L)
        for l in (L - 1, L - 2):
            n, h, e = s.level_n(l), s.level_h(l), es[l]
            u, d = rng.standard_normal((n, n, n)), rng.standard_normal((n, n, n))
            s.upload(MG3D_U, l, u)
            s.upload(MG3D_D, l, d)
            s.smooth(l, 0, 2)
            R.pre_smooth(u, d, e, h, sigma, 2)
            assert _same_bits(s.download(MG3D_U, l), u.reshape(-1)), f"pre-smoothing, level {l}"
            s.smooth(l, 1, 1)
            R.post_smooth(u, d, e, h, sigma, 1)
            assert _same_bits(s.download(MG3D_U, l), u.reshape(-1)), f"post-smoothing, level {l}"
            r = np.zeros((n, n, n))
            s.zero(MG3D_R, l)
            got = s.residual(l, store=True)
            want = R.residual(u, d, e, h, sigma, r)
            assert _same_bits(s.download(MG3D_R, l), r.reshape(-1)), f"residual, level {l}"
            assert got == pytest.approx(want, rel=1e-13)
            nc = s.level_n(l - 1)
            s.smooth_restrict(l, 1)
            R.pre_smooth(u, d, e, h, sigma, 1)
            R.residual(u, d, e, h, sigma, r)
            dc = np.zeros(nc ** 3)
            O.lib().orc_restrict(O.P(np.ascontiguousarray(r.reshape(-1))), n, O.P(dc), nc)
            assert _same_bits(s.download(MG3D_U, l), u.reshape(-1)), f"smooth_restrict u, level {l}"
            assert _same_bits(s.download(MG3D_D, l - 1), dc), f"smooth_restrict d, level {l - 1}"


def test_full_size_257():
    """257^3 with the default options, three cycles: u of the top level bit for bit"""
    c, L, sigma = 9, 6, 10.0
    eps = R.smooth_eps(_n(c, L))
    ref = R.Problem(c, L, 2, sigma, eps)
    ref.setup_test_problem()
    want = ref.vcycles(3)
    with M.Solver(c, L, 2) as s:
        s.set_shift(sigma)
        s.set_coefficient(eps)
        s.setup_test_problem()
        got = s.vcycles(3)
        assert _same_bits(s.download(MG3D_U, L - 1), ref.flat("u", L - 1))
        _assert_exact_norm(s, L, eps, sigma, got[-1])
    np.testing.assert_allclose(got, want, rtol=norm_rtol(ref.N[-1]))


def test_coefficient_of_every_level_is_the_injection():
    c, L = 5, 5
    eps = R.ball_eps(_n(c, L)) * R.exp_eps(_n(c, L))
    with M.Solver(c, L, 2) as s:
        assert not s.has_coefficient()
        s.set_coefficient(eps.reshape(-1))  # the flat form
        for l in range(L):
            m = L - 1 - l
            assert _same_bits(s.coefficient(l), eps[::2 ** m, ::2 ** m, ::2 ** m]), l
        eps2 = R.smooth_eps(_n(c, L))
        s.set_coefficient(eps2)  # another array replaces every level's
        for l in range(L):
            m = L - 1 - l
            assert _same_bits(s.coefficient(l), eps2[::2 ** m, ::2 ** m, ::2 ** m]), l


def test_fused_schedules_are_bypassed():
    """carry / legs forced on at 129^3 with lowered thresholds: the options keep their values, the bits stay the
    reference's (single vcycle calls, which run ahead on the constant path, included)"""
    c, L, sigma = 9, 5, 1.0
    eps = R.exp_eps(_n(c, L))
    ref = R.Problem(c, L, 2, sigma, eps)
    ref.setup_test_problem()
    want = ref.vcycles(5)
    for legs in (0, 1):
        with M.Solver(c, L, 2) as s:
            s.set_option("carry", 1)
            s.set_option("carry_min", 66)
            s.set_option("legs", legs)
            s.set_option("legs_min", 66)
            s.set_shift(sigma)
            s.set_coefficient(eps)
            s.setup_test_problem()
            got = [s.vcycle(), s.vcycle()] + list(s.vcycles(3))
            assert s.get_option("legs") == legs and s.get_option("carry_min") == 66
            _assert_levels(s, ref, L)
        np.testing.assert_allclose(got, want, rtol=norm_rtol(ref.N[-1]))


def test_run_ahead_state_across_a_change_of_operator():
    """legs at 129^3: vcycle (runs the next down-leg ahead), set_coefficient, cycles -- the reference of one constant cycle
    followed by coefficient cycles; then set_coefficient(None) and more cycles -- bit for bit a fresh constant context
    given the same u and d"""
    c, L = 9, 5
    N = _n(c, L)
    eps = R.smooth_eps(N)
    ref = R.Problem(c, L, 2, 0.0, None)
    ref.setup_test_problem()
    want = [ref.vcycle()]
    ref.set_coefficient(eps)
    want += list(ref.vcycles(3))
    with M.Solver(c, L, 2) as s:
        s.set_option("legs", 1)
        s.set_option("legs_min", 66)
        s.setup_test_problem()
        got = [s.vcycle()]
        s.set_coefficient(eps)
        got += list(s.vcycles(2)) + [s.vcycle()]
        _assert_levels(s, ref, L)
        np.testing.assert_allclose(got, want, rtol=norm_rtol(N))
        s.set_coefficient(None)
        assert not s.has_coefficient()
        u, d = s.download(MG3D_U, L - 1), s.download(MG3D_D, L - 1)
        after = [s.vcycle()] + list(s.vcycles(2))
        u_after = s.download(MG3D_U, L - 1)
    with M.Solver(c, L, 2) as f:
        f.set_option("legs", 1)
        f.set_option("legs_min", 66)
        f.get_details()
        f.upload(MG3D_U, L - 1, u)
        f.upload(MG3D_D, L - 1, d)
        fresh = [f.vcycle()] + list(f.vcycles(2))
        assert _same_bits(u_after, f.download(MG3D_U, L - 1))
    assert after == fresh


def test_manufactured_solution():
    """129^3, smooth eps: d = A u* with u* carrying its own Dirichlet values; fifteen cycles reach 1e-10 max|u*| and the
    mean convergence factor is below 0.25"""
    c, L = 9, 5
    N = _n(c, L)
    eps = R.smooth_eps(N)
    with M.Solver(c, L, 2) as s:
        h = s.level_h(L - 1)
        x = np.arange(N) * h
        ustar = (np.sin(np.pi * x)[:, None, None] * np.cos(2 * x)[None, :, None] * np.exp(x)[None, None, :]
                 + x[:, None, None] * x[None, None, :])
        d = R.apply(ustar, eps, h, 0.0)
        s.set_coefficient(eps)
        s.get_details()
        u0 = ustar.copy()
        u0[1:-1, 1:-1, 1:-1] = 0.
        s.upload(MG3D_U, L - 1, u0)
        s.upload(MG3D_D, L - 1, d)
        init = s.residual(L - 1, store=False)
        norms = s.vcycles(15)
        u = s.download(MG3D_U, L - 1).reshape(N, N, N)
    err = np.abs(u - ustar).max()
    assert err < 1e-10 * np.abs(ustar).max(), err
    # mean factor over the cycles above the rounding floor
    n = np.concatenate([[init], norms])
    k = int(np.argmax(n < 1e-10 * init)) if (n < 1e-10 * init).any() else len(n) - 1
    mean = (n[k] / n[0]) ** (1.0 / k)
    assert mean < 0.25, (mean, n)


def test_argument_and_state_rules():
    c, L = 5, 4
    N = _n(c, L)
    good = R.smooth_eps(N)
    with M.Solver(c, L, 2) as s:
        s.setup_test_problem()
        for bad_value in (0.0, -1.0, float("nan"), float("inf")):
            bad = good.copy()
            bad[3, 4, 5] = bad_value
            with pytest.raises(M.Mg3dError) as e:
                s.set_coefficient(bad)
            assert e.value.code == MG3D_ERR_ARG
            assert not s.has_coefficient()
        with pytest.raises(ValueError):
            s.set_coefficient(np.ones((N - 1, N, N)))
        with pytest.raises(ValueError):
            s.set_coefficient(np.ones(N ** 3 + 1))
        s.set_coefficient(good)
        for bad_value in (0.0, float("nan")):  # a refused array keeps the coefficient in place
            bad = good.copy()
            bad[1, 1, 1] = bad_value
            with pytest.raises(M.Mg3dError):
                s.set_coefficient(bad)
            assert s.has_coefficient()
            assert _same_bits(s.coefficient(L - 1), good)
        with pytest.raises(M.Mg3dError) as e:
            s.es_setup()
        assert e.value.code == MG3D_ERR_STATE
        with pytest.raises(M.Mg3dError) as e:
            s.es_vcycles(1)
        assert e.value.code == MG3D_ERR_STATE
        s.set_coefficient(None)
        with pytest.raises(M.Mg3dError) as e:
            s.coefficient(0)
        assert e.value.code == MG3D_ERR_STATE
    with M.Solver(c, L, 2) as s:
        n0 = c ** 3
        LU = np.zeros(n0 * n0)
        O.lib().orc_coarse_matrix(O.P(LU), c, s.level_h(0))
        O.lib().orc_lu_factor(O.P(LU), n0)
        s.set_lu(LU)
        s.set_coefficient(good)
        with pytest.raises(M.Mg3dError) as e:
            s.vcycles(1)
        assert e.value.code == MG3D_ERR_STATE
        s.get_details()  # a factor of the coefficient operator: cycles run again
        s.vcycles(1)
