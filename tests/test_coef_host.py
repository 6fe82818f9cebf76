"""The variable-coefficient operator (mg3d_ctx_set_coefficient) without a GPU: the library's coarse matrix against a numpy
assembly, and the numpy V-cycle of tests/_coef_ref.py against the screened reference and as a solver."""
import numpy as np
import pytest

import _coef_ref as R
import _screened_ref as S
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import P


def _lib_matrix(N, h, eps, sigma):
    A = np.zeros(N ** 6)
    M.lib().mg3d_coarse_matrix_coef(P(A), N, h, P(np.ascontiguousarray(eps, dtype=np.float64).reshape(-1)), sigma)
    return A


@pytest.mark.parametrize("N,h", [(3, 0.5), (5, 0.25), (9, 1.0 / 8)])
@pytest.mark.parametrize("field", ["smooth", "exp", "ball"])
@pytest.mark.parametrize("sigma", [0.0, 1.0, 1e4])
def test_coarse_matrix_coef_equals_numpy(N, h, field, sigma):
    eps = R.FIELDS[field](N)
    assert _lib_matrix(N, h, eps, sigma).tobytes() == R.coarse_matrix(N, h, eps, sigma).tobytes()


@pytest.mark.parametrize("N,h", [(3, 0.5), (5, 0.25), (9, 1.0 / 8)])
@pytest.mark.parametrize("sigma", [0.0, 1.0, 1e4])
def test_coarse_matrix_coef_of_one_is_the_shift_matrix(N, h, sigma):
    want = np.zeros(N ** 6)
    M.lib().mg3d_coarse_matrix_shift(P(want), N, h, sigma)
    assert _lib_matrix(N, h, np.ones((N, N, N)), sigma).tobytes() == want.tobytes()


@pytest.mark.parametrize("c,L,sigma", [(5, 4, 0.0), (3, 5, 10.0), (9, 3, 1e3)])
def test_reference_of_eps_one_is_the_screened_reference(c, L, sigma):
    """eps = 1: the same operator, but (s - hSq d)/dg against (1/dg)(s - hSq d) -- agreement to rounding, not bits"""
    N = (c - 1) * (1 << (L - 1)) + 1
    want = S.Problem(c, L, 2, sigma)
    got = R.Problem(c, L, 2, sigma, np.ones((N, N, N)))
    for p in (want, got):
        p.setup_test_problem()
    wn, gn = want.vcycles(3), got.vcycles(3)
    scale = np.abs(want.flat("u", L - 1)).max()  # (coarse corrections shrink to ~1e-17 as the cycle converges)
    for l in range(L):
        w, g = want.flat("u", l), got.flat("u", l)
        np.testing.assert_allclose(g, w, rtol=1e-13, atol=1e-13 * scale, err_msg=f"u level {l}")
    np.testing.assert_allclose(gn, wn, rtol=1e-11)


def test_reference_converges_on_a_smooth_coefficient():
    """33^3, eps = 1 + 1/2 sin(2 pi x) cos(pi y): every cycle cuts the residual by at least 5x"""
    c, L = 5, 4
    N = 33
    ref = R.Problem(c, L, 2, 0.0, R.smooth_eps(N))
    ref.setup_test_problem()
    e = ref.eps[-1]
    init = R.residual(ref.u[-1], ref.d[-1], e, ref.h, 0.0)
    norms = np.concatenate([[init], ref.vcycles(6)])
    ratios = norms[1:] / norms[:-1]
    assert (ratios < 0.2).all(), ratios


def test_binding_exposes_the_coefficient():
    for name in ("set_coefficient", "has_coefficient", "coefficient"):
        assert callable(getattr(M.Solver, name))
    for sym in ("mg3d_ctx_set_coefficient", "mg3d_ctx_has_coefficient", "mg3d_ctx_get_coefficient", "mg3d_coarse_matrix_coef"):
        assert getattr(M.lib(), sym) is not None
