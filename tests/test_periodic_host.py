"""Periodic boundaries (mg3d_ctx_set_periodic) without a GPU: the library's coarse matrix (mg3d_coarse_matrix_periodic)
against the numpy assembly of tests/_periodic_ref.py and its structure, and the numpy V-cycle as a solver of manufactured
periodic problems."""
import numpy as np
import pytest

import _coef_ref as CR
import _periodic_ref as R
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import P

MASKS = list(range(1, 8))


def _lib_matrix(N, h, eps, sigma, axes):
    A = np.zeros(N ** 6)
    e = None if eps is None else P(np.ascontiguousarray(eps, dtype=np.float64).reshape(-1))
    M.lib().mg3d_coarse_matrix_periodic(P(A), N, h, e, sigma, axes)
    return A


@pytest.mark.parametrize("N,h", [(5, 0.25), (9, 1.0 / 8)])
@pytest.mark.parametrize("sigma", [0.0, 1e3])
@pytest.mark.parametrize("field", [None, "exp"])
def test_mask_0_is_the_dirichlet_matrix(N, h, sigma, field):
    if field is None:
        want = np.zeros(N ** 6)
        M.lib().mg3d_coarse_matrix_shift(P(want), N, h, sigma)
        eps = None
    else:
        eps = CR.FIELDS[field](N)
        want = np.zeros(N ** 6)
        M.lib().mg3d_coarse_matrix_coef(P(want), N, h, P(np.ascontiguousarray(eps).reshape(-1)), sigma)
    assert _lib_matrix(N, h, eps, sigma, 0).tobytes() == want.tobytes()


@pytest.mark.parametrize("axes", MASKS)
@pytest.mark.parametrize("N,h", [(5, 0.25), (7, 1.0 / 6), (9, 1.0 / 8)])
@pytest.mark.parametrize("sigma", [0.0, 1e3])
@pytest.mark.parametrize("field", [None, "exp"])
def test_coarse_matrix_equals_numpy(axes, N, h, sigma, field):
    eps = None if field is None else CR.FIELDS[field](N)
    assert _lib_matrix(N, h, eps, sigma, axes).tobytes() == R.coarse_matrix(N, h, eps, sigma, axes).tobytes()


@pytest.mark.parametrize("axes", MASKS)
@pytest.mark.parametrize("sigma", [0.0, 1e3])
@pytest.mark.parametrize("field", [None, "smooth"])
def test_coarse_matrix_structure(axes, sigma, field):
    """unique rows of the constant operator sum to -sigma; the unique block is symmetric; duplicate rows, Dirichlet rows
    and the pinned row are identity rows"""
    N, h = 9, 1.0 / 8
    eps = None if field is None else CR.FIELDS[field](N)
    n = N ** 3
    A = _lib_matrix(N, h, eps, sigma, axes).reshape(n, n)
    unk = R.unique_mask(N, axes).reshape(-1)
    pin = R.pinned(axes, sigma)
    assert pin == (axes == 7 and sigma == 0.0)
    rows = np.flatnonzero(unk)
    ident = np.flatnonzero(~unk)
    if pin:
        assert rows[0] == 0
        ident = np.concatenate([[0], ident])
        rows = rows[1:]
    eye = np.zeros(n)
    for p in ident:
        eye[:] = 0.
        eye[p] = 1.
        assert np.array_equal(A[p], eye), p
    assert np.array_equal(A[np.ix_(rows, R.is_dup(N, axes).reshape(-1))], np.zeros((rows.size, R.is_dup(N, axes).sum())))
    B = A[np.ix_(rows, rows)]
    assert np.array_equal(B, B.T)
    if field is None:  # (the six neighbours of an unknown are among the columns: unknowns, Dirichlet points or the pin)
        np.testing.assert_allclose(A[rows].sum(axis=1), -sigma, rtol=1e-12, atol=1e-9)


def _solve(c, L, axes, sigma, cycles=12):
    """V(2,2) cycles of the numpy reference on the manufactured problem from u = 0 (Dirichlet values of u* on the faces):
    the max error against u* over the unique points (means removed when singular) and the residual factors"""
    ref = R.Problem(c, L, 2, sigma, None, axes)
    N = ref.N[-1]
    ustar, f = R.manufactured(N, axes, sigma)
    u0 = ustar.copy()
    u0[R.unique_mask(N, axes)] = 0.
    R.refresh(u0, axes)
    ref.u[-1][...] = u0
    ref.d[-1][...] = f
    n0 = R.residual(ref.u[-1], f, None, ref.h, sigma, axes)
    norms = np.concatenate([[n0], ref.vcycles(cycles)])
    m = R.unique_mask(N, axes)
    err = ref.u[-1][m] - ustar[m]
    if R.pinned(axes, sigma):
        err = err - err.mean()
    return np.abs(err).max(), norms


# the residual factor per V(2,2) cycle, measured with this reference (c = 5, 17^3 .. 65^3, cycles above 1e-10 of the
# initial residual): at most 0.262 with all three axes periodic and sigma = 0 (0.220 / 0.254 / 0.262 on the three sizes),
# 0.181 for mask 6, 0.11 with sigma = 1e3
FACTOR_BOUND = 0.3


@pytest.mark.parametrize("axes,sigma", [(7, 0.0), (7, 1e3), (6, 0.0), (6, 1e3)])
def test_numpy_vcycle_solves_manufactured_problem(axes, sigma):
    errs = []
    for L in (3, 4, 5):
        err, norms = _solve(5, L, axes, sigma, cycles=16)
        errs.append(err)
        above = norms[norms > 1e-10 * norms[0]]
        factors = above[1:] / above[:-1]
        assert factors.max() < FACTOR_BOUND, (L, factors)
        assert norms[-1] < 1e-11 * norms[0], norms
    # second order: the error against u* shrinks by about 4x per grid doubling
    for a, b in zip(errs, errs[1:]):
        assert 3.8 < a / b < 4.2, errs
