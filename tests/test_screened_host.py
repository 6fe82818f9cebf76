"""The screened operator (mg3d_ctx_set_shift) without a GPU: the numpy reference of tests/_screened_ref.py is the oracle's
V-cycle at sigma = 0, and the host-side coarse matrix of the library is the reference's construction at every sigma."""
import numpy as np
import pytest

import _oracle as O
import _screened_ref as S
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import P


@pytest.mark.parametrize("c,L", [(5, 4), (9, 3), (3, 5)])
def test_reference_at_sigma_zero_is_the_oracle(c, L):
    """sigma = 0: the composed reference reproduces orc_run_problem's finest u bit for bit, its norms to the summation
    tolerance (pairwise here, sequential there)."""
    want_norms, want_u, _, _ = O.run_problem(c, L, 2, 3)
    ref = S.Problem(c, L, 2, 0.0)
    ref.setup_test_problem()
    got = ref.vcycles(3)
    assert np.array_equal(ref.flat("u", L - 1), want_u)
    np.testing.assert_allclose(got, want_norms, rtol=1e-13)


def test_reference_fmg_at_sigma_zero_is_the_oracle():
    c, L = 5, 4
    H = O.Hierarchy(c, L)
    N = H.N[-1]
    O.lib().orc_fill_boundary(O.P(H.d[-1]), N, 1.0 / (N - 1))
    ref = S.Problem(c, L, 2, 0.0)
    ref.d[-1][...] = H.d[-1].reshape(N, N, N)
    O.lib().orc_fmg_initialize(H.ptrs(H.u), H.ptrs(H.d), H.ptrs(H.r), c, L, 2, 1.0, O.P(ref.LU))
    ref.fmg_initialize()
    for l in range(L):
        assert np.array_equal(ref.flat("u", l), H.u[l]), l


@pytest.mark.parametrize("N,h", [(3, 0.5), (5, 0.25), (9, 1.0 / 8)])
def test_coarse_matrix_shift(N, h):
    """mg3d_coarse_matrix_shift: at sigma = 0 the bytes of mg3d_coarse_matrix (and of the oracle's construction); at
    sigma > 0 the reference's matrix with the interior diagonal -(6 + sigma*h^2)/h^2."""
    n = N ** 3
    lib = M.lib()
    plain = np.zeros(n * n)
    lib.mg3d_coarse_matrix(P(plain), N, h)
    zero = np.zeros(n * n)
    lib.mg3d_coarse_matrix_shift(P(zero), N, h, 0.0)
    assert plain.tobytes() == zero.tobytes()
    assert zero.tobytes() == S.coarse_matrix(N, h, 0.0).tobytes()
    for sigma in (1.0, 1e4):
        got = np.zeros(n * n)
        lib.mg3d_coarse_matrix_shift(P(got), N, h, sigma)
        assert got.tobytes() == S.coarse_matrix(N, h, sigma).tobytes(), sigma
        assert not np.array_equal(got, plain)


def test_binding_exposes_the_shift():
    """the Python surface of the feature (the GPU tests drive it)"""
    for name in ("set_shift", "get_shift"):
        assert callable(getattr(M.Solver, name))
    assert callable(M.DistSolver.set_shift)
    for sym in ("mg3d_ctx_set_shift", "mg3d_ctx_get_shift", "mg3d_dist_set_shift", "mg3d_coarse_matrix_shift"):
        assert getattr(M.lib(), sym) is not None
