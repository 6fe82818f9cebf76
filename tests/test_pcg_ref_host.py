"""The CPU restatement of mg3d_pcg_solve (tests/_pcg_ref.py) checked on its own, without a GPU: the recurrence residual
tracks the true one, the converged iterate is the solution of the assembled operator, and its `apply` is the operator the
other references state."""
import numpy as np
import pytest

import _coef_ref as CR
import _pcg_ref as PR
import _periodic_ref as P

CASES = {"ball100": dict(eps="ball", sigma=0.0), "constant": dict(eps=None, sigma=0.0), "sigma10": dict(eps=None, sigma=10.0)}


def _problem(c, L, case):
    N = (c - 1) * (1 << (L - 1)) + 1
    eps = CR.ball_eps(N, 100.) if case["eps"] == "ball" else None
    return N, PR.make_problem(c, L, 2, case["sigma"], eps)


def _data(N, seed):
    rng = np.random.default_rng(seed)
    x0 = np.zeros((N, N, N))
    x0[1:-1, 1:-1, 1:-1] = rng.uniform(-1, 1, (N - 2,) * 3)
    face = np.ones((N, N, N), dtype=bool)
    face[1:-1, 1:-1, 1:-1] = False
    x0[face] = rng.uniform(-1, 1, int(face.sum()))  # Dirichlet values
    d = rng.uniform(-1, 1, (N, N, N))
    return x0, d


@pytest.mark.parametrize("name", sorted(CASES))
def test_recurrence_residual_is_the_true_residual(name):
    """17^3 (c = 5, L = 3): ||r_k|| of the recurrence against ||d - A x_k|| computed afresh, at every k <= 10, to 1e-10
    relative to the true one -- plus the rounding of the fresh evaluation itself: d - A x_k is a difference of terms of the
    size of r_0 however small r_k is, each rounded to 2^-53 relative with 8 operations per point, so the two can only be
    compared to about 1e-15 ||r_0||; 1e-14 ||r_0|| is allowed (at k = 7 of the ball the recurrence is down to 5e-7 ||r_0||
    and the two differ by 1e-16 ||r_0||, which is 2e-10 of r_7)."""
    N, prob = _problem(5, 3, CASES[name])
    x0, d = _data(N, 17)
    hist = []
    _, norms, _ = PR.pcg(prob, x0, d, 0.0, 1e-300, 10, history=hist)
    assert len(norms) == 11 and len(hist) == 10
    assert abs(norms[0] - PR.true_residual_norm(prob, x0, d)) <= 1e-15 * norms[0]
    for k, xk in enumerate(hist, start=1):
        true = PR.true_residual_norm(prob, xk, d)
        print(name, k, norms[k], true, abs(norms[k] - true) / true)
        assert abs(norms[k] - true) <= 1e-10 * true + 1e-14 * norms[0], (k, norms[k], true)
    assert norms[10] < 1e-6 * norms[0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_converged_iterate_solves_the_assembled_operator(name):
    """9^3 (c = 5, L = 2): after convergence to rtol 1e-12 the iterate is numpy.linalg.solve of the assembled matrix
    (identity rows on the Dirichlet faces).  The bound is the conditioning of that solve: cond(A) ~ 1e4 * eps ratio."""
    N, prob = _problem(5, 2, CASES[name])
    x0, d = _data(N, 9)
    x, norms, converged = PR.pcg(prob, x0, d, 1e-12, 0.0, 40)
    assert converged and len(norms) <= 25
    e = None if CASES[name]["eps"] is None else CR.ball_eps(N, 100.)
    A = P.coarse_matrix(N, prob.h, e, prob.sigma, 0).reshape(N ** 3, N ** 3)
    b = d.copy()
    face = np.ones((N, N, N), dtype=bool)
    face[1:-1, 1:-1, 1:-1] = False
    b[face] = x0[face]
    want = np.linalg.solve(A, b.reshape(-1)).reshape(N, N, N)
    assert np.array_equal(x[face], x0[face])
    err = np.abs(x - want).max() / np.abs(want).max()
    print(name, len(norms) - 1, err)
    assert err <= 1e-10


def test_apply_is_the_references_operator():
    """PR.apply against _coef_ref.apply (eps) bit for bit, and against the assembled periodic matrix"""
    N = 9
    rng = np.random.default_rng(3)
    v = rng.uniform(-1, 1, (N, N, N))
    prob = PR.make_problem(5, 2, 2, 3.0, CR.exp_eps(N))
    assert np.array_equal(PR.apply(prob, v), CR.apply(v, prob.eps[-1], prob.h, 3.0)[1:-1, 1:-1, 1:-1])
    per = PR.make_problem(5, 2, 2, 2.0, None, axes=6)
    P.refresh(v, 6)
    A = P.coarse_matrix(N, per.h, None, 2.0, 6).reshape(N ** 3, N ** 3)
    blk = P.unique_block(N, 6)
    np.testing.assert_allclose(PR.apply(per, v), (A @ v.reshape(-1)).reshape(N, N, N)[blk], rtol=0, atol=1e-11)
