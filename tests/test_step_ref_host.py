"""The specification of mg3d_step_advance itself, on the CPU restatement tests/_step_ref.py (no GPU): a sign or coefficient
error in the four forms of the right-hand side cannot hide behind a kernel that restates it faithfully.

All at 17^3 (c = 5, L = 3), V(2,2).  `python tests/test_step_ref_host.py` prints the measured figures behind the two
rounding slacks below."""
import math

import numpy as np
import pytest

import _coef_ref as CR
import _neumann_ref as NR
import _step_ref as SR
import _wpcg_ref as WR

C, L, NU, N = 5, 3, 2, 17
H = 1.0 / (N - 1)
DT = 0.01
THETAS = (1.0, 0.5, 0.75)
KAPPAS = (0.0, 3.0)
AXES = (0, 5, 7)  # Dirichlet everywhere; i and k periodic; all periodic (sigma > 0: not singular)
STEPS = 4
CYCLES = 12

# Rounding slack of the amplification test, relative to ||u0||_2: 4 x the worst excess of ||u_n - g^n u0||_2 over the
# derived bound sum_k ||r_k||_2 / sigma, where that is positive.  Measured on the CPU restatement over the 18 cases below
# (3 theta x 2 kappa x 3 masks): no case exceeds the bound -- the error is 0.07 to 0.40 of it (bound 1.6e-15 to 8.2e-12
# ||u0||_2), the largest excess -1.1e-15 ||u0||_2 (theta = 0.5, kappa = 3, Dirichlet) -- so there is nothing to allow.
SLACK_AMP = 0.0
# Rounding slack of the conservation test, relative to ||w||_2 ||u0||_2: 4 x the worst excess of the per-step change of
# sum(w u) over ||w||_2 ||r||_2 / sigma, where that is positive.  Measured over theta in {1, 0.5}, 4 steps each: the
# largest excess is -7.5e-4 (two cycles on a jump of 100 between Neumann faces leave a residual that rounding is nowhere
# near): nothing to allow.
SLACK_MASS = 0.0


def _eigen(axes):
    """u0 = product of sin(pi x) on Dirichlet axes and sin(2 pi x) on periodic ones, and the eigenvalue of the discrete
    Laplacian: -(4/h^2) sin^2(pi h/2) per Dirichlet axis, -(4/h^2) sin^2(pi h) per periodic axis"""
    x = np.linspace(0.0, 1.0, N)
    f, lam = [], 0.0
    for ax in range(3):
        if NR.per(axes, ax):
            f.append(np.sin(2 * np.pi * x))
            lam -= (4.0 / (H * H)) * math.sin(math.pi * H) ** 2
        else:
            v = np.sin(np.pi * x)
            v[0] = v[-1] = 0.0  # Dirichlet 0 exactly
            f.append(v)
            lam -= (4.0 / (H * H)) * math.sin(math.pi * H / 2) ** 2
    u0 = np.ascontiguousarray(f[0][:, None, None] * f[1][None, :, None] * f[2][None, None, :])
    NR.refresh(u0, axes)
    return u0, lam


def _l2(a):
    return math.sqrt(math.fsum((a * a).reshape(-1)))


def amplification_excess(theta, kappa, axes):
    """(||u_n - g^n u0|| - sum ||r_k|| / sigma) / ||u0||, and (sum ||r_k|| / sigma) / ||u0||, over the unknowns"""
    prob = SR.make_problem(C, L, NU, DT, theta, kappa, None, axes, 0)
    u0, lam = _eigen(axes)
    lam -= kappa
    g = (1.0 + (1.0 - theta) * DT * lam) / (1.0 - theta * DT * lam)
    assert abs(g) <= 1.0
    blk = NR.block(N, axes, 0)
    prob.u[-1][...] = u0
    norms, _, _ = SR.advance(prob, STEPS, CYCLES, None, DT, theta, kappa)
    solve = float(np.sum(norms)) / prob.sigma
    err = _l2(prob.u[-1][blk] - g ** STEPS * u0[blk])
    n0 = _l2(u0[blk])
    return (err - solve) / n0, solve / n0


@pytest.mark.parametrize("axes", AXES)
@pytest.mark.parametrize("kappa", KAPPAS)
@pytest.mark.parametrize("theta", THETAS)
def test_amplification_factor(theta, kappa, axes):
    """an eigenvector of the discrete operator is multiplied by g = (1 + (1 - theta) dt lam) / (1 - theta dt lam) per step:
    ||u_n - g^n u0|| <= sum_k ||r_k|| / sigma (||A_sigma^-1|| <= 1/sigma, |g| <= 1) plus the rounding slack"""
    excess, solve = amplification_excess(theta, kappa, axes)
    print(theta, kappa, axes, "excess", excess, "solve term", solve)
    assert solve < 1e-10
    assert excess <= SLACK_AMP


@pytest.mark.parametrize("axes,faces,ball", [(0, 0, False), (0, 22, True), (4, 15, True), (7, 0, False)])
@pytest.mark.parametrize("kappa", KAPPAS)
@pytest.mark.parametrize("theta", THETAS)
def test_source_fixed_point(theta, kappa, axes, faces, ball):
    """with s = -(L_h - kappa) v*, u = v* is a fixed point of the step: d = A_sigma v* to rounding"""
    eps = CR.ball_eps(N, 100.) if ball else None
    prob = SR.make_problem(C, L, NU, DT, theta, kappa, eps, axes, faces)
    blk = NR.block(N, axes, faces)
    v = WR.random_guess(N, axes, faces, seed=3, dirichlet=True)
    q = WR.apply(prob, v)
    c0 = 1.0 / (theta * DT)
    s = np.zeros((N, N, N))
    s[blk] = -(q + c0 * v[blk])  # (L_h - kappa) v = A_sigma v + c0 v
    d = SR.rhs(prob, v, s, DT, theta, kappa)
    a, c1, b = SR.coefficients(DT, theta)
    bound = 64 * 2.0 ** -53 * (a * _l2(v[blk]) + c1 * _l2(q) + b * _l2(s[blk]))
    print(theta, kappa, axes, faces, _l2(d - q), bound)
    assert _l2(d - q) <= bound


def conservation_excess(theta):
    """per step: (|change of sum(w u)| - ||w|| ||r|| / sigma) / (||w|| ||u0||), all six faces Neumann, kappa = 0, s = 0"""
    prob = SR.make_problem(C, L, NU, DT, theta, 0.0, CR.ball_eps(N, 100.), 0, 63)
    w = NR.weights(N, 0, 63)
    wn = _l2(w)
    u0 = WR.random_guess(N, 0, 63, seed=8)
    prob.u[-1][...] = u0
    mass = lambda: math.fsum((w * prob.u[-1]).reshape(-1))
    out, m = [], mass()
    for _ in range(STEPS):
        norms, _, _ = SR.advance(prob, 1, 2, None, DT, theta, 0.0)
        m1 = mass()
        out.append((abs(m1 - m) - wn * norms[0] / prob.sigma) / (wn * _l2(u0)))
        m = m1
    return out


@pytest.mark.parametrize("theta", (1.0, 0.5))
def test_conservation_between_neumann_faces(theta):
    """w, the trapezoid weight, is the left null vector of L: w.d = -sigma w.u0 for every theta (kappa = 0), so the
    weighted mass changes per step by w.r / sigma, at most ||w|| ||r|| / sigma (Cauchy-Schwarz), plus the rounding slack"""
    for k, ex in enumerate(conservation_excess(theta)):
        print(theta, k, ex)
        assert ex <= SLACK_MASS


def test_backward_euler_does_not_apply_the_operator():
    """theta == 1.0: q is not computed -- rhs works on a problem whose operator cannot be applied"""

    class NoOperator:
        sigma = SR.sigma_of(DT, 1.0, 0.0)
        N = [5, 9, N]
        axes, faces = 0, 0

        @property
        def h(self):
            raise AssertionError("theta = 1 applied the operator")

        eps = h

    rng = np.random.default_rng(4)
    u0, s = rng.uniform(-1, 1, (N, N, N)), rng.uniform(-1, 1, (N, N, N))
    a, _, b = SR.coefficients(DT, 1.0)
    blk = NR.block(N, 0, 0)
    assert np.array_equal(SR.rhs(NoOperator(), u0, None, DT, 1.0, 0.0), -(a * u0[blk]))
    assert np.array_equal(SR.rhs(NoOperator(), u0, s, DT, 1.0, 0.0), -(a * u0[blk] + b * s[blk]))
    NoOperator.sigma = SR.sigma_of(DT, 0.5, 0.0)
    with pytest.raises(AssertionError, match="applied the operator"):
        SR.rhs(NoOperator(), u0, None, DT, 0.5, 0.0)


if __name__ == "__main__":
    worst = max((amplification_excess(t, k, ax)[0], t, k, ax) for t in THETAS for k in KAPPAS for ax in AXES)
    print("amplification: largest excess / ||u0||", worst)
    for t in (1.0, 0.5):
        print("conservation, theta", t, "excess per step", conservation_excess(t))
