"""CPU restatement of mg3d_step_advance (include/mg3d.h): the theta-scheme for u_t = div(eps grad u) - kappa u + s over the
cycle of tests/_neumann_ref.py.  A step solves A_sigma u1 = d with the problem's operator at sigma = kappa + 1/(theta*dt):

    q    = A_sigma u0                              (_wpcg_ref.apply: the residual's expression, bit for bit)
    d    = -((a*u0 + c1*q) + b*s)                  at every unknown
    c0 = 1.0/(theta*dt);  a = c0/theta;  c1 = (1.0 - theta)/theta;  b = 1.0/theta

without a source d = -(a*u0 + c1*q); with theta == 1.0, c1 = 0 and q is not computed: d = -(a*u0 + b*s), or -(a*u0).
Then `cycles` V-cycles from u0 as the guess, or weighted PCG.  Test infrastructure only."""
import numpy as np

import _neumann_ref as NR
import _wpcg_ref as WR


def sigma_of(dt, theta, kappa):
    return kappa + 1.0 / (theta * dt)


def coefficients(dt, theta):
    c0 = 1.0 / (theta * dt)
    return c0 / theta, (1.0 - theta) / theta, 1.0 / theta


def rhs(prob, u0, s, dt, theta, kappa):
    """d on the block of unknowns; u0, s: (N, N, N) of the finest level (s None: no source).  prob.sigma must be
    sigma_of(dt, theta, kappa)"""
    assert prob.sigma == sigma_of(dt, theta, kappa)
    N = prob.N[-1]
    blk = NR.block(N, prob.axes, prob.faces)
    a, c1, b = coefficients(dt, theta)
    u = u0[blk]
    if theta == 1.0:
        if s is None:
            return -(a * u)
        return -(a * u + b * s[blk])
    q = WR.apply(prob, u0)
    if s is None:
        return -(a * u + c1 * q)
    return -((a * u + c1 * q) + b * s[blk])


def make_problem(c, L, nu, dt, theta, kappa, eps=None, axes=0, faces=0, grid_length=1.0):
    return NR.Problem(c, L, nu, sigma_of(dt, theta, kappa), eps, axes, faces, grid_length)


def write_rhs(prob, s, dt, theta, kappa):
    """d of the finest level at the unknowns only, from u of the finest level"""
    N = prob.N[-1]
    prob.d[-1][NR.block(N, prob.axes, prob.faces)] = rhs(prob, prob.u[-1], s, dt, theta, kappa)


def advance(prob, nsteps, cycles, s, dt, theta, kappa, method="vcycles", rtol=1e-8):
    """nsteps steps from prob.u[-1], in place.  Returns (one norm per step, iterations, converged): the last cycle's norm,
    0 iterations and False with V-cycles; _wpcg_ref.wpcg's last norm, the iterations over all steps and whether every
    step converged with method "wpcg" """
    norms, iters, conv = [], 0, True
    for _ in range(nsteps):
        write_rhs(prob, s, dt, theta, kappa)
        if method == "vcycles":
            norms.append(prob.vcycles(cycles)[-1])
        else:
            d = prob.d[-1].copy()
            x, nn, ok, _ = WR.wpcg(prob, prob.u[-1].copy(), d, rtol, 0.0, cycles)
            prob.u[-1][...] = x
            prob.d[-1][...] = d  # (the restatement's preconditioner uses the problem's u and d as work space)
            norms.append(nn[-1])
            iters += len(nn) - 1
            conv = conv and ok
    return np.array(norms), iters, (conv if method == "wpcg" else False)
