"""CPU reference of the nonlinear solves (mg3d_nl_residual, mg3d_nl_solve): the evaluation and the damped Newton iteration in
numpy.  The linear part of the evaluation is _shift_field_ref.residual_field without a field, the linear solves run on
_shift_field_ref.Hierarchy (its V-cycle, or its wpcg).  The nonlinear part uses numpy's exp / sinh / cosh, which are not the
device library's bit for bit: tests compare it by error bounds, never by bits.  Test infrastructure only.

    A u - g0*g*phi(beta*(u - uref)) = d         F = d - (A u - gp*ph),  s = (gp*beta)*dph         (include/mg3d.h)
"""
import math

import numpy as np

import _mask_ref as MR
import _neumann_ref as NR
import _shift_field_ref as SF

ARMIJO = 1e-4


class Term:
    """kind "exp" or "sinh", the scalars of mg3d_nl_setup and the optional weight g, (N, N, N)"""

    def __init__(self, kind, g0=1.0, beta=1.0, uref=0.0, g=None):
        assert kind in ("exp", "sinh")
        self.kind, self.g0, self.beta, self.uref, self.g = kind, float(g0), float(beta), float(uref), g


def phi(kind, w):
    """(ph, dph) in w's own precision"""
    if kind == "exp":
        ph = np.exp(w)
        return ph, ph
    return np.sinh(w), np.cosh(w)


def evaluate(u, d, e, h, sigma, axes, faces, mask, term):
    """(F, s) on the block of unknowns, both 0. at the fixed ones: the kernel's expressions in the kernel's order"""
    N = u.shape[0]
    blk = NR.block(N, axes, faces)
    lin = SF.residual_field(u, d, e, h, sigma, axes, faces, mask, None)
    with np.errstate(all="ignore"):
        w = term.beta * (u[blk] - term.uref)
        ph, dph = phi(term.kind, w)
        gp = term.g0 * term.g[blk] if term.g is not None else np.full(w.shape, term.g0)
        F = lin + gp * ph
        s = (gp * term.beta) * dph
    fx = MR.fixed(SF._mask(mask, N), axes, faces)[blk]
    F[fx] = 0.
    s[fx] = 0.
    return F, s


def norm(F):
    with np.errstate(all="ignore"):
        return float(np.sqrt((F * F).sum()))


def full(N, vals, axes, faces):
    """the block of unknowns as an (N, N, N) field: 0. at Dirichlet points, duplicates written"""
    a = np.zeros((N, N, N))
    NR.put(a, vals, NR.block(N, axes, faces), axes)
    return a


class Problem:
    """the context a solve runs on: hierarchy shape (c, L, nu), operator (sigma, eps, axes, faces, mask) and the term"""

    def __init__(self, c, L, term, nu=2, sigma=0.0, eps=None, axes=0, faces=0, mask=None, grid_length=1.0):
        self.c, self.L, self.nu, self.sigma, self.eps, self.axes, self.faces, self.mask = c, L, nu, sigma, eps, axes, faces, mask
        self.term, self.grid_length = term, grid_length
        self.N = (c - 1) * (1 << (L - 1)) + 1
        self.h = grid_length / (self.N - 1)

    def evaluate(self, u, d):
        return evaluate(u, d, self.eps, self.h, self.sigma, self.axes, self.faces, self.mask, self.term)

    def linearised(self, s_blk):
        """the hierarchy of A - s, s given on the block of unknowns"""
        return SF.Hierarchy(self.c, self.L, self.nu, self.sigma, self.eps, self.axes, self.faces, self.mask,
                            full(self.N, s_blk, self.axes, self.faces), self.grid_length)

    def linear_solve(self, s_blk, F_blk, method, cycles, rtol_lin):
        """delta, (N, N, N), from a zero guess; and the iterations spent"""
        prob = self.linearised(s_blk)
        rhs = full(self.N, F_blk, self.axes, self.faces)
        if method == "vcycles":
            prob.u[-1][...] = 0.
            prob.d[-1][...] = rhs
            for _ in range(cycles):
                prob.vcycle()
            return prob.u[-1].copy(), cycles
        x, norms, _, _, _ = SF.wpcg(prob, np.zeros((self.N,) * 3), rhs, rtol_lin, 0.0, cycles)
        return x, len(norms) - 1


def trial(x, delta, lam, axes, faces, mask):
    """t = x + lam*delta at the unknowns that are not fixed, x elsewhere, duplicates written"""
    N = x.shape[0]
    blk = NR.block(N, axes, faces)
    t = x.copy()
    vals = x[blk] + lam * delta[blk]
    fx = MR.fixed(SF._mask(mask, N), axes, faces)[blk]
    vals[fx] = x[blk][fx]
    NR.put(t, vals, blk, axes)
    return t


def solve(P, u0, d, max_newton=20, cycles=2, method="vcycles", rtol_lin=1e-2, rtol=1e-8, atol=0.0, max_halvings=10):
    """mg3d_nl_solve.  Returns (u, norms, info) with info the keys of the binding's dict plus "halvings_per_step" """
    x = np.array(u0, dtype=np.float64).copy()
    F, s = P.evaluate(x, d)
    n = norm(F)
    norms = [n]
    info = {"iterations": 0, "converged": False, "halvings": 0, "linear_iterations": 0, "last_lambda": 0.0, "norm0": n,
            "norm": n, "halvings_per_step": []}
    while True:
        info["converged"] = bool(n <= max(atol, rtol * norms[0]))
        if info["converged"] or info["iterations"] >= max_newton:
            break
        delta, its = P.linear_solve(s, F, method, cycles, rtol_lin)
        info["linear_iterations"] += its
        lam, accepted, halved = 1.0, False, 0
        for k in range(max_halvings + 1):
            t = trial(x, delta, lam, P.axes, P.faces, P.mask)
            Ft, st = P.evaluate(t, d)
            nt = norm(Ft)
            if math.isfinite(nt) and np.isfinite(st).all() and nt < (1.0 - ARMIJO * lam) * n:
                accepted = True
                break
            if k < max_halvings:
                lam *= 0.5
                halved += 1
        info["halvings"] += halved
        if not accepted:
            break
        x, F, s, n = t, Ft, st, nt
        norms.append(n)
        info["iterations"] += 1
        info["last_lambda"] = lam
        info["norm"] = n
        info["halvings_per_step"].append(halved)
    return x, np.array(norms), info


def undamped(P, u0, d, steps, rtol_lin=1e-10, max_iters=60):
    """The loop of _shift_field_ref.pb_newton for this equation, no line search: each step solves
    (A - s_k) u_{k+1} = d + N(u_k) - s_k u_k  from u_k by PCG to rtol_lin.  Returns the residual norms ||F(u_k)||, k = 0 ..,
    ending early at the first one that is not finite"""
    x = np.array(u0, dtype=np.float64).copy()
    out = []
    for _ in range(steps + 1):
        with np.errstate(all="ignore"):
            F, s = P.evaluate(x, d)
            out.append(norm(F))
            if not math.isfinite(out[-1]) or not np.isfinite(s).all() or len(out) == steps + 1:
                break
            # F = d - A x + N(x)  =>  d + N(x) - s x = F + A x - s x = F + (A - s) x: solve for the new iterate from x
            rhs = full(P.N, F + SF.apply(x, P.eps, P.h, P.sigma, P.axes, P.faces, P.mask, full(P.N, s, P.axes, P.faces)),
                       P.axes, P.faces)
            prob = P.linearised(s)
            x, _, _, _, _ = SF.wpcg(prob, x, rhs, rtol_lin, 0.0, max_iters)
    return np.array(out)


# ---- the problems of the tests

def boltzmann_problem(N, g0=50.0, beta=1.0):
    """Boltzmann electrons against a Gaussian ion cloud, grounded walls:  Delta u - g0 exp(beta u) = -rho  on [0, 1]^3,
    rho = 4e4 exp(-((x-.5)^2 + (y-.5)^2 + (z-.4)^2)/0.02), from u0 = 0.  Returns (term, u0, d)"""
    x = np.linspace(0.0, 1.0, N)
    r2 = (x[:, None, None] - 0.5) ** 2 + (x[None, :, None] - 0.5) ** 2 + (x[None, None, :] - 0.4) ** 2
    rho = 4e4 * np.exp(-r2 / 0.02)
    return Term("exp", g0, beta, 0.0), np.zeros((N, N, N)), np.ascontiguousarray(-rho)


def pb_start(N, kappa2=4.0):
    """_shift_field_ref.pb_problem for the solver: (term, u0 = the Dirichlet values of u* and zero inside, d = f, u*)"""
    ustar, f = SF.pb_problem(N, kappa2)
    u0 = ustar.copy()
    u0[1:-1, 1:-1, 1:-1] = 0.
    return Term("sinh", kappa2, 1.0, 0.0), u0, f, ustar


def lambda_min(N):
    """the smallest eigenvalue of -Delta_h on N^3 points of the unit cube with Dirichlet faces: (12/h^2) sin^2(pi h/2)"""
    h = 1.0 / (N - 1)
    return 12.0 / (h * h) * math.sin(math.pi * h / 2) ** 2


# What the restatement needs on the Boltzmann problem with cycles = 2 V-cycles, rtol = 1e-8, max_halvings = 10
# (tests/test_nl_ref_host.py asserts these): (N, beta) -> (iterations, the largest halving count of a step)
BOLTZMANN_NEEDS = {(17, 1.0): (7, 5), (17, 10.0): (8, 7), (33, 1.0): (7, 5), (33, 10.0): (8, 7)}


def caps(N, beta):
    """(max_newton, max_halvings) of the GPU tests: the restatement's iterations + 2, its largest halving count + 1"""
    it, hv = BOLTZMANN_NEEDS[(N, beta)]
    return it + 2, hv + 1
