"""CPU reference of full multigrid for the caller's problem (mg3d_fmg_interpolate, mg3d_fmg_solve) on top of
tests/_neumann_ref.py, the most general reference: the cubic interpolation with the library's term order, a V-cycle that
keeps its guess on the level it starts from, and the solve built from them with that module's own restriction, direct
solve and cycle.

Per axis (coarse side Nc, fine index x): x = 2I copies coarse I; x = 2I+1 takes coarse I-1, I, I+1, I+2 with -1/16, 9/16,
9/16, -1/16, an index outside the unique range wrapped modulo Nc-1 on a periodic axis and reflected at a Neumann face
(-1 -> 1, Nc -> Nc-2); next to a Dirichlet face the one-sided cubic over the four points nearest the face (low: coarse 0,
1, 2, 3 with 5/16, 15/16, -5/16, 1/16; high: coarse Nc-4 .. Nc-1 with 1/16, -5/16, 15/16, 5/16); with Nc < 4 coarse I, I+1
with 1/2, 1/2.  The value is sum_i(wi * sum_j(wj * sum_k(wk * u))): the k pass first, then j, then i; every sum starts
with its first term and adds the others left to right.  Test infrastructure only."""
import numpy as np

import _neumann_ref as NR

per, neu = NR.per, NR.neu

CENTRAL = (-0.0625, 0.5625, 0.5625, -0.0625)
ONE_SIDED = (0.3125, 0.9375, -0.3125, 0.0625)  # from the face inwards


def axis_terms(x, Nc, periodic, nlo, nhi):
    """[(coarse index, weight), ...] of fine index x in summation order"""
    I = x >> 1
    if not x & 1:
        return [(I, 1.0)]
    if Nc < 4:
        return [(I, 0.5), (I + 1, 0.5)]
    if periodic:
        return [((I - 1 + t) % (Nc - 1), CENTRAL[t]) for t in range(4)]
    if I == 0 and not nlo:
        return [(t, ONE_SIDED[t]) for t in range(4)]
    if I + 2 == Nc and not nhi:
        return [(Nc - 4 + t, ONE_SIDED[3 - t]) for t in range(4)]
    idx = [I - 1, I, I + 1, I + 2]
    if idx[0] < 0:
        idx[0] = 1
    if idx[3] > Nc - 1:
        idx[3] = Nc - 2
    return list(zip(idx, CENTRAL))


def _axis_pass(a, ax, Nc, lo, hi, periodic, nlo, nhi):
    """the interpolation along one axis: fine indices lo .. hi of that axis from the coarse ones"""
    out = []
    for x in range(lo, hi + 1):
        terms = axis_terms(x, Nc, periodic, nlo, nhi)
        acc = terms[0][1] * a.take(terms[0][0], axis=ax)
        for c, w in terms[1:]:
            acc = acc + w * a.take(c, axis=ax)
        out.append(acc)
    return np.stack(out, axis=ax)


def interpolant(uc, axes, faces):
    """the interpolant at the block of unknowns of the fine level (NR.block)"""
    Nc = uc.shape[0]
    Nf = 2 * Nc - 1
    a = np.asarray(uc, dtype=np.float64)
    for ax in (2, 1, 0):
        lo, hi = NR.lo_hi(Nf, axes, faces, ax)
        a = _axis_pass(a, ax, Nc, lo, hi, per(axes, ax), neu(faces, ax, 0), neu(faces, ax, 1))
    return a


def interpolate(uc, uf, axes, faces):
    """k_fmg_interp: every unknown of uf, and its periodic duplicates, overwritten; Dirichlet points stay"""
    Nf = uf.shape[0]
    assert Nf == 2 * uc.shape[0] - 1
    NR.put(uf, interpolant(uc, axes, faces), NR.block(Nf, axes, faces), axes)


def dirichlet_mask(N, axes, faces):
    """points on a face of a non-periodic axis that is not a Neumann face"""
    g = np.zeros((N, N, N), dtype=bool)
    for ax in range(3):
        if per(axes, ax):
            continue
        for hi_, end in ((0, 0), (1, N - 1)):
            if not neu(faces, ax, hi_):
                s = [slice(None)] * 3
                s[ax] = end
                g[tuple(s)] = True
    return g


def vcycle(prob, q, keep_guess=True):
    """Problem.vcycle from level q, except that with keep_guess u[q] is the guess as it stands (the levels below start
    from zero as always); returns the post-smoothing residual norm of level q"""
    if not keep_guess or q == prob.L - 1 or q == 0:
        return prob.vcycle(q)
    v = prob.u[q]
    for _ in range(prob.nu):
        prob.colour_pass(q, 1)
        prob.colour_pass(q, 0)
    prob.residual(q, prob.r[q])
    NR.restrict(prob.r[q], prob.d[q - 1], prob.axes, prob.faces)
    prob.vcycle(q - 1)
    NR.prolong(prob.u[q - 1], v, prob.axes, prob.faces)
    for _ in range(prob.nu):
        prob.colour_pass(q, 0)
        prob.colour_pass(q, 1)
    return prob.residual(q)


def fmg_solve(prob, cycles=1, keep_guess=True, interp=interpolate):
    """mg3d_fmg_solve on prob.u[-1] (its Dirichlet points) and prob.d[-1]; returns the residual norm after the last
    finest-level cycle.  keep_guess = False discards the guess below the finest level, as the reference's own F-cycle
    start does; interp(uc, uf, axes, faces) may be another interpolation that overwrites the unknowns."""
    assert cycles >= 1
    L, axes, faces = prob.L, prob.axes, prob.faces
    for l in range(L - 1, 0, -1):
        NR.restrict(prob.d[l], prob.d[l - 1], axes, faces)
        prob.u[l - 1][...] = prob.u[l][::2, ::2, ::2]
    m = dirichlet_mask(prob.N[0], axes, faces)
    if L > 1:
        prob.d[0][m] = prob.u[0][m]
        NR.coarse_solve(prob.LU, prob.d[0], prob.u[0], axes, faces, prob.sigma)
    else:  # one level: d is the caller's and stays
        b = prob.d[0].copy()
        b[m] = prob.u[0][m]
        NR.coarse_solve(prob.LU, b, prob.u[0], axes, faces, prob.sigma)
        return 0.0
    norm = 0.0
    for l in range(1, L):
        interp(prob.u[l - 1], prob.u[l], axes, faces)
        for _ in range(cycles):
            norm = vcycle(prob, l, keep_guess)
    return norm


def manufactured(N, axes, faces, sigma, eps=None, grad_eps=None):
    """NR.manufactured with another factor along an axis that has two Dirichlet faces: sin(pi x) + 1 + x instead of
    1 + x - x^2.  The 7-point stencil differentiates a quadratic exactly, so with the constant operator and Dirichlet
    faces all around NR.manufactured has NO discretisation error (u_h = u* to rounding) and nothing to compare an
    algebraic error with; this factor is smooth, has inhomogeneous boundary values and a truncation error."""
    def factors(ax):
        if per(axes, ax) or neu(faces, ax, 0) or neu(faces, ax, 1):
            return NR.axis_factors(N, axes, faces, ax)
        x = np.linspace(0.0, 1.0, N)
        return np.sin(np.pi * x) + 1.0 + x, np.pi * np.cos(np.pi * x) + 1.0, -np.pi * np.pi * np.sin(np.pi * x)
    F = [factors(ax) for ax in range(3)]
    o = NR._outer
    u = o(F[0][0], F[1][0], F[2][0])
    lap = o(F[0][2], F[1][0], F[2][0]) + o(F[0][0], F[1][2], F[2][0]) + o(F[0][0], F[1][0], F[2][2])
    if eps is None:
        f = lap - sigma * u
    else:
        gu = [o(F[0][1], F[1][0], F[2][0]), o(F[0][0], F[1][1], F[2][0]), o(F[0][0], F[1][0], F[2][1])]
        f = eps * lap + grad_eps[0] * gu[0] + grad_eps[1] * gu[1] + grad_eps[2] * gu[2] - sigma * u
    u, f = np.ascontiguousarray(u), np.ascontiguousarray(f)
    for a in (u, f):
        NR.refresh(a, axes)
    return u, f


def trilinear(uc, uf, axes, faces):
    """the prolongation's weights as an interpolation that overwrites: for comparison only"""
    Nf = uf.shape[0]
    z = np.zeros_like(uf)
    NR.prolong(uc, z, axes, faces)
    blk = NR.block(Nf, axes, faces)
    NR.put(uf, z[blk], blk, axes)
