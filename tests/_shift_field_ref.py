"""CPU reference of the screening field (mg3d_ctx_set_shift_field): the operator div(eps grad u) - (sigma + s_p) u in numpy
with the library's arithmetic -- colour pass, residual and A p with the per-point diagonal, the restriction of the field,
the coarse matrix, the pin and projection rules, the V-cycle, the (weighted) PCG over it, the stepper's right-hand side and
mg3d_fmg_solve.  Built on tests/_mask_ref.py by import: with s = None every function returns what that module returns, bit
for bit.

s is an (N, N, N) array of doubles >= 0.  The arithmetic is that of the eps stencils (_coef_ref._sum_diag on the extended
field of _neumann_ref.ext) with one change: the sum s(um) and D -- the sum of the six face means, exactly 6.0 over eps = 1 --
stay, and dg = D + (sigma + s_p)*hSq per point, in this order; the smoother divides by dg also when eps is None, where the
stencil runs over an array of ones (0.5*(1 + 1) is 1, 1*v is v).  A mask is applied as _mask_ref applies it: run the
unmasked operator, put the old values back.  mask = None stands for the all-zero mask.  Test infrastructure only."""
import math

import numpy as np

import _coef_ref as CR
import _fmg_ref as FR
import _mask_ref as MR
import _neumann_ref as NR
import _oracle as O
import _pcg_ref as PR
import _step_ref as SR
import _wpcg_ref as WR


def _mask(mask, N):
    return np.zeros((N, N, N), dtype=np.uint8) if mask is None else np.asarray(mask).reshape(N, N, N)


def stored(s, axes):
    """the field a level keeps: the caller's, periodic duplicates taking their sources' (mg3d_ctx_get_shift_field)"""
    a = np.array(s, dtype=np.float64).copy()
    NR.refresh(a, axes)
    return a


def restrict_field(s, L, axes, faces):
    """the fields of levels 0 .. L-1 from the finest one: s_{l-1} = the context's restriction of s_l (_neumann_ref.restrict:
    full weighting at every coarse unknown with wrapped or reflected taps, Dirichlet faces injected, duplicates copied)"""
    out = [stored(s, axes)]
    for _ in range(L - 1):
        n = (out[0].shape[0] + 1) // 2
        c = np.zeros((n, n, n))
        NR.restrict(out[0], c, axes, faces)
        out.insert(0, c)
    return out


def inject_field(s, L, axes):
    """the rule the library does NOT use (tools/shift_field_convergence.py measures both): s_{l-1}[I,J,K] = s_l[2I,2J,2K]"""
    return CR.inject(stored(s, axes), L)


def positive(s, axes, faces):
    """the unknowns at which the field is > 0, (N, N, N) bool"""
    if s is None:
        return np.zeros((1, 1, 1), dtype=bool)
    return (np.asarray(s) > 0.) & NR.unknown_mask(s.shape[0], axes, faces)


def _sum_diag(u, e, h, sigma, axes, faces, s):
    """neighbour sum, diagonal and centre value at every unknown"""
    if s is None:
        return NR._sum_diag(u, e, h, sigma, axes, faces)
    N = u.shape[0]
    X = NR.ext(u, axes, faces)
    E = NR.ext(np.ones((N, N, N)) if e is None else e, axes, faces)
    sm, dg = CR._sum_diag(X, E, (sigma + s[NR.block(N, axes, faces)]) * (h * h))
    return sm, dg, X[1:-1, 1:-1, 1:-1]


def colour_pass(u, d, e, h, sigma, axes, faces, colour, mask, s):
    N = u.shape[0]
    mask = _mask(mask, N)
    if s is None:
        return MR.colour_pass(u, d, e, h, sigma, axes, faces, colour, mask)
    keep = MR._keep(mask, axes, faces)
    old = u[keep].copy()
    blk = NR.block(N, axes, faces)
    hSq = h * h
    sm, dg, _ = _sum_diag(u, e, h, sigma, axes, faces, s)
    new = (sm - hSq * d[blk]) / dg
    vals = u[blk].copy()
    m = NR._colour_mask(N, axes, faces, colour)
    vals[m] = new[m]
    NR.put(u, vals, blk, axes)
    u[keep] = old


def residual_field(u, d, e, h, sigma, axes, faces, mask, s):
    """diff on the block of unknowns, 0. at the fixed ones"""
    N = u.shape[0]
    mask = _mask(mask, N)
    if s is None:
        return MR.residual_field(u, d, e, h, sigma, axes, faces, mask)
    blk = NR.block(N, axes, faces)
    invHsq = 1.0 / (h * h)
    sm, dg, c = _sum_diag(u, e, h, sigma, axes, faces, s)
    with np.errstate(all="ignore"):
        diff = d[blk] - invHsq * (sm - dg * c)
    diff[MR.fixed(mask, axes, faces)[blk]] = 0.
    return diff


def residual(u, d, e, h, sigma, axes, faces, mask, s, r=None):
    diff = residual_field(u, d, e, h, sigma, axes, faces, mask, s)
    if r is not None:
        NR.put(r, diff, NR.block(u.shape[0], axes, faces), axes)
    return float(np.sqrt((diff * diff).sum()))


def exact_residual_norm(u, d, e, h, sigma, axes, faces, mask, s):
    diff = residual_field(u, d, e, h, sigma, axes, faces, mask, s)
    return math.sqrt(math.fsum((diff * diff).reshape(-1)))


def apply(v, e, h, sigma, axes, faces, mask, s):
    """A v at the unknowns, 0. at the fixed ones: the residual's expression with d = 0, negated"""
    return -residual_field(v, np.zeros_like(v), e, h, sigma, axes, faces, mask, s)


def _any_fixed(mask, axes, faces):
    return mask is not None and bool(MR.fixed(mask, axes, faces).any())


def pinned(axes, faces, sigma, mask0, s0):
    """the pin of unknown (0,0,0) of level 0: the mask's condition, and level 0's field > 0 at no unknown of level 0"""
    return NR.pinned(axes, faces, sigma) and not _any_fixed(mask0, axes, faces) and not positive(s0, axes, faces).any()


def singular(axes, faces, sigma, mask0, mask_top, s0, s_top):
    """mg3d_wpcg_solve projects: pinned, no fixed unknown on the finest level and the finest field > 0 at no unknown"""
    return (pinned(axes, faces, sigma, mask0, s0) and not _any_fixed(mask_top, axes, faces)
            and not positive(s_top, axes, faces).any())


def coarse_matrix(N, h, e, sigma, axes, faces, mask, s):
    """mg3d_coarse_matrix_field in numpy: mg3d_coarse_matrix_mask when s is None; otherwise its rows with the diagonal
    -((D + (sigma + s_p)*hSq) * invHsq), D = 6.0 without eps, and the pin only where s is > 0 at no unknown"""
    mask = None if mask is None else np.asarray(mask).reshape(N, N, N)
    if s is None:
        return MR.coarse_matrix(N, h, e, sigma, axes, faces, mask)
    s = np.asarray(s, dtype=np.float64).reshape(N, N, N)
    n = N ** 3
    A = np.zeros((n, n))
    hSq = h * h
    invHsq = 1.0 / hSq
    idx = np.arange(n).reshape(N, N, N)
    unk = NR.unknown_mask(N, axes, faces) & ~MR.fixed(_mask(mask, N), axes, faces)
    if pinned(axes, faces, sigma, mask, s):
        unk[0, 0, 0] = False
    A[idx[~unk], idx[~unk]] = 1.0
    blk = NR.block(N, axes, faces)
    inner = unk[blk]
    p = idx[blk][inner]
    X = NR.ext(idx, axes, faces)
    nb = [X[:-2, 1:-1, 1:-1], X[2:, 1:-1, 1:-1], X[1:-1, :-2, 1:-1], X[1:-1, 2:, 1:-1], X[1:-1, 1:-1, :-2],
          X[1:-1, 1:-1, 2:]]
    nb = [q[inner] for q in nb]
    sp = s.reshape(-1)[p]
    if e is None:
        off = 1.0 * invHsq
        for q in nb:
            A[p, q] += off
        A[p, p] = -((6.0 + (sigma + sp) * hSq) * invHsq)
    else:
        ee = np.asarray(e, dtype=np.float64).reshape(-1)
        ep = ee[p]
        a = [0.5 * (ep + ee[q]) for q in nb]
        for ai, q in zip(a, nb):
            A[p, q] += ai * invHsq
        D = a[0] + a[1]
        for ai in a[2:]:
            D = D + ai
        A[p, p] = -((D + (sigma + sp) * hSq) * invHsq)
    return np.ascontiguousarray(A.reshape(-1))


def coarse_lu(N, h, e, sigma, axes, faces, mask, s):
    A = coarse_matrix(N, h, e, sigma, axes, faces, mask, s)
    O.lib().orc_lu_factor(O.P(A), N ** 3)
    return A


def coarse_solve(LU, d0, u0, axes, faces, pin, mask0, one_level=False):
    """_mask_ref.coarse_solve with the pin given: b = d with 0 at the duplicates, the pin and the fixed unknowns"""
    N = d0.shape[0]
    b = np.ascontiguousarray(d0).copy()
    fx = MR.fixed(_mask(mask0, N), axes, faces)
    b[fx] = u0[fx] if one_level else 0.
    b[NR.is_dup(N, axes)] = 0.
    if pin:
        b[0, 0, 0] = 0.
    x = np.zeros(N ** 3)
    O.lib().orc_lu_solve(O.P(LU), N ** 3, O.P(b.reshape(-1)), O.P(x))
    u0[...] = x.reshape(N, N, N)
    NR.refresh(u0, axes)


class Hierarchy(MR.Hierarchy):
    """_mask_ref.Hierarchy with a screening field: `s` is the finest level's, (N, N, N), or None; `mask` may be None.
    rule: "restrict" (the library's) or "inject" (for the measurement of the two rules)"""

    def __init__(self, c, L, nu, sigma, eps, axes, faces, mask, s, grid_length=1.0, rule="restrict", lu=True):
        N = O.level_sizes(c, L)[-1]
        MR.Hierarchy.__init__(self, c, L, nu, sigma, eps, axes, faces, _mask(mask, N), grid_length, lu=lu and s is None)
        self.s = None
        if s is not None:
            top = np.asarray(s, dtype=np.float64).reshape(N, N, N)
            self.s = restrict_field(top, L, axes, faces) if rule == "restrict" else inject_field(top, L, axes)
            if lu:
                self.LU = coarse_lu(c, self.h * (1 << (L - 1)), self.e(0), sigma, axes, faces, self.mask[0], self.s[0])

    def sf(self, l):
        return None if self.s is None else self.s[l]

    def pinned(self):
        return pinned(self.axes, self.faces, self.sigma, self.mask[0], self.sf(0))

    def is_singular(self):
        return singular(self.axes, self.faces, self.sigma, self.mask[0], self.mask[-1], self.sf(0), self.sf(-1))

    def colour_pass(self, q, colour):
        colour_pass(self.u[q], self.d[q], self.e(q), self.level_h(q), self.sigma, self.axes, self.faces, colour, self.mask[q],
                    self.sf(q))

    def residual(self, q, r=None):
        return residual(self.u[q], self.d[q], self.e(q), self.level_h(q), self.sigma, self.axes, self.faces, self.mask[q],
                        self.sf(q), r)

    def coarse_solve(self):
        coarse_solve(self.LU, self.d[0], self.u[0], self.axes, self.faces, self.pinned(), self.mask[0], self.L == 1)

    def top_residual_field(self, x, d):
        return residual_field(x, d, self.e(-1), self.h, self.sigma, self.axes, self.faces, self.mask[-1], self.sf(-1))

    def apply(self, v):
        return -self.top_residual_field(v, np.zeros_like(v))


# ---- (weighted) conjugate gradients: _mask_ref.wpcg with the field's residual, A p and projection rule

def wpcg(prob, x0, d, rtol, atol, max_iters, dots="exact", history=None):
    """mg3d_wpcg_solve (mg3d_pcg_solve where that one accepts the context: w = 1) on a Hierarchy.  Returns (x, norms r_0 ..
    r_k, converged, rhs_mean, singular)"""
    if prob.s is None:
        return MR.wpcg(prob, x0, d, rtol, atol, max_iters, dots, history)
    N = prob.N[-1]
    blk = NR.block(N, prob.axes, prob.faces)
    w, W = WR.weights(prob)
    sing = prob.is_singular()
    x = np.array(x0, dtype=np.float64).reshape(N, N, N).copy()
    d = np.asarray(d, dtype=np.float64).reshape(N, N, N)
    for a in prob.r:
        a[...] = 0.
    r = prob.top_residual_field(x, d)
    rhs_mean = 0.
    if sing:
        rhs_mean = WR.wsum(w, d[blk], dots) / W
        r = r - WR.wsum(w, r, dots) / W
    norms = [math.sqrt(PR.dot(r, r, dots))]
    target = max(rtol * norms[0], atol)
    if norms[0] == 0. or (max_iters > 0 and norms[0] <= target):
        return x, np.array(norms), True, rhs_mean, sing
    p = None
    rz_old = None
    keep = MR._keep(prob.mask[-1], prob.axes, prob.faces)
    for k in range(max_iters):
        z = WR.precondition(prob, r)
        rz = WR.wdot(w, r, z[blk], dots)
        m = WR.wsum(w, z[blk], dots) / W if sing else 0.
        if k == 0:
            pb = z[blk] - m
        else:
            pb = (z[blk] - m) + (rz / rz_old) * p[blk]
        p = np.zeros((N, N, N))
        NR.put(p, pb, blk, prob.axes)
        q = prob.apply(p)
        pap = WR.wdot(w, p[blk], q, dots)
        if not (rz < 0. and math.isfinite(rz) and pap < 0. and math.isfinite(pap)):
            return x, np.array(norms), False, rhs_mean, sing
        alpha = rz / pap
        old = x[keep].copy()
        NR.put(x, x[blk] + alpha * p[blk], blk, prob.axes)
        x[keep] = old
        r = r - alpha * q
        rz_old = rz
        norms.append(math.sqrt(PR.dot(r, r, dots)))
        if history is not None:
            history.append(x.copy())
        if norms[-1] <= target:
            return x, np.array(norms), True, rhs_mean, sing
    return x, np.array(norms), False, rhs_mean, sing


def cycle_blk(prob, r_blk):
    """M r: one V-cycle from a zero guess, block of unknowns to block of unknowns"""
    return MR.cycle_blk(prob, r_blk)


def spread(make, x0, d, iters):
    """_mask_ref.spread on make()'s Hierarchy: two restatement runs, exactly rounded dots against numpy's pairwise sums:
    ([relative difference of the iterates x_k for k in iters], the largest relative difference of the norms)"""
    ha, hb = [], []
    _, na, _, _, _ = wpcg(make(), x0, d, 0., 1e-300, max(iters), "exact", ha)
    _, nb, _, _, _ = wpcg(make(), x0, d, 0., 1e-300, max(iters), "plain", hb)
    return ([float(np.abs(ha[k - 1] - hb[k - 1]).max() / np.abs(ha[k - 1]).max()) for k in iters],
            float((np.abs(na[1:] - nb[1:]) / na[1:]).max()))


# ---- the theta-stepper: _step_ref.rhs with the field in q (no mask form: d at a fixed point is unspecified)

def step_rhs(prob, u0, src, dt, theta, kappa):
    """d of one step on the block of unknowns; prob.sigma must be _step_ref.sigma_of(dt, theta, kappa)"""
    if prob.s is None:
        return SR.rhs(prob, u0, src, dt, theta, kappa)
    assert prob.sigma == SR.sigma_of(dt, theta, kappa)
    blk = NR.block(prob.N[-1], prob.axes, prob.faces)
    a, c1, b = SR.coefficients(dt, theta)
    u = u0[blk]
    if theta == 1.0:
        return -(a * u) if src is None else -(a * u + b * src[blk])
    q = apply(u0, prob.e(-1), prob.h, prob.sigma, prob.axes, prob.faces, None, prob.sf(-1))
    if src is None:
        return -(a * u + c1 * q)
    return -((a * u + c1 * q) + b * src[blk])


def write_rhs(prob, src, dt, theta, kappa):
    prob.d[-1][NR.block(prob.N[-1], prob.axes, prob.faces)] = step_rhs(prob, prob.u[-1], src, dt, theta, kappa)


# ---- full multigrid: _fmg_ref.fmg_solve with the field's direct solve (no mask: mg3d_fmg_solve refuses one)

def fmg_solve(prob, cycles=1):
    if prob.s is None:
        return FR.fmg_solve(prob, cycles)
    assert cycles >= 1 and not prob.fixed(0).any() and not prob.fixed().any()
    L, axes, faces = prob.L, prob.axes, prob.faces
    for l in range(L - 1, 0, -1):
        NR.restrict(prob.d[l], prob.d[l - 1], axes, faces)
        prob.u[l - 1][...] = prob.u[l][::2, ::2, ::2]
    m = FR.dirichlet_mask(prob.N[0], axes, faces)
    if L == 1:
        b = prob.d[0].copy()
        b[m] = prob.u[0][m]
        coarse_solve(prob.LU, b, prob.u[0], axes, faces, prob.pinned(), None)
        return 0.0
    prob.d[0][m] = prob.u[0][m]
    prob.coarse_solve()
    norm = 0.0
    for l in range(1, L):
        FR.interpolate(prob.u[l - 1], prob.u[l], axes, faces)
        for _ in range(cycles):
            norm = FR.vcycle(prob, l, True)
    return norm


# ---- the fields and the worked example of the tests

def random_field(N, h, seed=11):
    """uniform in [0, 1/h^2]"""
    return np.random.default_rng(seed).uniform(0.0, 1.0 / (h * h), size=(N, N, N))


def smooth_field(N, amp=50.0):
    """amp * (1 + x y + 0.5 cos 2 pi z) on [0, 1]^3: smooth, positive, its mean of order amp"""
    x = np.linspace(0.0, 1.0, N)
    return np.ascontiguousarray(amp * (1.0 + x[:, None, None] * x[None, :, None] + 0.5 * np.cos(2 * np.pi * x)[None, None, :]))


def pb_problem(N, kappa2=4.0):
    """Poisson-Boltzmann, Delta u - kappa^2 sinh u = f on [0, 1]^3 with Dirichlet faces, manufactured
    u* = sin(pi x) sin(pi y) sin(pi z) + 0.5 x: returns (u*, f)"""
    x = np.linspace(0.0, 1.0, N)
    sx = np.sin(np.pi * x)
    w = sx[:, None, None] * sx[None, :, None] * sx[None, None, :]
    u = w + 0.5 * x[:, None, None]
    f = -3.0 * np.pi ** 2 * w - kappa2 * np.sinh(u)
    return np.ascontiguousarray(u), np.ascontiguousarray(f)


def pb_newton(N, c, L, kappa2, rtol, max_newton, newton_tol, max_iters=50, dots="exact"):
    """The Newton loop of INTEGRATION.md ("Screening field") in the restatement: from u_0 = the Dirichlet values and zero
    inside, each step solves  Delta u_{k+1} - s u_{k+1} = f + kappa^2 (sinh u_k - u_k cosh u_k),  s = kappa^2 cosh u_k,  by PCG
    to rtol from u_k, until max|u_{k+1} - u_k| <= newton_tol.  Returns (u, Newton steps taken, PCG iterations per step)"""
    ustar, f = pb_problem(N, kappa2)
    u = ustar.copy()
    u[1:-1, 1:-1, 1:-1] = 0.
    its = []
    for k in range(max_newton):
        s = kappa2 * np.cosh(u)
        d = f + kappa2 * (np.sinh(u) - u * np.cosh(u))
        prob = Hierarchy(c, L, 2, 0.0, None, 0, 0, None, s)
        x, norms, _, _, _ = wpcg(prob, u, d, rtol, 0.0, max_iters, dots)
        its.append(len(norms) - 1)
        step = float(np.abs(x - u).max())
        u = x
        if step <= newton_tol:
            return u, k + 1, its
    return u, max_newton, its
