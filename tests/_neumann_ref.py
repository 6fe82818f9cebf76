"""CPU reference of Neumann faces (mg3d_ctx_set_neumann), with or without periodic axes: numpy colour pass, residual,
restriction, prolongation, coarse matrix with its pin, the V-cycle built from them, the flux fold and the compatibility
weights, with the library's arithmetic.  Built on tests/_periodic_ref.py, whose functions these return bit for bit when
no face is a Neumann face.

axes is the mask of periodic axes (1 = i, 2 = j, 4 = k), faces the mask of Neumann faces (1 = i low, 2 = i high, 4 = j
low, 8 = j high, 16 = k low, 32 = k high; no bit on a periodic axis).  A point on a Neumann face is an unknown unless it
lies on a Dirichlet face.  The stencils are those of _screened_ref.py / _coef_ref.py applied to an extended copy of the
field (`ext`: on a periodic axis as _periodic_ref.ext; at a Neumann low face index 1 in front, at a Neumann high face
index N-2 behind), so the sums keep the same operands in the same order.  Nothing is duplicated at a Neumann face: `put`
is _periodic_ref.put.  Test infrastructure only."""
import itertools
import math

import numpy as np

import _coef_ref as CR
import _oracle as O
import _periodic_ref as PR
import _screened_ref as S

FACE_NAMES = ("ilo", "ihi", "jlo", "jhi", "klo", "khi")
per = PR.per
put = PR.put
refresh = PR.refresh
is_dup = PR.is_dup


def neu(faces, ax, hi):
    return (faces >> (2 * ax + hi)) & 1 == 1


def valid(axes, faces):
    return all(not (per(axes, ax) and (faces >> (2 * ax)) & 3) for ax in range(3))


def _ext_axis(a, axes, faces, ax):
    N = a.shape[ax]
    if per(axes, ax):
        return np.concatenate([a.take([N - 2], axis=ax), a.take(np.arange(N - 1), axis=ax), a.take([0], axis=ax)], axis=ax)
    parts = ([a.take([1], axis=ax)] if neu(faces, ax, 0) else []) + [a]
    if neu(faces, ax, 1):
        parts.append(a.take([N - 2], axis=ax))
    return np.concatenate(parts, axis=ax) if len(parts) > 1 else a


def ext(a, axes, faces):
    """a extended so that its interior [1:-1] is the block of unknowns and every stencil neighbour is in place"""
    for ax in range(3):
        a = _ext_axis(a, axes, faces, ax)
    return a


def lo_hi(N, axes, faces, ax):
    """first and last unknown index of an axis"""
    if per(axes, ax):
        return 0, N - 2
    return (0 if neu(faces, ax, 0) else 1), (N - 1 if neu(faces, ax, 1) else N - 2)


def block(N, axes, faces):
    """the slices of the unknowns the stencil kernels update"""
    return tuple(slice(lo_hi(N, axes, faces, ax)[0], lo_hi(N, axes, faces, ax)[1] + 1) for ax in range(3))


def unknown_mask(N, axes, faces):
    g = np.zeros((N, N, N), dtype=bool)
    g[block(N, axes, faces)] = True
    return g


def _colour_mask(N, axes, faces, colour, i=None):
    blk = block(N, axes, faces)
    ii, j, k = (np.arange(N)[s] for s in blk)
    if i is not None:
        ii = i
    return ((ii[:, None, None] + j[None, :, None] + k[None, None, :]) & 1) == colour


def _sum_diag_ext(X, E, h, sigma):
    hSq = h * h
    if E is None:
        return S._nbr_sum(X), 6.0 + sigma * hSq, X[1:-1, 1:-1, 1:-1]
    s, dg = CR._sum_diag(X, E, sigma * hSq)
    return s, dg, X[1:-1, 1:-1, 1:-1]


def _sum_diag(u, e, h, sigma, axes, faces):
    return _sum_diag_ext(ext(u, axes, faces), None if e is None else ext(e, axes, faces), h, sigma)


def colour_pass(u, d, e, h, sigma, axes, faces, colour):
    """one red-black pass in place over the unknowns; colour 1 = red (i + j + k odd); periodic duplicates follow"""
    N = u.shape[0]
    blk = block(N, axes, faces)
    hSq = h * h
    s, dg, _ = _sum_diag(u, e, h, sigma, axes, faces)
    if e is None:
        new = (1.0 / dg) * (s - hSq * d[blk])
    else:
        new = (s - hSq * d[blk]) / dg
    vals = u[blk].copy()
    m = _colour_mask(N, axes, faces, colour)
    vals[m] = new[m]
    put(u, vals, blk, axes)


def pre_smooth(u, d, e, h, sigma, axes, faces, iters):
    for _ in range(iters):
        colour_pass(u, d, e, h, sigma, axes, faces, 1)
        colour_pass(u, d, e, h, sigma, axes, faces, 0)


def post_smooth(u, d, e, h, sigma, axes, faces, iters):
    for _ in range(iters):
        colour_pass(u, d, e, h, sigma, axes, faces, 0)
        colour_pass(u, d, e, h, sigma, axes, faces, 1)


def residual_field(u, d, e, h, sigma, axes, faces):
    """diff at every unknown (the block of `block`)"""
    N = u.shape[0]
    invHsq = 1.0 / (h * h)
    s, dg, c = _sum_diag(u, e, h, sigma, axes, faces)
    return d[block(N, axes, faces)] - invHsq * (s - dg * c)


def residual(u, d, e, h, sigma, axes, faces, r=None):
    """r (optional) receives diff at the unknowns and the periodic duplicates; returns the norm over the unknowns"""
    diff = residual_field(u, d, e, h, sigma, axes, faces)
    if r is not None:
        put(r, diff, block(u.shape[0], axes, faces), axes)
    return float(np.sqrt((diff * diff).sum()))


def exact_residual_norm(u, d, e, N, h, sigma, axes, faces):
    """sqrt of the exactly rounded sum of the squared residuals over the unknowns"""
    sh = (N, N, N)
    diff = residual_field(np.asarray(u).reshape(sh), np.asarray(d).reshape(sh),
                          None if e is None else np.asarray(e).reshape(sh), h, sigma, axes, faces)
    return math.sqrt(math.fsum((diff * diff).reshape(-1)))


# ---- block forms: the same values from blocks of i-planes, for fields too large for whole-array temporaries

def _i_blocks(N, axes, faces, planes):
    """[a, b) blocks of `planes` unknown i-planes each, and for each the i-planes its stencils read: a-1 .. b, wrapped on
    a periodic axis, reflected at a Neumann face"""
    lo, hi = lo_hi(N, axes, faces, 0)
    for a in range(lo, hi + 1, planes):
        b = min(a + planes, hi + 1)
        rows = np.arange(a - 1, b + 1)
        if per(axes, 0):
            rows = rows % (N - 1)
        else:
            rows = np.where(rows < 0, 1, np.where(rows > N - 1, N - 2, rows))
        yield a, b, rows


def _ext_jk(a, axes, faces):
    for ax in (1, 2):
        a = _ext_axis(a, axes, faces, ax)
    return a


def _block_sum_diag(u, e, h, sigma, axes, faces, rows):
    return _sum_diag_ext(_ext_jk(u[rows], axes, faces), None if e is None else _ext_jk(e[rows], axes, faces), h, sigma)


def colour_pass_blocks(u, d, e, h, sigma, axes, faces, colour, planes=16):
    """colour_pass over blocks of i-planes with a one-plane halo: a pass writes points of one colour from neighbours of
    the other only, so the order of the blocks changes no value"""
    N = u.shape[0]
    hSq = h * h
    _, jb, kb = block(N, axes, faces)
    for a, b, rows in _i_blocks(N, axes, faces, planes):
        s, dg, _ = _block_sum_diag(u, e, h, sigma, axes, faces, rows)
        blk = (slice(a, b), jb, kb)
        if e is None:
            new = (1.0 / dg) * (s - hSq * d[blk])
        else:
            new = (s - hSq * d[blk]) / dg
        vals = u[blk].copy()
        m = _colour_mask(N, axes, faces, colour, i=np.arange(a, b))
        vals[m] = new[m]
        put(u, vals, blk, axes if a == 0 else axes & 6)


def residual_blocks(u, d, e, h, sigma, axes, faces, r=None, planes=16):
    """residual over blocks of i-planes: r (optional) receives what residual() stores, bit for bit; returns the norm as
    exact_residual_norm computes it (squares summed in extended precision)"""
    N = u.shape[0]
    invHsq = 1.0 / (h * h)
    _, jb, kb = block(N, axes, faces)
    total = np.longdouble(0)
    for a, b, rows in _i_blocks(N, axes, faces, planes):
        s, dg, c = _block_sum_diag(u, e, h, sigma, axes, faces, rows)
        blk = (slice(a, b), jb, kb)
        diff = d[blk] - invHsq * (s - dg * c)
        if r is not None:
            put(r, diff, blk, axes if a == 0 else axes & 6)
        total += np.sum((diff * diff).astype(np.longdouble))
    return float(np.sqrt(total))


# ---- transfers

def restrict(r, dc, axes, faces):
    """k_restrict with a boundary word: Dirichlet faces injected, every other point fully weighted (restrict_kernel's
    order) with wrapped or reflected fine neighbours; periodic duplicates copied"""
    Nf, Nc = r.shape[0], dc.shape[0]
    blk = PR._written(Nc, axes)
    idx = []
    for ax in range(3):
        I = np.arange(Nc)[blk[ax]]
        if per(axes, ax):
            idx.append([(2 * I - 1) % (Nf - 1), 2 * I, 2 * I + 1])
        else:
            lo, hi = 2 * I - 1, 2 * I + 1
            lo = np.where(lo < 0, 1 if neu(faces, ax, 0) else 0, lo)
            hi = np.where(hi > Nf - 1, Nf - 2 if neu(faces, ax, 1) else Nf - 1, hi)
            idx.append([lo, 2 * I, hi])
    val = np.zeros(tuple(len(x[0]) for x in idx))
    for ti, tj, tk in itertools.product(range(3), repeat=3):
        w = (0.25 if ti != 1 else 0.5) * (0.25 if tj != 1 else 0.5) * (0.25 if tk != 1 else 0.5)
        val = val + r[np.ix_(idx[0][ti], idx[1][tj], idx[2][tk])] * w
    face = np.zeros(val.shape, dtype=bool)
    for ax in range(3):
        if not per(axes, ax):
            s = [slice(None)] * 3
            for hi_, end in ((0, 0), (1, -1)):
                if not neu(faces, ax, hi_):
                    s[ax] = end
                    face[tuple(s)] = True
    inj = r[np.ix_(*(2 * np.arange(Nc)[blk[ax]] for ax in range(3)))]
    val[face] = inj[face]
    put(dc, val, blk, axes)


def prolong(ec, ef, axes, faces):
    """k_prolong with a boundary word: ef += P(ec) at every fine point that is not a duplicate.  A Neumann face needs
    nothing of its own: every parent of a fine face point lies on the same face"""
    PR.prolong(ec, ef, axes)


# ---- coarsest level

def pinned(axes, faces, sigma):
    return sigma == 0.0 and all(per(axes, ax) or (neu(faces, ax, 0) and neu(faces, ax, 1)) for ax in range(3))


def coarse_matrix(N, h, e, sigma, axes, faces):
    """mg3d_coarse_matrix_bc in numpy: identity rows on Dirichlet points, duplicates and the pin; wrapped and reflected
    rows (a reflected neighbour coincides with the one inside: its column receives both entries)"""
    if faces == 0:
        return PR.coarse_matrix(N, h, e, sigma, axes)
    n = N ** 3
    A = np.zeros((n, n))
    hSq = h * h
    invHsq = 1.0 / hSq
    idx = np.arange(n).reshape(N, N, N)
    unk = unknown_mask(N, axes, faces)
    if pinned(axes, faces, sigma):
        unk[0, 0, 0] = False
    A[idx[~unk], idx[~unk]] = 1.0
    inner = unk[block(N, axes, faces)]
    p = idx[block(N, axes, faces)][inner]
    X = ext(idx, axes, faces)
    nb = [X[:-2, 1:-1, 1:-1], X[2:, 1:-1, 1:-1], X[1:-1, :-2, 1:-1], X[1:-1, 2:, 1:-1], X[1:-1, 1:-1, :-2],
          X[1:-1, 1:-1, 2:]]
    nb = [q[inner] for q in nb]
    if e is None:
        off = 1.0 * invHsq
        for q in nb:
            A[p, q] += off  # (p is unique within one statement; a column hit twice is hit by two statements)
        A[p, p] = -((6.0 + sigma * hSq) * invHsq)
    else:
        ee = np.asarray(e, dtype=np.float64).reshape(-1)
        ep = ee[p]
        a = [0.5 * (ep + ee[q]) for q in nb]
        for ai, q in zip(a, nb):
            A[p, q] += ai * invHsq
        D = a[0] + a[1]
        for ai in a[2:]:
            D = D + ai
        A[p, p] = -((D + sigma * hSq) * invHsq)
    return np.ascontiguousarray(A.reshape(-1))


def coarse_lu(N, h, e, sigma, axes, faces):
    A = coarse_matrix(N, h, e, sigma, axes, faces)
    O.lib().orc_lu_factor(O.P(A), N ** 3)
    return A


def coarse_solve(LU, d0, u0, axes, faces, sigma):
    """the direct solve: b = d with 0 at the duplicates and the pin, x into u0, duplicates refreshed"""
    N = d0.shape[0]
    b = np.ascontiguousarray(d0).copy()
    b[is_dup(N, axes)] = 0.
    if pinned(axes, faces, sigma):
        b[0, 0, 0] = 0.
    x = np.zeros(N ** 3)
    O.lib().orc_lu_solve(O.P(LU), N ** 3, O.P(b.reshape(-1)), O.P(x))
    u0[...] = x.reshape(N, N, N)
    refresh(u0, axes)


class Problem:
    """Hierarchies u, d, r ((N, N, N), level 0 coarsest) of the operator with periodic axes `axes`, Neumann faces `faces`,
    sigma and eps (the finest level's, or None).  blocks: the stencils of levels of more than `blocks` points per side
    run in their block forms."""

    def __init__(self, c, L, nu, sigma, eps, axes, faces, grid_length=1.0, blocks=200, lu=True):
        assert valid(axes, faces)
        self.c, self.L, self.nu, self.sigma, self.axes, self.faces, self.blocks = c, L, nu, sigma, axes, faces, blocks
        self.N = O.level_sizes(c, L)
        self.h = grid_length / (self.N[-1] - 1)
        self.u = [np.zeros((n, n, n)) for n in self.N]
        self.d = [np.zeros((n, n, n)) for n in self.N]
        self.r = [np.zeros((n, n, n)) for n in self.N]
        self.eps = None
        if eps is not None:
            top = np.array(eps, dtype=np.float64).reshape((self.N[-1],) * 3)
            refresh(top, axes)
            self.eps = CR.inject(top, L)
        self.LU = None  # (lu = False: a subclass factors its own coarse matrix)
        if lu:
            self.LU = coarse_lu(c, self.h * (1 << (L - 1)), None if eps is None else self.eps[0], sigma, axes, faces)

    def e(self, l):
        return None if self.eps is None else self.eps[l]

    def level_h(self, l):
        return self.h * (1 << (self.L - 1 - l))

    def colour_pass(self, q, colour):
        fn = colour_pass_blocks if self.N[q] > self.blocks else colour_pass
        fn(self.u[q], self.d[q], self.e(q), self.level_h(q), self.sigma, self.axes, self.faces, colour)

    def residual(self, q, r=None):
        fn = residual_blocks if self.N[q] > self.blocks else residual
        return fn(self.u[q], self.d[q], self.e(q), self.level_h(q), self.sigma, self.axes, self.faces, r)

    def vcycle(self, q=None):
        q = self.L - 1 if q is None else q
        v, f = self.u[q], self.d[q]
        if q < self.L - 1:
            v[...] = 0.
        if q == 0:
            coarse_solve(self.LU, f, v, self.axes, self.faces, self.sigma)
            return 0.
        for _ in range(self.nu):
            self.colour_pass(q, 1)
            self.colour_pass(q, 0)
        self.residual(q, self.r[q])
        restrict(self.r[q], self.d[q - 1], self.axes, self.faces)
        self.vcycle(q - 1)
        prolong(self.u[q - 1], v, self.axes, self.faces)
        for _ in range(self.nu):
            self.colour_pass(q, 0)
            self.colour_pass(q, 1)
        return self.residual(q)

    def vcycles(self, count):
        return np.array([self.vcycle() for _ in range(count)])

    def flat(self, field, level):
        return np.ascontiguousarray({"u": self.u, "d": self.d, "r": self.r}[field][level].reshape(-1))


# ---- what the binding offers on the host

def weights(N, axes, faces):
    """the left null vector of the reflected operator: 1/2 per Neumann face a point lies on, 0 at Dirichlet points and
    periodic duplicates, 1 at the other unknowns (Solver.compatibility_weights)"""
    w = np.ones((N, N, N))
    for ax in range(3):
        for hi_, end in ((0, 0), (1, N - 1)):
            s = [slice(None)] * 3
            s[ax] = end
            if per(axes, ax):
                if hi_:
                    w[tuple(s)] = 0.
            else:
                w[tuple(s)] *= 0.5 if neu(faces, ax, hi_) else 0.
    return w


def fold_flux(d, e, h, faces, flux):
    """mg3d_neumann_fold_flux: d -= 2 a g / h on each Neumann face, a = 1 or the mean of eps at the face point and the
    point inside; flux maps a face number 0..5 to its (N, N) array"""
    N = d.shape[0]
    for f, g in sorted(flux.items()):
        if not (faces >> f) & 1:
            continue
        ax, hi_ = f // 2, f & 1
        s, t = [slice(None)] * 3, [slice(None)] * 3
        s[ax], t[ax] = (N - 1, N - 2) if hi_ else (0, 1)
        s, t = tuple(s), tuple(t)
        a = 1.0 if e is None else 0.5 * (e[s] + e[t])
        d[s] = d[s] - 2.0 * a * g / h
    return d


def axis_factors(N, axes, faces, ax):
    """factor of the manufactured solution along an axis, its first and second derivative: sin 2 pi x on a periodic axis,
    cos 2 pi x between two Neumann faces, a quarter wave with zero slope at the one Neumann face, 1 + x - x^2 otherwise"""
    x = np.linspace(0.0, 1.0, N)
    if per(axes, ax):
        w = 2 * np.pi
        return np.sin(w * x), w * np.cos(w * x), -w * w * np.sin(w * x)
    lo, hi = neu(faces, ax, 0), neu(faces, ax, 1)
    if lo and hi:
        w = 2 * np.pi
        return np.cos(w * x), -w * np.sin(w * x), -w * w * np.cos(w * x)
    w = 0.5 * np.pi
    if lo:
        return np.cos(w * x) + 1.0, -w * np.sin(w * x), -w * w * np.cos(w * x)
    if hi:
        return np.sin(w * x) + 1.0, w * np.cos(w * x), -w * w * np.sin(w * x)
    return 1.0 + x - x * x, 1.0 - 2.0 * x, np.full(N, -2.0)


def _outer(a, b, c):
    N = a.shape[0]
    return a.reshape(N, 1, 1) * b.reshape(1, N, 1) * c.reshape(1, 1, N)


def manufactured(N, axes, faces, sigma, eps=None, grad_eps=None):
    """(u*, f) on [0, 1]^3 with homogeneous flux on the Neumann faces: the product of axis_factors;
    f = div(eps grad u*) - sigma u* exactly (the continuous operator; eps = 1 when None, else eps and its gradient, three
    (N, N, N) arrays, are given)"""
    F = [axis_factors(N, axes, faces, ax) for ax in range(3)]
    u = _outer(F[0][0], F[1][0], F[2][0])
    lap = _outer(F[0][2], F[1][0], F[2][0]) + _outer(F[0][0], F[1][2], F[2][0]) + _outer(F[0][0], F[1][0], F[2][2])
    if eps is None:
        f = lap - sigma * u
    else:
        gu = [_outer(F[0][1], F[1][0], F[2][0]), _outer(F[0][0], F[1][1], F[2][0]), _outer(F[0][0], F[1][0], F[2][1])]
        f = eps * lap + grad_eps[0] * gu[0] + grad_eps[1] * gu[1] + grad_eps[2] * gu[2] - sigma * u
    u, f = np.ascontiguousarray(u), np.ascontiguousarray(f)
    for a in (u, f):
        refresh(a, axes)
    return u, f


def cos_eps(N):
    """a smooth coefficient that is even about every face (so reflection keeps second order) and periodic:
    eps = 1 + 0.3 cos 2 pi x cos 2 pi y cos 2 pi z, and its gradient"""
    x = np.linspace(0.0, 1.0, N)
    w = 2 * np.pi
    c, s = np.cos(w * x), -w * np.sin(w * x)
    eps = 1.0 + 0.3 * _outer(c, c, c)
    return np.ascontiguousarray(eps), [0.3 * _outer(s, c, c), 0.3 * _outer(c, s, c), 0.3 * _outer(c, c, s)]
