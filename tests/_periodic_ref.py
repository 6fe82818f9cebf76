"""CPU reference of periodic boundaries (mg3d_ctx_set_periodic): numpy colour pass, residual, restriction, prolongation,
duplicate refresh, coarse matrix with its pin, and the V-cycle built from them, with the library's arithmetic.

axes is a mask (1 = i, 2 = j, 4 = k).  On a periodic axis index N-1 duplicates index 0 and the unique points are 0 .. N-2;
on the other axes the faces are Dirichlet points, as in tests/_screened_ref.py.  The stencils are those of
_screened_ref.py (constant operator) and _coef_ref.py (eps) applied to a wrapped copy of the field (`ext`: on a periodic
axis the unique points with N-2 in front and 0 behind), so the sums keep the same operands in the same order.  Whatever
writes a block of unique points writes their duplicates as copies (`put`).  Test infrastructure only."""
import itertools

import numpy as np

import _coef_ref as CR
import _oracle as O
import _screened_ref as S


def per(axes, ax):
    return (axes >> ax) & 1 == 1


def ext(a, axes):
    """a with each periodic axis replaced by (N-2, 0 .. N-2, 0): its interior [1:-1] is the block of unique points"""
    N = a.shape[0]
    for ax in range(3):
        if per(axes, ax):
            a = np.concatenate([a.take([N - 2], axis=ax), a.take(np.arange(N - 1), axis=ax), a.take([0], axis=ax)], axis=ax)
    return a


def unique_block(N, axes):
    """the slices of the unique points the stencil kernels update (0 .. N-2 periodic, 1 .. N-2 otherwise)"""
    return tuple(slice(0, N - 1) if per(axes, ax) else slice(1, N - 1) for ax in range(3))


def put(a, vals, block, axes):
    """a[block] = vals, and every duplicate of a point of block (block starts at 0 on each periodic axis) the same value"""
    a[block] = vals
    N = a.shape[0]
    pa = [ax for ax in range(3) if per(axes, ax)]
    for r in range(1, len(pa) + 1):
        for sub in itertools.combinations(pa, r):
            dst = tuple(slice(N - 1, N) if ax in sub else block[ax] for ax in range(3))
            src = tuple(slice(0, 1) if ax in sub else slice(None) for ax in range(3))
            a[dst] = vals[src]


def refresh(a, axes):
    """every duplicate from its source (k_per_refresh): index N-1 of each periodic axis from index 0"""
    N = a.shape[0]
    for ax in range(3):
        if per(axes, ax):
            dst = [slice(None)] * 3
            src = [slice(None)] * 3
            dst[ax], src[ax] = N - 1, 0
            a[tuple(dst)] = a[tuple(src)]


def is_dup(N, axes):
    g = np.zeros((N, N, N), dtype=bool)
    for ax in range(3):
        if per(axes, ax):
            s = [slice(None)] * 3
            s[ax] = N - 1
            g[tuple(s)] = True
    return g


def unique_mask(N, axes):
    """the unknowns of the periodic problem: every point that is neither a duplicate nor on a Dirichlet face"""
    g = np.zeros((N, N, N), dtype=bool)
    g[unique_block(N, axes)] = True
    return g


def _colour_mask(N, axes, colour):
    blk = unique_block(N, axes)
    i, j, k = (np.arange(N)[s] for s in blk)
    return ((i[:, None, None] + j[None, :, None] + k[None, None, :]) & 1) == colour


def _sum_diag(u, e, h, sigma, axes):
    """neighbour sum and diagonal of every unique point: S._nbr_sum / CR._sum_diag on the wrapped field"""
    hSq = h * h
    X = ext(u, axes)
    if e is None:
        return S._nbr_sum(X), 6.0 + sigma * hSq, X[1:-1, 1:-1, 1:-1]
    s, dg = CR._sum_diag(X, ext(e, axes), sigma * hSq)
    return s, dg, X[1:-1, 1:-1, 1:-1]


def colour_pass(u, d, e, h, sigma, axes, colour):
    """one red-black pass in place over the unique points; colour 1 = red (i + j + k odd); duplicates follow"""
    N = u.shape[0]
    blk = unique_block(N, axes)
    hSq = h * h
    s, dg, _ = _sum_diag(u, e, h, sigma, axes)
    if e is None:
        new = (1.0 / dg) * (s - hSq * d[blk])
    else:
        new = (s - hSq * d[blk]) / dg
    vals = u[blk].copy()
    m = _colour_mask(N, axes, colour)
    vals[m] = new[m]
    put(u, vals, blk, axes)


def pre_smooth(u, d, e, h, sigma, axes, iters):
    for _ in range(iters):
        colour_pass(u, d, e, h, sigma, axes, 1)
        colour_pass(u, d, e, h, sigma, axes, 0)


def post_smooth(u, d, e, h, sigma, axes, iters):
    for _ in range(iters):
        colour_pass(u, d, e, h, sigma, axes, 0)
        colour_pass(u, d, e, h, sigma, axes, 1)


def residual_field(u, d, e, h, sigma, axes):
    """diff at every unique point (the block of unique_block)"""
    N = u.shape[0]
    invHsq = 1.0 / (h * h)
    s, dg, c = _sum_diag(u, e, h, sigma, axes)
    return d[unique_block(N, axes)] - invHsq * (s - dg * c)


def residual(u, d, e, h, sigma, axes, r=None):
    """r (optional) receives diff at the unique points and their duplicates; returns the norm over the unique points"""
    diff = residual_field(u, d, e, h, sigma, axes)
    if r is not None:
        put(r, diff, unique_block(u.shape[0], axes), axes)
    return float(np.sqrt((diff * diff).sum()))


def exact_residual_norm(u, d, e, N, h, sigma, axes):
    """sqrt of the exactly rounded sum of the squared residuals over the unique points"""
    sh = (N, N, N)
    diff = residual_field(np.asarray(u).reshape(sh), np.asarray(d).reshape(sh),
                          None if e is None else np.asarray(e).reshape(sh), h, sigma, axes)
    import math
    return math.sqrt(math.fsum((diff * diff).reshape(-1)))


def _i_blocks(N, axes, planes):
    """[a, b) blocks of `planes` unique i-planes each, and for each the i-planes its stencils read: a-1 .. b, wrapped"""
    lo = 0 if per(axes, 0) else 1
    for a in range(lo, N - 1, planes):
        b = min(a + planes, N - 1)
        yield a, b, np.arange(a - 1, b + 1) % (N - 1) if per(axes, 0) else np.arange(a - 1, b + 1)


def _ext_jk(a, axes):
    """ext on the j and k axes only: a holds a block of i-planes with their halo, the i-axis is not wrapped here"""
    for ax in (1, 2):
        if per(axes, ax):
            N = a.shape[ax]
            a = np.concatenate([a.take([N - 2], axis=ax), a.take(np.arange(N - 1), axis=ax), a.take([0], axis=ax)],
                               axis=ax)
    return a


def _block_sum_diag(u, e, h, sigma, axes, rows):
    """_sum_diag of the unique points of the i-planes rows[1:-1] (rows: those planes with their one-plane halo)"""
    X = _ext_jk(u[rows], axes)
    if e is None:
        return S._nbr_sum(X), 6.0 + sigma * h * h, X[1:-1, 1:-1, 1:-1]
    s, dg = CR._sum_diag(X, _ext_jk(e[rows], axes), sigma * h * h)
    return s, dg, X[1:-1, 1:-1, 1:-1]


def colour_pass_blocks(u, d, e, h, sigma, axes, colour, planes=16):
    """colour_pass evaluated over blocks of `planes` i-planes with a one-plane halo, for fields too large for the
    whole-array temporaries.  A pass writes points of one colour from neighbours of the other only, so the order of the
    blocks changes no value: the result is colour_pass's bit for bit."""
    N = u.shape[0]
    hSq = h * h
    _, jb, kb = unique_block(N, axes)
    j, k = np.arange(N)[jb], np.arange(N)[kb]
    for a, b, rows in _i_blocks(N, axes, planes):
        s, dg, _ = _block_sum_diag(u, e, h, sigma, axes, rows)
        blk = (slice(a, b), jb, kb)
        if e is None:
            new = (1.0 / dg) * (s - hSq * d[blk])
        else:
            new = (s - hSq * d[blk]) / dg
        vals = u[blk].copy()
        i = np.arange(a, b)
        m = ((i[:, None, None] + j[None, :, None] + k[None, None, :]) & 1) == colour
        vals[m] = new[m]
        put(u, vals, blk, axes if a == 0 else axes & 6)  # (the i-duplicates are the copies of plane 0)


def residual_blocks(u, d, e, h, sigma, axes, r=None, planes=16):
    """residual over blocks of i-planes: r (optional) receives what residual() stores there, bit for bit; returns the
    norm as exact_residual_norm computes it (the squares summed in extended precision; rounding ~ 2^-64 per term)"""
    N = u.shape[0]
    invHsq = 1.0 / (h * h)
    _, jb, kb = unique_block(N, axes)
    total = np.longdouble(0)
    for a, b, rows in _i_blocks(N, axes, planes):
        s, dg, c = _block_sum_diag(u, e, h, sigma, axes, rows)
        blk = (slice(a, b), jb, kb)
        diff = d[blk] - invHsq * (s - dg * c)
        if r is not None:
            put(r, diff, blk, axes if a == 0 else axes & 6)
        total += np.sum((diff * diff).astype(np.longdouble))
    return float(np.sqrt(total))


def _written(N, axes):
    """the points the grid transfers compute: 0 .. N-2 on a periodic axis, every index otherwise"""
    return tuple(slice(0, N - 1) if per(axes, ax) else slice(0, N) for ax in range(3))


def restrict(r, dc, axes):
    """k_restrict with a boundary word: Dirichlet faces injected, every other point fully weighted (restrict_kernel's
    order) with wrapped fine neighbours; duplicates copied"""
    Nf, Nc = r.shape[0], dc.shape[0]
    blk = _written(Nc, axes)
    idx = []
    for ax in range(3):
        I = np.arange(Nc)[blk[ax]]
        if per(axes, ax):
            idx.append([(2 * I - 1) % (Nf - 1), 2 * I, 2 * I + 1])
        else:
            idx.append([np.clip(2 * I - 1, 0, Nf - 1), 2 * I, np.clip(2 * I + 1, 0, Nf - 1)])
    val = np.zeros(tuple(len(x[0]) for x in idx))
    for ti, tj, tk in itertools.product(range(3), repeat=3):
        w = (0.25 if ti != 1 else 0.5) * (0.25 if tj != 1 else 0.5) * (0.25 if tk != 1 else 0.5)
        val = val + r[np.ix_(idx[0][ti], idx[1][tj], idx[2][tk])] * w
    face = np.zeros(val.shape, dtype=bool)
    for ax in range(3):
        if not per(axes, ax):
            s = [slice(None)] * 3
            for end in (0, -1):
                s[ax] = end
                face[tuple(s)] = True
    inj = r[np.ix_(*(2 * np.arange(Nc)[blk[ax]] for ax in range(3)))]
    val[face] = inj[face]
    put(dc, val, blk, axes)


def prolong(ec, ef, axes):
    """k_prolong with a boundary word: ef += P(ec) at every fine point that is not a duplicate (the parent order, the
    high parent wrapped on a periodic axis), duplicates copied.  Restated with the oracle's prolongation on copies whose
    duplicates are refreshed from their sources -- its parent at index Nc-1 is then the wrapped one."""
    Nc, Nf = ec.shape[0], ef.shape[0]
    c = np.ascontiguousarray(ec).copy()
    refresh(c, axes)
    f = np.ascontiguousarray(ef).copy()
    refresh(f, axes)
    cf, ff = c.reshape(-1), f.reshape(-1)
    O.lib().orc_prolong(O.P(cf), Nc, O.P(ff), Nf)
    blk = _written(Nf, axes)
    put(ef, f[blk], blk, axes)


def pinned(axes, sigma):
    return axes == 7 and sigma == 0.0


def coarse_matrix(N, h, e, sigma, axes):
    """mg3d_coarse_matrix_periodic in numpy: identity rows on Dirichlet faces, duplicates and the pin; wrapped rows"""
    if axes == 0:
        return S.coarse_matrix(N, h, sigma) if e is None else CR.coarse_matrix(N, h, e, sigma)
    n = N ** 3
    A = np.zeros((n, n))
    hSq = h * h
    invHsq = 1.0 / hSq
    idx = np.arange(n).reshape(N, N, N)
    unk = unique_mask(N, axes)
    if pinned(axes, sigma):
        unk[0, 0, 0] = False
    A[idx[~unk], idx[~unk]] = 1.0
    p = idx[unk]
    X = ext(idx, axes)
    inner = ext(unique_mask(N, axes), axes)[1:-1, 1:-1, 1:-1]
    if pinned(axes, sigma):
        inner[0, 0, 0] = False
    nb = [X[:-2, 1:-1, 1:-1], X[2:, 1:-1, 1:-1], X[1:-1, :-2, 1:-1], X[1:-1, 2:, 1:-1], X[1:-1, 1:-1, :-2],
          X[1:-1, 1:-1, 2:]]
    nb = [q[inner] for q in nb]
    if e is None:
        off = 1.0 * invHsq
        for q in nb:
            A[p, q] = off
        A[p, p] = -((6.0 + sigma * hSq) * invHsq)
    else:
        e = np.asarray(e, dtype=np.float64).reshape(N, N, N)
        ee = e.reshape(-1)
        ep = ee[p]
        a = [0.5 * (ep + ee[q]) for q in nb]
        for ai, q in zip(a, nb):
            A[p, q] = ai * invHsq
        D = a[0] + a[1]
        for ai in a[2:]:
            D = D + ai
        A[p, p] = -((D + sigma * hSq) * invHsq)
    return np.ascontiguousarray(A.reshape(-1))


def coarse_lu(N, h, e, sigma, axes):
    A = coarse_matrix(N, h, e, sigma, axes)
    O.lib().orc_lu_factor(O.P(A), N ** 3)
    return A


def coarse_solve(LU, d0, u0, axes, sigma):
    """the direct solve: b = d with 0 at the duplicates and the pin, x into u0, duplicates refreshed"""
    N = d0.shape[0]
    b = np.ascontiguousarray(d0).copy()
    b[is_dup(N, axes)] = 0.
    if pinned(axes, sigma):
        b[0, 0, 0] = 0.
    x = np.zeros(N ** 3)
    O.lib().orc_lu_solve(O.P(LU), N ** 3, O.P(b.reshape(-1)), O.P(x))
    u0[...] = x.reshape(N, N, N)
    refresh(u0, axes)


class Problem:
    """Hierarchies u, d, r ((N, N, N), level 0 coarsest) of the operator with periodic axes `axes`, sigma and eps (the
    finest level's, or None)."""

    def __init__(self, c, L, nu, sigma, eps, axes, grid_length=1.0):
        self.c, self.L, self.nu, self.sigma, self.axes = c, L, nu, sigma, axes
        self.N = O.level_sizes(c, L)
        self.h = grid_length / (self.N[-1] - 1)
        self.u = [np.zeros((n, n, n)) for n in self.N]
        self.d = [np.zeros((n, n, n)) for n in self.N]
        self.r = [np.zeros((n, n, n)) for n in self.N]
        self.eps = None
        if eps is not None:
            top = np.array(eps, dtype=np.float64).reshape((self.N[-1],) * 3)
            refresh(top, axes)  # the library keeps the sources at the duplicates
            self.eps = CR.inject(top, L)
        self.LU = coarse_lu(c, self.h * (1 << (L - 1)), None if eps is None else self.eps[0], sigma, axes)

    def e(self, l):
        return None if self.eps is None else self.eps[l]

    def level_h(self, l):
        return self.h * (1 << (self.L - 1 - l))

    def vcycle(self, q=None):
        q = self.L - 1 if q is None else q
        h = self.level_h(q)
        v, f, e = self.u[q], self.d[q], self.e(q)
        if q < self.L - 1:
            v[...] = 0.
        if q == 0:
            coarse_solve(self.LU, f, v, self.axes, self.sigma)
            return 0.
        pre_smooth(v, f, e, h, self.sigma, self.axes, self.nu)
        residual(v, f, e, h, self.sigma, self.axes, self.r[q])
        restrict(self.r[q], self.d[q - 1], self.axes)
        self.vcycle(q - 1)
        prolong(self.u[q - 1], v, self.axes)
        post_smooth(v, f, e, h, self.sigma, self.axes, self.nu)
        return residual(v, f, e, h, self.sigma, self.axes)

    def vcycles(self, count):
        return np.array([self.vcycle() for _ in range(count)])

    def flat(self, field, level):
        return np.ascontiguousarray({"u": self.u, "d": self.d, "r": self.r}[field][level].reshape(-1))


def manufactured(N, axes, sigma):
    """(u*, f) on [0, 1]^3: sin 2 pi x sin 2 pi y sin 2 pi z for mask 7; for another mask sin 2 pi on the periodic axes
    times 1 + x - x^2 on the others; f = Laplacian(u*) - sigma u* exactly (the continuous operator)"""
    x = np.linspace(0.0, 1.0, N)
    fac, lap = [], []
    for ax in range(3):
        if per(axes, ax):
            fac.append(np.sin(2 * np.pi * x))
            lap.append(-4 * np.pi ** 2 * np.sin(2 * np.pi * x))
        else:
            fac.append(1.0 + x - x * x)
            lap.append(np.full(N, -2.0))
    F = [a.reshape(sh) for a, sh in zip(fac, ((N, 1, 1), (1, N, 1), (1, 1, N)))]
    G = [a.reshape(sh) for a, sh in zip(lap, ((N, 1, 1), (1, N, 1), (1, 1, N)))]
    u = F[0] * F[1] * F[2]
    f = G[0] * F[1] * F[2] + F[0] * G[1] * F[2] + F[0] * F[1] * G[2] - sigma * u
    u, f = np.ascontiguousarray(u), np.ascontiguousarray(f)
    for a in (u, f):
        refresh(a, axes)
    return u, f
