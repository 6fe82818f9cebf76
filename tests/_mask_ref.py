"""CPU reference of fixed points inside the domain (mg3d_ctx_set_mask): numpy colour pass with skip, residual with zeros,
masked prolongation, mask injection, coarse matrix with identity rows, the pin rule, the V-cycle built from them and the
(weighted) PCG over it, with the library's arithmetic.  Built on tests/_neumann_ref.py by import: with an all-zero mask
every function returns what that module returns, bit for bit.

A mask is an (N, N, N) array of bytes, nonzero = fixed.  Only its FIXED UNKNOWNS matter (`fixed`): nonzero bytes on points
that are neither periodic duplicates nor on a Dirichlet face.  A fixed unknown is a Dirichlet point: the colour pass and
the prolongation skip it, the residual is 0. there, its neighbours read it through the ordinary stencil.  Stated here as
"run the unmasked operator, put the old values back": a colour pass reads the other colour only and the prolongation
reads the coarse level only, so skipping a point and restoring it are the same thing.  Test infrastructure only."""
import math

import numpy as np

import _neumann_ref as NR
import _oracle as O
import _pcg_ref as PR
import _periodic_ref as PER
import _step_ref as SR
import _wpcg_ref as WR


def inject(mask, L):
    """the masks of levels 0 .. L-1 from the finest one: m_{l-1}[I,J,K] = m_l[2I,2J,2K]"""
    out = [np.ascontiguousarray(mask)]
    for _ in range(L - 1):
        out.insert(0, np.ascontiguousarray(out[0][::2, ::2, ::2]))
    return out


def stored(mask, axes):
    """the bytes a level keeps: the caller's, periodic duplicates taking their sources' (mg3d_ctx_get_mask)"""
    m = np.array(mask, dtype=np.uint8).copy()
    PER.refresh(m, axes)
    return m


def fixed(mask, axes, faces):
    """the fixed unknowns, (N, N, N) bool"""
    N = mask.shape[0]
    return (np.asarray(mask) != 0) & NR.unknown_mask(N, axes, faces)


def _keep(mask, axes, faces):
    """fixed unknowns and their periodic duplicates: the points whose values are put back"""
    f = fixed(mask, axes, faces)
    PER.refresh(f, axes)
    return f


def colour_pass(u, d, e, h, sigma, axes, faces, colour, mask):
    keep = _keep(mask, axes, faces)
    old = u[keep].copy()
    NR.colour_pass(u, d, e, h, sigma, axes, faces, colour)
    u[keep] = old


def pre_smooth(u, d, e, h, sigma, axes, faces, iters, mask):
    for _ in range(iters):
        colour_pass(u, d, e, h, sigma, axes, faces, 1, mask)
        colour_pass(u, d, e, h, sigma, axes, faces, 0, mask)


def post_smooth(u, d, e, h, sigma, axes, faces, iters, mask):
    for _ in range(iters):
        colour_pass(u, d, e, h, sigma, axes, faces, 0, mask)
        colour_pass(u, d, e, h, sigma, axes, faces, 1, mask)


def residual_field(u, d, e, h, sigma, axes, faces, mask):
    """diff on the block of unknowns, 0. at the fixed ones (whatever d holds there)"""
    N = u.shape[0]
    with np.errstate(all="ignore"):
        diff = NR.residual_field(u, d, e, h, sigma, axes, faces)
    diff[fixed(mask, axes, faces)[NR.block(N, axes, faces)]] = 0.
    return diff


def residual(u, d, e, h, sigma, axes, faces, mask, r=None):
    diff = residual_field(u, d, e, h, sigma, axes, faces, mask)
    if r is not None:
        NR.put(r, diff, NR.block(u.shape[0], axes, faces), axes)
    return float(np.sqrt((diff * diff).sum()))


def exact_residual_norm(u, d, e, h, sigma, axes, faces, mask):
    diff = residual_field(u, d, e, h, sigma, axes, faces, mask)
    return math.sqrt(math.fsum((diff * diff).reshape(-1)))


def prolong(ec, ef, axes, faces, mask_f):
    keep = _keep(mask_f, axes, faces)
    old = ef[keep].copy()
    NR.prolong(ec, ef, axes, faces)
    ef[keep] = old


# ---- block forms, for levels too large for whole-array temporaries (_neumann_ref's block forms with the mask)

def colour_pass_blocks(u, d, e, h, sigma, axes, faces, colour, mask, planes=16):
    keep = _keep(mask, axes, faces)
    old = u[keep].copy()
    NR.colour_pass_blocks(u, d, e, h, sigma, axes, faces, colour, planes)
    u[keep] = old


def residual_blocks(u, d, e, h, sigma, axes, faces, mask, r=None, planes=16):
    """residual over blocks of i-planes: r (optional) receives what residual() stores, bit for bit; returns the norm over
    the free unknowns, squares summed in extended precision"""
    N = u.shape[0]
    invHsq = 1.0 / (h * h)
    _, jb, kb = NR.block(N, axes, faces)
    fx = fixed(mask, axes, faces)
    total = np.longdouble(0)
    for a, b, rows in NR._i_blocks(N, axes, faces, planes):
        s, dg, c = NR._block_sum_diag(u, e, h, sigma, axes, faces, rows)
        blk = (slice(a, b), jb, kb)
        with np.errstate(all="ignore"):
            diff = d[blk] - invHsq * (s - dg * c)
        diff[fx[blk]] = 0.
        if r is not None:
            NR.put(r, diff, blk, axes if a == 0 else axes & 6)
        total += np.sum((diff * diff).astype(np.longdouble))
    return float(np.sqrt(total))


def pinned(axes, faces, sigma, mask0):
    """the pin of unknown (0,0,0) of level 0: the old condition, and no fixed unknown on level 0"""
    return NR.pinned(axes, faces, sigma) and not fixed(mask0, axes, faces).any()


def singular(axes, faces, sigma, mask0, mask_top):
    """mg3d_wpcg_solve projects: pinned, and no fixed unknown on the finest level either"""
    return pinned(axes, faces, sigma, mask0) and not fixed(mask_top, axes, faces).any()


def coarse_matrix(N, h, e, sigma, axes, faces, mask):
    """mg3d_coarse_matrix_mask in numpy: mg3d_coarse_matrix_bc without a fixed unknown; otherwise its rows for any axes
    and faces with identity rows at the fixed unknowns as well, and no pin"""
    fx = None if mask is None else fixed(np.asarray(mask).reshape(N, N, N), axes, faces)
    if fx is None or not fx.any():
        return NR.coarse_matrix(N, h, e, sigma, axes, faces)
    n = N ** 3
    A = np.zeros((n, n))
    hSq = h * h
    invHsq = 1.0 / hSq
    idx = np.arange(n).reshape(N, N, N)
    unk = NR.unknown_mask(N, axes, faces) & ~fx
    A[idx[~unk], idx[~unk]] = 1.0
    blk = NR.block(N, axes, faces)
    inner = unk[blk]
    p = idx[blk][inner]
    X = NR.ext(idx, axes, faces)
    nb = [X[:-2, 1:-1, 1:-1], X[2:, 1:-1, 1:-1], X[1:-1, :-2, 1:-1], X[1:-1, 2:, 1:-1], X[1:-1, 1:-1, :-2],
          X[1:-1, 1:-1, 2:]]
    nb = [q[inner] for q in nb]
    if e is None:
        off = 1.0 * invHsq
        for q in nb:
            A[p, q] += off
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


def coarse_lu(N, h, e, sigma, axes, faces, mask):
    A = coarse_matrix(N, h, e, sigma, axes, faces, mask)
    O.lib().orc_lu_factor(O.P(A), N ** 3)
    return A


def coarse_solve(LU, d0, u0, axes, faces, sigma, mask0, one_level=False):
    """the direct solve: b = d with 0 at the duplicates, the pin and the fixed unknowns (a one-level hierarchy: u's own
    values at the fixed unknowns), x into u0, duplicates refreshed"""
    N = d0.shape[0]
    b = np.ascontiguousarray(d0).copy()
    fx = fixed(mask0, axes, faces)
    b[fx] = u0[fx] if one_level else 0.
    b[NR.is_dup(N, axes)] = 0.
    if pinned(axes, faces, sigma, mask0):
        b[0, 0, 0] = 0.
    x = np.zeros(N ** 3)
    O.lib().orc_lu_solve(O.P(LU), N ** 3, O.P(b.reshape(-1)), O.P(x))
    u0[...] = x.reshape(N, N, N)
    NR.refresh(u0, axes)


class Hierarchy(NR.Problem):
    """_neumann_ref.Problem with fixed points: `mask` is the finest level's, (N, N, N) bytes or bool"""

    def __init__(self, c, L, nu, sigma, eps, axes, faces, mask, grid_length=1.0, lu=True):
        NR.Problem.__init__(self, c, L, nu, sigma, eps, axes, faces, grid_length, lu=False)
        top = stored(np.asarray(mask).reshape((self.N[-1],) * 3), axes)
        self.mask = inject(top, L)
        if lu:
            self.LU = coarse_lu(c, self.h * (1 << (L - 1)), self.e(0), sigma, axes, faces, self.mask[0])

    def fixed(self, l=-1):
        return fixed(self.mask[l], self.axes, self.faces)

    def colour_pass(self, q, colour):
        colour_pass(self.u[q], self.d[q], self.e(q), self.level_h(q), self.sigma, self.axes, self.faces, colour, self.mask[q])

    def residual(self, q, r=None):
        return residual(self.u[q], self.d[q], self.e(q), self.level_h(q), self.sigma, self.axes, self.faces, self.mask[q], r)

    def prolong(self, q):
        prolong(self.u[q - 1], self.u[q], self.axes, self.faces, self.mask[q])

    def coarse_solve(self):
        coarse_solve(self.LU, self.d[0], self.u[0], self.axes, self.faces, self.sigma, self.mask[0], self.L == 1)

    def vcycle(self, q=None):
        q = self.L - 1 if q is None else q
        v = self.u[q]
        if q < self.L - 1:
            v[...] = 0.
        if q == 0:
            self.coarse_solve()
            return 0.
        for _ in range(self.nu):
            self.colour_pass(q, 1)
            self.colour_pass(q, 0)
        self.residual(q, self.r[q])
        NR.restrict(self.r[q], self.d[q - 1], self.axes, self.faces)
        self.vcycle(q - 1)
        self.prolong(q)
        for _ in range(self.nu):
            self.colour_pass(q, 0)
            self.colour_pass(q, 1)
        return self.residual(q)


# ---- (weighted) conjugate gradients over the masked cycle: _wpcg_ref.wpcg with the masked residual and projection rule

def top_residual_field(prob, x, d):
    return residual_field(x, d, WR._top_eps(prob), prob.h, prob.sigma, prob.axes, prob.faces, prob.mask[-1])


def apply(prob, v):
    """A v at the unknowns, 0. at the fixed ones"""
    return -top_residual_field(prob, v, np.zeros_like(v))


def is_singular(prob):
    return singular(prob.axes, prob.faces, prob.sigma, prob.mask[0], prob.mask[-1])


def wpcg(prob, x0, d, rtol, atol, max_iters, dots="exact", history=None):
    """mg3d_wpcg_solve (mg3d_pcg_solve where that one accepts the context: w = 1) on a Hierarchy.  Returns (x, norms r_0 ..
    r_k, converged, rhs_mean, singular).  z, r, p, q are 0. at the fixed unknowns, so x is never moved there."""
    N = prob.N[-1]
    blk = NR.block(N, prob.axes, prob.faces)
    w, W = WR.weights(prob)
    sing = is_singular(prob)
    x = np.array(x0, dtype=np.float64).reshape(N, N, N).copy()
    d = np.asarray(d, dtype=np.float64).reshape(N, N, N)
    for a in prob.r:
        a[...] = 0.
    r = top_residual_field(prob, x, d)
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
        q = apply(prob, p)
        pap = WR.wdot(w, p[blk], q, dots)
        if not (rz < 0. and math.isfinite(rz) and pap < 0. and math.isfinite(pap)):
            return x, np.array(norms), False, rhs_mean, sing
        alpha = rz / pap
        keep = _keep(prob.mask[-1], prob.axes, prob.faces)
        old = x[keep].copy()
        NR.put(x, x[blk] + alpha * p[blk], blk, prob.axes)
        x[keep] = old  # (x + alpha*0. is x, except that it turns a -0. into +0.)
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
    for a in prob.r:
        a[...] = 0.
    return WR.precondition(prob, r_blk)[NR.block(prob.N[-1], prob.axes, prob.faces)]


# ---- the theta-stepper over the masked hierarchy (_step_ref.advance with the masked solvers)

def advance(prob, nsteps, cycles, s, dt, theta, kappa, method="vcycles", rtol=1e-8):
    norms, iters, conv = [], 0, True
    for _ in range(nsteps):
        SR.write_rhs(prob, s, dt, theta, kappa)  # (d at fixed points: unspecified, never read)
        if method == "vcycles":
            norms.append(prob.vcycles(cycles)[-1])
        else:
            d = prob.d[-1].copy()
            x, nn, ok, _, _ = wpcg(prob, prob.u[-1].copy(), d, rtol, 0.0, cycles)
            prob.u[-1][...] = x
            prob.d[-1][...] = d
            norms.append(nn[-1])
            iters += len(nn) - 1
            conv = conv and ok
    return np.array(norms), iters, (conv if method == "wpcg" else False)


# ---- bodies and the two discrete-exact problems of the tests

def sphere(N, radius=0.2):
    x = np.linspace(0.0, 1.0, N)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    return ((X - 0.5) ** 2 + (Y - 0.5) ** 2 + (Z - 0.5) ** 2 <= radius * radius).astype(np.uint8)


def plate(N, plane, margin=None):
    """a one-point-thick plate on i = plane, `margin` points short of the faces in j and k (default N // 4)"""
    g = N // 4 if margin is None else margin
    m = np.zeros((N, N, N), dtype=np.uint8)
    m[plane, g:N - g, g:N - g] = 1
    return m


def needle(N):
    """a one-point-thick needle on odd j, k indices, along i over the middle half"""
    m = np.zeros((N, N, N), dtype=np.uint8)
    c = (N // 2) | 1
    m[N // 4:N - N // 4, c, c] = 1
    return m


def random_mask(N, density=0.1, seed=3):
    return (np.random.default_rng(seed).uniform(size=(N, N, N)) < density).astype(np.uint8)


def gpu_test_mask(N, seed=3):
    """the mask of the GPU tests: random at 10 % density, a solid block and a one-point-thick odd plate"""
    m = random_mask(N, 0.1, seed)
    a = N // 4
    m[a:a + 3, a:a + 4, a:a + 4] = 1
    m[(N // 2) | 1, 2:N - 2, 2:N - 2] = 1
    return m


def exact_problem(which, N=17):
    """i Dirichlet with u(i=0) = u(i=N-1) = 0, j and k periodic, d = 0.  "a": planes i >= 12 fixed at 1, exact u = i/12 on
    i <= 12.  "b": only plane i = 11 fixed at 1 (gone from both coarse levels), exact u = i/11 below it and (16 - i)/5
    above.  Returns (axes, faces, mask, u0 with the fixed values and a zero guess, exact u)."""
    assert N == 17
    i = np.arange(N, dtype=np.float64)[:, None, None] * np.ones((N, N, N))
    mask = np.zeros((N, N, N), dtype=np.uint8)
    if which == "a":
        mask[12:] = 1
        exact = np.where(i <= 12, i / 12.0, 1.0)
        exact[N - 1] = 0.
    else:
        mask[11] = 1
        exact = np.where(i <= 11, i / 11.0, (16.0 - i) / 5.0)
    u0 = np.zeros((N, N, N))
    u0[mask != 0] = 1.0
    u0[0] = 0.
    u0[N - 1] = 0.
    return 6, 0, mask, u0, exact


def spread(make, x0, d, iters):
    """two restatement runs of max(iters) iterations from x0 with right-hand side d on make()'s Hierarchy, exactly rounded
    dots against numpy's pairwise float64 sums: ([relative difference of the iterates x_k, max|a - b| / max|a|, for k in
    iters], the largest relative difference of the norms r_1 .. r_max)"""
    ha, hb = [], []
    _, na, _, _, _ = wpcg(make(), x0, d, 0., 1e-300, max(iters), "exact", ha)
    _, nb, _, _, _ = wpcg(make(), x0, d, 0., 1e-300, max(iters), "plain", hb)
    return ([float(np.abs(ha[k - 1] - hb[k - 1]).max() / np.abs(ha[k - 1]).max()) for k in iters],
            float((np.abs(na[1:] - nb[1:]) / na[1:]).max()))


def summation_spread(iters=(1, 2, 5)):
    """What a summation order is worth on the masked solver problems of tests/test_gpu_mask.py, measured as
    _pcg_ref.summation_spread does (`spread`), from the tests' own start; per problem the relative difference of the
    iterates x_k and the largest relative difference of the norms r_1 .. r_5"""
    cases = {}
    for which in ("a", "b"):
        axes, faces, mask, u0, _ = exact_problem(which)
        cases["exact " + which] = (lambda axes=axes, faces=faces, mask=mask: Hierarchy(5, 3, 2, 0.0, None, axes, faces, mask), u0)
    ball = sphere(33)
    u0 = np.zeros((33, 33, 33))
    u0[ball != 0] = 1.0
    cases["sphere 33"] = (lambda: Hierarchy(5, 4, 2, 0.0, None, 0, 0, ball), u0)
    return {name: spread(make, x0, np.zeros_like(x0), iters) for name, (make, x0) in cases.items()}


if __name__ == "__main__":
    for name, (u, n) in summation_spread().items():
        print(f"{name:10s} u, k = 1, 2, 5: " + " ".join(f"{v:.2e}" for v in u) + f"   norms: {n:.2e}")
