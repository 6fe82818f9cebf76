"""CPU reference of the screened operator  Delta_h u - sigma u = d  (mg3d_ctx_set_shift): a numpy colour pass and
residual with the library's arithmetic per level of spacing h,

    hSq = h*h;  dg = 6 + sigma*hSq;  sixth = 1./dg;  invHsq = 1./hSq
    smoother : v = sixth * ((((((up + dn) + jm) + jp) + km) + kp) - hSq*d)
    residual : diff = d - invHsq * (sum - dg*v)

composed with the oracle's restriction, prolongation and LU factor / solve into the V-cycle of orc_vcycle and the FMG start
of orc_fmg_initialize.  Each expression keeps the reference's association, so with float64 ufuncs (no fusion) every value
is the one the oracle computes at sigma = 0 and the one the GPU computes at any sigma.  Test infrastructure only."""
import numpy as np

import _oracle as O


def level_op(h, sigma):
    hSq = h * h
    dg = 6.0 + sigma * hSq
    return hSq, 1.0 / dg, 1.0 / hSq, dg


def _nbr_sum(u):
    s = u[:-2, 1:-1, 1:-1] + u[2:, 1:-1, 1:-1]
    s = s + u[1:-1, :-2, 1:-1]
    s = s + u[1:-1, 2:, 1:-1]
    s = s + u[1:-1, 1:-1, :-2]
    s = s + u[1:-1, 1:-1, 2:]
    return s


_masks = {}


def _mask(N, colour):
    key = (N, colour)
    if key not in _masks:
        i = np.arange(1, N - 1)
        _masks[key] = ((i[:, None, None] + i[None, :, None] + i[None, None, :]) & 1) == colour
    return _masks[key]


def colour_pass(u, d, h, sigma, colour):
    """mg_3d.h:438-443 with the screened diagonal; u, d: (N, N, N).  colour 1 = red (i + j + k odd), updated in place."""
    N = u.shape[0]
    if N < 3:
        return
    hSq, sixth, _, _ = level_op(h, sigma)
    s = _nbr_sum(u)
    s = s - hSq * d[1:-1, 1:-1, 1:-1]
    new = sixth * s
    m = _mask(N, colour)
    u[1:-1, 1:-1, 1:-1][m] = new[m]


def pre_smooth(u, d, h, sigma, iters):
    for _ in range(iters):
        colour_pass(u, d, h, sigma, 1)
        colour_pass(u, d, h, sigma, 0)


def post_smooth(u, d, h, sigma, iters):
    for _ in range(iters):
        colour_pass(u, d, h, sigma, 0)
        colour_pass(u, d, h, sigma, 1)


def residual_field(u, d, h, sigma):
    """diff on the interior, (N-2)^3 (mg_3d.h:819-821 with dg)."""
    _, _, invHsq, dg = level_op(h, sigma)
    s = _nbr_sum(u)
    s = s - dg * u[1:-1, 1:-1, 1:-1]
    return d[1:-1, 1:-1, 1:-1] - invHsq * s


def residual(u, d, h, sigma, r=None):
    """r (optional) written on the interior only (mg_3d.h:824-825); returns the norm (pairwise sum of the squares)."""
    diff = residual_field(u, d, h, sigma)
    if r is not None:
        r[1:-1, 1:-1, 1:-1] = diff
    return float(np.sqrt((diff * diff).sum()))


def exact_residual_norm(u, d, N, h, sigma):
    """twin of _oracle.exact_residual_norm for the screened operator: sqrt of the exactly rounded sum of the squares."""
    diff = residual_field(np.ascontiguousarray(u).reshape(N, N, N), np.ascontiguousarray(d).reshape(N, N, N), h, sigma)
    sq = (diff * diff).reshape(-1)
    total = np.longdouble(0)
    step = 1 << 24
    for a in range(0, sq.size, step):
        total += np.sum(sq[a:a + step].astype(np.longdouble))
    return float(np.sqrt(total))


def coarse_matrix(N, h, sigma):
    """orc_coarse_matrix with the interior diagonal overwritten by -(dg*invHsq)."""
    n = N ** 3
    A = np.zeros(n * n)
    O.lib().orc_coarse_matrix(O.P(A), N, h)
    A = A.reshape(n, n)
    _, _, invHsq, dg = level_op(h, sigma)
    i = np.arange(N)
    inner = ((i[:, None, None] > 0) & (i[:, None, None] < N - 1) & (i[None, :, None] > 0) & (i[None, :, None] < N - 1)
             & (i[None, None, :] > 0) & (i[None, None, :] < N - 1)).reshape(-1)
    p = np.nonzero(inner)[0]
    A[p, p] = -(dg * invHsq)
    return np.ascontiguousarray(A.reshape(-1))


def coarse_lu(N, h, sigma):
    A = coarse_matrix(N, h, sigma)
    (O.lib().orc_lu_factor_banded if N > 9 else O.lib().orc_lu_factor)(O.P(A), N ** 3)
    return A


class Problem:
    """Hierarchies u, d, r ((N, N, N) arrays, level 0 coarsest) with the screened operator of `sigma`."""

    def __init__(self, c, L, nu, sigma, grid_length=1.0):
        self.c, self.L, self.nu, self.sigma = c, L, nu, sigma
        self.N = O.level_sizes(c, L)
        self.h = grid_length / (self.N[-1] - 1)
        self.u = [np.zeros((n, n, n)) for n in self.N]
        self.d = [np.zeros((n, n, n)) for n in self.N]
        self.r = [np.zeros((n, n, n)) for n in self.N]
        self.LU = coarse_lu(c, self.h * (1 << (L - 1)), sigma)

    def set_shift(self, sigma):
        self.sigma = sigma
        self.LU = coarse_lu(self.c, self.h * (1 << (self.L - 1)), sigma)

    def setup_test_problem(self):
        """test_mg_3d.c:11-29: BC values on the faces of d and of u of the finest level, interior zero."""
        N = self.N[-1]
        for a in (self.d[-1], self.u[-1]):
            a[...] = 0.
            O.lib().orc_fill_boundary(O.P(a.reshape(-1)), N, self.h)

    def vcycle(self, q=None, h=None):
        """orc_vcycle with the screened operator; returns the post-smoothing residual norm of level q."""
        q = self.L - 1 if q is None else q
        h = self.h if h is None else h
        v, f = self.u[q], self.d[q]
        if q < self.L - 1:
            v[...] = 0.
        if q == 0:
            x = np.zeros(v.size)
            O.lib().orc_lu_solve(O.P(self.LU), v.size, O.P(np.ascontiguousarray(f.reshape(-1))), O.P(x))
            v[...] = x.reshape(v.shape)
            return 0.
        N, Nc = self.N[q], self.N[q - 1]
        pre_smooth(v, f, h, self.sigma, self.nu)
        residual(v, f, h, self.sigma, self.r[q])
        dc = np.zeros(Nc ** 3)
        O.lib().orc_restrict(O.P(self.r[q].reshape(-1)), N, O.P(dc), Nc)
        self.d[q - 1][...] = dc.reshape(Nc, Nc, Nc)
        self.vcycle(q - 1, 2 * h)
        vf = np.ascontiguousarray(v.reshape(-1))
        O.lib().orc_prolong(O.P(np.ascontiguousarray(self.u[q - 1].reshape(-1))), Nc, O.P(vf), N)
        v[...] = vf.reshape(v.shape)
        post_smooth(v, f, h, self.sigma, self.nu)
        return residual(v, f, h, self.sigma)

    def vcycles(self, count):
        return np.array([self.vcycle() for _ in range(count)])

    def fmg_initialize(self, grid_length=1.0):
        """orc_fmg_initialize (mg_dirichlet_analytic.c:771-806) with the screened operator."""
        N = self.c
        h = grid_length / (self.c - 1)
        u0 = self.u[0].reshape(-1)
        O.lib().orc_fill_boundary(O.P(u0), N, h)
        x = np.zeros(u0.size)
        O.lib().orc_lu_solve(O.P(self.LU), u0.size, O.P(np.ascontiguousarray(self.d[0].reshape(-1))), O.P(x))
        self.u[0][...] = x.reshape(self.u[0].shape)
        for l in range(1, self.L):
            Nc, N, h = N, 2 * N - 1, h * 0.5
            uf = np.ascontiguousarray(self.u[l].reshape(-1))
            O.lib().orc_prolong(O.P(np.ascontiguousarray(self.u[l - 1].reshape(-1))), Nc, O.P(uf), N)
            O.lib().orc_fill_boundary(O.P(uf), N, h)
            self.u[l][...] = uf.reshape(self.u[l].shape)
            self.u[l - 1][...] = 0.
            self.vcycle(l, h)

    def flat(self, field, level):
        return np.ascontiguousarray({"u": self.u, "d": self.d, "r": self.r}[field][level].reshape(-1))
