"""CPU reference of the variable-coefficient operator  div(eps grad u) - sigma u = d  (mg3d_ctx_set_coefficient): a numpy
colour pass and residual with the library's arithmetic per level of spacing h,

    a_im = 0.5*(e[p] + e[p-NN]) ... a_kp = 0.5*(e[p] + e[p+1])
    s    = (((((a_im*v[p-NN] + a_ip*v[p+NN]) + a_jm*v[p-N]) + a_jp*v[p+N]) + a_km*v[p-1]) + a_kp*v[p+1])
    D    = ((((a_im + a_ip) + a_jm) + a_jp) + a_km) + a_kp;   dg = D + sigma*hSq
    smoother : v = (s - hSq*d) / dg
    residual : diff = d - invHsq*(s - dg*v)

with eps of a coarser level injected (e_{l-1}[I,J,K] = e_l[2I,2J,2K]), composed with the oracle's restriction, prolongation
and LU factor / solve into the V-cycle of orc_vcycle and the FMG start of orc_fmg_initialize (the structure of
tests/_screened_ref.py).  float64 ufuncs do not fuse, so every value is the one the GPU computes.  Test infrastructure only."""
import numpy as np

import _oracle as O
import _screened_ref as S


def faces(e):
    """the six face means of every interior point, in the order i-, i+, j-, j+, k-, k+"""
    c = e[1:-1, 1:-1, 1:-1]
    return (0.5 * (c + e[:-2, 1:-1, 1:-1]), 0.5 * (c + e[2:, 1:-1, 1:-1]),
            0.5 * (c + e[1:-1, :-2, 1:-1]), 0.5 * (c + e[1:-1, 2:, 1:-1]),
            0.5 * (c + e[1:-1, 1:-1, :-2]), 0.5 * (c + e[1:-1, 1:-1, 2:]))


def _sum_diag(u, e, shift):
    a_im, a_ip, a_jm, a_jp, a_km, a_kp = faces(e)
    s = a_im * u[:-2, 1:-1, 1:-1] + a_ip * u[2:, 1:-1, 1:-1]
    s = s + a_jm * u[1:-1, :-2, 1:-1]
    s = s + a_jp * u[1:-1, 2:, 1:-1]
    s = s + a_km * u[1:-1, 1:-1, :-2]
    s = s + a_kp * u[1:-1, 1:-1, 2:]
    D = a_im + a_ip
    D = D + a_jm
    D = D + a_jp
    D = D + a_km
    D = D + a_kp
    return s, D + shift


def colour_pass(u, d, e, h, sigma, colour):
    """one red-black pass in place; colour 1 = red (i + j + k odd)"""
    N = u.shape[0]
    if N < 3:
        return
    hSq = h * h
    s, dg = _sum_diag(u, e, sigma * hSq)
    new = (s - hSq * d[1:-1, 1:-1, 1:-1]) / dg
    m = S._mask(N, colour)
    u[1:-1, 1:-1, 1:-1][m] = new[m]


def pre_smooth(u, d, e, h, sigma, iters):
    for _ in range(iters):
        colour_pass(u, d, e, h, sigma, 1)
        colour_pass(u, d, e, h, sigma, 0)


def post_smooth(u, d, e, h, sigma, iters):
    for _ in range(iters):
        colour_pass(u, d, e, h, sigma, 0)
        colour_pass(u, d, e, h, sigma, 1)


def residual_field(u, d, e, h, sigma):
    """diff on the interior, (N-2)^3"""
    hSq = h * h
    invHsq = 1.0 / hSq
    s, dg = _sum_diag(u, e, sigma * hSq)
    return d[1:-1, 1:-1, 1:-1] - invHsq * (s - dg * u[1:-1, 1:-1, 1:-1])


def residual(u, d, e, h, sigma, r=None):
    diff = residual_field(u, d, e, h, sigma)
    if r is not None:
        r[1:-1, 1:-1, 1:-1] = diff
    return float(np.sqrt((diff * diff).sum()))


def exact_residual_norm(u, d, e, N, h, sigma):
    """sqrt of the exactly rounded sum of the squared residuals (twin of _screened_ref.exact_residual_norm)"""
    diff = residual_field(np.ascontiguousarray(u).reshape(N, N, N), np.ascontiguousarray(d).reshape(N, N, N),
                          np.ascontiguousarray(e).reshape(N, N, N), h, sigma)
    sq = (diff * diff).reshape(-1)
    total = np.longdouble(0)
    step = 1 << 24
    for a in range(0, sq.size, step):
        total += np.sum(sq[a:a + step].astype(np.longdouble))
    return float(np.sqrt(total))


def apply(u, e, h, sigma):
    """the discrete operator on the interior of u (faces of the result are u's: the Dirichlet rows)"""
    hSq = h * h
    s, dg = _sum_diag(u, e, sigma * hSq)
    out = u.copy()
    out[1:-1, 1:-1, 1:-1] = (1.0 / hSq) * (s - dg * u[1:-1, 1:-1, 1:-1])
    return out


def coarse_matrix(N, h, e, sigma):
    """identity rows on the boundary; interior row p: a/h^2 at the six neighbours, -(dg/h^2) on the diagonal"""
    n = N ** 3
    A = np.zeros((n, n))
    e = np.asarray(e, dtype=np.float64).reshape(N, N, N)
    hSq = h * h
    invHsq = 1.0 / hSq
    idx = np.arange(n).reshape(N, N, N)
    bnd = np.ones((N, N, N), dtype=bool)
    bnd[1:-1, 1:-1, 1:-1] = False
    A[idx[bnd], idx[bnd]] = 1.0
    p = idx[1:-1, 1:-1, 1:-1].reshape(-1)
    fs = faces(e)
    NN = N * N
    for a, off in zip(fs, (-NN, NN, -N, N, -1, 1)):
        A[p, p + off] = (a * invHsq).reshape(-1)
    D = fs[0] + fs[1]
    for a in fs[2:]:
        D = D + a
    dg = D + sigma * hSq
    A[p, p] = -(dg * invHsq).reshape(-1)
    return np.ascontiguousarray(A.reshape(-1))


def coarse_lu(N, h, e, sigma):
    A = coarse_matrix(N, h, e, sigma)
    (O.lib().orc_lu_factor_banded if N > 9 else O.lib().orc_lu_factor)(O.P(A), N ** 3)
    return A


def inject(eps, L):
    """eps of every level, level 0 coarsest, from the finest level's (N, N, N) array"""
    out = [np.ascontiguousarray(eps)]
    for _ in range(L - 1):
        out.insert(0, np.ascontiguousarray(out[0][::2, ::2, ::2]))
    return out


class Problem(S.Problem):
    """_screened_ref.Problem with a coefficient eps ((N, N, N) of the finest level; None: the screened reference)."""

    def __init__(self, c, L, nu, sigma, eps, grid_length=1.0):
        super().__init__(c, L, nu, sigma, grid_length)
        self.set_coefficient(eps)

    def _coarse_h(self):
        return self.h * (1 << (self.L - 1))

    def set_coefficient(self, eps):
        self.eps = None if eps is None else inject(np.asarray(eps, dtype=np.float64).reshape((self.N[-1],) * 3), self.L)
        self._factor()

    def set_shift(self, sigma):
        self.sigma = sigma
        self._factor()

    def _factor(self):
        if self.eps is None:
            self.LU = S.coarse_lu(self.c, self._coarse_h(), self.sigma)
        else:
            self.LU = coarse_lu(self.c, self._coarse_h(), self.eps[0], self.sigma)

    def vcycle(self, q=None, h=None):
        if self.eps is None:
            return super().vcycle(q, h)
        q = self.L - 1 if q is None else q
        h = self.h if h is None else h
        v, f, e = self.u[q], self.d[q], self.eps[q]
        if q < self.L - 1:
            v[...] = 0.
        if q == 0:
            x = np.zeros(v.size)
            O.lib().orc_lu_solve(O.P(self.LU), v.size, O.P(np.ascontiguousarray(f.reshape(-1))), O.P(x))
            v[...] = x.reshape(v.shape)
            return 0.
        N, Nc = self.N[q], self.N[q - 1]
        pre_smooth(v, f, e, h, self.sigma, self.nu)
        residual(v, f, e, h, self.sigma, self.r[q])
        dc = np.zeros(Nc ** 3)
        O.lib().orc_restrict(O.P(self.r[q].reshape(-1)), N, O.P(dc), Nc)
        self.d[q - 1][...] = dc.reshape(Nc, Nc, Nc)
        self.vcycle(q - 1, 2 * h)
        vf = np.ascontiguousarray(v.reshape(-1))
        O.lib().orc_prolong(O.P(np.ascontiguousarray(self.u[q - 1].reshape(-1))), Nc, O.P(vf), N)
        v[...] = vf.reshape(v.shape)
        post_smooth(v, f, e, h, self.sigma, self.nu)
        return residual(v, f, e, h, self.sigma)


def smooth_eps(N):
    """1 + 1/2 sin(2 pi x) cos(pi y) on [0, 1]^3"""
    x = np.linspace(0.0, 1.0, N)
    return np.ascontiguousarray(np.broadcast_to(1.0 + 0.5 * np.sin(2 * np.pi * x)[:, None, None] * np.cos(np.pi * x)[None, :, None],
                                                (N, N, N)))


def exp_eps(N):
    """exp(2x + y): a ratio of about 20 over the domain"""
    x = np.linspace(0.0, 1.0, N)
    return np.ascontiguousarray(np.broadcast_to(np.exp(2 * x[:, None, None] + x[None, :, None]), (N, N, N)))


def ball_eps(N, jump=10.0):
    """jump inside the ball of radius 0.25 around the centre, 1 outside"""
    x = np.linspace(0.0, 1.0, N)
    r2 = (x[:, None, None] - 0.5) ** 2 + (x[None, :, None] - 0.5) ** 2 + (x[None, None, :] - 0.5) ** 2
    return np.where(r2 < 0.0625, jump, 1.0)


FIELDS = {"smooth": smooth_eps, "exp": exp_eps, "ball": ball_eps}
