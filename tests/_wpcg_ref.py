"""CPU restatement of mg3d_wpcg_solve: conjugate gradients in the w-weighted inner product, preconditioned by one V-cycle
per iteration, over the cycle of tests/_neumann_ref.py -- Neumann faces, periodic axes, sigma, eps, and the singular case
(every axis periodic or Neumann on both faces, sigma = 0).  With no Neumann face and no periodic axis the same class runs
the plain context.

w is _neumann_ref.weights on the unknowns: 1/2 per Neumann face a point lies on, 1 otherwise.  The reflected operator A
and the cycle are self-adjoint in <a, b>_w = sum w a b; r.z and p.Ap are taken in it, the norms stay Euclidean over the
unknowns.  In the singular case, with W = sum w:
    r_0 = (d - A x) - sum(w (d - A x)) / W          p = (z - sum(w z) / W) + beta p          r is never re-projected
and r.z is sum w r z of the z the cycle returned: r has w-mean zero, so the constant the projection removes from z does
not enter it.  d is never changed; rhs_mean = sum(w d) / W is what was projected out of it.

The cycles are bit-exact restatements of the library's and the vector updates keep its operand order; only the sums
differ from the GPU, in summation order: each product is rounded to float64 as on the GPU (w is a power of two: exact)
and the sum is exactly rounded (math.fsum), or, with dots="plain", numpy's pairwise float64 sum.  Signs are the library's:
A is negative (semi)definite, r = d - A x, z = V(r), both dots negative.  Test infrastructure only."""
import math

import numpy as np

import _coef_ref as CR
import _neumann_ref as NR
import _pcg_ref as PR


def _top_eps(prob):
    return None if prob.eps is None else prob.eps[-1]


def weights(prob):
    """w on the block of unknowns and W = sum w (a multiple of 1/8: exact)"""
    N = prob.N[-1]
    w = NR.weights(N, prob.axes, prob.faces)[NR.block(N, prob.axes, prob.faces)]
    assert w.min() >= 0.125
    return w, math.fsum(w.reshape(-1))


def singular(prob):
    return NR.pinned(prob.axes, prob.faces, prob.sigma)


def residual_field(prob, x, d):
    return NR.residual_field(x, d, _top_eps(prob), prob.h, prob.sigma, prob.axes, prob.faces)


def apply(prob, v):
    """A v at the unknowns: the residual's expression with d = 0, negated (0 - y is -y exactly)"""
    return -residual_field(prob, v, np.zeros_like(v))


def wsum(w, a, dots="exact"):
    prod = (w * a).reshape(-1)
    return math.fsum(prod) if dots == "exact" else float(np.sum(prod))


def wdot(w, a, b, dots="exact"):
    return wsum(w, a * b, dots)


def precondition(prob, r_blk):
    """z = one V-cycle from a zero guess with right-hand side r (given on the unknowns); the whole array"""
    N = prob.N[-1]
    prob.u[-1][...] = 0.
    prob.d[-1][...] = 0.
    prob.d[-1][NR.block(N, prob.axes, prob.faces)] = r_blk
    prob.vcycle()
    return prob.u[-1].copy()


_numpy_cycle = precondition


def wpcg(prob, x0, d, rtol, atol, max_iters, dots="exact", history=None, precondition=None):
    """Returns (x, norms r_0 .. r_k, converged, rhs_mean).  x0, d: (N, N, N) of the finest level, not modified.  history
    (a list) receives a copy of x after every iteration.  precondition(prob, r_blk) -> the whole array z replaces the numpy
    cycle (`precondition` above) -- prob then needs no hierarchy, only what residual_field and weights read and r = [];
    the residual, apply, every sum, the projection, the direction and the update stay the numpy code below."""
    cycle = _numpy_cycle if precondition is None else precondition
    N = prob.N[-1]
    blk = NR.block(N, prob.axes, prob.faces)
    w, W = weights(prob)
    sing = singular(prob)
    x = np.array(x0, dtype=np.float64).reshape(N, N, N).copy()
    d = np.asarray(d, dtype=np.float64).reshape(N, N, N)
    for a in prob.r:
        a[...] = 0.
    r = residual_field(prob, x, d)
    rhs_mean = 0.
    if sing:
        rhs_mean = wsum(w, d[blk], dots) / W
        r = r - wsum(w, r, dots) / W
    norms = [math.sqrt(PR.dot(r, r, dots))]
    target = max(rtol * norms[0], atol)
    if norms[0] == 0. or (max_iters > 0 and norms[0] <= target):
        return x, np.array(norms), True, rhs_mean
    p = None
    rz_old = None
    for k in range(max_iters):
        z = cycle(prob, r)
        rz = wdot(w, r, z[blk], dots)
        m = wsum(w, z[blk], dots) / W if sing else 0.
        if k == 0:
            pb = z[blk] - m
        else:
            beta = rz / rz_old
            pb = (z[blk] - m) + beta * p[blk]
        p = np.zeros((N, N, N))
        NR.put(p, pb, blk, prob.axes)
        q = apply(prob, p)
        pap = wdot(w, p[blk], q, dots)
        if not (rz < 0. and math.isfinite(rz) and pap < 0. and math.isfinite(pap)):
            return x, np.array(norms), False, rhs_mean
        alpha = rz / pap
        xb = x[blk] + alpha * p[blk]
        NR.put(x, xb, blk, prob.axes)
        r = r - alpha * q
        rz_old = rz
        norms.append(math.sqrt(PR.dot(r, r, dots)))
        if history is not None:
            history.append(x.copy())
        if norms[-1] <= target:
            return x, np.array(norms), True, rhs_mean
    return x, np.array(norms), False, rhs_mean


def wmean(prob, a):
    """sum(w a) / W over the unknowns, exactly rounded sum"""
    w, W = weights(prob)
    return wsum(w, np.asarray(a).reshape((prob.N[-1],) * 3)[NR.block(prob.N[-1], prob.axes, prob.faces)]) / W


def true_residual_norm(prob, x, d, project=None):
    """||d - A x|| over the unknowns; project (default: in the singular case) the w-mean is taken out first"""
    diff = residual_field(prob, x, d)
    if singular(prob) if project is None else project:
        w, W = weights(prob)
        diff = diff - wsum(w, diff) / W
    return math.sqrt(math.fsum((diff * diff).reshape(-1)))


def w_asymmetry(prob, op, seed=0):
    """|<x, op y>_w - <op x, y>_w| / |<x, op y>_w| for two random vectors on the unknowns (w-mean zero in the singular case,
    where the cycle is symmetric on that subspace only); op maps a block of unknowns to one: `apply_blk` or `cycle_blk`"""
    N = prob.N[-1]
    w, W = weights(prob)
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-1, 1, w.shape), rng.uniform(-1, 1, w.shape)
    proj = (lambda a: a - wsum(w, a) / W) if singular(prob) else (lambda a: a)
    x, y = proj(x), proj(y)
    a, b = wdot(w, x, proj(op(prob, y))), wdot(w, proj(op(prob, x)), y)
    return abs(a - b) / abs(a)


def apply_blk(prob, v_blk):
    N = prob.N[-1]
    v = np.zeros((N, N, N))
    NR.put(v, v_blk, NR.block(N, prob.axes, prob.faces), prob.axes)
    return apply(prob, v)


def cycle_blk(prob, r_blk):
    for a in prob.r:
        a[...] = 0.
    return precondition(prob, r_blk)[NR.block(prob.N[-1], prob.axes, prob.faces)]


def make_problem(c, L, nu, sigma=0.0, eps=None, axes=0, faces=0, grid_length=1.0):
    return NR.Problem(c, L, nu, sigma, eps, axes, faces, grid_length)


# ------------------------------------------------------------------------------------------------ the cases of the tests
# name: (c, L, sigma, eps of the finest level from N or None, periodic axes, Neumann faces)
_ball = lambda N: CR.ball_eps(N, 100.)
CASES = {
    "17_f1": (5, 3, 0.0, _ball, 0, 1),
    "17_f2": (5, 3, 0.0, _ball, 0, 2),
    "17_f4": (5, 3, 0.0, _ball, 0, 4),
    "17_f8": (5, 3, 0.0, _ball, 0, 8),
    "17_f16": (5, 3, 0.0, _ball, 0, 16),
    "17_f32": (5, 3, 0.0, _ball, 0, 32),
    "f63_ball": (5, 4, 0.0, _ball, 0, 63),  # singular
    "f63_slab": (5, 4, 0.0, lambda N: PR.slab_eps(N, 1e4), 0, 63),  # singular
    "per4_f15_ball": (5, 4, 0.0, _ball, 4, 15),  # singular
    "per7_ball": (5, 4, 0.0, _ball, 7, 0),  # singular, no Neumann face
    "f22_ball": (5, 4, 0.0, _ball, 0, 22),  # ihi + jlo + klo: not singular, edges shared with Dirichlet faces
    "f63_sigma3": (5, 4, 3.0, None, 0, 63),  # not singular: no projection
    "37_f25": (10, 3, 0.0, _ball, 0, 0b011001),  # off the 2^k+1 ladder: ilo + jhi + klo
    "25_per2_f51": (7, 3, 0.0, _ball, 2, 51),  # singular, off the ladder
}
SINGULAR = [n for n, c in CASES.items() if NR.pinned(c[4], c[5], c[2])]


def case_problem(name, nu=2):
    c, L, sigma, field, axes, faces = CASES[name]
    N = (c - 1) * (1 << (L - 1)) + 1
    eps = None if field is None else field(N)
    return N, eps, make_problem(c, L, nu, sigma, eps, axes, faces)


def random_guess(N, axes, faces, seed=5, dirichlet=False):
    """uniform(-1, 1) on the unknowns, periodic-consistent; Dirichlet points 0, or random as well"""
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(-1, 1, (N, N, N))
    if not dirichlet:
        x0[~NR.unknown_mask(N, axes, faces)] = 0.
    NR.refresh(x0, axes)
    return x0


def summation_spread(iters=(1, 2, 5), names=None):
    """for every case, from random_guess with d = 0, between a run with exactly rounded sums and one with numpy's pairwise
    float64 sums: the relative difference max|a - b| / max|a| of the iterates x_k, that of the norms, and, in the singular
    cases, the drift of the w-mean of x_k from that of the guess relative to max|x_0| (the larger of the two runs)"""
    out = {}
    for name in names or CASES:
        N, _, pa = case_problem(name)
        _, _, pb = case_problem(name)
        x0, d = random_guess(N, pa.axes, pa.faces), np.zeros((N, N, N))
        ha, hb = [], []
        _, na, _, _ = wpcg(pa, x0, d, 0., 1e-300, max(iters), "exact", ha)
        _, nb, _, _ = wpcg(pb, x0, d, 0., 1e-300, max(iters), "plain", hb)
        drift = None
        if singular(pa):
            m0 = wmean(pa, x0)
            drift = max(abs(wmean(pa, h[k - 1]) - m0) for h in (ha, hb) for k in iters) / np.abs(x0).max()
        out[name] = ([float(np.abs(ha[k - 1] - hb[k - 1]).max() / np.abs(ha[k - 1]).max()) for k in iters],
                     float((np.abs(na - nb) / na).max()), drift)
    return out


if __name__ == "__main__":
    sp = summation_spread()
    for name, (u, n, dr) in sp.items():
        print(f"{name:16s} u, k = 1, 2, 5: " + " ".join(f"{v:.2e}" for v in u) + f"   norms: {n:.2e}"
              + ("" if dr is None else f"   w-mean drift: {dr:.2e}"))
    print("largest per k:", " ".join(f"{max(v[0][i] for v in sp.values()):.2e}" for i in range(3)),
          "  norms:", f"{max(v[1] for v in sp.values()):.2e}",
          "  w-mean drift:", f"{max(v[2] for v in sp.values() if v[2] is not None):.2e}")
