"""CPU restatement of mg3d_pcg_solve: conjugate gradients preconditioned by one V-cycle per iteration, over the cycles of
tests/_screened_ref.py (constant operator, sigma), tests/_coef_ref.py (eps) and tests/_periodic_ref.py (periodic axes).

The cycles are bit-exact restatements of the library's, and the vector updates below keep its operand order
(x + alpha*p, r - alpha*q, z + beta*p, alpha = (r.z)/(p.Ap), beta Fletcher-Reeves); only the dots differ from the GPU, in
summation order: here each product is rounded to float64 as on the GPU and the sum is exactly rounded (math.fsum), or,
with dots="plain", numpy's pairwise float64 sum -- the pair of runs that measures what a summation order is worth.

The operator is negative definite; signs are the library's: r = d - A x, z = V(r) ~ A^-1 r, both dots negative.
Test infrastructure only."""
import math

import numpy as np

import _coef_ref as CR
import _periodic_ref as P


def _parts(prob):
    """(axes, eps of the finest level or None) of any of the three Problem classes"""
    axes = getattr(prob, "axes", 0)
    eps = getattr(prob, "eps", None)
    return axes, None if eps is None else eps[-1]


def apply(prob, v):
    """A v at the unknowns of the finest level (the block of P.unique_block): the residual's expression with d = 0,
    negated -- 0 - y is -y exactly, so this is invHsq*(s - dg*v) bit for bit"""
    axes, e = _parts(prob)
    return -P.residual_field(v, np.zeros_like(v), e, prob.h, prob.sigma, axes)


def residual_field(prob, x, d):
    axes, e = _parts(prob)
    return P.residual_field(x, d, e, prob.h, prob.sigma, axes)


def dot(a, b, dots="exact"):
    prod = (a * b).reshape(-1)
    return math.fsum(prod) if dots == "exact" else float(np.sum(prod))


def precondition(prob, r_blk):
    """z = one V-cycle from a zero guess with right-hand side r (given on the unknowns; its faces and duplicates are not
    read); returns the whole array: zero Dirichlet faces, consistent duplicates"""
    axes, _ = _parts(prob)
    N = prob.N[-1]
    prob.u[-1][...] = 0.
    prob.d[-1][...] = 0.
    prob.d[-1][P.unique_block(N, axes)] = r_blk
    prob.vcycle()
    return prob.u[-1].copy()


_numpy_cycle = precondition


def pcg(prob, x0, d, rtol, atol, max_iters, dots="exact", history=None, precondition=None):
    """Returns (x, norms r_0 .. r_k, converged).  x0, d: (N, N, N) of the finest level; x0 is not modified.  history
    (a list) receives a copy of x after every iteration.  precondition(prob, r_blk) -> the whole array z (zero Dirichlet
    faces, consistent duplicates) replaces the numpy cycle (`precondition` above) -- prob then needs no hierarchy, only
    what residual_field reads and r = []; the residual, apply, every dot, the direction and the update stay the numpy
    code below."""
    cycle = _numpy_cycle if precondition is None else precondition
    axes, _ = _parts(prob)
    N = prob.N[-1]
    blk = P.unique_block(N, axes)
    x = np.array(x0, dtype=np.float64).reshape(N, N, N).copy()
    d = np.asarray(d, dtype=np.float64).reshape(N, N, N)
    for a in prob.r:
        a[...] = 0.
    r = residual_field(prob, x, d)
    norms = [math.sqrt(dot(r, r, dots))]
    target = max(rtol * norms[0], atol)
    if norms[0] == 0. or (max_iters > 0 and norms[0] <= target):
        return x, np.array(norms), True
    p = None
    rz_old = None
    for k in range(max_iters):
        z = cycle(prob, r)
        rz = dot(r, z[blk], dots)
        if k == 0:
            p = z
        else:
            beta = rz / rz_old
            pb = z[blk] + beta * p[blk]
            p = z  # (faces of z are zero, as p's are)
            P.put(p, pb, blk, axes)
        q = apply(prob, p)
        pap = dot(p[blk], q, dots)
        if not (rz < 0. and math.isfinite(rz) and pap < 0. and math.isfinite(pap)):
            return x, np.array(norms), False
        alpha = rz / pap
        xb = x[blk] + alpha * p[blk]
        P.put(x, xb, blk, axes)
        r = r - alpha * q
        rz_old = rz
        norms.append(math.sqrt(dot(r, r, dots)))
        if history is not None:
            history.append(x.copy())
        if norms[-1] <= target:
            return x, np.array(norms), True
    return x, np.array(norms), False


def true_residual_norm(prob, x, d):
    diff = residual_field(prob, x, d)
    return math.sqrt(math.fsum((diff * diff).reshape(-1)))


def slab_eps(N, jump=1e4):
    """jump inside the slab 0.3 < x < 0.62, 1 outside"""
    x = np.linspace(0.0, 1.0, N)
    return np.ascontiguousarray(np.broadcast_to(np.where((x > 0.3) & (x < 0.62), jump, 1.0)[:, None, None], (N, N, N)))


def make_problem(c, L, nu, sigma=0.0, eps=None, axes=0, grid_length=1.0):
    """the restatement whose cycle the library runs for these settings"""
    if axes:
        return P.Problem(c, L, nu, sigma, eps, axes, grid_length)
    return CR.Problem(c, L, nu, sigma, eps, grid_length)


# ------------------------------------------------------------------------------------------------ the cases of the tests
# name: (c, L, sigma, eps of the finest level from N or None, periodic axes)
CASES = {
    "ball100": (5, 4, 0.0, lambda N: CR.ball_eps(N, 100.), 0),
    "ball0.01": (5, 4, 0.0, lambda N: CR.ball_eps(N, 0.01), 0),
    "slab1e4": (5, 4, 0.0, lambda N: slab_eps(N, 1e4), 0),
    "constant": (5, 4, 0.0, None, 0),
    "sigma100": (5, 4, 100.0, None, 0),
    "per6_smooth": (5, 4, 0.0, CR.smooth_eps, 6),
    "per7_sigma50": (5, 4, 50.0, None, 7),
    "37_ball100": (10, 3, 0.0, lambda N: CR.ball_eps(N, 100.), 0),  # off the 2^k+1 ladder, a k tail
    "25_per2_smooth": (7, 3, 0.0, CR.smooth_eps, 2),
}


def case_problem(name, nu=2):
    c, L, sigma, field, axes = CASES[name]
    N = (c - 1) * (1 << (L - 1)) + 1
    eps = None if field is None else field(N)
    return N, eps, make_problem(c, L, nu, sigma, eps, axes)


def random_guess(N, axes, seed=5, faces=False):
    """uniform(-1, 1) on the unknowns, periodic-consistent; Dirichlet faces 0, or random as well"""
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(-1, 1, (N, N, N))
    if not faces:
        keep = np.zeros((N, N, N), dtype=bool)
        keep[P.unique_block(N, axes)] = True
        x0[~keep] = 0.
    P.refresh(x0, axes)
    return x0


def summation_spread(iters=(1, 2, 5)):
    """for every case, from random_guess with d = 0: the relative difference max|a - b| / max|a| of the iterates x_k, and
    of the norms, between a run with exactly rounded dots and one with numpy's pairwise float64 sums"""
    out = {}
    for name in CASES:
        N, _, pa = case_problem(name)
        _, _, pb = case_problem(name)
        x0, d = random_guess(N, CASES[name][4]), np.zeros((N, N, N))
        ha, hb = [], []
        _, na, _ = pcg(pa, x0, d, 0., 1e-300, max(iters), "exact", ha)
        _, nb, _ = pcg(pb, x0, d, 0., 1e-300, max(iters), "plain", hb)
        out[name] = ([float(np.abs(ha[k - 1] - hb[k - 1]).max() / np.abs(ha[k - 1]).max()) for k in iters],
                     float((np.abs(na - nb) / na).max()))
    return out


if __name__ == "__main__":
    sp = summation_spread()
    for name, (u, n) in sp.items():
        print(f"{name:16s} u, k = 1, 2, 5: " + " ".join(f"{v:.2e}" for v in u) + f"   norms: {n:.2e}")
    print("largest per k:", " ".join(f"{max(v[0][i] for v in sp.values()):.2e}" for i in range(3)),
          "  norms:", f"{max(v[1] for v in sp.values()):.2e}")
