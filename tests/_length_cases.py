"""What tests/test_length_host.py and tests/test_gpu_length.py share: the operators, sizes and data of the runs on boxes
other than the unit cube, the restatement of each operator at a given grid_length, and the scaling identity.

The identity.  Multiply grid_length by s = 2^m; divide d, sigma, kappa and a step's source by s^2 = 4^m; multiply dt by
4^m; leave eps, the mask, u0 and the Dirichlet data alone.  Then h is 2^m times, hSq 4^m times, 1/hSq 4^-m times the other
run's, sigma*hSq and hSq*d are the same numbers, and every intermediate of every path is the other run's value times an
exact power of two: u of every level has the same bits, d below the top, r and every norm are exactly 4^-m times the other
run's, the gradient 2^-m times, flux and energy (h times a sum of unscaled terms, include/mg3d.h "Field output") 2^m times.
Scaling by a power of two commutes with every rounding as long as nothing overflows or becomes subnormal, whatever the
summation order.  Test infrastructure only."""
import math

import numpy as np

import _coef_ref as CR
import _mask_ref as MR
import _neumann_ref as NR
import _wpcg_ref as WR

LENGTHS = (3e-4, 3.0)            # the electrospray's own; h^2 > h and nothing dyadic
HOST_LENGTHS = (1.0, 3e-4, 3.0)  # bases of the identity on the CPU
MS = (2, -3)
# scale of the gradient: E, and two at which scale * (0.5 / h) and scale / (2 h) round differently at every h of the
# GPU tests that is no power of two (tests/test_length_host.py checks that)
GRAD_SCALES = (-1.0, 2.9, 0.3)
SIZES = {17: (5, 3), 33: (5, 4), 37: (10, 3)}  # a chunk tail, a tiny level, an off-ladder h (c - 1 odd: no periodic axis)

# name: (sigma, eps, periodic axes, Neumann faces, mask)
OPERATORS = {
    "constant": (0.0, False, 0, 0, False),
    "sigma": (3.5, False, 0, 0, False),
    "ball": (0.0, True, 0, 0, False),
    "per7_sigma": (3.5, False, 7, 0, False),
    "per4_f15": (0.0, False, 4, 15, False),   # singular
    "f63": (0.0, False, 0, 63, False),        # singular
    "f22_ball": (0.0, True, 0, 22, False),
    "sphere_f1": (0.0, False, 0, 1, True),    # a sphere of fixed points, Neumann on the low i face
}
PERIODIC = tuple(n for n, o in OPERATORS.items() if o[2])


def n_of(c, L):
    return (c - 1) * (1 << (L - 1)) + 1


def operator(name, N):
    """(sigma, eps or None, axes, faces, mask or None) of the finest level"""
    sigma, coef, axes, faces, masked = OPERATORS[name]
    eps = None
    if coef:
        eps = CR.ball_eps(N, 100.)
        NR.refresh(eps, axes)
    return sigma, eps, axes, faces, (MR.sphere(N) if masked else None)


def singular(name):
    sigma, _, axes, faces, masked = OPERATORS[name]
    return NR.pinned(axes, faces, sigma) and not masked


def reference(name, c, L, nu, grid_length, sigma=None):
    """the restatement of the operator on a box of side grid_length (sigma: another shift than the table's)"""
    sg, eps, axes, faces, mask = operator(name, n_of(c, L))
    sg = sg if sigma is None else sigma
    if mask is not None:
        return MR.Hierarchy(c, L, nu, sg, eps, axes, faces, mask, grid_length)
    return NR.Problem(c, L, nu, sg, eps, axes, faces, grid_length)


def data(name, N, grid_length, seed):
    """random u in (-1, 1) at every point (Dirichlet data included) and random d in (-50, 50) / grid_length^2 -- so that
    hSq*d weighs against the neighbour sum as it does on the unit cube -- periodic-consistent, d with its weighted mean
    over the unknowns taken out where the operator is singular"""
    _, _, axes, faces, _ = OPERATORS[name]
    rng = np.random.default_rng(seed)
    u = rng.uniform(-1, 1, (N, N, N))
    d = rng.uniform(-50, 50, (N, N, N)) / (grid_length * grid_length)
    if singular(name):
        blk = NR.block(N, axes, faces)
        w = NR.weights(N, axes, faces)[blk]
        d[blk] -= math.fsum((w * d[blk]).reshape(-1)) / math.fsum(w.reshape(-1))
    NR.refresh(u, axes)
    NR.refresh(d, axes)
    return u, d


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def normal(a):
    """finite, and no subnormal: what makes the identity a fair demand of these inputs"""
    a = np.asarray(a)
    tiny = np.finfo(a.dtype).tiny
    return bool(np.isfinite(a).all() and ((a == 0) | (np.abs(a) >= tiny)).all())


# ---- what a summation order is worth to three iterations of (weighted) PCG off the unit cube
PCG_OPERATORS = ("constant", "sigma", "ball", "per7_sigma")      # mg3d_pcg_solve accepts these
WPCG_OPERATORS = ("per4_f15", "f63", "f22_ball", "sphere_f1", "ball")
PCG_ITERS = 3


def krylov(name, c, L, grid_length, x0, d, iters, dots, weighted):
    """`iters` iterations of the restatement from x0: (iterates x_1 .. x_iters, norms r_0 .. r_iters).  weighted: the w
    inner product of mg3d_wpcg_solve (over the masked hierarchy where the operator has a mask), else _pcg_ref.pcg over
    the problem class mg3d_pcg_solve's own tests use"""
    import _pcg_ref as PR
    hist = []
    sg, eps, axes, faces, mask = operator(name, n_of(c, L))
    if not weighted:
        prob = PR.make_problem(c, L, 2, sg, eps, axes, grid_length)
        _, norms, _ = PR.pcg(prob, x0, d, 0., 1e-300, iters, dots, hist)
    elif mask is not None:
        _, norms, _, _, _ = MR.wpcg(reference(name, c, L, 2, grid_length), x0, d, 0., 1e-300, iters, dots, hist)
    else:
        prob = WR.make_problem(c, L, 2, sg, eps, axes, faces, grid_length)
        _, norms, _, _ = WR.wpcg(prob, x0, d, 0., 1e-300, iters, dots, hist)
    return hist, norms


def krylov_data(name, N, grid_length, seed=5):
    """the start of the PCG runs: data()'s u and d, u at a fixed point 1.0"""
    u, d = data(name, N, grid_length, seed)
    mask = operator(name, N)[4]
    if mask is not None:
        u[mask != 0] = 1.0
    return u, d


def summation_spread(weighted, sizes=(17, 33, 37), lengths=LENGTHS):
    """the procedure of _pcg_ref.summation_spread / _wpcg_ref.summation_spread at these lengths, on the data of the GPU
    tests: per k = 1 .. PCG_ITERS the largest relative difference max|a - b| / max|a| of the iterates x_k between a run
    with exactly rounded sums and one with numpy's pairwise float64 sums, and the largest one of the norms"""
    su, sn = [0.0] * PCG_ITERS, 0.0
    for name in (WPCG_OPERATORS if weighted else PCG_OPERATORS):
        for N in sizes:
            if N == 37 and name in PERIODIC:
                continue
            for length in lengths:
                c, L = SIZES[N]
                x0, d = krylov_data(name, N, length)
                ha, na = krylov(name, c, L, length, x0, d, PCG_ITERS, "exact", weighted)
                hb, nb = krylov(name, c, L, length, x0, d, PCG_ITERS, "plain", weighted)
                for k in range(PCG_ITERS):
                    su[k] = max(su[k], float(np.abs(ha[k] - hb[k]).max() / np.abs(ha[k]).max()))
                sn = max(sn, float((np.abs(na - nb) / na).max()))
    return su, sn


if __name__ == "__main__":
    for weighted in (False, True):
        su, sn = summation_spread(weighted)
        print("wpcg" if weighted else "pcg", "u, k = 1, 2, 3:", " ".join(f"{v:.2e}" for v in su), "  norms:", f"{sn:.2e}")
