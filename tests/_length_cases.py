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

# ---- the particle calls off the unit cube (tests/test_particle_length_host.py, tests/test_gpu_particle_length.py)
# N: ((c, L) under Dirichlet or Neumann faces, (c, L) with a periodic axis, which needs an even c - 1, or None).  Sizes at
# which a coordinate formed as i*h locates in cell i - 1 at one of LENGTHS (LOW_NODES); 65: the row pitch passes one
# 64-lane block
PARTICLE_SIZES = {21: ((6, 3), (11, 2)), 37: ((10, 3), None), 41: ((6, 4), (11, 3)), 65: ((5, 5), (5, 5))}
# (periodic axes, Neumann faces), the sets of tests/test_gpu_particles.py
BCS = {"dirichlet": (0, 0), "per7": (7, 0), "per4_f15": (4, 15), "f63": (0, 63), "f22": (0, 22), "f25": (0, 0b011001)}
# {(N, length): (nodes i with floor((i*h)/h) == i - 1, nodes with (i*h)/h > i)}, h = length / (N - 1) in float64, counted
# by _particle_ref.low_nodes; tests/test_particle_length_host.py asserts the table
# GRAD_SCALES and one more: at 3e-4 / 20 and 3e-4 / 40 none of the three tells scale * (0.5 / h) from scale / (2 h), 3.9
# does.  At 3.0 / 20 and 3.0 / 40 no scale does (none of 200 000 random ones in (1e-3, 1e3): 0.5 / h is too close to its
# exact value there), which tests/test_particle_length_host.py records
PARTICLE_GRAD_SCALES = GRAD_SCALES + (3.9,)
LOW_NODES = {(21, 3e-4): (3, 2), (37, 3e-4): (0, 0), (41, 3e-4): (5, 4), (65, 3e-4): (6, 0),
             (21, 3.0): (0, 2), (37, 3.0): (5, 0), (41, 3.0): (1, 3), (65, 3.0): (0, 0)}


def particle_shape(N, bc):
    """(c, L) of a particle case"""
    plain, periodic = PARTICLE_SIZES[N]
    return periodic if BCS[bc][0] else plain


def particle_cases(extra=(("per4_f15", 41, 3.0),)):
    """[(boundary set, N, length)]: every boundary set meets both lengths, the sizes rotate (no periodic set at 37), as
    _pruned of tests/test_gpu_length.py does it; `extra`: the rotation gives the periodic sets no size with a low node at
    3.0, so one such case is added"""
    out = []
    for i, bc in enumerate(BCS):
        for j, length in enumerate(LENGTHS):
            ok = [n for n in PARTICLE_SIZES if PARTICLE_SIZES[n][1] is not None or not BCS[bc][0]]
            out.append((bc, ok[(i + j) % len(ok)], length))
    return out + [c for c in extra if c not in out]


PUSH_COUNT, PUSHES = 1000, 3  # seeded particles beside the edge and node points; pushes in sequence
SORT_COUNT = 4099             # all particles of a sort case, the edge and node points first


def push_cases():
    """[(boundary set, N, length, with a mask)]: particle_cases(), the mask of two bodies on every other case, so that
    each length meets it under several boundary sets"""
    return [(bc, N, length, n % 2 == 0) for n, (bc, N, length) in enumerate(particle_cases())]


def scale_particles(m, xyz, vel=None, qm=None, accel=None):
    """the particle inputs of the identity at s = 2^m: positions, velocities and accel times s, q/m times s^2 (dt, drag, u,
    the charges and the mask stay; a deposit's scale takes s and d goes over s^2, as above)"""
    s = 2.0 ** m
    out = [np.asarray(xyz) * s]
    if vel is not None:
        out.append(np.asarray(vel) * np.asarray(vel).dtype.type(s))
    if qm is not None:
        out.append(np.asarray(qm) * (s * s))
    if accel is not None:
        out.append(tuple(a * s for a in accel))
    return out[0] if len(out) == 1 else tuple(out)


def fair_points(xyz):
    """the rows of xyz without a subnormal coordinate (a subnormal does not scale exactly; NaN and inf do): what the
    identity may be asked of"""
    xyz = np.asarray(xyz)
    tiny = np.finfo(np.float64).tiny
    return xyz[~((xyz != 0) & (np.abs(xyz) < tiny)).any(axis=1)]


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


# ---- the same for the screening field and the KEEP rule (tests/test_gpu_length_fields.py)
# name: (call, periodic axes, Neumann faces, eps, screening field, KEEP mask)
FIELD_KRYLOV = {
    "sfield_pcg": ("pcg_solve", 0, 0, True, True, False),     # the cases of tests/test_gpu_shift_field.py's solvers
    "sfield_wpcg": ("wpcg_solve", 0, 63, False, True, False),
    "keep_pcg": ("pcg_solve", 0, 0, False, False, True),      # _mask_keep_ref.thin_mask under KEEP
    "keep_wpcg": ("wpcg_solve", 4, 3, False, False, True),
    "keep_sfield_wpcg": ("wpcg_solve", 4, 3, False, True, True),
}
FIELD_KRYLOV_SIZES = (17, 33)


def field_krylov_problem(name, N, grid_length):
    """(make, x0, d): make() builds the restatement's hierarchy; x0 and d are data()'s -- u random in (-1, 1), 1.0 at the
    fixed points, d random in (-50, 50) / grid_length^2; the field is random in [0, 1/h^2] with this length's h"""
    import _mask_keep_ref as MK
    import _shift_field_ref as SF
    _, axes, faces, coef, with_field, masked = FIELD_KRYLOV[name]
    c, L = SIZES[N]
    h = grid_length / (N - 1)
    eps = CR.FIELDS["exp"](N) if coef else None
    field = SF.random_field(N, h) if with_field else None
    mask = MK.thin_mask(N) if masked else None
    rng = np.random.default_rng(5 + N)
    x0 = rng.uniform(-1, 1, (N, N, N))
    d = rng.uniform(-50, 50, (N, N, N)) / (grid_length * grid_length)
    if mask is not None:
        x0[mask != 0] = 1.0
    NR.refresh(x0, axes)
    NR.refresh(d, axes)

    def make():
        if mask is not None and field is not None:
            return MK.FieldHierarchy(c, L, 2, 0.0, eps, axes, faces, mask, field, grid_length)
        if mask is not None:
            return MK.Hierarchy(c, L, 2, 0.0, eps, axes, faces, mask, grid_length)
        return SF.Hierarchy(c, L, 2, 0.0, eps, axes, faces, None, field, grid_length)

    return make, x0, d, eps, field, mask


def field_krylov(prob, x0, d, iters, dots):
    """(iterates x_1 .. x_iters, norms r_0 .. r_iters) of the restatement on a hierarchy of field_krylov_problem"""
    import _shift_field_ref as SF
    hist = []
    solve = SF.wpcg if getattr(prob, "s", None) is not None else MR.wpcg
    _, norms, _, _, _ = solve(prob, x0, d, 0., 1e-300, iters, dots, hist)
    return hist, norms


def field_summation_spread(names, sizes=FIELD_KRYLOV_SIZES, lengths=LENGTHS):
    """summation_spread's procedure over the cases `names` of FIELD_KRYLOV: ([spread of x_k, k = 1 .. PCG_ITERS], spread of
    the norms), the largest over the names, sizes and lengths"""
    su, sn = [0.0] * PCG_ITERS, 0.0
    for name in names:
        for N in sizes:
            for length in lengths:
                make, x0, d = field_krylov_problem(name, N, length)[:3]
                ha, na = field_krylov(make(), x0, d, PCG_ITERS, "exact")
                hb, nb = field_krylov(make(), x0, d, PCG_ITERS, "plain")
                for k in range(PCG_ITERS):
                    su[k] = max(su[k], float(np.abs(ha[k] - hb[k]).max() / np.abs(ha[k]).max()))
                sn = max(sn, float((np.abs(na - nb) / na).max()))
    return su, sn


if __name__ == "__main__":
    for weighted in (False, True):
        su, sn = summation_spread(weighted)
        print("wpcg" if weighted else "pcg", "u, k = 1, 2, 3:", " ".join(f"{v:.2e}" for v in su), "  norms:", f"{sn:.2e}")
    for call in ("pcg_solve", "wpcg_solve"):
        su, sn = field_summation_spread([n for n, v in FIELD_KRYLOV.items() if v[0] == call])
        print("field/keep", call, "u, k = 1, 2, 3:", " ".join(f"{v:.2e}" for v in su), "  norms:", f"{sn:.2e}")
