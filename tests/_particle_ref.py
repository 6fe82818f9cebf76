"""CPU restatement of the particle coupling (mg3d_field_sample(_device), mg3d_deposit(_device); include/mg3d.h,
"Particles"): numpy with the library's operands in the library's order, operation by operation, and Python integers where
the library accumulates in 64-bit integers.

axes is the mask of periodic axes, faces the mask of Neumann faces, as in tests/_field_ref.py, whose gradient() gives the
nodal gradient the sample interpolates.  Positions are (M, 3): x along i, y along j, z along k.  Test infrastructure only."""
import math

import numpy as np

import _field_ref as FR

MAX_COUNT = 1 << 40
BLOCK = 256  # threads per block of the point kernels; the grid is capped at MG3D_PARTICLE_MAX_BLOCKS (csrc/mg3d_internal.h)


# --------------------------------------------------------------------------------------------------------------- locate
def locate_axis(x, h, N, periodic):
    """one axis: (inside (M,) bool, c (M,) int, w0, w1 (M,) float).  Entries of points outside are 0 / 0.0."""
    x = np.asarray(x, dtype=np.float64)
    n1 = float(N - 1)
    with np.errstate(all="ignore"):
        t = x / h
        inside = np.isfinite(x) & np.isfinite(t)
        if periodic:
            t = t - n1 * np.floor(t / n1)
            # what the rounding of the wrap leaves outside [0, N-1] goes to the nearer end (-0.0 stays)
            t = np.where(~(t >= 0.0), 0.0, t)
            t = np.where(t > n1, n1, t)
        else:
            inside = inside & (0.0 <= t) & (t <= n1)
        t = np.where(inside, t, 0.0)
        c = np.floor(t).astype(np.int64)
        c = np.where(c > N - 2, N - 2, c)
        f = t - c.astype(np.float64)
        w0, w1 = 1.0 - f, f
    return inside, c, w0, w1


def locate(xyz, h, N, axes):
    """(inside (M,), c (3, M), w (3, 2, M)): a point is inside when it is on every axis"""
    xyz = np.asarray(xyz, dtype=np.float64)
    parts = [locate_axis(xyz[:, ax], h, N, FR.per(axes, ax)) for ax in range(3)]
    inside = parts[0][0] & parts[1][0] & parts[2][0]
    c = np.stack([p[1] for p in parts])
    w = np.stack([np.stack([p[2], p[3]]) for p in parts])
    return inside, c, w


def source(idx, N, periodic):
    """a node index taken to its source: N-1 of a periodic axis is 0"""
    return np.where(idx == N - 1, 0, idx) if periodic else idx


def _corner_index(c, N, axes, a, b, cc):
    return (source(c[0] + a, N, FR.per(axes, 0)), source(c[1] + b, N, FR.per(axes, 1)), source(c[2] + cc, N, FR.per(axes, 2)))


# ---------------------------------------------------------------------------------------------------------------- sample
def _trilinear(field, c, w, N, axes):
    """sum_a wi_a * (sum_b wj_b * (sum_c wk_c * field[corner])), each sum (w0*v0) + (w1*v1)"""
    mid = []
    for a in range(2):
        inner = []
        for b in range(2):
            v0 = field[_corner_index(c, N, axes, a, b, 0)]
            v1 = field[_corner_index(c, N, axes, a, b, 1)]
            inner.append((w[2, 0] * v0) + (w[2, 1] * v1))
        mid.append((w[1, 0] * inner[0]) + (w[1, 1] * inner[1]))
    return (w[0, 0] * mid[0]) + (w[0, 1] * mid[1])


def sample(u, xyz, h, axes, faces, scale=1.0, grad=None):
    """(u (M,), grad (M, 3)) at the points: the trilinear interpolant of u and of the nodal gradient FR.gradient(u, h, axes,
    faces, scale) (pass it as `grad` when it is at hand); NaN for a point outside"""
    N = u.shape[0]
    xyz = np.asarray(xyz, dtype=np.float64)
    inside, c, w = locate(xyz, h, N, axes)
    g = FR.gradient(u, h, axes, faces, scale) if grad is None else grad
    with np.errstate(invalid="ignore"):
        out_u = np.where(inside, _trilinear(u, c, w, N, axes), np.nan)
        out_g = np.stack([np.where(inside, _trilinear(g[d], c, w, N, axes), np.nan) for d in range(3)], axis=1)
    return out_u, out_g


# --------------------------------------------------------------------------------------------------------------- deposit
def count_bits(count):
    """K: the smallest integer with count <= 2^K"""
    K = 0
    while (1 << K) < count:
        K += 1
    return K


def node_factor(N, axes, faces):
    """nf(p) = 2 per Neumann face the node lies on: (N, N, N) float"""
    f = [1.0 / FR.axis_weight(N, axes, faces, ax) for ax in range(3)]
    return f[0][:, None, None] * f[1][None, :, None] * f[2][None, None, :]


def accumulate(xyz, q, h, N, axes):
    """the integer accumulator of a deposit: ({(i, j, k): Python int, nonzero entries only}, ue), or ({}, None) when nothing
    deposits (no point inside with a finite q, or the largest |q| among them is 0).  The order of the points cannot matter:
    integer sums.  The 64-bit range is never left (|sum| <= 2^62 + count / 2), which the function asserts."""
    xyz = np.asarray(xyz, dtype=np.float64)
    q = np.broadcast_to(np.asarray(q, dtype=np.float64), (xyz.shape[0],))
    count = xyz.shape[0]
    inside, c, w = locate(xyz, h, N, axes)
    live = inside & np.isfinite(q)
    if not live.any():
        return {}, None
    A = float(np.max(np.abs(q[live])))
    if A == 0.0:
        return {}, None
    E = math.frexp(A)[1]  # ilogb(A) + 1, denormals included
    ue = E + count_bits(count) - 62
    ql, cl, wl = q[live], c[:, live], w[:, :, live]
    # the contributions are summed as two 31-bit halves in int64 (no sum of either half can overflow), then joined as
    # Python integers: exact whatever the number of points
    lo = np.zeros((N, N, N), dtype=np.int64)
    hi = np.zeros((N, N, N), dtype=np.int64)
    for a in range(2):
        for b in range(2):
            for cc in range(2):
                wt = (wl[0, a] * wl[1, b]) * wl[2, cc]
                n = np.rint(np.ldexp(ql * wt, -ue))  # (np.ldexp is C's ldexp, as math.ldexp: a host test compares them)
                assert np.all(np.abs(n) <= 2.0 ** 62)
                n = n.astype(np.int64)
                idx = _corner_index(cl, N, axes, a, b, cc)
                np.add.at(lo, idx, n & 0x7FFFFFFF)
                np.add.at(hi, idx, n >> 31)
    acc = {}
    for p in zip(*np.nonzero((lo != 0) | (hi != 0))):
        v = (int(hi[p]) << 31) + int(lo[p])
        assert abs(v) < 1 << 63
        if v:
            acc[tuple(int(x) for x in p)] = v
    return acc, ue


def deposit(d, xyz, q, h, axes, faces, scale=1.0):
    """d (N, N, N) after mg3d_deposit: a new array.  d[p] = d[p] + f * ldexp((double)acc, ue) where acc != 0,
    f = (scale * inv_h3) * nf(p); then the duplicates of the periodic axes are refreshed from their sources"""
    N = d.shape[0]
    out = np.array(d, dtype=np.float64, copy=True)
    acc, ue = accumulate(xyz, q, h, N, axes)
    if not acc:
        return out
    inv_h3 = 1.0 / ((h * h) * h)
    f0 = scale * inv_h3
    nf = node_factor(N, axes, faces)
    for p, a in acc.items():
        out[p] = out[p] + (f0 * nf[p]) * math.ldexp(float(a), ue)
    for ax in range(3):
        if FR.per(axes, ax):
            sl_hi, sl_lo = [slice(None)] * 3, [slice(None)] * 3
            sl_hi[ax], sl_lo[ax] = N - 1, 0
            out[tuple(sl_hi)] = out[tuple(sl_lo)]
    return out


# ------------------------------------------------------------------------------------------------------------ test points
def box_points(N, h, count, seed):
    """seeded uniform points inside the box [0, (N-1) h]^3"""
    return np.random.default_rng(seed).uniform(0.0, (N - 1) * h, (count, 3))


def edge_points(N, h, axes):
    """points that lie on nodes, on both ends of every axis, on cell boundaries, far outside on periodic axes and outside /
    not finite on the others: (M, 3).  index*h is exact only for a dyadic h: for any other h the point meant for node i is
    the double nearest to i*h, and (i*h)/h may round to just below i, which puts it into cell i-1 with w1 one ulp below 1
    (node_points() holds every node of an axis; tests/test_particle_length_host.py counts the nodes that do)."""
    length = (N - 1) * h
    nodes = [0.0, -0.0, h, (N - 2) * h, length, (N // 2) * h, 0.5 * h, length - 0.25 * h]
    pts = [(a, b, c) for a in nodes for b in (0.0, length, 1.5 * h) for c in (0.0, length, (N - 2) * h + 0.75 * h)]
    pts += [(b, a, c) for a in nodes for b in (0.25 * h, length) for c in (h, length)]
    pts += [(c, b, a) for a in nodes for b in (0.0, 2.5 * h) for c in (length, 0.125 * h)]
    mid = 1.25 * h
    odd = [-h, -0.5 * h, length + h, np.nextafter(length, np.inf), 3 * length + 0.5 * h, -5 * length - 1.75 * h, 1e6 * length + h,
           np.nan, np.inf, -np.inf, -1e300, 1e300, 5e-324, -5e-324]
    for ax in range(3):
        for v in odd:
            p = [mid, 2 * mid, 0.5 * mid]
            p[ax] = v
            pts.append(tuple(p))
    return np.array(pts, dtype=np.float64)


NODE_OFF = (0.3717, 0.6143)  # the other two coordinates of a node point, as fractions of the box: off the nodes, inside


def node_points(N, h, step=0):
    """for each axis all N coordinates i*h, formed as np.float64(i) * h, the other two coordinates at the fixed positions
    NODE_OFF inside the box: (3 N, 3), axis after axis, node after node.  step = +1 / -1: every node coordinate moved one
    ulp up / down with np.nextafter (below node 0 and above node N-1 that is outside on an axis that is not periodic)"""
    h = np.float64(h)
    x = np.array([np.float64(i) * h for i in range(N)], dtype=np.float64)
    if step:
        x = np.nextafter(x, np.float64(np.inf if step > 0 else -np.inf))
    length = np.float64(N - 1) * h
    pts = np.empty((3, N, 3), dtype=np.float64)
    for ax in range(3):
        pts[ax, :, (ax + 1) % 3] = NODE_OFF[0] * length
        pts[ax, :, (ax + 2) % 3] = NODE_OFF[1] * length
        pts[ax, :, ax] = x
    return pts.reshape(3 * N, 3)


def node_points_all(N, h):
    """the nodes, then the doubles one ulp above them, then those one ulp below: (9 N, 3)"""
    return np.concatenate([node_points(N, h, 0), node_points(N, h, 1), node_points(N, h, -1)])


def low_nodes(N, h):
    """(the i with floor((i*h)/h) == i - 1, the i with (i*h)/h > i), in float64 as the locator divides"""
    h = np.float64(h)
    t = np.array([(np.float64(i) * h) / h for i in range(N)])
    i = np.arange(N)
    return np.flatnonzero(np.floor(t) == i - 1), np.flatnonzero(t > i)
