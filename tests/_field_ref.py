"""CPU restatement of the field output (mg3d_field_gradient(_device), mg3d_field_flux, mg3d_field_energy; include/mg3d.h,
"Field output"): numpy with the library's operands in the library's order, operation by operation.

axes is the mask of periodic axes (1 = i, 2 = j, 4 = k), faces the mask of Neumann faces (1 = i low, 2 = i high, 4 = j
low, 8 = j high, 16 = k low, 32 = k high), as in tests/_neumann_ref.py.  On axis a index x is a duplicate if the axis is
periodic and x = N-1, on a Dirichlet face if the axis is not periodic and x = 0 / N-1 without the matching Neumann bit, on
a Neumann face with it.  The gradient is bit for bit what the kernel stores; the flux and the energy are returned as their
TERMS, to be summed by `fsum` (exactly rounded): the GPU's reduction is a different summation order.  Test infrastructure
only."""
import math

import numpy as np


def per(axes, ax):
    return (axes >> ax) & 1 == 1


def neu(faces, ax, hi):
    return (faces >> (2 * ax + hi)) & 1 == 1


def on_dirichlet(N, axes, faces, ax):
    """(N,) bool: the indices of an axis that lie on a Dirichlet face"""
    d = np.zeros(N, dtype=bool)
    if not per(axes, ax):
        d[0] = not neu(faces, ax, 0)
        d[N - 1] = not neu(faces, ax, 1)
    return d


def axis_weight(N, axes, faces, ax):
    """(N,) float: 1/2 on a Neumann face of the axis, else 1"""
    w = np.ones(N)
    if not per(axes, ax):
        if neu(faces, ax, 0):
            w[0] = 0.5
        if neu(faces, ax, 1):
            w[N - 1] = 0.5
    return w


def unknown_axis(N, axes, faces, ax):
    """(N,) bool: no duplicate, on no Dirichlet face"""
    u = ~on_dirichlet(N, axes, faces, ax)
    if per(axes, ax):
        u[N - 1] = False
    return u


def _outer(a, b, c):
    return a[:, None, None] * b[None, :, None] * c[None, None, :]


def fsum(*arrays):
    """the exactly rounded sum of every entry (zeros are dropped first: they change no exact sum)"""
    parts = []
    for a in arrays:
        a = np.asarray(a).reshape(-1)
        parts.append(a[a != 0])
    return math.fsum(np.concatenate(parts)) if parts else 0.0


# ------------------------------------------------------------------------------------------------------------- gradient
def gradient(u, h, axes, faces, scale):
    """scale * du/dx_a at every point: three (N, N, N) arrays.  A point is first taken to its source (index N-1 of a
    periodic axis -> 0, on all three axes); then per axis the wrapped / central / reflected / one-sided difference."""
    N = u.shape[0]
    cs = scale * (0.5 / h)
    src = u
    for ax in range(3):
        if per(axes, ax):
            src = np.take(src, list(range(N - 1)) + [0], axis=ax)
    out = []
    for ax in range(3):
        v = np.moveaxis(src, ax, 0)
        g = np.empty_like(v)
        if per(axes, ax):
            x = np.arange(N)
            xs = np.where(x == N - 1, 0, x)
            lo = np.where(xs == 0, N - 2, xs - 1)
            hi = np.where(xs == N - 2, 0, xs + 1)
            g[:] = (v[hi] - v[lo]) * cs
        else:
            g[1:N - 1] = (v[2:] - v[:N - 2]) * cs
            if neu(faces, ax, 0):
                g[0] = (v[1] - v[1]) * cs
            else:
                g[0] = ((4.0 * v[1] - 3.0 * v[0]) - v[2]) * cs
            if neu(faces, ax, 1):
                g[N - 1] = (v[N - 2] - v[N - 2]) * cs
            else:
                g[N - 1] = ((3.0 * v[N - 1] - 4.0 * v[N - 2]) + v[N - 3]) * cs
        out.append(np.ascontiguousarray(np.moveaxis(g, 0, ax)))
    return out


# ----------------------------------------------------------------------------------------------------------------- flux
def flux_points(mask, axes, faces, label=0):
    """(N, N, N) bool: the fixed unknowns whose byte is `label` (0: any nonzero byte)"""
    N = mask.shape[0]
    m = np.asarray(mask)
    unk = (unknown_axis(N, axes, faces, 0)[:, None, None] & unknown_axis(N, axes, faces, 1)[None, :, None]
           & unknown_axis(N, axes, faces, 2)[None, None, :])
    return unk & ((m != 0) if label == 0 else (m == label))


def _neighbours(x, N, axes, faces, ax):
    """the -1 / +1 neighbour indices of the unknown indices x of an axis: wrapped or reflected"""
    if per(axes, ax):
        return np.where(x == 0, N - 2, x - 1), np.where(x == N - 2, 0, x + 1)
    lo = np.where((x == 0) & neu(faces, ax, 0), 1, x - 1)
    hi = np.where((x == N - 1) & neu(faces, ax, 1), N - 2, x + 1)
    return lo, hi


def flux_terms(u, eps, mask, axes, faces, label=0):
    """t_p = w(p) * (s - D*u_p) at the points of flux_points(), in C order: s and D of the library's stencil at sigma = 0
    (D = 6, or the sum of the six face means), gathered at those points only"""
    N = u.shape[0]
    i, j, k = np.nonzero(flux_points(mask, axes, faces, label))
    (im, ip), (jm, jp), (km, kp) = (_neighbours(x, N, axes, faces, ax) for ax, x in enumerate((i, j, k)))
    nb = [(im, j, k), (ip, j, k), (i, jm, k), (i, jp, k), (i, j, km), (i, j, kp)]
    up = u[i, j, k]
    if eps is None:
        s = u[nb[0]] + u[nb[1]]
        for q in nb[2:]:
            s = s + u[q]
        D = 6.0
    else:
        eh = eps[i, j, k]
        a = [0.5 * (eh + eps[q]) for q in nb]
        s = a[0] * u[nb[0]] + a[1] * u[nb[1]]
        for aq, q in zip(a[2:], nb[2:]):
            s = s + aq * u[q]
        D = a[0] + a[1]
        for aq in a[2:]:
            D = D + aq
        D = D + 0.0
    w = (axis_weight(N, axes, faces, 1)[j] * axis_weight(N, axes, faces, 2)[k]) * axis_weight(N, axes, faces, 0)[i]
    return w * (s - D * up)


def flux(u, eps, mask, h, axes, faces, label=0):
    return h * fsum(flux_terms(u, eps, mask, axes, faces, label))


# --------------------------------------------------------------------------------------------------------------- energy
def energy_terms(u, eps, axes, faces):
    """the edge terms (w_e * a_e) * ((u_q - u_p) * (u_q - u_p)): a list of three arrays, the edges along i, j, k.  An edge
    belongs to its lower end p (no duplicate on any axis), runs to x+1 (wrapped from N-2 to 0 on a periodic axis, absent at
    N-1 on another) and is left out when p lies on a Dirichlet face of another axis.  (Every index set but the wrapped upper
    ends is a range, taken as a slice: no copy of a large field.)"""
    N = u.shape[0]
    out = []
    for a in range(3):
        sl, wv = [None] * 3, [None] * 3
        for b in range(3):
            if b == a:
                sl[b], wv[b] = slice(0, N - 1), np.ones(N - 1)
                continue
            keep = ~on_dirichlet(N, axes, faces, b)
            if per(axes, b):
                keep[N - 1] = False  # p is no duplicate
            x = np.nonzero(keep)[0]
            sl[b] = slice(x[0], x[-1] + 1)
            wv[b] = axis_weight(N, axes, faces, b)[sl[b]]
        P = tuple(sl)
        upper = slice(1, N)
        wrap = list(range(1, N - 1)) + [0]

        def ends(f):
            fp = f[P]
            if per(axes, a):
                others = tuple(slice(None) if b == a else sl[b] for b in range(3))
                return fp, np.take(f[others], wrap, axis=a)
            return fp, f[tuple(upper if b == a else sl[b] for b in range(3))]

        up, uq = ends(u)
        du = uq - up
        du *= du
        we = None
        if any((w != 1.0).any() for w in wv):
            we = _outer(*wv)
        if eps is not None:
            ep, eq = ends(eps)
            ae = 0.5 * (ep + eq)
            we = ae if we is None else we * ae
        if we is not None:  # (w_e * a_e) * (du * du); w_e = a_e = 1: the square itself
            du *= we
        out.append(du)
    return out


def energy(u, eps, h, axes, faces):
    return 0.5 * h * fsum(*energy_terms(u, eps, axes, faces))


# ------------------------------------------------------------------------------------- launch geometry of the two sums
WAVE, ROWS, CHUNK = 64, 4, 16


def _grid(nk, nj, planes, cap):
    gx, gy, chunk = -(-nk // WAVE), -(-nj // ROWS), CHUNK
    while gx * gy * -(-planes // chunk) > cap:
        chunk *= 2
    return gx, gy, -(-planes // chunk), chunk


def flux_grid(N, axes, faces, cap):
    """(gx, gy, gz, planes per block) of the flux launch: the unknowns of each axis over (64, 4) blocks, 16 planes per
    block, doubled until the partial sums fit under `cap` (column_grid of csrc/mg3d_kernels.hip)"""
    n = [int(unknown_axis(N, axes, faces, ax).sum()) for ax in range(3)]
    return _grid(n[2], n[1], n[0], cap)


def energy_grid(N, cap):
    """... of the energy launch: all N indices of every axis"""
    return _grid(N, N, N, cap)


# the sizes the sums are tested at, and the one past the cap of partial sums: 545 = 17 * 32 + 1 (c = 18, L = 6) is the
# smallest size with c <= 18 whose flux AND energy launches exceed MG3D_MAX_PARTIALS blocks at 16 planes per block
# (tests/test_field_ref_host.py derives that from the header)
SUM_SIZES = (17, 33, 37, 65)
CAP_SIZE = 545
