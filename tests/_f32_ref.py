"""What the binary32 / damped-Jacobi variant is held to on random data: V-cycles of its CPU restatement
(oracle/mg3d_oracle_f32.c, orc32_vcycle) on caller-supplied hierarchies, recorded level by level, and the operator
comparison shared by tests/test_gpu_f32.py and tests/test_gpu_f32_random.py.  Test infrastructure only."""
import ctypes as C
import os
from collections import OrderedDict

import numpy as np
import pytest

import _oracle as O

OMEGA = 6.0 / 7.0
CACHE_BYTES = 1 << 30  # least recently used runs leave first (three cycles at 289^3 hold 0.37 GB)
_cache = OrderedDict()


def rnd(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, n ** 3).astype(np.float32)


def same_bits(a, b):
    """equal values and equal signs of zero (tests/test_gpu_wpcg._same_bits)"""
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def first_difference(got, want, N, level):
    """Where two fields of one level part first, with the tile coordinates of the fused fp32 launches: k-tile and column
    in it (248 columns a tile), row in the 12-row and in the 10-row j-tile."""
    g, w = got.view(np.uint32), want.view(np.uint32)
    bad = np.flatnonzero(g != w)
    if bad.size == 0:
        return f"level {level} ({N}^3): same bits"
    p = int(bad[0])
    i, j, k = p // (N * N), (p // N) % N, p % N
    return (f"level {level} ({N}^3): {bad.size} points differ, first at (i, j, k) = ({i}, {j}, {k}): got {got[p]!r}, want {want[p]!r}; "
            f"k // 248 = {k // 248}, k % 248 = {k % 248}, j % 12 = {j % 12}, j % 10 = {j % 10}")


def assert_same_bits(got, want, N, level, what):
    assert same_bits(got, want), f"{what}: {first_difference(got, want, N, level)}"


def exact_residual_norm32(u, d, N, hd):
    """sqrt of the EXACTLY ROUNDED sum of the squared binary32 residuals of (u, d): the residual field from the
    restatement (bit-identical to the GPU's diffs whenever u and d are), each square in double (a binary32 squared is
    exact there), the sum in extended precision.  It differs from the GPU's number by the GPU's summation order only;
    the restatement's own return value is a sequential double sum with up to n 2^-53 of rounding error."""
    res = np.zeros(N ** 3, dtype=np.float32)
    O.lib().orc32_residual(O.PF(np.ascontiguousarray(u)), O.PF(np.ascontiguousarray(d)), N, np.float32(hd), O.PF(res))
    total = np.longdouble(0)
    step = 1 << 22
    for a in range(0, res.size, step):
        sq = res[a:a + step].astype(np.float64)
        total += np.sum((sq * sq).astype(np.longdouble))
    return float(np.sqrt(total))


def coarse_lu(c, L, grid_length=1.0):
    """the coarsest level's factors with the coarsest spacing, as orc32_run_problem builds them"""
    lib = O.lib()
    N = O.level_sizes(c, L)[-1]
    n0 = c ** 3
    LU = np.zeros(n0 * n0)
    lib.orc_coarse_matrix(O.P(LU), c, (grid_length / (N - 1)) * (1 << (L - 1)))
    lib.orc_lu_factor(O.P(LU), n0)
    return LU


class Cycle:
    """the state behind one V-cycle: the top u, u and d of every level below it, the exactly rounded norm"""

    def __init__(self, u_top, u_low, d_low, norm):
        self.u_top, self.u_low, self.d_low, self.norm = u_top, u_low, d_low, norm

    def nbytes(self):
        return self.u_top.nbytes + sum(a.nbytes for a in self.u_low) + sum(a.nbytes for a in self.d_low)


def run_cycles(c, L, nu, cycles, u0, d0, r0, grid_length=1.0):
    """`cycles` V-cycles of the restatement from (u0, d0, r0) on the top level and zeros below: a list of Cycle"""
    lib = O.lib()
    sizes = O.level_sizes(c, L)
    N, top = sizes[-1], L - 1
    u = [np.zeros(n ** 3, dtype=np.float32) for n in sizes]
    d = [np.zeros(n ** 3, dtype=np.float32) for n in sizes]
    r = [np.zeros(n ** 3, dtype=np.float32) for n in sizes]
    s = [np.zeros(n ** 3, dtype=np.float32) for n in sizes]
    u[top][:], d[top][:], r[top][:] = u0, d0, r0
    ptrs = [(O.fp * L)(*[O.PF(a) for a in xs]) for xs in (u, d, r, s)]
    LU = coarse_lu(c, L, grid_length)
    hd = grid_length / (N - 1)
    out = []
    # the sweeps are pointwise (any thread count gives the same bits); everything else of the restatement is serial
    lib.orc_set_threads(min(8, len(os.sched_getaffinity(0))))
    try:
        for _ in range(cycles):
            lib.orc32_vcycle(*ptrs, hd, top, nu, C.c_float(OMEGA), N, O.P(LU))
            out.append(Cycle(u[top].copy(), [a.copy() for a in u[:top]], [a.copy() for a in d[:top]],
                             exact_residual_norm32(u[top], d[top], N, hd)))
    finally:
        lib.orc_set_threads(1)
    return out


def random_start(c, L, seed):
    N = O.level_sizes(c, L)[-1]
    return rnd(N, seed), rnd(N, seed + 1), rnd(N, seed + 2)


def random_cycles(c, L, nu, cycles, seed, grid_length=1.0):
    """run_cycles from seeded uniform(-1, 1) u, d and r on the top level; one CPU run per (c, L, nu, cycles, seed).
    The results are shared: nobody writes to them."""
    key = (c, L, nu, cycles, seed, grid_length)
    if key in _cache:
        _cache.move_to_end(key)
        return _cache[key]
    out = run_cycles(c, L, nu, cycles, *random_start(c, L, seed), grid_length)
    for cyc in out:
        for a in [cyc.u_top] + cyc.u_low + cyc.d_low:
            a.flags.writeable = False
    _cache[key] = out
    while len(_cache) > 1 and sum(cyc.nbytes() for v in _cache.values() for cyc in v) > CACHE_BYTES:
        _cache.popitem(last=False)
    return out


def check_operators(c, L, sweeps, sequential_norm, grid_length=1.0, d_scale=1.0):
    """Every stand-alone operator of Solver32 on the top level of (c, L) against the restatement, on seeded random
    fields, bit for bit.  The residual's norm is held to the exactly rounded sum; with `sequential_norm` also to the
    restatement's own (sequentially summed) return value, which only small levels can meet at 1e-12.  grid_length: the
    box both sides are created for; d_scale: d is uniform(-1, 1) times this (1 / grid_length^2 keeps h^2 d in sight of u)."""
    import multigrid_parallel_amd as M
    from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U
    lib = O.lib()
    with M.Solver32(c, L, 2, OMEGA, grid_length) as s:
        top = L - 1
        N, Nc = s.level_n(top), s.level_n(top - 1)
        hd = grid_length / (N - 1)
        h = np.float32(hd)
        u, d = rnd(N, 1), (rnd(N, 2) * np.float32(d_scale)).astype(np.float32)
        s.upload(MG3D_U, top, u)
        s.upload(MG3D_D, top, d)
        # smoother: the sweep counts exercise both buffer parities, pairs and pair + single
        for iters in sweeps:
            s.upload(MG3D_U, top, u)
            s.smooth(top, iters)
            want, scratch = u.copy(), np.zeros_like(u)
            lib.orc32_smooth(O.PF(want), O.PF(d), O.PF(scratch), N, h, np.float32(OMEGA), iters)
            got = s.download(MG3D_U, top)
            assert np.array_equal(got, want), f"{iters} sweeps: {first_difference(got, want, N, top)}"
        # residual + norm
        r0 = rnd(N, 3)
        s.upload(MG3D_R, top, r0)
        got_norm = s.residual(top, store=True)
        want_r = r0.copy()
        want_norm = lib.orc32_residual(O.PF(want), O.PF(d), N, h, O.PF(want_r))
        got_r = s.download(MG3D_R, top)
        assert np.array_equal(got_r, want_r), first_difference(got_r, want_r, N, top)  # boundary of r untouched
        if sequential_norm:
            assert got_norm == pytest.approx(want_norm, rel=1e-12)
        exact = exact_residual_norm32(want, d, N, hd)
        print(f"operators ({c},{L}) {N}^3: residual norm / exactly rounded - 1 = {got_norm / exact - 1:.3e}")
        assert got_norm == pytest.approx(exact, rel=1e-12)
        # restriction
        s.restrict(top)
        want_dc = np.zeros(Nc ** 3, dtype=np.float32)
        lib.orc32_restrict(O.PF(want_r), N, O.PF(want_dc), Nc)
        got_dc = s.download(MG3D_D, top - 1)
        assert np.array_equal(got_dc, want_dc), first_difference(got_dc, want_dc, Nc, top - 1)
        # prolongation
        ec = rnd(Nc, 4)
        s.upload(MG3D_U, top - 1, ec)
        s.prolong(top)
        lib.orc32_prolong(O.PF(ec), Nc, O.PF(want), N)
        got = s.download(MG3D_U, top)
        assert np.array_equal(got, want), first_difference(got, want, N, top)
        # boundary fill
        s.zero(MG3D_U, top)
        s.fill_boundary(MG3D_U, top)
        want_b = np.zeros(N ** 3, dtype=np.float32)
        lib.orc32_fill_boundary(O.PF(want_b), N, hd)
        assert np.array_equal(s.download(MG3D_U, top), want_b)
        # coarsest solve through double
        n0 = c ** 3
        b0 = rnd(c, 5)
        s.upload(MG3D_D, 0, b0)
        s.coarse_solve()
        want_x = np.zeros(n0, dtype=np.float32)
        lib.orc32_coarse_solve(O.P(coarse_lu(c, L, grid_length)), n0, O.PF(b0), O.PF(want_x))
        assert np.array_equal(s.download(MG3D_U, 0), want_x)
