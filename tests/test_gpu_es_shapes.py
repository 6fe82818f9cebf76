"""csrc/mg3d_es.hip -- the mixed-boundary ("electrospray") path -- at the launch shapes and parameters that
tests/test_electrospray.py never reaches, against its statement oracle/mg3d_oracle_es.c (plain C, one thread):

- es_color_kernel with live lanes in a second 64-lane block in k (a lane owns the k-pair (2m, 2m+1): from 131^3 on; 145^3
  has 8 such lanes and 161^3 has 16, 129^3 launches the block with none), the k tail and the copy onto k = N-1 from there;
- es_fill_kernel where its later blocks write, and with a capillary potential other than 0;
- parameter sets off the default (_oracle.es_params): "wide" puts patch points on the rows next to the walls and on the
  face edges, "lattice" meets rr <= Rc^2 and Ri^2 < rr < Ro^2 with equality in exact arithmetic;
- random data at EVERY point -- walls, edges and corners too -- on every level, not only the finest;
- after a cycle u, d and r of every level, which shows the ghost-only launch behind the direct solve and the scale-0
  fill of the coarse levels;
- norms against the exactly rounded sum at the project's summation tolerance, a second batch of norms (more than
  sumsq_slots - 1 = 1023 cycles in one call), and the set-up behind a plain cycle that has run ahead.

Grid values bit for bit, sign of zero included.  tests/test_es_host.py holds the case tables and asserts without a GPU
that each set and size reaches what it is here for."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  before the package, as bench.py does: the HIP runtime is torch's

import _oracle as O
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U

from test_es_host import BATCH, BEHIND, FILL, ONE_CYCLE, SMOOTH_LOWER, SMOOTH_TOP, THREE_CYCLES

gpu = pytest.mark.gpu
SUM_RTOL = 1e-13  # a device reduction against the exactly rounded sum (tests/test_gpu_parity.py: EXACT_NORM_RTOL)
_SMOOTH = ((0, 1), (1, 1), (0, 2), (1, 3))  # (post, iters)


def _same_bits(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _plus_zero(a):
    a = np.asarray(a)
    return not a.any() and not np.signbit(a).any()


def _n(c, L):
    return O.level_sizes(c, L)[-1]


def _solver(c, L, nu, pm):
    import multigrid_parallel_amd as M
    return M.Solver(c, L, nu, grid_length=pm.length)


@functools.lru_cache(maxsize=None)
def _edges(N):
    """the twelve edges and eight corners of an N^3 grid, flat bool: points on two faces or more"""
    x = np.zeros(N, dtype=int)
    x[[0, N - 1]] = 1
    return ((x[:, None, None] + x[None, :, None] + x[None, None, :]) >= 2).reshape(-1)


def _random_fields(n, h, seed):
    """u and d random at every point of an n^3 level; d scaled by 1 / h^2 so that h^2 d is O(1) like u"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n ** 3), rng.standard_normal(n ** 3) / (h * h)


def _norm_ok(got, exact):
    print(f"norm {got!r} exact {exact!r} rel {abs(got - exact) / exact if exact else 0.0:.3e}")
    return abs(got - exact) <= SUM_RTOL * exact


def _smooth_level(s, po, l, n, h, seed):
    """es_smooth on level l from random u and d for every (post, iters) against orc_es_smooth"""
    v, d = _random_fields(n, h, seed)
    assert s.level_n(l) == n and s.level_h(l) == h
    edges = _edges(n)
    for post, iters in _SMOOTH:
        s.upload(MG3D_U, l, v)
        s.upload(MG3D_D, l, d)
        s.es_smooth(l, post, iters)
        want = v.copy()
        O.lib().orc_es_smooth(O.P(want), O.P(d), n, h, post, iters, C.byref(po))
        assert np.isfinite(want).all()
        assert _same_bits(want[edges], v[edges]) and not _same_bits(want[~edges], v[~edges])  # (the statement's own)
        got = s.download(MG3D_U, l).reshape(-1)
        assert _same_bits(got[edges], v[edges]), f"level {l} ({n}^3), post {post}, iters {iters}: an edge or corner was written"
        assert _same_bits(got, want), f"level {l} ({n}^3), post {post}, iters {iters}"
        assert _same_bits(s.download(MG3D_D, l), d), f"level {l}: d was written"


# ----------------------------------------------------------------------------------- 1 the smoother, finest level
@gpu
@pytest.mark.parametrize("name", O.ES_SETS)
@pytest.mark.parametrize("c,L", SMOOTH_TOP)
def test_smoother_finest_level(c, L, name):
    """es_color_kernel<true> at 33, 65, 129, 145 and 161 cubed with every parameter set: pre and post order, one to three
    iterations; the edges and corners keep the uploaded bits"""
    N = _n(c, L)
    po, pm = O.es_params(name, N)
    with _solver(c, L, 2, pm) as s:
        s.es_setup(pm)
        _smooth_level(s, po, L - 1, N, po.length / (N - 1), 1000 * N + len(name))


# ----------------------------------------------------------------------------------- 2 the smoother, lower levels
@gpu
@pytest.mark.parametrize("name", ["wide", "lattice"])
@pytest.mark.parametrize("c,L", SMOOTH_LOWER)
def test_smoother_lower_levels(c, L, name):
    """every level below the finest with its own h: the patches change their discrete shape from level to level (and the
    even size 10^3 of (10, 5) has no grid point in the centre of a face)"""
    N = _n(c, L)
    po, pm = O.es_params(name, N)
    sizes = O.level_sizes(c, L)
    with _solver(c, L, 2, pm) as s:
        s.es_setup(pm)
        for l in range(L - 1):
            n = sizes[l]
            _smooth_level(s, po, l, n, po.length / (n - 1), 1000 * n + l)


# ------------------------------------------------------------------------------------------ 3 the fill of the set-up
@gpu
@pytest.mark.parametrize("name", ["wide", "lattice"])
@pytest.mark.parametrize("c,L", FILL)
def test_setup_fills_the_finest_level_only(c, L, name):
    """after es_setup the finest u is orc_es_fill of zeros -- 75 V on the disc of x = 0, which a fill that skipped that
    face or dropped `scale` times the potential would miss -- and every other array of the hierarchy is +0. everywhere"""
    N = _n(c, L)
    po, pm = O.es_params(name, N)
    h = po.length / (N - 1)
    want = np.zeros(N ** 3)
    O.lib().orc_es_fill(O.P(want), N, h, C.byref(po), 1.0)
    x0, xl = O.es_patches(po, N, h)
    W = want.reshape(N, N, N)
    assert np.all(W[0][x0] == 75.0) and x0.sum() > 50 and np.all(W[-1][xl] == -1350.0) and xl.sum() > 50
    assert _plus_zero(W[0][~x0]) and _plus_zero(W[-1][~xl]) and _plus_zero(W[1:-1])
    rng = np.random.default_rng(N)
    with _solver(c, L, 2, pm) as s:
        for l in range(L):  # the set-up clears what it finds
            for f in (MG3D_U, MG3D_D, MG3D_R):
                s.upload(f, l, rng.standard_normal(s.level_n(l) ** 3))
        s.es_setup(pm)
        assert _same_bits(s.download(MG3D_U, L - 1), want)
        for l in range(L):
            for f, what in ((MG3D_U, "u"), (MG3D_D, "d"), (MG3D_R, "r")):
                if (f, l) != (MG3D_U, L - 1):
                    assert _plus_zero(s.download(f, l)), f"{what} of level {l}"


# -------------------------------------------------------------------------------------- 4 one cycle, every level
@gpu
@pytest.mark.parametrize("name", O.ES_SETS)
@pytest.mark.parametrize("c,L,nu", ONE_CYCLE)
def test_every_level_after_one_cycle(c, L, nu, name):
    """u, d and r of every level after es_vcycles(1) against orc_es_vcycle driven on a Hierarchy -- every point, the faces
    of r included (both sides leave them at the zeros of the set-up).  Level 0 shows the ghost-only launch behind the
    direct solve, the levels between the scale-0 fill"""
    N = _n(c, L)
    po, pm = O.es_params(name, N)
    h = po.length / (N - 1)
    H = O.Hierarchy(c, L)
    O.lib().orc_es_fill(O.P(H.u[-1]), N, h, C.byref(po), 1.0)
    LU = O.es_factor(c, h * (1 << (L - 1)), po)
    want = O.es_vcycle(H, nu, LU, po)
    for l in range(L):
        assert np.isfinite(H.u[l]).all() and np.isfinite(H.d[l]).all() and np.isfinite(H.r[l]).all()
        assert H.u[l].any() and (l == L - 1 or H.d[l].any()) and (l == 0 or H.r[l].any())
    assert _plus_zero(H.d[-1]) and _plus_zero(H.r[0])
    with _solver(c, L, nu, pm) as s:
        s.es_setup(pm)
        got = s.es_vcycles(1)
        for l in range(L):
            assert _same_bits(s.download(MG3D_U, l), H.u[l]), f"u level {l}"
            assert _same_bits(s.download(MG3D_D, l), H.d[l]), f"d level {l}"
            assert _same_bits(s.download(MG3D_R, l), H.r[l]), f"r level {l}"
    assert np.isfinite(want)
    assert _norm_ok(got[0], O.exact_residual_norm(H.u[-1], H.d[-1], N, h))


# ------------------------------------------------------------------------------------ 5 three cycles in one call
@functools.lru_cache(maxsize=None)
def _run(c, L, nu, cycles, name):
    """O.es_run of a named set, shared and left unchanged: (norms, u), finite"""
    po, _ = O.es_params(name, _n(c, L))
    norms, u, _ = O.es_run(c, L, nu, cycles, po)
    assert np.isfinite(norms).all() and np.isfinite(u).all(), (c, L, name, cycles)
    u.setflags(write=False)
    return norms, u


def _exact_norm_after(c, L, nu, cycles, name):
    N = _n(c, L)
    po, _ = O.es_params(name, N)
    return O.exact_residual_norm(_run(c, L, nu, cycles, name)[1], np.zeros(N ** 3), N, po.length / (N - 1))


@gpu
@pytest.mark.parametrize("c,L,name", THREE_CYCLES)
def test_three_cycles_in_one_call(c, L, name):
    """es_vcycles(3): the finest u, each norm against the exactly rounded sum of the statement's u after that cycle; and
    es_vcycles(2) followed by es_vcycles(1) has the same bits"""
    N, nu = _n(c, L), 2
    _, pm = O.es_params(name, N)
    _, want_u = _run(c, L, nu, 3, name)
    with _solver(c, L, nu, pm) as s, _solver(c, L, nu, pm) as t:
        s.es_setup(pm)
        got = s.es_vcycles(3)
        u = s.download(MG3D_U, L - 1)
        assert _same_bits(u, want_u)
        assert _plus_zero(s.download(MG3D_D, L - 1))
        t.es_setup(pm)
        split = list(t.es_vcycles(2)) + list(t.es_vcycles(1))
        assert _same_bits(t.download(MG3D_U, L - 1), u)
        assert np.array_equal(split, got)
    for k in range(3):
        assert _norm_ok(got[k], _exact_norm_after(c, L, nu, k + 1, name)), k


# ---------------------------------------------------------------------------------------- 6 a second batch of norms
@gpu
@pytest.mark.parametrize("name", ["default", "lattice"])
def test_second_norm_batch(name):
    """17^3, 1025 cycles in one call: mg3d_es_vcycles reads the norms back once per 1023 cycles, so cycles 1024 and 1025
    reuse slots 0 and 1"""
    c, L = BATCH
    N, nu, cycles = _n(c, L), 2, 1025
    _, pm = O.es_params(name, N)
    _, want_u = _run(c, L, nu, cycles, name)
    with _solver(c, L, nu, pm) as s:
        s.es_setup(pm)
        got = s.es_vcycles(cycles)
        assert _same_bits(s.download(MG3D_U, L - 1), want_u)
    assert len(got) == cycles and np.isfinite(got).all()
    for k in (1, 1023, 1024, 1025):
        assert _norm_ok(got[k - 1], _exact_norm_after(c, L, nu, k, name)), k


# --------------------------------------------------------------------------- 7 behind a cycle that has run ahead
@gpu
def test_setup_behind_a_cycle_that_has_run_ahead():
    """161^3: the plain problem's vcycle() ends ahead of itself (one launch per leg, as tests/test_gpu_field.py relies
    on); es_setup and two cycles on that context have the bits of a fresh context and of the statement"""
    c, L = BEHIND
    N, nu, q = _n(c, L), 2, L - 1
    _, pm = O.es_params("wide", N)
    _, want_u = _run(c, L, nu, 2, "wide")
    rng = np.random.default_rng(161)
    with _solver(c, L, nu, pm) as a, _solver(c, L, nu, pm) as b:
        a.get_details()
        a.upload(MG3D_U, q, rng.uniform(-1, 1, N ** 3))
        a.upload(MG3D_D, q, rng.uniform(-1, 1, N ** 3))
        a.timing_enable(1)
        a.timing_reset()
        a.vcycle()
        assert (q, "leg_up") in a.kernel_times()  # the schedule that runs ahead did run
        for s in (a, b):
            s.es_setup(pm)
        na, nb = a.es_vcycles(2), b.es_vcycles(2)
        ua = a.download(MG3D_U, q)
        assert _same_bits(ua, b.download(MG3D_U, q)) and np.array_equal(na, nb)
        assert _same_bits(ua, want_u)
        for l in range(L):
            for f in (MG3D_U, MG3D_D, MG3D_R):
                assert _same_bits(a.download(f, l), b.download(f, l)), (f, l)
    for k in range(2):
        assert _norm_ok(na[k], _exact_norm_after(c, L, nu, k + 1, "wide")), k
