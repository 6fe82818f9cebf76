"""Fixed points inside the domain (mg3d_ctx_set_mask) on the GPU, against the numpy restatement tests/_mask_ref.py: the
single operators, the launch tails of the MASK kernels, cycles, the solvers, the time stepper, the setters in every
order, the refusals and the device form.  Grid values bit for bit unless said otherwise; norms to the summation tolerance
of tests/test_gpu_neumann.py (test_gpu_parity.norm_rtol); the iterates and norms of mg3d_pcg_solve to the tolerance of
tests/test_gpu_pcg.py and those of mg3d_wpcg_solve to that of tests/test_gpu_wpcg.py: 100 x the summation spread each file
measured on the CPU.  One figure here is the masked problems' own, measured the same way (python tests/_mask_ref.py: two
restatement runs, exactly rounded dots against numpy's pairwise sums): on exact problem (b) the recurrence norm falls by
4e6 in five iterations and the two runs differ in it by 7.57e-11 at k = 5 (problem (a) 2.94e-14, the sphere 6.57e-15; the
iterates by at most 3.4e-16 everywhere) -- above both files' norm figures, so (b)'s norms are held to 100 x 7.57e-11.  Each mask is random at 10 % density plus a solid block plus a one-point-thick odd plate
(_mask_ref.gpu_test_mask) unless the test is about one body."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch  # before the package, as bench.py does: the HIP runtime is torch's

import _coef_ref as CR
import _mask_ref as MR
import _neumann_ref as NR
import _step_ref as SR
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U, MG3D_F64, MG3D_U8, mg3d_array

from test_gpu_parity import norm_rtol
import test_gpu_pcg as TP
import test_gpu_wpcg as TW

pytestmark = pytest.mark.gpu

MG3D_ERR_ARG, MG3D_ERR_STATE = 1, 5
# per entry point: the spread of the iterate x_k by k and of the norms, as its own test file measured them
SPREAD = {"pcg_solve": (TP.SPREAD_U, TP.SPREAD_NORM), "wpcg_solve": (TW.SPREAD_U, TW.SPREAD_NORM)}
SPREAD_NORM_EXACT_B = 7.57e-11  # measured on the masked problem itself, see above
# all Dirichlet; periodic mask 5; Neumann ILO | JHI; periodic k + Neumann on both i faces
BOUNDARIES = [(0, 0), (5, 0), (0, 1 | 8), (4, 3)]


def _same_bits(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _n(c, L):
    return (c - 1) * (1 << (L - 1)) + 1


def _eps(N):
    return CR.FIELDS["exp"](N)


def _solver(c, L, nu, sigma, eps, axes, faces, mask, factor=True):
    s = M.Solver(c, L, nu)
    s.set_shift(sigma)
    s.set_periodic(axes)
    s.set_neumann(faces)
    if eps is not None:
        s.set_coefficient(eps)
    if mask is not None:
        s.set_mask(mask)
    if factor:
        s.get_details()
    return s


def _random_problem(ref, rng):
    N = ref.N[-1]
    ref.u[-1][...] = rng.standard_normal((N, N, N))
    ref.d[-1][...] = rng.standard_normal((N, N, N))
    NR.refresh(ref.u[-1], ref.axes)
    NR.refresh(ref.d[-1], ref.axes)


def _upload(s, ref):
    s.upload(MG3D_U, ref.L - 1, ref.u[-1])
    s.upload(MG3D_D, ref.L - 1, ref.d[-1])


def _assert_levels(s, ref):
    for l in range(ref.L):
        assert _same_bits(s.download(MG3D_U, l), ref.u[l]), f"u level {l}"
    for l in range(ref.L - 1):
        assert _same_bits(s.download(MG3D_D, l), ref.d[l]), f"d level {l}"


# ------------------------------------------------------------------------------------------------- 1 single operators
@pytest.mark.parametrize("axes,faces", BOUNDARIES)
@pytest.mark.parametrize("sigma", [0.0, 3.5])
@pytest.mark.parametrize("field", ["const", "eps"])
def test_single_operators(axes, faces, sigma, field):
    """smooth (pre, post), residual (with and without r), restrict, prolong, coarse_solve at 17^3 on random data; u at
    the fixed points unchanged bitwise, r there 0., d there poisoned with NaN: never read"""
    c, L = 5, 3
    N = _n(c, L)
    eps = _eps(N) if field == "eps" else None
    mask = MR.gpu_test_mask(N)
    ref = MR.Hierarchy(c, L, 2, sigma, eps, axes, faces, mask)
    rng = np.random.default_rng(11 + faces + 64 * axes)
    with _solver(c, L, 2, sigma, eps, axes, faces, mask) as s:
        assert s.has_mask()
        for l in range(L):
            assert np.array_equal(s.get_mask(l), ref.mask[l]), f"the injected mask of level {l}"
        for l in (L - 1, L - 2):
            n, h, e, m = s.level_n(l), s.level_h(l), ref.e(l), ref.mask[l]
            fx = ref.fixed(l)
            assert fx.any()
            u, d = rng.standard_normal((n, n, n)), rng.standard_normal((n, n, n))
            d[fx] = np.nan
            NR.refresh(u, axes)
            u_in = u.copy()
            s.upload(MG3D_U, l, u)
            s.upload(MG3D_D, l, d)
            s.smooth(l, 0, 2)
            MR.pre_smooth(u, d, e, h, sigma, axes, faces, 2, m)
            assert _same_bits(s.download(MG3D_U, l), u), f"pre-smoothing, level {l}"
            s.smooth(l, 1, 1)
            MR.post_smooth(u, d, e, h, sigma, axes, faces, 1, m)
            got_u = s.download(MG3D_U, l).reshape(n, n, n)
            assert _same_bits(got_u, u), f"post-smoothing, level {l}"
            assert _same_bits(got_u[fx], u_in[fx]) and np.isfinite(got_u).all()
            r = rng.standard_normal((n, n, n))
            r_in = r.copy()
            s.upload(MG3D_R, l, r)
            norm_only = s.residual(l, store=False)
            assert _same_bits(s.download(MG3D_R, l), r_in), "the norm-only residual writes no r"
            got = s.residual(l, store=True)
            MR.residual(u, d, e, h, sigma, axes, faces, m, r)
            got_r = s.download(MG3D_R, l).reshape(n, n, n)
            assert _same_bits(got_r, r), f"residual, level {l}"
            assert not got_r[fx].any() and not np.signbit(got_r[fx]).any()
            assert got == norm_only
            exact = MR.exact_residual_norm(u, d, e, h, sigma, axes, faces, m)
            assert abs(got - exact) <= norm_rtol(n) * exact, (got, exact)
            nc = s.level_n(l - 1)
            dc = rng.standard_normal((nc, nc, nc))
            s.upload(MG3D_D, l - 1, dc)
            s.restrict(l)
            NR.restrict(r, dc, axes, faces)  # (unchanged: it reads the zeros the residual stored)
            assert _same_bits(s.download(MG3D_D, l - 1), dc), f"restrict, level {l}"
            ec = rng.standard_normal((nc, nc, nc))
            NR.refresh(ec, axes)
            s.upload(MG3D_U, l - 1, ec)
            before = u.copy()
            s.prolong(l)
            MR.prolong(ec, u, axes, faces, m)
            got_u = s.download(MG3D_U, l).reshape(n, n, n)
            assert _same_bits(got_u, u), f"prolong, level {l}"
            assert _same_bits(got_u[fx], before[fx])
        n0 = s.level_n(0)
        d0 = rng.standard_normal((n0, n0, n0))
        s.upload(MG3D_D, 0, d0)
        s.coarse_solve()
        u0 = np.zeros((n0, n0, n0))
        MR.coarse_solve(ref.LU, d0, u0, axes, faces, sigma, ref.mask[0])
        got0 = s.download(MG3D_U, 0).reshape(n0, n0, n0)
        assert _same_bits(got0, u0)
        assert not got0[ref.fixed(0)].any(), "a fixed point of level 0 holds the zero error"
        assert _same_bits(s.download(MG3D_D, 0), d0), "the direct solve leaves d of level 0 alone"


# ------------------------------------------------------------------------------------------------------ 2 launch tails
@pytest.mark.parametrize("c,axes", [(18, 0), (19, 7)])
@pytest.mark.parametrize("field", ["const", "eps"])
def test_launch_tails(c, axes, field):
    """the colour pass and the residual at 69^3 (all Dirichlet) and 73^3 (periodic): a partial last row group, several
    16-plane chunks and, for the column kernels (the residual and the eps colour pass), two k-blocks of 64 lanes; the
    constant colour pass, whose lanes own k-pairs, has one k-block of 35 or 37 pairs here (two from 65 pairs on:
    tests/test_gpu_mask_shapes.py).  Fixed points at the first and last unknown of a row, a column and a chunk.
    (No coarse factor: c^3 unknowns are too many for a dense one, and these entry points need none.)"""
    L, sigma = 3, 3.5
    N = _n(c, L)
    assert N in (69, 73)
    eps = _eps(N) if field == "eps" else None
    lo, hi = NR.lo_hi(N, axes, 0, 0)
    mask = MR.gpu_test_mask(N)
    ends = [lo, lo + 1, hi - 1, hi]
    chunk_i = sorted({lo + 15, lo + 16, lo + 17, lo + 31, lo + 32, hi - ((hi - lo) % 16), hi})
    lanes = sorted({lo + 62, lo + 63, lo + 64, lo + 65, hi})
    for i, j, k in itertools.product(ends + chunk_i, ends, ends + lanes):
        mask[i, j, k] = 1
    for i, j, k in itertools.product(ends, ends + [hi - 3, hi - 4], ends):
        mask[i, j, k] = 1
    rng = np.random.default_rng(N)
    u, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    NR.refresh(u, axes)
    m = MR.stored(mask, axes)
    fx = MR.fixed(m, axes, 0)
    u_in = u.copy()
    with _solver(c, L, 1, sigma, eps, axes, 0, mask, factor=False) as s:
        h = s.level_h(L - 1)
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        s.smooth(L - 1, 0, 1)
        MR.pre_smooth(u, d, eps, h, sigma, axes, 0, 1, m)
        got_u = s.download(MG3D_U, L - 1).reshape(N, N, N)
        assert _same_bits(got_u, u)
        assert _same_bits(got_u[fx], u_in[fx])
        r = np.zeros((N, N, N))
        s.zero(MG3D_R, L - 1)
        got = s.residual(L - 1, store=True)
        MR.residual(u, d, eps, h, sigma, axes, 0, m, r)
        got_r = s.download(MG3D_R, L - 1).reshape(N, N, N)
        assert _same_bits(got_r, r) and not got_r[fx].any()
        exact = MR.exact_residual_norm(u, d, eps, h, sigma, axes, 0, m)
        assert abs(got - exact) <= norm_rtol(N) * exact, (got, exact)


# ------------------------------------------------------------------------------------------------------------ 3 cycles
@pytest.mark.parametrize("c,L", [(5, 3), (5, 4)])
@pytest.mark.parametrize("axes,faces", BOUNDARIES)
@pytest.mark.parametrize("field,sigma", [("const", 0.0), ("eps", 3.5)])
def test_cycles(c, L, axes, faces, field, sigma):
    """mg3d_vcycle, then mg3d_vcycles(3): u of every level, d below the top, the norms -- 17^3 and 33^3"""
    N = _n(c, L)
    eps = _eps(N) if field == "eps" else None
    mask = MR.gpu_test_mask(N)
    ref = MR.Hierarchy(c, L, 2, sigma, eps, axes, faces, mask)
    _random_problem(ref, np.random.default_rng(N + faces + 64 * axes))
    u_in = ref.u[-1].copy()
    with _solver(c, L, 2, sigma, eps, axes, faces, mask) as s:
        _upload(s, ref)
        want = ref.vcycles(4)
        got = [s.vcycle()] + list(s.vcycles(3))
        _assert_levels(s, ref)
        fx = ref.fixed()
        assert _same_bits(s.download(MG3D_U, L - 1).reshape(N, N, N)[fx], u_in[fx])
    np.testing.assert_allclose(got, want, rtol=norm_rtol(N))


@pytest.mark.parametrize("axes,faces", BOUNDARIES)
@pytest.mark.parametrize("field", ["const", "eps"])
def test_zero_mask_is_the_context_without_one(axes, faces, field):
    """an all-zero mask: every grid value and norm of the same context without a mask on the unfused kernels, bit for bit
    (a periodic axis, a Neumann face or eps select them).  The all-Dirichlet constant context without a mask runs the
    fused schedules, which no option reaches around: there u is compared bit for bit with that context and with the
    restatement, which states the unfused kernels, and the norms to the summation tolerance"""
    c, L, N = 5, 4, 33
    eps = _eps(N) if field == "eps" else None
    ref = NR.Problem(c, L, 2, 1.5, eps, axes, faces)
    _random_problem(ref, np.random.default_rng(5))
    with _solver(c, L, 2, 1.5, eps, axes, faces, np.zeros(N ** 3, dtype=np.uint8)) as a, \
            _solver(c, L, 2, 1.5, eps, axes, faces, None) as b:
        assert a.has_mask() and not b.has_mask()
        _upload(a, ref)
        _upload(b, ref)
        na, nb = a.vcycles(3), b.vcycles(3)
        for l in range(L):
            assert _same_bits(a.download(MG3D_U, l), b.download(MG3D_U, l))
        if axes or faces or eps is not None:  # the same kernels, the same partial sums
            assert np.array_equal(na, nb)
        else:
            np.testing.assert_allclose(na, nb, rtol=norm_rtol(N))
        ref.vcycles(3)
        assert _same_bits(a.download(MG3D_U, L - 1), ref.u[-1])


@pytest.mark.parametrize("c,L", [(5, 4), (11, 5)])
def test_null_mask_restores_the_fused_schedules(c, L):
    """set_mask(None) after a mask and cycles with it: u, d and the norms of a fresh context, bit for bit -- at 33^3 and at
    161^3, where the fresh context runs one launch per leg"""
    N = _n(c, L)
    assert N in (33, 161)
    rng = np.random.default_rng(N)
    u, d = rng.standard_normal(N ** 3), rng.standard_normal(N ** 3)
    with M.Solver(c, L, 2) as a, M.Solver(c, L, 2) as b:
        a.get_details()
        b.get_details()
        a.set_mask(MR.sphere(N))
        a.upload(MG3D_U, L - 1, u)
        a.upload(MG3D_D, L - 1, d)
        a.vcycles(2)
        a.vcycle()
        a.set_mask(None)
        assert not a.has_mask()
        for s in (a, b):
            s.upload(MG3D_U, L - 1, u)
            s.upload(MG3D_D, L - 1, d)
        na = [a.vcycle(), a.vcycle()] + list(a.vcycles(3))
        nb = [b.vcycle(), b.vcycle()] + list(b.vcycles(3))
        assert na == nb
        assert _same_bits(a.download(MG3D_U, L - 1), b.download(MG3D_U, L - 1))
        assert _same_bits(a.download(MG3D_D, L - 2), b.download(MG3D_D, L - 2))
        with pytest.raises(M.Mg3dError) as ei:
            a.get_mask(0)
        assert ei.value.code == MG3D_ERR_STATE


# ----------------------------------------------------------------------------------------------------------- 4 solvers
_exact_runs = {}


def _exact_run(which):
    """the restatement's solve of a discrete-exact problem to rtol 1e-12, once: (problem, u0, exact, iterates, norms)"""
    if which not in _exact_runs:
        axes, faces, mask, u0, exact = MR.exact_problem(which)
        prob = MR.Hierarchy(5, 3, 2, 0.0, None, axes, faces, mask)
        hist = []
        _, norms, ok, _, _ = MR.wpcg(prob, u0, np.zeros_like(u0), 1e-12, 0.0, 60, history=hist)
        assert ok
        _exact_runs[which] = (prob, mask, u0, exact, hist, norms)
    return _exact_runs[which]


@pytest.mark.parametrize("call", ["pcg_solve", "wpcg_solve"])
@pytest.mark.parametrize("which", ["a", "b"])
def test_solvers_on_the_exact_problems(call, which):
    """u after 1, 2 and 5 iterations to the tolerance of tests/test_gpu_wpcg.py; to rtol 1e-12 the restatement's iteration
    count and the exact discrete solution to 1e-10; the fixed values bitwise.  (b)'s plate is gone from both coarse
    levels: plain cycles grow on it, the Krylov iteration does not care"""
    prob, mask, u0, exact, hist, ref_norms = _exact_run(which)
    N = 17
    with _solver(5, 3, 2, 0.0, None, prob.axes, prob.faces, mask) as s:
        s.upload(MG3D_D, 2, np.zeros(N ** 3))
        for k in (1, 2, 5):
            s.upload(MG3D_U, 2, u0)
            norms, info = getattr(s, call)(rtol=0.0, atol=1e-300, max_iters=k)
            u = s.download(MG3D_U, 2).reshape(N, N, N)
            rel = np.abs(u - hist[k - 1]).max() / np.abs(hist[k - 1]).max()
            nrel = (np.abs(norms - ref_norms[:k + 1]) / ref_norms[:k + 1]).max()
            print(which, call, k, "u", rel, "norms", nrel)
            assert info["iterations"] == k
            su, sn = SPREAD[call]
            if which == "b":
                sn = max(sn, SPREAD_NORM_EXACT_B)
            assert rel <= 100 * su[k] and nrel <= 100 * sn
        s.upload(MG3D_U, 2, u0)
        norms, info = getattr(s, call)(rtol=1e-12, max_iters=60)
        assert info["converged"] and info["iterations"] == len(ref_norms) - 1
        if call == "wpcg_solve":
            assert info["singular"] == 0
        u = s.download(MG3D_U, 2).reshape(N, N, N)
        err = np.abs(u - exact).max()
        print(which, call, "iterations", info["iterations"], "max error", err)
        assert err <= 1e-10
        assert _same_bits(u[mask != 0], u0[mask != 0])
        w = u.copy()
        NR.refresh(w, prob.axes)
        assert _same_bits(u, w), "duplicates differ from their sources"


@pytest.mark.parametrize("call", ["pcg_solve", "wpcg_solve"])
def test_solvers_on_the_sphere(call):
    """a sphere of radius 0.2 held at 1 in a grounded 33^3 box"""
    c, L, N = 5, 4, 33
    mask = MR.sphere(N)
    prob = MR.Hierarchy(c, L, 2, 0.0, None, 0, 0, mask)
    u0 = np.zeros((N, N, N))
    u0[mask != 0] = 1.0
    hist = []
    x, ref_norms, ok, _, _ = MR.wpcg(prob, u0, np.zeros_like(u0), 1e-10, 0.0, 60, history=hist)
    assert ok and len(hist) >= 5
    with _solver(c, L, 2, 0.0, None, 0, 0, mask) as s:
        s.upload(MG3D_D, L - 1, np.zeros(N ** 3))
        for k in (1, 2, 5):
            s.upload(MG3D_U, L - 1, u0)
            norms, info = getattr(s, call)(rtol=0.0, atol=1e-300, max_iters=k)
            u = s.download(MG3D_U, L - 1).reshape(N, N, N)
            rel = np.abs(u - hist[k - 1]).max() / np.abs(hist[k - 1]).max()
            nrel = (np.abs(norms - ref_norms[:k + 1]) / ref_norms[:k + 1]).max()
            print(call, k, "u", rel, "norms", nrel)
            assert rel <= 100 * SPREAD[call][0][k] and nrel <= 100 * SPREAD[call][1]
        s.upload(MG3D_U, L - 1, u0)
        norms, info = getattr(s, call)(rtol=1e-10, max_iters=60)
        assert info["converged"] and info["iterations"] == len(ref_norms) - 1
        u = s.download(MG3D_U, L - 1).reshape(N, N, N)
        assert _same_bits(u[mask != 0], u0[mask != 0])
        assert 0.0 <= u.min() and u.max() <= 1.0  # the discrete maximum principle


def test_one_fixed_point_makes_the_neumann_box_regular():
    """all six faces Neumann, sigma = 0: singular with an all-zero mask (projected, as before), regular with one fixed
    point -- on the finest level only, or surviving down to level 0 (then the pin goes too)"""
    c, L, N = 5, 3, 17
    rng = np.random.default_rng(2)
    d = rng.standard_normal((N, N, N))
    u0 = np.zeros((N, N, N))
    for point, pin0 in (((8, 8, 8), False), ((5, 7, 9), True)):
        mask = np.zeros((N, N, N), dtype=np.uint8)
        mask[point] = 1
        u0[point] = 0.75
        prob = MR.Hierarchy(c, L, 2, 0.0, None, 0, 63, mask)
        assert MR.pinned(0, 63, 0.0, prob.mask[0]) == pin0 and not MR.is_singular(prob)
        x, ref_norms, ok, _, _ = MR.wpcg(prob, u0, d, 1e-8, 0.0, 60)
        assert ok
        with _solver(c, L, 2, 0.0, None, 0, 63, mask) as s:
            s.upload(MG3D_U, L - 1, u0)
            s.upload(MG3D_D, L - 1, d)
            norms, info = s.wpcg_solve(rtol=1e-8, max_iters=60)
            assert info["singular"] == 0 and info["rhs_mean"] == 0. and info["converged"]
            assert info["iterations"] == len(ref_norms) - 1
            u = s.download(MG3D_U, L - 1).reshape(N, N, N)
            assert u[point] == 0.75
            true = s.residual(L - 1, store=False)
            assert true <= 1e-6 * norms[0]
            assert np.abs(u - x).max() <= 1e-6 * np.abs(x).max()
        u0[point] = 0.
    with _solver(c, L, 2, 0.0, None, 0, 63, np.zeros(N ** 3, dtype=np.uint8)) as s:
        s.upload(MG3D_U, L - 1, u0)
        s.upload(MG3D_D, L - 1, d)
        _, info = s.wpcg_solve(rtol=1e-8, max_iters=60)
        assert info["singular"] == 1 and info["converged"]


# ----------------------------------------------------------------------------------------------------------- 5 stepper
@pytest.mark.parametrize("method", ["vcycles", "wpcg"])
def test_step_advance(method):
    """three steps at 17^3 with a fixed block (Crank-Nicolson, a source, periodic k + Neumann i faces): u at the fixed
    points bitwise constant, u elsewhere against _step_ref driven by the masked hierarchy"""
    c, L, N = 5, 3, 17
    axes, faces, dt, theta, kappa = 4, 3, 1e-3, 0.5, 2.0
    mask = np.zeros((N, N, N), dtype=np.uint8)
    mask[5:9, 6:10, 4:8] = 1
    rng = np.random.default_rng(17)
    u0, src = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    NR.refresh(u0, axes)
    u0[mask != 0] = 2.5
    prob = MR.Hierarchy(c, L, 2, SR.sigma_of(dt, theta, kappa), None, axes, faces, mask)
    prob.u[-1][...] = u0
    cycles = 2 if method == "vcycles" else 1
    want_n, _, _ = MR.advance(prob, 3, cycles, src, dt, theta, kappa, method=method, rtol=0.0)
    with M.Solver(c, L, 2) as s:
        s.set_periodic(axes)
        s.set_neumann(faces)
        s.set_mask(mask)
        s.step_setup(dt, theta, kappa)
        s.get_details()
        s.step_set_source(src)
        s.upload(MG3D_U, L - 1, u0)
        norms, info = s.step_advance(3, cycles=cycles, method=method, rtol=0.0)
        assert info["steps"] == 3
        u = s.download(MG3D_U, L - 1).reshape(N, N, N)
    assert _same_bits(u[mask != 0], u0[mask != 0])
    if method == "vcycles":
        assert _same_bits(u, prob.u[-1])
        np.testing.assert_allclose(norms, want_n, rtol=norm_rtol(N))
    else:
        rel = np.abs(u - prob.u[-1]).max() / np.abs(prob.u[-1]).max()
        nrel = (np.abs(norms - want_n) / want_n).max()
        print("step wpcg: u", rel, "norms", nrel)
        assert rel <= 100 * TW.SPREAD_U[5] and nrel <= 100 * TW.SPREAD_NORM


# ------------------------------------------------------------------------------------------- 6 setters, state, refusals
def test_setters_in_every_order():
    """shift, coefficient, periodic, Neumann, mask in all 120 orders of the five setters, the factor built before the
    first, between two of them or after the last: the same bits.  Then a setter called twice: a periodic axis set and
    cleared again under a mask -- the duplicates' bytes are then their sources' for good (include/mg3d.h), everything
    else is the mask as given"""
    c, L, N = 5, 3, 17
    sigma, axes, faces = 3.5, 4, 3
    eps, mask = _eps(N), MR.gpu_test_mask(N)
    ref = MR.Hierarchy(c, L, 2, sigma, eps, axes, faces, mask)
    _random_problem(ref, np.random.default_rng(1))
    u, d = ref.u[-1].copy(), ref.d[-1].copy()
    want = ref.vcycles(2)
    setters = {"shift": lambda s: s.set_shift(sigma), "coef": lambda s: s.set_coefficient(eps),
               "periodic": lambda s: s.set_periodic(axes), "neumann": lambda s: s.set_neumann(faces),
               "mask": lambda s: s.set_mask(mask)}
    for n_, order in enumerate(itertools.permutations(setters)):
        with M.Solver(c, L, 2) as s:
            at = n_ % 6
            for pos, name in enumerate(order):
                if pos == at:
                    s.get_details()
                setters[name](s)
            if at == 5:
                s.get_details()
            s.upload(MG3D_U, L - 1, u)
            s.upload(MG3D_D, L - 1, d)
            got = s.vcycles(2)
            assert _same_bits(s.download(MG3D_U, L - 1), ref.u[-1]), order
            assert np.array_equal(s.get_mask(0), ref.mask[0]) and np.array_equal(s.get_mask(L - 1), ref.mask[-1]), order
            np.testing.assert_allclose(got, want, rtol=norm_rtol(N))
    # mask, a periodic i axis, the axis cleared, then a Neumann face where the duplicates were: plane N-1 holds plane 0's
    # bytes, as if the caller had passed them
    with M.Solver(c, L, 2) as s:
        s.get_details()
        s.set_mask(mask)
        s.set_periodic(1)
        s.set_periodic(0)
        s.set_neumann(2)
        kept = mask.copy()
        kept[N - 1] = kept[0]
        assert np.array_equal(s.get_mask(L - 1), kept)
        ref2 = MR.Hierarchy(c, L, 2, 0.0, None, 0, 2, kept)
        ref2.u[-1][...] = u
        ref2.d[-1][...] = d
        ref2.vcycles(2)
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        s.vcycles(2)
        assert _same_bits(s.download(MG3D_U, L - 1), ref2.u[-1])


def test_one_level_context_keeps_its_fixed_values():
    """L = 1: the direct solve is the solve, and its identity rows at the fixed unknowns take u's own values instead of the
    zero error of a cycle"""
    c = 9
    mask = MR.gpu_test_mask(c)
    rng = np.random.default_rng(8)
    for axes, faces, sigma in ((0, 0, 0.0), (4, 3, 3.5)):
        ref = MR.Hierarchy(c, 1, 2, sigma, None, axes, faces, mask)
        u, d = rng.standard_normal((c, c, c)), rng.standard_normal((c, c, c))
        NR.refresh(u, axes)
        fx = ref.fixed(0)
        assert fx.any()
        d[fx] = np.nan
        with _solver(c, 1, 2, sigma, None, axes, faces, mask) as s:
            s.upload(MG3D_U, 0, u)
            s.upload(MG3D_D, 0, d)
            s.coarse_solve()
            got = s.download(MG3D_U, 0).reshape(c, c, c)
        want = u.copy()
        MR.coarse_solve(ref.LU, d, want, axes, faces, sigma, ref.mask[0], one_level=True)
        assert _same_bits(got, want) and _same_bits(got[fx], u[fx]) and np.isfinite(got).all()


def test_a_new_mask_rebuilds_a_built_factor_and_drops_an_installed_one():
    c, L, N = 5, 3, 17
    m1, m2 = MR.sphere(N, 0.3), MR.gpu_test_mask(N)
    ref = MR.Hierarchy(c, L, 2, 0.0, None, 0, 0, m2)
    _random_problem(ref, np.random.default_rng(9))
    u, d = ref.u[-1].copy(), ref.d[-1].copy()
    ref.vcycles(1)
    with _solver(c, L, 2, 0.0, None, 0, 0, m1) as s:
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        s.vcycle()
        s.set_mask(m2)  # the cycle that ran ahead is finished, the factor of get_details() rebuilt
        s.upload(MG3D_U, L - 1, u)
        s.vcycles(1)
        assert _same_bits(s.download(MG3D_U, L - 1), ref.u[-1])
        s.set_lu(ref.LU)
        s.upload(MG3D_U, L - 1, u)
        s.vcycles(1)
        assert _same_bits(s.download(MG3D_U, L - 1), ref.u[-1])
        s.set_mask(m1)  # an installed factor is dropped
        with pytest.raises(M.Mg3dError) as ei:
            s.vcycles(1)
        assert ei.value.code == MG3D_ERR_STATE
        s.set_lu(ref.LU)
        s.set_mask(None)
        with pytest.raises(M.Mg3dError) as ei:
            s.vcycles(1)
        assert ei.value.code == MG3D_ERR_STATE


def test_refusals_change_nothing():
    c, L, N = 5, 3, 17
    mask = MR.gpu_test_mask(N)
    rng = np.random.default_rng(4)
    u = rng.standard_normal(N ** 3)
    with M.Solver(c, L, 2) as s:
        s.set_mask(mask)
        s.get_details()
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_U, L - 2, u[:9 ** 3])
        for call in (lambda: s.es_setup(), lambda: s.fmg_initialize(), lambda: s.fmg_solve(1), lambda: s.fmg_interpolate(L - 1)):
            with pytest.raises(M.Mg3dError) as ei:
                call()
            assert ei.value.code == MG3D_ERR_STATE
        assert s.L.mg3d_es_smooth(s._h, L - 1, 0, 1) == MG3D_ERR_STATE
        assert s.L.mg3d_es_vcycles(s._h, 1, None) == MG3D_ERR_STATE
        assert s.has_mask() and np.array_equal(s.get_mask(), mask)
        assert _same_bits(s.download(MG3D_U, L - 1), u) and _same_bits(s.download(MG3D_U, L - 2), u[:9 ** 3])
        s.vcycles(1)  # the factor is still there


# ------------------------------------------------------------------------------------------------------- 7 device form
def test_device_form():
    """uint8 and bool tensors, contiguous, permuted, sliced and zero-stride broadcast: the host form's bytes on every
    level and the host form's cycle; wrong dtype, host pointer, negative stride: MG3D_ERR_ARG, nothing changed"""
    c, L, N = 5, 3, 17
    axes = 5
    dev = torch.device("cuda:0")
    mask = MR.gpu_test_mask(N) * np.uint8(3)
    plate = np.zeros((N, N, N), dtype=np.uint8)
    plate[6:8] = 1
    rng = np.random.default_rng(6)
    u, d = rng.standard_normal(N ** 3), rng.standard_normal(N ** 3)

    def run(s):
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        n = s.vcycles(2)
        return n, s.download(MG3D_U, L - 1), [s.get_mask(l) for l in range(L)]

    with M.Solver(c, L, 2) as h, M.Solver(c, L, 2) as g:
        for s in (h, g):
            s.set_periodic(axes)
            s.get_details()
        t = torch.from_numpy(mask).to(dev)
        big = torch.zeros((2 * N, N + 3, N + 2), dtype=torch.uint8, device=dev)
        big[::2, 2:N + 2, 1:N + 1] = t
        views = {"contiguous": (mask, t), "bool": ((mask != 0), torch.from_numpy(mask != 0).to(dev)),
                 "permuted": (mask, t.permute(2, 0, 1).contiguous().permute(1, 2, 0)),
                 "sliced": (mask, big[::2, 2:N + 2, 1:N + 1]),
                 "broadcast": (plate, torch.from_numpy(plate[:, 0, 0].copy()).to(dev)[:, None, None].expand(N, N, N))}
        for name, (host, tensor) in views.items():
            assert tuple(tensor.shape) == (N, N, N)
            h.set_mask(host)
            g.set_mask_tensor(tensor)
            nh, uh, mh = run(h)
            ng, ug, mg = run(g)
            assert np.array_equal(nh, ng) and _same_bits(uh, ug), name
            want = MR.inject(MR.stored(np.asarray(host).astype(np.uint8), axes), L)
            for l in range(L):
                assert np.array_equal(mh[l], mg[l]) and np.array_equal(mg[l], want[l]), (name, l)
        before = [g.get_mask(l) for l in range(L)]
        lib = g.L
        st = (C.c_longlong * 3)(N * N, N, 1)
        f64 = torch.zeros((N, N, N), dtype=torch.float64, device=dev)
        host_bytes = np.zeros(N ** 3, dtype=np.uint8)
        bad = [mg3d_array(f64.data_ptr(), MG3D_F64, st), mg3d_array(host_bytes.ctypes.data, MG3D_U8, st),
               mg3d_array(t.data_ptr() + N - 1, MG3D_U8, (C.c_longlong * 3)(N * N, N, -1))]
        for a in bad:
            assert lib.mg3d_ctx_set_mask_device(g._h, C.byref(a), None) == MG3D_ERR_ARG
        u8 = mg3d_array(t.data_ptr(), MG3D_U8, st)
        assert lib.mg3d_upload_device(g._h, MG3D_U, L - 1, C.byref(u8), None) == MG3D_ERR_ARG
        assert lib.mg3d_ctx_set_coefficient_device(g._h, C.byref(u8), None) == MG3D_ERR_ARG
        for l in range(L):
            assert np.array_equal(g.get_mask(l), before[l])
        with pytest.raises(TypeError):
            g.set_mask_tensor(f64)
        g.set_mask_tensor(None)
        assert not g.has_mask()
