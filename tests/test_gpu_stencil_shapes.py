"""The stencil kernel family of csrc/mg3d_kernels.hip (smooth_color_kernel, coef_color_kernel, residual_kernel, and the
grid transfers beside them) at the shapes the 2^k+1 ladder never reaches, against the numpy reference of
tests/_periodic_ref.py -- itself pinned at mask 0 to tests/_screened_ref.py and tests/_coef_ref.py by
tests/test_stencil_ref_host.py:

- coarse grids c = 6, 7, 10, 11, 13: levels whose unique k-columns leave the last 64-lane wave and the last 4-row block
  partly filled in ways c = 3, 5, 9, 17 never do; the single operators at the top two levels and V-cycles on every level;
- 513^3 (exactly MG3D_MAX_PARTIALS column partials) and 577^3 (past it: column_grid() doubles the chunk to 32 planes, and
  a Dirichlet i-axis leaves a short last chunk), checked through the blockwise reference.

Grid values bit for bit with sign bits, duplicates periodic-consistent, norms against the exactly rounded sum.  The
constant operator with mask 0 runs under MG3D_NO_FUSE=1 (without it the fused sweep takes that path) against the C
oracle."""
import os
import re

import numpy as np
import pytest

import _coef_ref as CR
import _oracle as O
import _periodic_ref as R
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U

gpu = pytest.mark.gpu
EXACT_NORM_RTOL = 1e-13
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_bits(a, b):
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _consistent(a, axes):
    b = np.asarray(a).reshape((round(np.asarray(a).size ** (1 / 3)),) * 3)
    c = b.copy()
    R.refresh(c, axes)
    return _same_bits(b, c)


def _masks(c):
    """the masks coarse grid c allows: a periodic axis needs c - 1 even (and at least 4)"""
    return (0, 1, 2, 4, 3, 5, 6, 7) if (c - 1) % 2 == 0 and c >= 5 else (0,)


def _solver(c, L, nu, sigma, eps, axes):
    import multigrid_parallel_amd as M
    s = M.Solver(c, L, nu)
    s.set_shift(sigma)
    s.set_periodic(axes)
    if eps is not None:
        s.set_coefficient(eps)
    s.get_details()
    return s


class _Oracle:
    """the C oracle's operators on one level of the constant operator with mask 0, in the shape of R's functions"""

    @staticmethod
    def _call(f, u, d, *args):
        uf = np.ascontiguousarray(u.reshape(-1))
        out = f(O.P(uf), O.P(np.ascontiguousarray(d.reshape(-1))), u.shape[0], *args)
        u[...] = uf.reshape(u.shape)
        return out

    @classmethod
    def pre_smooth(cls, u, d, h, sigma, iters):
        cls._call(O.lib().orc_pre_smooth_shift, u, d, h, sigma, iters)

    @classmethod
    def post_smooth(cls, u, d, h, sigma, iters):
        cls._call(O.lib().orc_post_smooth_shift, u, d, h, sigma, iters)

    @staticmethod
    def residual(u, d, h, sigma, r):
        rf = np.ascontiguousarray(r.reshape(-1))
        O.lib().orc_residual_shift(O.P(np.ascontiguousarray(u.reshape(-1))), O.P(np.ascontiguousarray(d.reshape(-1))),
                                   u.shape[0], h, sigma, O.P(rf))
        r[...] = rf.reshape(r.shape)

    @staticmethod
    def restrict(r, dc):
        out = np.ascontiguousarray(dc.reshape(-1))
        O.lib().orc_restrict(O.P(np.ascontiguousarray(r.reshape(-1))), r.shape[0], O.P(out), dc.shape[0])
        dc[...] = out.reshape(dc.shape)

    @staticmethod
    def prolong(ec, ef):
        out = np.ascontiguousarray(ef.reshape(-1))
        O.lib().orc_prolong(O.P(np.ascontiguousarray(ec.reshape(-1))), ec.shape[0], O.P(out), ef.shape[0])
        ef[...] = out.reshape(ef.shape)


# ----------------------------------------------------------------------------------------------- single operators
# (field, sigma): eps with sigma 0 and 1e3, the constant operator with sigma 1e3
_OPS = [("ball", 0.0), ("exp", 1e3), (None, 1e3)]
_SINGLE = []
for _c in (6, 7, 10, 11, 13):
    for _o, (_f, _s) in enumerate(_OPS):
        for _i, _axes in enumerate(_masks(_c)):
            for _L in ((3, 4) if len(_masks(_c)) == 1 else (3 + (_i + _o) % 2,)):
                _SINGLE.append((_c, _L, _f, _s, _axes))


@gpu
@pytest.mark.parametrize("c,L,field,sigma,axes", _SINGLE)
def test_single_operators(monkeypatch, c, L, field, sigma, axes):
    """random u, d at the top two levels: smooth (post, iters) = (0,1), (1,2), (0,3); residual with r stored and not;
    smooth_residual; restrict of the stored r; prolong of a random coarse e; coarse_solve"""
    oracle = field is None and axes == 0
    if oracle:
        monkeypatch.setenv("MG3D_NO_FUSE", "1")  # read when the context is created
    N = O.level_sizes(c, L)[-1]
    eps = None if field is None else CR.FIELDS[field](N)
    ref = R.Problem(c, L, 1, sigma, eps, axes)
    rng = np.random.default_rng(1000 * c + 10 * L + axes)
    with _solver(c, L, 1, sigma, eps, axes) as s:
        for l in (L - 1, L - 2):
            n, h, e = s.level_n(l), s.level_h(l), ref.e(l)
            u, d = rng.standard_normal((n, n, n)), rng.standard_normal((n, n, n))
            R.refresh(u, axes)  # (a duplicate on a Dirichlet face is never written: it starts consistent)
            R.refresh(d, axes)
            s.upload(MG3D_U, l, u)
            s.upload(MG3D_D, l, d)
            for post, iters in ((0, 1), (1, 2), (0, 3)):
                s.smooth(l, post, iters)
                if oracle:
                    (_Oracle.post_smooth if post else _Oracle.pre_smooth)(u, d, h, sigma, iters)
                else:
                    (R.post_smooth if post else R.pre_smooth)(u, d, e, h, sigma, axes, iters)
                got = s.download(MG3D_U, l)
                assert _same_bits(got, u.reshape(-1)), f"smooth({post}, {iters}), level {l}"
                assert _consistent(got, axes), f"smooth({post}, {iters}), level {l}: duplicates"

            def residual(r):
                if oracle:
                    _Oracle.residual(u, d, h, sigma, r)
                else:
                    R.residual(u, d, e, h, sigma, axes, r)
                return R.exact_residual_norm(u, d, e, n, h, sigma, axes)

            r = np.zeros((n, n, n))
            s.zero(MG3D_R, l)
            got = s.residual(l, store=True)
            want = residual(r)
            stored = s.download(MG3D_R, l)
            assert _same_bits(stored, r.reshape(-1)), f"residual, level {l}"
            assert _consistent(stored, axes), f"residual, level {l}: duplicates"
            assert got == pytest.approx(want, rel=EXACT_NORM_RTOL), (got, want)
            assert s.residual(l, store=False) == pytest.approx(want, rel=EXACT_NORM_RTOL)
            assert _same_bits(s.download(MG3D_R, l), stored), "residual(store=False) wrote r"

            got = s.smooth_residual(l, 1, 2, store=True)
            if oracle:
                _Oracle.post_smooth(u, d, h, sigma, 2)
            else:
                R.post_smooth(u, d, e, h, sigma, axes, 2)
            want = residual(r)
            assert _same_bits(s.download(MG3D_U, l), u.reshape(-1)), f"smooth_residual u, level {l}"
            assert _same_bits(s.download(MG3D_R, l), r.reshape(-1)), f"smooth_residual r, level {l}"
            assert got == pytest.approx(want, rel=EXACT_NORM_RTOL), (got, want)

            nc = s.level_n(l - 1)
            dc = rng.standard_normal((nc, nc, nc))
            s.upload(MG3D_D, l - 1, dc)
            s.restrict(l)
            _Oracle.restrict(r, dc) if oracle else R.restrict(r, dc, axes)
            got = s.download(MG3D_D, l - 1)
            assert _same_bits(got, dc.reshape(-1)), f"restrict, level {l}"
            assert _consistent(got, axes), f"restrict, level {l}: duplicates"

            ec = rng.standard_normal((nc, nc, nc))
            R.refresh(ec, axes)
            s.upload(MG3D_U, l - 1, ec)
            s.prolong(l)
            _Oracle.prolong(ec, u) if oracle else R.prolong(ec, u, axes)
            got = s.download(MG3D_U, l)
            assert _same_bits(got, u.reshape(-1)), f"prolong, level {l}"
            assert _consistent(got, axes), f"prolong, level {l}: duplicates"
        d0 = rng.standard_normal((c, c, c))
        s.upload(MG3D_D, 0, d0)
        s.coarse_solve()
        u0 = np.zeros((c, c, c))
        R.coarse_solve(ref.LU, d0, u0, axes, sigma)
        got = s.download(MG3D_U, 0)
        assert _same_bits(got, u0.reshape(-1)), "coarse_solve"
        assert _consistent(got, axes), "coarse_solve: duplicates"


# ------------------------------------------------------------------------------------------------- V-cycle parity
# a sample of (c, L, nu, sigma, field, mask), not the product: every mask with c = 7, 11 and 13, nu 1..3, both sigmas and
# every eps field on each coarse grid, largest level 193^3; mask 0 without eps runs unfused
_VCYCLE = [
    (6, 4, 1, 0.0, "smooth", 0), (6, 5, 2, 1e3, "exp", 0), (6, 4, 3, 1e3, "ball", 0), (6, 5, 2, 1e3, None, 0),
    (6, 6, 1, 0.0, "exp", 0),
    (7, 4, 1, 0.0, None, 1), (7, 4, 2, 1e3, "smooth", 2), (7, 5, 3, 0.0, "exp", 4), (7, 4, 2, 0.0, "ball", 3),
    (7, 5, 1, 1e3, None, 5), (7, 4, 3, 1e3, "exp", 6), (7, 5, 2, 0.0, "smooth", 7), (7, 6, 1, 1e3, "exp", 5),
    (7, 6, 2, 0.0, None, 7), (7, 5, 2, 1e3, "ball", 0),
    (11, 3, 1, 1e3, "exp", 1), (11, 4, 2, 0.0, None, 2), (11, 3, 3, 0.0, "smooth", 4), (11, 4, 1, 1e3, "ball", 3),
    (11, 4, 3, 1e3, None, 6), (11, 3, 2, 0.0, "exp", 7), (11, 4, 2, 1e3, "smooth", 0), (11, 5, 1, 0.0, "exp", 5),
    (13, 3, 2, 1e3, None, 1), (13, 4, 1, 0.0, "exp", 2), (13, 3, 3, 1e3, "smooth", 4), (13, 4, 2, 0.0, None, 3),
    (13, 3, 1, 0.0, "ball", 6), (13, 4, 3, 1e3, "exp", 7), (13, 3, 2, 0.0, None, 0), (13, 4, 2, 1e3, "exp", 5),
]


@gpu
@pytest.mark.parametrize("c,L,nu,sigma,field,axes", _VCYCLE)
def test_vcycle_parity(monkeypatch, c, L, nu, sigma, field, axes):
    """u of every level and d below the top after vcycles(1) + vcycles(2) from a random start, bit for bit"""
    if field is None and axes == 0:
        monkeypatch.setenv("MG3D_NO_FUSE", "1")
    N = O.level_sizes(c, L)[-1]
    eps = None if field is None else CR.FIELDS[field](N)
    ref = R.Problem(c, L, nu, sigma, eps, axes)
    rng = np.random.default_rng(c * 100 + L * 10 + axes)
    ref.u[-1][...] = rng.standard_normal((N, N, N))
    ref.d[-1][...] = rng.standard_normal((N, N, N))
    R.refresh(ref.u[-1], axes)
    R.refresh(ref.d[-1], axes)
    with _solver(c, L, nu, sigma, eps, axes) as s:
        s.upload(MG3D_U, L - 1, ref.u[-1])
        s.upload(MG3D_D, L - 1, ref.d[-1])
        want = ref.vcycles(3)
        got = list(s.vcycles(1)) + list(s.vcycles(2))
        for l in range(L):
            u = s.download(MG3D_U, l)
            assert _same_bits(u, ref.flat("u", l)), f"u level {l}"
            assert _consistent(u, axes), f"u level {l}: duplicates"
        for l in range(L - 1):
            d = s.download(MG3D_D, l)
            assert _same_bits(d, ref.flat("d", l)), f"d level {l}"
            assert _consistent(d, axes), f"d level {l}: duplicates"
        exact = R.exact_residual_norm(s.download(MG3D_U, L - 1), s.download(MG3D_D, L - 1), ref.e(L - 1), N,
                                      s.level_h(L - 1), sigma, axes)
    assert got[-1] == pytest.approx(exact, rel=EXACT_NORM_RTOL), (got[-1], exact)
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=0)


# ---------------------------------------------------------------------------------- past the column partial cap
def _max_partials():
    text = open(os.path.join(ROOT, "multigrid_parallel_amd", "csrc", "mg3d_internal.h")).read()
    return int(re.search(r"#define\s+MG3D_MAX_PARTIALS\s+(\d+)", text).group(1))


def bc_extra(axes, faces, ax):
    """bc_extra() of csrc/mg3d_kernels.hip: the unknowns axis ax (0 i, 1 j, 2 k) has beyond the N - 2 interior ones --
    index 0 (a periodic axis or a Neumann low face) and index N-1 (a Neumann high face)"""
    return int(bool(axes >> ax & 1 or faces >> 2 * ax & 1)) + (faces >> (2 * ax + 1) & 1)


def column_grid(N, axes, faces=0):
    """column_grid() of csrc/mg3d_kernels.hip (with the planes stencil_window() leaves) for a single-domain level of N
    points, periodic axes `axes` and Neumann faces `faces`: (gx, gy, gz, chunk, planes)"""
    planes = N - 2 + bc_extra(axes, faces, 0)
    gx, gy = (N - 2 + bc_extra(axes, faces, 2) + 63) // 64, (N - 2 + bc_extra(axes, faces, 1) + 3) // 4
    chunk = 16
    while gx * gy * -(-planes // chunk) > _max_partials():
        chunk *= 2
    return gx, gy, -(-planes // chunk), chunk, planes


_BIG = {513: (9, 7), 577: (19, 6)}
# (field, sigma, mask); the constant operator with mask 0 runs unfused, against the C oracle
_BIG_CASES = [("exp", 10.0, 0), ("exp", 10.0, 5), (None, 10.0, 6), (None, 0.0, 0)]


def test_column_grid_reaches_the_shapes():
    """513^3 fills MG3D_MAX_PARTIALS exactly at chunk 16; 577^3 needs chunk > 16, with a short last chunk when the i-axis
    is Dirichlet and full chunks when it is periodic -- for every mask of the cases below"""
    for N, (c, L) in _BIG.items():
        assert O.level_sizes(c, L)[-1] == N
    for _, _, axes in _BIG_CASES:
        gx, gy, gz, chunk, _ = column_grid(513, axes)
        assert chunk == 16 and gx * gy * gz == _max_partials(), (axes, gx, gy, gz)
        gx, gy, gz, chunk, planes = column_grid(577, axes)
        assert chunk > 16 and gx * gy * gz <= _max_partials(), (axes, gx, gy, gz)
        last = planes - (gz - 1) * chunk
        assert (last < chunk) == (not axes & 1) and last > 0, (axes, planes, chunk)


@gpu
@pytest.mark.parametrize("field,sigma,axes", _BIG_CASES)
@pytest.mark.parametrize("N", sorted(_BIG))
def test_past_the_partial_cap(monkeypatch, N, field, sigma, axes):
    """the finest level: smooth(top, 0, 1) and residual(top, store=True) on random u, d bit for bit with the blockwise
    reference (the C oracle for the unfused constant operator), the norm exact; then two V-cycles: the last norm is the
    exact norm of the downloaded u, the norm falls, a periodic u stays consistent"""
    c, L = _BIG[N]
    oracle = field is None and axes == 0
    if oracle:
        monkeypatch.setenv("MG3D_NO_FUSE", "1")
    rng = np.random.default_rng(N + axes)
    u, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    R.refresh(u, axes)
    R.refresh(d, axes)
    e = None
    if field is not None:
        e = CR.FIELDS[field](N)
        R.refresh(e, axes)
    with _solver(c, L, 1, sigma, e, axes) as s:
        top, h = L - 1, s.level_h(L - 1)
        s.upload(MG3D_U, top, u)
        s.upload(MG3D_D, top, d)
        s.smooth(top, 0, 1)
        if oracle:
            O.lib().orc_set_threads(O.lib().orc_max_threads())
            try:
                _Oracle.pre_smooth(u, d, h, sigma, 1)
            finally:
                O.lib().orc_set_threads(1)
        else:
            R.colour_pass_blocks(u, d, e, h, sigma, axes, 1)
            R.colour_pass_blocks(u, d, e, h, sigma, axes, 0)
        got = s.download(MG3D_U, top)
        assert _same_bits(got, u.reshape(-1)), "smooth"
        del got
        s.zero(MG3D_R, top)
        nrm = s.residual(top, store=True)
        r = np.zeros((N, N, N))
        if oracle:
            O.lib().orc_set_threads(O.lib().orc_max_threads())
            try:
                _Oracle.residual(u, d, h, sigma, r)
            finally:
                O.lib().orc_set_threads(1)
            want = R.residual_blocks(u, d, e, h, sigma, axes)
        else:
            want = R.residual_blocks(u, d, e, h, sigma, axes, r)
        got = s.download(MG3D_R, top)
        assert _same_bits(got, r.reshape(-1)), "residual"
        del got, r, u
        assert nrm == pytest.approx(want, rel=EXACT_NORM_RTOL), (nrm, want)
        norms = s.vcycles(2)
        u = s.download(MG3D_U, top).reshape(N, N, N)
    exact = R.residual_blocks(u, d, e, h, sigma, axes)
    assert norms[-1] == pytest.approx(exact, rel=EXACT_NORM_RTOL), (norms[-1], exact)
    assert norms[1] < norms[0] < nrm, (nrm, norms)
    if axes:
        assert _consistent(u, axes)
