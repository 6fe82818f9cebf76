"""Full multigrid for the caller's problem on the GPU (mg3d_fmg_interpolate, mg3d_fmg_solve) against the numpy restatement
of tests/_fmg_ref.py: the interpolation kernel bit for bit on every point of u -- Dirichlet points and periodic duplicates
included, from a sentinel -- at the shapes where its tiles end or its forms meet; the solve bit for bit on the finest u,
with d untouched and the norm to the summation tolerance; the schedules of the cycles inside; what stays as it was
(mg3d_vcycle below the top, mg3d_fmg_initialize, the context after a solve); refusals and argument checks."""
import numpy as np
import pytest

import _coef_ref as CR
import _fmg_ref as F
import _neumann_ref as R
import _screened_ref as S
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U, Mg3dError

pytestmark = pytest.mark.gpu

MG3D_ERR_ARG, MG3D_ERR_STATE = 1, 5
NORM_RTOL = 1e-13  # the project's summation tolerance
SENTINEL = 12345.678


def _same_bits(a, b):
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _n(c, L):
    return (c - 1) * (1 << (L - 1)) + 1


def _solver(c, L, nu, sigma=0.0, eps=None, axes=0, faces=0):
    s = M.Solver(c, L, nu)
    s.set_shift(sigma)
    s.set_periodic(axes)
    s.set_neumann(faces)
    if eps is not None:
        s.set_coefficient(eps)
    s.get_details()
    return s


# ---- the interpolation kernel
# fine side -> (c, L) with the interpolation into the top level: 5 (Nc = 3, the two-term form), 9 (Nc = 5: both one-sided
# rows touch the central ones), 17, 33, 65 and 73 / 81 (past the 64-lane row by 1, 9 and 17 columns; 67 is no side of a
# hierarchy with a coarse grid small enough to factor, 73 none with the even c - 1 a periodic axis needs), 129 (several
# tiles in j, and the most chunks in i at the shortest chunk: k_fmg_interp marches 2 coarse planes a block at every side
# up to 129; the chunk lengths 4, 8 and 16 are held in tests/test_gpu_mask_keep_shapes.py at 145 .. 257)
_SHAPES = {5: (3, 2), 9: (5, 2), 17: (5, 3), 33: (5, 4), 65: (5, 5), 73: (10, 4), 81: (11, 4), 129: (5, 6)}
# (periodic axes, Neumann faces): none; each periodic axis, all three; each Neumann face; both faces of j; periodic k with
# Neumann i-low and Dirichlet j
_WORDS = [(0, 0), (1, 0), (2, 0), (4, 0), (7, 0)] + [(0, 1 << f) for f in range(6)] + [(0, 12), (4, 1)]
_INTERP = [(n, axes, faces) for n in (5, 9, 17, 33, 65) for axes, faces in _WORDS if not (axes and n == 5)]
_INTERP += [(73, 0, faces) for axes, faces in _WORDS if not axes] + [(81, axes, faces) for axes, faces in _WORDS if axes]
_INTERP += [(129, 4, 1)]


@pytest.mark.parametrize("n,axes,faces", _INTERP)
def test_interpolation_bit_for_bit(n, axes, faces):
    c, L = _SHAPES[n]
    assert _n(c, L) == n
    nc = (n + 1) // 2
    rng = np.random.default_rng(n + 1000 * axes + 8000 * faces)
    uc = rng.standard_normal((nc, nc, nc))  # (duplicates not consistent: none may be read)
    want = np.full((n, n, n), SENTINEL)
    F.interpolate(uc, want, axes, faces)
    assert (want == SENTINEL).sum() == (~R.unknown_mask(n, axes, faces) & ~R.is_dup(n, axes)).sum() + \
        (R.is_dup(n, axes) & F.dirichlet_mask(n, axes, faces)).sum()
    with _solver(c, L, 2, 0.0, None, axes, faces) as s:
        s.upload(MG3D_U, L - 2, uc)
        s.upload(MG3D_U, L - 1, np.full((n, n, n), SENTINEL))
        s.fmg_interpolate(L - 1)
        got = s.download(MG3D_U, L - 1).reshape(n, n, n)
        assert _same_bits(s.download(MG3D_U, L - 2), uc.reshape(-1))
    bad = np.argwhere(got != want)
    assert _same_bits(got, want), (len(bad), bad[:5].tolist())


# ---- the solve
def _operator(name, c, L):
    """(sigma, eps, axes, faces)"""
    return {"constant": (0.0, None, 0, 0), "sigma": (25.0, None, 0, 0), "ball": (0.0, CR.ball_eps(_n(c, L)), 0, 0),
            "periodic7": (3.0, None, 7, 0), "neumann31": (0.0, None, 0, 31), "singular63": (0.0, None, 0, 63)}[name]


def _caller_data(N, axes, faces, sigma, seed):
    """random d and random u (the interior is to be ignored, the Dirichlet points are the boundary data); in the singular
    case d with its weighted mean taken out"""
    rng = np.random.default_rng(seed)
    u, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    if R.pinned(axes, faces, sigma):
        w = R.weights(N, axes, faces)
        d = np.where(w > 0, d - (w * d).sum() / w.sum(), d)
    return u, d


_SOLVE = [(c, L, op, cycles) for c, L in ((5, 3), (3, 4), (5, 4), (9, 4))
          for op in ("constant", "sigma", "ball", "periodic7", "neumann31", "singular63") for cycles in (1, 2)
          if not (op == "periodic7" and c == 3)]


@pytest.mark.parametrize("c,L,op,cycles", _SOLVE)
def test_solve_parity(c, L, op, cycles):
    sigma, eps, axes, faces = _operator(op, c, L)
    N = _n(c, L)
    u, d = _caller_data(N, axes, faces, sigma, 7 * N + cycles)
    ref = R.Problem(c, L, 2, sigma, eps, axes, faces)
    ref.u[-1][...] = u
    ref.d[-1][...] = d
    want = F.fmg_solve(ref, cycles)
    with _solver(c, L, 2, sigma, eps, axes, faces) as s:
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        got = s.fmg_solve(cycles)
        gu, gd = s.download(MG3D_U, L - 1), s.download(MG3D_D, L - 1)
    assert _same_bits(gd, d.reshape(-1))
    m = F.dirichlet_mask(N, axes, faces).reshape(-1)
    assert _same_bits(gu[m], u.reshape(-1)[m])
    bad = np.argwhere(gu != ref.flat("u", L - 1))
    assert _same_bits(gu, ref.flat("u", L - 1)), (len(bad), bad[:5].tolist())
    print(f"norm {got!r} reference {want!r}")
    assert got == pytest.approx(want, rel=NORM_RTOL)


# ---- schedules do not matter
def _fmg_u(c, L, cycles, options, seed=5):
    N = _n(c, L)
    u, d = _caller_data(N, 0, 0, 0.0, seed)
    with _solver(c, L, 2) as s:
        for k, v in options.items():
            s.set_option(k, v)
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        norm = s.fmg_solve(cycles)
        return norm, s.download(MG3D_U, L - 1)


@pytest.mark.parametrize("options", [{"tiny": 0}, {"tiny_cycle": 0}, {"fuse_up_max": 0}])
def test_schedule_options_change_no_bit_at_33(options):
    base = _fmg_u(5, 4, 1, {})
    other = _fmg_u(5, 4, 1, options)
    assert _same_bits(base[1], other[1])
    assert other[0] == pytest.approx(base[0], rel=NORM_RTOL)


@pytest.mark.parametrize("options", [{"legs_min": 66, "legs": 1, "carry": 0}, {"carry_min": 66, "legs": 0, "carry": 1}])
def test_top_level_run_ahead_schedules_change_no_bit_at_129(options):
    """129^3 with the thresholds lowered as tests/test_gpu_legs.py does: the finest level's two cycles run one launch per
    leg, or carried, against the plain schedule"""
    plain = _fmg_u(9, 5, 2, {"legs": 0, "carry": 0})
    other = _fmg_u(9, 5, 2, options)
    assert _same_bits(plain[1], other[1])
    assert other[0] == pytest.approx(plain[0], rel=NORM_RTOL)


# ---- old behaviour is intact
def test_vcycle_below_the_top_still_starts_from_zero():
    c, L, q = 5, 4, 2
    N = _n(c, L)
    rng = np.random.default_rng(11)
    ref = S.Problem(c, L, 2, 0.0)
    nq = ref.N[q]
    dq = rng.standard_normal((nq, nq, nq))
    ref.d[q][...] = dq.reshape(ref.d[q].shape)
    want = ref.vcycle(q, ref.h * (1 << (L - 1 - q)))
    with _solver(c, L, 2) as s:
        s.upload(MG3D_U, q, rng.standard_normal((nq, nq, nq)))  # a guess that must be discarded
        s.upload(MG3D_D, q, dq)
        got = s.vcycle(q)
        assert _same_bits(s.download(MG3D_U, q), np.ascontiguousarray(ref.u[q]).reshape(-1))
    assert got == pytest.approx(want, rel=NORM_RTOL)
    assert N == 33


def test_fmg_initialize_is_unchanged():
    """mg3d_fmg_initialize, then two cycles: every level against the reference's own F-cycle start, as before"""
    c, L = 5, 4
    ref = S.Problem(c, L, 2, 0.0)
    ref.setup_test_problem()
    ref.fmg_initialize()
    with M.Solver(c, L, 2) as s:
        s.setup_test_problem()
        s.fmg_initialize()
        for l in range(L):
            assert _same_bits(s.download(MG3D_U, l), ref.flat("u", l)), l
        got = s.vcycles(2)
        want = ref.vcycles(2)
        assert _same_bits(s.download(MG3D_U, L - 1), ref.flat("u", L - 1))
    np.testing.assert_allclose(got, want, rtol=NORM_RTOL)


@pytest.mark.parametrize("op", ["constant", "periodic7"])
def test_context_is_usable_after_a_solve(op):
    c, L = 5, 4
    sigma, eps, axes, faces = _operator(op, c, L)
    N = _n(c, L)
    u, d = _caller_data(N, axes, faces, sigma, 21)
    with _solver(c, L, 2, sigma, eps, axes, faces) as s:
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        s.fmg_solve(1)
        u1 = s.download(MG3D_U, L - 1)
        n1 = s.vcycles(1)
        u2 = s.download(MG3D_U, L - 1)
    with _solver(c, L, 2, sigma, eps, axes, faces) as t:
        t.upload(MG3D_U, L - 1, u1)
        t.upload(MG3D_D, L - 1, d)
        n2 = t.vcycles(1)
        assert _same_bits(t.download(MG3D_U, L - 1), u2)
    np.testing.assert_allclose(n1, n2, rtol=NORM_RTOL)


# ---- refusals and arguments
def _loaded(s, L, N, seed=3):
    rng = np.random.default_rng(seed)
    u, d = rng.standard_normal(N ** 3), rng.standard_normal(N ** 3)
    s.upload(MG3D_U, L - 1, u)
    s.upload(MG3D_D, L - 1, d)
    return u, d


def _refused(s, L, u, d, code, call):
    with pytest.raises(Mg3dError) as e:
        call()
    assert e.value.code == code
    assert _same_bits(s.download(MG3D_U, L - 1), u) and _same_bits(s.download(MG3D_D, L - 1), d)


def test_arguments():
    c, L = 5, 3
    with _solver(c, L, 2) as s:
        u, d = _loaded(s, L, _n(c, L))
        _refused(s, L, u, d, MG3D_ERR_ARG, lambda: s.fmg_solve(0))
        _refused(s, L, u, d, MG3D_ERR_ARG, lambda: s.fmg_solve(-1))
        for level in (0, L, -1):
            _refused(s, L, u, d, MG3D_ERR_ARG, lambda: s.fmg_interpolate(level))


def test_refused_without_a_factor():
    c, L = 5, 3
    with M.Solver(c, L, 2) as s:
        u, d = _loaded(s, L, _n(c, L))
        _refused(s, L, u, d, MG3D_ERR_STATE, lambda: s.fmg_solve(1))
        _refused(s, L, u, d, MG3D_ERR_STATE, lambda: s.fmg_interpolate(1))


def test_refused_after_es_setup():
    c, L = 5, 3
    es = M.EsParams.default()
    with M.Solver(c, L, 2, grid_length=es.length) as s:
        s.es_setup(es)
        u, d = s.download(MG3D_U, L - 1), s.download(MG3D_D, L - 1)
        _refused(s, L, u, d, MG3D_ERR_STATE, lambda: s.fmg_solve(1))
        _refused(s, L, u, d, MG3D_ERR_STATE, lambda: s.fmg_interpolate(L - 1))
