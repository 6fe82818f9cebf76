"""Neumann faces (mg3d_ctx_set_neumann) on the GPU, against the numpy reference of tests/_neumann_ref.py: every grid
value bit for bit on every level for each single face, all six and masks mixed with periodic axes; the single operators;
the norm over the unknowns; Dirichlet points untouched; mask 0 after a Neumann mask; run-ahead state across a change of
mask; the argument and state rules; an inhomogeneous-flux solve through fold_flux; the singular case.

Left out on purpose (time on the GPU): the V-cycle parity product is not the full cross of masks x (c, L) x operators.
Every single face and mask 63 run with the constant operator (sigma = 0 and sigma > 0) and with eps, nu in {1, 2} and
c in {3, 5, 9} spread over them (_CASES below lists exactly what runs); the mixed periodic masks run at c in {5, 9}
only, which a periodic axis requires.  At 513^3 the single operators run (one colour pass of each colour, residual with
r and norm), not a whole V-cycle: its numpy reference alone takes minutes.

What this file does not run, tests/test_gpu_neumann_shapes.py does: the pairs of faces on one axis alone (3, 12, 48) and
every single face at 65^3 and 129^3, where a face fills or overflows the last lane / row / plane block by one; every mask
on the coarse grids off the 2^k+1 ladder (c = 6, 7, 10, 11, 13); smooth_residual and smooth_restrict; V-cycles with
keep_residual (r of every level); 513^3 with the masks that keep or double the chunk of planes, and 577^3; and the
setters in other orders: the coefficient before the masks, one nonzero mask after another, an axis from periodic to
Neumann and back, eps given under a periodic mask that is cleared afterwards."""
import math

import numpy as np
import pytest

import _coef_ref as CR
import _neumann_ref as R
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U

from test_gpu_parity import norm_rtol

pytestmark = pytest.mark.gpu

MG3D_ERR_ARG, MG3D_ERR_STATE = 1, 5
SINGLE = [1, 2, 4, 8, 16, 32]


def _same_bits(a, b):
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _n(c, L):
    return (c - 1) * (1 << (L - 1)) + 1


def _random_problem(ref, rng):
    N = ref.N[-1]
    ref.u[-1][...] = rng.standard_normal((N, N, N))
    ref.d[-1][...] = rng.standard_normal((N, N, N))
    R.refresh(ref.u[-1], ref.axes)
    R.refresh(ref.d[-1], ref.axes)


def _solver(c, L, nu, sigma, eps, axes, faces, ref=None):
    s = M.Solver(c, L, nu)
    s.set_shift(sigma)
    s.set_periodic(axes)
    s.set_neumann(faces)
    if eps is not None:
        s.set_coefficient(eps)
    s.get_details()
    if ref is not None:
        s.upload(MG3D_U, L - 1, ref.u[-1])
        s.upload(MG3D_D, L - 1, ref.d[-1])
    return s


def _assert_levels(s, ref, L):
    for l in range(L):
        assert _same_bits(s.download(MG3D_U, l), ref.flat("u", l)), f"u level {l}"
    for l in range(L - 1):
        assert _same_bits(s.download(MG3D_D, l), ref.flat("d", l)), f"d level {l}"


# (c, L, axes, faces, sigma, field, nu): every single face and 63 with the constant operator, sigma > 0 and eps
_CASES = []
for n_, faces in enumerate(SINGLE + [63]):
    c, L = [(5, 4), (3, 5), (9, 4)][n_ % 3]
    _CASES += [(c, L, 0, faces, 0.0, None, 1 + n_ % 2), (c, L, 0, faces, 1e3, None, 2 - n_ % 2),
               (c, L, 0, faces, 0.0, "smooth", 2 - n_ % 2), (c, L, 0, faces, 10.0, "exp", 1 + n_ % 2)]
# all six faces on every ladder, one c off the 2^k+1 ladder, and a sample of mixed masks
_CASES += [(3, 5, 0, 63, 0.0, None, 2), (5, 5, 0, 63, 0.0, "smooth", 2), (9, 5, 0, 63, 0.0, None, 1),
           (6, 4, 0, 63, 0.0, None, 2), (6, 4, 0, 9, 1.0, "exp", 1), (7, 4, 0, 36, 0.0, None, 2),
           (5, 4, 0, 21, 0.0, None, 2), (5, 4, 0, 42, 2.0, "smooth", 1), (9, 4, 0, 3, 0.0, None, 2)]
for c, L in [(5, 4), (9, 4)]:
    for axes, faces in [(6, 3), (1, 60), (6, 1), (1, 20), (2, 33), (5, 12)]:
        _CASES += [(c, L, axes, faces, 0.0, None, 2), (c, L, axes, faces, 5.0, "smooth", 1)]


@pytest.mark.parametrize("c,L,axes,faces,sigma,field,nu", _CASES)
def test_parity(c, L, axes, faces, sigma, field, nu):
    """u of every level and d below the top after vcycles(1) + vcycles(2), bit for bit, and the norms"""
    eps = None if field is None else CR.FIELDS[field](_n(c, L))
    ref = R.Problem(c, L, nu, sigma, eps, axes, faces)
    _random_problem(ref, np.random.default_rng(faces + 64 * axes))
    with _solver(c, L, nu, sigma, eps, axes, faces, ref) as s:
        assert (s.periodic, s.neumann) == (axes, faces)
        want = ref.vcycles(3)
        got = list(s.vcycles(1)) + list(s.vcycles(2))
        _assert_levels(s, ref, L)
        N, h = s.level_n(L - 1), s.level_h(L - 1)
        exact = R.exact_residual_norm(s.download(MG3D_U, L - 1), s.download(MG3D_D, L - 1), ref.e(L - 1), N, h, sigma,
                                      axes, faces)
        assert got[-1] == pytest.approx(exact, rel=norm_rtol(N)), (got[-1], exact)
    np.testing.assert_allclose(got, want, rtol=norm_rtol(ref.N[-1]))


def test_full_size_257():
    """257^3, all six faces, sigma > 0, nu = 1: the block forms of the reference, the multi-chunk launches"""
    c, L, faces, sigma = 9, 6, 63, 10.0
    ref = R.Problem(c, L, 1, sigma, None, 0, faces)
    _random_problem(ref, np.random.default_rng(257))
    with _solver(c, L, 1, sigma, None, 0, faces, ref) as s:
        want = ref.vcycles(2)
        got = s.vcycles(2)
        assert _same_bits(s.download(MG3D_U, L - 1), ref.flat("u", L - 1))
    np.testing.assert_allclose(got, want, rtol=norm_rtol(ref.N[-1]))


@pytest.mark.parametrize("field", [None, "smooth"])
def test_single_operators_513(field):
    """513^3 (past the cap of partial sums: chunks of 32 planes), all six faces: one pass of each colour and the residual
    with r and norm, against the block forms"""
    c, L, faces, sigma = 3, 9, 63, 3.0
    N = _n(c, L)
    assert N == 513
    rng = np.random.default_rng(513)
    u, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    eps = None if field is None else CR.FIELDS[field](N)
    with _solver(c, L, 1, sigma, eps, 0, faces) as s:
        h = s.level_h(L - 1)
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        s.smooth(L - 1, 0, 1)
        R.colour_pass_blocks(u, d, eps, h, sigma, 0, faces, 1)
        R.colour_pass_blocks(u, d, eps, h, sigma, 0, faces, 0)
        assert _same_bits(s.download(MG3D_U, L - 1), u.reshape(-1))
        r = np.zeros((N, N, N))
        s.zero(MG3D_R, L - 1)
        got = s.residual(L - 1, store=True)
        want = R.residual_blocks(u, d, eps, h, sigma, 0, faces, r)
        assert _same_bits(s.download(MG3D_R, L - 1), r.reshape(-1))
        assert abs(got - want) <= norm_rtol(N) * want, (got, want)


@pytest.mark.parametrize("axes,faces", [(0, f) for f in SINGLE] + [(0, 63), (0, 22), (6, 3), (1, 60), (4, 6)])
@pytest.mark.parametrize("field", [None, "exp"])
def test_single_operators(axes, faces, field):
    """smooth, residual (with and without r), restrict, prolong, coarse_solve on random data, bit for bit; the points on
    Dirichlet faces keep whatever they held through every entry point"""
    c, L = 5, 3
    sigma = 0.0 if R.pinned(axes, faces, 0.0) else 1.0
    rng = np.random.default_rng(11 + faces + 64 * axes)
    N = _n(c, L)
    eps = None if field is None else CR.FIELDS[field](N)
    ref = R.Problem(c, L, 2, sigma, eps, axes, faces)
    with _solver(c, L, 2, sigma, eps, axes, faces) as s:
        for l in (L - 1, L - 2):
            n, h, e = s.level_n(l), s.level_h(l), ref.e(l)
            fixed = ~R.unknown_mask(n, axes, faces) & ~R.is_dup(n, axes)
            u, d = rng.standard_normal((n, n, n)), rng.standard_normal((n, n, n))
            R.refresh(u, axes)
            u_in = u.copy()
            s.upload(MG3D_U, l, u)
            s.upload(MG3D_D, l, d)
            s.smooth(l, 0, 2)
            R.pre_smooth(u, d, e, h, sigma, axes, faces, 2)
            assert _same_bits(s.download(MG3D_U, l), u.reshape(-1)), f"pre-smoothing, level {l}"
            s.smooth(l, 1, 1)
            R.post_smooth(u, d, e, h, sigma, axes, faces, 1)
            assert _same_bits(s.download(MG3D_U, l), u.reshape(-1)), f"post-smoothing, level {l}"
            assert _same_bits(u[fixed], u_in[fixed])
            r = rng.standard_normal((n, n, n))
            r_in = r.copy()
            s.upload(MG3D_R, l, r)
            got_norm_only = s.residual(l, store=False)
            assert _same_bits(s.download(MG3D_R, l), r_in.reshape(-1)), "the norm-only residual writes no r"
            got = s.residual(l, store=True)
            want = R.residual(u, d, e, h, sigma, axes, faces, r)
            assert _same_bits(s.download(MG3D_R, l), r.reshape(-1)), f"residual, level {l}"
            assert _same_bits(r[fixed], r_in[fixed])
            assert got == got_norm_only
            exact = R.exact_residual_norm(u, d, e, n, h, sigma, axes, faces)
            assert abs(got - exact) <= norm_rtol(n) * exact, (got, want, exact)
            nc = s.level_n(l - 1)
            dc = rng.standard_normal((nc, nc, nc))
            s.upload(MG3D_D, l - 1, dc)
            s.restrict(l)
            R.restrict(r, dc, axes, faces)
            assert _same_bits(s.download(MG3D_D, l - 1), dc.reshape(-1)), f"restrict, level {l}"
            ec = rng.standard_normal((nc, nc, nc))
            R.refresh(ec, axes)
            s.upload(MG3D_U, l - 1, ec)
            s.prolong(l)
            R.prolong(ec, u, axes, faces)
            assert _same_bits(s.download(MG3D_U, l), u.reshape(-1)), f"prolong, level {l}"
        n0 = s.level_n(0)
        d0 = rng.standard_normal((n0, n0, n0))
        s.upload(MG3D_D, 0, d0)
        s.coarse_solve()
        u0 = np.zeros((n0, n0, n0))
        R.coarse_solve(ref.LU, d0, u0, axes, faces, sigma)
        assert _same_bits(s.download(MG3D_U, 0), u0.reshape(-1))


@pytest.mark.parametrize("faces", [1, 40, 63])
def test_norm_over_the_unknowns(faces):
    c, L, sigma = 9, 4, 0.0
    ref = R.Problem(c, L, 2, sigma, None, 0, faces)
    _random_problem(ref, np.random.default_rng(5))
    with _solver(c, L, 2, sigma, None, 0, faces, ref) as s:
        got = s.residual(L - 1, store=False)
        N, h = s.level_n(L - 1), s.level_h(L - 1)
        diff = R.residual_field(ref.u[-1], ref.d[-1], None, h, sigma, 0, faces)
        want = math.sqrt(math.fsum((diff * diff).reshape(-1)))
        assert abs(got - want) <= norm_rtol(N) * want, (got, want)
        assert diff.size == R.unknown_mask(N, 0, faces).sum()
        assert diff.size == (N - 2 + bin(faces & 3).count("1")) * (N - 2 + bin(faces & 12).count("1")) * (
            N - 2 + bin(faces & 48).count("1"))


@pytest.mark.parametrize("faces", [5, 63])
def test_dirichlet_points_untouched_by_cycles(faces):
    """NaN-free sentinels on every Dirichlet point of u survive V-cycles unchanged (mask 63 has none: nothing to keep)"""
    c, L = 5, 4
    N = _n(c, L)
    rng = np.random.default_rng(17)
    u, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    fixed = ~R.unknown_mask(N, 0, faces)
    with _solver(c, L, 2, 1.0, None, 0, faces) as s:
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        s.vcycles(2)
        s.vcycle()
        got = s.download(MG3D_U, L - 1).reshape(N, N, N)
    assert _same_bits(got[fixed], u[fixed])
    assert fixed.sum() == (0 if faces == 63 else N ** 3 - (N - 1) * (N - 1) * (N - 2))


def test_mask_0_after_a_neumann_mask_is_a_fresh_context():
    """bits of u, norms and the fused schedules of a fresh context (kernel timers: sweeps run again)"""
    c, L = 9, 5
    N = _n(c, L)
    rng = np.random.default_rng(9)
    u, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))

    def run(s):
        s.get_details()
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        s.timing_enable(True)
        s.timing_reset()
        norms = [s.vcycle()] + list(s.vcycles(3))
        kt = s.kernel_times()
        return norms, s.download(MG3D_U, L - 1), kt

    with M.Solver(c, L, 2) as s:
        s.set_neumann(("ilo", "khi"))
        assert s.neumann == 33
        s.get_details()
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        s.vcycles(1)
        s.set_neumann(())
        assert s.neumann == 0
        got = run(s)
    with M.Solver(c, L, 2) as f:
        want = run(f)
    assert got[0] == want[0]
    assert _same_bits(got[1], want[1])
    assert sorted(k for k, v in got[2].items() if v) == sorted(k for k, v in want[2].items() if v)


def test_run_ahead_state_across_a_change_of_mask():
    """legs at 129^3: vcycle (runs the next down-leg ahead), set_neumann, cycles -- the reference of one Dirichlet cycle
    followed by Neumann cycles"""
    c, L, faces = 9, 5, 63
    N = _n(c, L)
    rng = np.random.default_rng(13)
    import _screened_ref as S
    dref = S.Problem(c, L, 2, 0.0)
    dref.u[-1][...] = rng.standard_normal((N, N, N))
    dref.d[-1][...] = rng.standard_normal((N, N, N))
    u0, d0 = dref.u[-1].copy(), dref.d[-1].copy()
    first = dref.vcycle()
    ref = R.Problem(c, L, 2, 0.0, None, 0, faces)
    ref.u[-1][...] = dref.u[-1]
    ref.d[-1][...] = dref.d[-1]
    want = [first] + list(ref.vcycles(3))
    with M.Solver(c, L, 2) as s:
        s.set_option("legs", 1)
        s.set_option("legs_min", 66)
        s.get_details()
        s.upload(MG3D_U, L - 1, u0)
        s.upload(MG3D_D, L - 1, d0)
        got = [s.vcycle()]
        s.set_neumann(faces)
        got += list(s.vcycles(2)) + [s.vcycle()]
        assert _same_bits(s.download(MG3D_U, L - 1), ref.flat("u", L - 1))
    np.testing.assert_allclose(got, want, rtol=norm_rtol(N))


def test_argument_and_state_rules():
    with M.Solver(5, 3, 2) as s:
        s.get_details()
        for bad in (-1, 64, 1000):
            with pytest.raises(M.Mg3dError) as e:
                s.set_neumann(bad)
            assert e.value.code == MG3D_ERR_ARG
            assert s.neumann == 0
        with pytest.raises(ValueError):
            s.set_neumann(["imid"])
        s.set_neumann(["jlo", "khi"])
        assert s.neumann == 4 | 32
        s.set_neumann(36)  # the same mask: nothing changes
        for call in (lambda: s.es_setup(), lambda: s.es_vcycles(1), lambda: s.fmg_initialize(),
                     lambda: s.fill_boundary(MG3D_D, 2)):
            with pytest.raises(M.Mg3dError) as e:
                call()
            assert e.value.code == MG3D_ERR_STATE
        # a Neumann bit on a periodic axis: ERR_ARG from whichever setter comes second, nothing changes
        with pytest.raises(M.Mg3dError) as e:
            s.set_periodic(2)
        assert e.value.code == MG3D_ERR_ARG
        assert (s.periodic, s.neumann) == (0, 36)
        s.set_periodic(1)
        with pytest.raises(M.Mg3dError) as e:
            s.set_neumann(36 | 2)
        assert e.value.code == MG3D_ERR_ARG
        assert (s.periodic, s.neumann) == (1, 36)
        s.vcycles(1)
        s.set_periodic(0)
        s.set_neumann(0)
        s.fill_boundary(MG3D_D, 2)
    for c in (3, 4, 6):  # no constraint on c beyond c >= 3
        with M.Solver(c, 3, 2) as s:
            s.set_neumann(63)
            s.get_details()
            assert np.isfinite(s.vcycles(1)).all()
    with M.Solver(5, 3, 2) as s:  # a factor given to set_lu is dropped
        s.get_details()
        n0 = 125
        LU = np.zeros(n0 * n0)
        import _oracle as O
        O.lib().orc_coarse_matrix(O.P(LU), 5, s.level_h(0))
        O.lib().orc_lu_factor(O.P(LU), n0)
        s.set_lu(LU)
        s.set_neumann(1)
        with pytest.raises(M.Mg3dError) as e:
            s.vcycles(1)
        assert e.value.code == MG3D_ERR_STATE
        s.get_details()
        s.vcycles(1)
    with M.Solver(5, 3, 2) as s:  # eps on a Neumann face is read: checked
        s.set_neumann(1)
        eps = np.ones((17, 17, 17))
        eps[0, 3, 3] = -1.0
        with pytest.raises(M.Mg3dError) as e:
            s.set_coefficient(eps)
        assert e.value.code == MG3D_ERR_ARG
        assert not s.has_coefficient()
        eps[0, 3, 3] = 2.0
        s.set_coefficient(eps)
        assert s.coefficient()[0, 3, 3] == 2.0


def _numpy_solution(c, L, axes, faces, sigma, u0, f, cycles):
    ref = R.Problem(c, L, 2, sigma, None, axes, faces)
    ref.u[-1][...] = u0
    ref.d[-1][...] = f
    ref.vcycles(cycles)
    return ref.u[-1]


def test_inhomogeneous_flux_through_fold_flux():
    """u* = exp(x) sin(1 + y) (1 + z - z^2) with prescribed flux on i-low and j-high, Dirichlet elsewhere, 65^3: the
    library reaches the discretisation error of the numpy reference (the same cycles give the same bits), and that error
    is second order: it falls 3.6 .. 4.4 x from 33^3 to 65^3"""
    c, faces = 5, 1 | 8
    errs = []
    for L in (4, 5):
        N = _n(c, L)
        x = np.linspace(0.0, 1.0, N)
        X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
        us = np.exp(X) * np.sin(1 + Y) * (1 + Z - Z * Z)
        f = np.ascontiguousarray(np.exp(X) * np.sin(1 + Y) * (-2.0))  # u_xx + u_yy cancel
        flux = {"ilo": -us[0], "jhi": (np.exp(X) * np.cos(1 + Y) * (1 + Z - Z * Z))[:, -1]}
        u0 = us.copy()
        u0[R.unknown_mask(N, 0, faces)] = 0.
        with _solver(c, L, 2, 0.0, None, 0, faces) as s:
            d = s.fold_flux(f.copy(), flux)
            want_d = R.fold_flux(f.copy(), None, s.h, faces, {0: flux["ilo"], 3: flux["jhi"]})
            assert _same_bits(d, want_d)
            s.upload(MG3D_U, L - 1, u0)
            s.upload(MG3D_D, L - 1, d)
            norms = s.vcycles(14)
            u = s.download(MG3D_U, L - 1).reshape(N, N, N)
        want = _numpy_solution(c, L, 0, faces, 0.0, u0, d, 14)
        assert _same_bits(u, want)
        assert norms[-1] < 1e-9 * norms[0]
        errs.append(np.abs(u - us).max())
    assert 3.6 < errs[0] / errs[1] < 4.4, errs


@pytest.mark.parametrize("axes,faces", [(0, 63), (6, 3)])
def test_singular_case_with_a_compatible_right_hand_side(axes, faces):
    """sigma = 0, every axis closed: with sum(w f) = 0 the cycles converge and u(0,0,0) is the pinned value 0 ... on level
    0; on the finest level the point is an ordinary unknown that the smoother moves, so what is checked there is the
    solution up to a constant"""
    from test_neumann_host import FACTOR_BOUND
    c, L = 5, 5
    N = _n(c, L)
    _, f = R.manufactured(N, axes, faces, 0.0)
    with _solver(c, L, 2, 0.0, None, axes, faces) as s:
        w = s.compatibility_weights()
        assert _same_bits(w, R.weights(N, axes, faces))
        f = f - (w * f).sum() / w.sum()
        R.refresh(f, axes)
        s.upload(MG3D_D, L - 1, f)
        init = s.residual(L - 1, store=False)
        norms = np.concatenate([[init], s.vcycles(16)])
        u = s.download(MG3D_U, L - 1).reshape(N, N, N)
        assert s.download(MG3D_U, 0)[0] == 0.0  # the pinned unknown of level 0
    above = norms[norms > 1e-10 * norms[0]]
    assert (above[1:] / above[:-1]).max() < FACTOR_BOUND, norms
    assert norms[-1] < 1e-10 * norms[0], norms
    # the same cycles of the numpy reference give the same bits: its discretisation error (tests/test_neumann_host.py)
    assert _same_bits(u, _numpy_solution(c, L, axes, faces, 0.0, np.zeros((N, N, N)), f, 16))
