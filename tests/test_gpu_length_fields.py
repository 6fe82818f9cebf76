"""The screening field (mg3d_ctx_set_shift_field) and the KEEP coarsening rule with masked full multigrid on boxes other than
the unit cube (grid_length 3e-4 and 3.0): the sibling of tests/test_gpu_length.py for the features merged after it, with
its lengths, data (u in (-1, 1), d in (-50, 50) / length^2), tolerances and its part C.

B  against the restatements called with this length -- _shift_field_ref.Hierarchy(..., grid_length),
   _mask_keep_ref.Hierarchy / FieldHierarchy(..., grid_length) -- over pruned matrices in which every boundary set meets
   both lengths and the sizes rotate:
   screening field, the boundaries of tests/test_gpu_shift_field.py at 17^3, 33^3 and 37^3, the field random in [0, 1/h^2]
   with this length's h (so s*hSq weighs as on the unit cube): the restricted field of every level, one pass of each
   colour, the residual, two V-cycles, u of every level bit for bit; plain, with eps, with a mask, with set_shift on top;
   mg3d_step_advance (one step) and mg3d_fmg_solve against _shift_field_ref.step_rhs / fmg_solve.
   KEEP, _mask_keep_ref.thin_mask at 17^3, 25^3 = (7, 3) and 33^3 under the boundaries FEW of tests/test_gpu_mask_keep.py:
   the mask bytes of every level, two cycles (u of every level, d below the top), masked FMG with two cycles per level
   (its inner levels run _mask_keep_ref.vcycle_keep_guess); constant, eps with sigma, a screening field.
   Norms at the NORM_RTOL / SUM_RTOL of tests/test_gpu_length.py.

   mg3d_pcg_solve / mg3d_wpcg_solve with a screening field and under KEEP, three iterations.  What a summation order is
   worth at these lengths and data was measured on the CPU (python tests/_length_cases.py, its "field/keep" lines: two
   restatement runs, exactly rounded sums against numpy's pairwise float64 sums, largest over the cases of
   LC.FIELD_KRYLOV of that call, 17^3 and 33^3, both lengths), as max|a - b| / max|a| of x_k and of the norms:
       pcg_solve   k = 1: 4.43e-16   k = 2: 8.25e-16   k = 3: 6.49e-16   norms: 1.84e-15
       wpcg_solve  k = 1: 5.12e-15   k = 2: 1.51e-14   k = 3: 1.45e-14   norms: 5.87e-15
   (a strongly screened or pinned-down operator is well conditioned: the spread stays near rounding).  The GPU, a third
   order, is allowed 100 times the figure, and never less than 100 times the figure tests/test_gpu_pcg.py /
   tests/test_gpu_wpcg.py hold the same call to, which is the larger one here throughout (those files measure k = 1, 2
   and 5: k = 3 takes their k = 2 figure, the tighter neighbour).

C  the scaling identity between GPU runs at 129^3, base length 3e-4, m = 2 and -3: grid_length times 2^m, d, sigma and
   the field s(x) over 4^m -- u of every level the same bits, d below the top, the stored field of every level and every
   norm exactly 4^-m times, the mask bytes of every level equal -- for one screening-field operator and one KEEP operator.
   The base is pinned by part B at the smaller sizes; the coarsest level is solved again on the CPU with the factor of
   the coarsest spacing."""
import numpy as np
import pytest
import torch  # noqa: F401  (before the package, as bench.py does: the HIP runtime is torch's)

import _coef_ref as CR
import _length_cases as LC
import _mask_keep_ref as MK
import _mask_ref as MR
import _neumann_ref as NR
import _shift_field_ref as SF
import _step_ref as SR
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U
import test_gpu_pcg as TP
import test_gpu_wpcg as TW
from test_gpu_length import NORM_RTOL, SUM_RTOL, _assert_spacings
from test_gpu_mask_keep import FEW
from test_gpu_shift_field import BOUNDARIES

pytestmark = pytest.mark.gpu

same_bits = LC.same_bits
# measured, see above: {k: spread of x_k}, spread of the norms
SPREAD = {"pcg_solve": ({1: 4.43e-16, 2: 8.25e-16, 3: 6.49e-16}, 1.84e-15),
          "wpcg_solve": ({1: 5.12e-15, 2: 1.51e-14, 3: 1.45e-14}, 5.87e-15)}
FLOOR = {"pcg_solve": ({1: TP.SPREAD_U[1], 2: TP.SPREAD_U[2], 3: TP.SPREAD_U[2]}, TP.SPREAD_NORM),
         "wpcg_solve": ({1: TW.SPREAD_U[1], 2: TW.SPREAD_U[2], 3: TW.SPREAD_U[2]}, TW.SPREAD_NORM)}
KEEP_SIZES = {17: (5, 3), 25: (7, 3), 33: (5, 4)}
SF_VARIANTS = ("plain", "eps", "mask", "sigma")
KEEP_VARIANTS = ("const", "eps", "sfield")


def _rotated(boundaries, sizes, variants):
    """(axes, faces, N, length, variant): every boundary set meets both lengths, the sizes and the variants rotate (no
    periodic axis at 37^3: c - 1 odd), as _pruned of tests/test_gpu_length.py"""
    out = []
    for i, (axes, faces) in enumerate(boundaries):
        for j, length in enumerate(LC.LENGTHS):
            ok = [n for n in sizes if not (n == 37 and axes)]
            N, v = ok[(i + j) % len(ok)], variants[(i + j) % len(variants)]
            out.append(pytest.param(axes, faces, N, length, v, id=f"a{axes}-f{faces}-{N}-{length:g}-{v}"))
    return out


def _data(N, length, axes, seed):
    rng = np.random.default_rng(seed)
    u = rng.uniform(-1, 1, (N, N, N))
    d = rng.uniform(-50, 50, (N, N, N)) / (length * length)
    NR.refresh(u, axes)
    NR.refresh(d, axes)
    return u, d


def _solver(c, L, length, sigma, eps, axes, faces, mask, field, rule=None):
    s = M.Solver(c, L, 2, grid_length=length)
    _assert_spacings(s, c, L, length)
    s.set_shift(sigma)
    s.set_periodic(axes)
    s.set_neumann(faces)
    if eps is not None:
        s.set_coefficient(eps)
    if field is not None:
        s.set_shift_field(field)
    if rule is not None:
        s.set_mask_coarsening(rule)
    if mask is not None:
        s.set_mask(mask)
    s.get_details()
    return s


def _assert_levels(s, ref, what=""):
    for l in range(ref.L):
        assert same_bits(s.download(MG3D_U, l), ref.u[l].reshape(-1)), f"{what} u level {l}"
    for l in range(ref.L - 1):
        assert same_bits(s.download(MG3D_D, l), ref.d[l].reshape(-1)), f"{what} d level {l}"


def _assert_norms(got, want, what):
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    print(*what, "norms", got, np.abs(got - want) / want)
    np.testing.assert_allclose(got, want, rtol=NORM_RTOL)


# ======================================================================================================= B: the field
@pytest.mark.parametrize("axes,faces,N,length,variant", _rotated(BOUNDARIES, (17, 33, 37), SF_VARIANTS))
def test_screening_field(axes, faces, N, length, variant):
    c, L = LC.SIZES[N]
    h = length / (N - 1)
    field = SF.random_field(N, h)
    assert field.max() <= 1.0 / (h * h) and field.max() > 0.9 / (h * h)
    sigma = 0.75 / (length * length) if variant == "sigma" else 0.0
    eps = CR.FIELDS["exp"](N) if variant == "eps" else None
    mask = MR.gpu_test_mask(N) if variant == "mask" else None
    ref = SF.Hierarchy(c, L, 2, sigma, eps, axes, faces, mask, field, grid_length=length)
    rng = np.random.default_rng(N + faces + 64 * axes)
    dscale = 50.0 / (length * length)
    what = (axes, faces, N, length, variant)
    with _solver(c, L, length, sigma, eps, axes, faces, mask, field) as s:
        assert s.has_shift_field() and s.h == ref.h
        for l in range(L):
            assert s.level_h(l) == ref.level_h(l)
            assert same_bits(s.get_shift_field(l), ref.s[l]), f"the restricted field of level {l}"
        for l in (L - 1, L - 2):
            n, hl, e, m, f = ref.N[l], ref.level_h(l), ref.e(l), ref.mask[l], ref.s[l]
            u, d = rng.uniform(-1, 1, (n, n, n)), rng.uniform(-1, 1, (n, n, n)) * dscale
            NR.refresh(u, axes)
            s.upload(MG3D_U, l, u)
            s.upload(MG3D_D, l, d)
            s.smooth(l, 0, 1)
            for colour in (1, 0):
                SF.colour_pass(u, d, e, hl, sigma, axes, faces, colour, m, f)
            assert same_bits(s.download(MG3D_U, l).reshape(n, n, n), u), f"one pass of each colour (pre), level {l}"
            s.smooth(l, 1, 1)
            for colour in (0, 1):
                SF.colour_pass(u, d, e, hl, sigma, axes, faces, colour, m, f)
            assert same_bits(s.download(MG3D_U, l).reshape(n, n, n), u), f"one pass of each colour (post), level {l}"
            r = rng.uniform(-1, 1, (n, n, n))
            s.upload(MG3D_R, l, r)
            got = s.residual(l, store=True)
            SF.residual(u, d, e, hl, sigma, axes, faces, m, f, r)
            assert same_bits(s.download(MG3D_R, l).reshape(n, n, n), r), f"residual, level {l}"
            exact = SF.exact_residual_norm(u, d, e, hl, sigma, axes, faces, m, f)
            print(*what, l, "residual norm", got, exact, abs(got - exact) / exact)
            assert abs(got - exact) <= SUM_RTOL * exact
        for l in range(L):
            s.zero(MG3D_R, l)
        u, d = _data(N, length, axes, N)
        ref.u[-1][...] = u
        ref.d[-1][...] = d
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        want = ref.vcycles(2)
        got = s.vcycles(2)
        _assert_levels(s, ref, "after two cycles:")
        _assert_norms(got, want, what)
        assert LC.normal(ref.u[-1]) and ref.u[-1].any()


@pytest.mark.parametrize("length", LC.LENGTHS)
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_screening_field_step_advance(theta, length):
    """one step with a source at 17^3 (periodic k, Neumann i faces, eps): d at the unknowns is _shift_field_ref.step_rhs with
    the field in q, u after the step's two cycles bit for bit; dt = 1e-3 length^2, kappa = 2 / length^2"""
    c, L, N = 5, 3, 17
    axes, faces = 4, 3
    dt, kappa = 1e-3 * length * length, 2.0 / (length * length)
    eps = CR.FIELDS["exp"](N)
    field = SF.random_field(N, length / (N - 1))
    u0, src = _data(N, length, axes, 17)
    prob = SF.Hierarchy(c, L, 2, SR.sigma_of(dt, theta, kappa), eps, axes, faces, None, field, grid_length=length)
    prob.u[-1][...] = u0
    SF.write_rhs(prob, src, dt, theta, kappa)
    want_d = prob.d[-1].copy()
    want_n = prob.vcycles(2)
    with _solver(c, L, length, 0.0, eps, axes, faces, None, field) as s:
        s.step_setup(dt, theta, kappa)
        assert s.get_shift() == prob.sigma
        s.step_set_source(src)
        s.upload(MG3D_U, L - 1, u0)
        s.zero(MG3D_D, L - 1)
        norms, info = s.step_advance(1, cycles=2, method="vcycles")
        assert info["steps"] == 1 and info["time"] == dt
        blk = NR.block(N, axes, faces)
        assert same_bits(s.download(MG3D_D, L - 1).reshape(N, N, N)[blk], want_d[blk])
        assert same_bits(s.download(MG3D_U, L - 1), prob.u[-1].reshape(-1))
    _assert_norms(norms, want_n[-1:], ("step", theta, length))


@pytest.mark.parametrize("length", LC.LENGTHS)
@pytest.mark.parametrize("axes,faces,N", [(0, 0, 37), (4, 3, 33)])
def test_screening_field_fmg_solve(axes, faces, N, length):
    c, L = LC.SIZES[N]
    sigma = 0.5 / (length * length)
    field = SF.random_field(N, length / (N - 1))
    prob = SF.Hierarchy(c, L, 2, sigma, None, axes, faces, None, field, grid_length=length)
    u, d = _data(N, length, axes, 13)
    prob.u[-1][...] = u
    prob.d[-1][...] = d
    want = SF.fmg_solve(prob, 1)
    with _solver(c, L, length, sigma, None, axes, faces, None, field) as s:
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        got = s.fmg_solve(1)
        assert same_bits(s.download(MG3D_U, L - 1), prob.u[-1].reshape(-1))
        assert same_bits(s.download(MG3D_D, L - 1), d.reshape(-1))
    _assert_norms(got, want, ("fmg", axes, faces, N, length))


# ========================================================================================================== B: KEEP
def _keep_reference(c, L, length, sigma, eps, axes, faces, mask, field):
    if field is not None:
        return MK.FieldHierarchy(c, L, 2, sigma, eps, axes, faces, mask, field, grid_length=length)
    return MK.Hierarchy(c, L, 2, sigma, eps, axes, faces, mask, grid_length=length)


@pytest.mark.parametrize("axes,faces,N,length,variant", _rotated(FEW, (17, 25, 33), KEEP_VARIANTS))
def test_keep(axes, faces, N, length, variant):
    """the mask bytes of every level, two cycles and (without a field: mg3d_fmg_solve refuses the pair) masked full
    multigrid with two cycles per level -- d at the fixed points poisoned with NaN"""
    c, L = KEEP_SIZES[N]
    sigma = 3.5 / (length * length) if variant == "eps" else 0.0
    eps = CR.FIELDS["exp"](N) if variant == "eps" else None
    field = SF.random_field(N, length / (N - 1)) if variant == "sfield" else None
    mask = MK.thin_mask(N)
    ref = _keep_reference(c, L, length, sigma, eps, axes, faces, mask, field)
    u, d = _data(N, length, axes, N + faces)
    d[ref.fixed()] = np.nan
    what = (axes, faces, N, length, variant)
    with _solver(c, L, length, sigma, eps, axes, faces, mask, field, rule="keep") as s:
        for l in range(L):
            assert np.array_equal(s.get_mask(l), ref.mask[l]), f"the mask of level {l}"
            assert s.level_h(l) == ref.level_h(l)
        ref.u[-1][...] = u
        ref.d[-1][...] = d
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        want = ref.vcycles(2)
        got = s.vcycles(2)
        _assert_levels(s, ref, "after two cycles:")
        _assert_norms(got, want, what)
        fx = ref.fixed()
        assert fx.any() and same_bits(s.download(MG3D_U, L - 1).reshape(N, N, N)[fx], u[fx])
        for l in range(L):
            assert np.array_equal(s.get_mask(l), ref.mask[l]), f"the mask of level {l} after the cycles"
        if field is not None:
            return
        ref.u[-1][...] = u
        ref.d[-1][...] = d
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        want = MK.fmg_solve(ref, 2)
        got = s.fmg_solve(2)
        gu = s.download(MG3D_U, L - 1).reshape(N, N, N)
        assert np.isfinite(gu).all() and same_bits(gu, ref.u[-1]), "masked FMG"
        assert same_bits(gu[fx], u[fx])
        assert s.download(MG3D_D, L - 1).tobytes() == d.tobytes(), "d is the caller's, its NaN at the fixed points included"
        _assert_norms(got, want, what + ("fmg",))


# ======================================================================================================== B: Krylov
def _krylov_cases():
    out = []
    for i, name in enumerate(LC.FIELD_KRYLOV):
        for j, length in enumerate(LC.LENGTHS):
            N = LC.FIELD_KRYLOV_SIZES[(i + j) % len(LC.FIELD_KRYLOV_SIZES)]
            out.append(pytest.param(name, N, length, id=f"{name}-{N}-{length:g}"))
    return out


@pytest.mark.parametrize("name,N,length", _krylov_cases())
def test_krylov(name, N, length):
    """x_k and the norms r_0 .. r_k for k = 1, 2, 3 against the restatement with exactly rounded sums: 100 x the spread
    measured on the CPU at these lengths (the docstring of this file), never below the two solver files' own figures"""
    call, axes, faces = LC.FIELD_KRYLOV[name][:3]
    c, L = LC.SIZES[N]
    make, x0, d, eps, field, mask = LC.field_krylov_problem(name, N, length)
    prob = make()
    hist, ref_norms = LC.field_krylov(prob, x0, d, LC.PCG_ITERS, "exact")
    fx = prob.fixed()  # (of the stored mask: a periodic duplicate holds its source's byte)
    (su, sn), (fu, fn) = SPREAD[call], FLOOR[call]
    with _solver(c, L, length, 0.0, eps, axes, faces, mask, field, rule="keep" if mask is not None else None) as s:
        s.upload(MG3D_D, L - 1, d)
        for k in (1, 2, 3):
            s.upload(MG3D_U, L - 1, x0)
            norms, info = getattr(s, call)(rtol=0.0, atol=1e-300, max_iters=k)
            assert info["iterations"] == k and len(norms) == k + 1
            u = s.download(MG3D_U, L - 1).reshape(N, N, N)
            rel = np.abs(u - hist[k - 1]).max() / np.abs(hist[k - 1]).max()
            nrel = (np.abs(norms - ref_norms[:k + 1]) / ref_norms[:k + 1]).max()
            print(name, N, length, k, "u", rel, "norms", nrel)
            assert rel <= 100 * max(su[k], fu[k]), (k, rel)
            assert nrel <= 100 * max(sn, fn), (k, nrel)
            if mask is not None:
                assert fx.any() and same_bits(u[fx], x0[fx])


# ================================================================================================================ C
def _scaled_equal(got, base, factor, what):
    got, base = np.asarray(got), np.asarray(base)
    assert LC.normal(got) and LC.normal(base), what
    assert same_bits(got, base * factor), what


@pytest.mark.parametrize("case", ["field", "keep"])
def test_identity_between_gpu_runs(case):
    """129^3 = (9, 5), base length 3e-4, calls of one and two cycles.  field: periodic k, Neumann i faces, sigma on top of
    the field.  keep: Neumann ILO | JHI, the thin mask under KEEP with eps and a field"""
    c, L, length = 9, 5, 3e-4
    N = LC.n_of(c, L)
    h = length / (N - 1)
    field = SF.random_field(N, h)
    if case == "field":
        axes, faces, eps, mask, rule = 4, 3, None, None, None
    else:
        axes, faces, eps, mask, rule = 0, 1 | 8, CR.FIELDS["exp"](N), MK.thin_mask(N), "keep"
    sigma = 3.5 / (length * length)
    u, d = _data(N, length, axes, 91)
    if mask is not None:
        d[MR.fixed(MR.stored(mask, axes), axes, faces)] = 0.0

    def run(m):
        f = 4.0 ** m
        with _solver(c, L, length * 2.0 ** m, sigma / f, eps, axes, faces, mask, field / f, rule=rule) as s:
            s.upload(MG3D_U, L - 1, u)
            s.upload(MG3D_D, L - 1, d / f)
            norms = np.concatenate([s.vcycles(1), s.vcycles(2)])
            out = (norms, [s.download(MG3D_U, l) for l in range(L)], [s.download(MG3D_D, l) for l in range(L - 1)],
                   [s.get_shift_field(l) for l in range(L)], [s.get_mask(l) for l in range(L)] if mask is not None else [])
            if m == 0:  # the coarsest level's solve, with the factor of the COARSEST spacing
                s0, m0 = out[3][0].reshape(c, c, c), (out[4][0] if mask is not None else None)
                e0 = None if eps is None else eps[::1 << (L - 1), ::1 << (L - 1), ::1 << (L - 1)]
                LU = SF.coarse_lu(c, h * (1 << (L - 1)), e0, sigma, axes, faces, m0, s0)
                want = np.zeros((c, c, c))
                SF.coarse_solve(LU, out[2][0].reshape(c, c, c), want, axes, faces, False, m0)
                assert same_bits(out[1][0].reshape(c, c, c), want), "the coarsest level's solve"
            return out

    bn, bu, bd, bs, bm = run(0)
    want_s = SF.restrict_field(field, L, axes, faces)
    for l in range(L):
        assert same_bits(bs[l], want_s[l]), f"the restricted field of level {l}"
    if mask is not None:
        want_m = MK.keep(MR.stored(mask, axes), L, axes)
        for l in range(L):
            assert np.array_equal(bm[l], want_m[l]), f"the mask of level {l}"
    for m in LC.MS:
        norms, gu, gd, gs, gm = run(m)
        for l in range(L):
            _scaled_equal(gu[l], bu[l], 1.0, (m, "u", l))
            _scaled_equal(gs[l], bs[l], 4.0 ** -m, (m, "field", l))
        for l in range(L - 1):
            _scaled_equal(gd[l], bd[l], 4.0 ** -m, (m, "d", l))
        _scaled_equal(norms, bn, 4.0 ** -m, (m, "norms"))
        for a, b in zip(gm, bm):
            assert np.array_equal(a, b), (m, "mask")
