"""The restatements on boxes other than the unit cube (CPU only): every restatement tests/test_gpu_length.py leans on
satisfies the scaling identity of tests/_length_cases.py bit for bit -- grid_length times 2^m, d, sigma, kappa and the
source over 4^m, dt times 4^m: the same u on every level, d below the top, r and every norm exactly 4^-m times, the same
PCG iterates and counts, the gradient 2^-m times, flux and energy 2^m times -- at 17^3, from the base lengths 1.0, 3e-4
and 3.0, with m = 2 and -3, over every operator of the table.  Every compared array is finite and holds no subnormal
(data in +-50 / length^2, |m| <= 3): scaling by a power of two then commutes with every rounding.  Also the closed-form
slab of tests/test_field_ref_host.py on a box of side 3, and that the new grid_length arguments default to the unit cube."""
import numpy as np
import pytest

import _field_ref as FR
import _fmg_ref as FM
import _f32_ref as F32
import _length_cases as LC
import _mask_ref as MR
import _neumann_ref as NR
import _pcg_ref as PR
import _step_ref as SR
import _wpcg_ref as WR
from test_field_ref_host import slab_problem

C_, L_, NU = 5, 3, 2
N = LC.n_of(C_, L_)
DT, KAPPA = 0.01, 0.75
CASES = [(name, length) for name in LC.OPERATORS for length in LC.HOST_LENGTHS]


def _assert_scaled(got, base, factor, what):
    """got == factor * base bit for bit (factor a power of two), both normal"""
    got, base = np.asarray(got), np.asarray(base)
    assert LC.normal(got) and LC.normal(base), what
    assert LC.same_bits(got, base * factor), what


def _cycles(name, length, m):
    f = 4.0 ** m
    sg = LC.OPERATORS[name][0]
    ref = LC.reference(name, C_, L_, NU, length * 2.0 ** m, sigma=sg / f)
    u, d = LC.data(name, N, length, 1)
    ref.u[-1][...] = u
    ref.d[-1][...] = d / f
    norms = np.concatenate([ref.vcycles(1), ref.vcycles(2)])
    return ref, norms


@pytest.mark.parametrize("name,length", CASES)
def test_vcycles(name, length):
    base, bn = _cycles(name, length, 0)
    assert base.h == length / (N - 1) and base.level_h(0) == base.h * 4
    for m in LC.MS:
        ref, norms = _cycles(name, length, m)
        assert ref.h == base.h * 2.0 ** m
        for l in range(L_):
            _assert_scaled(ref.u[l], base.u[l], 1.0, (name, m, "u", l))
            _assert_scaled(ref.r[l], base.r[l], 4.0 ** -m, (name, m, "r", l))
        for l in range(L_ - 1):
            _assert_scaled(ref.d[l], base.d[l], 4.0 ** -m, (name, m, "d", l))
        _assert_scaled(norms, bn, 4.0 ** -m, (name, m, "norms"))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("length", LC.HOST_LENGTHS)
def test_krylov(weighted, length):
    """_pcg_ref.pcg / _wpcg_ref.wpcg / _mask_ref.wpcg, three iterations, exactly rounded and pairwise sums alike"""
    for name in (LC.WPCG_OPERATORS if weighted else LC.PCG_OPERATORS):
        x0, d = LC.krylov_data(name, N, length)
        for dots in ("exact", "plain"):
            bh, bn = LC.krylov(name, C_, L_, length, x0, d, 3, dots, weighted)
            assert len(bh) == 3
            for m in LC.MS:
                # sigma scales with d: the table's sigma belongs to the base run
                hist, norms = _krylov_scaled(name, length, m, x0, d, dots, weighted)
                assert len(hist) == len(bh)
                for k in range(3):
                    _assert_scaled(hist[k], bh[k], 1.0, (name, m, dots, "x", k))
                _assert_scaled(norms, bn, 4.0 ** -m, (name, m, dots, "norms"))


def _krylov_scaled(name, length, m, x0, d, dots, weighted):
    f = 4.0 ** m
    sg, eps, axes, faces, mask = LC.operator(name, N)
    hist = []
    gl = length * 2.0 ** m
    if not weighted:
        _, norms, _ = PR.pcg(PR.make_problem(C_, L_, NU, sg / f, eps, axes, gl), x0, d / f, 0., 1e-300, 3, dots, hist)
    elif mask is not None:
        _, norms, _, mean, _ = MR.wpcg(LC.reference(name, C_, L_, NU, gl, sg / f), x0, d / f, 0., 1e-300, 3, dots, hist)
    else:
        _, norms, _, mean = WR.wpcg(WR.make_problem(C_, L_, NU, sg / f, eps, axes, faces, gl), x0, d / f, 0., 1e-300, 3, dots, hist)
    return hist, norms


def _advance(name, length, m, theta, src, method):
    f = 4.0 ** m
    dt, kappa = DT * length * length * f, KAPPA / (length * length) / f
    ref = LC.reference(name, C_, L_, NU, length * 2.0 ** m, sigma=SR.sigma_of(dt, theta, kappa))
    u0, s = LC.data(name, N, length, 2)
    ref.u[-1][...] = u0
    adv = MR.advance if hasattr(ref, "mask") else SR.advance
    norms, iters, conv = adv(ref, 2, 2, s / f if src else None, dt, theta, kappa, method=method, rtol=0.0)
    return ref, norms, iters


@pytest.mark.parametrize("name,length", CASES)
def test_step(name, length):
    """_step_ref.advance (_mask_ref.advance over the masked hierarchy): two steps, theta 1 and 0.5, with and without a
    source, by V-cycles and by weighted PCG; dt = 0.01 length^2 and kappa = 0.75 / length^2 at the base"""
    for theta in (1.0, 0.5):
        for src in (True, False):
            for method in ("vcycles", "wpcg"):
                base, bn, bi = _advance(name, length, 0, theta, src, method)
                for m in LC.MS:
                    ref, norms, iters = _advance(name, length, m, theta, src, method)
                    what = (name, m, theta, src, method)
                    _assert_scaled(ref.u[-1], base.u[-1], 1.0, what)
                    blk = NR.block(N, ref.axes, ref.faces)
                    if method == "vcycles":
                        _assert_scaled(ref.d[-1][blk], base.d[-1][blk], 4.0 ** -m, what)
                    _assert_scaled(norms, bn, 4.0 ** -m, what)
                    assert iters == bi


def _fmg(name, length, m):
    f = 4.0 ** m
    sg = LC.OPERATORS[name][0]
    ref = LC.reference(name, C_, L_, NU, length * 2.0 ** m, sigma=sg / f)
    u, d = LC.data(name, N, length, 3)
    ref.u[-1][...] = u
    ref.d[-1][...] = d / f
    norm = FM.fmg_solve(ref, 2)
    return ref, norm


@pytest.mark.parametrize("name,length", [c for c in CASES if not LC.OPERATORS[c[0]][4]])
def test_fmg_and_field(name, length):
    """_fmg_ref.fmg_solve(2), then _field_ref.gradient and energy of its u"""
    base, bn = _fmg(name, length, 0)
    eps = base.e(L_ - 1)
    bg = FR.gradient(base.u[-1], base.h, base.axes, base.faces, -1.0)
    bw = FR.energy(base.u[-1], eps, base.h, base.axes, base.faces)
    for m in LC.MS:
        ref, norm = _fmg(name, length, m)
        _assert_scaled(ref.u[-1], base.u[-1], 1.0, (name, m, "u"))
        _assert_scaled([norm], [bn], 4.0 ** -m, (name, m, "norm"))
        g = FR.gradient(ref.u[-1], ref.h, ref.axes, ref.faces, -1.0)
        for a in range(3):
            _assert_scaled(g[a], bg[a], 2.0 ** -m, (name, m, "gradient", a))
        _assert_scaled([FR.energy(ref.u[-1], eps, ref.h, ref.axes, ref.faces)], [bw], 2.0 ** m, (name, m, "energy"))


@pytest.mark.parametrize("length", LC.HOST_LENGTHS)
def test_flux_of_the_masked_operator(length):
    """_field_ref.flux and energy of the masked hierarchy's u after three cycles: 2^m times"""
    name = "sphere_f1"
    base, _ = _cycles(name, length, 0)
    mask = base.mask[-1]
    bf = FR.flux(base.u[-1], None, mask, base.h, base.axes, base.faces)
    bw = FR.energy(base.u[-1], None, base.h, base.axes, base.faces)
    assert bf != 0.
    for m in LC.MS:
        ref, _ = _cycles(name, length, m)
        _assert_scaled([FR.flux(ref.u[-1], None, mask, ref.h, ref.axes, ref.faces)], [bf], 2.0 ** m, m)
        _assert_scaled([FR.energy(ref.u[-1], None, ref.h, ref.axes, ref.faces)], [bw], 2.0 ** m, m)


@pytest.mark.parametrize("length", LC.HOST_LENGTHS)
def test_f32_restatement(length):
    """_f32_ref.run_cycles with the new argument: binary32 u of every level the same bits, d below the top 4^-m times
    (the division of a binary32 d by 4^m is exact), the exactly rounded norm 4^-m times"""
    u0, d0, r0 = F32.random_start(C_, L_, 7)
    d0 = (d0 * np.float32(50.0 / (length * length))).astype(np.float32)
    r0 = (r0 / np.float32(length * length)).astype(np.float32)
    base = F32.run_cycles(C_, L_, NU, 2, u0, d0, r0, length)
    for m in LC.MS:
        f = np.float32(4.0 ** m)
        got = F32.run_cycles(C_, L_, NU, 2, u0, d0 / f, r0 / f, length * 2.0 ** m)
        for a, b in zip(got, base):
            _assert_scaled(a.u_top, b.u_top, np.float32(1.0), (m, "u top"))
            for l in range(L_ - 1):
                _assert_scaled(a.u_low[l], b.u_low[l], np.float32(1.0), (m, "u", l))
                _assert_scaled(a.d_low[l], b.d_low[l], np.float32(1.0) / f, (m, "d", l))
            _assert_scaled([a.norm], [b.norm], 4.0 ** -m, (m, "norm"))


def test_f32_restatement_default_is_the_unit_cube():
    u0, d0, r0 = F32.random_start(C_, L_, 7)
    a = F32.run_cycles(C_, L_, NU, 1, u0, d0, r0)[0]
    b = F32.run_cycles(C_, L_, NU, 1, u0, d0, r0, 1.0)[0]
    assert F32.same_bits(a.u_top, b.u_top) and a.norm == b.norm
    assert np.array_equal(F32.coarse_lu(C_, L_), F32.coarse_lu(C_, L_, 1.0))
    assert not np.array_equal(F32.coarse_lu(C_, L_), F32.coarse_lu(C_, L_, 3.0))


def test_make_problem_forwards_the_length():
    for make in (lambda **k: PR.make_problem(C_, L_, NU, **k), lambda **k: PR.make_problem(C_, L_, NU, axes=7, **k),
                 lambda **k: WR.make_problem(C_, L_, NU, faces=22, **k), lambda **k: SR.make_problem(C_, L_, NU, DT, 0.5, KAPPA, **k)):
        assert make().h == 1.0 / (N - 1)
        assert make(grid_length=3.0).h == 3.0 / (N - 1)
        assert not np.array_equal(make().LU, make(grid_length=3.0).LU)


def test_gradient_scales_tell_the_factor_forms_apart():
    """the header's cs = scale * (0.5 / h) against scale / (2 h): at every non-dyadic h of tests/test_gpu_length.py one of
    GRAD_SCALES gives another double (0.5 / h and 1 / (2 h) themselves are the same number: 2 h is exact)"""
    for length in LC.LENGTHS:
        for n in list(LC.SIZES) + [129]:
            h = length / (n - 1)
            assert 0.5 / h == 1.0 / (2.0 * h)
            assert any(s * (0.5 / h) != s / (2.0 * h) for s in LC.GRAD_SCALES), (length, n)


def test_slab_problem_on_a_box_of_side_three():
    """tests/test_field_ref_host.slab_problem on a box of side 3: u rises from 0 to 1 over 12 h = 2.25, across a section
    of 3 x 3.  From the header: *flux = h * sum t_p, t_p = u_11 - u_12 = -1/12 at the 16 x 16 unique points of plane 12
    (zero inside the body): F = -(3/16) * 256 / 12 = -4 -- the section 9 times the slope 1/2.25; *energy = 0.5 * h * (12
    planes of 256 edges of (1/12)^2) = 2 -- 1/2 * slope^2 * volume 9 * 2.25; W = -1/2 V F"""
    axes, faces, _, u, mask = slab_problem()
    h = 3.0 / 16
    F = FR.flux(u, None, mask, h, axes, faces, 3)
    W = FR.energy(u, None, h, axes, faces)
    assert abs(F + 4.0) <= 1e-12 and abs(W - 2.0) <= 1e-12
    assert abs(W + 0.5 * F) <= 1e-12
