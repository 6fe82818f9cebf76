"""The screening field (mg3d_ctx_set_shift_field) without a GPU: the numpy restatement tests/_shift_field_ref.py against
tests/_mask_ref.py (no field: bit for bit) and against itself (the two neutrality statements of include/mg3d.h), the
library's coarse matrix (mg3d_coarse_matrix_field) against the restatement, the restriction of the field, the pin rule,
second-order convergence with a smooth field, the symmetry of the restated preconditioner, and the exported symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _coef_ref as CR
import _fmg_ref as FR
import _mask_ref as MR
import _neumann_ref as NR
import _shift_field_ref as SF
import _wpcg_ref as WR
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import P

UB = C.POINTER(C.c_ubyte)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dp(a):
    return None if a is None else P(np.ascontiguousarray(a, dtype=np.float64).reshape(-1))


def _lib_matrix(N, h, e, sigma, axes, faces, mask, s):
    A = np.zeros(N ** 6)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
    M.lib().mg3d_coarse_matrix_field(P(A), N, h, _dp(e), sigma, axes, faces, None if m is None else m.ctypes.data_as(UB), _dp(s))
    return A


def _lib_mask_matrix(N, h, e, sigma, axes, faces, mask):
    A = np.zeros(N ** 6)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
    M.lib().mg3d_coarse_matrix_mask(P(A), N, h, _dp(e), sigma, axes, faces, None if m is None else m.ctypes.data_as(UB))
    return A


def _eps(N, seed=1):
    return np.random.default_rng(seed).uniform(0.5, 4.0, (N, N, N))


# (periodic axes, Neumann faces): axes 0, 7 and 4, faces 0, 63 and 3, in every combination the two setters accept
BCS = [(0, 0), (0, 63), (0, 3), (7, 0), (4, 0), (4, 3)]


@pytest.mark.parametrize("N", [5, 7])
@pytest.mark.parametrize("axes,faces", BCS)
@pytest.mark.parametrize("field", ["const", "eps"])
@pytest.mark.parametrize("masked", [False, True])
def test_coarse_matrix_field_equals_numpy(N, axes, faces, field, masked):
    """byte for byte, sigma 0 and 3.5, a random field and one with a single positive entry (the pin's edge); s = NULL is
    mg3d_coarse_matrix_mask; identity rows exactly where the restatement's rule puts them"""
    e = _eps(N) if field == "eps" else None
    h = 0.125
    rng = np.random.default_rng(N + axes + faces)
    mask = (rng.uniform(size=(N, N, N)) < 0.15).astype(np.uint8) if masked else None
    one = np.zeros((N, N, N))
    one[2, 1, 3] = 0.75
    face_only = np.where(NR.unknown_mask(N, axes, faces), 0.0, 2.0)  # positive on no unknown: the pin stays
    for sigma in (0.0, 3.5):
        assert _lib_matrix(N, h, e, sigma, axes, faces, mask, None).tobytes() == \
            _lib_mask_matrix(N, h, e, sigma, axes, faces, mask).tobytes()
        for s in (rng.uniform(0.0, 1.0 / (h * h), (N, N, N)), one, face_only, np.zeros((N, N, N))):
            got, want = _lib_matrix(N, h, e, sigma, axes, faces, mask, s), SF.coarse_matrix(N, h, e, sigma, axes, faces, mask, s)
            assert got.tobytes() == want.tobytes()
            A = got.reshape(N ** 3, N ** 3)
            ident = (A == np.eye(N ** 3)).all(axis=1).reshape(N, N, N)
            unk = NR.unknown_mask(N, axes, faces)
            if mask is not None:
                unk &= ~MR.fixed(mask, axes, faces)
            if SF.pinned(axes, faces, sigma, mask, s):
                unk[0, 0, 0] = False
            assert np.array_equal(ident, ~unk)


@pytest.mark.parametrize("axes,faces", BCS)
def test_zero_field_with_eps_and_null_field_agree_on_the_matrix(axes, faces):
    """D + (sigma + 0.0)*hSq is D + sigma*hSq: with eps an all-zero field writes the bytes of no field; without eps the
    field's matrix is that of eps = 1 everywhere with the same field"""
    N, h = 5, 0.25
    e = _eps(N)
    s = np.random.default_rng(2).uniform(0.0, 9.0, (N, N, N))
    for sigma in (0.0, 3.5):
        assert _lib_matrix(N, h, e, sigma, axes, faces, None, np.zeros((N, N, N))).tobytes() == \
            _lib_matrix(N, h, e, sigma, axes, faces, None, None).tobytes()
        assert _lib_matrix(N, h, None, sigma, axes, faces, None, s).tobytes() == \
            _lib_matrix(N, h, np.ones((N, N, N)), sigma, axes, faces, None, s).tobytes()


def _cycles(prob, u, d, count=2):
    prob.u[-1][...] = u
    prob.d[-1][...] = d
    return prob.vcycles(count)


def _same(a, b):
    for l in range(a.L):
        for x, y in ((a.u[l], b.u[l]), (a.d[l], b.d[l]), (a.r[l], b.r[l])):
            if not (np.array_equal(x, y) and np.array_equal(np.signbit(x), np.signbit(y))):
                return False
    return True


@pytest.mark.parametrize("axes,faces", [(0, 0), (5, 0), (0, 10), (4, 3)])
@pytest.mark.parametrize("field", ["const", "eps"])
def test_no_field_reproduces_the_mask_reference(axes, faces, field):
    """s = None: every function is _mask_ref's, bit for bit -- two cycles, (w)PCG, the stepper's d, full multigrid"""
    c, L, N = 5, 3, 17
    rng = np.random.default_rng(7)
    e = _eps(N) if field == "eps" else None
    mask = MR.random_mask(N, 0.05, 5)
    u, d = rng.uniform(-1, 1, (N, N, N)), rng.uniform(-1, 1, (N, N, N))
    NR.refresh(u, axes)
    a, b = MR.Hierarchy(c, L, 2, 3.5, e, axes, faces, mask), SF.Hierarchy(c, L, 2, 3.5, e, axes, faces, mask, None)
    assert np.array_equal(a.LU, b.LU)
    assert np.array_equal(_cycles(a, u, d), _cycles(b, u, d)) and _same(a, b)
    xa, na, _, _, _ = MR.wpcg(a, u, d, 0.0, 1e-300, 2)
    xb, nb, _, _, _ = SF.wpcg(b, u, d, 0.0, 1e-300, 2)
    assert np.array_equal(xa, xb) and np.array_equal(na, nb)
    A = SF.coarse_matrix(5, 0.25, None if e is None else e[::4, ::4, ::4], 3.5, axes, faces, mask[::4, ::4, ::4], None)
    assert np.array_equal(A, MR.coarse_matrix(5, 0.25, None if e is None else e[::4, ::4, ::4], 3.5, axes, faces, mask[::4, ::4, ::4]))
    # the stepper's d and full multigrid (no mask there)
    import _step_ref as SR
    dt, theta, kappa = 0.01, 0.5, 2.0
    sig = SR.sigma_of(dt, theta, kappa)
    a, b = NR.Problem(c, L, 2, sig, e, axes, faces), SF.Hierarchy(c, L, 2, sig, e, axes, faces, None, None)
    assert np.array_equal(SR.rhs(a, u, d, dt, theta, kappa), SF.step_rhs(b, u, d, dt, theta, kappa))
    for p in (a, b):
        p.u[-1][...] = u
        p.d[-1][...] = d
    assert FR.fmg_solve(a, 1) == SF.fmg_solve(b, 1) and np.array_equal(a.u[-1], b.u[-1])


@pytest.mark.parametrize("axes,faces", [(0, 0), (7, 0), (0, 63), (4, 3)])
@pytest.mark.parametrize("masked", [False, True])
def test_the_two_neutrality_statements(axes, faces, masked):
    """a zero field on an eps context is no field; a field without eps is eps = 1 everywhere with the same field: every grid
    value of two cycles, sign bits included, the norms and the factors"""
    c, L, N = 5, 3, 17
    rng = np.random.default_rng(3)
    mask = MR.gpu_test_mask(N) if masked else None
    u, d = rng.uniform(-1, 1, (N, N, N)), rng.uniform(-1, 1, (N, N, N))
    NR.refresh(u, axes)
    e = CR.exp_eps(N)
    for sigma in (0.0, 2.5):
        a = SF.Hierarchy(c, L, 2, sigma, e, axes, faces, mask, None)
        b = SF.Hierarchy(c, L, 2, sigma, e, axes, faces, mask, np.zeros((N, N, N)))
        assert np.array_equal(a.LU, b.LU)
        assert np.array_equal(_cycles(a, u, d), _cycles(b, u, d)) and _same(a, b)
        s = SF.random_field(N, a.h)
        a = SF.Hierarchy(c, L, 2, sigma, None, axes, faces, mask, s)
        b = SF.Hierarchy(c, L, 2, sigma, np.ones((N, N, N)), axes, faces, mask, s)
        assert np.array_equal(a.LU, b.LU)
        assert np.array_equal(_cycles(a, u, d), _cycles(b, u, d)) and _same(a, b)
        assert not np.array_equal(a.u[-1], SF.Hierarchy(c, L, 2, sigma, None, axes, faces, mask, None).u[-1])


def test_restriction_of_the_field():
    """full weighting at the coarse unknowns with the operator's taps, injection on Dirichlet faces, duplicates copied: a
    constant stays a constant at every unknown; a one-point-thick odd plane, gone under injection, keeps half its weight"""
    N = 17
    for axes, faces in BCS:
        lv = SF.restrict_field(np.full((N, N, N), 3.0), 3, axes, faces)
        assert [x.shape[0] for x in lv] == [5, 9, 17]
        for x in lv:
            assert np.array_equal(x, np.full(x.shape, 3.0))
    plane = np.zeros((N, N, N))
    plane[9] = 8.0
    lv = SF.restrict_field(plane, 3, 0, 0)
    assert np.array_equal(lv[1][4, 1:-1, 1:-1], np.full((7, 7), 2.0)) and np.array_equal(lv[1][5, 1:-1, 1:-1], np.full((7, 7), 2.0))
    assert not lv[1][[0, 1, 2, 3, 6, 7, 8]].any() and SF.inject_field(plane, 3, 0)[1].sum() == 0.0
    # periodic in k: the duplicate of the finest level is not the caller's but its source's; wrapped taps
    rng = np.random.default_rng(1)
    s = rng.uniform(0.0, 1.0, (N, N, N))
    lv = SF.restrict_field(s, 2, 4, 0)
    assert np.array_equal(lv[1][:, :, N - 1], s[:, :, 0]) and np.array_equal(lv[0][:, :, 8], lv[0][:, :, 0])
    want = sum(s[2 * 3 + a, 2 * 2 + b, (0 + cc) % (N - 1)] * (0.5 if a == 0 else 0.25) * (0.5 if b == 0 else 0.25) *
               (0.5 if cc == 0 else 0.25) for a in (-1, 0, 1) for b in (-1, 0, 1) for cc in (-1, 0, 1))
    assert abs(lv[0][3, 2, 0] - want) <= 1e-14 * want
    # a Dirichlet face point is injected
    assert lv[0][0, 2, 3] == s[0, 4, 6]


def test_pin_rule():
    N = 5
    zero = np.zeros((N, N, N))
    one = zero.copy()
    one[2, 2, 2] = 1e-300
    dup_only = zero.copy()
    dup_only[N - 1] = 1.0  # a duplicate plane of the all-periodic box: no unknown
    assert SF.pinned(7, 0, 0.0, None, None) and SF.pinned(7, 0, 0.0, None, zero) and SF.pinned(7, 0, 0.0, None, dup_only)
    assert not SF.pinned(7, 0, 0.0, None, one) and not SF.pinned(7, 0, 1.0, None, zero) and not SF.pinned(5, 0, 0.0, None, zero)
    assert SF.pinned(0, 63, 0.0, None, zero) and not SF.pinned(0, 63, 0.0, None, one)
    m = np.zeros((N, N, N), dtype=np.uint8)
    m[1, 1, 1] = 1
    assert not SF.pinned(0, 63, 0.0, m, zero)
    # full weighting carries a positive entry of the finest level to level 0: pin and projection go together
    top = np.zeros((9, 9, 9))
    top[3, 3, 3] = 1.0
    s0 = SF.restrict_field(top, 2, 0, 63)[0]
    assert not SF.pinned(0, 63, 0.0, None, s0) and not SF.singular(0, 63, 0.0, None, None, s0, top)
    assert SF.singular(0, 63, 0.0, None, None, zero, np.zeros((9, 9, 9)))


def _solve(c, L, sigma, s, u_star, f):
    """the discrete solution by restated PCG to rtol 1e-12 from the Dirichlet values; returns the max error against u*"""
    N = u_star.shape[0]
    prob = SF.Hierarchy(c, L, 2, sigma, None, 0, 0, None, s)
    x0 = u_star.copy()
    x0[1:-1, 1:-1, 1:-1] = 0.
    x, _, ok, _, _ = SF.wpcg(prob, x0, f, 1e-12, 0.0, 40)
    assert ok
    return float(np.abs(x - u_star).max())


def test_second_order_convergence_with_a_smooth_field():
    """Delta u - s(x) u = f, Dirichlet faces, u* = prod (sin(pi x_a) + 1 + x_a), s = 50 (1 + x y + 0.5 cos 2 pi z), solved to
    rounding at 17^3 and 33^3.  The error ratio is held to the ratio the same restatement gives with the scalar sigma =
    mean(s), less 10 %.  Why 10 %: the zeroth-order term has no truncation error, so both problems have the SAME truncation
    error tau_h = (h^2/12) sum d^4 u* / dx_a^4 + O(h^4) and differ only in the operator that maps it to the error; each
    ratio is 4 (1 + K h^2 + ...), with K h^2 the relative size of the h^4 term at h = 1/16.  For this u* (wave number pi)
    that term is (pi h)^2 / 30 * O(1) per operator, below 1 %; the two ratios can differ by the difference of two such
    terms, and 10 % is ten times that -- while a first-order defect (a field shifted by one point, a wrong h^2 scaling on a
    coarse level showing up as a stalled solve) halves the ratio."""
    res = {}
    for N, L in ((17, 3), (33, 4)):
        u_star, lap = FR.manufactured(N, 0, 0, 0.0)
        s = SF.smooth_field(N)
        sbar = float(s.mean())
        res[N] = (_solve(5, L, 0.0, s, u_star, lap - s * u_star), _solve(5, L, sbar, None, u_star, lap - sbar * u_star))
    ratio_field, ratio_scalar = res[17][0] / res[33][0], res[17][1] / res[33][1]
    print(f"errors {res}, ratio with the field {ratio_field:.3f}, with the scalar {ratio_scalar:.3f}")
    assert ratio_scalar > 3.5
    assert ratio_field >= 0.9 * ratio_scalar


@pytest.mark.parametrize("field", ["const", "eps"])
def test_the_restated_cycle_is_self_adjoint_with_a_field(field):
    """|<x, My>_w - <y, Mx>_w| <= 1e-10 |x| |My| at 17^3 with Neumann faces all round and a random field in [0, 1/h^2]; so is
    the operator: a non-negative diagonal changes neither symmetry"""
    c, L, N = 5, 3, 17
    e = CR.ball_eps(N, 100.) if field == "eps" else None
    prob = SF.Hierarchy(c, L, 2, 0.0, e, 0, 63, None, SF.random_field(N, 1.0 / (N - 1)))
    assert not prob.pinned() and not prob.is_singular()
    w, _ = WR.weights(prob)
    rng = np.random.default_rng(3)
    x, y = rng.uniform(-1, 1, w.shape), rng.uniform(-1, 1, w.shape)
    Mx, My = SF.cycle_blk(prob, x), SF.cycle_blk(prob, y)
    a, b = WR.wdot(w, x, My), WR.wdot(w, y, Mx)
    assert abs(a - b) <= 1e-10 * np.linalg.norm(x) * np.linalg.norm(My)
    Ax, Ay = prob.apply(x), prob.apply(y)
    a, b = WR.wdot(w, x, Ay), WR.wdot(w, y, Ax)
    assert abs(a - b) <= 1e-10 * np.linalg.norm(x) * np.linalg.norm(Ay)


DECLS = {
    "mg3d_ctx_set_shift_field": "int mg3d_ctx_set_shift_field(mg3d_ctx *ctx, const double *s);",
    "mg3d_ctx_set_shift_field_device": "int mg3d_ctx_set_shift_field_device(mg3d_ctx *ctx, const mg3d_array *s, void *stream);",
    "mg3d_ctx_has_shift_field": "int mg3d_ctx_has_shift_field(const mg3d_ctx *ctx, int *on);",
    "mg3d_ctx_get_shift_field": "int mg3d_ctx_get_shift_field(mg3d_ctx *ctx, int level, double *host);",
    "mg3d_coarse_matrix_field": "void mg3d_coarse_matrix_field(double *A, int N, double h, const double *eps, double sigma, "
                                "int periodic_axes, int neumann_faces, const unsigned char *mask, const double *s);",
}


def test_new_symbols_are_exported_with_the_declared_signatures():
    text = open(os.path.join(ROOT, "include", "mg3d.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"\s+", " ", text)
    text = re.sub(r"\s*([(),;*])\s*", r"\1", text)
    for sym, decl in DECLS.items():
        assert getattr(M.lib(), sym) is not None
        assert re.sub(r"\s*([(),;*])\s*", r"\1", decl) in text, sym
    for name in ("set_shift_field", "set_shift_field_tensor", "has_shift_field", "get_shift_field"):
        assert callable(getattr(M.Solver, name))
    lib = M.lib()
    assert lib.mg3d_ctx_set_shift_field.argtypes == [C.c_void_p, C.POINTER(C.c_double)]
    assert lib.mg3d_ctx_get_shift_field.argtypes == [C.c_void_p, C.c_int, C.POINTER(C.c_double)]
    assert len(lib.mg3d_coarse_matrix_field.argtypes) == 9 and lib.mg3d_coarse_matrix_field.restype is None


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present")
def test_entry_points_without_a_device():
    L = M.lib()
    on = C.c_int(7)
    buf = (C.c_double * 27)()
    assert L.mg3d_ctx_set_shift_field(None, buf) == 1  # MG3D_ERR_ARG: no context can exist without a device
    assert L.mg3d_ctx_set_shift_field_device(None, None, None) == 1
    assert L.mg3d_ctx_has_shift_field(None, C.byref(on)) == 1 and on.value == 7
    assert L.mg3d_ctx_get_shift_field(None, 0, buf) == 1
