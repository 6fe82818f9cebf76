"""Fixed points inside the domain (mg3d_ctx_set_mask) without a GPU: the numpy restatement tests/_mask_ref.py against
tests/_neumann_ref.py (all-zero mask: bit for bit), the library's coarse matrix (mg3d_coarse_matrix_mask) against the
restatement, the symmetry of the restated preconditioner, and two discrete-exact problems solved by restated PCG."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import _coef_ref as CR
import _mask_ref as MR
import _neumann_ref as NR
import _wpcg_ref as WR
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import P

UB = C.POINTER(C.c_ubyte)


def _lib_matrix(N, h, e, sigma, axes, faces, mask):
    A = np.zeros(N ** 6)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
    M.lib().mg3d_coarse_matrix_mask(P(A), N, h, None if e is None else P(np.ascontiguousarray(e).reshape(-1)), sigma, axes,
                                    faces, None if m is None else m.ctypes.data_as(UB))
    return A


def _lib_bc(N, h, e, sigma, axes, faces):
    A = np.zeros(N ** 6)
    M.lib().mg3d_coarse_matrix_bc(P(A), N, h, None if e is None else P(np.ascontiguousarray(e).reshape(-1)), sigma, axes, faces)
    return A


def _eps(N, seed=1):
    return np.random.default_rng(seed).uniform(0.5, 4.0, (N, N, N))


# (periodic axes, Neumann faces): Dirichlet, periodic, Neumann, mixed, and the closed boxes whose pin the mask may lift
BCS = [(0, 0), (5, 0), (0, 10), (4, 3), (7, 0), (0, 63), (2, 51)]


# (a periodic axis needs c - 1 >= 4: N = 3 runs the masks without one)
@pytest.mark.parametrize("N,axes,faces", [(N, a, f) for N in (3, 5, 9) for a, f in BCS if not (a and N - 1 < 4)])
@pytest.mark.parametrize("sigma", [0.0, 3.5])
@pytest.mark.parametrize("field", ["const", "eps"])
def test_coarse_matrix_mask_equals_numpy(N, axes, faces, sigma, field):
    e = _eps(N) if field == "eps" else None
    h = 0.125
    rng = np.random.default_rng(N + axes + faces)
    for density in (0.1, 0.5):
        mask = (rng.uniform(size=(N, N, N)) < density).astype(np.uint8) * rng.integers(1, 256, (N, N, N)).astype(np.uint8)
        got, want = _lib_matrix(N, h, e, sigma, axes, faces, mask), MR.coarse_matrix(N, h, e, sigma, axes, faces, mask)
        assert np.array_equal(got, want)
        # identity rows exactly at the Dirichlet points, the duplicates and the fixed unknowns; no pin with a fixed unknown
        A = got.reshape(N ** 3, N ** 3)
        ident = (A == np.eye(N ** 3)).all(axis=1).reshape(N, N, N)
        fx = MR.fixed(mask, axes, faces)
        unk = NR.unknown_mask(N, axes, faces) & ~fx
        if MR.pinned(axes, faces, sigma, mask):
            unk[0, 0, 0] = False
        assert np.array_equal(ident, ~unk)


@pytest.mark.parametrize("N", [5, 9])
@pytest.mark.parametrize("axes,faces", BCS)
@pytest.mark.parametrize("sigma", [0.0, 3.5])
@pytest.mark.parametrize("field", ["const", "eps"])
def test_null_and_zero_masks_give_the_bc_matrix(N, axes, faces, sigma, field):
    e = _eps(N) if field == "eps" else None
    want = _lib_bc(N, 0.25, e, sigma, axes, faces)
    assert np.array_equal(_lib_matrix(N, 0.25, e, sigma, axes, faces, None), want)
    assert np.array_equal(_lib_matrix(N, 0.25, e, sigma, axes, faces, np.zeros((N, N, N), dtype=np.uint8)), want)
    # bytes on Dirichlet faces and periodic duplicates alone are no fixed unknowns
    m = (~NR.unknown_mask(N, axes, faces)).astype(np.uint8)
    assert np.array_equal(_lib_matrix(N, 0.25, e, sigma, axes, faces, m), want)


@pytest.mark.parametrize("axes,faces", [(0, 0), (5, 0), (0, 10), (4, 3)])
@pytest.mark.parametrize("field", ["const", "eps"])
def test_zero_mask_reproduces_the_neumann_reference(axes, faces, field):
    c, L, N = 5, 3, 17
    rng = np.random.default_rng(7)
    e = _eps(N) if field == "eps" else None
    a = NR.Problem(c, L, 2, 3.5, e, axes, faces)
    b = MR.Hierarchy(c, L, 2, 3.5, e, axes, faces, np.zeros((N, N, N), dtype=np.uint8))
    assert np.array_equal(a.LU, b.LU)
    u, d = rng.uniform(-1, 1, (N, N, N)), rng.uniform(-1, 1, (N, N, N))
    NR.refresh(u, axes)
    for p in (a, b):
        p.u[-1][...] = u
        p.d[-1][...] = d
    na, nb = a.vcycles(2), b.vcycles(2)
    assert np.array_equal(na, nb)
    for l in range(L):
        assert np.array_equal(a.u[l], b.u[l]) and np.array_equal(a.d[l], b.d[l]) and np.array_equal(a.r[l], b.r[l])


def test_injection_and_stored_bytes():
    N = 17
    m = MR.gpu_test_mask(N)
    lv = MR.inject(MR.stored(m, 5), 3)
    assert [x.shape[0] for x in lv] == [5, 9, 17]
    assert np.array_equal(lv[1], lv[2][::2, ::2, ::2]) and np.array_equal(lv[0], lv[2][::4, ::4, ::4])
    assert np.array_equal(lv[2][N - 1], lv[2][0]) and np.array_equal(lv[2][:, :, N - 1], lv[2][:, :, 0])
    assert np.array_equal(lv[0][4], lv[0][0])
    # the one-point-thick odd plate is gone from every coarse level
    odd = MR.plate(N, 9)
    assert MR.inject(odd, 3)[1].sum() == 0 and MR.inject(MR.plate(N, 8), 3)[0].sum() > 0


def _odd_plate(N):
    return MR.plate(N, (N // 2) | 1, 2)


@pytest.mark.parametrize("axes,faces", [(0, 0), (4, 0), (0, 9), (4, 3)])
@pytest.mark.parametrize("body", ["random", "odd_plate"])
def test_the_restated_cycle_is_a_symmetric_preconditioner(axes, faces, body):
    """|<x, My> - <y, Mx>| <= 1e-10 |x| |My| for random x, y that are zero at the fixed points; the weighted inner product
    with a Neumann face"""
    c, L, N = 5, 3, 17
    mask = MR.random_mask(N, 0.1, 11) if body == "random" else _odd_plate(N)
    prob = MR.Hierarchy(c, L, 2, 0.0, CR.ball_eps(N, 100.), axes, faces, mask)
    blk = NR.block(N, axes, faces)
    free = ~prob.fixed()[blk]
    w, _ = WR.weights(prob)
    rng = np.random.default_rng(3)
    x, y = rng.uniform(-1, 1, w.shape) * free, rng.uniform(-1, 1, w.shape) * free
    Mx, My = MR.cycle_blk(prob, x), MR.cycle_blk(prob, y)
    assert not Mx[~free].any() and not My[~free].any()
    a, b = WR.wdot(w, x, My), WR.wdot(w, y, Mx)
    assert abs(a - b) <= 1e-10 * np.linalg.norm(x) * np.linalg.norm(My)


@pytest.mark.parametrize("which", ["a", "b"])
def test_discrete_exact_problems(which):
    """restated PCG to rtol 1e-12 reaches the exact discrete solution; plain cycles are recorded: they converge on (a),
    whose body survives on the coarse grids, and are not expected to on (b), whose plate is gone from both"""
    c, L, N = 5, 3, 17
    axes, faces, mask, u0, exact = MR.exact_problem(which)
    prob = MR.Hierarchy(c, L, 2, 0.0, None, axes, faces, mask)
    d = np.zeros((N, N, N))
    x, norms, ok, _, sing = MR.wpcg(prob, u0, d, 1e-12, 0.0, 60)
    assert ok and not sing
    err = np.abs(x - exact).max()
    print(f"problem ({which}): PCG iterations {len(norms) - 1}, max error {err:.3e}")
    assert err <= 1e-10
    assert np.array_equal(x[mask != 0], u0[mask != 0])
    prob.u[-1][...] = u0
    prob.d[-1][...] = d
    with np.errstate(all="ignore"):
        cyc = prob.vcycles(12)
    factor = (cyc[-1] / cyc[3]) ** (1.0 / 8) if cyc[3] > 0 and np.isfinite(cyc[-1]) else float("inf")
    print(f"problem ({which}): plain cycles, residual factor per cycle {factor:.3f}, norms {cyc[0]:.3e} -> {cyc[-1]:.3e}")
    if which == "a":
        assert factor < 0.5


def test_pin_rule():
    N = 5
    none = np.zeros((N, N, N), dtype=np.uint8)
    one = none.copy()
    one[2, 2, 2] = 1
    face_only = none.copy()
    face_only[N - 1] = 1  # a duplicate plane of the all-periodic box: no fixed unknown
    assert MR.pinned(7, 0, 0.0, none) and MR.pinned(7, 0, 0.0, face_only) and not MR.pinned(7, 0, 0.0, one)
    assert not MR.pinned(7, 0, 1.0, none) and not MR.pinned(5, 0, 0.0, none)
    assert MR.pinned(0, 63, 0.0, none) and not MR.pinned(0, 63, 0.0, one)
    # the coarse mask empty but the finest not: the pin stays, the projection goes
    top = np.zeros((9, 9, 9), dtype=np.uint8)
    top[3, 3, 3] = 1
    assert MR.pinned(0, 63, 0.0, MR.inject(top, 2)[0]) and not MR.singular(0, 63, 0.0, MR.inject(top, 2)[0], top)


@pytest.mark.parametrize("N", [3, 5, 9])
@pytest.mark.parametrize("sigma", [0.0, 3.5])
def test_the_plain_arguments_give_the_reference_matrix(N, sigma):
    """the long hop in one step: no eps, no periodic axis, no Neumann face and no mask (NULL and all-zero) is the
    reference's Dirichlet matrix (orc_coarse_matrix_shift), byte for byte; the same with eps = 1 everywhere"""
    import _oracle as O
    h = 0.125
    want = np.zeros(N ** 6)
    O.lib().orc_coarse_matrix_shift(O.P(want), N, h, sigma)
    for e in (None, np.ones((N, N, N))):
        for mask in (None, np.zeros((N, N, N), dtype=np.uint8)):
            assert _lib_matrix(N, h, e, sigma, 0, 0, mask).tobytes() == want.tobytes(), (e is not None, mask is not None)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present")
def test_entry_points_without_a_device():
    L = M.lib()
    on = C.c_int(7)
    buf = (C.c_ubyte * 27)()
    assert L.mg3d_ctx_set_mask(None, buf) == 1  # MG3D_ERR_ARG: no context can exist without a device
    assert L.mg3d_ctx_set_mask_device(None, None, None) == 1
    assert L.mg3d_ctx_has_mask(None, C.byref(on)) == 1 and on.value == 7
    assert L.mg3d_ctx_get_mask(None, 0, buf) == 1
    with pytest.raises(M.Mg3dError) as ei:
        M.Solver(5, 3, 2).set_mask(np.zeros(17 ** 3, dtype=np.uint8))
    assert ei.value.code == 2  # MG3D_ERR_NO_DEVICE, from the context


@pytest.mark.parametrize("axes,faces", BCS)
@pytest.mark.parametrize("field", ["const", "eps"])
def test_block_forms_equal_the_whole_array_forms(axes, faces, field):
    """colour_pass_blocks and residual_blocks (the forms the 513^3 GPU test is held to) against colour_pass and residual at
    21^3 with blocks of 5 planes -- a short last block -- and d poisoned at the fixed unknowns: u and r bit for bit, the
    norm that of exact_residual_norm"""
    N, h, sigma = 21, 0.05, 3.5
    e = _eps(N) if field == "eps" else None
    if e is not None:
        NR.refresh(e, axes)
    rng = np.random.default_rng(axes + 8 * faces)
    mask = MR.stored((rng.uniform(size=(N, N, N)) < 0.2).astype(np.uint8), axes)
    u, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    NR.refresh(u, axes)
    fx = MR.fixed(mask, axes, faces)
    assert fx.any()
    d[fx] = np.nan
    for colour in (1, 0):
        a, b = u.copy(), u.copy()
        MR.colour_pass(a, d, e, h, sigma, axes, faces, colour, mask)
        MR.colour_pass_blocks(b, d, e, h, sigma, axes, faces, colour, mask, planes=5)
        assert np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b)) and not np.array_equal(a, u)
        u = a
    ra = rng.standard_normal((N, N, N))
    rb = ra.copy()
    MR.residual(u, d, e, h, sigma, axes, faces, mask, ra)
    got = MR.residual_blocks(u, d, e, h, sigma, axes, faces, mask, rb, planes=5)
    assert np.array_equal(ra, rb) and np.array_equal(np.signbit(ra), np.signbit(rb)) and not rb[fx].any()
    exact = MR.exact_residual_norm(u, d, e, h, sigma, axes, faces, mask)
    assert abs(got - exact) <= 1e-14 * exact
