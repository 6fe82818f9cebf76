"""The KEEP kernels of the fixed-point mask and full multigrid past one k-block of THREADS and at every chunk length of the
cubic interpolation, against the numpy restatements tests/_mask_keep_ref.py and tests/_fmg_ref.py.

mask_keep_kernel, fmg_inject_kernel and the masked restriction run one thread per COARSE point, 64 lanes a block in k: their
second block exists from a coarse side of 65 on (fine 129^3), and holds an interior unknown from a coarse side above 65 on.
tests/test_gpu_mask_keep.py stops at fine 65^3 (coarse 33: one block).  Here: fine 129 (coarse 65: the only column of the
second block is the face), 145 (73), 161 (81), 193 (97) and 257 (129); 73 and 81 leave a tail of one row in j (blocks of 4
rows).  The mask is _mask_keep_ref.seam_mask: thin_mask (a random 10 % body: tens of thousands of lost points past coarse
column 64) with lost points of their own bytes planted around fine index 128 in k and in j.

k_fmg_interp picks the chunk of coarse planes a block marches through from the launch size (_chunk below restates it): 2
up to fine 129, 4 at 145 .. 177, 8 at 193 .. 241, 16 from 257.  tests/test_gpu_fmg.py compares the interpolation up to 129:
chunk 2 in every launch.  Here the three boundary modes, with and without fixed points, at 4, 8 and 16 -- the lead-in of a
chunk that starts inside the grid, several rotations of the window, the one-plane last chunk (coarse 129 = 8 * 16 + 1).

Every test asserts on the restatement alone that it reaches what it is for, before the GPU is asked.  Grid values and mask
bytes bit for bit; the norm to NORM_RTOL."""
import types

import numpy as np
import pytest
import torch  # noqa: F401  before the package, as bench.py does: the HIP runtime is torch's

import _coef_ref as CR
import _fmg_ref as FR
import _mask_keep_ref as MK
import _mask_ref as MR
import _neumann_ref as NR
import _shift_field_ref as SF
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U

from test_gpu_mask_keep import _assert_masks, _n, _random_problem, _same_bits, _solver, _upload

pytestmark = pytest.mark.gpu

NORM_RTOL = 1e-13  # the project's summation tolerance
SENTINEL = 12345.678
K_HIGH_NEUMANN = (0, 32 | 1)  # the high-k face (and the low-i face) Neumann: coarse column Nc-1 is an unknown
WORDS = [(0, 0), (7, 0), (4, 3), (2, 1 | 2 | 16), K_HIGH_NEUMANN]  # (periodic axes, Neumann faces)


def _shape(N, axes):
    """(c, L) of fine side N; a periodic axis needs an even c - 1"""
    c, L = {129: (5, 6), 145: (10, 5), 161: (11, 5) if axes else (6, 6), 193: (7, 6), 257: (9, 6)}[N]
    assert _n(c, L) == N and not (axes and (c - 1) % 2)
    return c, L


_MASKS = {}


def _seam_mask(N):
    if N not in _MASKS:
        _MASKS[N] = MK.seam_mask(N)
        _MASKS[N].setflags(write=False)
    return _MASKS[N]


def _assert_second_block(origin, N, what):
    """the restatement's lost points behind coarse column 63 on the level below a fine side N (see the module docstring)"""
    Nc = (N + 1) // 2
    inside, last = MK.second_block_counts(origin, Nc)
    print(f"{what}: lost points with 64 <= K <= Nc-2: {inside}, with K == Nc-1: {last}")
    assert last >= 1
    if N == 129:
        assert Nc == 65 and inside == 0  # column 64 is the face
    else:
        assert inside >= 1000


# --------------------------------------------------------------------------------------------------------- 1 hierarchy
_HIERARCHY = [(N, axes, faces) for N in (129, 145, 161, 193) for axes, faces in WORDS if not (axes and N == 145)]


@pytest.mark.parametrize("N,axes,faces", _HIERARCHY)
def test_hierarchy(N, axes, faces):
    """get_mask(level) on every level against the restatement, the rule set before the mask; at 161 also the rule set after
    the mask and KEEP -> INJECT giving the injected hierarchy again"""
    c, L = _shape(N, axes)
    mask = _seam_mask(N)
    top = MR.stored(mask, axes)
    want, origin = MK.keep(top, L, axes, origins=True)
    _assert_second_block(origin[L - 2], N, f"{N}^3 {(axes, faces)}")
    for F, byte in MK.seam_points(N):
        assert want[L - 2][tuple(x // 2 for x in F)] == byte
    with _solver(c, L, 2, 0.0, None, axes, faces, mask, factor=False) as s:
        _assert_masks(s, want, "rule before the mask")
    if N != 161:
        return
    inj = MR.inject(top, L)
    assert any(not np.array_equal(a, b) for a, b in zip(want, inj))
    with _solver(c, L, 2, 0.0, None, axes, faces, mask, rule=None, factor=False) as s:
        _assert_masks(s, inj, "default rule")
        s.set_mask_coarsening("keep")
        _assert_masks(s, want, "rule after the mask")
        s.set_mask_coarsening("inject")
        _assert_masks(s, inj, "KEEP -> INJECT")


# ------------------------------------------------------------------------------------------------- 2 masked full multigrid
_FMG = [(161, axes, faces, "const") for axes, faces in WORDS] + [(145, 0, 0, "const"), (161, 0, 0, "eps"), (161, 0, 0, "sfield")]


@pytest.mark.parametrize("N,axes,faces,field", _FMG)
def test_fmg(N, axes, faces, field):
    """mg3d_fmg_solve(1) with V(1,1) under KEEP: fmg_inject_kernel, the masked restriction, the coarse right-hand side from
    u's own values and the masked interpolation of every level, all with a second k-block of threads.  d holds NaN at every
    fixed unknown.  u of the finest level bit for bit; d the caller's bits, NaNs included; u at the Dirichlet and fixed
    points the caller's; u finite; the norm to NORM_RTOL"""
    c, L = _shape(N, axes)
    mask = _seam_mask(N)
    eps = CR.ball_eps(N) if field == "eps" else None
    sf = SF.random_field(N, 1.0 / (N - 1)) if field == "sfield" else None
    if sf is not None:
        ref = MK.FieldHierarchy(c, L, 1, 0.0, eps, axes, faces, mask, sf)
    else:
        ref = MK.Hierarchy(c, L, 1, 0.0, eps, axes, faces, mask)
    _random_problem(ref, np.random.default_rng(N + faces + 64 * axes), poison=True)
    u_in, d_in = ref.u[-1].copy(), ref.d[-1].copy()
    held = MR._keep(ref.mask[-1], axes, faces) | FR.dirichlet_mask(N, axes, faces)
    # what this test is for, on the restatement alone
    what = f"{N}^3 {(axes, faces)} {field}"
    _assert_second_block(ref.origin[L - 2], N, what)
    stands = ref.fixed(L - 2) & (ref.origin[L - 2] >= 0)  # coarse fixed unknowns that take u of a lost point
    poisoned = np.isnan(d_in)
    print(f"{what}: such unknowns past column 63: {int(stands[:, :, 64:].sum())}; NaN in d: {int(poisoned.sum())}, "
          f"past fine column 127: {int(poisoned[:, :, 128:].sum())}")
    assert stands[:, :, 64:].sum() >= 1000
    assert np.array_equal(poisoned, ref.fixed()) and poisoned[:, :, 128:].sum() >= 1000
    if (axes, faces) == K_HIGH_NEUMANN:
        assert stands[:, :, -1].any() and poisoned[:, :, -1].any()  # the last column is an unknown
    with _solver(c, L, 1, 0.0, eps, axes, faces, mask, sfield=sf) as s:
        _upload(s, ref)
        got = s.fmg_solve(1)
        u = s.download(MG3D_U, L - 1).reshape(N, N, N)
        d = s.download(MG3D_D, L - 1)
    want = MK.fmg_solve(ref, 1)
    assert np.isfinite(want) and np.isfinite(ref.u[-1]).all()
    print(f"{what}: norm {got!r} reference {want!r} relative difference {abs(got - want) / want:.3e}")
    assert np.isfinite(u).all()
    bad = np.argwhere(u != ref.u[-1])
    assert _same_bits(u, ref.u[-1]), (len(bad), bad[:5].tolist())
    assert _same_bits(d, d_in)
    assert _same_bits(u[held], u_in[held])
    assert abs(got - want) <= NORM_RTOL * want, (got, want)


# ---------------------------------------------------------------------------- 3 the interpolation at every chunk length
def _chunk(n):
    """the chunk length k_fmg_interp (csrc/mg3d_kernels.hip) takes for the interpolation into a fine side n: blocks of 64
    columns x 8 rows, and chunks of 16 coarse planes halved while the launch has fewer than 1024 blocks"""
    nc = (n + 1) // 2
    gx, gy = -(-n // 64), -(-n // 8)
    chunk = 16
    while chunk > 2 and gx * gy * -(-nc // chunk) < 1024:
        chunk //= 2
    return chunk


def _mode(axes, faces):
    """the boundary mode a launcher instantiates (bc_mode): 0 plain, 1 wrap, 2 reflect"""
    return 2 if faces else (1 if axes else 0)


# (fine side, periodic axes, Neumann faces); each runs without a mask and with one.  The periodic word at 257 is there for
# the wrap instantiations at chunk 16
_INTERP_WORDS = {145: [(0, 0), (0, 1 << 2), (0, 1 << 5)], 161: [(7, 0), (4, 1)], 193: [(0, 0), (7, 0), (0, 12)],
                 257: [(0, 0), (4, 1), (7, 0)]}
_INTERP = [(n, axes, faces, masked) for n, words in _INTERP_WORDS.items() for axes, faces in words for masked in (False, True)]
_BELOW_THE_TOP = (5, 7, 4, 1)  # (c, L, axes, faces): fmg_interpolate(L-2) into 129^3
# if the launcher's rule changes, these are where to look: the lists above were chosen for the rule restated in _chunk
assert {_chunk(n) for n in _INTERP_WORDS} | {_chunk(_n(_BELOW_THE_TOP[0], _BELOW_THE_TOP[1] - 1))} == {2, 4, 8, 16}
assert {(_chunk(n), _mode(axes, faces), masked) for n, axes, faces, masked in _INTERP} == \
    {(ch, mode, masked) for ch in (4, 8, 16) for mode in (0, 1, 2) for masked in (False, True)}
assert _chunk(257) == 16 and (129 - 1) % 16 == 0  # 257: the last chunk is the one coarse plane 128


def _interpolated(uc, uf, axes, faces, mask_f):
    """uf after mg3d_fmg_interpolate from uc; mask_f: the fine level's stored bytes or None"""
    if mask_f is None:
        FR.interpolate(uc, uf, axes, faces)
    else:
        MK.interpolate(types.SimpleNamespace(u={1: uf, 0: uc}, mask={1: mask_f}, axes=axes, faces=faces), 1)
    return uf


@pytest.mark.parametrize("n,axes,faces,masked", _INTERP)
def test_interpolation_bit_for_bit(n, axes, faces, masked):
    """fmg_interpolate(L-1) into a sentinel-filled top level from a random coarse u whose duplicates are NOT consistent
    (none may be read): every point of u; with a mask the fixed unknowns and their duplicates keep the sentinel; the
    coarse level unchanged"""
    c, L = _shape(n, axes)
    nc = (n + 1) // 2
    rng = np.random.default_rng(n + 1000 * axes + 8000 * faces)
    uc = rng.standard_normal((nc, nc, nc))
    mask = _seam_mask(n) if masked else None
    top = MR.stored(mask, axes) if masked else None
    want = _interpolated(uc, np.full((n, n, n), SENTINEL), axes, faces, top)
    untouched = ~NR.unknown_mask(n, axes, faces) & ~NR.is_dup(n, axes) | NR.is_dup(n, axes) & FR.dirichlet_mask(n, axes, faces)
    if masked:
        fixed = MR._keep(top, axes, faces)
        assert fixed[:, :, 128:].sum() >= 1000 and fixed[:, 128:, :].sum() >= 1000 and not (fixed & untouched).any()
        untouched = untouched | fixed
    assert np.array_equal(want == SENTINEL, untouched)
    with M.Solver(c, L, 2) as s:
        s.set_periodic(axes)
        s.set_neumann(faces)
        if masked:
            s.set_mask_coarsening("keep")
            s.set_mask(mask)
        s.get_details()
        s.upload(MG3D_U, L - 2, uc)
        s.upload(MG3D_U, L - 1, np.full((n, n, n), SENTINEL))
        s.fmg_interpolate(L - 1)
        got = s.download(MG3D_U, L - 1).reshape(n, n, n)
        assert _same_bits(s.download(MG3D_U, L - 2), uc)
    bad = np.argwhere(got != want)
    assert _same_bits(got, want), (len(bad), bad[:5].tolist())


def test_interpolation_below_the_top():
    """fmg_interpolate(L-2) in a 257^3 context with seam_mask under KEEP: into 129^3 with the KEEP-coarsened bytes of that
    level (fixed unknowns that injection lacks among them); the levels above and below unchanged"""
    c, L, axes, faces = _BELOW_THE_TOP
    N, n, nc = _n(c, L), _n(c, L - 1), _n(c, L - 2)
    assert (N, n, nc) == (257, 129, 65)
    mask = _seam_mask(N)
    top = MR.stored(mask, axes)
    masks, inj = MK.keep(top, L, axes), MR.inject(top, L)
    kept_only = MR.fixed(masks[L - 2], axes, faces) & (inj[L - 2] == 0)
    assert kept_only.sum() >= 1000 and kept_only[:, :, 64:].sum() >= 1000
    rng = np.random.default_rng(257)
    uc, above = rng.standard_normal((nc, nc, nc)), rng.standard_normal((N, N, N))
    want = _interpolated(uc, np.full((n, n, n), SENTINEL), axes, faces, masks[L - 2])
    assert (want[kept_only] == SENTINEL).all()
    with _solver(c, L, 2, 0.0, None, axes, faces, mask) as s:
        s.upload(MG3D_U, L - 1, above)
        s.upload(MG3D_U, L - 3, uc)
        s.upload(MG3D_U, L - 2, np.full((n, n, n), SENTINEL))
        s.fmg_interpolate(L - 2)
        got = s.download(MG3D_U, L - 2).reshape(n, n, n)
        assert _same_bits(s.download(MG3D_U, L - 1), above) and _same_bits(s.download(MG3D_U, L - 3), uc)
    bad = np.argwhere(got != want)
    assert _same_bits(got, want), (len(bad), bad[:5].tolist())
