"""The BC_REFLECT instantiations of csrc/mg3d_kernels.hip (Neumann faces, mg3d_ctx_set_neumann) at the launch shapes a
Neumann face creates, through every entry point, and the boundary setters as a state machine -- against the numpy
reference of tests/_neumann_ref.py (pinned to tests/_periodic_ref.py at faces = 0 by tests/test_neumann_host.py, r of
every level included):

- a Neumann face adds an unknown to its axis.  On the 2^k+1 ladder a PAIR of faces on one axis makes the count 2^k+1: one
  more 64-lane block in k with one live lane, one more 4-row block in j with one live row, one more chunk in i with one
  plane; a single face makes it 2^k (every block full), a low one starting at 0, a high one ending at N-1.  Each single
  face and each pair alone, so that a tail is tested while the other axes keep their Dirichlet range;
- coarse grids off the ladder (c = 6, 7, 10, 11, 13) with every single face, the pairs, 21, 42, 63 and masks mixed with
  periodic axes, through smooth, residual, smooth_residual, smooth_restrict, restrict, prolong and coarse_solve;
- V-cycles with mg3d_ctx_set_keep_residual(1): r of every level, Neumann face points included;
- 513^3 and 577^3: masks that stay exactly at MG3D_MAX_PARTIALS with chunk 16, masks that double the chunk, a last chunk
  of one plane (test_column_grid_reaches_the_neumann_shapes asserts each property from the header's cap);
- setter histories against a fresh context built in the final state: the coefficient before the masks, a nonzero mask
  replaced by another, an axis periodic -> Neumann -> periodic, eps given under a periodic mask that is then cleared.

Grid values bit for bit with sign bits; norms against the exactly rounded sum (EXACT_NORM_RTOL of
tests/test_gpu_stencil_shapes.py) and against the reference's own sum (norm_rtol of tests/test_gpu_parity.py).

Left out on purpose (time: the numpy block reference dominates): no more than the eight cases at 513^3 / 577^3, and
there one colour pass of each colour, the residual and two unreferenced V-cycles, not a V-cycle's parity; the single
operators run a sample of (c, mask, operator), not the product (test_sample_covers_every_pair states the condition)."""
import numpy as np
import pytest

import _coef_ref as CR
import _neumann_ref as R
import _oracle as O
import _screened_ref as S
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U

from test_gpu_parity import norm_rtol
from test_gpu_stencil_shapes import EXACT_NORM_RTOL, _max_partials, bc_extra, column_grid

gpu = pytest.mark.gpu
SINGLE = [1, 2, 4, 8, 16, 32]
PAIRS = [3, 12, 48]


def _same_bits(a, b):
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _n(c, L):
    return O.level_sizes(c, L)[-1]


def _solver(c, L, nu, sigma, eps, axes, faces, keep_r=False):
    import multigrid_parallel_amd as M
    s = M.Solver(c, L, nu)
    s.set_keep_residual(keep_r)
    s.set_shift(sigma)
    s.set_periodic(axes)
    s.set_neumann(faces)
    if eps is not None:
        s.set_coefficient(eps)
    s.get_details()
    assert (s.periodic, s.neumann) == (axes, faces)
    return s


def _random_start(N, axes, seed):
    rng = np.random.default_rng(seed)
    u, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    R.refresh(u, axes)
    R.refresh(d, axes)
    return u, d


def _problem(c, L, nu, sigma, eps, axes, faces, u, d):
    ref = R.Problem(c, L, nu, sigma, eps, axes, faces)
    ref.u[-1][...] = u
    ref.d[-1][...] = d
    return ref


def _assert_levels(s, ref, L, r=False, what=""):
    for l in range(L):
        assert _same_bits(s.download(MG3D_U, l), ref.flat("u", l)), f"{what}u level {l}"
    for l in range(L - 1):
        assert _same_bits(s.download(MG3D_D, l), ref.flat("d", l)), f"{what}d level {l}"
    if r:
        for l in range(L):
            assert _same_bits(s.download(MG3D_R, l), ref.flat("r", l)), f"{what}r level {l}"


def _assert_same_state(a, b, L, r=True):
    """two contexts: u of every level, d below the top, r of every level"""
    for l in range(L):
        assert _same_bits(a.download(MG3D_U, l), b.download(MG3D_U, l)), f"u level {l}"
        if l < L - 1:
            assert _same_bits(a.download(MG3D_D, l), b.download(MG3D_D, l)), f"d level {l}"
        if r:
            assert _same_bits(a.download(MG3D_R, l), b.download(MG3D_R, l)), f"r level {l}"


# ------------------------------------------------------------------------------------------------ launch geometry
def launch_shape(N, axes, faces):
    """what column_grid() launches for the residual and the eps colour pass of an N^3 level, and how full its last
    blocks are: lanes / rows / last = live lanes of the last 64-lane block in k, live rows of the last 4-row block in j,
    planes of the last chunk in i"""
    gx, gy, gz, chunk, planes = column_grid(N, axes, faces)
    nk, nj = N - 2 + bc_extra(axes, faces, 2), N - 2 + bc_extra(axes, faces, 1)
    return dict(gx=gx, gy=gy, gz=gz, chunk=chunk, planes=planes, lanes=nk - (gx - 1) * 64, rows=nj - (gy - 1) * 4,
                last=planes - (gz - 1) * chunk, partials=gx * gy * gz)


# the tail shapes on the ladder: (c, L) with N = 65, 65 and 129
_TAIL_SIZES = [(9, 4), (5, 5), (9, 5)]
_TAIL_MASKS = SINGLE + PAIRS
# past the cap: N -> (c, L); (N, axes, faces, field)
_BIG = {513: (9, 7), 577: (19, 6)}
_BIG_CASES = [(513, 0, 1, None), (513, 0, 3, None), (513, 0, 12, "exp"), (513, 0, 48, None), (513, 0, 21, None),
              (577, 0, 3, "exp"), (577, 0, 1, None), (577, 1, 12, None)]
# what each case past the cap was chosen for: keys of launch_shape, "cap" = MG3D_MAX_PARTIALS
_BIG_WHY = {
    (513, 0, 1): dict(chunk=16, partials="cap", last=16),  # 512 planes: exactly at the cap, every chunk full
    (513, 0, 21): dict(chunk=16, partials="cap", last=16, lanes=64, rows=4),  # 512 unknowns per axis, from 0
    (513, 0, 3): dict(chunk=32, gz=17, last=1),  # 513 planes: one more chunk would pass the cap -> doubled, one plane left
    (513, 0, 12): dict(chunk=32, gy=129, rows=1, last=31),  # one more row block passes the cap -> doubled; one live row
    (513, 0, 48): dict(chunk=32, gx=9, lanes=1, last=31),  # one more lane block passes the cap; one live lane
    (577, 0, 3): dict(chunk=32, gz=19, last=1),
    (577, 0, 1): dict(chunk=32, gz=18, last=32),
    (577, 1, 12): dict(chunk=32, gy=145, rows=1, last=32),  # a periodic i axis beside a Neumann pair in j
}


def test_column_grid_reaches_the_neumann_shapes():
    """every case of the tail and past-the-cap lists has the property it was chosen for, computed from column_grid()'s
    arithmetic and the header's MG3D_MAX_PARTIALS: a changed cap fails here instead of silently moving the cases"""
    cap = _max_partials()
    for c, L in _TAIL_SIZES:
        N = _n(c, L)
        assert N in (65, 129) and ((N - 1) & (N - 2)) == 0
        base = launch_shape(N, 0, 0)
        assert base["chunk"] == 16 and (base["lanes"], base["rows"], base["last"]) == (63, 3, 15)
        for faces in _TAIL_MASKS:
            sh = launch_shape(N, 0, faces)
            assert sh["chunk"] == 16
            for ax, blocks, live, full in ((0, "gz", "last", 16), (1, "gy", "rows", 4), (2, "gx", "lanes", 64)):
                bits = faces >> 2 * ax & 3
                lo, hi = R.lo_hi(N, 0, faces, ax)
                if bits == 3:  # a pair: 2^k + 1 unknowns, one more block with one live lane / row / plane
                    assert (sh[blocks], sh[live], lo, hi) == (base[blocks] + 1, 1, 0, N - 1), (N, faces, ax, sh)
                elif bits:  # one face: 2^k unknowns, every block full; a low face starts at 0, a high one ends at N-1
                    assert (sh[blocks], sh[live]) == (base[blocks], full), (N, faces, ax, sh)
                    assert (lo, hi) == ((0, N - 2) if bits == 1 else (1, N - 1))
                else:  # the other axes keep their Dirichlet range
                    assert (sh[blocks], sh[live], lo, hi) == (base[blocks], base[live], 1, N - 2), (N, faces, ax, sh)
    for N, (c, L) in _BIG.items():
        assert _n(c, L) == N
    assert launch_shape(513, 0, 0)["chunk"] == 16 and launch_shape(577, 0, 0)["chunk"] == 32
    assert sorted(_BIG_WHY) == sorted((N, axes, faces) for N, axes, faces, _ in _BIG_CASES)
    for key, why in _BIG_WHY.items():
        sh = launch_shape(*key)
        assert sh["partials"] <= cap and 0 < sh["last"] <= sh["chunk"], (key, sh)
        for k, v in why.items():
            assert sh[k] == (cap if v == "cap" else v), (key, k, sh)
    # mask 1 keeps 513^3 at chunk 16, masks 12 and 48 double it: one face flips the chunk choice
    assert [launch_shape(513, 0, f)["chunk"] for f in (1, 2, 42, 12, 48, 63)] == [16, 16, 16, 32, 32, 32]
    assert [launch_shape(513, 0, 63)[k] for k in ("gx", "gy", "gz", "last")] == [9, 129, 17, 1]


# ----------------------------------------------------------------------------------------------- single operators
# (field, sigma) as tests/test_gpu_stencil_shapes.py: eps with sigma 0 and 1e3, the constant operator with sigma 1e3
_OPS = [("ball", 0.0), ("exp", 1e3), (None, 1e3)]
_NEUMANN_MASKS = [(0, f) for f in SINGLE + PAIRS + [21, 42, 63]]
_MIXED_MASKS = [(1, 60), (6, 3), (2, 33), (5, 12), (4, 6)]  # (periodic axes, Neumann faces): c - 1 even only
_COARSE = (6, 7, 10, 11, 13)
# (c, L, axes, faces, field, sigma): a sample generated so that every (c, mask) pair runs with an operator and every
# (mask, operator) pair with a c (test_sample_covers_every_pair); the top two levels of L = 3 or 4
_SAMPLE = []
for _ci, _c in enumerate(_COARSE):
    for _mi, (_axes, _faces) in enumerate(_NEUMANN_MASKS):
        _SAMPLE.append((_c, 3 + (_ci + _mi) % 2, _axes, _faces) + _OPS[(_ci + _mi) % 3])
for _ci, _c in enumerate((7, 11, 13)):
    for _mi, (_axes, _faces) in enumerate(_MIXED_MASKS):
        _SAMPLE.append((_c, 3 + (_ci + _mi) % 2, _axes, _faces) + _OPS[(_ci + _mi) % 3])
# sigma = 0 with every axis closed: the pinned coarse matrix, with the constant operator
_SAMPLE += [(6, 4, 0, 63, None, 0.0), (10, 3, 0, 63, None, 0.0), (7, 4, 6, 3, None, 0.0), (13, 3, 6, 3, None, 0.0)]
# the tail shapes of the ladder at 65^3 (and 33^3 below it): each pair with both kinds of operator
_TAIL_SINGLE = [(9, 4, 0, f, field, sigma) for f in PAIRS for field, sigma in ((None, 1e3), ("exp", 0.0))]


def test_sample_covers_every_pair():
    pairs_c = {(c, axes, faces) for c, _, axes, faces, _, _ in _SAMPLE}
    pairs_op = {(axes, faces, field, sigma) for _, _, axes, faces, field, sigma in _SAMPLE}
    for c in _COARSE:
        for axes, faces in _NEUMANN_MASKS + (_MIXED_MASKS if c in (7, 11, 13) else []):
            assert (c, axes, faces) in pairs_c, (c, axes, faces)
    for axes, faces in _NEUMANN_MASKS + _MIXED_MASKS:
        for field, sigma in _OPS:
            assert (axes, faces, field, sigma) in pairs_op, (axes, faces, field, sigma)
    for axes, faces in ((0, 63), (6, 3)):
        assert (axes, faces, None, 0.0) in pairs_op and R.pinned(axes, faces, 0.0)
    assert len(_NEUMANN_MASKS) == 12 and len(set(_SAMPLE)) == len(_SAMPLE)
    assert all(R.valid(axes, faces) and (not axes or c % 2) for c, _, axes, faces, _, _ in _SAMPLE)


def _single_operators(c, L, axes, faces, field, sigma):
    """random u, d, r at the top two levels: smooth (post, iters) = (0,1), (1,2), (0,3); residual norm-only and stored;
    smooth_residual; restrict of the stored r; prolong of a random coarse e; smooth_restrict against pre_smooth +
    residual + restrict; coarse_solve.  What lies on a Dirichlet face keeps what was uploaded."""
    N = _n(c, L)
    eps = None if field is None else CR.FIELDS[field](N)
    ref = R.Problem(c, L, 1, sigma, eps, axes, faces)
    rng = np.random.default_rng(1000 * c + 10 * L + 64 * axes + faces)
    with _solver(c, L, 1, sigma, eps, axes, faces) as s:
        for l in (L - 1, L - 2):
            n, h, e = s.level_n(l), s.level_h(l), ref.e(l)
            fixed = (~R.unknown_mask(n, axes, faces) & ~R.is_dup(n, axes)).reshape(-1)
            u, d = rng.standard_normal((n, n, n)), rng.standard_normal((n, n, n))
            R.refresh(u, axes)
            u_in = u.reshape(-1).copy()
            s.upload(MG3D_U, l, u)
            s.upload(MG3D_D, l, d)
            for post, iters in ((0, 1), (1, 2), (0, 3)):
                s.smooth(l, post, iters)
                (R.post_smooth if post else R.pre_smooth)(u, d, e, h, sigma, axes, faces, iters)
                got = s.download(MG3D_U, l)
                assert _same_bits(got, u.reshape(-1)), f"smooth({post}, {iters}), level {l}"
                assert _same_bits(got[fixed], u_in[fixed]), f"smooth({post}, {iters}), level {l}: Dirichlet points"

            r = rng.standard_normal((n, n, n))
            r_in = r.reshape(-1).copy()
            s.upload(MG3D_R, l, r)
            exact = R.exact_residual_norm(u, d, e, n, h, sigma, axes, faces)
            print(f"level {l}: exact norm {exact!r}")
            got = s.residual(l, store=False)
            assert _same_bits(s.download(MG3D_R, l), r_in), "residual(store=False) wrote r"
            assert got == pytest.approx(exact, rel=EXACT_NORM_RTOL), (got, exact)
            got = s.residual(l, store=True)
            want = R.residual(u, d, e, h, sigma, axes, faces, r)
            stored = s.download(MG3D_R, l)
            assert _same_bits(stored, r.reshape(-1)), f"residual, level {l}"
            assert _same_bits(stored[fixed], r_in[fixed]), f"residual, level {l}: Dirichlet points"
            assert got == pytest.approx(exact, rel=EXACT_NORM_RTOL), (got, exact)
            assert got == pytest.approx(want, rel=norm_rtol(n)), (got, want)

            got = s.smooth_residual(l, 1, 2, store=True)
            R.post_smooth(u, d, e, h, sigma, axes, faces, 2)
            R.residual(u, d, e, h, sigma, axes, faces, r)
            exact = R.exact_residual_norm(u, d, e, n, h, sigma, axes, faces)
            dl = s.download(MG3D_U, l)
            assert _same_bits(dl, u.reshape(-1)), f"smooth_residual u, level {l}"
            assert _same_bits(dl[fixed], u_in[fixed]), f"smooth_residual, level {l}: Dirichlet points of u"
            stored = s.download(MG3D_R, l)
            assert _same_bits(stored, r.reshape(-1)), f"smooth_residual r, level {l}"
            assert _same_bits(stored[fixed], r_in[fixed]), f"smooth_residual, level {l}: Dirichlet points of r"
            assert got == pytest.approx(exact, rel=EXACT_NORM_RTOL), (got, exact)
            got = s.smooth_residual(l, 0, 1, store=False)
            R.pre_smooth(u, d, e, h, sigma, axes, faces, 1)
            exact = R.exact_residual_norm(u, d, e, n, h, sigma, axes, faces)
            assert _same_bits(s.download(MG3D_U, l), u.reshape(-1)), f"smooth_residual(store=False) u, level {l}"
            assert _same_bits(s.download(MG3D_R, l), stored), "smooth_residual(store=False) wrote r"
            assert got == pytest.approx(exact, rel=EXACT_NORM_RTOL), (got, exact)

            nc = s.level_n(l - 1)
            dc = rng.standard_normal((nc, nc, nc))
            s.upload(MG3D_D, l - 1, dc)
            s.restrict(l)
            R.restrict(r, dc, axes, faces)
            assert _same_bits(s.download(MG3D_D, l - 1), dc.reshape(-1)), f"restrict, level {l}"

            dc = rng.standard_normal((nc, nc, nc))
            s.upload(MG3D_D, l - 1, dc)
            s.smooth_restrict(l, 2)
            R.pre_smooth(u, d, e, h, sigma, axes, faces, 2)
            R.residual(u, d, e, h, sigma, axes, faces, r)
            R.restrict(r, dc, axes, faces)
            dl = s.download(MG3D_U, l)
            assert _same_bits(dl, u.reshape(-1)), f"smooth_restrict u, level {l}"
            assert _same_bits(dl[fixed], u_in[fixed]), f"smooth_restrict, level {l}: Dirichlet points of u"
            assert _same_bits(s.download(MG3D_D, l - 1), dc.reshape(-1)), f"smooth_restrict d, level {l - 1}"
            assert _same_bits(s.download(MG3D_D, l), d.reshape(-1)), f"d of level {l} was written"

            ec = rng.standard_normal((nc, nc, nc))
            R.refresh(ec, axes)
            s.upload(MG3D_U, l - 1, ec)
            s.prolong(l)
            R.prolong(ec, u, axes, faces)
            assert _same_bits(s.download(MG3D_U, l), u.reshape(-1)), f"prolong, level {l}"
        d0 = rng.standard_normal((c, c, c))
        s.upload(MG3D_D, 0, d0)
        s.coarse_solve()
        u0 = np.zeros((c, c, c))
        R.coarse_solve(ref.LU, d0, u0, axes, faces, sigma)
        assert _same_bits(s.download(MG3D_U, 0), u0.reshape(-1)), "coarse_solve"


@gpu
@pytest.mark.parametrize("c,L,axes,faces,field,sigma", _SAMPLE)
def test_single_operators(c, L, axes, faces, field, sigma):
    _single_operators(c, L, axes, faces, field, sigma)


@gpu
@pytest.mark.parametrize("c,L,axes,faces,field,sigma", _TAIL_SINGLE)
def test_single_operators_on_the_tail_shapes(c, L, axes, faces, field, sigma):
    """65^3 with a pair of faces on one axis: one live plane / row / lane in the last block (33^3 below it the same)"""
    _single_operators(c, L, axes, faces, field, sigma)


# ------------------------------------------------------------------------------------------------- V-cycle parity
# (c, L, faces, nu, field, sigma): every single face and every pair at each size, nu in {1, 2}, the constant operator and
# eps "exp" spread so that each mask meets both nu and both operators
_TAIL_VCYCLE = [(c, L, faces, 1 + (mi + si) % 2, (None, "exp")[(mi + (si + 1) // 2) % 2], (0.0, 10.0)[mi % 2])
                for si, (c, L) in enumerate(_TAIL_SIZES) for mi, faces in enumerate(_TAIL_MASKS)]


def _vcycle_parity(c, L, nu, sigma, field, axes, faces, keep_r):
    N = _n(c, L)
    eps = None if field is None else CR.FIELDS[field](N)
    u, d = _random_start(N, axes, c * 100 + L * 10 + faces + 64 * axes)
    ref = _problem(c, L, nu, sigma, eps, axes, faces, u, d)
    with _solver(c, L, nu, sigma, eps, axes, faces, keep_r) as s:
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        want = ref.vcycles(3)
        got = list(s.vcycles(1)) + list(s.vcycles(2))
        _assert_levels(s, ref, L, r=keep_r)
        exact = R.exact_residual_norm(s.download(MG3D_U, L - 1), s.download(MG3D_D, L - 1), ref.e(L - 1), N,
                                      s.level_h(L - 1), sigma, axes, faces)
        state = [s.download(MG3D_U, l) for l in range(L)] + [s.download(MG3D_D, l) for l in range(L - 1)]
    print(f"norms {got!r} reference {list(want)!r} exact {exact!r}")
    assert got[-1] == pytest.approx(exact, rel=EXACT_NORM_RTOL), (got[-1], exact)
    np.testing.assert_allclose(got, want, rtol=norm_rtol(N), atol=0)
    return got, state, ref


@gpu
@pytest.mark.parametrize("c,L,faces,nu,field,sigma", _TAIL_VCYCLE)
def test_vcycle_parity_on_the_tail_shapes(c, L, faces, nu, field, sigma):
    """u of every level and d below the top after vcycles(1) + vcycles(2) from a random start, bit for bit"""
    _vcycle_parity(c, L, nu, sigma, field, 0, faces, False)


@gpu
@pytest.mark.parametrize("c,L,axes,faces,field,sigma", [(9, 4, 0, 1, None, 0.0), (5, 4, 0, 40, "exp", 10.0),
                                                        (6, 4, 0, 63, None, 0.0), (5, 5, 6, 3, "smooth", 0.0)])
def test_keep_residual(c, L, axes, faces, field, sigma):
    """with mg3d_ctx_set_keep_residual(1): r of every level is the reference's, Neumann face points included (level 0
    has none: zero); u, d and the norms are those of the run without it"""
    plain, state, _ = _vcycle_parity(c, L, 2, sigma, field, axes, faces, False)
    kept, state_r, ref = _vcycle_parity(c, L, 2, sigma, field, axes, faces, True)
    assert plain == kept
    for a, b in zip(state, state_r):
        assert _same_bits(a, b)
    for l in range(1, L):  # (the comparison on the Neumann faces is not one of zeros)
        for f in range(6):
            if faces >> f & 1:
                sl = [slice(None)] * 3
                sl[f // 2] = -1 if f & 1 else 0
                assert ref.r[l][tuple(sl)].any(), (l, f)
    assert not ref.r[0].any()


# ---------------------------------------------------------------------------------- past the column partial cap
@gpu
@pytest.mark.parametrize("N,axes,faces,field", _BIG_CASES)
def test_past_the_partial_cap(N, axes, faces, field):
    """the finest level: one colour pass of each colour (smooth(top, 0, 1)) and residual(top, store=True) on random u, d
    bit for bit with the blockwise reference, the norm exact; then two V-cycles: the last norm is the exact norm of the
    downloaded u, and the norm falls"""
    c, L = _BIG[N]
    sigma = 10.0
    u, d = _random_start(N, axes, N + faces + 64 * axes)
    e = None
    if field is not None:
        e = CR.FIELDS[field](N)
        R.refresh(e, axes)
    with _solver(c, L, 1, sigma, e, axes, faces) as s:
        top, h = L - 1, s.level_h(L - 1)
        s.upload(MG3D_U, top, u)
        s.upload(MG3D_D, top, d)
        s.smooth(top, 0, 1)
        R.colour_pass_blocks(u, d, e, h, sigma, axes, faces, 1)
        R.colour_pass_blocks(u, d, e, h, sigma, axes, faces, 0)
        got = s.download(MG3D_U, top)
        assert _same_bits(got, u.reshape(-1)), "smooth"
        del got
        s.zero(MG3D_R, top)
        nrm = s.residual(top, store=True)
        r = np.zeros((N, N, N))
        want = R.residual_blocks(u, d, e, h, sigma, axes, faces, r)
        got = s.download(MG3D_R, top)
        assert _same_bits(got, r.reshape(-1)), "residual"
        del got, r, u
        print(f"residual norm {nrm!r} reference {want!r}")
        assert nrm == pytest.approx(want, rel=EXACT_NORM_RTOL), (nrm, want)
        norms = s.vcycles(2)
        u = s.download(MG3D_U, top).reshape(N, N, N)
    exact = R.residual_blocks(u, d, e, h, sigma, axes, faces)
    print(f"V-cycle norms {list(norms)!r} exact {exact!r}")
    assert norms[-1] == pytest.approx(exact, rel=EXACT_NORM_RTOL), (norms[-1], exact)
    assert norms[1] < norms[0] < nrm, (nrm, norms)


# ------------------------------------------------------------------ the setters as a state machine
def _chain(c, L, nu, sigma, eps, steps, u, d):
    """the numpy reference of a history: steps = [(axes, faces, cycles)], each a fresh R.Problem that starts from the u
    the one before left on the finest level (every other array a cycle reads it writes first, and r where it is not
    written is what a context that never had the earlier mask holds: zero).  Returns (the last Problem, its start u,
    every norm)"""
    norms, start = [], u
    for axes, faces, cycles in steps:
        start = u
        ref = _problem(c, L, nu, sigma, eps, axes, faces, u, d)
        norms += list(ref.vcycles(cycles))
        u = ref.u[-1]
    return ref, start, norms


def _set_masks(s, axes, faces):
    """the documented order: a Neumann bit on a periodic axis is refused by whichever setter comes second, so clear one
    before setting the other"""
    s.set_neumann(s.neumann & ~sum(3 << 2 * ax for ax in range(3) if axes >> ax & 1))
    s.set_periodic(s.periodic & axes)
    s.set_periodic(axes)
    s.set_neumann(faces)
    assert (s.periodic, s.neumann) == (axes, faces)


def _history(c, L, nu, sigma, field, steps, seed, keep_r=True, legs=False, first_dirichlet=False):
    """runs `steps` on one context (vcycles(1) + vcycles(cycles - 1) per step), then the last step alone on a fresh
    context built directly in the final state from the u the history had before its last step: both equal the numpy
    reference and each other in u of every level, d below the top, r of every level (keep_r) and the norms"""
    import multigrid_parallel_amd as M
    N = _n(c, L)
    eps = None if field is None else CR.FIELDS[field](N)
    if eps is not None:
        for axes, _, _ in steps:
            R.refresh(eps, axes)
    u, d = _random_start(N, 7, seed)
    want_first = []
    u_ref = u
    if first_dirichlet:  # one cycle of the fused Dirichlet schedules, which runs the next down-leg ahead
        dref = S.Problem(c, L, nu, sigma)
        dref.u[-1][...] = u
        dref.d[-1][...] = d
        want_first = [dref.vcycle()]
        u_ref = dref.u[-1]
    ref, start, want = _chain(c, L, nu, sigma, eps, steps, u_ref, d)
    want = want_first + want
    with M.Solver(c, L, nu) as s, M.Solver(c, L, nu) as f:
        got = []
        s.set_keep_residual(keep_r)
        s.set_shift(sigma)
        if legs:
            s.set_option("legs", 1)
            s.set_option("legs_min", 66)
        if eps is not None:
            s.set_coefficient(eps)
        s.get_details()
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        if first_dirichlet:
            got.append(s.vcycle())
        for axes, faces, cycles in steps:
            _set_masks(s, axes, faces)
            got += list(s.vcycles(1)) + list(s.vcycles(cycles - 1))
        _assert_levels(s, ref, L, r=keep_r, what="history: ")
        axes, faces, cycles = steps[-1]
        f.set_keep_residual(keep_r)
        f.set_shift(sigma)
        f.set_periodic(axes)
        f.set_neumann(faces)
        if eps is not None:
            f.set_coefficient(eps)
        f.get_details()
        f.upload(MG3D_U, L - 1, start)
        f.upload(MG3D_D, L - 1, d)
        fresh = list(f.vcycles(1)) + list(f.vcycles(cycles - 1))
        _assert_levels(f, ref, L, r=keep_r, what="fresh: ")
        _assert_same_state(s, f, L, r=keep_r)
    print(f"norms {got!r} reference {want!r}")
    assert got[-cycles:] == fresh
    np.testing.assert_allclose(got, want, rtol=norm_rtol(N), atol=0)


@gpu
@pytest.mark.parametrize("c,L,a,b,field,sigma", [(5, 4, 1, 2, None, 0.0), (6, 4, 63, 12, None, 0.0),
                                                 (5, 4, 12, 63, "exp", 5.0), (7, 3, 21, 42, "smooth", 0.0)])
def test_a_nonzero_mask_replaced_by_another(c, L, a, b, field, sigma):
    """faces a -> faces b with cycles before and after.  On the faces that turn Dirichlet again r is zeroed
    (boundary_changed): seen in r itself and, through the injection of those faces, in d of the coarser levels"""
    _history(c, L, 2, sigma, field, [(0, a, 2), (0, b, 3)], seed=a + 64 * b)


@gpu
def test_masks_replaced_behind_a_cycle_that_ran_ahead():
    """legs at 129^3: vcycle (runs the next down-leg ahead), faces 1, cycles, faces 2, cycles -- the reference of one
    Dirichlet cycle followed by the two Neumann runs.  (keep_residual off: with it no cycle runs ahead)"""
    _history(9, 5, 2, 0.0, None, [(0, 1, 2), (0, 2, 2)], seed=129, keep_r=False, legs=True, first_dirichlet=True)


@gpu
@pytest.mark.parametrize("field,sigma", [(None, 0.0), ("smooth", 3.0)])
def test_an_axis_from_periodic_to_neumann_and_back(field, sigma):
    """(axes 1, faces 0) -> (0, 3) -> (1, 0), each change through the documented order"""
    _history(9, 4, 2, sigma, field, [(1, 0, 2), (0, 3, 2), (1, 0, 2)], seed=31)


@gpu
@pytest.mark.parametrize("axes,faces,field", [(0, 63, "exp"), (6, 3, "smooth"), (1, 60, "exp"), (0, 9, "ball")])
def test_coefficient_before_the_masks(axes, faces, field):
    """set_coefficient and get_details first, then shift / periodic / neumann: the context of the usual order (eps
    already satisfies the duplicates, so both orders define the same operator), the coarse factor rebuilt"""
    import multigrid_parallel_amd as M
    c, L, nu, sigma = 5, 4, 2, 4.0
    N = _n(c, L)
    eps = CR.FIELDS[field](N)
    R.refresh(eps, axes)
    u, d = _random_start(N, axes, 7 + faces)
    ref = _problem(c, L, nu, sigma, eps, axes, faces, u, d)
    want = ref.vcycles(3)
    with M.Solver(c, L, nu) as s, _solver(c, L, nu, sigma, eps, axes, faces, True) as f:
        s.set_coefficient(eps)
        s.get_details()
        s.set_keep_residual(True)
        s.set_shift(sigma)
        s.set_periodic(axes)
        s.set_neumann(faces)
        for l in range(L):
            assert _same_bits(s.coefficient(l), f.coefficient(l)) and _same_bits(s.coefficient(l), ref.e(l))
        norms = []
        for x in (s, f):
            x.upload(MG3D_U, L - 1, u)
            x.upload(MG3D_D, L - 1, d)
            norms.append(list(x.vcycles(1)) + list(x.vcycles(2)))
            _assert_levels(x, ref, L, r=True)
        _assert_same_state(s, f, L)
    assert norms[0] == norms[1]
    np.testing.assert_allclose(norms[0], want, rtol=norm_rtol(N), atol=0)


@gpu
@pytest.mark.parametrize("after", [0, 2, 3])
def test_eps_given_under_a_periodic_mask_that_is_cleared(after):
    """eps uploaded under axes = 1 with caller values at the duplicates (i = N-1) that differ from their sources, then
    set_periodic(0) (and Neumann faces `after` on that axis): the operator is that of eps with the sources copied over
    the duplicates -- get_coefficient shows it on every level, and the cycles are the reference's with that array"""
    import multigrid_parallel_amd as M
    c, L, nu, sigma = 5, 4, 2, 2.0
    N = _n(c, L)
    given = CR.FIELDS["exp"](N)
    assert not np.array_equal(given[N - 1], given[0])
    eps = given.copy()
    R.refresh(eps, 1)
    u, d = _random_start(N, 1, 77)
    first = _problem(c, L, nu, sigma, eps, 1, 0, u, d)
    want = list(first.vcycles(1))
    ref = _problem(c, L, nu, sigma, eps, 0, after, first.u[-1], d)
    want += list(ref.vcycles(2))
    with M.Solver(c, L, nu) as s, _solver(c, L, nu, sigma, eps, 0, after, True) as f:
        s.set_keep_residual(True)
        s.set_shift(sigma)
        s.set_periodic(1)
        s.set_coefficient(given)
        s.get_details()
        assert _same_bits(s.coefficient(), eps)
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        got = list(s.vcycles(1))
        start = s.download(MG3D_U, L - 1)
        assert _same_bits(start, first.flat("u", L - 1))
        s.set_periodic(0)
        s.set_neumann(after)
        for l in range(L):
            assert _same_bits(s.coefficient(l), ref.e(l)), f"eps level {l}"
        got += list(s.vcycles(2))
        _assert_levels(s, ref, L, r=True, what="history: ")
        f.upload(MG3D_U, L - 1, start)
        f.upload(MG3D_D, L - 1, d)
        fresh = list(f.vcycles(2))
        _assert_levels(f, ref, L, r=True, what="fresh: ")
        _assert_same_state(s, f, L)
    assert got[1:] == fresh
    np.testing.assert_allclose(got, want, rtol=norm_rtol(N), atol=0)
