"""The MASK = true instantiations of csrc/mg3d_kernels.hip (fixed points inside the domain, mg3d_ctx_set_mask) at the launch
shapes tests/test_gpu_mask.py never reaches, against the numpy restatement tests/_mask_ref.py:

- a second 64-lane block in k, a partial last 4-row block in j and a short last chunk in i, for the column kernels
  (coef_color, residual, pcg_apply) and, from 65 k-pairs on, for the constant colour pass, whose lanes own k-pairs;
- every single Neumann face, the pairs, 21, 42, 63 and words mixed with periodic axes, with fixed unknowns placed on the
  Neumann faces, their edges and corners;
- the apply pass and mask_count_kernel through mg3d_pcg_solve / mg3d_wpcg_solve where one block, row or plane has ONE live
  member;
- cycles off the 2^k+1 ladder and at the sizes where a context without a mask runs ahead (carried cycles, one launch per
  leg), and set_mask on a context that has run ahead;
- the byte kernels (mask_pack, coef_inject<u8>, per_refresh<u8>) at two k-blocks from strided device arrays;
- one case past the cap of partial sums (513^3, chunk 32, a last chunk of one plane that is a Neumann face).

edge_mask(N, axes, faces) aims fixed unknowns at every one of those tails; the unmarked tests assert from column_grid()'s
arithmetic that each case has the shape its comment claims (test_the_cases_reach_the_shapes), that each targeted byte is
a fixed unknown (test_edge_mask_hits_fixed_unknowns) and that the restatement gives other bits when the bytes of one tail
alone are cleared (test_the_reference_sees_every_tail): a kernel that ignored the mask there would be caught.

Grid values bit for bit with sign bits; norms against the exactly rounded sum at norm_rtol(N) of tests/test_gpu_parity.py.
The solver iterates are held to 100 x the summation spread of the case, never below the figure tests/test_gpu_pcg.py /
test_gpu_wpcg.py hold the same call to.  The spreads of the four solver cases (python tests/test_gpu_mask_shapes.py:
spread_table(), two restatement runs, exactly rounded dots against numpy's pairwise sums):
                     u, k = 1    k = 2       norms
    65_f63           8.23e-16    6.88e-16    3.55e-15
    73_eps           3.70e-16    2.20e-16    7.63e-16
    81_per7          3.30e-16    2.99e-16    1.07e-15
    81_per4_f3_eps   3.87e-16    3.63e-16    1.71e-15
all below the existing files' figures (7.58e-15 / 8.18e-14 / 1.8e-14 for mg3d_pcg_solve, 1.04e-13 / 4.1e-12 / 9.6e-13 for
mg3d_wpcg_solve), which therefore govern."""
import itertools

import numpy as np
import pytest
import torch  # before the package, as bench.py does: the HIP runtime is torch's

import _coef_ref as CR
import _mask_ref as MR
import _neumann_ref as NR
import _oracle as O
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U

from test_gpu_neumann_shapes import PAIRS, SINGLE, _MIXED_MASKS, launch_shape
from test_gpu_parity import norm_rtol
from test_gpu_stencil_shapes import _max_partials

gpu = pytest.mark.gpu


def _same_bits(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _n(c, L):
    return O.level_sizes(c, L)[-1]


def _eps(field, N, axes):
    if field is None:
        return None
    e = CR.FIELDS["exp"](N)
    NR.refresh(e, axes)
    return e


# --------------------------------------------------------------------------------- 0 a mask that aims at the tails
def _tails(N, axes, faces):
    """the first index of the last 64-lane block in k, of the last 4-row block in j, of the last chunk in i"""
    sh = launch_shape(N, axes, faces)
    lo = [NR.lo_hi(N, axes, faces, ax)[0] for ax in range(3)]
    return lo[2] + 64 * (sh["gx"] - 1), lo[1] + 4 * (sh["gy"] - 1), lo[0] + sh["chunk"] * (sh["gz"] - 1)


def edge_targets(N, axes, faces):
    """the points edge_mask fixes on purpose, (n, 3): per axis the ends lo, lo+1, hi-1, hi of the unknowns, the k-block seams
    lo+62 .. lo+65, the chunk seams lo+15, +16, +17, +31, +32, +33; in k the pair seams 126 .. 130 of the constant pass, in i
    the first plane of the last chunk, in j the last row block; (seams of i) x (ends of j) x (seams of k) and (ends of i) x
    (seams of j) x (ends of k); on every Neumann face a point inside the face, one on each edge of its block of unknowns
    and its corners"""
    k_tail, j_tail, i_tail = _tails(N, axes, faces)
    lohi = [NR.lo_hi(N, axes, faces, ax) for ax in range(3)]
    ends, seams = [], []
    for ax, (lo, hi) in enumerate(lohi):
        e = [lo, lo + 1, hi - 1, hi]
        t = set(e) | {lo + o for o in (62, 63, 64, 65, 15, 16, 17, 31, 32, 33)}
        if ax == 2:
            t |= {126, 127, 128, 129, 130, k_tail}
        if ax == 0:
            t.add(i_tail)
        if ax == 1:
            t |= set(range(j_tail, hi + 1))
        ends.append(e)
        seams.append(sorted(x for x in t if lo <= x <= hi))
    pts = set(itertools.product(seams[0], ends[1], seams[2])) | set(itertools.product(ends[0], seams[1], ends[2]))
    for f in range(6):
        if not faces >> f & 1:
            continue
        ax, end = f // 2, (N - 1 if f & 1 else 0)
        b, c = [x for x in range(3) if x != ax]
        mid = {x: (lohi[x][0] + lohi[x][1]) // 2 + x for x in (b, c)}
        for vb, vc in ((mid[b], mid[c]), (mid[b] + 1, mid[c]), (lohi[b][0], mid[c]), (lohi[b][1], mid[c] + 1),
                       (mid[b], lohi[c][0]), (mid[b] + 1, lohi[c][1]), (lohi[b][1], lohi[c][1]), (lohi[b][0], lohi[c][0])):
            p = [0, 0, 0]
            p[ax], p[b], p[c] = end, vb, vc
            pts.add(tuple(p))
    return np.array(sorted(pts))


def edge_mask(N, axes, faces, seed=3):
    """random bytes at 10 % density (as _mask_ref.gpu_test_mask), bytes that must be ignored -- on every Dirichlet face, and
    on the periodic duplicates where their sources have none -- and 1 at edge_targets"""
    m = MR.random_mask(N, 0.1, seed)
    for ax in range(3):
        for hi_, end in ((0, 0), (1, N - 1)):
            s = [slice(None)] * 3
            s[ax] = end
            if NR.per(axes, ax):
                if hi_:
                    t = list(s)
                    t[ax] = 0
                    m[tuple(s)] = 0
                    m[tuple(s)][::2, ::3] = 1 - m[tuple(t)][::2, ::3]
            elif not NR.neu(faces, ax, hi_):
                m[tuple(s)][::2, ::3] = 1
    t = edge_targets(N, axes, faces)
    m[t[:, 0], t[:, 1], t[:, 2]] = 1
    return m


def regions(N, axes, faces, pairs=False):
    """the five tails as (N, N, N) bool: the last k-block (pairs: also within the second 64-pair block of the constant
    pass, k >= 128), the last row block, the last chunk, the Neumann faces, the first unknown of each axis"""
    k_tail, j_tail, i_tail = _tails(N, axes, faces)
    if pairs:
        k_tail = max(k_tail, 128)
    i, j, k = np.ogrid[:N, :N, :N]
    one = np.ones((N, N, N), dtype=bool)
    lo = [NR.lo_hi(N, axes, faces, ax)[0] for ax in range(3)]
    out = {"last k-block": one & (k >= k_tail), "last row block": one & (j >= j_tail), "last chunk": one & (i >= i_tail),
           "first unknowns": one & ((i == lo[0]) | (j == lo[1]) | (k == lo[2]))}
    if faces:
        on = ~one
        for f, x in enumerate((i, i, j, j, k, k)):
            if faces >> f & 1:
                on = on | (x == (N - 1 if f & 1 else 0))
        out["Neumann faces"] = on
    return out


# ------------------------------------------------------------------------------------------------------- the cases
# single operators: (c, L, axes, faces, field, sigma).  69^3 = (18, 3): every single face, the pairs, 21, 42, 63; 73^3 =
# (19, 3): the words mixed with periodic axes.  Each word with the constant operator and with eps, and at sigma 0 and 3.5
_WORDS = [(18, 0, f) for f in SINGLE + PAIRS + [21, 42, 63]] + [(19, a, f) for a, f in _MIXED_MASKS]
_SAMPLE = []
for _wi, (_c, _axes, _faces) in enumerate(_WORDS):
    _SAMPLE.append((_c, 3, _axes, _faces, None, (0.0, 3.5)[_wi % 2]))
    _SAMPLE.append((_c, 3, _axes, _faces, "exp", (3.5, 0.0)[_wi % 2]))
# the constant colour pass past one 64-pair block: (c, L, axes, faces, sigma, k-pairs, live lanes of the second block)
_PAIR_CASES = [(9, 5, 0, 32, 0.0, 65, 1), (9, 5, 0, 48, 3.5, 65, 1), (9, 5, 0, 63, 0.0, 65, 1),
               (10, 5, 0, 0, 3.5, 73, 8), (10, 5, 0, 0b011001, 0.0, 73, 8)]
# the solvers: name -> (c, L, sigma, field, axes, faces) and what launch_shape gives: unknowns per axis (k, j, i), live
# lanes of the last k-block, live rows of the last row block, planes of the last chunk
_SOLVER_CASES = {
    "65_f63": (9, 4, 0.0, None, 0, 63),  # the second k-block, the last row block, the last chunk: ONE live member each
    "73_eps": (10, 4, 0.0, "exp", 0, 0),  # off the ladder, the COEF apply
    "81_per7": (11, 4, 3.5, None, 7, 0),  # lo = 0 on every axis, wrap + mask
    "81_per4_f3_eps": (11, 4, 0.0, "exp", 4, 3),  # wrap + reflect + mask
}
_SOLVER_SHAPES = {"65_f63": ((65, 65, 65), 1, 1, 1), "73_eps": ((71, 71, 71), 7, 3, 7),
                  "81_per7": ((80, 80, 80), 16, 4, 16), "81_per4_f3_eps": ((80, 79, 81), 16, 3, 1)}
# cycles: name -> (c, L, nu, sigma, field, axes, faces, keep_r)
_CYCLE_CASES = {
    "145": (10, 5, 2, 0.0, None, 0, 0, False),  # where a context without a mask carries its cycles
    "161": (11, 5, 2, 0.0, None, 0, 0, False),  # where it runs one launch per leg
    "161_per4_f3_eps": (11, 5, 2, 3.5, "exp", 4, 3, True),
    "97_f63_odd": (13, 4, 2, 0.0, None, 0, 63, True),  # fixed unknowns on the finest level only: the pin stays
    "97_per5_eps": (7, 5, 2, 0.0, "exp", 5, 0, True),
}
_BYTES = (19, 3, 5)  # 73^3, periodic i and k
_BIG = (9, 7, 0, 3, 10.0)  # 513^3, both i faces Neumann, eps "exp"


def _all_words():
    """(N, axes, faces, pairs) of every case of every list"""
    out = [(_n(c, L), a, f, False) for c, L, a, f, _, _ in _SAMPLE]
    out += [(_n(c, L), a, f, True) for c, L, a, f, _, _, _ in _PAIR_CASES]
    out += [(_n(c, L), a, f, False) for c, L, _, _, a, f in _SOLVER_CASES.values()]
    out += [(_n(c, L), a, f, False) for c, L, _, _, _, a, f, _ in _CYCLE_CASES.values()]
    out += [(_n(_BYTES[0], _BYTES[1]), _BYTES[2], 0, False), (_n(_BIG[0], _BIG[1]), _BIG[2], _BIG[3], False)]
    return sorted(set(out))


def _odd_only(mask):
    """the mask without the points every index of which is even: nothing of it survives an injection"""
    m = mask.copy()
    m[::2, ::2, ::2] = 0
    return m


# ------------------------------------------------------------------------------------- 1 geometry, without a GPU
@pytest.mark.parametrize("N,axes,faces,pairs", [w for w in _all_words() if w[0] < 200])
def test_edge_mask_hits_fixed_unknowns(N, axes, faces, pairs):
    """every targeted point is a fixed unknown of the stored mask; at least half of the unknowns stay free; bytes lie
    where they must be ignored (513^3 is asserted by its GPU test: the arrays are large)"""
    _check_edge_mask(N, axes, faces, edge_mask(N, axes, faces))


def _check_edge_mask(N, axes, faces, mask):
    t = edge_targets(N, axes, faces)
    m = MR.stored(mask, axes)
    fx = MR.fixed(m, axes, faces)
    assert fx[t[:, 0], t[:, 1], t[:, 2]].all()
    unk = NR.unknown_mask(N, axes, faces)
    assert 2 * fx.sum() <= unk.sum()
    ignored = (mask != 0) & ~unk
    for ax in range(3):
        for hi_, end in ((0, 0), (1, N - 1)):
            s = [slice(None)] * 3
            s[ax] = end
            if NR.per(axes, ax):
                assert not hi_ or not np.array_equal(mask[tuple(s)], m[tuple(s)]), "a duplicate's own bytes"
            elif not NR.neu(faces, ax, hi_):
                assert ignored[tuple(s)].any(), "bytes on a Dirichlet face"
            else:  # the face, an edge of its block of unknowns and a corner
                lohi = [NR.lo_hi(N, axes, faces, x) for x in range(3) if x != ax]
                face = fx[tuple(s)]
                assert face[lohi[0][0] + 1:lohi[0][1], lohi[1][0] + 1:lohi[1][1]].any()
                assert face[lohi[0][0], lohi[1][0] + 1:lohi[1][1]].any() and face[lohi[0][1], lohi[1][1]]
    for name, reg in regions(N, axes, faces).items():
        assert (fx & reg).any(), name


def test_the_cases_reach_the_shapes():
    """launch_shape() -- column_grid() of the library restated from the header's MG3D_MAX_PARTIALS -- gives every case the
    property its comment claims: a changed cap or grid fails here instead of moving the cases silently"""
    assert _max_partials() == 32768
    for c, L, axes, faces, _, _ in _SAMPLE:
        N = _n(c, L)
        assert N == (73 if axes else 69) and (not axes or (c - 1) % 2 == 0)
        sh = launch_shape(N, axes, faces)
        unknowns = [NR.lo_hi(N, axes, faces, ax)[1] + 1 - NR.lo_hi(N, axes, faces, ax)[0] for ax in range(3)]
        # two k-blocks, a second one of 3 .. 9 lanes; 17 to 19 row blocks; five chunks of 16, the last of 3 .. 9 planes
        assert sh["gx"] == 2 and sh["chunk"] == 16 and sh["gz"] == 5 and sh["gy"] == -(-unknowns[1] // 4)
        assert (sh["lanes"], sh["rows"], sh["last"]) == (unknowns[2] - 64, (unknowns[1] - 1) % 4 + 1, unknowns[0] - 64)
        assert 3 <= sh["lanes"] <= 9 and 3 <= sh["last"] <= 9
    assert {launch_shape(69, 0, f)["rows"] for f in SINGLE + PAIRS} == {3, 4, 1}  # 67, 68 and 69 rows
    for c, L, axes, faces, _, pairs, live in _PAIR_CASES:
        N = _n(c, L)
        assert N in (129, 145)
        # smooth_color_kernel's grid: a lane owns the pair (2m, 2m+1), blocks of 64 pairs
        lo, hi = NR.lo_hi(N, axes, faces, 2)
        members = [[k for k in (2 * m, 2 * m + 1) if lo <= k <= hi] for m in range((N + 1) // 2)]
        assert (N + 1) // 2 == pairs >= 65 and sum(1 for m in members[64:] if m) == live
        if N == 129:
            assert members[64] == [128]  # one live lane, one live member
        sh = launch_shape(N, axes, faces)
        assert sh["gx"] >= 2 and sh["chunk"] == 16
    for name, (c, L, _, _, axes, faces) in _SOLVER_CASES.items():
        N = _n(c, L)
        sh = launch_shape(N, axes, faces)
        unknowns = tuple(NR.lo_hi(N, axes, faces, ax)[1] + 1 - NR.lo_hi(N, axes, faces, ax)[0] for ax in (2, 1, 0))
        assert (unknowns, sh["lanes"], sh["rows"], sh["last"]) == _SOLVER_SHAPES[name], (name, unknowns, sh)
        assert sh["gx"] == 2 and sh["chunk"] == 16
    assert [_n(c, L) for c, L, *_ in _SOLVER_CASES.values()] == [65, 73, 81, 81]
    for name, (c, L, _, _, _, axes, faces, _) in _CYCLE_CASES.items():
        N = _n(c, L)
        assert N == int(name.split("_")[0])
        assert launch_shape(N, axes, faces)["gx"] >= 2 and launch_shape(_n(c, L - 1), axes, faces)["gx"] >= (2 if N > 97 else 1)
        assert ((c - 1) & (c - 2)) != 0, "off the 2^k+1 ladder"
    c, L, axes = _BYTES
    assert _n(c, L) == 73 and launch_shape(73, axes, 0)["gx"] == 2
    c, L, axes, faces, _ = _BIG
    sh = launch_shape(_n(c, L), axes, faces)
    assert (_n(c, L), sh["chunk"], sh["gz"], sh["last"]) == (513, 32, 17, 1) and sh["partials"] <= _max_partials()
    t = edge_targets(513, axes, faces)
    assert {31, 32, 33, 512} <= set(t[:, 0])


def test_sample_covers_every_pair():
    """every boundary word runs with the constant operator and with eps, and at sigma 0 and at 3.5 -- not the product"""
    assert len(_WORDS) == 17 and len(set(_SAMPLE)) == len(_SAMPLE) == 34
    for c, axes, faces in _WORDS:
        assert NR.valid(axes, faces)
        mine = [(field, sigma) for c_, _, a, f, field, sigma in _SAMPLE if (c_, a, f) == (c, axes, faces)]
        assert {f for f, _ in mine} == {None, "exp"} and {s for _, s in mine} == {0.0, 3.5}
    ops = {(field, sigma) for _, _, _, _, field, sigma in _SAMPLE}
    assert ops == {(None, 0.0), (None, 3.5), ("exp", 0.0), ("exp", 3.5)}


_SENSITIVITY = sorted({(c, L, a, f, field, False) for c, L, a, f, field, _ in _SAMPLE}
                      | {(c, L, a, f, None, True) for c, L, a, f, _, _, _ in _PAIR_CASES}, key=str)


@pytest.mark.parametrize("c,L,axes,faces,field,pairs", _SENSITIVITY)
def test_the_reference_sees_every_tail(c, L, axes, faces, field, pairs):
    """with the bytes of one tail alone cleared, the restated colour pass (each colour), residual and prolongation give
    other bits on the finest level: a kernel that ignored the mask in that tail would not pass the GPU tests below"""
    N = _n(c, L)
    e = _eps(field, N, axes)
    h, sigma = 1.0 / (N - 1), 3.5
    m = MR.stored(edge_mask(N, axes, faces), axes)
    rng = np.random.default_rng(N + faces)
    u, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    nc = (N + 1) // 2
    ec = rng.standard_normal((nc, nc, nc))
    NR.refresh(u, axes)
    NR.refresh(ec, axes)

    def run(mask):
        out = []
        for colour in (1, 0):
            v = u.copy()
            MR.colour_pass(v, d, e, h, sigma, axes, faces, colour, mask)
            out.append(v)
        r = np.zeros((N, N, N))
        MR.residual(u, d, e, h, sigma, axes, faces, mask, r)
        v = u.copy()
        MR.prolong(ec, v, axes, faces, mask)
        return out + [r, v]

    base = run(m)
    regs = regions(N, axes, faces, pairs)
    assert len(regs) == (5 if faces else 4)
    for name, reg in regs.items():
        cleared = m.copy()
        cleared[reg] = 0
        moved = reg.copy()
        NR.refresh(moved, axes)  # a duplicate follows its source
        for what, a, b in zip(("red pass", "black pass", "residual", "prolong"), base, run(cleared)):
            assert not _same_bits(a, b), (name, what)
            assert _same_bits(a[~moved], b[~moved]), (name, what)  # (and nothing else moved)


# ----------------------------------------------------------------------------------------------- GPU: helpers
def _solver(c, L, nu, sigma, eps, axes, faces, mask, factor=True, keep_r=False):
    import multigrid_parallel_amd as M
    s = M.Solver(c, L, nu)
    s.set_keep_residual(keep_r)
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


def _norm_ok(got, exact, n):
    print(f"norm {got!r} exact {exact!r}")
    return abs(got - exact) <= norm_rtol(n) * exact


# ------------------------------------------------------------------------------ 2 single operators at the tails
def _single_operators(c, L, axes, faces, field, sigma):
    N = _n(c, L)
    top = _eps(field, N, axes)
    E = [None] * L if top is None else CR.inject(top, L)
    masks = MR.inject(MR.stored(edge_mask(N, axes, faces), axes), L)
    rng = np.random.default_rng(1000 * c + 64 * axes + faces)
    with _solver(c, L, 1, sigma, top, axes, faces, masks[-1], factor=False) as s:
        assert s.has_mask()
        for l in (L - 1, L - 2):
            n, h, e, m = s.level_n(l), s.level_h(l), E[l], masks[l]
            assert np.array_equal(s.get_mask(l), m), f"the injected mask of level {l}"
            fx = MR.fixed(m, axes, faces)
            assert fx.any()
            u, d = rng.standard_normal((n, n, n)), rng.standard_normal((n, n, n))
            d[fx] = np.nan  # never read
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
            assert _norm_ok(got, MR.exact_residual_norm(u, d, e, h, sigma, axes, faces, m), n)

            got = s.smooth_residual(l, 1, 2, store=True)
            MR.post_smooth(u, d, e, h, sigma, axes, faces, 2, m)
            MR.residual(u, d, e, h, sigma, axes, faces, m, r)
            got_u = s.download(MG3D_U, l).reshape(n, n, n)
            got_r = s.download(MG3D_R, l).reshape(n, n, n)
            assert _same_bits(got_u, u) and _same_bits(got_u[fx], u_in[fx]), f"smooth_residual u, level {l}"
            assert _same_bits(got_r, r), f"smooth_residual r, level {l}"
            assert not got_r[fx].any() and not np.signbit(got_r[fx]).any()
            assert _norm_ok(got, MR.exact_residual_norm(u, d, e, h, sigma, axes, faces, m), n)

            nc = s.level_n(l - 1)
            dc = rng.standard_normal((nc, nc, nc))
            s.upload(MG3D_D, l - 1, dc)
            s.restrict(l)
            NR.restrict(r, dc, axes, faces)  # (unchanged: it reads the zeros the residual stored)
            assert _same_bits(s.download(MG3D_D, l - 1), dc), f"restrict, level {l}"

            dc = rng.standard_normal((nc, nc, nc))
            s.upload(MG3D_D, l - 1, dc)
            s.smooth_restrict(l, 2)
            MR.pre_smooth(u, d, e, h, sigma, axes, faces, 2, m)
            MR.residual(u, d, e, h, sigma, axes, faces, m, r)
            NR.restrict(r, dc, axes, faces)
            got_u = s.download(MG3D_U, l).reshape(n, n, n)
            assert _same_bits(got_u, u) and _same_bits(got_u[fx], u_in[fx]), f"smooth_restrict u, level {l}"
            assert _same_bits(s.download(MG3D_D, l - 1), dc), f"smooth_restrict d, level {l - 1}"
            assert _same_bits(s.download(MG3D_D, l).reshape(n, n, n)[~fx], d[~fx]), f"d of level {l} was written"

            ec = rng.standard_normal((nc, nc, nc))  # faces included
            NR.refresh(ec, axes)
            s.upload(MG3D_U, l - 1, ec)
            before = u.copy()
            s.prolong(l)
            MR.prolong(ec, u, axes, faces, m)
            got_u = s.download(MG3D_U, l).reshape(n, n, n)
            assert _same_bits(got_u, u), f"prolong, level {l}"
            assert _same_bits(got_u[fx], before[fx]) and not _same_bits(got_u, before)


@gpu
@pytest.mark.parametrize("c,L,axes,faces,field,sigma", _SAMPLE)
def test_single_operators_at_the_tails(c, L, axes, faces, field, sigma):
    """69^3 and 73^3, the top two levels: smooth pre and post, residual with and without r (d NaN at the fixed unknowns),
    smooth_residual, restrict, smooth_restrict, prolong of random coarse data"""
    _single_operators(c, L, axes, faces, field, sigma)


@gpu
@pytest.mark.parametrize("c,L,axes,faces,sigma,pairs,live", _PAIR_CASES)
def test_constant_pass_past_one_k_block(c, L, axes, faces, sigma, pairs, live):
    """smooth_color_kernel<*, true> with 65 and 73 k-pairs -- a second block in k -- and the residual, the finest level"""
    N = _n(c, L)
    m = MR.stored(edge_mask(N, axes, faces), axes)
    fx = MR.fixed(m, axes, faces)
    rng = np.random.default_rng(N + faces)
    u, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    d[fx] = np.nan
    u_in = u.copy()
    with _solver(c, L, 1, sigma, None, axes, faces, m, factor=False) as s:
        l, h = L - 1, s.level_h(L - 1)
        s.upload(MG3D_U, l, u)
        s.upload(MG3D_D, l, d)
        s.smooth(l, 0, 1)
        MR.pre_smooth(u, d, None, h, sigma, axes, faces, 1, m)
        assert _same_bits(s.download(MG3D_U, l), u), "pre-smoothing"
        s.smooth(l, 1, 1)
        MR.post_smooth(u, d, None, h, sigma, axes, faces, 1, m)
        got_u = s.download(MG3D_U, l).reshape(N, N, N)
        assert _same_bits(got_u, u), "post-smoothing"
        assert _same_bits(got_u[fx], u_in[fx]) and np.isfinite(got_u).all()
        r = rng.standard_normal((N, N, N))
        r_in = r.copy()
        s.upload(MG3D_R, l, r)
        norm_only = s.residual(l, store=False)
        assert _same_bits(s.download(MG3D_R, l), r_in), "the norm-only residual writes no r"
        got = s.residual(l, store=True)
        MR.residual(u, d, None, h, sigma, axes, faces, m, r)
        got_r = s.download(MG3D_R, l).reshape(N, N, N)
        assert _same_bits(got_r, r), "residual"
        assert not got_r[fx].any() and not np.signbit(got_r[fx]).any() and got == norm_only
        assert _norm_ok(got, MR.exact_residual_norm(u, d, None, h, sigma, axes, faces, m), N)


# ------------------------------------------------------------------- 3 the apply pass and the count, through the solvers
def _solver_problem(name):
    """(Hierarchy factory, mask, x0, d) of a solver case: edge_mask, x0 and d random"""
    c, L, sigma, field, axes, faces = _SOLVER_CASES[name]
    N = _n(c, L)
    eps = _eps(field, N, axes)
    mask = edge_mask(N, axes, faces)
    rng = np.random.default_rng(N + faces + 64 * axes)
    x0, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    NR.refresh(x0, axes)
    NR.refresh(d, axes)
    return (lambda: MR.Hierarchy(c, L, 2, sigma, eps, axes, faces, mask)), eps, mask, x0, d


def spread_table():
    """the summation spread of each solver case (_mask_ref.spread): {name: ([u at k = 1, 2], norms)}"""
    out = {}
    for name in _SOLVER_CASES:
        make, _, _, x0, d = _solver_problem(name)
        out[name] = MR.spread(make, x0, d, (1, 2))
    return out


# measured, see the table above: the largest over the four cases
SPREAD_U = {1: 8.23e-16, 2: 6.88e-16}
SPREAD_NORM = 3.55e-15


def _tolerances(call, k):
    import test_gpu_pcg as TP
    import test_gpu_wpcg as TW
    f = TW if call == "wpcg_solve" else TP
    return 100 * max(SPREAD_U[k], f.SPREAD_U[k]), 100 * max(SPREAD_NORM, f.SPREAD_NORM)


_solver_refs = {}


def _solver_ref(name):
    if name not in _solver_refs:
        make, eps, mask, x0, d = _solver_problem(name)
        prob = make()
        assert not MR.is_singular(prob)
        hist = []
        _, norms, _, _, _ = MR.wpcg(prob, x0, d, 0., 1e-300, 2, "exact", hist)
        _solver_refs[name] = (eps, mask, x0, d, hist, norms)
    return _solver_refs[name]


@gpu
@pytest.mark.parametrize("name,call", [(n, call) for n, v in _SOLVER_CASES.items() for call in ("pcg_solve", "wpcg_solve")
                                       if call == "wpcg_solve" or not v[5]])
def test_solver_iterates(name, call):
    """u and the norms after k = 1 and 2 iterations against _mask_ref.wpcg from a random x0 with random d; the fixed values
    bitwise, the duplicates equal to their sources"""
    c, L, sigma, _, axes, faces = _SOLVER_CASES[name]
    N = _n(c, L)
    eps, mask, x0, d, hist, ref_norms = _solver_ref(name)
    fx = MR.fixed(MR.stored(mask, axes), axes, faces)
    with _solver(c, L, 2, sigma, eps, axes, faces, mask) as s:
        s.upload(MG3D_D, L - 1, d)
        for k in (1, 2):
            s.upload(MG3D_U, L - 1, x0)
            norms, info = getattr(s, call)(rtol=0.0, atol=1e-300, max_iters=k)
            assert info["iterations"] == k and len(norms) == k + 1 and not info["converged"]
            if call == "wpcg_solve":
                assert info["singular"] == 0 and info["rhs_mean"] == 0.
            u = s.download(MG3D_U, L - 1).reshape(N, N, N)
            rel = np.abs(u - hist[k - 1]).max() / np.abs(hist[k - 1]).max()
            nrel = (np.abs(norms - ref_norms[:k + 1]) / ref_norms[:k + 1]).max()
            tol_u, tol_n = _tolerances(call, k)
            print(name, call, k, "u", rel, "of", tol_u, "norms", nrel, "of", tol_n)
            assert rel <= tol_u and nrel <= tol_n
            assert _same_bits(u[fx], x0[fx])
            w = u.copy()
            NR.refresh(w, axes)
            assert _same_bits(u, w), "duplicates differ from their sources"
        assert _same_bits(s.download(MG3D_D, L - 1), d)


@gpu
@pytest.mark.parametrize("point", [(64, 64, 64), (63, 64, 64), (1, 1, 64), None])
def test_the_count_sees_one_fixed_unknown(point):
    """mask_count_kernel at 65^3 with all six faces Neumann and sigma = 0 -- 65 unknowns per axis: a second k-block, a last
    row block and a last chunk of ONE member each.  One fixed unknown in that corner (it survives down to level 0: the
    pin goes), one beside it and one on the high k face alone (the finest level only) make the operator regular; no
    fixed unknown: singular, projected"""
    c, L, N = 9, 4, 65
    rng = np.random.default_rng(2)
    d = rng.standard_normal((N, N, N))
    u0 = np.zeros((N, N, N))
    mask = np.zeros((N, N, N), dtype=np.uint8)
    if point is None:
        with _solver(c, L, 2, 0.0, None, 0, 63, mask) as s:
            s.upload(MG3D_U, L - 1, u0)
            s.upload(MG3D_D, L - 1, d)
            _, info = s.wpcg_solve(rtol=1e-8, max_iters=60)
            assert info["singular"] == 1 and info["converged"]
        return
    mask[point] = 1
    u0[point] = 0.75
    prob = MR.Hierarchy(c, L, 2, 0.0, None, 0, 63, mask)
    assert MR.pinned(0, 63, 0.0, prob.mask[0]) == (point != (64, 64, 64)) and not MR.is_singular(prob)
    assert prob.fixed().sum() == 1
    x, ref_norms, ok, _, _ = MR.wpcg(prob, u0, d, 1e-8, 0.0, 60)
    assert ok
    with _solver(c, L, 2, 0.0, None, 0, 63, mask) as s:
        s.upload(MG3D_U, L - 1, u0)
        s.upload(MG3D_D, L - 1, d)
        norms, info = s.wpcg_solve(rtol=1e-8, max_iters=60)
        print(point, "iterations", info["iterations"], "reference", len(ref_norms) - 1)
        assert info["singular"] == 0 and info["rhs_mean"] == 0. and info["converged"]
        assert info["iterations"] == len(ref_norms) - 1
        u = s.download(MG3D_U, L - 1).reshape(N, N, N)
        assert u[point] == 0.75
        assert np.abs(u - x).max() <= 1e-6 * np.abs(x).max()


# --------------------------------------------------- 4 cycles off the ladder and where the unmasked context runs ahead
def _cycle_mask(name):
    c, L, _, _, _, axes, faces, _ = _CYCLE_CASES[name]
    m = edge_mask(_n(c, L), axes, faces)
    return _odd_only(m) if name.endswith("_odd") else m


def _cycle_start(name):
    c, L, _, _, _, axes, faces, _ = _CYCLE_CASES[name]
    N = _n(c, L)
    rng = np.random.default_rng(N + faces + 64 * axes)
    u, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    NR.refresh(u, axes)
    NR.refresh(d, axes)
    return u, d


_first_cycle = {}  # name -> u of the finest level after the first restated cycle (the state test shares the 161^3 one)


def _assert_levels(s, ref, keep_r):
    for l in range(ref.L):
        assert _same_bits(s.download(MG3D_U, l), ref.u[l]), f"u level {l}"
        if l < ref.L - 1:
            assert _same_bits(s.download(MG3D_D, l), ref.d[l]), f"d level {l}"
        if keep_r:
            assert _same_bits(s.download(MG3D_R, l), ref.r[l]), f"r level {l}"


@gpu
@pytest.mark.parametrize("name", list(_CYCLE_CASES))
def test_cycles(name):
    """mg3d_vcycle, then mg3d_vcycles(1): u of every level, d below the top (r of every level with keep_residual) bit for
    bit after each, the norms"""
    c, L, nu, sigma, field, axes, faces, keep_r = _CYCLE_CASES[name]
    N = _n(c, L)
    eps = _eps(field, N, axes)
    mask = _cycle_mask(name)
    ref = MR.Hierarchy(c, L, nu, sigma, eps, axes, faces, mask)
    assert ref.fixed().any()
    if name.endswith("_odd"):
        assert not ref.fixed(L - 2).any() and MR.pinned(axes, faces, sigma, ref.mask[0])
    else:
        assert ref.fixed(0).any()
        if faces:  # coarse_rhs_kernel<true> and the coarse matrix meet fixed unknowns on both Neumann faces of level 0
            assert faces == 3 and ref.fixed(0)[0].any() and ref.fixed(0)[-1].any()
    u, d = _cycle_start(name)
    ref.u[-1][...] = u
    ref.d[-1][...] = d
    fx = ref.fixed()
    with _solver(c, L, nu, sigma, eps, axes, faces, mask, keep_r=keep_r) as s:
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        want = [ref.vcycle()]
        _first_cycle[name] = ref.u[-1].copy()
        got = [s.vcycle()]
        _assert_levels(s, ref, keep_r)
        want.append(ref.vcycle())
        got += list(s.vcycles(1))
        _assert_levels(s, ref, keep_r)
        assert _same_bits(s.download(MG3D_U, L - 1).reshape(N, N, N)[fx], u[fx])
    print(name, "norms", got, "reference", want)
    np.testing.assert_allclose(got, want, rtol=norm_rtol(N), atol=0)


@gpu
def test_set_mask_behind_a_cycle_that_ran_ahead():
    """161^3, all Dirichlet, constant: a context without a mask runs vcycles(2) -- one launch per leg, the next down-leg
    run ahead --, then set_mask, a new u and d and vcycles(1): the masked restatement's bits; then set_mask(None) and the
    same upload: the bits of a fresh context without a mask"""
    import multigrid_parallel_amd as M
    name = "161"
    c, L, nu, sigma, _, axes, faces, _ = _CYCLE_CASES[name]
    N = _n(c, L)
    mask = _cycle_mask(name)
    u, d = _cycle_start(name)
    if name not in _first_cycle:
        ref = MR.Hierarchy(c, L, nu, sigma, None, axes, faces, mask)
        ref.u[-1][...] = u
        ref.d[-1][...] = d
        ref.vcycle()
        _first_cycle[name] = ref.u[-1].copy()
    rng = np.random.default_rng(7)
    with M.Solver(c, L, nu) as a, M.Solver(c, L, nu) as b:
        for s in (a, b):
            s.get_details()
        a.upload(MG3D_U, L - 1, rng.standard_normal(N ** 3))
        a.upload(MG3D_D, L - 1, rng.standard_normal(N ** 3))
        a.vcycles(2)
        a.set_mask(mask)
        assert a.has_mask()
        a.upload(MG3D_U, L - 1, u)
        a.upload(MG3D_D, L - 1, d)
        a.vcycles(1)
        assert _same_bits(a.download(MG3D_U, L - 1), _first_cycle[name])
        a.set_mask(None)
        assert not a.has_mask()
        for s in (a, b):
            s.upload(MG3D_U, L - 1, u)
            s.upload(MG3D_D, L - 1, d)
        na, nb = a.vcycles(1), b.vcycles(1)
        assert np.array_equal(na, nb)
        assert _same_bits(a.download(MG3D_U, L - 1), b.download(MG3D_U, L - 1))
        assert _same_bits(a.download(MG3D_D, L - 2), b.download(MG3D_D, L - 2))


# ------------------------------------------------------------------------------------ 5 the byte kernels at two k-blocks
@gpu
def test_device_form_at_two_k_blocks():
    """73^3 with periodic i and k: set_mask_tensor from uint8 and bool tensors, contiguous, permuted, sliced out of a
    larger one and zero-stride broadcast -- on every level the restatement's bytes and the host form's.  Then the axes
    cleared and set under the mask: a duplicate keeps its source's bytes for good (include/mg3d.h)"""
    import multigrid_parallel_amd as M
    c, L, axes = _BYTES
    N = _n(c, L)
    dev = torch.device("cuda:0")
    mask = edge_mask(N, axes, 0) * np.uint8(3)
    plate = np.zeros((N, N, N), dtype=np.uint8)
    plate[[0, 1, 31, 32, 64, 65, N - 2]] = 7
    with M.Solver(c, L, 1) as h, M.Solver(c, L, 1) as g:
        for s in (h, g):
            s.set_periodic(axes)
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
            want = MR.inject(MR.stored(np.asarray(host).astype(np.uint8), axes), L)
            assert not np.array_equal(want[-1], np.asarray(host).astype(np.uint8)), "a duplicate's own bytes"
            for l in range(L):
                got = g.get_mask(l)
                assert np.array_equal(got, want[l]) and np.array_equal(h.get_mask(l), got), (name, l)
        # under the contiguous mask again: every setter refreshes the duplicates of the axes it is given and keeps the rest
        for s, setm in ((h, lambda: h.set_mask(mask)), (g, lambda: g.set_mask_tensor(t))):
            setm()
            kept = MR.stored(mask, axes)
            s.set_periodic(0)
            assert np.array_equal(s.get_mask(L - 1), kept)
            s.set_periodic(2)
            s.set_neumann(3)
            kept[:, N - 1, :] = kept[:, 0, :]  # planes i = N-1 and k = N-1 still hold the bytes of i = 0 and k = 0
            assert not np.array_equal(kept, MR.stored(mask, 2)) and np.array_equal(kept[N - 1], kept[0])
            want = MR.inject(kept, L)
            for l in range(L):
                assert np.array_equal(s.get_mask(l), want[l]), l
            assert (s.periodic, s.neumann) == (2, 3)


# --------------------------------------------------------------------------------------------------- 6 past the cap
@gpu
def test_past_the_partial_cap():
    """513^3, both i faces Neumann, eps: chunk 32 and 17 chunks, the last one the single plane of the high Neumann face;
    fixed unknowns in planes 31, 32, 33 and 512 among the others.  One colour pass of each colour and the residual with r
    against the block forms of the restatement"""
    c, L, axes, faces, sigma = _BIG
    N = _n(c, L)
    mask = edge_mask(N, axes, faces)
    t = edge_targets(N, axes, faces)
    fx = MR.fixed(mask, axes, faces)
    assert fx[t[:, 0], t[:, 1], t[:, 2]].all() and 2 * fx.sum() <= NR.unknown_mask(N, axes, faces).sum()
    for plane in (31, 32, 33, 512):
        assert fx[plane].any()
    rng = np.random.default_rng(N + faces)
    u, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    d[fx] = np.nan
    e = _eps("exp", N, axes)
    with _solver(c, L, 1, sigma, e, axes, faces, mask, factor=False) as s:
        top, h = L - 1, s.level_h(L - 1)
        s.upload(MG3D_U, top, u)
        s.upload(MG3D_D, top, d)
        fixed_in = u[fx].copy()
        s.smooth(top, 0, 1)
        MR.colour_pass_blocks(u, d, e, h, sigma, axes, faces, 1, mask)
        MR.colour_pass_blocks(u, d, e, h, sigma, axes, faces, 0, mask)
        got = s.download(MG3D_U, top).reshape(N, N, N)
        assert _same_bits(got, u), "smooth"
        assert _same_bits(got[fx], fixed_in)
        del got
        s.zero(MG3D_R, top)
        nrm = s.residual(top, store=True)
        r = np.zeros((N, N, N))
        want = MR.residual_blocks(u, d, e, h, sigma, axes, faces, mask, r)
        got = s.download(MG3D_R, top).reshape(N, N, N)
        assert _same_bits(got, r), "residual"
        assert not got[fx].any()
    assert _norm_ok(nrm, want, N)


if __name__ == "__main__":
    print(f"{'':20s} u, k = 1    k = 2       norms")
    for name, (su, sn) in spread_table().items():
        print(f"    {name:16s} " + "    ".join(f"{v:.2e}" for v in su) + f"    {sn:.2e}")
