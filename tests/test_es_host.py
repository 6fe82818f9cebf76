"""The mixed-boundary ("electrospray") path without a GPU: the host's coarse matrix against the statement's, byte for byte,
off the default parameters; the two parameter structs; and -- counted with the statement's own predicates and the launch
arithmetic of csrc/mg3d_es.hip restated -- that the parameter sets and sizes of tests/test_gpu_es_shapes.py reach what its
cases are there for.  A changed set, size or grid fails here instead of leaving a GPU case vacuous.

The case tables of the GPU file live here, so that this file imports nothing that needs a device."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import P

# (c, L) of the GPU cases, by what they run
SMOOTH_TOP = [(5, 4), (5, 5), (5, 6), (10, 5), (6, 6)]  # 33, 65, 129, 145, 161
SMOOTH_LOWER = [(10, 5), (5, 5)]  # every level below the finest: 10 19 37 73, 5 9 17 33
FILL = [(5, 5), (10, 5), (6, 6)]  # 65, 145, 161
ONE_CYCLE = [(5, 4, 2), (3, 5, 1), (10, 5, 2), (6, 6, 2)]  # (c, L, nu)
THREE_CYCLES = [(10, 5, s) for s in O.ES_SETS] + [(6, 6, "default"), (6, 6, "wide")]
BATCH = (5, 3)  # 17^3, 1025 cycles: sets default and lattice
BEHIND = (6, 6)

# the level-0 spacings mg3d_es_setup is asked for: the hierarchies above and those of tests/test_electrospray.py
_COARSE = {3: (5,), 5: (3, 4, 5, 6), 6: (6,), 9: (3, 5), 10: (5,), 11: (3,)}


def _n(c, L):
    return O.level_sizes(c, L)[-1]


def _gpu_sizes():
    return sorted({_n(c, L) for c, L in SMOOTH_TOP + FILL} | {_n(c, L) for c, L, _ in ONE_CYCLE + THREE_CYCLES}
                  | {_n(*BATCH), _n(*BEHIND)})


def test_the_sizes():
    assert _gpu_sizes() == [17, 33, 65, 129, 145, 161]
    assert [_n(c, L) for c, L in SMOOTH_TOP] == [33, 65, 129, 145, 161] and [_n(c, L) for c, L in FILL] == [65, 145, 161]
    assert all(n % 2 == 1 for n in _gpu_sizes())  # the centre of a face is a grid point: the lattice offsets exist


# ------------------------------------------------------------------------------------------------ 1 the coarse matrix
@pytest.mark.parametrize("name", O.ES_SETS)
@pytest.mark.parametrize("c", sorted(_COARSE))
def test_coarse_matrix_is_the_statements(c, name):
    """mg3d_es_coarse_matrix = orc_es_coarse_matrix byte for byte at the spacing of level 0, and its zero-gradient rows
    are the face points that the statement's predicates leave: 6 (c-2)^2 less the patch points inside the two x faces"""
    for L in _COARSE[c]:
        N = _n(c, L)
        po, pm = O.es_params(name, N)
        h0 = po.length / (N - 1) * (1 << (L - 1))  # mg_3d.h:287
        n = c ** 3
        want, got = np.zeros(n * n), np.zeros(n * n)
        O.lib().orc_es_coarse_matrix(O.P(want), c, h0, C.byref(po))
        M.lib().mg3d_es_coarse_matrix(P(got), c, h0, C.byref(pm))
        assert got.tobytes() == want.tobytes(), (c, L)
        x0, xl = O.es_patches(po, c, h0)
        walls = 6 * (c - 2) ** 2 - int(x0[1:-1, 1:-1].sum()) - int(xl[1:-1, 1:-1].sum())
        assert int((got == -1.0).sum()) == walls, (c, L)


def test_coarse_matrix_meets_patches():
    """some level 0 of the list has patch rows on each x face (the branch that leaves the identity row is taken)"""
    seen0 = seenl = 0
    for name in O.ES_SETS:
        for c, Ls in _COARSE.items():
            for L in Ls:
                N = _n(c, L)
                po, _ = O.es_params(name, N)
                x0, xl = O.es_patches(po, c, po.length / (N - 1) * (1 << (L - 1)))
                seen0 += int(x0[1:-1, 1:-1].sum())
                seenl += int(xl[1:-1, 1:-1].sum())
    assert seen0 > 10 and seenl > 10


# ------------------------------------------------------------------------------- 2 what the GPU cases rely on
@pytest.mark.parametrize("N", [n for n in _gpu_sizes() if n >= 145])
def test_wide_reaches_the_second_k_block(N):
    """x = L has patch and non-patch points with k >= 128: es_ghost's patch branch is taken and not taken from the second
    block of es_color_kernel (rows 1 .. N-2), and the third block of es_fill_kernel (64 points of k each) writes and skips.
    The disc of x = 0 ends before k = 128 (radius 43 h at 145^3, 48 h at 161^3): there the second block of the colour
    pass only copies, and the disc is written by the first two blocks of the fill"""
    po, _ = O.es_params("wide", N)
    x0, xl = O.es_patches(po, N, po.length / (N - 1))
    assert xl[:, 128:].any() and (~xl[:, 128:]).any()
    assert xl[1:-1, 128:N - 1].any() and (~xl[1:-1, 128:N - 1]).any()
    assert (~x0[1:-1, 128:N - 1]).any() and not x0[:, 129:].any()
    assert x0[:, :64].any() and x0[:, 64:128].any() and (~x0[:, 64:128]).any()


@pytest.mark.parametrize("N", [n for n in _gpu_sizes() if n >= 33])
def test_wide_reaches_the_walls(N):
    """patch points of x = L on the rows next to every wall and on a face edge: the threads of es_color_kernel that write
    the j and k walls meet "patch: do not copy"; the disc has many points and both faces keep wall points"""
    po, _ = O.es_params("wide", N)
    x0, xl = O.es_patches(po, N, po.length / (N - 1))
    assert xl[1:-1, N - 2].any() and xl[1:-1, 1].any() and xl[1, 1:-1].any() and xl[N - 2, 1:-1].any()
    assert xl[:, N - 1].any() and xl[:, 0].any() and xl[0, :].any() and xl[N - 1, :].any()
    assert not xl[0, 0] and not xl[N - 1, N - 1]  # (the corners of the face are outside the annulus)
    assert x0.sum() > 0.25 * N * N and not x0.all() and not xl.all()


def test_wide_at_145_as_counted():
    po, _ = O.es_params("wide", 145)
    _, xl = O.es_patches(po, 145, po.length / 144)
    assert (int(xl[:, 143].sum()), int(xl[:, 144].sum()), int(xl[:, 128:].sum())) == (129, 127, 2331)


@pytest.mark.parametrize("N", _gpu_sizes())
def test_lattice_meets_the_comparisons_with_equality(N):
    """offsets from the centre of the face, in units of h: (3, 4) and (5, 0) lie ON the disc's circle and are in (<=);
    (4, 4) is out; (6, 8) and (5, 12) lie ON the annulus's two circles and are out (strict); (10, 1) and (12, 4) are in"""
    po, _ = O.es_params("lattice", N)
    h, m = po.length / (N - 1), (N - 1) // 2
    assert h == O.ES_LATTICE_H and po.length / 2. == m * h
    x0, xl = O.es_patches(po, N, h)
    assert x0[m + 3, m + 4] and x0[m + 5, m] and not x0[m + 4, m + 4]
    assert x0[m - 4, m + 3] and x0[m, m - 5]
    assert not xl[m + 6, m + 8] and not xl[m - 8, m - 6]
    if N > 17:  # (at 17^3 the face ends 8 h from its centre: the outer circle is met from 33^3 on)
        assert not xl[m + 5, m + 12] and xl[m + 10, m + 1] and xl[m + 12, m + 4] and not xl[m - 12, m + 5]
    else:
        assert xl[m + 8, m + 7] and not xl[m + 8, m + 6]  # 113 and, on the inner circle, 100
    j, k = np.ogrid[:N, :N]
    rr = (j - m) ** 2 + (k - m) ** 2  # whole numbers: the predicates in exact arithmetic
    assert np.array_equal(x0, rr <= 25) and np.array_equal(xl, (rr > 100) & (rr < 169))


def _live(N, lane_lo, lane_hi, parity):
    """lanes m of [lane_lo, lane_hi) whose k = 2m + parity is an interior point (es_color_kernel)"""
    return [m for m in range(lane_lo, lane_hi) if 1 <= 2 * m + parity <= N - 2]


def test_lanes_of_the_second_k_block():
    """es_color's grid restated: a lane owns (2m, 2m+1), 64 lanes to a block.  129^3 launches a second block in which no
    lane is live; 145^3 has 8 and 161^3 has 16 live lanes there, and the copy onto k = N-1 is made from that block"""
    for N, live in ((129, 0), (145, 8), (161, 16)):
        gx = ((N + 1) // 2 + 63) // 64
        assert gx == 2
        for parity in (0, 1):
            assert len(_live(N, 64, 128, parity)) == live
            assert len(_live(N, 0, 64, parity)) == 64 - (parity == 0)  # k = 0 is the wall
        assert ((N - 2) // 2 >= 64) == (live > 0)  # the lane of k = N-2
    for N in (33, 65):
        assert ((N + 1) // 2 + 63) // 64 == 1
    # the last row block: 145 -> 3 rows, 161 -> 3, 129 -> 3
    assert [(N - 2 - 1) % 4 + 1 for N in (129, 145, 161)] == [3, 3, 3]


def test_fill_kernel_second_block():
    """es_fill_kernel: 64 points of k to a block, every k of the face.  At 65^3 the second block has one lane (k = 64);
    no set of the GPU cases makes it write there but the wide one -- which is why the fill is looked at with it"""
    N = 65
    for name in O.ES_SETS:
        po, _ = O.es_params(name, N)
        x0, xl = O.es_patches(po, N, po.length / (N - 1))
        assert (x0[:, 64:].any() or xl[:, 64:].any()) == (name == "wide")


# --------------------------------------------------------------------------------------------------- 3 the structs
def test_the_two_structs_have_one_layout():
    assert C.sizeof(M.EsParams) == C.sizeof(O.EsParams) == 48
    mine, theirs = M.EsParams._fields_, O.EsParams._fields_
    assert len(mine) == len(theirs) == 6
    for (a, ta), (b, tb) in zip(mine, theirs):
        assert ta is tb is C.c_double
        assert getattr(M.EsParams, a).offset == getattr(O.EsParams, b).offset
        assert a == b or a == b + "_radius"
    for name in O.ES_SETS:
        po, pm = O.es_params(name, 145)
        assert bytes(po) == bytes(pm)
    d = M.EsParams.default()
    assert bytes(d) == bytes(O.EsParams())
