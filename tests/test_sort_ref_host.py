"""The restatement of the particle reorder (tests/_sort_ref.py) and the coverage of the GPU cases, without a GPU: the cases
of tests/test_gpu_sort.py are held to what they were chosen for -- every class of particle, ties across tiles, every number
of sort passes, wrapped coordinates, the edge points."""
import numpy as np
import pytest

import _particle_ref as PR
import _push_ref as QR
import _sort_ref as SR


def _keys(N, bc, count, shift=0, with_fate=True):
    xyz, fate = SR.particles(N, bc, count)
    return SR.keys(xyz, fate if with_fate else None, SR.spacing(N), N, QR.BCS[bc][0], shift)


def test_key_ranges_and_passes():
    """6, 12, 18, 22 and 25 bits of cell keys at shift 0, fewer at shift 2; the keys of 321 pass 24 bits: a fourth pass of
    8-bit digits (a fifth of 6-bit ones)"""
    sizes = (5, 17, 65, 161, 321)
    assert [SR.key_bits(N, 0) for N in sizes] == [6, 12, 18, 22, 25]
    assert [SR.key_bits(N, 2) for N in sizes] == [0, 6, 12, 16, 19]
    assert all(SR.key_bits(N, 2) < SR.key_bits(N, 0) for N in sizes)
    assert [SR.passes(N, 0) for N in sizes] == [1, 2, 3, 3, 4]
    assert [SR.passes(N, 2) for N in sizes] == [1, 1, 2, 2, 3]
    assert SR.passes(321, 8) == 1 and SR.blocks(321, 8) == 2
    assert -(-25 // 6) == 5 and -(-SR.key_bits(161, 0) // 8) == 3
    assert SR.key_bits(257, 0) == 24 and SR.passes(257, 0) == 4 and SR.passes(161, 0) == 3  # (KMAX + 1 = 2^24 + 1 at 257)
    for N, (c, L) in SR.SIZES.items():
        assert (c - 1) * 2 ** (L - 1) + 1 == N


def test_restatement_on_a_case_by_hand():
    """N = 5, h = 1/4, shift 0 and 1: keys by hand, the stable order, the counts, the permute"""
    h = 0.25
    xyz = np.array([[0.9, 0.9, 0.9], [0.1, 0.1, 0.1], [1.0, 1.0, 1.0], [0.1, 0.1, 0.6], [np.nan, 0.1, 0.1], [0.1, 0.1, 0.1],
                    [0.1, 1.5, 0.1], [0.3, 0.1, 0.1]])
    fate = np.array([0, 0, 0, 0, 0, 7, 0, 0], dtype=np.int32)
    K = SR.keys(xyz, fate, h, 5, 0)
    assert K.tolist() == [63, 0, 63, 2, 64, 65, 64, 16]
    perm, counts = SR.sort(xyz, fate, h, 5, 0)
    assert perm.dtype == np.int32 and perm.tolist() == [1, 3, 7, 0, 2, 4, 6, 5] and counts.tolist() == [5, 2]
    assert SR.keys(xyz, None, h, 5, 0).tolist() == [63, 0, 63, 2, 64, 0, 64, 16]
    assert SR.keys(xyz, fate, h, 5, 0, shift=1).tolist() == [7, 0, 7, 1, 8, 9, 8, 0]
    # y = 1.5 wraps to 0.5 on a periodic j axis
    assert SR.keys(xyz, fate, h, 5, 2)[6] == (0 * 4 + 2) * 4 + 0
    vals = np.arange(8.0)
    assert SR.permute(perm, vals, xyz)[0].tolist() == [1., 3., 7., 0., 2., 4., 6., 5.]
    # float32 positions widen exactly
    x32 = xyz.astype(np.float32)
    assert np.array_equal(SR.keys(x32, fate, h, 5, 0), SR.keys(x32.astype(np.float64), fate, h, 5, 0))


@pytest.mark.parametrize("N,bc", SR.SMALL_CASES)
def test_small_cases_hold_every_class_and_the_edge_points(N, bc):
    axes = QR.BCS[bc][0]
    h = SR.spacing(N)
    edge = PR.edge_points(N, h, axes)
    for count in SR.SMALL_COUNTS:
        xyz, fate = SR.particles(N, bc, count)
        assert xyz.shape == (count, 3) and fate.shape == (count,) and fate.dtype == np.int32
        if count == 1:  # one particle has one class
            assert _keys(N, bc, 1)[0] < SR.kmax(N, 0)
            continue
        assert edge.shape[0] < count and np.array_equal(xyz[:edge.shape[0]], edge, equal_nan=True)
        for shift in (0, 2):
            inside, lost, dead = SR.classes(_keys(N, bc, count, shift), SR.kmax(N, shift))
            assert inside and lost and dead, (N, bc, count, shift)
            inside, lost, dead = SR.classes(_keys(N, bc, count, shift, with_fate=False), SR.kmax(N, shift))
            assert inside and lost and not dead
        if axes:
            length = (N - 1) * h
            ax = [a for a in range(3) if axes >> a & 1][0]
            finite = np.isfinite(xyz).all(axis=1)
            away = finite & ((xyz[:, ax] < 0.0) | (xyz[:, ax] > length))
            others_in = np.ones(count, dtype=bool)
            for a in range(3):
                if not axes >> a & 1:
                    others_in &= (xyz[:, a] >= 0.0) & (xyz[:, a] <= length)
            wrapped = away & others_in
            assert wrapped.any() and np.all(_keys(N, bc, count, 0, with_fate=False)[wrapped] < SR.kmax(N, 0))


@pytest.mark.parametrize("N,bc", SR.LARGE_CASES)
def test_large_cases_hold_every_class_and_ties_across_tiles(N, bc):
    for count in SR.LARGE_COUNTS:
        assert count > 3 * SR.FAR and count % SR.TILE not in (0, 1)
        for shift in (0, 2):
            K = _keys(N, bc, count, shift)
            inside, lost, dead = SR.classes(K, SR.kmax(N, shift))
            assert inside and lost and dead
            assert SR.far_ties(K, SR.kmax(N, shift)), (N, bc, count, shift)
    assert SR.LARGE_COUNTS[0] > 2048 * 256 and -(-SR.LARGE_COUNTS[1] // SR.TILE) > 1024
    assert sorted(N for N, _ in SR.LARGE_CASES) == [5, 17, 37, 65, 161, 321]
