"""CPU restatement of the particle reorder (mg3d_particle_sort(_device), mg3d_particle_permute_device; include/mg3d.h,
"Particles"): the keys from the locator of tests/_particle_ref.py with its periodic wrap, the fate rule of the header, numpy's
stable argsort -- stability makes the permutation unique --, the two counts from the keys, fancy indexing for the permute.

axes is the mask of periodic axes.  Positions are (M, 3).  Also the seeded particles of the sort tests, so that the host test
can hold the cases of the GPU test to their coverage.  Test infrastructure only."""
import functools

import numpy as np

import _particle_ref as PR
import _push_ref as QR

TILE = 2048  # MG3D_SORT_TILE (csrc/mg3d_internal.h): elements per tile of a sort pass
MAX_SHIFT = 8
MAX_COUNT = (1 << 31) - 1


def blocks(N, shift):
    """nb: blocks of 2^shift cells per side"""
    return ((N - 2) >> shift) + 1


def kmax(N, shift):
    return blocks(N, shift) ** 3


def key_bits(N, shift):
    """the bits of the largest cell key KMAX - 1"""
    return (kmax(N, shift) - 1).bit_length()


def passes(N, shift):
    """the 8-bit digits of the largest key KMAX + 1: the passes of the sort (1 + 3 * passes launches)"""
    return ((kmax(N, shift) + 1).bit_length() + 7) // 8


def keys(xyz, fate, h, N, axes, shift=0):
    """K (M,) int64: the cell key of a living particle inside, KMAX of a lost one, KMAX + 1 of a dead one"""
    xyz = np.asarray(xyz)
    assert xyz.dtype in (np.float64, np.float32)
    inside, c, _ = PR.locate(xyz.astype(np.float64), h, N, axes)  # (a float32 widens exactly)
    nb = blocks(N, shift)
    b = c >> shift
    K = np.where(inside, (b[0] * nb + b[1]) * nb + b[2], nb ** 3).astype(np.int64)
    if fate is not None:
        K = np.where(np.asarray(fate) != 0, nb ** 3 + 1, K)
    return K


def sort(xyz, fate, h, N, axes, shift=0):
    """(perm (M,) int32, counts (2,) int64): the stable argsort of the keys; the particles inside, the lost"""
    K = keys(xyz, fate, h, N, axes, shift)
    top = kmax(N, shift)
    perm = np.argsort(K, kind="stable").astype(np.int32)
    return perm, np.array([np.count_nonzero(K < top), np.count_nonzero(K == top)], dtype=np.int64)


def permute(perm, *arrays):
    return tuple(np.asarray(a)[perm] for a in arrays)


# ----------------------------------------------------------------------------------------------------------- test cases
# N: (c, L); a periodic axis needs an even c - 1: 37 = 18 * 2 + 1 there, and 161 and 321 (c = 6) take no periodic set
SIZES = {5: (5, 1), 17: (5, 3), 33: (5, 4), 37: (19, 2), 65: (5, 5), 161: (6, 6), 321: (6, 7)}
SMALL_COUNTS = (1, 255, 256, 257, 4099)
LARGE_COUNTS = (2048 * 256 + 259, (1 << 21) + 3)  # past the grid cap of the point kernels; past 1024 tiles (one scan chunk)
FAR = 4096  # ties this far apart lie in different tiles whatever the tile length up to 4096


def boundary_sets(N):
    if N == 37:
        return ("per7", "per4_f15")
    return tuple(bc for bc, (axes, _) in QR.BCS.items() if not axes or N in (5, 17, 65))


SMALL_CASES = [(N, bc) for N in (5, 17, 37, 65, 161, 321) for bc in boundary_sets(N)]
LARGE_CASES = [(5, "dirichlet"), (17, "per7"), (37, "per4_f15"), (65, "f63"), (161, "f22"), (321, "f25")]


def spacing(N, grid_length=1.0):
    return QR.spacing(N, grid_length)


@functools.lru_cache(maxsize=4)
def _particles(N, bc, count, grid_length=1.0, nodes=False):
    axes, _ = QR.BCS[bc]
    h = spacing(N, grid_length)
    length = (N - 1) * h
    rng = np.random.default_rng(100003 * N + 17 * count + axes)
    edge = PR.edge_points(N, h, axes) if count > 1 else np.zeros((0, 3))
    if nodes and count > 1:
        edge = np.concatenate([edge, PR.node_points_all(N, h)])
    xyz = np.concatenate([edge, PR.box_points(N, h, count, 11 * N + count)])[:count]
    fresh = np.arange(count) >= edge.shape[0]
    for ax in range(3):
        pick = fresh & (rng.uniform(size=count) < 0.1) & (count > 1)
        if axes >> ax & 1:  # periods away: the locator wraps them back inside
            xyz[pick, ax] += rng.integers(1, 4, count)[pick] * rng.choice([-1.0, 1.0], count)[pick] * length
        else:  # beyond a face: lost
            xyz[pick, ax] = np.where(rng.uniform(size=count) < 0.5, -0.3, 1.2)[pick] * length
    fate = np.where(rng.uniform(size=count) < 0.12,
                    rng.choice([3, 200, QR.FACE, QR.FACE + 5, QR.INVALID], count), 0).astype(np.int32)
    if count > 3 * FAR:  # one cell held by three living particles in three tiles
        where = [edge.shape[0], count // 2, count - 1]
        xyz[where] = (0.4 * length, 0.6 * length, 0.2 * length)
        fate[where] = 0
    if count == 1:
        fate[:] = 0
    xyz.setflags(write=False)
    fate.setflags(write=False)
    return xyz, fate


def particles(N, bc, count, grid_length=1.0, nodes=False):
    """(xyz (count, 3) float64, fate (count,) int32) of a case, read only: the edge points of the sample's tests first (a
    count of 1: one seeded point; nodes: PR.node_points_all behind them), seeded points inside, a tenth per axis moved whole
    periods away on a periodic axis and beyond a face on another, an eighth dead with the fates a push gives; past 3 * FAR
    particles one cell is held by three living particles at both ends and in the middle.  On a box of side grid_length"""
    return _particles(N, bc, count, grid_length, nodes)


def classes(K, top):
    """how many particles are inside, lost, dead"""
    return int(np.count_nonzero(K < top)), int(np.count_nonzero(K == top)), int(np.count_nonzero(K > top))


def far_ties(K, top):
    """whether some cell key is held by three particles whose old indices are more than FAR apart from one another"""
    order = np.argsort(K, kind="stable")
    Ks = K[order]
    starts = np.flatnonzero(np.r_[True, Ks[1:] != Ks[:-1]])
    ends = np.r_[starts[1:], Ks.size]
    for g in np.flatnonzero((ends - starts >= 3) & (Ks[starts] < top)):
        idx = order[starts[g]:ends[g]]  # ascending: the sort is stable
        lo = np.searchsorted(idx, idx[0] + FAR, side="right")
        if lo < idx.size and idx[lo] + FAR < idx[-1]:
            return True
    return False
