"""The restatement of the zero map's contract (tests/_dzero_ref.py) on inputs whose answer is known by construction: what
tests/test_gpu_dzero.py then holds the scan kernel's plane count to.  No GPU."""
import numpy as np

from _dzero_ref import interior_zero_planes


def _interior(N):
    return np.arange(N)[1:-1]


def test_all_plus_zero_is_every_interior_plane_and_never_a_boundary_plane():
    for N in (3, 5, 9, 33):
        z = interior_zero_planes(np.zeros((N, N, N)))
        assert not z[0] and not z[-1] and z[1:-1].all() and z.sum() == N - 2
    assert interior_zero_planes(np.zeros((2, 2, 2))).sum() == 0  # no interior at all


def test_faces_only_content_leaves_every_interior_plane_zero():
    N = 9
    d = np.zeros((N, N, N))
    rng = np.random.default_rng(1)
    for sl in ((0,), (-1,), (slice(None), 0), (slice(None), -1), (slice(None), slice(None), 0), (slice(None), slice(None), -1)):
        d[sl] = rng.uniform(1, 2, d[sl].shape)
    assert (d != 0).sum() == N ** 3 - (N - 2) ** 3
    assert interior_zero_planes(d).sum() == N - 2


def test_minus_zero_a_denormal_and_a_nan_each_make_their_plane_non_zero():
    N = 9
    for value in (-0.0, 5e-324, -5e-324, np.nan, 1.0):
        for i0 in (1, 4, N - 2):
            d = np.zeros((N, N, N))
            d[i0, 3, N - 2] = value
            z = interior_zero_planes(d)
            assert not z[i0], (value, i0)
            assert z.sum() == N - 3 and all(z[i] for i in _interior(N) if i != i0)


def test_a_value_on_a_face_of_an_interior_plane_does_not_count():
    N = 9
    for j, k in ((0, 4), (N - 1, 4), (4, 0), (4, N - 1), (0, 0)):
        d = np.zeros((N, N, N))
        d[4, j, k] = -0.0
        d[5, j, k] = 3.0
        assert interior_zero_planes(d).sum() == N - 2
    d = np.zeros((N, N, N))
    d[0, 4, 4] = d[N - 1, 4, 4] = 1.0  # interior points of the two boundary planes: those planes never count anyway
    assert interior_zero_planes(d).sum() == N - 2


def test_dense_content_is_no_plane():
    N = 9
    d = np.random.default_rng(2).uniform(-1, 1, (N, N, N))
    assert interior_zero_planes(d).sum() == 0
