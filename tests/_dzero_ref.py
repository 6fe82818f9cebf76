"""The contract of the zero map of a right-hand side (csrc/mg3d_kernels.hip, k_dzero_scan), restated in numpy: plane i of an
(N, N, N) field is "interior-zero" when every interior point (1 <= j, k <= N - 2) has the BIT PATTERN of +0.0 -- -0.0, a
denormal and a NaN all make it non-zero, the faces are not looked at --, and planes 0 and N - 1 never are."""
import numpy as np


def interior_zero_planes(d):
    """boolean array of length N: which planes i = const of the (N, N, N) float64 array d the map holds"""
    d = np.ascontiguousarray(d, dtype=np.float64)
    N = d.shape[0]
    assert d.shape == (N, N, N)
    out = np.zeros(N, dtype=bool)
    if N >= 3:
        bits = d.view(np.uint64)[1:-1, 1:-1, 1:-1]
        out[1:-1] = np.bitwise_or.reduce(bits.reshape(N - 2, -1), axis=1) == 0
    return out
