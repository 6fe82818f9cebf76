"""The CPU restatement of mg3d_wpcg_solve (tests/_wpcg_ref.py) checked on its own, without a GPU: the reflected operator
and the cycle are self-adjoint in the weighted inner product, every case of its table converges without breakdown, and
the launch geometry of the library's new reductions, restated from MG3D_MAX_PARTIALS, reaches the shapes the GPU tests
count on, and one term lost from a dot moves the iterate far beyond what tests/test_gpu_cg_shapes.py allows the GPU."""
import os
import re

import numpy as np
import pytest

import _coef_ref as CR
import _oracle as O
import _wpcg_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (periodic axes, Neumann faces) on 17^3 (c = 5, L = 3)
SYMMETRY = [(0, 1), (0, 37), (0, 63), (4, 15), (7, 0)]


@pytest.mark.parametrize("axes,faces", SYMMETRY)
@pytest.mark.parametrize("eps", [None, "ball"])
@pytest.mark.parametrize("op", ["A", "cycle"])
def test_self_adjoint_in_the_weighted_inner_product(axes, faces, eps, op):
    """|<x, B y>_w - <B x, y>_w| <= 1e-12 |<x, B y>_w| for B = A and B = the V(2,2) cycle from a zero guess; sigma = 0, so
    faces 63, axes 4 + faces 15 and axes 7 are the singular case: there x, y and B's result are taken on the subspace of
    w-mean zero, where the pinned coarse solve differs from a symmetric one by a constant.  Measured: <= 6e-15."""
    e = None if eps is None else CR.ball_eps(17, 100.)
    prob = WR.make_problem(5, 3, 2, 0.0, e, axes, faces)
    asym = WR.w_asymmetry(prob, WR.apply_blk if op == "A" else WR.cycle_blk, seed=axes * 64 + faces)
    print(axes, faces, eps, op, asym)
    assert asym <= 1e-12


@pytest.mark.parametrize("name", sorted(WR.CASES))
def test_every_case_converges_without_breakdown(name):
    """random guess, d = 0, to rtol 1e-10: converged (a breakdown returns unconverged), the norms end below the target, the
    true residual of the iterate -- projected in the singular case -- agrees with the recurrence's to 1e-6, and in the
    singular case the w-mean of x is that of the guess"""
    N, _, prob = WR.case_problem(name)
    x0 = WR.random_guess(N, prob.axes, prob.faces)
    d = np.zeros((N, N, N))
    x, norms, converged, rhs_mean = WR.wpcg(prob, x0, d, 1e-10, 0.0, 60)
    true = WR.true_residual_norm(prob, x, d)
    print(name, len(norms) - 1, norms[-1] / norms[0], abs(true - norms[-1]) / true)
    assert converged and norms[-1] <= 1e-10 * norms[0] and len(norms) - 1 <= 25
    assert abs(true - norms[-1]) <= 1e-6 * true and rhs_mean == 0.
    assert np.isfinite(x).all()
    unknown = WR.NR.unknown_mask(N, prob.axes, prob.faces) | WR.NR.is_dup(N, prob.axes)
    assert np.array_equal(x[~unknown], x0[~unknown])  # Dirichlet points
    if WR.singular(prob):
        assert abs(WR.wmean(prob, x) - WR.wmean(prob, x0)) <= 1e-14


# ------------------------------------------------------------------------------------------------------ launch geometry
def _max_partials():
    text = open(os.path.join(ROOT, "multigrid_parallel_amd", "csrc", "mg3d_internal.h")).read()
    return int(re.search(r"#define\s+MG3D_MAX_PARTIALS\s+(\d+)", text).group(1))


def pair_grid(N, axes, faces, cap=None, chunk=None):
    """pair_grid() of csrc/mg3d_kernels.hip with per-axis [lo, hi]: (gx, gy, gz, chunk, planes, pairs); cap: the whole array
    of partial sums for update + norm, half of it for the dot, which fills two runs; chunk given: the grid at that many
    planes per block, whatever the cap"""
    cap = _max_partials() if cap is None else cap
    lo, hi = zip(*(WR.NR.lo_hi(N, axes, faces, ax) for ax in range(3)))
    pairs, rows, planes = hi[2] // 2 + 1, hi[1] + 1 - lo[1], hi[0] + 1 - lo[0]
    gx, gy = -(-pairs // 64), -(-rows // 4)
    if chunk is None:
        chunk = 1
        while gx * gy * -(-planes // chunk) > cap:
            chunk *= 2
    return gx, gy, -(-planes // chunk), chunk, planes, pairs


def test_launch_geometry_of_the_new_reductions():
    """MG3D_MAX_PARTIALS = 32768.  513^3 with all six faces Neumann: 513 planes, 513 rows, 257 pairs -- one plane per block
    would take 339606 blocks; update + norm grows the chunk to 16 planes, the dot (two runs of half the cap) to 32, and
    both end in a last chunk of ONE plane.  Every case of the table stays at one plane per block under either cap.  37^3
    with khi Neumann has 19 pairs, the last one (36, 37) with one live member: a k tail of 19 of 64 lanes."""
    cap = _max_partials()
    assert cap == 32768 and O.level_sizes(9, 7)[-1] == 513
    gx, gy, gz, _, planes, pairs = pair_grid(513, 0, 63, chunk=1)
    assert (gx, gy, gz, planes, pairs) == (5, 129, 513, 513, 257) and gx * gy * gz > cap
    gx, gy, gz, chunk, planes, _ = pair_grid(513, 0, 63)
    assert chunk == 16 and gx * gy * gz <= cap and planes - (gz - 1) * chunk == 1
    gx, gy, gz, chunk, planes, _ = pair_grid(513, 0, 63, cap=cap // 2)
    assert chunk == 32 and gx * gy * gz <= cap // 2 and planes - (gz - 1) * chunk == 1
    for name, (c, L, _, _, axes, faces) in WR.CASES.items():
        N = O.level_sizes(c, L)[-1]
        assert pair_grid(N, axes, faces)[3] == 1 and pair_grid(N, axes, faces, cap=cap // 2)[3] == 1, name
    assert pair_grid(37, 0, 32)[5] == 19 and pair_grid(37, 0, 32)[0] == 1
    assert pair_grid(37, 0, 0)[5] == 18  # without the face: the walk of mg3d_pcg_solve
    # the pair (N-1, N) of a Neumann high k face stays inside the row: rows are padded to a multiple of 16 doubles
    for c, L, _, _, axes, faces in list(WR.CASES.values()) + [(9, 7, 0, None, 0, 63)]:
        N = O.level_sizes(c, L)[-1]
        assert N % 2 == 1 and ((N + 15) & ~15) >= N + 1


# ------------------------------------------------------------------------------------------------------------ sharpness
def test_one_lost_term_of_a_dot_moves_the_iterate(monkeypatch):
    """129^3 (c = 5, L = 6), all six faces Neumann, constant operator, random guess, d = 0, one iteration of the restatement
    alone: with the term of the single last unknown (128, 128, 128) -- the one live lane of the second k-block, the last
    row, the last plane -- left out of r.z, and separately out of p.Ap, x_1 moves by at least 1000 times what
    tests/test_gpu_cg_shapes.py allows the GPU at k = 1 (measured: 5.7e-7 either way): one lost lane, row or plane
    cannot hide under that margin.  The three runs share one cycle, z = V(r_0) is the same in all of them, and take
    numpy's sums: what a summation order is worth is nine orders below the effect."""
    from test_gpu_cg_shapes import tolerances
    N = 129
    prob = WR.make_problem(5, 6, 2, 0.0, None, 0, 63)
    x0, d = WR.random_guess(N, 0, 63), np.zeros((N, N, N))
    z = []

    def cycle(p, r_blk):
        if not z:
            z.append(WR.precondition(p, r_blk))
        return z[0].copy()

    real = WR.wdot

    def x1(drop):
        """drop: which weighted dot of the iteration loses the term (1: r.z, 2: p.Ap), or None"""
        calls = [0]

        def wdot(w, a, b, dots="exact"):
            calls[0] += 1
            if calls[0] == drop:
                a = a.copy()
                a[-1, -1, -1] = 0.  # (the product is then an exact zero: the term is gone from the sum)
            return real(w, a, b, dots)

        monkeypatch.setattr(WR, "wdot", wdot)
        hist = []
        WR.wpcg(prob, x0, d, 0., 1e-300, 1, "plain", hist, cycle)
        assert calls[0] == 2
        return hist[0]

    base = x1(None)
    tol = tolerances("wpcg", 1)[0]
    for drop, what in ((1, "r.z"), (2, "p.Ap")):
        moved = np.abs(x1(drop) - base).max() / np.abs(base).max()
        print(what, "moved x_1 by", moved, "; allowed on the GPU:", tol)
        assert moved >= 1000 * tol, (what, moved, tol)
