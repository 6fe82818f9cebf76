"""The pair-walk passes of csrc/mg3d_kernels.hip -- pcg_update, pcg_dot, pcg_direction, wpcg_dot, wpcg_direction,
wpcg_center -- past one 64-lane block in k and past the cap of partial sums, through mg3d_pcg_solve and mg3d_wpcg_solve
(step_rhs_be_kernel, the seventh, has its cases in tests/test_gpu_step.py).  tests/test_gpu_pcg.py and test_gpu_wpcg.py
hold the iterates to a reference only where pair_grid() gives one k-block and one plane per block; their 513^3 tests
compare r_norm with the true residual of the returned u, an identity that holds for any alpha and any direction, so a dot
or direction pass that drops a k-block, a lane or the short last chunk would pass them.

The reference.  The CPU restatements (tests/_pcg_ref.py, _wpcg_ref.py) cost a numpy V-cycle per iteration, too much at
these sizes.  The preconditioner of a solve is the context's own cycle from u = 0 with right-hand side r, and the suite
pins that cycle to the restatement bit for bit; so a second context (the "twin": same c, L, nu, sigma, eps, periodic axes
and Neumann faces) supplies z = V(r) through the restatements' precondition= argument, and the residual, apply, every
sum, the projection, the direction and the update stay numpy.  test_hybrid_reference_is_the_restatement anchors this: at
129^3 the hybrid run and the pure restatement give the same bits.

Tolerances.  As in the two files above: two reference runs, exactly rounded sums against numpy's pairwise float64 sums,
differ in the iterate x_k as max|a - b| / max|a| by the figures below, and the GPU, a third summation order, is allowed
100 times the figure.  The reference needs the twin, so the table was measured on an MI355X (hybrid runs of both kinds,
from random_guess with d = 0):
                              k = 1       k = 2       k = 3       norms       w-mean drift / max|x_0|
    w129_f63                  3.63e-15    2.79e-12    4.37e-11    1.07e-14    1.87e-17
    w129_f32_ball             6.08e-15    2.94e-13    1.01e-12    3.27e-14
    w145_f25_ball             5.19e-15    1.38e-13    6.42e-13    1.64e-14
    p145_ball                 0.0         5.01e-16    2.36e-15    1.15e-15
    p161_per7_sigma50         2.00e-14    2.50e-13    4.04e-12    2.67e-14
    w257_f63                  1.81e-14    1.90e-11                3.68e-14    1.59e-17
    p289                      1.14e-14    3.56e-13                2.89e-14
    the largest               2.00e-14    1.90e-11    4.37e-11    3.68e-14    1.87e-17
A case's own spread can come out as zero, so for each k the figure is the largest over the seven cases, and never less
than the figure the existing file of the same call holds on the GPU with (test_gpu_pcg.SPREAD_U / SPREAD_NORM,
test_gpu_wpcg.SPREAD_U / SPREAD_NORM / DRIFT; they have no k = 3: their k = 2 figure, the smaller one, is the floor
there)."""
import time

import numpy as np
import pytest

import _coef_ref as CR
import _neumann_ref as NR
import _oracle as O
import _pcg_ref as PR
import _wpcg_ref as WR
import multigrid_parallel_amd as M
import test_gpu_pcg as TP
import test_gpu_wpcg as TW
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U
from test_wpcg_ref_host import _max_partials, pair_grid

gpu = pytest.mark.gpu

_ball = lambda N: CR.ball_eps(N, 100.)
# name: (call, c, L, sigma, eps of the finest level from N or None, periodic axes, Neumann faces, iterations)
CASES = {
    # 65 k-pairs: two k-blocks, ONE live lane in the second (the pair (128, 129), one live member); 129 rows: a last
    # j-block of one row; singular: the centre pass and the projection in the direction pass
    "w129_f63": ("wpcg", 5, 6, 0.0, None, 0, 63, 3),
    # the same 65 pairs from the high k face alone, 127 rows and planes, not singular, the COEF apply
    "w129_f32_ball": ("wpcg", 5, 6, 0.0, _ball, 0, 32, 3),
    # off the 2^k+1 ladder: 72 pairs (8 live lanes in the second k-block), lo/hi mixed per axis: ilo + jhi + klo
    "w145_f25_ball": ("wpcg", 10, 5, 0.0, _ball, 0, 0b011001, 3),
    # the unweighted passes: 72 pairs, 143 rows: a last j-block of 3 rows
    "p145_ball": ("pcg", 10, 5, 0.0, _ball, 0, 0, 3),
    # lo = 0 on every axis: 80 pairs, 160 rows and planes
    "p161_per7_sigma50": ("pcg", 11, 5, 50.0, None, 7, 0, 3),
    # past the cap: 129 pairs: THREE k-blocks, one live lane in the third; update, centre and direction at 2 planes per
    # block and the two-sum dot (half the cap) at 4, each with a last chunk of ONE plane
    "w257_f63": ("wpcg", 9, 6, 0.0, None, 0, 63, 2),
    # the first Dirichlet size past the cap: 144 pairs: three k-blocks (16 live lanes); dot, direction and update at 2
    # planes per block with a last chunk of one plane
    "p289": ("pcg", 10, 6, 0.0, None, 0, 0, 2),
}
# what pair_grid() gives: (pairs, k-blocks, live lanes of the last, rows, rows of the last j-block, planes, chunk under
# the whole cap, planes of its last chunk, chunk under half the cap, planes of its last chunk)
SHAPES = {
    "w129_f63": (65, 2, 1, 129, 1, 129, 1, 1, 1, 1),
    "w129_f32_ball": (65, 2, 1, 127, 3, 127, 1, 1, 1, 1),
    "w145_f25_ball": (72, 2, 8, 144, 4, 144, 1, 1, 1, 1),
    "p145_ball": (72, 2, 8, 143, 3, 143, 1, 1, 1, 1),
    "p161_per7_sigma50": (80, 2, 16, 160, 4, 160, 1, 1, 1, 1),
    "w257_f63": (129, 3, 1, 257, 1, 257, 2, 1, 4, 1),
    "p289": (144, 3, 16, 287, 3, 287, 2, 1, 4, 3),  # (mg3d_pcg_solve's dot takes the whole cap)
}

# measured, see above: the largest figure over the seven cases
SPREAD_U = {1: 2.00e-14, 2: 1.90e-11, 3: 4.37e-11}
SPREAD_NORM = 3.68e-14
SPREAD_DRIFT = 1.87e-17  # of the w-mean, relative to max|x_0|


def _floor(call):
    """the figures the existing file of the same call holds on the GPU with: (u per k, norms)"""
    f = TW if call == "wpcg" else TP
    return {1: f.SPREAD_U[1], 2: f.SPREAD_U[2], 3: f.SPREAD_U[2]}, f.SPREAD_NORM


def tolerances(call, k):
    """(u, norms, w-mean drift) allowed on the GPU after k iterations"""
    fu, fn = _floor(call)
    return 100 * max(SPREAD_U[k], fu[k]), 100 * max(SPREAD_NORM, fn), 100 * max(SPREAD_DRIFT, TW.DRIFT)


def _same_bits(a, b):
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _size(name):
    return O.level_sizes(CASES[name][1], CASES[name][2])[-1]


# -------------------------------------------------------------------------------------------- the shapes, without a GPU
def test_the_cases_reach_the_shapes():
    """pair_grid() restated from MG3D_MAX_PARTIALS of the header (tests/test_wpcg_ref_host.py): every case reaches what its
    comment says -- if the cap or the grid changes this fails and the cases cannot silently move -- and the two past the
    cap are the smallest that are: 257^3 with Dirichlet faces (32640 blocks) and with three periodic axes (exactly the
    cap) stay at one plane per block"""
    cap = _max_partials()
    assert cap == 32768
    for name, (call, c, L, _, _, axes, faces, _) in CASES.items():
        N = _size(name)
        lo, hi = NR.lo_hi(N, axes, faces, 1)
        gx, gy, gz, chunk, planes, pairs = pair_grid(N, axes, faces)
        _, _, hz, half, _, _ = pair_grid(N, axes, faces, cap=cap // 2)
        got = (pairs, gx, pairs - (gx - 1) * 64, hi + 1 - lo, hi + 1 - lo - (gy - 1) * 4, planes, chunk,
               planes - (gz - 1) * chunk, half, planes - (hz - 1) * half)
        assert got == SHAPES[name], (name, got)
        assert gx >= 2 and gx * gy * gz <= cap and gx * gy * hz <= cap // 2
    assert [_size(n) for n in CASES] == [129, 129, 145, 145, 161, 257, 289]
    for axes, blocks in ((0, 32640), (7, 32768)):
        gx, gy, gz, chunk, _, _ = pair_grid(257, axes, 0)
        assert chunk == 1 and gx * gy * gz == blocks
    assert pair_grid(257, 0, 63, chunk=1)[:3] == (3, 65, 257) and 3 * 65 * 257 > cap


# ------------------------------------------------------------------------------------------------- the hybrid reference
class _Op:
    """what the restatements read of a problem when the cycle comes from elsewhere: the finest level's operator"""

    def __init__(self, N, sigma, eps, axes, faces):
        self.N, self.h, self.sigma, self.axes, self.faces = [N], 1.0 / (N - 1), sigma, axes, faces
        self.eps = None if eps is None else [eps]
        self.r = []


def _solver(name):
    _, c, L, sigma, field, axes, faces, _ = CASES[name]
    s = M.Solver(c, L, 2)
    s.set_shift(sigma)
    s.set_periodic(axes)
    s.set_neumann(faces)
    if field is not None:
        s.set_coefficient(field(_size(name)))
    s.get_details()
    return s


class _Twin:
    """a second context of the case; precondition(prob, r_blk) is its V-cycle from u = 0 with right-hand side r"""

    def __init__(self, name):
        self.s, self.q = _solver(name), CASES[name][2] - 1
        for l in range(self.q + 1):  # as the solve leaves them before its first cycle
            self.s.zero(MG3D_R, l)

    def precondition(self, prob, r_blk):
        N = prob.N[-1]
        d = np.zeros((N, N, N))
        d[NR.block(N, prob.axes, prob.faces)] = r_blk
        self.s.zero(MG3D_U, self.q)
        self.s.upload(MG3D_D, self.q, d)
        self.s.vcycle(want_norm=False)
        return self.s.download(MG3D_U, self.q).reshape(N, N, N)


def _operator(name):
    _, _, _, sigma, field, axes, faces, _ = CASES[name]
    N = _size(name)
    assert field is None or not axes
    return _Op(N, sigma, None if field is None else field(N), axes, faces)


def _guess(name):
    call, _, _, _, _, axes, faces, _ = CASES[name]
    N = _size(name)
    return WR.random_guess(N, axes, faces) if call == "wpcg" else PR.random_guess(N, axes)


def hybrid_run(name, dots="exact"):
    """the restatement of the case's call from random_guess with d = 0, its cycles from the twin:
    (x0, iterates x_1 .. x_k, norms r_0 .. r_k, converged)"""
    call, kmax = CASES[name][0], CASES[name][7]
    prob, x0 = _operator(name), _guess(name)
    d = np.zeros_like(x0)
    hist = []
    twin = _Twin(name)
    with twin.s:
        if call == "wpcg":
            _, norms, converged, rhs_mean = WR.wpcg(prob, x0, d, 0., 1e-300, kmax, dots, hist, twin.precondition)
            assert rhs_mean == 0.
        else:
            _, norms, converged = PR.pcg(prob, x0, d, 0., 1e-300, kmax, dots, hist, twin.precondition)
    assert len(hist) == kmax and len(norms) == kmax + 1
    return x0, hist, norms, converged


_last = {}  # the reference of one case: the large arrays of the one before are freed


def _reference(name):
    if name not in _last:
        _last.clear()
        _last[name] = hybrid_run(name)
    return _last[name]


@gpu
def test_hybrid_reference_is_the_restatement():
    """129^3 (c = 5, L = 6), all six faces Neumann, constant operator, random_guess, d = 0, exactly rounded sums: x_1, x_2
    and the norms of the hybrid run are those of the pure restatement bit for bit -- the same sums in the same order, so
    any difference would mean that the twin's cycle is not the cycle the restatement states"""
    name = "w129_f63"
    call, c, L, sigma, _, axes, faces, _ = CASES[name]
    x0, hist, norms, converged = _reference(name)
    prob = WR.make_problem(c, L, 2, sigma, None, axes, faces)
    pure = []
    _, pure_norms, pure_converged, _ = WR.wpcg(prob, x0, np.zeros_like(x0), 0., 1e-300, 2, "exact", pure)
    assert len(pure) == 2 and not pure_converged and not converged
    for k in (0, 1):
        assert _same_bits(hist[k], pure[k]), k + 1
    assert np.array_equal(norms[:3], pure_norms)


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_iterates_agree_with_the_hybrid_reference(name):
    """u after k = 1, 2(, 3) iterations against x_k, the norms r_0 .. r_k, info, the periodic duplicates, in the singular
    cases the w-mean of u, and an independent residual of the last u against r_norm.  Three iterations put two direction
    passes with beta != 0 behind the first one; random_guess is asymmetric data, so an index slip cannot hide"""
    t0 = time.perf_counter()
    call, _, L, _, _, axes, faces, kmax = CASES[name]
    x0, hist, ref_norms, ref_converged = _reference(name)
    t1 = time.perf_counter()
    prob = _operator(name)
    sing = call == "wpcg" and WR.singular(prob)
    q = L - 1
    with _solver(name) as s:
        for k in range(1, kmax + 1):
            s.upload(MG3D_U, q, x0)
            norms, info = getattr(s, call + "_solve")(rtol=0.0, atol=1e-300, max_iters=k)
            assert info["iterations"] == k and len(norms) == k + 1 and info["converged"] == ref_converged is False
            if call == "wpcg":
                assert info["singular"] == sing and info["rhs_mean"] == 0.
            u = s.download(MG3D_U, q).reshape(x0.shape)
            want = hist[k - 1]
            rel = np.abs(u - want).max() / np.abs(want).max()
            nrel = (np.abs(norms - ref_norms[:k + 1]) / ref_norms[:k + 1]).max()
            tol_u, tol_n, tol_d = tolerances(call, k)
            print(name, k, "u", rel, "of", tol_u, "norms", nrel, "of", tol_n)
            assert rel <= tol_u, (name, k, rel)
            assert nrel <= tol_n, (name, k, nrel)
            assert info["r_norm"] == norms[-1] and info["r0_norm"] == norms[0]
            if axes:
                w = u.copy()
                NR.refresh(w, axes)
                assert _same_bits(u, w), "duplicates differ from their sources"
            if sing:
                drift = abs(WR.wmean(prob, u) - WR.wmean(prob, x0)) / np.abs(x0).max()
                print(name, k, "w-mean drift", drift, "of", tol_d)
                assert drift <= tol_d, (name, k, drift)
        res = s.residual(q, store=False)
        print(name, "r_norm", info["r_norm"], "residual", res, abs(info["r_norm"] - res) / res)
        assert abs(info["r_norm"] - res) <= 1e-6 * res
    print(name, "reference %.1f s, GPU and checks %.1f s" % (t1 - t0, time.perf_counter() - t1))
