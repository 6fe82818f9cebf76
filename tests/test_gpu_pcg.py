"""mg3d_pcg_solve on the GPU against the CPU restatement of tests/_pcg_ref.py (cases and data: its CASES table and
random_guess, d = 0): robustness on jumping coefficients, agreement of the iterates, the true residual, the state the
solve leaves, periodic axes, refusals, and the launch shapes off the 2^k+1 ladder and past the cap of partial sums.

The cycles of the restatement are the library's bit for bit; only the dots differ, in summation order.  What a summation
order is worth was measured on the CPU (python tests/_pcg_ref.py): two restatement runs, exactly rounded dots against
numpy's pairwise float64 sums, differ in the iterate x_k, as max|a - b| / max|a| and largest over the nine cases, by
    k = 1: 7.58e-15      k = 2: 8.18e-14      k = 5: 1.32e-10      (norms, any k <= 5: 1.80e-14)
(d = 0, so x_k itself shrinks by about ten per iteration and a difference of fixed size grows relative to it).  The GPU,
a third summation order, is allowed 100 times the figure of the same k -- for every k at most 100 times the largest one."""
import os
import re

import numpy as np
import pytest

import _oracle as O
import _pcg_ref as PR
import _periodic_ref as P
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U

gpu = pytest.mark.gpu

MG3D_ERR_ARG, MG3D_ERR_STATE = 1, 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPREAD_U = {1: 7.58e-15, 2: 8.18e-14, 5: 1.32e-10}  # measured, see above
SPREAD_NORM = 1.80e-14
JUMPS = ["ball100", "ball0.01", "slab1e4"]
AGREE = JUMPS + ["constant", "sigma100", "per6_smooth", "per7_sigma50", "37_ball100", "25_per2_smooth"]


def _same_bits(a, b):
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _solver(name, build=True):
    c, L, sigma, _, axes = PR.CASES[name]
    N, eps, _ = PR.case_problem(name)
    s = M.Solver(c, L, 2)
    s.set_shift(sigma)
    s.set_periodic(axes)
    if eps is not None:
        s.set_coefficient(eps)
    if build:
        s.get_details()
    return s


_ref_runs = {}


def _restatement(name):
    """the restatement's run to rtol 1e-10 from random_guess with d = 0, computed once: (x0, iterates x_1.., norms)"""
    if name not in _ref_runs:
        N, _, prob = PR.case_problem(name)
        x0 = PR.random_guess(N, PR.CASES[name][4])
        hist = []
        _, norms, converged = PR.pcg(prob, x0, np.zeros((N, N, N)), 1e-10, 0.0, 60, history=hist)
        assert converged and len(hist) >= 5
        _ref_runs[name] = (x0, hist, norms)
    return _ref_runs[name]


def _top(name):
    return PR.CASES[name][1] - 1


# ------------------------------------------------------------------------------------------------------ 1 robustness
@gpu
@pytest.mark.parametrize("name", JUMPS)
def test_robust_on_jumps(name):
    """33^3, random guess, d = 0, rtol 1e-10: converged, in at most the restatement's count + 1 iterations (a norm may land
    on either side of the threshold under another summation order), and in fewer iterations than the same context needs
    plain V-cycles for the same reduction"""
    x0, hist, ref_norms = _restatement(name)
    q = _top(name)
    with _solver(name) as s:
        s.upload(MG3D_U, q, x0)
        norms, info = s.pcg_solve(rtol=1e-10, max_iters=60)
        s.upload(MG3D_U, q, x0)
        r0 = s.residual(q, store=False)
        cyc = s.vcycles(60)
    below = np.nonzero(cyc <= 1e-10 * r0)[0]
    n_cycles = int(below[0]) + 1 if below.size else 61
    print(name, "pcg", info["iterations"], "restatement", len(ref_norms) - 1, "vcycles", n_cycles)
    assert info["converged"] and len(norms) == info["iterations"] + 1
    assert info["iterations"] <= len(ref_norms) - 1 + 1
    assert info["iterations"] < n_cycles


# ----------------------------------------------------------------------------------- 2 agreement with the restatement
@gpu
@pytest.mark.parametrize("name", AGREE)
def test_iterates_agree_with_the_restatement(name):
    """u after 1, 2 and 5 iterations against x_k, and the norms r_0 .. r_k: 100 x the measured summation spread"""
    x0, hist, ref_norms = _restatement(name)
    q, axes = _top(name), PR.CASES[name][4]
    with _solver(name) as s:
        for k in (1, 2, 5):
            s.upload(MG3D_U, q, x0)
            norms, info = s.pcg_solve(rtol=0.0, atol=1e-300, max_iters=k)
            assert info["iterations"] == k and not info["converged"] and len(norms) == k + 1
            u = s.download(MG3D_U, q).reshape(x0.shape)
            want = hist[k - 1]
            rel = np.abs(u - want).max() / np.abs(want).max()
            nrel = (np.abs(norms - ref_norms[:k + 1]) / ref_norms[:k + 1]).max()
            print(name, k, "u", rel, "norms", nrel)
            assert rel <= 100 * SPREAD_U[k], (name, k, rel)  # measured spread 7.58e-15 / 8.18e-14 / 1.32e-10
            assert nrel <= 100 * SPREAD_NORM, (name, k, nrel)  # measured spread 1.80e-14
            if axes:
                w = u.copy()
                P.refresh(w, axes)
                assert _same_bits(u, w), "duplicates differ from their sources"
            assert info["r_norm"] == norms[-1] and info["r0_norm"] == norms[0]


# ------------------------------------------------------------------------------------------------------ 3 true residual
@gpu
@pytest.mark.parametrize("name", AGREE)
def test_true_residual(name):
    """after pcg_solve(rtol = 1e-8) an independent residual of the returned u is <= 2 rtol r0_norm and agrees with the
    recurrence's r_norm to 1e-6 relative"""
    x0, _, _ = _restatement(name)
    q = _top(name)
    with _solver(name) as s:
        s.upload(MG3D_U, q, x0)
        norms, info = s.pcg_solve(rtol=1e-8)
        res = s.residual(q, store=False)
    print(name, info, res, abs(info["r_norm"] - res) / res)
    assert info["converged"] and info["r_norm"] <= 1e-8 * info["r0_norm"]
    assert res <= 2 * 1e-8 * info["r0_norm"]
    assert abs(info["r_norm"] - res) <= 1e-6 * res


# --------------------------------------------------------------------------------------------------------------- 4 state
def _faces(N):
    f = np.ones((N, N, N), dtype=bool)
    f[1:-1, 1:-1, 1:-1] = False
    return f


@gpu
@pytest.mark.parametrize("name", ["ball100", "constant"])
def test_state_after_the_solve(name):
    """random Dirichlet values and a random d: d and the faces of u come back bit for bit, a following vcycles(1) is the
    one of a fresh context with the returned u and d uploaded, max_iters = 0 changes nothing"""
    N, _, _ = PR.case_problem(name)
    q = _top(name)
    u0 = PR.random_guess(N, 0, seed=9, faces=True)
    d0 = np.random.default_rng(10).uniform(-1, 1, (N, N, N))
    with _solver(name) as s, _solver(name) as fresh:
        s.upload(MG3D_U, q, u0)
        s.upload(MG3D_D, q, d0)
        r0 = s.residual(q, store=False)
        norms, info = s.pcg_solve(rtol=0.0, atol=1e-300, max_iters=0)
        assert info["iterations"] == 0 and len(norms) == 1 and info["r0_norm"] == r0 == norms[0] and not info["converged"]
        assert _same_bits(s.download(MG3D_U, q), u0.reshape(-1)) and _same_bits(s.download(MG3D_D, q), d0.reshape(-1))
        norms, info = s.pcg_solve(rtol=1e-8)
        assert info["converged"] and info["r0_norm"] == r0
        u1 = s.download(MG3D_U, q)
        assert _same_bits(s.download(MG3D_D, q), d0.reshape(-1))
        assert _same_bits(u1.reshape(N, N, N)[_faces(N)], u0[_faces(N)])
        n_a = s.vcycles(1)
        fresh.upload(MG3D_U, q, u1)
        fresh.upload(MG3D_D, q, d0)
        n_b = fresh.vcycles(1)
        assert _same_bits(s.download(MG3D_U, q), fresh.download(MG3D_U, q)) and n_a[0] == n_b[0]
        # a second solve reuses the work vectors: the same bits as the first one from the same data
        s.upload(MG3D_U, q, u0)
        norms2, _ = s.pcg_solve(rtol=1e-8)
        assert np.array_equal(norms, norms2) and _same_bits(s.download(MG3D_U, q), u1)


@gpu
def test_a_cycle_that_ran_ahead_is_finished_first():
    """129^3 with carried cycles (carry_min = 66): behind a single vcycle, which ends ahead of itself, the solve starts
    from that cycle's own u -- the bits of a context that had it uploaded"""
    c, L = 9, 5
    N = 129
    rng = np.random.default_rng(2)
    u0, d0 = rng.uniform(-1, 1, (N, N, N)), rng.uniform(-1, 1, (N, N, N))
    with M.Solver(c, L, 2) as s, M.Solver(c, L, 2) as t:
        for x in (s, t):
            x.set_option("carry_min", 66)
            x.get_details()
            x.upload(MG3D_U, L - 1, u0)
            x.upload(MG3D_D, L - 1, d0)
        s.vcycle()
        na, ia = s.pcg_solve(rtol=1e-6, max_iters=4)
        t.vcycle()
        t.upload(MG3D_U, L - 1, t.download(MG3D_U, L - 1))
        nb, ib = t.pcg_solve(rtol=1e-6, max_iters=4)
        assert ia == ib and np.array_equal(na, nb) and ia["iterations"] >= 1
        assert _same_bits(s.download(MG3D_U, L - 1), t.download(MG3D_U, L - 1))
        assert _same_bits(s.download(MG3D_D, L - 1), d0.reshape(-1))


# ------------------------------------------------------------------------------------------------------------ 5 periodic
@gpu
@pytest.mark.parametrize("name", ["per6_smooth", "per7_sigma50"])
def test_periodic_converges(name):
    x0, _, ref_norms = _restatement(name)
    q, axes = _top(name), PR.CASES[name][4]
    with _solver(name) as s:
        s.upload(MG3D_U, q, x0)
        norms, info = s.pcg_solve(rtol=1e-10)
        u = s.download(MG3D_U, q).reshape(x0.shape)
    assert info["converged"] and norms[-1] <= 1e-10 * norms[0] and info["iterations"] <= len(ref_norms)
    w = u.copy()
    P.refresh(w, axes)
    assert _same_bits(u, w)


@gpu
def test_singular_periodic_case_is_refused():
    N = 33
    u0, d0 = PR.random_guess(N, 7, seed=3), np.random.default_rng(4).uniform(-1, 1, (N, N, N))
    P.refresh(d0, 7)
    with M.Solver(5, 4, 2) as s:
        s.set_periodic(7)
        s.get_details()
        s.upload(MG3D_U, 3, u0)
        s.upload(MG3D_D, 3, d0)
        with pytest.raises(M.Mg3dError) as e:
            s.pcg_solve()
        assert e.value.code == MG3D_ERR_STATE
        assert _same_bits(s.download(MG3D_U, 3), u0.reshape(-1)) and _same_bits(s.download(MG3D_D, 3), d0.reshape(-1))


# ---------------------------------------------------------------------------------------------- 6 refusals and arguments
@gpu
def test_refusals_and_arguments():
    N = 17
    rng = np.random.default_rng(6)
    u0, d0 = rng.uniform(-1, 1, N ** 3), rng.uniform(-1, 1, N ** 3)

    def refused(s, code, **kw):
        with pytest.raises(M.Mg3dError) as e:
            s.pcg_solve(**kw)
        assert e.value.code == code, (kw, e.value)
        assert _same_bits(s.download(MG3D_U, 2), u0) and _same_bits(s.download(MG3D_D, 2), d0)

    for faces in (1, 2, 12, 63):
        with M.Solver(5, 3, 2) as s:
            s.set_neumann(faces)
            s.get_details()
            s.upload(MG3D_U, 2, u0)
            s.upload(MG3D_D, 2, d0)
            refused(s, MG3D_ERR_STATE)
    with M.Solver(5, 3, 2) as s:  # no coarse factor
        s.upload(MG3D_U, 2, u0)
        s.upload(MG3D_D, 2, d0)
        refused(s, MG3D_ERR_STATE)
        s.get_details()
        refused(s, MG3D_ERR_ARG, rtol=-1e-8)
        refused(s, MG3D_ERR_ARG, rtol=float("nan"))
        refused(s, MG3D_ERR_ARG, atol=-1.0)
        refused(s, MG3D_ERR_ARG, atol=float("inf"))
        refused(s, MG3D_ERR_ARG, max_iters=-1)
        refused(s, MG3D_ERR_ARG, rtol=0.0, atol=0.0, max_iters=0)
        norms, info = s.pcg_solve()  # and the context is still good
        assert info["converged"]
    es = M.EsParams.default()
    with M.Solver(5, 3, 2, grid_length=es.length) as s:  # the mixed-boundary factor
        s.es_setup(es)
        with pytest.raises(M.Mg3dError) as e:
            s.pcg_solve()
        assert e.value.code == MG3D_ERR_STATE


# --------------------------------------------------------------------------------------------------------- 7 launch shapes
def _max_partials():
    text = open(os.path.join(ROOT, "multigrid_parallel_amd", "csrc", "mg3d_internal.h")).read()
    return int(re.search(r"#define\s+MG3D_MAX_PARTIALS\s+(\d+)", text).group(1))


def pair_grid(N, axes, chunk=None):
    """pair_grid() of csrc/mg3d_kernels.hip, the geometry of the update, dot and direction passes: (gx, gy, gz, chunk);
    chunk given: the grid at that many planes per block, whatever the cap"""
    lo = [0 if axes >> ax & 1 else 1 for ax in range(3)]
    pairs, rows, planes = (N - 2) // 2 + 1, N - 1 - lo[1], N - 1 - lo[0]
    gx, gy = -(-pairs // 64), -(-rows // 4)
    if chunk is None:
        chunk = 1
        while gx * gy * -(-planes // chunk) > _max_partials():
            chunk *= 2
    return gx, gy, -(-planes // chunk), chunk


def test_513_exercises_the_chunk_growth():
    """MG3D_MAX_PARTIALS = 32768: at 513^3 the unchunked grid of the new reductions -- one plane per block -- has 261632
    blocks, eight times the cap, and the launcher grows the chunk to 8 planes; the apply pass walks the residual's column
    grid, which 513^3 fills exactly (tests/test_gpu_stencil_shapes.py).  The small cases stay at one plane per block."""
    assert _max_partials() == 32768 and O.level_sizes(9, 7)[-1] == 513
    gx, gy, gz, _ = pair_grid(513, 0, chunk=1)
    assert (gx, gy, gz) == (4, 128, 511) and gx * gy * gz > _max_partials()
    gx, gy, gz, chunk = pair_grid(513, 0)
    assert chunk == 8 and gx * gy * gz <= _max_partials() and 511 - (gz - 1) * chunk == 7  # a short last chunk
    for name in AGREE:
        N = PR.case_problem(name)[0]
        assert pair_grid(N, PR.CASES[name][4])[3] == 1
    assert pair_grid(37, 0)[:2] == (1, 9) and (37 - 2) // 2 + 1 == 18  # 18 of 64 lanes: a k tail


@gpu
def test_past_the_cap_513():
    """513^3 (c = 9, L = 7), constant operator, smooth guess, three iterations: r_norm of the recurrence against an
    independent residual of the returned u, 1e-9 relative -- a dropped block of partial sums breaks it at once"""
    c, L, N = 9, 7, 513
    x = np.sin(np.pi * np.linspace(0.0, 1.0, N))
    y = np.sin(2 * np.pi * np.linspace(0.0, 1.0, N))
    u0 = np.ascontiguousarray(x[:, None, None] * y[None, :, None] * x[None, None, :])
    with M.Solver(c, L, 2) as s:
        s.get_details()
        s.upload(MG3D_U, L - 1, u0)
        del u0
        norms, info = s.pcg_solve(rtol=0.0, atol=1e-300, max_iters=3)
        res = s.residual(L - 1, store=False)
    print("513^3", norms, res, abs(info["r_norm"] - res) / res)
    assert info["iterations"] == 3 and norms[-1] < norms[0]
    assert abs(info["r_norm"] - res) <= 1e-9 * res
