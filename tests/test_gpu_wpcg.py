"""mg3d_wpcg_solve on the GPU against the CPU restatement of tests/_wpcg_ref.py (cases and data: its CASES table and
random_guess, V(2,2), d = 0 unless stated): every Neumann face on its own, combinations with periodic axes, sigma and eps,
the singular case and its projection, shapes off the 2^k+1 ladder, robustness where plain cycles grow, the true residual,
an incompatible right-hand side, the state the solve leaves, the bits of mg3d_pcg_solve where that call works, refusals,
and 513^3 past the cap of partial sums.

The cycles of the restatement are the library's bit for bit; only the sums differ, in summation order.  What a summation
order is worth was measured on the CPU (python tests/_wpcg_ref.py): two restatement runs, exactly rounded sums against
numpy's pairwise float64 sums, differ in the iterate x_k, as max|a - b| / max|a|, by at most
                                   k = 1       k = 2       k = 5       norms, any k <= 5
    f63_slab (jump 1e4, singular)  3.20e-11    1.08e-09    1.27e-08    1.51e-11
    the other thirteen cases       1.04e-13    4.10e-12    1.58e-10    9.60e-13
(the slab's dots cancel four digits more than any other case's, so it keeps its own figures), and in the singular cases
the w-mean of x_k leaves that of the guess by at most 2.26e-17 max|x_0| in either run.  The GPU, a third summation order,
is allowed 100 times the figure."""
import numpy as np
import pytest

import _neumann_ref as NR
import _pcg_ref as PR
import _wpcg_ref as WR
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U

gpu = pytest.mark.gpu

MG3D_ERR_ARG, MG3D_ERR_STATE = 1, 5
SPREAD_U = {1: 1.04e-13, 2: 4.10e-12, 5: 1.58e-10}  # measured, see above
SPREAD_NORM = 9.60e-13
SPREAD_U_SLAB = {1: 3.20e-11, 2: 1.08e-09, 5: 1.27e-08}
SPREAD_NORM_SLAB = 1.51e-11
DRIFT = 2.26e-17  # of the w-mean, relative to max|x_0|
FACES = ["17_f1", "17_f2", "17_f4", "17_f8", "17_f16", "17_f32"]
COMBINED = ["f63_ball", "f63_slab", "per4_f15_ball", "per7_ball", "f22_ball", "f63_sigma3"]
OFF_LADDER = ["37_f25", "25_per2_f51"]
ALL = FACES + COMBINED + OFF_LADDER


def _same_bits(a, b):
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _solver(name):
    c, L, sigma, _, axes, faces = WR.CASES[name]
    _, eps, _ = WR.case_problem(name)
    s = M.Solver(c, L, 2)
    s.set_shift(sigma)
    s.set_periodic(axes)
    s.set_neumann(faces)
    if eps is not None:
        s.set_coefficient(eps)
    s.get_details()
    return s


def _top(name):
    return WR.CASES[name][1] - 1


_problems, _ref_runs = {}, {}


def _problem(name):
    if name not in _problems:
        _problems[name] = WR.case_problem(name)[2]
    return _problems[name]


def _restatement(name):
    """the restatement's run to rtol 1e-10 from random_guess with d = 0, computed once: (x0, iterates x_1.., norms)"""
    if name not in _ref_runs:
        prob = _problem(name)
        N = prob.N[-1]
        x0 = WR.random_guess(N, prob.axes, prob.faces)
        hist = []
        _, norms, converged, _ = WR.wpcg(prob, x0, np.zeros((N, N, N)), 1e-10, 0.0, 60, history=hist)
        assert converged and len(hist) >= 5
        _ref_runs[name] = (x0, hist, norms)
    return _ref_runs[name]


# ------------------------------------------------------------ 1 - 3 agreement with the restatement, case by case
@gpu
@pytest.mark.parametrize("name", ALL)
def test_iterates_agree_with_the_restatement(name):
    """u after 1, 2 and 5 iterations against x_k, and the norms r_0 .. r_k: 100 x the measured summation spread.  The six
    one-face cases at 17^3 catch a wrong first or last unknown or a wrong weight on any one face; the combinations cover
    edges and corners of several Neumann faces, a periodic axis beside them, the projection, and no projection with
    sigma; 37^3 and 25^3 the tails off the ladder."""
    x0, hist, ref_norms = _restatement(name)
    prob = _problem(name)
    q = _top(name)
    su, sn = (SPREAD_U_SLAB, SPREAD_NORM_SLAB) if name == "f63_slab" else (SPREAD_U, SPREAD_NORM)
    with _solver(name) as s:
        for k in (1, 2, 5):
            s.upload(MG3D_U, q, x0)
            norms, info = s.wpcg_solve(rtol=0.0, atol=1e-300, max_iters=k)
            assert info["iterations"] == k and not info["converged"] and len(norms) == k + 1
            assert info["singular"] == (name in WR.SINGULAR) and info["rhs_mean"] == 0.
            u = s.download(MG3D_U, q).reshape(x0.shape)
            want = hist[k - 1]
            rel = np.abs(u - want).max() / np.abs(want).max()
            nrel = (np.abs(norms - ref_norms[:k + 1]) / ref_norms[:k + 1]).max()
            print(name, k, "u", rel, "norms", nrel)
            assert rel <= 100 * su[k], (name, k, rel)
            assert nrel <= 100 * sn, (name, k, nrel)
            if prob.axes:
                w = u.copy()
                NR.refresh(w, prob.axes)
                assert _same_bits(u, w), "duplicates differ from their sources"
            if name in WR.SINGULAR:
                drift = abs(WR.wmean(prob, u) - WR.wmean(prob, x0)) / np.abs(x0).max()
                print(name, k, "w-mean drift", drift)
                assert drift <= 100 * DRIFT, (name, k, drift)
            assert info["r_norm"] == norms[-1] and info["r0_norm"] == norms[0]


# ------------------------------------------------------------------------------------------------------ 4 robustness
@gpu
def test_robust_where_plain_cycles_grow():
    """33^3, all six faces Neumann, ball 100, random guess, d = 0: the solve converges to 1e-10 in at most the restatement's
    count + 1 iterations (a norm may land on either side of the threshold under another summation order); 60 plain
    V-cycles from the same start do not reach 1e-10 r_0 -- on the restatement their residual grows by 1.083 per cycle"""
    name = "f63_ball"
    x0, _, ref_norms = _restatement(name)
    q = _top(name)
    with _solver(name) as s:
        s.upload(MG3D_U, q, x0)
        norms, info = s.wpcg_solve(rtol=1e-10, max_iters=60)
        s.upload(MG3D_U, q, x0)
        r0 = s.residual(q, store=False)
        cyc = s.vcycles(60)
    print(name, "wpcg", info["iterations"], "restatement", len(ref_norms) - 1, "vcycles: last/r0", cyc[-1] / r0,
          "ratio", cyc[-1] / cyc[-2])
    assert info["converged"] and len(norms) == info["iterations"] + 1 and norms[-1] <= 1e-10 * norms[0]
    assert info["iterations"] <= len(ref_norms) - 1 + 1
    assert not (cyc <= 1e-10 * r0).any()


# ------------------------------------------------------------------------------------------------------ 5 true residual
@gpu
@pytest.mark.parametrize("name", ALL)
def test_true_residual(name):
    """d = A x* for a random x* (compatible by construction), random guess: after wpcg_solve(rtol = 1e-8) an independent
    mg3d_residual of the returned u is <= 2 rtol r0_norm and agrees with the recurrence's r_norm to 1e-6 relative"""
    prob = _problem(name)
    N, q = prob.N[-1], _top(name)
    xs = WR.random_guess(N, prob.axes, prob.faces, seed=21)
    d = np.zeros((N, N, N))
    NR.put(d, WR.apply(prob, xs), NR.block(N, prob.axes, prob.faces), prob.axes)
    x0 = WR.random_guess(N, prob.axes, prob.faces)
    with _solver(name) as s:
        s.upload(MG3D_U, q, x0)
        s.upload(MG3D_D, q, d)
        norms, info = s.wpcg_solve(rtol=1e-8)
        res = s.residual(q, store=False)
    print(name, info, res, abs(info["r_norm"] - res) / res)
    assert info["converged"] and info["r_norm"] <= 1e-8 * info["r0_norm"]
    assert res <= 2 * 1e-8 * info["r0_norm"]
    assert abs(info["r_norm"] - res) <= 1e-6 * res


# --------------------------------------------------------------------------------------------------- 6 incompatible d
@gpu
def test_incompatible_right_hand_side():
    """33^3, all six faces Neumann (singular), d uniform(-1, 1): rhs_mean is sum(w d)/W, d comes back bit for bit, the stored
    residual of the returned u less its w-mean has the norm r_norm, and u keeps the w-mean of the guess"""
    name = "f63_ball"
    prob = _problem(name)
    N, q = prob.N[-1], _top(name)
    x0 = WR.random_guess(N, prob.axes, prob.faces)
    d = np.random.default_rng(12).uniform(-1, 1, (N, N, N))
    w, W = WR.weights(prob)
    want_mean = WR.wsum(w, d) / W
    with _solver(name) as s:
        s.upload(MG3D_U, q, x0)
        s.upload(MG3D_D, q, d)
        norms, info = s.wpcg_solve(rtol=1e-8)
        d_after = s.download(MG3D_D, q)
        u = s.download(MG3D_U, q)
        s.residual(q, store=True)
        r = s.download(MG3D_R, q).reshape(N, N, N)
    assert info["singular"] and info["converged"]
    print("rhs_mean", info["rhs_mean"], want_mean, abs(info["rhs_mean"] - want_mean) / abs(want_mean))
    assert abs(want_mean) > 1e-4  # the right-hand side IS incompatible
    assert abs(info["rhs_mean"] - want_mean) <= 1e-13 * abs(want_mean)
    assert _same_bits(d_after, d.reshape(-1))
    r = r - WR.wsum(w, r) / W
    rn = float(np.sqrt((r * r).sum()))
    print("projected residual", rn, info["r_norm"], abs(rn - info["r_norm"]) / rn)
    assert abs(rn - info["r_norm"]) <= 1e-6 * rn
    drift = abs(WR.wmean(prob, u) - WR.wmean(prob, x0)) / np.abs(x0).max()
    print("w-mean drift", drift)
    assert drift <= 100 * DRIFT


# --------------------------------------------------------------------------------------------------------------- 7 state
@gpu
@pytest.mark.parametrize("name", ["f22_ball", "per4_f15_ball"])
def test_state_after_the_solve(name):
    """random values at every point of u and a random d: d and the Dirichlet points of u come back bit for bit -- on faces 22
    those include the edges a Neumann face shares with a Dirichlet face --, periodic duplicates equal their sources, a
    following vcycles(1) is the one of a fresh context with the returned u and d uploaded, max_iters = 0 changes nothing"""
    prob = _problem(name)
    N, q = prob.N[-1], _top(name)
    u0 = WR.random_guess(N, prob.axes, prob.faces, seed=9, dirichlet=True)
    d0 = np.random.default_rng(10).uniform(-1, 1, (N, N, N))
    NR.refresh(d0, prob.axes)
    fixed = ~(NR.unknown_mask(N, prob.axes, prob.faces) | NR.is_dup(N, prob.axes))
    if name == "f22_ball":
        assert fixed[N - 1, N - 1, 5] and fixed[N - 1, 5, N - 1] and fixed[0, 0, 5] and not fixed[N - 1, 0, 0]
    with _solver(name) as s, _solver(name) as fresh:
        s.upload(MG3D_U, q, u0)
        s.upload(MG3D_D, q, d0)
        norms, info = s.wpcg_solve(rtol=0.0, atol=1e-300, max_iters=0)
        assert info["iterations"] == 0 and len(norms) == 1 and info["r0_norm"] == norms[0] and not info["converged"]
        if name not in WR.SINGULAR:
            assert norms[0] == s.residual(q, store=False)
        assert _same_bits(s.download(MG3D_U, q), u0.reshape(-1)) and _same_bits(s.download(MG3D_D, q), d0.reshape(-1))
        norms, info = s.wpcg_solve(rtol=1e-8)
        assert info["converged"]
        u1 = s.download(MG3D_U, q)
        assert _same_bits(s.download(MG3D_D, q), d0.reshape(-1))
        assert _same_bits(u1.reshape(N, N, N)[fixed], u0[fixed])
        w = u1.reshape(N, N, N).copy()
        NR.refresh(w, prob.axes)
        assert _same_bits(w.reshape(-1), u1)
        n_a = s.vcycles(1)
        fresh.upload(MG3D_U, q, u1)
        fresh.upload(MG3D_D, q, d0)
        n_b = fresh.vcycles(1)
        assert _same_bits(s.download(MG3D_U, q), fresh.download(MG3D_U, q)) and n_a[0] == n_b[0]
        # a second solve reuses the work vectors: the same bits as the first one from the same data
        s.upload(MG3D_U, q, u0)
        norms2, _ = s.wpcg_solve(rtol=1e-8)
        assert np.array_equal(norms, norms2) and _same_bits(s.download(MG3D_U, q), u1)


# ------------------------------------------------------------------------------- 8 the bits of pcg_solve where it works
@gpu
@pytest.mark.parametrize("name", ["ball100", "per6_smooth"])
def test_same_bits_as_pcg_solve(name):
    c, L, sigma, _, axes = PR.CASES[name]
    N, eps, _ = PR.case_problem(name)
    x0 = PR.random_guess(N, axes)
    out = []
    for call in ("pcg_solve", "wpcg_solve"):
        with M.Solver(c, L, 2) as s:
            s.set_shift(sigma)
            s.set_periodic(axes)
            s.set_coefficient(eps)
            s.get_details()
            s.upload(MG3D_U, L - 1, x0)
            norms, info = getattr(s, call)(rtol=1e-10)
            out.append((norms, info, s.download(MG3D_U, L - 1)))
    (na, ia, ua), (nb, ib, ub) = out
    assert ia["converged"] and ia["iterations"] >= 5
    assert np.array_equal(na, nb) and _same_bits(ua, ub)
    assert ib["singular"] is False and ib["rhs_mean"] == 0. and {k: ib[k] for k in ia} == ia


# ---------------------------------------------------------------------------------------------- 9 refusals and arguments
@gpu
def test_refusals_and_arguments():
    N = 17
    rng = np.random.default_rng(6)
    u0, d0 = rng.uniform(-1, 1, N ** 3), rng.uniform(-1, 1, N ** 3)

    def refused(s, code, **kw):
        with pytest.raises(M.Mg3dError) as e:
            s.wpcg_solve(**kw)
        assert e.value.code == code, (kw, e.value)
        assert _same_bits(s.download(MG3D_U, 2), u0) and _same_bits(s.download(MG3D_D, 2), d0)

    for faces in (12, 63):
        with M.Solver(5, 3, 2) as s:
            s.set_neumann(faces)
            s.upload(MG3D_U, 2, u0)
            s.upload(MG3D_D, 2, d0)
            refused(s, MG3D_ERR_STATE)  # no coarse factor
            s.get_details()
            refused(s, MG3D_ERR_ARG, rtol=-1e-8)
            refused(s, MG3D_ERR_ARG, rtol=float("nan"))
            refused(s, MG3D_ERR_ARG, atol=-1.0)
            refused(s, MG3D_ERR_ARG, atol=float("inf"))
            refused(s, MG3D_ERR_ARG, max_iters=-1)
            refused(s, MG3D_ERR_ARG, rtol=0.0, atol=0.0, max_iters=0)
            norms, info = s.wpcg_solve()  # and the context is still good
            assert info["converged"] and info["singular"] == (faces == 63)
    es = M.EsParams.default()
    with M.Solver(5, 3, 2, grid_length=es.length) as s:  # the mixed-boundary factor
        s.es_setup(es)
        u_es, d_es = s.download(MG3D_U, 2), s.download(MG3D_D, 2)
        with pytest.raises(M.Mg3dError) as e:
            s.wpcg_solve()
        assert e.value.code == MG3D_ERR_STATE
        assert _same_bits(s.download(MG3D_U, 2), u_es) and _same_bits(s.download(MG3D_D, 2), d_es)


# --------------------------------------------------------------------------------------------------------- 10 past the cap
@gpu
def test_past_the_cap_513():
    """513^3 (c = 9, L = 7), all six faces Neumann, constant operator, smooth guess cos(pi x) cos(2 pi y) cos(pi z), d = 0,
    three iterations: the chunks of tests/test_wpcg_ref_host.py (16 planes for update + norm, 32 for the dot, a last chunk
    of one plane).  r_norm of the recurrence against an independent residual of the returned u, 1e-9 relative -- a dropped
    block of partial sums breaks it at once; the norms decrease"""
    c, L, N = 9, 7, 513
    t = np.linspace(0.0, 1.0, N)
    u0 = np.ascontiguousarray(np.cos(np.pi * t)[:, None, None] * np.cos(2 * np.pi * t)[None, :, None]
                              * np.cos(np.pi * t)[None, None, :])
    with M.Solver(c, L, 2) as s:
        s.set_neumann(63)
        s.get_details()
        s.upload(MG3D_U, L - 1, u0)
        del u0
        norms, info = s.wpcg_solve(rtol=0.0, atol=1e-300, max_iters=3)
        res = s.residual(L - 1, store=False)
    print("513^3", norms, res, abs(info["r_norm"] - res) / res)
    assert info["iterations"] == 3 and info["singular"] and np.all(np.diff(norms) < 0)
    assert abs(info["r_norm"] - res) <= 1e-9 * res
