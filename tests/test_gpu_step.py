"""mg3d_step_advance on the GPU against the CPU restatement tests/_step_ref.py: grid values bit for bit, norms at the
project's summation tolerance (1e-13 relative, tests/_oracle.py).

1  the right-hand side alone, every kernel variant ({constant, eps} x boundary mode x {theta < 1, theta = 1} x {source,
   none}) at the sizes where its walks can go wrong, with a sentinel where d must not be written
2  whole steps, u and d, and a source replaced between two calls
3  161^3, where the one-launch legs (default) and the carried cycles (legs = 0) run ahead between steps, against the route a
   caller had before: download u, the right-hand side in numpy, upload d, vcycles
4  the weighted-PCG method against _wpcg_ref.wpcg
5  state and arguments

Periodic masks need c - 1 even (mg3d_ctx_set_periodic): 37^3 and 145^3 (c = 10) run the masks without a periodic axis.

The right-hand side has two walks.  theta < 1 takes the column walk of the stencil kernels (a lane per k); theta = 1 the
pair walk of the CG vector passes (a lane per k-pair, pair_grid() of csrc/mg3d_kernels.hip, restated in
tests/test_wpcg_ref_host.py), which needs 129^3 for a second 64-lane block and 257^3 with six Neumann faces to pass the
cap on blocks; the shapes of the large sizes are those tests/test_gpu_cg_shapes.py recomputes from the header."""

import numpy as np
import pytest

import _coef_ref as CR
import _neumann_ref as NR
import _step_ref as SR
import _wpcg_ref as WR
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U

gpu = pytest.mark.gpu

MG3D_ERR_ARG, MG3D_ERR_STATE = 1, 5
NORM_RTOL = 1e-13
DT, KAPPA = 0.01, 0.75
SENTINEL = 12345.678
# boundary word of a case: (periodic axes, Neumann faces)
BCS = {"dirichlet": (0, 0), "per7": (7, 0), "per4_f15": (4, 15), "f63": (0, 63), "f22": (0, 22),
       "f32": (0, 32), "f25": (0, 0b011001)}  # the high k face alone; ilo + jhi + klo
SMALL_BCS = ("dirichlet", "per7", "per4_f15", "f63", "f22")
THETA_SRC = [(theta, src) for theta in (1.0, 0.5) for src in (True, False)]
# (c, L): 17, 37 (off the 2^k+1 ladder), 33 (31 unknown planes: a 16-plane chunk and a 15-plane tail), 65 with Neumann
# k-faces (65 unknown k: in the column walk of theta < 1 a second 64-lane block with one live lane; the pair walk of
# theta = 1 has 33 k-pairs there, one block).  The pair walk past one k-block and past the cap:
#   129 f63, f32   65 pairs: a second k-block with one live lane; f63: 129 rows, a last j-block of one row
#   129 per7       64 pairs, lo = 0 on every axis (the WRAP column kernels at 128 unknown k: two full blocks)
#   145            off the ladder, 72 pairs: 8 live lanes in the second k-block; f25: lo/hi mixed per axis
#   257 f63        129 pairs: three k-blocks, one live lane; 3 * 65 * 257 blocks exceed the cap: two planes per block
#                  and a last chunk of ONE plane
SIZES = {17: (5, 3), 37: (10, 3), 33: (5, 4), 65: (5, 5), 129: (5, 6), 145: (10, 5), 257: (9, 6)}
RHS_CASES = ([(17, coef, bc) for coef in (False, True) for bc in SMALL_BCS]
             + [(37, coef, bc) for coef in (False, True) for bc in ("dirichlet", "f63", "f22")]
             + [(33, coef, bc) for coef in (False, True) for bc in SMALL_BCS]
             + [(65, coef, bc) for coef in (False, True) for bc in ("f63", "per4_f15")]
             + [(129, coef, bc) for coef in (False, True) for bc in ("f63", "f32", "per7")]
             + [(145, coef, bc) for coef in (False, True) for bc in ("dirichlet", "f25")]
             + [(257, False, "f63")])
STEP_CASES = [(N, coef, bc) for N in (17, 33) for coef in (False, True) for bc in SMALL_BCS]


def _same_bits(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


class _Op:
    """what _wpcg_ref.apply reads of a problem: the finest level's operator, without the hierarchy"""

    def __init__(self, N, sigma, eps, axes, faces):
        self.N, self.h, self.sigma, self.axes, self.faces = [N], 1.0 / (N - 1), sigma, axes, faces
        self.eps = None if eps is None else [eps]


def _eps(N, coef, axes):
    if not coef:
        return None
    e = CR.ball_eps(N, 100.)
    NR.refresh(e, axes)  # (the library copies the sources over the duplicates)
    return e


def _solver(N, coef, bc, theta=None, kappa=KAPPA, build=True):
    c, L = SIZES[N]
    axes, faces = BCS[bc]
    s = M.Solver(c, L, 2)
    s.set_periodic(axes)
    s.set_neumann(faces)
    if coef:
        s.set_coefficient(_eps(N, True, axes))
    if build:
        s.get_details()
    if theta is not None:
        s.step_setup(DT, theta, kappa)
    return s


def _fields(N, axes, faces, seed):
    rng = np.random.default_rng(seed)
    u0 = WR.random_guess(N, axes, faces, seed=seed, dirichlet=True)
    src = rng.uniform(-1, 1, (N, N, N))
    return u0, src


# ------------------------------------------------------------------------------------------------ 1 the right-hand side
@gpu
@pytest.mark.parametrize("N,coef,bc", RHS_CASES)
def test_rhs_alone(N, coef, bc):
    """step_advance(1, cycles=1), then d (specified to survive the solve) against _step_ref.rhs at the unknowns, and the
    sentinel everywhere else: Dirichlet points and periodic duplicates of d are not written"""
    axes, faces = BCS[bc]
    q = SIZES[N][1] - 1
    u0, src = _fields(N, axes, faces, 11)
    unk = NR.unknown_mask(N, axes, faces)
    blk = NR.block(N, axes, faces)
    eps = _eps(N, coef, axes)
    with _solver(N, coef, bc) as s:
        for theta, with_src in THETA_SRC:
            s.step_setup(DT, theta, KAPPA)
            assert s.get_shift() == SR.sigma_of(DT, theta, KAPPA)
            s.step_set_source(src if with_src else None)
            s.upload(MG3D_U, q, u0)
            s.upload(MG3D_D, q, np.full((N, N, N), SENTINEL))
            norms, info = s.step_advance(1, cycles=1)
            assert info["steps"] == 1 and info["time"] == DT and len(norms) == 1 and np.isfinite(norms[0])
            d = s.download(MG3D_D, q).reshape(N, N, N)
            want = SR.rhs(_Op(N, s.get_shift(), eps, axes, faces), u0, src if with_src else None, DT, theta, KAPPA)
            assert _same_bits(d[blk], want), (N, coef, bc, theta, with_src)
            assert np.all(d[~unk] == SENTINEL), (N, coef, bc, theta, with_src)
            assert _same_bits(s.download(MG3D_U, q).reshape(N, N, N)[~(unk | NR.is_dup(N, axes))],
                              u0[~(unk | NR.is_dup(N, axes))])


# ------------------------------------------------------------------------------------------------------------ 2 steps
def _reference_run(N, coef, bc, theta, src, u0, calls):
    """calls: [(nsteps, source or None), ...] on one problem; returns (u, d, norms)"""
    c, L = SIZES[N]
    axes, faces = BCS[bc]
    prob = SR.make_problem(c, L, 2, DT, theta, KAPPA, _eps(N, coef, axes), axes, faces)
    prob.u[-1][...] = u0
    norms = []
    for nsteps, s in calls:
        norms += list(SR.advance(prob, nsteps, 2, s, DT, theta, KAPPA)[0])
    return prob.u[-1], prob.d[-1], np.array(norms)


@gpu
@pytest.mark.parametrize("N,coef,bc", STEP_CASES)
def test_steps(N, coef, bc):
    """3 steps x 2 cycles: u (every point) and d (the unknowns; the rest stays 0) bit for bit, one norm per step"""
    axes, faces = BCS[bc]
    q = SIZES[N][1] - 1
    u0, src = _fields(N, axes, faces, 12)
    blk = NR.block(N, axes, faces)
    with _solver(N, coef, bc) as s:
        for theta, with_src in THETA_SRC:
            sv = src if with_src else None
            want_u, want_d, want_n = _reference_run(N, coef, bc, theta, sv, u0, [(3, sv)])
            s.step_setup(DT, theta, KAPPA)
            s.step_set_source(sv)
            s.upload(MG3D_U, q, u0)
            s.zero(MG3D_D, q)
            norms, info = s.step_advance(3, cycles=2)
            print(N, coef, bc, theta, with_src, norms, np.abs(norms - want_n) / want_n)
            assert info == {"steps": 3, "iterations": 0, "converged": False, "time": 3 * DT}
            assert _same_bits(s.download(MG3D_U, q), want_u), (theta, with_src)
            d = s.download(MG3D_D, q).reshape(N, N, N)
            assert _same_bits(d[blk], want_d[blk]), (theta, with_src)
            d[blk] = 0.
            assert not d.any()
            np.testing.assert_allclose(norms, want_n, rtol=NORM_RTOL)


@gpu
def test_source_replaced_between_calls():
    N, coef, bc, theta = 17, False, "dirichlet", 0.5
    u0, s1 = _fields(N, 0, 0, 13)
    s2 = np.random.default_rng(14).uniform(-1, 1, (N, N, N))
    want_u, want_d, want_n = _reference_run(N, coef, bc, theta, None, u0, [(2, s1), (1, s2)])
    blk = NR.block(N, 0, 0)
    with _solver(N, coef, bc, theta) as s:
        s.upload(MG3D_U, 2, u0)
        s.step_set_source(s1)
        na, _ = s.step_advance(2, cycles=2)
        s.step_set_source(s2)
        nb, _ = s.step_advance(1, cycles=2)
        assert _same_bits(s.download(MG3D_U, 2), want_u)
        assert _same_bits(s.download(MG3D_D, 2).reshape(N, N, N)[blk], want_d[blk])
        np.testing.assert_allclose(np.concatenate([na, nb]), want_n, rtol=NORM_RTOL)


# -------------------------------------------------------------------------------------------------------- 3 schedules
@gpu
@pytest.mark.parametrize("legs", [1, 0])
def test_schedules_that_run_ahead_161(legs):
    """161^3 (c = 6, L = 6), constant operator, Dirichlet faces, theta = 0.5, 3 steps x 2 cycles: the smallest size where
    the one-launch legs (legs_min 160) and, with legs = 0, the carried cycles (carry_min 130) apply -- the last cycle of
    a step leaves the next cycle's first red pass to be skipped (and, behind mg3d_vcycle, a down-leg running ahead).
    Against the route a caller had before, in a second context: download u, _step_ref.rhs, upload d, vcycles(2).  A
    stepper that does not finish the cycle before it writes d differs here"""
    c, L, N, theta = 6, 6, 161, 0.5
    u0 = WR.random_guess(N, 0, 0, seed=15, dirichlet=True)
    blk = NR.block(N, 0, 0)
    with M.Solver(c, L, 2) as a, M.Solver(c, L, 2) as b:
        for s in (a, b):
            s.set_option("legs", legs)
            s.get_details()
            s.upload(MG3D_U, L - 1, u0)
        a.step_setup(DT, theta, KAPPA)
        b.set_shift(SR.sigma_of(DT, theta, KAPPA))
        got_n, info = a.step_advance(3, cycles=2)
        op = _Op(N, b.get_shift(), None, 0, 0)
        want_n = []
        for _ in range(3):
            d = np.zeros((N, N, N))
            d[blk] = SR.rhs(op, b.download(MG3D_U, L - 1).reshape(N, N, N), None, DT, theta, KAPPA)
            b.upload(MG3D_D, L - 1, d)
            want_n.append(b.vcycles(2)[-1])
        assert info["steps"] == 3
        assert _same_bits(a.download(MG3D_U, L - 1), b.download(MG3D_U, L - 1))
        assert _same_bits(a.download(MG3D_D, L - 1).reshape(N, N, N)[blk], d[blk])
        np.testing.assert_allclose(got_n, want_n, rtol=NORM_RTOL)


# ------------------------------------------------------------------------------------------------------------- 4 wpcg
# tests/test_gpu_wpcg.py: the restatement's cycles are the library's bit for bit, only the sums differ in summation order;
# two restatement runs with different summation orders differ in the iterate after k iterations by at most these figures
# (max|a - b| / max|a|; measured there), the GPU is allowed 100 x.  Two steps of two iterations each are four iterations
# with one restart: the figure of the smallest tabulated k >= 4.
from test_gpu_wpcg import SPREAD_NORM, SPREAD_U  # noqa: E402


@gpu
@pytest.mark.parametrize("name", ["f22_ball", "f63_ball"])
def test_wpcg_method(name):
    c, L, _, _, axes, faces = WR.CASES[name]
    N = (c - 1) * (1 << (L - 1)) + 1
    eps = CR.ball_eps(N, 100.)
    theta = 0.5
    u0, src = _fields(N, axes, faces, 16)

    def reference(cycles, rtol):
        prob = SR.make_problem(c, L, 2, DT, theta, KAPPA, eps, axes, faces)
        prob.u[-1][...] = u0
        norms, iters, conv = SR.advance(prob, 2, cycles, src, DT, theta, KAPPA, method="wpcg", rtol=rtol)
        return prob.u[-1].copy(), norms, iters, conv

    with M.Solver(c, L, 2) as s:
        s.set_neumann(faces)
        s.set_coefficient(eps)
        s.get_details()
        s.step_setup(DT, theta, KAPPA)
        s.step_set_source(src)
        # exactly two iterations per step
        want_u, want_n, want_it, want_conv = reference(2, 0.0)
        assert want_it == 4 and not want_conv
        s.upload(MG3D_U, L - 1, u0)
        norms, info = s.step_advance(2, cycles=2, method="wpcg", rtol=0.0)
        u = s.download(MG3D_U, L - 1).reshape(N, N, N)
        rel = np.abs(u - want_u).max() / np.abs(want_u).max()
        nrel = (np.abs(norms - want_n) / want_n).max()
        print(name, "u", rel, "norms", nrel)
        assert info == {"steps": 2, "iterations": 4, "converged": False, "time": 2 * DT}
        assert rel <= 100 * SPREAD_U[5] and nrel <= 100 * SPREAD_NORM
        # to a tolerance: every step converges, the counts add up (a norm may land on either side of the threshold under
        # another summation order: one iteration per step, as tests/test_gpu_wpcg.py allows)
        want_u, want_n, want_it, want_conv = reference(30, 1e-6)
        assert want_conv
        s.upload(MG3D_U, L - 1, u0)
        norms, info = s.step_advance(2, cycles=30, method="wpcg", rtol=1e-6)
        print(name, info, want_it, norms, want_n)
        assert info["converged"] and info["steps"] == 2 and abs(info["iterations"] - want_it) <= 2
        # one step short of its tolerance: not converged
        s.upload(MG3D_U, L - 1, u0)
        _, info = s.step_advance(2, cycles=1, method="wpcg", rtol=1e-12)
        assert info["iterations"] == 2 and not info["converged"]


# ------------------------------------------------------------------------------------------------ 5 state and arguments
@gpu
def test_state_and_arguments():
    N, q = 17, 2
    rng = np.random.default_rng(17)
    u0, d0 = rng.uniform(-1, 1, N ** 3), rng.uniform(-1, 1, N ** 3)

    def refused(s, code, call, sigma):
        with pytest.raises(M.Mg3dError) as e:
            call()
        assert e.value.code == code, e.value
        assert _same_bits(s.download(MG3D_U, q), u0) and _same_bits(s.download(MG3D_D, q), d0)
        assert s.get_shift() == sigma

    with M.Solver(5, 3, 2) as s:
        s.upload(MG3D_U, q, u0)
        s.upload(MG3D_D, q, d0)
        s.get_details()
        refused(s, MG3D_ERR_STATE, lambda: s.step_advance(1), 0.0)  # mg3d_step_setup was never called
        for bad in [(0.0, 1.0, 0.0), (-1.0, 1.0, 0.0), (float("nan"), 1.0, 0.0), (float("inf"), 1.0, 0.0),
                    (DT, 0.4, 0.0), (DT, 1.1, 0.0), (DT, float("nan"), 0.0), (DT, 1.0, -1.0), (DT, 1.0, float("inf")),
                    (DT, 1.0, float("nan")), (1e-320, 1.0, 0.0)]:
            refused(s, MG3D_ERR_ARG, lambda: s.step_setup(*bad), 0.0)
        refused(s, MG3D_ERR_STATE, lambda: s.step_advance(1), 0.0)  # ... and a refused setup is none
        s.step_setup(DT, 0.5, KAPPA)
        sigma = SR.sigma_of(DT, 0.5, KAPPA)
        assert s.get_shift() == sigma
        refused(s, MG3D_ERR_ARG, lambda: s.step_advance(-1), sigma)
        refused(s, MG3D_ERR_ARG, lambda: s.step_advance(1, cycles=0), sigma)
        refused(s, MG3D_ERR_ARG, lambda: s.step_advance(1, method="wpcg", rtol=-1e-8), sigma)
        refused(s, MG3D_ERR_ARG, lambda: s.step_advance(1, method="wpcg", rtol=float("nan")), sigma)
        refused(s, MG3D_ERR_ARG, lambda: s.step_advance(1, method="wpcg", rtol=float("inf")), sigma)
        assert s.L.mg3d_step_advance(s._h, 1, 2, 2, 1e-8, None, None) == MG3D_ERR_ARG  # a method that is neither
        assert s.L.mg3d_step_advance(s._h, 1, -1, 2, 1e-8, None, None) == MG3D_ERR_ARG
        assert _same_bits(s.download(MG3D_U, q), u0) and _same_bits(s.download(MG3D_D, q), d0)
        with pytest.raises(ValueError):
            s.step_advance(1, method="jacobi")
        # nsteps = 0 changes nothing
        norms, info = s.step_advance(0)
        assert len(norms) == 0 and info == {"steps": 0, "iterations": 0, "converged": False, "time": 0.0}
        assert _same_bits(s.download(MG3D_U, q), u0) and _same_bits(s.download(MG3D_D, q), d0)
        # somebody changed the shift since
        s.set_shift(2.0)
        refused(s, MG3D_ERR_STATE, lambda: s.step_advance(1), 2.0)
        s.set_shift(sigma)  # ... and put it back
        norms, info = s.step_advance(1)
        assert info["steps"] == 1 and s.get_shift() == sigma
    with M.Solver(5, 3, 2) as s:  # no coarse factor
        s.upload(MG3D_U, q, u0)
        s.upload(MG3D_D, q, d0)
        s.step_setup(DT, 1.0, 0.0)
        refused(s, MG3D_ERR_STATE, lambda: s.step_advance(1), 1.0 / DT)
    # The mixed-boundary factor.  The driver has no test of its own for it: mg3d_es_setup needs sigma = 0 and the shift of
    # mg3d_step_setup is > 0 and drops the factor, so such a context is refused as "never set up" (before step_setup), as
    # "no coarse factor" (after it), or as "the shift changed" (step_setup, set_shift(0), es_setup) -- all three here
    es = M.EsParams.default()
    with M.Solver(5, 3, 2, grid_length=es.length) as s:
        s.es_setup(es)
        u_es, d_es = s.download(MG3D_U, q), s.download(MG3D_D, q)

        def refused_es():
            with pytest.raises(M.Mg3dError) as e:
                s.step_advance(1)
            assert e.value.code == MG3D_ERR_STATE
            assert _same_bits(s.download(MG3D_U, q), u_es) and _same_bits(s.download(MG3D_D, q), d_es)

        refused_es()
        s.step_setup(DT, 1.0, 0.0)
        with pytest.raises(M.Mg3dError) as e:  # sigma != 0
            s.es_setup(es)
        assert e.value.code == MG3D_ERR_STATE
        refused_es()
        s.set_shift(0.0)
        s.es_setup(es)
        u_es, d_es = s.download(MG3D_U, q), s.download(MG3D_D, q)
        refused_es()


@gpu
@pytest.mark.parametrize("bc", ["dirichlet", "per4_f15"])
def test_context_usable_afterwards_and_source_dropped(bc):
    """after step_advance, vcycles(1) is bit for bit the one of a fresh context with the same u, d and sigma uploaded;
    step_set_source(None) returns to the form without a source"""
    N, q, theta = 17, 2, 0.5
    axes, faces = BCS[bc]
    u0, src = _fields(N, axes, faces, 18)
    blk = NR.block(N, axes, faces)
    with _solver(N, True, bc, theta) as s, _solver(N, True, bc) as fresh:
        s.upload(MG3D_U, q, u0)
        s.step_set_source(src)
        s.step_advance(2, cycles=2)
        u1, d1 = s.download(MG3D_U, q), s.download(MG3D_D, q)
        n_a = s.vcycles(1)
        fresh.set_shift(s.get_shift())
        fresh.upload(MG3D_U, q, u1)
        fresh.upload(MG3D_D, q, d1)
        n_b = fresh.vcycles(1)
        assert _same_bits(s.download(MG3D_U, q), fresh.download(MG3D_U, q)) and n_a[0] == n_b[0]
        s.step_set_source(None)
        s.upload(MG3D_U, q, u0)
        s.step_advance(1, cycles=1)
        want = SR.rhs(_Op(N, s.get_shift(), _eps(N, True, axes), axes, faces), u0, None, DT, theta, KAPPA)
        assert _same_bits(s.download(MG3D_D, q).reshape(N, N, N)[blk], want)
