"""mg3d_nl_residual and mg3d_nl_solve on the GPU.

1  the linear part of the evaluation, bit for bit: with g0 = 0 nl_residual(store=True) gives the bits of Solver.residual on
   the same context and the same norm, for both kinds, {constant, eps} x boundary mode x {no mask, a masked ball}, at the
   sizes where the column walk can go wrong, a sentinel in r where nothing may be written; one case past the cap on partial
   sums (513^3 with a Neumann pair in j), GPU against GPU, with a CPU test of its launch geometry
2  the nonlinear part: F - lin and s against numpy with phi in np.longdouble, to the ulp bound derived at _phi_bounds
3  the composition, bit for bit through existing calls: s on every level against _shift_field_ref.restrict_field, one Newton
   step against set_shift_field + vcycles / wpcg_solve on a plain context
4  whole solves, by properties, with the caps of tests/_nl_ref.py
5  entry behind a cycle that has run ahead (161^3)
6  state and arguments

The norm in 1: a constant-coefficient Dirichlet context without a mask runs Solver.residual through the fused sweep kernel,
whose partial sums have another order than the column walk's; there the norm is compared, exactly, with that of the same
context with the fused schedules off (MG3D_NO_FUSE at creation: the column-walk residual kernel, the same F bits), and with
the fused one at the project's summation tolerance."""
import functools

import numpy as np
import pytest
import torch  # before the package, as bench.py does: the HIP runtime is torch's

import _coef_ref as CR
import _mask_ref as MR
import _neumann_ref as NR
import _nl_ref as NL
import _shift_field_ref as SF
import _wpcg_ref as WR
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U

from test_gpu_stencil_shapes import _max_partials, column_grid

gpu = pytest.mark.gpu

MG3D_ERR_ARG, MG3D_ERR_STATE = 1, 5
NORM_RTOL = 1e-13
SENTINEL = 12345.678
BCS = {"dirichlet": (0, 0), "per7": (7, 0), "per4_f15": (4, 15), "f63": (0, 63), "f22": (0, 22), "f12": (0, 12)}
SMALL_BCS = ("dirichlet", "per7", "per4_f15", "f63", "f22")
SIZES = {17: (5, 3), 33: (5, 4), 37: (10, 3), 65: (5, 5), 161: (6, 6), 513: (9, 7)}
# 17; 33 (31 unknown planes: a 16-plane chunk and a 15-plane tail); 37 off the 2^k+1 ladder (c - 1 odd: no periodic axis);
# 65 with Neumann k-faces (65 unknown k: a second 64-lane block with one live lane)
LIN_CASES = ([(17, coef, bc) for coef in (False, True) for bc in SMALL_BCS]
             + [(33, coef, bc) for coef in (False, True) for bc in SMALL_BCS]
             + [(37, coef, bc) for coef in (False, True) for bc in ("dirichlet", "f63", "f22")]
             + [(65, coef, bc) for coef in (False, True) for bc in ("f63", "per4_f15")])
NL_CASES = [case for case in LIN_CASES if case[0] != 37]
BIG = (513, "f12")
G0, BETA, UREF = 1.75, 1.5, 0.25
W_MAX = {"exp": 30.0, "sinh": 20.0}


def _same_bits(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _eps(N, coef, axes, jump=100.):
    if not coef:
        return None
    e = CR.ball_eps(N, jump)
    NR.refresh(e, axes)
    return e


def _ball(N, axes):
    return MR.stored(MR.sphere(N).astype(np.uint8), axes)


def _solver(N, coef, bc, masked=False, build=True, jump=100.):
    c, L = SIZES[N]
    axes, faces = BCS[bc]
    s = M.Solver(c, L, 2)
    s.set_periodic(axes)
    s.set_neumann(faces)
    if coef:
        s.set_coefficient(_eps(N, True, axes, jump))
    if masked:
        s.set_mask(_ball(N, axes))
    if build:
        s.get_details()
    return s


def _w_field(N, kind, seed):
    """u with w = BETA*(u - UREF) spread over [-W, W], every 7th point at |w| < 1e-8 (down to 1e-13), both signs"""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-W_MAX[kind], W_MAX[kind], (N, N, N))
    tiny = 10.0 ** rng.uniform(-13, -8, (N, N, N)) * rng.choice([-1.0, 1.0], (N, N, N))
    w.reshape(-1)[::7] = tiny.reshape(-1)[::7]
    return UREF + w / BETA


# ------------------------------------------------------------------------------------------------ 1 the linear part
def test_the_case_past_the_cap_has_the_launch_geometry_it_was_chosen_for():
    """column_grid()'s arithmetic and the header's MG3D_MAX_PARTIALS (no GPU): 513^3 Dirichlet sits exactly at the cap with
    chunk 16; the Neumann pair in j adds one row block of one live row, which passes the cap and doubles the chunk, leaving
    a last chunk of 31 planes; the small sizes have one chunk (17), a 15-plane tail (33), a lane block with one live lane
    (65 with Neumann k-faces)"""
    cap = _max_partials()
    N, bc = BIG
    assert (SIZES[N][0] - 1) * (1 << (SIZES[N][1] - 1)) + 1 == N
    gx, gy, gz, chunk, planes = column_grid(N, 0, 0)
    assert (gx, gy, gz, chunk) == (8, 128, 32, 16) and gx * gy * gz == cap
    gx, gy, gz, chunk, planes = column_grid(N, *BCS[bc])
    assert (gx, gy, gz, chunk, planes) == (8, 129, 16, 32, 511) and gx * gy * gz <= cap
    assert 8 * 129 * 32 > cap and planes - (gz - 1) * chunk == 31 and (N - 2 + 2) - (gy - 1) * 4 == 1
    assert column_grid(17, 0, 0) == (1, 4, 1, 16, 15)
    assert column_grid(33, 0, 0)[2:] == (2, 16, 31)
    assert column_grid(65, 0, 63)[0] == 2 and 65 - 64 == 1
    for n, (c, L) in SIZES.items():
        assert (c - 1) * (1 << (L - 1)) + 1 == n


@gpu
@pytest.mark.parametrize("N,coef,bc", LIN_CASES)
def test_linear_part_bit_for_bit(N, coef, bc, monkeypatch):
    axes, faces = BCS[bc]
    q = SIZES[N][1] - 1
    u = WR.random_guess(N, axes, faces, seed=N, dirichlet=True)
    d = np.random.default_rng(N + 1).uniform(-1, 1, (N, N, N))
    NR.refresh(d, axes)
    sentinel = np.full((N, N, N), SENTINEL)
    for masked in (False, True):
        with _solver(N, coef, bc, masked) as s:
            s.upload(MG3D_U, q, u)
            s.upload(MG3D_D, q, d)
            s.upload(MG3D_R, q, sentinel)
            want_n = s.residual(q, store=True)
            want = s.download(MG3D_R, q)
            assert (want == SENTINEL).sum() == (~(NR.unknown_mask(N, axes, faces) | NR.is_dup(N, axes))).sum()
            ref_n = want_n
            if not coef and bc == "dirichlet" and not masked:  # the fused sweep formed want_n: see the module docstring
                monkeypatch.setenv("MG3D_NO_FUSE", "1")
                with _solver(N, coef, bc, masked) as t:
                    monkeypatch.delenv("MG3D_NO_FUSE")
                    t.upload(MG3D_U, q, u)
                    t.upload(MG3D_D, q, d)
                    t.upload(MG3D_R, q, sentinel)
                    ref_n = t.residual(q, store=True)
                    assert _same_bits(t.download(MG3D_R, q), want)
                assert ref_n == pytest.approx(want_n, rel=NORM_RTOL)
            for kind in ("exp", "sinh"):
                s.nl_setup(kind, 0.0, 0.7, 0.1)
                s.upload(MG3D_R, q, sentinel)
                n = s.nl_residual(store=True)
                print(N, coef, bc, masked, kind, repr(n), repr(ref_n), repr(want_n))
                assert _same_bits(s.download(MG3D_R, q), want), (N, coef, bc, masked, kind)
                assert n == ref_n, (N, coef, bc, masked, kind)
                s.upload(MG3D_R, q, sentinel)
                assert s.nl_residual(store=False) == n
                assert np.all(s.download(MG3D_R, q) == SENTINEL)
                assert _same_bits(s.download(MG3D_U, q), u) and _same_bits(s.download(MG3D_D, q), d)
                assert not s.has_shift_field()


# ---------------------------------------------------------------------------------------------- 2 the nonlinear part
def _phi_bounds(kind):
    """The bound, in units of 2^-52 relative to the exact term (an ulp of a double x is at most 2^-52 |x|).
    The kernel forms  w = beta*(u - uref)  (restated bit for bit in numpy: the same two IEEE operations, no allowance),
    ph = phi(w), dph = phi'(w)  by the device library's double functions, built to the OpenCL conformance bounds -- exp 3 ulp,
    sinh 4 ulp, cosh 4 ulp --, gp = g0*g and gb = gp*beta (restated bit for bit), then
        t = fl(gp*ph)       one rounding, 1/2 ulp          |t - T| <= |T| (U_phi + 1/2) 2^-52       T = gp*phi(w) exact
        F = fl(lin + t)     one rounding of the SUM        |F - (lin + T)| <= |T| (U_phi + 1/2) 2^-52 + 2^-53 |lin + T|
        s = fl(gb*dph)      one rounding                   |s - S| <= |S| (U_phi' + 1/2) 2^-52     S = gb*phi'(w) exact
    lin is the linear part's own double (test 1 holds it to mg3d_residual bit for bit) and carries no allowance.  Products of
    two relative errors (2^-104) are covered by the factor 1 + 2^-40 on the whole bound.
    Returns (U_phi + 1/2, U_phi' + 1/2)."""
    return (3.5, 3.5) if kind == "exp" else (4.5, 4.5)


def _check_nonlinear(kind, u_blk, lin_blk, g_blk, F_blk, S_blk, fx):
    """F and s on a set of unknowns against the longdouble reference; returns the largest errors seen, in 2^-52 relative to
    the exact term, of the function part of F and of s"""
    ld = np.longdouble
    uF, uS = _phi_bounds(kind)
    w = BETA * (u_blk - UREF)
    ph, dph = NL.phi(kind, w.astype(ld))
    gp = G0 * g_blk if g_blk is not None else np.full(w.shape, G0)
    gb = gp * BETA
    T = gp.astype(ld) * ph
    Fref = lin_blk.astype(ld) + T
    Sref = gb.astype(ld) * dph
    assert np.all(F_blk[fx] == 0.) and np.all(S_blk[fx] == 0.)
    ok = ~fx
    eps52, slack = ld(2.0) ** -52, 1 + ld(2.0) ** -40
    errF = np.abs(F_blk.astype(ld) - Fref)[ok]
    errS = np.abs(S_blk.astype(ld) - Sref)[ok]
    sumF = (np.abs(Fref) * eps52 / 2)[ok]
    aT, aS = np.abs(T)[ok], np.abs(Sref)[ok]
    nz = aT > 0
    worstF = float(np.max(np.maximum(errF[nz] - sumF[nz], 0) / (aT[nz] * eps52))) if nz.any() else 0.
    nzs = aS > 0
    worstS = float(np.max(errS[nzs] / (aS[nzs] * eps52))) if nzs.any() else 0.
    small = np.abs(w[ok]) < 1e-8
    assert small.any() and (np.abs(w[ok]) > 0.9 * W_MAX[kind]).any()
    assert np.all(errF <= (aT * uF * eps52 + sumF) * slack), (kind, worstF)
    assert np.all(errS <= aS * uS * eps52 * slack), (kind, worstS)
    assert np.all(errS[~nzs] == 0)
    return worstF, worstS


def _weights(N, axes, seed):
    """None, an fp64 tensor view and an fp32 tensor view (both strided, neither contiguous), with the doubles they stand for"""
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.0, 2.0, (N, N, N))
    g.reshape(-1)[::5] = 0.
    NR.refresh(g, axes)
    dev = torch.device("cuda:0")
    t64 = torch.zeros((N, N, 2 * N), dtype=torch.float64, device=dev)
    t64[:, :, ::2] = torch.from_numpy(g).to(dev)
    t32 = torch.zeros((N, 2 * N, N), dtype=torch.float32, device=dev)
    t32[:, ::2, :] = torch.from_numpy(g.astype(np.float32)).to(dev)
    return [("none", None, None), ("f64", t64[:, :, ::2], g), ("f32", t32[:, ::2, :], g.astype(np.float32).astype(np.float64))]


@gpu
@pytest.mark.parametrize("N,coef,bc", NL_CASES)
def test_nonlinear_part_to_the_ulp_bound(N, coef, bc):
    axes, faces = BCS[bc]
    q = SIZES[N][1] - 1
    blk = NR.block(N, axes, faces)
    unk = NR.unknown_mask(N, axes, faces)
    d = np.random.default_rng(N + 2).uniform(-1, 1, (N, N, N))
    NR.refresh(d, axes)
    worst = {}
    for masked in (False, True):
        fx = MR.fixed(_ball(N, axes) if masked else np.zeros((N, N, N), dtype=np.uint8), axes, faces)[blk]
        with _solver(N, coef, bc, masked) as s:
            s.upload(MG3D_D, q, d)
            for kind in ("exp", "sinh"):
                u = _w_field(N, kind, N + 3)
                NR.refresh(u, axes)
                s.upload(MG3D_U, q, u)
                s.nl_setup(kind, 0.0, BETA, UREF)
                s.nl_set_weight(None)
                s.nl_residual(store=True)
                lin = s.download(MG3D_R, q).reshape(N, N, N)[blk]
                s.nl_setup(kind, G0, BETA, UREF)
                for name, tensor, g in _weights(N, axes, N + 4):
                    s.nl_set_weight_tensor(tensor)
                    nF = s.nl_residual(store=True)
                    F = s.download(MG3D_R, q).reshape(N, N, N)
                    norms, info = s.nl_solve(max_newton=0)
                    S = s.get_shift_field(q).reshape(N, N, N)
                    assert info["iterations"] == 0 and norms[0] == nF == info["norm0"] == info["norm"]
                    assert np.all(S[~(unk | NR.is_dup(N, axes))] == 0.)
                    wF, wS = _check_nonlinear(kind, u[blk], lin, None if g is None else g[blk], F[blk], S[blk], fx)
                    worst[kind] = tuple(max(a, b) for a, b in zip(worst.get(kind, (0., 0.)), (wF, wS)))
                    s.set_shift_field(None)
                    assert not s.has_shift_field()
                # the host form stores what the fp64 tensor stores
                _, t64, g64 = _weights(N, axes, N + 4)[1]
                s.nl_set_weight(g64)
                n_host = s.nl_residual(store=True)
                F_host = s.download(MG3D_R, q)
                s.nl_set_weight_tensor(t64)
                assert s.nl_residual(store=True) == n_host and _same_bits(s.download(MG3D_R, q), F_host)
    print("largest error in units of 2^-52 relative (F's function part, s):", N, coef, bc, worst)


@gpu
def test_past_the_partial_cap():
    """513^3 with a Neumann pair in j (chunk 32, 8 x 129 x 16 blocks), per kind on a u that spans the kind's range of w: the
    linear part against Solver.residual on the GPU, every bit of r and the norm; then g0 > 0 on a seeded sample of 10^5
    unknowns to the ulp bound"""
    N, bc = BIG
    axes, faces = BCS[bc]
    q = SIZES[N][1] - 1
    rng = np.random.default_rng(513)
    d = rng.uniform(-1, 1, (N, N, N))
    idx = tuple(rng.integers(lo, hi + 1, 100000) for lo, hi in (NR.lo_hi(N, axes, faces, ax) for ax in range(3)))
    sentinel = np.full((N, N, N), SENTINEL)
    with _solver(N, False, bc) as s:
        s.upload(MG3D_D, q, d)
        del d
        for kind in ("exp", "sinh"):
            u = _w_field(N, kind, 514)
            s.upload(MG3D_U, q, u)
            s.upload(MG3D_R, q, sentinel)
            want_n = s.residual(q, store=True)
            want = s.download_tensor(MG3D_R, q)
            assert int((want == SENTINEL).sum()) == N ** 3 - (N - 2) * N * (N - 2)
            tidx = tuple(torch.from_numpy(i).to(want.device) for i in idx)
            lin = want[tidx].cpu().numpy()
            s.nl_setup(kind, 0.0, BETA, UREF)
            s.upload(MG3D_R, q, sentinel)
            n = s.nl_residual(store=True)
            got = s.download_tensor(MG3D_R, q)
            assert torch.equal(got.view(torch.int64), want.view(torch.int64)), kind
            assert n == want_n
            del got, want
            s.nl_setup(kind, G0, BETA, UREF)
            nF = s.nl_residual(store=True)
            F = s.download_tensor(MG3D_R, q)[tidx].cpu().numpy()
            norms, info = s.nl_solve(max_newton=0)
            assert norms[0] == nF
            S = s.get_shift_field(q).reshape(N, N, N)[idx]
            s.set_shift_field(None)
            wF, wS = _check_nonlinear(kind, u[idx], lin, None, F, S, np.zeros(len(F), dtype=bool))
            print("513^3 sample, largest error in units of 2^-52 relative (F's function part, s):", kind, wF, wS)


# ------------------------------------------------------------------------------------------------- 3 the composition
def _pb_fields(N, coef, bc):
    axes, faces = BCS[bc]
    term, _, f, ustar = NL.pb_start(N, 4.0)
    u0 = ustar.copy()
    u0[NR.unknown_mask(N, axes, faces)] = 0.
    return u0, f


@gpu
@pytest.mark.parametrize("method", ["vcycles", "wpcg"])
@pytest.mark.parametrize("N,coef,bc", [(N, coef, bc) for N in (17, 33) for coef in (False, True) for bc in ("dirichlet", "f22")])
def test_one_newton_step_is_the_existing_calls_composed(N, coef, bc, method):
    """eps jumps by 10 in a ball here, not by 100 as elsewhere in this file: with 100 and Neumann faces two V-cycles are too
    inexact a solve for the full step -- the restatement halves once there, and so does the device -- and this test is about
    the step lambda = 1"""
    axes, faces = BCS[bc]
    L = SIZES[N][1]
    q = L - 1
    unk = NR.unknown_mask(N, axes, faces)
    u0, f = _pb_fields(N, coef, bc)
    cycles, rtol_lin = (2, 0.0) if method == "vcycles" else (3, 1e-2)
    with _solver(N, coef, bc, jump=10.) as A, _solver(N, coef, bc, jump=10.) as B:
        A.nl_setup("sinh", 4.0, 1.0, 0.0)
        A.upload(MG3D_U, q, u0)
        A.upload(MG3D_D, q, f)
        norms0, info0 = A.nl_solve(max_newton=0)
        assert A.has_shift_field() and info0["iterations"] == 0 and not info0["converged"] and len(norms0) == 1
        assert _same_bits(A.download(MG3D_U, q), u0) and _same_bits(A.download(MG3D_D, q), f)
        s0 = A.get_shift_field(q).reshape(N, N, N)
        assert (s0[unk] >= 4.0).all()
        for l, want in enumerate(SF.restrict_field(s0, L, axes, faces)):
            assert _same_bits(A.get_shift_field(l), want), l
        A.zero(MG3D_R, q)
        n0 = A.nl_residual(store=True)
        F0 = A.download(MG3D_R, q)
        assert n0 == norms0[0] == info0["norm0"]
        # context B: the caller's route through existing calls
        B.set_shift_field(s0)
        B.upload(MG3D_D, q, F0)
        B.zero(MG3D_U, q)
        if method == "vcycles":
            B.vcycles(cycles)
        else:
            B.wpcg_solve(rtol_lin, 0.0, cycles)
        delta = B.download(MG3D_U, q).reshape(N, N, N)
        norms, info = A.nl_solve(max_newton=1, cycles=cycles, method=method, rtol_lin=rtol_lin)
        got = A.download(MG3D_U, q).reshape(N, N, N)
        assert _same_bits(got[unk], u0[unk] + delta[unk])
        assert _same_bits(got[~unk], u0[~unk])
        assert _same_bits(A.download(MG3D_D, q), f)
        assert info["iterations"] == 1 and info["halvings"] == 0 and info["last_lambda"] == 1.0 and len(norms) == 2
        assert norms[0] == n0 and norms[1] == info["norm"] == A.nl_residual() and norms[1] < norms[0]
        assert info["linear_iterations"] == cycles if method == "vcycles" else 1 <= info["linear_iterations"] <= cycles
        assert A.has_shift_field()


# ------------------------------------------------------------------------------------------------- 4 whole solves
@functools.lru_cache(maxsize=None)
def _boltzmann_reference(N, beta):
    """the same discrete system solved on the CPU to 1e-12"""
    term, u0, d = NL.boltzmann_problem(N, 50.0, beta)
    u, norms, info = NL.solve(NL.Problem(5, SIZES[N][1], term), u0, d, max_newton=60, cycles=6, rtol=1e-12, max_halvings=20)
    assert info["converged"], norms
    u.setflags(write=False)
    return u


def _armijo(norms, info, max_halvings):
    """every accepted norm below its predecessor by the Armijo factor: of the step's own lambda where the call reports it
    (the last step), of the smallest lambda the call may have taken elsewhere"""
    for k in range(1, len(norms)):
        lam = info["last_lambda"] if k == len(norms) - 1 else 0.5 ** max_halvings
        assert norms[k] < (1.0 - 1e-4 * lam) * norms[k - 1], (k, norms)


@gpu
@pytest.mark.parametrize("N", [17, 33])
@pytest.mark.parametrize("beta", [1.0, 10.0])
def test_boltzmann_electrons(N, beta):
    q = SIZES[N][1] - 1
    term, u0, d = NL.boltzmann_problem(N, 50.0, beta)
    max_newton, max_halvings = NL.caps(N, beta)
    with _solver(N, False, "dirichlet") as s:
        s.nl_setup("exp", 50.0, beta, 0.0)
        s.upload(MG3D_U, q, u0)
        s.upload(MG3D_D, q, d)
        norms, info = s.nl_solve(max_newton=max_newton, cycles=2, rtol=1e-8, max_halvings=max_halvings)
        u = s.download(MG3D_U, q).reshape(N, N, N)
        assert _same_bits(s.download(MG3D_D, q), d) and s.has_shift_field()
    print(N, beta, info, list(norms))
    assert info["converged"] and info["iterations"] <= max_newton and len(norms) == info["iterations"] + 1
    assert info["halvings"] <= info["iterations"] * max_halvings and info["linear_iterations"] == 2 * info["iterations"]
    assert norms[-1] == info["norm"] <= 1e-8 * info["norm0"] and norms[0] == info["norm0"]
    _armijo(norms, info, max_halvings)
    F, _ = NL.evaluate(u, d, None, 1.0 / (N - 1), 0.0, 0, 0, None, term)
    assert abs(NL.norm(F) - info["norm"]) <= 1e-10 * info["norm0"]
    ref = _boltzmann_reference(N, beta)
    dist = float(np.sqrt(((u - ref) ** 2).sum()))
    print("distance to the CPU solution", dist, "bound", info["norm"] / NL.lambda_min(N))
    assert dist <= info["norm"] / NL.lambda_min(N)


@gpu
def test_poisson_boltzmann_error_is_the_restatements():
    N = 33
    q = SIZES[N][1] - 1
    term, u0, f, ustar = NL.pb_start(N, 4.0)
    want_u, _, want_info = NL.solve(NL.Problem(5, SIZES[N][1], term), u0, f, max_newton=12, cycles=3, rtol=1e-11)
    want_err = float(np.abs(want_u - ustar).max())
    assert want_info["converged"] and want_info["halvings"] == 0 and want_err < 5e-3
    with _solver(N, False, "dirichlet") as s:
        s.nl_setup("sinh", 4.0)
        s.upload(MG3D_U, q, u0)
        s.upload(MG3D_D, q, f)
        norms, info = s.nl_solve(max_newton=want_info["iterations"] + 2, cycles=3, rtol=1e-11, max_halvings=1)
        u = s.download(MG3D_U, q).reshape(N, N, N)
    err = float(np.abs(u - ustar).max())
    print(info, "error", err, "CPU error", want_err)
    assert info["converged"] and info["halvings"] == 0
    assert abs(err - want_err) <= 1e-6 * want_err


def _caps_of(P, u0, d, **kw):
    """the caps of a case outside _nl_ref.BOLTZMANN_NEEDS, from the restatement's own run: iterations + 2, the largest
    halving count + 1"""
    _, _, info = NL.solve(P, u0, d, max_newton=40, max_halvings=20, **kw)
    assert info["converged"], info
    return info["iterations"] + 2, max(info["halvings_per_step"] + [0]) + 1


@gpu
def test_weight_zero_inside_a_conductor_and_on_half_the_box():
    """Boltzmann electrons at 17^3 around a grounded ball (a mask), the electrons confined to the half x < 1/2: g = 0 inside
    the conductor and on the other half, where the equation is Poisson's"""
    N, q = 17, 2
    term, u0, d = NL.boltzmann_problem(N, 50.0, 1.0)
    mask = _ball(N, 0)
    g = np.ones((N, N, N))
    g[N // 2:, :, :] = 0.
    g[mask != 0] = 0.
    term.g = g
    P = NL.Problem(5, 3, term, mask=mask)
    max_newton, max_halvings = _caps_of(P, u0, d, cycles=2)
    with _solver(N, False, "dirichlet", masked=True) as s:
        s.nl_setup("exp", 50.0, 1.0, 0.0)
        s.nl_set_weight(g)
        s.upload(MG3D_U, q, u0)
        s.upload(MG3D_D, q, d)
        norms, info = s.nl_solve(max_newton=max_newton, cycles=2, max_halvings=max_halvings)
        u = s.download(MG3D_U, q).reshape(N, N, N)
        S = s.get_shift_field(q).reshape(N, N, N)
    print(info, list(norms))
    assert info["converged"]
    _armijo(norms, info, max_halvings)
    assert np.all(S[g == 0.] == 0.) and np.all(S[1:-1, 1:-1, 1:-1][g[1:-1, 1:-1, 1:-1] > 0.] > 0.)
    assert _same_bits(u[mask != 0], u0[mask != 0])
    F, _ = P.evaluate(u, d)
    assert abs(NL.norm(F) - info["norm"]) <= 1e-10 * info["norm0"]


@gpu
def test_all_neumann_box_by_wpcg():
    """every face a Neumann face, sigma = 0: the context alone is singular (its coarse solve pins a point, wpcg projects),
    the linearisation A - s with s > 0 is not -- the solve converges, and with g0 = 0 it is refused"""
    N, q = 17, 2
    term, u0, d = NL.boltzmann_problem(N, 50.0, 1.0)
    d = 0.01 * d
    P = NL.Problem(5, 3, term, faces=63)
    kw = dict(cycles=8, method="wpcg", rtol_lin=1e-3)
    max_newton, max_halvings = _caps_of(P, u0, d, **kw)
    with _solver(N, False, "f63") as s:
        s.upload(MG3D_U, q, u0)
        s.upload(MG3D_D, q, d)
        s.nl_setup("exp", 0.0, 1.0, 0.0)
        with pytest.raises(M.Mg3dError) as e:
            s.nl_solve(max_newton=3)
        assert e.value.code == MG3D_ERR_STATE and "singular" in str(e.value) and not s.has_shift_field()
        s.nl_setup("exp", 50.0, 1.0, 0.0)
        s.nl_set_weight(np.zeros((N, N, N)))
        with pytest.raises(M.Mg3dError) as e:
            s.nl_solve(max_newton=3)
        assert e.value.code == MG3D_ERR_STATE and not s.has_shift_field()
        s.nl_set_weight(None)
        norms, info = s.nl_solve(max_newton=max_newton, max_halvings=max_halvings, **kw)
        u = s.download(MG3D_U, q).reshape(N, N, N)
    print(info, list(norms))
    assert info["converged"] and 0 < info["linear_iterations"] <= 8 * info["iterations"]
    _armijo(norms, info, max_halvings)
    F, _ = P.evaluate(u, d)
    assert abs(NL.norm(F) - info["norm"]) <= 1e-10 * info["norm0"]


# ----------------------------------------------------------------------------- 5 behind a cycle that has run ahead
@gpu
@pytest.mark.parametrize("legs", [1, 0])
def test_entry_behind_a_cycle_that_has_run_ahead(legs):
    """161^3 (c = 6, L = 6): vcycles(1) and then a single vcycle(), which ends with the launch that begins the next cycle
    (one launch per leg, or the carried cycles with legs = 0); nl_solve finishes that cycle first -- its u equals, bit for
    bit, that of a context given the same u and d by upload"""
    N = 161
    c, L = SIZES[N]
    q = L - 1
    _, u0, f, _ = NL.pb_start(N, 4.0)

    def cycled():
        s = M.Solver(c, L, 2)
        s.set_option("legs", legs)
        s.get_details()
        s.nl_setup("sinh", 4.0)
        s.upload(MG3D_U, q, u0)
        s.upload(MG3D_D, q, f)
        s.vcycles(1)
        s.vcycle()
        return s

    with cycled() as A, cycled() as B, M.Solver(c, L, 2) as Cx:
        normsA, infoA = A.nl_solve(max_newton=1)
        ub = B.download(MG3D_U, q)
        Cx.set_option("legs", legs)
        Cx.get_details()
        Cx.nl_setup("sinh", 4.0)
        Cx.upload(MG3D_U, q, ub)
        Cx.upload(MG3D_D, q, f)
        normsC, infoC = Cx.nl_solve(max_newton=1)
        assert infoA == infoC and list(normsA) == list(normsC) and infoA["iterations"] == 1
        assert _same_bits(A.download(MG3D_U, q), Cx.download(MG3D_U, q))
        assert _same_bits(A.download(MG3D_D, q), f)


# ------------------------------------------------------------------------------------------- 6 state and arguments
def _raw_solve(s, max_newton=2, method=0, cycles=2, rtol_lin=1e-2, rtol=1e-8, atol=0.0, max_halvings=10):
    return s.L.mg3d_nl_solve(s._h, max_newton, method, cycles, rtol_lin, rtol, atol, max_halvings, None, None)


def _snapshot(s, q):
    return (s.download(MG3D_U, q), s.download(MG3D_D, q), s.has_shift_field(),
            s.get_shift_field(q) if s.has_shift_field() else None)


def _assert_untouched(s, q, snap):
    now = _snapshot(s, q)
    assert _same_bits(now[0], snap[0]) and _same_bits(now[1], snap[1]) and now[2] == snap[2]
    if snap[2]:
        assert _same_bits(now[3], snap[3])


@gpu
def test_state_and_arguments():
    N, q = 17, 2
    term, u0, d = NL.boltzmann_problem(N, 50.0, 1.0)
    nan, inf = float("nan"), float("inf")
    with _solver(N, False, "dirichlet") as s, _solver(N, False, "dirichlet") as plain:
        for t in (s, plain):
            t.upload(MG3D_U, q, u0)
            t.upload(MG3D_D, q, d)
        snap = _snapshot(s, q)
        # before mg3d_nl_setup
        assert _raw_solve(s) == MG3D_ERR_STATE and b"mg3d_nl_setup" in s.L.mg3d_last_error()
        assert s.L.mg3d_nl_residual(s._h, 0, None) == MG3D_ERR_STATE
        # mg3d_nl_setup: bad arguments change nothing
        for bad in ((2, 1., 1., 0.), (-1, 1., 1., 0.), (0, -1., 1., 0.), (0, nan, 1., 0.), (0, inf, 1., 0.), (0, 1., 0., 0.),
                    (0, 1., -2., 0.), (0, 1., inf, 0.), (0, 1., 1., nan), (0, 1., 1., inf)):
            assert s.L.mg3d_nl_setup(s._h, *bad) == MG3D_ERR_ARG, bad
        assert _raw_solve(s) == MG3D_ERR_STATE  # (still not set up)
        s.nl_setup("exp", 50.0, 1.0, 0.0)
        n_before = s.nl_residual()
        assert s.L.mg3d_nl_setup(s._h, 1, -3., 1., 0.) == MG3D_ERR_ARG and s.nl_residual() == n_before
        # the weight: entries checked as the screening field's
        g = np.ones((N, N, N))
        s.nl_set_weight(0.5 * g)
        n_half = s.nl_residual()
        assert n_half != n_before
        for value in (-1e-300, nan, inf):
            badg = g.copy()
            badg[3, 4, 5] = value
            with pytest.raises(M.Mg3dError) as e:
                s.nl_set_weight(badg)
            assert e.value.code == MG3D_ERR_ARG and f"g[{(3 * N + 4) * N + 5}]" in str(e.value)
            with pytest.raises(M.Mg3dError) as e:
                s.nl_set_weight_tensor(torch.from_numpy(badg).to("cuda:0"))
            assert e.value.code == MG3D_ERR_ARG
            assert s.nl_residual() == n_half
        s.nl_set_weight(None)
        assert s.nl_residual() == n_before
        # mg3d_nl_solve: bad arguments change nothing
        for kw in (dict(max_newton=-1), dict(method=2), dict(method=-1), dict(cycles=0), dict(max_halvings=-1), dict(rtol=-1.),
                   dict(rtol=nan), dict(atol=inf), dict(atol=-1.), dict(method=1, rtol_lin=-1.), dict(method=1, rtol_lin=nan)):
            assert _raw_solve(s, **kw) == MG3D_ERR_ARG, kw
            assert b"mg3d_nl_solve" in s.L.mg3d_last_error()
        _assert_untouched(s, q, snap)
        # a caller's screening field is refused, and stays
        field = SF.smooth_field(N, 3.0)
        s.set_shift_field(field)
        snap_f = _snapshot(s, q)
        assert _raw_solve(s) == MG3D_ERR_STATE and b"screening field" in s.L.mg3d_last_error()
        _assert_untouched(s, q, snap_f)
        plain.set_shift_field(field)
        assert _same_bits(s.vcycles(1), plain.vcycles(1)) and _same_bits(s.download(MG3D_U, q), plain.download(MG3D_U, q))
        s.set_shift_field(None)
        plain.set_shift_field(None)
        for t in (s, plain):
            t.upload(MG3D_U, q, u0)
        # a line search that fails: max_halvings = 0 (tests/test_nl_ref_host.py: the restatement refuses the full step)
        norms, info = s.nl_solve(max_newton=5, cycles=2, max_halvings=0)
        assert info["iterations"] == 0 and not info["converged"] and info["halvings"] == 0 and info["last_lambda"] == 0.0
        assert len(norms) == 1 and norms[0] == info["norm"] == info["norm0"] == n_before
        assert _same_bits(s.download(MG3D_U, q), u0) and _same_bits(s.download(MG3D_D, q), d) and s.has_shift_field()
        first = s.get_shift_field(q)
        assert np.all(first.reshape(N, N, N)[1:-1, 1:-1, 1:-1] == 50.0)  # s(x) at x = 0: g0*beta*exp(0)
        # the context is usable: a second solve overwrites the first one's field
        mn, mh = NL.caps(N, 1.0)
        norms, info = s.nl_solve(max_newton=mn, cycles=2, max_halvings=mh)
        assert info["converged"] and s.has_shift_field() and not _same_bits(s.get_shift_field(q), first)
        # ... and after set_shift_field(None) a cycle gives the bits of a context that never had a field
        s.set_shift_field(None)
        assert not s.has_shift_field()
        s.upload(MG3D_U, q, u0)
        assert _same_bits(s.vcycles(2), plain.vcycles(2)) and _same_bits(s.download(MG3D_U, q), plain.download(MG3D_U, q))
    # no coarse factor; a factor that mg3d_ctx_build_coarse did not build; a context after mg3d_es_setup
    with _solver(N, False, "dirichlet", build=False) as s:
        s.nl_setup("exp", 50.0)
        s.upload(MG3D_U, q, u0)
        s.upload(MG3D_D, q, d)
        snap = _snapshot(s, q)
        assert _raw_solve(s) == MG3D_ERR_STATE and b"coarse factor" in s.L.mg3d_last_error()
        _assert_untouched(s, q, snap)
    es = M.EsParams.default()
    with M.Solver(5, 3, 2, grid_length=es.length) as s:
        s.es_setup(es)
        s.nl_setup("exp", 50.0)
        assert _raw_solve(s) == MG3D_ERR_STATE and b"mg3d_es_setup" in s.L.mg3d_last_error()
        assert not s.has_shift_field()
