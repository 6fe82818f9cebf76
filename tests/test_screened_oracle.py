"""The screened twins of the C oracle (orc_*_shift in oracle/mg3d_oracle.c) without a GPU: bit for bit the numpy reference of
tests/_screened_ref.py on every level's u and d at any sigma, and at sigma = 0 the unshifted oracle and the golden vectors
of the compiled reference.  The GPU tests of the screened operator at 513^3 (too large for the numpy reference) check
against orc_run_problem_shift, so this file is what makes that check mean the same as the smaller ones."""
import hashlib
import os

import numpy as np
import pytest

import _oracle as O
import _screened_ref as S

V = np.load(os.path.join(O.GOLDEN, "vcycle.npz"))
G = np.load(os.path.join(O.GOLDEN, "operators.npz"))


@pytest.fixture(autouse=True)
def _one_thread():
    O.lib().orc_set_threads(1)


def _same_bits(a, b):
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _hierarchy(ref):
    """an oracle Hierarchy holding the reference's current state, level by level"""
    H = O.Hierarchy(ref.c, ref.L)
    for l in range(ref.L):
        H.u[l][:] = ref.flat("u", l)
        H.d[l][:] = ref.flat("d", l)
        H.r[l][:] = ref.flat("r", l)
    return H


def _random_start(ref, seed):
    """seeded random interior u and d on the finest level (boundary values of the test problem stay): no x <-> z symmetry"""
    rng = np.random.default_rng(seed)
    N = ref.N[-1]
    ref.setup_test_problem()
    ref.u[-1][1:-1, 1:-1, 1:-1] = rng.uniform(-1, 1, (N - 2,) * 3)
    ref.d[-1][1:-1, 1:-1, 1:-1] = rng.uniform(-1e3, 1e3, (N - 2,) * 3)


def _lu(c, h, sigma):
    A = np.zeros(c ** 6)
    O.lib().orc_coarse_matrix_shift(O.P(A), c, h, sigma)
    (O.lib().orc_lu_factor_banded if c > 9 else O.lib().orc_lu_factor)(O.P(A), c ** 3)
    return A


@pytest.mark.parametrize("N,h", [(3, 0.5), (5, 0.25), (9, 1.0 / 8), (9, 1.0 / 64)])
@pytest.mark.parametrize("sigma", [0.0, 1e-12, 1.0, 1e4])
def test_coarse_matrix_shift_is_the_reference(N, h, sigma):
    A = np.zeros(N ** 6)
    O.lib().orc_coarse_matrix_shift(O.P(A), N, h, sigma)
    assert A.tobytes() == S.coarse_matrix(N, h, sigma).tobytes()
    if sigma == 0.0:
        B = np.zeros(N ** 6)
        O.lib().orc_coarse_matrix(O.P(B), N, h)
        assert A.tobytes() == B.tobytes()


@pytest.mark.parametrize("N", [5, 9, 17, 33])
@pytest.mark.parametrize("sigma", [1e-12, 1.0, 1e4])
@pytest.mark.parametrize("post,iters", [(0, 1), (1, 2), (0, 3)])
def test_smoother_and_residual_are_the_reference(N, sigma, post, iters):
    rng = np.random.default_rng(N * 7 + iters)
    h = 1.0 / (N - 1)
    u = rng.uniform(-1, 1, N ** 3)
    d = rng.uniform(-1e3, 1e3, N ** 3)
    want = u.copy().reshape(N, N, N)
    (S.post_smooth if post else S.pre_smooth)(want, d.reshape(N, N, N), h, sigma, iters)
    (O.lib().orc_post_smooth_shift if post else O.lib().orc_pre_smooth_shift)(O.P(u), O.P(d), N, h, sigma, iters)
    assert _same_bits(u, want.reshape(-1))
    r = np.zeros(N ** 3)
    nrm = O.lib().orc_residual_shift(O.P(u), O.P(d), N, h, sigma, O.P(r))
    want_r = np.zeros((N, N, N))
    want_n = S.residual(want, d.reshape(N, N, N), h, sigma, want_r)
    assert _same_bits(r, want_r.reshape(-1))
    assert nrm == pytest.approx(want_n, rel=1e-13)  # sequential sum here, pairwise in numpy
    assert O.lib().orc_residual_shift(O.P(u), O.P(d), N, h, sigma, None) == nrm


@pytest.mark.parametrize("N", [5, 9, 17, 33])
def test_twins_at_sigma_zero_are_the_golden_operators(N):
    """sigma = 0: the golden smoother and residual vectors of the compiled reference, byte for byte"""
    h = 1.0 / (N - 1)
    for name, post, it in (("pre1", 0, 1), ("pre2", 0, 2), ("post1", 1, 1), ("post3", 1, 3)):
        v = G[f"sm_v0_{N}"].copy()
        (O.lib().orc_post_smooth_shift if post else O.lib().orc_pre_smooth_shift)(O.P(v), O.P(G[f"sm_d0_{N}"]), N, h, 0.0, it)
        assert v.tobytes() == G[f"sm_{name}_{N}"].tobytes(), name
    res = np.zeros(N ** 3)
    nrm = O.lib().orc_residual_shift(O.P(G[f"sm_v0_{N}"]), O.P(G[f"sm_d0_{N}"]), N, h, 0.0, O.P(res))
    assert res.tobytes() == G[f"res_r_{N}"].tobytes()
    assert nrm == G[f"res_norm_{N}"][0]


# sizes 17^3 .. 65^3, every nu, three sigmas; the non-2^k+1 coarse grids 6 and 7 too
VCYCLE_CASES = [(9, 2, 2), (5, 3, 1), (5, 3, 3), (3, 5, 2), (9, 3, 1), (9, 3, 3), (5, 5, 2), (9, 4, 2), (7, 3, 2), (6, 4, 3)]


@pytest.mark.parametrize("c,L,nu", VCYCLE_CASES)
@pytest.mark.parametrize("sigma", [1e-12, 1.0, 1e4])
@pytest.mark.parametrize("data", ["test", "random"])
def test_vcycle_shift_is_the_reference_on_every_level(c, L, nu, sigma, data):
    """three V-cycles through orc_vcycle_shift and through _screened_ref.Problem: u of every level, d below the top and r
    of every level bit for bit after each cycle, norms to the summation order"""
    ref = S.Problem(c, L, nu, sigma)
    if data == "test":
        ref.setup_test_problem()
    else:
        _random_start(ref, c * 100 + L * 10 + nu)
    H = _hierarchy(ref)
    LU = _lu(c, ref.h * (1 << (L - 1)), sigma)
    assert LU.tobytes() == ref.LU.tobytes()
    N = ref.N[-1]
    for cyc in range(3):
        got = O.lib().orc_vcycle_shift(H.ptrs(H.u), H.ptrs(H.d), H.ptrs(H.r), ref.h, sigma, L - 1, L, nu, N, O.P(LU))
        want = ref.vcycle()
        assert got == pytest.approx(want, rel=1e-13), cyc
        for l in range(L):
            assert _same_bits(H.u[l], ref.flat("u", l)), (cyc, "u", l)
            assert _same_bits(H.r[l], ref.flat("r", l)), (cyc, "r", l)
        for l in range(L - 1):
            assert _same_bits(H.d[l], ref.flat("d", l)), (cyc, "d", l)


@pytest.mark.parametrize("c,L,nu", [(5, 4, 2), (3, 5, 1), (9, 3, 3), (3, 6, 2)])
@pytest.mark.parametrize("sigma", [1e-12, 1.0, 1e4])
def test_fmg_initialize_shift_is_the_reference(c, L, nu, sigma):
    ref = S.Problem(c, L, nu, sigma)
    ref.setup_test_problem()
    H = _hierarchy(ref)
    LU = _lu(c, ref.h * (1 << (L - 1)), sigma)
    ref.fmg_initialize()
    O.lib().orc_fmg_initialize_shift(H.ptrs(H.u), H.ptrs(H.d), H.ptrs(H.r), c, L, nu, sigma, 1.0, O.P(LU))
    for l in range(L):
        assert _same_bits(H.u[l], ref.flat("u", l)), ("u", l)
    for l in range(L - 1):
        assert _same_bits(H.d[l], ref.flat("d", l)), ("d", l)


@pytest.mark.parametrize("c,L,nu,sigma", [(9, 3, 2, 10.0), (5, 5, 1, 1e4), (17, 2, 2, 1.0), (6, 4, 3, 1e-12)])
def test_run_problem_shift_is_the_reference(c, L, nu, sigma):
    """the driver the 513^3 GPU tests use: its u and norms are Problem's, its initial norm the l2 norm of d, and its grid
    values do not depend on the OpenMP thread count"""
    ref = S.Problem(c, L, nu, sigma)
    ref.setup_test_problem()
    want = ref.vcycles(3)
    norms, u, init, _ = O.run_problem_shift(c, L, nu, sigma, 3)
    assert _same_bits(u, ref.flat("u", L - 1))
    np.testing.assert_allclose(norms, want, rtol=1e-13)
    assert init == O.lib().orc_l2norm(O.P(ref.flat("d", L - 1)), ref.N[-1] ** 3)
    O.lib().orc_set_threads(4)
    n4, u4, _, _ = O.run_problem_shift(c, L, nu, sigma, 3)
    assert _same_bits(u4, u)
    np.testing.assert_allclose(n4, norms, rtol=1e-13)


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


@pytest.mark.parametrize("c,L,nu", [(3, 3, 1), (3, 5, 2), (5, 3, 3), (9, 2, 2), (5, 5, 2), (9, 5, 2)])
def test_run_problem_shift_at_zero_is_the_oracle_and_the_golden_history(c, L, nu):
    key = f"{c}_{L}_{nu}"
    cycles = len(V[f"norms_{key}"])
    norms, u, init, _ = O.run_problem_shift(c, L, nu, 0.0, cycles)
    want_norms, want_u, want_init, _ = O.run_problem(c, L, nu, cycles)
    assert u.tobytes() == want_u.tobytes()
    assert norms.tobytes() == want_norms.tobytes() and init == want_init
    assert init == V[f"init_{key}"][0]
    assert np.array_equal(_sha(u), V[f"usha_{key}"])
    np.testing.assert_allclose(norms, V[f"norms_{key}"], rtol=4e-16, atol=0)  # (see test_oracle_golden: sqrt of a square)


@pytest.mark.parametrize("c,L,nu", [(5, 4, 2), (3, 5, 1)])
def test_fmg_shift_at_zero_is_the_golden_start(c, L, nu):
    key = f"fmg_{c}_{L}_{nu}"
    H = O.Hierarchy(c, L)
    N, h = H.N[-1], 1.0 / (H.N[-1] - 1)
    LU = _lu(c, h * (1 << (L - 1)), 0.0)
    O.lib().orc_fill_boundary(O.P(H.d[-1]), N, h)
    O.lib().orc_fill_boundary(O.P(H.u[-1]), N, h)
    O.lib().orc_fmg_initialize_shift(H.ptrs(H.u), H.ptrs(H.d), H.ptrs(H.r), c, L, nu, 0.0, 1.0, O.P(LU))
    assert H.u[-1].tobytes() == V[f"u0_{key}"].tobytes()
    norms = [O.lib().orc_vcycle_shift(H.ptrs(H.u), H.ptrs(H.d), H.ptrs(H.r), h, 0.0, L - 1, L, nu, N, O.P(LU))
             for _ in range(3)]
    assert np.array_equal(np.array(norms), V[f"norms_{key}"])
    assert H.u[-1].tobytes() == V[f"u_{key}"].tobytes()


def test_sigma_changes_every_level():
    """the shift is not lost anywhere: sigma = 1e-12 at 65^3 differs from sigma = 0 (on the coarsest level dg != 6)"""
    c, L, nu = 9, 4, 2
    h0 = 1.0 / 8
    assert 6.0 + 1e-12 * h0 * h0 != 6.0 and 6.0 + 1e-12 * (h0 / 8) ** 2 == 6.0
    a, ua, _, _ = O.run_problem_shift(c, L, nu, 1e-12, 2)
    b, ub, _, _ = O.run_problem_shift(c, L, nu, 0.0, 2)
    assert not np.array_equal(ua, ub)
