"""The variable-coefficient operator on i-slabs (mg3d_dist_set_coefficient), verified on ONE GPU through the loopback
transport (all ranks virtual, in this process).  Every result is compared with a single-domain Solver given the same eps
and sigma -- itself pinned bit for bit to the numpy reference of tests/_coef_ref.py by tests/test_gpu_coef.py: grid values
bit for bit (sign bits included), norms to the summation tolerance, the last one against the exactly rounded sum."""
import numpy as np
import pytest

import _coef_ref as R
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U

pytestmark = pytest.mark.gpu

MG3D_ERR_ARG, MG3D_ERR_STATE = 1, 5
EXACT_NORM_RTOL = 1e-13


def _n(c, L):
    return (c - 1) * (1 << (L - 1)) + 1


def _same_bits(a, b):
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _single(c, L, nu, sigma, eps, calls=(1, 2)):
    """norms and (u of every level, d of every level below the top) of a Solver after vcycles(k) for k in calls"""
    with M.Solver(c, L, nu) as s:
        s.set_shift(sigma)
        s.set_coefficient(eps)
        s.setup_test_problem()
        norms = np.concatenate([s.vcycles(k) for k in calls])
        return norms, [s.download(MG3D_U, l) for l in range(L)], [s.download(MG3D_D, l) for l in range(L - 1)]


def _dist(c, L, nu, P, sigma, eps, calls=(1, 2), keep=False):
    with M.DistSolver(c, L, nu, nranks=P) as d:
        d.set_shift(sigma)
        d.set_coefficient(eps)
        assert d.has_coefficient()
        if keep:
            d.set_keep_residual(True)
        d.setup_test_problem()
        norms = np.concatenate([d.vcycles(k) for k in calls])
        assert d.carried_cycles() == 0 and d.legs_cycles() == 0
        u, dd = [d.download(MG3D_U, l) for l in range(L)], [d.download(MG3D_D, l) for l in range(L - 1)]
        exact = R.exact_residual_norm(u[-1], d.download(MG3D_D, L - 1), eps, d.N, d.h, sigma)
        return norms, u, dd, exact, d.first_level


# one shape per rank count whose slabs hold 16 planes at least (8: every level that can be split is)
_SHAPES = {2: (5, 5), 3: (3, 6), 4: (5, 5), 8: (9, 5)}


@pytest.mark.parametrize("min_planes", [8, 16])
@pytest.mark.parametrize("field", sorted(R.FIELDS))
@pytest.mark.parametrize("sigma", [0.0, 1e3])
@pytest.mark.parametrize("nu", [1, 2, 3])
@pytest.mark.parametrize("P", [2, 3, 4, 8])
def test_parity(monkeypatch, P, nu, sigma, field, min_planes):
    c, L = _SHAPES[P]
    if ((c - 1) << (L - 1)) // P < max(min_planes, 2 * nu + 2):
        pytest.skip("no level gives every rank that many planes")
    monkeypatch.setenv("MG3D_SLAB_MIN_PLANES", str(min_planes))
    eps = R.FIELDS[field](_n(c, L))
    want_norms, want_u, want_d = _single(c, L, nu, sigma, eps)
    norms, u, dd, exact, _ = _dist(c, L, nu, P, sigma, eps)
    for l in range(L):
        assert _same_bits(u[l], want_u[l]), f"u level {l}"
    for l in range(L - 1):
        assert _same_bits(dd[l], want_d[l]), f"d level {l}"
    np.testing.assert_allclose(norms, want_norms, rtol=1e-11, atol=0)
    assert norms[-1] == pytest.approx(exact, rel=EXACT_NORM_RTOL)


# coarse grids off the 2^k+1 ladder, every rank at least 8 planes on the levels it splits: 97^3 on 3 ranks, 81^3 on 2,
# on 4 and on 3 (owned planes 12, 14, 15 on the first split level, 41^3)
_OFF_LADDER = [(7, 5, 3, "exp"), (11, 4, 2, "ball"), (6, 5, 4, "smooth"), (6, 5, 3, "exp")]


@pytest.mark.parametrize("sigma", [0.0, 1e3])
@pytest.mark.parametrize("nu", [1, 3])
@pytest.mark.parametrize("c,L,P,field", _OFF_LADDER)
def test_parity_off_ladder(monkeypatch, c, L, P, field, nu, sigma):
    monkeypatch.setenv("MG3D_SLAB_MIN_PLANES", "8")
    eps = R.FIELDS[field](_n(c, L))
    want_norms, want_u, want_d = _single(c, L, nu, sigma, eps)
    norms, u, dd, exact, first = _dist(c, L, nu, P, sigma, eps)
    assert 1 <= first < L, first
    for l in range(L):
        assert _same_bits(u[l], want_u[l]), f"u level {l}"
    for l in range(L - 1):
        assert _same_bits(dd[l], want_d[l]), f"d level {l}"
    np.testing.assert_allclose(norms, want_norms, rtol=1e-11, atol=0)
    assert norms[-1] == pytest.approx(exact, rel=EXACT_NORM_RTOL)


@pytest.mark.parametrize("policy", ["coarse_gather", "no_overlap", "keep_residual"])
@pytest.mark.parametrize("c,L,nu,P,min_planes", [(5, 5, 2, 4, 8), (9, 5, 2, 8, 16), (3, 6, 1, 3, 8), (9, 5, 3, 2, 16)])
def test_policies_same_bits(monkeypatch, policy, c, L, nu, P, min_planes):
    """coarse levels on rank 0 only (right-hand side gathered, correction broadcast), every exchange on the compute stream,
    r kept: the bits of the default schedule and of the single domain"""
    monkeypatch.setenv("MG3D_SLAB_MIN_PLANES", str(min_planes))
    eps, sigma = R.ball_eps(_n(c, L)), 1e3
    want_norms, want_u, want_d = _single(c, L, nu, sigma, eps)
    base = _dist(c, L, nu, P, sigma, eps)
    if policy == "coarse_gather":
        monkeypatch.setenv("MG3D_COARSE_GATHER", "1")
    if policy == "no_overlap":
        monkeypatch.setenv("MG3D_NO_OVERLAP", "1")
    norms, u, dd, exact, ld = _dist(c, L, nu, P, sigma, eps, keep=policy == "keep_residual")
    # (rank 0 alone holds the replicated levels below the broadcast correction with coarse_gather)
    lo = ld - 1 if policy == "coarse_gather" else 0
    for l in range(lo, L):
        assert _same_bits(u[l], want_u[l]) and _same_bits(u[l], base[1][l]), f"u level {l}"
    for l in range(max(lo, ld), L - 1):
        assert _same_bits(dd[l], want_d[l]), f"d level {l}"
    np.testing.assert_allclose(norms, want_norms, rtol=1e-11, atol=0)
    np.testing.assert_allclose(norms, base[0], rtol=1e-13, atol=0)
    assert norms[-1] == pytest.approx(exact, rel=EXACT_NORM_RTOL)


@pytest.mark.parametrize("c,L,P,cycles,field", [(9, 6, 4, 3, "ball"), (9, 7, 8, 3, "exp")])
def test_full_size(c, L, P, cycles, field):
    """257^3 on 4 ranks and 513^3 on 8, default options: the finest u bit for bit"""
    eps, sigma = R.FIELDS[field](_n(c, L)), 0.0
    with M.Solver(c, L, 2) as s:
        s.set_coefficient(eps)
        s.setup_test_problem()
        want_norms = s.vcycles(cycles)
        want_u = s.download(MG3D_U, L - 1)
    with M.DistSolver(c, L, 2, nranks=P) as d:
        d.set_coefficient(eps)
        d.setup_test_problem()
        norms = d.vcycles(cycles)
        assert d.carried_cycles() == 0 and d.legs_cycles() == 0
        u = d.download(MG3D_U, L - 1)
    del eps
    assert _same_bits(u, want_u)
    np.testing.assert_allclose(norms, want_norms, rtol=1e-11, atol=0)


@pytest.mark.parametrize("legs", ["1", "0"])
def test_schedules_bypassed_then_restored(monkeypatch, legs):
    """257^3, V(2,2): the one-launch legs (default) or the carried cycles (legs = 0) advance on the constant operator, stand
    still while eps is set, and advance again after set_coefficient(None) -- whose cycles then equal a fresh DistSolver that
    never had eps, started from the same u.  The constant cycles before the switch leave red_tail set."""
    monkeypatch.setenv("MG3D_LEGS", legs)
    c, L, P = 9, 6, 4
    eps = R.exp_eps(_n(c, L))
    count = (lambda d: d.legs_cycles()) if legs == "1" else (lambda d: d.carried_cycles())
    with M.Solver(c, L, 2) as s:
        s.setup_test_problem()
        s.vcycles(3)
        s.set_coefficient(eps)
        want_coef = s.vcycles(3)
        want_mid = s.download(MG3D_U, L - 1)
    with M.DistSolver(c, L, 2, nranks=P) as d:
        d.setup_test_problem()
        d.vcycles(3)
        n0 = count(d)
        assert n0 == 2
        d.set_coefficient(eps)
        coef = d.vcycles(3)
        assert count(d) == n0 and d.legs_cycles() + d.carried_cycles() == n0
        mid = d.download(MG3D_U, L - 1)
        d.set_coefficient(None)
        assert not d.has_coefficient()
        after = d.vcycles(3)
        assert count(d) == n0 + 2
        u_after = d.download(MG3D_U, L - 1)
    assert _same_bits(mid, want_mid)
    np.testing.assert_allclose(coef, want_coef, rtol=1e-11, atol=0)
    with M.DistSolver(c, L, 2, nranks=P) as f:
        f.setup_test_problem()
        f.upload(MG3D_U, L - 1, mid)
        fresh = f.vcycles(3)
        assert count(f) == 2
        assert _same_bits(f.download(MG3D_U, L - 1), u_after)
    assert np.array_equal(fresh, after)


def test_changing_eps(monkeypatch):
    """cycles with eps_A, set_coefficient(eps_B), more cycles: the same sequence on a Solver, bit for bit"""
    monkeypatch.setenv("MG3D_SLAB_MIN_PLANES", "8")
    c, L, nu, P, sigma = 5, 5, 2, 4, 1e3
    N = _n(c, L)
    ea, eb = R.smooth_eps(N), R.ball_eps(N)
    res = []
    for mk in (lambda: M.Solver(c, L, nu), lambda: M.DistSolver(c, L, nu, nranks=P)):
        with mk() as x:
            x.set_shift(sigma)
            x.set_coefficient(ea)
            x.setup_test_problem()
            n1 = x.vcycles(2)
            x.set_coefficient(eb)
            n2 = x.vcycles(3)
            res.append((np.concatenate([n1, n2]), [x.download(MG3D_U, l) for l in range(L)], x.coefficient(L - 2)))
    for l in range(L):
        assert _same_bits(res[0][1][l], res[1][1][l]), f"u level {l}"
    assert _same_bits(res[0][2], res[1][2])
    np.testing.assert_allclose(res[1][0], res[0][0], rtol=1e-11, atol=0)


@pytest.mark.parametrize("c,L,P,min_planes", [(3, 6, 3, 8), (9, 5, 8, 16), (5, 5, 2, 16)])
def test_coefficient_of_every_level(monkeypatch, c, L, P, min_planes):
    monkeypatch.setenv("MG3D_SLAB_MIN_PLANES", str(min_planes))
    eps = R.ball_eps(_n(c, L)) * R.exp_eps(_n(c, L))
    with M.Solver(c, L, 2) as s, M.DistSolver(c, L, 2, nranks=P) as d:
        s.set_coefficient(eps)
        d.set_coefficient(eps)
        assert 1 <= d.first_level < L
        want = R.inject(eps, L)
        for l in range(L):
            got = d.coefficient(l)
            assert got.shape == (d.level_n(l),) * 3
            assert _same_bits(got, s.coefficient(l)) and _same_bits(got, want[l]), f"level {l}"


def test_rules():
    c, L, nu, P = 5, 5, 2, 4
    N = _n(c, L)
    ea = R.exp_eps(N)
    with M.DistSolver(c, L, nu, nranks=P) as d:
        with pytest.raises(M.Mg3dError) as e:
            d.coefficient(L - 1)
        assert e.value.code == MG3D_ERR_STATE
        with pytest.raises(TypeError):
            d.set_coefficient(ea.astype(np.float32))
        with pytest.raises(ValueError):
            d.set_coefficient(ea[:-1])
        with pytest.raises(ValueError):
            d.set_coefficient(np.ones((N, N, N + 1)))
        for bad in (0.0, -1.0, np.nan, np.inf):
            x = ea.copy()
            x[N // 2, 3, 4] = bad
            with pytest.raises(M.Mg3dError) as e:
                d.set_coefficient(x)
            assert e.value.code == MG3D_ERR_ARG
            assert not d.has_coefficient()
        d.set_coefficient(ea)
        before = [d.coefficient(l) for l in range(L)]
        d.setup_test_problem()
        d.vcycles(1)
        u0 = d.download(MG3D_U, L - 1)
        for bad in (0.0, -1.0, np.nan, np.inf):
            x = R.ball_eps(N)
            x[1, N - 2, 0] = bad
            with pytest.raises(M.Mg3dError) as e:
                d.set_coefficient(x)
            assert e.value.code == MG3D_ERR_ARG
            assert d.has_coefficient()
            for l in range(L):
                assert _same_bits(d.coefficient(l), before[l])
        with pytest.raises(M.Mg3dError) as e:
            d.coefficient(L)
        assert e.value.code == MG3D_ERR_ARG
        got = d.vcycles(2)
        got_u = d.download(MG3D_U, L - 1)
    with M.DistSolver(c, L, nu, nranks=P) as f:  # the same cycles without the failed calls in between
        f.set_coefficient(ea)
        f.setup_test_problem()
        f.vcycles(1)
        assert _same_bits(f.download(MG3D_U, L - 1), u0)
        assert np.array_equal(f.vcycles(2), got)
        assert _same_bits(f.download(MG3D_U, L - 1), got_u)


def test_single_rank_communicator_agreement(monkeypatch):
    """MG3D_FORCE_COMM=1 gives one rank a real RCCL communicator: set_coefficient runs its agreement all-reduce (also on a
    refused array and on the way back to the constant operator), and the cycles equal the loopback run"""
    c, L, nu, sigma = 5, 5, 2, 1e3
    eps = R.smooth_eps(_n(c, L))
    with M.DistSolver(c, L, nu, nranks=1) as d:
        d.set_shift(sigma)
        d.set_coefficient(eps)
        d.setup_test_problem()
        want = d.vcycles(3)
        want_u = d.download(MG3D_U, L - 1)
    monkeypatch.setenv("MG3D_FORCE_COMM", "1")
    with M.DistSolver(c, L, nu, rank=0, nranks=1, unique_id=M.DistSolver.unique_id()) as d:
        assert d.comm_info()[0] == 1
        bad = eps.copy()
        bad[2, 2, 2] = np.nan
        with pytest.raises(M.Mg3dError) as e:
            d.set_coefficient(bad)
        assert e.value.code == MG3D_ERR_ARG and not d.has_coefficient()
        d.set_coefficient(eps)
        d.set_coefficient(None)
        d.set_shift(sigma)
        d.set_coefficient(eps)
        assert d.has_coefficient()
        d.setup_test_problem()
        got = d.vcycles(3)
        assert _same_bits(d.download(MG3D_U, L - 1), want_u)
    np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
