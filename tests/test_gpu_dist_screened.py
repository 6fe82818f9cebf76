"""The screened operator on i-slabs (mg3d_dist_set_shift) through the loopback transport: every plan of tests/test_gpu_dist.py
-- plain, carried (SWEEP_TAP), one launch per leg with edge windows, red_tail across calls, coarse gather, no overlap,
keep-residual -- at P = 2, 3, 4, 8 and nu = 1, 2, 3 with sigma > 0, bit for bit against the single-domain Solver with the
same sigma and against the numpy reference of tests/_screened_ref.py on every distributed level; and 513^3 on 8, 4 and 2
slabs against the C oracle's screened twin."""
import numpy as np
import pytest

import _screened_ref as S
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U

from test_gpu_parity import norm_rtol
from test_gpu_screened_variants import SIGMA_513, _same_bits, exact_norm_513, oracle_513, reference, start_data

pytestmark = pytest.mark.gpu

EXACT_NORM_RTOL = 1e-13  # the slab path's reduction against the exactly rounded sum (tests/test_gpu_dist.py)
CALLS = (4, 1, 2)        # red_tail and carried state cross the calls


def _plan_env(monkeypatch, plan, min_planes, overlap, gather):
    monkeypatch.setenv("MG3D_SLAB_MIN_PLANES", str(min_planes))
    monkeypatch.setenv("MG3D_NO_OVERLAP", "0" if overlap else "1")
    if gather:
        monkeypatch.setenv("MG3D_COARSE_GATHER", "1")
    else:
        monkeypatch.delenv("MG3D_COARSE_GATHER", raising=False)
    monkeypatch.setenv("MG3D_CARRY_MIN", "66")
    monkeypatch.setenv("MG3D_LEGS_MIN", "66")
    monkeypatch.setenv("MG3D_NO_CARRY", "0" if plan == "carried" else "1")
    monkeypatch.setenv("MG3D_LEGS", "1" if plan == "legs" else "0")


def _load_dist(d, c, L, data):
    u, f, _ = start_data(c, L, data)
    d.setup_test_problem()  # (builds the coarse factor of the ranks' sigma)
    d.upload(MG3D_U, L - 1, u)
    d.upload(MG3D_D, L - 1, f)


def _load_single(s, c, L, data):
    u, f, _ = start_data(c, L, data)
    s.get_details()
    s.upload(MG3D_U, L - 1, u)
    s.upload(MG3D_D, L - 1, f)


def _exact_norm(d, L, sigma):
    return S.exact_residual_norm(d.download(MG3D_U, L - 1), d.download(MG3D_D, L - 1), d.N, d.h, sigma)


# (c, L, nu, P, min_planes, plan, overlap, coarse gather, keep residual, sigma, data)
CASES = [
    (9, 5, 2, 2, 16, "carried", 1, 0, 0, 10.0, "test"),
    (9, 5, 2, 8, 16, "carried", 0, 0, 0, 1.0, "random"),
    (5, 6, 2, 4, 8, "carried", 1, 0, 0, 1e-12, "test"),
    (3, 7, 2, 3, 16, "carried", 1, 0, 0, 1e4, "random"),
    (9, 5, 2, 8, 16, "legs", 1, 0, 0, 1.0, "random"),
    (9, 5, 2, 4, 8, "legs", 0, 0, 0, 1e4, "test"),
    (3, 7, 2, 3, 16, "legs", 1, 0, 0, 10.0, "test"),
    (6, 5, 2, 2, 16, "legs", 1, 0, 0, 1.0, "random"),
    (9, 5, 2, 2, 8, "plain", 1, 0, 0, 1e4, "random"),
    (9, 5, 1, 4, 8, "plain", 1, 0, 0, 1e4, "random"),
    (9, 5, 1, 8, 16, "legs", 0, 0, 0, 1.0, "test"),       # nu = 1: no per-leg plan, the plain one runs
    (9, 5, 3, 2, 16, "carried", 1, 0, 0, 1.0, "test"),    # nu = 3: no carried plan either
    (7, 5, 3, 3, 8, "plain", 0, 0, 0, 10.0, "random"),
    (5, 5, 1, 8, 8, "plain", 1, 0, 0, 1.0, "test"),
    (9, 5, 2, 8, 16, "plain", 1, 1, 0, 10.0, "random"),
    (9, 5, 3, 4, 8, "plain", 1, 1, 0, 1e4, "test"),
    (3, 6, 2, 3, 8, "legs", 1, 1, 0, 1.0, "random"),     # 65^3: neither fast plan, the plain one runs
    (9, 5, 2, 4, 16, "legs", 1, 1, 0, 1e4, "random"),
    (5, 6, 2, 2, 8, "carried", 0, 1, 0, 10.0, "test"),
    (9, 5, 2, 4, 8, "carried", 1, 0, 1, 1.0, "random"),   # keep-residual: the plain plan, r compared too
    (9, 5, 1, 2, 16, "plain", 0, 0, 1, 10.0, "test"),
    (6, 5, 3, 8, 8, "plain", 1, 0, 1, 1e4, "random"),
]


@pytest.mark.parametrize("c,L,nu,P,min_planes,plan,overlap,gather,keep,sigma,data", CASES)
def test_slabs_equal_the_single_domain_and_the_reference(monkeypatch, c, L, nu, P, min_planes, plan, overlap, gather, keep,
                                                         sigma, data):
    _plan_env(monkeypatch, plan, min_planes, overlap, gather)
    want = reference(c, L, nu, sigma, data, sum(CALLS))
    with M.Solver(c, L, nu) as s:
        s.set_shift(sigma)
        s.set_keep_residual(bool(keep))
        _load_single(s, c, L, data)
        single = [s.vcycles(k) for k in CALLS]
        single_u = s.download(MG3D_U, L - 1)
    with M.DistSolver(c, L, nu, nranks=P) as d:
        assert 1 <= d.first_level < L
        d.set_shift(sigma)
        d.set_keep_residual(bool(keep))
        _load_dist(d, c, L, data)
        norms = np.concatenate([d.vcycles(k) for k in CALLS])
        runs = nu == 2 and not keep and d.N > 65
        assert d.carried_cycles() == (4 if plan == "carried" and runs else 0)  # 3 + 0 + 1
        assert d.legs_cycles() == (4 if plan == "legs" and runs else 0)
        u = d.download(MG3D_U, L - 1)
        assert _same_bits(u, single_u)
        for l in range(d.first_level, L):
            assert _same_bits(d.download(MG3D_U, l), want[("u", l)]), f"u level {l}"
            if l < L - 1:
                assert _same_bits(d.download(MG3D_D, l), want[("d", l)]), f"d level {l}"
            if keep:
                assert _same_bits(d.download(MG3D_R, l), want[("r", l)]), f"r level {l}"
        assert norms[-1] == pytest.approx(_exact_norm(d, L, sigma), rel=EXACT_NORM_RTOL)
    np.testing.assert_allclose(norms, want["norms"], rtol=norm_rtol(d.N), atol=0)
    np.testing.assert_allclose(norms, np.concatenate(single), rtol=1e-11, atol=0)


@pytest.mark.parametrize("plan,P", [("carried", 2), ("legs", 4), ("plain", 3)])
def test_shift_changed_between_calls_on_slabs(monkeypatch, plan, P):
    """vcycles(4) with sigma1 (red_tail and the last cycle's state behind it), set_shift(sigma2), vcycles(3): equal to the
    reference that switches sigma after four cycles"""
    c, L, s1, s2 = 9, 5, 1e4, 1.0
    _plan_env(monkeypatch, plan, 16, 1, 0)
    ref = S.Problem(c, L, 2, s1)
    u, f, _ = start_data(c, L, "random")
    N = ref.N[-1]
    ref.u[-1][...] = u.reshape(N, N, N)
    ref.d[-1][...] = f.reshape(N, N, N)
    want = list(ref.vcycles(4))
    ref.set_shift(s2)
    want += list(ref.vcycles(3))
    with M.DistSolver(c, L, 2, nranks=P) as d:
        d.set_shift(s1)
        _load_dist(d, c, L, "random")
        norms = list(d.vcycles(4))
        d.set_shift(s2)
        norms += list(d.vcycles(3))
        assert d.carried_cycles() == (5 if plan == "carried" else 0)  # 3 + 2
        assert d.legs_cycles() == (5 if plan == "legs" else 0)
        for l in range(d.first_level, L):
            assert _same_bits(d.download(MG3D_U, l), ref.flat("u", l)), f"u level {l}"
            if l < L - 1:
                assert _same_bits(d.download(MG3D_D, l), ref.flat("d", l)), f"d level {l}"
        assert norms[-1] == pytest.approx(_exact_norm(d, L, s2), rel=EXACT_NORM_RTOL)
    np.testing.assert_allclose(norms, want, rtol=norm_rtol(N), atol=0)


@pytest.mark.parametrize("P", [8, 4, 2])
def test_513_cubed_on_slabs(P):
    """`9 7 2`, sigma = 10, two cycles in the default plan (one launch per leg at this size) on P slabs: the whole solution
    vector against the oracle's; at P = 8 the slab path's norm against the exactly rounded sum"""
    want_norms, want_u = oracle_513(2)
    with M.DistSolver(9, 7, 2, nranks=P) as d:
        d.set_shift(SIGMA_513)
        d.setup_test_problem()
        norms = d.vcycles(2)
        assert d.legs_cycles() == 1 and d.carried_cycles() == 0
        u = d.download(MG3D_U, 6)
        if P == 8:
            exact = exact_norm_513(u, d.download(MG3D_D, 6), 513, d.h, SIGMA_513)
            assert norms[-1] == pytest.approx(exact, rel=EXACT_NORM_RTOL)
    assert _same_bits(u, want_u)
    np.testing.assert_allclose(norms, want_norms, rtol=norm_rtol(513), atol=0)
