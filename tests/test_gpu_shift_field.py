"""The screening field (mg3d_ctx_set_shift_field) on the GPU, against the numpy restatement tests/_shift_field_ref.py: the
single operators and cycles, the restricted hierarchy, the setter forms, the refusals, the neutrality statements, the
singular rule, the solvers, the stepper, full multigrid, the setters in every order and the Poisson-Boltzmann example of
INTEGRATION.md.  Grid values bit for bit, sign bits included, unless said otherwise; norms to the summation tolerance of
tests/test_gpu_parity.py (norm_rtol).

The solvers are held to 100 x the summation spread, never below the figure tests/test_gpu_pcg.py / tests/test_gpu_wpcg.py
hold the same call to.  The spread of the cases here was measured on the CPU as tests/test_gpu_mask_shapes.py does
(python tests/test_gpu_shift_field.py: two restatement runs, exactly rounded dots against numpy's pairwise sums, 33^3,
a random field in [0, 1/h^2]):
    pcg  (Dirichlet, eps exp):        x_1 2.53e-16, x_2 3.95e-16, x_5 3.52e-16, norms 5.19e-15
    wpcg (faces 63, sigma 0, no eps): x_1 0.00e+00, x_2 0.00e+00, x_5 9.39e-17, norms 1.72e-16
(a strongly screened operator is well conditioned: the spread stays at rounding, and on the second case the two runs agree
to the bit for two iterations), all below the two files' own figures, which therefore are the bound."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch  # before the package, as bench.py does: the HIP runtime is torch's

import _coef_ref as CR
import _mask_ref as MR
import _neumann_ref as NR
import _shift_field_ref as SF
import _step_ref as SR
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U, MG3D_F32, MG3D_F64, mg3d_array

from test_gpu_parity import norm_rtol
import test_gpu_pcg as TP
import test_gpu_wpcg as TW

pytestmark = pytest.mark.gpu

MG3D_ERR_ARG, MG3D_ERR_STATE = 1, 5
# measured on the CPU for the cases of test_solvers (module docstring); the bound takes the larger of these and the files' own
SPREAD_U = {"pcg_solve": {1: 2.53e-16, 2: 3.95e-16, 5: 3.52e-16}, "wpcg_solve": {1: 0.0, 2: 0.0, 5: 9.39e-17}}
SPREAD_NORM = {"pcg_solve": 5.19e-15, "wpcg_solve": 1.72e-16}
FILE = {"pcg_solve": TP, "wpcg_solve": TW}
# all Dirichlet; every axis periodic; every face Neumann; periodic k + Neumann on both i faces
BOUNDARIES = [(0, 0), (7, 0), (0, 63), (4, 3)]


def _bound(call, k):
    f = FILE[call]
    return 100 * max(SPREAD_U[call][k], f.SPREAD_U[k]), 100 * max(SPREAD_NORM[call], f.SPREAD_NORM)


def _same_bits(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _n(c, L):
    return (c - 1) * (1 << (L - 1)) + 1


def _eps(N):
    return CR.FIELDS["exp"](N)


def _solver(c, L, nu, sigma, eps, axes, faces, mask, field, factor=True):
    s = M.Solver(c, L, nu)
    s.set_shift(sigma)
    s.set_periodic(axes)
    s.set_neumann(faces)
    if eps is not None:
        s.set_coefficient(eps)
    if mask is not None:
        s.set_mask(mask)
    if field is not None:
        s.set_shift_field(field)
    if factor:
        s.get_details()
    return s


def _random_problem(ref, rng):
    N = ref.N[-1]
    ref.u[-1][...] = rng.standard_normal((N, N, N))
    ref.d[-1][...] = rng.standard_normal((N, N, N))
    NR.refresh(ref.u[-1], ref.axes)
    NR.refresh(ref.d[-1], ref.axes)


def _upload(s, ref):
    s.upload(MG3D_U, ref.L - 1, ref.u[-1])
    s.upload(MG3D_D, ref.L - 1, ref.d[-1])


def _field(N, seed=11):
    return SF.random_field(N, 1.0 / (N - 1), seed)


# --------------------------------------------------------------------------------------- 1 bit parity and the hierarchy
@pytest.mark.parametrize("c", [5, 7])
@pytest.mark.parametrize("axes,faces", BOUNDARIES)
@pytest.mark.parametrize("coef", ["const", "eps"])
@pytest.mark.parametrize("masked", [False, True])
def test_bit_parity(c, axes, faces, coef, masked):
    """17^3 (c = 5) and 25^3 (c = 7, off the ladder), L = 3, sigma = 0.75 and a random field in [0, 1/h^2]: the restricted
    field of every level; mg3d_smooth (pre and post), mg3d_residual with the store on and off, three cycles -- u, r and d of
    every level"""
    L, sigma = 3, 0.75
    N = _n(c, L)
    eps = _eps(N) if coef == "eps" else None
    mask = MR.gpu_test_mask(N) if masked else None
    field = _field(N)
    ref = SF.Hierarchy(c, L, 2, sigma, eps, axes, faces, mask, field)
    rng = np.random.default_rng(N + faces + 64 * axes)
    with _solver(c, L, 2, sigma, eps, axes, faces, mask, field) as s:
        assert s.has_shift_field() and s.has_coefficient() == (eps is not None)
        for l in range(L):
            assert _same_bits(s.get_shift_field(l), ref.s[l]), f"the restricted field of level {l}"
        for l in (L - 1, L - 2):
            n, h, e, m, f = s.level_n(l), s.level_h(l), ref.e(l), ref.mask[l], ref.s[l]
            u, d = rng.standard_normal((n, n, n)), rng.standard_normal((n, n, n))
            NR.refresh(u, axes)
            s.upload(MG3D_U, l, u)
            s.upload(MG3D_D, l, d)
            s.smooth(l, 0, 1)
            for colour in (1, 0):
                SF.colour_pass(u, d, e, h, sigma, axes, faces, colour, m, f)
            assert _same_bits(s.download(MG3D_U, l), u), f"pre-smoothing, level {l}"
            s.smooth(l, 1, 1)
            for colour in (0, 1):
                SF.colour_pass(u, d, e, h, sigma, axes, faces, colour, m, f)
            assert _same_bits(s.download(MG3D_U, l), u), f"post-smoothing, level {l}"
            r = rng.standard_normal((n, n, n))
            r_in = r.copy()
            s.upload(MG3D_R, l, r)
            norm_only = s.residual(l, store=False)
            assert _same_bits(s.download(MG3D_R, l), r_in), "the norm-only residual writes no r"
            got = s.residual(l, store=True)
            SF.residual(u, d, e, h, sigma, axes, faces, m, f, r)
            assert _same_bits(s.download(MG3D_R, l), r), f"residual, level {l}"
            assert got == norm_only
            exact = SF.exact_residual_norm(u, d, e, h, sigma, axes, faces, m, f)
            assert abs(got - exact) <= norm_rtol(n) * exact, (got, exact)
        for l in range(L):
            s.zero(MG3D_R, l)
        _random_problem(ref, rng)
        _upload(s, ref)
        want = ref.vcycles(3)
        got = [s.vcycle()] + list(s.vcycles(2))
        for l in range(L):
            assert _same_bits(s.download(MG3D_U, l), ref.u[l]), f"u level {l}"
        for l in range(L - 1):
            assert _same_bits(s.download(MG3D_D, l), ref.d[l]), f"d level {l}"
        for l in range(1, L):
            assert _same_bits(s.download(MG3D_R, l), ref.r[l]), f"r level {l}"
    np.testing.assert_allclose(got, want, rtol=norm_rtol(N))


# ------------------------------------------------------------------------------------------------------- 2 setter forms
def test_setter_forms():
    """the device setter from a contiguous, a permuted, a sliced and a float32 tensor stores the bytes of the host form on
    every level, and cycles to the same bits; wrong dtype, host pointer, negative stride: MG3D_ERR_ARG, nothing changed"""
    c, L, N = 5, 3, 17
    axes = 5
    dev = torch.device("cuda:0")
    field = _field(N)
    f32 = field.astype(np.float32)
    rng = np.random.default_rng(6)
    u, d = rng.standard_normal(N ** 3), rng.standard_normal(N ** 3)

    def run(s):
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        n = s.vcycles(2)
        return n, s.download(MG3D_U, L - 1), [s.get_shift_field(l) for l in range(L)]

    with M.Solver(c, L, 2) as h, M.Solver(c, L, 2) as g:
        for s in (h, g):
            s.set_periodic(axes)
            s.get_details()
        t = torch.from_numpy(field).to(dev)
        big = torch.zeros((2 * N, N + 3, N + 2), dtype=torch.float64, device=dev)
        big[::2, 2:N + 2, 1:N + 1] = t
        views = {"contiguous": (field, t), "permuted": (field, t.permute(2, 0, 1).contiguous().permute(1, 2, 0)),
                 "sliced": (field, big[::2, 2:N + 2, 1:N + 1]),
                 "float32": (f32.astype(np.float64), torch.from_numpy(f32).to(dev))}
        for name, (host, tensor) in views.items():
            assert tuple(tensor.shape) == (N, N, N)
            h.set_shift_field(host)
            g.set_shift_field_tensor(tensor)
            nh, uh, fh = run(h)
            ng, ug, fg = run(g)
            assert np.array_equal(nh, ng) and _same_bits(uh, ug), name
            want = SF.restrict_field(host, L, axes, 0)
            for l in range(L):
                assert _same_bits(fh[l], fg[l]) and _same_bits(fg[l], want[l]), (name, l)
        before = [g.get_shift_field(l) for l in range(L)]
        lib = g.L
        st = (C.c_longlong * 3)(N * N, N, 1)
        host_arr = np.zeros(N ** 3)
        bad = [mg3d_array(t.data_ptr(), 2, st), mg3d_array(host_arr.ctypes.data, MG3D_F64, st),
               mg3d_array(t.data_ptr() + 8 * (N - 1), MG3D_F64, (C.c_longlong * 3)(N * N, N, -1))]
        for a in bad:
            assert lib.mg3d_ctx_set_shift_field_device(g._h, C.byref(a), None) == MG3D_ERR_ARG
        for l in range(L):
            assert _same_bits(g.get_shift_field(l), before[l])
        g.set_shift_field_tensor(None)
        assert not g.has_shift_field()
        with pytest.raises(M.Mg3dError) as ei:
            g.get_shift_field(0)
        assert ei.value.code == MG3D_ERR_STATE


# ----------------------------------------------------------------------------------------------------- 3 invalid entries
@pytest.mark.parametrize("form", ["host", "device", "device32"])
def test_invalid_entries(form):
    """a negative, a NaN and an inf entry each: MG3D_ERR_ARG naming the entry; two together: the lowest dense index; entries
    on a periodic duplicate are not looked at; the next cycle gives the bits it would have given"""
    c, L, N = 5, 3, 17
    axes = 4
    good = _field(N)
    ref = SF.Hierarchy(c, L, 2, 0.0, None, axes, 0, None, good)
    _random_problem(ref, np.random.default_rng(2))
    u, d = ref.u[-1].copy(), ref.d[-1].copy()
    ref.vcycles(1)
    dev = torch.device("cuda:0")

    def put(s, a):
        if form == "host":
            s.set_shift_field(a)
        elif form == "device":
            s.set_shift_field_tensor(torch.from_numpy(a).to(dev))
        else:
            s.set_shift_field_tensor(torch.from_numpy(a.astype(np.float32)).to(dev))

    with _solver(c, L, 2, 0.0, None, axes, 0, None, good) as s:
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        for value in (-1.0, -1e-300 if form != "device32" else -1e-30, np.nan, np.inf):
            bad = good.copy()
            bad[3, 4, 5] = value
            with pytest.raises(M.Mg3dError) as ei:
                put(s, bad)
            assert ei.value.code == MG3D_ERR_ARG and f"s[{(3 * N + 4) * N + 5}]" in str(ei.value), str(ei.value)
        bad = good.copy()
        bad[9, 1, 1] = np.nan
        bad[2, 16, 3] = -2.0
        bad[2, 3, 16] = -7.0  # a duplicate of the periodic k axis: skipped
        with pytest.raises(M.Mg3dError) as ei:
            put(s, bad)
        assert f"s[{(2 * N + 16) * N + 3}] = -2" in str(ei.value), str(ei.value)
        dup = good.copy()
        dup[:, :, N - 1] = -1.0
        if form == "host":
            put(s, dup)  # only duplicates are bad: accepted, and they take their sources' values
            assert _same_bits(s.get_shift_field(L - 1), ref.s[-1])
        s.vcycles(1)
        assert _same_bits(s.download(MG3D_U, L - 1), ref.u[-1])
        for l in range(L):
            assert _same_bits(s.get_shift_field(l), ref.s[l])


# ------------------------------------------------------------------------------------------------------- 4 neutrality
@pytest.mark.parametrize("axes,faces", BOUNDARIES)
def test_zero_field_on_an_eps_context_is_no_field(axes, faces):
    c, L, N = 5, 4, 33
    eps = _eps(N)
    rng = np.random.default_rng(5)
    u, d = rng.standard_normal(N ** 3), rng.standard_normal(N ** 3)
    with _solver(c, L, 2, 1.5, eps, axes, faces, None, np.zeros(N ** 3)) as a, \
            _solver(c, L, 2, 1.5, eps, axes, faces, None, None) as b:
        assert a.has_shift_field() and not b.has_shift_field()
        for s in (a, b):
            s.upload(MG3D_U, L - 1, u)
            s.upload(MG3D_D, L - 1, d)
        na, nb = a.vcycles(3), b.vcycles(3)
        assert np.array_equal(na, nb)
        for l in range(L):
            assert _same_bits(a.download(MG3D_U, l), b.download(MG3D_U, l))
        assert a.residual(L - 1, store=True) == b.residual(L - 1, store=True)
        assert _same_bits(a.download(MG3D_R, L - 1), b.download(MG3D_R, L - 1))


@pytest.mark.parametrize("axes,faces", BOUNDARIES)
def test_a_field_without_eps_is_eps_one_with_the_field(axes, faces):
    c, L, N = 5, 4, 33
    field = _field(N)
    rng = np.random.default_rng(5)
    u, d = rng.standard_normal(N ** 3), rng.standard_normal(N ** 3)
    with _solver(c, L, 2, 1.5, None, axes, faces, None, field) as a, \
            _solver(c, L, 2, 1.5, np.ones(N ** 3), axes, faces, None, field) as b:
        assert not a.has_coefficient() and b.has_coefficient()
        with pytest.raises(M.Mg3dError) as ei:
            a.coefficient()
        assert ei.value.code == MG3D_ERR_STATE
        for s in (a, b):
            s.upload(MG3D_U, L - 1, u)
            s.upload(MG3D_D, L - 1, d)
        na, nb = a.vcycles(3), b.vcycles(3)
        assert np.array_equal(na, nb)
        for l in range(L):
            assert _same_bits(a.download(MG3D_U, l), b.download(MG3D_U, l))
        # eps set and cleared under the field: the internal ones come and go
        a.set_coefficient(_eps(N))
        a.set_coefficient(None)
        assert not a.has_coefficient() and a.has_shift_field()
        for s in (a, b):
            s.upload(MG3D_U, L - 1, u)
        assert np.array_equal(a.vcycles(2), b.vcycles(2))
        assert _same_bits(a.download(MG3D_U, L - 1), b.download(MG3D_U, L - 1))


@pytest.mark.parametrize("c,L", [(5, 4), (6, 6)])
def test_null_field_restores_the_fused_schedules(c, L):
    """set_shift_field(None) after a field and cycles with it: u, d, the norms and the count of launches without d of a
    fresh context -- at 33^3 and at 161^3, where the fresh context runs one launch per leg"""
    N = _n(c, L)
    assert N in (33, 161)
    rng = np.random.default_rng(N)
    u = rng.standard_normal(N ** 3)
    d = np.zeros(N ** 3)  # (the zero map is full: the legs of the 161^3 context take the kernels without d)
    with M.Solver(c, L, 2) as a, M.Solver(c, L, 2) as b:
        a.get_details()
        b.get_details()
        a.set_shift_field(_field(N))
        a.upload(MG3D_U, L - 1, u)
        a.upload(MG3D_D, L - 1, d)
        a.vcycles(2)
        a.vcycle()
        assert a.dnone_launches() == 0
        a.set_shift_field(None)
        assert not a.has_shift_field()
        for s in (a, b):
            s.upload(MG3D_U, L - 1, u)
            s.upload(MG3D_D, L - 1, d)
        na = [a.vcycle(), a.vcycle()] + list(a.vcycles(3))
        nb = [b.vcycle(), b.vcycle()] + list(b.vcycles(3))
        assert na == nb
        assert _same_bits(a.download(MG3D_U, L - 1), b.download(MG3D_U, L - 1))
        assert _same_bits(a.download(MG3D_D, L - 2), b.download(MG3D_D, L - 2))
        assert a.dnone_launches() == b.dnone_launches() and (N == 33 or b.dnone_launches() > 0)
        with pytest.raises(M.Mg3dError) as ei:
            a.get_shift_field(0)
        assert ei.value.code == MG3D_ERR_STATE


# ---------------------------------------------------------------------------------------------------- 5 singular rule
def test_singular_rule():
    """faces 63, sigma = 0: a zero field leaves the system singular (projected); one positive entry at an unknown makes it
    regular, and full weighting carries it to level 0, where the pinned row goes"""
    c, L, N = 5, 3, 17
    rng = np.random.default_rng(2)
    d = rng.standard_normal((N, N, N))
    u0 = np.zeros((N, N, N))
    one = np.zeros((N, N, N))
    one[5, 7, 9] = 40.0
    with _solver(c, L, 2, 0.0, None, 0, 63, None, np.zeros(N ** 3)) as s:
        s.upload(MG3D_U, L - 1, u0)
        s.upload(MG3D_D, L - 1, d)
        _, info = s.wpcg_solve(rtol=1e-8, max_iters=60)
        assert info["singular"] == 1 and info["converged"]
    prob = SF.Hierarchy(c, L, 2, 0.0, None, 0, 63, None, one)
    assert not prob.pinned() and not prob.is_singular() and prob.s[0].max() > 0
    A = SF.coarse_matrix(c, prob.level_h(0), None, 0.0, 0, 63, None, prob.s[0]).reshape(c ** 3, c ** 3)
    assert A[0, 0] != 1.0 and A[0, 1] != 0.0, "no pinned row"
    x, ref_norms, ok, _, _ = SF.wpcg(prob, u0, d, 1e-8, 0.0, 60)
    assert ok
    with _solver(c, L, 2, 0.0, None, 0, 63, None, one) as s:
        assert _same_bits(s.get_shift_field(0), prob.s[0])
        # the factor the context built is the restatement's: a coarse solve of a random right-hand side, bit for bit
        d0 = rng.standard_normal((c, c, c))
        s.upload(MG3D_D, 0, d0)
        s.coarse_solve()
        want0 = np.zeros((c, c, c))
        SF.coarse_solve(prob.LU, d0, want0, 0, 63, False, None)
        assert _same_bits(s.download(MG3D_U, 0), want0) and want0[0, 0, 0] != 0.0
        s.upload(MG3D_U, L - 1, u0)
        s.upload(MG3D_D, L - 1, d)
        norms, info = s.wpcg_solve(rtol=1e-8, max_iters=60)
        assert info["singular"] == 0 and info["rhs_mean"] == 0. and info["converged"]
        assert info["iterations"] == len(ref_norms) - 1
        u = s.download(MG3D_U, L - 1).reshape(N, N, N)
        assert np.abs(u - x).max() <= 1e-6 * np.abs(x).max()


# ----------------------------------------------------------------------------------------------------------- 6 solvers
def _solver_case(call):
    """(c, L, sigma, eps, axes, faces, field, x0, d) of the solver tests at 33^3"""
    c, L, N = 5, 4, 33
    rng = np.random.default_rng(21)
    field = _field(N)
    d = rng.standard_normal((N, N, N))
    if call == "pcg_solve":
        x0 = rng.standard_normal((N, N, N))
        return c, L, 0.0, _eps(N), 0, 0, field, x0, d
    x0 = rng.standard_normal((N, N, N))
    return c, L, 0.0, None, 0, 63, field, x0, d


@pytest.mark.parametrize("call", ["pcg_solve", "wpcg_solve"])
def test_solvers(call):
    """u after 1, 2 and 5 iterations and the norms against the restatement, to 100 x the summation spread (module
    docstring); to rtol 1e-10 the restatement's iteration count"""
    c, L, sigma, eps, axes, faces, field, x0, d = _solver_case(call)
    N = _n(c, L)
    prob = SF.Hierarchy(c, L, 2, sigma, eps, axes, faces, None, field)
    hist = []
    _, ref_norms, ok, _, sing = SF.wpcg(prob, x0, d, 1e-10, 0.0, 60, history=hist)
    assert ok and not sing and len(hist) >= 5
    with _solver(c, L, 2, sigma, eps, axes, faces, None, field) as s:
        s.upload(MG3D_D, L - 1, d)
        for k in (1, 2, 5):
            s.upload(MG3D_U, L - 1, x0)
            norms, info = getattr(s, call)(rtol=0.0, atol=1e-300, max_iters=k)
            u = s.download(MG3D_U, L - 1).reshape(N, N, N)
            rel = np.abs(u - hist[k - 1]).max() / np.abs(hist[k - 1]).max()
            nrel = (np.abs(norms - ref_norms[:k + 1]) / ref_norms[:k + 1]).max()
            print(call, k, "u", rel, "norms", nrel)
            bu, bn = _bound(call, k)
            assert info["iterations"] == k and rel <= bu and nrel <= bn
        s.upload(MG3D_U, L - 1, x0)
        norms, info = getattr(s, call)(rtol=1e-10, max_iters=60)
        assert info["converged"] and info["iterations"] == len(ref_norms) - 1
        if call == "wpcg_solve":
            assert info["singular"] == 0


# ------------------------------------------------------------------------------------------- 7 stepper, full multigrid
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("coef", ["const", "eps"])
def test_step_rhs(theta, coef):
    """d after one mg3d_step_advance with a source (periodic k + Neumann i faces, 17^3): the stepper's right-hand side with
    the field in q, bit for bit at the unknowns; u after two cycles, bit for bit"""
    c, L, N = 5, 3, 17
    axes, faces, dt, kappa = 4, 3, 1e-3, 2.0
    eps = _eps(N) if coef == "eps" else None
    field = _field(N)
    rng = np.random.default_rng(17)
    u0, src = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    NR.refresh(u0, axes)
    prob = SF.Hierarchy(c, L, 2, SR.sigma_of(dt, theta, kappa), eps, axes, faces, None, field)
    prob.u[-1][...] = u0
    SF.write_rhs(prob, src, dt, theta, kappa)
    want_d = prob.d[-1].copy()
    want_n = prob.vcycles(2)
    with M.Solver(c, L, 2) as s:
        s.set_periodic(axes)
        s.set_neumann(faces)
        if eps is not None:
            s.set_coefficient(eps)
        s.set_shift_field(field)
        s.step_setup(dt, theta, kappa)
        s.get_details()
        s.step_set_source(src)
        s.upload(MG3D_U, L - 1, u0)
        s.zero(MG3D_D, L - 1)
        norms, info = s.step_advance(1, cycles=2, method="vcycles")
        assert info["steps"] == 1
        blk = NR.block(N, axes, faces)
        got_d = s.download(MG3D_D, L - 1).reshape(N, N, N)
        assert _same_bits(got_d[blk], want_d[blk])
        assert _same_bits(s.download(MG3D_U, L - 1), prob.u[-1])
    np.testing.assert_allclose(norms, want_n[-1:], rtol=norm_rtol(N))


@pytest.mark.parametrize("axes,faces", [(0, 0), (4, 3)])
def test_fmg_solve(axes, faces):
    c, L, N = 5, 3, 17
    field = _field(N)
    rng = np.random.default_rng(13)
    prob = SF.Hierarchy(c, L, 2, 0.5, None, axes, faces, None, field)
    _random_problem(prob, rng)
    u, d = prob.u[-1].copy(), prob.d[-1].copy()
    want = SF.fmg_solve(prob, 1)
    with _solver(c, L, 2, 0.5, None, axes, faces, None, field) as s:
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        got = s.fmg_solve(1)
        assert _same_bits(s.download(MG3D_U, L - 1), prob.u[-1])
        assert abs(got - want) <= norm_rtol(N) * want


# ------------------------------------------------------------------------------------------------ 8 setters, refusals
_ORDER_REF = {}
SETTERS = ("shift", "coef", "periodic", "neumann", "mask", "field")


def _order_case():
    """the one case of the setter orders, its restatement run once: 9^3 (c = 5, L = 2), periodic k + Neumann i faces"""
    if not _ORDER_REF:
        c, L, N = 5, 2, 9
        sigma, axes, faces = 3.5, 4, 3
        eps, mask, field = _eps(N), MR.gpu_test_mask(N), _field(N)
        ref = SF.Hierarchy(c, L, 2, sigma, eps, axes, faces, mask, field)
        _random_problem(ref, np.random.default_rng(1))
        u, d = ref.u[-1].copy(), ref.d[-1].copy()
        _ORDER_REF["case"] = (c, L, N, sigma, axes, faces, eps, mask, field, ref, u, d, ref.vcycles(2))
    return _ORDER_REF["case"]


@pytest.mark.parametrize("first", SETTERS)
def test_setters_in_every_order(first):
    """shift, coefficient, periodic, Neumann, mask and field in all 720 orders of the six setters (120 per case: the orders
    that begin with `first`), the factor built before the first, between two of them or after the last: the same bits of u,
    the same stored fields on every level"""
    c, L, N, sigma, axes, faces, eps, mask, field, ref, u, d, want = _order_case()
    setters = {"shift": lambda s: s.set_shift(sigma), "coef": lambda s: s.set_coefficient(eps),
               "periodic": lambda s: s.set_periodic(axes), "neumann": lambda s: s.set_neumann(faces),
               "mask": lambda s: s.set_mask(mask), "field": lambda s: s.set_shift_field(field)}
    rest = [n for n in SETTERS if n != first]
    for n_, tail in enumerate(itertools.permutations(rest)):
        order = (first,) + tail
        with M.Solver(c, L, 2) as s:
            at = n_ % 7
            for pos, name in enumerate(order):
                if pos == at:
                    s.get_details()
                setters[name](s)
            if at == 6:
                s.get_details()
            s.upload(MG3D_U, L - 1, u)
            s.upload(MG3D_D, L - 1, d)
            got = s.vcycles(2)
            assert _same_bits(s.download(MG3D_U, L - 1), ref.u[-1]), order
            for l in range(L):
                assert _same_bits(s.get_shift_field(l), ref.s[l]), (order, l)
            np.testing.assert_allclose(got, want, rtol=norm_rtol(N))


def test_refusals_change_nothing():
    c, L, N = 5, 3, 17
    field = _field(N)
    with M.Solver(c, L, 2) as s:
        s.set_shift_field(field)
        s.get_details()
        for call in (lambda: s.es_setup(), lambda: s.fmg_initialize()):
            with pytest.raises(M.Mg3dError) as ei:
                call()
            assert ei.value.code == MG3D_ERR_STATE
        assert s.L.mg3d_es_smooth(s._h, L - 1, 0, 1) == MG3D_ERR_STATE
        assert s.L.mg3d_es_vcycles(s._h, 1, None) == MG3D_ERR_STATE
        assert s.has_shift_field() and _same_bits(s.get_shift_field(), field)
        s.vcycles(1)  # the factor is still there


def test_a_new_field_rebuilds_a_built_factor_and_drops_an_installed_one():
    c, L, N = 5, 3, 17
    f1, f2 = _field(N, 1), _field(N, 2)
    ref = SF.Hierarchy(c, L, 2, 0.0, None, 0, 0, None, f2)
    _random_problem(ref, np.random.default_rng(9))
    u, d = ref.u[-1].copy(), ref.d[-1].copy()
    ref.vcycles(1)
    with _solver(c, L, 2, 0.0, None, 0, 0, None, f1) as s:
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        s.vcycle()
        s.set_shift_field(f2)  # the factor of get_details() is rebuilt
        s.upload(MG3D_U, L - 1, u)
        s.vcycles(1)
        assert _same_bits(s.download(MG3D_U, L - 1), ref.u[-1])
        s.set_lu(ref.LU)
        s.set_shift_field(f1)  # an installed factor is dropped
        with pytest.raises(M.Mg3dError) as ei:
            s.vcycles(1)
        assert ei.value.code == MG3D_ERR_STATE


# ---------------------------------------------------------------------------------------------------- 9 worked example
def test_poisson_boltzmann_newton_through_tensors():
    """Delta u - kappa^2 sinh u = f at 33^3, manufactured u*, the loop of INTEGRATION.md: s and d are formed by torch on the
    device from the tensor the solver wrote, set with set_shift_field_tensor / upload_tensor, solved by pcg_solve.  The same
    loop in the restatement is the reference: the same number of Newton steps and PCG iterations per step, the iterate to
    100 x the x_5 spread of the PCG bound above per Newton step taken (torch's sinh and cosh may differ from numpy's in the
    last bit, which enters s and d at rounding level like a summation order), and the discretisation error of the CPU run"""
    c, L, N = 5, 4, 33
    kappa2, rtol, newton_tol = 4.0, 1e-10, 1e-9
    want_u, want_steps, want_its = SF.pb_newton(N, c, L, kappa2, rtol, 10, newton_tol)
    ustar, f = SF.pb_problem(N, kappa2)
    want_err = np.abs(want_u - ustar).max()
    assert want_steps <= 8 and want_err < 5e-3
    dev = torch.device("cuda:0")
    ft = torch.from_numpy(f).to(dev)
    u0 = ustar.copy()
    u0[1:-1, 1:-1, 1:-1] = 0.
    u = torch.from_numpy(u0).to(dev)
    its, steps = [], 0
    with M.Solver(c, L, 2) as s:
        s.get_details()
        for k in range(10):
            s.set_shift_field_tensor(kappa2 * torch.cosh(u))
            s.upload_tensor(MG3D_D, L - 1, ft + kappa2 * (torch.sinh(u) - u * torch.cosh(u)))
            s.upload_tensor(MG3D_U, L - 1, u)
            _, info = s.pcg_solve(rtol=rtol, max_iters=50)
            its.append(info["iterations"])
            new = s.download_tensor(MG3D_U, L - 1)
            step = float((new - u).abs().max())
            u = new
            steps = k + 1
            if step <= newton_tol:
                break
    got = u.cpu().numpy()
    err = np.abs(got - ustar).max()
    rel = np.abs(got - want_u).max() / np.abs(want_u).max()
    print("Newton steps", steps, "PCG iterations", its, "error", err, "CPU error", want_err, "iterate difference", rel)
    assert steps == want_steps and its == want_its
    assert rel <= steps * _bound("pcg_solve", 5)[0]
    assert abs(err - want_err) <= 1e-6 * want_err


def _measure_spread():
    for call in ("pcg_solve", "wpcg_solve"):
        c, L, sigma, eps, axes, faces, field, x0, d = _solver_case(call)
        us, n = SF.spread(lambda: SF.Hierarchy(c, L, 2, sigma, eps, axes, faces, None, field), x0, d, (1, 2, 5))
        print(f"{call:10s} x_1, x_2, x_5: " + " ".join(f"{v:.2e}" for v in us) + f"   norms: {n:.2e}")


if __name__ == "__main__":
    _measure_spread()
