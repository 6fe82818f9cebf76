"""Device arrays on the GPU: upload_tensor / download_tensor / step_set_source_tensor / set_coefficient_tensor against the
host forms on a twin context -- every grid value bit for bit (the F64 form stores the same bytes), norms at the project's
summation tolerance.

1  round trips, every field, a middle and the top level, contiguous / permuted / sliced / float32 / stride 0
2  carried state at 161^3 (one-launch legs, and the carried cycles with legs = 0): the device forms finish a cycle that ran
   ahead as the host forms do and leave the run-ahead on
3  the coefficient: every level of eps, the cycles behind it, the check (lowest bad dense index), duplicates, None
4  the stepper with a source replaced between calls
5  stream ordering: the two uses the contract promises, run as a caller would (they cannot prove the absence of a race)
6  arguments

Sizes (c, L): 13 -- a row shorter than the 16-double pitch; 17 -- pitch 32, 15 padding columns; 33 -- pitch 48; 65 -- a second
64-lane block with one live lane; 161 -- the run-ahead schedules."""
import numpy as np
import pytest
import torch  # before the package, as bench.py does: the HIP runtime is torch's

import _coef_ref as CR
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U

gpu = pytest.mark.gpu

MG3D_ERR_ARG = 1
NORM_RTOL = 1e-13
SENTINEL = 12345.678
SIZES = {13: (4, 3), 17: (5, 3), 33: (5, 4), 65: (5, 5), 161: (6, 6)}
FIELDS = (MG3D_U, MG3D_D, MG3D_R)
BCS = {"dirichlet": (0, 0), "per7": (7, 0), "f63": (0, 63)}


def _same_bits(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def _host(t):
    return t.cpu().numpy()


def _levels(N):
    L = SIZES[N][1]
    return (L - 2, L - 1)


def _sentinels(s, level, field):
    """the other two fields of the level hold a pattern; returns a check that they still do"""
    n = s.level_n(level)
    pat = {f: SENTINEL + f + np.arange(n ** 3, dtype=np.float64) for f in FIELDS if f != field}
    for f, p in pat.items():
        s.upload(f, level, p)
    return lambda: all(_same_bits(s.download(f, level), p) for f, p in pat.items())


# ------------------------------------------------------------------------------------------------------- 1 round trips
@gpu
@pytest.mark.parametrize("N", [13, 17, 33, 65])
def test_round_trips_f64(N):
    c, L = SIZES[N]
    rng = np.random.default_rng(N)
    with M.Solver(c, L, 2) as s:
        for level in _levels(N):
            n = s.level_n(level)
            for field in FIELDS:
                intact = _sentinels(s, level, field)
                x = rng.uniform(-1, 1, (n, n, n))
                x[0, 0, 0], x[-1, -1, -1] = -0.0, 5e-324
                # device in, host out
                s.upload_tensor(field, level, _dev(x))
                assert _same_bits(s.download(field, level), x), (level, field)
                assert intact(), (level, field)
                # host in, device out
                y = rng.uniform(-1, 1, (n, n, n))
                s.upload(field, level, y)
                out = s.download_tensor(field, level)
                assert out.dtype == torch.float64 and out.is_cuda and tuple(out.shape) == (n, n, n) and out.is_contiguous()
                assert _same_bits(_host(out), y), (level, field)
                assert intact(), (level, field)


@gpu
@pytest.mark.parametrize("N", [13, 17, 33, 65])
def test_round_trips_through_views(N):
    """a permute(2,1,0) source (k stride n^2) and a sliced destination big[::2, :, 1:] whose gaps keep their sentinel"""
    c, L = SIZES[N]
    rng = np.random.default_rng(100 + N)
    with M.Solver(c, L, 2) as s:
        for level in _levels(N):
            n = s.level_n(level)
            for field in FIELDS:
                intact = _sentinels(s, level, field)
                x = rng.uniform(-1, 1, (n, n, n))
                src = _dev(x.transpose(2, 1, 0)).permute(2, 1, 0)  # logical x, memory transposed
                assert src.stride() == (1, n, n * n)
                s.upload_tensor(field, level, src)
                assert _same_bits(s.download(field, level), x), (level, field)
                big = torch.full((2 * n, n, n + 1), SENTINEL, dtype=torch.float64, device="cuda")
                view = big[::2, :, 1:]
                assert s.download_tensor(field, level, out=view) is view
                got = _host(big)
                assert _same_bits(got[::2, :, 1:], x), (level, field)
                assert np.all(got[1::2] == SENTINEL) and np.all(got[:, :, 0] == SENTINEL)
                # ... and a permuted destination
                back = torch.empty((n, n, n), dtype=torch.float64, device="cuda").permute(2, 1, 0)
                s.download_tensor(field, level, out=back)
                assert _same_bits(_host(back), x)
                assert intact(), (level, field)


@gpu
@pytest.mark.parametrize("N", [13, 17, 33, 65])
def test_round_trips_f32_and_broadcast(N):
    c, L = SIZES[N]
    rng = np.random.default_rng(200 + N)
    with M.Solver(c, L, 2) as s:
        for level in _levels(N):
            n = s.level_n(level)
            for field in FIELDS:
                intact = _sentinels(s, level, field)
                x32 = _dev(rng.uniform(-1, 1, (n, n, n)).astype(np.float32))
                s.upload_tensor(field, level, x32)
                assert _same_bits(s.download(field, level), _host(x32.double())), (level, field)  # widened exactly
                y = rng.uniform(-1, 1, (n, n, n)) * 10.0 ** rng.integers(-30, 30, (n, n, n))
                y[0, 0, 1], y[0, 0, 2], y[0, 0, 3] = 1e39, -1e-46, 1.0 + 2.0 ** -24  # overflow, underflow, a tie
                s.upload(field, level, y)
                out = s.download_tensor(field, level, dtype=torch.float32)
                assert out.dtype == torch.float32
                with np.errstate(over="ignore"):
                    want = s.download(field, level).astype(np.float32)  # round to nearest even
                assert _same_bits(_host(out), want), (level, field)
                # a scalar expanded to the level: strides 0
                s.upload_tensor(field, level, torch.tensor(-2.75, dtype=torch.float64, device="cuda").expand(n, n, n))
                assert _same_bits(s.download(field, level), np.full(n ** 3, -2.75))
                assert intact(), (level, field)


# ----------------------------------------------------------------------------------------------------- 2 carried state
@gpu
@pytest.mark.parametrize("legs", [1, 0])
def test_carried_state_161(legs):
    """a: the device forms, b: the host forms, driven identically.  vcycle() ends ahead of itself (a down-leg in spare
    buffers with the legs, three passes into the next cycle with the carried cycles)."""
    N = 161
    c, L = SIZES[N]
    q = L - 1
    rng = np.random.default_rng(161 + legs)
    u0, d0, d1 = (rng.uniform(-1, 1, (N, N, N)) for _ in range(3))
    with M.Solver(c, L, 2) as a, M.Solver(c, L, 2) as b:
        for s in (a, b):
            s.set_option("legs", legs)
            s.get_details()
            s.upload(MG3D_U, q, u0)
            s.upload(MG3D_D, q, d0)
        na, nb = a.vcycle(), b.vcycle()
        np.testing.assert_allclose(na, nb, rtol=NORM_RTOL)
        assert _same_bits(_host(a.download_tensor(MG3D_U, q)), b.download(MG3D_U, q))
        na, nb = a.vcycle(), b.vcycle()  # (a download only reads: the cycle goes on from where it was)
        np.testing.assert_allclose(na, nb, rtol=NORM_RTOL)
        a.upload_tensor(MG3D_D, q, _dev(d1))
        b.upload(MG3D_D, q, d1)
        na, nb = a.vcycles(2), b.vcycles(2)
        print(legs, na, nb, np.abs(na - nb) / nb)
        np.testing.assert_allclose(na, nb, rtol=NORM_RTOL)
        assert _same_bits(a.download(MG3D_U, q), b.download(MG3D_U, q))
        assert _same_bits(a.download(MG3D_D, q), d1)
        # the device forms switched nothing off: the same launches in the next single cycle, the same bits
        for s in (a, b):
            s.timing_enable(1)
            s.timing_reset()
        na, nb = a.vcycle(), b.vcycle()
        ka = {key: n for key, (n, _) in a.kernel_times().items()}
        kb = {key: n for key, (n, _) in b.kernel_times().items()}
        print(legs, sorted(ka.items()))
        assert ka == kb and ka
        assert (q, "leg_up" if legs else "sweep4+norm") in ka  # the schedule that runs ahead did run
        np.testing.assert_allclose(na, nb, rtol=NORM_RTOL)
        assert _same_bits(_host(a.download_tensor(MG3D_U, q)), b.download(MG3D_U, q))


# ------------------------------------------------------------------------------------------------------- 3 coefficient
def _coef_pair(N, bc):
    c, L = SIZES[N]
    axes, faces = BCS[bc]
    pair = []
    for _ in range(2):
        s = M.Solver(c, L, 2)
        s.set_periodic(axes)
        s.set_neumann(faces)
        pair.append(s)
    return pair


def _cycles_agree(a, b, N, seed, cycles=3):
    q = a.num_levels - 1
    rng = np.random.default_rng(seed)
    u0, d0 = rng.uniform(-1, 1, (N, N, N)), rng.uniform(-1, 1, (N, N, N))
    for s in (a, b):
        s.get_details()
        s.upload(MG3D_U, q, u0)
        s.upload(MG3D_D, q, d0)
    na, nb = a.vcycles(cycles), b.vcycles(cycles)
    assert _same_bits(a.download(MG3D_U, q), b.download(MG3D_U, q))
    assert np.array_equal(na, nb), (na, nb)


@gpu
@pytest.mark.parametrize("bc", list(BCS))
@pytest.mark.parametrize("N", [17, 33])
def test_coefficient_equals_the_host_form(N, bc):
    eps = CR.ball_eps(N, 100.)
    for dtype in (torch.float64, torch.float32):
        a, b = _coef_pair(N, bc)
        with a, b:
            t = _dev(eps, dtype)
            a.set_coefficient_tensor(t)
            b.set_coefficient(_host(t.double()))  # float32: eps.astype(float32).astype(float64)
            assert a.has_coefficient()
            for l in range(a.num_levels):
                assert _same_bits(a.coefficient(l), b.coefficient(l)), (dtype, l)
            _cycles_agree(a, b, N, 300 + N)
    # through a view: the same values, memory transposed
    a, b = _coef_pair(N, bc)
    with a, b:
        rough = eps * np.random.default_rng(N).uniform(0.5, 2.0, eps.shape)
        a.set_coefficient_tensor(_dev(rough.transpose(2, 1, 0)).permute(2, 1, 0))
        b.set_coefficient(rough)
        for l in range(a.num_levels):
            assert _same_bits(a.coefficient(l), b.coefficient(l)), l
        _cycles_agree(a, b, N, 310 + N)


@gpu
@pytest.mark.parametrize("N", [17, 33])
def test_coefficient_check_names_the_lowest_bad_index(N):
    c, L = SIZES[N]
    eps = CR.ball_eps(N, 100.)
    lo, hi = (2, N - 1, 3), (N - 2, 0, N - 1)  # (hi sits in another block row and in the last k lane group)
    p_lo = (lo[0] * N + lo[1]) * N + lo[2]
    with M.Solver(c, L, 2) as a, M.Solver(c, L, 2) as b:
        for bad in (float("nan"), 0.0, -1.0, float("inf")):
            for permuted in (False, True):
                e = eps.copy()
                e[lo] = e[hi] = bad
                t = _dev(e.transpose(2, 1, 0)).permute(2, 1, 0) if permuted else _dev(e)
                with pytest.raises(M.Mg3dError) as err:
                    a.set_coefficient_tensor(t)
                assert err.value.code == MG3D_ERR_ARG
                assert f"eps[{p_lo}] = " in str(err.value), (bad, str(err.value))
                assert not a.has_coefficient()
        e32 = _dev(eps, torch.float32)
        e32[hi] = float("nan")
        with pytest.raises(M.Mg3dError) as err:
            a.set_coefficient_tensor(e32)
        assert err.value.code == MG3D_ERR_ARG and f"eps[{(hi[0] * N + hi[1]) * N + hi[2]}] = " in str(err.value)
        assert not a.has_coefficient()
        _cycles_agree(a, b, N, 320 + N, cycles=1)  # ... and the context is the untouched one
    # a refused array leaves a coefficient that was set before in place
    a, b = _coef_pair(N, "dirichlet")
    with a, b:
        a.set_coefficient_tensor(_dev(eps))
        b.set_coefficient(eps)
        e = eps.copy()
        e[hi] = -3.0
        with pytest.raises(M.Mg3dError):
            a.set_coefficient_tensor(_dev(e))
        for l in range(a.num_levels):
            assert _same_bits(a.coefficient(l), b.coefficient(l)), l
        _cycles_agree(a, b, N, 330 + N, cycles=1)


@gpu
def test_coefficient_periodic_duplicates_are_not_checked():
    N = 17
    eps = CR.ball_eps(N, 100.) * np.random.default_rng(5).uniform(0.5, 2.0, (N, N, N))
    eps[N - 1, 3, 4] = eps[2, N - 1, 5] = eps[6, 7, N - 1] = eps[N - 1, N - 1, N - 1] = float("nan")
    a, b = _coef_pair(N, "per7")
    with a, b:
        a.set_coefficient_tensor(_dev(eps))
        b.set_coefficient(eps)  # the host form accepts it as well
        for l in range(a.num_levels):
            ea = a.coefficient(l)
            assert np.isfinite(ea).all() and _same_bits(ea, b.coefficient(l)), l
        _cycles_agree(a, b, N, 340)
    a, b = _coef_pair(N, "dirichlet")  # ... without the periodic axis the same entry is refused
    with a, b:
        with pytest.raises(M.Mg3dError) as err:
            a.set_coefficient_tensor(_dev(eps))
        assert err.value.code == MG3D_ERR_ARG and f"eps[{(2 * N + N - 1) * N + 5}] = " in str(err.value)


@gpu
def test_coefficient_none_is_the_constant_operator():
    N = 17
    c, L = SIZES[N]
    with M.Solver(c, L, 2) as a, M.Solver(c, L, 2) as fresh:
        a.set_coefficient_tensor(None)  # nothing to drop
        assert not a.has_coefficient()
        a.set_coefficient_tensor(_dev(CR.ball_eps(N, 100.)))
        a.get_details()
        assert a.has_coefficient()
        a.set_coefficient_tensor(None)
        assert not a.has_coefficient()
        _cycles_agree(a, fresh, N, 350)


# ----------------------------------------------------------------------------------------------------------- 4 stepper
@gpu
@pytest.mark.parametrize("coef", [False, True])
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("N", [17, 33])
def test_stepper_source_from_a_tensor(N, theta, coef):
    c, L = SIZES[N]
    q = L - 1
    rng = np.random.default_rng(400 + N)
    u0, s0, s1 = (rng.uniform(-1, 1, (N, N, N)) for _ in range(3))
    with M.Solver(c, L, 2) as a, M.Solver(c, L, 2) as b:
        for s in (a, b):
            if coef:
                s.set_coefficient(CR.ball_eps(N, 100.))
            s.get_details()
            s.step_setup(0.01, theta, 0.75)
            s.upload(MG3D_U, q, u0)
        t0 = _dev(s0)
        a.step_set_source_tensor(t0)
        t0.zero_()  # the array is the caller's again when the call returns
        b.step_set_source(s0)
        na0, nb0 = a.step_advance(3)[0], b.step_advance(3)[0]
        a.step_set_source_tensor(_dev(s1.transpose(2, 1, 0)).permute(2, 1, 0))
        b.step_set_source(s1)
        na1, nb1 = a.step_advance(2)[0], b.step_advance(2)[0]
        assert np.array_equal(na0, nb0) and np.array_equal(na1, nb1)
        assert _same_bits(a.download(MG3D_U, q), b.download(MG3D_U, q))
        assert _same_bits(a.download(MG3D_D, q), b.download(MG3D_D, q))
        # float32, and no source at all
        a.step_set_source_tensor(_dev(s0, torch.float32))
        b.step_set_source(s0.astype(np.float32).astype(np.float64))
        assert np.array_equal(a.step_advance(1)[0], b.step_advance(1)[0])
        assert _same_bits(a.download(MG3D_U, q), b.download(MG3D_U, q))
        a.step_set_source_tensor(None)
        b.step_set_source(None)
        assert np.array_equal(a.step_advance(1)[0], b.step_advance(1)[0])
        assert _same_bits(a.download(MG3D_U, q), b.download(MG3D_U, q))
        assert _same_bits(a.download(MG3D_D, q), b.download(MG3D_D, q))


# --------------------------------------------------------------------------------------------------- 5 stream ordering
@gpu
def test_stream_ordering_upload_then_overwrite_and_download_then_use():
    N = 65
    c, L = SIZES[N]
    q = L - 1
    base = np.random.default_rng(500).uniform(0.5, 1.5, (N, N, N))
    want = base.copy()
    for i in range(50):  # the same chain in numpy: IEEE multiply and add, one rounding each
        want = want * 1.0009765625 + (i * 0.125)
    side = torch.cuda.Stream()
    with M.Solver(c, L, 2) as s:
        x = _dev(base)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for i in range(50):
                x = x * 1.0009765625 + (i * 0.125)
            s.upload_tensor(MG3D_U, q, x)
            x.zero_()
        assert _same_bits(s.download(MG3D_U, q), want)  # (the host form waits for the context's stream)
        with torch.cuda.stream(side):
            out = s.download_tensor(MG3D_U, q)
            y = out * 1
        torch.cuda.synchronize()
        assert _same_bits(_host(y), want)
        assert not _host(x).any()


# ----------------------------------------------------------------------------------------------------------- 6 arguments
@gpu
def test_arguments():
    N = 17
    c, L = SIZES[N]
    q = L - 1
    u0 = np.random.default_rng(600).uniform(-1, 1, N ** 3)
    good = torch.ones(N, N, N, dtype=torch.float64, device="cuda")

    def refused(exc, call, code=None):
        with pytest.raises(exc) as e:
            call()
        if code is not None:
            assert e.value.code == code, e.value
        for f in FIELDS:
            assert _same_bits(s.download(f, q), u0 + f)

    with M.Solver(c, L, 2) as s:
        for f in FIELDS:
            s.upload(f, q, u0 + f)
        cpu = torch.ones(N, N, N, dtype=torch.float64)
        refused(ValueError, lambda: s.upload_tensor(MG3D_U, q, cpu))
        refused(ValueError, lambda: s.download_tensor(MG3D_U, q, out=cpu))
        refused(ValueError, lambda: s.step_set_source_tensor(cpu))
        refused(ValueError, lambda: s.set_coefficient_tensor(cpu))
        wrong = torch.ones(N, N, N + 1, dtype=torch.float64, device="cuda")
        refused(ValueError, lambda: s.upload_tensor(MG3D_U, q, wrong))
        refused(ValueError, lambda: s.upload_tensor(MG3D_U, q - 1, good))  # the shape of another level
        refused(ValueError, lambda: s.download_tensor(MG3D_U, q, out=wrong))
        refused(ValueError, lambda: s.step_set_source_tensor(wrong))
        refused(ValueError, lambda: s.set_coefficient_tensor(wrong))
        refused(TypeError, lambda: s.upload_tensor(MG3D_U, q, good.half()))
        refused(TypeError, lambda: s.upload_tensor(MG3D_U, q, u0.reshape(N, N, N)))
        refused(M.Mg3dError, lambda: s.upload_tensor(3, q, good), MG3D_ERR_ARG)
        refused(M.Mg3dError, lambda: s.upload_tensor(-1, q, good), MG3D_ERR_ARG)
        refused(M.Mg3dError, lambda: s.download_tensor(3, q, out=good), MG3D_ERR_ARG)
        refused((ValueError, M.Mg3dError), lambda: s.upload_tensor(MG3D_U, L, good))
        refused((ValueError, M.Mg3dError), lambda: s.download_tensor(MG3D_U, -1))
        refused(ValueError, lambda: s.download_tensor(MG3D_U, q, out=good[0:1].expand(N, N, N)))
        assert np.all(_host(good) == 1.0)
        # the library's own checks, past the Python ones: a descriptor built by hand
        import ctypes as C
        from multigrid_parallel_amd.binding import array_desc
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def rc(fn, *args):
            return fn(s._h, *args, stream)

        for call in (lambda a: rc(s.L.mg3d_upload_device, MG3D_U, q, a), lambda a: rc(s.L.mg3d_download_device, MG3D_U, q, a),
                     lambda a: rc(s.L.mg3d_step_set_source_device, a), lambda a: rc(s.L.mg3d_ctx_set_coefficient_device, a)):
            a = array_desc(good)
            a.ptr = None
            assert call(C.byref(a)) == MG3D_ERR_ARG
            a = array_desc(good)
            a.dtype = 2
            assert call(C.byref(a)) == MG3D_ERR_ARG
            a = array_desc(good)
            a.stride[1] = -N
            assert call(C.byref(a)) == MG3D_ERR_ARG
            a = array_desc(cpu)  # host memory
            assert call(C.byref(a)) == MG3D_ERR_ARG
        a = array_desc(good)
        a.stride[0] = 0
        assert rc(s.L.mg3d_download_device, MG3D_U, q, C.byref(a)) == MG3D_ERR_ARG
        assert rc(s.L.mg3d_upload_device, MG3D_U, L, C.byref(array_desc(good))) == MG3D_ERR_ARG
        assert rc(s.L.mg3d_upload_device, MG3D_U, q, None) == MG3D_ERR_ARG
        assert not s.has_coefficient()
        for f in FIELDS:
            assert _same_bits(s.download(f, q), u0 + f)
        torch.cuda.synchronize()
        assert np.all(_host(good) == 1.0)
