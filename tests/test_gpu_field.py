"""The field output on the GPU -- mg3d_field_gradient(_device), mg3d_field_flux, mg3d_field_energy -- against the numpy
restatement tests/_field_ref.py.

1  the gradient into a contiguous (3, N, N, N) float64 tensor, bit for bit (sign of zero included) on random u -- every
   point of u random, Dirichlet faces and periodic duplicates too, so a tap that reads a duplicate or leaves the array
   shows.  The kernel's plane chunk is 4, not 16: 5 (c = 5, L = 1) is the smallest ladder size with a full chunk and a
   shorter tail and stands beside 33 in the list; 17 / 33 = four / eight chunks and a one-plane tail that is the high
   face (a chunk that STARTS on the face), 37 = off the ladder, 65 / 129 = a second / third 64-lane k-block with one live
   lane and a last j-block of one row.
2  its output forms: float32, interleaved storage (k stride 3), permuted views, a slice of a larger tensor whose gaps keep
   a sentinel, absent components, mixed dtypes; the host form.
3  flux and energy against the exactly rounded sums of the restated terms, at the summation tolerance 1e-13 (flux:
   relative to the sum of |t_p|, the terms carry signs); labels, a fixed point on a Neumann face, bytes on Dirichlet
   faces and duplicates; the slab problem with its closed-form values; one size past the cap of partial sums
   (tests/test_field_ref_host.py derives it); determinism.
4  arguments and state: errors leave the outputs untouched; behind a cycle that has run ahead the calls see the finished
   cycle and the next cycle goes on as if they had not been made; after a solve the energy and -1/2 V F are what the
   restatement computes from the downloaded u."""
import ctypes as C
import math

import numpy as np
import pytest
import torch  # before the package, as bench.py does: the HIP runtime is torch's

import _coef_ref as CR
import _field_ref as FR
import _mask_ref as MR
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_F32, MG3D_F64, MG3D_U, P, mg3d_array
from test_field_ref_host import slab_problem

gpu = pytest.mark.gpu

MG3D_ERR_ARG, MG3D_ERR_STATE = 1, 5
SUM_RTOL = 1e-13  # the project's summation tolerance (tests/_oracle.py)
SENTINEL = 12345.678
# N: (c, L)
SIZES = {5: (5, 1), 17: (5, 3), 33: (5, 4), 37: (10, 3), 65: (5, 5), 129: (5, 6), 161: (6, 6), FR.CAP_SIZE: (18, 6)}
# a periodic axis needs an even c - 1: 37 = 18 * 2 + 1 there (the calls look at the finest level only)
PERIODIC_37 = (19, 2)
# (periodic axes, Neumann faces), named as in tests/test_gpu_step.py
BCS = {"dirichlet": (0, 0), "per7": (7, 0), "per4_f15": (4, 15), "f63": (0, 63), "f22": (0, 22), "f25": (0, 0b011001)}
ALL_BCS = tuple(BCS)

GRADIENT_CASES = ([(N, bc, extra) for N in (5, 17, 33) for bc in ALL_BCS for extra in (False, True)]
                  + [(37, "dirichlet", False), (37, "f63", False), (65, "per7", False), (65, "f63", False),
                     (129, "f25", False)])
SUM_CASES = [(N, bc, coef) for N in FR.SUM_SIZES for bc in ALL_BCS for coef in (False, True)]


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _host(t):
    return t.cpu().numpy()


def field_mask(N):
    """a ball (label 1), a plate on plane N // 4 outside it (label 2), one point on the low i face and one on the high j
    face (label 5: fixed unknowns of weight 1/2 where those are Neumann faces, ignored where they are Dirichlet faces), and
    bytes on the high i face and on the last k index -- a Dirichlet face, a Neumann face or a periodic duplicate"""
    m = MR.sphere(N).astype(np.uint8)
    plate = MR.plate(N, N // 4) != 0
    m[plate & (m == 0)] = 2
    m[0, N // 2, N // 2] = 5
    m[N // 2, N - 1, N // 2 + 1] = 5
    m[N - 1, 1:4, 1:4] = 6
    m[2:5, 2:5, N - 1] = 1
    return m


def _solver(N, bc, coef=False, mask=None):
    axes, faces = BCS[bc]
    c, L = PERIODIC_37 if N == 37 and axes else SIZES[N]
    s = M.Solver(c, L, 2)
    assert s.N == N
    s.set_periodic(axes)
    s.set_neumann(faces)
    if coef:
        s.set_coefficient(CR.ball_eps(N))
    if mask is not None:
        s.set_mask(mask)
    return s


def _random_u(N, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (N, N, N))


# ----------------------------------------------------------------------------------------------------------- 1 gradient
@gpu
@pytest.mark.parametrize("N,bc,extra", GRADIENT_CASES)
def test_gradient_bits(N, bc, extra):
    """extra: eps and a mask are set, which must make no difference"""
    axes, faces = BCS[bc]
    u = _random_u(N, 1000 * N + axes * 64 + faces)
    with _solver(N, bc, coef=extra, mask=field_mask(N) if extra else None) as s:
        q = s.num_levels - 1
        s.upload(MG3D_U, q, u)
        s.timing_enable(1)
        s.timing_reset()
        for scale in (-1.0, 0.37):
            g = s.gradient_tensor(scale=scale)
            assert g.dtype == torch.float64 and tuple(g.shape) == (3, N, N, N) and g.is_contiguous() and g.is_cuda
            want = FR.gradient(u, s.h, axes, faces, scale)
            got = _host(g)
            for a in range(3):
                assert _same_bits(got[a], want[a]), (N, bc, scale, a, np.argwhere(got[a] != want[a])[:4])
        s.sync()
        assert s.kernel_times()[(q, "pack")][0] == 2  # one launch per call, counted with the array I/O
        assert _same_bits(s.download(MG3D_U, q).reshape(N, N, N), u)


# ------------------------------------------------------------------------------------------------------- 2 output forms
@gpu
@pytest.mark.parametrize("N", [17, 65])
def test_gradient_output_forms(N):
    bc = "per4_f15"
    axes, faces = BCS[bc]
    u = _random_u(N, 2000 + N) * 10.0 ** np.random.default_rng(N).integers(-3, 3, (N, N, N))
    dev = dict(dtype=torch.float64, device="cuda")
    with _solver(N, bc) as s:
        s.upload(MG3D_U, s.num_levels - 1, u)
        want = FR.gradient(u, s.h, axes, faces, -1.0)
        want32 = [w.astype(np.float32) for w in want]
        # float32: rounded to nearest even
        g32 = s.gradient_tensor(dtype=torch.float32, scale=-1.0)
        assert g32.dtype == torch.float32
        for a in range(3):
            assert _same_bits(_host(g32)[a], want32[a]), a
        # interleaved storage: component last in memory, k stride 3
        big = torch.full((N, N, N, 3), SENTINEL, **dev)
        view = big.permute(3, 0, 1, 2)
        assert view.stride() == (1, 3 * N * N, 3 * N, 3)
        assert s.gradient_tensor(out=view, scale=-1.0) is view
        for a in range(3):
            assert _same_bits(_host(big)[..., a], want[a]), a
        # permuted views
        comps = [torch.full((N, N, N), SENTINEL, **dev).permute(2, 1, 0) for _ in range(3)]
        s.gradient_tensor(out=comps, scale=-1.0)
        for a in range(3):
            assert _same_bits(_host(comps[a]), want[a]), a
        # a slice of a larger tensor: the gaps keep their sentinel
        big = torch.full((3, 2 * N, N, N + 1), SENTINEL, **dev)
        s.gradient_tensor(out=big[:, ::2, :, 1:], scale=-1.0)
        got = _host(big)
        for a in range(3):
            assert _same_bits(got[a, ::2, :, 1:], want[a]), a
        assert np.all(got[:, 1::2] == SENTINEL) and np.all(got[:, :, :, 0] == SENTINEL)
        # one and two components absent: the unwanted arrays keep their sentinel
        for wanted in ((0, 2), (1,), (2,)):
            keep = torch.full((3, N, N, N), SENTINEL, **dev)
            s.gradient_tensor(out=[keep[a] if a in wanted else None for a in range(3)], scale=-1.0)
            got = _host(keep)
            for a in range(3):
                assert _same_bits(got[a], want[a]) if a in wanted else np.all(got[a] == SENTINEL), (wanted, a)
        # mixed dtypes per component
        mixed = [torch.full((N, N, N), SENTINEL, dtype=dt, device="cuda") for dt in (torch.float64, torch.float32, torch.float64)]
        s.gradient_tensor(out=mixed, scale=-1.0)
        assert _same_bits(_host(mixed[0]), want[0]) and _same_bits(_host(mixed[1]), want32[1]) and _same_bits(_host(mixed[2]), want[2])


@gpu
@pytest.mark.parametrize("N,bc", [(17, "per4_f15"), (65, "f63"), (37, "dirichlet")])
def test_gradient_host_form_equals_the_device_form(N, bc):
    u = _random_u(N, 3000 + N)
    with _solver(N, bc) as s:
        s.upload(MG3D_U, s.num_levels - 1, u)
        dev = _host(s.gradient_tensor(scale=-1.0))
        host = s.gradient(scale=-1.0)
        for a in range(3):
            assert host[a].shape == (N, N, N) and _same_bits(host[a], dev[a]), a
        # one component alone: the others are not touched
        gj = np.full(N ** 3, SENTINEL)
        M.binding.check(s.L.mg3d_field_gradient(s._h, -1.0, None, P(gj), None))
        assert _same_bits(gj.reshape(N, N, N), dev[1])


# ------------------------------------------------------------------------------------------------------ 3 flux, energy
def _check_sums(s, u, eps, mask, axes, faces, labels):
    h = s.h
    for label in labels:
        t = FR.flux_terms(u, eps, mask, axes, faces, label)
        want, scale = h * FR.fsum(t), h * FR.fsum(np.abs(t))
        got = s.field_flux(label)
        print("flux", label, t.size, got, want, abs(got - want) / scale if scale else 0.)
        assert abs(got - want) <= SUM_RTOL * scale, (label, got, want)
        assert s.field_flux(label) == got  # the same call on the same data: the same bits
        if t.size == 0:
            assert got == 0. and math.copysign(1., got) > 0
    want = FR.energy(u, eps, h, axes, faces)
    got = s.field_energy()
    print("energy", got, want, abs(got - want) / want)
    assert want > 0 and abs(got - want) <= SUM_RTOL * want
    assert s.field_energy() == got


@gpu
@pytest.mark.parametrize("N,bc,coef", SUM_CASES)
def test_flux_and_energy(N, bc, coef):
    axes, faces = BCS[bc]
    u = _random_u(N, 4000 * N + axes * 64 + faces + coef)
    mask = field_mask(N)
    with _solver(N, bc, coef=coef, mask=mask) as s:
        q = s.num_levels - 1
        s.upload(MG3D_U, q, u)
        eps = s.coefficient() if coef else None
        _check_sums(s, u, eps, mask, axes, faces, (0, 1, 2, 5, 200))
        # label 5 sits on faces only: fixed unknowns exactly where those are Neumann faces
        # (index 0 of a periodic axis is an unknown like any other)
        assert FR.flux_points(mask, axes, faces, 5).sum() == (FR.neu(faces, 0, 0) or FR.per(axes, 0)) + FR.neu(faces, 1, 1)
        assert _same_bits(s.download(MG3D_U, q).reshape(N, N, N), u)
    # the energy needs no mask
    with _solver(N, bc, coef=coef) as s:
        s.upload(MG3D_U, s.num_levels - 1, u)
        want = FR.energy(u, eps, s.h, axes, faces)
        assert abs(s.field_energy() - want) <= SUM_RTOL * want


@gpu
def test_slab_problem():
    """uploaded, not solved: F = -4/3 through the body with label 3, W = 2/3, and W = -1/2 V F with V = 1"""
    axes, faces, h, u, mask = slab_problem()
    with M.Solver(5, 3, 2) as s:
        assert s.N == 17 and s.h == h
        s.set_periodic(axes)
        s.set_mask(mask)
        s.upload(MG3D_U, 2, u)
        F, W, F0, F4 = s.field_flux(3), s.field_energy(), s.field_flux(0), s.field_flux(4)
    print(F, W)
    assert abs(F + 4.0 / 3.0) <= 1e-12 and abs(W - 2.0 / 3.0) <= 1e-12 and F0 == F
    assert F4 == 0. and math.copysign(1., F4) > 0


@gpu
def test_sums_past_the_cap_of_partials():
    """CAP_SIZE, constant operator, Dirichlet faces: both launches run 32 planes per block (tests/test_field_ref_host.py).
    u is zero but for random blobs in the first block, across the first chunk boundary, in the middle and in the last
    block of every axis; the body is a small ball in the middle and a few points in the first and the last blocks"""
    N = FR.CAP_SIZE
    rng = np.random.default_rng(N)
    u = np.zeros((N, N, N))
    t = torch.zeros((N, N, N), dtype=torch.float64, device="cuda")
    mask = np.zeros((N, N, N), dtype=np.uint8)
    for lo in (0, 28, N // 2 - 4, N - 8):
        blob = rng.uniform(-1, 1, (8, 8, 8))
        u[lo:lo + 8, lo:lo + 8, lo:lo + 8] = blob
        t[lo:lo + 8, lo:lo + 8, lo:lo + 8] = torch.from_numpy(blob).cuda()
        mask[lo + 1:lo + 4, lo + 2:lo + 5, lo + 3:lo + 7] = 1
    x = np.arange(N) - N // 2
    mask[(x[:, None, None] ** 2 + x[None, :, None] ** 2 + x[None, None, :] ** 2) <= 9] = 1
    with _solver(N, "dirichlet") as s:
        s.upload_tensor(MG3D_U, s.num_levels - 1, t)
        del t
        s.set_mask(mask)
        _check_sums(s, u, None, mask, 0, 0, (1,))


# --------------------------------------------------------------------------------------------------- 4 arguments, state
@gpu
def test_arguments():
    N = 17
    u = _random_u(N, 5)
    with _solver(N, "f63") as s:
        L, h = s.L, s._h
        s.upload(MG3D_U, 2, u)
        keep = torch.full((3, N, N, N), SENTINEL, dtype=torch.float64, device="cuda")
        untouched = lambda: bool(torch.all(keep == SENTINEL))
        ap = C.POINTER(mg3d_array)

        def device_rc(descs, scale=1.0, ctx=h):
            ptrs = (ap * 3)(*[C.pointer(d) if d is not None else ap() for d in descs])
            return L.mg3d_field_gradient_device(ctx, scale, ptrs, None)

        def desc(t, dtype=MG3D_F64, strides=None, ptr=None):
            return mg3d_array(t.data_ptr() if ptr is None else ptr, dtype, (C.c_longlong * 3)(*(strides or t.stride())))

        good = [desc(keep[a]) for a in range(3)]
        assert device_rc(good, ctx=None) == MG3D_ERR_ARG  # a NULL context
        assert device_rc([None, None, None]) == MG3D_ERR_ARG  # nothing wanted
        assert L.mg3d_field_gradient_device(h, 1.0, None, None) == MG3D_ERR_ARG
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert device_rc(good, scale=bad) == MG3D_ERR_ARG
        assert device_rc([good[0], desc(keep[1], dtype=7), good[2]]) == MG3D_ERR_ARG  # a bad dtype
        assert device_rc([good[0], desc(keep[1], dtype=2), good[2]]) == MG3D_ERR_ARG  # bytes are a mask's
        assert device_rc([good[0], good[1], desc(keep[2], strides=(N * N, N, 0))]) == MG3D_ERR_ARG  # a stride < 1
        assert device_rc([good[0], good[1], desc(keep[2], strides=(N * N, -N, 1))]) == MG3D_ERR_ARG
        foreign = np.zeros(N ** 3)
        assert device_rc([desc(keep[0], ptr=foreign.ctypes.data), good[1], good[2]]) == MG3D_ERR_ARG  # host memory
        assert device_rc([desc(keep[0], ptr=0), good[1], good[2]]) == MG3D_ERR_ARG
        with pytest.raises(M.Mg3dError) as e:
            s.gradient_tensor(out=[None, None, None])
        assert e.value.code == MG3D_ERR_ARG
        s.sync()
        assert untouched() and not foreign.any()
        # the host form
        hg = [np.full(N ** 3, SENTINEL) for _ in range(3)]
        assert L.mg3d_field_gradient(None, 1.0, P(hg[0]), P(hg[1]), P(hg[2])) == MG3D_ERR_ARG
        assert L.mg3d_field_gradient(h, 1.0, None, None, None) == MG3D_ERR_ARG
        assert L.mg3d_field_gradient(h, float("nan"), P(hg[0]), P(hg[1]), P(hg[2])) == MG3D_ERR_ARG
        assert all(np.all(a == SENTINEL) for a in hg)
        # flux and energy
        f = C.c_double(SENTINEL)
        assert L.mg3d_field_flux(h, 0, C.byref(f)) == MG3D_ERR_STATE and b"mask" in L.mg3d_last_error()  # no mask
        s.set_mask(field_mask(N))
        assert L.mg3d_field_flux(None, 0, C.byref(f)) == MG3D_ERR_ARG
        assert L.mg3d_field_flux(h, 0, None) == MG3D_ERR_ARG
        assert L.mg3d_field_flux(h, -1, C.byref(f)) == MG3D_ERR_ARG and L.mg3d_field_flux(h, 256, C.byref(f)) == MG3D_ERR_ARG
        assert L.mg3d_field_energy(None, C.byref(f)) == MG3D_ERR_ARG and L.mg3d_field_energy(h, None) == MG3D_ERR_ARG
        assert f.value == SENTINEL
        assert L.mg3d_field_flux(h, 255, C.byref(f)) == 0 and f.value == 0.
        # every refusal left the context as it was
        assert _same_bits(s.download(MG3D_U, 2).reshape(N, N, N), u)
        for a in range(3):
            assert _same_bits(_host(s.gradient_tensor(out=keep))[a], FR.gradient(u, s.h, 0, 63, 1.0)[a])


@gpu
@pytest.mark.parametrize("legs", [1, 0])
def test_behind_a_cycle_that_has_run_ahead_161(legs):
    """vcycle() at 161^3 ends ahead of itself (one launch per leg; the carried cycles with legs = 0).  a makes the field
    calls there and nothing else; b downloads instead, which is known to read only.  The gradient and the energy are the
    restatement's of the finished cycle's u, and the next cycle of a has b's bits: norm and u"""
    N = 161
    c, L = SIZES[N]
    q = L - 1
    rng = np.random.default_rng(161 + legs)
    u0, d0 = rng.uniform(-1, 1, (N, N, N)), rng.uniform(-1, 1, (N, N, N))
    with M.Solver(c, L, 2) as a, M.Solver(c, L, 2) as b:
        for s in (a, b):
            s.set_option("legs", legs)
            s.get_details()
            s.upload(MG3D_U, q, u0)
            s.upload(MG3D_D, q, d0)
            s.timing_enable(1)
            s.timing_reset()
        na, nb = a.vcycle(), b.vcycle()
        assert na == nb
        assert (q, "leg_up" if legs else "sweep4+norm") in a.kernel_times()  # the schedule that runs ahead did run
        g = _host(a.gradient_tensor(scale=-1.0))
        W = a.field_energy()
        gh = a.gradient(scale=-1.0)
        u = b.download(MG3D_U, q).reshape(N, N, N)
        want = FR.gradient(u, a.h, 0, 0, -1.0)
        for k in range(3):
            assert _same_bits(g[k], want[k]) and _same_bits(gh[k], want[k]), k
        Wref = FR.energy(u, None, a.h, 0, 0)
        assert abs(W - Wref) <= SUM_RTOL * Wref
        na, nb = a.vcycles(1), b.vcycles(1)
        assert na[0] == nb[0]
        assert _same_bits(a.download(MG3D_U, q), b.download(MG3D_U, q))
        assert _same_bits(a.download(MG3D_D, q).reshape(N, N, N), d0)


@gpu
def test_capacitance_after_a_solve_33():
    """the grounded box with a ball at potential V ("Field output"), solved by mg3d_pcg_solve: the energy
    and -1/2 V F are what the restatement computes from the downloaded u, at the summation tolerance; how well the two
    agree with each other depends on the solve and is printed"""
    N, V = 33, 2.0
    mask = MR.sphere(N).astype(np.uint8)
    with _solver(N, "dirichlet", mask=mask) as s:
        q = s.num_levels - 1
        s.get_details()
        u0 = np.zeros((N, N, N))
        u0[mask != 0] = V
        s.upload(MG3D_U, q, u0)
        s.zero(MG3D_D, q)
        norms, info = s.pcg_solve(rtol=1e-12, max_iters=40)
        assert info["converged"]
        W, F = s.field_energy(), s.field_flux(1)
        u = s.download(MG3D_U, q).reshape(N, N, N)
        assert np.all(u[mask != 0] == V)
        t = FR.flux_terms(u, None, mask, 0, 0, 1)
        Wref, Fref = FR.energy(u, None, s.h, 0, 0), s.h * FR.fsum(t)
        print("W", W, Wref, "-VF/2", -0.5 * V * F, -0.5 * V * Fref, "C from W", 2 * W / V ** 2, "C from F", -F / V,
              "mutual", abs(W + 0.5 * V * F) / W)
        assert abs(W - Wref) <= SUM_RTOL * Wref
        assert abs(-0.5 * V * F - -0.5 * V * Fref) <= SUM_RTOL * 0.5 * V * s.h * FR.fsum(np.abs(t))
