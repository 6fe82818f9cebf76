"""The particle coupling on the GPU -- mg3d_field_sample(_device), mg3d_deposit(_device) -- against the numpy / Python-int
restatement tests/_particle_ref.py, bit for bit.

1  the sample on random u -- every point of u random, Dirichlet faces and periodic duplicates too, so a tap that reads a
   duplicate or leaves the array shows -- at seeded points inside the box and at the edge points of the restatement: exact
   nodes, both ends of every axis, cell boundaries, coordinates far outside on periodic axes, coordinates outside, NaN and
   inf on the others (NaN out).  5 (c = 5, L = 1): one cell touches both faces and the one-sided taps reach N-3; 17; 37 off
   the ladder; 65: the row pitch goes past one 64-lane block.  Counts 1, 255, 256, 257, 4099 and one past the grid cap
   (tests/test_particle_ref_host.py derives it).
2  its forms: an (M, 3) tensor, three separate tensors, float32 positions and outputs, a strided slice of a larger output
   whose gaps keep a sentinel, absent outputs, the host form.
3  the deposit onto a random d on every boundary set, with eps and a mask set (no difference), charges of both signs over
   12 decades; all-zero q; two contexts; the points reversed and shuffled; the duplicates of d; a broadcast q; float32;
   the host form; the launch counts.
4  state at 161^3: behind a cycle that has run ahead the deposit and the sample see the finished cycle; after the deposit
   the next cycles are those of a fresh context with the same u and d, the zero map is rescanned; after the sample the
   next cycle goes on as if it had not been made.
5  arguments: every refusal leaves outputs, d and the launch counts untouched."""
import ctypes as C

import numpy as np
import pytest
import torch  # before the package, as bench.py does: the HIP runtime is torch's

import _coef_ref as CR
import _field_ref as FR
import _mask_ref as MR
import _particle_ref as PR
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_F64, MG3D_U, P, mg3d_vec
from test_particle_ref_host import PAST_CAP_COUNT

gpu = pytest.mark.gpu

MG3D_ERR_ARG = 1
SENTINEL = 12345.678
# N: (c, L)
SIZES = {5: (5, 1), 17: (5, 3), 37: (10, 3), 65: (5, 5), 161: (6, 6)}
# a periodic axis needs an even c - 1: 37 = 18 * 2 + 1 there (the calls look at the finest level only)
PERIODIC_37 = (19, 2)
# (periodic axes, Neumann faces), the sets of tests/test_gpu_field.py
BCS = {"dirichlet": (0, 0), "per7": (7, 0), "per4_f15": (4, 15), "f63": (0, 63), "f22": (0, 22), "f25": (0, 0b011001)}
ALL_BCS = tuple(BCS)

# (N, bc, seeded points beside the edge points, eps and a mask set)
CASES = ([(5, bc, 257, True) for bc in ALL_BCS] + [(17, bc, 255, False) for bc in ALL_BCS]
         + [(37, "dirichlet", 4099, False), (37, "per7", 256, False), (37, "f25", 1, True), (65, "f63", 256, False),
            (65, "per4_f15", 1, False), (65, "f22", 4099, False), (17, "per4_f15", PAST_CAP_COUNT, False)])


def _same_bits(a, b):
    """equal values with equal signs of zero; NaN where and only where the other has one"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return (np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb])
            and np.array_equal(np.signbit(a[~na]), np.signbit(b[~nb])))


def _host(t):
    return t.cpu().numpy()


def _dev(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def _solver(N, bc, extra=False):
    axes, faces = BCS[bc]
    c, L = PERIODIC_37 if N == 37 and axes else SIZES[N]
    s = M.Solver(c, L, 2)
    assert s.N == N
    s.set_periodic(axes)
    s.set_neumann(faces)
    if extra:
        s.set_coefficient(CR.ball_eps(N))
        s.set_mask(MR.sphere(N).astype(np.uint8))
    return s


def _random(N, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (N, N, N))


def _points(N, h, axes, count, seed):
    """`count` seeded points inside the box, then the edge points (a count of 1: the one point alone)"""
    if count == 1:
        return PR.box_points(N, h, 1, seed)
    return np.concatenate([PR.box_points(N, h, count, seed), PR.edge_points(N, h, axes)])


def _charges(count, seed):
    """both signs, 12 decades"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.1, 1.0, count) * rng.choice([-1.0, 1.0], count) * 10.0 ** rng.integers(-6, 6, count)


def _pack_count(s):
    s.sync()
    return s.kernel_times().get((s.num_levels - 1, "pack"), (0, 0.))[0]


# ------------------------------------------------------------------------------------------------------------- 1 sample
@gpu
@pytest.mark.parametrize("N,bc,count,extra", CASES)
def test_sample_bits(N, bc, count, extra):
    axes, faces = BCS[bc]
    u = _random(N, 1000 * N + axes * 64 + faces)
    with _solver(N, bc, extra) as s:
        q = s.num_levels - 1
        xyz = _points(N, s.h, axes, count, 7 * N + count)
        M_ = xyz.shape[0]
        s.upload(MG3D_U, q, u)
        s.timing_enable(1)
        s.timing_reset()
        pos = _dev(xyz)
        for n, scale in enumerate((-1.0, 0.37)):
            gu, gg = s.sample_tensor(pos, scale=scale)
            assert gu.dtype == torch.float64 and tuple(gu.shape) == (M_,) and tuple(gg.shape) == (M_, 3) and gg.is_cuda
            wu, wg = PR.sample(u, xyz, s.h, axes, faces, scale)
            assert _same_bits(_host(gu), wu), (N, bc, np.argwhere(_host(gu) != wu)[:4])
            assert _same_bits(_host(gg), wg), (N, bc, scale, np.argwhere(_host(gg) != wg)[:4])
            assert _pack_count(s) == n + 1  # one launch per call, counted with the array I/O
        if count > 1:
            assert np.isnan(wu).any() and np.isfinite(wu[:count]).all()  # the edge points do hold points outside
        assert _same_bits(s.download(MG3D_U, q).reshape(N, N, N), u)


# -------------------------------------------------------------------------------------------------------------- 2 forms
@gpu
@pytest.mark.parametrize("N,bc", [(17, "per4_f15"), (37, "dirichlet")])
def test_sample_forms(N, bc):
    axes, faces = BCS[bc]
    u = _random(N, 2000 + N) * 10.0 ** np.random.default_rng(N).integers(-3, 3, (N, N, N))
    with _solver(N, bc) as s:
        s.upload(MG3D_U, s.num_levels - 1, u)
        xyz = _points(N, s.h, axes, 300, 21)
        M_ = xyz.shape[0]
        wu, wg = PR.sample(u, xyz, s.h, axes, faces, -1.0)
        pos = _dev(xyz)
        # three separate tensors; a transposed (3, M) storage
        gu, gg = s.sample_tensor([pos[:, 0].contiguous(), pos[:, 1].contiguous(), pos[:, 2].contiguous()], scale=-1.0)
        assert _same_bits(_host(gu), wu) and _same_bits(_host(gg), wg)
        gu, gg = s.sample_tensor(pos.t().contiguous().t(), scale=-1.0)
        assert _same_bits(_host(gu), wu) and _same_bits(_host(gg), wg)
        # float32 positions: widened exactly
        with np.errstate(over="ignore"):
            xyz32 = xyz.astype(np.float32)
        w32u, w32g = PR.sample(u, xyz32.astype(np.float64), s.h, axes, faces, -1.0)
        gu, gg = s.sample_tensor(_dev(xyz32, torch.float32), scale=-1.0)
        assert gu.dtype == torch.float64 and _same_bits(_host(gu), w32u) and _same_bits(_host(gg), w32g)
        # float32 outputs: rounded to nearest even
        gu, gg = s.sample_tensor(pos, scale=-1.0, dtype=torch.float32)
        assert gu.dtype == torch.float32 and gg.dtype == torch.float32
        assert _same_bits(_host(gu), wu.astype(np.float32)) and _same_bits(_host(gg), wg.astype(np.float32))
        # a strided slice of a larger output: the gaps keep their sentinel
        big_u = torch.full((2 * M_ + 1,), SENTINEL, dtype=torch.float64, device="cuda")
        big_g = torch.full((M_, 7), SENTINEL, dtype=torch.float64, device="cuda")
        ru, rg = s.sample_tensor(pos, scale=-1.0, out_u=big_u[1::2], out_grad=big_g[:, 2:7:2])
        assert ru.data_ptr() == big_u[1::2].data_ptr()
        hu, hg = _host(big_u), _host(big_g)
        assert _same_bits(hu[1::2], wu) and np.all(hu[0::2] == SENTINEL)
        assert _same_bits(hg[:, 2:7:2], wg) and np.all(hg[:, [0, 1, 3, 5]] == SENTINEL)
        # absent outputs
        gu, gg = s.sample_tensor(pos, want_grad=False, scale=-1.0)
        assert gg is None and _same_bits(_host(gu), wu)
        gu, gg = s.sample_tensor(pos, want_u=False, scale=-1.0)
        assert gu is None and _same_bits(_host(gg), wg)
        keep = torch.full((M_, 3), SENTINEL, dtype=torch.float64, device="cuda")
        vp = C.POINTER(mg3d_vec)
        descs = [mg3d_vec(pos[:, a].data_ptr(), MG3D_F64, 3) for a in range(3)]
        pp = (vp * 3)(*[C.pointer(d) for d in descs])
        gj = mg3d_vec(keep[:, 1].data_ptr(), MG3D_F64, 3)
        gp = (vp * 3)(vp(), C.pointer(gj), vp())
        M.binding.check(s.L.mg3d_field_sample_device(s._h, M_, pp, -1.0, None, gp, None))
        hk = _host(keep)
        assert _same_bits(hk[:, 1], wg[:, 1]) and np.all(hk[:, [0, 2]] == SENTINEL)
        # the host form: the bits of the device form; one output alone
        hu, hg = s.sample(xyz, scale=-1.0)
        assert _same_bits(hu, wu) and _same_bits(hg, wg)
        only = np.full(M_, SENTINEL)
        M.binding.check(s.L.mg3d_field_sample(s._h, M_, P(np.ascontiguousarray(xyz).reshape(-1)), -1.0, P(only), None))
        assert _same_bits(only, wu)
        # no point at all: nothing launched
        s.timing_enable(1)
        s.timing_reset()
        gu, gg = s.sample_tensor(pos[:0])
        assert tuple(gu.shape) == (0,) and tuple(gg.shape) == (0, 3) and _pack_count(s) == 0


# ------------------------------------------------------------------------------------------------------------ 3 deposit
@gpu
@pytest.mark.parametrize("N,bc,count,extra", CASES)
def test_deposit_bits(N, bc, count, extra):
    axes, faces = BCS[bc]
    d0 = _random(N, 3000 * N + axes * 64 + faces)
    scale = -1.0 / 8.8541878128e-12 * 1e-15
    with _solver(N, bc, extra) as s, _solver(N, bc) as other:
        q = s.num_levels - 1
        xyz = _points(N, s.h, axes, count, 9 * N + count)
        M_ = xyz.shape[0]
        ch = _charges(M_, 11 * N + count)
        if M_ > 20:
            ch[3], ch[5] = np.nan, -np.inf  # not deposited
        want = PR.deposit(d0, xyz, ch, s.h, axes, faces, scale)
        pos, qt = _dev(xyz), _dev(ch)
        s.upload(MG3D_D, q, d0)
        s.timing_enable(1)
        s.timing_reset()
        s.deposit_tensor(pos, qt, scale=scale)
        assert _pack_count(s) == (4 if axes else 3)  # scan, accumulate, apply (+ the duplicate refresh)
        got = s.download(MG3D_D, q).reshape(N, N, N)
        assert _same_bits(got, want), (N, bc, np.argwhere(got != want)[:4])
        assert not _same_bits(got, d0)
        for ax in range(3):  # the duplicates of d equal their sources
            if FR.per(axes, ax):
                assert _same_bits(np.take(got, N - 1, axis=ax), np.take(got, 0, axis=ax))
        # another context, the points reversed: the same bits; shuffled, through the host form
        other.upload(MG3D_D, q, d0)
        other.deposit_tensor(pos.flip(0), qt.flip(0), scale=scale)
        assert _same_bits(other.download(MG3D_D, q).reshape(N, N, N), want)
        if M_ <= 5000:
            perm = np.random.default_rng(N).permutation(M_)
            other.upload(MG3D_D, q, d0)
            other.deposit(xyz[perm], ch[perm], scale=scale)
            assert _same_bits(other.download(MG3D_D, q).reshape(N, N, N), want)
        # all-zero q leaves d bit-identical, the state handling still happens
        s.upload(MG3D_D, q, d0)
        s.deposit_tensor(pos, torch.zeros(M_, dtype=torch.float64, device="cuda"), scale=scale)
        assert _same_bits(s.download(MG3D_D, q).reshape(N, N, N), d0) and s.dzero_planes()[1] == 1


@gpu
@pytest.mark.parametrize("N,bc", [(17, "f25"), (37, "per7")])
def test_deposit_forms(N, bc):
    axes, faces = BCS[bc]
    d0 = _random(N, 4000 + N)
    with _solver(N, bc) as s:
        q = s.num_levels - 1
        xyz = _points(N, s.h, axes, 300, 23)
        M_ = xyz.shape[0]
        ch = _charges(M_, 24)
        pos = _dev(xyz)

        def run(*a, **k):
            s.upload(MG3D_D, q, d0)
            s.deposit_tensor(*a, **k)
            return s.download(MG3D_D, q).reshape(N, N, N)

        # a broadcast q (stride 0): one charge for all
        one = torch.tensor([2.5e-3], dtype=torch.float64, device="cuda").expand(M_)
        assert one.stride() == (0,)
        assert _same_bits(run(pos, one, scale=3.0), PR.deposit(d0, xyz, np.full(M_, 2.5e-3), s.h, axes, faces, 3.0))
        # three separate tensors, q a strided slice
        wide = torch.zeros(2 * M_, dtype=torch.float64, device="cuda")
        wide[::2] = _dev(ch)
        want = PR.deposit(d0, xyz, ch, s.h, axes, faces, -2.0)
        assert _same_bits(run([pos[:, a].contiguous() for a in range(3)], wide[::2], scale=-2.0), want)
        # float32 positions and charges: widened exactly
        with np.errstate(over="ignore"):
            xyz32, ch32 = xyz.astype(np.float32), ch.astype(np.float32)
        want32 = PR.deposit(d0, xyz32.astype(np.float64), ch32.astype(np.float64), s.h, axes, faces, -2.0)
        assert _same_bits(run(_dev(xyz32, torch.float32), _dev(ch32, torch.float32), scale=-2.0), want32)
        # the host form
        s.upload(MG3D_D, q, d0)
        s.deposit(xyz, ch, scale=-2.0)
        assert _same_bits(s.download(MG3D_D, q).reshape(N, N, N), want)
        # only points outside, and no point at all: d untouched, the state handling still happens
        for p_, q_ in ((_dev(np.full((3, 3), np.nan)), _dev(np.ones(3))), (pos[:0], _dev(ch)[:0])):
            s.zero(MG3D_D, q)
            assert s.dzero_planes()[1] == 2
            s.deposit_tensor(p_, q_)
            assert s.dzero_planes()[1] == 1
            assert not s.download(MG3D_D, q).any()


# -------------------------------------------------------------------------------------------------------------- 4 state
@gpu
def test_deposit_behind_a_cycle_that_has_run_ahead_161():
    """vcycle() at 161^3 ends ahead of itself (one launch per leg).  The deposit finishes that cycle, adds to d and marks
    it written: d is the restatement's, the zero map is to be rescanned (state 1), and the next two cycles are, in norms
    and u, those of a fresh context that had the same u and the downloaded d uploaded"""
    N = 161
    c, L = SIZES[N]
    q = L - 1
    rng = np.random.default_rng(161)
    u0 = rng.uniform(-1, 1, (N, N, N))
    d0 = np.zeros((N, N, N))
    d0[40:60] = rng.uniform(-1, 1, (20, N, N))  # most planes of d are zero: the zero map matters
    with M.Solver(c, L, 2) as a, M.Solver(c, L, 2) as b:
        xyz = PR.box_points(N, a.h, 4099, 5)[:, :] * np.array([0.5, 1.0, 1.0])  # the lower half of the planes
        ch = _charges(4099, 6)
        for s in (a, b):
            s.get_details()
        a.upload(MG3D_U, q, u0)
        a.upload(MG3D_D, q, d0)
        a.timing_enable(1)
        a.timing_reset()
        a.vcycle()
        assert a.dzero_planes()[1] == 2
        assert (q, "leg_up") in a.kernel_times()  # the schedule that runs ahead did run
        a.deposit_tensor(_dev(xyz), _dev(ch), scale=-1.0)
        assert a.dzero_planes() == (0, 1)
        u1, d1 = a.download(MG3D_U, q), a.download(MG3D_D, q)
        assert _same_bits(d1.reshape(N, N, N), PR.deposit(d0, xyz, ch, a.h, 0, 0, -1.0))
        b.upload(MG3D_U, q, u1)
        b.upload(MG3D_D, q, d1)
        na, nb = a.vcycles(2), b.vcycles(2)
        assert np.array_equal(na, nb)
        assert _same_bits(a.download(MG3D_U, q), b.download(MG3D_U, q))
        assert a.dzero_planes() == b.dzero_planes() and a.dzero_planes()[1] == 2


@gpu
@pytest.mark.parametrize("legs", [1, 0])
def test_sample_behind_a_cycle_that_has_run_ahead_161(legs):
    """a samples behind vcycle() and does nothing else; b downloads instead, which is known to read only.  The sample is
    the restatement's of the finished cycle's u, and the next cycle of a has b's bits: norm and u"""
    N = 161
    c, L = SIZES[N]
    q = L - 1
    rng = np.random.default_rng(162 + legs)
    u0, d0 = rng.uniform(-1, 1, (N, N, N)), rng.uniform(-1, 1, (N, N, N))
    with M.Solver(c, L, 2) as a, M.Solver(c, L, 2) as b:
        xyz = _points(N, a.h, 0, 1000, 8)
        for s in (a, b):
            s.set_option("legs", legs)
            s.get_details()
            s.upload(MG3D_U, q, u0)
            s.upload(MG3D_D, q, d0)
            s.timing_enable(1)
            s.timing_reset()
        assert a.vcycle() == b.vcycle()
        assert (q, "leg_up" if legs else "sweep4+norm") in a.kernel_times()
        gu, gg = a.sample_tensor(_dev(xyz), scale=-1.0)
        hu, hg = a.sample(xyz, scale=-1.0)
        u = b.download(MG3D_U, q).reshape(N, N, N)
        wu, wg = PR.sample(u, xyz, a.h, 0, 0, -1.0)
        assert _same_bits(_host(gu), wu) and _same_bits(_host(gg), wg) and _same_bits(hu, wu) and _same_bits(hg, wg)
        na, nb = a.vcycles(1), b.vcycles(1)
        assert na[0] == nb[0]
        assert _same_bits(a.download(MG3D_U, q), b.download(MG3D_U, q))
        assert _same_bits(a.download(MG3D_D, q).reshape(N, N, N), d0)


# ------------------------------------------------------------------------------------------------------------- 5 errors
@gpu
def test_refusals_leave_everything_untouched():
    N, M_ = 17, 40
    u, d0 = _random(N, 51), _random(N, 52)
    with _solver(N, "f63") as s:
        q = s.num_levels - 1
        L, h = s.L, s._h
        s.upload(MG3D_U, q, u)
        s.upload(MG3D_D, q, d0)
        s.timing_enable(1)
        s.timing_reset()
        xyz = PR.box_points(N, s.h, M_, 53)
        pos = _dev(xyz)
        qt = _dev(_charges(M_, 54))
        ou = torch.full((M_,), SENTINEL, dtype=torch.float64, device="cuda")
        og = torch.full((M_, 3), SENTINEL, dtype=torch.float64, device="cuda")
        vp = C.POINTER(mg3d_vec)

        def vec(t, dtype=MG3D_F64, stride=None, ptr=None):
            return mg3d_vec(t.data_ptr() if ptr is None else ptr, dtype, t.stride(0) if stride is None else stride)

        def ptrs(descs):
            return (vp * 3)(*[C.pointer(v) if v is not None else vp() for v in descs])

        good_pos = [vec(pos[:, a]) for a in range(3)]
        good_g = [vec(og[:, a]) for a in range(3)]
        good_u, good_q = vec(ou), vec(qt)
        foreign = np.zeros(3 * M_)

        def sample_rc(ctx=h, count=M_, p=good_pos, scale=1.0, vu=good_u, g=good_g):
            return L.mg3d_field_sample_device(ctx, count, ptrs(p) if p is not None else None, scale,
                                              C.byref(vu) if vu is not None else None, ptrs(g) if g is not None else None, None)

        def deposit_rc(ctx=h, count=M_, p=good_pos, vq=good_q, scale=1.0):
            return L.mg3d_deposit_device(ctx, count, ptrs(p) if p is not None else None,
                                         C.byref(vq) if vq is not None else None, scale, None)

        bad_vectors = [vec(pos[:, 1], dtype=7), vec(pos[:, 1], dtype=2), vec(pos[:, 1], stride=-3),
                       vec(pos[:, 1], ptr=foreign.ctypes.data), vec(pos[:, 1], ptr=0)]
        for rc in (sample_rc, deposit_rc):
            assert rc(ctx=None) == MG3D_ERR_ARG  # a NULL context
            assert rc(p=None) == MG3D_ERR_ARG  # NULL positions
            assert rc(count=-1) == MG3D_ERR_ARG and rc(count=(1 << 40) + 1) == MG3D_ERR_ARG
            for bad in (float("nan"), float("inf"), -float("inf")):
                assert rc(scale=bad) == MG3D_ERR_ARG
            for v in bad_vectors:
                assert rc(p=[good_pos[0], v, good_pos[2]]) == MG3D_ERR_ARG
            assert rc(p=[good_pos[0], good_pos[1], None]) == MG3D_ERR_ARG
        assert sample_rc(vu=None, g=None) == MG3D_ERR_ARG  # nothing wanted
        assert sample_rc(vu=None, g=[None, None, None]) == MG3D_ERR_ARG
        assert sample_rc(vu=vec(ou, stride=0)) == MG3D_ERR_ARG  # an output needs a stride >= 1
        assert sample_rc(g=[good_g[0], vec(og[:, 1], stride=0), good_g[2]]) == MG3D_ERR_ARG
        assert sample_rc(vu=vec(ou, dtype=5)) == MG3D_ERR_ARG
        assert sample_rc(vu=vec(ou, ptr=foreign.ctypes.data)) == MG3D_ERR_ARG
        assert deposit_rc(vq=None) == MG3D_ERR_ARG  # a NULL q
        for v in bad_vectors:
            assert deposit_rc(vq=v) == MG3D_ERR_ARG
        # the host forms
        hx, hq = np.ascontiguousarray(xyz).reshape(-1), _charges(M_, 55)
        hu, hg = np.full(M_, SENTINEL), np.full(3 * M_, SENTINEL)
        assert L.mg3d_field_sample(None, M_, P(hx), 1.0, P(hu), P(hg)) == MG3D_ERR_ARG
        assert L.mg3d_field_sample(h, M_, None, 1.0, P(hu), P(hg)) == MG3D_ERR_ARG
        assert L.mg3d_field_sample(h, M_, P(hx), 1.0, None, None) == MG3D_ERR_ARG
        assert L.mg3d_field_sample(h, -1, P(hx), 1.0, P(hu), P(hg)) == MG3D_ERR_ARG
        assert L.mg3d_field_sample(h, M_, P(hx), float("nan"), P(hu), P(hg)) == MG3D_ERR_ARG
        assert L.mg3d_deposit(None, M_, P(hx), P(hq), 1.0) == MG3D_ERR_ARG
        assert L.mg3d_deposit(h, M_, None, P(hq), 1.0) == MG3D_ERR_ARG and L.mg3d_deposit(h, M_, P(hx), None, 1.0) == MG3D_ERR_ARG
        assert L.mg3d_deposit(h, M_, P(hx), P(hq), float("inf")) == MG3D_ERR_ARG
        assert np.all(hu == SENTINEL) and np.all(hg == SENTINEL) and not foreign.any()
        # the tensor forms: a host tensor, wrong shapes, wrong types
        with pytest.raises(ValueError):
            s.sample_tensor(pos.cpu())
        with pytest.raises(ValueError):
            s.deposit_tensor(pos, qt.cpu())
        with pytest.raises(ValueError):
            s.sample_tensor(pos[:, :2])
        with pytest.raises(ValueError):
            s.sample_tensor([pos[:, 0], pos[:, 1]])
        with pytest.raises(ValueError):
            s.sample_tensor([pos[:, 0], pos[:, 1], pos[:5, 2]])
        with pytest.raises(ValueError):
            s.sample_tensor(pos, out_u=ou[:-1])
        with pytest.raises(ValueError):
            s.sample_tensor(pos, out_grad=og[:, :2])
        with pytest.raises(ValueError):
            s.sample_tensor(pos, out_u=ou[:1].expand(M_))
        with pytest.raises(ValueError):
            s.deposit_tensor(pos, qt[:-1])
        with pytest.raises(TypeError):
            s.sample_tensor(pos.to(torch.float16))
        with pytest.raises(TypeError):
            s.deposit_tensor(pos, qt.to(torch.int64))
        with pytest.raises(M.Mg3dError) as e:
            s.sample_tensor(pos, want_u=False, want_grad=False)
        assert e.value.code == MG3D_ERR_ARG
        # every refusal left outputs, d, u and the launch counts as they were
        assert _pack_count(s) == 0
        assert bool(torch.all(ou == SENTINEL)) and bool(torch.all(og == SENTINEL))
        assert _same_bits(s.download(MG3D_D, q).reshape(N, N, N), d0) and _same_bits(s.download(MG3D_U, q).reshape(N, N, N), u)
        gu, gg = s.sample_tensor(pos, out_u=ou, out_grad=og)
        wu, wg = PR.sample(u, xyz, s.h, 0, 63, 1.0)
        assert _same_bits(_host(gu), wu) and _same_bits(_host(gg), wg)
