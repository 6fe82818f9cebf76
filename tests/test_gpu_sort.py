"""The particle reorder on the GPU -- mg3d_particle_sort(_device), mg3d_particle_permute_device -- against the numpy
restatement tests/_sort_ref.py, bit for bit: stability makes the permutation unique.

1  bits: perm and counts on every boundary set of tests/_push_ref.py at N = 5, 17, 37 (periodic), 65, 161 and 321, counts 1,
   255, 256, 257, 4099, one past the grid cap of the point kernels and one past 1024 tiles, shift 0 and 2 (8 once at 321),
   float64 and float32 positions, with and without a fate vector; the launches counted (1 + 3 passes).  Degenerate inputs:
   one cell, sorted, reversed, all dead, all lost.  tests/test_sort_ref_host.py holds these cases to their coverage.
2  forms: (M, 3) tensors and three vectors, strided slices whose gaps keep a sentinel, a broadcast fate, the host form, no
   particle at all; the permute: one launch for up to 16 vectors, fancy indexing bit for bit with mixed types, NaN and
   -0.0, entries of perm out of range.
3  the loop: deposit, three cycles and push, five times, as it is and with a reorder before every step.
4  state at 161^3: behind a cycle that has run ahead a sort changes nothing.
5  arguments: every refusal leaves perm, counts, the outputs and the launch counts untouched."""
import ctypes as C

import numpy as np
import pytest
import torch  # before the package, as bench.py does: the HIP runtime is torch's

import _push_ref as QR
import _sort_ref as SR
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_F32, MG3D_F64, MG3D_I32, MG3D_U, P, mg3d_vec

gpu = pytest.mark.gpu

MG3D_ERR_ARG = 1
SENTINEL = 12345.678
ISENT = -7


def _same_bits(a, b):
    """the same bytes: signs of zero and NaN payloads included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _host(t):
    return t.cpu().numpy()


def _dev(a, dtype=None):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def _solver(N, bc, mask=None):
    axes, faces = QR.BCS[bc]
    c, L = SR.SIZES[N]
    s = M.Solver(c, L, 2)
    assert s.N == N and s.h == SR.spacing(N)
    s.set_periodic(axes)
    s.set_neumann(faces)
    if mask is not None:
        s.set_mask(mask)
    return s


def _pack_count(s):
    s.sync()
    return s.kernel_times().get((s.num_levels - 1, "pack"), (0, 0.))[0]


def _check_sort(s, N, bc, xyz, fate, shift, f32=False):
    """one sort_tensor against the restatement, its launches counted"""
    axes = QR.BCS[bc][0]
    with np.errstate(over="ignore"):  # (1e300 becomes inf: lost either way)
        pos = xyz.astype(np.float32) if f32 else xyz
    want, wc = SR.sort(pos, fate, s.h, N, axes, shift)
    s.timing_reset()
    perm, counts = s.sort_tensor(_dev(pos), None if fate is None else _dev(fate), shift=shift)
    assert _pack_count(s) == 1 + 3 * SR.passes(N, shift)
    got, gc = _host(perm), _host(counts)
    assert got.dtype == np.int32 and gc.dtype == np.int64 and gc.shape == (2,)
    assert np.array_equal(gc, wc), (N, bc, xyz.shape[0], shift, f32, gc, wc)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (N, bc, xyz.shape[0], shift, f32, bad[:4], got[bad[:4]], want[bad[:4]])


# --------------------------------------------------------------------------------------------------------------- 1 bits
@gpu
@pytest.mark.parametrize("N,bc", SR.SMALL_CASES)
def test_sort_bits_small(N, bc):
    with _solver(N, bc) as s:
        s.timing_enable(1)
        for count in SR.SMALL_COUNTS:
            xyz, fate = SR.particles(N, bc, count)
            for shift in (0, 2):
                for f32 in (False, True):
                    for f in (fate, None):
                        _check_sort(s, N, bc, xyz, f, shift, f32)


@gpu
@pytest.mark.parametrize("N,bc", SR.LARGE_CASES)
def test_sort_bits_large(N, bc):
    with _solver(N, bc) as s:
        s.timing_enable(1)
        for n, count in enumerate(SR.LARGE_COUNTS):
            xyz, fate = SR.particles(N, bc, count)
            _check_sort(s, N, bc, xyz, fate, 0, f32=bool(n))
            _check_sort(s, N, bc, xyz, None if n else fate, 2, f32=not n)
        if N == 321:
            xyz, fate = SR.particles(N, bc, SR.SMALL_COUNTS[-1])
            _check_sort(s, N, bc, xyz, fate, 8)
            # a smaller count behind a larger one: the scratch stays, the tiles are the smaller count's
            _check_sort(s, N, bc, xyz, fate, 0)


@gpu
@pytest.mark.parametrize("N,bc,count", [(65, "dirichlet", 5000), (17, "per7", 4099), (321, "f22", 2 * SR.TILE + 1)])
def test_sort_degenerate_inputs(N, bc, count):
    axes = QR.BCS[bc][0]
    h = SR.spacing(N)
    rng = np.random.default_rng(N + count)
    ident = np.arange(count, dtype=np.int32)
    alive = np.zeros(count, dtype=np.int32)
    with _solver(N, bc) as s:
        s.timing_enable(1)
        # every particle in one cell: the identity
        one = (np.array([1.25, 2.5, 0.75]) + rng.uniform(0.0, 0.2, (count, 3))) * h
        assert np.array_equal(SR.sort(one, alive, h, N, axes)[0], ident)
        perm, counts = s.sort_tensor(_dev(one), _dev(alive))
        assert np.array_equal(_host(perm), ident) and _host(counts).tolist() == [count, 0]
        # already sorted, and in reverse order
        xyz = SR.particles(N, bc, count)[0]
        order = SR.sort(xyz, None, h, N, axes)[0]
        _check_sort(s, N, bc, xyz[order], None, 0)
        assert np.array_equal(SR.sort(xyz[order], None, h, N, axes)[0], ident)
        _check_sort(s, N, bc, xyz[order[::-1]], None, 0)
        _check_sort(s, N, bc, xyz[order[::-1]], None, 2, f32=True)
        # every particle dead; every particle lost: the original order
        dead = rng.choice([3, QR.FACE + 1, QR.INVALID], count).astype(np.int32)
        perm, counts = s.sort_tensor(_dev(xyz), _dev(dead))
        assert np.array_equal(_host(perm), ident) and _host(counts).tolist() == [0, 0]
        lost = np.full((count, 3), np.nan)
        lost[::2] = np.inf
        perm, counts = s.sort_tensor(_dev(lost), _dev(alive), shift=2)
        assert np.array_equal(_host(perm), ident) and _host(counts).tolist() == [0, count]


# -------------------------------------------------------------------------------------------------------------- 2 forms
@gpu
@pytest.mark.parametrize("N,bc", [(17, "per4_f15"), (65, "dirichlet")])
def test_sort_forms(N, bc):
    axes = QR.BCS[bc][0]
    count = 4099
    xyz, fate = SR.particles(N, bc, count)
    with _solver(N, bc) as s:
        h = s.h
        want, wc = SR.sort(xyz, fate, h, N, axes)
        pos, ft = _dev(xyz), _dev(fate)
        # (M, 3) tensors and three separate vectors
        perm, counts = s.sort_tensor(pos, ft)
        assert np.array_equal(_host(perm), want) and np.array_equal(_host(counts), wc)
        perm, counts = s.sort_tensor([pos[:, a].contiguous() for a in range(3)], ft)
        assert np.array_equal(_host(perm), want) and np.array_equal(_host(counts), wc)
        # strided slices of larger buffers: the gaps keep their sentinels
        big_x = torch.full((count, 7), SENTINEL, dtype=torch.float64, device="cuda")
        big_f = torch.full((2 * count + 1,), 5, dtype=torch.int32, device="cuda")
        big_p = torch.full((3 * count,), ISENT, dtype=torch.int32, device="cuda")
        big_x[:, 2:7:2], big_f[1::2] = pos, ft
        s.timing_enable(1)
        s.timing_reset()
        out, counts = s.sort_tensor(big_x[:, 2:7:2], big_f[1::2], out=big_p[1::3])
        assert _pack_count(s) == 1 + 3 * SR.passes(N, 0)
        hp = _host(big_p).reshape(count, 3)
        assert out.data_ptr() == big_p[1::3].data_ptr() and np.array_equal(hp[:, 1], want) and np.all(hp[:, [0, 2]] == ISENT)
        assert np.array_equal(_host(counts), wc)
        assert np.all(_host(big_x)[:, [0, 1, 3, 5]] == SENTINEL) and _same_bits(_host(big_x)[:, 2:7:2], xyz)
        assert np.all(_host(big_f)[0::2] == 5) and np.array_equal(_host(big_f)[1::2], fate)
        # a broadcast fate (stride 0): all alive, all dead
        for value in (0, 9):
            one = torch.tensor([value], dtype=torch.int32, device="cuda").expand(count)
            w, c = SR.sort(xyz, np.full(count, value, dtype=np.int32), h, N, axes, 2)
            perm, counts = s.sort_tensor(pos, one, shift=2)
            assert np.array_equal(_host(perm), w) and np.array_equal(_host(counts), c)
        # the host form: the bits of the device form
        keep = (xyz.copy(), fate.copy())
        gp, gc = s.sort(xyz, fate)
        assert gp.dtype == np.int32 and np.array_equal(gp, want) and gc == (int(wc[0]), int(wc[1]))
        gp, gc = s.sort(xyz, shift=2)
        w, c = SR.sort(xyz, None, h, N, axes, 2)
        assert np.array_equal(gp, w) and gc == (int(c[0]), int(c[1]))
        assert _same_bits(xyz, keep[0]) and np.array_equal(fate, keep[1])
        # no particle at all: nothing launched, the counts not written
        s.timing_reset()
        perm, counts = s.sort_tensor(pos[:0], ft[:0])
        assert perm.shape == (0,) and _pack_count(s) == 0 and _host(counts).tolist() == [0, 0]
        cd = torch.full((2,), 77, dtype=torch.int64, device="cuda")
        v = [mg3d_vec(0, MG3D_F64, 1)] * 3
        vp = C.POINTER(mg3d_vec)
        assert s.L.mg3d_particle_sort_device(s._h, 0, (vp * 3)(*[C.pointer(d) for d in v]), None, 0,
                                             C.byref(mg3d_vec(0, MG3D_I32, 1)), C.c_void_p(cd.data_ptr()), None) == 0
        assert _pack_count(s) == 0 and _host(cd).tolist() == [77, 77]
        gp, gc = s.sort(np.zeros((0, 3)))
        assert gp.shape == (0,) and gc == (0, 0)
        (empty,) = s.permute_tensors(perm, pos[:0])
        assert empty.shape == (0, 3) and _pack_count(s) == 0


@gpu
def test_permute_forms():
    N, count = 17, 4099
    rng = np.random.default_rng(99)
    with _solver(N, "dirichlet") as s:
        s.timing_enable(1)
        perm = rng.permutation(count).astype(np.int32)
        f64 = rng.uniform(-1, 1, (count, 3))
        f64[5] = (np.nan, -0.0, np.inf)
        f64.view(np.uint64)[6, 0] = 0x7FF4000000ABCDEF  # a signalling payload
        f32 = rng.uniform(-1, 1, (count, 3)).astype(np.float32)
        f32[7] = (np.float32(np.nan), np.float32(-0.0), -np.float32(np.inf))
        f32.view(np.uint32)[8, 1] = 0xFFA12345
        i32 = rng.integers(-2 ** 31, 2 ** 31 - 1, count).astype(np.int32)
        q = rng.uniform(-1, 1, count)
        qm = rng.uniform(-1, 1, count).astype(np.float32)
        host = [f64, f32, q, qm, i32]
        dev = [_dev(a) for a in host]
        assert _same_bits(_host(dev[0]), f64) and _same_bits(_host(dev[1]), f32)  # the payloads reached the device
        dp = _dev(perm)
        # nine vectors: one launch; fancy indexing bit for bit
        s.timing_reset()
        outs = s.permute_tensors(dp, *dev)
        assert _pack_count(s) == 1
        for o, t, a in zip(outs, dev, host):
            assert o.dtype == t.dtype and o.shape == t.shape and o.data_ptr() != t.data_ptr()
            assert _same_bits(_host(o), a[perm]) and _same_bits(_host(t), a)
        # sixteen vectors: one launch; seventeen: two
        s.timing_reset()
        outs = s.permute_tensors(dp, *([dev[0]] * 5 + [dev[2]]))
        assert _pack_count(s) == 1 and all(_same_bits(_host(o), f64[perm]) for o in outs[:5])
        assert _same_bits(_host(outs[5]), q[perm])
        s.timing_reset()
        outs = s.permute_tensors(dp, *([dev[1]] * 5 + [dev[4], dev[3]]))
        assert _pack_count(s) == 2 and all(_same_bits(_host(o), f32[perm]) for o in outs[:5])
        assert _same_bits(_host(outs[5]), i32[perm]) and _same_bits(_host(outs[6]), qm[perm])
        # views as sources: a transposed (3, M) buffer, a strided slice, a broadcast
        tr = _dev(np.ascontiguousarray(f64.T)).T
        wide = torch.full((2 * count,), ISENT, dtype=torch.int32, device="cuda")
        wide[::2] = dev[4]
        one = torch.tensor([2.5], dtype=torch.float32, device="cuda").expand(count)
        outs = s.permute_tensors(dp, tr, wide[::2], one)
        assert _same_bits(_host(outs[0]), f64[perm]) and _same_bits(_host(outs[1]), i32[perm])
        assert np.all(_host(outs[2]) == np.float32(2.5))
        # the C call with strided destinations whose gaps keep a sentinel; -1 and count in perm leave their element alone
        bad = perm.copy()
        bad[3], bad[count - 2] = -1, count
        dbad = torch.full((2 * count,), ISENT, dtype=torch.int32, device="cuda")
        dbad[1::2] = _dev(bad)
        big = [torch.full((count, 5), SENTINEL, dtype=torch.float64, device="cuda"),
               torch.full((3 * count,), -SENTINEL, dtype=torch.float32, device="cuda"),
               torch.full((2 * count + 1,), ISENT, dtype=torch.int32, device="cuda")]
        dst = [big[0][:, 1], big[0][:, 3], big[1][2::3], big[2][1::2]]
        src = [dev[0][:, 0], dev[0][:, 2], dev[3], dev[4]]
        codes = {torch.float64: MG3D_F64, torch.float32: MG3D_F32, torch.int32: MG3D_I32}

        def vec(t):
            return mg3d_vec(t.data_ptr(), codes[t.dtype], t.stride(0))

        vp = C.POINTER(mg3d_vec)
        vs, vd = [vec(t) for t in src], [vec(t) for t in dst]
        s.timing_reset()
        assert s.L.mg3d_particle_permute_device(s._h, count, C.byref(vec(dbad[1::2])), 4, (vp * 4)(*[C.pointer(d) for d in vs]),
                                                (vp * 4)(*[C.pointer(d) for d in vd]), None) == 0
        assert _pack_count(s) == 1
        ok = (bad >= 0) & (bad < count)
        safe = np.where(ok, bad, 0)
        h0, h1, h2 = _host(big[0]), _host(big[1]), _host(big[2])
        assert _same_bits(h0[:, 1], np.where(ok, f64[safe, 0], SENTINEL)) and _same_bits(h0[:, 3], np.where(ok, f64[safe, 2], SENTINEL))
        assert np.all(h0[:, [0, 2, 4]] == SENTINEL)
        assert _same_bits(h1[2::3], np.where(ok, qm[safe], np.float32(-SENTINEL)).astype(np.float32))
        assert np.all(h1.reshape(count, 3)[:, :2] == np.float32(-SENTINEL))
        assert _same_bits(h2[1::2], np.where(ok, i32[safe], ISENT).astype(np.int32)) and np.all(h2[0::2] == ISENT)
        assert np.array_equal(_host(dbad)[0::2], np.full(count, ISENT)) and (~ok).sum() == 2


# ---------------------------------------------------------------------------------------------------------------- 3 loop
@gpu
def test_loop_with_a_reorder_before_every_step():
    """five steps of deposit -> vcycles(3) -> push on a, and on b the same with sort and permute before every step: d after
    each deposit is the same (the deposit does not depend on the order), b's particles are a's under the accumulated
    permutation, the tables of fates are equal"""
    N, bc = 33, "dirichlet"
    axes, faces = QR.BCS[bc]
    h = SR.spacing(N)
    mask = QR.bodies(N)
    xyz, vel, _ = QR.particles(N, h, axes, 3000, 31 + N)
    M_ = xyz.shape[0]
    charge = np.random.default_rng(N).choice([-1.0, 1.0, 2.0], M_)
    qm = charge * (0.2 * h / (QR.DT * QR.DT))
    scale = -(h ** 3)
    with _solver(N, bc, mask) as a, _solver(N, bc, mask) as b:
        q = a.num_levels - 1
        for s in (a, b):
            s.set_mask_coarsening("keep")
            s.get_details()
        A = [_dev(xyz), _dev(vel), _dev(qm), _dev(charge), torch.zeros(M_, dtype=torch.int32, device="cuda")]
        B = [t.clone() for t in A]
        acc = np.arange(M_)
        moved = 0
        for step in range(5):
            perm, counts = b.sort_tensor(B[0], B[4], shift=step % 2)
            hp = _host(perm)
            want, wc = SR.sort(_host(B[0]), _host(B[4]), h, N, axes, step % 2)
            assert np.array_equal(hp, want) and np.array_equal(_host(counts), wc)
            B = list(b.permute_tensors(perm, *B))
            acc = acc[hp]
            moved += int(np.count_nonzero(hp != np.arange(M_)))
            for s, (pos, v, qt, ct, ft) in ((a, A), (b, B)):
                s.deposit_tensor(pos, torch.where(ft == 0, ct, torch.zeros_like(ct)), scale=scale)
            assert _same_bits(a.download(MG3D_D, q), b.download(MG3D_D, q)), step
            for s, (pos, v, qt, ct, ft) in ((a, A), (b, B)):
                s.vcycles(3)
                s.push_tensor(pos, v, qt, QR.DT, ft)
            for ta, tb in zip(A, B):
                assert _same_bits(_host(tb), _host(ta)[acc]), step
            assert _same_bits(a.download(MG3D_U, q), b.download(MG3D_U, q)), step
        fa = _host(A[4])
        assert np.array_equal(a.push_counts(), b.push_counts()) and a.push_counts().any()
        assert moved and (fa == 0).any() and (fa != 0).any()
        # the living first: b's fates are sorted into alive / lost-or-dead by the last reorder up to the last push
        assert sorted(acc.tolist()) == list(range(M_))


# --------------------------------------------------------------------------------------------------------------- 4 state
@gpu
def test_sort_behind_a_cycle_that_has_run_ahead_161():
    """a sorts behind vcycle(); b does nothing.  The next cycle of a has b's bits: norm, u and d"""
    N = 161
    c, L = SR.SIZES[N]
    q = L - 1
    rng = np.random.default_rng(163)
    u0, d0 = rng.uniform(-1, 1, (N, N, N)), rng.uniform(-1, 1, (N, N, N))
    xyz, fate = SR.particles(N, "dirichlet", 4099)
    with M.Solver(c, L, 2) as a, M.Solver(c, L, 2) as b:
        for s in (a, b):
            s.get_details()
            s.upload(MG3D_U, q, u0)
            s.upload(MG3D_D, q, d0)
            s.timing_enable(1)
            s.timing_reset()
        assert a.vcycle() == b.vcycle()
        assert (q, "leg_up") in a.kernel_times()  # the schedule that runs ahead did run
        perm, counts = a.sort_tensor(_dev(xyz), _dev(fate))
        (moved,) = a.permute_tensors(perm, _dev(xyz))
        want, wc = SR.sort(xyz, fate, a.h, N, 0)
        assert np.array_equal(_host(perm), want) and np.array_equal(_host(counts), wc)
        assert _same_bits(_host(moved), xyz[want])
        na, nb = a.vcycles(1), b.vcycles(1)
        assert na[0] == nb[0]
        assert _same_bits(a.download(MG3D_U, q), b.download(MG3D_U, q))
        assert _same_bits(a.download(MG3D_D, q).reshape(N, N, N), d0)


# ------------------------------------------------------------------------------------------------------------- 5 errors
@gpu
def test_refusals_leave_everything_untouched():
    N, count = 17, 300
    xyz, fate = SR.particles(N, "f63", count)
    with _solver(N, "f63") as s:
        L, h = s.L, s._h
        pos, ft = _dev(xyz), _dev(fate)
        perm = torch.full((count,), ISENT, dtype=torch.int32, device="cuda")
        counts = torch.full((2,), 77, dtype=torch.int64, device="cuda")
        good, _ = s.sort_tensor(pos, ft)  # one good sort first: the scratch exists
        vals = torch.full((count,), SENTINEL, dtype=torch.float64, device="cuda")
        outs = [torch.full((count,), -SENTINEL, dtype=torch.float64, device="cuda"),
                torch.full((count,), ISENT, dtype=torch.int32, device="cuda")]
        s.timing_enable(1)
        s.timing_reset()
        vp = C.POINTER(mg3d_vec)
        foreign = np.zeros(3 * count)
        foreign_counts = np.full(2, 77, dtype=np.int64)

        def vec(t, dtype=MG3D_F64, stride=None, ptr=None):
            return mg3d_vec(t.data_ptr() if ptr is None else ptr, dtype, t.stride(0) if stride is None else stride)

        def ptrs(descs):
            return (vp * len(descs))(*[C.pointer(d) if d is not None else vp() for d in descs])

        good_pos = [vec(pos[:, a]) for a in range(3)]
        good_f, good_p = vec(ft, dtype=MG3D_I32), vec(perm, dtype=MG3D_I32)

        def rc(ctx=h, n=count, p=good_pos, vf=good_f, shift=0, vperm=good_p, cd=counts.data_ptr()):
            return L.mg3d_particle_sort_device(ctx, n, ptrs(p) if p is not None else None,
                                               C.byref(vf) if vf is not None else None, shift,
                                               C.byref(vperm) if vperm is not None else None, C.c_void_p(cd), None)

        assert rc(ctx=None) == MG3D_ERR_ARG
        for bad in (-1, 9, 1 << 20):
            assert rc(shift=bad) == MG3D_ERR_ARG
        assert rc(n=-1) == MG3D_ERR_ARG and rc(n=1 << 31) == MG3D_ERR_ARG and rc(n=(1 << 40)) == MG3D_ERR_ARG
        assert rc(p=None) == MG3D_ERR_ARG and rc(p=[good_pos[0], None, good_pos[2]]) == MG3D_ERR_ARG
        for bv in (vec(pos[:, 1], dtype=MG3D_I32), vec(pos[:, 1], dtype=2), vec(pos[:, 1], stride=-3),
                   vec(pos[:, 1], ptr=foreign.ctypes.data), vec(pos[:, 1], ptr=0)):
            assert rc(p=[good_pos[0], bv, good_pos[2]]) == MG3D_ERR_ARG
        for bv in (vec(ft, dtype=MG3D_F32), vec(ft, dtype=MG3D_F64), vec(ft, dtype=MG3D_I32, stride=-1),
                   vec(ft, dtype=MG3D_I32, ptr=foreign.ctypes.data)):
            assert rc(vf=bv) == MG3D_ERR_ARG
        assert rc(vperm=None) == MG3D_ERR_ARG
        for bv in (vec(perm, dtype=MG3D_F64), vec(perm, dtype=MG3D_F32), vec(perm, dtype=MG3D_I32, stride=0),
                   vec(perm, dtype=MG3D_I32, stride=-1), vec(perm, dtype=MG3D_I32, ptr=foreign.ctypes.data),
                   vec(perm, dtype=MG3D_I32, ptr=0)):
            assert rc(vperm=bv) == MG3D_ERR_ARG
        assert rc(cd=foreign_counts.ctypes.data) == MG3D_ERR_ARG
        # the permute
        dperm = vec(good, dtype=MG3D_I32)
        src = [vec(vals), vec(ft, dtype=MG3D_I32)]
        dst = [vec(outs[0]), vec(outs[1], dtype=MG3D_I32)]

        def rp(ctx=h, n=count, vperm=dperm, nvec=2, vs=src, vd=dst):
            return L.mg3d_particle_permute_device(ctx, n, C.byref(vperm) if vperm is not None else None, nvec,
                                                  ptrs(vs) if vs is not None else None,
                                                  ptrs(vd) if vd is not None else None, None)

        many_s, many_d = [src[0]] * 17, [dst[0]] * 17
        assert rp(ctx=None) == MG3D_ERR_ARG and rp(vperm=None) == MG3D_ERR_ARG
        assert rp(nvec=0) == MG3D_ERR_ARG and rp(nvec=-1) == MG3D_ERR_ARG
        assert rp(nvec=17, vs=many_s, vd=many_d) == MG3D_ERR_ARG
        assert rp(n=-1) == MG3D_ERR_ARG and rp(n=1 << 31) == MG3D_ERR_ARG
        assert rp(vs=None) == MG3D_ERR_ARG and rp(vd=None) == MG3D_ERR_ARG
        assert rp(vs=[src[0], None]) == MG3D_ERR_ARG and rp(vd=[None, dst[1]]) == MG3D_ERR_ARG
        assert rp(vperm=vec(good, dtype=MG3D_F32)) == MG3D_ERR_ARG and rp(vperm=vec(good, dtype=MG3D_I32, stride=-1)) == MG3D_ERR_ARG
        assert rp(vperm=vec(good, dtype=MG3D_I32, ptr=foreign.ctypes.data)) == MG3D_ERR_ARG
        # a dtype mismatch in a pair, a dtype that is none of the three, bad strides, foreign pointers
        assert rp(vd=[vec(outs[0], dtype=MG3D_F32), dst[1]]) == MG3D_ERR_ARG
        assert rp(vs=[src[0], vec(ft, dtype=MG3D_F32)]) == MG3D_ERR_ARG
        assert rp(vs=[vec(vals, dtype=2), src[1]], vd=[vec(outs[0], dtype=2), dst[1]]) == MG3D_ERR_ARG
        assert rp(vd=[vec(outs[0], stride=0), dst[1]]) == MG3D_ERR_ARG
        assert rp(vd=[dst[0], vec(outs[1], dtype=MG3D_I32, stride=0)]) == MG3D_ERR_ARG
        assert rp(vs=[vec(vals, stride=-1), src[1]]) == MG3D_ERR_ARG
        assert rp(vs=[vec(vals, ptr=foreign.ctypes.data), src[1]]) == MG3D_ERR_ARG
        assert rp(vd=[dst[0], vec(outs[1], dtype=MG3D_I32, ptr=foreign.ctypes.data)]) == MG3D_ERR_ARG
        # the host form
        hx = np.ascontiguousarray(xyz).reshape(-1)
        hp = np.full(count, ISENT, dtype=np.int32)
        hc = (C.c_longlong * 2)(77, 77)
        ip = C.POINTER(C.c_int)
        assert L.mg3d_particle_sort(None, count, P(hx), None, 0, hp.ctypes.data_as(ip), hc) == MG3D_ERR_ARG
        assert L.mg3d_particle_sort(h, count, None, None, 0, hp.ctypes.data_as(ip), hc) == MG3D_ERR_ARG
        assert L.mg3d_particle_sort(h, count, P(hx), None, 0, None, hc) == MG3D_ERR_ARG
        assert L.mg3d_particle_sort(h, count, P(hx), None, 9, hp.ctypes.data_as(ip), hc) == MG3D_ERR_ARG
        assert L.mg3d_particle_sort(h, -1, P(hx), None, 0, hp.ctypes.data_as(ip), hc) == MG3D_ERR_ARG
        assert L.mg3d_particle_sort(h, 1 << 31, P(hx), None, 0, hp.ctypes.data_as(ip), hc) == MG3D_ERR_ARG
        assert np.all(hp == ISENT) and list(hc) == [77, 77]
        # the tensor forms: wrong devices, shapes and types
        with pytest.raises(ValueError):
            s.sort_tensor(pos.cpu(), ft)
        with pytest.raises(ValueError):
            s.sort_tensor(pos, ft[:-1])
        with pytest.raises(ValueError):
            s.sort_tensor(pos, ft.cpu())
        with pytest.raises(TypeError):
            s.sort_tensor(pos, ft.to(torch.int64))
        with pytest.raises(TypeError):
            s.sort_tensor(pos, ft, out=perm.to(torch.int64))
        with pytest.raises(ValueError):
            s.sort_tensor(pos, ft, out=perm[:1].expand(count))
        with pytest.raises(M.Mg3dError) as e:
            s.sort_tensor(pos, ft, shift=9)
        assert e.value.code == MG3D_ERR_ARG
        with pytest.raises(TypeError):
            s.permute_tensors(good.to(torch.int64), vals)
        with pytest.raises(TypeError):
            s.permute_tensors(good, vals.to(torch.float16))
        with pytest.raises(ValueError):
            s.permute_tensors(good, vals[:-1])
        with pytest.raises(ValueError):
            s.permute_tensors(good, vals.cpu())
        # every refusal left perm, the counts, the outputs and the launch counts as they were
        assert _pack_count(s) == 0 and not foreign.any() and np.all(foreign_counts == 77)
        assert np.all(_host(perm) == ISENT) and _host(counts).tolist() == [77, 77]
        assert np.all(_host(outs[0]) == -SENTINEL) and np.all(_host(outs[1]) == ISENT)
        assert _same_bits(_host(pos), xyz) and np.array_equal(_host(ft), fate) and np.all(_host(vals) == SENTINEL)
        assert M.MG3D_PERMUTE_MAX_VECS == 16
