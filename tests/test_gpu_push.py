"""The particle mover on the GPU -- mg3d_particle_push(_device), mg3d_particle_counts -- against the numpy restatement
tests/_push_ref.py, bit for bit.

1  bits: random u at every point, the seeded points and the edge points of the sample's tests with random velocities, on
   every boundary set, N = 5 (c = 5, L = 1), 17, 37 and 65, counts 1, 255, 256, 257, 4099 and one past the grid cap, with
   and without a mask of two bodies labelled 3 and 200: positions, velocities, fates and the table of counts after each of
   twenty pushes in sequence (three past the cap); the particles shuffled: the outputs permuted, the counts the same.
   tests/test_push_ref_host.py holds these cases to their coverage: every exit, reflection, wrap, label, INVALID, survivors.
2  forms: (M, 3) tensors and three vectors, float32 velocities and q/m, a broadcast q/m, strided slices of larger buffers
   whose gaps keep a sentinel, particles dead on entry, the host form, no particle at all, one launch per call.
3  the loop: five steps of deposit, three cycles and push against the same loop with the push restated on the downloaded u.
4  state at 161^3: behind a cycle that has run ahead the push sees the finished cycle and the next cycle goes on as if it
   had not been made.
5  arguments: every refusal leaves the vectors, the table and the launch counts untouched; MG3D_I32 is the fate's alone."""
import ctypes as C

import numpy as np
import pytest
import torch  # before the package, as bench.py does: the HIP runtime is torch's

import _particle_ref as PR
import _push_ref as QR
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import (MG3D_D, MG3D_F32, MG3D_F64, MG3D_I32, MG3D_U, P, mg3d_array, mg3d_push_params,
                                            mg3d_vec)

gpu = pytest.mark.gpu

MG3D_ERR_ARG = 1
SENTINEL = 12345.678
# N: (c, L); a periodic axis needs an even c - 1: 37 = 18 * 2 + 1 there
SIZES = {5: (5, 1), 17: (5, 3), 33: (5, 4), 37: (10, 3), 65: (5, 5), 161: (6, 6)}
PERIODIC_37 = (19, 2)


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


def _solver(N, bc, mask=None):
    axes, faces = QR.BCS[bc]
    c, L = PERIODIC_37 if N == 37 and axes else SIZES[N]
    s = M.Solver(c, L, 2)
    assert s.N == N and s.h == QR.spacing(N)
    s.set_periodic(axes)
    s.set_neumann(faces)
    if mask is not None:
        s.set_mask(mask)
    return s


def _pack_count(s):
    s.sync()
    return s.kernel_times().get((s.num_levels - 1, "pack"), (0, 0.))[0]


def _counts_equal(got, want):
    return got.dtype == np.uint64 and got.shape == (QR.SLOTS,) and np.array_equal(got, want)


# --------------------------------------------------------------------------------------------------------------- 1 bits
@gpu
@pytest.mark.parametrize("N,bc,count,with_mask,pushes", QR.CASES)
def test_push_bits(N, bc, count, with_mask, pushes):
    u, mask, xyz, vel, qm, accel, drag = QR.case_data(N, bc, count, with_mask)
    want = QR.run_case(N, bc, count, with_mask, pushes)
    M_ = xyz.shape[0]
    perm = np.random.default_rng(N + count).permutation(M_)
    with _solver(N, bc, mask) as s, _solver(N, bc, mask) as other:
        q = s.num_levels - 1
        assert not s.push_counts().any()  # all zero before the first push
        for t in (s, other):
            t.upload(MG3D_U, q, u)
        s.timing_enable(1)
        s.timing_reset()
        pos, v, fate = _dev(xyz), _dev(vel), torch.zeros(M_, dtype=torch.int32, device="cuda")
        pos2, v2, fate2 = _dev(xyz[perm]), _dev(vel[perm]), torch.zeros(M_, dtype=torch.int32, device="cuda")
        qt, qt2 = _dev(qm), _dev(qm[perm])
        for n, (wx, wv, wf, wt) in enumerate(want):
            s.push_tensor(pos, v, qt, QR.DT, fate, scale=-1.0, accel=accel, drag=drag)
            assert _pack_count(s) == n + 1  # one launch per call, counted with the array I/O
            gx, gv, gf = _host(pos), _host(v), _host(fate)
            assert np.array_equal(gf, wf), (N, bc, n, np.argwhere(gf != wf)[:4])
            assert _same_bits(gx, wx), (N, bc, n, np.argwhere(gx != wx)[:4])
            assert _same_bits(gv, wv), (N, bc, n, np.argwhere(gv != wv)[:4])
            assert _counts_equal(s.push_counts(), wt)
            # the particles shuffled, on another context: the outputs permuted, the counts the same
            other.push_tensor(pos2, v2, qt2, QR.DT, fate2, scale=-1.0, accel=accel, drag=drag)
        assert np.array_equal(_host(fate2), wf[perm]) and _same_bits(_host(pos2), wx[perm]) and _same_bits(_host(v2), wv[perm])
        assert _counts_equal(other.push_counts(), wt)
        # reset: the copy first, zeros behind it
        assert _counts_equal(s.push_counts(reset=True), wt) and not s.push_counts().any()
        assert _same_bits(s.download(MG3D_U, q).reshape(N, N, N), u)


# -------------------------------------------------------------------------------------------------------------- 2 forms
@gpu
@pytest.mark.parametrize("N,bc,with_mask", [(17, "per4_f15", True), (37, "dirichlet", False)])
def test_push_forms(N, bc, with_mask):
    axes, faces = QR.BCS[bc]
    u, mask, xyz, vel, qm, accel, drag = QR.case_data(N, bc, 300, with_mask)
    M_ = xyz.shape[0]
    h = QR.spacing(N)
    zero = np.zeros(M_, dtype=np.int32)

    def ref(vel_=vel, qm_=qm, fate_=zero, table=None):
        return QR.push(u, mask, xyz, vel_, qm_, fate_, h, axes, faces, QR.DT, -1.0, accel, drag, table)

    wx, wv, wf = ref()
    kw = dict(scale=-1.0, accel=accel, drag=drag)
    with _solver(N, bc, mask) as s:
        s.upload(MG3D_U, s.num_levels - 1, u)

        def fresh():
            return _dev(xyz), _dev(vel), torch.zeros(M_, dtype=torch.int32, device="cuda")

        # (M, 3) tensors
        pos, v, fate = fresh()
        s.push_tensor(pos, v, _dev(qm), QR.DT, fate, **kw)
        assert _same_bits(_host(pos), wx) and _same_bits(_host(v), wv) and np.array_equal(_host(fate), wf)
        # three vectors each
        pos, v, fate = fresh()
        px, pv = [pos[:, a].contiguous() for a in range(3)], [v[:, a].contiguous() for a in range(3)]
        s.push_tensor(px, pv, _dev(qm), QR.DT, fate, **kw)
        assert _same_bits(np.stack([_host(t) for t in px], axis=1), wx)
        assert _same_bits(np.stack([_host(t) for t in pv], axis=1), wv) and np.array_equal(_host(fate), wf)
        # float32 velocities and q/m: widened exactly on the way in, rounded to nearest even on the way out
        with np.errstate(over="ignore", invalid="ignore"):
            vel32, qm32 = vel.astype(np.float32), qm.astype(np.float32)
        w32x, w32v, w32f = ref(vel32, qm32)
        pos, _, fate = fresh()
        v32 = _dev(vel32, torch.float32)
        s.push_tensor(pos, v32, _dev(qm32, torch.float32), QR.DT, fate, **kw)
        assert w32v.dtype == np.float32 and _same_bits(_host(v32), w32v)
        assert _same_bits(_host(pos), w32x) and np.array_equal(_host(fate), w32f)
        # a broadcast q/m: a Python float, and an expanded tensor
        one = 0.01 * h * h / (QR.DT * QR.DT)
        bx, bv, bf = ref(qm_=one)
        for form in (one, torch.tensor([one], dtype=torch.float64, device="cuda").expand(M_)):
            pos, v, fate = fresh()
            s.push_tensor(pos, v, form, QR.DT, fate, **kw)
            assert _same_bits(_host(pos), bx) and _same_bits(_host(v), bv) and np.array_equal(_host(fate), bf)
        # strided slices of larger buffers: the gaps keep their sentinels; particles dead on entry keep theirs too
        dead = np.zeros(M_, dtype=bool)
        dead[::7] = True
        entry = np.where(dead, 5, 0).astype(np.int32)
        entry[14] = QR.FACE + 3
        entry[21] = QR.INVALID
        sx, sv = xyz.copy(), vel.copy()
        sx[dead], sv[dead] = SENTINEL, -SENTINEL
        table = QR.new_table()
        dx, dv, dfate = QR.push(u, mask, sx, sv, qm, entry, h, axes, faces, QR.DT, -1.0, accel, drag, table)
        assert np.all(dx[dead] == SENTINEL) and np.all(dv[dead] == -SENTINEL) and np.array_equal(dfate[dead], entry[dead])
        big_x = torch.full((M_, 7), SENTINEL, dtype=torch.float64, device="cuda")
        big_v = torch.full((2 * M_, 4), -SENTINEL, dtype=torch.float64, device="cuda")
        big_f = torch.full((2 * M_ + 1,), -7, dtype=torch.int32, device="cuda")
        big_q = torch.full((3 * M_,), SENTINEL, dtype=torch.float64, device="cuda")
        big_x[:, 2:7:2], big_v[::2, 1:4], big_f[1::2], big_q[::3] = _dev(sx), _dev(sv), _dev(entry, torch.int32), _dev(qm)
        s.push_counts(reset=True)
        s.timing_enable(1)
        s.timing_reset()
        s.push_tensor(big_x[:, 2:7:2], big_v[::2, 1:4], big_q[::3], QR.DT, big_f[1::2], **kw)
        assert _pack_count(s) == 1
        hx, hv, hf, hq = _host(big_x), _host(big_v), _host(big_f), _host(big_q)
        assert _same_bits(hx[:, 2:7:2], dx) and np.all(hx[:, [0, 1, 3, 5]] == SENTINEL)
        assert _same_bits(hv[::2, 1:4], dv) and np.all(hv[1::2] == -SENTINEL) and np.all(hv[:, 0] == -SENTINEL)
        assert np.array_equal(hf[1::2], dfate) and np.all(hf[0::2] == -7)
        assert np.all(hq.reshape(M_, 3)[:, 1:] == SENTINEL)
        assert _counts_equal(s.push_counts(), table)  # the dead are not counted again
        # the host form: the bits of the device form, new arrays
        s.push_counts(reset=True)
        keep = (xyz.copy(), vel.copy())
        table = QR.new_table()
        wx, wv, wf = ref(table=table)
        gx, gv, gf = s.push(xyz, vel, qm, QR.DT, **kw)
        assert _same_bits(gx, wx) and _same_bits(gv, wv) and gf.dtype == np.int32 and np.array_equal(gf, wf)
        assert _same_bits(xyz, keep[0]) and _same_bits(vel, keep[1]) and _counts_equal(s.push_counts(), table)
        gx, gv, gf = s.push(sx, sv, qm, QR.DT, fate=entry, **kw)
        assert _same_bits(gx, dx) and _same_bits(gv, dv) and np.array_equal(gf, dfate)
        # no particle at all: nothing launched
        s.timing_reset()
        pos, v, fate = fresh()
        s.push_tensor(pos[:0], v[:0], _dev(qm)[:0], QR.DT, fate[:0], **kw)
        assert _pack_count(s) == 0 and _same_bits(_host(pos), xyz) and not _host(fate).any()


# ---------------------------------------------------------------------------------------------------------------- 3 loop
@gpu
@pytest.mark.parametrize("N,bc,with_mask", [(17, "dirichlet", True), (33, "f22", False)])
def test_loop_of_deposit_cycles_and_push(N, bc, with_mask):
    """five steps of deposit -> vcycles(3) -> push on a, and on b the same with the push restated on the downloaded u: the
    particles and u agree bit for bit after every step"""
    axes, faces = QR.BCS[bc]
    h = QR.spacing(N)
    mask = QR.bodies(N) if with_mask else None
    xyz, vel, _ = QR.particles(N, h, axes, 300, 31 + N)
    M_ = xyz.shape[0]
    charge = np.random.default_rng(N).choice([-1.0, 1.0, 2.0], M_)
    qm = charge * (0.2 * h / (QR.DT * QR.DT))
    scale = -(h ** 3)
    fate = np.zeros(M_, dtype=np.int32)
    with _solver(N, bc, mask) as a, _solver(N, bc, mask) as b:
        q = a.num_levels - 1
        for s in (a, b):
            if with_mask:
                s.set_mask_coarsening("keep")
            s.get_details()
        pos, v, ft, qt, ct = _dev(xyz), _dev(vel), _dev(fate, torch.int32), _dev(qm), _dev(charge)
        for step in range(5):
            a.deposit_tensor(pos, torch.where(ft == 0, ct, torch.zeros_like(ct)), scale=scale)
            a.vcycles(3)
            a.push_tensor(pos, v, qt, QR.DT, ft)
            b.deposit(xyz, np.where(fate == 0, charge, 0.0), scale=scale)
            b.vcycles(3)
            ub = b.download(MG3D_U, q).reshape(N, N, N)
            xyz, vel, fate = QR.push(ub, mask, xyz, vel, qm, fate, h, axes, faces, QR.DT)
            assert np.array_equal(_host(ft), fate), step
            assert _same_bits(_host(pos), xyz) and _same_bits(_host(v), vel), step
            assert _same_bits(a.download(MG3D_U, q).reshape(N, N, N), ub), step
        assert ub.any() and (fate == 0).any()


# --------------------------------------------------------------------------------------------------------------- 4 state
@gpu
def test_push_behind_a_cycle_that_has_run_ahead_161():
    """a pushes behind vcycle() and does nothing else; b downloads instead, which is known to read only.  The push is the
    restatement's on the finished cycle's u, and the next cycle of a has b's bits: norm, u and d"""
    N = 161
    c, L = SIZES[N]
    q = L - 1
    rng = np.random.default_rng(163)
    u0, d0 = rng.uniform(-1, 1, (N, N, N)), rng.uniform(-1, 1, (N, N, N))
    with M.Solver(c, L, 2) as a, M.Solver(c, L, 2) as b:
        xyz, vel, qm = QR.particles(N, a.h, 0, 1000, 8)
        for s in (a, b):
            s.get_details()
            s.upload(MG3D_U, q, u0)
            s.upload(MG3D_D, q, d0)
            s.timing_enable(1)
            s.timing_reset()
        assert a.vcycle() == b.vcycle()
        assert (q, "leg_up") in a.kernel_times()  # the schedule that runs ahead did run
        pos, v, fate = _dev(xyz), _dev(vel), torch.zeros(xyz.shape[0], dtype=torch.int32, device="cuda")
        a.push_tensor(pos, v, _dev(qm), QR.DT, fate)
        u = b.download(MG3D_U, q).reshape(N, N, N)
        table = QR.new_table()
        wx, wv, wf = QR.push(u, None, xyz, vel, qm, np.zeros(xyz.shape[0], dtype=np.int32), a.h, 0, 0, QR.DT, table=table)
        assert _same_bits(_host(pos), wx) and _same_bits(_host(v), wv) and np.array_equal(_host(fate), wf)
        assert _counts_equal(a.push_counts(), table) and (wf == 0).any() and (wf != 0).any()
        na, nb = a.vcycles(1), b.vcycles(1)
        assert na[0] == nb[0]
        assert _same_bits(a.download(MG3D_U, q), b.download(MG3D_U, q))
        assert _same_bits(a.download(MG3D_D, q).reshape(N, N, N), d0)


# ------------------------------------------------------------------------------------------------------------- 5 errors
@gpu
def test_refusals_leave_everything_untouched():
    N, M_ = 17, 40
    u = QR.field(N, 51)
    with _solver(N, "f63", QR.bodies(N)) as s:
        q = s.num_levels - 1
        L, h = s.L, s._h
        s.upload(MG3D_U, q, u)
        xyz = PR.box_points(N, s.h, M_, 53)
        pos, v = _dev(xyz), torch.full((M_, 3), 0.25, dtype=torch.float64, device="cuda")
        qt = torch.full((M_,), 0.5, dtype=torch.float64, device="cuda")
        fate = torch.zeros(M_, dtype=torch.int32, device="cuda")
        # one good push first, of one particle whose position is not finite: the table exists and holds something
        pos[0, 0] = float("nan")
        s.push_tensor(pos, v, qt, 0.01, fate)
        before = s.push_counts()
        assert before[QR.INVALID] == 1
        fate.zero_()
        pos.copy_(_dev(xyz))
        keep = [_host(t).copy() for t in (pos, v, qt, fate)]
        s.timing_enable(1)
        s.timing_reset()
        vp = C.POINTER(mg3d_vec)

        def vec(t, dtype=MG3D_F64, stride=None, ptr=None):
            return mg3d_vec(t.data_ptr() if ptr is None else ptr, dtype, t.stride(0) if stride is None else stride)

        def ptrs(descs):
            return (vp * 3)(*[C.pointer(d) if d is not None else vp() for d in descs])

        good_pos, good_vel = [vec(pos[:, a]) for a in range(3)], [vec(v[:, a]) for a in range(3)]
        good_q, good_f = vec(qt), vec(fate, dtype=MG3D_I32)
        good_p = mg3d_push_params(0.01, -1.0, (C.c_double * 3)(0., 0., 0.), 0.0)
        foreign = np.zeros(3 * M_)

        def rc(ctx=h, count=M_, p=good_pos, w=good_vel, vq=good_q, vf=good_f, par=good_p):
            return L.mg3d_particle_push_device(ctx, count, ptrs(p) if p is not None else None,
                                               ptrs(w) if w is not None else None, C.byref(vq) if vq is not None else None,
                                               C.byref(vf) if vf is not None else None,
                                               C.byref(par) if par is not None else None, None)

        def params(dt=0.01, scale=-1.0, accel=(0., 0., 0.), drag=0.0):
            return mg3d_push_params(dt, scale, (C.c_double * 3)(*accel), drag)

        nan, inf = float("nan"), float("inf")
        assert rc(ctx=None) == MG3D_ERR_ARG and rc(p=None) == MG3D_ERR_ARG and rc(w=None) == MG3D_ERR_ARG
        assert rc(vq=None) == MG3D_ERR_ARG and rc(vf=None) == MG3D_ERR_ARG and rc(par=None) == MG3D_ERR_ARG
        assert rc(count=-1) == MG3D_ERR_ARG and rc(count=(1 << 40) + 1) == MG3D_ERR_ARG
        for bad in (0.0, -0.01, nan, inf, -inf):
            assert rc(par=params(dt=bad)) == MG3D_ERR_ARG
        for bad in (nan, inf, -inf):
            assert rc(par=params(scale=bad)) == MG3D_ERR_ARG
            assert rc(par=params(drag=bad)) == MG3D_ERR_ARG
            for a in range(3):
                acc = [0., 0., 0.]
                acc[a] = bad
                assert rc(par=params(accel=acc)) == MG3D_ERR_ARG
        assert rc(par=params(drag=-1e-300)) == MG3D_ERR_ARG
        bad_vectors = [vec(pos[:, 1], dtype=7), vec(pos[:, 1], dtype=2), vec(pos[:, 1], dtype=MG3D_I32),
                       vec(pos[:, 1], stride=-3), vec(pos[:, 1], stride=0), vec(pos[:, 1], ptr=foreign.ctypes.data),
                       vec(pos[:, 1], ptr=0)]
        for bv in bad_vectors:
            assert rc(p=[good_pos[0], bv, good_pos[2]]) == MG3D_ERR_ARG
            assert rc(w=[good_vel[0], good_vel[1], bv]) == MG3D_ERR_ARG
        assert rc(p=[good_pos[0], vec(pos[:, 1], dtype=MG3D_F32), good_pos[2]]) == MG3D_ERR_ARG  # positions: float64 only
        assert rc(p=[good_pos[0], good_pos[1], None]) == MG3D_ERR_ARG and rc(w=[None, good_vel[1], good_vel[2]]) == MG3D_ERR_ARG
        for bv in (vec(qt, dtype=7), vec(qt, dtype=2), vec(qt, dtype=MG3D_I32), vec(qt, stride=-1),
                   vec(qt, ptr=foreign.ctypes.data), vec(qt, ptr=0)):
            assert rc(vq=bv) == MG3D_ERR_ARG
        for bv in (vec(fate, dtype=MG3D_F32), vec(fate, dtype=MG3D_F64), vec(fate, dtype=2), vec(fate, dtype=4),
                   vec(fate, dtype=MG3D_I32, stride=0), vec(fate, dtype=MG3D_I32, stride=-1),
                   vec(fate, dtype=MG3D_I32, ptr=foreign.ctypes.data), vec(fate, dtype=MG3D_I32, ptr=0)):
            assert rc(vf=bv) == MG3D_ERR_ARG
        # the host form and the counts
        hx, hv, hq = np.ascontiguousarray(xyz).reshape(-1), np.full(3 * M_, 0.25), np.full(M_, 0.5)
        hf = np.zeros(M_, dtype=np.int32)
        pf = hf.ctypes.data_as(C.POINTER(C.c_int))
        gp = C.byref(good_p)
        assert L.mg3d_particle_push(None, M_, P(hx), P(hv), P(hq), pf, gp) == MG3D_ERR_ARG
        assert L.mg3d_particle_push(h, M_, None, P(hv), P(hq), pf, gp) == MG3D_ERR_ARG
        assert L.mg3d_particle_push(h, M_, P(hx), None, P(hq), pf, gp) == MG3D_ERR_ARG
        assert L.mg3d_particle_push(h, M_, P(hx), P(hv), None, pf, gp) == MG3D_ERR_ARG
        assert L.mg3d_particle_push(h, M_, P(hx), P(hv), P(hq), None, gp) == MG3D_ERR_ARG
        assert L.mg3d_particle_push(h, M_, P(hx), P(hv), P(hq), pf, None) == MG3D_ERR_ARG
        assert L.mg3d_particle_push(h, -1, P(hx), P(hv), P(hq), pf, gp) == MG3D_ERR_ARG
        assert L.mg3d_particle_push(h, M_, P(hx), P(hv), P(hq), pf, C.byref(params(dt=nan))) == MG3D_ERR_ARG
        assert np.array_equal(hx, np.ascontiguousarray(xyz).reshape(-1)) and np.all(hv == 0.25) and not hf.any()
        out = (C.c_ulonglong * QR.SLOTS)(*([7] * QR.SLOTS))
        assert L.mg3d_particle_counts(None, out, 0) == MG3D_ERR_ARG and L.mg3d_particle_counts(h, None, 1) == MG3D_ERR_ARG
        assert list(out) == [7] * QR.SLOTS
        # MG3D_I32 is the fate's alone: the sample, the deposit and the mg3d_array calls keep refusing it
        ou = torch.full((M_,), SENTINEL, dtype=torch.float64, device="cuda")
        i32 = vec(fate, dtype=MG3D_I32)
        assert L.mg3d_field_sample_device(h, M_, ptrs([good_pos[0], vec(pos[:, 1], dtype=MG3D_I32), good_pos[2]]), 1.0,
                                          C.byref(vec(ou)), None, None) == MG3D_ERR_ARG
        assert L.mg3d_field_sample_device(h, M_, ptrs(good_pos), 1.0, C.byref(i32), None, None) == MG3D_ERR_ARG
        assert L.mg3d_deposit_device(h, M_, ptrs(good_pos), C.byref(i32), 1.0, None) == MG3D_ERR_ARG
        cube = torch.zeros((N, N, N), dtype=torch.float32, device="cuda")
        arr = mg3d_array(cube.data_ptr(), MG3D_I32, (C.c_longlong * 3)(N * N, N, 1))
        assert L.mg3d_upload_device(h, MG3D_D, q, C.byref(arr), None) == MG3D_ERR_ARG
        assert L.mg3d_download_device(h, MG3D_U, q, C.byref(arr), None) == MG3D_ERR_ARG
        assert L.mg3d_ctx_set_mask_device(h, C.byref(arr), None) == MG3D_ERR_ARG
        assert L.mg3d_ctx_set_coefficient_device(h, C.byref(arr), None) == MG3D_ERR_ARG
        ap = C.POINTER(mg3d_array)
        assert L.mg3d_field_gradient_device(h, 1.0, (ap * 3)(C.pointer(arr), ap(), ap()), None) == MG3D_ERR_ARG
        # the tensor forms: wrong devices, shapes and types
        with pytest.raises(ValueError):
            s.push_tensor(pos.cpu(), v, qt, 0.01, fate)
        with pytest.raises(ValueError):
            s.push_tensor(pos, v[:-1], qt, 0.01, fate)
        with pytest.raises(ValueError):
            s.push_tensor(pos, v, qt[:-1], 0.01, fate)
        with pytest.raises(ValueError):
            s.push_tensor(pos, v, qt, 0.01, fate[:-1])
        with pytest.raises(ValueError):
            s.push_tensor(pos, v, qt, 0.01, fate.cpu())
        with pytest.raises(ValueError):
            s.push_tensor(pos, v, qt, 0.01, fate[:1].expand(M_))
        with pytest.raises(TypeError):
            s.push_tensor(pos.to(torch.float32), v, qt, 0.01, fate)
        with pytest.raises(TypeError):
            s.push_tensor(pos, v, qt, 0.01, fate.to(torch.int64))
        with pytest.raises(TypeError):
            s.push_tensor(pos, v.to(torch.float16), qt, 0.01, fate)
        with pytest.raises(M.Mg3dError) as e:
            s.push_tensor(pos, v, qt, -0.01, fate)
        assert e.value.code == MG3D_ERR_ARG
        # every refusal left the vectors, the table, u and the launch counts as they were
        assert _pack_count(s) == 0 and not foreign.any() and bool(torch.all(ou == SENTINEL))
        for t, k in zip((pos, v, qt, fate), keep):
            assert _same_bits(_host(t), k)
        assert np.array_equal(s.push_counts(), before)
        assert _same_bits(s.download(MG3D_U, q).reshape(N, N, N), u)
        assert M.MG3D_FATE_ALIVE == 0 and M.MG3D_FATE_FACE == 256 and M.MG3D_FATE_INVALID == 262 and M.MG3D_FATE_SLOTS == 263
