"""The particle calls on boxes other than the unit cube (grid_length 3e-4, the electrospray's own, and 3.0) --
mg3d_field_sample(_device), mg3d_deposit(_device), mg3d_particle_push(_device), mg3d_particle_sort(_device),
mg3d_particle_permute_device -- against the restatements tests/_particle_ref.py, _push_ref.py and _sort_ref.py called with
this length's h = grid_length / (N - 1), bit for bit.  Sizes 21, 37, 41 and 65: at these h is no power of two and a
coordinate formed as i*h locates, at some nodes, in cell i - 1 with w1 just below 1 (tests/_length_cases.LOW_NODES);
_particle_ref.node_points_all puts a point on every node of every axis and one ulp to either side of it.  The matrix is
pruned: every boundary set meets both lengths, the sizes rotate (tests/_length_cases.particle_cases).
tests/test_particle_length_host.py holds these cases to their coverage and the restatements to the scaling identity.

1  sample: random u at every point, seeded points, the edge points and the node points, the scales of
   LC.PARTICLE_GRAD_SCALES (scale * (0.5 / h) and scale / (2 h) round apart wherever a scale can tell them apart);
   float32 positions and outputs; eps and a mask set; one count past the grid cap.
2  deposit onto a random d in (-50, 50) / length^2, charges of both signs over 12 decades, the duplicates of d, the launch
   counts; all-zero q.
3  push: three pushes in sequence, positions, velocities, fates and the table after each; float32 velocities; a loop of
   deposit, two cycles and push on a 3e-4 box against the same loop with the push restated on the downloaded u.
4  sort and permute: the permutation and both counts at shift 0 and 2, nine vectors of mixed type permuted in one launch, a
   loop of push, sort and permute.
5  the scaling identity between GPU runs at 41^3 with a periodic axis and Neumann faces (m = 2, -3): positions,
   velocities and accel times s = 2^m, q/m times s^2, the deposit's scale times s, d over s^2 -- the same sampled u, the
   gradient 2^-m times, positions and velocities s times, the same fates, table and permutation, d s^-2 times.
Every context reports h = length / (N - 1) and level spacings that double exactly (_assert_spacings)."""
import numpy as np
import pytest
import torch  # before the package, as bench.py does: the HIP runtime is torch's

import _coef_ref as CR
import _field_ref as FR
import _length_cases as LC
import _mask_ref as MR
import _particle_ref as PR
import _push_ref as QR
import _sort_ref as SR
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U
from test_gpu_length import _assert_spacings
from test_gpu_particles import _charges, _same_bits

gpu = pytest.mark.gpu

CASES = [pytest.param(bc, N, length, id=f"{bc}-{N}-{length:g}") for bc, N, length in LC.particle_cases()]
PUSH_CASES = [pytest.param(bc, N, length, mask, id=f"{bc}-{N}-{length:g}-{'mask' if mask else 'free'}")
              for bc, N, length, mask in LC.push_cases()]
COUNT = 1000  # seeded points beside the edge and node points


def _host(t):
    return t.cpu().numpy()


def _dev(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device="cuda")


def _solver(N, bc, length, extra=False, mask=None):
    axes, faces = LC.BCS[bc]
    c, L = LC.particle_shape(N, bc)
    s = M.Solver(c, L, 2, grid_length=length)
    _assert_spacings(s, c, L, length)
    assert s.h == QR.spacing(N, length)
    s.set_periodic(axes)
    s.set_neumann(faces)
    if extra:
        s.set_coefficient(CR.ball_eps(N))
        s.set_mask(MR.sphere(N).astype(np.uint8))
    if mask is not None:
        s.set_mask(mask)
    return s


def _random(N, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (N, N, N))


def _points(N, h, axes, count, seed):
    """seeded points inside the box, the edge points, every node of every axis and its two neighbours"""
    return np.concatenate([PR.box_points(N, h, count, seed), PR.edge_points(N, h, axes), PR.node_points_all(N, h)])


def _pack_count(s):
    s.sync()
    return s.kernel_times().get((s.num_levels - 1, "pack"), (0, 0.))[0]


# ------------------------------------------------------------------------------------------------------------- 1 sample
def _check_sample(s, u, xyz, axes, faces, scales, what):
    pos = _dev(xyz)
    for scale in scales:
        gu, gg = s.sample_tensor(pos, scale=scale)
        wu, wg = PR.sample(u, xyz, s.h, axes, faces, scale)
        assert _same_bits(_host(gu), wu), (what, scale, np.argwhere(_host(gu) != wu)[:4])
        assert _same_bits(_host(gg), wg), (what, scale, np.argwhere(_host(gg) != wg)[:4])
    return wu


@gpu
@pytest.mark.parametrize("bc,N,length", CASES)
def test_sample_bits(bc, N, length):
    axes, faces = LC.BCS[bc]
    u = _random(N, 1000 * N + axes * 64 + faces)
    with _solver(N, bc, length) as s:
        q = s.num_levels - 1
        xyz = _points(N, s.h, axes, COUNT, 7 * N + axes)
        s.upload(MG3D_U, q, u)
        s.timing_enable(1)
        s.timing_reset()
        wu = _check_sample(s, u, xyz, axes, faces, LC.PARTICLE_GRAD_SCALES, (bc, N, length))
        assert _pack_count(s) == len(LC.PARTICLE_GRAD_SCALES)  # one launch per call
        assert np.isnan(wu).any() and np.isfinite(wu[:COUNT]).all()
        hu, hg = s.sample(xyz, scale=2.9)  # the host form
        wu, wg = PR.sample(u, xyz, s.h, axes, faces, 2.9)
        assert _same_bits(hu, wu) and _same_bits(hg, wg)
        assert _same_bits(s.download(MG3D_U, q).reshape(N, N, N), u)


@gpu
@pytest.mark.parametrize("bc,N", [("f25", 41), ("per7", 21)])
def test_sample_float32_positions_and_outputs(bc, N):
    """3e-4: the float32 positions widen exactly (the node points become other doubles, with their own quotients), the
    float32 outputs are the restatement's rounded to nearest even"""
    length = 3e-4
    axes, faces = LC.BCS[bc]
    u = _random(N, 2000 + N)
    with _solver(N, bc, length) as s:
        s.upload(MG3D_U, s.num_levels - 1, u)
        xyz = _points(N, s.h, axes, COUNT, 21)
        with np.errstate(over="ignore"):
            xyz32 = xyz.astype(np.float32)
        for scale in LC.PARTICLE_GRAD_SCALES:
            wu, wg = PR.sample(u, xyz32.astype(np.float64), s.h, axes, faces, scale)
            gu, gg = s.sample_tensor(_dev(xyz32, torch.float32), scale=scale)
            assert gu.dtype == torch.float64 and _same_bits(_host(gu), wu) and _same_bits(_host(gg), wg), scale
            gu, gg = s.sample_tensor(_dev(xyz32, torch.float32), scale=scale, dtype=torch.float32)
            assert gu.dtype == torch.float32 and gg.dtype == torch.float32
            with np.errstate(over="ignore"):
                assert _same_bits(_host(gu), wu.astype(np.float32)) and _same_bits(_host(gg), wg.astype(np.float32)), scale


@gpu
@pytest.mark.parametrize("length", LC.LENGTHS)
def test_sample_with_eps_and_a_mask_set(length):
    """no difference expected, as on the unit cube: the sample reads u alone"""
    N, bc = 41, "f22"
    axes, faces = LC.BCS[bc]
    u = _random(N, 77)
    with _solver(N, bc, length, extra=True) as s:
        s.upload(MG3D_U, s.num_levels - 1, u)
        _check_sample(s, u, _points(N, s.h, axes, COUNT, 5), axes, faces, LC.PARTICLE_GRAD_SCALES, (bc, N, length))


@gpu
def test_sample_past_the_grid_cap():
    """QR.PAST_CAP_COUNT points at 21^3 on the 3e-4 box: the blocks stride, and the node points are in every stride"""
    N, bc, length = 21, "f25", 3e-4
    axes, faces = LC.BCS[bc]
    u = _random(N, 78)
    with _solver(N, bc, length) as s:
        s.upload(MG3D_U, s.num_levels - 1, u)
        nodes = PR.node_points_all(N, s.h)
        seeded = PR.box_points(N, s.h, QR.PAST_CAP_COUNT - 2 * nodes.shape[0], 9)
        xyz = np.concatenate([nodes, seeded, nodes])
        assert xyz.shape[0] == QR.PAST_CAP_COUNT
        _check_sample(s, u, xyz, axes, faces, (2.9,), "past the cap")


# ------------------------------------------------------------------------------------------------------------ 2 deposit
@gpu
@pytest.mark.parametrize("bc,N,length", CASES)
def test_deposit_bits(bc, N, length):
    axes, faces = LC.BCS[bc]
    d0 = np.random.default_rng(3000 * N + axes * 64 + faces).uniform(-50, 50, (N, N, N)) / (length * length)
    scale = -1.0 / 8.8541878128e-12 * 1e-15
    with _solver(N, bc, length) as s:
        q = s.num_levels - 1
        xyz = _points(N, s.h, axes, COUNT, 9 * N + axes)
        M_ = xyz.shape[0]
        ch = _charges(M_, 11 * N)
        ch[3], ch[5] = np.nan, -np.inf  # not deposited
        want = PR.deposit(d0, xyz, ch, s.h, axes, faces, scale)
        pos, qt = _dev(xyz), _dev(ch)
        s.upload(MG3D_D, q, d0)
        s.timing_enable(1)
        s.timing_reset()
        s.deposit_tensor(pos, qt, scale=scale)
        assert _pack_count(s) == (4 if axes else 3)  # scan, accumulate, apply (+ the duplicate refresh)
        got = s.download(MG3D_D, q).reshape(N, N, N)
        assert _same_bits(got, want), (bc, N, length, np.argwhere(got != want)[:4])
        assert not _same_bits(got, d0)
        for ax in range(3):  # the duplicates of d equal their sources
            if FR.per(axes, ax):
                assert _same_bits(np.take(got, N - 1, axis=ax), np.take(got, 0, axis=ax))
        # the points reversed, through the host form: the same bits
        s.upload(MG3D_D, q, d0)
        s.deposit(xyz[::-1], ch[::-1], scale=scale)
        assert _same_bits(s.download(MG3D_D, q).reshape(N, N, N), want)


@gpu
@pytest.mark.parametrize("length", LC.LENGTHS)
def test_deposit_of_zero_charges(length):
    """all-zero q leaves d bit-identical, the state handling still happens"""
    N, bc = 21, "per4_f15"
    axes, faces = LC.BCS[bc]
    d0 = _random(N, 31) * (50.0 / (length * length))
    with _solver(N, bc, length) as s:
        q = s.num_levels - 1
        xyz = _points(N, s.h, axes, COUNT, 3)
        s.upload(MG3D_D, q, d0)
        s.deposit_tensor(_dev(xyz), torch.zeros(xyz.shape[0], dtype=torch.float64, device="cuda"), scale=-2.0)
        assert _same_bits(s.download(MG3D_D, q).reshape(N, N, N), d0) and s.dzero_planes()[1] == 1


# --------------------------------------------------------------------------------------------------------------- 3 push
def _check_pushes(bc, N, length, with_mask, vel_dtype=np.float64):
    u, mask, xyz, vel, qm, accel, drag = QR.case_data(N, bc, LC.PUSH_COUNT, with_mask, length, nodes=True)
    want = QR.run_case(N, bc, LC.PUSH_COUNT, with_mask, LC.PUSHES, None, length, nodes=True, vel_dtype=vel_dtype)
    M_ = xyz.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        vel = vel.astype(vel_dtype)
    with _solver(N, bc, length, mask=mask) as s:
        q = s.num_levels - 1
        s.upload(MG3D_U, q, u)
        s.timing_enable(1)
        s.timing_reset()
        pos, fate, qt = _dev(xyz), torch.zeros(M_, dtype=torch.int32, device="cuda"), _dev(qm)
        v = _dev(vel, torch.float32 if vel_dtype == np.float32 else torch.float64)
        for n, (wx, wv, wf, wt) in enumerate(want):
            s.push_tensor(pos, v, qt, QR.DT, fate, scale=-1.0, accel=accel, drag=drag)
            assert _pack_count(s) == n + 1
            gx, gv, gf = _host(pos), _host(v), _host(fate)
            assert np.array_equal(gf, wf), (bc, N, length, n, np.argwhere(gf != wf)[:4], gf[gf != wf][:4], wf[gf != wf][:4])
            assert _same_bits(gx, wx), (bc, N, length, n, np.argwhere(gx != wx)[:4])
            assert wv.dtype == vel_dtype and _same_bits(gv, wv), (bc, N, length, n, np.argwhere(gv != wv)[:4])
            got = s.push_counts()
            assert got.dtype == np.uint64 and np.array_equal(got, wt), n
        assert _same_bits(s.download(MG3D_U, q).reshape(N, N, N), u)


@gpu
@pytest.mark.parametrize("bc,N,length,with_mask", PUSH_CASES)
def test_push_bits(bc, N, length, with_mask):
    _check_pushes(bc, N, length, with_mask)


@gpu
@pytest.mark.parametrize("length", LC.LENGTHS)
def test_push_float32_velocities(length):
    _check_pushes("f25", 41, length, True, np.float32)


@gpu
@pytest.mark.parametrize("N,bc,with_mask", [(21, "dirichlet", True), (41, "f22", False)])
def test_loop_of_deposit_cycles_and_push(N, bc, with_mask):
    """three steps of deposit -> vcycles(2) -> push on a 3e-4 box, and on b the same with the push restated on the
    downloaded u: the particles and u agree bit for bit after every step.  q/m and the deposit's scale are those of the
    unit-cube loop of tests/test_gpu_push.py taken through the identity (q/m times length^2, scale times length), so u and
    the kicks in units of h are the unit cube's"""
    length = 3e-4
    axes, faces = LC.BCS[bc]
    h = QR.spacing(N, length)
    mask = QR.bodies(N) if with_mask else None
    xyz, vel, _ = QR.particles(N, h, axes, 300, 31 + N, nodes=True)
    M_ = xyz.shape[0]
    charge = np.random.default_rng(N).choice([-1.0, 1.0, 2.0], M_)
    qm = charge * (0.2 * h * length / (QR.DT * QR.DT))
    scale = -(h ** 3) / (length * length)
    fate = np.zeros(M_, dtype=np.int32)
    with _solver(N, bc, length, mask=mask) as a, _solver(N, bc, length, mask=mask) as b:
        q = a.num_levels - 1
        for s in (a, b):
            if with_mask:
                s.set_mask_coarsening("keep")
            s.get_details()
        pos, v, ft, qt, ct = _dev(xyz), _dev(vel), _dev(fate, torch.int32), _dev(qm), _dev(charge)
        for step in range(3):
            a.deposit_tensor(pos, torch.where(ft == 0, ct, torch.zeros_like(ct)), scale=scale)
            a.vcycles(2)
            a.push_tensor(pos, v, qt, QR.DT, ft)
            b.deposit(xyz, np.where(fate == 0, charge, 0.0), scale=scale)
            b.vcycles(2)
            ub = b.download(MG3D_U, q).reshape(N, N, N)
            xyz, vel, fate = QR.push(ub, mask, xyz, vel, qm, fate, h, axes, faces, QR.DT)
            assert np.array_equal(_host(ft), fate), step
            assert _same_bits(_host(pos), xyz) and _same_bits(_host(v), vel), step
            assert _same_bits(a.download(MG3D_U, q).reshape(N, N, N), ub), step
        assert ub.any() and (fate == 0).any() and (fate != 0).any()


# --------------------------------------------------------------------------------------------------------------- 4 sort
def _check_sort(s, N, bc, xyz, fate, shift, f32=False):
    axes = LC.BCS[bc][0]
    with np.errstate(over="ignore"):
        pos = xyz.astype(np.float32) if f32 else xyz
    want, wc = SR.sort(pos, fate, s.h, N, axes, shift)
    s.timing_reset()
    perm, counts = s.sort_tensor(_dev(pos, torch.float32 if f32 else torch.float64),
                                 None if fate is None else _dev(fate, torch.int32), shift=shift)
    assert _pack_count(s) == 1 + 3 * SR.passes(N, shift)
    got, gc = _host(perm), _host(counts)
    assert got.dtype == np.int32 and gc.dtype == np.int64 and gc.shape == (2,)
    assert np.array_equal(gc, wc), (N, bc, shift, f32, gc, wc)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (N, bc, shift, f32, bad[:4], got[bad[:4]], want[bad[:4]])
    return perm, want


@gpu
@pytest.mark.parametrize("bc,N,length", CASES)
def test_sort_and_permute_bits(bc, N, length):
    """the permutation (stable: unique, so it pins every key's order) and both counts at shift 0 and 2, float64 and float32
    positions, with and without the fates; then nine vectors of mixed type through one permute launch"""
    xyz, fate = SR.particles(N, bc, LC.SORT_COUNT, length, nodes=True)
    rng = np.random.default_rng(N)
    with _solver(N, bc, length) as s:
        s.timing_enable(1)
        for shift in (0, 2):
            for f32 in (False, True):
                for f in (fate, None):
                    perm, want = _check_sort(s, N, bc, xyz, f, shift, f32)
        vel32 = rng.uniform(-1, 1, (LC.SORT_COUNT, 3)).astype(np.float32)
        q, qm32 = rng.uniform(-1, 1, LC.SORT_COUNT), rng.uniform(-1, 1, LC.SORT_COUNT).astype(np.float32)
        host = [np.array(xyz), vel32, q, qm32, np.array(fate)]
        dev = [_dev(a, None) for a in host]
        s.timing_reset()
        outs = s.permute_tensors(perm, *dev)  # 3 + 3 + 1 + 1 + 1 vectors
        assert _pack_count(s) == 1
        for o, a in zip(outs, host):
            ho = _host(o)
            assert ho.dtype == a.dtype and ho.tobytes() == np.ascontiguousarray(a[want]).tobytes()


@gpu
def test_sort_past_the_grid_cap():
    N, bc, length = 41, "per7", 3e-4
    xyz, fate = SR.particles(N, bc, QR.PAST_CAP_COUNT, length, nodes=True)
    with _solver(N, bc, length) as s:
        s.timing_enable(1)
        _check_sort(s, N, bc, xyz, fate, 0)
        _check_sort(s, N, bc, xyz, fate, 2, f32=True)


@gpu
def test_loop_of_push_sort_and_permute():
    """three steps of push -> sort -> permute at 41^3 on the 3e-4 box against the restatements, step by step"""
    N, bc, length = 41, "per4_f15", 3e-4
    axes, faces = LC.BCS[bc]
    u, mask, xyz, vel, qm, accel, drag = QR.case_data(N, bc, LC.PUSH_COUNT, True, length, nodes=True)
    M_ = xyz.shape[0]
    h = QR.spacing(N, length)
    fate = np.zeros(M_, dtype=np.int32)
    table = QR.new_table()
    with _solver(N, bc, length, mask=mask) as s:
        s.upload(MG3D_U, s.num_levels - 1, u)
        T = [_dev(xyz), _dev(vel), _dev(qm), _dev(fate, torch.int32)]
        moved = 0
        for step in range(3):
            s.push_tensor(T[0], T[1], T[2], QR.DT, T[3], scale=-1.0, accel=accel, drag=drag)
            xyz, vel, fate = QR.push(u, mask, xyz, vel, qm, fate, h, axes, faces, QR.DT, -1.0, accel, drag, table)
            perm, counts = s.sort_tensor(T[0], T[3], shift=step % 2 * 2)
            want, wc = SR.sort(xyz, fate, h, N, axes, step % 2 * 2)
            assert np.array_equal(_host(perm), want) and np.array_equal(_host(counts), wc), step
            T = list(s.permute_tensors(perm, *T))
            xyz, vel, qm, fate = xyz[want], vel[want], qm[want], fate[want]
            moved += int(np.count_nonzero(want != np.arange(M_)))
            for t, a in zip(T, (xyz, vel, qm)):
                assert _same_bits(_host(t), a), step
            assert np.array_equal(_host(T[3]), fate), step
            assert np.array_equal(s.push_counts(), table), step
        assert moved and (fate == 0).any() and (fate != 0).any()


# ----------------------------------------------------------------------------------------------------------- 5 identity
def _scaled(got, base, factor, what):
    got, base = np.asarray(got), np.asarray(base)
    fin = np.isfinite(base)
    assert np.array_equal(np.isnan(got), np.isnan(base)), what
    assert LC.normal(got[fin]) and LC.normal(base[fin]), what
    assert LC.same_bits(got[fin], base[fin] * base.dtype.type(factor)), what


@gpu
@pytest.mark.parametrize("length", LC.LENGTHS)
def test_identity_between_gpu_runs(length):
    """41^3 = (11, 3), periodic k, Neumann on the i and j faces, a mask of two bodies: sample, deposit, three pushes and
    the sorts behind them at grid_length * 2^m against the run at grid_length"""
    N, bc = 41, "per4_f15"
    axes, faces = LC.BCS[bc]
    u, mask, xyz, vel, qm, accel, drag = QR.case_data(N, bc, LC.PUSH_COUNT, True, length, nodes=True)
    # (a subnormal coordinate does not scale exactly: the identity is not asked of the two edge points that hold one)
    rows = ~((xyz != 0) & (np.abs(xyz) < np.finfo(np.float64).tiny)).any(axis=1)
    xyz, vel, qm = xyz[rows], vel[rows], qm[rows]
    assert np.array_equal(xyz, LC.fair_points(xyz), equal_nan=True) and np.isnan(xyz).any()
    M_ = xyz.shape[0]
    ch = _charges(M_, 17)
    d0 = _random(N, 5) * (50.0 / (length * length))
    dep_scale = -2.9

    def run(m):
        f = 2.0 ** m
        x, v, k, a = LC.scale_particles(m, xyz, vel, qm, accel)
        with _solver(N, bc, length * f, mask=mask) as s:
            q = s.num_levels - 1
            s.upload(MG3D_U, q, u)
            s.upload(MG3D_D, q, d0 / (f * f))
            pos = _dev(x)
            samples = [tuple(_host(t) for t in s.sample_tensor(pos, scale=scale)) for scale in LC.PARTICLE_GRAD_SCALES]
            s.deposit_tensor(pos, _dev(ch), scale=dep_scale * f)
            d = s.download(MG3D_D, q)
            vt, qt, ft = _dev(v), _dev(k), torch.zeros(M_, dtype=torch.int32, device="cuda")
            steps = []
            for _ in range(LC.PUSHES):
                s.push_tensor(pos, vt, qt, QR.DT, ft, scale=-1.0, accel=a, drag=drag)
                sorts = [tuple(_host(t) for t in s.sort_tensor(pos, ft, shift=shift)) for shift in (0, 2)]
                steps.append((_host(pos), _host(vt), _host(ft), s.push_counts(), sorts))
            return samples, d, steps, s.h

    bs, bd, bsteps, h = run(0)
    # the base run against the restatement: the identity cannot see an error that scales alike
    assert h == QR.spacing(N, length)
    for scale, (gu, gg) in zip(LC.PARTICLE_GRAD_SCALES, bs):
        wu, wg = PR.sample(u, xyz, h, axes, faces, scale)
        assert _same_bits(gu, wu) and _same_bits(gg, wg), scale
    assert _same_bits(bd.reshape(N, N, N), PR.deposit(d0, xyz, ch, h, axes, faces, dep_scale))
    for m in LC.MS:
        gs, gd, gsteps, _ = run(m)
        for (gu, gg), (wu, wg) in zip(gs, bs):
            _scaled(gu, wu, 1.0, (m, "u"))
            _scaled(gg, wg, 2.0 ** -m, (m, "gradient"))
        _scaled(gd, bd, 4.0 ** -m, (m, "d"))
        for n, (g, w) in enumerate(zip(gsteps, bsteps)):
            _scaled(g[0], w[0], 2.0 ** m, (m, n, "x"))
            _scaled(g[1], w[1], 2.0 ** m, (m, n, "v"))
            assert np.array_equal(g[2], w[2]) and np.array_equal(g[3], w[3]), (m, n)
            for (gp, gc), (wp, wc) in zip(g[4], w[4]):
                assert np.array_equal(gp, wp) and np.array_equal(gc, wc), (m, n, "sort")
    assert (bsteps[-1][2] == 0).any() and (bsteps[-1][2] != 0).any()
