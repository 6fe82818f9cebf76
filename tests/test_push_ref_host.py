"""The restatement of the particle mover (tests/_push_ref.py) against physics and its own invariants -- no GPU, no library:
the leapfrog parabola in a uniform field, the mirror at a Neumann wall, the wrap of a periodic axis, the drag-free bits, the
largest inside coordinate xhi, and the coverage of the cases the GPU test runs (tests/test_gpu_push.py): with its seeds
every outcome a case can produce does occur."""
from fractions import Fraction

import numpy as np
import pytest

import _field_ref as FR
import _particle_ref as PR
import _push_ref as QR
from test_particle_ref_host import PAST_CAP_COUNT

EPS = 2.0 ** -53  # the unit roundoff of a double
H = 2.0 ** -4     # a power of two: index * h is exact


def _push_n(u, xyz, vel, qm, n, axes=0, faces=0, dt=2.0 ** -3, mask=None, **kw):
    fate = np.zeros(xyz.shape[0], dtype=np.int32)
    path = []
    for _ in range(n):
        xyz, vel, fate = QR.push(u, mask, xyz, vel, qm, fate, H, axes, faces, dt, **kw)
        path.append((xyz, vel, fate))
    return path


def test_the_count_past_the_cap_is_the_sample_tests_count():
    assert QR.PAST_CAP_COUNT == PAST_CAP_COUNT


def test_parabola_in_a_uniform_field():
    """u = -E0 x with E0 and h dyadic: every nodal value and every nodal gradient, the one-sided forms included, is exact, so
    E = E0 at every node and the trajectory is the leapfrog parabola v_n = v_0 + n a dt, x_n = x_0 + n dt v_0 +
    a dt^2 n (n + 1) / 2 with a = qm E0 + g, up to rounding.  The bound from the operations of one step:
      gather  : a level of the nested sum is (w0*V0) + (w1*V1) with w0 = fl(1 - f): at most 4 roundings on values within
                the bound of the level below, three levels: |E - E0| <= 13 eps E0 (first order, one eps of slack)
      kick    : k*E, + gdt, v0 + ..: three roundings; (* inv is exact, inv = 1): the velocity gains at most
                eps (14 |k E0| + |k E0 + gdt| + Vmax) =: ev per step, so after j steps |dv_j| <= j ev
      drift   : dt*v (dt a power of two: exact), x + ..: one rounding: the position gains dt |dv_j| + eps Xmax in step j
    hence |dx_n| <= dt ev n (n + 1) / 2 + n eps Xmax; second-order terms are covered by a factor 2."""
    N, E0, g, dt, qm, steps = 17, 0.75, -0.25, 2.0 ** -3, 0.5, 12
    x = np.arange(N) * H
    u = np.broadcast_to((-E0 * x)[:, None, None], (N, N, N)).copy()
    assert np.all(FR.gradient(u, H, 0, 0, -1.0)[0] == E0) and not FR.gradient(u, H, 0, 0, -1.0)[1].any()
    xyz = np.array([[0.1371, 0.4123, 0.6017], [0.3, 0.55, 0.2]])
    vel = np.array([[0.21, 0.013, -0.11], [-0.05, 0.07, 0.09]])
    path = _push_n(u, xyz, vel, qm, steps, dt=dt, accel=(g, 0.0, 0.0))
    a = Fraction(qm) * Fraction(E0) + Fraction(g)
    kE, gdt = abs(qm * dt * E0), abs(dt * g)
    for m in range(2):
        x0, v0 = [Fraction(float(c)) for c in xyz[m]], [Fraction(float(c)) for c in vel[m]]
        vmax = max(abs(float(v0[0] + n * a * Fraction(dt))) for n in range(steps + 1))
        ev = EPS * (14 * kE + (kE + gdt) + vmax)
        for n, (px, pv, pf) in enumerate(path, start=1):
            assert pf[m] == 0
            want_v = v0[0] + n * a * Fraction(dt)
            want_x = x0[0] + n * Fraction(dt) * v0[0] + a * Fraction(dt) ** 2 * Fraction(n * (n + 1), 2)
            assert abs(Fraction(float(pv[m, 0])) - want_v) <= 2 * n * ev
            assert abs(Fraction(float(px[m, 0])) - want_x) <= 2 * (dt * ev * n * (n + 1) / 2 + n * EPS * 1.0)
            for ax in (1, 2):  # no field across: the velocity keeps its bits, the position is n roundings off the line
                assert pv[m, ax] == vel[m, ax]
                assert abs(Fraction(float(px[m, ax])) - (x0[ax] + n * Fraction(dt) * v0[ax])) <= n * EPS * 1.0


def test_mirror_at_a_neumann_wall():
    """free flight (u = 0) at the low faces, which mirror about 0: negation is exact, so the reflected path has the bits of
    the absolute value of the unreflected one.  At the high faces the mirror is about xhi = length: the same to one rounding
    of the box length per step: one in the drift of either path (the free one reaches up to twice the length), two in the
    reflection."""
    N, dt, steps = 17, 2.0 ** -3, 10
    u = np.zeros((N, N, N))
    xyz = np.array([[0.0731, 0.0417, 0.0291], [0.9371, 0.9533, 0.9817]])
    vel = np.array([[-0.23, -0.31, -0.17], [0.27, 0.19, 0.33]])
    events = QR.new_events()
    path = _push_n(u, xyz, vel, 0.0, steps, faces=63, dt=dt, events=events)
    length = (N - 1) * H
    assert QR.constants(N, H, dt)[5] == length
    free = xyz.copy()
    for n, (px, pv, pf) in enumerate(path, start=1):
        free = free + (dt * vel)
        assert not pf.any()
        assert np.array_equal(px[0], np.abs(free[0])) and np.array_equal(np.abs(pv[0]), np.abs(vel[0]))
        assert np.all(np.abs(px[1] - np.where(free[1] > length, 2 * length - free[1], free[1])) <= (3 * n + 2) * EPS * length)
        assert np.array_equal(np.sign(pv[0]), np.where(free[0] < 0, 1.0, -1.0))
        assert np.array_equal(np.sign(pv[1]), np.where(free[1] > length, -1.0, 1.0))
    assert events["reflect_lo"] == [1, 1, 1] and events["reflect_hi"] == [1, 1, 1]


def test_wrap_samples_the_same_field():
    """dyadic positions and velocities on periodic axes: the drift and the wrap are exact, and the wrapped position samples
    the bits the unwrapped one does (the locator wraps that one itself)"""
    N, dt = 17, 2.0 ** -3
    rng = np.random.default_rng(5)
    u = rng.uniform(-1, 1, (N, N, N))
    M = 400
    xyz = rng.integers(0, 2 ** 20, (M, 3)) * 2.0 ** -20
    vel = rng.integers(-2 ** 12, 2 ** 12, (M, 3)) * 2.0 ** -12 * (1.5 * H / dt)
    events = QR.new_events()
    (px, pv, pf), = _push_n(np.zeros((N, N, N)), xyz, vel, 0.0, 1, axes=7, dt=dt, events=events)
    free = xyz + dt * vel
    assert not pf.any() and np.array_equal(pv, vel)
    assert min(events["wrap_lo"]) > 0 and min(events["wrap_hi"]) > 0
    moved = px != free
    assert moved.any() and np.all(np.abs(px - free)[moved] == 1.0) and np.all((px >= 0.0) & (px < 1.0))
    for scale in (-1.0, 0.37):
        a, b = PR.sample(u, px, H, 7, 0, scale), PR.sample(u, free, H, 7, 0, scale)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_no_drag_has_the_bits_of_the_drag_free_formula():
    N, dt = 17, 0.1
    rng = np.random.default_rng(9)
    u = rng.uniform(-1, 1, (N, N, N))
    assert QR.constants(N, H, dt, drag=0.0)[2] == 1.0
    xyz = PR.box_points(N, H, 300, 3) * 0.8 + 0.1
    vel = rng.uniform(-1, 1, (300, 3)) * 0.1
    qm = rng.uniform(-1, 1, 300) * 1e-3
    accel = (0.01, -0.02, 0.03)
    (px, pv, pf), = _push_n(u, xyz, vel, qm, 1, dt=dt, accel=accel)
    E = PR.sample(u, xyz, H, 0, 0, -1.0)[1]
    v1 = vel + (((qm * dt)[:, None] * E) + (dt * np.array(accel))[None, :])
    assert not pf.any() and np.array_equal(pv, v1) and np.array_equal(px, xyz + (dt * v1))
    # and with drag the velocity is that one times inv
    (qx, qv, qf), = _push_n(u, xyz, vel, qm, 1, dt=dt, accel=accel, drag=0.7)
    assert np.array_equal(qv, v1 * (1.0 / (1.0 + 0.7 * dt)))


@pytest.mark.parametrize("N", [5, 17, 33, 37, 65, 161, 257, 513])
def test_xhi_locates_inside(N):
    for h in (QR.spacing(N), H, 3.7 / (N - 1)):
        cs, gdt, inv, n1, xper, xhi = QR.constants(N, h, QR.DT)
        assert xhi / h <= N - 1 and xhi <= xper and xper - xhi <= 8 * EPS * xper
        assert PR.locate_axis(np.array([xhi]), h, N, False)[0][0]
        x = xhi * np.random.default_rng(N).uniform(0, 1, 1000)
        assert PR.locate_axis(x, h, N, False)[0].all()


@pytest.mark.parametrize("N,bc,count,with_mask,pushes", QR.CASES)
def test_the_gpu_cases_cover_every_outcome(N, bc, count, with_mask, pushes):
    """with the seeds of tests/test_gpu_push.py every outcome the case can produce occurs in the restatement: an exit through
    each Dirichlet face, a reflection at each Neumann face, a wrap in both directions on each periodic axis, each label,
    INVALID, survivors.  (A case of one particle shows the one-point launch, not the outcomes.)"""
    axes, faces = QR.BCS[bc]
    events = QR.new_events()
    states = QR.run_case(N, bc, count, with_mask, pushes, events)
    xyz, vel, fate, table = states[-1]
    assert table[0] == 0 and int(table.sum()) == int((fate != 0).sum())
    assert np.array_equal(np.bincount(fate[fate != 0], minlength=QR.SLOTS), table.astype(np.int64))
    if count == 1:
        return
    assert (fate == 0).any() and table[QR.INVALID] > 0
    for ax in range(3):
        if FR.per(axes, ax):
            assert events["wrap_lo"][ax] > 0 and events["wrap_hi"][ax] > 0
            assert table[QR.FACE + 2 * ax] == 0 and table[QR.FACE + 2 * ax + 1] == 0
            continue
        for hi, key in ((0, "reflect_lo"), (1, "reflect_hi")):
            if FR.neu(faces, ax, hi):
                assert events[key][ax] > 0
            else:
                assert table[QR.FACE + 2 * ax + hi] > 0
    for label in QR.LABELS:
        assert (table[label] > 0) == with_mask
