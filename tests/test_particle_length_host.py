"""The particle cases on boxes other than the unit cube, without a GPU: the cases of tests/test_gpu_particle_length.py are
held to what they were chosen for, and the restatements (tests/_particle_ref.py, _push_ref.py, _sort_ref.py) to the scaling
identity of tests/_length_cases.py.

1  node coverage: a coordinate formed as i*h locates in cell i - 1, with w1 just below 1, at some nodes whenever h is no
   power of two.  The counts per (N, length) are LC.LOW_NODES; every length meets at least two sizes that have such nodes;
   PR.node_points holds every one of them on every axis.  The far face n1*h locates in cell N - 2 with w1 == 1.0.
2  push coverage: with the seeds of the GPU cases every wall acts in three pushes -- a reflection at each Neumann face, a
   wrap in both directions on each periodic axis, an exit through each Dirichlet face -- and the table of fates holds both
   conductor labels and INVALID.
3  sort coverage: the living, the lost and the dead, ties, and a living node point whose key is that of cell i - 1.
4  the identity: positions, velocities and accel times s = 2^m, q/m times s^2, the deposit's scale times s, d over s^2 --
   the same cells and weight bits, the same sampled u, the gradient 2^-m times, pushed positions and velocities exactly s
   times, the same fates, table and permutation, the deposited d exactly s^-2 times."""
import numpy as np
import pytest

import _field_ref as FR
import _length_cases as LC
import _particle_ref as PR
import _push_ref as QR
import _sort_ref as SR

PAIRS = sorted({(N, length) for _, N, length in LC.particle_cases()})
IDENTITY_CASES = [(41, "per4_f15"), (21, "f25")]


def _h(N, length):
    return QR.spacing(N, length)


# ------------------------------------------------------------------------------------------------------------- 1 nodes
def test_the_boundary_sets_and_sizes_are_the_particle_tests():
    assert LC.BCS == QR.BCS
    for N, shapes in LC.PARTICLE_SIZES.items():
        for shape in shapes:
            assert shape is None or LC.n_of(*shape) == N
        assert shapes[1] is None or (shapes[1][0] - 1) % 2 == 0
    assert QR.spacing(37) == 1.0 / 36 and QR.spacing(37, 3.0) == 3.0 / 36 and SR.spacing(41, 3e-4) == 3e-4 / 40


def test_low_node_counts():
    """the table of the issue, so that a later change of sizes cannot empty the coverage"""
    assert set(LC.LOW_NODES) == {(N, length) for N in LC.PARTICLE_SIZES for length in LC.LENGTHS}
    for (N, length), (low, high) in LC.LOW_NODES.items():
        lo, hi = PR.low_nodes(N, _h(N, length))
        assert (lo.size, hi.size) == (low, high), (N, length, lo, hi)
    for length in LC.LENGTHS:  # the dyadic-friendly sizes of the other files have none: why these sizes were added
        for N in (17, 33):
            lo, hi = PR.low_nodes(N, _h(N, length))
            assert lo.size == 0 and hi.size == 0


def test_every_length_meets_two_sizes_with_low_nodes():
    assert PAIRS == sorted(LC.LOW_NODES)  # the GPU cases use every pair of the table
    for length, sizes in ((3e-4, {21, 41, 65}), (3.0, {37, 41})):
        have = {N for N, ln in PAIRS if ln == length and LC.LOW_NODES[(N, ln)][0] > 0}
        assert have == sizes and len(have) >= 2
    for axes_wanted in (False, True):  # and so does every length under a periodic set and under one without
        for length in LC.LENGTHS:
            assert any(LC.LOW_NODES[(N, ln)][0] > 0 for bc, N, ln in LC.particle_cases()
                       if ln == length and bool(LC.BCS[bc][0]) == axes_wanted), (axes_wanted, length)


@pytest.mark.parametrize("N,length", PAIRS)
def test_node_points_hold_the_low_nodes(N, length):
    h = _h(N, length)
    low = PR.low_nodes(N, h)[0]
    pts = PR.node_points(N, h)
    assert pts.shape == (3 * N, 3)
    for periodic in (False, True):
        for ax in range(3):
            rows = pts[ax * N:(ax + 1) * N]
            assert np.array_equal(rows[:, ax], np.array([np.float64(i) * h for i in range(N)]))
            inside, c, w0, w1 = PR.locate_axis(rows[:, ax], h, N, periodic)
            assert inside.all()
            below = np.flatnonzero(c[:N - 1] == np.arange(N - 1) - 1)
            assert np.array_equal(below, low[low < N - 1]), (N, length, ax)
            assert np.all((w1[below] < 1.0) & (w1[below] >= 1.0 - N * 2.0 ** -52))
            for other in ((ax + 1) % 3, (ax + 2) % 3):  # the other coordinates: inside, off the nodes, the same for all
                t = rows[:, other] / h
                assert np.all(t == t[0]) and 0.0 < t[0] < N - 1 and abs(t[0] - round(t[0])) > 0.05
    up, down = PR.node_points(N, h, 1), PR.node_points(N, h, -1)
    for ax in range(3):
        x = pts[ax * N:(ax + 1) * N, ax]
        assert np.all(up[ax * N:(ax + 1) * N, ax] > x) and np.all(down[ax * N:(ax + 1) * N, ax] < x)
        assert np.array_equal(np.nextafter(up[ax * N:(ax + 1) * N, ax], -np.inf), x)
        assert np.array_equal(np.nextafter(down[ax * N:(ax + 1) * N, ax], np.inf), x)
    assert np.array_equal(PR.node_points_all(N, h), np.concatenate([pts, up, down]))
    # one ulp below node 0 and one above node N-1 are outside where the axis is not periodic
    assert not PR.locate_axis(down[0:1, 0], h, N, False)[0][0] and not PR.locate_axis(up[N - 1:N, 0], h, N, False)[0][0]


@pytest.mark.parametrize("N,length", sorted(LC.LOW_NODES))
def test_the_far_face_is_exact(N, length):
    h = np.float64(_h(N, length))
    n1 = np.float64(N - 1)
    assert (n1 * h) / h == n1
    inside, c, w0, w1 = PR.locate_axis(np.array([n1 * h]), h, N, False)
    assert inside[0] and c[0] == N - 2 and w1[0] == 1.0 and w0[0] == 0.0
    assert QR.constants(N, h, QR.DT)[5] == n1 * h  # xhi is xper: the loop that lowers it never turns


@pytest.mark.parametrize("N,length", sorted(LC.LOW_NODES))
def test_gradient_scales_tell_the_factor_forms_apart(N, length):
    """cs = scale * (0.5 / h) against scale / (2 h): one of LC.PARTICLE_GRAD_SCALES gives another double at every h used
    here but 3.0 / 20 and 3.0 / 40, where the two forms agree for every scale tried (0.5 / h is too close to exact)"""
    h = _h(N, length)
    apart = any(s * (0.5 / h) != s / (2.0 * h) for s in LC.PARTICLE_GRAD_SCALES)
    if length == 3.0 and N in (21, 41):
        tried = np.random.default_rng(0).uniform(1e-3, 1e3, 20000)
        assert not apart and not (tried * (0.5 / h) != tried / (2.0 * h)).any()
    else:
        assert apart


# -------------------------------------------------------------------------------------------------------------- 2 push
_TABLES = {}


@pytest.mark.parametrize("bc,N,length,with_mask", LC.push_cases())
def test_push_cases_cover_every_wall(bc, N, length, with_mask):
    axes, faces = QR.BCS[bc]
    events = QR.new_events()
    states = QR.run_case(N, bc, LC.PUSH_COUNT, with_mask, LC.PUSHES, events, length, nodes=True)
    xyz, vel, fate, table = states[-1]
    _TABLES[(bc, N, length)] = table
    assert xyz.shape[0] <= 5000
    assert table[0] == 0 and int(table.sum()) == int((fate != 0).sum())
    assert (fate == 0).any() and table[QR.INVALID] > 0
    for ax in range(3):
        if FR.per(axes, ax):
            assert events["wrap_lo"][ax] > 0 and events["wrap_hi"][ax] > 0, (ax, events)
            assert table[QR.FACE + 2 * ax] == 0 and table[QR.FACE + 2 * ax + 1] == 0
            continue
        for hi, key in ((0, "reflect_lo"), (1, "reflect_hi")):
            if FR.neu(faces, ax, hi):
                assert events[key][ax] > 0, (ax, key, events)
            else:
                assert table[QR.FACE + 2 * ax + hi] > 0, (ax, hi)
    for label in QR.LABELS:
        assert (table[label] > 0) == with_mask
    # the node points are there, and the particles that sit on low nodes are pushed from cell i - 1
    first = QR.case_data(N, bc, LC.PUSH_COUNT, with_mask, length, nodes=True)[2]
    assert np.array_equal(first[-9 * N:], PR.node_points_all(N, _h(N, length)))


def test_push_tables_hold_every_fate():
    """over the cases: both labels, a Dirichlet face of each parity (low and high), INVALID -- at each length"""
    if len(_TABLES) < len(LC.push_cases()):
        for bc, N, length, with_mask in LC.push_cases():
            _TABLES[(bc, N, length)] = QR.run_case(N, bc, LC.PUSH_COUNT, with_mask, LC.PUSHES, None, length, nodes=True)[-1][3]
    for length in LC.LENGTHS:
        total = sum(t.astype(np.int64) for (bc, N, ln), t in _TABLES.items() if ln == length)
        assert all(total[label] > 0 for label in QR.LABELS) and total[QR.INVALID] > 0
        assert all(total[QR.FACE + f] > 0 for f in range(6))


# -------------------------------------------------------------------------------------------------------------- 3 sort
@pytest.mark.parametrize("bc,N,length", LC.particle_cases())
def test_sort_cases_hold_every_class_ties_and_low_nodes(bc, N, length):
    axes = QR.BCS[bc][0]
    h = _h(N, length)
    xyz, fate = SR.particles(N, bc, LC.SORT_COUNT, length, nodes=True)
    n_edge = PR.edge_points(N, h, axes).shape[0]
    assert xyz.shape == (LC.SORT_COUNT, 3) and np.array_equal(xyz[n_edge:n_edge + 9 * N], PR.node_points_all(N, h))
    for shift in (0, 2):
        K = SR.keys(xyz, fate, h, N, axes, shift)
        top = SR.kmax(N, shift)
        inside, lost, dead = SR.classes(K, top)
        assert inside and lost and dead
        cells, counts = np.unique(K[K < top], return_counts=True)
        assert (counts >= 2).any()  # ties: the order among them is the stable sort's
    low = PR.low_nodes(N, h)[0]
    low = low[low < N - 1]
    assert (low.size > 0) == (LC.LOW_NODES[(N, length)][0] > 0)
    if low.size:
        K = SR.keys(xyz, fate, h, N, axes, 0)
        _, c, _ = PR.locate(xyz, h, N, axes)
        nb = SR.blocks(N, 0)
        hit = 0
        for ax in range(3):
            rows = n_edge + ax * N + low
            assert np.array_equal(c[ax, rows], low - 1)
            alive = rows[fate[rows] == 0]
            hit += alive.size
            assert np.array_equal(K[alive], (c[0, alive] * nb + c[1, alive]) * nb + c[2, alive])
        assert hit > 0


# ---------------------------------------------------------------------------------------------------------- 4 identity
def _points(N, h, axes, seed):
    pts = np.concatenate([PR.box_points(N, h, 500, seed), PR.edge_points(N, h, axes), PR.node_points_all(N, h)])
    return LC.fair_points(pts)


def _assert_scaled(got, base, factor, what):
    got, base = np.asarray(got), np.asarray(base)
    fin = np.isfinite(base)
    assert np.array_equal(np.isnan(got), np.isnan(base)), what
    assert LC.normal(got[fin]) and LC.normal(base[fin]), what
    assert LC.same_bits(got[fin], base[fin] * base.dtype.type(factor)), what


@pytest.mark.parametrize("length", LC.HOST_LENGTHS)
@pytest.mark.parametrize("N,bc", IDENTITY_CASES)
def test_identity_of_locate_sample_and_deposit(N, bc, length):
    axes, faces = QR.BCS[bc]
    h = _h(N, length)
    xyz = _points(N, h, axes, 5)
    u = QR.field(N, 3)
    d0 = np.random.default_rng(N).uniform(-50, 50, (N, N, N)) / (length * length)
    q = np.random.default_rng(N + 1).uniform(-1, 1, xyz.shape[0]) * 10.0 ** np.random.default_rng(N + 2).integers(-6, 6, xyz.shape[0])
    scale = -2.9
    bi, bcell, bw = PR.locate(xyz, h, N, axes)
    bu, bg = PR.sample(u, xyz, h, axes, faces, scale)
    bd = PR.deposit(d0, xyz, q, h, axes, faces, scale)
    assert bi.any() and not bi.all() and not LC.same_bits(bd, d0)
    for m in LC.MS:
        s = 2.0 ** m
        hs = _h(N, length * s)
        assert hs == h * s
        xs = LC.scale_particles(m, xyz)
        inside, cell, w = PR.locate(xs, hs, N, axes)
        assert np.array_equal(inside, bi) and np.array_equal(cell, bcell) and LC.same_bits(w, bw)
        gu, gg = PR.sample(u, xs, hs, axes, faces, scale)
        _assert_scaled(gu, bu, 1.0, (m, "u"))
        _assert_scaled(gg, bg, 2.0 ** -m, (m, "gradient"))
        gd = PR.deposit(d0 / (s * s), xs, q, hs, axes, faces, scale * s)
        _assert_scaled(gd, bd, 4.0 ** -m, (m, "d"))


@pytest.mark.parametrize("length", LC.HOST_LENGTHS)
@pytest.mark.parametrize("N,bc", IDENTITY_CASES)
def test_identity_of_push_and_sort(N, bc, length):
    axes, faces = QR.BCS[bc]
    h = _h(N, length)
    u, mask, xyz, vel, qm, accel, drag = QR.case_data(N, bc, 500, True, length, nodes=True)
    keep = ~((xyz != 0) & (np.abs(xyz) < np.finfo(np.float64).tiny)).any(axis=1)
    xyz, vel, qm = xyz[keep], vel[keep], qm[keep]

    def run(m):
        hs = _h(N, length * 2.0 ** m)
        x, v, k, a = LC.scale_particles(m, xyz, vel, qm, accel)
        fate = np.zeros(x.shape[0], dtype=np.int32)
        table = QR.new_table()
        out = []
        for _ in range(LC.PUSHES):
            x, v, fate = QR.push(u, mask, x, v, k, fate, hs, axes, faces, QR.DT, -1.0, a, drag, table)
            out.append((x, v, fate, table.copy(), SR.sort(x, fate, hs, N, axes, 0), SR.sort(x, fate, hs, N, axes, 2)))
        return out

    base = run(0)
    assert (base[-1][2] == 0).any() and (base[-1][2] != 0).any()
    for m in LC.MS:
        for n, (got, want) in enumerate(zip(run(m), base)):
            _assert_scaled(got[0], want[0], 2.0 ** m, (m, n, "x"))
            _assert_scaled(got[1], want[1], 2.0 ** m, (m, n, "v"))
            assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]), (m, n)
            for a, b in zip(got[4:], want[4:]):
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (m, n, "sort")
