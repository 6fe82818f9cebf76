"""The restatement of the particle coupling (tests/_particle_ref.py) against properties it does not assume -- no GPU: the
sample at a node is the nodal gradient, a linear u samples to its slope, the deposit conserves charge and is the transpose
of the gather, no order of the points changes a bit, the edges of the box are inside and what lies past them is not; and
the count the GPU test uses past the grid cap of the point kernels really is past it."""
import math
import os
import re

import numpy as np
import pytest

import _field_ref as FR
import _particle_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (periodic axes, Neumann faces), as in tests/test_gpu_field.py
BCS = {"dirichlet": (0, 0), "per7": (7, 0), "per4_f15": (4, 15), "f63": (0, 63), "f22": (0, 22), "f25": (0, 0b011001)}
H = 2.0 ** -4  # a power of two: index * h and (index * h) / h are exact

# one count past the grid cap of the point kernels: a thread of the first block takes a second point
PAST_CAP_COUNT = 2048 * 256 + 259


def max_blocks():
    text = open(os.path.join(ROOT, "multigrid_parallel_amd", "csrc", "mg3d_internal.h")).read()
    return int(re.search(r"#define\s+MG3D_PARTICLE_MAX_BLOCKS\s+(\d+)", text).group(1))


def test_the_count_past_the_cap_is_past_it():
    cap = max_blocks() * PR.BLOCK
    assert cap < PAST_CAP_COUNT <= cap + 2 * PR.BLOCK  # some threads stride on, most do not: both paths in one launch
    assert PAST_CAP_COUNT % PR.BLOCK not in (0, 1)


def _random_u(N, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (N, N, N))


def _unique(N, axes):
    """(N, N, N) bool: no duplicate on any periodic axis"""
    m = np.ones((N, N, N), dtype=bool)
    for ax in range(3):
        if FR.per(axes, ax):
            sl = [slice(None)] * 3
            sl[ax] = N - 1
            m[tuple(sl)] = False
    return m


def _weights(N, axes, faces):
    w = [FR.axis_weight(N, axes, faces, ax) for ax in range(3)]
    return w[0][:, None, None] * w[1][None, :, None] * w[2][None, None, :]


@pytest.mark.parametrize("bc", list(BCS))
@pytest.mark.parametrize("N", [5, 9])
def test_sample_at_a_node_is_the_nodal_value(N, bc):
    axes, faces = BCS[bc]
    u = _random_u(N, 10 * N + axes + faces)
    i, j, k = (a.reshape(-1) for a in np.meshgrid(*[np.arange(N)] * 3, indexing="ij"))
    xyz = np.stack([i * H, j * H, k * H], axis=1)
    su, sg = PR.sample(u, xyz, H, axes, faces, scale=-1.0)
    g = FR.gradient(u, H, axes, faces, -1.0)
    src = u
    for ax in range(3):
        if FR.per(axes, ax):
            src = np.take(src, list(range(N - 1)) + [0], axis=ax)  # a duplicate is read at its source
    assert np.array_equal(su, src.reshape(-1))
    for d in range(3):
        assert np.array_equal(sg[:, d], g[d].reshape(-1)), d


@pytest.mark.parametrize("bc", list(BCS))
def test_linear_u_samples_to_its_slope(bc):
    """along every axis whose two faces are Dirichlet faces a linear u is admissible: central and one-sided differences
    are exact for it, and so is the trilinear interpolant"""
    N = 9
    axes, faces = BCS[bc]
    slope = np.array([0.75, -1.5, 2.25])
    lin = [ax for ax in range(3) if not FR.per(axes, ax) and not FR.neu(faces, ax, 0) and not FR.neu(faces, ax, 1)]
    x = np.arange(N) * H
    u = np.full((N, N, N), 0.5)
    for ax in lin:
        shape = [1, 1, 1]
        shape[ax] = N
        u = u + slope[ax] * x.reshape(shape)
    xyz = PR.box_points(N, H, 500, 77)
    su, sg = PR.sample(u, xyz, H, axes, faces)
    want_u = 0.5 + sum(slope[ax] * xyz[:, ax] for ax in lin)
    assert np.all(np.abs(su - want_u) <= 8 * np.finfo(float).eps * (1 + np.abs(want_u)))
    for ax in lin:
        assert np.all(np.abs(sg[:, ax] - slope[ax]) <= 64 * np.finfo(float).eps * abs(slope[ax]) * N), ax
    if bc == "dirichlet":
        assert lin == [0, 1, 2]


def _charges(count, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.1, 1.0, count) * rng.choice([-1.0, 1.0], count) * 10.0 ** rng.integers(-6, 6, count)


@pytest.mark.parametrize("bc", list(BCS))
def test_charge_is_conserved(bc):
    """sum over the unique nodes of w(p) * h^3 * (the change of d) / scale = sum of q, within 8 * count * 2^ue.  4099 points:
    the bound is about the integer rounding (half a unit for each of a point's eight contributions); the rounding of the
    weights (2^-52 of a charge), of (double)acc (2^-53 of a node's sum) and of the two sums compared here stay under it
    from some hundred points on, when the unit 2^ue = A * 2^(K-61) has grown past them."""
    N, count = 9, 4099
    axes, faces = BCS[bc]
    scale = -4.0  # h and scale powers of two: every factor of the sum is exact
    xyz = PR.box_points(N, H, count, 31)
    q = _charges(count, 32)
    acc, ue = PR.accumulate(xyz, q, H, N, axes)
    d = PR.deposit(np.zeros((N, N, N)), xyz, q, H, axes, faces, scale)
    terms = (_weights(N, axes, faces) * (H * H * H) * d / scale)[_unique(N, axes)]
    got, want = FR.fsum(terms), math.fsum(q)
    assert abs(got - want) <= 8 * count * math.ldexp(1.0, ue), (got, want, ue)
    assert abs(want) > 1e3 * count * math.ldexp(1.0, ue)  # (the bound is not the size of the sum itself)


@pytest.mark.parametrize("bc", list(BCS))
def test_the_integers_conserve_charge_exactly_for_dyadic_weights(bc):
    """five points whose weights are multiples of 1/8: the eight weights of a point sum to 1 exactly, so in exact
    arithmetic the accumulator holds the sum of q to half a unit per contribution -- 4 * count * 2^ue"""
    from fractions import Fraction
    N, count = 9, 5
    axes, _ = BCS[bc]
    xyz = np.random.default_rng(5).integers(0, 8 * (N - 1) + 1, (count, 3)) * (H / 8)
    q = _charges(count, 32)
    acc, ue = PR.accumulate(xyz, q, H, N, axes)
    unit = Fraction(2) ** ue
    assert abs(sum(acc.values()) * unit - sum(Fraction(float(v)) for v in q)) <= 4 * count * unit


@pytest.mark.parametrize("bc", list(BCS))
def test_gather_and_scatter_are_transposes(bc):
    N, count = 9, 4099
    axes, faces = BCS[bc]
    u = _random_u(N, 400 + axes + faces)
    xyz = PR.box_points(N, H, count, 41)
    q = _charges(count, 42)
    su, _ = PR.sample(u, xyz, H, axes, faces)
    acc, ue = PR.accumulate(xyz, q, H, N, axes)
    lhs = math.fsum(q * su)
    rhs = math.fsum(u[p] * math.ldexp(float(a), ue) for p, a in acc.items())
    assert abs(lhs - rhs) <= 8 * count * math.ldexp(1.0, ue) * np.abs(u).max(), (lhs, rhs)
    assert all(not (FR.per(axes, ax) and p[ax] == N - 1) for p in acc for ax in range(3))  # no duplicate is written


@pytest.mark.parametrize("bc", ["dirichlet", "per4_f15", "f63"])
def test_no_order_of_the_points_changes_a_bit(bc):
    N, count = 9, 1000
    axes, faces = BCS[bc]
    xyz = np.concatenate([PR.box_points(N, H, count, 51), PR.edge_points(N, H, axes)])
    q = _charges(xyz.shape[0], 52)
    q[7], q[11] = np.nan, np.inf
    d0 = _random_u(N, 53)
    want = PR.deposit(d0, xyz, q, H, axes, faces, -1.0)
    for perm in (np.arange(xyz.shape[0])[::-1], np.random.default_rng(54).permutation(xyz.shape[0])):
        got = PR.deposit(d0, xyz[perm], q[perm], H, axes, faces, -1.0)
        assert got.tobytes() == want.tobytes()


def test_edge_points():
    N = 9
    length = (N - 1) * H
    inside, c, w0, w1 = PR.locate_axis([0.0, -0.0, length], H, N, False)
    assert inside.all() and list(c) == [0, 0, N - 2] and list(w1) == [0.0, 0.0, 1.0] and list(w0) == [1.0, 1.0, 0.0]
    inside, c, w0, w1 = PR.locate_axis([0.0, -0.0, length], H, N, True)  # x = length is x = 0 of the next period
    assert inside.all() and list(c) == [0, 0, 0] and list(w1) == [0.0, 0.0, 0.0] and list(w0) == [1.0, 1.0, 1.0]
    bad = [np.nextafter(length, np.inf), np.nan, np.inf, -np.inf, -H, np.nextafter(0.0, -1.0) * 1e300]
    inside, *_ = PR.locate_axis(bad, H, N, False)
    assert not inside.any()
    inside, *_ = PR.locate_axis([np.nan, np.inf, -np.inf], H, N, True)
    assert not inside.any()
    # periodic coordinates several periods outside, negative or not, agree with their wrapped images where the wrap is
    # exact: dyadic coordinates and a power-of-two period
    base = np.array([0.0, 0.5 * H, 1.75 * H, 3 * H, length - 0.25 * H])
    want = PR.locate_axis(base, H, N, True)
    for periods in (1, 3, -1, -4, 1000, -1000):
        got = PR.locate_axis(base + periods * length, H, N, True)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), periods
    # far outside every finite coordinate is still inside, with a cell of the grid
    inside, c, w0, w1 = PR.locate_axis([1e300, -1e300, 5e-324, -5e-324, 1e6 * length + H / 3], H, N, True)
    assert inside.all() and np.all((0 <= c) & (c <= N - 2)) and np.all((0 <= w1) & (w1 <= 1)) and np.all((0 <= w0) & (w0 <= 1))
    # the sample of a point outside is NaN, its charge is not deposited
    u = _random_u(N, 61)
    xyz = np.array([[H, H, H], [H, -H, H], [np.nan, H, H], [H, H, 2 * length]])
    su, sg = PR.sample(u, xyz, H, 0, 0)
    assert np.isfinite(su[0]) and np.isfinite(sg[0]).all() and np.isnan(su[1:]).all() and np.isnan(sg[1:]).all()
    assert PR.deposit(np.zeros((N, N, N)), xyz[1:], np.ones(3), H, 0, 0).any() == False  # noqa: E712
    one = PR.deposit(np.zeros((N, N, N)), xyz, np.ones(4), H, 0, 0)
    assert np.argwhere(one != 0).tolist() == [[1, 1, 1]] and one[1, 1, 1] == 1.0 / H ** 3


def test_neumann_faces_double_and_zero_charges_leave_d_alone():
    N = 5
    d0 = _random_u(N, 71)
    xyz = np.array([[0.0, 2 * H, 0.0], [4 * H, 4 * H, 4 * H]])
    got = PR.deposit(np.zeros((N, N, N)), xyz, np.array([1.0, 3.0]), H, 0, 0b010001, 1.0)  # i low and k low are Neumann faces
    assert got[0, 2, 0] == 4.0 / H ** 3 and got[4, 4, 4] == 3.0 / H ** 3 and np.count_nonzero(got) == 2
    assert PR.deposit(d0, xyz, np.zeros(2), H, 0, 63).tobytes() == d0.tobytes()
    assert PR.deposit(d0, xyz, np.array([np.nan, -0.0]), H, 0, 63).tobytes() == d0.tobytes()


def test_numpys_ldexp_is_the_c_librarys():
    rng = np.random.default_rng(81)
    x = rng.uniform(-1, 1, 2000) * 10.0 ** rng.integers(-300, 300, 2000)
    for e in (-1100, -62, -3, 0, 7, 61, 900):
        with np.errstate(over="ignore", under="ignore"):
            got = np.ldexp(x, e)
        for a, b in zip(x, got):
            try:
                want = math.ldexp(a, e)
            except OverflowError:
                want = math.copysign(math.inf, a)
            assert want == b
    assert PR.count_bits(1) == 0 and PR.count_bits(2) == 1 and PR.count_bits(3) == 2 and PR.count_bits(4099) == 13
    assert PR.count_bits(1 << 40) == 40
