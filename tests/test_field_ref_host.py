"""The CPU restatement of the field output (tests/_field_ref.py) checked on its own, without a GPU: the gradient against
closed forms, the discrete Green identity that ties the energy to the flux, the slab problem where nothing has to be
solved, and the launch geometry of the two reductions restated from MG3D_MAX_PARTIALS."""
import math

import numpy as np
import pytest

import _field_ref as FR
from test_wpcg_ref_host import _max_partials

# (periodic axes, Neumann faces)
GREEN = [(0, 0), (7, 0), (0, 63), (4, 15), (0, 25), (2, 33), (0, 22)]


def test_gradient_of_a_quadratic_is_exact_on_a_dirichlet_box():
    """central and three-point one-sided differences are exact on quadratics: what is left is the rounding of the operands
    of the formulas, 32 * 2^-53 * max|u| / h"""
    N = 17
    h = 1.0 / (N - 1)
    x = np.arange(N) * h
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    u = 0.7 * X * X - 1.3 * Y * Y + 0.4 * Z * Z + 0.9 * X * Y - 0.6 * Y * Z + 1.1 * Z * X + 0.3 * X - 0.8 * Y + 0.5 * Z + 2.0
    want = [1.4 * X + 0.9 * Y + 1.1 * Z + 0.3, -2.6 * Y + 0.9 * X - 0.6 * Z - 0.8, 0.8 * Z - 0.6 * Y + 1.1 * X + 0.5]
    bound = 32 * 2.0 ** -53 * np.abs(u).max() / h
    for scale in (1.0, -1.0):
        got = FR.gradient(u, h, 0, 0, scale)
        for a in range(3):
            err = np.abs(got[a] - scale * want[a]).max()
            print(scale, a, err, bound)
            assert err <= bound


def test_periodic_duplicate_takes_its_sources_bits():
    """sin(2 pi x) on a periodic i axis, times a profile in j and k: sin(2 pi) is not 0. in floating point, so u's own
    duplicate plane differs from plane 0 -- the gradient's does not, in any component, and plane 0 is the wrapped difference"""
    N = 17
    h = 1.0 / (N - 1)
    x = np.arange(N) * h
    u = np.sin(2 * np.pi * x)[:, None, None] * (1.0 + x * x)[None, :, None] * np.cos(x)[None, None, :]
    assert not np.array_equal(u[N - 1], u[0])
    g = FR.gradient(u, h, 1, 0, 1.0)
    for a in range(3):
        assert np.array_equal(g[a][N - 1], g[a][0]) and np.array_equal(np.signbit(g[a][N - 1]), np.signbit(g[a][0]))
    assert np.array_equal(g[0][0], (u[1] - u[N - 2]) * (1.0 * (0.5 / h)))
    np.testing.assert_allclose(g[0][0], 2 * np.pi * (1.0 + x * x)[:, None] * np.cos(x)[None, :], rtol=0.03)


@pytest.mark.parametrize("faces", [63, 22, 25, 1, 32])
def test_normal_component_on_a_neumann_face_is_zero(faces):
    N = 9
    u = np.random.default_rng(faces).uniform(-1, 1, (N, N, N))
    g = FR.gradient(u, 1.0 / (N - 1), 0, faces, -1.0)
    for ax in range(3):
        for hi in (0, 1):
            face = np.take(g[ax], N - 1 if hi else 0, axis=ax)
            if FR.neu(faces, ax, hi):
                assert not face.any()
            else:
                assert face.any()


@pytest.mark.parametrize("axes,faces", GREEN)
def test_green_identity(axes, faces):
    """sum_e w_e a_e (du)^2 = - sum_p w(p) u_p (s - D u_p) over every unknown, for random u vanishing on the Dirichlet
    faces and random eps, to 1e-12 relative"""
    N = 9
    rng = np.random.default_rng(100 * axes + faces)
    u = rng.uniform(-1, 1, (N, N, N))
    eps = rng.uniform(0.5, 2.0, (N, N, N))
    for ax in range(3):
        d = FR.on_dirichlet(N, axes, faces, ax)
        np.moveaxis(u, ax, 0)[d] = 0.
    everywhere = np.ones((N, N, N), dtype=np.uint8)
    for e in (None, eps):
        lhs = FR.fsum(*FR.energy_terms(u, e, axes, faces))
        t = FR.flux_terms(u, e, everywhere, axes, faces)
        rhs = -FR.fsum(u[FR.flux_points(everywhere, axes, faces)] * t)
        print(axes, faces, e is not None, lhs, rhs, abs(lhs - rhs) / lhs)
        assert lhs > 0 and abs(lhs - rhs) <= 1e-12 * lhs


def slab_problem():
    """17^3, j and k periodic, i Dirichlet; u = i/12 up to plane 12 and 1 beyond; planes 12..15 fixed with label 3:
    (axes, faces, h, u, mask).  Discrete-exact: F = -4/3, W = 2/3"""
    N = 17
    i = np.arange(N, dtype=np.float64)[:, None, None] * np.ones((N, N, N))
    u = np.where(i <= 12, i / 12.0, 1.0)
    mask = np.zeros((N, N, N), dtype=np.uint8)
    mask[12:16] = 3
    return 6, 0, 1.0 / (N - 1), u, mask


def test_slab_problem():
    axes, faces, h, u, mask = slab_problem()
    F = FR.flux(u, None, mask, h, axes, faces, 3)
    W = FR.energy(u, None, h, axes, faces)
    print(F, W)
    assert abs(F + 4.0 / 3.0) <= 1e-12 and abs(W - 2.0 / 3.0) <= 1e-12
    assert FR.flux(u, None, mask, h, axes, faces, 0) == F
    F4 = FR.flux(u, None, mask, h, axes, faces, 4)
    assert F4 == 0. and not math.copysign(1., F4) < 0
    assert abs(W + 0.5 * 1.0 * F) <= 1e-12  # W = -1/2 V F with V = 1


def test_the_cap_size_doubles_the_chunk_and_the_sizes_below_do_not():
    """the launch geometry of the flux and the energy sums from MG3D_MAX_PARTIALS of the header: at CAP_SIZE with Dirichlet
    faces both launches exceed the cap at 16 planes per block and run 32; at every size of SUM_SIZES -- the next smaller
    one, 65, in particular -- neither does.  (513, between them, stays at 16 for the flux: exactly the cap.)"""
    cap = _max_partials()
    assert cap == 32768
    for N in FR.SUM_SIZES:
        for axes, faces in ((0, 0), (7, 0), (0, 63)):
            assert FR.flux_grid(N, axes, faces, cap)[3] == 16 and FR.energy_grid(N, cap)[3] == 16
    N = FR.CAP_SIZE
    assert max(FR.SUM_SIZES) == 65 < N
    gx, gy, gz, chunk = FR.flux_grid(N, 0, 0, cap)
    assert (gx, gy, gz, chunk) == (9, 136, 17, 32) and gx * gy * -(-(N - 2) // 16) > cap >= gx * gy * gz
    assert (N - 2) - (gz - 1) * chunk == 31  # a shorter last chunk
    gx, gy, gz, chunk = FR.energy_grid(N, cap)
    assert (gx, gy, gz, chunk) == (9, 137, 18, 32) and gx * gy * -(-N // 16) > cap >= gx * gy * gz
    assert N - (gz - 1) * chunk == 1  # a last chunk of one plane
    assert FR.flux_grid(513, 0, 0, cap)[3] == 16
