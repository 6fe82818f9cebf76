"""The mixed-boundary ("electrospray") problem of the reference's original program, mg_3d_bkup.c: Dirichlet
patches on the two x faces, zero-gradient walls by ghost copy everywhere else, carried by the live red-black V-cycle.

PARITY UNPINNED: mg_3d_bkup.c does not compile against the current headers and its smoother is the order-dependent
lexicographic Gauss-Seidel, so the reference can produce no vector for it.  The CPU tests pin the statement
(oracle/mg3d_oracle_es.c) to the properties the problem must have; the GPU tests hold csrc/mg3d_es.hip to that
statement bit for bit.  The launch shapes past one k-block, the parameter sets off the default, random data on every level
and every level after a cycle are in tests/test_gpu_es_shapes.py (cases checked by tests/test_es_host.py)."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O


def test_patches_follow_the_reference_geometry():
    """mg_3d_bkup.c:739-778: disc rr <= Rc^2 on x = 0, annulus Ri^2 < rr < Ro^2 on x = L, centred in (y, z)."""
    lib, p = O.lib(), O.EsParams()
    N = 65
    h = p.length / (N - 1)
    y = np.arange(N) * h - p.length / 2
    rr = y[:, None] ** 2 + y[None, :] ** 2
    x0 = np.array([[lib.orc_es_dirichlet_x0(C.byref(p), h, j, k) for k in range(N)] for j in range(N)], dtype=bool)
    xl = np.array([[lib.orc_es_dirichlet_xl(C.byref(p), h, j, k) for k in range(N)] for j in range(N)], dtype=bool)
    assert np.array_equal(x0, rr <= p.capillary_radius ** 2) and x0.sum() > 0
    assert np.array_equal(xl, (rr > p.extractor_inner ** 2) & (rr < p.extractor_outer ** 2)) and xl.sum() > 100
    v = np.zeros(N ** 3)
    lib.orc_es_fill(O.P(v), N, h, C.byref(p), 1.0)
    V = v.reshape(N, N, N)
    assert np.all(V[-1][xl] == -1350.0) and np.all(V[-1][~xl] == 0) and np.all(V[1:-1] == 0) and np.all(V[0] == 0)


def test_ghost_copy_makes_walls_zero_gradient():
    """After a smoothing pass every wall point that is not a Dirichlet patch equals the interior point in front of it
    (mg_3d_bkup.c:84-133); patch points keep their potential; edges and corners are never written."""
    lib, p = O.lib(), O.EsParams()
    N = 17
    h = p.length / (N - 1)
    rng = np.random.default_rng(3)
    v, d = rng.uniform(-1, 1, N ** 3), rng.uniform(-1, 1, N ** 3) * 1e9
    lib.orc_es_fill(O.P(v), N, h, C.byref(p), 1.0)
    before = v.copy().reshape(N, N, N)
    lib.orc_es_smooth(O.P(v), O.P(d), N, h, 0, 1, C.byref(p))
    V = v.reshape(N, N, N)
    x0 = np.array([[lib.orc_es_dirichlet_x0(C.byref(p), h, j, k) for k in range(N)] for j in range(N)], dtype=bool)
    xl = np.array([[lib.orc_es_dirichlet_xl(C.byref(p), h, j, k) for k in range(N)] for j in range(N)], dtype=bool)
    inner = (slice(1, -1), slice(1, -1))
    assert np.array_equal(V[0][inner][~x0[inner]], V[1][inner][~x0[inner]])
    assert np.array_equal(V[-1][inner][~xl[inner]], V[-2][inner][~xl[inner]])
    assert np.array_equal(V[0][x0], before[0][x0]) and np.array_equal(V[-1][xl], before[-1][xl])
    assert np.array_equal(V[1:-1, 0, 1:-1], V[1:-1, 1, 1:-1]) and np.array_equal(V[1:-1, -1, 1:-1], V[1:-1, -2, 1:-1])
    assert np.array_equal(V[1:-1, 1:-1, 0], V[1:-1, 1:-1, 1]) and np.array_equal(V[1:-1, 1:-1, -1], V[1:-1, 1:-1, -2])
    assert np.array_equal(V[0, 0, :], before[0, 0, :]) and np.array_equal(V[:, 0, 0], before[:, 0, 0])  # edges untouched


def test_vcycle_converges_to_a_physical_potential():
    """33^3: the cycle converges -- slowly, as first-order ghost-copy walls and patches whose discrete shape changes from
    level to level make it (measured: an alternating history with a geometric-mean factor of 0.85 per V(2,2) cycle; with
    the original's pinned coarsest walls 0.93-0.96) -- and the potential is physical: maximum principle (between the two
    electrode potentials), symmetric in y <-> z like the geometry, falling monotonically along the axis."""
    norms, u, init = O.es_run(5, 4, 2, 40)
    assert init > 0 and norms[-1] < 5e-3 * norms[0] and (norms[-1] / norms[0]) ** (1 / 39) < 0.9
    assert np.all(norms[2:] < norms[:-2])  # every second cycle lower than two before
    N = 33
    U = u.reshape(N, N, N)[:, 1:-1, 1:-1]
    assert U.min() >= -1350.0 and U.max() <= 0.0
    np.testing.assert_allclose(U, U.transpose(0, 2, 1), rtol=0, atol=1e-7 * 1350)
    axis = u.reshape(N, N, N)[:, N // 2, N // 2]
    assert np.all(np.diff(axis[:-1]) < 0) and axis[0] == 0.0 and -600 < axis[1] < -400 and axis[-2] < -1200


@pytest.mark.gpu
@pytest.mark.parametrize("c,L,nu", [(5, 4, 2), (9, 3, 1), (3, 5, 2), (5, 5, 3), (11, 3, 2), (13, 3, 2)])
def test_gpu_matches_the_statement(c, L, nu):
    import multigrid_parallel_amd as M
    from multigrid_parallel_amd.binding import MG3D_U
    cycles = 6
    want_n, want_u, _ = O.es_run(c, L, nu, cycles)
    es = M.EsParams.default()
    with M.Solver(c, L, nu, grid_length=es.length) as s:
        s.es_setup(es)
        got = s.es_vcycles(cycles)
        u = s.download(MG3D_U, L - 1)
    assert np.array_equal(u, want_u)
    np.testing.assert_allclose(got, want_n, rtol=1e-11, atol=0)


@pytest.mark.gpu
def test_gpu_smoother_and_ghost_copies_match_the_statement():
    import multigrid_parallel_amd as M
    from multigrid_parallel_amd.binding import MG3D_D, MG3D_U
    lib, p = O.lib(), O.EsParams()
    c, L = 5, 3
    N = 17
    h = p.length / (N - 1)
    rng = np.random.default_rng(11)
    v, d = rng.uniform(-1, 1, N ** 3), rng.uniform(-1, 1, N ** 3) * 1e9
    with M.Solver(c, L, 2, grid_length=p.length) as s:
        s.es_setup()
        for post, iters in ((0, 1), (1, 2), (0, 3)):
            s.upload(MG3D_U, L - 1, v)
            s.upload(MG3D_D, L - 1, d)
            s.es_smooth(L - 1, post, iters)
            want = v.copy()
            lib.orc_es_smooth(O.P(want), O.P(d), N, h, post, iters, C.byref(p))
            assert np.array_equal(s.download(MG3D_U, L - 1), want), (post, iters)


@pytest.mark.gpu
def test_gpu_electrospray_129_cubed_vtk(tmp_path):
    """The size the original was run at is not recorded; 129^3 (9 5 2): converges, output through the VTK writer."""
    import multigrid_parallel_amd as M
    from multigrid_parallel_amd.binding import MG3D_U
    es = M.EsParams.default()
    with M.Solver(9, 5, 2, grid_length=es.length) as s:
        s.es_setup(es)
        norms = s.es_vcycles(30)
        u = s.download(MG3D_U, 4)
    assert norms[-1] < 0.1 * norms[0] and np.all(norms[2:] < norms[:-2])
    U = u.reshape(129, 129, 129)
    assert U[1:-1, 1:-1, 1:-1].min() >= -1350.0 and U[1:-1, 1:-1, 1:-1].max() <= 0.0
    out = tmp_path / "electrospray.vtk"
    assert M.lib().mg3d_write_vtk(str(out).encode(), u.ctypes.data_as(C.POINTER(C.c_double)), s.h, 129) == 0
    assert out.stat().st_size > 129 ** 3 * 10
