"""ctypes binding of oracle/liboracle.so (the CPU checker).  Test infrastructure only."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
dp = C.POINTER(C.c_double)
fp = C.POINTER(C.c_float)


def P(a):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(dp)


def PF(a):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(fp)


_lib = None


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
        L.orc_bc_func.restype = C.c_double
        L.orc_bc_func.argtypes = [C.c_double] * 3
        L.orc_fill_boundary.argtypes = [dp, C.c_int, C.c_double]
        L.orc_coarse_matrix.argtypes = [dp, C.c_int, C.c_double]
        L.orc_lu_factor.argtypes = [dp, C.c_int]
        L.orc_lu_factor_banded.argtypes = [dp, C.c_int]
        L.orc_lu_factor_banded.restype = None
        L.orc_lu_solve.argtypes = [dp, C.c_int, dp, dp]
        L.orc_smooth_color.argtypes = [dp, dp, C.c_int, C.c_double, C.c_int]
        L.orc_pre_smooth.argtypes = [dp, dp, C.c_int, C.c_double, C.c_int]
        L.orc_post_smooth.argtypes = [dp, dp, C.c_int, C.c_double, C.c_int]
        L.orc_residual.restype = C.c_double
        L.orc_residual.argtypes = [dp, dp, C.c_int, C.c_double, dp]
        L.orc_restrict.argtypes = [dp, C.c_int, dp, C.c_int]
        L.orc_prolong.argtypes = [dp, C.c_int, dp, C.c_int]
        L.orc_l2norm.restype = C.c_double
        L.orc_l2norm.argtypes = [dp, C.c_long]
        L.orc_vcycle.restype = C.c_double
        L.orc_vcycle.argtypes = [C.POINTER(dp)] * 3 + [C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, dp]
        L.orc_fmg_initialize.argtypes = [C.POINTER(dp)] * 3 + [C.c_int, C.c_int, C.c_int, C.c_double, dp]
        L.orc_run_problem.restype = C.c_double
        L.orc_run_problem.argtypes = [C.c_int] * 5 + [dp, dp, dp]
        # the screened operator (sigma-taking twins; pinned to _screened_ref and, at sigma = 0, to the functions above)
        L.orc_smooth_color_shift.argtypes = [dp, dp, C.c_int, C.c_double, C.c_double, C.c_int]
        L.orc_pre_smooth_shift.argtypes = [dp, dp, C.c_int, C.c_double, C.c_double, C.c_int]
        L.orc_post_smooth_shift.argtypes = [dp, dp, C.c_int, C.c_double, C.c_double, C.c_int]
        L.orc_residual_shift.restype = C.c_double
        L.orc_residual_shift.argtypes = [dp, dp, C.c_int, C.c_double, C.c_double, dp]
        L.orc_coarse_matrix_shift.argtypes = [dp, C.c_int, C.c_double, C.c_double]
        L.orc_vcycle_shift.restype = C.c_double
        L.orc_vcycle_shift.argtypes = [C.POINTER(dp)] * 3 + [C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, dp]
        L.orc_fmg_initialize_shift.argtypes = [C.POINTER(dp)] * 3 + [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, dp]
        L.orc_run_problem_shift.restype = C.c_double
        L.orc_run_problem_shift.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, dp, dp, dp]
        # single precision / Jacobi / F-cycle variant (oracle/mg3d_oracle_f32.c, parity unpinned)
        L.orc32_fill_boundary.argtypes = [fp, C.c_int, C.c_double]
        L.orc32_jacobi.argtypes = [fp, fp, fp, C.c_int, C.c_float, C.c_float]
        L.orc32_smooth.argtypes = [fp, fp, fp, C.c_int, C.c_float, C.c_float, C.c_int]
        L.orc32_residual.restype = C.c_double
        L.orc32_residual.argtypes = [fp, fp, C.c_int, C.c_float, fp]
        L.orc32_restrict.argtypes = [fp, C.c_int, fp, C.c_int]
        L.orc32_prolong.argtypes = [fp, C.c_int, fp, C.c_int]
        L.orc32_coarse_solve.argtypes = [dp, C.c_int, fp, fp]
        L.orc32_vcycle.restype = C.c_double
        L.orc32_vcycle.argtypes = [C.POINTER(fp)] * 4 + [C.c_double, C.c_int, C.c_int, C.c_float, C.c_int, dp]
        L.orc32_run_problem.restype = C.c_double
        L.orc32_run_problem.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, dp, fp]
        # the mixed-boundary ("electrospray") problem (oracle/mg3d_oracle_es.c, parity unpinned)
        L.orc_es_fill.argtypes = [dp, C.c_int, C.c_double, C.c_void_p, C.c_double]
        L.orc_es_smooth.argtypes = [dp, dp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p]
        L.orc_es_ghost_all.argtypes = [dp, C.c_int, C.c_double, C.c_void_p]
        L.orc_es_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, dp, dp, dp]
        L.orc_es_dirichlet_x0.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int]
        L.orc_es_dirichlet_xl.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int]
        L.orc_es_coarse_matrix.argtypes = [dp, C.c_int, C.c_double, C.c_void_p]
        L.orc_es_coarse_matrix.restype = None
        L.orc_es_vcycle.restype = C.c_double
        L.orc_es_vcycle.argtypes = [C.POINTER(dp)] * 3 + [C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, dp, C.c_void_p]
        L.orc_max_threads.restype = C.c_int
        L.orc_set_threads.argtypes = [C.c_int]
        # one thread unless a test asks for more: on a box whose core count exceeds this process's CPU share (the GPU
        # box: 256 cores, 16 granted) the OpenMP default makes every parallel region of a small problem take milliseconds
        L.orc_set_threads(1)
        _lib = L
    return _lib


def level_sizes(c, L):
    return [(c - 1) * (1 << l) + 1 for l in range(L)]


class Hierarchy:
    """Three level hierarchies u, d, r as the reference allocates them (mg_3d.h:30-48)."""

    def __init__(self, c, L):
        self.c, self.L = c, L
        self.N = level_sizes(c, L)
        self.u = [np.zeros(n ** 3) for n in self.N]
        self.d = [np.zeros(n ** 3) for n in self.N]
        self.r = [np.zeros(n ** 3) for n in self.N]

    def ptrs(self, xs):
        return (dp * self.L)(*[P(a) for a in xs])


def run_problem(c, L, nu, cycles, mode=0, want_u=True):
    N = level_sizes(c, L)[-1]
    norms = np.zeros(cycles)
    u = np.zeros(N ** 3) if want_u else None
    init = C.c_double(0)
    secs = lib().orc_run_problem(c, L, nu, cycles, mode, P(norms), P(u) if want_u else None, C.byref(init))
    return norms, u, init.value, secs


def run_problem_shift(c, L, nu, sigma, cycles, want_u=True):
    """orc_run_problem_shift: run_problem (mode 0) with the screened operator"""
    N = level_sizes(c, L)[-1]
    norms = np.zeros(cycles)
    u = np.zeros(N ** 3) if want_u else None
    init = C.c_double(0)
    secs = lib().orc_run_problem_shift(c, L, nu, sigma, cycles, P(norms), P(u) if want_u else None, C.byref(init))
    return norms, u, init.value, secs


def exact_residual_norm(u, d, N, h):
    """sqrt of the EXACTLY ROUNDED sum of the squared residuals of (u, d): the residual field from the oracle
    (mg_3d.h:819-821; bit-identical to the GPU's diffs whenever u and d are), each square rounded to double as both
    sides do, the sum in extended precision by numpy's pairwise summation (error ~ log2(n) 2^-64: nothing at the 1e-13 the
    GPU reduction is held to).  The oracle's own return value is the reference's SEQUENTIAL sum and carries that sum's
    rounding error (up to n 2^-53): it pins the reference's number, this pins the GPU's reduction."""
    res = np.zeros(N ** 3)
    lib().orc_residual(P(np.ascontiguousarray(u)), P(np.ascontiguousarray(d)), N, h, P(res))
    sq = res * res
    total = np.longdouble(0)
    step = 1 << 24
    for a in range(0, sq.size, step):  # chunked: the extended-precision copy of a 513^3 field would be 2 GB
        total += np.sum(sq[a:a + step].astype(np.longdouble))
    return float(np.sqrt(total))


class EsParams(C.Structure):
    """orc_es_params (same layout as the product's mg3d_es_params); defaults = mg_3d_bkup.c:12-18"""
    _fields_ = [("length", C.c_double), ("capillary_radius", C.c_double), ("extractor_inner", C.c_double),
                ("extractor_outer", C.c_double), ("capillary_voltage", C.c_double), ("extractor_voltage", C.c_double)]

    def __init__(self):
        super().__init__(3e-4, 1.326e-5, 1e-4, 1.4e-4, 0.0, -1350.0)


def es_run(c, L, nu, cycles, params=None):
    p = params or EsParams()
    N = level_sizes(c, L)[-1]
    norms, u, init = np.zeros(cycles), np.zeros(N ** 3), C.c_double(0)
    lib().orc_es_run(c, L, nu, cycles, C.byref(p), P(norms), P(u), C.cast(C.byref(init), dp))
    return norms, u, init.value


ES_SETS = ("default", "wide", "lattice")
ES_LATTICE_H = 2.0 ** -10


def es_params(name, N=None):
    """A named parameter set of the mixed-boundary problem for a finest level of N^3, as (EsParams of the oracle, EsParams
    of the binding): the same six doubles under the two structs' field names.
    default  mg_3d_bkup.c:12-18: both patches in the middle of their faces, the capillary at 0 V.
    wide     an annulus that reaches the rows next to the walls and the face edges, a disc of thousands of points at 75 V.
    lattice  h = 2^-10 and radii that are whole multiples of it: rr and the squared radii are exact, so the inclusive
             disc (5h: the offsets (3, 4) and (5, 0) lie ON it) and the strict annulus (10h .. 13h: (6, 8) and (5, 12) lie
             on its two circles) are met with equality on the finest level.  The solver takes grid_length = length."""
    p = EsParams()
    if name == "wide":
        p.capillary_radius, p.extractor_inner, p.extractor_outer, p.capillary_voltage = 0.9e-4, 1.2e-4, 2.0e-4, 75.0
    elif name == "lattice":
        h = ES_LATTICE_H
        p.length = (N - 1) * h
        p.capillary_radius, p.extractor_inner, p.extractor_outer = 5 * h, 10 * h, 13 * h
        p.capillary_voltage, p.extractor_voltage = 75.0, -1350.0
    else:
        assert name == "default", name
    from multigrid_parallel_amd.binding import EsParams as ProductEsParams
    return p, ProductEsParams(*[getattr(p, f) for f, _ in EsParams._fields_])


def es_patches(p, N, h):
    """the Dirichlet patches of an N^3 level with spacing h as two (N, N) bool arrays over (j, k): x = 0 and x = L"""
    L_ = lib()
    x0 = np.array([[L_.orc_es_dirichlet_x0(C.byref(p), h, j, k) for k in range(N)] for j in range(N)], dtype=bool)
    xl = np.array([[L_.orc_es_dirichlet_xl(C.byref(p), h, j, k) for k in range(N)] for j in range(N)], dtype=bool)
    return x0, xl


def es_factor(c, h0, p):
    """the factored coarsest operator of the mixed-boundary problem as orc_es_run builds it"""
    A = np.zeros(c ** 3 * c ** 3)
    lib().orc_es_coarse_matrix(P(A), c, h0, C.byref(p))
    lib().orc_lu_factor(P(A), c ** 3)
    return A


def es_vcycle(H, nu, LU, p):
    """one orc_es_vcycle from the finest level of the Hierarchy H (u, d, r of every level stay observable); its norm"""
    N = H.N[-1]
    return lib().orc_es_vcycle(H.ptrs(H.u), H.ptrs(H.d), H.ptrs(H.r), p.length / (N - 1), H.L - 1, H.L, nu, N, P(LU), C.byref(p))
