"""The nonlinear solve on the CPU (no GPU needed): the numpy restatement tests/_nl_ref.py of mg3d_nl_solve on the problems of
the GPU tests -- what it needs there (the caps tests/test_gpu_nl.py uses), why it has a line search, that it is second order
-- and the C boundary of the new entry points."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _nl_ref as NL
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import SIGNATURES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mg3d_nl_setup", "mg3d_nl_set_weight", "mg3d_nl_set_weight_device", "mg3d_nl_residual", "mg3d_nl_solve")


@pytest.mark.parametrize("N,L", [(17, 3), (33, 4)])
@pytest.mark.parametrize("beta", [1.0, 10.0])
def test_boltzmann_converges_within_the_recorded_counts(N, L, beta):
    """Delta u - 50 exp(beta u) = -rho from u = 0 with cycles = 2 V-cycles a step: converged to 1e-8, in exactly the
    iterations and with exactly the largest halving count that _nl_ref.BOLTZMANN_NEEDS records -- 7 steps, halvings
    [5, 2, 0, ...] at beta = 1; 8 steps, [7, 4, 1, 0, ...] at beta = 10, on both grids -- every accepted norm below its
    predecessor by the Armijo factor, and the end quadratic.  The caps of the GPU tests are these + 2 and + 1."""
    term, u0, d = NL.boltzmann_problem(N, 50.0, beta)
    u, norms, info = NL.solve(NL.Problem(5, L, term), u0, d, max_newton=40, cycles=2, rtol=1e-8, max_halvings=20)
    hv = info["halvings_per_step"]
    print(N, beta, info["iterations"], hv, norms)
    assert info["converged"] and norms[-1] <= 1e-8 * norms[0]
    assert (info["iterations"], max(hv)) == NL.BOLTZMANN_NEEDS[(N, beta)]
    assert hv == ([5, 2] + [0] * 5 if beta == 1.0 else [7, 4, 1] + [0] * 5)
    assert NL.caps(N, beta) == (info["iterations"] + 2, max(hv) + 1)
    for k in range(1, len(norms)):
        assert norms[k] < (1.0 - NL.ARMIJO * 0.5 ** hv[k - 1]) * norms[k - 1]
    ratios = norms[1:] / norms[:-1]
    assert ratios[-3] < 1e-2 and ratios[-2] < 1e-3  # the full steps at the end square the error, down to the linear solves' own
    # max_halvings = 0 must be refused on the first step: the GPU test of a failing line search rests on it
    _, n0, i0 = NL.solve(NL.Problem(5, L, term), u0, d, max_newton=5, cycles=2, max_halvings=0)
    assert i0["iterations"] == 0 and not i0["converged"] and len(n0) == 1


@pytest.mark.parametrize("beta", [1.0, 10.0])
def test_the_undamped_loop_does_not_survive_the_boltzmann_problem(beta):
    """The reason for the line search: the loop of INTEGRATION.md "Screening field" (_shift_field_ref.pb_newton's form) on the
    same problem at 17^3 is not converged after 40 steps (beta = 1: the first step overshoots to a residual of 1e80, which
    then falls by 1/e a step) or turns non-finite (beta = 10: the first step)."""
    term, u0, d = NL.boltzmann_problem(17, 50.0, beta)
    norms = NL.undamped(NL.Problem(5, 3, term), u0, d, 40)
    print(beta, norms[:3], norms[-1], len(norms))
    assert not np.isfinite(norms).all() or (len(norms) == 41 and norms[-1] > 1e-8 * norms[0])
    if beta == 1.0:
        assert np.isfinite(norms).all() and norms[-1] > 1e40 and 0.3 < norms[-1] / norms[-2] < 0.45
    else:
        assert len(norms) == 2 and not math.isfinite(norms[1])


def test_poisson_boltzmann_is_second_order():
    """_shift_field_ref.pb_problem with kappa^2 = 4 through the solver at 17^3 and 33^3: no halving is needed, and the error
    against u* falls about fourfold"""
    err = []
    for N, L in ((17, 3), (33, 4)):
        term, u0, d, ustar = NL.pb_start(N, 4.0)
        u, norms, info = NL.solve(NL.Problem(5, L, term), u0, d, rtol=1e-10)
        assert info["converged"] and info["halvings"] == 0 and info["iterations"] <= 8
        err.append(float(np.abs(u - ustar).max()))
    print(err)
    assert 3.6 < err[0] / err[1] < 4.4


def test_new_symbols_are_declared_exported_bound_and_refuse_null():
    hdr = open(os.path.join(ROOT, "include", "mg3d.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = M.lib()
    raw = C.CDLL(M.lib_path())
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert hasattr(raw, name) and name in SIGNATURES
    for word in ("MG3D_NL_EXP = 0", "MG3D_NL_SINH = 1", "typedef struct mg3d_nl_info"):
        assert word in code
    assert "have no nonlinear solve" in hdr
    one = C.c_double(7.0)
    assert L.mg3d_nl_setup(None, 0, 1.0, 1.0, 0.0) == 1  # MG3D_ERR_ARG
    assert b"mg3d_nl_setup" in L.mg3d_last_error()
    assert L.mg3d_nl_set_weight(None, None) == 1
    assert L.mg3d_nl_set_weight_device(None, None, None) == 1
    assert L.mg3d_nl_residual(None, 0, C.byref(one)) == 1 and one.value == 7.0
    norms = np.full(3, 7.0)
    assert L.mg3d_nl_solve(None, 2, 0, 2, 1e-2, 1e-8, 0.0, 10, norms.ctypes.data_as(C.POINTER(C.c_double)), None) == 1
    assert b"mg3d_nl_solve" in L.mg3d_last_error() and list(norms) == [7.0] * 3
