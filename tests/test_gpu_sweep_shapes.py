"""Every compiled tile shape of the fused sweep gives the default shape's bits.  The TRY lists of dispatch<S, RES>
(csrc/mg3d_sweep.hip; mirrored in TRY below, and compared with the source by the first test) compile 43 shapes (RJ rows a
thread, NW waves, PF planes in flight) that the options sweep_rj / sweep_nw / sweep_pf (MG3D_SWEEP_CFG) select; the A/B tools
rely on them to compute what the default computes.  A request that names no compiled shape runs the default, so each case
FIRST asks mg3d_ctx_sweep_taken whether the requested shape ran for its family on the finest level: a silent fall-back fails.

The schedule and nu that bring a family <S, RES> onto the finest level (all with legs = 0 unless said, sweep_tune = 0):

    plain      legs = 0, carry = 0, nu = 2     <4,0> the pre-smoother's four passes, <0,2> residual + restriction, and the
                                               norm-only pair (RST = false: <2,1> 4,8,1 and 4,8,2 without a stored r) of the
                                               post-smoother's second launch
    keep_r     plain with mg3d_ctx_set_keep_residual, nu = 2       <0,1> the residual stored
    v11_keep_r the same with nu = 1            <2,1> two passes + the residual stored (every shape of the list, 4,8,1 too)
    v11_split  plain, nu = 1, fuse_rst2 = 0    <2,0> the pre-smoother's two passes
    v11_fused  plain, nu = 1, fuse_rst2 = 1    <2,2> two passes + residual + restriction
    leg4       plain, nu = 2, fuse_leg_max = 2^20                  <4,2> the whole down-leg in one two-row launch
    carried    carry = 1, carry_min = 66, nu = 2                   <1,2> one pass + residual + restriction, <4,3> the tapped launch
    legs       legs = 1, legs_min = carry_min = 66, carry = 0, nu = 2, option sweep_pf alone: the other planes-in-flight
               instantiation of the four leg kernels without d (3 - MG3D_LEG_ND_PF_DOWN / _UP), on problems whose d is +0 inside

<4,1> (four passes + residual without restriction, five shapes) is in the mirror but has no case: mg3d_stage_plan never puts a
residual on a four-pass launch unless it restricts (<4,2>), so no schedule of the library reaches it.

Sizes: 97^3, several j-tiles for every tile height (16, 24, 32, 48 rows) and one k-tile; 161^3, a partly empty second k-tile.
Problems: the benchmark's and two seeded random right-hand sides (the legs cases: the benchmark's and a random u inside).
Each case: u of every level and d of every level below the finest bitwise equal to the default-shape run of the same schedule
(computed once per size and schedule, and held once to the oracle: u of the finest level bitwise, norms at norm_rtol); every
norm against that run's at 1e-13 (only the grouping of the partial sums differs), the last against the exactly rounded sum."""
import os
import re

import numpy as np
import pytest
import torch  # noqa: F401  before the package, as bench.py does: the HIP runtime is torch's

import _oracle as O
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U
from test_gpu_dnone import _cycles, _same
from test_gpu_parity import assert_norm_exact, norm_rtol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {97: (7, 5), 161: (11, 5)}

# csrc/mg3d_sweep.hip, the TRY lists of dispatch<S, RES>: (S, RES) -> [(RJ, NW, PF)]
TRY = {
    (4, 1): [(6, 4, 1), (6, 4, 2), (4, 4, 2), (4, 8, 1), (2, 8, 2)],
    (4, 0): [(8, 4, 1), (6, 4, 2), (6, 4, 3), (4, 8, 1), (4, 8, 2), (2, 8, 2), (2, 8, 4), (2, 16, 1)],
    (2, 1): [(4, 8, 1), (8, 4, 2), (6, 4, 2), (2, 16, 1), (6, 8, 1)],
    (2, 0): [(6, 8, 1), (8, 4, 2), (4, 8, 1), (4, 8, 2), (4, 8, 3), (2, 8, 4), (2, 16, 1)],
    (0, 1): [(4, 8, 1), (8, 4, 2), (4, 8, 2), (4, 8, 3), (2, 8, 4), (2, 16, 1)],
    (0, 2): [(4, 8, 1), (4, 8, 2), (2, 8, 2), (2, 8, 4), (2, 16, 1), (6, 8, 1)],
    (4, 2): [(2, 8, 1), (2, 8, 2)],
    (2, 2): [(4, 8, 1)],
    (1, 2): [(4, 8, 1), (4, 8, 2)],
    (4, 3): [(4, 8, 1)],
}
UNREACHABLE = {(4, 1)}  # see the docstring

# family -> (schedule, kind of launch, fields that tell the family's launch of the finest level from the others of its kind)
FAMILY = {
    (4, 0): ("plain", "passes", dict(PRO=0)),
    (0, 2): ("plain", "passes_res", dict()),
    (0, 1): ("keep_r", "passes_res", dict()),
    (2, 1): ("v11_keep_r", "passes_res", dict(RST=1)),
    (2, 0): ("v11_split", "passes", dict(PRO=0)),
    (2, 2): ("v11_fused", "passes_res", dict()),
    (4, 2): ("leg4", "passes_res", dict()),
    (1, 2): ("carried", "passes_res", dict()),
    (4, 3): ("carried", "tap", dict()),
}
# name -> (nu, keep_residual, options)
SCHEDULES = {
    "plain": (2, False, dict(legs=0, carry=0)),
    "keep_r": (2, True, dict(legs=0, carry=0)),
    "v11_keep_r": (1, True, dict(legs=0, carry=0)),
    "v11_split": (1, False, dict(legs=0, carry=0, fuse_rst2=0)),
    "v11_fused": (1, False, dict(legs=0, carry=0, fuse_rst2=1)),
    "leg4": (2, False, dict(legs=0, carry=0, fuse_leg_max=1 << 20)),
    "carried": (2, False, dict(legs=0, carry=1, carry_min=66)),
    "legs": (2, False, dict(legs=1, carry=0, legs_min=66, carry_min=66)),
}
PROBLEMS = ("benchmark", "rhs1", "rhs2")
LEG_PROBLEMS = ("benchmark", "random_u")  # d +0 inside: the kernels without d


def test_the_mirror_equals_the_try_lists():
    """the mirror against the TRY lists of csrc/mg3d_sweep.hip: a shape added there has no case here until it is listed"""
    src = open(os.path.join(ROOT, "multigrid_parallel_amd", "csrc", "mg3d_sweep.hip")).read()
    got = {}
    for s_, res, rj, nw, pf in re.findall(r"\bTRY\((\d+), (\d+), (\d+), (\d+), (\d+)\)", src):
        got.setdefault((int(s_), int(res)), []).append((int(rj), int(nw), int(pf)))
    assert got == TRY
    assert sum(len(v) for v in TRY.values()) == 43 and set(FAMILY) | UNREACHABLE == set(TRY)


# ------------------------------------------------------------------------------------------------------------ the problems
_starts = {}


def start(N, problem):
    """(u, d) of the finest level to upload behind mg3d_setup_test_problem; None: keep what that wrote"""
    if (N, problem) not in _starts:
        h = 1.0 / (N - 1)
        face = np.zeros(N ** 3)
        O.lib().orc_fill_boundary(O.P(face), N, h)
        u, d = None, None
        if problem in ("rhs1", "rhs2"):
            d = face.copy()
            d.reshape(N, N, N)[1:-1, 1:-1, 1:-1] = np.random.default_rng(7000 + 10 * N + int(problem[-1])).uniform(-50., 50., (N - 2,) * 3)
        elif problem == "random_u":
            u = face.copy()
            u.reshape(N, N, N)[1:-1, 1:-1, 1:-1] = np.random.default_rng(7000 + 10 * N).uniform(-1., 1., (N - 2,) * 3)
        else:
            assert problem == "benchmark"
        _starts[(N, problem)] = (face, u, d)
    return _starts[(N, problem)]


def pattern(sched):
    if sched == "legs":
        return _cycles  # six cycles: tapped and untapped legs
    return lambda s: list(s.vcycles(3)) + list(s.vcycles(1))


def run(N, sched, shape, problems):
    """one Solver, every problem in turn: [(norms, u of every level, d of every level below the finest)], the solver's records
    by kind, and the check of the last norm of each problem against the exactly rounded sum"""
    c, L = SIZES[N]
    nu, keep_r, options = SCHEDULES[sched]
    out = []
    with M.Solver(c, L, nu) as s:
        assert s.N == N
        for k, v in dict(options, sweep_tune=0, **shape).items():
            s.set_option(k, v)
        if keep_r:
            s.set_keep_residual(True)
        for problem in problems:
            _, u, d = start(N, problem)
            s.setup_test_problem()
            if u is not None:
                s.upload(MG3D_U, L - 1, u)
            if d is not None:
                s.upload(MG3D_D, L - 1, d)
            norms = np.array(pattern(sched)(s))
            assert np.all(np.isfinite(norms)) and np.all(norms > 0.)
            assert_norm_exact(s, L - 1, norms[-1])
            out.append((norms, [s.download(MG3D_U, l) for l in range(L)], [s.download(MG3D_D, l) for l in range(L - 1)]))
        taken = {kind: s.sweep_taken(kind)[1] for kind in ("passes", "passes_res", "tap", "leg_down", "leg_up")}
    return out, taken


_oracle = {}


def oracle(N, nu, problem, cycles):
    if (N, nu, problem, cycles) not in _oracle:
        c, L = SIZES[N]
        lib = O.lib()
        lib.orc_set_threads(8)
        try:
            if problem == "benchmark":
                norms, u, _, _ = O.run_problem(c, L, nu, cycles)
            else:
                face, u0, d0 = start(N, problem)
                H = O.Hierarchy(c, L)
                h = 1.0 / (N - 1)
                H.u[-1][:] = face if u0 is None else u0
                H.d[-1][:] = face if d0 is None else d0
                LU = np.zeros(c ** 3 * c ** 3)
                lib.orc_coarse_matrix(O.P(LU), c, h * (1 << (L - 1)))
                (lib.orc_lu_factor_banded if c > 9 else lib.orc_lu_factor)(O.P(LU), c ** 3)
                norms = np.array([lib.orc_vcycle(H.ptrs(H.u), H.ptrs(H.d), H.ptrs(H.r), h, L - 1, L, nu, N, O.P(LU))
                                  for _ in range(cycles)])
                u = H.u[-1]
        finally:
            lib.orc_set_threads(1)
        _oracle[(N, nu, problem, cycles)] = (norms, u)
    return _oracle[(N, nu, problem, cycles)]


_defaults = {}


def default_run(N, sched):
    """the default shapes under the schedule, held once to the oracle"""
    if (N, sched) not in _defaults:
        problems = LEG_PROBLEMS if sched == "legs" else PROBLEMS
        out, taken = run(N, sched, {}, problems)
        for problem, (norms, us, _) in zip(problems, out):
            want_norms, want_u = oracle(N, SCHEDULES[sched][0], problem, len(norms))
            _same(us[-1], want_u, f"default shapes, {sched}, {problem}: u of the finest level against the oracle")
            np.testing.assert_allclose(norms, want_norms, rtol=norm_rtol(N))
        _defaults[(N, sched)] = (out, taken)
    return _defaults[(N, sched)]


def top_records(taken, kind, N, **fields):
    return [r for r in taken[kind] if r["N"] == N and all(r[k] == v for k, v in fields.items())]


def assert_same_as_default(N, sched, out, problems):
    base = default_run(N, sched)[0]
    assert len(out) == len(base) == len(problems)
    for problem, got, want in zip(problems, out, base):
        for l, (x, y) in enumerate(zip(got[1], want[1])):
            _same(x, y, f"{problem}: u of level {l}")
        for l, (x, y) in enumerate(zip(got[2], want[2])):
            _same(x, y, f"{problem}: d of level {l}")
        assert len(got[1]) == len(want[1]) == SIZES[N][1] and len(got[2]) == len(want[2]) == SIZES[N][1] - 1
        print(f"{problem}: norms {got[0]!r}\ndefault {want[0]!r}\nmax rel {np.max(np.abs(got[0] / want[0] - 1.)):.3e}")
        np.testing.assert_allclose(got[0], want[0], rtol=1e-13)


SHAPE_CASES = [(fam, shape) for fam in TRY if fam not in UNREACHABLE for shape in TRY[fam]]


@pytest.mark.parametrize("N", sorted(SIZES))
@pytest.mark.parametrize("fam,shape", SHAPE_CASES, ids=["S%d-RES%d-%d.%d.%d" % (f + sh) for f, sh in SHAPE_CASES])
def test_compiled_shape_gives_the_bits_of_the_default(N, fam, shape):
    sched, kind, tell = FAMILY[fam]
    S_, RES = fam
    # the schedule brings the family onto the finest level (seen in the default run's own records)
    assert top_records(default_run(N, sched)[1], kind, N, S=S_, RES=RES, **tell), "the schedule does not reach the family"
    rj, nw, pf = shape
    out, taken = run(N, sched, dict(sweep_rj=rj, sweep_nw=nw, sweep_pf=pf), PROBLEMS)
    recs = top_records(taken, kind, N, S=S_, RES=RES, **tell)
    assert recs, "the family did not run on the finest level"
    for r in recs:
        assert (r["RJ"], r["NW"], r["PF"]) == shape, f"asked for {shape}, ran {r}"
        assert r["ntk"] == (1 if N <= 128 else 2) and r["blocks"] == r["ntj"] * r["ntk"] * -(-N // r["CI"]), r
    assert_same_as_default(N, sched, out, PROBLEMS)


@pytest.mark.parametrize("N", sorted(SIZES))
@pytest.mark.parametrize("pf", [1, 2])
def test_norm_only_shapes_give_the_bits_of_the_default(N, pf):
    """the RST = false pair: two passes + the residual NORM (no r assembled), the finest level's second post-smoothing launch"""
    out, taken = run(N, "plain", dict(sweep_rj=4, sweep_nw=8, sweep_pf=pf), PROBLEMS)
    recs = top_records(taken, "passes_res", N, S=2, RES=1)
    assert recs, "the norm launch did not run on the finest level"
    for r in recs:
        assert (r["RJ"], r["NW"], r["PF"], r["RST"]) == (4, 8, pf, 0), r
    assert_same_as_default(N, "plain", out, PROBLEMS)


@pytest.mark.parametrize("N", sorted(SIZES))
@pytest.mark.parametrize("pf", [1, 2])
def test_other_planes_in_flight_of_the_kernels_without_d(N, pf):
    """option sweep_pf alone under the legs schedule: pf = 2 is the down-leg's other instantiation (its default holds one
    plane in flight), pf = 1 the up-leg's (default two); each with and without a norm half.  Both legs then run with pf."""
    dflt = default_run(N, "legs")[1]
    for leg, want in (("leg_down", 1), ("leg_up", 2)):
        recs = top_records(dflt, leg, N)
        assert recs and all(r["ND"] == 1 and r["PF"] == want for r in recs), (leg, recs)
    out, taken = run(N, "legs", dict(sweep_pf=pf), LEG_PROBLEMS)
    for leg, tap in (("leg_down", 0), ("leg_up", 4)):
        recs = top_records(taken, leg, N)
        assert {r["TAP"] for r in recs} == {tap, -1}, (leg, recs)
        for r in recs:
            assert r["ND"] == 1 and r["DZ"] == 0 and (r["RJ"], r["NW"], r["PF"]) == (4, 8, pf), (leg, r)
    assert_same_as_default(N, "legs", out, LEG_PROBLEMS)
