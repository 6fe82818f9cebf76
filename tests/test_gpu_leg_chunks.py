"""The one-launch legs (csrc/mg3d_sweep.hip, SWEEP_LEG_DOWN / SWEEP_LEG_UP) at forced chunk lengths.  launch_sweep cuts a level
into i-chunks of CI planes; for the legs it always takes the cost model's choice, a function of the device's CU count, so the
other leg tests run whatever 256 CUs give at their size -- chunks of 2 to 12 planes at 81^3 .. 161^3, shorter than the kernel's
warm-up plus drain.  Here option sweep_ci sets the length, and mg3d_ctx_sweep_taken says that the legs ran with it:

    1, 2, 3        shorter than the warm-up            17            odd, longer than the warm-up          32
    (N + 1) // 2   the production layout: two chunks, the second starting on an odd plane
    N // 2         an even start and a third chunk of one plane
    N - 1          a last chunk of one plane           N             one chunk

Schedule as tests/test_gpu_dnone.py (legs_min = carry_min = 66, legs = 1, carry = 0) with sweep_tune = 0, and its call pattern
_cycles: tapped and untapped legs, a leg behind a red tail, the down-leg mg3d_vcycle runs ahead.  Sizes as
tests/test_gpu_dnone_restrict.py: 81^3 one k-tile and a last j-tile mostly outside the grid, 97^3 several j-tiles, 129^3 two
k-tiles, 161^3 a partly empty second k-tile.  Kernel families, by what the legs do with d:

    nod_bench   no d (ND): the benchmark's problem, d_zero_skip = 1
    nod_rand    no d (ND): the same with a seeded random u inside, so that neighbouring r values do not nearly cancel
    map         the d window through a partial zero map (DZ): random u, a d with a band of non-zero interior planes
    dense       the d window reading every plane: random u, dense random d, d_zero_skip = 0

Every length meets every family at 129^3; 1, (N + 1) // 2, N - 1 and N meet every family at all four sizes.  The bar of each
case: u of the finest level bitwise the oracle's (signed zeros included); u of every level and d of every level below the finest
bitwise those of the plain schedule (legs = 0, carry = 0, d_zero_skip = 0, sweep_ci = 0: computed once per size and problem);
every norm against the plain run's at 1e-13 (only the grouping of the partial sums differs) and the oracle's at norm_rtol, the
last one against the exactly rounded sum."""
import numpy as np
import pytest
import torch  # before the package, as bench.py does: the HIP runtime is torch's

import _oracle as O
import _screened_ref as S
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U
from test_gpu_dnone import _cycles, _same
from test_gpu_parity import EXACT_NORM_RTOL, assert_norm_exact, norm_rtol

pytestmark = pytest.mark.gpu

SIZES = {81: (6, 5), 97: (7, 5), 129: (9, 5), 161: (11, 5)}
FAMILIES = ("nod_bench", "nod_rand", "map", "dense")
CYCLES = 6  # of _cycles
LEG_PARTIALS_CAP = 32768 // 2  # MG3D_MAX_PARTIALS / 2: each leg launch forms half a norm (csrc/mg3d_ctx.hip, part_a / part_b)
SIGMA = 37.5


def lengths(N):
    return [1, 2, 3, 17, 32, (N + 1) // 2, N // 2, N - 1, N]


def lengths_everywhere(N):
    return [1, (N + 1) // 2, N - 1, N]


CASES = [(N, fam, ci) for N in sorted(SIZES) for fam in FAMILIES for ci in (lengths(N) if N == 129 else lengths_everywhere(N))]


# ------------------------------------------------------------------------------------------------------------ the problems
_starts = {}


def start(N, fam):
    """u and d of the finest level, dense N^3: the reference's boundary function on the faces of both, the family's interior"""
    if (N, fam) not in _starts:
        h = 1.0 / (N - 1)
        u = np.zeros(N ** 3)
        O.lib().orc_fill_boundary(O.P(u), N, h)
        d = u.copy()
        u3, d3 = u.reshape(N, N, N), d.reshape(N, N, N)
        rng = np.random.default_rng(4000 + N)
        if fam != "nod_bench":
            u3[1:-1, 1:-1, 1:-1] = rng.uniform(-1., 1., (N - 2,) * 3)
        if fam == "map":  # six planes, from an odd one on: every other interior plane stays +0.0
            lo = N // 3 | 1
            d3[lo:lo + 6, 1:-1, 1:-1] = rng.uniform(-50., 50., (6, N - 2, N - 2))
        elif fam == "dense":
            d3[1:-1, 1:-1, 1:-1] = rng.uniform(-50., 50., (N - 2,) * 3)
        _starts[(N, fam)] = (u, d)
    return _starts[(N, fam)]


def load(s, N, fam):
    """the family's start on a Solver.  The no-d families keep the d mg3d_setup_test_problem wrote (its zero map is full without
    a scan); the others upload theirs"""
    u, d = start(N, fam)
    top = SIZES[N][1] - 1
    s.setup_test_problem()
    if fam != "nod_bench":
        s.upload(MG3D_U, top, u)
    if fam in ("map", "dense"):
        s.upload(MG3D_D, top, d)


def solver(N, fam, ci, legs=True, sigma=0.0):
    c, L = SIZES[N]
    s = M.Solver(c, L, 2)
    assert s.N == N
    s.set_option("legs_min", 66)
    s.set_option("carry_min", 66)
    s.set_option("legs", 1 if legs else 0)
    s.set_option("carry", 0)
    s.set_option("sweep_tune", 0)
    s.set_option("sweep_ci", ci)
    s.set_option("d_zero_skip", (0 if fam == "dense" else 1) if legs else 0)
    if sigma:
        s.set_shift(sigma)
    return s


def levels(s):
    top = s.num_levels - 1
    return [s.download(MG3D_U, l) for l in range(top + 1)], [s.download(MG3D_D, l) for l in range(top)]


_plain, _oracle, _screened = {}, {}, {}


def plain(N, fam, sigma=0.0):
    """norms, u of every level, d of every level below the finest: the plain schedule, the model's chunks, every plane of d read"""
    if (N, fam, sigma) not in _plain:
        with solver(N, fam, 0, legs=False, sigma=sigma) as s:
            load(s, N, fam)
            norms = np.array(_cycles(s))
            _plain[(N, fam, sigma)] = (norms,) + tuple(levels(s))
    return _plain[(N, fam, sigma)]


def oracle(N, fam):
    """norms and u of the finest level after the cycles of _cycles, from oracle/: run_problem for the benchmark's problem, a
    Hierarchy stepped with orc_vcycle for the others"""
    if (N, fam) not in _oracle:
        c, L = SIZES[N]
        lib = O.lib()
        lib.orc_set_threads(8)
        try:
            if fam == "nod_bench":
                norms, u, _, _ = O.run_problem(c, L, 2, CYCLES)
            else:
                H = O.Hierarchy(c, L)
                assert H.N[-1] == N
                h = 1.0 / (N - 1)
                u0, d0 = start(N, fam)
                H.u[-1][:] = u0
                H.d[-1][:] = d0
                LU = np.zeros(c ** 3 * c ** 3)
                lib.orc_coarse_matrix(O.P(LU), c, h * (1 << (L - 1)))
                (lib.orc_lu_factor_banded if c > 9 else lib.orc_lu_factor)(O.P(LU), c ** 3)
                norms = np.array([lib.orc_vcycle(H.ptrs(H.u), H.ptrs(H.d), H.ptrs(H.r), h, L - 1, L, 2, N, O.P(LU))
                                  for _ in range(CYCLES)])
                u = H.u[-1]
        finally:
            lib.orc_set_threads(1)
        _oracle[(N, fam)] = (norms, u)
    return _oracle[(N, fam)]


def screened(N, fam):
    """the same from tests/_screened_ref.py with sigma = SIGMA"""
    if (N, fam) not in _screened:
        c, L = SIZES[N]
        ref = S.Problem(c, L, 2, SIGMA)
        u0, d0 = start(N, fam)
        ref.u[-1][...] = u0.reshape(N, N, N)
        ref.d[-1][...] = d0.reshape(N, N, N)
        norms = ref.vcycles(CYCLES)
        _screened[(N, fam)] = (norms, ref.flat("u", L - 1))
    return _screened[(N, fam)]


# ------------------------------------------------------------------------------------------------------------ the records
def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def check_leg_records(s, N, fam, ci):
    """the launches mg3d_ctx_sweep_taken reports for the two legs: the kernels of the family, the forced chunk length, a grid
    within the legs' room for partial sums, the block numbering launch_sweep documents for that many blocks, and the launches of
    _cycles -- down-leg: 3 behind a cycle whose norm it completes (TAP 0), 2 behind a finished cycle; up-leg: 3 that start a
    norm (TAP 4), 3 that end a call.  Returns {leg: xcd_remap}"""
    nd, dz = int(fam.startswith("nod")), int(fam == "map")
    want = {"leg_down": dict(S=3, RES=2, RJ=4, NW=8, PF=1, PRO=0, counts={0: 3, -1: 2}),
            "leg_up": dict(S=4, RES=0, RJ=4, NW=8, PF=2 if nd else 1, PRO=1, counts={4: 3, -1: 3})}
    remap = {}
    for leg, w in want.items():
        launches, recs = s.sweep_taken(leg)
        assert launches == sum(w["counts"].values()), (leg, launches)
        assert {r["TAP"]: r["count"] for r in recs} == w["counts"] and len(recs) == 2, (leg, recs)
        for r in recs:
            assert r["N"] == N and r["ND"] == nd and r["DZ"] == dz, (leg, r)
            assert all(r[k] == w[k] for k in ("S", "RES", "RJ", "NW", "PF", "PRO")), (leg, r)
            assert r["CI"] == min(ci, N), (leg, r)  # precondition: the forced length reached the leg
            assert r["ntk"] == (1 if N <= 128 else 2) and r["ntj"] >= 2, (leg, r)
            assert r["blocks"] == r["ntj"] * r["ntk"] * -(-N // r["CI"]), (leg, r)
            assert r["blocks"] <= LEG_PARTIALS_CAP, (leg, r)  # precondition: no launch can be refused for partial sums
            assert r["xcd_remap"] == (0 if r["blocks"] < 64 else 1 if r["blocks"] <= cus() else 2), (leg, r, cus())
        assert recs[0]["xcd_remap"] == recs[1]["xcd_remap"]
        remap[leg] = recs[0]["xcd_remap"]
    return remap


_remaps = {}  # (N, fam, ci) -> {leg: xcd_remap}, filled by the matrix below


def run_case(N, fam, ci, sigma=0.0):
    base = plain(N, fam, sigma)
    want_norms, want_u = screened(N, fam) if sigma else oracle(N, fam)
    top = SIZES[N][1] - 1
    with solver(N, fam, ci, sigma=sigma) as s:
        load(s, N, fam)
        norms = np.array(_cycles(s))
        assert len(norms) == CYCLES
        remap = check_leg_records(s, N, fam, ci)
        assert s.dnone_launches() == (11 if fam.startswith("nod") else 0)
        us, ds = levels(s)
        _same(us[top], want_u, "u of the finest level against the oracle")
        assert len(us) == len(base[1]) == top + 1 and len(ds) == len(base[2]) == top
        for l, (x, y) in enumerate(zip(us, base[1])):
            _same(x, y, f"u of level {l} against the plain schedule")
        for l, (x, y) in enumerate(zip(ds, base[2])):
            _same(x, y, f"d of level {l} against the plain schedule")
        assert np.count_nonzero(ds[-1]) > ds[-1].size // 4  # (the restriction's output is no field of zeros)
        print(f"norms {norms!r}\nplain {base[0]!r}\nmax rel {np.max(np.abs(norms / base[0] - 1.)):.3e}")
        assert np.all(np.isfinite(norms)) and np.all(norms > 0.)
        np.testing.assert_allclose(norms, base[0], rtol=1e-13)
        np.testing.assert_allclose(norms, want_norms, rtol=norm_rtol(N))
        if sigma:
            want = S.exact_residual_norm(us[top], s.download(MG3D_D, top), N, s.level_h(top), sigma)
            assert norms[-1] == pytest.approx(want, rel=EXACT_NORM_RTOL), (norms[-1], want)
        else:
            assert_norm_exact(s, top, norms[-1])
    return remap


def test_the_getter_counts_launches_and_refuses_bad_arguments():
    """mg3d_ctx_sweep_taken on a 33^3 context: nothing before the first cycle; afterwards the counts of a kind's distinct
    records add up to its launches, the legs and the tapped launch never ran (below their thresholds), a record past the end is
    zeroed with count 0, and a kind that does not exist or a negative index is MG3D_ERR_ARG"""
    import ctypes as C
    from multigrid_parallel_amd.binding import SWEEP_KINDS, SWEEP_TAKEN_FIELDS
    with M.Solver(5, 4, 2) as s:
        s.setup_test_problem()
        assert all(s.sweep_taken(kind) == (0, []) for kind in SWEEP_KINDS)
        s.vcycles(3)
        for kind in ("passes", "passes_res"):
            launches, recs = s.sweep_taken(kind)
            assert launches > 0 and sum(r["count"] for r in recs) == launches
            assert {r["N"] for r in recs} == {17, 33}  # (9^3 runs in one workgroup: mg3d_tiny.hip, no sweep launch)
            assert len({tuple(r[f] for f in SWEEP_TAKEN_FIELDS) for r in recs}) == len(recs)
        assert all(s.sweep_taken(kind) == (0, []) for kind in ("tap", "leg_down", "leg_up"))
        out = (C.c_int * len(SWEEP_TAKEN_FIELDS))(*([7] * len(SWEEP_TAKEN_FIELDS)))
        count = C.c_ulonglong(7)
        assert s.L.mg3d_ctx_sweep_taken(s._h, SWEEP_KINDS["passes"], 32, out, C.byref(count), None) == 0
        assert list(out) == [0] * len(SWEEP_TAKEN_FIELDS) and count.value == 0
        for kind, which in ((-1, 0), (len(SWEEP_KINDS), 0), (0, -1)):
            assert s.L.mg3d_ctx_sweep_taken(s._h, kind, which, out, None, None) == 1


@pytest.mark.parametrize("N,fam,ci", CASES, ids=[f"{N}-{fam}-ci{ci}" for N, fam, ci in CASES])
def test_forced_chunk_length_changes_no_bit(N, fam, ci):
    _remaps[(N, fam, ci)] = run_case(N, fam, ci)


@pytest.mark.parametrize("fam", FAMILIES)
def test_every_block_numbering_runs_on_each_leg_kernel(fam):
    """xcd_remap: 0 blocks as numbered, 1 the whole grid regrouped (one round of blocks), 2 every chunk's layer regrouped
    (several rounds).  On 256 CUs the lengths N, 17 and 2 at 129^3 give 12, 96 and 780 blocks: all three on each leg kernel.
    On a part with another CU count the matrix above still holds each launch to launch_sweep's rule for its own count"""
    N = 129
    seen = {"leg_down": set(), "leg_up": set()}
    for ci in (N, 17, 2):
        if (N, fam, ci) not in _remaps:
            _remaps[(N, fam, ci)] = run_case(N, fam, ci)
        for leg, v in _remaps[(N, fam, ci)].items():
            seen[leg].add(v)
    if cus() == 256:
        assert seen == {"leg_down": {0, 1, 2}, "leg_up": {0, 1, 2}}, seen


@pytest.mark.parametrize("fam", ["nod_bench", "map", "dense"])
def test_production_layout_screened(fam):
    """sigma > 0 (dg != 6 in the residual the down-leg restricts) at the production layout of 129^3: two chunks, the second
    one starting on an odd plane; against tests/_screened_ref.py"""
    N = 129
    run_case(N, fam, (N + 1) // 2, sigma=SIGMA)
