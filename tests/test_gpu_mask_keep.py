"""The KEEP coarsening rule of the fixed-point mask (mg3d_ctx_set_mask_coarsening) and full multigrid with a mask under it
(mg3d_fmg_solve, mg3d_fmg_interpolate) on the GPU, against the numpy restatement tests/_mask_keep_ref.py: the hierarchy on
every level for every shape and boundary combination, the setters in every order, cycles (with eps and with a screening
field), the solvers and the stepper, the default rule untouched, masked FMG, the refusals.  Grid values and mask bytes bit
for bit; norms to the summation tolerance of tests/test_gpu_mask.py (test_gpu_parity.norm_rtol); the iterates and norms
of mg3d_pcg_solve / mg3d_wpcg_solve to the tolerances tests/test_gpu_mask.py holds them to under injection (100 x the
summation spread its files measured on the CPU).  The mask of most tests is _mask_keep_ref.thin_mask: the bodies of
_mask_ref.gpu_test_mask (random 10 %, a thick block, a one-point plate on an odd plane), a needle on odd j, k, and eleven
named points with the room around them cleared so that each IS lost under every boundary mask -- (1,1,1), (N-2,N-2,N-2),
one whose upper parent lies on the last plane of each axis, one on each face (tests/test_mask_keep_host.py asserts it).
Shapes: 17^3 and 33^3 (c = 5), 25^3 (c = 7, off the 2^k+1 ladder), and 65^3 (c = 5, L = 5) for the row pitch past one
k-block of 64 lanes."""
import itertools

import numpy as np
import pytest
import torch  # before the package, as bench.py does: the HIP runtime is torch's

import _coef_ref as CR
import _mask_keep_ref as MK
import _mask_ref as MR
import _neumann_ref as NR
import _shift_field_ref as SF
import _step_ref as SR
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U

from test_gpu_parity import norm_rtol
import test_gpu_mask as TM
import test_gpu_wpcg as TW

pytestmark = pytest.mark.gpu

MG3D_ERR_ARG, MG3D_ERR_STATE = 1, 5
SHAPES = [(5, 3), (5, 4), (7, 3)]
# Dirichlet; one periodic axis (each); all periodic; the Neumann faces one at a time; periodic combined with Neumann
BOUNDARIES = ([(0, 0), (1, 0), (2, 0), (4, 0), (7, 0)] + [(0, 1 << f) for f in range(6)] + [(4, 3), (1, 4 | 32), (2, 1 | 2 | 16)])
FEW = [(0, 0), (5, 0), (0, 1 | 8), (4, 3)]  # those of tests/test_gpu_mask.py


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _n(c, L):
    return (c - 1) * (1 << (L - 1)) + 1


def _solver(c, L, nu, sigma, eps, axes, faces, mask, rule="keep", factor=True, sfield=None):
    s = M.Solver(c, L, nu)
    s.set_shift(sigma)
    s.set_periodic(axes)
    s.set_neumann(faces)
    if eps is not None:
        s.set_coefficient(eps)
    if sfield is not None:
        s.set_shift_field(sfield)
    if rule is not None:
        s.set_mask_coarsening(rule)
    s.set_mask(mask)
    if factor:
        s.get_details()
    return s


def _random_problem(ref, rng, poison=False):
    N = ref.N[-1]
    ref.u[-1][...] = rng.standard_normal((N, N, N))
    ref.d[-1][...] = rng.standard_normal((N, N, N))
    NR.refresh(ref.u[-1], ref.axes)
    NR.refresh(ref.d[-1], ref.axes)
    if poison:
        ref.d[-1][ref.fixed()] = np.nan


def _upload(s, ref):
    s.upload(MG3D_U, ref.L - 1, ref.u[-1])
    s.upload(MG3D_D, ref.L - 1, ref.d[-1])


def _assert_masks(s, want, what=""):
    for l, m in enumerate(want):
        got = s.get_mask(l)
        assert np.array_equal(got, m), f"{what}: the mask of level {l} ({int((got != m).sum())} bytes differ)"


# --------------------------------------------------------------------------------------------------------- 1 hierarchy
@pytest.mark.parametrize("c,L", SHAPES)
@pytest.mark.parametrize("axes,faces", BOUNDARIES)
def test_hierarchy(c, L, axes, faces):
    """get_mask(level) on every level against the restatement; the rule set before the mask and after it; KEEP -> INJECT
    gives the injected hierarchy again; the thin bodies are there: every level below the finest has fixed points that the
    injection lacks"""
    N = _n(c, L)
    mask = MK.thin_mask(N)
    top = MR.stored(mask, axes)
    want, inj = MK.keep(top, L, axes), MR.inject(top, L)
    for l in range(L - 1):
        assert ((want[l] != 0) & (inj[l] == 0)).any(), f"level {l}: no fixed point that injection lacks"
    with M.Solver(c, L, 2) as a, M.Solver(c, L, 2) as b:
        for s in (a, b):
            s.set_periodic(axes)
            s.set_neumann(faces)
        assert a.get_mask_coarsening() == "inject"
        a.set_mask_coarsening("keep")
        assert a.get_mask_coarsening() == "keep" and not a.has_mask()
        a.set_mask(mask)
        b.set_mask(mask)
        _assert_masks(b, inj, "default rule")
        b.set_mask_coarsening(1)
        _assert_masks(a, want, "rule before the mask")
        _assert_masks(b, want, "rule after the mask")
        b.set_mask_coarsening("keep")  # the same rule again
        _assert_masks(b, want, "the same rule again")
        b.set_mask_coarsening("inject")
        _assert_masks(b, inj, "KEEP -> INJECT")
        a.set_mask(None)
        assert a.get_mask_coarsening() == "keep"
        a.set_mask(mask)  # the stored rule applies to the next mask
        _assert_masks(a, want, "the next mask")


@pytest.mark.parametrize("axes,faces", [(0, 0), (7, 0), (2, 1 | 2 | 16)])
def test_hierarchy_at_65(axes, faces):
    """65^3: the fine level's rows of bytes are longer than one block of 64 lanes.  mask_keep_kernel runs one thread per
    COARSE point and the coarse side is 33 here, so its threads stay in one k-block; the second block of threads, with
    lost points behind coarse column 63, is reached in tests/test_gpu_mask_keep_shapes.py (145^3 .. 193^3)"""
    c, L, N = 5, 5, 65
    mask = MK.thin_mask(N)
    for p in itertools.product((61, 63), (1, 63), (62, 63, 64)):  # lost points around the lane-block boundary
        mask[p] = 8
    want = MK.keep(MR.stored(mask, axes), L, axes)
    with _solver(c, L, 2, 0.0, None, axes, faces, mask, factor=False) as s:
        _assert_masks(s, want, "65^3")


SETTERS = ("shift", "coef", "periodic", "neumann", "mask", "rule")
_ORDER_REF = {}


def _order_case():
    """the problem of the setter-order tests and its restatement, computed once"""
    if not _ORDER_REF:
        c, L, N = 5, 3, 17
        sigma, axes, faces = 3.5, 4, 3
        eps, mask = CR.FIELDS["exp"](N), MK.thin_mask(N)
        ref = MK.Hierarchy(c, L, 2, sigma, eps, axes, faces, mask)
        _random_problem(ref, np.random.default_rng(1))
        u, d = ref.u[-1].copy(), ref.d[-1].copy()
        _ORDER_REF["case"] = (c, L, N, sigma, axes, faces, eps, mask, ref, u, d, ref.vcycles(2))
    return _ORDER_REF["case"]


@pytest.mark.parametrize("first", SETTERS)
def test_setters_in_every_order(first):
    """shift, coefficient, periodic, Neumann, mask and the coarsening rule in all 720 orders of the six setters (120 per
    case: the orders that begin with `first`), the factor built before the first, between two of them or after the last:
    the same mask bytes on every level, the same u bit for bit, the norms to the summation tolerance"""
    c, L, N, sigma, axes, faces, eps, mask, ref, u, d, want = _order_case()
    setters = {"shift": lambda s: s.set_shift(sigma), "coef": lambda s: s.set_coefficient(eps),
               "periodic": lambda s: s.set_periodic(axes), "neumann": lambda s: s.set_neumann(faces),
               "mask": lambda s: s.set_mask(mask), "rule": lambda s: s.set_mask_coarsening("keep")}
    rest = [n for n in SETTERS if n != first]
    for n_, tail in enumerate(itertools.permutations(rest)):
        order = (first,) + tail
        with M.Solver(c, L, 2) as s:
            at = n_ % 7
            for pos, name in enumerate(order):
                if pos == at:
                    s.get_details()
                setters[name](s)
            if at == 6:
                s.get_details()
            _assert_masks(s, ref.mask, str(order))
            s.upload(MG3D_U, L - 1, u)
            s.upload(MG3D_D, L - 1, d)
            got = s.vcycles(2)
            assert _same_bits(s.download(MG3D_U, L - 1), ref.u[-1]), order
            np.testing.assert_allclose(got, want, rtol=norm_rtol(N))


def test_a_change_of_the_periodic_mask_coarsens_again():
    """under KEEP: a periodic axis set and cleared again, then a Neumann face where the duplicates were -- the finest
    duplicates are rewritten for good (plane N-1 holds plane 0's bytes from then on) and the lower levels are coarsened
    again from the finest one each time"""
    c, L, N, _, _, _, _, mask, _, u, d, _ = _order_case()
    with M.Solver(c, L, 2) as s:
        s.get_details()
        s.set_mask_coarsening("keep")
        s.set_mask(mask)
        _assert_masks(s, MK.keep(mask, L, 0), "Dirichlet")
        s.set_periodic(1)
        kept = MR.stored(mask, 1)
        assert not np.array_equal(kept, mask)
        assert any(not np.array_equal(x, y) for x, y in zip(MK.keep(kept, L, 1)[:-1], MK.keep(mask, L, 0)[:-1]))
        _assert_masks(s, MK.keep(kept, L, 1), "periodic i")
        s.set_periodic(0)
        _assert_masks(s, MK.keep(kept, L, 0), "the axis cleared: plane N-1 holds plane 0's bytes")
        s.set_neumann(2)
        _assert_masks(s, MK.keep(kept, L, 0), "a Neumann face where the duplicates were")
        ref2 = MK.Hierarchy(c, L, 2, 0.0, None, 0, 2, kept)
        ref2.u[-1][...] = u
        ref2.d[-1][...] = d
        ref2.vcycles(2)
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        s.vcycles(2)
        assert _same_bits(s.download(MG3D_U, L - 1), ref2.u[-1])


# ------------------------------------------------------------------------------------------------------------ 2 cycles
@pytest.mark.parametrize("c,L", SHAPES)
@pytest.mark.parametrize("axes,faces", FEW)
@pytest.mark.parametrize("field,sigma", [("const", 0.0), ("eps", 3.5), ("sfield", 0.0)])
def test_cycles(c, L, axes, faces, field, sigma):
    """three mg3d_vcycles under KEEP: u of every level and d below the top bit for bit, the norms to the summation
    tolerance; constant operator, eps with sigma, a screening field"""
    N = _n(c, L)
    eps = CR.FIELDS["exp"](N) if field == "eps" else None
    mask = MK.thin_mask(N)
    sf = None
    if field == "sfield":
        sf = SF.random_field(N, 1.0 / (N - 1))
        ref = MK.FieldHierarchy(c, L, 2, sigma, eps, axes, faces, mask, sf)
    else:
        ref = MK.Hierarchy(c, L, 2, sigma, eps, axes, faces, mask)
    _random_problem(ref, np.random.default_rng(N + faces + 64 * axes), poison=True)
    u_in = ref.u[-1].copy()
    with _solver(c, L, 2, sigma, eps, axes, faces, mask, sfield=sf) as s:
        _upload(s, ref)
        want = ref.vcycles(3)
        got = s.vcycles(3)
        for l in range(L):
            assert _same_bits(s.download(MG3D_U, l), ref.u[l]), f"u level {l}"
        for l in range(L - 1):
            assert _same_bits(s.download(MG3D_D, l), ref.d[l]), f"d level {l}"
        fx = ref.fixed()
        assert _same_bits(s.download(MG3D_U, L - 1).reshape(N, N, N)[fx], u_in[fx])
    np.testing.assert_allclose(got, want, rtol=norm_rtol(N))


def test_cycles_contract_on_the_thin_mask_where_injection_grows():
    """33^3 Dirichlet box, gpu_test_mask held at 1, a random right-hand side (seed 1), ten cycles on the GPU: under KEEP
    norm_10 < norm_4, under injection norm_10 > norm_4 (tests/test_mask_keep_host.py has the same on the restatement:
    0.42 and 1.78 per cycle)"""
    c, L, N = 5, 4, 33
    mask = MR.gpu_test_mask(N)
    u0 = np.zeros((N, N, N))
    u0[mask != 0] = 1.0
    d = np.random.default_rng(1).standard_normal((N, N, N))
    norms = {}
    for rule in ("keep", "inject"):
        with _solver(c, L, 2, 0.0, None, 0, 0, mask, rule=rule) as s:
            s.upload(MG3D_U, L - 1, u0)
            s.upload(MG3D_D, L - 1, d)
            norms[rule] = s.vcycles(10)
            print(rule, (norms[rule][9] / norms[rule][3]) ** (1.0 / 6))
    assert norms["keep"][9] < norms["keep"][3]
    assert norms["inject"][9] > norms["inject"][3]


# ----------------------------------------------------------------------------------------------- 3 solvers and stepper
_exact_b = {}


def _exact_b_run():
    """the restatement's solve of exact problem (b) under KEEP to rtol 1e-12, once"""
    if not _exact_b:
        axes, faces, mask, u0, exact = MR.exact_problem("b")
        prob = MK.Hierarchy(5, 3, 2, 0.0, None, axes, faces, mask)
        hist = []
        _, norms, ok, _, _ = MR.wpcg(prob, u0, np.zeros_like(u0), 1e-12, 0.0, 60, history=hist)
        assert ok
        _exact_b["run"] = (prob, mask, u0, exact, hist, norms)
    return _exact_b["run"]


@pytest.mark.parametrize("call", ["pcg_solve", "wpcg_solve"])
def test_solvers_on_exact_problem_b(call):
    """the plane that injection loses, under KEEP, held as tests/test_gpu_mask.py holds it under injection: u after 1, 2
    and 5 iterations and the norms to that file's tolerances; to rtol 1e-12 the restatement's iteration count and the exact
    discrete solution to 1e-10; the fixed values bitwise"""
    prob, mask, u0, exact, hist, ref_norms = _exact_b_run()
    N = 17
    with _solver(5, 3, 2, 0.0, None, prob.axes, prob.faces, mask) as s:
        s.upload(MG3D_D, 2, np.zeros(N ** 3))
        for k in (1, 2, 5):
            s.upload(MG3D_U, 2, u0)
            norms, info = getattr(s, call)(rtol=0.0, atol=1e-300, max_iters=k)
            u = s.download(MG3D_U, 2).reshape(N, N, N)
            rel = np.abs(u - hist[k - 1]).max() / np.abs(hist[k - 1]).max()
            nrel = (np.abs(norms - ref_norms[:k + 1]) / ref_norms[:k + 1]).max()
            print(call, k, "u", rel, "norms", nrel)
            assert info["iterations"] == k
            su, sn = TM.SPREAD[call]
            assert rel <= 100 * su[k] and nrel <= 100 * max(sn, TM.SPREAD_NORM_EXACT_B)
        s.upload(MG3D_U, 2, u0)
        norms, info = getattr(s, call)(rtol=1e-12, max_iters=60)
        assert info["converged"] and info["iterations"] == len(ref_norms) - 1
        if call == "wpcg_solve":
            assert info["singular"] == 0
        u = s.download(MG3D_U, 2).reshape(N, N, N)
        err = np.abs(u - exact).max()
        print(call, "iterations", info["iterations"], "max error", err)
        assert err <= 1e-10
        assert _same_bits(u[mask != 0], u0[mask != 0])
        w = u.copy()
        NR.refresh(w, prob.axes)
        assert _same_bits(u, w), "duplicates differ from their sources"


@pytest.mark.parametrize("call", ["pcg_solve", "wpcg_solve"])
def test_solvers_on_the_plate(call):
    """a one-point plate on an odd plane held at 1 in a grounded 33^3 box, as tests/test_gpu_mask.py holds the sphere"""
    c, L, N = 5, 4, 33
    mask = MR.plate(N, (N // 2) | 1)
    prob = MK.Hierarchy(c, L, 2, 0.0, None, 0, 0, mask)
    u0 = np.zeros((N, N, N))
    u0[mask != 0] = 1.0
    hist = []
    x, ref_norms, ok, _, _ = MR.wpcg(prob, u0, np.zeros_like(u0), 1e-10, 0.0, 60, history=hist)
    assert ok and len(hist) >= 5
    with _solver(c, L, 2, 0.0, None, 0, 0, mask) as s:
        s.upload(MG3D_D, L - 1, np.zeros(N ** 3))
        for k in (1, 2, 5):
            s.upload(MG3D_U, L - 1, u0)
            norms, info = getattr(s, call)(rtol=0.0, atol=1e-300, max_iters=k)
            u = s.download(MG3D_U, L - 1).reshape(N, N, N)
            rel = np.abs(u - hist[k - 1]).max() / np.abs(hist[k - 1]).max()
            nrel = (np.abs(norms - ref_norms[:k + 1]) / ref_norms[:k + 1]).max()
            print(call, k, "u", rel, "norms", nrel)
            assert rel <= 100 * TM.SPREAD[call][0][k] and nrel <= 100 * TM.SPREAD[call][1]
        s.upload(MG3D_U, L - 1, u0)
        norms, info = getattr(s, call)(rtol=1e-10, max_iters=60)
        assert info["converged"] and info["iterations"] == len(ref_norms) - 1
        u = s.download(MG3D_U, L - 1).reshape(N, N, N)
        assert _same_bits(u[mask != 0], u0[mask != 0])
        assert 0.0 <= u.min() and u.max() <= 1.0  # the discrete maximum principle


def test_keep_lifts_the_pin_of_the_neumann_box():
    """all six faces Neumann, sigma = 0, one fixed point at odd indices: under injection it is gone from level 0 and the
    pin stays; under KEEP it reaches level 0 and the pin goes -- the same counts, read by the same rule"""
    c, L, N = 5, 3, 17
    point = (5, 7, 9)
    mask = np.zeros((N, N, N), dtype=np.uint8)
    mask[point] = 1
    rng = np.random.default_rng(2)
    d = rng.standard_normal((N, N, N))
    u0 = np.zeros((N, N, N))
    u0[point] = 0.75
    assert MR.pinned(0, 63, 0.0, MR.inject(mask, L)[0]) and not MR.pinned(0, 63, 0.0, MK.keep(mask, L)[0])
    prob = MK.Hierarchy(c, L, 2, 0.0, None, 0, 63, mask)
    x, ref_norms, ok, _, _ = MR.wpcg(prob, u0, d, 1e-8, 0.0, 60)
    assert ok
    with _solver(c, L, 2, 0.0, None, 0, 63, mask) as s:
        assert s.get_mask(0)[1, 1, 2] == 1
        s.upload(MG3D_U, L - 1, u0)
        s.upload(MG3D_D, L - 1, d)
        norms, info = s.wpcg_solve(rtol=1e-8, max_iters=60)
        assert info["singular"] == 0 and info["converged"] and info["iterations"] == len(ref_norms) - 1
        u = s.download(MG3D_U, L - 1).reshape(N, N, N)
        assert u[point] == 0.75
        assert np.abs(u - x).max() <= 1e-6 * np.abs(x).max()


@pytest.mark.parametrize("method", ["vcycles", "wpcg"])
def test_step_advance(method):
    """three Crank-Nicolson steps at 17^3 with the thin mask (a source, periodic k + Neumann i faces), as
    tests/test_gpu_mask.py steps its block: u at the fixed points bitwise constant, u elsewhere against _step_ref driven
    by the KEEP hierarchy"""
    c, L, N = 5, 3, 17
    axes, faces, dt, theta, kappa = 4, 3, 1e-3, 0.5, 2.0
    mask = MK.thin_mask(N)
    rng = np.random.default_rng(17)
    u0, src = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    u0[mask != 0] = 2.5
    NR.refresh(u0, axes)
    prob = MK.Hierarchy(c, L, 2, SR.sigma_of(dt, theta, kappa), None, axes, faces, mask)
    prob.u[-1][...] = u0
    cycles = 2 if method == "vcycles" else 1
    want_n, _, _ = MR.advance(prob, 3, cycles, src, dt, theta, kappa, method=method, rtol=0.0)
    with M.Solver(c, L, 2) as s:
        s.set_periodic(axes)
        s.set_neumann(faces)
        s.set_mask(mask)
        s.step_setup(dt, theta, kappa)
        s.get_details()
        s.set_mask_coarsening("keep")  # (behind the factor: it is rebuilt)
        s.step_set_source(src)
        s.upload(MG3D_U, L - 1, u0)
        norms, info = s.step_advance(3, cycles=cycles, method=method, rtol=0.0)
        assert info["steps"] == 3
        u = s.download(MG3D_U, L - 1).reshape(N, N, N)
    fx = prob.fixed()
    assert _same_bits(u[fx], u0[fx])
    if method == "vcycles":
        assert _same_bits(u, prob.u[-1])
        np.testing.assert_allclose(norms, want_n, rtol=norm_rtol(N))
    else:
        rel = np.abs(u - prob.u[-1]).max() / np.abs(prob.u[-1]).max()
        nrel = (np.abs(norms - want_n) / want_n).max()
        print("step wpcg: u", rel, "norms", nrel)
        assert rel <= 100 * TW.SPREAD_U[5] and nrel <= 100 * TW.SPREAD_NORM


# -------------------------------------------------------------------------------------------- 4 the default is untouched
@pytest.mark.parametrize("axes,faces", FEW)
def test_inject_is_unchanged(axes, faces):
    """a context that never heard of the call, one that set INJECT explicitly and one that went KEEP -> INJECT (with a
    built factor and cycles under KEEP in between): masks, u of every level and norms agree bit for bit, and with the
    restatement of the injected hierarchy"""
    c, L, N = 5, 4, 33
    eps, mask = CR.FIELDS["exp"](N), MK.thin_mask(N)
    ref = MR.Hierarchy(c, L, 2, 1.5, eps, axes, faces, mask)
    _random_problem(ref, np.random.default_rng(5))
    with _solver(c, L, 2, 1.5, eps, axes, faces, mask, rule=None) as a, \
            _solver(c, L, 2, 1.5, eps, axes, faces, mask, rule="inject") as b, \
            _solver(c, L, 2, 1.5, eps, axes, faces, mask, rule="keep") as k:
        _upload(k, ref)
        k.vcycles(2)
        k.vcycle()
        k.set_mask_coarsening("inject")
        out = []
        for s in (a, b, k):
            assert s.get_mask_coarsening() == "inject"
            _upload(s, ref)
            n = [s.vcycle()] + list(s.vcycles(2))
            out.append((n, [s.download(MG3D_U, l) for l in range(L)], [s.get_mask(l) for l in range(L)]))
        for n, u, m in out[1:]:
            assert np.array_equal(np.array(n), np.array(out[0][0]))
            for l in range(L):
                assert _same_bits(u[l], out[0][1][l]) and np.array_equal(m[l], out[0][2][l])
        ref.vcycles(3)
        assert _same_bits(out[0][1][L - 1], ref.u[-1])
        for l in range(L):
            assert np.array_equal(out[0][2][l], ref.mask[l])


# ----------------------------------------------------------------------------------------------------------- 5 full multigrid
@pytest.mark.parametrize("c,L", SHAPES)
@pytest.mark.parametrize("axes,faces", BOUNDARIES)
def test_fmg(c, L, axes, faces):
    """mg3d_fmg_solve(1) and (2) under KEEP: the finest-level u of the restatement bit for bit, the norm to the summation
    tolerance, u at the fixed and Dirichlet points and d of the finest level the caller's bits -- d at the fixed points
    poisoned with NaN beforehand; mg3d_fmg_interpolate alone on every level.  The constant operator; eps with sigma on
    the combinations of tests/test_gpu_mask.py"""
    N = _n(c, L)
    mask = MK.thin_mask(N)
    fields = [("const", 0.0)] + ([("eps", 3.5)] if (axes, faces) in FEW else [])
    for field, sigma in fields:
        eps = CR.FIELDS["exp"](N) if field == "eps" else None
        ref = MK.Hierarchy(c, L, 2, sigma, eps, axes, faces, mask)
        rng = np.random.default_rng(N + faces + 64 * axes)
        _random_problem(ref, rng, poison=True)
        u_in, d_in = ref.u[-1].copy(), ref.d[-1].copy()
        held = MR._keep(ref.mask[-1], axes, faces) | MK.FR.dirichlet_mask(N, axes, faces)
        assert ref.fixed().any() and np.isnan(d_in).any()
        with _solver(c, L, 2, sigma, eps, axes, faces, mask) as s:
            for cycles in (1, 2):
                ref.u[-1][...] = u_in
                ref.d[-1][...] = d_in
                _upload(s, ref)
                want = MK.fmg_solve(ref, cycles)
                got = s.fmg_solve(cycles)
                u = s.download(MG3D_U, L - 1).reshape(N, N, N)
                assert np.isfinite(u).all()
                assert _same_bits(u, ref.u[-1]), (field, cycles)
                assert _same_bits(u[held], u_in[held])
                assert _same_bits(s.download(MG3D_D, L - 1), d_in)
                assert abs(got - want) <= norm_rtol(N) * want, (got, want)
            for l in range(1, L):
                n, nc = s.level_n(l), s.level_n(l - 1)
                ref.u[l][...] = rng.standard_normal((n, n, n))
                ref.u[l - 1][...] = rng.standard_normal((nc, nc, nc))
                NR.refresh(ref.u[l], axes)
                NR.refresh(ref.u[l - 1], axes)
                before = ref.u[l].copy()
                s.upload(MG3D_U, l, ref.u[l])
                s.upload(MG3D_U, l - 1, ref.u[l - 1])
                s.fmg_interpolate(l)
                MK.interpolate(ref, l)
                got_u = s.download(MG3D_U, l).reshape(n, n, n)
                assert _same_bits(got_u, ref.u[l]), f"interpolate, level {l}"
                fx = ref.fixed(l)
                assert fx.any() and _same_bits(got_u[fx], before[fx])


@pytest.mark.parametrize("axes,faces", [(0, 0), (2, 1 | 2 | 16)])
def test_fmg_at_65(axes, faces):
    """65^3 (c = 5, L = 5): rows past one block of 64 lanes in the masked restriction, injection and interpolation"""
    c, L, N = 5, 5, 65
    mask = MK.thin_mask(N)
    for p in itertools.product((61, 63), (1, 63), (62, 63, 64)):
        mask[p] = 8
    ref = MK.Hierarchy(c, L, 2, 0.0, None, axes, faces, mask)
    _random_problem(ref, np.random.default_rng(N + axes), poison=True)
    u_in, d_in = ref.u[-1].copy(), ref.d[-1].copy()
    with _solver(c, L, 2, 0.0, None, axes, faces, mask) as s:
        _upload(s, ref)
        want = MK.fmg_solve(ref, 1)
        got = s.fmg_solve(1)
        u = s.download(MG3D_U, L - 1).reshape(N, N, N)
        assert _same_bits(u, ref.u[-1])
        assert _same_bits(u[ref.fixed()], u_in[ref.fixed()])
        assert _same_bits(s.download(MG3D_D, L - 1), d_in)
        assert abs(got - want) <= norm_rtol(N) * want


def test_fmg_on_one_level():
    """L = 1: the direct solve with u's own values at the fixed unknowns and the Dirichlet points; d stays"""
    c = 9
    mask = MK.thin_mask(c)
    rng = np.random.default_rng(8)
    for axes, faces, sigma in ((0, 0, 0.0), (4, 3, 3.5)):
        ref = MK.Hierarchy(c, 1, 2, sigma, None, axes, faces, mask)
        _random_problem(ref, rng, poison=True)
        d_in = ref.d[0].copy()
        with _solver(c, 1, 2, sigma, None, axes, faces, mask) as s:
            _upload(s, ref)
            assert s.fmg_solve(1) == 0.0 and MK.fmg_solve(ref, 1) == 0.0
            assert _same_bits(s.download(MG3D_U, 0), ref.u[0])
            assert _same_bits(s.download(MG3D_D, 0), d_in)


def test_fmg_beats_one_cycle_on_the_plate():
    """the plate held at 1 in a grounded 33^3 box, d = 0: the residual norm after fmg_solve(1) under KEEP against ONE
    plain KEEP cycle from the zero guess.  The restatement has 1.59e3 against 6.56e3 (tests/test_mask_keep_host.py)"""
    c, L, N = 5, 4, 33
    mask = MR.plate(N, (N // 2) | 1)
    u0 = np.zeros((N, N, N))
    u0[mask != 0] = 1.0
    with _solver(c, L, 2, 0.0, None, 0, 0, mask) as s:
        s.upload(MG3D_D, L - 1, np.zeros(N ** 3))
        s.upload(MG3D_U, L - 1, u0)
        fmg = s.fmg_solve(1)
        s.upload(MG3D_U, L - 1, u0)
        one = s.vcycles(1)[0]
    print("fmg_solve(1)", fmg, "one cycle", one)
    assert fmg < one


# ------------------------------------------------------------------------------------------------------------ 6 refusals
def test_fmg_under_inject_is_refused_and_a_bad_rule_changes_nothing():
    c, L, N = 5, 3, 17
    mask = MK.thin_mask(N)
    rng = np.random.default_rng(4)
    u = rng.standard_normal(N ** 3)
    with M.Solver(c, L, 2) as s:
        s.set_mask(mask)
        s.get_details()
        s.upload(MG3D_U, L - 1, u)
        for rule in ("inject", None):
            if rule:
                s.set_mask_coarsening(rule)
            for call in (lambda: s.fmg_solve(1), lambda: s.fmg_interpolate(L - 1)):
                with pytest.raises(M.Mg3dError) as ei:
                    call()
                assert ei.value.code == MG3D_ERR_STATE and "mg3d_ctx_set_mask_coarsening" in str(ei.value)
        before = [s.get_mask(l) for l in range(L)]
        for bad in (2, -1, 7):
            with pytest.raises(M.Mg3dError) as ei:
                s.set_mask_coarsening(bad)
            assert ei.value.code == MG3D_ERR_ARG
        with pytest.raises(ValueError):
            s.set_mask_coarsening("both")
        assert s.L.mg3d_ctx_set_mask_coarsening(None, 1) == MG3D_ERR_ARG
        assert s.L.mg3d_ctx_get_mask_coarsening(s._h, None) == MG3D_ERR_ARG
        assert s.get_mask_coarsening() == "inject"
        for l in range(L):
            assert np.array_equal(s.get_mask(l), before[l])
        assert _same_bits(s.download(MG3D_U, L - 1), u)
        s.vcycles(1)  # the factor is still there
        s.set_mask_coarsening("keep")
        for call in (lambda: s.es_setup(), lambda: s.fmg_initialize()):  # these keep refusing a mask
            with pytest.raises(M.Mg3dError) as ei:
                call()
            assert ei.value.code == MG3D_ERR_STATE
        s.fmg_solve(1)
