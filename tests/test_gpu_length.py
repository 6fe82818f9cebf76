"""Every solver path on boxes other than the unit cube (grid_length 3e-4, the electrospray's own, and 3.0: h^2 > h, nothing
dyadic).  Operators, sizes, data and the scaling identity: tests/_length_cases.py; tests/test_length_host.py shows the
identity on every restatement used here.

B  every feature against its restatement called with this length's h = grid_length / (N - 1), at 17^3 = (5, 3), 33^3 =
   (5, 4) and 37^3 = (10, 3), over a pruned matrix in which every operator meets both lengths: the single operators, cycles,
   mg3d_fmg_solve, mg3d_step_advance, the field output and the fp32 variant bit for bit, sums at the project's summation
   tolerance 1e-13 against the exactly rounded sum (fp32 norms: the 1e-12 of tests/test_gpu_f32_random.py).  The analytic
   boundary paths are held to orc_fill_boundary and _screened_ref's setup_test_problem / fmg_initialize(grid_length);
   orc_run_problem itself has no length argument (GRID_LENGTH = 1 of the reference), its restatement _screened_ref.Problem
   has.  d is random in (-50, 50) / length^2, so that hSq*d weighs against the neighbour sum as on the unit cube.

   mg3d_pcg_solve / mg3d_wpcg_solve, three iterations: the restatement's cycles are the library's bit for bit, only the
   sums differ in order.  What an order is worth at THESE lengths and data was measured on the CPU (python
   tests/_length_cases.py: two restatement runs, exactly rounded sums against numpy's pairwise float64 sums, largest over
   the operators, the three sizes and both lengths), as max|a - b| / max|a| of the iterate x_k and of the norms:
       pcg   k = 1: 5.13e-14   k = 2: 1.83e-14   k = 3: 7.23e-14   norms: 6.71e-11
       wpcg  k = 1: 7.41e-15   k = 2: 2.26e-12   k = 3: 2.30e-12   norms: 1.68e-13
   The GPU, a third order, is allowed 100 times the figure, as in tests/test_gpu_pcg.py and tests/test_gpu_wpcg.py.

C  the scaling identity between GPU runs, where the fused and distributed paths live: grid_length times 2^m (m = 2, -3),
   d, sigma, kappa, source over 4^m, dt times 4^m -- u of every level the same bits, d below the top and every norm exactly
   4^-m times, PCG iterates and counts the same, the gradient 2^-m times, flux and energy 2^m times (include/mg3d.h:
   *flux = h * sum, *energy = 0.5 * h * sum, the sums of unscaled terms).  No CPU reference of the cycle is needed; the
   unit-length runs at these shapes are pinned to the oracle by tests/test_gpu_legs.py, tests/test_gpu_parity.py and
   tests/test_gpu_screened_variants.py (the bases at 3e-4 by the identity from them).  The identity cannot see a spacing
   that is wrong by the same factor in both runs (another level's h): the base run's coarsest level is therefore solved
   again on the CPU with the factor of the coarsest spacing, 2^(L-1) * grid_length / (N - 1), and the gradient is
   compared with _field_ref.gradient.

The features merged after this file have siblings of their own, with these lengths, data and tolerances:
   tests/test_gpu_length_fields.py    the screening field (mg3d_ctx_set_shift_field), the KEEP coarsening rule and masked
                                      full multigrid, PCG / WPCG over both: parts B and C; its identity runs are pinned
                                      by its own part B at the smaller sizes
   tests/test_gpu_particle_length.py  sample, deposit, push, sort and permute at 21, 37, 41 and 65 points per side, where a
                                      coordinate i*h locates in cell i - 1; its identity runs at 41^3 are pinned to the
                                      restatements in the same test
   tests/test_particle_length_host.py the coverage of those particle cases and the identity on their restatements"""
import numpy as np
import pytest
import torch  # noqa: F401  (before the package, as bench.py does: the HIP runtime is torch's)

import _f32_ref as F32
import _field_ref as FR
import _fmg_ref as FM
import _length_cases as LC
import _mask_ref as MR
import _neumann_ref as NR
import _oracle as O
import _screened_ref as S
import _step_ref as SR
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U, check
from test_field_ref_host import slab_problem

pytestmark = pytest.mark.gpu

SUM_RTOL = 1e-13   # the project's summation tolerance: a device reduction against the exactly rounded sum
NORM_RTOL = 1e-13  # tests/test_gpu_step.py, tests/test_gpu_fmg.py: a device norm against the restatement's
F32_NORM_RTOL = 1e-12  # tests/test_gpu_f32_random.py
# measured, see above: {k: spread of x_k}, spread of the norms
SPREAD = {"pcg_solve": ({1: 5.13e-14, 2: 1.83e-14, 3: 7.23e-14}, 6.71e-11),
          "wpcg_solve": ({1: 7.41e-15, 2: 2.26e-12, 3: 2.30e-12}, 1.68e-13)}
DT, KAPPA = 0.01, 0.75  # times / over length^2
GRAD_SCALES = LC.GRAD_SCALES
same_bits = LC.same_bits


def _pruned(names, sizes=(17, 33, 37)):
    """(operator, N, length): every operator meets both lengths, the sizes rotate (no periodic axis at 37^3: c - 1 odd)"""
    out = []
    for i, name in enumerate(names):
        for j, length in enumerate(LC.LENGTHS):
            ok = [n for n in sizes if not (n == 37 and name in LC.PERIODIC)]
            out.append(pytest.param(name, ok[(i + j) % len(ok)], length, id=f"{name}-{ok[(i + j) % len(ok)]}-{length:g}"))
    return out


ALL = tuple(LC.OPERATORS)
NO_MASK = tuple(n for n in ALL if not LC.OPERATORS[n][4])


def _assert_spacings(s, c, L, length):
    """.h is grid_length / (N - 1) bit for bit, level_h doubles exactly down the levels, level_n is the level's side --
    as far as the class reports them (Solver: all three; DistSolver: .h and level_n; the fp32 classes: level_n)"""
    N = LC.n_of(c, L)
    assert s.N == N
    if hasattr(s, "h"):
        assert s.h == length / (N - 1), (s.h, length / (N - 1))
    for l in range(L):
        assert s.level_n(l) == (c - 1) * (1 << l) + 1
        if hasattr(s, "level_h"):
            assert s.level_h(l) == (length / (N - 1)) * (1 << (L - 1 - l)), l
            if l:
                assert s.level_h(l - 1) == 2.0 * s.level_h(l)


def _solver(name, c, L, nu, length, sigma=None, factor=True):
    sg, eps, axes, faces, mask = LC.operator(name, LC.n_of(c, L))
    s = M.Solver(c, L, nu, grid_length=length)
    _assert_spacings(s, c, L, length)
    s.set_shift(sg if sigma is None else sigma)
    s.set_periodic(axes)
    s.set_neumann(faces)
    if eps is not None:
        s.set_coefficient(eps)
    if mask is not None:
        s.set_mask(mask)
    if factor:
        s.get_details()
    return s


def _mask_of(ref, l):
    return ref.mask[l] if hasattr(ref, "mask") else np.zeros((ref.N[l],) * 3, dtype=np.uint8)


def _assert_levels(s, ref, what=""):
    for l in range(ref.L):
        assert same_bits(s.download(MG3D_U, l), ref.flat("u", l)), f"{what} u level {l}"
    for l in range(ref.L - 1):
        assert same_bits(s.download(MG3D_D, l), ref.flat("d", l)), f"{what} d level {l}"


# ================================================================================================================ B
@pytest.mark.parametrize("length", LC.LENGTHS)
@pytest.mark.parametrize("c,L", sorted(LC.SIZES.values()) + [(9, 5), (11, 5)])
def test_reported_spacings(c, L, length):
    """every solver class (the slab classes from 33^3 on: two ranks need a level with 8 planes each)"""
    with M.Solver(c, L, 2, grid_length=length) as s:
        _assert_spacings(s, c, L, length)
    with M.Solver32(c, L, 2, grid_length=length) as s32:
        _assert_spacings(s32, c, L, length)
    if LC.n_of(c, L) < 33:
        return
    with M.DistSolver(c, L, 2, nranks=2, grid_length=length) as d:
        _assert_spacings(d, c, L, length)
    with M.DistSolver32(c, L, 2, nranks=2, grid_length=length) as d32:
        _assert_spacings(d32, c, L, length)


@pytest.mark.parametrize("name,N,length", _pruned(ALL))
def test_single_operators(name, N, length):
    """smooth (pre, post), residual (stored r and norm), restrict, prolong on the two finest levels, coarse_solve, on
    random data, with the restatement's own h of each level"""
    c, L = LC.SIZES[N]
    ref = LC.reference(name, c, L, 2, length)
    sigma, axes, faces = ref.sigma, ref.axes, ref.faces
    rng = np.random.default_rng(N + 7 * len(name))
    dscale = 50.0 / (length * length)
    with _solver(name, c, L, 2, length) as s:
        for l in (L - 1, L - 2):
            n, h, e, m = ref.N[l], ref.level_h(l), ref.e(l), _mask_of(ref, l)
            u, d = rng.uniform(-1, 1, (n, n, n)), rng.uniform(-1, 1, (n, n, n)) * dscale
            NR.refresh(u, axes)
            s.upload(MG3D_U, l, u)
            s.upload(MG3D_D, l, d)
            s.smooth(l, 0, 2)
            MR.pre_smooth(u, d, e, h, sigma, axes, faces, 2, m)
            assert same_bits(s.download(MG3D_U, l).reshape(n, n, n), u), f"pre-smoothing, level {l}"
            s.smooth(l, 1, 1)
            MR.post_smooth(u, d, e, h, sigma, axes, faces, 1, m)
            assert same_bits(s.download(MG3D_U, l).reshape(n, n, n), u), f"post-smoothing, level {l}"
            r = rng.uniform(-1, 1, (n, n, n))
            s.upload(MG3D_R, l, r)
            got = s.residual(l, store=True)
            MR.residual(u, d, e, h, sigma, axes, faces, m, r)
            assert same_bits(s.download(MG3D_R, l).reshape(n, n, n), r), f"residual, level {l}"
            exact = MR.exact_residual_norm(u, d, e, h, sigma, axes, faces, m)
            print(name, N, length, l, "norm", got, exact, abs(got - exact) / exact)
            assert abs(got - exact) <= SUM_RTOL * exact
            nc = ref.N[l - 1]
            dc = rng.uniform(-1, 1, (nc, nc, nc))
            s.upload(MG3D_D, l - 1, dc)
            s.restrict(l)
            NR.restrict(r, dc, axes, faces)
            assert same_bits(s.download(MG3D_D, l - 1).reshape(nc, nc, nc), dc), f"restrict, level {l}"
            ec = rng.uniform(-1, 1, (nc, nc, nc))
            NR.refresh(ec, axes)
            s.upload(MG3D_U, l - 1, ec)
            s.prolong(l)
            MR.prolong(ec, u, axes, faces, m)
            assert same_bits(s.download(MG3D_U, l).reshape(n, n, n), u), f"prolong, level {l}"
        d0 = rng.uniform(-1, 1, (c, c, c)) * dscale
        s.upload(MG3D_D, 0, d0)
        s.coarse_solve()
        u0 = np.zeros((c, c, c))
        MR.coarse_solve(ref.LU, d0, u0, axes, faces, sigma, _mask_of(ref, 0))
        assert same_bits(s.download(MG3D_U, 0).reshape(c, c, c), u0), "coarse_solve"


@pytest.mark.parametrize("name,N,length", _pruned(ALL))
def test_cycles(name, N, length):
    """vcycles(1), vcycles(2), vcycles(3): u of every level and d below the top bit for bit after each call"""
    c, L = LC.SIZES[N]
    ref = LC.reference(name, c, L, 2, length)
    u, d = LC.data(name, N, length, N)
    ref.u[-1][...] = u
    ref.d[-1][...] = d
    with _solver(name, c, L, 2, length) as s:
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        for k in (1, 2, 3):
            got = s.vcycles(k)
            want = ref.vcycles(k)
            _assert_levels(s, ref, f"after the call of {k}:")
            print(name, N, length, k, got, np.abs(got - want) / want)
            np.testing.assert_allclose(got, want, rtol=NORM_RTOL)
        exact = MR.exact_residual_norm(ref.u[-1], ref.d[-1], ref.e(L - 1), ref.h, ref.sigma, ref.axes, ref.faces, _mask_of(ref, L - 1))
        assert abs(got[-1] - exact) <= SUM_RTOL * exact


@pytest.mark.parametrize("name,N,length", _pruned(NO_MASK))
def test_fmg_solve(name, N, length):
    c, L = LC.SIZES[N]
    ref = LC.reference(name, c, L, 2, length)
    u, d = LC.data(name, N, length, N + 1)
    ref.u[-1][...] = u
    ref.d[-1][...] = d
    want = FM.fmg_solve(ref, 2)
    with _solver(name, c, L, 2, length) as s:
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        got = s.fmg_solve(2)
        assert same_bits(s.download(MG3D_U, L - 1), ref.flat("u", L - 1))
        assert same_bits(s.download(MG3D_D, L - 1), d.reshape(-1))
    print(name, N, length, got, want)
    assert got == pytest.approx(want, rel=NORM_RTOL)


@pytest.mark.parametrize("name,N,length", _pruned(ALL, sizes=(17, 33)))
def test_step_advance(name, N, length):
    """two steps of two V-cycles, theta 1 and 0.5, with and without a source; dt = 0.01 length^2, kappa = 0.75 / length^2"""
    c, L = LC.SIZES[N]
    dt, kappa = DT * length * length, KAPPA / (length * length)
    u0, src = LC.data(name, N, length, N + 2)
    with _solver(name, c, L, 2, length) as s:
        for theta in (1.0, 0.5):
            for with_src in (True, False):
                sv = src if with_src else None
                ref = LC.reference(name, c, L, 2, length, sigma=SR.sigma_of(dt, theta, kappa))
                ref.u[-1][...] = u0
                adv = MR.advance if hasattr(ref, "mask") else SR.advance
                want_n, _, _ = adv(ref, 2, 2, sv, dt, theta, kappa)
                s.step_setup(dt, theta, kappa)
                assert s.get_shift() == ref.sigma
                s.step_set_source(sv)
                s.upload(MG3D_U, L - 1, u0)
                s.zero(MG3D_D, L - 1)
                norms, info = s.step_advance(2, cycles=2)
                assert info["steps"] == 2 and info["time"] == 2 * dt
                what = (name, N, length, theta, with_src)
                assert same_bits(s.download(MG3D_U, L - 1), ref.flat("u", L - 1)), what
                blk = NR.block(N, ref.axes, ref.faces)
                free = ~ref.fixed()[blk] if hasattr(ref, "mask") else np.ones(ref.d[-1][blk].shape, dtype=bool)
                got_d = s.download(MG3D_D, L - 1).reshape(N, N, N)[blk]
                assert same_bits(got_d[free], ref.d[-1][blk][free]), what  # (d at a fixed point: unspecified)
                print(*what, norms, np.abs(norms - want_n) / want_n)
                np.testing.assert_allclose(norms, want_n, rtol=NORM_RTOL)


def _krylov_cases(names):
    return _pruned(names)


@pytest.mark.parametrize("call,name,N,length",
                         [pytest.param("pcg_solve", *p.values, id="pcg-" + p.id) for p in _krylov_cases(LC.PCG_OPERATORS)]
                         + [pytest.param("wpcg_solve", *p.values, id="wpcg-" + p.id) for p in _krylov_cases(LC.WPCG_OPERATORS)])
def test_krylov(call, name, N, length):
    """x_k and the norms r_0 .. r_k for k = 1, 2, 3 against the restatement with exactly rounded sums: 100 x the spread
    measured on the CPU at these lengths (the docstring of this file)"""
    c, L = LC.SIZES[N]
    x0, d = LC.krylov_data(name, N, length)
    hist, ref_norms = LC.krylov(name, c, L, length, x0, d, LC.PCG_ITERS, "exact", call == "wpcg_solve")
    su, sn = SPREAD[call]
    with _solver(name, c, L, 2, length) as s:
        s.upload(MG3D_D, L - 1, d)
        for k in (1, 2, 3):
            s.upload(MG3D_U, L - 1, x0)
            norms, info = getattr(s, call)(rtol=0.0, atol=1e-300, max_iters=k)
            assert info["iterations"] == k and len(norms) == k + 1
            u = s.download(MG3D_U, L - 1).reshape(N, N, N)
            rel = np.abs(u - hist[k - 1]).max() / np.abs(hist[k - 1]).max()
            nrel = (np.abs(norms - ref_norms[:k + 1]) / ref_norms[:k + 1]).max()
            print(call, name, N, length, k, "u", rel, "norms", nrel)
            assert rel <= 100 * su[k], (k, rel)
            assert nrel <= 100 * sn, (k, nrel)


@pytest.mark.parametrize("length", LC.LENGTHS)
@pytest.mark.parametrize("c,L", sorted(LC.SIZES.values()))
def test_analytic_boundary_paths(c, L, length):
    """setup_test_problem, fill_boundary of every level and fmg_initialize read the coordinates x = i*h: against
    orc_fill_boundary with the level's h and _screened_ref's setup_test_problem / fmg_initialize(grid_length), then two
    cycles -- the constant operator and two shifts"""
    N = LC.n_of(c, L)
    for sigma in (0.0, 3.5, 25.0 / (length * length)):
        ref = S.Problem(c, L, 2, sigma, length)
        ref.setup_test_problem()
        with M.Solver(c, L, 2, grid_length=length) as s:
            _assert_spacings(s, c, L, length)
            s.set_shift(sigma)
            s.setup_test_problem()
            for f, name in ((MG3D_U, "u"), (MG3D_D, "d")):
                assert same_bits(s.download(f, L - 1), ref.flat(name, L - 1)), (sigma, name)
            for l in range(L):
                n = ref.N[l]
                want = np.full(n ** 3, 0.25)
                O.lib().orc_fill_boundary(O.P(want), n, (length / (N - 1)) * (1 << (L - 1 - l)))
                s.upload(MG3D_R, l, np.full(n ** 3, 0.25))
                s.fill_boundary(MG3D_R, l)
                assert same_bits(s.download(MG3D_R, l), want), (sigma, "fill_boundary", l)
                s.zero(MG3D_R, l)  # (the restriction injects the faces of r)
            ref.fmg_initialize(length)
            s.fmg_initialize()
            for l in range(L):
                assert same_bits(s.download(MG3D_U, l), ref.flat("u", l)), (sigma, "fmg_initialize", l)
            got, want = s.vcycles(2), ref.vcycles(2)
            _assert_levels(s, ref, f"sigma {sigma}:")
            np.testing.assert_allclose(got, want, rtol=NORM_RTOL)


def _labelled_mask(N):
    """a ball (label 1) and a plate on plane N // 4 outside it (label 2)"""
    m = MR.sphere(N).astype(np.uint8)
    m[(MR.plate(N, N // 4) != 0) & (m == 0)] = 2
    return m


def _check_sums(s, u, eps, mask, h, axes, faces):
    for label in (0, 1, 2):
        t = FR.flux_terms(u, eps, mask, axes, faces, label)
        want, scale = h * FR.fsum(t), h * FR.fsum(np.abs(t))
        got = s.field_flux(label)
        print("flux", label, got, want, abs(got - want) / scale)
        assert t.size and abs(got - want) <= SUM_RTOL * scale, (label, got, want)
    want = FR.energy(u, eps, h, axes, faces)
    got = s.field_energy()
    print("energy", got, want, abs(got - want) / want)
    assert want > 0 and abs(got - want) <= SUM_RTOL * want


@pytest.mark.parametrize("name,N,length", _pruned(ALL))
def test_field_output(name, N, length):
    """the gradient (host and device form) bit for bit at three scales, flux (a labelled mask on top of every operator) and energy at the
    summation tolerance, from a random u"""
    c, L = LC.SIZES[N]
    _, eps, axes, faces, _ = LC.operator(name, N)
    h = length / (N - 1)
    u = np.random.default_rng(N + 3).uniform(-1, 1, (N, N, N))
    mask = _labelled_mask(N)
    with _solver(name, c, L, 2, length, factor=False) as s:
        assert s.h == h
        s.set_mask(mask)
        s.upload(MG3D_U, L - 1, u)
        for scale in GRAD_SCALES:
            got, want = s.gradient(scale), FR.gradient(u, h, axes, faces, scale)
            dev = s.gradient_tensor(scale=scale).cpu().numpy()  # the device form: one launch for the three components
            for a in range(3):
                assert same_bits(got[a], want[a]) and same_bits(dev[a], want[a]), (scale, a)
        _check_sums(s, u, eps, mask, h, axes, faces)


def test_slab_problem_on_a_box_of_side_three():
    """tests/test_field_ref_host.slab_problem at grid_length 3 (values derived from the header in
    tests/test_length_host.py): F = -4 through the body with label 3, W = 2, W = -1/2 V F with V = 1"""
    axes, faces, _, u, mask = slab_problem()
    with M.Solver(5, 3, 2, grid_length=3.0) as s:
        assert s.h == 3.0 / 16
        s.set_periodic(axes)
        s.set_mask(mask)
        s.upload(MG3D_U, 2, u)
        F, W, F0 = s.field_flux(3), s.field_energy(), s.field_flux(0)
    print(F, W)
    assert abs(F + 4.0) <= SUM_RTOL * 4.0 and abs(W - 2.0) <= SUM_RTOL * 2.0 and F0 == F
    assert abs(W + 0.5 * F) <= SUM_RTOL * 2.0


def _f32_start(c, L, length, seed=7):
    u0, d0, r0 = F32.random_start(c, L, seed)
    scale = np.float32(50.0 / (length * length))
    return u0, (d0 * scale).astype(np.float32), (r0 * scale).astype(np.float32)


@pytest.mark.parametrize("length", LC.LENGTHS)
@pytest.mark.parametrize("c,L", [(5, 4), (10, 3)])
def test_f32(c, L, length):
    """Solver32: each mg3d32_* operator (tests/_f32_ref.check_operators with the length, d in +-50 / length^2) and three
    V(2,2) cycles on random data against orc32_vcycle with this h: u of every level and d below the top bit for bit, the
    norms against the exactly rounded sums"""
    F32.check_operators(c, L, sweeps=(1, 2, 3, 4), sequential_norm=False, grid_length=length,
                        d_scale=50.0 / (length * length))
    start = _f32_start(c, L, length)
    ref = F32.run_cycles(c, L, 2, 3, *start, length)
    assert all(LC.normal(cyc.u_top) for cyc in ref)
    sizes = O.level_sizes(c, L)
    with M.Solver32(c, L, 2, F32.OMEGA, length) as s:
        _assert_spacings(s, c, L, length)
        for f, a in zip((MG3D_U, MG3D_D, MG3D_R), start):
            s.upload(f, L - 1, a)
        got = []
        for cyc in ref:
            got += list(s.vcycles(1))
            F32.assert_same_bits(s.download(MG3D_U, L - 1), cyc.u_top, sizes[-1], L - 1, "u")
            for l in range(L - 1):
                F32.assert_same_bits(s.download(MG3D_D, l), cyc.d_low[l], sizes[l], l, "d")
                F32.assert_same_bits(s.download(MG3D_U, l), cyc.u_low[l], sizes[l], l, "u")
    want = np.array([cyc.norm for cyc in ref])
    print(c, L, length, np.array(got) / want - 1)
    np.testing.assert_allclose(got, want, rtol=F32_NORM_RTOL, atol=0)


# ================================================================================================================ C
def _scaled_equal(got, base, factor, what):
    got, base = np.asarray(got), np.asarray(base)
    assert LC.normal(got) and LC.normal(base), what
    assert same_bits(got, base * factor), what


def _kernels(s, level):
    return {kn: n for (lvl, kn), (n, _) in s.kernel_times().items() if lvl == level}


SCHEDULES = {
    "plain": {"carry": 0, "legs": 0},
    "legs": {"carry": 0, "legs": 1, "legs_min": 66},
    "carry": {"carry": 1, "carry_min": 66, "legs": 0},
    "default": {},
}


def _assert_schedule_ran(sched, nu, N, kt):
    """as tests/test_gpu_screened_variants._assert_variant_ran: a silent fallback must not turn a case into a copy of
    another.  default: one launch per leg from 160 points per side at nu = 2, else none of the run-ahead schedules"""
    assert "colour_pass" not in kt, kt  # the fused kernels ran
    ahead = ("sweep4+norm", "sweep1+restrict", "leg_up", "leg_down")
    if sched == "legs" or (sched == "default" and nu == 2 and N >= 160):
        assert kt.get("leg_up", 0) > 0 and kt.get("leg_down", 0) > 0 and "sweep4+norm" not in kt, kt
    elif sched == "carry":
        assert kt.get("sweep4+norm", 0) > 0 and kt.get("sweep1+restrict", 0) > 0 and "leg_up" not in kt, kt
    else:
        assert not any(kn in kt for kn in ahead), kt


def _assert_coarsest_solve(s, name, c, L, length, sigma):
    """u of level 0 is the direct solve of d of level 0 with the factor of the COARSEST spacing (the identity holds as
    well for a factor built from another level's h)"""
    ref_sigma, eps, axes, faces, mask = LC.operator(name, LC.n_of(c, L))
    e0 = None if eps is None else eps[::1 << (L - 1), ::1 << (L - 1), ::1 << (L - 1)]
    m0 = np.zeros((c, c, c), dtype=np.uint8) if mask is None else MR.inject(MR.stored(mask, axes), L)[0]
    h0 = (length / (LC.n_of(c, L) - 1)) * (1 << (L - 1))
    LU = MR.coarse_lu(c, h0, e0, sigma, axes, faces, m0)
    d0 = s.download(MG3D_D, 0).reshape(c, c, c)
    want = np.zeros((c, c, c))
    MR.coarse_solve(LU, d0, want, axes, faces, sigma, m0)
    assert same_bits(s.download(MG3D_U, 0).reshape(c, c, c), want), "the coarsest level's solve"


def _cycle_run(name, c, L, nu, length, m, sigma, u, d, calls, sched="default", check_coarse=False):
    """one GPU run at grid_length * 2^m: (norms, u of every level, d below the top), d and sigma over 4^m"""
    f = 4.0 ** m
    with _solver(name, c, L, nu, length * 2.0 ** m, sigma=sigma / f) as s:
        for k, v in SCHEDULES[sched].items():
            s.set_option(k, v)
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d / f)
        s.timing_enable(1)
        norms = np.concatenate([s.vcycles(k) for k in calls])
        kt = _kernels(s, L - 1)
        s.timing_enable(0)
        if check_coarse:
            _assert_coarsest_solve(s, name, c, L, length * 2.0 ** m, sigma / f)
        return norms, [s.download(MG3D_U, l) for l in range(L)], [s.download(MG3D_D, l) for l in range(L - 1)], kt


def _assert_identity(run, name, c, L, nu, length, sigma, seed, calls, sched="default", fused=False):
    N = LC.n_of(c, L)
    u, d = LC.data(name, N, length, seed)
    bn, bu, bd, kt = run(name, c, L, nu, length, 0, sigma, u, d, calls, sched, check_coarse=True)
    if fused:
        _assert_schedule_ran(sched, nu, N, kt)
    for m in LC.MS:
        norms, gu, gd, kt = run(name, c, L, nu, length, m, sigma, u, d, calls, sched)
        if fused:
            _assert_schedule_ran(sched, nu, N, kt)
        for l in range(L):
            _scaled_equal(gu[l], bu[l], 1.0, (m, "u", l))
        for l in range(L - 1):
            _scaled_equal(gd[l], bd[l], 4.0 ** -m, (m, "d", l))
        _scaled_equal(norms, bn, 4.0 ** -m, (m, "norms"))


# (c, L, nu, schedule, base length)
FUSED_CASES = ([(9, 5, 2, sched, length) for sched in ("plain", "legs", "carry") for length in (1.0, 3e-4)]
               + [(11, 5, 2, "default", 1.0), (11, 5, 2, "default", 3e-4), (9, 6, 2, "default", 1.0),
                  (9, 5, 1, "default", 1.0), (9, 5, 3, "default", 1.0)])


@pytest.mark.parametrize("c,L,nu,sched,length", FUSED_CASES)
def test_identity_on_the_fused_schedules(c, L, nu, sched, length):
    """the constant operator with sigma = 3.5 / length^2 (dg differs per level), random u and d, calls of 1 then 2 cycles:
    129^3 plain, one launch per leg, carried; 161^3 (off the ladder) and 257^3 (three k-tiles) on the default schedule"""
    _assert_identity(_cycle_run, "constant", c, L, nu, length, 3.5 / (length * length), 100 * c + L, (1, 2), sched, fused=True)


UNFUSED = {"sigma50": ("constant", 50.0), "ball": ("ball", 0.0), "per7": ("per7_sigma", 3.5), "f63": ("f63", 0.0),
           "sphere": ("sphere_f1", 0.0)}


@pytest.mark.parametrize("length", [1.0, 3e-4])
@pytest.mark.parametrize("case", sorted(UNFUSED))
def test_identity_on_the_unfused_families(case, length):
    """129^3, three cycles: sigma = 50 / length^2, the eps ball, per7 (sigma = 3.5 / length^2), f63 (singular) and the
    sphere mask with a Neumann face"""
    name, sigma = UNFUSED[case]
    _assert_identity(_cycle_run, name, 9, 5, 2, length, sigma / (length * length), 77, (3,))


@pytest.mark.parametrize("call,name", [("pcg_solve", "ball"), ("wpcg_solve", "f63"), ("wpcg_solve", "sphere_f1")])
def test_identity_of_the_krylov_solvers(call, name):
    """129^3, three iterations from base length 3e-4: the iterates bit for bit, the same counts, norms 4^-m times"""
    c, L, length = 9, 5, 3e-4
    N = LC.n_of(c, L)
    x0, d = LC.krylov_data(name, N, length)
    sigma = LC.OPERATORS[name][0]

    def run(m):
        f = 4.0 ** m
        with _solver(name, c, L, 2, length * 2.0 ** m, sigma=sigma / f) as s:
            s.upload(MG3D_U, L - 1, x0)
            s.upload(MG3D_D, L - 1, d / f)
            norms, info = getattr(s, call)(rtol=0.0, atol=1e-300, max_iters=3)
            return norms, info["iterations"], s.download(MG3D_U, L - 1)

    bn, bi, bu = run(0)
    assert bi == 3
    for m in LC.MS:
        norms, iters, u = run(m)
        assert iters == bi
        _scaled_equal(u, bu, 1.0, (m, "u"))
        _scaled_equal(norms, bn, 4.0 ** -m, (m, "norms"))


@pytest.mark.parametrize("length", [1.0, 3e-4])
def test_identity_of_step_advance(length):
    """129^3, f22 with the eps ball, two steps of two cycles at theta = 0.5 with a source"""
    name, c, L, theta = "f22_ball", 9, 5, 0.5
    N = LC.n_of(c, L)
    u0, src = LC.data(name, N, length, 31)

    def run(m):
        f = 4.0 ** m
        with _solver(name, c, L, 2, length * 2.0 ** m) as s:
            s.step_setup(DT * length * length * f, theta, KAPPA / (length * length) / f)
            s.step_set_source(src / f)
            s.upload(MG3D_U, L - 1, u0)
            norms, info = s.step_advance(2, cycles=2)
            assert info["steps"] == 2
            return norms, s.download(MG3D_U, L - 1), s.download(MG3D_D, L - 1)

    bn, bu, bd = run(0)
    blk = NR.block(N, 0, 22)
    for m in LC.MS:
        norms, u, d = run(m)
        _scaled_equal(u, bu, 1.0, (m, "u"))
        _scaled_equal(d.reshape(N, N, N)[blk], bd.reshape(N, N, N)[blk] * 1.0, 4.0 ** -m, (m, "d"))
        _scaled_equal(norms, bn, 4.0 ** -m, (m, "norms"))


@pytest.mark.parametrize("length", [1.0, 3e-4])
def test_identity_of_fmg_and_the_field_output(length):
    """129^3, per4 with faces 15: fmg_solve(1), then the gradient (2^-m times; at the base also against
    _field_ref.gradient, which the identity cannot replace: 0.5 / h in another form scales alike), the energy and, with a
    labelled mask set after the solve, the flux (2^m times each)"""
    name, c, L = "per4_f15", 9, 5
    N = LC.n_of(c, L)
    _, _, axes, faces, _ = LC.operator(name, N)
    u0, d = LC.data(name, N, length, 41)
    mask = _labelled_mask(N)

    def run(m):
        f = 4.0 ** m
        with _solver(name, c, L, 2, length * 2.0 ** m) as s:
            s.upload(MG3D_U, L - 1, u0)
            s.upload(MG3D_D, L - 1, d / f)
            norm = s.fmg_solve(1)
            u = s.download(MG3D_U, L - 1)
            grads = {scale: s.gradient(scale) for scale in GRAD_SCALES}
            w = s.field_energy()
            s.set_mask(mask)
            return norm, u, grads, w, [s.field_flux(label) for label in (0, 1, 2)], s.h

    bn, bu, bg, bw, bf, h = run(0)
    assert h == length / (N - 1)
    for scale in GRAD_SCALES:
        want = FR.gradient(bu.reshape(N, N, N), h, axes, faces, scale)
        for a in range(3):
            assert same_bits(bg[scale][a], want[a]), (scale, a)
    for m in LC.MS:
        norm, u, grads, w, fl, _ = run(m)
        _scaled_equal(u, bu, 1.0, (m, "u"))
        _scaled_equal([norm], [bn], 4.0 ** -m, (m, "norm"))
        for scale in GRAD_SCALES:
            for a in range(3):
                _scaled_equal(grads[scale][a], bg[scale][a], 2.0 ** -m, (m, "gradient", scale, a))
        _scaled_equal([w], [bw], 2.0 ** m, (m, "energy"))
        _scaled_equal(fl, bf, 2.0 ** m, (m, "flux"))


# ---- slabs through the loopback transport
def _dist_run(name, c, L, nu, length, m, sigma, u, d, calls, sched="default", check_coarse=False):
    f = 4.0 ** m
    gl = length * 2.0 ** m
    _, eps, _, _, _ = LC.operator(name, LC.n_of(c, L))
    with M.DistSolver(c, L, nu, nranks=4, grid_length=gl) as ds:
        _assert_spacings(ds, c, L, gl)
        assert 1 <= ds.first_level < L
        if sigma:
            ds.set_shift(sigma / f)
        if eps is not None:
            ds.set_coefficient(eps)
        check(ds.L.mg3d_dist_build_coarse(ds._h, ds.h * (1 << (L - 1))))
        ds.upload(MG3D_U, L - 1, u)
        ds.upload(MG3D_D, L - 1, d / f)
        norms = np.concatenate([ds.vcycles(k) for k in calls])
        lv = range(ds.first_level, L)
        u_out = [ds.download(MG3D_U, l) if l in lv else np.zeros(1) for l in range(L)]
        d_out = [ds.download(MG3D_D, l) if l in lv else np.zeros(1) for l in range(L - 1)]
        return norms, u_out, d_out, {}


@pytest.mark.parametrize("name,sigma", [("constant", 0.0), ("constant", 50.0), ("ball", 0.0)],
                         ids=["plain", "set_shift", "set_coefficient"])
def test_identity_on_slabs(monkeypatch, name, sigma):
    """DistSolver (9, 5) on four virtual slabs of at least 8 planes: u and d of every distributed level, the norms; the
    base run's finest u is the single domain's"""
    monkeypatch.setenv("MG3D_SLAB_MIN_PLANES", "8")
    c, L, length = 9, 5, 1.0

    def run(nm, c_, L_, nu, length_, m, sg, u, d, calls, sched, check_coarse=False):
        out = _dist_run(nm, c_, L_, nu, length_, m, sg, u, d, calls)
        if check_coarse:  # the base run: against the single domain
            single = _cycle_run(nm, c_, L_, nu, length_, 0, sg, u, d, calls)
            assert same_bits(out[1][-1], single[1][-1])
        return out

    _assert_identity(run, name, c, L, 2, length, sigma, 55, (1, 2))


@pytest.mark.parametrize("dist", [False, True])
def test_identity_of_the_f32_variant(monkeypatch, dist):
    """Solver32 and DistSolver32 (four slabs) at (9, 5), nu = 2, two calls: the division of a binary32 d by 4^m is exact"""
    monkeypatch.setenv("MG3D_SLAB_MIN_PLANES", "8")
    c, L, length = 9, 5, 1.0
    u0, d0, _ = _f32_start(c, L, length, seed=9)

    def run(m):
        gl = length * 2.0 ** m
        make = (lambda: M.DistSolver32(c, L, 2, nranks=4, grid_length=gl)) if dist else (lambda: M.Solver32(c, L, 2, grid_length=gl))
        with make() as s:
            _assert_spacings(s, c, L, gl)
            s.upload(MG3D_U, L - 1, u0)
            s.upload(MG3D_D, L - 1, d0 / np.float32(4.0 ** m))
            norms = np.concatenate([s.vcycles(1), s.vcycles(2)])
            return norms, s.download(MG3D_U, L - 1), s.download(MG3D_D, L - 2)

    bn, bu, bd = run(0)
    for m in LC.MS:
        norms, u, d = run(m)
        _scaled_equal(u, bu, np.float32(1.0), (m, "u"))
        _scaled_equal(d, bd, np.float32(4.0 ** -m), (m, "d"))
        _scaled_equal(norms, bn, 4.0 ** -m, (m, "norms"))
