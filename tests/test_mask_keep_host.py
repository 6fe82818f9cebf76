"""The KEEP coarsening rule of the fixed-point mask (mg3d_ctx_set_mask_coarsening) and full multigrid with a mask, on the
numpy restatement tests/_mask_keep_ref.py alone: the invariant, what the rule leaves alone, duplicates, labels, and that
plain cycles contract under KEEP where they grow under injection.  No GPU."""
import itertools

import numpy as np
import pytest

import _mask_keep_ref as MK
import _mask_ref as MR
import _neumann_ref as NR

SHAPES = [(5, 3), (5, 4), (7, 3)]  # 17^3, 33^3, 25^3
AXES = [0, 1, 4, 5, 7]


def _n(c, L):
    return (c - 1) * (1 << (L - 1)) + 1


def _masks(N):
    return {"thin": MK.thin_mask(N), "gpu_test_mask": MR.gpu_test_mask(N), "plate": MR.plate(N, (N // 2) | 1),
            "needle": MR.needle(N), "random": MR.random_mask(N), "sphere": MR.sphere(N)}


def _brute(mf):
    """the rule as include/mg3d.h states it, point by point"""
    N = mf.shape[0]
    Nc = (N + 1) // 2
    mc = np.zeros((Nc, Nc, Nc), dtype=np.uint8)
    for I, J, K in itertools.product(range(Nc), repeat=3):
        if mf[2 * I, 2 * J, 2 * K]:
            mc[I, J, K] = mf[2 * I, 2 * J, 2 * K]
            continue
        for a, b, c in MK.ORDER:
            F = (2 * I + a, 2 * J + b, 2 * K + c)
            if max(F) > N - 1 or not mf[F]:
                continue
            if all(mf[2 * (I + a * al), 2 * (J + b * be), 2 * (K + c * ga)] == 0
                   for al, be, ga in itertools.product((0, 1), repeat=3)):
                mc[I, J, K] = mf[F]
                break
    return mc


@pytest.mark.parametrize("axes", [0, 5])
def test_the_vectorised_rule_is_the_stated_rule(axes):
    N = 17
    m = MR.stored(MK.thin_mask(N), axes)
    mc, origin = MK.keep_level(m, axes)
    want = _brute(m)
    MR.PER.refresh(want, axes)
    assert np.array_equal(mc, want)
    got = origin >= 0
    assert np.array_equal(got, (mc != 0) & (m[::2, ::2, ::2] == 0))
    assert np.array_equal(m.reshape(-1)[origin[got]], mc[got]), "a coarse byte is the byte of the point it stands for"


@pytest.mark.parametrize("N", [17, 25, 33, 65])
@pytest.mark.parametrize("axes", range(8))
def test_the_named_points_of_the_test_mask_are_lost(N, axes):
    """every point thin_mask names -- (1,1,1), (N-2,N-2,N-2), the three whose upper parent is on the last plane of an axis,
    the six on the faces -- is there after the periodic duplicates took their sources' bytes, is lost by the stated rule,
    and is the point its lower parent stands for (a duplicate parent: what its source stands for); the bodies are there too"""
    m = MR.stored(MK.thin_mask(N), axes)
    mc, origin = MK.keep_level(m, axes)
    idx = np.arange(N ** 3).reshape(N, N, N)
    pts = MK.thin_points(N)
    assert len(pts) == 11 and len({F for F, _ in pts.values()}) == 11
    for name, (F, byte) in pts.items():
        C = tuple(x // 2 for x in F)
        assert m[F] == byte, name
        parents = {(C[0] + al * (F[0] & 1), C[1] + be * (F[1] & 1), C[2] + ga * (F[2] & 1))
                   for al, be, ga in itertools.product((0, 1), repeat=3)}
        assert all(m[2 * P[0], 2 * P[1], 2 * P[2]] == 0 for P in parents), f"{name}: a parent's own fine point is fixed"
        src = tuple(0 if MR.PER.per(axes, ax) and F[ax] == N - 1 else F[ax] for ax in range(3))
        assert mc[C] == byte and origin[C] == idx[src], name
    assert origin[0, 0, 0] == idx[1, 1, 1]
    q = (N // 2) | 1
    assert (m[q, 4:N - 4, 4:N - 4] != 0).mean() > 0.9 and m[N // 4 + 1, N // 4 + 1, N // 4 + 1] == 1  # the plate, the block
    assert (m[N // 4 + 2:N - N // 4 - 2, q, q] != 0).mean() > 0.7  # the needle
    assert 0.08 < (m != 0).mean() < 0.2


# (c, L, periodic axes): the shapes and periodic words of tests/test_gpu_mask_keep_shapes.py past coarse column 64
SEAM_CASES = [(10, 5, 0), (6, 6, 0), (11, 5, 7), (11, 5, 4), (11, 5, 2)]


@pytest.mark.parametrize("c,L,axes", SEAM_CASES)
def test_the_seam_mask_reaches_past_coarse_column_64(c, L, axes):
    """seam_mask at 145^3 and 161^3, what tests/test_gpu_mask_keep_shapes.py relies on: every planted point (and every named
    point of thin_mask under it) is lost by the stated rule and is the point its lower parent stands for, with its own
    byte; on the level below the finest at least 1000 lost points have a coarse column 64 <= K <= Nc-2 and at least one
    has K == Nc-1; the invariant holds on every level.  Measured: 16146 and 1041 at 145^3; 39755 and 1315 at 161^3
    without a periodic axis, 40240 and 2454 with all three"""
    N = _n(c, L)
    assert N in (145, 161)
    Nc = (N + 1) // 2
    m = MR.stored(MK.seam_mask(N), axes)
    levels, origins = MK.keep(m, L, axes, origins=True)
    mc, origin = levels[L - 2], origins[L - 2]
    idx = np.arange(N ** 3).reshape(N, N, N)
    planted = MK.seam_points(N)
    assert len({F for F, _ in planted}) == len({b for _, b in planted}) == len(planted) == 72
    assert {F[2] for F, _ in planted} >= set(MK.SEAM) and {F[1] for F, _ in planted} >= set(MK.SEAM)
    for F, byte in planted + list(MK.thin_points(N).values()):
        C = tuple(x // 2 for x in F)
        assert m[F] == byte, F
        parents = {(C[0] + al * (F[0] & 1), C[1] + be * (F[1] & 1), C[2] + ga * (F[2] & 1))
                   for al, be, ga in itertools.product((0, 1), repeat=3)}
        assert all(m[2 * P[0], 2 * P[1], 2 * P[2]] == 0 for P in parents), f"{F}: a parent's own fine point is fixed"
        src = tuple(0 if MR.PER.per(axes, ax) and F[ax] == N - 1 else F[ax] for ax in range(3))
        assert mc[C] == byte and origin[C] == idx[src], F
    assert {F[2] // 2 for F, _ in planted} >= {62, 63, 64, 65}  # both sides of the boundary between the k-blocks
    inside, last = MK.second_block_counts(origin, Nc)
    print(N, axes, "lost points with 64 <= K <= Nc-2:", inside, "with K == Nc-1:", last)
    assert inside >= 1000 and last >= 1
    for l in range(1, L):
        assert MK.parents_fixed(levels[l], levels[l - 1]).all(), l
    assert 0.08 < (m != 0).mean() < 0.2


@pytest.mark.parametrize("c,L", SHAPES)
@pytest.mark.parametrize("axes", AXES)
def test_every_fixed_point_has_a_fixed_parent_on_every_level(c, L, axes):
    """the invariant, on raw bytes, for every test mask; injection breaks it on each of the thin ones"""
    N = _n(c, L)
    for name, mask in _masks(N).items():
        top = MR.stored(mask, axes)
        levels = MK.keep(top, L, axes)
        assert np.array_equal(levels[-1], top)
        for l in range(1, L):
            assert MK.parents_fixed(levels[l], levels[l - 1]).all(), (name, l)
            dup = levels[l - 1].copy()
            MR.PER.refresh(dup, axes)
            assert np.array_equal(dup, levels[l - 1]), f"{name}: coarse duplicates differ from their sources on level {l - 1}"
            assert set(np.unique(levels[l - 1])) <= set(np.unique(levels[l])), f"{name}: a label appeared on level {l - 1}"
        if name != "sphere":
            inj = MR.inject(top, L)
            assert not all(MK.parents_fixed(inj[l], inj[l - 1]).all() for l in range(1, L)), name


@pytest.mark.parametrize("N,L", [(33, 4), (65, 5)])
def test_keep_is_injection_on_the_sphere(N, L):
    top = MR.stored(MR.sphere(N), 0)
    for a, b in zip(MK.keep(top, L), MR.inject(top, L)):
        assert np.array_equal(a, b)


def test_labels_survive():
    """the plate's, the needle's and the single points' labels reach level 0; a body keeps one label per level"""
    N, L = 33, 4
    mask = np.zeros((N, N, N), dtype=np.uint8)
    mask[MR.plate(N, (N // 2) | 1) != 0] = 7
    mask[MR.needle(N) != 0] = 9
    mask[1, 1, 1] = 11
    mask[N - 2, N - 2, N - 2] = 13
    levels = MK.keep(mask, L)
    for l in range(L):
        assert set(np.unique(levels[l])) == {0, 7, 9, 11, 13}, l
    n0 = levels[0].shape[0]
    assert levels[0][0, 0, 0] == 11 and levels[0][n0 - 2, n0 - 2, n0 - 2] == 13  # the lower parent, level by level
    inj = MR.inject(mask, L)
    assert not inj[0].any() and not inj[L - 2].any()


def test_the_lost_plane_of_exact_problem_b_stays():
    """plane i = 11 at 17^3, gone from both coarse levels under injection: under KEEP plane 5 of level 1 and plane 2 of
    level 0 (the lower parent each time: the bias towards the low index)"""
    axes, faces, mask, _, _ = MR.exact_problem("b")
    top = MR.stored(mask, axes)
    inj, kept = MR.inject(top, 3), MK.keep(top, 3, axes)
    assert not inj[1].any() and not inj[0].any()
    for l, plane in ((1, 5), (0, 2)):
        want = np.zeros_like(kept[l])
        want[plane] = 1
        assert np.array_equal(kept[l], want), l


def test_cycles_contract_under_keep_and_grow_under_injection():
    """33^3 Dirichlet box, c = 5, V(2,2), gpu_test_mask held at 1, a random right-hand side (seed 1): ten restatement
    cycles.  Measured: a factor of 0.42 per cycle under KEEP, 1.78 under injection (tools/mask_coarsening_convergence.py)"""
    N, L = 33, 4
    mask = MR.gpu_test_mask(N)
    d = np.random.default_rng(1).standard_normal((N, N, N))
    norms = {}
    for rule in (MK.KEEP, MK.INJECT):
        prob = MK.Hierarchy(5, L, 2, 0.0, None, 0, 0, mask, rule=rule)
        prob.u[-1][mask != 0] = 1.0
        prob.d[-1][...] = d
        norms[rule] = prob.vcycles(10)
        print(rule, norms[rule], (norms[rule][9] / norms[rule][3]) ** (1.0 / 6))
    assert norms[MK.KEEP][9] < norms[MK.KEEP][3]
    assert norms[MK.INJECT][9] > norms[MK.INJECT][3]


def test_the_inject_rule_is_the_parent_class():
    N, L = 17, 3
    mask = MK.thin_mask(N)
    a = MK.Hierarchy(5, L, 2, 0.0, None, 4, 3, mask, rule=MK.INJECT)
    b = MR.Hierarchy(5, L, 2, 0.0, None, 4, 3, mask)
    for x, y in zip(a.mask, b.mask):
        assert np.array_equal(x, y)
    assert np.array_equal(a.LU, b.LU)


@pytest.mark.parametrize("axes,faces", [(0, 0), (5, 0), (0, 1 | 8), (4, 3), (7, 0)])
def test_masked_fmg_keeps_the_callers_values_and_never_reads_d_at_fixed_points(axes, faces):
    """the restatement of mg3d_fmg_solve with a mask at 17^3: u at the fixed and Dirichlet points and d come back as given,
    NaN in d at the fixed points reaches nothing, the result does not depend on what u held elsewhere, and every level's
    fixed unknowns carry a potential of the finest level's body during the descent"""
    c, L, N = 5, 3, 17
    mask = MK.thin_mask(N)
    rng = np.random.default_rng(3)
    u, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    NR.refresh(u, axes)
    NR.refresh(d, axes)
    prob = MK.Hierarchy(c, L, 2, 0.0, None, axes, faces, mask)
    fx = prob.fixed()
    held = MR._keep(prob.mask[-1], axes, faces) | MK.FR.dirichlet_mask(N, axes, faces)
    u[fx] = 2.5
    NR.refresh(u, axes)
    results = []
    for poison, other in ((False, 0.0), (True, 1e3)):
        prob = MK.Hierarchy(c, L, 2, 0.0, None, axes, faces, mask)
        prob.u[-1][...] = np.where(held, u, other)
        prob.d[-1][...] = d
        if poison:
            prob.d[-1][fx] = np.nan
        d_in = prob.d[-1].copy()
        for l in range(L - 1, 0, -1):  # the descent of u alone (fmg_solve below does it again)
            MK.inject_u(prob, l)
            f = prob.fixed(l - 1)
            assert f.any() and (prob.u[l - 1][f] == 2.5).all(), f"level {l - 1}: a fixed unknown without the body's potential"
        norm = MK.fmg_solve(prob, 1)
        assert np.isfinite(norm) and np.isfinite(prob.u[-1]).all()
        assert np.array_equal(prob.u[-1][held], u[held])
        assert np.array_equal(prob.d[-1], d_in, equal_nan=True)
        results.append(prob.u[-1].copy())
    assert np.array_equal(results[0], results[1])


def test_fmg_beats_one_cycle_on_the_plate():
    """the plate held at 1 in a grounded 33^3 box, d = 0: the residual norm after fmg_solve(1) under KEEP is below that
    of one plain KEEP cycle from the zero guess (measured 1.59e3 against 6.56e3) -- the inequality the GPU test asserts"""
    N, L = 33, 4
    mask = MR.plate(N, (N // 2) | 1)
    norms = []
    for solve in (lambda p: MK.fmg_solve(p, 1), lambda p: p.vcycle()):
        prob = MK.Hierarchy(5, L, 2, 0.0, None, 0, 0, mask)
        prob.u[-1][mask != 0] = 1.0
        norms.append(solve(prob))
    print(norms)
    assert norms[0] < norms[1]
