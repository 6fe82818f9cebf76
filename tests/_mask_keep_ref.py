"""CPU reference of the second coarsening rule of the fixed-point mask (mg3d_ctx_set_mask_coarsening, MG3D_MASK_KEEP) and
of full multigrid with a mask under it (mg3d_fmg_solve, mg3d_fmg_interpolate), on top of tests/_mask_ref.py and
tests/_fmg_ref.py by import, with the library's arithmetic.

KEEP, level l -> l-1, on the stored bytes of the fine level (its periodic duplicates hold their sources' bytes; raw
bytes, no boundary word): a coarse point C whose own fine point 2C is fixed takes that byte (injection); otherwise it takes
the byte of the first LOST fine point among F = 2C + (a, b, c) in the order (0,0,1), (0,1,0), (0,1,1), (1,0,0), (1,0,1),
(1,1,0), (1,1,1) -- F inside the array, its byte nonzero, and the byte at 2P zero for every parent P = C + (a*al, b*be,
c*ga), al, be, ga in {0, 1} --, or 0; then the coarse duplicates take their sources' bytes.  `origin` says which F that was.

Masked FMG: d restricted with 0. in place of d at the fixed unknowns, u injected except that a coarse fixed unknown that
stands for a lost point takes u of that point, level 0 solved with u's own values at Dirichlet AND fixed points, the cubic
interpolation not writing fine fixed points, cycles that keep the guess.  Test infrastructure only."""
import numpy as np

import _fmg_ref as FR
import _mask_ref as MR
import _neumann_ref as NR
import _periodic_ref as PER
import _shift_field_ref as SF

INJECT, KEEP = 0, 1  # MG3D_MASK_INJECT, MG3D_MASK_KEEP
ORDER = [(0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]


def keep_level(mf, axes=0):
    """one level: (the coarse bytes, origin) from the fine level's stored bytes; origin[C] is the flat fine index of the
    lost point C stands for, -1 where C is injected or not fixed (a duplicate holds its source's)"""
    mf = np.ascontiguousarray(mf, dtype=np.uint8)
    N = mf.shape[0]
    Nc = (N + 1) // 2
    inj = mf[::2, ::2, ::2]
    mc = inj.copy()
    origin = np.full((Nc, Nc, Nc), -1, dtype=np.int64)
    idx = np.arange(N ** 3, dtype=np.int64).reshape(N, N, N)
    zero = inj == 0  # "the byte at 2P is zero"
    open_ = zero.copy()  # C takes no byte yet
    for a, b, c in ORDER:
        # F = 2C + (a, b, c) exists for C up to Nc-1-a, Nc-1-b, Nc-1-c
        at = (slice(0, Nc - a), slice(0, Nc - b), slice(0, Nc - c))
        F = mf[a::2, b::2, c::2]
        lost = F != 0
        for al in range(a + 1):
            for be in range(b + 1):
                for ga in range(c + 1):
                    lost = lost & zero[al:Nc - a + al, be:Nc - b + be, ga:Nc - c + ga]
        take = lost & open_[at]
        mc[at][take] = F[take]
        origin[at][take] = idx[a::2, b::2, c::2][take]
        open_[at][take] = False
    PER.refresh(mc, axes)
    PER.refresh(origin, axes)
    return mc, origin


def keep(mask, L, axes=0, origins=False):
    """the masks of levels 0 .. L-1 from the finest one's stored bytes under KEEP, beside _mask_ref.inject (origins: also
    the list of origin arrays, entry l belonging to level l < L-1, None for the finest)"""
    out = [np.ascontiguousarray(mask, dtype=np.uint8)]
    org = [None]
    for _ in range(L - 1):
        mc, o = keep_level(out[0], axes)
        out.insert(0, mc)
        org.insert(0, o)
    return (out, org) if origins else out


def parents_fixed(mf, mc):
    """the invariant: True where a fine point is not fixed or at least one of its parents on the coarse level is (raw
    bytes); parents of F: floor(F/2) + (odd_i*al, odd_j*be, odd_k*ga)"""
    N, Nc = mf.shape[0], mc.shape[0]
    c = mc != 0
    x = np.arange(N)
    lo, hi = x // 2, np.minimum((x + 1) // 2, Nc - 1)
    ok = np.zeros((N, N, N), dtype=bool)
    for pi in (lo, hi):
        for pj in (lo, hi):
            for pk in (lo, hi):
                ok |= c[np.ix_(pi, pj, pk)]
    return ok | (mf == 0)


class Hierarchy(MR.Hierarchy):
    """_mask_ref.Hierarchy with the coarser masks taken under `rule` (KEEP by default; INJECT: the parent class itself)"""

    def __init__(self, c, L, nu, sigma, eps, axes, faces, mask, grid_length=1.0, rule=KEEP):
        MR.Hierarchy.__init__(self, c, L, nu, sigma, eps, axes, faces, mask, grid_length, lu=rule != KEEP)
        self.rule = rule
        self.origin = [None] * L
        if rule == KEEP:
            self.mask, self.origin = keep(self.mask[-1], L, axes, origins=True)
            self.LU = MR.coarse_lu(c, self.h * (1 << (L - 1)), self.e(0), sigma, axes, faces, self.mask[0])


class FieldHierarchy(SF.Hierarchy):
    """_shift_field_ref.Hierarchy (a mask and a screening field s) with the coarser masks taken under KEEP"""

    def __init__(self, c, L, nu, sigma, eps, axes, faces, mask, s, grid_length=1.0):
        SF.Hierarchy.__init__(self, c, L, nu, sigma, eps, axes, faces, mask, s, grid_length, lu=False)
        self.mask, self.origin = keep(self.mask[-1], L, axes, origins=True)
        self.LU = SF.coarse_lu(c, self.h * (1 << (L - 1)), self.e(0), sigma, axes, faces, self.mask[0], self.sf(0))


# ---- full multigrid with a mask

def restrict_d(prob, l):
    """d[l-1] = the restriction of d[l] with 0. stored at the fixed unknowns of level l (d there may hold anything)"""
    dz = prob.d[l].copy()
    dz[prob.fixed(l)] = 0.
    NR.restrict(dz, prob.d[l - 1], prob.axes, prob.faces)


def inject_u(prob, l):
    """u[l-1] = the injection of u[l]; a fixed unknown C of level l-1 with m_l[2C] == 0 takes u[l] at the lost point it
    stands for; a periodic duplicate asks at its source"""
    uc = prob.u[l - 1]
    uc[...] = prob.u[l][::2, ::2, ::2]
    org = prob.origin[l - 1]
    if org is None:
        return
    sel = prob.fixed(l - 1) & (org >= 0)
    PER.refresh(sel, prob.axes)
    uc[sel] = prob.u[l].reshape(-1)[org[sel]]


def interpolate(prob, l):
    """mg3d_fmg_interpolate(l): _fmg_ref.interpolate, the fixed unknowns of level l (and their duplicates) not written"""
    uf = prob.u[l]
    keep_ = MR._keep(prob.mask[l], prob.axes, prob.faces)
    old = uf[keep_].copy()
    FR.interpolate(prob.u[l - 1], uf, prob.axes, prob.faces)
    uf[keep_] = old


def vcycle_keep_guess(prob, q):
    """Hierarchy.vcycle from level q with u[q] as it stands as the guess (the levels below start from zero)"""
    if q == prob.L - 1 or q == 0:
        return prob.vcycle(q)
    for _ in range(prob.nu):
        prob.colour_pass(q, 1)
        prob.colour_pass(q, 0)
    prob.residual(q, prob.r[q])
    NR.restrict(prob.r[q], prob.d[q - 1], prob.axes, prob.faces)
    prob.vcycle(q - 1)
    prob.prolong(q)
    for _ in range(prob.nu):
        prob.colour_pass(q, 0)
        prob.colour_pass(q, 1)
    return prob.residual(q)


def fmg_solve(prob, cycles=1):
    """mg3d_fmg_solve on a Hierarchy: prob.u[-1] (its Dirichlet and fixed points) and prob.d[-1]; returns the residual
    norm after the last finest-level cycle"""
    assert cycles >= 1
    L, axes, faces = prob.L, prob.axes, prob.faces
    for l in range(L - 1, 0, -1):
        restrict_d(prob, l)
        inject_u(prob, l)
    m = FR.dirichlet_mask(prob.N[0], axes, faces)
    b = prob.d[0] if L > 1 else prob.d[0].copy()  # (one level: d is the caller's and stays)
    b[m] = prob.u[0][m]
    MR.coarse_solve(prob.LU, b, prob.u[0], axes, faces, prob.sigma, prob.mask[0], one_level=True)
    norm = 0.0
    for l in range(1, L):
        interpolate(prob, l)
        for _ in range(cycles):
            norm = vcycle_keep_guess(prob, l)
    return norm


# ---- the test mask

def thin_points(N):
    """the named lost points of thin_mask: name -> ((i, j, k), byte)"""
    q = (N // 2) | 1
    pts = {"low corner": ((1, 1, 1), 3), "high corner": ((N - 2, N - 2, N - 2), 4)}
    for ax in range(3):
        p = [q, q + 2, q - 2]
        p[ax] = N - 2  # the upper parent has index Nc-1 along ax: a periodic duplicate where the axis is periodic
        pts[f"upper parent on the last plane of axis {ax}"] = (tuple(p), 5)
        for end in (0, N - 1):
            p = [q + 2, q - 2, q]
            p[ax] = end  # on a face (a Neumann face where the face is one), odd along the other two axes
            pts[f"face {2 * ax + (end != 0)}"] = (tuple(p), 6)
    return pts


def _images(p, N):
    """p and the points that share its bytes when axes are periodic: index 0 and index N-1 stand for each other"""
    alts = [(x,) if x not in (0, N - 1) else (0, N - 1) for x in p]
    return [(i, j, k) for i in alts[0] for j in alts[1] for k in alts[2]]


def thin_mask(N, seed=3):
    """The mask of the KEEP tests.  The bodies of _mask_ref.gpu_test_mask -- random at 10 % density, a thick block, a
    one-point plate on an odd plane -- and a needle on odd j, k (byte 2 or 3), then the named points of thin_points, each
    made LOST whatever the boundary masks: around a named point F the fine points 2P of all its parents P and the other
    children of its lower parent C = floor(F/2) are cleared (with their images under periodic axes: index 0 and N-1 of an
    axis stand for each other), so that C stands for F and nothing else (origin[C] = F).  Named: lost points at (1,1,1) and
    (N-2,N-2,N-2), one whose upper parent lies on the last plane of each axis, one on each of the six faces."""
    m = MR.gpu_test_mask(N, seed)
    m |= MR.needle(N) * np.uint8(2)
    pts = thin_points(N)
    for F, _ in pts.values():
        C = tuple(x // 2 for x in F)
        odd = tuple(x & 1 for x in F)
        clear = []
        for t in range(8):
            a, b, c = t >> 2, (t >> 1) & 1, t & 1
            clear.append((2 * C[0] + a, 2 * C[1] + b, 2 * C[2] + c))  # C's own fine point and its children
            clear.append((2 * (C[0] + a * odd[0]), 2 * (C[1] + b * odd[1]), 2 * (C[2] + c * odd[2])))  # the parents' fine points
        for p in clear:
            if max(p) <= N - 1:
                for g in _images(p, N):
                    m[g] = 0
    for F, byte in pts.values():
        for g in _images(F, N):
            m[g] = byte
    return m


SEAM = (125, 127, 129, 131)  # fine indices around coarse index 64: its lower parents are coarse 62 .. 65


def seam_points(N):
    """the planted lost points of seam_mask: [((i, j, k), byte), ...], the bytes all different.  All three indices odd: k
    in SEAM (those below N-1) with i and j in {1, N//2|1, N-2}, then the same with j and k exchanged; a named point of
    thin_mask is left to it"""
    q = (N // 2) | 1
    side = (1, q, N - 2)
    seam = [x for x in SEAM if x <= N - 2]
    pts = [(i, j, k) for i in side for j in side for k in seam]
    pts += [(i, k, j) for i, j, k in pts if (i, k, j) not in pts]
    named = {F for F, _ in thin_points(N).values()}  # (129: the high corner is one of thin_mask's)
    pts = [p for p in pts if p not in named]
    assert len(pts) < 200
    return [(p, 32 + n) for n, p in enumerate(pts)]


def seam_mask(N, seed=3):
    """thin_mask with lost points planted where the threads of a kernel that runs one thread per COARSE point pass from
    their first block of 64 lanes in k into the second (N >= 129: coarse side >= 65), and the same pattern along j.  Each
    planted point F is made lost as thin_mask makes its named points lost: the fine points 2P of its eight parents and the
    other children of its lower parent C = floor(F/2) are cleared with their images, so that origin[C] = F under every
    periodic mask (no planted point lies on a face).  Its byte is its own (seam_points): a coarse byte taken from the wrong
    fine point is a wrong byte."""
    m = thin_mask(N, seed)
    pts = seam_points(N)
    for F, _ in pts:
        for t in range(8):
            a, b, c = t >> 2, (t >> 1) & 1, t & 1
            for p in ((F[0] - 1 + a, F[1] - 1 + b, F[2] - 1 + c),  # 2C and the children of C
                      (F[0] - 1 + 2 * a, F[1] - 1 + 2 * b, F[2] - 1 + 2 * c)):  # the parents' fine points
                for g in _images(p, N):
                    m[g] = 0
    for F, byte in pts:
        m[F] = byte
    return m


def second_block_counts(origin_level, Nc):
    """(lost points whose coarse point has 64 <= K <= Nc-2, those with K == Nc-1) of one level's origin array: what a
    kernel with one thread per coarse point reaches only in its second block of 64 lanes"""
    lost = origin_level >= 0
    return int(lost[:, :, 64:Nc - 1].sum()), int(lost[:, :, Nc - 1].sum())


