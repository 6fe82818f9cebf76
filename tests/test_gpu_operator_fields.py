"""The operator fields of one context -- the coefficient eps, the fixed-point mask, the screening field s -- set, replaced and
cleared NEXT TO ONE ANOTHER.  The other files set the fields in every order but clear each one only on its own; this file
walks one context through the transitions between them:

    1 a field on a constant context (the kernels run over the internal eps = 1)    6 other periodic and Neumann masks under both
    2 eps set (the internal ones released)                                         7 the mask cleared
    3 eps cleared while the field stays (the ones are back)                        8 the field cleared
    4 the field replaced by another                                                9 no boundary mask: the fused constant context
    5 a mask set

once through the host forms and once through the tensor forms, from Dirichlet faces and from periodic k + Neumann on both i
faces.  After every step the same random u and d are uploaded and two cycles run.  The reference is the numpy restatement
tests/_shift_field_ref.Hierarchy, built fresh for what the context holds at that step -- not another context of the library:
the same bits of u, the same bits of eps, mask and field on every level where set, the has_* answers, the norms to the
summation tolerance of tests/test_gpu_parity.py (norm_rtol).

17^3 (c = 5, L = 3): nothing here depends on launch tails; tests/test_gpu_mask_shapes.py and test_gpu_shift_field_shapes.py
hold the count and check kernels past one k-block.  The second start runs with sigma = 0 and ends step 6 with every axis
periodic or Neumann on both faces: steps 6 and 7 are regular through the mask and the positive field, step 8 is the pinned,
singular context -- the counts of both fields have to be gone with them.

What a context keeps of an array is tracked as the library documents it: periodic duplicates take their sources' values when
a field is set, and a mask's and a field's again whenever the periodic axes change (for good).

The kernels without d (mg3d_ctx_dnone_launches) only exist above 65 points per side, so that step 9 is the fused context
again is shown by a second walk at 97^3 (c = 7, L = 5, the options of tests/test_gpu_dnone.py) with d = 0 and no restatement:
no launch without d while any field or boundary mask is set, and the count grows again behind step 9."""
import numpy as np
import pytest
import torch  # before the package, as bench.py does: the HIP runtime is torch's

import _coef_ref as CR
import _mask_ref as MR
import _neumann_ref as NR
import _shift_field_ref as SF
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_U

from test_gpu_parity import norm_rtol

pytestmark = pytest.mark.gpu

# start (axes, faces), the masks of step 6, sigma
RUNS = {"dirichlet": ((0, 0), (2, 3), 0.75), "periodic_k_neumann_i": ((4, 3), (1, 60), 0.0)}
STEPS = ("field", "eps", "eps cleared", "field replaced", "mask", "boundaries", "mask cleared", "field cleared", "constant")


def _same_bits(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _n(c, L):
    return (c - 1) * (1 << (L - 1)) + 1


class _Held:
    """what the context holds: the boundary masks and the finest level's arrays as stored (None: not set)"""

    def __init__(self, axes, faces):
        self.axes, self.faces = axes, faces
        self.eps = self.mask = self.field = None

    def periodic(self, axes):
        self.axes = axes
        if self.mask is not None:
            self.mask = MR.stored(self.mask, axes)
        if self.field is not None:
            self.field = SF.stored(self.field, axes)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda:0"))


def _set(s, form, what, a):
    if form == "host":
        {"eps": s.set_coefficient, "mask": s.set_mask, "field": s.set_shift_field}[what](a)
    else:
        {"eps": s.set_coefficient_tensor, "mask": s.set_mask_tensor, "field": s.set_shift_field_tensor}[what](_dev(a))


def _boundaries(s, held, axes, faces):
    """Neumann faces off first: an axis is periodic or has Neumann faces, never both"""
    s.set_neumann(0)
    s.set_periodic(axes)
    s.set_neumann(faces)
    held.periodic(axes)
    held.faces = faces


def _walk(s, form, run, N):
    """the nine steps on solver s; yields (step, what the context holds) behind each"""
    (axes, faces), alt, _ = RUNS[run]
    eps, mask = CR.FIELDS["exp"](N), MR.gpu_test_mask(N)
    f1, f2 = (SF.random_field(N, 1.0 / (N - 1), seed) for seed in (1, 2))
    held = _Held(axes, faces)
    for step in STEPS:
        if step in ("field", "field replaced"):
            _set(s, form, "field", f1 if step == "field" else f2)
            held.field = SF.stored(f1 if step == "field" else f2, held.axes)
        elif step == "eps":
            _set(s, form, "eps", eps)
            held.eps = eps
        elif step == "mask":
            _set(s, form, "mask", mask)
            held.mask = MR.stored(mask, held.axes)
        elif step == "boundaries":
            _boundaries(s, held, *alt)
        elif step == "constant":
            _boundaries(s, held, 0, 0)
        else:
            what = {"eps cleared": "eps", "mask cleared": "mask", "field cleared": "field"}[step]
            _set(s, form, what, None)
            setattr(held, what, None)
        yield step, held


_WANT = {}


def _want(run, step, held, c, L, u, d):
    """the restatement's two cycles from (u, d) for what the context holds, once per (run, step): the host and the tensor walk
    share it"""
    if (run, step) not in _WANT:
        ref = SF.Hierarchy(c, L, 2, RUNS[run][2], held.eps, held.axes, held.faces, held.mask, held.field)
        ref.u[-1][...] = u
        ref.d[-1][...] = d
        NR.refresh(ref.u[-1], held.axes)
        NR.refresh(ref.d[-1], held.axes)
        start = ref.u[-1].copy(), ref.d[-1].copy()
        _WANT[run, step] = ref, start, ref.vcycles(2)
    return _WANT[run, step]


@pytest.mark.parametrize("form", ["host", "tensor"])
@pytest.mark.parametrize("run", sorted(RUNS))
def test_walk_against_the_restatement(run, form):
    c, L = 5, 3
    N = _n(c, L)
    (axes, faces), _, sigma = RUNS[run]
    rng = np.random.default_rng(17)
    u, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    with M.Solver(c, L, 2) as s:
        s.set_shift(sigma)
        s.set_periodic(axes)
        s.set_neumann(faces)
        s.get_details()  # every step from here on rebuilds the factor
        for step, held in _walk(s, form, run, N):
            ref, (u0, d0), want = _want(run, step, held, c, L, u, d)
            assert (s.has_coefficient(), s.has_mask(), s.has_shift_field()) == \
                (held.eps is not None, held.mask is not None, held.field is not None), step
            assert (s.periodic, s.neumann) == (held.axes, held.faces), step
            s.upload(MG3D_U, L - 1, u0)
            s.upload(MG3D_D, L - 1, d0)
            got = s.vcycles(2)
            assert _same_bits(s.download(MG3D_U, L - 1), ref.u[-1]), step
            for l in range(L):
                if held.eps is not None:
                    assert _same_bits(s.coefficient(l), ref.e(l)), (step, l)
                if held.mask is not None:
                    assert np.array_equal(s.get_mask(l), ref.mask[l]), (step, l)
                if held.field is not None:
                    assert _same_bits(s.get_shift_field(l), ref.s[l]), (step, l)
            np.testing.assert_allclose(got, want, rtol=norm_rtol(N), err_msg=step)
        if run != "dirichlet":
            pinned = _WANT[run, "field cleared"][0]
            assert pinned.pinned() and pinned.is_singular(), "step 8 of this run is the singular context"


@pytest.mark.parametrize("form", ["host", "tensor"])
def test_walk_ends_in_the_fused_schedules(form):
    """97^3, d = 0 (the zero map is full): the fresh context's legs take the kernels without d; none does during the walk;
    behind step 9 the count grows again"""
    c, L = 7, 5
    N = _n(c, L)
    u, d = np.random.default_rng(N).standard_normal(N ** 3), np.zeros(N ** 3)

    def cycles(s):
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        s.vcycles(2)
        s.vcycle()
        return s.dnone_launches()

    with M.Solver(c, L, 2) as s:
        for key, value in (("legs_min", 66), ("carry_min", 66), ("legs", 1), ("carry", 0)):  # as tests/test_gpu_dnone.py
            s.set_option(key, value)
        s.get_details()
        fresh = cycles(s)
        assert fresh > 0
        for step, held in _walk(s, form, "dirichlet", N):
            if step != "constant":
                assert cycles(s) == fresh, step
        assert not (s.has_coefficient() or s.has_mask() or s.has_shift_field() or s.periodic or s.neumann)
        assert cycles(s) > fresh
