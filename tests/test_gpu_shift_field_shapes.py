"""The SFIELD = true instantiations of csrc/mg3d_kernels.hip (the screening field, mg3d_ctx_set_shift_field) at the launch
shapes tests/test_gpu_shift_field.py never reaches, against the numpy restatement tests/_shift_field_ref.py -- the shapes
tests/test_gpu_mask_shapes.py established for the column kernels: a second 64-lane block in k, a partial last 4-row block
in j and a short last chunk in i.

    65_f63          65^3, Neumann faces all round: ONE live lane, row and plane in the last blocks
    73_eps          73^3, eps, off the ladder, with a mask (the form that takes the field AND the bytes)
    81_per7         81^3, every axis periodic: the unknowns start at 0
    81_per4_f3_eps  81^3, periodic k, Neumann i faces, eps, with a mask

Per case, with a random field in [0, 1/h^2] -- a field read at a wrong offset changes bits (test_the_reference_sees_every_tail)
--: one residual, one colour pass of each colour, one A p through a one-iteration PCG; and once, at 73^3, the check, pack,
refresh and restriction kernels from strided float64 and float32 device arrays at two k-blocks.  The unmarked test asserts
from column_grid()'s arithmetic that each case has the shape claimed.  No 513^3 case: the cap of partial sums is a property
of the shared column walk and column_grid(), which tests/test_gpu_stencil_shapes.py, test_gpu_neumann_shapes.py and
test_gpu_mask_shapes.py cover past the cap; the field adds one load at the point's own offset and no shape of its own.

Grid values bit for bit with sign bits; norms against the exactly rounded sum at norm_rtol(N) of tests/test_gpu_parity.py.
The iterate after the one PCG iteration is held to 100 x the summation spread, never below the figure
tests/test_gpu_pcg.py / test_gpu_wpcg.py hold the same call to.  The spreads of the four cases (python
tests/test_gpu_shift_field_shapes.py: two restatement runs, exactly rounded dots against numpy's pairwise sums):
                     u, k = 1    norms
    65_f63           0.00e+00    0.00e+00
    73_eps           0.00e+00    0.00e+00
    81_per7          0.00e+00    1.21e-16
    81_per4_f3_eps   0.00e+00    0.00e+00
(after ONE iteration of this strongly screened operator the two runs agree to the bit in all but one norm), all below the
existing files' figures, which therefore govern."""
import numpy as np
import pytest
import torch  # before the package, as bench.py does: the HIP runtime is torch's

import _coef_ref as CR
import _mask_ref as MR
import _neumann_ref as NR
import _oracle as O
import _shift_field_ref as SF
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_D, MG3D_R, MG3D_U

from test_gpu_mask_shapes import regions
from test_gpu_neumann_shapes import launch_shape
from test_gpu_parity import norm_rtol
from test_gpu_stencil_shapes import _max_partials

gpu = pytest.mark.gpu

# name -> (c, L, sigma, eps, axes, faces, masked) and what launch_shape gives: unknowns per axis (k, j, i), live lanes of
# the last k-block, live rows of the last row block, planes of the last chunk
CASES = {
    "65_f63": (9, 4, 0.0, None, 0, 63, False),
    "73_eps": (10, 4, 0.0, "exp", 0, 0, True),
    "81_per7": (11, 4, 3.5, None, 7, 0, False),
    "81_per4_f3_eps": (11, 4, 0.0, "exp", 4, 3, True),
}
SHAPES = {"65_f63": ((65, 65, 65), 1, 1, 1), "73_eps": ((71, 71, 71), 7, 3, 7),
          "81_per7": ((80, 80, 80), 16, 4, 16), "81_per4_f3_eps": ((80, 79, 81), 16, 3, 1)}
# measured, see the table above: the largest over the four cases
SPREAD_U = {1: 0.0}
SPREAD_NORM = 1.21e-16


def _same_bits(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def _n(c, L):
    return O.level_sizes(c, L)[-1]


def _problem(name):
    """(eps, mask, field, u, d) of a case: random data, duplicates consistent"""
    c, L, _, coef, axes, faces, masked = CASES[name]
    N = _n(c, L)
    eps = None
    if coef is not None:
        eps = CR.FIELDS[coef](N)
        NR.refresh(eps, axes)
    mask = MR.gpu_test_mask(N) if masked else None
    field = SF.random_field(N, 1.0 / (N - 1), seed=N)
    rng = np.random.default_rng(N + faces)
    u, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    NR.refresh(u, axes)
    NR.refresh(d, axes)
    return eps, mask, field, u, d


def _solver(name, eps, mask, field, factor):
    c, L, sigma, _, axes, faces, _ = CASES[name]
    s = M.Solver(c, L, 2)
    s.set_shift(sigma)
    s.set_periodic(axes)
    s.set_neumann(faces)
    if eps is not None:
        s.set_coefficient(eps)
    if mask is not None:
        s.set_mask(mask)
    s.set_shift_field(field)
    if factor:
        s.get_details()
    return s


# ------------------------------------------------------------------------------------- 1 geometry, without a GPU
def test_the_cases_reach_the_shapes():
    """launch_shape() -- column_grid() of the library restated from the header's MG3D_MAX_PARTIALS -- gives every case the
    shape its line in the module docstring claims: two k-blocks, chunks of 16 planes, the tails of SHAPES"""
    assert _max_partials() == 32768
    assert [_n(c, L) for c, L, *_ in CASES.values()] == [65, 73, 81, 81]
    for name, (c, L, _, _, axes, faces, _) in CASES.items():
        N = _n(c, L)
        sh = launch_shape(N, axes, faces)
        unknowns = tuple(NR.lo_hi(N, axes, faces, ax)[1] + 1 - NR.lo_hi(N, axes, faces, ax)[0] for ax in (2, 1, 0))
        assert (unknowns, sh["lanes"], sh["rows"], sh["last"]) == SHAPES[name], (name, unknowns, sh)
        assert sh["gx"] == 2 and sh["chunk"] == 16 and sh["gz"] >= 5 and sh["partials"] <= _max_partials()


@pytest.mark.parametrize("name", ["65_f63", "73_eps"])
def test_the_reference_sees_every_tail(name):
    """with the field of one tail alone changed -- the last k-block, the last row block, the last chunk, the first unknowns,
    the Neumann faces --, the restated colour pass (each colour) and residual give other bits there: a kernel that read the
    field at a wrong offset in that tail, or not at all, would not pass the GPU tests below"""
    c, L, sigma, _, axes, faces, _ = CASES[name]
    N = _n(c, L)
    eps, mask, field, u, d = _problem(name)
    h = 1.0 / (N - 1)
    f = SF.stored(field, axes)

    def run(fld):
        out = []
        for colour in (1, 0):
            v = u.copy()
            SF.colour_pass(v, d, eps, h, sigma, axes, faces, colour, mask, fld)
            out.append(v)
        r = np.zeros((N, N, N))
        SF.residual(u, d, eps, h, sigma, axes, faces, mask, fld, r)
        return out + [r]

    base = run(f)
    for where, reg in regions(N, axes, faces).items():
        other = f.copy()
        other[reg] = other[reg] * 0.5 + 1.0
        for what, a, b in zip(("red pass", "black pass", "residual"), base, run(other)):
            assert not np.array_equal(a[reg], b[reg]), (where, what)
            assert _same_bits(a[~reg], b[~reg]), (where, what)


# ------------------------------------------------------------------------------------------------ 2 single operators
@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_single_operators(name):
    """one residual (r stored) and one colour pass of each colour on the finest level, random u and d"""
    c, L, sigma, _, axes, faces, _ = CASES[name]
    N = _n(c, L)
    eps, mask, field, u, d = _problem(name)
    f = SF.stored(field, axes)
    with _solver(name, eps, mask, field, factor=False) as s:
        h = s.level_h(L - 1)
        assert _same_bits(s.get_shift_field(L - 1), f)
        s.upload(MG3D_U, L - 1, u)
        s.upload(MG3D_D, L - 1, d)
        r = np.zeros((N, N, N))
        s.zero(MG3D_R, L - 1)
        got = s.residual(L - 1, store=True)
        SF.residual(u, d, eps, h, sigma, axes, faces, mask, f, r)
        assert _same_bits(s.download(MG3D_R, L - 1), r)
        exact = SF.exact_residual_norm(u, d, eps, h, sigma, axes, faces, mask, f)
        assert abs(got - exact) <= norm_rtol(N) * exact, (got, exact)
        s.smooth(L - 1, 0, 1)  # red, then black
        for colour in (1, 0):
            SF.colour_pass(u, d, eps, h, sigma, axes, faces, colour, mask, f)
        assert _same_bits(s.download(MG3D_U, L - 1), u)
        s.smooth(L - 1, 1, 1)  # black, then red: each colour once more, on other data
        for colour in (0, 1):
            SF.colour_pass(u, d, eps, h, sigma, axes, faces, colour, mask, f)
        assert _same_bits(s.download(MG3D_U, L - 1), u)


# ------------------------------------------------------------------------------------------- 3 A p through one iteration
def _tolerances(call):
    import test_gpu_pcg as TP
    import test_gpu_wpcg as TW
    f = TW if call == "wpcg_solve" else TP
    return 100 * max(SPREAD_U[1], f.SPREAD_U[1]), 100 * max(SPREAD_NORM, f.SPREAD_NORM)


def _make(name, eps, mask, field):
    c, L, sigma, _, axes, faces, _ = CASES[name]
    return lambda: SF.Hierarchy(c, L, 2, sigma, eps, axes, faces, mask, field)


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_one_pcg_iteration(name):
    """q = A p of the SFIELD apply kernel, through the iterate and the two norms of one iteration from a random x0:
    mg3d_pcg_solve, mg3d_wpcg_solve where a face is a Neumann face"""
    c, L, sigma, _, axes, faces, _ = CASES[name]
    N = _n(c, L)
    call = "wpcg_solve" if faces else "pcg_solve"
    eps, mask, field, x0, d = _problem(name)
    prob = _make(name, eps, mask, field)()
    assert not prob.is_singular()
    hist = []
    _, ref_norms, _, _, _ = SF.wpcg(prob, x0, d, 0., 1e-300, 1, "exact", hist)
    with _solver(name, eps, mask, field, factor=True) as s:
        s.upload(MG3D_U, L - 1, x0)
        s.upload(MG3D_D, L - 1, d)
        norms, info = getattr(s, call)(rtol=0.0, atol=1e-300, max_iters=1)
        assert info["iterations"] == 1 and len(norms) == 2
        u = s.download(MG3D_U, L - 1).reshape(N, N, N)
    rel = np.abs(u - hist[0]).max() / np.abs(hist[0]).max()
    nrel = (np.abs(norms - ref_norms[:2]) / ref_norms[:2]).max()
    tol_u, tol_n = _tolerances(call)
    print(name, call, "u", rel, "of", tol_u, "norms", nrel, "of", tol_n)
    assert rel <= tol_u and nrel <= tol_n


# ------------------------------------------------------------------------------------- 4 the device form at two k-blocks
@gpu
def test_device_form_from_strided_arrays():
    """73^3, periodic i and k: the check, the pack, the duplicate refresh and the restrictions from a sliced float64 view, a
    permuted one and a float32 tensor: the host form's bytes on every level; a bad entry in the second k-block of the last
    row is found through the strides"""
    c, L, axes = 19, 3, 5
    N = _n(c, L)
    assert N == 73 and launch_shape(N, axes, 0)["gx"] == 2
    dev = torch.device("cuda:0")
    field = SF.random_field(N, 1.0 / (N - 1), seed=4)
    f32 = field.astype(np.float32)
    t = torch.from_numpy(field).to(dev)
    big = torch.full((2 * N, N + 3, N + 2), -1.0, dtype=torch.float64, device=dev)
    big[::2, 2:N + 2, 1:N + 1] = t
    views = {"sliced": (field, big[::2, 2:N + 2, 1:N + 1]),
             "permuted": (field, t.permute(2, 0, 1).contiguous().permute(1, 2, 0)),
             "float32": (f32.astype(np.float64), torch.from_numpy(f32).to(dev))}
    with M.Solver(c, L, 2) as s:
        s.set_periodic(axes)
        for name, (host, tensor) in views.items():
            s.set_shift_field_tensor(tensor)
            want = SF.restrict_field(host, L, axes, 0)
            for l in range(L):
                assert _same_bits(s.get_shift_field(l), want[l]), (name, l)
        kept = [s.get_shift_field(l) for l in range(L)]
        big[2 * (N - 2), 2 + N - 1, 1 + 70] = float("nan")
        big[2 * (N - 2), 2 + N - 1, 1 + 71] = -3.0
        with pytest.raises(M.Mg3dError) as ei:
            s.set_shift_field_tensor(big[::2, 2:N + 2, 1:N + 1])
        assert ei.value.code == 1 and f"s[{((N - 2) * N + N - 1) * N + 70}] = nan" in str(ei.value), str(ei.value)
        for l in range(L):
            assert _same_bits(s.get_shift_field(l), kept[l])


def spread_table():
    out = {}
    for name in CASES:
        eps, mask, field, x0, d = _problem(name)
        out[name] = SF.spread(_make(name, eps, mask, field), x0, d, (1,))
    return out


if __name__ == "__main__":
    for name, (u, n) in spread_table().items():
        print(f"{name:16s} {u[0]:.2e}    {n:.2e}")
