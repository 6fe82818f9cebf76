"""The numpy references pinned to each other without a GPU, at coarse grids off the 2^k+1 ladder (c - 1 not a power of 2):
tests/_periodic_ref.py with mask 0 is tests/_screened_ref.py (eps None) and tests/_coef_ref.py bit for bit -- the single
operators and two V-cycles on every level -- and its blockwise colour pass and residual (the form the 513^3 and 577^3 GPU
tests need to keep host memory bounded) are its whole-array functions bit for bit on every mask."""
import numpy as np
import pytest

import _coef_ref as CR
import _oracle as O
import _periodic_ref as R
import _screened_ref as S

COARSE = [6, 7, 10, 11]


def _same_bits(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _eps(field, N):
    return None if field is None else CR.FIELDS[field](N)


def _dirichlet_ref(e):
    """the mask-0 twin of R's functions: _screened_ref without eps, _coef_ref with it"""
    if e is None:
        return (lambda u, d, h, s, n: S.pre_smooth(u, d, h, s, n), lambda u, d, h, s, n: S.post_smooth(u, d, h, s, n),
                lambda u, d, h, s, r: S.residual(u, d, h, s, r))
    return (lambda u, d, h, s, n: CR.pre_smooth(u, d, e, h, s, n), lambda u, d, h, s, n: CR.post_smooth(u, d, e, h, s, n),
            lambda u, d, h, s, r: CR.residual(u, d, e, h, s, r))


@pytest.mark.parametrize("c", COARSE)
@pytest.mark.parametrize("field", [None, "smooth", "exp"])
@pytest.mark.parametrize("sigma", [0.0, 1e3])
def test_mask_0_single_operators(c, field, sigma):
    """pre_smooth, post_smooth, residual with r, restrict and prolong of the top level of a 3-level hierarchy"""
    L = 3
    N, Nc = O.level_sizes(c, L)[-1], O.level_sizes(c, L)[-2]
    h = 1.0 / (N - 1)
    e = _eps(field, N)
    pre, post, res = _dirichlet_ref(e)
    rng = np.random.default_rng(100 * c + (field is None) + int(sigma))
    u, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    a, b = u.copy(), u.copy()
    R.pre_smooth(a, d, e, h, sigma, 0, 2)
    pre(b, d, h, sigma, 2)
    assert _same_bits(a, b), "pre-smoothing"
    R.post_smooth(a, d, e, h, sigma, 0, 3)
    post(b, d, h, sigma, 3)
    assert _same_bits(a, b), "post-smoothing"
    ra, rb = np.zeros((N, N, N)), np.zeros((N, N, N))
    na = R.residual(a, d, e, h, sigma, 0, ra)
    nb = res(b, d, h, sigma, rb)
    assert _same_bits(ra, rb) and na == nb, "residual"
    ra = rng.standard_normal((N, N, N))
    dc, want = rng.standard_normal((Nc, Nc, Nc)), np.zeros(Nc ** 3)
    R.restrict(ra, dc, 0)
    O.lib().orc_restrict(O.P(ra.reshape(-1)), N, O.P(want), Nc)
    assert _same_bits(dc.reshape(-1), want), "restrict"
    ec = rng.standard_normal((Nc, Nc, Nc))
    want = u.reshape(-1).copy()
    R.prolong(ec, u, 0)
    O.lib().orc_prolong(O.P(ec.reshape(-1)), Nc, O.P(want), N)
    assert _same_bits(u.reshape(-1), want), "prolong"


@pytest.mark.parametrize("c", COARSE)
@pytest.mark.parametrize("field", [None, "smooth", "exp"])
@pytest.mark.parametrize("sigma", [0.0, 1e3])
def test_mask_0_vcycles(c, field, sigma):
    """two V(2,2) cycles of a 3-level Problem from a random start: u, d and r of every level, and the norms"""
    L, nu = 3, 2
    N = O.level_sizes(c, L)[-1]
    eps = _eps(field, N)
    ref = R.Problem(c, L, nu, sigma, eps, 0)
    want = CR.Problem(c, L, nu, sigma, eps)
    rng = np.random.default_rng(7 * c)
    for p in (ref, want):
        p.u[-1][...] = rng.standard_normal((N, N, N)) if p is ref else ref.u[-1]
        p.d[-1][...] = rng.standard_normal((N, N, N)) if p is ref else ref.d[-1]
    got, exp = ref.vcycles(2), want.vcycles(2)
    assert _same_bits(got, exp), (got, exp)
    for f in ("u", "d", "r"):
        for l in range(L):
            assert _same_bits(ref.flat(f, l), want.flat(f, l)), f"{f} level {l}"


@pytest.mark.parametrize("axes", range(8))
@pytest.mark.parametrize("field", [None, "exp"])
@pytest.mark.parametrize("planes", [1, 5])
def test_blockwise_equals_whole_array(axes, field, planes):
    """colour_pass_blocks (both colours) and residual_blocks at 13^3 against colour_pass and residual: every point bit
    for bit, duplicates included (random values at the duplicates going in); the norm against the exactly rounded one"""
    N, sigma = 13, 1e3
    h = 1.0 / (N - 1)
    e = _eps(field, N)
    rng = np.random.default_rng(axes + 8 * planes)
    u, d = rng.standard_normal((N, N, N)), rng.standard_normal((N, N, N))
    a, b = u.copy(), u.copy()
    for colour in (1, 0, 0, 1):
        R.colour_pass(a, d, e, h, sigma, axes, colour)
        R.colour_pass_blocks(b, d, e, h, sigma, axes, colour, planes)
        assert _same_bits(a, b), f"colour {colour}"
    ra = rng.standard_normal((N, N, N))
    rb = ra.copy()
    R.residual(a, d, e, h, sigma, axes, ra)
    got = R.residual_blocks(b, d, e, h, sigma, axes, rb, planes)
    assert _same_bits(ra, rb)
    want = R.exact_residual_norm(a, d, e, N, h, sigma, axes)
    assert got == pytest.approx(want, rel=1e-15)
