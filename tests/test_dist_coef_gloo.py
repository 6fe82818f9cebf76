"""World-size-2 and -3 run of the i-slab V-cycle with a variable coefficient (mg3d_dist_set_coefficient) on CPU: real
processes, torch.distributed `gloo`, every transfer read from the PRODUCT's plain exchange plan (mg3d_dist_plan, policy 0
or 1) by test_dist_gloo.PlanRunner.

What is under test is the halo and window argument of the coefficient cycle in csrc/mg3d_dist.hip (dist_coef_smooth):
with H = 2*nu + 2 exact halo planes on entry, pass t of S = 2*nu colour passes only has to produce the owned planes
+- (margin + S - t) -- margin 2 before the stored residual, 1 before the top-level norm -- the residual r only owned +- 1,
and the norm only the owned planes.  Every plane outside those windows is poisoned with NaN before the next exchange
refreshes it: the assembled u must still equal the whole-domain numpy reference (tests/_coef_ref.py) bit for bit.  The
per-slab arithmetic is _coef_ref's stencil on a window of planes, colours by global index; the replicated levels run
_coef_ref.Problem.  No GPU, no HIP compute."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _coef_ref as R
import _plan as PL
import _slab_numpy as S
import multigrid_parallel_amd as M
from test_dist_gloo import PlanRunner, Slab, free_port, owned


def _rows(ni, ig0, N, i_lo, i_hi):
    """interior local planes [lo, hi] (inclusive) of the window [i_lo, i_hi), as k_smooth_color / k_residual clip it"""
    lo = max(1, 1 - ig0, i_lo)
    hi = min(ni - 2, N - 2 - ig0, i_hi - 1)
    return lo, hi


def colour_pass(u, d, e, h, sigma, colour, ig0, N, i_lo, i_hi):
    """coef_color_kernel<false> on the local planes [i_lo, i_hi) of a slab (colour 1 = red, by GLOBAL index)"""
    lo, hi = _rows(u.shape[0], ig0, N, i_lo, i_hi)
    if hi < lo:
        return
    hSq = h * h
    s, dg = R._sum_diag(u[lo - 1:hi + 2], e[lo - 1:hi + 2], sigma * hSq)
    new = (s - hSq * d[lo:hi + 1, 1:-1, 1:-1]) / dg
    ii = (np.arange(lo, hi + 1) + ig0)[:, None, None]
    jj = np.arange(1, N - 1)[None, :, None]
    kk = np.arange(1, N - 1)[None, None, :]
    mask = ((ii + jj + kk) & 1) == colour
    u[lo:hi + 1, 1:-1, 1:-1][mask] = new[mask]


def residual(u, d, e, h, sigma, r, ig0, N, i_lo, i_hi, acc_lo, acc_hi):
    """residual_kernel<true, false>: r (optional) on the window, returns sum diff^2 over the local planes [acc_lo, acc_hi)"""
    lo, hi = _rows(u.shape[0], ig0, N, i_lo, i_hi)
    if hi < lo:
        return 0.0
    hSq = h * h
    s, dg = R._sum_diag(u[lo - 1:hi + 2], e[lo - 1:hi + 2], sigma * hSq)
    diff = d[lo:hi + 1, 1:-1, 1:-1] - (1.0 / hSq) * (s - dg * u[lo:hi + 1, 1:-1, 1:-1])
    if r is not None:
        r[lo:hi + 1, 1:-1, 1:-1] = diff
    a, b = max(lo, acc_lo), min(hi + 1, acc_hi)
    return float((diff[a - lo:b - lo] ** 2).sum()) if b > a else 0.0


def smooth(sl, h, sigma, nu, post, margin):
    """2*nu passes, pass t producing owned +- (margin + S - t) only"""
    S2 = 2 * nu
    c1 = 0 if post else 1
    for t in range(1, S2 + 1):
        w = margin + S2 - t
        colour_pass(sl.u, sl.d, sl.e, h, sigma, c1 ^ ((t - 1) & 1), sl.ig0, sl.N, sl.own_lo - w, sl.own_hi + w)


def poison(a, sl, w):
    """NaN on every local plane outside owned +- w: what the windows leave stale"""
    a[:max(0, sl.own_lo - w)] = np.nan
    a[sl.own_hi + w:] = np.nan


def worker(r, P, port, c, L, nu, sigma, field, cycles, out_path, policy):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=r, world_size=P)
    lib = M.lib()
    H = lib.mg3d_slab_halo(nu)
    ld = lib.mg3d_slab_first_level(c, L, P, H)
    ref = R.Problem(c, L, nu, sigma, None)  # geometry and spacings of the whole domain
    Nf = ref.N[-1]
    hs = [ref.h * (1 << (L - 1 - l)) for l in range(L)]
    es = R.inject(R.FIELDS[field](Nf), L)
    lv = {l: Slab(c, L, P, H, l, r) for l in range(ld, L)}
    for l, sl in lv.items():
        sl.e = np.ascontiguousarray(es[l][sl.ig0:sl.ig0 + sl.ni])  # eps of every local plane, halos included
    rep = R.Problem(c, ld, nu, sigma, es[ld - 1])  # the replicated levels 0 .. ld-1 (coarse factor from level 0's eps)
    Ncr = rep.N[-1]
    ref.setup_test_problem()
    top = lv[L - 1]
    top.u[:] = ref.u[-1][top.ig0:top.ig0 + top.ni]
    top.d[:] = ref.d[-1][top.ig0:top.ig0 + top.ni]
    norms = []
    plan = PlanRunner(c, L, P, nu, r, policy)

    def array_of(fld, level):
        if level >= ld:
            return getattr(lv[level], "ud"[fld])
        return (rep.u if fld == 0 else rep.d)[level]

    for _ in range(cycles):
        plan.start_cycle()  # the plain plan: never carried, never legs
        for l in range(L - 1, ld - 1, -1):  # ---- down (dist_down_leg, its coefficient form)
            sl = lv[l]
            if l < L - 1:
                sl.u[:] = 0.0
            smooth(sl, hs[l], sigma, nu, False, 2)
            poison(sl.u, sl, 2)  # the residual reads u on owned +- 2 only
            poison(sl.r, sl, 1)  # the restriction reads r on owned +- 1 only
            residual(sl.u, sl.d, sl.e, hs[l], sigma, sl.r, sl.ig0, sl.N, sl.own_lo - 1, sl.own_hi + 1, 0, 0)
            if l - 1 >= ld:
                sc = lv[l - 1]
                S.restrict_planes(sl.r, sl.ig0, sl.N, sc.d, sc.ig0, sc.N, sc.own_lo, sc.own_hi)
                plan.run(PL.HALO_D, l - 1, array_of)
            else:
                flo, fhi = owned(c, L, P, H, ld, r)
                S.restrict_planes(sl.r, sl.ig0, sl.N, rep.d[ld - 1], 0, Ncr, 0 if r == 0 else flo // 2,
                                  Ncr if r == P - 1 else fhi // 2)
                plan.run(PL.RHS_GATHER if policy else PL.RHS_ALLGATHER, ld - 1, array_of)
            plan.run(PL.HALO_U_DOWN, l, array_of)  # every halo plane of u, poisoned ones included
            assert not np.isnan(sl.u).any()
        if not policy or r == 0:  # ---- replicated levels (dist_replicated_levels)
            rep.u[ld - 1][...] = 0.0
            rep.vcycle(ld - 1, hs[ld - 1])
        else:
            rep.u[ld - 1][...] = np.nan  # must be overwritten by the broadcast
        if policy:
            plan.run(PL.CORR_BCAST, ld - 1, array_of)
        for l in range(ld, L):  # ---- up (dist_up_leg, its coefficient form)
            sl = lv[l]
            if l - 1 >= ld:
                sc = lv[l - 1]
                plan.run(PL.HALO_U_UP, l - 1, array_of)
                assert not np.isnan(sc.u).any()
                S.prolong_planes(sc.u, sc.ig0, sc.N, sl.u, sl.ig0, sl.N, 0, sl.ni)
            else:
                S.prolong_planes(rep.u[ld - 1], 0, Ncr, sl.u, sl.ig0, sl.N, 0, sl.ni)
            smooth(sl, hs[l], sigma, nu, True, 1)
            if l < L - 1:
                poison(sl.u, sl, 0)  # the next level up refreshes every halo plane of this correction first
        # the top level: planes 2..H come by exchange, plane 1 is the post-smoother's; the norm covers the owned planes
        poison(top.u, top, 1)
        plan.run(PL.HALO_U_NEXT, L - 1, array_of)
        assert not np.isnan(top.u).any()
        ss = residual(top.u, top.d, top.e, hs[L - 1], sigma, None, top.ig0, top.N, top.own_lo, top.own_hi,
                      top.own_lo, top.own_hi)
        parts = plan.run(PL.NORM, L - 1, array_of, norm_part=ss)
        assert plan.cur == len(plan.ph), "the cycle used every phase of the plan"
        norms.append(float(np.sqrt(sum(parts))))
    mine = torch.from_numpy(top.u[top.own_lo:top.own_hi].copy())
    if r == 0:
        u = np.zeros((Nf, Nf, Nf))
        u[top.glo:top.ghi] = mine.numpy()
        for q in range(1, P):
            lo, hi = owned(c, L, P, H, L - 1, q)
            t = torch.empty((hi - lo, Nf, Nf), dtype=torch.float64)
            dist.recv(t, q)
            u[lo:hi] = t.numpy()
        np.savez(out_path, u=u.reshape(-1), norms=np.array(norms))
    else:
        dist.send(mine, 0)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("c,L,nu,P,min_planes,policy,sigma,field", [
    (5, 5, 2, 2, 16, 0, 0.0, "exp"), (5, 5, 1, 2, 8, 0, 1e3, "ball"), (3, 6, 2, 3, 8, 0, 0.0, "smooth"),
    (3, 6, 3, 3, 16, 0, 1e3, "exp"), (5, 5, 3, 2, 8, 0, 0.0, "ball"),
    (5, 5, 2, 2, 16, 1, 1e3, "smooth"), (3, 6, 1, 3, 8, 1, 0.0, "exp")])
def test_coef_slab_schedule_over_gloo(tmp_path, monkeypatch, c, L, nu, P, min_planes, policy, sigma, field):
    monkeypatch.setenv("MG3D_SLAB_MIN_PLANES", str(min_planes))
    if ((c - 1) << (L - 1)) // P < max(min_planes, 2 * nu + 2):
        pytest.skip("no level gives every rank that many planes")
    cycles = 3
    out = str(tmp_path / "res.npz")
    mp.spawn(worker, args=(P, free_port(), c, L, nu, sigma, field, cycles, out, policy), nprocs=P, join=True)
    got = np.load(out)
    ref = R.Problem(c, L, nu, sigma, R.FIELDS[field](R.Problem(c, L, nu, sigma, None).N[-1]))
    ref.setup_test_problem()
    want = ref.vcycles(cycles)
    assert np.array_equal(got["u"], ref.u[-1].reshape(-1))
    np.testing.assert_allclose(got["norms"], want, rtol=1e-12)
