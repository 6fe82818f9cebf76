/*
 * mg3d_pcg.hip -- conjugate gradients preconditioned by the context's own V-cycle (mg3d_pcg_solve, include/mg3d.h).
 *
 * The cycle is a symmetric preconditioner: red,black before and black,red behind the coarse correction, the restriction
 * 1/8 of the prolongation's transpose, every level's operator symmetric (arithmetic face means), a zero guess below the
 * finest level.  A is negative definite, so CG runs on -A; carried through, every quantity below is the library's own:
 *     r = d - A x                z = one V-cycle from u = 0 with right-hand side r   (z ~ A^-1 r)
 *     alpha = (r.z)/(p.Ap)       x += alpha p,  r -= alpha Ap                        (both dots negative)
 *     beta = (r.z)_new/(r.z)_old p = z + beta p                                      (Fletcher-Reeves)
 *
 * Where the vectors live.  x is the finest level's u itself and d is never written: for the length of a solve the level's
 * u and d POINTERS are exchanged for two work vectors, z and r, so that the context's own cycle code
 * (mg3d_enqueue_vcycle, whatever schedule its options select) reads r as its right-hand side and leaves z where it keeps
 * u -- the fused schedules exchange u and the level's second buffer as they go, so z is whatever the level calls u when the
 * cycle returns.  The pointers are put back on every way out.  The caller's Dirichlet faces of u and every bit of d are
 * therefore untouched by construction, not by copying back.  p and q = Ap are two more work vectors; Dirichlet faces of
 * z, r, p, q are zero from their allocation (z is cleared before every cycle) and no pass writes them.
 *
 * Per iteration (kernels in mg3d_kernels.hip, byte counts in DESIGN.md):
 *     apply + dot      q = A p, p.q                    one pass
 *     update + norm    x += alpha p, r -= alpha q, r.r one pass; alpha from the two device scalars
 *     <one 32-byte copy to the host: p.q, r.z, r.r -- stop on the norm or on breakdown>
 *     clear z, V-cycle
 *     dot              r.z                             light pass
 *     direction        p = z + beta p                  light pass; beta from the two device scalars
 * The scalars are slots of the context's sumsq array; nothing but the one copy per iteration crosses to the host.
 */
#include "mg3d_ctx.h"

#include <math.h>

#define fail mg3d_fail
#define HIPCHK(call)                                                                                    \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(MG3D_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                                      \
    } while (0)
#define CHK(call)           \
    do {                    \
        int rc_ = (call);   \
        if (rc_ != MG3D_OK) \
            return rc_;     \
    } while (0)

/* slots of ctx->sumsq: 0 the initial residual, 1 the norm the cycle computes of its own system (dropped) */
enum { S_R0 = 0, S_CYCLE = 1, S_RZ = 2 /* and 3: this iteration's and the next one's */, S_PAP = 4, S_RR = 5, S_END = 6 };
enum { V_Z = 0, V_R, V_P, V_Q };

static int pcg_alloc(mg3d_ctx *ctx)
{
    const Level &top = ctx->lv[ctx->L - 1];
    if (ctx->pcg_v[0])
        return MG3D_OK;
    double *v[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int t = 0; t < 4; t++) {
        hipError_t e = hipMalloc(&v[t], top.elems * sizeof(double));
        if (e == hipSuccess)
            e = hipMemsetAsync(v[t], 0, top.elems * sizeof(double), ctx->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(ctx->stream);
            for (double *w : v)
                if (w)
                    (void)hipFree(w);
            return fail(e == hipErrorOutOfMemory ? MG3D_ERR_ALLOC : MG3D_ERR_HIP, "mg3d_pcg_solve: work vectors: %s",
                        hipGetErrorString(e));
        }
    }
    for (int t = 0; t < 4; t++)
        ctx->pcg_v[t] = v[t];
    return MG3D_OK;
}

static int pcg_launch_ok(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(MG3D_ERR_HIP, "mg3d_pcg_solve: %s: kernel launch failed: %s", what, hipGetErrorString(e));
    return MG3D_OK;
}

/* the iterations, with z and r standing in for u and d of the top level (the caller exchanges and restores the pointers) */
static int pcg_iterate(mg3d_ctx *ctx, double *x, double target, int max_iters, double *norms, int &iters, int &converged,
                       double &r_norm)
{
    Level &top = ctx->lv[ctx->L - 1];
    const int q = ctx->L - 1, bc = mg3d_ctx_bc(ctx);
    const double *e = ctx->eps.empty() ? nullptr : ctx->eps[q];
    const LevelOp op = mg3d_op(ctx, top);
    hipStream_t s = ctx->stream;
    double *const sc = ctx->sumsq, *const r = ctx->pcg_v[V_R], *const p = ctx->pcg_v[V_P], *const qv = ctx->pcg_v[V_Q];
    for (int k = 0;; k++) {
        /* z = V(r): the cycle starts from u = 0 on the top level too (faces included: the error's Dirichlet values) */
        HIPCHK(hipMemsetAsync(top.f[MG3D_U], 0, top.elems * sizeof(double), s));
        CHK(mg3d_enqueue_vcycle(ctx, q, S_CYCLE, 0));
        ctx->red_tail = false; /* u and d of the top level change under the next cycle */
        const double *z = top.f[MG3D_U];
        double *const rz = sc + S_RZ + (k & 1), *const rz_old = sc + S_RZ + ((k + 1) & 1);
        if (k_pcg_dot(top.g, bc, r, z, ctx->partials, rz, s) < 0)
            return fail(MG3D_ERR_STATE, "mg3d_pcg_solve: the level has no launch shape");
        if (k == 0)
            HIPCHK(hipMemcpyAsync(p, z, top.elems * sizeof(double), hipMemcpyDeviceToDevice, s)); /* p = z */
        else
            k_pcg_direction(top.g, bc, p, z, rz, rz_old, s);
        k_pcg_apply_dot(top.g, p, e, op, ctx->sigma, bc, qv, ctx->partials, sc + S_PAP, s);
        k_pcg_update_norm(top.g, bc, x, r, p, qv, rz, sc + S_PAP, ctx->partials, sc + S_RR, s);
        CHK(pcg_launch_ok("iteration"));
        HIPCHK(hipMemcpyAsync(ctx->h_sumsq + S_RZ, sc + S_RZ, (S_END - S_RZ) * sizeof(double), hipMemcpyDeviceToHost, s));
        CHK(mg3d_sync(ctx));
        const double h_rz = ctx->h_sumsq[S_RZ + (k & 1)], h_pap = ctx->h_sumsq[S_PAP];
        if (!(h_rz < 0. && isfinite(h_rz) && h_pap < 0. && isfinite(h_pap)))
            return MG3D_OK; /* breakdown: the update kernel saw the same numbers and wrote nothing */
        r_norm = sqrt(ctx->h_sumsq[S_RR]);
        iters = k + 1;
        if (norms)
            norms[iters] = r_norm;
        if (r_norm <= target) {
            converged = 1;
            return MG3D_OK;
        }
        if (iters >= max_iters)
            return MG3D_OK;
    }
}

extern "C" int mg3d_pcg_solve(mg3d_ctx *ctx, double rtol, double atol, int max_iters, double *norms, mg3d_pcg_info *info)
{
    if (!ctx)
        return fail(MG3D_ERR_ARG, "mg3d_pcg_solve: NULL context");
    if (!(rtol >= 0.) || !(atol >= 0.) || !isfinite(rtol) || !isfinite(atol) || max_iters < 0)
        return fail(MG3D_ERR_ARG, "mg3d_pcg_solve: rtol and atol must be finite and >= 0, max_iters >= 0 (%g, %g, %d)", rtol,
                    atol, max_iters);
    if (rtol == 0. && atol == 0. && max_iters == 0)
        return fail(MG3D_ERR_ARG, "mg3d_pcg_solve: rtol = atol = 0 needs max_iters > 0");
    if (ctx->neumann)
        return fail(MG3D_ERR_STATE, "mg3d_pcg_solve: the context has Neumann faces (mg3d_ctx_set_neumann): the reflected "
                                    "operator is not symmetric in the Euclidean inner product");
    if (ctx->periodic && mg3d_ctx_pinned(ctx))
        return fail(MG3D_ERR_STATE, "mg3d_pcg_solve: every axis periodic with sigma = 0 is singular: the pinned row of the "
                                    "coarse matrix makes the cycle an unsymmetric preconditioner");
    if (ctx->have_es)
        return fail(MG3D_ERR_STATE, "mg3d_pcg_solve: the context holds the mixed-boundary factor of mg3d_es_setup");
    if (!ctx->have_lu)
        return fail(MG3D_ERR_STATE, "mg3d_pcg_solve: no coarse LU set (mg3d_ctx_build_coarse / mg3d_ctx_set_lu)");
    CHK(mg3d_drop_carry(ctx)); /* a cycle that has run ahead is finished first */
    const int q = ctx->L - 1, bc = mg3d_ctx_bc(ctx);
    Level &top = ctx->lv[q];
    const double *e = ctx->eps.empty() ? nullptr : ctx->eps[q];
    hipStream_t s = ctx->stream;
    if (max_iters > 0)
        CHK(pcg_alloc(ctx));
    /* r_0 = d - A x; with iterations to come it is stored as the first right-hand side of the cycle */
    k_residual(top.g, top.f[MG3D_U], e, top.f[MG3D_D], mg3d_op(ctx, top), ctx->sigma, bc,
               max_iters > 0 ? ctx->pcg_v[V_R] : nullptr, ctx->partials, ctx->sumsq + S_R0, s);
    CHK(pcg_launch_ok("initial residual"));
    HIPCHK(hipMemcpyAsync(ctx->h_sumsq + S_R0, ctx->sumsq + S_R0, sizeof(double), hipMemcpyDeviceToHost, s));
    CHK(mg3d_sync(ctx));
    const double r0 = sqrt(ctx->h_sumsq[S_R0]);
    int iters = 0, converged = 0;
    double r_norm = r0;
    if (norms)
        norms[0] = r0;
    int rc = MG3D_OK;
    const double target = fmax(rtol * r0, atol);
    if (r0 == 0. || (max_iters > 0 && r0 <= target)) {
        converged = 1;
    } else if (max_iters > 0) {
        /* The faces of a coarse right-hand side are an injection of the faces of r of the level above (faces_dirty), which
         * no cycle writes: cleared, so that the cycle is the linear map the method needs whatever r held */
        for (int l = 0; l <= q; l++) {
            HIPCHK(hipMemsetAsync(ctx->lv[l].f[MG3D_R], 0, ctx->lv[l].elems * sizeof(double), s));
            mg3d_ctx_touched(ctx, MG3D_R, l);
        }
        double *const x = top.f[MG3D_U], *const d = top.f[MG3D_D];
        top.f[MG3D_U] = ctx->pcg_v[V_Z];
        top.f[MG3D_D] = ctx->pcg_v[V_R];
        rc = pcg_iterate(ctx, x, target, max_iters, norms, iters, converged, r_norm);
        if (rc != MG3D_OK)
            (void)hipStreamSynchronize(s);
        (void)mg3d_drop_carry(ctx);
        ctx->pcg_v[V_Z] = top.f[MG3D_U]; /* the fused schedules exchange u and the level's second buffer */
        top.f[MG3D_U] = x;
        top.f[MG3D_D] = d;
        if (rc == MG3D_OK && ctx->periodic) {
            k_per_refresh(top.g, x, bc, s); /* the passes write unique points only */
            rc = pcg_launch_ok("duplicate refresh");
        }
        if (rc == MG3D_OK)
            rc = mg3d_sync(ctx);
    }
    if (info) {
        info->iterations = iters;
        info->converged = converged;
        info->r0_norm = r0;
        info->r_norm = r_norm;
    }
    return rc;
}
