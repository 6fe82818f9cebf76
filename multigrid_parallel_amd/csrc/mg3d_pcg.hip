/*
 * mg3d_pcg.hip -- conjugate gradients preconditioned by the context's own V-cycle (mg3d_pcg_solve and mg3d_wpcg_solve,
 * include/mg3d.h).
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
 * z, r, p, q are zero from their allocation (z is cleared before every cycle) and no pass writes them.  Fixed points
 * (mg3d_ctx_set_mask) are Dirichlet points in the interior: the residual stores r = 0. there, the cycle never writes z
 * there, apply + dot stores q = 0. there, so p stays 0. and the update, dot and direction passes -- which do visit them --
 * move nothing: x keeps the caller's value (the update stores x + alpha*0. there: the same value, except that a -0. the
 * caller uploaded becomes +0.).
 *
 * Per iteration (kernels in mg3d_kernels.hip, byte counts in DESIGN.md):
 *     apply + dot      q = A p, p.q                    one pass
 *     update + norm    x += alpha p, r -= alpha q, r.r one pass; alpha from the two device scalars
 *     <one 32-byte copy to the host: p.q, r.z, r.r -- stop on the norm or on breakdown>
 *     clear z, V-cycle
 *     dot              r.z                             light pass
 *     direction        p = z + beta p                  light pass; beta from the two device scalars
 * The scalars are slots of the context's sumsq array; nothing but the one copy per iteration crosses to the host.
 *
 * mg3d_wpcg_solve (Neumann faces, the singular case) is the same iteration in the inner product sum of w*a*b, w = 1/2 per
 * Neumann face a point lies on: the reflected operator is self-adjoint in it, and so is the cycle -- red-black Gauss-Seidel
 * does not see a scaling of rows, and the reflected full weighting is W_c^-1 P^T W_f / 8.  r.z and p.Ap are weighted; the
 * norms stay Euclidean.  In the singular case (mg3d_ctx_pinned; W = sum of w) the system is solved on the subspace of
 * w-mean zero: r_0 has its w-mean taken out once, every z loses sum(w z)/W as it enters the direction -- the pinned coarse
 * solve differs from a symmetric pseudo-inverse by a constant only -- and r.z is that of the z the cycle returned, since
 * <r, 1>_w = 0.  Per iteration the passes are the four above: the dot returns sum(w z) from the same read of z, the
 * direction pass subtracts the mean and also forms the first direction (no copy).
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
/* the weighted solve's own, never copied inside an iteration: sum(w z); sum(w r_0), sum(w d); a sum nobody reads */
enum { S_WZ = S_END, S_WR, S_WD, S_DROP };
enum { V_Z = 0, V_R, V_P, V_Q };

/* the inner product of a solve: Euclidean (mg3d_pcg_solve), or weighted, with the projection of the singular case */
struct InnerProduct {
    bool weighted, singular;
    double W; /* sum of w over the unknowns */
};

static int pcg_alloc(mg3d_ctx *ctx, const char *name)
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
            return mg3d_alloc_fail(e, name, "work vectors");
        }
    }
    for (int t = 0; t < 4; t++)
        ctx->pcg_v[t] = v[t];
    return MG3D_OK;
}

static int pcg_launch_ok(const char *name, const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(MG3D_ERR_HIP, "%s: %s: kernel launch failed: %s", name, what, hipGetErrorString(e));
    return MG3D_OK;
}

/* the iterations, with z and r standing in for u and d of the top level (the caller exchanges and restores the pointers) */
static int pcg_iterate(mg3d_ctx *ctx, const char *name, const InnerProduct &ip, double *x, double target, int max_iters,
                       double *norms, int &iters, int &converged, double &r_norm)
{
    Level &top = ctx->lv[ctx->L - 1];
    const int q = ctx->L - 1, bc = mg3d_ctx_bc(ctx);
    const LevelOperator A = mg3d_level_operator(ctx, q);
    hipStream_t s = ctx->stream;
    double *const sc = ctx->sumsq, *const r = ctx->pcg_v[V_R], *const p = ctx->pcg_v[V_P], *const qv = ctx->pcg_v[V_Q];
    for (int k = 0;; k++) {
        /* z = V(r): the cycle starts from u = 0 on the top level too (faces included: the error's Dirichlet values) */
        HIPCHK(hipMemsetAsync(top.f[MG3D_U], 0, top.elems * sizeof(double), s));
        CHK(mg3d_enqueue_vcycle(ctx, q, S_CYCLE, 0));
        ctx->red_tail = false; /* u and d of the top level change under the next cycle */
        const double *z = top.f[MG3D_U];
        double *const rz = sc + S_RZ + (k & 1), *const rz_old = sc + S_RZ + ((k + 1) & 1);
        if ((ip.weighted ? k_wpcg_dot(top.g, bc, r, z, ctx->partials, rz, sc + S_WZ, s)
                         : k_pcg_dot(top.g, bc, r, z, ctx->partials, rz, s)) < 0)
            return fail(MG3D_ERR_STATE, "%s: the level has no launch shape", name);
        if (ip.weighted) {
            if (k == 0) /* whatever an earlier solve left where this context has no unknowns */
                HIPCHK(hipMemsetAsync(p, 0, top.elems * sizeof(double), s));
            k_wpcg_direction(top.g, bc, p, z, rz, rz_old, sc + S_WZ, ip.singular ? ip.W : 0., k == 0, s);
        } else if (k == 0)
            HIPCHK(hipMemcpyAsync(p, z, top.elems * sizeof(double), hipMemcpyDeviceToDevice, s)); /* p = z */
        else
            k_pcg_direction(top.g, bc, p, z, rz, rz_old, s);
        {
            StageScope kt(ctx, q, MG3D_K_PCG_APPLY, true);
            k_pcg_apply_dot(top.g, p, A, qv, ctx->partials, sc + S_PAP, s);
        }
        k_pcg_update_norm(top.g, bc, x, r, p, qv, rz, sc + S_PAP, ctx->partials, sc + S_RR, s);
        CHK(pcg_launch_ok(name, "iteration"));
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

static int pcg_check_args(const char *name, const mg3d_ctx *ctx, double rtol, double atol, int max_iters)
{
    if (!ctx)
        return fail(MG3D_ERR_ARG, "%s: NULL context", name);
    if (!(rtol >= 0.) || !(atol >= 0.) || !isfinite(rtol) || !isfinite(atol) || max_iters < 0)
        return fail(MG3D_ERR_ARG, "%s: rtol and atol must be finite and >= 0, max_iters >= 0 (%g, %g, %d)", name, rtol, atol,
                    max_iters);
    if (rtol == 0. && atol == 0. && max_iters == 0)
        return fail(MG3D_ERR_ARG, "%s: rtol = atol = 0 needs max_iters > 0", name);
    return MG3D_OK;
}

static int pcg_check_state(const char *name, const mg3d_ctx *ctx)
{
    if (ctx->have_es)
        return fail(MG3D_ERR_STATE, "%s: the context holds the mixed-boundary factor of mg3d_es_setup", name);
    if (!ctx->have_lu)
        return fail(MG3D_ERR_STATE, "%s: no coarse LU set (mg3d_ctx_build_coarse / mg3d_ctx_set_lu)", name);
    return MG3D_OK;
}

/* the solve of a checked call in the inner product ip */
static int pcg_run(mg3d_ctx *ctx, const char *name, const InnerProduct &ip, double rtol, double atol, int max_iters,
                   double *norms, mg3d_wpcg_info *info)
{
    CHK(mg3d_drop_carry(ctx)); /* a cycle that has run ahead is finished first */
    const int q = ctx->L - 1, bc = mg3d_ctx_bc(ctx);
    Level &top = ctx->lv[q];
    hipStream_t s = ctx->stream;
    const bool stored = max_iters > 0 || ip.singular; /* the projection works on the stored residual */
    if (stored)
        CHK(pcg_alloc(ctx, name));
    /* r_0 = d - A x; with iterations to come it is stored as the first right-hand side of the cycle */
    k_residual(top.g, top.f[MG3D_U], top.f[MG3D_D], mg3d_level_operator(ctx, q), stored ? ctx->pcg_v[V_R] : nullptr,
               ctx->partials, ctx->sumsq + S_R0, s);
    if (ip.singular) {
        /* sum(w r_0) and sum(w d), then r_0 -= sum(w r_0)/W and its norm */
        double *const sc = ctx->sumsq, *const r = ctx->pcg_v[V_R];
        if (k_wpcg_dot(top.g, bc, top.f[MG3D_D], r, ctx->partials, sc + S_DROP, sc + S_WR, s) < 0)
            return fail(MG3D_ERR_STATE, "%s: the level has no launch shape", name);
        k_wpcg_dot(top.g, bc, r, top.f[MG3D_D], ctx->partials, sc + S_DROP, sc + S_WD, s);
        k_wpcg_center(top.g, bc, r, sc + S_WR, ip.W, ctx->partials, sc + S_R0, s);
        HIPCHK(hipMemcpyAsync(ctx->h_sumsq + S_WD, sc + S_WD, sizeof(double), hipMemcpyDeviceToHost, s));
    }
    CHK(pcg_launch_ok(name, "initial residual"));
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
        mg3d_ctx_touched(ctx, MG3D_D, q); /* the cycles' d is the residual, rewritten every iteration: no zero map of it */
        rc = pcg_iterate(ctx, name, ip, x, target, max_iters, norms, iters, converged, r_norm);
        if (rc != MG3D_OK)
            (void)hipStreamSynchronize(s);
        (void)mg3d_drop_carry(ctx);
        ctx->pcg_v[V_Z] = top.f[MG3D_U]; /* the fused schedules exchange u and the level's second buffer */
        top.f[MG3D_U] = x;
        top.f[MG3D_D] = d;
        if (rc == MG3D_OK && ctx->periodic) {
            k_per_refresh(top.g, x, bc, s); /* the passes write unique points only */
            rc = pcg_launch_ok(name, "duplicate refresh");
        }
        if (rc == MG3D_OK)
            rc = mg3d_sync(ctx);
    }
    if (info) {
        info->iterations = iters;
        info->converged = converged;
        info->r0_norm = r0;
        info->r_norm = r_norm;
        info->singular = ip.singular;
        info->rhs_mean = ip.singular ? ctx->h_sumsq[S_WD] / ip.W : 0.;
    }
    return rc;
}

extern "C" int mg3d_pcg_solve(mg3d_ctx *ctx, double rtol, double atol, int max_iters, double *norms, mg3d_pcg_info *info)
{
    const char *const name = "mg3d_pcg_solve";
    CHK(pcg_check_args(name, ctx, rtol, atol, max_iters));
    if (ctx->neumann)
        return fail(MG3D_ERR_STATE, "mg3d_pcg_solve: the context has Neumann faces (mg3d_ctx_set_neumann): the reflected "
                                    "operator is not symmetric in the Euclidean inner product (mg3d_wpcg_solve)");
    if (ctx->periodic && mg3d_ctx_pinned(ctx))
        return fail(MG3D_ERR_STATE, "mg3d_pcg_solve: every axis periodic with sigma = 0 is singular: the pinned row of the "
                                    "coarse matrix makes the cycle an unsymmetric preconditioner (mg3d_wpcg_solve)");
    CHK(pcg_check_state(name, ctx));
    mg3d_wpcg_info w;
    const int rc = pcg_run(ctx, name, InnerProduct{false, false, 0.}, rtol, atol, max_iters, norms, info ? &w : nullptr);
    if (info) {
        info->iterations = w.iterations;
        info->converged = w.converged;
        info->r0_norm = w.r0_norm;
        info->r_norm = w.r_norm;
    }
    return rc;
}

extern "C" int mg3d_wpcg_solve(mg3d_ctx *ctx, double rtol, double atol, int max_iters, double *norms, mg3d_wpcg_info *info)
{
    const char *const name = "mg3d_wpcg_solve";
    CHK(pcg_check_args(name, ctx, rtol, atol, max_iters));
    CHK(pcg_check_state(name, ctx));
    /* without a Neumann face w = 1 and, unless the operator is singular, this is mg3d_pcg_solve's iteration: its passes */
    InnerProduct ip;
    ip.singular = mg3d_ctx_singular(ctx); /* (a fixed unknown of the finest level removes the constants from the kernel) */
    ip.weighted = ctx->neumann != 0 || ip.singular;
    ip.W = k_wpcg_weight_sum(ctx->lv[ctx->L - 1].g, mg3d_ctx_bc(ctx));
    return pcg_run(ctx, name, ip, rtol, atol, max_iters, norms, info);
}
