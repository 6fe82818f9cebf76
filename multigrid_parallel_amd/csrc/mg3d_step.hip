/*
 * mg3d_step.hip -- implicit time stepping on the device (mg3d_step_setup, mg3d_step_set_source, mg3d_step_advance,
 * include/mg3d.h): the theta-scheme for  u_t = div(eps grad u) - kappa u + s  with the context's operator and boundaries.
 *
 * With L the context's operator at sigma = 0 and A_sigma = L - sigma, one step of length dt is
 *     (u1 - u0)/dt = theta (L u1 - kappa u1) + (1 - theta)(L u0 - kappa u0) + s
 * Divided by theta, with c0 = 1/(theta dt) and sigma = kappa + c0:
 *     A_sigma u1 = -(c0/theta) u0 - ((1 - theta)/theta) (L u0 - kappa u0 + c0 u0) - s/theta
 * since -c0 u0 - ((1 - theta)/theta)(L u0 - kappa u0) = -(c0/theta) u0 - ((1 - theta)/theta)(L u0 - kappa u0 + c0 u0) with
 * 1 + c1 = 1/theta; and L u0 - kappa u0 = q + c0 u0 for q = A_sigma u0, the one thing the library's kernels compute.  So
 *     d = -((a u0 + c1 q) + b s),   a = c0/theta,  c1 = (1 - theta)/theta,  b = 1/theta
 * -- one launch (k_step_rhs, mg3d_kernels.hip), no field leaves the device.  theta = 1: c1 = 0 and q is not formed.
 *
 * A step is that launch and then the context's own solve from u0 as the guess: mg3d_vcycles(cycles), schedules included,
 * or mg3d_wpcg_solve(rtol, 0, cycles).  sigma > 0: the operator is never singular.  A cycle that has run ahead is finished
 * before the launch (mg3d_drop_carry): the launch reads u and writes d of the top level, which also ends the shortcut of
 * the next cycle's first red pass (red_tail).
 */
#include "mg3d_ctx.h"

#include <math.h>

#include <vector>

#define fail mg3d_fail

extern "C" int mg3d_step_setup(mg3d_ctx *ctx, double dt, double theta, double kappa)
{
    if (!ctx)
        return fail(MG3D_ERR_ARG, "mg3d_step_setup: NULL context");
    if (!(dt > 0.) || !isfinite(dt) || !(theta >= 0.5 && theta <= 1.) || !(kappa >= 0.) || !isfinite(kappa))
        return fail(MG3D_ERR_ARG, "mg3d_step_setup: need dt > 0, 0.5 <= theta <= 1, kappa >= 0, all finite (%g, %g, %g)", dt,
                    theta, kappa);
    const double c0 = 1.0 / (theta * dt), sigma = kappa + c0;
    if (!isfinite(sigma))
        return fail(MG3D_ERR_ARG, "mg3d_step_setup: kappa + 1/(theta*dt) is not finite (%g, %g, %g)", dt, theta, kappa);
    const int rc = mg3d_ctx_set_shift(ctx, sigma);
    if (rc != MG3D_OK)
        return rc;
    ctx->step_set = true;
    ctx->step_dt = dt;
    ctx->step_theta = theta;
    ctx->step_kappa = kappa;
    ctx->step_sigma = sigma;
    return MG3D_OK;
}

/* the source field of the finest level, zeroed, unless the context has it already */
static int step_src_alloc(mg3d_ctx *ctx)
{
    if (ctx->step_src)
        return MG3D_OK;
    const Level &top = ctx->lv[ctx->L - 1];
    double *v = nullptr;
    hipError_t e = hipMalloc(&v, top.elems * sizeof(double));
    if (e == hipSuccess)
        e = hipMemsetAsync(v, 0, top.elems * sizeof(double), ctx->stream); /* (the padding of the rows) */
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->stream);
        if (v)
            (void)hipFree(v);
        return mg3d_alloc_fail(e, "mg3d_step_set_source", "the source field");
    }
    ctx->step_src = v;
    return MG3D_OK;
}

extern "C" int mg3d_step_set_source(mg3d_ctx *ctx, const double *s)
{
    if (!ctx)
        return fail(MG3D_ERR_ARG, "mg3d_step_set_source: NULL context");
    if (!s) {
        ctx->step_has_src = false;
        return MG3D_OK;
    }
    const Level &top = ctx->lv[ctx->L - 1];
    const int N = top.g.N;
    const int rc = step_src_alloc(ctx);
    if (rc != MG3D_OK)
        return rc;
    /* (a step still in flight reads the field: the copy is ordered behind it on the context's stream) */
    hipError_t e = hipMemcpy2DAsync(ctx->step_src, top.g.pitch * sizeof(double), s, N * sizeof(double), N * sizeof(double),
                                    (size_t)N * N, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess)
        return fail(MG3D_ERR_HIP, "mg3d_step_set_source: upload: %s", hipGetErrorString(e));
    ctx->step_has_src = true;
    return MG3D_OK;
}

/* the same from a device array (mg3d_array): packed into the source field on the context's stream, behind any step in
 * flight and behind what the caller's stream did to the array; no host synchronisation */
extern "C" int mg3d_step_set_source_device(mg3d_ctx *ctx, const mg3d_array *s, void *stream)
{
    static const char who[] = "mg3d_step_set_source_device";
    if (!ctx)
        return fail(MG3D_ERR_ARG, "%s: NULL context", who);
    if (!s) {
        ctx->step_has_src = false;
        return MG3D_OK;
    }
    int rc = mg3d_array_check(ctx, s, false, who);
    if (rc == MG3D_OK)
        rc = step_src_alloc(ctx);
    if (rc == MG3D_OK)
        rc = mg3d_stream_join(ctx, (hipStream_t)stream, false, who);
    if (rc != MG3D_OK)
        return rc;
    const int q = ctx->L - 1;
    {
        StageScope kt(ctx, q, MG3D_K_PACK, true);
        k_pack(ctx->lv[q].g, ctx->step_src, *s, ctx->stream);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(MG3D_ERR_HIP, "%s: kernel launch failed: %s", who, hipGetErrorString(e));
    ctx->step_has_src = true;
    return mg3d_stream_join(ctx, (hipStream_t)stream, true, who);
}

/* steps [0, nsteps) of a checked call; `done` counts the completed ones */
static int step_run(mg3d_ctx *ctx, int nsteps, int method, int cycles, double rtol, double *norms, int &done, int &iters,
                    int &converged)
{
    const int q = ctx->L - 1;
    const double theta = ctx->step_theta;
    const bool be = theta == 1.0;
    const double c0 = 1.0 / (theta * ctx->step_dt);
    const double a = c0 / theta, c1 = (1.0 - theta) / theta, b = 1.0 / theta;
    std::vector<double> cyc; /* mg3d_vcycles' norms: the step's is the last one */
    if (method == MG3D_STEP_VCYCLES) {
        try {
            cyc.resize((size_t)cycles);
        } catch (...) {
            return fail(MG3D_ERR_ALLOC, "mg3d_step_advance: %d norms do not fit", cycles);
        }
    }
    for (int n = 0; n < nsteps; n++) {
        int rc = mg3d_drop_carry(ctx); /* between steps too: the last cycle of a step may have run ahead */
        if (rc != MG3D_OK)
            return rc;
        const Level &top = ctx->lv[q];
        {
            StageScope kt(ctx, q, MG3D_K_STEP_RHS, true);
            if (k_step_rhs(top.g, top.f[MG3D_U], ctx->step_has_src ? ctx->step_src : nullptr, mg3d_level_operator(ctx, q), a, c1,
                           b, be, top.f[MG3D_D], ctx->stream) < 0)
                return fail(MG3D_ERR_STATE, "mg3d_step_advance: the level has no launch shape");
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return fail(MG3D_ERR_HIP, "mg3d_step_advance: right-hand side: kernel launch failed: %s", hipGetErrorString(e));
        mg3d_ctx_touched(ctx, MG3D_D, q);
        double norm = 0.;
        if (method == MG3D_STEP_VCYCLES) {
            rc = mg3d_vcycles(ctx, cycles, cyc.data());
            if (rc == MG3D_OK)
                norm = cyc.back();
        } else {
            mg3d_wpcg_info w = {};
            rc = mg3d_wpcg_solve(ctx, rtol, 0., cycles, nullptr, &w);
            if (rc == MG3D_OK) {
                iters += w.iterations;
                converged = converged && w.converged;
                norm = w.r_norm;
            }
        }
        if (rc != MG3D_OK)
            return rc;
        if (norms)
            norms[n] = norm;
        done = n + 1;
    }
    return MG3D_OK;
}

extern "C" int mg3d_step_advance(mg3d_ctx *ctx, int nsteps, int method, int cycles, double rtol, double *norms,
                                 mg3d_step_info *info)
{
    if (!ctx)
        return fail(MG3D_ERR_ARG, "mg3d_step_advance: NULL context");
    if (nsteps < 0 || (method != MG3D_STEP_VCYCLES && method != MG3D_STEP_WPCG) || cycles < 1)
        return fail(MG3D_ERR_ARG, "mg3d_step_advance: need nsteps >= 0, a method of MG3D_STEP_*, cycles >= 1 (%d, %d, %d)",
                    nsteps, method, cycles);
    if (method == MG3D_STEP_WPCG && (!(rtol >= 0.) || !isfinite(rtol)))
        return fail(MG3D_ERR_ARG, "mg3d_step_advance: rtol must be finite and >= 0 (%g)", rtol);
    if (!ctx->step_set)
        return fail(MG3D_ERR_STATE, "mg3d_step_advance: mg3d_step_setup was not called");
    if (ctx->sigma != ctx->step_sigma)
        return fail(MG3D_ERR_STATE, "mg3d_step_advance: the context's shift (%g) is no longer the one mg3d_step_setup set (%g)",
                    ctx->sigma, ctx->step_sigma);
    /* (a context after mg3d_es_setup never gets here: that call needs sigma = 0 and mg3d_step_setup's shift is > 0 and
     * drops its factor, so one of the tests around this comment has already refused it) */
    if (!ctx->have_lu)
        return fail(MG3D_ERR_STATE, "mg3d_step_advance: no coarse LU set (mg3d_ctx_build_coarse / mg3d_ctx_set_lu)");
    int done = 0, iters = 0, converged = 1;
    const int rc = nsteps > 0 ? step_run(ctx, nsteps, method, cycles, rtol, norms, done, iters, converged) : MG3D_OK;
    if (info) {
        info->steps = done;
        info->iterations = iters;
        info->converged = method == MG3D_STEP_WPCG && rc == MG3D_OK && converged;
        info->time = done * ctx->step_dt;
    }
    return rc;
}
