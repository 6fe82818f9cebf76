/*
 * mg3d_field.hip -- field output on the device (mg3d_field_gradient, mg3d_field_gradient_device, mg3d_field_flux,
 * mg3d_field_energy, include/mg3d.h "Field output"): what a caller wants of a solved potential u of
 * div(eps grad u) - sigma u = f  -- the field E = -grad u, the charge on each embedded conductor, the stored energy --
 * formed from u of the finest level with the context's own boundary logic: periodic wraps, reflected Neumann faces, the
 * face means of eps and the fixed-point bytes.  The kernels are in mg3d_kernels.hip ("field output").
 *
 * All four calls only read the context.  A cycle that has run ahead is finished first exactly as mg3d_download_device
 * does (mg3d_drop_carry_keep: red_tail stays, the next cycle continues as if nothing had been asked); no field, option,
 * factor or flag changes.  The two sums use the context's partial sums and the last slot of its norms, both free between
 * entry points.  sigma enters none of the three quantities.
 *
 *   gradient : one launch, u read once, every wanted component stored from the same registers; it reads or writes a
 *              caller's array, so it counts under MG3D_K_PACK.  The host form runs that launch once per wanted component
 *              into one dense N^3 scratch buffer of its own (allocated for the call, freed at return) and copies it out;
 *              it never goes through r or any other field of the context.
 *   flux     : F = h * sum of t_p over the fixed unknowns with the label, the multiplication on the host behind the fold.
 *   energy   : W = 0.5 * h * sum over the owned edges, likewise.
 * The sums are per-block partials folded by one block in a fixed order (k_fold): the same call on the same data gives
 * the same bits.  Each of the two synchronises with the host once.
 */
#include "mg3d_ctx.h"

#include <math.h>

#define fail mg3d_fail

static int field_launch_ok(const char *who)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(MG3D_ERR_HIP, "%s: kernel launch failed: %s", who, hipGetErrorString(e));
    return MG3D_OK;
}

/* the finest level of a context these calls serve: a single-domain level of at least three points per side */
int mg3d_field_level(const mg3d_ctx *ctx, const char *who)
{
    const Geom &g = ctx->lv[ctx->L - 1].g;
    if (g.N < 3 || g.ni != g.N || g.nj != g.N || g.nk != g.N)
        return fail(MG3D_ERR_STATE, "%s: needs a single-domain level of at least 3 points per side (%d x %d x %d of %d)", who,
                    g.ni, g.nj, g.nk, g.N);
    return MG3D_OK;
}

/* the gradient launch on the context's stream, behind a cycle that has run ahead */
static int gradient_enqueue(mg3d_ctx *ctx, double scale, const mg3d_array *const out[3], const char *who)
{
    int rc = mg3d_drop_carry_keep(ctx); /* (reads only, as mg3d_download_device) */
    if (rc != MG3D_OK)
        return rc;
    const int q = ctx->L - 1;
    const Level &top = ctx->lv[q];
    const double cs = scale * (0.5 / top.h);
    {
        StageScope kt(ctx, q, MG3D_K_PACK, true);
        if (k_gradient(top.g, top.f[MG3D_U], mg3d_ctx_bc(ctx), cs, out, ctx->stream) < 0)
            return fail(MG3D_ERR_STATE, "%s: the level has no launch shape", who);
    }
    return field_launch_ok(who);
}

static int gradient_args(const mg3d_ctx *ctx, double scale, bool any, const char *who)
{
    if (!ctx)
        return fail(MG3D_ERR_ARG, "%s: NULL context", who);
    if (!any)
        return fail(MG3D_ERR_ARG, "%s: no component wanted (all three NULL)", who);
    if (!isfinite(scale))
        return fail(MG3D_ERR_ARG, "%s: scale must be finite (%g)", who, scale);
    return mg3d_field_level(ctx, who);
}

extern "C" int mg3d_field_gradient_device(mg3d_ctx *ctx, double scale, const mg3d_array *const out[3], void *stream)
{
    static const char who[] = "mg3d_field_gradient_device";
    int rc = gradient_args(ctx, scale, out && (out[0] || out[1] || out[2]), who);
    for (int a = 0; a < 3 && rc == MG3D_OK; a++)
        if (out[a])
            rc = mg3d_array_check(ctx, out[a], true, who);
    if (rc == MG3D_OK)
        rc = mg3d_stream_join(ctx, (hipStream_t)stream, false, who); /* (what the caller's stream still does with out) */
    if (rc == MG3D_OK)
        rc = gradient_enqueue(ctx, scale, out, who);
    if (rc != MG3D_OK)
        return rc;
    return mg3d_stream_join(ctx, (hipStream_t)stream, true, who);
}

extern "C" int mg3d_field_gradient(mg3d_ctx *ctx, double scale, double *gi, double *gj, double *gk)
{
    static const char who[] = "mg3d_field_gradient";
    int rc = gradient_args(ctx, scale, gi || gj || gk, who);
    if (rc != MG3D_OK)
        return rc;
    const int N = ctx->lv[ctx->L - 1].g.N;
    const size_t bytes = (size_t)N * N * N * sizeof(double);
    double *scratch = nullptr;
    hipError_t e = hipMalloc(&scratch, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return mg3d_alloc_fail(e, who, "the scratch buffer");
    }
    const mg3d_array dense = {scratch, MG3D_F64, {(long long)N * N, N, 1}};
    double *const host[3] = {gi, gj, gk};
    for (int a = 0; a < 3 && rc == MG3D_OK; a++) {
        if (!host[a])
            continue;
        const mg3d_array *out[3] = {nullptr, nullptr, nullptr};
        out[a] = &dense;
        rc = gradient_enqueue(ctx, scale, out, who);
        if (rc != MG3D_OK)
            break;
        e = hipMemcpyAsync(host[a], scratch, bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(ctx->stream); /* (the next component overwrites the buffer) */
        if (e != hipSuccess)
            rc = fail(MG3D_ERR_HIP, "%s: copy to the host: %s", who, hipGetErrorString(e));
    }
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(scratch);
    return rc;
}

/* the folded sum of a launch, from the last slot of the context's norms: the call's one host synchronisation */
static int field_read_sum(mg3d_ctx *ctx, int slot, double *sum, const char *who)
{
    hipError_t e = hipMemcpyAsync(ctx->h_sumsq + slot, ctx->sumsq + slot, sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess)
        return fail(MG3D_ERR_HIP, "%s: reading the sum: %s", who, hipGetErrorString(e));
    *sum = ctx->h_sumsq[slot];
    return MG3D_OK;
}

extern "C" int mg3d_field_flux(mg3d_ctx *ctx, int label, double *flux)
{
    static const char who[] = "mg3d_field_flux";
    if (!ctx)
        return fail(MG3D_ERR_ARG, "%s: NULL context", who);
    if (!flux)
        return fail(MG3D_ERR_ARG, "%s: NULL result pointer", who);
    if (label < 0 || label > 255)
        return fail(MG3D_ERR_ARG, "%s: label %d (0: every fixed point, 1..255: the points with that byte)", who, label);
    if (!ctx->mask.set())
        return fail(MG3D_ERR_STATE, "%s: the context has no mask (mg3d_ctx_set_mask)", who);
    int rc = mg3d_field_level(ctx, who);
    if (rc == MG3D_OK)
        rc = mg3d_drop_carry_keep(ctx);
    if (rc != MG3D_OK)
        return rc;
    const int q = ctx->L - 1, slot = ctx->sumsq_slots - 1;
    const Level &top = ctx->lv[q];
    if (k_field_flux(top.g, top.f[MG3D_U], mg3d_level_operator(ctx, q, false), label, ctx->partials, ctx->sumsq + slot, ctx->stream) < 0)
        return fail(MG3D_ERR_STATE, "%s: the level has no launch shape", who);
    rc = field_launch_ok(who);
    double sum = 0.;
    if (rc == MG3D_OK)
        rc = field_read_sum(ctx, slot, &sum, who);
    if (rc != MG3D_OK)
        return rc;
    *flux = top.h * sum;
    return MG3D_OK;
}

extern "C" int mg3d_field_energy(mg3d_ctx *ctx, double *energy)
{
    static const char who[] = "mg3d_field_energy";
    if (!ctx)
        return fail(MG3D_ERR_ARG, "%s: NULL context", who);
    if (!energy)
        return fail(MG3D_ERR_ARG, "%s: NULL result pointer", who);
    int rc = mg3d_field_level(ctx, who);
    if (rc == MG3D_OK)
        rc = mg3d_drop_carry_keep(ctx);
    if (rc != MG3D_OK)
        return rc;
    const int q = ctx->L - 1, slot = ctx->sumsq_slots - 1;
    const Level &top = ctx->lv[q];
    if (k_field_energy(top.g, top.f[MG3D_U], mg3d_level_operator(ctx, q, false), ctx->partials, ctx->sumsq + slot, ctx->stream) < 0)
        return fail(MG3D_ERR_STATE, "%s: the level has no launch shape", who);
    rc = field_launch_ok(who);
    double sum = 0.;
    if (rc == MG3D_OK)
        rc = field_read_sum(ctx, slot, &sum, who);
    if (rc != MG3D_OK)
        return rc;
    *energy = 0.5 * top.h * sum;
    return MG3D_OK;
}
