/*
 * mg3d_es.hip -- the mixed-boundary ("electrospray") problem of the reference's original program on the live
 * operators.  PARITY UNPINNED: mg_3d_bkup.c neither compiles nor uses an order-independent smoother,
 * so no vector of it can be reproduced; the semantics are defined here and restated in plain C by the test
 * infrastructure, which the tests compare with bit for bit.
 *
 * From mg_3d_bkup.c: the geometry and potentials (:12-18), the Dirichlet patches (:739-778: capillary disc on x = 0,
 * extractor annulus on x = L, radii measured from the centre of the (y, z) face with the level's own spacing) and the
 * zero-gradient walls everywhere else, imposed by copying a freshly updated interior value onto the wall point behind
 * it (:84-133) on every level.  From mg_3d.h: everything else -- red-black passes (:640-781) with the update of
 * :438-443, residual, restriction, prolongation, the dense LU with identity boundary rows, the cycle (:1242-1362).
 * A wall point is written only by the interior point in front of it and read only by that point, so within a colour
 * pass the copies are order-independent: one thread updates its point and writes up to three wall points.
 * After the prolongation (which touches every fine point, :1000-1145) the Dirichlet patch points are put back to their
 * potential (finest level) or to zero (error equation).  The coarsest operator gets zero-gradient rows on the walls
 * (mg3d_es_coarse_matrix; the original pins them to zero, which stalls the cycle at a factor of 0.93-0.96), and the
 * ghost copy is applied once behind the direct solve.
 *
 * This is the reason smoothenAtIndex still carries center[] and the radius arguments (mg_3d.h:432-436).  The path is
 * one launch per colour pass: it is a feature row, not the benchmark path.
 */
#include "mg3d_ctx.h"

#include <math.h>
#include <stdlib.h>

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

extern "C" int mg3d_es_default_params(mg3d_es_params *p)
{
    if (!p)
        return fail(MG3D_ERR_ARG, "mg3d_es_default_params: NULL");
    p->length = 3e-4;                  /* GRID_LENGTH, mg_3d_bkup.c:12 */
    p->capillary_radius = 1.326e-5;    /* :14 */
    p->extractor_inner_radius = 1e-4;  /* :15 */
    p->extractor_outer_radius = 1.4e-4; /* :16 */
    p->capillary_voltage = 0.;         /* :17 */
    p->extractor_voltage = -1350.;     /* :18 */
    return MG3D_OK;
}

__device__ __forceinline__ double es_rr(const mg3d_es_params &p, double h, int j, int k)
{
    const double ty = j * h - p.length / 2., tz = k * h - p.length / 2.; /* mg_3d_bkup.c:98-100 */
    return ty * ty + tz * tz;
}
__device__ __forceinline__ bool es_dirichlet_x0(const mg3d_es_params &p, double h, int j, int k)
{
    return es_rr(p, h, j, k) <= p.capillary_radius * p.capillary_radius; /* :755 */
}
__device__ __forceinline__ bool es_dirichlet_xl(const mg3d_es_params &p, double h, int j, int k)
{
    const double rr = es_rr(p, h, j, k); /* :771-773 */
    return rr > p.extractor_inner_radius * p.extractor_inner_radius && rr < p.extractor_outer_radius * p.extractor_outer_radius;
}

/* ghost copy behind the interior point (i, j, k) (mg_3d_bkup.c:84-133) */
__device__ __forceinline__ void es_ghost(const Geom &g, double *v, const mg3d_es_params &p, double h, int i, int j, int k,
                                         long long q, double val)
{
    if (i == 1 && !es_dirichlet_x0(p, h, j, k))
        v[q - g.plane] = val;
    if (i == g.ni - 2 && !es_dirichlet_xl(p, h, j, k))
        v[q + g.plane] = val;
    if (j == 1)
        v[q - g.pitch] = val;
    if (j == g.nj - 2)
        v[q + g.pitch] = val;
    if (k == 1)
        v[q - 1] = val;
    if (k == g.nk - 2)
        v[q + 1] = val;
}

/* one colour pass (mg_3d.h:438-443, 658-702) + the ghost copies; a lane owns the k-pair (2m, 2m+1) of one row and
 * updates the member of the colour being swept.  update = false: only the ghost copies (behind the direct solve). */
template <bool UPDATE>
__global__ void __launch_bounds__(256) es_color_kernel(Geom g, double *__restrict__ v, const double *__restrict__ d,
                                                       double h, double hSq, double sixth, int color, mg3d_es_params p)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = 1 + blockIdx.y * blockDim.y + threadIdx.y;
    const int i = 1 + blockIdx.z;
    if (j > g.nj - 2)
        return;
    const int k = 2 * m + ((color + i + j) & 1);
    if (k < 1 || k > g.nk - 2)
        return;
    const long long q = g.plane * i + (long long)g.pitch * j + k;
    double val;
    if (UPDATE) {
        double s = v[q - g.plane] + v[q + g.plane];
        s = s + v[q - g.pitch];
        s = s + v[q + g.pitch];
        s = s + v[q - 1];
        s = s + v[q + 1];
        s = s - hSq * d[q];
        val = sixth * s;
        v[q] = val;
    } else {
        val = v[q];
    }
    es_ghost(g, v, p, h, i, j, k, q, val);
}

/* Dirichlet patches of the two x faces: scale * potential */
__global__ void __launch_bounds__(256) es_fill_kernel(Geom g, double *__restrict__ v, double h, double scale, mg3d_es_params p)
{
    const int k = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
    if (k >= g.nk || j >= g.nj)
        return;
    if (es_dirichlet_x0(p, h, j, k))
        v[(long long)g.pitch * j + k] = scale * p.capillary_voltage;
    if (es_dirichlet_xl(p, h, j, k))
        v[g.plane * (g.ni - 1) + (long long)g.pitch * j + k] = scale * p.extractor_voltage;
}

static void es_color(mg3d_ctx *ctx, int level, int color, bool update)
{
    Level &l = ctx->lv[level];
    const Geom &g = l.g;
    if (g.ni < 3)
        return;
    dim3 block(64, 4, 1), grid(((g.nk + 1) / 2 + 63) / 64, (g.nj - 2 + 3) / 4, g.ni - 2);
    if (update)
        hipLaunchKernelGGL(es_color_kernel<true>, grid, block, 0, ctx->stream, g, l.f[MG3D_U], l.f[MG3D_D], l.h, l.h * l.h,
                           1. / 6, color, ctx->es);
    else
        hipLaunchKernelGGL(es_color_kernel<false>, grid, block, 0, ctx->stream, g, l.f[MG3D_U], l.f[MG3D_D], l.h, l.h * l.h,
                           1. / 6, color, ctx->es);
}

static void es_fill(mg3d_ctx *ctx, int level, double scale)
{
    Level &l = ctx->lv[level];
    hipLaunchKernelGGL(es_fill_kernel, dim3((l.g.nk + 63) / 64, (l.g.nj + 3) / 4, 1), dim3(64, 4, 1), 0, ctx->stream, l.g,
                       l.f[MG3D_U], l.h, scale, ctx->es);
}

static void es_smooth(mg3d_ctx *ctx, int level, int post, int iters)
{
    for (int s = 0; s < iters; s++) { /* pre: red, black (mg_3d.h:657-702); post: black, red (:728-773) */
        es_color(ctx, level, post ? 0 : 1, true);
        es_color(ctx, level, post ? 1 : 0, true);
    }
}

static int launch_ok_es(const char *who)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(MG3D_ERR_HIP, "%s: kernel launch failed: %s", who, hipGetErrorString(e));
    return MG3D_OK;
}

extern "C" int mg3d_es_setup(mg3d_ctx *ctx, const mg3d_es_params *p)
{
    CHK(mg3d_drop_carry(ctx));
    if (ctx && ctx->eps.set()) /* the mixed-boundary problem has a constant coefficient (checked before its own state) */
        return fail(MG3D_ERR_STATE, "mg3d_es_setup: the context has a variable coefficient (mg3d_ctx_set_coefficient); set it to NULL");
    if (ctx && ctx->periodic) /* the mixed-boundary problem is defined on six faces */
        return fail(MG3D_ERR_STATE, "mg3d_es_setup: the context has periodic axes (mg3d_ctx_set_periodic); set them to 0");
    if (ctx && ctx->neumann)
        return fail(MG3D_ERR_STATE, "mg3d_es_setup: the context has Neumann faces (mg3d_ctx_set_neumann); set them to 0");
    if (ctx && ctx->mask.set())
        return fail(MG3D_ERR_STATE, "mg3d_es_setup: the context has fixed points (mg3d_ctx_set_mask); set the mask to NULL");
    if (ctx && ctx->sfield.set())
        return fail(MG3D_ERR_STATE, "mg3d_es_setup: the context has a screening field (mg3d_ctx_set_shift_field); set it to NULL");
    if (!ctx || !p || !(p->length > 0.))
        return fail(MG3D_ERR_ARG, "mg3d_es_setup: bad arguments");
    if (ctx->sigma != 0.) /* the mixed-boundary problem keeps the reference's operator */
        return fail(MG3D_ERR_STATE, "mg3d_es_setup: the context has a screened operator (mg3d_ctx_set_shift); set the shift to 0");
    if (p->length != ctx->length)
        return fail(MG3D_ERR_ARG, "mg3d_es_setup: the context was created with grid length %g, the problem has %g", ctx->length,
                    p->length);
    ctx->es = *p;
    for (int lv = 0; lv < ctx->L; lv++) {
        Level &l = ctx->lv[lv];
        for (int f = 0; f < 3; f++) {
            HIPCHK(hipMemsetAsync(l.f[f], 0, l.elems * sizeof(double), ctx->stream));
            mg3d_ctx_touched(ctx, f, lv); /* written from outside the cycle: the coarse faces are injected afresh */
        }
    }
    const int top = ctx->L - 1;
    {
        const int N0 = ctx->lv[0].g.N;
        const long long n = (long long)N0 * N0 * N0;
        if (n * n >= 2147483647LL)
            return fail(MG3D_ERR_ARG, "mg3d_es_setup: coarse grid %d^3 too large for a dense factor", N0);
        double *A = (double *)calloc((size_t)(n * n), sizeof(double));
        if (!A)
            return fail(MG3D_ERR_ALLOC, "mg3d_es_setup: out of host memory");
        mg3d_es_coarse_matrix(A, N0, ctx->lv[0].h, p); /* mg_3d.h:287: spacing of the coarsest level */
        mg3d_lu_factor(A, (int)n);
        const int rc = mg3d_ctx_set_lu(ctx, A); /* clears have_es: the factor now loaded is ... */
        free(A);
        CHK(rc);
    }
    ctx->have_es = true; /* ... the mixed-boundary one: mg3d_vcycle* / mg3d_fmg_initialize / mg3d_coarse_solve refuse it */
    es_fill(ctx, top, 1.);
    return launch_ok_es("mg3d_es_setup");
}

extern "C" int mg3d_es_smooth(mg3d_ctx *ctx, int level, int post, int iters)
{
    CHK(mg3d_drop_carry(ctx));
    if (ctx && ctx->eps.set()) /* the mixed-boundary problem has a constant coefficient (checked before its own state) */
        return fail(MG3D_ERR_STATE, "mg3d_es_smooth: the context has a variable coefficient (mg3d_ctx_set_coefficient); set it to NULL");
    if (ctx && ctx->periodic) /* the mixed-boundary problem is defined on six faces */
        return fail(MG3D_ERR_STATE, "mg3d_es_smooth: the context has periodic axes (mg3d_ctx_set_periodic); set them to 0");
    if (ctx && ctx->neumann)
        return fail(MG3D_ERR_STATE, "mg3d_es_smooth: the context has Neumann faces (mg3d_ctx_set_neumann); set them to 0");
    if (ctx && ctx->mask.set())
        return fail(MG3D_ERR_STATE, "mg3d_es_smooth: the context has fixed points (mg3d_ctx_set_mask); set the mask to NULL");
    if (ctx && ctx->sfield.set())
        return fail(MG3D_ERR_STATE, "mg3d_es_smooth: the context has a screening field (mg3d_ctx_set_shift_field); set it to NULL");
    if (!ctx || !ctx->have_es || level < 0 || level >= ctx->L || iters < 0)
        return fail(MG3D_ERR_ARG, "mg3d_es_smooth: bad arguments (mg3d_es_setup first)");
    if (ctx->sigma != 0.) /* the mixed-boundary problem keeps the reference's operator */
        return fail(MG3D_ERR_STATE, "mg3d_es_smooth: the context has a screened operator (mg3d_ctx_set_shift); set the shift to 0");
    es_smooth(ctx, level, post, iters);
    return launch_ok_es("mg3d_es_smooth");
}

/* the plain operator of a level: the reference's Laplacian, no shift, no eps, Dirichlet faces as the kernels see them */
static LevelOperator es_operator(const Level &lev) { return {mg3d_level_op(lev.h, 0.), 0., nullptr, 0, nullptr}; }

static int es_vcycle(mg3d_ctx *ctx, int q, int slot)
{
    hipStream_t s = ctx->stream;
    if (!ctx->have_es || !ctx->have_lu) /* mg3d_ctx_set_lu / mg3d_ctx_build_coarse since the set-up: Dirichlet factor loaded */
        return fail(MG3D_ERR_STATE, "mg3d_es_vcycles: the context's coarse factor is not the mixed-boundary one (mg3d_es_setup)");
    for (int l = q; l >= 1; l--) {
        Level &lev = ctx->lv[l], &lc = ctx->lv[l - 1];
        if (l < ctx->L - 1)
            HIPCHK(hipMemsetAsync(lev.f[MG3D_U], 0, lev.elems * sizeof(double), s)); /* mg_3d.h:1258-1259 */
        es_smooth(ctx, l, 0, ctx->iters);                                                            /* :1282 */
        k_residual(lev.g, lev.f[MG3D_U], lev.f[MG3D_D], es_operator(lev), lev.f[MG3D_R], ctx->partials,
                   ctx->sumsq + ctx->sumsq_slots - 1, s);                                           /* :1294 */
        k_restrict(lev.g, lev.f[MG3D_R], lc.g, lc.f[MG3D_D], 0, s);                                  /* :1310 */
    }
    {
        Level &l0 = ctx->lv[0];
        if (0 < ctx->L - 1)
            HIPCHK(hipMemsetAsync(l0.f[MG3D_U], 0, l0.elems * sizeof(double), s));
        k_lu_solve(ctx->lu, ctx->lu_in, l0.g, l0.f[MG3D_D], l0.f[MG3D_U], ctx->lu_work, s); /* :1270 */
        es_color(ctx, 0, 0, false);                                             /* the ghost copies, both colours */
        es_color(ctx, 0, 1, false);
    }
    for (int l = 1; l <= q; l++) {
        Level &lev = ctx->lv[l], &lc = ctx->lv[l - 1];
        k_prolong(lc.g, lc.f[MG3D_U], lev.g, lev.f[MG3D_U], 0, s); /* :1331 */
        es_fill(ctx, l, l == ctx->L - 1 ? 1. : 0.);
        es_smooth(ctx, l, 1, ctx->iters);                       /* :1341 */
        if (l == q)
            k_residual(lev.g, lev.f[MG3D_U], lev.f[MG3D_D], es_operator(lev), nullptr, ctx->partials, ctx->sumsq + slot,
                       s);                                      /* :1354 */
    }
    return launch_ok_es("mg3d_es_vcycles");
}

extern "C" int mg3d_es_vcycles(mg3d_ctx *ctx, int count, double *norms)
{
    CHK(mg3d_drop_carry(ctx));
    if (ctx && ctx->eps.set()) /* the mixed-boundary problem has a constant coefficient (checked before its own state) */
        return fail(MG3D_ERR_STATE, "mg3d_es_vcycles: the context has a variable coefficient (mg3d_ctx_set_coefficient); set it to NULL");
    if (ctx && ctx->periodic) /* the mixed-boundary problem is defined on six faces */
        return fail(MG3D_ERR_STATE, "mg3d_es_vcycles: the context has periodic axes (mg3d_ctx_set_periodic); set them to 0");
    if (ctx && ctx->neumann)
        return fail(MG3D_ERR_STATE, "mg3d_es_vcycles: the context has Neumann faces (mg3d_ctx_set_neumann); set them to 0");
    if (ctx && ctx->mask.set())
        return fail(MG3D_ERR_STATE, "mg3d_es_vcycles: the context has fixed points (mg3d_ctx_set_mask); set the mask to NULL");
    if (ctx && ctx->sfield.set())
        return fail(MG3D_ERR_STATE, "mg3d_es_vcycles: the context has a screening field (mg3d_ctx_set_shift_field); set it to NULL");
    if (!ctx || count < 0 || !ctx->have_es)
        return fail(MG3D_ERR_ARG, "mg3d_es_vcycles: bad arguments (mg3d_es_setup first)");
    if (ctx->sigma != 0.) /* the mixed-boundary problem keeps the reference's operator */
        return fail(MG3D_ERR_STATE, "mg3d_es_vcycles: the context has a screened operator (mg3d_ctx_set_shift); set the shift to 0");
    if (ctx->L < 2)
        return fail(MG3D_ERR_ARG, "mg3d_es_vcycles: needs at least two levels");
    const int batch = ctx->sumsq_slots - 1;
    for (int done = 0; done < count;) {
        const int nb = count - done < batch ? count - done : batch;
        for (int c = 0; c < nb; c++)
            CHK(es_vcycle(ctx, ctx->L - 1, c));
        HIPCHK(hipMemcpyAsync(ctx->h_sumsq, ctx->sumsq, nb * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (norms)
            for (int c = 0; c < nb; c++)
                norms[done + c] = sqrt(ctx->h_sumsq[c]);
        done += nb;
    }
    return MG3D_OK;
}
