/*
 * mg3d_nl.hip -- nonlinear Poisson on the device (mg3d_nl_setup, mg3d_nl_set_weight, mg3d_nl_residual, mg3d_nl_solve,
 * include/mg3d.h): damped Newton-multigrid for  A u - g0*g*phi(beta*(u - uref)) = d,  phi = exp or sinh, with the context's
 * operator A and boundaries.
 *
 * Newton in correction form.  With F(x) = d - (A x - gp*phi(w)) the residual and s(x) = gp*beta*phi'(w) >= 0 the derivative
 * of the nonlinear term, the step solves  (A - s) delta = F  -- the context's own operator with s as its screening field
 * (mg3d_ctx_set_shift_field), so the linear solve is the context's own: mg3d_vcycles or mg3d_wpcg_solve from delta = 0 with F
 * as the right-hand side.  One launch (k_nl_eval, mg3d_kernels.hip) forms F into d of the finest level, s into the finest level
 * of the screening field, the partial sums of F^2 and the count of s that are not finite; the field's install path
 * (mg3d_operator.hip) restricts s down the hierarchy and rebuilds the coarse factor.  The step is damped by backtracking on
 * ||F||: t = x + lambda*delta (k_nl_trial), lambda halved until ||F(t)|| < (1 - 1e-4*lambda)*||F(x)|| -- an undamped step of
 * the exponential overshoots by orders of magnitude from a cold start (tests/test_nl_ref_host.py keeps the case).
 *
 * Where the vectors live.  x, t and the caller's d are three fields of the library's own (nl_v); during a solve u of the finest
 * level holds delta and d holds F, so that the context's solvers run as they are; on every way out u := x and d := the
 * caller's, copied back whole.  Every evaluation ends with one host synchronisation (the norm, the count).  The new launches
 * count under the kernel timer MG3D_K_PACK.
 */
#include "mg3d_ctx.h"

#include <math.h>
#include <stdio.h>

#include <utility>
#include <vector>

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

extern "C" int mg3d_nl_setup(mg3d_ctx *ctx, int kind, double g0, double beta, double uref)
{
    if (!ctx)
        return fail(MG3D_ERR_ARG, "mg3d_nl_setup: NULL context");
    if ((kind != MG3D_NL_EXP && kind != MG3D_NL_SINH) || !(g0 >= 0.) || !isfinite(g0) || !(beta > 0.) || !isfinite(beta) ||
        !isfinite(uref))
        return fail(MG3D_ERR_ARG, "mg3d_nl_setup: need a kind of MG3D_NL_*, g0 >= 0, beta > 0, all finite (%d, %g, %g, %g)", kind,
                    g0, beta, uref);
    ctx->nl_set = true;
    ctx->nl_kind = kind;
    ctx->nl_g0 = g0 == 0. ? 0. : g0; /* (-0 is stored as +0) */
    ctx->nl_beta = beta;
    ctx->nl_uref = uref;
    return MG3D_OK;
}

/* a field of the finest level in its padded layout, zeroed, unless *p holds one already */
static int nl_field_alloc(mg3d_ctx *ctx, double **p, const char *who, const char *what)
{
    if (*p)
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
        return mg3d_alloc_fail(e, who, what);
    }
    *p = v;
    return MG3D_OK;
}

extern "C" int mg3d_nl_set_weight(mg3d_ctx *ctx, const double *g)
{
    static const char who[] = "mg3d_nl_set_weight";
    if (!ctx)
        return fail(MG3D_ERR_ARG, "%s: NULL context", who);
    if (!g) {
        ctx->nl_has_g = false;
        return MG3D_OK;
    }
    CHK(mg3d_field_level(ctx, who));
    CHK(mg3d_check_weight_host(ctx, g, "g", who));
    CHK(nl_field_alloc(ctx, &ctx->nl_g, who, "the weight field"));
    const Geom &tg = ctx->lv[ctx->L - 1].g;
    /* (a solve still in flight reads the field: the copy is ordered behind it on the context's stream) */
    hipError_t e = hipMemcpy2DAsync(ctx->nl_g, tg.pitch * sizeof(double), g, tg.N * sizeof(double), tg.N * sizeof(double),
                                    (size_t)tg.N * tg.N, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess)
        return fail(MG3D_ERR_HIP, "%s: upload: %s", who, hipGetErrorString(e));
    ctx->nl_has_g = true;
    return MG3D_OK;
}

/* the same from a device array (mg3d_array): checked on the device (one host synchronisation), then packed into the weight
 * field on the context's stream, behind what the caller's stream did to the array */
extern "C" int mg3d_nl_set_weight_device(mg3d_ctx *ctx, const mg3d_array *g, void *stream)
{
    static const char who[] = "mg3d_nl_set_weight_device";
    if (!ctx)
        return fail(MG3D_ERR_ARG, "%s: NULL context", who);
    if (!g) {
        ctx->nl_has_g = false;
        return MG3D_OK;
    }
    CHK(mg3d_field_level(ctx, who));
    CHK(mg3d_array_check(ctx, g, false, who));
    CHK(mg3d_stream_join(ctx, (hipStream_t)stream, false, who));
    CHK(mg3d_check_weight_device(ctx, *g, "g", who));
    CHK(nl_field_alloc(ctx, &ctx->nl_g, who, "the weight field"));
    const int q = ctx->L - 1;
    {
        StageScope kt(ctx, q, MG3D_K_PACK, true);
        k_pack(ctx->lv[q].g, ctx->nl_g, *g, ctx->stream);
    }
    CHK(mg3d_launch_ok(who));
    ctx->nl_has_g = true;
    return mg3d_stream_join(ctx, (hipStream_t)stream, true, who);
}

/* One evaluation at v with right-hand side d: F (NULL: not stored), sf (NULL: not wanted), n = ||F||, bad = how many sf are
 * not finite.  One host synchronisation.  (With sf the context has io_chk.) */
static int nl_eval(mg3d_ctx *ctx, const char *who, const double *v, const double *d, double *F, double *sf, double &n,
                   unsigned long long &bad)
{
    const int q = ctx->L - 1;
    const Level &top = ctx->lv[q];
    hipStream_t s = ctx->stream;
    bad = 0;
    if (sf)
        HIPCHK(hipMemsetAsync(ctx->io_chk, 0, sizeof(unsigned long long), s));
    int np;
    {
        StageScope kt(ctx, q, MG3D_K_PACK, true);
        np = k_nl_eval(top.g, v, d, mg3d_level_operator(ctx, q, false), ctx->nl_kind, ctx->nl_has_g ? ctx->nl_g : nullptr,
                       ctx->nl_g0, ctx->nl_beta, ctx->nl_uref, F, sf, ctx->partials, ctx->sumsq, ctx->io_chk, s);
    }
    if (np < 0)
        return fail(MG3D_ERR_STATE, "%s: the level has no launch shape", who);
    CHK(mg3d_launch_ok(who));
    HIPCHK(hipMemcpyAsync(ctx->h_sumsq, ctx->sumsq, sizeof(double), hipMemcpyDeviceToHost, s));
    if (sf)
        HIPCHK(hipMemcpyAsync(&bad, ctx->io_chk, sizeof bad, hipMemcpyDeviceToHost, s));
    CHK(mg3d_sync(ctx));
    n = sqrt(ctx->h_sumsq[0]);
    return MG3D_OK;
}

extern "C" int mg3d_nl_residual(mg3d_ctx *ctx, int store, double *norm)
{
    static const char who[] = "mg3d_nl_residual";
    if (!ctx)
        return fail(MG3D_ERR_ARG, "%s: NULL context", who);
    if (!ctx->nl_set)
        return fail(MG3D_ERR_STATE, "%s: mg3d_nl_setup was not called", who);
    CHK(mg3d_field_level(ctx, who));
    CHK(mg3d_drop_carry(ctx));
    const int q = ctx->L - 1;
    const Level &top = ctx->lv[q];
    double n = 0.;
    unsigned long long bad = 0;
    CHK(nl_eval(ctx, who, top.f[MG3D_U], top.f[MG3D_D], store ? top.f[MG3D_R] : nullptr, nullptr, n, bad));
    if (store)
        mg3d_ctx_touched(ctx, MG3D_R, q);
    if (norm)
        *norm = n;
    return MG3D_OK;
}

/* would A - s be singular whatever u is: the context alone is (every axis closed, sigma = 0, no fixed unknown) and g0*g is
 * > 0 at no unknown.  The weight's positive entries are counted as the screening field's are (k_field_count), under the
 * present boundary masks; one host synchronisation, in this case alone */
static int nl_singular(mg3d_ctx *ctx, const char *who, bool &singular)
{
    singular = false;
    bool closed = ctx->sigma == 0. && ctx->mask.count[1] == 0;
    for (int ax = 0; ax < 3; ax++)
        closed = closed && ((ctx->periodic >> ax & 1) || (ctx->neumann >> (2 * ax) & 3) == 3);
    if (!closed)
        return MG3D_OK;
    if (ctx->nl_g0 == 0.) {
        singular = true;
        return MG3D_OK;
    }
    if (!ctx->nl_has_g)
        return MG3D_OK;
    if (!ctx->io_chk)
        CHK(mg3d_device_alloc((void **)&ctx->io_chk, 2 * sizeof(unsigned long long), who));
    unsigned long long pos = 0;
    HIPCHK(hipMemsetAsync(ctx->io_chk, 0, sizeof pos, ctx->stream));
    k_field_count(ctx->lv[ctx->L - 1].g, ctx->nl_g, mg3d_ctx_bc(ctx), ctx->io_chk, ctx->stream);
    HIPCHK(hipMemcpyAsync(&pos, ctx->io_chk, sizeof pos, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    CHK(mg3d_launch_ok(who));
    singular = pos == 0;
    return MG3D_OK;
}

struct NlAsk {
    int max_newton, method, cycles, max_halvings;
    double rtol_lin, rtol, atol;
    double *norms;
};

/* the finest level's field holds s(x): onto every level, and the factor of A - s */
static int nl_install(mg3d_ctx *ctx, const char *who)
{
    CHK(mg3d_sfield_rebuild(ctx, who));
    return mg3d_operator_changed(ctx);
}

/* the iteration of a checked call whose fields exist: x, t, f are nl_v; u and d of the finest level are the solve's from the
 * first evaluation on.  installed: the lower levels of the field and the factor are those of the finest level's s */
static int nl_iterate(mg3d_ctx *ctx, const char *who, const NlAsk &a, mg3d_nl_info &o, bool &installed)
{
    const int q = ctx->L - 1, bc = mg3d_ctx_bc(ctx);
    hipStream_t s = ctx->stream;
    const size_t bytes = ctx->lv[q].elems * sizeof(double);
    double *const f = ctx->nl_v[2];
    double n = 0., n_t = 0.;
    unsigned long long bad = 0;
    CHK(nl_eval(ctx, who, ctx->nl_v[0], f, ctx->lv[q].f[MG3D_D], ctx->sfield.lv[q], n, bad));
    o.norm0 = o.norm = n;
    if (a.norms)
        a.norms[0] = n;
    if (bad || !isfinite(n)) /* nothing to linearise about: s(x) is not a field the operator can take */
        return fail(MG3D_ERR_ARG, "%s: the residual or the linearisation at the initial u is not finite (||F|| = %g, %llu entries of s)",
                    who, n, bad);
    std::vector<double> cyc;
    if (a.method == MG3D_STEP_VCYCLES) {
        try {
            cyc.resize((size_t)a.cycles);
        } catch (...) {
            return fail(MG3D_ERR_ALLOC, "%s: %d norms do not fit", who, a.cycles);
        }
    }
    for (;;) {
        o.converged = n <= fmax(a.atol, a.rtol * o.norm0);
        if (o.converged || o.iterations >= a.max_newton)
            return MG3D_OK;
        CHK(nl_install(ctx, who));
        installed = true;
        /* (A - s) delta = F from delta = 0, Dirichlet points included: the correction's values there */
        CHK(mg3d_drop_carry(ctx));
        HIPCHK(hipMemsetAsync(ctx->lv[q].f[MG3D_U], 0, bytes, s));
        if (a.method == MG3D_STEP_VCYCLES) {
            CHK(mg3d_vcycles(ctx, a.cycles, cyc.data()));
            o.linear_iterations += a.cycles;
        } else {
            mg3d_wpcg_info w = {};
            CHK(mg3d_wpcg_solve(ctx, a.rtol_lin, 0., a.cycles, nullptr, &w));
            o.linear_iterations += w.iterations;
        }
        CHK(mg3d_drop_carry(ctx)); /* the last cycle may have run ahead */
        const double *const delta = ctx->lv[q].f[MG3D_U];
        double lambda = 1.;
        bool accepted = false;
        for (int trial = 0; trial <= a.max_halvings; trial++) {
            {
                StageScope kt(ctx, q, MG3D_K_PACK, true);
                if (k_nl_trial(ctx->lv[q].g, bc, ctx->nl_v[0], delta, lambda, ctx->nl_v[1], ctx->mask.at(q), s) < 0)
                    return fail(MG3D_ERR_STATE, "%s: the level has no launch shape", who);
            }
            installed = false; /* the finest level's field is s(t) from here */
            CHK(nl_eval(ctx, who, ctx->nl_v[1], f, ctx->lv[q].f[MG3D_D], ctx->sfield.lv[q], n_t, bad));
            if (isfinite(n_t) && bad == 0 && n_t < (1. - 1e-4 * lambda) * n) {
                accepted = true;
                break;
            }
            if (trial < a.max_halvings) {
                lambda *= 0.5;
                o.halvings++;
            }
        }
        if (!accepted) { /* back to F(x) and s(x); the caller sees converged = 0 */
            CHK(nl_eval(ctx, who, ctx->nl_v[0], f, ctx->lv[q].f[MG3D_D], ctx->sfield.lv[q], n, bad));
            return MG3D_OK;
        }
        std::swap(ctx->nl_v[0], ctx->nl_v[1]);
        n = n_t;
        o.iterations++;
        o.last_lambda = lambda;
        o.norm = n;
        if (a.norms)
            a.norms[o.iterations] = n;
    }
}

extern "C" int mg3d_nl_solve(mg3d_ctx *ctx, int max_newton, int method, int cycles, double rtol_lin, double rtol, double atol,
                             int max_halvings, double *norms, mg3d_nl_info *info)
{
    static const char who[] = "mg3d_nl_solve";
    if (!ctx)
        return fail(MG3D_ERR_ARG, "%s: NULL context", who);
    if (max_newton < 0 || (method != MG3D_STEP_VCYCLES && method != MG3D_STEP_WPCG) || cycles < 1 || max_halvings < 0)
        return fail(MG3D_ERR_ARG, "%s: need max_newton >= 0, a method of MG3D_STEP_*, cycles >= 1, max_halvings >= 0 (%d, %d, %d, %d)",
                    who, max_newton, method, cycles, max_halvings);
    if (!(rtol >= 0.) || !isfinite(rtol) || !(atol >= 0.) || !isfinite(atol) ||
        (method == MG3D_STEP_WPCG && (!(rtol_lin >= 0.) || !isfinite(rtol_lin))))
        return fail(MG3D_ERR_ARG, "%s: rtol, atol and rtol_lin must be finite and >= 0 (%g, %g, %g)", who, rtol, atol, rtol_lin);
    if (!ctx->nl_set)
        return fail(MG3D_ERR_STATE, "%s: mg3d_nl_setup was not called", who);
    if (ctx->sfield.set() && !ctx->sfield_nl)
        return fail(MG3D_ERR_STATE, "%s: the context has a screening field of the caller's (mg3d_ctx_set_shift_field): the call "
                                    "installs its own", who);
    if (ctx->have_es)
        return fail(MG3D_ERR_STATE, "%s: the context holds the mixed-boundary factor of mg3d_es_setup", who);
    if (!ctx->have_lu || !ctx->lu_built)
        return fail(MG3D_ERR_STATE, "%s: no coarse factor of mg3d_ctx_build_coarse (every linearisation rebuilds it)", who);
    CHK(mg3d_field_level(ctx, who));
    bool singular = false;
    CHK(nl_singular(ctx, who, singular));
    if (singular)
        return fail(MG3D_ERR_STATE, "%s: the linearised operator would be singular: every axis closed, sigma = 0, no fixed "
                                    "unknown, and g0*g > 0 at no unknown", who);
    CHK(mg3d_drop_carry(ctx)); /* a cycle that has run ahead is finished first */
    /* everything that can fail for want of memory, before the first write */
    for (int t = 0; t < 3; t++)
        CHK(nl_field_alloc(ctx, &ctx->nl_v[t], who, "the solve's fields"));
    const int q = ctx->L - 1;
    hipStream_t s = ctx->stream;
    const size_t bytes = ctx->lv[q].elems * sizeof(double);
    const bool fresh = !ctx->sfield.set();
    CHK(mg3d_sfield_prepare(ctx, who));
    ctx->sfield_nl = true;
    if (fresh) /* the kernel writes the unknowns: the Dirichlet points of s, which the restriction injects, are 0. */
        HIPCHK(hipMemsetAsync(ctx->sfield.lv[q], 0, bytes, s));
    /* x := u, t := u (its Dirichlet points: no pass writes them), f := d */
    HIPCHK(hipMemcpyAsync(ctx->nl_v[0], ctx->lv[q].f[MG3D_U], bytes, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->nl_v[1], ctx->lv[q].f[MG3D_U], bytes, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(ctx->nl_v[2], ctx->lv[q].f[MG3D_D], bytes, hipMemcpyDeviceToDevice, s));
    mg3d_ctx_touched(ctx, MG3D_D, q); /* d is the solve's from here: no zero map of it */
    const NlAsk ask = {max_newton, method, cycles, max_halvings, rtol_lin, rtol, atol, norms};
    mg3d_nl_info o = {};
    bool installed = false;
    int rc = nl_iterate(ctx, who, ask, o, installed);
    /* every way out: s(x) on all levels, u := x, d := f */
    if (rc == MG3D_OK && !installed)
        rc = nl_install(ctx, who);
    (void)mg3d_drop_carry(ctx);
    hipError_t e = hipMemcpyAsync(ctx->lv[q].f[MG3D_U], ctx->nl_v[0], bytes, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess)
        e = hipMemcpyAsync(ctx->lv[q].f[MG3D_D], ctx->nl_v[2], bytes, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess)
        e = hipStreamSynchronize(s);
    mg3d_ctx_touched(ctx, MG3D_D, q, false, MG3D_WROTE_CALLER); /* the caller's d again */
    if (rc == MG3D_OK && e != hipSuccess)
        rc = fail(MG3D_ERR_HIP, "%s: putting u and d back: %s", who, hipGetErrorString(e));
    if (rc != MG3D_OK && ctx->sfield.set()) {
        /* no field of a linearisation that did not complete stays behind (the first error is the one reported) */
        char first[512];
        snprintf(first, sizeof first, "%s", mg3d_last_error());
        (void)mg3d_ctx_set_shift_field(ctx, nullptr);
        (void)fail(rc, "%s", first);
    }
    if (info)
        *info = o;
    return rc;
}
