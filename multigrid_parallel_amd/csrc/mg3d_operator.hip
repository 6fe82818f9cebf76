/*
 * mg3d_operator.hip -- what the operator of a context is made of, behind the C ABI (include/mg3d.h): the shift sigma, the
 * three per-level fields (the coefficient eps, the fixed-point bytes, the screening field s; OperatorField, mg3d_ctx.h) and
 * the boundary masks (periodic axes, Neumann faces).
 *
 * Every setter keeps one contract.  The argument is checked before anything changes; a cycle that has run ahead is finished
 * with the operator it started with (mg3d_drop_carry); whatever can fail for want of memory is allocated before the first
 * write; nothing half-installed stays behind a HIP error; there is one host synchronisation behind the writes, behind which
 * the caller's array has been read; and the coarse factor is rebuilt or dropped (operator_changed).  The steps the fields
 * share are written once, below; the setters call them in their own order.
 */
#include "mg3d_ctx.h"

#include <math.h>
#include <stdio.h>

#include <algorithm>

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

/* the operator of the context changed (sigma, a field, the boundary masks): a factor of mg3d_ctx_build_coarse is built again
 * for the spacing it was built with, one installed by mg3d_ctx_set_lu (or mg3d_es_setup) is dropped: the next cycle returns
 * MG3D_ERR_STATE until a factor is set again */
static int operator_changed(mg3d_ctx *ctx)
{
    if (!ctx->have_lu)
        return MG3D_OK;
    if (ctx->lu_built) {
        const int rc = mg3d_ctx_build_coarse(ctx, ctx->lu_h);
        if (rc == MG3D_OK)
            return MG3D_OK;
        /* no factor of the old operator may survive next to the new one */
        (void)hipStreamSynchronize(ctx->stream);
        mg3d_free_lu(ctx);
        ctx->lu_built = false;
        return rc;
    }
    HIPCHK(hipStreamSynchronize(ctx->stream)); /* a solve still in flight reads the factor */
    mg3d_free_lu(ctx);
    ctx->have_es = false;
    return MG3D_OK;
}

/* The screened operator Delta_h u - sigma u = d on every level (LevelOp).  The argument is checked before anything
 * changes.  Then: a cycle that has run ahead is finished with the operator it started with (mg3d_drop_carry), and a new
 * sigma rebuilds or drops the factor (operator_changed). */
extern "C" int mg3d_ctx_set_shift(mg3d_ctx *ctx, double sigma)
{
    if (!ctx || !(sigma >= 0.) || !isfinite(sigma))
        return fail(MG3D_ERR_ARG, "mg3d_ctx_set_shift: %s", ctx ? "sigma must be finite and >= 0" : "NULL context");
    CHK(mg3d_drop_carry(ctx));
    if (sigma == ctx->sigma)
        return MG3D_OK;
    ctx->sigma = sigma == 0. ? 0. : sigma; /* (-0 is stored as +0) */
    return operator_changed(ctx);
}

extern "C" int mg3d_ctx_get_shift(const mg3d_ctx *ctx, double *sigma)
{
    if (!ctx || !sigma)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_get_shift: NULL argument");
    *sigma = ctx->sigma;
    return MG3D_OK;
}

/* the two 64-bit device words of the value check and of the counts, and the padded level-0 right-hand side of the direct
 * solve (k_coarse_rhs): allocated on first use, freed with the context */
static int ensure_io_chk(mg3d_ctx *ctx, const char *who)
{
    return ctx->io_chk ? MG3D_OK : mg3d_device_alloc((void **)&ctx->io_chk, 2 * sizeof(unsigned long long), who);
}
static int ensure_per_b(mg3d_ctx *ctx, const char *who)
{
    return ctx->per_b ? MG3D_OK : mg3d_device_alloc((void **)&ctx->per_b, ctx->lv[0].elems * sizeof(double), who);
}

/* ------------------------------------------------------- the steps the fields share (OperatorField<T>, mg3d_ctx.h) */

/* Allocate: one array per level in the padded layout unless the field is set already, all or nothing -- f is untouched
 * when an allocation fails.  Bytes are zeroed (their row padding is read as "not fixed"); doubles are not */
template <class T> static int field_alloc(mg3d_ctx *ctx, OperatorField<T> &f, const char *who)
{
    if (f.set())
        return MG3D_OK;
    const bool bytes = sizeof(T) == 1;
    std::vector<T *> a(ctx->L, nullptr);
    for (int l = 0; l < ctx->L; l++) {
        int rc = mg3d_device_alloc((void **)&a[l], ctx->lv[l].elems * sizeof(T), who);
        if (rc == MG3D_OK && bytes) {
            const hipError_t e = hipMemsetAsync(a[l], 0, ctx->lv[l].elems, ctx->stream);
            if (e != hipSuccess)
                rc = mg3d_alloc_fail(e, who, "hipMalloc");
        }
        if (rc == MG3D_OK)
            continue;
        if (bytes)
            (void)hipStreamSynchronize(ctx->stream); /* (memsets of the levels before this one) */
        for (T *q : a)
            if (q)
                (void)hipFree(q);
        return rc;
    }
    f.lv = a;
    return MG3D_OK;
}

/* Free: a field leaves the context (mg3d_field_free), and with the screening field the eps = 1 it ran over */
template <class T> static void field_drop(mg3d_ctx *ctx, OperatorField<T> &f)
{
    mg3d_field_free(f);
    if (!ctx->sfield.set())
        mg3d_field_free(ctx->ones);
}

/* Clear (the setter's NULL): a cycle that has run ahead is finished, a context without the field is left as it is, and
 * launches in flight read the field, hence the synchronisation before it is freed */
template <class T> static int field_clear(mg3d_ctx *ctx, OperatorField<T> &f)
{
    CHK(mg3d_drop_carry(ctx));
    if (!f.set())
        return MG3D_OK;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    field_drop(ctx, f);
    return operator_changed(ctx);
}

/* Abandon: a field whose levels, host copy or counts could not be brought up to date (a HIP error) -- no half-installed
 * field stays behind: the context is left without it, and without a factor of the operator that had it.  The first error is
 * the one reported.  (The mask and the screening field come here; eps has no such step behind coefficient_written.) */
template <class T> static int field_abandon(mg3d_ctx *ctx, OperatorField<T> &f, int rc)
{
    (void)hipStreamSynchronize(ctx->stream);
    field_drop(ctx, f);
    (void)operator_changed(ctx);
    return rc;
}

/* the one text of a refused entry: the lowest bad dense index and its value; `bad` (the device check's): how many there are */
static int bad_entry(const char *who, const char *name, bool zero_ok, long long p, double v, unsigned long long bad = 0)
{
    char more[48] = "";
    if (bad)
        snprintf(more, sizeof more, "; %llu entries are not", bad);
    return fail(MG3D_ERR_ARG, "%s: %s[%lld] = %g (every entry must be finite and %s%s)", who, name, p, v, zero_ok ? ">= 0" : "> 0",
                more);
}

/* Host check of the caller's dense N^3 doubles: every entry finite and > 0 (ZERO_OK: >= 0; a template argument as in
 * coef_check_kernel, the loop runs over 17 million entries at 257^3).  With periodic axes the duplicates are not read:
 * neither checked nor kept (their sources are copied over them) */
template <bool ZERO_OK> static int check_host(const mg3d_ctx *ctx, const double *a, const char *name, const char *who)
{
    const int N = ctx->lv[ctx->L - 1].g.N;
    const long long n = (long long)N * N * N;
    const int ax = ctx->periodic;
    auto dup = [&](long long q) {
        return ((ax & 1) && q / ((long long)N * N) == N - 1) || ((ax & 2) && (q / N) % N == N - 1) || ((ax & 4) && q % N == N - 1);
    };
    for (long long p = 0; p < n; p++)
        if ((!(ZERO_OK ? a[p] >= 0. : a[p] > 0.) || !isfinite(a[p])) && !(ax && dup(p)))
            return bad_entry(who, name, ZERO_OK, p, a[p]);
    return MG3D_OK;
}

/* Device check of a caller's array, the same rule: a launch that reads the array as given; its two integers -- how many
 * bad entries, the lowest dense index among them -- cross to the host in io_chk.  One host synchronisation.  (The context
 * has io_chk, and its stream has been joined with the caller's.) */
static int check_device(mg3d_ctx *ctx, const mg3d_array &a, bool zero_ok, const char *name, const char *who)
{
    const Geom &g = ctx->lv[ctx->L - 1].g;
    const int N = g.N;
    unsigned long long chk[2] = {0, 0};
    HIPCHK(hipMemsetAsync(ctx->io_chk, 0, sizeof(unsigned long long), ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->io_chk + 1, 0xff, sizeof(unsigned long long), ctx->stream));
    (zero_ok ? k_field_check : k_coef_check)(g, a, ctx->periodic, ctx->io_chk, ctx->stream);
    HIPCHK(hipMemcpyAsync(chk, ctx->io_chk, sizeof chk, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    CHK(mg3d_launch_ok(who));
    if (chk[0] == 0)
        return MG3D_OK;
    const long long p = (long long)chk[1];
    const long long off = a.stride[0] * (p / ((long long)N * N)) + a.stride[1] * ((p / N) % N) + a.stride[2] * (p % N);
    double v = 0.;
    float v32 = 0.f;
    if (a.dtype == MG3D_F32) {
        HIPCHK(hipMemcpy(&v32, (const float *)a.ptr + off, sizeof v32, hipMemcpyDeviceToHost));
        v = (double)v32;
    } else {
        HIPCHK(hipMemcpy(&v, (const double *)a.ptr + off, sizeof v, hipMemcpyDeviceToHost));
    }
    return bad_entry(who, name, zero_ok, p, v, chk[0]);
}

/* the finest level of a field of doubles from the caller's dense host array, or packed from the caller's device array:
 * enqueued only (the setter's synchronisation comes behind the coarser levels) */
static int top_from_host(mg3d_ctx *ctx, OperatorField<double> &f, const double *host)
{
    const Geom &g = ctx->lv[ctx->L - 1].g;
    HIPCHK(hipMemcpy2DAsync(f.lv[ctx->L - 1], g.pitch * sizeof(double), host, g.N * sizeof(double), g.N * sizeof(double),
                            (size_t)g.N * g.N, hipMemcpyHostToDevice, ctx->stream));
    return MG3D_OK;
}
static void top_from_device(mg3d_ctx *ctx, OperatorField<double> &f, const mg3d_array &a)
{
    StageScope kt(ctx, ctx->L - 1, MG3D_K_PACK, true);
    k_pack(ctx->lv[ctx->L - 1].g, f.lv[ctx->L - 1], a, ctx->stream);
}

/* Download: one level into a dense host array.  Enqueued only */
template <class T> static int level_to_host(mg3d_ctx *ctx, const OperatorField<T> &f, int level, T *host)
{
    const Geom &g = ctx->lv[level].g;
    HIPCHK(hipMemcpy2DAsync(host, g.N * sizeof(T), f.lv[level], g.pitch * sizeof(T), g.N * sizeof(T), (size_t)g.N * g.N,
                            hipMemcpyDeviceToHost, ctx->stream));
    return MG3D_OK;
}

/* Copy level 0 to its dense host vector, for the coarse matrix.  Enqueued only: the setter keeps its one synchronisation */
template <class T> static int level0_to_host(mg3d_ctx *ctx, OperatorField<T> &f)
{
    const size_t N0 = (size_t)ctx->lv[0].g.N;
    f.host0.resize(N0 * N0 * N0);
    return level_to_host(ctx, f, 0, f.host0.data());
}

/* Count: the unknowns that the field singles out on level 0 and on the finest level under the present boundary masks --
 * the fixed ones of a mask, those with s > 0 of a screening field -- through the two words of io_chk into f.count.
 * Enqueued only: the counts are there behind the next synchronisation.  (The context has io_chk.) */
static void count_launch(const Geom &g, const unsigned char *m, int bc, unsigned long long *out, hipStream_t s)
{
    k_mask_count(g, m, bc, out, s);
}
static void count_launch(const Geom &g, const double *f, int bc, unsigned long long *out, hipStream_t s)
{
    k_field_count(g, f, bc, out, s);
}
template <class T> static int field_count(mg3d_ctx *ctx, OperatorField<T> &f)
{
    const int top = ctx->L - 1, bc = mg3d_ctx_bc(ctx);
    HIPCHK(hipMemsetAsync(ctx->io_chk, 0, sizeof f.count, ctx->stream));
    count_launch(ctx->lv[0].g, f.lv[0], bc, ctx->io_chk, ctx->stream);
    count_launch(ctx->lv[top].g, f.lv[top], bc, ctx->io_chk + 1, ctx->stream);
    HIPCHK(hipMemcpyAsync(f.count, ctx->io_chk, sizeof f.count, hipMemcpyDeviceToHost, ctx->stream));
    return MG3D_OK;
}

/* what the host keeps of a mask or a screening field whose levels have been written: the counts and level 0.  One host
 * synchronisation -- behind it a caller's array has been read */
template <class T> static int field_to_host(mg3d_ctx *ctx, OperatorField<T> &f, const char *who)
{
    CHK(field_count(ctx, f));
    CHK(level0_to_host(ctx, f));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return mg3d_launch_ok(who);
}

/* the three mg3d_ctx_has_* and the three getters of a level as the kernels use it */
template <class T> static int field_has(const mg3d_ctx *ctx, OperatorField<T> mg3d_ctx::*f, int *on, const char *who)
{
    if (!ctx || !on)
        return fail(MG3D_ERR_ARG, "%s: NULL argument", who);
    *on = (ctx->*f).set() ? 1 : 0;
    return MG3D_OK;
}
template <class T>
static int field_get(mg3d_ctx *ctx, OperatorField<T> mg3d_ctx::*f, int level, T *host, const char *who, const char *what)
{
    CHK(mg3d_check_field_level(ctx, 0, level, who));
    if (!host)
        return fail(MG3D_ERR_ARG, "%s: NULL host pointer", who);
    if (!(ctx->*f).set())
        return fail(MG3D_ERR_STATE, "%s: no %s set", who, what);
    CHK(level_to_host(ctx, ctx->*f, level, host));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MG3D_OK;
}

/* eps = 1 at the N^3 points of every level, for a context with a field and no coefficient: the eps kernels alone have the
 * field form.  Written by k_pack from one double (every stride 0), which io_chk holds for the length of these launches --
 * whoever uses io_chk next on the stream sets it first.  (The context has io_chk.) */
static int ensure_ones(mg3d_ctx *ctx, const char *who)
{
    if (ctx->ones.set())
        return MG3D_OK;
    static const double one = 1.;
    CHK(field_alloc(ctx, ctx->ones, who));
    HIPCHK(hipMemcpyAsync(ctx->io_chk, &one, sizeof one, hipMemcpyHostToDevice, ctx->stream));
    const mg3d_array src = {ctx->io_chk, MG3D_F64, {0, 0, 0}};
    for (int l = 0; l < ctx->L; l++)
        k_pack(ctx->lv[l].g, ctx->ones.lv[l], src, ctx->stream);
    return MG3D_OK;
}

/* ------------------------------------------------------------------------------------ the variable coefficient */

/* what both forms of mg3d_ctx_set_coefficient do once the finest level's eps is written: its duplicates, the injections,
 * level 0's eps back on the host for the coarse matrix, one host synchronisation -- behind it the caller's array has been
 * read --, the coarse factor */
static int coefficient_written(mg3d_ctx *ctx, const char *who)
{
    const int L = ctx->L;
    k_per_refresh(ctx->lv[L - 1].g, ctx->eps.lv[L - 1], ctx->periodic, ctx->stream);
    for (int l = L - 1; l >= 1; l--)
        k_coef_inject(ctx->lv[l].g, ctx->eps.lv[l], ctx->lv[l - 1].g, ctx->eps.lv[l - 1], ctx->stream);
    CHK(level0_to_host(ctx, ctx->eps));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    CHK(mg3d_launch_ok(who));
    /* (a screening field ran the eps kernels over eps = 1 until now; nothing in flight reads it any more) */
    mg3d_field_free(ctx->ones);
    return operator_changed(ctx);
}

/* The variable-coefficient operator div(eps grad u) - sigma u = d (mg3d_kernels.hip) on every level: eps of the finest level
 * as given, of each coarser one by injection.  The array is checked before anything changes; then, as for a new sigma, a
 * cycle that has run ahead is finished with the operator it started with and the coarse factor is rebuilt or dropped.
 * NULL: back to the constant-coefficient operator and its fused schedules. */
extern "C" int mg3d_ctx_set_coefficient(mg3d_ctx *ctx, const double *eps)
{
    static const char who[] = "mg3d_ctx_set_coefficient";
    if (!ctx)
        return fail(MG3D_ERR_ARG, "%s: NULL context", who);
    if (eps)
        CHK(check_host<false>(ctx, eps, "eps", who));
    CHK(mg3d_drop_carry(ctx));
    if (!eps) {
        if (ctx->eps.set() && ctx->sfield.set()) { /* a screening field stays: its eps kernels go on over eps = 1 */
            CHK(ensure_io_chk(ctx, who));
            CHK(ensure_ones(ctx, who));
        }
        return field_clear(ctx, ctx->eps);
    }
    CHK(field_alloc(ctx, ctx->eps, who));
    CHK(top_from_host(ctx, ctx->eps, eps));
    return coefficient_written(ctx, who); /* (the host array may go once the call returns) */
}

/* mg3d_ctx_set_coefficient from a device array, step for step: the check, then the carried cycle, the pack into the finest
 * level's eps, the duplicates, the injections (coefficient_written).  Two host synchronisations; behind the second one the
 * array has been read, so the caller's stream needs no event of ours. */
extern "C" int mg3d_ctx_set_coefficient_device(mg3d_ctx *ctx, const mg3d_array *eps, void *stream)
{
    static const char who[] = "mg3d_ctx_set_coefficient_device";
    if (!ctx)
        return fail(MG3D_ERR_ARG, "%s: NULL context", who);
    if (!eps)
        return mg3d_ctx_set_coefficient(ctx, nullptr);
    CHK(mg3d_array_check(ctx, eps, false, who));
    CHK(ensure_io_chk(ctx, who));
    CHK(mg3d_stream_join(ctx, (hipStream_t)stream, false, who));
    CHK(check_device(ctx, *eps, false, "eps", who));
    CHK(mg3d_drop_carry(ctx));
    CHK(field_alloc(ctx, ctx->eps, "mg3d_ctx_set_coefficient")); /* (reported under the host form's name) */
    top_from_device(ctx, ctx->eps, *eps);
    return coefficient_written(ctx, who);
}

extern "C" int mg3d_ctx_has_coefficient(const mg3d_ctx *ctx, int *on)
{
    return field_has(ctx, &mg3d_ctx::eps, on, "mg3d_ctx_has_coefficient");
}

extern "C" int mg3d_ctx_get_coefficient(mg3d_ctx *ctx, int level, double *host)
{
    return field_get(ctx, &mg3d_ctx::eps, level, host, "mg3d_ctx_get_coefficient", "coefficient");
}

/* ------------------------------------------------------------------------------------------------ fixed points */

/* Levels L-2 .. 0 of the mask from the finest level's stored bytes (its duplicates hold their sources') by the context's
 * rule: injection, or MG3D_MASK_KEEP (k_mask_keep), behind which each coarse level's duplicates take their sources' bytes
 * before the next level reads them -- a duplicate plane sees fewer fine points than its source does.  Enqueued only */
static void mask_coarsen(mg3d_ctx *ctx)
{
    const int bc = mg3d_ctx_bc(ctx);
    for (int l = ctx->L - 1; l >= 1; l--) {
        if (ctx->mask_rule == MG3D_MASK_KEEP) {
            k_mask_keep(ctx->lv[l].g, ctx->mask.lv[l], ctx->lv[l - 1].g, ctx->mask.lv[l - 1], ctx->stream);
            k_mask_refresh(ctx->lv[l - 1].g, ctx->mask.lv[l - 1], bc, ctx->stream);
        } else {
            k_mask_inject(ctx->lv[l].g, ctx->mask.lv[l], ctx->lv[l - 1].g, ctx->mask.lv[l - 1], ctx->stream);
        }
    }
}

/* the mask from a checked device array: the cycle that has run ahead, then everything that can fail for want of memory
 * (nothing has changed when it does), the pack into the finest level (duplicates from their sources), the coarser levels
 * by the context's rule, the counts and level 0's bytes for the coarse matrix, the coarse factor */
static int mask_install(mg3d_ctx *ctx, const mg3d_array &a, const char *who)
{
    const int L = ctx->L;
    CHK(mg3d_drop_carry(ctx));
    CHK(ensure_io_chk(ctx, who));
    CHK(ensure_per_b(ctx, who));
    CHK(field_alloc(ctx, ctx->mask, who));
    {
        StageScope kt(ctx, L - 1, MG3D_K_PACK, true);
        k_mask_pack(ctx->lv[L - 1].g, ctx->mask.lv[L - 1], a, mg3d_ctx_bc(ctx), ctx->stream);
    }
    mask_coarsen(ctx);
    const int rc = field_to_host(ctx, ctx->mask, who);
    if (rc != MG3D_OK)
        return field_abandon(ctx, ctx->mask, rc);
    return operator_changed(ctx);
}

/* Fixed points (mg3d_kernels.hip): one byte per point of every level, the finest level's as given, the others' by the
 * context's coarsening rule (injection unless mg3d_ctx_set_mask_coarsening said otherwise).  NULL: no mask again. */
extern "C" int mg3d_ctx_set_mask(mg3d_ctx *ctx, const unsigned char *mask)
{
    static const char who[] = "mg3d_ctx_set_mask";
    if (!ctx)
        return fail(MG3D_ERR_ARG, "%s: NULL context", who);
    if (!mask)
        return field_clear(ctx, ctx->mask);
    /* through a dense device copy and the pack of the device form: one code path writes the levels */
    const long long N = ctx->lv[ctx->L - 1].g.N, n = N * N * N;
    unsigned char *tmp = nullptr;
    CHK(mg3d_device_alloc((void **)&tmp, (size_t)n, who));
    int out = MG3D_OK;
    const hipError_t cp = hipMemcpyAsync(tmp, mask, (size_t)n, hipMemcpyHostToDevice, ctx->stream);
    if (cp != hipSuccess)
        out = fail(MG3D_ERR_HIP, "%s: hipMemcpyAsync: %s", who, hipGetErrorString(cp));
    else {
        const mg3d_array a = {tmp, MG3D_U8, {N * N, N, 1}};
        out = mask_install(ctx, a, who);
    }
    (void)hipStreamSynchronize(ctx->stream); /* (the host array and the copy may go once the call returns) */
    (void)hipFree(tmp);
    return out;
}

/* the device form: the descriptor is checked before anything happens; every byte value is valid, so there is no check on
 * the device; the one host synchronisation is field_to_host's, behind which the array has been read */
extern "C" int mg3d_ctx_set_mask_device(mg3d_ctx *ctx, const mg3d_array *mask, void *stream)
{
    static const char who[] = "mg3d_ctx_set_mask_device";
    if (!ctx)
        return fail(MG3D_ERR_ARG, "%s: NULL context", who);
    if (!mask)
        return field_clear(ctx, ctx->mask);
    CHK(mg3d_array_check(ctx, mask, false, who, true));
    CHK(mg3d_stream_join(ctx, (hipStream_t)stream, false, who));
    return mask_install(ctx, *mask, who);
}

extern "C" int mg3d_ctx_has_mask(const mg3d_ctx *ctx, int *on) { return field_has(ctx, &mg3d_ctx::mask, on, "mg3d_ctx_has_mask"); }

extern "C" int mg3d_ctx_get_mask(mg3d_ctx *ctx, int level, unsigned char *host)
{
    return field_get(ctx, &mg3d_ctx::mask, level, host, "mg3d_ctx_get_mask", "mask");
}

/* How the levels below the finest take the mask: operator state, for grid values depend on it -- no launch option.  The
 * argument is checked before anything changes.  Without a mask the rule is kept for the next one.  With one, a rule that
 * differs from the present one: a cycle that has run ahead is finished with the hierarchy it started with, levels L-2 .. 0
 * are taken again from the finest level's stored bytes, the fixed unknowns counted and level 0 read back (one host
 * synchronisation), the coarse factor rebuilt or dropped.  The same rule again changes nothing. */
extern "C" int mg3d_ctx_set_mask_coarsening(mg3d_ctx *ctx, int rule)
{
    static const char who[] = "mg3d_ctx_set_mask_coarsening";
    if (!ctx)
        return fail(MG3D_ERR_ARG, "%s: NULL context", who);
    if (rule != MG3D_MASK_INJECT && rule != MG3D_MASK_KEEP)
        return fail(MG3D_ERR_ARG, "%s: rule = %d (MG3D_MASK_INJECT or MG3D_MASK_KEEP)", who, rule);
    if (rule == ctx->mask_rule)
        return MG3D_OK;
    if (!ctx->mask.set()) {
        ctx->mask_rule = rule;
        return MG3D_OK;
    }
    CHK(mg3d_drop_carry(ctx));
    ctx->mask_rule = rule;
    mask_coarsen(ctx);
    const int rc = field_to_host(ctx, ctx->mask, who);
    if (rc != MG3D_OK)
        return field_abandon(ctx, ctx->mask, rc);
    return operator_changed(ctx);
}

extern "C" int mg3d_ctx_get_mask_coarsening(const mg3d_ctx *ctx, int *rule)
{
    if (!ctx || !rule)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_get_mask_coarsening: NULL argument");
    *rule = ctx->mask_rule;
    return MG3D_OK;
}

/* ------------------------------------------------------------------------------------------ the screening field */

/* Everything below the finest level's field, under the present boundary masks: its periodic duplicates from their sources,
 * each coarser level by the context's own restriction (k_restrict with the boundary word: full weighting at every coarse
 * unknown with the operator's wrapped or reflected taps, injection on Dirichlet faces, duplicates written), then the counts
 * and level 0's field for the coarse matrix (field_to_host: one host synchronisation).  A HIP error leaves the context
 * without a field.  (The context has a field and io_chk.) */
static int sfield_rebuild(mg3d_ctx *ctx, const char *who)
{
    const int L = ctx->L, bc = mg3d_ctx_bc(ctx);
    k_per_refresh(ctx->lv[L - 1].g, ctx->sfield.lv[L - 1], bc, ctx->stream);
    for (int l = L - 1; l >= 1; l--)
        k_restrict(ctx->lv[l].g, ctx->sfield.lv[l], ctx->lv[l - 1].g, ctx->sfield.lv[l - 1], bc, ctx->stream);
    const int rc = field_to_host(ctx, ctx->sfield, who);
    return rc == MG3D_OK ? MG3D_OK : field_abandon(ctx, ctx->sfield, rc);
}

/* what both forms of mg3d_ctx_set_shift_field do before the finest level's field is written -- everything that can fail for
 * want of memory, nothing has changed when it does */
static int sfield_prepare(mg3d_ctx *ctx, const char *who)
{
    CHK(ensure_io_chk(ctx, who));
    CHK(ensure_per_b(ctx, who)); /* (a positive entry may lift the pin of a context whose boundaries are set later) */
    if (!ctx->eps.set())
        CHK(ensure_ones(ctx, who));
    return field_alloc(ctx, ctx->sfield, who);
}

/* The operator div(eps grad u) - (sigma + s) u = d on every level (mg3d_kernels.hip): one double >= 0 per point, s of the
 * finest level as given, of each coarser one by restriction.  The contract of mg3d_ctx_set_coefficient: the array is checked
 * before anything changes (periodic duplicates are skipped); then a cycle that has run ahead is finished with the operator
 * it started with and the coarse factor is rebuilt or dropped.  NULL: back to the context as it was, its fused schedules
 * included. */
extern "C" int mg3d_ctx_set_shift_field(mg3d_ctx *ctx, const double *s)
{
    static const char who[] = "mg3d_ctx_set_shift_field";
    if (!ctx)
        return fail(MG3D_ERR_ARG, "%s: NULL context", who);
    if (!s) {
        ctx->sfield_nl = false; /* (whatever the context keeps is not mg3d_nl_solve's any more) */
        return field_clear(ctx, ctx->sfield);
    }
    CHK(check_host<true>(ctx, s, "s", who));
    CHK(mg3d_drop_carry(ctx));
    CHK(sfield_prepare(ctx, who));
    ctx->sfield_nl = false; /* the caller's field from here on */
    CHK(top_from_host(ctx, ctx->sfield, s));
    CHK(sfield_rebuild(ctx, who)); /* (the host array may go once the call returns) */
    return operator_changed(ctx);
}

/* the device form, step for step that of mg3d_ctx_set_coefficient_device: the check, then the carried cycle, the pack into
 * the finest level's field, the duplicates, the restrictions and the counts (sfield_rebuild).  Two host synchronisations;
 * behind the second one the array has been read, so the caller's stream needs no event of ours. */
extern "C" int mg3d_ctx_set_shift_field_device(mg3d_ctx *ctx, const mg3d_array *s, void *stream)
{
    static const char who[] = "mg3d_ctx_set_shift_field_device";
    if (!ctx)
        return fail(MG3D_ERR_ARG, "%s: NULL context", who);
    if (!s)
        return mg3d_ctx_set_shift_field(ctx, nullptr);
    CHK(mg3d_array_check(ctx, s, false, who));
    CHK(ensure_io_chk(ctx, who));
    CHK(mg3d_stream_join(ctx, (hipStream_t)stream, false, who));
    CHK(check_device(ctx, *s, true, "s", who));
    CHK(mg3d_drop_carry(ctx));
    CHK(sfield_prepare(ctx, who));
    ctx->sfield_nl = false; /* the caller's field from here on */
    top_from_device(ctx, ctx->sfield, *s);
    CHK(sfield_rebuild(ctx, who));
    return operator_changed(ctx);
}

/* the install path for mg3d_nl.hip (mg3d_ctx.h) */
int mg3d_sfield_prepare(mg3d_ctx *ctx, const char *who) { return sfield_prepare(ctx, who); }
int mg3d_sfield_rebuild(mg3d_ctx *ctx, const char *who) { return sfield_rebuild(ctx, who); }
int mg3d_operator_changed(mg3d_ctx *ctx) { return operator_changed(ctx); }
int mg3d_check_weight_host(const mg3d_ctx *ctx, const double *a, const char *name, const char *who)
{
    return check_host<true>(ctx, a, name, who);
}
int mg3d_check_weight_device(mg3d_ctx *ctx, const mg3d_array &a, const char *name, const char *who)
{
    CHK(ensure_io_chk(ctx, who));
    return check_device(ctx, a, true, name, who);
}

extern "C" int mg3d_ctx_has_shift_field(const mg3d_ctx *ctx, int *on)
{
    return field_has(ctx, &mg3d_ctx::sfield, on, "mg3d_ctx_has_shift_field");
}

extern "C" int mg3d_ctx_get_shift_field(mg3d_ctx *ctx, int level, double *host)
{
    return field_get(ctx, &mg3d_ctx::sfield, level, host, "mg3d_ctx_get_shift_field", "field");
}

/* ------------------------------------------------------------------------------------------ the boundary masks */

/* the boundary masks changed.  Under a screening field: the finest level's duplicates of a periodic axis take their
 * sources' values, and the coarser levels and the counts are taken again, for the restriction is the boundary word's.  Under
 * a mask: the duplicates take their sources' bytes -- for good: the caller's bytes there are not kept, an axis that stops
 * being periodic finds its plane N-1 with plane 0's bytes -- and which fixed points are unknowns is counted again; under
 * MG3D_MASK_KEEP the lower levels are coarsened again from the finest one (re-injection alone would not do: which lost point a
 * coarse point stands for depends on the duplicates' bytes).  Then the coarse factor, as for every change of the operator */
static int boundaries_changed(mg3d_ctx *ctx, const char *who)
{
    if (ctx->sfield.set())
        CHK(sfield_rebuild(ctx, who));
    if (!ctx->mask.set())
        return operator_changed(ctx);
    if (ctx->mask_rule == MG3D_MASK_KEEP) {
        k_mask_refresh(ctx->lv[ctx->L - 1].g, ctx->mask.lv[ctx->L - 1], mg3d_ctx_bc(ctx), ctx->stream);
        mask_coarsen(ctx);
    } else {
        for (int l = 0; l < ctx->L; l++)
            k_mask_refresh(ctx->lv[l].g, ctx->mask.lv[l], mg3d_ctx_bc(ctx), ctx->stream);
    }
    const int rc = field_to_host(ctx, ctx->mask, who);
    if (rc != MG3D_OK)
        return field_abandon(ctx, ctx->mask, rc);
    return operator_changed(ctx);
}

/* The tail of mg3d_ctx_set_periodic and mg3d_ctx_set_neumann: the boundary masks become (per, neu).  The coarse faces that
 * the restriction weighted are injections again (and vice versa), so every level's are redone; and on a face that was a
 * face of unknowns and is a Dirichlet face now, r of every level still holds the residuals of the other operator where a
 * Dirichlet cycle never writes and the injection reads -- zeroed, as in a context that never had the mask.  Then the
 * fields and the coarse factor (boundaries_changed). */
static int set_boundaries(mg3d_ctx *ctx, int per, int neu, const char *who)
{
    if (per || neu)
        CHK(ensure_per_b(ctx, who));
    const int per0 = ctx->periodic, neu0 = ctx->neumann;
    ctx->periodic = per;
    ctx->neumann = neu;
    auto unknown_faces = [](int periodic, int neumann) {
        int m = neumann;
        for (int ax = 0; ax < 3; ax++)
            if (periodic >> ax & 1)
                m |= 3 << (2 * ax);
        return m;
    };
    const int back = unknown_faces(per0, neu0) & ~unknown_faces(ctx->periodic, ctx->neumann);
    for (int l = 0; l < ctx->L; l++)
        k_zero_faces(ctx->lv[l].g, ctx->lv[l].f[MG3D_R], back, ctx->stream);
    std::fill(ctx->faces_dirty.begin(), ctx->faces_dirty.end(), 1);
    return boundaries_changed(ctx, who);
}

/* Periodic axes (mg3d_kernels.hip): a mask of MG3D_PERIODIC_I / _J / _K.  The argument is checked before anything
 * changes -- a mask outside 0..7, or a nonzero one on a hierarchy whose coarsest level has fewer than 4 or an odd number
 * of unique points per side, is MG3D_ERR_ARG.  Then, as for a new sigma, a cycle that has run ahead is finished with the
 * operator it started with and the coarse factor is rebuilt (mg3d_ctx_build_coarse) or dropped.  0: Dirichlet faces
 * everywhere again, the fused schedules included. */
extern "C" int mg3d_ctx_set_periodic(mg3d_ctx *ctx, int axes)
{
    if (!ctx)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_set_periodic: NULL context");
    if (axes < 0 || axes > 7)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_set_periodic: axes = %d (a mask of MG3D_PERIODIC_I | _J | _K, 0..7)", axes);
    const int N0 = ctx->lv[0].g.N;
    if (axes && ((N0 - 1) % 2 != 0 || N0 - 1 < 4))
        return fail(MG3D_ERR_ARG, "mg3d_ctx_set_periodic: the coarsest level has %d points per side (c - 1 must be even and >= 4)",
                    N0);
    for (int ax = 0; ax < 3; ax++)
        if ((axes >> ax & 1) && (ctx->neumann >> (2 * ax) & 3))
            return fail(MG3D_ERR_ARG, "mg3d_ctx_set_periodic: axis %d has a Neumann face (mg3d_ctx_set_neumann: mask %d)", ax,
                        ctx->neumann);
    CHK(mg3d_drop_carry(ctx));
    if (axes == ctx->periodic)
        return MG3D_OK;
    return set_boundaries(ctx, axes, ctx->neumann, "mg3d_ctx_set_periodic");
}

extern "C" int mg3d_ctx_get_periodic(const mg3d_ctx *ctx, int *axes)
{
    if (!ctx || !axes)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_get_periodic: NULL argument");
    *axes = ctx->periodic;
    return MG3D_OK;
}

/* Neumann faces (mg3d_kernels.hip): a mask of MG3D_NEUMANN_ILO ... _KHI.  The argument is checked before anything changes
 * -- a mask outside 0..63, or one with a bit on a periodic axis, is MG3D_ERR_ARG.  Then, as for a new sigma, a cycle that
 * has run ahead is finished with the operator it started with and the coarse factor is rebuilt (mg3d_ctx_build_coarse) or
 * dropped.  0: no Neumann face again, the fused schedules included (when no axis is periodic). */
extern "C" int mg3d_ctx_set_neumann(mg3d_ctx *ctx, int faces)
{
    if (!ctx)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_set_neumann: NULL context");
    if (faces < 0 || faces > 63)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_set_neumann: faces = %d (a mask of MG3D_NEUMANN_ILO ... _KHI, 0..63)", faces);
    for (int ax = 0; ax < 3; ax++)
        if ((ctx->periodic >> ax & 1) && (faces >> (2 * ax) & 3))
            return fail(MG3D_ERR_ARG, "mg3d_ctx_set_neumann: faces = %d has a bit on periodic axis %d (mg3d_ctx_set_periodic: mask %d)",
                        faces, ax, ctx->periodic);
    CHK(mg3d_drop_carry(ctx));
    if (faces == ctx->neumann)
        return MG3D_OK;
    return set_boundaries(ctx, ctx->periodic, faces, "mg3d_ctx_set_neumann");
}

extern "C" int mg3d_ctx_get_neumann(const mg3d_ctx *ctx, int *faces)
{
    if (!ctx || !faces)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_get_neumann: NULL argument");
    *faces = ctx->neumann;
    return MG3D_OK;
}
