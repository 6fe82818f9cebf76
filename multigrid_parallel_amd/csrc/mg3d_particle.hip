/*
 * mg3d_particle.hip -- particle coupling on the device (mg3d_field_sample(_device), mg3d_deposit(_device), include/mg3d.h
 * "Particles"): the potential and its gradient gathered at points, point charges scattered into d of the finest level,
 * both with the context's own boundary logic.  The kernels are in mg3d_kernels.hip ("particles").
 *
 *   sample  : reads the context only, as the field output does (mg3d_drop_carry_keep: red_tail stays, the next cycle
 *             continues as if nothing had been asked).  One launch for all wanted outputs, counted under MG3D_K_PACK.
 *   deposit : writes d of the finest level, so its state handling is mg3d_upload_device's: mg3d_drop_carry first, then
 *             mg3d_ctx_touched(MG3D_D, finest, MG3D_WROTE_CALLER) -- the zero map is rescanned by the next cycle.  The sum
 *             runs in 64-bit integers (scan, accumulate, apply: three launches under MG3D_K_PACK, the duplicate refresh of
 *             a periodic context a fourth): integer adds commute, so the bits depend neither on the run nor on the order
 *             of the points.  The unit of the integers is chosen on the device; the host never waits for it.
 *   push    : mg3d_particle_push(_device), mg3d_particle_counts: one kick-and-drift step of the particles whose fate is 0
 *             with the context's walls and conductors.  Reads the context only, as the sample; one launch under
 *             MG3D_K_PACK; the fates are counted in a table of 64-bit integers on the device (integer adds again).
 *   reorder : mg3d_particle_sort(_device), mg3d_particle_permute_device: the stable permutation that puts the particles in
 *             cell order (the lost behind the living, the dead last) by a radix sort of (key, old index), 1 + 3 launches a
 *             pass under MG3D_K_PACK, and the gather of up to 16 attribute vectors in one launch.  Reads the geometry and
 *             no field: a cycle that has run ahead is left as it is.  The scratch belongs to the context and grows with
 *             the count.
 * The device forms do not synchronise with the host.  The host forms stage through buffers allocated for the call, run
 * the same launches and synchronise once.
 */
#include "mg3d_ctx.h"

#include <math.h>
#include <string.h>

#define fail mg3d_fail

#define PART_MAX_COUNT (1LL << 40)

static int part_launch_ok(const char *who)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(MG3D_ERR_HIP, "%s: kernel launch failed: %s", who, hipGetErrorString(e));
    return MG3D_OK;
}

/* a caller's vector, checked as an array is (mg3d_array_check: the pointer, the dtype, the stride) */
static int vec_check(const mg3d_ctx *ctx, const mg3d_vec *v, long long count, bool writable, const char *who)
{
    if (!v)
        return fail(MG3D_ERR_ARG, "%s: NULL vector", who);
    /* a vector of no elements has no pointer to look at (an empty tensor's is NULL): the context's own scratch word stands
     * in, dtype and stride are checked as ever */
    void *const ptr = count == 0 ? (void *)ctx->sumsq : v->ptr;
    const mg3d_array a = {ptr, v->dtype, {v->stride, v->stride, v->stride}};
    return mg3d_array_check(ctx, &a, writable, who);
}

/* what both calls ask of their arguments before anything happens; pos is checked only by the device forms */
static int part_args(const mg3d_ctx *ctx, long long count, double scale, const char *who)
{
    if (!ctx)
        return fail(MG3D_ERR_ARG, "%s: NULL context", who);
    if (count < 0 || count > PART_MAX_COUNT)
        return fail(MG3D_ERR_ARG, "%s: count = %lld (0 .. 2^40)", who, count);
    if (!isfinite(scale))
        return fail(MG3D_ERR_ARG, "%s: scale must be finite (%g)", who, scale);
    return mg3d_field_level(ctx, who);
}

static int pos_check(const mg3d_ctx *ctx, long long count, const mg3d_vec *const pos[3], const char *who)
{
    if (!pos)
        return fail(MG3D_ERR_ARG, "%s: NULL positions", who);
    for (int a = 0; a < 3; a++) {
        const int rc = vec_check(ctx, pos[a], count, false, who);
        if (rc != MG3D_OK)
            return rc;
    }
    return MG3D_OK;
}

/* ---------------------------------------------------------------------------------------------------------- sample */
static bool sample_wanted(const mg3d_vec *u_out, const mg3d_vec *const grad_out[3])
{
    return u_out || (grad_out && (grad_out[0] || grad_out[1] || grad_out[2]));
}

/* the sample launch on the context's stream, behind a cycle that has run ahead */
static int sample_enqueue(mg3d_ctx *ctx, long long count, const mg3d_vec *const pos[3], double scale, const mg3d_vec *u_out,
                          const mg3d_vec *const grad_out[3], const char *who)
{
    int rc = mg3d_drop_carry_keep(ctx); /* (reads only, as mg3d_download_device) */
    if (rc != MG3D_OK)
        return rc;
    const int q = ctx->L - 1;
    const Level &top = ctx->lv[q];
    const double cs = scale * (0.5 / top.h);
    {
        StageScope kt(ctx, q, MG3D_K_PACK, true);
        if (k_part_sample(top.g, top.f[MG3D_U], mg3d_ctx_bc(ctx), top.h, cs, count, pos, u_out, grad_out, ctx->stream) < 0)
            return fail(MG3D_ERR_STATE, "%s: the level has no launch shape", who);
    }
    return part_launch_ok(who);
}

extern "C" int mg3d_field_sample_device(mg3d_ctx *ctx, long long count, const mg3d_vec *const pos[3], double scale,
                                        const mg3d_vec *u_out, const mg3d_vec *const grad_out[3], void *stream)
{
    static const char who[] = "mg3d_field_sample_device";
    int rc = part_args(ctx, count, scale, who);
    if (rc == MG3D_OK && !sample_wanted(u_out, grad_out))
        rc = fail(MG3D_ERR_ARG, "%s: no output wanted (u and all three components NULL)", who);
    if (rc == MG3D_OK)
        rc = pos_check(ctx, count, pos, who);
    if (rc == MG3D_OK && u_out)
        rc = vec_check(ctx, u_out, count, true, who);
    for (int a = 0; a < 3 && rc == MG3D_OK && grad_out; a++)
        if (grad_out[a])
            rc = vec_check(ctx, grad_out[a], count, true, who);
    if (rc != MG3D_OK || count == 0)
        return rc;
    rc = mg3d_stream_join(ctx, (hipStream_t)stream, false, who); /* (what the caller's stream still does with the outputs) */
    if (rc == MG3D_OK)
        rc = sample_enqueue(ctx, count, pos, scale, u_out, grad_out, who);
    if (rc != MG3D_OK)
        return rc;
    return mg3d_stream_join(ctx, (hipStream_t)stream, true, who);
}

/* ---------------------------------------------------------------------------------------------------------- deposit */
/* the accumulator and the word of max |q|, on first use */
static int deposit_alloc(mg3d_ctx *ctx, const char *who)
{
    if (!ctx->dep_max) {
        const int rc = mg3d_device_alloc((void **)&ctx->dep_max, sizeof(unsigned long long), who);
        if (rc != MG3D_OK)
            return rc;
    }
    if (!ctx->dep_acc)
        return mg3d_device_alloc((void **)&ctx->dep_acc, ctx->lv[ctx->L - 1].elems * sizeof(long long), who);
    return MG3D_OK;
}

/* the deposit's launches on the context's stream and its state handling, mg3d_upload_device's on d of the finest level */
static int deposit_enqueue(mg3d_ctx *ctx, long long count, const mg3d_vec *const pos[3], const mg3d_vec *qv, double scale,
                           const char *who)
{
    const int q = ctx->L - 1;
    const Level &top = ctx->lv[q];
    const int bc = mg3d_ctx_bc(ctx);
    if (count > 0) {
        int K = 0;
        while ((1LL << K) < count)
            K++;
        const double inv_h3 = 1.0 / ((top.h * top.h) * top.h);
        const double f0 = scale * inv_h3;
        hipError_t e = hipMemsetAsync(ctx->dep_max, 0, sizeof(unsigned long long), ctx->stream);
        if (e == hipSuccess)
            e = hipMemsetAsync(ctx->dep_acc, 0, top.elems * sizeof(long long), ctx->stream);
        if (e != hipSuccess)
            return fail(MG3D_ERR_HIP, "%s: clearing the accumulator: %s", who, hipGetErrorString(e));
        int launched;
        {
            StageScope kt(ctx, q, MG3D_K_PACK, true);
            launched = k_part_scan(top.g, bc, top.h, count, pos, qv, ctx->dep_max, ctx->stream);
        }
        if (launched == 0) {
            StageScope kt(ctx, q, MG3D_K_PACK, true);
            launched = k_part_accumulate(top.g, bc, top.h, count, K, pos, qv, ctx->dep_max, ctx->dep_acc, ctx->stream);
        }
        if (launched == 0) {
            StageScope kt(ctx, q, MG3D_K_PACK, true);
            launched = k_part_apply(top.g, bc, f0, K, ctx->dep_max, ctx->dep_acc, top.f[MG3D_D], ctx->stream);
        }
        if (launched < 0)
            return fail(MG3D_ERR_STATE, "%s: the level has no launch shape", who);
        if (bc & 7) {
            StageScope kt(ctx, q, MG3D_K_PACK, true);
            k_per_refresh(top.g, top.f[MG3D_D], bc, ctx->stream, ctx->dep_max); /* (apply writes unique points only) */
        }
    }
    mg3d_ctx_touched(ctx, MG3D_D, q, false, MG3D_WROTE_CALLER);
    return part_launch_ok(who);
}

extern "C" int mg3d_deposit_device(mg3d_ctx *ctx, long long count, const mg3d_vec *const pos[3], const mg3d_vec *qv,
                                   double scale, void *stream)
{
    static const char who[] = "mg3d_deposit_device";
    int rc = part_args(ctx, count, scale, who);
    if (rc == MG3D_OK)
        rc = pos_check(ctx, count, pos, who);
    if (rc == MG3D_OK)
        rc = vec_check(ctx, qv, count, false, who);
    if (rc == MG3D_OK)
        rc = deposit_alloc(ctx, who);
    if (rc == MG3D_OK)
        rc = mg3d_drop_carry(ctx);
    if (rc == MG3D_OK)
        rc = mg3d_stream_join(ctx, (hipStream_t)stream, false, who);
    if (rc == MG3D_OK)
        rc = deposit_enqueue(ctx, count, pos, qv, scale, who);
    if (rc != MG3D_OK)
        return rc;
    return mg3d_stream_join(ctx, (hipStream_t)stream, true, who);
}

/* ------------------------------------------------------------------------------------------------------------- push */
/* the parameters of a push: a positive finite step, finite scale and acceleration, a finite drag >= 0 */
static int push_params_check(const mg3d_push_params *p, const char *who)
{
    if (!p)
        return fail(MG3D_ERR_ARG, "%s: NULL parameters", who);
    if (!isfinite(p->dt) || !(p->dt > 0.0))
        return fail(MG3D_ERR_ARG, "%s: dt must be finite and > 0 (%g)", who, p->dt);
    if (!isfinite(p->scale))
        return fail(MG3D_ERR_ARG, "%s: scale must be finite (%g)", who, p->scale);
    for (int a = 0; a < 3; a++)
        if (!isfinite(p->accel[a]))
            return fail(MG3D_ERR_ARG, "%s: accel[%d] must be finite (%g)", who, a, p->accel[a]);
    if (!isfinite(p->drag) || p->drag < 0.0)
        return fail(MG3D_ERR_ARG, "%s: drag must be finite and >= 0 (%g)", who, p->drag);
    return MG3D_OK;
}

/* the fate vector: MG3D_I32 and nothing else, written, so a stride >= 1; its four-byte elements let the pointer and the
 * stride be checked as a float vector's */
static int fate_check(const mg3d_ctx *ctx, const mg3d_vec *fate, long long count, const char *who)
{
    if (!fate)
        return fail(MG3D_ERR_ARG, "%s: NULL fate vector", who);
    if (fate->dtype != MG3D_I32)
        return fail(MG3D_ERR_ARG, "%s: the fate vector has dtype %d (MG3D_I32)", who, fate->dtype);
    const mg3d_vec as_f32 = {fate->ptr, MG3D_F32, fate->stride};
    return vec_check(ctx, &as_f32, count, true, who);
}

/* the table of counters, allocated and zeroed on the context's stream with the first push */
static int push_alloc(mg3d_ctx *ctx, const char *who)
{
    if (ctx->push_table)
        return MG3D_OK;
    const size_t bytes = MG3D_FATE_SLOTS * sizeof(unsigned long long);
    const int rc = mg3d_device_alloc((void **)&ctx->push_table, bytes, who);
    if (rc != MG3D_OK)
        return rc;
    const hipError_t e = hipMemsetAsync(ctx->push_table, 0, bytes, ctx->stream);
    if (e != hipSuccess) {
        (void)hipFree(ctx->push_table);
        ctx->push_table = nullptr;
        return fail(MG3D_ERR_HIP, "%s: clearing the table of fates: %s", who, hipGetErrorString(e));
    }
    return MG3D_OK;
}

/* the push launch on the context's stream, behind a cycle that has run ahead */
static int push_enqueue(mg3d_ctx *ctx, long long count, const mg3d_vec *const pos[3], const mg3d_vec *const vel[3],
                        const mg3d_vec *qm, const mg3d_vec *fate, const mg3d_push_params *p, const char *who)
{
    int rc = mg3d_drop_carry_keep(ctx); /* (reads only, as the sample) */
    if (rc != MG3D_OK)
        return rc;
    const int q = ctx->L - 1;
    const Level &top = ctx->lv[q];
    {
        StageScope kt(ctx, q, MG3D_K_PACK, true);
        if (k_part_push(top.g, top.f[MG3D_U], ctx->mask.at(q), mg3d_ctx_bc(ctx), top.h, count, pos, vel, qm, fate, *p,
                        ctx->push_table, ctx->stream) < 0)
            return fail(MG3D_ERR_STATE, "%s: the level has no launch shape", who);
    }
    return part_launch_ok(who);
}

extern "C" int mg3d_particle_push_device(mg3d_ctx *ctx, long long count, const mg3d_vec *const pos[3],
                                         const mg3d_vec *const vel[3], const mg3d_vec *qm, const mg3d_vec *fate,
                                         const mg3d_push_params *p, void *stream)
{
    static const char who[] = "mg3d_particle_push_device";
    int rc = push_params_check(p, who);
    if (rc == MG3D_OK)
        rc = part_args(ctx, count, p->scale, who);
    if (rc == MG3D_OK && (!pos || !vel))
        rc = fail(MG3D_ERR_ARG, "%s: NULL %s", who, pos ? "velocities" : "positions");
    for (int a = 0; a < 3 && rc == MG3D_OK; a++) {
        if (pos[a] && pos[a]->dtype != MG3D_F64)
            rc = fail(MG3D_ERR_ARG, "%s: pos[%d] has dtype %d (positions are updated in MG3D_F64 only)", who, a, pos[a]->dtype);
        if (rc == MG3D_OK)
            rc = vec_check(ctx, pos[a], count, true, who);
        if (rc == MG3D_OK)
            rc = vec_check(ctx, vel[a], count, true, who);
    }
    if (rc == MG3D_OK)
        rc = vec_check(ctx, qm, count, false, who);
    if (rc == MG3D_OK)
        rc = fate_check(ctx, fate, count, who);
    if (rc != MG3D_OK || count == 0)
        return rc;
    rc = push_alloc(ctx, who);
    if (rc == MG3D_OK)
        rc = mg3d_stream_join(ctx, (hipStream_t)stream, false, who);
    if (rc == MG3D_OK)
        rc = push_enqueue(ctx, count, pos, vel, qm, fate, p, who);
    if (rc != MG3D_OK)
        return rc;
    return mg3d_stream_join(ctx, (hipStream_t)stream, true, who);
}

extern "C" int mg3d_particle_counts(mg3d_ctx *ctx, unsigned long long out[MG3D_FATE_SLOTS], int reset)
{
    static const char who[] = "mg3d_particle_counts";
    if (!ctx || !out)
        return fail(MG3D_ERR_ARG, "%s: NULL %s", who, ctx ? "output" : "context");
    const size_t bytes = MG3D_FATE_SLOTS * sizeof(unsigned long long);
    if (!ctx->push_table) { /* no push yet */
        memset(out, 0, bytes);
        return MG3D_OK;
    }
    hipError_t e = hipMemcpyAsync(out, ctx->push_table, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && reset)
        e = hipMemsetAsync(ctx->push_table, 0, bytes, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess || es != hipSuccess)
        return fail(MG3D_ERR_HIP, "%s: %s", who, hipGetErrorString(e != hipSuccess ? e : es));
    return MG3D_OK;
}

/* ---------------------------------------------------------------------------------------------------------- reorder */
#define SORT_MAX_COUNT 2147483647LL
#define SORT_MAX_SHIFT 8

/* a vector of MG3D_I32 (the sort's fate and perm, the permute's perm); four-byte elements, checked as the push's fate is */
static int i32_check(const mg3d_ctx *ctx, const mg3d_vec *v, long long count, bool writable, const char *who, const char *what)
{
    if (!v)
        return fail(MG3D_ERR_ARG, "%s: NULL %s vector", who, what);
    if (v->dtype != MG3D_I32)
        return fail(MG3D_ERR_ARG, "%s: the %s vector has dtype %d (MG3D_I32)", who, what, v->dtype);
    const mg3d_vec as_f32 = {v->ptr, MG3D_F32, v->stride};
    return vec_check(ctx, &as_f32, count, writable, who);
}

/* the sort's own arguments; *passes = the 8-bit digits of KMAX + 1 */
static int sort_args(const mg3d_ctx *ctx, long long count, int shift, int *passes, const char *who)
{
    if (!ctx)
        return fail(MG3D_ERR_ARG, "%s: NULL context", who);
    if (count < 0 || count > SORT_MAX_COUNT)
        return fail(MG3D_ERR_ARG, "%s: count = %lld (0 .. 2^31 - 1)", who, count);
    if (shift < 0 || shift > SORT_MAX_SHIFT)
        return fail(MG3D_ERR_ARG, "%s: shift = %d (0 .. %d)", who, shift, SORT_MAX_SHIFT);
    const int rc = mg3d_field_level(ctx, who);
    if (rc != MG3D_OK)
        return rc;
    const unsigned long long nb = (unsigned long long)((ctx->lv[ctx->L - 1].g.N - 2) >> shift) + 1ULL;
    const unsigned long long top = nb * nb * nb + 1ULL; /* the largest key */
    if (top > 0xFFFFFFFFULL)
        return fail(MG3D_ERR_ARG, "%s: %llu^3 + 2 keys do not fit 32 bits: a larger shift is needed", who, nb);
    int bits = 0;
    while (top >> bits)
        bits++;
    *passes = (bits + 7) / 8;
    return MG3D_OK;
}

static long long sort_tiles(long long count) { return (count + MG3D_SORT_TILE - 1) / MG3D_SORT_TILE; }
static size_t sort_bytes(long long count) { return 4 * (4 * (size_t)count + 256 * (size_t)(sort_tiles(count) + 1)); }

/* the scratch for `count` particles; a larger one replaces a smaller one only once it exists */
static int sort_alloc(mg3d_ctx *ctx, long long count, const char *who)
{
    if (count <= ctx->sort_cap)
        return MG3D_OK;
    unsigned *buf = nullptr;
    const int rc = mg3d_device_alloc((void **)&buf, sort_bytes(count), who);
    if (rc != MG3D_OK)
        return rc;
    if (ctx->sort_buf)
        (void)hipFree(ctx->sort_buf);
    ctx->sort_buf = buf;
    ctx->sort_cap = count;
    return MG3D_OK;
}

/* the sort's launches on the context's stream: 1 + 3 * passes of them.  Reads the geometry and no field: a cycle that has
 * run ahead stays as it is. */
static int sort_enqueue(mg3d_ctx *ctx, long long count, const mg3d_vec *const pos[3], const mg3d_vec *fate, int shift,
                        int passes, const mg3d_vec *perm, long long *counts_dev, const char *who)
{
    const int q = ctx->L - 1;
    const Level &top = ctx->lv[q];
    const size_t cap = (size_t)ctx->sort_cap;
    unsigned *kin = ctx->sort_buf, *kout = ctx->sort_buf + cap;
    int *iin = (int *)(ctx->sort_buf + 2 * cap), *iout = (int *)(ctx->sort_buf + 3 * cap);
    unsigned *const tot = ctx->sort_buf + 4 * cap, *const table = tot + 256;
    if (counts_dev) {
        const hipError_t e = hipMemsetAsync(counts_dev, 0, 2 * sizeof(long long), ctx->stream);
        if (e != hipSuccess)
            return fail(MG3D_ERR_HIP, "%s: clearing the counts: %s", who, hipGetErrorString(e));
    }
    {
        StageScope kt(ctx, q, MG3D_K_PACK, true);
        if (k_sort_keys(top.g, mg3d_ctx_bc(ctx), top.h, count, pos, fate, shift, kin, (unsigned long long *)counts_dev,
                        ctx->stream) < 0)
            return fail(MG3D_ERR_STATE, "%s: the level has no launch shape", who);
    }
    for (int p = 0; p < passes; p++) {
        const bool last = p == passes - 1;
        {
            StageScope kt(ctx, q, MG3D_K_PACK, true);
            k_sort_hist(kin, count, 8 * p, table, ctx->stream);
        }
        {
            StageScope kt(ctx, q, MG3D_K_PACK, true);
            k_sort_rowscan(count, table, tot, ctx->stream);
        }
        {
            StageScope kt(ctx, q, MG3D_K_PACK, true);
            k_sort_scatter(kin, p == 0 ? nullptr : iin, last ? nullptr : kout, last ? (int *)perm->ptr : iout,
                           last ? perm->stride : 1, count, 8 * p, table, tot, ctx->stream);
        }
        unsigned *const tk = kin;
        kin = kout;
        kout = tk;
        int *const ti = iin;
        iin = iout;
        iout = ti;
    }
    return part_launch_ok(who);
}

extern "C" int mg3d_particle_sort_device(mg3d_ctx *ctx, long long count, const mg3d_vec *const pos[3], const mg3d_vec *fate,
                                         int shift, const mg3d_vec *perm, long long *counts_dev, void *stream)
{
    static const char who[] = "mg3d_particle_sort_device";
    int passes = 0;
    int rc = sort_args(ctx, count, shift, &passes, who);
    if (rc == MG3D_OK)
        rc = pos_check(ctx, count, pos, who);
    if (rc == MG3D_OK && fate)
        rc = i32_check(ctx, fate, count, false, who, "fate");
    if (rc == MG3D_OK)
        rc = i32_check(ctx, perm, count, true, who, "perm");
    if (rc == MG3D_OK && counts_dev) {
        const mg3d_vec c = {counts_dev, MG3D_F64, 1};
        rc = vec_check(ctx, &c, 2, true, who);
    }
    if (rc != MG3D_OK || count == 0)
        return rc;
    rc = sort_alloc(ctx, count, who);
    if (rc == MG3D_OK)
        rc = mg3d_stream_join(ctx, (hipStream_t)stream, false, who);
    if (rc == MG3D_OK)
        rc = sort_enqueue(ctx, count, pos, fate, shift, passes, perm, counts_dev, who);
    if (rc != MG3D_OK)
        return rc;
    return mg3d_stream_join(ctx, (hipStream_t)stream, true, who);
}

extern "C" int mg3d_particle_permute_device(mg3d_ctx *ctx, long long count, const mg3d_vec *perm, int nvec,
                                            const mg3d_vec *const *src, const mg3d_vec *const *dst, void *stream)
{
    static const char who[] = "mg3d_particle_permute_device";
    if (!ctx)
        return fail(MG3D_ERR_ARG, "%s: NULL context", who);
    if (count < 0 || count > SORT_MAX_COUNT)
        return fail(MG3D_ERR_ARG, "%s: count = %lld (0 .. 2^31 - 1)", who, count);
    if (nvec < 1 || nvec > MG3D_PERMUTE_MAX_VECS)
        return fail(MG3D_ERR_ARG, "%s: nvec = %d (1 .. %d)", who, nvec, MG3D_PERMUTE_MAX_VECS);
    if (!src || !dst)
        return fail(MG3D_ERR_ARG, "%s: NULL %s", who, src ? "destinations" : "sources");
    int rc = i32_check(ctx, perm, count, false, who, "perm");
    for (int v = 0; v < nvec && rc == MG3D_OK; v++) {
        if (!src[v] || !dst[v])
            return fail(MG3D_ERR_ARG, "%s: NULL vector (%s[%d])", who, src[v] ? "dst" : "src", v);
        if (src[v]->dtype != dst[v]->dtype)
            return fail(MG3D_ERR_ARG, "%s: src[%d] has dtype %d, dst[%d] has dtype %d", who, v, src[v]->dtype, v,
                        dst[v]->dtype);
        if (src[v]->dtype == MG3D_I32) {
            rc = i32_check(ctx, src[v], count, false, who, "source");
            if (rc == MG3D_OK)
                rc = i32_check(ctx, dst[v], count, true, who, "destination");
        } else {
            rc = vec_check(ctx, src[v], count, false, who);
            if (rc == MG3D_OK)
                rc = vec_check(ctx, dst[v], count, true, who);
        }
    }
    if (rc != MG3D_OK || count == 0)
        return rc;
    rc = mg3d_stream_join(ctx, (hipStream_t)stream, false, who);
    if (rc != MG3D_OK)
        return rc;
    {
        StageScope kt(ctx, ctx->L - 1, MG3D_K_PACK, true);
        if (k_part_permute(count, perm, nvec, src, dst, ctx->stream) < 0)
            return fail(MG3D_ERR_STATE, "%s: nothing to launch", who);
    }
    rc = part_launch_ok(who);
    if (rc != MG3D_OK)
        return rc;
    return mg3d_stream_join(ctx, (hipStream_t)stream, true, who);
}

/* ------------------------------------------------------------------------------------------------------ host forms */
/* `doubles` doubles of device memory for one call of a host form */
struct Staging {
    double *p = nullptr;
    ~Staging()
    {
        if (p)
            (void)hipFree(p);
    }
    int alloc(size_t doubles, const char *who)
    {
        const hipError_t e = hipMalloc(&p, doubles * sizeof(double));
        if (e == hipSuccess)
            return MG3D_OK;
        (void)hipGetLastError();
        p = nullptr;
        return mg3d_alloc_fail(e, who, "the staging buffer");
    }
};

extern "C" int mg3d_field_sample(mg3d_ctx *ctx, long long count, const double *xyz, double scale, double *u, double *grad)
{
    static const char who[] = "mg3d_field_sample";
    int rc = part_args(ctx, count, scale, who);
    if (rc != MG3D_OK)
        return rc;
    if (!u && !grad)
        return fail(MG3D_ERR_ARG, "%s: no output wanted (u and grad NULL)", who);
    if (!xyz)
        return fail(MG3D_ERR_ARG, "%s: NULL positions", who);
    if (count == 0)
        return MG3D_OK;
    /* one buffer: the positions (3 per point), u (1), the gradient (3) */
    const size_t n = (size_t)count;
    Staging buf;
    rc = buf.alloc(7 * n, who);
    if (rc != MG3D_OK)
        return rc;
    double *const dx = buf.p, *const du = buf.p + 3 * n, *const dg = buf.p + 4 * n;
    const mg3d_vec px = {dx, MG3D_F64, 3}, py = {dx + 1, MG3D_F64, 3}, pz = {dx + 2, MG3D_F64, 3};
    const mg3d_vec vu = {du, MG3D_F64, 1}, g0 = {dg, MG3D_F64, 3}, g1 = {dg + 1, MG3D_F64, 3}, g2 = {dg + 2, MG3D_F64, 3};
    const mg3d_vec *const pos[3] = {&px, &py, &pz};
    const mg3d_vec *const gout[3] = {&g0, &g1, &g2};
    hipError_t e = hipMemcpyAsync(dx, xyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess)
        rc = fail(MG3D_ERR_HIP, "%s: copy to the device: %s", who, hipGetErrorString(e));
    if (rc == MG3D_OK)
        rc = sample_enqueue(ctx, count, pos, scale, u ? &vu : nullptr, grad ? gout : nullptr, who);
    if (rc == MG3D_OK && u)
        e = hipMemcpyAsync(u, du, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (rc == MG3D_OK && e == hipSuccess && grad)
        e = hipMemcpyAsync(grad, dg, 3 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream); /* (also before the buffer goes) */
    if (rc == MG3D_OK && (e != hipSuccess || es != hipSuccess))
        rc = fail(MG3D_ERR_HIP, "%s: copy to the host: %s", who, hipGetErrorString(e != hipSuccess ? e : es));
    return rc;
}

extern "C" int mg3d_deposit(mg3d_ctx *ctx, long long count, const double *xyz, const double *qh, double scale)
{
    static const char who[] = "mg3d_deposit";
    int rc = part_args(ctx, count, scale, who);
    if (rc != MG3D_OK)
        return rc;
    if (!xyz)
        return fail(MG3D_ERR_ARG, "%s: NULL positions", who);
    if (!qh)
        return fail(MG3D_ERR_ARG, "%s: NULL charges", who);
    const size_t n = (size_t)count;
    Staging buf;
    if (count > 0)
        rc = buf.alloc(4 * n, who);
    if (rc == MG3D_OK)
        rc = deposit_alloc(ctx, who);
    if (rc == MG3D_OK)
        rc = mg3d_drop_carry(ctx);
    if (rc != MG3D_OK)
        return rc;
    double *const dx = buf.p, *const dq = buf.p + 3 * n;
    const mg3d_vec px = {dx, MG3D_F64, 3}, py = {dx + 1, MG3D_F64, 3}, pz = {dx + 2, MG3D_F64, 3}, vq = {dq, MG3D_F64, 1};
    const mg3d_vec *const pos[3] = {&px, &py, &pz};
    if (count > 0) {
        hipError_t e = hipMemcpyAsync(dx, xyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(dq, qh, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess)
            rc = fail(MG3D_ERR_HIP, "%s: copy to the device: %s", who, hipGetErrorString(e));
    }
    if (rc == MG3D_OK)
        rc = deposit_enqueue(ctx, count, pos, &vq, scale, who);
    const hipError_t es = hipStreamSynchronize(ctx->stream); /* (before the buffer goes) */
    if (rc == MG3D_OK && es != hipSuccess)
        rc = fail(MG3D_ERR_HIP, "%s: %s", who, hipGetErrorString(es));
    return rc;
}

extern "C" int mg3d_particle_push(mg3d_ctx *ctx, long long count, double *xyz, double *vxyz, const double *qm, int *fate,
                                  const mg3d_push_params *p)
{
    static const char who[] = "mg3d_particle_push";
    int rc = push_params_check(p, who);
    if (rc == MG3D_OK)
        rc = part_args(ctx, count, p->scale, who);
    if (rc != MG3D_OK)
        return rc;
    if (!xyz || !vxyz || !qm || !fate)
        return fail(MG3D_ERR_ARG, "%s: NULL %s", who, !xyz ? "positions" : !vxyz ? "velocities" : !qm ? "q/m" : "fates");
    if (count == 0)
        return MG3D_OK;
    /* one buffer: the positions (3 per particle), the velocities (3), q/m (1), then the fates as ints */
    const size_t n = (size_t)count;
    Staging buf;
    rc = buf.alloc(7 * n + (n + 1) / 2, who);
    if (rc == MG3D_OK)
        rc = push_alloc(ctx, who);
    if (rc != MG3D_OK)
        return rc;
    double *const dx = buf.p, *const dv = buf.p + 3 * n, *const dq = buf.p + 6 * n;
    int *const df = (int *)(buf.p + 7 * n);
    const mg3d_vec px = {dx, MG3D_F64, 3}, py = {dx + 1, MG3D_F64, 3}, pz = {dx + 2, MG3D_F64, 3};
    const mg3d_vec vx = {dv, MG3D_F64, 3}, vy = {dv + 1, MG3D_F64, 3}, vz = {dv + 2, MG3D_F64, 3};
    const mg3d_vec vq = {dq, MG3D_F64, 1}, vf = {df, MG3D_I32, 1};
    const mg3d_vec *const pos[3] = {&px, &py, &pz};
    const mg3d_vec *const vel[3] = {&vx, &vy, &vz};
    hipError_t e = hipMemcpyAsync(dx, xyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(dv, vxyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(dq, qm, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(df, fate, n * sizeof(int), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess)
        rc = fail(MG3D_ERR_HIP, "%s: copy to the device: %s", who, hipGetErrorString(e));
    if (rc == MG3D_OK)
        rc = push_enqueue(ctx, count, pos, vel, &vq, &vf, p, who);
    if (rc == MG3D_OK)
        e = hipMemcpyAsync(xyz, dx, 3 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (rc == MG3D_OK && e == hipSuccess)
        e = hipMemcpyAsync(vxyz, dv, 3 * n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (rc == MG3D_OK && e == hipSuccess)
        e = hipMemcpyAsync(fate, df, n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream); /* (also before the buffer goes) */
    if (rc == MG3D_OK && (e != hipSuccess || es != hipSuccess))
        rc = fail(MG3D_ERR_HIP, "%s: copy to the host: %s", who, hipGetErrorString(e != hipSuccess ? e : es));
    return rc;
}

extern "C" int mg3d_particle_sort(mg3d_ctx *ctx, long long count, const double *xyz, const int *fate, int shift, int *perm,
                                  long long *counts)
{
    static const char who[] = "mg3d_particle_sort";
    int passes = 0;
    int rc = sort_args(ctx, count, shift, &passes, who);
    if (rc != MG3D_OK)
        return rc;
    if (!xyz || !perm)
        return fail(MG3D_ERR_ARG, "%s: NULL %s", who, xyz ? "permutation" : "positions");
    if (count == 0)
        return MG3D_OK;
    /* one buffer: the positions (3 per particle), the two counts, then the fates and the permutation as ints */
    const size_t n = (size_t)count;
    Staging buf;
    rc = buf.alloc(3 * n + 2 + n + 1, who);
    if (rc == MG3D_OK)
        rc = sort_alloc(ctx, count, who);
    if (rc != MG3D_OK)
        return rc;
    double *const dx = buf.p;
    long long *const dc = (long long *)(buf.p + 3 * n);
    int *const df = (int *)(buf.p + 3 * n + 2), *const dp = df + n;
    const mg3d_vec px = {dx, MG3D_F64, 3}, py = {dx + 1, MG3D_F64, 3}, pz = {dx + 2, MG3D_F64, 3};
    const mg3d_vec vf = {df, MG3D_I32, 1}, vp = {dp, MG3D_I32, 1};
    const mg3d_vec *const pos[3] = {&px, &py, &pz};
    hipError_t e = hipMemcpyAsync(dx, xyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && fate)
        e = hipMemcpyAsync(df, fate, n * sizeof(int), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess)
        rc = fail(MG3D_ERR_HIP, "%s: copy to the device: %s", who, hipGetErrorString(e));
    if (rc == MG3D_OK)
        rc = sort_enqueue(ctx, count, pos, fate ? &vf : nullptr, shift, passes, &vp, counts ? dc : nullptr, who);
    if (rc == MG3D_OK)
        e = hipMemcpyAsync(perm, dp, n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
    if (rc == MG3D_OK && e == hipSuccess && counts)
        e = hipMemcpyAsync(counts, dc, 2 * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream); /* (also before the buffer goes) */
    if (rc == MG3D_OK && (e != hipSuccess || es != hipSuccess))
        rc = fail(MG3D_ERR_HIP, "%s: copy to the host: %s", who, hipGetErrorString(e != hipSuccess ? e : es));
    return rc;
}
