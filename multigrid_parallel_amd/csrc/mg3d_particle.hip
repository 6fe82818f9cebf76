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
