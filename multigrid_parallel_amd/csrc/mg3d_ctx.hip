/*
 * mg3d_ctx.hip -- solver context and V-cycle sequencing behind the C ABI (include/mg3d.h).
 *
 * The context is the device-resident counterpart of the reference's global
 * state (mg_3d.h:19-28): three level hierarchies u, d, r plus the factored
 * coarsest operator.  Everything is enqueued on one HIP stream; the only host
 * synchronisations are the ones an entry point's contract requires (returning
 * a norm, copying data back).
 */
#include "mg3d_ctx.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

/* ------------------------------------------------------------------ errors */
static thread_local char g_err[512] = "";

int mg3d_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
#define fail mg3d_fail

int mg3d_alloc_fail(hipError_t e, const char *who, const char *what)
{
    const int code = e == hipErrorOutOfMemory ? MG3D_ERR_ALLOC : MG3D_ERR_HIP;
    return what ? fail(code, "%s: %s: %s", who, what, hipGetErrorString(e)) : fail(code, "%s failed: %s", who, hipGetErrorString(e));
}

int mg3d_device_alloc(void **p, size_t bytes, const char *who)
{
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess)
        return MG3D_OK;
    *p = nullptr;
    return mg3d_alloc_fail(e, who, "hipMalloc");
}

#define HIPCHK(call)                                                                                       \
    do {                                                                                                   \
        hipError_t e_ = (call);                                                                            \
        if (e_ != hipSuccess)                                                                              \
            return fail(MG3D_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__,    \
                        __LINE__);                                                                         \
    } while (0)

#define CHK(call)              \
    do {                       \
        int rc_ = (call);      \
        if (rc_ != MG3D_OK)    \
            return rc_;        \
    } while (0)

extern "C" const char *mg3d_last_error(void) { return g_err; }

static const char *const kStageNames[MG3D_NUM_STAGES] = {"Smoother1",          "CalcResidual1", "Restrict Residual",
                                                         "Recurse, Direct Solve", "Prolongate&Correct", "Smoother2",
                                                         "CalcResidual2"}; /* mg_3d.h:136-137 */

static const char *const kKernelNames[MG3D_NUM_KERNELS] = {"sweep4", "sweep2", "sweep2+residual", "residual",
                                                           "restrict", "prolong", "coarse_solve", "colour_pass",
                                                           "sweep4+norm", "sweep1+restrict", "leg_down", "leg_up",
                                                           "pcg_apply", "step_rhs", "pack"};

extern "C" const char *mg3d_kernel_name(int k) { return (k >= 0 && k < MG3D_NUM_KERNELS) ? kKernelNames[k] : "?"; }

extern "C" const char *mg3d_stage_name(int stage)
{
    return (stage >= 0 && stage < MG3D_NUM_STAGES) ? kStageNames[stage] : "?";
}

extern "C" int mg3d_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

static int require_device(void)
{
    if (mg3d_device_count() <= 0)
        return fail(MG3D_ERR_NO_DEVICE, "no HIP device available: libmg3d has no CPU fallback");
    return MG3D_OK;
}

/* ----------------------------------------------------------------- context */
static hipEvent_t take_event(mg3d_ctx *ctx)
{
    hipEvent_t e = nullptr;
    if (!ctx->event_pool.empty()) {
        e = ctx->event_pool.back();
        ctx->event_pool.pop_back();
    } else if (hipEventCreate(&e) != hipSuccess) {
        e = nullptr;
    }
    return e;
}

/* call only after the stream has been synchronised */
static void resolve_timers(mg3d_ctx *ctx)
{
    for (auto &p : ctx->pending) {
        float ms = 0.f;
        if (p.a && p.b && hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            StageTimer &t = ctx->timers[(size_t)p.slot];
            t.calls++;
            t.seconds += ms * 1e-3;
        }
        if (p.a)
            ctx->event_pool.push_back(p.a);
        if (p.b)
            ctx->event_pool.push_back(p.b);
    }
    ctx->pending.clear();
}

/* scoped event pair: a stage of the reference's timing table, or (kernel = true) one kernel launch.
 * timing: 1 every level, 2 the finest level, 3 the finest level's kernel scopes only (what bench.py's roofline needs: 8
 * marker packets per cycle instead of 24; each costs ~5 us of idle queue, 0.09 against 0.04 ms of a 3.3 ms cycle.  Binding
 * the pair to the dispatch itself, hipExtLaunchKernelGGL, measured the same 0.04 ms as the 8 markers: not kept), 4 + k
 * (k >= 0): as 3, but only every (k + 2)-th full cycle carries the markers (a sample of the timed region).
 * Declared in mg3d_ctx.h: mg3d_pcg.hip and mg3d_step.hip time a launch of theirs with it. */
StageScope::StageScope(mg3d_ctx *c, int l, int s, bool kernel) : ctx(c)
{
    p.slot = kernel ? c->L * MG3D_NUM_STAGES + l * MG3D_NUM_KERNELS + s : l * MG3D_NUM_STAGES + s;
    p.a = p.b = nullptr;
    on = ctx->timing == 1 || (ctx->timing == 2 && l == ctx->L - 1) ||
         (ctx->timing >= 3 && kernel && l == ctx->L - 1 && ctx->timing_phase == 0);
    if (on && (p.a = take_event(ctx)))
        (void)hipEventRecord(p.a, ctx->stream);
}
StageScope::~StageScope()
{
    if (!on)
        return;
    if ((p.b = take_event(ctx)))
        (void)hipEventRecord(p.b, ctx->stream);
    ctx->pending.push_back(p);
}

static void free_band(LuBand &b)
{
    for (double *p : {b.lcol, b.ucol, b.diag, b.lrot, b.urot, b.stream})
        if (p)
            (void)hipFree(p);
    if (b.in_map)
        (void)hipFree(b.in_map);
    memset(&b, 0, sizeof b);
}

void mg3d_free_lu(mg3d_ctx *ctx)
{
    free_band(ctx->lu);
    free_band(ctx->lu_in);
    if (ctx->lu_work)
        (void)hipFree(ctx->lu_work);
    ctx->lu_work = nullptr;
    ctx->have_lu = false;
}

extern "C" int mg3d_ctx_destroy(mg3d_ctx *ctx)
{
    if (!ctx)
        return MG3D_OK;
    if (ctx->stream)
        (void)hipStreamSynchronize(ctx->stream);
    for (auto &l : ctx->lv)
    {
        for (int k = 0; k < 3; k++)
            if (l.f[k])
                (void)hipFree(l.f[k]);
        if (l.alt)
            (void)hipFree(l.alt);
    }
    mg3d_free_lu(ctx);
    mg3d_field_free(ctx->eps);
    mg3d_field_free(ctx->mask);
    mg3d_field_free(ctx->sfield);
    mg3d_field_free(ctx->ones);
    if (ctx->per_b)
        (void)hipFree(ctx->per_b);
    for (double *v : ctx->pcg_v)
        if (v)
            (void)hipFree(v);
    if (ctx->step_src)
        (void)hipFree(ctx->step_src);
    if (ctx->nl_g)
        (void)hipFree(ctx->nl_g);
    for (double *v : ctx->nl_v)
        if (v)
            (void)hipFree(v);
    if (ctx->io_chk)
        (void)hipFree(ctx->io_chk);
    if (ctx->dep_acc)
        (void)hipFree(ctx->dep_acc);
    if (ctx->dep_max)
        (void)hipFree(ctx->dep_max);
    if (ctx->push_table)
        (void)hipFree(ctx->push_table);
    if (ctx->sort_buf)
        (void)hipFree(ctx->sort_buf);
    for (hipEvent_t e : ctx->io_ev)
        if (e)
            (void)hipEventDestroy(e);
    if (ctx->dz_map)
        (void)hipFree(ctx->dz_map);
    if (ctx->partials)
        (void)hipFree(ctx->partials);
    if (ctx->sumsq)
        (void)hipFree(ctx->sumsq);
    if (ctx->h_sumsq)
        (void)hipHostFree(ctx->h_sumsq);
    resolve_timers(ctx);
    for (hipEvent_t e : ctx->event_pool)
        (void)hipEventDestroy(e);
    if (ctx->stream && ctx->own_stream)
        (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return MG3D_OK;
}

/* ------------------------------------------------------------------ options
 * One table: key, environment override (read once per context creation), how the environment value maps, default. */
struct OptionRow {
    const char *key, *env;
    int mode; /* 0: the value is the integer; 1: "1" means 0 (a NO_ switch), anything else 1; 2: "rj,nw,pf" */
    int dflt;
};
static const OptionRow kOptionTable[MG3D_OPT_COUNT] = {
    {"carry", "MG3D_NO_CARRY", 1, 1},
    {"carry_min", "MG3D_CARRY_MIN", 0, 130},
    {"legs", "MG3D_LEGS", 0, 1},
    {"legs_min", "MG3D_LEGS_MIN", 0, 160},
    {"tiny", "MG3D_NO_TINY", 1, 1},
    {"tiny_cycle", "MG3D_NO_TINY_CYCLE", 1, 1},
    {"lu_reduced", "MG3D_LU_REDUCED", 0, 1},
    {"fuse_rst2", "MG3D_FUSE_RST2", 0, -1},
    {"small_max", "MG3D_SMALL_MAX", 0, 129},
    {"fuse_leg_max", "MG3D_FUSE_LEG_MAX", 0, 0},
    {"fuse_up_max", "MG3D_FUSE_UP_MAX", 0, 1 << 20},
    {"sweep_tune", "MG3D_SWEEP_TUNE", 0, -1},
    {"sweep_tune_log", "MG3D_SWEEP_TUNE_LOG", 0, 0},
    {"sweep_ci", "MG3D_SWEEP_CI", 0, 0},
    {"sweep_rj", "MG3D_SWEEP_CFG", 2, 0},
    {"sweep_nw", nullptr, 0, 0},
    {"sweep_pf", nullptr, 0, 0},
    {"d_zero_skip", "MG3D_D_ZERO_SKIP", 0, 1},
    {"zero_front", "MG3D_ZERO_FRONT", 0, 1},
    {"fuse_down_min", "MG3D_FUSE_DOWN_MIN", 0, 130},
};

void mg3d_options_init(mg3d_options *o)
{
    for (int i = 0; i < MG3D_OPT_COUNT; i++) {
        const OptionRow &r = kOptionTable[i];
        o->v[i] = r.dflt;
        const char *e = r.env ? getenv(r.env) : nullptr; /* context creation: the only place the environment is read */
        if (!e || !e[0])
            continue;
        if (r.mode == 0)
            o->v[i] = atoi(e);
        else if (r.mode == 1)
            o->v[i] = e[0] == '1' ? 0 : 1;
        else {
            int rj = 0, nw = 0, pf = 0;
            if (sscanf(e, "%d,%d,%d", &rj, &nw, &pf) >= 2) {
                o->v[MG3D_OPT_SWEEP_RJ] = rj;
                o->v[MG3D_OPT_SWEEP_NW] = nw;
                o->v[MG3D_OPT_SWEEP_PF] = pf;
            }
            i += 2; /* the two rows behind it were just set */
        }
    }
}

int mg3d_option_index(const char *key)
{
    if (key)
        for (int i = 0; i < MG3D_OPT_COUNT; i++)
            if (strcmp(key, kOptionTable[i].key) == 0)
                return i;
    return -1;
}

const char *mg3d_option_key(int index) { return index >= 0 && index < MG3D_OPT_COUNT ? kOptionTable[index].key : nullptr; }

extern "C" const char *mg3d_option_name(int index) { return mg3d_option_key(index); }

static mg3d_ctx *ctx_new(int L, int iters)
{
    mg3d_ctx *ctx = new mg3d_ctx();
    ctx->c = 0;
    ctx->length = 0.;
    ctx->L = L;
    ctx->iters = iters;
    ctx->have_lu = false;
    ctx->sigma = 0.;
    ctx->lu_built = false;
    ctx->lu_h = 0.;
    ctx->periodic = 0;
    ctx->neumann = 0;
    ctx->per_b = nullptr;
    memset(&ctx->lu, 0, sizeof ctx->lu);
    memset(&ctx->lu_in, 0, sizeof ctx->lu_in);
    ctx->lu_work = nullptr;
    ctx->partials = ctx->sumsq = ctx->h_sumsq = nullptr;
    ctx->sumsq_slots = 0;
    ctx->stream = nullptr;
    ctx->own_stream = true;
    ctx->timing = 0;
    ctx->timing_phase = 0;
    ctx->timers.assign((size_t)L * (MG3D_NUM_STAGES + MG3D_NUM_KERNELS), StageTimer{0, 0.});
    ctx->lv.resize(L);
    for (auto &l : ctx->lv)
        l.f[0] = l.f[1] = l.f[2] = l.alt = nullptr;
    ctx->have_es = false;
    ctx->faces_dirty.assign(L, 1);
    ctx->faces_always.assign(L, 0);
    ctx->fused = true;
    ctx->carried = false;
    ctx->legs_state = ctx->legs_slot = ctx->legs_npa = 0;
    mg3d_options_init(&ctx->opt);
    ctx->raw_top = false;
    if (hipGetDevice(&ctx->device) != hipSuccess)
        ctx->device = 0;
    ctx->keep_r = false;
    if (const char *e = getenv("MG3D_KEEP_R"))
        ctx->keep_r = e[0] == '1';
    if (const char *e = getenv("MG3D_NO_FUSE"))
        ctx->fused = !(e[0] == '1');
    return ctx;
}

/* carried cycles (see mg3d_enqueue_vcycle): back to the finished cycle's own result.  The launch that carried the cycle
 * over took u behind the cycle's first two post-smoothing passes (still intact in the alt buffer) through its last two,
 * tapped the norm there and went on into the next cycle: the finished cycle's u itself was never written.  It is those
 * two passes (black, red) from alt -- one launch, paid only when somebody wants to see or change the state between two
 * cycles.  Every entry point that reads or writes level data, or changes what a cycle is, calls this first; only
 * mg3d_vcycle(s) continue from the carried state. */
int mg3d_drop_carry(mg3d_ctx *ctx)
{
    /* whoever calls this may go on to change u or d of the top level: the next cycle can no longer rely on its first red
     * pass being the identity (red_tail, mg3d_enqueue_vcycle); mg3d_vcycle(s) themselves use mg3d_drop_carry_keep */
    if (ctx)
        ctx->red_tail = false;
    return mg3d_drop_carry_keep(ctx);
}

int mg3d_drop_carry_keep(mg3d_ctx *ctx)
{
    if (ctx && ctx->legs_state != 0) {
        /* one launch per leg: behind mg3d_vcycle the next cycle's down-leg has run ahead into the alt buffers; the finished
         * cycle's own u is intact in the top level's alt, the coarser level's right-hand side was never touched -- swap
         * back, no launch.  (State 2 only exists inside mg3d_vcycles: u is final, the norm's second half is abandoned.) */
        if (ctx->legs_state == 3) {
            swap_u(ctx->lv[ctx->L - 1]);
        }
        ctx->legs_state = 0;
    }
    if (!ctx || !ctx->carried)
        return MG3D_OK;
    Level &l = ctx->lv[ctx->L - 1];
    SweepLaunch w = mg3d_level_sweep(ctx, l); /* ... here the other way round: alt -> u, black, red */
    w.vin = l.alt;
    w.vout = l.f[MG3D_U];
    w.S = 2;
    w.c1 = 0;
    const int np = k_sweep(ctx->opt, w, ctx->stream);
    /* a failure leaves the context where it was -- u three passes into the next cycle, `carried` still set: the caller
     * returns the error instead of going on with (and handing out) a state nobody asked for; a later call tries again */
    if (np < 0)
        return fail(MG3D_ERR_STATE, "carried cycle: the two passes that finish it could not be launched");
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(MG3D_ERR_HIP, "carried cycle: the two passes that finish it: %s", hipGetErrorString(e));
    ctx->carried = false;
    return MG3D_OK;
}

void mg3d_ctx_touched(mg3d_ctx *ctx, int field, int level, bool raw_pointer, int how)
{
    /* d of the top level: what its zero map is worth now (dz_state, mg3d_ctx.h) */
    if (field == MG3D_D && level == ctx->L - 1 && how != MG3D_WROTE_FACES) {
        ctx->dz_raw = ctx->dz_raw || raw_pointer;
        if (ctx->dz_raw || how == MG3D_WROTE_DEVICE || !ctx->dz_map) {
            ctx->dz_state = MG3D_DZ_NONE;
        } else if (how == MG3D_WROTE_CALLER) {
            ctx->dz_state = MG3D_DZ_UNKNOWN;
        } else { /* cleared, in stream order behind the memset: every interior plane, nothing to scan */
            k_dzero_fill(ctx->lv[level].g, ctx->dz_map, ctx->stream);
            ctx->dz_state = MG3D_DZ_VALID;
            ctx->dz_planes = ctx->lv[level].g.ni > 2 ? ctx->lv[level].g.ni - 2 : 0;
        }
    }
    /* a raw device pointer to u or d of the top level: the library no longer sees every write to them, so a single
     * mg3d_vcycle call does not run ahead into the next cycle any more (mg3d_vcycles still carries INSIDE a call) */
    if (raw_pointer && level == ctx->L - 1 && (field == MG3D_U || field == MG3D_D))
        ctx->raw_top = true;
    const int l = field == MG3D_R ? level : field == MG3D_D ? level + 1 : -1;
    if (l >= 1 && l < ctx->L) {
        ctx->faces_dirty[l] = 1;
        if (raw_pointer)
            ctx->faces_always[l] = 1;
    }
}

static int ctx_create_sizes(const int *n_per_level, const double *h_per_level, int L, int iters, mg3d_ctx **out)
{
    CHK(require_device());
    mg3d_ctx *ctx = ctx_new(L, iters);
#define CTXCHK(call)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess) {                                                                          \
            int rc_ = mg3d_alloc_fail(e_, #call);                                                        \
            mg3d_ctx_destroy(ctx);                                                                       \
            return rc_;                                                                                  \
        }                                                                                                \
    } while (0)
    CTXCHK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    for (int l = 0; l < L; l++) {
        Level &lev = ctx->lv[l];
        const int N = n_per_level[l];
        lev.g.N = N;
        lev.g.ni = lev.g.nj = lev.g.nk = N;
        lev.g.ig0 = 0;
        lev.g.pitch = mg3d_pitch_for(N);
        lev.g.plane = (long long)lev.g.pitch * N;
        lev.h = h_per_level[l];
        lev.elems = (size_t)lev.g.plane * N;
        for (int k = 0; k < 3; k++) {
            CTXCHK(hipMalloc(&lev.f[k], lev.elems * sizeof(double)));
            CTXCHK(hipMemsetAsync(lev.f[k], 0, lev.elems * sizeof(double), ctx->stream)); /* calloc, mg_3d.h:44 */
        }
        CTXCHK(hipMalloc(&lev.alt, lev.elems * sizeof(double)));
        CTXCHK(hipMemsetAsync(lev.alt, 0, lev.elems * sizeof(double), ctx->stream));
    }
    CTXCHK(hipMalloc(&ctx->dz_map, mg3d_dzero_words(ctx->lv[L - 1].g.ni) * sizeof(unsigned)));
    CTXCHK(hipMalloc(&ctx->partials, MG3D_MAX_PARTIALS * sizeof(double)));
    ctx->sumsq_slots = 1024;
    CTXCHK(hipMalloc(&ctx->sumsq, ctx->sumsq_slots * sizeof(double)));
    CTXCHK(hipHostMalloc(&ctx->h_sumsq, ctx->sumsq_slots * sizeof(double)));
    CTXCHK(hipStreamSynchronize(ctx->stream));
#undef CTXCHK
    *out = ctx;
    return MG3D_OK;
}

extern "C" int mg3d_ctx_create(int coarse_pts, int num_levels, int smooth_iters, double grid_length, mg3d_ctx **out)
{
    if (!out || coarse_pts < 3 || num_levels < 1 || num_levels > 24 || smooth_iters < 0)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_create: bad arguments (c=%d L=%d iters=%d)", coarse_pts, num_levels,
                    smooth_iters);
    const long long finest = ((long long)(coarse_pts - 1) << (num_levels - 1)) + 1; /* mg_3d.h:126-127 */
    if (finest > 2049)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_create: finest grid %lld^3 too large", finest);
    std::vector<int> n(num_levels);
    std::vector<double> h(num_levels);
    const double spacing = grid_length / (double)(finest - 1); /* mg_3d.h:143 */
    for (int l = 0; l < num_levels; l++) {
        n[l] = (coarse_pts - 1) * (1 << l) + 1; /* mg_3d.h:41 */
        h[l] = 0.;
    }
    /* spacing doubles per coarser level exactly as vcycle does (h_coarse = 2*h, mg_3d.h:1303) */
    h[num_levels - 1] = spacing;
    for (int l = num_levels - 2; l >= 0; l--)
        h[l] = 2 * h[l + 1];
    CHK(ctx_create_sizes(n.data(), h.data(), num_levels, smooth_iters, out));
    (*out)->c = coarse_pts;
    (*out)->length = grid_length;
    return MG3D_OK;
}

extern "C" int mg3d_ctx_num_levels(const mg3d_ctx *ctx) { return ctx ? ctx->L : 0; }
extern "C" int mg3d_ctx_level_n(const mg3d_ctx *ctx, int level)
{
    return (ctx && level >= 0 && level < ctx->L) ? ctx->lv[level].g.N : 0;
}
extern "C" double mg3d_ctx_level_h(const mg3d_ctx *ctx, int level)
{
    return (ctx && level >= 0 && level < ctx->L) ? ctx->lv[level].h : 0.;
}
extern "C" int mg3d_ctx_set_keep_residual(mg3d_ctx *ctx, int keep)
{
    CHK(mg3d_drop_carry(ctx));
    if (!ctx)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_set_keep_residual: NULL context");
    ctx->keep_r = keep != 0;
    return MG3D_OK;
}

/* launch / schedule policy by key (the table in INTEGRATION.md): takes effect from the next call on; anything that
 * changes what a cycle is first finishes a cycle that has run ahead */
extern "C" int mg3d_ctx_set_option(mg3d_ctx *ctx, const char *key, int value)
{
    CHK(mg3d_drop_carry(ctx));
    if (!ctx)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_set_option: NULL context");
    const int i = mg3d_option_index(key);
    if (i < 0)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_set_option: no option \"%s\"", key ? key : "(null)");
    ctx->opt.v[i] = value;
    return MG3D_OK;
}

extern "C" int mg3d_ctx_get_option(const mg3d_ctx *ctx, const char *key, int *value)
{
    const int i = mg3d_option_index(key);
    if (!ctx || !value || i < 0)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_get_option: NULL argument or no option \"%s\"", key ? key : "(null)");
    *value = ctx->opt.v[i];
    return MG3D_OK;
}

extern "C" int mg3d_ctx_set_smooth_iters(mg3d_ctx *ctx, int iters)
{
    CHK(mg3d_drop_carry(ctx));
    if (!ctx || iters < 0)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_set_smooth_iters: bad arguments");
    ctx->iters = iters;
    return MG3D_OK;
}

/* --------------------------------------------------------------- coarse LU */
/* Banded, column-major copy of a row-major LU factor (entry (i, j) = at(i, j)) for the device solve:
 * bw = populated half bandwidth (max |i-j| with LU[i][j] != 0). */
template <class At> static int build_band(LuBand &out, long long n, At at)
{
    int bw = 1;
    for (long long i = 0; i < n; i++) {
        long long lo = 0, hi = n - 1;
        while (lo < i && at(i, lo) == 0.)
            lo++;
        while (hi > i && at(i, hi) == 0.)
            hi--;
        if (i - lo > bw)
            bw = (int)(i - lo);
        if (hi - i > bw)
            bw = (int)(hi - i);
    }
    std::vector<double> lcol((size_t)n * bw, 0.), ucol((size_t)n * bw, 0.), diag((size_t)2 * ((n + 63) / 64 * 64), 1.);
    int fast_div = 1;
    const long long npad = (n + 63) / 64 * 64;
    for (long long j = 0; j < n; j++) {
        diag[j] = at(j, j);
        /* reciprocal for lu_div(): correctly rounded by the host's IEEE division; 0 = "divide the ordinary way" */
        const double ad = fabs(diag[j]);
        if (!(ad >= 0x1p-460 && ad <= 0x1p460))
            fast_div = 0;
        diag[npad + j] = 1.0 / diag[j];
        for (int t = 0; t < bw; t++) {
            const long long il = j + 1 + t, iu = j - 1 - t;
            if (il < n)
                lcol[j * bw + t] = at(il, j);
            if (iu >= 0)
                ucol[j * bw + t] = at(iu, j);
        }
    }
    free_band(out);
    out.n = (int)n;
    out.bw = bw;
    out.fast_div = fast_div;
    out.npad = (int)npad;
    HIPCHK(hipMalloc(&out.lcol, lcol.size() * sizeof(double)));
    HIPCHK(hipMalloc(&out.ucol, ucol.size() * sizeof(double)));
    HIPCHK(hipMalloc(&out.diag, diag.size() * sizeof(double)));
    HIPCHK(hipMemcpy(out.lcol, lcol.data(), lcol.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(out.ucol, ucol.data(), ucol.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(out.diag, diag.data(), diag.size() * sizeof(double), hipMemcpyHostToDevice));
    /* narrow bands (coarse grids up to 11^3): lane-rotated copies for the single-wave kernel */
    const int R = (bw + 63) / 64;
    if (R <= 2 && 4 * (size_t)n * sizeof(double) <= 60000) {
        std::vector<double> lrot((size_t)n * 64 * R, 0.), urot((size_t)n * 64 * R, 0.);
        for (long long j = 0; j < n; j++)
            for (int q = 0; q < R; q++)
                for (int l = 0; l < 64; l++) {
                    const int tf = (int)((l - j - 1) & 63) + 64 * q, tb = (int)((j - 1 - l) & 63) + 64 * q;
                    const long long irow_f = j + 1 + tf, irow_b = j - 1 - tb;
                    if (tf < bw && irow_f < n)
                        lrot[(size_t)j * 64 * R + 64 * q + l] = at(irow_f, j);
                    if (tb < bw && irow_b >= 0)
                        urot[(size_t)j * 64 * R + 64 * q + l] = at(irow_b, j);
                }
        HIPCHK(hipMalloc(&out.lrot, lrot.size() * sizeof(double)));
        HIPCHK(hipMalloc(&out.urot, urot.size() * sizeof(double)));
        HIPCHK(hipMemcpy(out.lrot, lrot.data(), lrot.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(out.urot, urot.data(), urot.size() * sizeof(double), hipMemcpyHostToDevice));
        out.rot_r = R;
        /* stream for the loader/solver kernel (see lu_solve_stream_kernel) when its LDS ring fits */
        const int CH = mg3d_lu_stream_chunk((int)n, R);
        if (CH > 0) {
            const long long nch = npad / CH, step_d = 64 * R;
            std::vector<double> st((size_t)((2 * nch + 2) * CH * step_d), 0.);
            /* per lane the pair is stored as (factor for sum A, factor for sum B) of lu_stream_half: a lane
             * that has already finalised its unknown of the current 64-step chunk (or does so in this step)
             * carries its nearer row in B */
            for (long long j = 0; j < n; j++)
                for (int l = 0; l < 64; l++) {
                    const int of = (int)(j & 63), ob = (int)(j & 63);
                    const bool swf = R == 2 && l <= of, swb = R == 2 && l >= ob;
                    for (int q = 0; q < R; q++) {
                        const int qf = swf ? 1 - q : q, qb = swb ? 1 - q : q;
                        st[(size_t)(j * step_d + l * R + qf)] = lrot[(size_t)j * 64 * R + 64 * q + l];
                        st[(size_t)((npad + (npad - 1 - j)) * step_d + l * R + qb)] = urot[(size_t)j * 64 * R + 64 * q + l];
                    }
                }
            HIPCHK(hipMalloc(&out.stream, st.size() * sizeof(double)));
            HIPCHK(hipMemcpy(out.stream, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice));
            out.stream_ch = CH;
        }
    }
    return MG3D_OK;
}

static int install_lu(mg3d_ctx *ctx, const double *LU, long long n, size_t work_doubles)
{
    mg3d_free_lu(ctx);
    CHK(build_band(ctx->lu, n, [&](long long i, long long j) { return LU[i * n + j]; }));
    HIPCHK(hipMalloc(&ctx->lu_work, work_doubles * sizeof(double)));
    /* The reduced system.  A row of the factor that is the identity row (constructCoarseMatrixA's boundary rows,
     * mg_3d.h:179-185; elimination leaves them alone) gives x[i] = b[i] in both substitutions, and when that b[i] is
     * +-0 -- every boundary entry of a V-cycle's coarse right-hand side: the injected faces of a residual that is never
     * written there, mg_3d.h:824-825, 879-958 -- its products with other rows' factors are +-0 and change no running sum
     * (sums start at +0 and never become -0).  What is left is the factor restricted to the other rows (9^3: 343 of 729
     * unknowns, half-band 49 instead of 81): the same values in the same order for every remaining term, i.e. the same
     * bits, in less than half the strictly sequential steps.  The solve kernel checks the right-hand side and takes
     * the full system whenever an identity row's entry is not a zero (the F-cycle start, host-pointer calls). */
    if (!ctx->opt.v[MG3D_OPT_LU_REDUCED] || !ctx->lu.stream_ch) /* (option lu_reduced, read per factor: tests compare both) */
        return MG3D_OK;
    std::vector<int> map((size_t)n, -1), rows;
    for (long long i = 0; i < n; i++) {
        bool ident = LU[i * n + i] == 1.;
        const long long lo = i - ctx->lu.bw < 0 ? 0 : i - ctx->lu.bw, hi = i + ctx->lu.bw >= n ? n - 1 : i + ctx->lu.bw;
        for (long long j = lo; j <= hi && ident; j++)
            ident = j == i || LU[i * n + j] == 0.;
        if (!ident) {
            map[(size_t)i] = (int)rows.size();
            rows.push_back((int)i);
        }
    }
    const long long ni = (long long)rows.size(), npad_in = (ni + 63) / 64 * 64;
    if (ni == 0 || ni == n || 2 * npad_in > ctx->lu.npad)
        return MG3D_OK; /* nothing to gain, or the reduced vectors do not fit beside the full right-hand side in LDS */
    CHK(build_band(ctx->lu_in, ni, [&](long long a, long long b) { return LU[(long long)rows[(size_t)a] * n + rows[(size_t)b]]; }));
    if (!ctx->lu_in.stream_ch) {
        free_band(ctx->lu_in);
        return MG3D_OK;
    }
    HIPCHK(hipMalloc(&ctx->lu.in_map, (size_t)n * sizeof(int)));
    HIPCHK(hipMemcpy(ctx->lu.in_map, map.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    return MG3D_OK;
}

extern "C" int mg3d_ctx_set_lu(mg3d_ctx *ctx, const double *LU)
{
    CHK(mg3d_drop_carry(ctx));
    if (!ctx || !LU)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_set_lu: NULL argument");
    const int N0 = ctx->lv[0].g.N;
    const long long n = (long long)N0 * N0 * N0;
    if (n * n >= 2147483647LL) /* assert(totalNodes*totalNodes < INT_MAX), mg_3d.h:163 */
        return fail(MG3D_ERR_ARG, "mg3d_ctx_set_lu: coarse grid %d^3 too large for a dense factor", N0);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->lu_built = false;
    CHK(install_lu(ctx, LU, n, 2 * (size_t)n));
    ctx->have_lu = true;
    ctx->have_es = false; /* whatever factor was loaded before (mg3d_es_setup re-arms it after its own call) */
    return MG3D_OK;
}

extern "C" int mg3d_ctx_build_coarse(mg3d_ctx *ctx, double h_coarse)
{
    CHK(mg3d_drop_carry(ctx));
    if (!ctx)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_build_coarse: NULL context");
    const int N0 = ctx->lv[0].g.N;
    const long long n = (long long)N0 * N0 * N0;
    if (n * n >= 2147483647LL)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_build_coarse: coarse grid %d^3 too large for a dense factor", N0);
    double *A = (double *)calloc((size_t)(n * n), sizeof(double)); /* mg_3d.h:283 */
    if (!A)
        return fail(MG3D_ERR_ALLOC, "mg3d_ctx_build_coarse: out of host memory");
    mg3d_coarse_matrix_field(A, N0, h_coarse, ctx->eps.set() ? ctx->eps.host0.data() : nullptr, ctx->sigma, ctx->periodic,
                             ctx->neumann, ctx->mask.set() ? ctx->mask.host0.data() : nullptr,
                             ctx->sfield.set() ? ctx->sfield.host0.data() : nullptr); /* mg_3d.h:288 */
    mg3d_lu_factor(A, (int)n);                             /* mg_3d.h:289 */
    const int rc = mg3d_ctx_set_lu(ctx, A);
    free(A);
    if (rc == MG3D_OK) { /* remembered: mg3d_ctx_set_shift builds it again for another sigma */
        ctx->lu_built = true;
        ctx->lu_h = h_coarse;
    }
    return rc;
}

/* Device arrays (mg3d_array, include/mg3d.h): the descriptor checks and the stream join of every mg3d_*_device entry point. */
int mg3d_array_check(const mg3d_ctx *ctx, const mg3d_array *a, bool writable, const char *who, bool bytes)
{
    if (!a || !a->ptr)
        return fail(MG3D_ERR_ARG, "%s: NULL array", who);
    if (bytes && a->dtype != MG3D_U8)
        return fail(MG3D_ERR_ARG, "%s: dtype %d (MG3D_U8)", who, a->dtype);
    if (!bytes && a->dtype != MG3D_F64 && a->dtype != MG3D_F32)
        return fail(MG3D_ERR_ARG, "%s: dtype %d (MG3D_F64 or MG3D_F32)", who, a->dtype);
    for (int ax = 0; ax < 3; ax++)
        if (a->stride[ax] < (writable ? 1 : 0))
            return fail(MG3D_ERR_ARG, "%s: stride[%d] = %lld (%s)", who, ax, a->stride[ax],
                        writable ? "an array that is written needs every stride >= 1" : "a stride must be >= 0");
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    const hipError_t e = hipPointerGetAttributes(&at, a->ptr);
    if (e != hipSuccess) {
        (void)hipGetLastError(); /* (an unknown pointer is the caller's error, not a launch failure of the next kernel) */
        return fail(MG3D_ERR_ARG, "%s: %p is not device memory (%s)", who, a->ptr, hipGetErrorString(e));
    }
    if (at.type != hipMemoryTypeDevice || at.device != ctx->device)
        return fail(MG3D_ERR_ARG, "%s: %p is not device memory of device %d (memory type %d, device %d)", who, a->ptr,
                    ctx->device, (int)at.type, at.device);
    return MG3D_OK;
}

int mg3d_stream_join(mg3d_ctx *ctx, hipStream_t caller, bool out, const char *who)
{
    hipEvent_t &ev = ctx->io_ev[out ? 1 : 0];
    hipError_t e = hipSuccess;
    if (!ev)
        e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e == hipSuccess)
        e = hipEventRecord(ev, out ? ctx->stream : caller);
    if (e == hipSuccess)
        e = hipStreamWaitEvent(out ? caller : ctx->stream, ev, 0);
    if (e != hipSuccess)
        return fail(MG3D_ERR_HIP, "%s: joining the caller's stream: %s", who, hipGetErrorString(e));
    return MG3D_OK;
}

/* ----------------------------------------------------------- data movement */
int mg3d_check_field_level(const mg3d_ctx *ctx, int field, int level, const char *who)
{
    if (!ctx || field < 0 || field > 2 || level < 0 || level >= ctx->L)
        return fail(MG3D_ERR_ARG, "%s: bad field/level (%d, %d)", who, field, level);
    return MG3D_OK;
}

extern "C" int mg3d_upload(mg3d_ctx *ctx, int field, int level, const double *host)
{
    CHK(mg3d_drop_carry(ctx));
    CHK(mg3d_check_field_level(ctx, field, level, "mg3d_upload"));
    if (!host)
        return fail(MG3D_ERR_ARG, "mg3d_upload: NULL host pointer");
    const Level &l = ctx->lv[level];
    const int N = l.g.N;
    HIPCHK(hipMemcpy2DAsync(l.f[field], l.g.pitch * sizeof(double), host, N * sizeof(double), N * sizeof(double),
                            (size_t)N * N, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    mg3d_ctx_touched(ctx, field, level, false, MG3D_WROTE_CALLER);
    return MG3D_OK;
}

extern "C" int mg3d_download(mg3d_ctx *ctx, int field, int level, double *host)
{
    CHK(mg3d_drop_carry_keep(ctx)); /* (reads only: the next cycle may still continue behind the last one, see red_tail) */
    CHK(mg3d_check_field_level(ctx, field, level, "mg3d_download"));
    if (!host)
        return fail(MG3D_ERR_ARG, "mg3d_download: NULL host pointer");
    const Level &l = ctx->lv[level];
    const int N = l.g.N;
    HIPCHK(hipMemcpy2DAsync(host, N * sizeof(double), l.f[field], l.g.pitch * sizeof(double), N * sizeof(double),
                            (size_t)N * N, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return MG3D_OK;
}

/* The device-array forms: the arguments are checked before anything happens, then the carried state is treated as in the
 * host form, and the kernel runs on the context's stream between the two halves of the join -- no host synchronisation. */
extern "C" int mg3d_upload_device(mg3d_ctx *ctx, int field, int level, const mg3d_array *src, void *stream)
{
    static const char who[] = "mg3d_upload_device";
    CHK(mg3d_check_field_level(ctx, field, level, who));
    CHK(mg3d_array_check(ctx, src, false, who));
    CHK(mg3d_drop_carry(ctx));
    const Level &l = ctx->lv[level];
    CHK(mg3d_stream_join(ctx, (hipStream_t)stream, false, who));
    {
        StageScope kt(ctx, level, MG3D_K_PACK, true);
        k_pack(l.g, l.f[field], *src, ctx->stream);
    }
    mg3d_ctx_touched(ctx, field, level, false, MG3D_WROTE_CALLER);
    CHK(mg3d_launch_ok(who));
    return mg3d_stream_join(ctx, (hipStream_t)stream, true, who);
}

extern "C" int mg3d_download_device(mg3d_ctx *ctx, int field, int level, const mg3d_array *dst, void *stream)
{
    static const char who[] = "mg3d_download_device";
    CHK(mg3d_check_field_level(ctx, field, level, who));
    CHK(mg3d_array_check(ctx, dst, true, who));
    CHK(mg3d_drop_carry_keep(ctx)); /* (reads only, as mg3d_download) */
    const Level &l = ctx->lv[level];
    CHK(mg3d_stream_join(ctx, (hipStream_t)stream, false, who)); /* (what the caller's stream still does with dst) */
    {
        StageScope kt(ctx, level, MG3D_K_PACK, true);
        k_unpack(l.g, l.f[field], *dst, ctx->stream);
    }
    CHK(mg3d_launch_ok(who));
    return mg3d_stream_join(ctx, (hipStream_t)stream, true, who);
}

extern "C" int mg3d_zero(mg3d_ctx *ctx, int field, int level)
{
    CHK(mg3d_drop_carry(ctx));
    CHK(mg3d_check_field_level(ctx, field, level, "mg3d_zero"));
    const Level &l = ctx->lv[level];
    HIPCHK(hipMemsetAsync(l.f[field], 0, l.elems * sizeof(double), ctx->stream));
    mg3d_ctx_touched(ctx, field, level, false, MG3D_WROTE_ZERO);
    return MG3D_OK;
}

extern "C" int mg3d_sync(mg3d_ctx *ctx)
{
    if (!ctx)
        return fail(MG3D_ERR_ARG, "mg3d_sync: NULL context");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    resolve_timers(ctx);
    return MG3D_OK;
}

extern "C" int mg3d_device_view(mg3d_ctx *ctx, int field, int level, void **dev_ptr, int *pitch_doubles,
                                long *plane_doubles)
{
    CHK(mg3d_drop_carry(ctx));
    CHK(mg3d_check_field_level(ctx, field, level, "mg3d_device_view"));
    const Level &l = ctx->lv[level];
    mg3d_ctx_touched(ctx, field, level, true);
    if (dev_ptr)
        *dev_ptr = l.f[field];
    if (pitch_doubles)
        *pitch_doubles = l.g.pitch;
    if (plane_doubles)
        *plane_doubles = (long)l.g.plane;
    return MG3D_OK;
}

/* what the context knows of the zero map of the top level's d (tests, tools): the planes whose bit is set -- 0 unless the
 * map is valid -- and the state itself */
extern "C" int mg3d_ctx_dzero_planes(const mg3d_ctx *ctx, int *planes, int *state)
{
    if (!ctx)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_dzero_planes: NULL context");
    if (planes)
        *planes = ctx->dz_state == MG3D_DZ_VALID ? ctx->dz_planes : 0;
    if (state)
        *state = ctx->dz_state;
    return MG3D_OK;
}

/* launches that took a kernel without d (mg3d_ctx.h, dnone_launches) */
extern "C" int mg3d_ctx_dnone_launches(const mg3d_ctx *ctx, unsigned long long *launches)
{
    if (!ctx || !launches)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_dnone_launches: NULL argument");
    *launches = ctx->dnone_launches;
    return MG3D_OK;
}

/* the sweep launches this context has taken, by kind (mg3d_ctx.h, sweep_taken; SweepTakenLog): host bookkeeping only */
extern "C" int mg3d_ctx_sweep_taken(const mg3d_ctx *ctx, int kind, int which, int out[MG3D_SWEEP_TAKEN_FIELDS],
                                    unsigned long long *count, unsigned long long *launches)
{
    static_assert(sizeof(SweepTaken) == MG3D_SWEEP_TAKEN_FIELDS * sizeof(int), "SweepTaken is the MG3D_SWEEP_TAKEN_* fields in order");
    static_assert(MG3D_SWEEP_KIND_LEG_UP + 1 == MG3D_SWEEP_KINDS && MG3D_SWEEP_KIND_PASSES == SWEEP_PASSES &&
                      MG3D_SWEEP_KIND_PASSES_RES == SWEEP_PASSES_RES && MG3D_SWEEP_KIND_TAP == SWEEP_TAP &&
                      MG3D_SWEEP_KIND_LEG_DOWN == SWEEP_LEG_DOWN && MG3D_SWEEP_KIND_LEG_UP == SWEEP_LEG_UP,
                  "MG3D_SWEEP_KIND_* are SweepKind");
    if (!ctx || !out)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_sweep_taken: NULL argument");
    if (kind < 0 || kind >= MG3D_SWEEP_KINDS || which < 0)
        return fail(MG3D_ERR_ARG, "mg3d_ctx_sweep_taken: no such kind, or a negative index");
    const SweepTakenLog &log = ctx->sweep_taken;
    const bool have = which < log.n[kind];
    if (have)
        memcpy(out, &log.e[kind][which].t, sizeof(SweepTaken));
    else
        memset(out, 0, sizeof(SweepTaken));
    if (count)
        *count = have ? log.e[kind][which].count : 0;
    if (launches)
        *launches = log.launches[kind];
    return MG3D_OK;
}

/* ----------------------------------------------------------------- operators */
int mg3d_launch_ok(const char *who)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(MG3D_ERR_HIP, "%s: kernel launch failed: %s", who, hipGetErrorString(e));
    return MG3D_OK;
}

static int read_norm(mg3d_ctx *ctx, int slot, double *norm)
{
    if (!norm)
        return MG3D_OK;
    HIPCHK(hipMemcpyAsync(ctx->h_sumsq + slot, ctx->sumsq + slot, sizeof(double), hipMemcpyDeviceToHost,
                          ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    resolve_timers(ctx);
    *norm = sqrt(ctx->h_sumsq[slot]); /* mg_3d.h:841 */
    return MG3D_OK;
}

/* what mg3d_stage_plan is asked about a stage on a level of this context */
static StageAsk stage_ask(const mg3d_ctx *ctx, int level, int post, int iters, int want_res, bool has_coarse, bool need_norm,
                          bool pro_offered, bool zero_in = false)
{
    const Geom &g = ctx->lv[level].g;
    return StageAsk{g.N, g.nj, post != 0, iters, want_res, has_coarse, need_norm, pro_offered, /* leg4_form */ true, zero_in,
                    /* down_form */ true};
}

/* One launch of a stage's list on a single-domain level (fused sweep): u -> alt, swapped behind a launch with passes; the
 * residual's partial sums folded into sumsq[slot].  first: the stage's first launch (zero_in applies to it). */
static int enqueue_stage_step(mg3d_ctx *ctx, int level, int post, const StageStep &st, bool first, int want_res, int slot,
                              Level *coarse, const Level *pro, bool zero_in, bool need_norm)
{
    Level &l = ctx->lv[level];
    SweepLaunch w = mg3d_level_sweep(ctx, l);
    w.kind = st.res ? SWEEP_PASSES_RES : SWEEP_PASSES;
    w.S = st.S;
    w.c1 = post ? 0 : 1; /* pre: red first (mg_3d.h:657); post: black first (mg_3d.h:728) */
    if (zero_in && first)
        w.vin = nullptr;
    if (st.res && want_res == 2 && !st.rst)
        w.r = l.f[MG3D_R];
    if (st.res && need_norm)
        w.partials = ctx->partials;
    if (st.rst) {
        w.gc = &coarse->g;
        w.dc = coarse->f[MG3D_D];
    }
    if (st.pro) {
        w.gce = &pro->g;
        w.ec = pro->f[MG3D_U];
    }
    int np;
    {
        StageScope kt(ctx, level, st.S == 4 ? MG3D_K_SWEEP4 : st.S == 2 ? (st.res ? MG3D_K_SWEEP2_RES : MG3D_K_SWEEP2)
                                                                        : MG3D_K_RESIDUAL, true);
        np = k_sweep(ctx->opt, w, ctx->stream);
    }
    if (np < 0) /* nothing was launched: no buffer swap, no fold of partial sums that were never written */
        return fail(MG3D_ERR_STATE, "fused sweep: no kernel for %d colour passes%s on level %d", st.S,
                    st.res ? " + residual" : "", level);
    if (st.S > 0)
        swap_u(l);
    if (st.res && need_norm)
        k_fold(ctx->partials, np, ctx->sumsq + slot, ctx->stream);
    return MG3D_OK;
}

/* iters x (two colour passes), optionally followed by the residual of the result.
 * Fused path: the launches of mg3d_stage_plan, each reading u and writing the alternate buffer; the
 * residual rides on the last launch.  want_res: 0 none, 1 norm only,
 * 2 store r (+ norm).  The squared norm goes to sumsq[slot]. */
static int enqueue_smooth_residual(mg3d_ctx *ctx, int level, int post, int iters, int want_res, int slot,
                                    Level *coarse = nullptr, const Level *pro = nullptr, bool zero_in = false,
                                    bool need_norm = true)
{
    /* need_norm = false: only r (or its restriction) is wanted -- the V-cycle drops the pre-smoothing norm
     * (mg_3d.h:1294 ignores calculateResidual's value) -- so no partial sums are produced or folded */
    /* zero_in: u of this level is to be taken as identically zero (the memset of mg_3d.h:1258-1259 folded
     * into the first launch: it neither reads u nor needs it zeroed); only valid when a launch with S > 0 follows */
    /* pro != NULL: the smoother's input is u + P(pro->u) (prolongateAndCorrectError, mg_3d.h:1331, folded
     * into the first launch's loads) where the stage's list says so: the caller asks pro_fusable() first */
    /* coarse != NULL (with want_res != 0): the residual is restricted on the fly into the interior of
     * coarse->d and never stored; the caller adds the face injection (k_restrict, faces_only) */
    Level &l = ctx->lv[level];
    hipStream_t s = ctx->stream;
    if (mg3d_fused(ctx)) {
        const StagePlan plan = mg3d_stage_plan(ctx->opt, stage_ask(ctx, level, post, iters, want_res, coarse != nullptr, need_norm,
                                                                   pro != nullptr, zero_in));
        for (int k = 0; mg3d_stage_launch(plan, k); k++)
            CHK(enqueue_stage_step(ctx, level, post, *mg3d_stage_launch(plan, k), k == 0, want_res, slot, coarse, pro, zero_in, need_norm));
        return MG3D_OK;
    }
    const int c1 = post ? 0 : 1;
    const LevelOperator A = mg3d_level_operator(ctx, level);
    for (int it = 0; it < 2 * iters; it++) {
        StageScope kt(ctx, level, MG3D_K_COLOUR_PASS, true);
        k_smooth_color(l.g, l.f[MG3D_U], l.f[MG3D_D], A, c1 ^ (it & 1), s);
    }
    if (want_res) {
        StageScope kt(ctx, level, MG3D_K_RESIDUAL, true);
        k_residual(l.g, l.f[MG3D_U], l.f[MG3D_D], A, want_res == 2 ? l.f[MG3D_R] : nullptr, ctx->partials, ctx->sumsq + slot, s);
    }
    return MG3D_OK;
}

/* can the prolongation ride on the first smoothing launch?  (asked of the stage's own list: it needs a smoothing-only first
 * launch of a shape with the registers for it) */
static bool pro_fusable(const mg3d_ctx *ctx, int iters, int want_res, int level)
{
    return mg3d_fused(ctx) && mg3d_stage_plan(ctx->opt, stage_ask(ctx, level, 1, iters, want_res, false, true, true)).step[0].pro;
}

/* the unfused grid transfers and the direct solve (the launchers take the form for the context's boundary word) */
static void enqueue_restrict(mg3d_ctx *ctx, int level, bool faces_only = false)
{
    const Level &lev = ctx->lv[level], &lc = ctx->lv[level - 1];
    k_restrict(lev.g, lev.f[MG3D_R], lc.g, lc.f[MG3D_D], mg3d_ctx_bc(ctx), ctx->stream, -1, -1, faces_only);
}

static void enqueue_prolong(mg3d_ctx *ctx, int level)
{
    const Level &lev = ctx->lv[level], &lc = ctx->lv[level - 1];
    k_prolong(lc.g, lc.f[MG3D_U], lev.g, lev.f[MG3D_U], mg3d_ctx_bc(ctx), ctx->stream, -1, -1, mg3d_level_operator(ctx, level).m);
}

/* The direct solve.  Where the coarsest matrix has identity rows inside the domain -- fixed points, the duplicates of a
 * periodic axis, the pinned point (mg3d_ctx_pinned) of Neumann faces all round -- the factor solves for b = d with those
 * rows' values in place (k_coarse_rhs: 0; a one-level context has no cycle above the solve, its fixed points keep u's own
 * values); the duplicates of x are then copied from their sources.  Otherwise (Dirichlet faces, Neumann faces without the
 * pin) b is d itself, and there is no duplicate to refresh */
static void enqueue_coarse_solve(mg3d_ctx *ctx, const double *rhs = nullptr /* NULL: d of level 0 */,
                                 bool own_values = false /* the fixed points keep u's values (mg3d_fmg_solve: the solve of the problem itself) */)
{
    Level &l0 = ctx->lv[0];
    if (!rhs)
        rhs = l0.f[MG3D_D];
    const int bc = mg3d_ctx_bc(ctx), pin = mg3d_ctx_pinned(ctx);
    const unsigned char *m = mg3d_level_operator(ctx, 0).m;
    if (m || ctx->periodic || (ctx->neumann && pin)) {
        k_coarse_rhs(l0.g, rhs, ctx->per_b, bc, pin, m, (ctx->L == 1 || own_values) ? l0.f[MG3D_U] : nullptr, ctx->stream);
        rhs = ctx->per_b;
    }
    k_lu_solve(ctx->lu, ctx->lu_in, l0.g, rhs, l0.f[MG3D_U], ctx->lu_work, ctx->stream);
    k_per_refresh(l0.g, l0.f[MG3D_U], bc, ctx->stream);
}

static int enqueue_smooth(mg3d_ctx *ctx, int level, int post, int iters)
{
    return enqueue_smooth_residual(ctx, level, post, iters, 0, 0);
}

static int enqueue_residual(mg3d_ctx *ctx, int level, int store, int slot)
{
    return enqueue_smooth_residual(ctx, level, 0, 0, store ? 2 : 1, slot);
}

extern "C" int mg3d_smooth(mg3d_ctx *ctx, int level, int post, int iters)
{
    CHK(mg3d_drop_carry(ctx));
    CHK(mg3d_check_field_level(ctx, 0, level, "mg3d_smooth"));
    if (iters < 0)
        return fail(MG3D_ERR_ARG, "mg3d_smooth: negative iteration count");
    CHK(enqueue_smooth(ctx, level, post, iters));
    return mg3d_launch_ok("mg3d_smooth");
}

extern "C" int mg3d_residual(mg3d_ctx *ctx, int level, int store, double *norm)
{
    CHK(mg3d_drop_carry(ctx));
    CHK(mg3d_check_field_level(ctx, 0, level, "mg3d_residual"));
    CHK(enqueue_residual(ctx, level, store, 0));
    CHK(mg3d_launch_ok("mg3d_residual"));
    return read_norm(ctx, 0, norm);
}

extern "C" int mg3d_smooth_residual(mg3d_ctx *ctx, int level, int post, int iters, int store, double *norm)
{
    CHK(mg3d_drop_carry(ctx));
    CHK(mg3d_check_field_level(ctx, 0, level, "mg3d_smooth_residual"));
    if (iters < 0)
        return fail(MG3D_ERR_ARG, "mg3d_smooth_residual: negative iteration count");
    CHK(enqueue_smooth_residual(ctx, level, post, iters, store ? 2 : 1, 0));
    CHK(mg3d_launch_ok("mg3d_smooth_residual"));
    return read_norm(ctx, 0, norm);
}

extern "C" int mg3d_smooth_restrict(mg3d_ctx *ctx, int level, int iters)
{
    CHK(mg3d_drop_carry(ctx));
    CHK(mg3d_check_field_level(ctx, 0, level, "mg3d_smooth_restrict"));
    if (level < 1 || iters < 0)
        return fail(MG3D_ERR_ARG, "mg3d_smooth_restrict: bad level/iteration count");
    Level &lc = ctx->lv[level - 1];
    CHK(enqueue_smooth_residual(ctx, level, 0, iters, 2, ctx->sumsq_slots - 1, mg3d_fused(ctx) ? &lc : nullptr, nullptr, false,
                                /* need_norm: only without the fused restriction, whose shapes have no norm */ !mg3d_fused(ctx)));
    enqueue_restrict(ctx, level, mg3d_fused(ctx));
    return mg3d_launch_ok("mg3d_smooth_restrict");
}

extern "C" int mg3d_restrict(mg3d_ctx *ctx, int level)
{
    CHK(mg3d_drop_carry(ctx));
    CHK(mg3d_check_field_level(ctx, 0, level, "mg3d_restrict"));
    if (level < 1)
        return fail(MG3D_ERR_ARG, "mg3d_restrict: level 0 has no coarser level");
    enqueue_restrict(ctx, level);
    return mg3d_launch_ok("mg3d_restrict");
}

extern "C" int mg3d_prolong(mg3d_ctx *ctx, int level)
{
    CHK(mg3d_drop_carry(ctx));
    CHK(mg3d_check_field_level(ctx, 0, level, "mg3d_prolong"));
    if (level < 1)
        return fail(MG3D_ERR_ARG, "mg3d_prolong: level 0 has no coarser level");
    enqueue_prolong(ctx, level);
    return mg3d_launch_ok("mg3d_prolong");
}

extern "C" int mg3d_coarse_solve(mg3d_ctx *ctx)
{
    CHK(mg3d_drop_carry(ctx));
    if (!ctx)
        return fail(MG3D_ERR_ARG, "mg3d_coarse_solve: NULL context");
    if (!ctx->have_lu)
        return fail(MG3D_ERR_STATE, "mg3d_coarse_solve: no coarse LU set (mg3d_ctx_build_coarse / mg3d_ctx_set_lu)");
    if (ctx->have_es)
        return fail(MG3D_ERR_STATE, "mg3d_coarse_solve: the context holds the mixed-boundary factor of mg3d_es_setup");
    enqueue_coarse_solve(ctx);
    return mg3d_launch_ok("mg3d_coarse_solve");
}

extern "C" int mg3d_l2norm(mg3d_ctx *ctx, int field, int level, double *norm)
{
    CHK(mg3d_drop_carry_keep(ctx)); /* (reads only) */
    CHK(mg3d_check_field_level(ctx, field, level, "mg3d_l2norm"));
    k_sumsq(ctx->lv[level].g, ctx->lv[level].f[field], ctx->partials, ctx->sumsq, ctx->stream);
    CHK(mg3d_launch_ok("mg3d_l2norm"));
    return read_norm(ctx, 0, norm);
}

/* ------------------------------------------------------------------ V-cycle */
/* vcycle, mg_3d.h:1242-1362, unrolled: descend q..1, solve level 0, ascend 1..q.
 * The squared post-smoothing norm of level q goes to sumsq[slot]. */
/* Carried cycles.  Back to back, V-cycle n ends with post-smoothing passes black, red, black, red and the residual norm,
 * and cycle n+1 begins with pre-smoothing passes red, black, red, black on the same u and d (mg_3d.h:728 / :657).  That
 * first red pass recomputes every red point from black neighbours no pass has touched since the red pass before it: the
 * same operands in the same expression, the same bits -- it is the identity.  What is left is ONE alternating run
 *      [prolongation] B R | B R <norm of cycle n> B R | B [residual, restriction]
 * which three launches cover instead of four: prolongation + 2 passes (as before), four passes with the norm tapped
 * after the second (SWEEP_TAP: no stage of its own), one pass + residual + restriction -- 9 n w + 2 n_c w instead of
 * 11 n w + 2 n_c w compulsory bytes per cycle on the top level.  The tap launch reads u of cycle n and writes the other
 * buffer; cycle n's own u (the tapped state) is never written -- mg3d_drop_carry makes it from that input when it is
 * wanted.  mg3d_vcycles never ends a call in the carried state (its last cycle ends the ordinary way); mg3d_vcycle does.  Only V(2,2) from the finest level of a context with
 * at least three levels, fused sweeps, r not kept; MG3D_NO_CARRY=1 switches it off (tests compare both). */
/* One launch per leg ("two launches per level", round 4).  The alternating run of colour passes between two cycles
 *      [prolongation] B R B R <norm of cycle n> (R = identity) B R B [residual, restriction]
 * is cut at the norm instead: the up-leg is ONE launch (prolongation + four passes, SWEEP_LEG_UP) and the down-leg is ONE
 * launch (three passes + residual + restriction, SWEEP_LEG_DOWN) -- 6 n w + 2 n_c w compulsory bytes per cycle on the top
 * level instead of 9 n w + 2 n_c w.  No launch has a stage for the norm: the residual of the points the up-leg's last pass
 * (red) has just updated falls out of that pass's neighbour sums, the residual of the black points out of the sums the
 * next down-leg's first pass (black) forms before it updates them -- two runs of partial sums, folded into one norm.  The
 * cycle's own u is the up-leg's output: nothing is speculative inside mg3d_vcycles.  Behind a single mg3d_vcycle call
 * the next cycle's down-leg runs at once, into the alt buffers (u of the top level, d of the level below), so that the
 * norm is complete when the call returns; whatever the caller does instead of another cycle swaps back
 * (mg3d_drop_carry: no launch).  Same conditions as the carried cycles.  Default from 160 points per side (option
 * legs_min): same-box A/B by size, round 4 (ms per cycle, carried / legs): 385^3 1.23 / 1.30, 513^3 2.53 / 2.45, 641^3 4.99 / 4.80,
 * 769^3 11.31 / 10.76, 1025^3 20.65 / 16.79 (profiles/r04_legs_by_size.txt); option legs = 0 keeps the carried cycles. */
bool mg3d_can_legs(const mg3d_ctx *ctx, int q)
{
    /* the conditions of the carried cycles, except their own switch and threshold */
    const Geom &g = ctx->lv[q].g;
    return mg3d_fused(ctx) && !ctx->have_es && q == ctx->L - 1 && q >= 2 &&
           mg3d_can_run_ahead(ctx->opt, true, -1, ctx->iters, ctx->keep_r, g.N, g.nj);
}

bool mg3d_can_carry(const mg3d_ctx *ctx, int q)
{
    /* from 257^3 up: there the launch saved is bytes (257^3: +5 %, 513^3: +17 %, 1025^3: +16 % V-cycles/s); at 129^3 a
     * launch is pipeline fill and the plain schedule's lighter launches are 1 % ahead.  MG3D_CARRY_MIN=<points per side>
     * moves the threshold (the tests run 129^3 problems); never at 65^3 and below (the two launches only exist in
     * the four-rows-per-thread shapes) */
    const Geom &g = ctx->lv[q].g;
    return mg3d_fused(ctx) && !ctx->have_es && q == ctx->L - 1 && q >= 2 &&
           mg3d_can_run_ahead(ctx->opt, false, -1, ctx->iters, ctx->keep_r, g.N, g.nj) &&
           pro_fusable(ctx, 2, 1, q); /* the split up-leg whose first launch the carried cycle keeps */
}

/* What one cycle does on which level, settled before its first launch (mg3d_enqueue_vcycle). */
struct CycleState {
    int q, slot, carry_out;
    bool tiny;      /* level 1 below the top of the cycle, small enough for one workgroup's LDS: two launches instead of five */
    bool tiny_cyc;  /* ... and the whole bottom of the cycle (level 1 down, the direct solve, level 1 up) as ONE launch when the
                       reduced factor exists (mg3d_tiny.hip, tiny_cycle_kernel); MG3D_NO_TINY_CYCLE=1 keeps the three launches
                       (tests compare) */
    bool can_legs, can_carry;
    bool carry_in;  /* the previous cycle carried into this one */
    int legs_in;    /* legs_state the previous cycle left */
    /* red_tail: the last thing that happened to u of the top level was the red pass that ends a cycle, and nothing has touched
     * u or d since (every entry point that could clears the flag through mg3d_drop_carry; not once a raw pointer is out) --
     * this cycle's first red pass is the identity then, ACROSS calls as inside one: its down-leg is the one launch of three
     * passes + residual + restriction (no norm half: the finished cycle formed its norm itself) instead of four passes, then
     * residual + restriction (0.84 against 0.67 + 0.50 ms at 513^3) */
    bool red_in;
};

static double *part_a(mg3d_ctx *ctx) { return ctx->partials; } /* the two halves of a norm that two leg launches form */
static double *part_b(mg3d_ctx *ctx) { return ctx->partials + MG3D_MAX_PARTIALS / 2; }

/* The face injection of the restriction l -> l-1 (:879-958), inside the caller's MG3D_ST_RESTRICT scope.  faces_only: the
 * interior was restricted on the fly, and the faces only have something new to copy after r of this level or d of the
 * coarser one was written from outside the cycle (faces_dirty), or always once a raw pointer to one of them is out. */
static void restrict_stage(mg3d_ctx *ctx, int l, bool faces_only)
{
    if (faces_only && !ctx->faces_dirty[l] && !ctx->faces_always[l])
        return;
    StageScope kt(ctx, l, MG3D_K_RESTRICT, true);
    /* (periodic axes: never faces_only -- the periodic faces are fully weighted on every cycle) */
    enqueue_restrict(ctx, l, faces_only);
    ctx->faces_dirty[l] = 0;
}

/* behind a down-leg whose one launch held the residual and the restriction: both stages counted (~0 s), the faces injected */
static void down_leg_tail(mg3d_ctx *ctx, int l)
{
    { StageScope t(ctx, l, MG3D_ST_RESIDUAL1); }
    StageScope t(ctx, l, MG3D_ST_RESTRICT);
    restrict_stage(ctx, l, true);
}

/* the three-pass down-leg launch of the one-launch-per-leg schedule: black, red, black (the first red pass is the identity
 * behind a finished cycle) + residual + restriction into dc (:1282 + :1294 + :1310).  norm_half: on its way the black half
 * of the norm of the cycle in front of it, folded with that cycle's red half (npa partial sums) into sumsq[slot]. */
static int launch_leg_down(mg3d_ctx *ctx, int l, double *dc, bool norm_half, int npa, int slot)
{
    Level &lev = ctx->lv[l], &lc = ctx->lv[l - 1];
    SweepLaunch w = mg3d_level_sweep(ctx, lev);
    w.kind = SWEEP_LEG_DOWN;
    w.S = 3;
    w.gc = &lc.g;
    w.dc = dc;
    w.partials = norm_half ? part_b(ctx) : nullptr;
    w.max_partials = MG3D_MAX_PARTIALS / 2;
    StageScope kt(ctx, l, MG3D_K_LEG_DOWN, true);
    const int np = k_sweep(ctx->opt, w, ctx->stream);
    if (np < 0)
        return fail(MG3D_ERR_STATE, "one launch per leg: no kernel for the down-leg");
    swap_u(lev);
    if (norm_half)
        k_fold2(part_a(ctx), npa, part_b(ctx), np, ctx->sumsq + slot, ctx->stream);
    return MG3D_OK;
}

/* down-leg of the top level, one launch per leg, behind another cycle (legs_in) or a finished one (red_in).
 * (a cycle with no cycle in front of it takes the ordinary down-leg -- four passes, then residual +
 * restriction: the one-launch form of THAT leg needs a six-plane window, spills 180 bytes at eight rows per thread
 * and took 2.1 ms against 0.66 + 0.49: profiles/r04_bench_kernel_stats_note.txt) */
static int down_leg_ahead(mg3d_ctx *ctx, const CycleState &c, int l)
{
    Level &lc = ctx->lv[l - 1];
    {
        StageScope t(ctx, l, MG3D_ST_SMOOTH1);
        if (c.legs_in == 3) {
            /* this cycle's down-leg ran behind the previous mg3d_vcycle call: its u is the top level's u already,
             * its restricted residual sits in the coarser level's alt buffer */
            double *t2 = lc.f[MG3D_D];
            lc.f[MG3D_D] = lc.alt;
            lc.alt = t2;
            ctx->faces_dirty[l] = 1; /* the two buffers take turns as d: inject the faces into this one */
        } else {
            /* (behind a cycle of this call: the black half of its norm; behind a finished one: none) */
            CHK(launch_leg_down(ctx, l, lc.f[MG3D_D], !c.red_in, ctx->legs_npa, ctx->legs_slot));
        }
    }
    down_leg_tail(ctx, l);
    return MG3D_OK;
}

/* down-leg of the top level behind a carried cycle: the one pre-smoothing pass that is left (black) + residual +
 * restriction (:1282 + :1294 + :1310) */
static int down_leg_carried(mg3d_ctx *ctx, int l)
{
    Level &lev = ctx->lv[l], &lc = ctx->lv[l - 1];
    {
        StageScope t(ctx, l, MG3D_ST_SMOOTH1);
        StageScope kt(ctx, l, MG3D_K_SWEEP1_RESTRICT, true);
        SweepLaunch w = mg3d_level_sweep(ctx, lev);
        w.kind = SWEEP_PASSES_RES;
        w.S = 1;
        w.c1 = 0;
        w.gc = &lc.g;
        w.dc = lc.f[MG3D_D];
        if (k_sweep(ctx->opt, w, ctx->stream) < 0)
            return fail(MG3D_ERR_STATE, "carried cycle: no kernel for one pass + residual + restriction");
        swap_u(lev);
    }
    down_leg_tail(ctx, l);
    return MG3D_OK;
}

/* level 1 in one workgroup: the whole bottom of the cycle (:1258 ... :1341 of levels 1, 0) or its down-leg
 * (:1258 + :1282 + :1294 + :1310) as one launch, which injects the faces itself */
static void down_leg_tiny(mg3d_ctx *ctx, const CycleState &c)
{
    Level &lev = ctx->lv[1], &l0 = ctx->lv[0];
    {
        StageScope t(ctx, 1, MG3D_ST_SMOOTH1);
        StageScope kt(ctx, 1, MG3D_K_SWEEP4, true);
        if (c.tiny_cyc)
            k_tiny_cycle(lev.g, lev.f[MG3D_U], lev.f[MG3D_D], lev.f[MG3D_R], l0.g, l0.f[MG3D_D], l0.f[MG3D_U], ctx->lu, ctx->lu_in,
                         mg3d_level_operator(ctx, 1).op, ctx->iters, ctx->stream);
        else
            k_tiny_down(lev.g, lev.f[MG3D_U], lev.f[MG3D_D], lev.f[MG3D_R], l0.g, l0.f[MG3D_D], mg3d_level_operator(ctx, 1).op,
                        ctx->iters, ctx->stream);
    }
    { StageScope t(ctx, 1, MG3D_ST_RESIDUAL1); } /* inside the launch above: counted, ~0 s */
    { StageScope t(ctx, 1, MG3D_ST_RESTRICT); }
    ctx->faces_dirty[1] = 0;
}

/* the down-leg of every other level: zero guess (keep_guess: the level's u as it is), pre-smoother, residual, restriction */
static int down_leg_ordinary(mg3d_ctx *ctx, int l, bool keep_guess)
{
    Level &lev = ctx->lv[l];
    /* :1258-1259: the zero initial guess of a coarser level; with the fused sweep the first launch simply
     * does not read u (and writes every plane of the other buffer), so no memset is needed */
    const bool zero = l < ctx->L - 1 && !keep_guess;
    const bool zero_in = zero && mg3d_fused(ctx) && ctx->iters > 0;
    if (zero && !zero_in)
        (void)hipMemsetAsync(lev.f[MG3D_U], 0, lev.elems * sizeof(double), ctx->stream);
    if (mg3d_fused(ctx)) { /* pre-smoother and residual in one pass over the level (:1282 + :1294) */
        {
            StageScope t(ctx, l, MG3D_ST_SMOOTH1);
            CHK(enqueue_smooth_residual(ctx, l, 0, ctx->iters, 2, ctx->sumsq_slots - 1,
                                        ctx->keep_r ? nullptr : &ctx->lv[l - 1], nullptr, zero_in, false));
        }
        StageScope t(ctx, l, MG3D_ST_RESIDUAL1); /* fused into the launch above: counted, ~0 s */
    } else {
        {
            StageScope t(ctx, l, MG3D_ST_SMOOTH1);
            CHK(enqueue_smooth(ctx, l, 0, ctx->iters)); /* :1282 */
        }
        StageScope t(ctx, l, MG3D_ST_RESIDUAL1);
        CHK(enqueue_residual(ctx, l, 1, ctx->sumsq_slots - 1)); /* :1294 (norm discarded) */
    }
    StageScope t(ctx, l, MG3D_ST_RESTRICT);
    /* :1310; when the interior was restricted on the fly only the face injection is left */
    restrict_stage(ctx, l, mg3d_fused(ctx) && !ctx->keep_r);
    return MG3D_OK;
}

/* level 0: the direct solve (:1270), unless the single-workgroup launch of level 1 held it */
static void bottom(mg3d_ctx *ctx, const CycleState &c)
{
    if (c.tiny_cyc) {
        StageScope t(ctx, 0, MG3D_ST_RECURSE); /* inside the launch above */
        return;
    }
    Level &l0 = ctx->lv[0];
    if (0 < ctx->L - 1)
        (void)hipMemsetAsync(l0.f[MG3D_U], 0, l0.elems * sizeof(double), ctx->stream);
    StageScope t(ctx, 0, MG3D_ST_RECURSE);
    StageScope kt(ctx, 0, MG3D_K_COARSE_SOLVE, true);
    enqueue_coarse_solve(ctx);
}

/* level 1 in one workgroup: prolongation + post-smoother as one launch (:1331 + :1341), or nothing left to do */
static void up_leg_tiny(mg3d_ctx *ctx, const CycleState &c)
{
    Level &lev = ctx->lv[1], &l0 = ctx->lv[0];
    { StageScope t(ctx, 1, MG3D_ST_PROLONG); } /* inside the launch below (tiny_cyc: the one on the way down) */
    {
        StageScope t(ctx, 1, MG3D_ST_SMOOTH2);
        if (!c.tiny_cyc) {
            StageScope kt(ctx, 1, MG3D_K_SWEEP4, true);
            k_tiny_up(lev.g, lev.f[MG3D_U], lev.f[MG3D_D], l0.g, l0.f[MG3D_U], mg3d_level_operator(ctx, 1).op, ctx->iters, ctx->stream);
        }
    }
    { StageScope t(ctx, 1, MG3D_ST_RESIDUAL2); }
}

/* up-leg of the top level as ONE launch: prolongation + black, red, black, red (:1331 + :1341); with another cycle behind it,
 * the red half of the norm (:1354) from the last pass's sums */
static int up_leg_legs(mg3d_ctx *ctx, const CycleState &c, int l)
{
    Level &lev = ctx->lv[l], &lc = ctx->lv[l - 1];
    { StageScope t(ctx, l, MG3D_ST_PROLONG); } /* :1331, folded into the launch below */
    {
        StageScope t(ctx, l, MG3D_ST_SMOOTH2);
        SweepLaunch w = mg3d_level_sweep(ctx, lev);
        w.kind = SWEEP_LEG_UP;
        w.gce = &lc.g;
        w.ec = lc.f[MG3D_U];
        w.partials = c.carry_out ? part_a(ctx) : nullptr;
        w.max_partials = MG3D_MAX_PARTIALS / 2;
        int npa;
        {
            StageScope kt(ctx, l, MG3D_K_LEG_UP, true);
            npa = k_sweep(ctx->opt, w, ctx->stream);
        }
        if (npa < 0)
            return fail(MG3D_ERR_STATE, "one launch per leg: no kernel for the up-leg");
        swap_u(lev);
        if (c.carry_out == 1) { /* the next cycle of this mg3d_vcycles call completes the norm */
            ctx->legs_state = 2;
            ctx->legs_slot = c.slot;
            ctx->legs_npa = npa;
        } else if (c.carry_out == 2) {
            /* mg3d_vcycle: the next cycle's down-leg now, into the alt buffers (see mg3d_can_legs) */
            CHK(launch_leg_down(ctx, l, lc.alt, true, npa, c.slot));
            ctx->legs_state = 3;
        }
    }
    StageScope t(ctx, l, MG3D_ST_RESIDUAL2);
    if (!c.carry_out)
        CHK(enqueue_residual(ctx, l, 0, c.slot)); /* :1354, the last cycle of a call: a launch of its own */
    return MG3D_OK;
}

/* up-leg of the top level of a cycle that carries into the next one */
static int up_leg_carried(mg3d_ctx *ctx, const CycleState &c, int l)
{
    Level &lev = ctx->lv[l];
    { StageScope t(ctx, l, MG3D_ST_PROLONG); } /* :1331, folded into the launch below */
    {
        StageScope t(ctx, l, MG3D_ST_SMOOTH2);
        /* prolongation + the first two post-smoothing passes: the launch the ordinary cycle starts its up-leg with */
        const StagePlan split = mg3d_stage_plan(ctx->opt, stage_ask(ctx, l, 1, 2, 1, false, true, true));
        CHK(enqueue_stage_step(ctx, l, 1, split.step[0], true, 0, c.slot, nullptr, &ctx->lv[l - 1], false, true));
        /* black, red (:1341, second half) <norm, :1354> black, red (:1282 of the next cycle, its first red pass
         * being the identity) */
        StageScope kt(ctx, l, MG3D_K_SWEEP4_NORM, true);
        SweepLaunch w = mg3d_level_sweep(ctx, lev);
        w.kind = SWEEP_TAP;
        w.c1 = 0;
        w.partials = ctx->partials;
        const int np = k_sweep(ctx->opt, w, ctx->stream);
        if (np < 0)
            return fail(MG3D_ERR_STATE, "carried cycle: no kernel for four passes + norm tap");
        swap_u(lev);
        k_fold(ctx->partials, np, ctx->sumsq + c.slot, ctx->stream);
        ctx->carried = true;
    }
    { StageScope t(ctx, l, MG3D_ST_RESIDUAL2); }
    return MG3D_OK;
}

/* the up-leg of every other level: prolongation, post-smoother and, on the top level, the residual norm */
static int up_leg_ordinary(mg3d_ctx *ctx, const CycleState &c, int l)
{
    const int want_norm = l == c.q ? 1 : 0;
    const bool pro = pro_fusable(ctx, ctx->iters, want_norm, l);
    {
        StageScope t(ctx, l, MG3D_ST_PROLONG); /* :1331; ~0 s when folded into the smoother's loads */
        if (!pro) {
            StageScope kt(ctx, l, MG3D_K_PROLONG, true);
            enqueue_prolong(ctx, l);
        }
    }
    if (mg3d_fused(ctx)) { /* (prolongation,) post-smoother and residual norm (:1331 + :1341 + :1354) */
        {
            StageScope t(ctx, l, MG3D_ST_SMOOTH2);
            /* the norm of a level below the top one is computed and dropped by the reference (:1320
             * ignores the recursive call's value): skip it, nothing observable changes */
            CHK(enqueue_smooth_residual(ctx, l, 1, ctx->iters, want_norm, c.slot, nullptr, pro ? &ctx->lv[l - 1] : nullptr));
        }
        StageScope t(ctx, l, MG3D_ST_RESIDUAL2); /* fused into the launch above: counted, ~0 s */
        return MG3D_OK;
    }
    {
        StageScope t(ctx, l, MG3D_ST_SMOOTH2);
        CHK(enqueue_smooth(ctx, l, 1, ctx->iters)); /* :1341 */
    }
    StageScope t(ctx, l, MG3D_ST_RESIDUAL2);
    if (l == c.q)
        CHK(enqueue_residual(ctx, l, 0, c.slot)); /* :1354; below the top level the value is dropped (:1320) */
    return MG3D_OK;
}

/* The caller's new d of the top level (dz_state, mg3d_ctx.h): one pass over it, once, and the map read back -- the launches
 * take it only when it holds a plane.  The one host synchronisation is paid per upload of d, not per cycle. */
static int dzero_scan(mg3d_ctx *ctx)
{
    const Level &top = ctx->lv[ctx->L - 1];
    std::vector<unsigned> words((size_t)mg3d_dzero_words(top.g.ni));
    k_dzero_scan(top.g, top.f[MG3D_D], ctx->dz_map, ctx->stream);
    CHK(mg3d_launch_ok("mg3d_vcycle: zero map of d"));
    HIPCHK(hipMemcpyAsync(words.data(), ctx->dz_map, words.size() * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->dz_planes = 0;
    for (unsigned w : words)
        ctx->dz_planes += __builtin_popcount(w);
    ctx->dz_state = MG3D_DZ_VALID;
    return MG3D_OK;
}

int mg3d_enqueue_vcycle(mg3d_ctx *ctx, int q, int slot, int carry_out, bool keep_guess)
{
    if (!ctx->have_lu)
        return fail(MG3D_ERR_STATE, "mg3d_vcycle: no coarse LU set (mg3d_ctx_build_coarse / mg3d_ctx_set_lu)");
    if (ctx->have_es)
        return fail(MG3D_ERR_STATE, "mg3d_vcycle: the context holds the mixed-boundary factor of mg3d_es_setup "
                                    "(mg3d_es_vcycles, or load the Dirichlet factor again)");
    const int L = ctx->L;
    struct PhaseTick { /* sampled kernel timers (timing >= 4): full cycles are counted off, also on an early return */
        mg3d_ctx *c;
        bool full;
        ~PhaseTick()
        {
            if (full && c->timing >= 4)
                c->timing_phase = (c->timing_phase + 1) % (c->timing - 2);
        }
    } tick{ctx, q == L - 1};
    /* ---- what this cycle is, and what the one before left behind */
    CycleState c;
    c.q = q;
    c.slot = slot;
    c.carry_out = carry_out;
    c.tiny = ctx->opt.v[MG3D_OPT_TINY] && mg3d_fused(ctx) && !ctx->keep_r && q >= 2 && ctx->iters >= 1 &&
             k_tiny_fits(ctx->lv[1].g, ctx->lv[0].g);
    c.tiny_cyc = c.tiny && ctx->opt.v[MG3D_OPT_TINY_CYCLE] && k_tiny_cycle_fits(ctx->lv[1].g, ctx->lv[0].g, ctx->lu, ctx->lu_in);
    c.can_legs = mg3d_can_legs(ctx, q);
    c.can_carry = !c.can_legs && mg3d_can_carry(ctx, q);
    if ((ctx->carried && !c.can_carry) || (ctx->legs_state != 0 && !c.can_legs)) /* e.g. MG3D_NO_CARRY set between two calls: finish the carried cycle, go on plainly */
        CHK(mg3d_drop_carry_keep(ctx));
    c.carry_in = ctx->carried;
    ctx->carried = false;
    c.legs_in = ctx->legs_state;
    ctx->legs_state = 0;
    c.red_in = q == L - 1 && c.legs_in == 0 && !c.carry_in && ctx->red_tail && c.can_legs && !ctx->raw_top;
    ctx->red_tail = false;
    if (q == L - 1 && ctx->dz_state == MG3D_DZ_UNKNOWN && ctx->opt.v[MG3D_OPT_D_ZERO_SKIP] && mg3d_fused(ctx))
        CHK(dzero_scan(ctx));
    /* ---- down: the top level continues what ran ahead of it, level 1 fits one workgroup, the rest is ordinary */
    for (int l = q; l >= 1; l--) {
        if (l == q && c.can_legs && (c.legs_in != 0 || c.red_in))
            CHK(down_leg_ahead(ctx, c, l));
        else if (l == q && c.carry_in)
            CHK(down_leg_carried(ctx, l));
        else if (l == 1 && c.tiny)
            down_leg_tiny(ctx, c);
        else
            CHK(down_leg_ordinary(ctx, l, keep_guess && l == q));
    }
    bottom(ctx, c);
    /* ---- up: level 1 as on the way down; the top level in the schedule that lets the next cycle run ahead */
    for (int l = 1; l <= q; l++) {
        if (l == 1 && c.tiny)
            up_leg_tiny(ctx, c);
        else if (l == q && c.can_legs)
            CHK(up_leg_legs(ctx, c, l));
        else if (l == q && carry_out && c.can_carry)
            CHK(up_leg_carried(ctx, c, l));
        else
            CHK(up_leg_ordinary(ctx, c, l));
    }
    /* a whole V(2,2) cycle from the top level has ended with its last red pass and nothing runs ahead: see red_in */
    if (q == L - 1 && ctx->legs_state == 0 && !ctx->carried && ctx->iters == 2 && mg3d_fused(ctx))
        ctx->red_tail = true;
    return mg3d_launch_ok("mg3d_vcycle");
}

extern "C" int mg3d_vcycle(mg3d_ctx *ctx, int level, double *norm)
{
    CHK(mg3d_check_field_level(ctx, 0, level, "mg3d_vcycle"));
    if (level == 0) { /* q == 0: direct solve, returns 0 (mg_3d.h:1262-1277) */
        CHK(mg3d_coarse_solve(ctx));
        if (norm)
            *norm = 0.;
        return MG3D_OK;
    }
    if (level != ctx->L - 1)
        CHK(mg3d_drop_carry(ctx)); /* (a cycle from a lower level rewrites the levels below the top one only -- but it ends whatever ran ahead) */
    /* One cycle per call is how the reference's solve loop runs (SolverLinSolve, mg_3d.h:1415-1420): the call ends with
     * the launch that also begins the NEXT cycle -- speculatively; whatever the caller does instead of another cycle
     * first puts the finished cycle's own u back (mg3d_drop_carry), and the norm returned is this cycle's either way.
     * Not once a raw pointer to u or d of the top level is out (mg3d_ctx_touched). */
    const int rc = mg3d_enqueue_vcycle(ctx, level, 0, ctx->raw_top ? 0 : 2);
    if (rc != MG3D_OK) {
        (void)mg3d_drop_carry(ctx); /* the first error is the one reported */
        return rc;
    }
    return read_norm(ctx, 0, norm);
}

extern "C" int mg3d_vcycles(mg3d_ctx *ctx, int count, double *norms)
{
    if (!ctx || count < 0)
        return fail(MG3D_ERR_ARG, "mg3d_vcycles: bad arguments");
    const int q = ctx->L - 1;
    if (q == 0) {
        for (int c = 0; c < count; c++) {
            CHK(mg3d_coarse_solve(ctx));
            if (norms)
                norms[c] = 0.;
        }
        return mg3d_sync(ctx);
    }
    const int batch = ctx->sumsq_slots - 1;
    if (count == 0) /* (behind a single mg3d_vcycle call the first cycle continues from the carried state) */
        CHK(mg3d_drop_carry_keep(ctx));
    struct Guard { /* an error return must not leave u of the top level a few passes into a cycle nobody asked for */
        mg3d_ctx *c;
        ~Guard() { (void)mg3d_drop_carry_keep(c); }
    } guard{ctx};
    for (int done = 0; done < count;) {
        const int nb = (count - done < batch) ? count - done : batch;
        for (int c = 0; c < nb; c++)
            /* every cycle but the last carries into the next; one launch per leg: not across a batch's norm read-back */
            CHK(mg3d_enqueue_vcycle(ctx, q, c, (done + c + 1 < count && (c + 1 < nb || !mg3d_can_legs(ctx, q))) ? 1 : 0));
        HIPCHK(hipMemcpyAsync(ctx->h_sumsq, ctx->sumsq, nb * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        resolve_timers(ctx);
        if (norms)
            for (int c = 0; c < nb; c++)
                norms[done + c] = sqrt(ctx->h_sumsq[c]);
        done += nb;
    }
    return MG3D_OK;
}

/* -------------------------------------------------------------------- FMG */
extern "C" int mg3d_fill_boundary(mg3d_ctx *ctx, int field, int level)
{
    CHK(mg3d_drop_carry(ctx));
    CHK(mg3d_check_field_level(ctx, field, level, "mg3d_fill_boundary"));
    if (ctx->periodic) /* BCFunc is defined on all six faces */
        return fail(MG3D_ERR_STATE, "mg3d_fill_boundary: the context has periodic axes (mg3d_ctx_set_periodic); set them to 0");
    if (ctx->neumann)
        return fail(MG3D_ERR_STATE, "mg3d_fill_boundary: the context has Neumann faces (mg3d_ctx_set_neumann); set them to 0");
    k_fill_boundary(ctx->lv[level].g, ctx->lv[level].f[field], ctx->lv[level].h, ctx->stream);
    mg3d_ctx_touched(ctx, field, level, false, MG3D_WROTE_FACES);
    return mg3d_launch_ok("mg3d_fill_boundary");
}

/* SolverFMGInitialize, mg_dirichlet_analytic.c:771-806 */
extern "C" int mg3d_fmg_initialize(mg3d_ctx *ctx)
{
    CHK(mg3d_drop_carry(ctx));
    if (!ctx)
        return fail(MG3D_ERR_ARG, "mg3d_fmg_initialize: NULL context");
    if (ctx->periodic) /* the F-cycle start fills BCFunc into all six faces */
        return fail(MG3D_ERR_STATE, "mg3d_fmg_initialize: the context has periodic axes (mg3d_ctx_set_periodic); set them to 0");
    if (ctx->neumann)
        return fail(MG3D_ERR_STATE, "mg3d_fmg_initialize: the context has Neumann faces (mg3d_ctx_set_neumann); set them to 0");
    if (ctx->mask.set())
        return fail(MG3D_ERR_STATE, "mg3d_fmg_initialize: the context has fixed points (mg3d_ctx_set_mask); set the mask to NULL");
    if (ctx->sfield.set()) /* the F-cycle start is the reference's, whose operator has no field */
        return fail(MG3D_ERR_STATE, "mg3d_fmg_initialize: the context has a screening field (mg3d_ctx_set_shift_field); set it to NULL");
    if (!ctx->have_lu)
        return fail(MG3D_ERR_STATE, "mg3d_fmg_initialize: no coarse LU set");
    if (ctx->have_es)
        return fail(MG3D_ERR_STATE, "mg3d_fmg_initialize: the context holds the mixed-boundary factor of mg3d_es_setup");
    hipStream_t s = ctx->stream;
    k_fill_boundary(ctx->lv[0].g, ctx->lv[0].f[MG3D_U], ctx->lv[0].h, s);                                  /* :780 */
    k_lu_solve(ctx->lu, ctx->lu_in, ctx->lv[0].g, ctx->lv[0].f[MG3D_D], ctx->lv[0].f[MG3D_U], ctx->lu_work, s);         /* :783 */
    for (int l = 1; l < ctx->L; l++) {
        Level &lev = ctx->lv[l], &lc = ctx->lv[l - 1];
        k_prolong(lc.g, lc.f[MG3D_U], lev.g, lev.f[MG3D_U], 0, s);                                           /* :795 */
        k_fill_boundary(lev.g, lev.f[MG3D_U], lev.h, s);                                                     /* :798 */
        (void)hipMemsetAsync(lc.f[MG3D_U], 0, lc.elems * sizeof(double), s);                                 /* :801 */
        CHK(mg3d_enqueue_vcycle(ctx, l, ctx->sumsq_slots - 1));                                              /* :804 */
    }
    return mg3d_launch_ok("mg3d_fmg_initialize");
}

/* Full multigrid for the caller's problem (include/mg3d.h): what mg3d_fmg_initialize cannot be while it is pinned to the
 * reference -- the caller's d and Dirichlet values, every operator of the context, a cubic interpolation, and V-cycles
 * that keep the interpolated guess (keep_guess of mg3d_enqueue_vcycle). */
static int fmg_check(mg3d_ctx *ctx, const char *who)
{
    /* (under injection a thin body is absent from the levels full multigrid starts on) */
    if (ctx->mask.set() && ctx->mask_rule == MG3D_MASK_INJECT)
        return fail(MG3D_ERR_STATE,
                    "%s: the context has fixed points coarsened by injection (mg3d_ctx_set_mask); call "
                    "mg3d_ctx_set_mask_coarsening(MG3D_MASK_KEEP), or set the mask to NULL",
                    who);
    if (!ctx->have_lu)
        return fail(MG3D_ERR_STATE, "%s: no coarse LU set (mg3d_ctx_build_coarse / mg3d_ctx_set_lu)", who);
    if (ctx->have_es)
        return fail(MG3D_ERR_STATE, "%s: the context holds the mixed-boundary factor of mg3d_es_setup", who);
    return MG3D_OK;
}

extern "C" int mg3d_fmg_interpolate(mg3d_ctx *ctx, int level)
{
    if (!ctx || level < 1 || level >= ctx->L)
        return fail(MG3D_ERR_ARG, "mg3d_fmg_interpolate: %s", ctx ? "level outside 1 .. L-1" : "NULL context");
    CHK(fmg_check(ctx, "mg3d_fmg_interpolate"));
    CHK(mg3d_drop_carry(ctx));
    const Level &lev = ctx->lv[level], &lc = ctx->lv[level - 1];
    k_fmg_interp(lc.g, lc.f[MG3D_U], lev.g, lev.f[MG3D_U], mg3d_ctx_bc(ctx), ctx->stream, ctx->mask.at(level));
    return mg3d_launch_ok("mg3d_fmg_interpolate");
}

extern "C" int mg3d_fmg_solve(mg3d_ctx *ctx, int cycles, double *norm)
{
    if (!ctx || cycles < 1)
        return fail(MG3D_ERR_ARG, "mg3d_fmg_solve: %s", ctx ? "cycles must be >= 1" : "NULL context");
    CHK(fmg_check(ctx, "mg3d_fmg_solve"));
    CHK(mg3d_drop_carry(ctx));
    const int L = ctx->L, bc = mg3d_ctx_bc(ctx);
    hipStream_t s = ctx->stream;
    /* 1. the right-hand side down the hierarchy by the context's own restriction, u by injection: the Dirichlet values.
     * With fixed points (MG3D_MASK_KEEP): d counts as 0. at the fixed unknowns, where it is never read, and a coarse fixed
     * point that stands for a lost fine one takes that one's u, so every level's body carries its conductor's potential */
    for (int l = L - 1; l >= 1; l--) {
        const Level &lev = ctx->lv[l], &lc = ctx->lv[l - 1];
        const unsigned char *mf = ctx->mask.at(l);
        k_restrict(lev.g, lev.f[MG3D_D], lc.g, lc.f[MG3D_D], bc, s, -1, -1, false, mf);
        if (mf)
            k_fmg_inject(lev.g, lev.f[MG3D_U], mf, lc.g, lc.f[MG3D_U], bc, s);
        else
            k_coef_inject(lev.g, lev.f[MG3D_U], lc.g, lc.f[MG3D_U], s);
        mg3d_ctx_touched(ctx, MG3D_D, l - 1); /* its faces are no injection of r any more: the cycles inject them again */
    }
    /* 2. the direct solve, its identity rows taking the Dirichlet values, those of the fixed unknowns included (a one-level
     * context keeps its d: the right-hand side is put together in r) */
    Level &l0 = ctx->lv[0];
    double *rhs = l0.f[MG3D_D];
    if (L == 1) {
        rhs = l0.f[MG3D_R];
        HIPCHK(hipMemcpyAsync(rhs, l0.f[MG3D_D], l0.elems * sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    k_dirichlet_rhs(l0.g, l0.f[MG3D_U], rhs, bc, s);
    enqueue_coarse_solve(ctx, rhs, true);
    CHK(mg3d_launch_ok("mg3d_fmg_solve"));
    if (L == 1) {
        if (norm)
            *norm = 0.;
        return mg3d_sync(ctx);
    }
    /* 3. up: the cubic interpolant as the guess, `cycles` V-cycles that keep it; d of level l and the Dirichlet points of
     * u of level l are still those of step 1 -- a cycle from below writes d below l and u at or below l - 1 only */
    for (int l = 1; l < L - 1; l++) {
        k_fmg_interp(ctx->lv[l - 1].g, ctx->lv[l - 1].f[MG3D_U], ctx->lv[l].g, ctx->lv[l].f[MG3D_U], bc, s, ctx->mask.at(l));
        for (int c = 0; c < cycles; c++)
            CHK(mg3d_enqueue_vcycle(ctx, l, ctx->sumsq_slots - 1, 0, true));
    }
    k_fmg_interp(ctx->lv[L - 2].g, ctx->lv[L - 2].f[MG3D_U], ctx->lv[L - 1].g, ctx->lv[L - 1].f[MG3D_U], bc, s,
                 ctx->mask.at(L - 1));
    CHK(mg3d_launch_ok("mg3d_fmg_solve"));
    std::vector<double> norms((size_t)cycles);
    CHK(mg3d_vcycles(ctx, cycles, norms.data())); /* the finest level: its schedules, its guard */
    if (norm)
        *norm = norms.back();
    return MG3D_OK;
}

/* ------------------------------------------------------------------- timing */
extern "C" int mg3d_timing_enable(mg3d_ctx *ctx, int on)
{
    if (!ctx)
        return fail(MG3D_ERR_ARG, "mg3d_timing_enable: NULL context");
    ctx->timing = (on >= 1 && on <= 64) ? on : 0;
    ctx->timing_phase = 0;
    return MG3D_OK;
}

extern "C" int mg3d_timing_reset(mg3d_ctx *ctx) /* resetTimingInfo, timing_info.h:34-38 */
{
    if (!ctx)
        return fail(MG3D_ERR_ARG, "mg3d_timing_reset: NULL context");
    if (!ctx->pending.empty()) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        resolve_timers(ctx);
    }
    for (auto &t : ctx->timers)
        t = StageTimer{0, 0.};
    return MG3D_OK;
}

extern "C" int mg3d_kernel_time_get(mg3d_ctx *ctx, int level, int kernel, int *num_launches, double *seconds)
{
    if (!ctx || level < 0 || level >= ctx->L || kernel < 0 || kernel >= MG3D_NUM_KERNELS)
        return fail(MG3D_ERR_ARG, "mg3d_kernel_time_get: bad level/kernel");
    if (!ctx->pending.empty()) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        resolve_timers(ctx);
    }
    const StageTimer &t = ctx->timers[(size_t)ctx->L * MG3D_NUM_STAGES + (size_t)level * MG3D_NUM_KERNELS + kernel];
    if (num_launches)
        *num_launches = t.calls;
    if (seconds)
        *seconds = t.seconds;
    return MG3D_OK;
}

extern "C" int mg3d_timing_get(mg3d_ctx *ctx, int level, int stage, int *num_calls, double *seconds)
{
    if (!ctx || level < 0 || level >= ctx->L || stage < 0 || stage >= MG3D_NUM_STAGES)
        return fail(MG3D_ERR_ARG, "mg3d_timing_get: bad level/stage");
    if (!ctx->pending.empty()) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        resolve_timers(ctx);
    }
    const StageTimer &t = ctx->timers[(size_t)level * MG3D_NUM_STAGES + stage];
    if (num_calls)
        *num_calls = t.calls;
    if (seconds)
        *seconds = t.seconds;
    return MG3D_OK;
}

/* page-locked host arrays for the facade's finest u and d (mg_3d.h:275-293 hands their addresses to the caller,
 * and they cross PCIe around every solve: pageable memory downloads at 15 GB/s, page-locked at PCIe rate) */
extern "C" int mg3d_host_alloc(size_t bytes, void **out)
{
    if (!out || bytes == 0)
        return fail(MG3D_ERR_ARG, "mg3d_host_alloc: bad arguments");
    if (mg3d_device_count() <= 0)
        return fail(MG3D_ERR_NO_DEVICE, "no HIP device available: libmg3d has no CPU fallback");
    void *p = nullptr;
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    if (e != hipSuccess)
        return fail(MG3D_ERR_ALLOC, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    memset(p, 0, bytes);
    *out = p;
    return MG3D_OK;
}

extern "C" int mg3d_host_free(void *p)
{
    if (p && hipHostFree(p) != hipSuccess)
        return fail(MG3D_ERR_HIP, "hipHostFree failed");
    return MG3D_OK;
}

/* ----------------------------------------------- host-pointer operator forms */
struct ScratchCtx { /* a one- or two-level context for a single host-pointer call */
    mg3d_ctx *ctx = nullptr;
    ~ScratchCtx() { mg3d_ctx_destroy(ctx); }
};

static int scratch_create(const int *n, const double *h, int L, ScratchCtx &sc)
{
    CHK(ctx_create_sizes(n, h, L, 0, &sc.ctx));
    sc.ctx->c = n[0];
    sc.ctx->length = 0.;
    return MG3D_OK;
}

extern "C" int mg3d_host_smooth(double *v, const double *d, int N, double h, int iters, int post)
{
    if (!v || !d || N < 1 || iters < 0)
        return fail(MG3D_ERR_ARG, "mg3d_host_smooth: bad arguments");
    ScratchCtx sc;
    CHK(scratch_create(&N, &h, 1, sc));
    CHK(mg3d_upload(sc.ctx, MG3D_U, 0, v));
    CHK(mg3d_upload(sc.ctx, MG3D_D, 0, d));
    CHK(mg3d_smooth(sc.ctx, 0, post, iters));
    return mg3d_download(sc.ctx, MG3D_U, 0, v);
}

extern "C" int mg3d_host_residual(const double *v, const double *d, int N, double h, double *res, double *norm)
{
    if (!v || !d || N < 1)
        return fail(MG3D_ERR_ARG, "mg3d_host_residual: bad arguments");
    ScratchCtx sc;
    CHK(scratch_create(&N, &h, 1, sc));
    CHK(mg3d_upload(sc.ctx, MG3D_U, 0, v));
    CHK(mg3d_upload(sc.ctx, MG3D_D, 0, d));
    if (res) /* only the interior of res is written (mg_3d.h:824-825): keep the caller's boundary values */
        CHK(mg3d_upload(sc.ctx, MG3D_R, 0, res));
    CHK(mg3d_residual(sc.ctx, 0, res != nullptr, norm));
    if (res)
        CHK(mg3d_download(sc.ctx, MG3D_R, 0, res));
    return MG3D_OK;
}

extern "C" int mg3d_host_restrict(const double *r, int Nf, double *dc, int Nc)
{
    if (!r || !dc || Nc < 1 || Nf != 2 * Nc - 1)
        return fail(MG3D_ERR_ARG, "mg3d_host_restrict: need Nf == 2*Nc-1 (got %d, %d)", Nf, Nc);
    const int n[2] = {Nc, Nf};
    const double h[2] = {2., 1.};
    ScratchCtx sc;
    CHK(scratch_create(n, h, 2, sc));
    CHK(mg3d_upload(sc.ctx, MG3D_R, 1, r));
    CHK(mg3d_restrict(sc.ctx, 1));
    return mg3d_download(sc.ctx, MG3D_D, 0, dc);
}

extern "C" int mg3d_host_prolong(const double *ec, int Nc, double *ef, int Nf)
{
    if (!ec || !ef || Nc < 1 || Nf != 2 * Nc - 1)
        return fail(MG3D_ERR_ARG, "mg3d_host_prolong: need Nf == 2*Nc-1 (got %d, %d)", Nf, Nc);
    const int n[2] = {Nc, Nf};
    const double h[2] = {2., 1.};
    ScratchCtx sc;
    CHK(scratch_create(n, h, 2, sc));
    CHK(mg3d_upload(sc.ctx, MG3D_U, 0, ec));
    CHK(mg3d_upload(sc.ctx, MG3D_U, 1, ef));
    CHK(mg3d_prolong(sc.ctx, 1));
    return mg3d_download(sc.ctx, MG3D_U, 1, ef);
}

extern "C" int mg3d_host_lu_solve(const double *LU, int n, const double *b, double *x)
{
    if (!LU || !b || !x || n < 1)
        return fail(MG3D_ERR_ARG, "mg3d_host_lu_solve: bad arguments");
    /* treat the n-vector as an n x 1 x 1 "grid" so the padded-layout solve kernel applies */
    CHK(require_device());
    ScratchCtx sc;
    mg3d_ctx *ctx = sc.ctx = ctx_new(1, 0);
    HIPCHK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    CHK(install_lu(ctx, LU, n, 4 * (size_t)n));
    double *db = ctx->lu_work + 2 * (size_t)n, *dx = db + n;
    HIPCHK(hipMemcpy(db, b, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    Geom g;
    g.N = g.ni = n;
    g.nj = g.nk = 1;
    g.pitch = 1;
    g.plane = 1;
    g.ig0 = 0;
    k_lu_solve(ctx->lu, ctx->lu_in, g, db, dx, ctx->lu_work, ctx->stream);
    CHK(mg3d_launch_ok("mg3d_host_lu_solve"));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(x, dx, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return MG3D_OK;
}

extern "C" int mg3d_host_vcycle(double **u, double **f, double **res, double h, int q, int num_levels, int iters,
                                int N, const double *LU, double *norm, int *stage_calls, double *stage_seconds)
{
    if (!u || !f || !res || !LU || q < 0 || q >= num_levels || N < 3 || iters < 0)
        return fail(MG3D_ERR_ARG, "mg3d_host_vcycle: bad arguments");
    /* level sizes below q: N_coarse = (N+1)/2 (mg_3d.h:1302), h_coarse = 2h (mg_3d.h:1303) */
    std::vector<int> n(q + 1);
    std::vector<double> hh(q + 1);
    n[q] = N;
    hh[q] = h;
    for (int l = q - 1; l >= 0; l--) {
        if (n[l + 1] < 3 || (n[l + 1] & 1) == 0)
            return fail(MG3D_ERR_ARG, "mg3d_host_vcycle: level %d has %d points per side, cannot coarsen", l + 1,
                        n[l + 1]);
        n[l] = (n[l + 1] + 1) / 2;
        hh[l] = 2 * hh[l + 1];
    }
    ScratchCtx sc;
    CHK(scratch_create(n.data(), hh.data(), q + 1, sc));
    mg3d_ctx *ctx = sc.ctx;
    /* the memset of mg_3d.h:1258 is skipped only on the caller's finest level (q == numLevels-1):
     * emulate by telling the context how many levels the caller's hierarchy has */
    ctx->iters = iters;
    ctx->keep_r = true; /* the caller owns res[] and may read it */
    ctx->timing = (stage_calls || stage_seconds) ? 1 : 0;
    CHK(mg3d_ctx_set_lu(ctx, LU));
    CHK(mg3d_upload(ctx, MG3D_U, q, u[q]));
    CHK(mg3d_upload(ctx, MG3D_D, q, f[q]));
    /* r is written on interiors only: start from the caller's arrays so untouched entries survive */
    for (int l = 1; l <= q; l++)
        CHK(mg3d_upload(ctx, MG3D_R, l, res[l]));
    if (q == 0) {
        {
            StageScope t(ctx, 0, MG3D_ST_RECURSE);
            CHK(mg3d_coarse_solve(ctx));
        }
        if (norm)
            *norm = 0.;
        CHK(mg3d_download(ctx, MG3D_U, 0, u[0]));
        if (stage_calls)
            stage_calls[MG3D_ST_RECURSE] += ctx->timers[MG3D_ST_RECURSE].calls;
        if (stage_seconds)
            stage_seconds[MG3D_ST_RECURSE] += ctx->timers[MG3D_ST_RECURSE].seconds;
        return MG3D_OK;
    }
    if (q < num_levels - 1) /* not the caller's finest level: its guess is zeroed first (:1258) */
        CHK(mg3d_zero(ctx, MG3D_U, q));
    CHK(mg3d_enqueue_vcycle(ctx, q, 0));
    double nrm = 0.;
    CHK(read_norm(ctx, 0, &nrm)); /* synchronises and resolves the stage timers */
    if (norm)
        *norm = nrm;
    for (size_t t = 0; t < (size_t)ctx->L * MG3D_NUM_STAGES; t++) {
        if (stage_calls)
            stage_calls[t] += ctx->timers[t].calls;
        if (stage_seconds)
            stage_seconds[t] += ctx->timers[t].seconds;
    }
    for (int l = 0; l <= q; l++) {
        CHK(mg3d_download(ctx, MG3D_U, l, u[l]));
        if (l < q)
            CHK(mg3d_download(ctx, MG3D_D, l, f[l]));
        if (l >= 1)
            CHK(mg3d_download(ctx, MG3D_R, l, res[l]));
    }
    return MG3D_OK;
}
