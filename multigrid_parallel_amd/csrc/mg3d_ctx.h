/* mg3d_ctx.h -- solver context internals shared by mg3d_ctx.hip, mg3d_operator.hip and the other files that work on a
 * context (not installed). */
#ifndef MG3D_CTX_H
#define MG3D_CTX_H

#include <vector>

#include "mg3d_internal.h"

enum { MG3D_DZ_NONE = 0, MG3D_DZ_UNKNOWN, MG3D_DZ_VALID }; /* mg3d_ctx::dz_state */

struct Level {
    Geom g;
    double h;
    size_t elems; /* doubles allocated per field */
    double *f[3]; /* u, d, r */
    double *alt;  /* second copy of u: the fused sweep writes out of place, then the two are swapped */
};

struct StageTimer {
    int calls;
    double seconds;
};

/* One per-level field of the operator (mg3d_operator.hip): eps, the fixed-point bytes, the screening field.  lv: one device
 * array per level in the padded layout of the level's doubles (empty: the context has no such field); host0: level 0's,
 * dense, for the coarse matrix; count: unknowns of level 0 ([0]) and of the finest level ([1]) that the field singles out
 * under the present boundary masks -- what is counted is the field's own business, mg3d_ctx says it for each */
template <class T> struct OperatorField {
    std::vector<T *> lv;
    std::vector<T> host0;
    unsigned long long count[2] = {0, 0};
    bool set() const { return !lv.empty(); }
    T *at(int level) const { return lv.empty() ? nullptr : lv[level]; }
};
/* frees the levels and forgets the host copy and the counts (every way a field leaves a context, mg3d_ctx_destroy too;
 * nothing in flight may read it any more) */
template <class T> static inline void mg3d_field_free(OperatorField<T> &f)
{
    for (T *p : f.lv)
        (void)hipFree(p);
    f = OperatorField<T>();
}

struct mg3d_ctx {
    int c, L, iters;
    double length;
    std::vector<Level> lv;
    hipStream_t stream;
    bool own_stream; /* false when a distributed driver shares one stream between contexts */
    LuBand lu;
    LuBand lu_in; /* the factor without its identity rows (n == 0: not built), see install_lu */
    bool have_lu;
    /* the screened operator Delta_h u - sigma u (mg3d_ctx_set_shift; 0: the reference's Poisson operator) and where the
     * factor came from: lu_built -- mg3d_ctx_build_coarse(lu_h), rebuilt for a new sigma; else mg3d_ctx_set_lu, dropped */
    double sigma;
    bool lu_built;
    double lu_h;
    /* the variable coefficient of div(eps grad u) - sigma u (mg3d_ctx_set_coefficient): eps of every level in the padded
     * layout (not set: the constant-coefficient operator) and level 0's, dense, for the coarse matrix; no counts */
    OperatorField<double> eps;
    /* fixed points (mg3d_ctx_set_mask): one byte per point of every level in the padded layout, the finest level's as given
     * and the others' by the context's coarsening rule (mask_rule below; not set: no mask); level 0's, dense, for the coarse matrix; and how many fixed UNKNOWNS
     * level 0 and the finest level have under the present boundary masks (recounted when those change) */
    OperatorField<unsigned char> mask;
    /* how the levels below the finest take the mask (mg3d_ctx_set_mask_coarsening): MG3D_MASK_INJECT as above, or
     * MG3D_MASK_KEEP, under which a fixed fine point that injection loses fixes its lower parent.  Operator state: kept while
     * there is no mask, for the next one */
    int mask_rule = MG3D_MASK_INJECT;
    /* the screening field of div(eps grad u) - (sigma + s) u (mg3d_ctx_set_shift_field): s of every level in the padded
     * layout, the finest level's as given and each coarser one's by the context's own restriction (not set: no field); level
     * 0's, dense, for the coarse matrix; how many UNKNOWNS of level 0 and of the finest level have s > 0 under the present
     * boundary masks (retaken, with the coarser levels, when those change) */
    OperatorField<double> sfield;
    /* while the context has a field and no eps, eps = 1 at every point of every level for the eps kernels, which alone
     * have the field form (not set otherwise; the context still has no coefficient: mg3d_ctx_has_coefficient); neither a
     * host copy nor counts */
    OperatorField<double> ones;
    /* periodic axes (mg3d_ctx_set_periodic; MG3D_PERIODIC_* mask, 0: Dirichlet faces everywhere) and the padded level-0
     * right-hand side of the direct solve that k_per_coarse_rhs builds from d (allocated with the first nonzero mask) */
    int periodic;
    double *per_b;
    /* Neumann faces (mg3d_ctx_set_neumann; MG3D_NEUMANN_* mask, no bit on a periodic axis; 0: none).  The kernels take
     * both masks as one boundary word (mg3d_ctx_bc) */
    int neumann;
    double *lu_work;  /* 2n doubles */
    double *partials; /* MG3D_MAX_PARTIALS doubles */
    double *sumsq;    /* device slots for squared norms */
    int sumsq_slots;
    double *h_sumsq;  /* pinned mirror */
    bool keep_r; /* materialise r on every level (reference-visible array) instead of restricting it on the fly */
    /* The faces of a coarse right-hand side are an injection of the fine residual's faces (mg_3d.h:879-958), and
     * calculateResidual never writes those (:824-825): they only change when somebody outside the cycle writes r of
     * level l or d of level l-1.  faces_dirty[l] says the injection l -> l-1 has to be redone (set at creation, by
     * upload / zero of those fields); faces_always[l] after a raw device pointer to one of them was handed out. */
    std::vector<char> faces_dirty, faces_always;
    /* the mixed-boundary problem of csrc/mg3d_es.hip, after mg3d_es_setup */
    bool have_es;
    mg3d_es_params es;
    /* carried cycles (mg3d_vcycles, see mg3d_enqueue_vcycle): u of the top level already holds the first three
     * pre-smoothing passes of the NEXT cycle; the finished cycle's own result is in the level's alt buffer */
    bool carried;
    /* one launch per leg on the top level (mg3d_enqueue_vcycle, "two launches per level"): 0 nothing outstanding;
     * 2 (inside mg3d_vcycles) the finished cycle's u is final, the second half of its norm rides on the next cycle's
     * down-leg (legs_slot, legs_npa: where it goes, how many partial sums the up-leg left); 3 (behind mg3d_vcycle) the
     * NEXT cycle's down-leg has already run, speculatively: u of the top level is three passes into it and the coarser
     * level's next right-hand side sits in that level's alt buffer; the finished cycle's own u is in the top level's alt */
    int legs_state, legs_slot, legs_npa;
    /* the last thing that happened to u of the top level is the red pass that ends a V(2,2) cycle and neither u nor d has been
     * touched since (mg3d_drop_carry clears it: every entry point that reads or writes level data calls that first): the next
     * cycle's first red pass is the identity also ACROSS calls, its down-leg can be the one launch (mg3d_enqueue_vcycle) */
    bool red_tail = false;
    /* mg3d_pcg_solve (mg3d_pcg.hip): four work vectors of the finest level in its padded layout -- z, r, p, q -- allocated
     * on first use, freed with the context.  During a solve the first two stand in for the level's u and d */
    double *pcg_v[4] = {nullptr, nullptr, nullptr, nullptr};
    /* the time stepper (mg3d_step.hip): dt, theta, kappa of mg3d_step_setup and the shift it set -- a context whose sigma
     * is no longer that one refuses to advance; the source of the finest level in its padded layout, allocated on first
     * use and kept (step_has_src says whether it is in use), freed with the context */
    bool step_set = false;
    double step_dt = 0., step_theta = 0., step_kappa = 0., step_sigma = 0.;
    double *step_src = nullptr;
    bool step_has_src = false;
    /* the nonlinear term (mg3d_nl.hip): kind, g0, beta, uref of mg3d_nl_setup; the weight g of the finest level in its
     * padded layout (nl_has_g: in use); the solve's own fields of that level -- nl_v[0] the iterate x, [1] the trial t,
     * [2] the caller's d --, all allocated on first use, kept and freed with the context.  sfield_nl: the screening field the
     * context has was left by mg3d_nl_solve (the next solve overwrites it; the public field setters clear the flag) */
    bool nl_set = false;
    int nl_kind = 0;
    double nl_g0 = 0., nl_beta = 0., nl_uref = 0.;
    double *nl_g = nullptr;
    bool nl_has_g = false;
    double *nl_v[3] = {nullptr, nullptr, nullptr};
    bool sfield_nl = false;
    /* device arrays (mg3d_*_device): the device that was current when the context was created -- a caller's array must
     * live there --, the two events of the stream join (io_ev[0] recorded on the caller's stream, io_ev[1] on the
     * context's; created on first use, freed with the context) and the two 64-bit results of k_coef_check on the device */
    int device = 0;
    hipEvent_t io_ev[2] = {nullptr, nullptr};
    unsigned long long *io_chk = nullptr;
    /* mg3d_deposit(_device) (mg3d_particle.hip): the integer accumulator, one long long per element of the finest level's
     * layout, and the word that takes max |q|; allocated on the first deposit, freed with the context */
    long long *dep_acc = nullptr;
    unsigned long long *dep_max = nullptr;
    /* mg3d_particle_push(_device): the MG3D_FATE_SLOTS cumulative 64-bit counters of the fates, on the device; allocated and
     * zeroed with the first push, freed with the context */
    unsigned long long *push_table = nullptr;
    /* mg3d_particle_sort(_device): one allocation for sort_cap particles -- two key and two index buffers of sort_cap words,
     * the digit table and the row sums (mg3d_particle.hip: sort_bytes) --; made on first use, grown when count grows, freed
     * with the context */
    unsigned *sort_buf = nullptr;
    long long sort_cap = 0;
    bool raw_top; /* a raw device pointer to u or d of the top level was handed out (mg3d_device_view) */
    /* The zero map of d of the top level (k_dzero_scan: bit i = plane i is +0.0 at every interior point), which the fused
     * sweep launches of that level take so as not to read those planes (mg3d_level_sweep).  Every writer of that d says
     * what it did through mg3d_ctx_touched; dz_state is what is known since:
     *   MG3D_DZ_NONE    nothing, and nothing will be found out: a kernel of the library wrote d (the time stepper, the inner
     *                   solves of the CG drivers, the slab path) -- no launch takes the map
     *   MG3D_DZ_UNKNOWN the caller gave a new d (mg3d_upload, mg3d_upload_device): the next cycle from the top level of a fused
     *                   context scans it, once
     *   MG3D_DZ_VALID   the map is d's; dz_planes bits are set (0: no launch takes it)
     * dz_raw: a raw pointer to that d is out (mg3d_device_view) -- MG3D_DZ_NONE for good, as raw_top */
    unsigned *dz_map = nullptr; /* device, mg3d_dzero_words(ni) words, allocated with the context */
    int dz_state = MG3D_DZ_UNKNOWN, dz_planes = 0; /* (created zeroed: the first cycle's scan finds that out) */
    bool dz_raw = false;
    /* launches that took a kernel without d because the map was full (SweepLaunch::d_none; mg3d_ctx_dnone_launches).
     * Counted where the launch is described, through the const context of mg3d_level_sweep */
    mutable unsigned long long dnone_launches = 0;
    /* what the sweep launches of this context were: kernel, chunk length, grid (SweepLaunch::taken; mg3d_ctx_sweep_taken),
     * written by k_sweep on the host through the const context of mg3d_level_sweep */
    mutable SweepTakenLog sweep_taken = {};
    mg3d_options opt; /* launch / schedule policy (mg3d_options_init at creation, mg3d_ctx_set_option afterwards) */
    bool fused; /* fused sweep kernel (default) or one launch per colour pass (MG3D_NO_FUSE=1) */
    int timing; /* 0 off, 1 every level, 2 finest level only, 3 finest level's kernel timers only, 4 + k: 3 on every (k+2)-th cycle */
    int timing_phase; /* cycles since the last sampled one (timing >= 4) */
    std::vector<StageTimer> timers; /* [L][MG3D_NUM_STAGES] */
    /* stage timing never stalls the stream: event pairs are recorded in-stream and
     * resolved at the next host synchronisation the entry point does anyway */
    struct Pending {
        int slot; /* index into timers: stage timers first ([level][stage]), then kernel timers */
        hipEvent_t a, b;
    };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> event_pool;
};

/* the fused sweep writes out of place: u and its second copy change roles behind every launch with colour passes */
static inline void swap_u(Level &l)
{
    double *t = l.f[MG3D_U];
    l.f[MG3D_U] = l.alt;
    l.alt = t;
}
/* the fused schedules (sweep, tiny, carried cycles, legs) apply: not with a variable coefficient, whose levels run colour
 * passes and residual of k_smooth_color / k_residual with the plain restriction, prolongation and coarse solve between
 * them, nor with a periodic axis or a Neumann face, whose levels run those with wrapped or reflected neighbours and the
 * transfers k_restrict / k_prolong launch for a boundary word, nor with fixed points, whose levels run the MASK forms, nor
 * with a screening field, whose levels run the SFIELD forms of the eps kernels */
static inline bool mg3d_fused(const mg3d_ctx *ctx)
{
    return ctx->fused && !ctx->eps.set() && ctx->periodic == 0 && ctx->neumann == 0 && !ctx->mask.set() &&
           !ctx->sfield.set();
}
/* a sweep launch on a level of this context, u -> alt: the caller adds what the launch does (SweepLaunch) */
static inline SweepLaunch mg3d_level_sweep(const mg3d_ctx *ctx, const Level &l)
{
    SweepLaunch w;
    w.g = &l.g;
    w.op = mg3d_level_op(l.h, ctx->sigma);
    w.vin = l.f[MG3D_U];
    w.d = l.f[MG3D_D];
    /* the top level's d comes with its zero map when that is known to hold a plane (the one place a launch gets its d) */
    if (&l == &ctx->lv[ctx->L - 1] && ctx->dz_state == MG3D_DZ_VALID && ctx->dz_planes > 0 && ctx->opt.v[MG3D_OPT_D_ZERO_SKIP] &&
        mg3d_fused(ctx)) {
        w.d_zero = ctx->dz_map;
        /* a full map: the launches that have a kernel without d take that one (option 1; 2: the map only) */
        if (l.g.ni > 2 && ctx->dz_planes == l.g.ni - 2 && ctx->opt.v[MG3D_OPT_D_ZERO_SKIP] == 1) {
            w.d_none = true;
            w.d_none_taken = &ctx->dnone_launches;
        }
    }
    w.vout = l.alt;
    w.taken = &ctx->sweep_taken;
    return w;
}
/* the boundary word of the context's levels for the launchers of mg3d_kernels.hip */
static inline int mg3d_ctx_bc(const mg3d_ctx *ctx) { return mg3d_bc(ctx->periodic, ctx->neumann); }
/* the operator of a level of this context for the stencil launchers: the constants of its spacing and the context's sigma,
 * its eps (NULL: constant), the boundary word, its fixed-point bytes (NULL: the context has no mask) and its screening field
 * (NULL: none; with one and no eps, e is eps = 1 at every point).  screened = false: the operator without the field -- the
 * field output, which ignores s as it ignores sigma */
static inline LevelOperator mg3d_level_operator(const mg3d_ctx *ctx, int level, bool screened = true)
{
    const bool field = screened && ctx->sfield.set();
    return {mg3d_level_op(ctx->lv[level].h, ctx->sigma),
            ctx->sigma,
            ctx->eps.set() ? ctx->eps.at(level) : (field ? ctx->ones.at(level) : nullptr),
            mg3d_ctx_bc(ctx),
            ctx->mask.at(level),
            field ? ctx->sfield.at(level) : nullptr};
}
/* sigma = 0, every axis periodic or Neumann on both faces, no fixed unknown on level 0 and no unknown of level 0 at which
 * its screening field is > 0: constants are in the kernel of the coarsest operator, unknown (0,0,0) of level 0 is pinned */
static inline bool mg3d_ctx_pinned(const mg3d_ctx *ctx)
{
    bool closed = true;
    for (int ax = 0; ax < 3; ax++)
        closed = closed && ((ctx->periodic >> ax & 1) || (ctx->neumann >> (2 * ax) & 3) == 3);
    return closed && ctx->sigma == 0. && ctx->mask.count[0] == 0 && ctx->sfield.count[0] == 0;
}
/* ... and none on the finest level either: the system itself is singular (mg3d_wpcg_solve projects) */
static inline bool mg3d_ctx_singular(const mg3d_ctx *ctx)
{
    return mg3d_ctx_pinned(ctx) && ctx->mask.count[1] == 0 && ctx->sfield.count[1] == 0;
}
/* field `field` of `level` was written from outside the cycle (see faces_dirty), and how -- what the zero map of the top
 * level's d (dz_state) makes of it: MG3D_WROTE_DEVICE a kernel of the library wrote values nobody has looked at (NONE),
 * MG3D_WROTE_CALLER the caller's values arrived (UNKNOWN: scanned before the next cycle), MG3D_WROTE_ZERO the field was
 * cleared (VALID, every interior plane, no scan), MG3D_WROTE_FACES only its faces were written (unchanged: the map is about
 * interior points) */
enum { MG3D_WROTE_DEVICE = 0, MG3D_WROTE_CALLER, MG3D_WROTE_ZERO, MG3D_WROTE_FACES };
void mg3d_ctx_touched(mg3d_ctx *ctx, int field, int level, bool raw_pointer = false, int how = MG3D_WROTE_DEVICE);
/* scoped event pair of the timers (mg3d_timing_enable): a stage of the reference's timing table on level l, or
 * (kernel = true) one kernel launch, s a MG3D_K_* id; nothing is recorded while the timers are off (mg3d_ctx.hip) */
struct StageScope {
    mg3d_ctx *ctx;
    mg3d_ctx::Pending p;
    bool on;
    StageScope(mg3d_ctx *c, int l, int s, bool kernel = false);
    ~StageScope();
};
/* records a failure text for mg3d_last_error() and returns `code` */
int mg3d_fail(int code, const char *fmt, ...);
/* a HIP call that may have allocated failed: MG3D_ERR_ALLOC when the device is out of memory, else MG3D_ERR_HIP, with the
 * text "<who>: <what>: <HIP's text>" (what NULL: "<who> failed: <HIP's text>", who the call itself) */
int mg3d_alloc_fail(hipError_t e, const char *who, const char *what = nullptr);
/* hipMalloc for entry point `who`; *p is NULL when it fails */
int mg3d_device_alloc(void **p, size_t bytes, const char *who);
/* enqueue one V-cycle from level q of a (single-domain) context; squared norm of level q to sumsq[slot] */
/* carry_out: end the cycle with the launch that also starts the next one (only mg3d_vcycles asks, and never for the
 * last cycle of a call); ignored where mg3d_can_carry() says no */
/* carry_out: 0 the cycle ends the ordinary way; 1 another cycle of the same call follows; 2 the call ends here and runs
 * ahead speculatively (mg3d_vcycle) */
/* keep_guess: below the finest level, u of level q is the initial guess instead of being zeroed (mg3d_fmg_solve); the
 * levels below q start from zero as always */
int mg3d_enqueue_vcycle(mg3d_ctx *ctx, int q, int slot, int carry_out = 0, bool keep_guess = false);
bool mg3d_can_carry(const mg3d_ctx *ctx, int q);
bool mg3d_can_legs(const mg3d_ctx *ctx, int q);
/* carried state -> the finished cycle's own u; a no-op (MG3D_OK) otherwise.  An error leaves the carried state in place. */
int mg3d_drop_carry(mg3d_ctx *ctx);
int mg3d_drop_carry_keep(mg3d_ctx *ctx); /* the same without clearing red_tail: mg3d_vcycle(s) themselves */
/* what mg3d_ctx.hip and mg3d_operator.hip both need of mg3d_ctx.hip: */
/* MG3D_ERR_HIP "<who>: kernel launch failed: ..." when a launch since the last look left an error */
int mg3d_launch_ok(const char *who);
/* MG3D_ERR_ARG unless ctx is a context, field one of MG3D_U / _D / _R and level one of its levels */
int mg3d_check_field_level(const mg3d_ctx *ctx, int field, int level, const char *who);
/* frees the coarse factor and its work space (nothing in flight may read them any more) */
void mg3d_free_lu(mg3d_ctx *ctx);
/* device arrays (mg3d_ctx.hip; mg3d_step.hip uses them for the source).  mg3d_array_check: MG3D_ERR_ARG unless `a` is a
 * usable descriptor of device memory of the context's device (`writable`: every stride >= 1).  mg3d_stream_join: the
 * two-way join of the caller's stream with the context's -- out = false, before the kernel: the context's stream waits for
 * what the caller's stream holds now; out = true, behind it: the caller's stream waits for what the context's holds now.
 * No host synchronisation. */
int mg3d_array_check(const mg3d_ctx *ctx, const mg3d_array *a, bool writable, const char *who, bool bytes = false /* MG3D_U8 and nothing else: a mask */);
int mg3d_stream_join(mg3d_ctx *ctx, hipStream_t caller, bool out, const char *who);
/* the finest level of a context as the field output and the particle calls need it (mg3d_field.hip): MG3D_ERR_STATE unless
 * it is a single-domain level of at least three points per side */
int mg3d_field_level(const mg3d_ctx *ctx, const char *who);
/* the install path of the screening field (mg3d_operator.hip) for mg3d_nl_solve, which writes the finest level's field with
 * a kernel of its own -- the kernel counts the entries that are not finite, there is no host check of s here:
 * mg3d_sfield_prepare everything that can fail for want of memory (the field of every level, eps = 1 for a context without
 * eps, the two device words io_chk), nothing has changed when it does; mg3d_sfield_rebuild the finest level's duplicates,
 * the restrictions, the counts and level 0's field (one host synchronisation; a HIP error leaves the context without a
 * field); mg3d_operator_changed the coarse factor rebuilt or dropped.  mg3d_check_weight_*: the value check of the field
 * setters (finite and >= 0), on a host or a device array, under another name */
int mg3d_sfield_prepare(mg3d_ctx *ctx, const char *who);
int mg3d_sfield_rebuild(mg3d_ctx *ctx, const char *who);
int mg3d_operator_changed(mg3d_ctx *ctx);
int mg3d_check_weight_host(const mg3d_ctx *ctx, const double *a, const char *name, const char *who);
int mg3d_check_weight_device(mg3d_ctx *ctx, const mg3d_array &a, const char *name, const char *who);

#endif
