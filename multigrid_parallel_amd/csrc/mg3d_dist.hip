/*
 * mg3d_dist.hip -- the V-cycle on i-slabs of several GPUs (one process per GPU, RCCL over xGMI).
 *
 * Partition: the reference's OpenMP path already splits every operator over the slowest index i
 * (`#pragma omp for` over i, mg_3d.h:658-659); its implicit barriers become plane exchanges here.
 * Rank r owns the global planes [b_l(r), b_l(r+1)) of level l, with b_{l+1} = 2*b_l, so coarse plane ic
 * and fine plane 2*ic always have the same owner.  Levels too small to give every rank 16 planes are
 * REPLICATED: the restricted right-hand side is all-gathered once per cycle and every rank runs the
 * remaining levels (and the gauss_elim.h direct solve) redundantly on identical data -- what a gather to
 * rank 0 followed by a broadcast would deliver, bit for bit, with one collective instead of two.
 *
 * Halo: H = 2*nu + 2 planes on each side.  The fused sweep applies S = 2*nu colour passes per launch; a
 * slab end that is not refreshed between passes goes stale one plane per pass, so after a sweep the
 * local planes [S, ni-S) are exact, the residual on [S+1, ni-S-1) -- which covers the owned planes and
 * the one extra fine plane restriction needs (H = S+2).  Planes are contiguous in memory, so a halo is
 * one ncclSend/ncclRecv pair per neighbour, no packing.
 *
 * Exchanges per distributed level l and cycle:
 *   d_(l-1)  after restriction (small; on the compute stream, the coarser level needs it at once);
 *   u_l      after pre-smoothing + restriction.  Nothing touches u_l again until the prolongation on the
 *            way up, so this -- the large one -- runs on the communication stream (its own communicator)
 *            underneath all the smoothing of the coarser levels;
 *   u_(l-1)  after the coarser level's post-smoothing (an eighth of the volume): with fresh halos on the
 *            coarse correction AND on u_l the prolongation is applied to halo planes as well, and the
 *            post-smoother starts at once from 6 exact halo planes, one launch, no exchange;
 *   finest u after post-smoothing, for the next cycle's pre-smoother: on the communication stream,
 *            underneath the residual-norm kernel.  That kernel reads the first halo plane on either side,
 *            so the exchange leaves it alone (the local post-smoother already produced its exact value)
 *            and refreshes planes 2..H only.
 *
 * Transports: RCCL (ncclCommInitRank from a unique id the launcher distributes), or "loopback": all
 * ranks are virtual, live in this process on one GPU and exchange by device copies -- the same
 * schedule code, used to verify the decomposition bit for bit on a single-GPU box.
 */
#include "mg3d_ctx.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <rccl/rccl.h>

#include "mg3d_plan.h"

#define fail mg3d_fail
#define HIPCHK(call)                                                                                    \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(MG3D_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                        __LINE__);                                                                      \
    } while (0)
#define NCCLCHK(call)                                                                                    \
    do {                                                                                                 \
        ncclResult_t e_ = (call);                                                                        \
        if (e_ != ncclSuccess)                                                                           \
            return fail(MG3D_ERR_HIP, "%s failed: %s (%s:%d)", #call, ncclGetErrorString(e_), __FILE__, \
                        __LINE__);                                                                       \
    } while (0)
#define CHK(call)           \
    do {                    \
        int rc_ = (call);   \
        if (rc_ != MG3D_OK) \
            return rc_;     \
    } while (0)

/* ------------------------------------------------------------------------------------------ plan */
extern "C" int mg3d_slab_halo(int smooth_iters) { return 2 * smooth_iters + 2; }

/* first distributed level: every rank must own at least max(16, halo) planes there.  Thinner slabs are launch-
 * latency bound either way (a 65^3 level costs a rank the same whether it sweeps 8+12 planes or all 65), so
 * replicating them is free in kernel time and saves three exchanges per level and cycle (loopback rehearsal, 8
 * ranks: 9.16 ms per cycle with 65^3 replicated against 9.22 distributed; 129^3 replicated as well: 9.61).
 * MG3D_SLAB_MIN_PLANES overrides the 16 (minimum 8): a knob for tuning on real xGMI. */
extern "C" int mg3d_slab_first_level(int coarse_pts, int num_levels, int nranks, int halo)
{
    const char *e = getenv("MG3D_SLAB_MIN_PLANES"); /* read per call: host-side planning only */
    const int v = e ? atoi(e) : 16;
    const int floor_planes = v > 8 ? v : 8;
    const int need = halo > floor_planes ? halo : floor_planes;
    for (int l = 1; l < num_levels; l++) {
        const long long n1 = ((long long)(coarse_pts - 1) << l);
        if (n1 / nranks >= need)
            return l;
    }
    return num_levels; /* nothing can be distributed */
}

/* owned planes [lo, hi) of `rank` on `level` (level >= first distributed level) */
extern "C" int mg3d_slab_owned(int coarse_pts, int num_levels, int nranks, int halo, int level, int rank, int *lo,
                               int *hi)
{
    const int ld = mg3d_slab_first_level(coarse_pts, num_levels, nranks, halo);
    if (level < ld || level >= num_levels || rank < 0 || rank >= nranks)
        return MG3D_ERR_ARG;
    const long long n1 = ((long long)(coarse_pts - 1) << ld); /* N-1 on level ld */
    auto cut = [&](int r) -> long long {
        if (r <= 0)
            return 0;
        const long long Nl = ((long long)(coarse_pts - 1) << level) + 1;
        if (r >= nranks)
            return Nl;
        /* even cut on the first distributed level (its coarse partner ld-1 is split at exact halves),
         * doubled per finer level: b_{l+1} = 2 b_l */
        return ((((n1 / 2) * r) / nranks) * 2) << (level - ld);
    };
    *lo = (int)cut(rank);
    *hi = (int)cut(rank + 1);
    return MG3D_OK;
}

static int build_plan(Plan &pl, int c, int L, int P, int nu, int rank, int overlap, int policy)
{
    if (c < 3 || L < 2 || nu < 1 || P < 1 || rank < 0 || rank >= P)
        return MG3D_ERR_ARG;
    PlanGeom G{c, L, P, nu, mg3d_slab_halo(nu), 0, 16};
    G.ld = mg3d_slab_first_level(c, L, P, G.H);
    if (G.ld >= L)
        return MG3D_ERR_ARG;
    pl = Plan();
    const int lc = G.ld - 1, Nc = ((c - 1) << lc) + 1;
    const long long pec = plan_plane_elems(G, Nc);
    const int cs = overlap ? 1 : 0;
    /* policy bit 3 (8): the cycle before this one ended with the one-launch up-leg (bit 2), which forms only the red half of
     * its residual norm; the black half falls out of this cycle's one-launch down-leg, and the norm is reduced behind it */
    if ((policy & 8) && nu == 2)
        plan_norm(pl, G, L - 1, rank);
    for (int l = L - 1; l >= G.ld; l--) { /* down */
        /* first what the coarser level waits for (its right-hand side), then the large u exchange that hides underneath the
         * coarser levels: with ONE communicator, driven from one in-order stream, the issue order is the execution order */
        if (l - 1 >= G.ld) {
            plan_halo(pl, G, MG3D_XK_HALO_D, MG3D_D, l - 1, rank, 0, 0);
        } else if (policy & 1) {
            const int ph = plan_open_phase(pl, MG3D_XK_RHS_GATHER, lc);
            for (int r = 1; r < P; r++) {
                int lo, hi;
                plan_coarse_range(G, r, &lo, &hi);
                if (rank == r)
                    pl.e.push_back(mg3d_xfer{ph, MG3D_XK_RHS_GATHER, MG3D_XOP_SEND, 0, MG3D_D, lc, lo, hi - lo, pec, 0});
                if (rank == 0)
                    pl.e.push_back(mg3d_xfer{ph, MG3D_XK_RHS_GATHER, MG3D_XOP_RECV, r, MG3D_D, lc, lo, hi - lo, pec, 0});
            }
        } else {
            plan_rhs_allgather(pl, G);
        }
        plan_halo(pl, G, MG3D_XK_HALO_U_DOWN, MG3D_U, l, rank, 0, cs);
    }
    if (policy & 1) {
        const int ph = plan_open_phase(pl, MG3D_XK_CORR_BCAST, lc);
        if (P > 1)
            pl.e.push_back(mg3d_xfer{ph, MG3D_XK_CORR_BCAST, MG3D_XOP_BCAST, 0, MG3D_U, lc, 0, Nc, pec, 0});
    }
    for (int l = G.ld; l < L; l++) { /* up */
        if (l - 1 >= G.ld)
            plan_halo(pl, G, MG3D_XK_HALO_U_UP, MG3D_U, l - 1, rank, 0, 0);
        if (l == L - 1) {
            /* policy bit 1: the cycle is carried into the next one (csrc/mg3d_ctx.hip "carried cycles", V(2,2) only): its
             * last launch has used up every halo plane and already holds three of the next cycle's pre-smoothing passes;
             * the one launch left of that down-leg (one pass + residual + restriction) reads three planes either side */
            /* policy bit 2 (4): one launch per leg (csrc/mg3d_ctx.hip, "one launch per leg"): the up-leg's one launch writes
             * the owned planes only; the next cycle's down-leg (three passes + residual + restriction) reads five either side */
            if ((policy & 4) && nu == 2)
                plan_halo(pl, G, MG3D_XK_HALO_U_NEXT, MG3D_U, l, rank, 0, cs, 5);
            else if ((policy & 2) && nu == 2)
                plan_halo(pl, G, MG3D_XK_HALO_U_NEXT, MG3D_U, l, rank, 0, cs, 3);
            else
                plan_halo(pl, G, MG3D_XK_HALO_U_NEXT, MG3D_U, l, rank, 1, cs);
        }
    }
    if (!((policy & 4) && nu == 2)) /* (bit 2: this cycle's norm is completed and reduced by the next cycle) */
        plan_norm(pl, G, L - 1, rank);
    pl.begin.push_back((int)pl.e.size());
    /* stream: 0 the compute stream (overlap off: every exchange sits where the schedule issues it); overlap on: EVERY
     * exchange is issued on the communication stream with the one communicator -- 1: the compute stream joins at once
     * (the exchange is on the critical path), 2: it joins when it next needs the field (the exchange runs underneath the
     * launches in between: the u halos on the way down, the finest u's halos for the next cycle) */
    for (auto &e : pl.e)
        e.stream = !overlap ? 0 : (e.kind == MG3D_XK_HALO_U_DOWN || e.kind == MG3D_XK_HALO_U_NEXT) ? 2 : 1;
    return MG3D_OK;
}

extern "C" int mg3d_dist_plan(int coarse_pts, int num_levels, int nranks, int smooth_iters, int rank, int overlap,
                              int policy, mg3d_xfer *out, int max_entries)
{
    Plan pl;
    const int rc = build_plan(pl, coarse_pts, num_levels, nranks, smooth_iters, rank, overlap, policy);
    if (rc != MG3D_OK)
        return rc < 0 ? rc : -rc;
    if (out)
        for (int i = 0; i < (int)pl.e.size() && i < max_entries; i++)
            out[i] = pl.e[(size_t)i];
    return (int)pl.e.size();
}

/* ------------------------------------------------------------------------------------- structures */
struct SlabLevel {
    Level lv;
    int glo, ghi;         /* owned global planes */
    int own_lo, own_hi;   /* the same in local plane indices */
    int h_lo, h_hi;       /* halo planes below / above (0 at a physical boundary) */
    double *eps = nullptr; /* mg3d_dist_set_coefficient: eps of this level on every local plane, halos included */
};

struct RankState {
    int legs_npa = 0; /* partial sums the one-launch up-leg has left in coarse->partials */
    int rank;
    std::vector<SlabLevel> dl; /* distributed levels ld .. L-1, index l - ld */
    mg3d_ctx *coarse;          /* replicated levels 0 .. ld-1 */
    double *gather;            /* P doubles: per-rank partial sums of squares */
};

struct mg3d_dist {
    int c, L, nu, P, ld, H;
    double length;
    bool loopback;
    int device;
    ncclComm_t comm;  /* compute-stream collectives and exchanges */
    bool have_comm;
    hipStream_t stream; /* every operation of every local rank is ordered on this one stream */
    hipStream_t comm_stream; /* the u halo exchanges that hide under coarser levels / the norm run here */
    hipEvent_t ev_ready, ev_now; /* compute -> communication stream ("the data is ready"), and back ("it has arrived") */
    std::vector<hipEvent_t> ev_u; /* per level: "the u halos of this level have arrived" */
    std::vector<char> u_pending;  /* per level: ev_u[l] has been recorded and not yet waited for */
    bool overlap; /* MG3D_NO_OVERLAP=1 keeps every exchange on the compute stream */
    std::vector<RankState> rs;
    double *h_norms; /* pinned */
    double *d_norms; /* device: squared norms per cycle */
    int norm_slots;
    std::vector<double> spacing; /* per level */
    double *selftest; /* MG3D_FORCE_COMM=1 on one rank: H planes of the finest level, target of the self-addressed receives */
    /* the exchange plan of one cycle for every local rank (mg3d_dist_plan): the transports below execute it entry by
     * entry and hold no plane arithmetic of their own */
    std::vector<Plan> plans;       /* one cycle on its own */
    std::vector<Plan> plans_carry; /* a cycle that ends ahead into the next one (policy bit 1) */
    std::vector<Plan> plans_legs[3]; /* one launch per leg: a cycle whose up-leg is one launch (policy | 4), one between two such
                                      * (| 12), the one that only completes its predecessor's norm (| 8) */
    bool legs_pending;             /* the last cycle's norm is half formed (red half in every rank's partials[0 .. legs_npa)) */
    bool red_tail;                 /* u of the finest level was last changed by the red pass that ends a V(2,2) cycle, all its halo
                                    * planes are exact and neither u nor d has been touched since (cleared by every entry point that
                                    * could): the next call's first cycle takes the one-launch down-leg too (csrc/mg3d_ctx.hip, red_tail) */
    bool legs_fixed, legs_on;      /* as carry_fixed / carry_on: agreed between the ranks of an RCCL job at creation */
    int n_legs;                    /* cycles whose up-leg ran as one launch (mg3d_dist_legs_cycles) */
    const std::vector<Plan> *cur;  /* the plan of the cycle being enqueued */
    bool carried;                  /* u of the top level holds three pre-smoothing passes of the next cycle */
    /* a call failed after a cycle of it had carried: u of the top level is three passes into a cycle nobody finished and
     * nothing here can put the finished cycle's own u back (the single-domain path has mg3d_drop_carry; on slabs that
     * would be two passes over the owned planes AND a full halo exchange -- on a handle whose transport may just have
     * failed).  Every later call that reads or continues from u fails loudly until u of the top level is uploaded again. */
    bool poisoned;
    /* carried cycles on or off, decided ONCE for a multi-rank RCCL job (mg3d_dist_create: the ranks agree by an
     * all-reduce) -- the two plans differ in the HALO_U_NEXT phase (3 planes against H - 1), and ranks that read
     * MG3D_NO_CARRY / MG3D_CARRY_MIN differently per cycle would post sends and receives of different sizes: a hang or
     * corrupted halos without a diagnostic.  Loopback and single-rank handles follow their options (mg3d_dist_set_option)
     * from cycle to cycle (the tests toggle them). */
    bool carry_fixed, carry_on;
    int n_carried;                 /* cycles that ended that way (mg3d_dist_carried_cycles) */
    /* a variable coefficient is set (mg3d_dist_set_coefficient): eps on every slab level, the replicated contexts have it too;
     * the cycle is the plain one of the unfused kernels (dist_enqueue_vcycle, dist_coef_smooth), no carried cycles or legs */
    bool coef;
    int phase;  /* next phase of the cycle being enqueued */
    int policy; /* bit 0: coarse levels on rank 0 only (MG3D_COARSE_GATHER=1) */
    /* per-phase cost (mg3d_dist_timing_enable): event pairs, resolved at the next synchronisation */
    bool timing;
    struct Timed {
        int bucket; /* 0 cycle, 1 exchange on the compute stream, 2 exchange on the communication stream, 3 coarse levels */
        hipEvent_t a, b;
    };
    std::vector<Timed> timed;
    std::vector<hipEvent_t> ev_pool;
    double t_ms[4];
    int t_cycles;
};

static hipEvent_t dist_take_event(mg3d_dist *D)
{
    hipEvent_t e = nullptr;
    if (!D->ev_pool.empty()) {
        e = D->ev_pool.back();
        D->ev_pool.pop_back();
    } else if (hipEventCreate(&e) != hipSuccess) {
        e = nullptr;
    }
    return e;
}

struct DistScope { /* event pair around a piece of the cycle on stream s */
    mg3d_dist *D;
    mg3d_dist::Timed t;
    hipStream_t s;
    DistScope(mg3d_dist *d, int bucket, hipStream_t st) : D(d), s(st)
    {
        t.bucket = bucket;
        t.a = t.b = nullptr;
        if (D->timing && (t.a = dist_take_event(D)))
            (void)hipEventRecord(t.a, s);
    }
    ~DistScope()
    {
        if (!D->timing || !t.a)
            return;
        if ((t.b = dist_take_event(D)))
            (void)hipEventRecord(t.b, s);
        D->timed.push_back(t);
    }
};

/* call only after the streams have been synchronised */
static void dist_resolve_timers(mg3d_dist *D)
{
    for (auto &t : D->timed) {
        float ms = 0.f;
        if (t.a && t.b && hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess)
            D->t_ms[t.bucket] += ms;
        if (t.a)
            D->ev_pool.push_back(t.a);
        if (t.b)
            D->ev_pool.push_back(t.b);
    }
    D->timed.clear();
}

static SlabLevel &SL(mg3d_dist *D, RankState &R, int l) { return R.dl[l - D->ld]; }

__global__ void sum_in_order_kernel(const double *__restrict__ parts, int n, double *__restrict__ out)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double t = 0.;
        for (int i = 0; i < n; i++)
            t += parts[i];
        *out = t;
    }
}

static bool dist_carry_policy(mg3d_dist *D);
static bool dist_legs_policy(mg3d_dist *D);
static int dist_refuse_poisoned(const mg3d_dist *D, const char *who);

extern "C" int mg3d_comm_unique_id(void *out128)
{
    if (!out128)
        return fail(MG3D_ERR_ARG, "mg3d_comm_unique_id: NULL");
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is expected to be 128 bytes");
    ncclUniqueId id;
    NCCLCHK(ncclGetUniqueId(&id));
    memcpy(out128, &id, sizeof id);
    return MG3D_OK;
}

extern "C" int mg3d_dist_destroy(mg3d_dist *D)
{
    if (!D)
        return MG3D_OK;
    if (D->comm_stream)
        (void)hipStreamSynchronize(D->comm_stream);
    if (D->stream)
        (void)hipStreamSynchronize(D->stream);
    dist_resolve_timers(D);
    for (auto e : D->ev_pool)
        (void)hipEventDestroy(e);
    if (D->ev_ready)
        (void)hipEventDestroy(D->ev_ready);
    if (D->ev_now)
        (void)hipEventDestroy(D->ev_now);
    for (auto e : D->ev_u)
        if (e)
            (void)hipEventDestroy(e);
    if (D->comm_stream)
        (void)hipStreamDestroy(D->comm_stream);
    for (auto &R : D->rs) {
        for (auto &s : R.dl) {
            for (int k = 0; k < 3; k++)
                if (s.lv.f[k])
                    (void)hipFree(s.lv.f[k]);
            if (s.lv.alt)
                (void)hipFree(s.lv.alt);
            if (s.eps)
                (void)hipFree(s.eps);
        }
        if (R.gather)
            (void)hipFree(R.gather);
    }
    /* contexts that borrow the shared stream go first, its owner last */
    for (auto &R : D->rs)
        if (R.coarse && !R.coarse->own_stream) {
            mg3d_ctx_destroy(R.coarse);
            R.coarse = nullptr;
        }
    for (auto &R : D->rs)
        if (R.coarse)
            mg3d_ctx_destroy(R.coarse);
    if (D->selftest)
        (void)hipFree(D->selftest);
    if (D->d_norms)
        (void)hipFree(D->d_norms);
    if (D->h_norms)
        (void)hipHostFree(D->h_norms);
    if (D->have_comm)
        (void)ncclCommDestroy(D->comm);
    delete D;
    return MG3D_OK;
}

extern "C" int mg3d_dist_create(int coarse_pts, int num_levels, int smooth_iters, double grid_length, int rank,
                                int nranks, const void *unique_id, int device, mg3d_dist **out)
{
    if (!out || coarse_pts < 3 || num_levels < 2 || smooth_iters < 1 || nranks < 1 || rank < 0 || rank >= nranks)
        return fail(MG3D_ERR_ARG, "mg3d_dist_create: bad arguments");
    if (mg3d_device_count() <= 0)
        return fail(MG3D_ERR_NO_DEVICE, "no HIP device available: libmg3d has no CPU fallback");
    HIPCHK(hipSetDevice(device));
    mg3d_dist *D = new mg3d_dist();
    D->c = coarse_pts;
    D->L = num_levels;
    D->nu = smooth_iters;
    D->P = nranks;
    D->length = grid_length;
    D->H = mg3d_slab_halo(smooth_iters);
    D->ld = mg3d_slab_first_level(coarse_pts, num_levels, nranks, D->H);
    D->loopback = unique_id == nullptr;
    D->device = device;
    D->have_comm = false;
    D->selftest = nullptr;
    D->stream = nullptr;
    D->h_norms = D->d_norms = nullptr;
    D->comm_stream = nullptr;
    D->ev_ready = D->ev_now = nullptr;
    D->phase = 0;
    D->timing = false;
    D->t_cycles = 0;
    for (double &x : D->t_ms)
        x = 0.;
    D->policy = (getenv("MG3D_COARSE_GATHER") && getenv("MG3D_COARSE_GATHER")[0] == '1') ? 1 : 0;
    /* Overlap of the large u exchanges with the launches in between (round 4: ONE communicator).  Every exchange is issued
     * on the communication stream -- the only stream that ever drives the communicator, so RCCL sees one in-order sequence
     * of operations, identical on all ranks -- behind an event of the compute stream ("the planes are ready"); the compute
     * stream joins by an event when it needs the planes: at once for the exchanges on the critical path, later for the u
     * halos, whose transfers then run underneath the coarser levels / the interior of the next launch.  Default for both
     * transports (rounds 2-3 needed a second communicator for this and kept it off for RCCL); MG3D_NO_OVERLAP=1 keeps
     * every exchange on the compute stream. */
    {
        const bool off = getenv("MG3D_NO_OVERLAP") && getenv("MG3D_NO_OVERLAP")[0] == '1';
        D->overlap = !off;
    }
    if (D->ld >= num_levels) {
        delete D;
        return fail(MG3D_ERR_ARG, "mg3d_dist_create: %d ranks leave no level with >= 8 planes per rank", nranks);
    }
    /* spacing per level: finest = length/(N-1), doubled per coarser level (mg_3d.h:143,1303) */
    D->spacing.resize(num_levels);
    const long long finest = ((long long)(coarse_pts - 1) << (num_levels - 1)) + 1;
    D->spacing[num_levels - 1] = grid_length / (double)(finest - 1);
    for (int l = num_levels - 2; l >= 0; l--)
        D->spacing[l] = 2 * D->spacing[l + 1];
#define DCHK(call)                                                                        \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            int rc_ = mg3d_alloc_fail(e_, #call);                                         \
            mg3d_dist_destroy(D);                                                         \
            return rc_;                                                                   \
        }                                                                                 \
    } while (0)
    const int first = D->loopback ? 0 : rank, last = D->loopback ? nranks : rank + 1;
    for (int r = first; r < last; r++) {
        RankState R;
        R.rank = r;
        R.coarse = nullptr;
        R.gather = nullptr;
        D->rs.push_back(R);
    }
    for (auto &R : D->rs) {
        /* replicated part: an ordinary single-domain context of the ld lowest levels */
        const int rc = mg3d_ctx_create(coarse_pts, D->ld, smooth_iters, 1.0, &R.coarse);
        if (rc != MG3D_OK) {
            mg3d_dist_destroy(D);
            return rc;
        }
        for (int l = 0; l < D->ld; l++)
            R.coarse->lv[l].h = D->spacing[l];
        if (!D->stream)
            D->stream = R.coarse->stream; /* shared by all local ranks: one ordered queue */
        else {
            (void)hipStreamDestroy(R.coarse->stream);
            R.coarse->stream = D->stream;
            R.coarse->own_stream = false;
        }
        DCHK(hipMalloc(&R.gather, sizeof(double) * nranks));
        R.dl.resize(num_levels - D->ld);
        for (int l = D->ld; l < num_levels; l++) {
            SlabLevel &s = R.dl[l - D->ld];
            for (int k = 0; k < 3; k++)
                s.lv.f[k] = nullptr;
            s.lv.alt = nullptr;
            mg3d_slab_owned(coarse_pts, num_levels, nranks, D->H, l, R.rank, &s.glo, &s.ghi);
            const int N = (coarse_pts - 1) * (1 << l) + 1;
            s.h_lo = R.rank > 0 ? D->H : 0;
            s.h_hi = R.rank < nranks - 1 ? D->H : 0;
            Geom &g = s.lv.g;
            g.N = N;
            g.nj = g.nk = N;
            g.ig0 = s.glo - s.h_lo;
            g.ni = (s.ghi - s.glo) + s.h_lo + s.h_hi;
            g.pitch = mg3d_pitch_for(N);
            g.plane = (long long)g.pitch * N;
            s.own_lo = s.h_lo;
            s.own_hi = s.h_lo + (s.ghi - s.glo);
            s.lv.h = D->spacing[l];
            s.lv.elems = (size_t)g.plane * g.ni;
            for (int k = 0; k < 3; k++) {
                DCHK(hipMalloc(&s.lv.f[k], s.lv.elems * sizeof(double)));
                DCHK(hipMemsetAsync(s.lv.f[k], 0, s.lv.elems * sizeof(double), D->stream));
            }
            DCHK(hipMalloc(&s.lv.alt, s.lv.elems * sizeof(double)));
            DCHK(hipMemsetAsync(s.lv.alt, 0, s.lv.elems * sizeof(double), D->stream));
        }
    }
    DCHK(hipStreamCreateWithFlags(&D->comm_stream, hipStreamNonBlocking));
    DCHK(hipEventCreateWithFlags(&D->ev_ready, hipEventDisableTiming));
    DCHK(hipEventCreateWithFlags(&D->ev_now, hipEventDisableTiming));
    D->ev_u.assign(num_levels, nullptr);
    D->u_pending.assign(num_levels, 0);
    for (int l = D->ld; l < num_levels; l++)
        DCHK(hipEventCreateWithFlags(&D->ev_u[l], hipEventDisableTiming));
    D->norm_slots = 1024;
    DCHK(hipMalloc(&D->d_norms, sizeof(double) * D->norm_slots));
    DCHK(hipHostMalloc(&D->h_norms, sizeof(double) * D->norm_slots));
    DCHK(hipStreamSynchronize(D->stream));
#undef DCHK
    /* MG3D_FORCE_COMM=1: build the communicators for a single rank too (lets a one-GPU box exercise the unique-id
     * marshalling, ncclCommInitRank and ncclCommSplit of the multi-process path) */
    const bool force_comm = getenv("MG3D_FORCE_COMM") && getenv("MG3D_FORCE_COMM")[0] == '1';
    if (!D->loopback && (nranks > 1 || force_comm)) {
        ncclUniqueId id;
        memcpy(&id, unique_id, sizeof id);
        ncclResult_t e = ncclCommInitRank(&D->comm, nranks, id, rank);
        if (e != ncclSuccess) {
            const int rc = fail(MG3D_ERR_HIP, "ncclCommInitRank failed: %s", ncclGetErrorString(e));
            mg3d_dist_destroy(D);
            return rc;
        }
        D->have_comm = true;
        if (nranks > 1)
            k_sweep_set_tune_default(0); /* no host-blocking first-use measurement while ranks wait for each other */
        if (nranks == 1) { /* forced: scratch for the self-addressed exchanges */
            const Geom &gt = D->rs[0].dl.back().lv.g;
            if (hipMalloc(&D->selftest, (size_t)D->H * gt.plane * sizeof(double)) != hipSuccess)
                D->selftest = nullptr;
        }
    }
    /* the plan every exchange below is read from; built after the overlap decision is final */
    D->plans.resize(D->rs.size());
    for (size_t ri = 0; ri < D->rs.size(); ri++) {
        const int rc = build_plan(D->plans[ri], coarse_pts, num_levels, nranks, smooth_iters, D->rs[ri].rank,
                                  D->overlap ? 1 : 0, D->policy);
        if (rc != MG3D_OK) {
            mg3d_dist_destroy(D);
            return fail(rc, "mg3d_dist_create: no exchange plan for rank %d of %d", D->rs[ri].rank, nranks);
        }
    }
    D->plans_carry.resize(D->rs.size());
    for (size_t ri = 0; ri < D->rs.size(); ri++)
        (void)build_plan(D->plans_carry[ri], coarse_pts, num_levels, nranks, smooth_iters, D->rs[ri].rank, D->overlap ? 1 : 0,
                         D->policy | 2); /* same arguments as above: cannot fail where that did not */
    static const int legs_bits[3] = {4, 12, 8};
    for (int v = 0; v < 3; v++) {
        D->plans_legs[v].resize(D->rs.size());
        for (size_t ri = 0; ri < D->rs.size(); ri++)
            (void)build_plan(D->plans_legs[v][ri], coarse_pts, num_levels, nranks, smooth_iters, D->rs[ri].rank, D->overlap ? 1 : 0,
                             D->policy | legs_bits[v]);
    }
    D->cur = &D->plans;
    D->carried = false;
    D->poisoned = false;
    D->n_carried = 0;
    D->carry_fixed = false;
    D->carry_on = false;
    D->legs_pending = false;
    D->red_tail = false;
    D->legs_fixed = false;
    D->legs_on = false;
    D->n_legs = 0;
    D->coef = false;
    if (D->have_comm && nranks > 1) {
        /* every rank must pick the same plan variant: all-reduce MIN of "carried cycles are on here", "one launch per leg is" */
        int mine[2] = {dist_carry_policy(D) ? 1 : 0, dist_legs_policy(D) ? 1 : 0}, *dflag = nullptr;
        bool ok = hipMalloc(&dflag, sizeof(mine)) == hipSuccess &&
                  hipMemcpyAsync(dflag, mine, sizeof(mine), hipMemcpyHostToDevice, D->stream) == hipSuccess &&
                  ncclAllReduce(dflag, dflag, 2, ncclInt, ncclMin, D->comm, D->stream) == ncclSuccess &&
                  hipMemcpyAsync(mine, dflag, sizeof(mine), hipMemcpyDeviceToHost, D->stream) == hipSuccess &&
                  hipStreamSynchronize(D->stream) == hipSuccess;
        if (dflag)
            (void)hipFree(dflag);
        if (!ok) {
            mg3d_dist_destroy(D);
            return fail(MG3D_ERR_HIP, "mg3d_dist_create: the ranks could not agree on the cycle schedule (all-reduce failed)");
        }
        D->carry_fixed = true;
        D->carry_on = mine[0] != 0;
        D->legs_fixed = true;
        D->legs_on = mine[1] != 0;
    }
    *out = D;
    return MG3D_OK;
}

extern "C" int mg3d_dist_timing_enable(mg3d_dist *D, int on)
{
    if (!D)
        return fail(MG3D_ERR_ARG, "mg3d_dist_timing_enable: NULL");
    HIPCHK(hipStreamSynchronize(D->comm_stream));
    HIPCHK(hipStreamSynchronize(D->stream));
    dist_resolve_timers(D);
    D->timing = on != 0;
    if (on) {
        for (double &x : D->t_ms)
            x = 0.;
        D->t_cycles = 0;
    }
    return MG3D_OK;
}

extern "C" int mg3d_dist_timing_get(mg3d_dist *D, double ms[4], int *cycles)
{
    if (!D || !ms)
        return fail(MG3D_ERR_ARG, "mg3d_dist_timing_get: NULL");
    HIPCHK(hipStreamSynchronize(D->comm_stream));
    HIPCHK(hipStreamSynchronize(D->stream));
    dist_resolve_timers(D);
    for (int i = 0; i < 4; i++)
        ms[i] = D->t_ms[i];
    if (cycles)
        *cycles = D->t_cycles;
    return MG3D_OK;
}

extern "C" int mg3d_dist_comm_info(const mg3d_dist *D, int *rccl_ranks, int *overlap, int *device)
{
    if (!D)
        return fail(MG3D_ERR_ARG, "mg3d_dist_comm_info: NULL");
    int n = 0;
    if (D->have_comm)
        NCCLCHK(ncclCommCount(D->comm, &n));
    if (rccl_ranks)
        *rccl_ranks = n; /* 0: no RCCL communicator (loopback, or one rank) */
    if (overlap)
        *overlap = D->overlap ? 1 : 0;
    if (device)
        *device = D->device;
    return MG3D_OK;
}

extern "C" int mg3d_dist_first_level(const mg3d_dist *D) { return D ? D->ld : -1; }
extern "C" int mg3d_dist_halo(const mg3d_dist *D) { return D ? D->H : -1; }
extern "C" int mg3d_dist_carried_cycles(const mg3d_dist *D) { return D ? D->n_carried : -1; }
extern "C" int mg3d_dist_legs_cycles(const mg3d_dist *D) { return D ? D->n_legs : -1; }

/* launch / schedule policy by key (mg3d_ctx_set_option) for every local rank.  carry / carry_min of a multi-rank RCCL job
 * are fixed when the handle is created (the ranks agree there) and refuse to change. */
extern "C" int mg3d_dist_set_option(mg3d_dist *D, const char *key, int value)
{
    if (!D)
        return fail(MG3D_ERR_ARG, "mg3d_dist_set_option: NULL");
    D->red_tail = false;
    const int i = mg3d_option_index(key);
    if (i < 0)
        return fail(MG3D_ERR_ARG, "mg3d_dist_set_option: no option \"%s\"", key ? key : "(null)");
    if ((D->carry_fixed && (i == MG3D_OPT_CARRY || i == MG3D_OPT_CARRY_MIN)) || (D->legs_fixed && (i == MG3D_OPT_LEGS || i == MG3D_OPT_LEGS_MIN)))
        return fail(MG3D_ERR_STATE, "mg3d_dist_set_option: %s is agreed between the ranks at creation", key);
    if (D->carried || D->legs_pending)
        return fail(MG3D_ERR_STATE, "mg3d_dist_set_option: inside a carried cycle");
    for (auto &R : D->rs)
        CHK(mg3d_ctx_set_option(R.coarse, key, value));
    return MG3D_OK;
}

extern "C" int mg3d_dist_set_keep_residual(mg3d_dist *D, int keep)
{
    if (!D)
        return fail(MG3D_ERR_ARG, "mg3d_dist_set_keep_residual: NULL");
    D->red_tail = false;
    CHK(dist_refuse_poisoned(D, "mg3d_dist_set_keep_residual"));
    for (auto &R : D->rs)
        R.coarse->keep_r = keep != 0;
    return MG3D_OK;
}

extern "C" int mg3d_dist_build_coarse(mg3d_dist *D, double h_coarse)
{
    if (!D)
        return fail(MG3D_ERR_ARG, "mg3d_dist_build_coarse: NULL");
    D->red_tail = false;
    for (auto &R : D->rs)
        CHK(mg3d_ctx_build_coarse(R.coarse, h_coarse));
    return MG3D_OK;
}

/* the screened operator (mg3d_ctx_set_shift) on every local rank: its slab levels take sigma from the rank's replicated
 * context (mg3d_level_op), whose coarse factor is rebuilt there.  A multi-rank job must agree on sigma (not checked). */
extern "C" int mg3d_dist_set_shift(mg3d_dist *D, double sigma)
{
    if (!D || !(sigma >= 0.) || !isfinite(sigma))
        return fail(MG3D_ERR_ARG, "mg3d_dist_set_shift: %s", D ? "sigma must be finite and >= 0" : "NULL");
    if (D->carried || D->legs_pending)
        return fail(MG3D_ERR_STATE, "mg3d_dist_set_shift: inside a carried cycle");
    D->red_tail = false;
    for (auto &R : D->rs)
        CHK(mg3d_ctx_set_shift(R.coarse, sigma));
    return MG3D_OK;
}

static void dist_free_eps(mg3d_dist *D)
{
    for (auto &R : D->rs)
        for (auto &sl : R.dl) {
            if (sl.eps)
                (void)hipFree(sl.eps);
            sl.eps = nullptr;
        }
    D->coef = false;
}

/* The variable-coefficient operator (mg3d_ctx_set_coefficient) on every local rank.  eps_full is the finest level's dense
 * N^3 array; every level takes its injection, subsampled here on the host, because a coarse slab's halo planes are not
 * injections of planes the fine slab holds: each rank uploads its window of every distributed level, halos included, and
 * its replicated context gets level ld-1's (which builds the coarse matrix from level 0's).  With an RCCL communicator the
 * ranks first agree by one all-reduce: any rank's invalid array fails the call on every rank (MG3D_ERR_ARG), ranks that
 * disagree on on / off fail it with MG3D_ERR_STATE (a coefficient rank walks the plain plan, a constant one may walk the
 * legs or carried plan: their exchanges would never match).  The VALUES of eps are not compared between ranks, nor is
 * sigma.  NULL: the constant operator and its schedules again. */
extern "C" int mg3d_dist_set_coefficient(mg3d_dist *D, const double *eps)
{
    if (!D)
        return fail(MG3D_ERR_ARG, "mg3d_dist_set_coefficient: NULL handle");
    if (D->carried || D->legs_pending)
        return fail(MG3D_ERR_STATE, "mg3d_dist_set_coefficient: inside a carried cycle");
    D->red_tail = false;
    const int L = D->L;
    const long long N = ((long long)(D->c - 1) << (L - 1)) + 1, n = N * N * N;
    long long bad = -1;
    if (eps)
        for (long long p = 0; p < n && bad < 0; p++)
            if (!(eps[p] > 0.) || !isfinite(eps[p]))
                bad = p;
    const int on = eps ? 1 : 0;
    int all_valid = bad < 0, agree = 1;
    if (D->have_comm) {
        /* MIN of {valid here, on here, off here}: every rank valid, every rank on, every rank off */
        int f[3] = {bad < 0 ? 1 : 0, on, 1 - on}, *dflag = nullptr;
        bool ok = hipStreamSynchronize(D->comm_stream) == hipSuccess && hipMalloc(&dflag, sizeof(f)) == hipSuccess &&
                  hipMemcpyAsync(dflag, f, sizeof(f), hipMemcpyHostToDevice, D->stream) == hipSuccess &&
                  ncclAllReduce(dflag, dflag, 3, ncclInt, ncclMin, D->comm, D->stream) == ncclSuccess &&
                  hipMemcpyAsync(f, dflag, sizeof(f), hipMemcpyDeviceToHost, D->stream) == hipSuccess &&
                  hipStreamSynchronize(D->stream) == hipSuccess;
        if (dflag)
            (void)hipFree(dflag);
        if (!ok)
            return fail(MG3D_ERR_HIP, "mg3d_dist_set_coefficient: the ranks could not agree (all-reduce failed)");
        all_valid = f[0];
        agree = f[1] + f[2] == 1;
    }
    if (bad >= 0)
        return fail(MG3D_ERR_ARG, "mg3d_dist_set_coefficient: eps[%lld] = %g (every entry must be finite and > 0)", bad,
                    eps[bad]);
    if (!all_valid)
        return fail(MG3D_ERR_ARG, "mg3d_dist_set_coefficient: another rank's eps has an entry that is not finite and > 0");
    if (!agree)
        return fail(MG3D_ERR_STATE, "mg3d_dist_set_coefficient: the ranks disagree on whether a coefficient is set");
    HIPCHK(hipStreamSynchronize(D->comm_stream));
    HIPCHK(hipStreamSynchronize(D->stream)); /* launches in flight read eps */
    if (!eps) {
        dist_free_eps(D);
        for (auto &R : D->rs)
            CHK(mg3d_ctx_set_coefficient(R.coarse, nullptr));
        return MG3D_OK;
    }
    if (!D->coef) {
        for (auto &R : D->rs)
            for (auto &sl : R.dl) {
                const int rc = mg3d_device_alloc((void **)&sl.eps, sl.lv.elems * sizeof(double), "mg3d_dist_set_coefficient");
                if (rc == MG3D_OK)
                    continue;
                dist_free_eps(D);
                return rc;
            }
    }
    std::vector<double> sub;
    for (int l = L - 1; l >= D->ld - 1; l--) {
        const long long Nl = ((long long)(D->c - 1) << l) + 1, st = 1LL << (L - 1 - l);
        const double *src = eps;
        if (l < L - 1) { /* the injection: every st-th point of the finest level */
            sub.resize((size_t)(Nl * Nl * Nl));
            for (long long i = 0; i < Nl; i++)
                for (long long j = 0; j < Nl; j++)
                    for (long long k = 0; k < Nl; k++)
                        sub[(size_t)((i * Nl + j) * Nl + k)] = eps[((i * st) * N + j * st) * N + k * st];
            src = sub.data();
        }
        if (l < D->ld) {
            for (auto &R : D->rs)
                CHK(mg3d_ctx_set_coefficient(R.coarse, src));
            continue;
        }
        for (auto &R : D->rs) {
            SlabLevel &sl = SL(D, R, l);
            const Geom &g = sl.lv.g;
            HIPCHK(hipMemcpy2DAsync(sl.eps, g.pitch * sizeof(double), src + (size_t)g.ig0 * Nl * Nl, Nl * sizeof(double),
                                    Nl * sizeof(double), (size_t)g.ni * Nl, hipMemcpyHostToDevice, D->stream));
        }
        HIPCHK(hipStreamSynchronize(D->stream)); /* before `sub` is rewritten */
    }
    D->coef = true;
    return MG3D_OK;
}

extern "C" int mg3d_dist_has_coefficient(const mg3d_dist *D, int *on)
{
    if (!D || !on)
        return fail(MG3D_ERR_ARG, "mg3d_dist_has_coefficient: NULL argument");
    *on = D->coef ? 1 : 0;
    return MG3D_OK;
}

/* eps of a level as the kernels use it: the planes each local rank owns into the full host array (replicated levels: all) */
extern "C" int mg3d_dist_get_coefficient(mg3d_dist *D, int level, double *host)
{
    if (!D || !host || level < 0 || level >= D->L)
        return fail(MG3D_ERR_ARG, "mg3d_dist_get_coefficient: %s", (!D || !host) ? "NULL argument" : "bad level");
    if (!D->coef)
        return fail(MG3D_ERR_STATE, "mg3d_dist_get_coefficient: no coefficient set");
    if (level < D->ld)
        return mg3d_ctx_get_coefficient(D->rs[0].coarse, level, host);
    for (auto &R : D->rs) {
        SlabLevel &sl = SL(D, R, level);
        const Geom &g = sl.lv.g;
        const int N = g.N;
        HIPCHK(hipMemcpy2DAsync(host + (size_t)sl.glo * N * N, N * sizeof(double), sl.eps + g.plane * sl.own_lo,
                                g.pitch * sizeof(double), N * sizeof(double), (size_t)(sl.own_hi - sl.own_lo) * N,
                                hipMemcpyDeviceToHost, D->stream));
    }
    HIPCHK(hipStreamSynchronize(D->stream));
    return MG3D_OK;
}

/* ------------------------------------------------------------------------------------ data movement */
static int dist_field_ptr(mg3d_dist *D, RankState &R, int field, int level, double **ptr, Geom *g)
{
    if (field < 0 || field > 2 || level < 0 || level >= D->L)
        return fail(MG3D_ERR_ARG, "mg3d_dist: bad field/level (%d, %d)", field, level);
    if (level >= D->ld) {
        *ptr = SL(D, R, level).lv.f[field];
        *g = SL(D, R, level).lv.g;
    } else {
        *ptr = R.coarse->lv[level].f[field];
        *g = R.coarse->lv[level].g;
    }
    return MG3D_OK;
}

/* host is the FULL N^3 array (reference layout); every local rank takes its slab (halos included) */
extern "C" int mg3d_dist_upload(mg3d_dist *D, int field, int level, const double *host)
{
    if (!D || !host)
        return fail(MG3D_ERR_ARG, "mg3d_dist_upload: NULL");
    D->red_tail = false;
    if (field == MG3D_U && level == D->L - 1)
        D->poisoned = false; /* u of the finest level, halos included, is replaced: nothing of the failed call is left */
    for (auto &R : D->rs) {
        double *p;
        Geom g;
        CHK(dist_field_ptr(D, R, field, level, &p, &g));
        const int N = g.N;
        HIPCHK(hipMemcpy2DAsync(p, g.pitch * sizeof(double), host + (size_t)g.ig0 * N * N, N * sizeof(double),
                                N * sizeof(double), (size_t)g.ni * N, hipMemcpyHostToDevice, D->stream));
        if (level < D->ld)
            mg3d_ctx_touched(R.coarse, field, level);
    }
    HIPCHK(hipStreamSynchronize(D->stream));
    return MG3D_OK;
}

/* writes the planes each local rank OWNS into the full host array (other planes untouched) */
extern "C" int mg3d_dist_download(mg3d_dist *D, int field, int level, double *host)
{
    if (!D || !host)
        return fail(MG3D_ERR_ARG, "mg3d_dist_download: NULL");
    CHK(dist_refuse_poisoned(D, "mg3d_dist_download"));
    for (auto &R : D->rs) {
        double *p;
        Geom g;
        CHK(dist_field_ptr(D, R, field, level, &p, &g));
        const int N = g.N;
        int lo = 0, hi = g.ni, glo = 0;
        if (level >= D->ld) {
            SlabLevel &s = SL(D, R, level);
            lo = s.own_lo;
            hi = s.own_hi;
            glo = s.glo;
        }
        HIPCHK(hipMemcpy2DAsync(host + (size_t)glo * N * N, N * sizeof(double), p + g.plane * lo,
                                g.pitch * sizeof(double), N * sizeof(double), (size_t)(hi - lo) * N,
                                hipMemcpyDeviceToHost, D->stream));
    }
    HIPCHK(hipStreamSynchronize(D->stream));
    return MG3D_OK;
}

extern "C" int mg3d_dist_sync(mg3d_dist *D)
{
    if (!D)
        return fail(MG3D_ERR_ARG, "mg3d_dist_sync: NULL");
    HIPCHK(hipStreamSynchronize(D->stream));
    return MG3D_OK;
}

/* --------------------------------------------------------------------------------------- transport */
/* Executes the next phase of the cycle's plan for every local rank; `kind` / `level` say where the schedule believes it
 * is -- a mismatch means schedule and plan have come apart, and nothing is sent.  RCCL: one group of the rank's
 * sends / receives / broadcasts exactly as listed.  Loopback: every send is copied into the receive entry that names it
 * in the peer's plan of the same phase (counts must agree), every broadcast range from the root's array into all others. */
static int run_phase(mg3d_dist *D, int kind, int level, hipStream_t s, int bucket = 1 /* timer: 1 waited for at once, 2 overlapped */)
{
    const int ph = D->phase++;
    for (auto &pl : *D->cur)
        if (ph >= (int)pl.kind.size() || pl.kind[(size_t)ph] != kind || pl.level[(size_t)ph] != level)
            return fail(MG3D_ERR_STATE, "slab schedule and exchange plan out of step at phase %d (schedule: kind %d level %d)",
                        ph, kind, level);
    if (D->P == 1) {
        /* forced single-rank communicators (MG3D_FORCE_COMM=1): a grouped send/receive addressed to itself, landing in
         * a scratch buffer -- a one-GPU self-test of the calls, streams and events */
        const bool halo = kind == MG3D_XK_HALO_U_DOWN || kind == MG3D_XK_HALO_D || kind == MG3D_XK_HALO_U_UP ||
                          kind == MG3D_XK_HALO_U_NEXT;
        if (D->have_comm && D->selftest && halo) {
            SlabLevel &a = SL(D, D->rs[0], level);
            const int n = D->H - (kind == MG3D_XK_HALO_U_NEXT ? 1 : 0);
            const size_t cnt = (size_t)n * a.lv.g.plane;
            const int field = kind == MG3D_XK_HALO_D ? MG3D_D : MG3D_U;
            ncclComm_t comm = D->comm;
            NCCLCHK(ncclGroupStart());
            NCCLCHK(ncclSend(a.lv.f[field] + a.lv.g.plane * a.own_lo, cnt, ncclDouble, 0, comm, s));
            NCCLCHK(ncclRecv(D->selftest, cnt, ncclDouble, 0, comm, s));
            NCCLCHK(ncclGroupEnd());
        }
        return MG3D_OK;
    }
    DistScope timer(D, bucket, s);
    auto base = [&](size_t ri, const mg3d_xfer &e) -> double * {
        RankState &R = D->rs[ri];
        return e.level >= D->ld ? SL(D, R, e.level).lv.f[e.field] : R.coarse->lv[e.level].f[e.field];
    };
    auto sumsq = [&](size_t ri) -> double * { return D->rs[ri].coarse->sumsq; };
    return plan_run<double>(*D->cur, ph, D->loopback, D->comm, ncclDouble, s, base, sumsq, D->rs[0].gather);
}

/* One exchange phase.  Overlap on (the default): issued on the communication stream -- the one stream that drives the one
 * communicator -- behind everything queued on the compute stream so far; `defer` = false: the compute stream joins at once
 * (the exchange is on the critical path), true: it joins in await_u(l), i.e. the transfer runs underneath whatever the
 * compute stream does until then (u halos of level l only: one pending exchange per level). */
static int exchange(mg3d_dist *D, int kind, int l, bool defer)
{
    if (!D->overlap || (D->P == 1 && !D->selftest))
        return run_phase(D, kind, l, D->stream);
    HIPCHK(hipEventRecord(D->ev_ready, D->stream));
    HIPCHK(hipStreamWaitEvent(D->comm_stream, D->ev_ready, 0));
    CHK(run_phase(D, kind, l, D->comm_stream, defer ? 2 : 1));
    if (defer) {
        HIPCHK(hipEventRecord(D->ev_u[l], D->comm_stream));
        D->u_pending[l] = 1;
    } else {
        HIPCHK(hipEventRecord(D->ev_now, D->comm_stream));
        HIPCHK(hipStreamWaitEvent(D->stream, D->ev_now, 0));
    }
    return MG3D_OK;
}

/* Start refreshing the u halos of level l behind everything queued on the compute stream so far, without
 * holding the compute stream up; await_u() makes the compute stream wait for the arrival. */
static int start_u_exchange(mg3d_dist *D, int kind, int l) { return exchange(D, kind, l, true); }

static int await_u(mg3d_dist *D, int l)
{
    if (D->u_pending[l]) {
        HIPCHK(hipStreamWaitEvent(D->stream, D->ev_u[l], 0));
        D->u_pending[l] = 0;
    }
    return MG3D_OK;
}

/* total = sum over ranks (in rank order, so every rank gets the same bits) of each rank's sumsq[0] */
static int reduce_norm(mg3d_dist *D, int slot)
{
    hipStream_t s = D->stream;
    CHK(exchange(D, MG3D_XK_NORM, D->L - 1, false));
    RankState &R = D->rs[0];
    if (D->P == 1 || (!D->loopback && !D->have_comm)) {
        if (D->P == 1 && D->have_comm) { /* forced single-rank communicator: the collective itself (self-test), on the stream
                                          * that drives the communicator */
            hipStream_t xs = (D->overlap && D->selftest) ? D->comm_stream : s;
            if (xs != s) {
                HIPCHK(hipEventRecord(D->ev_ready, s));
                HIPCHK(hipStreamWaitEvent(xs, D->ev_ready, 0));
            }
            NCCLCHK(ncclAllGather(R.coarse->sumsq, R.gather, 1, ncclDouble, D->comm, xs));
            if (xs != s) {
                HIPCHK(hipEventRecord(D->ev_now, xs));
                HIPCHK(hipStreamWaitEvent(s, D->ev_now, 0));
            }
        } else
            HIPCHK(hipMemcpyAsync(R.gather, R.coarse->sumsq, sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    hipLaunchKernelGGL(sum_in_order_kernel, dim3(1), dim3(64), 0, s, R.gather, D->P, D->d_norms + slot);
    return MG3D_OK;
}

/* ----------------------------------------------------------------------------------------- V-cycle */
struct RestrictTarget { /* where a rank's restricted residual goes: coarse geometry, array, local planes */
    const Geom *gc;
    double *dc;
    int lo, hi;
};
static void restrict_into(SweepLaunch &w, const RestrictTarget &t)
{
    w.gc = t.gc;
    w.dc = t.dc;
    w.ic_lo = t.lo;
    w.ic_hi = t.hi;
}

struct ProlongSource { /* per local rank: the coarse correction an up-leg folds into its first launch */
    const Geom *gc;
    const double *ec;
};
static void prolong_from(SweepLaunch &w, const ProlongSource &p)
{
    w.gce = p.gc;
    w.ec = p.ec;
}

/* What one cycle does, settled before its first launch (dist_begin_cycle): the slab counterpart of mg3d_ctx.hip's CycleState.
 * What a cycle leaves for the next one (carried, legs_pending, red_tail) stays on the handle. */
struct SlabCycle {
    int slot;
    bool carry_out, legs_out; /* another cycle follows, and this one ends ahead into it (dist_enqueue_vcycle) */
    bool carry_in, legs_in;   /* the previous cycle did */
    bool red_in;              /* behind a finished cycle of an earlier call (red_tail): the one-launch down-leg without a norm half */
    bool can_legs, can_carry, keep_r;
};

struct Window {
    int lo, hi;
};
/* the owned planes of a slab level and m more on either side, as far as the slab has them */
static Window slab_window(const SlabLevel &sl, int m)
{
    return Window{sl.own_lo - m < 0 ? 0 : sl.own_lo - m, sl.own_hi + m > sl.lv.g.ni ? sl.lv.g.ni : sl.own_hi + m};
}

/* The launches of a smoothing stage on distributed level l: the single domain's list (mg3d_stage_plan) with the slab path's
 * two differences as inputs -- it has no one-launch form of the whole down-leg (leg4_form), and the norm is wanted exactly
 * where want_res == 1 (the pre-smoothing norm is dropped, :1294).  has_coarse: a list of restriction targets was passed
 * (with keep_r the down-leg passes a list of empty ones: the stage still splits as if it restricted). */
static StagePlan dist_stage_plan(mg3d_dist *D, int l, int post, int want_res, bool has_coarse, bool pro_offered)
{
    const Geom &g = SL(D, D->rs[0], l).lv.g;
    return mg3d_stage_plan(D->rs[0].coarse->opt,
                           StageAsk{g.N, g.nj, post != 0, D->nu, want_res, has_coarse, want_res == 1, pro_offered, /* leg4_form */ false, /* zero_in */ false,
                                    /* down_form */ false});
}

/* a sweep launch on rank ri's slab of level l, u -> alt, over the owned planes; the norm counts the owned planes */
static SweepLaunch slab_sweep(mg3d_dist *D, size_t ri, int l)
{
    SlabLevel &sl = SL(D, D->rs[ri], l);
    SweepLaunch w = mg3d_level_sweep(D->rs[ri].coarse, sl.lv);
    w.i_lo = w.acc_lo = sl.own_lo;
    w.i_hi = w.acc_hi = sl.own_hi;
    return w;
}

static void swap_u_all(mg3d_dist *D, int l) /* every local rank's u and alt of level l change roles */
{
    for (auto &R : D->rs)
        swap_u(SL(D, R, l).lv);
}

/* The launch that makes u of the finest level final for this cycle, over the owned planes +- margin, and the HALO_U_NEXT
 * exchange behind it.  Edge windows first (round 4): the first and last E output planes -- the window's margin + the planes
 * the exchange skips + those it sends -- go first, as ONE launch of two chunks per rank, u -> alt; the buffers change roles
 * and the exchange runs on the communication stream underneath the second launch, alt -> u, which makes the interior.  Same
 * bits: the chunking of a sweep launch is a work distribution only.  Without a communication stream, or where some rank's
 * window is shorter than 2E + 2 planes (thin slabs): one launch per rank, the swap, the exchange.
 * make(ri, split, n_edge) describes rank ri's launch but for its window: n_edge < 0 the first (or only) one, otherwise the
 * interior behind an edge launch that wrote n_edge partial sums.  done(ri, n_first, n_in) follows the rank's last launch
 * (n_in 0: not split): where the sums go and how they are folded is the callers', and the norm's bits depend on it. */
template <class Make, class Done>
static int edge_first(mg3d_dist *D, int l, int margin, int E, const char *what, Make make, Done done)
{
    bool split = D->overlap && D->P > 1;
    std::vector<Window> win;
    for (auto &R : D->rs) {
        win.push_back(slab_window(SL(D, R, l), margin));
        split = split && win.back().hi - win.back().lo >= 2 * E + 2;
    }
    std::vector<int> n_first(D->rs.size());
    for (size_t ri = 0; ri < D->rs.size(); ri++) {
        SweepLaunch w = make(ri, split, -1);
        w.i_lo = win[ri].lo;
        w.i_hi = win[ri].hi;
        w.edge = split ? E : 0;
        n_first[ri] = k_sweep(D->rs[ri].coarse->opt, w, D->stream);
        if (n_first[ri] <= 0) /* nothing was launched: no buffer swap, no fold */
            return fail(MG3D_ERR_STATE, "slab sweep: no kernel for %s%s on level %d", split ? "the edge windows of " : "", what, l);
        if (!split)
            done(ri, n_first[ri], 0);
    }
    swap_u_all(D, l); /* the exchange sends from (and lands in) the NEW buffer */
    CHK(start_u_exchange(D, MG3D_XK_HALO_U_NEXT, l));
    for (size_t ri = 0; split && ri < D->rs.size(); ri++) {
        Level &lv = SL(D, D->rs[ri], l).lv;
        SweepLaunch w = make(ri, split, n_first[ri]);
        w.vin = lv.alt;
        w.vout = lv.f[MG3D_U];
        w.i_lo = win[ri].lo + E;
        w.i_hi = win[ri].hi - E;
        const int n_in = k_sweep(D->rs[ri].coarse->opt, w, D->stream);
        if (n_in <= 0)
            return fail(MG3D_ERR_STATE, "slab sweep: no kernel for the interior window of %s on level %d", what, l);
        done(ri, n_first[ri], n_in);
    }
    return MG3D_OK;
}

/* ... where it ends with the top level's norm: the partial sums of a split launch go to the two halves of the rank's partials
 * and are folded edges first.  (Never with the prolongation: mg3d_stage_plan puts that on a launch before the norm's.) */
static int edge_first_norm(mg3d_dist *D, int l, int margin, int E, SweepKind kind, int S, int c1)
{
    auto make = [&](size_t ri, bool split, int n_edge) {
        SweepLaunch w = slab_sweep(D, ri, l);
        w.kind = kind;
        w.S = S;
        w.c1 = c1;
        w.partials = D->rs[ri].coarse->partials + (n_edge < 0 ? 0 : MG3D_MAX_PARTIALS / 2);
        w.max_partials = split ? MG3D_MAX_PARTIALS / 2 : MG3D_MAX_PARTIALS;
        return w;
    };
    auto fold = [&](size_t ri, int n_first, int n_in) {
        mg3d_ctx *cx = D->rs[ri].coarse;
        if (n_in)
            k_fold2(cx->partials, n_first, cx->partials + MG3D_MAX_PARTIALS / 2, n_in, cx->sumsq, D->stream);
        else
            k_fold(cx->partials, n_first, cx->sumsq, D->stream);
    };
    return edge_first(D, l, margin, E, kind == SWEEP_TAP ? "four passes + norm tap" : "colour passes + norm", make, fold);
}

/* One launch of a stage's list on distributed level l for every local rank, then the buffer swap (as mg3d_ctx.hip's
 * enqueue_stage_step).  zero_in: u is identically zero and not read; tgt / pro: where st.rst restricts to, st.pro prolongs from. */
static int slab_stage_step(mg3d_dist *D, int l, int post, int want_res, const StageStep &st, bool zero_in, const RestrictTarget *tgt,
                           const ProlongSource *pro)
{
    for (size_t ri = 0; ri < D->rs.size(); ri++) {
        SlabLevel &sl = SL(D, D->rs[ri], l);
        mg3d_ctx *cx = D->rs[ri].coarse;
        const bool rst = st.rst && tgt[ri].dc != nullptr;
        /* output planes of a smoothing launch: the owned planes plus what the next consumer reads beyond them -- the
         * residual/restriction behind a pre-smoother needs u on owned +-2, the top-level norm owned +-1; the remaining halo
         * planes are refreshed by an exchange before anything reads them again.  Only the LAST smoothing launch of the stage
         * may be trimmed: an earlier one feeds the next launch's whole dependence cone. */
        Window win = st.last ? slab_window(sl, post ? 1 : 2) : Window{0, sl.lv.g.ni};
        /* a pure residual launch (S == 0) only has to produce what is consumed: the norm and the on-the-fly restriction need
         * the owned planes (their neighbours come from the pipeline's warm-up / drain), a stored r one more on either side */
        if (st.S == 0)
            win = slab_window(sl, (want_res == 2 && !rst) ? 1 : 0);
        SweepLaunch w = slab_sweep(D, ri, l);
        w.kind = st.res ? SWEEP_PASSES_RES : SWEEP_PASSES;
        w.S = st.S;
        w.c1 = post ? 0 : 1;
        if (zero_in)
            w.vin = nullptr;
        if (st.res && want_res == 2 && !rst)
            w.r = sl.lv.f[MG3D_R];
        if (st.res && want_res == 1) /* the pre-smoothing norm is dropped (:1294) */
            w.partials = cx->partials;
        if (rst)
            restrict_into(w, tgt[ri]);
        if (st.pro)
            prolong_from(w, pro[ri]);
        w.i_lo = win.lo;
        w.i_hi = win.hi;
        const int np = k_sweep(cx->opt, w, D->stream);
        if (np < 0) /* nothing was launched: no buffer swap, no fold */
            return fail(MG3D_ERR_STATE, "slab sweep: no kernel for %d colour passes%s on level %d", st.S, st.res ? " + residual" : "", l);
        if (st.res && want_res == 1)
            k_fold(cx->partials, np, cx->sumsq, D->stream);
    }
    if (st.S > 0)
        swap_u_all(D, l);
    return MG3D_OK;
}

/* One smoothing stage on distributed level l for every local rank: iters x two colour passes, optional residual (want_res 2:
 * r stored or restricted on the fly into tgt[], 1: norm only, over OWNED planes, into the rank's coarse->sumsq[0]).  Same launch
 * policy as the single-domain path.  On entry the halos of u and d on this level are exact (H planes).  With want_res 1 (the
 * top level's post-smoother) the exchange of the u halos for the next cycle, planes 2..H, starts as soon as u is final: with
 * the last smoothing launch where that takes the norm (edge_first, E = the window's margin 1 + the plane skipped + the H - 1
 * sent), else before the pure residual launch (it reads owned +-1 only).
 * tgt: where the residual is restricted to (keep_r: a list of empty targets, see dist_stage_plan); pro: the correction the
 * first launch may fold in; zero_in (down-leg): u is identically zero, the first launch does not read it. */
static int stage_smooth(mg3d_dist *D, int l, int post, int want_res, const RestrictTarget *tgt, const ProlongSource *pro = nullptr,
                        bool zero_in = false)
{
    const StagePlan plan = dist_stage_plan(D, l, post, want_res, tgt != nullptr, pro != nullptr);
    for (int k = 0; mg3d_stage_launch(plan, k); k++) {
        const StageStep &st = *mg3d_stage_launch(plan, k);
        if (want_res == 1 && st.S == 0)
            CHK(start_u_exchange(D, MG3D_XK_HALO_U_NEXT, l));
        if (want_res == 1 && st.S > 0 && st.res)
            CHK(edge_first_norm(D, l, 1, D->H + 1, SWEEP_PASSES_RES, st.S, post ? 0 : 1));
        else
            CHK(slab_stage_step(D, l, post, want_res, st, zero_in && k == 0, tgt, pro));
    }
    return MG3D_OK;
}

/* the variable-coefficient operator on a rank's slab of a level (slabs: no boundary word, no mask) */
static LevelOperator slab_operator(const RankState &R, const SlabLevel &sl)
{
    return LevelOperator{mg3d_level_op(sl.lv.h, R.coarse->sigma), R.coarse->sigma, sl.eps, 0, nullptr};
}

/* One smoothing stage of the variable-coefficient operator (mg3d_kernels.hip) on distributed level l for every local rank: the
 * single-domain schedule (2*nu colour passes in place, then the residual) with windows.  On entry u, d and eps are exact on
 * every local plane.  Pass t of S = 2*nu produces the owned planes +- (margin + S - t), its dependence cone, and no more:
 * margin 2 before a stored residual, 1 before the top-level norm.  want_res 2: r on owned +-1, what the restriction reads
 * (its norm is dropped, :1294); 1: the exchange of planes 2..H of u for the next cycle starts, then the norm of the OWNED
 * planes into the rank's coarse->sumsq[0] -- it reads u on owned +-1, which the post-smoother made exact and the exchange
 * does not touch (the halo planes still hold stale values: the norm window keeps them out); 0: passes only. */
static int dist_coef_smooth(mg3d_dist *D, int l, int post, int want_res)
{
    hipStream_t s = D->stream;
    const int S = 2 * D->nu, c1 = post ? 0 : 1, margin = want_res == 2 ? 2 : 1;
    for (auto &R : D->rs) {
        SlabLevel &sl = SL(D, R, l);
        Level &lv = sl.lv;
        mg3d_ctx *cx = R.coarse;
        const LevelOperator A = slab_operator(R, sl);
        for (int t = 1; t <= S; t++) { /* :1282 / :1341 */
            const int w = margin + S - t;
            k_smooth_color(lv.g, lv.f[MG3D_U], lv.f[MG3D_D], A, c1 ^ ((t - 1) & 1), s, sl.own_lo - w, sl.own_hi + w);
        }
        if (want_res == 2) /* :1294 */
            k_residual(lv.g, lv.f[MG3D_U], lv.f[MG3D_D], A, lv.f[MG3D_R], cx->partials, cx->sumsq + cx->sumsq_slots - 1, s,
                       sl.own_lo - 1, sl.own_hi + 1, 0, 0);
    }
    if (want_res != 1)
        return MG3D_OK;
    CHK(start_u_exchange(D, MG3D_XK_HALO_U_NEXT, l));
    for (auto &R : D->rs) { /* :1354 */
        SlabLevel &sl = SL(D, R, l);
        k_residual(sl.lv.g, sl.lv.f[MG3D_U], sl.lv.f[MG3D_D], slab_operator(R, sl), nullptr, R.coarse->partials, R.coarse->sumsq, s,
                   sl.own_lo, sl.own_hi, sl.own_lo, sl.own_hi);
    }
    return MG3D_OK;
}

/* carried cycles on slabs (csrc/mg3d_ctx.hip has the argument): same conditions as the single-domain path */
static bool dist_carry_policy(mg3d_dist *D) /* what the options say (carry, carry_min), for this level geometry */
{
    return mg3d_run_ahead_policy(D->rs[0].coarse->opt, false, SL(D, D->rs[0], D->L - 1).lv.g.N);
}

/* one launch per leg on slabs (csrc/mg3d_ctx.hip "one launch per leg"; options legs, legs_min): same conditions as the carried
 * cycles, which it replaces where both apply */
static bool dist_legs_policy(mg3d_dist *D)
{
    return mg3d_run_ahead_policy(D->rs[0].coarse->opt, true, SL(D, D->rs[0], D->L - 1).lv.g.N);
}

static bool dist_can_legs(mg3d_dist *D)
{
    /* (legs_fixed: the ranks of a multi-process job agreed on the schedule at creation) */
    const mg3d_ctx *cx = D->rs[0].coarse;
    const Geom &g = SL(D, D->rs[0], D->L - 1).lv.g;
    return !D->coef && D->H >= 5 && mg3d_can_run_ahead(cx->opt, true, D->legs_fixed ? D->legs_on : -1, D->nu, cx->keep_r, g.N, g.nj);
}

static bool dist_can_carry(mg3d_dist *D)
{
    const mg3d_ctx *cx = D->rs[0].coarse;
    const Geom &g = SL(D, D->rs[0], D->L - 1).lv.g;
    return !D->coef && mg3d_can_run_ahead(cx->opt, false, D->carry_fixed ? D->carry_on : -1, D->nu, cx->keep_r, g.N, g.nj) &&
           dist_stage_plan(D, D->L - 1, 1, 1, false, true).step[0].pro; /* the split up-leg whose first launch the carried cycle keeps */
}

/* Down-leg of the finest level behind another cycle (its norm's black half rides along) or a finished one (red_in).
 * The down-leg as ONE launch over the owned planes: three passes (black first -- the cycle's first red pass is the
 * identity behind the previous cycle's last one), residual, restriction; it reads five planes either side, which
 * the previous cycle's last exchange refreshed.  On its way it forms the black half of the previous cycle's
 * residual norm, whose red half the one-launch up-leg left in partials[0 .. legs_npa): folded and reduced here. */
static int dist_down_leg_ahead(mg3d_dist *D, int l, const RestrictTarget *tgt, bool red_in, int slot)
{
    for (size_t ri = 0; ri < D->rs.size(); ri++) {
        RankState &R = D->rs[ri];
        SlabLevel &sl = SL(D, R, l);
        mg3d_ctx *cx = R.coarse;
        SweepLaunch w = slab_sweep(D, ri, l);
        w.kind = SWEEP_LEG_DOWN;
        w.S = 3;
        w.partials = red_in ? nullptr : cx->partials + MG3D_MAX_PARTIALS / 2;
        w.max_partials = MG3D_MAX_PARTIALS / 2;
        restrict_into(w, tgt[ri]);
        const int npb = k_sweep(cx->opt, w, D->stream);
        if (npb <= 0)
            return fail(MG3D_ERR_STATE, "slab sweep: no kernel for the one-launch down-leg on level %d", l);
        if (!red_in)
            k_fold2(cx->partials, R.legs_npa, w.partials, npb, cx->sumsq, D->stream);
        swap_u(sl.lv);
    }
    if (!red_in)
        CHK(reduce_norm(D, slot - 1));
    return MG3D_OK;
}

/* Down-leg of the finest level behind a carried cycle: the one pre-smoothing pass that is left (black) + residual +
 * restriction in one launch over the owned planes: it reads three planes either side, which the previous cycle's last
 * exchange refreshed */
static int dist_down_leg_carried(mg3d_dist *D, int l, const RestrictTarget *tgt)
{
    for (size_t ri = 0; ri < D->rs.size(); ri++) {
        SlabLevel &sl = SL(D, D->rs[ri], l);
        SweepLaunch w = slab_sweep(D, ri, l);
        w.kind = SWEEP_PASSES_RES;
        w.S = 1;
        w.c1 = 0;
        restrict_into(w, tgt[ri]);
        if (k_sweep(D->rs[ri].coarse->opt, w, D->stream) < 0)
            return fail(MG3D_ERR_STATE, "slab sweep: no kernel for one pass + residual + restriction on level %d", l);
        swap_u(sl.lv);
    }
    return MG3D_OK;
}

/* Up-leg of the finest level as ONE launch: prolongation + four passes over the owned planes (it uses up four of the H halo
 * planes of u and of the correction), the red half of the norm from the last pass's own sums.  The first and last five planes
 * are what the exchange for the next down-leg sends (edge_first).  The sums of a split launch lie one behind the other in
 * partials[0 .. legs_npa), unfolded: the next cycle's down-leg folds them with its black half (dist_down_leg_ahead). */
static int dist_up_leg_legs(mg3d_dist *D, int l, const ProlongSource *pro)
{
    auto up = [&](size_t ri, bool, int n_edge) {
        SweepLaunch w = slab_sweep(D, ri, l);
        w.kind = SWEEP_LEG_UP;
        w.partials = D->rs[ri].coarse->partials + (n_edge < 0 ? 0 : n_edge);
        w.max_partials = n_edge < 0 ? MG3D_MAX_PARTIALS / 4 : MG3D_MAX_PARTIALS / 2 - n_edge;
        prolong_from(w, pro[ri]);
        return w;
    };
    CHK(edge_first(D, l, 0, 5, "the one-launch up-leg", up, [&](size_t ri, int n1, int n2) { D->rs[ri].legs_npa = n1 + n2; }));
    D->legs_pending = true;
    D->n_legs++;
    return MG3D_OK;
}

/* Up-leg of the finest level of a cycle that carries into the next one (as mg3d_ctx.hip's up_leg_carried): the first launch of
 * the split post-smoothing stage -- prolongation + two passes, on every local plane -- then four passes with the norm tapped
 * after the second: black, red (:1341, second half) <norm, :1354> black, red (:1282 of the next cycle, its first red pass
 * being the identity).  The tap launch makes the owned planes only: its passes use up the halo planes the first launch has
 * left, and dist_down_leg_carried gets three fresh ones by exchange first (E = 0 + 0 + 3). */
static int dist_up_leg_carried(mg3d_dist *D, int l, const ProlongSource *pro)
{
    const StagePlan split = dist_stage_plan(D, l, 1, 1, false, true);
    CHK(slab_stage_step(D, l, 1, 1, split.step[0], false, nullptr, pro));
    CHK(edge_first_norm(D, l, 0, 3, SWEEP_TAP, 4, 0));
    D->carried = true;
    D->n_carried++;
    return MG3D_OK;
}

static int dist_refuse_poisoned(const mg3d_dist *D, const char *who)
{
    if (D->poisoned)
        return fail(MG3D_ERR_STATE, "%s: an earlier mg3d_dist_vcycles call failed after one of its cycles had run ahead into the "
                                    "next: u of the finest level is mid-cycle; upload it again first", who);
    return MG3D_OK;
}

/* where each local rank's residual of distributed level l is restricted to: its slab of level l-1 or, below the last
 * distributed level, the rank's replicated context -- the owned coarse planes (plus the physical boundary planes at the ends
 * of the domain) */
static void restrict_targets(mg3d_dist *D, int l, RestrictTarget *tgt)
{
    for (size_t ri = 0; ri < D->rs.size(); ri++) {
        RankState &R = D->rs[ri];
        SlabLevel &sl = SL(D, R, l);
        if (l - 1 >= D->ld) {
            SlabLevel &sc = SL(D, R, l - 1);
            tgt[ri] = RestrictTarget{&sc.lv.g, sc.lv.f[MG3D_D], sc.own_lo, sc.own_hi};
        } else {
            Level &lc = R.coarse->lv[D->ld - 1];
            tgt[ri] = RestrictTarget{&lc.g, lc.f[MG3D_D], R.rank == 0 ? 0 : sl.glo / 2, R.rank == D->P - 1 ? lc.g.N : sl.ghi / 2};
        }
    }
}

/* Settles what the cycle is before its first launch: which run-ahead state it continues, which it may leave, and the
 * exchange plan that goes with the two.  carry_out / legs_out as asked for by dist_enqueue_vcycle. */
static int dist_begin_cycle(mg3d_dist *D, SlabCycle &c, int slot, bool carry_out, bool legs_out)
{
    D->phase = 0;
    c.slot = slot;
    c.can_legs = dist_can_legs(D);
    c.legs_in = D->legs_pending;
    c.can_carry = !c.can_legs && dist_can_carry(D);
    c.carry_in = D->carried;
    if ((c.carry_in && !c.can_carry) || (c.legs_in && (!c.can_legs || slot < 1))) {
        D->carried = false;
        D->legs_pending = false;
        return fail(MG3D_ERR_STATE, "mg3d_dist_vcycles: carried state met a cycle that cannot continue it");
    }
    c.carry_out = carry_out && c.can_carry;
    c.legs_out = legs_out && c.can_legs;
    D->cur = c.legs_out ? &D->plans_legs[c.legs_in ? 1 : 0] : c.legs_in ? &D->plans_legs[2] : c.carry_out ? &D->plans_carry : &D->plans;
    D->carried = false;
    D->legs_pending = false;
    c.red_in = !c.legs_in && !c.carry_in && c.can_legs && D->red_tail;
    D->red_tail = false;
    c.keep_r = D->rs[0].coarse->keep_r;
    return MG3D_OK;
}

/* Down-leg of distributed level l.  On entry the halos of d are exact (upload / the exchange behind the restriction above)
 * and those of u refreshed since it last changed (the finest level: upload, or the exchange the previous cycle ended with; below
 * it u is the zero guess, mg_3d.h:1258, folded into the first sweep launch).  tgt is filled here; none: a list of empty targets. */
static int dist_down_leg(mg3d_dist *D, const SlabCycle &c, int l, RestrictTarget *tgt, const RestrictTarget *none)
{
    const bool top = l == D->L - 1;
    restrict_targets(D, l, tgt);
    CHK(await_u(D, l));
    if (top && (c.legs_in || c.red_in))
        CHK(dist_down_leg_ahead(D, l, tgt, c.red_in, c.slot));
    else if (top && c.carry_in)
        CHK(dist_down_leg_carried(D, l, tgt));
    else if (D->coef) {
        /* variable coefficient: zero guess below the finest level (:1258) on every local plane, passes, r stored */
        if (!top)
            for (auto &R : D->rs)
                (void)hipMemsetAsync(SL(D, R, l).lv.f[MG3D_U], 0, SL(D, R, l).lv.elems * sizeof(double), D->stream);
        CHK(dist_coef_smooth(D, l, 0, 2));
    } else /* :1282 + :1294 + :1310 (interior of the coarse rhs on the fly unless r is to be kept) */
        CHK(stage_smooth(D, l, 0, 2, c.keep_r ? none : tgt, nullptr, !top));
    for (size_t ri = 0; ri < D->rs.size(); ri++) {
        SlabLevel &sl = SL(D, D->rs[ri], l);
        k_restrict(sl.lv.g, sl.lv.f[MG3D_R], *tgt[ri].gc, tgt[ri].dc, 0, D->stream, tgt[ri].lo, tgt[ri].hi, !c.keep_r && !D->coef);
    }
    /* the coarser level starts from its right-hand side at once: only owned planes were produced */
    if (l - 1 < D->ld)
        CHK(exchange(D, (D->policy & 1) ? MG3D_XK_RHS_GATHER : MG3D_XK_RHS_ALLGATHER, D->ld - 1, false));
    else
        CHK(exchange(D, MG3D_XK_HALO_D, l - 1, false));
    /* u of this level is final until the prolongation on the way up: refresh its halos underneath the
     * coarser levels (issued behind the right-hand side's exchange: one communicator, one in-order stream) */
    return start_u_exchange(D, MG3D_XK_HALO_U_DOWN, l);
}

/* The replicated levels: the ordinary V-cycle from level ld-1 (its guess zeroed first, :1258), on every rank -- or,
 * with MG3D_COARSE_GATHER=1, on rank 0 alone, whose correction is then broadcast (same bits either way: the ranks
 * would have computed identical copies) */
static int dist_replicated_levels(mg3d_dist *D)
{
    const int lc_top = D->ld - 1;
    {
        DistScope timer(D, 3, D->stream);
        for (auto &R : D->rs) {
            if ((D->policy & 1) && R.rank != 0)
                continue;
            Level &lc = R.coarse->lv[lc_top];
            (void)hipMemsetAsync(lc.f[MG3D_U], 0, lc.elems * sizeof(double), D->stream);
            R.coarse->red_tail = false; /* u and d of the context's top level were rewritten behind its back (here; the restriction) */
            mg3d_ctx_touched(R.coarse, MG3D_D, lc_top); /* ... by kernels: its zero map is void (the slab path takes none) */
            if (lc_top == 0)
                CHK(mg3d_coarse_solve(R.coarse));
            else
                CHK(mg3d_enqueue_vcycle(R.coarse, lc_top, R.coarse->sumsq_slots - 1));
        }
    }
    if (D->policy & 1)
        CHK(exchange(D, MG3D_XK_CORR_BCAST, lc_top, false));
    return MG3D_OK;
}

/* Up-leg of distributed level l: prolongation (:1331) on every local plane, halos included -- the correction's halos
 * (post-smoothed on owned +-1 only) are refreshed first, those of u have been under way since the pre-smoother -- then the
 * post-smoother and, on the finest level, the norm (:1341, :1354): all H halo planes of u are exact here, the post-smoother
 * uses up 2*nu of them.  The next cycle's pre-smoother wants fresh halos on the finest u: that exchange starts underneath the
 * norm, which reads the first halo plane on either side -- the post-smoother made it exact, the exchange leaves it alone. */
static int dist_up_leg(mg3d_dist *D, const SlabCycle &c, int l)
{
    const bool top = l == D->L - 1;
    if (l - 1 >= D->ld)
        CHK(exchange(D, MG3D_XK_HALO_U_UP, l - 1, false));
    CHK(await_u(D, l));
    const int want = top ? 1 : 0;
    /* the prolongation rides on the post-smoother's first launch: the top level's split stage, and (option fuse_up_max, as
     * on a single domain) the four-pass launch of a V(2,2) cycle on the levels below it */
    const bool fold = !D->coef && dist_stage_plan(D, l, 1, want, false, true).step[0].pro;
    std::vector<ProlongSource> pro(D->rs.size());
    for (size_t ri = 0; ri < D->rs.size(); ri++) {
        RankState &R = D->rs[ri];
        SlabLevel &sl = SL(D, R, l);
        Level &lc = l - 1 >= D->ld ? SL(D, R, l - 1).lv : R.coarse->lv[D->ld - 1];
        pro[ri] = ProlongSource{&lc.g, lc.f[MG3D_U]};
        if (!fold)
            k_prolong(lc.g, lc.f[MG3D_U], sl.lv.g, sl.lv.f[MG3D_U], 0, D->stream, 0, sl.lv.g.ni);
    }
    if (top && c.legs_out)
        return dist_up_leg_legs(D, l, pro.data());
    if (D->coef)
        return dist_coef_smooth(D, l, 1, want);
    if (top && c.carry_out)
        return dist_up_leg_carried(D, l, pro.data());
    return stage_smooth(D, l, 1, want, nullptr, fold ? pro.data() : nullptr);
}

/* One V-cycle: the distributed levels down, the replicated levels, the distributed levels up, the norm.
 * carry_out: another cycle of this call follows (it may be enqueued ahead into); legs_out: it follows in the same batch of norm
 * slots (its down-leg completes this cycle's norm into slot `slot`, which the batch then reads back) */
static int dist_enqueue_vcycle(mg3d_dist *D, int slot, bool carry_out = false, bool legs_out = false)
{
    SlabCycle c;
    CHK(dist_begin_cycle(D, c, slot, carry_out, legs_out));
    DistScope cycle_timer(D, 0, D->stream);
    if (D->timing)
        D->t_cycles++;
    for (auto &R : D->rs)
        if (!R.coarse->have_lu)
            return fail(MG3D_ERR_STATE, "mg3d_dist_vcycles: no coarse LU set (mg3d_dist_build_coarse)");
    std::vector<RestrictTarget> tgt(D->rs.size()), none(D->rs.size(), RestrictTarget{nullptr, nullptr, -1, -1});
    for (int l = D->L - 1; l >= D->ld; l--)
        CHK(dist_down_leg(D, c, l, tgt.data(), none.data()));
    CHK(dist_replicated_levels(D));
    for (int l = D->ld; l < D->L; l++)
        CHK(dist_up_leg(D, c, l));
    if (!c.legs_out)
        CHK(reduce_norm(D, slot));
    /* a whole V(2,2) cycle has ended the ordinary way: its last pass was red, the exchange behind it leaves all H halo planes
     * of u exact (plain plan: planes 2..H by exchange, plane 1 as the post-smoother made it) */
    if (!c.legs_out && !c.carry_out && D->nu == 2 && !D->coef)
        D->red_tail = true;
    if (D->phase != (int)(*D->cur)[0].kind.size())
        return fail(MG3D_ERR_STATE, "slab schedule ended after %d of the plan's %d phases", D->phase, (int)(*D->cur)[0].kind.size());
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(MG3D_ERR_HIP, "mg3d_dist_vcycles: kernel launch failed: %s", hipGetErrorString(e));
    return MG3D_OK;
}

extern "C" int mg3d_dist_vcycles(mg3d_dist *D, int count, double *norms)
{
    if (!D || count < 0)
        return fail(MG3D_ERR_ARG, "mg3d_dist_vcycles: bad arguments");
    CHK(dist_refuse_poisoned(D, "mg3d_dist_vcycles"));
    const int carried_before = D->n_carried;
    /* any error return below: if a cycle of this call has carried, u of the finest level may be three passes into a cycle
     * that was never finished (also across a batch boundary, where D->carried is still set) -- see `poisoned` */
    struct Guard {
        mg3d_dist *d;
        int before;
        bool ok;
        ~Guard()
        {
            if (!ok && (d->carried || d->n_carried != before))
                d->poisoned = true;
            if (!ok)
                d->carried = false, d->legs_pending = false, d->red_tail = false; /* (a half-formed norm is simply lost: u itself is a finished cycle's) */
        }
    } guard{D, carried_before, false};
    for (int done = 0; done < count;) {
        const int nb = (count - done < D->norm_slots) ? count - done : D->norm_slots;
        for (int c = 0; c < nb; c++) {
            /* every cycle but the last of a call ends ahead into the next one (a call never ends in the carried state) */
            CHK(dist_enqueue_vcycle(D, c, done + c + 1 < count, c + 1 < nb));
        }
        CHK(await_u(D, D->L - 1)); /* the compute stream joins the exchange of the finest u halos that the last cycle started */
        HIPCHK(hipMemcpyAsync(D->h_norms, D->d_norms, nb * sizeof(double), hipMemcpyDeviceToHost, D->stream));
        HIPCHK(hipStreamSynchronize(D->stream));
        HIPCHK(hipStreamSynchronize(D->comm_stream));
        dist_resolve_timers(D);
        /* an RCCL failure that surfaced asynchronously (a peer died, a transport error): an error here, not a hang or a
         * wrong number later */
        if (D->have_comm && D->comm) {
            ncclResult_t ae = ncclSuccess;
            NCCLCHK(ncclCommGetAsyncError(D->comm, &ae));
            if (ae != ncclSuccess)
                return fail(MG3D_ERR_HIP, "RCCL reported an asynchronous error: %s", ncclGetErrorString(ae));
        }
        if (norms)
            for (int c = 0; c < nb; c++)
                norms[done + c] = sqrt(D->h_norms[c]);
        done += nb;
    }
    guard.ok = true;
    return MG3D_OK;
}
