/* mg3d_internal.h -- shared between mg3d_ctx.hip and mg3d_kernels.hip (not installed). */
#ifndef MG3D_INTERNAL_H
#define MG3D_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stddef.h>

#include "mg3d.h"

/* Geometry of one (local) level as the kernels see it.
 * Device layout: idx = plane*i + pitch*j + k, pitch % 16 == 0 (128-byte rows),
 * plane = pitch*nj.  A single-GPU level has ni = nj = nk = N and ig0 = 0; an
 * i-slab of a distributed level has ni = owned planes + 2 (halo or physical
 * boundary on either side) and ig0 = global index of its local plane 0. */
struct Geom {
    int ni, nj, nk;
    int pitch;
    long long plane;
    int ig0; /* global i of local plane 0 (colour parity, grid-transfer alignment) */
    int N;   /* global points per side */
};

static inline int mg3d_pitch_for(int nk) { return (nk + 15) & ~15; }

/* The constants of one level's operator, the screened 7-point Laplacian  Delta_h u - sigma u = d  (sigma >= 0, set per
 * context by mg3d_ctx_set_shift; 0 is the reference's Poisson operator):
 *   smoother  v = sixth * (((((((up + dn) + jm) + jp) + km) + kp) - hSq*d)          (mg_3d.h:438-443)
 *   residual  diff = d - invHsq * (sum - dg*v)                                       (mg_3d.h:819-821)
 * With sigma = 0 every constant is the reference's own double: dg = 6 + 0*hSq = 6, sixth = 1./6, invHsq = 1./(h*h). */
struct LevelOp {
    double hSq, sixth, invHsq, dg;
};
static inline LevelOp mg3d_level_op(double h, double sigma)
{
    LevelOp op;
    op.hSq = h * h;             /* mg_3d.h:644 */
    op.dg = 6 + sigma * op.hSq; /* the diagonal times h^2 */
    op.sixth = 1. / op.dg;      /* mg_3d.h:646 */
    op.invHsq = 1. / op.hSq;    /* mg_3d.h:797 */
    return op;
}

struct LuBand {
    int n;        /* unknowns */
    int bw;       /* half bandwidth actually populated (max |i-j| with LU[i][j] != 0) */
    double *lcol; /* [n][bw]  lcol[j*bw+t] = LU[j+1+t][j]   (strictly lower, by column) */
    double *ucol; /* [n][bw]  ucol[j*bw+t] = LU[j-1-t][j]   (strictly upper, by column) */
    int npad;     /* n rounded up to a multiple of 64 (identity rows appended) */
    double *diag; /* [2*npad]: the diagonal, then RN(1/diagonal); 1 on the padding */
    int fast_div; /* every diagonal entry lies in lu_div()'s safe window: the reciprocals may be used */
    /* lane-rotated copies for the single-wave solve (bw <= 64*rot_r): entry [j][64*q + l] is the
     * factor of the row lane l accumulates at step j: forward row j+1+((l-j-1)&63)+64q, backward row
     * j-1-((j-1-l)&63)-64q; zero outside the band / matrix */
    int rot_r;    /* 0 when not built */
    double *lrot; /* [n][64*rot_r] */
    double *urot; /* [n][64*rot_r] */
    /* the same factors as ONE stream in the order the streamed solve consumes them: 2*npad/64 chunks of 64
     * steps (forward steps j = 0..npad-1, then backward steps j = npad-1..0) plus two spare chunks the
     * loaders may over-read; a step is 64 lanes x rot_r doubles, [lane][q] */
    int stream_ch; /* 64 when built, else 0 */
    double *stream;
    /* full factor only, when a reduced factor (the system without its identity rows) exists beside it: index of
     * unknown p in the reduced system, -1 for an identity row (mg3d_ctx.hip, install_lu) */
    int *in_map;
};

#define MG3D_MAX_PARTIALS 32768

/* Launch and schedule policy of ONE context: defaults, then the environment as an override read once when the context
 * is created (mg3d_options_init), afterwards only mg3d_ctx_set_option / mg3d_dist_set_option / mg3d32_set_option.
 * Nothing on a launch path reads the environment; two contexts of one process may differ.  Keys and environment names:
 * kOptionTable in mg3d_ctx.hip, the table in INTEGRATION.md. */
enum {
    MG3D_OPT_CARRY = 0,    /* consecutive V(2,2) cycles share a launch on the finest level ("carried cycles") */
    MG3D_OPT_CARRY_MIN,    /* ... from this many points per side (130) */
    MG3D_OPT_LEGS,         /* one launch per leg on the finest level instead (round 4; 1) */
    MG3D_OPT_LEGS_MIN,     /* ... from this many points per side (160: at 129^3 the carried cycles are 6 % faster, from 193^3 the legs win 3 - 24 %) */
    MG3D_OPT_TINY,         /* the level above the coarsest one in one workgroup */
    MG3D_OPT_TINY_CYCLE,   /* ... together with the direct solve in ONE launch */
    MG3D_OPT_LU_REDUCED,   /* install the factor without its identity rows beside the full one */
    MG3D_OPT_FUSE_RST2,    /* two passes + residual + restriction as one launch: -1 from 130 points per side, 0 never, 1 always */
    MG3D_OPT_SMALL_MAX,    /* largest level side that runs the two-rows-per-thread shapes (129) */
    MG3D_OPT_FUSE_LEG_MAX, /* largest level side whose legs run as one (two-row) launch each (0) */
    MG3D_OPT_FUSE_UP_MAX,  /* largest level side whose up-leg folds the prolongation into a four-pass launch (0) */
    MG3D_OPT_SWEEP_TUNE,   /* first-use measurement of chunk lengths: -1 on unless a multi-rank job, 0 off, 1 on */
    MG3D_OPT_SWEEP_TUNE_LOG,
    MG3D_OPT_SWEEP_CI,     /* > 0: planes per chunk of every fused sweep launch (measurement only) */
    MG3D_OPT_SWEEP_RJ,     /* > 0: another compiled tile shape (rows per thread, waves, planes in flight); unknown ones */
    MG3D_OPT_SWEEP_NW,     /*      fall back to the default */
    MG3D_OPT_SWEEP_PF,
    MG3D_OPT_D_ZERO_SKIP,  /* the planes of the top level's d that are +0.0 at every interior point are not read (the zero map, mg3d_ctx.h): 0 off, 1 the map and, when it is full, the leg kernels without d (default), 2 the map only */
    MG3D_OPT_ZERO_FRONT,   /* the four-pass launch from the zero guess (a coarse level's pre-smoother) forms its first pass from d as the plane arrives and runs a three-pass kernel (ZF, mg3d_sweep_kernel.h): 1 (default), 0 the four-pass kernel on an input that is not read */
    MG3D_OPT_FUSE_DOWN_MIN, /* smallest level side whose V(2,2) pre-smoother from the zero guess, residual and restriction run as ONE launch behind the zero front (130; 0 never; needs zero_front, never at or below fuse_leg_max) */
    MG3D_OPT_COUNT
};
struct mg3d_options {
    int v[MG3D_OPT_COUNT];
};
void mg3d_options_init(mg3d_options *o);          /* defaults + environment */
int mg3d_option_index(const char *key);           /* -1: no such key */
const char *mg3d_option_key(int index);           /* NULL past the end */

/* One level's operator as the stencil launchers take it: the constants op; sigma, the context's shift; e, eps of the level
 * in the padded layout for div(eps grad u) - sigma u (mg3d_ctx_set_coefficient), NULL for the constant operator of op; bc,
 * the boundary word mg3d_bc(periodic, neumann): the MG3D_PERIODIC_* mask of wrapped axes (mg3d_ctx_set_periodic), whose
 * duplicate points receive copies, and above it the MG3D_NEUMANN_* mask of reflected faces (mg3d_ctx_set_neumann), whose
 * points are unknowns; m, the level's fixed-point bytes in the padded layout (mg3d_ctx_set_mask), NULL for none -- the
 * colour pass skips a fixed point, the residual is 0. there, apply_dot's q is 0. there.  bc and m are nonzero on
 * single-domain levels only, which take no windows; s, the level's screening field in the padded layout
 * (mg3d_ctx_set_shift_field), NULL for none -- div(eps grad u) - (sigma + s) u, with e set (the eps kernels alone have the
 * form: a context without eps gives them eps = 1 at every point); k_smooth_color, k_residual, k_pcg_apply_dot and k_step_rhs
 * take it, the field output does not look at it.  A context's level: mg3d_level_operator (mg3d_ctx.h). */
struct LevelOperator {
    LevelOp op;
    double sigma;
    const double *e;
    int bc;
    const unsigned char *m;
    const double *s;
};
static inline int mg3d_bc(int periodic, int neumann) { return periodic | neumann << 3; }

/* launchers (mg3d_kernels.hip); all asynchronous on `s` */
/* One colour pass in place and the residual of a level's operator A.  The residual writes res (optional) on the interior
 * and partials (one per block), then reduces them, in a fixed order, into *sumsq_out.  Windows as k_sweep's: i_lo / i_hi
 * the local planes produced, acc_lo / acc_hi those entering the norm; -1 / -1 every plane (a single-domain level) */
void k_smooth_color(const Geom &g, double *v, const double *d, const LevelOperator &A, int color, hipStream_t s,
                    int i_lo = -1, int i_hi = -1);
void k_residual(const Geom &g, const double *v, const double *d, const LevelOperator &A, double *res, double *partials,
                double *sumsq_out, hipStream_t s, int i_lo = -1, int i_hi = -1, int acc_lo = 0, int acc_hi = -1);
void k_sumsq(const Geom &g, const double *a, double *partials, double *sumsq_out, hipStream_t s);
/* The vector passes of mg3d_pcg_solve and mg3d_wpcg_solve on a single-domain level, bc the boundary word.  Each
 * touches the unknowns alone, the set the residual counts; sums are per-block partials folded in a fixed order into one
 * device double.  Scalars are read from device memory.  Return value: the number of partials (0: none needed), -1 when the
 * level has no launch shape.  k_pcg_dot and k_pcg_direction take periodic axes only (no Neumann face).
 *   apply_dot   : q = A p (the operator of k_residual), *dot_out = sum of w*p*q, w = 1/2 per Neumann face
 *                 the point lies on (1 everywhere without one)
 *   update_norm : alpha = *rz / *pap; x += alpha p, r -= alpha q, *rr_out = sum of r*r; writes nothing unless both dots
 *                 are finite and negative (the operator is negative definite)
 *   dot         : *dot_out = sum of a*b
 *   direction   : beta = *rz_new / *rz_old; p = z + beta p */
int k_pcg_apply_dot(const Geom &g, const double *p, const LevelOperator &A, double *q, double *partials, double *dot_out,
                    hipStream_t s);
int k_pcg_update_norm(const Geom &g, int bc, double *x, double *r, const double *p, const double *q, const double *rz,
                      const double *pap, double *partials, double *rr_out, hipStream_t s);
int k_pcg_dot(const Geom &g, int bc, const double *a, const double *b, double *partials, double *dot_out, hipStream_t s);
int k_pcg_direction(const Geom &g, int bc, double *p, const double *z, const double *rz_new, const double *rz_old,
                    hipStream_t s);
/* mg3d_wpcg_solve's own passes, with the weight w above:
 *   wpcg_dot       : *dot_out = sum of w*a*b, *sum_out = sum of w*b, from one read; two runs of partials, half the cap each
 *   wpcg_direction : m = W > 0 ? *wsum / W : 0; beta = *rz_new / *rz_old; p = (z - m) + beta p; first: p = z - m
 *   wpcg_center    : r -= *wsum / W, *rr_out = sum of r*r
 *   weight_sum     : W = sum of w over the unknowns (a multiple of 1/8: exact) */
int k_wpcg_dot(const Geom &g, int bc, const double *a, const double *b, double *partials, double *dot_out, double *sum_out,
               hipStream_t s);
int k_wpcg_direction(const Geom &g, int bc, double *p, const double *z, const double *rz_new, const double *rz_old,
                     const double *wsum, double W, bool first, hipStream_t s);
int k_wpcg_center(const Geom &g, int bc, double *r, const double *wsum, double W, double *partials, double *rr_out,
                  hipStream_t s);
double k_wpcg_weight_sum(const Geom &g, int bc);
/* The right-hand side of one theta-step (mg3d_step_advance) on a single-domain level, at the unknowns only:
 *   d = -((a*u0 + c1*q) + b*src),  q = A u0 as apply_dot forms it (A.m is not looked at);  src NULL: no b*src term
 *   backward_euler: c1 = 0 and q is not computed -- d = -(a*u0 + b*src), a streaming pass
 * Return value: 0, or -1 when the level has no launch shape (nothing launched) */
int k_step_rhs(const Geom &g, const double *u0, const double *src, const LevelOperator &A, double a, double c1, double b,
               bool backward_euler, double *d, hipStream_t s);
/* The nonlinear term of mg3d_nl_residual / mg3d_nl_solve on a single-domain level (formulas at the kernels):
 *   k_nl_eval  : F = d - (A v - gp*phi(w)) and sf = gp*beta*phi'(w) at the unknowns, w = beta*(v - uref), gp = g0*gw[p] or g0
 *                (gw NULL), phi by kind (MG3D_NL_EXP, MG3D_NL_SINH); A is the operator WITHOUT a screening field (A.s NULL).
 *                F (NULL: not stored) also at the duplicates, sf (NULL: not wanted) at the unknowns only, both 0. at fixed
 *                points; *sumsq_out = the sum of F^2 through partials and k_fold, residual_kernel's order; with sf,
 *                *bad += the number of sf that are not finite (the caller zeroes it).  Return value: the number of partials
 *                (0: no unknowns, *sumsq_out = 0), -1 when the level has no launch shape or A has a field: nothing launched
 *   k_nl_trial : t = x + lambda*dl at the unknowns and their duplicates, t = x at the fixed points of m (NULL: no mask);
 *                Dirichlet points of t are not written.  0, or -1: no launch shape */
int k_nl_eval(const Geom &g, const double *v, const double *d, const LevelOperator &A, int kind, const double *gw, double g0,
              double beta, double uref, double *F, double *sf, double *partials, double *sumsq_out, unsigned long long *bad,
              hipStream_t s);
int k_nl_trial(const Geom &g, int bc, const double *x, const double *dl, double lambda, double *t, const unsigned char *m,
               hipStream_t s);
/* The grid transfers.  bc = 0: ic_lo/ic_hi, if_lo/if_hi: local plane range to produce; -1 = every local plane that is not
 * a slab halo.  bc = mg3d_bc(periodic, neumann) != 0 (single-domain levels): every plane, full weighting on periodic and
 * Neumann faces too, duplicates written with their sources; the window and faces_only are not looked at */
void k_restrict(const Geom &gf, const double *r, const Geom &gc, double *dc, int bc, hipStream_t s, int ic_lo = -1,
                int ic_hi = -1, bool faces_only = false /* injection on the coarse faces only */,
                const unsigned char *mf = nullptr /* the fine level's fixed points (single-domain levels, any bc): 0. in place of r there */);
void k_prolong(const Geom &gc, const double *ec, const Geom &gf, double *ef, int bc, hipStream_t s, int if_lo = -1,
               int if_hi = -1, const unsigned char *mf = nullptr /* the fine level's fixed points: the point form, skipping them */);
/* BCFunc(i*h, j*h, k*h) = x*x - 2*y*y + z*z on the six faces of a field (mg_3d.h:89-90, 1147-1239) */
void k_fill_boundary(const Geom &g, double *v, double h, hipStream_t s);
/* The zero map of a right-hand side: one bit per plane of a single-domain level, 32 planes a word; bit i set = every
 * interior point of plane i (1 <= j <= nj-2, 1 <= k <= nk-2) has the bit pattern of +0.0 -- -0.0, denormals and NaNs count
 * as non-zero --, never set for planes 0 and ni-1.  k_dzero_scan: the map of d, one pass over it; k_dzero_fill: every
 * interior plane's bit, the map of a d that was just zeroed */
__host__ __device__ static inline int mg3d_dzero_words(int ni) { return (ni + 31) / 32; }
void k_dzero_scan(const Geom &g, const double *d, unsigned *map, hipStream_t s);
void k_dzero_fill(const Geom &g, unsigned *map, hipStream_t s);
/* folds np per-block partial sums, in a fixed order, into *out */
void k_fold(const double *partials, int np, double *out, hipStream_t s);
/* the same over two runs of partial sums (a norm whose halves two launches formed): *out = fold(pa) + fold(pb) */
void k_fold2(const double *pa, int na, const double *pb, int nb, double *out, hipStream_t s);
/* fused sweep (mg3d_sweep.hip).  Everything ONE launch can be asked to do is a field of SweepLaunch: a call site sets the
 * fields it uses, the rest keep their defaults, and k_sweep alone resolves "-1 = all". */
void k_sweep_set_tune_default(int on); /* first-use chunk measurement on / off where the option says -1 */
bool k_sweep_fuse_rst2(const mg3d_options &o, int N); /* two passes + residual + restriction as ONE launch on a level of N points per side */
enum SweepKind {
    SWEEP_PASSES,     /* S colour passes starting with colour c1, from vin into vout (vout != vin) */
    SWEEP_PASSES_RES, /* ... then the residual of the result (S = 0: the residual alone, vout ignored): r receives it on the
                         interior, partials one sum of diff^2 per block; with a restriction target (S = 0, 1, 2 or 4) neither */
    SWEEP_TAP,        /* FOUR passes starting with colour c1 and, into partials, the residual norm of the state after the
                         SECOND one: the launch that ends one V-cycle -- its last two post-smoothing passes and its norm --
                         and begins the next (mg3d_ctx.hip, "carried cycles") */
    SWEEP_LEG_DOWN,   /* one launch per leg of a V(2,2) cycle (mg3d_sweep.hip, "one launch per leg"): S = 3 passes black first
                         (behind another cycle) + residual + restriction into dc; partials: the sum of diff^2 of the INCOMING
                         state over the colour the first pass updates */
    SWEEP_LEG_UP      /* ... the input is vin + P(ec), four passes black first; partials: the sum of diff^2 of the RESULT over
                         the colour the last pass updated.  (The legs set c1 themselves and never measure chunk lengths.) */
};
/* What k_sweep launched, written on the host when it launches (mg3d_ctx_sweep_taken, include/mg3d.h: the same order as
 * MG3D_SWEEP_TAKEN_*): the template arguments of the kernel, whether the instantiation that reads d through its zero map
 * ran (DZ), the chunk length, the grid and its block numbering, the tiling, and the level's points per side. */
struct SweepTaken {
    int S, RES, RJ, NW, PF, ND, DZ, CI, blocks, xcd_remap, ntj, ntk, PRO, RST, DP, TAP, N;
};
/* the launches of one context, by kind: the distinct records, the most recent one first, each with the number of launches
 * it stands for; at most MG3D_SWEEP_TAKEN_KEEP of a kind (the one used longest ago goes), `launches` counts them all */
#define MG3D_SWEEP_KINDS 5
#define MG3D_SWEEP_TAKEN_KEEP 32
struct SweepTakenLog {
    struct Entry {
        SweepTaken t;
        unsigned long long count;
    };
    Entry e[MG3D_SWEEP_KINDS][MG3D_SWEEP_TAKEN_KEEP];
    int n[MG3D_SWEEP_KINDS];
    unsigned long long launches[MG3D_SWEEP_KINDS];
};
struct SweepLaunch {
    /* optional: where k_sweep records the launch it takes (nothing when it launches nothing); host side only */
    SweepTakenLog *taken = nullptr;
    /* the level: its local geometry, operator constants and arrays */
    const Geom *g = nullptr;
    LevelOp op = {};
    const double *vin = nullptr; /* NULL: identically zero, not read (the zero guess of a coarser level) */
    const double *d = nullptr;
    /* optional: the zero map of d (k_dzero_scan), bit i set = plane i of d is +0.0 at every interior point and is not read.
     * Single-domain levels with Dirichlet faces only: there no face entry of d enters a stored value */
    const unsigned *d_zero = nullptr;
    /* optional: d is +0.0 at EVERY interior point (the map is full).  A launch that has a kernel without d (the legs) takes it
     * and then looks at neither d nor the map; every other launch goes by d_zero as before.  d_none_taken, if given, is
     * incremented by one for a launch that took such a kernel */
    bool d_none = false;
    unsigned long long *d_none_taken = nullptr;
    double *vout = nullptr;
    /* what the launch does */
    SweepKind kind = SWEEP_PASSES;
    int S = 0;  /* colour passes (SWEEP_TAP and SWEEP_LEG_UP: always four) */
    int c1 = 1; /* colour of the first pass: 1 red, 0 black */
    double *r = nullptr;
    double *partials = nullptr;
    int max_partials = MG3D_MAX_PARTIALS; /* room in partials */
    /* optional: also restrict the residual (full weighting) into the interior of the coarse right-hand side dc, local
     * coarse planes [ic_lo, ic_hi), -1 / -1 all of them; r then never travels to memory */
    const Geom *gc = nullptr;
    double *dc = nullptr;
    int ic_lo = -1, ic_hi = -1;
    /* optional: the input is vin + P(ec), the trilinear prolongation of the coarse field ec (smoothing-only launches black
     * first, S = 2 or 4; SWEEP_LEG_UP) */
    const Geom *gce = nullptr;
    const double *ec = nullptr;
    /* window: [i_lo, i_hi) the local output planes of this launch, -1 / -1 all -- several launches with disjoint windows
     * and the same vin / vout make up one sweep (overlap with halo exchange); [acc_lo, acc_hi) the local planes entering
     * the norm, 0 / -1 all; edge > 0: only the first and the last `edge` planes of [i_lo, i_hi), as one launch of two chunks
     * (-1 when the range is shorter than 2 * edge): the planes a halo exchange sends first, the interior in a second launch */
    int i_lo = -1, i_hi = -1, acc_lo = 0, acc_hi = -1, edge = 0;
};
/* Returns the number of partials written (>= 0; 0 also for an empty window: nothing launched) or -1 when the request has no
 * instantiation: nothing was launched. */
int k_sweep(const mg3d_options &o, const SweepLaunch &w, hipStream_t s);

/* ---- the launches of ONE smoothing stage with the fused sweep: `iters` x two colour passes, optionally followed by the
 * residual of the result.  The single-domain path (mg3d_ctx.hip) and the slab path (mg3d_dist.hip) both run the list this
 * returns; questions about a stage ("does its first launch take the prolongation?") are asked of the same list. */
struct StageAsk {
    int N, nj;        /* of the level: global points per side, local rows */
    bool post;        /* post-smoother (black first) or pre-smoother */
    int iters;
    int want_res;     /* 0 none, 1 norm only, 2 r stored or restricted (+ norm) */
    bool has_coarse;  /* a restriction target exists: the residual may be restricted on the fly */
    bool need_norm;   /* the norm of the residual is wanted */
    bool pro_offered; /* a prolongation source is offered: the first launch may take u + P(e) as its input */
    bool leg4_form;   /* the single domain has the whole down-leg as one two-row launch (option fuse_leg_max); the slab path does not */
    bool zero_in;     /* the stage starts from the zero guess: its first launch has no input */
    bool down_form;   /* the single domain has the zero-guess down-leg as one launch behind the zero front (option fuse_down_min); the slab path keeps its launches */
};
struct StageStep {
    int S;      /* colour passes of the launch: 4, 2 or 0 (the residual alone) */
    int times;  /* how often the launch repeats (the leading four-pass launches of a long stage) */
    bool res;   /* carries the residual */
    bool rst;   /* ... restricted on the fly */
    bool pro;   /* takes the prolongation into its loads (the stage's first launch only) */
    bool last;  /* no colour pass follows it in this stage */
};
struct StagePlan {
    int n;
    StageStep step[3];
};
static inline StagePlan mg3d_stage_plan(const mg3d_options &o, const StageAsk &q)
{
    StagePlan p = {0, {}};
    /* Where the norm is wanted behind FOUR post-smoothing passes (the top level of a V(2,2) cycle) the stage
     * runs as 2 + 2 passes: the first launch takes the prolongation into its loads (the 2-pass shape has the
     * registers for it: 0.77 ms against 0.74 ms without), the second one the residual norm (0.90 ms) --
     * 1.67 ms instead of 0.56 (prolongation) + 0.82 (4 passes) + 0.47 (norm).  Below the top level no norm
     * is formed and prolongation + 4 passes in two launches stays cheaper. */
    const bool sp = q.post && 2 * q.iters == 4 && q.want_res == 1;
    /* The prolongation rides on a smoothing-only first launch: the 2-pass first launch of a split stage takes it almost for
     * free.  On a 4-pass first launch of a level above small_max it used to be SLOWER (the four-row shape spilt; round 2 measured
     * 1.48 ms against 0.85 + 0.56 at 513^3).  Since the prolongation is applied at the end of the step before (MG3D_PRO_LATE in
     * the kernel) that shape has 248 VGPRs and no scratch: the 257^3 level of the 513^3 problem takes 0.12 instead of
     * 0.058 + 0.112 ms, the cycle 2.18 -> 2.13 ms -- fuse_up_max now defaults to every level.  Small levels: the
     * two-rows-per-thread four-pass shape has the registers for it (k_sweep). */
    const int up_max = q.leg4_form && o.v[MG3D_OPT_FUSE_LEG_MAX] > o.v[MG3D_OPT_FUSE_UP_MAX] ? o.v[MG3D_OPT_FUSE_LEG_MAX]
                                                                                              : o.v[MG3D_OPT_FUSE_UP_MAX];
    const bool pro = q.pro_offered && q.post &&
                     (sp || (2 * q.iters == 4 && q.want_res == 0 && (q.nj & 1) != 0 && q.N <= up_max));
    int passes = 2 * q.iters;
    bool done_res = q.want_res == 0;
    while (passes > 0 || !done_res) {
        const int S = (sp && passes >= 2) ? 2 : passes >= 4 ? 4 : passes; /* 4, 2 or 0 */
        const bool last = passes - S == 0;
        /* small levels (<= fuse_leg_max points per side): the whole down-leg -- four passes, residual,
         * restriction -- as one launch of the two-rows-per-thread shape: it wastes three quarters of its rows
         * and saves a launch where launches are paid in latency, not in bytes */
        const bool leg4 = q.leg4_form && S == 4 && q.has_coarse && !q.need_norm && q.want_res != 0 && q.N <= o.v[MG3D_OPT_FUSE_LEG_MAX];
        /* the residual rides on a 2-pass launch; behind 4 passes it gets its own launch (the 5-stage
         * window leaves too few registers for a tile with a useful interior: measured 1.9 ms fused
         * against 0.85 + 0.76 ms split on a 513^3 level) */
        /* two passes + residual + restriction (the down-leg of V(1,1), the tail of V(3,3)'s): one launch from 130
         * points per side up, two below (k_sweep_fuse_rst2) */
        /* larger levels (>= fuse_down_min points per side) from the zero guess: the front forms the first red pass from d, three
         * passes, residual and restriction ride behind it in the four-row shape -- d is read once, u and the coarse d written
         * once, where four passes and then residual + restriction read d twice and u once more (k_sweep: S = 3, RES = 2) */
        const bool down = q.down_form && q.zero_in && !q.post && 2 * q.iters == 4 && passes == 4 && q.has_coarse && !q.need_norm &&
                          q.want_res != 0 && o.v[MG3D_OPT_ZERO_FRONT] != 0 && o.v[MG3D_OPT_FUSE_DOWN_MIN] > 0 &&
                          q.N >= o.v[MG3D_OPT_FUSE_DOWN_MIN] && q.N > o.v[MG3D_OPT_FUSE_LEG_MAX];
        const bool res = last && q.want_res != 0 && (S != 4 || leg4 || down) && !(S == 2 && q.has_coarse && !k_sweep_fuse_rst2(o, q.N));
        const StageStep st = {S, 1, res, res && q.has_coarse, pro && passes == 2 * q.iters, last};
        StageStep *prev = p.n ? &p.step[p.n - 1] : nullptr;
        if (prev && prev->S == S && !prev->res && !res && !prev->pro && prev->last == last)
            prev->times++; /* (the leading four-pass launches of a stage of more than two sweeps) */
        else if (p.n < 3)
            p.step[p.n++] = st;
        done_res = done_res || res;
        passes -= S;
    }
    return p;
}

/* the k-th launch of a stage (k = 0, 1, ...: a step counts `times` times), NULL behind the last one */
static inline const StageStep *mg3d_stage_launch(const StagePlan &p, int k)
{
    for (int i = 0; i < p.n; k -= p.step[i++].times)
        if (k < p.step[i].times)
            return &p.step[i];
    return nullptr;
}

/* what the options say about one launch per leg (legs, legs_min) or the carried cycles (carry, carry_min) on a finest level
 * of N points per side */
static inline bool mg3d_run_ahead_policy(const mg3d_options &o, bool legs, int N)
{
    return o.v[legs ? MG3D_OPT_LEGS : MG3D_OPT_CARRY] != 0 && N >= o.v[legs ? MG3D_OPT_LEGS_MIN : MG3D_OPT_CARRY_MIN];
}
/* The conditions the one-launch legs and the carried cycles share, single domain and slabs: the schedule's own switch and
 * threshold unless the caller fixed it (forced = 0 / 1; -1: by the options), V(2,2), r not kept, a level the
 * four-rows-per-thread shapes exist for (never at 65^3 and below) with an odd number of rows. */
static inline bool mg3d_can_run_ahead(const mg3d_options &o, bool legs, int forced, int iters, bool keep_r, int N, int nj)
{
    const bool on = forced >= 0 ? forced != 0 : mg3d_run_ahead_policy(o, legs, N);
    return on && iters == 2 && !keep_r && N > 65 && (nj & 1) != 0;
}
/* mg3d_tiny.hip: the level above the coarsest one in one workgroup (LDS-resident), when it fits (N <= 17) */
bool k_tiny_fits(const Geom &g, const Geom &gc);
/* zero guess, `iters` x (red, black), residual, restriction (interior + face injection from r's boundary) into dc */
void k_tiny_down(const Geom &g, double *u, const double *d, const double *r, const Geom &gc, double *dc, const LevelOp &op,
                 int iters, hipStream_t s);
/* u += P(ec) at every point, then `iters` x (black, red) */
void k_tiny_up(const Geom &g, double *u, const double *d, const Geom &gc, const double *ec, const LevelOp &op, int iters,
               hipStream_t s);
/* the bottom of the cycle in one launch: tiny_down on level 1, the direct solve of level 0 (reduced factor lin, the full
 * one as its fall-back), tiny_up on level 1; dc / xc receive level 0's right-hand side and solution */
bool k_tiny_cycle_fits(const Geom &g, const Geom &gc, const LuBand &lu, const LuBand &lin);
void k_tiny_cycle(const Geom &g, double *u, const double *d, const double *r, const Geom &gc, double *dc, double *xc,
                  const LuBand &lu, const LuBand &lin, const LevelOp &op, int iters, hipStream_t s);
/* eps of the coarser level by injection at every point */
void k_coef_inject(const Geom &gf, const double *ef, const Geom &gc, double *ec, hipStream_t s);
/* periodic axes, Neumann faces and fixed points (bc = mg3d_bc(periodic, neumann), single-domain levels): the right-hand
 * side of the direct solve -- b = d except in identity rows: 0 in the duplicates' and (pin) the pinned point's, and at the
 * fixed unknowns of m (NULL: no mask) 0. -- or ufix there when given (a one-level context) --; and a duplicate refresh
 * (gate, a word in device memory: nothing is written while it is 0 -- the deposit's "did anything deposit") */
void k_coarse_rhs(const Geom &g, const double *d, double *b, int bc, int pin, const unsigned char *m, const double *ufix,
                  hipStream_t s);
void k_per_refresh(const Geom &g, double *v, int bc, hipStream_t s, const unsigned long long *gate = nullptr);
/* fixed points (mg3d_ctx_set_mask): one byte per point of a single-domain level in the padded layout (the doubles' index).
 * k_mask_pack: the caller's dense-indexed bytes (mg3d_array of MG3D_U8, any strides) into it, periodic duplicates taking
 * their sources'; k_mask_inject / k_mask_refresh: the coarser level's bytes by injection, the duplicates' from their sources;
 * k_mask_count: *out += the number of fixed UNKNOWNS (no duplicate, on no Dirichlet face) */
void k_mask_pack(const Geom &g, unsigned char *m, const mg3d_array &a, int bc, hipStream_t s);
void k_mask_inject(const Geom &gf, const unsigned char *mf, const Geom &gc, unsigned char *mc, hipStream_t s);
void k_mask_refresh(const Geom &g, unsigned char *m, int bc, hipStream_t s);
/* MG3D_MASK_KEEP: the coarser level's bytes by injection where the coarse point's own fine point is fixed, else the byte of
 * the first lost fine point it is the lower parent of (mg3d_kernels.hip); the caller refreshes the coarse duplicates */
void k_mask_keep(const Geom &gf, const unsigned char *mf, const Geom &gc, unsigned char *mc, hipStream_t s);
void k_mask_count(const Geom &g, const unsigned char *m, int bc, unsigned long long *out, hipStream_t s);
/* full multigrid (mg3d_fmg_solve): every unknown of the fine level (and its periodic duplicates) overwritten with the
 * tensor-product cubic interpolant of the coarse u -- never a Dirichlet point; and d = u at the Dirichlet points of a level,
 * the right-hand side of the direct solve's identity rows.  Single-domain levels, bc the boundary word.  mf: the fine level's
 * fixed points, which the interpolation does not write either.  k_fmg_inject: u of the coarser level under MG3D_MASK_KEEP --
 * injection, a coarse fixed unknown that stands for a lost fine point taking that point's u */
void k_fmg_interp(const Geom &gc, const double *uc, const Geom &gf, double *uf, int bc, hipStream_t s,
                  const unsigned char *mf = nullptr);
void k_fmg_inject(const Geom &gf, const double *uf, const unsigned char *mf, const Geom &gc, double *uc, int bc, hipStream_t s);
void k_dirichlet_rhs(const Geom &g, const double *u, double *d, int bc, hipStream_t s);
/* zeros on the faces of a single-domain level given as a MG3D_NEUMANN_* mask */
void k_zero_faces(const Geom &g, double *v, int faces, hipStream_t s);
/* device arrays (mg3d_array, include/mg3d.h; single-domain levels): element (i,j,k) of the caller's array is
 * ptr[stride[0]*i + stride[1]*j + stride[2]*k] in 64-bit arithmetic, float or double; the walk is the level-wide one, k
 * fastest across the wave, so stride[2] == 1 is coalesced on both sides.
 * k_pack: v[i,j,k] = (double)a[i,j,k] at the N^3 points -- the row padding of v is never written.
 * k_unpack: a[i,j,k] = v[i,j,k], rounded to nearest for float -- the row padding of v is never read.
 * k_coef_check: out[0] += the number of entries of a that are not finite and > 0, out[1] = min(out[1], the lowest dense
 * index (i*N + j)*N + k among them); the duplicates of the periodic axes (bits 0..2 of bc) are skipped.  Folded per block,
 * then one 64-bit atomic add and one atomic min per block that found any: integers, no order to depend on.  The caller sets
 * out = {0, ~0} first. */
void k_pack(const Geom &g, double *v, const mg3d_array &a, hipStream_t s);
void k_unpack(const Geom &g, const double *v, const mg3d_array &a, hipStream_t s);
void k_coef_check(const Geom &g, const mg3d_array &a, int bc, unsigned long long *out, hipStream_t s);
/* the screening field (mg3d_ctx_set_shift_field).  k_field_check: k_coef_check with "finite and >= 0".  k_field_count:
 * *out += the number of UNKNOWNS (k_mask_count's) at which the level's field f, in the padded layout, is > 0 */
void k_field_check(const Geom &g, const mg3d_array &a, int bc, unsigned long long *out, hipStream_t s);
void k_field_count(const Geom &g, const double *f, int bc, unsigned long long *out, hipStream_t s);
/* field output (mg3d_field.hip; single-domain levels, bc the boundary word; include/mg3d.h "Field output" has the formulas).
 * k_gradient: cs * (the central / wrapped / reflected / one-sided difference of u) per axis at all N^3 points into the
 * caller's arrays out[0..2] (NULL: not wanted; at least one; float or double each, any strides >= 1), one launch.
 * k_field_flux: *out = the sum of w(p)*(s - D*u_p) over the fixed unknowns whose byte m[p] is `label` (0: any nonzero).
 * k_field_energy: *out = the sum of (w_e*a_e)*(u_q - u_p)^2 over the owned edges.
 * Both sums: one partial per block, folded in a fixed order.  Return value: the number of partials (k_gradient: 0), -1 when
 * the level has no launch shape (nothing launched). */
int k_gradient(const Geom &g, const double *u, int bc, double cs, const mg3d_array *const out[3], hipStream_t s);
int k_field_flux(const Geom &g, const double *u, const LevelOperator &A, int label, double *partials, double *out,
                 hipStream_t s);
int k_field_energy(const Geom &g, const double *u, const LevelOperator &A, double *partials, double *out, hipStream_t s);
/* particles (mg3d_particle.hip; single-domain levels, bc the boundary word, h the level's spacing; include/mg3d.h
 * "Particles" has the formulas).  One thread per point in 256-thread blocks, at most MG3D_PARTICLE_MAX_BLOCKS of them:
 * past that a thread strides on to further points.  pos, q: the caller's vectors, checked by the entry point.
 * k_part_sample: u and the nodal gradient (cs = scale * (0.5 / h)) interpolated to the points, NaN for a point outside,
 *   into u_out / grad_out[0..2] (NULL: not wanted), one launch.
 * k_part_push: one step of mg3d_particle_push_device for the particles whose fate is 0 -- the host constants are formed
 *   here from pp and h --, mask the level's fixed-point bytes in the padded layout (NULL: no mask), table the
 *   MG3D_FATE_SLOTS 64-bit counters; pos, vel, qm and fate the caller's vectors (fate of MG3D_I32), one launch.
 * The deposit, K the smallest integer with count <= 2^K, amax one 64-bit word and acc one long long per element of the
 * level's layout, both zeroed by the caller:
 *   k_part_scan       : *amax = the largest bit pattern of |q| over the points inside with a finite q
 *   k_part_accumulate : acc[source of node] += llrint(ldexp(q * w, -ue)) per point and corner, ue from *amax and K
 *   k_part_apply      : d[p] = d[p] + (f0 * nf(p)) * ldexp((double)acc[p], ue) where acc[p] != 0, f0 = scale / h^3
 * The last two do nothing while *amax is 0.  Return value: 0, -1 when the level has no launch shape (nothing launched). */
#define MG3D_PARTICLE_MAX_BLOCKS 2048
int k_part_sample(const Geom &g, const double *u, int bc, double h, double cs, long long count, const mg3d_vec *const pos[3],
                  const mg3d_vec *u_out, const mg3d_vec *const grad_out[3], hipStream_t s);
int k_part_push(const Geom &g, const double *u, const unsigned char *mask, int bc, double h, long long count,
                const mg3d_vec *const pos[3], const mg3d_vec *const vel[3], const mg3d_vec *qm, const mg3d_vec *fate,
                const mg3d_push_params &pp, unsigned long long *table, hipStream_t s);
int k_part_scan(const Geom &g, int bc, double h, long long count, const mg3d_vec *const pos[3], const mg3d_vec *q,
                unsigned long long *amax, hipStream_t s);
int k_part_accumulate(const Geom &g, int bc, double h, long long count, int K, const mg3d_vec *const pos[3],
                      const mg3d_vec *q, const unsigned long long *amax, long long *acc, hipStream_t s);
int k_part_apply(const Geom &g, int bc, double f0, int K, const unsigned long long *amax, const long long *acc, double *d,
                 hipStream_t s);
/* The reorder (mg3d_particle_sort_device, mg3d_particle_permute_device), ntiles = ceil(count / MG3D_SORT_TILE):
 *   k_sort_keys    : keys[m] = the key of particle m (fate NULL: all alive; nb^3 + 1 must fit 32 bits, the entry point
 *                    checks); counts (NULL: not wanted; two 64-bit words zeroed by the caller) += the inside and the lost.
 *                    -1 when the level has no launch shape.
 *   k_sort_hist    : table[digit * ntiles + tile] = the tile's keys whose bits sh .. sh+7 are `digit` (256 * ntiles words)
 *   k_sort_rowscan : every row of the table scanned in place, exclusive; tot[digit] = the row's sum (256 words)
 *   k_sort_scatter : the stable scatter of (kin, iin) by that digit into (kout, iout[iout_stride * .]); iin NULL: the old
 *                    index of element e is e; kout NULL: the keys are not written (the last pass)
 *   k_part_permute : dst[v][m] = src[v][perm[m]], v < nvec <= MG3D_PERMUTE_MAX_VECS, one launch; the entry point has
 *                    checked the vectors (a pair of one dtype, MG3D_F64 eight bytes an element, the others four) */
#define MG3D_SORT_TILE 2048
int k_sort_keys(const Geom &g, int bc, double h, long long count, const mg3d_vec *const pos[3], const mg3d_vec *fate,
                int shift, unsigned *keys, unsigned long long *counts, hipStream_t s);
void k_sort_hist(const unsigned *keys, long long count, int sh, unsigned *table, hipStream_t s);
void k_sort_rowscan(long long count, unsigned *table, unsigned *tot, hipStream_t s);
void k_sort_scatter(const unsigned *kin, const int *iin, unsigned *kout, int *iout, long long iout_stride, long long count,
                    int sh, const unsigned *table, const unsigned *tot, hipStream_t s);
int k_part_permute(long long count, const mg3d_vec *perm, int nvec, const mg3d_vec *const *src, const mg3d_vec *const *dst,
                   hipStream_t s);
/* b and x are level-0 grids in the padded layout g0; work holds 2n doubles */
/* steps per chunk of the streamed solve for n unknowns and rot_r = R on the current device, 0 if it cannot run */
int mg3d_lu_stream_chunk(int n, int R);
void k_lu_solve(const LuBand &lu, const LuBand &lu_in /* reduced factor; n == 0: none */, const Geom &g0, const double *b_pad, double *x_pad, double *work, hipStream_t s);

#endif
