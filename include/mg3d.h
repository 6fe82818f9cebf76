/*
 * mg3d.h -- C ABI of libmg3d.so, the MI355X (gfx950) implementation of the
 * reference's 3D geometric-multigrid V-cycle (knram06/multigrid_parallel,
 * mg_3d.h).  Plain C: opaque context, raw pointers, sizes, int status codes.
 * No C++ exceptions, no torch types cross this boundary.
 *
 * The reference has no FFI; its boundary is textual inclusion of mg_3d.h
 * (test_mg_3d.c:4-6).  include/mg_3d.h in this repo is the drop-in header
 * whose functions forward to the entry points below.  Every entry point cites
 * the reference definition it replaces (file:line under the reference tree).
 *
 * All grids are fp64, vertex centred, idx = N*N*i + N*j + k with k contiguous
 * on the HOST side (mg_3d.h:43-44).  On the device every level is kept in a
 * padded layout (k-pitch a multiple of 16 doubles); mg3d_upload/download
 * convert.  There is NO CPU fallback: every compute entry point returns
 * MG3D_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef MG3D_H
#define MG3D_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mg3d_ctx mg3d_ctx;

enum {
    MG3D_OK = 0,
    MG3D_ERR_ARG = 1,       /* bad argument (NULL, size, level out of range) */
    MG3D_ERR_NO_DEVICE = 2, /* no HIP device: the product has no CPU path */
    MG3D_ERR_HIP = 3,       /* a HIP runtime call failed; see mg3d_last_error() */
    MG3D_ERR_ALLOC = 4,
    MG3D_ERR_STATE = 5      /* e.g. V-cycle requested before the coarse LU was set */
};

/* fields of a level (mg_3d.h:26: double **u, **d, **r) */
enum { MG3D_U = 0, MG3D_D = 1, MG3D_R = 2 };

/* stages of the per-level timing table (mg_3d.h:136-137) */
enum {
    MG3D_ST_SMOOTH1 = 0, MG3D_ST_RESIDUAL1, MG3D_ST_RESTRICT, MG3D_ST_RECURSE,
    MG3D_ST_PROLONG, MG3D_ST_SMOOTH2, MG3D_ST_RESIDUAL2, MG3D_NUM_STAGES
};

const char *mg3d_last_error(void);     /* thread-local text of the last failure */
const char *mg3d_stage_name(int stage); /* "Smoother1", ... (mg_3d.h:136-137) */
int mg3d_device_count(void);            /* 0 when no usable device */

/* ------------------------------------------------------------------ context
 * Replaces SolverInitialize's allocation (mg_3d.h:107-144, 30-48): three
 * hierarchies u,d,r of num_levels levels, level l having
 * ((coarse_pts-1)*2^l+1)^3 points, all zero; spacing = grid_length/(N-1). */
int mg3d_ctx_create(int coarse_pts, int num_levels, int smooth_iters, double grid_length, mg3d_ctx **out);
int mg3d_ctx_destroy(mg3d_ctx *ctx); /* SolverFinalize, mg_3d.h:1452-1467 */
int mg3d_ctx_num_levels(const mg3d_ctx *ctx);
int mg3d_ctx_level_n(const mg3d_ctx *ctx, int level); /* points per side, mg_3d.h:41 */
double mg3d_ctx_level_h(const mg3d_ctx *ctx, int level);
int mg3d_ctx_set_smooth_iters(mg3d_ctx *ctx, int iters);
/* keep != 0: every V-cycle materialises the residual arrays r[level] as the reference does (mg_3d.h:1294).
 * Default 0: the residual is restricted into the coarse right-hand side on the fly and r is not written --
 * u, d and the returned norms are identical either way.  mg3d_host_vcycle always keeps r. */
int mg3d_ctx_set_keep_residual(mg3d_ctx *ctx, int keep);

/* Coarsest operator.  mg3d_ctx_build_coarse = constructCoarseMatrixA +
 * convertToLU_InPlace as SolverGetDetails does (mg_3d.h:282-289), with the
 * spacing the caller chooses (mg_3d.h:287 passes h*2^(L-1);
 * test_mg_3d_dirichlet.c:40 passes the finest h).  mg3d_ctx_set_lu installs a
 * caller-factored row-major LU (n = coarse_pts^3) instead. */
int mg3d_ctx_build_coarse(mg3d_ctx *ctx, double h_coarse);
int mg3d_ctx_set_lu(mg3d_ctx *ctx, const double *LU);

/* Screened operator.  Every operator of the context -- smoother, residual, the coarsest matrix -- becomes the one of
 *     Delta_h u - sigma u = d        (sigma >= 0; the residual stays d - (Delta_h u - sigma u), mg_3d.h:819-821)
 * per level of spacing h:  smoother  v = (1/dg) * (sum of the six neighbours - h^2 d),  dg = 6 + sigma*h^2;
 * residual  d - (sum - dg*v)/h^2;  coarse matrix diagonal -dg/h^2 (mg3d_coarse_matrix_shift).  The default sigma = 0 is
 * the reference's operator, bit for bit.  Implicit diffusion (backward Euler, u1 - dt*Delta u1 = u0): sigma = 1/dt with
 * the right-hand side d = -u0/dt -- mg3d_step_advance below does it, and the theta-scheme, on the device.
 * A negative, NaN or infinite sigma is MG3D_ERR_ARG and changes nothing.  Otherwise a
 * cycle that has run ahead is finished first; a new sigma rebuilds a factor of mg3d_ctx_build_coarse (same h_coarse) and
 * drops one installed by mg3d_ctx_set_lu or mg3d_es_setup (the next cycle returns MG3D_ERR_STATE until a factor is set
 * again); a call that leaves sigma as it is changes nothing.  mg3d_es_* refuse a context with sigma != 0 (MG3D_ERR_STATE);
 * the mg3d_host_* forms and include/mg_3d.h always use sigma = 0, as the reference does. */
int mg3d_ctx_set_shift(mg3d_ctx *ctx, double sigma);
int mg3d_ctx_get_shift(const mg3d_ctx *ctx, double *sigma);

/* Variable coefficient.  Every operator of the context becomes the one of
 *     div(eps grad u) - sigma u = d        (eps > 0 at every grid point, vertex-centred; sigma as mg3d_ctx_set_shift)
 * with face means a = 0.5*(eps_p + eps_q) over the six neighbours q (order i-, i+, j-, j+, k-, k+):  s = sum of a*v_q,
 * dg = sum of a + sigma*h^2;  smoother  v = (s - h^2 d)/dg;  residual  d - (s - dg*v)/h^2;  coarse matrix
 * mg3d_coarse_matrix_coef of level 0's eps.  eps is the finest level's, a dense N^3 host array; a coarser level takes
 * eps by injection (e_{l-1}[I,J,K] = e_l[2I,2J,2K]).  An entry that is not finite and > 0 is MG3D_ERR_ARG and changes
 * nothing.  Otherwise, as for mg3d_ctx_set_shift, a cycle that has run ahead is finished first, and a factor of
 * mg3d_ctx_build_coarse is rebuilt (one of mg3d_ctx_set_lu / mg3d_es_setup dropped).  Another array replaces eps on every
 * level; NULL returns to the constant-coefficient operator, bit for bit.  With a coefficient every level runs colour
 * passes and residual of their own kernels: the fused schedules and their options (carry, legs, tiny, tiny_cycle,
 * fuse_*, sweep_*) keep their values but do not apply.  mg3d_es_* refuse such a context (MG3D_ERR_STATE).  The slab form
 * has its own call, mg3d_dist_set_coefficient; the fp32 (mg3d32_*, mg3d32_dist_*), mixed-boundary (mg3d_es_*) and
 * mg3d_host_* forms and the drop-in mg_3d.h have no coefficient. */
int mg3d_ctx_set_coefficient(mg3d_ctx *ctx, const double *eps); /* finest level, dense N^3 host array; NULL: constant operator again */
int mg3d_ctx_has_coefficient(const mg3d_ctx *ctx, int *on);
int mg3d_ctx_get_coefficient(mg3d_ctx *ctx, int level, double *host); /* the injected eps of a level, dense n^3; MG3D_ERR_STATE without one */

/* Periodic boundaries per axis.  axes is a mask of MG3D_PERIODIC_I / _J / _K (any of 0..7); 0 is the Dirichlet operator
 * of every face, bit for bit and with the fused schedules.  A level keeps its N points per side and its layouts; on a
 * periodic axis index N-1 is the DUPLICATE of index 0, the unique points are 0 .. N-2 and face points there are unknowns
 * (non-periodic axes keep their Dirichlet faces).  No kernel reads a duplicate of u, d, r or eps: stencils reach across
 * the wrap to the unique point, and whatever writes a unique point on a periodic face writes its duplicates too, so a
 * downloaded u (or r with keep_residual) is periodic-consistent.  The restriction fully weights the periodic faces, the
 * coarse matrix is mg3d_coarse_matrix_periodic, the residual norm counts every unique point once.  All three axes
 * periodic with sigma = 0 is singular (constants are in the kernel): the coarse matrix pins unique point (0,0,0) of level
 * 0 to 0, u is determined up to a constant, and f must have zero mean over the unique points -- the library projects
 * neither f nor u, and the residual stalls at that mean otherwise.  A mask outside 0..7, or a nonzero one when c - 1 is
 * odd or below 4, is MG3D_ERR_ARG and changes nothing; otherwise, as for mg3d_ctx_set_shift, a cycle that has run ahead
 * is finished first and a factor of mg3d_ctx_build_coarse is rebuilt (one of mg3d_ctx_set_lu / mg3d_es_setup dropped);
 * the same mask again changes nothing.  With a periodic axis the fused schedules and their options do not apply (values
 * kept), and mg3d_es_*, mg3d_fmg_initialize and mg3d_fill_boundary return MG3D_ERR_STATE.  The slab (mg3d_dist_*), fp32
 * (mg3d32_*) and mg3d_host_* forms have no periodic mode.  mg3d_ctx_set_coefficient on a periodic context neither checks
 * nor keeps eps at the duplicates: their sources are copied over them. */
enum { MG3D_PERIODIC_I = 1, MG3D_PERIODIC_J = 2, MG3D_PERIODIC_K = 4 };
int mg3d_ctx_set_periodic(mg3d_ctx *ctx, int axes);
int mg3d_ctx_get_periodic(const mg3d_ctx *ctx, int *axes);

/* Neumann boundaries per face.  faces is a mask of MG3D_NEUMANN_ILO / _IHI / _JLO / _JHI / _KLO / _KHI (any of 0..63); 0
 * is the operator without Neumann faces, bit for bit and with the same schedules and launches.  A level keeps its N
 * points per side and its layouts.  A point on a Neumann face is an UNKNOWN -- an edge or corner point too, unless it
 * also lies on a Dirichlet face: then it is a Dirichlet point that nothing writes.  There are no duplicates and nothing
 * outside the array.  The operator imposes the homogeneous condition du/dn = 0 by reflection: at index 0 of a Neumann low
 * face the -1 neighbour is read at index 1, at index N-1 of a Neumann high face the +1 neighbour at N-2, for u and, with
 * a coefficient, for eps as well (the face coefficient 0.5*(eps_0 + eps_1) then counts twice); smoother and residual keep
 * their arithmetic and operand order, and red-black colours stay (i + j + k) & 1 over all unknowns (a reflected
 * neighbour has the other colour: any c >= 3).  The restriction fully weights every coarse unknown, Neumann face points
 * included, with reflected fine neighbours; the prolongation corrects the Neumann face points; eps goes down the
 * hierarchy by injection; the coarse matrix is mg3d_coarse_matrix_bc; the residual norm counts every unknown once.
 * With periodic axes the masks combine per axis: an axis is periodic, or each of its two faces is Dirichlet or Neumann; a
 * Neumann bit on a periodic axis is MG3D_ERR_ARG from whichever of the two setters is called second.
 * Singular case: sigma = 0 and every axis either periodic or Neumann on both faces -- constants are in the kernel.  The
 * coarse matrix then pins unknown (0,0,0) of level 0 to 0 (identity row, right-hand side taken as 0), as the periodic
 * case does, and the library projects neither f nor u.  The reflected operator is not symmetric: its left null vector
 * is the trapezoid weight w = 1/2 per Neumann face a point lies on (1/4 on an edge of two, 1/8 at a corner of three), so
 * the compatibility condition is WEIGHTED: sum of w*f over the unknowns = 0; the residual stalls at that weighted mean
 * otherwise.  mg3d_wpcg_solve solves to a tolerance in that weighted inner product and does project, on its own vectors.
 * A prescribed flux g = du/dn (outward normal) keeps the operator homogeneous and is folded into the right-hand side by
 * mg3d_neumann_fold_flux (below) before the upload.
 * A mask outside 0..63, or a bit on a periodic axis, is MG3D_ERR_ARG and changes nothing; otherwise, as for
 * mg3d_ctx_set_periodic, a cycle that has run ahead is finished first with the operator it started with and a factor of
 * mg3d_ctx_build_coarse is rebuilt (one of mg3d_ctx_set_lu / mg3d_es_setup dropped); the same mask again changes
 * nothing.  With a nonzero mask the fused schedules and their options do not apply (values kept), and mg3d_es_*,
 * mg3d_fmg_initialize and mg3d_fill_boundary return MG3D_ERR_STATE.  The slab (mg3d_dist_*), fp32 (mg3d32_*) and
 * mg3d_host_* forms have no Neumann mode.  mg3d_ctx_set_coefficient checks and keeps eps on Neumann faces: they are read. */
enum {
    MG3D_NEUMANN_ILO = 1,
    MG3D_NEUMANN_IHI = 2,
    MG3D_NEUMANN_JLO = 4,
    MG3D_NEUMANN_JHI = 8,
    MG3D_NEUMANN_KLO = 16,
    MG3D_NEUMANN_KHI = 32
};
int mg3d_ctx_set_neumann(mg3d_ctx *ctx, int faces);
int mg3d_ctx_get_neumann(const mg3d_ctx *ctx, int *faces);

/* Fixed points inside the domain (embedded conductors).  mask is one byte per point of the finest level, a dense N^3 host
 * array; nonzero means FIXED.  A fixed point is a Dirichlet point, exactly like a point on a Dirichlet face: u there is
 * whatever the caller uploaded and nothing ever changes it -- no smoother, prolongation, mg3d_pcg_solve / mg3d_wpcg_solve
 * update or projection, no mg3d_step_advance (one exception to "bit for bit": the CG update pass visits fixed points and
 * stores u + alpha*0. there, the same value, but a -0. the caller uploaded comes back as +0.) --, d there is never read, the residual there is 0 (r is stored as 0. where the
 * residual stores, nothing enters the norm), and its neighbours read its u through the ordinary stencil (with a
 * coefficient also its eps: mg3d_ctx_set_coefficient keeps checking eps at fixed points).  A byte on a point that is a
 * Dirichlet face point already is ignored; on a periodic context the duplicates' bytes are ignored and take their sources'
 * -- for good: whether the mask or the periodic axis comes first, index N-1 of that axis holds index 0's bytes from then on,
 * also after the axis stops being periodic (pass the mask again to have other bytes there);
 * a point on a Neumann face may be fixed.  The mask is orthogonal to the rest of the operator: constant or eps, sigma,
 * periodic axes and Neumann faces keep their arithmetic and combine freely with it, the setters work in every order.
 * Hierarchy: a coarser level takes the mask by injection (m_{l-1}[I,J,K] = m_l[2I,2J,2K], like eps); below the finest level
 * u starts at zero, so the fixed points hold the zero error they must; the restriction is unchanged (it reads the zeros the
 * residual stored); the prolongation skips fine fixed points (masked levels take the point form); at level 0 the
 * right-hand side of the direct solve is 0 at fixed points and the matrix is mg3d_coarse_matrix_mask -- identity rows
 * there (a one-level context solves with u's own values at its fixed points).  Restriction and prolongation stay transposes
 * on the unknowns: the cycle remains a symmetric preconditioner.
 * Injection loses a body thinner than the coarse spacing -- a one-point plate on an odd plane is gone from every coarse
 * level -- and plain cycles then converge slowly or GROW: mg3d_vcycle(s) are for bodies that survive on the coarse grids,
 * mg3d_pcg_solve / mg3d_wpcg_solve are the solvers for thin ones ("Embedded conductors") -- or the
 * hierarchy keeps them: mg3d_ctx_set_mask_coarsening(MG3D_MASK_KEEP) below, under which plain cycles contract on thin bodies.
 * Singular cases: the pin of unknown (0,0,0) of level 0 applies iff the condition of mg3d_ctx_set_neumann holds AND level
 * 0's mask has no fixed unknown; mg3d_wpcg_solve projects iff that condition holds and the FINEST mask has no fixed
 * unknown (a fixed unknown removes the constants from the kernel).
 * State, as for mg3d_ctx_set_coefficient: a cycle that has run ahead is finished first with the operator it started with;
 * a factor of mg3d_ctx_build_coarse is rebuilt, one of mg3d_ctx_set_lu / mg3d_es_setup dropped.  NULL returns to the
 * context without a mask, bit for bit and with its fused schedules; an all-zero mask is a mask: every grid value and norm
 * is that of the context without one on the unfused kernels.  With a mask the fused, carried, per-leg and
 * single-workgroup schedules do not apply (option values kept).  Refused with MG3D_ERR_STATE, nothing changed, on a context
 * with a mask: mg3d_es_*, mg3d_fmg_initialize, and -- while the mask is coarsened by injection, under which a thin body is
 * absent from the levels full multigrid starts on -- mg3d_fmg_solve, mg3d_fmg_interpolate (accepted under
 * MG3D_MASK_KEEP, mg3d_ctx_set_mask_coarsening).  mg3d_step_advance works as it is: fixed points are Dirichlet values
 * constant in time, d there is unspecified.  The slab, fp32 and mg3d_host_* forms and the drop-in header have no mask.
 * mg3d_ctx_set_mask_device: the same from a device array (mg3d_array below) of dtype MG3D_U8 -- nothing else --, any
 * element strides >= 0; the pointer is checked and the streams joined as for mg3d_ctx_set_coefficient_device.  Every byte
 * value is valid, so nothing is checked on the device; the call synchronises with the host once, to read back level 0's
 * mask for the coarse matrix and the numbers of fixed unknowns.  NULL: no mask.
 * mg3d_ctx_get_mask: the mask a level holds, under either coarsening rule, dense n^3 (periodic duplicates hold their
 * sources' bytes). */
int mg3d_ctx_set_mask(mg3d_ctx *ctx, const unsigned char *mask); /* finest level, dense N^3 host array; NULL: no mask */
int mg3d_ctx_has_mask(const mg3d_ctx *ctx, int *on);
int mg3d_ctx_get_mask(mg3d_ctx *ctx, int level, unsigned char *host); /* the level's mask, dense n^3; MG3D_ERR_STATE without one */
/* How the coarser levels take the mask.  MG3D_MASK_INJECT, the default: injection as above, every byte, count and grid value
 * what it is without this call.  MG3D_MASK_KEEP: a fixed point that injection would lose fixes ONE coarse point, so a body
 * thinner than the coarse spacing stays on every level without growing thicker level by level.  Level l -> l-1 (fine side N,
 * coarse side Nc), on the stored bytes of the fine level, whose periodic duplicates hold their sources' bytes; raw bytes, no
 * boundary word, nothing outside the array is read.  For the coarse point C = (I, J, K):
 *   1. m_f[2C] != 0: m_c[C] = m_f[2C], the injection.
 *   2. otherwise the fine points F = 2C + (a, b, c), a, b, c in {0, 1} not all zero, are looked at in the order (0,0,1),
 *      (0,1,0), (0,1,1), (1,0,0), (1,0,1), (1,1,0), (1,1,1); an F with an index > N-1 is skipped (only where a coarse index is
 *      Nc-1).  F is LOST when m_f[F] != 0 and m_f[2P] == 0 for every parent P = C + (a*al, b*be, c*ga), al, be, ga in {0, 1},
 *      of F.  m_c[C] is the byte of the first lost F, or 0 when there is none.
 *   3. the coarse level's periodic duplicates take their sources' bytes (a duplicate plane Nc-1 sees fewer F than its source).
 * So every fixed fine point has a fixed parent on the next level: an injected one, or its lower parent floor(F/2).  A body
 * that injection represents already is left exactly as injection has it (a ball of radius 0.2 at 33^3 or 65^3: the same
 * hierarchy).  Effects: BIAS -- a lost body moves by up to one fine spacing towards the LOW index on each level, since the
 * lower parent is taken; the rule is not mirror-symmetric, the price of not thickening the body.  LABELS -- a coarse byte is
 * the byte of the point it stands for.  The cycle stays a SYMMETRIC preconditioner for any coarse mask (the restriction
 * reads the zeros the residual stores at fine fixed points, coarse fixed points hold zero error, the prolongation skips
 * fine fixed points), so mg3d_pcg_solve, mg3d_wpcg_solve and mg3d_step_advance work unchanged.  The SINGULAR-case rules
 * read the same counts: under MG3D_MASK_KEEP a thin body reaches level 0, so the pin is lifted where injection would have kept
 * it.  Plain cycles that GROW on thin bodies under injection (factor 1.6 to 4.7 per cycle at 33^3 and 65^3) contract under
 * MG3D_MASK_KEEP (0.42 to 0.54; INTEGRATION.md, "Embedded conductors", has the table).
 * Operator state, not a launch option (grid values depend on it): it may be set before or after the mask and every other
 * setter, in every order.  A rule that is neither of the two, or a NULL pointer: MG3D_ERR_ARG, nothing changed.  Without a
 * mask the rule is stored for the next mg3d_ctx_set_mask(_device).  With one, a call that CHANGES the rule finishes a cycle
 * that has run ahead, takes levels L-2 .. 0 again from the finest level's stored bytes, recounts the fixed unknowns and
 * reads back level 0 (one host synchronisation), and rebuilds or drops the coarse factor as every setter does; the same rule
 * again changes nothing.  When the periodic mask changes, the finest duplicates are rewritten for good as above and, under
 * MG3D_MASK_KEEP, the lower levels are coarsened again from the finest one. */
enum { MG3D_MASK_INJECT = 0, MG3D_MASK_KEEP = 1 };
int mg3d_ctx_set_mask_coarsening(mg3d_ctx *ctx, int rule);
int mg3d_ctx_get_mask_coarsening(const mg3d_ctx *ctx, int *rule);
/* (mg3d_ctx_set_mask_device is declared with the other device-array calls, behind mg3d_array) */

/* Screening field: sigma per grid point.  s is one double per point of the finest level, a dense N^3 host array, every entry
 * finite and >= 0.  Every operator of the context becomes the one of
 *     div(eps grad u) - (sigma + s_p) u = d        (sigma the scalar of mg3d_ctx_set_shift, added per point; eps as set, or 1)
 * with the arithmetic of the variable-coefficient kernels and one change: s(um) and D, the sum of the six face means --
 * exactly 6.0 without eps --, stay, and  dg = D + (sigma + s_p)*h^2, formed per point in this order;  smoother
 * v = (sum - h^2 d)/dg, an IEEE division also without eps;  residual  d - (sum - dg*v)/h^2;  A p of the CG solvers and q of the
 * stepper likewise;  coarse matrix mg3d_coarse_matrix_field, diagonal -((D + (sigma + s_p)*h^2)/h^2).  So an all-zero field
 * on a context with eps gives every grid value and norm of the context without a field, bit for bit; and a field without eps
 * gives what eps = 1.0 at every point gives with the same field -- the library runs that case on the eps kernels over an
 * internal array of ones (mg3d_ctx_has_coefficient still reports 0, mg3d_ctx_get_coefficient still MG3D_ERR_STATE;
 * INTEGRATION.md, "Screening field", has the cost).
 * Uses: a Newton step of Poisson-Boltzmann, Delta u - kappa^2 sinh u = f, is a solve with s = kappa^2 cosh u_k; decay or
 * reaction rates that vary in space under mg3d_step_advance; sponge layers.  A huge penalty inside a body is the job of
 * mg3d_ctx_set_mask, not of this field (below).  A Robin face is NOT offered as a helper: its term scales with 1/h per
 * level, which no coarsening of a stored field reproduces.
 * Hierarchy: s of a coarser level is the context's own restriction of the finer one -- FULL WEIGHTING at every coarse
 * unknown, with the wrapped (periodic) or reflected (Neumann) taps the operator has, injection at the points of Dirichlet
 * faces (never used), periodic duplicates copies of their sources.  Not injection, which loses a feature thinner than the
 * coarse spacing from every coarse level; with full weighting a thin feature is smeared, not lost, and plain cycles keep
 * converging (INTEGRATION.md has the measurements, and the one case injection wins: a penalty of 1e6 inside a ball).
 * When the boundary masks change, the coarser levels are restricted again.  On a periodic axis the duplicates of the
 * finest level are neither checked nor kept, for good, as for the mask.
 * Singular cases, as the mask's: the pin of unknown (0,0,0) of level 0 applies iff the condition of mg3d_ctx_set_neumann
 * holds AND level 0's mask has no fixed unknown AND level 0's field is > 0 at no unknown; mg3d_wpcg_solve projects iff that
 * holds and the FINEST mask has no fixed unknown and the finest field is > 0 at no unknown.
 * The contract is mg3d_ctx_set_coefficient's: the array is checked before anything changes (periodic duplicates skipped);
 * an entry that is not finite or is < 0 is MG3D_ERR_ARG and changes nothing, the message naming the lowest dense index
 * among them and its value.  Otherwise a cycle that has run ahead is finished first with the operator it started with, a
 * factor of mg3d_ctx_build_coarse is rebuilt and one of mg3d_ctx_set_lu / mg3d_es_setup dropped.  Another array replaces the
 * field on every level; NULL returns to the context as it was, bit for bit and with its fused schedules.  The setters
 * (shift, coefficient, periodic, neumann, mask, field) work in every order.  With a field the context runs the unfused
 * kernels, as with eps: the fused, carried, per-leg and single-workgroup options keep their values and do not apply, the
 * zero map of d is unused.  The field holds under mg3d_smooth, mg3d_residual, mg3d_vcycle(s), mg3d_pcg_solve /
 * mg3d_wpcg_solve (a non-negative diagonal keeps operator and cycle self-adjoint in the same inner products),
 * mg3d_fmg_solve (where no mask forbids it) and mg3d_step_*: mg3d_step_setup keeps setting the scalar, the equation stepped
 * is u_t = div(eps grad u) - (kappa + s_p) u + source, the field enters d through q and the stepper's formulas stand.
 * mg3d_field_*, mg3d_field_sample* and mg3d_deposit* ignore the field, as they ignore sigma.  mg3d_es_* and
 * mg3d_fmg_initialize return MG3D_ERR_STATE.  The slab, fp32 and mg3d_host_* forms and the drop-in header have no field.
 * mg3d_ctx_set_shift_field_device: the same from a device array (mg3d_array below), MG3D_F64 or MG3D_F32, any strides >= 0,
 * checked on the device before anything changes, with the stream ordering and the two host synchronisations of
 * mg3d_ctx_set_coefficient_device; MG3D_F64 stores the same bytes as the host form.
 * mg3d_ctx_get_shift_field: the restricted field of a level, dense n^3. */
int mg3d_ctx_set_shift_field(mg3d_ctx *ctx, const double *s); /* finest level, dense N^3 host array; NULL: no field */
int mg3d_ctx_has_shift_field(const mg3d_ctx *ctx, int *on);
int mg3d_ctx_get_shift_field(mg3d_ctx *ctx, int level, double *host); /* the restricted field of a level, dense n^3; MG3D_ERR_STATE without one */
/* (mg3d_ctx_set_shift_field_device is declared with the other device-array calls, behind mg3d_array) */

/* ------------------------------------------------------------ data movement
 * Host arrays are dense N^3 (reference layout). */
int mg3d_upload(mg3d_ctx *ctx, int field, int level, const double *host);
int mg3d_download(mg3d_ctx *ctx, int field, int level, double *host);
int mg3d_zero(mg3d_ctx *ctx, int field, int level); /* memset of mg_3d.h:1258-1259 */
int mg3d_sync(mg3d_ctx *ctx);
/* raw device view of a level for callers that share device memory (tests, bench) */
int mg3d_device_view(mg3d_ctx *ctx, int field, int level, void **dev_ptr, int *pitch_doubles, long *plane_doubles);

/* Device arrays: the four data entry points for arrays that already live in the memory of the context's device -- a field,
 * the stepper's source, eps.  Ordered on streams, not on the host; the library sees every write, so unlike
 * mg3d_device_view nothing is switched off (no raw-pointer flag, the run-ahead schedules stay) and nothing dangles.
 * mg3d_array describes a dense-INDEXED N x N x N array (N of the level, of the finest level for source and eps): element
 * (i, j, k) is ptr[stride[0]*i + stride[1]*j + stride[2]*k], strides in ELEMENTS, in any order and with any gaps (a
 * permuted or sliced tensor); the index is formed in 64 bits.  The library reads or writes exactly these N^3 elements and
 * trusts the strides: they must stay inside the caller's allocation.
 *   values   : MG3D_F64 stores the same bytes as the host form -- the field, every level of the injected eps, the source.
 *              MG3D_F32 is widened exactly on the way in and rounded to nearest (even) on the way out.  On the way in a
 *              stride may be 0 (a broadcast array); mg3d_download_device needs every stride >= 1, and overlap between the
 *              elements of dst beyond that is the caller's business.  The row padding of the device layout is neither
 *              written by an upload nor read by a download, as in the host forms.
 *   errors   : MG3D_ERR_ARG, nothing changed: a NULL context, array or ptr, an unknown dtype, a negative stride, a zero
 *              stride on download, a bad field or level, a ptr that hipPointerGetAttributes does not report as device memory
 *              of the context's device (the device current when the context was created).
 *   state    : exactly the host forms'.  mg3d_upload_device finishes a cycle that has run ahead and marks the field written
 *              as mg3d_upload does; mg3d_download_device only reads, as mg3d_download.
 *   ordering : `stream` is the hipStream_t on which the caller produced src or will consume dst; NULL is the null stream.
 *              The call makes the context's stream wait for an event recorded on `stream`, enqueues its kernel on the
 *              context's stream, and makes `stream` wait for an event recorded behind the kernel.  On return the caller may
 *              enqueue on `stream` anything that reads dst, and may overwrite or free src on `stream` (the discipline of a
 *              stream-ordered caching allocator); work on OTHER streams of the caller is not ordered.  mg3d_upload_device,
 *              mg3d_download_device and mg3d_step_set_source_device do not synchronise with the host.  The two events are
 *              created once per context and freed with it.
 * mg3d_step_set_source_device: mg3d_step_set_source from a device array -- the source field is allocated on first use
 *   (MG3D_ERR_ALLOC, nothing changed, when it does not fit) and written behind any step still in flight; NULL drops the
 *   source.  May be called between mg3d_step_advance calls; values at Dirichlet points and periodic duplicates are never used.
 * mg3d_ctx_set_coefficient_device: mg3d_ctx_set_coefficient from a device array, the same contract in the same order.
 *   The array is checked on the device before anything changes, as given (F32 widened), periodic duplicates skipped: an
 *   entry that is not finite and > 0 is MG3D_ERR_ARG, the message names the LOWEST dense index (i*N + j)*N + k among them and
 *   its value.  Otherwise a cycle that has run ahead is finished, eps of the finest level is written, its duplicates
 *   refreshed, the coarser levels injected, level 0's eps read back for the coarse matrix (the subsample the host form
 *   takes, bit for bit) and the coarse factor rebuilt or dropped.  This call DOES synchronise with the host, twice: for the
 *   result of the check and for level 0's eps; when it returns the array has been read.  NULL: the constant operator again.
 * kernel timer: MG3D_K_PACK counts the launches that read or write a caller's array.
 * Out of scope: the slab form (mg3d_dist_*), the fp32 solver (mg3d32_*) and the mg3d_host_* forms take host arrays only;
 * half precision and bf16; a persistent zero-copy alias of a field (the run-ahead schedules swap the buffers behind u and
 * d, an alias cannot stay valid).  mg3d_device_view is unchanged. */
enum { MG3D_F64 = 0, MG3D_F32 = 1, MG3D_U8 = 2 /* bytes: mg3d_ctx_set_mask_device only, which takes nothing else */ };
typedef struct mg3d_array {
    void *ptr;           /* element (0,0,0), device memory of the context's device */
    int dtype;           /* MG3D_F64 / MG3D_F32 (MG3D_U8: a mask) */
    long long stride[3]; /* in ELEMENTS, for i, j, k */
} mg3d_array;
int mg3d_upload_device(mg3d_ctx *ctx, int field, int level, const mg3d_array *src, void *stream);
int mg3d_download_device(mg3d_ctx *ctx, int field, int level, const mg3d_array *dst, void *stream);
int mg3d_step_set_source_device(mg3d_ctx *ctx, const mg3d_array *s /* NULL: no source */, void *stream);
int mg3d_ctx_set_coefficient_device(mg3d_ctx *ctx, const mg3d_array *eps /* NULL: constant operator */, void *stream);
int mg3d_ctx_set_mask_device(mg3d_ctx *ctx, const mg3d_array *mask /* dtype MG3D_U8 only; NULL: no mask */, void *stream);
int mg3d_ctx_set_shift_field_device(mg3d_ctx *ctx, const mg3d_array *s /* MG3D_F64 or MG3D_F32; NULL: no field */, void *stream);

/* ------------------------------------------------------------ field output
 * What is wanted of a solved potential u of div(eps grad u) - sigma u = f: the field E = -grad u, the charge u induces on
 * each embedded conductor, the stored energy (capacitance: C = Q/V = 2W/V^2) -- formed on the device from u of the FINEST
 * level with the context's own periodic wraps, reflected Neumann faces, face means of eps and fixed-point bytes.  All four
 * calls only read the context: a cycle that has run ahead is finished exactly as mg3d_download_device finishes it, and no
 * field, option, factor or flag changes -- the next mg3d_vcycle(s) gives the bits it would have given.  They work with
 * every operator and boundary combination of a context (constant or eps, any sigma, periodic axes, Neumann faces, with or
 * without a mask); sigma enters none of the three quantities.
 * Notation: N, h the finest level's points per side and spacing.  On axis a index x is a DUPLICATE if the axis is periodic
 * and x = N-1; it lies ON A DIRICHLET FACE if the axis is not periodic and (x = 0 without the MG3D_NEUMANN_ low bit of the
 * axis or x = N-1 without its high bit), ON A NEUMANN FACE if the axis is not periodic and the matching bit is set.  w(p) is
 * 1/2 per Neumann face the point p lies on (the weight of mg3d_wpcg_solve).
 *
 * mg3d_field_gradient_device: scale * du/dx_a at EVERY one of the N^3 points -- Dirichlet faces, fixed points and periodic
 *   duplicates included -- into out[a] (a = 0, 1, 2 for i, j, k; NULL: component not wanted).  cs = scale * (0.5 / h), in
 *   this order, on the host.  A point is first taken to its source (index N-1 of a periodic axis -> 0, on all three axes:
 *   no duplicate of u is read and a duplicate gets its source's bits); then per axis, the other two indices held:
 *     periodic axis           : lo = (x == 0) ? N-2 : x-1, hi = (x == N-2) ? 0 : x+1, value (u[hi] - u[lo]) * cs
 *     1 <= x <= N-2 otherwise : (u[x+1] - u[x-1]) * cs
 *     x = 0,   Neumann face   : (u[1] - u[1]) * cs          (the reflected tap: a zero)
 *     x = 0,   Dirichlet face : ((4.0*u[1] - 3.0*u[0]) - u[2]) * cs
 *     x = N-1, Neumann face   : (u[N-2] - u[N-2]) * cs
 *     x = N-1, Dirichlet face : ((3.0*u[N-1] - 4.0*u[N-2]) + u[N-3]) * cs
 *   Operands in this order, uncontracted.  scale = 1: the gradient; scale = -1: E.  The mask is IGNORED: a body held at one
 *   potential differences to zero inside on its own, and its surface is resolved as the grid resolves any surface.
 *   out[a] follows the mg3d_array contract of mg3d_download_device word for word -- MG3D_F64 (these bytes) or MG3D_F32
 *   (rounded to nearest even) per component, strides >= 1 in elements in any order and with any gaps, 64-bit index, the
 *   pointer checked, the two-event stream ordering, no host synchronisation.  All wanted components come out of ONE launch
 *   that reads u once; overlap between the output arrays is the caller's business.  MG3D_ERR_ARG, nothing written: a NULL
 *   context, all three components NULL, a scale that is not finite, a bad dtype, a stride < 1, a foreign pointer.  The
 *   launch counts under the kernel timer MG3D_K_PACK (it writes a caller's array).
 * mg3d_field_gradient: the same into dense N^3 host arrays (NULL: not wanted).  It runs the launch once per wanted
 *   component into one dense N^3 scratch buffer on the device, allocated for the call and freed at return (MG3D_ERR_ALLOC,
 *   nothing written, when it does not fit), each followed by a copy to the host; no field of the context is used.
 * mg3d_field_flux: the flux of eps grad u into the fixed points.  The mask's bytes are kept verbatim everywhere, so a byte
 *   value 1..255 is a free LABEL of a body.  P = the fixed unknowns (no duplicate, on no Dirichlet face, byte != 0) whose
 *   byte equals `label`, or all of them for label = 0:
 *       t_p = w(p) * (s - D*u_p),   *flux = h * (sum of t_p over P)
 *   s and D the neighbour sum and diagonal of the context's stencil at p, wrapped or reflected neighbours and operand order
 *   as in the residual, at sigma = 0: D = 6 for the constant operator, else the sum of the six face means 0.5*(eps_p + eps_q).
 *   This is h^3 times the sigma = 0 operator at the body's points; for a converged solution with d = 0 around the body it is
 *   the net flux of eps grad u into it -- times -eps_0 the charge (the caller's constant).  Per-block partial sums folded in
 *   a fixed order, the multiplication by h on the host: the same call on the same data gives the same bits.  MG3D_ERR_STATE
 *   on a context without a mask; MG3D_ERR_ARG for a label outside 0..255 or a NULL flux; a label no point carries gives +0.
 *   One host synchronisation.
 * mg3d_field_energy:  *energy = 0.5 * h * (sum over the grid edges e = (p, q) of w_e * a_e * (u_q - u_p)^2).  An edge
 *   belongs to its lower end p, which must be no duplicate on any axis; along axis a it runs to x+1, wrapped from N-2 to 0
 *   on a periodic axis, absent at x = N-1 on another; it is LEFT OUT when p lies on a Dirichlet face of another axis (both
 *   ends are boundary data); w_e = 1/2 per Neumann face of another axis p lies on; a_e = 1 or 0.5*(eps_p + eps_q).  Each
 *   term is (w_e * a_e) * ((u_q - u_p) * (u_q - u_p)), a point's three edges are added in i, j, k order; partial sums, fold,
 *   synchronisation as above.  Works with or without a mask (edges inside a body contribute what their u gives).  With
 *   these conventions the discrete Green identity is exact: for u vanishing on the Dirichlet faces
 *       sum_e w_e a_e (u_q - u_p)^2 = - sum_p w(p) u_p (s - D u_p)   over every unknown p, fixed ones included,
 *   so for a grounded box with one body at potential V and a converged solve with d = 0:  W = -1/2 V F.
 * Out of scope: the slab (mg3d_dist_*), fp32 (mg3d32_*) and mg3d_host_* forms; levels below the finest; eps grad u as an
 * output; max |E|; the flux through patches of Dirichlet FACES. */
int mg3d_field_gradient(mg3d_ctx *ctx, double scale, double *gi, double *gj, double *gk); /* dense N^3 host arrays; NULL: component not wanted */
int mg3d_field_gradient_device(mg3d_ctx *ctx, double scale, const mg3d_array *const out[3] /* out[a] NULL: not wanted */, void *stream);
int mg3d_field_flux(mg3d_ctx *ctx, int label, double *flux);
int mg3d_field_energy(mg3d_ctx *ctx, double *energy);

/* ------------------------------------------------------------ particles
 * The two halves of a particle-in-cell or droplet-tracking loop that touch the grid: the GATHER of the potential and its
 * gradient at points (mg3d_field_sample*) and the SCATTER of point charges into the right-hand side (mg3d_deposit*) --
 * on the FINEST level of a single-domain fp64 context, with the context's own periodic wraps, reflected Neumann faces and
 * one-sided differences on Dirichlet faces, in the notation of "Field output" above.  Both are deterministic, and the
 * deposit does not depend on the order of the points either; tests/_particle_ref.py restates both bit for bit.
 *
 * mg3d_vec: a 1-D strided vector in device memory -- element m is ptr[stride*m], stride in ELEMENTS, the index formed in 64
 *   bits.  Three of them are the positions (pos[0] the coordinate along i, pos[1] along j, pos[2] along k): an (M, 3) array
 *   is three vectors of stride 3 whose pointers are one element apart, three separate arrays are three vectors of stride
 *   1.  Checked as mg3d_array is: ptr must be device memory of the context's device, dtype MG3D_F64 or MG3D_F32 (widened
 *   exactly on the way in, rounded to nearest even on the way out), stride >= 0 on input (0: a broadcast) and >= 1 on
 *   output; the library trusts the stride to stay inside the caller's allocation.
 *
 * Locating a point, per axis a with coordinate x (node index <-> coordinate is index*h, as in mg3d_fill_boundary_host):
 *     t = x / h                                               (one IEEE division)
 *     periodic axis : t = t - (double)(N-1) * floor(t / (double)(N-1)); every finite x is inside.  (A t that the rounding
 *                     of these three operations leaves below 0 or above N-1 -- a point within rounding of the period's
 *                     seam, or a coordinate so large that its ulp exceeds h -- is taken to 0 or N-1.)
 *     another axis  : the point is OUTSIDE unless 0 <= t && t <= N-1  (x = 0, -0.0 and x = length are inside)
 *     a coordinate or a quotient t that is not finite makes the point OUTSIDE on any axis
 *     c = (int)floor(t), c = N-2 where it would be larger;  f = t - (double)c;  w0 = 1.0 - f,  w1 = f
 *   The point's cell has the nodes c and c+1 on each axis, with the weights w0 and w1.  A node index that is a duplicate
 *   is read or written at its source: no duplicate of u or d is ever read.
 *
 * mg3d_field_sample_device: for each of `count` points, into element m of the wanted outputs (u_out, grad_out[0..2]; NULL:
 *   not wanted, at least one must be):
 *     u_out       = sum_a wi_a * ( sum_b wj_b * ( sum_c wk_c * u[corner a,b,c] ) )
 *     grad_out[d] = the same nested sum over g_d[corner], g_d exactly what mg3d_field_gradient_device stores at that node
 *                   for component d with this `scale` (cs = scale * (0.5 / h) formed on the host): the trilinear interpolant
 *                   of the nodal gradient, the momentum-conserving gather of PIC codes.  scale = -1: E.
 *   Each sum is (w0*v0) + (w1*v1), left to right, uncontracted.  `scale` does not enter u_out; eps and the mask play no
 *   part.  An OUTSIDE point gets a quiet NaN in every wanted output; no count of them is reported (that would need a
 *   synchronisation).  Read-only in the sense of "Field output": a cycle that has run ahead is finished as
 *   mg3d_download_device finishes it, nothing else changes.  The two-event stream ordering of "Device arrays", no host
 *   synchronisation.  ONE launch serves all wanted outputs (one thread per point, 256 per block, at most
 *   MG3D_PARTICLE_MAX_BLOCKS blocks, each thread striding on); it counts under the kernel timer MG3D_K_PACK.
 *   MG3D_ERR_ARG, nothing written: a NULL context or pos, count < 0 or > 2^40, nothing wanted, a scale that is not finite,
 *   a bad vector.  count == 0: MG3D_OK, nothing launched (the pointers of the vectors are then not looked at).
 * mg3d_deposit_device: ADDS the cloud-in-cell density of `count` point charges q to d of the finest level:
 *       d[p] += scale * nf(p) * (sum_m q_m W_m(p)) / h^3,    W_m(p) = (wi*wj)*wk of point m at node p
 *   nf(p) = 2 per Neumann face p lies on (1, 2, 4 or 8) = 1 / w(p): the node's control volume is a half, a quarter, an
 *   eighth -- the reflected operator sees the mirror charge.  For div(eps grad u) = -rho/eps_0 pass scale = -1/eps_0.
 *   OUTSIDE points and points whose q is not finite add nothing.  Fixed points and Dirichlet points receive their share
 *   like any node: d there is never read, a charge landing on a conductor is absorbed.
 *   The sum is accumulated in 64-bit INTEGERS (integer atomic adds commute: no order to depend on), in four launches:
 *     scan       : A = max |q_m| over the points that are inside with a finite q (an integer atomic max on the bit pattern).
 *                  A == 0 (or no such point): d is not touched.
 *     unit       : E = ilogb(A) + 1, K the smallest integer with count <= 2^K, ue = E + K - 62 -- chosen by the kernels
 *                  from A in device memory, the host never sees it.  No sum can overflow: count * A / 2^ue <= 2^62.
 *     accumulate : per point and corner n = llrint(ldexp(q * ((wi*wj)*wk), -ue)) (to nearest even; the product in this order,
 *                  uncontracted), added to a dense accumulator of one long long per node that the call zeroes first.
 *     apply      : where acc != 0:  d[p] = d[p] + f * ldexp((double)acc, ue),  f = (scale * inv_h3) * nf(p),
 *                  inv_h3 = 1.0 / ((h*h)*h) formed on the host in this order; nodes with acc == 0 are not written.
 *     refresh    : on a context with a periodic axis the duplicates of d are then refreshed from their sources (the launch
 *                  writes nothing while A == 0).
 *   Precision: each contribution is rounded to a multiple of 2^ue <= A * 2^(K-61) -- with 10^6 points 2^-41 of the largest
 *   charge --, eight of them per point: the total charge is conserved to 4 * count * 2^ue (plus the rounding of the weights).
 *   State: exactly mg3d_upload_device's on MG3D_D of the finest level -- a cycle that has run ahead is finished and the next
 *   one starts afresh, d counts as the caller's new values (the zero map is rescanned by the next cycle) -- also when
 *   A == 0 or count == 0 (count == 0 launches nothing).  Stream ordering as above, no host synchronisation.  The
 *   accumulator (N^3 long long in the device layout) is allocated on the first deposit and freed with the context:
 *   MG3D_ERR_ALLOC, nothing changed, when it does not fit.  Kernel timer: scan, accumulate and apply count under
 *   MG3D_K_PACK, 3 launches per call; the duplicate refresh of a periodic context is a fourth.
 *   MG3D_ERR_ARG, nothing changed: the conditions of the sample, or a NULL q.
 * mg3d_field_sample, mg3d_deposit: the same from host arrays -- xyz is count x 3 (x, y, z of point m at xyz[3*m ..]), u and
 *   q hold count doubles, grad count x 3; u or grad may be NULL (not wanted).  They stage through device buffers allocated
 *   for the call (MG3D_ERR_ALLOC, nothing changed, when they do not fit), run the same launches and synchronise once;
 *   the results have the bits of the device forms.
 * Out of scope: the slab (mg3d_dist_*), fp32 (mg3d32_*) and mg3d_host_* forms; higher-order shapes (TSC); a count of the
 * points that were outside (mg3d_particle_sort_device below gives one). */
typedef struct mg3d_vec {
    void *ptr;        /* element 0, device memory of the context's device */
    int dtype;        /* MG3D_F64 / MG3D_F32 */
    long long stride; /* in ELEMENTS */
} mg3d_vec;
int mg3d_field_sample_device(mg3d_ctx *ctx, long long count, const mg3d_vec *const pos[3], double scale,
                             const mg3d_vec *u_out /* NULL: not wanted */,
                             const mg3d_vec *const grad_out[3] /* NULL, or entries NULL: not wanted */, void *stream);
int mg3d_deposit_device(mg3d_ctx *ctx, long long count, const mg3d_vec *const pos[3], const mg3d_vec *q, double scale,
                        void *stream);
int mg3d_field_sample(mg3d_ctx *ctx, long long count, const double *xyz /* count x 3 */, double scale, double *u /* count; NULL: not wanted */,
                      double *grad /* count x 3; NULL: not wanted */);
int mg3d_deposit(mg3d_ctx *ctx, long long count, const double *xyz /* count x 3 */, const double *q /* count */, double scale);

/* The MOVE between gather and scatter: one kick-and-drift step of `count` particles with the context's own boundary word and
 * mask -- periodic axes wrap, Neumann faces reflect (the operator's mirror), Dirichlet faces and labelled conductors
 * retire a particle and count it.  The sampled field never leaves registers.  tests/_push_ref.py restates it bit for bit.
 *
 * Vectors (mg3d_vec, checked as above; overlap between them is the caller's business):
 *     pos[a]  MG3D_F64 only, stride >= 1, updated in place.  (A float position rounded on store can land outside a
 *             reflecting wall: positions stay in double.)
 *     vel[a]  MG3D_F64 or MG3D_F32 (rounded to nearest even on store), stride >= 1, updated in place
 *     qm      MG3D_F64 or MG3D_F32, stride >= 0 (0: one charge-to-mass ratio for all)
 *     fate    MG3D_I32 -- a dtype that this vector and the vectors of the reorder below take, every other call keeps
 *             refusing it --, stride >= 1, read and
 *             written: MG3D_FATE_ALIVE (0), a conductor's label 1..255, MG3D_FATE_FACE + f for face f = 0..5 (ilo, ihi,
 *             jlo, jhi, klo, khi), MG3D_FATE_INVALID.
 * Host constants, formed in this order (N, h of the finest level):
 *     cs = scale*(0.5/h);  gdt[a] = dt*accel[a];  inv = 1.0/(1.0 + drag*dt);  n1 = (double)(N-1);  xper = n1*h;
 *     xhi = xper; while (xhi/h > n1) xhi = nextafter(xhi, 0)      (the largest coordinate known to locate inside; division
 *                                                                   is monotone, so every x <= xhi does)
 * Per particle m whose fate[m] == 0 on entry (any other value: the particle is dead, nothing of it is read further and
 * nothing is written), every operation uncontracted:
 *   1 locate x0 as the sample does.  Not inside: the fate is set, pos and vel are not written, the particle is done.  The
 *     fate is MG3D_FATE_INVALID if a coordinate or its quotient t is not finite; otherwise MG3D_FATE_FACE + 2a (t < 0) or
 *     + 2a+1 (t > N-1) for the first axis a, in i, j, k order, on which the point is outside.
 *   2 gather: E_a = the bits of grad_out[a] of mg3d_field_sample_device at x0 with this `scale` (cs above).
 *   3 kick and drift:  k = qm_m*dt;  v1_a = (v0_a + ((k*E_a) + gdt[a])) * inv;  x1_a = x0_a + (dt*v1_a)
 *     -- dv/dt = (q/m) E + accel - drag*v with the drag taken implicitly.  If k, a v1_a or an x1_a is not finite the fate is
 *     MG3D_FATE_INVALID and nothing else is written.
 *   4 walls, per axis a = 0, 1, 2 independently, tt = x1_a/h:
 *       periodic axis          : tt < 0: x1_a = x1_a + xper;  tt >= n1: x1_a = x1_a - xper   (one wrap; the locator wraps the rest)
 *       tt < 0,  Neumann face  : x1_a = -x1_a, v1_a = -v1_a          Dirichlet face: exit through face 2a
 *       tt > n1, Neumann face  : x1_a = xhi - (x1_a - xhi), v1_a = -v1_a    Dirichlet face: exit through face 2a+1
 *     The fate is MG3D_FATE_FACE + f of the first exit in axis order; wraps and reflections on the other axes still apply to
 *     what is stored.  One reflection per axis and step: a particle that moves more than a box length is retired by
 *     step 1 of the next push.  Keeping |v|*dt < h is the caller's job -- a body thinner than the step can be tunnelled.
 *   5 conductors, on a context with a mask and only while the fate is still 0: x1 is located as in step 1 (a point that
 *     is not inside skips this step); the nearest node is n_a = c_a + (w1_a >= 0.5), on a periodic axis N-1 becomes 0; b
 *     is the byte mg3d_ctx_get_mask(finest) returns at that node; b != 0 makes the fate b.
 *   6 stores: the final x1, v1 and -- where it changed -- the fate, also for particles retired in steps 4 and 5: the caller
 *     sees where they hit.  Every transition from 0 to a fate f adds 1 to slot f of a table of MG3D_FATE_SLOTS 64-bit
 *     counters on the device (an integer atomic add: the counts have the same bits in every run and for every order of
 *     the particles), allocated and zeroed with the first push and freed with the context (MG3D_ERR_ALLOC, nothing
 *     changed, when it does not fit).
 * Read-only in the sense of "Field output": a cycle that has run ahead is finished as the sample finishes it, and no field,
 * option, factor or flag changes; sigma, eps and the screening field play no part.  ONE launch per call (the sample's
 * shape: 256 threads, at most MG3D_PARTICLE_MAX_BLOCKS blocks, striding on), counted under MG3D_K_PACK; the two-event
 * stream ordering of "Device arrays", no host synchronisation.  count == 0: MG3D_OK, nothing launched or allocated.
 * MG3D_ERR_ARG, nothing changed: a NULL context, pos, vel, vector or params; count < 0 or > 2^40; dt not finite or <= 0; scale
 * or an accel not finite; drag negative or not finite; a bad dtype or stride; a foreign pointer.
 * mg3d_particle_push: the same on host arrays -- xyz and vxyz count x 3, qm count doubles, fate count ints --, staged
 *   like mg3d_field_sample: one device buffer for the call, one synchronisation, the bits of the device form.
 * mg3d_particle_counts: synchronises once and copies the cumulative table; slot 0 is always 0 and the table is all zero
 *   before the first push; reset != 0 zeroes the table behind the copy.
 * Out of scope: magnetic fields (Boris); charge-weighted tallies (the caller's bincount of fate weighted by q);
 * compaction (mg3d_particle_sort_device below puts the dead last); the slab and fp32 forms. */
enum { MG3D_I32 = 3 };   /* beside MG3D_F64/F32/U8: the fate vector of the push, the fate, perm and data vectors of the reorder; every other call keeps refusing it */
enum { MG3D_FATE_ALIVE = 0,        /* 1..255: absorbed by the conductor whose mask byte is this label */
       MG3D_FATE_FACE = 256,       /* + f, f = 0..5 (ilo, ihi, jlo, jhi, klo, khi): left the box through / lies beyond face f */
       MG3D_FATE_INVALID = 262,    /* a coordinate, velocity, q/m or field value that is not finite */
       MG3D_FATE_SLOTS = 263 };
typedef struct mg3d_push_params {
    double dt;        /* > 0 */
    double scale;     /* the force field is scale * grad u, exactly mg3d_field_sample's grad_out; -1: E = -grad u */
    double accel[3];  /* a constant acceleration (gravity), along i, j, k */
    double drag;      /* gamma >= 0: dv/dt = (q/m) E + accel - gamma v, the drag taken implicitly */
} mg3d_push_params;
int mg3d_particle_push_device(mg3d_ctx *ctx, long long count, const mg3d_vec *const pos[3], const mg3d_vec *const vel[3],
                              const mg3d_vec *qm, const mg3d_vec *fate, const mg3d_push_params *p, void *stream);
int mg3d_particle_push(mg3d_ctx *ctx, long long count, double *xyz, double *vxyz, const double *qm, int *fate,
                       const mg3d_push_params *p);           /* host arrays, count x 3; staged like mg3d_field_sample */
int mg3d_particle_counts(mg3d_ctx *ctx, unsigned long long out[MG3D_FATE_SLOTS], int reset);

/* The REORDER: particles sorted by cell with the library's own locator, the lost and the dead moved behind the living, and
 * every attribute moved in one launch.  The grid kernels above are much faster on points in cell order, and a cloud that
 * starts sorted does not stay so.  tests/_sort_ref.py restates both calls bit for bit.
 *
 * mg3d_particle_sort_device writes into perm the STABLE permutation that sorts the particles by the key K below: perm[m] is
 *   the old index of the particle that belongs at place m.  With N and h of the finest level, c_a the cell index of
 *   "Locating a point" on axis a (periodic wraps included), b_a = c_a >> shift, nb = ((N-2) >> shift) + 1, KMAX = nb*nb*nb:
 *     fate given and fate[m] != 0                           : K = KMAX + 1   (dead; its position is not read)
 *     otherwise, the point is OUTSIDE (not finite included) : K = KMAX       (lost)
 *     otherwise                                             : K = (b_0*nb + b_1)*nb + b_2   (the device layout's order, k fastest)
 *   Equal keys keep the order of their old indices, so the result is unique and has the same bits in every run: the living in
 *   cell order, then the lost, then the dead, the last two groups in their original order.  shift (0 .. 8) sorts by blocks of
 *   2^shift cells per side: fewer key bits, nearly the same locality.  KMAX + 1 must fit 32 bits (nb <= 1625), else MG3D_ERR_ARG.
 *   counts_dev (device memory, checked as every device pointer, or NULL): counts_dev[0] = the particles with K < KMAX,
 *   counts_dev[1] = those with K == KMAX.
 *   Vectors: pos[a] MG3D_F64 or MG3D_F32 (widened exactly), stride >= 0; fate MG3D_I32, stride >= 0, read only, NULL: all alive;
 *   perm MG3D_I32, stride >= 1, written.  0 <= count <= 2^31 - 1; count == 0: MG3D_OK, nothing launched, counts_dev not written.
 *   State: reads the geometry (N, h, the boundary word) and no field; a cycle that has run ahead is NOT finished, the next
 *   mg3d_vcycle gives the bits it would have given.  The two-event stream ordering of "Device arrays", no host
 *   synchronisation: the number of passes depends on KMAX + 2 alone, no launch decision on device data.
 *   The sort: a key launch, then a least-significant-digit radix sort with 8-bit digits, P = ceil(B / 8) passes for the B bits
 *   of KMAX + 1, three launches a pass (digit counts per tile of 2048 elements -- a constant, whatever the grid --, an
 *   exclusive scan of the [digit][tile] table, a stable scatter whose places are prefix + rank, the ranks from wave ballots
 *   and per-wave counts in LDS; no atomic decides a place): 1 + 3*P launches under MG3D_K_PACK (4, 7, 10 or 13).
 *   Scratch: two key and two index buffers and the digit tables, 16*count + 1024*(ceil(count/2048) + 1) bytes, allocated on
 *   first use, re-allocated when count grows (the one moment the call may wait for the device), freed with the context;
 *   MG3D_ERR_ALLOC, nothing changed, when they do not fit.
 *   MG3D_ERR_ARG, nothing written or launched: a NULL context, pos or perm; count out of range; shift outside 0 .. 8; keys
 *   past 32 bits; a bad dtype or stride; a foreign pointer.
 * mg3d_particle_permute_device: dst[v][m] = src[v][perm[m]] for every v < nvec (1 .. MG3D_PERMUTE_MAX_VECS) and m < count, ONE
 *   launch under MG3D_K_PACK that reads perm once.  Each pair (src[v], dst[v]) has one dtype out of MG3D_F64, MG3D_F32,
 *   MG3D_I32; the bytes are copied as they are (-0.0 and NaN payloads survive).  src stride >= 0, dst stride >= 1; out of
 *   place, overlap is the caller's business.  A perm[m] outside 0 .. count-1 writes nothing for that m and reads nothing out
 *   of bounds.  Stream ordering as above; count == 0 launches nothing.  MG3D_ERR_ARG, nothing written: a NULL argument, a
 *   bad nvec, a dtype mismatch in a pair, a bad stride, a foreign pointer, count < 0 or > 2^31 - 1.
 * mg3d_particle_sort: the sort on host arrays -- xyz count x 3, fate count ints or NULL, perm count ints, counts 2 entries
 *   or NULL --, staged like mg3d_field_sample: one synchronisation, the bits of the device form.
 * Out of scope: sorting in place; 64-bit permutations; the sorted keys or per-cell ranges; the slab and fp32 forms. */
enum { MG3D_PERMUTE_MAX_VECS = 16 };
int mg3d_particle_sort_device(mg3d_ctx *ctx, long long count, const mg3d_vec *const pos[3],
                              const mg3d_vec *fate /* MG3D_I32, read only; NULL: all alive */, int shift,
                              const mg3d_vec *perm /* MG3D_I32, stride >= 1, written */,
                              long long *counts_dev /* 2 entries in device memory, or NULL */, void *stream);
int mg3d_particle_permute_device(mg3d_ctx *ctx, long long count, const mg3d_vec *perm /* MG3D_I32 */, int nvec,
                                 const mg3d_vec *const *src, const mg3d_vec *const *dst, void *stream);
int mg3d_particle_sort(mg3d_ctx *ctx, long long count, const double *xyz /* count x 3 */, const int *fate /* or NULL */,
                       int shift, int *perm /* count */, long long *counts /* 2, or NULL */);

/* ------------------------------------------------ operators on device levels
 * mg3d_smooth     : preSmoother (post=0, mg_3d.h:640-709: iters x red,black)
 *                   postSmoother (post=1, mg_3d.h:711-781: iters x black,red)
 * mg3d_residual   : calculateResidual (mg_3d.h:794-842); store!=0 writes r on
 *                   the interior; *norm = sqrt(sum diff^2) (may be NULL)
 * mg3d_restrict   : restrictResidual r[level] -> d[level-1] (mg_3d.h:844-998)
 * mg3d_prolong    : prolongateAndCorrectError u[level-1] -> u[level] (mg_3d.h:1000-1145)
 * mg3d_coarse_solve: solveWithLU(LU, n, d[0], u[0]) (gauss_elim.h:31-60)
 * mg3d_l2norm     : GetL2NormOfVector over all N^3 entries (mg_3d.h:783-792) */
int mg3d_smooth(mg3d_ctx *ctx, int level, int post, int iters);
int mg3d_residual(mg3d_ctx *ctx, int level, int store, double *norm);
/* smoother followed by the residual of its result, as vcycle does back to back (mg_3d.h:1282+1294,
 * 1341+1354), in ONE pass over the level (fused sweep kernel) */
int mg3d_smooth_residual(mg3d_ctx *ctx, int level, int post, int iters, int store, double *norm);
/* smoother, residual and restriction of it into d[level-1] (mg_3d.h:1282+1294+1310) without storing r */
int mg3d_smooth_restrict(mg3d_ctx *ctx, int level, int iters);
int mg3d_restrict(mg3d_ctx *ctx, int level);
int mg3d_prolong(mg3d_ctx *ctx, int level);
int mg3d_coarse_solve(mg3d_ctx *ctx);
int mg3d_l2norm(mg3d_ctx *ctx, int field, int level, double *norm);

/* One V-cycle from `level` down (vcycle, mg_3d.h:1242-1362); *norm receives the
 * post-smoothing residual norm of `level` (the value SolverLinSolve returns,
 * mg_3d.h:1415-1420).  mg3d_vcycles runs `count` cycles from the finest level
 * back to back with a single host synchronisation at the end.
 * Consecutive V(2,2) cycles from a finest level of at least 257^3 share a launch ("carried cycles"): the
 * first red pre-smoothing pass of a cycle that follows another one is the identity, so a cycle's last two post-smoothing
 * passes, its norm and the next cycle's pre-smoothing passes run as one launch.  mg3d_vcycles does so inside a call;
 * mg3d_vcycle(finest level) ends ahead of itself, and every other entry point first restores the finished cycle's own u
 * (every grid value -- u, d, r of every level -- is that of separate cycles, bit for bit; the returned norm sums the same
 * squares in another grouping of per-block partial sums and agrees to the summation tolerance, <= 1e-13 relative against
 * the exactly rounded sum: tests/test_gpu_parity.py; MG3D_NO_CARRY=1 switches it off).
 * From 160 points per side (options legs, legs_min; round 4) the finest level runs ONE launch per leg instead --
 * prolongation + four passes, three passes + residual + restriction -- with the norm's two halves taken from the launches
 * on either side of it; behind a single mg3d_vcycle the next cycle's down-leg runs ahead into spare buffers and is swapped
 * back when anything else is asked (csrc/mg3d_ctx.hip, mg3d_can_legs).  Same bits; option legs = 0 keeps the carried cycles. */
int mg3d_vcycle(mg3d_ctx *ctx, int level, double *norm);
int mg3d_vcycles(mg3d_ctx *ctx, int count, double *norms);

/* Solving to a tolerance: conjugate gradients preconditioned by one V-cycle per iteration, for the finest level's system
 * A u = d of the context's operator -- constant, sigma, eps, periodic axes.  The cycle is a symmetric preconditioner
 * (red,black before and black,red behind the coarse correction, the restriction 1/8 of the prolongation's transpose, every
 * level's operator symmetric with arithmetic face means, a zero guess below the finest level), and where the cycle's own
 * factor degrades on a jump in eps ("Variable coefficient") the Krylov iteration keeps 0.07 - 0.21 per
 * iteration.  A is negative definite: CG runs on -A with z = -(one V-cycle from a zero guess with right-hand side r), signs
 * carried through; beta is Fletcher-Reeves, (r_{k+1}.z_{k+1}) / (r_k.z_k).
 *   in : u of the finest level as uploaded -- Dirichlet values on its faces, any interior: the guess; d of the finest level:
 *        the right-hand side; the coarse factor set as for mg3d_vcycle (MG3D_ERR_STATE without one).  A cycle that has run
 *        ahead is finished first.
 *   out: u holds the iterate, its Dirichlet faces the caller's values bit for bit, on a periodic context its duplicates
 *        equal to their sources; d of the finest level is the caller's bit for bit.  u and d of the lower levels and r of
 *        every level are unspecified.  The context is usable for mg3d_vcycle(s) as before: mg3d_vcycles(1) from the
 *        returned u gives, bit for bit, what a context gives that had this u and d uploaded.
 * The V-cycles inside go through the context's own cycle code with whatever schedule its options select (grid values never
 * depend on them).  Norms are Euclidean over the unknowns: every unique non-Dirichlet point once, the set mg3d_residual
 * counts; r_0 = d - A u of the guess is computed, the later ones are the recurrence's.  The solve stops when
 * ||r_k|| <= max(rtol * ||r_0||, atol) (converged = 1; also at once when the guess satisfies it, r_0 = 0 included), after
 * max_iters iterations, or on breakdown -- p.Ap or r.z not finite or of the wrong sign: the last good iterate stays in u,
 * converged = 0, MG3D_OK.  norms, if not NULL, has max_iters + 1 entries and receives ||r_0|| .. ||r_iterations||.
 * rtol, atol >= 0 and finite, max_iters >= 0, not all three 0 -- otherwise MG3D_ERR_ARG and nothing changes.  max_iters = 0
 * computes r0_norm only and changes nothing.  Sums are per-block partial sums folded in a fixed order: the same call on the
 * same data gives the same bits.  Four work vectors of the finest level's size are allocated on the first call with
 * max_iters > 0 and freed with the context (MG3D_ERR_ALLOC, nothing changed, when they do not fit).
 * Refused with MG3D_ERR_STATE, nothing changed: a context with a Neumann face (the reflected operator is not symmetric in
 * the Euclidean inner product -- see its left null vector w above: it is self-adjoint only in the w-weighted one); the
 * singular case, every axis periodic with sigma = 0 (the pinned row of the coarse matrix breaks the symmetry of the
 * preconditioner); a context after mg3d_es_setup.  The slab, fp32 and mg3d_host_* forms have no such entry point.
 * Use it with a coefficient that jumps; for the constant operator mg3d_vcycles converges at 0.16 per 2 ms cycle and the
 * extra passes of an iteration cost more than they save ("Solving to a tolerance").  mg3d_wpcg_solve below
 * solves the two refused cases, Neumann faces and the singular operator, in the weighted inner product. */
typedef struct mg3d_pcg_info {
    int iterations;        /* preconditioned iterations performed (updates of u; on breakdown one V-cycle more was run) */
    int converged;         /* 1: ||r_k|| <= max(rtol*||r_0||, atol) was reached */
    double r0_norm;        /* ||d - A u|| of the guess the caller uploaded */
    double r_norm;         /* recurrence residual norm at return */
} mg3d_pcg_info;
int mg3d_pcg_solve(mg3d_ctx *ctx, double rtol, double atol, int max_iters,
                   double *norms /* NULL or max_iters+1 entries: r_0 .. r_k */,
                   mg3d_pcg_info *info /* may be NULL */);

/* The same iteration in the weighted inner product <a, b>_w = sum of w*a*b over the unknowns, w = 1/2 per Neumann face a
 * point lies on and 1 otherwise (the weights of mg3d_ctx_set_neumann's compatibility condition; computed from the point's
 * index inside the kernels, a power of two: the products are exact).  The reflected operator is self-adjoint in it and so
 * is the cycle, so conjugate gradients apply where mg3d_pcg_solve refuses, and where plain cycles on a jumping eps between
 * Neumann faces do not merely slow down but grow ("Weighted PCG").
 * Everything mg3d_pcg_solve states about in, out, state, arguments, breakdown, determinism and work vectors holds, except:
 *   accepted : every context mg3d_pcg_solve accepts -- the call is then that one, the same u and norms bit for bit; any
 *              mask of Neumann faces beside periodic axes, sigma and eps; the singular case (every axis periodic or Neumann
 *              on both faces, sigma = 0) with or without a Neumann face.  Refused with MG3D_ERR_STATE, nothing changed: a
 *              context after mg3d_es_setup, one without a coarse factor.
 *   dots     : r.z and p.Ap are weighted; alpha, beta and the sign tests are mg3d_pcg_solve's (A stays negative
 *              (semi)definite).  Norms, r0_norm, r_norm and the stopping test stay Euclidean over the unknowns, the
 *              quantity mg3d_residual returns.
 *   singular : the system is solved on the subspace of w-mean zero.  With W = sum of w: r_0 = (d - A u) - sum(w (d - A u))/W,
 *              every z has sum(w z)/W taken out as it enters the direction, r is not projected again.  d is never written;
 *              rhs_mean reports sum(w d)/W, the part of d that was projected out -- not 0 (to rounding) means the caller's
 *              right-hand side is incompatible and the solution returned is that of d - rhs_mean.  u keeps the w-mean of the
 *              guess up to rounding.  The norms are those of the projected residual: mg3d_residual of the returned u agrees
 *              with r_norm when d is compatible, and after its w-mean is taken out otherwise.  The work vectors are
 *              allocated also with max_iters = 0.
 * Points of u on a Neumann face that also lie on a Dirichlet face are Dirichlet points: untouched. */
typedef struct mg3d_wpcg_info {
    int iterations, converged;
    double r0_norm, r_norm; /* as mg3d_pcg_info */
    int singular;           /* 1: the projected system was solved */
    double rhs_mean;        /* singular: sum(w*d)/sum(w) over the unknowns, the part of d that was projected out; else 0 */
} mg3d_wpcg_info;
int mg3d_wpcg_solve(mg3d_ctx *ctx, double rtol, double atol, int max_iters,
                    double *norms /* NULL or max_iters+1 entries: r_0 .. r_k */,
                    mg3d_wpcg_info *info /* may be NULL */);

/* Full-multigrid initialisation, SolverFMGInitialize (mg_dirichlet_analytic.c:771-806; commented copy
 * mg_3d.h:1364-1404): BCs on u[0], direct solve, then for every level prolong the coarser solution, impose the
 * Dirichlet values BCFunc on the six faces (on the device), zero the coarser level, one V-cycle from that level. */
int mg3d_fmg_initialize(mg3d_ctx *ctx);
/* Full multigrid for the CALLER's problem: the finest level's d and Dirichlet values, on every operator the context
 * supports (constant, sigma, eps, any periodic mask, any Neumann mask).  mg3d_fmg_initialize above stays what the reference
 * is -- one analytic test problem, Dirichlet faces only, and its interpolated guess is discarded below the finest level.
 *   in : u of the finest level as uploaded -- only its Dirichlet points AND its fixed points (mg3d_ctx_set_mask under
 *        MG3D_MASK_KEEP) are read, whatever else it holds is ignored; d of the finest level (never read at a fixed point: it
 *        may hold anything there, NaN included); the coarse factor set as for mg3d_vcycle; cycles >= 1, otherwise
 *        MG3D_ERR_ARG and nothing changes.  A cycle that has run ahead is finished first.
 *   1. for l = L-1 .. 1: d[l-1] = the context's own restriction of d[l] (full weighting of the unknowns; Dirichlet points
 *      are injected and never enter a weighted sum, so the caller need not define d there), u[l-1] = injection of u[l]
 *      (u[l-1][I,J,K] = u[l][2I,2J,2K]: the Dirichlet values); then d[0] = u[0] at every Dirichlet point of level 0, the
 *      right-hand side of the direct solve's identity rows
 *   2. level 0: the direct solve, duplicates and the pinned row as in a cycle
 *   3. for l = 1 .. L-1: mg3d_fmg_interpolate(l), then `cycles` V-cycles from level l that keep u[l] as their guess (the
 *      levels below l start from zero as in every cycle); on l = L-1 they are mg3d_vcycles(cycles), schedules included
 *   With fixed points: in 1. d[l] counts as 0. at the fixed unknowns of level l (the bits of restricting a copy with zeros
 *      stored there), and a coarse point C that is a fixed unknown of level l-1 while m_l[2C] == 0 -- it stands for a lost fine
 *      point F, step 2 of mg3d_ctx_set_mask_coarsening -- takes u[l][F] instead of u[l][2C], so each level's body carries its
 *      conductor's potential; in 2. the identity rows of level 0's fixed unknowns take u[0] there, as the Dirichlet points
 *      do; in 3. the interpolation does not write a fixed unknown of the fine level and reads coarse fixed points like any
 *      other value.
 *   out: u of the finest level holds the result, its Dirichlet points and fixed points the caller's bit for bit, its periodic duplicates
 *        equal to their sources; d of the finest level is the caller's bit for bit; *norm (may be NULL) is the residual
 *        norm after the last finest-level cycle, the value mg3d_vcycles returns.  u and d of the lower levels and r are
 *        unspecified.  The context is usable as before: mg3d_vcycles(1) from the returned u gives, bit for bit, what a
 *        context gives that had this u and d uploaded.
 * With V(2,2) and cycles = 1 the algebraic error of the result is below the discretisation error ("Full
 * multigrid start"): what six or seven cycles from a zero guess do.  The singular case has mg3d_vcycle's caveat: nothing
 * is projected, d must be compatible, u is fixed by the pin.
 * mg3d_fmg_interpolate: u[level] at every unknown (and its periodic duplicates) is OVERWRITTEN with the interpolant of
 * u[level-1]; Dirichlet points and fixed points of u[level] are never written, those of u[level-1] are read like any other
 * point.  Per
 * axis (coarse side Nc): an even fine index 2I copies coarse I; an odd one, 2I+1, takes coarse I-1, I, I+1, I+2 with
 * -1/16, 9/16, 9/16, -1/16 -- an index outside the unique range wrapped modulo Nc-1 on a periodic axis, reflected at a
 * Neumann face (-1 -> 1, Nc -> Nc-2); next to a Dirichlet face the one-sided cubic over the four points nearest the face
 * (low: coarse 0, 1, 2, 3 with 5/16, 15/16, -5/16, 1/16; high: coarse Nc-4 .. Nc-1 with 1/16, -5/16, 15/16, 5/16); with
 * Nc < 4 coarse I, I+1 with 1/2, 1/2.  The value is the tensor product sum_i(wi * sum_j(wj * sum_k(wk * u))), each sum
 * left to right in the order given, uncontracted (tests/_fmg_ref.py restates it bit for bit).  1 <= level < L, otherwise
 * MG3D_ERR_ARG.
 * Both return MG3D_ERR_STATE, nothing changed, on a context without a coarse factor, after mg3d_es_setup, or with a mask
 * coarsened by injection (MG3D_MASK_INJECT, the default; the message names mg3d_ctx_set_mask_coarsening).  The slab,
 * fp32 and mg3d_host_* forms have no such entry points. */
int mg3d_fmg_interpolate(mg3d_ctx *ctx, int level);
int mg3d_fmg_solve(mg3d_ctx *ctx, int cycles, double *norm /* may be NULL */);

/* Implicit time stepping on the device: the theta-scheme for
 *     u_t = div(eps grad u) - kappa u + s        (kappa >= 0 constant; s an optional source held on the device)
 * with the context's operator (constant or eps) and boundaries: Dirichlet values are whatever the Dirichlet points of u
 * hold -- fixed in time, never written --, periodic axes as set, Neumann faces homogeneous.  A prescribed flux is folded
 * into the source by the caller: s = -fold_flux(-s) (mg3d_neumann_fold_flux subtracts 2 a g / h from what it is given).
 * With L the operator at sigma = 0, one step of length dt, 1/2 <= theta <= 1 (1: backward Euler, 1/2: Crank-Nicolson), is
 *     (u1 - u0)/dt = theta (L - kappa) u1 + (1 - theta)(L - kappa) u0 + s
 * and, divided by theta, the system  A_sigma u1 = d  of the context's operator at sigma = kappa + 1/(theta*dt), where
 *     q    = A_sigma u0 = invHsq*(S - dg*u0)     the expression, operand order and neighbour order of mg3d_pcg_solve's A p
 *     d[p] = -((a*u0[p] + c1*q[p]) + b*s[p])     at every unknown (the set mg3d_residual counts)
 *     c0 = 1.0/(theta*dt);  a = c0/theta;  c1 = (1.0 - theta)/theta;  b = 1.0/theta      (host, double, in this order)
 * (L u0 - kappa u0 = q + c0 u0 and 1 + c1 = 1/theta).  Without a source the b*s term is absent, d = -(a*u0 + c1*q); with
 * theta == 1.0 exactly c1 = 0 and q is not computed, d = -(a*u0 + b*s), or -(a*u0).  Uncontracted: tests/_step_ref.py
 * restates d bit for bit.  d is written at the unknowns only: its Dirichlet points and periodic duplicates keep what they
 * hold.  Nothing but the norms crosses to the host.
 * mg3d_step_setup: dt > 0, 0.5 <= theta <= 1, kappa >= 0, all finite (and their sigma finite), otherwise MG3D_ERR_ARG and
 *   nothing changes.  Sets the context's shift to kappa + 1/(theta*dt) as mg3d_ctx_set_shift does -- a cycle that has run
 *   ahead is finished first, a factor of mg3d_ctx_build_coarse is rebuilt, one of mg3d_ctx_set_lu dropped -- and stores
 *   dt, theta, kappa.  Call it again for another dt.
 * mg3d_step_set_source: s of the finest level, a dense N^3 host array, uploaded into a field of the library's own that is
 *   allocated on the first call and freed with the context (MG3D_ERR_ALLOC, nothing changed, when it does not fit); NULL
 *   drops the source.  May be called between mg3d_step_advance calls, for a source that changes in time.  Values of s at
 *   Dirichlet points and duplicates are never used.
 * mg3d_step_advance: nsteps steps from u of the finest level.  Per step: a cycle that has run ahead is finished; d is
 *   formed in one launch; the system is solved with u as it stands as the guess --
 *     MG3D_STEP_VCYCLES  cycles >= 1 V-cycles, exactly mg3d_vcycles(cycles), schedules included; the step's norm is the last
 *                        cycle's; rtol is ignored; iterations and converged stay 0
 *     MG3D_STEP_WPCG     mg3d_wpcg_solve(rtol, 0, cycles): at most `cycles` iterations; the step's norm is its r_norm;
 *                        iterations accumulates over the steps, converged is 1 only if every step converged (sigma > 0:
 *                        the operator is never singular)
 *   norms, if not NULL, receives one norm per step; time is steps*dt of this call.
 *   out: u of the finest level holds u at the new time, its Dirichlet points the caller's bit for bit, its periodic
 *        duplicates equal to their sources; d of the finest level holds the last step's right-hand side; the lower levels
 *        and r are unspecified.  The context is usable as before: mg3d_vcycles(1) afterwards gives, bit for bit, what a
 *        context gives that had this u, d and sigma set.
 *   MG3D_ERR_ARG, nothing changed: nsteps < 0, a method that is neither, cycles < 1, MG3D_STEP_WPCG with an rtol that is
 *   negative or not finite.  MG3D_ERR_STATE, nothing changed: mg3d_step_setup was never called; the context's sigma is no
 *   longer the one it set (mg3d_ctx_set_shift since); no coarse factor.  A context after mg3d_es_setup is refused through
 *   these three: mg3d_es_setup needs sigma = 0, and the shift of mg3d_step_setup, which is > 0, drops its factor.
 *   nsteps = 0 changes nothing.  A HIP error (or MG3D_ERR_ALLOC from the first MG3D_STEP_WPCG step's work vectors) is returned as it is;
 *   info->steps says how many steps completed.
 * The slab (mg3d_dist_*), fp32 (mg3d32_*) and mg3d_host_* forms have no stepper: single domain only. */
enum { MG3D_STEP_VCYCLES = 0, MG3D_STEP_WPCG = 1 };
typedef struct mg3d_step_info {
    int steps;       /* steps completed by this call */
    int iterations;  /* MG3D_STEP_WPCG: iterations over all steps */
    int converged;   /* MG3D_STEP_WPCG: 1 when every step reached rtol */
    double time;     /* steps * dt */
} mg3d_step_info;
int mg3d_step_setup(mg3d_ctx *ctx, double dt, double theta, double kappa);
int mg3d_step_set_source(mg3d_ctx *ctx, const double *s /* finest level, dense N^3 host; NULL: no source */);
int mg3d_step_advance(mg3d_ctx *ctx, int nsteps, int method, int cycles, double rtol,
                      double *norms /* NULL or nsteps entries */, mg3d_step_info *info /* may be NULL */);

/* ------------------------------------------------------------ nonlinear solves
 * Damped Newton-multigrid on the device for
 *     A u - g0 * g(x) * phi(beta*(u - uref)) = d
 * with A the context's linear operator and boundaries as set (constant or eps, sigma, periodic axes, Neumann faces, mask),
 * phi = exp (MG3D_NL_EXP: Boltzmann electrons, div(eps grad u) - g exp(beta (u - uref)) = -rho_i/eps0) or phi = sinh
 * (MG3D_NL_SINH: Poisson-Boltzmann, Delta u - kappa^2 sinh u = f), g0 >= 0, beta > 0 and uref finite scalars, g >= 0 an
 * optional weight per point (none: 1).  d and the Dirichlet values of u are the caller's, as for every solve; a prescribed
 * Neumann flux is folded into d (mg3d_neumann_fold_flux).  Finest level of a single-domain fp64 context.
 * The evaluation, one launch on the residual's column walk; per unknown, uncontracted and in this order:
 *     w   = beta*(u[p] - uref)
 *     ph  = exp(w), dph = ph      or      ph = sinh(w), dph = cosh(w)      (the device library's double functions)
 *     gp  = g0*g[p]                                                        (no weight: gp = g0)
 *     lin = d[p] - invHsq*(S - dg*u[p])      mg3d_residual's expression for the operator at sigma WITHOUT a screening field
 *     F   = lin + gp*ph                      the nonlinear residual
 *     s   = (gp*beta)*dph                    the screening field of the linearisation, A - s
 * F and s are 0. at fixed points.  tests/_nl_ref.py restates it in numpy.
 * mg3d_nl_setup: kind MG3D_NL_EXP or MG3D_NL_SINH, g0 >= 0, beta > 0, all three finite; otherwise MG3D_ERR_ARG and nothing
 *   changes.  Stores the four; call it again for other values.  Touches neither fields nor the factor.
 * mg3d_nl_set_weight: g of the finest level, a dense N^3 host array, every entry finite and >= 0, checked as
 *   mg3d_ctx_set_shift_field checks its own (periodic duplicates skipped; MG3D_ERR_ARG names the lowest bad index), uploaded
 *   into a field of the library's own that is allocated on the first call and freed with the context (MG3D_ERR_ALLOC, nothing
 *   changed, when it does not fit); NULL drops the weight.  Values at Dirichlet points and duplicates are never used.
 * mg3d_nl_set_weight_device: the same from a device array, MG3D_F64 or MG3D_F32, any strides >= 0, checked on the device
 *   (one host synchronisation), packed on the context's stream behind what the caller's stream did to the array.
 * mg3d_nl_residual: F at every unknown of the finest level from u and d as they stand; *norm (may be NULL) = sqrt of the sum
 *   of F^2, per-block partial sums folded in a fixed order as mg3d_residual's; store != 0: F goes into r of the finest level,
 *   duplicates written, Dirichlet and fixed points keep / get 0. as under mg3d_residual.  With g0 = 0 it is mg3d_residual of a
 *   context without a screening field, bit for bit.  A screening field on the context (mg3d_nl_solve leaves one) is NOT part of
 *   A here.  Read-only otherwise (a cycle that has run ahead is finished first).  MG3D_ERR_STATE without mg3d_nl_setup.
 * mg3d_nl_solve: inexact Newton in correction form with backtracking on ||F||, from u of the finest level:
 *     x := u, f := d                        (fields of the library's own, allocated before the first write)
 *     evaluate at x -> F into d, s into the screening field's finest level, n := ||F||; norm0 := n
 *     repeat up to max_newton times, stopping when n <= max(atol, rtol*norm0):
 *         install s: restrict it down the hierarchy and rebuild the coarse factor, what mg3d_ctx_set_shift_field_device does
 *                    behind its pack
 *         u := 0 everywhere; solve (A - s) delta = F by
 *             MG3D_STEP_VCYCLES  mg3d_vcycles(cycles)                   (rtol_lin ignored)
 *             MG3D_STEP_WPCG     mg3d_wpcg_solve(rtol_lin, 0, cycles)
 *         lambda := 1; up to max_halvings + 1 trials:
 *             t := x + lambda*delta at the unknowns (Dirichlet and fixed points of x copied, duplicates written)
 *             evaluate at t -> F, s, n_t
 *             accept if n_t and every s are finite and n_t < (1 - 1e-4*lambda)*n; else lambda := lambda/2
 *         accepted: x := t, n := n_t;   none accepted: evaluate at x again, stop, converged = 0
 *     on every exit: s(x) installed on all levels; u := x; d := f bit for bit; the lower levels and r are unspecified
 *   norms, if not NULL, has max_newton + 1 entries: norms[0] = norm0, norms[k] = n behind Newton step k.  info (may be NULL):
 *   the counts below.  One host synchronisation per evaluation (the norm and the count of non-finite s) beside those of the
 *   install and of the linear solve.
 *   After the call the context is the linearisation at the solution: mg3d_ctx_has_shift_field reports 1, a cycle solves
 *   (A - s) v = d; mg3d_ctx_set_shift_field(ctx, NULL) drops the field and returns to the context as it was.  A screening
 *   field the CALLER installed is refused (MG3D_ERR_STATE, nothing changed): folding it in is not offered; one left by an
 *   earlier mg3d_nl_solve is overwritten.  max_newton = 0 evaluates, installs s(x) and returns.
 *   MG3D_ERR_ARG, nothing changed: max_newton < 0, a method that is neither, cycles < 1, max_halvings < 0, rtol or atol (or,
 *   with MG3D_STEP_WPCG, rtol_lin) negative or not finite.  MG3D_ERR_STATE, nothing changed: mg3d_nl_setup never called; a
 *   caller's screening field; no coarse factor, or one that mg3d_ctx_build_coarse did not build (every install rebuilds it);
 *   a context after mg3d_es_setup; a linearisation that would be singular -- every axis closed (periodic or Neumann on both
 *   faces), sigma = 0, no fixed unknown and g0*g > 0 at no unknown.  A HIP or allocation error is returned as it is, u and d
 *   put back where that is still possible; info says how far the solve got.
 * The slab (mg3d_dist_*), fp32 (mg3d32_*) and mg3d_host_* forms have no nonlinear solve: single domain, fp64 only. */
enum { MG3D_NL_EXP = 0, MG3D_NL_SINH = 1 };
typedef struct mg3d_nl_info {
    int iterations;        /* Newton steps accepted */
    int converged;         /* 1 when n <= max(atol, rtol*norm0) was reached */
    int halvings;          /* halvings of lambda over all steps */
    int linear_iterations; /* V-cycles (MG3D_STEP_VCYCLES) or CG iterations (MG3D_STEP_WPCG) over all steps */
    double last_lambda;    /* lambda of the last accepted step (0: none) */
    double norm0, norm;    /* ||F|| at the caller's u and at the returned u */
} mg3d_nl_info;
int mg3d_nl_setup(mg3d_ctx *ctx, int kind, double g0, double beta, double uref);
int mg3d_nl_set_weight(mg3d_ctx *ctx, const double *g /* finest level, dense N^3 host; NULL: no weight */);
int mg3d_nl_set_weight_device(mg3d_ctx *ctx, const mg3d_array *g /* NULL: no weight */, void *stream);
int mg3d_nl_residual(mg3d_ctx *ctx, int store, double *norm /* may be NULL */);
int mg3d_nl_solve(mg3d_ctx *ctx, int max_newton, int method, int cycles, double rtol_lin, double rtol, double atol,
                  int max_halvings, double *norms /* NULL or max_newton + 1 entries */, mg3d_nl_info *info /* may be NULL */);
/* setupBoundaryConditions (mg_3d.h:1147-1239) on a device-resident field */
int mg3d_fill_boundary(mg3d_ctx *ctx, int field, int level);

/* Launch and schedule policy of a context, by key.  Defaults, then the environment as an override read ONCE when the
 * context is created, afterwards only this call: nothing on a launch path reads the environment, two contexts of one
 * process may differ.  Grid values never depend on any of them (tests/test_gpu_parity.py, tests/test_gpu_legs.py compare).
 *   key             default  environment at creation   meaning
 *   carry           1        MG3D_NO_CARRY=1 -> 0      consecutive V(2,2) cycles share a launch on the finest level
 *   carry_min       130      MG3D_CARRY_MIN            ... from this many points per side
 *   legs            1        MG3D_LEGS                 one launch per leg on the finest level instead (see above)
 *   legs_min        160      MG3D_LEGS_MIN             ... from this many points per side (below: the carried cycles)
 *   tiny            1        MG3D_NO_TINY=1 -> 0       the level above the coarsest one in one workgroup
 *   tiny_cycle      1        MG3D_NO_TINY_CYCLE=1 -> 0 ... together with the direct solve in one launch
 *   lu_reduced      1        MG3D_LU_REDUCED           install the factor without its identity rows (read per factor)
 *   fuse_rst2       -1       MG3D_FUSE_RST2            2 passes + residual + restriction in one launch: -1 from 130 points
 *                                                      per side, 0 never, 1 always
 *   small_max       129      MG3D_SMALL_MAX            largest level side that runs the two-rows-per-thread shapes
 *   fuse_leg_max    0        MG3D_FUSE_LEG_MAX         largest level side whose legs run as one (two-row) launch each
 *   fuse_up_max     1048576  MG3D_FUSE_UP_MAX          largest level side whose up-leg folds the prolongation into 4 passes
 *                                                      (default: every level; 0: the prolongation is its own launch below the top)
 *   sweep_tune      -1       MG3D_SWEEP_TUNE           first-use measurement of chunk lengths: -1 on unless the process
 *                                                      drives a multi-rank RCCL job, 0 off, 1 on
 *   sweep_tune_log  0        MG3D_SWEEP_TUNE_LOG       print the measured choices
 *   sweep_ci        0        MG3D_SWEEP_CI             > 0: planes per chunk of every fused sweep launch (measurement)
 *   sweep_rj/nw/pf  0        MG3D_SWEEP_CFG="rj,nw,pf" another compiled tile shape (unknown ones fall back to the default)
 *   d_zero_skip     1        MG3D_D_ZERO_SKIP          the fused launches of the finest level do not read the planes of d that
 *                                                      are +0.0 at every interior point (the zero map, below) and, when
 *                                                      that holds for EVERY interior plane, the two leg launches of the
 *                                                      finest level run kernels with no d at all; 2: the map only;
 *                                                      0: every plane is read
 *   zero_front      1        MG3D_ZERO_FRONT           the four-pass launch that starts a coarse level from the zero guess
 *                                                      forms its first pass from d as a plane arrives and runs a three-pass
 *                                                      kernel; 0: the four-pass kernel on an input that is not read
 *   fuse_down_min   130      MG3D_FUSE_DOWN_MIN        smallest level side whose V(2,2) down-leg from the zero guess is ONE
 *                                                      launch: the zero front, three passes, the residual and its
 *                                                      restriction (needs zero_front; levels above fuse_leg_max only); 0: never
 * mg3d_option_name(i) enumerates the keys (NULL past the end).  mg3d_dist_set_option forwards to every local rank (carry /
 * carry_min of a multi-rank job are agreed at creation and refuse to change); mg3d32_set_option knows "pairs", "fuse",
 * "carry" (MG3D_F32_NO_PAIRS / _NO_FUSE / _NO_CARRY at creation).  A context with a variable coefficient
 * (mg3d_ctx_set_coefficient) keeps and reports every value, but of these only lu_reduced applies to it: its levels run
 * the coefficient kernels, never the fused, carried, per-leg or single-workgroup schedules. */
int mg3d_ctx_set_option(mg3d_ctx *ctx, const char *key, int value);
int mg3d_ctx_get_option(const mg3d_ctx *ctx, const char *key, int *value);
const char *mg3d_option_name(int index);
/* The zero map.  A source-free problem (d = 0 inside the domain: a Laplace problem with boundary values, conductors, fixed
 * potentials) or a localised source leaves most planes i = const of the finest level's d at +0.0 in every interior point.
 * The context keeps one bit per plane saying so, and the fused launches of the finest level form such a plane's d in
 * registers instead of reading it: the same bits -- -0.0, denormals and NaNs count as non-zero, faces are not looked at
 * (no face entry of d enters a value the fused kernels store) --, a read of the level less per launch.  mg3d_zero sets every
 * bit; mg3d_fill_boundary leaves the map alone; mg3d_upload / mg3d_upload_device have the next cycle scan the new d once
 * (one pass over it and one host synchronisation per upload, none per cycle); mg3d_step_advance, mg3d_pcg_solve /
 * mg3d_wpcg_solve and mg3d_device_view of that d switch the map off (the last for good, as the run-ahead of mg3d_vcycle).
 * Contexts with a variable coefficient, periodic axes, Neumann faces or fixed points never use it.
 * mg3d_ctx_dzero_planes: how many planes the map holds (0 unless it is valid) and its state -- 0 off, 1 to be scanned by
 * the next cycle, 2 valid; either pointer may be NULL.  For tests and tools. */
int mg3d_ctx_dzero_planes(const mg3d_ctx *ctx, int *planes, int *state);
/* mg3d_ctx_dnone_launches: how many launches of this context have run a kernel without d because the map was full
 * (d_zero_skip = 1, d +0.0 at every interior point of the finest level: the flagship problem, every source-free one).  The
 * same bits as with the map alone or without it: h^2 * (+0.0) is +0.0, x - (+0.0) is x.  For tests and tools. */
int mg3d_ctx_dnone_launches(const mg3d_ctx *ctx, unsigned long long *launches);
/* mg3d_ctx_sweep_taken: which fused sweep launches this context has taken -- a record the launcher writes on the host when
 * it launches; no kernel knows of it.  Grid values never depend on the chunk length or on the tile shape (options sweep_ci,
 * sweep_rj/nw/pf), and a request that names no compiled shape runs the default one: this is how a test or an A/B tool sees
 * what ran.  Per kind of launch the context keeps the DISTINCT records, the most recent first (at most 32 of a kind; the one
 * used longest ago is dropped): `which` = 0 is the kind's last launch, 1 the distinct one before it, ...  out receives the
 * MG3D_SWEEP_TAKEN_FIELDS ints named below, *count how many launches had exactly this record, *launches every launch of the
 * kind (either may be NULL).  Past the end of the list out is zeroed and *count is 0.  MG3D_ERR_ARG: no such kind, a
 * negative index, NULL ctx or out.  The slab path (mg3d_dist_*) and the fp32 solver keep no records.  For tests and tools.
 *   kinds:  PASSES colour passes alone; PASSES_RES ... with the residual (norm, r, or its restriction); TAP the launch two
 *           carried cycles share; LEG_DOWN / LEG_UP the one-launch legs
 *   fields: S colour passes, RES 0 none / 1 residual / 2 residual restricted / 3 norm tapped after the second pass, RJ rows a
 *           thread, NW waves, PF planes in flight, ND the kernel without d, DZ the kernel that reads d through its zero
 *           map, CI planes per chunk, BLOCKS of the grid, XCD_REMAP 0 blocks as numbered / 1 the whole grid regrouped / 2
 *           every chunk's layer regrouped, NTJ x NTK tiles, PRO prolongation in the loads, RST 0 the norm-only residual,
 *           DP slots of the d window parked in LDS, TAP the colour pass behind which a half of the norm is formed (-1 none), N points per side
 *           of the level */
enum { MG3D_SWEEP_KIND_PASSES = 0, MG3D_SWEEP_KIND_PASSES_RES, MG3D_SWEEP_KIND_TAP, MG3D_SWEEP_KIND_LEG_DOWN, MG3D_SWEEP_KIND_LEG_UP };
enum {
    MG3D_SWEEP_TAKEN_S = 0, MG3D_SWEEP_TAKEN_RES, MG3D_SWEEP_TAKEN_RJ, MG3D_SWEEP_TAKEN_NW, MG3D_SWEEP_TAKEN_PF,
    MG3D_SWEEP_TAKEN_ND, MG3D_SWEEP_TAKEN_DZ, MG3D_SWEEP_TAKEN_CI, MG3D_SWEEP_TAKEN_BLOCKS, MG3D_SWEEP_TAKEN_XCD_REMAP,
    MG3D_SWEEP_TAKEN_NTJ, MG3D_SWEEP_TAKEN_NTK, MG3D_SWEEP_TAKEN_PRO, MG3D_SWEEP_TAKEN_RST, MG3D_SWEEP_TAKEN_DP,
    MG3D_SWEEP_TAKEN_TAP, MG3D_SWEEP_TAKEN_N, MG3D_SWEEP_TAKEN_FIELDS
};
int mg3d_ctx_sweep_taken(const mg3d_ctx *ctx, int kind, int which, int out[MG3D_SWEEP_TAKEN_FIELDS],
                         unsigned long long *count, unsigned long long *launches);

/* per-stage timers (timing_info.h:6-47), filled from hipEvent pairs recorded in-stream (no stall).
 * on: 0 = off, 1 = every level, 2 = finest level only, 3 = the kernel timers of the finest level only (no stage
 * timers: a third of the marker packets, what bench.py's roofline object needs), 4 + k = as 3 on every (k+2)-th full
 * cycle only (a sample of the timed region: each marker costs ~5 us of idle queue). */
int mg3d_timing_enable(mg3d_ctx *ctx, int on);
int mg3d_timing_reset(mg3d_ctx *ctx);
int mg3d_timing_get(mg3d_ctx *ctx, int level, int stage, int *num_calls, double *seconds);
/* diagnostic: phase stamps (100 MHz clock) of the last single-workgroup coarse cycle launch (csrc/mg3d_tiny.hip):
 * start, d loaded, pre-smoothed, residual, restricted, solve start, solve end, correction ready, prolonged, post-smoothed, stored */
int mg3d_debug_tiny_stamps(long long *out16);
/* per-kernel timers, same mechanism, one event pair around each launch of the kernels below */
enum {
    MG3D_K_SWEEP4 = 0,   /* fused sweep, 4 colour passes */
    MG3D_K_SWEEP2,       /* fused sweep, 2 colour passes */
    MG3D_K_SWEEP2_RES,   /* fused sweep, 2 colour passes + residual */
    MG3D_K_RESIDUAL,     /* residual (+ r store) of the current field */
    MG3D_K_RESTRICT, MG3D_K_PROLONG, MG3D_K_COARSE_SOLVE, MG3D_K_COLOUR_PASS,
    MG3D_K_SWEEP4_NORM,     /* carried cycles (mg3d_vcycles): a cycle's last 2 post-smoothing passes, its residual norm and
                               the next cycle's first pre-smoothing passes in one launch */
    MG3D_K_SWEEP1_RESTRICT, /* carried cycles: the last pre-smoothing pass + residual + restriction */
    MG3D_K_LEG_DOWN,        /* one launch per leg: the pre-smoothing passes + residual + restriction */
    MG3D_K_LEG_UP,          /* one launch per leg: prolongation + the post-smoothing passes (+ half of the norm) */
    MG3D_K_PCG_APPLY,       /* mg3d_pcg_solve / mg3d_wpcg_solve: q = A p and its dot (the fold of the partial sums included) */
    MG3D_K_STEP_RHS,        /* mg3d_step_advance: the right-hand side of a step */
    MG3D_K_PACK,            /* device arrays (mg3d_*_device): the pack and unpack launches */
    MG3D_NUM_KERNELS
};
const char *mg3d_kernel_name(int kernel);
int mg3d_kernel_time_get(mg3d_ctx *ctx, int level, int kernel, int *num_launches, double *seconds);

/* ------------------------------------------------------------ mixed boundary conditions ("electrospray")
 * The problem the reference was written for (mg_3d_bkup.c:12-18, 84-133, 739-778): Dirichlet patches on the two x
 * faces -- a capillary disc and an extractor annulus -- and zero-gradient walls everywhere else, imposed by copying a
 * freshly smoothed interior value onto the wall point behind it.  Carried by the live operators of mg_3d.h
 * (csrc/mg3d_es.hip; parity unpinned: the original neither compiles nor is order-independent).  The context must have
 * been created with grid_length == params->length. */
typedef struct mg3d_es_params {
    double length;                  /* side of the cube (GRID_LENGTH, mg_3d_bkup.c:12) */
    double capillary_radius;        /* Dirichlet disc on x = 0 (:14) */
    double extractor_inner_radius;  /* Dirichlet annulus on x = length (:15-16) */
    double extractor_outer_radius;
    double capillary_voltage;       /* (:17) */
    double extractor_voltage;       /* (:18) */
} mg3d_es_params;
int mg3d_es_default_params(mg3d_es_params *p); /* the reference's #defines */
/* host: the coarsest operator with zero-gradient rows on the walls (A zeroed by the caller, (N^3)^2 doubles) */
void mg3d_es_coarse_matrix(double *A, int N, double h, const mg3d_es_params *p);
int mg3d_es_setup(mg3d_ctx *ctx, const mg3d_es_params *p); /* zero fields, patches on the finest u, coarse LU */
int mg3d_es_smooth(mg3d_ctx *ctx, int level, int post, int iters); /* red-black passes + ghost copies */
int mg3d_es_vcycles(mg3d_ctx *ctx, int count, double *norms);

/* ------------------------------------------------------------ several GPUs (i-slabs)
 * The reference splits every operator over the slowest index i between OpenMP threads (mg_3d.h:658-659);
 * here rank r of nranks (one process per GPU) owns a contiguous range of i-planes of every level large
 * enough, exchanges halo planes with its two neighbours by RCCL send/recv, and the small levels plus the
 * direct solve are replicated after one all-gather of the restricted right-hand side.  See
 * csrc/mg3d_dist.hip.  unique_id: 128 bytes from mg3d_comm_unique_id() on rank 0, distributed by the
 * launcher; NULL selects the loopback transport (all ranks virtual, in this process, on `device`).
 * mg3d_dist_upload/download take the FULL N^3 host array; a rank reads its slab / writes its owned planes. */
typedef struct mg3d_dist mg3d_dist;
int mg3d_comm_unique_id(void *out128);
int mg3d_dist_create(int coarse_pts, int num_levels, int smooth_iters, double grid_length, int rank, int nranks,
                     const void *unique_id, int device, mg3d_dist **out);
int mg3d_dist_destroy(mg3d_dist *d);
/* ranks in the RCCL communicator (ncclCommCount; 0 without one), whether the exchanges run on the communication stream
 * (one communicator; the u halos then travel underneath the launches in between: the default, MG3D_NO_OVERLAP=1 at
 * creation keeps everything on the compute stream), the HIP device in use */
int mg3d_dist_comm_info(const mg3d_dist *d, int *rccl_ranks, int *overlap, int *device);
int mg3d_dist_first_level(const mg3d_dist *d); /* lowest distributed level */
int mg3d_dist_halo(const mg3d_dist *d);        /* halo planes per side */
int mg3d_dist_carried_cycles(const mg3d_dist *d); /* cycles since creation that ended ahead into the next one ("carried cycles") */
int mg3d_dist_legs_cycles(const mg3d_dist *d);    /* cycles since creation whose up-leg on the finest level ran as ONE launch (options legs, legs_min;
                                                   * plan policy bits 4 / 8 of mg3d_dist_plan): their norm is completed by the next cycle's down-leg */
int mg3d_dist_build_coarse(mg3d_dist *d, double h_coarse);
/* as mg3d_ctx_set_shift, for every local rank's levels and the replicated coarse levels.  Every rank of a multi-rank job
 * must pass the same sigma (not checked). */
int mg3d_dist_set_shift(mg3d_dist *d, double sigma);
/* Variable coefficient on slabs: the semantics of mg3d_ctx_set_coefficient (eps of level l is the injection of the
 * caller's array, the coarse matrix comes from level 0's, sigma from mg3d_dist_set_shift, the two in either order).  Every
 * rank passes the FULL finest-level N^3 array and takes its window of every level, halos included.  An entry that is not
 * finite and > 0 is MG3D_ERR_ARG and changes nothing.  With an RCCL communicator (a multi-rank job, or MG3D_FORCE_COMM=1)
 * the call runs one all-reduce on it before anything changes: if any rank's array is invalid every rank returns
 * MG3D_ERR_ARG, if the ranks disagree on whether a coefficient is set every rank returns MG3D_ERR_STATE.  The values of eps
 * are not compared between ranks, nor is sigma: every rank must pass the same ones.  With a coefficient the cycle walks the
 * plain exchange plan (policy 0 or 1): no carried cycles, no one-launch legs.  MG3D_ERR_STATE inside a carried cycle.
 * NULL: the constant operator and its schedules again, as on a fresh handle. */
int mg3d_dist_set_coefficient(mg3d_dist *d, const double *eps_full); /* finest level, dense N^3 host array; NULL: constant operator again */
int mg3d_dist_has_coefficient(const mg3d_dist *d, int *on);
int mg3d_dist_get_coefficient(mg3d_dist *d, int level, double *host_full); /* injected eps of a level; writes the planes each local rank owns, as mg3d_dist_download; MG3D_ERR_STATE without one */
int mg3d_dist_set_keep_residual(mg3d_dist *d, int keep); /* as mg3d_ctx_set_keep_residual */
int mg3d_dist_set_option(mg3d_dist *d, const char *key, int value); /* as mg3d_ctx_set_option, for every local rank */
int mg3d_dist_upload(mg3d_dist *d, int field, int level, const double *host_full);
int mg3d_dist_download(mg3d_dist *d, int field, int level, double *host_full);
int mg3d_dist_vcycles(mg3d_dist *d, int count, double *norms);
int mg3d_dist_sync(mg3d_dist *d);
/* the partition itself (pure host arithmetic, usable without a GPU) */
int mg3d_slab_halo(int smooth_iters);
int mg3d_slab_first_level(int coarse_pts, int num_levels, int nranks, int halo);
int mg3d_slab_owned(int coarse_pts, int num_levels, int nranks, int halo, int level, int rank, int *lo, int *hi);

/* The exchange plan of ONE V-cycle for one rank (pure host arithmetic, usable without a GPU): every transfer the rank
 * takes part in, in issue order.  The library's own transports (RCCL and loopback) execute exactly this list -- they hold
 * no plane arithmetic of their own -- so a property checked on the plans of all ranks (every send has its receive with the
 * same count, offsets inside the slab and on the same global planes, every rank walks the same phases) is a property of
 * what runs on the GPUs.  What each phase stands for in the reference: the implicit barrier at the end of an orphaned
 * `omp for` (mg_3d.h:658-702, 807-842, 961-995, 1007-1145), after which every thread sees its neighbours' planes.
 * A phase = one ncclGroupStart/End (all ranks issue the same phases in the same order); offsets and counts are in planes
 * of `plane_elems` elements: LOCAL plane indices of the rank's slab for distributed levels, global ones for the
 * replicated level's arrays.  stream: 0 compute stream (overlap off); overlap on: every exchange is issued on the
 * communication stream, the only stream that drives the one communicator -- 1 the compute stream joins at once, 2 it joins
 * when it next needs the field (the transfer runs underneath the launches in between).  policy bit 0: the coarse levels are solved on rank 0 only (right-hand side gathered,
 * correction broadcast: MG3D_COARSE_GATHER=1) instead of replicated on every rank behind one all-gather.  Bit 1 (2): a V(2,2) cycle that
 * ends ahead into the next one ("carried cycles": HALO_U_NEXT brings three planes).  Bit 2 (4): a V(2,2) cycle whose up-leg on the
 * finest level is ONE launch (HALO_U_NEXT brings planes 1..5, no NORM phase at the end: the next cycle's one-launch down-leg
 * completes the norm); bit 3 (8): the cycle behind such a one (a NORM phase first, behind its down-leg).  8 alone: the last of a run. */
enum { MG3D_XK_HALO_U_DOWN = 0, /* u_l after pre-smoothing + restriction, for the prolongation on the way up */
       MG3D_XK_HALO_D,          /* d_(l-1) after restriction */
       MG3D_XK_RHS_ALLGATHER,   /* d of the first replicated level: one broadcast per owner */
       MG3D_XK_RHS_GATHER,      /* policy bit 0: the same planes to rank 0 only */
       MG3D_XK_CORR_BCAST,      /* policy bit 0: u of the first replicated level from rank 0 */
       MG3D_XK_HALO_U_UP,       /* u_(l-1), the coarse correction, before the prolongation into level l */
       MG3D_XK_HALO_U_NEXT,     /* finest u after post-smoothing, halo planes 2..H, for the next cycle */
       MG3D_XK_NORM,            /* per-rank sums of squares, all-gathered */
       MG3D_XK_COUNT };
enum { MG3D_XOP_SEND = 0, MG3D_XOP_RECV, MG3D_XOP_BCAST, MG3D_XOP_ALLGATHER };
typedef struct mg3d_xfer {
    int phase;       /* 0, 1, ... in issue order within the cycle */
    int kind;        /* MG3D_XK_* */
    int op;          /* MG3D_XOP_* */
    int peer;        /* send/recv: the other rank; broadcast: the root; all-gather: -1 */
    int field, level;
    int offset;      /* first plane (send: source, recv: destination, broadcast: both) */
    int count;       /* planes */
    long long plane_elems;
    int stream;
} mg3d_xfer;
/* returns the number of entries (out may be NULL to ask for it), or a negative MG3D_ERR_* */
int mg3d_dist_plan(int coarse_pts, int num_levels, int nranks, int smooth_iters, int rank, int overlap, int policy,
                   mg3d_xfer *out, int max_entries);
/* per-phase cost of the slab path, from event pairs on the streams the phases run on (on = 1; off by default):
 * ms[0] whole cycles, ms[1] exchanges the compute stream waits for at once, ms[2] exchanges that run overlapped,
 * ms[3] the replicated (or rank-0) coarse levels incl. the direct solve; kernels on the distributed levels =
 * ms[0] - ms[1] - ms[3].  Sums since the last enable; *cycles = cycles covered. */
int mg3d_dist_timing_enable(mg3d_dist *d, int on);
int mg3d_dist_timing_get(mg3d_dist *d, double ms[4], int *cycles);

/* ------------------------------------- host-pointer forms (reference signatures)
 * Same argument meaning as the reference functions; data is staged to the
 * device, computed there, and copied back.  They exist so that drivers that
 * call the operators directly (test_mg_3d_dirichlet.c:51,60) link unchanged. */
int mg3d_host_smooth(double *v, const double *d, int N, double h, int iters, int post);
int mg3d_host_residual(const double *v, const double *d, int N, double h, double *res, double *norm);
int mg3d_host_restrict(const double *r, int Nf, double *dc, int Nc);
int mg3d_host_prolong(const double *ec, int Nc, double *ef, int Nf);
int mg3d_host_lu_solve(const double *LU, int n, const double *b, double *x);
/* vcycle(u,f,res,h,q,numLevels,smootherIter,N,LU), mg_3d.h:1242: caller-owned
 * host hierarchies (allocGridLevels).  Levels 0..q are copied back after the cycle.
 * stage_calls / stage_seconds (optional, (q+1)*MG3D_NUM_STAGES entries, [level][stage])
 * are incremented by this cycle's per-stage event timings (tInfo of mg_3d.h:1279-1359). */
int mg3d_host_vcycle(double **u, double **f, double **res, double h, int q, int num_levels, int iters, int N,
                     const double *LU, double *norm, int *stage_calls, double *stage_seconds);

/* --------------------------------------------------- host-only helpers (no device)
 * mg3d_bc_func            : BCFunc (mg_3d.h:89-90)
 * mg3d_fill_boundary_host : setupBoundaryConditions (mg_3d.h:1147-1239)
 * mg3d_coarse_matrix*     : constructCoarseMatrixA (mg_3d.h:147-273), A zeroed by caller.  ONE builder writes every form;
 *                           each entry point is that builder with the arguments it does not name at their neutral
 *                           values (sigma = 0, eps NULL, no periodic axis, no Neumann face, mask NULL), so any two agree
 *                           byte for byte where their arguments do:
 *   mg3d_coarse_matrix         : the reference's Dirichlet matrix
 *   mg3d_coarse_matrix_shift   : + the screened operator (diagonal -(6 + sigma*h^2)/h^2)
 *   mg3d_coarse_matrix_coef    : + the variable-coefficient operator (mg3d_ctx_set_coefficient; eps dense N^3)
 *   mg3d_coarse_matrix_periodic: + periodic axes (mg3d_ctx_set_periodic; eps NULL for the constant operator)
 *   mg3d_coarse_matrix_bc      : + Neumann faces (mg3d_ctx_set_neumann): reflected rows for the Neumann face unknowns
 *   mg3d_coarse_matrix_mask    : + fixed points (mg3d_ctx_set_mask; mask dense N^3 bytes): identity rows at the fixed
 *                                unknowns, and the pin only without one
 *   mg3d_coarse_matrix_field   : + the screening field (mg3d_ctx_set_shift_field; s dense N^3, >= 0, NULL for none): the
 *                                diagonal -((D + (sigma + s[p])*h^2)/h^2), D the sum of the six face means or exactly 6.0,
 *                                and the pin only where s is > 0 at no unknown -- the form mg3d_ctx_build_coarse calls
 * mg3d_neumann_fold_flux  : a prescribed outward normal derivative g folded into the right-hand side d (dense N^3) of the
 *                           homogeneous Neumann operator: d -= 2*a*g/h at each point of each Neumann face in `faces`, a = 1
 *                           (eps NULL) or 0.5*(eps_face + eps_inner), summed over the faces an edge or corner point lies
 *                           on.  g[f] (f = 0..5: ilo, ihi, jlo, jhi, klo, khi) is a dense N^2 array over the face's other
 *                           two indices in i, j, k order, NULL = 0; g itself may be NULL.  Returns MG3D_OK or MG3D_ERR_ARG.
 * mg3d_lu_factor          : convertToLU_InPlace (gauss_elim.h:9-29)
 * mg3d_lu_solve_host      : NOT provided -- the solve runs on the device only
 * mg3d_l2norm_host        : GetL2NormOfVector (mg_3d.h:783-792)
 * mg3d_smooth_edges_host  : updateEdgeValues (mg_3d.h:304-430; cosmetic, never read by the stencil)
 * mg3d_write_vtk          : writeOutputData (postprocess.h:5-47) */
double mg3d_bc_func(double x, double y, double z);
void mg3d_fill_boundary_host(double *v, int N, double h);
void mg3d_coarse_matrix(double *A, int N, double h);
void mg3d_coarse_matrix_shift(double *A, int N, double h, double sigma);
void mg3d_coarse_matrix_coef(double *A, int N, double h, const double *eps, double sigma); /* host only, A zeroed by caller */
void mg3d_coarse_matrix_periodic(double *A, int N, double h, const double *eps /* NULL: constant */, double sigma,
                                 int axes); /* host only, A zeroed by caller; axes = 0: _shift / _coef */
void mg3d_coarse_matrix_bc(double *A, int N, double h, const double *eps /* NULL: constant */, double sigma,
                           int periodic_axes, int neumann_faces); /* host only, A zeroed by caller */
void mg3d_coarse_matrix_mask(double *A, int N, double h, const double *eps /* NULL: constant */, double sigma,
                             int periodic_axes, int neumann_faces, const unsigned char *mask /* NULL: none */);
void mg3d_coarse_matrix_field(double *A, int N, double h, const double *eps /* NULL: constant */, double sigma,
                              int periodic_axes, int neumann_faces, const unsigned char *mask /* NULL: none */,
                              const double *s /* NULL: none */);
int mg3d_neumann_fold_flux(double *d, const double *eps /* NULL: constant */, int N, double h, int faces,
                           const double *const *g);
void mg3d_lu_factor(double *a, int n);
double mg3d_l2norm_host(const double *d, long n);
void mg3d_smooth_edges_host(double *u, int N);
int mg3d_write_vtk(const char *file_name, const double *grid, double h, int N);
/* zero-filled page-locked host memory (hipHostMalloc): arrays the facade moves across PCIe on every solve */
int mg3d_host_alloc(size_t bytes, void **out);
int mg3d_host_free(void *p);

/* ---- single precision / damped Jacobi / F-cycle variant (BASELINE configs[4]) --------------------------
 * PARITY UNPINNED: the reference has no fp32 arithmetic and no Jacobi smoother; its FMG start exists only as
 * mg_dirichlet_analytic.c:771-806 (commented copy mg_3d.h:1364-1404).  Semantics are defined by
 * csrc/mg3d_f32.hip and restated in plain C by the test infrastructure: binary32 storage and grid arithmetic with the
 * reference's association per operator, v' = v + omega*((1/6)(sum6 - h^2 d) - v) out of place, the reference's
 * double LU factors on the coarsest level (rhs widened, solution rounded), norms accumulated in double.
 * Fields and levels are numbered as above (MG3D_U/D/R, 0 = coarsest); host arrays are N^3 floats, k fastest. */
typedef struct mg3d32_ctx mg3d32_ctx;
int mg3d32_create(int coarse_pts, int num_levels, int smooth_iters, double omega, double grid_length,
                  mg3d32_ctx **out);
int mg3d32_destroy(mg3d32_ctx *ctx);
int mg3d32_set_option(mg3d32_ctx *ctx, const char *key, int value); /* "pairs", "fuse", "carry": see mg3d_ctx_set_option */
int mg3d32_level_n(const mg3d32_ctx *ctx, int level);
int mg3d32_upload(mg3d32_ctx *ctx, int field, int level, const float *host);
int mg3d32_download(mg3d32_ctx *ctx, int field, int level, float *host);
int mg3d32_zero(mg3d32_ctx *ctx, int field, int level);
int mg3d32_sync(mg3d32_ctx *ctx);
int mg3d32_fill_boundary(mg3d32_ctx *ctx, int field, int level);   /* BCFunc (mg_3d.h:89) on the six faces */
int mg3d32_smooth(mg3d32_ctx *ctx, int level, int iters);          /* `iters` damped-Jacobi sweeps */
int mg3d32_residual(mg3d32_ctx *ctx, int level, int store, double *norm); /* mg_3d.h:794-842 in binary32 */
int mg3d32_restrict(mg3d32_ctx *ctx, int level);                   /* r(level) -> d(level-1), mg_3d.h:844-998 */
int mg3d32_prolong(mg3d32_ctx *ctx, int level);                    /* u(level) += P u(level-1), mg_3d.h:1000-1145 */
int mg3d32_coarse_solve(mg3d32_ctx *ctx);                          /* gauss_elim.h:31-60 through double */
int mg3d32_vcycles(mg3d32_ctx *ctx, int count, double *norms);     /* mg_3d.h:1242-1362 with the Jacobi smoother */
/* F-cycle start, mg_dirichlet_analytic.c:771-806.  Unlike the reference's vcycle (which zeroes u[q] on entry below the
 * finest level, :698-700, and thereby discards the interpolated guess everywhere but on the finest level -- behaviour the
 * fp64 mg3d_fmg_initialize reproduces), this variant zeroes only the coarser level before descending: the interpolated
 * guess is kept on every level. */
int mg3d32_fmg_initialize(mg3d32_ctx *ctx);
/* kernel timers of the finest level's launches (event pairs in-stream, resolved by mg3d32_vcycles' own synchronisation):
 * mg3d32_kernel_name(k) is NULL past the last kernel */
int mg3d32_timing_enable(mg3d32_ctx *ctx, int on);
const char *mg3d32_kernel_name(int kernel);
int mg3d32_kernel_time_get(mg3d32_ctx *ctx, int kernel, int *num_launches, double *seconds);

/* The same variant on i-slabs of several GPUs (csrc/mg3d_f32_dist.hip; BASELINE configs[4]: 1025^3 on 8 GPUs): the
 * partition and schedule of mg3d_dist_* with H = smooth_iters + 2 halo planes (a Jacobi sweep uses up one plane per
 * sweep).  unique_id as for mg3d_dist_create; NULL = loopback (all ranks virtual in this process).  upload/download
 * take the FULL N^3 float array. */
typedef struct mg3d32_dist mg3d32_dist;
int mg3d32_slab_halo(int smooth_iters);
/* the exchange plan of this variant's V-cycle from distributed level q (the F-cycle start runs one from every level;
 * want_norm = 0 leaves the norm phase out), same entry format and the same executor as mg3d_dist_plan; element = float */
int mg3d32_dist_plan(int coarse_pts, int num_levels, int nranks, int smooth_iters, int rank, int q, int want_norm,
                     mg3d_xfer *out, int max_entries);
int mg3d32_dist_create(int coarse_pts, int num_levels, int smooth_iters, double omega, double grid_length, int rank,
                       int nranks, const void *unique_id, int device, mg3d32_dist **out);
int mg3d32_dist_destroy(mg3d32_dist *d);
int mg3d32_dist_first_level(const mg3d32_dist *d);
int mg3d32_dist_halo(const mg3d32_dist *d);
int mg3d32_dist_comm_info(const mg3d32_dist *d, int *rccl_ranks, int *device);
int mg3d32_dist_upload(mg3d32_dist *d, int field, int level, const float *host_full);
int mg3d32_dist_download(mg3d32_dist *d, int field, int level, float *host_full);
int mg3d32_dist_zero(mg3d32_dist *d, int field, int level);
int mg3d32_dist_fill_boundary(mg3d32_dist *d, int field, int level);
int mg3d32_dist_vcycles(mg3d32_dist *d, int count, double *norms);
int mg3d32_dist_fmg_initialize(mg3d32_dist *d); /* needs d of every level (boundary values), u zero */
int mg3d32_dist_sync(mg3d32_dist *d);

#ifdef __cplusplus
}
#endif
#endif /* MG3D_H */
