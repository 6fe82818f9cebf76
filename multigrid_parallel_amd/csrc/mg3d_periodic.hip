/*
 * mg3d_periodic.hip -- gfx950 kernels of periodic boundaries (mg3d_ctx_set_periodic).
 *
 * axes is a bit mask (MG3D_PERIODIC_I = 1, _J = 2, _K = 4).  A level keeps its N points per side; on a periodic axis index
 * N-1 is the DUPLICATE of index 0 and the unique points are 0 .. N-2 (an even count, so red-black colours agree across
 * the wrap).  On a non-periodic axis the faces 0 and N-1 stay Dirichlet points that no kernel here writes.
 *
 *   - Nothing reads a duplicate: a stencil reaches across the wrap to the unique point (i-1 at i = 0 is N-2, i+1 at N-2
 *     is 0), and every kernel that writes a unique point on a periodic face also writes its duplicates (edges and
 *     corners included), so written fields are always periodic-consistent.
 *   - Colour pass and residual keep the arithmetic of the other kernels exactly; only neighbour indices change:
 *       constant operator (LevelOp, mg3d_kernels.hip):
 *         s = (((((v_im + v_ip) + v_jm) + v_jp) + v_km) + v_kp);  v = sixth*(s - hSq*d);  diff = d - invHsq*(s - dg*v)
 *       eps set (mg3d_coef.hip): face means, s and dg as coef_stencil; v = (s - hSq*d)/dg;  diff = d - invHsq*(s - dg*v)
 *   - Restriction: the 27-point full weighting of restrict_kernel (same order) on every coarse point that lies on no
 *     Dirichlet face, with wrapped fine neighbours on periodic axes; Dirichlet faces are injected as before.
 *   - Prolongation: the parent order of prolong_kernel, the coarse "high" parent wrapped to 0 on a periodic axis.
 * tests/_periodic_ref.py states the same in numpy.
 *
 * Layout as mg3d_kernels.hip (single-domain levels only: ig0 = 0, ni = nj = nk = N).  The residual and the colour pass
 * with eps give each thread one (j, k) column of `chunk` planes, lanes contiguous in k, and keep the i-1 / i / i+1 values
 * of v (and eps) in registers; the j and k neighbour offsets are per-column constants, so the only per-point additions
 * over k_coef_* / k_residual are the i wrap (a select on the plane of i+1) and one predicate for the duplicate stores.
 * The constant colour pass keeps the one-point-per-thread shape of k_smooth_color.
 */
#include "mg3d_internal.h"

#define WAVE 64

__device__ __forceinline__ long long pidx(const Geom &g, int i, int j, int k)
{
    return g.plane * i + (long long)g.pitch * j + k;
}

/* the offsets to the -1 / +1 neighbour along an axis of stride `st` at index x (unique range), wrapped when periodic */
__device__ __forceinline__ long long nb_lo(int x, int N, bool per, long long st) { return (per && x == 0) ? (N - 2) * st : -st; }
__device__ __forceinline__ long long nb_hi(int x, int N, bool per, long long st) { return (per && x == N - 2) ? -(N - 2) * st : st; }

/* x to p and to every duplicate of p: di / dj / dk say whether p lies on the periodic face 0 of that axis */
__device__ __forceinline__ void store_dup(const Geom &g, double *__restrict__ a, long long p, double x, bool di, bool dj,
                                          bool dk)
{
    a[p] = x;
    if (!(di | dj | dk))
        return;
    const long long si = (long long)(g.N - 1) * g.plane, sj = (long long)(g.N - 1) * g.pitch, sk = g.N - 1;
    for (int m = 1; m < 8; m++) {
        if (((m & 1) && !di) || ((m & 2) && !dj) || ((m & 4) && !dk))
            continue;
        a[p + ((m & 1) ? si : 0) + ((m & 2) ? sj : 0) + ((m & 4) ? sk : 0)] = x;
    }
}

/* neighbour sum and diagonal of point p; vb / va and eb / eh / ea: v and eps of planes i-1, i, i+1 of the column,
 * oj* / ok*: the column's (possibly wrapped) j and k offsets */
template <bool COEF>
__device__ __forceinline__ void per_stencil(const double *__restrict__ v, const double *__restrict__ e, long long p,
                                            long long ojm, long long ojp, long long okm, long long okp, double vb,
                                            double va, double eb, double eh, double ea, double dg0, double &s, double &dg)
{
    if constexpr (COEF) {
        const double a_im = 0.5 * (eh + eb);
        const double a_ip = 0.5 * (eh + ea);
        const double a_jm = 0.5 * (eh + e[p + ojm]);
        const double a_jp = 0.5 * (eh + e[p + ojp]);
        const double a_km = 0.5 * (eh + e[p + okm]);
        const double a_kp = 0.5 * (eh + e[p + okp]);
        double t = a_im * vb + a_ip * va;
        t = t + a_jm * v[p + ojm];
        t = t + a_jp * v[p + ojp];
        t = t + a_km * v[p + okm];
        t = t + a_kp * v[p + okp];
        s = t;
        double D = a_im + a_ip;
        D = D + a_jm;
        D = D + a_jp;
        D = D + a_km;
        D = D + a_kp;
        dg = D + dg0; /* dg0 = sigma*hSq */
    } else {
        double t = vb + va;
        t = t + v[p + ojm];
        t = t + v[p + ojp];
        t = t + v[p + okm];
        t = t + v[p + okp];
        s = t;
        dg = dg0; /* dg0 = 6 + sigma*hSq */
    }
}

/* the geometry of one thread's column: unique ranges start at 0 on a periodic axis, at 1 otherwise */
struct PerColumn {
    int j, k, i0, i1;
    bool pi, dj, dk;
    long long ojm, ojp, okm, okp;
};

__device__ __forceinline__ bool per_column(const Geom &g, int axes, int chunk, PerColumn &c)
{
    const int N = g.N;
    c.pi = axes & 1;
    const bool pj = axes & 2, pk = axes & 4;
    c.k = (pk ? 0 : 1) + blockIdx.x * WAVE + threadIdx.x;
    c.j = (pj ? 0 : 1) + blockIdx.y * 4 + threadIdx.y;
    c.i0 = (c.pi ? 0 : 1) + blockIdx.z * chunk;
    c.i1 = min(c.i0 + chunk, N - 1);
    if (c.k > N - 2 || c.j > N - 2)
        return false;
    c.dj = pj && c.j == 0;
    c.dk = pk && c.k == 0;
    c.ojm = nb_lo(c.j, N, pj, g.pitch);
    c.ojp = nb_hi(c.j, N, pj, g.pitch);
    c.okm = nb_lo(c.k, N, pk, 1);
    c.okp = nb_hi(c.k, N, pk, 1);
    return true;
}

/* ------------------------------------------------------------------ smoother
 * One red-black colour pass in place over the unique points.  Everything a point reads has the other colour (the wrap
 * joins 0 and N-2, of opposite parity), and a duplicate has its source's colour: it is written in the same pass and read
 * by none.
 * Constant operator: smooth_color_kernel's shape (a lane owns the k-pair (2m, 2m+1) of one row and updates the member
 * of the colour swept), with the six neighbour offsets wrapped per thread.  Measured at 513^3 the column form below took
 * 0.76 ms against 0.64 ms of k_smooth_color for this operator; this shape keeps its launch. */
__global__ void __launch_bounds__(256) per_color_kernel(Geom g, double *__restrict__ v, const double *__restrict__ d,
                                                        double hSq, double sixth, int color, int axes)
{
    const int N = g.N;
    const bool pi = axes & 1, pj = axes & 2, pk = axes & 4;
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = (pj ? 0 : 1) + blockIdx.y * blockDim.y + threadIdx.y;
    const int i = (pi ? 0 : 1) + blockIdx.z;
    if (j > N - 2)
        return;
    const int k = 2 * m + ((color + i + j) & 1);
    if (k < (pk ? 0 : 1) || k > N - 2)
        return;
    const long long p = pidx(g, i, j, k);
    double s = v[p + nb_lo(i, N, pi, g.plane)] + v[p + nb_hi(i, N, pi, g.plane)];
    s = s + v[p + nb_lo(j, N, pj, g.pitch)];
    s = s + v[p + nb_hi(j, N, pj, g.pitch)];
    s = s + v[p + nb_lo(k, N, pk, 1)];
    s = s + v[p + nb_hi(k, N, pk, 1)];
    s = s - hSq * d[p];
    store_dup(g, v, p, sixth * s, pi && i == 0, pj && j == 0, pk && k == 0);
}

/* eps set: the column form of coef_color_kernel -- a thread owns one (j, k) column of `chunk` planes and keeps v and eps
 * of planes i-1, i, i+1 in registers */
__global__ void __launch_bounds__(256) per_coef_color_kernel(Geom g, double *__restrict__ v, const double *__restrict__ e,
                                                             const double *__restrict__ d, double hSq, double shift,
                                                             int color, int axes, int chunk)
{
    PerColumn c;
    if (!per_column(g, axes, chunk, c))
        return;
    const int N = g.N;
    long long p = pidx(g, c.i0, c.j, c.k);
    const long long pb = p + nb_lo(c.i0, N, c.pi, g.plane);
    double vb = v[pb], vh = v[p];
    double eb = e[pb], eh = e[p];
    for (int i = c.i0; i < c.i1; i++, p += g.plane) {
        const long long pa = p + nb_hi(i, N, c.pi, g.plane);
        const double va = v[pa], ea = e[pa];
        if (((i + c.j + c.k) & 1) == color) {
            double s, dg;
            per_stencil<true>(v, e, p, c.ojm, c.ojp, c.okm, c.okp, vb, va, eb, eh, ea, shift, s, dg);
            store_dup(g, v, p, (s - hSq * d[p]) / dg, c.pi && i == 0, c.dj, c.dk);
        }
        /* (a point updated here is the i-1 neighbour of a plane this pass does not update: its old value is never used) */
        vb = vh;
        vh = va;
        eb = eh;
        eh = ea;
    }
}

/* chunk of planes per thread: 16 as residual_kernel, doubled until the partial sums fit */
static int per_chunk(int planes, int gx, int gy)
{
    int chunk = 16;
    while ((long long)gx * gy * ((planes + chunk - 1) / chunk) > MG3D_MAX_PARTIALS)
        chunk *= 2;
    return chunk;
}

/* unique points per side that the stencil kernels visit on an axis */
static inline int per_span(int N, int axes, int bit) { return (axes & bit) ? N - 1 : N - 2; }
/* k-pairs per row of the constant colour pass (as k_smooth_color) */
static inline int N_pairs(int N) { return (N + 1) / 2; }

void k_per_color(const Geom &g, double *v, const double *e, const double *d, const LevelOp &op, double shift, int color,
                 int axes, hipStream_t s)
{
    const int ni = per_span(g.N, axes, 1), nj = per_span(g.N, axes, 2), nk = per_span(g.N, axes, 4);
    if (ni < 1 || nj < 1 || nk < 1)
        return;
    if (!e) {
        const dim3 grid(((N_pairs(g.N)) + WAVE - 1) / WAVE, (nj + 3) / 4, ni);
        hipLaunchKernelGGL(per_color_kernel, grid, dim3(WAVE, 4, 1), 0, s, g, v, d, op.hSq, op.sixth, color, axes);
        return;
    }
    const int gx = (nk + WAVE - 1) / WAVE, gy = (nj + 3) / 4;
    const int chunk = per_chunk(ni, gx, gy);
    hipLaunchKernelGGL(per_coef_color_kernel, dim3(gx, gy, (ni + chunk - 1) / chunk), dim3(WAVE, 4, 1), 0, s, g, v, e, d,
                       op.hSq, shift, color, axes, chunk);
}

/* ------------------------------------------------------------------ residual
 * diff at every unique point; res (optional) receives it there and at the duplicates; partials one sum of diff^2 per
 * block (lanes by shuffle tree, waves 0..3 in order), folded by k_fold: the norm counts every unknown once. */
__device__ __forceinline__ double per_block_sum(double x, double *lds4)
{
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1)
        x += __shfl_down(x, off, WAVE);
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    if ((tid & (WAVE - 1)) == 0)
        lds4[tid / WAVE] = x;
    __syncthreads();
    return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}

template <bool COEF>
__global__ void __launch_bounds__(256) per_residual_kernel(Geom g, const double *__restrict__ v,
                                                           const double *__restrict__ e, const double *__restrict__ d,
                                                           double invHsq, double dg0, double *__restrict__ res,
                                                           double *__restrict__ partials, int axes, int chunk)
{
    __shared__ double lds4[4];
    double acc = 0.;
    PerColumn c;
    if (per_column(g, axes, chunk, c)) {
        const int N = g.N;
        long long p = pidx(g, c.i0, c.j, c.k);
        const long long pb = p + nb_lo(c.i0, N, c.pi, g.plane);
        double vb = v[pb], vh = v[p];
        double eb = 0., eh = 0.;
        if constexpr (COEF) {
            eb = e[pb];
            eh = e[p];
        }
        for (int i = c.i0; i < c.i1; i++, p += g.plane) {
            const long long pa = p + nb_hi(i, N, c.pi, g.plane);
            const double va = v[pa];
            double ea = 0.;
            if constexpr (COEF)
                ea = e[pa];
            double s, dg;
            per_stencil<COEF>(v, e, p, c.ojm, c.ojp, c.okm, c.okp, vb, va, eb, eh, ea, dg0, s, dg);
            const double diff = d[p] - invHsq * (s - dg * vh);
            if (res)
                store_dup(g, res, p, diff, c.pi && i == 0, c.dj, c.dk);
            acc += diff * diff;
            vb = vh;
            vh = va;
            if constexpr (COEF) {
                eb = eh;
                eh = ea;
            }
        }
    }
    const double tot = per_block_sum(acc, lds4);
    if (threadIdx.x == 0 && threadIdx.y == 0)
        partials[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tot;
}

void k_per_residual(const Geom &g, const double *v, const double *e, const double *d, const LevelOp &op, double shift,
                    int axes, double *res, double *partials, double *sumsq_out, hipStream_t s)
{
    const int ni = per_span(g.N, axes, 1), nj = per_span(g.N, axes, 2), nk = per_span(g.N, axes, 4);
    if (ni < 1 || nj < 1 || nk < 1) {
        (void)hipMemsetAsync(sumsq_out, 0, sizeof(double), s);
        return;
    }
    const int gx = (nk + WAVE - 1) / WAVE, gy = (nj + 3) / 4;
    const int chunk = per_chunk(ni, gx, gy);
    const int gz = (ni + chunk - 1) / chunk;
    const dim3 grid(gx, gy, gz), block(WAVE, 4, 1);
    if (e)
        hipLaunchKernelGGL(per_residual_kernel<true>, grid, block, 0, s, g, v, e, d, op.invHsq, shift, res, partials, axes,
                           chunk);
    else
        hipLaunchKernelGGL(per_residual_kernel<false>, grid, block, 0, s, g, v, e, d, op.invHsq, op.dg, res, partials, axes,
                           chunk);
    k_fold(partials, gx * gy * gz, sumsq_out, s);
}

/* --------------------------------------------------------------- restriction
 * One thread per coarse point.  A point on a Dirichlet face (index 0 or Nc-1 of a non-periodic axis) is injected,
 * dc = r(2I, 2J, 2K), as restrict_kernel does; every other unique point -- periodic face points included -- takes the
 * full weighting val = 0; val += r(2I-1+ti, ...) * w in restrict_kernel's order, with fine index -1 wrapped to Nf-2
 * (2I+1 <= Nf-2 never wraps).  Duplicates are written as copies by the thread of their source. */
__global__ void __launch_bounds__(256) per_restrict_kernel(Geom gf, const double *__restrict__ r, Geom gc,
                                                           double *__restrict__ dc, int axes)
{
    const int kc = blockIdx.x * WAVE + threadIdx.x;
    const int jc = blockIdx.y * 4 + threadIdx.y;
    const int ic = blockIdx.z;
    const int Nc = gc.N, Nf = gf.N;
    const bool pi = axes & 1, pj = axes & 2, pk = axes & 4;
    if (kc >= Nc || jc >= Nc || ic >= Nc)
        return;
    if ((pi && ic == Nc - 1) || (pj && jc == Nc - 1) || (pk && kc == Nc - 1))
        return; /* a duplicate: its source's thread writes it */
    const long long pf = pidx(gf, 2 * ic, 2 * jc, 2 * kc);
    const bool face = (!pi && (ic == 0 || ic == Nc - 1)) || (!pj && (jc == 0 || jc == Nc - 1)) ||
                      (!pk && (kc == 0 || kc == Nc - 1));
    double val;
    if (face) {
        val = r[pf];
    } else {
        const long long oi[3] = {ic == 0 ? (Nf - 2) * gf.plane : -gf.plane, 0, gf.plane};
        const long long oj[3] = {jc == 0 ? (long long)(Nf - 2) * gf.pitch : -(long long)gf.pitch, 0, gf.pitch};
        const long long ok[3] = {kc == 0 ? (long long)(Nf - 2) : -1, 0, 1};
        val = 0.;
#pragma unroll
        for (int ti = 0; ti < 3; ti++)
#pragma unroll
            for (int tj = 0; tj < 3; tj++)
#pragma unroll
                for (int tk = 0; tk < 3; tk++) {
                    const double w = (ti != 1 ? 0.25 : 0.5) * (tj != 1 ? 0.25 : 0.5) * (tk != 1 ? 0.25 : 0.5);
                    val += r[pf + oi[ti] + oj[tj] + ok[tk]] * w;
                }
    }
    store_dup(gc, dc, pidx(gc, ic, jc, kc), val, pi && ic == 0, pj && jc == 0, pk && kc == 0);
}

void k_per_restrict(const Geom &gf, const double *r, const Geom &gc, double *dc, int axes, hipStream_t s)
{
    dim3 grid((gc.N + WAVE - 1) / WAVE, (gc.N + 3) / 4, gc.N);
    hipLaunchKernelGGL(per_restrict_kernel, grid, dim3(WAVE, 4, 1), 0, s, gf, r, gc, dc, axes);
}

/* -------------------------------------------------------------- prolongation
 * ef += P(ec) at every fine point that is not a duplicate (Dirichlet faces included, as prolong_kernel), in
 * prolong_kernel's parent order; on a periodic axis the high parent il+1 = Nc-1 is read at its source 0.  The thread
 * of a point writes the sum to its duplicates too, so neither a fine nor a coarse duplicate is ever read. */
__global__ void __launch_bounds__(256) per_prolong_kernel(Geom gc, const double *__restrict__ ec, Geom gf,
                                                          double *__restrict__ ef, int axes)
{
    const int k = blockIdx.x * WAVE + threadIdx.x;
    const int j = blockIdx.y * 4 + threadIdx.y;
    const int i = blockIdx.z;
    const int Nc = gc.N, Nf = gf.N;
    const bool pi = axes & 1, pj = axes & 2, pk = axes & 4;
    if (k >= Nf || j >= Nf)
        return;
    if ((pi && i == Nf - 1) || (pj && j == Nf - 1) || (pk && k == Nf - 1))
        return;
    const int oi = i & 1, oj = j & 1, ok = k & 1;
    const int il = (i - oi) / 2, jl = (j - oj) / 2, kl = (k - ok) / 2;
    const long long c0 = pidx(gc, il, jl, kl);
    const long long sI = (pi && il + 1 == Nc - 1) ? -(long long)il * gc.plane : gc.plane;
    const long long sJ = (pj && jl + 1 == Nc - 1) ? -(long long)jl * gc.pitch : gc.pitch;
    const long long sK = (pk && kl + 1 == Nc - 1) ? -(long long)kl : 1;
    double t = 0.;
    switch (oi + oj + ok) {
    case 3:
        t += ec[c0];
        t += ec[c0 + sK];
        t += ec[c0 + sJ];
        t += ec[c0 + sJ + sK];
        t += ec[c0 + sI];
        t += ec[c0 + sI + sK];
        t += ec[c0 + sI + sJ];
        t += ec[c0 + sI + sJ + sK];
        t *= 0.125;
        break;
    case 2:
        if (!oi) {
            t += ec[c0];
            t += ec[c0 + sJ];
            t += ec[c0 + sK];
            t += ec[c0 + sJ + sK];
        } else if (!oj) {
            t += ec[c0];
            t += ec[c0 + sI];
            t += ec[c0 + sK];
            t += ec[c0 + sI + sK];
        } else {
            t += ec[c0];
            t += ec[c0 + sJ];
            t += ec[c0 + sI];
            t += ec[c0 + sI + sJ];
        }
        t *= 0.25;
        break;
    case 1:
        t += ec[c0];
        t += ec[c0 + (oi ? sI : 0) + (oj ? sJ : 0) + (ok ? sK : 0)];
        t *= 0.5;
        break;
    default:
        t = ec[c0];
    }
    const long long p = pidx(gf, i, j, k);
    store_dup(gf, ef, p, ef[p] + t, pi && i == 0, pj && j == 0, pk && k == 0);
}

void k_per_prolong(const Geom &gc, const double *ec, const Geom &gf, double *ef, int axes, hipStream_t s)
{
    dim3 grid((gf.N + WAVE - 1) / WAVE, (gf.N + 3) / 4, gf.N);
    hipLaunchKernelGGL(per_prolong_kernel, grid, dim3(WAVE, 4, 1), 0, s, gc, ec, gf, ef, axes);
}

/* ------------------------------------------------------------- coarsest level
 * The right-hand side of the direct solve (mg3d_coarse_matrix_periodic): d at every point, except 0 in the identity
 * rows of the duplicates and of the pinned point (0,0,0) -- so a duplicate's d is never read, and those rows' solution
 * is 0 until the refresh below copies the sources over the duplicates. */
__global__ void __launch_bounds__(256) per_coarse_rhs_kernel(Geom g, const double *__restrict__ d, double *__restrict__ b,
                                                             int axes, int pin)
{
    const int k = blockIdx.x * WAVE + threadIdx.x;
    const int j = blockIdx.y * 4 + threadIdx.y;
    const int i = blockIdx.z;
    const int N = g.N;
    if (k >= N || j >= N)
        return;
    const bool dup = ((axes & 1) && i == N - 1) || ((axes & 2) && j == N - 1) || ((axes & 4) && k == N - 1);
    const long long p = pidx(g, i, j, k);
    b[p] = (dup || (pin && (i | j | k) == 0)) ? 0. : d[p];
}

void k_per_coarse_rhs(const Geom &g, const double *d, double *b, int axes, int pin, hipStream_t s)
{
    dim3 grid((g.N + WAVE - 1) / WAVE, (g.N + 3) / 4, g.N);
    hipLaunchKernelGGL(per_coarse_rhs_kernel, grid, dim3(WAVE, 4, 1), 0, s, g, d, b, axes, pin);
}

/* Every duplicate of a field from its source: blockIdx.z = the axis whose duplicate plane a thread covers; (a, b) the
 * other two indices.  The source maps every periodic index N-1 to 0, so only unique points are read; an edge or corner
 * duplicate is written by each plane it lies in, with the same value. */
__global__ void __launch_bounds__(256) per_refresh_kernel(Geom g, double *__restrict__ v, int axes)
{
    const int b = blockIdx.x * WAVE + threadIdx.x, a = blockIdx.y * 4 + threadIdx.y, ax = blockIdx.z;
    const int N = g.N;
    if (a >= N || b >= N || !(axes & (1 << ax)))
        return;
    int i = ax == 0 ? N - 1 : a, j = ax == 1 ? N - 1 : (ax == 0 ? a : b), k = ax == 2 ? N - 1 : b;
    const int si = (axes & 1) && i == N - 1 ? 0 : i, sj = (axes & 2) && j == N - 1 ? 0 : j,
              sk = (axes & 4) && k == N - 1 ? 0 : k;
    v[pidx(g, i, j, k)] = v[pidx(g, si, sj, sk)];
}

void k_per_refresh(const Geom &g, double *v, int axes, hipStream_t s)
{
    if (!axes)
        return;
    dim3 grid((g.N + WAVE - 1) / WAVE, (g.N + 3) / 4, 3);
    hipLaunchKernelGGL(per_refresh_kernel, grid, dim3(WAVE, 4, 1), 0, s, g, v, axes);
}
