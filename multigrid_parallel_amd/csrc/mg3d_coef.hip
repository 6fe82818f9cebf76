/*
 * mg3d_coef.hip -- gfx950 kernels of the variable-coefficient operator (mg3d_ctx_set_coefficient):
 *
 *     div(eps grad u) - sigma u = d,   eps > 0 vertex-centred, one value per grid point of every level.
 *
 * Face coefficients are arithmetic means, neighbours in the reference's order (i-, i+, j-, j+, k-, k+), no contraction
 * (-ffp-contract=off):
 *   a_im = 0.5*(e[p] + e[p-NN]), a_ip = 0.5*(e[p] + e[p+NN]), ... a_kp = 0.5*(e[p] + e[p+1])
 *   s    = (((((a_im*v[p-NN] + a_ip*v[p+NN]) + a_jm*v[p-N]) + a_jp*v[p+N]) + a_km*v[p-1]) + a_kp*v[p+1])
 *   D    = ((((a_im + a_ip) + a_jm) + a_jp) + a_km) + a_kp;   dg = D + sigma*hSq
 *   smoother : v[p] = (s - hSq*d[p]) / dg          (IEEE division)
 *   residual : diff = d[p] - invHsq*(s - dg*v[p])
 * Coarse levels take eps by injection, e_{l-1}[I,J,K] = e_l[2I,2J,2K].  tests/_coef_ref.py states the same in numpy.
 *
 * Layout and colours as mg3d_kernels.hip: idx = plane*i + pitch*j + k; colour (ig0 + i + j + k) & 1, 1 = red.
 * Both stencil kernels give each thread one (j, k) column of `chunk` planes, lanes contiguous in k, and keep the
 * i-1 / i / i+1 values of v and eps of the column in registers (as residual_kernel does for v).
 *
 * Windows (the i-slabs of mg3d_dist.hip, conventions of k_sweep): [i_lo, i_hi) are the local planes a launch produces,
 * clipped to the interior 1 .. ni-2; [acc_lo, acc_hi) the local planes whose diff^2 enters the norm.  -1 / -1: every
 * plane, the launches of a single-domain level.
 */
#include "mg3d_internal.h"

#define WAVE 64

__device__ __forceinline__ long long cidx(const Geom &g, int i, int j, int k)
{
    return g.plane * i + (long long)g.pitch * j + k;
}

/* the weighted neighbour sum s and the diagonal dg of point p; eb / eh / ea and vb / va: eps and v of planes i-1, i, i+1
 * of the column (v of plane i itself is not part of the sum) */
__device__ __forceinline__ void coef_stencil(const Geom &g, const double *__restrict__ v, const double *__restrict__ e,
                                             long long p, double vb, double va, double eb, double eh, double ea,
                                             double shift, double &s, double &dg)
{
    const double a_im = 0.5 * (eh + eb);
    const double a_ip = 0.5 * (eh + ea);
    const double a_jm = 0.5 * (eh + e[p - g.pitch]);
    const double a_jp = 0.5 * (eh + e[p + g.pitch]);
    const double a_km = 0.5 * (eh + e[p - 1]);
    const double a_kp = 0.5 * (eh + e[p + 1]);
    double t = a_im * vb + a_ip * va;
    t = t + a_jm * v[p - g.pitch];
    t = t + a_jp * v[p + g.pitch];
    t = t + a_km * v[p - 1];
    t = t + a_kp * v[p + 1];
    s = t;
    double D = a_im + a_ip;
    D = D + a_jm;
    D = D + a_jp;
    D = D + a_km;
    D = D + a_kp;
    dg = D + shift;
}

/* ------------------------------------------------------------------ smoother
 * One red-black colour pass in place.  A thread updates the points of its column that have colour `color` (every other
 * plane); everything it reads -- the six neighbours -- has the other colour, which this pass never writes.  Boundary
 * points are never written. */
__global__ void __launch_bounds__(256) coef_color_kernel(Geom g, double *__restrict__ v, const double *__restrict__ e,
                                                         const double *__restrict__ d, double hSq, double shift,
                                                         int color, int chunk, int i_lo, int i_hi)
{
    const int k = 1 + blockIdx.x * WAVE + threadIdx.x;
    const int j = 1 + blockIdx.y * 4 + threadIdx.y;
    const int i0 = i_lo + blockIdx.z * chunk;
    const int i1 = min(i0 + chunk, i_hi);
    if (k > g.nk - 2 || j > g.nj - 2)
        return;
    long long p = cidx(g, i0, j, k);
    double vb = v[p - g.plane], vh = v[p];
    double eb = e[p - g.plane], eh = e[p];
    for (int i = i0; i < i1; i++, p += g.plane) {
        const double va = v[p + g.plane], ea = e[p + g.plane];
        if (((g.ig0 + i + j + k) & 1) == color) {
            double s, dg;
            coef_stencil(g, v, e, p, vb, va, eb, eh, ea, shift, s, dg);
            v[p] = (s - hSq * d[p]) / dg;
        }
        /* (a point updated here is the i-1 neighbour of a plane this pass does not update: its old value is never used) */
        vb = vh;
        vh = va;
        eb = eh;
        eh = ea;
    }
}

/* chunk of planes per thread: 16 as residual_kernel, doubled until the partial sums fit */
static int coef_chunk(int planes, int gx, int gy)
{
    int chunk = 16;
    while ((long long)gx * gy * ((planes + chunk - 1) / chunk) > MG3D_MAX_PARTIALS)
        chunk *= 2;
    return chunk;
}

/* the window [i_lo, i_hi) clipped to the interior planes 1 .. ni-2; false: nothing to produce */
static bool coef_window(const Geom &g, int &i_lo, int &i_hi)
{
    if (g.ni < 3 || g.nj < 3 || g.nk < 3)
        return false;
    i_lo = i_lo < 1 ? 1 : i_lo;
    i_hi = (i_hi < 0 || i_hi > g.ni - 1) ? g.ni - 1 : i_hi;
    return i_hi > i_lo;
}

void k_coef_color(const Geom &g, double *v, const double *e, const double *d, double hSq, double shift, int color,
                  hipStream_t s, int i_lo, int i_hi)
{
    if (!coef_window(g, i_lo, i_hi))
        return;
    const int gx = (g.nk - 2 + WAVE - 1) / WAVE, gy = (g.nj - 2 + 3) / 4;
    const int chunk = coef_chunk(i_hi - i_lo, gx, gy);
    const int gz = (i_hi - i_lo + chunk - 1) / chunk;
    hipLaunchKernelGGL(coef_color_kernel, dim3(gx, gy, gz), dim3(WAVE, 4, 1), 0, s, g, v, e, d, hSq, shift, color, chunk,
                       i_lo, i_hi);
}

/* ------------------------------------------------------------------ residual
 * diff on the interior; res (optional) receives it there, partials one sum of diff^2 per block (lanes by shuffle tree,
 * waves 0..3 in order -- the fixed order of mg3d_kernels.hip), folded by k_fold. */
__device__ __forceinline__ double coef_block_sum(double x, double *lds4)
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

__global__ void __launch_bounds__(256) coef_residual_kernel(Geom g, const double *__restrict__ v,
                                                            const double *__restrict__ e, const double *__restrict__ d,
                                                            double invHsq, double shift, double *__restrict__ res,
                                                            double *__restrict__ partials, int chunk, int i_lo,
                                                            int i_hi, int acc_lo, int acc_hi)
{
    __shared__ double lds4[4];
    const int k = 1 + blockIdx.x * WAVE + threadIdx.x;
    const int j = 1 + blockIdx.y * 4 + threadIdx.y;
    const int i0 = i_lo + blockIdx.z * chunk;
    const int i1 = min(i0 + chunk, i_hi);
    double acc = 0.;
    if (k <= g.nk - 2 && j <= g.nj - 2) {
        long long p = cidx(g, i0, j, k);
        double vb = v[p - g.plane], vh = v[p];
        double eb = e[p - g.plane], eh = e[p];
        for (int i = i0; i < i1; i++, p += g.plane) {
            const double va = v[p + g.plane], ea = e[p + g.plane];
            double s, dg;
            coef_stencil(g, v, e, p, vb, va, eb, eh, ea, shift, s, dg);
            const double diff = d[p] - invHsq * (s - dg * vh);
            if (res)
                res[p] = diff;
            if (i >= acc_lo && i < acc_hi)
                acc += diff * diff;
            vb = vh;
            vh = va;
            eb = eh;
            eh = ea;
        }
    }
    const double tot = coef_block_sum(acc, lds4);
    if (threadIdx.x == 0 && threadIdx.y == 0)
        partials[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tot;
}

void k_coef_residual(const Geom &g, const double *v, const double *e, const double *d, double invHsq, double shift,
                     double *res, double *partials, double *sumsq_out, hipStream_t s, int i_lo, int i_hi, int acc_lo,
                     int acc_hi)
{
    if (!coef_window(g, i_lo, i_hi)) {
        (void)hipMemsetAsync(sumsq_out, 0, sizeof(double), s);
        return;
    }
    if (acc_hi < 0)
        acc_hi = g.ni;
    const int gx = (g.nk - 2 + WAVE - 1) / WAVE, gy = (g.nj - 2 + 3) / 4;
    const int chunk = coef_chunk(i_hi - i_lo, gx, gy);
    const int gz = (i_hi - i_lo + chunk - 1) / chunk;
    hipLaunchKernelGGL(coef_residual_kernel, dim3(gx, gy, gz), dim3(WAVE, 4, 1), 0, s, g, v, e, d, invHsq, shift, res,
                       partials, chunk, i_lo, i_hi, acc_lo, acc_hi);
    k_fold(partials, gx * gy * gz, sumsq_out, s);
}

/* ----------------------------------------------------------------- injection
 * eps of the coarse level at every point, boundary included: ec[I,J,K] = ef[2I,2J,2K] (single-domain levels) */
__global__ void __launch_bounds__(256) coef_inject_kernel(Geom gf, const double *__restrict__ ef, Geom gc,
                                                          double *__restrict__ ec)
{
    const int kc = blockIdx.x * WAVE + threadIdx.x;
    const int jc = blockIdx.y * 4 + threadIdx.y;
    const int ic = blockIdx.z;
    if (kc >= gc.nk || jc >= gc.nj)
        return;
    ec[cidx(gc, ic, jc, kc)] = ef[cidx(gf, 2 * ic, 2 * jc, 2 * kc)];
}

void k_coef_inject(const Geom &gf, const double *ef, const Geom &gc, double *ec, hipStream_t s)
{
    dim3 grid((gc.nk + WAVE - 1) / WAVE, (gc.nj + 3) / 4, gc.ni);
    hipLaunchKernelGGL(coef_inject_kernel, grid, dim3(WAVE, 4, 1), 0, s, gf, ef, gc, ec);
}
