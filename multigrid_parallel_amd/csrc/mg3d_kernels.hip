/*
 * mg3d_kernels.hip -- gfx950 kernels of the multigrid V-cycle outside the fused sweeps.
 *
 * Arithmetic contract: every expression keeps the reference's association
 * (cited per kernel) and the file is compiled with -ffp-contract=off, so each
 * grid value is bit-identical to the reference CPU path; only the residual
 * norm's summation order differs (deterministic two-stage tree here).
 *
 * Layout: idx = plane*i + pitch*j + k (k contiguous, 128-byte aligned rows).
 * Colour of a point: (ig0 + i + j + k) & 1; 1 = red, 0 = black (mg_3d.h:669,693).
 *
 * Operators of the colour pass and the residual (neighbours in the reference's order i-, i+, j-, j+, k-, k+):
 *   constant (LevelOp: the screened 7-point Laplacian, sigma >= 0):
 *     s = (((((v[p-NN] + v[p+NN]) + v[p-N]) + v[p+N]) + v[p-1]) + v[p+1])
 *     smoother : v[p] = sixth * (s - hSq*d[p])                      (smoothenAtIndex, mg_3d.h:438-443)
 *     residual : diff = d[p] - invHsq * (s - dg*v[p])               (calculateResidual, mg_3d.h:819-821)
 *   variable coefficient (mg3d_ctx_set_coefficient): div(eps grad u) - sigma u = d, eps > 0 vertex-centred, one value
 *   per grid point of every level; face coefficients are arithmetic means:
 *     a_im = 0.5*(e[p] + e[p-NN]), a_ip = 0.5*(e[p] + e[p+NN]), ... a_kp = 0.5*(e[p] + e[p+1])
 *     s    = (((((a_im*v[p-NN] + a_ip*v[p+NN]) + a_jm*v[p-N]) + a_jp*v[p+N]) + a_km*v[p-1]) + a_kp*v[p+1])
 *     D    = ((((a_im + a_ip) + a_jm) + a_jp) + a_km) + a_kp;   dg = D + sigma*hSq
 *     smoother : v[p] = (s - hSq*d[p]) / dg          (IEEE division)
 *     residual : diff = d[p] - invHsq*(s - dg*v[p])
 *   Coarse levels take eps by injection, e_{l-1}[I,J,K] = e_l[2I,2J,2K].  tests/_coef_ref.py states the same in numpy.
 *
 * Periodic axes (mg3d_ctx_set_periodic; axes is a mask, MG3D_PERIODIC_I = 1, _J = 2, _K = 4; single-domain levels only:
 * ig0 = 0, ni = nj = nk = N).  A level keeps its N points per side; on a periodic axis index N-1 is the DUPLICATE of
 * index 0 and the unique points are 0 .. N-2 (an even count, so red-black colours agree across the wrap).  On a
 * non-periodic axis the faces 0 and N-1 stay Dirichlet points that no kernel here writes.
 *   - Nothing reads a duplicate: a stencil reaches across the wrap to the unique point (i-1 at i = 0 is N-2, i+1 at N-2
 *     is 0), and every kernel that writes a unique point on a periodic face also writes its duplicates (edges and
 *     corners included), so written fields are always periodic-consistent.
 *   - Colour pass and residual keep the arithmetic above exactly; only neighbour indices change.
 *   - Restriction: the 27-point full weighting (one order, restrict_kernel) on every coarse point that lies on no
 *     Dirichlet face, with wrapped fine neighbours on periodic axes; Dirichlet faces are injected as before.
 *   - Prolongation: the one parent order (stated at the prolongation kernels), the coarse "high" parent wrapped to 0 on
 *     a periodic axis.
 *   tests/_periodic_ref.py states the same in numpy.
 *
 * Neumann faces (mg3d_ctx_set_neumann; a mask of MG3D_NEUMANN_ILO = 1, _IHI = 2, _JLO = 4, _JHI = 8, _KLO = 16, _KHI = 32
 * on the non-periodic axes; single-domain levels only).  A point on a Neumann face is an unknown; where it also lies on
 * a Dirichlet face it is a Dirichlet point.  Nothing is duplicated and nothing lies outside the array: homogeneous
 * du/dn = 0 is imposed by REFLECTION -- at index 0 of a Neumann low face the -1 neighbour is read at index 1, at N-1 of
 * a Neumann high face the +1 neighbour at N-2, for v and for eps alike.  The unknowns of an axis are [lo, hi] with lo = 0
 * on a periodic axis or a Neumann low face, else 1, and hi = N-1 on a Neumann high face, else N-2.
 *   - Colour pass and residual keep the arithmetic above exactly; a reflected neighbour has the other colour.
 *   - Restriction: full weighting on every coarse unknown, reflected fine neighbours at Neumann faces.
 *   - Prolongation: unchanged -- every parent of a fine face point lies on the same face.
 *   tests/_neumann_ref.py states the same in numpy.
 *
 * Fixed points (mg3d_ctx_set_mask): a level may carry one byte per point in its padded layout (the index of the doubles),
 * nonzero = fixed.  A fixed unknown is a Dirichlet point: the colour pass skips it, the residual is 0. there (stored as
 * 0., d not read, +0. into the norm), q = A p is 0. there, the prolongation skips it; its neighbours read it through the
 * ordinary stencil.  Bytes on Dirichlet faces lie outside every launch; bytes on periodic duplicates are never read.
 * Coarse levels take the mask by injection.  tests/_mask_ref.py states the same in numpy.
 *
 * Screening field (mg3d_ctx_set_shift_field): a level may carry one double s >= 0 per point in its padded layout, and its
 * operator is div(eps grad u) - (sigma + s) u: s, D and every expression above stay, with dg = D + (sigma + s[p])*hSq formed
 * per point in this order.  Only the eps kernels have the form (SFIELD); a context without eps runs them over eps = 1 at
 * every point, where 0.5*(1 + 1) is 1, 1*v is v and D is 6.  Coarse levels take s by the restriction below (full weighting
 * at the unknowns, injection on Dirichlet faces).  tests/_shift_field_ref.py states the same in numpy.
 *
 * The launchers take both masks as one boundary word bc = periodic axes | Neumann faces << 3 (mg3d_bc); the stencil
 * kernels are instantiated per boundary mode: BC_PLAIN (bc = 0), BC_WRAP (periodic axes only), BC_REFLECT (a Neumann
 * face, with or without periodic axes).
 */
#include "mg3d_internal.h"

#include <assert.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <type_traits>

#define WAVE 64

__device__ __forceinline__ long long gidx(const Geom &g, int i, int j, int k)
{
    return g.plane * i + (long long)g.pitch * j + k;
}

/* boundary modes of the stencil kernels and the bits of the boundary word */
enum { BC_PLAIN = 0, BC_WRAP = 1, BC_REFLECT = 2 };
static inline int bc_mode(int bc) { return (bc >> 3) ? BC_REFLECT : (bc ? BC_WRAP : BC_PLAIN); }
/* the one launch ladder: f(coef, mode, mask) with eps set or not, the boundary mode of bc and whether the level has fixed
 * points (m) as compile-time constants --
 * dispatch_op(e, bc, m, [&](auto coef, auto mode, auto mask) { launch_op(mask, OP_KERNELS(kernel, coef(), mode(), false), ...); })
 * (the `false`: no screening field; a launcher of the eps side asks for A.s itself and takes OP_KERNELS_FIELD, below) */
template <class F>
static void dispatch_op(const double *e, int bc, const unsigned char *m, F f)
{
    const auto with_mode = [&](auto coef, auto mask) {
        switch (bc_mode(bc)) {
        case BC_REFLECT:
            return f(coef, std::integral_constant<int, BC_REFLECT>(), mask);
        case BC_WRAP:
            return f(coef, std::integral_constant<int, BC_WRAP>(), mask);
        default:
            return f(coef, std::integral_constant<int, BC_PLAIN>(), mask);
        }
    };
    const auto with_coef = [&](auto mask) {
        if (e)
            with_mode(std::true_type(), mask);
        else
            with_mode(std::false_type(), mask);
    };
    if (m)
        with_coef(std::true_type());
    else
        with_coef(std::false_type());
}
/* MASK, the third constant of the family: the kernel takes the level's fixed-point bytes as one more, LAST argument.  The
 * MASK = false instantiation has no such argument at all -- its argument list, and with it its code, is what it was before
 * the flag existed.  launch_op appends m for the instantiation that takes it. */
typedef const unsigned char *__restrict__ MaskPtr;
__device__ __forceinline__ bool mask_fixed(long long) { return false; }
__device__ __forceinline__ bool mask_fixed(long long p, const unsigned char *m) { return m[p] != 0; }
#define OP_KERNELS(kernel, ...) kernel<__VA_ARGS__, false>, kernel<__VA_ARGS__, true, MaskPtr>
template <class Mask, class... P0, class... P1, class... A>
static void launch_op(Mask, void (*plain)(P0...), void (*masked)(P1...), dim3 grid, dim3 block, hipStream_t s,
                      const unsigned char *m, A... args)
{
    if constexpr (Mask::value)
        hipLaunchKernelGGL(masked, grid, block, 0, s, args..., m);
    else
        hipLaunchKernelGGL(plain, grid, block, 0, s, args...);
}
/* SFIELD, the fourth constant, on the eps side of the family only: the level has a screening field s (mg3d_ctx_set_shift_field)
 * and the diagonal is dg = D + (sigma + s[p])*hSq, formed per point in this order.  The kernel takes the field and hSq as
 * one more trailing argument, in front of the mask; the argument every kernel has for sigma*hSq carries sigma itself.  s is
 * read at the point's own offset, lanes contiguous in k, as d is.  As with MASK, the SFIELD = false instantiations have no
 * such argument: their argument lists and their code are what they were. */
struct FieldArg {
    const double *__restrict__ s;
    double hSq;
};
#define OP_KERNELS_FIELD(kernel, ...) kernel<__VA_ARGS__, true, false, FieldArg>, kernel<__VA_ARGS__, true, true, FieldArg, MaskPtr>
/* the trailing arguments of an instantiation are (), (m), (f) or (f, m): the point's diagonal term beside D, and is it fixed */
__device__ __forceinline__ double point_dg0(double dg0, long long) { return dg0; }
__device__ __forceinline__ double point_dg0(double dg0, long long, const unsigned char *) { return dg0; }
template <class... M> __device__ __forceinline__ double point_dg0(double sigma, long long p, FieldArg f, M...)
{
    return (sigma + f.s[p]) * f.hSq;
}
__device__ __forceinline__ bool mask_fixed(long long p, FieldArg, const unsigned char *m) { return m[p] != 0; }
/* is the low / high face of axis ax (0 i, 1 j, 2 k) a Neumann face */
__host__ __device__ __forceinline__ bool bc_ref_lo(int bc, int ax) { return (bc >> (3 + 2 * ax)) & 1; }
__host__ __device__ __forceinline__ bool bc_ref_hi(int bc, int ax) { return (bc >> (4 + 2 * ax)) & 1; }

/* the offsets to the -1 / +1 neighbour along an axis of stride `st` at index x (an unknown): plain, wrapped when the axis
 * is periodic (0 reads N-2, N-2 reads 0), reflected at a Neumann face (rlo: 0 reads 1; rhi: N-1 reads N-2) */
__device__ __forceinline__ long long nb_lo(int x, int N, bool per, bool rlo, long long st)
{
    return (per && x == 0) ? (N - 2) * st : ((rlo && x == 0) ? st : -st);
}
__device__ __forceinline__ long long nb_hi(int x, int N, bool per, bool rhi, long long st)
{
    return (per && x == N - 2) ? -(N - 2) * st : ((rhi && x == N - 1) ? -st : st);
}

/* is (i, j, k) an unknown of a single-domain level: no periodic duplicate, on no Dirichlet face */
__device__ __forceinline__ bool bc_unknown(int bc, int N, int i, int j, int k)
{
    const int x[3] = {i, j, k};
    bool unk = true;
    for (int ax = 0; ax < 3; ax++)
        unk = unk && ((bc >> ax & 1) ? x[ax] != N - 1
                                     : !((x[ax] == 0 && !bc_ref_lo(bc, ax)) || (x[ax] == N - 1 && !bc_ref_hi(bc, ax))));
    return unk;
}

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

/* ------------------------------------------------------------------ stencils
 * One kernel family for the colour pass and the residual of every operator above, templated on what differs:
 *   COEF  eps is set: face means and an IEEE division instead of the constant `sixth`
 *   BC    the boundary mode: BC_PLAIN folds to the plain offsets; BC_WRAP an axis is periodic: wrapped neighbour offsets
 *         and duplicate stores; BC_REFLECT a face is a Neumann face: reflected offsets there, the unknowns of an axis are
 *         [lo, hi], and whatever axis is periodic beside it wraps as in BC_WRAP
 *   MASK  the level has fixed points: one byte per point and pass, read where the point's own d would be (lanes
 *         contiguous in k, as the walk has them); the bytes are the pack M of one trailing argument
 *   SFIELD (with COEF only) the level has a screening field: dg = D + (sigma + s[p])*hSq, one more double per point and pass,
 *         read where the point's own d is (FieldArg)
 * The residual and the colour pass with eps give each thread one (j, k) column of `chunk` planes, lanes contiguous in
 * k, and keep the i-1 / i / i+1 values of v (and eps) of the column in registers; the constant colour pass gives a lane
 * one k-pair of a row (measured at 513^3 the column form of that pass took 0.76 ms against 0.64 ms).
 *
 * Windows (the i-slabs of mg3d_dist.hip, conventions of k_sweep): [i_lo, i_hi) are the local planes a launch produces,
 * clipped to the unique interior planes; [acc_lo, acc_hi) the local planes whose diff^2 enters the norm.  -1 / -1: every
 * plane, the launches of a single-domain level. */

/* neighbour sum s and diagonal dg of point p; vb / va and eb / eh / ea: v and eps of planes i-1, i, i+1 of the column
 * (v of plane i itself is not part of the sum), oj* / ok*: the column's j and k neighbour offsets */
template <bool COEF>
__device__ __forceinline__ void stencil(const double *__restrict__ v, const double *__restrict__ e, long long p,
                                        long long ojm, long long ojp, long long okm, long long okp, double vb, double va,
                                        double eb, double eh, double ea, double dg0, double &s, double &dg)
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

/* one thread's column: planes [i0, i1) of row j, column k; the first unknown j and k are 0 on a periodic axis or a
 * Neumann low face, 1 otherwise, the last N-1 on a Neumann high face, else N-2 (the launcher clips [i_lo, i_hi) the same
 * way); pi / dj / dk: the axis wraps at i = 0 / this row / this column has duplicates; ril / rih: the i axis reflects at
 * 0 / at N-1.  A periodic or Neumann level is single-domain (nj = nk = N): its last unknown j and k are taken from N, as
 * the wrap is -- from nj / nk the eps kernels compile to 74 - 76 VGPRs, below occupancy 8 */
struct Column {
    int j, k, i0, i1;
    bool pi, dj, dk, ril, rih;
    long long ojm, ojp, okm, okp;
};

template <int BC>
__device__ __forceinline__ bool column(const Geom &g, int bc, int chunk, int i_lo, int i_hi, Column &c)
{
    const bool pj = BC && (bc & 2), pk = BC && (bc & 4);
    const bool rjl = BC == BC_REFLECT && bc_ref_lo(bc, 1), rjh = BC == BC_REFLECT && bc_ref_hi(bc, 1);
    const bool rkl = BC == BC_REFLECT && bc_ref_lo(bc, 2), rkh = BC == BC_REFLECT && bc_ref_hi(bc, 2);
    c.pi = BC && (bc & 1);
    c.ril = BC == BC_REFLECT && bc_ref_lo(bc, 0);
    c.rih = BC == BC_REFLECT && bc_ref_hi(bc, 0);
    c.k = ((pk || rkl) ? 0 : 1) + blockIdx.x * WAVE + threadIdx.x;
    c.j = ((pj || rjl) ? 0 : 1) + blockIdx.y * 4 + threadIdx.y;
    c.i0 = i_lo + blockIdx.z * chunk;
    c.i1 = min(c.i0 + chunk, i_hi);
    if (c.k > (BC ? g.N : g.nk) - (rkh ? 1 : 2) || c.j > (BC ? g.N : g.nj) - (rjh ? 1 : 2))
        return false;
    c.dj = pj && c.j == 0;
    c.dk = pk && c.k == 0;
    c.ojm = nb_lo(c.j, g.N, pj, rjl, g.pitch);
    c.ojp = nb_hi(c.j, g.N, pj, rjh, g.pitch);
    c.okm = nb_lo(c.k, g.N, pk, rkl, 1);
    c.okp = nb_hi(c.k, g.N, pk, rkh, 1);
    return true;
}

/* how many unknowns axis ax has beyond the ni-2 / nj-2 / nk-2 interior ones: index 0 (a periodic axis or a Neumann low
 * face) and index N-1 (a Neumann high face) */
static int bc_extra(int bc, int ax) { return ((bc >> ax & 1) || bc_ref_lo(bc, ax)) + bc_ref_hi(bc, ax); }

/* the window [i_lo, i_hi) clipped to the planes of unknowns (from 0 on a periodic i axis or a Neumann low face, else from
 * 1, up to ni-2, or ni-1 on a Neumann high face); false: nothing to produce */
static bool stencil_window(const Geom &g, int bc, int &i_lo, int &i_hi)
{
    if (g.ni < 3 - (bc & 1) || g.nj < 3 - (bc >> 1 & 1) || g.nk < 3 - (bc >> 2 & 1))
        return false;
    const int lo = ((bc & 1) || bc_ref_lo(bc, 0)) ? 0 : 1, hi = g.ni - 1 + bc_ref_hi(bc, 0);
    i_lo = i_lo < lo ? lo : i_lo;
    i_hi = (i_hi < 0 || i_hi > hi) ? hi : i_hi;
    return i_hi > i_lo;
}

/* the column grid: the unknown j and k of a level over (WAVE, 4) blocks; chunk of planes per thread: 16, doubled until
 * the partial sums fit */
static dim3 column_grid(const Geom &g, int bc, int planes, int &chunk)
{
    const int gx = (g.nk - 2 + bc_extra(bc, 2) + WAVE - 1) / WAVE, gy = (g.nj - 2 + bc_extra(bc, 1) + 3) / 4;
    chunk = 16;
    while ((long long)gx * gy * ((planes + chunk - 1) / chunk) > MG3D_MAX_PARTIALS)
        chunk *= 2;
    return dim3(gx, gy, (planes + chunk - 1) / chunk);
}

/* The column walk of every kernel below that keeps a column in registers: from plane c.i0 it carries v -- and eps with
 * COEF -- of the planes i-1, i, i+1 (the plane behind the first one through nb_lo, the plane ahead through nb_hi) and calls
 * body(pt) once per plane.  The stencil is the body's to evaluate: the colour pass skips it on the planes of the other
 * colour. */
template <bool COEF>
struct ColumnPoint {
    int i;       /* the plane */
    long long p; /* the point's offset */
    double vh;   /* v[p] as it was when the walk loaded it */
    const Column &c;
    const double *v; /* (not __restrict__, here and in the walk: the colour pass stores into v while the walk reads it) */
    const double *__restrict__ e;
    double vb, va, eb, eh, ea;
    /* the point lies on the periodic face i = 0: store_dup's first flag (the other two are c.dj, c.dk) */
    __device__ __forceinline__ bool di() const { return c.pi && i == 0; }
    /* stencil<COEF> at this point */
    __device__ __forceinline__ void sum(double dg0, double &s, double &dg) const
    {
        stencil<COEF>(v, e, p, c.ojm, c.ojp, c.okm, c.okp, vb, va, eb, eh, ea, dg0, s, dg);
    }
};

template <bool COEF, class Body>
__device__ __forceinline__ void walk_column(const Geom &g, const Column &c, const double *v, const double *__restrict__ e,
                                            Body body)
{
    long long p = gidx(g, c.i0, c.j, c.k);
    const long long pb = p + nb_lo(c.i0, g.N, c.pi, c.ril, g.plane);
    double vb = v[pb], vh = v[p];
    double eb = 0., eh = 0.;
    if constexpr (COEF) {
        eb = e[pb];
        eh = e[p];
    }
    for (int i = c.i0; i < c.i1; i++, p += g.plane) {
        const long long pa = p + nb_hi(i, g.N, c.pi, c.rih, g.plane);
        const double va = v[pa];
        double ea = 0.;
        if constexpr (COEF)
            ea = e[pa];
        body(ColumnPoint<COEF>{i, p, vh, c, v, e, vb, va, eb, eh, ea});
        vb = vh;
        vh = va;
        if constexpr (COEF) {
            eb = eh;
            eh = ea;
        }
    }
}

/* ------------------------------------------------------------------ smoother
 * One red-black colour pass in place over the unique interior points.  Everything a point reads -- the six neighbours
 * -- has the other colour, which this pass never writes (the wrap joins 0 and N-2, of opposite parity); a duplicate has
 * its source's colour: it is written in the same pass and read by none.  Boundary points are never written.
 * Constant operator: each lane owns the k-pair (2m, 2m+1) of one row and updates the member whose colour is being
 * swept.  A periodic level is single-domain (ig0 = 0, ni = nj = nk = N): with PER its range and colour come from N and
 * axes alone -- taken from i_lo, ig0, nj and nk the launch ran 3.5 % slower at 257^3. */
template <int BC, bool MASK, class... M>
__global__ void __launch_bounds__(256) smooth_color_kernel(Geom g, double *__restrict__ v, const double *__restrict__ d,
                                                           double hSq, double sixth, int color, int bc, int i_lo, M... fixed)
{
    static_assert(sizeof...(M) == (MASK ? 1 : 0), "MASK: the mask is the one trailing argument");
    constexpr bool REF = BC == BC_REFLECT;
    const bool pi = BC && (bc & 1), pj = BC && (bc & 2), pk = BC && (bc & 4);
    const bool ril = REF && bc_ref_lo(bc, 0), rih = REF && bc_ref_hi(bc, 0), rjl = REF && bc_ref_lo(bc, 1),
               rjh = REF && bc_ref_hi(bc, 1), rkl = REF && bc_ref_lo(bc, 2), rkh = REF && bc_ref_hi(bc, 2);
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = ((pj || rjl) ? 0 : 1) + blockIdx.y * blockDim.y + threadIdx.y;
    const int i = (BC ? ((pi || ril) ? 0 : 1) : i_lo) + blockIdx.z;
    if (j > (BC ? g.N : g.nj) - (rjh ? 1 : 2))
        return;
    const int k = 2 * m + ((color + (BC ? 0 : g.ig0) + i + j) & 1);
    if (k < ((pk || rkl) ? 0 : 1) || k > (BC ? g.N : g.nk) - (rkh ? 1 : 2))
        return;
    const long long p = gidx(g, i, j, k);
    if constexpr (MASK)
        if (mask_fixed(p, fixed...))
            return;
    double s = v[p + nb_lo(i, g.N, pi, ril, g.plane)] + v[p + nb_hi(i, g.N, pi, rih, g.plane)];
    s = s + v[p + nb_lo(j, g.N, pj, rjl, g.pitch)];
    s = s + v[p + nb_hi(j, g.N, pj, rjh, g.pitch)];
    s = s + v[p + nb_lo(k, g.N, pk, rkl, 1)];
    s = s + v[p + nb_hi(k, g.N, pk, rkh, 1)];
    s = s - hSq * d[p];
    store_dup(g, v, p, sixth * s, pi && i == 0, pj && j == 0, pk && k == 0);
}

/* eps set: a thread updates the points of its column that have colour `color` (every other plane) */
template <int BC, bool SFIELD, bool MASK, class... M>
__global__ void __launch_bounds__(256) coef_color_kernel(Geom g, double *__restrict__ v, const double *__restrict__ e,
                                                         const double *__restrict__ d, double hSq, double shift,
                                                         int color, int bc, int chunk, int i_lo, int i_hi, M... fixed)
{
    static_assert(sizeof...(M) == (SFIELD ? 1 : 0) + (MASK ? 1 : 0), "SFIELD, MASK: the field, then the mask, trail");
    Column c;
    if (!column<BC>(g, bc, chunk, i_lo, i_hi, c))
        return;
    /* (a point updated here is the i-1 neighbour of a plane this pass does not update: the old value the walk carries on
     * is never used) */
    walk_column<true>(g, c, v, e, [&](const ColumnPoint<true> &pt) {
        if (((g.ig0 + pt.i + c.j + c.k) & 1) != color)
            return;
        if constexpr (MASK)
            if (mask_fixed(pt.p, fixed...))
                return;
        double s, dg;
        pt.sum(point_dg0(shift, pt.p, fixed...), s, dg);
        store_dup(g, v, pt.p, (s - hSq * d[pt.p]) / dg, pt.di(), c.dj, c.dk);
    });
}

void k_smooth_color(const Geom &g, double *v, const double *d, const LevelOperator &A, int color, hipStream_t s, int i_lo,
                    int i_hi)
{
    if (!stencil_window(g, A.bc, i_lo, i_hi))
        return;
    const dim3 block(WAVE, 4, 1);
    dispatch_op(A.e, A.bc, A.m, [&](auto coef, auto mode, auto mask) {
        if constexpr (coef()) {
            int chunk;
            const dim3 grid = column_grid(g, A.bc, i_hi - i_lo, chunk);
            if (A.s)
                launch_op(mask, OP_KERNELS_FIELD(coef_color_kernel, mode()), grid, block, s, A.m, g, v, A.e, d, A.op.hSq, A.sigma,
                          color, A.bc, chunk, i_lo, i_hi, FieldArg{A.s, A.op.hSq});
            else
                launch_op(mask, OP_KERNELS(coef_color_kernel, mode(), false), grid, block, s, A.m, g, v, A.e, d, A.op.hSq,
                          A.sigma * A.op.hSq, color, A.bc, chunk, i_lo, i_hi);
        } else {
            const int pairs = (g.nk + 1) / 2;
            const dim3 grid((pairs + WAVE - 1) / WAVE, (g.nj - 2 + bc_extra(A.bc, 1) + 3) / 4, i_hi - i_lo);
            launch_op(mask, OP_KERNELS(smooth_color_kernel, mode()), grid, block, s, A.m, g, v, d, A.op.hSq, A.op.sixth, color,
                      A.bc, i_lo);
        }
    });
}

/* ------------------------------------------------------------ boundary fill
 * setupBoundaryConditions, mg_3d.h:1147-1239: v = BCFunc(i*h, j*h, k*h) = ((x*x) - ((2*y)*y)) + (z*z) on
 * every point of the six faces (mg_3d.h:89-90; same operation order as the C expression, no contraction). */
__global__ void __launch_bounds__(256) fill_boundary_kernel(Geom g, double *__restrict__ v, double h)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    const int j = blockIdx.y * 4 + threadIdx.y;
    const int i = blockIdx.z;
    if (k >= g.nk || j >= g.nj)
        return;
    const int ig = g.ig0 + i;
    if (!(ig == 0 || ig == g.N - 1 || j == 0 || j == g.nj - 1 || k == 0 || k == g.nk - 1))
        return;
    const double x = ig * h, y = j * h, z = k * h;
    v[gidx(g, i, j, k)] = x * x - 2 * y * y + z * z;
}

void k_fill_boundary(const Geom &g, double *v, double h, hipStream_t s)
{
    dim3 grid((g.nk + 63) / 64, (g.nj + 3) / 4, g.ni);
    hipLaunchKernelGGL(fill_boundary_kernel, grid, dim3(64, 4, 1), 0, s, g, v, h);
}

/* ------------------------------------------------------------- block reduce */
__device__ __forceinline__ double wave_sum(double x)
{
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1)
        x += __shfl_down(x, off, WAVE);
    return x;
}

/* sum over a 256-thread block, fixed order: lanes by shuffle tree, waves 0..3 sequentially */
__device__ __forceinline__ double block_sum_256(double x, double *lds4)
{
    const int tid = threadIdx.y * blockDim.x + threadIdx.x;
    x = wave_sum(x);
    if ((tid & (WAVE - 1)) == 0)
        lds4[tid / WAVE] = x;
    __syncthreads();
    return ((lds4[0] + lds4[1]) + lds4[2]) + lds4[3];
}

/* final stage: one block folds np partials in a fixed order */
__global__ void __launch_bounds__(256) fold_partials_kernel(const double *__restrict__ partials, int np,
                                                            double *__restrict__ out)
{
    __shared__ double lds4[4];
    double acc = 0.;
    for (int t = threadIdx.x; t < np; t += 256)
        acc += partials[t];
    const double tot = block_sum_256(acc, lds4);
    if (threadIdx.x == 0)
        *out = tot;
}

/* ------------------------------------------------------------------ residual
 * diff at every unique interior point; res (optional) receives it there and at the duplicates (mg_3d.h:824-825), partials
 * one sum of diff^2 per block (lanes by shuffle tree, waves 0..3 in order), folded by k_fold: the norm counts every
 * unknown once. */
template <bool COEF, int BC, bool SFIELD, bool MASK, class... M>
__global__ void __launch_bounds__(256) residual_kernel(Geom g, const double *__restrict__ v, const double *__restrict__ e,
                                                       const double *__restrict__ d, double invHsq, double dg0,
                                                       double *__restrict__ res, double *__restrict__ partials, int bc,
                                                       int chunk, int i_lo, int i_hi, int acc_lo, int acc_hi, M... fixed)
{
    static_assert(sizeof...(M) == (SFIELD ? 1 : 0) + (MASK ? 1 : 0), "SFIELD, MASK: the field, then the mask, trail");
    static_assert(COEF || !SFIELD, "SFIELD: the eps side only");
    __shared__ double lds4[4];
    double acc = 0.;
    Column c;
    if (column<BC>(g, bc, chunk, i_lo, i_hi, c)) {
        /* walk_column's walk written out: as a body of the walk, residual_kernel<false, 0> without r measured above the
         * parent's two runs in one of the two benches that time it (profiles/kernels_refactor_ab.txt), so the kernel keeps
         * its own copy; a change to the walk is made here too */
        long long p = gidx(g, c.i0, c.j, c.k);
        const long long pb = p + nb_lo(c.i0, g.N, c.pi, c.ril, g.plane);
        double vb = v[pb], vh = v[p];
        double eb = 0., eh = 0.;
        if constexpr (COEF) {
            eb = e[pb];
            eh = e[p];
        }
        for (int i = c.i0; i < c.i1; i++, p += g.plane) {
            const long long pa = p + nb_hi(i, g.N, c.pi, c.rih, g.plane);
            const double va = v[pa];
            double ea = 0.;
            if constexpr (COEF)
                ea = e[pa];
            double s, dg;
            stencil<COEF>(v, e, p, c.ojm, c.ojp, c.okm, c.okp, vb, va, eb, eh, ea, point_dg0(dg0, p, fixed...), s, dg);
            double diff;
            if constexpr (MASK) /* a fixed point: 0., whatever d and the sums hold */
                diff = mask_fixed(p, fixed...) ? 0. : d[p] - invHsq * (s - dg * vh);
            else
                diff = d[p] - invHsq * (s - dg * vh);
            if (res)
                store_dup(g, res, p, diff, c.pi && i == 0, c.dj, c.dk);
            if (BC || (i >= acc_lo && i < acc_hi)) /* periodic and Neumann levels have no windows */
                acc += diff * diff;
            vb = vh;
            vh = va;
            if constexpr (COEF) {
                eb = eh;
                eh = ea;
            }
        }
    }
    const double tot = block_sum_256(acc, lds4);
    if (threadIdx.x == 0 && threadIdx.y == 0)
        partials[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tot;
}

__global__ void __launch_bounds__(256) fold2_partials_kernel(const double *__restrict__ pa, int na,
                                                             const double *__restrict__ pb, int nb, double *__restrict__ out)
{
    __shared__ double lds4[4];
    double acc = 0.;
    for (int t = threadIdx.x; t < na; t += 256)
        acc += pa[t];
    const double ta = block_sum_256(acc, lds4);
    __syncthreads();
    acc = 0.;
    for (int t = threadIdx.x; t < nb; t += 256)
        acc += pb[t];
    const double tb = block_sum_256(acc, lds4);
    if (threadIdx.x == 0)
        *out = ta + tb;
}

void k_fold2(const double *pa, int na, const double *pb, int nb, double *out, hipStream_t s)
{
    hipLaunchKernelGGL(fold2_partials_kernel, dim3(1), dim3(256), 0, s, pa, na, pb, nb, out);
}

void k_fold(const double *partials, int np, double *out, hipStream_t s)
{
    hipLaunchKernelGGL(fold_partials_kernel, dim3(1), dim3(256), 0, s, partials, np, out);
}

/* the diagonal's constant term as the column kernels take it: sigma*h^2 beside the face means of eps, else op's 6 + sigma*h^2 */
static double op_dg0(const LevelOperator &A) { return A.e ? A.sigma * A.op.hSq : A.op.dg; }

void k_residual(const Geom &g, const double *v, const double *d, const LevelOperator &A, double *res, double *partials,
                double *sumsq_out, hipStream_t s, int i_lo, int i_hi, int acc_lo, int acc_hi)
{
    if (!stencil_window(g, A.bc, i_lo, i_hi)) {
        (void)hipMemsetAsync(sumsq_out, 0, sizeof(double), s);
        return;
    }
    if (acc_hi < 0)
        acc_hi = g.ni;
    int chunk;
    const dim3 grid = column_grid(g, A.bc, i_hi - i_lo, chunk), block(WAVE, 4, 1);
    dispatch_op(A.e, A.bc, A.m, [&](auto coef, auto mode, auto mask) {
        if constexpr (coef())
            if (A.s) {
                launch_op(mask, OP_KERNELS_FIELD(residual_kernel, true, mode()), grid, block, s, A.m, g, v, A.e, d, A.op.invHsq,
                          A.sigma, res, partials, A.bc, chunk, i_lo, i_hi, acc_lo, acc_hi, FieldArg{A.s, A.op.hSq});
                return;
            }
        launch_op(mask, OP_KERNELS(residual_kernel, coef(), mode(), false), grid, block, s, A.m, g, v, A.e, d, A.op.invHsq,
                  op_dg0(A), res, partials, A.bc, chunk, i_lo, i_hi, acc_lo, acc_hi);
    });
    k_fold(partials, (int)(grid.x * grid.y * grid.z), sumsq_out, s);
}

/* ------------------------------------------------------- conjugate gradients
 * The vector passes of mg3d_pcg_solve and mg3d_wpcg_solve (mg3d_pcg.hip) on one single-domain level.  Every pass
 * touches the unknowns only -- the points the residual counts -- so Dirichlet faces and periodic duplicates of its
 * operands are neither read as unknowns nor written; every sum is per-block partials folded by one block (k_fold).
 * With a Neumann face (BC_REFLECT, mg3d_wpcg_solve) the dots are taken in the inner product the reflected operator is
 * self-adjoint in: sum of w*a*b, w = 1/2 per Neumann face the point lies on -- computed from the point's index and the
 * boundary word, a power of two, so w*(a*b) is the rounded product scaled exactly.
 *
 * apply + dot: q = A p and sum of w*p*q.  The residual's column walk, neighbour offsets and operand order:
 * q = invHsq*(s - dg*p), which is what the residual subtracts from d. */
/* 1/2 when index x of axis ax lies on a Neumann face, else 1 */
__device__ __forceinline__ double bc_weight(int bc, int ax, int x, int N)
{
    return ((x == 0 && bc_ref_lo(bc, ax)) || (x == N - 1 && bc_ref_hi(bc, ax))) ? 0.5 : 1.;
}
template <bool COEF, int BC, bool SFIELD, bool MASK, class... M>
__global__ void __launch_bounds__(256) pcg_apply_kernel(Geom g, const double *__restrict__ v, const double *__restrict__ e,
                                                        double invHsq, double dg0, double *__restrict__ q,
                                                        double *__restrict__ partials, int bc, int chunk, int i_lo,
                                                        int i_hi, M... fixed)
{
    static_assert(sizeof...(M) == (SFIELD ? 1 : 0) + (MASK ? 1 : 0), "SFIELD, MASK: the field, then the mask, trail");
    static_assert(COEF || !SFIELD, "SFIELD: the eps side only");
    __shared__ double lds4[4];
    double acc = 0.;
    Column c;
    if (column<BC>(g, bc, chunk, i_lo, i_hi, c)) {
        double wjk = 1.;
        if constexpr (BC == BC_REFLECT)
            wjk = bc_weight(bc, 1, c.j, g.N) * bc_weight(bc, 2, c.k, g.N);
        walk_column<COEF>(g, c, v, e, [&](const ColumnPoint<COEF> &pt) {
            double s, dg;
            pt.sum(point_dg0(dg0, pt.p, fixed...), s, dg);
            double ap;
            if constexpr (MASK) /* a fixed point: q = 0. (p is 0. there, so nothing enters the dot) */
                ap = mask_fixed(pt.p, fixed...) ? 0. : invHsq * (s - dg * pt.vh);
            else
                ap = invHsq * (s - dg * pt.vh);
            q[pt.p] = ap;
            if constexpr (BC == BC_REFLECT)
                acc += (wjk * bc_weight(bc, 0, pt.i, g.N)) * (pt.vh * ap);
            else
                acc += pt.vh * ap;
        });
    }
    const double tot = block_sum_256(acc, lds4);
    if (threadIdx.x == 0 && threadIdx.y == 0)
        partials[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tot;
}

int k_pcg_apply_dot(const Geom &g, const double *p, const LevelOperator &A, double *q, double *partials, double *dot_out,
                    hipStream_t s)
{
    int i_lo = -1, i_hi = -1;
    if (!stencil_window(g, A.bc, i_lo, i_hi)) {
        (void)hipMemsetAsync(dot_out, 0, sizeof(double), s);
        return 0;
    }
    int chunk;
    const dim3 grid = column_grid(g, A.bc, i_hi - i_lo, chunk), block(WAVE, 4, 1);
    dispatch_op(A.e, A.bc, A.m, [&](auto coef, auto mode, auto mask) {
        if constexpr (coef())
            if (A.s) {
                launch_op(mask, OP_KERNELS_FIELD(pcg_apply_kernel, true, mode()), grid, block, s, A.m, g, p, A.e, A.op.invHsq,
                          A.sigma, q, partials, A.bc, chunk, i_lo, i_hi, FieldArg{A.s, A.op.hSq});
                return;
            }
        launch_op(mask, OP_KERNELS(pcg_apply_kernel, coef(), mode(), false), grid, block, s, A.m, g, p, A.e, A.op.invHsq,
                  op_dg0(A), q, partials, A.bc, chunk, i_lo, i_hi);
    });
    const int np = (int)(grid.x * grid.y * grid.z);
    k_fold(partials, np, dot_out, s);
    return np;
}

/* The streaming passes.  A lane owns the aligned k-pair (2m, 2m+1) of a row -- one 16-byte access per operand; rows are
 * 128-byte aligned and a pair never leaves its row's pitch -- over `chunk` planes; the member of a pair that is no
 * unknown (a Dirichlet face, the duplicate k = N-1) keeps the value that was loaded.  The unknowns of an axis are
 * [lo, hi]: lo 0 on a periodic axis or a Neumann low face, else 1; hi N-1 on a Neumann high face, else N-2 (N is odd
 * and rows are padded to a multiple of 16 doubles: the pair (N-1, N) stays inside its row's pitch). */
struct PairRange {
    int lo[3], hi[3];
};
struct PairWalk {
    long long p;
    int i0, j, k;
    int n; /* planes */
    bool m0, m1;
};
__device__ __forceinline__ bool pair_walk(const Geom &g, const PairRange &u, int chunk, PairWalk &w)
{
    w.k = 2 * (blockIdx.x * WAVE + threadIdx.x);
    w.j = u.lo[1] + blockIdx.y * 4 + threadIdx.y;
    w.i0 = u.lo[0] + blockIdx.z * chunk;
    if (w.k > u.hi[2] || w.j > u.hi[1])
        return false;
    w.m0 = w.k >= u.lo[2];
    w.m1 = w.k + 1 <= u.hi[2];
    w.n = min(chunk, u.hi[0] + 1 - w.i0);
    w.p = gidx(g, w.i0, w.j, w.k);
    return true;
}
__device__ __forceinline__ bool pcg_finite_neg(double x) { return x < 0. && x >= -1.7976931348623157e308; }

/* update + norm: alpha = (r.z)/(p.Ap); x += alpha p, r -= alpha q, sum of r*r.  The operator is negative definite: both
 * dots are negative in a healthy iteration.  Otherwise (breakdown) nothing is written -- x stays the last good iterate --
 * and the host, which reads the same two numbers, ends the solve. */
__global__ void __launch_bounds__(256) pcg_update_kernel(Geom g, double *__restrict__ x, double *__restrict__ r,
                                                         const double *__restrict__ pv, const double *__restrict__ qv,
                                                         const double *__restrict__ rz, const double *__restrict__ pap,
                                                         double *__restrict__ partials, PairRange u, int chunk)
{
    __shared__ double lds4[4];
    double acc = 0.;
    PairWalk w;
    const double num = *rz, den = *pap;
    const bool ok = pcg_finite_neg(num) && pcg_finite_neg(den);
    if (ok && pair_walk(g, u, chunk, w)) {
        const double alpha = num / den;
        for (int t = 0; t < w.n; t++, w.p += g.plane) {
            double2 xx = *reinterpret_cast<double2 *>(x + w.p), rr = *reinterpret_cast<double2 *>(r + w.p);
            const double2 pp = *reinterpret_cast<const double2 *>(pv + w.p), qq = *reinterpret_cast<const double2 *>(qv + w.p);
            if (w.m0) {
                xx.x = xx.x + alpha * pp.x;
                rr.x = rr.x - alpha * qq.x;
                acc += rr.x * rr.x;
            }
            if (w.m1) {
                xx.y = xx.y + alpha * pp.y;
                rr.y = rr.y - alpha * qq.y;
                acc += rr.y * rr.y;
            }
            *reinterpret_cast<double2 *>(x + w.p) = xx;
            *reinterpret_cast<double2 *>(r + w.p) = rr;
        }
    }
    const double tot = block_sum_256(acc, lds4);
    if (threadIdx.x == 0 && threadIdx.y == 0)
        partials[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tot;
}

/* dot: sum of a*b over the unknowns */
__global__ void __launch_bounds__(256) pcg_dot_kernel(Geom g, const double *__restrict__ a, const double *__restrict__ b,
                                                      double *__restrict__ partials, PairRange u, int chunk)
{
    __shared__ double lds4[4];
    double acc = 0.;
    PairWalk w;
    if (pair_walk(g, u, chunk, w)) {
        for (int t = 0; t < w.n; t++, w.p += g.plane) {
            const double2 aa = *reinterpret_cast<const double2 *>(a + w.p), bb = *reinterpret_cast<const double2 *>(b + w.p);
            if (w.m0)
                acc += aa.x * bb.x;
            if (w.m1)
                acc += aa.y * bb.y;
        }
    }
    const double tot = block_sum_256(acc, lds4);
    if (threadIdx.x == 0 && threadIdx.y == 0)
        partials[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tot;
}

/* direction: beta = (r.z)_new / (r.z)_old (Fletcher-Reeves); p = z + beta p */
__global__ void __launch_bounds__(256) pcg_direction_kernel(Geom g, double *__restrict__ pv, const double *__restrict__ z,
                                                            const double *__restrict__ rz_new,
                                                            const double *__restrict__ rz_old, PairRange u, int chunk)
{
    PairWalk w;
    if (!pair_walk(g, u, chunk, w))
        return;
    const double beta = *rz_new / *rz_old;
    for (int t = 0; t < w.n; t++, w.p += g.plane) {
        double2 pp = *reinterpret_cast<double2 *>(pv + w.p);
        const double2 zz = *reinterpret_cast<const double2 *>(z + w.p);
        if (w.m0)
            pp.x = zz.x + beta * pp.x;
        if (w.m1)
            pp.y = zz.y + beta * pp.y;
        *reinterpret_cast<double2 *>(pv + w.p) = pp;
    }
}

/* The weighted passes of mg3d_wpcg_solve.  wdot: sum of w*a*b and sum of w*b over the unknowns from one read of a and b
 * (r.z and, for the projection of the singular case, the w-sum of z), into two runs of partials. */
__device__ __forceinline__ double pair_weight(int bc, int N, int j, int k)
{
    return bc_weight(bc, 1, j, N) * bc_weight(bc, 2, k, N);
}
__global__ void __launch_bounds__(256) wpcg_dot_kernel(Geom g, const double *__restrict__ a, const double *__restrict__ b,
                                                       double *__restrict__ pab, double *__restrict__ pb, int bc,
                                                       PairRange u, int chunk)
{
    __shared__ double lds4[4];
    double acc = 0., sum = 0.;
    PairWalk w;
    if (pair_walk(g, u, chunk, w)) {
        const double w0 = pair_weight(bc, g.N, w.j, w.k), w1 = pair_weight(bc, g.N, w.j, w.k + 1);
        for (int t = 0; t < w.n; t++, w.p += g.plane) {
            const double2 aa = *reinterpret_cast<const double2 *>(a + w.p), bb = *reinterpret_cast<const double2 *>(b + w.p);
            const double wi = bc_weight(bc, 0, w.i0 + t, g.N);
            if (w.m0) {
                acc += (wi * w0) * (aa.x * bb.x);
                sum += (wi * w0) * bb.x;
            }
            if (w.m1) {
                acc += (wi * w1) * (aa.y * bb.y);
                sum += (wi * w1) * bb.y;
            }
        }
    }
    const int blk = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const double tot = block_sum_256(acc, lds4);
    if (threadIdx.x == 0 && threadIdx.y == 0)
        pab[blk] = tot;
    __syncthreads();
    const double tot_b = block_sum_256(sum, lds4);
    if (threadIdx.x == 0 && threadIdx.y == 0)
        pb[blk] = tot_b;
}

/* direction: p = (z - m) + beta p; m = *wsum / W, the w-mean of z (W = 0: no projection, m = 0), beta Fletcher-Reeves;
 * first: the direction of iteration 0, p = z - m, p is not read */
__global__ void __launch_bounds__(256) wpcg_direction_kernel(Geom g, double *__restrict__ pv, const double *__restrict__ z,
                                                             const double *__restrict__ rz_new,
                                                             const double *__restrict__ rz_old,
                                                             const double *__restrict__ wsum, double W, int first,
                                                             PairRange u, int chunk)
{
    PairWalk w;
    if (!pair_walk(g, u, chunk, w))
        return;
    const double m = W > 0. ? *wsum / W : 0.;
    const double beta = first ? 0. : *rz_new / *rz_old;
    for (int t = 0; t < w.n; t++, w.p += g.plane) {
        double2 pp = make_double2(0., 0.);
        if (!first)
            pp = *reinterpret_cast<double2 *>(pv + w.p);
        const double2 zz = *reinterpret_cast<const double2 *>(z + w.p);
        if (w.m0)
            pp.x = first ? zz.x - m : (zz.x - m) + beta * pp.x;
        if (w.m1)
            pp.y = first ? zz.y - m : (zz.y - m) + beta * pp.y;
        *reinterpret_cast<double2 *>(pv + w.p) = pp;
    }
}

/* the projection of the first residual in the singular case: r -= *wsum / W, sum of r*r */
__global__ void __launch_bounds__(256) wpcg_center_kernel(Geom g, double *__restrict__ r, const double *__restrict__ wsum,
                                                          double W, double *__restrict__ partials, PairRange u, int chunk)
{
    __shared__ double lds4[4];
    double acc = 0.;
    PairWalk w;
    if (pair_walk(g, u, chunk, w)) {
        const double m = *wsum / W;
        for (int t = 0; t < w.n; t++, w.p += g.plane) {
            double2 rr = *reinterpret_cast<double2 *>(r + w.p);
            if (w.m0) {
                rr.x = rr.x - m;
                acc += rr.x * rr.x;
            }
            if (w.m1) {
                rr.y = rr.y - m;
                acc += rr.y * rr.y;
            }
            *reinterpret_cast<double2 *>(r + w.p) = rr;
        }
    }
    const double tot = block_sum_256(acc, lds4);
    if (threadIdx.x == 0 && threadIdx.y == 0)
        partials[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tot;
}

/* the pair grid: the k-pairs (from 0 up to the last unknown k) and unknown rows of a level over (WAVE, 4) blocks, one
 * plane per block in z; planes per block doubled from 1 until the partial sums fit in `cap` */
static bool pair_grid(const Geom &g, int bc, dim3 &grid, int &chunk, PairRange &u, int cap)
{
    if (g.N < 3 || g.ni != g.N || g.nj != g.N || g.nk != g.N)
        return false;
    for (int ax = 0; ax < 3; ax++) {
        u.lo[ax] = ((bc >> ax & 1) || bc_ref_lo(bc, ax)) ? 0 : 1;
        u.hi[ax] = bc_ref_hi(bc, ax) ? g.N - 1 : g.N - 2;
    }
    const int pairs = u.hi[2] / 2 + 1, rows = u.hi[1] + 1 - u.lo[1], planes = u.hi[0] + 1 - u.lo[0];
    const int gx = (pairs + WAVE - 1) / WAVE, gy = (rows + 3) / 4;
    chunk = 1;
    while ((long long)gx * gy * ((planes + chunk - 1) / chunk) > cap)
        chunk *= 2;
    grid = dim3(gx, gy, (planes + chunk - 1) / chunk);
    return true;
}

/* one pair pass: kernel(g, args..., u, chunk) over the pair grid with room for CAP partial sums; the number of blocks --
 * of partial sums, where the kernel forms them -- or -1: the level has no launch shape, nothing launched */
template <int CAP = MG3D_MAX_PARTIALS, class... P, class... A>
static int pair_launch(void (*kernel)(Geom, P...), const Geom &g, int bc, hipStream_t s, A... args)
{
    dim3 grid;
    int chunk;
    PairRange u;
    if (!pair_grid(g, bc, grid, chunk, u, CAP))
        return -1;
    hipLaunchKernelGGL(kernel, grid, dim3(WAVE, 4, 1), 0, s, g, args..., u, chunk);
    return (int)(grid.x * grid.y * grid.z);
}

int k_pcg_update_norm(const Geom &g, int bc, double *x, double *r, const double *p, const double *q, const double *rz,
                      const double *pap, double *partials, double *rr_out, hipStream_t s)
{
    const int np = pair_launch(pcg_update_kernel, g, bc, s, x, r, p, q, rz, pap, partials);
    if (np > 0)
        k_fold(partials, np, rr_out, s);
    return np;
}

int k_pcg_dot(const Geom &g, int bc, const double *a, const double *b, double *partials, double *dot_out, hipStream_t s)
{
    const int np = pair_launch(pcg_dot_kernel, g, bc, s, a, b, partials);
    if (np > 0)
        k_fold(partials, np, dot_out, s);
    return np;
}

int k_pcg_direction(const Geom &g, int bc, double *p, const double *z, const double *rz_new, const double *rz_old,
                    hipStream_t s)
{
    return pair_launch(pcg_direction_kernel, g, bc, s, p, z, rz_new, rz_old) < 0 ? -1 : 0;
}

int k_wpcg_dot(const Geom &g, int bc, const double *a, const double *b, double *partials, double *dot_out, double *sum_out,
               hipStream_t s)
{
    double *const pb = partials + MG3D_MAX_PARTIALS / 2;
    const int np = pair_launch<MG3D_MAX_PARTIALS / 2>(wpcg_dot_kernel, g, bc, s, a, b, partials, pb, bc);
    if (np > 0) {
        k_fold(partials, np, dot_out, s);
        k_fold(pb, np, sum_out, s);
    }
    return np;
}

int k_wpcg_direction(const Geom &g, int bc, double *p, const double *z, const double *rz_new, const double *rz_old,
                     const double *wsum, double W, bool first, hipStream_t s)
{
    return pair_launch(wpcg_direction_kernel, g, bc, s, p, z, rz_new, rz_old, wsum, W, first ? 1 : 0) < 0 ? -1 : 0;
}

int k_wpcg_center(const Geom &g, int bc, double *r, const double *wsum, double W, double *partials, double *rr_out,
                  hipStream_t s)
{
    const int np = pair_launch(wpcg_center_kernel, g, bc, s, r, wsum, W, partials);
    if (np > 0)
        k_fold(partials, np, rr_out, s);
    return np;
}

double k_wpcg_weight_sum(const Geom &g, int bc)
{
    double W = 1.;
    for (int ax = 0; ax < 3; ax++) {
        const int lo = ((bc >> ax & 1) || bc_ref_lo(bc, ax)) ? 0 : 1, hi = bc_ref_hi(bc, ax) ? g.N - 1 : g.N - 2;
        W *= (hi + 1 - lo) - 0.5 * (bc_ref_lo(bc, ax) + bc_ref_hi(bc, ax));
    }
    return W;
}

/* ------------------------------------------------------------- time stepping
 * The right-hand side of one theta-step of mg3d_step_advance (mg3d_step.hip, include/mg3d.h) from u0 = v, written at the
 * unknowns only: Dirichlet points and periodic duplicates of d keep what they hold (nothing reads them).
 *     q    = invHsq*(s - dg*v[p])                 pcg_apply_kernel's expression, operand and neighbour order
 *     d[p] = -((a*v[p] + c1*q) + b*src[p])        src == NULL: d[p] = -(a*v[p] + c1*q)
 * theta < 1: pcg_apply_kernel's body on the column walk with one more operand and neither a sum nor partials.  src is a
 * uniform branch: the six instantiations stay six.  Both launches take the grids of the passes they are modelled on (column_grid,
 * pair_grid) as they are: the cap on blocks those keep for the partial sums means nothing here and does no harm. */
template <bool COEF, int BC, bool SFIELD, class... M>
__global__ void __launch_bounds__(256) step_rhs_kernel(Geom g, const double *__restrict__ v, const double *__restrict__ e,
                                                       const double *__restrict__ src, double invHsq, double dg0, double a,
                                                       double c1, double b, double *__restrict__ d, int bc, int chunk,
                                                       int i_lo, int i_hi, M... field)
{
    static_assert(sizeof...(M) == (SFIELD ? 1 : 0) && (COEF || !SFIELD), "SFIELD: the field trails, on the eps side only");
    Column c;
    if (!column<BC>(g, bc, chunk, i_lo, i_hi, c))
        return;
    walk_column<COEF>(g, c, v, e, [&](const ColumnPoint<COEF> &pt) {
        double s, dg;
        pt.sum(point_dg0(dg0, pt.p, field...), s, dg);
        const double q = invHsq * (s - dg * pt.vh);
        double t = a * pt.vh + c1 * q;
        if (src)
            t = t + b * src[pt.p];
        d[pt.p] = -t;
    });
}

/* theta == 1 (backward Euler): c1 = 0 and no stencil -- d[p] = -(a*v[p] + b*src[p]), or -(a*v[p]) without a source, as a
 * streaming pass over the k-pairs; the member of a pair that is no unknown keeps the d that was loaded */
__global__ void __launch_bounds__(256) step_rhs_be_kernel(Geom g, const double *__restrict__ v,
                                                          const double *__restrict__ src, double a, double b,
                                                          double *__restrict__ d, PairRange u, int chunk)
{
    PairWalk w;
    if (!pair_walk(g, u, chunk, w))
        return;
    for (int t = 0; t < w.n; t++, w.p += g.plane) {
        double2 dd = *reinterpret_cast<double2 *>(d + w.p);
        const double2 vv = *reinterpret_cast<const double2 *>(v + w.p);
        double2 x = make_double2(a * vv.x, a * vv.y);
        if (src) {
            const double2 ss = *reinterpret_cast<const double2 *>(src + w.p);
            x.x = x.x + b * ss.x;
            x.y = x.y + b * ss.y;
        }
        if (w.m0)
            dd.x = -x.x;
        if (w.m1)
            dd.y = -x.y;
        *reinterpret_cast<double2 *>(d + w.p) = dd;
    }
}

int k_step_rhs(const Geom &g, const double *u0, const double *src, const LevelOperator &A, double a, double c1, double b,
               bool backward_euler, double *d, hipStream_t s)
{
    if (backward_euler)
        return pair_launch(step_rhs_be_kernel, g, A.bc, s, u0, src, a, b, d) < 0 ? -1 : 0;
    if (g.N < 3 || g.ni != g.N || g.nj != g.N || g.nk != g.N)
        return -1;
    int i_lo = -1, i_hi = -1;
    if (!stencil_window(g, A.bc, i_lo, i_hi))
        return 0;
    int chunk;
    const dim3 grid = column_grid(g, A.bc, i_hi - i_lo, chunk), block(WAVE, 4, 1);
    /* (no MASK form: d at a fixed point is never read, what the pass writes there is unspecified) */
    dispatch_op(A.e, A.bc, nullptr, [&](auto coef, auto mode, auto) {
        if constexpr (coef())
            if (A.s) {
                hipLaunchKernelGGL((step_rhs_kernel<true, mode(), true, FieldArg>), grid, block, 0, s, g, u0, A.e, src,
                                   A.op.invHsq, A.sigma, a, c1, b, d, A.bc, chunk, i_lo, i_hi, FieldArg{A.s, A.op.hSq});
                return;
            }
        hipLaunchKernelGGL((step_rhs_kernel<coef(), mode(), false>), grid, block, 0, s, g, u0, A.e, src, A.op.invHsq, op_dg0(A), a,
                           c1, b, d, A.bc, chunk, i_lo, i_hi);
    });
    return 0;
}

/* ------------------------------------------------------------- the nonlinear term
 * mg3d_nl_residual and mg3d_nl_solve (mg3d_nl.hip, include/mg3d.h):  A u - g0*g(x)*phi(beta*(u - uref)) = d  with A the
 * level's operator WITHOUT a screening field.  The evaluation: residual_kernel's walk, neighbour offsets and operand order for
 * the linear part, then per unknown, uncontracted and in this order
 *     w   = beta*(v[p] - uref)
 *     ph  = exp(w), dph = ph              (KIND = MG3D_NL_EXP)     ph = sinh(w), dph = cosh(w)     (MG3D_NL_SINH)
 *     gp  = g0*gw[p]                      (WEIGHT; else gp = g0)
 *     lin = d[p] - invHsq*(s - dg*v[p])   residual_kernel's diff
 *     F   = lin + gp*ph                   the nonlinear residual d - (A u - gp*ph)
 *     sf  = (gp*beta)*dph                 the screening field of the linearisation A - sf
 * F (optional) is stored at the unknowns and their duplicates, sf (optional) at the unknowns (the install path refreshes the
 * field's duplicates); a fixed point has F = 0. and sf = 0., neither d nor gw is read there.  partials: one sum of F^2 per
 * block, residual_kernel's order; with sf, *bad += the block's count of sf that are not finite -- an integer, so the order of
 * the atomics does not matter.  exp, sinh and cosh are the device library's double functions: sinh keeps its relative
 * accuracy at small |w|, which a difference of exponentials would lose. */
struct NlTerm {
    double g0, beta, uref;
};
template <bool COEF, int BC, int KIND, bool WEIGHT, bool MASK, class... M>
__global__ void __launch_bounds__(256) nl_eval_kernel(Geom g, const double *__restrict__ v, const double *__restrict__ e,
                                                      const double *__restrict__ d, const double *__restrict__ gw,
                                                      double invHsq, double dg0, NlTerm nl, double *__restrict__ F,
                                                      double *__restrict__ sf, double *__restrict__ partials,
                                                      unsigned long long *__restrict__ bad, int bc, int chunk, int i_lo,
                                                      int i_hi, M... fixed)
{
    static_assert(sizeof...(M) == (MASK ? 1 : 0), "MASK: the mask trails");
    __shared__ double lds4[4];
    double acc = 0.;
    int nbad = 0;
    Column c;
    if (column<BC>(g, bc, chunk, i_lo, i_hi, c)) {
        walk_column<COEF>(g, c, v, e, [&](const ColumnPoint<COEF> &pt) {
            double s, dg;
            pt.sum(dg0, s, dg);
            double diff = 0., sv = 0.;
            if (!(MASK && mask_fixed(pt.p, fixed...))) {
                const double w = nl.beta * (pt.vh - nl.uref);
                double ph, dph;
                if constexpr (KIND == MG3D_NL_EXP) {
                    ph = exp(w);
                    dph = ph;
                } else {
                    ph = sinh(w);
                    dph = cosh(w);
                }
                double gp = nl.g0;
                if constexpr (WEIGHT)
                    gp = nl.g0 * gw[pt.p];
                const double lin = d[pt.p] - invHsq * (s - dg * pt.vh);
                diff = lin + gp * ph;
                sv = (gp * nl.beta) * dph;
            }
            if (F)
                store_dup(g, F, pt.p, diff, pt.di(), c.dj, c.dk);
            if (sf) {
                sf[pt.p] = sv;
                nbad += !(fabs(sv) <= 1.7976931348623157e308);
            }
            acc += diff * diff;
        });
    }
    const double tot = block_sum_256(acc, lds4);
    const bool first = threadIdx.x == 0 && threadIdx.y == 0;
    if (first)
        partials[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tot;
    if (sf) { /* (uniform: a kernel argument) */
        __syncthreads();
        const double nb = block_sum_256((double)nbad, lds4); /* at most 256 * chunk: exact */
        if (first && nb > 0.)
            atomicAdd(bad, (unsigned long long)nb);
    }
}

int k_nl_eval(const Geom &g, const double *v, const double *d, const LevelOperator &A, int kind, const double *gw, double g0,
              double beta, double uref, double *F, double *sf, double *partials, double *sumsq_out, unsigned long long *bad,
              hipStream_t s)
{
    if (g.N < 3 || g.ni != g.N || g.nj != g.N || g.nk != g.N || A.s)
        return -1;
    int i_lo = -1, i_hi = -1;
    if (!stencil_window(g, A.bc, i_lo, i_hi)) {
        (void)hipMemsetAsync(sumsq_out, 0, sizeof(double), s);
        return 0;
    }
    int chunk;
    const dim3 grid = column_grid(g, A.bc, i_hi - i_lo, chunk), block(WAVE, 4, 1);
    const NlTerm nl = {g0, beta, uref};
    dispatch_op(A.e, A.bc, A.m, [&](auto coef, auto mode, auto mask) {
        const auto go = [&](auto kd, auto wt) {
            launch_op(mask, OP_KERNELS(nl_eval_kernel, coef(), mode(), kd(), wt()), grid, block, s, A.m, g, v, A.e, d, gw,
                      A.op.invHsq, op_dg0(A), nl, F, sf, partials, bad, A.bc, chunk, i_lo, i_hi);
        };
        const auto with_kind = [&](auto wt) {
            if (kind == MG3D_NL_SINH)
                go(std::integral_constant<int, MG3D_NL_SINH>(), wt);
            else
                go(std::integral_constant<int, MG3D_NL_EXP>(), wt);
        };
        if (gw)
            with_kind(std::true_type());
        else
            with_kind(std::false_type());
    });
    const int np = (int)(grid.x * grid.y * grid.z);
    k_fold(partials, np, sumsq_out, s);
    return np;
}

/* The trial point of the line search, t = x + lambda*dl at the unknowns (their duplicates written with them); a fixed point
 * of m (NULL: no mask) takes x as it is.  Dirichlet points of t are not written: the caller copied them from x once.  The
 * column grid, one (j, k) column of `chunk` planes a thread, no stencil */
template <int BC>
__global__ void __launch_bounds__(256) nl_trial_kernel(Geom g, const double *__restrict__ x, const double *__restrict__ dl,
                                                       double lambda, double *__restrict__ t,
                                                       const unsigned char *__restrict__ m, int bc, int chunk, int i_lo,
                                                       int i_hi)
{
    Column c;
    if (!column<BC>(g, bc, chunk, i_lo, i_hi, c))
        return;
    long long p = gidx(g, c.i0, c.j, c.k);
    for (int i = c.i0; i < c.i1; i++, p += g.plane) {
        const double xv = x[p];
        const double tv = (m && m[p] != 0) ? xv : xv + lambda * dl[p];
        store_dup(g, t, p, tv, c.pi && i == 0, c.dj, c.dk);
    }
}

int k_nl_trial(const Geom &g, int bc, const double *x, const double *dl, double lambda, double *t, const unsigned char *m,
               hipStream_t s)
{
    if (g.N < 3 || g.ni != g.N || g.nj != g.N || g.nk != g.N)
        return -1;
    int i_lo = -1, i_hi = -1;
    if (!stencil_window(g, bc, i_lo, i_hi))
        return 0;
    int chunk;
    const dim3 grid = column_grid(g, bc, i_hi - i_lo, chunk), block(WAVE, 4, 1);
    switch (bc_mode(bc)) {
    case BC_REFLECT:
        hipLaunchKernelGGL(nl_trial_kernel<BC_REFLECT>, grid, block, 0, s, g, x, dl, lambda, t, m, bc, chunk, i_lo, i_hi);
        break;
    case BC_WRAP:
        hipLaunchKernelGGL(nl_trial_kernel<BC_WRAP>, grid, block, 0, s, g, x, dl, lambda, t, m, bc, chunk, i_lo, i_hi);
        break;
    default:
        hipLaunchKernelGGL(nl_trial_kernel<BC_PLAIN>, grid, block, 0, s, g, x, dl, lambda, t, m, bc, chunk, i_lo, i_hi);
    }
    return 0;
}

/* GetL2NormOfVector (mg_3d.h:783-792) over every point of a level, boundary included */
__global__ void __launch_bounds__(256) sumsq_kernel(Geom g, const double *__restrict__ a,
                                                    double *__restrict__ partials)
{
    __shared__ double lds4[4];
    double acc = 0.;
    const long long rows = (long long)g.ni * g.nj;
    for (long long row = blockIdx.x * 4 + threadIdx.y; row < rows; row += (long long)gridDim.x * 4) {
        const double *r = a + (row / g.nj) * g.plane + (row % g.nj) * g.pitch;
        for (int k = threadIdx.x; k < g.nk; k += 64)
            acc += r[k] * r[k];
    }
    const double tot = block_sum_256(acc, lds4);
    if (threadIdx.x == 0 && threadIdx.y == 0)
        partials[blockIdx.x] = tot;
}

void k_sumsq(const Geom &g, const double *a, double *partials, double *sumsq_out, hipStream_t s)
{
    long long rows = (long long)g.ni * g.nj;
    int nb = (int)((rows + 3) / 4);
    if (nb > 2048)
        nb = 2048;
    hipLaunchKernelGGL(sumsq_kernel, dim3(nb), dim3(64, 4, 1), 0, s, g, a, partials);
    hipLaunchKernelGGL(fold_partials_kernel, dim3(1), dim3(256), 0, s, partials, nb, sumsq_out);
}

/* ------------------------------------------------------- the zero map of a right-hand side
 * Bit i of map (32 planes a word) is set when every INTERIOR point of plane i of d -- 1 <= j <= nj-2, 1 <= k <= nk-2 -- has
 * the bit pattern of +0.0.  The 64-bit patterns are ORed, not compared as numbers: -0.0, a denormal and a NaN all make a
 * plane non-zero.  The faces and the row padding are not looked at; planes 0 and ni-1 never get their bit.  One block per
 * interior plane, one pass over d in 16-byte loads (rows are 128-byte aligned, pairs start on even k), one atomicOr per
 * plane that is zero. */
__global__ void __launch_bounds__(1024) dzero_scan_kernel(Geom g, const double *__restrict__ d, unsigned *__restrict__ map)
{
    __shared__ unsigned long long lds16[16];
    const int i = blockIdx.x + 1;
    const unsigned long long *p = reinterpret_cast<const unsigned long long *>(d) + g.plane * i;
    unsigned long long acc = 0ull;
    for (int j = 1 + threadIdx.y; j <= g.nj - 2; j += 16) {
        const ulonglong2 *row = reinterpret_cast<const ulonglong2 *>(p + (long long)g.pitch * j);
        for (int k = 2 * threadIdx.x; k <= g.nk - 2; k += 128) {
            const ulonglong2 v = row[k >> 1];
            acc |= (k >= 1 ? v.x : 0ull) | (k + 1 <= g.nk - 2 ? v.y : 0ull);
        }
    }
    for (int off = 32; off > 0; off >>= 1)
        acc |= __shfl_down(acc, off, 64);
    if (threadIdx.x == 0)
        lds16[threadIdx.y] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        unsigned long long all = 0ull;
        for (int w = 0; w < 16; w++)
            all |= lds16[w];
        if (all == 0ull)
            atomicOr(map + (i >> 5), 1u << (i & 31));
    }
}

/* every interior plane's bit: what the scan makes of a d that was just zeroed */
__global__ void __launch_bounds__(64) dzero_fill_kernel(int ni, unsigned *__restrict__ map)
{
    const int w = blockIdx.x * 64 + threadIdx.x;
    if (w >= mg3d_dzero_words(ni))
        return;
    unsigned v = 0u;
    for (int b = 0; b < 32; b++) {
        const int i = 32 * w + b;
        v |= (i >= 1 && i <= ni - 2) ? 1u << b : 0u;
    }
    map[w] = v;
}

void k_dzero_scan(const Geom &g, const double *d, unsigned *map, hipStream_t s)
{
    (void)hipMemsetAsync(map, 0, mg3d_dzero_words(g.ni) * sizeof(unsigned), s);
    if (g.ni >= 3 && g.nj >= 3 && g.nk >= 3)
        hipLaunchKernelGGL(dzero_scan_kernel, dim3(g.ni - 2), dim3(64, 16, 1), 0, s, g, d, map);
}

void k_dzero_fill(const Geom &g, unsigned *map, hipStream_t s)
{
    hipLaunchKernelGGL(dzero_fill_kernel, dim3((mg3d_dzero_words(g.ni) + 63) / 64), dim3(64), 0, s, g.ni, map);
}

/* --------------------------------------------------------------- restriction
 * restrictResidual, mg_3d.h:844-998.  Coarse Dirichlet faces: injection d_c = r(2i,2j,2k) (:879-958).  Every other coarse
 * point: val = 0; val += r(2i-1+ti, 2j-1+tj, 2k-1+tk) * w[ti][tj][tk] for ti, tj, tk = 0..2 in that nesting (:973-989),
 * w = (1/4,1/2,1/4)^3.  One thread per coarse point.
 *   BC_PLAIN: the i-slabs' form.  "Face" in i means a PHYSICAL boundary plane (global index 0 or Nc-1); the fine plane of
 *     coarse local plane ic is 2*(gc.ig0+ic) - gf.ig0; [ic_lo, ic_hi) are the local coarse planes produced.
 *   otherwise (periodic axes, Neumann faces; one instantiation serves both; single-domain levels, every plane): a face
 *     point is injected only where its face is a Dirichlet face; periodic and Neumann face points take the full
 *     weighting, whose -1 / +1 taps are the neighbours the stencil has at the fine point (2i, 2j, 2k) -- nb_lo / nb_hi:
 *     fine index -1 wrapped to Nf-2 on a periodic axis (2I+1 <= Nf-2 never wraps) and reflected to 1 at a Neumann low
 *     face, fine index Nf reflected to Nf-2 at a Neumann high face.  A duplicate is written as a copy by the thread of
 *     its source.
 *   With the fine level's fixed-point bytes (the pack M, one trailing argument; mg3d_fmg_solve's restriction of d) a weighted
 *     tap at a fixed point counts as 0. whatever r holds there, NaN included: the bits of restricting a copy with zeros
 *     stored at the fixed unknowns.  Every weighted tap is an unknown (never a Dirichlet face point or a duplicate), so the
 *     raw byte decides; an injected face point is no unknown and is copied as ever.  The instantiations without the
 *     pack have neither the argument nor the test. */
template <int BC, class... M>
__global__ void __launch_bounds__(256) restrict_kernel(Geom gf, const double *__restrict__ r, Geom gc,
                                                       double *__restrict__ dc, int bc, int ic_lo, int ic_hi, M... fixed)
{
    const bool pi = BC && (bc & 1), pj = BC && (bc & 2), pk = BC && (bc & 4);
    const bool ril = BC && bc_ref_lo(bc, 0), rih = BC && bc_ref_hi(bc, 0), rjl = BC && bc_ref_lo(bc, 1),
               rjh = BC && bc_ref_hi(bc, 1), rkl = BC && bc_ref_lo(bc, 2), rkh = BC && bc_ref_hi(bc, 2);
    const int kc = blockIdx.x * WAVE + threadIdx.x;
    const int jc = blockIdx.y * 4 + threadIdx.y;
    const int ic = ic_lo + blockIdx.z;
    const int nj = BC ? gc.N : gc.nj, nk = BC ? gc.N : gc.nk;
    if (kc >= nk || jc >= nj || ic >= ic_hi)
        return;
    const int icg = (BC ? 0 : gc.ig0) + ic;
    if ((pi && icg == gc.N - 1) || (pj && jc == nj - 1) || (pk && kc == nk - 1))
        return; /* a duplicate: its source's thread writes it */
    const int fi = 2 * icg - (BC ? 0 : gf.ig0), fj = 2 * jc, fk = 2 * kc;
    const long long pf = gidx(gf, fi, fj, fk);
    const bool face = (!pi && ((icg == 0 && !ril) || (icg == gc.N - 1 && !rih))) ||
                      (!pj && ((jc == 0 && !rjl) || (jc == nj - 1 && !rjh))) ||
                      (!pk && ((kc == 0 && !rkl) || (kc == nk - 1 && !rkh)));
    double val;
    if (face) {
        val = r[pf];
    } else {
        /* (BC_PLAIN: the constant offsets -plane, +plane, -pitch, +pitch, -1, +1) */
        const long long oi[3] = {nb_lo(fi, gf.N, pi, ril, gf.plane), 0, nb_hi(fi, gf.N, pi, rih, gf.plane)};
        const long long oj[3] = {nb_lo(fj, gf.N, pj, rjl, gf.pitch), 0, nb_hi(fj, gf.N, pj, rjh, gf.pitch)};
        const long long ok[3] = {nb_lo(fk, gf.N, pk, rkl, 1), 0, nb_hi(fk, gf.N, pk, rkh, 1)};
        val = 0.;
#pragma unroll
        for (int ti = 0; ti < 3; ti++)
#pragma unroll
            for (int tj = 0; tj < 3; tj++)
#pragma unroll
                for (int tk = 0; tk < 3; tk++) {
                    const double w = (ti != 1 ? 0.25 : 0.5) * (tj != 1 ? 0.25 : 0.5) * (tk != 1 ? 0.25 : 0.5);
                    const long long q = pf + oi[ti] + oj[tj] + ok[tk];
                    val += (mask_fixed(q, fixed...) ? 0. : r[q]) * w;
                }
    }
    store_dup(gc, dc, gidx(gc, ic, jc, kc), val, pi && icg == 0, pj && jc == 0, pk && kc == 0);
}

/* injection on the six coarse faces only (mg_3d.h:879-958): one thread per face point.
 * blockIdx.z = face: 0/1 the physical i-faces, 2/3 the j-faces, 4/5 the k-faces */
__global__ void __launch_bounds__(256) restrict_faces_kernel(Geom gf, const double *__restrict__ r, Geom gc,
                                                             double *__restrict__ dc, int ic_lo, int ic_hi)
{
    const int b = blockIdx.x * 64 + threadIdx.x, a = blockIdx.y * 4 + threadIdx.y, f = blockIdx.z;
    int ic, jc, kc;
    if (f < 2) {
        const int icg = f == 0 ? 0 : gc.N - 1;
        ic = icg - gc.ig0;
        jc = a;
        kc = b;
        if (ic < ic_lo || ic >= ic_hi || jc >= gc.nj || kc >= gc.nk)
            return;
    } else if (f < 4) {
        ic = ic_lo + a;
        jc = f == 2 ? 0 : gc.nj - 1;
        kc = b;
        if (ic >= ic_hi || kc >= gc.nk)
            return;
    } else {
        ic = ic_lo + a;
        jc = b;
        kc = f == 4 ? 0 : gc.nk - 1;
        if (ic >= ic_hi || jc >= gc.nj)
            return;
    }
    const int fi = 2 * (gc.ig0 + ic) - gf.ig0;
    dc[gidx(gc, ic, jc, kc)] = r[gidx(gf, fi, 2 * jc, 2 * kc)];
}

void k_restrict(const Geom &gf, const double *r, const Geom &gc, double *dc, int bc, hipStream_t s, int ic_lo, int ic_hi,
                bool faces_only, const unsigned char *mf)
{
    const dim3 block(WAVE, 4, 1);
    if (mf) { /* a single-domain level, any boundary word (0 too: the Dirichlet faces' injection and plain offsets) */
        const dim3 grid((gc.N + WAVE - 1) / WAVE, (gc.N + 3) / 4, gc.N);
        hipLaunchKernelGGL((restrict_kernel<BC_WRAP, MaskPtr>), grid, block, 0, s, gf, r, gc, dc, bc, 0, gc.N, mf);
        return;
    }
    if (bc) { /* a single-domain level: every plane, never faces only -- periodic and Neumann faces are fully weighted */
        const dim3 grid((gc.N + WAVE - 1) / WAVE, (gc.N + 3) / 4, gc.N);
        hipLaunchKernelGGL(restrict_kernel<BC_WRAP>, grid, block, 0, s, gf, r, gc, dc, bc, 0, gc.N);
        return;
    }
    /* local coarse planes written: physical boundary planes and owned planes; a
     * halo plane (local 0 / ni-1 that is not a physical boundary) is the neighbour's */
    const int lo = ic_lo >= 0 ? ic_lo : ((gc.ig0 == 0) ? 0 : 1);
    const int hi = ic_hi >= 0 ? ic_hi : ((gc.ig0 + gc.ni == gc.N) ? gc.ni : gc.ni - 1);
    if (hi <= lo)
        return;
    if (faces_only) {
        const int m = max(max(gc.nj, gc.nk), hi - lo);
        const dim3 grid((m + 63) / 64, (m + 3) / 4, 6);
        hipLaunchKernelGGL(restrict_faces_kernel, grid, block, 0, s, gf, r, gc, dc, lo, hi);
        return;
    }
    const dim3 grid((gc.nk + 63) / 64, (gc.nj + 3) / 4, hi - lo);
    hipLaunchKernelGGL(restrict_kernel<BC_PLAIN>, grid, block, 0, s, gf, r, gc, dc, 0, lo, hi);
}

/* eps of the coarse level at every point, boundary included: ec[I,J,K] = ef[2I,2J,2K] (single-domain levels) */
template <class T>
__global__ void __launch_bounds__(256) coef_inject_kernel(Geom gf, const T *__restrict__ ef, Geom gc, T *__restrict__ ec)
{
    const int kc = blockIdx.x * WAVE + threadIdx.x;
    const int jc = blockIdx.y * 4 + threadIdx.y;
    const int ic = blockIdx.z;
    if (kc >= gc.nk || jc >= gc.nj)
        return;
    ec[gidx(gc, ic, jc, kc)] = ef[gidx(gf, 2 * ic, 2 * jc, 2 * kc)];
}

void k_coef_inject(const Geom &gf, const double *ef, const Geom &gc, double *ec, hipStream_t s)
{
    dim3 grid((gc.nk + WAVE - 1) / WAVE, (gc.nj + 3) / 4, gc.ni);
    hipLaunchKernelGGL(coef_inject_kernel<double>, grid, dim3(WAVE, 4, 1), 0, s, gf, ef, gc, ec);
}

/* the fixed-point bytes of the coarse level the same way: mc[I,J,K] = mf[2I,2J,2K] */
void k_mask_inject(const Geom &gf, const unsigned char *mf, const Geom &gc, unsigned char *mc, hipStream_t s)
{
    dim3 grid((gc.nk + WAVE - 1) / WAVE, (gc.nj + 3) / 4, gc.ni);
    hipLaunchKernelGGL(coef_inject_kernel<unsigned char>, grid, dim3(WAVE, 4, 1), 0, s, gf, mf, gc, mc);
}

/* MG3D_MASK_KEEP (include/mg3d.h): the coarse point C = (I, J, K) whose own fine point 2C is not fixed stands for the first
 * LOST fine point among F = 2C + (a, b, c), (a, b, c) = (0,0,1), (0,1,0), (0,1,1), (1,0,0) ... (1,1,1): one with a nonzero
 * byte none of whose parents C + (a*al, b*be, c*ga), al, be, ga in {0, 1}, has a nonzero byte at its own fine point.  Raw
 * bytes of the fine level, its duplicates holding their sources'; an F past index N-1 is skipped, and then every parent
 * lies inside: 2I + 1 <= N-1 gives 2(I + 1) <= N-1.  At most 15 bytes read.  Returns the offset of that F, or -1 */
__device__ __forceinline__ long long keep_lost(const Geom &gf, const unsigned char *__restrict__ mf, int I, int J, int K)
{
    const int N = gf.N;
    const long long p0 = gidx(gf, 2 * I, 2 * J, 2 * K);
    for (int t = 1; t < 8; t++) {
        const int a = t >> 2, b = (t >> 1) & 1, c = t & 1;
        if (2 * I + a > N - 1 || 2 * J + b > N - 1 || 2 * K + c > N - 1)
            continue;
        const long long pF = p0 + a * gf.plane + b * (long long)gf.pitch + c;
        if (!mf[pF])
            continue;
        bool lost = true;
        for (int q = 0; q < 8; q++)
            if (!(q & ~t)) /* the parents: the subsets of (a, b, c) */
                lost = lost && mf[p0 + 2 * ((q >> 2) * gf.plane + ((q >> 1) & 1) * (long long)gf.pitch + (q & 1))] == 0;
        if (lost)
            return pF;
    }
    return -1;
}

/* one thread per coarse point, set-up time only; the caller refreshes the coarse duplicates behind it (k_mask_refresh) */
__global__ void __launch_bounds__(256) mask_keep_kernel(Geom gf, const unsigned char *__restrict__ mf, Geom gc,
                                                        unsigned char *__restrict__ mc)
{
    const int kc = blockIdx.x * WAVE + threadIdx.x;
    const int jc = blockIdx.y * 4 + threadIdx.y;
    const int ic = blockIdx.z;
    if (kc >= gc.N || jc >= gc.N)
        return;
    unsigned char b = mf[gidx(gf, 2 * ic, 2 * jc, 2 * kc)];
    if (!b) {
        const long long p = keep_lost(gf, mf, ic, jc, kc);
        if (p >= 0)
            b = mf[p];
    }
    mc[gidx(gc, ic, jc, kc)] = b;
}

void k_mask_keep(const Geom &gf, const unsigned char *mf, const Geom &gc, unsigned char *mc, hipStream_t s)
{
    assert(gf.N == 2 * gc.N - 1); /* (every hierarchy meets it, as for k_prolong: operator state is never left unwritten) */
    dim3 grid((gc.N + WAVE - 1) / WAVE, (gc.N + 3) / 4, gc.N);
    hipLaunchKernelGGL(mask_keep_kernel, grid, dim3(WAVE, 4, 1), 0, s, gf, mf, gc, mc);
}

/* u of the coarse level for mg3d_fmg_solve under MG3D_MASK_KEEP: the injection uc[C] = uf[2C], except that a fixed unknown
 * of the coarse level whose own fine point is not fixed -- it stands for a lost fine point -- takes u of that fine point,
 * the conductor's potential.  A periodic duplicate asks at its source, so it holds its source's value. */
__global__ void __launch_bounds__(256) fmg_inject_kernel(Geom gf, const double *__restrict__ uf,
                                                         const unsigned char *__restrict__ mf, Geom gc,
                                                         double *__restrict__ uc, int bc)
{
    const int k = blockIdx.x * WAVE + threadIdx.x;
    const int j = blockIdx.y * 4 + threadIdx.y;
    const int i = blockIdx.z;
    const int N = gc.N;
    if (k >= N || j >= N)
        return;
    const int si = ((bc & 1) && i == N - 1) ? 0 : i, sj = ((bc & 2) && j == N - 1) ? 0 : j, sk = ((bc & 4) && k == N - 1) ? 0 : k;
    long long q = gidx(gf, 2 * i, 2 * j, 2 * k);
    if (bc_unknown(bc, N, si, sj, sk) && !mf[gidx(gf, 2 * si, 2 * sj, 2 * sk)]) {
        const long long p = keep_lost(gf, mf, si, sj, sk);
        if (p >= 0)
            q = p;
    }
    uc[gidx(gc, i, j, k)] = uf[q];
}

void k_fmg_inject(const Geom &gf, const double *uf, const unsigned char *mf, const Geom &gc, double *uc, int bc, hipStream_t s)
{
    assert(gf.N == 2 * gc.N - 1);
    dim3 grid((gc.N + WAVE - 1) / WAVE, (gc.N + 3) / 4, gc.N);
    hipLaunchKernelGGL(fmg_inject_kernel, grid, dim3(WAVE, 4, 1), 0, s, gf, uf, mf, gc, uc, bc);
}

/* -------------------------------------------------------------- prolongation
 * prolongateAndCorrectError, mg_3d.h:1000-1145: ef[p] += P(ec) at EVERY fine point.
 * Parent order per parity class (o = odd flags of i,j,k; l = low coarse index):
 *   o=(1,1,1): ((((((c000+c001)+c010)+c011)+c100)+c101)+c110)+c111, *0.125   (:1028-1048)
 *   i even   : ((c(jl,kl)+c(jl+1,kl))+c(jl,kl+1))+c(jl+1,kl+1),       *0.25    (:1064-1067)
 *   j even   : ((c(il,kl)+c(il+1,kl))+c(il,kl+1))+c(il+1,kl+1),       *0.25    (:1075-1078)
 *   k even   : ((c(il,jl)+c(il,jl+1))+c(il+1,jl))+c(il+1,jl+1),       *0.25    (:1085-1088)
 *   one odd  : (low + high) * 0.5                                               (:1110-1133)
 *   none odd : copy                                                             (:1138)
 * The running sum starts from 0. (0. + x == x), as retVal does. */
/* Cell-based form, the Dirichlet levels' (the V-cycle, the i-slabs): a thread owns one coarse cell (jc, m) -- the 2 x 2
 * fine points (2jc, 2jc+1) x (2m, 2m+1) of every fine plane -- and marches along i.  The eight coarse corners
 * E[a][b][c] = ec(il+a, jc+b, m+c) of the current cell stay in registers and are reused by the two fine
 * planes that share them; fine data moves as 16-byte k-pairs.  The parent order above. */
__global__ void __launch_bounds__(256) prolong_cell_kernel(Geom gc, const double *__restrict__ ec, Geom gf,
                                                           double *__restrict__ ef, int if_lo, int if_hi, int chunk)
{
    const int m = blockIdx.x * 64 + threadIdx.x;
    const int jc = blockIdx.y * 4 + threadIdx.y;
    const int k0 = 2 * m, j0 = 2 * jc;
    if (k0 >= gf.nk || j0 >= gf.nj)
        return;
    const int i_beg = if_lo + blockIdx.z * chunk;
    const int i_end = min(if_hi, i_beg + chunk);
    const bool row1 = j0 + 1 < gf.nj;
    const int m1 = min(m + 1, gc.nk - 1), jc1 = min(jc + 1, gc.nj - 1);
    const long long c00 = (long long)gc.pitch * jc + m, c01 = (long long)gc.pitch * jc + m1;
    const long long c10 = (long long)gc.pitch * jc1 + m, c11 = (long long)gc.pitch * jc1 + m1;
    double E0[2][2], E1[2][2]; /* coarse planes `have` and `have + 1`, [b][c] */
    int have = -0x40000000;
    auto load = [&](int il, double(&E)[2][2]) {
        const double *pl = ec + gc.plane * min(max(il, 0), gc.ni - 1);
        E[0][0] = pl[c00];
        E[0][1] = pl[c01];
        E[1][0] = pl[c10];
        E[1][1] = pl[c11];
    };
    for (int i = i_beg; i < i_end; i++) {
        const int ig = gf.ig0 + i, oi = ig & 1;
        const int il = (ig - oi) / 2 - gc.ig0;
        if (have != il) {
            if (have + 1 == il) {
                E0[0][0] = E1[0][0];
                E0[0][1] = E1[0][1];
                E0[1][0] = E1[1][0];
                E0[1][1] = E1[1][1];
            } else {
                load(il, E0);
            }
            load(il + 1, E1);
            have = il;
        }
        double t00, t01, t10, t11; /* [row parity][col parity] */
        if (!oi) {
            t00 = E0[0][0];
            t01 = (E0[0][0] + E0[0][1]) * 0.5;
            t10 = (E0[0][0] + E0[1][0]) * 0.5;
            t11 = (((E0[0][0] + E0[1][0]) + E0[0][1]) + E0[1][1]) * 0.25; /* i even: (jl,kl)(jl+1,kl)(jl,kl+1)(jl+1,kl+1) */
        } else {
            t00 = (E0[0][0] + E1[0][0]) * 0.5;
            t01 = (((E0[0][0] + E1[0][0]) + E0[0][1]) + E1[0][1]) * 0.25; /* j even: (il,kl)(il+1,kl)(il,kl+1)(il+1,kl+1) */
            t10 = (((E0[0][0] + E0[1][0]) + E1[0][0]) + E1[1][0]) * 0.25; /* k even: (il,jl)(il,jl+1)(il+1,jl)(il+1,jl+1) */
            double t = E0[0][0] + E0[0][1];
            t = t + E0[1][0];
            t = t + E0[1][1];
            t = t + E1[0][0];
            t = t + E1[0][1];
            t = t + E1[1][0];
            t = t + E1[1][1];
            t11 = t * 0.125;
        }
        double *row = ef + gf.plane * i + (long long)gf.pitch * j0 + k0;
        double2 a = *reinterpret_cast<double2 *>(row);
        a.x += t00;
        a.y += t01;
        *reinterpret_cast<double2 *>(row) = a;
        if (row1) {
            double2 b = *reinterpret_cast<double2 *>(row + gf.pitch);
            b.x += t10;
            b.y += t11;
            *reinterpret_cast<double2 *>(row + gf.pitch) = b;
        }
    }
}

/* Point form, one thread per fine point, for the levels with periodic axes, Neumann faces or fixed points: ef += P(ec) at every fine
 * point that is not a duplicate (Dirichlet faces included: their coarse parents hold zeros), in the parent order above;
 * on a periodic axis the high parent il+1 = Nc-1 is read at its source 0.  The thread of a point writes the sum to its
 * duplicates too, so neither a fine nor a coarse duplicate is ever read.  A Neumann face needs nothing of its own: every
 * parent of a fine face point lies on the same face, and this kernel corrects the face points with the rest (axes: the
 * periodic bits of the boundary word).  With fixed points (the pack M: the fine level's bytes and the boundary word, two
 * trailing arguments) a fine fixed UNKNOWN is skipped -- a byte on a Dirichlet face is ignored, the face point is corrected
 * as ever.  A Dirichlet level takes this form only when it has fixed points: k_prolong. */
__device__ __forceinline__ bool prolong_fixed(const Geom &g, int i, int j, int k, const unsigned char *m, int bc)
{
    return bc_unknown(bc, g.N, i, j, k) && m[gidx(g, i, j, k)] != 0;
}
template <class... M>
__global__ void __launch_bounds__(256) prolong_kernel(Geom gc, const double *__restrict__ ec, Geom gf,
                                                      double *__restrict__ ef, int axes, M... fixed)
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
    if constexpr (sizeof...(M) != 0)
        if (prolong_fixed(gf, i, j, k, fixed...))
            return;
    const int oi = i & 1, oj = j & 1, ok = k & 1;
    const int il = (i - oi) / 2, jl = (j - oj) / 2, kl = (k - ok) / 2;
    const long long c0 = gidx(gc, il, jl, kl);
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
    const long long p = gidx(gf, i, j, k);
    store_dup(gf, ef, p, ef[p] + t, pi && i == 0, pj && j == 0, pk && k == 0);
}

/* bc = 0 without fixed points: the cell form.  Its one condition, which every hierarchy meets -- a level keeps nj = nk = N
 * and Nf = 2*Nc - 1 -- is asserted: a Dirichlet level without a mask has no other form.  A boundary word or fixed points
 * (mf) select the point form */
void k_prolong(const Geom &gc, const double *ec, const Geom &gf, double *ef, int bc, hipStream_t s, int if_lo, int if_hi,
               const unsigned char *mf)
{
    if (bc || mf) { /* a single-domain level: every plane */
        const dim3 grid((gf.N + WAVE - 1) / WAVE, (gf.N + 3) / 4, gf.N);
        if (mf)
            hipLaunchKernelGGL((prolong_kernel<MaskPtr, int>), grid, dim3(WAVE, 4, 1), 0, s, gc, ec, gf, ef, bc & 7, mf, bc);
        else
            hipLaunchKernelGGL(prolong_kernel<>, grid, dim3(WAVE, 4, 1), 0, s, gc, ec, gf, ef, bc & 7);
        return;
    }
    assert(gf.nk == 2 * gc.nk - 1 && gf.nj == 2 * gc.nj - 1);
    const int lo = if_lo >= 0 ? if_lo : ((gf.ig0 == 0) ? 0 : 1);
    const int hi = if_hi >= 0 ? if_hi : ((gf.ig0 + gf.ni == gf.N) ? gf.ni : gf.ni - 1);
    if (hi <= lo)
        return;
    const int gx = ((gf.nk + 1) / 2 + 63) / 64, gy = ((gf.nj + 1) / 2 + 3) / 4;
    int chunk = 64; /* a few hundred to a few thousand blocks, like the sweep */
    while (chunk > 4 && (long long)gx * gy * ((hi - lo + chunk - 1) / chunk) < 2048)
        chunk /= 2;
    const dim3 grid(gx, gy, (hi - lo + chunk - 1) / chunk);
    hipLaunchKernelGGL(prolong_cell_kernel, grid, dim3(64, 4, 1), 0, s, gc, ec, gf, ef, lo, hi, chunk);
}

/* --------------------------------------------------------- FMG interpolation
 * mg3d_fmg_interpolate / mg3d_fmg_solve: every unknown of the fine level is OVERWRITTEN with the tensor-product cubic
 * interpolant of the coarse u (nothing is added; Dirichlet points are never written; periodic duplicates as store_dup).
 * Per axis, coarse side Nc, fine index x:
 *   x = 2I              one term: coarse I, weight 1
 *   x = 2I+1, Nc >= 4   four terms over coarse I-1, I, I+1, I+2 with -1/16, 9/16, 9/16, -1/16; an index outside the unique
 *                       range wraps modulo Nc-1 on a periodic axis and reflects at a Neumann face (-1 -> 1, Nc -> Nc-2);
 *                       next to a Dirichlet face the one-sided cubic over the four points nearest that face: low side
 *                       (x = 1) coarse 0, 1, 2, 3 with 5/16, 15/16, -5/16, 1/16, high side (x = Nf-2) coarse Nc-4 .. Nc-1
 *                       with 1/16, -5/16, 15/16, 5/16
 *   x = 2I+1, Nc < 4    two terms: coarse I, I+1 with 1/2, 1/2
 * value = sum_a wi[a] * (sum_b wj[b] * (sum_c wk[c] * uc[i_a, j_b, k_c])), every sum left to right in the order listed
 * (the first term starts the sum), no contraction; all weights are binary fractions.  tests/_fmg_ref.py states the same in
 * numpy.
 *
 * A term list is held as window slots: slot s stands for the logical coarse index I-1+s, which fmg_phys maps to the point
 * that is read (wrapped, reflected; at a Dirichlet face -1 maps to 3 and Nc to Nc-4, the fourth point of the one-sided
 * form, so the four slots always hold the four points of every form and only their order differs).
 *
 * A block produces the fine tile 8 rows x 64 columns (rows and columns counted from 0: 512-byte aligned row stores) of
 * the fine planes 2I, 2I+1 of a chunk of coarse planes I, marching along i.  Per coarse plane: the k pass from global
 * memory (seven coarse rows x 64 fine columns, into LDS), one barrier, the j pass from LDS into registers; a thread owns
 * two (row, column) pairs and keeps their j-passed values of the four coarse planes of the i window in registers. */
enum { FMG_EVEN = 0, FMG_LIN, FMG_CEN, FMG_LOW, FMG_HIGH };

struct FmgAxis {
    int Nc;
    bool per, rlo, rhi;
};

__device__ __forceinline__ FmgAxis fmg_axis(int Nc, int bc, int ax)
{
    return FmgAxis{Nc, (bc >> ax & 1) != 0, bc_ref_lo(bc, ax), bc_ref_hi(bc, ax)};
}

/* the coarse point read for logical index l (-1 .. Nc+1; what no form uses is clamped into the array) */
__device__ __forceinline__ int fmg_phys(const FmgAxis &a, int l)
{
    int p;
    if (a.per)
        p = l < 0 ? l + a.Nc - 1 : (l >= a.Nc - 1 ? l - (a.Nc - 1) : l);
    else if (l < 0)
        p = a.rlo ? 1 : 3;
    else if (l >= a.Nc)
        p = a.rhi ? a.Nc - 2 : a.Nc - 4;
    else
        p = l;
    return min(max(p, 0), a.Nc - 1);
}

/* the form of fine index x = 2I + odd */
__device__ __forceinline__ int fmg_form(const FmgAxis &a, int I, int odd)
{
    if (!odd)
        return FMG_EVEN;
    if (a.Nc < 4)
        return FMG_LIN;
    if (!a.per && !a.rlo && I == 0)
        return FMG_LOW;
    if (!a.per && !a.rhi && I + 2 == a.Nc)
        return FMG_HIGH;
    return FMG_CEN;
}

/* a form as n terms in summation order: window slots s and weights w (unused entries: slot 1, weight 0) */
struct FmgTaps {
    int n, s[4];
    double w[4];
};

__device__ __forceinline__ FmgTaps fmg_taps(int form)
{
    switch (form) {
    case FMG_EVEN:
        return FmgTaps{1, {1, 1, 1, 1}, {1., 0., 0., 0.}};
    case FMG_LIN:
        return FmgTaps{2, {1, 2, 1, 1}, {0.5, 0.5, 0., 0.}};
    case FMG_LOW:
        return FmgTaps{4, {1, 2, 3, 0}, {0.3125, 0.9375, -0.3125, 0.0625}};
    case FMG_HIGH:
        return FmgTaps{4, {3, 0, 1, 2}, {0.0625, -0.3125, 0.9375, 0.3125}};
    default:
        return FmgTaps{4, {0, 1, 2, 3}, {-0.0625, 0.5625, 0.5625, -0.0625}};
    }
}

/* the sum of a form over its terms x0 .. x3 (already in summation order) */
__device__ __forceinline__ double fmg_sum(const FmgTaps &t, double x0, double x1, double x2, double x3)
{
    double acc = t.w[0] * x0;
    const double a2 = acc + t.w[1] * x1;
    const double a4 = (a2 + t.w[2] * x2) + t.w[3] * x3;
    return t.n == 1 ? acc : (t.n == 2 ? a2 : a4);
}

#define FMG_TJ 8  /* fine rows of a tile */
#define FMG_CJ 7  /* coarse rows its j pass reads: logical Jc0-1 .. Jc0+5 */

/* With fixed points (the pack M: the fine level's bytes, one trailing argument) a fixed unknown of the fine level is not
 * written; every store goes to an unknown, so the raw byte decides.  Without the pack: the kernel as it was */
template <int BC, class... M>
__global__ void __launch_bounds__(256) fmg_interp_kernel(Geom gc, const double *__restrict__ uc, Geom gf,
                                                         double *__restrict__ uf, int bc, int chunk, M... fixed)
{
    __shared__ double T1[2][FMG_CJ][WAVE];
    const int Nc = gc.N, Nf = gf.N;
    const int cbc = BC ? bc : 0;
    const FmgAxis ai = fmg_axis(Nc, cbc, 0), aj = fmg_axis(Nc, cbc, 1), ak = fmg_axis(Nc, cbc, 2);
    const int tx = threadIdx.x, ty = threadIdx.y;
    /* unknown ranges of the fine level (column<BC> / stencil_window) */
    const int ilo = (ai.per || ai.rlo) ? 0 : 1, ihi = Nf - (ai.rhi ? 1 : 2);
    const int jlo = (aj.per || aj.rlo) ? 0 : 1, jhi = Nf - (aj.rhi ? 1 : 2);
    const int klo = (ak.per || ak.rlo) ? 0 : 1, khi = Nf - (ak.rhi ? 1 : 2);
    /* k pass: this thread's fine column and the coarse columns of its terms */
    const int k = blockIdx.x * WAVE + tx;
    const int kx = min(k, Nf - 1);
    const FmgTaps tk = fmg_taps(fmg_form(ak, kx >> 1, kx & 1));
    int kc[4];
#pragma unroll
    for (int t = 0; t < 4; t++)
        kc[t] = fmg_phys(ak, (kx >> 1) - 1 + tk.s[t]);
    /* ... and its (up to) two coarse rows: tile rows ty and ty + 4 */
    const int Jc0 = blockIdx.y * (FMG_TJ / 2);
    const long long rowa = (long long)gc.pitch * fmg_phys(aj, Jc0 - 1 + ty);
    const long long rowb = (long long)gc.pitch * fmg_phys(aj, Jc0 - 1 + min(ty + 4, FMG_CJ - 1));
    const bool has_b = ty + 4 < FMG_CJ;
    /* j pass: this thread's two fine rows ty and ty + 4 of the tile, column tx */
    int j[2], r[2][4];
    FmgTaps tj[2];
    bool ok[2];
#pragma unroll
    for (int m = 0; m < 2; m++) {
        j[m] = blockIdx.y * FMG_TJ + ty + 4 * m;
        const int jx = min(j[m], Nf - 1);
        tj[m] = fmg_taps(fmg_form(aj, jx >> 1, jx & 1));
#pragma unroll
        for (int t = 0; t < 4; t++)
            r[m][t] = min((jx >> 1) - Jc0 + tj[m].s[t], FMG_CJ - 1);
        ok[m] = j[m] >= jlo && j[m] <= jhi && k >= klo && k <= khi;
    }
    const bool dk = ak.per && k == 0;

    /* the j-passed values of this thread's two points on coarse plane `l` (logical); every thread of the block calls it */
    int step = 0;
    auto plane = [&](int l, double &o0, double &o1) {
        const double *pl = uc + gc.plane * fmg_phys(ai, l);
        double(*T)[WAVE] = T1[step & 1];
        step++;
        T[ty][tx] = fmg_sum(tk, pl[rowa + kc[0]], pl[rowa + kc[1]], pl[rowa + kc[2]], pl[rowa + kc[3]]);
        if (has_b)
            T[ty + 4][tx] = fmg_sum(tk, pl[rowb + kc[0]], pl[rowb + kc[1]], pl[rowb + kc[2]], pl[rowb + kc[3]]);
        __syncthreads(); /* two buffers: the readers of this one are two barriers ahead of its next writers */
        o0 = fmg_sum(tj[0], T[r[0][0]][tx], T[r[0][1]][tx], T[r[0][2]][tx], T[r[0][3]][tx]);
        o1 = fmg_sum(tj[1], T[r[1][0]][tx], T[r[1][1]][tx], T[r[1][2]][tx], T[r[1][3]][tx]);
    };
    auto store = [&](int i, int m, double x) {
        if (ok[m] && !mask_fixed(gidx(gf, i, j[m], k), fixed...))
            store_dup(gf, uf, gidx(gf, i, j[m], k), x, ai.per && i == 0, aj.per && j[m] == 0, dk);
    };

    const int I0 = blockIdx.z * chunk, I1 = min(I0 + chunk, Nc);
    double W[4][2]; /* window slots 0 .. 3 = logical coarse planes I-1 .. I+2 */
    plane(I0 - 1, W[0][0], W[0][1]);
    plane(I0, W[1][0], W[1][1]);
    plane(I0 + 1, W[2][0], W[2][1]);
    for (int I = I0; I < I1; I++) {
        plane(I + 2, W[3][0], W[3][1]);
        const int i = 2 * I;
        if (i >= ilo && i <= ihi) {
            store(i, 0, W[1][0]);
            store(i, 1, W[1][1]);
        }
        if (i + 1 <= ihi) {
            const int form = fmg_form(ai, I, 1);
            const FmgTaps ti = fmg_taps(form);
#pragma unroll
            for (int m = 0; m < 2; m++) {
                double x;
                if (form == FMG_LOW)
                    x = fmg_sum(ti, W[1][m], W[2][m], W[3][m], W[0][m]);
                else if (form == FMG_HIGH)
                    x = fmg_sum(ti, W[3][m], W[0][m], W[1][m], W[2][m]);
                else if (form == FMG_LIN)
                    x = fmg_sum(ti, W[1][m], W[2][m], W[1][m], W[1][m]);
                else
                    x = fmg_sum(ti, W[0][m], W[1][m], W[2][m], W[3][m]);
                store(i + 1, m, x);
            }
        }
#pragma unroll
        for (int m = 0; m < 2; m++) {
            W[0][m] = W[1][m];
            W[1][m] = W[2][m];
            W[2][m] = W[3][m];
        }
    }
}

void k_fmg_interp(const Geom &gc, const double *uc, const Geom &gf, double *uf, int bc, hipStream_t s, const unsigned char *mf)
{
    if (gf.N != 2 * gc.N - 1 || gc.N < 3)
        return;
    const int gx = (gf.N + WAVE - 1) / WAVE, gy = (gf.N + FMG_TJ - 1) / FMG_TJ;
    int chunk = 16; /* three coarse planes of lead-in per chunk; shorter chunks while the grid is small */
    while (chunk > 2 && (long long)gx * gy * ((gc.N + chunk - 1) / chunk) < 1024)
        chunk /= 2;
    const dim3 grid(gx, gy, (gc.N + chunk - 1) / chunk), block(WAVE, 4, 1);
    const int mode = bc_mode(bc);
    if (mf) {
        if (mode == BC_REFLECT)
            hipLaunchKernelGGL((fmg_interp_kernel<BC_REFLECT, MaskPtr>), grid, block, 0, s, gc, uc, gf, uf, bc, chunk, mf);
        else if (mode == BC_WRAP)
            hipLaunchKernelGGL((fmg_interp_kernel<BC_WRAP, MaskPtr>), grid, block, 0, s, gc, uc, gf, uf, bc, chunk, mf);
        else
            hipLaunchKernelGGL((fmg_interp_kernel<BC_PLAIN, MaskPtr>), grid, block, 0, s, gc, uc, gf, uf, bc, chunk, mf);
    } else if (mode == BC_REFLECT)
        hipLaunchKernelGGL(fmg_interp_kernel<BC_REFLECT>, grid, block, 0, s, gc, uc, gf, uf, bc, chunk);
    else if (mode == BC_WRAP)
        hipLaunchKernelGGL(fmg_interp_kernel<BC_WRAP>, grid, block, 0, s, gc, uc, gf, uf, bc, chunk);
    else
        hipLaunchKernelGGL(fmg_interp_kernel<BC_PLAIN>, grid, block, 0, s, gc, uc, gf, uf, bc, chunk);
}

/* d = u at every Dirichlet point of a (single-domain) level -- a face point of a non-periodic axis whose face is not a
 * Neumann face: the right-hand side of the identity rows of the direct solve (mg3d_fmg_solve) */
__global__ void __launch_bounds__(256) dirichlet_rhs_kernel(Geom g, const double *__restrict__ u, double *__restrict__ d,
                                                            int bc)
{
    const int k = blockIdx.x * WAVE + threadIdx.x;
    const int j = blockIdx.y * 4 + threadIdx.y;
    const int i = blockIdx.z;
    const int N = g.N;
    if (k >= N || j >= N)
        return;
    const int x[3] = {i, j, k};
    bool dir = false;
    for (int ax = 0; ax < 3; ax++)
        dir = dir || (!(bc >> ax & 1) && ((x[ax] == 0 && !bc_ref_lo(bc, ax)) || (x[ax] == N - 1 && !bc_ref_hi(bc, ax))));
    if (dir)
        d[gidx(g, i, j, k)] = u[gidx(g, i, j, k)];
}

void k_dirichlet_rhs(const Geom &g, const double *u, double *d, int bc, hipStream_t s)
{
    dim3 grid((g.N + WAVE - 1) / WAVE, (g.N + 3) / 4, g.N);
    hipLaunchKernelGGL(dirichlet_rhs_kernel, grid, dim3(WAVE, 4, 1), 0, s, g, u, d, bc);
}

/* ------------------------------------------------------------- coarsest level
 * The level-0 right-hand side of the direct solve where the coarsest matrix (mg3d_coarse_matrix_mask) has identity rows
 * inside the domain: d at every point, except 0 in the rows of the periodic duplicates and of the pinned point (0,0,0) --
 * so a duplicate's d is never read, and those rows' solution is 0 until the refresh below copies the sources over the
 * duplicates -- and, MASK, at a fixed unknown the value of its row: 0., the error a fixed point holds in a cycle (ufix NULL),
 * or u's own value there (a one-level context: the direct solve IS the solve).  MASK = false has neither argument. */
__device__ __forceinline__ bool coarse_fixed(long long, double &) { return false; }
__device__ __forceinline__ bool coarse_fixed(long long p, double &x, const unsigned char *m, const double *ufix)
{
    if (!m[p])
        return false;
    x = ufix ? ufix[p] : 0.;
    return true;
}
template <bool MASK, class... M>
__global__ void __launch_bounds__(256) coarse_rhs_kernel(Geom g, const double *__restrict__ d, double *__restrict__ b, int bc,
                                                         int pin, M... fixed)
{
    static_assert(sizeof...(M) == (MASK ? 2 : 0), "MASK: the mask and ufix are the two trailing arguments");
    const int k = blockIdx.x * WAVE + threadIdx.x;
    const int j = blockIdx.y * 4 + threadIdx.y;
    const int i = blockIdx.z;
    const int N = g.N;
    if (k >= N || j >= N)
        return;
    const int axes = bc & 7;
    const bool dup = ((axes & 1) && i == N - 1) || ((axes & 2) && j == N - 1) || ((axes & 4) && k == N - 1);
    const long long p = gidx(g, i, j, k);
    double x = 0.;
    if (!(dup || (pin && (i | j | k) == 0)) && !(MASK && bc_unknown(bc, N, i, j, k) && coarse_fixed(p, x, fixed...)))
        x = d[p];
    b[p] = x;
}

void k_coarse_rhs(const Geom &g, const double *d, double *b, int bc, int pin, const unsigned char *m, const double *ufix,
                  hipStream_t s)
{
    const dim3 grid((g.N + WAVE - 1) / WAVE, (g.N + 3) / 4, g.N), block(WAVE, 4, 1);
    if (m)
        hipLaunchKernelGGL((coarse_rhs_kernel<true, MaskPtr, const double *>), grid, block, 0, s, g, d, b, bc, pin, m, ufix);
    else
        hipLaunchKernelGGL((coarse_rhs_kernel<false>), grid, block, 0, s, g, d, b, bc, pin);
}

/* Every duplicate of a field from its source: blockIdx.z = the axis whose duplicate plane a thread covers; (a, b) the
 * other two indices.  The source maps every periodic index N-1 to 0, so only unique points are read; an edge or corner
 * duplicate is written by each plane it lies in, with the same value. */
template <class T>
__global__ void __launch_bounds__(256) per_refresh_kernel(Geom g, T *__restrict__ v, int axes,
                                                          const unsigned long long *__restrict__ gate)
{
    const int b = blockIdx.x * WAVE + threadIdx.x, a = blockIdx.y * 4 + threadIdx.y, ax = blockIdx.z;
    const int N = g.N;
    if (a >= N || b >= N || !(axes & (1 << ax)) || (gate && *gate == 0))
        return;
    int i = ax == 0 ? N - 1 : a, j = ax == 1 ? N - 1 : (ax == 0 ? a : b), k = ax == 2 ? N - 1 : b;
    const int si = (axes & 1) && i == N - 1 ? 0 : i, sj = (axes & 2) && j == N - 1 ? 0 : j,
              sk = (axes & 4) && k == N - 1 ? 0 : k;
    v[gidx(g, i, j, k)] = v[gidx(g, si, sj, sk)];
}

void k_per_refresh(const Geom &g, double *v, int bc, hipStream_t s, const unsigned long long *gate)
{
    const int axes = bc & 7;
    if (!axes)
        return;
    dim3 grid((g.N + WAVE - 1) / WAVE, (g.N + 3) / 4, 3);
    hipLaunchKernelGGL(per_refresh_kernel<double>, grid, dim3(WAVE, 4, 1), 0, s, g, v, axes, gate);
}

void k_mask_refresh(const Geom &g, unsigned char *m, int bc, hipStream_t s)
{
    const int axes = bc & 7;
    if (!axes)
        return;
    dim3 grid((g.N + WAVE - 1) / WAVE, (g.N + 3) / 4, 3);
    hipLaunchKernelGGL(per_refresh_kernel<unsigned char>, grid, dim3(WAVE, 4, 1), 0, s, g, m, axes,
                       (const unsigned long long *)nullptr);
}

/* ------------------------------------------------------------- fixed points */

/* the fixed UNKNOWNS of a level, counted: one 64-bit atomic add per block that found any.  T = double: the unknowns at
 * which a screening field is > 0 (k_field_count) */
template <class T>
__global__ void __launch_bounds__(256) mask_count_kernel(Geom g, const T *__restrict__ m, int bc,
                                                         unsigned long long *__restrict__ out)
{
    const int k = blockIdx.x * WAVE + threadIdx.x;
    const int j = blockIdx.y * 4 + threadIdx.y;
    const int i = blockIdx.z;
    const int N = g.N;
    const bool fixed = k < N && j < N && bc_unknown(bc, N, i, j, k) && m[gidx(g, i, j, k)] > (T)0;
    __shared__ unsigned int row_cnt[4];
    const unsigned long long bal = __ballot(fixed);
    if (threadIdx.x == 0)
        row_cnt[threadIdx.y] = (unsigned int)__popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        const unsigned long long cnt = (unsigned long long)row_cnt[0] + row_cnt[1] + row_cnt[2] + row_cnt[3];
        if (cnt)
            atomicAdd(out, cnt);
    }
}

void k_mask_count(const Geom &g, const unsigned char *m, int bc, unsigned long long *out, hipStream_t s)
{
    dim3 grid((g.N + WAVE - 1) / WAVE, (g.N + 3) / 4, g.N);
    hipLaunchKernelGGL(mask_count_kernel<unsigned char>, grid, dim3(WAVE, 4, 1), 0, s, g, m, bc, out);
}

void k_field_count(const Geom &g, const double *f, int bc, unsigned long long *out, hipStream_t s)
{
    dim3 grid((g.N + WAVE - 1) / WAVE, (g.N + 3) / 4, g.N);
    hipLaunchKernelGGL(mask_count_kernel<double>, grid, dim3(WAVE, 4, 1), 0, s, g, f, bc, out);
}

/* the caller's bytes (any element strides) into the level's padded layout; a periodic duplicate takes its source's byte */
__global__ void __launch_bounds__(256) mask_pack_kernel(Geom g, unsigned char *__restrict__ m,
                                                        const unsigned char *__restrict__ a, long long si, long long sj,
                                                        long long sk, int axes)
{
    const int k = blockIdx.x * WAVE + threadIdx.x;
    const int j = blockIdx.y * 4 + threadIdx.y;
    const int i = blockIdx.z;
    const int N = g.N;
    if (k >= N || j >= N)
        return;
    const int qi = ((axes & 1) && i == N - 1) ? 0 : i, qj = ((axes & 2) && j == N - 1) ? 0 : j,
              qk = ((axes & 4) && k == N - 1) ? 0 : k;
    m[gidx(g, i, j, k)] = a[si * qi + sj * qj + sk * qk];
}

void k_mask_pack(const Geom &g, unsigned char *m, const mg3d_array &a, int bc, hipStream_t s)
{
    dim3 grid((g.N + WAVE - 1) / WAVE, (g.N + 3) / 4, g.N);
    hipLaunchKernelGGL(mask_pack_kernel, grid, dim3(WAVE, 4, 1), 0, s, g, m, (const unsigned char *)a.ptr, a.stride[0],
                       a.stride[1], a.stride[2], bc & 7);
}

/* Zeros of a field on the faces of the mask `faces` (MG3D_NEUMANN_* numbering: bit 2*ax low, 2*ax+1 high): blockIdx.z =
 * the face, (a, b) its other two indices.  For r when faces stop being unknowns: a Dirichlet face of r is never written by
 * a cycle and is injected into the coarse right-hand side, so what the residual of the other operator left there must go. */
__global__ void __launch_bounds__(256) zero_faces_kernel(Geom g, double *__restrict__ v, int faces)
{
    const int b = blockIdx.x * WAVE + threadIdx.x, a = blockIdx.y * 4 + threadIdx.y, f = blockIdx.z;
    const int N = g.N;
    if (a >= N || b >= N || !(faces >> f & 1))
        return;
    const int ax = f >> 1, x = (f & 1) ? N - 1 : 0;
    v[gidx(g, ax == 0 ? x : a, ax == 1 ? x : (ax == 0 ? a : b), ax == 2 ? x : b)] = 0.;
}

void k_zero_faces(const Geom &g, double *v, int faces, hipStream_t s)
{
    if (!faces)
        return;
    dim3 grid((g.N + WAVE - 1) / WAVE, (g.N + 3) / 4, 6);
    hipLaunchKernelGGL(zero_faces_kernel, grid, dim3(WAVE, 4, 1), 0, s, g, v, faces);
}

/* ------------------------------------------------------------- device arrays
 * A caller's N^3 array in device memory (mg3d_array: float or double, any element strides) into and out of a level's padded
 * layout.  One thread per point, k across the wave: with a k stride of 1 both sides move whole rows; any other stride is
 * served as it comes.  The strided index is 64-bit.  Only the N points of a row are touched on the padded side. */
template <class T>
__global__ void __launch_bounds__(256) pack_kernel(Geom g, double *__restrict__ v, const T *__restrict__ a, long long si,
                                                   long long sj, long long sk)
{
    const int k = blockIdx.x * WAVE + threadIdx.x;
    const int j = blockIdx.y * 4 + threadIdx.y;
    const int i = blockIdx.z;
    if (k >= g.N || j >= g.N)
        return;
    v[gidx(g, i, j, k)] = (double)a[si * i + sj * j + sk * k];
}

template <class T>
__global__ void __launch_bounds__(256) unpack_kernel(Geom g, const double *__restrict__ v, T *__restrict__ a, long long si,
                                                     long long sj, long long sk)
{
    const int k = blockIdx.x * WAVE + threadIdx.x;
    const int j = blockIdx.y * 4 + threadIdx.y;
    const int i = blockIdx.z;
    if (k >= g.N || j >= g.N)
        return;
    a[si * i + sj * j + sk * k] = (T)v[gidx(g, i, j, k)]; /* (float: round to nearest even) */
}

/* A wave is one row of 64 k: its bad entries as a ballot, the lowest bad lane is the lowest dense index of the row; the
 * block's four rows meet in LDS and thread (0,0) issues the two atomics, only when the block found anything.
 * ZERO_OK: a screening field (k_field_check) -- finite and >= 0 instead of > 0. */
template <class T, bool ZERO_OK>
__global__ void __launch_bounds__(256) coef_check_kernel(Geom g, const T *__restrict__ a, long long si, long long sj,
                                                         long long sk, int axes, unsigned long long *__restrict__ out)
{
    const int k = blockIdx.x * WAVE + threadIdx.x;
    const int j = blockIdx.y * 4 + threadIdx.y;
    const int i = blockIdx.z;
    const int N = g.N;
    bool bad = false;
    if (k < N && j < N) {
        const bool dup = ((axes & 1) && i == N - 1) || ((axes & 2) && j == N - 1) || ((axes & 4) && k == N - 1);
        if (!dup) {
            const double e = (double)a[si * i + sj * j + sk * k];
            bad = !(ZERO_OK ? e >= 0. : e > 0.) || !(e <= 1.7976931348623157e308); /* NaN, <= 0 (ZERO_OK: < 0), +inf */
        }
    }
    __shared__ unsigned long long row_min[4];
    __shared__ unsigned int row_cnt[4];
    const unsigned long long m = __ballot(bad);
    if (threadIdx.x == 0) {
        row_cnt[threadIdx.y] = (unsigned int)__popcll(m);
        row_min[threadIdx.y] = m ? ((unsigned long long)i * N + j) * N + (blockIdx.x * WAVE + (__ffsll((long long)m) - 1)) : ~0ULL;
    }
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) {
        unsigned long long cnt = 0, lo = ~0ULL;
        for (int r = 0; r < 4; r++) {
            cnt += row_cnt[r];
            lo = row_min[r] < lo ? row_min[r] : lo;
        }
        if (cnt) {
            atomicAdd(out, cnt);
            atomicMin(out + 1, lo);
        }
    }
}

void k_pack(const Geom &g, double *v, const mg3d_array &a, hipStream_t s)
{
    dim3 grid((g.N + WAVE - 1) / WAVE, (g.N + 3) / 4, g.N);
    if (a.dtype == MG3D_F32)
        hipLaunchKernelGGL(pack_kernel<float>, grid, dim3(WAVE, 4, 1), 0, s, g, v, (const float *)a.ptr, a.stride[0],
                           a.stride[1], a.stride[2]);
    else
        hipLaunchKernelGGL(pack_kernel<double>, grid, dim3(WAVE, 4, 1), 0, s, g, v, (const double *)a.ptr, a.stride[0],
                           a.stride[1], a.stride[2]);
}

void k_unpack(const Geom &g, const double *v, const mg3d_array &a, hipStream_t s)
{
    dim3 grid((g.N + WAVE - 1) / WAVE, (g.N + 3) / 4, g.N);
    if (a.dtype == MG3D_F32)
        hipLaunchKernelGGL(unpack_kernel<float>, grid, dim3(WAVE, 4, 1), 0, s, g, v, (float *)a.ptr, a.stride[0], a.stride[1],
                           a.stride[2]);
    else
        hipLaunchKernelGGL(unpack_kernel<double>, grid, dim3(WAVE, 4, 1), 0, s, g, v, (double *)a.ptr, a.stride[0],
                           a.stride[1], a.stride[2]);
}

template <bool ZERO_OK>
static void launch_check(const Geom &g, const mg3d_array &a, int bc, unsigned long long *out, hipStream_t s)
{
    dim3 grid((g.N + WAVE - 1) / WAVE, (g.N + 3) / 4, g.N);
    if (a.dtype == MG3D_F32)
        hipLaunchKernelGGL((coef_check_kernel<float, ZERO_OK>), grid, dim3(WAVE, 4, 1), 0, s, g, (const float *)a.ptr,
                           a.stride[0], a.stride[1], a.stride[2], bc & 7, out);
    else
        hipLaunchKernelGGL((coef_check_kernel<double, ZERO_OK>), grid, dim3(WAVE, 4, 1), 0, s, g, (const double *)a.ptr,
                           a.stride[0], a.stride[1], a.stride[2], bc & 7, out);
}

void k_coef_check(const Geom &g, const mg3d_array &a, int bc, unsigned long long *out, hipStream_t s)
{
    launch_check<false>(g, a, bc, out, s);
}

void k_field_check(const Geom &g, const mg3d_array &a, int bc, unsigned long long *out, hipStream_t s)
{
    launch_check<true>(g, a, bc, out, s);
}

/* --------------------------------------------------------------- field output
 * The gradient of u of a single-domain level at every one of its N^3 points, into up to three caller's arrays (GradOut,
 * include/mg3d.h "Field output").  cs = scale * (0.5 / h).  Per axis, at index x of the point's SOURCE (a periodic
 * duplicate N-1 takes index 0 of that axis, on all three axes, so no duplicate of u is read and a duplicate gets its
 * source's bits), with c = u at the source:
 *   periodic axis, Neumann face, interior : (u[hi] - u[lo]) * cs -- wrapped (nb_lo / nb_hi) or reflected: at a Neumann
 *                                           face both taps are the same inner neighbour, a zero
 *   x = 0 on a Dirichlet face             : ((4.0*u[1] - 3.0*c) - u[2]) * cs
 *   x = N-1 on a Dirichlet face           : ((3.0*c - 4.0*u[N-2]) + u[N-3]) * cs
 * GradAxis holds that for one index: two tap offsets relative to the source point and which of the three forms applies.
 * Shape: (WAVE, 4) blocks, lanes contiguous in k, over ALL N indices of k and j (not column<BC>'s unknowns); a thread
 * walks a chunk of planes and carries u of the planes behind, at and ahead of the source plane in registers, as
 * walk_column does -- one new plane tap per point, plus the third tap on the two planes of a Dirichlet i face; the four
 * in-plane taps are the cache lines the neighbouring rows and lanes load (taking the k taps from the neighbouring lanes'
 * registers instead measured slower: 1.39 against 1.29 ms).  With a k stride of 1 each component store is a row segment.
 * eps and the mask play no part. */
struct GradOut {
    void *p[3];         /* NULL: component not wanted */
    long long s[3][3];  /* element strides of component a for i, j, k */
    int f32[3];         /* float (rounded to nearest even) instead of double */
};
struct GradAxis {
    int src;          /* the source index */
    long long oa, ob; /* kind 0: the +1 and -1 taps; 1: indices 1 and 2; 2: indices N-2 and N-3 */
    int kind;         /* 0 central, 1 / 2 one-sided at the low / high Dirichlet face */
};
template <int BC>
__device__ __forceinline__ GradAxis grad_axis(int bc, int ax, int x, int N, long long st)
{
    const bool per = BC && (bc >> ax & 1);
    const bool rlo = BC == BC_REFLECT && bc_ref_lo(bc, ax), rhi = BC == BC_REFLECT && bc_ref_hi(bc, ax);
    GradAxis a;
    a.src = (per && x == N - 1) ? 0 : x;
    a.kind = per ? 0 : ((x == 0 && !rlo) ? 1 : ((x == N - 1 && !rhi) ? 2 : 0));
    if (a.kind == 1) {
        a.oa = st;
        a.ob = 2 * st;
    } else if (a.kind == 2) {
        a.oa = -st;
        a.ob = -2 * st;
    } else {
        a.oa = nb_hi(a.src, N, per, rhi, st);
        a.ob = nb_lo(a.src, N, per, rlo, st);
    }
    return a;
}
/* the value of one axis from its two taps ta (at oa), tb (at ob) and the centre c */
__device__ __forceinline__ double grad_value(int kind, double ta, double tb, double c, double cs)
{
    if (kind == 1)
        return ((4.0 * ta - 3.0 * c) - tb) * cs;
    if (kind == 2)
        return ((3.0 * c - 4.0 * ta) + tb) * cs;
    return (ta - tb) * cs;
}
__device__ __forceinline__ void grad_store(const GradOut &o, int a, int i, int j, int k, double x)
{
    if (!o.p[a])
        return;
    const long long q = o.s[a][0] * i + o.s[a][1] * j + o.s[a][2] * k;
    /* written once, read by nobody here: nontemporal, the cache keeps u's planes (513^3, three float64 components, 16
     * planes per thread: 1.36 -> 1.29 ms) */
    if (o.f32[a])
        __builtin_nontemporal_store((float)x, (float *)o.p[a] + q); /* (round to nearest even) */
    else
        __builtin_nontemporal_store(x, (double *)o.p[a] + q);
}
/* planes per thread.  The carry pays from two planes on (one plane per thread, every tap loaded: 1.36 ms at 513^3); past
 * that a SHORTER chunk is faster with three components -- 16 planes 1.29 ms, 8 1.25, 4 1.19, 2 1.18 -- though not with one
 * (0.79 - 0.80 ms throughout): the blocks in flight then cover few plane positions, and the four arrays are streamed
 * through nearly in order instead of at some thirty places each */
#define GRAD_CHUNK 4

template <int BC>
__global__ void __launch_bounds__(256) gradient_kernel(Geom g, const double *__restrict__ u, GradOut o, double cs, int bc,
                                                       int chunk)
{
    const int N = g.N;
    const int k = blockIdx.x * WAVE + threadIdx.x;
    const int j = blockIdx.y * 4 + threadIdx.y;
    if (k >= N || j >= N)
        return;
    const int i0 = blockIdx.z * chunk, i1 = min(i0 + chunk, N);
    const GradAxis aj = grad_axis<BC>(bc, 1, j, N, g.pitch), ak = grad_axis<BC>(bc, 2, k, N, 1);
    const long long row = (long long)g.pitch * aj.src + ak.src;
    /* u at and behind the first source plane: the -1 tap, plane N-2 on the Dirichlet high face (a chunk may start there);
     * on the Dirichlet low face nothing lies behind and the one-sided form does not look at vb */
    GradAxis ai = grad_axis<BC>(bc, 0, i0, N, g.plane);
    long long p = g.plane * ai.src + row;
    double vh = u[p];
    double vb = ai.kind == 0 ? u[p + ai.ob] : (ai.kind == 2 ? u[p + ai.oa] : vh);
    for (int i = i0; i < i1; i++) {
        ai = grad_axis<BC>(bc, 0, i, N, g.plane);
        p = g.plane * ai.src + row;
        /* the plane ahead; on the Dirichlet high face there is none and the taps are N-2 (carried) and N-3 */
        const double va = ai.kind == 2 ? vb : u[p + ai.oa];
        double gi;
        if (ai.kind == 0)
            gi = grad_value(0, va, vb, vh, cs);
        else
            gi = grad_value(ai.kind, va, u[p + ai.ob], vh, cs);
        const double gj = grad_value(aj.kind, u[p + aj.oa], u[p + aj.ob], vh, cs);
        const double gk = grad_value(ak.kind, u[p + ak.oa], u[p + ak.ob], vh, cs);
        grad_store(o, 0, i, j, k, gi);
        grad_store(o, 1, i, j, k, gj);
        grad_store(o, 2, i, j, k, gk);
        vb = vh;
        vh = va;
    }
}

int k_gradient(const Geom &g, const double *u, int bc, double cs, const mg3d_array *const out[3], hipStream_t s)
{
    if (g.N < 3 || g.ni != g.N || g.nj != g.N || g.nk != g.N)
        return -1;
    GradOut o;
    for (int a = 0; a < 3; a++) {
        o.p[a] = out[a] ? out[a]->ptr : nullptr;
        o.f32[a] = out[a] && out[a]->dtype == MG3D_F32;
        for (int t = 0; t < 3; t++)
            o.s[a][t] = out[a] ? out[a]->stride[t] : 0;
    }
    const int chunk = GRAD_CHUNK;
    const dim3 grid((g.N + WAVE - 1) / WAVE, (g.N + 3) / 4, (g.N + chunk - 1) / chunk), block(WAVE, 4, 1);
    switch (bc_mode(bc)) {
    case BC_REFLECT:
        hipLaunchKernelGGL(gradient_kernel<BC_REFLECT>, grid, block, 0, s, g, u, o, cs, bc, chunk);
        break;
    case BC_WRAP:
        hipLaunchKernelGGL(gradient_kernel<BC_WRAP>, grid, block, 0, s, g, u, o, cs, bc, chunk);
        break;
    default:
        hipLaunchKernelGGL(gradient_kernel<BC_PLAIN>, grid, block, 0, s, g, u, o, cs, bc, chunk);
    }
    return 0;
}

/* ----------------------------------------------------------------- particles
 * The gather and the scatter between points and a single-domain level (include/mg3d.h "Particles"; the launchers'
 * contract is in mg3d_internal.h).  One thread per point, 256 per block, the grid capped at MG3D_PARTICLE_MAX_BLOCKS with
 * a stride loop behind it.  PartVec is a caller's vector (mg3d_vec), PartCell the cell of a point on one axis: the lower
 * node c (0 .. N-2) and the weights of c and c+1. */
struct PartVec {
    void *p; /* NULL: not given / not wanted */
    long long s;
    int f32;
};
struct PartPos {
    PartVec x[3];
};
struct PartOut {
    PartVec v[4]; /* u, then the three components of the gradient */
};
static PartVec part_vec(const mg3d_vec *v)
{
    PartVec o = {nullptr, 0, 0};
    if (v) {
        o.p = v->ptr;
        o.s = v->stride;
        o.f32 = v->dtype == MG3D_F32;
    }
    return o;
}
__device__ __forceinline__ double part_load(const PartVec &v, long long m)
{
    return v.f32 ? (double)((const float *)v.p)[v.s * m] : ((const double *)v.p)[v.s * m];
}
__device__ __forceinline__ void part_store(const PartVec &v, long long m, double x)
{
    if (!v.p)
        return;
    if (v.f32)
        ((float *)v.p)[v.s * m] = (float)x; /* (round to nearest even) */
    else
        ((double *)v.p)[v.s * m] = x;
}
struct PartCell {
    int c;
    double w0, w1;
};
/* false: the point is outside on this axis */
template <int BC>
__device__ __forceinline__ bool part_locate(int bc, int ax, double x, double h, int N, PartCell &o)
{
    const double n1 = (double)(N - 1);
    double t = x / h;
    if (!isfinite(x) || !isfinite(t))
        return false;
    if (BC && (bc >> ax & 1)) {
        t = t - n1 * floor(t / n1);
        /* what the rounding of the wrap leaves outside [0, N-1] goes to the nearer end (-0.0 stays) */
        if (!(t >= 0.0))
            t = 0.0;
        if (t > n1)
            t = n1;
    } else if (!(0.0 <= t && t <= n1)) {
        return false;
    }
    int c = (int)floor(t);
    if (c > N - 2)
        c = N - 2;
    const double f = t - (double)c;
    o.c = c;
    o.w0 = 1.0 - f;
    o.w1 = f;
    return true;
}
template <int BC>
__device__ __forceinline__ bool part_locate3(int bc, const PartPos &pos, long long m, double h, int N, PartCell (&cell)[3])
{
    bool in = true;
#pragma unroll
    for (int ax = 0; ax < 3; ax++)
        in = part_locate<BC>(bc, ax, part_load(pos.x[ax], m), h, N, cell[ax]) && in;
    return in;
}
/* the nested sum over the eight corners of a cell, val(a*4 + b*2 + c) the value at corner (a, b, c) */
template <class F>
__device__ __forceinline__ double part_trilinear(const PartCell (&cell)[3], F val)
{
    double mid[2];
#pragma unroll
    for (int a = 0; a < 2; a++) {
        const double in0 = (cell[2].w0 * val(a * 4 + 0)) + (cell[2].w1 * val(a * 4 + 1));
        const double in1 = (cell[2].w0 * val(a * 4 + 2)) + (cell[2].w1 * val(a * 4 + 3));
        mid[a] = (cell[1].w0 * in0) + (cell[1].w1 * in1);
    }
    return (cell[0].w0 * mid[0]) + (cell[0].w1 * mid[1]);
}

/* The gather of the sample and of the push at a located point.  The eight corners of the cell are taken to their sources and
 * loaded once; the nodal gradient at a corner is grad_value of grad_axis's taps, as gradient_kernel forms it.  Of a corner's
 * two taps along an axis one is, away from the boundary forms, the cell's other corner on that axis and comes from its
 * register: 8 + 24 loads of u per point.  want(t) says whether value t (0: u, 1 + d: component d of the gradient) is
 * asked for, emit(t, x) takes it. */
template <int BC, class W, class E>
__device__ __forceinline__ void part_gather(const Geom &g, const double *__restrict__ u, int bc, double cs,
                                            const PartCell (&cell)[3], W want, E emit)
{
    const int N = g.N;
    GradAxis ga[3][2];
#pragma unroll
    for (int e = 0; e < 2; e++) {
        ga[0][e] = grad_axis<BC>(bc, 0, cell[0].c + e, N, g.plane);
        ga[1][e] = grad_axis<BC>(bc, 1, cell[1].c + e, N, g.pitch);
        ga[2][e] = grad_axis<BC>(bc, 2, cell[2].c + e, N, 1);
    }
    long long p[8];
    double v[8];
#pragma unroll
    for (int t = 0; t < 8; t++) {
        p[t] = g.plane * ga[0][t >> 2].src + (long long)g.pitch * ga[1][(t >> 1) & 1].src + ga[2][t & 1].src;
        v[t] = u[p[t]];
    }
    if (want(0))
        emit(0, part_trilinear(cell, [&](int t) { return v[t]; }));
#pragma unroll
    for (int d = 0; d < 3; d++) {
        if (!want(1 + d))
            continue;
        const int bit = 4 >> d;
        const double gd = part_trilinear(cell, [&](int t) {
            const GradAxis &A = ga[d][(t & bit) ? 1 : 0];
            const long long po = p[t ^ bit], qa = p[t] + A.oa, qb = p[t] + A.ob;
            const double ta = qa == po ? v[t ^ bit] : u[qa];
            const double tb = qb == po ? v[t ^ bit] : u[qb];
            return grad_value(A.kind, ta, tb, v[t], cs);
        });
        emit(1 + d, gd);
    }
}

/* The sample: the gather into the caller's wanted outputs, NaN for a point outside. */
template <int BC>
__global__ void __launch_bounds__(256) part_sample_kernel(Geom g, const double *__restrict__ u, PartPos pos, long long count,
                                                          double h, double cs, int bc, PartOut o)
{
    const int N = g.N;
    const bool wanted[4] = {o.v[0].p != nullptr, o.v[1].p != nullptr, o.v[2].p != nullptr, o.v[3].p != nullptr};
    for (long long m = blockIdx.x * 256LL + threadIdx.x; m < count; m += 256LL * gridDim.x) {
        PartCell cell[3];
        if (!part_locate3<BC>(bc, pos, m, h, N, cell)) {
            const double nan = __builtin_nan("");
#pragma unroll
            for (int t = 0; t < 4; t++)
                part_store(o.v[t], m, nan);
            continue;
        }
        part_gather<BC>(g, u, bc, cs, cell, [&](int t) { return wanted[t]; },
                        [&](int t, double x) { part_store(o.v[t], m, x); });
    }
}

/* The push (include/mg3d.h "Particles", mg3d_particle_push_device): locate, gather E, kick and drift, the walls of the
 * context's boundary word, the conductors of its mask, then the stores and one count per particle that changes its fate.
 * Every floating-point operation is spelled as the header spells it. */
struct PartPush {
    double dt, cs, gdt[3], inv, xper, xhi; /* the host's constants */
    PartPos vel;
    PartVec qm;
    int *fate;
    long long fate_stride;
};
template <int BC>
__global__ void __launch_bounds__(256) part_push_kernel(Geom g, const double *__restrict__ u,
                                                        const unsigned char *__restrict__ mask, PartPos pos, long long count,
                                                        double h, int bc, PartPush a, unsigned long long *__restrict__ table)
{
    const int N = g.N;
    const double n1 = (double)(N - 1);
    for (long long m = blockIdx.x * 256LL + threadIdx.x; m < count; m += 256LL * gridDim.x) {
        int *const fp = a.fate + a.fate_stride * m;
        if (*fp != MG3D_FATE_ALIVE)
            continue;
        /* 1: locate x0; a point that is not inside only changes its fate */
        double x[3];
        PartCell cell[3];
        bool in = true, finite = true;
        int face = -1;
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
            x[ax] = part_load(pos.x[ax], m);
            const double t = x[ax] / h;
            const bool here = part_locate<BC>(bc, ax, x[ax], h, N, cell[ax]);
            in = in && here;
            finite = finite && isfinite(x[ax]) && isfinite(t);
            if (!here && face < 0)
                face = 2 * ax + (t < 0.0 ? 0 : 1);
        }
        int f = MG3D_FATE_ALIVE;
        if (!in) {
            f = finite ? MG3D_FATE_FACE + face : MG3D_FATE_INVALID;
        } else {
            /* 2: E, the sample's gradient with cs */
            double E[3];
            part_gather<BC>(g, u, bc, a.cs, cell, [](int t) { return t != 0; }, [&](int t, double e) { E[t - 1] = e; });
            /* 3: kick and drift */
            const double k = part_load(a.qm, m) * a.dt;
            double v[3];
            bool ok = isfinite(k);
#pragma unroll
            for (int ax = 0; ax < 3; ax++) {
                v[ax] = (part_load(a.vel.x[ax], m) + ((k * E[ax]) + a.gdt[ax])) * a.inv;
                x[ax] = x[ax] + (a.dt * v[ax]);
                ok = ok && isfinite(v[ax]) && isfinite(x[ax]);
            }
            if (!ok) {
                f = MG3D_FATE_INVALID;
            } else {
                /* 4: walls, each axis on its own; the first exit in axis order is the fate */
#pragma unroll
                for (int ax = 0; ax < 3; ax++) {
                    const double tt = x[ax] / h;
                    if (BC && (bc >> ax & 1)) {
                        if (tt < 0.0)
                            x[ax] = x[ax] + a.xper;
                        else if (tt >= n1)
                            x[ax] = x[ax] - a.xper;
                    } else if (tt < 0.0) {
                        if (BC == BC_REFLECT && bc_ref_lo(bc, ax)) {
                            x[ax] = -x[ax];
                            v[ax] = -v[ax];
                        } else if (f == MG3D_FATE_ALIVE) {
                            f = MG3D_FATE_FACE + 2 * ax;
                        }
                    } else if (tt > n1) {
                        if (BC == BC_REFLECT && bc_ref_hi(bc, ax)) {
                            x[ax] = a.xhi - (x[ax] - a.xhi);
                            v[ax] = -v[ax];
                        } else if (f == MG3D_FATE_ALIVE) {
                            f = MG3D_FATE_FACE + 2 * ax + 1;
                        }
                    }
                }
                /* 5: conductors: the mask byte of the node nearest to the final position, where that is inside */
                if (mask && f == MG3D_FATE_ALIVE) {
                    int n[3];
                    bool there = true;
#pragma unroll
                    for (int ax = 0; ax < 3; ax++) {
                        PartCell c = {0, 0., 0.};
                        there = part_locate<BC>(bc, ax, x[ax], h, N, c) && there;
                        n[ax] = c.c + (c.w1 >= 0.5 ? 1 : 0);
                        if (BC && (bc >> ax & 1) && n[ax] == N - 1)
                            n[ax] = 0;
                    }
                    if (there)
                        f = mask[gidx(g, n[0], n[1], n[2])];
                }
                /* 6: the position and velocity of survivors and of what steps 4 and 5 retired */
#pragma unroll
                for (int ax = 0; ax < 3; ax++) {
                    part_store(pos.x[ax], m, x[ax]);
                    part_store(a.vel.x[ax], m, v[ax]);
                }
            }
        }
        if (f != MG3D_FATE_ALIVE) {
            *fp = f;
            atomicAdd(table + f, 1ULL);
        }
    }
}

static dim3 part_grid(long long count)
{
    const long long blocks = (count + 255) / 256;
    return dim3((unsigned)(blocks < MG3D_PARTICLE_MAX_BLOCKS ? blocks : MG3D_PARTICLE_MAX_BLOCKS), 1, 1);
}
static bool part_level_ok(const Geom &g) { return g.N >= 3 && g.ni == g.N && g.nj == g.N && g.nk == g.N; }
static PartPos part_pos(const mg3d_vec *const pos[3])
{
    PartPos p;
    for (int a = 0; a < 3; a++)
        p.x[a] = part_vec(pos[a]);
    return p;
}

int k_part_sample(const Geom &g, const double *u, int bc, double h, double cs, long long count, const mg3d_vec *const pos[3],
                  const mg3d_vec *u_out, const mg3d_vec *const grad_out[3], hipStream_t s)
{
    if (!part_level_ok(g) || count <= 0)
        return -1;
    PartOut o;
    o.v[0] = part_vec(u_out);
    for (int a = 0; a < 3; a++)
        o.v[1 + a] = part_vec(grad_out ? grad_out[a] : nullptr);
    const PartPos p = part_pos(pos);
    const dim3 grid = part_grid(count), block(256, 1, 1);
    switch (bc_mode(bc)) {
    case BC_REFLECT:
        hipLaunchKernelGGL(part_sample_kernel<BC_REFLECT>, grid, block, 0, s, g, u, p, count, h, cs, bc, o);
        break;
    case BC_WRAP:
        hipLaunchKernelGGL(part_sample_kernel<BC_WRAP>, grid, block, 0, s, g, u, p, count, h, cs, bc, o);
        break;
    default:
        hipLaunchKernelGGL(part_sample_kernel<BC_PLAIN>, grid, block, 0, s, g, u, p, count, h, cs, bc, o);
    }
    return 0;
}

int k_part_push(const Geom &g, const double *u, const unsigned char *mask, int bc, double h, long long count,
                const mg3d_vec *const pos[3], const mg3d_vec *const vel[3], const mg3d_vec *qm, const mg3d_vec *fate,
                const mg3d_push_params &pp, unsigned long long *table, hipStream_t s)
{
    if (!part_level_ok(g) || count <= 0)
        return -1;
    PartPush a;
    a.dt = pp.dt;
    a.cs = pp.scale * (0.5 / h);
    for (int ax = 0; ax < 3; ax++)
        a.gdt[ax] = pp.dt * pp.accel[ax];
    a.inv = 1.0 / (1.0 + pp.drag * pp.dt);
    const double n1 = (double)(g.N - 1);
    a.xper = n1 * h;
    a.xhi = a.xper;
    while (a.xhi / h > n1) /* the largest coordinate known to locate inside */
        a.xhi = nextafter(a.xhi, 0.0);
    a.vel = part_pos(vel);
    a.qm = part_vec(qm);
    a.fate = (int *)fate->ptr;
    a.fate_stride = fate->stride;
    const PartPos p = part_pos(pos);
    const dim3 grid = part_grid(count), block(256, 1, 1);
    switch (bc_mode(bc)) {
    case BC_REFLECT:
        hipLaunchKernelGGL(part_push_kernel<BC_REFLECT>, grid, block, 0, s, g, u, mask, p, count, h, bc, a, table);
        break;
    case BC_WRAP:
        hipLaunchKernelGGL(part_push_kernel<BC_WRAP>, grid, block, 0, s, g, u, mask, p, count, h, bc, a, table);
        break;
    default:
        hipLaunchKernelGGL(part_push_kernel<BC_PLAIN>, grid, block, 0, s, g, u, mask, p, count, h, bc, a, table);
    }
    return 0;
}

/* The deposit.  scan: the largest |q| among the points that will deposit, as its bit pattern (for non-negative doubles the
 * order of the patterns is the order of the values): a thread's own maximum, the wave's by shuffles, one atomic per wave. */
template <int BC>
__global__ void __launch_bounds__(256) part_scan_kernel(Geom g, PartPos pos, PartVec q, long long count, double h, int bc,
                                                        unsigned long long *__restrict__ amax)
{
    unsigned long long best = 0;
    for (long long m = blockIdx.x * 256LL + threadIdx.x; m < count; m += 256LL * gridDim.x) {
        const double qv = part_load(q, m);
        PartCell cell[3];
        if (!isfinite(qv) || !part_locate3<BC>(bc, pos, m, h, g.N, cell))
            continue;
        const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(qv));
        best = b > best ? b : best;
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(best, off, WAVE);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & (WAVE - 1)) == 0 && best != 0)
        atomicMax(amax, best);
}
/* the unit 2^ue of the accumulator from A = max |q| and K; false: nothing deposits */
__device__ __forceinline__ bool part_unit(const unsigned long long *amax, int K, int &ue)
{
    const unsigned long long b = *amax;
    if (b == 0)
        return false;
    ue = ilogb(__longlong_as_double((long long)b)) + 1 + K - 62;
    return true;
}
/* accumulate: eight 64-bit integer adds per point, at the sources of the cell's nodes */
template <int BC>
__global__ void __launch_bounds__(256) part_accumulate_kernel(Geom g, PartPos pos, PartVec q, long long count, double h, int bc,
                                                              int K, const unsigned long long *__restrict__ amax,
                                                              long long *__restrict__ acc)
{
    int ue;
    if (!part_unit(amax, K, ue))
        return;
    const int N = g.N;
    for (long long m = blockIdx.x * 256LL + threadIdx.x; m < count; m += 256LL * gridDim.x) {
        const double qv = part_load(q, m);
        PartCell cell[3];
        if (!isfinite(qv) || !part_locate3<BC>(bc, pos, m, h, N, cell))
            continue;
        long long off[3][2];
        const long long st[3] = {g.plane, g.pitch, 1};
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
            const bool per = BC && (bc >> ax & 1);
            off[ax][0] = st[ax] * cell[ax].c;
            off[ax][1] = (per && cell[ax].c + 1 == N - 1) ? 0 : st[ax] * (cell[ax].c + 1);
        }
#pragma unroll
        for (int t = 0; t < 8; t++) {
            const int a = t >> 2, b = (t >> 1) & 1, c = t & 1;
            const double w = ((a ? cell[0].w1 : cell[0].w0) * (b ? cell[1].w1 : cell[1].w0)) * (c ? cell[2].w1 : cell[2].w0);
            const long long n = llrint(ldexp(qv * w, -ue));
            if (n != 0)
                atomicAdd((unsigned long long *)(acc + (off[0][a] + off[1][b] + off[2][c])), (unsigned long long)n);
        }
    }
}
/* apply: over all N^3 nodes (the duplicates' accumulators stay 0), lanes contiguous in k */
__global__ void __launch_bounds__(256) part_apply_kernel(Geom g, int bc, double f0, int K,
                                                         const unsigned long long *__restrict__ amax,
                                                         const long long *__restrict__ acc, double *__restrict__ d)
{
    int ue;
    if (!part_unit(amax, K, ue))
        return;
    const int N = g.N;
    const int k = blockIdx.x * WAVE + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, i = blockIdx.z;
    if (k >= N || j >= N)
        return;
    const long long p = gidx(g, i, j, k);
    const long long a = acc[p];
    if (a == 0)
        return;
    const int x[3] = {i, j, k};
    double nf = 1.0;
#pragma unroll
    for (int ax = 0; ax < 3; ax++)
        if ((x[ax] == 0 && bc_ref_lo(bc, ax)) || (x[ax] == N - 1 && bc_ref_hi(bc, ax)))
            nf *= 2.0;
    d[p] = d[p] + (f0 * nf) * ldexp((double)a, ue);
}

int k_part_scan(const Geom &g, int bc, double h, long long count, const mg3d_vec *const pos[3], const mg3d_vec *q,
                unsigned long long *amax, hipStream_t s)
{
    if (!part_level_ok(g) || count <= 0)
        return -1;
    const PartPos p = part_pos(pos);
    const PartVec qv = part_vec(q);
    const dim3 grid = part_grid(count), block(256, 1, 1);
    switch (bc_mode(bc)) {
    case BC_REFLECT:
        hipLaunchKernelGGL(part_scan_kernel<BC_REFLECT>, grid, block, 0, s, g, p, qv, count, h, bc, amax);
        break;
    case BC_WRAP:
        hipLaunchKernelGGL(part_scan_kernel<BC_WRAP>, grid, block, 0, s, g, p, qv, count, h, bc, amax);
        break;
    default:
        hipLaunchKernelGGL(part_scan_kernel<BC_PLAIN>, grid, block, 0, s, g, p, qv, count, h, bc, amax);
    }
    return 0;
}

int k_part_accumulate(const Geom &g, int bc, double h, long long count, int K, const mg3d_vec *const pos[3],
                      const mg3d_vec *q, const unsigned long long *amax, long long *acc, hipStream_t s)
{
    if (!part_level_ok(g) || count <= 0)
        return -1;
    const PartPos p = part_pos(pos);
    const PartVec qv = part_vec(q);
    const dim3 grid = part_grid(count), block(256, 1, 1);
    switch (bc_mode(bc)) {
    case BC_REFLECT:
        hipLaunchKernelGGL(part_accumulate_kernel<BC_REFLECT>, grid, block, 0, s, g, p, qv, count, h, bc, K, amax, acc);
        break;
    case BC_WRAP:
        hipLaunchKernelGGL(part_accumulate_kernel<BC_WRAP>, grid, block, 0, s, g, p, qv, count, h, bc, K, amax, acc);
        break;
    default:
        hipLaunchKernelGGL(part_accumulate_kernel<BC_PLAIN>, grid, block, 0, s, g, p, qv, count, h, bc, K, amax, acc);
    }
    return 0;
}

int k_part_apply(const Geom &g, int bc, double f0, int K, const unsigned long long *amax, const long long *acc, double *d,
                 hipStream_t s)
{
    if (!part_level_ok(g))
        return -1;
    const dim3 grid((g.N + WAVE - 1) / WAVE, (g.N + 3) / 4, g.N);
    hipLaunchKernelGGL(part_apply_kernel, grid, dim3(WAVE, 4, 1), 0, s, g, bc, f0, K, amax, acc, d);
    return 0;
}

/* The reorder (include/mg3d.h "Particles", mg3d_particle_sort_device): a key per particle from the sample's locator, then a
 * least-significant-digit radix sort of (key, old index) with 8-bit digits.  A pass is three launches over tiles of
 * MG3D_SORT_TILE consecutive elements -- a constant, so the order cannot depend on a launch shape:
 *   hist    : table[digit][tile] = how many keys of the tile have that digit
 *   rowscan : each row of the table scanned in place (exclusive) by one block, the row's sum into tot[digit]
 *   scatter : element e of tile T with digit d goes to  (sum of tot[< d]) + table[d][T] + (its rank among the tile's
 *             elements of digit d in index order).
 * The rank: wave w of the block owns elements w*512 .. w*512+511 of the tile, lane l takes w*512 + 64*r + l in round r;
 * a round's rank is the number of lower lanes with the same digit (eight ballots give the lanes that match) plus the wave's
 * count of that digit from its earlier rounds, kept in LDS and advanced by the lowest matching lane; the waves' counts are
 * then turned into offsets in wave order.  Sums and ranks only: no atomic whose arrival order could decide a place, so the
 * sort is stable and has the same bits in every run.  The first pass takes the index of an element for its old index, the
 * last one writes no keys and stores the indices into the caller's perm. */
template <int BC>
__global__ void __launch_bounds__(256) sort_key_kernel(PartPos pos, PartVec fate, long long count, double h, int N, int bc,
                                                       int shift, unsigned nb, unsigned *__restrict__ keys,
                                                       unsigned long long *__restrict__ counts)
{
    const unsigned kmax = nb * nb * nb;
    unsigned n_in = 0, n_lost = 0;
    for (long long m = blockIdx.x * 256LL + threadIdx.x; m < count; m += 256LL * gridDim.x) {
        unsigned K = kmax + 1u; /* dead */
        if (!fate.p || ((const int *)fate.p)[fate.s * m] == 0) {
            PartCell cell[3];
            if (part_locate3<BC>(bc, pos, m, h, N, cell)) {
                K = (((unsigned)cell[0].c >> shift) * nb + ((unsigned)cell[1].c >> shift)) * nb + ((unsigned)cell[2].c >> shift);
                n_in++;
            } else {
                K = kmax; /* lost */
                n_lost++;
            }
        }
        keys[m] = K;
    }
    if (!counts)
        return;
    /* integer sums: a thread's own, the wave's by shuffles, one atomic add per wave */
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        n_in += __shfl_down(n_in, o, WAVE);
        n_lost += __shfl_down(n_lost, o, WAVE);
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        if (n_in)
            atomicAdd(counts, (unsigned long long)n_in);
        if (n_lost)
            atomicAdd(counts + 1, (unsigned long long)n_lost);
    }
}

/* the lanes of the wave that are valid and hold the digit d of this lane */
__device__ __forceinline__ unsigned long long sort_match(unsigned d, bool valid)
{
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long bal = __ballot(bit);
        m &= bit ? bal : ~bal;
    }
    return m;
}
/* the exclusive prefix of v over the 256 threads of the block and the block's sum; ws: four words of LDS, free again on
 * return */
__device__ __forceinline__ unsigned sort_block_scan(unsigned v, unsigned *ws, unsigned &total)
{
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    unsigned inc = v;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const unsigned t = __shfl_up(inc, o, WAVE);
        if (lane >= o)
            inc += t;
    }
    if (lane == WAVE - 1)
        ws[w] = inc;
    __syncthreads();
    unsigned pre = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const unsigned t = ws[i];
        pre += i < w ? t : 0u;
        tot += t;
    }
    __syncthreads();
    total = tot;
    return pre + (inc - v);
}

__global__ void __launch_bounds__(256) sort_hist_kernel(const unsigned *__restrict__ keys, long long count, int sh,
                                                        unsigned ntiles, unsigned *__restrict__ table)
{
    __shared__ unsigned hist[256];
    const int tid = threadIdx.x;
    const unsigned long long lt = (1ULL << (tid & (WAVE - 1))) - 1ULL;
    hist[tid] = 0;
    __syncthreads();
    const long long e0 = (long long)blockIdx.x * MG3D_SORT_TILE + tid;
#pragma unroll
    for (int r = 0; r < MG3D_SORT_TILE / 256; r++) {
        const long long e = e0 + 256LL * r;
        const bool valid = e < count;
        const unsigned d = valid ? (keys[e] >> sh) & 255u : 0u;
        const unsigned long long m = sort_match(d, valid);
        if (valid && (m & lt) == 0) /* the lowest matching lane adds for all of them (an integer sum in LDS) */
            atomicAdd(&hist[d], (unsigned)__popcll(m));
    }
    __syncthreads();
    table[(size_t)tid * ntiles + blockIdx.x] = hist[tid];
}

__global__ void __launch_bounds__(256) sort_rowscan_kernel(unsigned *__restrict__ table, unsigned ntiles,
                                                           unsigned *__restrict__ tot)
{
    __shared__ unsigned ws[4];
    unsigned *const row = table + (size_t)blockIdx.x * ntiles;
    unsigned carry = 0;
    for (unsigned c0 = 0; c0 < ntiles; c0 += 1024u) {
        const unsigned i0 = c0 + 4u * threadIdx.x;
        unsigned v[4], sum = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            v[j] = i0 + j < ntiles ? row[i0 + j] : 0u;
            sum += v[j];
        }
        unsigned total;
        unsigned run = carry + sort_block_scan(sum, ws, total);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (i0 + j < ntiles)
                row[i0 + j] = run;
            run += v[j];
        }
        carry += total;
    }
    if (threadIdx.x == 0)
        tot[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(256) sort_scatter_kernel(const unsigned *__restrict__ kin, const int *__restrict__ iin,
                                                           unsigned *__restrict__ kout, int *__restrict__ iout,
                                                           long long iout_stride, long long count, int sh, unsigned ntiles,
                                                           const unsigned *__restrict__ table,
                                                           const unsigned *__restrict__ tot)
{
    constexpr int ROUNDS = MG3D_SORT_TILE / 256;
    __shared__ unsigned wcnt[4][256];
    __shared__ unsigned ws[4];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const unsigned long long lt = (1ULL << lane) - 1ULL;
#pragma unroll
    for (int i = 0; i < 4; i++)
        wcnt[i][tid] = 0;
    /* thread tid speaks for digit tid: where the tile's elements of that digit begin */
    unsigned total;
    const unsigned first = sort_block_scan(tot[tid], ws, total) + table[(size_t)tid * ntiles + blockIdx.x];
    /* (the scan's barriers stand between the zeroes above and the rounds below) */
    volatile unsigned *const mine = wcnt[w];
    const long long e0 = (long long)blockIdx.x * MG3D_SORT_TILE + (long long)w * (WAVE * ROUNDS) + lane;
    unsigned key[ROUNDS], rank[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; r++) {
        const long long e = e0 + (long long)WAVE * r;
        const bool valid = e < count;
        key[r] = valid ? kin[e] : 0u;
        const unsigned d = (key[r] >> sh) & 255u;
        const unsigned long long m = sort_match(d, valid);
        const unsigned prev = mine[d];
        rank[r] = prev + (unsigned)__popcll(m & lt);
        __builtin_amdgcn_wave_barrier();
        if (valid && (m & lt) == 0)
            mine[d] = prev + (unsigned)__popcll(m);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    unsigned run = first;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const unsigned c = wcnt[i][tid];
        wcnt[i][tid] = run;
        run += c;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < ROUNDS; r++) {
        const long long e = e0 + (long long)WAVE * r;
        if (e >= count)
            continue;
        const long long dst = (long long)wcnt[w][(key[r] >> sh) & 255u] + rank[r];
        if (dst >= count)
            continue;
        if (kout)
            kout[dst] = key[r];
        iout[iout_stride * dst] = iin ? iin[e] : (int)e;
    }
}

int k_sort_keys(const Geom &g, int bc, double h, long long count, const mg3d_vec *const pos[3], const mg3d_vec *fate,
                int shift, unsigned *keys, unsigned long long *counts, hipStream_t s)
{
    if (!part_level_ok(g) || count <= 0)
        return -1;
    const PartPos p = part_pos(pos);
    const PartVec f = part_vec(fate);
    const unsigned nb = ((unsigned)(g.N - 2) >> shift) + 1u;
    const dim3 grid = part_grid(count), block(256, 1, 1);
    if (bc & 7)
        hipLaunchKernelGGL(sort_key_kernel<BC_WRAP>, grid, block, 0, s, p, f, count, h, g.N, bc, shift, nb, keys, counts);
    else
        hipLaunchKernelGGL(sort_key_kernel<BC_PLAIN>, grid, block, 0, s, p, f, count, h, g.N, bc, shift, nb, keys, counts);
    return 0;
}

void k_sort_hist(const unsigned *keys, long long count, int sh, unsigned *table, hipStream_t s)
{
    const unsigned ntiles = (unsigned)((count + MG3D_SORT_TILE - 1) / MG3D_SORT_TILE);
    hipLaunchKernelGGL(sort_hist_kernel, dim3(ntiles, 1, 1), dim3(256, 1, 1), 0, s, keys, count, sh, ntiles, table);
}

void k_sort_rowscan(long long count, unsigned *table, unsigned *tot, hipStream_t s)
{
    const unsigned ntiles = (unsigned)((count + MG3D_SORT_TILE - 1) / MG3D_SORT_TILE);
    hipLaunchKernelGGL(sort_rowscan_kernel, dim3(256, 1, 1), dim3(256, 1, 1), 0, s, table, ntiles, tot);
}

void k_sort_scatter(const unsigned *kin, const int *iin, unsigned *kout, int *iout, long long iout_stride, long long count,
                    int sh, const unsigned *table, const unsigned *tot, hipStream_t s)
{
    const unsigned ntiles = (unsigned)((count + MG3D_SORT_TILE - 1) / MG3D_SORT_TILE);
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(ntiles, 1, 1), dim3(256, 1, 1), 0, s, kin, iin, kout, iout, iout_stride,
                       count, sh, ntiles, table, tot);
}

/* The permute (mg3d_particle_permute_device): dst[v][m] = src[v][perm[m]] for up to MG3D_PERMUTE_MAX_VECS vectors, four or
 * eight bytes an element copied as they are; a perm[m] outside 0 .. count-1 reads and writes nothing.  The loop over the
 * vectors is unrolled with constant indices: the descriptors stay in the kernel's arguments. */
struct PermVecs {
    const void *src[MG3D_PERMUTE_MAX_VECS];
    void *dst[MG3D_PERMUTE_MAX_VECS];
    long long ss[MG3D_PERMUTE_MAX_VECS], ds[MG3D_PERMUTE_MAX_VECS];
    int wide[MG3D_PERMUTE_MAX_VECS]; /* eight bytes an element */
    int n;
};
__global__ void __launch_bounds__(256) part_permute_kernel(const int *__restrict__ perm, long long ps, long long count,
                                                           PermVecs a)
{
    for (long long m = blockIdx.x * 256LL + threadIdx.x; m < count; m += 256LL * gridDim.x) {
        const long long p = perm[ps * m];
        if (p < 0 || p >= count)
            continue;
#pragma unroll
        for (int v = 0; v < MG3D_PERMUTE_MAX_VECS; v++) {
            if (v >= a.n)
                break;
            if (a.wide[v])
                ((unsigned long long *)a.dst[v])[a.ds[v] * m] = ((const unsigned long long *)a.src[v])[a.ss[v] * p];
            else
                ((unsigned *)a.dst[v])[a.ds[v] * m] = ((const unsigned *)a.src[v])[a.ss[v] * p];
        }
    }
}

int k_part_permute(long long count, const mg3d_vec *perm, int nvec, const mg3d_vec *const *src, const mg3d_vec *const *dst,
                   hipStream_t s)
{
    if (count <= 0 || nvec < 1 || nvec > MG3D_PERMUTE_MAX_VECS)
        return -1;
    PermVecs a;
    memset(&a, 0, sizeof a);
    a.n = nvec;
    for (int v = 0; v < nvec; v++) {
        a.src[v] = src[v]->ptr;
        a.dst[v] = dst[v]->ptr;
        a.ss[v] = src[v]->stride;
        a.ds[v] = dst[v]->stride;
        a.wide[v] = src[v]->dtype == MG3D_F64;
    }
    hipLaunchKernelGGL(part_permute_kernel, part_grid(count), dim3(256, 1, 1), 0, s, (const int *)perm->ptr, perm->stride,
                       count, a);
    return 0;
}

/* The flux through the fixed unknowns: t_p = w(p) * (s - D*u_p) summed over the fixed unknowns p whose byte is `label`
 * (label 0: every nonzero byte), s and D of stencil<COEF> with dg0 = 6 (constant) or 0 (eps: D the sum of the six face
 * means) -- h^2 times the sigma = 0 operator --, w(p) = 1/2 per Neumann face p lies on.  The residual's column walk over
 * the unknowns, so bytes on Dirichlet faces and periodic duplicates are never looked at; one partial per block. */
template <bool COEF, int BC>
__global__ void __launch_bounds__(256) field_flux_kernel(Geom g, const double *__restrict__ v, const double *__restrict__ e,
                                                         const unsigned char *__restrict__ m, int label, double dg0,
                                                         double *__restrict__ partials, int bc, int chunk, int i_lo, int i_hi)
{
    __shared__ double lds4[4];
    double acc = 0.;
    Column c;
    if (column<BC>(g, bc, chunk, i_lo, i_hi, c)) {
        double wjk = 1.;
        if constexpr (BC == BC_REFLECT)
            wjk = bc_weight(bc, 1, c.j, g.N) * bc_weight(bc, 2, c.k, g.N);
        walk_column<COEF>(g, c, v, e, [&](const ColumnPoint<COEF> &pt) {
            const int b = m[pt.p];
            if (b == 0 || (label != 0 && b != label))
                return;
            double s, dg;
            pt.sum(dg0, s, dg);
            if constexpr (BC == BC_REFLECT)
                acc += (wjk * bc_weight(bc, 0, pt.i, g.N)) * (s - dg * pt.vh);
            else
                acc += s - dg * pt.vh;
        });
    }
    const double tot = block_sum_256(acc, lds4);
    if (threadIdx.x == 0 && threadIdx.y == 0)
        partials[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tot;
}

int k_field_flux(const Geom &g, const double *u, const LevelOperator &A, int label, double *partials, double *out,
                 hipStream_t s)
{
    int i_lo = -1, i_hi = -1;
    if (!stencil_window(g, A.bc, i_lo, i_hi)) {
        (void)hipMemsetAsync(out, 0, sizeof(double), s);
        return 0;
    }
    int chunk;
    const dim3 grid = column_grid(g, A.bc, i_hi - i_lo, chunk), block(WAVE, 4, 1);
    const double dg0 = A.e ? 0. : 6.; /* (the flux of div(eps grad u): sigma is no part of it) */
    dispatch_op(A.e, A.bc, nullptr, [&](auto coef, auto mode, auto) {
        hipLaunchKernelGGL((field_flux_kernel<coef(), mode()>), grid, block, 0, s, g, u, A.e, A.m, label, dg0, partials, A.bc,
                           chunk, i_lo, i_hi);
    });
    const int np = (int)(grid.x * grid.y * grid.z);
    k_fold(partials, np, out, s);
    return np;
}

/* The energy sum: over the edges e = (p, q) owned by their lower end p -- no duplicate on any axis --, along axis a to
 * x+1 (wrapped from N-2 to 0 on a periodic axis, absent at x = N-1 on another), left out when p lies on a Dirichlet face
 * of another axis,  (w_e * a_e) * ((u_q - u_p) * (u_q - u_p)),  w_e = 1/2 per Neumann face of another axis p lies on,
 * a_e = 1 or 0.5*(eps_p + eps_q); a point's edges are added in i, j, k order.  Threads over ALL N indices of j and k,
 * chunks of planes (16, doubled until the partial sums fit), u and eps of the plane ahead carried. */
struct EnergyAxis {
    bool own, edge, dir; /* the index is no duplicate; it has an edge to x+1; it lies on a Dirichlet face */
    double w;            /* 1/2 on a Neumann face */
    long long o;         /* offset to the upper end */
};
template <int BC>
__device__ __forceinline__ EnergyAxis energy_axis(int bc, int ax, int x, int N, long long st)
{
    const bool per = BC && (bc >> ax & 1);
    const bool rlo = BC == BC_REFLECT && bc_ref_lo(bc, ax), rhi = BC == BC_REFLECT && bc_ref_hi(bc, ax);
    EnergyAxis a;
    a.own = !(per && x == N - 1);
    a.edge = x <= N - 2;
    a.dir = !per && ((x == 0 && !rlo) || (x == N - 1 && !rhi));
    a.w = BC == BC_REFLECT ? bc_weight(bc, ax, x, N) : 1.;
    a.o = nb_hi(x, N, per, false, st);
    return a;
}
template <bool COEF, int BC>
__global__ void __launch_bounds__(256) field_energy_kernel(Geom g, const double *__restrict__ u, const double *__restrict__ e,
                                                           double *__restrict__ partials, int bc, int chunk)
{
    __shared__ double lds4[4];
    double acc = 0.;
    const int N = g.N;
    const int k = blockIdx.x * WAVE + threadIdx.x;
    const int j = blockIdx.y * 4 + threadIdx.y;
    const int i0 = blockIdx.z * chunk, i1 = min(i0 + chunk, N);
    if (k < N && j < N) {
        const EnergyAxis aj = energy_axis<BC>(bc, 1, j, N, g.pitch), ak = energy_axis<BC>(bc, 2, k, N, 1);
        if (aj.own && ak.own) {
            long long p = gidx(g, i0, j, k);
            double uh = u[p], eh = 0.;
            if constexpr (COEF)
                eh = e[p];
            for (int i = i0; i < i1; i++, p += g.plane) {
                const EnergyAxis ai = energy_axis<BC>(bc, 0, i, N, g.plane);
                double ua = 0., ea = 0.;
                if (ai.edge) { /* (also the next plane's own values) */
                    ua = u[p + ai.o];
                    if constexpr (COEF)
                        ea = e[p + ai.o];
                }
                if (ai.own) {
                    if (ai.edge && !aj.dir && !ak.dir) {
                        const double du = ua - uh;
                        acc += ((aj.w * ak.w) * (COEF ? 0.5 * (eh + ea) : 1.)) * (du * du);
                    }
                    if (aj.edge && !ai.dir && !ak.dir) {
                        const double du = u[p + aj.o] - uh;
                        double a = 1.;
                        if constexpr (COEF)
                            a = 0.5 * (eh + e[p + aj.o]);
                        acc += ((ai.w * ak.w) * a) * (du * du);
                    }
                    if (ak.edge && !ai.dir && !aj.dir) {
                        const double du = u[p + ak.o] - uh;
                        double a = 1.;
                        if constexpr (COEF)
                            a = 0.5 * (eh + e[p + ak.o]);
                        acc += ((ai.w * aj.w) * a) * (du * du);
                    }
                }
                /* the plane ahead in memory is i+1 unless the edge wrapped (i = N-2 of a periodic axis): then i+1 = N-1 is the
                 * duplicate plane, owned by nobody, and the walk ends there */
                uh = ua;
                eh = ea;
            }
        }
    }
    const double tot = block_sum_256(acc, lds4);
    if (threadIdx.x == 0 && threadIdx.y == 0)
        partials[(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = tot;
}

int k_field_energy(const Geom &g, const double *u, const LevelOperator &A, double *partials, double *out, hipStream_t s)
{
    if (g.N < 3 || g.ni != g.N || g.nj != g.N || g.nk != g.N)
        return -1;
    const int gx = (g.N + WAVE - 1) / WAVE, gy = (g.N + 3) / 4;
    int chunk = 16;
    while ((long long)gx * gy * ((g.N + chunk - 1) / chunk) > MG3D_MAX_PARTIALS)
        chunk *= 2;
    const dim3 grid(gx, gy, (g.N + chunk - 1) / chunk), block(WAVE, 4, 1);
    dispatch_op(A.e, A.bc, nullptr, [&](auto coef, auto mode, auto) {
        hipLaunchKernelGGL((field_energy_kernel<coef(), mode()>), grid, block, 0, s, g, u, A.e, partials, A.bc, chunk);
    });
    const int np = (int)(grid.x * grid.y * grid.z);
    k_fold(partials, np, out, s);
    return np;
}

/* ------------------------------------------------------- coarsest direct solve
 * solveWithLU, gauss_elim.h:31-60, on the banded factor.
 *   forward : z[i] = b[i] - sum_{j<i, ascending}  LU[i][j]*z[j]
 *   backward: x[i] = (z[i] - sum_{j>i, descending} LU[i][j]*x[j]) / LU[i][i]
 * Column-oriented: at step j the finished x[j] is broadcast and every row
 * inside the band adds its product.  Each row's sum therefore receives its
 * terms in exactly the reference's order (j ascending / descending), so the
 * result is bit-identical; only exact-zero factors outside the band are
 * skipped (adding +-0 never changes a sum that started from +0).
 *
 * One wave: lane l owns rows == l (mod 64); with bw <= 64*R a lane has at most
 * R rows in flight, their running sums live in registers, x[j] travels by
 * v_readlane.  No LDS traffic on the dependency chain, no barriers. */
#include "mg3d_lu_dev.h"

template <int R>
__global__ void __launch_bounds__(64) lu_solve_wave_kernel(LuBand lu, Geom g0, const double *__restrict__ b_pad,
                                                           double *__restrict__ x_pad)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int lane = threadIdx.x, n = lu.n;
    double *b = lds, *z = lds + n, *dg = lds + 2 * n; /* x overwrites b; dg = diagonal, then its reciprocals */
    const int NN = g0.nj * g0.nk;
    auto pad_of = [&](int p) -> long long {
        const int i = p / NN, rem = p - i * NN;
        const int j = rem / g0.nk, k = rem - j * g0.nk;
        return g0.plane * i + (long long)g0.pitch * j + k;
    };
    for (int p = lane; p < n; p += WAVE) {
        b[p] = b_pad[pad_of(p)];
        dg[p] = lu.diag[p];
        dg[n + p] = lu.diag[lu.npad + p];
    }
    __syncthreads();
    lu_wave_pass<R, true, false>(lu, lane, b, z, dg);
    __syncthreads();
    if (lu.fast_div)
        lu_wave_pass<R, false, true>(lu, lane, z, b, dg);
    else
        lu_wave_pass<R, false, false>(lu, lane, z, b, dg);
    __syncthreads();
    for (int p = lane; p < n; p += WAVE)
        x_pad[pad_of(p)] = b[p];
}

/* RI > 0: a reduced factor `lin` (the system without its identity rows, R = RI) exists beside the full one.  It is taken
 * when every identity row's right-hand side entry is +-0 -- then those unknowns are x = b and contribute +-0 to every
 * other row's running sums, which changes none of them (install_lu, mg3d_ctx.hip) -- else the full system. */
template <int R, int RI>
__global__ void __launch_bounds__(192) lu_solve_stream_kernel(LuBand lu, LuBand lin, Geom g0, const double *__restrict__ b_pad,
                                                             double *__restrict__ x_pad)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    constexpr int CD = 64 * 64 * R; /* doubles per chunk of the full system's ring (the reduced one's is not larger) */
    const int tid = threadIdx.x, lane = tid & 63, n = lu.n, npad = lu.npad;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double *ring = lds, *b = lds + 2 * CD, *z = b + npad, *dg = z + npad; /* x overwrites b; dg: diagonal, reciprocals */
    const int NN = g0.nj * g0.nk;
    auto pad_of = [&](int p) -> long long {
        const int i = p / NN, rem = p - i * NN;
        const int j = rem / g0.nk, k = rem - j * g0.nk;
        return g0.plane * i + (long long)g0.pitch * j + k;
    };
    int nonzero = 0;
    for (int p = tid; p < npad; p += 192) {
        const double v = p < n ? b_pad[pad_of(p)] : 0.;
        b[p] = v;
        if (RI > 0 && p < n)
            nonzero |= lu.in_map[p] < 0 && (__double_as_longlong(v) << 1) != 0ll;
    }
    if constexpr (RI > 0) {
        if (!__syncthreads_or(nonzero)) { /* workgroup-uniform */
            const int ni = lin.n, npi = lin.npad; /* 2 * npi <= npad (install_lu): both vectors fit into z's place */
            double *bi = z, *zi = z + npi;
            for (int p = tid; p < npi; p += 192) {
                bi[p] = 0.;
                dg[p] = lin.diag[p];
                dg[npi + p] = lin.diag[npi + p];
            }
            __syncthreads();
            for (int p = tid; p < n; p += 192) {
                const int q = lu.in_map[p];
                if (q >= 0)
                    bi[q] = b[p];
            }
            (void)ni;
            lu_stream_solve<RI>(lin, ring, bi, zi, dg, lane, wave);
            for (int p = tid; p < n; p += 192) {
                const int q = lu.in_map[p];
                x_pad[pad_of(p)] = q >= 0 ? bi[q] : b[p]; /* identity row: x = (b - (+0)) / 1 = b, the sign of a zero kept */
            }
            return;
        }
    }
    for (int p = tid; p < npad; p += 192) {
        dg[p] = lu.diag[p];
        dg[npad + p] = lu.diag[npad + p];
    }
    lu_stream_solve<R>(lu, ring, b, z, dg, lane, wave);
    for (int p = tid; p < n; p += 192)
        x_pad[pad_of(p)] = b[p];
}

static size_t lu_stream_lds(int npad, int R) { return sizeof(double) * (2 * (size_t)64 * 64 * R + 4 * (size_t)npad); }

int mg3d_lu_stream_chunk(int n, int R)
{
    if (R < 1 || R > 2)
        return 0;
    int dev = 0, max_lds = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess)
        return 0;
    return lu_stream_lds((n + 63) / 64 * 64, R) <= (size_t)max_lds ? 64 : 0;
}

template <int R, int RI>
static bool launch_lu_stream(const LuBand &lu, const LuBand &lin, const Geom &g0, const double *b_pad, double *x_pad,
                             hipStream_t s)
{
    const size_t lds = lu_stream_lds(lu.npad, R);
    /* a slot ring beyond 64 KB has to be asked for, per kernel and per device: exactly what is needed (the kernel's few
     * static bytes -- the workgroup vote -- count against the same 160 KB) */
    if (lds > 65536) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        static std::mutex mu;
        static std::map<int, size_t> granted; /* device -> bytes granted; 0 = refused */
        std::lock_guard<std::mutex> lock(mu);
        auto it = granted.find(dev);
        if (it == granted.end() || (it->second != 0 && it->second < lds)) {
            const bool ok = hipFuncSetAttribute(reinterpret_cast<const void *>(&lu_solve_stream_kernel<R, RI>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
            (void)hipGetLastError();
            granted[dev] = ok ? lds : 0;
            it = granted.find(dev);
        }
        if (it->second == 0)
            return false;
    }
    hipLaunchKernelGGL((lu_solve_stream_kernel<R, RI>), dim3(1), dim3(192), lds, s, lu, lin, g0, b_pad, x_pad);
    return true;
}

/* Generic fallback for wide bands (coarse grids beyond 9^3): one 1024-thread
 * block, running sums of the rows in flight kept in a global ring `acc[n]`,
 * one barrier per step.  Same per-row term order as above. */
__global__ void __launch_bounds__(1024) lu_solve_block_kernel(LuBand lu, Geom g0, const double *__restrict__ b_pad,
                                                              double *__restrict__ x_pad, double *__restrict__ z,
                                                              double *__restrict__ acc)
{
    const int n = lu.n, bw = lu.bw, tid = threadIdx.x;
    const int NN = g0.nj * g0.nk;
    auto pad_of = [&](int p) -> long long {
        const int i = p / NN, rem = p - i * NN;
        const int j = rem / g0.nk, k = rem - j * g0.nk;
        return g0.plane * i + (long long)g0.pitch * j + k;
    };
    __shared__ double bc;
    for (int i = tid; i < n; i += 1024)
        acc[i] = 0.;
    __syncthreads();
    for (int j = 0; j < n; j++) {
        if (tid == 0) {
            bc = b_pad[pad_of(j)] - acc[j];
            z[j] = bc;
        }
        __syncthreads();
        const double zj = bc;
        for (int t = tid; t < bw && j + 1 + t < n; t += 1024)
            acc[j + 1 + t] += lu.lcol[(long long)j * bw + t] * zj;
        __syncthreads();
    }
    for (int i = tid; i < n; i += 1024)
        acc[i] = 0.;
    __syncthreads();
    for (int j = n - 1; j >= 0; j--) {
        if (tid == 0) {
            bc = (z[j] - acc[j]) / lu.diag[j];
            x_pad[pad_of(j)] = bc;
        }
        __syncthreads();
        const double xj = bc;
        for (int t = tid; t < bw && j - 1 - t >= 0; t += 1024)
            acc[j - 1 - t] += lu.ucol[(long long)j * bw + t] * xj;
        __syncthreads();
    }
}

void k_lu_solve(const LuBand &lu, const LuBand &lu_in, const Geom &g0, const double *b_pad, double *x_pad, double *work,
                hipStream_t s)
{
    double *z = work, *acc = work + lu.n;
    const size_t lds = sizeof(double) * 4 * (size_t)lu.n;
    /* the reduced factor rides along when it exists (narrower band: one row per lane) */
    const bool red = lu.in_map && lu_in.n > 0 && lu_in.stream_ch == 64 && lu_in.rot_r == 1 && 2 * lu_in.npad <= lu.npad;
    if (lu.stream_ch == 64 && lu.rot_r == 2 && red && launch_lu_stream<2, 1>(lu, lu_in, g0, b_pad, x_pad, s))
        return;
    if (lu.stream_ch == 64 && lu.rot_r == 2 && launch_lu_stream<2, 0>(lu, lu, g0, b_pad, x_pad, s))
        return;
    if (lu.stream_ch == 64 && lu.rot_r == 1 && red && launch_lu_stream<1, 1>(lu, lu_in, g0, b_pad, x_pad, s))
        return;
    if (lu.stream_ch == 64 && lu.rot_r == 1 && launch_lu_stream<1, 0>(lu, lu, g0, b_pad, x_pad, s))
        return;
    if (lu.rot_r == 1)
        hipLaunchKernelGGL(lu_solve_wave_kernel<1>, dim3(1), dim3(64), lds, s, lu, g0, b_pad, x_pad);
    else if (lu.rot_r == 2)
        hipLaunchKernelGGL(lu_solve_wave_kernel<2>, dim3(1), dim3(64), lds, s, lu, g0, b_pad, x_pad);
    else
        hipLaunchKernelGGL(lu_solve_block_kernel, dim3(1), dim3(1024), 0, s, lu, g0, b_pad, x_pad, z, acc);
}
