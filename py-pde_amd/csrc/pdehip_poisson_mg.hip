// pdehip_poisson_mg.hip — the multigrid V-cycle that preconditions the conjugate gradients of the Poisson solver, and sweep 1 of the
// preconditioned loop (see pdehip_poisson_mg.h).  Kernels of a cycle on a level with `smooth` = 2:
//   poisson_mg_smooth0_kernel   the first TWO Jacobi sweeps from a zero guess in one pass: z1 = omega r / d is pointwise in r, so
//                               z2 = z1 + omega (r - (-A) z1) / d is a 7-point stencil on r with the diagonal taken from the position
//                               of every cell it touches (read r, write z; the ghost cells of r hold the homogeneous conditions)
//   poisson_mg_restrict_kernel  residual and restriction: a thread owns one coarse cell, forms r - (-A) z on its children and stores
//                               their mean; the fine residual is never stored
//   poisson_mg_coarse_kernel    the last level when it has <= 1024 cells: all its sweeps by ONE workgroup, the iterate in LDS
//   poisson_mg_prolong_kernel   z += the value of the parent cell
//   poisson_mg_sweep_kernel     one Jacobi sweep t = z + omega (r - (-A) z) / d (the post-sweeps; sweeps past the second elsewhere)
// Ghost cells of z come from launch_ghosts with the faces of the level.  All vectors fp64 in the ghost-padded layout of norm_grid.
#include "pdehip_poisson_mg.h"

#include <vector>

namespace pdehip {

// what a kernel knows of a level
struct MgDev : RowGrid {
    int ndim;
    int loc[3];            // the axis has local faces (they enter the diagonal); 0: periodic or not there
    double s[3];           // 1 / dx^2; 0 on axes the grid does not have
    double flo[3], fhi[3]; // factor1 of the lower / upper face
    const double *alo[3], *ahi[3];   // ... or its coefficient array (cells of the face in C order)
    double d0, wd0, omega; // diagonal of a cell that touches no face, omega / d0
};

struct MgLevel {
    pdehip_grid_t g;
    NGrid n;
    MgDev dev;
    pdehip_bc_face_t faces[2 * PDEHIP_MAX_DIM];
    double *r = nullptr, *z = nullptr, *t = nullptr;   // level 0: r is the residual of the loop, t the handle's w
    double *arr[2 * PDEHIP_MAX_DIM] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // averaged coefficient arrays (levels > 0)
    int half[3] = {0, 0, 0};   // normalised axes halved on the way to the next level
    long cells = 0;
};

constexpr int kMgCoarseCells = 1024;   // the last level runs in LDS up to this many cells (4 per thread of one workgroup)

struct PoissonMg {
    std::vector<MgLevel> lv;
    int smooth = 2, coarse_sweeps = 32;
    double omega = 0;
    size_t bytes = 0;
};

namespace {

// omega / d of cell (i, j, k): the exact diagonal of -A from the position; cells that touch no face skip the division
__device__ __forceinline__ double mg_wd(const MgDev &L, long i, long j, long k)
{
    double d = L.d0;
    if (L.loc[0]) {
        if (i == 0) d = d - L.s[0] * (L.alo[0] ? L.alo[0][j * L.n2 + k] : L.flo[0]);
        if (i == L.n0 - 1) d = d - L.s[0] * (L.ahi[0] ? L.ahi[0][j * L.n2 + k] : L.fhi[0]);
    }
    if (L.loc[1]) {
        if (j == 0) d = d - L.s[1] * (L.alo[1] ? L.alo[1][i * L.n2 + k] : L.flo[1]);
        if (j == L.n1 - 1) d = d - L.s[1] * (L.ahi[1] ? L.ahi[1][i * L.n2 + k] : L.fhi[1]);
    }
    if (L.loc[2]) {
        if (k == 0) d = d - L.s[2] * (L.alo[2] ? L.alo[2][i * L.n1 + j] : L.flo[2]);
        if (k == L.n2 - 1) d = d - L.s[2] * (L.ahi[2] ? L.ahi[2][i * L.n1 + j] : L.fhi[2]);
    }
    if (d == L.d0) return L.wd0;
    return d > 0 ? L.omega / d : 0.0;
}
// the cell whose diagonal a ghost cell next to (.., c, ..) takes: the adjacent one (ghost = f * adjacent) or the other end (periodic)
__device__ __forceinline__ long mg_below(long c, long n, int loc) { return c > 0 ? c - 1 : (loc ? 0 : n - 1); }
__device__ __forceinline__ long mg_above(long c, long n, int loc) { return c < n - 1 ? c + 1 : (loc ? n - 1 : 0); }

// The first sweep(s) from z = 0.  two == 0: z = omega r / d.  two != 0: the second sweep in the same pass.  z1 of a ghost cell is
// omega r_ghost / d of the cell the ghost cell copies, because r_ghost = f r_adjacent (or the periodic image) is already in memory.
template <int VEC>
__global__ void __launch_bounds__(256) poisson_mg_smooth0_kernel(MgDev L, int two, const double *r, double *z, const PoissonCtl *ctl)
{
    if (ctl_stopped(ctl->head)) return;   // uniform
    typedef double V __attribute__((ext_vector_type(VEC)));
    for_row_pieces<VEC>(L, [&](long i, long j, long k, long e) {
        const V c = *(const V *)(r + e);
        V wd, z1, out;
#pragma unroll
        for (int m = 0; m < VEC; m++) {
            wd[m] = mg_wd(L, i, j, k + m);
            z1[m] = wd[m] * c[m];
        }
        if (!two) {
            *(V *)(z + e) = z1;
            return;
        }
        const double left = mg_wd(L, i, j, mg_below(k, L.n2, L.loc[2])) * r[e - 1];
        const double right = mg_wd(L, i, j, mg_above(k + VEC - 1, L.n2, L.loc[2])) * r[e + VEC];
        V up, dn, xm, xp;
        if (L.ndim >= 2) {
            const V ru = *(const V *)(r + e - L.p1), rd = *(const V *)(r + e + L.p1);
            const long jm = mg_below(j, L.n1, L.loc[1]), jp = mg_above(j, L.n1, L.loc[1]);
#pragma unroll
            for (int m = 0; m < VEC; m++) {
                up[m] = mg_wd(L, i, jm, k + m) * ru[m];
                dn[m] = mg_wd(L, i, jp, k + m) * rd[m];
            }
        }
        if (L.ndim == 3) {
            const V ru = *(const V *)(r + e - L.p0), rd = *(const V *)(r + e + L.p0);
            const long im = mg_below(i, L.n0, L.loc[0]), ip = mg_above(i, L.n0, L.loc[0]);
#pragma unroll
            for (int m = 0; m < VEC; m++) {
                xm[m] = mg_wd(L, im, j, k + m) * ru[m];
                xp[m] = mg_wd(L, ip, j, k + m) * rd[m];
            }
        }
#pragma unroll
        for (int m = 0; m < VEC; m++) {
            const double cen = z1[m], vm = 2 * cen;
            const double zl = (m == 0) ? left : (double)z1[m > 0 ? m - 1 : 0], zr = (m == VEC - 1) ? right : (double)z1[m < VEC - 1 ? m + 1 : m];
            double az = (vm - zl - zr) * L.s[2];
            if (L.ndim >= 2) az = az + (vm - up[m] - dn[m]) * L.s[1];
            if (L.ndim == 3) az = az + (vm - xm[m] - xp[m]) * L.s[0];
            out[m] = cen + wd[m] * (c[m] - az);
        }
        *(V *)(z + e) = out;
    });
}

// (-A) z of VEC cells of a row; the ghost cells of z are in memory
template <int VEC, typename V>
__device__ __forceinline__ V mg_minus_a(const MgDev &L, const double *z, long e, const V &c)
{
    const double left = z[e - 1], right = z[e + VEC];
    V up, dn, xm, xp, az;
    if (L.ndim >= 2) { up = *(const V *)(z + e - L.p1); dn = *(const V *)(z + e + L.p1); }
    if (L.ndim == 3) { xm = *(const V *)(z + e - L.p0); xp = *(const V *)(z + e + L.p0); }
#pragma unroll
    for (int m = 0; m < VEC; m++) {
        const double vm = 2 * c[m];
        const double zl = (m == 0) ? left : (double)c[m > 0 ? m - 1 : 0], zr = (m == VEC - 1) ? right : (double)c[m < VEC - 1 ? m + 1 : m];
        double a = (vm - zl - zr) * L.s[2];
        if (L.ndim >= 2) a = a + (vm - up[m] - dn[m]) * L.s[1];
        if (L.ndim == 3) a = a + (vm - xm[m] - xp[m]) * L.s[0];
        az[m] = a;
    }
    return az;
}

// one Jacobi sweep: out = z + omega (r - (-A) z) / d
template <int VEC>
__global__ void __launch_bounds__(256) poisson_mg_sweep_kernel(MgDev L, const double *r, const double *z, double *out, const PoissonCtl *ctl)
{
    if (ctl_stopped(ctl->head)) return;   // uniform
    typedef double V __attribute__((ext_vector_type(VEC)));
    for_row_pieces<VEC>(L, [&](long i, long j, long k, long e) {
        const V c = *(const V *)(z + e), rv = *(const V *)(r + e);
        const V az = mg_minus_a<VEC, V>(L, z, e, c);
        V o;
#pragma unroll
        for (int m = 0; m < VEC; m++) o[m] = c[m] + mg_wd(L, i, j, k + m) * (rv[m] - az[m]);
        *(V *)(out + e) = o;
    });
}

// residual and restriction: rc(coarse cell) = mean over its children of r - (-A) z.  HZ = children along the fastest axis (2: one
// 16-byte access per row of children); h0, h1 = children along the two other axes.  Sum in a fixed order.
template <int HZ>
__global__ void __launch_bounds__(256) poisson_mg_restrict_kernel(MgDev L, MgDev C, int h0, int h1, const double *r, const double *z, double *rc, const PoissonCtl *ctl)
{
    if (ctl_stopped(ctl->head)) return;   // uniform
    typedef double V __attribute__((ext_vector_type(HZ)));
    const double scale = 1.0 / (double)(h0 * h1 * HZ);
    for_row_pieces<1>(C, [&](long ic, long jc, long kc, long ec) {
        double sum = 0;
        for (int a = 0; a < h0; a++)
            for (int b = 0; b < h1; b++) {
                const long e = L.off + (ic * h0 + a) * L.p0 + (jc * h1 + b) * L.p1 + kc * HZ;
                const V c = *(const V *)(z + e), rv = *(const V *)(r + e);
                const V az = mg_minus_a<HZ, V>(L, z, e, c);
#pragma unroll
                for (int m = 0; m < HZ; m++) sum = sum + (rv[m] - az[m]);
            }
        rc[ec] = sum * scale;
    });
}

// prolongation and correction: z += zc(parent); sh = 1 on the halved axes
template <int VEC>
__global__ void __launch_bounds__(256) poisson_mg_prolong_kernel(MgDev L, MgDev C, int sh0, int sh1, int sh2, const double *zc, double *z, const PoissonCtl *ctl)
{
    if (ctl_stopped(ctl->head)) return;   // uniform
    typedef double V __attribute__((ext_vector_type(VEC)));
    for_row_pieces<VEC>(L, [&](long i, long j, long k, long e) {
        const long ec = C.off + (i >> sh0) * C.p0 + (j >> sh1) * C.p1;
        V v = *(const V *)(z + e);
#pragma unroll
        for (int m = 0; m < VEC; m++) v[m] = v[m] + zc[ec + ((k + m) >> sh2)];
        *(V *)(z + e) = v;
    });
}

// The last level in ONE workgroup: `sweeps` Jacobi sweeps from zero with the iterate in LDS (compact: cells, then one slot that stays
// zero).  A thread owns up to four cells and keeps their omega r / d, omega / d and the LDS slots of their six neighbours; a
// neighbour beyond a local face is the zero slot (the face is in the diagonal), one beyond a periodic end the cell at the other end:
// z' = z + (omega / d) (r - d z + sum s_a (z_lower + z_upper)) = omega r / d + (1 - omega) z + (omega / d) sum s_a (z_lower + z_upper).
__global__ void __launch_bounds__(256) poisson_mg_coarse_kernel(MgDev L, int sweeps, const double *r, double *z, const PoissonCtl *ctl)
{
    if (ctl_stopped(ctl->head)) return;   // uniform
    __shared__ double buf[2][kMgCoarseCells + 1];
    const int cells = (int)(L.n0 * L.n1 * L.n2);
    constexpr int CPT = kMgCoarseCells / 256;
    double c0[CPT], wd[CPT];
    int nb[CPT][6];
    long at[CPT];
#pragma unroll
    for (int m = 0; m < CPT; m++) {
        const int c = (int)threadIdx.x + 256 * m;
        c0[m] = 0; wd[m] = 0; at[m] = 0;
#pragma unroll
        for (int q = 0; q < 6; q++) nb[m][q] = cells;
        if (c < cells) {
            const long k = c % L.n2, j = (c / L.n2) % L.n1, i = c / (L.n2 * L.n1);
            at[m] = L.off + i * L.p0 + j * L.p1 + k;
            wd[m] = mg_wd(L, i, j, k);
            c0[m] = wd[m] * r[at[m]];
            const long st0 = L.n1 * L.n2, st1 = L.n2;
            if (L.ndim == 3) {
                if (i > 0) nb[m][0] = c - (int)st0; else if (!L.loc[0]) nb[m][0] = c + (int)((L.n0 - 1) * st0);
                if (i < L.n0 - 1) nb[m][1] = c + (int)st0; else if (!L.loc[0]) nb[m][1] = c - (int)((L.n0 - 1) * st0);
            }
            if (L.ndim >= 2) {
                if (j > 0) nb[m][2] = c - (int)st1; else if (!L.loc[1]) nb[m][2] = c + (int)((L.n1 - 1) * st1);
                if (j < L.n1 - 1) nb[m][3] = c + (int)st1; else if (!L.loc[1]) nb[m][3] = c - (int)((L.n1 - 1) * st1);
            }
            if (k > 0) nb[m][4] = c - 1; else if (!L.loc[2]) nb[m][4] = c + (int)(L.n2 - 1);
            if (k < L.n2 - 1) nb[m][5] = c + 1; else if (!L.loc[2]) nb[m][5] = c - (int)(L.n2 - 1);
        }
    }
#pragma unroll
    for (int m = 0; m < CPT; m++) {
        const int c = (int)threadIdx.x + 256 * m;
        if (c < cells) buf[0][c] = c0[m];
    }
    if (threadIdx.x == 0) { buf[0][cells] = 0; buf[1][cells] = 0; }
    __syncthreads();
    int cur = 0;
    const double keep = 1.0 - L.omega;
    for (int s = 1; s < sweeps; s++) {
#pragma unroll
        for (int m = 0; m < CPT; m++) {
            const int c = (int)threadIdx.x + 256 * m;
            if (c < cells) {
                const double *b = buf[cur];
                const double nbs = (b[nb[m][0]] + b[nb[m][1]]) * L.s[0] + (b[nb[m][2]] + b[nb[m][3]]) * L.s[1] + (b[nb[m][4]] + b[nb[m][5]]) * L.s[2];
                buf[1 - cur][c] = c0[m] + keep * b[c] + wd[m] * nbs;
            }
        }
        cur = 1 - cur;
        __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < CPT; m++) {
        const int c = (int)threadIdx.x + 256 * m;
        if (c < cells) z[at[m]] = buf[cur][c];
    }
}

// a coefficient array of a face, averaged over the children of every coarse face cell
__global__ void __launch_bounds__(256) poisson_mg_face_kernel(const double *fine, double *coarse, long m1c, long m2c, int h1, int h2, long m2f)
{
    const long total = m1c * m2c;
    for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const long u = t / m2c, v = t % m2c;
        double s = 0;
        for (int a = 0; a < h1; a++)
            for (int b = 0; b < h2; b++) s = s + fine[(u * h1 + a) * m2f + v * h2 + b];
        coarse[t] = s / (double)(h1 * h2);
    }
}

// sweep 1 of the preconditioned loop: w = -A z and the wave's shares of r.z, z.w and r.r
template <int VEC>
__global__ void __launch_bounds__(256) poisson_mg_apply_kernel(MgDev L, const double *z, const double *r, double *w, PoissonCtl *ctl)
{
    if (ctl_stopped(ctl->head)) return;   // uniform
    ctl_announce(ctl->head, (long)gridDim.x * (blockDim.x >> 6));
    typedef double V __attribute__((ext_vector_type(VEC)));
    double s_rz = 0, s_zw = 0, s_rr = 0;
    for_row_pieces<VEC>(L, [&](long, long, long, long e) {
        const V c = *(const V *)(z + e), rv = *(const V *)(r + e);
        const V az = mg_minus_a<VEC, V>(L, z, e, c);
#pragma unroll
        for (int m = 0; m < VEC; m++) {
            s_rz = s_rz + rv[m] * c[m];
            s_zw = s_zw + c[m] * az[m];
            s_rr = s_rr + rv[m] * rv[m];
        }
        *(V *)(w + e) = az;
    });
    wave_partials<3>(poisson_slots(ctl), {s_rz, s_zw, s_rr}, wave_slot(), ctl->head.capacity);
}

// the stop word of a solve that is over would switch a lone application of the cycle off
__global__ void poisson_mg_open_kernel(PoissonCtl *c) { c->head.stop = 0; }

int mg_ghosts(const MgLevel &L, double *v, void *st) { return launch_ghosts(L.n, 1, L.faces, v, as_stream(st)); }

// `count` Jacobi sweeps from zero; the result is L.z
int mg_from_zero(PoissonHandle *h, MgLevel &L, int count, void *st)
{
    const bool even = L.n.n[2] % 2 == 0;
    const int two = count >= 2 ? 1 : 0;
    if (two) PDEHIP_TRY(mg_ghosts(L, L.r, st));
    PDEHIP_LAUNCH_ROWS(even, L.cells, st, poisson_mg_smooth0_kernel<VEC>, L.dev, two, L.r, L.z, h->ctl);
    for (int s = two ? 2 : 1; s < count; s++) {
        PDEHIP_TRY(mg_ghosts(L, L.z, st));
        PDEHIP_LAUNCH_ROWS(even, L.cells, st, poisson_mg_sweep_kernel<VEC>, L.dev, L.r, L.z, L.t, h->ctl);
        double *sw = L.z; L.z = L.t; L.t = sw;
    }
    return 0;
}

int mg_cycle(PoissonHandle *h, size_t l, void *st)
{
    PoissonMg *mg = h->mg;
    MgLevel &L = mg->lv[l];
    const bool even = L.n.n[2] % 2 == 0;
    if (l + 1 == mg->lv.size()) {
        if (L.cells <= kMgCoarseCells) {
            hipLaunchKernelGGL(poisson_mg_coarse_kernel, dim3(1), dim3(256), 0, as_stream(st), L.dev, mg->coarse_sweeps, L.r, L.z, h->ctl);
            PDEHIP_HIP(hipGetLastError());
            return 0;
        }
        return mg_from_zero(h, L, mg->coarse_sweeps, st);   // a grid that does not coarsen far enough: the sweeps one by one
    }
    MgLevel &C = mg->lv[l + 1];
    PDEHIP_TRY(mg_from_zero(h, L, mg->smooth, st));
    PDEHIP_TRY(mg_ghosts(L, L.z, st));
    const int h0 = L.half[0] ? 2 : 1, h1 = L.half[1] ? 2 : 1;
    if (L.half[2]) hipLaunchKernelGGL((poisson_mg_restrict_kernel<2>), dim3(blocks_for(C.cells)), dim3(256), 0, as_stream(st), L.dev, C.dev, h0, h1, L.r, L.z, C.r, h->ctl);
    else hipLaunchKernelGGL((poisson_mg_restrict_kernel<1>), dim3(blocks_for(C.cells)), dim3(256), 0, as_stream(st), L.dev, C.dev, h0, h1, L.r, L.z, C.r, h->ctl);
    PDEHIP_HIP(hipGetLastError());
    PDEHIP_TRY(mg_cycle(h, l + 1, st));
    PDEHIP_LAUNCH_ROWS(even, L.cells, st, poisson_mg_prolong_kernel<VEC>, L.dev, C.dev, L.half[0], L.half[1], L.half[2], C.z, L.z, h->ctl);
    for (int s = 0; s < mg->smooth; s++) {
        PDEHIP_TRY(mg_ghosts(L, L.z, st));
        PDEHIP_LAUNCH_ROWS(even, L.cells, st, poisson_mg_sweep_kernel<VEC>, L.dev, L.r, L.z, L.t, h->ctl);
        double *sw = L.z; L.z = L.t; L.t = sw;
    }
    return 0;
}

// z = M r on level 0 (r = the handle's r).  The sweeps alternate between the level's z and the handle's w, which holds nothing
// between two iterations: whichever of the two buffers the result is not in is w afterwards.
int mg_precondition(PoissonHandle *h, void *st)
{
    MgLevel &L = h->mg->lv[0];
    L.r = h->r;
    L.t = h->w;
    PDEHIP_TRY(mg_cycle(h, 0, st));
    h->w = L.t;
    return 0;
}

void fill_dev(MgLevel &L, double omega)
{
    MgDev &d = L.dev;
    const NGrid &n = L.n;
    memset(&d, 0, sizeof(d));
    static_cast<RowGrid &>(d) = make_row_grid(n);
    d.ndim = n.ndim;
    d.omega = omega;
    double d0 = 0;
    for (int ar = 0; ar < n.ndim; ar++) {
        const int ax = 3 - n.ndim + ar;
        const pdehip_bc_face_t &lo = L.faces[2 * ar], &hi = L.faces[2 * ar + 1];
        d.s[ax] = n.lap_scale[ax];
        d0 += 2 * d.s[ax];
        const bool periodic = n.n[ax] > 1 && lo.index1 == n.n[ax] - 1;
        d.loc[ax] = periodic ? 0 : 1;
        d.flo[ax] = lo.factor1; d.fhi[ax] = hi.factor1;
        d.alo[ax] = (lo.flags & PDEHIP_BCF_ARRAYS) ? lo.factor1_arr : nullptr;
        d.ahi[ax] = (hi.flags & PDEHIP_BCF_ARRAYS) ? hi.factor1_arr : nullptr;
    }
    d.d0 = d0;
    d.wd0 = d0 > 0 ? omega / d0 : 0.0;
}

}  // namespace

void poisson_mg_release(PoissonHandle *h)
{
    if (!h || !h->mg) return;
    PoissonMg *mg = h->mg;
    for (size_t l = 0; l < mg->lv.size(); l++) {
        MgLevel &L = mg->lv[l];
        if (l > 0) {
            if (L.r) (void)hipFree(L.r);
            if (L.t) (void)hipFree(L.t);
        }
        // (level 0: r and t are the handle's; its z is one of the two buffers the cycle alternates between - the other one is h->w)
        if (L.z) (void)hipFree(L.z);
        for (double *a : L.arr)
            if (a) (void)hipFree(a);
    }
    delete mg;
    h->mg = nullptr;
}

int poisson_mg_set(PoissonHandle *h, pdehip_poisson_mg_t *o)
{
    poisson_mg_release(h);
    if (!o) return 0;
    if (o->smooth < 0 || o->coarse_sweeps < 0 || o->max_levels < 0 || !(o->omega >= 0) || o->omega >= 2) PDEHIP_FAIL(E_VALUE, "poisson_set_multigrid: bad smooth / coarse_sweeps / max_levels / omega");
    PoissonMg *mg = new PoissonMg();
    h->mg = mg;
    const NGrid &n0 = h->n64;
    mg->smooth = o->smooth ? o->smooth : 2;
    mg->coarse_sweeps = o->coarse_sweeps ? o->coarse_sweeps : 32;
    mg->omega = o->omega > 0 ? o->omega : 2.0 * n0.ndim / (2.0 * n0.ndim + 1.0);
    size_t bytes = 0;
    hipError_t e = hipSuccess;
    auto alloc = [&](double **p, size_t count) {
        if (e == hipSuccess) e = hipMalloc((void **)p, count * sizeof(double));
        if (e == hipSuccess) e = hipMemset(*p, 0, count * sizeof(double));
        if (e == hipSuccess) bytes += count * sizeof(double);
    };
    // level 0: the grid of the work vectors and the homogeneous faces of the handle
    {
        MgLevel L;
        L.g = h->g64;
        L.n = n0;
        memcpy(L.faces, h->faces_a, sizeof(L.faces));
        mg->lv.push_back(L);
    }
    while (true) {
        MgLevel &F = mg->lv.back();
        F.cells = F.n.n[0] * F.n.n[1] * F.n.n[2];
        fill_dev(F, mg->omega);
        if (F.cells <= 512 || (o->max_levels > 0 && (int)mg->lv.size() >= o->max_levels) || (int)mg->lv.size() >= PDEHIP_MG_MAX_LEVELS) break;
        bool any = false;
        MgLevel C;
        C.g = F.g;
        for (int ar = 0; ar < F.n.ndim; ar++) {
            const int ax = 3 - F.n.ndim + ar;
            if (F.g.shape[ar] >= 4 && F.g.shape[ar] % 2 == 0) {
                F.half[ax] = 1;
                C.g.shape[ar] = F.g.shape[ar] / 2;
                C.g.dx[ar] = F.g.dx[ar] * 2;
                any = true;
            }
        }
        if (!any) break;
        int rc = norm_grid(&C.g, &C.n);
        if (rc) { poisson_mg_release(h); return rc; }
        // the same homogeneous faces one level down; coefficient arrays averaged over the children of each coarse face cell
        for (int ar = 0; ar < F.n.ndim && e == hipSuccess; ar++) {
            const int ax = 3 - F.n.ndim + ar;
            const int o1 = (ax == 0) ? 1 : 0, o2 = (ax == 2) ? 1 : 2;
            for (int side = 0; side < 2; side++) {
                const int q = 2 * ar + side;
                const pdehip_bc_face_t &ff = F.faces[q];
                pdehip_bc_face_t &cf = C.faces[q];
                cf = ff;
                const long lf = F.n.n[ax], lc = C.n.n[ax];
                const long adjacent_f = side ? lf - 1 : 0;
                const bool local = ff.index1 == adjacent_f;
                cf.index1 = local ? (side ? lc - 1 : 0) : (side ? 0 : lc - 1);
                if (ff.flags & PDEHIP_BCF_ARRAYS) {
                    const long m1c = C.n.n[o1], m2c = C.n.n[o2];
                    alloc(&C.arr[q], (size_t)(m1c * m2c));
                    if (e != hipSuccess) break;
                    hipLaunchKernelGGL(poisson_mg_face_kernel, dim3(blocks_for(m1c * m2c)), dim3(256), 0, 0, ff.factor1_arr, C.arr[q], m1c, m2c, F.half[o1] ? 2 : 1, F.half[o2] ? 2 : 1, F.n.n[o2]);
                    if (e == hipSuccess) e = hipGetLastError();
                    cf.factor1_arr = C.arr[q];
                }
            }
        }
        if (e != hipSuccess) break;
        const size_t count = (size_t)(C.n.pc + kAllocSlack);
        alloc(&C.r, count);
        alloc(&C.z, count);
        alloc(&C.t, count);
        mg->lv.push_back(C);
        if (e != hipSuccess) break;
    }
    alloc(&mg->lv[0].z, (size_t)(n0.pc + kAllocSlack));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        poisson_mg_release(h);
        PDEHIP_FAIL(100 + (int)e, "poisson_set_multigrid: %s", hipGetErrorString(e));
    }
    mg->bytes = bytes;
    o->smooth = mg->smooth;
    o->coarse_sweeps = mg->coarse_sweeps;
    o->omega = mg->omega;
    o->levels = (int32_t)mg->lv.size();
    o->bytes = (uint64_t)bytes;
    memset(o->shapes, 0, sizeof(o->shapes));
    for (size_t l = 0; l < mg->lv.size(); l++)
        for (int ar = 0; ar < n0.ndim; ar++) o->shapes[l][ar] = mg->lv[l].g.shape[ar];
    return 0;
}

int poisson_mg_sweep1(PoissonHandle *h, const double **z, void *st)
{
    PDEHIP_TRY(mg_precondition(h, st));
    MgLevel &L = h->mg->lv[0];
    PDEHIP_TRY(mg_ghosts(L, L.z, st));
    PDEHIP_LAUNCH_ROWS(L.n.n[2] % 2 == 0, L.cells, st, poisson_mg_apply_kernel<VEC>, L.dev, L.z, h->r, h->w, h->ctl);
    *z = L.z;
    return 0;
}

void poisson_mg_note(const PoissonHandle *h)
{
    note_kernel("poisson_mg_apply_kernel<%d> (w = -A z with the wave sums of r.z, z.w and r.r in the sweep; z = M r by a V-cycle over %d levels)",
                h->n64.n[2] % 2 == 0 ? 2 : 1, (int)h->mg->lv.size());
}

}  // namespace pdehip

using namespace pdehip;

extern "C" {

int pdehip_poisson_set_multigrid(void *handle, pdehip_poisson_mg_t *opts)
{
    PoissonHandle *h = (PoissonHandle *)handle;
    if (!h) PDEHIP_FAIL(E_VALUE, "poisson_set_multigrid: NULL pointer");
    return poisson_mg_set(h, opts);
}

int pdehip_poisson_precondition(void *handle, const void *r_full, void *z_full, void *stream)
{
    PoissonHandle *h = (PoissonHandle *)handle;
    if (!h || !r_full || !z_full) PDEHIP_FAIL(E_VALUE, "poisson_precondition: NULL pointer");
    if (!h->mg) PDEHIP_FAIL(E_VALUE, "poisson_precondition: the handle has no hierarchy (pdehip_poisson_set_multigrid)");
    hipStream_t s = as_stream(stream);
    const size_t bytes = (size_t)h->n64.pc * sizeof(double);
    PDEHIP_HIP(hipMemcpyAsync(h->r, r_full, bytes, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(poisson_mg_open_kernel, dim3(1), dim3(1), 0, s, h->ctl);
    PDEHIP_HIP(hipGetLastError());
    PDEHIP_TRY(mg_precondition(h, stream));
    PDEHIP_HIP(hipMemcpyAsync(z_full, h->mg->lv[0].z, bytes, hipMemcpyDeviceToDevice, s));
    return 0;
}

}  // extern "C"
