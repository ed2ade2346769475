// pdehip_interp.hip — linear interpolation of fields on the device: arbitrary points (probes), the cell centres of another
// Cartesian grid (regridding), and the edge / corner ghost cells such points read next to two or three walls.
//
// Semantics: pde/backends/numba/grids.py:102-190 (make_interpolation_axis_data) and :193-347 (make_single_interpolator), operation
// by operation; pde/grids/boundaries/axes.py:475-495 for the corners.  Weights and sums are fp64 whatever the field's type (numba
// promotes the float32 element against the float64 weight), rounded once at the store; -ffp-contract=off keeps the term order.
#include "pdehip_common.h"

namespace pdehip {
namespace {

struct InterpAxis {
    long size, pitch;      // valid cells and pitch (elements) of the SOURCE axis
    double lo, dx;         // grid.axes_bounds[axis][0], grid.discretization[axis]
    int periodic;
};
struct InterpArgs {
    InterpAxis ax[3];      // grid order; entries >= NDIM unused
    int ghost, ncomp;      // with_ghost_cells, components (planar pairs of complex data count twice)
    long pc, off;          // component pitch and offset of interior cell (0,0,0) of the source
    long npoints;
};

// support cells as VALID indices (-1 / size = the ghost cells) and weights of one coordinate
struct AxisData {
    long cl, ch;
    double wl, wh;
    int ok;
};

__device__ inline AxisData axis_data(double coord, const InterpAxis &x, int ghost)
{
    AxisData r;
    r.cl = r.ch = 0; r.wl = r.wh = 0.0; r.ok = 1;
    // c_l, d_l = divmod((coord - lo) / dx - 0.5, 1.0)   grids.py:142, by the rule of CPython's float divmod (floatobject.c: fmod, then the
    // sign fix-up - a tiny negative quotient gives (-1.0, 1.0), where floor alone would give (-1.0, ~1.0 - 1e-17 -> 1.0) by luck only)
    const double vx = (coord - x.lo) / x.dx - 0.5;
    double mod = fmod(vx, 1.0);
    double div = (vx - mod) / 1.0;
    if (mod != 0.0) {
        if (mod < 0.0) { mod += 1.0; div -= 1.0; }
    } else {
        mod = 0.0;
    }
    double c_l;
    if (div != 0.0) {
        c_l = floor(div);
        if (div - c_l > 0.5) c_l += 1.0;
    } else {
        c_l = copysign(0.0, vx / 1.0);
    }
    const double d_l = mod;
    const double q = c_l + d_l;
    const double size = (double)x.size;
    if (x.periodic) {                                  // grids.py:145-148
        if (!(fabs(c_l) <= 1.7976931348623157e308)) { r.ok = 0; return r; }     // (int(nan) / int(inf) raise in the reference)
        double m = fmod(c_l, size);
        if (m < 0.0) m += size;                        // Python's %: the sign of the divisor
        r.cl = (long)m;
        r.ch = (r.cl + 1) % x.size;
    } else if (ghost) {                                // grids.py:150-156
        if (-0.5 <= q && q <= size - 0.5) {
            r.cl = (long)c_l;
            r.ch = r.cl + 1;
        } else { r.ok = 0; return r; }
    } else {                                           // grids.py:158-170
        if (0.0 <= q && q < size - 1.0) {
            r.cl = (long)c_l;
            r.ch = r.cl + 1;
        } else if (size - 1.0 <= q && q <= size - 0.5) {
            r.cl = r.ch = (long)c_l;
        } else if (-0.5 <= q && q <= 0.0) {
            r.cl = r.ch = (long)c_l + 1;
        } else { r.ok = 0; return r; }
        if (r.cl < 0) r.cl += x.size;                  // data[..., -1]: (-1.0, 1.0) from the fix-up reads the last cell, with weight 0
        if (r.ch < 0) r.ch += x.size;
    }
    r.wl = 1.0 - d_l;                                  // grids.py:173-181
    r.wh = d_l;
    if (r.wl < 1e-15) r.wl = 0.0;
    if (r.wh < 1e-15) r.wh = 0.0;
    // nothing above can leave the array; a support cell outside it would be a bug here, never a read
    const long first = (ghost && !x.periodic) ? -1 : 0, last = (ghost && !x.periodic) ? x.size : x.size - 1;
    if (r.cl < first || r.cl > last || r.ch < first || r.ch > last) r.ok = 0;
    return r;
}

// the 2 / 4 / 8 term sums of grids.py:259, :293-298, :334-343 (left to right)
template <typename T>
__device__ inline double sum1(const T *d, const AxisData &X, long px)
{
    return X.wl * (double)d[X.cl * px] + X.wh * (double)d[X.ch * px];
}
template <typename T>
__device__ inline double sum2(const T *d, const AxisData &X, const AxisData &Y, long px, long py)
{
    return X.wl * Y.wl * (double)d[X.cl * px + Y.cl * py] + X.wl * Y.wh * (double)d[X.cl * px + Y.ch * py] +
           X.wh * Y.wl * (double)d[X.ch * px + Y.cl * py] + X.wh * Y.wh * (double)d[X.ch * px + Y.ch * py];
}
template <typename T>
__device__ inline double sum3(const T *d, const AxisData &X, const AxisData &Y, const AxisData &Z, long px, long py, long pz)
{
    return X.wl * Y.wl * Z.wl * (double)d[X.cl * px + Y.cl * py + Z.cl * pz] + X.wl * Y.wl * Z.wh * (double)d[X.cl * px + Y.cl * py + Z.ch * pz] +
           X.wl * Y.wh * Z.wl * (double)d[X.cl * px + Y.ch * py + Z.cl * pz] + X.wl * Y.wh * Z.wh * (double)d[X.cl * px + Y.ch * py + Z.ch * pz] +
           X.wh * Y.wl * Z.wl * (double)d[X.ch * px + Y.cl * py + Z.cl * pz] + X.wh * Y.wl * Z.wh * (double)d[X.ch * px + Y.cl * py + Z.ch * pz] +
           X.wh * Y.wh * Z.wl * (double)d[X.ch * px + Y.ch * py + Z.cl * pz] + X.wh * Y.wh * Z.wh * (double)d[X.ch * px + Y.ch * py + Z.ch * pz];
}

// ---- arbitrary points: one thread per point, all components; out is (ncomp, npoints) -------------------------------------------
template <typename T, int NDIM>
__global__ void __launch_bounds__(256) interp_points_kernel(InterpArgs a, const T *__restrict__ data, const double *__restrict__ pts,
                                                            const double *__restrict__ fill, T *__restrict__ out, unsigned long long *oob)
{
    unsigned long long bad = 0;
    for (long p = blockIdx.x * (long)blockDim.x + threadIdx.x; p < a.npoints; p += (long)gridDim.x * blockDim.x) {
        const AxisData X = axis_data(pts[p * NDIM], a.ax[0], a.ghost);
        AxisData Y = X, Z = X;
        int ok = X.ok;
        if (NDIM >= 2) { Y = axis_data(pts[p * NDIM + 1], a.ax[1], a.ghost); ok &= Y.ok; }
        if (NDIM >= 3) { Z = axis_data(pts[p * NDIM + 2], a.ax[2], a.ghost); ok &= Z.ok; }
        if (!ok) {                                     // grids.py:251-256: the fill value, or the host raises DomainError
            if (fill) {
                for (int c = 0; c < a.ncomp; c++) out[c * a.npoints + p] = (T)fill[c];
            } else {
                bad++;
            }
            continue;
        }
        const T *d = data + a.off;
        for (int c = 0; c < a.ncomp; c++, d += a.pc) {
            double v;
            if (NDIM == 1) v = sum1(d, X, a.ax[0].pitch);
            else if (NDIM == 2) v = sum2(d, X, Y, a.ax[0].pitch, a.ax[1].pitch);
            else v = sum3(d, X, Y, Z, a.ax[0].pitch, a.ax[1].pitch, a.ax[2].pitch);
            out[c * a.npoints + p] = (T)v;
        }
    }
    if (bad) atomicAdd(oob, bad);
}

// ---- regridding: per-axis tables, then rows of the target ------------------------------------------------------------------------
struct AxisTables {
    long *cl, *ch;
    double *wl, *wh;
    int *ok;
};
inline AxisTables split_tables(void *tables, long total)
{
    AxisTables t;
    char *p = (char *)tables;
    t.cl = (long *)p; p += 8 * total;
    t.ch = (long *)p; p += 8 * total;
    t.wl = (double *)p; p += 8 * total;
    t.wh = (double *)p; p += 8 * total;
    t.ok = (int *)p;
    return t;
}

struct RegridArgs {
    InterpArgs src;
    long dn[3];            // target cells per axis (grid order)
    long dstart[3];        // first table entry of each axis
    long dpitch[3];        // pitches of the target's axes
    long dpc, doff;
    long total;            // table entries
    long rows;             // target rows = product of dn over all axes but the last
    long chunk;            // cells of a row one block walks
};

__global__ void __launch_bounds__(256) regrid_tables_kernel(RegridArgs a, const double *__restrict__ coords, AxisTables t)
{
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    AxisData r;
    if (i >= a.dstart[2]) r = axis_data(coords[i], a.src.ax[2], a.src.ghost);
    else if (i >= a.dstart[1]) r = axis_data(coords[i], a.src.ax[1], a.src.ghost);
    else r = axis_data(coords[i], a.src.ax[0], a.src.ghost);
    t.cl[i] = r.cl; t.ch[i] = r.ch; t.wl[i] = r.wl; t.wh[i] = r.wh; t.ok[i] = r.ok;
}

inline __device__ AxisData load_axis(const AxisTables &t, long i)
{
    AxisData r;
    r.cl = t.cl[i]; r.ch = t.ch[i]; r.wl = t.wl[i]; r.wh = t.wh[i]; r.ok = t.ok[i];
    return r;
}

// One block walks one piece of one target row (the fastest axis): the slower axes' support rows and weights are the same for the
// whole block (uniform loads), neighbouring lanes store neighbouring cells and read the same or neighbouring source cells of at most
// 2 (2-D) / 4 (3-D) source rows.
template <typename T, int NDIM>
__global__ void __launch_bounds__(256) regrid_kernel(RegridArgs a, AxisTables t, const T *__restrict__ src, const double *__restrict__ fill,
                                                     T *__restrict__ dst, unsigned long long *oob)
{
    unsigned long long bad = 0;
    const long nlast = a.dn[NDIM - 1];
    const long k0 = blockIdx.y * a.chunk, k1 = (k0 + a.chunk < nlast) ? k0 + a.chunk : nlast;
    for (long row = blockIdx.x; row < a.rows; row += gridDim.x) {
        AxisData X, Y;
        X.cl = X.ch = Y.cl = Y.ch = 0; X.wl = X.wh = Y.wl = Y.wh = 0.0; X.ok = Y.ok = 1;
        long drow = a.doff;
        if (NDIM == 2) {
            X = load_axis(t, row);
            drow += row * a.dpitch[0];
        } else if (NDIM == 3) {
            const long i = row / a.dn[1], j = row - i * a.dn[1];
            X = load_axis(t, i);
            Y = load_axis(t, a.dstart[1] + j);
            drow += i * a.dpitch[0] + j * a.dpitch[1];
        }
        const int row_ok = X.ok & Y.ok;
        // (w_x * w_y) of grids.py:334-343 is the same for every cell of the row
        const double wll = X.wl * Y.wl, wlh = X.wl * Y.wh, whl = X.wh * Y.wl, whh = X.wh * Y.wh;
        const long px = a.src.ax[0].pitch, py = a.src.ax[1].pitch;
        for (long k = k0 + threadIdx.x; k < k1; k += blockDim.x) {
            const AxisData Z = load_axis(t, a.dstart[NDIM - 1] + k);
            T *o = dst + drow + k;
            if (!(row_ok & Z.ok)) {
                if (fill) {
                    for (int c = 0; c < a.src.ncomp; c++) o[c * a.dpc] = (T)fill[c];
                } else {
                    bad++;
                }
                continue;
            }
            const T *d = src + a.src.off;
            for (int c = 0; c < a.src.ncomp; c++, d += a.src.pc) {
                double v;
                if (NDIM == 1) {
                    v = Z.wl * (double)d[Z.cl] + Z.wh * (double)d[Z.ch];
                } else if (NDIM == 2) {
                    v = X.wl * Z.wl * (double)d[X.cl * px + Z.cl] + X.wl * Z.wh * (double)d[X.cl * px + Z.ch] +
                        X.wh * Z.wl * (double)d[X.ch * px + Z.cl] + X.wh * Z.wh * (double)d[X.ch * px + Z.ch];
                } else {
                    v = wll * Z.wl * (double)d[X.cl * px + Y.cl * py + Z.cl] + wll * Z.wh * (double)d[X.cl * px + Y.cl * py + Z.ch] +
                        wlh * Z.wl * (double)d[X.cl * px + Y.ch * py + Z.cl] + wlh * Z.wh * (double)d[X.cl * px + Y.ch * py + Z.ch] +
                        whl * Z.wl * (double)d[X.ch * px + Y.cl * py + Z.cl] + whl * Z.wh * (double)d[X.ch * px + Y.cl * py + Z.ch] +
                        whh * Z.wl * (double)d[X.ch * px + Y.ch * py + Z.cl] + whh * Z.wh * (double)d[X.ch * px + Y.ch * py + Z.ch];
                }
                o[c * a.dpc] = (T)v;
            }
        }
    }
    if (bad) atomicAdd(oob, bad);
}

// ---- edge and corner ghost cells (axes.py:475-495): means of the neighbouring ghost cells, in the field's own type ---------------
struct CornerArgs {
    long n[3], p[3];       // normalised axes: valid cells, pitches
    long pc, base;         // component pitch; offset of FULL cell (0,0,0) (the lower ghost corner)
    int ncomp, ndim, phase;   // phase 0: edges of a 3-D grid (interior cells along the edge) / corners of a 2-D grid; 1: corners of a 3-D grid
    long total;
};

template <typename T>
__global__ void __launch_bounds__(256) ghost_corners_kernel(CornerArgs a, T *data)
{
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= a.total) return;
    if (a.ndim == 2) {
        // d[i, j] = (d[nxt[i], j] + d[i, nxt[j]]) / 2, axes 1 and 2 of the normalised grid
        const int corner = (int)(t & 3);
        T *d = data + (t >> 2) * a.pc + a.base;
        const long gi = (corner & 2) ? a.n[1] + 1 : 0, gj = (corner & 1) ? a.n[2] + 1 : 0;
        const long ni = (corner & 2) ? a.n[1] : 1, nj = (corner & 1) ? a.n[2] : 1;
        const T s = d[ni * a.p[1] + gj * a.p[2]] + d[gi * a.p[1] + nj * a.p[2]];
        d[gi * a.p[1] + gj * a.p[2]] = s / (T)2;
        return;
    }
    if (a.phase == 0) {
        // the three families of edges: along x (ghost y, z), along y (ghost x, z), along z (ghost x, y); interior cells along the edge
        const long per = 4 * (a.n[0] + a.n[1] + a.n[2]);
        const long comp = t / per;
        long e = t - comp * per;
        T *d = data + comp * a.pc + a.base;
        int along, u, v;                          // the edge's axis and the two ghost axes (u < v)
        if (e < 4 * a.n[0]) { along = 0; u = 1; v = 2; }
        else if (e < 4 * (a.n[0] + a.n[1])) { e -= 4 * a.n[0]; along = 1; u = 0; v = 2; }
        else { e -= 4 * (a.n[0] + a.n[1]); along = 2; u = 0; v = 1; }
        const long nal = along == 0 ? a.n[0] : (along == 1 ? a.n[1] : a.n[2]);
        const long pal = along == 0 ? a.p[0] : (along == 1 ? a.p[1] : a.p[2]);
        const long nu = u == 0 ? a.n[0] : a.n[1], pu = u == 0 ? a.p[0] : a.p[1];
        const long nv = v == 1 ? a.n[1] : a.n[2], pv = v == 1 ? a.p[1] : a.p[2];
        const int corner = (int)(e / nal);
        const long s = e - corner * nal + 1;     // full index along the edge
        const long gi = (corner & 2) ? nu + 1 : 0, gj = (corner & 1) ? nv + 1 : 0;
        const long ni = (corner & 2) ? nu : 1, nj = (corner & 1) ? nv : 1;
        const T sum = d[s * pal + ni * pu + gj * pv] + d[s * pal + gi * pu + nj * pv];
        d[s * pal + gi * pu + gj * pv] = sum / (T)2;
        return;
    }
    // d[i, j, k] = (d[nxt[i], j, k] + d[i, nxt[j], k] + d[i, j, nxt[k]]) / 3
    const int corner = (int)(t & 7);
    T *d = data + (t >> 3) * a.pc + a.base;
    const long gi = (corner & 4) ? a.n[0] + 1 : 0, gj = (corner & 2) ? a.n[1] + 1 : 0, gk = (corner & 1) ? a.n[2] + 1 : 0;
    const long ni = (corner & 4) ? a.n[0] : 1, nj = (corner & 2) ? a.n[1] : 1, nk = (corner & 1) ? a.n[2] : 1;
    const T s = d[ni * a.p[0] + gj * a.p[1] + gk * a.p[2]] + d[gi * a.p[0] + nj * a.p[1] + gk * a.p[2]] + d[gi * a.p[0] + gj * a.p[1] + nk * a.p[2]];
    d[gi * a.p[0] + gj * a.p[1] + gk * a.p[2]] = s / (T)3;
}

int fill_source(const pdehip_grid_t *g, const NGrid &n, int ncomp, const int *periodic, const double *lo, int with_ghost_cells, InterpArgs *a)
{
    if (!periodic || !lo) PDEHIP_FAIL(E_VALUE, "interpolate: NULL pointer");
    if (ncomp < 1) PDEHIP_FAIL(E_VALUE, "interpolate: ncomp must be >= 1");
    memset(a, 0, sizeof(*a));
    for (int d = 0; d < g->ndim; d++) {
        const int ax = 3 - g->ndim + d;
        if (!(g->dx[d] > 0)) PDEHIP_FAIL(E_VALUE, "interpolate: discretization of axis %d must be positive", d);
        a->ax[d].size = n.n[ax];
        a->ax[d].pitch = n.p[ax];
        a->ax[d].lo = lo[d];
        a->ax[d].dx = g->dx[d];
        a->ax[d].periodic = periodic[d] ? 1 : 0;
    }
    a->ghost = with_ghost_cells ? 1 : 0;
    a->ncomp = ncomp;
    a->pc = n.pc;
    a->off = n.off;
    return 0;
}

}  // namespace
}  // namespace pdehip

using namespace pdehip;

extern "C" int pdehip_interpolate_points(const pdehip_grid_t *g, int ncomp, const int *periodic, const double *lo, int with_ghost_cells,
                                         const void *data_full, const double *points, int64_t npoints, const double *fill, void *out,
                                         void *oob_count, void *stream)
{
    NGrid n;
    PDEHIP_TRY(norm_grid(g, &n));
    InterpArgs a;
    PDEHIP_TRY(fill_source(g, n, ncomp, periodic, lo, with_ghost_cells, &a));
    if (npoints < 0) PDEHIP_FAIL(E_VALUE, "interpolate_points: negative number of points");
    if (npoints == 0) return 0;
    if (!data_full || !points || !out || (!fill && !oob_count)) PDEHIP_FAIL(E_VALUE, "interpolate_points: NULL pointer");
    a.npoints = npoints;
    long blocks = (npoints + 255) / 256;
    if (blocks > 2048) blocks = 2048;              // 8 blocks of 256 threads on each of the 256 compute units; grid-stride beyond
    hipStream_t s = as_stream(stream);
    unsigned long long *cnt = (unsigned long long *)oob_count;
#define PDEHIP_POINTS(T, ND) \
    hipLaunchKernelGGL((interp_points_kernel<T, ND>), dim3((unsigned)blocks), dim3(256), 0, s, a, (const T *)data_full, points, fill, (T *)out, cnt)
    if (n.dtype == PDEHIP_F64) {
        if (g->ndim == 1) PDEHIP_POINTS(double, 1); else if (g->ndim == 2) PDEHIP_POINTS(double, 2); else PDEHIP_POINTS(double, 3);
    } else {
        if (g->ndim == 1) PDEHIP_POINTS(float, 1); else if (g->ndim == 2) PDEHIP_POINTS(float, 2); else PDEHIP_POINTS(float, 3);
    }
#undef PDEHIP_POINTS
    note_kernel("interp_points_kernel<%s,%d>", n.dtype == PDEHIP_F64 ? "double" : "float", g->ndim);
    PDEHIP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pdehip_interpolate_to_grid(const pdehip_grid_t *src, int ncomp, const int *periodic, const double *src_lo, int with_ghost_cells,
                                          const void *src_full, const pdehip_grid_t *dst, const double *dst_coords, const double *fill,
                                          void *dst_full, void *tables, void *oob_count, void *stream)
{
    NGrid n, m;
    PDEHIP_TRY(norm_grid(src, &n));
    PDEHIP_TRY(norm_grid(dst, &m));
    if (src->ndim != dst->ndim || src->dtype != dst->dtype) PDEHIP_FAIL(E_VALUE, "interpolate_to_grid: the grids differ in the number of axes or in the type");
    RegridArgs a;
    memset(&a, 0, sizeof(a));
    PDEHIP_TRY(fill_source(src, n, ncomp, periodic, src_lo, with_ghost_cells, &a.src));
    if (!src_full || !dst_full || !dst_coords || !tables || (!fill && !oob_count)) PDEHIP_FAIL(E_VALUE, "interpolate_to_grid: NULL pointer");
    if (src_full == dst_full) PDEHIP_FAIL(E_VALUE, "interpolate_to_grid: source and target are the same array");
    const int nd = src->ndim;
    long total = 0, rows = 1;
    for (int d = 0; d < 3; d++) a.dstart[d] = -1;
    for (int d = 0; d < nd; d++) {
        const int ax = 3 - nd + d;
        a.dn[d] = m.n[ax];
        a.dpitch[d] = m.p[ax];
        a.dstart[d] = total;
        total += m.n[ax];
        if (d < nd - 1) rows *= m.n[ax];
    }
    for (int d = nd; d < 3; d++) a.dstart[d] = total;      // (the table kernel picks the axis by the start of the next one)
    a.dpc = m.pc; a.doff = m.off; a.total = total; a.rows = rows;
    a.chunk = 1024;
    const AxisTables t = split_tables(tables, total);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(regrid_tables_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, dst_coords, t);
    PDEHIP_HIP(hipGetLastError());
    const long nlast = a.dn[nd - 1];
    const long chunks = (nlast + a.chunk - 1) / a.chunk;
    if (chunks > 65535) PDEHIP_FAIL(E_NOTIMPL, "interpolate_to_grid: more than %ld cells along the last axis of the target", 65535 * a.chunk);
    const long bx = rows > (1L << 20) ? (1L << 20) : rows;
    const unsigned threads = nlast >= 256 ? 256 : (unsigned)(((nlast + 63) / 64) * 64);
    unsigned long long *cnt = (unsigned long long *)oob_count;
#define PDEHIP_REGRID(T, ND) \
    hipLaunchKernelGGL((regrid_kernel<T, ND>), dim3((unsigned)bx, (unsigned)chunks), dim3(threads), 0, s, a, t, (const T *)src_full, fill, (T *)dst_full, cnt)
    if (n.dtype == PDEHIP_F64) {
        if (nd == 1) PDEHIP_REGRID(double, 1); else if (nd == 2) PDEHIP_REGRID(double, 2); else PDEHIP_REGRID(double, 3);
    } else {
        if (nd == 1) PDEHIP_REGRID(float, 1); else if (nd == 2) PDEHIP_REGRID(float, 2); else PDEHIP_REGRID(float, 3);
    }
#undef PDEHIP_REGRID
    note_kernel("regrid_kernel<%s,%d>", n.dtype == PDEHIP_F64 ? "double" : "float", nd);
    PDEHIP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pdehip_set_ghost_corners(const pdehip_grid_t *g, int ncomp, void *data_full, void *stream)
{
    NGrid n;
    PDEHIP_TRY(norm_grid(g, &n));
    if (!data_full) PDEHIP_FAIL(E_VALUE, "set_ghost_corners: NULL pointer");
    if (ncomp < 1) PDEHIP_FAIL(E_VALUE, "set_ghost_corners: ncomp must be >= 1");
    if (g->ndim < 2) return 0;                     // axes.py:475: nothing to do on one axis
    CornerArgs a;
    memset(&a, 0, sizeof(a));
    for (int ax = 0; ax < 3; ax++) { a.n[ax] = n.n[ax]; a.p[ax] = n.p[ax]; }
    a.pc = n.pc;
    a.base = n.off - n.gh[0] * n.p[0] - n.gh[1] * n.p[1] - n.gh[2] * n.p[2];
    a.ncomp = ncomp; a.ndim = g->ndim;
    hipStream_t s = as_stream(stream);
    for (int phase = 0; phase < (g->ndim == 3 ? 2 : 1); phase++) {
        a.phase = phase;
        a.total = (long)ncomp * (g->ndim == 2 ? 4 : (phase == 0 ? 4 * (n.n[0] + n.n[1] + n.n[2]) : 8));
        const unsigned blocks = (unsigned)((a.total + 255) / 256);
        if (n.dtype == PDEHIP_F64) hipLaunchKernelGGL((ghost_corners_kernel<double>), dim3(blocks), dim3(256), 0, s, a, (double *)data_full);
        else hipLaunchKernelGGL((ghost_corners_kernel<float>), dim3(blocks), dim3(256), 0, s, a, (float *)data_full);
        PDEHIP_HIP(hipGetLastError());
    }
    return 0;
}
