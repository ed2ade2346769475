// pdehip_project.hip — reduced-dimensional pictures of a field where it lives: the sum (x weight), the maximum or the minimum of every
// component over a subset of the axes, and dense copies of interior boxes (slices, lines, single cells).
//
// Semantics: pde/fields/scalar.py:269-427 (ScalarField.project / .slice), pde/grids/base.py:1286-1341 (grid.integrate over axes),
// pde/grids/cartesian.py:296-402 (get_line_data / get_image_data).
//
// TWO reduction kernels, chained by the host until the mask is empty.  Every stage but the first reads a dense fp64 array another
// stage left in the stream's scratch; the last stage writes the caller's array.
//   project_row_kernel    removes the FASTEST axis: a group of 1, 2, 4 ... 64 lanes (the smallest power of two that covers the pieces of
//                         a row) takes one row, each lane pieces of VEC cells with four loads in flight, then a butterfly over the group.
//                         Result: a dense (n0, n1) array, on which the same kernel removes the next axis.
//   project_march_kernel  removes SLOWER axes and keeps the fastest: a thread owns VEC cells of an output row and marches over the removed
//                         cells with four loads in flight; the lanes of a wave read one contiguous piece of a row at every step.  The
//                         removed extent is cut into segments of kProjectSegment cells (the cut depends on the shape only); with more
//                         than one segment the result is a dense (segments, output cells) array, on which the same kernel removes axis 0.
// Every thread's order is fixed by the launch geometry and no atomics are used: two calls give equal bits.  A term of a sum is
// (double)x * weight, one rounding; every addition is one rounding (compiled without FMA contraction in every build).  The maximum
// keeps a NaN once it met one (np.max); the minimum is -max(-x), both negations exact.
#include "pdehip_common.h"
#include "pdehip_pieces.h"
#include "pdehip_scratch.h"
#include "pdehip_sweep.h"

namespace pdehip {
namespace {

constexpr long kProjectSegment = 128;      // removed cells one thread of the march marches over (tests/project_cases.py: SEGMENT)
constexpr long kProjectBlocksMax = 1024;   // workgroups of a launch; what is beyond takes a grid-stride turn (tests/project_cases.py: TURN_THREADS)

struct OpSum {
    __device__ static double identity() { return 0.0; }
    __device__ static double apply(double a, double b) { return a + b; }
};
// NaN wins, whichever side it comes from, and stays
struct OpMaxNan {
    __device__ static double identity() { return __longlong_as_double((long long)0xfff0000000000000ULL); }
    __device__ static double apply(double a, double b) { return (b > a || b != b) ? b : a; }
};

struct ProjectArgs {
    RowGrid g;             // the array this stage reads: the field (device layout) or a dense array of an earlier stage
    long in_cs, out_cs;    // elements from one component to the next, input and output
    const void *in;
    void *out;
    double weight;         // factor of every term (sum: the weight in the first stage; maximum: 1, minimum: -1; later stages: 1)
    double out_scale;      // factor of every result (-1 in the last stage of a minimum, else 1)
    int out_f32;           // the output holds float (last stage of an extremum of an fp32 field), else double
    int gw;                // row kernel: lanes of a group
    long m1, m;            // march kernel: removed cells of axis 1 (1 where it is kept) and of both axes together
    long nq, qs;           // ... cells and pitch of the kept slower axis (1 cell if both are removed)
    long nseg;             // ... segments the removed cells are cut into
};

template <class OP, typename T, int VEC>
__device__ __forceinline__ void take(double &acc, const T (&v)[VEC], double weight)
{
#pragma unroll
    for (int q = 0; q < VEC; q++) acc = OP::apply(acc, (double)v[q] * weight);
}
__device__ __forceinline__ void put(const ProjectArgs &a, long at, double v)
{
    v = v * a.out_scale;
    if (a.out_f32) ((float *)a.out)[at] = (float)v;
    else ((double *)a.out)[at] = v;
}

template <typename T, int VEC, class OP>
__global__ void __launch_bounds__(256) project_row_kernel(ProjectArgs a)
{
    const T *in = (const T *)a.in + (long)blockIdx.y * a.in_cs + a.g.off;
    const int gw = a.gw;
    const long per_row = a.g.n2 / VEC;
    const long rows = a.g.n0 * a.g.n1;
    const long groups = (long)gridDim.x * 256 / gw;
    const long first = (blockIdx.x * 256L + threadIdx.x) / gw;
    const int lane = (int)threadIdx.x & (gw - 1);
    const long rounds = (rows + groups - 1) / groups;      // the same for every lane: the butterfly below runs with all lanes
    for (long it = 0; it < rounds; it++) {
        const long row = first + it * groups;
        const bool valid = row < rows;
        double acc = OP::identity();
        if (valid) {
            const long i = row / a.g.n1, j = row - i * a.g.n1;
            const T *p = in + i * a.g.p0 + j * a.g.p1;
            long c = lane;
            for (; c + 3L * gw < per_row; c += 4L * gw) {
                T v[4][VEC];
#pragma unroll
                for (int u = 0; u < 4; u++) load_piece<T, VEC>(p + (c + (long)u * gw) * VEC, v[u]);
#pragma unroll
                for (int u = 0; u < 4; u++) take<OP, T, VEC>(acc, v[u], a.weight);
            }
            for (; c < per_row; c += gw) {
                T v[VEC];
                load_piece<T, VEC>(p + c * VEC, v);
                take<OP, T, VEC>(acc, v, a.weight);
            }
        }
        for (int ofs = gw >> 1; ofs >= 1; ofs >>= 1) acc = OP::apply(acc, __shfl_xor(acc, ofs, 64));
        if (valid && lane == 0) put(a, (long)blockIdx.y * a.out_cs + row, acc);
    }
}

template <typename T, int VEC, class OP>
__global__ void __launch_bounds__(256) project_march_kernel(ProjectArgs a)
{
    const T *in = (const T *)a.in + (long)blockIdx.y * a.in_cs + a.g.off;
    const long per_row = a.g.n2 / VEC;
    const long pieces = a.nq * per_row;
    const long total = pieces * a.nseg;
    const long wrap = a.g.p0 - a.m1 * a.g.p1;      // from behind the last removed cell of axis 1 to the first one of the next layer
    for (long t = blockIdx.x * 256L + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const long seg = t / pieces, rest = t - seg * pieces;
        const long q = rest / per_row, k = (rest - q * per_row) * VEC;
        long r = seg * kProjectSegment;
        const long end = r + kProjectSegment < a.m ? r + kProjectSegment : a.m;
        const long i = r / a.m1;
        long j = r - i * a.m1;
        const T *p = in + q * a.qs + i * a.g.p0 + j * a.g.p1 + k;
        double acc[VEC];
#pragma unroll
        for (int x = 0; x < VEC; x++) acc[x] = OP::identity();
        for (; r + 4 <= end; r += 4) {
            T v[4][VEC];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                load_piece<T, VEC>(p, v[u]);
                p += a.g.p1;
                if (++j == a.m1) { j = 0; p += wrap; }
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int x = 0; x < VEC; x++) acc[x] = OP::apply(acc[x], (double)v[u][x] * a.weight);
        }
        for (; r < end; r++) {
            T v[VEC];
            load_piece<T, VEC>(p, v);
            p += a.g.p1;
            if (++j == a.m1) { j = 0; p += wrap; }
#pragma unroll
            for (int x = 0; x < VEC; x++) acc[x] = OP::apply(acc[x], (double)v[x] * a.weight);
        }
        const long at = (long)blockIdx.y * a.out_cs + seg * (a.nq * a.g.n2) + q * a.g.n2 + k;
#pragma unroll
        for (int x = 0; x < VEC; x++) put(a, at + x, acc[x]);
    }
}

// ---- boxes ---------------------------------------------------------------------------------------------------------------------------
struct BoxArgs {
    long p0, p1, off, pc;  // the field
    long lo[3], n[3];      // the box, normalised axes
    const void *in;
    void *out;
};
template <typename T>
__global__ void __launch_bounds__(256) extract_box_kernel(BoxArgs a)
{
    const T *in = (const T *)a.in + (long)blockIdx.y * a.pc + a.off;
    const long total = a.n[0] * a.n[1] * a.n[2];
    T *out = (T *)a.out + (long)blockIdx.y * total;
    for (long t = blockIdx.x * 256L + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        long rest = t;
        const long k = rest % a.n[2]; rest /= a.n[2];
        const long j = rest % a.n[1];
        const long i = rest / a.n[1];
        out[t] = in[(a.lo[0] + i) * a.p0 + (a.lo[1] + j) * a.p1 + a.lo[2] + k];
    }
}

// ---- the partial results of the stages: two halves used in turn, one buffer per STREAM (calls on one stream are ordered; two streams
// reducing at the same time must not share one), grown on demand and kept until pdehip_release_scratch ---------------------------------
struct ProjectScratch { double *p; size_t doubles; };
int release_partials();
StreamTable<ProjectScratch> g_table(release_partials);

int release_partials()
{
    return g_table.release([](ProjectScratch &s) { (void)hipFree(s.p); });
}

int project_scratch(hipStream_t st, size_t doubles, double **p)
{
    return g_table.with(st, [&](ProjectScratch &s) -> int {
        if (s.doubles < doubles) {
            if (s.p) (void)hipFree(s.p);       // (hipFree waits for the device: no stage still reads the old buffer)
            s.p = nullptr; s.doubles = 0;
            PDEHIP_HIP(hipMalloc(&s.p, sizeof(double) * doubles));
            s.doubles = doubles;
        }
        *p = s.p;
        return 0;
    });
}

// what a stage reads
struct Stage {
    RowGrid g;
    long cs;               // elements from one component to the next
    const void *ptr;
    int f64, vec;
};

template <class OP>
void launch_stage(bool row, const Stage &s, unsigned blocks, int ncomp, hipStream_t st, const ProjectArgs &a)
{
    dispatch_piece(s.f64 ? PDEHIP_F64 : PDEHIP_F32, s.vec, [&](auto type, auto width) {
        typedef decltype(type) T;
        constexpr int V = decltype(width)::value;
        if (row) hipLaunchKernelGGL((project_row_kernel<T, V, OP>), dim3(blocks, ncomp), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((project_march_kernel<T, V, OP>), dim3(blocks, ncomp), dim3(256), 0, st, a);
    });
}

}  // namespace
}  // namespace pdehip

using namespace pdehip;

extern "C" int pdehip_project(const pdehip_grid_t *g, int ncomp, const void *arr_full, int axes_mask, int method, double weight,
                              void *out_dev, void *stream)
{
    NGrid n;
    PDEHIP_TRY(norm_grid(g, &n));
    if (!arr_full || !out_dev) PDEHIP_FAIL(E_VALUE, "project: NULL pointer");
    if (ncomp < 1 || ncomp > 64) PDEHIP_FAIL(E_VALUE, "project: 1..64 components");
    if (axes_mask <= 0 || axes_mask >= (1 << n.ndim)) PDEHIP_FAIL(E_VALUE, "project: the mask %d names no axis or an axis the grid does not have", axes_mask);
    if (method != PDEHIP_PROJECT_SUM && method != PDEHIP_PROJECT_MAX && method != PDEHIP_PROJECT_MIN) PDEHIP_FAIL(E_VALUE, "project: unknown method %d", method);
    if (((uintptr_t)arr_full & 15) != 0 || ((uintptr_t)out_dev & 7) != 0) PDEHIP_FAIL(E_VALUE, "project: misaligned array (16 bytes for the field, 8 for the result)");
    const bool sum = method == PDEHIP_PROJECT_SUM;
    const bool f64 = n.dtype == PDEHIP_F64;
    hipStream_t st = as_stream(stream);

    // bit `a` of the mask is axis `a` of the grid; bit b of `mask`: normalised axis b (an n-D grid has the trailing n axes)
    int mask = 0;
    for (int a = 0; a < n.ndim; a++)
        if (axes_mask & (1 << a)) mask |= 1 << (3 - n.ndim + a);

    Stage s;
    s.g = make_row_grid(n); s.cs = n.pc; s.ptr = arr_full; s.f64 = f64;
    s.vec = piece_width(n, arr_full, nullptr);      // (the field is on a 16-byte boundary: checked above)
    // the first stage leaves the largest intermediate array
    const long rows = n.n[0] * n.n[1];
    size_t half = 0;
    if (mask & 4) {
        half = (mask & 3) ? (size_t)rows : 0;
    } else {
        const long m = ((mask & 1) ? n.n[0] : 1) * ((mask & 2) ? n.n[1] : 1);
        const long nseg = (m + kProjectSegment - 1) / kProjectSegment;
        half = nseg > 1 ? (size_t)(nseg * (rows / m) * n.n[2]) : 0;
    }
    double *scratch = nullptr;
    if (half) PDEHIP_TRY(project_scratch(st, 2 * half * ncomp, &scratch));

    char name[192];
    int len = 0, turn = 0;
    double w = sum ? weight : (method == PDEHIP_PROJECT_MIN ? -1.0 : 1.0);
    while (mask) {
        ProjectArgs a;
        memset(&a, 0, sizeof(a));
        a.g = s.g; a.in_cs = s.cs; a.in = s.ptr; a.weight = w; a.out_scale = 1.0; a.gw = 1;
        a.m1 = a.m = a.nq = a.nseg = 1;
        Stage next;
        next.f64 = 1; next.vec = 1;
        bool last, row = (mask & 4) != 0;
        long out_cells, threads;
        if (row) {
            const long per_row = s.g.n2 / s.vec;
            while (a.gw < 64 && a.gw < per_row) a.gw *= 2;
            out_cells = s.g.n0 * s.g.n1;
            threads = out_cells * a.gw;
            last = (mask & 3) == 0;
            next.g = RowGrid{1, s.g.n0, s.g.n1, out_cells, s.g.n1, 0};
            mask = (mask & 3) << 1;
        } else {
            const bool r0 = (mask & 1) != 0, r1 = (mask & 2) != 0;
            a.m1 = r1 ? s.g.n1 : 1; a.m = (r0 ? s.g.n0 : 1) * a.m1;
            a.nq = (r0 && r1) ? 1 : (r0 ? s.g.n1 : s.g.n0);
            a.qs = (r0 && r1) ? 0 : (r0 ? s.g.p1 : s.g.p0);
            a.nseg = (a.m + kProjectSegment - 1) / kProjectSegment;
            const long line = a.nq * s.g.n2;
            out_cells = a.nseg * line;
            threads = out_cells / s.vec;
            last = a.nseg == 1;
            next.g = RowGrid{a.nseg, 1, line, line, line, 0};
            mask = last ? 0 : 1;
        }
        a.out_cs = out_cells;
        if (last) {
            a.out = out_dev;
            a.out_scale = method == PDEHIP_PROJECT_MIN ? -1.0 : 1.0;
            a.out_f32 = !sum && !f64;
        } else {
            a.out = scratch + (size_t)turn * half * ncomp;
        }
        const unsigned blocks = blocks_for(threads, kProjectBlocksMax);
        if (sum) launch_stage<OpSum>(row, s, blocks, ncomp, st, a);
        else launch_stage<OpMaxNan>(row, s, blocks, ncomp, st, a);
        len += snprintf(name + len, sizeof(name) - len, "%sproject_%s_kernel<%s,%d,%s>", len ? "+" : "", row ? "row" : "march",
                        s.f64 ? "double" : "float", s.vec, sum ? "sum" : "max");
        if (len >= (int)sizeof(name)) len = (int)sizeof(name) - 1;
        next.cs = out_cells; next.ptr = a.out;
        s = next;
        w = 1.0;
        turn ^= 1;
    }
    note_kernel("%s", name);
    PDEHIP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pdehip_extract_box(const pdehip_grid_t *g, int ncomp, const void *arr_full, const long *lo, const long *extent,
                                  void *out_dev, void *stream)
{
    NGrid n;
    PDEHIP_TRY(norm_grid(g, &n));
    if (!arr_full || !out_dev || !lo || !extent) PDEHIP_FAIL(E_VALUE, "extract_box: NULL pointer");
    if (ncomp < 1 || ncomp > 64) PDEHIP_FAIL(E_VALUE, "extract_box: 1..64 components");
    const uintptr_t esize = (uintptr_t)elem_size(n.dtype);
    if (((uintptr_t)arr_full & 15) != 0 || ((uintptr_t)out_dev & (esize - 1)) != 0) PDEHIP_FAIL(E_VALUE, "extract_box: misaligned array (16 bytes for the field, one element for the result)");
    BoxArgs a;
    a.p0 = n.p[0]; a.p1 = n.p[1]; a.off = n.off; a.pc = n.pc; a.in = arr_full; a.out = out_dev;
    for (int ax = 0; ax < 3; ax++) { a.lo[ax] = 0; a.n[ax] = 1; }
    for (int d = 0; d < n.ndim; d++) {
        const int ax = 3 - n.ndim + d;
        if (lo[d] < 0 || extent[d] < 1 || lo[d] > n.n[ax] - extent[d])
            PDEHIP_FAIL(E_VALUE, "extract_box: axis %d: [%ld, %ld + %ld) is not a box inside %ld cells", d, lo[d], lo[d], extent[d], n.n[ax]);
        a.lo[ax] = lo[d]; a.n[ax] = extent[d];
    }
    const unsigned blocks = blocks_for(a.n[0] * a.n[1] * a.n[2], kProjectBlocksMax);
    if (n.dtype == PDEHIP_F64) hipLaunchKernelGGL((extract_box_kernel<double>), dim3(blocks, ncomp), dim3(256), 0, as_stream(stream), a);
    else hipLaunchKernelGGL((extract_box_kernel<float>), dim3(blocks, ncomp), dim3(256), 0, as_stream(stream), a);
    note_kernel("extract_box_kernel<%s>", n.dtype == PDEHIP_F64 ? "double" : "float");
    PDEHIP_HIP(hipGetLastError());
    return 0;
}
