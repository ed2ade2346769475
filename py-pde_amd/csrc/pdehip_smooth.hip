// pdehip_smooth.hip — one pass of a separable Gaussian filter along one axis of a field, where the field lives.
//
// Semantics: pde/fields/datafield_base.py:988-1035 (DataFieldBase.smooth): scipy.ndimage.gaussian_filter1d axis by axis, mode "wrap" on
// periodic axes and "reflect" (half-sample symmetric) elsewhere.  The arithmetic of a pass is written out in include/pdehip.h; it is
// scipy's symmetric branch: the centre term first, then the pairs from the outermost one inwards, every product and every addition one
// fp64 rounding (this unit is compiled without FMA contraction in every build), an fp32 field converted exactly on load and rounded once
// on store.  The weights come from the host (numpy's exp is the one scipy uses); they are staged per stream and the kernels read them
// with a wave-uniform index, i.e. through the scalar cache into scalar registers.
//
// THREE kernels; the first two stage the cells a workgroup needs ONCE in LDS, as fp64, with the wrapped or reflected index resolved at
// staging time, and then read 2r+1 values per output from LDS:
//   gauss_row_kernel<T>        the FASTEST axis.  A wave owns a piece of kRowLanes = 64 cells of one row: it stages 64 + 2r cells and
//                              every lane writes one output.  A workgroup holds kRowPieces = 4 such pieces (consecutive pieces of the
//                              rows in memory order).  Halo share (64 + 2r) / 64.
//   gauss_march_kernel<T,VEC>  any SLOWER axis.  The lanes lie along the fastest axis (VEC cells per lane: 16-byte accesses where the row
//                              length is a multiple of 2 doubles / 4 floats, else one cell): a workgroup stages (L + 2r) cells of the
//                              filtered axis x kMarchWidth = 32 cells of the fastest axis and writes L = kMarchLength = 64 x 32 outputs.
//                              Halo share (L + 2r) / L.  In LDS a row of the tile is 32 consecutive doubles: the lanes of a wave read
//                              consecutive addresses at every tap.
//   gauss_cell_kernel<T>       any axis, any radius, any extent: one output per thread, the neighbours through the caches, the index
//                              resolved at every tap.  Runs when the tile plus halo does not fit, and under PDEHIP_SMOOTH_CELL.
//
// LDS budget: kSmoothLdsDoubles = 5120 doubles = 40 KiB per workgroup of 256 threads, so that FOUR workgroups (four waves per SIMD) fit
// the 160 KiB of a CU.  The radius caps follow from it and the tiles, and from nothing else:
//   kRowRadiusMax   = (5120 / 4 - 64) / 2 = 608      (4 pieces x (64 + 2r) doubles)
//   kMarchRadiusMax = (5120 / 32 - 64) / 2 = 48      ((64 + 2r) x 32 doubles)
// Launches are capped at kSmoothBlocksMax workgroups per component; what is beyond takes a grid-stride turn.  No atomics, every output
// has one writer and one order: two calls give equal bits.
#include "pdehip_common.h"
#include "pdehip_pieces.h"
#include "pdehip_scratch.h"
#include "pdehip_sweep.h"

namespace pdehip {
namespace {

constexpr long kSmoothLdsDoubles = 5120;
constexpr int kRowLanes = 64;
constexpr int kRowPieces = 4;
constexpr int kRowRadiusMax = (int)(kSmoothLdsDoubles / kRowPieces - kRowLanes) / 2;
constexpr int kMarchWidth = 32;
constexpr int kMarchLength = 64;
constexpr int kMarchRadiusMax = (int)(kSmoothLdsDoubles / kMarchWidth - kMarchLength) / 2;
constexpr long kSmoothBlocksMax = 2048;      // workgroups of a launch (tests/smooth_cases.py: BLOCKS_MAX)
constexpr long kSmoothExtentMax = 1L << 30;  // the LDS instances resolve indices in 32 bits (2n must fit)
static_assert(kRowPieces * (kRowLanes + 2 * kRowRadiusMax) <= kSmoothLdsDoubles, "row tile exceeds the LDS budget");
static_assert((kMarchLength + 2 * kMarchRadiusMax) * kMarchWidth <= kSmoothLdsDoubles, "march tile exceeds the LDS budget");
static_assert(kRowRadiusMax == 608 && kMarchRadiusMax == 48, "the caps quoted in the header comment and in include/pdehip.h");

struct SmoothArgs {
    long n[3];         // normalised axes: interior cells
    long p0, p1;       // pitches of axes 0 and 1 (axis 2: 1)
    long pc, off;      // elements of a component, offset of interior cell (0, 0, 0)
    long na, ps;       // the filtered axis: cells and pitch
    long nq, qs;       // march: the other slower axis
    int axis;          // normalised
    int mode;          // PDEHIP_SMOOTH_WRAP / _REFLECT
    int r;
};

// the cell of [0, n) that position p of the extended line shows: p mod n (wrap), or p mod 2n mirrored at n - 1/2 (reflect)
template <typename I>
__device__ __forceinline__ I resolve(I p, I n, int mode)
{
    if (p >= 0 && p < n) return p;
    if (mode == PDEHIP_SMOOTH_WRAP) {
        const I q = p % n;
        return q < 0 ? q + n : q;
    }
    const I m = 2 * n;
    I q = p % m;
    if (q < 0) q += m;
    return q < n ? q : m - 1 - q;
}

// VEC fp64 results in one access, each rounded once to the field's type (beside store_piece of pdehip_pieces.h, not an overload of it:
// for an fp64 field the two would be one signature)
template <typename T, int VEC>
__device__ __forceinline__ void store_cells(T *p, const double (&v)[VEC])
{
    if constexpr (VEC == 1) {
        p[0] = (T)v[0];
    } else {
        typedef T vec_t __attribute__((ext_vector_type(VEC)));
        vec_t x;
#pragma unroll
        for (int q = 0; q < VEC; q++) x[q] = (T)v[q];
        *(vec_t *)p = x;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) gauss_row_kernel(SmoothArgs a, const T *__restrict__ in, T *__restrict__ out, const double *__restrict__ w)
{
    __shared__ double tile[kSmoothLdsDoubles];
    in += (long)blockIdx.y * a.pc + a.off;
    out += (long)blockIdx.y * a.pc + a.off;
    const int r = a.r, n = (int)a.n[2];
    const int wave = (int)threadIdx.x / kRowLanes, lane = (int)threadIdx.x % kRowLanes;
    const int span = kRowLanes + 2 * r;
    double *mine = tile + wave * span;
    const long per_row = (n + kRowLanes - 1) / kRowLanes;
    const long pieces = a.n[0] * a.n[1] * per_row;
    const long stride = (long)gridDim.x * kRowPieces;
    const long rounds = (pieces + stride - 1) / stride;      // the same for every thread: the barriers below are met by all
    for (long it = 0; it < rounds; it++) {
        const long piece = (it * gridDim.x + blockIdx.x) * kRowPieces + wave;
        const bool valid = piece < pieces;
        long base = 0;
        int c0 = 0;
        if (valid) {
            const long row = piece / per_row;
            c0 = (int)(piece - row * per_row) * kRowLanes;
            const long i = row / a.n[1], j = row - i * a.n[1];
            base = i * a.p0 + j * a.p1;
            for (int s = lane; s < span; s += kRowLanes) mine[s] = (double)in[base + resolve<int>(c0 + s - r, n, a.mode)];
        }
        __syncthreads();
        if (valid && c0 + lane < n) {
            const double *c = mine + r + lane;
            double t = c[0] * w[0];
            for (int j = r; j >= 1; j--) t = t + (c[-j] + c[j]) * w[j];
            out[base + c0 + lane] = (T)t;
        }
        __syncthreads();
    }
}

template <typename T, int VEC>
__global__ void __launch_bounds__(256) gauss_march_kernel(SmoothArgs a, const T *__restrict__ in, T *__restrict__ out, const double *__restrict__ w)
{
    __shared__ double tile[kSmoothLdsDoubles];
    constexpr int TPR = kMarchWidth / VEC;      // threads along a row of the tile
    constexpr int RY = 256 / TPR;               // rows of the tile the workgroup takes at a time
    in += (long)blockIdx.y * a.pc + a.off;
    out += (long)blockIdx.y * a.pc + a.off;
    const int tx = (int)threadIdx.x % TPR, ty = (int)threadIdx.x / TPR;
    const int r = a.r, n = (int)a.na;
    const long xt = (a.n[2] + kMarchWidth - 1) / kMarchWidth, yt = (n + kMarchLength - 1) / kMarchLength;
    const long tiles = a.nq * yt * xt;
    for (long t = blockIdx.x; t < tiles; t += gridDim.x) {      // (t depends on the workgroup alone: the barriers are met by all)
        const long q = t / (yt * xt), rest = t - q * (yt * xt);
        const long ytile = rest / xt;
        const int y0 = (int)ytile * kMarchLength;
        const long x = (rest - ytile * xt) * kMarchWidth + tx * VEC;
        const bool inside = x < a.n[2];         // (n2 is a multiple of VEC: a lane is inside with all its cells or with none)
        const long base = q * a.qs + x;
        const int len = n - y0 < kMarchLength ? n - y0 : kMarchLength;
        if (inside)
            for (int s = ty; s < len + 2 * r; s += RY) {
                T v[VEC];
                load_piece<T, VEC>(in + base + (long)resolve<int>(y0 + s - r, n, a.mode) * a.ps, v);
#pragma unroll
                for (int k = 0; k < VEC; k++) tile[s * kMarchWidth + tx * VEC + k] = (double)v[k];
            }
        __syncthreads();
        if (inside)
            for (int y = ty; y < len; y += RY) {
                const double *c = tile + (y + r) * kMarchWidth + tx * VEC;
                double acc[VEC];
                const double w0 = w[0];
#pragma unroll
                for (int k = 0; k < VEC; k++) acc[k] = c[k] * w0;
                for (int j = r; j >= 1; j--) {
                    const double wj = w[j];
#pragma unroll
                    for (int k = 0; k < VEC; k++) acc[k] = acc[k] + (c[k - j * kMarchWidth] + c[k + j * kMarchWidth]) * wj;
                }
                store_cells<T, VEC>(out + base + (long)(y0 + y) * a.ps, acc);
            }
        __syncthreads();
    }
}

template <typename T>
__global__ void __launch_bounds__(256) gauss_cell_kernel(SmoothArgs a, const T *__restrict__ in, T *__restrict__ out, const double *__restrict__ w)
{
    in += (long)blockIdx.y * a.pc + a.off;
    out += (long)blockIdx.y * a.pc + a.off;
    const long total = a.n[0] * a.n[1] * a.n[2];
    const int r = a.r;
    for (long t = blockIdx.x * 256L + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        long rest = t;
        const long k = rest % a.n[2]; rest /= a.n[2];
        const long j = rest % a.n[1];
        const long i = rest / a.n[1];
        const long e = i * a.p0 + j * a.p1 + k;
        const long c = a.axis == 0 ? i : (a.axis == 1 ? j : k);
        const long line = e - c * a.ps;
        double acc = (double)in[e] * w[0];
        for (int m = r; m >= 1; m--) {
            const long lo = resolve<long>(c - m, a.na, a.mode), hi = resolve<long>(c + m, a.na, a.mode);
            acc = acc + ((double)in[line + lo * a.ps] + (double)in[line + hi * a.ps]) * w[m];
        }
        out[e] = (T)acc;
    }
}

// ---- the weights of a pass on the device: per STREAM a ring of kWeightSlots slots, each a pinned host copy (filled before the entry
// returns: the caller's array is consumed) and its device twin (filled by a copy in stream order, behind the kernels that still read
// what the slot held).  A slot is taken again only after its last copy has left the pinned memory.  Grown on demand, kept until
// pdehip_release_scratch ---------------------------------------------------------------------------------------------------------------
constexpr int kWeightSlots = 4;
struct WeightRing {
    double *dev = nullptr, *pinned = nullptr;
    size_t doubles = 0;                  // of one slot
    hipEvent_t copied[kWeightSlots] = {};
    bool pending[kWeightSlots] = {};
    unsigned turn = 0;
};
int release_rings();
StreamTable<WeightRing> g_table(release_rings);

void free_ring(WeightRing &s)
{
    if (s.dev) (void)hipFree(s.dev);             // (hipFree waits for the device: no kernel still reads the weights)
    if (s.pinned) (void)hipHostFree(s.pinned);
    for (int k = 0; k < kWeightSlots; k++) {
        if (s.copied[k]) (void)hipEventDestroy(s.copied[k]);
        s.copied[k] = nullptr;
        s.pending[k] = false;
    }
    s.dev = s.pinned = nullptr;
    s.doubles = 0;
}

int release_rings() { return g_table.release(free_ring); }

int stage_weights(hipStream_t st, const double *weights, size_t count, const double **dev)
{
    return g_table.with(st, [&](WeightRing &s) -> int {
        if (s.doubles < count) {
            free_ring(s);
            size_t cap = 64;
            while (cap < count) cap *= 2;
            PDEHIP_HIP(hipMalloc(&s.dev, sizeof(double) * cap * kWeightSlots));
            PDEHIP_HIP(hipHostMalloc((void **)&s.pinned, sizeof(double) * cap * kWeightSlots, hipHostMallocDefault));
            for (int k = 0; k < kWeightSlots; k++) PDEHIP_HIP(hipEventCreateWithFlags(&s.copied[k], hipEventDisableTiming));
            s.doubles = cap;
        }
        const unsigned k = s.turn++ % kWeightSlots;
        if (s.pending[k]) PDEHIP_HIP(hipEventSynchronize(s.copied[k]));
        double *host = s.pinned + k * s.doubles, *device = s.dev + k * s.doubles;
        memcpy(host, weights, sizeof(double) * count);
        PDEHIP_HIP(hipMemcpyAsync(device, host, sizeof(double) * count, hipMemcpyHostToDevice, st));
        PDEHIP_HIP(hipEventRecord(s.copied[k], st));
        s.pending[k] = true;
        *dev = device;
        return 0;
    });
}

}  // namespace
}  // namespace pdehip

using namespace pdehip;

extern "C" int pdehip_smooth_axis(const pdehip_grid_t *g, int ncomp, const void *in_full, void *out_full, int axis, int mode, int radius,
                                  const double *weights, void *stream)
{
    NGrid n;
    PDEHIP_TRY(norm_grid(g, &n));
    if (!in_full || !out_full || !weights) PDEHIP_FAIL(E_VALUE, "smooth_axis: NULL pointer");
    if (ncomp < 1 || ncomp > 64) PDEHIP_FAIL(E_VALUE, "smooth_axis: 1..64 components");
    if (axis < 0 || axis >= n.ndim) PDEHIP_FAIL(E_VALUE, "smooth_axis: the grid has no axis %d", axis);
    const bool force_cell = (mode & PDEHIP_SMOOTH_CELL) != 0;
    const int m = mode & ~PDEHIP_SMOOTH_CELL;
    if (m != PDEHIP_SMOOTH_WRAP && m != PDEHIP_SMOOTH_REFLECT) PDEHIP_FAIL(E_VALUE, "smooth_axis: unknown mode %d", mode);
    if (radius < 0) PDEHIP_FAIL(E_VALUE, "smooth_axis: negative radius %d", radius);
    const uintptr_t bytes = (uintptr_t)ncomp * (uintptr_t)n.pc * (uintptr_t)elem_size(n.dtype);
    const uintptr_t lo_in = (uintptr_t)in_full, lo_out = (uintptr_t)out_full;
    if (lo_in < lo_out + bytes && lo_out < lo_in + bytes) PDEHIP_FAIL(E_VALUE, "smooth_axis: the input and the output overlap (a pass cannot run in place)");
    if (((lo_in | lo_out) & 15) != 0) PDEHIP_FAIL(E_VALUE, "smooth_axis: misaligned array (16 bytes)");
    hipStream_t st = as_stream(stream);
    const double *w = nullptr;
    PDEHIP_TRY(stage_weights(st, weights, (size_t)radius + 1, &w));

    SmoothArgs a;
    memset(&a, 0, sizeof(a));
    for (int ax = 0; ax < 3; ax++) a.n[ax] = n.n[ax];
    a.p0 = n.p[0]; a.p1 = n.p[1]; a.pc = n.pc; a.off = n.off;
    a.axis = 3 - n.ndim + axis;
    a.na = n.n[a.axis]; a.ps = n.p[a.axis];
    a.nq = 1; a.qs = 0;
    if (a.axis < 2) { a.nq = n.n[1 - a.axis]; a.qs = n.p[1 - a.axis]; }
    a.mode = m; a.r = radius;
    const bool f64 = n.dtype == PDEHIP_F64;
    const char *type = f64 ? "double" : "float";
    const bool fits = !force_cell && a.na < kSmoothExtentMax && n.n[2] < kSmoothExtentMax;

#define PDEHIP_SMOOTH(kernel, T, blocks) \
    hipLaunchKernelGGL((kernel), dim3(blocks, ncomp), dim3(256), 0, st, a, (const T *)in_full, (T *)out_full, w)
    if (fits && a.axis == 2 && radius <= kRowRadiusMax) {
        const long pieces = n.n[0] * n.n[1] * ((n.n[2] + kRowLanes - 1) / kRowLanes);
        const unsigned blocks = clamp_blocks((pieces + kRowPieces - 1) / kRowPieces, kSmoothBlocksMax);
        if (f64) PDEHIP_SMOOTH(gauss_row_kernel<double>, double, blocks);
        else PDEHIP_SMOOTH(gauss_row_kernel<float>, float, blocks);
        note_kernel("gauss_row_kernel<%s>", type);
    } else if (fits && a.axis < 2 && radius <= kMarchRadiusMax) {
        const long tiles = a.nq * ((a.na + kMarchLength - 1) / kMarchLength) * ((n.n[2] + kMarchWidth - 1) / kMarchWidth);
        const unsigned blocks = clamp_blocks(tiles, kSmoothBlocksMax);
        const int vec = piece_width(n, in_full, out_full);      // (both arrays are on 16-byte boundaries: checked above)
        dispatch_piece(n.dtype, vec, [&](auto t, auto width) {
            typedef decltype(t) T;
            PDEHIP_SMOOTH((gauss_march_kernel<T, decltype(width)::value>), T, blocks);
        });
        note_kernel("gauss_march_kernel<%s,%d>", type, vec);
    } else {
        const unsigned blocks = blocks_for(n.n[0] * n.n[1] * n.n[2], kSmoothBlocksMax);
        if (f64) PDEHIP_SMOOTH(gauss_cell_kernel<double>, double, blocks);
        else PDEHIP_SMOOTH(gauss_cell_kernel<float>, float, blocks);
        note_kernel("gauss_cell_kernel<%s>", type);
    }
#undef PDEHIP_SMOOTH
    PDEHIP_HIP(hipGetLastError());
    return 0;
}
