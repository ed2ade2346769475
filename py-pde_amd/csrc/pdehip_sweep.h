// pdehip_sweep.h — what the pointwise sweeps of the device-side loops (pdehip_fixedpoint.hip, pdehip_poisson.hip, pdehip_poisson_mg.hip)
// and of the analysis kernels (pdehip_stats.hip, pdehip_hist.hip, pdehip_project.hip; pdehip_smooth.hip takes the clamp) share in the
// offline build: the row loop, alone and with loads in flight, the launch geometry, the final sum, minimum or maximum of the wave partials
// (wave_partials, pdehip_device.h, is the other half) and the read-back of a control block.
#pragma once

#include "pdehip_common.h"

namespace pdehip {

// interior cell (i, j, k) of an array in the ghost-padded layout of norm_grid: element off + i * p0 + j * p1 + k
struct RowGrid {
    long n0, n1, n2;       // cells (normalised axes; 1 on axes the grid does not have)
    long p0, p1, off;      // pitches and the offset of cell (0, 0, 0)
};
inline RowGrid make_row_grid(const NGrid &n) { return RowGrid{n.n[0], n.n[1], n.n[2], n.p[0], n.p[1], n.off}; }

// A thread takes VEC cells of a row (16-byte accesses where the row length is even), pieces in a grid-stride loop: a fixed order per
// thread.  fn(i, j, k, element of the first cell of the piece).
template <int VEC, class F>
__device__ __forceinline__ void for_row_pieces(const RowGrid &g, F &&fn)
{
    const long per_row = g.n2 / VEC;
    const long total = g.n0 * g.n1 * per_row;
    for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        long rest = t;
        const long k = (rest % per_row) * VEC; rest /= per_row;
        const long j = rest % g.n1;
        const long i = rest / g.n1;
        fn(i, j, k, g.off + i * g.p0 + j * g.p1 + k);
    }
}
// The row loop of for_row_pieces<VEC> with the loads of kAhead pieces issued before the first of them is used: what is done per cell
// there (pdehip_hist.hip: a search, votes, LDS adds) is long enough to leave the memory idle behind a single load per thread.
// load(element, values) fills the values of a piece, use(values) consumes them; the order per thread is fixed.
constexpr int kAhead = 4;
template <typename T, int VEC, class L, class U>
__device__ __forceinline__ void for_row_pieces_ahead(const RowGrid &g, L &&load, U &&use)
{
    const long per_row = g.n2 / VEC;
    const long total = g.n0 * g.n1 * per_row;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += kAhead * stride) {
        T v[kAhead][VEC];
#pragma unroll
        for (int u = 0; u < kAhead; u++) {
            const long tu = t + u * stride < total ? t + u * stride : t;      // (past the end: the first piece once more, not used)
            long rest = tu;
            const long k = (rest % per_row) * VEC; rest /= per_row;
            const long j = rest % g.n1;
            const long i = rest / g.n1;
            load(g.off + i * g.p0 + j * g.p1 + k, v[u]);
        }
#pragma unroll
        for (int u = 0; u < kAhead; u++)
            if (t + u * stride < total) use(v[u]);
    }
}
__device__ __forceinline__ int wave_slot() { return (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); }

// workgroups of 256 threads for `items` pieces; the cap bounds the waves of a launch and with them the slots a loop needs
constexpr long kSweepBlocksMax = 8192;
constexpr int kSweepWavesMax = (int)(kSweepBlocksMax * (256 / 64));
inline unsigned clamp_blocks(long wanted, long cap) { return (unsigned)(wanted < 1 ? 1 : (wanted > cap ? cap : wanted)); }
inline unsigned blocks_for(long items, long cap = kSweepBlocksMax) { return clamp_blocks((items + 255) / 256, cap); }
// launch of a row sweep over `cells` cells: `kernel` names its instance with VEC, which is 2 where the row length is even, else 1
#define PDEHIP_LAUNCH_ROWS(even, cells, st, kernel, ...)                                                                              \
    do {                                                                                                                             \
        if (even) { constexpr int VEC = 2; hipLaunchKernelGGL((kernel), dim3(blocks_for((cells) / 2)), dim3(256), 0, as_stream(st), __VA_ARGS__); } \
        else { constexpr int VEC = 1; hipLaunchKernelGGL((kernel), dim3(blocks_for(cells)), dim3(256), 0, as_stream(st), __VA_ARGS__); }            \
        PDEHIP_HIP(hipGetLastError());                                                                                               \
    } while (0)

// The final sums of N interleaved columns of wave partials by ONE workgroup of 256 threads: thread i adds the slots i, i + 256, ... in
// that order, then a tree over the 256 sums in LDS - the same order in every run.  Every thread returns with the sums.
template <int N>
__device__ __forceinline__ void sum_slots(const double *slots, int n, double (&out)[N])
{
    __shared__ double part[N][256];
#pragma unroll
    for (int q = 0; q < N; q++) out[q] = 0;
    for (int i = threadIdx.x; i < n; i += 256)
#pragma unroll
        for (int q = 0; q < N; q++) out[q] = out[q] + slots[N * i + q];
#pragma unroll
    for (int q = 0; q < N; q++) part[q][threadIdx.x] = out[q];
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w)
#pragma unroll
            for (int q = 0; q < N; q++) part[q][threadIdx.x] = part[q][threadIdx.x] + part[q][threadIdx.x + w];
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < N; q++) out[q] = part[q][0];
}
// ---- minimum / maximum: the same two halves as wave_sum (pdehip_device.h) and sum_slots.  A minimum or maximum does not depend on the
// order, so the bits are those of any other order; the operands must not be NaN (the callers select finite values, or flag a NaN in a
// column of its own).
struct SlotMin {
    __device__ static double identity() { return __longlong_as_double(0x7ff0000000000000LL); }    // +inf
    __device__ static double apply(double a, double b) { return b < a ? b : a; }
};
struct SlotMax {
    __device__ static double identity() { return __longlong_as_double((long long)0xfff0000000000000ULL); }    // -inf
    __device__ static double apply(double a, double b) { return b > a ? b : a; }
};
template <class OP>
__device__ __forceinline__ double wave_reduce(double v)
{
#pragma unroll
    for (int ofs = 32; ofs >= 1; ofs >>= 1) v = OP::apply(v, __shfl_xor(v, ofs, 64));
    return v;
}
__device__ __forceinline__ double wave_min(double v) { return wave_reduce<SlotMin>(v); }
__device__ __forceinline__ double wave_max(double v) { return wave_reduce<SlotMax>(v); }
// OP over N interleaved columns of wave results by ONE workgroup of 256 threads; every thread returns with the results
template <class OP, int N>
__device__ __forceinline__ void reduce_slots(const double *slots, int n, double (&out)[N])
{
    __shared__ double part[N][256];
#pragma unroll
    for (int q = 0; q < N; q++) out[q] = OP::identity();
    // four slots per round: the loads of a round do not wait for one another (a fold of 32768 slots is 32 rounds instead of 128)
    for (int i = threadIdx.x; i < n; i += 4 * 256) {
        double v[4][N];
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int q = 0; q < N; q++) v[u][q] = (i + 256 * u < n) ? slots[N * (i + 256 * u) + q] : OP::identity();
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int q = 0; q < N; q++) out[q] = OP::apply(out[q], v[u][q]);
    }
#pragma unroll
    for (int q = 0; q < N; q++) part[q][threadIdx.x] = out[q];
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w)
#pragma unroll
            for (int q = 0; q < N; q++) part[q][threadIdx.x] = OP::apply(part[q][threadIdx.x], part[q][threadIdx.x + w]);
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < N; q++) out[q] = part[q][0];
}
// slots a one-workgroup kernel sums: what the last sweep announced, as far as the buffer holds it
__device__ __forceinline__ int ctl_nslots(const CtlHead &h) { return h.nslots < h.capacity ? h.nslots : h.capacity; }

// a control block read back through pinned memory: the one host synchronisation of a batch
inline int read_ctl(void *host, void *pinned, const void *dev, size_t bytes, void *st)
{
    PDEHIP_HIP(hipMemcpyAsync(pinned, dev, bytes, hipMemcpyDeviceToHost, as_stream(st)));
    PDEHIP_HIP(hipStreamSynchronize(as_stream(st)));
    memcpy(host, pinned, bytes);
    return 0;
}

}  // namespace pdehip
