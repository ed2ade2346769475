// pdehip_hist.hip — the distribution of a field where it lives: the histogram of every component (or of the norm over the components)
// over given edges, and the exact order statistics behind quantiles and the median.
//
// Semantics: include/pdehip.h.  Both results are integers or elements of the field, so they do not depend on any order of evaluation: two
// runs give equal bits although the partial counts of the workgroups are folded with 64-bit integer adds in global memory.
// Every sweep: workgroups of 256 threads, the interior rows in the order of for_row_pieces<VEC> (16-byte loads where the row length allows, four pieces in flight per thread),
// 32-bit counters in LDS; lanes of a wave that hit the same counter are combined before the LDS add (a two-phase field puts nearly every
// cell in two bins, a field of equal values puts every digit of the selection in one bucket).  Compiled without FMA contraction in every
// build, like the statistics (the norm over the components is evaluated the same way).
#include "pdehip_common.h"
#include "pdehip_pieces.h"
#include "pdehip_scratch.h"
#include "pdehip_sweep.h"

namespace pdehip {
namespace {

constexpr int kHistBinsMax = 4096;
constexpr int kSelectQMax = 8;
constexpr int kSelectTargets = 2 * kSelectQMax;      // rank k and rank min(k + 1, n - 1) of every q
constexpr int kSelectDigits = 256;                   // 8-bit digits: 8 sweeps for fp64, 4 for fp32

// Workgroups of a sweep.  Every workgroup ends with one 64-bit add per non-zero counter, so the cap is lower than that of the statistics
// and lower still where a workgroup has thousands of counters; 2048 workgroups are 8 waves per SIMD on 256 CUs.
inline unsigned hist_blocks(long pieces, int counters)
{
    return blocks_for(pieces, counters > 1024 ? 768 : 2048);
}

// One more cell for counter `slot` (lanes with !active only take part in the votes).  Two rounds in which the lanes that share the slot
// of the first remaining lane are counted by ONE add, then one add per lane that is left: one or two values that dominate cost one or
// two adds per wave instead of 64 adds to one address, a spread-out field pays two votes.  All lanes of the wave that are in the
// loop call it together.
__device__ __forceinline__ void lds_count(unsigned *cnt, int slot, bool active)
{
#pragma unroll
    for (int r = 0; r < 2; r++) {
        if (active) {
            const int first = __builtin_amdgcn_readfirstlane(slot);
            const bool same = slot == first;
            const unsigned long long m = __ballot(same);
            if (same) {
                const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                if (below == 0) atomicAdd(&cnt[first], (unsigned)__popcll(m));
                active = false;
            }
        }
    }
    if (active) atomicAdd(&cnt[slot], 1u);
}

// ---- histogram --------------------------------------------------------------------------------------------------------------------------
struct HistArgs {
    RowGrid g;
    long pc;                       // elements of one component
    int ncomp;                     // components under the norm (1 without)
    int nbins;
    const void *in;                // component 0; without the norm workgroup row blockIdx.y takes component blockIdx.y
    const double *edges;           // nbins + 1
    unsigned long long *counts;    // nbins + 3 per block: the bins, below, above, NaN (zeroed before the launch)
    double e0, inv_w;              // equal bins: the guess is (x - e0) * inv_w
};

// LDS: nbins + 1 edges (fp64), then nbins + 3 counters (32 bits: a workgroup counts fewer than 2^32 cells) - 49 172 bytes at 4096 bins.
template <typename T, int VEC, bool NORM, bool UNIFORM>
__global__ void __launch_bounds__(256, 8) hist_sweep_kernel(HistArgs a)   // (8 waves per SIMD: at most 64 vector registers)
{
    extern __shared__ double hist_lds[];
    const int nb = a.nbins;
    double *edge = hist_lds;
    unsigned *cnt = (unsigned *)(hist_lds + nb + 1);
    for (int i = threadIdx.x; i <= nb; i += 256) edge[i] = a.edges[i];
    for (int i = threadIdx.x; i < nb + 3; i += 256) cnt[i] = 0;
    __syncthreads();
    const double lo = edge[0], hi = edge[nb];
    const T *in = (const T *)a.in + (NORM ? 0L : (long)blockIdx.y * a.pc);
    for_row_pieces_ahead<T, VEC>(a.g, [&](long e, T (&v)[VEC]) { piece_values<T, VEC, NORM>(in + e, a.pc, a.ncomp, v); }, [&](const T (&v)[VEC]) {
#pragma unroll
        for (int q = 0; q < VEC; q++) {
            const double x = (double)v[q];
            int b;
            if (x != x) {
                b = nb + 2;
            } else if (x < lo) {
                b = nb;
            } else if (x > hi) {
                b = nb + 1;
            } else if (UNIFORM) {
                // a guess from the scaled distance, settled by the edges themselves: e[b] <= x < e[b + 1], the last bin closed
                b = (int)fmin((x - a.e0) * a.inv_w, (double)(nb - 1));
                while (b > 0 && x < edge[b]) b--;
                while (b < nb - 1 && x >= edge[b + 1]) b++;
            } else {
                // the largest b in [0, nbins - 1] with e[b] <= x
                int l = 0, h = nb - 1;
                while (l < h) {
                    const int mid = (l + h + 1) >> 1;
                    if (edge[mid] <= x) l = mid; else h = mid - 1;
                }
                b = l;
            }
            lds_count(cnt, b, true);
        }
    });
    __syncthreads();
    unsigned long long *out = a.counts + (size_t)blockIdx.y * (nb + 3);
    for (int i = threadIdx.x; i < nb + 3; i += 256) {
        const unsigned c = cnt[i];
        if (c) atomicAdd(&out[i], (unsigned long long)c);
    }
}

// ---- selection: radix selection on the order-preserving integer image of the value bits ----------------------------------------------------
template <typename T> struct KeyOf;
template <> struct KeyOf<double> { typedef unsigned long long type; };
template <> struct KeyOf<float> { typedef unsigned type; };
// a < b as numbers <=> key(a) < key(b) as unsigned integers (-0 sorts before +0; NaN never gets here)
__device__ __forceinline__ unsigned long long order_key(double x)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}
__device__ __forceinline__ unsigned order_key(float x)
{
    const unsigned u = __float_as_uint(x);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
template <typename K>
__device__ __forceinline__ K key_bits(K key)
{
    const K sign = (K)1 << (sizeof(K) * 8 - 1);
    return (key & sign) ? (key ^ sign) : (K)~key;
}

// The control block of one block of results (a component, or the norm), in device memory: the host never reads it.  A TARGET is one rank
// to find (two per q); targets whose leading digits agree so far form a GROUP and share one row of digit counts.
struct SelectCtl {
    unsigned long long hist[kSelectTargets][kSelectDigits];   // per group: the cells with the group's prefix, by their next digit
    unsigned long long n, n_nan;
    unsigned long long prefix[kSelectTargets];                // per group: the leading digits found so far
    unsigned long long rank[kSelectTargets];                  // per target: its rank among the cells with its group's prefix
    int group_of[kSelectTargets];
    int ngroups, ntargets;
};
struct SelectArgs {
    RowGrid g;
    long pc;
    int ncomp;
    int pass;
    const void *in;
    SelectCtl *ctl;                // one per block; workgroup row blockIdx.y takes block blockIdx.y
};
struct SelectQ {
    double q[kSelectQMax];
    int nq;
};

// One pass: the counts of digit `pass` (from the top) over the cells whose leading digits equal a group's prefix; the first pass also counts
// the NaN cells.  LDS: 16 x 256 counters and one for NaN, 16 388 bytes.
template <typename T, int VEC, bool NORM>
__global__ void __launch_bounds__(256, 8) select_sweep_kernel(SelectArgs a)   // (8 waves per SIMD: at most 64 vector registers)
{
    typedef typename KeyOf<T>::type K;
    constexpr int BITS = (int)sizeof(K) * 8;
    constexpr int NAN_SLOT = kSelectTargets * kSelectDigits;
    __shared__ unsigned cnt[NAN_SLOT + 1];
    __shared__ K prefix[kSelectTargets];
    SelectCtl *ctl = a.ctl + blockIdx.y;
    const bool first = a.pass == 0;
    const int ng = first ? 1 : ctl->ngroups;
    if (ng == 0) return;                       // no cell that is a number: nothing to select
    for (int i = threadIdx.x; i < ng * kSelectDigits; i += 256) cnt[i] = 0;
    if (threadIdx.x == 0) cnt[NAN_SLOT] = 0;
    if ((int)threadIdx.x < ng) prefix[threadIdx.x] = first ? (K)0 : (K)ctl->prefix[threadIdx.x];
    __syncthreads();
    const int shift = BITS - 8 * (a.pass + 1);
    const T *in = (const T *)a.in + (NORM ? 0L : (long)blockIdx.y * a.pc);
    for_row_pieces_ahead<T, VEC>(a.g, [&](long e, T (&v)[VEC]) { piece_values<T, VEC, NORM>(in + e, a.pc, a.ncomp, v); }, [&](const T (&v)[VEC]) {
#pragma unroll
        for (int q = 0; q < VEC; q++) {
            const T x = v[q];
            const bool nan = x != x;
            const K key = order_key(x);
            const K lead = first ? (K)0 : (K)(key >> ((shift + 8) & (BITS - 1)));
            int row = -1;
            for (int gi = 0; gi < ng; gi++) row = (lead == prefix[gi]) ? gi : row;
            int slot = row * kSelectDigits + (int)((key >> shift) & (K)(kSelectDigits - 1));
            bool active = !nan && row >= 0;
            if (first && nan) { slot = NAN_SLOT; active = true; }
            lds_count(cnt, slot, active);
        }
    });
    __syncthreads();
    unsigned long long *out = &ctl->hist[0][0];
    for (int i = threadIdx.x; i < ng * kSelectDigits; i += 256) {
        const unsigned c = cnt[i];
        if (c) atomicAdd(&out[i], (unsigned long long)c);
    }
    if (threadIdx.x == 0 && cnt[NAN_SLOT]) atomicAdd(&ctl->n_nan, (unsigned long long)cnt[NAN_SLOT]);
}

// inclusive sums over the 256 threads of the workgroup; buf[255] is the total for every thread afterwards
__device__ __forceinline__ unsigned long long scan256(unsigned long long c, unsigned long long *buf)
{
    __syncthreads();
    buf[threadIdx.x] = c;
    __syncthreads();
    for (int ofs = 1; ofs < 256; ofs <<= 1) {
        const unsigned long long below = (int)threadIdx.x >= ofs ? buf[threadIdx.x - ofs] : 0;
        __syncthreads();
        buf[threadIdx.x] += below;
        __syncthreads();
    }
    return buf[threadIdx.x];
}

// Behind each pass, ONE workgroup per block: the first pass fixes n and the ranks (k = floor((n - 1) * q) in fp64 and min(k + 1, n - 1));
// every pass finds, per target, the digit whose bucket holds its rank, the rank inside that bucket, and the groups of the next pass; the
// last pass writes the elements.  The host takes no part between the passes.
template <typename T>
__global__ void __launch_bounds__(256) select_scan_kernel(SelectCtl *ctls, int pass, int npasses, SelectQ q, T *lower, T *upper,
                                                          unsigned long long *info)
{
    typedef typename KeyOf<T>::type K;
    __shared__ unsigned long long buf[256];
    __shared__ unsigned long long s_rank[kSelectTargets], s_prefix[kSelectTargets], s_new[kSelectTargets];
    __shared__ unsigned long long s_next[kSelectTargets];     // the prefixes of the next pass's groups (LDS: indexed at run time)
    __shared__ int s_group[kSelectTargets], s_digit[kSelectTargets];
    SelectCtl *ctl = ctls + blockIdx.x;
    const int tid = threadIdx.x;
    const int ng_old = pass == 0 ? 1 : ctl->ngroups;
    int nt;
    if (pass == 0) {
        scan256(ctl->hist[0][tid], buf);
        const unsigned long long n = buf[255];
        nt = n ? 2 * q.nq : 0;
        if (tid < nt) {
            const double v = (double)(n - 1) * q.q[tid >> 1];
            unsigned long long k = (unsigned long long)floor(v);
            k = k > n - 1 ? n - 1 : k;
            if ((tid & 1) && k < n - 1) k++;
            s_rank[tid] = k;
            s_group[tid] = 0;
        }
        if (tid == 0) {
            s_prefix[0] = 0;
            ctl->n = n;
            info[2 * blockIdx.x] = n;
            info[2 * blockIdx.x + 1] = ctl->n_nan;
        }
    } else {
        nt = ctl->ntargets;
        if (tid < nt) { s_rank[tid] = ctl->rank[tid]; s_group[tid] = ctl->group_of[tid]; }
        if (tid < ng_old) s_prefix[tid] = ctl->prefix[tid];
    }
    if (tid < kSelectTargets) { s_digit[tid] = 0; s_new[tid] = 0; }
    __syncthreads();
    for (int t = 0; t < nt; t++) {
        const unsigned long long r = s_rank[t];
        const unsigned long long c = ctl->hist[s_group[t]][tid];
        const unsigned long long upto = scan256(c, buf);
        if (c != 0 && upto - c <= r && r < upto) { s_digit[t] = tid; s_new[t] = r - (upto - c); }    // exactly one thread
    }
    __syncthreads();
    if (tid == 0) {
        const bool last = pass == npasses - 1;
        int ng = 0;
        for (int t = 0; t < nt; t++) {
            const unsigned long long p = (s_prefix[s_group[t]] << 8) | (unsigned long long)s_digit[t];
            int gi = 0;
            while (gi < ng && s_next[gi] != p) gi++;
            if (gi == ng) { s_next[ng] = p; ctl->prefix[ng] = p; ng++; }
            ctl->group_of[t] = gi;
            ctl->rank[t] = s_new[t];
            if (last) {
                const K bits = key_bits<K>((K)p);
                K *dst = (K *)((t & 1) ? upper : lower) + (size_t)blockIdx.x * q.nq + (t >> 1);
                *dst = bits;
            }
        }
        ctl->ngroups = ng;
        ctl->ntargets = nt;
        if (last && nt == 0) {
            const K nan = sizeof(K) == 8 ? (K)0x7ff8000000000000ULL : (K)0x7fc00000u;
            for (int j = 0; j < q.nq; j++) {
                ((K *)lower)[(size_t)blockIdx.x * q.nq + j] = nan;
                ((K *)upper)[(size_t)blockIdx.x * q.nq + j] = nan;
            }
        }
    }
    // the rows of this pass are zero again for the next one (every read of them lies before the barrier above)
    for (int gi = 0; gi < ng_old; gi++) ctl->hist[gi][tid] = 0;
}

// ---- per stream: pinned host memory for the edges of a call (they are checked on the host) and the control blocks of the selection;
// allocated at the stream's first call, kept until pdehip_release_scratch -------------------------------------------------------------------
struct HistScratch { double *edges_host; SelectCtl *ctl; };
int release_blocks();
StreamTable<HistScratch> g_table(release_blocks);

int release_blocks()
{
    return g_table.release([](HistScratch &h) {
        (void)hipFree(h.ctl);                  // (hipFree waits for the device: no pass still uses the control blocks)
        (void)hipHostFree(h.edges_host);
    });
}

int hist_scratch(hipStream_t st, HistScratch *s)
{
    return g_table.with(st, [&](HistScratch &h) -> int {
        if (!h.ctl) {
            PDEHIP_HIP(hipHostMalloc((void **)&h.edges_host, sizeof(double) * (kHistBinsMax + 1), hipHostMallocDefault));
            const hipError_t e = hipMalloc((void **)&h.ctl, sizeof(SelectCtl) * 64);
            if (e != hipSuccess) {
                (void)hipHostFree(h.edges_host);
                h.edges_host = nullptr; h.ctl = nullptr;
                PDEHIP_FAIL(100 + (int)e, "hipMalloc of the selection's control blocks failed: %s", hipGetErrorString(e));
            }
        }
        *s = h;
        return 0;
    });
}

template <bool NORM, bool UNIFORM>
void launch_hist(const NGrid &n, int vec, dim3 grid, size_t lds, hipStream_t st, const HistArgs &a)
{
    dispatch_piece(n.dtype, vec, [&](auto type, auto width) {
        hipLaunchKernelGGL((hist_sweep_kernel<decltype(type), decltype(width)::value, NORM, UNIFORM>), grid, dim3(256), lds, st, a);
    });
}

template <bool NORM>
void launch_select(const NGrid &n, int vec, dim3 grid, hipStream_t st, const SelectArgs &a)
{
    dispatch_piece(n.dtype, vec, [&](auto type, auto width) {
        hipLaunchKernelGGL((select_sweep_kernel<decltype(type), decltype(width)::value, NORM>), grid, dim3(256), 0, st, a);
    });
}

}  // namespace
}  // namespace pdehip

using namespace pdehip;

extern "C" int pdehip_histogram(const pdehip_grid_t *g, int ncomp, const void *arr_full, int norm, int nbins, const double *edges_dev,
                                uint64_t *counts_dev, void *stream)
{
    NGrid n;
    PDEHIP_TRY(norm_grid(g, &n));
    if (!arr_full || !edges_dev || !counts_dev) PDEHIP_FAIL(E_VALUE, "histogram: NULL pointer");
    if (ncomp < 1 || ncomp > 64) PDEHIP_FAIL(E_VALUE, "histogram: 1..64 components");
    if (nbins < 1 || nbins > kHistBinsMax) PDEHIP_FAIL(E_VALUE, "histogram: 1..%d bins (got %d)", kHistBinsMax, nbins);
    if (((uintptr_t)arr_full & 15) != 0 || (((uintptr_t)edges_dev | (uintptr_t)counts_dev) & 7) != 0)
        PDEHIP_FAIL(E_VALUE, "histogram: misaligned array (16 bytes for the field, 8 for the edges and the counts)");
    hipStream_t st = as_stream(stream);
    HistScratch s;
    PDEHIP_TRY(hist_scratch(st, &s));
    // the edges decide every count: they are checked here, on the host (at most 32 KB come down; the caller waits for the counts anyway)
    double *e = s.edges_host;
    PDEHIP_HIP(hipMemcpyAsync(e, edges_dev, sizeof(double) * (nbins + 1), hipMemcpyDeviceToHost, st));
    PDEHIP_HIP(hipStreamSynchronize(st));
    for (int i = 0; i <= nbins; i++) {
        if (!std::isfinite(e[i])) PDEHIP_FAIL(E_VALUE, "histogram: edge %d is not finite", i);
        if (i > 0 && !(e[i] > e[i - 1])) PDEHIP_FAIL(E_VALUE, "histogram: the edges must increase strictly (edge %d)", i);
    }
    // equal bins: every edge within a quarter of a bin of its place, so that the guess is off by one bin at the most
    const double width = (e[nbins] - e[0]) / nbins;
    const double inv_w = 1.0 / width;
    bool uniform = std::isfinite(width) && std::isfinite(inv_w) && width > 0.0;
    for (int i = 1; i < nbins && uniform; i++) uniform = std::fabs(e[i] - (e[0] + i * width)) <= 0.25 * width;

    const int blocks_out = norm ? 1 : ncomp;
    const int vec = piece_width(n, arr_full, nullptr);
    const long cells = n.n[0] * n.n[1] * n.n[2];
    HistArgs a;
    a.g = make_row_grid(n); a.pc = n.pc; a.ncomp = norm ? ncomp : 1; a.nbins = nbins; a.in = arr_full; a.edges = edges_dev;
    a.counts = (unsigned long long *)counts_dev; a.e0 = e[0]; a.inv_w = inv_w;
    PDEHIP_HIP(hipMemsetAsync(counts_dev, 0, sizeof(uint64_t) * (size_t)blocks_out * (nbins + 3), st));
    const dim3 grid(hist_blocks(cells / vec, nbins + 3), blocks_out);
    const size_t lds = sizeof(double) * (nbins + 1) + sizeof(unsigned) * (nbins + 3);
    if (norm) {
        if (uniform) launch_hist<true, true>(n, vec, grid, lds, st, a); else launch_hist<true, false>(n, vec, grid, lds, st, a);
    } else {
        if (uniform) launch_hist<false, true>(n, vec, grid, lds, st, a); else launch_hist<false, false>(n, vec, grid, lds, st, a);
    }
    note_kernel("hist_sweep_kernel<%s,%d,%d,%d>", n.dtype == PDEHIP_F64 ? "double" : "float", vec, norm ? 1 : 0, uniform ? 1 : 0);
    PDEHIP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pdehip_quantile_select(const pdehip_grid_t *g, int ncomp, const void *arr_full, int norm, int nq, const double *q_host,
                                      void *lower_dev, void *upper_dev, uint64_t *info_dev, void *stream)
{
    NGrid n;
    PDEHIP_TRY(norm_grid(g, &n));
    if (!arr_full || !q_host || !lower_dev || !upper_dev || !info_dev) PDEHIP_FAIL(E_VALUE, "quantile_select: NULL pointer");
    if (ncomp < 1 || ncomp > 64) PDEHIP_FAIL(E_VALUE, "quantile_select: 1..64 components");
    if (nq < 1 || nq > kSelectQMax) PDEHIP_FAIL(E_VALUE, "quantile_select: 1..%d quantiles in one call (got %d)", kSelectQMax, nq);
    const uintptr_t esize = (uintptr_t)elem_size(n.dtype);
    if (((uintptr_t)arr_full & 15) != 0 || (((uintptr_t)lower_dev | (uintptr_t)upper_dev) & (esize - 1)) != 0 || ((uintptr_t)info_dev & 7) != 0)
        PDEHIP_FAIL(E_VALUE, "quantile_select: misaligned array (16 bytes for the field, the element size for the results, 8 for the counts)");
    SelectQ q;
    memset(&q, 0, sizeof(q));
    q.nq = nq;
    for (int j = 0; j < nq; j++) {
        if (!(q_host[j] >= 0.0 && q_host[j] <= 1.0)) PDEHIP_FAIL(E_VALUE, "quantile_select: q[%d] = %g is not in [0, 1]", j, q_host[j]);
        q.q[j] = q_host[j];
    }
    hipStream_t st = as_stream(stream);
    HistScratch s;
    PDEHIP_TRY(hist_scratch(st, &s));
    const int blocks_out = norm ? 1 : ncomp;
    const int vec = piece_width(n, arr_full, nullptr);
    const long cells = n.n[0] * n.n[1] * n.n[2];
    const bool f64 = n.dtype == PDEHIP_F64;
    const int npasses = f64 ? 8 : 4;
    SelectArgs a;
    a.g = make_row_grid(n); a.pc = n.pc; a.ncomp = norm ? ncomp : 1; a.in = arr_full; a.ctl = s.ctl;
    PDEHIP_HIP(hipMemsetAsync(s.ctl, 0, sizeof(SelectCtl) * blocks_out, st));
    const dim3 grid(hist_blocks(cells / vec, kSelectDigits), blocks_out);
    for (int pass = 0; pass < npasses; pass++) {
        a.pass = pass;
        if (norm) launch_select<true>(n, vec, grid, st, a); else launch_select<false>(n, vec, grid, st, a);
        if (f64)
            hipLaunchKernelGGL((select_scan_kernel<double>), dim3(blocks_out), dim3(256), 0, st, s.ctl, pass, npasses, q, (double *)lower_dev,
                               (double *)upper_dev, (unsigned long long *)info_dev);
        else
            hipLaunchKernelGGL((select_scan_kernel<float>), dim3(blocks_out), dim3(256), 0, st, s.ctl, pass, npasses, q, (float *)lower_dev,
                               (float *)upper_dev, (unsigned long long *)info_dev);
    }
    note_kernel("select_sweep_kernel<%s,%d,%d>", f64 ? "double" : "float", vec, norm ? 1 : 0);
    PDEHIP_HIP(hipGetLastError());
    return 0;
}
