// pdehip_stats.hip — statistics of a field where it lives: count, sum, extrema, mean and the sum of squared deviations of every
// component (or of the norm over the components), and the steady-state test of a state against its snapshot.
//
// Semantics: pde/fields/datafield_base.py:846-897 (integral, average, fluctuations, magnitude), pde/fields/vectorial.py:420-431 and
// pde/fields/tensorial.py:333-337 (the norm over the components), pde/trackers/trackers.py:819-844 (SteadyStateTracker.handle).
// Every sweep: workgroups of 256 threads through blocks_for, the interior rows through for_row_pieces<VEC> (16-byte loads where the row
// length allows), per wave a butterfly and one store per column into the wave's slot, then ONE workgroup that folds the slots in a
// fixed order.  No atomics: two runs give equal bits.  Compiled without FMA contraction in every build.
#include "pdehip_common.h"
#include "pdehip_pieces.h"
#include "pdehip_scratch.h"
#include "pdehip_sweep.h"

namespace pdehip {
namespace {

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

struct StatsArgs {
    RowGrid g;
    long pc;               // elements of one component
    int ncomp;             // components under the norm (1 without)
    const void *in;        // the component; with the norm: component 0
    double *sums;          // first sweep: {n_finite, n_nonfinite, sum} interleaved per slot; second sweep: m2 per slot
    double *extrema;       // {-min, max} interleaved per slot: ONE fold with the maximum serves both (a negation is exact)
    double *out;           // the block of eight of this component
};

// the values of one piece (pdehip_pieces.h): the cells themselves, or the norm over the components
template <typename T, int VEC, bool NORM>
__device__ __forceinline__ void piece_values(const StatsArgs &a, long e, T (&v)[VEC])
{
    pdehip::piece_values<T, VEC, NORM>((const T *)a.in + e, a.pc, a.ncomp, v);
}

// first sweep: the finite cells' count, sum, minimum and maximum (fp64, from values converted exactly) and the count of the others
template <typename T, int VEC, bool NORM>
__global__ void __launch_bounds__(256) stats_sweep_kernel(StatsArgs a)
{
    double cnt = 0, bad = 0, sum = 0, mn = SlotMin::identity(), mx = SlotMax::identity();
    for_row_pieces<VEC>(a.g, [&](long, long, long, long e) {
        T v[VEC];
        piece_values<T, VEC, NORM>(a, e, v);
#pragma unroll
        for (int q = 0; q < VEC; q++) {
            const double x = (double)v[q];
            const bool ok = (x - x == 0.0);   // x - x is 0 for finite x, NaN for NaN and +-inf
            cnt = cnt + (ok ? 1.0 : 0.0);
            bad = bad + (ok ? 0.0 : 1.0);
            sum = sum + (ok ? x : 0.0);
            mn = ok ? SlotMin::apply(mn, x) : mn;
            mx = ok ? SlotMax::apply(mx, x) : mx;
        }
    });
    cnt = wave_sum(cnt); bad = wave_sum(bad); sum = wave_sum(sum);
    mn = wave_min(mn); mx = wave_max(mx);
    const int slot = wave_slot();
    if ((threadIdx.x & 63) == 0 && slot < kSweepWavesMax) {
        a.sums[3 * slot] = cnt; a.sums[3 * slot + 1] = bad; a.sums[3 * slot + 2] = sum;
        a.extrema[2 * slot] = -mn; a.extrema[2 * slot + 1] = mx;
    }
}
// ... folded by one workgroup into {n_finite, n_nonfinite, sum, min, max, mean, m2 = NaN, 0}
__global__ void __launch_bounds__(256) stats_finish_kernel(StatsArgs a, int nslots)
{
    double s[3], m[2];
    sum_slots<3>(a.sums, nslots, s);
    reduce_slots<SlotMax, 2>(a.extrema, nslots, m);
    if (threadIdx.x == 0) {
        const bool any = s[0] > 0.0;
        a.out[0] = s[0]; a.out[1] = s[1]; a.out[2] = s[2];
        a.out[3] = any ? -m[0] : quiet_nan();
        a.out[4] = any ? m[1] : quiet_nan();
        a.out[5] = any ? s[2] / s[0] : quiet_nan();
        a.out[6] = quiet_nan();
        a.out[7] = 0.0;
    }
}
// second sweep: sum of (x - mean)^2 over the finite cells, the mean read from the block the first pass left (numpy's two-pass variance)
template <typename T, int VEC, bool NORM>
__global__ void __launch_bounds__(256) stats_m2_kernel(StatsArgs a)
{
    const double mean = a.out[5];
    double acc = 0;
    for_row_pieces<VEC>(a.g, [&](long, long, long, long e) {
        T v[VEC];
        piece_values<T, VEC, NORM>(a, e, v);
#pragma unroll
        for (int q = 0; q < VEC; q++) {
            const double x = (double)v[q];
            const double d = x - mean;
            acc = acc + ((x - x == 0.0) ? d * d : 0.0);
        }
    });
    acc = wave_sum(acc);
    const int slot = wave_slot();
    if ((threadIdx.x & 63) == 0 && slot < kSweepWavesMax) a.sums[slot] = acc;
}
__global__ void __launch_bounds__(256) stats_m2_finish_kernel(StatsArgs a, int nslots)
{
    double s[1];
    sum_slots<1>(a.sums, nslots, s);
    if (threadIdx.x == 0) a.out[6] = a.out[0] > 0.0 ? s[0] : quiet_nan();
}

// ---- steady state: r = |(last - cur) / elapsed| - rtol * |cur| over the finite cells of cur, and last <- cur, in one sweep -------------
struct SteadyArgs {
    RowGrid g;
    long pc;
    int ncomp;
    const void *cur;
    void *last;
    double elapsed, rtol;  // already rounded to the field's type
    double *sums;          // cells that took part, per slot
    double *maxs;          // {max r over the cells whose r is a number, 1 if an r was NaN} interleaved per slot
    double *out;
};
template <typename T, int VEC>
__global__ void __launch_bounds__(256) steady_sweep_kernel(SteadyArgs a)
{
    const T elapsed = (T)a.elapsed, rtol = (T)a.rtol;
    double cnt = 0, mx = SlotMax::identity(), nan = 0;
    for_row_pieces<VEC>(a.g, [&](long, long, long, long e) {
        for (int c = 0; c < a.ncomp; c++) {
            T x[VEC], l[VEC];
            load_piece<T, VEC>((const T *)a.cur + c * a.pc + e, x);
            load_piece<T, VEC>((const T *)a.last + c * a.pc + e, l);
            store_piece<T, VEC>((T *)a.last + c * a.pc + e, x);
#pragma unroll
            for (int q = 0; q < VEC; q++) {
                const bool ok = (x[q] - x[q] == (T)0);
                const T rate = (l[q] - x[q]) / elapsed;
                const double r = (double)(fabs(rate) - rtol * fabs(x[q]));
                const bool number = (r == r);
                cnt = cnt + (ok ? 1.0 : 0.0);
                mx = (ok && number) ? SlotMax::apply(mx, r) : mx;
                nan = (ok && !number) ? 1.0 : nan;
            }
        }
    });
    cnt = wave_sum(cnt); mx = wave_max(mx); nan = wave_max(nan);
    const int slot = wave_slot();
    if ((threadIdx.x & 63) == 0 && slot < kSweepWavesMax) {
        a.sums[slot] = cnt;
        a.maxs[2 * slot] = mx; a.maxs[2 * slot + 1] = nan;
    }
}
__global__ void __launch_bounds__(256) steady_finish_kernel(SteadyArgs a, int nslots)
{
    double s[1], m[2];
    sum_slots<1>(a.sums, nslots, s);
    reduce_slots<SlotMax, 2>(a.maxs, nslots, m);
    if (threadIdx.x == 0) {
        a.out[0] = (m[1] > 0.0 || !(s[0] > 0.0)) ? quiet_nan() : m[0];   // NaN wins like np.max; no cell at all: the host raises
        a.out[1] = s[0];
    }
}

// The slots of the sweeps: 3 + 1 + 1 columns for each of the kSweepWavesMax waves a launch has at most (1.3 MB), one buffer per STREAM
// (calls on one stream are ordered; two streams reducing at the same time must not share one: sum_scratch, pdehip_ops.hip), allocated at
// the stream's first call and kept until pdehip_release_scratch.
struct StatsScratch { double *sums, *pairs; };      // three columns of sums, two columns of extrema
int release_slots();
StreamTable<double *> g_table(release_slots);

int release_slots()
{
    return g_table.release([](double *p) { (void)hipFree(p); });   // (hipFree waits for the device: no sweep still reads the slots)
}

int stats_scratch(hipStream_t st, StatsScratch *s)
{
    return g_table.with(st, [&](double *&p) -> int {
        if (!p) PDEHIP_HIP(hipMalloc(&p, sizeof(double) * 5 * kSweepWavesMax));
        s->sums = p;
        s->pairs = p + 3L * kSweepWavesMax;
        return 0;
    });
}

template <bool NORM>
void launch_stats(const NGrid &n, int vec, unsigned blocks, hipStream_t st, const StatsArgs &a, bool second)
{
    dispatch_piece(n.dtype, vec, [&](auto type, auto width) {
        typedef decltype(type) T;
        constexpr int V = decltype(width)::value;
        if (second) hipLaunchKernelGGL((stats_m2_kernel<T, V, NORM>), dim3(blocks), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((stats_sweep_kernel<T, V, NORM>), dim3(blocks), dim3(256), 0, st, a);
    });
}

}  // namespace
}  // namespace pdehip

using namespace pdehip;

extern "C" int pdehip_field_stats(const pdehip_grid_t *g, int ncomp, const void *arr_full, int norm, int want_m2, double *out_dev, void *stream)
{
    NGrid n;
    PDEHIP_TRY(norm_grid(g, &n));
    if (!arr_full || !out_dev) PDEHIP_FAIL(E_VALUE, "field_stats: NULL pointer");
    if (ncomp < 1 || ncomp > 64) PDEHIP_FAIL(E_VALUE, "field_stats: 1..64 components");
    hipStream_t st = as_stream(stream);
    StatsScratch s;
    PDEHIP_TRY(stats_scratch(st, &s));
    const int vec = piece_width(n, arr_full, nullptr);
    const long cells = n.n[0] * n.n[1] * n.n[2];
    const unsigned blocks = blocks_for(cells / vec);
    const int nslots = (int)blocks * 4;
    StatsArgs a;
    a.g = make_row_grid(n); a.pc = n.pc; a.sums = s.sums; a.extrema = s.pairs;
    const int blocks_out = norm ? 1 : ncomp;
    for (int c = 0; c < blocks_out; c++) {
        a.ncomp = norm ? ncomp : 1;
        a.in = (const char *)arr_full + (size_t)c * n.pc * elem_size(n.dtype);
        a.out = out_dev + 8 * c;
        for (int pass = 0; pass < (want_m2 ? 2 : 1); pass++) {
            if (norm) launch_stats<true>(n, vec, blocks, st, a, pass == 1);
            else launch_stats<false>(n, vec, blocks, st, a, pass == 1);
            if (pass == 0) hipLaunchKernelGGL(stats_finish_kernel, dim3(1), dim3(256), 0, st, a, nslots);
            else hipLaunchKernelGGL(stats_m2_finish_kernel, dim3(1), dim3(256), 0, st, a, nslots);
        }
    }
    note_kernel("stats_sweep_kernel<%s,%d,%d>", n.dtype == PDEHIP_F64 ? "double" : "float", vec, norm ? 1 : 0);
    PDEHIP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pdehip_steady_state(const pdehip_grid_t *g, int ncomp, const void *cur_full, void *last_full, double elapsed, double rtol,
                                   double *out_dev, void *stream)
{
    NGrid n;
    PDEHIP_TRY(norm_grid(g, &n));
    if (!cur_full || !last_full || !out_dev) PDEHIP_FAIL(E_VALUE, "steady_state: NULL pointer");
    if (cur_full == last_full) PDEHIP_FAIL(E_VALUE, "steady_state: the snapshot must not be the state itself");
    if (ncomp < 1) PDEHIP_FAIL(E_VALUE, "steady_state: ncomp must be >= 1");
    hipStream_t st = as_stream(stream);
    StatsScratch s;
    PDEHIP_TRY(stats_scratch(st, &s));
    const int vec = piece_width(n, cur_full, last_full);
    const long cells = n.n[0] * n.n[1] * n.n[2];
    const unsigned blocks = blocks_for(cells / vec);
    SteadyArgs a;
    a.g = make_row_grid(n); a.pc = n.pc; a.ncomp = ncomp; a.cur = cur_full; a.last = last_full;
    // a Python float next to an fp32 array is rounded to fp32 first (numpy)
    a.elapsed = n.dtype == PDEHIP_F64 ? elapsed : (double)(float)elapsed;
    a.rtol = n.dtype == PDEHIP_F64 ? rtol : (double)(float)rtol;
    a.sums = s.sums; a.maxs = s.pairs; a.out = out_dev;
    dispatch_piece(n.dtype, vec, [&](auto type, auto width) {
        hipLaunchKernelGGL((steady_sweep_kernel<decltype(type), decltype(width)::value>), dim3(blocks), dim3(256), 0, st, a);
    });
    hipLaunchKernelGGL(steady_finish_kernel, dim3(1), dim3(256), 0, st, a, (int)blocks * 4);
    note_kernel("steady_sweep_kernel<%s,%d>", n.dtype == PDEHIP_F64 ? "double" : "float", vec);
    PDEHIP_HIP(hipGetLastError());
    return 0;
}
