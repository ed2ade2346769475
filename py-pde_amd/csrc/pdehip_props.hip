// pdehip_props.hip — where every domain of a labelling is, what box it fills and how much of the field it holds: per label the anchor (its
// first cell in C order), the sums of the cells' offsets from the anchor, the smallest and largest offset per axis and a fixed-point sum
// of the field in two 64-bit limbs.
//
// Semantics: include/pdehip.h.  Why offsets from an anchor, why limbs, which accesses are atomic: DESIGN.md §4.15b.  In short:
//   (a) props_init_kernel    anchors to INT32_MAX, boxes to (INT32_MAX, INT32_MIN), everything else to zero
//   (b) props_anchor_kernel  anchor[k] = the smallest linear cell index with label k + 1: one atomicMin per (wave, label); labels outside
//                            0 ... ndomains are counted here and never used as an index
//   (c) props_sum_kernel<T>  per cell the offsets d_a from the domain's anchor (minimal image on periodic axes) and, with a field, the
//                            two integers hi, lo of its value; the lanes of a wave that share a label are combined by a masked wave
//                            reduction and a wave keeps the label it met last with its partial results in registers, as
//                            domain_sizes_kernel does (pdehip_label.hip): one percolating domain costs one flush per wave
// Everything that is added, minimised or maximised across waves is an integer: the results do not depend on the order in which workgroups
// run, there is no floating-point atomic anywhere.  No kernel waits for another workgroup; between the kernels there is stream order.
#include "pdehip_common.h"
#include "pdehip_scratch.h"
#include "pdehip_sweep.h"

namespace pdehip {
namespace {

constexpr long kPropsBlocksMax = 4096;          // the cap of domain_sizes_kernel: more workgroups only mean more flushes of a held label
constexpr int kIntMax = 2147483647, kIntMin = -2147483647 - 1;

struct PropsArgs {
    int n0, n1, n2;                // interior cells of the normalised axes
    int per0, per1, per2;          // periodic axes (never a padded axis)
    long p0, p1, off;              // pitches and the first interior cell of the field's device layout
    long cells, ndomains;
    int eh, el;                    // exponents of the two limbs
    double absmax;
    const void *in;                // NULL: no limbs
    const int *labels;
    int *anchor;
    long long *moment;
    int *box;
    long long *limb;
    unsigned *excluded;
};

// ---- relaxed agent-scope atomics on the words other workgroups add to in the same launch ---------------------------------------------------
__device__ __forceinline__ void add64(long long *p, long long v)
{
    if (v) (void)__hip_atomic_fetch_add((unsigned long long *)p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void min32(int *p, int v) { (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void max32(int *p, int v) { (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- integer wave reductions: every lane returns with the result ---------------------------------------------------------------------------
__device__ __forceinline__ long long wave_add(long long v)
{
#pragma unroll
    for (int ofs = 32; ofs >= 1; ofs >>= 1) v += __shfl_xor(v, ofs, 64);
    return v;
}
__device__ __forceinline__ int wave_imin(int v)
{
#pragma unroll
    for (int ofs = 32; ofs >= 1; ofs >>= 1) { const int o = __shfl_xor(v, ofs, 64); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ int wave_imax(int v)
{
#pragma unroll
    for (int ofs = 32; ofs >= 1; ofs >>= 1) { const int o = __shfl_xor(v, ofs, 64); v = o > v ? o : v; }
    return v;
}

// what one label has collected: sums of offsets, smallest and largest offset, the limbs, the cells left out of them
struct Part {
    long long m0, m1, m2, lh, ll;
    int lo0, lo1, lo2, hi0, hi1, hi2;
    unsigned ex;
};
__device__ __forceinline__ void merge(Part &h, const Part &p)
{
    h.m0 += p.m0; h.m1 += p.m1; h.m2 += p.m2; h.lh += p.lh; h.ll += p.ll;
    h.lo0 = p.lo0 < h.lo0 ? p.lo0 : h.lo0; h.lo1 = p.lo1 < h.lo1 ? p.lo1 : h.lo1; h.lo2 = p.lo2 < h.lo2 ? p.lo2 : h.lo2;
    h.hi0 = p.hi0 > h.hi0 ? p.hi0 : h.hi0; h.hi1 = p.hi1 > h.hi1 ? p.hi1 : h.hi1; h.hi2 = p.hi2 > h.hi2 ? p.hi2 : h.hi2;
    h.ex += p.ex;
}
// one set of atomics for label `lab` (1 ... ndomains), by ONE lane
template <bool FIELD>
__device__ __forceinline__ void flush(const PropsArgs &a, int lab, const Part &p)
{
    const long k = lab - 1;
    add64(a.moment + 3 * k, p.m0); add64(a.moment + 3 * k + 1, p.m1); add64(a.moment + 3 * k + 2, p.m2);
    int *b = a.box + 6 * k;
    min32(b, p.lo0); max32(b + 1, p.hi0); min32(b + 2, p.lo1); max32(b + 3, p.hi1); min32(b + 4, p.lo2); max32(b + 5, p.hi2);
    if (FIELD) {
        add64(a.limb + 2 * k, p.lh); add64(a.limb + 2 * k + 1, p.ll);
        if (p.ex) (void)__hip_atomic_fetch_add(a.excluded + k, p.ex, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
// The lanes with `in` combined; `src` is the first of them.  Where all of them lie in one row (the usual case: cells are taken in C order)
// only the offset along the fastest axis varies by lane: the other two sums are count x offset.
template <bool FIELD>
__device__ __forceinline__ Part combine(bool in, int src, int row, const Part &mine)
{
    Part p;
    const unsigned long long m = __ballot(in);
    const long long cnt = __popcll(m);
    const bool one_row = __ballot(in && row != __shfl(row, src)) == 0;
    if (one_row) {
        const int d0 = __shfl(mine.lo0, src), d1 = __shfl(mine.lo1, src);
        p.m0 = cnt * d0; p.m1 = cnt * d1;
        p.lo0 = p.hi0 = d0; p.lo1 = p.hi1 = d1;
    } else {
        p.m0 = wave_add(in ? mine.m0 : 0); p.m1 = wave_add(in ? mine.m1 : 0);
        p.lo0 = wave_imin(in ? mine.lo0 : kIntMax); p.hi0 = wave_imax(in ? mine.hi0 : kIntMin);
        p.lo1 = wave_imin(in ? mine.lo1 : kIntMax); p.hi1 = wave_imax(in ? mine.hi1 : kIntMin);
    }
    p.m2 = wave_add(in ? mine.m2 : 0);
    p.lo2 = wave_imin(in ? mine.lo2 : kIntMax); p.hi2 = wave_imax(in ? mine.hi2 : kIntMin);
    p.lh = p.ll = 0; p.ex = 0;
    if (FIELD) {
        p.lh = wave_add(in ? mine.lh : 0); p.ll = wave_add(in ? mine.ll : 0);
        p.ex = (unsigned)__popcll(__ballot(in && mine.ex));
    }
    return p;
}

// the offset of index i from the anchor's index ai along an axis of n cells: the minimal image on a periodic axis
__device__ __forceinline__ int frame_offset(int i, int ai, int n, int periodic)
{
    int d = i - ai;
    if (periodic) {
        const int h = n / 2;
        int t = d + h;                    // ((d + h) mod n) - h with -n < d < n
        if (t < 0) t += n;
        else if (t >= n) t -= n;
        d = t - h;
    }
    return d;
}

// ---- (a) ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) props_init_kernel(PropsArgs a)
{
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= a.ndomains) return;
    a.anchor[k] = kIntMax;
    for (int q = 0; q < 3; q++) { a.moment[3 * k + q] = 0; a.box[6 * k + 2 * q] = kIntMax; a.box[6 * k + 2 * q + 1] = kIntMin; }
    if (a.in) { a.limb[2 * k] = 0; a.limb[2 * k + 1] = 0; a.excluded[k] = 0; }
}

// ---- (b) the first cell of every label: cells are taken in ascending order, so the first cell a wave meets of a label is its smallest ----------
__global__ void __launch_bounds__(256) props_anchor_kernel(const int *labels, long cells, long ndomains, int *anchor, unsigned long long *bad)
{
    const long stride = (long)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    int held = 0, held_c = 0;          // (0: nothing held); the same in every lane: the control flow below is uniform
    for (long base = (long)blockIdx.x * 256; base < cells; base += stride) {
        const long c = base + threadIdx.x;
        const int lab = c < cells ? labels[c] : 0;
        const bool wrong = lab < 0 || (long)lab > ndomains;
        const unsigned long long w = __ballot(wrong);
        if (w && lane == 0) atomicAdd(bad, (unsigned long long)__popcll(w));
        bool active = lab != 0 && !wrong;
        unsigned long long act = __ballot(active);
        if (act) {
            const int src = __ffsll((long long)act) - 1;
            const int first = __shfl(lab, src);
            if (first != held) {
                if (held && lane == 0) min32(anchor + held - 1, held_c);
                held = first;
                held_c = __shfl((int)c, src);
            }
            active = active && lab != first;
        }
        act = __ballot(active);
        if (act) {
            const int src = __ffsll((long long)act) - 1;
            const int first = __shfl(lab, src);
            if (lane == src) min32(anchor + first - 1, (int)c);
            active = active && lab != first;
        }
        if (active) min32(anchor + lab - 1, (int)c);
    }
    if (held && lane == 0) min32(anchor + held - 1, held_c);
}

// ---- (c) ---------------------------------------------------------------------------------------------------------------------------------
template <typename T, bool FIELD>
__global__ void __launch_bounds__(256) props_sum_kernel(PropsArgs a)
{
    const long stride = (long)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    const unsigned plane = (unsigned)a.n1 * (unsigned)a.n2;          // (cells < 2^31)
    int held = 0;                       // (0: nothing held); held and H are the same in every lane: the control flow below is uniform
    Part H = {};
    for (long base = (long)blockIdx.x * 256; base < a.cells; base += stride) {
        const long c = base + threadIdx.x;
        const int lab = c < a.cells ? a.labels[c] : 0;
        bool active = lab > 0 && (long)lab <= a.ndomains;
        Part mine = {};
        int row = 0;
        if (active) {
            const unsigned uc = (unsigned)c, ua = (unsigned)a.anchor[lab - 1];          // (written by the launch before: a plain load)
            const int i = (int)(uc / plane), j = (int)((uc % plane) / (unsigned)a.n2), k = (int)(uc % (unsigned)a.n2);
            const int ai = (int)(ua / plane), aj = (int)((ua % plane) / (unsigned)a.n2), ak = (int)(ua % (unsigned)a.n2);
            row = (int)(uc / (unsigned)a.n2);
            const int d0 = frame_offset(i, ai, a.n0, a.per0), d1 = frame_offset(j, aj, a.n1, a.per1), d2 = frame_offset(k, ak, a.n2, a.per2);
            mine.m0 = d0; mine.m1 = d1; mine.m2 = d2;
            mine.lo0 = mine.hi0 = d0; mine.lo1 = mine.hi1 = d1; mine.lo2 = mine.hi2 = d2;
            if (FIELD) {
                const double v = (double)((const T *)a.in)[a.off + (long)i * a.p0 + (long)j * a.p1 + k];
                if (fabs(v) <= a.absmax) {          // (NaN and +-inf: false)
                    const double hi = rint(ldexp(v, -a.eh));
                    const double r = v - ldexp(hi, a.eh);          // exact
                    mine.lh = (long long)hi;
                    mine.ll = (long long)rint(ldexp(r, -a.el));
                } else {
                    mine.ex = 1;
                }
            }
        }
        unsigned long long act = __ballot(active);
        if (act) {          // the lanes that share the label of the first active lane go to the held label
            const int src = __ffsll((long long)act) - 1;
            const int first = __shfl(lab, src);
            const bool in = active && lab == first;
            const Part p = combine<FIELD>(in, src, row, mine);
            if (first != held) {
                if (held && lane == 0) flush<FIELD>(a, held, H);
                held = first;
                H = p;
            } else {
                merge(H, p);
            }
            active = active && !in;
        }
        act = __ballot(active);
        if (act) {          // a second round for the next label: one set of atomics; then one set per lane that is left
            const int src = __ffsll((long long)act) - 1;
            const int first = __shfl(lab, src);
            const bool in = active && lab == first;
            const Part p = combine<FIELD>(in, src, row, mine);
            if (lane == src) flush<FIELD>(a, first, p);
            active = active && !in;
        }
        if (active) flush<FIELD>(a, lab, mine);
    }
    if (held && lane == 0) flush<FIELD>(a, held, H);
}

// ---- per stream: the counter of refused labels, on the device and in pinned host memory --------------------------------------------------------
struct PropsScratch {
    unsigned long long *bad_dev, *bad_host;
};
int release_props();
StreamTable<PropsScratch> g_props(release_props);

int release_props()
{
    return g_props.release([](PropsScratch &s) {
        if (s.bad_dev) (void)hipFree(s.bad_dev);
        if (s.bad_host) (void)hipHostFree(s.bad_host);
    });
}

int props_scratch(hipStream_t st, PropsScratch *out)
{
    return g_props.with(st, [&](PropsScratch &s) -> int {      // (a new entry is all zeros)
        if (!s.bad_dev) PDEHIP_HIP(hipMalloc((void **)&s.bad_dev, 16));
        if (!s.bad_host) PDEHIP_HIP(hipHostMalloc((void **)&s.bad_host, 16, hipHostMallocDefault));
        *out = s;
        return 0;
    });
}

}  // namespace
}  // namespace pdehip

using namespace pdehip;

extern "C" int pdehip_domain_properties(const pdehip_grid_t *g, const void *arr_full, const int32_t *labels_dev, int64_t ndomains,
                                        const int *periodic_host, double absmax, int32_t *anchor_dev, int64_t *moment_dev, int32_t *box_dev,
                                        int64_t *limb_dev, uint32_t *excluded_dev, void *stream)
{
    NGrid n;
    PDEHIP_TRY(norm_grid(g, &n));
    if (ndomains < 0 || ndomains > 2147483647LL) PDEHIP_FAIL(E_VALUE, "domain_properties: 0 ... 2^31 - 1 domains (got %lld)", (long long)ndomains);
    if (!labels_dev || !periodic_host) PDEHIP_FAIL(E_VALUE, "domain_properties: NULL pointer");
    if (ndomains > 0 && (!anchor_dev || !moment_dev || !box_dev || (arr_full && (!limb_dev || !excluded_dev))))
        PDEHIP_FAIL(E_VALUE, "domain_properties: NULL pointer");
    if (!(absmax >= 0.0) || !(absmax < 0x1p1023)) PDEHIP_FAIL(E_VALUE, "domain_properties: absmax must be a number in [0, 2^1023) (got %g)", absmax);
    const double cells_f = (double)n.n[0] * (double)n.n[1] * (double)n.n[2];
    if (cells_f > 2147483647.0) PDEHIP_FAIL(E_VALUE, "domain_properties: %.0f interior cells, at most 2^31 - 1", cells_f);
    if (((uintptr_t)arr_full & 15) != 0 || ((uintptr_t)labels_dev & 3) != 0 || ((uintptr_t)anchor_dev & 3) != 0 || ((uintptr_t)moment_dev & 7) != 0 ||
        ((uintptr_t)box_dev & 3) != 0 || (arr_full && (((uintptr_t)limb_dev & 7) != 0 || ((uintptr_t)excluded_dev & 3) != 0)))
        PDEHIP_FAIL(E_VALUE, "domain_properties: misaligned array (16 bytes for the field, 8 for moments and limbs, 4 for labels, anchors, boxes and counts)");
    hipStream_t st = as_stream(stream);
    PropsScratch s;
    PDEHIP_TRY(props_scratch(st, &s));

    PropsArgs a;
    a.n0 = (int)n.n[0]; a.n1 = (int)n.n[1]; a.n2 = (int)n.n[2];
    int per[3] = {0, 0, 0};
    for (int d = 0; d < n.ndim; d++) per[3 - n.ndim + d] = periodic_host[d] != 0;
    a.per0 = per[0]; a.per1 = per[1]; a.per2 = per[2];
    a.p0 = n.p[0]; a.p1 = n.p[1]; a.off = n.off;
    a.cells = n.n[0] * n.n[1] * n.n[2];
    a.ndomains = (long)ndomains;
    // the limbs: hi counts units of 2^eh, lo units of 2^el; |hi| <= 2^(62 - L) and |lo| <= 2^30 per cell, so neither sum of up to 2^L cells overflows
    int L = 0, E = 0;
    while ((1LL << L) < (long long)a.cells) L++;
    (void)frexp(absmax, &E);
    a.eh = E - (62 - L);
    a.el = a.eh - 31;
    a.absmax = absmax;
    a.in = arr_full; a.labels = (const int *)labels_dev; a.anchor = (int *)anchor_dev; a.moment = (long long *)moment_dev; a.box = (int *)box_dev;
    a.limb = (long long *)limb_dev; a.excluded = (unsigned *)excluded_dev;

    PDEHIP_HIP(hipMemsetAsync(s.bad_dev, 0, 16, st));
    const unsigned blocks = blocks_for(a.cells, kPropsBlocksMax);
    if (ndomains > 0) hipLaunchKernelGGL(props_init_kernel, dim3((unsigned)((ndomains + 255) / 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(props_anchor_kernel, dim3(blocks), dim3(256), 0, st, a.labels, a.cells, a.ndomains, a.anchor, s.bad_dev);
    if (ndomains > 0) {
        const bool f64 = n.dtype == PDEHIP_F64;
        if (!arr_full) hipLaunchKernelGGL((props_sum_kernel<double, false>), dim3(blocks), dim3(256), 0, st, a);
        else if (f64) hipLaunchKernelGGL((props_sum_kernel<double, true>), dim3(blocks), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((props_sum_kernel<float, true>), dim3(blocks), dim3(256), 0, st, a);
        note_kernel("props_sum_kernel<%s,%d>", f64 || !arr_full ? "double" : "float", arr_full ? 1 : 0);
    }
    PDEHIP_HIP(hipGetLastError());
    // labels outside 0 ... ndomains were counted, not used: the call is refused with their number (the caller reads the results next)
    PDEHIP_HIP(hipMemcpyAsync(s.bad_host, s.bad_dev, 8, hipMemcpyDeviceToHost, st));
    PDEHIP_HIP(hipStreamSynchronize(st));
    if (s.bad_host[0] != 0)
        PDEHIP_FAIL(E_VALUE, "domain_properties: %llu cells have a label outside 0 ... %lld", (unsigned long long)s.bad_host[0], (long long)ndomains);
    return 0;
}
