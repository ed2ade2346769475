// pdehip_label.hip — the domains of a field where it lives: connected-component labels of the cells with lo <= x <= hi, numbered like
// scipy.ndimage.label, and the number of cells of every label.
//
// Semantics: include/pdehip.h.  The algorithm and why every loop ends: DESIGN.md §4.15.  In short: union-find in which the root of a
// domain is its smallest linear (C order) cell index, so parent[i] <= i ALWAYS and every `find` walks a strictly decreasing chain.
//   (a) label_tile_kernel   one workgroup labels one tile of kT0 x kT1 x kT2 cells entirely in LDS and writes parent[] (-1: background)
//   (b) label_seam_kernel   unites the pairs of neighbours that lie in different tiles or are neighbours through a periodic wrap;
//                           EVERY access to parent[] in it is a relaxed agent-scope atomic (workgroups on different XCDs have private
//                           L2s: a plain load of a word another workgroup has written in the same launch can be stale)
//   (c) label_flatten_kernel  labels[i] = root of i, into the SECOND array (plain loads: parent[] was written by earlier launches),
//                           and the number of roots and of foreground cells per chunk of kChunk cells
//   (d) label_scan_kernel   ONE workgroup: exclusive sums of the chunks' root counts, {K, foreground} to info
//       label_number_kernel parent[root] = 1 + the C-order count of the roots before it (chunk offset + ballots inside the chunk)
//       label_write_kernel  labels[i] = parent[labels[i]], 0 for background
//   (e) domain_sizes_kernel integer adds; the lanes of a wave that hit the same label are combined, and a wave keeps the label it met
//                           last in a register (one percolating domain costs one add per wave, not one per cell)
// Everything is integer work: the result does not depend on the order in which workgroups run.  No kernel waits for another workgroup.
#include "pdehip_common.h"
#include "pdehip_scratch.h"

namespace pdehip {
namespace {

constexpr int kT0 = 4, kT1 = 8, kT2 = 32;           // the tile of (a): 1024 cells, 4 per thread, 4 KB of LDS
constexpr int kTile = kT0 * kT1 * kT2;
constexpr int kChunk = 4096;                        // cells of one chunk of (c) / (d): 16 per thread
constexpr int kChunkIts = kChunk / 256;

// the half of the neighbourhood with a smaller C-order offset: the 3 faces first, then the 10 edges and corners of full connectivity
__constant__ signed char kBack[13][3] = {{0, 0, -1},  {0, -1, 0},  {-1, 0, 0},  {0, -1, -1}, {0, -1, 1}, {-1, 0, -1}, {-1, 0, 1},
                                         {-1, -1, 0}, {-1, 1, 0},  {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};

struct LabelArgs {
    int n0, n1, n2;                // interior cells of the normalised axes
    int nt0, nt1, nt2;             // tiles per axis
    int per0, per1, per2;          // periodic axes (never a padded axis)
    long p0, p1, off;              // pitches and the first interior cell of the field's device layout
    double lo, hi;
    const void *in;
    int *parent;
};

// ---- union-find on an int array with parent[i] <= i; A = 0: LDS of this workgroup, A = 1: global memory shared with other workgroups ----
template <int A>
__device__ __forceinline__ int uf_load(int *p, int i)
{
    if (A) return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <int A>
__device__ __forceinline__ int uf_min(int *p, int i, int v)
{
    if (A) return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// the root of foreground cell x: every step goes to a smaller index (parent[i] <= i), so it ends after at most x steps
template <int A>
__device__ __forceinline__ int uf_find(int *p, int x)
{
    for (int q = uf_load<A>(p, x); q != x; q = uf_load<A>(p, x)) x = q;
    return x;
}
// Unite the sets of foreground cells a and b.  Each turn either returns or continues with a strictly smaller `a` while `b` never grows
// (a + b decreases and is >= 0): the loop ends whatever other threads do.  The only write is atomicMin(parent[a], b) with b < a.
template <int A>
__device__ __forceinline__ void uf_union(int *p, int a, int b)
{
    for (;;) {
        a = uf_find<A>(p, a);
        b = uf_find<A>(p, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = uf_min<A>(p, a, b);
        if (old == a) return;          // a was still a root and now hangs under b
        a = old;                       // another thread hung a under `old` first (old < a): the set of `old` is to be united with b
    }
}

// ---- (a) one tile in LDS ---------------------------------------------------------------------------------------------------------------
template <typename T, bool FULL>
__global__ void __launch_bounds__(256) label_tile_kernel(LabelArgs a)
{
    __shared__ int lab[kTile];
    long t = blockIdx.x;
    const int tz = (int)(t % a.nt2); t /= a.nt2;
    const int ty = (int)(t % a.nt1);
    const int tx = (int)(t / a.nt1);
    const int b0 = tx * kT0, b1 = ty * kT1, b2 = tz * kT2;
    const T *in = (const T *)a.in;
#pragma unroll
    for (int m = 0; m < kTile / 256; m++) {
        const int l = (int)threadIdx.x + 256 * m;
        const int i = b0 + l / (kT1 * kT2), j = b1 + (l / kT2) % kT1, k = b2 + l % kT2;
        bool fg = false;
        if (i < a.n0 && j < a.n1 && k < a.n2) {
            const double x = (double)in[a.off + (long)i * a.p0 + (long)j * a.p1 + k];
            fg = a.lo <= x && x <= a.hi;          // (NaN: false)
        }
        lab[l] = fg ? l : -1;
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < kTile / 256; m++) {
        const int l = (int)threadIdx.x + 256 * m;
        if (uf_load<0>(lab, l) < 0) continue;
        const int l0 = l / (kT1 * kT2), l1 = (l / kT2) % kT1, l2 = l % kT2;
        for (int d = 0; d < (FULL ? 13 : 3); d++) {
            const int q0 = l0 + kBack[d][0], q1 = l1 + kBack[d][1], q2 = l2 + kBack[d][2];
            if (q0 < 0 || q1 < 0 || q1 >= kT1 || q2 < 0 || q2 >= kT2) continue;          // (q0 <= l0: never above the tile)
            const int nb = (q0 * kT1 + q1) * kT2 + q2;
            if (uf_load<0>(lab, nb) >= 0) uf_union<0>(lab, l, nb);          // (a cell beyond the grid's end is background)
        }
    }
    __syncthreads();
    // the local C order of a tile's cells is their global C order: the smallest local index is the smallest global one
#pragma unroll
    for (int m = 0; m < kTile / 256; m++) {
        const int l = (int)threadIdx.x + 256 * m;
        const int i = b0 + l / (kT1 * kT2), j = b1 + (l / kT2) % kT1, k = b2 + l % kT2;
        if (i >= a.n0 || j >= a.n1 || k >= a.n2) continue;
        int out = -1;
        if (lab[l] >= 0) {
            const int r = uf_find<0>(lab, l);          // (nothing writes lab[] any more)
            out = ((b0 + r / (kT1 * kT2)) * a.n1 + b1 + (r / kT2) % kT1) * a.n2 + b2 + r % kT2;
        }
        a.parent[((long)i * a.n1 + j) * a.n2 + k] = out;
    }
}

// ---- (b) the pairs the tiles have not seen: one thread per cell, only cells with such a pair touch memory ------------------------------------
template <bool FULL>
__global__ void __launch_bounds__(256) label_seam_kernel(LabelArgs a)
{
    const long cells = (long)a.n0 * a.n1 * a.n2;
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= cells) return;
    const int k = (int)(c % a.n2), j = (int)((c / a.n2) % a.n1), i = (int)(c / ((long)a.n1 * a.n2));
    // backward offsets are -1 or 0 on axis 0 and -1, 0 or +1 on the others: away from these faces every backward neighbour is in the same tile
    // (an axis of one layer has no backward neighbour of its own: through a wrap it reaches cells of the same layer, which are neighbours anyway)
    const bool edge0 = a.n0 > 1 && i % kT0 == 0, edge1 = a.n1 > 1 && (j % kT1 == 0 || j % kT1 == kT1 - 1 || j == a.n1 - 1),
               edge2 = k % kT2 == 0 || k % kT2 == kT2 - 1 || k == a.n2 - 1;
    if (!(edge0 || edge1 || edge2)) return;
    if (uf_load<1>(a.parent, (int)c) < 0) return;
    for (int d = 0; d < (FULL ? 13 : 3); d++) {
        int q0 = i + kBack[d][0], q1 = j + kBack[d][1], q2 = k + kBack[d][2];
        bool wrapped = false;
        if (q0 < 0 || q0 >= a.n0) { if (!a.per0) continue; q0 = q0 < 0 ? a.n0 - 1 : 0; wrapped = true; }
        if (q1 < 0 || q1 >= a.n1) { if (!a.per1) continue; q1 = q1 < 0 ? a.n1 - 1 : 0; wrapped = true; }
        if (q2 < 0 || q2 >= a.n2) { if (!a.per2) continue; q2 = q2 < 0 ? a.n2 - 1 : 0; wrapped = true; }
        if (!wrapped && q0 / kT0 == i / kT0 && q1 / kT1 == j / kT1 && q2 / kT2 == k / kT2) continue;          // united in LDS
        const int nb = (q0 * a.n1 + q1) * a.n2 + q2;
        if (nb != (int)c && uf_load<1>(a.parent, nb) >= 0) uf_union<1>(a.parent, (int)c, nb);
    }
}

// ---- (c) roots into the second array, roots and foreground cells per chunk -------------------------------------------------------------
__global__ void __launch_bounds__(256) label_flatten_kernel(const int *parent, int *labels, long cells, unsigned *chunk_roots, unsigned *chunk_fg)
{
    __shared__ unsigned s_roots, s_fg;
    if (threadIdx.x == 0) { s_roots = 0; s_fg = 0; }
    __syncthreads();
    unsigned roots = 0, fg = 0;
#pragma unroll 4
    for (int it = 0; it < kChunkIts; it++) {
        const long c = (long)blockIdx.x * kChunk + it * 256 + threadIdx.x;
        if (c >= cells) break;
        int x = parent[c];
        if (x >= 0) {
            int at = (int)c;
            while (x != at) { at = x; x = parent[at]; }          // (strictly decreasing: parent[i] <= i)
            fg++;
            roots += x == (int)c;
        }
        labels[c] = x;
    }
    // (integer adds: the sums do not depend on their order)
    for (int s = 32; s > 0; s >>= 1) { roots += __shfl_down(roots, s); fg += __shfl_down(fg, s); }
    if ((threadIdx.x & 63) == 0) { atomicAdd(&s_roots, roots); atomicAdd(&s_fg, fg); }
    __syncthreads();
    if (threadIdx.x == 0) { chunk_roots[blockIdx.x] = s_roots; chunk_fg[blockIdx.x] = s_fg; }
}

// ---- (d) a deterministic scan: ONE workgroup turns the chunks' root counts into the number of roots before each chunk ---------------------
__global__ void __launch_bounds__(256) label_scan_kernel(unsigned *chunk_roots, const unsigned *chunk_fg, long nchunks, unsigned long long *info)
{
    __shared__ unsigned long long buf[256], fbuf[256];
    const long per = (nchunks + 255) / 256;
    const long lo = threadIdx.x * per, hi = lo + per < nchunks ? lo + per : nchunks;
    unsigned long long mine = 0, fg = 0;
    for (long q = lo; q < hi; q++) { mine += chunk_roots[q]; fg += chunk_fg[q]; }
    buf[threadIdx.x] = mine;
    fbuf[threadIdx.x] = fg;
    __syncthreads();
    for (int ofs = 1; ofs < 256; ofs <<= 1) {
        const unsigned long long below = (int)threadIdx.x >= ofs ? buf[threadIdx.x - ofs] : 0, fbelow = (int)threadIdx.x >= ofs ? fbuf[threadIdx.x - ofs] : 0;
        __syncthreads();
        buf[threadIdx.x] += below;
        fbuf[threadIdx.x] += fbelow;
        __syncthreads();
    }
    unsigned run = (unsigned)(buf[threadIdx.x] - mine);          // (K < 2^31)
    for (long q = lo; q < hi; q++) { const unsigned c = chunk_roots[q]; chunk_roots[q] = run; run += c; }
    if (threadIdx.x == 255) { info[0] = buf[255]; info[1] = fbuf[255]; }
}

// parent[root] = its label: 1 + the roots before its chunk + the roots before it inside the chunk (C order: turn, wave, lane)
__global__ void __launch_bounds__(256) label_number_kernel(const int *labels, int *parent, long cells, const unsigned *chunk_before)
{
    __shared__ unsigned cnt[kChunkIts * 4];
    const int wave = threadIdx.x >> 6;
    unsigned long long mask[kChunkIts];
#pragma unroll
    for (int it = 0; it < kChunkIts; it++) {
        const long c = (long)blockIdx.x * kChunk + it * 256 + threadIdx.x;
        const bool root = c < cells && labels[c] == (int)c;
        mask[it] = __ballot(root);
        if ((threadIdx.x & 63) == 0) cnt[it * 4 + wave] = (unsigned)__popcll(mask[it]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned run = chunk_before[blockIdx.x] + 1;
        for (int q = 0; q < kChunkIts * 4; q++) { const unsigned c = cnt[q]; cnt[q] = run; run += c; }
    }
    __syncthreads();
    const unsigned lane = threadIdx.x & 63;
#pragma unroll
    for (int it = 0; it < kChunkIts; it++) {
        const unsigned long long m = mask[it];
        if ((m >> lane) & 1ULL) {
            const long c = (long)blockIdx.x * kChunk + it * 256 + threadIdx.x;
            parent[c] = (int)(cnt[it * 4 + wave] + (unsigned)__popcll(m & ((1ULL << lane) - 1ULL)));
        }
    }
}

__global__ void __launch_bounds__(256) label_write_kernel(int *labels, const int *parent, long cells)
{
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= cells) return;
    const int r = labels[c];
    labels[c] = r < 0 ? 0 : parent[r];
}

// ---- (e) the cells of every label ------------------------------------------------------------------------------------------------------
// A wave keeps the label it counted last and its count in (uniform) registers and adds them when another label comes first: cells are
// taken in C order, so the lanes of a wave mostly sit in one or two domains.  Labels outside 0 ... ndomains are counted in *bad.
__global__ void __launch_bounds__(256) domain_sizes_kernel(const int *labels, long cells, long ndomains, unsigned long long *sizes, unsigned long long *bad)
{
    const long stride = (long)gridDim.x * 256;
    const int lane = threadIdx.x & 63;
    int held = 0;                       // (0: nothing held); held and held_n are the same in every lane: the control flow below is uniform
    unsigned long long held_n = 0;
    for (long base = (long)blockIdx.x * 256; base < cells; base += stride) {
        const long c = base + threadIdx.x;
        const int lab = c < cells ? labels[c] : 0;
        const bool wrong = lab < 0 || (long)lab > ndomains;
        const unsigned long long w = __ballot(wrong);
        if (w && lane == 0) atomicAdd(bad, (unsigned long long)__popcll(w));
        bool active = lab != 0 && !wrong;
        unsigned long long act = __ballot(active);
        if (act) {          // the lanes that share the label of the first active lane go to the held count
            const int first = __shfl(lab, __ffsll((long long)act) - 1);
            const unsigned long long m = __ballot(active && lab == first);
            if (first != held) {
                if (held && lane == 0) atomicAdd(&sizes[held - 1], held_n);
                held = first;
                held_n = 0;
            }
            held_n += (unsigned long long)__popcll(m);
            active = active && lab != first;
        }
        act = __ballot(active);
        if (act) {          // a second round for the next label: one add; then one add per lane that is left
            const int src = __ffsll((long long)act) - 1;
            const int first = __shfl(lab, src);
            const unsigned long long m = __ballot(active && lab == first);
            if (lane == src) atomicAdd(&sizes[first - 1], (unsigned long long)__popcll(m));
            active = active && lab != first;
        }
        if (active) atomicAdd(&sizes[lab - 1], 1ULL);
    }
    if (held && lane == 0) atomicAdd(&sizes[held - 1], held_n);
}

// ---- per stream: the parent array (4 bytes per cell, grown on demand), the chunk counts of the scan, the counter of refused labels ---------
struct LabelScratch {
    int *parent;
    long parent_cells;
    unsigned *chunks;                // roots, then foreground cells, per chunk
    long chunk_slots;
    unsigned long long *bad_dev, *bad_host;
};
int release_arrays();
StreamTable<LabelScratch> g_table(release_arrays);

int release_arrays()
{
    return g_table.release([](LabelScratch &s) {
        if (s.parent) (void)hipFree(s.parent);
        if (s.chunks) (void)hipFree(s.chunks);
        if (s.bad_dev) (void)hipFree(s.bad_dev);
        if (s.bad_host) (void)hipHostFree(s.bad_host);
    });
}

int label_scratch(hipStream_t st, long cells, LabelScratch *out)
{
    return g_table.with(st, [&](LabelScratch &s) -> int {      // (a new entry is all zeros)
        if (!s.bad_dev) {
            PDEHIP_HIP(hipMalloc((void **)&s.bad_dev, 16));
            PDEHIP_HIP(hipHostMalloc((void **)&s.bad_host, 16, hipHostMallocDefault));
        }
        if (cells > s.parent_cells) {
            // (hipFree waits for the device: no launch still uses the smaller arrays)
            if (s.parent) (void)hipFree(s.parent);
            if (s.chunks) (void)hipFree(s.chunks);
            s.parent = nullptr; s.chunks = nullptr; s.parent_cells = 0; s.chunk_slots = 0;
            const long slots = (cells + kChunk - 1) / kChunk;
            PDEHIP_HIP(hipMalloc((void **)&s.parent, sizeof(int) * (size_t)cells));
            const hipError_t e = hipMalloc((void **)&s.chunks, sizeof(unsigned) * 2 * (size_t)slots);
            if (e != hipSuccess) {
                (void)hipFree(s.parent);
                s.parent = nullptr;
                PDEHIP_FAIL(100 + (int)e, "hipMalloc of the labelling's chunk counts failed: %s", hipGetErrorString(e));
            }
            s.parent_cells = cells;
            s.chunk_slots = slots;
        }
        *out = s;
        return 0;
    });
}

}  // namespace
}  // namespace pdehip

using namespace pdehip;

extern "C" int pdehip_label_domains(const pdehip_grid_t *g, const void *arr_full, double lo, double hi, int connectivity,
                                    const int *periodic_host, int32_t *labels_dev, uint64_t *info_dev, void *stream)
{
    NGrid n;
    PDEHIP_TRY(norm_grid(g, &n));
    if (!arr_full || !periodic_host || !labels_dev || !info_dev) PDEHIP_FAIL(E_VALUE, "label_domains: NULL pointer");
    if (lo != lo || hi != hi || lo > hi) PDEHIP_FAIL(E_VALUE, "label_domains: the bounds must be numbers with lo <= hi (got %g, %g)", lo, hi);
    if (connectivity != 1 && connectivity != n.ndim)
        PDEHIP_FAIL(E_VALUE, "label_domains: connectivity 1 (faces) or %d (all neighbours) on a %d-D grid (got %d)", n.ndim, n.ndim, connectivity);
    const double cells_f = (double)n.n[0] * (double)n.n[1] * (double)n.n[2];
    if (cells_f > 2147483647.0) PDEHIP_FAIL(E_VALUE, "label_domains: %.0f interior cells, at most 2^31 - 1", cells_f);
    if (((uintptr_t)arr_full & 15) != 0 || ((uintptr_t)labels_dev & 3) != 0 || ((uintptr_t)info_dev & 7) != 0)
        PDEHIP_FAIL(E_VALUE, "label_domains: misaligned array (16 bytes for the field, 4 for the labels, 8 for info)");
    const long cells = n.n[0] * n.n[1] * n.n[2];
    hipStream_t st = as_stream(stream);
    LabelScratch s;
    PDEHIP_TRY(label_scratch(st, cells, &s));

    LabelArgs a;
    a.n0 = (int)n.n[0]; a.n1 = (int)n.n[1]; a.n2 = (int)n.n[2];
    a.nt0 = (a.n0 + kT0 - 1) / kT0; a.nt1 = (a.n1 + kT1 - 1) / kT1; a.nt2 = (a.n2 + kT2 - 1) / kT2;
    int per[3] = {0, 0, 0};
    for (int d = 0; d < n.ndim; d++) per[3 - n.ndim + d] = periodic_host[d] != 0;
    a.per0 = per[0]; a.per1 = per[1]; a.per2 = per[2];
    a.p0 = n.p[0]; a.p1 = n.p[1]; a.off = n.off;
    a.lo = lo; a.hi = hi; a.in = arr_full; a.parent = s.parent;
    const bool full = connectivity != 1;          // (1-D: connectivity 1 IS all neighbours)
    const bool f64 = n.dtype == PDEHIP_F64;
    const long tiles = (long)a.nt0 * a.nt1 * a.nt2;          // (at most 2^31 / 32 workgroups)
    const unsigned per_cell = (unsigned)((cells + 255) / 256);
    const long nchunks = (cells + kChunk - 1) / kChunk;
    unsigned *chunk_roots = s.chunks, *chunk_fg = s.chunks + s.chunk_slots;
    if (f64) {
        if (full) hipLaunchKernelGGL((label_tile_kernel<double, true>), dim3((unsigned)tiles), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((label_tile_kernel<double, false>), dim3((unsigned)tiles), dim3(256), 0, st, a);
    } else {
        if (full) hipLaunchKernelGGL((label_tile_kernel<float, true>), dim3((unsigned)tiles), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((label_tile_kernel<float, false>), dim3((unsigned)tiles), dim3(256), 0, st, a);
    }
    if (full) hipLaunchKernelGGL((label_seam_kernel<true>), dim3(per_cell), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((label_seam_kernel<false>), dim3(per_cell), dim3(256), 0, st, a);
    hipLaunchKernelGGL(label_flatten_kernel, dim3((unsigned)nchunks), dim3(256), 0, st, (const int *)s.parent, (int *)labels_dev, cells, chunk_roots, chunk_fg);
    hipLaunchKernelGGL(label_scan_kernel, dim3(1), dim3(256), 0, st, chunk_roots, (const unsigned *)chunk_fg, nchunks, (unsigned long long *)info_dev);
    hipLaunchKernelGGL(label_number_kernel, dim3((unsigned)nchunks), dim3(256), 0, st, (const int *)labels_dev, s.parent, cells, (const unsigned *)chunk_roots);
    hipLaunchKernelGGL(label_write_kernel, dim3(per_cell), dim3(256), 0, st, (int *)labels_dev, (const int *)s.parent, cells);
    note_kernel("label_tile_kernel<%s,%d>", f64 ? "double" : "float", full ? 1 : 0);
    PDEHIP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pdehip_domain_sizes(const int32_t *labels_dev, int64_t ncells, int64_t ndomains, uint64_t *sizes_dev, void *stream)
{
    if (!labels_dev || (!sizes_dev && ndomains > 0)) PDEHIP_FAIL(E_VALUE, "domain_sizes: NULL pointer");
    if (ncells < 1 || ndomains < 0 || ndomains > 2147483647LL)
        PDEHIP_FAIL(E_VALUE, "domain_sizes: at least one cell and 0 ... 2^31 - 1 domains (got %lld, %lld)", (long long)ncells, (long long)ndomains);
    if (((uintptr_t)labels_dev & 3) != 0 || ((uintptr_t)sizes_dev & 7) != 0)
        PDEHIP_FAIL(E_VALUE, "domain_sizes: misaligned array (4 bytes for the labels, 8 for the sizes)");
    hipStream_t st = as_stream(stream);
    LabelScratch s;
    PDEHIP_TRY(label_scratch(st, 0, &s));
    PDEHIP_HIP(hipMemsetAsync(s.bad_dev, 0, 16, st));
    if (ndomains > 0) PDEHIP_HIP(hipMemsetAsync(sizes_dev, 0, sizeof(uint64_t) * (size_t)ndomains, st));
    const long want = (long)((ncells + 255) / 256);
    const unsigned blocks = (unsigned)(want > 4096 ? 4096 : want);
    hipLaunchKernelGGL(domain_sizes_kernel, dim3(blocks), dim3(256), 0, st, (const int *)labels_dev, (long)ncells, (long)ndomains,
                       (unsigned long long *)sizes_dev, s.bad_dev);
    PDEHIP_HIP(hipGetLastError());
    // labels outside 0 ... ndomains were counted, not written: the call is refused with their number (the caller waits for the sizes anyway)
    PDEHIP_HIP(hipMemcpyAsync(s.bad_host, s.bad_dev, 8, hipMemcpyDeviceToHost, st));
    PDEHIP_HIP(hipStreamSynchronize(st));
    if (s.bad_host[0] != 0)
        PDEHIP_FAIL(E_VALUE, "domain_sizes: %llu cells have a label outside 0 ... %lld", (unsigned long long)s.bad_host[0], (long long)ndomains);
    return 0;
}
