// pdehip_fft.hip — the forward transform of a field where it lives, and the sums of its power over shells of |k|: what
// `np.fft.fftn(state.data)` and a radial average in a tracker callback answer, without moving the state to the host.
//
// Semantics: include/pdehip.h.  Dataflow, limbs and LDS budget: DESIGN.md §4.17.  In short:
//   fft_rows_kernel<T>     the interior rows of the fastest axis, converted exactly to fp64, as complex lines with a zero imaginary part;
//                          the first n2 / 2 + 1 outputs of every line go to the dense half spectrum
//   fft_lines_kernel       one slower axis of the half spectrum, in place: tiles of at least 8 neighbouring columns (128 bytes) per line
//                          index, ragged at the end of the columns, because n2 / 2 + 1 is never a multiple of the tile
//   inverse_lines_kernel   the same tiles with the twiddles conjugated at the copy into LDS (a sign flip is exact): a slower axis of the
//                          inverse transform, in place
//   inverse_rows_kernel<T> the fastest axis of the inverse: every stored row of n2 / 2 + 1 elements becomes a full complex line (element
//                          N - k is the conjugate of element k), the real part of the result times 1 / size goes to the interior cells
//   shell_max_kernel       per shell the mode count (weight 2 inside the Hermitian half, 1 on its two faces) and the largest weighted
//                          power as an integer maximum of the bit image
//   shell_params_kernel    per shell the exponents of three fixed-point limbs from that maximum and the count
//   shell_limb_kernel      per shell the three 64-bit integer sums of the limbs of every weighted power
// Every line is transformed in LDS by the SAME schedule whatever the extent, the tile or the launch: bit reversal at the load, then
// log2(N) in-place radix-2 stages (decimation in time), butterfly (u, v) -> (u + w v, u - w v) with w from a table made on the host and
// w v = (ac - bd) + i (ad + bc), one rounding per operation (no FMA contraction in any build).  An output element is a fixed expression
// of the inputs: which lane, wave or workgroup evaluates a butterfly does not enter.  Everything that is combined across waves is an
// integer (counts, maxima of bit images, limbs): no floating-point atomic, two calls give equal bits, a serial host version too.
#include "pdehip_fft.h"
#include "pdehip_sweep.h"

namespace pdehip {
namespace {

constexpr int kShellBinsMax = 4096;
constexpr long kFftBlocksMax = 1024;            // workgroups of a transform pass (each holds 8 KiB or more of LDS)
constexpr long kShellBlocksMax = 2048;          // workgroups of a shell sweep (each ends with one atomic per shell it met)
constexpr int kTileMin = 8;                     // columns of a strided tile: 8 complex128 are 128 contiguous bytes per line index
constexpr long kTileElems = 2048;               // ... and more columns for short lines, up to this many elements (32 KiB) per tile

// ---- the twiddle table: exp(-2 pi i m / N), 0 <= m < N / 2, from angles in the first octant (the same lines: tests/shim) -----------------
void twiddle(long m, long n, double *re, double *im)
{
    long q = m;
    bool negate = false, swap = false;
    if (4 * q > n) { q = n / 2 - q; negate = true; }          // pi - a: the cosine changes sign
    if (8 * q > n) { q = n / 4 - q; swap = true; }            // pi / 2 - a: cosine and sine change places
    const double a = 6.283185307179586476925 * (double)q / (double)n;
    double c = cos(a), s = sin(a);
    if (swap) { const double t = c; c = s; s = t; }
    if (negate) c = -c;
    *re = c;
    *im = -s;
}

__device__ __forceinline__ unsigned bit_reverse(unsigned i, int log2n) { return log2n ? __brev(i) >> (32 - log2n) : 0u; }

// The stages of `lines` lines of N = 1 << log2n elements in LDS; element idx of line b is x[idx * s_idx + b * s_line], already in
// bit-reversed order.  tw: the N / 2 twiddles, in LDS too.  All threads of the workgroup call it; it ends behind a barrier.
__device__ __forceinline__ void fft_stages(cplx *x, const cplx *tw, int log2n, int lines, int log2lines_or_neg, int s_idx, int s_line)
{
    const int half_n = (1 << log2n) >> 1;
    const int work = half_n * lines;
    for (int s = 1; s <= log2n; s++) {
        __syncthreads();
        const int half = 1 << (s - 1);
        for (int e = threadIdx.x; e < work; e += 256) {
            int t, b;
            if (log2lines_or_neg >= 0) { t = e >> log2lines_or_neg; b = e & (lines - 1); }     // columns of a tile: the line varies fastest
            else { b = e / half_n; t = e - b * half_n; }                                      // rows: the butterfly varies fastest
            const int kk = t & (half - 1);
            const int i = ((t >> (s - 1)) << s) + kk;
            cplx *pu = x + (long)i * s_idx + (long)b * s_line;
            cplx *pv = pu + (long)half * s_idx;
            const cplx w = tw[kk << (log2n - s)];
            const cplx u = *pu, v = *pv;
            cplx p;
            p.x = w.x * v.x - w.y * v.y;
            p.y = w.x * v.y + w.y * v.x;
            cplx lo, hi;
            lo.x = u.x + p.x; lo.y = u.y + p.y;
            hi.x = u.x - p.x; hi.y = u.y - p.y;
            *pu = lo;
            *pv = hi;
        }
    }
    __syncthreads();
}

// ---- the fastest axis: real rows to half-spectrum rows ------------------------------------------------------------------------------------
struct RowsArgs {
    RowGrid g;
    long pc;                       // elements of one component of the field
    long rows;                     // n0 * n1
    int log2n, batch, nh;          // N = n2 = 1 << log2n; rows of one batch; n2 / 2 + 1
    const void *in;                // component 0; workgroup row blockIdx.y takes component blockIdx.y
    cplx *out;                     // (components, rows, nh)
    const cplx *tw;                // n2 / 2 twiddles
};

// LDS: batch * N elements, then N / 2 twiddles
template <typename T>
__global__ void __launch_bounds__(256) fft_rows_kernel(RowsArgs a)
{
    extern __shared__ cplx fft_lds[];
    const int n = 1 << a.log2n;
    cplx *x = fft_lds, *tw = fft_lds + (long)a.batch * n;
    for (int i = threadIdx.x; i < n / 2; i += 256) tw[i] = a.tw[i];
    const T *in = (const T *)a.in + (long)blockIdx.y * a.pc;
    cplx *out = a.out + (long)blockIdx.y * a.rows * a.nh;
    const long batches = (a.rows + a.batch - 1) / a.batch;
    for (long bt = blockIdx.x; bt < batches; bt += gridDim.x) {
        __syncthreads();                                       // (the stores of the batch before have read the lines)
        for (int e = threadIdx.x; e < a.batch * n; e += 256) {
            const int b = e >> a.log2n, idx = e & (n - 1);
            const long row = bt * a.batch + b;
            cplx v;
            v.x = 0.0; v.y = 0.0;
            if (row < a.rows) {
                const long i = row / a.g.n1, j = row - i * a.g.n1;
                v.x = (double)in[a.g.off + i * a.g.p0 + j * a.g.p1 + idx];
            }
            x[(long)b * n + bit_reverse((unsigned)idx, a.log2n)] = v;
        }
        fft_stages(x, tw, a.log2n, a.batch, -1, 1, n);
        for (int e = threadIdx.x; e < a.batch * a.nh; e += 256) {
            const int b = e / a.nh, k = e - b * a.nh;
            const long row = bt * a.batch + b;
            if (row < a.rows) out[row * a.nh + k] = x[(long)b * n + k];
        }
    }
}

// ---- a slower axis of the half spectrum, in place: element (o, idx, w) is spec[(o * N + idx) * width + w] -----------------------------------
struct LinesArgs {
    cplx *spec;
    long outer, width;             // slabs; columns of a slab (nh for axis 1, n1 * nh for axis 0)
    int log2n, log2t;              // N = 1 << log2n; columns of a tile
    const cplx *tw;
};

// LDS: N * tile elements (the column varies fastest), then N / 2 twiddles
__global__ void __launch_bounds__(256) fft_lines_kernel(LinesArgs a)
{
    extern __shared__ cplx fft_lds[];
    const int n = 1 << a.log2n, tile = 1 << a.log2t;
    cplx *x = fft_lds, *tw = fft_lds + (long)n * tile;
    for (int i = threadIdx.x; i < n / 2; i += 256) tw[i] = a.tw[i];
    const long tiles = (a.width + tile - 1) >> a.log2t;
    const long items = a.outer * tiles;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const long o = it / tiles, w0 = (it - o * tiles) << a.log2t;
        cplx *base = a.spec + o * n * a.width;
        __syncthreads();
        for (int e = threadIdx.x; e < n * tile; e += 256) {
            const int idx = e >> a.log2t, c = e & (tile - 1);
            cplx v;
            v.x = 0.0; v.y = 0.0;
            if (w0 + c < a.width) v = base[(long)idx * a.width + w0 + c];       // (a ragged tile: the columns past the end are zeros)
            x[(long)bit_reverse((unsigned)idx, a.log2n) * tile + c] = v;
        }
        fft_stages(x, tw, a.log2n, tile, a.log2t, tile, 1);
        for (int e = threadIdx.x; e < n * tile; e += 256) {
            const int idx = e >> a.log2t, c = e & (tile - 1);
            if (w0 + c < a.width) base[(long)idx * a.width + w0 + c] = x[(long)idx * tile + c];
        }
    }
}

// ---- the inverse: the same butterflies with conjugated twiddles, axis 0, then axis 1, then the fastest axis ---------------------------------
// LDS, tiles and the ragged-tile rule of fft_lines_kernel
__global__ void __launch_bounds__(256) inverse_lines_kernel(LinesArgs a)
{
    extern __shared__ cplx fft_lds[];
    const int n = 1 << a.log2n, tile = 1 << a.log2t;
    cplx *x = fft_lds, *tw = fft_lds + (long)n * tile;
    for (int i = threadIdx.x; i < n / 2; i += 256) {
        cplx w = a.tw[i];
        w.y = -w.y;
        tw[i] = w;
    }
    const long tiles = (a.width + tile - 1) >> a.log2t;
    const long items = a.outer * tiles;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const long o = it / tiles, w0 = (it - o * tiles) << a.log2t;
        cplx *base = a.spec + o * n * a.width;
        __syncthreads();
        for (int e = threadIdx.x; e < n * tile; e += 256) {
            const int idx = e >> a.log2t, c = e & (tile - 1);
            cplx v;
            v.x = 0.0; v.y = 0.0;
            if (w0 + c < a.width) v = base[(long)idx * a.width + w0 + c];
            x[(long)bit_reverse((unsigned)idx, a.log2n) * tile + c] = v;
        }
        fft_stages(x, tw, a.log2n, tile, a.log2t, tile, 1);
        for (int e = threadIdx.x; e < n * tile; e += 256) {
            const int idx = e >> a.log2t, c = e & (tile - 1);
            if (w0 + c < a.width) base[(long)idx * a.width + w0 + c] = x[(long)idx * tile + c];
        }
    }
}

struct InvRowsArgs {
    RowGrid g;
    long pc;                       // elements of one component of the field
    long rows;                     // n0 * n1
    int log2n, batch, nh;          // N = n2 = 1 << log2n; rows of one batch; n2 / 2 + 1
    double inv_size;               // 1 / (n0 n1 n2): a power of two
    const cplx *in;                // (components, rows, nh)
    void *out;                     // component 0; workgroup row blockIdx.y takes component blockIdx.y
    const cplx *tw;                // n2 / 2 twiddles of the forward transform
};

// LDS: batch * N elements, then N / 2 twiddles
template <typename T>
__global__ void __launch_bounds__(256) inverse_rows_kernel(InvRowsArgs a)
{
    extern __shared__ cplx fft_lds[];
    const int n = 1 << a.log2n;
    cplx *x = fft_lds, *tw = fft_lds + (long)a.batch * n;
    for (int i = threadIdx.x; i < n / 2; i += 256) {
        cplx w = a.tw[i];
        w.y = -w.y;
        tw[i] = w;
    }
    const cplx *in = a.in + (long)blockIdx.y * a.rows * a.nh;
    T *out = (T *)a.out + (long)blockIdx.y * a.pc;
    const long batches = (a.rows + a.batch - 1) / a.batch;
    for (long bt = blockIdx.x; bt < batches; bt += gridDim.x) {
        __syncthreads();                                       // (the stores of the batch before have read the lines)
        for (int e = threadIdx.x; e < a.batch * n; e += 256) {
            const int b = e >> a.log2n, idx = e & (n - 1);
            const long row = bt * a.batch + b;
            cplx v;
            v.x = 0.0; v.y = 0.0;
            if (row < a.rows) {
                if (2 * idx <= n) v = in[row * a.nh + idx];                     // stored, with whatever imaginary part sits at 0 and N / 2
                else { v = in[row * a.nh + (n - idx)]; v.y = -v.y; }             // the mirror image
            }
            x[(long)b * n + bit_reverse((unsigned)idx, a.log2n)] = v;
        }
        fft_stages(x, tw, a.log2n, a.batch, -1, 1, n);
        for (int e = threadIdx.x; e < a.batch * n; e += 256) {
            const int b = e >> a.log2n, k = e & (n - 1);
            const long row = bt * a.batch + b;
            if (row < a.rows) {
                const long i = row / a.g.n1, j = row - i * a.g.n1;
                out[a.g.off + i * a.g.p0 + j * a.g.p1 + k] = (T)(x[(long)b * n + k].x * a.inv_size);
            }
        }
    }
}

// ---- shells -----------------------------------------------------------------------------------------------------------------------------------
struct ShellArgs {
    unsigned n0, n1, n2, nh;
    long total;                    // n0 * n1 * nh modes of the half spectrum
    int nbins;
    const cplx *spec;              // one component
    const double *kfreq;           // n0 + n1 + n2 frequencies (normalised axes)
    const double *edges;           // nbins + 1
    unsigned long long *counts;    // nbins + 2, or NULL (every component but the first)
    unsigned long long *maxbits;   // nbins + 2
    int2 *params;                  // nbins + 2: (eh, L), L < 0: no limbs for this shell
    long long *limb;               // 3 * (nbins + 2)
};

// the slot of |k|: e[b] <= k < e[b + 1], the last bin closed (pdehip_histogram); nbins: below, nbins + 1: above
__device__ __forceinline__ int shell_slot(const double *edge, int nb, double k)
{
    if (k < edge[0]) return nb;
    if (k > edge[nb]) return nb + 1;
    int l = 0, h = nb - 1;
    while (l < h) {
        const int mid = (l + h + 1) >> 1;
        if (edge[mid] <= k) l = mid; else h = mid - 1;
    }
    return l;
}
// mode t of the half spectrum: its slot, its weight and its weighted power
__device__ __forceinline__ void shell_mode(const ShellArgs &a, const double *edge, long t, int *slot, unsigned *weight, double *power)
{
    const unsigned ut = (unsigned)t;
    const unsigned k = ut % a.nh, rest = ut / a.nh;
    const unsigned j = rest % a.n1, i = rest / a.n1;
    const double f0 = a.kfreq[i], f1 = a.kfreq[a.n0 + j], f2 = a.kfreq[a.n0 + a.n1 + k];
    const double kk = sqrt((f0 * f0 + f1 * f1) + f2 * f2);
    *slot = shell_slot(edge, a.nbins, kk);
    const unsigned w = (k > 0 && 2 * k < a.n2) ? 2u : 1u;
    const cplx z = a.spec[t];
    const double p = z.x * z.x + z.y * z.y;
    *weight = w;
    *power = w == 2u ? 2.0 * p : p;
}

__device__ __forceinline__ long long wave_add64(long long v)
{
#pragma unroll
    for (int ofs = 32; ofs >= 1; ofs >>= 1) v += __shfl_xor(v, ofs, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_max64(unsigned long long v)
{
#pragma unroll
    for (int ofs = 32; ofs >= 1; ofs >>= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)v, ofs, 64);
        v = o > v ? o : v;
    }
    return v;
}

// LDS: nbins + 1 edges, nbins + 2 maxima (64 bits), nbins + 2 counters (32 bits) - 81 964 bytes at 4096 bins
__global__ void __launch_bounds__(256) shell_max_kernel(ShellArgs a)
{
    extern __shared__ double shell_lds[];
    const int nb = a.nbins, lane = threadIdx.x & 63;
    double *edge = shell_lds;
    unsigned long long *mx = (unsigned long long *)(shell_lds + nb + 1);
    unsigned *cnt = (unsigned *)(mx + nb + 2);
    for (int i = threadIdx.x; i <= nb; i += 256) edge[i] = a.edges[i];
    for (int i = threadIdx.x; i < nb + 2; i += 256) { mx[i] = 0; cnt[i] = 0; }
    __syncthreads();
    const long stride = (long)gridDim.x * 256;
    for (long base = (long)blockIdx.x * 256; base < a.total; base += stride) {       // (uniform in the workgroup: every lane takes part in the votes)
        const long t = base + threadIdx.x;
        bool active = t < a.total;
        int slot = 0;
        unsigned w = 0;
        double p = 0.0;
        if (active) shell_mode(a, edge, t, &slot, &w, &p);
        const unsigned long long bits = (unsigned long long)__double_as_longlong(p);     // p >= 0 or NaN: ordered like the integers
#pragma unroll
        for (int r = 0; r < 2; r++) {          // the lanes that share the slot of the first remaining lane: one set of LDS atomics
            const unsigned long long act = __ballot(active);
            if (act) {
                const int src = __ffsll((long long)act) - 1;
                const int first = __shfl(slot, src);
                const bool in = active && slot == first;
                const unsigned long long m = wave_max64(in ? bits : 0ULL);
                const long long c = wave_add64(in ? (long long)w : 0LL);
                if (lane == src) { atomicMax(&mx[first], m); atomicAdd(&cnt[first], (unsigned)c); }
                active = active && !in;
            }
        }
        if (active) { atomicMax(&mx[slot], bits); atomicAdd(&cnt[slot], w); }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb + 2; i += 256) {
        if (mx[i]) atomicMax(&a.maxbits[i], mx[i]);
        if (a.counts && cnt[i]) atomicAdd(&a.counts[i], (unsigned long long)cnt[i]);
    }
}

// E with m = x 2^-E in [1/2, 1) for the bit image of a finite x > 0 (frexp, subnormal numbers included)
__host__ __device__ inline int exponent_of(unsigned long long bits)
{
    const int e = (int)((bits >> 52) & 0x7ff);
    if (e) return e - 1022;
    return (63 - __builtin_clzll(bits)) - 1073;
}
// (eh, L) of a shell whose largest weighted power has the bit image `bits` and which holds `count` modes: L = ceil(log2(count)),
// eh = E - (62 - L).  L = -1: no limbs (an empty shell, a maximum of zero, or one that is not finite - the sum is the maximum itself).
__host__ __device__ inline void limb_params(unsigned long long bits, unsigned long long count, int *eh, int *L)
{
    *eh = 0; *L = -1;
    if (count == 0 || bits == 0 || bits >= 0x7ff0000000000000ULL) return;
    int l = 0;
    while ((1ULL << l) < count) l++;
    *L = l;
    *eh = exponent_of(bits) - (62 - l);
}

__global__ void __launch_bounds__(256) shell_params_kernel(const unsigned long long *maxbits, const unsigned long long *counts, int2 *params, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int eh, L;
    limb_params(maxbits[i], counts[i], &eh, &L);
    params[i] = make_int2(eh, L);
}

// LDS: nbins + 1 edges, 3 (nbins + 2) limbs - 131 116 bytes at 4096 bins
__global__ void __launch_bounds__(256) shell_limb_kernel(ShellArgs a)
{
    extern __shared__ double shell_lds[];
    const int nb = a.nbins, lane = threadIdx.x & 63;
    double *edge = shell_lds;
    unsigned long long *limb = (unsigned long long *)(shell_lds + nb + 1);
    for (int i = threadIdx.x; i <= nb; i += 256) edge[i] = a.edges[i];
    for (int i = threadIdx.x; i < 3 * (nb + 2); i += 256) limb[i] = 0;
    __syncthreads();
    const long stride = (long)gridDim.x * 256;
    for (long base = (long)blockIdx.x * 256; base < a.total; base += stride) {
        const long t = base + threadIdx.x;
        bool active = t < a.total;
        int slot = 0;
        long long h = 0, m = 0, l = 0;
        if (active) {
            unsigned w;
            double v;
            shell_mode(a, edge, t, &slot, &w, &v);
            const int2 par = a.params[slot];
            if (par.y < 0) {
                active = false;
            } else {
                // three limbs, D = 63 - L bits apart: hi counts units of 2^eh, mid of 2^(eh - D), lo of 2^(eh - 2 D); v <= 2^E
                const int D = 63 - par.y, eh = par.x, em = eh - D, el = em - D;
                const double fh = rint(ldexp(v, -eh));
                const double r1 = v - ldexp(fh, eh);               // exact
                const double fm = rint(ldexp(r1, -em));
                const double r2 = r1 - ldexp(fm, em);              // exact
                const double fl = rint(ldexp(r2, -el));
                h = (long long)fh; m = (long long)fm; l = (long long)fl;
            }
        }
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const unsigned long long act = __ballot(active);
            if (act) {
                const int src = __ffsll((long long)act) - 1;
                const int first = __shfl(slot, src);
                const bool in = active && slot == first;
                const long long sh = wave_add64(in ? h : 0LL), sm = wave_add64(in ? m : 0LL), sl = wave_add64(in ? l : 0LL);
                if (lane == src) {
                    atomicAdd(&limb[3 * first], (unsigned long long)sh);
                    atomicAdd(&limb[3 * first + 1], (unsigned long long)sm);
                    atomicAdd(&limb[3 * first + 2], (unsigned long long)sl);
                }
                active = active && !in;
            }
        }
        if (active) {
            atomicAdd(&limb[3 * slot], (unsigned long long)h);
            atomicAdd(&limb[3 * slot + 1], (unsigned long long)m);
            atomicAdd(&limb[3 * slot + 2], (unsigned long long)l);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * (nb + 2); i += 256)
        if (limb[i]) atomicAdd((unsigned long long *)a.limb + i, limb[i]);
}

// The sum of a shell from its limbs, rounded ONCE to nearest: the limbs are carried into three non-negative digits D bits apart, the
// 64 leading bits of the 3 D-bit integer and a sticky bit for the rest are converted (the same lines: tests/shim).
double limbs_to_double(long long lh, long long lm, long long ll, int eh, int L)
{
    const int D = 63 - L, el = eh - 2 * D;
    const long long mask = (long long)((1ULL << D) - 1);
    lm += ll >> D; ll &= mask;                 // (>> of a negative integer: towards minus infinity, which is the carry of a floor)
    lh += lm >> D; lm &= mask;
    if (lh < 0) return 0.0;                    // (never: every term is a rounded non-negative number)
    unsigned long long w[4] = {0, 0, 0, 0};
    const unsigned long long digit[3] = {(unsigned long long)ll, (unsigned long long)lm, (unsigned long long)lh};
    for (int q = 0; q < 3; q++) {
        const int at = q * D, word = at >> 6, bit = at & 63;
        w[word] |= digit[q] << bit;
        if (bit) w[word + 1] |= digit[q] >> (64 - bit);
    }
    int top = 2;
    while (top > 0 && !w[top]) top--;
    if (top == 0) return ldexp((double)w[0], el);
    const int msb = 63 - __builtin_clzll(w[top]);
    const int s = 64 * top + msb - 63;         // the window: bits s ... s + 63
    const int word = s >> 6, bit = s & 63;
    unsigned long long win = w[word] >> bit;
    if (bit) win |= w[word + 1] << (64 - bit);
    bool sticky = bit && (w[word] & ((1ULL << bit) - 1));
    for (int q = 0; q < word; q++) sticky = sticky || w[q];
    return ldexp((double)(win | (sticky ? 1ULL : 0ULL)), el + s);
}

// ---- per stream (FftScratch, pdehip_fft.h) ----------------------------------------------------------------------------------------------------
int release_fft();
StreamTable<FftScratch> g_fft(release_fft);

void free_entry(FftScratch &s)
{
    (void)hipFree(s.tw_dev); (void)hipFree(s.kf_dev); (void)hipFree(s.spec); (void)hipFree(s.maxbits); (void)hipFree(s.params);
    (void)hipFree(s.limb); (void)hipFree(s.mu_dev); (void)hipFree(s.sol_x); (void)hipFree(s.sol_w); (void)hipFree(s.sol_ctl);
    (void)hipHostFree(s.tw_host); (void)hipHostFree(s.edges_host); (void)hipHostFree(s.host); (void)hipHostFree(s.mu_host); (void)hipHostFree(s.sol_pinned);
    memset(&s, 0, sizeof(s));
}
int release_fft() { return g_fft.release(free_entry); }

// the tables of the three axes on the device (made again only when an extent differs from the call before on this stream)
int fft_tables(hipStream_t st, const long n[3], const cplx **tw)
{
    return g_fft.with(st, [&](FftScratch &s) -> int {
        if (!s.tw_dev) {
            PDEHIP_HIP(hipMalloc((void **)&s.tw_dev, sizeof(cplx) * kFftFastMax));
            PDEHIP_HIP(hipHostMalloc((void **)&s.tw_host, sizeof(cplx) * kFftFastMax, hipHostMallocDefault));
        }
        if (s.tw_n[0] != n[0] || s.tw_n[1] != n[1] || s.tw_n[2] != n[2]) {
            PDEHIP_HIP(hipStreamSynchronize(st));          // (a copy of the tables before may still read the pinned memory)
            long at = 0;
            for (int ax = 0; ax < 3; ax++)
                for (long m = 0; m < n[ax] / 2; m++, at++) twiddle(m, n[ax], &s.tw_host[at].x, &s.tw_host[at].y);
            if (at) PDEHIP_HIP(hipMemcpyAsync(s.tw_dev, s.tw_host, sizeof(cplx) * at, hipMemcpyHostToDevice, st));
            for (int ax = 0; ax < 3; ax++) s.tw_n[ax] = n[ax];
        }
        tw[0] = s.tw_dev; tw[1] = s.tw_dev + n[0] / 2; tw[2] = s.tw_dev + n[0] / 2 + n[1] / 2;
        return 0;
    });
}

int grow_spectrum(FftScratch &s, size_t spec_bytes)
{
    if (s.spec_bytes < spec_bytes) {
        if (s.spec) PDEHIP_HIP(hipFree(s.spec));       // (hipFree waits for the device)
        s.spec = nullptr; s.spec_bytes = 0;
        const hipError_t e = hipMalloc((void **)&s.spec, spec_bytes);
        if (e != hipSuccess) PDEHIP_FAIL(100 + (int)e, "hipMalloc of %zu bytes for the spectrum failed: %s", spec_bytes, hipGetErrorString(e));
        s.spec_bytes = spec_bytes;
    }
    return 0;
}

int shell_scratch(hipStream_t st, size_t spec_bytes, size_t slots, FftScratch *out)
{
    return g_fft.with(st, [&](FftScratch &s) -> int {
        if (!s.kf_dev) {
            PDEHIP_HIP(hipMalloc((void **)&s.kf_dev, sizeof(double) * (2 * kFftSlowMax + kFftFastMax)));
            PDEHIP_HIP(hipHostMalloc((void **)&s.edges_host, sizeof(double) * (kShellBinsMax + 1), hipHostMallocDefault));
            PDEHIP_HIP(hipMalloc((void **)&s.params, sizeof(int2) * (kShellBinsMax + 2)));
        }
        PDEHIP_TRY(grow_spectrum(s, spec_bytes));
        if (s.slots < slots) {
            if (s.maxbits) PDEHIP_HIP(hipFree(s.maxbits));
            if (s.limb) PDEHIP_HIP(hipFree(s.limb));
            if (s.host) PDEHIP_HIP(hipHostFree(s.host));
            s.maxbits = nullptr; s.limb = nullptr; s.host = nullptr; s.slots = 0;
            PDEHIP_HIP(hipMalloc((void **)&s.maxbits, sizeof(unsigned long long) * slots));
            PDEHIP_HIP(hipMalloc((void **)&s.limb, sizeof(long long) * 3 * slots));
            PDEHIP_HIP(hipHostMalloc((void **)&s.host, sizeof(unsigned long long) * 6 * slots, hipHostMallocDefault));
            s.slots = slots;
        }
        *out = s;
        return 0;
    });
}

int log2_of(long n)
{
    int l = 0;
    while ((1L << l) < n) l++;
    return l;
}

}  // namespace

StreamTable<FftScratch> &fft_table() { return g_fft; }

// 0, or the refusal of the dry run: every normalised axis absent or a power of two up to 1024, the fastest up to 4096
int fft_check(const pdehip_grid_t *g, NGrid *n)
{
    PDEHIP_TRY(norm_grid(g, n));
    for (int a = 0; a < n->ndim; a++) {
        const int ax = 3 - n->ndim + a;
        const long ext = n->n[ax], cap = ax == 2 ? kFftFastMax : kFftSlowMax;
        if ((ext & (ext - 1)) != 0 || ext > cap)
            PDEHIP_FAIL(E_NOTIMPL, "fft: axis %d has %ld cells; a power of two up to %ld is needed (%ld on the fastest axis)", a, ext, cap, kFftFastMax);
    }
    return 0;
}

namespace {

// every launch asks for its dynamic LDS: up to 136 KiB of the CU's 160 KiB
template <class K>
int allow_lds(K kernel, size_t bytes)
{
    if (bytes > 65536) PDEHIP_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}

}  // namespace

namespace fft {

int spectrum_scratch(hipStream_t st, size_t spec_bytes, cplx **spec)
{
    return g_fft.with(st, [&](FftScratch &s) -> int {
        PDEHIP_TRY(grow_spectrum(s, spec_bytes));
        *spec = s.spec;
        return 0;
    });
}

// the transform of `ncomp` components of `in` into `spec` (ncomp, n0, n1, nh); the names of the launches are appended to `names`
int forward(const NGrid &n, int ncomp, const void *in, cplx *spec, hipStream_t st, std::string *names)
{
    const cplx *tw[3];
    PDEHIP_TRY(fft_tables(st, n.n, tw));
    const long nh = n.n[2] / 2 + 1;
    {
        RowsArgs a;
        a.g = make_row_grid(n); a.pc = n.pc; a.rows = n.n[0] * n.n[1]; a.log2n = log2_of(n.n[2]); a.nh = (int)nh;
        a.batch = (int)(n.n[2] >= 512 ? 1 : 512 / n.n[2]);
        a.in = in; a.out = spec; a.tw = tw[2];
        const long batches = (a.rows + a.batch - 1) / a.batch;
        const size_t lds = sizeof(cplx) * ((size_t)a.batch * n.n[2] + n.n[2] / 2);
        const dim3 grid(clamp_blocks(batches, kFftBlocksMax), ncomp);
        if (n.dtype == PDEHIP_F64) {
            PDEHIP_TRY(allow_lds(&fft_rows_kernel<double>, lds));
            hipLaunchKernelGGL((fft_rows_kernel<double>), grid, dim3(256), lds, st, a);
        } else {
            PDEHIP_TRY(allow_lds(&fft_rows_kernel<float>, lds));
            hipLaunchKernelGGL((fft_rows_kernel<float>), grid, dim3(256), lds, st, a);
        }
        PDEHIP_HIP(hipGetLastError());
        *names += n.dtype == PDEHIP_F64 ? "fft_rows_kernel<double>" : "fft_rows_kernel<float>";
    }
    for (int ax = 1; ax >= 0; ax--) {
        if (n.n[ax] < 2) continue;
        LinesArgs a;
        a.spec = spec; a.log2n = log2_of(n.n[ax]); a.tw = tw[ax];
        a.outer = ax == 1 ? (long)ncomp * n.n[0] : (long)ncomp;
        a.width = ax == 1 ? nh : n.n[1] * nh;
        const long tile = n.n[ax] * kTileMin >= kTileElems ? kTileMin : kTileElems / n.n[ax];
        a.log2t = log2_of(tile);
        const long items = a.outer * ((a.width + tile - 1) / tile);
        const size_t lds = sizeof(cplx) * ((size_t)n.n[ax] * tile + n.n[ax] / 2);
        PDEHIP_TRY(allow_lds(&fft_lines_kernel, lds));
        hipLaunchKernelGGL(fft_lines_kernel, dim3(clamp_blocks(items, kFftBlocksMax)), dim3(256), lds, st, a);
        PDEHIP_HIP(hipGetLastError());
        *names += "+fft_lines_kernel";
    }
    return 0;
}

// The inverse of `forward`: axis 0, then axis 1 of the half spectrum in place (`spec` is consumed), then every row of the fastest axis
// as a full complex line; the real part times 1 / size goes to the interior cells of `out`, a full array of n.  The names of the
// launches are appended to `names`, joined by '+'.
int inverse(const NGrid &n, int ncomp, cplx *spec, void *out, hipStream_t st, std::string *names)
{
    const cplx *tw[3];
    PDEHIP_TRY(fft_tables(st, n.n, tw));
    const long nh = n.n[2] / 2 + 1;
    for (int ax = 0; ax <= 1; ax++) {
        if (n.n[ax] < 2) continue;
        LinesArgs a;
        a.spec = spec; a.log2n = log2_of(n.n[ax]); a.tw = tw[ax];
        a.outer = ax == 1 ? (long)ncomp * n.n[0] : (long)ncomp;
        a.width = ax == 1 ? nh : n.n[1] * nh;
        const long tile = n.n[ax] * kTileMin >= kTileElems ? kTileMin : kTileElems / n.n[ax];
        a.log2t = log2_of(tile);
        const long items = a.outer * ((a.width + tile - 1) / tile);
        const size_t lds = sizeof(cplx) * ((size_t)n.n[ax] * tile + n.n[ax] / 2);
        PDEHIP_TRY(allow_lds(&inverse_lines_kernel, lds));
        hipLaunchKernelGGL(inverse_lines_kernel, dim3(clamp_blocks(items, kFftBlocksMax)), dim3(256), lds, st, a);
        PDEHIP_HIP(hipGetLastError());
        *names += "inverse_lines_kernel+";
    }
    InvRowsArgs a;
    a.g = make_row_grid(n); a.pc = n.pc; a.rows = n.n[0] * n.n[1]; a.log2n = log2_of(n.n[2]); a.nh = (int)nh;
    a.batch = (int)(n.n[2] >= 512 ? 1 : 512 / n.n[2]);
    a.inv_size = 1.0 / (double)(n.n[0] * n.n[1] * n.n[2]);
    a.in = spec; a.out = out; a.tw = tw[2];
    const long batches = (a.rows + a.batch - 1) / a.batch;
    const size_t lds = sizeof(cplx) * ((size_t)a.batch * n.n[2] + n.n[2] / 2);
    const dim3 grid(clamp_blocks(batches, kFftBlocksMax), ncomp);
    if (n.dtype == PDEHIP_F64) {
        PDEHIP_TRY(allow_lds(&inverse_rows_kernel<double>, lds));
        hipLaunchKernelGGL((inverse_rows_kernel<double>), grid, dim3(256), lds, st, a);
    } else {
        PDEHIP_TRY(allow_lds(&inverse_rows_kernel<float>, lds));
        hipLaunchKernelGGL((inverse_rows_kernel<float>), grid, dim3(256), lds, st, a);
    }
    PDEHIP_HIP(hipGetLastError());
    *names += n.dtype == PDEHIP_F64 ? "inverse_rows_kernel<double>" : "inverse_rows_kernel<float>";
    return 0;
}

}  // namespace fft
}  // namespace pdehip

using namespace pdehip;
using pdehip::fft::forward;
using pdehip::fft::inverse;

extern "C" int pdehip_fft_supported(const pdehip_grid_t *g)
{
    NGrid n;
    return fft_check(g, &n);
}

extern "C" int pdehip_fft_forward(const pdehip_grid_t *g, int ncomp, const void *arr_full, void *spectrum_dev, void *stream)
{
    NGrid n;
    PDEHIP_TRY(fft_check(g, &n));
    if (!arr_full || !spectrum_dev) PDEHIP_FAIL(E_VALUE, "fft_forward: NULL pointer");
    if (ncomp < 1 || ncomp > 64) PDEHIP_FAIL(E_VALUE, "fft_forward: 1..64 components");
    if ((((uintptr_t)arr_full | (uintptr_t)spectrum_dev) & 15) != 0) PDEHIP_FAIL(E_VALUE, "fft_forward: misaligned array (16 bytes for the field and the spectrum)");
    std::string names;
    PDEHIP_TRY(forward(n, ncomp, arr_full, (cplx *)spectrum_dev, as_stream(stream), &names));
    note_kernel("%s", names.c_str());
    return 0;
}

extern "C" int pdehip_fft_inverse(const pdehip_grid_t *g, int ncomp, void *spectrum_dev, void *out_full, void *stream)
{
    NGrid n;
    PDEHIP_TRY(fft_check(g, &n));
    if (!spectrum_dev || !out_full) PDEHIP_FAIL(E_VALUE, "fft_inverse: NULL pointer");
    if (ncomp < 1 || ncomp > 64) PDEHIP_FAIL(E_VALUE, "fft_inverse: 1..64 components");
    if ((((uintptr_t)spectrum_dev | (uintptr_t)out_full) & 15) != 0) PDEHIP_FAIL(E_VALUE, "fft_inverse: misaligned array (16 bytes for the spectrum and the field)");
    std::string names;
    PDEHIP_TRY(inverse(n, ncomp, (cplx *)spectrum_dev, out_full, as_stream(stream), &names));
    note_kernel("%s", names.c_str());
    return 0;
}

extern "C" int pdehip_shell_spectrum(const pdehip_grid_t *g, int ncomp, const void *arr_full, const double *kfreq_dev, int nbins,
                                     const double *edges_dev, uint64_t *counts_dev, double *sums_dev, void *stream)
{
    NGrid n;
    PDEHIP_TRY(fft_check(g, &n));
    if (!arr_full || !kfreq_dev || !edges_dev || !counts_dev || !sums_dev) PDEHIP_FAIL(E_VALUE, "shell_spectrum: NULL pointer");
    if (ncomp < 1 || ncomp > 64) PDEHIP_FAIL(E_VALUE, "shell_spectrum: 1..64 components");
    if (nbins < 1 || nbins > kShellBinsMax) PDEHIP_FAIL(E_VALUE, "shell_spectrum: 1..%d bins (got %d)", kShellBinsMax, nbins);
    if (((uintptr_t)arr_full & 15) != 0 || (((uintptr_t)kfreq_dev | (uintptr_t)edges_dev | (uintptr_t)counts_dev | (uintptr_t)sums_dev) & 7) != 0)
        PDEHIP_FAIL(E_VALUE, "shell_spectrum: misaligned array (16 bytes for the field, 8 for frequencies, edges, counts and sums)");
    hipStream_t st = as_stream(stream);
    const long nh = n.n[2] / 2 + 1, total = n.n[0] * n.n[1] * nh;
    const int ns = nbins + 2;
    FftScratch s;
    PDEHIP_TRY(shell_scratch(st, sizeof(cplx) * (size_t)total, (size_t)ncomp * ns, &s));
    // the edges decide every count: they are checked here, on the host, as pdehip_histogram checks them
    double *e = s.edges_host;
    PDEHIP_HIP(hipMemcpyAsync(e, edges_dev, sizeof(double) * (nbins + 1), hipMemcpyDeviceToHost, st));
    PDEHIP_HIP(hipStreamSynchronize(st));
    for (int i = 0; i <= nbins; i++) {
        if (!std::isfinite(e[i])) PDEHIP_FAIL(E_VALUE, "shell_spectrum: edge %d is not finite", i);
        if (i > 0 && !(e[i] > e[i - 1])) PDEHIP_FAIL(E_VALUE, "shell_spectrum: the edges must increase strictly (edge %d)", i);
    }
    // the frequencies of the normalised axes: an axis the grid does not have has the one frequency 0
    PDEHIP_HIP(hipMemsetAsync(s.kf_dev, 0, sizeof(double) * (n.n[0] + n.n[1] + n.n[2]), st));
    {
        long at_in = 0, at_out = 0;
        for (int ax = 0; ax < 3; ax++) {
            if (ax >= 3 - n.ndim) {
                PDEHIP_HIP(hipMemcpyAsync(s.kf_dev + at_out, kfreq_dev + at_in, sizeof(double) * n.n[ax], hipMemcpyDeviceToDevice, st));
                at_in += n.n[ax];
            }
            at_out += n.n[ax];
        }
    }
    PDEHIP_HIP(hipMemsetAsync(counts_dev, 0, sizeof(uint64_t) * ns, st));
    PDEHIP_HIP(hipMemsetAsync(s.maxbits, 0, sizeof(unsigned long long) * (size_t)ncomp * ns, st));
    PDEHIP_HIP(hipMemsetAsync(s.limb, 0, sizeof(long long) * 3 * (size_t)ncomp * ns, st));

    ShellArgs a;
    a.n0 = (unsigned)n.n[0]; a.n1 = (unsigned)n.n[1]; a.n2 = (unsigned)n.n[2]; a.nh = (unsigned)nh; a.total = total; a.nbins = nbins;
    a.spec = s.spec; a.kfreq = s.kf_dev; a.edges = edges_dev; a.params = s.params;
    const unsigned blocks = blocks_for(total, kShellBlocksMax);
    const size_t lds_max = sizeof(double) * (nbins + 1) + 12 * (size_t)ns, lds_limb = sizeof(double) * (nbins + 1) + 24 * (size_t)ns;
    PDEHIP_TRY(allow_lds(&shell_max_kernel, lds_max));
    PDEHIP_TRY(allow_lds(&shell_limb_kernel, lds_limb));
    std::string names;
    const long pc_bytes = n.pc * elem_size(n.dtype);
    for (int c = 0; c < ncomp; c++) {
        names.clear();
        PDEHIP_TRY(forward(n, 1, (const char *)arr_full + (size_t)c * pc_bytes, s.spec, st, &names));
        a.counts = c == 0 ? (unsigned long long *)counts_dev : nullptr;
        a.maxbits = s.maxbits + (size_t)c * ns;
        a.limb = s.limb + 3 * (size_t)c * ns;
        hipLaunchKernelGGL(shell_max_kernel, dim3(blocks), dim3(256), lds_max, st, a);
        hipLaunchKernelGGL(shell_params_kernel, dim3((ns + 255) / 256), dim3(256), 0, st, a.maxbits, (const unsigned long long *)counts_dev, s.params, ns);
        hipLaunchKernelGGL(shell_limb_kernel, dim3(blocks), dim3(256), lds_limb, st, a);
        PDEHIP_HIP(hipGetLastError());
    }
    names += "+shell_max_kernel+shell_params_kernel+shell_limb_kernel";
    note_kernel("%s", names.c_str());
    // the limbs become sums on the host, rounded once each (the caller reads them next): maxima, limbs and counts come down, the sums go up
    const size_t slots = (size_t)ncomp * ns;
    unsigned long long *h_max = s.host, *h_cnt = s.host + slots;
    long long *h_limb = (long long *)(s.host + 2 * slots);
    double *h_sum = (double *)(s.host + 5 * slots);
    PDEHIP_HIP(hipMemcpyAsync(h_max, s.maxbits, sizeof(unsigned long long) * slots, hipMemcpyDeviceToHost, st));
    PDEHIP_HIP(hipMemcpyAsync(h_cnt, counts_dev, sizeof(unsigned long long) * ns, hipMemcpyDeviceToHost, st));
    PDEHIP_HIP(hipMemcpyAsync(h_limb, s.limb, sizeof(long long) * 3 * slots, hipMemcpyDeviceToHost, st));
    PDEHIP_HIP(hipStreamSynchronize(st));
    for (int c = 0; c < ncomp; c++)
        for (int i = 0; i < ns; i++) {
            const size_t at = (size_t)c * ns + i;
            int eh, L;
            limb_params(h_max[at], h_cnt[i], &eh, &L);
            if (L < 0) memcpy(&h_sum[at], &h_max[at], 8);          // zero, infinity or NaN: the maximum itself
            else h_sum[at] = limbs_to_double(h_limb[3 * at], h_limb[3 * at + 1], h_limb[3 * at + 2], eh, L);
        }
    PDEHIP_HIP(hipMemcpyAsync(sums_dev, h_sum, sizeof(double) * slots, hipMemcpyHostToDevice, st));
    PDEHIP_HIP(hipStreamSynchronize(st));
    return 0;
}
