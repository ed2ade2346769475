/*
 * pdehip_shim_spectrum.c — HOST implementation of pdehip_fft_supported, pdehip_fft_forward and pdehip_shell_spectrum (include/pdehip.h).
 * TESTS ONLY.
 *
 * An addition to the host shim (pdehip_shim.c, see the notice there): tests/spectrum_shimlib.py links this file with the shim's objects
 * into tests/shim/_build/libpdehip_shim_spectrum.so, so that pde_hip/spectrum.py runs through the REAL py-pde without a GPU, and so that
 * the device kernels (csrc/pdehip_fft.hip) have a serial statement of their arithmetic to be compared with bit by bit.  The product never
 * builds or loads it.
 *
 * Plain serial C on the shim's layout (pdehip_layout): one line at a time through the schedule the header describes - bit reversal, then
 * log2(N) in-place radix-2 stages with the twiddles of the host table - and per mode the three limbs, added in C order.  No tiles, no
 * LDS, no waves: what is shared with the device code is the table, the butterfly, the limbs and their conversion, nothing else.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/pdehip.h"

int shim_set_error(int code, const char *msg);

typedef struct { double re, im; } cplx_t;

typedef struct {
    long n[3], p[3];       /* normalised axes: cells and pitches */
    long pc, off;
    int ndim, f64;
} rows_t;

static int make_rows(const pdehip_grid_t *g, rows_t *r)
{
    int64_t lay[8];
    int rc = pdehip_layout(g, lay);
    if (rc) return rc;
    r->n[0] = r->n[1] = r->n[2] = 1;
    for (int d = 0; d < g->ndim; d++) r->n[3 - g->ndim + d] = (long)g->shape[d];
    r->p[0] = (long)lay[0]; r->p[1] = (long)lay[1]; r->p[2] = 1;
    r->pc = (long)lay[2]; r->off = (long)lay[3];
    r->ndim = g->ndim;
    r->f64 = g->dtype == PDEHIP_F64;
    return 0;
}

static int check_extents(const pdehip_grid_t *g, rows_t *r)
{
    int rc = make_rows(g, r);
    if (rc) return rc;
    for (int ax = 3 - r->ndim; ax < 3; ax++) {
        const long ext = r->n[ax], cap = ax == 2 ? 4096 : 1024;
        if ((ext & (ext - 1)) != 0 || ext > cap) return shim_set_error(2, "shim: fft: an axis is not a power of two within the limits");
    }
    return 0;
}

/* exp(-2 pi i m / N), 0 <= m < N / 2, from an angle in the first octant (the same lines: csrc/pdehip_fft.hip) */
static void twiddle(long m, long n, double *re, double *im)
{
    long q = m;
    int negate = 0, swap = 0;
    if (4 * q > n) { q = n / 2 - q; negate = 1; }
    if (8 * q > n) { q = n / 4 - q; swap = 1; }
    const double a = 6.283185307179586476925 * (double)q / (double)n;
    double c = cos(a), s = sin(a);
    if (swap) { const double t = c; c = s; s = t; }
    if (negate) c = -c;
    *re = c;
    *im = -s;
}

/* one line of n = 1 << log2n elements `stride` apart, in place: gathered bit-reversed, log2n stages, scattered in natural order */
static void fft_line(cplx_t *x, long stride, int log2n, const cplx_t *tw, cplx_t *work)
{
    const long n = 1L << log2n;
    for (long i = 0; i < n; i++) {
        long rev = 0;
        for (int b = 0; b < log2n; b++) rev |= ((i >> b) & 1L) << (log2n - 1 - b);
        work[rev] = x[i * stride];
    }
    for (int s = 1; s <= log2n; s++) {
        const long half = 1L << (s - 1);
        for (long t = 0; t < n / 2; t++) {
            const long kk = t & (half - 1);
            const long i = ((t >> (s - 1)) << s) + kk;
            const cplx_t w = tw[kk << (log2n - s)], u = work[i], v = work[i + half];
            cplx_t p;
            p.re = w.re * v.re - w.im * v.im;
            p.im = w.re * v.im + w.im * v.re;
            work[i].re = u.re + p.re; work[i].im = u.im + p.im;
            work[i + half].re = u.re - p.re; work[i + half].im = u.im - p.im;
        }
    }
    for (long i = 0; i < n; i++) x[i * stride] = work[i];
}

static int log2_of(long n)
{
    int l = 0;
    while ((1L << l) < n) l++;
    return l;
}

/* the half spectrum (n0, n1, nh) of one component */
static int forward_one(const rows_t *r, const void *arr, cplx_t *spec)
{
    const long n0 = r->n[0], n1 = r->n[1], n2 = r->n[2], nh = n2 / 2 + 1;
    long longest = n2 > n1 ? n2 : n1;
    if (n0 > longest) longest = n0;
    cplx_t *tw = (cplx_t *)malloc(sizeof(cplx_t) * (size_t)(longest / 2 + 1));
    cplx_t *line = (cplx_t *)malloc(sizeof(cplx_t) * (size_t)longest);
    cplx_t *work = (cplx_t *)malloc(sizeof(cplx_t) * (size_t)longest);
    if (!tw || !line || !work) { free(tw); free(line); free(work); return shim_set_error(3, "shim: fft: out of memory"); }
    for (long m = 0; m < n2 / 2; m++) twiddle(m, n2, &tw[m].re, &tw[m].im);
    for (long i = 0; i < n0; i++)
        for (long j = 0; j < n1; j++) {
            const long e = r->off + i * r->p[0] + j * r->p[1];
            for (long k = 0; k < n2; k++) {
                line[k].re = r->f64 ? ((const double *)arr)[e + k] : (double)((const float *)arr)[e + k];
                line[k].im = 0.0;
            }
            fft_line(line, 1, log2_of(n2), tw, work);
            memcpy(spec + (i * n1 + j) * nh, line, sizeof(cplx_t) * (size_t)nh);
        }
    if (n1 > 1) {
        for (long m = 0; m < n1 / 2; m++) twiddle(m, n1, &tw[m].re, &tw[m].im);
        for (long i = 0; i < n0; i++)
            for (long k = 0; k < nh; k++) fft_line(spec + i * n1 * nh + k, nh, log2_of(n1), tw, work);
    }
    if (n0 > 1) {
        for (long m = 0; m < n0 / 2; m++) twiddle(m, n0, &tw[m].re, &tw[m].im);
        for (long w = 0; w < n1 * nh; w++) fft_line(spec + w, n1 * nh, log2_of(n0), tw, work);
    }
    free(tw); free(line); free(work);
    return 0;
}

int pdehip_fft_supported(const pdehip_grid_t *g)
{
    rows_t r;
    return check_extents(g, &r);
}

int pdehip_fft_forward(const pdehip_grid_t *g, int ncomp, const void *arr_full, void *spectrum, void *stream)
{
    (void)stream;
    rows_t r;
    int rc = check_extents(g, &r);
    if (rc) return rc;
    if (!arr_full || !spectrum) return shim_set_error(1, "shim: fft_forward: NULL pointer");
    if (ncomp < 1 || ncomp > 64) return shim_set_error(1, "shim: fft_forward: 1..64 components");
    if ((((uintptr_t)arr_full | (uintptr_t)spectrum) & 15) != 0) return shim_set_error(1, "shim: fft_forward: misaligned array");
    const long per = r.n[0] * r.n[1] * (r.n[2] / 2 + 1);
    const size_t esize = r.f64 ? 8 : 4;
    for (int c = 0; c < ncomp; c++) {
        rc = forward_one(&r, (const char *)arr_full + (size_t)c * (size_t)r.pc * esize, (cplx_t *)spectrum + (size_t)c * per);
        if (rc) return rc;
    }
    return 0;
}

/* ---- shells ------------------------------------------------------------------------------------------------------------------------------ */
static int slot_of(const double *e, int nb, double k)
{
    if (k < e[0]) return nb;
    if (k > e[nb]) return nb + 1;
    int lo = 0, hi = nb - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (e[mid] <= k) lo = mid; else hi = mid - 1;
    }
    return lo;
}

static int exponent_of(uint64_t bits)
{
    const int e = (int)((bits >> 52) & 0x7ff);
    if (e) return e - 1022;
    return (63 - __builtin_clzll(bits)) - 1073;
}
static void limb_params(uint64_t bits, uint64_t count, int *eh, int *L)
{
    *eh = 0; *L = -1;
    if (count == 0 || bits == 0 || bits >= 0x7ff0000000000000ULL) return;
    int l = 0;
    while ((1ULL << l) < count) l++;
    *L = l;
    *eh = exponent_of(bits) - (62 - l);
}

/* the same lines: csrc/pdehip_fft.hip */
static double limbs_to_double(int64_t lh, int64_t lm, int64_t ll, int eh, int L)
{
    const int D = 63 - L, el = eh - 2 * D;
    const int64_t mask = (int64_t)((1ULL << D) - 1);
    lm += ll >> D; ll &= mask;
    lh += lm >> D; lm &= mask;
    if (lh < 0) return 0.0;
    uint64_t w[4] = {0, 0, 0, 0};
    const uint64_t digit[3] = {(uint64_t)ll, (uint64_t)lm, (uint64_t)lh};
    for (int q = 0; q < 3; q++) {
        const int at = q * D, word = at >> 6, bit = at & 63;
        w[word] |= digit[q] << bit;
        if (bit) w[word + 1] |= digit[q] >> (64 - bit);
    }
    int top = 2;
    while (top > 0 && !w[top]) top--;
    if (top == 0) return ldexp((double)w[0], el);
    const int msb = 63 - __builtin_clzll(w[top]);
    const int s = 64 * top + msb - 63;
    const int word = s >> 6, bit = s & 63;
    uint64_t win = w[word] >> bit;
    if (bit) win |= w[word + 1] << (64 - bit);
    int sticky = bit && (w[word] & ((1ULL << bit) - 1));
    for (int q = 0; q < word; q++) sticky = sticky || w[q];
    return ldexp((double)(win | (sticky ? 1ULL : 0ULL)), el + s);
}

int pdehip_shell_spectrum(const pdehip_grid_t *g, int ncomp, const void *arr_full, const double *kfreq, int nbins, const double *edges,
                          uint64_t *counts, double *sums, void *stream)
{
    (void)stream;
    rows_t r;
    int rc = check_extents(g, &r);
    if (rc) return rc;
    if (!arr_full || !kfreq || !edges || !counts || !sums) return shim_set_error(1, "shim: shell_spectrum: NULL pointer");
    if (ncomp < 1 || ncomp > 64) return shim_set_error(1, "shim: shell_spectrum: 1..64 components");
    if (nbins < 1 || nbins > 4096) return shim_set_error(1, "shim: shell_spectrum: 1..4096 bins");
    if (((uintptr_t)arr_full & 15) != 0 || (((uintptr_t)kfreq | (uintptr_t)edges | (uintptr_t)counts | (uintptr_t)sums) & 7) != 0)
        return shim_set_error(1, "shim: shell_spectrum: misaligned array");
    for (int i = 0; i <= nbins; i++) {
        if (!isfinite(edges[i])) return shim_set_error(1, "shim: shell_spectrum: an edge is not finite");
        if (i > 0 && !(edges[i] > edges[i - 1])) return shim_set_error(1, "shim: shell_spectrum: the edges must increase strictly");
    }
    const long n0 = r.n[0], n1 = r.n[1], n2 = r.n[2], nh = n2 / 2 + 1, total = n0 * n1 * nh;
    const int ns = nbins + 2;
    /* the frequencies of the normalised axes: a missing axis has the one frequency 0 */
    double *f[3];
    double zero = 0.0;
    long at = 0;
    for (int ax = 0; ax < 3; ax++) {
        if (ax >= 3 - r.ndim) { f[ax] = (double *)kfreq + at; at += r.n[ax]; }
        else f[ax] = &zero;
    }
    cplx_t *spec = (cplx_t *)malloc(sizeof(cplx_t) * (size_t)total);
    int *slot = (int *)malloc(sizeof(int) * (size_t)total);
    double *v = (double *)malloc(sizeof(double) * (size_t)total);
    uint64_t *mx = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)ns);
    int64_t *limb = (int64_t *)malloc(sizeof(int64_t) * 3 * (size_t)ns);
    if (!spec || !slot || !v || !mx || !limb) {
        free(spec); free(slot); free(v); free(mx); free(limb);
        return shim_set_error(3, "shim: shell_spectrum: out of memory");
    }
    memset(counts, 0, sizeof(uint64_t) * (size_t)ns);
    const size_t esize = r.f64 ? 8 : 4;
    for (int c = 0; c < ncomp && !rc; c++) {
        rc = forward_one(&r, (const char *)arr_full + (size_t)c * (size_t)r.pc * esize, spec);
        if (rc) break;
        memset(mx, 0, sizeof(uint64_t) * (size_t)ns);
        memset(limb, 0, sizeof(int64_t) * 3 * (size_t)ns);
        long t = 0;
        for (long i = 0; i < n0; i++)
            for (long j = 0; j < n1; j++)
                for (long k = 0; k < nh; k++, t++) {
                    const double f0 = f[0][i], f1 = f[1][j], f2 = f[2][k];
                    const double kk = sqrt((f0 * f0 + f1 * f1) + f2 * f2);
                    const int b = slot_of(edges, nbins, kk);
                    const unsigned w = (k > 0 && 2 * k < n2) ? 2u : 1u;
                    const double p = spec[t].re * spec[t].re + spec[t].im * spec[t].im;
                    v[t] = w == 2u ? 2.0 * p : p;
                    slot[t] = b;
                    uint64_t bits;
                    memcpy(&bits, &v[t], 8);
                    if (bits > mx[b]) mx[b] = bits;
                    if (c == 0) counts[b] += w;
                }
        for (t = 0; t < total; t++) {
            int eh, L;
            limb_params(mx[slot[t]], counts[slot[t]], &eh, &L);
            if (L < 0) continue;
            const int D = 63 - L, em = eh - D, el = em - D;
            const double fh = rint(ldexp(v[t], -eh));
            const double r1 = v[t] - ldexp(fh, eh);
            const double fm = rint(ldexp(r1, -em));
            const double r2 = r1 - ldexp(fm, em);
            const double fl = rint(ldexp(r2, -el));
            limb[3 * slot[t]] += (int64_t)fh; limb[3 * slot[t] + 1] += (int64_t)fm; limb[3 * slot[t] + 2] += (int64_t)fl;
        }
        for (int b = 0; b < ns; b++) {
            int eh, L;
            limb_params(mx[b], counts[b], &eh, &L);
            double *out = sums + (size_t)c * ns + b;
            if (L < 0) memcpy(out, &mx[b], 8);
            else *out = limbs_to_double(limb[3 * b], limb[3 * b + 1], limb[3 * b + 2], eh, L);
        }
    }
    free(spec); free(slot); free(v); free(mx); free(limb);
    return rc;
}
