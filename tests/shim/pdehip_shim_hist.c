/*
 * pdehip_shim_hist.c — HOST implementation of pdehip_histogram and pdehip_quantile_select (include/pdehip.h).  TESTS ONLY.
 *
 * An addition to the host shim (pdehip_shim.c, see the notice there): tests/hist_shimlib.py links this file with the shim's objects into
 * tests/shim/_build/libpdehip_shim_hist.so, so that the Python side of the distribution functions (pde_hip/distribution.py) runs through
 * the REAL py-pde without a GPU.  The product never builds or loads it.
 *
 * Plain serial C on the shim's compact layout (pdehip_layout): a binary search on the edges and a sort of the order-preserving keys - no
 * launch geometry, no LDS counters, no radix passes: the device kernels (csrc/pdehip_hist.hip) are tested on the GPU.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/pdehip.h"

int shim_set_error(int code, const char *msg);

typedef struct {
    long n[3], p[3];       /* normalised axes: cells and pitches */
    long pc, off;
    int f64;
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
    r->f64 = g->dtype == PDEHIP_F64;
    return 0;
}

/* the value of a cell in the field's type: the component itself, or sqrt(x_0 * x_0 + x_1 * x_1 + ...) */
static double cell_f64(const rows_t *r, const void *arr, long e, int ncomp, int norm)
{
    const double *a = (const double *)arr + e;
    if (!norm) return a[0];
    double s = a[0] * a[0];
    for (int c = 1; c < ncomp; c++) s = s + a[c * r->pc] * a[c * r->pc];
    return sqrt(s);
}
static float cell_f32(const rows_t *r, const void *arr, long e, int ncomp, int norm)
{
    const float *a = (const float *)arr + e;
    if (!norm) return a[0];
    float s = a[0] * a[0];
    for (int c = 1; c < ncomp; c++) s = s + a[c * r->pc] * a[c * r->pc];
    return sqrtf(s);
}

int pdehip_histogram(const pdehip_grid_t *g, int ncomp, const void *arr_full, int norm, int nbins, const double *edges, uint64_t *counts,
                     void *stream)
{
    (void)stream;
    rows_t r;
    int rc = make_rows(g, &r);
    if (rc) return rc;
    if (!arr_full || !edges || !counts) return shim_set_error(1, "shim: histogram: NULL pointer");
    if (ncomp < 1 || ncomp > 64) return shim_set_error(1, "shim: histogram: 1..64 components");
    if (nbins < 1 || nbins > 4096) return shim_set_error(1, "shim: histogram: 1..4096 bins");
    if (((uintptr_t)arr_full & 15) != 0 || (((uintptr_t)edges | (uintptr_t)counts) & 7) != 0) return shim_set_error(1, "shim: histogram: misaligned array");
    for (int i = 0; i <= nbins; i++) {
        if (!isfinite(edges[i])) return shim_set_error(1, "shim: histogram: an edge is not finite");
        if (i > 0 && !(edges[i] > edges[i - 1])) return shim_set_error(1, "shim: histogram: the edges must increase strictly");
    }
    const int blocks = norm ? 1 : ncomp;
    for (int b = 0; b < blocks; b++) {
        uint64_t *cnt = counts + (size_t)b * (nbins + 3);
        memset(cnt, 0, sizeof(uint64_t) * (nbins + 3));
        const long base = r.off + (norm ? 0 : (long)b * r.pc);
        for (long i = 0; i < r.n[0]; i++)
            for (long j = 0; j < r.n[1]; j++)
                for (long k = 0; k < r.n[2]; k++) {
                    const long e = base + i * r.p[0] + j * r.p[1] + k;
                    const double x = r.f64 ? cell_f64(&r, arr_full, e, ncomp, norm) : (double)cell_f32(&r, arr_full, e, ncomp, norm);
                    if (x != x) { cnt[nbins + 2]++; continue; }
                    if (x < edges[0]) { cnt[nbins]++; continue; }
                    if (x > edges[nbins]) { cnt[nbins + 1]++; continue; }
                    int lo = 0, hi = nbins - 1;      /* the largest bin whose lower edge is <= x */
                    while (lo < hi) {
                        const int mid = (lo + hi + 1) / 2;
                        if (edges[mid] <= x) lo = mid; else hi = mid - 1;
                    }
                    cnt[lo]++;
                }
    }
    return 0;
}

/* a < b as numbers <=> key(a) < key(b) as unsigned integers */
static uint64_t key_f64(double x)
{
    uint64_t u;
    memcpy(&u, &x, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}
static uint64_t key_f32(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    return (u >> 31) ? (uint32_t)~u : (u | 0x80000000u);
}
static int cmp_u64(const void *a, const void *b)
{
    const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b;
    return x < y ? -1 : (x > y ? 1 : 0);
}

int pdehip_quantile_select(const pdehip_grid_t *g, int ncomp, const void *arr_full, int norm, int nq, const double *q, void *lower,
                           void *upper, uint64_t *info, void *stream)
{
    (void)stream;
    rows_t r;
    int rc = make_rows(g, &r);
    if (rc) return rc;
    if (!arr_full || !q || !lower || !upper || !info) return shim_set_error(1, "shim: quantile_select: NULL pointer");
    if (ncomp < 1 || ncomp > 64) return shim_set_error(1, "shim: quantile_select: 1..64 components");
    if (nq < 1 || nq > 8) return shim_set_error(1, "shim: quantile_select: 1..8 quantiles");
    const uintptr_t esize = r.f64 ? 8 : 4;
    if (((uintptr_t)arr_full & 15) != 0 || (((uintptr_t)lower | (uintptr_t)upper) & (esize - 1)) != 0 || ((uintptr_t)info & 7) != 0)
        return shim_set_error(1, "shim: quantile_select: misaligned array");
    for (int j = 0; j < nq; j++)
        if (!(q[j] >= 0.0 && q[j] <= 1.0)) return shim_set_error(1, "shim: quantile_select: q is not in [0, 1]");
    const long cells = r.n[0] * r.n[1] * r.n[2];
    uint64_t *keys = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)cells);
    if (!keys) return shim_set_error(3, "shim: quantile_select: out of memory");
    const int blocks = norm ? 1 : ncomp;
    for (int b = 0; b < blocks; b++) {
        const long base = r.off + (norm ? 0 : (long)b * r.pc);
        uint64_t n = 0, n_nan = 0;
        for (long i = 0; i < r.n[0]; i++)
            for (long j = 0; j < r.n[1]; j++)
                for (long k = 0; k < r.n[2]; k++) {
                    const long e = base + i * r.p[0] + j * r.p[1] + k;
                    if (r.f64) {
                        const double x = cell_f64(&r, arr_full, e, ncomp, norm);
                        if (x != x) n_nan++; else keys[n++] = key_f64(x);
                    } else {
                        const float x = cell_f32(&r, arr_full, e, ncomp, norm);
                        if (x != x) n_nan++; else keys[n++] = key_f32(x);
                    }
                }
        qsort(keys, (size_t)n, sizeof(uint64_t), cmp_u64);
        info[2 * b] = n; info[2 * b + 1] = n_nan;
        for (int j = 0; j < nq; j++) {
            uint64_t bits[2];
            for (int side = 0; side < 2; side++) {
                if (n == 0) { bits[side] = r.f64 ? 0x7ff8000000000000ULL : 0x7fc00000ULL; continue; }
                uint64_t k = (uint64_t)floor((double)(n - 1) * q[j]);
                if (k > n - 1) k = n - 1;
                if (side && k < n - 1) k++;
                const uint64_t key = keys[k], sign = r.f64 ? 0x8000000000000000ULL : 0x80000000ULL;
                bits[side] = (key & sign) ? (key ^ sign) : (r.f64 ? ~key : (uint32_t)~key);
            }
            if (r.f64) {
                ((uint64_t *)lower)[(size_t)b * nq + j] = bits[0];
                ((uint64_t *)upper)[(size_t)b * nq + j] = bits[1];
            } else {
                ((uint32_t *)lower)[(size_t)b * nq + j] = (uint32_t)bits[0];
                ((uint32_t *)upper)[(size_t)b * nq + j] = (uint32_t)bits[1];
            }
        }
    }
    free(keys);
    return 0;
}
