/*
 * pdehip_shim_stats.c — HOST implementation of pdehip_field_stats and pdehip_steady_state (include/pdehip.h).  TESTS ONLY.
 *
 * An addition to the host shim (pdehip_shim.c, see the notice there): tests/stats_shimlib.py links this file with the shim's objects into
 * tests/shim/_build/libpdehip_shim_stats.so, so that the Python side of the device statistics (pde_hip/statistics.py, the trackers of the
 * plugin) runs through the REAL py-pde without a GPU.  The product never builds or loads it.
 *
 * Plain serial C on the shim's compact layout (pdehip_layout): no launch geometry, no slots - the device kernels
 * (csrc/pdehip_stats.hip) are tested on the GPU.  Compiled with -ffp-contract=off like the rest of the shim: one rounding per operation.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

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

/* the value of a cell: the component itself, or sqrt(x_0 * x_0 + x_1 * x_1 + ...) in the field's type */
static double cell_value(const rows_t *r, const void *arr, long e, int ncomp, int norm)
{
    if (r->f64) {
        const double *a = (const double *)arr + e;
        if (!norm) return a[0];
        double s = a[0] * a[0];
        for (int c = 1; c < ncomp; c++) s = s + a[c * r->pc] * a[c * r->pc];
        return sqrt(s);
    }
    const float *a = (const float *)arr + e;
    if (!norm) return (double)a[0];
    float s = a[0] * a[0];
    for (int c = 1; c < ncomp; c++) s = s + a[c * r->pc] * a[c * r->pc];
    return (double)sqrtf(s);
}

int pdehip_field_stats(const pdehip_grid_t *g, int ncomp, const void *arr_full, int norm, int want_m2, double *out, void *stream)
{
    (void)stream;
    rows_t r;
    int rc = make_rows(g, &r);
    if (rc) return rc;
    if (!arr_full || !out) return shim_set_error(1, "shim: field_stats: NULL pointer");
    if (ncomp < 1 || ncomp > 64) return shim_set_error(1, "shim: field_stats: 1..64 components");
    const int blocks = norm ? 1 : ncomp;
    for (int b = 0; b < blocks; b++) {
        const long base = r.off + (long)b * r.pc;
        double cnt = 0, bad = 0, sum = 0, mn = INFINITY, mx = -INFINITY, m2 = 0;
        for (int pass = 0; pass < (want_m2 ? 2 : 1); pass++) {
            const double mean = cnt > 0 ? sum / cnt : NAN;
            for (long i = 0; i < r.n[0]; i++)
                for (long j = 0; j < r.n[1]; j++)
                    for (long k = 0; k < r.n[2]; k++) {
                        const double x = cell_value(&r, arr_full, base + i * r.p[0] + j * r.p[1] + k, norm ? ncomp : 1, norm);
                        if (pass == 0) {
                            if (isfinite(x)) { cnt += 1; sum = sum + x; if (x < mn) mn = x; if (x > mx) mx = x; }
                            else bad += 1;
                        } else if (isfinite(x)) {
                            const double d = x - mean;
                            m2 = m2 + d * d;
                        }
                    }
        }
        double *o = out + 8 * b;
        o[0] = cnt; o[1] = bad; o[2] = sum;
        o[3] = cnt > 0 ? mn : NAN; o[4] = cnt > 0 ? mx : NAN; o[5] = cnt > 0 ? sum / cnt : NAN;
        o[6] = (want_m2 && cnt > 0) ? m2 : NAN;
        o[7] = 0;
    }
    return 0;
}

#define STEADY(T, ABS)                                                                                                            \
    static void steady_##T(const rows_t *r, int ncomp, const T *cur, T *last, T elapsed, T rtol, double *out)                     \
    {                                                                                                                             \
        double cnt = 0, mx = -INFINITY;                                                                                           \
        int nan = 0;                                                                                                              \
        for (int c = 0; c < ncomp; c++)                                                                                           \
            for (long i = 0; i < r->n[0]; i++)                                                                                    \
                for (long j = 0; j < r->n[1]; j++)                                                                                \
                    for (long k = 0; k < r->n[2]; k++) {                                                                          \
                        const long e = r->off + c * r->pc + i * r->p[0] + j * r->p[1] + k;                                        \
                        const T x = cur[e], l = last[e];                                                                          \
                        last[e] = x;                                                                                              \
                        if (!isfinite(x)) continue;                                                                               \
                        const T rate = (l - x) / elapsed;                                                                         \
                        const double v = (double)(ABS(rate) - rtol * ABS(x));                                                     \
                        cnt += 1;                                                                                                 \
                        if (v != v) nan = 1; else if (v > mx) mx = v;                                                             \
                    }                                                                                                             \
        out[0] = (nan || !(cnt > 0)) ? NAN : mx;                                                                                  \
        out[1] = cnt;                                                                                                             \
    }
STEADY(double, fabs)
STEADY(float, fabsf)

int pdehip_steady_state(const pdehip_grid_t *g, int ncomp, const void *cur_full, void *last_full, double elapsed, double rtol, double *out,
                        void *stream)
{
    (void)stream;
    rows_t r;
    int rc = make_rows(g, &r);
    if (rc) return rc;
    if (!cur_full || !last_full || !out) return shim_set_error(1, "shim: steady_state: NULL pointer");
    if (cur_full == last_full) return shim_set_error(1, "shim: steady_state: the snapshot must not be the state itself");
    if (ncomp < 1) return shim_set_error(1, "shim: steady_state: ncomp must be >= 1");
    if (r.f64) steady_double(&r, ncomp, (const double *)cur_full, (double *)last_full, elapsed, rtol, out);
    else steady_float(&r, ncomp, (const float *)cur_full, (float *)last_full, (float)elapsed, (float)rtol, out);
    return 0;
}
