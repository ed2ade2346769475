/*
 * pdehip_shim_project.c — HOST implementation of pdehip_project and pdehip_extract_box (include/pdehip.h).  TESTS ONLY.
 *
 * An addition to the host shim (pdehip_shim.c, see the notice there): tests/project_shimlib.py links this file with the shim's objects
 * into tests/shim/_build/libpdehip_shim_project.so, so that the Python side of the device projections (pde_hip/projection.py, the
 * resident-field methods under `device_projections`) runs through the REAL py-pde without a GPU.  The product never builds or loads it.
 *
 * Plain serial C on the shim's compact layout (pdehip_layout): no launch geometry, no stages - the device kernels
 * (csrc/pdehip_project.hip) are tested on the GPU.  Compiled with -ffp-contract=off like the rest of the shim: one rounding per operation.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/pdehip.h"

int shim_set_error(int code, const char *msg);

typedef struct {
    long n[3], p[3];       /* normalised axes: cells and pitches */
    long pc, off;
    int f64, ndim;
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
    r->ndim = g->ndim;
    return 0;
}

static double cell(const rows_t *r, const void *arr, long e) { return r->f64 ? ((const double *)arr)[e] : (double)((const float *)arr)[e]; }

int pdehip_project(const pdehip_grid_t *g, int ncomp, const void *arr_full, int axes_mask, int method, double weight, void *out, void *stream)
{
    (void)stream;
    rows_t r;
    int rc = make_rows(g, &r);
    if (rc) return rc;
    if (!arr_full || !out) return shim_set_error(1, "shim: project: NULL pointer");
    if (ncomp < 1 || ncomp > 64) return shim_set_error(1, "shim: project: 1..64 components");
    if (axes_mask <= 0 || axes_mask >= (1 << r.ndim)) return shim_set_error(1, "shim: project: empty or foreign mask");
    if (method < PDEHIP_PROJECT_SUM || method > PDEHIP_PROJECT_MIN) return shim_set_error(1, "shim: project: unknown method");
    if (((uintptr_t)arr_full & 15) != 0 || ((uintptr_t)out & 7) != 0) return shim_set_error(1, "shim: project: misaligned array");
    int removed[3] = {0, 0, 0};
    for (int d = 0; d < r.ndim; d++) removed[3 - r.ndim + d] = (axes_mask >> d) & 1;
    long keep[3], drop[3];     /* extents of the loops over the output cells and over the removed cells */
    for (int ax = 0; ax < 3; ax++) { keep[ax] = removed[ax] ? 1 : r.n[ax]; drop[ax] = removed[ax] ? r.n[ax] : 1; }
    long at = 0;
    for (int c = 0; c < ncomp; c++)
        for (long i = 0; i < keep[0]; i++)
            for (long j = 0; j < keep[1]; j++)
                for (long k = 0; k < keep[2]; k++) {
                    double acc = method == PDEHIP_PROJECT_SUM ? 0.0 : (method == PDEHIP_PROJECT_MAX ? -INFINITY : INFINITY);
                    for (long a = 0; a < drop[0]; a++)
                        for (long b = 0; b < drop[1]; b++)
                            for (long d = 0; d < drop[2]; d++) {
                                const double x = cell(&r, arr_full, r.off + c * r.pc + (i + a) * r.p[0] + (j + b) * r.p[1] + k + d);
                                if (method == PDEHIP_PROJECT_SUM) acc = acc + x * weight;
                                else if (x != x || (method == PDEHIP_PROJECT_MAX ? x > acc : x < acc)) acc = x;
                                /* (a NaN stays: no number compares above or below it) */
                            }
                    if (method != PDEHIP_PROJECT_SUM && !r.f64) ((float *)out)[at++] = (float)acc;
                    else ((double *)out)[at++] = acc;
                }
    return 0;
}

int pdehip_extract_box(const pdehip_grid_t *g, int ncomp, const void *arr_full, const long *lo, const long *extent, void *out, void *stream)
{
    (void)stream;
    rows_t r;
    int rc = make_rows(g, &r);
    if (rc) return rc;
    if (!arr_full || !out || !lo || !extent) return shim_set_error(1, "shim: extract_box: NULL pointer");
    if (ncomp < 1 || ncomp > 64) return shim_set_error(1, "shim: extract_box: 1..64 components");
    if (((uintptr_t)arr_full & 15) != 0 || ((uintptr_t)out & (r.f64 ? 7 : 3)) != 0) return shim_set_error(1, "shim: extract_box: misaligned array");
    long l[3] = {0, 0, 0}, n[3] = {1, 1, 1};
    for (int d = 0; d < r.ndim; d++) {
        const int ax = 3 - r.ndim + d;
        if (lo[d] < 0 || extent[d] < 1 || lo[d] > r.n[ax] - extent[d]) return shim_set_error(1, "shim: extract_box: the box is not inside the grid");
        l[ax] = lo[d]; n[ax] = extent[d];
    }
    long at = 0;
    for (int c = 0; c < ncomp; c++)
        for (long i = 0; i < n[0]; i++)
            for (long j = 0; j < n[1]; j++)
                for (long k = 0; k < n[2]; k++, at++) {
                    const long e = r.off + c * r.pc + (l[0] + i) * r.p[0] + (l[1] + j) * r.p[1] + l[2] + k;
                    if (r.f64) ((double *)out)[at] = ((const double *)arr_full)[e];
                    else ((float *)out)[at] = ((const float *)arr_full)[e];
                }
    return 0;
}
