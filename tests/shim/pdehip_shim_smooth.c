/*
 * pdehip_shim_smooth.c — HOST implementation of pdehip_smooth_axis (include/pdehip.h).  TESTS ONLY.
 *
 * An addition to the host shim (pdehip_shim.c, see the notice there): tests/smooth_shimlib.py links this file with the shim's objects, the
 * statistics and the projection sources into tests/shim/_build/libpdehip_shim_smooth.so, so that the Python side of the device smoothing
 * (pde_hip/smoothing.py, the resident-field method under `device_smoothing`) runs through the REAL py-pde without a GPU.  The product
 * never builds or loads it.
 *
 * Plain serial C on the shim's compact layout (pdehip_layout): no tiles, no instances - the device kernels (csrc/pdehip_smooth.hip) are
 * tested on the GPU.  Compiled with -ffp-contract=off like the rest of the shim: one rounding per operation.
 */
#include <stddef.h>
#include <stdint.h>

#include "../../include/pdehip.h"

int shim_set_error(int code, const char *msg);

static long resolve(long p, long n, int wrap)
{
    if (wrap) {
        long q = p % n;
        return q < 0 ? q + n : q;
    }
    long q = p % (2 * n);
    if (q < 0) q += 2 * n;
    return q < n ? q : 2 * n - 1 - q;
}

int pdehip_smooth_axis(const pdehip_grid_t *g, int ncomp, const void *in_full, void *out_full, int axis, int mode, int radius,
                       const double *weights, void *stream)
{
    (void)stream;
    int64_t lay[8];
    int rc = pdehip_layout(g, lay);
    if (rc) return rc;
    if (!in_full || !out_full || !weights) return shim_set_error(1, "shim: smooth_axis: NULL pointer");
    if (ncomp < 1 || ncomp > 64) return shim_set_error(1, "shim: smooth_axis: 1..64 components");
    if (axis < 0 || axis >= g->ndim) return shim_set_error(1, "shim: smooth_axis: the grid has no such axis");
    const int m = mode & ~PDEHIP_SMOOTH_CELL;
    if (m != PDEHIP_SMOOTH_WRAP && m != PDEHIP_SMOOTH_REFLECT) return shim_set_error(1, "shim: smooth_axis: unknown mode");
    if (radius < 0) return shim_set_error(1, "shim: smooth_axis: negative radius");
    const int f64 = g->dtype == PDEHIP_F64;
    const long pc = (long)lay[2], off = (long)lay[3];
    const uintptr_t bytes = (uintptr_t)ncomp * (uintptr_t)pc * (f64 ? 8 : 4);
    const uintptr_t a = (uintptr_t)in_full, b = (uintptr_t)out_full;
    if (a < b + bytes && b < a + bytes) return shim_set_error(1, "shim: smooth_axis: the input and the output overlap");
    if (((a | b) & 15) != 0) return shim_set_error(1, "shim: smooth_axis: misaligned array");
    long n[3] = {1, 1, 1}, p[3] = {(long)lay[0], (long)lay[1], 1};
    for (int d = 0; d < g->ndim; d++) n[3 - g->ndim + d] = (long)g->shape[d];
    const int ax = 3 - g->ndim + axis;
    const int wrap = m == PDEHIP_SMOOTH_WRAP;
    for (int c = 0; c < ncomp; c++)
        for (long i = 0; i < n[0]; i++)
            for (long j = 0; j < n[1]; j++)
                for (long k = 0; k < n[2]; k++) {
                    const long e = off + c * pc + i * p[0] + j * p[1] + k;
                    const long at = ax == 0 ? i : (ax == 1 ? j : k);
                    const long line = e - at * p[ax];
#define CELL(q) (f64 ? ((const double *)in_full)[line + (q) * p[ax]] : (double)((const float *)in_full)[line + (q) * p[ax]])
                    double t = CELL(at) * weights[0];
                    for (int w = radius; w >= 1; w--) t = t + (CELL(resolve(at - w, n[ax], wrap)) + CELL(resolve(at + w, n[ax], wrap))) * weights[w];
#undef CELL
                    if (f64) ((double *)out_full)[e] = t;
                    else ((float *)out_full)[e] = (float)t;
                }
    return 0;
}
