/*
 * pdehip_shim_interp.c — HOST implementation of the interpolation entry points of include/pdehip.h.  TESTS ONLY.
 *
 * An addition to the host shim (pdehip_shim.c, see the notice there): tests/interp_shimlib.py links this file with the shim's objects into
 * a second library, tests/shim/_build/libpdehip_shim_interp.so, so that the Python side of interpolation (pde_hip/interpolation.py, the
 * plugin class, the error classes, the result classes) runs through the REAL py-pde without a GPU.  The product never builds or loads it.
 *
 * Plain serial C of pde/backends/numba/grids.py:102-347 and pde/grids/boundaries/axes.py:475-495 on the shim's compact layout
 * (pdehip_layout): no tables, no launch geometry - the device kernels (csrc/pdehip_interp.hip) are tested on the GPU.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/pdehip.h"

int shim_set_error(int code, const char *msg);

typedef struct {
    long size, pitch;
    double lo, dx;
    int periodic;
} axis_t;

typedef struct {
    long cl, ch;
    double wl, wh;
} support_t;

/* grids.py:136-188; returns 0 where the coordinate is out of bounds.  Indices are VALID indices (-1 / size: the ghost cells). */
static int axis_data(double coord, const axis_t *x, int ghost, support_t *r)
{
    /* c_l, d_l = divmod(v, 1.0) by CPython's rule (floatobject.c float_divmod) */
    const double vx = (coord - x->lo) / x->dx - 0.5;
    double mod = fmod(vx, 1.0), div = (vx - mod) / 1.0, c_l;
    if (mod != 0.0) {
        if (mod < 0.0) { mod += 1.0; div -= 1.0; }
    } else {
        mod = 0.0;
    }
    if (div != 0.0) {
        c_l = floor(div);
        if (div - c_l > 0.5) c_l += 1.0;
    } else {
        c_l = copysign(0.0, vx / 1.0);
    }
    const double d_l = mod, q = c_l + d_l, size = (double)x->size;
    if (x->periodic) {
        if (!isfinite(c_l)) return 0;
        double m = fmod(c_l, size);
        if (m < 0.0) m += size;
        r->cl = (long)m;
        r->ch = (r->cl + 1) % x->size;
    } else if (ghost) {
        if (!(-0.5 <= q && q <= size - 0.5)) return 0;
        r->cl = (long)c_l;
        r->ch = r->cl + 1;
    } else {
        if (0.0 <= q && q < size - 1.0) { r->cl = (long)c_l; r->ch = r->cl + 1; }
        else if (size - 1.0 <= q && q <= size - 0.5) r->cl = r->ch = (long)c_l;
        else if (-0.5 <= q && q <= 0.0) r->cl = r->ch = (long)c_l + 1;
        else return 0;
        if (r->cl < 0) r->cl += x->size;
        if (r->ch < 0) r->ch += x->size;
    }
    r->wl = 1.0 - d_l;
    r->wh = d_l;
    if (r->wl < 1e-15) r->wl = 0.0;
    if (r->wh < 1e-15) r->wh = 0.0;
    return 1;
}

typedef struct {
    axis_t ax[3];
    int ndim, f64, ghost;
    long pc, off;
} source_t;

static int make_source(const pdehip_grid_t *g, const int *periodic, const double *lo, int ghost, source_t *s)
{
    int64_t lay[8];
    int rc = pdehip_layout(g, lay);
    if (rc) return rc;
    if (!periodic || !lo) return shim_set_error(1, "shim: interpolate: NULL pointer");
    const long p3[3] = {(long)lay[0], (long)lay[1], 1};
    s->ndim = g->ndim; s->f64 = g->dtype == PDEHIP_F64; s->ghost = ghost ? 1 : 0;
    s->pc = (long)lay[2]; s->off = (long)lay[3];
    for (int d = 0; d < g->ndim; d++) {
        s->ax[d].size = (long)g->shape[d];
        s->ax[d].pitch = p3[3 - g->ndim + d];
        s->ax[d].lo = lo[d];
        s->ax[d].dx = g->dx[d];
        s->ax[d].periodic = periodic[d] ? 1 : 0;
    }
    return 0;
}

static double load(const source_t *s, const void *data, long i) { return s->f64 ? ((const double *)data)[i] : (double)((const float *)data)[i]; }
static void store(int f64, void *data, long i, double v) { if (f64) ((double *)data)[i] = v; else ((float *)data)[i] = (float)v; }

/* the 2 / 4 / 8 term sum of grids.py:259, :293-298, :334-343: terms in the order x (slowest) .. z, lower before upper, weights
 * multiplied and terms added left to right */
static double value_at(const source_t *s, const void *data, long comp, const support_t *sup)
{
    double sum = 0.0;
    for (int t = 0; t < (1 << s->ndim); t++) {
        long idx = s->off + comp * s->pc;
        double w = 0.0;
        for (int d = 0; d < s->ndim; d++) {
            const int hi = (t >> (s->ndim - 1 - d)) & 1;
            idx += (hi ? sup[d].ch : sup[d].cl) * s->ax[d].pitch;
            w = d == 0 ? (hi ? sup[d].wh : sup[d].wl) : w * (hi ? sup[d].wh : sup[d].wl);
        }
        const double term = w * load(s, data, idx);
        sum = t == 0 ? term : sum + term;
    }
    return sum;
}

int pdehip_interpolate_points(const pdehip_grid_t *g, int ncomp, const int *periodic, const double *lo, int with_ghost_cells,
                              const void *data_full, const double *points, int64_t npoints, const double *fill, void *out,
                              void *oob_count, void *stream)
{
    (void)stream;
    source_t s;
    int rc = make_source(g, periodic, lo, with_ghost_cells, &s);
    if (rc) return rc;
    for (int64_t p = 0; p < npoints; p++) {
        support_t sup[3];
        int ok = 1;
        for (int d = 0; d < s.ndim; d++) ok &= axis_data(points[p * s.ndim + d], &s.ax[d], s.ghost, &sup[d]);
        for (int c = 0; c < ncomp && (ok || fill); c++) store(s.f64, out, c * npoints + p, ok ? value_at(&s, data_full, c, sup) : fill[c]);
        if (!ok && !fill) ++*(uint64_t *)oob_count;
    }
    return 0;
}

int pdehip_interpolate_to_grid(const pdehip_grid_t *src, int ncomp, const int *periodic, const double *src_lo, int with_ghost_cells,
                               const void *src_full, const pdehip_grid_t *dst, const double *dst_coords, const double *fill,
                               void *dst_full, void *tables, void *oob_count, void *stream)
{
    (void)stream; (void)tables;
    source_t s;
    int64_t lay[8];
    int rc = make_source(src, periodic, src_lo, with_ghost_cells, &s);
    if (!rc) rc = pdehip_layout(dst, lay);
    if (rc) return rc;
    if (src->ndim != dst->ndim || src->dtype != dst->dtype) return shim_set_error(1, "shim: interpolate_to_grid: the grids differ");
    const long p3[3] = {(long)lay[0], (long)lay[1], 1};
    long n[3] = {1, 1, 1}, dp[3] = {0, 0, 0}, start[3] = {0, 0, 0}, total = 1, at = 0;
    for (int d = 0; d < s.ndim; d++) { n[d] = (long)dst->shape[d]; dp[d] = p3[3 - s.ndim + d]; start[d] = at; at += n[d]; total *= n[d]; }
    for (long cell = 0; cell < total; cell++) {
        long i[3], rest = cell, o = (long)lay[3];
        for (int d = s.ndim - 1; d >= 0; d--) { i[d] = rest % n[d]; rest /= n[d]; o += i[d] * dp[d]; }
        support_t sup[3];
        int ok = 1;
        for (int d = 0; d < s.ndim; d++) ok &= axis_data(dst_coords[start[d] + i[d]], &s.ax[d], s.ghost, &sup[d]);
        for (int c = 0; c < ncomp && (ok || fill); c++) store(s.f64, dst_full, o + c * (long)lay[2], ok ? value_at(&s, src_full, c, sup) : fill[c]);
        if (!ok && !fill) ++*(uint64_t *)oob_count;
    }
    return 0;
}

/* axes.py:475-495 in the field's own type: d[i, j] = (d[nxt[i], j] + d[i, nxt[j]]) / 2 on the corners of a 2-D grid and along the edges
 * of a 3-D grid, then d[i, j, k] = (d[nxt[i], j, k] + d[i, nxt[j], k] + d[i, j, nxt[k]]) / 3 on its corners */
#define CORNERS(T)                                                                                                               \
    static void corners_##T(T *d, int nd, const long *n, const long *p)                                                         \
    {                                                                                                                            \
        for (int u = 0; u < nd; u++)                                                                                             \
            for (int v = u + 1; v < nd; v++) {                                                                                   \
                const int w = 3 - u - v; /* the axis along the edge (3-D only) */                                                \
                const long len = nd == 3 ? n[w] : 1, pw = nd == 3 ? p[w] : 0;                                                    \
                for (int corner = 0; corner < 4; corner++)                                                                       \
                    for (long s = 1; s <= len; s++) {                                                                            \
                        const long gi = (corner & 2) ? n[u] + 1 : 0, gj = (corner & 1) ? n[v] + 1 : 0;                           \
                        const long ni = (corner & 2) ? n[u] : 1, nj = (corner & 1) ? n[v] : 1;                                   \
                        const long e = nd == 3 ? s * pw : 0;                                                                     \
                        d[e + gi * p[u] + gj * p[v]] = (d[e + ni * p[u] + gj * p[v]] + d[e + gi * p[u] + nj * p[v]]) / (T)2;     \
                    }                                                                                                            \
            }                                                                                                                    \
        if (nd < 3) return;                                                                                                      \
        for (int corner = 0; corner < 8; corner++) {                                                                             \
            const long gi = (corner & 4) ? n[0] + 1 : 0, gj = (corner & 2) ? n[1] + 1 : 0, gk = (corner & 1) ? n[2] + 1 : 0;     \
            const long ni = (corner & 4) ? n[0] : 1, nj = (corner & 2) ? n[1] : 1, nk = (corner & 1) ? n[2] : 1;                 \
            d[gi * p[0] + gj * p[1] + gk * p[2]] =                                                                               \
                (d[ni * p[0] + gj * p[1] + gk * p[2]] + d[gi * p[0] + nj * p[1] + gk * p[2]] + d[gi * p[0] + gj * p[1] + nk * p[2]]) / (T)3; \
        }                                                                                                                        \
    }
CORNERS(double)
CORNERS(float)

int pdehip_set_ghost_corners(const pdehip_grid_t *g, int ncomp, void *data_full, void *stream)
{
    (void)stream;
    int64_t lay[8];
    int rc = pdehip_layout(g, lay);
    if (rc) return rc;
    if (g->ndim < 2) return 0;
    const long p3[3] = {(long)lay[0], (long)lay[1], 1};
    long n[3], p[3], base = (long)lay[3];
    for (int d = 0; d < g->ndim; d++) { n[d] = (long)g->shape[d]; p[d] = p3[3 - g->ndim + d]; base -= p[d]; }
    for (int c = 0; c < ncomp; c++) {
        if (g->dtype == PDEHIP_F64) corners_double((double *)data_full + base + c * (long)lay[2], g->ndim, n, p);
        else corners_float((float *)data_full + base + c * (long)lay[2], g->ndim, n, p);
    }
    return 0;
}
