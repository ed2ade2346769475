/*
 * pdehip_shim_label.c — HOST implementation of pdehip_label_domains and pdehip_domain_sizes (include/pdehip.h).  TESTS ONLY.
 *
 * An addition to the host shim (pdehip_shim.c, see the notice there): tests/label_shimlib.py links this file with the shim's objects into
 * tests/shim/_build/libpdehip_shim_label.so, so that the Python side of the domain functions (pde_hip/domains.py) runs through the REAL
 * py-pde without a GPU.  The product never builds or loads it.
 *
 * Plain sequential C on the shim's compact layout (pdehip_layout): one union-find over all cells with the smaller index as the root, then
 * one pass in C order that numbers the roots - no tiles, no seams, no atomics: the device kernels (csrc/pdehip_label.hip) are tested on
 * the GPU.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/pdehip.h"

int shim_set_error(int code, const char *msg);

static int32_t find_root(int32_t *parent, int32_t x)
{
    while (parent[x] != x) {
        parent[x] = parent[parent[x]];
        x = parent[x];
    }
    return x;
}

int pdehip_label_domains(const pdehip_grid_t *g, const void *arr_full, double lo, double hi, int connectivity, const int *periodic,
                         int32_t *labels, uint64_t *info, void *stream)
{
    (void)stream;
    int64_t lay[8];
    int rc = pdehip_layout(g, lay);
    if (rc) return rc;
    if (!arr_full || !periodic || !labels || !info) return shim_set_error(1, "shim: label_domains: NULL pointer");
    if (lo != lo || hi != hi || lo > hi) return shim_set_error(1, "shim: label_domains: the bounds must be numbers with lo <= hi");
    if (connectivity != 1 && connectivity != g->ndim) return shim_set_error(1, "shim: label_domains: connectivity 1 or ndim");
    long n[3] = {1, 1, 1};
    int per[3] = {0, 0, 0};
    double cells_f = 1.0;
    for (int d = 0; d < g->ndim; d++) {
        n[3 - g->ndim + d] = (long)g->shape[d];
        per[3 - g->ndim + d] = periodic[d] != 0;
        cells_f *= (double)g->shape[d];
    }
    if (cells_f > 2147483647.0) return shim_set_error(1, "shim: label_domains: more than 2^31 - 1 cells");
    if (((uintptr_t)arr_full & 15) != 0 || ((uintptr_t)labels & 3) != 0 || ((uintptr_t)info & 7) != 0)
        return shim_set_error(1, "shim: label_domains: misaligned array");
    const long p0 = (long)lay[0], p1 = (long)lay[1], off = (long)lay[3];
    const long cells = n[0] * n[1] * n[2];
    int32_t *parent = (int32_t *)malloc(sizeof(int32_t) * (size_t)cells);
    if (!parent) return shim_set_error(3, "shim: label_domains: out of memory");
    uint64_t fg = 0;
    for (long i = 0; i < n[0]; i++)
        for (long j = 0; j < n[1]; j++)
            for (long k = 0; k < n[2]; k++) {
                const long e = off + i * p0 + j * p1 + k, c = (i * n[1] + j) * n[2] + k;
                const double x = g->dtype == PDEHIP_F64 ? ((const double *)arr_full)[e] : (double)((const float *)arr_full)[e];
                const int in = lo <= x && x <= hi;
                parent[c] = in ? (int32_t)c : -1;
                fg += (uint64_t)in;
            }
    const int full = connectivity != 1;
    for (long i = 0; i < n[0]; i++)
        for (long j = 0; j < n[1]; j++)
            for (long k = 0; k < n[2]; k++) {
                const long c = (i * n[1] + j) * n[2] + k;
                if (parent[c] < 0) continue;
                for (int d0 = -1; d0 <= 1; d0++)
                    for (int d1 = -1; d1 <= 1; d1++)
                        for (int d2 = -1; d2 <= 1; d2++) {
                            const int steps = (d0 != 0) + (d1 != 0) + (d2 != 0);
                            if (steps == 0 || (!full && steps > 1)) continue;
                            long q[3] = {i + d0, j + d1, k + d2};
                            int inside = 1;
                            for (int a = 0; a < 3; a++) {
                                if (q[a] >= 0 && q[a] < n[a]) continue;
                                if (!per[a]) { inside = 0; break; }
                                q[a] = q[a] < 0 ? n[a] - 1 : 0;
                            }
                            if (!inside) continue;
                            const long nb = (q[0] * n[1] + q[1]) * n[2] + q[2];
                            if (parent[nb] < 0) continue;
                            const int32_t ra = find_root(parent, (int32_t)c), rb = find_root(parent, (int32_t)nb);
                            if (ra < rb) parent[rb] = ra; else if (rb < ra) parent[ra] = rb;
                        }
            }
    /* a root is the first cell of its domain in C order and the root of a cell never lies behind it: one pass numbers everything */
    int32_t count = 0;
    for (long c = 0; c < cells; c++) {
        if (parent[c] < 0) { labels[c] = 0; continue; }
        const int32_t r = find_root(parent, (int32_t)c);
        labels[c] = r == (int32_t)c ? ++count : labels[r];
    }
    free(parent);
    info[0] = (uint64_t)count;
    info[1] = fg;
    return 0;
}

int pdehip_domain_sizes(const int32_t *labels, int64_t ncells, int64_t ndomains, uint64_t *sizes, void *stream)
{
    (void)stream;
    if (!labels || (!sizes && ndomains > 0)) return shim_set_error(1, "shim: domain_sizes: NULL pointer");
    if (ncells < 1 || ndomains < 0 || ndomains > 2147483647LL) return shim_set_error(1, "shim: domain_sizes: bad counts");
    if (((uintptr_t)labels & 3) != 0 || ((uintptr_t)sizes & 7) != 0) return shim_set_error(1, "shim: domain_sizes: misaligned array");
    if (ndomains > 0) memset(sizes, 0, sizeof(uint64_t) * (size_t)ndomains);
    uint64_t bad = 0;
    for (int64_t c = 0; c < ncells; c++) {
        const int32_t v = labels[c];
        if (v < 0 || (int64_t)v > ndomains) bad++;
        else if (v > 0) sizes[v - 1]++;
    }
    if (bad) return shim_set_error(1, "shim: domain_sizes: cells with a label outside 0 ... ndomains");
    return 0;
}
