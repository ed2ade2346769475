/*
 * pdehip_shim_props.c — HOST implementation of pdehip_domain_properties (include/pdehip.h).  TESTS ONLY.
 *
 * An addition to the host shim (pdehip_shim.c, see the notice there): tests/props_shimlib.py links this file with the shim's objects and
 * the other additions into tests/shim/_build/libpdehip_shim_props.so, so that the Python side of the domain properties
 * (pde_hip/domains.py) runs through the REAL py-pde without a GPU.  The product never builds or loads it.
 *
 * Plain sequential C on the shim's compact layout (pdehip_layout): one pass for the anchors, one for everything else - no waves, no
 * held labels, no atomics: the device kernels (csrc/pdehip_props.hip) are tested on the GPU.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/pdehip.h"

int shim_set_error(int code, const char *msg);

static int32_t frame_offset(int64_t i, int64_t ai, int64_t n, int periodic)
{
    int64_t d = i - ai;
    if (periodic) {
        const int64_t h = n / 2;
        d = ((d + h) % n + n) % n - h;
    }
    return (int32_t)d;
}

int pdehip_domain_properties(const pdehip_grid_t *g, const void *arr_full, const int32_t *labels, int64_t ndomains, const int *periodic,
                             double absmax, int32_t *anchor, int64_t *moment, int32_t *box, int64_t *limb, uint32_t *excluded, void *stream)
{
    (void)stream;
    int64_t lay[8];
    int rc = pdehip_layout(g, lay);
    if (rc) return rc;
    if (ndomains < 0 || ndomains > 2147483647LL) return shim_set_error(1, "shim: domain_properties: 0 ... 2^31 - 1 domains");
    if (!labels || !periodic) return shim_set_error(1, "shim: domain_properties: NULL pointer");
    if (ndomains > 0 && (!anchor || !moment || !box || (arr_full && (!limb || !excluded))))
        return shim_set_error(1, "shim: domain_properties: NULL pointer");
    if (!(absmax >= 0.0) || !(absmax < 0x1p1023)) return shim_set_error(1, "shim: domain_properties: absmax must be a number in [0, 2^1023)");
    int64_t n[3] = {1, 1, 1};
    int per[3] = {0, 0, 0};
    double cells_f = 1.0;
    for (int d = 0; d < g->ndim; d++) {
        n[3 - g->ndim + d] = (int64_t)g->shape[d];
        per[3 - g->ndim + d] = periodic[d] != 0;
        cells_f *= (double)g->shape[d];
    }
    if (cells_f > 2147483647.0) return shim_set_error(1, "shim: domain_properties: more than 2^31 - 1 cells");
    if (((uintptr_t)arr_full & 15) != 0 || ((uintptr_t)labels & 3) != 0 || ((uintptr_t)anchor & 3) != 0 || ((uintptr_t)moment & 7) != 0 ||
        ((uintptr_t)box & 3) != 0 || (arr_full && (((uintptr_t)limb & 7) != 0 || ((uintptr_t)excluded & 3) != 0)))
        return shim_set_error(1, "shim: domain_properties: misaligned array");
    const int64_t p0 = lay[0], p1 = lay[1], off = lay[3];
    const int64_t cells = n[0] * n[1] * n[2];
    int L = 0, E = 0;
    while ((1LL << L) < cells) L++;
    (void)frexp(absmax, &E);
    const int eh = E - (62 - L), el = eh - 31;
    for (int64_t k = 0; k < ndomains; k++) {
        anchor[k] = INT32_MAX;
        for (int a = 0; a < 3; a++) { moment[3 * k + a] = 0; box[6 * k + 2 * a] = INT32_MAX; box[6 * k + 2 * a + 1] = INT32_MIN; }
        if (arr_full) { limb[2 * k] = 0; limb[2 * k + 1] = 0; excluded[k] = 0; }
    }
    uint64_t bad = 0;
    for (int64_t c = 0; c < cells; c++) {
        const int32_t v = labels[c];
        if (v < 0 || (int64_t)v > ndomains) bad++;
        else if (v > 0 && anchor[v - 1] == INT32_MAX) anchor[v - 1] = (int32_t)c;          /* (ascending: the first is the smallest) */
    }
    for (int64_t c = 0; c < cells; c++) {
        const int32_t v = labels[c];
        if (v <= 0 || (int64_t)v > ndomains) continue;
        const int64_t k = v - 1, at = anchor[k];
        const int64_t idx[3] = {c / (n[1] * n[2]), (c / n[2]) % n[1], c % n[2]};
        const int64_t aidx[3] = {at / (n[1] * n[2]), (at / n[2]) % n[1], at % n[2]};
        for (int a = 0; a < 3; a++) {
            const int32_t d = frame_offset(idx[a], aidx[a], n[a], per[a]);
            moment[3 * k + a] += d;
            if (d < box[6 * k + 2 * a]) box[6 * k + 2 * a] = d;
            if (d > box[6 * k + 2 * a + 1]) box[6 * k + 2 * a + 1] = d;
        }
        if (!arr_full) continue;
        const int64_t e = off + idx[0] * p0 + idx[1] * p1 + idx[2];
        const double x = g->dtype == PDEHIP_F64 ? ((const double *)arr_full)[e] : (double)((const float *)arr_full)[e];
        if (!(fabs(x) <= absmax)) { excluded[k]++; continue; }
        const double hi = rint(ldexp(x, -eh));
        const double r = x - ldexp(hi, eh);
        limb[2 * k] += (int64_t)hi;
        limb[2 * k + 1] += (int64_t)rint(ldexp(r, -el));
    }
    if (bad) return shim_set_error(1, "shim: domain_properties: cells with a label outside 0 ... ndomains");
    return 0;
}
