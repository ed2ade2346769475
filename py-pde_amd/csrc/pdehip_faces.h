// pdehip_faces.h - which faces of a BC table the stencil kernels evaluate on the fly, and their conversion to the kernels' table.
// Plain host C++ without a HIP header: the library includes it through pdehip_common.h, a CPU test asks the same functions
// (tests/test_faces_cpu.py through tests/shim/faces_probe.cpp).
#pragma once

#include <cstring>

#include "../../include/pdehip.h"

namespace pdehip {

// input-side BCs the stencil kernel evaluates on the fly (scalar first-order conditions)
struct InputBCs {
    int on[3][2];      // [normalised axis][lower, upper]
    long idx[3][2];
    double c[3][2], f[3][2];
};

// a face the kernels evaluate on the fly: first order, scalar coefficients, its cell inside the `n` cells of the axis
inline bool scalar_face(const pdehip_bc_face_t &r, long n) { return r.kind == PDEHIP_BC_ORDER1 && r.flags == 0 && r.index1 >= 0 && r.index1 < n; }

inline void set_input_bc(InputBCs *fg, int ax, int side, const pdehip_bc_face_t &r)
{
    fg->on[ax][side] = 1; fg->idx[ax][side] = r.index1; fg->c[ax][side] = r.const_v; fg->f[ax][side] = r.factor1;
}

// faces (grid axes) -> on-the-fly BC table (normalised axes: grid axis a of `ndim` is axis 3 - ndim + a of n3); false when a face is not a
// scalar first-order condition.  All or nothing: for the kernels that cannot leave a face to the ghost kernel.
// xplain (pdehip_common.h): 2 / 3 = of the slowest axis only the lower / upper face is a condition (pass first_axis = 1 with it)
inline bool faces_to_input_bcs(int ndim, const long *n3, const pdehip_bc_face_t *faces, InputBCs *fg, int first_axis = 0, int xplain = 0)
{
    memset(fg, 0, sizeof(*fg));
    auto convert = [&](int a, int side) {
        const int ax = 3 - ndim + a;
        const pdehip_bc_face_t &r = faces[2 * a + side];
        if (!scalar_face(r, n3[ax])) return false;
        set_input_bc(fg, ax, side, r);
        return true;
    };
    if (xplain > 1 && !convert(0, xplain == 2 ? 0 : 1)) return false;   // one local face on the slowest axis (first / last slab of a non-periodic axis)
    for (int a = first_axis; a < ndim; a++)
        for (int side = 0; side < 2; side++)
            if (!convert(a, side)) return false;
    return true;
}

// The splitting form, for the kernels that follow the ghost kernel: every scalar face on an axis of `axis_mask` (bit per normalised axis)
// goes to `fg` when the call can fuse at all; `rest` becomes the table for launch_ghosts with those faces skipped (axes beyond `ndim`
// zeroed).  Returns how many faces went where; `rest` needs the ghost kernel only when its count is not zero.
struct FaceSplit {
    int fused, rest;
};
inline FaceSplit split_faces(int ndim, const long *n3, const pdehip_bc_face_t *faces, bool can_fuse, int axis_mask, InputBCs *fg,
                             pdehip_bc_face_t rest[2 * PDEHIP_MAX_DIM])
{
    FaceSplit s = {0, 0};
    memset(fg, 0, sizeof(*fg));
    for (int a = 0; a < PDEHIP_MAX_DIM; a++)
        for (int side = 0; side < 2; side++) {
            pdehip_bc_face_t &r = rest[2 * a + side];
            if (a >= ndim) { memset(&r, 0, sizeof(r)); continue; }
            r = faces[2 * a + side];
            if (r.kind == PDEHIP_BC_SKIP) continue;
            const int ax = 3 - ndim + a;
            if (can_fuse && ((axis_mask >> ax) & 1) && scalar_face(r, n3[ax])) {
                set_input_bc(fg, ax, side, r);
                r.kind = PDEHIP_BC_SKIP;
                s.fused++;
            } else {
                s.rest++;
            }
        }
    return s;
}

}  // namespace pdehip
