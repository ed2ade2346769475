// TESTS ONLY: the conversion of face tables to the on-the-fly table of the stencil kernels (py-pde_amd/csrc/pdehip_faces.h) behind a C interface,
// built with g++ by tests/test_faces_cpu.py.  No HIP, no GPU: the header is plain host C++.
#include "../../py-pde_amd/csrc/pdehip_faces.h"

using namespace pdehip;

namespace {
// f[5 per face]: kind flags index1 const_v factor1
void read_faces(int ndim, const double *f, pdehip_bc_face_t *faces)
{
    memset(faces, 0, sizeof(pdehip_bc_face_t) * 2 * PDEHIP_MAX_DIM);
    for (int i = 0; i < 2 * ndim; i++, f += 5) {
        faces[i].kind = (int32_t)f[0]; faces[i].flags = (int32_t)f[1]; faces[i].index1 = (int64_t)f[2];
        faces[i].const_v = f[3]; faces[i].factor1 = f[4];
    }
}
// fg[4 per (normalised axis, side)]: on idx c f
void write_table(const InputBCs &t, double *fg)
{
    for (int ax = 0; ax < 3; ax++)
        for (int side = 0; side < 2; side++, fg += 4) { fg[0] = t.on[ax][side]; fg[1] = (double)t.idx[ax][side]; fg[2] = t.c[ax][side]; fg[3] = t.f[ax][side]; }
}
}  // namespace

extern "C" {

long faces_probe_scalar(const double *f, long n)
{
    pdehip_bc_face_t faces[2 * PDEHIP_MAX_DIM];
    read_faces(1, f, faces);
    return scalar_face(faces[0], n);
}

// all or nothing; returns 1 and the table, or 0
long faces_probe_all(long ndim, const long *n3, const double *f, long first_axis, long xplain, double *fg)
{
    pdehip_bc_face_t faces[2 * PDEHIP_MAX_DIM];
    read_faces((int)ndim, f, faces);
    InputBCs t;
    if (!faces_to_input_bcs((int)ndim, n3, faces, &t, (int)first_axis, (int)xplain)) return 0;
    write_table(t, fg);
    return 1;
}

// the splitting form; rest_kind[6]: the kinds of the table left for the ghost kernel; counts[2]: fused, rest
void faces_probe_split(long ndim, const long *n3, const double *f, long can_fuse, long axis_mask, double *fg, long *rest_kind, long *counts)
{
    pdehip_bc_face_t faces[2 * PDEHIP_MAX_DIM], rest[2 * PDEHIP_MAX_DIM];
    read_faces((int)ndim, f, faces);
    memset(rest, 0x5a, sizeof(rest));   // (axes beyond ndim must come back zeroed)
    InputBCs t;
    const FaceSplit s = split_faces((int)ndim, n3, faces, can_fuse != 0, (int)axis_mask, &t, rest);
    write_table(t, fg);
    for (int i = 0; i < 2 * PDEHIP_MAX_DIM; i++) rest_kind[i] = rest[i].kind;
    counts[0] = s.fused; counts[1] = s.rest;
}
}
