// euler4_image_probe.cpp - tests only: the LDS image of the four-step sweep (py-pde_amd/csrc/pdehip_euler4_plan.h: image_index, read_index,
// patch_of_thread - the functions the kernel itself indexes with) behind extern "C", built by g++ in tests/test_euler4_image.py.  No HIP, no GPU.
#include "../../py-pde_amd/csrc/pdehip_euler4_plan.h"

using namespace pdehip::e4plan;

extern "C" {

// TY TZ PY HALO LEVELS NPY NPZ PATCHES THREADS ARR NARR GUARD IMAGE READ_KINDS allocation (doubles)
void e4image_geometry(long *out)
{
    const long v[] = {TY, TZ, PY, HALO, LEVELS, NPY, NPZ, PATCHES, THREADS, ARR, NARR, GUARD, IMAGE, READ_KINDS, (long)LEVELS * LROWS * LPITCH};
    for (unsigned k = 0; k < sizeof(v) / sizeof(v[0]); k++) out[k] = v[k];
}

int e4image_patch_of_thread(int t) { return patch_of_thread(t); }
int e4image_index(int level, int row, int cell, int patch) { return image_index(level, row, cell, patch); }
int e4image_read_index(int level, int kind, int patch) { return read_index(level, kind, patch); }

}
