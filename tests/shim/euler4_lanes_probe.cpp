// euler4_lanes_probe.cpp - tests only: the lane -> patch map and the wave roles of the four-step sweep (py-pde_amd/csrc/pdehip_euler4_plan.h:
// lane_patch, wave_levels - the functions the kernel itself uses) with the image they index (image_index, read_index) behind extern "C",
// built by g++ in tests/test_euler4_lanes.py.  No HIP, no GPU.
#include "../../py-pde_amd/csrc/pdehip_euler4_plan.h"

using namespace pdehip::e4plan;

extern "C" {

// TY TZ PY HALO LEVELS NPY NPZ PATCHES THREADS READ_KINDS WAVES OWNER_WAVES IMAGE
void e4lanes_geometry(long *out)
{
    const long v[] = {TY, TZ, PY, HALO, LEVELS, NPY, NPZ, PATCHES, THREADS, READ_KINDS, WAVES, OWNER_WAVES, IMAGE};
    for (unsigned k = 0; k < sizeof(v) / sizeof(v[0]); k++) out[k] = v[k];
}

int e4lanes_lane_patch(int t) { return lane_patch(t); }
int e4lanes_wave_levels(int w) { return wave_levels(w); }
int e4lanes_index(int level, int row, int cell, int patch) { return image_index(level, row, cell, patch); }
int e4lanes_read_index(int level, int kind, int patch) { return read_index(level, kind, patch); }

}
