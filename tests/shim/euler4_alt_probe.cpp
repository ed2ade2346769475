// euler4_alt_probe.cpp - tests only: the second buffers of the images of levels 1 and 2 of the four-step sweep and the order of a phase
// (py-pde_amd/csrc/pdehip_euler4_plan.h: alt_index, alt_read_index, SCHEDULE - what the kernel itself indexes with and follows) with the
// lane -> patch map and the first buffers behind extern "C", built by g++ in tests/test_euler4_double_buffer.py.  No HIP, no GPU.
#include "../../py-pde_amd/csrc/pdehip_euler4_plan.h"

using namespace pdehip::e4plan;

extern "C" {

// PY NPY NPZ PATCHES THREADS READ_KINDS WAVES ARR GUARD ALT_LEVELS ALT_LEVEL ALT_IMAGE ALT_BYTES LDS_BYTES SCHEDULE_EVENTS
void e4alt_geometry(long *out)
{
    const long v[] = {PY, NPY, NPZ, PATCHES, THREADS, READ_KINDS, WAVES, ARR, GUARD, ALT_LEVELS, ALT_LEVEL, ALT_IMAGE, ALT_BYTES, LDS_BYTES, SCHEDULE_EVENTS};
    for (unsigned k = 0; k < sizeof(v) / sizeof(v[0]); k++) out[k] = v[k];
}

int e4alt_lane_patch(int t) { return lane_patch(t); }
int e4alt_wave_levels(int w) { return wave_levels(w); }
int e4alt_index(int level, int row, int cell, int patch) { return alt_index(level, row, cell, patch); }
int e4alt_read_index(int level, int kind, int patch) { return alt_read_index(level, kind, patch); }
int e4alt_image_index(int level, int row, int cell, int patch) { return image_index(level, row, cell, patch); }
int e4alt_image_read_index(int level, int kind, int patch) { return read_index(level, kind, patch); }

// event k of a phase: op (0 store, 1 read, 2 barrier), image, other (1: the buffer of the other parity), interval
void e4alt_schedule(int k, int *out)
{
    out[0] = SCHEDULE[k].op; out[1] = SCHEDULE[k].image; out[2] = SCHEDULE[k].other; out[3] = SCHEDULE[k].interval;
}

}
