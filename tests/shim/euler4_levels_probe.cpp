// euler4_levels_probe.cpp - tests only: the levels a lane of the four-step sweep is needed at and the bound on its 32-bit plane offsets
// (py-pde_amd/csrc/pdehip_euler4_plan.h: lane_levels, offsets_fit - the functions the kernel and its launcher use) behind extern "C", built
// by g++ in tests/test_euler4_lane_levels.py.  No HIP, no GPU.
#include "../../py-pde_amd/csrc/pdehip_euler4_plan.h"

using namespace pdehip::e4plan;

extern "C" {

int e4levels_lane_levels(int t) { return lane_levels(t); }
int e4levels_offsets_fit(long off, long p0) { return offsets_fit(off, p0) ? 1 : 0; }

}
