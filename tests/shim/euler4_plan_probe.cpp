// euler4_plan_probe.cpp - tests only: the gate of the four-step sweep (py-pde_amd/csrc/pdehip_euler4_plan.h) behind extern "C", built by
// g++ in tests/test_euler4_plan.py.  No HIP, no GPU.
#include "../../py-pde_amd/csrc/pdehip_euler4_plan.h"

using namespace pdehip::e4plan;

extern "C" {

// q: elem ndim n0 n1 n2 per0 per1 per2 diffusion const_faces unit knob
// out: accepted unit nty ntz nxc nblocks lx block
void e4plan_probe(const long *q, long *out, char *name, long name_size)
{
    Query s;
    s.elem = (int)q[0]; s.ndim = (int)q[1]; s.n0 = q[2]; s.n1 = q[3]; s.n2 = q[4];
    for (int k = 0; k < 3; k++) s.per[k] = (int)q[5 + k];
    s.diffusion = q[8] != 0; s.const_faces = q[9] != 0; s.unit = q[10] != 0; s.knob = (int)q[11];
    const Choice c = plan(s);
    out[0] = c.accepted; out[1] = c.unit; out[2] = c.nty; out[3] = c.ntz; out[4] = c.nxc; out[5] = c.nblocks; out[6] = c.lx; out[7] = c.block;
    name[0] = 0;
    if (c.accepted) format_name(c, name, (size_t)name_size);
}

// TY TZ PY HALO MIN_CHUNK THREADS LDS_BYTES
void e4plan_geometry(long *out)
{
    out[0] = TY; out[1] = TZ; out[2] = PY; out[3] = HALO; out[4] = MIN_CHUNK; out[5] = THREADS; out[6] = LDS_BYTES;
}

int e4plan_knob() { return knob_from_env(); }

}
