// TESTS ONLY: the planner of the run-time built one-level sweeps (py-pde_amd/csrc/pdehip_jit_plan.h) behind a C interface, built with g++ by
// tests/test_jit_cases_cpu.py.  No HIP, no GPU: the header is plain host C++.
#include "../../py-pde_amd/csrc/pdehip_jit_plan.h"

using namespace pdehip::jitplan;

extern "C" {

// q[10]: elem ndim n0 n1 n2 aligned stage kind nk fused
// k[4] (NULL: nothing set): ry cz wy blocks
// out[15]: generic elem vec ry cz wy hasx ibc stage tails ntz nty lx nxc nblocks; returns the threads per workgroup
long jitplan_probe(const long *q, const long *k, long *out, char *name, long name_size)
{
    Query Q;
    Q.elem = (int)q[0]; Q.ndim = (int)q[1]; Q.n0 = q[2]; Q.n1 = q[3]; Q.n2 = q[4];
    Q.aligned = q[5] != 0; Q.stage = q[6] != 0; Q.kind = (int)q[7]; Q.nk = (int)q[8]; Q.fused = q[9] != 0;
    Knobs K;
    if (k) { K.ry = (int)k[0]; K.cz = (int)k[1]; K.wy = (int)k[2]; K.blocks = k[3]; }
    const Choice c = plan(Q, K);
    const long v[15] = {c.generic, c.elem, c.vec, c.ry, c.cz, c.wy, c.hasx, c.ibc, c.stage, c.tails, c.ntz, c.nty, c.lx, c.nxc, c.nblocks};
    for (int i = 0; i < 15; i++) out[i] = v[i];
    format_name(c, name, (size_t)name_size);
    return (long)c.threads;
}

// the knobs as read from the environment of this process (the same order as k[] above)
void jitplan_knobs_from_env(long *k)
{
    const Knobs K = knobs_from_env();
    k[0] = K.ry; k[1] = K.cz; k[2] = K.wy; k[3] = K.blocks;
}

// ---- the route of the fixed-step Euler loop ----
// k[3] (NULL: the defaults): tile tile_cells graph
static LoopKnobs loop_knobs(const long *k)
{
    LoopKnobs K;
    if (k) { K.tile = k[0] != 0; K.tile_cells = k[1]; K.graph = k[2] != 0; }
    return K;
}

// p[7 per pass, the first min(npasses, 2) passes]: src extras[0] extras[1] extras[2] out faces second_body
// q[7]: npasses ncomp ndim n1 n2 nsteps bc_program; returns the mode of the tile kernel or 0
long jitplan_tile_mode(const long *p, const long *q, const long *k)
{
    PassDesc d[2];
    for (int i = 0; i < 2 && i < q[0]; i++, p += 7) d[i] = {(int)p[0], {(int)p[1], (int)p[2], (int)p[3]}, (int)p[4], p[5] != 0, p[6] != 0};
    return tile_mode(d, (int)q[0], (int)q[1], (int)q[2], q[3], q[4], q[5], q[6] != 0, loop_knobs(k));
}

long jitplan_replay_applies(long uses_time, long nsteps, long comm, const long *k) { return replay_applies(uses_time != 0, nsteps, comm != 0, loop_knobs(k)); }

void jitplan_loop_knobs_from_env(long *k)
{
    const LoopKnobs K = loop_knobs_from_env();
    k[0] = K.tile; k[1] = K.tile_cells; k[2] = K.graph;
}
}
