// TESTS ONLY: the planner of the two-step sweeps (py-pde_amd/csrc/pdehip_euler2_plan.h) behind a C interface, built with g++ by
// tests/test_euler2_plan.py.  No HIP, no GPU: the header is plain host C++.
#include "../../py-pde_amd/csrc/pdehip_euler2_plan.h"

using namespace pdehip::e2plan;

extern "C" {

// q[15]: elem ndim n0 n1 n2 per0 per1 per2 xplain ends m2 plan unit stage_alias narrow_only
// k[16] (NULL: the defaults): ry blocks order off f32_vec f32_ry f32_svec f32_sry wide4_off stage_wide open_off open_y_off per3_off peryz_off minlx unit_off
// out[24]: accepted family elem vec ry m2 has_y ragged xs nt unit open_tail open_y ntz nty nxc xstride nblocks lx nwy nwz block per0 has_instance
void e2plan_probe(const long *q, const long *k, long *out, char *name, long name_size)
{
    Query Q;
    Q.elem = (int)q[0]; Q.ndim = (int)q[1]; Q.n0 = q[2]; Q.n1 = q[3]; Q.n2 = q[4];
    for (int i = 0; i < 3; i++) Q.per[i] = (int)q[5 + i];
    Q.xplain = (int)q[8]; Q.ends = (int)q[9]; Q.m2 = (int)q[10]; Q.plan = q[11] != 0; Q.unit = q[12] != 0; Q.stage_alias = q[13] != 0; Q.narrow_only = q[14] != 0;
    Knobs K;
    if (k) {
        K.ry = (int)k[0]; K.blocks = k[1]; K.order = (int)k[2]; K.off = k[3] != 0;
        K.f32_vec = (int)k[4]; K.f32_ry = (int)k[5]; K.f32_svec = (int)k[6]; K.f32_sry = (int)k[7];
        K.wide4_off = k[8] != 0; K.stage_wide = (int)k[9]; K.open_off = k[10] != 0; K.open_y_off = k[11] != 0; K.per3_off = k[12] != 0; K.peryz_off = k[13] != 0;
        K.minlx = k[14]; K.unit_off = k[15] != 0;
    }
    const Choice c = plan(Q, K);
    const long v[24] = {c.accepted, c.family, c.elem, c.vec, c.ry, c.m2, c.has_y, c.ragged, c.xs, c.nt, c.unit, c.open_tail, c.open_y, c.ntz, c.nty, c.nxc, c.xstride,
                        c.nblocks, c.lx, c.nwy, c.nwz, (long)c.block, c.per0, c.accepted && !Q.plan && has_instance(c)};
    for (int i = 0; i < 24; i++) out[i] = v[i];
    format_name(c, name, (size_t)name_size);
}

// the compiled instances of one (element size, cells per lane): 7 numbers each (family ry has_y ragged xs nt stage); returns their count
int e2plan_instances(int elem, int vec, long *out, int max)
{
    int count;
    const Instance *list = instances(elem, vec, &count);
    for (int i = 0; i < count && i < max; i++) {
        const long v[7] = {list[i].family, list[i].ry, list[i].has_y, list[i].ragged, list[i].xs, list[i].nt, list[i].stage};
        for (int j = 0; j < 7; j++) out[7 * i + j] = v[j];
    }
    return count;
}

// the knobs as read from the environment of this process (the same order as k[] above)
void e2plan_knobs_from_env(long *k)
{
    const Knobs K = knobs_from_env();
    const long v[16] = {K.ry, K.blocks, K.order, K.off, K.f32_vec, K.f32_ry, K.f32_svec, K.f32_sry, K.wide4_off, K.stage_wide, K.open_off, K.open_y_off, K.per3_off, K.peryz_off, K.minlx, K.unit_off};
    for (int i = 0; i < 16; i++) k[i] = v[i];
}
}
