// pdehip_kernels_e4.hip - launch logic and offline instances of the four-step sweep (pdehip_march4.inc): four Euler steps of the diffusion
// equation per launch on all-periodic fp64 grids, the time levels in LDS.  Its own translation unit and code object, next to
// pdehip_kernels_e2.hip, and like it compiled TWICE (py-pde_amd/Makefile): as pdehip::exactv with -ffp-contract=off (bit-identical to the CPU
// oracle; the default) and, with -DPDEHIP_FAST_VARIANT -ffp-contract=fast, as pdehip::fastv (pdehip_set_fastmath).
#include <type_traits>

#include "pdehip_common.h"
#include "pdehip_euler2_plan.h"
#include "pdehip_euler4_plan.h"

#ifdef PDEHIP_FAST_VARIANT
#define PDEHIP_VARIANT_NS fastv
#else
#define PDEHIP_VARIANT_NS exactv
#endif
namespace pdehip {
namespace PDEHIP_VARIANT_NS {

#include "pdehip_march4.inc"

// *done = false (nothing launched) when e4plan::plan declines or the arrays are outside what the kernel addresses; the caller then goes on
// with two-step and single-step sweeps.  `const_faces`: the right-hand side has no program of conditions and no faces given as arrays.
int launch_euler4(const NGrid &n, const void *in, void *out, double s1, double s2, const InputBCs &fg, bool const_faces, hipStream_t st, bool *done)
{
    *done = false;
    const int knob = e4plan::knob_from_env();
    if (knob == 0 || e2plan::knobs().off || force_generic_kernels() || n.ndim != 3 || n.dtype != PDEHIP_F64 || in == out) return 0;
    if ((uintptr_t)in % 16 || (uintptr_t)out % 16 || n.off % 2 || n.p[0] % 2 || n.p[1] % 2 || n.p[0] >= (1L << 31)) return 0;
    // a lane's byte offset inside a plane is a 32-bit register, and so is the number of a plane
    if (!e4plan::offsets_fit(n.off, n.p[0]) || n.n[0] >= (1L << 30)) return 0;
    e4plan::Query q;
    q.elem = 8; q.ndim = n.ndim; q.n0 = n.n[0]; q.n1 = n.n[1]; q.n2 = n.n[2];
    for (int k = 0; k < 3; k++) q.per[k] = classify_axis(fg, k, n.n[k]);
    q.diffusion = true; q.const_faces = const_faces; q.knob = knob;
    q.unit = n.lap_scale[0] == 1.0 && n.lap_scale[1] == 1.0 && n.lap_scale[2] == 1.0 && s1 == 1.0;
    const e4plan::Choice c = e4plan::plan(q);
    if (!c.accepted) return 0;
    LapArgs a;
    memset(&a, 0, sizeof(a));
    a.in = in; a.out = out; a.y = in;
    a.n0 = n.n[0]; a.n1 = n.n[1]; a.n2 = n.n[2];
    a.p0 = n.p[0]; a.p1 = n.p[1]; a.off = n.off;
    a.o_off = n.off; a.o_s0 = a.p0; a.o_s1 = a.p1;
    a.sx = n.lap_scale[0]; a.sy = n.lap_scale[1]; a.sz = n.lap_scale[2];
    a.s1 = s1; a.s2 = s2;
    a.ndim = 3;
    for (int k = 0; k < 3; k++) a.per[k] = 1;
    a.lx = c.lx; a.xstride = c.lx; a.nxc = c.nxc; a.nty = c.nty; a.ntz = c.ntz; a.nblocks = c.nblocks;
    const void *kernel = c.unit ? reinterpret_cast<const void *>(&euler4_kernel<double, E2_DIFFUSION_UNIT>)
                                : reinterpret_cast<const void *>(&euler4_kernel<double, E2_DIFFUSION>);
    char name[160];
    e4plan::format_name(c, name, sizeof(name));
    note_kernel("%s", name);
    void *args[] = {&a};
    // dynamic LDS: the second buffers of images 1 and 2 (preload_e4_kernels has asked for the size; a captured launch carries it in its node)
    PDEHIP_HIP(hipLaunchKernel(kernel, dim3((unsigned)c.nblocks), dim3(c.block), args, (size_t)e4plan::ALT_BYTES, st));
    *done = true;
    return 0;
}

// (the code object of this translation unit is loaded when the device is selected, not in the middle of a run: preload_stencil_kernels)
// Both instances are told how much dynamic LDS their launches ask for.  A runtime that refuses the size fails the device selection with its
// error, and one that refuses it at the launch fails the run: there is no other version of this kernel.
int preload_e4_kernels()
{
    const void *const kernels[] = {reinterpret_cast<const void *>(&euler4_kernel<double, E2_DIFFUSION_UNIT>),
                                   reinterpret_cast<const void *>(&euler4_kernel<double, E2_DIFFUSION>)};
    for (const void *kernel : kernels) {
        PDEHIP_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)e4plan::ALT_BYTES));
        hipFuncAttributes attr;
        PDEHIP_HIP(hipFuncGetAttributes(&attr, kernel));
    }
    return 0;
}

}  // namespace PDEHIP_VARIANT_NS
}  // namespace pdehip
