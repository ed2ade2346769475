// pdehip_kernels_e2.hip - launch logic and offline instances of the two-level sweeps (pdehip_march2.inc): two Euler steps per sweep, the fused
// Cahn-Hilliard right-hand side, Runge-Kutta stage sweeps.  Split from pdehip_kernels.hip (round 6): its own translation unit and code object.
// Same compile flags (-ffp-contract=off: bit-identical to the CPU oracle).
#include "pdehip_common.h"
#include "pdehip_euler2_plan.h"

// Compiled TWICE (py-pde_amd/Makefile): as pdehip::exactv with -ffp-contract=off (bit-identical to the CPU oracle; the default) and, with
// -DPDEHIP_FAST_VARIANT -ffp-contract=fast, as pdehip::fastv (FMA contraction like numba's default fastmath, pde/backends/numba/utils.py:330-336;
// opt-in through pdehip_set_fastmath, results within 1e-10 of the exact build).  pdehip_dispatch.hip picks one per call.
#ifdef PDEHIP_FAST_VARIANT
#define PDEHIP_VARIANT_NS fastv
#else
#define PDEHIP_VARIANT_NS exactv
#endif
namespace pdehip {
namespace PDEHIP_VARIANT_NS {

#include "pdehip_march2.inc"

// ---------------------------------------------------------------------------------------------
// two Euler steps per sweep (pdehip_march2.inc).  *done = false when the grid / BCs are outside
// what the kernel covers; the caller then takes two single steps.  What runs is decided by
// e2plan::plan (pdehip_euler2_plan.h); this file instantiates the kernels and launches.
// ---------------------------------------------------------------------------------------------
static_assert(e2plan::M2_DIFFUSION == E2_DIFFUSION && e2plan::M2_CH_EULER == E2_CH_EULER && e2plan::M2_CH_SCALED == E2_CH_SCALED && e2plan::M2_CUSTOM == E2_CUSTOM &&
                  e2plan::M2_CUSTOM2 == E2_CUSTOM2 && e2plan::M2_CH_STAGE == E2_CH_STAGE && e2plan::M2_DIFFUSION_UNIT == E2_DIFFUSION_UNIT,
              "pdehip_euler2_plan.h and pdehip_device.h disagree");

// the compiled instance of a choice (the lists of pdehip_euler2_plan.h); nullptr: none
template <typename T, int VEC>
static const void *euler2_instance(const e2plan::Choice &c)
{
#define PDEHIP_E2_FN(...) reinterpret_cast<const void *>(&__VA_ARGS__)
    // unit spacing x streaming stores
#define PDEHIP_E2_L(FAM_, ...)                                                                                                               \
    if (c.family == e2plan::FAM_)                                                                                                            \
        return c.unit ? (c.nt ? PDEHIP_E2_FN(__VA_ARGS__, E2_DIFFUSION_UNIT, true>) : PDEHIP_E2_FN(__VA_ARGS__, E2_DIFFUSION_UNIT, false>)) \
                      : (c.nt ? PDEHIP_E2_FN(__VA_ARGS__, E2_DIFFUSION, true>) : PDEHIP_E2_FN(__VA_ARGS__, E2_DIFFUSION, false>));
#define PDEHIP_E2_S(FAM_, ...) \
    if (c.family == e2plan::FAM_) return PDEHIP_E2_FN(__VA_ARGS__);
#define PDEHIP_E2_P(RY_, HY_, RG_, XS_, NT_, ST_)                                                                                           \
    if (c.family == e2plan::PLAIN && c.ry == RY_ && c.has_y == HY_ && c.ragged == RG_ && c.xs == XS_ && c.nt == NT_) {                      \
        if constexpr (!XS_) {   /* every instance except the one-sided slab ends */                                                         \
            if (c.m2 == E2_DIFFUSION && c.unit) return PDEHIP_E2_FN(euler2_kernel<T, VEC, RY_, E2_DIFFUSION_UNIT, HY_, RG_, XS_, NT_>);     \
        }                                                                                                                                   \
        if (c.m2 == E2_DIFFUSION) return PDEHIP_E2_FN(euler2_kernel<T, VEC, RY_, E2_DIFFUSION, HY_, RG_, XS_, NT_>);                        \
        if (c.m2 == E2_CH_EULER) return PDEHIP_E2_FN(euler2_kernel<T, VEC, RY_, E2_CH_EULER, HY_, RG_, XS_, NT_>);                          \
        if (c.m2 == E2_CH_SCALED) return PDEHIP_E2_FN(euler2_kernel<T, VEC, RY_, E2_CH_SCALED, HY_, RG_, XS_, NT_>);                        \
        if constexpr (ST_) {                                                                                                                \
            if (c.m2 == E2_CH_STAGE) return PDEHIP_E2_FN(euler2_kernel<T, VEC, RY_, E2_CH_STAGE, HY_, RG_, false, false>);                  \
        }                                                                                                                                   \
        return nullptr;                                                                                                                     \
    }
    if constexpr (sizeof(T) == 8) { PDEHIP_E2_INSTANCES_F64_2(PDEHIP_E2_P, PDEHIP_E2_L, PDEHIP_E2_S) }
    else if constexpr (VEC == 4) { PDEHIP_E2_INSTANCES_F32_4(PDEHIP_E2_P, PDEHIP_E2_L, PDEHIP_E2_S) }
    else { PDEHIP_E2_INSTANCES_F32_2(PDEHIP_E2_P, PDEHIP_E2_L, PDEHIP_E2_S) }
#undef PDEHIP_E2_P
#undef PDEHIP_E2_S
#undef PDEHIP_E2_L
#undef PDEHIP_E2_FN
    return nullptr;
}

template <typename T>
static int launch_euler2_t(const NGrid &n, LapArgs a, int xplain, hipStream_t st, bool *done, bool dry_run, int ends, int m2,
                           Euler2Plan *plan, bool narrow_only)
{
    e2plan::Query q;
    q.elem = sizeof(T); q.ndim = n.ndim; q.n0 = a.n0; q.n1 = a.n1; q.n2 = a.n2;
    for (int k = 0; k < 3; k++) q.per[k] = a.per[k];
    q.xplain = xplain; q.ends = ends; q.m2 = m2; q.plan = plan != nullptr; q.narrow_only = narrow_only;
    q.unit = a.sx == 1.0 && a.sy == 1.0 && a.sz == 1.0 && a.s1 == 1.0;
    q.stage_alias = false;
    if (m2 == E2_CH_STAGE) {
        q.stage_alias = a.st_out == a.st_y || a.out == a.st_y;
        for (int m = 0; m < 5; m++) q.stage_alias = q.stage_alias || (a.st_k[m] && (a.st_k[m] == a.st_out || a.st_k[m] == a.out));
    }
    const e2plan::Choice c = e2plan::plan(q, e2plan::knobs());
    if (!c.accepted) return 0;
    if (dry_run) { *done = true; return 0; }
    a.ntz = c.ntz; a.nty = c.nty; a.lx = c.lx; a.nxc = c.nxc; a.xstride = c.xstride; a.nwy = c.nwy; a.nblocks = c.nblocks;
    a.z_open = c.open_tail > 0; a.no_swizzle = 0; a.per[0] = c.per0;
    if (plan) {   // the caller launches a run-time compiled instance itself (pdehip_jit.hip)
        plan->a = a; plan->grid = (unsigned)c.nblocks; plan->block = c.block; plan->ry = c.ry; plan->has_y = c.has_y;
        *done = true;
        return 0;
    }
    if (m2 == E2_CUSTOM || m2 == E2_CUSTOM2) PDEHIP_FAIL(E_RUNTIME, "internal: the custom two-level kernel exists only as a run-time build");
    const void *kernel;
    if constexpr (sizeof(T) == 8) kernel = euler2_instance<T, 2>(c);
    else kernel = c.vec == 4 ? euler2_instance<T, 4>(c) : euler2_instance<T, 2>(c);
    if (!kernel) return 0;   // no instance of this shape (the caller takes the pass-by-pass path)
    char name[192];
    e2plan::format_name(c, name, sizeof(name));
    if (name[0]) note_kernel("%s", name);
    void *args[] = {&a};
    PDEHIP_HIP(hipLaunchKernel(kernel, dim3((unsigned)c.nblocks), dim3(c.block), args, 0, st));
    if (c.open_tail || c.open_y) PDEHIP_TRY(shell_open_rows(n, a, (int)c.open_tail, (int)c.open_y, st));   // the last columns of every row, the last rows of every plane
    *done = true;
    return 0;
}

int launch_euler2(const NGrid &n, const void *in, void *out, double s1, double s2, const InputBCs &fg,
                  int xplain, hipStream_t st, bool *done, bool dry_run, int ends, int m2, const InputBCs *fg1, double gamma,
                  Euler2Plan *plan, const StageFuse *stage, int yzplain)
{
    *done = false;
    if ((m2 == E2_CH_STAGE) != (stage != nullptr)) PDEHIP_FAIL(E_RUNTIME, "internal: stage sweep without / with a stage descriptor");
    const long vec = 16 / elem_size(n.dtype);
    if ((m2 == E2_CH_EULER || m2 == E2_CH_SCALED || m2 == E2_CH_STAGE) && !fg1) PDEHIP_FAIL(E_RUNTIME, "internal: fused Cahn-Hilliard sweep without the faces of mu");
    if (e2plan::knobs().off || force_generic_kernels() || (n.ndim != 3 && n.ndim != 2) || in == out) return 0;
    // kernel axes (march, rows, lanes) <- normalised grid axes: 3-D (0, 1, 2); 2-D (1, -, 2): the march axis is the first
    // grid axis and there are no rows
    const int am = n.ndim == 3 ? 0 : 1;
    if (n.ndim == 2 && xplain) return 0;
    if (n.n[am] < (xplain ? 1 : 4) || (n.ndim == 3 && n.n[1] < 4) || n.n[2] < 4 || n.p[am] >= (1L << 31)) return 0;
    const bool narrow_only = n.dtype == PDEHIP_F32 && n.off % vec != 0 && n.off % 2 == 0;   // (e2plan::Query)
    if ((uintptr_t)in % 16 || (uintptr_t)out % 16 || (n.off % vec && !narrow_only) || n.p[am] % vec || n.p[1] % vec) return 0;
    LapArgs a;
    memset(&a, 0, sizeof(a));
    for (int k = 0; k < 3; k++) {   // k = kernel axis
        if (k == 0 && xplain == 1) continue;
        if (k == 0 && xplain > 1) {
            // first / last slab of a non-periodic axis: ONE local face (the other side has real halo planes)
            const int side = xplain == 2 ? 0 : 1;
            const InputBCs &f1 = fg1 ? *fg1 : fg;
            const long want = side ? n.n[am] - 1 : 0;
            if (!fg.on[am][side] || fg.idx[am][side] != want || !f1.on[am][side] || f1.idx[am][side] != want) return 0;
            a.ibc[0][side].on = 1; a.ibc[0][side].idx = want; a.ibc[0][side].c = fg.c[am][side]; a.ibc[0][side].f = fg.f[am][side];
            a.ibc1[0][side].on = 1; a.ibc1[0][side].idx = want; a.ibc1[0][side].c = f1.c[am][side]; a.ibc1[0][side].f = f1.f[am][side];
            continue;
        }
        if (k == 1 && n.ndim == 2) { a.per[1] = 1; continue; }
        // block decomposition (pdehip_block2_loops.h): `n` describes a BOX of a larger array - two real halo rows (bit 0) / columns
        // (bit 1) on either side in memory; no faces on those axes
        if (k >= 1 && n.ndim == 3 && (yzplain & (1 << (k - 1)))) { a.per[k] = 2; continue; }
        const int ax = (k == 0) ? am : k;
        // both faces periodic, or both local (virtual point from the adjacent cell); the same for both levels
        const int cls = classify_axis(fg, ax, n.n[ax]);
        if (cls < 0 || (fg1 && classify_axis(*fg1, ax, n.n[ax]) != cls)) return 0;
        a.per[k] = cls;
        for (int side = 0; side < 2; side++) {
            a.ibc[k][side].on = 1;
            a.ibc[k][side].idx = fg.idx[ax][side];
            a.ibc[k][side].c = fg.c[ax][side];
            a.ibc[k][side].f = fg.f[ax][side];
            const InputBCs &f1 = fg1 ? *fg1 : fg;
            a.ibc1[k][side].on = 1;
            a.ibc1[k][side].idx = f1.idx[ax][side];
            a.ibc1[k][side].c = f1.c[ax][side];
            a.ibc1[k][side].f = f1.f[ax][side];
        }
    }
    a.gamma = gamma;
    if (stage) {
        if (!stage->y || !stage->out2 || stage->out2 == in || ((stage->kind == 0 || stage->kind == 3) && !out)) PDEHIP_FAIL(E_VALUE, "stage sweep: NULL or aliased array pointer");
        a.st_kind = stage->kind; a.st_y = stage->y; a.st_out = stage->out2; a.st_err = stage->err;
        int nk = 0;
        for (int m = 0; m < 5 && stage->k[m]; m++, nk++) { a.st_k[m] = stage->k[m]; a.st_c[m] = stage->c[m]; }
        if ((stage->kind == 1 && nk != 3) || (stage->kind == 2 && (nk != 4 || !stage->err)) || (stage->kind == 3 && nk != 1) ||
            (stage->kind == 4 && (nk != 2 || !stage->err || stage->k[1] != in)))
            PDEHIP_FAIL(E_RUNTIME, "internal: malformed stage descriptor");
        a.st_c[5] = stage->c_new;
        if (!stage_aligned(a)) return 0;
    }
    a.in = in; a.out = out; a.y = in;
    a.n0 = n.n[am]; a.n1 = n.ndim == 3 ? n.n[1] : 1; a.n2 = n.n[2];
    a.p0 = n.p[am]; a.p1 = n.ndim == 3 ? n.p[1] : 0; a.off = n.off;
    a.o_off = n.off; a.o_s0 = a.p0; a.o_s1 = a.p1;
    a.sx = n.lap_scale[am]; a.sy = n.lap_scale[1]; a.sz = n.lap_scale[2];
    a.s1 = s1; a.s2 = s2;
    a.ndim = n.ndim; a.any_ibc = 1;
    // squared central gradient of the custom epilogue, kernel-axis order (cartesian.py:661: 0.25 / dx**2)
    a.gs[0] = 0.25 / (n.dx[am] * n.dx[am]); a.gs[1] = 0.25 / (n.dx[1] * n.dx[1]); a.gs[2] = 0.25 / (n.dx[2] * n.dx[2]);
    if (n.dtype == PDEHIP_F64) return launch_euler2_t<double>(n, a, xplain, st, done, dry_run, ends, m2, plan, false);
    return launch_euler2_t<float>(n, a, xplain, st, done, dry_run, ends, m2, plan, narrow_only);
}

// (see preload_stencil_kernels, pdehip_kernels.hip: the code object of this translation unit is loaded when the device is selected, not in the middle of a run)
int preload_e2_kernels()
{
    hipFuncAttributes attr;
    PDEHIP_HIP(hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&euler2_kernel<double, 2, 4, E2_DIFFUSION, true, false, false, false>)));
    return 0;
}

}  // namespace PDEHIP_VARIANT_NS
}  // namespace pdehip
