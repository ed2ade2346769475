// pdehip_f32p.hip — the pure-fp32 arithmetic mode of fp32 fields: pdehip_laplace_f32p, pdehip_euler_run_f32p, pdehip_f32p_supported.
//
// Every other kernel of the library computes fp32 fields in fp64 registers (numba's promotion); the reference's torch backend
// rounds every operation to fp32 instead (pde/backends/torch/operators/cartesian.py:55-83, pde/backends/torch/_solvers.py:149).  The
// entry points here reproduce that arithmetic bit for bit; the mode travels per call, by the choice of entry point - there is no
// process-wide switch.  Built once (exact only: -ffp-contract=off); the kernels are in pdehip_f32p.inc.
#include "pdehip_common.h"

namespace pdehip {
namespace {

#include "pdehip_f32p.inc"

int fill_args(const pdehip_grid_t *g, const char *who, NGrid *n, F32pArgs *a)
{
    PDEHIP_TRY(norm_grid(g, n));
    if (n->dtype != PDEHIP_F32) PDEHIP_FAIL(E_NOTIMPL, "%s: the pure-fp32 arithmetic mode serves fp32 fields only", who);
    if (n->n[1] * n->n[2] >= (1L << 31)) PDEHIP_FAIL(E_NOTIMPL, "%s: more than 2^31 - 1 cells in a plane of the two fastest axes", who);
    memset(a, 0, sizeof(*a));
    a->n0 = n->n[0]; a->n1 = n->n[1]; a->n2 = n->n[2];
    a->p0 = n->p[0]; a->p1 = n->p[1];
    a->off = n->off;
    // s_a = fp32(dx_a ** -2): the power in double, rounded once
    a->s0 = (float)n->lap_scale[0]; a->s1 = (float)n->lap_scale[1]; a->s2 = (float)n->lap_scale[2];
    a->per0 = a->per1 = a->per2 = 1;
    a->seg = 1; a->nyt = a->nseg = a->nxc = 1;
    return 0;
}

void set_output(F32pArgs *a, const NGrid &n, int layout)
{
    const OutStr o = out_strides(n, layout);
    a->o_off = o.off; a->o_s0 = o.s0; a->o_s1 = o.s1;
}

// planes per march so that a launch has about `want` waves (at least 8 planes: a march starts with up to four extra plane loads)
int choose_segment(long n0, long waves_per_plane_set, long want)
{
    long nseg = want / (waves_per_plane_set > 0 ? waves_per_plane_set : 1);
    if (nseg < 1) nseg = 1;
    long seg = (n0 + nseg - 1) / nseg;
    if (seg < 8) seg = 8;
    if (seg > n0) seg = n0;
    return (int)seg;
}

template <bool EULER>
void launch_generic(int ndim, const F32pArgs &a, const float *in, float *out, hipStream_t s)
{
    // planes by blockIdx.y, the cells of a plane flat over blockIdx.x (both strided inside the kernel beyond the limits used here)
    const long plane = a.n1 * a.n2, bx = (plane + 255) / 256;
    const dim3 grid((unsigned)(bx > 65536 ? 65536 : bx), (unsigned)(a.n0 > 65535 ? 65535 : a.n0)), block(256);
    if (ndim == 1) hipLaunchKernelGGL((f32p_generic_kernel<1, EULER>), grid, block, 0, s, a, in, out);
    else if (ndim == 2) hipLaunchKernelGGL((f32p_generic_kernel<2, EULER>), grid, block, 0, s, a, in, out);
    else hipLaunchKernelGGL((f32p_generic_kernel<3, EULER>), grid, block, 0, s, a, in, out);
}

// the march instances take 3-D grids whose rows are whole 16-byte vectors
bool lap_fast(const NGrid &n, const void *in, const void *out)
{
    return n.ndim == 3 && n.n[2] % 4 == 0 && n.n[2] >= 4 && (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0;
}
bool euler_fast(const NGrid &n) { return n.ndim == 3 && n.n[2] % 4 == 0 && n.n[2] >= 4 && n.n[2] <= 1024 && n.n[0] >= 2 && n.n[1] >= 2; }

// faces of the Euler loop: every axis periodic, or zero-derivative on both sides (ghost = the adjacent cell); 1 / 0, -1 = refused
int face_pattern(const pdehip_bc_face_t &lo, const pdehip_bc_face_t &hi, long n)
{
    const pdehip_bc_face_t *f[2] = {&lo, &hi};
    for (int s = 0; s < 2; s++)
        if (f[s]->kind != PDEHIP_BC_ORDER1 || f[s]->flags != 0 || f[s]->const_v != 0.0 || f[s]->factor1 != 1.0) return -1;
    if (lo.index1 == 0 && hi.index1 == n - 1) return 0;          // (n == 1: a periodic axis is the same thing)
    if (lo.index1 == n - 1 && hi.index1 == 0) return 1;
    return -1;
}

int euler_faces(const pdehip_grid_t *g, const pdehip_rhs_t *rhs, const NGrid &n, F32pArgs *a)
{
    if (rhs->kind != PDEHIP_RHS_DIFFUSION) PDEHIP_FAIL(E_NOTIMPL, "euler_run_f32p: only the diffusion equation has a pure-fp32 Euler loop");
    if (rhs->bc_program) PDEHIP_FAIL(E_NOTIMPL, "euler_run_f32p: faces given as expressions are not covered by the pure-fp32 Euler loop");
    int per[3] = {1, 1, 1};
    for (int d = 0; d < g->ndim; d++) {
        const int ax = 3 - g->ndim + d;
        per[ax] = face_pattern(rhs->bc_c[2 * d], rhs->bc_c[2 * d + 1], n.n[ax]);
        if (per[ax] < 0)
            PDEHIP_FAIL(E_NOTIMPL, "euler_run_f32p: axis %d is neither periodic nor zero-derivative on both sides - the pure-fp32 Euler loop "
                        "refuses inhomogeneous faces (the reference's torch stepper rounds their ghost cells differently)", d);
    }
    a->per0 = per[0]; a->per1 = per[1]; a->per2 = per[2];
    return 0;
}

}  // namespace
}  // namespace pdehip

using namespace pdehip;

/* Laplacian, pure fp32 */
extern "C" int pdehip_laplace_f32p(const pdehip_grid_t *g, const void *in_full, void *out, int out_layout, void *stream)
{
    NGrid n;
    F32pArgs a;
    PDEHIP_TRY(fill_args(g, "laplace_f32p", &n, &a));
    if (!in_full || !out) PDEHIP_FAIL(E_VALUE, "laplace_f32p: NULL pointer");
    if (in_full == out) PDEHIP_FAIL(E_VALUE, "laplace_f32p: input and output are the same array");
    if (out_layout != PDEHIP_OUT_VALID && out_layout != PDEHIP_OUT_FULL) PDEHIP_FAIL(E_VALUE, "laplace_f32p: unknown output layout %d", out_layout);
    set_output(&a, n, out_layout);
    hipStream_t s = as_stream(stream);
    if (lap_fast(n, in_full, out)) {
        a.nxc = (int)((a.n2 + 255) / 256);
        a.nyt = (int)((a.n1 + kF32pRows - 1) / kF32pRows);
        a.seg = choose_segment(a.n0, (long)a.nxc * a.nyt, 8192);
        a.nseg = (int)((a.n0 + a.seg - 1) / a.seg);
        const long waves = (long)a.nxc * a.nyt * a.nseg;
        hipLaunchKernelGGL(lap32_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, a, (const float *)in_full, (float *)out);
        note_kernel("lap32_kernel<march,R=%d,seg=%d>", kF32pRows, a.seg);
    } else {
        launch_generic<false>(g->ndim, a, (const float *)in_full, (float *)out, s);
        note_kernel("lap32_kernel<generic,%d>", g->ndim);
    }
    PDEHIP_HIP(hipGetLastError());
    return 0;
}

/* answer: 0 = refused, 1 = accepted (one cell per thread), 2 = accepted (the march instance) */
extern "C" int pdehip_f32p_supported(const pdehip_grid_t *g, const pdehip_rhs_t *rhs, int *answer)
{
    if (!answer) PDEHIP_FAIL(E_VALUE, "f32p_supported: NULL pointer");
    *answer = 0;
    NGrid n;
    F32pArgs a;
    if (fill_args(g, "f32p_supported", &n, &a) != 0) return 0;
    if (!rhs) {
        *answer = (n.ndim == 3 && n.n[2] % 4 == 0 && n.n[2] >= 4) ? 2 : 1;
        return 0;
    }
    if (euler_faces(g, rhs, n, &a) != 0) return 0;
    *answer = euler_fast(n) ? 2 : 1;
    return 0;
}

/* fixed-step Euler loop of the diffusion equation, pure fp32 */
extern "C" int pdehip_euler_run_f32p(const pdehip_grid_t *g, const pdehip_rhs_t *rhs, void *buf_a, void *buf_b, double dt, int64_t nsteps,
                                     void **result, void *stream)
{
    NGrid n;
    F32pArgs a;
    PDEHIP_TRY(fill_args(g, "euler_run_f32p", &n, &a));
    if (!rhs || !buf_a || !buf_b || !result) PDEHIP_FAIL(E_VALUE, "euler_run_f32p: NULL pointer");
    if (buf_a == buf_b) PDEHIP_FAIL(E_VALUE, "euler_run_f32p: the two buffers are the same array");
    if (nsteps < 0) PDEHIP_FAIL(E_VALUE, "euler_run_f32p: negative number of steps");
    PDEHIP_TRY(euler_faces(g, rhs, n, &a));
    set_output(&a, n, PDEHIP_OUT_FULL);
    a.D = (float)rhs->param;
    a.dt = (float)dt;
    hipStream_t s = as_stream(stream);
    const bool force_generic = (rhs->reserved & PDEHIP_RHS_F32P_ONE_STEP) != 0;   // per call: the one-step instance on every grid
    const bool fast = euler_fast(n) && !force_generic && (uintptr_t)buf_a % 16 == 0 && (uintptr_t)buf_b % 16 == 0;
    float *cur = (float *)buf_a, *nxt = (float *)buf_b;
    int64_t left = nsteps;
    if (fast && left >= 2) {
        const int nw = (int)((a.n2 + 255) / 256);
        a.nxc = nw;
        a.nyt = (int)((a.n1 + kF32pRows - 1) / kF32pRows);
        a.seg = choose_segment(a.n0, (long)nw * a.nyt, 4096);
        a.nseg = (int)((a.n0 + a.seg - 1) / a.seg);
        const dim3 grid((unsigned)((long)a.nyt * a.nseg)), block(64 * nw);
        for (; left >= 2; left -= 2) {
            hipLaunchKernelGGL(euler32_kernel, grid, block, 0, s, a, (const float *)cur, nxt);
            float *t = cur; cur = nxt; nxt = t;
        }
        note_kernel("euler32_kernel<two-step,R=%d,waves=%d,seg=%d>", kF32pRows, nw, a.seg);
        PDEHIP_HIP(hipGetLastError());
    }
    if (left > 0) {
        for (; left > 0; left--) {
            launch_generic<true>(g->ndim, a, (const float *)cur, nxt, s);
            float *t = cur; cur = nxt; nxt = t;
        }
        if (!(fast && nsteps >= 2)) note_kernel("euler32_kernel<generic,%d>", g->ndim);
        PDEHIP_HIP(hipGetLastError());
    }
    *result = cur;
    return 0;
}
