// pdehip_fixedpoint.hip — what the fixed-point solvers (pdehip_fixedpoint.h) need besides the stage sweeps: the control block's kernels
// (start of a call, start of a step, final sum + stop test), the pointwise form of the iteration for right-hand sides whose sweep
// cannot carry it, and the read-back through pinned memory.
#include "pdehip_sweep.h"
#include "pdehip_fixedpoint.h"

namespace pdehip {

namespace {

// start of a call: parameters of the stop test, counters of the call
__global__ void fixedpoint_init_kernel(FixedPointCtl *c, int maxiter, double maxerr2, double size, int capacity)
{
    c->head = CtlHead{0, 0, capacity, 0, 0, 0, maxiter, 0};
    c->err = 0; c->evals = 0; c->maxerr2 = maxerr2; c->size = size;
}

// start of a step (after a failed step nothing runs any more: `stop` stays)
__global__ void fixedpoint_begin_kernel(FixedPointCtl *c)
{
    if (c->head.failed) return;
    c->head.iters = 0; c->head.converged = 0; c->head.stop = 0;
}

// The final sum of an iteration (sum_slots: one workgroup, a fixed order) and its stop test (implicit.py:99-104,
// crank_nicolson.py:105-110: `err / state.size < maxerror**2`).
__global__ void __launch_bounds__(256) fixedpoint_finish_kernel(FixedPointCtl *c)
{
    CtlHead &h = c->head;
    if (h.stop) return;   // uniform
    double sum[1];
    sum_slots<1>((const double *)c + kFixedPointSlots, ctl_nslots(h), sum);
    if (threadIdx.x == 0) {
        const double err = sum[0] / c->size;
        c->err = err;
        h.iters = h.iters + 1;
        c->evals = c->evals + 1;
        if (h.nslots > h.capacity) { h.failed = 2; h.stop = 1; }   // (never: the buffer is sized for any launch geometry)
        else if (err < c->maxerr2) { h.converged = 1; h.stop = 1; }   // false for NaN, like the reference
        else if (h.iters >= h.maxiter) { h.failed = 1; h.stop = 1; }
    }
}

struct CombineArgs {
    RowGrid g;
    long pc;   // elements between two components
    int ncomp;
    const void *prev, *k, *state_t, *rate_t;
    void *out;
    double c, a_prev, a_cn;
    double *ctl;
};

// The iteration's update and norm as a pointwise pass (k = rhs(prev) comes from a sweep of its own): the same expressions in the same
// order as st_kind 5 of the stage sweeps (pdehip_march.inc), so both forms give the same bits.  Cells per thread in a grid-stride
// loop: a fixed order per thread; block sum in a fixed order; one slot per WAVE slot of the launch like the sweeps.
template <typename T>
__global__ void __launch_bounds__(256) fixedpoint_combine_kernel(CombineArgs a)
{
    if (fixedpoint_stopped(a.ctl)) return;
    fixedpoint_announce(a.ctl, (long)gridDim.x * (blockDim.x >> 6));
    const long total = (long)a.ncomp * a.g.n0 * a.g.n1 * a.g.n2;
    double esum = 0;
    for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        long r = t;
        const long kk = r % a.g.n2; r /= a.g.n2;
        const long j = r % a.g.n1; r /= a.g.n1;
        const long i = r % a.g.n0;
        const long comp = r / a.g.n0;
        const long e = comp * a.pc + a.g.off + i * a.g.p0 + j * a.g.p1 + kk;
        const double pv = (double)((const T *)a.prev)[e], kn = (double)((const T *)a.k)[e], yv = (double)((const T *)a.state_t)[e];
        double nv;
        if (!a.rate_t) {
            nv = yv + a.c * kn;                                           // implicit.py:95
        } else {
            const double cn = yv + a.c * (kn + (double)((const T *)a.rate_t)[e]);   // crank_nicolson.py:99-101
            nv = a.a_prev * pv + a.a_cn * cn;                             // crank_nicolson.py:103
        }
        const T o = (T)nv;
        ((T *)a.out)[e] = o;
        const double df = (double)o - pv;
        esum = esum + df * df;
    }
    fixedpoint_wave_partial(a.ctl, esum, wave_slot());
}

thread_local FixedPointCtl *g_pinned = nullptr;

}  // namespace

int fixedpoint_fail(int code, const char *msg) { PDEHIP_FAIL(code, "%s", msg); }

int fixedpoint_init(double *ctl_dev, size_t ctl_bytes, const pdehip_fixedpoint_t *p, double size, void *st)
{
    if (ctl_bytes < (kFixedPointSlots + 64) * sizeof(double) || (uintptr_t)ctl_dev % 8 != 0) PDEHIP_FAIL(E_VALUE, "fixedpoint_run: the control block is too small (pdehip_fixedpoint_ctl_bytes) or misaligned");
    const size_t cap = ctl_bytes / sizeof(double) - kFixedPointSlots;
    hipLaunchKernelGGL(fixedpoint_init_kernel, dim3(1), dim3(1), 0, as_stream(st), (FixedPointCtl *)ctl_dev, p->maxiter, p->maxerror2, size,
                       (int)(cap > 0x7fffffff ? 0x7fffffff : cap));
    PDEHIP_HIP(hipGetLastError());
    return 0;
}

int fixedpoint_begin(double *ctl_dev, void *st)
{
    hipLaunchKernelGGL(fixedpoint_begin_kernel, dim3(1), dim3(1), 0, as_stream(st), (FixedPointCtl *)ctl_dev);
    PDEHIP_HIP(hipGetLastError());
    return 0;
}

int fixedpoint_finish(double *ctl_dev, void *st)
{
    hipLaunchKernelGGL(fixedpoint_finish_kernel, dim3(1), dim3(256), 0, as_stream(st), (FixedPointCtl *)ctl_dev);
    PDEHIP_HIP(hipGetLastError());
    return 0;
}

int fixedpoint_combine(const pdehip_grid_t *g, int ncomp, const void *prev, const void *k, const void *state_t, const void *rate_t, void *out,
                       double c, double a_prev, double a_cn, double *ctl_dev, void *st)
{
    NGrid n;
    PDEHIP_TRY(norm_grid(g, &n));
    if (!prev || !k || !state_t || !out || !ctl_dev || ncomp < 1) PDEHIP_FAIL(E_VALUE, "fixedpoint_combine: NULL pointer");
    CombineArgs a;
    a.g = make_row_grid(n); a.pc = n.pc;
    a.ncomp = ncomp; a.prev = prev; a.k = k; a.state_t = state_t; a.rate_t = rate_t; a.out = out; a.c = c; a.a_prev = a_prev; a.a_cn = a_cn; a.ctl = ctl_dev;
    const long items = (long)ncomp * n.n[0] * n.n[1] * n.n[2];
    const unsigned blocks = blocks_for((items + 3) / 4);   // four cells per thread
    if (n.dtype == PDEHIP_F64) hipLaunchKernelGGL((fixedpoint_combine_kernel<double>), dim3(blocks), dim3(256), 0, as_stream(st), a);
    else hipLaunchKernelGGL((fixedpoint_combine_kernel<float>), dim3(blocks), dim3(256), 0, as_stream(st), a);
    PDEHIP_HIP(hipGetLastError());
    return 0;
}

int fixedpoint_read(FixedPointCtl *host, const double *ctl_dev, void *st)
{
    if (!g_pinned) PDEHIP_HIP(hipHostMalloc((void **)&g_pinned, sizeof(FixedPointCtl), hipHostMallocDefault));
    return read_ctl(host, g_pinned, ctl_dev, sizeof(FixedPointCtl), st);
}

void fixedpoint_note(bool fused, const char *sweep)
{
    if (!fused) { note_kernel("fixedpoint_combine_kernel (slope sweep + pointwise fixed-point update with the convergence norm)"); return; }
    char last[192];
    snprintf(last, sizeof(last), "%s", sweep ? sweep : pdehip_last_kernel_name());
    char *fm = strstr(last, " [fastmath");   // (note_kernel appends it again)
    if (fm) *fm = 0;
    note_kernel("%.120s + fixed-point epilogue (st_kind 5: update and convergence norm in the sweep)", last);
}

}  // namespace pdehip

using namespace pdehip;

extern "C" {

int pdehip_fixedpoint_ctl_bytes(const pdehip_grid_t *g, int ncomp, size_t *bytes)
{
    NGrid n;
    PDEHIP_TRY(norm_grid(g, &n));
    if (!bytes || ncomp < 1) PDEHIP_FAIL(E_VALUE, "fixedpoint_ctl_bytes: NULL pointer");
    // one slot per wave of the sweep that writes them: a wave owns at least one piece of 64 cells of one row over one or more planes,
    // a workgroup has at most 16 waves stacked along the rows (idle ones included); the pointwise form launches at most kSweepWavesMax
    const size_t waves = (size_t)n.n[0] * (size_t)(n.n[1] + 16) * (size_t)(n.n[2] / 64 + 1);
    const size_t slots = waves > (size_t)kSweepWavesMax ? waves : (size_t)kSweepWavesMax;
    *bytes = (kFixedPointSlots + slots) * sizeof(double);
    return 0;
}

}  // extern "C"
