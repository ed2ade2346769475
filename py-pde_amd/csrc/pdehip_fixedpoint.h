// pdehip_fixedpoint.h — the fixed-point solvers of the reference (implicit Euler pde/solvers/implicit.py:74-110, Crank-Nicolson
// pde/solvers/crank_nicolson.py:80-113), written ONCE against the evaluator policy of pdehip_rk_loops.h.
//
// A step is `state_t = state`, a first estimate, then iterations `x <- a_prev * x + a_cn * (state_t + c * (rhs(x, t + dt) [+ rate_t]))`
// until mean |x_new - x|^2 < maxerror^2.  Every iteration is ONE sweep where the stage kernels carry the epilogue (StageFuse kind 5:
// update and the wave's share of the norm), else the slope into a scratch array and the pointwise fixedpoint_combine_kernel.  A
// one-workgroup kernel behind it sums the shares in a fixed order, does the stop test ON THE DEVICE and writes the control block
// (FixedPointCtl, pdehip_device.h; the two halves of the sum, wave_sum and sum_slots of pdehip_sweep.h, and the head of the block
// are those of every device-side loop).
//
// The host does not synchronise per iteration: it enqueues a BATCH of iterations - every launch of a batch reads the block's `stop`
// word at entry and returns at once when the step is over - and reads the block back through pinned memory once per batch.  A
// skipped launch writes nothing, so the iteration count names the buffer that holds the result.  Batch size: what the step before
// needed plus one (2 for the first step), or pdehip_fixedpoint_t::batch.  Nothing on the device waits for anything.
//
// Buffers: the state array of the caller and two work arrays rotate as state_t / iterate / iterate (no copy per step).
#pragma once

#include <cstring>

#include "pdehip_slab_loops.h"   // StageFuse, SLAB_TRY

namespace pdehip {

// evaluators return this (nothing of the iteration launched) when the sweep cannot carry the update and no scratch array was given
enum { FP_NEED_SCRATCH = -77 };

// pdehip_fixedpoint.hip
int fixedpoint_init(double *ctl_dev, size_t ctl_bytes, const pdehip_fixedpoint_t *p, double size, void *st);
int fixedpoint_begin(double *ctl_dev, void *st);
int fixedpoint_combine(const pdehip_grid_t *g, int ncomp, const void *prev, const void *k, const void *state_t, const void *rate_t, void *out,
                       double c, double a_prev, double a_cn, double *ctl_dev, void *st);
int fixedpoint_finish(double *ctl_dev, void *st);
int fixedpoint_read(FixedPointCtl *host, const double *ctl_dev, void *st);
int fixedpoint_fail(int code, const char *msg);
void fixedpoint_note(bool fused, const char *sweep = nullptr);   // pdehip_last_kernel_name: the instance the iterations ran on

namespace fp {

template <class Eval>
int run(Eval &ev, const pdehip_grid_t *g, int ncomp, double size, pdehip_fixedpoint_t *p, double dt, double t0, int64_t nsteps, void *state,
        void *const *work, double *ctl_dev, size_t ctl_bytes, void **result, void *st)
{
    if (!p || !state || !work || !ctl_dev || !result || !work[0] || !work[1]) return fixedpoint_fail(1, "fixedpoint_run: NULL pointer");
    if (p->scheme != 0 && p->scheme != 1) return fixedpoint_fail(1, "fixedpoint_run: scheme must be 0 (implicit Euler) or 1 (Crank-Nicolson)");
    if (p->maxiter < 1 || !(p->maxerror2 >= 0) || nsteps < 0 || p->batch < 0) return fixedpoint_fail(1, "fixedpoint_run: bad maxiter / maxerror / step count / batch");
    const bool cn = p->scheme == 1;
    void *rate_t = cn ? work[2] : nullptr, *kscratch = work[3];
    if (cn && !rate_t) return fixedpoint_fail(1, "fixedpoint_run: Crank-Nicolson needs the array of rate_t");
    // implicit.py:95: state_t + dt * rhs;  crank_nicolson.py:99-103: state_t + dt / 2 * (rhs + rate_t), alpha * prev + (1 - alpha) * state_cn
    const double c = cn ? dt / 2 : dt;
    const double a_prev = cn ? p->explicit_fraction : 0.0, a_cn = cn ? 1 - p->explicit_fraction : 1.0;
    p->status = 0;
    SLAB_TRY(fixedpoint_init(ctl_dev, ctl_bytes, p, size, st));
    void *cur = state, *fa = work[0], *fb = work[1];
    bool fused = false;
    // one sweep x -> out of the fixed-point map at the faces of time `t` (the first estimate and every iteration)
    auto sweep = [&](void *x, void *out, void *state_t, double t) -> int {
        StageFuse sf;
        memset(&sf, 0, sizeof(sf));
        sf.kind = 5; sf.y = state_t; sf.k[0] = rate_t; sf.k[1] = x; sf.c[0] = a_prev; sf.c[1] = a_cn; sf.c_new = c; sf.out2 = out; sf.err = ctl_dev;
        SLAB_TRY(ev.slope(x, kscratch, 1.0, t, &sf, &fused, st));
        if (!fused) SLAB_TRY(fixedpoint_combine(g, ncomp, x, kscratch, state_t, rate_t, out, c, a_prev, a_cn, ctl_dev, st));
        return 0;
    };
    FixedPointCtl host;
    memset(&host, 0, sizeof(host));
    for (int64_t s = 0; s < nsteps; s++) {
        const double t = t0 + (double)s * dt;
        void *state_t = cur;
        SLAB_TRY(fixedpoint_begin(ctl_dev, st));
        bool f0 = false;
        if (cn) SLAB_TRY(ev.slope(state_t, rate_t, 1.0, t, nullptr, &f0, st));   // rate_t = rhs(state_t, t)   crank_nicolson.py:85
        // first estimate: implicit Euler at the faces of t (implicit.py:85), Crank-Nicolson at those of t + dt (crank_nicolson.py:88-90)
        {
            const int rc = sweep(state_t, fa, state_t, cn ? t + dt : t);
            if (rc == FP_NEED_SCRATCH) { p->status = 2; *result = cur; return 0; }
            if (rc) return rc;
        }
        p->evaluations += cn ? 2 : 1;
        int enq = 0;
        int batch = p->batch > 0 ? p->batch : (p->last_iterations > 0 ? p->last_iterations + 1 : 2);
        while (true) {
            const int nb = batch < p->maxiter - enq ? batch : p->maxiter - enq;
            for (int b = 0; b < nb; b++, enq++) {
                void *x = (enq % 2 == 0) ? fa : fb, *out = (enq % 2 == 0) ? fb : fa;
                SLAB_TRY(sweep(x, out, state_t, t + dt));
                SLAB_TRY(fixedpoint_finish(ctl_dev, st));
            }
            SLAB_TRY(fixedpoint_read(&host, ctl_dev, st));
            if (host.head.stop) break;
            if (enq >= p->maxiter || host.head.iters != enq) return fixedpoint_fail(3, "internal: the fixed-point control block is out of step with the host");
        }
        p->evaluations += host.head.iters;
        p->err = host.err;
        p->last_iterations = host.head.iters;
        if (p->iterations) p->iterations[s] = host.head.iters;
        if (host.head.failed) {
            if (host.head.failed != 1) return fixedpoint_fail(3, "internal: the partial sums of the fixed-point norm do not fit their buffer");
            p->status = 1;   // maxiter iterations without convergence: the remaining steps are not enqueued
            *result = cur;
            return 0;
        }
        // iteration n wrote fb for odd n, fa for even n; the two other buffers are free again
        void *res = (host.head.iters % 2 == 1) ? fb : fa, *other = (host.head.iters % 2 == 1) ? fa : fb;
        fa = other; fb = cur; cur = res;
        p->steps_done++;
    }
    p->fused = fused ? 1 : 0;
    if (nsteps > 0) fixedpoint_note(fused, ev.sweep_name());
    *result = cur;
    return 0;
}

}  // namespace fp
}  // namespace pdehip
