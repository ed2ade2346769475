// pdehip_poisson.hip — Poisson's and Laplace's equation on the device by conjugate gradients (see pdehip_poisson.h): the handle, the
// one-workgroup kernel behind every sweep 1 (both dot products in a fixed order, alpha / beta, stop test), the pointwise sweep 2, the
// start (right-hand side of the split system, projection of singular systems) and the end (mean of x, the reference's `allclose` test).
#include "pdehip_poisson_mg.h"

namespace pdehip {

namespace {

// interior cell (i, j, k) in the fp64 work layout and in the layout of the caller's field
struct PGrid {
    long n0, n1, n2;
    long p0, p1, off;      // work vectors
    long fp0, fp1, foff;   // field arrays (equal to the above for fp64 fields)
};

PGrid make_pgrid(const NGrid &n64, const NGrid &nf)
{
    PGrid g;
    g.n0 = n64.n[0]; g.n1 = n64.n[1]; g.n2 = n64.n[2];
    g.p0 = n64.p[0]; g.p1 = n64.p[1]; g.off = n64.off;
    g.fp0 = nf.p[0]; g.fp1 = nf.p[1]; g.foff = nf.off;
    return g;
}

// cells in a grid-stride loop, one per thread and turn: fn(offset in a work vector, offset in a field array)
template <class F>
__device__ __forceinline__ void for_cells(const PGrid &g, F &&fn)
{
    const long total = g.n0 * g.n1 * g.n2;
    for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        long r = t;
        const long k = r % g.n2; r /= g.n2;
        const long j = r % g.n1;
        const long i = r / g.n1;
        fn(g.off + i * g.p0 + j * g.p1 + k, g.foff + i * g.fp0 + j * g.fp1 + k);
    }
}
__device__ __forceinline__ int wave_slot() { return (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); }

// start of a solve: parameters of the stop test, counters
__global__ void poisson_init_kernel(PoissonCtl *c, int maxiter, double rtol, double atol, double size, int capacity)
{
    c->rr = 0; c->rw = 0; c->iters = 0; c->converged = 0; c->failed = 0; c->stop = 0; c->nslots = 0; c->maxiter = maxiter;
    c->alpha = 0; c->beta = 0; c->capacity = capacity; c->reserved = 0; c->bnorm = 0; c->tol = 0; c->rtol = rtol; c->atol = atol;
    c->mean = 0; c->size = size; c->count = 0; c->resid2 = 0;
}

// r = v - f: the right-hand side of (-A) u = -(f - v) and, x = 0, the first residual (common.py:104 `rhs = np.ravel(arr) - vec`);
// every wave's share of its sum goes to the first of its two slots (singular systems subtract the mean)
template <typename T>
__global__ void __launch_bounds__(256) poisson_rhs_kernel(PGrid g, const T *f, const double *v, double *r, double *ctl)
{
    fixedpoint_announce(ctl, (long)gridDim.x * (blockDim.x >> 6));
    double s = 0;
    for_cells(g, [&](long e, long ef) {
        const double b = v[e] - (double)f[ef];
        r[e] = b;
        s = s + b;
    });
    poisson_wave_partial(ctl, s, 0.0, wave_slot());
}

// every wave's share of the sum of x (singular systems: the minimum-norm solution has mean zero)
__global__ void __launch_bounds__(256) poisson_sum_kernel(PGrid g, const double *x, double *ctl)
{
    fixedpoint_announce(ctl, (long)gridDim.x * (blockDim.x >> 6));
    double s = 0;
    for_cells(g, [&](long e, long) { s = s + x[e]; });
    poisson_wave_partial(ctl, s, 0.0, wave_slot());
}

__global__ void __launch_bounds__(256) poisson_shift_kernel(PGrid g, double *x, const double *ctl)
{
    const double m = ((const PoissonCtl *)ctl)->mean;
    for_cells(g, [&](long e, long) { x[e] = x[e] - m; });
}

// The reference's acceptance test of a least-squares solution (common.py:134 `np.allclose(mat.dot(result), rhs, rtol=1e-5, atol=1e-5)`)
// against the UNPROJECTED right-hand side b = f - v: w = -A x, so A x - b = -w - (f - v).  Shares of the count of violating cells
// (a NaN violates) and of |A x - b|^2 (common.py:135).
template <typename T>
__global__ void __launch_bounds__(256) poisson_check_kernel(PGrid g, const T *f, const double *v, const double *w, double *ctl)
{
    fixedpoint_announce(ctl, (long)gridDim.x * (blockDim.x >> 6));
    double cnt = 0, res = 0;
    for_cells(g, [&](long e, long ef) {
        const double b = (double)f[ef] - v[e];
        const double d = -w[e] - b;
        if (!(fabs(d) <= 1e-5 + 1e-5 * fabs(b))) cnt = cnt + 1.0;
        res = res + d * d;
    });
    poisson_wave_partial(ctl, cnt, res, wave_slot());
}

template <typename T>
__global__ void __launch_bounds__(256) poisson_store_kernel(PGrid g, const double *x, T *out)
{
    for_cells(g, [&](long e, long ef) { out[ef] = (T)x[e]; });
}

// ONE workgroup: thread i adds the slots i, i + 256, ... in that order, then a tree over the 256 sums in LDS - the same order in every
// run (fixedpoint_finish_kernel).  Both columns of the slots at once; the sums end in s0, s1 of thread 0.
__device__ __forceinline__ void sum_slots(const double *ctl, int n, double &s0, double &s1)
{
    __shared__ double part[2][256];
    s0 = 0; s1 = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        s0 = s0 + ctl[kPoissonSlots + 2 * i];
        s1 = s1 + ctl[kPoissonSlots + 2 * i + 1];
    }
    part[0][threadIdx.x] = s0;
    part[1][threadIdx.x] = s1;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if ((int)threadIdx.x < w) {
            part[0][threadIdx.x] = part[0][threadIdx.x] + part[0][threadIdx.x + w];
            part[1][threadIdx.x] = part[1][threadIdx.x] + part[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    s0 = part[0][0];
    s1 = part[1][0];
}

// what = 0: mean = first sum / cells;  1: count = first sum, resid2 = second sum
__global__ void __launch_bounds__(256) poisson_reduce_kernel(double *ctl, int what)
{
    PoissonCtl *c = (PoissonCtl *)ctl;
    const int n = c->nslots < c->capacity ? c->nslots : c->capacity;
    double s0, s1;
    sum_slots(ctl, n, s0, s1);
    if (threadIdx.x == 0) {
        if (what == 0) c->mean = s0 / c->size;
        else { c->count = s0; c->resid2 = s1; }
    }
}

// Behind sweep 1 of iteration k: gamma = r.r, delta = r.w (w = -A r), the stop test on r, and the step lengths of the update that
// follows (Chronopoulos-Gear): beta = gamma / gamma_prev, alpha = gamma / (delta - beta * gamma / alpha_prev); beta = 0 for k = 0.
// The denominator is p.q of the direction the update builds: <= 0 means the system is not definite (or rounding has eaten it).
__global__ void __launch_bounds__(256) poisson_finish_kernel(double *ctl)
{
    PoissonCtl *c = (PoissonCtl *)ctl;
    if (c->stop) return;   // uniform
    const int n = c->nslots < c->capacity ? c->nslots : c->capacity;
    double gamma, delta;
    sum_slots(ctl, n, gamma, delta);
    if (threadIdx.x != 0) return;
    const double gamma_prev = c->rr, alpha_prev = c->alpha;
    c->rr = gamma;
    c->rw = delta;
    if (c->nslots > c->capacity) { c->failed = 4; c->stop = 1; return; }   // (never: the buffer is sized for any launch geometry)
    if (c->iters == 0) {
        c->bnorm = sqrt(gamma);
        const double t = c->rtol * c->bnorm;
        c->tol = t > c->atol ? t : c->atol;
    }
    if (!isfinite(gamma) || !isfinite(delta)) { c->failed = 2; c->stop = 1; return; }
    if (sqrt(gamma) <= c->tol) { c->converged = 1; c->stop = 1; return; }
    if (c->iters >= c->maxiter) { c->failed = 1; c->stop = 1; return; }
    double beta = 0, denom = delta;
    if (c->iters > 0) {
        beta = gamma / gamma_prev;
        denom = delta - beta * gamma / alpha_prev;
    }
    if (!(delta > 0) || !(denom > 0)) { c->failed = 3; c->stop = 1; return; }
    c->alpha = gamma / denom;
    c->beta = beta;
    c->iters = c->iters + 1;
}

// sweep 1: w = -A r and the wave's shares of r.r and r.w.  The ghost cells of r hold the homogeneous conditions (ghost kernel in front
// of this launch).  A thread takes VEC cells of a row (16-byte accesses where the row length is even), rows in a grid-stride loop: a
// fixed order per thread.  The Laplacian in the reference's order (pde/backends/numba/operators/cartesian.py:112-116, :147-151,
// :220-227); the neighbouring rows and planes come out of the caches (the launch walks the planes in order).
template <int VEC>
__global__ void __launch_bounds__(256) poisson_apply_kernel(PGrid g, int ndim, double sx, double sy, double sz, const double *r, double *w, double *ctl)
{
    if (fixedpoint_stopped(ctl)) return;   // uniform
    fixedpoint_announce(ctl, (long)gridDim.x * (blockDim.x >> 6));
    typedef double V __attribute__((ext_vector_type(VEC)));
    const long per_row = g.n2 / VEC;
    const long total = g.n0 * g.n1 * per_row;
    double s_rr = 0, s_rw = 0;
    for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        long rest = t;
        const long k = (rest % per_row) * VEC; rest /= per_row;
        const long j = rest % g.n1;
        const long i = rest / g.n1;
        const long e = g.off + i * g.p0 + j * g.p1 + k;
        const V c = *(const V *)(r + e);
        const double left = r[e - 1], right = r[e + VEC];
        V up, dn, xm, xp;
        if (ndim >= 2) { up = *(const V *)(r + e - g.p1); dn = *(const V *)(r + e + g.p1); }
        if (ndim == 3) { xm = *(const V *)(r + e - g.p0); xp = *(const V *)(r + e + g.p0); }
        V wv;
#pragma unroll
        for (int m = 0; m < VEC; m++) {
            const double cen = c[m], vm = 2 * cen;
            const double zl = (m == 0) ? left : (double)c[m > 0 ? m - 1 : 0], zr = (m == VEC - 1) ? right : (double)c[m < VEC - 1 ? m + 1 : m];
            const double lz = (zl - vm + zr) * sz;
            double lap = lz;
            if (ndim == 2) lap = (up[m] - vm + dn[m]) * sy + lz;
            if (ndim == 3) lap = (xm[m] - vm + xp[m]) * sx + (up[m] - vm + dn[m]) * sy + lz;
            const double wn = -lap;
            wv[m] = wn;
            s_rr = s_rr + cen * cen;
            s_rw = s_rw + cen * wn;
        }
        *(V *)(w + e) = wv;
    }
    poisson_wave_partial(ctl, s_rr, s_rw, wave_slot());
}

// sweep 2: p = r + beta p, q = w + beta q, x += alpha p, r -= alpha q with alpha, beta from the control block (two uniform loads).
// A thread takes VEC cells of a row (16-byte accesses where the row length is even); rows in a grid-stride loop.
template <int VEC>
__global__ void __launch_bounds__(256) poisson_update_kernel(PGrid g, double *x, double *r, double *p, double *q, const double *w, const double *ctl)
{
    const PoissonCtl *c = (const PoissonCtl *)ctl;
    if (c->stop) return;   // uniform
    const double alpha = c->alpha, beta = c->beta;
    typedef double V __attribute__((ext_vector_type(VEC)));
    const long per_row = g.n2 / VEC;
    const long total = g.n0 * g.n1 * per_row;
    for (long t = blockIdx.x * (long)blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        long rest = t;
        const long k = (rest % per_row) * VEC; rest /= per_row;
        const long j = rest % g.n1;
        const long i = rest / g.n1;
        const long e = g.off + i * g.p0 + j * g.p1 + k;
        const V rv = *(const V *)(r + e), wv = *(const V *)(w + e);
        V pv = *(const V *)(p + e), qv = *(const V *)(q + e), xv = *(const V *)(x + e);
        V rn;
#pragma unroll
        for (int m = 0; m < VEC; m++) {
            pv[m] = rv[m] + beta * pv[m];
            qv[m] = wv[m] + beta * qv[m];
            xv[m] = xv[m] + alpha * pv[m];
            rn[m] = rv[m] - alpha * qv[m];
        }
        *(V *)(p + e) = pv;
        *(V *)(q + e) = qv;
        *(V *)(x + e) = xv;
        *(V *)(r + e) = rn;
    }
}

unsigned blocks_for(long items)
{
    long b = (items + 255) / 256;
    if (b < 1) b = 1;
    if (b > 8192) b = 8192;   // at most 32768 waves: what the slots always hold
    return (unsigned)b;
}

const char *face_name(int q, char *buf, size_t len)
{
    snprintf(buf, len, "%s face of axis %d", (q & 1) ? "upper" : "lower", q / 2);
    return buf;
}

int poisson_read(PoissonHandle *h, PoissonCtl *host, void *st)
{
    PDEHIP_HIP(hipMemcpyAsync(h->pinned, h->ctl, sizeof(PoissonCtl), hipMemcpyDeviceToHost, as_stream(st)));
    PDEHIP_HIP(hipStreamSynchronize(as_stream(st)));
    *host = *h->pinned;
    return 0;
}

void poisson_release(PoissonHandle *h)
{
    if (!h) return;
    poisson_mg_release(h);
    void *dev[] = {h->zero_face, h->x, h->r, h->p, h->q, h->w, h->ctl};
    for (void *d : dev)
        if (d) (void)hipFree(d);
    if (h->pinned) (void)hipHostFree(h->pinned);
    delete h;
}

// sweep 1: the homogeneous conditions into the ghost cells of r (they are written even when the solve is over: nothing reads them
// afterwards), then w = -A r with the shares of r.r and r.w
int poisson_sweep1(PoissonHandle *h, void *st)
{
    const NGrid &n = h->n64;
    PDEHIP_TRY(launch_ghosts(n, 1, h->faces_a, h->r, as_stream(st)));
    const PGrid pg = make_pgrid(n, n);
    const long cells = pg.n0 * pg.n1 * pg.n2;
    if (pg.n2 % 2 == 0) hipLaunchKernelGGL((poisson_apply_kernel<2>), dim3(blocks_for(cells / 2)), dim3(256), 0, as_stream(st), pg, n.ndim, n.lap_scale[0], n.lap_scale[1], n.lap_scale[2], h->r, h->w, h->ctl);
    else hipLaunchKernelGGL((poisson_apply_kernel<1>), dim3(blocks_for(cells)), dim3(256), 0, as_stream(st), pg, n.ndim, n.lap_scale[0], n.lap_scale[1], n.lap_scale[2], h->r, h->w, h->ctl);
    PDEHIP_HIP(hipGetLastError());
    return 0;
}

int poisson_sweep2(PoissonHandle *h, void *st)
{
    const PGrid pg = make_pgrid(h->n64, h->n64);
    const long cells = pg.n0 * pg.n1 * pg.n2;
    if (pg.n2 % 2 == 0) hipLaunchKernelGGL((poisson_update_kernel<2>), dim3(blocks_for(cells / 2)), dim3(256), 0, as_stream(st), pg, h->x, h->r, h->p, h->q, h->w, h->ctl);
    else hipLaunchKernelGGL((poisson_update_kernel<1>), dim3(blocks_for(cells)), dim3(256), 0, as_stream(st), pg, h->x, h->r, h->p, h->q, h->w, h->ctl);
    PDEHIP_HIP(hipGetLastError());
    return 0;
}

template <typename T>
int poisson_solve_t(PoissonHandle *h, const T *rhs, T *out, pdehip_poisson_t *io, void *st)
{
    hipStream_t s = as_stream(st);
    const PGrid pg = make_pgrid(h->n64, h->nf);
    const long cells = pg.n0 * pg.n1 * pg.n2;
    const unsigned nb = blocks_for(cells);
    double *ctl = h->ctl;
    // x = 0 (ghost cells and padding too), p = q = 0;  w = v = L(0) with the faces as given (cartesian.py `vector`)
    PDEHIP_HIP(hipMemsetAsync(h->x, 0, h->vec_bytes, s));
    PDEHIP_HIP(hipMemsetAsync(h->p, 0, h->vec_bytes, s));
    PDEHIP_HIP(hipMemsetAsync(h->q, 0, h->vec_bytes, s));
    PDEHIP_TRY(laplace_with_input_bcs(&h->g64, h->x, nullptr, h->w, LAP_PLAIN, 0, 0, 0, h->faces, st));
    hipLaunchKernelGGL(poisson_init_kernel, dim3(1), dim3(1), 0, s, (PoissonCtl *)ctl, io->maxiter, io->rtol, io->atol, (double)cells, h->capacity);
    hipLaunchKernelGGL((poisson_rhs_kernel<T>), dim3(nb), dim3(256), 0, s, pg, rhs, h->w, h->r, ctl);
    if (h->singular) {
        // the constants span the null space of A: project them out of b; the iterates from x = 0 then stay orthogonal to them
        hipLaunchKernelGGL(poisson_reduce_kernel, dim3(1), dim3(256), 0, s, ctl, 0);
        hipLaunchKernelGGL(poisson_shift_kernel, dim3(nb), dim3(256), 0, s, pg, h->r, ctl);
    }
    PDEHIP_HIP(hipGetLastError());
    PoissonCtl host;
    memset(&host, 0, sizeof(host));
    const int batch = io->batch > 0 ? io->batch : 32;
    // iteration k = sweep 1, the one-workgroup kernel, sweep 2; the test of the last update needs one more sweep 1
    long enq = 0;
    const long most = (long)io->maxiter + 1;
    while (true) {
        const long nbatch = batch < most - enq ? batch : most - enq;
        for (long b = 0; b < nbatch; b++, enq++) {
            if (h->mg) { PDEHIP_TRY(poisson_mg_iteration(h, st)); continue; }   // the preconditioned loop: same control block, same stop rule
            PDEHIP_TRY(poisson_sweep1(h, st));
            hipLaunchKernelGGL(poisson_finish_kernel, dim3(1), dim3(256), 0, s, ctl);
            PDEHIP_TRY(poisson_sweep2(h, st));
        }
        PDEHIP_TRY(poisson_read(h, &host, st));
        if (host.stop) break;
        if (enq >= most || host.iters != enq) PDEHIP_FAIL(E_RUNTIME, "internal: the control block of the Poisson solver is out of step with the host");
    }
    if (host.failed == 4) PDEHIP_FAIL(E_RUNTIME, "internal: the partial sums of the Poisson solver do not fit their buffer");
    io->iterations = host.iters;
    io->residual = sqrt(host.rr);
    io->rhs_norm = host.bnorm;
    io->status = host.failed;   // 0 converged, 1 maxiter, 2 non-finite, 3 breakdown
    io->check_residual = 0;
    if (h->singular && host.converged) {
        // the minimum-norm solution (what the reference's lsmr returns): mean zero ...
        hipLaunchKernelGGL(poisson_sum_kernel, dim3(nb), dim3(256), 0, s, pg, h->x, ctl);
        hipLaunchKernelGGL(poisson_reduce_kernel, dim3(1), dim3(256), 0, s, ctl, 0);
        hipLaunchKernelGGL(poisson_shift_kernel, dim3(nb), dim3(256), 0, s, pg, h->x, ctl);
        PDEHIP_HIP(hipGetLastError());
        // ... and the reference's test of it against the right-hand side as given: w = -A x, q = v = L(0) once more (p = 0)
        PDEHIP_TRY(laplace_with_input_bcs(&h->g64, h->x, nullptr, h->w, LAP_SCALED, -1.0, 1.0, 0, h->faces_a, st));
        PDEHIP_HIP(hipMemsetAsync(h->p, 0, h->vec_bytes, s));
        PDEHIP_TRY(laplace_with_input_bcs(&h->g64, h->p, nullptr, h->q, LAP_PLAIN, 0, 0, 0, h->faces, st));
        hipLaunchKernelGGL((poisson_check_kernel<T>), dim3(nb), dim3(256), 0, s, pg, rhs, h->q, h->w, ctl);
        hipLaunchKernelGGL(poisson_reduce_kernel, dim3(1), dim3(256), 0, s, ctl, 1);
        PDEHIP_HIP(hipGetLastError());
        PDEHIP_TRY(poisson_read(h, &host, st));
        io->check_residual = sqrt(host.resid2);
        if (host.count != 0) io->status = 4;
    }
    hipLaunchKernelGGL((poisson_store_kernel<T>), dim3(nb), dim3(256), 0, s, pg, h->x, out);
    PDEHIP_HIP(hipGetLastError());
    if (h->mg) poisson_mg_note(h);
    else note_kernel("poisson_apply_kernel<%d> (w = -A r with the wave sums of r.r and r.w in the sweep)", pg.n2 % 2 == 0 ? 2 : 1);
    return 0;
}

}  // namespace

}  // namespace pdehip

using namespace pdehip;

extern "C" {

int pdehip_poisson_create(const pdehip_grid_t *g, const pdehip_bc_face_t *faces, void **handle)
{
    if (!g || !faces || !handle) PDEHIP_FAIL(E_VALUE, "poisson_create: NULL pointer");
    *handle = nullptr;
    PoissonHandle *h = new PoissonHandle();
    h->g = *g;
    h->g64 = *g;
    h->g64.dtype = PDEHIP_F64;
    int rc = norm_grid(&h->g, &h->nf);
    if (!rc) rc = norm_grid(&h->g64, &h->n64);
    if (rc) { delete h; return rc; }
    const NGrid &n = h->n64;
    // Which conditions: first-order faces that take the virtual point from the adjacent cell (they only touch the diagonal of the matrix)
    // or from the other end of the axis on both of its sides (periodic: a symmetric link)
    long max_face = 1;
    bool singular = true, arrays = false;
    char nm[64];
    for (int a = 0; a < PDEHIP_MAX_DIM; a++)
        for (int side = 0; side < 2; side++) {
            const int q = 2 * a + side;
            memset(&h->faces[q], 0, sizeof(h->faces[q]));
            memset(&h->faces_a[q], 0, sizeof(h->faces_a[q]));
            if (a >= n.ndim) continue;
            const pdehip_bc_face_t &f = faces[q];
            const long len = n.n[3 - n.ndim + a];
            auto refuse = [&](const char *why) {
                char buf[400];
                snprintf(buf, sizeof(buf), "poisson_solver: the %s %s", face_name(q, nm, sizeof(nm)), why);
                set_error(buf);
                delete h;
                return (int)E_NOTIMPL;
            };
            if (f.kind == PDEHIP_BC_ORDER2) return refuse("is a second-order condition (it reads a second cell, `index2`): the matrix is not symmetric and conjugate gradients do not apply");
            if (f.kind != PDEHIP_BC_ORDER1) return refuse("carries no condition the solver can put into its matrix (kind SKIP: ghost cells set by the caller)");
            if (f.flags & PDEHIP_BCF_NORMAL) return refuse("is a condition on the normal component of a vector field: the solver takes scalar fields");
            const long adjacent = side ? len - 1 : 0, wrapped = side ? 0 : len - 1;
            if (f.index1 != adjacent && f.index1 != wrapped) return refuse("takes its virtual point from a cell that is neither adjacent nor periodic");
            if (f.index1 == wrapped && len > 1) {
                const pdehip_bc_face_t &o = faces[2 * a + (1 - side)];
                const bool per = !(f.flags & PDEHIP_BCF_ARRAYS) && f.const_v == 0 && f.factor1 == 1 && o.kind == PDEHIP_BC_ORDER1 && !(o.flags & PDEHIP_BCF_ARRAYS) &&
                                 o.index1 == (side ? len - 1 : 0) && o.const_v == 0 && o.factor1 == 1;
                if (!per) return refuse("links the two ends of its axis without being periodic: the matrix is not symmetric");
            }
            h->faces[q] = f;
            h->faces_a[q] = f;
            h->faces_a[q].const_v = 0;
            if (f.flags & PDEHIP_BCF_ARRAYS) {
                if (!f.const_arr || !f.factor1_arr) { set_error("poisson_create: BC arrays missing"); delete h; return E_VALUE; }
                long cells = 1;
                for (int b = 0; b < n.ndim; b++)
                    if (b != a) cells *= n.n[3 - n.ndim + b];
                if (cells > max_face) max_face = cells;
                arrays = true;
                // singular only if every factor of the face is exactly one: read the array once
                double *host = (double *)malloc((size_t)cells * sizeof(double));
                bool ones = host != nullptr;
                if (host && hipMemcpy(host, f.factor1_arr, (size_t)cells * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess) {
                    for (long m = 0; m < cells && ones; m++) ones = host[m] == 1.0;
                } else {
                    ones = false;
                }
                free(host);
                singular = singular && ones;
            } else {
                singular = singular && f.factor1 == 1.0;
            }
        }
    h->singular = singular;
    h->vec_bytes = (size_t)(n.pc + kAllocSlack) * sizeof(double);
    // one pair of slots per wave of the sweep that writes them (the bound of pdehip_fixedpoint_ctl_bytes)
    const size_t waves = (size_t)n.n[0] * (size_t)(n.n[1] + 16) * (size_t)(n.n[2] / 64 + 1);
    const size_t slots = waves > 32768 ? waves : 32768;
    h->capacity = (int)(slots > 0x3fffffff ? 0x3fffffff : slots);
    const size_t ctl_bytes = (kPoissonSlots + 2 * (size_t)h->capacity) * sizeof(double);
    double **vecs[] = {&h->x, &h->r, &h->p, &h->q, &h->w};
    hipError_t e = hipSuccess;
    for (double **v : vecs) {
        if (e == hipSuccess) e = hipMalloc((void **)v, h->vec_bytes);
        if (e == hipSuccess) e = hipMemset(*v, 0, h->vec_bytes);
    }
    if (e == hipSuccess) e = hipMalloc((void **)&h->ctl, ctl_bytes);
    if (e == hipSuccess) e = hipMemset(h->ctl, 0, ctl_bytes);
    if (e == hipSuccess) e = hipHostMalloc((void **)&h->pinned, sizeof(PoissonCtl), hipHostMallocDefault);
    if (e == hipSuccess && arrays) {
        e = hipMalloc((void **)&h->zero_face, (size_t)max_face * sizeof(double));
        if (e == hipSuccess) e = hipMemset(h->zero_face, 0, (size_t)max_face * sizeof(double));
        for (int q = 0; q < 2 * n.ndim; q++)
            if (h->faces_a[q].flags & PDEHIP_BCF_ARRAYS) h->faces_a[q].const_arr = h->zero_face;
    }
    if (e != hipSuccess) {
        poisson_release(h);
        PDEHIP_FAIL(100 + (int)e, "poisson_create: %s", hipGetErrorString(e));
    }
    *handle = h;
    return 0;
}

int pdehip_poisson_solve(void *handle, const void *rhs_full, void *out_full, pdehip_poisson_t *io, void *stream)
{
    PoissonHandle *h = (PoissonHandle *)handle;
    if (!h || !rhs_full || !out_full || !io) PDEHIP_FAIL(E_VALUE, "poisson_solve: NULL pointer");
    if (io->maxiter < 1 || !(io->rtol >= 0) || !(io->atol >= 0) || io->batch < 0) PDEHIP_FAIL(E_VALUE, "poisson_solve: bad rtol / atol / maxiter / batch");
    io->singular = h->singular ? 1 : 0;
    io->reserved = 0;
    if (h->g.dtype == PDEHIP_F64) return poisson_solve_t<double>(h, (const double *)rhs_full, (double *)out_full, io, stream);
    return poisson_solve_t<float>(h, (const float *)rhs_full, (float *)out_full, io, stream);
}

int pdehip_poisson_destroy(void *handle)
{
    poisson_release((PoissonHandle *)handle);
    return 0;
}

}  // extern "C"
