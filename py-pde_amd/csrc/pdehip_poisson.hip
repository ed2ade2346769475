// pdehip_poisson.hip — Poisson's and Laplace's equation on the device by conjugate gradients (see pdehip_poisson.h): the handle, the
// one-workgroup kernel behind every sweep 1 (the dot products in a fixed order, alpha / beta, stop test) and the pointwise sweep 2 of
// the plain and the preconditioned loop, the start (right-hand side of the split system, projection of singular systems) and the end
// (mean of x, the reference's `allclose` test).
#include "pdehip_poisson_mg.h"

namespace pdehip {

namespace {

// the fp64 work vectors and the caller's field arrays (the same layout for fp64 fields)
struct PGrid { RowGrid work, field; };

// cells in a grid-stride loop, one per thread and turn: fn(offset in a work vector, offset in a field array)
template <class F>
__device__ __forceinline__ void for_cells(const PGrid &g, F &&fn)
{
    for_row_pieces<1>(g.work, [&](long i, long j, long k, long e) { fn(e, g.field.off + i * g.field.p0 + j * g.field.p1 + k); });
}

// start of a solve: parameters of the stop test, counters
__global__ void poisson_init_kernel(PoissonCtl *c, int maxiter, double rtol, double atol, double size)
{
    *c = PoissonCtl{};
    c->head.capacity = kSweepWavesMax; c->head.maxiter = maxiter; c->rtol = rtol; c->atol = atol; c->size = size;
}

// r = v - f: the right-hand side of (-A) u = -(f - v) and, x = 0, the first residual (common.py:104 `rhs = np.ravel(arr) - vec`);
// every wave's share of its sum goes to the first of its two slots (singular systems subtract the mean)
template <typename T>
__global__ void __launch_bounds__(256) poisson_rhs_kernel(PGrid g, const T *f, const double *v, double *r, PoissonCtl *c)
{
    ctl_announce(c->head, (long)gridDim.x * (blockDim.x >> 6));
    double s = 0;
    for_cells(g, [&](long e, long ef) {
        const double b = v[e] - (double)f[ef];
        r[e] = b;
        s = s + b;
    });
    wave_partials<2>(poisson_slots(c), {s, 0.0}, wave_slot(), c->head.capacity);
}

// every wave's share of the sum of x (singular systems: the minimum-norm solution has mean zero)
__global__ void __launch_bounds__(256) poisson_sum_kernel(PGrid g, const double *x, PoissonCtl *c)
{
    ctl_announce(c->head, (long)gridDim.x * (blockDim.x >> 6));
    double s = 0;
    for_cells(g, [&](long e, long) { s = s + x[e]; });
    wave_partials<2>(poisson_slots(c), {s, 0.0}, wave_slot(), c->head.capacity);
}

__global__ void __launch_bounds__(256) poisson_shift_kernel(PGrid g, double *x, const PoissonCtl *c)
{
    const double m = c->mean;
    for_cells(g, [&](long e, long) { x[e] = x[e] - m; });
}

// The reference's acceptance test of a least-squares solution (common.py:134 `np.allclose(mat.dot(result), rhs, rtol=1e-5, atol=1e-5)`)
// against the UNPROJECTED right-hand side b = f - v: w = -A x, so A x - b = -w - (f - v).  Shares of the count of violating cells
// (a NaN violates) and of |A x - b|^2 (common.py:135).
template <typename T>
__global__ void __launch_bounds__(256) poisson_check_kernel(PGrid g, const T *f, const double *v, const double *w, PoissonCtl *c)
{
    ctl_announce(c->head, (long)gridDim.x * (blockDim.x >> 6));
    double cnt = 0, res = 0;
    for_cells(g, [&](long e, long ef) {
        const double b = (double)f[ef] - v[e];
        const double d = -w[e] - b;
        if (!(fabs(d) <= 1e-5 + 1e-5 * fabs(b))) cnt = cnt + 1.0;
        res = res + d * d;
    });
    wave_partials<2>(poisson_slots(c), {cnt, res}, wave_slot(), c->head.capacity);
}

template <typename T>
__global__ void __launch_bounds__(256) poisson_store_kernel(PGrid g, const double *x, T *out)
{
    for_cells(g, [&](long e, long ef) { out[ef] = (T)x[e]; });
}

// what = 0: mean = first sum / cells;  1: count = first sum, resid2 = second sum
__global__ void __launch_bounds__(256) poisson_reduce_kernel(PoissonCtl *c, int what)
{
    double s[2];
    sum_slots<2>(poisson_slots(c), ctl_nslots(c->head), s);
    if (threadIdx.x == 0) {
        if (what == 0) c->mean = s[0] / c->size;
        else { c->count = s[0]; c->resid2 = s[1]; }
    }
}

// Behind sweep 1 of iteration k: gamma = r.z, delta = z.w (w = -A z), the stop test on the TRUE residual sqrt(r.r), and the step
// lengths of the update that follows (Chronopoulos-Gear): beta = gamma / gamma_prev, alpha = gamma / (delta - beta * gamma / alpha_prev);
// beta = 0 for k = 0.  The denominator is p.q of the direction the update builds: <= 0 means the system is not definite (or rounding
// has eaten it).  PRECOND: z = M r and sweep 1 left three columns (r.z, z.w, r.r); else z = r and the two columns are r.r, r.w.
template <bool PRECOND>
__global__ void __launch_bounds__(256) poisson_finish_kernel(PoissonCtl *c)
{
    CtlHead &h = c->head;
    if (h.stop) return;   // uniform
    constexpr int N = PRECOND ? 3 : 2;
    double s[N];
    sum_slots<N>(poisson_slots(c), ctl_nslots(h), s);
    if (threadIdx.x != 0) return;
    const double gamma = s[0], delta = s[1], rr = s[PRECOND ? 2 : 0];
    const double gamma_prev = c->gamma, alpha_prev = c->alpha;
    c->gamma = gamma;
    c->rr = rr;
    c->rw = delta;
    if (h.nslots > h.capacity) { h.failed = 4; h.stop = 1; return; }   // (never: blocks_for caps every launch at the slots)
    if (h.iters == 0) {
        c->bnorm = sqrt(rr);
        const double t = c->rtol * c->bnorm;
        c->tol = t > c->atol ? t : c->atol;
    }
    if (!isfinite(gamma) || !isfinite(delta) || !isfinite(rr)) { h.failed = 2; h.stop = 1; return; }
    if (sqrt(rr) <= c->tol) { h.converged = 1; h.stop = 1; return; }
    if (h.iters >= h.maxiter) { h.failed = 1; h.stop = 1; return; }
    double beta = 0, denom = delta;
    if (h.iters > 0) {
        beta = gamma / gamma_prev;
        denom = delta - beta * gamma / alpha_prev;
    }
    if (!(delta > 0) || !(denom > 0) || !(gamma > 0)) { h.failed = 3; h.stop = 1; return; }   // (gamma = r.r > 0 here in the plain loop)
    c->alpha = gamma / denom;
    c->beta = beta;
    h.iters = h.iters + 1;
}

// sweep 1: w = -A r and the wave's shares of r.r and r.w.  The ghost cells of r hold the homogeneous conditions (ghost kernel in front
// of this launch).  The Laplacian in the reference's order (pde/backends/numba/operators/cartesian.py:112-116, :147-151, :220-227);
// the neighbouring rows and planes come out of the caches (the launch walks the planes in order).
template <int VEC>
__global__ void __launch_bounds__(256) poisson_apply_kernel(RowGrid g, int ndim, double sx, double sy, double sz, const double *r, double *w, PoissonCtl *ctl)
{
    if (ctl_stopped(ctl->head)) return;   // uniform
    ctl_announce(ctl->head, (long)gridDim.x * (blockDim.x >> 6));
    typedef double V __attribute__((ext_vector_type(VEC)));
    double s_rr = 0, s_rw = 0;
    for_row_pieces<VEC>(g, [&](long, long, long, long e) {
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
    });
    wave_partials<2>(poisson_slots(ctl), {s_rr, s_rw}, wave_slot(), ctl->head.capacity);
}

// sweep 2: p = z + beta p, q = w + beta q, x += alpha p, r -= alpha q with alpha, beta from the control block (two uniform loads).
// PRECOND: z = M r is an array of its own; else z is the r the thread has loaded anyway.
template <int VEC, bool PRECOND>
__global__ void __launch_bounds__(256) poisson_update_kernel(RowGrid g, double *x, double *r, double *p, double *q, const double *z, const double *w, const PoissonCtl *c)
{
    if (ctl_stopped(c->head)) return;   // uniform
    const double alpha = c->alpha, beta = c->beta;
    typedef double V __attribute__((ext_vector_type(VEC)));
    for_row_pieces<VEC>(g, [&](long, long, long, long e) {
        const V wv = *(const V *)(w + e);
        V pv = *(const V *)(p + e), qv = *(const V *)(q + e), xv = *(const V *)(x + e), rv = *(const V *)(r + e);
        const V zv = PRECOND ? *(const V *)(z + e) : rv;
#pragma unroll
        for (int m = 0; m < VEC; m++) {
            pv[m] = zv[m] + beta * pv[m];
            qv[m] = wv[m] + beta * qv[m];
            xv[m] = xv[m] + alpha * pv[m];
            rv[m] = rv[m] - alpha * qv[m];
        }
        *(V *)(p + e) = pv;
        *(V *)(q + e) = qv;
        *(V *)(x + e) = xv;
        *(V *)(r + e) = rv;
    });
}

const char *face_name(int q, char *buf, size_t len)
{
    snprintf(buf, len, "%s face of axis %d", (q & 1) ? "upper" : "lower", q / 2);
    return buf;
}

int poisson_read(PoissonHandle *h, PoissonCtl *host, void *st) { return read_ctl(host, h->pinned, h->ctl, sizeof(PoissonCtl), st); }

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

// One iteration: sweep 1, the one-workgroup kernel, sweep 2.  Plain loop, sweep 1: the homogeneous conditions into the ghost cells of r
// (they are written even when the solve is over: nothing reads them afterwards), then w = -A r with the shares of r.r and r.w.
// Preconditioned loop: poisson_mg_sweep1 (z = M r, w = -A z, three shares).
int poisson_iteration(PoissonHandle *h, void *st)
{
    const NGrid &n = h->n64;
    const RowGrid g = make_row_grid(n);
    const long cells = g.n0 * g.n1 * g.n2;
    const bool even = g.n2 % 2 == 0;
    if (h->mg) {
        const double *z = nullptr;
        PDEHIP_TRY(poisson_mg_sweep1(h, &z, st));
        hipLaunchKernelGGL(poisson_finish_kernel<true>, dim3(1), dim3(256), 0, as_stream(st), h->ctl);
        PDEHIP_LAUNCH_ROWS(even, cells, st, (poisson_update_kernel<VEC, true>), g, h->x, h->r, h->p, h->q, z, h->w, h->ctl);
        return 0;
    }
    PDEHIP_TRY(launch_ghosts(n, 1, h->faces_a, h->r, as_stream(st)));
    PDEHIP_LAUNCH_ROWS(even, cells, st, poisson_apply_kernel<VEC>, g, n.ndim, n.lap_scale[0], n.lap_scale[1], n.lap_scale[2], h->r, h->w, h->ctl);
    hipLaunchKernelGGL(poisson_finish_kernel<false>, dim3(1), dim3(256), 0, as_stream(st), h->ctl);
    PDEHIP_LAUNCH_ROWS(even, cells, st, (poisson_update_kernel<VEC, false>), g, h->x, h->r, h->p, h->q, (const double *)nullptr, h->w, h->ctl);
    return 0;
}

template <typename T>
int poisson_solve_t(PoissonHandle *h, const T *rhs, T *out, pdehip_poisson_t *io, void *st)
{
    hipStream_t s = as_stream(st);
    const PGrid pg{make_row_grid(h->n64), make_row_grid(h->nf)};
    const long cells = pg.work.n0 * pg.work.n1 * pg.work.n2;
    const unsigned nb = blocks_for(cells);
    PoissonCtl *ctl = h->ctl;
    // x = 0 (ghost cells and padding too), p = q = 0;  w = v = L(0) with the faces as given (cartesian.py `vector`)
    PDEHIP_HIP(hipMemsetAsync(h->x, 0, h->vec_bytes, s));
    PDEHIP_HIP(hipMemsetAsync(h->p, 0, h->vec_bytes, s));
    PDEHIP_HIP(hipMemsetAsync(h->q, 0, h->vec_bytes, s));
    PDEHIP_TRY(laplace_with_input_bcs(&h->g64, h->x, nullptr, h->w, LAP_PLAIN, 0, 0, 0, h->faces, st));
    hipLaunchKernelGGL(poisson_init_kernel, dim3(1), dim3(1), 0, s, ctl, io->maxiter, io->rtol, io->atol, (double)cells);
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
    // the test of the last update needs one more sweep 1
    long enq = 0;
    const long most = (long)io->maxiter + 1;
    while (true) {
        const long nbatch = batch < most - enq ? batch : most - enq;
        for (long b = 0; b < nbatch; b++, enq++) PDEHIP_TRY(poisson_iteration(h, st));
        PDEHIP_TRY(poisson_read(h, &host, st));
        if (host.head.stop) break;
        if (enq >= most || host.head.iters != enq) PDEHIP_FAIL(E_RUNTIME, "internal: the control block of the Poisson solver is out of step with the host");
    }
    if (host.head.failed == 4) PDEHIP_FAIL(E_RUNTIME, "internal: the partial sums of the Poisson solver do not fit their buffer");
    io->iterations = host.head.iters;
    io->residual = sqrt(host.rr);
    io->rhs_norm = host.bnorm;
    io->status = host.head.failed;   // 0 converged, 1 maxiter, 2 non-finite, 3 breakdown
    io->check_residual = 0;
    if (h->singular && host.head.converged) {
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
    else note_kernel("poisson_apply_kernel<%d> (w = -A r with the wave sums of r.r and r.w in the sweep)", pg.work.n2 % 2 == 0 ? 2 : 1);
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
    double **vecs[] = {&h->x, &h->r, &h->p, &h->q, &h->w};
    hipError_t e = hipSuccess;
    for (double **v : vecs) {
        if (e == hipSuccess) e = hipMalloc((void **)v, h->vec_bytes);
        if (e == hipSuccess) e = hipMemset(*v, 0, h->vec_bytes);
    }
    if (e == hipSuccess) e = hipMalloc((void **)&h->ctl, kPoissonCtlBytes);
    if (e == hipSuccess) e = hipMemset(h->ctl, 0, kPoissonCtlBytes);
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
