// pdehip_fftsolve.hip — Poisson's equation on all-periodic grids without an iteration: the periodic 3/5/7-point Laplacian is diagonal in
// Fourier space, so two transforms (pdehip_fft.hip) and one pointwise division solve A u = f to rounding.
//
// Semantics: include/pdehip.h.  Dataflow, tables and scratch: DESIGN.md §4.7.  In short:
//   forward transform of f (fp64 arithmetic for both field types) into the stream's scratch spectrum
//   fftsolve_divide_kernel   u^(m) = (f^(m) / mu(m)) * (-1) over the half spectrum, mu(m) = (mu0[i] + mu1[j]) + mu2[k] from three host
//                            tables; u^(0) = 0 exactly (the projection onto zero mean); f^(0) / size, the mean of f, is kept for the test
//   inverse transform into an fp64 full array x
//   periodic ghost cells of x, w = A x with the stencil kernels every other path uses
//   fftsolve_check_kernel    the reference's acceptance test of a singular solve and the true residual: every wave's share of four sums in
//                            a slot of its own (no floating-point atomic), added on the host in slot order; the same sweep stores x,
//                            rounded once to the field type
// The IEEE division is the compiler's; every operation is rounded once (no FMA contraction in any build).
#include "pdehip_fft.h"
#include "pdehip_sweep.h"

namespace pdehip {
namespace {

constexpr long kCheckBlocksMax = 2048;                         // workgroups of the test: 8192 waves, four sums each
constexpr int kCheckWavesMax = (int)(kCheckBlocksMax * 4);
constexpr int kCheckHead = 8;                                  // doubles in front of the slots: [0] the mean of f
constexpr size_t kCheckCtlBytes = sizeof(double) * (kCheckHead + 4 * (size_t)kCheckWavesMax);

// the eigenvalue of -d^2/dx^2 on a periodic axis of n cells, mode m (the same lines: tests/shim)
double lap_eigenvalue(long m, long n, double scale)
{
    const long mm = m < n - m ? m : n - m;
    const double s = sin(3.14159265358979323846 * (double)mm / (double)n);
    return (4.0 * (s * s)) * scale;
}

struct DivideArgs {
    unsigned n0, n1, nh;
    long total;                    // n0 * n1 * nh modes of the half spectrum
    double size;                   // n0 * n1 * n2
    cplx *spec;
    const double *mu;              // n0 + n1 + n2 eigenvalues
    double *ctl;                   // [0] receives f^(0) / size
};

__global__ void __launch_bounds__(256) fftsolve_divide_kernel(DivideArgs a)
{
    const long stride = (long)gridDim.x * 256;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < a.total; t += stride) {
        cplx z = a.spec[t];
        if (t == 0) {
            a.ctl[0] = z.x / a.size;
            z.x = 0.0; z.y = 0.0;
        } else {
            const unsigned ut = (unsigned)t;
            const unsigned k = ut % a.nh, rest = ut / a.nh;
            const unsigned j = rest % a.n1, i = rest / a.n1;
            const double mu = (a.mu[i] + a.mu[a.n0 + j]) + a.mu[a.n0 + a.n1 + k];
            z.x = (z.x / mu) * -1.0;
            z.y = (z.y / mu) * -1.0;
        }
        a.spec[t] = z;
    }
}

struct CheckArgs {
    RowGrid work, field;           // the fp64 scratch arrays and the caller's arrays
    int f32;                       // type of f and out
    const void *f;
    const double *x, *w;
    void *out;
    double *ctl;                   // [0]: the mean of f; the slots start at kCheckHead
};

// The reference's acceptance test of a least-squares solution (common.py:134 `np.allclose(mat.dot(result), rhs, rtol=1e-5, atol=1e-5)`)
// against the right-hand side as given, the residual against the projected one, and the store of x.  One instance for both field types:
// the sweep is bound by the three fp64 streams it reads.
__global__ void __launch_bounds__(256) fftsolve_check_kernel(CheckArgs a)
{
    const double mean = a.ctl[0];
    double cnt = 0, res = 0, resp = 0, fp = 0;
    for_row_pieces<1>(a.work, [&](long i, long j, long k, long e) {
        const long ef = a.field.off + i * a.field.p0 + j * a.field.p1 + k;
        const double f = a.f32 ? (double)((const float *)a.f)[ef] : ((const double *)a.f)[ef];
        const double wv = a.w[e], xv = a.x[e];
        const double d = wv - f;
        if (!(fabs(d) <= 1e-5 + 1e-5 * fabs(f))) cnt = cnt + 1.0;
        res = res + d * d;
        const double g = f - mean;
        const double dp = wv - g;
        resp = resp + dp * dp;
        fp = fp + g * g;
        if (a.f32) ((float *)a.out)[ef] = (float)xv;
        else ((double *)a.out)[ef] = xv;
    });
    const int capacity = kCheckWavesMax;
    wave_partials<4>(a.ctl + kCheckHead, {cnt, res, resp, fp}, wave_slot(), capacity);
}

// what the solve keeps per stream, in the entry of the transforms
int solve_scratch(hipStream_t st, const NGrid &n64, FftScratch *out)
{
    return fft_table().with(st, [&](FftScratch &s) -> int {
        if (!s.mu_dev) {
            PDEHIP_HIP(hipMalloc((void **)&s.mu_dev, sizeof(double) * (2 * kFftSlowMax + kFftFastMax)));
            PDEHIP_HIP(hipHostMalloc((void **)&s.mu_host, sizeof(double) * (2 * kFftSlowMax + kFftFastMax), hipHostMallocDefault));
            PDEHIP_HIP(hipMalloc((void **)&s.sol_ctl, kCheckCtlBytes));
            PDEHIP_HIP(hipHostMalloc((void **)&s.sol_pinned, kCheckCtlBytes, hipHostMallocDefault));
        }
        bool same = true;
        for (int ax = 0; ax < 3; ax++) same = same && s.mu_n[ax] == n64.n[ax] && s.mu_scale[ax] == n64.lap_scale[ax];
        if (!same) {
            PDEHIP_HIP(hipStreamSynchronize(st));          // (a copy of the tables before may still read the pinned memory)
            long at = 0;
            for (int ax = 0; ax < 3; ax++)
                for (long m = 0; m < n64.n[ax]; m++, at++) s.mu_host[at] = lap_eigenvalue(m, n64.n[ax], n64.lap_scale[ax]);
            PDEHIP_HIP(hipMemcpyAsync(s.mu_dev, s.mu_host, sizeof(double) * at, hipMemcpyHostToDevice, st));
            for (int ax = 0; ax < 3; ax++) { s.mu_n[ax] = n64.n[ax]; s.mu_scale[ax] = n64.lap_scale[ax]; }
        }
        const size_t bytes = (size_t)(n64.pc + kAllocSlack) * sizeof(double);
        if (s.sol_bytes < bytes) {
            if (s.sol_x) PDEHIP_HIP(hipFree(s.sol_x));     // (hipFree waits for the device)
            if (s.sol_w) PDEHIP_HIP(hipFree(s.sol_w));
            s.sol_x = s.sol_w = nullptr; s.sol_bytes = 0;
            hipError_t e = hipMalloc((void **)&s.sol_x, bytes);
            if (e == hipSuccess) e = hipMalloc((void **)&s.sol_w, bytes);
            if (e != hipSuccess) {
                (void)hipFree(s.sol_x);
                s.sol_x = nullptr;
                PDEHIP_FAIL(100 + (int)e, "hipMalloc of 2 x %zu bytes for the direct Poisson solve failed: %s", bytes, hipGetErrorString(e));
            }
            s.sol_bytes = bytes;
        }
        *out = s;
        return 0;
    });
}

}  // namespace
}  // namespace pdehip

using namespace pdehip;

extern "C" int pdehip_poisson_fft(const pdehip_grid_t *g, const void *rhs_full, void *out_full, pdehip_poisson_t *io, void *stream)
{
    NGrid nf;
    PDEHIP_TRY(fft_check(g, &nf));
    if (!rhs_full || !out_full || !io) PDEHIP_FAIL(E_VALUE, "poisson_fft: NULL pointer");
    if ((((uintptr_t)rhs_full | (uintptr_t)out_full) & 15) != 0) PDEHIP_FAIL(E_VALUE, "poisson_fft: misaligned array (16 bytes for the right-hand side and the result)");
    if (!(io->rtol >= 0) || !(io->atol >= 0)) PDEHIP_FAIL(E_VALUE, "poisson_fft: bad rtol / atol");
    pdehip_grid_t g64 = *g;
    g64.dtype = PDEHIP_F64;
    NGrid n64;
    PDEHIP_TRY(norm_grid(&g64, &n64));
    hipStream_t st = as_stream(stream);
    const long nh = n64.n[2] / 2 + 1, total = n64.n[0] * n64.n[1] * nh, cells = n64.n[0] * n64.n[1] * n64.n[2];
    cplx *spec = nullptr;
    PDEHIP_TRY(fft::spectrum_scratch(st, sizeof(cplx) * (size_t)total, &spec));
    FftScratch s;
    PDEHIP_TRY(solve_scratch(st, n64, &s));

    std::string names;
    PDEHIP_TRY(fft::forward(nf, 1, rhs_full, spec, st, &names));
    {
        DivideArgs a;
        a.n0 = (unsigned)n64.n[0]; a.n1 = (unsigned)n64.n[1]; a.nh = (unsigned)nh; a.total = total; a.size = (double)cells;
        a.spec = spec; a.mu = s.mu_dev; a.ctl = s.sol_ctl;
        hipLaunchKernelGGL(fftsolve_divide_kernel, dim3(blocks_for(total, kCheckBlocksMax)), dim3(256), 0, st, a);
        PDEHIP_HIP(hipGetLastError());
        names += "+fftsolve_divide_kernel+";
    }
    PDEHIP_TRY(fft::inverse(n64, 1, spec, s.sol_x, st, &names));
    // the test the CG path applies: periodic ghost cells of x, w = A x
    pdehip_bc_face_t faces[2 * PDEHIP_MAX_DIM];
    memset(faces, 0, sizeof(faces));
    for (int a = 0; a < n64.ndim; a++)
        for (int side = 0; side < 2; side++) {
            pdehip_bc_face_t &f = faces[2 * a + side];
            f.kind = PDEHIP_BC_ORDER1;
            f.index1 = side ? 0 : g->shape[a] - 1;
            f.factor1 = 1.0;
        }
    PDEHIP_TRY(launch_ghosts(n64, 1, faces, s.sol_x, st));
    PDEHIP_TRY(laplace_with_input_bcs(&g64, s.sol_x, nullptr, s.sol_w, LAP_PLAIN, 0, 0, 0, faces, stream));
    const unsigned nb = blocks_for(cells, kCheckBlocksMax);
    {
        CheckArgs a;
        a.work = make_row_grid(n64); a.field = make_row_grid(nf); a.f32 = nf.dtype == PDEHIP_F32;
        a.f = rhs_full; a.x = s.sol_x; a.w = s.sol_w; a.out = out_full; a.ctl = s.sol_ctl;
        hipLaunchKernelGGL(fftsolve_check_kernel, dim3(nb), dim3(256), 0, st, a);
        PDEHIP_HIP(hipGetLastError());
        names += "+fftsolve_check_kernel";
    }
    const int waves = (int)nb * 4;
    PDEHIP_HIP(hipMemcpyAsync(s.sol_pinned, s.sol_ctl, sizeof(double) * (kCheckHead + 4 * (size_t)waves), hipMemcpyDeviceToHost, st));
    PDEHIP_HIP(hipStreamSynchronize(st));
    // the shares of the waves, added in slot order
    double sum[4] = {0, 0, 0, 0};
    for (int w = 0; w < waves; w++)
        for (int q = 0; q < 4; q++) sum[q] = sum[q] + s.sol_pinned[kCheckHead + 4 * w + q];
    io->iterations = 0;
    io->singular = 1;
    io->reserved = 0;
    io->check_residual = sqrt(sum[1]);
    io->residual = sqrt(sum[2]);
    io->rhs_norm = sqrt(sum[3]);
    const double t = io->rtol * io->rhs_norm, tol = t > io->atol ? t : io->atol;
    if (!std::isfinite(sum[0]) || !std::isfinite(sum[1]) || !std::isfinite(sum[2]) || !std::isfinite(sum[3])) io->status = 2;
    else if (sum[0] != 0) io->status = 4;
    else if (io->residual > tol) io->status = 1;
    else io->status = 0;
    note_kernel("%s", names.c_str());
    return 0;
}
