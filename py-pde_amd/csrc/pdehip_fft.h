// pdehip_fft.h — what pdehip_fft.hip shares with the direct Poisson solve (pdehip_fftsolve.hip): the dry run, the passes of the forward
// and of the inverse transform on a stream, and the per-stream scratch both units keep in ONE table (pdehip_release_scratch frees it).
// Semantics: include/pdehip.h.  Dataflow: DESIGN.md §4.17 (transforms), §4.7 (the solve).
#pragma once

#include <string>

#include "pdehip_common.h"
#include "pdehip_scratch.h"

namespace pdehip {

typedef double2 cplx;
constexpr long kFftSlowMax = 1024, kFftFastMax = 4096;

// per stream: twiddles, frequencies, the spectrum of one component, maxima, parameters and limbs, pinned host memory; and, for the direct
// solve, the eigenvalue tables, two fp64 full arrays and the partial sums of its test
struct FftScratch {
    cplx *tw_dev, *tw_host;                    // kFftFastMax entries: the tables of axes 0, 1, 2 one after the other
    long tw_n[3];                              // the extents the tables were made for
    double *kf_dev;                            // 2 kFftSlowMax + kFftFastMax frequencies of the normalised axes
    double *edges_host;                        // kShellBinsMax + 1
    cplx *spec; size_t spec_bytes;
    unsigned long long *maxbits; int2 *params; long long *limb; size_t slots;          // per (component, slot); params: one component's
    unsigned long long *host;                  // pinned: maxima, limbs, counts, sums of a call
    size_t host_slots;
    // pdehip_poisson_fft
    double *mu_dev, *mu_host;                  // 2 kFftSlowMax + kFftFastMax eigenvalues of the normalised axes, one axis after the other
    long mu_n[3]; double mu_scale[3];          // the extents and 1 / dx^2 the tables were made for
    double *sol_x, *sol_w; size_t sol_bytes;   // fp64 full arrays of the grid: the solution and A x
    double *sol_ctl, *sol_pinned;              // the mean of f, then four partial sums per wave of the test; its pinned mirror
};
StreamTable<FftScratch> &fft_table();

// 0, or the refusal of the dry run: every normalised axis absent or a power of two up to 1024, the fastest up to 4096
int fft_check(const pdehip_grid_t *g, NGrid *n);

namespace fft {
// the spectrum buffer of the stream, at least `spec_bytes` long
int spectrum_scratch(hipStream_t st, size_t spec_bytes, cplx **spec);
// the transform of `ncomp` components of `in` (a full array of n) into `spec` (ncomp, n0, n1, nh); the names of the launches are appended
int forward(const NGrid &n, int ncomp, const void *in, cplx *spec, hipStream_t st, std::string *names);
// ... and back: `spec` is consumed (the slow axes run in place), the interior cells of `out` (a full array of n) receive the real part
// of the unnormalised inverse times 1 / size, rounded once to the type of n
int inverse(const NGrid &n, int ncomp, cplx *spec, void *out, hipStream_t st, std::string *names);
}  // namespace fft

}  // namespace pdehip
