// pdehip_poisson.h — the stationary solve of the reference: `poisson_solver` (pde/backends/scipy/operators/cartesian.py:472-489,
// common.py:71-146), the operator behind solve_poisson_equation / solve_laplace_equation (pde/pdes/laplace.py:28-125).
//
// The reference assembles the Laplacian with its boundary conditions as a sparse matrix plus a constant vector, `L u = A u + v`, and
// hands `A u = f - v` to a direct solver.  Here the same splitting is solved by conjugate gradients on the device:
//   A = the Laplacian with the HOMOGENEOUS part of every face (`ghost = factor1 * value`: a copy of the face table with the constants
//       zeroed, so the stencil kernels with their on-the-fly faces serve unchanged),
//   v = L(0), one call of the operator on a zero field with the faces as given.
// First-order faces only touch the diagonal (Dirichlet, Neumann, Robin) or link the two ends of an axis symmetrically (periodic): A is
// symmetric and -A positive (semi-)definite.  The loop solves (-A) u = v - f.
//
// Iteration: the single-reduction form of Chronopoulos and Gear.  Sweep 1 (poisson_apply_kernel) computes w = -A r with the stencil and,
// in the same pass, every wave's share of r.r and r.w; the ghost cells of r are set by the ghost kernel in front of it (faces only: a
// launch over O(N^2) cells).  It is a kernel of its own: as one more run-time epilogue of lap_march_kernel the two sums cost instances
// of the Runge-Kutta stage sweeps their last registers (scratch: 1072 bytes in the fp32 4 x 4 tile with tails, 68 in a contracted
// fp64 one), and those sweeps are not to get slower for this.  A one-workgroup kernel adds the shares in a fixed order, derives alpha
// and beta, does the stop test and writes the control block (PoissonCtl below).  Sweep 2 is pointwise: p = r + beta p, q = w + beta q, x += alpha p, r -= alpha q.  Every launch
// reads the block's stop word at entry and returns at once when the solve is over; the host enqueues a batch of iterations and reads
// the block through pinned memory once per batch.  Nothing on the device waits; the result does not depend on the batch size.
//
// All work vectors and scalars are fp64 whatever the type of the field: an fp32 field is converted on the way in and out.
#pragma once

#include <cstddef>

#include "pdehip_common.h"

namespace pdehip {

// Control block and the two deterministic dot products.  One device allocation like the fixed-point block (pdehip_device.h): this
// block, then (at kPoissonSlots doubles from its start) TWO partial sums per wave of the sweep that ran last.  `stop`, `nslots` and
// `capacity` sit where FixedPointCtl has them, so fixedpoint_stopped and fixedpoint_announce serve both.  Only the one-workgroup
// kernels write the block during a solve.
struct PoissonCtl {
    double rr;           // r.r of the iteration that ran last
    double rw;           // r.w, w = -A r
    int iters;           // updates of x done
    int converged;       // ||r|| <= tol held
    int failed;          // 1: maxiter updates without convergence, 2: a non-finite scalar, 3: breakdown (r.w <= 0 or p.q <= 0 for a definite system), 4: internal
    int stop;            // converged | failed: every later launch of the solve returns at once
    int nslots;          // waves of the last sweep (two partial sums each)
    int maxiter;
    double alpha, beta;  // step lengths of the update that follows (Chronopoulos-Gear)
    int capacity;        // waves the buffer behind the block holds
    int reserved;
    double bnorm;        // ||b||_2, b = the right-hand side of the split system (r of iteration 0)
    double tol;          // max(rtol * ||b||, atol)
    double rtol, atol;
    double mean;         // singular systems: the mean of b / of x that the pointwise kernels subtract
    double size;         // cells
    double count;        // singular systems: cells that violate |A x - b| <= 1e-5 + 1e-5 |b|
    double resid2;       // singular systems: |A x - b|^2 of that test
};
constexpr int kPoissonSlots = 16;   // doubles in front of the partial sums
static_assert(sizeof(PoissonCtl) == kPoissonSlots * sizeof(double), "the control block of the Poisson solver overlaps its partial sums");
static_assert(offsetof(PoissonCtl, stop) == offsetof(FixedPointCtl, stop) && offsetof(PoissonCtl, nslots) == offsetof(FixedPointCtl, nslots) &&
              offsetof(PoissonCtl, capacity) == offsetof(FixedPointCtl, capacity), "fixedpoint_stopped / fixedpoint_announce read both control blocks");
// end of a sweep of the solver: the butterfly sums of fixedpoint_wave_partial for both dot products (every lane ends with the same
// bits, in an order fixed by the lane numbers), two stores per wave into its slots.  No atomics.
__device__ __forceinline__ void poisson_wave_partial(double *ctl, double s_rr, double s_rw, int slot)
{
#pragma unroll
    for (int ofs = 32; ofs >= 1; ofs >>= 1) {
        s_rr = s_rr + __shfl_xor(s_rr, ofs, 64);
        s_rw = s_rw + __shfl_xor(s_rw, ofs, 64);
    }
    if ((threadIdx.x & 63) == 0 && slot < ((const PoissonCtl *)ctl)->capacity) {
        ctl[kPoissonSlots + 2 * slot] = s_rr;
        ctl[kPoissonSlots + 2 * slot + 1] = s_rw;
    }
}

struct PoissonMg;   // pdehip_poisson_mg.hip: the hierarchy of the multigrid preconditioner

struct PoissonHandle {
    pdehip_grid_t g;       // the grid of the fields handed to pdehip_poisson_solve
    pdehip_grid_t g64;     // the same grid in fp64: layout of the work vectors
    NGrid nf, n64;
    pdehip_bc_face_t faces[2 * PDEHIP_MAX_DIM];     // as given: v = L(0)
    pdehip_bc_face_t faces_a[2 * PDEHIP_MAX_DIM];   // constants zeroed: the matrix A
    double *zero_face = nullptr;   // the `const_arr` of the homogeneous copy of faces with coefficient arrays
    double *x = nullptr, *r = nullptr, *p = nullptr, *q = nullptr, *w = nullptr;
    size_t vec_bytes = 0;
    double *ctl = nullptr;         // PoissonCtl + two partial sums per wave
    int capacity = 0;
    PoissonCtl *pinned = nullptr;
    bool singular = false;         // every face periodic or Neumann: A has the constants in its null space
    PoissonMg *mg = nullptr;       // pdehip_poisson_set_multigrid: the solve runs the preconditioned loop (pdehip_poisson_mg.h)
};

}  // namespace pdehip
