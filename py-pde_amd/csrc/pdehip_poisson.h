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
// fp64 one), and those sweeps are not to get slower for this.  A one-workgroup kernel (poisson_finish_kernel) adds the shares in a
// fixed order, derives alpha and beta, does the stop test and writes the control block (PoissonCtl below).  Sweep 2
// (poisson_update_kernel) is pointwise: p = r + beta p, q = w + beta q, x += alpha p, r -= alpha q.  Both are templates on PRECOND: the
// preconditioned loop (pdehip_poisson_mg.h) is the same recurrence with z = M r in the place of r and its own sweep 1.  Every launch
// reads the block's stop word at entry and returns at once when the solve is over; the host enqueues a batch of iterations and reads
// the block through pinned memory once per batch.  Nothing on the device waits; the result does not depend on the batch size.
//
// All work vectors and scalars are fp64 whatever the type of the field: an fp32 field is converted on the way in and out.
#pragma once

#include <cstddef>

#include "pdehip_sweep.h"

namespace pdehip {

// Control block and the deterministic dot products.  One device allocation like the fixed-point block (pdehip_device.h): this block,
// then (at kPoissonSlots doubles from its start) up to kPoissonColumns interleaved partial sums per wave of the sweep that ran last:
// two in the plain loop (r.r, r.w) and around a solve, three in the preconditioned loop (r.z, z.w, r.r).  Every kernel of the solver is
// launched through blocks_for, so kSweepWavesMax slots hold any launch.  Only the one-workgroup kernels write the block during a solve.
struct PoissonCtl {
    CtlHead head;        // iters: updates of x done; failed = 2: a non-finite scalar, 3: breakdown (r.z, z.w or p.q <= 0 for a definite system), 4: internal
    double rr;           // r.r of the iteration that ran last: the stop test is sqrt(rr) <= tol
    double rw;           // delta = z.w, w = -A z (z = r in the plain loop)
    double gamma;        // r.z (equal to rr in the plain loop)
    double alpha, beta;  // step lengths of the update that follows (Chronopoulos-Gear)
    double bnorm;        // ||b||_2, b = the right-hand side of the split system (r of iteration 0)
    double tol;          // max(rtol * ||b||, atol)
    double rtol, atol;
    double mean;         // singular systems: the mean of b / of x that the pointwise kernels subtract
    double size;         // cells
    double count;        // singular systems: cells that violate |A x - b| <= 1e-5 + 1e-5 |b|
    double resid2;       // singular systems: |A x - b|^2 of that test
};
constexpr int kPoissonSlots = 24;     // doubles in front of the partial sums
constexpr int kPoissonColumns = 3;
static_assert(sizeof(PoissonCtl) <= kPoissonSlots * sizeof(double), "the control block of the Poisson solver overlaps its partial sums");
constexpr size_t kPoissonCtlBytes = (kPoissonSlots + (size_t)kPoissonColumns * kSweepWavesMax) * sizeof(double);
__device__ __forceinline__ double *poisson_slots(PoissonCtl *c) { return (double *)c + kPoissonSlots; }

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
    PoissonCtl *ctl = nullptr;     // the block and its slots: kPoissonCtlBytes
    PoissonCtl *pinned = nullptr;
    bool singular = false;         // every face periodic or Neumann: A has the constants in its null space
    PoissonMg *mg = nullptr;       // pdehip_poisson_set_multigrid: the solve runs the preconditioned loop (pdehip_poisson_mg.h)
};

}  // namespace pdehip
