// pdehip_poisson_mg.h — the preconditioner of the Poisson solver: one geometric multigrid V-cycle `z = M r` (pdehip_poisson_mg.hip) and
// the preconditioned loop around it (method "mgcg").
//
// Hierarchy: level l+1 halves every axis of level l whose extent is even and >= 4; the other axes keep extent and spacing.  It ends
// when no axis qualifies or a level has <= 512 cells.  Every level carries the REDISCRETISED Laplacian (spacing doubled on the halved
// axes) with the same homogeneous faces (`ghost = factor1 * adjacent` / periodic); coefficient arrays of a face are averaged over the
// children of each coarse face cell.
// Smoother: damped Jacobi with the exact diagonal of -A, d = sum_a s_a (2 - [lower face] f_lo - [upper face] f_hi) (2 s_a on periodic
// axes), computed from the position of the cell; omega = 2/3, 4/5, 6/7 in 1, 2, 3 dimensions.  `smooth` sweeps before and after the
// coarse-grid correction, `coarse_sweeps` from zero on the last level.  Transfers: mean of the children down, copy to the children up
// (P = 2^k R^T).  Same sweeps before and after, a symmetric smoother, P ~ R^T: M is symmetric and positive - a fixed linear operator,
// so conjugate-gradient theory holds and results are reproducible.
//
// Loop (Chronopoulos-Gear, one reduction point per iteration): z = M r; w = -A z with every wave's share of r.z, z.w and r.r (sweep 1,
// this file's poisson_mg_apply_kernel: three columns of the handle's slots).  Behind it the kernels of the plain loop with PRECOND
// (pdehip_poisson.hip): gamma = r.z, delta = z.w, beta = gamma / gamma_prev, alpha = gamma / (delta - beta gamma / alpha_prev); the
// stop test on the TRUE residual norm sqrt(r.r); p = z + beta p, q = w + beta q, x += alpha p, r -= alpha q.
// Singular systems: A annihilates constants, so a constant component that M adds to z changes none of w, q, r, gamma (r has mean
// zero: the right-hand side was projected) and delta; it only travels into x, whose mean is removed at the end as in the plain loop.
#pragma once

#include "pdehip_poisson.h"

namespace pdehip {

int poisson_mg_set(PoissonHandle *h, pdehip_poisson_mg_t *opts);   // builds (opts != NULL) or drops the hierarchy of a handle
void poisson_mg_release(PoissonHandle *h);
// sweep 1 of the preconditioned loop: the cycle z = M r, then w = -A z with the three sums; *z = the array the cycle left z in.  The
// one-workgroup kernel and sweep 2 behind it are those of the plain loop (pdehip_poisson.hip).  Every launch returns at entry when
// the control block says the solve is over.
int poisson_mg_sweep1(PoissonHandle *h, const double **z, void *st);
void poisson_mg_note(const PoissonHandle *h);   // pdehip_last_kernel_name after a solve

}  // namespace pdehip
