/*
 * pdehip.h — C ABI of libpdehip.so, the MI355X (gfx950) backend for py-pde's
 * Cartesian finite-difference operators + explicit time steppers.
 *
 * This is the drop-in boundary: the entry points below are what a
 * `pde.backends` plugin binds through ctypes.  Every function cites the reference
 * interface it replaces (paths relative to the py-pde source tree).  There are no
 * torch / numpy types in any signature: plain pointers, sizes and POD structs.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; the message of the
 *     last failure (per thread) is returned by pdehip_last_error().
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *   - all array pointers are DEVICE pointers unless the name says `host`.
 *   - a "full" array is the ghost-padded C-contiguous array of py-pde
 *     (pde/grids/base.py:329-337, pde/fields/base.py:116-160): shape
 *     (ncomp, N0+2, N1+2, N2+2) (unused axes dropped), interior cell (i,j,k) lives
 *     at [i+1, j+1, k+1].  A "valid" array is the C-contiguous interior
 *     (ncomp, N0, N1, N2).
 *   - ON THE DEVICE a full array keeps the ghost-padded index space of the reference but
 *     every row of the fastest axis is shifted/padded so that its first interior cell is
 *     16-byte aligned and the row pitch is a multiple of 16 bytes (all hot-kernel accesses
 *     are aligned dwordx4).  pdehip_layout() reports pitches and the allocation size;
 *     pdehip_valid_to_full / pdehip_hostfull_to_full convert from the host layouts.  Layers
 *     along axis 0 stay contiguous (one block per slab face for the halo exchange).
 *   - dtype PDEHIP_F32 stores fp32.  TWO arithmetic modes exist for such fields, chosen PER CALL by the entry point:
 *       "fp64" (default; every entry point but the three below): all arithmetic between a load and the store of
 *         one kernel runs in fp64 registers (numba promotes float32 array elements against float64 closure
 *         constants the same way, SURVEY.md §7 "fp32"), rounded to fp32 once at the store;
 *       "fp32" (pdehip_laplace_f32p, pdehip_euler_run_f32p; pdehip_f32p_supported is their dry run): every operation
 *         is rounded to fp32 and the constants dx**-2, D and dt enter as fp32 - the arithmetic of the reference's
 *         torch backend on fp32 fields, bit for bit (contract at those entry points).
 *   - the arithmetic of every kernel follows the reference expression order and is
 *     compiled with -ffp-contract=off, so results are bit-identical to the CPU
 *     oracle (oracle/pde_oracle.c) and to the reference's eager torch-CPU backend
 *     (fp32 fields: the default mode matches the reference's numba backend, the "fp32" mode its torch backend).
 */
#ifndef PDEHIP_H
#define PDEHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDEHIP_MAX_DIM 3
#define PDEHIP_ABI_VERSION 8

enum { PDEHIP_F64 = 0, PDEHIP_F32 = 1 };
/* derivative flavour, pde/backends/numba/operators/cartesian.py:386-587 `method` */
enum { PDEHIP_CENTRAL = 0, PDEHIP_FORWARD = 1, PDEHIP_BACKWARD = 2 };
/* layout of an operator's output array */
enum { PDEHIP_OUT_VALID = 0, PDEHIP_OUT_FULL = 1 };

/* Geometry of a CartesianGrid / UnitGrid (pde/grids/cartesian.py:36-146, :473-507).
 * `shape` and `dx` mirror grid.shape / grid.discretization. */
typedef struct pdehip_grid {
    int32_t ndim;                  /* 1, 2 or 3 */
    int32_t dtype;                 /* PDEHIP_F64 | PDEHIP_F32 */
    int64_t shape[PDEHIP_MAX_DIM]; /* valid cells per axis; unused axes must be 1 */
    double dx[PDEHIP_MAX_DIM];     /* grid.discretization */
} pdehip_grid_t;

/* One side of one axis of a BoundariesList, already reduced to virtual-point data
 * (pde/grids/boundaries/local.py:1611-1636 ConstBC1stOrderBase.set_ghost_cells,
 *  :2022-2061 ConstBC2ndOrderBase.set_ghost_cells, data from get_virtual_point_data
 *  :1728-1731 periodic, :1749-1753 Dirichlet, :1773-1778 Neumann, :1927-1938 Mixed,
 *  :2081-2103 Curvature):
 *      ghost = const + factor1 * full[index1 + 1]  (+ factor2 * full[index2 + 1])
 * evaluated on the interior of the face only (corners/edges are never written).
 */
enum { PDEHIP_BC_SKIP = 0, PDEHIP_BC_ORDER1 = 1, PDEHIP_BC_ORDER2 = 2 };
enum {
    PDEHIP_BCF_ARRAYS = 1, /* const/factor given per (component, face cell) as fp64 device
                              arrays of shape (ncomp, face cells in C order) */
    PDEHIP_BCF_NORMAL = 2  /* `bc.normal`: only vector component == axis is written */
};
typedef struct pdehip_bc_face {
    int32_t kind;  /* PDEHIP_BC_* */
    int32_t flags; /* PDEHIP_BCF_* */
    int64_t index1, index2; /* indices into the VALID array along the axis */
    double const_v, factor1, factor2; /* used when !(flags & PDEHIP_BCF_ARRAYS) */
    const double *const_arr, *factor1_arr, *factor2_arr; /* used when ARRAYS */
} pdehip_bc_face_t;
/* Faces are stored as faces[2*axis + upper] (lower = 0, upper = 1); they are applied in
 * the reference order axis 0 (upper, lower), axis 1 (upper, lower), ...
 * (pde/backends/numba/backend.py:335-340, pde/grids/boundaries/axis.py:236-238). */

/* Right-hand side of the PDEs on the hot path, evaluated by the fused steppers. */
enum {
    PDEHIP_RHS_DIFFUSION = 0,    /* D * laplace(c)            pde/pdes/diffusion.py:119-121 */
    PDEHIP_RHS_CAHN_HILLIARD = 1 /* laplace(c**3 - c - g*laplace(c)) pde/pdes/cahn_hilliard.py:115-122 */
};
/* flags in pdehip_rhs_t.reserved, read ONLY by the entry points that say so (0 everywhere else) */
enum { PDEHIP_RHS_F32P_ONE_STEP = 1 /* pdehip_euler_run_f32p: one step per launch on every grid (the instance the two-step sweep is tested against) */ };
typedef struct pdehip_rhs {
    int32_t kind;
    int32_t reserved;               /* PDEHIP_RHS_* flags, else 0 */
    double param;                   /* diffusivity D, or interface_width g */
    pdehip_bc_face_t bc_c[2 * PDEHIP_MAX_DIM];  /* BCs of the state field */
    pdehip_bc_face_t bc_mu[2 * PDEHIP_MAX_DIM]; /* BCs of mu (Cahn-Hilliard only) */
    void *scratch_mu;               /* full array (Cahn-Hilliard only) */
    /* Faces whose coefficient arrays depend on time (expression conditions that contain `t`) or on the field (conditions that
     * are not affine in the adjacent value): a program from pdehip_bcprog_create that rewrites the const / factor arrays the face
     * tables above point to, or NULL.  Every entry point that evaluates the right-hand side runs it for the time AND the input
     * field of THAT evaluation first, on the same stream (only faces of bc_c may read the field) (Euler: t + i*dt,
     * Runge-Kutta: the stage times t + a_s*dt; pde/solvers/euler.py:172-175, pde/solvers/runge_kutta.py:52-59, :135-145 pass
     * `t` to the right-hand side, which hands it to the conditions as args={"t": t}: pde/pdes/diffusion.py:119-121). */
    void *bc_program;
    double t;                       /* time of a single evaluation (rhs_scaled, rk4_step, rkf45_attempt, ab2_step) / of the
                                       first step of a fixed-step run (euler_run, rk4_run); ignored without bc_program */
} pdehip_rhs_t;

/* ---- boundary conditions given as expressions, evaluated ON THE DEVICE --------------------------------------------------------
 * Replaces the per-call evaluation of ExpressionBC (pde/grids/boundaries/local.py:766-1150; numba twin
 * pde/backends/numba/_boundaries.py:256-394, torch twin pde/backends/torch/_boundaries.py:258-345).  A condition whose virtual
 * point F(value, dx, coords, t) is affine in the adjacent value is  ghost = A(dx, coords, t) + B(dx, coords, t) * value, i.e. a
 * first-order face with per-cell coefficient arrays (PDEHIP_BCF_ARRAYS).  A condition that is NOT affine in `value` is the same
 * face with A = F(value now, dx, coords, t), B = 0, rewritten from the field every time the conditions are applied
 * (`reads_value`: the program reads the cell `value_index` of the field along the face's axis, like the reference's
 * `arr[..., value_cell]`, local.py:1089-1135).  A program is C source (compiled with hiprtc) that defines
 *     PDEHIP_BC_FN void bc_face(int face, double value, double dx, double c0, double c1, double c2, double t, double *A, double *B)
 * (c0..c2 = coordinates of the wall point along the grid axes; value = 0 for faces that do not read the field), plus one
 * descriptor per face: where A and B go and how the face cell (i1, i2) maps to coordinates.  pdehip_bcprog_run evaluates all
 * faces of the program for time t - and the field `state_full` - in ONE launch; the stencil kernels and the ghost kernel then
 * read the arrays as usual. */
typedef struct pdehip_bcprog_face {
    double *const_arr, *factor_arr;   /* fp64 device arrays of m1 * m2 face cells (C order), written by the program */
    int64_t m1, m2;                   /* face extents along the remaining grid axes in grid order (1 where there is none) */
    double origin[3], step[3];        /* per coordinate k: index[k] == 0: c[k] = origin[k] (the wall, or an unused slot);        */
    int32_t index[3];                 /*   index[k] == 1 / 2: c[k] = (first[k] + i1 / i2 + 0.5) * step[k] + origin[k] - cell centres of */
    int32_t reads_value;              /*   the reference (discretize_interval, pde/grids/base.py:88-113), operation by operation */
    double dx;                        /* spacing normal to the wall */
    int32_t axis;                     /* reads_value: grid axis normal to the face, ...                                      */
    int32_t component;                /*   ... component of the field (0 for a scalar field) and ...                          */
    int64_t value_index;              /*   ... valid index along `axis` of the cells whose values are handed to bc_face        */
    int64_t first[3];                 /* per coordinate k with index[k] != 0: global index of the face's first cell - the face of a slab / block of a
                                         decomposed grid evaluates c[k] = ((first[k] + i) + 0.5) * step[k] + origin[k] with the bounds of the WHOLE grid,
                                         bit-identical to the undecomposed run (0 for a whole grid)                              */
} pdehip_bcprog_face_t;
/* `grid`: layout of the fields handed to pdehip_bcprog_run (NULL when no face reads the field) */
int pdehip_bcprog_create(const char *source, int nfaces, const pdehip_bcprog_face_t *faces, const pdehip_grid_t *grid, void **handle);
/* `state_full`: the field the conditions are about to be applied to (may be NULL when no face reads it) */
int pdehip_bcprog_run(void *handle, double t, const void *state_full, void *stream);
int pdehip_bcprog_destroy(void *handle);

/* ---- runtime ------------------------------------------------------------------ */
const char *pdehip_last_error(void);
/* name of the stencil-kernel instance the calling thread launched last (template name with its tile shape and switches), "" before the first
 * launch; ABI version 7.  Measurement aid: bench.py labels its roofline with the instance that ran.  (No counterpart in the reference.) */
const char *pdehip_last_kernel_name(void);
/* Arithmetic mode of the stencil kernels (Laplacian / gradient / divergence, the fused right-hand sides and time steps, ghost cells, run-time
 * compiled expression kernels), process-wide; ABI version 7.  0 (default): compiled with -ffp-contract=off - every rounding of the reference's
 * expression order, results bit-identical to its numpy / torch-CPU evaluation.  1: the same kernels compiled with FMA contraction - what
 * numba's default `fastmath` (pde/backends/numba/utils.py:330-336; config `backend.numba.fastmath`, pde/backends/numba/config.py:20-26) allows
 * the reference's own numba backend; results agree with the exact build within 1e-10 relative (tests/test_hip_fastmath.py), ~10-20 % fewer
 * fp64 operations per cell.  Per call, every kernel instance is held to the rounding-error bound of its own expression - an FMA only removes a
 * rounding, nothing is reassociated - against a reference in extended precision (tests/test_hip_fastmath_instances.py, tests/fastmath_cases.py).  Set it before building steppers: kernels of expression PDEs are compiled for the mode current at their first use. */
int pdehip_set_fastmath(int on);
int pdehip_get_fastmath(int *on);
int pdehip_abi_version(void);
int pdehip_device_count(int *count);
int pdehip_set_device(int device);
int pdehip_device_name(char *buf, size_t len);
/* memory: replaces numpy allocation in NumbaBackend.make_operator
 * (pde/backends/numba/backend.py:460-517) and TorchBackend.numpy_to_native
 * (pde/backends/torch/backend.py:217-238); memory is zero-initialised */
int pdehip_malloc(void **ptr, size_t bytes);
int pdehip_free(void *ptr);
int pdehip_memset(void *ptr, int value, size_t bytes, void *stream);
int pdehip_memcpy_h2d(void *dst, const void *src_host, size_t bytes, void *stream);
int pdehip_memcpy_d2h(void *dst_host, const void *src, size_t bytes, void *stream);
int pdehip_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream);
/* the same by a kernel with streaming stores (16-byte aligned pointers, a multiple of 16 bytes): the fastest copy order on MI355X, the
 * yardstick bench.py prices the stencil kernels against (no reference counterpart: numpy copies on the host) */
int pdehip_copy_nt(void *dst, const void *src, size_t bytes, void *stream);
int pdehip_stream_create(void **stream);
int pdehip_stream_destroy(void *stream);
int pdehip_stream_synchronize(void *stream);
int pdehip_stream_wait_event(void *stream, void *event);
int pdehip_event_create(void **event);
int pdehip_event_destroy(void *event);
int pdehip_event_record(void *event, void *stream);
int pdehip_event_synchronize(void *event);
int pdehip_event_elapsed_ms(void *start, void *stop, float *ms);

/* Device layout of a full array of this grid.  out8 = { pitch of normalised axis 0, pitch of
 * normalised axis 1, elements per component, offset of interior cell (0,..,0), column of the
 * first interior cell in a row, elements to allocate for ONE component incl. tail slack,
 * tail slack, pitch (elements) of one layer along the grid's axis 0 }.  A device full array
 * of `ncomp` components needs (ncomp * out8[2] + out8[6]) elements. */
int pdehip_layout(const pdehip_grid_t *g, int64_t *out8);

/* ---- data movement between the valid and the full layout ----------------------
 * replaces NumpyBackend.make_valid_data_setter (pde/backends/numpy/backend.py:72-115) */
int pdehip_valid_to_full(const pdehip_grid_t *g, int ncomp, const void *valid, void *full,
                         void *stream);
int pdehip_full_to_valid(const pdehip_grid_t *g, int ncomp, const void *full, void *valid,
                         void *stream);
/* The same between HOST memory and a device full array, complete on return: the valid data of a field as the
 * reference holds it — `field.data` is a strided view of the ghost-padded host array (pde/fields/base.py:116-160,
 * pde/grids/base.py:329-337) — uploaded from / downloaded into that view without a contiguous host copy.
 * host_strides[4] (bytes): { between components, along the grid's axes right-aligned to three (entries of axes the
 * grid does not have are ignored) }; the fastest axis must be contiguous (host_strides[3] == element size, else
 * PDEHIP_E_VALUE).  Contiguous host memory: one hipMemcpy; windows: rows gathered / scattered through pinned chunks
 * while the DMA engine works, large fields on several threads.  Replaces the host side of TorchBackend.numpy_to_native /
 * native_to_numpy (pde/backends/torch/backend.py:217-260). */
int pdehip_upload_valid(const pdehip_grid_t *g, int ncomp, const void *host, const int64_t *host_strides,
                        void *full, void *stream);
int pdehip_download_valid(const pdehip_grid_t *g, int ncomp, const void *full, void *host,
                          const int64_t *host_strides, void *stream);
/* `hostfull` = a device copy of the reference's compact host full array (shape + 2 per axis,
 * `field._data_full`, pde/fields/datafield_base.py:93-126), ghost cells included */
int pdehip_hostfull_to_full(const pdehip_grid_t *g, int ncomp, const void *hostfull_dev,
                            void *full, void *stream);
int pdehip_full_to_hostfull(const pdehip_grid_t *g, int ncomp, const void *full,
                            void *hostfull_dev, void *stream);

/* ---- ghost cells ---------------------------------------------------------------
 * replaces NumbaBackend.make_ghost_cell_setter (pde/backends/numba/backend.py:184-404) */
int pdehip_set_ghost_cells(const pdehip_grid_t *g, int ncomp, const pdehip_bc_face_t *faces,
                           void *data_full, void *stream);

/* ---- operators (no BCs: the caller guarantees ghost cells are set) ---------------
 * replace the closures returned by make_laplace / make_gradient / make_divergence
 * (pde/backends/numba/operators/cartesian.py:332-383, :553-587, :962-996), signature
 * (arr_full, out_valid) of BackendBase.make_operator_no_bc (pde/backends/base.py:482-521).
 * `out_layout` selects whether `out` is a valid or a full array (the interior of a full
 * array is written, its ghost cells are left untouched). */
int pdehip_laplace(const pdehip_grid_t *g, const void *in_full, void *out, int out_layout,
                   void *stream);
/* The SPECTRAL Laplacian of periodic 1-D / 2-D grids: out = ifft(factor * fft(in)).real with factor = -(2 pi fftfreq)^2 summed over the
 * axes - `_make_laplace_numba_spectral_1d` / `_2d`, pde/backends/numba/operators/cartesian.py:232-330, chosen by `spectral=True` /
 * `use_spectral` (:359-372).  The transform is hipFFT's (loaded at run time); ghost cells of in_full are not read (every axis is
 * periodic: the caller checks).  3-D: error "not implemented", like the reference (:369-370). */
int pdehip_laplace_spectral(const pdehip_grid_t *g, const void *in_full, void *out, int out_layout, void *stream);
int pdehip_gradient(const pdehip_grid_t *g, int method, const void *in_full, void *out,
                    int out_layout, void *stream);
int pdehip_divergence(const pdehip_grid_t *g, int method, const void *in_full, void *out,
                      int out_layout, void *stream);
/* sum_a (d_a f)^2, pde/backends/numba/operators/cartesian.py:590-809; central != 0 selects
 * the central-difference form */
int pdehip_gradient_squared(const pdehip_grid_t *g, int central, const void *in_full, void *out,
                            int out_layout, void *stream);

/* 2-D Laplacian with the nine-point stencil (pde/backends/numba/operators/cartesian.py:153-190; `corner_weight` w: 1/2
 * Oono-Puri, 1/3 Mehrstellen; w = 0 is pdehip_laplace).  The four CORNER ghost cells of `in_full` are written first, as the
 * reference's make_corner_point_setter_2d does (:36-78: copies across a periodic axis — periodic2 = grid.periodic —, else
 * the mean of the two adjacent face ghosts); the face ghost cells must be set by the caller.  This is the one operator
 * that writes its input (SURVEY.md 8b "ownership"). */
int pdehip_laplace9(const pdehip_grid_t *g, const int *periodic2, double corner_weight, void *in_full, void *out,
                    int out_layout, void *stream);

/* first (order = 1, `method` as above) or second (order = 2, central) derivative along ONE axis:
 * the `d_dx`, `d_dy_forward`, `d2_dx2`, ... pattern operators of NumbaBackend.get_operator_info
 * (pde/backends/numba/backend.py:119-182), formulas of make_derivative / make_derivative2
 * (pde/backends/numba/operators/common.py:19-193): (r - l) / (2 dx), (r - c) / dx, (c - l) / dx,
 * (r - 2 c + l) * (1 / dx**2) */
int pdehip_axis_derivative(const pdehip_grid_t *g, int axis, int order, int method, const void *in_full,
                           void *out, int out_layout, void *stream);

/* ---- fused stencil + pointwise kernels (all arrays full) --------------------------
 * out = s2 * (s1 * laplace(in))                       [k = dt * (D * lap), RK stages] */
int pdehip_laplace_scaled(const pdehip_grid_t *g, const void *in_full, void *out_full, double s1,
                          double s2, void *stream);
/* out = y + s2 * (s1 * laplace(in)); y may alias in    [Euler: pde/solvers/euler.py:172-175] */
int pdehip_laplace_euler(const pdehip_grid_t *g, const void *in_full, const void *y_full,
                         void *out_full, double s1, double s2, void *stream);
/* TWO explicit Euler steps of the diffusion equation in one sweep (temporal blocking):
 *     out = E(E(in)),  E(u) = u + dt * (D * laplace(u)) with the BCs `faces` applied to u
 * i.e. two iterations of the loop body of pde/backends/numba/_solvers.py:98-108 with
 * pde/solvers/euler.py:172-175 and pde/pdes/diffusion.py:119-121, bit-identical to two single steps;
 * the intermediate level lives in registers only, ghost cells of `in` are neither read nor written.
 * Covers 3-D grids whose fastest axis is a multiple of 64 x 16 bytes, an even number of rows, >= 4 cells
 * per axis, and faces that are periodic or scalar first-order (Dirichlet / Neumann / mixed) per axis pair.
 * *done = 0 and nothing is written when the case is not covered (pdehip_euler_run then falls back to
 * single steps by itself). */
int pdehip_diffusion_euler2(const pdehip_grid_t *g, const pdehip_bc_face_t *faces, const void *in_full,
                            void *out_full, double diffusivity, double dt, int *done, void *stream);
/* `nsteps` (1..8 for the diffusion equation, 1..4 for Cahn-Hilliard) explicit Euler steps of a 2-D grid in ONE launch: a
 * workgroup keeps a tile plus halo in LDS and advances it through all time levels (temporal blocking), BCs applied to every
 * level — bit-identical to `nsteps` iterations of the loop body of pde/backends/numba/_solvers.py:98-108 (euler.py:172-175 with
 * diffusion.py:119-121 / cahn_hilliard.py:115-122).  For grids of a few MB (BASELINE configs 1-3), where a step per launch is
 * bound by launch and cache latency, not by HBM.  *done = 0 (nothing written) when the grid is not 2-D, a face is not periodic
 * / scalar first-order with the virtual point from the adjacent cell, or `nsteps` is out of range; pdehip_euler_run uses it by
 * itself and falls back to the register-pipelined kernels. */
int pdehip_euler_multi_2d(const pdehip_grid_t *g, const pdehip_rhs_t *rhs, const void *in_full, void *out_full, double dt,
                          int nsteps, int *done, void *stream);
/* The same two steps on a sub-slab of layers of a larger array (building block of pdehip_slab_euler2_run): `g_sub` has
 * the extent of the sub-slab along axis 0, `in_full` / `out_full` point ONE LAYER BEFORE its first layer, and the array
 * holds TWO real layers beyond the sub-slab on the sides named by `halo_sides` (1 = both sides, 2 = upper side only, the
 * lower face is the physical face `faces[0]`; 3 = lower side only, upper face `faces[1]`, index1 = extent - 1).  Replaces
 * the _MPIBC virtual points of pde/grids/boundaries/local.py:561-662 for both time levels. */
int pdehip_diffusion_euler2_slab(const pdehip_grid_t *g_sub, const pdehip_bc_face_t *faces, const void *in_full,
                                 void *out_full, double diffusivity, double dt, int halo_sides, int *done, void *stream);
/* ONE sweep for the Cahn-Hilliard right-hand side (pde/pdes/cahn_hilliard.py:115-122): mu = c^3 - c - gamma*laplace(c)
 * with the faces of c, then laplace(mu) with the faces of mu; mu lives in registers only (same two-level kernel as
 * pdehip_diffusion_euler2, bit-identical to pdehip_cahn_hilliard_mu + pdehip_laplace_euler / _scaled):
 *     euler != 0: out = c + dt * laplace(mu)   (one explicit Euler step)      euler == 0: out = dt * laplace(mu)
 * *done = 0 and nothing written when grid / faces are not covered (same rules as pdehip_diffusion_euler2, and the
 * faces of c and mu must be periodic on the same axes); pdehip_rhs_scaled / pdehip_euler_run use it by themselves. */
int pdehip_cahn_hilliard_fused(const pdehip_grid_t *g, const pdehip_bc_face_t *faces_c,
                               const pdehip_bc_face_t *faces_mu, const void *c_full, void *out_full, double gamma,
                               double dt, int euler, int *done, void *stream);
/* mu = c*c*c - c - gamma * laplace(c)                  [pde/pdes/cahn_hilliard.py:116-120] */
int pdehip_cahn_hilliard_mu(const pdehip_grid_t *g, const void *c_full, void *mu_full,
                            double gamma, void *stream);

/* ---- pointwise helpers over the interior of full arrays ----------------------------
 * out = y + sum_j coef[j] * k[j], evaluated left to right (pde/solvers/runge_kutta.py:135-153);
 * n <= 6; y == NULL drops the leading term (then out = coef[0]*k[0] + ...) */
int pdehip_lincomb(const pdehip_grid_t *g, int ncomp, void *out_full, const void *y_full, int n,
                   const double *coef_host, const void *const *k_full_host, void *stream);
/* y += (k1 + 2*k2 + 2*k3 + k4) / 6                     [pde/solvers/runge_kutta.py:60] */
int pdehip_rk4_combine(const pdehip_grid_t *g, int ncomp, void *y_full, const void *k1,
                       const void *k2, const void *k3, const void *k4, void *stream);
/* y += dt * (1.5 * rate_cur - 0.5 * rate_prev)        [Adams-Bashforth: pde/solvers/adams_bashforth.py:41-44,
 * pde/backends/numba/_solvers.py:160-167; the rates are unscaled right-hand sides = pdehip_rhs_scaled with dt = 1] */
int pdehip_ab2_combine(const pdehip_grid_t *g, int ncomp, void *y_full, const void *rate_cur,
                       const void *rate_prev, double dt, void *stream);
/* RKF45 tail (pde/solvers/runge_kutta.py:146-152):
 *   err  = max | r1 k1 + r3 k3 + r4 k4 + r5 k5 + r6 k6 |   -> *err_dev (fp64 device scalar)
 *   ynew = y + c1 k1 + c3 k3 + c4 k4 + c5 k5
 * *err_dev is reset by the call; NaN propagates like numpy's max. */
int pdehip_rkf45_combine(const pdehip_grid_t *g, int ncomp, const void *y, void *ynew,
                         const void *const *k6_host, double *err_dev, void *stream);
/* max |a - b| over the interior -> *out_dev (generic error estimate pde/solvers/base.py:416) */
/* *out_dev = max |z| over complex data held as pairs of real components of the full array (component 2p = real part, 2p + 1 =
 * imaginary part): the error norm `np.abs(error).max()` of the adaptive schemes when the state is complex
 * (pde/solvers/runge_kutta.py:147-148, pde/solvers/euler.py:253; complex states: pde/solvers/controller.py:430-432).  NaN wins. */
int pdehip_max_abs_pairs(const pdehip_grid_t *g, int npairs, const void *arr_full, double *out_dev, void *stream);
/* End of an adaptive Euler attempt, pde/backends/numba/_solvers.py:381-394 (numpy twin pde/solvers/euler.py:238-256):
 *   out = half + k                       `step_small += 0.5 * dt * rate_midpoint`   (k = that product, half = state + dt/2 * rate)
 *   *err_dev = max |(y + dt * rate) - out|      `np.abs(step_large - step_small).max()`, step_large is never stored
 * The loops below compute the same inside the sweep that produces k (stage kind 4). */
int pdehip_euler_adaptive_combine(const pdehip_grid_t *g, int ncomp, const void *y_full, const void *rate_full, double dt,
                                  const void *half_full, const void *k_full, void *out_full, double *err_dev, void *stream);
int pdehip_max_abs_diff(const pdehip_grid_t *g, int ncomp, const void *a_full, const void *b_full,
                        double *out_dev, void *stream);

/* y += scale * xi over the interior, xi ~ N(0, 1) independent per cell: the noise increment of an Euler-Maruyama step
 * (pde/solvers/euler.py:66-147: `state += sqrt(dt) * sqrt(noise_variance / cell_volume) * dW`; the reference draws dW with
 * numba's / torch's generator, pde/backends/numba/backend.py make_gaussian_noise, pde/backends/torch/backend.py:603-625).
 * Counter-based generator: xi of cell q (C-order index of the VALID array, component-major) in call number `counter` is
 * Box-Muller(Philox4x32-10(key = seed, counter = {q_lo, q_hi, counter_lo, counter_hi})) — reproducible for a given seed, independent of the
 * launch geometry and of how the grid is split over devices (pass the global cell offset of the slab in `cell_offset`). */
int pdehip_add_gaussian_noise(const pdehip_grid_t *g, int ncomp, void *y_full, double scale, uint64_t seed, uint64_t counter,
                              uint64_t cell_offset, void *stream);

/* out_dev[c] = cell_volume * sum over the interior of component c (fp64 device scalars, one per component): the integral of
 * a field on a Cartesian grid (uniform cell volumes) — NumbaBackend.make_integrator (pde/backends/numba/backend.py:555-652),
 * used by conservation checks and post-step logic without moving the field to the host.  Two passes (per-workgroup partial
 * sums, then one workgroup): the result does not depend on scheduling; it differs from the reference's sequential sum by
 * the usual reordering error (relative 1e-13 at 512^3). */
int pdehip_integrate(const pdehip_grid_t *g, int ncomp, const void *arr_full, double cell_volume, double *out_dev, void *stream);
/* out_dev[c] = number of cells of component c that are NaN or +-inf (as a double): the check of the reference's
 * ConsistencyTracker (`np.all(np.isfinite(field.data))`, pde/trackers/trackers.py:974-1003) without moving the field to the host -
 * 8 bytes per component cross PCIe instead of the whole state at every interrupt. */
int pdehip_count_nonfinite(const pdehip_grid_t *g, int ncomp, const void *arr_full, double *out_dev, void *stream);

/* ---- fused time steppers ----------------------------------------------------------
 * k_out = dt * rhs(y): applies the BCs of y (and of mu) — on the fly inside the stencil kernel where the
 * faces allow it, else by setting the ghost cells in place — then evaluates the RHS;
 * replaces NumbaBackend.make_pde_rhs + the `dt * rhs(...)` temporaries
 * (pde/backends/numba/backend.py:1158-1196, pde/solvers/runge_kutta.py:52-59) */
int pdehip_rhs_scaled(const pdehip_grid_t *g, const pdehip_rhs_t *rhs, void *y_full,
                      void *k_out_full, double dt, void *stream);
/* `nsteps` explicit Euler steps with fixed dt, ping-ponging between buf_a (initial state)
 * and buf_b; *result receives the buffer holding the final state (which of the two depends on the number
 * of sweeps: the diffusion RHS advances two steps per sweep where pdehip_diffusion_euler2 covers the grid).
 * Replaces the jitted
 * fixed-step loop (pde/backends/numba/_solvers.py:93-104) around
 * EulerSolver._make_single_step_fixed_dt (pde/solvers/euler.py:149-179). */
int pdehip_euler_run(const pdehip_grid_t *g, const pdehip_rhs_t *rhs, void *buf_a, void *buf_b,
                     double dt, int64_t nsteps, void **result, void *stream);
/* one classical RK4 step in place on y (pde/solvers/runge_kutta.py:29-66);
 * work = 5 full arrays (scratch: slopes and stage inputs; their contents after the call are unspecified).
 * Where the stencil kernels cover grid and faces every stage is ONE sweep: the slope and, from the slope still in
 * registers, the input of the next stage / the new state (17 instead of 23 arrays moved per step); the result is
 * bit-identical to the sequence rhs_scaled + lincomb + rk4_combine, which remains the fallback. */
int pdehip_rk4_step(const pdehip_grid_t *g, const pdehip_rhs_t *rhs, void *y_full,
                    void *const *work5_host, double dt, void *stream);
/* One Adams-Bashforth step (pde/solvers/adams_bashforth.py:40-47) in ONE sweep: rate_cur = rhs(y_in) (kept for the
 * next step) and y_out = y_in + dt * (1.5 * rate_cur - 0.5 * rate_prev), bit-identical to pdehip_rhs_scaled(dt = 1) +
 * pdehip_ab2_combine.  *fused = 0 and nothing launched where the stencil kernels do not carry the stage epilogue
 * (1-D, odd rows, faces the two-level kernel does not cover for Cahn-Hilliard): the caller runs those two. */
int pdehip_ab2_step(const pdehip_grid_t *g, const pdehip_rhs_t *rhs, void *y_in_full, void *y_out_full,
                    void *rate_cur_full, const void *rate_prev_full, double dt, int *fused, void *stream);
/* `nsteps` RK4 steps with fixed dt in place on y: the fixed-step loop (pde/backends/numba/_solvers.py:93-104) around
 * pdehip_rk4_step.  Small grids (launch-bound) replay a cached hipGraph of 8 steps, like pdehip_euler_run. */
int pdehip_rk4_run(const pdehip_grid_t *g, const pdehip_rhs_t *rhs, void *y_full, void *const *work5_host,
                   double dt, int64_t nsteps, void *stream);
/* one RKF45 attempt (pde/solvers/runge_kutta.py:68-156): ynew and *err_dev are produced,
 * y is unchanged apart from its ghost cells; work = 7 full arrays (scratch: k1..k6, tmp; contents unspecified after
 * the call, ynew doubles as a stage input until the last sweep).  Fused like pdehip_rk4_step: six sweeps, the last
 * one computes the new state and the max-norm of the error estimate from k6 in registers (36 instead of 45 arrays). */
int pdehip_rkf45_attempt(const pdehip_grid_t *g, const pdehip_rhs_t *rhs, void *y_full,
                         void *ynew_full, void *const *work7_host, double dt, double *err_dev,
                         void *stream);

/* ---- slab-parallel layer: one process per GPU, axis-0 slabs, RCCL over xGMI -----------------------
 * Replaces the reference's MPI path: face exchange inside every right-hand side
 * (pde/backends/numba_mpi/backend.py:30-194, pde/grids/boundaries/local.py:561-662), the MAX
 * all-reduce of the adaptive error (pde/backends/base.py:678-712) and the MPI stepper wrapper
 * (pde/solvers/explicit_mpi.py:133-226).  `librccl_path` names the librccl.so already loaded in the
 * process (RCCL is resolved with dlsym, not linked).  Rank 0 creates a 128-byte unique id, the host
 * distributes it, every rank calls pdehip_comm_create.  `lower` / `upper` are the neighbour ranks
 * along axis 0 (-1 = physical boundary). */
int pdehip_comm_unique_id(const char *librccl_path, void *id128);
int pdehip_comm_create(const char *librccl_path, const void *id128, int rank, int size, void **comm);
int pdehip_comm_destroy(void *comm);
/* What RCCL reports about the communicator (ABI version 7; measurement aid: the N > 1 bench line records that RCCL really spans N ranks on N
 * devices): out5 = {ncclCommCount, ncclCommUserRank, ncclCommCuDevice, ncclGetVersion, HIP device of the caller}, -1 where unavailable;
 * pci_bus_id (>= 16 bytes) = hipDeviceGetPCIBusId of that device.  Reference counterpart: MPI.COMM_WORLD.size / rank of pde/tools/mpi.py:40-61. */
int pdehip_comm_info(void *comm, int *out5, char *pci_bus_id, size_t n);
/* send valid layers 1 / n of the local slab to the neighbours, receive their layers into the ghost
 * layers n+1 / 0 (ncclSend/ncclRecv in one group, enqueued on `stream`) */
int pdehip_halo_exchange(void *comm, const pdehip_grid_t *g_local, void *buf_full, int lower, int upper,
                         void *stream);
/* in-place MAX over all ranks of one fp64 device scalar; NaN wins like numpy.max */
int pdehip_allreduce_max(void *comm, double *dev_scalar, void *stream);
/* `nsteps` Euler steps of the diffusion right-hand side on the local slab: the exchange of the new
 * boundary layers overlaps the interior kernel (second HIP stream); no host synchronisation */
int pdehip_slab_euler_run(void *comm, const pdehip_grid_t *g_local, const pdehip_rhs_t *rhs, int lower,
                          int upper, void *buf_a, void *buf_b, double dt, int64_t nsteps, void **result,
                          void *stream);
/* Same contract, two steps per sweep (see pdehip_diffusion_euler2): TWO layers per side are exchanged once
 * per two steps, so both the HBM traffic per step and the number of exchanges are halved.  The slab is worked
 * on in a private copy with two halo layers per side; the result is written back to `buf_a` (*result).
 * Preconditions the CALLER checks globally (all ranks must take the same path): both neighbours exist on every
 * rank (periodic slowest axis; replaces the _MPIBC exchange of pde/grids/boundaries/local.py:561-662 for both
 * levels), >= 4 local layers on every rank, and *ok != 0 from pdehip_slab_euler2_supported (grid shape, dtype
 * and the faces of the two other axes are covered by the kernel).  E_NOTIMPL otherwise. */
int pdehip_slab_euler2_supported(const pdehip_grid_t *g_local, const pdehip_rhs_t *rhs, int *ok);
/* Cahn-Hilliard right-hand side on a slab in ONE sweep (pdehip_cahn_hilliard_fused with real halo layers on the slowest
 * axis): two layers of c per side are exchanged, mu needs no exchange of its own (the reference exchanges c and mu,
 * one layer each, per evaluation).  `c_ext` / `out_ext` are slab arrays with TWO halo layers per side (the layout of a
 * slab of n+2 layers; own layers 2..n+1).  euler != 0: out = c + dt*laplace(mu); euler == 0: out = dt*laplace(mu).
 * Same global preconditions as pdehip_slab_euler2_run, with >= 2 own layers per rank and pdehip_slab_ch_supported. */
int pdehip_slab_ch_supported(const pdehip_grid_t *g_local, const pdehip_rhs_t *rhs, int *ok);
int pdehip_slab_ch_sweep(void *comm, const pdehip_grid_t *g_local, const pdehip_rhs_t *rhs, int lower, int upper,
                         void *c_ext, void *out_ext, double dt, int euler, void *stream);
int pdehip_slab_euler2_run(void *comm, const pdehip_grid_t *g_local, const pdehip_rhs_t *rhs, int lower,
                           int upper, void *buf_a, void *buf_b, double dt, int64_t nsteps, void **result,
                           void *stream);
/* Scratch buffers of the process-wide context that serves the slab / block loops WITHOUT a communicator (comm == NULL: one process, no
 * neighbours): freed here (after the runs that use them), allocated again on demand.  A communicator frees its own in pdehip_comm_destroy.
 * (ABI version 7; the reference has no counterpart: numpy arrays are garbage-collected.) */
int pdehip_release_scratch(void);
/* Communication-avoiding variant (ABI version 7): FOUR halo layers per side, ONE exchange per FOUR steps (two two-step sweeps per group).
 * Default schedule (3; PDEHIP_SLAB_DEEP_MODE = 1..4 selects another, read per call): FOUR private arrays with four halo layers per side -
 * three state arrays in rotation (cur -> mid -> nxt) and one scratch array.  The compute stream runs the two interior sweeps of a group
 * (the layers that read own cells only); the halo stream computes the four boundary layers per exchanged side of `nxt` a whole group
 * ahead - straight from `cur` and its halos, in two short two-step passes through the scratch array - and sends / receives them, so the
 * exchange and the boundary work stay off the critical path and the two chains meet once per group.  Schedule 4: the second boundary pass
 * reads what the first interior sweep produced instead of recomputing it.  Schedules 1 and 2 (two private arrays): every sweep on ONE
 * stream, the first sweep of a group computes two layers more per exchanged side and is cut into an interior launch, which runs while the
 * exchange of the group before is in flight, and a boundary launch that waits for it (2: the second sweep is cut too); the halo stream
 * carries ncclSend / ncclRecv only.  Every schedule computes each cell from the same inputs in the same order: bit-identical results.
 * Replaces the blocking per-step exchange of pde/solvers/explicit_mpi.py:133-226 + pde/backends/numba_mpi/backend.py:163-194.  Same
 * contract and preconditions as pdehip_slab_euler2_run, with >= 8 local layers on EVERY rank (the caller checks globally) and *ok != 0
 * from pdehip_slab_euler4_supported. */
int pdehip_slab_euler4_supported(const pdehip_grid_t *g_local, const pdehip_rhs_t *rhs, int *ok);
int pdehip_slab_euler4_run(void *comm, const pdehip_grid_t *g_local, const pdehip_rhs_t *rhs, int lower,
                           int upper, void *buf_a, void *buf_b, double dt, int64_t nsteps, void **result,
                           void *stream);

/* ---- slab-parallel Runge-Kutta and the adaptive loop (one C call per run: no host work per stage) ----------------
 * `flags` (PDEHIP_SLAB_*) select code paths that every rank must take alike; the caller ANDs the local answers of
 * pdehip_slab_flags_supported over all ranks (MIN all-reduce) before the first call.  Arrays that serve as stage inputs
 * (y, ynew, work[3] (k4), the last work array (tmp)) — simplest: ALL slab arrays — must be allocated with one spare layer
 * (pdehip_layout out8[7] elements) before and after, because the fused Cahn-Hilliard sweep reads TWO halo layers per side
 * (exchanged into that spare room).  `comm` may be NULL when lower == upper == -1 (single process, no exchange): the same
 * loops then serve the serial adaptive stepper. */
enum {
    PDEHIP_SLAB_FUSED_CH = 1,    /* Cahn-Hilliard right-hand side as one two-level sweep after ONE exchange of two layers of c */
    PDEHIP_SLAB_FUSED_STAGE = 2  /* Runge-Kutta combination inside the sweep that computes the slope */
};
int pdehip_slab_flags_supported(const pdehip_grid_t *g_local, const pdehip_rhs_t *rhs, int lower, int upper, int *flags);
/* k_out = dt * rhs(y) on the slab incl. the halo exchange(s): replaces NumbaMPIBackend's operator + _MPIBC exchange per
 * right-hand side (pde/backends/numba_mpi/backend.py:30-194) */
int pdehip_slab_rhs_scaled(void *comm, const pdehip_grid_t *g_local, const pdehip_rhs_t *rhs, int lower, int upper, int flags,
                           void *y_full, void *k_out_full, double dt, void *stream);
/* `nsteps` Euler steps of ANY fused right-hand side, one exchange + sweep per step (Cahn-Hilliard; the diffusion equation has
 * the overlapped loops pdehip_slab_euler_run / pdehip_slab_euler2_run) */
int pdehip_slab_euler_sweeps(void *comm, const pdehip_grid_t *g_local, const pdehip_rhs_t *rhs, int lower, int upper, int flags,
                             void *buf_a, void *buf_b, double dt, int64_t nsteps, void **result, void *stream);
/* `nsteps` classical RK4 steps in place on y (pde/solvers/runge_kutta.py:29-66, loop pde/backends/numba/_solvers.py:93-104) */
int pdehip_slab_rk4_run(void *comm, const pdehip_grid_t *g_local, const pdehip_rhs_t *rhs, int lower, int upper, int flags,
                        void *y_full, void *const *work5_host, double dt, int64_t nsteps, void *stream);
/* Adaptive RKF45 from t_start to t_end: the loop of pde/backends/numba/_solvers.py:249-281 with the controller of
 * pde/solvers/base.py:572-592 and the MAX all-reduce of the error estimate (pde/backends/base.py:678-712).  In: t_start, t_end,
 * dt (first trial step), tolerance, dt_min, dt_max; the counters and statistics are ACCUMULATED (zero them before the first
 * call of a run).  Out: dt (next trial step), t_last, steps, attempts, statistics of the accepted steps.  *result = y or ynew,
 * whichever holds the final state.  A step size below dt_min is reported as an error (code 3) with the reference's message. */
typedef struct pdehip_adaptive {
    double t_start, t_end, dt, tolerance, dt_min, dt_max;
    double t_last;
    int64_t steps, attempts;
    int64_t stat_count;
    double stat_min, stat_max, stat_mean, stat_m2;
} pdehip_adaptive_t;
int pdehip_slab_rkf45_run(void *comm, const pdehip_grid_t *g_local, const pdehip_rhs_t *rhs, int lower, int upper, int flags,
                          void *y_full, void *ynew_full, void *const *work7_host, double *err_dev, pdehip_adaptive_t *ctl,
                          void **result, void *stream);

/* ADAPTIVE EULER from t_start to t_end - the reference's own loop `_make_adaptive_stepper_euler`, pde/backends/numba/_solvers.py:322-466
 * (numpy twin pde/solvers/euler.py:181-283), NOT the generic one-step-versus-two-half-steps estimate: the rate of the current state
 * is carried from attempt to attempt (a rejected attempt re-uses it), and after an accepted attempt the new rate is evaluated at the
 * time BEFORE `t += dt` (:402-407) - with time-dependent conditions or explicit time in the equation results and step counts depend
 * on that.  Control block and error handling as pdehip_slab_rkf45_run; work3 = rate, half step, slope scratch (slab arrays: the
 * half step is a sweep input).  Two sweeps per accepted attempt where the stage epilogues cover the grid (kinds 0 and 4). */
int pdehip_slab_euler_adaptive_run(void *comm, const pdehip_grid_t *g_local, const pdehip_rhs_t *rhs, int lower, int upper, int flags,
                                   void *y_full, void *ynew_full, void *const *work3_host, double *err_dev, pdehip_adaptive_t *ctl,
                                   void **result, void *stream);
/* the same on one device (no communicator, flags decided here) */
int pdehip_euler_adaptive_run(const pdehip_grid_t *g, const pdehip_rhs_t *rhs, void *y_full, void *ynew_full, void *const *work3_host,
                              double *err_dev, pdehip_adaptive_t *ctl, void **result, void *stream);

/* ---- BLOCK decomposition: one process per GPU owns a box of the grid (e.g. 2 x 2 x 2 for 512^3 on 8 GPUs) -----------------------
 * Replaces GridMesh with a multi-axis decomposition (pde/grids/_mesh.py:59-93 `_get_optimal_decomposition`, :401-444 neighbours) and the
 * face exchange `_MPIBC` of every decomposed axis (pde/grids/boundaries/local.py:561-662).  nb6[2 * axis + side] = rank of the neighbour
 * across that face of the local block, or -1 for a physical face (whose condition stays in the face tables of `rhs`; periodic axes
 * with ONE block keep their periodic condition).  One ghost layer per face; faces normal to the fast axes travel through packed
 * staging buffers.  Why: per xGMI link a 256^3 block moves 0.5 MiB per face where a 64 x 512 x 512 slab moves 2 MiB (xGMI is point
 * to point), see csrc/pdehip_block_loops.h. */
/* fill the ghost layers of buf_full on all faces that have a neighbour (one RCCL group) */
int pdehip_block_exchange(void *comm, const pdehip_grid_t *g_local, const int *nb6, void *buf_full, void *stream);
/* time loops on a block, ONE call per run: scheme 0 = `nsteps` explicit Euler steps (y_full / ynew_full ping-pong, *result names
 * the final one), 1 = `nsteps` RK4 steps in place (work: k1..k4, tmp), 2 = the adaptive RKF45 loop `ctl` incl. the MAX all-reduce
 * of the error (work: k1..k6, tmp), 3 = the reference's adaptive Euler loop `ctl` (pdehip_slab_euler_adaptive_run; work: rate, half
 * step, slope scratch).  Every right-hand side exchanges the faces of its input first (Cahn-Hilliard: c, then mu - the
 * reference's sequence); fuse_stage != 0: diffusion stages carry their Runge-Kutta combination (decide it for ALL ranks alike).
 * The time of the first step is rhs->t. */
int pdehip_block_run(void *comm, const pdehip_grid_t *g_local, const pdehip_rhs_t *rhs, const int *nb6, int fuse_stage, int scheme,
                     void *y_full, void *ynew_full, void *const *work_host, double *err_dev, double dt, int64_t nsteps,
                     pdehip_adaptive_t *ctl, void **result, void *stream);

/* ---- products of tensor fields, cell by cell (ABI version 6) ------------------------------------------------------------------------
 * Replaces BackendBase.make_inner_prod_operator / make_outer_prod_operator (pde/backends/base.py:567-610; numpy: np.einsum per rank
 * combination, pde/backends/numpy/backend.py:285-363; numba: pde/backends/numba/backend.py:654-893), which `DataFieldBase.dot` /
 * `VectorField.outer_product` / `make_dot_operator` use (pde/fields/datafield_base.py:965).  kind 0: vector . vector -> scalar, 1: tensor
 * . vector -> vector, 2: vector . tensor -> vector, 3: tensor . tensor -> tensor, 4: outer product of two vectors -> tensor; the vector
 * dimension is g->ndim; all arrays FULL, component-major (tensor entries in C order).  complex_pairs != 0: every tensor entry is a
 * planar (re, im) pair (the layout of complex states, pde_hip/complex_expr.py); conjugate != 0: the second operand is conjugated
 * (the reference's default for `dot`). */
int pdehip_field_product(const pdehip_grid_t *g, int kind, int complex_pairs, int conjugate, const void *a_full, const void *b_full,
                         void *out_full, void *stream);

/* ---- the FAST block decomposition: two Euler steps per sweep on a box, halos two layers deep incl. the edges, ONE message per
 * neighbouring rank, the exchange hidden behind the next sweep (csrc/pdehip_block2_loops.h; ABI version 6) -------------------------
 * Replaces the same reference code as pdehip_block_run (GridMesh pde/grids/_mesh.py:59-93, :401-444; the blocking face exchange inside
 * every right-hand side pde/backends/numba_mpi/backend.py:163-194, pde/grids/boundaries/local.py:561-662) for the case the benchmark
 * runs: DiffusionPDE, fixed-step Euler, a 3-D grid that is periodic on every axis.  dims3 / coords3: blocks per axis and the block of
 * this rank (ranks in C order of the block indices, like GridMesh); cut3[a] != 0: axis a is exchanged (several blocks - or one block
 * that sends its halo to itself: the probe of the exchange path on one device), else it wraps inside the kernels.  A cut of the fastest
 * axis is covered for fp64 (its halo cells live in the padding of the rows); where pdehip_block2_supported answers 0 the caller takes
 * pdehip_block_run.  buf_a: the state (full array of
 * g_local), advanced in place by `nsteps` (EVEN) steps; buf_b is not touched (kept for the signature of the other loops).
 * Bit-identical to single steps. */
int pdehip_block2_supported(const pdehip_grid_t *g_local, const pdehip_rhs_t *rhs, const int *cut3, int *ok);
int pdehip_block2_euler_run(void *comm, const pdehip_grid_t *g_local, const pdehip_rhs_t *rhs, const int *dims3, const int *coords3,
                            const int *cut3, void *buf_a, void *buf_b, double dt, int64_t nsteps, void **result, void *stream);

/* ---- run-time specialised right-hand sides (generic `PDE({...})` expressions) ----------------------
 * Replaces the sympy -> numba code generation of pde/pdes/pde.py:401-499 / pde/tools/expressions.py:
 * 361-388.  `epilogue_body` is the body of
 *     double pde_epilogue(double c, double lap, double gsq, double e0, double e1, double e2, const double *p)
 * (C statements ending in `return ...;`).  pdehip_jit_apply evaluates, for every interior cell,
 *     out = pde_epilogue(in, laplace(in), gradient_squared(in), extra[0], extra[1], extra[2], params)
 * in ONE pass of the register-pipelined stencil kernel compiled around the epilogue with hiprtc
 * (cached per tile shape); `in_faces` are evaluated on the fly / by the ghost kernel first (NULL: ghost
 * cells of `in_full` are already set).  All arrays are FULL arrays of the same grid. */
int pdehip_jit_create(const char *epilogue_body, void **handle);
int pdehip_jit_destroy(void *handle);
/* compile (not load) the kernels of this expression for a dtype / dimension: works without a GPU */
int pdehip_jit_check(void *handle, int dtype, int ndim);
int pdehip_jit_apply(void *handle, const pdehip_grid_t *g, void *in_full, const void *const *extra3_host,
                     void *out_full, const double *params_host, int nparams, const pdehip_bc_face_t *in_faces,
                     void *stream);
/* pdehip_jit_apply whose result is the slope k of a Runge-Kutta stage (the epilogue computes dt * F), followed in the
 * SAME sweep by the pointwise combination of the scheme (pde/solvers/runge_kutta.py:52-61, :135-150):
 *   kind 0: k_out = k,  out2 = y + sum_m coef[m] * k_prev[m] + c_new * k      (input of the next stage)
 *   kind 1: out2 = y + (k_prev[0] + 2 k_prev[1] + 2 k_prev[2] + k) / 6        (RK4 update; k_out unused, out2 may be y)
 *   kind 2: out2 = y + c1 k1 + c3 k3 + c4 k4 + c5 k5 and *err_dev = max |error estimate| with k6 = k,
 *           k_prev = {k1, k3, k4, k5}                                         (end of an RKF45 attempt)
 *   kind 4: out2 = k_prev[1] + k and *err_dev = max |(y + coef[0] * k_prev[0]) - out2| with k_prev = {carried rate, half step},
 *           coef[0] = dt, k = dt/2 * F(half step)                             (end of an adaptive Euler attempt, pdehip_euler_adaptive_combine)
 * Same expressions in the same order as pdehip_lincomb / pdehip_rk4_combine / pdehip_rkf45_combine: bit-identical to
 * pdehip_jit_apply followed by them.  *done = 0 (nothing launched) when only the generic kernel covers the grid. */
int pdehip_jit_apply_stage(void *handle, const pdehip_grid_t *g, void *in_full, const void *const *extra3_host,
                           void *k_out_full, const double *params_host, int nparams, const pdehip_bc_face_t *in_faces,
                           int kind, const void *y_full, int nk, const void *const *k_prev_host, const double *coef_host,
                           double c_new, void *out2_full, double *err_dev, int *done, void *stream);
/* TWO applications in one sweep: out = f(f(in)), f(u) = pde_epilogue(u, laplace(u), gradient_squared(u); params), with
 * the BCs `faces` applied to u before each application and the intermediate level in registers — two explicit Euler
 * steps of a one-pass expression PDE (epilogue = the Euler update `u + dt * F(u, ...)`; no extra arrays, no explicit
 * time).  Replaces two iterations of the fixed-step loop pde/backends/numba/_solvers.py:98-108 around the compiled
 * right-hand side of pde/pdes/pde.py:401-499.  *done = 0 (nothing launched) when grid or faces are not covered: same
 * rules as pdehip_diffusion_euler2; the caller then calls pdehip_jit_apply twice. */
int pdehip_jit_euler2(void *handle, const pdehip_grid_t *g, const void *in_full, void *out_full,
                      const double *params_host, int nparams, const pdehip_bc_face_t *faces, int *done, void *stream);
/* Two-pass expressions in ONE sweep (e.g. `laplace(c**3 - c - laplace(c))`, Swift-Hohenberg): handle from
 * pdehip_jit_create2(body1, body2);  tmp = body1(u, laplace u, gradient_squared u; params) is kept in registers,
 *     out = body2(tmp, laplace tmp, gradient_squared tmp, e0 = u; params)
 * with `faces_u` applied to u and `faces_tmp` to tmp (the reference applies them when it evaluates the inner and the
 * outer operator: pde/pdes/pde.py:299-399).  *done = 0 when grid / faces are not covered: the caller then runs the two
 * passes through pdehip_jit_apply. */
int pdehip_jit_create2(const char *body1, const char *body2, void **handle);
int pdehip_jit_fused2(void *handle, const pdehip_grid_t *g, const void *in_full, void *out_full,
                      const double *params_host, int nparams, const pdehip_bc_face_t *faces_u,
                      const pdehip_bc_face_t *faces_tmp, int *done, void *stream);

/* The fixed-step explicit Euler loop of an expression PDE (one or several scalar components) in ONE call: `nsteps` times the
 * sequence of passes, each pdehip_jit_apply of its handle, the state ping-ponging between two buffers.  Replaces the loop
 * pde/backends/numba/_solvers.py:98-108 (`for i in range(steps): t = t_start + i * dt; single_step(state, t)`) around
 * pde/solvers/euler.py:172-175 for the compiled right-hand sides of pde/pdes/pde.py:401-499 - a Python loop over the passes
 * costs 40-85 us per step on small grids where the kernels need 2-5 us (profiles/r02_time_small_expr.md).
 * Array indices of a pass: >= 0 selects fixed[index] (temporaries, constant arrays, coordinates); -1 - k selects component k
 * of the CURRENT state as `src` / `extras` and component k of the NEXT state as `out`; PDEHIP_JIT_NONE: no array.  The
 * epilogue of the pass that writes the next state must be the Euler update `state + dt * F` (parameters p[0] = dt,
 * p[1] = t).  state_a holds the state on entry; *result is the buffer that holds it afterwards.  uses_time = 0 allows replaying a
 * captured hipGraph for long runs (PDEHIP_JIT_GRAPH=1; measured slower than the plain launches of this loop, so off by default). */
#define PDEHIP_JIT_NONE INT32_MIN
/* DECOMPOSED grids (one box per GPU): a pass whose `exchange` is set fills the ghost layers of its `src` from the neighbours before it
 * runs - pdehip_halo_exchange (slab: lower / upper) or pdehip_block_exchange (blocks: nb6) on the loop's stream - like `_MPIBC` inside
 * every operator of the reference's MPI path (pde/grids/boundaries/local.py:561-662, pde/solvers/explicit_mpi.py:133-226).  The caller
 * sets it on the FIRST pass of an evaluation that applies operators to an array (the operand of a nested operator is an intermediate
 * field: exchanged like the state); the faces towards neighbours are PDEHIP_BC_SKIP in `faces`.  The adaptive loops reduce their
 * error norm over all ranks of `comm` (MAX, NaN wins: pde/backends/base.py:678-712). */
typedef struct {
    void *comm;
    int32_t blocks;          /* 0: axis-0 slab (lower / upper), 1: block decomposition (nb6) */
    int32_t lower, upper;
    int32_t nb6[6];
} pdehip_exchange_t;
typedef struct {
    void *handle;
    int32_t src;
    int32_t extras[3];
    int32_t out;
    const pdehip_bc_face_t *faces;   /* conditions applied to src before the pass (NULL: none) */
    const pdehip_exchange_t *exchange;   /* decomposed grids: exchange the ghost layers of src first (NULL: nothing) */
} pdehip_jit_pass_t;
int pdehip_jit_euler_run(const pdehip_grid_t *g, const pdehip_jit_pass_t *passes, int npasses, void *const *fixed, int nfixed,
                         void *state_a, void *state_b, int ncomp, double dt, double t0, int uses_time, int64_t nsteps,
                         void *bc_program, void **result, void *stream);
/* Runge-Kutta loops of an expression PDE in ONE call: `nsteps` classical RK4 steps with fixed dt (ctl == NULL;
 * pde/solvers/runge_kutta.py:29-66 inside the loop pde/backends/numba/_solvers.py:98-108), or the ADAPTIVE Runge-Kutta-Fehlberg
 * loop from ctl->t_start to ctl->t_end (runge_kutta.py:68-156 inside pde/backends/numba/_solvers.py:249-281 with the controller
 * pde/solvers/base.py:572-592; the host reads 8 bytes per attempt, nothing per stage).  The passes are those of
 * pdehip_jit_euler_run with another meaning of the state indices: -1 - k as `src` / `extras` is component k of the STAGE INPUT,
 * as `out` component k of the SLOPE; the epilogue of the passes that write a slope must compute `dt * F` (p[0] = dt of the
 * step, p[1] = time of the stage).  work: 5 (RK4: k1..k4, tmp) or 7 (RKF45: k1..k6, tmp) arrays of ncomp components each; y
 * is advanced in place (RK4) or ping-pongs with ynew (adaptive: *result names the array holding the final state).  A single-
 * component expression whose last pass runs on the vectorised kernel takes the stage epilogue of pdehip_jit_apply_stage
 * (stage_fuse bit 0); everything else combines with pdehip_lincomb / pdehip_rk4_combine / pdehip_rkf45_combine: bit-identical.
 * stage_fuse bit 1 (adaptive loops only): the components are the planar (re, im) PAIRS of complex fields - the error norm is the
 * modulus, `np.abs(error).max()` of a complex array (runge_kutta.py:147-148, pde/solvers/euler.py:253): new state and an explicit error
 * field through pdehip_lincomb, then pdehip_max_abs_pairs; the error field is ONE MORE work array (work[7]; adaptive Euler: work3[3]).
 * bc_program (or NULL): time-dependent faces, refreshed for every stage time. */
int pdehip_jit_rk_run(const pdehip_grid_t *g, const pdehip_jit_pass_t *passes, int npasses, void *const *fixed, int nfixed,
                      int ncomp, void *y, void *ynew, void *const *work_host, double *err_dev, double dt, double t0, int64_t nsteps,
                      pdehip_adaptive_t *ctl, int stage_fuse, void *bc_program, void **result, void *stream);

/* The reference's adaptive Euler loop (pde/backends/numba/_solvers.py:322-466) for an expression PDE in ONE call: passes as in
 * pdehip_jit_rk_run (the slope passes compute `p[0] * F`; the carried rate is obtained with p[0] = 1), work3 = rate, half step, slope
 * scratch (ncomp components each).  stage_fuse != 0: single-component expressions take the stage epilogues (kinds 0 and 4 of
 * pdehip_jit_apply_stage) where the vectorised kernel covers the grid. */
int pdehip_jit_euler_adaptive_run(const pdehip_grid_t *g, const pdehip_jit_pass_t *passes, int npasses, void *const *fixed, int nfixed,
                                  int ncomp, void *y, void *ynew, void *const *work3_host, double *err_dev, pdehip_adaptive_t *ctl,
                                  int stage_fuse, void *bc_program, void **result, void *stream);

/* ---- implicit Euler and Crank-Nicolson (ABI version 8) -------------------------------------------------------------------
 * The reference's fixed-point solvers: pde/solvers/implicit.py:74-110 (`state = state_t + dt * rhs(state, t + dt)`, first estimate
 * with rhs(state_t, t)) and pde/solvers/crank_nicolson.py:80-113 (`state_cn = state_t + dt / 2 * (rhs(state, t + dt) + rate_t)`,
 * `state = alpha * state + (1 - alpha) * state_cn`), both iterated until `sum |state - prev|^2 / state.size < maxerror^2` or `maxiter`
 * iterations have passed (then the reference raises ConvergenceError).  One call advances `nsteps` steps of size dt.
 *
 * An iteration is ONE sweep where the stage kernels carry it (diffusion: lap_march_kernel with the fixed-point epilogue - right-hand
 * side, update and the sweep's share of the norm, fp64 partial sums, one per wave in a fixed slot, no atomics), else the slope
 * sweep and one pointwise kernel for update and norm (Cahn-Hilliard, 1-D, systems).  A one-workgroup kernel sums the partials in a
 * fixed order and does the stop test on the device; the host enqueues batches of iterations, whose launches return at entry once
 * the step is over, and reads the 64-byte control block through pinned memory once per batch (`batch` = 0: the iterations of the
 * step before plus one, 2 at the start).  Results do not depend on the batch size.
 *
 * work4 = two arrays of the state's size (iterates; the state array itself is the third buffer of the rotation), the array of
 * rate_t (Crank-Nicolson, else NULL), a scratch array for the slope (may be NULL: status 2 and nothing advanced when the right-hand
 * side needs it).  ctl_dev: device memory of pdehip_fixedpoint_ctl_bytes bytes.  *result names the array that holds the state
 * afterwards (the state array or one of the two iterates).  Time-dependent faces (bc_program): the first estimate of implicit Euler
 * and rate_t see them at t, everything else at t + dt; rhs->t is the time of the first step. */
typedef struct pdehip_fixedpoint {
    int32_t scheme;              /* 0: implicit Euler, 1: Crank-Nicolson */
    int32_t maxiter;             /* >= 1 */
    double explicit_fraction;    /* Crank-Nicolson: alpha */
    double maxerror2;            /* maxerror ** 2 */
    int32_t batch;               /* iterations enqueued between two reads of the control block; 0: adaptive */
    int32_t last_iterations;     /* in / out: iterations of the step before (0: none yet) */
    int64_t steps_done;          /* out (+=): completed steps */
    int64_t evaluations;         /* out (+=): right-hand-side evaluations, n + 2 (implicit) / n + 3 (Crank-Nicolson) per step of n iterations */
    int32_t status;              /* out: 0 done, 1 a step did not converge within maxiter (later steps not started; state unspecified), 2 scratch needed */
    int32_t fused;               /* out: 1 = the iterations ran as one sweep each */
    double err;                  /* out: the norm of the last iteration */
    int32_t *iterations;         /* NULL or host array of nsteps entries: iterations of every step */
} pdehip_fixedpoint_t;
int pdehip_fixedpoint_ctl_bytes(const pdehip_grid_t *g, int ncomp, size_t *bytes);
int pdehip_fixedpoint_run(const pdehip_grid_t *g, const pdehip_rhs_t *rhs, pdehip_fixedpoint_t *fp, double dt, int64_t nsteps, void *state_full,
                          void *const *work4_host, void *ctl_dev, size_t ctl_bytes, void **result, void *stream);
/* The same loops around the passes of an expression PDE (passes as in pdehip_jit_rk_run: -1 - k as `src` / `extras` is component k of the
 * iterate, as `out` component k of the rate; the passes that write a rate compute `p[0] * F` and get p[0] = 1, p[1] = the time).  A
 * single-component expression whose last pass runs on the vectorised kernel takes the fixed-point epilogue in that pass (stage_fuse bit 0);
 * systems and complex states (planar (re, im) pairs; stage_fuse bit 1: `state.size` counts a pair once) use the pointwise kernel on all
 * components at once.  Arrays of work4 hold ncomp components each. */
int pdehip_jit_fixedpoint_run(const pdehip_grid_t *g, const pdehip_jit_pass_t *passes, int npasses, void *const *fixed, int nfixed, int ncomp,
                              pdehip_fixedpoint_t *fp, double dt, double t0, int64_t nsteps, void *state_full, void *const *work4_host,
                              void *ctl_dev, size_t ctl_bytes, int stage_fuse, void *bc_program, void **result, void *stream);

/* ---- Poisson's and Laplace's equation (optional entry points: the ABI version stays 8, a library without them still loads) ----
 * The reference's one stationary solve: the operator `poisson_solver` (pde/backends/scipy/operators/cartesian.py:472-489, which builds
 * the Laplacian with its conditions as a sparse matrix plus a constant vector, `_get_laplace_matrix`, and hands both to
 * make_general_poisson_solver, pde/backends/scipy/operators/common.py:71-146: spsolve, else lsmr), used by solve_poisson_equation /
 * solve_laplace_equation (pde/pdes/laplace.py:28-125).  Here: `L u = f` with L = the 3/5/7-point Laplacian of the grid and the given
 * faces, split like the reference into L u = A u + v (A: every face with its constant dropped; v = L(0)) and solved as
 * (-A) u = v - f by conjugate gradients ON THE DEVICE, single-reduction form (Chronopoulos-Gear): per iteration one stencil sweep
 * w = -A r that also leaves every wave's share of r.r and r.w (poisson_apply_kernel behind the ghost kernel; fp64 partial sums in fixed
 * slots, no atomics), a one-workgroup kernel (sums in a fixed order, alpha, beta, stop test `||r|| <= max(rtol * ||f - v||, atol)`, control
 * block) and one pointwise sweep (p, q, x, r).  The host enqueues `batch` iterations, whose launches return at entry once the solve
 * is over, and reads the control block through pinned memory once per batch; results do not depend on the batch size and
 * two runs give equal bits.  Fields fp64 or fp32; work vectors and scalars are fp64 either way.
 *
 * Faces: first-order conditions whose virtual point comes from the adjacent cell (Dirichlet, Neumann, mixed / Robin; scalar or
 * PDEHIP_BCF_ARRAYS coefficients) or periodic axes - they keep A symmetric.  Second-order faces (`index2`), PDEHIP_BC_SKIP and
 * PDEHIP_BCF_NORMAL are refused (PDEHIP_E_NOTIMPL, the message names the face).  Coefficient arrays are read at every solve, so a
 * bc program may rewrite them between solves; whether the system is singular is decided in pdehip_poisson_create.
 *
 * Singular systems (every face periodic or Neumann, i.e. factor1 == 1 everywhere): the reference falls through spsolve's
 * MatrixRankWarning to lsmr - the minimum-norm least-squares solution - and raises unless `A x` is allclose to the right-hand side
 * (common.py:112-141).  Here the mean of the right-hand side is projected out, the iterates start from 0, the mean of x is removed
 * at the end, and one more sweep counts the cells with |A x - (f - v)| > 1e-5 + 1e-5 |f - v|: status 4 if there are any.
 *
 * The handle owns the five work vectors (x, r, p, q, w), the control block with its slots (three partial sums for each of the 32768
 * waves a launch of the solver has at most: 786 KB whatever the grid) and its pinned mirror; it serves any number of
 * right-hand sides.  `rhs_full` and `out_full` are full arrays of the grid (only interior cells are read / written; they may be the
 * same array). */
typedef struct pdehip_poisson {
    double rtol, atol;           /* in: stop at ||r||_2 <= max(rtol * ||f - v||_2, atol) */
    int32_t maxiter;             /* in: >= 1, updates of x at most */
    int32_t batch;               /* in: iterations enqueued between two reads of the control block; 0: 32 */
    int32_t iterations;          /* out: updates of x done */
    int32_t status;              /* out: 0 converged, 1 maxiter updates without convergence, 2 a non-finite scalar, 3 breakdown (r.Ar or p.Ap
                                    not positive: the system is not definite), 4 singular system whose solution fails the reference's test */
    double residual;             /* out: ||r||_2 of the last iterate (the recurrence's residual) */
    double rhs_norm;             /* out: ||f - v||_2 (singular systems: after the projection) */
    double check_residual;       /* out: singular systems: ||A x - (f - v)||_2 of the final test (common.py:135) */
    int32_t singular;            /* out: 1 = the system was treated as singular */
    int32_t reserved;
} pdehip_poisson_t;
int pdehip_poisson_create(const pdehip_grid_t *g, const pdehip_bc_face_t *faces, void **handle);
int pdehip_poisson_solve(void *handle, const void *rhs_full, void *out_full, pdehip_poisson_t *io, void *stream);
int pdehip_poisson_destroy(void *handle);

/* The multigrid preconditioner of the same solve (optional entry points as well; the ABI version stays 8).  Plain conjugate gradients need
 * a number of iterations proportional to the extent of the grid; with one geometric V-cycle `z = M r` per iteration the count no
 * longer depends on it.  pdehip_poisson_set_multigrid builds the hierarchy on a handle (`opts` = NULL drops it); pdehip_poisson_solve
 * on a handle with a hierarchy runs the PRECONDITIONED single-reduction loop: z = M r, w = -A z with the shares of r.z, z.w and r.r
 * in the sweep, beta = r.z / (r.z)_prev, alpha = r.z / (z.w - beta r.z / alpha_prev), p = z + beta p, q = w + beta q, x += alpha p,
 * r -= alpha q.  The one-workgroup kernel and the pointwise sweep are those of the plain loop (which is the case z = r); the stop rule
 * is the same, on the true residual norm sqrt(r.r): `rtol` means the same thing for both.  Status, singular systems, batches and bit-reproducibility as above.
 *
 * The cycle: level l+1 halves every axis of level l whose extent is even and >= 4 (the other axes keep extent and spacing) until no
 * axis qualifies, a level has <= 512 cells, or `max_levels` levels exist.  Every level carries the rediscretised Laplacian with the
 * same homogeneous faces (coefficient arrays averaged over the children of each coarse face cell, once, in this call: rebuild the
 * hierarchy when a bc program has rewritten them).  Smoother: damped Jacobi with the exact diagonal, `smooth` sweeps before and after
 * the coarse-grid correction, `coarse_sweeps` sweeps from zero on the last level (in LDS, one workgroup, when it has <= 1024 cells).
 * Restriction = mean of the children, prolongation = copy to the children.  M is symmetric and positive definite.
 * LIMIT: an odd extent stops the coarsening of its axis (513^3 has one level, 500 x 500 x 300 ends at 125 x 125 x 75); the cycle is
 * then a weaker preconditioner and the sweeps of a large last level run one launch each - correct, but slower.
 * MEMORY: level 0 adds one work vector to the five of the handle, every further level three vectors of its size - in 3-D about
 * 3/7 of a work vector in all (`bytes`; the partial sums of the loop are in the slots of the handle and not counted). */
#define PDEHIP_MG_MAX_LEVELS 32
typedef struct pdehip_poisson_mg {
    int32_t smooth;              /* in: Jacobi sweeps before and after the coarse-grid correction; 0: 2.  out: the value used */
    int32_t coarse_sweeps;       /* in: sweeps from zero on the last level; 0: 32.  out: the value used */
    int32_t max_levels;          /* in: levels at most; 0: as many as the rule above gives */
    int32_t levels;              /* out: levels built (1: the grid does not coarsen - the cycle is `coarse_sweeps` Jacobi sweeps) */
    double omega;                /* in: damping of the smoother; 0: 2/3, 4/5, 6/7 in 1, 2, 3 dimensions.  out: the value used */
    int64_t shapes[PDEHIP_MG_MAX_LEVELS][PDEHIP_MAX_DIM];   /* out: extents of every level along the grid's axes */
    uint64_t bytes;              /* out: device memory the hierarchy allocated */
} pdehip_poisson_mg_t;
int pdehip_poisson_set_multigrid(void *handle, pdehip_poisson_mg_t *opts);
/* One application z = M r of the cycle on two full fp64 arrays of the grid (interior cells of r_full are read, all of z_full is
 * written; they may be the same array).  Uses the work vectors of the handle: not while a solve on it is in flight. */
int pdehip_poisson_precondition(void *handle, const void *r_full, void *z_full, void *stream);

/* ---- linear interpolation on the device (optional entry points; the ABI version stays 8) -----------------------------------------
 * Replaces `make_interpolation_axis_data` and `make_single_interpolator` (pde/backends/numba/grids.py:102-190, :193-347) behind
 * `BackendBase.make_interpolator` (pde/backends/base.py:606-632, numba twin pde/backends/numba/backend.py:895-988), operation by
 * operation: per axis `c_l, d_l = divmod((coord - lo) / dx - 0.5, 1.0)` by the rule of CPython's float divmod, the reference's
 * branches with its inequalities (periodic: wrap; valid data only: bulk / one-sided upper / one-sided lower; with_ghost_cells:
 * the bulk rule on [-0.5, size - 0.5]), weights below 1e-15 set to 0, the 2 / 4 / 8 term sum left to right.  Weights and sums are
 * fp64 for fp32 fields too, rounded once at the store.  `data_full` is a full array in the device layout (pdehip_layout) in BOTH
 * modes: "valid data only" reads its interior with the one-sided branches (an index of -1, which the divmod rule yields for a tiny
 * negative quotient, reads the last cell like `data[..., -1]`, with weight 0).  `ncomp` components are done in one launch (complex
 * data: planar pairs, each part with the same real weights).  `periodic` and `lo` are HOST arrays of `ndim` entries
 * (grid.periodic, grid.axes_bounds[a][0]).
 *
 * Points out of bounds (grids.py:156, :170, :251-256; a coordinate that is not finite counts as out of bounds): with `fill`
 * (DEVICE array of `ncomp` doubles) that value is stored; without (NULL) nothing is stored for the point and it is counted into
 * `oob_count` (DEVICE uint64, added to - zero it before).  No assert, no trap: the host raises `DomainError`.
 *
 * pdehip_interpolate_points: `points` = (npoints, ndim) fp64 on the device, `out` = (ncomp, npoints) in the grid's dtype.  One thread
 * per point, grid-stride, 64-bit offsets. */
int pdehip_interpolate_points(const pdehip_grid_t *g, int ncomp, const int *periodic_host, const double *lo_host, int with_ghost_cells,
                              const void *data_full, const double *points, int64_t npoints, const double *fill, void *out,
                              void *oob_count, void *stream);
/* pdehip_interpolate_to_grid: the points are the cell centres of another Cartesian grid (`ScalarField.interpolate_to_grid`,
 * pde/fields/scalar.py:468; DataFieldBase.interpolate_to_grid pde/fields/datafield_base.py:703-733), so support cells and weights are
 * separable: a small kernel fills per-axis tables (c_li, c_hi, w_l, w_h, in-bounds flag for every target index of every axis) from
 * `dst_coords` (DEVICE, the target's grid.axes_coords one axis after the other), the main kernel walks the target's rows along
 * the fastest axis and writes the interior of the full array `dst_full` (its ghost cells are left alone).  `tables`: DEVICE
 * workspace of 40 bytes per entry of `dst_coords`.  Same arithmetic and term order as pdehip_interpolate_points: equal bits. */
int pdehip_interpolate_to_grid(const pdehip_grid_t *src, int ncomp, const int *periodic_host, const double *src_lo_host, int with_ghost_cells,
                               const void *src_full, const pdehip_grid_t *dst, const double *dst_coords, const double *fill,
                               void *dst_full, void *tables, void *oob_count, void *stream);
/* Edge and corner ghost cells the way `BoundariesList.set_ghost_cells(..., set_corners=True)` fills them
 * (pde/grids/boundaries/axes.py:458-501; used by `field.interpolate(point, bc=...)`, pde/fields/datafield_base.py:690-693): call
 * AFTER pdehip_set_ghost_cells on the same stream.  2-D: corner = (d[nxt(i), j] + d[i, nxt(j)]) / 2; 3-D: the interior cells of the
 * twelve edges the same way from the two adjacent face ghost cells, then corner = (sum of the three adjacent edge cells) / 3; in the
 * field's own type, like numpy.  1-D grids: nothing to do.  pdehip_set_ghost_cells itself is unchanged. */
int pdehip_set_ghost_corners(const pdehip_grid_t *g, int ncomp, void *data_full, void *stream);

/* ---- the PURE-fp32 arithmetic mode of fp32 fields (optional entry points; the ABI version stays 8) --------------------------------
 * Write (-), (+), (x) for fp32 operations, each rounded to fp32, never contracted (-ffp-contract=off), and s_a = fp32(dx_a ** -2) (the
 * power in double, rounded once).  The contract:
 *     per-axis term    t_a = ((l_a (-) 2c) (+) r_a) (x) s_a            (2c is exact)
 *     Laplacian        t_0,  t_0 (+) t_1,  (t_0 (+) t_1) (+) t_2        in grid-axis order
 *     Euler step       u' = u (+) (fp32(dt) (x) (fp32(D) (x) lap(u)))
 *     a zero-derivative face: the neighbour beyond the wall IS the adjacent cell (a copy, no arithmetic); a periodic face: the cell at
 *     the other end of the axis
 *     k steps in one sweep equal k single steps bit for bit (the intermediate level is an fp32 value either way).
 * This is the arithmetic of the reference's torch backend on fp32 fields: the Laplacian of pde/backends/torch/operators/cartesian.py:55-83
 * and the Euler update of pde/backends/torch/_solvers.py:149 (`state + dt * rhs`, DiffusionPDE's `D * laplace(state)`,
 * pde/pdes/diffusion.py:119-121).  A numpy fp32 restatement of the lines above equals that backend bit for bit for the Laplacian with
 * value / derivative / mixed faces (ghost cells from `set_ghost_cells` on the fp32 field) and for Euler runs with periodic and
 * zero-derivative faces (tests/golden/make_golden_f32p.py asserts it).  It does NOT hold for inhomogeneous faces inside the Euler loop:
 * the reference's torch stepper rounds their ghost cells differently from its own `set_ghost_cells` - the loop refuses them.
 *
 * The mode travels per call, by the choice of entry point; there is no process-wide switch.  fp32 grids only (PDEHIP_E_NOTIMPL else).
 *
 * pdehip_laplace_f32p: pdehip_laplace in this arithmetic (same arguments; the caller has set the ghost cells of in_full).  Replaces the
 * closure of make_laplace of the torch backend (pde/backends/torch/operators/cartesian.py:55-83).  3-D grids whose fastest axis is a
 * multiple of four cells: lap32_kernel<march> (register march along axis 0, 16-byte row accesses, fastest-axis neighbours by DPP);
 * everything else: lap32_kernel<generic> (one cell per thread). */
int pdehip_laplace_f32p(const pdehip_grid_t *g, const void *in_full, void *out, int out_layout, void *stream);
/* pdehip_euler_run_f32p: pdehip_euler_run for PDEHIP_RHS_DIFFUSION in this arithmetic: `nsteps` explicit Euler steps, ping-ponging
 * between buf_a (initial state) and buf_b; *result receives the buffer holding the final state.  Replaces the fixed-step loop of the
 * torch backend (EulerStepper, pde/backends/torch/_solvers.py:127-149) for DiffusionPDE.  Every axis must be periodic or zero-derivative
 * on both sides (scalar first-order faces with const 0, factor 1 and the periodic / adjacent index; PDEHIP_E_NOTIMPL otherwise, before
 * anything is launched); ghost cells of the buffers are neither read nor written.  3-D grids whose fastest axis is a multiple of four
 * cells and at most 1024 (two cells at least on the other axes): euler32_kernel<two-step> advances two steps per sweep, an odd last step and every other grid take
 * euler32_kernel<generic> (one step per launch, any number of axes, any extent; rhs->reserved & PDEHIP_RHS_F32P_ONE_STEP forces it for that call:
 * the yardstick the two-step instance is tested against). */
int pdehip_euler_run_f32p(const pdehip_grid_t *g, const pdehip_rhs_t *rhs, void *buf_a, void *buf_b, double dt, int64_t nsteps,
                          void **result, void *stream);
/* Dry run: *answer = 0 when pdehip_laplace_f32p (rhs == NULL) / pdehip_euler_run_f32p (rhs given) would refuse the grid or the faces,
 * 1 = accepted by the one-cell-per-thread instance, 2 = accepted by the march / two-step instance.  The answer is about grid and faces
 * only: the march / two-step instances also need every array on a 16-byte boundary (what pdehip_malloc and the component pitches of
 * pdehip_layout give) and a call without PDEHIP_RHS_F32P_ONE_STEP - a call that fails either takes the one-cell-per-thread instance,
 * with equal bits (pdehip_last_kernel_name tells).  Launches nothing; always returns 0 (pdehip_last_error holds the reason of a refusal). */
int pdehip_f32p_supported(const pdehip_grid_t *g, const pdehip_rhs_t *rhs, int *answer);

/* ---- statistics of a field where it lives (optional entry points; the ABI version stays 8) ----------------------------------------
 * What a tracker asks of a running simulation without moving the state to the host.  Both entries read the INTERIOR cells of full
 * arrays in the device layout (ghost cells and row padding never enter a result), sweep with 16-byte loads where the row length allows,
 * leave one partial result per wave in a fixed slot and fold the slots with one workgroup in a fixed order: no atomics, two runs give
 * equal bits.  The slots (1.3 MB) are kept per stream and freed by pdehip_release_scratch.
 *
 * pdehip_field_stats: replaces the host reductions behind `DataFieldBase.integral`, `.average`, `.fluctuations` and `.magnitude`
 * (pde/fields/datafield_base.py:846-897; `grid.integrate` = sum x cell volume on Cartesian grids, `np.std` = numpy's two-pass variance).
 * For every component c (1 <= ncomp <= 64) eight doubles at out_dev + 8 * c:
 *     {n_finite, n_nonfinite, sum, min, max, mean, m2, 0}
 * sum, min and max over the FINITE cells, in fp64 from values converted exactly; mean = sum / n_finite; m2 = sum of (x - mean)^2 over the
 * finite cells, by a SECOND sweep on the same stream that reads the mean from out_dev (launched only with want_m2 != 0, else m2 = NaN).
 * n_finite == 0: min, max, mean and m2 are NaN.  norm != 0: ONE block of eight for s = sqrt(x_0 * x_0 + x_1 * x_1 + ...) over the
 * components, evaluated in the field's own type in component order, one rounding per operation: the norm behind `to_scalar("auto")` of
 * vector and tensor fields (pde/fields/vectorial.py:420-431, pde/fields/tensorial.py:333-337). */
int pdehip_field_stats(const pdehip_grid_t *g, int ncomp, const void *arr_full, int norm, int want_m2, double *out_dev, void *stream);
/* pdehip_steady_state: the test of `SteadyStateTracker.handle` (pde/trackers/trackers.py:819-844) in ONE sweep over all components: for
 * every interior cell where `cur` is finite r = |(last - cur) / elapsed| - rtol * |cur|, in the field's type and in this order (a
 * division, not a product with a reciprocal; elapsed and rtol rounded to the field's type first, like a Python float next to an fp32
 * array).  out_dev[0] = max r (NaN if any such r is NaN, like np.max; NaN too when no cell took part), out_dev[1] = number of cells
 * that took part.  The same sweep copies cur to last in EVERY interior cell, the others included (`self._last_data[:] = field.data`);
 * ghost cells of `last` are left alone.  `last_full` must not be `cur_full`. */
int pdehip_steady_state(const pdehip_grid_t *g, int ncomp, const void *cur_full, void *last_full, double elapsed, double rtol,
                        double *out_dev, void *stream);

/* ---- projections and boxes of a field where it lives (optional entry points; the ABI version stays 8) ------------------------------
 * The reduced-dimensional pictures a tracker writes out of a 3-D run, without moving the state to the host.  Both entries read the
 * INTERIOR cells of a full array in the device layout (ghost cells and row padding never enter a result); arr_full is on a 16-byte
 * boundary (what pdehip_malloc and the component pitch of pdehip_layout give).  No atomics: two calls give equal bits.
 *
 * pdehip_project: replaces `ScalarField.project` (pde/fields/scalar.py:269-339) on the arrays behind it: `grid.integrate(data, axes)`
 * (pde/grids/base.py:1286-1341; a sum over the removed axes of data x cell volume) and `np.max` / `np.min` over the removed axes
 * (pde/fields/scalar.py:325-329); `project_#` of `CartesianGrid.get_line_data` (pde/grids/cartesian.py:296-372) is the sum with weight 1,
 * divided by the number of removed cells on the host.  Bit a of axes_mask removes axis a of the grid (the grid's own order); the mask
 * is not empty and names no other axis; removing every axis leaves one value per component.  out_dev: a dense C-ordered array
 * (ncomp, retained extents...).
 *   PDEHIP_PROJECT_SUM   per output cell the sum of (double)x * weight over the removed cells; every term and every addition is one
 *                        fp64 rounding (never FMA-contracted), the order is fixed by the shape.  Output: double for both field types
 *                        (an fp32 array times the fp64 cell volumes is fp64 in numpy).  NaN and +-inf propagate by the arithmetic.
 *   PDEHIP_PROJECT_MAX / _MIN   output in the field's own type, the bits of np.max / np.min: NaN if any removed cell of the output cell
 *                        is NaN, +-inf are ordinary values; the sign of a zero result is unspecified when both zeros occur.  weight is
 *                        ignored.
 * Removing the fastest axis is a reduction of each row by a group of 1 ... 64 lanes; removing slower axes is a march of each thread
 * over the removed cells in segments of 128, with whole pieces of rows read by the lanes of a wave at every step; the partial results
 * (one per row, or one per segment and output cell) go through dense fp64 arrays that the same two kernels reduce further, in a fixed
 * order.  These arrays are kept per stream, grown on demand and freed by pdehip_release_scratch. pdehip_last_kernel_name gives the
 * chain of instances, joined by `+`.
 *
 * pdehip_extract_box: replaces the index expressions of `ScalarField.slice` (pde/fields/scalar.py:341-427), of `cut_#` in
 * `CartesianGrid.get_line_data` and of `CartesianGrid.get_image_data` (pde/grids/cartesian.py:374-402): the interior box
 * [lo, lo + extent) of every component as a dense C-ordered array (ncomp, extent...) of the field's type.  lo and extent have one
 * entry per axis of the grid, in the grid's own order; the box lies inside the grid and no extent is 0.  A slice is a box of extent 1 on
 * the removed axes.
 *
 * Both refuse (status PDEHIP_E_VALUE, message in pdehip_last_error) NULL pointers, ncomp outside 1 ... 64, an empty or foreign
 * mask, an unknown method, a box that is not inside the grid and a misaligned array. */
#define PDEHIP_PROJECT_SUM 0
#define PDEHIP_PROJECT_MAX 1
#define PDEHIP_PROJECT_MIN 2
int pdehip_project(const pdehip_grid_t *g, int ncomp, const void *arr_full, int axes_mask, int method, double weight,
                   void *out_dev, void *stream);
int pdehip_extract_box(const pdehip_grid_t *g, int ncomp, const void *arr_full, const long *lo, const long *extent,
                       void *out_dev, void *stream);

/* ---- Gaussian smoothing of a field where it lives: one pass along one axis (optional entry point; the ABI version stays 8) -----------
 * Replaces one call of `scipy.ndimage.gaussian_filter1d` in `DataFieldBase.smooth` (pde/fields/datafield_base.py:988-1035) on the
 * arrays behind it; the caller chains one pass per axis (pde_hip/smoothing.py).  Bit for bit scipy's result, given scipy's weights.
 *
 * One pass filters axis `axis` (the grid's own order) of extent n with radius r >= 0 and the weights w[0..r], w[0] the centre weight
 * (the upper half of the symmetric kernel).  For every interior cell i along that axis, in fp64:
 *
 *     t = x[i] * w[0]
 *     for j = r, r-1, ..., 1:   t = t + (x[idx(i-j)] + x[idx(i+j)]) * w[j]
 *     out[i] = t
 *
 * Every product and every addition is one fp64 rounding, never contracted into an FMA (scipy's symmetric branch, its line buffers are
 * double).  An fp32 field is converted exactly to fp64 on load and rounded once to fp32 on store - in both settings of the fp32
 * arithmetic mode.  idx(p) holds for ANY r, including r >= n, r >= 2n and n == 1:
 *     PDEHIP_SMOOTH_WRAP      p mod n                                       (mode "wrap": periodic axes)
 *     PDEHIP_SMOOTH_REFLECT   q = p mod 2n, then q < n ? q : 2n - 1 - q     (mode "reflect": scipy's half-sample symmetric extension)
 * with the mathematical (non-negative) modulus.  r == 0 is the copy x * w[0].  NaN and +-inf propagate by the arithmetic.  Only
 * INTERIOR cells of the full device layout are read and written: ghost cells and row padding of out_full are left as they were, and
 * in_full is not modified.  No atomics: two calls give equal bits.
 *
 * weights: HOST memory, radius + 1 values, consumed before the call returns (they are staged in per-stream scratch that
 * pdehip_release_scratch frees).  They come from the host because numpy's exp is the one scipy uses and libm's may differ in the last
 * bit: pde_hip/smoothing.py::gaussian_weights.
 *
 * Instances (pdehip_last_kernel_name names the one that ran): `gauss_row_kernel<T>` filters the fastest axis through LDS, radius up to
 * 608; `gauss_march_kernel<T,VEC>` any slower axis through LDS, radius up to 48 (VEC = 2 doubles / 4 floats per lane where the row
 * length is a multiple of that, else 1); `gauss_cell_kernel<T>` takes everything else: any radius, axis and extent, one output cell per
 * thread.  PDEHIP_SMOOTH_CELL or'ed into the mode forces the last one (the yardstick of the tests).
 *
 * Refused (status PDEHIP_E_VALUE, message in pdehip_last_error): NULL pointers, ncomp outside 1 ... 64, an axis the grid does not have,
 * an unknown mode, radius < 0, in_full == out_full or overlapping arrays, an array that is not on a 16-byte boundary. */
#define PDEHIP_SMOOTH_WRAP    0
#define PDEHIP_SMOOTH_REFLECT 1
#define PDEHIP_SMOOTH_CELL    16   /* or'ed into mode: force the one-cell-per-thread instance (the yardstick of the tests) */
int pdehip_smooth_axis(const pdehip_grid_t *g, int ncomp, const void *in_full, void *out_full, int axis, int mode,
                       int radius, const double *weights /* host, radius + 1 values, consumed before return */, void *stream);

/* ---- the distribution of a field where it lives: histogram and exact order statistics (optional entry points; the ABI version stays 8) --
 * What `np.histogram(state.data)` and `np.quantile(state.data, q)` in a tracker callback answer, without moving the state to the host.
 * Both entries read the INTERIOR cells of full arrays in the device layout (ghost cells and row padding never enter a result), sweep
 * with 16-byte loads where the row length allows, and take 1 <= ncomp <= 64.  Without norm there is one block of results per component;
 * norm != 0: ONE block for s = sqrt(x_0 * x_0 + x_1 * x_1 + ...) over the components, evaluated as pdehip_field_stats evaluates it.
 * The results are integers and elements of the field: they do not depend on the order of evaluation, two calls give equal bits.  The
 * workgroups count in 32-bit LDS counters (lanes of a wave that hit the same counter are combined first) and fold them with 64-bit
 * integer adds in global memory.  Pinned host memory for the edges and the control blocks of the selection are kept per stream and
 * freed by pdehip_release_scratch.  pdehip_last_kernel_name names the instance of the sweep.
 *
 * pdehip_histogram: edges_dev holds nbins + 1 fp64 edges e[0] < e[1] < ... < e[nbins], all finite, 1 <= nbins <= 4096.  Every block
 * receives nbins + 3 unsigned 64-bit counts at counts_dev + block * (nbins + 3):
 *     count[i], i < nbins   the cells with e[i] <= x < e[i + 1]; the last bin also takes x == e[nbins]
 *     count[nbins]          the cells below e[0] (-inf included)
 *     count[nbins + 1]      the cells above e[nbins] (+inf included)
 *     count[nbins + 2]      the cells that are NaN
 * Comparisons are in fp64 on the exactly converted value; the sum of a block is the number of interior cells.  The definition is by
 * the edges alone: the kernel guesses a bin (a scaled subtraction where the bins are equal, a binary search else) and settles the guess
 * by comparing with the edges, which gives the counts of `np.histogram` for `bins=int, range=...` with the edges numpy returns and for
 * explicit edge arrays.  The edges are read back and checked on the host before the sweep is launched (the call waits for the stream).
 *
 * pdehip_quantile_select: q_host holds 1 <= nq <= 8 values in [0, 1] (HOST memory, consumed before the call returns).  For every block
 * and every q[j], with n the number of cells that are not NaN, v = (n - 1) * q[j] in fp64 and k = floor(v):
 *     lower_dev[block * nq + j]   the k-th smallest such cell (k = 0: the minimum)
 *     upper_dev[block * nq + j]   the min(k + 1, n - 1)-th
 * both in the field's own type and with the bits of an element of the field; +-inf are ordinary values; when +0 and -0 both occur the
 * sign of a zero result is unspecified.  info_dev + 2 * block receives {n, number of NaN cells} as unsigned 64-bit integers.  n == 0:
 * lower and upper are NaN.  Method: radix selection on the order-preserving integer image of the value bits, 8-bit digits from the top -
 * 8 sweeps for fp64, 4 for fp32, all q in the same sweeps.  Each sweep counts, per digit value, the cells whose leading digits match a
 * target's; a one-workgroup kernel behind it picks the next digit and the remaining rank of every target in a control block on the
 * device.  The host does not synchronise between the passes (or at all).
 *
 * Both refuse (status PDEHIP_E_VALUE, message in pdehip_last_error) NULL pointers, ncomp outside 1 ... 64, nbins outside 1 ... 4096,
 * nq outside 1 ... 8, a q outside [0, 1], edges that are not finite or not strictly increasing, and a misaligned array (16 bytes for
 * the field, 8 for edges, counts and info, the element size for lower and upper). */
int pdehip_histogram(const pdehip_grid_t *g, int ncomp, const void *arr_full, int norm, int nbins, const double *edges_dev,
                     uint64_t *counts_dev, void *stream);
int pdehip_quantile_select(const pdehip_grid_t *g, int ncomp, const void *arr_full, int norm, int nq, const double *q_host,
                           void *lower_dev, void *upper_dev, uint64_t *info_dev, void *stream);

/* ---- the domains of a field where it lives: connected components and their sizes (optional entry points; the ABI version stays 8) -------
 * What `scipy.ndimage.label(state.data > c0)` followed by `np.bincount` in a tracker callback answers (how many droplets, how large is
 * each), without moving the state to the host.  All results are integers: they equal scipy's, two calls give equal bits.
 *
 * pdehip_label_domains reads the INTERIOR cells of ONE real component in the device layout (fp64 or fp32, 1-D to 3-D; ghost cells and
 * row padding never enter).  A cell is FOREGROUND iff lo <= x <= hi, compared in fp64 on the exactly converted value; infinite bounds
 * are allowed, a NaN cell is background.  Two foreground cells are neighbours if they differ by one step along one axis (connectivity
 * 1: the 2 ndim face neighbours) or by at most one step along every axis (connectivity ndim: all 3^ndim - 1 neighbours,
 * `generate_binary_structure(ndim, ndim)`); an axis a with periodic_host[a] != 0 (ndim ints in HOST memory, consumed before the call
 * returns) wraps, corners included under full connectivity.  A domain is a class of the transitive closure.
 *     labels_dev   dense C-ordered int32 array of the interior shape (no ghost cells, no pitch): 0 for background, 1 ... K for the
 *                  cells of a domain; domains are numbered in the C order of their FIRST cell (scipy's numbering)
 *     info_dev     {K, number of foreground cells} as unsigned 64-bit integers
 * Method: union-find in which the root of a domain is its smallest linear cell index (parent[i] <= i always, so every walk to a root
 * goes down and ends).  `label_tile_kernel<T,FULL>` labels tiles of 4 x 8 x 32 cells in LDS, `label_seam_kernel<FULL>` unites across
 * tile faces, edges, corners and the periodic wrap with relaxed agent-scope atomics only (atomicMin on the larger root), a flatten
 * kernel writes every cell's root to labels_dev, roots are counted per chunk of 4096 cells, one workgroup scans the counts, and the
 * labels are written: no ticket counter, the order in which workgroups run does not enter.  Scratch memory - the parent array, 4 bytes
 * per cell, and the chunk counts - is kept per stream and freed by pdehip_release_scratch.  A stream's first call, and a call on a grid with more cells than any
 * before on that stream, allocates (and frees the smaller arrays), which waits for the device; every other call synchronises nothing.
 * pdehip_last_kernel_name names the instance of the tile kernel.
 * Refused (status PDEHIP_E_VALUE, message in pdehip_last_error): NULL pointers, lo > hi or a NaN bound, a connectivity other than 1 or
 * ndim, more than 2^31 - 1 interior cells, a misaligned array (16 bytes for the field, 4 for the labels, 8 for info).
 *
 * pdehip_domain_sizes: sizes_dev[k], k < ndomains, receives the number of the ncells cells of labels_dev with label k + 1 (unsigned
 * 64-bit; integer adds, the lanes of a wave that hit the same label combined first).  ndomains == 0 writes nothing (sizes_dev may be
 * NULL).  Labels outside 0 ... ndomains are counted, never used as an index: if there is one the call is refused with their number
 * (PDEHIP_E_VALUE) and sizes_dev holds the counts of the labels in range.  The call waits for the stream (the caller reads the sizes
 * next).  Also refused: NULL pointers, ncells < 1, ndomains outside 0 ... 2^31 - 1, a misaligned array (4 bytes / 8 bytes). */
int pdehip_label_domains(const pdehip_grid_t *g, const void *arr_full, double lo, double hi, int connectivity,
                         const int *periodic_host, int32_t *labels_dev, uint64_t *info_dev, void *stream);
int pdehip_domain_sizes(const int32_t *labels_dev, int64_t ncells, int64_t ndomains, uint64_t *sizes_dev, void *stream);

/* pdehip_domain_properties (optional entry point; the ABI version stays 8): where every domain of a labelling is, what box it fills and
 * how much of the field it holds - what `scipy.ndimage.center_of_mass`, `find_objects` and `sum_labels` answer on the host.  All outputs
 * are integers: they do not depend on the order in which workgroups run and two calls give equal bits; centroids, boxes and sums are
 * derived from them on the host (pde_hip/domains.py).  labels_dev: dense C-ordered int32 labels of the interior shape of g (0:
 * background, 1 ... ndomains), those of pdehip_label_domains or any other.  Axes are normalised to three (an n-D grid has the trailing n;
 * a missing axis has one cell, is open, and its columns are 0); n_a is the interior extent of axis a, periodic_host as above.  Domain k
 * (label k + 1) receives
 *     anchor_dev[k]                int32: the smallest C-order linear interior index among its cells
 *     moment_dev[3 k + a]          int64: the sum over its cells of the frame offset d_a = i_a - i_a(anchor) on an open axis,
 *                                  ((i_a - i_a(anchor) + h) mod n_a) - h with h = n_a / 2 (integer division, mathematical mod) on a
 *                                  periodic one - the minimal image relative to the anchor
 *     box_dev[6 k + 2 a], [+ 1]    int32: the smallest and the largest d_a
 * and, with arr_full != NULL (ONE real component in the device layout, fp64 or fp32 as g says),
 *     excluded_dev[k]              uint32: its cells whose value is not finite or exceeds absmax in magnitude; they add nothing below
 *     limb_dev[2 k], [+ 1]         int64: the sums of hi and lo over its other cells, where with L = ceil(log2(interior cells)), E the
 *                                  exponent frexp(absmax) returns, eh = E - (62 - L), el = eh - 31 and v the value converted exactly
 *                                  to fp64: hi = rint(ldexp(v, -eh)), r = v - ldexp(hi, eh) (exact), lo = rint(ldexp(r, -el)).
 *                                  The sum of the field over the domain is ldexp(limb[0], eh) + ldexp(limb[1], el), within 2^(el - 1) per
 *                                  cell; |hi| <= 2^(62 - L) and |lo| <= 2^30, so neither 64-bit sum overflows.  absmax == 0: zero limbs.
 *                                  absmax is below 2^1023, so that ldexp(hi, eh) <= 2^E is finite.
 * With arr_full == NULL limb_dev and excluded_dev are not touched.  A label without a cell keeps anchor INT32_MAX, box (INT32_MAX,
 * INT32_MIN) and zeros.  ndomains == 0 writes nothing (the outputs may be NULL).  72 bytes per domain in all.
 * Three launches: initialisation; `props_anchor_kernel` (atomicMin per (wave, label)); `props_sum_kernel<T,FIELD>`, in which the lanes of
 * a wave that share a label are combined by a masked wave reduction and a wave keeps the label it met last with its partial results in
 * registers, as in pdehip_domain_sizes: one set of relaxed agent-scope integer atomics (64-bit adds, 32-bit min / max) per (wave, label).
 * No floating-point atomic anywhere.  Labels outside 0 ... ndomains are counted, never used as an index: if there is one the call is
 * refused with their number (PDEHIP_E_VALUE).  The call waits for the stream to read that count (the caller reads the results next);
 * 16 bytes each of device and pinned host memory are kept per stream and freed by pdehip_release_scratch.  pdehip_last_kernel_name
 * names the instance of the last kernel.  Also refused: NULL or misaligned pointers (16 bytes for the field, 8 for moments and limbs, 4
 * for the others), ndomains outside 0 ... 2^31 - 1, more than 2^31 - 1 interior cells, unsupported types, an absmax that is negative, NaN or not below 2^1023. */
int pdehip_domain_properties(const pdehip_grid_t *g, const void *arr_full, const int32_t *labels_dev, int64_t ndomains,
                             const int *periodic_host, double absmax, int32_t *anchor_dev, int64_t *moment_dev, int32_t *box_dev,
                             int64_t *limb_dev, uint32_t *excluded_dev, void *stream);

/* ---- the spectrum of a field where it lives: forward transform and sums of the power over shells of |k| (optional entry points; the
 * ABI version stays 8) -------------------------------------------------------------------------------------------------------------------
 * What `np.fft.fftn(state.data)` followed by a radial average in a tracker callback answers, without moving the state to the host.  All
 * three read the INTERIOR cells of real full arrays in the device layout (fp64 or fp32, 1-D to 3-D; ghost cells and row padding never
 * enter, the input is never written).  Axes are normalised to three (an n-D grid has the trailing n; a missing axis has one cell); n_a is
 * the interior extent of axis a and nh = n_2 / 2 + 1.
 *
 * pdehip_fft_supported: 0 where every axis of g has a power-of-two extent, at most 1024 cells and at most 4096 on the fastest axis (an
 * extent of 1 counts as an absent axis); else PDEHIP_E_NOTIMPL with the axis and its extent named in pdehip_last_error.  Nothing is
 * launched.  The other two entries refuse the same grids the same way.
 *
 * pdehip_fft_forward: spectrum_dev receives the unnormalised forward transform F(m) = sum_x f(x) exp(-2 pi i m.x / n) of every
 * component as complex128 in C order (ncomp, n_0, n_1, nh) - the Hermitian half `np.fft.rfftn` returns.  Both field types are transformed
 * in fp64; an fp32 element is converted exactly at the load.  Every line, whatever its extent N, goes through ONE schedule in LDS: the
 * elements are stored bit-reversed, then stage s = 1 ... log2(N) replaces the pair (u, v) = (x[i], x[i + h]), h = 2^(s - 1),
 * i = (t >> (s - 1) << s) + k, k = t mod h, for t = 0 ... N / 2 - 1 by (u + p, u - p), where p = w v = (ac - bd) + i (ad + bc) for
 * w = a + i b = W[k N / 2^s] and v = c + i d, every operation rounded once (no FMA contraction in any build).  W[m] = exp(-2 pi i m / N),
 * 0 <= m < N / 2, is a table made on the host from cos and sin of an angle in the first octant; nothing on the device evaluates a
 * trigonometric function.  The fastest axis is transformed first, each row as a complex line with zero imaginary parts of which the
 * first nh outputs are kept, then axis 1 and axis 0 of the half spectrum in place, in tiles of at least 8 neighbouring columns (128
 * contiguous bytes per line index; the tile at the end of the columns is ragged).  An output is a fixed expression of the inputs: it
 * has the same bits however the butterflies are spread over lanes, waves and workgroups, and a serial host version gives equal bits.
 * A line takes 16 N bytes of LDS and its table 8 N: at most 96 KiB for a row of 4096 cells, 136 KiB for a tile of lines of 1024.
 *
 * pdehip_shell_spectrum: kfreq_dev holds the frequencies of the axes of g one after the other (sum of the extents; the caller uploads
 * `np.fft.fftfreq(n_a, dx_a)`), edges_dev nbins + 1 finite fp64 edges e[0] < ... < e[nbins], 1 <= nbins <= 4096.  Mode (i, j, k) of the
 * half spectrum, k < nh, has |k| = sqrt((f_0[i]^2 + f_1[j]^2) + f_2[k]^2) in that order (a missing axis contributes 0), falls into slot
 * b with e[b] <= |k| < e[b + 1] (the last bin closed; slot nbins: below e[0], slot nbins + 1: above e[nbins] - pdehip_histogram's rule),
 * has the weight 2 for 0 < k < n_2 / 2 and 1 otherwise (its mirror image is not stored), and the weighted power
 * v = weight * (re * re + im * im).
 *     counts_dev[b], b < nbins + 2            uint64: the sum of the weights, i.e. the modes of the FULL spectrum in the slot; the same
 *                                             for all components; the sum over the slots is the number of interior cells
 *     sums_dev[c * (nbins + 2) + b]           fp64: the sum of v over the slot for component c
 * A sum does not depend on the order of the modes.  A first sweep takes count and the largest v of every slot (integer maximum of the
 * bit image).  With E the exponent frexp returns for that maximum, L = ceil(log2(count)), D = 63 - L, eh = E - (62 - L), em = eh - D and
 * el = em - D, a second sweep adds for every mode the three integers hi = rint(ldexp(v, -eh)), mid = rint(ldexp(r, -em)) with
 * r = v - ldexp(hi, eh) (exact) and lo = rint(ldexp(r', -el)) with r' = r - ldexp(mid, em) (exact): |hi|, |mid|, |lo| <= 2^(62 - L), so
 * no 64-bit sum of up to 2^L of them overflows, and the three sums hold the sum of v within count * 2^(el - 1), which is below
 * 2^(4 L - 188) of the sum itself.  Lanes of a wave that meet the same slot are combined first, workgroups add in LDS and fold with
 * 64-bit integer atomics: no floating-point atomic anywhere.  The limbs are read back and converted on the host - carried into three
 * non-negative digits, the leading 64 bits and a sticky bit rounded ONCE to nearest - and the sums are written to sums_dev; the call
 * waits for the stream twice (edges, limbs).  A slot whose maximum is zero, infinite or NaN gets that maximum as its sum.
 * With several components the transform of each reuses one spectrum buffer.  Spectrum, tables, maxima and limbs are kept per stream,
 * grown on demand and freed by pdehip_release_scratch.  pdehip_last_kernel_name gives the chain of the instances launched for the last
 * component, joined by '+'.
 *
 * Refused (status PDEHIP_E_VALUE, message in pdehip_last_error): NULL pointers, ncomp outside 1 ... 64, nbins outside 1 ... 4096, edges
 * that are not finite or not strictly increasing, a misaligned array (16 bytes for the field and the spectrum, 8 for the others). */
int pdehip_fft_supported(const pdehip_grid_t *g);
int pdehip_fft_forward(const pdehip_grid_t *g, int ncomp, const void *arr_full, void *spectrum_dev, void *stream);
int pdehip_shell_spectrum(const pdehip_grid_t *g, int ncomp, const void *arr_full, const double *kfreq_dev, int nbins,
                          const double *edges_dev, uint64_t *counts_dev, double *sums_dev, void *stream);

/* ---- the inverse transform, and Poisson's equation on all-periodic grids solved by it (optional entry points; the ABI version stays 8) -------
 * pdehip_fft_inverse: spectrum_dev is the dense half spectrum (ncomp, n_0, n_1, nh) pdehip_fft_forward writes; out_full, a full array of g
 * (fp64 or fp32), receives in its INTERIOR cells f(x) = Re sum_m F(m) exp(+2 pi i m.x / n) / size, size = n_0 n_1 n_2 (a power of two: the
 * scaling is exact).  Ghost cells, row padding and slack are not written.  The spectrum is CONSUMED: the slow-axis passes run in place.
 * Dataflow, fixed like the forward's: axis 0, then axis 1 of the half spectrum (inverse_lines_kernel: tiles, ragged-tile rule and LDS
 * layout of fft_lines_kernel), then the fastest axis (inverse_rows_kernel<T>); absent axes and axes of extent 1 are skipped.  The
 * butterflies and their schedule are those of the forward transform with the twiddles W[m] conjugated at the copy of the table into LDS
 * (a sign flip is exact).  A row becomes a full complex line of N = n_2 elements: element k <= N / 2 is the stored element as it is -
 * including whatever imaginary part sits at k = 0 and k = N / 2 -, element N - k for 0 < k < N / 2 its conjugate; the line is loaded
 * bit-reversed, transformed, and the REAL part times 1 / size is stored, rounded once to the type of g; the imaginary part is dropped
 * (it vanishes for the spectrum of a real field).  max(1, 512 / N) rows per workgroup.  Every output element is a fixed expression of
 * the spectrum, independent of the lane, wave or workgroup that evaluates it; one rounding per operation; a serial host version gives
 * equal bits.  LDS as for the forward transform: at most 96 KiB for rows and 136 KiB for lines.  Grid limits, refusals and alignment
 * checks are those of pdehip_fft_forward.  pdehip_last_kernel_name gives the chain of launches joined by '+'.
 *
 * pdehip_poisson_fft: solves A u = f where A is the 3/5/7-point Laplacian of g with periodic wrap on EVERY axis (the caller vouches for
 * that: the call takes no faces; v = L(0) = 0) and returns the minimum-norm (zero-mean) solution, as the reference's lsmr branch and
 * pdehip_poisson_solve do for singular systems.  No iteration:
 *   1. the forward transform of rhs_full (fp64 arithmetic for both field types; rhs_full is not modified) into a scratch spectrum;
 *   2. fftsolve_divide_kernel over the half spectrum: u^(m) = (f^(m) / mu(m)) * (-1), an IEEE division per part, and u^(0) = 0 exactly
 *      whatever f^(0) is - that is the projection, no mean is computed or subtracted.  mu(m) = (mu_0[i] + mu_1[j]) + mu_2[k] in that order
 *      from per-axis host tables mu_a[m] = (4 (s s)) scale_a, s = sin(pi m' / n_a) with the angle 3.14159265358979323846 * m' / n_a,
 *      m' = min(m, n_a - m), scale_a = 1 / dx_a^2 as the Laplacian kernels use it; an absent axis has the one entry 0.  (The sine form,
 *      because 2 cos - 2 loses the low modes to cancellation.)
 *   3. the passes of pdehip_fft_inverse into an fp64 full-layout scratch array x;
 *   4. the acceptance test pdehip_poisson_solve applies to singular systems: periodic ghost cells of x, w = A x with the stencil
 *      kernels, then one sweep (fftsolve_check_kernel) whose waves leave their shares of four sums in slots of their own - no
 *      floating-point atomic; the host adds them in slot order -: the count of cells with !(|w - f| <= 1e-5 + 1e-5 |f|),
 *      sum (w - f)^2, sum (w - (f - fbar))^2 and sum (f - fbar)^2 with fbar = f^(0) / size read from the spectrum before step 2;
 *   5. x is stored to out_full, rounded once to the field type (in the sweep of step 4; out_full may be rhs_full).
 * io: in rtol, atol (maxiter and batch are ignored).  Out: iterations = 0, singular = 1, rhs_norm = ||f - fbar||_2,
 * residual = ||A x - (f - fbar)||_2 - the TRUE residual, not a recurrence -, check_residual = ||A x - f||_2, and status 2 if a sum is not
 * finite, else 4 if the count is not zero (an inconsistent right-hand side: the reference's RuntimeError), else 1 if
 * residual > max(rtol * rhs_norm, atol), else 0.  The attainable residual of ANY fp64 method is about u ||A|| ||x|| (u = 2^-53): a smooth
 * right-hand side on a 4096-cell 1-D grid can therefore miss an rtol near 1e-10; that is reported (status 1), not hidden.
 * The eigenvalue tables, the spectrum, x, w and the slots (256 KiB) are kept per stream with the scratch of the transforms and freed by
 * pdehip_release_scratch.  The call waits for the stream once.  pdehip_last_kernel_name gives the chain of the transform and solve
 * launches: it ends in "+fftsolve_divide_kernel+<inverse passes>+fftsolve_check_kernel".  Grids are refused as by pdehip_fft_supported;
 * also refused (PDEHIP_E_VALUE): NULL pointers, arrays not on a 16-byte boundary, rtol or atol negative or NaN. */
int pdehip_fft_inverse(const pdehip_grid_t *g, int ncomp, void *spectrum_dev, void *out_full, void *stream);
int pdehip_poisson_fft(const pdehip_grid_t *g, const void *rhs_full, void *out_full, pdehip_poisson_t *io, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PDEHIP_H */
