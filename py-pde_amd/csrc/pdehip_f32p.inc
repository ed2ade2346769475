// pdehip_f32p.inc — device code of the PURE-fp32 arithmetic mode (include/pdehip.h "pure fp32"): the Laplacian and the explicit Euler
// step of the diffusion equation with every operation rounded to fp32, in the reference's torch order
// (pde/backends/torch/operators/cartesian.py:55-83, pde/backends/torch/_solvers.py:149):
//     t_a = ((l_a - 2c) + r_a) * s_a,  s_a = fp32(dx_a ** -2);   lap = t_0 [+ t_1 [+ t_2]] in grid-axis order
//     u'  = u + fp32(dt) * (fp32(D) * lap(u))
// Compiled with -ffp-contract=off: no operation is fused, so packing two cells into v_pk_*_f32 changes no bit.
// Included by pdehip_f32p.hip only; the templates of pdehip_march*.inc are not touched.

typedef float f4 __attribute__((ext_vector_type(4)));

struct F32pArgs {
    long n0, n1, n2;        // valid cells of the normalised axes (unused leading axes: 1)
    long p0, p1;            // pitches of a full array (elements); the fastest axis has pitch 1
    long off;               // offset of interior cell (0,0,0) in a full array
    long o_off, o_s0, o_s1; // the same for the output (valid or full layout)
    float s0, s1, s2;       // fp32(dx ** -2) per normalised axis
    float D, dt;            // Euler: fp32(D), fp32(dt)
    int per0, per1, per2;   // Euler: 1 = periodic axis, 0 = zero-derivative faces ("the neighbour beyond the wall is the cell itself")
    int seg;                // planes of axis 0 one march covers
    int nyt, nseg, nxc;     // tiles along axis 1, segments along axis 0, 256-cell chunks along axis 2
};

constexpr int kF32pRows = 4;    // rows of axis 1 a lane keeps in registers (R); the fast tile is seg planes x R rows x 256 cells per wave

// wavefront shift by one lane (DPP wave_shr:1 / wave_shl:1): lane i receives `src` of lane i - 1 (resp. i + 1); lane 0 (resp. 63),
// which has no source lane, keeps `old` - the value from outside the 256-cell chunk.  One DPP move per value at 4 bytes.
__device__ __forceinline__ float f32p_shr1(float old, float src)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float f32p_shl1(float old, float src)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(src), 0x130, 0xf, 0xf, false));
}

// Laplacian of four cells of a row of a 3-D grid: zm / zp the same cells one plane below / above (axis 0), ym / yp one row below / above
// (axis 1), xl / xr the cells left of c.x and right of c.w (axis 2)
__device__ __forceinline__ f4 f32p_lap_row(f4 c, f4 zm, f4 zp, f4 ym, f4 yp, float xl, float xr, float s0, float s1, float s2)
{
    const f4 two = c + c;                          // 2c is exact
    const f4 t0 = ((zm - two) + zp) * s0;
    const f4 t1 = ((ym - two) + yp) * s1;
    f4 lx, rx;
    lx.x = xl; lx.y = c.x; lx.z = c.y; lx.w = c.z;
    rx.x = c.y; rx.y = c.z; rx.z = c.w; rx.w = xr;
    const f4 t2 = ((lx - two) + rx) * s2;
    return (t0 + t1) + t2;
}
__device__ __forceinline__ f4 f32p_euler_row(f4 c, f4 lap, float D, float dt)
{
    return c + dt * (D * lap);
}

// index of the cell that stands for cell q of an axis of n cells: wrapped (periodic) or clamped (zero-derivative: the ghost cell is a
// copy of the adjacent cell).  Exact for -n <= q < 2n - the callers stay within two cells of the axis and the march instances ask for
// n >= 2; one compare-and-add, never a division, and the result is clamped into the axis whatever q is (rows of a tile beyond the
// grid are loaded from valid addresses and never used).
__device__ __forceinline__ long f32p_map(long q, long n, int per)
{
    if (per) q = q < 0 ? q + n : (q >= n ? q - n : q);
    return q < 0 ? 0 : (q >= n ? n - 1 : q);
}

// ---- one cell per thread: any number of axes, any extent ----------------------------------------------------------------------
// EULER = false: out = lap(in), the ghost cells of `in` are read (the caller has set them).  EULER = true: one Euler step, the
// neighbours beyond a wall come from f32p_map - the ghost cells of `in` are neither read nor written.
template <int NDIM, bool EULER>
__global__ void __launch_bounds__(256) f32p_generic_kernel(F32pArgs a, const float *__restrict__ in, float *__restrict__ out)
{
    // blockIdx.y walks the planes of axis 0 (strided beyond the limit of a launch), blockIdx.x / threadIdx.x the cells of a plane in
    // C order: one 32-bit division per cell (the host checks that a plane has fewer than 2^31 cells)
    const unsigned n2 = (unsigned)a.n2, plane = (unsigned)(a.n1 * a.n2);
    for (long i = blockIdx.y; i < a.n0; i += gridDim.y) {
        for (unsigned t = blockIdx.x * 256u + threadIdx.x; t < plane; t += gridDim.x * 256u) {
            const long j = t / n2, k = t - (unsigned)j * n2;
            const float *c = in + a.off + i * a.p0 + j * a.p1 + k;
            const float cv = *c, two = cv + cv;
            float acc = 0.0f;
            if (NDIM >= 3) {
                const float l = EULER ? c[(f32p_map(i - 1, a.n0, a.per0) - i) * a.p0] : c[-a.p0];
                const float h = EULER ? c[(f32p_map(i + 1, a.n0, a.per0) - i) * a.p0] : c[a.p0];
                acc = ((l - two) + h) * a.s0;
            }
            if (NDIM >= 2) {
                const float l = EULER ? c[(f32p_map(j - 1, a.n1, a.per1) - j) * a.p1] : c[-a.p1];
                const float h = EULER ? c[(f32p_map(j + 1, a.n1, a.per1) - j) * a.p1] : c[a.p1];
                const float t1 = ((l - two) + h) * a.s1;
                acc = NDIM >= 3 ? acc + t1 : t1;
            }
            {
                const float l = EULER ? c[f32p_map(k - 1, a.n2, a.per2) - k] : c[-1];
                const float h = EULER ? c[f32p_map(k + 1, a.n2, a.per2) - k] : c[1];
                const float t2 = ((l - two) + h) * a.s2;
                acc = NDIM >= 2 ? acc + t2 : t2;
            }
            out[a.o_off + i * a.o_s0 + j * a.o_s1 + k] = EULER ? cv + a.dt * (a.D * acc) : acc;
        }
    }
}

// ---- the Laplacian of 3-D grids whose fastest axis is a multiple of four cells: register march along axis 0 -----------------------
// A wave owns `seg` planes x R rows x 256 cells: a lane holds four cells of a row (one aligned 16-byte access on the 128-byte-aligned
// rows) for the R rows and their two neighbour rows, in three planes (below / centre / above); the neighbours along the fastest axis
// come from the adjacent lanes by DPP, the two cells outside the chunk by one scalar load each in lanes 0 and 63.  The ghost cells of
// `in` are read.  Registers: (R + (R + 2) + (R + 2)) x 4 = 64 data VGPRs at R = 4 (four waves per SIMD: at most 128); no LDS.  (A fourth
// plane in flight, rotated by name, took 182 registers and was slower: profiles/f32p_time.md.)
__global__ void __launch_bounds__(256) lap32_kernel(F32pArgs a, const float *__restrict__ in, float *__restrict__ out)
{
    constexpr int R = kF32pRows;
    const int lane = threadIdx.x & 63;
    const long w = blockIdx.x * 4L + (threadIdx.x >> 6);
    const long xc = w % a.nxc, yt = (w / a.nxc) % a.nyt, sg = w / (a.nxc * (long)a.nyt);
    if (sg >= a.nseg) return;                                   // (whole waves: there is no barrier in this kernel)
    const long base = xc * 256 + 4 * lane;
    const bool active = base < a.n2;                            // n2 % 4 == 0: a vector lies inside the row or outside it
    const long lbase = active ? base : 0;
    const bool first = lane == 0, last = active && (lane == 63 || base + 4 >= a.n2);
    const long j0 = yt * R, i0 = sg * a.seg, i1 = i0 + a.seg < a.n0 ? i0 + a.seg : a.n0;
    long ro[R + 2];                                             // rows j0 - 1 .. j0 + R; rows beyond the upper ghost row are not needed: clamped
#pragma unroll
    for (int r = 0; r < R + 2; r++) {
        const long j = j0 - 1 + r;
        ro[r] = (j > a.n1 ? a.n1 : j) * a.p1;
    }
    const float *p = in + a.off + lbase;
    f4 prev[R], cur[R + 2], nxt[R + 2];
#pragma unroll
    for (int r = 0; r < R; r++) prev[r] = *(const f4 *)(p + (i0 - 1) * a.p0 + ro[r + 1]);
#pragma unroll
    for (int r = 0; r < R + 2; r++) cur[r] = *(const f4 *)(p + i0 * a.p0 + ro[r]);
    for (long i = i0; i < i1; i++) {
        const float *pc = p + i * a.p0;
#pragma unroll
        for (int r = 0; r < R + 2; r++) nxt[r] = *(const f4 *)(pc + a.p0 + ro[r]);
#pragma unroll
        for (int r = 0; r < R; r++) {
            const f4 c = cur[r + 1];
            float el = 0.0f, er = 0.0f;
            if (first) el = pc[ro[r + 1] - 1];                  // the lower ghost cell, or the last cell of the chunk before
            if (last) er = pc[ro[r + 1] + 4];                   // the upper ghost cell, or the first cell of the next chunk
            const float xl = f32p_shr1(el, c.w);
            float xr = f32p_shl1(er, c.x);
            if (last) xr = er;
            const f4 v = f32p_lap_row(c, prev[r], nxt[r + 1], cur[r], cur[r + 2], xl, xr, a.s0, a.s1, a.s2);
            if (active && j0 + r < a.n1) *(f4 *)(out + a.o_off + i * a.o_s0 + (j0 + r) * a.o_s1 + base) = v;
        }
#pragma unroll
        for (int r = 0; r < R; r++) prev[r] = cur[r + 1];
#pragma unroll
        for (int r = 0; r < R + 2; r++) cur[r] = nxt[r];
    }
}

// ---- two Euler steps of the diffusion equation per sweep, 3-D grids, every axis periodic or zero-derivative ---------------------
// out = E(E(in)), E(u) = u + dt * (D * lap(u)), bit for bit two single steps: the intermediate level u1 = E(in) is an fp32 value
// whether it is stored or not.  A workgroup of NW <= 4 waves spans the WHOLE fastest axis (n2 <= 1024, n2 % 4 == 0; wave w owns cells
// 256 w .. 256 w + 255) for R rows of axis 1 and `seg` planes of axis 0, and marches along axis 0:
//   level 0: a lane keeps three planes of R + 4 rows (two rows of halo on either side), cells beyond a wall by f32p_map (wrapped /
//            clamped loads: the ghost cells of `in` are never read); the neighbours along the fastest axis by DPP, the cell outside the
//            wave's chunk by a scalar load in lanes 0 / last;
//   level 1: three planes of R + 2 rows in registers, computed redundantly on the halo rows ((R + 2) / R of the level-1 work); a
//            zero-derivative wall makes the level-1 row / plane beyond it a COPY of the adjacent one (it is not recomputed from mirrored
//            level-0 data: (l - 2c) + r is not symmetric in l and r); the two level-1 cells outside a wave's chunk travel through LDS
//            (3 slots x 4 waves x 2 sides x R floats = 384 bytes, one barrier per plane);
//   level 2: R rows, stored with aligned 16-byte accesses.
// A march starts with two level-1 planes computed directly (four plane loads), then every plane costs one plane load, one level-1 plane
// and one level-2 plane; level 2 runs one plane behind level 1, so that the plane loads are in flight while it is computed.  Budget at R = 4: level 0 (8 + 8 + 6) x 4 = 88, level 1 (4 + 6 + 6) x 4 = 64 data VGPRs, <= 256 in all
// (two waves per SIMD at least; __launch_bounds__(256)), 384 bytes of LDS, no scratch.
struct F32pPlane { f4 v[kF32pRows + 4]; };
struct F32pLevel1 { f4 v[kF32pRows + 2]; };

struct F32pTile {
    long ro[kF32pRows + 4];     // offsets of the mapped rows j0 - 2 .. j0 + R + 1 (wave-uniform; the plane pointer carries the lane's column)
    long xl, xr;                // offsets within a row of the cells left / right of the lane's four cells, mapped
    long j0;
    bool first, last, active;
    int wave, nw;
};

__device__ __forceinline__ void f32p_load_plane(const F32pArgs &a, const F32pTile &t, const float *__restrict__ p, long q, F32pPlane &P)
{
    const float *pp = p + f32p_map(q, a.n0, a.per0) * a.p0;
#pragma unroll
    for (int r = 0; r < kF32pRows + 4; r++) P.v[r] = *(const f4 *)(pp + t.ro[r]);
}

// level 1 of the rows j0 - 1 .. j0 + R of plane q (B: that plane of level 0, A / C: the planes below / above)
__device__ __forceinline__ void f32p_level1(const F32pArgs &a, const F32pTile &t, const float *__restrict__ p, long q, const F32pPlane &A,
                                            const F32pPlane &B, const F32pPlane &C, F32pLevel1 &L)
{
    constexpr int R = kF32pRows;
    const float *pp = p + f32p_map(q, a.n0, a.per0) * a.p0;
#pragma unroll
    for (int r = 0; r < R + 2; r++) {
        const f4 c = B.v[r + 1];
        const long row = t.ro[r + 1];
        float el = 0.0f, er = 0.0f;
        if (t.first) el = pp[row + t.xl];
        if (t.last) er = pp[row + t.xr];
        const float xl = f32p_shr1(el, c.w);
        float xr = f32p_shl1(er, c.x);
        if (t.last) xr = er;
        const f4 lap = f32p_lap_row(c, A.v[r + 1], C.v[r + 1], B.v[r], B.v[r + 2], xl, xr, a.s0, a.s1, a.s2);
        L.v[r] = f32p_euler_row(c, lap, a.D, a.dt);
    }
    if (!a.per1) {                                              // zero-derivative walls of axis 1: copies, wave-uniform conditions
        if (t.j0 == 0) L.v[0] = L.v[1];
#pragma unroll
        for (int r = 1; r < R + 2; r++)
            if (t.j0 - 1 + r == a.n1) L.v[r] = L.v[r - 1];
    }
}

// the level-1 cells at the two ends of the wave's chunk, rows j0 .. j0 + R - 1, into buffer `buf`
__device__ __forceinline__ void f32p_publish(const F32pTile &t, float *lds, int buf, const F32pLevel1 &L)
{
    constexpr int R = kF32pRows;
    float *dst = lds + ((buf * 4 + t.wave) * 2) * R;
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (t.first) dst[r] = L.v[r + 1].x;
        if (t.last) dst[R + r] = L.v[r + 1].w;
    }
}

// level 2 of plane q from level 1 (Lc: that plane, Lp / Ln: below / above); the edges of Lc are in buffer `buf`
__device__ __forceinline__ void f32p_level2(const F32pArgs &a, const F32pTile &t, const float *lds, int buf, long q, long base,
                                            const F32pLevel1 &Lp, const F32pLevel1 &Lc, const F32pLevel1 &Ln, float *__restrict__ out)
{
    constexpr int R = kF32pRows;
    const int wl = t.wave > 0 ? t.wave - 1 : t.nw - 1, wr = t.wave < t.nw - 1 ? t.wave + 1 : 0;
    const float *left = lds + ((buf * 4 + wl) * 2 + 1) * R, *right = lds + ((buf * 4 + wr) * 2) * R;
    const bool wall_l = t.wave == 0 && !a.per2, wall_r = t.wave == t.nw - 1 && !a.per2;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const f4 c = Lc.v[r + 1];
        float el = 0.0f, er = 0.0f;
        if (t.first) el = wall_l ? c.x : left[r];
        if (t.last) er = wall_r ? c.w : right[r];
        const float xl = f32p_shr1(el, c.w);
        float xr = f32p_shl1(er, c.x);
        if (t.last) xr = er;
        const f4 lap = f32p_lap_row(c, Lp.v[r + 1], Ln.v[r + 1], Lc.v[r], Lc.v[r + 2], xl, xr, a.s0, a.s1, a.s2);
        const f4 v = f32p_euler_row(c, lap, a.D, a.dt);
        if (t.active && t.j0 + r < a.n1) *(f4 *)(out + a.o_off + q * a.o_s0 + (t.j0 + r) * a.o_s1 + base) = v;
    }
}

// one plane of the march: on entry A / B = level 0 of planes q / q + 1, X / Y / Z = level 1 of planes q - 2 / q - 1 / q with the edges of
// Y published in slot `rd`.  The loads of level 0 of plane q + 2 (into C) are issued first and are in flight while level 2 of plane
// q - 1 is computed and stored; then level 1 of plane q + 1 replaces X and its edges go to slot `wr` (the slot read one plane earlier:
// every wave has passed the barrier behind that read).  q == q1: the last plane of the march, nothing more to load or to prepare.
__device__ __forceinline__ void f32p_march_plane(const F32pArgs &a, const F32pTile &t, const float *__restrict__ p, float *lds, long q, long q1,
                                                 int rd, int wr, long base, const F32pPlane &A, const F32pPlane &B, F32pPlane &C, F32pLevel1 &X,
                                                 const F32pLevel1 &Y, const F32pLevel1 &Z, float *__restrict__ out)
{
    const bool more = q < q1;
    if (more) f32p_load_plane(a, t, p, q + 2, C);
    f32p_level2(a, t, lds, rd, q - 1, base, X, Y, Z, out);
    if (more) {
        if (!a.per0 && q + 1 == a.n0) X = Z;                    // zero-derivative wall of axis 0: level 1 beyond it is a copy
        else f32p_level1(a, t, p, q + 1, A, B, C, X);
        f32p_publish(t, lds, wr, X);
    }
    __syncthreads();
}

__global__ void __launch_bounds__(256) euler32_kernel(F32pArgs a, const float *__restrict__ in, float *__restrict__ out)
{
    constexpr int R = kF32pRows;
    __shared__ float lds[3 * 4 * 2 * R];
    F32pTile t;
    const int lane = threadIdx.x & 63;
    t.wave = threadIdx.x >> 6;
    t.nw = blockDim.x >> 6;
    const long yt = blockIdx.x % a.nyt, sg = blockIdx.x / a.nyt;      // (the host launches nyt * nseg workgroups: every one has work)
    const long base = t.wave * 256L + 4 * lane;
    t.active = base < a.n2;
    const long lbase = t.active ? base : 0;
    t.first = lane == 0;
    t.last = t.active && (lane == 63 || base + 4 >= a.n2);
    t.j0 = yt * R;
#pragma unroll
    for (int r = 0; r < R + 4; r++) t.ro[r] = f32p_map(t.j0 - 2 + r, a.n1, a.per1) * a.p1;
    t.xl = f32p_map(lbase - 1, a.n2, a.per2) - lbase;
    t.xr = f32p_map(lbase + 4, a.n2, a.per2) - lbase;
    const long q0 = sg * a.seg, q1 = q0 + a.seg < a.n0 ? q0 + a.seg : a.n0;
    const float *p = in + a.off + lbase;

    F32pPlane P0, P1, P2;
    F32pLevel1 L0, L1, L2;
    // start: level 1 of planes q0 - 1 (L0) and q0 (L1) directly, level 0 of planes q0 (P0) and q0 + 1 (P1)
    f32p_load_plane(a, t, p, q0 - 1, P2);
    f32p_load_plane(a, t, p, q0, P0);
    f32p_load_plane(a, t, p, q0 + 1, P1);
    f32p_level1(a, t, p, q0, P2, P0, P1, L1);
    if (!a.per0 && q0 == 0) {
        L0 = L1;
    } else {
        F32pPlane Pm;
        f32p_load_plane(a, t, p, q0 - 2, Pm);
        f32p_level1(a, t, p, q0 - 1, Pm, P2, P0, L0);
    }
    f32p_publish(t, lds, 0, L1);
    f32p_load_plane(a, t, p, q0 + 2, P2);
    if (!a.per0 && q0 + 1 == a.n0) L2 = L1;
    else f32p_level1(a, t, p, q0 + 1, P0, P1, P2, L2);
    f32p_publish(t, lds, 1, L2);
    __syncthreads();
    // the march, unrolled by three so that planes, levels and LDS slots rotate by name (no register moves); level 2 runs one plane
    // behind level 1, so the loop ends one plane after the last one (the conditions are the same for every wave of the workgroup)
    for (long q = q0 + 1; q <= q1; q += 3) {
        f32p_march_plane(a, t, p, lds, q, q1, 0, 2, base, P1, P2, P0, L0, L1, L2, out);
        if (q + 1 > q1) break;
        f32p_march_plane(a, t, p, lds, q + 1, q1, 1, 0, base, P2, P0, P1, L1, L2, L0, out);
        if (q + 2 > q1) break;
        f32p_march_plane(a, t, p, lds, q + 2, q1, 2, 1, base, P0, P1, P2, L2, L0, L1, out);
    }
}
