// pdehip_march.inc — the hot kernel (included by pdehip_kernels.hip inside namespace pdehip).
//
// Register-pipelined Laplacian with a fused pointwise epilogue and (template IBC) boundary
// conditions evaluated ON THE FLY on the input side.
//
// A wavefront owns a tile of RY rows x CZ chunks (one chunk = 64 lanes x 16 bytes) and marches over
// `lx` planes of the slowest axis keeping the planes i-1 (centre rows), i and i+1..i+PF in
// registers.  Addressing: every row/plane base is wave-uniform (SGPR pair); a lane contributes one
// 32-bit offset and the chunk offset is an instruction immediate — no per-load 64-bit VALU math.
// Lanes beyond the end of a row are NOT clamped: they read the upper ghost cell / row padding /
// the next row (always inside the allocation, see kAllocSlack) and never store; the first idle
// lane therefore naturally holds the ghost cell its left neighbour needs.  A row length that is not a
// multiple of the 16-byte vector ends INSIDE a lane's vector: that lane computes all its elements (the
// ones past the row end from the ghost cell / padding it loaded) and stores only the valid ones
// (`nval`), so any row length runs in this kernel — no cliff to the one-cell-per-thread kernel.
//
// IBC: for a face whose BC is `ghost = const + factor * arr[idx]` with scalar coefficients
// (pde/grids/boundaries/local.py:1611-1636) the kernel never reads the ghost layer: the halo row /
// plane / cell is loaded from layer `idx` instead and transformed in registers — the same
// arithmetic as the ghost-cell kernel, so results are bit-identical, but an Euler step needs no
// ghost pass at all (a separate pass over the ghost cells of the fastest axis alone costs 8 % of
// the step: 4 KiB-strided 8-byte accesses).
//
// TAILS: the instance for rows that end inside a lane's vector or leave whole chunks of the tile beyond the row.  Rows that
// are a multiple of the vector AND fill their tiles' chunks take the TAILS = false instance, which carries none of that
// bookkeeping (same-box A/B at 512^3 fp64: 0.394-0.415 ms without it, 0.444-0.475 ms with it — registers, not branches).
template <typename T, int VEC, int RY, int CZ, int WY, int PF, int MODE, bool HAS_X, bool Y_IS_IN, bool IBC, bool TAILS, bool NT = false>
__device__ __forceinline__ void lap_march_body(const LapArgs &a)
{
    typedef typename VecT<T, VEC>::type V;
    constexpr int CW = 64 * VEC;   // cells per chunk
    constexpr int NP = HAS_X ? PF + 1 : 1;
    // the Runge-Kutta stage epilogue (LapArgs::st_*) follows the built-in slope (LAP_STAGE) or, in run-time builds that
    // ask for it, the generated one (LAP_CUSTOM with PDE_STAGE)
#ifdef PDE_STAGE
    constexpr bool kStage = MODE == LAP_STAGE || (MODE == LAP_CUSTOM && PDE_STAGE);
#else
    constexpr bool kStage = MODE == LAP_STAGE;
#endif
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform -> SGPR
    const unsigned lo = (unsigned)lane * VEC;                        // the lane's only address term

    // fixed-point iteration (st_kind 5) of a step that has already converged or failed: nothing to do (uniform: one scalar load)
    if (kStage && a.st_kind == 5) {
        if (fixedpoint_stopped(a.st_err)) return;
        fixedpoint_announce(a.st_err, a.nblocks * WY);   // (no strip in front of a stage sweep)
    }
    const int fp_slot = (int)blockIdx.x * WY + (int)(threadIdx.x >> 6);   // st_kind 5: the wave's slot of the convergence norm (a vector register on purpose)
    const long bid0 = (long)blockIdx.x - a.strip_blocks;   // (a multiple of 8 workgroups in front belong to the strip of split rows)
    long bid = a.no_swizzle ? bid0 : xcd_swizzle(bid0, a.nblocks);
    const long tz = bid % a.ntz;
    bid /= a.ntz;
    const long ty = bid % a.nty;
    const long xc = bid / a.nty;

    const long kw = tz * (CW * CZ);                 // first cell of the wave tile (valid index)
    const long j0 = ty * (WY * RY) + (long)w * RY;  // first row of the wave tile
    if (j0 >= a.n1) {                               // whole wave outside (no barriers are used)
        if (kStage && a.st_kind == 5) fixedpoint_wave_partial(a.st_err, 0.0, fp_slot);   // (its slot of the convergence norm)
        return;
    }
    const long i0 = xc * a.lx;
    const long i1 = (i0 + a.lx < a.n0) ? i0 + a.lx : a.n0;

    bool ok[CZ];
    int nval[CZ];   // valid cells of the lane's vector: VEC inside the row, 1..VEC-1 in the lane the row ends in, <= 0 beyond
#pragma unroll
    for (int c = 0; c < CZ; c++) {
        const long left = a.n2 - (kw + c * CW + (long)lo);
        ok[c] = left > 0;
        nval[c] = TAILS ? (left >= VEC ? VEC : (int)left) : (left > 0 ? VEC : 0);
    }
    // wave-uniform: chunks that lie entirely beyond the row (and its upper ghost cell, which the first idle lane presents
    // to its left neighbour) are skipped — a tile of CZ chunks over the end of a short row costs only its active chunks
    bool act[CZ];
#pragma unroll
    for (int c = 0; c < CZ; c++) act[c] = !TAILS || kw + (long)c * CW <= a.n2;
    // stores of a vector whose lane may hold the end of the row
    auto store = [&](T *p, const V &v, int n) {
        // NT (a compile-time instance like in euler2_kernel: a run-time branch around the two kinds of store is merged into plain
        // stores): streaming stores for outputs larger than the 256 MB Infinity Cache - 0.379 vs 0.397-0.406 ms per 512^3 fp64
        // Laplacian in a same-box A/B (profiles/r03_ab_nontemporal.md); non-temporal LOADS cost 40 % (halo rows miss the L2)
        if (!TAILS || n >= VEC) {
            if (NT) __builtin_nontemporal_store(v, (V *)p);
            else *(V *)p = v;
            return;
        }
#pragma unroll
        for (int q = 0; q < VEC - 1; q++)
            if (q < n) p[q] = v[q];
    };

    // wave-uniform row offsets (relative to a plane base, tile origin included).  ytr[r] != 0 marks a
    // halo row that is a virtual row: loaded from row idx and transformed (1 = lower, 2 = upper BC).
    long roff[RY + 2];
    int ytr[RY + 2];
#pragma unroll
    for (int r = 0; r < RY + 2; r++) {
        long j = j0 + r - 1;
        ytr[r] = 0;
        if (IBC && j == -1 && a.ibc[1][0].on) { j = a.ibc[1][0].idx; ytr[r] = 1; }
        else if (IBC && j == a.n1 && a.ibc[1][1].on) { j = a.ibc[1][1].idx; ytr[r] = 2; }
        else if (j > a.n1) j = a.n1;   // rows beyond the grid: clamp onto the upper ghost row (unused)
        roff[r] = a.off + j * a.p1 + kw;
    }
    // halo cells of the tile: lanes < 32 fetch the cell left of it, lanes >= 32 the cell right of it
    long zh_rel = (lane < 32) ? -1 : (long)CW * CZ;
    if (kw + zh_rel > a.n2) zh_rel = a.n2 - kw;
    bool zh_tr = false;
    double zh_c = 0, zh_f = 0;
    if (IBC) {
        // (no dynamic indexing of the argument struct: it would be spilled to scratch memory)
        const bool upper = lane >= 32;
        const bool at_edge = upper ? (kw + (long)CW * CZ >= a.n2) : (kw == 0);
        const bool on = upper ? (a.ibc[2][1].on != 0) : (a.ibc[2][0].on != 0);
        if (at_edge && on) {
            zh_rel = (upper ? a.ibc[2][1].idx : a.ibc[2][0].idx) - kw;
            zh_tr = true;
            zh_c = upper ? a.ibc[2][1].c : a.ibc[2][0].c;
            zh_f = upper ? a.ibc[2][1].f : a.ibc[2][0].f;
        }
    }

    // uniform: upper virtual cell of a row that ends inside this tile needs a fix-up (see load_plane)
    const bool zfix = IBC && a.ibc[2][1].on && (kw + (long)CW * CZ > a.n2);
    // element of the lane's vector that holds the upper virtual cell (index n2 of the row), -1 = not in this lane
    int zq[CZ];
#pragma unroll
    for (int c = 0; c < CZ; c++) {
        const long d = a.n2 - (kw + c * CW + (long)lo);
        zq[c] = (d >= 0 && d < VEC) ? (int)d : -1;
    }

    const T *in = (const T *)a.in;
    T *out = (T *)a.out;
    const T *yin = (const T *)a.y;

    V pl[NP][RY + 2][CZ];   // [0] = current plane, [1..] = prefetched planes
    T zh[NP][RY];
    V prev[HAS_X ? RY : 1][CZ];
    // skipped chunks are never loaded: give their registers a defined value once
#pragma unroll
    for (int c = 0; c < CZ; c++)
        if (!act[c]) {
#pragma unroll
            for (int q = 0; q < VEC; q++) {
#pragma unroll
                for (int s_ = 0; s_ < NP; s_++)
#pragma unroll
                    for (int r = 0; r < RY + 2; r++) pl[s_][r][c][q] = 0;
#pragma unroll
                for (int r = 0; r < (HAS_X ? RY : 1); r++) prev[r][c][q] = 0;
            }
        }

    // ghost = const + factor * value, rounded to the storage type like a stored ghost cell
    auto virt = [&](V v, double c, double f) {
        V o;
#pragma unroll
        for (int q = 0; q < VEC; q++) o[q] = (T)(c + f * (double)v[q]);
        return o;
    };
    // plane index -> source plane + BC transform (0 none, 1 lower, 2 upper)
    auto plane_src = [&](long &i) {
        if (IBC && HAS_X) {
            if (i == -1 && a.ibc[0][0].on) { i = a.ibc[0][0].idx; return 1; }
            if (i == a.n0 && a.ibc[0][1].on) { i = a.ibc[0][1].idx; return 2; }
        }
        return 0;
    };

    auto load_plane = [&](long i, int slot) {
        const int xtr = plane_src(i);
        const T *p = in + i * a.p0;   // uniform
#pragma unroll
        for (int r = 0; r < RY + 2; r++) {
            const T *prow = p + roff[r];   // uniform
#pragma unroll
            for (int c = 0; c < CZ; c++)
                if (act[c]) pl[slot][r][c] = PDEHIP_LDV((const V *)(prow + lo + c * CW));
        }
#pragma unroll
        for (int r = 0; r < RY; r++) zh[slot][r] = (p + roff[r + 1])[zh_rel];
        if (IBC) {
#pragma unroll
            for (int r = 0; r < RY; r++)
                zh[slot][r] = zh_tr ? (T)(zh_c + zh_f * (double)zh[slot][r]) : zh[slot][r];
#pragma unroll
            for (int r = 0; r < RY + 2; r++)
                if (ytr[r]) {
                    const double c = (ytr[r] == 1) ? a.ibc[1][0].c : a.ibc[1][1].c, f = (ytr[r] == 1) ? a.ibc[1][0].f : a.ibc[1][1].f;
#pragma unroll
                    for (int cz = 0; cz < CZ; cz++) pl[slot][r][cz] = virt(pl[slot][r][cz], c, f);
                }
            if (xtr) {
                const double c = (xtr == 1) ? a.ibc[0][0].c : a.ibc[0][1].c, f = (xtr == 1) ? a.ibc[0][0].f : a.ibc[0][1].f;
#pragma unroll
                for (int r = 0; r < RY + 2; r++)
#pragma unroll
                    for (int cz = 0; cz < CZ; cz++) pl[slot][r][cz] = virt(pl[slot][r][cz], c, f);
            }
            if (zfix) {
                // the row ends inside the tile: the first idle lane must hold the upper virtual cell,
                // because its left neighbour takes it through the DPP shift / readlane
#pragma unroll
                for (int r = 0; r < RY; r++) {
                    const double vr = readlane_d((double)zh[slot][r], 63);
#pragma unroll
                    for (int cz = 0; cz < CZ; cz++)
#pragma unroll
                        for (int q = 0; q < (TAILS ? VEC : 1); q++)
                            if (zq[cz] == q) pl[slot][r + 1][cz][q] = (T)vr;
                }
            }
        }
    };

    if (HAS_X) {
        long ip = i0 - 1;   // plane i0-1: centre rows only
        const int xtr = plane_src(ip);
        const T *p = in + ip * a.p0;
#pragma unroll
        for (int r = 0; r < RY; r++) {
            const T *prow = p + roff[r + 1];
#pragma unroll
            for (int c = 0; c < CZ; c++)
                if (act[c]) prev[r][c] = PDEHIP_LDV((const V *)(prow + lo + c * CW));
        }
        if (IBC && xtr) {
            const double c = (xtr == 1) ? a.ibc[0][0].c : a.ibc[0][1].c, f = (xtr == 1) ? a.ibc[0][0].f : a.ibc[0][1].f;
#pragma unroll
            for (int r = 0; r < RY; r++)
#pragma unroll
                for (int cz = 0; cz < CZ; cz++) prev[r][cz] = virt(prev[r][cz], c, f);
        }
#pragma unroll
        for (int q = 0; q < PF; q++) load_plane((i0 + q > a.n0) ? a.n0 : i0 + q, q);
    } else {
        load_plane(0, 0);
    }

    double emax = 0;   // LAP_STAGE, st_kind 2 / 4: the lane's share of the error norm
    double esum = 0;   // st_kind 5: the lane's share of sum (new - prev)^2, cells in the order of the march
    for (long i = i0; i < i1; i++) {
        if (HAS_X) load_plane((i + PF > a.n0) ? a.n0 : i + PF, PF);   // clamped onto the upper ghost plane
#pragma unroll
        for (int r = 0; r < RY; r++) {
            const bool row_ok = (j0 + r) < a.n1;
            T *orow = out + a.o_off + i * a.o_s0 + (j0 + r) * a.o_s1 + kw;                 // uniform
            const T *yrow = (MODE == LAP_EULER && !Y_IS_IN) ? yin + i * a.p0 + a.off + (j0 + r) * a.p1 + kw : nullptr;
#pragma unroll
            for (int c = 0; c < CZ; c++) {
                if (!act[c]) continue;   // uniform
                const V cc = pl[0][r + 1][c], up = pl[0][r][c], dn = pl[0][r + 2][c];
                V yv;
                if (MODE == LAP_EULER && !Y_IS_IN) yv = *(const V *)(yrow + lo + c * CW);
                V syv, skv[5], stv;
                if (kStage) {
                    // state and earlier slopes at the cell itself (uniform base + the lane's offset)
                    const long eb = i * a.p0 + a.off + (j0 + r) * a.p1 + kw;
                    syv = *(const V *)((const T *)a.st_y + eb + lo + c * CW);
#pragma unroll
                    for (int m = 0; m < 5; m++) {
#pragma unroll
                        for (int q = 0; q < VEC; q++) skv[m][q] = 0;
                        // (kinds 4, 5: when st_k[1], the half step / the previous iterate, is the input array of this sweep its value at the cell is already in registers)
                        if (a.st_k[m] && !((a.st_kind == 4 || a.st_kind == 5) && m == 1 && a.st_k[1] == a.in)) skv[m] = *(const V *)((const T *)a.st_k[m] + eb + lo + c * CW);   // uniform
                    }
                }
                V exv[3];
                if (MODE == LAP_CUSTOM) {
#pragma unroll
                    for (int m = 0; m < 3; m++) {
#pragma unroll
                        for (int q = 0; q < VEC; q++) exv[m][q] = 0;
                        if (a.ex[m])   // uniform
                            exv[m] = *(const V *)((const T *)a.ex[m] + i * a.p0 + a.off + (j0 + r) * a.p1 + kw + lo + c * CW);
                    }
                }
                // neighbours across the chunk boundary: previous/next chunk of the same wave, or the halo
                double oldl = (double)zh[0][r], oldr = (double)zh[0][r];
                if (c > 0) oldl = readlane_d((double)pl[0][r + 1][c > 0 ? c - 1 : 0][VEC - 1], 63);
                if (c < CZ - 1) oldr = readlane_d((double)pl[0][r + 1][c < CZ - 1 ? c + 1 : c][0], 0);
                const double zl = wave_shr1(oldl, (double)cc[VEC - 1]);
                const double zr = wave_shl1(oldr, (double)cc[0]);
                V res, gxv, gyv;   // res doubles as the last gradient component (z)
#pragma unroll
                for (int q = 0; q < VEC; q++) {
                    const double cen = (double)cc[q];
                    const double left = (q == 0) ? zl : (double)cc[q > 0 ? q - 1 : 0];
                    const double right = (q == VEC - 1) ? zr : (double)cc[q < VEC - 1 ? q + 1 : q];
                    const double xm = HAS_X ? (double)prev[r][c][q] : 0.0, xp = HAS_X ? (double)pl[HAS_X ? 1 : 0][r + 1][c][q] : 0.0;
                    if (MODE <= LAP_CH_MU || MODE == LAP_CUSTOM || MODE == LAP_STAGE) {
                        const double vm = 2 * cen;
                        double lap;
                        if (HAS_X) {
                            // cartesian.py:220-227
                            const double lx = (xm - vm + xp) * a.sx;
                            const double ly = ((double)up[q] - vm + (double)dn[q]) * a.sy;
                            const double lz = (left - vm + right) * a.sz;
                            lap = lx + ly + lz;
                        } else {
                            // cartesian.py:147-151 (2-D; 1-D is handled by the generic kernel)
                            const double ly = ((double)up[q] - vm + (double)dn[q]) * a.sy;
                            const double lz = (left - vm + right) * a.sz;
                            lap = ly + lz;
                        }
                        if (MODE == LAP_CUSTOM) {
                            // run-time generated pointwise epilogue on (centre, laplacian, squared gradient,
                            // centre values of up to three more arrays, scalar parameters)
                            const double dyc = (double)dn[q] - (double)up[q], dzc = right - left;
                            double gsq = dyc * dyc * a.gs[1] + dzc * dzc * a.gs[2];                 // cartesian.py:665-668
                            if (HAS_X) { const double dxc = xp - xm; gsq = dxc * dxc * a.gs[0] + dyc * dyc * a.gs[1] + dzc * dzc * a.gs[2]; }
                            // per-axis derivatives (operators/common.py:60-110, :150-190); what the epilogue does not use is dropped
                            PdeDer d;
                            d.d1[0] = HAS_X ? (xp - xm) / a.dd1[0] : 0.0;
                            d.d2[0] = HAS_X ? (xp - vm + xm) * a.dd2[0] : 0.0;
                            d.d1[1] = dyc / a.dd1[1];
                            d.d2[1] = ((double)dn[q] - vm + (double)up[q]) * a.dd2[1];
                            d.d1[2] = dzc / a.dd1[2];
                            d.d2[2] = (right - vm + left) * a.dd2[2];
                            d.gr[0] = HAS_X ? (xp - xm) * a.dg[0] : 0.0;   // cartesian.py:451-454 (gradient), :876-879 (divergence)
                            d.gr[1] = dyc * a.dg[1];
                            d.gr[2] = dzc * a.dg[2];
                            res[q] = (T)pde_epilogue(cen, lap, gsq, (double)exv[0][q], (double)exv[1][q], (double)exv[2][q], a.par, d);
                        } else {
                            double yy = 0;
                            if (MODE == LAP_EULER) yy = Y_IS_IN ? cen : (double)yv[q];
                            res[q] = (T)epilogue<MODE>(lap, cen, yy, a.s1, a.s2, a.gamma);
                        }
                        if (kStage) {
                            const double kn = (double)res[q];   // the slope as stored (rounded to T)
                            if (a.st_kind == 0) {
                                // left to right like `y + b1*k1 + b2*k2 + ...` (lincomb_kernel), the new slope last
                                double acc = (double)syv[q];
#pragma unroll
                                for (int m = 0; m < 5; m++)
                                    if (a.st_k[m]) acc = acc + a.st_c[m] * (double)skv[m][q];
                                acc = acc + a.st_c[5] * kn;
                                stv[q] = (T)acc;
                            } else if (a.st_kind == 1) {
                                // pde/solvers/runge_kutta.py:60 (rk4_combine_kernel)
                                const double s = ((double)skv[0][q] + 2 * (double)skv[1][q] + 2 * (double)skv[2][q] + kn) / 6;
                                stv[q] = (T)((double)syv[q] + s);
                            } else if (a.st_kind == 3) {
                                // pde/solvers/adams_bashforth.py:44 (ab2_combine_kernel): st_c[5] = dt, st_k[0] = the previous rate
                                const double s = a.st_c[5] * (1.5 * kn - 0.5 * (double)skv[0][q]);
                                stv[q] = (T)((double)syv[q] + s);
                            } else if (a.st_kind == 5) {
                                // fixed-point iteration, pde/solvers/implicit.py:94-97 / crank_nicolson.py:98-103 (fixedpoint_combine_kernel):
                                // st_k[1] = the previous iterate (the input of this sweep, or of the first pass of the expression), kn = rhs(prev), syv = state_t
                                const double pv = (a.st_k[1] == a.in) ? cen : (double)skv[1][q];
                                double nv;
                                if (!a.st_k[0]) {
                                    nv = (double)syv[q] + a.st_c[5] * kn;
                                } else {
                                    const double cn = (double)syv[q] + a.st_c[5] * (kn + (double)skv[0][q]);
                                    nv = a.st_c[0] * pv + a.st_c[1] * cn;
                                }
                                stv[q] = (T)nv;
                                const double df = (double)stv[q] - pv;
                                if (q < nval[c] && row_ok) esum = esum + df * df;
                            } else if (a.st_kind == 4) {
                                // end of an adaptive Euler attempt, pde/backends/numba/_solvers.py:381-394 (euler_adaptive_combine_kernel):
                                // the input of this sweep is the half step, kn = dt/2 * rate_midpoint, st_k[0] = the carried rate, st_c[0] = dt
                                stv[q] = (T)((a.st_k[1] == a.in ? cen : (double)skv[1][q]) + kn);
                                const double large = (double)(T)((double)syv[q] + a.st_c[0] * (double)skv[0][q]);
                                if (q < nval[c] && row_ok) emax = max_nan(emax, abs_nan_canon(large - (double)stv[q]));
                            } else {
                                // pde/solvers/runge_kutta.py:117-125, :147-150 (rkf45_combine_kernel, same quotients)
                                const double r1 = 1.0 / 360, r3 = -128.0 / 4275, r4 = -2197.0 / 75240, r5 = 1.0 / 50, r6 = 2.0 / 55;
                                const double c1 = 25.0 / 216, c3 = 1408.0 / 2565, c4 = 2197.0 / 4104, c5 = -1.0 / 5;
                                const double d1 = skv[0][q], d3 = skv[1][q], d4 = skv[2][q], d5 = skv[3][q], d6 = kn;
                                const double el = r1 * d1 + r3 * d3 + r4 * d4 + r5 * d5 + r6 * d6;
                                if (q < nval[c] && row_ok) emax = max_nan(emax, abs_nan_canon(el));
                                stv[q] = (T)((double)syv[q] + c1 * d1 + c3 * d3 + c4 * d4 + c5 * d5);
                            }
                        }
                    } else if (MODE == LAP_GRAD_C || MODE == LAP_GRAD_F || MODE == LAP_GRAD_B) {
                        // cartesian.py:464-474, :516-548: (hi - lo) * (0.5/dx), (hi - c) / (c - lo) * (1/dx)
                        const double dx_ = (MODE == LAP_GRAD_C) ? xp - xm : (MODE == LAP_GRAD_F) ? xp - cen : cen - xm;
                        const double dy_ = (MODE == LAP_GRAD_C) ? (double)dn[q] - (double)up[q] : (MODE == LAP_GRAD_F) ? (double)dn[q] - cen : cen - (double)up[q];
                        const double dz_ = (MODE == LAP_GRAD_C) ? right - left : (MODE == LAP_GRAD_F) ? right - cen : cen - left;
                        if (HAS_X) gxv[q] = (T)(dx_ * a.gs[0]);
                        gyv[q] = (T)(dy_ * a.gs[1]);
                        res[q] = (T)(dz_ * a.gs[2]);
                    } else if (MODE == LAP_GRADSQ_C) {
                        // cartesian.py:665-668, :745-748: sum (hi - lo)**2 * (0.25/dx**2)
                        const double dy_ = (double)dn[q] - (double)up[q], dz_ = right - left;
                        const double ty = dy_ * dy_ * a.gs[1], tz = dz_ * dz_ * a.gs[2];
                        if (HAS_X) { const double dx_ = xp - xm; res[q] = (T)(dx_ * dx_ * a.gs[0] + ty + tz); }
                        else res[q] = (T)(ty + tz);
                    } else {
                        // cartesian.py:674-688, :754-768: sum ((hi-c)**2 + (c-lo)**2) * (0.5/dx**2)
                        const double yl = (double)dn[q] - cen, yr = cen - (double)up[q], zl_ = right - cen, zr_ = cen - left;
                        const double ty = (yl * yl + yr * yr) * a.gs[1], tz = (zl_ * zl_ + zr_ * zr_) * a.gs[2];
                        if (HAS_X) { const double xl = xp - cen, xr = cen - xm; res[q] = (T)((xl * xl + xr * xr) * a.gs[0] + ty + tz); }
                        else res[q] = (T)(ty + tz);
                    }
                }
                if (ok[c] && row_ok) {
                    if (MODE == LAP_GRAD_C || MODE == LAP_GRAD_F || MODE == LAP_GRAD_B) {
                        // component-major output (dim, ...): x (3-D only), y, z
                        T *po = orow + lo + c * CW;
                        if (HAS_X) { store(po, gxv, nval[c]); store(po + a.o_sc, gyv, nval[c]); store(po + 2 * a.o_sc, res, nval[c]); }
                        else { store(po, gyv, nval[c]); store(po + a.o_sc, res, nval[c]); }
                    } else if (kStage) {
                        if (a.st_kind == 0 || a.st_kind == 3) store(orow + lo + c * CW, res, nval[c]);
                        store((T *)a.st_out + i * a.p0 + a.off + (j0 + r) * a.p1 + kw + lo + c * CW, stv, nval[c]);
                    } else {
                        store(orow + lo + c * CW, res, nval[c]);
                    }
                }
            }
        }
        if (HAS_X) {   // rotate the register pipeline
#pragma unroll
            for (int r = 0; r < RY; r++)
#pragma unroll
                for (int c = 0; c < CZ; c++) prev[r][c] = pl[0][r + 1][c];
#pragma unroll
            for (int q = 0; q < PF; q++) {
#pragma unroll
                for (int r = 0; r < RY + 2; r++)
#pragma unroll
                    for (int c = 0; c < CZ; c++) pl[q][r][c] = pl[q + 1][r][c];
#pragma unroll
                for (int r = 0; r < RY; r++) zh[q][r] = zh[q + 1][r];
            }
        }
    }
    if (kStage) {
        if (a.st_kind == 2 || a.st_kind == 4) {   // uniform: one atomic per wave (a launch has a few thousand waves)
            unsigned long long b = (unsigned long long)__double_as_longlong(emax);
#pragma unroll
            for (int ofs = 32; ofs >= 1; ofs >>= 1) {
                const unsigned long long o = __shfl_xor(b, ofs, 64);
                b = (o > b) ? o : b;
            }
            if (lane == 0 && b > *(volatile unsigned long long *)a.st_err) atomicMax((unsigned long long *)a.st_err, b);   // the cell only grows
        }
        if (a.st_kind == 5) fixedpoint_wave_partial(a.st_err, esum, fp_slot);   // uniform
    }
}

// The columns of split rows behind the vectorised part (launch_laplace_t): 3-D, ghost cells from memory.  A thread walks 8 rows of one
// column with the row neighbours in registers; the workgroups of the strip come FIRST in the launch, so their scattered 8-byte accesses
// (every operand in a cache line of its own) overlap with the streaming of the main part instead of following it as a launch of their own
// (44 us for the one extra column of 513^3, profiles/r04_time_sizes.md).  Same expressions as lap_generic_kernel.
template <typename T, int MODE>
__device__ __forceinline__ void lap_strip(const LapArgs &a)
{
    // rows per thread: 8 per column of the strip - the NUMBER of strip workgroups in front of the main part is what costs (520 of them at
    // 513^3: 0.44-0.47 ms; 2048 - four columns, or one cell per thread - 0.61-0.67 ms), so wider strips walk longer columns instead
    const int RS = 8 * a.strip_n2;
    const long njg = (a.n1 + RS - 1) / RS;
    const long total = a.n0 * njg * a.strip_n2;
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long k = a.n2 + t % a.strip_n2, jg = (t / a.strip_n2) % njg, i = t / (njg * a.strip_n2);   // (the columns of a row in neighbouring lanes: one cache line)
    const long j0 = jg * RS;
    const int nr = (int)((a.n1 - j0 < RS) ? a.n1 - j0 : RS);
    const T *c = (const T *)a.in + a.off + i * a.p0 + j0 * a.p1 + k;
    const T *yin = (const T *)(a.y ? a.y : a.in) + a.off + i * a.p0 + j0 * a.p1 + k;
    T *out = (T *)a.out + a.o_off + i * a.o_s0 + j0 * a.o_s1 + k;
    double up = (double)c[-a.p1], mid = (double)c[0];
    for (int r = 0; r < nr; r++, c += a.p1, yin += a.p1, out += a.o_s1) {
        const double dn = (double)c[a.p1];
        const double vm = 2 * mid;
        const double lx = ((double)c[-a.p0] - vm + (double)c[a.p0]) * a.sx;
        const double ly = (up - vm + dn) * a.sy;
        const double lz = ((double)c[-1] - vm + (double)c[1]) * a.sz;
        const double lap = lx + ly + lz;
        double yy = 0;
        if (MODE == LAP_EULER) yy = (double)yin[0];
        out[0] = (T)epilogue<MODE>(lap, mid, yy, a.s1, a.s2, a.gamma);
        up = mid;
        mid = dn;
    }
}

template <typename T, int VEC, int RY, int CZ, int WY, int PF, int MODE, bool HAS_X, bool Y_IS_IN, bool IBC, bool TAILS, bool NT = false>
__global__ void __launch_bounds__(64 * WY) lap_march_kernel(LapArgs a)
{
    if constexpr (HAS_X && MODE <= LAP_CH_MU && !IBC) {
        if (a.strip_blocks > 0 && (long)blockIdx.x < a.strip_blocks) {
            lap_strip<T, MODE>(a);
            return;
        }
    }
    lap_march_body<T, VEC, RY, CZ, WY, PF, MODE, HAS_X, Y_IS_IN, IBC, TAILS, NT>(a);
}
