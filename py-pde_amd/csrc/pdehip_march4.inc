// pdehip_march4.inc - four Euler steps of the diffusion equation per sweep, fp64, 3-D, every axis periodic:
//     out = E(E(E(E(in)))),   E(u) = u + s2 * (s1 * laplace(u))          pde/solvers/euler.py:172-175
// The 3-D counterpart of pdehip_tile2d.inc (time levels in LDS) with the march of pdehip_march2.inc: one read and one write of the field per
// FOUR steps.  Included inside namespace pdehip::exactv / pdehip::fastv by pdehip_kernels_e4.hip; geometry: pdehip_euler4_plan.h.
//
// A workgroup owns TY x TZ outputs (rows x fastest axis) and marches along axis 0 over an x-chunk of `lx` planes.  Level L (1 ... 4) is
// evaluated on the tile grown by 4 - L cells per side and on the chunk grown by 4 - L planes per end: the halo is recomputed, neighbouring
// workgroups read the same input lines (from L2).  Periodic wraps are resolved in the load addresses: rows and columns once, planes per phase.
//
// A thread owns the same patch of PY rows x 2 cells at every level and keeps, for each of the levels 0 ... 3, its own cells of three
// consecutive planes in registers.  Neighbours inside the patch come from those registers; the others from the LDS image of the level's middle
// plane.  The levels run skewed: iteration i (local planes count from the first loaded one) computes
//     level 1 at plane i + 1,   level 2 at plane i,   level 3 at plane i - 1,   level 4 at plane i - 2   (stored from i = 6 on)
// The loop is unrolled three times so that the rotation of the plane buffers is a renaming (like euler2_body).  What the first iterations
// compute from planes that do not exist yet (zeros) never reaches a stored cell: level L at plane p reads level L - 1 at p - 1 ... p + 1 only.
//
// The image (e4plan::image_index): per level, patch row and patch cell one array indexed by the patch number, sixteen arrays of 720 doubles
// between two guard runs of 36, inside the allocation of LEVELS * LROWS * LPITCH doubles.  Every neighbour is a constant offset of the
// thread's own index (e4plan::read_index): above [row 1][cell][patch - 36], below [row 0][cell][patch + 36], left [row][cell 1][patch - 1],
// right [row][cell 0][patch + 1].  Every access of a lane is a base plus its patch number, and the patches of a half-wave differ modulo 32,
// those of a quarter-wave modulo 16: no bank conflicts, whatever the base (tests/test_euler4_lanes.py computes the banks).  What a patch at the rim of the region reads - through the row wrap (patch - 1 of a
// row's first patch is the last one of the row above), from a neighbouring array or a guard run - is unspecified.  Such a value only ever
// feeds a cell outside the valid region of its level: level L is valid on the region of level 0 shrunk by L cells per side,
//     level 0: 40 x 72,   level 1: 38 x 70,   level 2: 36 x 68,   level 3: 34 x 66,   level 4: 32 x 64 (the outputs),
// a cell that is valid at level L has all four in-plane neighbours inside the region of level L - 1, and those are read where their owners
// stored them (the same test enumerates it).  The guard runs are zeroed once so that whole images compare equal; no result depends on it.
//
// A phase (one iteration) has two barriers, A and B (e4plan::SCHEDULE is this order as a table; tests/test_euler4_double_buffer.py replays
// it).  Image l holds the middle plane of level l; level l + 1 reads it in every phase and the middle plane of the NEXT iteration must take
// its place (level 0: plane i + 2, loaded earlier; level l: what level l - 1 computes in this phase).  A barrier per image guarded that
// overwrite against the reads and brought the waves into step four times per phase.  Now the images of levels 1 and 2 have a second buffer
// (e4plan::alt_index; dynamic LDS, an object of its own) and the two change places from phase to phase, p = the parity of the iteration:
//     store image 3               level 3's middle plane, computed by l = 2 of the phase before and still in its registers
//     l = 0: read image 0, level 1;   store image 1[1 - p]
//     barrier A                   every wave has read image 0
//     store image 0               plane i + 2
//     l = 1: read image 1[p], level 2;   store image 2[1 - p]
//     l = 2: read image 2[p], level 3    (stays in registers until B has passed)
//     l = 3: read image 3, level 4 -> the field (owner waves)
//     barrier B                   every wave has read image 3
// Waves run freely between two barriers, so a store and a read of one buffer are ordered exactly when a barrier lies between them:
//   * buffers 1[1 - p] and 2[1 - p] were last read in the phase before, ahead of its B, and are next read in the next phase, behind this B
//     (and its A);
//   * image 0 is read before A and written behind it; its next read lies behind B;
//   * image 3 is read before B and written behind it; its next read lies behind A of the next phase.
// The stores of levels 1 and 2 are issued where their data is produced and nothing waits for them but the next barrier.  The buffer bases
// are wave-uniform (scalar registers, swapped after B); a lane adds its patch number to them.  The prologue stores the middle planes of
// iteration 0 (parity 0) into the buffers 0 and zeroes the second buffers with their guard runs, behind one barrier.
//
// Waves have roles (e4plan::lane_patch, wave_levels; the lane -> patch map is not the row-major numbering of the image).  A patch is needed at
// as many levels as its distance from the rim of the region allows - an output patch at all four, the ring around the outputs at levels
// 1 ... 3, the outer ring at level 1 - and the map gathers the output patches in waves 0 ... 7, the halo patches in waves 8 ... 11, so that a
// halo wave skips, by scalar branches, the levels none of its patches is needed at: the neighbour reads, the arithmetic and the image stores
// of those levels (level 0's image stores and the plane loads stay), 42 wave-levels per phase instead of 48 and at most 11 instead of 12 on
// a SIMD.  Only the owner waves store to the field.  Every wave executes every barrier of every phase - the skips enclose no barrier - and
// the trip count depends on the workgroup alone.  The cells of a skipped level keep the zeros of the prologue in the image; they are read
// only by cells that are invalid at their own level, like the unspecified values above (tests/test_euler4_lanes.py enumerates it by lane
// and by role: whatever a valid cell reads was stored by a wave that executes that level).  The results are the same bits as before.
//
// Per cell the arithmetic is `laplace` + `update` of pdehip_march2.inc (cartesian.py:220-227) in the same order: bit-identical to four single
// steps in the exact build.  One thing is written differently: each `neighbour - 2 * centre` is one fused multiply-add (PDEHIP_E4_MINUS_TWICE:
// the doubling is exact, so the bits are the same) instead of a doubling shared by the three axes and a subtraction each - 10 fp64 instructions
// per cell and level where there were 11.  The kernel's time follows its fp64 instruction count (the fp64 pipe is busy for more than half of a
// launch and nothing that was rescheduled around it moved the time; profiles/euler4_vmcnt_time.md).
template <typename T, int M2>
__global__ void __launch_bounds__(e4plan::THREADS) euler4_kernel(const LapArgs a)
{
    static_assert(sizeof(T) == 8 && (M2 == E2_DIFFUSION || M2 == E2_DIFFUSION_UNIT), "fp64 diffusion only");
    using namespace e4plan;
    typedef typename VecT<T, 2>::type V;
    __shared__ __attribute__((aligned(16))) T lds[LEVELS * LROWS * LPITCH];
    // the second buffers of images 1 and 2 (ALT_BYTES of dynamic LDS): an object of its own, wherever it lies relative to `lds`
    extern __shared__ __attribute__((aligned(16))) unsigned char euler4_alt[];
    typedef __attribute__((address_space(3))) T LT;

    // the lane's patch and the wave's role (e4plan::lane_patch): both wave-uniform values are scalars, so every branch on them is one
    const int tid = lane_patch((int)threadIdx.x);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int nlev = wave_levels(wave);                        // the wave executes levels 1 ... nlev
    const bool owner = wave < OWNER_WAVES;                     // an owner wave: output patches only, and all of them are in owner waves
    const int py = tid / NPZ, pz = tid - py * NPZ;
    const int ly = py * PY, lz = 2 * pz;                       // first row / column of the patch in the region of level 0

    const long w = xcd_swizzle((long)blockIdx.x, a.nblocks);
    const long tiles = a.nty * a.ntz;
    const long xc = w / tiles, tile = w - xc * tiles;
    const long ty = tile / a.ntz, tz = tile - ty * a.ntz;
    const long x0 = xc * a.xstride;
    const int lx = (int)((a.n0 - x0 < (long)a.lx) ? a.n0 - x0 : (long)a.lx);
    auto wrap = [](long i, long n) { return i < 0 ? i + n : (i >= n ? i - n : i); };   // (n >= the tile / 16 planes: one wrap is enough)

    long roff[PY];   // element offset of the patch's rows in a plane
    const long zc = wrap(tz * TZ - HALO + lz, a.n2);           // even: a patch never straddles the wrap
#pragma unroll
    for (int r = 0; r < PY; r++) roff[r] = a.off + wrap(ty * TY - HALO + ly + r, a.n1) * a.p1 + zc;
    const T *in = (const T *)a.in;
    T *out = (T *)a.out;
    auto plane_src = [&](int q) { return wrap(x0 - HALO + q, a.n0) * a.p0; };   // local plane q of level 0
    const int qlast = lx + 2 * HALO - 1;
    auto load_plane = [&](int q, V (&dst)[PY]) {
        const long po = plane_src(q < qlast ? q : qlast);      // (the prefetch behind the last plane repeats it)
#pragma unroll
        for (int r = 0; r < PY; r++) dst[r] = PDEHIP_LDV((const V *)(in + po + roff[r]));
    };

    // The patch number twice.  Every array is read twice per level, at offsets a constant apart; through the same index the compiler merges
    // the two into one two-address read, which runs at half the rate of two single 8-byte reads.  It cannot see through the empty asm.
    const int me = tid;
    int me2 = tid;
    asm volatile("" : "+v"(me2));
    if ((int)threadIdx.x < GUARD) lds[threadIdx.x] = lds[IMAGE - GUARD + threadIdx.x] = 0;   // (no result depends on it)
    // The two buffers of image l = 1, 2 as bases that alt_index / alt_read_index are added to: cur[l - 1] is read in this phase, oth[l - 1]
    // written; they change places after every phase (wave-uniform values: scalar moves, and one add per index register and phase).
    // Buffer 0 is the level's part of `lds`, buffer 1 lies in the dynamic array.
    LT *const alt = (LT *)euler4_alt;
    LT *cur[ALT_LEVELS] = {(LT *)lds + (image_index(1, 0, 0, 0) - alt_index(1, 0, 0, 0)), (LT *)lds + (image_index(2, 0, 0, 0) - alt_index(2, 0, 0, 0))};
    LT *oth[ALT_LEVELS] = {alt, alt};
    for (int k = (int)threadIdx.x; k < ALT_IMAGE; k += THREADS) alt[k] = 0;   // arrays and guard runs: a skipped level's cells stay zero

    auto update = [&](double xm, double xp, double up, double dn, double left, double right, double cen) {
        // (xm - 2 * cen) + xp and so on, as the reference rounds them
        const double dx = PDEHIP_E4_MINUS_TWICE(xm, cen) + xp, dy = PDEHIP_E4_MINUS_TWICE(up, cen) + dn, dz = PDEHIP_E4_MINUS_TWICE(left, cen) + right;
        if (M2 == E2_DIFFUSION_UNIT) return cen + a.s2 * (dx + dy + dz);   // all scales are exactly 1.0
        const double ex = dx * a.sx;
        const double ey = dy * a.sy;
        const double ez = dz * a.sz;
        return epilogue<LAP_EULER>(ex + ey + ez, cen, cen, a.s1, a.s2, a.gamma);
    };
    // the eight neighbour cells of the patch in the image of level l
    auto fetch = [&](int l, T (&nb)[READ_KINDS]) {
#pragma unroll
        for (int k = 0; k < READ_KINDS; k++) {
            const bool second = k == RD_BELOW1 || k == RD_LEFT1 || k == RD_RIGHT0 || k == RD_RIGHT1;   // the second read of its array
            nb[k] = lds[read_index(l, k, second ? me2 : me)];
        }
    };
    // one level up: the plane of `mid` at the next level, from the thread's cells of three planes and the neighbours of the middle one
    auto level = [&](const V (&old)[PY], const V (&mid)[PY], const V (&nw)[PY], const T (&nb)[READ_KINDS], V (&res)[PY]) {
        const V above = V{nb[RD_ABOVE0], nb[RD_ABOVE1]}, below = V{nb[RD_BELOW0], nb[RD_BELOW1]};
#pragma unroll
        for (int r = 0; r < PY; r++) {
            const double left = nb[RD_LEFT0 + r], right = nb[RD_RIGHT0 + r];
            const V up = r == 0 ? above : mid[r > 0 ? r - 1 : 0], dn = r == PY - 1 ? below : mid[r < PY - 1 ? r + 1 : r];
            res[r][0] = update(old[r][0], nw[r][0], up[0], dn[0], left, mid[r][1], mid[r][0]);
            res[r][1] = update(old[r][1], nw[r][1], up[1], dn[1], mid[r][0], right, mid[r][1]);
        }
    };
    auto store_level = [&](int l, const V (&pl)[PY]) {
#pragma unroll
        for (int r = 0; r < PY; r++) {
            lds[image_index(l, r, 0, me)] = pl[r][0];
            lds[image_index(l, r, 1, me)] = pl[r][1];
        }
    };

    // the same for images 1 and 2, in the buffer at `base` (cur or oth)
    auto fetch_alt = [&](int l, LT *base, T (&nb)[READ_KINDS]) {
        LT *const b = base + me, *const b2 = base + me2;
#pragma unroll
        for (int k = 0; k < READ_KINDS; k++) {
            const bool second = k == RD_BELOW1 || k == RD_LEFT1 || k == RD_RIGHT0 || k == RD_RIGHT1;
            nb[k] = (second ? b2 : b)[alt_read_index(l, k, 0)];
        }
    };
    auto store_alt = [&](int l, LT *base, const V (&pl)[PY]) {
        LT *const b = base + me;
#pragma unroll
        for (int r = 0; r < PY; r++) {
            b[alt_index(l, r, 0, 0)] = pl[r][0];
            b[alt_index(l, r, 1, 0)] = pl[r][1];
        }
    };

    // R[L][s]: level L, plane slot s; slot of local plane j = j mod 3
    V R[LEVELS][3][PY], pre[PY];
#pragma unroll
    for (int l = 0; l < LEVELS; l++)
#pragma unroll
        for (int s = 0; s < 3; s++)
#pragma unroll
            for (int r = 0; r < PY; r++) R[l][s][r] = V{0, 0};
    load_plane(0, R[0][0]);
    load_plane(1, R[0][1]);
    load_plane(2, R[0][2]);
#pragma unroll
    for (int l = 0; l < LEVELS; l++) store_level(l, R[l][(4 - l) % 3]);   // the middle planes of iteration 0 (level 0: plane 1; the others: zeros)
    __syncthreads();

    // iteration i, i mod 3 == K: level 0 holds planes i, i + 1, i + 2 in slots K, K + 1, K + 2 (mod 3); level L the planes L lower.
    // The order of the LDS traffic and the two barriers is e4plan::SCHEDULE.
    auto phase = [&](int i, auto kc) {
        constexpr int K = decltype(kc)::value;
        load_plane(i + 3, pre);   // needed at the next iteration
        // level 3's middle plane of THIS iteration, computed by l = 2 of the one before (iteration 0: the prologue's zeros once more)
        if (LEVELS - 1 <= nlev) store_level(LEVELS - 1, R[LEVELS - 1][(K + 1) % 3]);
#pragma unroll
        for (int l = 0; l < LEVELS; l++) {
            // level l holds planes (i - l, i + 1 - l, i + 2 - l); level l + 1 gets plane i + 1 - l, in the slot of its plane i - 2 - l
            const V (&old)[PY] = R[l][(K + 3 - l) % 3];
            const V (&mid)[PY] = R[l][(K + 4 - l) % 3];
            const V (&nw)[PY] = R[l][(K + 5 - l) % 3];
            if (l == 0 || l < nlev) {   // level l + 1 is one of the wave's (every wave executes level 1)
                T nb[READ_KINDS];
                if (l == 0 || l == LEVELS - 1) fetch(l, nb);
                else fetch_alt(l, cur[l - 1], nb);
                if (l < LEVELS - 1) {
                    V (&res)[PY] = R[l + 1][(K + 4 - l) % 3];
                    level(old, mid, nw, nb, res);
                    // the middle plane of level l + 1 at the next iteration, into the buffer nobody reads in this phase (level 3: kept in
                    // its registers until barrier B has passed)
                    if (l + 1 < LEVELS - 1) store_alt(l + 1, oth[l], res);
                } else {                // (owner waves only: nlev == LEVELS)
                    V res[PY];
                    level(old, mid, nw, nb, res);
                    const int q = i - 2;   // the local plane of level 4: output plane x0 + q - HALO
                    if (owner && q >= HALO) {
                        const long po = (x0 + q - HALO) * a.p0;
#pragma unroll
                        for (int r = 0; r < PY; r++) __builtin_nontemporal_store(res[r], (V *)(out + po + roff[r]));
                    }
                }
            }
            if (l == 0) {
                __syncthreads();        // A: every wave has read the image of level 0 ...
                store_level(0, nw);     // ... plane i + 2 takes its place
            }
        }
        __syncthreads();                // B: every wave has read the image of level 3 (and the buffers `cur` of levels 1 and 2)
#pragma unroll
        for (int r = 0; r < PY; r++) R[0][K][r] = pre[r];   // plane i is dead: plane i + 3 takes its slot
#pragma unroll
        for (int b = 0; b < ALT_LEVELS; b++) {
            LT *const t = cur[b];
            cur[b] = oth[b];
            oth[b] = t;
        }
    };
    const int iend = lx + 2 * HALO - 3;   // the last iteration: level 4 at plane lx + HALO - 1
    for (int i = 0;; i += 3) {
        phase(i, std::integral_constant<int, 0>());
        if (i + 1 > iend) break;
        phase(i + 1, std::integral_constant<int, 1>());
        if (i + 2 > iend) break;
        phase(i + 2, std::integral_constant<int, 2>());
        if (i + 3 > iend) break;
    }
}
