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
// The loop is unrolled six times so that the rotation of the plane buffers (over three phases, like euler2_body) and the change of the
// image buffers (over two, below) are both a renaming.  What the first iterations
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
// The stores of levels 1 and 2 are issued where their data is produced and nothing waits for them but the next barrier.  The parity is a
// compile-time constant of the unrolled loop, so every access of either buffer is a lane's index register plus an immediate.  The prologue
// stores the middle planes of iteration 0 (parity 0) into the buffers 0 and zeroes the second buffers with their guard runs, behind one barrier.
//
// A phase executes fp64 arithmetic, LDS and memory instructions and next to nothing else per lane (profiles/euler4_phase_diet_time.md: about
// 17 integer and move instructions per wave and phase became about one):
//   * a plane's base - input and output - is a wave-uniform pointer formed once per phase in scalar registers, and a row of a lane's patch
//     is a loop-invariant 32-bit byte offset inside the plane (e4plan::offsets_fit; the launcher declines an array whose planes are larger):
//     the loads and the non-temporal stores take the scalar base, and no lane adds 64-bit addresses;
//   * the plane that is loaded goes straight into the slot of the plane that dies - what level 0 still needs of that one, old - 2 * mid, is
//     taken first - so three register sets rotate through the unrolled phases and nothing is moved;
//   * the loop has one exit: whole rounds of six phases, then the (at most five) phases left over.  Several exits shared a block that
//     moved the live planes into common registers once per round.
//
// Waves have roles (e4plan::lane_patch, wave_levels; the lane -> patch map is not the row-major numbering of the image).  A patch is needed at
// as many levels as its distance from the rim of the region allows - an output patch at all four, the ring around the outputs at levels
// 1 ... 3, the outer ring at level 1 - and the map gathers the output patches in waves 0 ... 7, the halo patches in waves 8 ... 11, so that a
// halo wave skips, by scalar branches, the levels none of its patches is needed at: the neighbour reads, the arithmetic and the image stores
// of those levels (level 0's image stores and the plane loads stay), 42 wave-levels per phase instead of 48 and at most 11 instead of 12 on
// a SIMD.  Only the owner waves store to the field.  Every wave executes every barrier of every phase - the skips enclose no barrier - and
// the trip count depends on the workgroup alone.  The cells of a skipped level keep the zeros of the prologue in the image; they are read
// only by cells that are invalid at their own level, like the unspecified values above (tests/test_euler4_lanes.py enumerates it by lane
// and by role: whatever a valid cell reads was stored by a wave that executes that level).  The same holds lane by lane: inside the halo
// waves 8 ... 10 a level runs only in the lanes whose patch is needed at it (e4plan::lane_levels, `lanes` below), the cells of a masked lane
// keep the prologue's zeros too, and tests/test_euler4_lane_levels.py enumerates that a valid cell reads none of them.  The results are the
// same bits as before.
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

    // Addresses: a plane's base is a wave-uniform pointer (a scalar register pair, formed once per phase), a row of the patch a loop-invariant
    // 32-bit byte offset of the lane inside the plane (e4plan::offsets_fit, asked by the launcher): loads and stores take the scalar base
    // with a 32-bit lane offset, and no lane adds 64-bit addresses in the loop.
    unsigned roff[PY];   // byte offset of the patch's rows in a plane
    const long zc = wrap(tz * TZ - HALO + lz, a.n2);           // even: a patch never straddles the wrap
#pragma unroll
    for (int r = 0; r < PY; r++) roff[r] = (unsigned)((a.off + wrap(ty * TY - HALO + ly + r, a.n1) * a.p1 + zc) * (long)sizeof(T));
    unsigned soff[PY];   // the same offsets once more, for the field stores (a copy that the stores' own block can pin)
#pragma unroll
    for (int r = 0; r < PY; r++) soff[r] = roff[r];
    const char *in = (const char *)a.in;
    char *out = (char *)a.out;
    // local plane q of level 0, in bytes (the plane number in 32 bits, which the launcher asks for: a scalar compare, where 64 bits take a vector one)
    const int x0i = (int)x0, n0i = (int)a.n0;
    auto plane_src = [&](int q) {
        const int x = x0i - HALO + q;
        return (long)(x < 0 ? x + n0i : (x >= n0i ? x - n0i : x)) * a.p0 * (long)sizeof(T);
    };
    const int qlast = lx + 2 * HALO - 1;
    auto load_plane = [&](int q, V (&dst)[PY]) {
        const char *const base = in + plane_src(q < qlast ? q : qlast);      // (the prefetch behind the last plane repeats it)
#pragma unroll
        for (int r = 0; r < PY; r++) dst[r] = PDEHIP_LDV((const V *)(base + roff[r]));
    };

    // The patch number twice.  Every array is read twice per level, at offsets a constant apart; through the same index the compiler merges
    // the two into one two-address read, which runs at half the rate of two single 8-byte reads.  It cannot see through the empty asm.
    const int me = tid;
    int me2 = tid;
    asm volatile("" : "+v"(me2));
    if ((int)threadIdx.x < GUARD) lds[threadIdx.x] = lds[IMAGE - GUARD + threadIdx.x] = 0;   // (no result depends on it)
    // The two buffers of image l = 1, 2: buffer 0 is the level's part of `lds` (image_index, read_index), buffer 1 lies in the dynamic array
    // (alt_index, alt_read_index).  Which of the two a phase reads is its parity, a compile-time constant of the unrolled loop: every access
    // is an index register plus an immediate.
    LT *const alt = (LT *)euler4_alt;
    for (int k = (int)threadIdx.x; k < ALT_IMAGE; k += THREADS) alt[k] = 0;   // arrays and guard runs: a skipped level's cells stay zero

    auto update = [&](double dxm, double xp, double up, double dn, double left, double right, double cen) {
        // (xm - 2 * cen) + xp and so on, as the reference rounds them; dxm = xm - 2 * cen comes from the caller
        const double dx = dxm + xp, dy = PDEHIP_E4_MINUS_TWICE(up, cen) + dn, dz = PDEHIP_E4_MINUS_TWICE(left, cen) + right;
        if (M2 == E2_DIFFUSION_UNIT) return cen + a.s2 * (dx + dy + dz);   // all scales are exactly 1.0
        const double ex = dx * a.sx;
        const double ey = dy * a.sy;
        const double ez = dz * a.sz;
        return epilogue<LAP_EULER>(ex + ey + ez, cen, cen, a.s1, a.s2, a.gamma);
    };
    // old - 2 * mid: all that a level needs of its oldest plane
    auto minus_twice = [&](const V (&old)[PY], const V (&mid)[PY], V (&d)[PY]) {
#pragma unroll
        for (int r = 0; r < PY; r++) d[r] = V{PDEHIP_E4_MINUS_TWICE(old[r][0], mid[r][0]), PDEHIP_E4_MINUS_TWICE(old[r][1], mid[r][1])};
    };
    // the eight neighbour cells of the patch in the image of level l, buffer `buf` (1: images 1 and 2 only)
    auto fetch = [&](int l, int buf, T (&nb)[READ_KINDS]) {
#pragma unroll
        for (int k = 0; k < READ_KINDS; k++) {
            const bool second = k == RD_BELOW1 || k == RD_LEFT1 || k == RD_RIGHT0 || k == RD_RIGHT1;   // the second read of its array
            nb[k] = buf ? alt[alt_read_index(l, k, second ? me2 : me)] : lds[read_index(l, k, second ? me2 : me)];
        }
    };
    // one level up: the plane of `mid` at the next level, from the thread's cells of three planes (the oldest as d = old - 2 * mid) and the
    // neighbours of the middle one
    auto level = [&](const V (&d)[PY], const V (&mid)[PY], const V (&nw)[PY], const T (&nb)[READ_KINDS], V (&res)[PY]) {
        const V above = V{nb[RD_ABOVE0], nb[RD_ABOVE1]}, below = V{nb[RD_BELOW0], nb[RD_BELOW1]};
#pragma unroll
        for (int r = 0; r < PY; r++) {
            const double left = nb[RD_LEFT0 + r], right = nb[RD_RIGHT0 + r];
            const V up = r == 0 ? above : mid[r > 0 ? r - 1 : 0], dn = r == PY - 1 ? below : mid[r < PY - 1 ? r + 1 : r];
            res[r][0] = update(d[r][0], nw[r][0], up[0], dn[0], left, mid[r][1], mid[r][0]);
            res[r][1] = update(d[r][1], nw[r][1], up[1], dn[1], mid[r][0], right, mid[r][1]);
        }
    };
    auto store_level = [&](int l, int buf, const V (&pl)[PY]) {
#pragma unroll
        for (int r = 0; r < PY; r++) {
            if (buf) {
                alt[alt_index(l, r, 0, me)] = pl[r][0];
                alt[alt_index(l, r, 1, me)] = pl[r][1];
            } else {
                lds[image_index(l, r, 0, me)] = pl[r][0];
                lds[image_index(l, r, 1, me)] = pl[r][1];
            }
        }
    };

    // R[L][s]: level L, plane slot s; slot of local plane j = j mod 3
    V R[LEVELS][3][PY];
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
    for (int l = 0; l < LEVELS; l++) store_level(l, 0, R[l][(4 - l) % 3]);   // the middle planes of iteration 0 (level 0: plane 1; the others: zeros)
    __syncthreads();

    // iteration i, i mod 3 == K, i mod 2 == P: level 0 holds planes i, i + 1, i + 2 in slots K, K + 1, K + 2 (mod 3); level L the planes L
    // lower; images 1 and 2 are read in their buffers P and written in their buffers 1 - P.  The order of the LDS traffic and the two
    // barriers is e4plan::SCHEDULE.  A phase executes fp64 arithmetic, LDS and memory instructions and nothing per lane besides: the plane
    // that is loaded goes straight into the slot of the plane that dies (what level 0 still needs of that one, old - 2 * mid, is taken
    // first), so the rotation of the slots is a renaming over three phases, the parity one over two, and the loop is unrolled six times.
    //
    // Dead lanes masked.  Inside the halo waves 8 ... 10 a lane's patch is not needed at every level its wave executes (e4plan::lane_levels:
    // the ring-0 lanes of wave 8 and of waves 9 and 10 at levels 2 and 3; the spare lanes of waves 9 and 10, which repeat patches of the other
    // wave, at every level): 232 of the 2688 lane-levels of a phase.  In those waves the work of level `level` - neighbour reads, arithmetic,
    // image stores; for the repeated patches level 0's image stores too - runs in the lanes that need it alone; in the owner waves and in
    // wave 11 the condition is true in every lane.  The compiler folds the two cases into one lane mask per level, loop-invariant and held
    // in scalar registers, so a section costs every wave three scalar instructions and no vector one.  The plane loads stay outside: every
    // lane loads (a load inside a branch makes the wait for the plane loaded a phase ago drain the one just issued).  No barrier stands
    // inside a section.
    const int mylevels = lane_levels((int)threadIdx.x);
    const bool masked = wave >= OWNER_WAVES && wave < WAVES - 1;
    auto lanes = [&](int level, auto work) {
        if (masked) {
            if (level <= mylevels) work();
        } else
            work();
    };
    auto phase = [&](int i, auto kc, auto pc) {
        constexpr int K = decltype(kc)::value, P = decltype(pc)::value;
        // (The offsets pass through an empty asm once per phase.  Without it their zero-extension is hoisted out of the loop, a register
        // pair per row, and every load and store adds 64 bits per lane again instead of taking the scalar base.)
#pragma unroll
        for (int r = 0; r < PY; r++) asm volatile("" : "+v"(roff[r]));
        V d0[PY];
        minus_twice(R[0][K], R[0][(K + 1) % 3], d0);
        load_plane(i + 3, R[0][K]);   // plane i is dead: plane i + 3, needed at the next iteration, takes its slot
        // level 3's middle plane of THIS iteration, computed by l = 2 of the one before (iteration 0: the prologue's zeros once more)
        if (LEVELS - 1 <= nlev) lanes(LEVELS - 1, [&] { store_level(LEVELS - 1, 0, R[LEVELS - 1][(K + 1) % 3]); });
#pragma unroll
        for (int l = 0; l < LEVELS; l++) {
            // level l holds planes (i - l, i + 1 - l, i + 2 - l); level l + 1 gets plane i + 1 - l, in the slot of its plane i - 2 - l
            const V (&old)[PY] = R[l][(K + 3 - l) % 3];
            const V (&mid)[PY] = R[l][(K + 4 - l) % 3];
            const V (&nw)[PY] = R[l][(K + 5 - l) % 3];
            auto up = [&] {
                T nb[READ_KINDS];
                fetch(l, (l == 0 || l == LEVELS - 1) ? 0 : P, nb);
                V d[PY];
                if (l > 0) minus_twice(old, mid, d);
                if (l < LEVELS - 1) {
                    V (&res)[PY] = R[l + 1][(K + 4 - l) % 3];
                    level(l == 0 ? d0 : d, mid, nw, nb, res);
                    // the middle plane of level l + 1 at the next iteration, into the buffer nobody reads in this phase (level 3: kept in
                    // its registers until barrier B has passed)
                    if (l + 1 < LEVELS - 1) store_level(l + 1, 1 - P, res);
                } else {                // (owner waves only: nlev == LEVELS)
                    V res[PY];
                    level(d, mid, nw, nb, res);
                    const int q = i - 2;   // the local plane of level 4: output plane x0 + q - HALO
                    if (owner && q >= HALO) {
                        char *const base = out + (x0 + q - HALO) * a.p0 * (long)sizeof(T);   // wave-uniform
#pragma unroll
                        for (int r = 0; r < PY; r++) {
                            asm volatile("" : "+v"(soff[r]));   // (as above, in the block of the stores)
                            __builtin_nontemporal_store(res[r], (V *)(base + soff[r]));
                        }
                    }
                }
            };
            if (l == LEVELS - 1) {
                if (l < nlev) up();     // (owner waves only: no lane of theirs is masked)
            } else if (l == 0 || l < nlev)
                lanes(l + 1, up);       // level l + 1 is one of the wave's (every wave executes level 1)
            if (l == 0) {
                __syncthreads();        // A: every wave has read the image of level 0 ...
                lanes(1, [&] { store_level(0, 0, nw); });   // ... plane i + 2 takes its place
            }
        }
        __syncthreads();                // B: every wave has read the image of level 3 (and the buffers P of levels 1 and 2)
    };
    // One exit: whole rounds of six phases, then the phases left over (at most five), which go on where a round would.  The trip counts
    // depend on the workgroup alone.
    const int nphases = lx + 2 * HALO - 2;   // the last iteration computes level 4 at plane lx + HALO - 1
    typedef std::integral_constant<int, 0> C0;
    typedef std::integral_constant<int, 1> C1;
    typedef std::integral_constant<int, 2> C2;
    int i = 0;
    for (; i + 6 <= nphases; i += 6) {
        phase(i, C0(), C0());
        phase(i + 1, C1(), C1());
        phase(i + 2, C2(), C0());
        phase(i + 3, C0(), C1());
        phase(i + 4, C1(), C0());
        phase(i + 5, C2(), C1());
    }
    const int left = nphases - i;
    if (left > 0) {
        phase(i, C0(), C0());
        if (left > 1) {
            phase(i + 1, C1(), C1());
            if (left > 2) {
                phase(i + 2, C2(), C0());
                if (left > 3) {
                    phase(i + 3, C0(), C1());
                    if (left > 4) phase(i + 4, C1(), C0());
                }
            }
        }
    }
}
