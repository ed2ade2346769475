// pdehip_euler4_plan.h - whether a four-step sweep (pdehip_march4.inc: four Euler steps per launch, the time levels exchange their current
// plane through LDS) runs, and with which x-chunks.  Plain host C++17 without a HIP header, like pdehip_euler2_plan.h: the launcher
// (pdehip_kernels_e4.hip) asks plan() and launches what it answers, a CPU probe (tests/shim/euler4_plan_probe.cpp) asks the same function.
#pragma once

#include <cstdio>
#include <cstdlib>

namespace pdehip {
namespace e4plan {

// The tile.  A workgroup owns TY x TZ outputs (rows x fastest axis) and reads (TY + 8) x (TZ + 8) cells of every input plane; a thread owns
// a patch of PY rows x 2 cells at every level.  Work of the four levels on the shrinking regions: (38*70 + 36*68 + 34*66 + 32*64) / (4 * 32*64)
// = 1.15 x.  (40 / PY) * (72 / 2) = 720 patches: 768 threads, 48 of which repeat halo patches (lane_patch).
constexpr int TY = 32, TZ = 64, PY = 2, LEVELS = 4, HALO = 4;
constexpr int RY = TY + 2 * HALO, RZ = TZ + 2 * HALO;           // the region of level 0
constexpr int NPY = RY / PY, NPZ = RZ / 2, PATCHES = NPY * NPZ;
constexpr int THREADS = (PATCHES + 63) / 64 * 64;
// the LDS allocation: LEVELS * LROWS * LPITCH doubles (what a row-major picture of each level with a ring around it took; the size is kept)
constexpr int LROWS = RY + 2, LPITCH = RZ + 4;
constexpr long LDS_BYTES = (long)LEVELS * LROWS * LPITCH * 8;
// The image inside that allocation: one array of ARR doubles per level, patch row and patch cell, indexed by the patch number, so that a
// wave's 64 lanes touch 64 consecutive doubles in every access; GUARD doubles in front of the first and behind the last array.
constexpr int ARR = PATCHES, NARR = LEVELS * PY * 2, GUARD = NPZ;
constexpr int IMAGE = GUARD + NARR * ARR + GUARD;
static_assert(PY == 2 && IMAGE <= LEVELS * LROWS * LPITCH, "the image of the four-step sweep fits its LDS allocation");

// The row-major numbering of the patches, which is the numbering of the IMAGE (image_index, read_index: patch = py * NPZ + pz), padded to
// THREADS entries: the THREADS - PATCHES entries behind the last patch repeat the patch 64 lower - a halo patch - so that 64 consecutive
// entries still touch 64 different consecutive doubles modulo 64.  It was the kernel's lane assignment (thread = patch) and no longer is:
// the kernel takes a lane's patch from lane_patch below.  tests/test_euler4_image.py enumerates the image through this numbering.
constexpr int patch_of_thread(int t) { return t < PATCHES ? t : t - 64; }
static_assert(PATCHES >= 64 && (PATCHES - 64) / NPZ * PY >= HALO + TY, "repeated patches are halo patches");

// The kernel's lane assignment: which patch lane t of the workgroup holds, by the role of its wave.  A patch is needed at as many levels as
// its distance from the rim of the region allows: the 16 x 32 = 512 output patches at all four, the 100 patches of the ring around them
// (py = 1, 18 or pz = 1, 34: "ring 1") at levels 1 ... 3, the 108 patches of the outer ring (py = 0, 19 or pz = 0, 35: "ring 0") at level 1
// alone; 2048 + 300 + 108 = 2456 patch-levels where thread = patch computed 768 * 4 = 3072.  So that whole waves can skip what is not needed:
//   waves 0 ... 7   the output patches; wave k holds the patch rows 2 + 2k (lanes 0 ... 31: pz = 2 ... 33) and 3 + 2k (lanes 32 ... 63).
//                   Four levels, and the only waves that store to the field: 512 contiguous bytes per half-wave and row.
//   wave 8          the four rim columns pz = 0, 1, 34, 35 of the patch rows 2 ... 17, four lanes per row: 32 patches of ring 1, 32 of ring 0.
//   wave 9          patches 32 ... 71: the end of patch row 0 (pz = 32 ... 35) and patch row 1; 40 lanes.
//   wave 10         patches 648 ... 687: patch row 18 and the beginning of patch row 19 (pz = 0 ... 3); 40 lanes.
//                   Waves 8 ... 10 execute levels 1 ... 3.  The other 24 lanes of waves 9 and 10 repeat patches of the OTHER wave of the two
//                   (the same values to the same cells of the image twice), chosen by their residues - see below.
//   wave 11         patches 0 ... 31 and 688 ... 719, the rest of ring 0: level 1 only.
// Waves w, w + 4, w + 8 share a SIMD: three SIMDs execute 4 + 4 + 3 = 11 wave-levels per phase and one 4 + 4 + 1 = 9, 42 instead of 48.
// Bank conflicts: every access of a lane is base + its patch number, so an 8-byte read (two groups of 32 lanes on 64 banks) is conflict-free
// when the patches of a half-wave differ modulo 32, and an 8-byte store (four groups of 16 lanes on 32 banks) when those of a quarter-wave
// differ modulo 16.  Runs of consecutive patches do; NPZ = 36 = 4 (mod 32), so the four rim columns of patch row py have the residues
// 4 py + 0 ... 3, and eight / four consecutive rows fill a half / quarter of wave 8 exactly; the repeated patches of waves 9 and 10 are runs
// that complete the residues of their half: 64 ... 71 | 648 ... 671 are 0 ... 7 | 8 ... 31 (mod 32), 680 ... 687 | 64 ... 71 | 48 ... 63 are
// 8 ... 15 | 0 ... 7 | 16 ... 31.  tests/test_euler4_lanes.py enumerates all of this.
constexpr int WAVES = THREADS / 64, OWNER_WAVES = 8;
constexpr int wave_levels(int w) { return w < OWNER_WAVES ? LEVELS : w < WAVES - 1 ? LEVELS - 1 : 1; }   // levels 1 ... wave_levels(w) are executed
constexpr int lane_patch(int t)
{
    const int w = t >> 6, lane = t & 63;
    if (w < OWNER_WAVES) return (HALO / PY + 2 * w + (lane >> 5)) * NPZ + HALO / 2 + (lane & 31);
    if (w == 8) return (HALO / PY + (lane >> 2)) * NPZ + ((lane & 2) ? NPZ - 4 : 0) + (lane & 3);   // pz = 0, 1, 34, 35
    if (w == 9) return lane < 40 ? 32 + lane : 648 + (lane - 40);
    if (w == 10) return lane < 40 ? 648 + lane : lane < 48 ? 64 + (lane - 40) : lane;
    return lane < 32 ? lane : PATCHES - 64 + lane;
}
static_assert(TY == 32 && TZ == 64 && PY == 2 && HALO == 4 && WAVES == 12, "lane_patch is written for this tile");
static_assert(OWNER_WAVES * 64 == (TY / PY) * (TZ / 2), "the output patches fill the owner waves exactly");

// The highest level lane t's patch is needed at - 4 for an output patch, 3 for a patch of ring 1, 1 for a patch of ring 0 (a patch k patches
// from the rim holds the cells 2k and 2k + 1 from the rim, and a cell c from the rim is valid up to level c) - and 0 for the second copy of a
// repeated patch, the one in the spare lanes 40 ... 63 of waves 9 and 10: the other copy does its work.  Inside waves 8 ... 10 the kernel
// runs level l + 1 of a phase in the lanes with l < lane_levels(t) only (tests/test_euler4_lane_levels.py enumerates what that leaves).
constexpr int lane_levels(int t)
{
    const int w = t >> 6, lane = t & 63;
    if ((w == 9 || w == 10) && lane >= 40) return 0;
    const int p = lane_patch(t), py = p / NPZ, pz = p - py * NPZ;
    const int dy = py < NPY - 1 - py ? py : NPY - 1 - py, dz = pz < NPZ - 1 - pz ? pz : NPZ - 1 - pz;
    const int ring = dy < dz ? dy : dz;
    return 2 * ring + 1 < LEVELS ? 2 * ring + 1 : LEVELS;
}

// index (in doubles) of cell `cell` (0, 1) of row `row` (0 ... PY - 1) of patch `patch` at level `level` (0 ... LEVELS - 1)
constexpr int image_index(int level, int row, int cell, int patch) { return GUARD + ((level * PY + row) * 2 + cell) * ARR + patch; }

// The eight cells of a level that a patch reads from the image - the others are its own registers - as constant offsets of its own number:
// the row above is the last row of the patch NPZ lower, the row below the first row of the patch NPZ higher, the left neighbour cell 1 of
// the patch before, the right neighbour cell 0 of the patch behind.  At the rim of the region such an index lies in the neighbouring array
// or in a guard run; pdehip_march4.inc says why that is harmless and tests/test_euler4_image.py enumerates it.
enum ReadKind { RD_ABOVE0, RD_ABOVE1, RD_BELOW0, RD_BELOW1, RD_LEFT0, RD_LEFT1, RD_RIGHT0, RD_RIGHT1, READ_KINDS };
constexpr int read_index(int level, int kind, int patch)
{
    return kind < RD_BELOW0  ? image_index(level, PY - 1, kind - RD_ABOVE0, patch - NPZ)
         : kind < RD_LEFT0   ? image_index(level, 0, kind - RD_BELOW0, patch + NPZ)
         : kind < RD_RIGHT0  ? image_index(level, kind - RD_LEFT0, 1, patch - 1)
                             : image_index(level, kind - RD_RIGHT0, 0, patch + 1);
}

// The second buffers of the images of levels 1 and 2 (two barriers per phase: pdehip_march4.inc).  Each has the shape of a level of the
// image - a guard run, PY * 2 arrays indexed by the patch number, a guard run - and the two lie one behind the other in an allocation of
// their own, the kernel's dynamic LDS (ALT_BYTES at the launch); the four images above stay in the static allocation.  alt_index and
// alt_read_index are image_index and read_index with another base: every access of a lane is again a base plus its patch number, so the
// residue rule of lane_patch carries over, and a neighbour is the same constant offset of the patch number.  Levels 1 and 2 only.
constexpr int ALT_LEVELS = 2, ALT_LEVEL = GUARD + PY * 2 * ARR + GUARD;    // buffers; doubles per buffer
constexpr int ALT_IMAGE = ALT_LEVELS * ALT_LEVEL;
constexpr long ALT_BYTES = (long)ALT_IMAGE * 8;
constexpr int alt_index(int level, int row, int cell, int patch) { return (level - 1) * ALT_LEVEL + GUARD + (row * 2 + cell) * ARR + patch; }
constexpr int alt_read_index(int level, int kind, int patch)
{
    return kind < RD_BELOW0  ? alt_index(level, PY - 1, kind - RD_ABOVE0, patch - NPZ)
         : kind < RD_LEFT0   ? alt_index(level, 0, kind - RD_BELOW0, patch + NPZ)
         : kind < RD_RIGHT0  ? alt_index(level, kind - RD_LEFT0, 1, patch - 1)
                             : alt_index(level, kind - RD_RIGHT0, 0, patch + 1);
}
static_assert(LDS_BYTES % 16 == 0 && ALT_BYTES % 16 == 0 && LDS_BYTES + ALT_BYTES <= 160 * 1024, "static and dynamic LDS of the four-step sweep");

// The order of a phase of pdehip_march4.inc, which the kernel follows and tests/test_euler4_double_buffer.py replays: what a wave does to
// which image between which barriers.  `other`: 0 = the buffer of the phase's parity p (images 0 and 3 have one buffer: always 0),
// 1 = the buffer 1 - p.  `interval`: 0 = between barrier B of the phase before (the prologue's barrier) and A, 1 = between A and B.
// Waves run freely inside an interval, so a store and a read of one buffer are ordered if and only if they lie in different intervals.
enum SchedOp { SCH_STORE, SCH_READ, SCH_BARRIER };
struct SchedEvent { int op, image, other, interval; };
constexpr SchedEvent SCHEDULE[] = {
    {SCH_STORE, 3, 0, 0},     // level 3's middle plane of this phase, computed in the phase before
    {SCH_READ, 0, 0, 0},      // l = 0: level 1 ...
    {SCH_STORE, 1, 1, 0},     // ... into the other buffer of image 1
    {SCH_BARRIER, -1, 0, 0},  // A: every wave has read image 0
    {SCH_STORE, 0, 0, 1},     // plane i + 2
    {SCH_READ, 1, 0, 1},      // l = 1: level 2 ...
    {SCH_STORE, 2, 1, 1},     // ... into the other buffer of image 2
    {SCH_READ, 2, 0, 1},      // l = 2: level 3, kept in registers
    {SCH_READ, 3, 0, 1},      // l = 3: level 4, to the field
    {SCH_BARRIER, -1, 0, 1},  // B: every wave has read image 3
};
constexpr int SCHEDULE_EVENTS = sizeof(SCHEDULE) / sizeof(SCHEDULE[0]);

// x - 2 * c in ONE instruction.  The reference computes vm = 2 * c and then x - vm (cartesian.py:220-227): two roundings on paper, but doubling
// is exact, so x - vm is the real number x - 2c rounded once - which is what the fused multiply-add returns.  Bit for bit the same for all
// finite c up to half the largest double (beyond it 2 * c overflows to infinity and the fused form does not; tests/test_euler4_fma.py walks
// zeros of both signs, subnormals, cancellations and the largest magnitudes through a CPU probe).  Three of these per cell replace one
// doubling and three subtractions: 10 instead of 11 fp64 instructions per cell and level in the kernel of pdehip_march4.inc.  (A macro: the
// one form of an expression that the kernel and the host probe can share from a header without HIP qualifiers.)
#define PDEHIP_E4_MINUS_TWICE(x, c) __builtin_fma(-2.0, (c), (x))

// The kernel addresses a cell as a plane's base (a wave-uniform pointer) plus the lane's byte offset inside the plane, an unsigned 32-bit
// register: 8 * (off + row * p1 + column) with row * p1 + column < p0 (`off`: the first valid cell of the array, `p0`: the plane pitch, both
// in doubles).  True when every such offset is below 2^32; the launcher declines otherwise.
constexpr bool offsets_fit(long off, long p0) { return off >= 0 && p0 > 0 && off <= (1L << 29) && p0 <= (1L << 29) - off; }

constexpr long MIN_CHUNK = 8;      // the fewest output planes of an x-chunk (each chunk recomputes 2 * HALO planes more)
constexpr long WANT_CHUNK = 16;     // chunks are not made shorter than this to fill the chip
constexpr long CUS = 256;           // one workgroup per CU (LDS)
static_assert(RY % PY == 0 && HALO % PY == 0 && TZ % 2 == 0 && THREADS <= 1024 && LDS_BYTES <= 160 * 1024, "tile of the four-step sweep");

// PDEHIP_EULER4, read at every call: 0 = off, 1 = on wherever an instance exists, unset = the default gate (-1)
inline int knob_from_env()
{
    const char *e = getenv("PDEHIP_EULER4");
    if (!e || !e[0]) return -1;
    return e[0] == '0' ? 0 : 1;
}

struct Query {
    int elem;             // 8: fp64
    int ndim;
    long n0, n1, n2;      // march axis, rows, fastest axis
    int per[3];           // 1: periodic
    bool diffusion;       // the diffusion right-hand side ...
    bool const_faces;     // ... with constant conditions: no program of conditions, no faces given as arrays
    bool unit;            // unit spacing and D = 1
    int knob;             // knob_from_env()
};

struct Choice {
    bool accepted = false;
    bool unit = false;
    long nty = 0, ntz = 0, nxc = 0, nblocks = 0;
    int lx = 0;           // output planes per x-chunk (the last chunk may be shorter)
    unsigned block = THREADS;
};

// By default only fields beyond three times the 256 MB Infinity Cache.  Measured at 512^3 = 1 GiB: 0.136 against 0.192 ms per step
// (profiles/euler4_time.md).  The 400 MiB that select the tall two-step tile would also admit 256 x 512 x 512 (512 MiB), a share whose two-step
// instance tests/test_hip_share_sizes.py pins and which was not measured: the gate is narrower instead.  (Forced, the path also wins at 256^3,
// same file (d): lowering the threshold is a change of its own.)
constexpr double DEFAULT_MIN_BYTES = 768.0 * 1048576.0;

inline Choice plan(const Query &q)
{
    Choice c;
    if (q.knob == 0 || !q.diffusion || !q.const_faces) return c;
    if (q.elem != 8 || q.ndim != 3 || q.per[0] != 1 || q.per[1] != 1 || q.per[2] != 1) return c;
    if (q.n1 < TY || q.n1 % TY || q.n2 < TZ || q.n2 % TZ || q.n0 < 2 * HALO + MIN_CHUNK) return c;
    if (q.knob < 0 && (double)q.n0 * (double)q.n1 * (double)q.n2 * 8.0 <= DEFAULT_MIN_BYTES) return c;
    c.nty = q.n1 / TY; c.ntz = q.n2 / TZ;
    const long tiles = c.nty * c.ntz;
    // x-chunks: whole rounds of one workgroup per CU where the tiles allow it (512^3: 128 tiles x 2 chunks), chunks of WANT_CHUNK planes at least
    long nxc = (CUS + tiles - 1) / tiles;
    if (nxc > q.n0 / WANT_CHUNK) nxc = q.n0 / WANT_CHUNK;
    if (nxc < 1) nxc = 1;
    const long lx = (q.n0 + nxc - 1) / nxc;
    c.lx = (int)lx;
    c.nxc = (q.n0 + lx - 1) / lx;
    c.nblocks = c.nxc * tiles;
    c.unit = q.unit;
    c.accepted = true;
    return c;
}

inline void format_name(const Choice &c, char *buf, size_t size)
{
    snprintf(buf, size, "euler4_kernel<double,%s> (%dx%d tile, 4 levels in LDS, all-periodic)", c.unit ? "E2_DIFFUSION_UNIT" : "E2_DIFFUSION", TY, TZ);
}

}  // namespace e4plan
}  // namespace pdehip
