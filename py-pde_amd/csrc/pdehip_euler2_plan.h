// pdehip_euler2_plan.h - what a two-step sweep (pdehip_march2.inc) runs: which instance, which tile, open rows / open tile columns, the
// x-chunk count, the wave cap, streaming or plain stores, the workgroup shape.  Plain host C++17 without a HIP header: the launcher
// (pdehip_kernels_e2.hip) asks plan() and launches what it answers, a CPU test (tests/test_euler2_plan.py) asks the same function.
// Outside the exactv / fastv namespaces: one copy.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace pdehip {
namespace e2plan {

// the two fused levels: the values of E2_* (pdehip_device.h is device code; pdehip_kernels_e2.hip asserts that the two agree)
enum { M2_DIFFUSION = 0, M2_CH_EULER = 1, M2_CH_SCALED = 2, M2_CUSTOM = 3, M2_CUSTOM2 = 4, M2_CH_STAGE = 5, M2_DIFFUSION_UNIT = 6 };

// kernel templates of pdehip_march2.inc
enum Family { PLAIN /* euler2_kernel */, PER, PERYZ, TALL, TALL_PER, WIDE4, STAGE1W };

// ---------------------------------------------------------------------------------------------
// The compiled instances, one list per (T, VEC): the launcher instantiates exactly these, has_instance() below answers from them.
//   P(RY, HAS_Y, RAGGED, XS, NT, STAGE)  euler2_kernel<T, VEC, RY, m2, HAS_Y, RAGGED, XS, NT> for diffusion (and its unit form unless XS), the
//                                        Euler and the scaled Cahn-Hilliard sweep; STAGE: also with the Runge-Kutta stage epilogue
//   L(FAMILY, template-id up to M2)      all-periodic / tall diffusion tiles, each as unit x NT (four instances)
//   S(FAMILY, template-id)               a single instance
// RAGGED: the variant without the ragged-row code (rows end at chunk boundaries) exists for the 4-row fp64 tile only: there the 5 VGPRs decide
// whether the loads can be issued early (8-19 % at 256^3 and slab-sized grids).  XS: the one-sided halo modes of the first / last slab of a
// non-periodic axis are separate instances (with the ragged-row code): compiled into the hot instances they cost 5-9 % through register
// allocation alone.  STAGE: the epilogue (six more streams) exists for real halo layers on BOTH sides only, without streaming stores, and does
// not fit the ragged 4-row fp64 tile without spilling; the wide fp32 tile carries it with one row (220 VGPRs; two waves per SIMD with more rows:
// 256 VGPRs + scratch) or as euler2_stage1w_kernel at one wave per SIMD.
// ---------------------------------------------------------------------------------------------
#define PDEHIP_E2_INSTANCES_F64_2(P, L, S)                                                                                        \
    L(TALL_PER, euler2_tall_per_kernel<T, VEC) L(TALL, euler2_tall_kernel<T, VEC, 8)                                              \
    L(PERYZ, euler2_peryz_kernel<T, VEC) L(PER, euler2_per_kernel<T, VEC)                                                         \
    P(1, false, true, false, false, true) P(2, true, true, false, false, true) P(2, true, true, true, false, false)              \
    P(4, true, true, false, false, false) P(4, true, false, false, false, true) P(4, true, false, false, true, false)            \
    P(4, true, true, false, true, false) P(4, true, true, true, false, false)
#define PDEHIP_E2_INSTANCES_F32_4(P, L, S)                                                                                        \
    L(WIDE4, euler2_wide4_kernel<T, VEC) S(STAGE1W, euler2_stage1w_kernel<T, VEC, 2, true>)                                       \
    P(1, false, true, false, false, true) P(2, true, true, false, false, false) P(2, true, true, true, false, false)             \
    P(1, true, true, false, false, true)
#define PDEHIP_E2_INSTANCES_F32_2(P, L, S)   /* narrow fp32 tiles, 3-D only */                                                    \
    P(4, true, true, false, false, true) P(2, true, true, false, false, true) P(1, true, true, false, false, true)               \
    P(4, true, true, true, false, false) P(2, true, true, true, false, false)

struct Instance { Family family; int ry; bool has_y, ragged, xs, nt, stage; };
inline const Instance *instances(int elem, int vec, int *count)
{
#define PDEHIP_E2_P(RY, HY, RG, XS, NT, ST) {PLAIN, RY, HY, RG, XS, NT, ST},
#define PDEHIP_E2_L(FAM, ...) {FAM, 0, true, false, false, false, false},
    static const Instance f64_2[] = {PDEHIP_E2_INSTANCES_F64_2(PDEHIP_E2_P, PDEHIP_E2_L, PDEHIP_E2_L)};
    static const Instance f32_4[] = {PDEHIP_E2_INSTANCES_F32_4(PDEHIP_E2_P, PDEHIP_E2_L, PDEHIP_E2_L)};
    static const Instance f32_2[] = {PDEHIP_E2_INSTANCES_F32_2(PDEHIP_E2_P, PDEHIP_E2_L, PDEHIP_E2_L)};
#undef PDEHIP_E2_P
#undef PDEHIP_E2_L
    if (elem == 8 && vec == 2) { *count = (int)(sizeof(f64_2) / sizeof(Instance)); return f64_2; }
    if (elem == 4 && vec == 4) { *count = (int)(sizeof(f32_4) / sizeof(Instance)); return f32_4; }
    if (elem == 4 && vec == 2) { *count = (int)(sizeof(f32_2) / sizeof(Instance)); return f32_2; }
    *count = 0;
    return nullptr;
}

// ---------------------------------------------------------------------------------------------
// tuning knobs, read once
// ---------------------------------------------------------------------------------------------
struct Knobs {
    // PDEHIP_EULER2="ry,blocks,waves" tile rows / wave tiles per sweep / waves per workgroup (tuning aid), PDEHIP_EULER2=off disables the kernel
    int ry = 0; long blocks = 0; int order = -1; bool off = false;
    // PDEHIP_F32_TILE="vec,ry[,stage_vec,stage_ry]" overrides the fp32 tile choice (tuning aid)
    int f32_vec = 0, f32_ry = 0, f32_svec = 0, f32_sry = 0;
    bool wide4_off = false;    // PDEHIP_F32_WIDE4=0 (A/B)
    int stage_wide = 0;        // PDEHIP_F32_STAGE_WIDE=1: the fp32 stage sweeps on euler2_stage1w_kernel
    bool open_off = false;     // PDEHIP_OPEN_ROWS=0 (A/B)
    bool open_y_off = false;   // PDEHIP_OPEN_Y=0 (A/B)
    bool per3_off = false;     // PDEHIP_E2_PER3=0 (A/B)
    bool peryz_off = false;    // PDEHIP_E2_PERYZ=0 (A/B)
    long minlx = 0;            // PDEHIP_E2_MINLX: shortest x-chunk (tuning aid)
    bool unit_off = false;     // PDEHIP_NO_UNIT (A/B aid)
};
inline Knobs knobs_from_env()
{
    Knobs k;
    auto zero = [](const char *name) { const char *e = getenv(name); return e && e[0] == '0'; };
    const char *e = getenv("PDEHIP_EULER2");
    if (e && !strcmp(e, "off")) k.off = true;
    else if (e) sscanf(e, "%d,%ld,%d", &k.ry, &k.blocks, &k.order);
    if ((e = getenv("PDEHIP_F32_TILE"))) sscanf(e, "%d,%d,%d,%d", &k.f32_vec, &k.f32_ry, &k.f32_svec, &k.f32_sry);
    k.wide4_off = zero("PDEHIP_F32_WIDE4");
    if ((e = getenv("PDEHIP_F32_STAGE_WIDE"))) k.stage_wide = atoi(e);
    k.open_off = zero("PDEHIP_OPEN_ROWS");
    k.open_y_off = zero("PDEHIP_OPEN_Y");
    k.per3_off = zero("PDEHIP_E2_PER3");
    k.peryz_off = zero("PDEHIP_E2_PERYZ");
    if ((e = getenv("PDEHIP_E2_MINLX"))) k.minlx = atol(e);
    k.unit_off = getenv("PDEHIP_NO_UNIT") != nullptr;
    return k;
}
inline const Knobs &knobs()
{
    static const Knobs k = knobs_from_env();
    return k;
}

// what the decision reads
struct Query {
    int elem;            // 8: fp64, 4: fp32 (fp32 storage, fp64 registers)
    int ndim;            // 3, or 2: march along the first grid axis, a "plane" is one row (n1 == 1)
    long n0, n1, n2;     // kernel axes: march, rows, lanes
    int per[3];          // 1: periodic, 0: both faces local, 2: box of a larger array (real halo rows / columns; axes 1 and 2)
    int xplain;          // real halo planes instead of BCs on the slowest axis: both sides (1), upper side only (2), lower side only (3)
    int ends;            // > 0: boundary sweep of a slab, the first and the last `ends` planes in ONE launch
    int m2;              // M2_* (never M2_DIFFUSION_UNIT: `unit` says so)
    bool plan;           // the caller launches a run-time compiled instance itself (pdehip_jit.hip)
    bool unit;           // sx == sy == sz == s1 == 1
    bool stage_alias;    // stage sweep: something it writes is one of its pointwise inputs
    bool narrow_only;    // an fp32 box that starts two cells into a four-cell vector (the interior of a block whose fastest axis is cut:
                         // pdehip_block2_loops.h): the narrow tile's 8-byte vectors take it
};

struct Choice {
    bool accepted = false;
    Family family = PLAIN;
    int elem = 0, vec = 0, ry = 0, m2 = 0;
    bool has_y = false, ragged = false, xs = false, nt = false, unit = false;   // (unit: the E2_DIFFUSION_UNIT instance runs)
    long open_tail = 0, open_y = 0;   // columns / rows behind the tiles, left to shell_open_rows (pdehip_shell.hip)
    long ntz = 0, nty = 0, nxc = 0, xstride = 0, nblocks = 0;
    int lx = 0, nwy = 1, nwz = 1;
    unsigned block = 0;
    int per0 = 0;                     // LapArgs::per[0]
};

inline bool has_instance(const Choice &c)
{
    int count;
    const Instance *list = instances(c.elem, c.vec, &count);
    for (int i = 0; i < count; i++) {
        const Instance &s = list[i];
        if (s.family != c.family) continue;
        if (c.family != PLAIN) return true;
        if (s.ry == c.ry && s.has_y == c.has_y && s.ragged == c.ragged && s.xs == c.xs && s.nt == c.nt) return c.m2 != M2_CH_STAGE || s.stage;
    }
    return false;
}

// the name pdehip_last_kernel_name reports (a key of profiles/traffic.json).  Empty: the instance reports none (euler2_stage1w_kernel).
inline void format_name(const Choice &c, char *buf, size_t size)
{
    const char *m2 = c.unit ? "E2_DIFFUSION_UNIT" : "E2_DIFFUSION", *nt = c.nt ? "NT" : "plain stores";
    switch (c.family) {
    case TALL_PER: snprintf(buf, size, "euler2_tall_per_kernel<double,2,%s,%s> (8 rows, 3 plane buffers, 1 wave per SIMD, all-periodic)", m2, nt); break;
    case TALL: snprintf(buf, size, "euler2_tall_kernel<double,2,8,%s,%s> (8 rows, 4 plane buffers, 1 wave per SIMD)", m2, nt); break;
    case PERYZ: snprintf(buf, size, "euler2_peryz_kernel<double,2,%s,%s> (4 rows, 2 waves per SIMD, rows and fastest axis periodic, halo planes along the march axis)", m2, nt); break;
    case PER: snprintf(buf, size, "euler2_per_kernel<double,2,%s,%s> (4 rows, 2 waves per SIMD, all-periodic)", m2, nt); break;
    case WIDE4: snprintf(buf, size, "euler2_wide4_kernel<float,4,%s,%s> (4 rows, 1 wave per SIMD, all-periodic)", m2, nt); break;
    case STAGE1W: snprintf(buf, size, "%s", ""); break;
    default:
        snprintf(buf, size, "euler2_kernel<%s,%d,%d,m2=%d%s,%s,%s,%s,%s>", c.elem == 8 ? "double" : "float", c.vec, c.ry, c.m2, c.unit ? " unit" : "", c.has_y ? "3-D" : "2-D",
                 c.ragged ? "ragged" : "aligned rows", c.xs ? "one-sided" : "two-sided", nt);
    }
}

// ---------------------------------------------------------------------------------------------
// one tile: VEC cells per lane, `ry_f32` rows for fp32 (fp64: 4-row tiles, 226 VGPRs, 2 waves per SIMD)
// ---------------------------------------------------------------------------------------------
inline Choice plan_tile(const Query &q, const Knobs &t2, int VEC, int ry_f32)
{
    Choice c;
    c.elem = q.elem; c.vec = VEC; c.m2 = q.m2;
    const long CW = 64 * VEC;
    const int m2 = q.m2, xplain = q.xplain, ends = q.ends;
    const bool f64 = q.elem == 8, plan = q.plan;
    const bool has_y = c.has_y = q.ndim == 3;
    const double cells = (double)q.n0 * q.n1 * q.n2, bytes = cells * q.elem;
    int ry = (t2.ry && t2.ry != 8) ? t2.ry : 4;   // (8: the tall tile where it applies, see `tall`)
    if (!f64) ry = ry_f32;
    // the tall tile (8 rows, one wave per SIMD, four plane buffers: pdehip_march2.inc): the plain two-step diffusion sweep of fp64
    // grids whose rows end at chunk boundaries.  PDEHIP_EULER2=8 selects it (measurement: profiles/r03_e2_tile_shapes.log)
    // Round 5 (rows on 128-byte lines): the tall tile wins for fields well beyond the Infinity Cache - 512^3 0.2157 -> 0.2108 ms per step (mean of
    // four alternations), 512 x 512 x 256 +3.7 %, 384^3 +2.6 % - and loses below (256^3 -3 %, 128 x 512 x 512 -0.7 %): profiles/r05_ab_tall_tile.log.
    // PDEHIP_EULER2=8 forces it, PDEHIP_EULER2=4 the 4-row tile.  (The tall tile WITH the ragged-row code, for extents that are not multiples of the tile,
    // was built and measured slower than the 4-row tile everywhere - 513^3 440 against 479, 511^3 538 against 599 Gcell-steps/s: profiles/r05_ab_tall_ragged.log.)
    // Round 6: by default only for all-periodic grids (the 3-buffer instance without the face code, euler2_tall_per_kernel); with faces the 4-row tile
    // with late loads and branches is ahead of the tall one now (512^3: 0.443 against 0.488 ms per launch, profiles/r06_e2_bench6.md)
    const bool all_periodic = xplain == 0 && q.per[0] == 1 && q.per[1] == 1 && q.per[2] == 1;
    const bool tall_auto = t2.ry == 0 && bytes > 400.0 * 1048576.0 && all_periodic && !t2.per3_off;
    const bool tall_want = f64 && VEC == 2 && (t2.ry == 8 || tall_auto) && has_y && !plan && xplain == 0 && ends == 0 && m2 == M2_DIFFUSION &&
                           q.per[1] != 2 && q.per[2] != 2;
    // Row counts that are not a multiple of the tile: the last tile is moved back until it ends with the last row (it
    // recomputes rows of its neighbour, pdehip_march2.inc).  With at least 8 tiles per column the big tile with <= 1/8 of
    // redundant rows beats the exactly fitting smaller one (1.5 x instead of 2 x of the intermediate level); an odd number
    // of non-periodic rows has no exactly fitting tile at all.
    // "Open" rows: a row one to eight cells longer than a whole number of chunks (513 = 4 x 128 + 1) gave the moved last chunk a wave of
    // its own that marched every plane for one vector - 25 % more waves (fp64 513^3 0.281 against 0.228 ms per step at 512^3, fp32 0.268
    // against 0.167).  Instead the tiles cover the whole chunks - the halo columns right of the last one are real cells, or the virtual
    // column through the `zhi2` code of the ragged instances - and the remaining columns are recomputed from the input by the LDS-tiled
    // kernel of pdehip_shell.hip (two layers next to the upper face of the fastest axis).  PDEHIP_OPEN_ROWS=0: off (A/B).
    const bool open_case = !t2.open_off && !plan && xplain == 0 && ends == 0 && m2 == M2_DIFFUSION && q.per[1] != 2 && q.per[2] != 2;
    long open_tail = 0;
    if (open_case && q.n2 > CW && q.n2 % CW >= 1 && q.n2 % CW <= 8) open_tail = q.n2 % CW;
    const long n2t = q.n2 - open_tail;   // the columns the tiles cover
    // "Open" COLUMNS of tiles (round 6): one to four rows beyond a whole number of tiles (513 = 64 x 8 + 1) are left to the same recomputing kernel
    // instead of a moved last tile - the tiles then divide the wave slots like those of the multiple of the tile below (513^3: 516 tiles of 4 rows
    // gave 3 x-chunks = 1548 of 2048 wave slots; 512 rows x 512 columns: the tall tile, 256 x 4 = 1024 of 1024).  The halo rows of the last tiles are
    // real rows (or the wrapped ones: `n1` stays the row count of the grid); next to a local upper face the last tile's output row under the
    // virtual row is wrong and recomputed with the rows behind it (the two layers of a job overlap it for an odd remainder).
    // fp64 fields of 8 M cells and more (below, the extra launch costs more than the moved tile).  PDEHIP_OPEN_ROWS=0 / PDEHIP_OPEN_Y=0: off (A/B).
    long open_y = 0;
    // (fp32: for the wide 4-row tile of all-periodic grids - plan() asks for it with ry_f32 = 4)
    const bool open_y_type = (f64 && VEC == 2) || (!f64 && VEC == 4 && ry_f32 == 4);
    if (open_case && !t2.open_y_off && open_y_type && has_y && cells >= 8388608.0 && q.n1 >= 64) {
        // (the recomputing kernel takes six jobs of two layers: the open columns of the fastest axis first)
        const long jobs_left = 6 - (open_tail + 1) / 2;
        const bool tall_rows = tall_want && n2t % CW == 0 && (t2.ry == 8 || (n2t / CW) % 4 == 0) && (q.n1 % 8) >= 1 && ((q.n1 % 8) + 1) / 2 <= jobs_left;
        const long unit_rows = tall_rows ? 8 : 4;
        const long r = q.n1 % unit_rows;
        if (r >= 1 && r <= (unit_rows == 8 ? 7 : 3) && (r + 1) / 2 <= jobs_left) {
            // ... where it fills the wave slots better than the moved last tile does (519 rows = 129 tiles of 4 + 3: as badly quantised as 130 tiles -
            // the extra launch then only costs: 517^3 fp32 664 -> 642 Gcell-steps/s, profiles/r06_call35_sizes.log)
            auto fill = [](long tiles, long slots) { return tiles >= slots ? 1.0 : (double)((slots / tiles) * tiles) / (double)slots; };
            const long ntz_ = (n2t + CW - 1) / CW;
            const long slots_open = (unit_rows == 8 || !f64) ? 1024 : 2048, slots_moved = !f64 ? 1024 : 2048;
            const double with_open = fill((q.n1 - r) / unit_rows * ntz_, slots_open), with_moved = fill((q.n1 + 3) / 4 * ntz_, slots_moved);
            if (with_open > with_moved + 0.08) open_y = r;
        }
    }
    const long n1t = q.n1 - open_y;      // the rows the tiles cover
    // (the tall tile has no code for the virtual FAR column of an open row with one more cell: the ragged 4-row instance takes those)
    // (chosen automatically only where the chunks of a row come in fours - workgroups of four waves that stream whole rows: 300 x 512 x 640, five
    // chunks = one-wave workgroups, 561.6 on the tall tile against 585.4 Gcell-steps/s on the 4-row tile, 384 columns 518 against 572:
    // profiles/r06_call32_sizes.log)
    const bool tall = tall_want && n2t % CW == 0 && n1t % 8 == 0 && !(open_tail == 1 && !q.per[2]) && (t2.ry == 8 || (n2t / CW) % 4 == 0);
    const int ry_want = ry;
    while (ry > 1 && n1t % ry) ry /= 2;
    if (has_y && ry < ry_want) {
        int big = ry_want;
        while (big > ry && n1t < 8L * big) big /= 2;
        if (big > ry) ry = big;
        else if (ry == 1) ry = 2;   // (1-row tiles exist for periodic rows of fp32 grids only and recompute 3 x)
    }
    // the stage epilogue (six more streams) does not fit the ragged 4-row fp64 tile without spilling: 2-row tiles there
    const long n2v = (n2t + VEC - 1) / VEC * VEC;   // a row that ends inside a vector: the last chunk is moved back by n2v - n2 cells
    if (m2 == M2_CH_STAGE && f64 && ry == 4 && n2v % CW != 0) ry = 2;
    if (!has_y) ry = 1;
    if (tall) ry = 8;
    if ((ry != 1 && ry != 2 && ry != 4 && !tall) || n1t < ry || (n2v != n2t && n2t < CW)) return c;
    const bool overlap = n2v != n2t || n1t % ry != 0;
    // the wide fp32 tile has no registers for the virtual row / column in a tile's OUTER halo position (next to a moved tile
    // with local faces): the narrow tile takes those grids (plan())
    if (!f64 && VEC == 4 && ((has_y && n1t % ry != 0 && !q.per[1]) || (q.n2 % CW == 1 && !q.per[2]))) return c;
    // cells of overlapping tiles are computed and stored twice: nothing a sweep writes may be one of its pointwise inputs
    // (the new state of RK4 written over the old one: those sweeps combine with the pointwise kernels)
    if (overlap && m2 == M2_CH_STAGE && q.stage_alias) return c;
    c.ry = ry;
    c.open_tail = open_tail; c.open_y = open_y;
    c.ntz = (n2t + CW - 1) / CW;   // the row may end inside the last chunk
    c.nty = (n1t + ry - 1) / ry;
    const long tiles = c.ntz * c.nty;
    // every x-chunk recomputes two planes of the intermediate level and re-reads four input planes
    long nxc = 2;
    if (ends > 0) {
        // boundary sweep of a slab: the first and the last `ends` planes in ONE launch
        c.lx = ends; c.nxc = 2; c.xstride = q.n0 - ends;
    } else if (!has_y) {
        // 2-D: a wave's march is a chain of dependent row loads (~1 us each out of the Infinity Cache for grids of a few
        // MB), so short chunks win until the chip is full: up to ~4096 waves, chunks of at least `minlx` rows (the
        // 4 overlap rows per chunk cost no HBM traffic for cache-resident grids)
        const long minlx = t2.order > 0 ? t2.order : 2;
        nxc = (t2.blocks ? t2.blocks : 4096) / tiles;
        if (nxc > q.n0 / minlx) nxc = q.n0 / minlx;
        if (nxc < 1) nxc = 1;
    } else {
        // ONE full round of 2048 wave tiles (256 CUs x 8 wave slots at 2 waves per SIMD): measured best or equal from 64 to
        // 512 planes (0.126 vs 0.131 ms/step at 256 planes, 0.066 vs 0.071 at 128 with 4096 tiles; in the slab loop the
        // boundary sweep and the RCCL kernel otherwise queue up behind the second round:
        // profiles/r01_time_tiles_vs_planes.log).  Interior sweep of a THIN slab (exchange-bound): at most 1536, so that
        // the RCCL kernel of the halo stream finds free wave slots at once - workgroups march for the whole sweep, a kernel
        // launched behind a full round waits for it to end (measured: 90 us for 13 us of work).
        const bool thin = xplain && q.n0 < 96;
        // a box of the fast block loop (plain rows / columns): 7/8 of a round - the rim, pack, RCCL and unpack kernels of the halo stream
        // otherwise wait for the END of the sweep (0.0536 -> 0.0501 ms per step at 256 x 128 x 512, profiles/r05_probe_block.md)
        const bool boxed = q.per[1] == 2 || q.per[2] == 2;
        const bool wide1 = !f64 && VEC == 4 && (m2 == M2_CH_STAGE ? ry == 2 : ry == 4) && has_y;   // (euler2_stage1w_kernel, euler2_wide4_kernel: one wave per SIMD)
        const long cap = t2.blocks ? t2.blocks : ((tall || wide1) ? 1024 : (thin ? 1536 : (boxed ? 1792 : 2048)));   // (the tall tile runs one wave per SIMD)
        if (thin) {
            nxc = cap / tiles;
            long minlx = 16;
            while (minlx > 2 && tiles * (q.n0 / minlx) < cap) minlx /= 2;
            if (t2.minlx > 0) minlx = t2.minlx;
            if (nxc > q.n0 / minlx) nxc = q.n0 / minlx;
            if (nxc < 1) nxc = 1;
        } else {
            // The number of x-chunks by a cost model.  A wave marches lx + 2 planes; the chip holds `cap` of them.  While they
            // fit (W <= cap) the sweep is bound by the bytes (W * L) down to the latency floor of a lone march; beyond, the
            // waves left over for the last round march ALONE at that floor: tile counts just above a divisor of `cap` (512 x 513
            // x 512: 516 tiles, 4 chunks = 2064 waves took 0.307 ms per step against 0.225 for 512^3; 300^3: 225 tiles, 10
            // chunks = 2250 waves) take one chunk less instead.  Chunks shorter than 16 planes (two recomputed planes per
            // chunk: > 12.5 % extra work) only while the first round is not full (100^3: 19.7 -> 8.1 us per step).
            double best = 0;
            nxc = 1;
            for (long k = 1; k <= q.n0 / 2 || k == 1; k++) {
                const long lx = (q.n0 + k - 1) / k, real = (q.n0 + lx - 1) / lx;
                if (real != k) continue;   // the same chunking as a smaller count
                if (t2.minlx > 0 ? lx < t2.minlx : (lx < 16 && (k - 1) * tiles >= cap)) break;
                const long W = real * tiles;
                const double full = (double)(W / cap), part = (double)(W % cap) / (double)cap;
                // a wave needs 1.6 - 1.9 us per plane whether the chip is full or not (200^3: 1200 waves of 19 planes took as long
                // per plane as 2000 waves of 12): one round costs its march length, nearly whatever its size; the waves of an
                // incomplete LAST round start while the round before drains (measured: 0.36 of a round for a handful)
                double rounds = W <= cap ? 0.85 + 0.15 * (double)W / (double)cap : full + (part > 0 ? (part > 0.36 ? part : 0.36) : 0.0);
                const double cost = (double)(lx + 2) * rounds;
                if (best == 0 || cost < best) { best = cost; nxc = k; }
            }
        }
    }
    if (ends <= 0) {
        const long lx = (q.n0 + nxc - 1) / nxc;
        c.lx = (int)lx;
        c.nxc = (q.n0 + lx - 1) / lx;
        c.xstride = lx;
    }
    // waves per workgroup = neighbouring chunks of the same rows (1, 2 or 4; PDEHIP_EULER2 third field overrides)
    c.nwz = (c.ntz % 4 == 0) ? 4 : (c.ntz % 2 == 0 ? 2 : 1);
    if (has_y && t2.order > 0) {   // tuning aid: third field = 10 * (waves along the rows) + (waves along the fastest axis)
        const int wz_ = t2.order % 10, wy_ = t2.order / 10 > 0 ? t2.order / 10 : 1;
        if (wz_ > 0 && c.ntz % wz_ == 0 && c.nty % wy_ == 0 && wz_ * wy_ <= 4) { c.nwz = wz_; c.nwy = wy_; }
    }
    c.nblocks = c.nxc * tiles / (c.nwz * c.nwy);
    c.block = 64u * c.nwz * c.nwy;
    // real halo planes instead of BCs on the slowest axis: both sides (1), upper side only (2), lower side only (3)
    c.per0 = xplain ? (xplain == 1 ? 2 : (xplain == 2 ? 3 : 4)) : q.per[0];
    const bool xs = xplain > 1;
    // (the virtual rows next to a moved last tile - pdehip_march2.inc: ylo2 / yhi2 - are part of the ragged-row code)
    // (... and so is the virtual FAR column right of the last chunk of an open row with one more cell: zhi2)
    c.xs = xs;
    c.ragged = xs || !(f64 && ry == 4 && n2v % CW == 0) || (has_y && n1t % ry != 0 && !q.per[1]) || (open_tail == 1 && !q.per[2]);
    if (plan) {   // (a run-time build: any m2, two-sided tiles of 2 or 4 rows, 1 row in 2-D)
        c.accepted = has_y ? (ry == 2 || ry == 4) : ry == 1;
        return c;
    }
    // the stage epilogue exists for real halo layers on BOTH sides (a run-time argument of the plain instances) but not as
    // one-sided (XS) instances: the first / last slab of a non-periodic axis combines with the pointwise kernels
    if (m2 == M2_CH_STAGE && xs) return c;
    // NT: streaming stores, for the hot instance and fields that do not fit the 256 MB Infinity Cache
    const bool big = bytes > 192.0 * 1048576.0;
#if defined(PDEHIP_NT_LOADS) && PDEHIP_NT_LOADS == 2
    const bool nt = false;   // A/B variant: non-temporal loads, plain stores
#else
    // (round 6: also the ragged 4-row fp64 diffusion tile of two-sided grids - 500 x 500 x 300, rows that end inside a chunk - has a streaming-store form)
    const bool nt = (!c.ragged || (f64 && ry == 4 && has_y && !xs && m2 == M2_DIFFUSION)) && m2 != M2_CH_STAGE && big;
#endif
    // unit spacing and D = 1 (UnitGrid benchmarks): the 3-D instances exist without the multiplications by 1.0 (fp32 and the
    // cache-resident sizes are VALU-bound: up to 10 %)
    const bool unit = !t2.unit_off && q.unit;
    // every axis periodic: the instances without the code of the local faces (pdehip_march2.inc, PER3).  PDEHIP_E2_PER3=0: off (A/B)
    const bool per3 = !t2.per3_off && all_periodic && m2 == M2_DIFFUSION && f64 && VEC == 2 && has_y;
    if (tall) {
        // (the tall instances take streaming stores and the unit form whatever PDEHIP_NT_LOADS and PDEHIP_NO_UNIT say)
        c.family = per3 ? TALL_PER : TALL;
        c.ragged = false; c.nt = big; c.unit = q.unit;
    } else if (f64 && VEC == 2 && !t2.peryz_off && xplain == 1 && q.per[1] == 1 && q.per[2] == 1 && m2 == M2_DIFFUSION && has_y && ry == 4 && !c.ragged && !open_tail && !open_y) {
        // a slab of a grid that is periodic along its rows and its fastest axis, real halo planes on both sides (interior and boundary sweeps of the
        // slab loops): the all-periodic 4-row body with the march axis as the arguments say (PER3 = 2).  PDEHIP_E2_PERYZ=0: off (A/B)
        c.family = PERYZ; c.nt = nt; c.unit = unit;
    } else if (per3 && ry == 4 && !c.ragged) {   // (fp64, 4 rows, rows that end at chunk boundaries - or open rows: their last columns are left to shell_open_rows)
        c.family = PER; c.nt = nt; c.unit = unit;
    } else if (!f64 && VEC == 4 && ry == 4 && m2 == M2_DIFFUSION) {
        // fp32 diffusion: the wide 4-row tile at one wave per SIMD (pdehip_march2.inc), which has no code for faces, halo planes or slab ends
        if (!all_periodic || ends != 0) return c;
        // streaming stores for fields beyond the Infinity Cache (512^3: 874 against 848 Gcell-steps/s)
        c.family = WIDE4; c.nt = big; c.unit = unit;
    } else if (!f64 && VEC == 4 && m2 == M2_CH_STAGE && ry == 2 && has_y) {   // the wide fp32 stage tile at one wave per SIMD (pdehip_march2.inc)
        c.family = STAGE1W;
    } else {
        c.family = PLAIN; c.nt = nt; c.unit = unit && m2 == M2_DIFFUSION && !xs;   // (the one-sided slab ends have no unit form)
    }
    // a 1-row tile of a 3-D grid is its own neighbour's halo: the tile of row 1 reads the virtual row -1, which only the
    // tile of row 0 transforms (`ylo`) - correct for periodic rows only
    if (has_y && ry == 1 && !q.per[1]) return c;
    // Is there an instance of this tile?  One case answers "covered" without one and is then declined by the launcher (kept as it was found,
    // profiles/e2_dispatch_refactor.md): the fp64 stage sweep whose ROWS make the 4-row tile ragged (a moved last tile next to local faces).
    const bool stage_rows = f64 && m2 == M2_CH_STAGE && c.family == PLAIN && ry == 4 && c.ragged;
    c.accepted = has_instance(c) || stage_rows;
    return c;
}

// ---------------------------------------------------------------------------------------------
// the decision: fp64 has one tile shape; fp32 tries its tiles in turn
// fp32 tiles (fp32 storage, fp64 registers).  The wide tile - 4 cells per lane (16-byte accesses), 2 rows - is at 252 VGPRs
// without room for the stage epilogue (256 + 64 B of scratch with it).  The NARROW tile - 2 cells per lane (8-byte accesses),
// 4 rows, the shape of the fp64 tile - needs 194 VGPRs (204 with the stage epilogue) and recomputes 1.5 x instead of 2 x of
// the intermediate level.
// ---------------------------------------------------------------------------------------------
inline Choice plan(const Query &q, const Knobs &k)
{
    if (q.elem == 8) return plan_tile(q, k, 2, 0);
    const bool stage = q.m2 == M2_CH_STAGE, d3 = q.ndim == 3;
    if (q.narrow_only) return (!d3 || q.plan || stage) ? Choice() : plan_tile(q, k, 2, 4);
    // Measured at 256^3 / 512^3 (profiles/r03_f32_tiles.md): the sweeps without the stage epilogue are fastest on the wide
    // 2-row tile (diffusion 0.0233 vs 0.0249 ms per step, Cahn-Hilliard 0.0575 vs 0.0585); the Runge-Kutta stage sweeps
    // need the narrow 4-row tile to carry their epilogue at all (RKF45 attempt 0.786 -> 0.755 ms).  The run-time built
    // kernels of pdehip_jit.hip keep the wide tile (`plan`).
    int vec = 4, ry = 2;
    const double cells = (double)q.n0 * q.n1 * q.n2;
    // rows that fill the 128-cell chunks of the narrow tile much better than the 256-cell chunks of the wide one
    // (300 cells: 78 % against 59 % of the lanes own cells; 513: 80 % against 67 %)
    // (rows one to eight cells beyond whole chunks leave those cells to another kernel: plan_tile, "open" rows)
    auto fill = [&](long cw) {
        const long t = q.n2 % cw;
        return (q.n2 > cw && t >= 1 && t <= 8) ? 1.0 : (double)q.n2 / (double)((q.n2 + cw - 1) / cw * cw);
    };
    const bool narrow_fills = fill(128) > 1.15 * fill(256);
    // all-periodic diffusion: the wide tile with four rows at one wave per SIMD (round 6; PDEHIP_F32_WIDE4=0: off, A/B).  With faces it was measured
    // too: 441.6-443.1 against 420.5-424.7 us per launch at 512^3, 61.7 against 61.6 at 256^3 in the kernel trace (profiles/r06_f32_wide4.md) - not used there
    // (grids of a few MB are bound by the latency of a march, not by instructions: 64 x 64 x 256 lost 4 %)
    const bool wide4 = !k.wide4_off && d3 && !q.plan && q.m2 == M2_DIFFUSION && q.xplain == 0 && q.ends == 0 && q.per[0] == 1 && q.per[1] == 1 && q.per[2] == 1 &&
                       (q.n1 % 4 == 0 || (cells >= 8388608.0 && q.n1 >= 64)) &&   // (or one to three rows more, left open: plan_tile)
                       !k.f32_vec && cells >= 2097152.0;
    // (rows that fill the 256-cell chunks of the wide tile badly go to the narrow tile below: 384 cells = 1.5 chunks lost 24 % here)
    if (wide4 && !narrow_fills) {
        const Choice c = plan_tile(q, k, 4, 4);
        if (c.accepted) return c;
    }
    if (d3 && !q.plan) {
        if (stage) { vec = k.f32_svec ? k.f32_svec : 2; ry = k.f32_svec ? k.f32_sry : 4; }
        else if (k.f32_vec) { vec = k.f32_vec; ry = k.f32_ry; }
        else if (narrow_fills) { vec = 2; ry = 4; }
    }
    // PDEHIP_F32_STAGE_WIDE=1: the stage sweeps on the wide 2-row tile at ONE wave per SIMD (16-byte accesses; euler2_stage1w_kernel)
    if (stage && k.stage_wide && d3 && !q.plan && !k.f32_svec) { vec = 4; ry = 2; }
    else if (stage && vec == 4 && ry > 1 && d3) ry = 1;   // the wide tile carries the stage epilogue with one row only
    if (vec == 2) return plan_tile(q, k, 2, ry);
    const Choice c = plan_tile(q, k, 4, ry);
    // what the wide tile declines (rows shorter than its chunk that end inside a 4-cell vector, moved last tiles next to
    // local faces) the narrow tile (2-cell vectors, 4 rows) may still take
    if (!c.accepted && d3 && !q.plan) return plan_tile(q, k, 2, 4);
    return c;
}

}  // namespace e2plan
}  // namespace pdehip
