// pdehip_jit_plan.h - what a run-time built one-level sweep (pdehip_jit.hip: lap_march_body<..., LAP_CUSTOM, ...> around a generated epilogue)
// runs: the generic kernel or the instance (RY, CZ, WY, HASX, IBC, STAGE, TAILS), and the launch geometry (wave tiles per plane, planes per
// workgroup, x-chunks, workgroups, threads); and which route the fixed-step Euler loop takes (tile_mode, replay_applies).  Plain host C++17
// without a HIP header: pdehip_jit.hip asks plan() and launches what it answers, CPU tests (tests/test_jit_cases_cpu.py,
// tests/test_tile2d_cases_cpu.py through tests/shim/jit_plan_probe.cpp) ask the same functions.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace pdehip {
namespace jitplan {

// tuning knobs, read once per process by pdehip_jit.hip; 0: not set
struct Knobs {
    int ry = 0;        // PDEHIP_JIT_RY: rows per wave tile (kernels are built on demand)
    int cz = 0;        // PDEHIP_JIT_CZ: chunks per wave tile (an upper limit)
    int wy = 0;        // PDEHIP_JIT_WY: waves per workgroup of the stage sweeps
    long blocks = 0;   // PDEHIP_JIT_BLOCKS: wave tiles per sweep
};
inline Knobs knobs_from_env()
{
    Knobs k;
    const char *e;
    if ((e = getenv("PDEHIP_JIT_RY"))) k.ry = atoi(e);
    if ((e = getenv("PDEHIP_JIT_CZ"))) k.cz = atoi(e);
    if ((e = getenv("PDEHIP_JIT_WY"))) k.wy = atoi(e);
    if ((e = getenv("PDEHIP_JIT_BLOCKS"))) k.blocks = atol(e);
    return k;
}

// what the decision reads
struct Query {
    int elem;          // 8: fp64, 4: fp32 (fp32 storage, fp64 registers)
    int ndim;          // 1, 2 or 3
    long n0, n1, n2;   // kernel axes: march (1 below 3-D), rows (1 in 1-D), lanes
    bool aligned;      // every array pointer of the call is 16-byte aligned
    bool stage;        // the Runge-Kutta stage epilogue follows the generated one (StageFuse)
    int kind;          // StageFuse::kind of a stage sweep
    int nk;            // earlier slopes of a stage sweep, counted up to two: 0, 1, or 2 for "k[1] is set"
    bool fused;        // at least one face is applied on the fly
};

// the vectorised kernel takes any row length of a 2-D / 3-D grid whose arrays can be read in 16-byte vectors
inline bool vectorised(int ndim, bool aligned) { return ndim >= 2 && aligned; }

struct Choice {
    bool generic = false;   // the one-cell-per-thread kernel (no stage epilogue: a stage sweep of such a call launches nothing)
    int elem = 0, vec = 0, ry = 0, cz = 0, wy = 1;
    bool hasx = false, ibc = false, stage = false, tails = false;
    long ntz = 0, nty = 0, lx = 1, nxc = 1, nblocks = 0;
    unsigned threads = 0;
};

inline Choice plan(const Query &q, const Knobs &t)
{
    Choice c;
    c.elem = q.elem;
    if (!vectorised(q.ndim, q.aligned)) {
        c.generic = true;
        c.vec = c.ry = c.cz = 1;
        const long b = (q.n0 * q.n1 * q.n2 + 255) / 256;
        c.nblocks = b > 8192 ? 8192 : (b < 1 ? 1 : b);
        c.threads = 256;
        return c;
    }
    const int vec = c.vec = q.elem == 8 ? 2 : 4;
    const long chunk = 64L * vec;
    const long chunks = (q.n2 + chunk - 1) / chunk;
    int cz = chunks >= 4 ? 4 : (chunks >= 2 ? 2 : 1);
    // measured: 2-row tiles win in 2-D as well (4096^2 Allen-Cahn 80 % vs 40 % of the HBM peak with 8 rows)
    int ry = 2;
    // stage sweeps: 1-row tiles.  The 2-row stage kernel (28 KB of code) runs at its one-wave-per-SIMD speed when it
    // is loaded through hipModuleLoadData (4.9 vs 3.7 ms per RK4 step at 512^3; the same code built into the library
    // is not affected, nor is this one once librocprofiler-sdk.so is in the process); with half the code the
    // effect is gone (4.0 ms): profiles/r01_time_expr_rk.md
    if (q.stage) ry = 1;
    if (t.ry > 0) ry = t.ry;
    if (t.cz > 0 && t.cz <= cz) cz = t.cz;
    auto n_tiles = [&](int ry_, int cz_) {
        const long per_plane = ((q.n1 + ry_ - 1) / ry_) * ((q.n2 + chunk * cz_ - 1) / (chunk * cz_));
        return q.ndim == 3 ? per_plane * q.n0 : per_plane;
    };
    while (cz > 1 && n_tiles(ry, cz) < 512) cz /= 2;
    c.ry = ry; c.cz = cz;
    c.hasx = q.ndim == 3; c.ibc = q.fused; c.stage = q.stage;
    const int wy = c.wy = (q.stage && t.wy > 0) ? t.wy : 1;
    c.tails = (q.n2 % vec != 0) || (chunks % cz != 0);   // rows that end inside a vector / idle chunks in the last tile (pdehip_march.inc)
    c.ntz = (q.n2 + chunk * cz - 1) / (chunk * cz);
    c.nty = (q.n1 + (long)wy * ry - 1) / ((long)wy * ry);
    const long tiles = c.ntz * c.nty;
    long lx = q.n0;
    if (c.hasx) {
        // stages with few pointwise streams: two waves per SIMD (see launch_laplace_t, profiles/r01_time_rk.md)
        const long want = t.blocks > 0 ? t.blocks : ((q.stage && (q.kind == 1 || q.nk < 2)) ? 2048 : 1024);
        long nxc = (want / wy + tiles - 1) / tiles;   // `want` counts waves
        if (nxc < 1) nxc = 1;
        if (nxc > q.n0) nxc = q.n0;
        lx = (q.n0 + nxc - 1) / nxc;
    }
    c.lx = lx;
    c.nxc = (q.n0 + lx - 1) / lx;
    c.nblocks = c.nxc * tiles;
    c.threads = 64u * (unsigned)wy;
    return c;
}

// the name pdehip_last_kernel_name reports after the launch
inline void format_name(const Choice &c, char *buf, size_t size)
{
    const char *T = c.elem == 8 ? "double" : "float";
    if (c.generic) { snprintf(buf, size, "pde_kernel<generic,%s> (run-time built)", T); return; }
    snprintf(buf, size, "pde_kernel<%s,%d,RY=%d,CZ=%d,WY=%d,%s,%s,%s,%s> (lx=%ld, %ld x-chunk%s; run-time built)", T, c.vec, c.ry, c.cz, c.wy,
             c.hasx ? "3-D" : "2-D", c.ibc ? "ibc" : "-", c.stage ? "stage" : "-", c.tails ? "tails" : "-", c.lx, c.nxc, c.nxc == 1 ? "" : "s");
}

// ---- the route of the fixed-step Euler loop (pdehip_jit_euler_run): the tile kernel, the replay of a captured block, or plain launches ----
struct LoopKnobs {
    bool tile = true;              // PDEHIP_TILE2D: "0" / "off" keeps the loop away from the tile kernel
    long tile_cells = 1L << 21;    // PDEHIP_TILE2D_CELLS: the largest grid the tile kernel takes
    bool graph = false;            // PDEHIP_JIT_GRAPH=1: replay a captured block of steps
};
inline LoopKnobs loop_knobs_from_env()
{
    LoopKnobs k;
    const char *e = getenv("PDEHIP_TILE2D");
    k.tile = !(e && (e[0] == '0' || !strcmp(e, "off")));
    if ((e = getenv("PDEHIP_TILE2D_CELLS")) != nullptr) k.tile_cells = atol(e);
    k.graph = (e = getenv("PDEHIP_JIT_GRAPH")) && e[0] == '1';
    return k;
}

// what the route reads of a pass (pdehip_jit_pass_t, include/pdehip.h)
constexpr int kNoArray = INT32_MIN;   // PDEHIP_JIT_NONE
struct PassDesc {
    int src, extras[3], out;   // >= 0: a fixed array, -1 - k: component k of the state, kNoArray
    bool faces;                // the pass has a table of conditions
    bool second_body;          // its handle carries a second epilogue (pdehip_jit_create2)
};

// The mode in which the tile kernel (pdehip_tile2d.inc) takes the loop, or 0.  p: the first min(npasses, 2) passes.
//   2, one field: ONE pass of the state alone
//   3, two fields: one pass per field, each reading its own component through the stencil and at most the OTHER component's centre value (slot e0)
//   4, a two-pass chain of ONE field: tmp = f1(state), state' = f2(tmp; e0 = state)
// n1, n2: rows and lanes of the 2-D grid.  (Whether the kernel covers the faces of the passes is plan_tile2d's decision, after this one.)
inline int tile_mode(const PassDesc *p, int npasses, int ncomp, int ndim, long n1, long n2, long nsteps, bool bc_program, const LoopKnobs &k)
{
    if (!k.tile || bc_program || ndim != 2 || n1 * n2 > k.tile_cells || nsteps < 2) return 0;
    auto none = [](int v) { return v == kNoArray; };
    auto own_pass = [&](const PassDesc &q, int comp, int other) {
        return q.src == -1 - comp && q.out == -1 - comp && (none(q.extras[0]) || q.extras[0] == -1 - other) && none(q.extras[1]) && none(q.extras[2]) &&
               q.faces && !q.second_body;
    };
    if (npasses == 1 && ncomp == 1 && own_pass(p[0], 0, 0) && none(p[0].extras[0])) return 2;
    if (npasses == 2 && ncomp == 2 && own_pass(p[0], 0, 1) && own_pass(p[1], 1, 0)) return 3;
    if (npasses == 2 && ncomp == 1 && p[0].src == -1 && p[0].out >= 0 && none(p[0].extras[0]) && none(p[0].extras[1]) && none(p[0].extras[2]) && p[0].faces &&
        p[1].src == p[0].out && p[1].out == -1 && (none(p[1].extras[0]) || p[1].extras[0] == -1) && none(p[1].extras[1]) && none(p[1].extras[2]) && p[1].faces &&
        !p[0].second_body && !p[1].second_body)
        return 4;
    return 0;
}

// The replay of a captured block: the first two steps always run as plain launches (they build the kernels), then whole blocks of
// kReplayBlock steps, worth it from four blocks on.  Explicit time changes the arguments of every step; `comm`: the passes exchange
// ghost layers through a communicator (no RCCL groups inside a captured graph).
constexpr long kReplayBlock = 16;
inline bool replay_applies(bool uses_time, long nsteps, bool comm, const LoopKnobs &k)
{
    return k.graph && !uses_time && nsteps - 2 >= 4 * kReplayBlock && !comm;
}

}  // namespace jitplan
}  // namespace pdehip
