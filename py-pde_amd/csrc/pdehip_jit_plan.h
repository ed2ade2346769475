// pdehip_jit_plan.h - what a run-time built one-level sweep (pdehip_jit.hip: lap_march_body<..., LAP_CUSTOM, ...> around a generated epilogue)
// runs: the generic kernel or the instance (RY, CZ, WY, HASX, IBC, STAGE, TAILS), and the launch geometry (wave tiles per plane, planes per
// workgroup, x-chunks, workgroups, threads).  Plain host C++17 without a HIP header: pdehip_jit.hip asks plan() and launches what it answers,
// a CPU test (tests/test_jit_cases_cpu.py through tests/shim/jit_plan_probe.cpp) asks the same function.
#pragma once

#include <cstdio>
#include <cstdlib>

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

}  // namespace jitplan
}  // namespace pdehip
