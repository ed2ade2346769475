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
// = 1.15 x.  (40 / PY) * (72 / 2) = 720 patches: 768 threads, the last 48 repeat patch 0 (a halo patch: it stores nothing).
constexpr int TY = 32, TZ = 64, PY = 2, LEVELS = 4, HALO = 4;
constexpr int RY = TY + 2 * HALO, RZ = TZ + 2 * HALO;           // the region of level 0
constexpr int NPY = RY / PY, NPZ = RZ / 2, PATCHES = NPY * NPZ;
constexpr int THREADS = (PATCHES + 63) / 64 * 64;
// one plane of one level in LDS: a ring of one row / two cells that nothing writes around the region (16-byte alignment of the patches)
constexpr int LROWS = RY + 2, LPITCH = RZ + 4;
constexpr long LDS_BYTES = (long)LEVELS * LROWS * LPITCH * 8;
constexpr long MIN_CHUNK = 8;       // the fewest output planes of an x-chunk (each chunk recomputes 2 * HALO planes more)
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
