// pt_kernels.hip -- wavefront (Laine-style) spectral path tracer for gfx950: the kernels and
// device routines, the functions that pick a kernel instance for a launch (pt_select.h) and
// the single-question probes of the mi_pt_* C ABI (include/mi_pt.h), each entry point under
// its kernel. The rest of the ABI is host code of its own: pt_create.hip (mi_pt_create) and
// pt_render.hip (the pool, the launches of an iteration, the render driver); pt_pool.h holds
// what both sides read. One resident pool of path slots lives in HBM as
// structure-of-arrays "planes" (plane k of slot i at base + k*pool + i, so every
// per-bin access of a wave is one coalesced 256-B transaction). One iteration is
//
//   generate : flush finished paths into the film, refill empty slots from a global
//              work counter (pixel, sample#) -> Halton camera sample -> camera ray
//   extend   : BVH2 closest-hit traversal, short stack staged in LDS
//   shade    : emission, termination, BSDF frame, light choice + light sample (NEE),
//              BSDF sample for MIS, BSDF sample for the continuation, Russian roulette;
//              streams the 31 bins of beta / contributions through HBM planes
//   shadow   : any-hit traversal of the NEE shadow rays, adds unoccluded contributions
//   mis      : the BSDF-sampled rays of the direct-lighting estimates: is the closest hit the
//              sampled light's shape? (a visibility query up to that shape, k_trav MODE 3; the
//              closest-hit traversal, MODE 2, for scenes with instances or a masked emitter); adds the
//              emission if so; closes the per-vertex direct-lighting statistics
//
// which restates, per path vertex, PathIntegrator::Li (src/integrators/path.cpp:64-188)
// with UniformSampleOneLight / EstimateDirect (src/core/integrator.cpp:85-215) inside
// SamplerIntegrator::Render's sample loop (src/core/integrator.cpp:228-342). Halton
// dimensions are consumed in the reference's order, so every path makes the same
// decisions as the CPU reference up to floating-point differences of libm functions.
// No MFMA: this path is latency/bandwidth bound (traversal) and VALU bound (shading).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <type_traits>
#include "d_sampling.h"
#include "d_texture.h"
#include "d_lens.h"
#include "d_camera.h"
#include "pt_host.h"

using namespace dpt;

// This file is compiled six times in parallel (Makefile): MIPT_PART 0 holds every kernel but the shading kernel's instances,
// with the kernel selection and the probes; parts 1-3 and 5 hold the k_shade instances (95 % of the compile
// time; MIPT_SHADE_INSTANCES says which), part 4 the BSDF probe's kernels and their launcher (LaunchBsdfProbe: test-only code, kept out of the
// parts a render runs). Without MIPT_PART (tools/isa_stats.py without --part) every kernel is in one translation unit.
// MIPT_HAS_MAIN guards part 0's kernels and what names them; the library's other host code is pt_create.hip and pt_render.hip.
#ifdef MIPT_PART
#define MIPT_HAS_MAIN (MIPT_PART == 0)
#else
#define MIPT_HAS_MAIN 1
#endif

namespace dptk {   // (the pool's types, the counters and the tuning macros that the host units read too: pt_pool.h)

DEV float Get4(const float4 &v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : (k == 2 ? v.z : v.w)); }
DEV void Set4(float4 &v, int k, float x) { if (k == 0) v.x = x; else if (k == 1) v.y = x; else if (k == 2) v.z = x; else v.w = x; }
DEV int LPlane(int flags) { return (flags & F_L_IN_B) ? Q_LB : Q_L; }        // the line that holds the path's L
DEV int LOtherPlane(int flags) { return (flags & F_L_IN_B) ? Q_L : Q_LB; }   // ... and the one for the candidate
DEV int StateWord(int flags, int bounces, int dim) { return (flags & FLAG_MASK) | ((bounces & 0xff) << BOUNCE_SHIFT) | (int)((unsigned)(dim & 0x3ff) << DIM_SHIFT); }
DEV int StateBounces(int word) { return (word >> BOUNCE_SHIFT) & 0xff; }
DEV int StateDim(int word) { return (int)((unsigned)word >> DIM_SHIFT); }
// Conservative: false only if the ray o + t d, t >= 0, stays outside the box; [*lo, *hi] contains the parameters at which it is inside.
DEV bool RaySpanInBox(const V3 &o, const V3 &d, const float4 &bmin, const float4 &bmax, float *spanLo, float *spanHi) {
    float t0 = 0.f, t1 = kInfinity;
    const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z}, lo[3] = {bmin.x, bmin.y, bmin.z}, hi[3] = {bmax.x, bmax.y, bmax.z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (dd[a] == 0.f) { if (oo[a] < lo[a] || oo[a] > hi[a]) return false; continue; }
        const float inv = 1.f / dd[a];
        float ta = (lo[a] - oo[a]) * inv, tb = (hi[a] - oo[a]) * inv;
        if (ta > tb) { const float tt = ta; ta = tb; tb = tt; }
        tb *= 1.0001f;   // (rounding of the products: widen the exit)
        if (ta > t0) t0 = ta;
        if (tb < t1) t1 = tb;
    }
    *spanLo = t0; *spanHi = t1;
    return !(t0 > t1);
}
// The two words k_trav<3> reads beside a MIS ray (R_MI1.z, .w): the end tHi of the span in which the sampled light's shape can
// be hit, and that shape's primitive | c << 27 with tLo = tHi (1 - 2^-c) at or below the span's start (c = 0: tLo = 0).
DEV void MisSpanWords(float lo, float hi, unsigned prim, float *tHi, float *word) {
    const float w = 1.f - lo / hi;          // tLo = hi (1 - 2^-c) <= lo  <=>  2^-c >= w
    int c = 126 - (int)((__float_as_uint(w) >> 23) & 0xffu);
    if (!(w > 0.f)) c = 20;
    c = (lo > 0.f && hi < kInfinity) ? max(0, min(c, 20)) : 0;   // (1 - 2^-c is exact in a float up to c = 24)
    *tHi = hi;
    *word = __uint_as_float(prim | ((unsigned)c << MIS_EXCL_BITS));
}

// Ray::time of the slot's path: the camera ray's, which every ray the path spawns keeps (Interaction::SpawnRay[To] pass the
// interaction's time on, interaction.h:64-86). A plane of its own that exists only in scenes with moving instances and is
// read only where a ray meets an instance; elsewhere the shutter-open time, which nothing then depends on.
DEV float PathTime(const DScene &s, const Pool &pool, uint32_t slot) { return s.motions ? pool.F(s.timePlane, slot) : s.camera.shutter_open; }
// SurfaceInteraction::instanceId of a hit reached through instance k (primitive.cpp:89; the wrapper of a moving shape: 0)
DEV unsigned InstanceIdOf(const mi_instance &in, int k) { return in.instance_id ? in.instance_id : (in.motion ? 0u : (unsigned)k + 1u); }

DEV DevStats &Stats(DevCounters *ctr) { return ctr->stats[blockIdx.x & (STAT_STRIPES - 1)]; }

DEV unsigned long long WaveSum(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
DEV void CountAdd(unsigned long long *ctr, unsigned long long v) {
    v = WaveSum(v);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(ctr, v);
}

// Wave-level compaction: every lane of the wave calls this (convergent); lanes with
// pred get consecutive queue positions from one atomic per wave (ballot + popcount).
DEV void QueueAppend(unsigned *counter, uint32_t *queue, bool pred, uint32_t value) {
    const unsigned long long mask = __ballot(pred);
    if (mask == 0) return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)mask) - 1;
    unsigned base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned)__popcll(mask));
    base = __shfl(base, leader, 64);
    if (pred) queue[base + __popcll(mask & ((1ull << lane) - 1))] = value;
}

// Block-level compaction: every thread of the block calls this (it synchronises); threads
// with pred get consecutive positions from ONE atomicAdd per block. `scratch` is 5 words of
// LDS that no other call of the same kernel uses.
DEV unsigned BlockReserve(unsigned *counter, bool pred, unsigned *scratch) {
    const unsigned long long mask = __ballot(pred);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) scratch[wave] = (unsigned)__popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned tot = scratch[0] + scratch[1] + scratch[2] + scratch[3];
        scratch[4] = tot ? atomicAdd(counter, tot) : 0;
    }
    __syncthreads();
    unsigned base = scratch[4];
    for (int w = 0; w < wave; ++w) base += scratch[w];
    return base + (unsigned)__popcll(mask & ((1ull << lane) - 1));
}

// Three reservations behind ONE pair of barriers, their atomics issued by three different waves (k_shade ends in an append to
// the shadow queue, one to the MIS queue and one to the queue of the dark MIS rays; one after the other they cost three atomic
// round trips and six barriers). `scratch`: 15 words of LDS.
DEV void BlockReserve3(unsigned *counterA, bool predA, unsigned *counterB, bool predB, unsigned *counterC, bool predC, unsigned *scratch,
                       unsigned *posA, unsigned *posB, unsigned *posC) {
    const unsigned long long mA = __ballot(predA), mB = __ballot(predB), mC = __ballot(predC);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { scratch[wave] = (unsigned)__popcll(mA); scratch[5 + wave] = (unsigned)__popcll(mB); scratch[10 + wave] = (unsigned)__popcll(mC); }
    __syncthreads();
    if (lane == 0 && wave < 3) {
        unsigned *sc = scratch + 5 * wave;
        const unsigned tot = sc[0] + sc[1] + sc[2] + sc[3];
        sc[4] = tot ? atomicAdd(wave == 0 ? counterA : (wave == 1 ? counterB : counterC), tot) : 0;
    }
    __syncthreads();
    unsigned a = scratch[4], b = scratch[9], c = scratch[14];
    for (int w = 0; w < wave; ++w) { a += scratch[w]; b += scratch[5 + w]; c += scratch[10 + w]; }
    const unsigned long long lt = (1ull << lane) - 1ull;
    *posA = a + (unsigned)__popcll(mA & lt);
    *posB = b + (unsigned)__popcll(mB & lt);
    *posC = c + (unsigned)__popcll(mC & lt);
}

// ------------------------------------------------------------------ traversal
struct Hit {
    int prim;
    float t, b0, b1, b2;
    int inst = -1;   // the object instance the hit primitive was reached through (mi_instance index), -1: a world primitive
};

// BVHAccel::Intersect / IntersectP (bvh.cpp:662-738) with Bounds3::IntersectP
// (geometry.h:1420-1447) over the "wide" node array: an interior node carries the boxes
// of both children, so one 64-B fetch decides both child visits and the ray's chain of
// dependent loads is halved. The visit semantics are the reference's:
//   * near child (by dirIsNeg[axis]) first; the far child is pushed only if its box is
//     hit, together with its entry distance tMin;
//   * when popped, the far child is re-validated with `tMin < tMax` -- the only part of
//     the reference's box test that depends on the (shrinking) ray tMax -- so exactly the
//     nodes the reference would enter are entered, and leaf primitives are tested in the
//     same order against the same tMax: equal-t ties resolve identically.
// SIMT schedule: "while-while" (walk interior nodes until the lane holds a leaf, then the
// wave tests leaves together). Quadric primitives are postponed: recorded in encounter
// order with the ray's tMax of that moment and replayed after the triangles in the
// reference's order (ResolveQuadrics), so the interval-arithmetic sphere code runs at full
// lane utilisation.
// (TMIN = false: the any-hit kernel keeps no entry distances -- a shadow ray's tMax never shrinks, so an entry pushed in
// front of it stays in front of it -- which takes the stack from 36 to 24 KB per block: five blocks per CU instead of four)
template <bool TMIN>
struct TravLdsT {
    int node[STACK_LDS][BLOCK];
    int meta[STACK_LDS][BLOCK];
    float tmin[TMIN ? STACK_LDS : 1][BLOCK];
};
// The block's traversal stack lives in one LDS object reached by name (no generic pointers).
template <bool TMIN>
DEV TravLdsT<TMIN> &TravStack() {
    __shared__ TravLdsT<TMIN> stack;
    return stack;
}
struct TravSpill {
    int node[STACK_SPILL];
    int meta[STACK_SPILL];
    float tmin[STACK_SPILL];
};
struct RayCtx {  // per-lane ray constants
    float ox, oy, oz, dx, dy, dz, ix, iy, iz;
    bool n0, n1, n2;
    bool slow;   // a component of the direction is zero (an infinite reciprocal): only then can a slab product be NaN (BoxTestFast)
    DEV int Octant() const { return (n0 ? 1 : 0) | (n1 ? 2 : 0) | (n2 ? 4 : 0); }
};
DEV void InitRayCtx(RayCtx &r, float ox, float oy, float oz, float dx, float dy, float dz) {
    r.ox = ox; r.oy = oy; r.oz = oz; r.dx = dx; r.dy = dy; r.dz = dz;
    r.ix = 1.f / dx; r.iy = 1.f / dy; r.iz = 1.f / dz;
    r.n0 = r.ix < 0; r.n1 = r.iy < 0; r.n2 = r.iz < 0;
    r.slow = !(absf(r.ix) < kInfinity && absf(r.iy) < kInfinity && absf(r.iz) < kInfinity);
}
// Bounds3::IntersectP(ray, invDir, dirIsNeg); also returns the final tMin.
DEV bool BoxTest(const RayCtx &r, float mnx, float mny, float mnz, float mxx, float mxy, float mxz, float tMaxRay, float *tMinOut) {
    const float k = 1 + 2 * gammaf(3);
    float tMin = ((r.n0 ? mxx : mnx) - r.ox) * r.ix;
    float tMx = ((r.n0 ? mnx : mxx) - r.ox) * r.ix;
    float tyMin = ((r.n1 ? mxy : mny) - r.oy) * r.iy;
    float tyMax = ((r.n1 ? mny : mxy) - r.oy) * r.iy;
    tMx *= k;
    tyMax *= k;
    bool hit = !(tMin > tyMax || tyMin > tMx);
    if (tyMin > tMin) tMin = tyMin;
    if (tyMax < tMx) tMx = tyMax;
    float tzMin = ((r.n2 ? mxz : mnz) - r.oz) * r.iz;
    float tzMax = ((r.n2 ? mnz : mxz) - r.oz) * r.iz;
    tzMax *= k;
    hit = hit && !(tMin > tzMax || tzMin > tMx);
    if (tzMin > tMin) tMin = tzMin;
    if (tzMax < tMx) tMx = tzMax;
    *tMinOut = tMin;
    return hit && (tMin < tMaxRay) && (tMx > 0);
}

// The same test for a ray whose reciprocal direction is finite (RayCtx::slow == false). Then no slab product is NaN (a
// finite difference times a finite factor), and without NaNs the reference's selects and compare-and-assign steps are
// minima and maxima: the near plane's product is the smaller of the two (rounding is monotone), `if (tyMin > tMin) tMin =
// tyMin` is a maximum, and the two early-outs together reject exactly the rays whose largest entry exceeds their smallest
// scaled exit (the x-y test failing implies the x-y-z test failing). Same products, same comparisons, same tMin: 29
// instructions a box instead of 42 (six selects and four compare-and-select pairs become three v_min, three v_max, one
// v_max3 and one v_min3). With a zero direction component (0 * inf = NaN when the origin lies in a slab plane) the NaN
// takes the reference's path through the comparisons, and the wave takes BoxTest.
DEV bool BoxTestFast(const RayCtx &r, float mnx, float mny, float mnz, float mxx, float mxy, float mxz, float tMaxRay, float *tMinOut) {
    const float k = 1 + 2 * gammaf(3);
    const float ax = (mnx - r.ox) * r.ix, bx = (mxx - r.ox) * r.ix;
    const float ay = (mny - r.oy) * r.iy, by = (mxy - r.oy) * r.iy;
    const float az = (mnz - r.oz) * r.iz, bz = (mxz - r.oz) * r.iz;
    const float tMin = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(ax, bx), __builtin_fminf(ay, by)), __builtin_fminf(az, bz));
    const float tMx = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(ax, bx) * k, __builtin_fmaxf(ay, by) * k), __builtin_fmaxf(az, bz) * k);
    *tMinOut = tMin;
    return (tMin <= tMx) && (tMin < tMaxRay) && (tMx > 0);
}

// One traversal state machine step set, shared by the persistent kernel and the plain
// per-ray routine. cur >= 0: interior node to open; -2: take the next stack entry; -1: done.
struct TravState {
    int cur, sp;
};
template <bool TMIN = true>
DEV void StackPush(TravSpill &sp, int lane, int &n, int node, int meta, float tmin) {
    TravLdsT<TMIN> &lds = TravStack<TMIN>();
    if (n >= STACK_LDS + STACK_SPILL) return;   // (cannot happen: mi_pt_create bounds the depth of the tree it uploads)
    if (n < STACK_LDS) { lds.node[n][lane] = node; lds.meta[n][lane] = meta; if (TMIN) lds.tmin[n][lane] = tmin; }
    else {
        // keep the LDS and the scratch path apart: merged into one store through a selected
        // generic pointer, hipcc 7.2 emits an illegal address-space test for gfx950
        sp.node[n - STACK_LDS] = node; sp.meta[n - STACK_LDS] = meta; sp.tmin[n - STACK_LDS] = tmin;
        asm volatile("" ::: "memory");
    }
    ++n;
}
template <bool TMIN = true>
DEV void StackPop(TravSpill &sp, int lane, int &n, int *node, int *meta, float *tmin) {
    TravLdsT<TMIN> &lds = TravStack<TMIN>();
    --n;
    if (n < STACK_LDS) { *node = lds.node[n][lane]; *meta = lds.meta[n][lane]; *tmin = TMIN ? lds.tmin[n][lane] : 0.f; }
    else {
        int nd = sp.node[n - STACK_LDS], mt = sp.meta[n - STACK_LDS];
        float tm = sp.tmin[n - STACK_LDS];
        asm volatile("" : "+v"(nd), "+v"(mt), "+v"(tm));  // pins the scratch loads in this branch
        *node = nd; *meta = mt; *tmin = tm;
    }
}
// ---- where a wide-4 record's hit children go (OpenNode<4>). `perm` holds the slot visited k-th at bits 2k..2k+1 and `hm`
// the slots whose boxes are hit. The first hit slot in visiting order is taken; the others go to the stack so that they pop
// in that order: the last visited lowest. So the place of a slot above the stack pointer is the number of hit slots visited
// AFTER it -- its rank --, which needs no other slot's values: the slots after slot s are a function of `perm` alone (four
// 4-bit masks, LaterMasks), the rank is a population count, and the slot whose rank is the highest is the one taken.
constexpr unsigned ANY_HIT_PERM = 0xE4u;   // the record's own order: slot k is visited k-th
constexpr unsigned LaterMasks(unsigned perm) {   // bits 4s..4s+3: the slots visited after slot s
    unsigned m = 0;
    for (int k = 0; k < 4; ++k) {
        unsigned later = 0;
        for (int j = k + 1; j < 4; ++j) later |= 1u << ((perm >> (2 * j)) & 3u);
        m |= later << (4 * ((perm >> (2 * k)) & 3u));
    }
    return m;
}
constexpr unsigned PermOf(unsigned laterMasks) {   // the order byte again: the slot with 3 - k slots after it is visited k-th
    unsigned perm = 0;
    for (int s = 1; s < 4; ++s) perm |= (unsigned)s << (2 * (3 - __builtin_popcount((laterMasks >> (4 * s)) & 0xfu)));
    return perm;
}
constexpr int RankOf(unsigned laterMasks, unsigned hm, int s) { return __builtin_popcount(hm & (laterMasks >> (4 * s)) & 0xfu); }
constexpr int RankOfAnyHit(unsigned hm, int s) { return __builtin_popcount((hm & 0xfu) >> (s + 1)); }   // = RankOf(LaterMasks(ANY_HIT_PERM), hm, s)
// A compile-time model of both formulations: the slot taken (-1: none) and the slots the stack receives, lowest first.
struct PushModel {
    int taken = -1, n = 0;
    int at[4] = {-1, -1, -1, -1};
};
constexpr PushModel ModelPushLoop(unsigned perm, unsigned hm) {   // the sequential loop (OpenNode's PushInOrder)
    PushModel m;
    for (int k = 3; k >= 0; --k) {
        const int sl = (int)((perm >> (2 * k)) & 3u);
        if ((hm >> sl) & 1u) {
            if (m.taken >= 0) m.at[m.n++] = m.taken;
            m.taken = sl;
        }
    }
    return m;
}
constexpr PushModel ModelPushRank(unsigned perm, unsigned hm, bool anyHit) {   // the rank stores
    PushModel m;
    const int top = __builtin_popcount(hm) - 1;
    for (int s = 0; s < 4; ++s) {
        if (!((hm >> s) & 1u)) continue;
        const int rank = anyHit ? RankOfAnyHit(hm, s) : RankOf(LaterMasks(perm), hm, s);
        if (rank == top) m.taken = s;
        else m.at[rank] = s;
    }
    m.n = top > 0 ? top : 0;
    return m;
}
constexpr bool IsSlotPermutation(unsigned perm) {
    unsigned seen = 0;
    for (int k = 0; k < 4; ++k) seen |= 1u << ((perm >> (2 * k)) & 3u);
    return seen == 0xfu;
}
constexpr bool PushModelsAgree(bool anyHit) {
    int perms = 0;
    for (unsigned perm = 0; perm < 256; ++perm) {
        if (anyHit ? perm != ANY_HIT_PERM : !IsSlotPermutation(perm)) continue;
        ++perms;
        if (PermOf(LaterMasks(perm)) != perm) return false;
        for (unsigned hm = 0; hm < 16; ++hm) {
            const PushModel a = ModelPushLoop(perm, hm), b = ModelPushRank(perm, hm, anyHit);
            if (a.taken != b.taken || a.n != b.n) return false;
            for (int i = 0; i < 4; ++i) if (a.at[i] != b.at[i]) return false;
        }
    }
    return perms == (anyHit ? 1 : 24);
}
static_assert(PushModelsAgree(false), "closest hit: for the 24 visiting orders x 16 hit masks the rank stores leave the slot taken and the stack as the sequential loop does");
static_assert(PushModelsAgree(true), "any hit (the record's own order): the rank stores leave the slot taken and the stack as the sequential loop does");
// The closest-hit kernels read a record's four masks from a table in LDS (256 x 16 bits, filled at kernel entry by
// FillLaterTable, thread t entry t): one ds_read as soon as the order byte is known, ahead of the box arithmetic.
DEV unsigned short (&LaterTable())[256] {
    __shared__ unsigned short table[256];
    return table;
}
DEV void FillLaterTable() {
    static_assert(BLOCK >= 256, "one thread per entry of the table");
    if (threadIdx.x < 256) LaterTable()[threadIdx.x] = (unsigned short)LaterMasks(threadIdx.x);
    __syncthreads();
}
// What each lane of k_trav pushed (mi_pt_trav_stack_stats): [0] entries in all, [1] entries at places beyond the stack's LDS
// part. A word per lane and count in LDS, added to without a result (k_trav's hot instances have no register to spare for
// them); the kernel clears its lanes' words at entry and adds them to the statistics once, at its end.
DEV unsigned (&PushCounts())[2][BLOCK] {
    __shared__ unsigned counts[2][BLOCK];
    return counts;
}
template <bool COUNTED>
DEV void CountPushes(int lane, int which, unsigned n) {
    if constexpr (COUNTED) __hip_atomic_fetch_add(&PushCounts()[which][lane], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Open interior node `cur`: test its children's boxes, take the first one hit in the reference's visiting order, push the
// others (with their entry distances) so that they pop in that order. Returns whether a child was taken.
//
// W = 2: a record per BVH2 interior node (both children's boxes). W = 4: a record per two-level subtree of the BVH2 -- the
// boxes of up to four grandchildren (a child that is a leaf stands for itself) and, for each of the 8 sign combinations of
// the ray direction, the order in which the reference's traversal would reach them (near child first at the subtree's
// root by its split axis, then near grandchild first inside each child by the child's axis; bvh.cpp:686-692). The child's
// own box is not tested: a ray that hits a grandchild's box hits the child's box (it contains it, and the slab arithmetic
// is monotone), and the entry-distance re-validation at pop time is the only tMax-dependent part of the test. So the lane
// enters the same leaves in the same order against the same tMax as the BVH2 traversal -- closest hits, equal-t ties and
// the count of primitive tests are unchanged -- with half the dependent node fetches per ray.
//
// The pushes of a W = 4 record (KTRAV: the caller is k_trav, which filled LaterTable and keeps PushCounts; the per-ray routines
// compute the masks in registers and count nothing).
// A lane whose entries all stay inside the stack's LDS part -- sp + hit children - 1 <= STACK_LDS -- stores each hit slot that
// is not the one taken at the place its rank gives: predicated LDS stores from the slot's own registers, one depth test and
// one update of sp per record. A lane that would cross into TravSpill takes the sequential loop (StackPush with its two store
// paths); a wave pays for both only in passes where one of its lanes is that deep. Either way the stack holds the same
// entries at the same places (PushModelsAgree).
template <int W, bool TMIN = true, bool FAST = false, bool KTRAV = false>
DEV bool OpenNode(const float4 *__restrict__ wnodes, int cur, const RayCtx &r, float tMax, TravSpill &spill, int lane, int &sp,
                  int *tkChild, int *tkMeta, unsigned &nodeCount) {
    if constexpr (W == 2) {
        const float4 a = wnodes[4 * cur], b = wnodes[4 * cur + 1], c = wnodes[4 * cur + 2];
        const float4 dd = wnodes[4 * cur + 3];
        const int childL = __float_as_int(dd.x), childR = __float_as_int(dd.y);
        const int metaL = __float_as_int(dd.z), metaR = __float_as_int(dd.w);
        const bool haveR = (metaR & 0xffff) != 0xffff;
        float tL, tR = 0;
        const bool hitL = BoxTest(r, a.x, a.y, a.z, a.w, b.x, b.y, tMax, &tL);
        const bool hitR = haveR && BoxTest(r, b.z, b.w, c.x, c.y, c.z, c.w, tMax, &tR);
        nodeCount += haveR ? 2 : 0;
        const int axis = (metaL >> 16) & 0xff;
        const bool negAxis = (axis == 0) ? r.n0 : ((axis == 1) ? r.n1 : r.n2);
        // near child first (bvh.cpp:686-692): left unless the ray runs against the split axis
        const bool hitF = negAxis ? hitR : hitL, hitS = negAxis ? hitL : hitR;
        const int chF = negAxis ? childR : childL, chS = negAxis ? childL : childR;
        const int mtF = (negAxis ? metaR : metaL) & 0xffff, mtS = (negAxis ? metaL : metaR) & 0xffff;
        const float tS = negAxis ? tL : tR;
        if (hitF) {
            *tkChild = chF; *tkMeta = mtF;
            if (hitS) {
                CountPushes<KTRAV>(lane, 0, 1u);
                if (sp >= STACK_LDS) CountPushes<KTRAV>(lane, 1, 1u);
                StackPush<TMIN>(spill, lane, sp, chS, mtS, tS);
            }
            return true;
        }
        if (hitS) { *tkChild = chS; *tkMeta = mtS; return true; }
        return false;
    } else {
        const float4 *__restrict__ n = wnodes + 8 * (size_t)cur;
        const float4 q0 = n[0], q1 = n[1], q2 = n[2], q3 = n[3], q4 = n[4], q5 = n[5], q6 = n[6], q7 = n[7];
        const unsigned c01 = __float_as_uint(q7.x), c23 = __float_as_uint(q7.y);
        const int cnt0 = (int)(c01 & 0xffffu), cnt1 = (int)(c01 >> 16), cnt2 = (int)(c23 & 0xffffu), cnt3 = (int)(c23 >> 16);
        const bool have1 = cnt1 != 0xffff, have2 = cnt2 != 0xffff, have3 = cnt3 != 0xffff;
        // (an any-hit ray -- TMIN = false -- may take the children in any order: whether something occludes it does not
        // depend on it, so it takes them as they lie in the record and skips the octant's visiting order: shadow launches -6 %)
        // The octant's order byte is taken out of the record here, once, while q7 is in registers, and its masks are asked
        // for at once: both are in hand when the box tests are through.
        unsigned later = 0;
        if constexpr (TMIN) {
            const int oct = r.Octant();
            const unsigned ordWord = (oct & 4) ? __float_as_uint(q7.w) : __float_as_uint(q7.z);
            unsigned perm = (ordWord >> (8 * (oct & 3))) & 0xffu;
            asm volatile("" : "+v"(perm));   // (pins the byte: otherwise the order word is loaded again behind the box tests)
            if constexpr (KTRAV) later = LaterTable()[perm];
            else later = LaterMasks(perm);
        }
        float t0, t1 = 0, t2 = 0, t3 = 0;
        bool h0, h1, h2, h3;
        if constexpr (FAST) {   // (every walking lane's reciprocal direction is finite: the caller asked the wave)
            h0 = BoxTestFast(r, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, tMax, &t0);
            h1 = BoxTestFast(r, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, tMax, &t1) && have1;
            h2 = BoxTestFast(r, q3.x, q3.y, q3.z, q3.w, q4.x, q4.y, tMax, &t2) && have2;
            h3 = BoxTestFast(r, q4.z, q4.w, q5.x, q5.y, q5.z, q5.w, tMax, &t3) && have3;
        } else {
            h0 = BoxTest(r, q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, tMax, &t0);
            h1 = have1 && BoxTest(r, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, tMax, &t1);
            h2 = have2 && BoxTest(r, q3.x, q3.y, q3.z, q3.w, q4.x, q4.y, tMax, &t2);
            h3 = have3 && BoxTest(r, q4.z, q4.w, q5.x, q5.y, q5.z, q5.w, tMax, &t3);
        }
        nodeCount += 1u + (have1 ? 1u : 0u) + (have2 ? 1u : 0u) + (have3 ? 1u : 0u);
        const unsigned hm = (h0 ? 1u : 0u) | (h1 ? 2u : 0u) | (h2 ? 4u : 0u) | (h3 ? 8u : 0u);
        if constexpr (TMIN && KTRAV) asm volatile("" : "+v"(later));   // (the table read is issued above, not in the branch below)
        if (hm == 0u) return false;
        const int l0 = __float_as_int(q6.x), l1 = __float_as_int(q6.y), l2 = __float_as_int(q6.z), l3 = __float_as_int(q6.w);
        const int top = __builtin_popcount(hm) - 1;   // entries to push
        CountPushes<KTRAV>(lane, 0, (unsigned)top);
        if (sp + top <= STACK_LDS) {
            const int k0 = TMIN ? RankOf(later, hm, 0) : RankOfAnyHit(hm, 0), k1 = TMIN ? RankOf(later, hm, 1) : RankOfAnyHit(hm, 1);
            const int k2 = TMIN ? RankOf(later, hm, 2) : RankOfAnyHit(hm, 2), k3 = TMIN ? RankOf(later, hm, 3) : RankOfAnyHit(hm, 3);
            TravLdsT<TMIN> &lds = TravStack<TMIN>();
            int *nodeAt = &lds.node[sp][lane], *metaAt = &lds.meta[sp][lane];   // place `sp` of the lane; rank k lies k rows above
            float *tminAt = &lds.tmin[TMIN ? sp : 0][lane];
            if (h0 && k0 != top) { nodeAt[k0 * BLOCK] = l0; metaAt[k0 * BLOCK] = cnt0; if constexpr (TMIN) tminAt[k0 * BLOCK] = t0; }
            if (h1 && k1 != top) { nodeAt[k1 * BLOCK] = l1; metaAt[k1 * BLOCK] = cnt1; if constexpr (TMIN) tminAt[k1 * BLOCK] = t1; }
            if (h2 && k2 != top) { nodeAt[k2 * BLOCK] = l2; metaAt[k2 * BLOCK] = cnt2; if constexpr (TMIN) tminAt[k2 * BLOCK] = t2; }
            if (h3 && k3 != top) { nodeAt[k3 * BLOCK] = l3; metaAt[k3 * BLOCK] = cnt3; if constexpr (TMIN) tminAt[k3 * BLOCK] = t3; }
            sp += top;
            const bool tk0 = h0 && k0 == top, tk1 = h1 && k1 == top, tk2 = h2 && k2 == top;   // (one hit slot has the highest rank)
            *tkChild = tk0 ? l0 : (tk1 ? l1 : (tk2 ? l2 : l3));
            *tkMeta = tk0 ? cnt0 : (tk1 ? cnt1 : (tk2 ? cnt2 : cnt3));
            return true;
        }
        // PushInOrder, for a lane whose entries reach beyond the LDS part.
        // from the last visited to the first: a slot that is hit displaces the candidate found so far onto the stack, so the
        // stack receives the later ones first and the first one in order stays in hand
        CountPushes<KTRAV>(lane, 1, (unsigned)(sp + top - (sp > STACK_LDS ? sp : STACK_LDS)));
        const unsigned perm = TMIN ? PermOf(later) : ANY_HIT_PERM;   // (the masks were kept across the box tests, the byte was not)
        int cand = -1;
#pragma unroll
        for (int k = 3; k >= 0; --k) {
            const int sl = (int)((perm >> (2 * k)) & 3u);
            if ((hm >> sl) & 1u) {
                if (cand >= 0) {
                    const int lk = cand == 0 ? l0 : (cand == 1 ? l1 : (cand == 2 ? l2 : l3));
                    const int ct = cand == 0 ? cnt0 : (cand == 1 ? cnt1 : (cand == 2 ? cnt2 : cnt3));
                    const float tt = cand == 0 ? t0 : (cand == 1 ? t1 : (cand == 2 ? t2 : t3));
                    StackPush<TMIN>(spill, lane, sp, lk, ct, tt);
                }
                cand = sl;
            }
        }
        *tkChild = cand == 0 ? l0 : (cand == 1 ? l1 : (cand == 2 ? l2 : l3));
        *tkMeta = cand == 0 ? cnt0 : (cand == 1 ? cnt1 : (cand == 2 ? cnt2 : cnt3));
        return true;
    }
}

// Advance until the lane holds a leaf (returns true with leafOffset/leafCount) or the
// traversal is finished (returns false, st.cur == -1).
template <int W>
DEV bool NextLeaf(const float4 *__restrict__ wnodes, const RayCtx &r, float tMax, TravState &st, TravSpill &spill,
                  int lane, int *leafOffset, int *leafCount, unsigned &nodeCount, int floor = 0) {
    while (st.cur != -1) {
        int tkChild = 0, tkMeta = 0;
        bool got = false;
        if (st.cur >= 0) got = OpenNode<W>(wnodes, st.cur, r, tMax, spill, lane, st.sp, &tkChild, &tkMeta, nodeCount);
        while (!got && st.sp > floor) {  // a popped node is entered only if still in front of tMax
            float t;
            StackPop(spill, lane, st.sp, &tkChild, &tkMeta, &t);
            got = t < tMax;
        }
        if (!got) { st.cur = -1; return false; }
        if (tkMeta > 0) { *leafOffset = tkChild; *leafCount = tkMeta & LEAF_COUNT_MASK; st.cur = -2; return true; }
        st.cur = tkChild;
    }
    return false;
}
DEV void StartTraversal(const DScene &s, const RayCtx &r, float tMax, TravState &st, unsigned &nodeCount) {
    st.sp = 0;
    st.cur = -1;
    if (s.nNodes == 0) return;
    float t;
    ++nodeCount;
    if (BoxTest(r, s.wbMin[0], s.wbMin[1], s.wbMin[2], s.wbMax[0], s.wbMax[1], s.wbMax[2], tMax, &t)) st.cur = 0;
}

constexpr int MAX_PENDING_SPHERES = 3;

// Plain per-ray traversal with inline quadric tests (mi_pt_trace and the overflow path
// of ResolveQuadrics). TOP: the world's tree, whose leaves may hold object instances -- a TransformedPrimitive
// (primitive.cpp:78-99) takes the ray to the instance's space and traverses the object's tree with it, above the entries
// the world's traversal has on the stack (`floor`); a hit inside hands its tMax back to the world ray.
// MOTION: the scene has moving instances (the entry takes Interpolate(time)); without it the code is the static one.
template <bool ANY, int W, bool TOP, bool MOTION = false>
DEV bool TraverseTree(const DScene &s, int rootRecord, bool rootHit, const V3 &ro, const V3 &rd, float &tMax, int floor, int inst,
                      Hit *hit, unsigned &nodeCount, unsigned &triCount, float time) {
    const int lane = threadIdx.x;
    RayCtx r;
    InitRayCtx(r, ro.x, ro.y, ro.z, rd.x, rd.y, rd.z);
    TravSpill spill;
    TravState st;
    st.sp = floor;
    st.cur = rootHit ? rootRecord : -1;
    bool found = false;
    const float4 *__restrict__ primTri = s.primTri;
    int leafOffset = 0, leafCount = 0;
    while (NextLeaf<W>(s.wnodes, r, tMax, st, spill, lane, &leafOffset, &leafCount, nodeCount, floor)) {
        for (int i = 0; i < leafCount; ++i) {
            const int prim = leafOffset + i;
            const float4 v0 = primTri[3 * prim];
            const unsigned pf = __float_as_uint(v0.w);
            if constexpr (TOP && W == 4) {
                if (pf & PRIM_FLAG_INSTANCE) {
                    const int k = __float_as_int(primTri[3 * prim + 1].w);
                    Ray ir;   // Inverse(InstanceToWorld)(r), at the ray's time
                    if constexpr (MOTION) {
                        float w2i[16];
                        InstanceW2I(s, k, time, w2i);
                        ir = XfRay(w2i, Ray(ro, rd, tMax));
                    } else
                        ir = XfRay(s.instances[k].w2i, Ray(ro, rd, tMax));
                    RayCtx rc;
                    InitRayCtx(rc, ir.o.x, ir.o.y, ir.o.z, ir.d.x, ir.d.y, ir.d.z);
                    const float4 bMin = s.instRootBounds[2 * k], bMax = s.instRootBounds[2 * k + 1];
                    float tBox, tIn = ir.tMax;
                    ++nodeCount;
                    const bool boxHit = BoxTest(rc, bMin.x, bMin.y, bMin.z, bMax.x, bMax.y, bMax.z, tIn, &tBox);
                    if (TraverseTree<ANY, W, false>(s, s.instWideRoot[k], boxHit, ir.o, ir.d, tIn, st.sp, k, hit, nodeCount, triCount, time)) {
                        if (ANY) return true;
                        tMax = tIn;   // r.tMax = ray.tMax
                        found = true;
                    }
                    continue;
                }
            }
            if (pf & PRIM_FLAG_SPHERE) {   // tested where it is met, against the tMax of that moment (the reference's order)
                const int sph = __float_as_int(primTri[3 * prim + 1].w);
                float t;
                if (QuadricHitT(s, sph, ro, rd, tMax, &t)) {
                    if (ANY) return true;
                    tMax = t;
                    hit->prim = prim; hit->t = t; hit->b0 = hit->b1 = hit->b2 = 0; hit->inst = inst;
                    found = true;
                }
                continue;
            }
            const float4 v1 = primTri[3 * prim + 1], v2 = primTri[3 * prim + 2];
            ++triCount;
            TriHit th;
            if (TriTest(V3(v0.x, v0.y, v0.z), V3(v1.x, v1.y, v1.z), V3(v2.x, v2.y, v2.z), ro, rd, tMax, &th)) {
                if ((pf & PRIM_FLAG_ALPHA) &&
                    ((pf & PRIM_FLAG_DEGENERATE) || !AlphaPass(s, __float_as_int(v1.w), th.b0, th.b1, th.b2, ANY))) continue;
                if (ANY) return true;
                if (!(pf & PRIM_FLAG_DEGENERATE)) {
                    tMax = th.t;
                    hit->prim = prim; hit->t = th.t; hit->b0 = th.b0; hit->b1 = th.b1; hit->b2 = th.b2; hit->inst = inst;
                    found = true;
                }
            }
        }
    }
    return found;
}
// INST: compiled for scenes with object instances (the nested traversal costs the calling kernel ~40 VGPRs)
template <bool ANY, int W, bool INST, bool MOTION = false>
DEV bool TraverseW(const DScene &s, const V3 &ro, const V3 &rd, float tMax, Hit *hit, unsigned &nodeCount, unsigned &triCount, float time) {
    RayCtx r;
    InitRayCtx(r, ro.x, ro.y, ro.z, rd.x, rd.y, rd.z);
    TravState st;
    StartTraversal(s, r, tMax, st, nodeCount);
    return TraverseTree<ANY, W, INST, MOTION>(s, 0, st.cur >= 0, ro, rd, tMax, 0, -1, hit, nodeCount, triCount, time);
}

template <bool ANY, bool INST, bool MOTION = false>
DEV bool Traverse(const DScene &s, const V3 &ro, const V3 &rd, float tMax, Hit *hit, unsigned &nodeCount, unsigned &triCount, float time) {
    if (s.bvhWidth == 4) return TraverseW<ANY, 4, INST, MOTION>(s, ro, rd, tMax, hit, nodeCount, triCount, time);
    return TraverseW<ANY, 2, false>(s, ro, rd, tMax, hit, nodeCount, triCount, time);
}

template <bool DISKS = true>
DEV void HitInteraction(const DScene &s, int prim, const V3 &ro, const V3 &rd, float b0, float b1, float b2, SurfaceInteraction *si);

// ------------------------------------------------------------------ persistent traversal
// One launch traverses every ray of a class (MODE 0: path rays of the alive slots, closest
// hit; 1: NEE shadow rays of shadowQ, any hit; 2: MIS rays of misQ, closest hit; 3: the same rays as visibility queries,
// see TRAV_IS_ANY, pt_pool.h; 4: the dark MIS rays of darkQ, any hit, no answer). A fixed
// grid of waves pulls rays from a device-wide cursor: lanes whose ray finished fetch a new
// one as soon as fewer than REFILL_BELOW lanes of the wave are still traversing (dynamic
// fetch), so a long ray no longer idles the other 63 lanes. Quadrics are only recorded
// (I_PEND*); k_resolve_* tests them afterwards at full lane utilisation.
#ifndef MIPT_REFILL_BELOW
#define MIPT_REFILL_BELOW 44   // (same-box A/B with the two-level records: 44 against 32, killeroo +1 %, the 10M-triangle scene +2 %)
#endif
constexpr int REFILL_BELOW = MIPT_REFILL_BELOW;
#ifndef MIPT_TRI_BATCH
#define MIPT_TRI_BATCH 16
#endif
constexpr int TRI_BATCH = MIPT_TRI_BATCH;
#ifndef MIPT_COOP_KMAX
#define MIPT_COOP_KMAX 4
#endif
static_assert(MIPT_REFILL_BELOW >= 1 && MIPT_REFILL_BELOW <= 64 && MIPT_TRI_BATCH >= 1 &&
              MIPT_TRI_BATCH <= 64 && MIPT_COOP_KMAX >= 1 && MIPT_COOP_KMAX <= 8, "traversal tuning macros out of range");
constexpr int COOP_KMAX = MIPT_COOP_KMAX;   // (triangle, ray) pairs a waiting lane hands to the wave per pass (pbrt's default leaf size)
#ifndef MIPT_TRAV_CHUNK
#define MIPT_TRAV_CHUNK 128
#endif
static_assert(MIPT_TRAV_CHUNK >= 64 && MIPT_TRAV_CHUNK <= (1 << 20), "MIPT_TRAV_CHUNK: at least a wave's worth of entries per cursor atomic");
constexpr int TRAV_CHUNK = MIPT_TRAV_CHUNK;  // work-list entries a wave reserves per cursor atomic (twice that for launches of
                                             // 8M rays and more: the cursor word takes ~88 adds/us, and 30M rays in chunks of
                                             // 128 are 234k adds -- same-box A/B: killeroo +3.7 % with 256, the 10M-triangle
                                             // scene's 6M-ray launches -1 %, so the size follows the launch)

#ifndef MIPT_TRAV_WAVES_PER_EU
#define MIPT_TRAV_WAVES_PER_EU 4
#endif
// ALPHA: the scene has meshes with alpha masks (the mask test is compiled into this instance only)
// INST: the scene has object instances (TransformedPrimitive, primitive.cpp:78-99). A lane that meets an instance in a world
// leaf pushes ONE return entry (the rest of that leaf and the world ray's tMax; meta < 0 marks it), swaps its ray for
// Inverse(InstanceToWorld)(ray) and walks the object's tree above that entry; popping the entry reloads the world ray from
// the pool and resumes the leaf -- with the instance ray's tMax if something was hit inside (`r.tMax = ray.tMax`). The
// sequence of box tests, primitive tests and tMax updates per ray is the reference's recursion unrolled.
// MOTION (with INST): the scene has moving instances -- the entry into an instance takes Interpolate(ray time) (InstanceW2I);
// the instances of scenes whose instances all stand still are compiled without that code (measured: with it behind a
// launch-uniform branch an instanced static frame cost 3.3 % more, profiles/object_motion_static_cost.jsonl).
template <int MODE, bool ALPHA, int W, bool INST = false, bool MOTION = false>
// MODE 3: the MIS rays again, as a visibility query (scenes without instances and without an alpha mask on an emitter's own mesh: DScene::misAny). The estimator
// reads one bit of a MIS ray -- is the closest hit the sampled light's shape (integrator.cpp:196-203) -- so k_shade hands
// over the span [tLo, tHi] of the ray in which that shape can be hit and the shape's primitive, and this walks the tree as the
// any-hit kernel does (no entry distances, no child ordering, five blocks per CU) with Triangle::Intersect's acceptance
// rules: a primitive other than the light's that is accepted below tLo ends the ray (occluded whatever the visiting order);
// one accepted inside the span only marks the ray ambiguous (the outcome depends on the order in which the reference meets
// the two), and an ambiguous ray, or one that met a quadric, is traversed again by the reference-order routine
// (k_resolve_overflow). Rays towards the environment light, and the dark rays, whose answer nothing reads (MIS_EXCL_DARK),
// carry tLo = tHi = infinity: any hit ends them. A dark ray is traced and counted like any other -- by this kernel or by
// MODE 2, whichever the scene uses -- but it writes nothing at its slot: its answer is MIS_ANSWER_DARK.
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu((TRAV_IS_ANY(MODE) && !ALPHA) ? MIPT_TRAV_WAVES_PER_EU_ANY : MIPT_TRAV_WAVES_PER_EU, (TRAV_IS_ANY(MODE) && !ALPHA) ? MIPT_TRAV_WAVES_PER_EU_ANY : MIPT_TRAV_WAVES_PER_EU)))
k_trav(DScene s, Pool pool, DevCounters *ctr) {
    constexpr bool ANY = TRAV_IS_ANY(MODE);
    constexpr bool PSEM = (MODE == 1);      // Triangle::IntersectP's acceptance rules (MODE 3 asks with Intersect's)
    constexpr bool MISANY = (MODE == 3);
    constexpr bool DARK = (MODE == 4);      // the dark MIS rays of Pool::darkQ: MODE 3's walk for tLo = tHi = infinity and no light primitive, no answer
    constexpr int QM = (MISANY || DARK) ? 2 : MODE;   // the queue and cursor of the class (DARK: DevCounters::darkNext)
    static_assert(!((MISANY || DARK) && INST), "the visibility form of the MIS rays is not built for scenes with instances");
    int excl = -1;                          // MISANY: the sampled light's primitive. MODE 2 as well: MIS_EXCL_DARK or not
    float tLo = 0;                          // MISANY: hits accepted at or beyond it are ambiguous
    bool ambiguous = false;
    const int lane = threadIdx.x;
    const int wlane = threadIdx.x & 63;
    const unsigned nPrim = (MODE == 0) ? ctr->primCount.v : 0, nCont = (MODE == 0) ? ctr->contCount.v : 0;
    const unsigned total = (MODE == 0) ? nPrim + nCont : ((MODE == 1) ? ctr->shadowCount.v : (DARK ? ctr->darkCount.v : ctr->misCount.v));
    const uint32_t *__restrict__ queue = (MODE == 0) ? pool.extQ : ((MODE == 1) ? pool.shadowQ : (DARK ? pool.darkQ : pool.misQ));
    (void)excl; (void)tLo; (void)ambiguous;
    const unsigned travChunk = (total >= (1u << 23)) ? 2u * (unsigned)TRAV_CHUNK : (unsigned)TRAV_CHUNK;
    const float4 *__restrict__ primTri = s.primTri;
    unsigned nodeCount = 0, triCount = 0, rayCount = 0;
    PushCounts()[0][lane] = 0u; PushCounts()[1][lane] = 0u;   // (the lane's own words: no barrier)
    if constexpr (W == 4 && !ANY) FillLaterTable();
    bool has = false;
    uint32_t slot = 0;
    unsigned myEntry = 0;   // MODE 1, 2: the ray's place in its queue (the answer goes beside the queue: shadowQ[n + myEntry], misQ[n + 2 myEntry])
    RayCtx r;
    InitRayCtx(r, 0, 0, 0, 1, 1, 1);
    float tMax = 0;
    TravState st;
    st.cur = -1; st.sp = 0;
    TravSpill spill;
    int nPend = 0, hitPrim = -1;
    float hitT = 0, hitB0 = 0, hitB1 = 0, hitB2 = 0;
    int leafOff = 0, leafCnt = 0;
    bool leafSimple = false;          // the leaf in hand holds triangles only (LEAF_SIMPLE)
    __shared__ int sTask[BLOCK];      // cooperative leaf test: per wave, task -> (owner lane, position in its leaf)
    int curInst = -1, hitInst = -1;   // INST: the instance the lane is inside, and the one its closest hit so far lies in
    bool hitInCur = false;            // INST: something was hit since the lane entered curInst
    TriRay triRay;
    triRay.kz = 2; triRay.Sx = triRay.Sy = 0; triRay.Sz = 1;
    bool exhausted = false;
#ifdef MIPT_TRAV_STATS
    unsigned long long dbgPasses = 0, dbgHas = 0, dbgWalk = 0, dbgWalkPasses = 0, dbgTriPasses = 0, dbgTri = 0, dbgDeepPasses = 0;
#endif
    unsigned chunkNext = 0, chunkEnd = 0;  // wave-uniform: the range of the work list this wave reserved
    while (true) {
        // ---- fetch rays for idle lanes
        if (!exhausted) {
            const unsigned long long idle = __ballot(!has);
            if (idle) {
                if (chunkNext == chunkEnd) {  // the wave's private range is used up: reserve a chunk more
                    unsigned base = 0;
                    if (wlane == 0) base = atomicAdd(DARK ? &ctr->darkNext.v : &ctr->travNext[QM].v, travChunk);
                    base = __shfl(base, 0, 64);
                    chunkNext = min(base, total);
                    chunkEnd = min(base + travChunk, total);
                    if (base >= total) exhausted = true;
                }
                const unsigned first = chunkNext;
                chunkNext = min(chunkNext + (unsigned)__popcll(idle), chunkEnd);
                if (!has) {
                    const unsigned my = first + __popcll(idle & ((1ull << wlane) - 1));
                    if (my < chunkEnd) {
                        if (MODE == 0) slot = queue[(my < nPrim) ? my : pool.n - nCont + (my - nPrim)];
                        else slot = queue[my];
                        if (MODE != 0 && !DARK) myEntry = my;
                        {
                            const float4 r0 = pool.R((MODE == 0) ? R_RAY0 : ((MODE == 1) ? R_SH0 : R_MI0), slot);
                            const float4 r1 = pool.R((MODE == 0) ? R_RAY1 : ((MODE == 1) ? R_SH1 : R_MI1), slot);
                            if (MODE == 0) InitRayCtx(r, r0.x, r0.y, r0.z, r1.x, r1.y, r1.z);
                            else InitRayCtx(r, r0.x, r0.y, r0.z, r0.w, r1.x, r1.y);
                            tMax = (MODE == 0) ? r0.w : ((MODE == 1) ? 1 - kShadowEpsilon : (MISANY ? r1.z : kInfinity));   // (a dark ray's R_MI1.z is infinity as well)
                            if (MODE == 2) excl = (int)(__float_as_uint(r1.w) & MIS_EXCL_NONE);
                            if (MISANY) {   // (k_shade: R_MI1 = d.y, d.z, tHi, light primitive | width code << 27; tLo = tHi (1 - 2^-code))
                                const unsigned xw = __float_as_uint(r1.w);
                                excl = (int)(xw & MIS_EXCL_NONE);
                                const unsigned code = xw >> MIS_EXCL_BITS;
                                tLo = code == 0 ? 0.f : tMax * (1.f - __uint_as_float((127u - code) << 23));
                                ambiguous = false;
                            }
                            StartTraversal(s, r, tMax, st, nodeCount);
                            triRay = MakeTriRay(V3(r.dx, r.dy, r.dz));
                            nPend = 0; hitPrim = -1;
                            hitT = hitB0 = hitB1 = hitB2 = 0;
                            leafCnt = 0;
                            curInst = hitInst = -1; hitInCur = false;
                            ++rayCount;
                            if (st.cur >= 0) has = true;
                            else if (DARK) {}   // (counted; nothing to answer)
                            else if (MODE == 1) pool.shadowQ[pool.n + myEntry] = 0u;   // nothing to traverse: unoccluded
                            else if (MODE == 2) {
                                const bool dark = excl == (int)MIS_EXCL_DARK;
                                *reinterpret_cast<uint2 *>(pool.misQ + pool.n + 2 * (size_t)myEntry) = make_uint2(0xffffffffu, dark ? MIS_ANSWER_DARK : 0u);
                                if (!dark) pool.R(R_HIT, slot) = make_float4(0.f, 0.f, 0.f, 0.f);
                            } else if (MISANY) {
                                *reinterpret_cast<uint2 *>(pool.misQ + pool.n + 2 * (size_t)myEntry) = make_uint2(0xffffffffu, excl == (int)MIS_EXCL_DARK ? MIS_ANSWER_DARK : 0u);
                            } else {  // the ray misses the world bound: nothing to traverse
                                pool.I(I_HITPRIM, slot) = -1;
                                pool.I(I_NPEND, slot) = 0;
                                if (INST && MODE == 0) pool.I(I_HITINST, slot) = -1;
                                if (!ANY) pool.R(R_HIT, slot) = make_float4(0.f, 0.f, 0.f, 0.f);
                            }
                        }
                    }
                }
            }
        }
        if (!__any(has)) {
            if (exhausted) break;
            continue;  // every fetched slot was dead: fetch again
        }
        // ---- step the lanes until enough of them have run dry. Every pass opens one
        // interior node in each lane that holds one; lanes that reached a leaf wait, and once
        // TRI_BATCH lanes wait (or nobody is left walking) their leaves are tested -- triangles-only
        // leaves by the whole wave (cooperative test below), the others one primitive per waiting
        // lane -- so both the box code and the triangle code run on well-filled waves.
        // Per lane the sequence of node visits, pops and primitive tests is unchanged.
        while (true) {
            const bool walking = has && st.cur >= 0;
            const bool inLeaf = has && leafCnt > 0;
            const int nLeaf = __popcll(__ballot(inLeaf));
            const bool anyWalk = __any(walking);
#ifdef MIPT_TRAV_STATS
            ++dbgPasses; dbgHas += __popcll(__ballot(has)); dbgWalk += __popcll(__ballot(walking));
            if (anyWalk) ++dbgWalkPasses;
            if (nLeaf > 0 && (nLeaf >= TRI_BATCH || !anyWalk)) { ++dbgTriPasses; dbgTri += nLeaf; }
#endif
            bool needPop = false, got = false, finished = false;
            int tkChild = 0, tkMeta = 0;
            if (walking) {
                if (__any(r.slow)) got = OpenNode<W, !ANY, false, true>(s.wnodes, st.cur, r, tMax, spill, lane, st.sp, &tkChild, &tkMeta, nodeCount);
                else got = OpenNode<W, !ANY, W == 4, true>(s.wnodes, st.cur, r, tMax, spill, lane, st.sp, &tkChild, &tkMeta, nodeCount);
                needPop = !got;
                st.cur = -1;
            }
#ifdef MIPT_TRAV_STATS
            if (__any(walking && got && st.sp > STACK_LDS)) ++dbgDeepPasses;   // (a lane of the wave took the sequential pushes)
#endif
            const bool triPass = nLeaf > 0 && (nLeaf >= TRI_BATCH || !anyWalk);   // (wave-uniform)
            // ---- cooperative leaf test. A lane waiting at a triangles-only leaf hands up to COOP_KMAX of its (ray, triangle)
            // pairs to the wave: the pairs of all waiting lanes are numbered owner by owner, lane w tests pair w with the
            // owner's ray against the owner's tMax of this moment, and the owner then takes the outcome the sequential loop
            // of BVHAccel::Intersect would have reached: of the pairs that hit, in leaf order, each is accepted unless the
            // test's one tMax-dependent line (tScaled against tMax * det, triangle.cpp:262-266) rejects it with the tMax
            // left by the hit accepted before it. One pass finishes a whole leaf at the utilisation of (pairs / 64) instead
            // of one triangle per waiting lane (a fifth of the wave on the 10M-triangle scene).
            if (triPass && __any(inLeaf && leafSimple)) {
                const bool coop = inLeaf && leafSimple;
                const int want = coop ? min(leafCnt, COOP_KMAX) : 0;
                int base = 0, total = 0;
#pragma unroll
                for (int b = 0; b < COOP_KMAX; ++b) {
                    const unsigned long long m = __ballot(want > b);
                    base += __popcll(m & ((1ull << wlane) - 1));
                    total += __popcll(m);
                }
                const int grant = max(0, min(want, 64 - base));
                int *taskOwner = &sTask[threadIdx.x & ~63];
                for (int k = 0; k < grant; ++k) taskOwner[base + k] = wlane | (k << 8);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const int nTask = min(total, 64);
                const bool worker = wlane < nTask;
                const int ow = worker ? taskOwner[wlane] : wlane;
                const int owner = ow & 63, tk = ow >> 8;
                const int wOff = __shfl(leafOff, owner, 64);
                const float wox = __shfl(r.ox, owner, 64), woy = __shfl(r.oy, owner, 64), woz = __shfl(r.oz, owner, 64);
                TriRay wtr;
                wtr.kz = __shfl(triRay.kz, owner, 64);
                wtr.Sx = __shfl(triRay.Sx, owner, 64); wtr.Sy = __shfl(triRay.Sy, owner, 64); wtr.Sz = __shfl(triRay.Sz, owner, 64);
                const float wT = __shfl(tMax, owner, 64);
                const int wExcl = MISANY ? __shfl(excl, owner, 64) : -1;
                const float wLo = MISANY ? __shfl(tLo, owner, 64) : 0.f;
                bool res = false, resClear = false;
                float rT = 0, rB0 = 0, rB1 = 0, rB2 = 0, rDet = 0, rTs = 0;
                if (worker) {
                    const int prim = wOff + tk;
                    const float4 v0 = primTri[3 * prim], v1 = primTri[3 * prim + 1], v2 = primTri[3 * prim + 2];
                    const unsigned pf = __float_as_uint(v0.w);
                    TriHit th;
                    if (TriTestRay(V3(v0.x, v0.y, v0.z), V3(v1.x, v1.y, v1.z), V3(v2.x, v2.y, v2.z), V3(wox, woy, woz), wtr, wT, &th, &rDet, &rTs)) {
                        bool counts = true;
                        if constexpr (ALPHA)
                            if (pf & PRIM_FLAG_ALPHA)
                                counts = !(pf & PRIM_FLAG_DEGENERATE) && AlphaPass(s, __float_as_int(v1.w), th.b0, th.b1, th.b2, PSEM);   // (the shadow mask is IntersectP's alone, triangle.cpp:531-570)
                        res = counts && (PSEM || !(pf & PRIM_FLAG_DEGENERATE));
                        if (MISANY) { res = res && prim != wExcl; resClear = res && th.t < wLo; }
                        rT = th.t; rB0 = th.b0; rB1 = th.b1; rB2 = th.b2;
                    }
                }
                const unsigned long long hitMask = __ballot(res);
                const unsigned seg = grant > 0 ? (unsigned)(hitMask >> base) & ((1u << grant) - 1u) : 0u;   // bit k: my k-th pair hit
                if (MISANY) {
                    const unsigned long long clearMask = __ballot(resClear);
                    const unsigned segClear = grant > 0 ? (unsigned)(clearMask >> base) & ((1u << grant) - 1u) : 0u;
                    if (segClear) { hitPrim = leafOff + (__ffs(segClear) - 1); finished = true; triCount += (unsigned)__ffs(segClear); }
                    else {
#ifndef MIPT_EXP_IGNORE_AMBIGUOUS   // (mutation build: tests/test_gpu_parity.py::test_mis_rays_... must fail with it)
                        if (seg) ambiguous = true;
#endif
                        triCount += (unsigned)grant;
                    }
                } else if (ANY) {   // (DARK: MODE 3's rule with every accepted hit below tLo -- res leaves the degenerate triangles out, PSEM is off)
                    if (seg) { hitPrim = leafOff + (__ffs(seg) - 1); finished = true; triCount += (unsigned)__ffs(seg); }
                    else triCount += (unsigned)grant;
                } else {
                    int win = -1;
                    const bool multi = __popc(seg) >= 2;
                    if (__any(multi)) {   // two hits in one leaf: replay the sequence exactly
                        unsigned rem = multi ? seg : 0u;
                        float cur = tMax;
                        while (__any(rem != 0u)) {
                            const int k = rem ? (__ffs(rem) - 1) : 0;
                            const int src = rem ? base + k : wlane;
                            const float dk = __shfl(rDet, src, 64), tsk = __shfl(rTs, src, 64), tk2 = __shfl(rT, src, 64);
                            if (rem) {
                                const bool beyond = dk < 0 ? (tsk < cur * dk) : (tsk > cur * dk);
                                if (!beyond) { cur = tk2; win = k; }
                                rem &= rem - 1u;
                            }
                        }
                    }
                    if (!multi && seg) win = __ffs(seg) - 1;
                    const int src = win >= 0 ? base + win : wlane;
                    const float hT = __shfl(rT, src, 64), hB0 = __shfl(rB0, src, 64), hB1 = __shfl(rB1, src, 64), hB2 = __shfl(rB2, src, 64);
                    if (win >= 0) {
                        tMax = hT;
                        hitPrim = leafOff + win; hitT = hT; hitB0 = hB0; hitB1 = hB1; hitB2 = hB2;
                        if (INST) { hitInst = curInst; hitInCur = true; }
                    }
                    triCount += (unsigned)grant;
                }
                if (grant > 0) {
                    leafOff += grant; leafCnt -= grant;
                    needPop = !finished && leafCnt == 0;
                }
            }
            if (triPass && inLeaf && !leafSimple) {
                const int prim = leafOff;
                ++leafOff; --leafCnt;
                const float4 v0 = primTri[3 * prim];
                const unsigned pf = __float_as_uint(v0.w);
                bool entered = false;
                if (INST && (pf & PRIM_FLAG_INSTANCE)) {
                    // TransformedPrimitive::Intersect[P]: the ray in the instance's space, then the object's BVH from its root
                    const int k = __float_as_int(primTri[3 * prim + 1].w);
                    CountPushes<true>(lane, 0, 1u);
                    if (st.sp >= STACK_LDS) CountPushes<true>(lane, 1, 1u);
                    StackPush<!ANY>(spill, lane, st.sp, leafOff, -(leafCnt + 1), tMax);
                    Ray ir;
                    if constexpr (MOTION) {
                        float w2i[16];   // (a moving instance: the slot's ray time, read here alone)
                        InstanceW2I(s, k, PathTime(s, pool, slot), w2i);
                        ir = XfRay(w2i, Ray(V3(r.ox, r.oy, r.oz), V3(r.dx, r.dy, r.dz), tMax));
                    } else
                        ir = XfRay(s.instances[k].w2i, Ray(V3(r.ox, r.oy, r.oz), V3(r.dx, r.dy, r.dz), tMax));
                    InitRayCtx(r, ir.o.x, ir.o.y, ir.o.z, ir.d.x, ir.d.y, ir.d.z);
                    triRay = MakeTriRay(ir.d);
                    tMax = ir.tMax;
                    curInst = k; hitInCur = false;
                    leafCnt = 0;
                    const float4 bMin = s.instRootBounds[2 * k], bMax = s.instRootBounds[2 * k + 1];
                    float tBox;
                    ++nodeCount;
                    got = BoxTest(r, bMin.x, bMin.y, bMin.z, bMax.x, bMax.y, bMax.z, tMax, &tBox);
                    tkChild = s.instWideRoot[k]; tkMeta = 0;
                    entered = true;
                } else if (INST && curInst >= 0 && (pf & PRIM_FLAG_SPHERE)) {
                    // a quadric of an instanced object: tested where it is met, with the instance's ray
                    float t;
                    if (QuadricHitT(s, __float_as_int(primTri[3 * prim + 1].w), V3(r.ox, r.oy, r.oz), V3(r.dx, r.dy, r.dz), tMax, &t)) {
                        if (ANY) { hitPrim = prim; finished = true; }
                        else { tMax = t; hitPrim = prim; hitT = t; hitB0 = hitB1 = hitB2 = 0; hitInst = curInst; hitInCur = true; }
                    }
                } else
                if (MISANY && prim == excl) {}   // the sampled light's own shape
                else if ((MODE >= 2) && (pf & PRIM_FLAG_SPHERE) && (DARK || excl == (int)MIS_EXCL_DARK)) {}   // (a dark ray's quadrics: nothing resolves them)
                else if (pf & PRIM_FLAG_SPHERE) {
                    if ((nPend & 0xff) < MAX_PEND) {
                        pool.I(I_PEND0 + (nPend & 0xff), slot) = prim;
                        if (!ANY) pool.F(P_TENC0 + (nPend & 0xff), slot) = tMax;   // (see ResolveQuadrics)
                        ++nPend;
                    }
                    else nPend |= PEND_OVERFLOW;
                } else {
                    const float4 v1 = primTri[3 * prim + 1], v2 = primTri[3 * prim + 2];
                    ++triCount;
                    TriHit th;
                    if (TriTestRay(V3(v0.x, v0.y, v0.z), V3(v1.x, v1.y, v1.z), V3(v2.x, v2.y, v2.z), V3(r.ox, r.oy, r.oz),
                                   triRay, tMax, &th)) {
                        // meshes with an alpha mask: IntersectP then rejects degenerate triangles too, and both reject
                        // hits where the mask is 0 (triangle.cpp:331-338, 531-570)
                        bool counts = true;
                        if constexpr (ALPHA)
                            if (pf & PRIM_FLAG_ALPHA)
                                counts = !(pf & PRIM_FLAG_DEGENERATE) && AlphaPass(s, __float_as_int(v1.w), th.b0, th.b1, th.b2, PSEM);   // (the shadow mask is IntersectP's alone, triangle.cpp:531-570)
                        if (!counts) {}
                        else if (PSEM) { hitPrim = prim; finished = true; }
                        else if (DARK) { if (!(pf & PRIM_FLAG_DEGENERATE)) { hitPrim = prim; finished = true; } }   // (MODE 3 with tLo = infinity)
                        else if (MISANY) {
                            if (!(pf & PRIM_FLAG_DEGENERATE)) {
                                if (th.t < tLo) { hitPrim = prim; finished = true; }
                                else ambiguous = true;
                            }
                        }
                        else if (!(pf & PRIM_FLAG_DEGENERATE)) {
                            tMax = th.t;
                            hitPrim = prim; hitT = th.t; hitB0 = th.b0; hitB1 = th.b1; hitB2 = th.b2;
                            if (INST) { hitInst = curInst; hitInCur = true; }
                        }
                    }
                }
                needPop = entered ? !got : (!finished && leafCnt == 0);
            }
            if (needPop) {  // a popped node is entered only if still in front of tMax
                while (!got && st.sp > 0) {
                    float t;
                    StackPop<!ANY>(spill, lane, st.sp, &tkChild, &tkMeta, &t);
                    if (INST && tkMeta < 0) {   // back from the instance: the world ray again, and the rest of the leaf
                        const float4 r0 = pool.R((MODE == 0) ? R_RAY0 : ((MODE == 1) ? R_SH0 : R_MI0), slot);
                        const float4 r1 = pool.R((MODE == 0) ? R_RAY1 : ((MODE == 1) ? R_SH1 : R_MI1), slot);
                        if (MODE == 0) InitRayCtx(r, r0.x, r0.y, r0.z, r1.x, r1.y, r1.z);
                        else InitRayCtx(r, r0.x, r0.y, r0.z, r0.w, r1.x, r1.y);
                        triRay = MakeTriRay(V3(r.dx, r.dy, r.dz));
                        if (!hitInCur) tMax = ANY ? 1 - kShadowEpsilon : t;   // (a hit inside: r.tMax = ray.tMax; any-hit: no entry distances are kept)
                        curInst = -1;
                        tkMeta = -tkMeta - 1;      // primitives left in the world leaf
                        got = tkMeta > 0;
                        continue;
                    }
                    got = ANY || t < tMax;
                }
                finished = !got;
            }
            if (got) {
                if (tkMeta > 0) { leafOff = tkChild; leafCnt = tkMeta & LEAF_COUNT_MASK; leafSimple = (tkMeta & LEAF_SIMPLE) != 0; }
                else st.cur = tkChild;
            }
            if (finished && DARK) {   // no answer, nothing at the slot
                has = false;
                leafCnt = 0;
            } else
            if (finished && MODE == 1) {
                pool.shadowQ[pool.n + myEntry] = (hitPrim >= 0 ? 0x80000000u : 0u) | (unsigned)nPend;
                has = false;
                leafCnt = 0;
            } else
            if (finished && MODE == 2) {
                const bool dark = excl == (int)MIS_EXCL_DARK;
                *reinterpret_cast<uint2 *>(pool.misQ + pool.n + 2 * (size_t)myEntry) = make_uint2((unsigned)hitPrim, dark ? MIS_ANSWER_DARK : (unsigned)nPend);
                if (!dark) pool.R(R_HIT, slot) = make_float4(hitT, hitB0, hitB1, hitB2);
                has = false;
                leafCnt = 0;
            } else
            if (finished && MISANY) {   // an occluder's primitive, -1: nothing in front of the light's span, -2: ambiguous
                *reinterpret_cast<uint2 *>(pool.misQ + pool.n + 2 * (size_t)myEntry) = make_uint2(hitPrim >= 0 ? (unsigned)hitPrim : (ambiguous ? 0xfffffffeu : 0xffffffffu), excl == (int)MIS_EXCL_DARK ? MIS_ANSWER_DARK : (unsigned)nPend);
                has = false;
                leafCnt = 0;
            } else
            if (finished) {
                pool.I(I_HITPRIM, slot) = hitPrim;
                pool.I(I_NPEND, slot) = nPend;
                if (!ANY) pool.R(R_HIT, slot) = make_float4(hitT, hitB0, hitB1, hitB2);
                if (INST && MODE == 0) pool.I(I_HITINST, slot) = hitInst;
                has = false;
                leafCnt = 0;
            }
            const int active = __popcll(__ballot(has));
            if (active == 0 || (!exhausted && active < REFILL_BELOW)) break;
        }
    }
#ifdef MIPT_TRAV_STATS
    if (blockIdx.x == 7 && threadIdx.x == 0 && total > 1000000)
        printf("TRAVSTAT mode %d total %u passes %llu has/pass %.1f walkPasses %llu walk/walkPass %.1f triPasses %llu tri/triPass %.1f deepPushPasses %llu\n", MODE, total, dbgPasses,
               (double)dbgHas / dbgPasses, dbgWalkPasses, (double)dbgWalk / (dbgWalkPasses ? dbgWalkPasses : 1), dbgTriPasses, (double)dbgTri / (dbgTriPasses ? dbgTriPasses : 1), dbgDeepPasses);
#endif
    DevStats &st8 = Stats(ctr);
    if (MODE == 1) CountAdd(&st8.shadowRays, rayCount);
    else CountAdd(&st8.regularRays, rayCount);
    CountAdd(&st8.nodesVisited, nodeCount);
    CountAdd(&st8.triTests, triCount);
    CountAdd(&st8.stackPushed, PushCounts()[0][lane]);
    CountAdd(&st8.stackBeyondLds, PushCounts()[1][lane]);
    if (MODE == 0) { CountAdd(&st8.extendNodes, nodeCount); CountAdd(&st8.extendTris, triCount); CountAdd(&st8.extendRays, rayCount); }
    if (DARK) {   // (mi_pt_dark_launch_stats: what the launch found in its queue against what it traced)
        CountAdd(&st8.darkRays, rayCount);
        if (blockIdx.x == 0 && threadIdx.x == 0 && total) atomicAdd(&st8.darkEntries, (unsigned long long)total);
    }
}

// Quadrics recorded by k_trav, tested after the triangles at full lane utilisation -- with the outcome of the reference's
// order. Sphere::Intersect rejects a root whose error-bounded UPPER end lies beyond tMax (sphere.cpp:77-82), so when a
// triangle and a sphere are met within that error bound of each other (a sphere resting on a quad: fuzz scene 2004), which
// one is the hit depends on which was met first. So each postponed quadric keeps the ray's tMax of the moment it was met
// (P_TENC*), and this replays the reference's sequence: quadric j is tested against min(that tMax, the closest quadric
// accepted before it); a triangle hit that the traversal found AFTER the last accepted quadric survives only if it is
// closer than that quadric. (Shadow rays: tMax never changes, the order does not matter.) On overflow the ray is
// re-traversed by the reference-order routine with inline quadric tests (Retraverse), in k_resolve_overflow alone: the
// resolve kernels proper are compiled without it (it cost them 40-56 VGPRs and all but 650 of 12 000 instructions).
template <bool ANY>
DEV bool ResolveQuadrics(const DScene &s, const Pool &pool, uint32_t slot, const V3 &ro, const V3 &rd, float tMaxIn, Hit *h, bool foundTri, int np) {
    if (ANY) {
        for (int j = 0; j < (np & 0xff); ++j) {
            const int prim = pool.I(I_PEND0 + j, slot);
            float t;
            if (QuadricHitT(s, __float_as_int(s.primTri[3 * prim + 1].w), ro, rd, tMaxIn, &t)) return true;
        }
        return foundTri;
    }
    float tBest = kInfinity, tEncBest = 0.f;
    int primBest = -1;
    for (int j = 0; j < (np & 0xff); ++j) {
        const int prim = pool.I(I_PEND0 + j, slot);
        const float tEnc = pool.F(P_TENC0 + j, slot);
        float t;
        if (QuadricHitT(s, __float_as_int(s.primTri[3 * prim + 1].w), ro, rd, minf(tEnc, tBest), &t)) { tBest = t; primBest = prim; tEncBest = tEnc; }
    }
    if (primBest < 0) return foundTri;
    if (foundTri && tEncBest > h->t && h->t <= tBest) return true;   // the triangle was found later, and in front of the quadric
    h->prim = primBest; h->t = tBest; h->b0 = h->b1 = h->b2 = 0; h->inst = -1;
    return true;
}
// (*h is written only when something is hit)
template <bool ANY, bool INST, bool MOTION = false>
DEV bool Retraverse(const DScene &s, const V3 &ro, const V3 &rd, float tMax, Hit *h, float time) {
    Hit h2;
    h2.prim = -1; h2.t = 0; h2.b0 = h2.b1 = h2.b2 = 0;
    unsigned n2 = 0, t2 = 0;  // statistics were already counted by k_trav
    const bool found = Traverse<ANY, INST, MOTION>(s, ro, rd, tMax, &h2, n2, t2, time);
    if (found) *h = h2;
    return found;
}

// A shadow or MIS ray in its two records: origin, direction (r1.z: the end of the light's span, MIS rays only)
DEV V3 PackedRayO(const float4 &r0) { return V3(r0.x, r0.y, r0.z); }
DEV V3 PackedRayD(const float4 &r0, const float4 &r1) { return V3(r0.w, r1.x, r1.y); }
// Hit <-> the R_HIT record
DEV float4 HitRecord(const Hit &h) { return make_float4(h.t, h.b0, h.b1, h.b2); }
DEV void SetHitRecord(Hit *h, const float4 &hr) { h->t = hr.x; h->b0 = hr.y; h->b1 = hr.z; h->b2 = hr.w; }
// The shading class of a hit primitive (mi_pt_create packs it into primTri[3 * prim].w); a miss has a class of its own.
DEV int ClassOfPrim(const float4 *__restrict__ primTri, int prim) {
    return (prim >= 0) ? (int)((__float_as_uint(primTri[3 * prim].w) >> PRIM_CLASS_SHIFT) & (unsigned)(MAX_CLASSES - 1)) : MISS_CLASS;
}

// A vertex at which the path ends with nothing to shade and no emitted light to look up (path.cpp:91-101 looks for emitted
// light only at the camera ray's vertex and after a specular bounce): the ray escaped and there is no environment light or
// no look-up is owed, or it hit something at the depth limit and no look-up is owed. A third of killeroo's path rays end so:
// the resolve step finishes their slots itself (FinishedWord) and the shading queues never see them.
DEV bool EndsUnshaded(int word, int prim, int maxDepth, int nInfiniteLights) {
    const int bounces = StateBounces(word);
    const bool emitCheck = bounces == 0 || (word & F_SPECULAR);
    return prim < 0 ? (!emitCheck || nInfiniteLights == 0) : (bounces >= maxDepth && !emitCheck);
}
// The state word of a path that ends with no estimate pending: which line holds L and what is still implicit are carried
// over, bounces (ReportValue(pathLength, bounces)) and the sampler dimension stay.
DEV int FinishedWord(int word) { return StateWord(F_FINISHED | (word & (F_L_IN_B | F_L_ZERO | F_BETA_ONE)), StateBounces(word), StateDim(word)); }

// The per-(chunk, wave) counts of a block, cnt[(ch * BLOCK / 64 + w) * stride], become their exclusive prefix in place; returns
// the total, which the caller reserves on its queue cursor in one add. Run by one thread between two barriers.
DEV unsigned ChunkWavePrefix(unsigned *cnt, int stride) {
    unsigned tot = 0;
    for (int ch = 0; ch < SLOT_CHUNKS; ++ch)
        for (int w = 0; w < BLOCK / 64; ++w) { unsigned &e = cnt[(ch * (BLOCK / 64) + w) * stride]; const unsigned n = e; e = tot; tot += n; }
    return tot;
}

template <bool INST>
__global__ void __launch_bounds__(BLOCK) k_resolve_extend(DScene s, Pool pool, DevCounters *ctr) {
    // append to the class queues: one atomic per class and block
    __shared__ unsigned sCnt[SLOT_CHUNKS][BLOCK / 64][MAX_CLASSES], sBase[MAX_CLASSES];
    // The rays with postponed quadrics are a minority spread over the block's slots: they are listed first and resolved
    // afterwards by all lanes together, so the interval-arithmetic sphere test runs on full waves instead of on the few
    // lanes of each chunk that hold such a ray (Cornell: a seventh of the rays, the kernel 2.5x faster).
    __shared__ unsigned char sCls[SLOT_CHUNKS][BLOCK];   // per slot of the block: 0x80 | class when the slot holds a traced path
    __shared__ unsigned short sPend[SLOT_CHUNKS * BLOCK];
    __shared__ unsigned sPendCount;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned pathLen = 0;   // bounces of the paths that end here
    if (threadIdx.x == 0) sPendCount = 0;
    __syncthreads();
    const float4 *__restrict__ primTri = s.primTri;   // (by value: a reference to the kernel argument would move it to scratch)
    // ---- phase A: every slot's hit primitive; rays with a quadric list go onto the block's list
#pragma unroll 1
    for (int ch = 0; ch < SLOT_CHUNKS; ++ch) {
        const uint32_t slot = (blockIdx.x * SLOT_CHUNKS + ch) * BLOCK + threadIdx.x;
        unsigned char cc = 0;
        const int word = slot < pool.n ? pool.I(I_FLAGS, slot) : 0;
        if (word & F_ALIVE) {
            const int npend = pool.I(I_NPEND, slot);
            if (npend & PEND_OVERFLOW) pool.ovfQ[atomicAdd(&ctr->ovfCount[0].v, 1u)] = slot;   // k_resolve_overflow commits this one
            else if (npend != 0) sPend[atomicAdd(&sPendCount, 1u)] = (unsigned short)(ch * BLOCK + threadIdx.x);
            else {
                const int prim = pool.I(I_HITPRIM, slot);
                if (EndsUnshaded(word, prim, s.maxDepth, s.nInfiniteLights)) { pool.I(I_FLAGS, slot) = FinishedWord(word); pathLen += (unsigned)StateBounces(word); }
                else cc = (unsigned char)(0x80 | ClassOfPrim(primTri, prim));
            }
        }
        sCls[ch][threadIdx.x] = cc;
    }
    __syncthreads();
    // ---- phase B: the listed rays, one per lane
    const unsigned nPend = sPendCount;
#pragma unroll 1
    for (unsigned i = threadIdx.x; i < nPend; i += BLOCK) {
        const unsigned e = sPend[i];
        const uint32_t slot = blockIdx.x * SLOT_CHUNKS * BLOCK + e;
        int prim = pool.I(I_HITPRIM, slot);
        const float4 r0 = pool.R(R_RAY0, slot), r1 = pool.R(R_RAY1, slot), hr = pool.R(R_HIT, slot);
        V3 ro(r0.x, r0.y, r0.z), rd(r1.x, r1.y, r1.z);
        Hit h;
        h.prim = prim; SetHitRecord(&h, hr);
        if (INST) h.inst = pool.I(I_HITINST, slot);
        const bool found = ResolveQuadrics<false>(s, pool, slot, ro, rd, r0.w, &h, prim >= 0, pool.I(I_NPEND, slot));
        prim = found ? h.prim : -1;
        pool.I(I_HITPRIM, slot) = prim;
        pool.R(R_HIT, slot) = HitRecord(h);
        if (INST) pool.I(I_HITINST, slot) = h.inst;
        const int word = pool.I(I_FLAGS, slot);
        if (EndsUnshaded(word, prim, s.maxDepth, s.nInfiniteLights)) { pool.I(I_FLAGS, slot) = FinishedWord(word); pathLen += (unsigned)StateBounces(word); }   // (sCls stays 0)
        else sCls[e / BLOCK][e % BLOCK] = (unsigned char)(0x80 | ClassOfPrim(primTri, prim));
    }
    __syncthreads();
    // ---- phase C: ranks within (chunk, wave, class), the block's range of each class queue, the queue entries
    unsigned rankLo = 0, rankHi = 0;              // per chunk: 8 bits of rank within the wave and class
#pragma unroll 1
    for (int ch = 0; ch < SLOT_CHUNKS; ++ch) {
        const unsigned cc = sCls[ch][threadIdx.x];
        const bool traced = (cc & 0x80u) != 0;
        const int cls = (int)(cc & 0x7fu);
        unsigned rank = 0;
        for (int c = 0; c < MAX_CLASSES; ++c) {
            if (!((s.classMask >> c) & 1)) continue;
            const unsigned long long m = __ballot(traced && cls == c);
            if (lane == 0) sCnt[ch][wave][c] = (unsigned)__popcll(m);
            if (traced && cls == c) rank = (unsigned)__popcll(m & ((1ull << lane) - 1));
        }
        if (ch < 4) rankLo |= rank << (8 * ch); else rankHi |= rank << (8 * (ch - 4));
    }
    __syncthreads();
    if (threadIdx.x < MAX_CLASSES && ((s.classMask >> threadIdx.x) & 1)) {
        const int c = threadIdx.x;   // the block's range of queue c in one add
        const unsigned tot = ChunkWavePrefix(&sCnt[0][0][c], MAX_CLASSES);
        sBase[c] = tot ? atomicAdd(&ctr->shadeCount[c].v, tot) : 0;
    }
    __syncthreads();
#pragma unroll 1
    for (int ch = 0; ch < SLOT_CHUNKS; ++ch) {
        const unsigned cc = sCls[ch][threadIdx.x];
        if (!(cc & 0x80u)) continue;
        const int cls = (int)(cc & 0x7fu);
        const unsigned rank = ((ch < 4 ? rankLo >> (8 * ch) : rankHi >> (8 * (ch - 4))) & 255u);
        const uint32_t slot = (blockIdx.x * SLOT_CHUNKS + ch) * BLOCK + threadIdx.x;
        pool.shadeQ[(size_t)cls * pool.n + sBase[cls] + sCnt[ch][wave][cls] + rank] = slot;
    }
    CountAdd(&Stats(ctr).pathLengthSum, pathLen);
}

// A shadow ray's verdict on its slot's flags. L += contribution: the candidate line holds the sum already (F_CAND, written by
// k_shade), an unoccluded ray makes it the path's L; an occluded one leaves L where it is. With a MIS ray pending
// k_resolve_mis closes the estimate, else it ends here.
DEV int CommitShadowVerdict(int flags, bool occluded, unsigned &zero) {
    const bool added = !occluded && (flags & F_NEE_NZ);
    if (!occluded) flags = (flags ^ F_L_IN_B) & ~F_L_ZERO;
    flags &= ~(F_SHADOW | F_CAND | F_NEE_NZ);
    if (flags & F_MIS) { if (added) flags |= F_A_ADDED; }
    else { if (!added) ++zero; flags &= ~(F_NEE | F_A_ADDED); }
    return flags;
}

template <bool INST>
__global__ void __launch_bounds__(BLOCK) k_resolve_shadow(DScene s, Pool pool, DevCounters *ctr) {
    // (the grid is sized by what is resident, LaunchResolve: each block walks the queue in steps of the grid)
    const unsigned count = ctr->shadowCount.v;
    unsigned zero = 0;
    for (uint32_t qi = blockIdx.x * BLOCK + threadIdx.x; qi < count; qi += gridDim.x * BLOCK) {
        const uint32_t slot = pool.shadowQ[qi];
        const int flags = pool.I(I_FLAGS, slot);
        const unsigned verdict = pool.shadowQ[pool.n + qi];   // k_trav<1>'s answer, in queue order
        bool occluded = (verdict >> 31) != 0u;
        const int npend = occluded ? 0 : (int)(verdict & 0x7fffffffu);
        if (npend & PEND_OVERFLOW) { pool.ovfQ[(size_t)pool.n + atomicAdd(&ctr->ovfCount[1].v, 1u)] = slot; continue; }   // k_resolve_overflow commits this one
        if (npend != 0) {
            const float4 r0 = pool.R(R_SH0, slot), r1 = pool.R(R_SH1, slot);
            Hit h;
            occluded = ResolveQuadrics<true>(s, pool, slot, PackedRayO(r0), PackedRayD(r0, r1), 1 - kShadowEpsilon, &h, false, npend);
        }
        pool.I(I_FLAGS, slot) = CommitShadowVerdict(flags, occluded, zero);
    }
    CountAdd(&Stats(ctr).zeroRadiancePaths, zero);
}

// L += the pending MIS contribution (Q_LMIS, written by k_shade); returns whether a bin of it was non-zero.
DEV bool AddMisContribution(const Pool &pool, uint32_t slot, int &flags) {
    bool added = false;
    const bool lZero = (flags & F_L_ZERO) != 0;
    for (int c = 0; c < NQ; ++c) {
        const float4 a = pool.Q(Q_LMIS + c, slot);
        added |= (a.x != 0.f) | (a.y != 0.f) | (a.z != 0.f) | (a.w != 0.f);
        float4 l = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!lZero) l = pool.Q(LPlane(flags) + c, slot);
        l.x += a.x; l.y += a.y; l.z += a.z; l.w += a.w;
        pool.Q(LPlane(flags) + c, slot) = l;
    }
    flags &= ~F_L_ZERO;
    return added;
}
// The MIS ray closes its vertex's direct-lighting estimate: zero radiance if neither it nor the light sample (F_A_ADDED) added.
// (Not a dark ray: its estimate never had F_MIS and was closed with added = false by CommitShadowVerdict or by k_shade.)
DEV void CloseMisEstimate(const Pool &pool, uint32_t slot, int flags, bool added, unsigned &zero) {
    if (!added && !(flags & F_A_ADDED)) ++zero;
    pool.I(I_FLAGS, slot) = flags & ~(F_NEE | F_MIS | F_A_ADDED);
}

// A MIS ray and the record of the hit k_trav<2> found for it (h.prim comes with the queue entry). They are fetched only by the
// few rays that need them: postponed quadrics, or a hit on the sampled light whose facing has to be tested (most MIS rays hit
// something else: 48 B of scattered reads saved)
DEV void LoadMisRay(const Pool &pool, uint32_t slot, V3 &ro, V3 &rd, Hit &h, bool &have) {
    if (have) return;
    const float4 r0 = pool.R(R_MI0, slot), r1 = pool.R(R_MI1, slot), hr = pool.R(R_HIT, slot);
    ro = PackedRayO(r0); rd = PackedRayD(r0, r1);
    if (h.prim >= 0) SetHitRecord(&h, hr);
    have = true;
}
// The closest hit of a MIS ray after its quadrics (h, when found). OVF: the list overflowed, the ray is traversed again.
template <bool INST, bool OVF, bool MOTION = false>
DEV bool MisClosestHit(const DScene &s, const Pool &pool, uint32_t slot, int npend, V3 &ro, V3 &rd, Hit &h, bool &haveRay) {
    bool found = h.prim >= 0;
    if (npend != 0) {
        LoadMisRay(pool, slot, ro, rd, h, haveRay);
        if constexpr (OVF) found = Retraverse<false, INST, MOTION>(s, ro, rd, kInfinity, &h, MOTION ? PathTime(s, pool, slot) : 0.f);
        else found = ResolveQuadrics<false>(s, pool, slot, ro, rd, kInfinity, &h, found, npend);
    }
    return found;
}

// One MIS ray's commit. OVF = false (k_resolve_mis): a ray whose quadric list overflowed goes to k_resolve_overflow, which
// runs this again with OVF = true.
template <bool INST, bool OVF, bool MOTION = false>
DEV void ResolveMisSlot(const DScene &s, const Pool &pool, DevCounters *ctr, uint32_t slot, int hitPrim, int npend, unsigned &zero) {
    int flags = pool.I(I_FLAGS, slot);
    V3 ro, rd;
    Hit h;
    h.prim = hitPrim; h.t = 0.f; h.b0 = h.b1 = h.b2 = 0.f;
    bool haveRay = false;
    if (!OVF && (npend & PEND_OVERFLOW)) { pool.ovfQ[2 * (size_t)pool.n + atomicAdd(&ctr->ovfCount[2].v, 1u)] = slot; return; }
    const bool found = MisClosestHit<INST, OVF, MOTION>(s, pool, slot, npend, ro, rd, h, haveRay);
    bool added = false;
    const int misLight = s.nLights > 1 ? pool.I(I_MISLIGHT, slot) : 0;
    if (!found && s.lights[misLight].type == MI_LIGHT_INFINITE) added |= AddMisContribution(pool, slot, flags);   // Li = light.Le(ray), integrator.cpp:204
    if (found) {
        const int lightNum = misLight;
        if (s.prims[h.prim].area_light == lightNum) {
            const mi_light &l = s.lights[lightNum];
            bool emit = l.two_sided != 0;
            if (!emit) {
                LoadMisRay(pool, slot, ro, rd, h, haveRay);
                SurfaceInteraction li;
                HitInteraction(s, h.prim, ro, rd, h.b0, h.b1, h.b2, &li);
                emit = Dot(li.n, -rd) > 0;
            }
            if (emit) added |= AddMisContribution(pool, slot, flags);
        }
    }
    CloseMisEstimate(pool, slot, flags, added, zero);
}
// The commit of a MIS ray that k_trav<3> answered as a visibility query (DScene::misAny). word0: an occluder's primitive,
// -1 (nothing accepted up to the end of the light's span) or -2 (something accepted inside the span). A ray that is
// ambiguous, met a quadric on its way to an area light, or reaches a sphere whose root the reference could reject against a
// hit beyond the span, goes to k_resolve_overflow: the closest-hit routine in the reference's order, then ResolveMisSlot.
DEV void ResolveMisVisibility(const DScene &s, const Pool &pool, DevCounters *ctr, uint32_t slot, int word0, int npend, unsigned &zero) {
    int flags = pool.I(I_FLAGS, slot);
    bool exact = (npend & PEND_OVERFLOW) != 0, add = false;
    if (!exact) {
        const int misLight = s.nLights > 1 ? pool.I(I_MISLIGHT, slot) : 0;
        const mi_light &l = s.lights[misLight];
        if (l.type == MI_LIGHT_INFINITE) {   // Li = light.Le(ray) if nothing is hit, integrator.cpp:204
            bool found = word0 >= 0;
            if (!found && (npend & 0xff)) {
                const float4 r0 = pool.R(R_MI0, slot), r1 = pool.R(R_MI1, slot);
                Hit h;
                found = ResolveQuadrics<true>(s, pool, slot, PackedRayO(r0), PackedRayD(r0, r1), kInfinity, &h, false, npend);
            }
            add = !found;
        } else if (word0 >= 0) {}           // a primitive in front of the light's span
        else if (word0 == -2 || (npend & 0xff)) exact = true;
        else {                              // nothing up to the end of the span: the light's shape, if the ray meets it, is the closest hit
            const float4 r0 = pool.R(R_MI0, slot), r1 = pool.R(R_MI1, slot);
            const V3 ro = PackedRayO(r0), rd = PackedRayD(r0, r1);
            if (l.shape < 0 && IsDisk(s, ~l.shape)) {   // a disk: the triangle's way (k_shade: Shape::Pdf has intersected it, else there is no ray)
                SurfaceInteraction li;
                float t;
                if (l.two_sided != 0) add = true;
                else if (DiskInteraction(s.disks[~l.shape - s.nSpheres], ro, rd, kInfinity, &li, &t)) add = Dot(li.n, -rd) > 0;
            } else if (l.shape < 0) {
                const mi_sphere &sp = s.spheres[~l.shape];
                SurfaceInteraction li;
                float t, t2;
                if (SphereInteraction(sp, ro, rd, kInfinity, &li, &t)) {
                    if (!SphereHitT(sp, ro, rd, r1.z, &t2)) exact = true;   // (its upper error bound lies beyond the span)
                    else add = l.two_sided != 0 || Dot(li.n, -rd) > 0;
                }
            } else if (l.two_sided != 0) add = true;   // (k_shade: Shape::Pdf has intersected the triangle, else there is no ray)
            else {
                const int32_t *v = &s.triIndices[3 * l.shape];
                TriHit th;
                if (TriTest(LoadV3(s.P, v[0]), LoadV3(s.P, v[1]), LoadV3(s.P, v[2]), ro, rd, kInfinity, &th)) {
                    SurfaceInteraction li;
                    TriInteraction(s, l.shape, th.b0, th.b1, th.b2, rd, &li);
                    add = Dot(li.n, -rd) > 0;
                }
            }
        }
    }
    if (exact) { pool.ovfQ[2 * (size_t)pool.n + atomicAdd(&ctr->ovfCount[2].v, 1u)] = slot; return; }
    const bool added = add && AddMisContribution(pool, slot, flags);
    CloseMisEstimate(pool, slot, flags, added, zero);
}
template <bool INST>
__global__ void __launch_bounds__(BLOCK) k_resolve_mis(DScene s, Pool pool, DevCounters *ctr) {
    const unsigned count = ctr->misCount.v;   // (a resident-sized grid walks the queue, as in k_resolve_shadow)
    unsigned zero = 0, darkSeen = 0;
    for (uint32_t qi = blockIdx.x * BLOCK + threadIdx.x; qi < count; qi += gridDim.x * BLOCK) {
        const uint2 v = *reinterpret_cast<const uint2 *>(pool.misQ + pool.n + 2 * (size_t)qi);   // k_trav<2>'s / k_trav<3>'s answer, in queue order
        // a dark ray: nothing reads its answer, and its estimate is closed already (k_trav<2> scenes and mi_pt_trace_wavefront
        // only: where k_trav<3> serves the queue the dark rays have Pool::darkQ and none comes by here)
        if (v.y & MIS_ANSWER_DARK) { ++darkSeen; continue; }
        if (!INST && s.misAny) ResolveMisVisibility(s, pool, ctr, pool.misQ[qi], (int)v.x, (int)v.y, zero);
        else ResolveMisSlot<INST, false>(s, pool, ctr, pool.misQ[qi], (int)v.x, (int)v.y, zero);
    }
    CountAdd(&Stats(ctr).zeroRadiancePaths, zero);
    CountAdd(&Stats(ctr).misDarkSeen, darkSeen);
}

// The rays whose list of postponed quadrics overflowed (more than MAX_PEND quadrics met: PEND_OVERFLOW), handed over by
// the three resolve kernels: re-traversed by the reference-order routine with inline quadric tests, then committed as the
// resolve kernel would have (mode 0: hit record + shading queue; 1: occlusion + L += the light sample; 2: the MIS commit).
// A fixed small grid walks the queue; it is empty for all but quadric-heavy scenes.
template <bool INST, bool MOTION = false>
__global__ void __launch_bounds__(BLOCK) k_resolve_overflow(DScene s, Pool pool, DevCounters *ctr, int mode) {
    const unsigned count = ctr->ovfCount[mode].v;
    unsigned zero = 0, pathLen = 0;
    for (unsigned qi = blockIdx.x * BLOCK + threadIdx.x; qi < count; qi += gridDim.x * BLOCK) {
        const uint32_t slot = pool.ovfQ[(size_t)mode * pool.n + qi];
        if (mode == 0) {
            const float4 r0 = pool.R(R_RAY0, slot), r1 = pool.R(R_RAY1, slot);
            Hit h;
            h.prim = -1; h.t = 0.f; h.b0 = h.b1 = h.b2 = 0.f;
            const bool found = Retraverse<false, INST, MOTION>(s, V3(r0.x, r0.y, r0.z), V3(r1.x, r1.y, r1.z), r0.w, &h, MOTION ? PathTime(s, pool, slot) : 0.f);
            const int prim = found ? h.prim : -1;
            pool.I(I_HITPRIM, slot) = prim;
            pool.R(R_HIT, slot) = HitRecord(h);
            if (INST) pool.I(I_HITINST, slot) = h.inst;
            const int word = pool.I(I_FLAGS, slot);
            if (EndsUnshaded(word, prim, s.maxDepth, s.nInfiniteLights)) { pool.I(I_FLAGS, slot) = FinishedWord(word); pathLen += (unsigned)StateBounces(word); }
            else {
                const int cls = ClassOfPrim(s.primTri, prim);
                pool.shadeQ[(size_t)cls * pool.n + atomicAdd(&ctr->shadeCount[cls].v, 1u)] = slot;
            }
        } else if (mode == 1) {
            const float4 r0 = pool.R(R_SH0, slot), r1 = pool.R(R_SH1, slot);
            Hit h;
            const bool occluded = Retraverse<true, INST, MOTION>(s, PackedRayO(r0), PackedRayD(r0, r1), 1 - kShadowEpsilon, &h, MOTION ? PathTime(s, pool, slot) : 0.f);
            pool.I(I_FLAGS, slot) = CommitShadowVerdict(pool.I(I_FLAGS, slot), occluded, zero);
        } else
            ResolveMisSlot<INST, true, MOTION>(s, pool, ctr, slot, -1, PEND_OVERFLOW, zero);   // (re-traversed from scratch)
    }
    CountAdd(&Stats(ctr).zeroRadiancePaths, zero);
    CountAdd(&Stats(ctr).pathLengthSum, pathLen);
}

// ------------------------------------------------------------------ generate
// MOVING (mi_camera.animated, uniform over a launch): the ray's time is Lerp(timeU, shutterOpen, shutterClose)
// (perspective.cpp:141) and CameraToWorld is the AnimatedTransform at that time (MovingCameraToWorld, d_scene.h). The
// instance for a camera that does not move is the code it always was: no time, one matrix.
template <bool MOVING = false>
DEV void CameraRay(const DScene &s, float pFilmX, float pFilmY, float lensU, float lensV, Ray *out, float timeU = 0.f, float *timeOut = nullptr) {
    // PerspectiveCamera::GenerateRayDifferential, perspective.cpp:95-146 (differentials feed
    // only texture filtering; every texture on this path is constant)
    const mi_camera &cam = s.camera;
    V3 pCamera = XfPoint(cam.raster_to_camera, V3(pFilmX, pFilmY, 0));
    V3 dir = Normalize(V3(pCamera.x, pCamera.y, pCamera.z));
    Ray ray(V3(0, 0, 0), dir);
    if (cam.lens_radius > 0) {
        float dx, dy;
        ConcentricSampleDisk(lensU, lensV, &dx, &dy);
        float lx = cam.lens_radius * dx, ly = cam.lens_radius * dy;
        float ft = cam.focal_distance / ray.d.z;
        V3 pFocus = ray.at(ft);
        ray.o = V3(lx, ly, 0);
        ray.d = Normalize(pFocus - ray.o);
    }
    if constexpr (MOVING) {
        const float time = lerpf(timeU, cam.shutter_open, cam.shutter_close);
        if (timeOut) *timeOut = time;
        float m[16];
        MovingCameraToWorld(s.cameraMotion, time, m);
        *out = XfRay(m, ray);
    } else
        *out = XfRay(cam.camera_to_world, ray);
}

#if MIPT_HAS_MAIN
// FilmTile::AddSample + MergeFilmTile (film.h:123-163, film.cpp:124-142) as float atomics
// into the resident film [pixel][32] (31 bins + filter-weight sum = one 128-B row), then the refill of the
// freed slots with new camera samples, then the extend work list.
//
// A block owns SLOT_CHUNKS x 256 consecutive slots and makes three passes over them, so that everything it needs from a
// shared cursor is asked for ONCE per block (a word takes ~88 returning atomics per microsecond; see SLOT_CHUNKS, pt_pool.h):
//   pass 1  flush the finished paths of each chunk into the film -- each finished lane stages its guarded radiance in LDS
//           (row stride 33 words: conflict-free both ways); the samples of a wave that go to the same pixel are summed
//           there and leave as ONE 128-B row update, two pixels per wave instruction (the full-rate shape for gfx950
//           float atomics) -- and count the slots that are free now;
//   ------  one atomicAdd on the work counter for all of them;
//   pass 2  camera sample and camera ray for each free slot that drew a work item inside the bounds (an item outside
//           them -- a pixel of an edge tile beyond the film -- leaves its slot idle for this iteration: the host stops
//           when no path is alive AND the work counter has passed the end); count new and continuing paths;
//   ------  one atomicAdd each on the two cursors of the extend work list;
//   pass 3  write the work list: new camera rays from the front (consecutive samples of a pixel: the most coherent rays),
//           continuing paths from the back.
// MOVING: the camera moves (mi_camera.animated): the camera sample's time is evaluated and the ray goes through the transform at that time.
// REAL: Camera "realistic" (mi_scene_desc.camera_type): the ray comes through the lens system (LensCameraRay) with a weight, kept in
// P_WEIGHT and multiplied into the sample at the flush. A sample of weight 0 is a camera ray that traces nothing: its slot is
// finished here (L = 0), stays out of the extend list, counts as alive -- the host's next iteration flushes it -- and a
// "spectralpath" band that is vignetted restarts as the next band like any finished one.
// TIME: the scene has moving instances: the ray's time -- Lerp(time sample, shutterOpen, shutterClose), perspective.cpp:141 --
// goes to the pool's time plane (PathTime), so the time sample is evaluated in front of a camera that stands still too.
// CAM: the camera's mi_camera_type. MI_CAMERA_ORTHOGRAPHIC / MI_CAMERA_ENVIRONMENT (d_camera.h): weight 1, no weight plane; in
// front of textures (DScene::lensDiff) the ray's differentials go to the planes the realistic camera's go to.
template <bool MOVING, int CAM, bool TIME = false>
__global__ void __launch_bounds__(BLOCK) k_generate(DScene s, Pool pool, float *film, DevCounters *ctr, WorkDesc wd) {
    constexpr bool REAL = CAM == MI_CAMERA_REALISTIC;
    __shared__ float sL[BLOCK * 33];
    __shared__ float sFilter[256];  // the 16x16 filter table, one LDS copy per block
    __shared__ unsigned sWant[SLOT_CHUNKS][BLOCK / 64], sPrim[SLOT_CHUNKS][BLOCK / 64], sCont[SLOT_CHUNKS][BLOCK / 64];
    __shared__ unsigned long long sWorkBase;
    __shared__ unsigned sPrimBase, sContBase, sTotWant, sTotFin;
    __shared__ unsigned sFinCnt[SLOT_CHUNKS][BLOCK / 64];
    __shared__ unsigned short sFin[SLOT_CHUNKS * BLOCK];   // the block's finished slots: offset in the block | 0x8000 if L reads as zero | 0x4000 if it lives in Q_LB
    static_assert(SLOT_CHUNKS * BLOCK <= 0x4000, "sFin: the offset shares its word with two flags");
    sFilter[threadIdx.x] = s.filterTable[threadIdx.x];
    __syncthreads();
    unsigned bad = 0, cam = 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int waveBase = threadIdx.x & ~63;
    const unsigned long long ltMask = (1ull << lane) - 1ull;
    const int nBands = s.nBands;
    unsigned wantBits = 0, restartBits = 0, contBits = 0, gotBits = 0;   // bit ch: state of this thread's slot in chunk ch
    unsigned finBits = 0, finZeroBits = 0, finInBBits = 0;
    // ---------------------------------------------------------------- pass 1: film flush
    // The finished paths are a third of the block's slots: they are listed first (in slot order: neighbours in the list are
    // samples of the same pixel more often than not) and flushed by all lanes together, as the refill below -- chunk by
    // chunk, a third of each wave worked through eight dependent round trips to memory (state word, then the L line) and
    // the kernel waited them out at four blocks per CU (in-kernel stamps, round 3: 78 % of the kernel in this pass).
    {
        int fl[SLOT_CHUNKS];
#pragma unroll
        for (int ch = 0; ch < SLOT_CHUNKS; ++ch) {   // (all eight loads in flight together)
            const uint32_t slot = (blockIdx.x * SLOT_CHUNKS + ch) * BLOCK + threadIdx.x;
            fl[ch] = slot < pool.n ? pool.I(I_FLAGS, slot) : -1;
        }
#pragma unroll
        for (int ch = 0; ch < SLOT_CHUNKS; ++ch) {
            const uint32_t slot = (blockIdx.x * SLOT_CHUNKS + ch) * BLOCK + threadIdx.x;
            const bool valid = slot < pool.n;
            const int flags = fl[ch];
            const bool fin = valid && (flags & F_FINISHED);
            // Integrator "spectralpath" (spectralpath.cpp:258-318): nBands paths per camera sample; a finished
            // path hands its bins to the sample's stitched spectrum and the slot restarts on the same camera ray
            // with the sampler dimension running on; the last band flushes the stitched spectrum.
            const bool restart = fin && nBands > 1 && pool.I(I_BAND, slot) + 1 < nBands;
            const bool want = valid && (fin || (flags & FLAG_MASK) == 0) && !restart;   // (a flushed slot is free)
            if (fin) finBits |= 1u << ch;
            if (fin && (flags & F_L_ZERO)) finZeroBits |= 1u << ch;
            if (fin && (flags & F_L_IN_B)) finInBBits |= 1u << ch;
            if (want) wantBits |= 1u << ch;
            if (restart) restartBits |= 1u << ch;
            if (valid && !fin && (flags & F_ALIVE)) contBits |= 1u << ch;
            const unsigned long long wm = __ballot(want), fm = __ballot(fin);
            if (lane == 0) { sWant[ch][wave] = (unsigned)__popcll(wm); sFinCnt[ch][wave] = (unsigned)__popcll(fm); }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {   // the block's range of the work list in one add
        const unsigned tot = ChunkWavePrefix(&sWant[0][0], 1);
        sWorkBase = tot ? atomicAdd(&ctr->nextWork, (unsigned long long)tot) : ~0ull;
        sTotWant = tot;
    }
    if (threadIdx.x == 64) sTotFin = ChunkWavePrefix(&sFinCnt[0][0], 1);
    __syncthreads();
#pragma unroll 1
    for (int ch = 0; ch < SLOT_CHUNKS; ++ch) {
        const bool fin = (finBits >> ch) & 1u;
        const unsigned long long fm = __ballot(fin);
        if (fin) sFin[sFinCnt[ch][wave] + (unsigned)__popcll(fm & ltMask)] =
            (unsigned short)((ch * BLOCK + threadIdx.x) | (((finZeroBits >> ch) & 1u) ? 0x8000u : 0u) | (((finInBBits >> ch) & 1u) ? 0x4000u : 0u));
    }
    __syncthreads();
    const unsigned totFin = sTotFin;
#pragma unroll 1
    for (unsigned round = 0; round < (totFin + BLOCK - 1) / BLOCK; ++round) {
        const unsigned fi = round * BLOCK + threadIdx.x;
        const bool fin = fi < totFin;
        const unsigned fe = fin ? sFin[fi] : 0u;
        const uint32_t slot = blockIdx.x * SLOT_CHUNKS * BLOCK + (fe & 0x3fffu);
        float myFx = 0, myFy = 0;
        [[maybe_unused]] float myW = 1.f;
        int myZero = 0;
        bool restart = false;
        if (fin) {
            int band = 0;
            if (nBands > 1) band = pool.I(I_BAND, slot);
            myFx = pool.F(P_FILMX, slot);   // (asked for with the L line: behind the guards, the film rows waited a round trip of their own)
            myFy = pool.F(P_FILMY, slot);
            if constexpr (REAL) myW = pool.F(P_WEIGHT, slot);   // (spectralpath: the last band's)
            // guards of SamplerIntegrator::Render, integrator.cpp:295-316
            float yy = 0.f;
            bool hasNaN = false;
            float *row = &sL[threadIdx.x * 33];
            const bool lZero = (fe & 0x8000u) != 0;
            const int lPlane = (fe & 0x4000u) ? Q_LB : Q_L;
            for (int c = 0; c < NQ; ++c) {
                float4 v4 = make_float4(0.f, 0.f, 0.f, 0.f);
                if (!lZero) v4 = pool.Q(lPlane + c, slot);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int b = 4 * c + k;
                    if (b < MI_NSPEC) {
                        const float v = Get4(v4, k);
                        hasNaN |= isnanf_(v);
                        yy += s.cieY[b] * v;
                        row[b] = v;
                    }
                }
            }
            float y = YScale(yy);
            bool zero = false;
            if (hasNaN) zero = true;
            else if ((double)y < -1e-5) zero = true;
            else if (isinff(y)) zero = true;
            if (zero) ++bad;
            if (nBands > 1) {
                const int lo = s.bandDelta * band, hi = min(s.bandDelta * (band + 1), MI_NSPEC);
                for (int c = 0; c < NQ; ++c) {   // bins [lo, hi) of the stitched spectrum <- this band's path
                    if (4 * c + 3 < lo || 4 * c >= hi) continue;
                    float4 v4 = pool.Q(Q_LCA + c, slot);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int b = 4 * c + k;
                        if (b >= lo && b < hi) Set4(v4, k, zero ? 0.f : row[b]);
                    }
                    pool.Q(Q_LCA + c, slot) = v4;
                }
                zero = false;
                if (band + 1 < nBands) restart = true;
                else {
                    yy = 0.f;
                    for (int c = 0; c < NQ; ++c) {
                        const float4 v4 = pool.Q(Q_LCA + c, slot);
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int b = 4 * c + k;
                            if (b < MI_NSPEC) {
                                const float v = Get4(v4, k);
                                yy += s.cieY[b] * v;
                                row[b] = v;
                            }
                        }
                    }
                    y = YScale(yy);
                }
            }
            if (!zero && !restart && y > s.maxSampleLuminance) {  // FilmTile::AddSample clamp, film.h:126-127
                const float scaleL = s.maxSampleLuminance / y;
                for (int b = 0; b < MI_NSPEC; ++b) row[b] *= scaleL;
            }
            myZero = zero ? 1 : 0;
        }
        // (a wave reads only the rows its own lanes staged, and its LDS accesses complete in order: nothing to wait for, the
        // fences keep the compiler from moving the accesses -- at workgroup scope each one also waited for every film atomic
        // in flight)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        {
            const int half = lane >> 5, bin = lane & 31;
            const int filterTableSize = 16;
            const float invRx = 1 / s.filterRadius[0], invRy = 1 / s.filterRadius[1];
            const int w = s.croppedBounds[2] - s.croppedBounds[0];
            // The sample's footprint (FilmTile::AddSample, film.h:131-141). With a radius of at most half a pixel -- the box
            // filter of the BASELINE scenes -- it is one pixel for every sample that does not sit exactly on a pixel border.
            int p0x = 0, p0y = 0, p1x = 0, p1y = 0, myTarget = -1;
            float myFw = 0.f;
            if (fin && !restart) {
                const float dx = myFx - 0.5f, dy = myFy - 0.5f;
                p0x = (int)ceilf(dx - s.filterRadius[0]); p0y = (int)ceilf(dy - s.filterRadius[1]);
                p1x = (int)floorf(dx + s.filterRadius[0]) + 1; p1y = (int)floorf(dy + s.filterRadius[1]) + 1;
                p0x = max(p0x, s.croppedBounds[0]); p0y = max(p0y, s.croppedBounds[1]);
                p1x = min(p1x, s.croppedBounds[2]); p1y = min(p1y, s.croppedBounds[3]);
                if (p1x - p0x == 1 && p1y - p0y == 1) {
                    const float fy = absf((p0y - dy) * invRy * filterTableSize), fx = absf((p0x - dx) * invRx * filterTableSize);
                    const int iy = min((int)floorf(fy), filterTableSize - 1), ix = min((int)floorf(fx), filterTableSize - 1);
                    myFw = sFilter[iy * filterTableSize + ix];
                    myTarget = (p0x - s.croppedBounds[0]) + (p0y - s.croppedBounds[1]) * w;
                }
            }
            // Single-pixel samples: summed per pixel in LDS, one row update per pixel. Two pixels per pass, half-wave h
            // summing the rows of group h bin by bin.
            unsigned long long todo = __ballot(myTarget >= 0);
            while (todo) {
                const int j0 = __ffsll((long long)todo) - 1;
                const int t0 = __shfl(myTarget, j0, 64);
                const unsigned long long g0 = __ballot(myTarget == t0) & todo;
                todo &= ~g0;
                unsigned long long g1 = 0ull;
                int t1 = -1;
                if (todo) {
                    const int j1 = __ffsll((long long)todo) - 1;
                    t1 = __shfl(myTarget, j1, 64);
                    g1 = __ballot(myTarget == t1) & todo;
                    todo &= ~g1;
                }
                unsigned long long g = half ? g1 : g0;
                const int tgt = half ? t1 : t0;
                float acc = 0.f;
                const int nWalk = max(__popcll(g0), __popcll(g1));
                for (int it = 0; it < nWalk; ++it) {   // both halves walk their own group, in step (the shuffles need every lane)
                    const bool have = g != 0ull;
                    const int p = have ? __ffsll((long long)g) - 1 : 0;
                    g &= g - 1;
                    const float fw = __shfl(myFw, p, 64);
                    const int zero = __shfl(myZero, p, 64);
                    float sw = 1.f;
                    if constexpr (REAL) sw = __shfl(myW, p, 64);
                    if (have) {
                        if (bin == 31) acc += fw;                                                // filterWeightSum += fw
                        else if (!zero) acc += (sL[(waveBase + p) * 33 + bin] * sw) * fw;       // contribSum += L * sampleWeight * fw
                    }
                }
                if (tgt >= 0 && acc != 0.f) atomicAdd(film + (size_t)tgt * 32 + bin, acc);   // (x + 0 == x: a black bin is not sent)
            }
            // Wider footprints (other filters, samples on a pixel border): one row update per sample and pixel reached.
            unsigned long long mask = __ballot(fin && !restart && myTarget < 0);
            while (mask) {
                const int j0 = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                int j1 = -1;
                if (mask) { j1 = __ffsll((long long)mask) - 1; mask &= mask - 1; }
                const int j = half ? j1 : j0;
                const int src = j >= 0 ? j : 0;
                const float pfx = __shfl(myFx, src, 64), pfy = __shfl(myFy, src, 64);
                const int zero = __shfl(myZero, src, 64);
                float sw = 1.f;
                if constexpr (REAL) sw = __shfl(myW, src, 64);
                const int q0x = __shfl(p0x, src, 64), q0y = __shfl(p0y, src, 64), q1x = __shfl(p1x, src, 64), q1y = __shfl(p1y, src, 64);
                if (j >= 0) {
                    const float val = (bin < MI_NSPEC) ? sL[(waveBase + j) * 33 + bin] : 0.f;
                    const float dx = pfx - 0.5f, dy = pfy - 0.5f;
                    for (int y2 = q0y; y2 < q1y; ++y2) {
                        float fy = absf((y2 - dy) * invRy * filterTableSize);
                        int iy = min((int)floorf(fy), filterTableSize - 1);
                        for (int x2 = q0x; x2 < q1x; ++x2) {
                            float fx = absf((x2 - dx) * invRx * filterTableSize);
                            int ix = min((int)floorf(fx), filterTableSize - 1);
                            float fw = sFilter[iy * filterTableSize + ix];
                            size_t pix = (size_t)(x2 - s.croppedBounds[0]) + (size_t)(y2 - s.croppedBounds[1]) * w;
                            float *dst = film + pix * 32 + bin;
                            if (bin == 31) atomicAdd(dst, fw);                     // filterWeightSum += fw
                            else if (!zero && val != 0.f) atomicAdd(dst, (val * sw) * fw);   // contribSum += L * sampleWeight * fw (x + 0 == x: a black bin is not sent)
                        }
                    }
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // the rows are read before the next round overwrites them
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    // ---------------------------------------------------------------- pass 2: refill
    // The free slots are a third of the block's slots, spread over all chunks: they are listed (in slot order, so work item
    // base + i still goes to the i-th free slot) and refilled by all lanes together -- the camera sample (index of the
    // Halton / Sobol' sample, five dimensions, the camera ray) runs on full waves.
    unsigned short *sFree = (unsigned short *)sL;                 // (pass 1's rows are dead now)
    unsigned char *sGot = (unsigned char *)(sL + SLOT_CHUNKS * BLOCK / 2);
#pragma unroll 1
    for (int ch = 0; ch < SLOT_CHUNKS; ++ch) {
        const bool want = (wantBits >> ch) & 1u;
        const unsigned long long wm = __ballot(want);
        if (want) sFree[sWant[ch][wave] + (unsigned)__popcll(wm & ltMask)] = (unsigned short)(ch * BLOCK + threadIdx.x);
        sGot[ch * BLOCK + threadIdx.x] = 0;
    }
    __syncthreads();
    const unsigned totWant = sTotWant;
    const unsigned nRounds = (nBands > 1) ? SLOT_CHUNKS : 0;   // spectralpath: the restarting slots, chunk by chunk as before
    bool anyAlive = false;
#pragma unroll 1
    for (unsigned it = 0; it < nRounds + (totWant + BLOCK - 1) / BLOCK; ++it) {
        const bool restartRound = it < nRounds;
        unsigned e = 0;
        bool want = false, restart = false;
        if (restartRound) { e = it * BLOCK + threadIdx.x; restart = (restartBits >> it) & 1u; }
        else { const unsigned i = (it - nRounds) * BLOCK + threadIdx.x; want = i < totWant; if (want) e = sFree[i]; }
        const uint32_t slot = blockIdx.x * SLOT_CHUNKS * BLOCK + e;
        bool got = false;
        int px = 0, py = 0, band = 0;
        long long sampleNum = 0;
        int dimBefore = 0;
        if (restart) {  // next band of the same camera sample
            dimBefore = StateDim(pool.I(I_FLAGS, slot));   // (the band's path goes on with the sampler dimension the last one reached)
            const int pix = pool.I(I_PIXEL, slot);
            px = (int)(short)(pix & 0xffff); py = pix >> 16;
            sampleNum = pool.I(I_SAMPLE, slot);
            band = pool.I(I_BAND, slot);
            got = true;
        }
        if (want) {
            const unsigned long long w = sWorkBase + (unsigned long long)((it - nRounds) * BLOCK + threadIdx.x);
            if (w < wd.totalWork) {
                // work order: runs of wd.run consecutive samples of a pixel, pixel by pixel through the shard's tiles, then
                // the next run (so the lanes of a wave hold neighbouring samples of a few pixels: the most coherent camera
                // rays, and finished samples that can be summed before they reach the film)
                const unsigned run = (unsigned)wd.run;
                const unsigned long long perChunk = (unsigned long long)wd.nTilesShard * 256ull * run;
                const unsigned long long chunk = w / perChunk;
                const unsigned long long inChunk = w % perChunk;
                sampleNum = wd.sampleBegin + (long long)(chunk * run + (inChunk % run));
                unsigned rem = (unsigned)(inChunk / run);
                int tileLocal = rem >> 8, pix = rem & 255;
                int tile = wd.shardIndex + tileLocal * wd.shardCount;
                int tx = tile % wd.nTilesX, ty = tile / wd.nTilesX;
                int blk = pix >> 6, within = pix & 63;
                px = s.sampleBounds[0] + tx * 16 + (within & 7) + (blk & 1) * 8;
                py = s.sampleBounds[1] + ty * 16 + (within >> 3) + (blk >> 1) * 8;
                if (px < s.sampleBounds[2] && py < s.sampleBounds[3] && px >= s.pixelBounds[0] && px < s.pixelBounds[2] &&
                    py >= s.pixelBounds[1] && py < s.pixelBounds[3])
                    got = true;
            }
        }
        if (got) {
            // GetCameraSample (sampler.cpp:46-52): pFilm = dims 0,1; time = dim 2; pLens = dims 3,4
            float u0, u1, lu, lv;
            int dimAfter;
            float tu = 0.f;
            const uint64_t index = CameraSampleDims<MOVING || TIME>(s, px, py, sampleNum, &u0, &u1, &lu, &lv, &dimAfter, &tu);
            if constexpr (TIME) pool.F(s.timePlane, slot) = lerpf(tu, s.camera.shutter_open, s.camera.shutter_close);
            float pfx = (float)px + u0, pfy = (float)py + u1;
            Ray ray;
            bool traced = true;   // REAL: the ray got through the lens (GenerateRayDifferential's weight > 0: Li is called)
            if constexpr (REAL) {
                float wavelength = 550.f;
                if (nBands > 1) wavelength = BandWavelength(s.bandDelta, restart ? band + 1 : 0);
                V3 diff[4];   // (always asked for, stored only under lensDiff: a pointer chosen at run time moved the array to private memory)
                const float rayWeight = LensCameraRay<MOVING>(s, pfx, pfy, lu, lv, tu, wavelength, &ray, nullptr, diff, s.invSqrtSpp);
                traced = rayWeight > 0;
                if (s.lensDiff && traced) {   // (uniform)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        pool.F(P_LENSDIFF + 3 * k, slot) = diff[k].x; pool.F(P_LENSDIFF + 3 * k + 1, slot) = diff[k].y; pool.F(P_LENSDIFF + 3 * k + 2, slot) = diff[k].z;
                    }
                }
                pool.F(P_WEIGHT, slot) = s.ignoreRayWeight ? 1.f : rayWeight;   // (Integrator "metadata": IgnoreRayWeight)
            } else if constexpr (CAM == MI_CAMERA_ORTHOGRAPHIC || CAM == MI_CAMERA_ENVIRONMENT) {
                if (s.lensDiff) {   // (uniform; the environment camera's offset rays are two more rays: made only where a texture reads them)
                    V3 diff[4];
                    OptInCameraRay<CAM, MOVING>(s, pfx, pfy, lu, lv, tu, &ray, nullptr, diff, s.invSqrtSpp);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        pool.F(P_LENSDIFF + 3 * k, slot) = diff[k].x; pool.F(P_LENSDIFF + 3 * k + 1, slot) = diff[k].y; pool.F(P_LENSDIFF + 3 * k + 2, slot) = diff[k].z;
                    }
                } else
                    OptInCameraRay<CAM, MOVING>(s, pfx, pfy, lu, lv, tu, &ray, nullptr, nullptr, 0.f);
            } else
                CameraRay<MOVING>(s, pfx, pfy, lu, lv, &ray, tu);
            ++cam;
            if (traced) {
                pool.R(R_RAY0, slot) = make_float4(ray.o.x, ray.o.y, ray.o.z, ray.tMax);
                pool.R(R_RAY1, slot) = make_float4(ray.d.x, ray.d.y, ray.d.z, 1.f);   // etaScale = 1
            }
            pool.F(P_FILMX, slot) = pfx; pool.F(P_FILMY, slot) = pfy;

            if (s.storePixelSample) {   // (a moving camera in front of textures: k_shade evaluates the sample's time again)
                pool.I(I_PIXEL, slot) = (px & 0xffff) | (py << 16);
                pool.I(I_SAMPLE, slot) = (int)sampleNum;
            }
            if (!(restart && s.samplerType >= MI_SAMPLER_RANDOM)) {   // (a restarted band draws on from where its stream stands)
                pool.I(I_IDXLO, slot) = (int)(uint32_t)index;
                if (!s.index32) pool.I(I_IDXHI, slot) = (int)(uint32_t)(index >> 32);
            }
            const bool pixelSampler = IsPixelSampler(s);
            if (!restart && pixelSampler) pool.I(I_DIM, slot) = dimAfter;
            if (nBands > 1) {
                pool.I(I_BAND, slot) = restart ? band + 1 : 0;
                if (!restart) for (int c = 0; c < NQ; ++c) pool.Q(Q_LCA + c, slot) = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            pool.I(I_FLAGS, slot) = StateWord(traced ? (F_ALIVE | F_L_ZERO | F_BETA_ONE | F_DIFF) : (F_FINISHED | F_L_ZERO | F_BETA_ONE), 0,
                                              pixelSampler ? 0 : (restart ? dimBefore : dimAfter));   // L = 0, beta = 1, not stored
            sGot[e] = (REAL && !traced) ? 2 : 1;
        } else if (want) pool.I(I_FLAGS, slot) = 0;   // stays free (its finished path has been flushed)
    }
    __syncthreads();
#pragma unroll 1
    for (int ch = 0; ch < SLOT_CHUNKS; ++ch) {
        const bool got = REAL ? sGot[ch * BLOCK + threadIdx.x] == 1 : sGot[ch * BLOCK + threadIdx.x] != 0;
        if (got) gotBits |= 1u << ch;
        const bool isCont = ((contBits >> ch) & 1u) != 0;
        anyAlive |= got || isCont;
        if constexpr (REAL) anyAlive |= sGot[ch * BLOCK + threadIdx.x] == 2;   // (finished above, flushed by the next iteration)
        // the extend work list: new camera rays first (lanes of a traversal wave then hold neighbouring samples)
        const unsigned long long pm = __ballot(got), cm = __ballot(isCont);
        if (lane == 0) { sPrim[ch][wave] = (unsigned)__popcll(pm); sCont[ch][wave] = (unsigned)__popcll(cm); }
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const unsigned tot = ChunkWavePrefix(threadIdx.x == 0 ? &sPrim[0][0] : &sCont[0][0], 1);
        const unsigned base = tot ? atomicAdd(threadIdx.x == 0 ? &ctr->primCount.v : &ctr->contCount.v, tot) : 0;
        if (threadIdx.x == 0) sPrimBase = base; else sContBase = base;
    }
    if (__any(anyAlive) && lane == 0) ctr->alive.v = 1;   // (a flag, not a count: the host only asks whether any path is left)
    __syncthreads();
    // ---------------------------------------------------------------- pass 3: the extend work list
#pragma unroll 1
    for (int ch = 0; ch < SLOT_CHUNKS; ++ch) {
        const uint32_t slot = (blockIdx.x * SLOT_CHUNKS + ch) * BLOCK + threadIdx.x;
        const bool isPrim = (gotBits >> ch) & 1u, isCont = (contBits >> ch) & 1u;
        const unsigned long long pm = __ballot(isPrim), cm = __ballot(isCont);
        if (isPrim) pool.extQ[sPrimBase + sPrim[ch][wave] + (unsigned)__popcll(pm & ltMask)] = slot;
        if (isCont) pool.extQ[pool.n - 1 - (sContBase + sCont[ch][wave] + (unsigned)__popcll(cm & ltMask))] = slot;
    }
    CountAdd(&Stats(ctr).cameraRays, cam);
    CountAdd(&Stats(ctr).badSamples, bad);
}

// The k_generate of a scene's camera: a uniform choice per launch.
GenerateKernel GenerateKernelOf(const DScene &s) {
    const bool moving = s.camera.animated != 0;
    if (s.motions) {
        switch (s.cameraType) {
        case MI_CAMERA_REALISTIC: return moving ? k_generate<true, MI_CAMERA_REALISTIC, true> : k_generate<false, MI_CAMERA_REALISTIC, true>;
        case MI_CAMERA_ORTHOGRAPHIC: return moving ? k_generate<true, MI_CAMERA_ORTHOGRAPHIC, true> : k_generate<false, MI_CAMERA_ORTHOGRAPHIC, true>;
        case MI_CAMERA_ENVIRONMENT: return moving ? k_generate<true, MI_CAMERA_ENVIRONMENT, true> : k_generate<false, MI_CAMERA_ENVIRONMENT, true>;
        default: return moving ? k_generate<true, MI_CAMERA_PERSPECTIVE, true> : k_generate<false, MI_CAMERA_PERSPECTIVE, true>;
        }
    }
    switch (s.cameraType) {
    case MI_CAMERA_REALISTIC: return moving ? k_generate<true, MI_CAMERA_REALISTIC> : k_generate<false, MI_CAMERA_REALISTIC>;
    case MI_CAMERA_ORTHOGRAPHIC: return moving ? k_generate<true, MI_CAMERA_ORTHOGRAPHIC> : k_generate<false, MI_CAMERA_ORTHOGRAPHIC>;
    case MI_CAMERA_ENVIRONMENT: return moving ? k_generate<true, MI_CAMERA_ENVIRONMENT> : k_generate<false, MI_CAMERA_ENVIRONMENT>;
    default: return moving ? k_generate<true, MI_CAMERA_PERSPECTIVE> : k_generate<false, MI_CAMERA_PERSPECTIVE>;
    }
}

#endif   // MIPT_HAS_MAIN

// Transform::operator()(const SurfaceInteraction&), transform.cpp:262-297, with an instance's InstanceToWorld: the fields the
// path reads (SurfaceInteraction) and the ones textures and bump mapping read besides (TriShading).
DEV void InteractionToWorld(const float *m, const float *mInv, SurfaceInteraction *si) {
    V3 pErr;
    si->p = XfPointErr2(m, si->p, si->pError, &pErr);
    si->pError = pErr;
    si->n = Normalize(XfNormal(mInv, si->n));
    si->wo = Normalize(XfVector(m, si->wo));
    si->dpdu = XfVector(m, si->dpdu);
    si->shN = Normalize(XfNormal(mInv, si->shN));
    si->shDpdu = XfVector(m, si->shDpdu);
    si->shN = Faceforward(si->shN, si->n);
}
DEV void InteractionToWorld(const mi_instance &in, SurfaceInteraction *si) { InteractionToWorld(in.i2w, in.w2i, si); }
DEV void ShadingToWorld(const float *m, const float *mInv, TriShading *ts) {
    ts->dpdv = XfVector(m, ts->dpdv);
    ts->shDpdv = XfVector(m, ts->shDpdv);
    ts->dndu = XfNormal(mInv, ts->dndu);
    ts->dndv = XfNormal(mInv, ts->dndv);
}

// Build the SurfaceInteraction of a recorded hit.
// (DISKS: see ShapeSample, d_sampling.h)
template <bool DISKS>
DEV void HitInteraction(const DScene &s, int prim, const V3 &ro, const V3 &rd, float b0, float b1, float b2, SurfaceInteraction *si) {
    const mi_prim p = s.prims[prim];
    if (p.shape >= 0) TriInteraction(s, p.shape, b0, b1, b2, rd, si);
    else { float t; QuadricInteraction<DISKS>(s, ~p.shape, ro, rd, kInfinity, si, &t); }
}

// The hit vertex in world space. A hit inside an object instance: the interaction is built with the ray in the instance's
// space and taken to the world by InstanceToWorld (TransformedPrimitive::Intersect, primitive.cpp:78-92). The only place that
// chooses between the matrices of a moving instance (both of Interpolate(ray.time), held as values) and the record of a static one.
// (The interactions and the moving instance's matrices are objects of their own, neither members nor pointed to by one: they
// are indexed at run time, which keeps them in private memory, and as members they took the whole vertex there: +176 B of
// private segment per instance; a stored pointer to the matrices still cost 16 B.)
// MOTION (TM_INSTANCES instances only): the scene has moving instances -- a hit inside one is carried by the two matrices of
// Interpolate(ray time), held as values. The MOTION = false instances read the instance's record in place.
template <bool MOTION>
struct MovingMatrices { float w2i[MOTION ? 16 : 1], i2w[MOTION ? 16 : 1]; };
template <bool INST, bool MOTION>
struct HitVertex {
    V3 ro, rd;
    int inst;
    V3 roS, rdS;   // the ray in the space the hit shape was intersected in
    DEV const float *W2I(const DScene &s, const MovingMatrices<MOTION> &mm) const { if constexpr (MOTION) return mm.w2i; else return s.instances[inst].w2i; }
    DEV const float *I2W(const DScene &s, const MovingMatrices<MOTION> &mm) const { if constexpr (MOTION) return mm.i2w; else return s.instances[inst].i2w; }
};
// isectObj (may be null): the interaction in the instance's space, set for inst >= 0.
template <bool DISKS, bool INST, bool MOTION>
DEV void BuildHitVertex(const DScene &s, const Pool &pool, uint32_t slot, int prim, const float4 &ray0, const float4 &ray1, bool needIsect,
                        MovingMatrices<MOTION> &mm, HitVertex<INST, MOTION> &hv, SurfaceInteraction *isect, SurfaceInteraction *isectObj) {
    hv.ro = V3(ray0.x, ray0.y, ray0.z); hv.rd = V3(ray1.x, ray1.y, ray1.z);
    hv.inst = -1;
    hv.roS = hv.ro; hv.rdS = hv.rd;
    if constexpr (INST) {
        if (needIsect) hv.inst = pool.I(I_HITINST, slot);
        if (hv.inst >= 0) {
            if constexpr (MOTION) {
                const float time = PathTime(s, pool, slot);
                InstanceW2I(s, hv.inst, time, mm.w2i);
                InstanceI2W(s, hv.inst, time, mm.i2w);
            }
            const Ray ir = XfRay(hv.W2I(s, mm), Ray(hv.ro, hv.rd, kInfinity)); hv.roS = ir.o; hv.rdS = ir.d;
        }
    }
    if (needIsect) { const float4 hr = pool.R(R_HIT, slot); HitInteraction<DISKS>(s, prim, hv.roS, hv.rdS, hr.y, hr.z, hr.w, isect); }
    if constexpr (INST) {
        if (hv.inst >= 0) {
            if (isectObj) *isectObj = *isect;
            InteractionToWorld(hv.I2W(s, mm), hv.W2I(s, mm), isect);
        }
    }
}

// (the shading kernel's dimensions start after the camera sample's, so dim >= 5 here)

// ------------------------------------------------------------------ shade
// One path vertex per lane, for the slots of one material class (queue built by
// k_extend: NL = 2 for materials with <= 2 lobes, NL = 8 otherwise -- "sorted" shading:
// a wave runs one class of BSDF code and the common class keeps its lobe lists in
// registers). Spectra are streamed bin by bin; each of the three spectral passes
// (light sample, MIS sample, continuation) computes its values and its black/non-black
// decision in one sweep.
// The path's throughput quad c (see F_BETA_ONE).
DEV float4 LoadBeta(const Pool &pool, int c, uint32_t slot, bool betaOne) {
    float4 bt = make_float4(1.f, 1.f, 1.f, 1.f);
    if (!betaOne) bt = pool.Q(Q_BETA + c, slot);
    return bt;
}

// Whole-line stores of a spectrum from a shading wave. The memory side takes a store instruction as it comes: 64 lanes
// each storing 16 B of its own path's line leave L2 as 64 partial 64-B writes, and a spectrum written quad by quad
// costs 8 x 64 B of write traffic for 128 B of data (PMC: k_shade wrote 1.66 KB per vertex for 0.36 KB of state). So
// the lanes park their quads in an LDS tile and the wave stores them eight lanes per path, every store instruction
// covering whole 128-B lines. Works from divergent code: only the lanes that are active at the call take part, the
// k-th group of eight active lanes storing the lines of the k-th, (k+G)-th, ... path that has something to store.
struct SpectrumTile {
    float4 q[NQ][BLOCK];
    int slotOf[BLOCK];
    unsigned char laneOf[BLOCK], specOf[BLOCK];
};
// (`spectrum` may differ from lane to lane: it travels with the path)
DEV void StoreSpectrumLines(SpectrumTile &t, const Pool &pool, int spectrum, uint32_t slot, bool wrote) {
    const int lane = threadIdx.x & 63, wbase = threadIdx.x & ~63;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const unsigned long long active = __ballot(1), wmask = __ballot(wrote);
    const int nW = __popcll(wmask), nGroups = __popcll(active) >> 3;
    if (nGroups == 0) {   // fewer than eight lanes here: each stores its own quads
        if (wrote) for (int c = 0; c < NQ; ++c) pool.Q(spectrum + c, slot) = t.q[c][threadIdx.x];
        return;
    }
    if (wrote) {
        const int rw = __popcll(wmask & lt);
        t.slotOf[wbase + rw] = (int)slot;
        t.laneOf[wbase + rw] = (unsigned char)lane;
        t.specOf[wbase + rw] = (unsigned char)spectrum;
    }
    // (the exchange stays inside the wave -- rows wbase .. wbase + 63 -- and a wave's LDS accesses complete in order: the
    // fences only keep the compiler from moving them. At workgroup scope each one was also a wait for every load and store
    // the wave had in flight, the second one for the line stores just issued)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the tile and the list are written before they are read
    __builtin_amdgcn_wave_barrier();
    const int ra = __popcll(active & lt), g = ra >> 3, c = ra & 7;
    if (g < nGroups)
        for (int e = g; e < nW; e += nGroups)
            pool.Q((int)t.specOf[wbase + e] + c, (uint32_t)t.slotOf[wbase + e]) = t.q[c][wbase + t.laneOf[wbase + e]];
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // ... and read before the tile is reused
    __builtin_amdgcn_wave_barrier();
}

#ifndef MIPT_SHADE_WAVES_PER_EU
#define MIPT_SHADE_WAVES_PER_EU 4
#endif

// LENS (textured instances only, chosen per launch for a realistic camera in front of textures: DScene::lensDiff): the
// camera ray's differentials are loaded from the pool planes k_generate wrote (P_LENSDIFF); the LENS = false instances hold
// no trace of that and compile to the code they were.
// k_shade's own note beside the flags it is forming: the vertex has a dark MIS ray, which goes to the MIS queue but not into
// the state word (StateWord keeps FLAG_BITS bits).
constexpr int SHADE_DARK_RAY = 1 << FLAG_BITS;

// ---- the stages of a vertex, in k_shade's order. Every routine is inlined and templated on the axes it reads.
// Queue entry: the grid covers the queues of `classes` back to back, each padded to whole blocks.
struct ShadeEntry { int cls; unsigned count; uint32_t qi; };   // the class (-1: past the last queue), its queue's length, the lane's index in it
DEV ShadeEntry ShadeQueueEntry(const DevCounters *ctr, unsigned classes) {
    ShadeEntry e = {-1, 0u, 0u};
    unsigned blk = blockIdx.x;
    for (int c = 0; c < MAX_CLASSES; ++c) {
        if (!((classes >> c) & 1)) continue;
        const unsigned n = ctr->shadeCount[c].v, nb = (n + BLOCK - 1) / BLOCK;
        if (blk < nb) { e.cls = c; e.count = n; break; }
        blk -= nb;
    }
    e.qi = blk * BLOCK + threadIdx.x;
    return e;
}
// Path head: the state word (flags | bounces | sampler dimension, StateWord) unpacked once, and the hit primitive.
struct PathHead {
    int word, flags, bounces, dim, prim, lPlane;   // lPlane: the line that holds the path's L
    bool lZero, betaOne, found, emitCheck;         // emitCheck: the vertex may show emitted light, path.cpp:91
};
DEV PathHead LoadPathHead(const Pool &pool, uint32_t slot) {
    PathHead h;
    h.word = pool.I(I_FLAGS, slot);
    h.flags = h.word & FLAG_MASK; h.bounces = StateBounces(h.word); h.dim = StateDim(h.word);
    h.lZero = (h.flags & F_L_ZERO) != 0; h.betaOne = (h.flags & F_BETA_ONE) != 0; h.lPlane = LPlane(h.flags);
    h.prim = pool.I(I_HITPRIM, slot);
    h.found = h.prim >= 0;
    h.emitCheck = h.bounces == 0 || (h.flags & F_SPECULAR);
    return h;
}

// L += beta * Le over the path's eight quads; `leQuad(c)` is the emitter's Le, quad c.
template <typename LeQuad>
DEV void AddEmitted(const Pool &pool, uint32_t slot, int lPlane, bool betaOne, bool lZero, LeQuad leQuad) {
#pragma unroll 1
    for (int c = 0; c < NQ; ++c) {
        const float4 bt = LoadBeta(pool, c, slot, betaOne);
        float4 L4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (!lZero) L4 = pool.Q(lPlane + c, slot);
        const float4 Le = leQuad(c);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int b = 4 * c + k;
            if (b < MI_NSPEC) Set4(L4, k, Get4(L4, k) + Get4(bt, k) * Get4(Le, k));
        }
        pool.Q(lPlane + c, slot) = L4;
    }
}
// Emitted light at the vertex, path.cpp:91-101: the hit emitter's, or scene.infiniteLights' for an escaped ray. Returns lZero.
template <unsigned TM>
DEV bool EmittedLight(const DScene &s, const Pool &pool, uint32_t slot, const PathHead &h, const V3 &n, const V3 &rd) {
    bool lZero = h.lZero;
    if (h.emitCheck && h.found) {
        const int li = s.prims[h.prim].area_light;
        if (li >= 0) {
            const mi_light &l = s.lights[li];
            if (l.two_sided || Dot(n, -rd) > 0) {
                AddEmitted(pool, slot, h.lPlane, h.betaOne, lZero, [&](int c) -> float4 { return LoadSpec4(l.L, c); });
                lZero = false;
            }
        }
    }
    if (h.emitCheck && !h.found) {
        for (int il = 0; TM_LIGHT(TM, MI_LIGHT_INFINITE) && il < s.nInfiniteLights; ++il) {
            const IllumRGB le = InfiniteLe(s, s.lights[s.infiniteLights[il]], rd);
            AddEmitted(pool, slot, h.lPlane, h.betaOne, lZero, [&](int c) -> float4 {
                float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (4 * c + k < MI_NSPEC) Set4(q, k, IllumBin(s, le, 4 * c + k));
                return q;
            });
            lZero = false;
        }
    }
    return lZero;
}

// An interface without BSDF: the path continues through it, path.cpp:108-113. Flags and bounce count stay as they are, but
// the spawned ray has no differentials.
DEV void PassThroughInterface(const Pool &pool, uint32_t slot, const PathHead &h, const SurfaceInteraction &isect, const V3 &rd) {
    Ray r = SpawnRay(isect, rd);
    pool.R(R_RAY0, slot) = make_float4(r.o.x, r.o.y, r.o.z, r.tMax);
    if (h.flags & F_DIFF) pool.I(I_FLAGS, slot) = h.word & ~F_DIFF;
}

// SurfaceInteraction::ComputeDifferentials, interaction.cpp:99-143, for a camera ray. LENS: the lens camera's offset rays,
// which k_generate stored; otherwise the perspective camera's, static or animated.
template <bool LENS>
DEV TexDifferentials VertexDifferentials(const DScene &s, const Pool &pool, uint32_t slot, const V3 &ro, const V3 &rd, const SurfaceInteraction &isect, const V3 &dpdv) {
    if constexpr (LENS) {
        CamDifferentials cd;
        cd.rxOrigin = V3(pool.F(P_LENSDIFF + 0, slot), pool.F(P_LENSDIFF + 1, slot), pool.F(P_LENSDIFF + 2, slot));
        cd.ryOrigin = V3(pool.F(P_LENSDIFF + 3, slot), pool.F(P_LENSDIFF + 4, slot), pool.F(P_LENSDIFF + 5, slot));
        cd.rxDirection = V3(pool.F(P_LENSDIFF + 6, slot), pool.F(P_LENSDIFF + 7, slot), pool.F(P_LENSDIFF + 8, slot));
        cd.ryDirection = V3(pool.F(P_LENSDIFF + 9, slot), pool.F(P_LENSDIFF + 10, slot), pool.F(P_LENSDIFF + 11, slot));
        return ComputeDifferentials(isect.p, isect.n, isect.dpdu, dpdv, cd);
    } else {
        float lu = 0.f, lv = 0.f;
        // CameraToWorld for the offset rays: one call of CameraDifferentials on one local array
        float c2w[16];
        if (s.camera.animated) {   // (uniform) the camera sample's time and lens position again, and the transform at that time
            const int pixw = pool.I(I_PIXEL, slot);
            float cu0, cu1, tu;
            CameraSampleDims<true>(s, (int)(short)(pixw & 0xffff), pixw >> 16, (long long)pool.I(I_SAMPLE, slot), &cu0, &cu1, &lu, &lv, nullptr, &tu);
            MovingCameraToWorld(s.cameraMotion, lerpf(tu, s.camera.shutter_open, s.camera.shutter_close), c2w);
        } else {
            if (s.camera.lens_radius > 0) {   // the camera sample's lens position again
                const int pixw = pool.I(I_PIXEL, slot);
                float cu0, cu1;
                CameraSampleDims(s, (int)(short)(pixw & 0xffff), pixw >> 16, (long long)pool.I(I_SAMPLE, slot), &cu0, &cu1, &lu, &lv);
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) c2w[i] = s.camera.camera_to_world[i];
        }
        const CamDifferentials cd = CameraDifferentials(s, c2w, pool.F(P_FILMX, slot), pool.F(P_FILMY, slot), lu, lv, ro, rd, s.invSqrtSpp);
        return ComputeDifferentials(isect.p, isect.n, isect.dpdu, dpdv, cd);
    }
}

// The textured roughness and sigma of the material at the hit, into the frame's overrides:
// `rough = roughness->Evaluate(*si); if (remapRoughness) rough = RoughnessToAlpha(rough)` (plastic.cpp:57-62 ...).
// Returns whether the raw roughnesses (MI_ROUGH_GLASS: the values before the remap) are both 0.
template <bool NOISE>
DEV bool RoughnessOverrides(const DScene &s, const mi_material *mat, float u, float v, const V3 &p, const TexDifferentials &td, BSDFFrame &fr) {
    float rawU = mat->bxdf[0].p[6], rawV = mat->bxdf[0].p[7];
    if (mat->rough_flags & MI_ROUGH_DISNEY) {   // `Float rough = roughness->Evaluate(*si)`, disney.cpp:491
        fr.ov.disney = true;
        fr.ov.rough = EvalFloatImageTexture<NOISE>(s, mat->rough_tex[0], u, v, p, td);
    } else
    if (mat->rough_tex[0] >= 0) {
        const float rv = EvalFloatImageTexture<NOISE>(s, mat->rough_tex[0], u, v, p, td);
        fr.ov.u = (mat->rough_flags & MI_ROUGH_REMAP) ? RoughnessToAlpha(rv) : rv;
        fr.ov.onU = true;
        rawU = rv;
    }
    if (mat->rough_tex[1] >= 0) {
        if (mat->rough_tex[1] == mat->rough_tex[0]) { fr.ov.v = fr.ov.u; rawV = rawU; }
        else {
            const float rv = EvalFloatImageTexture<NOISE>(s, mat->rough_tex[1], u, v, p, td);
            fr.ov.v = (mat->rough_flags & MI_ROUGH_REMAP) ? RoughnessToAlpha(rv) : rv;
            rawV = rv;
        }
        fr.ov.onV = true;
    }
    if (mat->sigma_tex >= 0) {   // `Float sig = Clamp(sigma->Evaluate(*si), 0, 90)`, matte.cpp:57; OrenNayar's constructor
        const float sig = clampf(EvalFloatImageTexture<NOISE>(s, mat->sigma_tex, u, v, p, td), 0.f, 90.f);
        if (sig == 0) fr.ov.sigMode = 2;
        else {
            const float sigma = (kPi / 180) * sig, sigma2 = sigma * sigma;
            fr.ov.sigMode = 1;
            fr.ov.sigA = 1.f - (sigma2 / (2.f * (sigma2 + 0.33f)));
            fr.ov.sigB = 0.45f * sigma2 / (sigma2 + 0.09f);
        }
    }
    return rawU == 0 && rawV == 0;
}

// Which lobes the material adds at this hit: its lobe textures evaluated into `lt`, a lobe kept when the spectrum its rule
// tests is not black (matte.cpp:55-63, plastic.cpp:52-68, uber.cpp:60-100, ...).
template <int NL, bool NOISE>
DEV unsigned LobePresenceMask(const DScene &s, const mi_material *mat, float u, float v, const V3 &p, const TexDifferentials &td, LobeTexT<NL> &lt) {
    unsigned mask = 0u;
    for (int i = 0; i < mat->n_bxdfs; ++i) {
        const mi_lobe_tex ltx = mat->tex[i];
        if (ltx.tex_R < 0 && ltx.tex_S < 0) { mask |= 1u << i; continue; }
        if (i >= NL) continue;
        if (ltx.tex_R >= 0) {
            lt.r[i] = EvalImageTexture<NOISE>(s, ltx.tex_R, u, v, p, td);
            if (ltx.rule == MI_LOBE_METAL) lt.hasK |= 1u << i;   // (k's texture: the lobe's R stays the constant)
            else lt.hasR |= 1u << i;
            if (ltx.flags & MI_LOBE_TEX_MUL_R) lt.mulR |= 1u << i;
        }
        if (ltx.tex_S >= 0) {
            lt.s[i] = EvalImageTexture<NOISE>(s, ltx.tex_S, u, v, p, td);
            lt.hasS |= 1u << i;
            if (ltx.flags & MI_LOBE_TEX_MUL_S) lt.mulS |= 1u << i;
        }
        lt.rules |= (unsigned)(ltx.rule & 15) << (4 * i);
        if (ltx.rule >= MI_LOBE_ALWAYS) {   // "disney": lobes are added whatever the colour is
            if (ltx.rule >= MI_LOBE_DISNEY_SHEEN && ltx.rule <= MI_LOBE_DISNEY_STRANS && lt.lum == 0.f) {   // lum = c.y(), once per vertex (every lobe has the same colour)
                float yy = 0.f;
                for (int b = 0; b < MI_NSPEC; ++b) yy += SpecYBinAccum(s, b, TexBin(lt.basis, lt.textures, lt.r[i], b));
                lt.lum = YScale(yy);
            }
            mask |= 1u << i;
            continue;
        }
        // (the spectrum the material tests with IsBlack(), a quad of bins at a time; only what the lobe's rule reads)
        unsigned rNZ = 0u, sNZ = 0u, texNZ = 0u;
        auto orQuad = [](unsigned &acc, const float4 &q, int c) {
            OrNonZero(acc, q.x); OrNonZero(acc, q.y); OrNonZero(acc, q.z);
            if (c != NQ - 1) OrNonZero(acc, q.w);   // bin 31 does not exist
        };
#pragma unroll 1
        for (int c = 0; c < NQ; ++c) {
            if (ltx.rule != MI_LOBE_IF_TEX) orQuad(rNZ, TexturedQuad(lt, mat->bxdf[i], i, 0, c), c);
            if (ltx.rule == MI_LOBE_IF_R_OR_S) orQuad(sNZ, TexturedQuad(lt, mat->bxdf[i], i, 1, c), c);
            if (ltx.rule == MI_LOBE_IF_TEX) {
                if (ltx.tex_R >= 0) orQuad(texNZ, TexQuad(lt.basis, lt.textures, lt.r[i], c), c);
                if (ltx.tex_S >= 0) orQuad(texNZ, TexQuad(lt.basis, lt.textures, lt.s[i], c), c);
            }
        }
        const bool rNonBlack = rNZ != 0u, sNonBlack = sNZ != 0u, texNonBlack = texNZ != 0u;
        const bool present = ltx.rule == MI_LOBE_IF_R_OR_S ? (rNonBlack || sNonBlack) : (ltx.rule == MI_LOBE_IF_TEX ? texNonBlack : rNonBlack);
        if (present) mask |= 1u << i;
    }
    return mask;
}

// Material::ComputeScatteringFunctions with image textures: evaluate them at the hit (which Bump() may move), fill the
// frame's overrides and lobe mask and the lobe textures.
template <int NL, unsigned TM, bool LENS, bool MOTION>
DEV void TexturedScattering(const DScene &s, const Pool &pool, uint32_t slot, const PathHead &h,
                            const HitVertex<(TM & TM_INSTANCES) != 0, MOTION> &hv, const MovingMatrices<MOTION> &mm, SurfaceInteraction &isect, const SurfaceInteraction &isectObj,
                            const mi_material *mat, BSDFFrame &fr, LobeTexT<NL> &lt) {
    constexpr bool DISKS = TM_HOLDS_DISKS(TM), NOISE = TM_HOLDS_NOISE(TM);
    lt.hasR = lt.hasS = lt.mulR = lt.mulS = 0u;
    lt.rules = 0u; lt.lum = 0.f; lt.hasK = 0u;
    lt.basis = s.rgbIllum; lt.textures = s.textures;
    float u = 0.f, v = 0.f;
    TriShading tsh;
    bool haveUV = false;
    if (mat->textured) {
        const int shape = s.prims[h.prim].shape;
        if (shape >= 0) {
            const float4 hr = pool.R(R_HIT, slot);
            TriTexCoords(s, shape, hr.y, hr.z, hr.w, hv.inst >= 0 ? isectObj : isect, &u, &v, &tsh);
            haveUV = true;
        } else if (DISKS && IsDisk(s, ~shape))
            haveUV = DiskTexCoords(s.disks[~shape - s.nSpheres], hv.roS, hv.rdS, &u, &v, &tsh);
        else
            haveUV = SphereTexCoords(s.spheres[~shape], hv.roS, hv.rdS, &u, &v, &tsh);
        if constexpr ((TM & TM_INSTANCES) != 0) {
            if (hv.inst >= 0) ShadingToWorld(hv.I2W(s, mm), hv.W2I(s, mm), &tsh);
        }
    }
    if (haveUV) {
        TexDifferentials td;
        td.dudx = td.dvdx = td.dudy = td.dvdy = 0;
        td.dpdx = td.dpdy = V3(0, 0, 0);
        if (h.flags & F_DIFF) td = VertexDifferentials<LENS>(s, pool, slot, hv.ro, hv.rd, isect, tsh.dpdv);
        if (mat->bump_tex >= 0) Bump<NOISE>(s, mat->bump_tex, u, v, td, tsh, &isect);   // `if (bumpMap) Bump(bumpMap, si)`
        const bool rawSmooth = RoughnessOverrides<NOISE>(s, mat, u, v, isect.p, td, fr);
        unsigned mask = LobePresenceMask<NL, NOISE>(s, mat, u, v, isect.p, td, lt);
        if (mat->rough_flags & MI_ROUGH_GLASS) mask &= rawSmooth ? 1u : ~1u;   // glass.cpp:66: `isSpecular = urough == 0 && vrough == 0` at this hit; lobe 0 is the FresnelSpecular one
        fr.mask = mask;
    }
}

// ---- the pieces of a spectral pass (the divisor chain and the straight-line quad's pieces: d_bsdf.h, PdfChain and StraightPass)
// f of the evaluated direction, quad c: summed into the lane's tile column (ACCUM), or formed from the lobe list.
template <int NL, unsigned TM, bool ACCUM>
DEV float4 FQuad(const SpectrumTile &tile, const BSDFEvalT<NL> &ev, const mi_bxdf *bx, int c, const LobeTexT<NL> *ltp) {
    if constexpr (ACCUM) return tile.q[c][threadIdx.x];
    else return EvalQuad<NL, TM>(ev, bx, c, ltp);
}

// Commit: the vertex's final flags and state word, and which ray queues the slot joins. Returns 1 for a direct-lighting
// estimate that is already known to be black.
DEV unsigned CommitVertex(const DScene &s, const Pool &pool, uint32_t slot, const PathHead &h, int newFlags, bool finished, bool lZero, bool betaWritten,
                          int dimNow, bool *wantShadow, bool *wantMis, bool *wantDark) {
    unsigned zeroNow = 0;
    if (finished) newFlags = (newFlags & (F_NEE | F_SHADOW | F_MIS | F_CAND | F_NEE_NZ | SHADE_DARK_RAY)) | F_FINISHED;
    else newFlags |= F_ALIVE;
    if (lZero) newFlags |= F_L_ZERO;
    newFlags |= h.flags & F_L_IN_B;
    if (h.betaOne && !betaWritten) newFlags |= F_BETA_ONE;
    *wantShadow = (newFlags & F_SHADOW) != 0;
    // (a dark ray has a queue of its own where k_trav<3> serves the live ones; with k_trav<2> both share misQ)
    *wantDark = s.misAny && (newFlags & SHADE_DARK_RAY) != 0;
    *wantMis = (newFlags & F_MIS) != 0 || (!s.misAny && (newFlags & SHADE_DARK_RAY) != 0);
    // a direct-lighting estimate with neither ray pending (a dark MIS ray is none) is already known to be black
    if ((newFlags & F_NEE) && !*wantShadow && !(newFlags & F_MIS)) { ++zeroNow; newFlags &= ~F_NEE; }
    pool.I(I_FLAGS, slot) = StateWord(newFlags, finished ? h.bounces : h.bounces + 1, dimNow);
    return zeroNow;
}

// What an instance compiles its spectral passes as.
template <int NL, unsigned TM> constexpr bool ShadeSimpleSpectra = NL <= 2 && TM_SIMPLE_KINDS(TM);   // the straight-line passes (d_bsdf.h, SimpleLobes)
// more than two lobes: f is summed lobe by lobe into the lane's column of the spectrum tile (AccumulateF, d_bsdf.h)
template <int NL, unsigned TM> constexpr bool ShadeAccum = NL > 2 || (TM & TM_TEXTURED) != 0;   // (image-textured lobes too: their spectra quad by quad, TexturedQuad)
// The lane's column of the spectrum tile, as AccumulateF reads and writes it.
struct TileColumnRead { const SpectrumTile &t; DEV float4 operator()(int c) const { return t.q[c][threadIdx.x]; } };
struct TileColumnWrite { SpectrumTile &t; DEV void operator()(int c, const float4 &v) const { t.q[c][threadIdx.x] = v; } };
// Direct lighting, the light-sample term (EstimateDirect, integrator.cpp:107-165): f * Li * weight / pdf into the candidate
// line, the shadow ray. Returns the flags it sets.
template <int NL, unsigned TM>
DEV int LightSampleTerm(const DScene &s, const Pool &pool, SpectrumTile &tile, uint32_t slot, const PathHead &h, const SurfaceInteraction &isect,
                        const BSDFFrame &fr, const mi_material *mat, const LobeTexT<NL> *ltp, bool lZero, const mi_light &light, float uL0, float uL1,
                        const Divisor &selDiv, bool selIsOne) {
    constexpr bool SIMPLE_SPECTRA = ShadeSimpleSpectra<NL, TM>, ACCUM = ShadeAccum<NL, TM>;
    const TileColumnRead rdTile{tile};
    const TileColumnWrite wrTile{tile};
    auto loadBeta = [&](int c) -> float4 { return LoadBeta(pool, c, slot, h.betaOne); };
    const int nonSpec = MI_BSDF_ALL & ~MI_BSDF_SPECULAR;
    int flags = 0;
    const LightSample ls = SampleLi<TM>(s, light, isect, uL0, uL1);
    const float lightPdf = ls.pdf;
    if (lightPdf > 0 && !ls.black) {
        BSDFEvalT<NL> ev;
        if constexpr (ACCUM) AccumulateF<NL, TM>(fr, isect.wo, ls.wi, nonSpec, ltp, rdTile, wrTile);
        else BSDF_f<NL, TM>(fr, isect.wo, ls.wi, nonSpec, &ev);
        const float absdot = AbsDot(ls.wi, isect.shN);
        const float scatteringPdf = BSDF_Pdf<TM>(fr, isect.wo, ls.wi, nonSpec);
        const bool delta = IsDeltaLight<TM_HOLDS_PROJECTION(TM)>(light);
        float weight = 1.f;
        if (!delta) { float pf = 1 * lightPdf, pg = 1 * scatteringPdf; weight = (pf * pf) / (pf * pf + pg * pg); }
        const PdfChain div = MakePdfChain(MakeDivisor(lightPdf), selDiv, selIsOne);
        bool fNonBlack = false, liNonBlack = false, nzAny = false;
        // the path's L so far, quad c: the candidate is L + contribution (F_CAND)
        auto lBase = [&](int c) -> float4 { return lZero ? make_float4(0.f, 0.f, 0.f, 0.f) : pool.Q(h.lPlane + c, slot); };
        auto neeQuad = [&](int c, const float4 &fq, const float4 &Lq) {
            const float4 bt = loadBeta(c), l4 = lBase(c);
            float4 out = l4;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int b = 4 * c + k;
                if (b < MI_NSPEC) {
                    const float f = Get4(fq, k) * absdot;
                    const float Li = Get4(Lq, k);
                    fNonBlack |= (f != 0.f);
                    liNonBlack |= (Li != 0.f);
                    const float Ld = DivChainExact(delta ? f * Li : (f * Li) * weight, div);
                    const float contrib = Get4(bt, k) * Ld;
                    nzAny |= (contrib != 0.f);
                    Set4(out, k, Get4(l4, k) + contrib);
                }
            }
            tile.q[c][threadIdx.x] = out;
        };
        if constexpr (SIMPLE_SPECTRA) {
            // straight-line form (d_bsdf.h, SimpleLobes); a quad in which a quotient leaves DivBy's fast range is redone with DivBy
            const StraightPass<NL> sp = MakeStraightPass<NL, TM>(ev, mat->bxdf, div);
            unsigned accF = 0u, accLi = 0u, accNz = 0u;
            auto quad = [&](int c, auto exactTag) {
                constexpr bool EXACT = decltype(exactTag)::value;
                DivTrack trk;
                const float4 bt = loadBeta(c), l4 = lBase(c);   // (the loads first: f's evaluation covers them)
                const float4 fq = StraightQuadF<NL, TM, EXACT>(sp, true, c, c == NQ - 1, trk);
                float4 Lq = LiQuad<TM>(s, light, ls, c);
                if (c == NQ - 1) Lq.w = 0.f;   // bin 31 does not exist
                unsigned aF = 0u, aLi = 0u, aNz = 0u;
                float o[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float f = Get4(fq, k) * absdot;
                    const float Li = Get4(Lq, k);
                    OrNonZero(aF, f); OrNonZero(aLi, Li);
                    const float x = (f * Li) * weight;   // (weight == 1 for a delta light: x * 1 == x)
                    o[k] = Get4(bt, k) * DivChain<EXACT>(x, div, trk);
                    OrNonZero(aNz, o[k]);
                }
                if (!QuadHolds<EXACT>(trk)) return false;
                tile.q[c][threadIdx.x] = make_float4(l4.x + o[0], l4.y + o[1], l4.z + o[2], l4.w + o[3]);
                accF |= aF; accLi |= aLi; accNz |= aNz;
                return true;
            };
#pragma unroll 1
            for (int c = 0; c < NQ; ++c)
                if (!quad(c, std::false_type{})) quad(c, std::true_type{});
            fNonBlack |= accF != 0u; liNonBlack |= accLi != 0u; nzAny |= accNz != 0u;
        } else {
#pragma unroll 1
            for (int c = 0; c < NQ; ++c) neeQuad(c, FQuad<NL, TM, ACCUM>(tile, ev, mat->bxdf, c, ltp), LiQuad<TM>(s, light, ls, c));
        }
        // the tile holds L + contribution, the candidate (F_CAND): only one whose shadow ray will be traced
        // is ever read
        const bool traced = fNonBlack && liNonBlack;
        StoreSpectrumLines(tile, pool, LOtherPlane(h.flags), slot, traced);
        if (traced) flags |= F_CAND | (nzAny ? F_NEE_NZ : 0);
        if (traced) {  // the shadow ray is traced iff f != 0 (integrator.cpp:138-150)
            Ray sr = SpawnRayTo(isect, ls.pLight);
            pool.R(R_SH0, slot) = make_float4(sr.o.x, sr.o.y, sr.o.z, sr.d.x);
            pool.R(R_SH1, slot) = make_float4(sr.d.y, sr.d.z, 0.f, 0.f);
            flags |= F_SHADOW;
        }
    }
    return flags;
}
// Direct lighting, the BSDF-sample term with MIS (integrator.cpp:167-213): the span of the sampled light along the ray, the
// dark rays, the contribution line, the MIS ray. Returns the flags it sets.
template <int NL, unsigned TM>
DEV int BsdfSampleTerm(const DScene &s, const Pool &pool, SpectrumTile &tile, uint32_t slot, const PathHead &h, const SurfaceInteraction &isect,
                       const BSDFFrame &fr, const mi_material *mat, const LobeTexT<NL> *ltp, const mi_light &light, int lightNum, float uS0, float uS1,
                       const Divisor &selDiv, bool selIsOne) {
    constexpr bool SIMPLE_SPECTRA = ShadeSimpleSpectra<NL, TM>, ACCUM = ShadeAccum<NL, TM>;
    constexpr bool DISKS = TM_HOLDS_DISKS(TM);
    const TileColumnRead rdTile{tile};
    const TileColumnWrite wrTile{tile};
    auto loadBeta = [&](int c) -> float4 { return LoadBeta(pool, c, slot, h.betaOne); };
    const int nonSpec = MI_BSDF_ALL & ~MI_BSDF_SPECULAR;
    int flags = 0;
    if (!IsDeltaLight<TM_HOLDS_PROJECTION(TM)>(light)) {  // BSDF sampling with MIS, integrator.cpp:167-213
        V3 wi;
        float sPdf = 0;
        int sampledType = 0;
        BSDFEvalT<NL> ev;
        V3 wiLocal;
        const bool ok = BSDF_Sample_f<NL, TM, !ACCUM>(fr, isect.wo, &wi, uS0, uS1, &sPdf, nonSpec, &sampledType, &ev, &wiLocal);
        if (ok && sPdf > 0) {
            const float absdot = AbsDot(wi, isect.shN);
            // Pdf_Li has no side effect: evaluate it before knowing whether f is black
            float weight = 1;
            bool go = true;
            float tShape = -1.f;   // a triangle light: where wi meets it
            if (!(sampledType & MI_BSDF_SPECULAR)) {
                const float lp = (TM_LIGHT(TM, MI_LIGHT_INFINITE) && light.type == MI_LIGHT_INFINITE) ? InfinitePdfLi(s, light, wi)
                                                                   : ShapePdf<DISKS>(s, light.shape, light.area, isect, wi, &tShape);
                if (lp == 0) go = false;
                else { float pf = 1 * sPdf, pg = 1 * lp; weight = (pf * pf) / (pf * pf + pg * pg); }
            }
            const bool isEnvLight = TM_LIGHT(TM, MI_LIGHT_INFINITE) && light.type == MI_LIGHT_INFINITE;
            IllumRGB envLe;
            envLe.i1 = envLe.i2 = 0; envLe.w0 = envLe.w1 = envLe.w2 = 0;
            if (isEnvLight && go) envLe = InfiniteLe(s, light, wi);   // light.Le(ray) when the ray escapes
            const PdfChain div = MakePdfChain(MakeDivisor(sPdf), selDiv, selIsOne);
            bool fNonBlack = false;
            // a ray that cannot reach the sampled area light is traced all the same (the reference
            // traces it), but its contribution is never read: a dark ray (MIS_EXCL_DARK)
            const Ray mr = SpawnRay(isect, wi);
            float spanLo = 0.f, spanHi = kInfinity;
            const bool dark = go && !isEnvLight && !RaySpanInBox(mr.o, mr.d, s.lightBounds[2 * lightNum], s.lightBounds[2 * lightNum + 1], &spanLo, &spanHi);
            float misTHi = kInfinity, misWord = __uint_as_float(MIS_EXCL_NONE | (31u << MIS_EXCL_BITS));   // (environment light, dark ray: any hit ends it)
            if (s.misAny && go && !dark && !isEnvLight) {
                // a triangle: Shape::Pdf has intersected it (the same test the traversal runs); a sphere: its span in the
                // dilated bounds. Either way widened by what the float arithmetic of the triangle and box tests can disagree
                // by about where things are along the ray: those work on coordinates relative to the ray's origin, so their
                // absolute error in t grows with the distance of the farthest vertex, a few ulps of it (a ray that starts
                // 1e-3 above a 2000-unit ground plane meets it at a t that is 10 % noise, and the plane's box later than that:
                // tests/test_gpu_parity.py::test_mis_visibility_kernel_verdicts_on_recorded_rays). 64 ulps of the distance to
                // the far corner of the world bound: inside the span the reference's visiting order decides, outside it cannot.
                const float far = maxf(absf(mr.o.x - s.wbMin[0]), absf(s.wbMax[0] - mr.o.x)) + maxf(absf(mr.o.y - s.wbMin[1]), absf(s.wbMax[1] - mr.o.y)) +
                                  maxf(absf(mr.o.z - s.wbMin[2]), absf(s.wbMax[2] - mr.o.z));
#ifdef MIPT_EXP_NO_SPAN_SLACK   // (experiment build; no test scene so far tells it from the default)
                const float slack = 0.f * far;
#else
                const float slack = far * 0x1p-18f;
#endif
                if (tShape > 0.f) MisSpanWords(tShape * (1.f - 1e-5f) - slack, tShape * (1.f + 1e-5f) + slack, (unsigned)s.lightPrim[lightNum], &misTHi, &misWord);
                else MisSpanWords(spanLo * 0.9999f - slack, spanHi + slack, (unsigned)s.lightPrim[lightNum], &misTHi, &misWord);
            }
            if constexpr (ACCUM) {   // f of the sampled direction into the tile (only if something will read it)
                if (go) {
                    if (ev.n > 0) AccumulateSpecular<NL, TM>(ev.lobes[0], mat->bxdf, ltp, rdTile, wrTile);
                    else AccumulateFLocal<NL, TM>(fr, fr.WorldToLocal(isect.wo), wiLocal, Dot(wi, fr.ng) * Dot(isect.wo, fr.ng) > 0, nonSpec, ltp, rdTile, wrTile);
                }
            }
            auto darkQuad = [&](int c, const float4 &fq) {   // (only: is f black? -- that decides whether the ray exists)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (4 * c + k < MI_NSPEC) fNonBlack |= (Get4(fq, k) * absdot != 0.f);
            };
            // (when the light's pdf for wi is 0 the estimate ends here, integrator.cpp:186-187:
            // nothing reads the spectrum then, so it is not formed)
            auto misQuad = [&](int c, const float4 &fq, const float4 &Lq) {
                const float4 bt = loadBeta(c);
                float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int b = 4 * c + k;
                    if (b < MI_NSPEC) {
                        const float f = Get4(fq, k) * absdot;
                        fNonBlack |= (f != 0.f);
                        const float LiB = isEnvLight ? IllumBin(s, envLe, b) : Get4(Lq, k);   // Le of the light if the ray reaches it
                        const float Ld = DivChainExact((f * LiB) * weight, div);  // f * Li * Tr(=1) * weight / scatteringPdf / the light's choice
                        Set4(out, k, Get4(bt, k) * Ld);
                    }
                }
                tile.q[c][threadIdx.x] = out;
            };
            const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (SIMPLE_SPECTRA) {
                const StraightPass<NL> sp = MakeStraightPass<NL, TM>(ev, mat->bxdf, div);
                unsigned accF = 0u;
                if (dark) {
                    auto quad = [&](int c, auto exactTag) {
                        constexpr bool EXACT = decltype(exactTag)::value;
                        DivTrack trk;
                        const float4 fq = StraightQuadF<NL, TM, EXACT>(sp, false, c, c == NQ - 1, trk);   // (f alone: no pdf divides it)
                        unsigned aF = 0u;
#pragma unroll
                        for (int k = 0; k < 4; ++k) OrNonZero(aF, Get4(fq, k) * absdot);
                        if (!QuadHolds<EXACT>(trk)) return false;
                        accF |= aF;
                        return true;
                    };
#pragma unroll 1
                    for (int c = 0; c < NQ; ++c)
                        if (!quad(c, std::false_type{})) quad(c, std::true_type{});
                }
                if (go && !dark) {
                    auto quad = [&](int c, auto exactTag) {
                        constexpr bool EXACT = decltype(exactTag)::value;
                        DivTrack trk;
                        const float4 bt = loadBeta(c);
                        const float4 fq = StraightQuadF<NL, TM, EXACT>(sp, true, c, c == NQ - 1, trk);
                        float4 Lq = isEnvLight ? zero4 : LoadSpec4(light.L, c);
                        if (c == NQ - 1) Lq.w = 0.f;
                        unsigned aF = 0u;
                        float o[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const float f = Get4(fq, k) * absdot;
                            OrNonZero(aF, f);
                            const float LiB = isEnvLight ? ((4 * c + k < MI_NSPEC) ? IllumBin(s, envLe, min(4 * c + k, MI_NSPEC - 1)) : 0.f) : Get4(Lq, k);
                            o[k] = Get4(bt, k) * DivChain<EXACT>((f * LiB) * weight, div, trk);
                        }
                        if (!QuadHolds<EXACT>(trk)) return false;
                        tile.q[c][threadIdx.x] = make_float4(o[0], o[1], o[2], o[3]);
                        accF |= aF;
                        return true;
                    };
#pragma unroll 1
                    for (int c = 0; c < NQ; ++c)
                        if (!quad(c, std::false_type{})) quad(c, std::true_type{});
                }
                fNonBlack |= accF != 0u;
            } else if (go) {   // (dark implies go; one loop, so that f's code is inlined once: two sites had left it an out-of-line call)
#pragma unroll 1
                for (int c = 0; c < NQ; ++c) {
                    const float4 fq = FQuad<NL, TM, ACCUM>(tile, ev, mat->bxdf, c, ltp);
                    if (dark) darkQuad(c, fq);
                    else misQuad(c, fq, isEnvLight ? zero4 : LoadSpec4(light.L, c));
                }
            }
            StoreSpectrumLines(tile, pool, Q_LMIS, slot, go && !dark);   // whole 128-B lines, as for the light sample
            if (fNonBlack && go) {
                // (a dark ray is queued and traced, but the estimate does not wait for it: no F_MIS)
                if (dark) misWord = __uint_as_float(MIS_EXCL_DARK | (31u << MIS_EXCL_BITS));
                pool.R(R_MI0, slot) = make_float4(mr.o.x, mr.o.y, mr.o.z, mr.d.x);
                pool.R(R_MI1, slot) = make_float4(mr.d.y, mr.d.z, misTHi, misWord);
                if (s.nLights > 1 && !dark) pool.I(I_MISLIGHT, slot) = lightNum;   // (one light: k_resolve_mis knows which)
                flags |= dark ? SHADE_DARK_RAY : F_MIS;
            }
        }
    }
    return flags;
}
// Direct lighting: UniformSampleOneLight + EstimateDirect, integrator.cpp:85-215 -- the light choice and the five dimensions of
// the estimate, then its two terms. Returns the flags it sets (F_NEE: the vertex has non-specular lobes and counts as a path).
template <int NL, unsigned TM>
DEV int DirectLighting(const DScene &s, const Pool &pool, SpectrumTile &tile, uint32_t slot, const PathHead &h, const SurfaceInteraction &isect,
                       const BSDFFrame &fr, const mi_material *mat, const LobeTexT<NL> *ltp, bool lZero, PathSampler &ps,
                       const int *__restrict__ pixelPlane, const int *__restrict__ samplePlane) {
    constexpr bool HALTON_ONLY = (TM & TM_SAMPLERS) == 0;
    const int nonSpec = MI_BSDF_ALL & ~MI_BSDF_SPECULAR;
    int flags = 0;
    if (NumComponents(fr, nonSpec) > 0) {
        flags |= F_NEE;
        if (s.nLights > 0) {
            const uint32_t di = LightDistribIndex(s, isect.p);
            float selPdf;
            // the five dimensions of the estimate (light choice, light sample, BSDF sample)
            // (Halton, 32-bit indices: all five in one call -- ScrambledDimensions5, d_sampling.h. The four of the estimate are
            // then there before the light is chosen; the dimension counter still moves as the reference's does, by one here
            // and by four more only where the estimate is made.)
            float u5[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            const bool grouped = HALTON_ONLY && s.index32;
            if (grouped) {
                const Halton5 r = ScrambledDimensions5(HaltonTable(s.haltonDims), (uint32_t)ps.index, ps.dim);
                u5[0] = r.u0; u5[1] = r.u1; u5[2] = r.u2; u5[3] = r.u3; u5[4] = r.u4;
                ps.dim += 1;
            } else u5[0] = Get1D<HALTON_ONLY>(s, ps, pixelPlane, samplePlane, slot);
            const int lightNum = SampleDiscrete(s.ldFunc + (size_t)di * s.nLights, s.ldCdf + (size_t)di * (s.nLights + 1),
                                                s.ldFuncInt[di], (int)s.nLights, u5[0], &selPdf);
            if (selPdf != 0) {
                // uLight = Get2D(), uScattering = Get2D() (integrator.cpp:100-101)
                if (grouped) ps.dim += 4;
                else if constexpr (HALTON_ONLY) {   // (indices beyond 32 bits: the single-dimension routine, one call site)
#pragma unroll 1
                    for (int k = 1; k < 5; ++k) {   // (selects, not u5[k]: an array indexed by a loop counter lives in private memory)
                        const float v = Get1D<true>(s, ps, pixelPlane, samplePlane, slot);
                        u5[1] = k == 1 ? v : u5[1]; u5[2] = k == 2 ? v : u5[2]; u5[3] = k == 3 ? v : u5[3]; u5[4] = k == 4 ? v : u5[4];
                    }
                } else {
                    Get2D<HALTON_ONLY>(s, ps, pixelPlane, samplePlane, slot, &u5[1], &u5[2]);
                    Get2D<HALTON_ONLY>(s, ps, pixelPlane, samplePlane, slot, &u5[3], &u5[4]);
                }
                const float uL0 = u5[1], uL1 = u5[2], uS0 = u5[3], uS1 = u5[4];
                const mi_light &light = s.lights[lightNum];
                const bool selIsOne = (selPdf == 1.f);  // x / 1 == x: skip the division
                const Divisor selDiv = MakeDivisor(selPdf);
                flags |= LightSampleTerm<NL, TM>(s, pool, tile, slot, h, isect, fr, mat, ltp, lZero, light, uL0, uL1, selDiv, selIsOne);
                flags |= BsdfSampleTerm<NL, TM>(s, pool, tile, slot, h, isect, fr, mat, ltp, light, lightNum, uS0, uS1, selDiv, selIsOne);
            }
        }
    }
    return flags;
}
// Continuation, path.cpp:131-184: the BSDF sample for the next direction, the new throughput, Russian roulette, the next ray.
// etaScaleIn: the ray's (R_RAY1.w). Returns the flags it sets; *finished: the path ends here.
template <int NL, unsigned TM>
DEV int Continuation(const DScene &s, const Pool &pool, SpectrumTile &tile, uint32_t slot, const PathHead &h, const SurfaceInteraction &isect,
                     const BSDFFrame &fr, const mi_material *mat, const LobeTexT<NL> *ltp, const V3 &rd, float etaScaleIn, PathSampler &ps,
                     const int *__restrict__ pixelPlane, const int *__restrict__ samplePlane, bool *finished, bool *betaWritten) {
    constexpr bool SIMPLE_SPECTRA = ShadeSimpleSpectra<NL, TM>, ACCUM = ShadeAccum<NL, TM>;
    constexpr bool HALTON_ONLY = (TM & TM_SAMPLERS) == 0;
    const TileColumnRead rdTile{tile};
    const TileColumnWrite wrTile{tile};
    auto loadBeta = [&](int c) -> float4 { return LoadBeta(pool, c, slot, h.betaOne); };
    int flags = 0;
    V3 wo = -rd, wi;
    float pdf = 0;
    int sflags = 0;
    float u2[2] = {0.f, 0.f};
    if (HALTON_ONLY && s.index32) {   // (as in DirectLighting: both dimensions in one call)
        const Halton2 r = ScrambledDimensions2(HaltonTable(s.haltonDims), (uint32_t)ps.index, ps.dim);
        u2[0] = r.u0; u2[1] = r.u1;
        ps.dim += 2;
    } else if constexpr (HALTON_ONLY) {
#pragma unroll 1
        for (int k = 0; k < 2; ++k) {
            const float v = Get1D<true>(s, ps, pixelPlane, samplePlane, slot);
            u2[0] = k == 0 ? v : u2[0]; u2[1] = k == 1 ? v : u2[1];
        }
    } else Get2D<HALTON_ONLY>(s, ps, pixelPlane, samplePlane, slot, &u2[0], &u2[1]);
    const float u0 = u2[0], u1 = u2[1];
    BSDFEvalT<NL> ev;
    V3 wiLocal;
    const bool ok = BSDF_Sample_f<NL, TM, !ACCUM>(fr, wo, &wi, u0, u1, &pdf, MI_BSDF_ALL, &sflags, &ev, &wiLocal);
    if constexpr (ACCUM) {
        if (ok && pdf != 0.f) {
            if (ev.n > 0) AccumulateSpecular<NL, TM>(ev.lobes[0], mat->bxdf, ltp, rdTile, wrTile);
            else AccumulateFLocal<NL, TM>(fr, fr.WorldToLocal(wo), wiLocal, Dot(wi, fr.ng) * Dot(wo, fr.ng) > 0, MI_BSDF_ALL, ltp, rdTile, wrTile);
        }
    }
    bool fNonBlack = false;
    if (ok && pdf != 0.f) {
        const float absdot = AbsDot(wi, isect.shN);
        float etaScale = etaScaleIn;
        if ((sflags & MI_BSDF_SPECULAR) && (sflags & MI_BSDF_TRANSMISSION)) {
            float eta = mat->eta;
            etaScale *= (Dot(wo, isect.n) > 0) ? (eta * eta) : 1 / (eta * eta);
        }
        const PdfChain div = MakePdfChain(MakeDivisor(pdf));
        float maxRR = 0;
        auto contQuad = [&](int c, const float4 &fq) {  // beta *= f * |wi.ns| / pdf (only meaningful when f is not black)
            float4 bt = loadBeta(c);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int b = 4 * c + k;
                if (b < MI_NSPEC) {
                    const float f = Get4(fq, k);
                    fNonBlack |= (f != 0.f);
                    const float nb = Get4(bt, k) * DivChainExact(f * absdot, div);
                    Set4(bt, k, nb);
                    const float rr = nb * etaScale;
                    maxRR = (b == 0) ? rr : maxf(maxRR, rr);
                }
            }
            tile.q[c][threadIdx.x] = bt;
        };
        if constexpr (SIMPLE_SPECTRA) {
            const StraightPass<NL> sp = MakeStraightPass<NL, TM>(ev, mat->bxdf, div);
            unsigned accF = 0u;
            auto quad = [&](int c, auto exactTag) {
                constexpr bool EXACT = decltype(exactTag)::value;
                DivTrack trk;
                const float4 bt = loadBeta(c);
                const float4 fq = StraightQuadF<NL, TM, EXACT>(sp, true, c, c == NQ - 1, trk);
                unsigned aF = 0u;
                float o[4], mr = maxRR;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float f = Get4(fq, k);
                    OrNonZero(aF, f);
                    o[k] = Get4(bt, k) * DivChain<EXACT>(f * absdot, div, trk);
                    const float rr = o[k] * etaScale;
                    if (k == 0) mr = (c == 0) ? rr : maxf(mr, rr);
                    else if (k < 3) mr = maxf(mr, rr);
                    else mr = (c == NQ - 1) ? mr : maxf(mr, rr);
                }
                if (c == NQ - 1) o[3] = bt.w;   // (the pad word keeps what it held)
                if (!QuadHolds<EXACT>(trk)) return false;
                tile.q[c][threadIdx.x] = make_float4(o[0], o[1], o[2], o[3]);
                accF |= aF;
                maxRR = mr;
                return true;
            };
#pragma unroll 1
            for (int c = 0; c < NQ; ++c)
                if (!quad(c, std::false_type{})) quad(c, std::true_type{});
            fNonBlack |= accF != 0u;
        } else {
#pragma unroll 1
            for (int c = 0; c < NQ; ++c) contQuad(c, FQuad<NL, TM, ACCUM>(tile, ev, mat->bxdf, c, ltp));
        }
        // (the new throughput is stored below, once it is known that a later vertex will read it)
        bool killed = false;
        if (fNonBlack) {
            // Russian roulette, path.cpp:176-184
            if (maxRR < s.rrThreshold && h.bounces > 3) {
                float q = maxf(.05f, 1 - maxRR);
                float uRR;
                if (HALTON_ONLY && s.index32) uRR = ScrambledDimensions1(HaltonTable(s.haltonDims), (uint32_t)ps.index, ps.dim++);
                else uRR = Get1D<HALTON_ONLY>(s, ps, pixelPlane, samplePlane, slot);
                if (uRR < q) killed = true;
                else {
                    const Divisor inv = MakeDivisor(1 - q);
#pragma unroll 1
                    for (int c = 0; c < NQ; ++c) {
                        float4 bt = tile.q[c][threadIdx.x];   // (the new beta, parked in the tile)
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (4 * c + k < MI_NSPEC) Set4(bt, k, DivBy(Get4(bt, k), inv));
                        tile.q[c][threadIdx.x] = bt;
                    }
                }
            }
        }
        // the next vertex reads the throughput if it is shaded (bounces + 1 < maxDepth) or may show emitted
        // light (after a specular bounce, path.cpp:91-101); a path that ends here, or whose last ray only
        // has to be traced, leaves none behind
        const bool needBeta = fNonBlack && !killed && (h.bounces + 1 < s.maxDepth || (sflags & MI_BSDF_SPECULAR));
        StoreSpectrumLines(tile, pool, Q_BETA, slot, needBeta);
        if (needBeta) *betaWritten = true;
        if (fNonBlack) {
            if (killed) *finished = true;
            else {
                const Ray nr = SpawnRay(isect, wi);
                pool.R(R_RAY0, slot) = make_float4(nr.o.x, nr.o.y, nr.o.z, nr.tMax);
                pool.R(R_RAY1, slot) = make_float4(nr.d.x, nr.d.y, nr.d.z, etaScale);
                if (sflags & MI_BSDF_SPECULAR) flags |= F_SPECULAR;
            }
        }
    }
    if (!(ok && pdf != 0.f && fNonBlack)) *finished = true;
    return flags;
}
template <int NL, unsigned TM, bool LENS = false, bool MOTION = false>
__global__ void __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(MIPT_SHADE_WAVES_PER_EU, 8))) k_shade(DScene s, Pool pool, DevCounters *ctr, unsigned classes) {
    const ShadeEntry entry = ShadeQueueEntry(ctr, classes);
    constexpr bool HALTON_ONLY = (TM & TM_SAMPLERS) == 0;
    constexpr bool DISKS = TM_HOLDS_DISKS(TM);   // (a scene with disks is shaded by the general instances alone: ShadeInstanceOf)
    __shared__ SpectrumTile tile;
    unsigned totalPaths = 0, pathLen = 0, zeroNow = 0;
    bool wantShadow = false, wantMis = false, wantDark = false;
    uint32_t slot = 0;
    if (entry.cls >= 0 && entry.qi < entry.count) {
        slot = pool.shadeQ[(size_t)entry.cls * pool.n + entry.qi];
        const PathHead h = LoadPathHead(pool, slot);
        bool betaWritten = false;
        int dimNow = h.dim;
        // the ray and the interaction are needed by vertices that will be shaded or may show emitted light; an escaped
        // ray without environment lights and a path at its last vertex need neither (k_resolve_extend ends those itself and
        // does not queue them, EndsUnshaded: what this kernel writes for one, below, is FinishedWord)
        const bool needIsect = h.found && (h.bounces < s.maxDepth || h.emitCheck);
        const bool needRay = needIsect || (!h.found && h.emitCheck && TM_LIGHT(TM, MI_LIGHT_INFINITE) && s.nInfiniteLights > 0);
        float4 ray0 = make_float4(0.f, 0.f, 0.f, 0.f), ray1 = make_float4(0.f, 0.f, 1.f, 1.f);
        if (needRay) { ray0 = pool.R(R_RAY0, slot); ray1 = pool.R(R_RAY1, slot); }
        MovingMatrices<MOTION> mm;
        HitVertex<(TM & TM_INSTANCES) != 0, MOTION> hv;
        SurfaceInteraction isect, isectObj;
        BuildHitVertex<DISKS>(s, pool, slot, h.prim, ray0, ray1, needIsect, mm, hv, &isect, &isectObj);
        const V3 &rd = hv.rd;
        bool lZero = EmittedLight<TM>(s, pool, slot, h, isect.n, rd);
        bool finished = !h.found || h.bounces >= s.maxDepth;
        const bool passThrough = !finished && s.prims[h.prim].material < 0;
        if (passThrough) PassThroughInterface(pool, slot, h, isect, rd);
        int newFlags = 0;
        if (!finished && !passThrough) {
            const mi_material *mat = &s.materials[s.prims[h.prim].material];
            BSDFFrame fr;
            fr.m = mat;
            fr.mask = 0xffu;
            fr.ov.u = fr.ov.v = 0.f; fr.ov.onU = fr.ov.onV = false;
            fr.ov.sigMode = 0; fr.ov.sigA = fr.ov.sigB = 0.f;
            fr.ov.disney = false; fr.ov.rough = 0.f;
            LobeTexT<NL> lt;
            const LobeTexT<NL> *ltp = nullptr;
            if constexpr ((TM & TM_TEXTURED) != 0) {
                TexturedScattering<NL, TM, LENS, MOTION>(s, pool, slot, h, hv, mm, isect, isectObj, mat, fr, lt);
                ltp = &lt;
            }
            // BSDF ctor, reflection.h:170-176 (after Bump(): it reads the shading geometry)
            fr.ns = isect.shN; fr.ng = isect.n; fr.ss = Normalize(isect.shDpdu); fr.ts = Cross(fr.ns, fr.ss);
            PathSampler ps;
            ps.index = (uint32_t)pool.I(I_IDXLO, slot);
            if (!s.index32) ps.index |= (uint64_t)(uint32_t)pool.I(I_IDXHI, slot) << 32;
            ps.dim = dimNow;
            if constexpr (!HALTON_ONLY) { if (IsPixelSampler(s)) ps.dim = pool.I(I_DIM, slot); }
            const int *__restrict__ pixelPlane = pool.i + (size_t)I_PIXEL * pool.n, *__restrict__ samplePlane = pool.i + (size_t)I_SAMPLE * pool.n;
            newFlags |= DirectLighting<NL, TM>(s, pool, tile, slot, h, isect, fr, mat, ltp, lZero, ps, pixelPlane, samplePlane);
            if (newFlags & F_NEE) ++totalPaths;
            newFlags |= Continuation<NL, TM>(s, pool, tile, slot, h, isect, fr, mat, ltp, rd, ray1.w, ps, pixelPlane, samplePlane, &finished, &betaWritten);
            dimNow = ps.dim;
            if constexpr (!HALTON_ONLY) { if (IsPixelSampler(s)) { pool.I(I_DIM, slot) = ps.dim; dimNow = 0; } }
            if (!HALTON_ONLY && s.samplerType >= MI_SAMPLER_RANDOM) {   // the stream moves on with the path
                pool.I(I_IDXLO, slot) = (int)(uint32_t)ps.index;
                pool.I(I_IDXHI, slot) = (int)(uint32_t)(ps.index >> 32);
            }
        }
        if (!passThrough) {
            if (finished) pathLen = (unsigned)h.bounces;   // ReportValue(pathLength, bounces): `bounces` at the break of path.cpp's loop
            zeroNow = CommitVertex(s, pool, slot, h, newFlags, finished, lZero, betaWritten, dimNow, &wantShadow, &wantMis, &wantDark);
        }
    }
    __shared__ unsigned sAppend[15];
    unsigned posS, posM, posD;
    BlockReserve3(&ctr->shadowCount.v, wantShadow, &ctr->misCount.v, wantMis, &ctr->darkCount.v, wantDark, sAppend, &posS, &posM, &posD);
    if (wantShadow) pool.shadowQ[posS] = slot;
    if (wantMis) pool.misQ[posM] = slot;
    if (wantDark) pool.darkQ[posD] = slot;
    {   // the three statistics of a wave in one reduction: per lane at most one path, one black estimate and 255 bounces
        unsigned packed = totalPaths | (zeroNow << 8) | (pathLen << 16);
        for (int off = 32; off > 0; off >>= 1) packed += __shfl_down(packed, off, 64);
        if ((threadIdx.x & 63) == 0 && packed) {
            DevStats &st8 = Stats(ctr);
            if (packed & 0xffu) atomicAdd(&st8.totalPaths, (unsigned long long)(packed & 0xffu));
            if ((packed >> 8) & 0xffu) atomicAdd(&st8.zeroRadiancePaths, (unsigned long long)((packed >> 8) & 0xffu));
            if (packed >> 16) atomicAdd(&st8.pathLengthSum, (unsigned long long)(packed >> 16));
        }
    }
}

#if MIPT_HAS_MAIN
// ------------------------------------------------------------------ spatial light distribution (create time)
__global__ void k_build_spatial(DScene s, float *func, float *cdf, float *funcInt, uint32_t nVox) {
    const uint32_t vox = blockIdx.x * blockDim.x + threadIdx.x;
    if (vox >= nVox) return;
    const int nL = (int)s.nLights;
    int pi[3];
    pi[0] = vox % s.nVoxels[0];
    pi[1] = (vox / s.nVoxels[0]) % s.nVoxels[1];
    pi[2] = vox / (s.nVoxels[0] * s.nVoxels[1]);
    float lo[3], hi[3];
    for (int i = 0; i < 3; ++i) {
        float t0 = (float)pi[i] / (float)s.nVoxels[i], t1 = (float)(pi[i] + 1) / (float)s.nVoxels[i];
        float a = lerpf(t0, s.wbMin[i], s.wbMax[i]), b = lerpf(t1, s.wbMin[i], s.wbMax[i]);
        lo[i] = minf(a, b); hi[i] = maxf(a, b);
    }
    float *f = func + (size_t)vox * nL;
    for (int j = 0; j < nL; ++j) f[j] = 0.f;
    const int nSamples = 128;
    for (int i = 0; i < nSamples; ++i) {
        float t[3] = {RadicalInverse(s, 0, i), RadicalInverse(s, 1, i), RadicalInverse(s, 2, i)};
        Interaction intr;
        intr.p = V3(lerpf(t[0], lo[0], hi[0]), lerpf(t[1], lo[1], hi[1]), lerpf(t[2], lo[2], hi[2]));
        intr.wo = V3(1, 0, 0);
        float u0 = RadicalInverse(s, 3, i), u1 = RadicalInverse(s, 4, i);
        for (int j = 0; j < nL; ++j) {
            const mi_light &l = s.lights[j];
            LightSample ls = SampleLi<TM_ALL>(s, l, intr, u0, u1);
            if (ls.pdf > 0) {
                float yy = 0.f;
                if (!ls.black) for (int b = 0; b < MI_NSPEC; ++b) yy += s.cieY[b] * LiBin<TM_ALL>(s, l, ls, b);
                f[j] += YScale(yy) / ls.pdf;
            }
        }
    }
    float sumContrib = 0;
    for (int j = 0; j < nL; ++j) sumContrib += f[j];
    float avgContrib = sumContrib / (float)((size_t)nSamples * (size_t)nL);
    float minContrib = (avgContrib > 0) ? (float)(.001 * (double)avgContrib) : 1.f;
    for (int j = 0; j < nL; ++j) f[j] = maxf(f[j], minContrib);
    // Distribution1D ctor, sampling.h:57-70
    float *c = cdf + (size_t)vox * (nL + 1);
    c[0] = 0;
    for (int j = 1; j < nL + 1; ++j) c[j] = c[j - 1] + f[j - 1] / nL;
    float fi = c[nL];
    if (fi == 0) { for (int j = 1; j < nL + 1; ++j) c[j] = (float)j / (float)nL; }
    else { for (int j = 1; j < nL + 1; ++j) c[j] /= fi; }
    funcInt[vox] = fi;
}

// ------------------------------------------------------------------ pixel samplers' tables (create time)
// ZeroTwoSequenceSampler::StartPixel (zerotwosequence.cpp:53-69) / StratifiedSampler::StartPixel (stratified.cpp:43-58) for every
// pixel at once, one lane per pixel, each with the pixel's own PCG32 stream (mi_sampler_type): all 1D tables, then all 2D
// tables, each scrambled / jittered and shuffled in the reference's order of RNG draws (VanDerCorput / Sobol2D,
// lowdiscrepancy.h:149-227; StratifiedSample1D / 2D, sampling.cpp:42-60; Shuffle, sampling.h:150-157).
DEV uint32_t PcgBounded(uint64_t &state, uint64_t inc, uint32_t b) {   // RNG::UniformUInt32(b), rng.h:112-121
    const uint32_t threshold = (~b + 1u) % b;
    while (true) {
        const uint32_t r = PcgNext(state, inc);
        if (r >= threshold) return r % b;
    }
}
__global__ void k_pixel_tables(DScene s, float *tab1, float *tab2, unsigned long long nPix) {
    const unsigned long long pix = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= nPix) return;
    const int spp = (int)s.samplesPerPixel, dims = s.pixelDims;
    const uint64_t inc = (((uint64_t)pix) << 1u) | 1u;
    uint64_t state = RandomStreamStart(inc);
    const bool zeroTwo = s.samplerType == MI_SAMPLER_ZEROTWO;
    for (int d = 0; d < dims; ++d) {   // the 1D tables
        float *v = tab1 + ((size_t)pix * dims + d) * (size_t)spp;
        if (zeroTwo) {   // VanDerCorput(1, spp, ...): the generator matrix is the bit-reversed identity, C[k] = 2^(31 - k)
            uint32_t x = PcgNext(state, inc);
            for (int i = 0; i < spp; ++i) {
                v[i] = minf((float)x * 0x1p-32f, kOneMinusEpsilon);
                x ^= 0x80000000u >> __builtin_ctz((unsigned)(i + 1));
            }
            for (int i = 0; i < spp; ++i) (void)PcgBounded(state, inc, 1u);   // Shuffle of each sample's single value: one draw apiece
        } else {
            const float invN = 1.f / (float)spp;
            for (int i = 0; i < spp; ++i) {
                const float delta = s.jitter ? PcgFloat(state, inc) : 0.5f;
                v[i] = minf(((float)i + delta) * invN, kOneMinusEpsilon);
            }
        }
        for (int i = 0; i < spp; ++i) {   // Shuffle(v, spp, 1, rng)
            const int other = i + (int)PcgBounded(state, inc, (uint32_t)(spp - i));
            const float t = v[i]; v[i] = v[other]; v[other] = t;
        }
    }
    for (int d = 0; d < dims; ++d) {   // the 2D tables
        float2 *v = reinterpret_cast<float2 *>(tab2) + ((size_t)pix * dims + d) * (size_t)spp;
        if (zeroTwo) {   // Sobol2D(1, spp, ...): second matrix = Pascal's triangle mod 2, column k = column k-1 ^ (column k-1 >> 1)
            uint32_t x0 = PcgNext(state, inc), x1 = PcgNext(state, inc);
            uint32_t col[32];
            col[0] = 0x80000000u;
            for (int k = 1; k < 32; ++k) col[k] = col[k - 1] ^ (col[k - 1] >> 1);
            for (int i = 0; i < spp; ++i) {
                v[i] = make_float2(minf((float)x0 * 0x1p-32f, kOneMinusEpsilon), minf((float)x1 * 0x1p-32f, kOneMinusEpsilon));
                const int k = __builtin_ctz((unsigned)(i + 1));
                x0 ^= 0x80000000u >> k;
                x1 ^= col[k];
            }
            for (int i = 0; i < spp; ++i) (void)PcgBounded(state, inc, 1u);
        } else {
            const float dx = 1.f / (float)s.xSamples, dy = 1.f / (float)s.ySamples;
            int i = 0;
            for (int y = 0; y < s.ySamples; ++y)
                for (int x = 0; x < s.xSamples; ++x, ++i) {
                    const float jx = s.jitter ? PcgFloat(state, inc) : 0.5f;
                    const float jy = s.jitter ? PcgFloat(state, inc) : 0.5f;
                    v[i] = make_float2(minf(((float)x + jx) * dx, kOneMinusEpsilon), minf(((float)y + jy) * dy, kOneMinusEpsilon));
                }
        }
        for (int i = 0; i < spp; ++i) {
            const int other = i + (int)PcgBounded(state, inc, (uint32_t)(spp - i));
            const float2 t = v[i]; v[i] = v[other]; v[other] = t;
        }
    }
}

// ------------------------------------------------------------------ camera rays and texture lookups on their own (mi_pt_camera_rays, mi_pt_texture_*)
// mi_pt_camera_rays: CameraSampleDims and CameraRay as k_generate calls them, one listed sample per thread.
template <bool MOVING>
__global__ void k_camera_rays(DScene s, const int32_t *__restrict__ samples, uint32_t n, float *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int px = samples[3 * i], py = samples[3 * i + 1];
    const long long sampleNum = samples[3 * i + 2];
    float u0, u1, lu, lv, tu = 0.f, time = s.camera.shutter_open;
    CameraSampleDims<MOVING>(s, px, py, sampleNum, &u0, &u1, &lu, &lv, nullptr, &tu);
    Ray ray;
    CameraRay<MOVING>(s, (float)px + u0, (float)py + u1, lu, lv, &ray, tu, &time);
    float *o = out + 8 * (size_t)i;
    o[0] = ray.o.x; o[1] = ray.o.y; o[2] = ray.o.z; o[3] = ray.d.x; o[4] = ray.d.y; o[5] = ray.d.z; o[6] = ray.tMax; o[7] = time;
}

// mi_pt_camera_rays_ex: the same with the ray's weight and its scaled differentials; a realistic camera's through LensCameraRay.
// CAM: the camera's mi_camera_type (the orthographic and environment cameras through OptInCameraRay, d_camera.h).
template <bool MOVING, int CAM>
__global__ void k_camera_rays_ex(DScene s, const int32_t *__restrict__ samples, uint32_t n, int band, float *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int px = samples[3 * i], py = samples[3 * i + 1];
    const long long sampleNum = samples[3 * i + 2];
    float u0, u1, lu, lv, tu = 0.f;
    CameraSampleDims<true>(s, px, py, sampleNum, &u0, &u1, &lu, &lv, nullptr, &tu);   // (the time sample also where no transform waits for it: the ray's time is reported)
    float time = lerpf(tu, s.camera.shutter_open, s.camera.shutter_close);
    const float pfx = (float)px + u0, pfy = (float)py + u1;
    Ray ray;
    float weight = 1.f;
    V3 diff[4];
    if constexpr (CAM == MI_CAMERA_REALISTIC) {
        const float wavelength = s.nBands > 1 ? BandWavelength(s.bandDelta, band) : 550.f;
        weight = LensCameraRay<MOVING>(s, pfx, pfy, lu, lv, tu, wavelength, &ray, &time, diff, s.invSqrtSpp);
    } else if constexpr (CAM == MI_CAMERA_ORTHOGRAPHIC || CAM == MI_CAMERA_ENVIRONMENT) {
        OptInCameraRay<CAM, MOVING>(s, pfx, pfy, lu, lv, tu, &ray, &time, diff, s.invSqrtSpp);   // (every band gets the same ray: neither camera reads the wavelength)
    } else {
        CameraRay<MOVING>(s, pfx, pfy, lu, lv, &ray, tu, &time);
        float m[16];
        if constexpr (MOVING) MovingCameraToWorld(s.cameraMotion, time, m);
        else for (int k = 0; k < 16; ++k) m[k] = s.cameraMotion->camera_to_world[k];
        const CamDifferentials cd = CameraDifferentials(s, m, pfx, pfy, lu, lv, ray.o, ray.d, s.invSqrtSpp);
        diff[0] = cd.rxOrigin; diff[1] = cd.ryOrigin; diff[2] = cd.rxDirection; diff[3] = cd.ryDirection;
    }
    float *o = out + MI_CAMERA_RAY_EX_FLOATS * (size_t)i;
    for (int k = 0; k < MI_CAMERA_RAY_EX_FLOATS; ++k) o[k] = 0.f;
    o[7] = time; o[8] = weight;
    if (weight == 0) return;
    o[0] = ray.o.x; o[1] = ray.o.y; o[2] = ray.o.z; o[3] = ray.d.x; o[4] = ray.d.y; o[5] = ray.d.z; o[6] = ray.tMax;
    for (int k = 0; k < 4; ++k) { o[9 + 3 * k] = diff[k].x; o[10 + 3 * k] = diff[k].y; o[11 + 3 * k] = diff[k].z; }
}

// The samples (px, py, sample number) of the camera-ray entry point `entry`: the pixel indexes per-pixel tables (Halton offsets, a
// pixel sampler's tables), so it lies inside the sample bounds, and a pixel sampler's sample number inside its tables.
static int CheckCameraSamples(const mi_pt *pt, const int32_t *samples, uint32_t n, const char *entry) {
    const DScene &s = pt->scene;
    for (uint32_t i = 0; i < n; ++i) {
        const int px = samples[3 * i], py = samples[3 * i + 1];
        if (px < s.sampleBounds[0] || px >= s.sampleBounds[2] || py < s.sampleBounds[1] || py >= s.sampleBounds[3] || samples[3 * i + 2] < 0 ||
            (s.samplerType >= MI_SAMPLER_ZEROTWO && samples[3 * i + 2] >= pt->spp)) {
            g_err = std::string(entry) + ": a sample lies outside the sample bounds (or beyond a pixel sampler's tables)";
            return MI_ERR_INVALID;
        }
    }
    return MI_OK;
}

extern "C" int mi_pt_camera_rays(mi_pt *pt, const int32_t *samples, uint32_t n, float *out) {
    if (!pt || !samples || !out) { g_err = "null argument"; return MI_ERR_INVALID; }
    if (n > (1u << 24)) { g_err = "mi_pt_camera_rays: more than 2^24 samples"; return MI_ERR_INVALID; }
    if (n == 0) return MI_OK;
    const DScene &s = pt->scene;
    if (s.cameraType != MI_CAMERA_PERSPECTIVE) {   // the lens camera's ray at 550 nm (band 0) or an opt-in camera's, in this call's layout
        std::vector<float> ex((size_t)n * MI_CAMERA_RAY_EX_FLOATS);
        const int rc = mi_pt_camera_rays_ex(pt, samples, n, 0, ex.data());
        if (rc != MI_OK) return rc;
        for (uint32_t i = 0; i < n; ++i) memcpy(out + 8 * (size_t)i, ex.data() + (size_t)i * MI_CAMERA_RAY_EX_FLOATS, 8 * sizeof(float));
        return MI_OK;
    }
    if (const int rc = CheckCameraSamples(pt, samples, n, "mi_pt_camera_rays")) return rc;
    return RunProbe(pt->device, samples, (size_t)n * 3 * sizeof(int32_t), out, (size_t)n * 8 * sizeof(float), [&](void *ds, void *dout) {
        hipLaunchKernelGGL((s.camera.animated ? k_camera_rays<true> : k_camera_rays<false>), ProbeGrid(n), dim3(BLOCK), 0, 0, s, (int32_t *)ds, n, (float *)dout);
    });
}

extern "C" int mi_pt_camera_rays_ex(mi_pt *pt, const int32_t *samples, uint32_t n, int32_t band, float *out) {
    if (!pt || !samples || !out) { g_err = "null argument"; return MI_ERR_INVALID; }
    if (n > (1u << 24)) { g_err = "mi_pt_camera_rays_ex: more than 2^24 samples"; return MI_ERR_INVALID; }
    const DScene &s = pt->scene;
    if (band < 0 || band >= std::max(1, s.nBands)) { g_err = "mi_pt_camera_rays_ex: no such band"; return MI_ERR_INVALID; }
    if (n == 0) return MI_OK;
    if (const int rc = CheckCameraSamples(pt, samples, n, "mi_pt_camera_rays_ex")) return rc;
    const bool moving = s.camera.animated != 0;
    auto kernel = moving ? k_camera_rays_ex<true, MI_CAMERA_PERSPECTIVE> : k_camera_rays_ex<false, MI_CAMERA_PERSPECTIVE>;
    if (s.cameraType == MI_CAMERA_REALISTIC) kernel = moving ? k_camera_rays_ex<true, MI_CAMERA_REALISTIC> : k_camera_rays_ex<false, MI_CAMERA_REALISTIC>;
    if (s.cameraType == MI_CAMERA_ORTHOGRAPHIC) kernel = moving ? k_camera_rays_ex<true, MI_CAMERA_ORTHOGRAPHIC> : k_camera_rays_ex<false, MI_CAMERA_ORTHOGRAPHIC>;
    if (s.cameraType == MI_CAMERA_ENVIRONMENT) kernel = moving ? k_camera_rays_ex<true, MI_CAMERA_ENVIRONMENT> : k_camera_rays_ex<false, MI_CAMERA_ENVIRONMENT>;
    return RunProbe(pt->device, samples, (size_t)n * 3 * sizeof(int32_t), out, (size_t)n * MI_CAMERA_RAY_EX_FLOATS * sizeof(float), [&](void *ds, void *dout) {
        hipLaunchKernelGGL(kernel, ProbeGrid(n), dim3(BLOCK), 0, 0, s, (int32_t *)ds, n, (int)band, (float *)dout);
    });
}

__global__ void k_texture_lookup(DScene s, int tex, const float *q, uint32_t n, float *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const mi_texture &t = s.textures[tex];
    const RGB3 v = MipLookup(s, s.mipmaps[t.mipmap], q[6 * i], q[6 * i + 1], q[6 * i + 2], q[6 * i + 3], q[6 * i + 4], q[6 * i + 5], t.filter, t.max_aniso);
    out[3 * i] = v.r; out[3 * i + 1] = v.g; out[3 * i + 2] = v.b;
}

extern "C" int mi_pt_texture_lookup(mi_pt *pt, int32_t tex, uint32_t n, const float *queries, float *rgb) {
    if (!pt || !queries || !rgb) { g_err = "null argument"; return MI_ERR_INVALID; }
    if (tex < 0 || (uint32_t)tex >= pt->nTextures) { g_err = "texture index out of range"; return MI_ERR_INVALID; }
    if (pt->textureTypes[tex] != MI_TEX_IMAGEMAP) { g_err = "mi_pt_texture_lookup: not an image texture"; return MI_ERR_INVALID; }
    if (n == 0) return MI_OK;
    return RunProbe(pt->device, queries, (size_t)n * 6 * sizeof(float), rgb, (size_t)n * 3 * sizeof(float), [&](void *dq, void *dout) {
        hipLaunchKernelGGL(k_texture_lookup, ProbeGrid(n), dim3(BLOCK), 0, 0, pt->scene, tex, (float *)dq, n, (float *)dout);
    });
}

// mi_pt_texture_probe: a noise texture's value for an interaction given by its world p, dpdx and dpdy, as k_shade asks for it
__global__ void k_texture_probe(DScene s, int tex, const float *q, uint32_t n, float *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *r = q + 9 * (size_t)i;
    TexDifferentials td;
    td.dudx = td.dvdx = td.dudy = td.dvdy = 0;
    td.dpdx = V3(r[3], r[4], r[5]); td.dpdy = V3(r[6], r[7], r[8]);
    out[i] = EvalFloatImageTexture<true>(s, tex, 0.f, 0.f, V3(r[0], r[1], r[2]), td);
}

extern "C" int mi_pt_texture_probe(mi_pt *pt, int32_t tex, uint32_t n, const float *queries, float *out) {
    if (!pt || !queries || !out) { g_err = "null argument"; return MI_ERR_INVALID; }
    if (tex < 0 || (uint32_t)tex >= pt->nTextures) { g_err = "texture index out of range"; return MI_ERR_INVALID; }
    if (!MI_TEX_IS_NOISE(pt->textureTypes[tex])) { g_err = "mi_pt_texture_probe: not a noise texture"; return MI_ERR_INVALID; }
    if (n > (1u << 24)) { g_err = "mi_pt_texture_probe: more than 2^24 queries"; return MI_ERR_INVALID; }
    if (n == 0) return MI_OK;
    return RunProbe(pt->device, queries, (size_t)n * 9 * sizeof(float), out, (size_t)n * sizeof(float), [&](void *dq, void *dout) {
        hipLaunchKernelGGL(k_texture_probe, ProbeGrid(n), dim3(BLOCK), 0, 0, pt->scene, (int)tex, (float *)dq, n, (float *)dout);
    });
}

// mi_pt_texture_eval_probe: any texture record at an interaction given in full, through the routines k_shade evaluates it with.
// mode 0: the record's 2-D mapping; mode 1: its value -- a spectrum texture's bins (TexBin over the compact form, as the lobes
// read it), a float texture's value times post_scale in bin 0
__global__ void k_texture_eval_probe(DScene s, int tex, int mode, const float *q, uint32_t n, float *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *r = q + MI_TEXTURE_EVAL_QUERY_FLOATS * (size_t)i;
    const V3 p(r[0], r[1], r[2]);
    TexDifferentials td;
    td.dpdx = V3(r[3], r[4], r[5]); td.dpdy = V3(r[6], r[7], r[8]);
    const float u = r[9], v = r[10];
    td.dudx = r[11]; td.dvdx = r[12]; td.dudy = r[13]; td.dvdy = r[14];
    const mi_texture &t = s.textures[tex];
    if (mode == 0) {
        const TexCoord2D c = MapTexture2D<true>(t, u, v, p, td);
        float *o = out + 6 * (size_t)i;
        o[0] = c.s; o[1] = c.t; o[2] = c.dsdx; o[3] = c.dtdx; o[4] = c.dsdy; o[5] = c.dtdy;
        return;
    }
    float *o = out + MI_NSPEC * (size_t)i;
    if (t.is_float) {
        o[0] = EvalFloatImageTexture<true>(s, tex, u, v, p, td);
        for (int b = 1; b < MI_NSPEC; ++b) o[b] = 0.f;
        return;
    }
    const IllumRGB value = EvalImageTexture<true>(s, tex, u, v, p, td);
    for (int b = 0; b < MI_NSPEC; ++b) o[b] = TexBin(s.rgbIllum, s.textures, value, b);
}

extern "C" int mi_pt_texture_eval_probe(mi_pt *pt, int32_t tex, int32_t mode, uint32_t n, const float *queries, float *out) {
    if (!pt || !queries || !out) { g_err = "null argument"; return MI_ERR_INVALID; }
    if (tex < 0 || (uint32_t)tex >= pt->nTextures) { g_err = "texture index out of range"; return MI_ERR_INVALID; }
    if (mode < 0 || mode > 1) { g_err = "mi_pt_texture_eval_probe: mode must be 0 or 1"; return MI_ERR_INVALID; }
    if (mode == 0 && !MI_TEX_HAS_MAPPING2D(pt->textureTypes[tex])) { g_err = "mi_pt_texture_eval_probe: the record has no 2-D mapping"; return MI_ERR_INVALID; }
    if (n > (1u << 24)) { g_err = "mi_pt_texture_eval_probe: more than 2^24 queries"; return MI_ERR_INVALID; }
    if (n == 0) return MI_OK;
    const size_t nOut = mode == 0 ? 6 : MI_NSPEC;
    return RunProbe(pt->device, queries, (size_t)n * MI_TEXTURE_EVAL_QUERY_FLOATS * sizeof(float), out, (size_t)n * nOut * sizeof(float), [&](void *dq, void *dout) {
        hipLaunchKernelGGL(k_texture_eval_probe, ProbeGrid(n), dim3(BLOCK), 0, 0, pt->scene, (int)tex, (int)mode, (float *)dq, n, (float *)dout);
    });
}

// ------------------------------------------------------------------ one quadric on its own (mi_pt_shape_probe)
__global__ void k_shape_probe(DScene s, int q, int mode, const float *in, uint32_t n, float *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool disk = IsDisk(s, q);
    if (mode == 0) {
        const float *r = in + 7 * (size_t)i;
        float *o = out + MI_SHAPE_PROBE_HIT_FLOATS * (size_t)i;
        for (int k = 0; k < MI_SHAPE_PROBE_HIT_FLOATS; ++k) o[k] = 0.f;
        const V3 ro(r[0], r[1], r[2]), rd(r[3], r[4], r[5]);
        float tT = 0.f, t = 0.f;
        const bool hitT = QuadricHitT(s, q, ro, rd, r[6], &tT);   // (the any-hit form and the full one must agree)
        SurfaceInteraction si;
        if (!QuadricInteraction(s, q, ro, rd, r[6], &si, &t)) { o[0] = hitT ? -1.f : 0.f; return; }
        float u = 0.f, v = 0.f;
        TriShading ts;
        if (disk) DiskTexCoords(s.disks[q - s.nSpheres], ro, rd, &u, &v, &ts);
        else SphereTexCoords(s.spheres[q], ro, rd, &u, &v, &ts);
        o[0] = (hitT && tT == t) ? 1.f : -1.f;
        o[1] = t;
        o[2] = si.p.x; o[3] = si.p.y; o[4] = si.p.z;
        o[5] = si.n.x; o[6] = si.n.y; o[7] = si.n.z;
        o[8] = u; o[9] = v;
        o[10] = si.dpdu.x; o[11] = si.dpdu.y; o[12] = si.dpdu.z;
        o[13] = ts.dpdv.x; o[14] = ts.dpdv.y; o[15] = ts.dpdv.z;
        return;
    }
    // the reference point as Shape::SolidAngle makes it (shape.cpp:90-91): no normal, no error bound
    const float *r = in + (mode == 1 ? 5 : 6) * (size_t)i;
    Interaction ref;
    ref.p = V3(r[0], r[1], r[2]);
    ref.pError = V3(0, 0, 0); ref.n = V3(0, 0, 0); ref.wo = V3(0, 0, 1);
    if (mode == 1) {
        float *o = out + MI_SHAPE_PROBE_SAMPLE_FLOATS * (size_t)i;
        float pdf = 0.f;
        const Interaction it = ShapeSample(s, ~q, ref, r[3], r[4], &pdf);
        o[0] = it.p.x; o[1] = it.p.y; o[2] = it.p.z; o[3] = it.n.x; o[4] = it.n.y; o[5] = it.n.z; o[6] = pdf;
    } else {
        const float area = disk ? DiskArea(s.disks[q - s.nSpheres]) : SphereArea(s.spheres[q]);
        out[i] = ShapePdf(s, ~q, area, ref, V3(r[3], r[4], r[5]));
    }
}

extern "C" int mi_pt_shape_probe(mi_pt *pt, int32_t quadric, int32_t mode, uint32_t n, const float *queries, float *out) {
    if (!pt || !queries || !out) { g_err = "null argument"; return MI_ERR_INVALID; }
    if (quadric < 0 || (uint32_t)quadric >= pt->nQuadrics) { g_err = "mi_pt_shape_probe: quadric index out of range"; return MI_ERR_INVALID; }
    if (mode < 0 || mode > 2) { g_err = "mi_pt_shape_probe: mode must be 0, 1 or 2"; return MI_ERR_INVALID; }
    if (n > (1u << 24)) { g_err = "mi_pt_shape_probe: more than 2^24 queries"; return MI_ERR_INVALID; }
    if (n == 0) return MI_OK;
    const size_t nIn = mode == 0 ? 7 : (mode == 1 ? 5 : 6);
    const size_t nOut = mode == 0 ? MI_SHAPE_PROBE_HIT_FLOATS : (mode == 1 ? MI_SHAPE_PROBE_SAMPLE_FLOATS : 1);
    return RunProbe(pt->device, queries, (size_t)n * nIn * sizeof(float), out, (size_t)n * nOut * sizeof(float), [&](void *dq, void *dout) {
        hipLaunchKernelGGL(k_shape_probe, ProbeGrid(n), dim3(BLOCK), 0, 0, pt->scene, (int)quadric, (int)mode, (float *)dq, n, (float *)dout);
    });
}

// ------------------------------------------------------------------ one light on its own (mi_pt_light_probe)
// SampleLi / LiBin / ShapeSample with the full mask, as the general k_shade instance holds them; InfinitePdfLi, ShapePdf and
// InfiniteLe as its MIS branch calls them. The reference point: no error bound, wo = +z, the query's normal.
__global__ void k_light_probe(DScene s, int light, int mode, const float *in, uint32_t n, float *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const mi_light &l = s.lights[light];
    if (mode == 2) {
        float *o = out + MI_NSPEC * (size_t)i;
        if (l.type == MI_LIGHT_INFINITE) {
            const float *r = in + 3 * (size_t)i;
            const IllumRGB le = InfiniteLe(s, l, V3(r[0], r[1], r[2]));
            for (int b = 0; b < MI_NSPEC; ++b) o[b] = IllumBin(s, le, b);
        } else {   // DiffuseAreaLight::L(n, w), diffuse.h:56-58: the test k_shade makes where a path meets an emitter
            const float *r = in + 6 * (size_t)i;
            const bool emits = l.two_sided || Dot(V3(r[0], r[1], r[2]), V3(r[3], r[4], r[5])) > 0;
            for (int b = 0; b < MI_NSPEC; ++b) o[b] = emits ? l.L[b] : 0.f;
        }
        return;
    }
    const float *r = in + (mode == 0 ? 8 : 9) * (size_t)i;
    Interaction ref;
    ref.p = V3(r[0], r[1], r[2]);
    ref.pError = V3(0, 0, 0); ref.n = V3(r[3], r[4], r[5]); ref.wo = V3(0, 0, 1);
    if (mode == 0) {
        float *o = out + MI_LIGHT_PROBE_SAMPLE_FLOATS * (size_t)i;
        for (int k = 0; k < MI_LIGHT_PROBE_SAMPLE_FLOATS; ++k) o[k] = 0.f;
        const LightSample ls = SampleLi<TM_ALL>(s, l, ref, r[6], r[7]);
        if (ls.black && ls.pdf == 0) return;   // Sample_Li returned before it had a direction
        o[0] = ls.wi.x; o[1] = ls.wi.y; o[2] = ls.wi.z; o[3] = ls.pdf;
        o[4] = ls.pLight.p.x; o[5] = ls.pLight.p.y; o[6] = ls.pLight.p.z;
        if (l.type == MI_LIGHT_DIFFUSE_AREA) { o[7] = ls.pLight.n.x; o[8] = ls.pLight.n.y; o[9] = ls.pLight.n.z; }
        if (!ls.black) for (int b = 0; b < MI_NSPEC; ++b) o[10 + b] = LiBin<TM_ALL>(s, l, ls, b);
    } else {
        const V3 wi(r[6], r[7], r[8]);
        out[i] = IsDeltaLight(l) ? 0.f : (l.type == MI_LIGHT_INFINITE ? InfinitePdfLi(s, l, wi) : ShapePdf<true>(s, l.shape, l.area, ref, wi));
    }
}

extern "C" int mi_pt_light_probe(mi_pt *pt, int32_t light, int32_t mode, uint32_t n, const float *queries, float *out) {
    if (!pt || !queries || !out) { g_err = "null argument"; return MI_ERR_INVALID; }
    if (light < 0 || (size_t)light >= pt->lightTypes.size()) { g_err = "mi_pt_light_probe: light index out of range"; return MI_ERR_INVALID; }
    if (mode < 0 || mode > 2) { g_err = "mi_pt_light_probe: mode must be 0, 1 or 2"; return MI_ERR_INVALID; }
    const int type = pt->lightTypes[light];
    const bool delta = type == MI_LIGHT_POINT || type == MI_LIGHT_DISTANT || type == MI_LIGHT_SPOT || type == MI_LIGHT_PROJECTION;
    if (mode == 2 && delta) { g_err = "mi_pt_light_probe: mode 2 (Le / L) on a delta light"; return MI_ERR_INVALID; }
    if (n > (1u << 24)) { g_err = "mi_pt_light_probe: more than 2^24 queries"; return MI_ERR_INVALID; }
    if (n == 0) return MI_OK;
    const size_t nIn = mode == 0 ? 8 : (mode == 1 ? 9 : (type == MI_LIGHT_INFINITE ? 3 : 6));
    const size_t nOut = mode == 0 ? MI_LIGHT_PROBE_SAMPLE_FLOATS : (mode == 1 ? 1 : MI_NSPEC);
    return RunProbe(pt->device, queries, (size_t)n * nIn * sizeof(float), out, (size_t)n * nOut * sizeof(float), [&](void *dq, void *dout) {
        hipLaunchKernelGGL(k_light_probe, ProbeGrid(n), dim3(BLOCK), 0, 0, pt->scene, (int)light, (int)mode, (float *)dq, n, (float *)dout);
    });
}

// ------------------------------------------------------------------ the Halton routines on their own (mi_pt_sampler_probe)
// Query i = (index, first dimension) as two 64-bit words; `group` values per query: the grouped routines k_shade calls (5, 2, 1;
// 32-bit indices) or ScrambledDimension (0: one value, any index). Neighbouring lanes get what the caller gives them: different
// dimensions and digit counts in one wave run the interleaved loops with some chains finished and others not.
__global__ void k_sampler_probe(DScene s, int group, const uint64_t *in, uint32_t n, float *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t index = in[2 * (size_t)i];
    const int dim = (int)in[2 * (size_t)i + 1];
    if (group == 5) {
        const Halton5 r = ScrambledDimensions5(HaltonTable(s.haltonDims), (uint32_t)index, dim);
        float *o = out + 5 * (size_t)i;
        o[0] = r.u0; o[1] = r.u1; o[2] = r.u2; o[3] = r.u3; o[4] = r.u4;
    } else if (group == 2) {
        const Halton2 r = ScrambledDimensions2(HaltonTable(s.haltonDims), (uint32_t)index, dim);
        out[2 * (size_t)i] = r.u0; out[2 * (size_t)i + 1] = r.u1;
    } else if (group == 1) out[i] = ScrambledDimensions1(HaltonTable(s.haltonDims), (uint32_t)index, dim);
    else out[i] = ScrambledDimension(s.primes, s.primeSums, s.perms, s.primeMagic, index, dim);
}

extern "C" int mi_pt_sampler_probe(mi_pt *pt, int32_t group, uint32_t n, const uint64_t *indices, const int32_t *first_dims, float *out) {
    if (!pt || !indices || !first_dims || !out) { g_err = "null argument"; return MI_ERR_INVALID; }
    if (group != 0 && group != 1 && group != 2 && group != 5) { g_err = "mi_pt_sampler_probe: group must be 0, 1, 2 or 5"; return MI_ERR_INVALID; }
    if (n > (1u << 24)) { g_err = "mi_pt_sampler_probe: more than 2^24 queries"; return MI_ERR_INVALID; }
    const int count = group == 0 ? 1 : group;
    std::vector<uint64_t> q(2 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
        if (first_dims[i] < 2 || first_dims[i] + count > pt->samplerDims) { g_err = "mi_pt_sampler_probe: dimensions outside [2, n_dims)"; return MI_ERR_INVALID; }
        if (group != 0 && (indices[i] >> 32)) { g_err = "mi_pt_sampler_probe: the grouped routines take 32-bit indices"; return MI_ERR_INVALID; }
        q[2 * (size_t)i] = indices[i];
        q[2 * (size_t)i + 1] = (uint64_t)first_dims[i];
    }
    if (n == 0) return MI_OK;
    return RunProbe(pt->device, q.data(), q.size() * sizeof(uint64_t), out, (size_t)n * count * sizeof(float), [&](void *dq, void *dout) {
        hipLaunchKernelGGL(k_sampler_probe, ProbeGrid(n), dim3(BLOCK), 0, 0, pt->scene, (int)group, (const uint64_t *)dq, n, (float *)dout);
    });
}

// ------------------------------------------------------------------ scalar helpers on their own (mi_pt_math_probe)
__global__ void k_math_probe(int op, uint32_t n, const float *x, const float *y, float *out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x0 = x[2 * i], x1 = x[2 * i + 1], y0 = y[2 * i], y1 = y[2 * i + 1];
    float *o = out + 3 * (size_t)i;
    o[0] = o[1] = o[2] = 0.f;
    if (op == 0) { o[0] = NextFloatUp(x0); o[1] = NextFloatDown(x0); }
    else if (op >= 1 && op <= 4) {
        const EFloat a(x0, x1), b(y0, y1);
        const EFloat r = op == 1 ? a + b : (op == 2 ? a - b : (op == 3 ? a * b : a / b));
        o[0] = r.v; o[1] = r.low; o[2] = r.high;
    } else if (op == 5) {
        const float cdf[10] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9}, func[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
        float pdf;
        o[0] = (float)SampleDiscrete(func, cdf, 1.f, 9, x0, &pdf);
    } else if (op == 6) {   // x0 / y0 by DivBy and by DivFast with a tracker of its own
        const Divisor dv = MakeDivisor(y0);
        DivTrack trk;
        trk.Reset(dv.fast);
        o[0] = DivBy(x0, dv);
        o[1] = DivFast(x0, y0, 1.f / y0, trk);
        o[2] = trk.Bad() ? 1.f : 0.f;
    }
}

extern "C" int mi_pt_math_probe(int device_ordinal, int op, uint32_t n, const float *x, const float *y, float *out) {
    if (!x || !y || !out || op < 0 || op > 6) { g_err = "mi_pt_math_probe: bad argument"; return MI_ERR_INVALID; }
    if (n == 0) return MI_OK;
    int nDev = 0;
    if (hipGetDeviceCount(&nDev) != hipSuccess || device_ordinal < 0 || device_ordinal >= nDev) { g_err = "no HIP device available (this path has no CPU fallback)"; return MI_ERR_NO_DEVICE; }
    HIPCHK(hipSetDevice(device_ordinal));
    DevBuf dx, dy, dout;   // (two inputs: not RunProbe's shape)
    HIPCHK(dx.alloc((size_t)n * 2 * sizeof(float)));
    HIPCHK(dy.alloc((size_t)n * 2 * sizeof(float)));
    HIPCHK(dout.alloc((size_t)n * 3 * sizeof(float)));
    HIPCHK(hipMemcpy(dx.p, x, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dy.p, y, (size_t)n * 2 * sizeof(float), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_math_probe, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, 0, op, n, dx.as<float>(), dy.as<float>(), dout.as<float>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, dout.p, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return MI_OK;
}

// ------------------------------------------------------------------ standalone traversal (mi_pt_trace)
// stride: floats per ray -- 7, or 8 with the ray's time behind tMax (mi_pt_trace_timed)
__global__ void __launch_bounds__(BLOCK) k_trace(DScene s, const float *rays, uint32_t n, int anyHit, float *hits, int stride) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float *r = rays + (size_t)i * stride;
    V3 ro(r[0], r[1], r[2]), rd(r[3], r[4], r[5]);
    unsigned nodes = 0, tris = 0;
    Hit h;
    h.prim = -1; h.t = 0; h.b0 = h.b1 = h.b2 = 0;
    int prim;
    const float time = stride == 8 ? r[7] : s.camera.shutter_open;   // (a ray without a time of its own: the shutter-open time)
    if (s.motions) {   // (uniform)
        if (anyHit) prim = Traverse<true, true, true>(s, ro, rd, r[6], &h, nodes, tris, time) ? 0 : -1;
        else prim = Traverse<false, true, true>(s, ro, rd, r[6], &h, nodes, tris, time) ? h.prim : -1;
    } else if (anyHit) prim = Traverse<true, true>(s, ro, rd, r[6], &h, nodes, tris, time) ? 0 : -1;
    else prim = Traverse<false, true>(s, ro, rd, r[6], &h, nodes, tris, time) ? h.prim : -1;
    float *o = hits + (size_t)i * 4;
    o[0] = __int_as_float(prim);
    o[1] = (prim >= 0 && !anyHit) ? h.t : 0.f;
    o[2] = (prim >= 0 && !anyHit) ? h.b0 : 0.f;
    o[3] = (prim >= 0 && !anyHit) ? h.b1 : 0.f;
}

// ------------------------------------------------------------------ recorded rays through the render's own kernels (mi_pt_trace_wavefront)
// Loads ray i into slot i of the pool exactly as k_generate / k_shade leave a path ray (mode 0), an NEE shadow ray (1) or a
// BSDF-sampled MIS ray (2), and lists it in that mode's work list. The shadow mode's flags make k_resolve_shadow's commit
// readable without a spectrum: the candidate line "holds L + the light sample" (F_CAND), so an unoccluded ray flips F_L_IN_B and clears F_L_ZERO.
// timePlane >= 0: the scene has moving instances; a ray of 8 floats brings its time, the others take the given one (the
// shutter-open time).
__global__ void __launch_bounds__(BLOCK) k_trace_load(Pool pool, DevCounters *ctr, const float *rays, uint32_t n, int mode, int timePlane, float time, int stride) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i == 0) {
        if (mode == 0) { ctr->primCount.v = n; ctr->contCount.v = 0; }
        else if (mode == 1) ctr->shadowCount.v = n;
        else ctr->misCount.v = n;
    }
    if (i >= pool.n) return;
    int flags = 0;
    if (i < n) {
        const float *r = rays + (size_t)i * stride;
        if (mode == 0) {
            pool.R(R_RAY0, i) = make_float4(r[0], r[1], r[2], r[6]);
            pool.R(R_RAY1, i) = make_float4(r[3], r[4], r[5], 1.f);
            pool.extQ[i] = i;
            flags = F_ALIVE;
        } else {
            pool.R(mode == 1 ? R_SH0 : R_MI0, i) = make_float4(r[0], r[1], r[2], r[3]);
            // (mode 3, the visibility form of a MIS ray: the span ends at the given tMax and starts at tMax (1 - 2^-8); no primitive left out)
            pool.R(mode == 1 ? R_SH1 : R_MI1, i) = make_float4(r[4], r[5], mode == 3 ? r[6] : 0.f, mode == 3 ? __uint_as_float(MIS_EXCL_NONE | (8u << MIS_EXCL_BITS)) : 0.f);
            (mode == 1 ? pool.shadowQ : pool.misQ)[i] = i;
            flags = mode == 1 ? (F_ALIVE | F_NEE | F_SHADOW | F_L_ZERO | F_CAND | F_NEE_NZ) : (F_ALIVE | F_NEE | F_MIS);
        }
        if (timePlane >= 0) pool.F(timePlane, i) = stride == 8 ? r[7] : time;
        pool.I(I_HITPRIM, i) = -2;   // (every ray must be answered: k_trav overwrites this)
        if (mode == 1) pool.shadowQ[pool.n + i] = 0xfffffffeu;   // (... a shadow or MIS ray's answer lies beside its queue entry)
        if (mode >= 2) { pool.misQ[pool.n + 2 * (size_t)i] = mode == 3 ? 0xfffffffdu : 0xfffffffeu; pool.misQ[pool.n + 2 * (size_t)i + 1] = 0u; }
        pool.I(I_NPEND, i) = 0;
        pool.I(I_HITINST, i) = -1;
        pool.I(I_MISLIGHT, i) = 0;
    }
    pool.I(I_FLAGS, i) = flags;
}
// what k_trav left in the planes, before the resolve step
__global__ void __launch_bounds__(BLOCK) k_trace_raw(Pool pool, uint32_t n, int mode, float *extra) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    if (mode == 1) {   // the answer word: -2 = never answered; else bit 31 occluded | postponed quadrics
        const unsigned v = pool.shadowQ[pool.n + i];
        extra[4 * (size_t)i + 2] = __int_as_float(v == 0xfffffffeu ? 0 : (int)(v & 0x7fffffffu));
        extra[4 * (size_t)i + 3] = __int_as_float(v == 0xfffffffeu ? -2 : ((v >> 31) ? 0 : -1));
        return;
    }
    if (mode >= 2) {
        extra[4 * (size_t)i + 2] = __int_as_float((int)pool.misQ[pool.n + 2 * (size_t)i + 1]);
        extra[4 * (size_t)i + 3] = __int_as_float((int)pool.misQ[pool.n + 2 * (size_t)i]);
        return;
    }
    extra[4 * (size_t)i + 2] = __int_as_float(pool.I(I_NPEND, i));
    extra[4 * (size_t)i + 3] = __int_as_float(pool.I(I_HITPRIM, i));
}
// The committed answer. Mode 0: the planes as k_resolve_extend / k_resolve_overflow left them. Mode 1: k_resolve_shadow's
// verdict (see k_trace_load). Mode 2: k_resolve_mis consumes its hit in place (ResolveMisSlot), so its quadric step
// (MisClosestHit) is run here.
template <bool INST, bool MOTION = false>
__global__ void __launch_bounds__(BLOCK) k_trace_read(DScene s, Pool pool, uint32_t n, int mode, float *hits, float *extra) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    int prim = mode >= 2 ? (int)pool.misQ[pool.n + 2 * (size_t)i] : pool.I(I_HITPRIM, i), inst = -1;
    float4 hr = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mode == 0) { hr = pool.R(R_HIT, i); if (INST) inst = pool.I(I_HITINST, i); }
    else if (mode == 1) prim = (pool.I(I_FLAGS, i) & F_L_ZERO) ? 0 : -1;
    else if (mode == 3) {}   // (k_trav<3>'s verdict as it stands: an occluder, -1, -2 = ambiguous; -3 = never answered)
    else {
        V3 ro, rd;
        Hit h;
        h.prim = prim; h.t = 0.f; h.b0 = h.b1 = h.b2 = 0.f;
        bool haveRay = false;
        LoadMisRay(pool, i, ro, rd, h, haveRay);   // (at once: the hit is recorded here whether it has quadrics or not)
        const int npend = (int)pool.misQ[pool.n + 2 * (size_t)i + 1];
        const bool found = (npend & PEND_OVERFLOW) ? MisClosestHit<INST, true, MOTION>(s, pool, i, npend, ro, rd, h, haveRay)
                                                   : MisClosestHit<INST, false>(s, pool, i, npend, ro, rd, h, haveRay);
        prim = found ? h.prim : -1;
        hr = HitRecord(h);
        inst = h.inst;
    }
    const bool rec = prim >= 0 && mode != 1 && mode != 3;
    float *o = hits + (size_t)i * 4;
    o[0] = __int_as_float(prim);
    o[1] = rec ? hr.x : 0.f; o[2] = rec ? hr.y : 0.f; o[3] = rec ? hr.z : 0.f;
    if (extra) { extra[4 * (size_t)i] = rec ? hr.w : 0.f; extra[4 * (size_t)i + 1] = __int_as_float(rec ? inst : -1); }
}

__global__ void k_film_split(const float *film32, float *filmSum, float *weightSum, size_t nPix) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nPix * 32) return;
    size_t pix = i >> 5;
    int b = (int)(i & 31);
    float v = film32[i];
    if (b < 31) { if (filmSum) filmSum[pix * 31 + b] = v; }
    else if (weightSum) weightSum[pix] = v;
}

// ------------------------------------------------------------------ metadata
// Integrator "metadata" (MetadataIntegrator::Li, src/integrators/metadata.cpp:52-89): a pass is k_generate -> k_trav<0> ->
// k_resolve_extend (+ k_resolve_overflow) -> this kernel, and the camera ray's closest hit is the whole answer. Every slot
// that is still alive after the resolve step -- a hit, or a miss that an environment light kept in the miss class -- ends
// here: a hit gets its value by `strategy` (mi_metadata_strategy) in the line that holds the path's L, a miss keeps L = 0
// (F_L_ZERO), and the state word is FinishedWord's, so the next k_generate flushes the slot through the guards of
// SamplerIntegrator::Render and the filter like any radiance (integrator.cpp:277-323; the ray weight of the perspective
// camera is 1). isect.p is rebuilt by the routine k_shade uses -- BuildHitVertex: HitInteraction with the ray of the space the hit
// lies in, InteractionToWorld for a hit inside an instance -- so it is the point shading sees, bit for bit. `primMeta`: the ids of
// every primitive, parallel to DScene::prims (mi_prim_meta); the instance id of a hit reached through a
// TransformedPrimitive is that instance's number + 1 (primitive.cpp:89).
//
// Stores: the pool is walked densely and a slot's spectrum is one 128-B line. A lane that stores its own eight quads issues
// eight instructions of 64 scattered 16-B pieces (measured: 1.77 ms per launch on 31 M slots); here the lanes park their
// values in LDS (four words say what all 32 are) and the wave stores eight lanes per line, every instruction covering whole
// lines (SpectrumTile's pattern in k_shade): 1.09 ms. DESIGN.md 5b has the measurement.
// Quad c of the spectrum {a, b, c, rest, rest, ..., rest} (bin 31 is padding and stays 0), given as v = (a, b, c, rest).
DEV float4 MetadataQuad(const float4 &v, int c) {
    if (c == 0) return v;
    return make_float4(v.w, v.w, v.w, c == NQ - 1 ? 0.f : v.w);
}
template <bool INST, bool MOTION = false>
__global__ void __launch_bounds__(BLOCK) k_commit_metadata(DScene s, Pool pool, const mi_prim_meta *__restrict__ primMeta, int strategy) {
    const uint32_t slot = blockIdx.x * BLOCK + threadIdx.x;
    const int word = slot < pool.n ? pool.I(I_FLAGS, slot) : 0;
    bool wrote = false;
    float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((word & F_ALIVE) && !(word & F_FINISHED)) {
        const int prim = pool.I(I_HITPRIM, slot);
        if (prim >= 0 && (uint32_t)prim < s.nPrims) {
            if (strategy == MI_METADATA_MATERIAL || strategy == MI_METADATA_MESH) {
                unsigned id = strategy == MI_METADATA_MATERIAL ? primMeta[prim].material_id : primMeta[prim].instance_id;
                if (INST && strategy == MI_METADATA_MESH) {
                    const int inst = pool.I(I_HITINST, slot);
                    if (inst >= 0) id = InstanceIdOf(s.instances[inst], inst);
                }
                const float v = (float)id;   // L = Spectrum(isect.materialId) / Spectrum(isect.instanceId), metadata.cpp:71-75
                val = make_float4(v, v, v, v);
            } else {
                MovingMatrices<MOTION> mm;
                HitVertex<INST, MOTION> hv;
                SurfaceInteraction isect;
                BuildHitVertex<true>(s, pool, slot, prim, pool.R(R_RAY0, slot), pool.R(R_RAY1, slot), true, mm, hv, &isect, nullptr);
                if (strategy == MI_METADATA_DEPTH) {
                    const V3 toIntersect = isect.p - hv.ro;   // metadata.cpp:68-69
                    const float v = toIntersect.Length();
                    val = make_float4(v, v, v, v);
                } else
                    val = make_float4(isect.p.x, isect.p.y, isect.p.z, 0.f);   // L[0..2] = isect.p, metadata.cpp:79-81
            }
            wrote = true;
        }
        pool.I(I_FLAGS, slot) = FinishedWord(wrote ? word & ~F_L_ZERO : word);
    }
    const int lPlane = LPlane(word);
    __shared__ float4 sVal[BLOCK];
    __shared__ uint32_t sLine[BLOCK];   // the line of the slot's L: its first quad is pool.q[line * NQ]
    const int lane = threadIdx.x & 63, wbase = threadIdx.x & ~63;
    const unsigned long long wmask = __ballot(wrote);
    const int nW = __popcll(wmask);
    if (wrote) {
        const int rw = __popcll(wmask & ((1ull << lane) - 1ull));
        sVal[wbase + rw] = val;
        sLine[wbase + rw] = (uint32_t)(pool.QuadIndex(lPlane, slot) >> 3);
    }
    // (the exchange stays inside the wave, whose LDS accesses complete in order: the fence only keeps the compiler from moving them)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int c = lane & 7;
    for (int e = lane >> 3; e < nW; e += 8)   // eight lanes per path: one store instruction covers eight whole lines
        pool.q[((size_t)sLine[wbase + e] << 3) + c] = MetadataQuad(sVal[wbase + e], c);
}

#endif   // MIPT_HAS_MAIN

// Every k_shade instance, in launch order (LaunchShade): X(part, NL, TM). The part is the MIPT_PART that compiles the
// instance; without MIPT_PART the kernel table instantiates them all. The parts also carry the device compile flags (Makefile,
// HIPFLAGS_part<N>): 1 (the matte and plastic instances) and 2 (the other instances without image textures) are built without
// SLP packing, 3 and 5 (every instance that reads image textures, TM_TEXTURED) at plain -O3 -- DESIGN section 4, round 8.
// A new instance needs a row in tests/test_shade_instances_gpu.py (the suite fails without a GPU until it has one).
#define MIPT_SHADE_INSTANCES(X) \
    X(1, 2, TM_DIFFUSE | TM_LIGHTS_ALL) X(1, 2, TM_DIFFUSE | TM_LIGHTS_NO_ENV) \
    X(1, 2, TM_DIFFUSE | TM_LIGHTS_ALL | TM_SAMPLERS) X(1, 2, TM_DIFFUSE | TM_LIGHTS_NO_ENV | TM_SAMPLERS) \
    X(1, 2, TM_PLASTIC | TM_LIGHTS_ALL) X(1, 2, TM_PLASTIC | TM_LIGHTS_NO_ENV) \
    X(1, 2, TM_PLASTIC | TM_LIGHTS_ALL | TM_SAMPLERS) X(1, 2, TM_PLASTIC | TM_LIGHTS_NO_ENV | TM_SAMPLERS) \
    X(2, 2, TM_GENERIC) \
    X(2, 2, TM_GLASS | TM_LIGHTS_ALL | TM_SAMPLERS) \
    X(2, 4, TM_UBER | TM_LIGHTS_ALL | TM_SAMPLERS) \
    X(2, MI_MAX_BXDFS, TM_DISNEY | TM_LIGHTS_ALL | TM_SAMPLERS) \
    X(2, 4, TM_GENERIC) \
    X(3, 4, TM_FULL) \
    X(2, MI_MAX_BXDFS, TM_GENERIC) \
    X(3, 2, TM_DIFFUSE | TM_TEXTURED | TM_LIGHTS_ALL | TM_SAMPLERS) \
    X(3, 2, TM_PLASTIC | TM_TEXTURED | TM_LIGHTS_ALL | TM_SAMPLERS) \
    X(3, 2, TM_FULL) \
    X(3, MI_MAX_BXDFS, TM_FULL) \
    X(5, 2, TM_ALL) \
    X(5, MI_MAX_BXDFS, TM_ALL)
// The LENS = true twins of the instances above that read image textures (TM_TEXTURED): not part of the plan's table, a launch
// takes the twin where the scene has a realistic camera in front of textures (LaunchShade).
#define MIPT_SHADE_LENS_INSTANCES(X) \
    X(3, 4, TM_FULL) \
    X(3, 2, TM_DIFFUSE | TM_TEXTURED | TM_LIGHTS_ALL | TM_SAMPLERS) \
    X(3, 2, TM_PLASTIC | TM_TEXTURED | TM_LIGHTS_ALL | TM_SAMPLERS) \
    X(3, 2, TM_FULL) \
    X(3, MI_MAX_BXDFS, TM_FULL) \
    X(5, 2, TM_ALL) \
    X(5, MI_MAX_BXDFS, TM_ALL)
// The MOTION = true twins of the instances that hold the instance code (TM_INSTANCES), each with its LENS twin: a launch takes
// them where the scene has moving instances (LaunchShade). Not part of the plan's table either.
#define MIPT_SHADE_MOTION_INSTANCES(X) \
    X(5, 2, TM_ALL) \
    X(5, MI_MAX_BXDFS, TM_ALL)
#ifdef MIPT_PART   // each part defines its own instances and declares the others
#if MIPT_PART == 1
#define MIPT_SHADE_IN_1
#else
#define MIPT_SHADE_IN_1 extern
#endif
#if MIPT_PART == 2
#define MIPT_SHADE_IN_2
#else
#define MIPT_SHADE_IN_2 extern
#endif
#if MIPT_PART == 3
#define MIPT_SHADE_IN_3
#else
#define MIPT_SHADE_IN_3 extern
#endif
#if MIPT_PART == 5
#define MIPT_SHADE_IN_5
#else
#define MIPT_SHADE_IN_5 extern
#endif
#define MIPT_SHADE_INSTANCE(P_, NL_, TM_) MIPT_SHADE_IN_##P_ template __global__ void k_shade<NL_, (TM_)>(DScene, Pool, DevCounters *, unsigned);
MIPT_SHADE_INSTANCES(MIPT_SHADE_INSTANCE)
#define MIPT_SHADE_LENS_INSTANCE(P_, NL_, TM_) MIPT_SHADE_IN_##P_ template __global__ void k_shade<NL_, (TM_), true>(DScene, Pool, DevCounters *, unsigned);
MIPT_SHADE_LENS_INSTANCES(MIPT_SHADE_LENS_INSTANCE)
#define MIPT_SHADE_MOTION_INSTANCE(P_, NL_, TM_) MIPT_SHADE_IN_##P_ template __global__ void k_shade<NL_, (TM_), false, true>(DScene, Pool, DevCounters *, unsigned); \
                                                 MIPT_SHADE_IN_##P_ template __global__ void k_shade<NL_, (TM_), true, true>(DScene, Pool, DevCounters *, unsigned);
MIPT_SHADE_MOTION_INSTANCES(MIPT_SHADE_MOTION_INSTANCE)
#endif

// ------------------------------------------------------------------ the BSDF on its own (mi_pt_bsdf_probe)
// d_bsdf.h reads these bits of an instance's mask: the lobe types, the Fresnel kinds, TM_TEXTURED and TM_SCALED. The light,
// sampler and instance bits never reach it, so the probe is compiled once per (NL, TM & TM_BSDF_BITS): the rows below, which
// BsdfProbeRow() looks an instance of MIPT_SHADE_INSTANCES up in (tests/test_shade_plan.py: every instance has a row).
constexpr unsigned TM_BSDF_BITS = 0x7fffu | (0xffu << 16) | TM_TEXTURED | TM_SCALED;
#define MIPT_BSDF_PROBE_ROWS(X) \
    X(2, TM_DIFFUSE) X(2, TM_PLASTIC) X(2, TM_GLASS) X(2, TM_GENERIC) X(2, TM_FULL) \
    X(2, TM_DIFFUSE | TM_TEXTURED) X(2, TM_PLASTIC | TM_TEXTURED) \
    X(4, TM_UBER) X(4, TM_GENERIC) X(4, TM_FULL) \
    X(MI_MAX_BXDFS, TM_DISNEY) X(MI_MAX_BXDFS, TM_GENERIC) X(MI_MAX_BXDFS, TM_FULL)

#if !defined(MIPT_PART) || MIPT_PART == 4
// One query per lane, in the frame oracle_bsdf builds (ns = ng = +z, ss = +x, ts = +y), every lobe of the material on, no
// override: the frame k_shade has at an untextured material. The 31 bins come out of the routines k_shade<NL, TM> calls:
//   form 0  BSDF_f / BSDF_Sample_f<FILL> and EvalBin (the definition)
//   form 1  the same lobe list through EvalQuad
//   form 2  the straight-line form as the passes write it (the dark MIS pass: f alone, no pdf chain); the retry loop exists
//           only inline in the stage routines (LightSampleTerm, BsdfSampleTerm, Continuation), so its three lines are repeated here
//   form 3  AccumulateF (mode 0); AccumulateSpecular / AccumulateFLocal as BsdfSampleTerm chooses (mode 1), into a column
//           of the lane's own
// Lanes past n leave at once, so a wave holds exactly the queries 64 w .. 64 w + 63 (form 2's tests are per wave).
template <int NL, unsigned TM>
__global__ void __launch_bounds__(BLOCK) k_bsdf_probe(DScene s, int material, int mode, int form, int flags, const float *in, uint32_t n, float *out) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float *q = in + 8 * (size_t)i;
    const int stride = form == 2 ? MI_BSDF_PROBE_STRAIGHT_FLOATS : MI_BSDF_PROBE_FLOATS;
    float *o = out + (size_t)stride * i;
    for (int k = 0; k < stride; ++k) o[k] = 0.f;
    const mi_material *mat = &s.materials[material];
    BSDFFrame fr;
    fr.m = mat;
    fr.mask = 0xffu;
    fr.ov.u = fr.ov.v = 0.f; fr.ov.onU = fr.ov.onV = false;
    fr.ov.sigMode = 0; fr.ov.sigA = fr.ov.sigB = 0.f;
    fr.ov.disney = false; fr.ov.rough = 0.f;
    fr.ns = V3(0, 0, 1); fr.ng = V3(0, 0, 1); fr.ss = Normalize(V3(1, 0, 0)); fr.ts = Cross(fr.ns, fr.ss);
    LobeTexT<NL> lt;
    const LobeTexT<NL> *ltp = nullptr;
    if constexpr ((TM & TM_TEXTURED) != 0) {   // (what TexturedScattering leaves for a material without image textures)
        lt.hasR = lt.hasS = lt.mulR = lt.mulS = 0u;
        lt.rules = 0u; lt.lum = 0.f; lt.hasK = 0u;
        lt.basis = s.rgbIllum; lt.textures = s.textures;
        ltp = &lt;
    }
    const V3 wo(q[0], q[1], q[2]);
    V3 wi(q[3], q[4], q[5]), wiLocal;
    float pdf = 0.f;
    int sampledType = 0;
    BSDFEvalT<NL> ev;
    ev.n = 0;
    bool ok = true;
    if (mode == 0) {
        if (form != 3) BSDF_f<NL, TM>(fr, wo, wi, flags, &ev);
        pdf = BSDF_Pdf<TM>(fr, wo, wi, flags);
    } else {
        wi = V3(0, 0, 0);
        if (form != 3) ok = BSDF_Sample_f<NL, TM, true>(fr, wo, &wi, q[6], q[7], &pdf, flags, &sampledType, &ev, &wiLocal);
        else if constexpr (ShadeAccum<NL, TM>) ok = BSDF_Sample_f<NL, TM, false>(fr, wo, &wi, q[6], q[7], &pdf, flags, &sampledType, &ev, &wiLocal);
        if (!ok) return;   // (a black sample: the oracle's record is all zero)
    }
    o[31] = pdf; o[32] = wi.x; o[33] = wi.y; o[34] = wi.z; o[35] = (float)sampledType;
    if (form == 0) {
        for (int b = 0; b < MI_NSPEC; ++b) o[b] = EvalBin<NL, TM>(ev, mat->bxdf, b, ltp);
    } else if (form == 1) {
#pragma unroll 1
        for (int c = 0; c < NQ; ++c) {
            const float4 fq = EvalQuad<NL, TM>(ev, mat->bxdf, c, ltp);
            for (int k = 0; k < 4; ++k) if (4 * c + k < MI_NSPEC) o[4 * c + k] = Get4(fq, k);
        }
    } else if (form == 2) {
        if constexpr (ShadeSimpleSpectra<NL, TM>) {
            const StraightPass<NL> sp = MakeStraightPass<NL, TM>(ev, mat->bxdf, MakePdfChain(MakeDivisor(1.f)));
            bool retried = false, bad = false;
#pragma unroll 1
            for (int c = 0; c < NQ; ++c) {
                DivTrack trk;
                float4 fq = StraightQuadF<NL, TM, false>(sp, false, c, c == NQ - 1, trk);
                bad |= trk.Bad();
                if (!QuadHolds<false>(trk)) {   // (the passes' retry: the quad again, every quotient by DivBy)
                    retried = true;
                    fq = StraightQuadF<NL, TM, true>(sp, false, c, c == NQ - 1, trk);
                }
                for (int k = 0; k < 4; ++k) if (4 * c + k < MI_NSPEC) o[4 * c + k] = Get4(fq, k);
            }
            o[36] = retried ? 1.f : 0.f;
            o[37] = bad ? 1.f : 0.f;
        }
    } else {
        if constexpr (ShadeAccum<NL, TM>) {
            float4 col[NQ];
            auto rd = [&](int c) -> float4 { return col[c]; };
            auto wr = [&](int c, const float4 &v) { col[c] = v; };
            if (mode == 0) AccumulateF<NL, TM>(fr, wo, wi, flags, ltp, rd, wr);
            else if (ev.n > 0) AccumulateSpecular<NL, TM>(ev.lobes[0], mat->bxdf, ltp, rd, wr);
            else AccumulateFLocal<NL, TM>(fr, fr.WorldToLocal(wo), wiLocal, Dot(wi, fr.ng) * Dot(wo, fr.ng) > 0, flags, ltp, rd, wr);
#pragma unroll 1
            for (int c = 0; c < NQ; ++c)
                for (int k = 0; k < 4; ++k) if (4 * c + k < MI_NSPEC) o[4 * c + k] = Get4(col[c], k);
        }
    }
}

struct BsdfProbeRow {
    int nl;
    unsigned tm, forms;
    void (*kernel)(DScene, int, int, int, int, const float *, uint32_t, float *);
};
#define MIPT_BSDF_PROBE_ROW(NL_, TM_) {NL_, (TM_) & TM_BSDF_BITS, 3u | (ShadeSimpleSpectra<NL_, ((TM_) & TM_BSDF_BITS)> ? 4u : 0u) | (ShadeAccum<NL_, ((TM_) & TM_BSDF_BITS)> ? 8u : 0u), \
                                       k_bsdf_probe<NL_, ((TM_) & TM_BSDF_BITS)>},
static const BsdfProbeRow kBsdfProbeRows[] = {MIPT_BSDF_PROBE_ROWS(MIPT_BSDF_PROBE_ROW)};
#undef MIPT_BSDF_PROBE_ROW
static const BsdfProbeRow *BsdfProbeRowOf(int nl, unsigned tm) {
    for (const BsdfProbeRow &r : kBsdfProbeRows)
        if (r.nl == nl && r.tm == (tm & TM_BSDF_BITS)) return &r;
    return nullptr;
}
unsigned BsdfProbeForms(int nl, unsigned tm) {
    const BsdfProbeRow *r = BsdfProbeRowOf(nl, tm);
    return r ? r->forms : 0u;
}
bool LaunchBsdfProbe(int nl, unsigned tm, const DScene &s, int material, int mode, int form, int flags, const float *dq, uint32_t n, float *dout) {
    const BsdfProbeRow *r = BsdfProbeRowOf(nl, tm);
    if (!r || form < 0 || form > 3 || !((r->forms >> form) & 1u)) return false;
    hipLaunchKernelGGL(r->kernel, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, 0, s, material, mode, form, flags, dq, n, dout);
    return true;
}
#endif   // MIPT_PART 4

#if MIPT_HAS_MAIN
// ------------------------------------------------------------------ kernel selection (pt_select.h)
// The functions and tables that name a kernel instance, for the host units: what they mention is instantiated here, in part 0.
template <int NL, unsigned TM, bool LENS>
constexpr auto MotionShadeKernel() -> void (*)(DScene, Pool, DevCounters *, unsigned) {
    if constexpr ((TM & TM_INSTANCES) != 0) return k_shade<NL, TM, LENS, true>;
    else return nullptr;
}
template <int NL, unsigned TM>
constexpr auto LensShadeKernel() -> void (*)(DScene, Pool, DevCounters *, unsigned) {
    if constexpr ((TM & TM_TEXTURED) != 0) return k_shade<NL, TM, true>;
    else return nullptr;
}
#define MIPT_SHADE_ENTRY(P_, NL_, TM_) {NL_, (TM_), {{k_shade<NL_, (TM_)>, LensShadeKernel<NL_, (TM_)>()}, {MotionShadeKernel<NL_, (TM_), false>(), MotionShadeKernel<NL_, (TM_), true>()}}},
static const ShadeInstance kShadeInstances[] = {MIPT_SHADE_INSTANCES(MIPT_SHADE_ENTRY)};
#undef MIPT_SHADE_ENTRY
static_assert(sizeof(kShadeInstances) / sizeof(kShadeInstances[0]) == N_SHADE_INSTANCES, "N_SHADE_INSTANCES (pt_select.h) counts the rows of MIPT_SHADE_INSTANCES");
const ShadeInstance &ShadeInstanceAt(int i) { return kShadeInstances[i]; }

// The k_shade instance of a shading class (an index into kShadeInstances, -1: none) from its lobe types and Fresnel kinds
// `types` and its longest lobe list `lobes` (the overflow class counts MI_MAX_BXDFS lobes; the miss class has neither
// types nor lobes, so it takes the matte instance). `hot`: the lights and sampler bits of the scene's variant of the matte
// and plastic instances.
// `disks`: the scene has disks, whose code only the instances compiled for every lobe, light and sampler hold (TM_HOLDS_DISKS):
// no class of such a scene fits an instance compiled for a subset, so those are the code they were before disks.
// `noise`: the scene has noise textures, or textures of the other classes and mappings that need the hit point or came with them
// (MI_TEX_IS_GENERAL), whose code only the general texture-evaluating instances hold (TM_HOLDS_NOISE): every
// textured class of such a scene goes there, and the textured matte and plastic instances are the code they were before.
// `projection`: the scene has a projection light, whose code the same instances hold as the disks' (TM_HOLDS_PROJECTION): any
// class can draw that light, so every class of such a scene goes where a scene with disks sends it.
int ShadeInstanceOf(unsigned types, int lobes, bool instanced, unsigned hot, bool disks, bool noise, bool projection) {
    disks |= projection;
    auto pick = [](int nl, unsigned tm) {
        for (int i = 0; i < N_SHADE_INSTANCES; ++i)
            if (kShadeInstances[i].nl == nl && kShadeInstances[i].tm == tm) return i;
        return -1;
    };
    auto fits = [types, disks](unsigned tm) { return !disks && (types & ~tm) == 0; };
    // (textured "disney" classes go to the eight-lobe instance whatever their lobe count: only that one reads the rules
    // that form their spectra from the colour -- LobeTexT::rules, d_bsdf.h)
    const unsigned disneyBits = (1u << MI_BXDF_DISNEY_DIFFUSE) | (1u << MI_BXDF_DISNEY_FAKE_SS) | (1u << MI_BXDF_DISNEY_RETRO) |
                                (1u << MI_BXDF_DISNEY_SHEEN) | (1u << MI_BXDF_DISNEY_CLEARCOAT) | (1u << (16 + MI_FRESNEL_DISNEY));
    const bool textured = (types & TM_TEXTURED) != 0, texturedDisney = textured && (types & disneyBits) != 0;
    // scenes with object instances: the two fully general instances, by lobe count
    if (instanced) return pick(lobes > 2 || texturedDisney ? MI_MAX_BXDFS : 2, TM_ALL);
    // the other instances are compiled for a subset of the lobe types and take the classes that fit
    if (!textured && lobes <= 2) {
        if (fits(TM_DIFFUSE)) return pick(2, TM_DIFFUSE | hot);
        if (fits(TM_PLASTIC)) return pick(2, TM_PLASTIC | hot);
        if (fits(TM_GLASS)) return pick(2, TM_GLASS | TM_LIGHTS_ALL | TM_SAMPLERS);
        return pick(2, TM_GENERIC);
    }
    if (!textured) {   // the lobe sets of "uber" and "disney": instances without the rest of the BxDF code
        if (lobes <= 4 && fits(TM_UBER)) return pick(4, TM_UBER | TM_LIGHTS_ALL | TM_SAMPLERS);
        if (fits(TM_DISNEY)) return pick(MI_MAX_BXDFS, TM_DISNEY | TM_LIGHTS_ALL | TM_SAMPLERS);
        return pick(lobes <= 4 ? 4 : MI_MAX_BXDFS, TM_GENERIC);
    }
    if (!noise && lobes <= 2 && fits(TM_DIFFUSE | TM_TEXTURED)) return pick(2, TM_DIFFUSE | TM_TEXTURED | TM_LIGHTS_ALL | TM_SAMPLERS);
    if (!noise && lobes <= 2 && fits(TM_PLASTIC | TM_TEXTURED)) return pick(2, TM_PLASTIC | TM_TEXTURED | TM_LIGHTS_ALL | TM_SAMPLERS);
    return pick(texturedDisney ? MI_MAX_BXDFS : lobes <= 2 ? 2 : lobes <= 4 ? 4 : MI_MAX_BXDFS, TM_FULL);
}

extern "C" int mi_pt_bsdf_probe(mi_pt *pt, int32_t material, int32_t instance, int32_t mode, int32_t form, int32_t flags, uint32_t n, const float *queries, float *out) {
    if (!pt || !queries || !out) { g_err = "null argument"; return MI_ERR_INVALID; }
    if (material < 0 || (size_t)material >= pt->materialLobes.size()) { g_err = "mi_pt_bsdf_probe: material index out of range"; return MI_ERR_INVALID; }
    if (instance < 0 || instance >= N_SHADE_INSTANCES) { g_err = "mi_pt_bsdf_probe: instance index out of range"; return MI_ERR_INVALID; }
    if (mode < 0 || mode > 1) { g_err = "mi_pt_bsdf_probe: mode must be 0 or 1"; return MI_ERR_INVALID; }
    if (pt->materialLobes[material] < 0) { g_err = "mi_pt_bsdf_probe: the material reads an image texture"; return MI_ERR_INVALID; }
    const ShadeInstance &si = kShadeInstances[instance];
    if (pt->materialLobes[material] > si.nl) { g_err = "mi_pt_bsdf_probe: the material has more lobes than the instance holds"; return MI_ERR_INVALID; }
    if (form < 0 || form > 3 || !((BsdfProbeForms(si.nl, si.tm) >> form) & 1u)) { g_err = "mi_pt_bsdf_probe: the instance does not compile this form"; return MI_ERR_INVALID; }
    if (n > (1u << 24)) { g_err = "mi_pt_bsdf_probe: more than 2^24 queries"; return MI_ERR_INVALID; }
    if (n == 0) return MI_OK;
    const size_t nOut = form == 2 ? MI_BSDF_PROBE_STRAIGHT_FLOATS : MI_BSDF_PROBE_FLOATS;
    return RunProbe(pt->device, queries, (size_t)n * 8 * sizeof(float), out, (size_t)n * nOut * sizeof(float), [&](void *dq, void *dout) {
        LaunchBsdfProbe(si.nl, si.tm, pt->scene, (int)material, (int)mode, (int)form, (int)flags, (const float *)dq, n, (float *)dout);
    });
}

// The k_trav instance of a ray class for the scene. Scenes with object instances always have the wide-4 records
// (BuildBvhTables) and never MODE 3 (misAny is 0 for them): three instances serve them.
template <int MODE>
static SceneKernel TravKernel(const mi_pt *pt) {
    if (pt->hasInstances)   // (never asked for MODE 3 or 4)
        return pt->scene.motions ? k_trav<MODE >= 3 ? 2 : MODE, true, 4, true, true> : k_trav<MODE >= 3 ? 2 : MODE, true, 4, true>;
    const bool w4 = pt->scene.bvhWidth == 4;
    if (pt->hasAlphaMasks) return w4 ? k_trav<MODE, true, 4> : k_trav<MODE, true, 2>;
    return w4 ? k_trav<MODE, false, 4> : k_trav<MODE, false, 2>;
}
SceneKernel TravKernelOf(const mi_pt *pt, int mode) {
    return mode == 0 ? TravKernel<0>(pt) : mode == 1 ? TravKernel<1>(pt) : mode == 3 ? TravKernel<3>(pt) : mode == 4 ? TravKernel<4>(pt) : TravKernel<2>(pt);
}

// The resolve kernels of the three ray classes, by [class][instanced].
static const SceneKernel kResolve[3][2] = {{k_resolve_extend<false>, k_resolve_extend<true>},
                                           {k_resolve_shadow<false>, k_resolve_shadow<true>},
                                           {k_resolve_mis<false>, k_resolve_mis<true>}};
SceneKernel ResolveKernelOf(const mi_pt *pt, int mode) { return kResolve[mode][pt->hasInstances ? 1 : 0]; }

OverflowKernel OverflowKernelOf(const mi_pt *pt) {
    return pt->hasInstances ? (pt->scene.motions ? k_resolve_overflow<true, true> : k_resolve_overflow<true>) : k_resolve_overflow<false>;
}
MetadataKernel MetadataCommitKernelOf(const mi_pt *pt) {
    return pt->hasInstances ? (pt->scene.motions ? k_commit_metadata<true, true> : k_commit_metadata<true>) : k_commit_metadata<false>;
}
TraceReadKernel TraceReadKernelOf(const mi_pt *pt) {
    return pt->hasInstances ? (pt->scene.motions ? k_trace_read<true, true> : k_trace_read<true>) : k_trace_read<false>;
}
#endif   // MIPT_HAS_MAIN


}  // namespace dptk
