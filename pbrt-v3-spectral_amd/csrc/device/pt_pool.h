// pt_pool.h -- what the kernels (pt_kernels.hip) and the host units (pt_create.hip, pt_render.hip) both read of the path pool
// and its counters: the planes of a slot and their layout (Pool), the slot flags, the device counters and the work
// description, and the tuning macros that both sides read. The MIPT_* defaults by side:
//   shared (here)        MIPT_STACK_LDS, MIPT_TRAV_BLOCKS_PER_CU, MIPT_TRAV_WAVES_PER_EU_ANY, MIPT_SLOT_CHUNKS
//   kernels only         MIPT_REFILL_BELOW, MIPT_TRI_BATCH, MIPT_COOP_KMAX, MIPT_TRAV_CHUNK, MIPT_TRAV_WAVES_PER_EU,
//                        MIPT_SHADE_WAVES_PER_EU (pt_kernels.hip)
//   host only            MIPT_DARK_BLOCKS_PER_CU, MIPT_DARK_AFTER_SHADOW, MIPT_QUEUE_GRID_RESIDENT (pt_render.hip)
// The Makefile gives HIPEXTRA to every unit, so a tuning build (tools/build_variants.sh) sees one value everywhere.
#pragma once
#include <cstddef>
#include "d_scene.h"

namespace dptk {   // (named: k_shade's instances are shared between the parts, so the types in its signature need linkage)

constexpr int BLOCK = 256;
#ifndef MIPT_STACK_LDS
#define MIPT_STACK_LDS 12
#endif
constexpr int STACK_LDS = MIPT_STACK_LDS;       // traversal stack entries (node, meta, tMin) staged in LDS per lane
constexpr int STACK_SPILL = 64 - STACK_LDS;     // deeper entries (pbrt allows 64 in total, bvh.cpp:670)
static_assert(STACK_LDS >= 1 && STACK_LDS <= 63 && STACK_LDS * BLOCK * 12 <= 160 * 1024, "MIPT_STACK_LDS: 1..63 entries, and the block's stack must fit the CU's LDS");

// ---- float planes
enum : int {
    P_FILMX = 0, P_FILMY,
    P_TENC0, P_TENC1, P_TENC2, P_TENC3,   // the ray's tMax when the k-th postponed quadric was met (closest-hit traversals)
    P_COUNT
};
// Camera "realistic" only: one more float plane behind the others (a pool is allocated with FloatPlanes(scene) of them) -- the
// weight GenerateRayDifferential returned for the slot's camera ray, which the film flush multiplies the sample by. A plane
// and not a second evaluation at the flush: the weight is the outcome of three to five lens traces.
constexpr int P_WEIGHT = P_COUNT;
// ... and, in front of image textures only (DScene::lensDiff), twelve more: the camera ray's scaled differentials rxOrigin,
// ryOrigin, rxDirection, ryDirection as LensCameraRay leaves them (they come from the offset rays' lens traces). k_generate
// writes them, the textured k_shade instances load them where they rebuild a perspective camera's from the film position.
constexpr int P_LENSDIFF = P_COUNT + 1, N_LENSDIFF = 12;
// ---- float4 record planes: values that are read and written together travel in one 16-B access
enum : int {
    R_RAY0 = 0,   // path ray: o.xyz, tMax
    R_RAY1,       //           d.xyz, etaScale
    R_SH0, R_SH1, // shadow ray (tMax = 1 - ShadowEpsilon): o.xyz d.x | d.y d.z - -
    R_MI0, R_MI1, // MIS ray: same packing
    R_HIT,        // t, b0, b1, b2 of the last traversal (path ray, or MIS ray)
    R_COUNT
};
// The two quads of a ray are neighbours in memory ([ray][slot][2]: 32 B per slot), so the pair a shading lane stores --
// and a traversal lane loads -- falls into ONE 64-B sector instead of two planes' sectors (the memory side moves whole
// sectors: a scattered 16-B store cost ~45 B there, PMC of round 1).
// ---- spectral planes. A 31-bin spectrum of a slot is stored as NQ = 8 float4 "quad planes": bins
// 4c..4c+3 of slot i at q[(set + c) * pool + i] (bin 31 is padding, kept 0 in everything that is summed or
// tested). One 16-B access per lane moves four bins, so a spectral pass issues a quarter of the memory
// instructions of one-float planes and -- the lanes of a shading wave hold scattered slots -- touches fewer
// cache lines per bin.
constexpr int NQ = 8;
enum : int {
    Q_L = 0,                // radiance gathered by the path
    Q_BETA = NQ,            // throughput
    Q_LB = 2 * NQ,          // the second line of the path's radiance (F_L_IN_B, F_CAND)
    Q_LMIS = 3 * NQ,        // pending BSDF-sample (MIS) contribution
    Q_COUNT = 4 * NQ,
    Q_LCA = Q_COUNT         // Integrator "spectralpath" only: the sample's stitched bands
};
// ---- int planes
enum : int { I_HITPRIM = 0, I_PIXEL, I_SAMPLE, I_IDXLO, I_IDXHI, I_DIM /* pixel samplers only: see StateWord */, I_FLAGS, I_MISLIGHT,
             I_NPEND, I_PEND0, I_PEND1, I_PEND2, I_PEND3,  // quadrics postponed by the traversal kernel
             I_BAND,                                       // spectralpath: band (path number) of the camera sample
             I_HITINST,                                    // instance the hit primitive was reached through, -1 = none (scenes with instances)
             I_COUNT };
constexpr int MAX_PEND = 4;
constexpr int PEND_OVERFLOW = 0x100;  // more quadrics met than MAX_PEND: the resolve kernel re-traverses
// ---- slot flags
enum : int {
    F_ALIVE = 1, F_FINISHED = 2, F_SPECULAR = 4, F_SHADOW = 8, F_MIS = 16, F_NEE = 32, F_A_ADDED = 64,
    // The path's radiance L has two lines, Q_L and Q_LB, and this bit says which one holds it. A light sample's contribution
    // used to wait in a line of its own until its shadow ray was resolved, and k_resolve_shadow then read it, read L and
    // wrote L: 384 B per unoccluded ray in a kernel that does nothing else. Now k_shade writes the CANDIDATE L + contribution
    // into the line that does not hold L (F_CAND; it has the throughput and the contribution in hand, and L costs it one
    // more read -- none while L is still empty), and an unoccluded ray flips this bit: the resolve moves no spectrum at all.
    F_L_IN_B = 128,
    // A new path has L = 0 and beta = 1. Writing those 16 quads into freshly (sparsely) refilled slots cost as
    // much as the rest of k_generate, so they stay implicit until something else is written there:
    F_L_ZERO = 256,     // Q_L holds no value yet; it reads as 0 (0 + x == x)
    F_BETA_ONE = 512,   // Q_BETA holds no value yet; it reads as 1 (1 * x == x)
    F_DIFF = 1024,      // the path ray is still the camera ray: it has ray differentials (RayDifferential::hasDifferentials)
    // F_CAND: the line that does not hold L holds L + the pending light sample's contribution (see F_L_IN_B); the shadow ray
    // decides. F_NEE_NZ: that contribution has a non-zero bin.
    F_CAND = 2048, F_NEE_NZ = 4096
};
// A DARK MIS ray has no flag: the BSDF-sampled ray is traced (the reference traces and counts it), but it cannot reach the
// sampled area light -- it misses the dilated bounds of the light's shape: Sphere::Pdf gives every direction the cone's pdf,
// sphere.cpp:294-310, so the estimate goes on for rays that point away from the sphere -- so its contribution is neither
// formed nor stored in Q_LMIS and nothing reads its answer. For the state machine such an estimate has no MIS ray at all
// (no F_MIS): the shadow ray's commit closes it (CommitShadowVerdict), or k_shade itself when there is no shadow ray either.
// Where the live MIS rays are visibility queries (DScene::misAny) the ray goes to a queue of its own (Pool::darkQ) and
// k_trav<4> traces it for the counters alone. In the other scenes it still goes to the MIS queue, marked in its record
// (MIS_EXCL_DARK), k_trav<2> answers MIS_ANSWER_DARK in the queue's answer words and touches no slot, and k_resolve_mis
// skips the entry on that word alone.
// The I_FLAGS word carries the path's bounce count and sampler dimension beside the flags: bits 0-13 the flags above, 14-21
// `bounces` (mi_pt_create bounds max_depth by 255), 22-31 the next sampler dimension (the Halton / Sobol' tables end at 1000 /
// 1024 dimensions; the random sampler only counts). Three 4-byte planes used to hold them: a shading lane read and wrote
// all three at scattered slots (~45 B each way at the memory side, PMC of round 2), k_generate stored all three per new
// path. One word: every kernel that reads the flags has the other two for nothing. (A pixel sampler's two table counters
// need 32 bits: they stay in the I_DIM plane.)
constexpr int FLAG_BITS = 14, FLAG_MASK = (1 << FLAG_BITS) - 1, BOUNCE_SHIFT = 14, DIM_SHIFT = 22;
static_assert(F_NEE_NZ < (1 << FLAG_BITS), "slot flags outgrew their field");
constexpr unsigned MIS_EXCL_BITS = 27, MIS_EXCL_NONE = (1u << MIS_EXCL_BITS) - 1u;
constexpr unsigned MIS_EXCL_DARK = MIS_EXCL_NONE - 1u;   // in place of the light's primitive: a dark ray (no primitive has this number, BuildLightPrims)
constexpr unsigned MIS_ANSWER_DARK = 0x80000000u;        // bit 31 of a MIS ray's second answer word (beside the postponed quadrics): a dark ray's

// Shading classes: materials with the same lobe-type list share a class (ids in order of
// first appearance, the 15th and later share class 14); class 15 holds the vertices without a
// BSDF (escaped rays, interface primitives). A wave of k_shade works on one class only.
constexpr int MAX_CLASSES = 16;
constexpr int MISS_CLASS = 15;

struct Pool {
    float *f;
    float4 *q;   // spectral quad planes
    float4 *r;   // record planes
    int *i;
    uint32_t *shadowQ, *misQ;  // compacted slot indices of this iteration's shadow / MIS rays. shadowQ[n + k]: the any-hit
                               // traversal's answer for entry k (bit 31: occluded; below it the count of postponed quadrics |
                               // PEND_OVERFLOW) -- in queue order, so k_resolve_shadow reads it as whole lines where the
                               // hit words of the slot planes cost it a sector each. misQ[n + 2k], [n + 2k + 1]: hit
                               // primitive and postponed quadrics of MIS ray k, likewise (its t and barycentrics, which
                               // k_resolve_mis rarely needs, stay in the slot's R_HIT). A dark ray's second word is
                               // MIS_ANSWER_DARK: k_resolve_mis skips the entry without touching its slot
    uint32_t *darkQ;           // DScene::misAny: the slots of this iteration's dark MIS rays (n entries), which then stay out of
                               // misQ. Nothing answers them: k_trav<4> walks this queue for the counters alone, on a stream
                               // of its own beside the next iteration (RenderSub)
    uint32_t *extQ;            // this iteration's path rays: new camera rays from the front (coherent: consecutive
                               // samples of a pixel), continuing paths from the back
    uint32_t *shadeQ;          // slots to shade: MAX_CLASSES queues of n entries, one per shading class
    uint32_t *ovfQ;            // rays whose list of postponed quadrics overflowed: 3 queues of n entries (extend / shadow / MIS)
    uint32_t n;
    // where (plane, slot) lies in f / i, in q and in r: the host reads single slots back through these (mi_pt_debug_path)
    __host__ __device__ __forceinline__ size_t ScalarIndex(int plane, uint32_t slot) const { return (size_t)plane * n + slot; }
    // a slot's 8 quads of one spectrum are one 128-B line: [spectrum][slot][quad] ([slot][spectrum][quad], the
    // spectra of a slot in one page, measured the same)
    __host__ __device__ __forceinline__ size_t QuadIndex(int plane, uint32_t slot) const { return (((size_t)(plane >> 3) * n + slot) << 3) + (plane & 7); }
    __host__ __device__ __forceinline__ size_t RecordIndex(int plane, uint32_t slot) const {
        return plane < R_HIT ? (((size_t)(plane >> 1) * n + slot) << 1) + (plane & 1) : (size_t)plane * n + slot;
    }
    DEV float &F(int plane, uint32_t slot) const { return f[ScalarIndex(plane, slot)]; }
    DEV float4 &Q(int plane, uint32_t slot) const { return q[QuadIndex(plane, slot)]; }
    // (the choice is made here once more, between two references: with it inside the index alone k_trav<2>, k_trav<3> and
    // k_shade come out with other register assignments and one to six instructions more or fewer)
    DEV float4 &R(int plane, uint32_t slot) const { return plane < R_HIT ? r[RecordIndex(plane, slot)] : r[ScalarIndex(plane, slot)]; }
    DEV int &I(int plane, uint32_t slot) const { return i[ScalarIndex(plane, slot)]; }
};

// Statistics are striped: STAT_STRIPES copies, each on its own 128-B line, picked by block
// index, so the per-wave atomics of a launch do not all serialise on one L2 line; the host
// adds the stripes up. The queue cursors cannot be striped (they hand out consecutive
// positions); they are bumped once per block instead (BlockReserve) and sit on lines of
// their own.
constexpr int STAT_STRIPES = 64;
struct alignas(128) DevStats {
    unsigned long long cameraRays, regularRays, shadowRays, totalPaths, zeroRadiancePaths, pathLengthSum, nodesVisited,
        triTests, badSamples, extendNodes, extendTris, extendRays;
    // the dark MIS rays (mi_pt_dark_launch_stats): rays k_trav<4> traced, entries its launches found in Pool::darkQ, and
    // entries of Pool::misQ that k_resolve_mis skipped as dark (scenes without the queue of their own)
    unsigned long long darkRays, darkEntries, misDarkSeen;
    // the traversal stacks (mi_pt_trav_stack_stats): entries k_trav pushed, and those of them beyond the LDS part
    unsigned long long stackPushed, stackBeyondLds;
};
static_assert(sizeof(DevStats) == 256, "a stripe of the statistics is two 128-B lines of its own");
struct alignas(128) DevCursor {
    unsigned int v;
};
struct DevCounters {
    DevStats stats[STAT_STRIPES];
    alignas(128) unsigned long long nextWork;   // global work counter
    // cleared together every iteration:
    DevCursor alive;                    // slots alive after generate
    DevCursor shadowCount, misCount;    // entries in Pool::shadowQ / misQ
    DevCursor primCount, contCount;     // entries at the front / back of Pool::extQ
    DevCursor shadeCount[MAX_CLASSES];  // entries in shading queue c
    DevCursor travNext[3];              // work cursors of the persistent traversal kernels (extend/shadow/mis)
    DevCursor ovfCount[3];              // entries in Pool::ovfQ (extend/shadow/mis)
    // NOT cleared with them: the dark traversal of iteration i runs beside iteration i + 1, whose clear it must not meet.
    // Whoever launches k_trav<4> clears both behind it, on the kernel's stream.
    DevCursor darkCount, darkNext;      // entries in Pool::darkQ, and the work cursor of k_trav<4>
};
constexpr size_t ITER_CLEAR_BYTES = sizeof(DevCursor) * (5 + MAX_CLASSES + 3 + 3);
constexpr size_t DARK_CLEAR_BYTES = sizeof(DevCursor) * 2;
static_assert(offsetof(DevCounters, darkCount) >= offsetof(DevCounters, alive) + ITER_CLEAR_BYTES && offsetof(DevCounters, darkNext) == offsetof(DevCounters, darkCount) + sizeof(DevCursor),
              "the dark cursors lie behind the block that every iteration clears, side by side");

struct WorkDesc {
    unsigned long long totalWork;
    int nTilesX, nTilesY, nTilesShard, shardIndex, shardCount;
    long long spp, sampleBegin;
    int run;   // consecutive samples of a pixel handed out together (a power of two dividing spp, at most MIPT_WORK_RUN = 16)
};

// Device bytes of one path slot: planes, records, spectra and its entries in the queues.
inline size_t PoolSlotBytes(int nQuadPlanes, int nFloatPlanes) {
    return (size_t)nFloatPlanes * sizeof(float) + (size_t)nQuadPlanes * sizeof(float4) + (size_t)R_COUNT * sizeof(float4) + (size_t)I_COUNT * sizeof(int) +
           (size_t)(7 + MAX_CLASSES + 3) * sizeof(uint32_t);
}

// A leaf's primitive count in the traversal records carries LEAF_SIMPLE when every primitive of the leaf is a triangle (no
// quadric to postpone, no instance to enter): those leaves go through the cooperative test of k_trav.
constexpr int LEAF_SIMPLE = 0x4000, LEAF_COUNT_MASK = 0x3fff;

// ---- tuning macros that size a grid on the host (pt_render.hip) and a loop or an occupancy in a kernel (pt_kernels.hip): one
// definition each, here. (MIPT_STACK_LDS above is one of them; the macros that only kernels read stay by those kernels.)
// The grid of the persistent traversal kernels (k_trav): blocks per CU, and the blocks of the any-hit instances that a CU holds.
#ifndef MIPT_TRAV_BLOCKS_PER_CU
#define MIPT_TRAV_BLOCKS_PER_CU 4
#endif
constexpr int TRAV_BLOCKS_PER_CU = MIPT_TRAV_BLOCKS_PER_CU;
static_assert(MIPT_TRAV_BLOCKS_PER_CU >= 1 && MIPT_TRAV_BLOCKS_PER_CU <= 8, "traversal tuning macros out of range");
#ifndef MIPT_TRAV_WAVES_PER_EU_ANY
#define MIPT_TRAV_WAVES_PER_EU_ANY 5   // the any-hit kernel (without the alpha-mask code): 96 VGPRs and a 24-KB stack allow five blocks per CU
#endif
// The k_trav modes that walk as the any-hit kernel does (1: shadow rays, 3: MIS rays as visibility queries, 4: dark MIS rays).
#define TRAV_IS_ANY(MODE_) ((MODE_) == 1 || (MODE_) == 3 || (MODE_) == 4)

// Slots per block of the kernels that walk the whole pool (k_generate, k_resolve_extend): SLOT_CHUNKS x 256. Every block
// ends in a returning atomicAdd on a queue cursor, and one word takes ~88 of those per microsecond whoever issues them
// (MI355X_MICROARCH.md, "dequeue"): with one 256-slot chunk per block a 32M-slot pool sent 131k adds to each cursor per
// launch, a floor of 1.5 ms under kernels that have 1.4-2 ms of work. Eight chunks per block: 16k adds, 0.19 ms.
#ifndef MIPT_SLOT_CHUNKS
#define MIPT_SLOT_CHUNKS 8
#endif
constexpr int SLOT_CHUNKS = MIPT_SLOT_CHUNKS;
// k_resolve_extend keeps a slot's rank within its (chunk, wave, class) in 8 bits per chunk of two 32-bit words (rankLo /
// rankHi), k_generate a bit per chunk in 32-bit masks and the block's slot numbers in 16 bits: more than 8 chunks would
// shift ranks out of their word (round 2's `-DMIPT_SLOT_CHUNKS=16` tuning build queued slots twice, overran a ray queue and
// died of a GPU memory fault -- the "Aborted" of gpurun_out/call_var.log -- which also left the device unusable for the two
// builds benched after it in that call). The tuning macros are checked where they are defined.
static_assert(SLOT_CHUNKS >= 1 && SLOT_CHUNKS <= 8, "MIPT_SLOT_CHUNKS: 1..8 (rank words of k_resolve_extend, chunk masks of k_generate)");
static_assert(SLOT_CHUNKS * BLOCK / 2 + SLOT_CHUNKS * BLOCK / 4 <= BLOCK * 33, "k_generate: the free-slot list and its flags live in the flush rows");

// The grid of k_resolve_overflow: fixed and small (its queue is empty for all but quadric-heavy scenes).
constexpr int OVERFLOW_GRID = 512;

}  // namespace dptk
