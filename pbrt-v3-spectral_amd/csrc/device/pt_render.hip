// pt_render.hip -- the path pool of a sub-renderer, the launches of one wavefront iteration, the render driver (RenderSub,
// RenderFrame) and the entry points that run those launches: the renders, the path dump, the recorded-ray traces and the
// read-outs of what a render left. Host code only: the kernels it launches are in pt_kernels.hip (pt_select.h).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "pt_host.h"

// Spectral quad planes of a path slot: spectralpath keeps one set more, the stitched spectrum of the camera sample (Q_LCA).
static int QuadPlanes(const DScene &s) { return Q_COUNT + (s.nBands > 1 ? NQ : 0); }
// Float planes of a path slot: a realistic camera keeps the ray weight (P_WEIGHT).
// (the orthographic and environment cameras have weight 1 and no such plane -- except in front of textures, where the
// differentials' planes keep their numbers behind it)
static int FloatPlanes(const DScene &s) { return P_COUNT + (s.cameraType == MI_CAMERA_REALISTIC || s.lensDiff ? 1 : 0) + (s.lensDiff ? N_LENSDIFF : 0) + (s.motions ? 1 : 0); }
// (the time plane of a scene with moving instances: the last one)
int TimePlaneOf(const DScene &s) { return s.motions ? FloatPlanes(s) - 1 : 0; }

static void FreePool(Pool &p) {
    hipFree(p.f); hipFree(p.q); hipFree(p.r); hipFree(p.i); hipFree(p.shadowQ); hipFree(p.extQ); hipFree(p.misQ); hipFree(p.darkQ); hipFree(p.shadeQ); hipFree(p.ovfQ);
    p = Pool{};   // n = 0, every pointer null: a later render cannot mistake a half-built pool for a usable one
}

// The one way a sub-renderer gives its pool back: the memory and every record of it, so that mi_pt_pool_info and the next
// render's memory budget count nothing that is no longer held.
void ReleasePool(SubRenderer &sub) {
    FreePool(sub.pool);
    sub.poolQuadPlanes = 0; sub.poolFloatPlanes = 0;
    sub.poolBytes = 0;
}

// The blocks that k_shade needs for the queues of `classes`: the kernel's prologue lays them back to back, each padded to
// whole blocks on its own, so the sum of the ceilings and not the ceiling of the sum.
unsigned long long ShadeGridBlocks(const uint32_t *counts, unsigned classes) {
    unsigned long long blocks = 0;
    for (int c = 0; c < MAX_CLASSES; ++c)
        if ((classes >> c) & 1u) blocks += ((unsigned long long)counts[c] + BLOCK - 1) / BLOCK;
    return blocks;
}

namespace {

// Samples per pixel of one pass.
long long PassSpp(const mi_pt *pt, const mi_render_params *rp) { return rp->spp_override > 0 ? rp->spp_override : pt->spp; }

// Failure-safe: the new pool is built aside and swapped in only when every allocation succeeded; after a failure the
// sub-renderer holds no pool at all (n == 0), so the next render allocates afresh instead of launching on stale sizes.
int EnsurePool(SubRenderer &sub, uint32_t n, int nQuadPlanes, int nFloatPlanes) {
    Pool &p = sub.pool;
    if (p.n == n && p.f && sub.poolQuadPlanes == nQuadPlanes && sub.poolFloatPlanes == nFloatPlanes) return MI_OK;
    ReleasePool(sub);
    Pool t{};
    const bool ok = hipMalloc((void **)&t.f, (size_t)nFloatPlanes * n * sizeof(float)) == hipSuccess &&
                    hipMalloc((void **)&t.q, (size_t)nQuadPlanes * n * sizeof(float4)) == hipSuccess &&
                    hipMalloc((void **)&t.r, (size_t)R_COUNT * n * sizeof(float4)) == hipSuccess &&
                    hipMalloc((void **)&t.i, (size_t)I_COUNT * n * sizeof(int)) == hipSuccess &&
                    hipMalloc((void **)&t.shadowQ, (size_t)2 * n * sizeof(uint32_t)) == hipSuccess &&
                    hipMalloc((void **)&t.extQ, (size_t)n * sizeof(uint32_t)) == hipSuccess &&
                    hipMalloc((void **)&t.misQ, (size_t)3 * n * sizeof(uint32_t)) == hipSuccess &&
                    hipMalloc((void **)&t.darkQ, (size_t)n * sizeof(uint32_t)) == hipSuccess &&
                    hipMalloc((void **)&t.shadeQ, (size_t)MAX_CLASSES * n * sizeof(uint32_t)) == hipSuccess &&
                    hipMalloc((void **)&t.ovfQ, (size_t)3 * n * sizeof(uint32_t)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();   // the failed hipMalloc must not poison the next call's hipGetLastError
        FreePool(t);
        g_err = "hipMalloc(path pool of " + std::to_string(n) + " slots) failed";
        return MI_ERR_NOMEM;
    }
    t.n = n;
    p = t;
    sub.poolQuadPlanes = nQuadPlanes;
    sub.poolFloatPlanes = nFloatPlanes;
    sub.poolBytes = (size_t)n * PoolSlotBytes(nQuadPlanes, nFloatPlanes);
    return MI_OK;
}

// -----------------------------------------------------------------------------
// The launches of one wavefront iteration, shared by RenderSub, the path-dump tool and mi_pt_trace_wavefront
// -----------------------------------------------------------------------------
// `closestMis`: the MIS rays (mode 2) with the closest-hit kernel even where the scene could ask them as visibility queries.
// Mode 4: the dark MIS rays of Pool::darkQ (DScene::misAny scenes only). `beside`: on that stream and on exactly `travGrid`.
void LaunchTraversal(mi_pt *pt, SubRenderer &sub, int mode, dim3 travGrid, bool closestMis = false, hipStream_t beside = nullptr) {
    if (mode == 2 && pt->scene.misAny && !closestMis) mode = 3;   // the MIS rays as visibility queries (k_trav, MODE 3)
    if (!beside && TRAV_IS_ANY(mode) && !pt->hasAlphaMasks && !pt->hasInstances && travGrid.x == (unsigned)pt->numCUs * TRAV_BLOCKS_PER_CU) travGrid.x = (unsigned)pt->numCUs * MIPT_TRAV_WAVES_PER_EU_ANY;   // (a full-size launch: one more block per CU)
    hipLaunchKernelGGL(TravKernelOf(pt, mode), travGrid, dim3(BLOCK), 0, beside ? beside : sub.stream, pt->scene, sub.pool, sub.ctr);
}

// The dark MIS rays (DScene::misAny: Pool::darkQ, k_trav<4>). Nothing inside the iteration reads what the kernel does -- it
// adds to regularRays, nodesVisited and triTests -- so it need not stand in the chain of dependent launches: it runs on
// SubRenderer::darkStream from the end of k_shade, beside the shadow and live MIS stages and the next iteration's k_generate,
// k_trav<0> and k_resolve_extend, on a grid small enough to leave those their blocks. It reads darkQ and the R_MI planes,
// whose next writer is the next k_shade: LaunchShade waits for evDarkDone. All ordering is stream events.
// MIPT_DARK_BLOCKS_PER_CU: the grid of that launch. MIPT_DARK_AFTER_SHADOW: hand over after k_resolve_shadow instead.
#ifndef MIPT_DARK_BLOCKS_PER_CU
#define MIPT_DARK_BLOCKS_PER_CU 3   // (same-box A/B of 1, 2, 3, 5 at both hand-over points: DESIGN.md, round 7)
#endif
#ifndef MIPT_DARK_AFTER_SHADOW
#define MIPT_DARK_AFTER_SHADOW 0
#endif
static_assert(MIPT_DARK_BLOCKS_PER_CU >= 1 && MIPT_DARK_BLOCKS_PER_CU <= MIPT_TRAV_WAVES_PER_EU_ANY, "MIPT_DARK_BLOCKS_PER_CU: 1 .. the blocks of the any-hit kernels that a CU holds");
static_assert(MIPT_DARK_AFTER_SHADOW == 0 || MIPT_DARK_AFTER_SHADOW == 1, "MIPT_DARK_AFTER_SHADOW: 0 or 1");

// The time of the launch in evDark[k] into the MIS class. Called when the host knows that launch complete.
void HarvestDark(SubRenderer &sub, int k) {
    if (!sub.darkTimed[k]) return;
    sub.darkTimed[k] = false;
    float ms = 0;
    if (hipEventElapsedTime(&ms, sub.evDark[k][0], sub.evDark[k][1]) == hipSuccess) sub.t[5] += ms * 1e-3;
    else (void)hipGetLastError();   // (a time not had is no reason to stop the render, and must not be taken for a launch's error)
}

int LaunchDarkBeside(mi_pt *pt, SubRenderer &sub, unsigned poolBlocks) {
    const int k = (int)(sub.darkSeq & 1);
    // the launch before the last used this set: the k_shade after it waited for its end, and the host has waited for the
    // main stream since (the read after k_generate)
    HarvestDark(sub, k);
    HIPCHK(hipEventRecord(sub.evDarkGo, sub.stream));
    HIPCHK(hipStreamWaitEvent(sub.darkStream, sub.evDarkGo, 0));
    HIPCHK(hipEventRecord(sub.evDark[k][0], sub.darkStream));
    LaunchTraversal(pt, sub, 4, dim3(std::min(poolBlocks, (unsigned)pt->numCUs * MIPT_DARK_BLOCKS_PER_CU)), false, sub.darkStream);
    HIPCHK(hipEventRecord(sub.evDark[k][1], sub.darkStream));
    HIPCHK(hipMemsetAsync(&sub.ctr->darkCount, 0, DARK_CLEAR_BYTES, sub.darkStream));
    HIPCHK(hipEventRecord(sub.evDarkDone, sub.darkStream));
    sub.darkTimed[k] = true;
    sub.darkPending = true;
    ++sub.darkSeq; ++sub.darkLaunches;
    return MI_OK;
}

// MIPT_DARK_STREAM=0, and the tools that step through an iteration: the same kernel in line, after the live MIS stage.
int LaunchDarkInLine(mi_pt *pt, SubRenderer &sub, dim3 travGrid) {
    LaunchTraversal(pt, sub, 4, travGrid);
    HIPCHK(hipMemsetAsync(&sub.ctr->darkCount, 0, DARK_CLEAR_BYTES, sub.stream));
    ++sub.darkLaunches;
    return MI_OK;
}

// Before the next writer of darkQ and the R_MI planes, and before the counters are read: the main stream behind the dark one.
int JoinDark(SubRenderer &sub) {
    if (sub.darkPending) HIPCHK(hipStreamWaitEvent(sub.stream, sub.evDarkDone, 0));
    sub.darkPending = false;
    return MI_OK;
}

// The grid of a kernel that walks a queue in steps of the grid (k_resolve_shadow, k_resolve_mis): QUEUE_GRID_RESIDENT times the
// blocks the device holds at once, at most the `poolBlocks` that cover the longest queue there can be. A block that finds
// its queue ended is not free, and a pool-sized grid has 390 k of them (0.18 ms per launch, however short the queue).
// MIPT_QUEUE_BLOCKS (read at every render; for tests) caps the grid.
#ifndef MIPT_QUEUE_GRID_RESIDENT
#define MIPT_QUEUE_GRID_RESIDENT 4
#endif
constexpr unsigned QUEUE_GRID_RESIDENT = MIPT_QUEUE_GRID_RESIDENT;
static_assert(QUEUE_GRID_RESIDENT >= 1 && QUEUE_GRID_RESIDENT <= 64, "MIPT_QUEUE_GRID_RESIDENT: 1..64");
dim3 QueueGrid(const mi_pt *pt, int blocksPerCU, unsigned poolBlocks) {
    unsigned want = (unsigned)pt->numCUs * (unsigned)std::max(1, blocksPerCU) * QUEUE_GRID_RESIDENT;
    if (pt->queueBlocksCap) want = std::min(want, pt->queueBlocksCap);
    return dim3(std::max(1u, std::min(want, poolBlocks)));
}
void ReadQueueBlocksCap(mi_pt *pt) {
    const char *e = getenv("MIPT_QUEUE_BLOCKS");
    pt->queueBlocksCap = e ? (unsigned)std::max(0, atoi(e)) : 0u;
    e = getenv("MIPT_SHADE_GRID");   // (read with it, at every render: "pool" = the grids before the class counts sized them)
    pt->shadeGridPool = e && strcmp(e, "pool") == 0;
    e = getenv("MIPT_DARK_STREAM");   // (likewise: "0" = the dark MIS rays in line on the main stream)
    pt->darkInLine = e && strcmp(e, "0") == 0;
}
// What follows the traversal of ray class `mode` (0: path rays, 1: shadow rays, 2: MIS rays): its resolve kernel on `grid`,
// then k_resolve_overflow for the rays that the quadric lists or the visibility queries (MODE 3) handed over.
void LaunchResolve(mi_pt *pt, SubRenderer &sub, int mode, dim3 grid) {
    if (mode != 0) grid = QueueGrid(pt, pt->resolveBlocksPerCU[mode], grid.x);   // (k_resolve_extend takes the pool's slots, not a queue)
    hipLaunchKernelGGL(ResolveKernelOf(pt, mode), grid, dim3(BLOCK), 0, sub.stream, pt->scene, sub.pool, sub.ctr);
    if (pt->hasQuadrics || (mode == 2 && pt->scene.misAny))
        hipLaunchKernelGGL(OverflowKernelOf(pt), dim3(OVERFLOW_GRID), dim3(BLOCK), 0, sub.stream, pt->scene, sub.pool, sub.ctr, mode);
}

// The last stage of a metadata pass (instead of LaunchShade and the shadow and MIS stages): every slot, one per thread.
void LaunchMetadataCommit(mi_pt *pt, SubRenderer &sub, dim3 grid) {
    hipLaunchKernelGGL(MetadataCommitKernelOf(pt), grid, dim3(BLOCK), 0, sub.stream, pt->scene, sub.pool, pt->primMeta, pt->metaStrategy);
}

// The shading queues' lengths of this iteration, on the host: one copy of the 16 cursors (a line each) into the
// sub-renderer's pinned block and one wait. After LaunchResolve(.., 0, ..), whose k_resolve_overflow appends to the queues too.
int ReadShadeCounts(SubRenderer &sub, uint32_t *counts) {
    HIPCHK(hipMemcpyAsync(sub.reads->shadeCount, sub.ctr->shadeCount, sizeof(sub.reads->shadeCount), hipMemcpyDeviceToHost, sub.stream));
    HIPCHK(hipStreamSynchronize(sub.stream));
    for (int c = 0; c < MAX_CLASSES; ++c) counts[c] = sub.reads->shadeCount[c].v;
    return MI_OK;
}

// Every k_shade instance of the plan on the blocks its queues fill (an instance with empty queues is not launched): a
// block past the queues is not free (1.4 ns each, 0.53 ms per launch on the 96M-slot pool's 393 232), and in a full iteration
// the instances share one pool's worth of vertices. The price is a host round trip per iteration (ReadShadeCounts).
// MIPT_SHADE_GRID=pool: `grid` (the pool's blocks) + MAX_CLASSES for every instance, as before, and no read.
int LaunchShade(mi_pt *pt, SubRenderer &sub, dim3 grid) {
    uint32_t counts[MAX_CLASSES];
    if (!pt->shadeGridPool) {
        const int rc = ReadShadeCounts(sub, counts);
        if (rc != MI_OK) return rc;
    }
    {   // (behind the read, so that the host does not wait for the dark traversal as well)
        const int rc = JoinDark(sub);
        if (rc != MI_OK) return rc;
    }
    for (int i = 0; i < N_SHADE_INSTANCES; ++i) {
        if (!pt->shadeClasses[i]) continue;
        const unsigned long long blocks = pt->shadeGridPool ? (unsigned long long)grid.x + MAX_CLASSES : ShadeGridBlocks(counts, pt->shadeClasses[i]);
        if (blocks == 0) continue;
        const ShadeInstance &si = ShadeInstanceAt(i);
        const bool lens = pt->scene.lensDiff && si.kernel[0][1];   // (a realistic camera in front of textures: the twin that loads the stored differentials)
        const bool motion = pt->scene.motions && si.kernel[1][0];   // (moving instances: the twin that interpolates)
        hipLaunchKernelGGL(si.kernel[motion][lens], dim3((unsigned)blocks), dim3(BLOCK), 0, sub.stream, pt->scene, sub.pool, sub.ctr, pt->shadeClasses[i]);
        ++sub.shadeLaunches;
        sub.shadeBlocks += blocks;
    }
    return MI_OK;
}

// Tiles of 16 samples along one axis of the sample bounds.
int TilesAlong(const DScene &s, int axis) { return (s.sampleBounds[2 + axis] - s.sampleBounds[axis] + 15) / 16; }

// The work of one pass of one sub-renderer: of the 16 x 16 tiles of the sample bounds every shardCount-th from shardIndex on,
// `spp` samples from sample number `sampleBegin` in each of their pixels, handed out in runs (MIPT_WORK_RUN caps them).
// mi_pt_debug_path asks the same way for the one tile of its pixel.
WorkDesc PlanWork(const DScene &s, int shardIndex, int shardCount, long long spp, long long sampleBegin) {
    WorkDesc wd{};
    wd.nTilesX = TilesAlong(s, 0);
    wd.nTilesY = TilesAlong(s, 1);
    const int nTiles = wd.nTilesX * wd.nTilesY;
    wd.shardIndex = shardIndex;
    wd.shardCount = shardCount;
    wd.nTilesShard = (wd.shardIndex < nTiles) ? (nTiles - wd.shardIndex + wd.shardCount - 1) / wd.shardCount : 0;
    wd.spp = spp;
    wd.sampleBegin = sampleBegin;
    wd.totalWork = (unsigned long long)wd.nTilesShard * 256ull * (unsigned long long)wd.spp;
    int runCap = 256;  // (round 3, with the dense film flush: 64 -> 256 takes 5 % off k_generate, killeroo +0.9 %, the 10M-triangle scene
                       // +0.7 %, cornell-glass the same; 1024 measures as 256. Same-box A/B at the end of round 2: 16 -> 64 took 4 % off k_generate and 1 % off the camera-ray
                       // traversal, the other kernels unchanged -- 3596 -> 3620 Mray/s; 128 ... 1024 measure the same as 64.
                       // Earlier in the round longer runs cost the shading kernels 2-5 % and 16 was the optimum.)
    if (const char *e = getenv("MIPT_WORK_RUN")) runCap = std::max(1, atoi(e));
    wd.run = 1;
    while (2 * wd.run <= runCap && wd.spp % (2 * wd.run) == 0) wd.run *= 2;
    return wd;
}

// The pool of a render of `wd` on one of `subCount` sub-renderers, its slots of nQuadPlanes and nFloatPlanes: `pathPool` slots
// in all (mi_render_params.path_pool), or by default what the work, the measurements below and the device's free memory
// ask for. Allocated (EnsurePool) when this returns MI_OK, `poolN` slots.
int SizePool(SubRenderer &sub, const WorkDesc &wd, uint32_t pathPool, int subCount, int nQuadPlanes, int nFloatPlanes, uint32_t &poolN) {
    // Default pool: one slot per sample to render, up to the cap (earlier in round 2, at half: a 1/8 shard took 0.1196 s with the
    // quarter's 16M slots, 0.1169 s with 32M), at most 96M slots in total (below)
    // and at least 4M (8M per sub-renderer when several share the GPU): bigger pools mean fewer, better-filled
    // launches, but the last iterations of a render drain the pool at low occupancy, which a small job (one
    // shard of a multi-GPU frame) feels. Measured on the 1024-spp killeroo frame and its shards
    // (tools/shard_tune.py): a 1/8 shard on four sub-renderers takes 0.149 s with 16M slots and 0.143 s with
    // 32M; 64M slots (47 GB) make the traversal launches 3 % faster and k_shade / k_generate 4-6 % slower
    // (the path state outgrows the TLB reach), no gain for the full frame.
    poolN = pathPool;
    if (poolN == 0) {
        const unsigned long long quarter = wd.totalWork * (unsigned long long)subCount;   // (all of them: a 1/8 shard of the killeroo frame takes 0.1071 s on 32M slots, 0.1046 s on 64M)
        const unsigned long long floorN = subCount > 1 ? (8ull << 20) * (unsigned long long)subCount : (1ull << 22);
        // (`quarter`: half, since round 2.) The cap: 96M slots = 77 GB of path state of the 288 GB. With the kernels of the end
        // of round 2 bigger pools pay again (fewer, longer launches: the persistent traversal kernels lose less to their
        // tails, k_shade and k_generate no longer slow down): killeroo 1024 spp 3740 Mray/s at 32M, 3880 at 64M, 3912 at
        // 96M, 3931 at 128M; the 10M-triangle scene +0.4 %, cornell-glass -0.3 % at 64M.
        poolN = (uint32_t)std::min<unsigned long long>(3ull << 25, std::max<unsigned long long>(floorN, quarter));
    }
    poolN = std::max<uint32_t>(BLOCK, poolN / subCount / BLOCK * BLOCK);
    if (pathPool == 0) {
        // the default is a preference: it takes at most 65 % of what the device has free (counting what this sub-renderer's
        // present pool would give back), so that what comes after the pool -- the film staging of the hand-over, RCCL's
        // buffers at the first collective, another renderer in the process -- still finds memory
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) == hipSuccess) {
            const size_t budget = (size_t)(0.65 * (double)(freeB + sub.poolBytes)) / (size_t)subCount;
            const size_t fit = budget / PoolSlotBytes(nQuadPlanes, nFloatPlanes) / BLOCK * BLOCK;
            if (fit < poolN) poolN = (uint32_t)std::max<size_t>(fit, (size_t)BLOCK);
        } else (void)hipGetLastError();
    }
    if (wd.totalWork < poolN) poolN = (uint32_t)((wd.totalWork + BLOCK - 1) / BLOCK * BLOCK);
    if (poolN < BLOCK) poolN = BLOCK;
    int rc = EnsurePool(sub, poolN, nQuadPlanes, nFloatPlanes);
    // the default size is a preference, not a requirement: on a device that cannot hold it the render goes on with half,
    // a quarter, ... (an explicit mi_render_params.path_pool is taken at its word and fails)
    while (rc == MI_ERR_NOMEM && pathPool == 0 && poolN > (1u << 22)) {
        poolN = poolN / 2 / BLOCK * BLOCK;
        rc = EnsurePool(sub, poolN, nQuadPlanes, nFloatPlanes);
    }
    return rc;
}

}  // namespace

extern "C" {

// One sub-renderer = one path pool with its queues and counters on its own HIP stream.
// mi_pt_render splits its tile shard over pt->subs.size() sub-renderers that run
// concurrently (one host thread each): while one pool is in a traversal kernel's tail
// the other pool's kernels fill the idle CUs, which a single dependent chain of launches
// cannot do.
static int RenderSub(mi_pt *pt, SubRenderer &sub, const mi_render_params *rp, int subIndex, int subCount) {
    HIPCHK(hipSetDevice(pt->device));
    hipStream_t st = sub.stream;
    const DScene &s = pt->scene;
    const WorkDesc wd = PlanWork(s, rp->shard_index + rp->shard_count * subIndex, rp->shard_count * subCount, PassSpp(pt, rp), rp->sample_begin);
    sub.iterations = 0;
    sub.shadeLaunches = sub.shadeBlocks = 0;
    // (a render that failed half way may have left the dark stream busy: nothing of it may meet this render's clears)
    HIPCHK(hipStreamSynchronize(sub.darkStream));
    sub.darkPending = false; sub.darkTimed[0] = sub.darkTimed[1] = false;
    sub.darkLaunches = 0;
    for (double &t : sub.t) t = 0;
    sub.result = DevCounters{};
    if (wd.totalWork == 0) return MI_OK;
    uint32_t poolN = 0;
    int rc = SizePool(sub, wd, rp->path_pool, subCount, QuadPlanes(s), FloatPlanes(s), poolN);
    if (rc != MI_OK) return rc;
    HIPCHK(hipMemsetAsync(sub.pool.i + (size_t)I_FLAGS * poolN, 0, (size_t)poolN * sizeof(int), st));
    HIPCHK(hipMemsetAsync(sub.ctr, 0, sizeof(DevCounters), st));
    const dim3 grid((poolN + BLOCK - 1) / BLOCK), block(BLOCK);
    const dim3 chunkGrid((grid.x + SLOT_CHUNKS - 1) / SLOT_CHUNKS);   // kernels that take SLOT_CHUNKS x 256 slots per block
    const dim3 travGrid(std::min<unsigned>(grid.x, (unsigned)pt->numCUs * TRAV_BLOCKS_PER_CU));
    // Per-kernel-class time: HIP events at the kernel boundaries of every iteration,
    // read back after the per-iteration sync that the alive counter needs anyway.
    // (first event, second event, the class in SubRenderer::t that the time between them goes to)
    static const int kSpans[][3] = {{0, 1, 1}, {1, 2, 2}, {2, 3, 3}, {3, 4, 4}, {4, 5, 5},
                                    // the closest-hit traversal launch alone: from an event recorded right before it (after the host's
                                    // per-iteration read of `alive`), so the host round trip is in [2] but not in [6]
                                    {7, 6, 6}};
    auto harvest = [&](int set, bool full) {   // (`full`: the iteration went on past k_generate, whose span comes first)
        float ms = 0;
        for (const int (&sp)[3] : kSpans) {
            hipEventElapsedTime(&ms, sub.evIter[set][sp[0]], sub.evIter[set][sp[1]]); sub.t[sp[2]] += ms * 1e-3;
            if (!full) return;
        }
    };
    int set = 0;
    bool havePrev = false;   // the other event set holds a full iteration whose times are not in sub.t yet
    while (true) {
        hipEvent_t *ev = sub.evIter[set];
        HIPCHK(hipMemsetAsync(&sub.ctr->alive, 0, ITER_CLEAR_BYTES, st));
        HIPCHK(hipEventRecord(ev[0], st));
        hipLaunchKernelGGL(GenerateKernelOf(s), chunkGrid, block, 0, st, s, sub.pool, pt->film, sub.ctr, wd);
        HIPCHK(hipEventRecord(ev[1], st));
        HIPCHK(hipMemcpyAsync(&sub.reads->alive, &sub.ctr->alive.v, sizeof(unsigned), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&sub.reads->drawn, &sub.ctr->nextWork, sizeof(sub.reads->drawn), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const unsigned alive = sub.reads->alive;
        const unsigned long long drawn = sub.reads->drawn;
        if (havePrev) harvest(set ^ 1, true);
        // done when no path is alive and every work item has been drawn (an iteration can draw nothing but items outside
        // the pixel bounds and leave the pool empty with work still to hand out)
        if (alive == 0) {
            harvest(set, false);
            if (drawn >= wd.totalWork) break;
        } else {
            HIPCHK(hipEventRecord(ev[7], st));
            LaunchTraversal(pt, sub, 0, travGrid);
            HIPCHK(hipEventRecord(ev[6], st));
            LaunchResolve(pt, sub, 0, chunkGrid);
            HIPCHK(hipEventRecord(ev[2], st));
            if (pt->metaStrategy >= 0) {   // a metadata pass: the hit is the answer (its commit is timed as the shade class; no shadow or MIS rays)
                LaunchMetadataCommit(pt, sub, grid);
                HIPCHK(hipEventRecord(ev[3], st));
                HIPCHK(hipEventRecord(ev[4], st));
                HIPCHK(hipEventRecord(ev[5], st));
            } else {
                const bool darkBeside = s.misAny && !pt->darkInLine;
                if ((rc = LaunchShade(pt, sub, grid)) != MI_OK) return rc;
                HIPCHK(hipEventRecord(ev[3], st));
                if (darkBeside && !MIPT_DARK_AFTER_SHADOW && (rc = LaunchDarkBeside(pt, sub, grid.x)) != MI_OK) return rc;
                LaunchTraversal(pt, sub, 1, travGrid);
                LaunchResolve(pt, sub, 1, grid);
                HIPCHK(hipEventRecord(ev[4], st));
                if (darkBeside && MIPT_DARK_AFTER_SHADOW && (rc = LaunchDarkBeside(pt, sub, grid.x)) != MI_OK) return rc;
                LaunchTraversal(pt, sub, 2, travGrid);
                LaunchResolve(pt, sub, 2, grid);
                if (s.misAny && pt->darkInLine && (rc = LaunchDarkInLine(pt, sub, travGrid)) != MI_OK) return rc;
                HIPCHK(hipEventRecord(ev[5], st));
            }
            HIPCHK(hipGetLastError());   // a launch of this iteration that was refused (bad configuration) stops the render here
        }
        havePrev = alive != 0;
        set ^= 1;
        if (++sub.iterations > 100000000ull) { g_err = "render loop did not terminate"; return MI_ERR_HIP; }
    }
    if ((rc = JoinDark(sub)) != MI_OK) return rc;   // the last iteration's dark rays are in the counters too
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipStreamSynchronize(sub.darkStream));
    HarvestDark(sub, 0); HarvestDark(sub, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(&sub.result, sub.ctr, sizeof(DevCounters), hipMemcpyDeviceToHost));
    sub.stackPushed = sub.stackBeyondLds = 0;
    for (const DevStats &r : sub.result.stats) { sub.stackPushed += r.stackPushed; sub.stackBeyondLds += r.stackBeyondLds; }
    return MI_OK;
}

// One frame (or pass, or shard) into the film and out to the caller: the body shared by mi_pt_render and mi_pt_render_metadata,
// which differ in pt->metaStrategy and in the DScene the pass sees.
static int RenderFrame(mi_pt *pt, const mi_render_params *rp, float *film_sum, float *weight_sum, mi_counters *counters) {
    if (!pt || !rp) { g_err = "null argument"; return MI_ERR_INVALID; }
    if (rp->shard_count < 1 || rp->shard_index < 0 || rp->shard_index >= rp->shard_count) { g_err = "bad shard"; return MI_ERR_INVALID; }
    {   // sample numbers are ints in the path state (I_SAMPLE) and in the oracle: [sample_begin, sample_begin + spp) stays below 2^31 - 1
        const long long passSpp = PassSpp(pt, rp);
        if (rp->sample_begin < 0 || rp->sample_begin > 0x7fffffffll || passSpp > 0x7fffffffll - rp->sample_begin) {
            g_err = "sample numbers out of range: sample_begin >= 0 and sample_begin + spp <= 2^31 - 1";
            return MI_ERR_INVALID;
        }
    }
    if (pt->scene.samplerType >= MI_SAMPLER_ZEROTWO &&
        (rp->sample_begin < 0 || rp->sample_begin + PassSpp(pt, rp) > pt->spp)) {
        g_err = "a pixel sampler (02sequence / stratified) has tables for samples_per_pixel samples: the pass asks for sample numbers beyond them";
        return MI_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(pt->device));
    ReadQueueBlocksCap(pt);
    {   // what this pass lets the kernels leave out (DScene::index32 / storePixelSample)
        DScene &sc = pt->scene;
        const unsigned long long lastSample = (unsigned long long)rp->sample_begin + (unsigned long long)PassSpp(pt, rp);
        sc.index32 = (sc.samplerType == MI_SAMPLER_HALTON && (lastSample + 1ull) * (unsigned long long)std::max(1, sc.sampleStride) < (1ull << 32)) ? 1 : 0;
        sc.storePixelSample = (sc.samplerType >= MI_SAMPLER_RANDOM || sc.nBands > 1 || (pt->nTextures > 0 && (sc.camera.lens_radius > 0 || sc.camera.animated))) ? 1 : 0;
    }
    hipStream_t st = (hipStream_t)rp->stream;
    if (!(rp->flags & MI_RENDER_ACCUMULATE)) HIPCHK(hipMemsetAsync(pt->film, 0, pt->nPix * 32 * sizeof(float), st));
    HIPCHK(hipStreamSynchronize(st));
    if (!(rp->flags & MI_RENDER_FILM_ON_DEVICE)) {   // the hand-over's staging before the pools size themselves
        if (film_sum && !pt->stageSum) HIPCHK(hipMalloc((void **)&pt->stageSum, pt->nPix * 31 * sizeof(float)));
        if (weight_sum && !pt->stageW) HIPCHK(hipMalloc((void **)&pt->stageW, pt->nPix * sizeof(float)));
    }
    const int nSub = (int)pt->subs.size();
    std::vector<int> rcs(nSub, MI_OK);
    std::vector<std::string> errs(nSub);
    const auto t0 = std::chrono::steady_clock::now();
    {
        std::vector<std::thread> threads;
        for (int k = 1; k < nSub; ++k)
            threads.emplace_back([&, k] { rcs[k] = RenderSub(pt, pt->subs[k], rp, k, nSub); errs[k] = g_err; });
        rcs[0] = RenderSub(pt, pt->subs[0], rp, 0, nSub);
        errs[0] = g_err;
        for (auto &t : threads) t.join();
    }
    for (int k = 0; k < nSub; ++k)
        if (rcs[k] != MI_OK) {
            // a failed sub-renderer may have left kernels queued: nothing of the caller's may be touched after we return
            (void)hipDeviceSynchronize();
            g_err = errs[k];
            return rcs[k];
        }
    HIPCHK(hipDeviceSynchronize());
    pt->lastSeconds[0] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    unsigned long long iterations = 0;
    DevStats c{};
    for (int i = 1; i < 7; ++i) pt->lastSeconds[i] = 0;
    for (const SubRenderer &sub : pt->subs) {
        for (int i = 1; i < 7; ++i) pt->lastSeconds[i] += sub.t[i];
        iterations += sub.iterations;
        for (const DevStats &r : sub.result.stats) {
            c.cameraRays += r.cameraRays; c.regularRays += r.regularRays; c.shadowRays += r.shadowRays;
            c.totalPaths += r.totalPaths; c.zeroRadiancePaths += r.zeroRadiancePaths; c.pathLengthSum += r.pathLengthSum;
            c.nodesVisited += r.nodesVisited; c.triTests += r.triTests; c.badSamples += r.badSamples;
            c.extendNodes += r.extendNodes; c.extendTris += r.extendTris; c.extendRays += r.extendRays;
        }
    }
    if (counters) {
        *counters = mi_counters{};
        counters->camera_rays = c.cameraRays; counters->regular_rays = c.regularRays; counters->shadow_rays = c.shadowRays;
        counters->total_paths = c.totalPaths; counters->zero_radiance_paths = c.zeroRadiancePaths;
        counters->path_length_sum = c.pathLengthSum; counters->bvh_nodes_visited = c.nodesVisited;
        counters->tri_tests = c.triTests; counters->bad_samples = c.badSamples;
        counters->iterations = iterations;
        counters->extend_rays = c.extendRays;
        counters->extend_nodes = c.extendNodes; counters->extend_tri_tests = c.extendTris;
        counters->launches[0] = counters->launches[1] = counters->launches[2] = iterations;
    }
    if (film_sum || weight_sum) {
        const bool onDev = (rp->flags & MI_RENDER_FILM_ON_DEVICE) != 0;
        float *dSum = nullptr, *dW = nullptr;
        if (onDev) { dSum = film_sum; dW = weight_sum; }
        else {   // staging for the host hand-over: allocated once per renderer (above), freed by mi_pt_destroy
            if (film_sum) dSum = pt->stageSum;
            if (weight_sum) dW = pt->stageW;
        }
        size_t total = pt->nPix * 32;
        hipLaunchKernelGGL(k_film_split, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, pt->film, dSum, dW, pt->nPix);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        if (!onDev) {
            if (film_sum) HIPCHK(hipMemcpy(film_sum, dSum, pt->nPix * 31 * sizeof(float), hipMemcpyDeviceToHost));
            if (weight_sum) HIPCHK(hipMemcpy(weight_sum, dW, pt->nPix * sizeof(float), hipMemcpyDeviceToHost));
        }
    }
    return MI_OK;
}

int mi_pt_render(mi_pt *pt, const mi_render_params *rp, float *film_sum, float *weight_sum, mi_counters *counters) {
    return RenderFrame(pt, rp, film_sum, weight_sum, counters);
}

int mi_pt_render_metadata(mi_pt *pt, const mi_render_params *rp, int strategy, float *film_sum, float *weight_sum, mi_counters *counters) {
    if (!pt || !rp) { g_err = "null argument"; return MI_ERR_INVALID; }
    if (strategy < MI_METADATA_DEPTH || strategy > MI_METADATA_COORDINATES) { g_err = "mi_pt_render_metadata: unknown strategy"; return MI_ERR_INVALID; }
    if (pt->primMetaHost.size() != pt->scene.nPrims) { g_err = "mi_pt_render_metadata: the scene description came without prim_meta"; return MI_ERR_INVALID; }
    HIPCHK(hipSetDevice(pt->device));
    if (!pt->primMeta) {   // the first metadata pass of this renderer
        const int rc = Upload(pt, pt->primMetaHost.data(), pt->primMetaHost.size(), &pt->primMeta);
        if (rc != MI_OK) { pt->primMeta = nullptr; return rc; }
    }
    // the pass's own view of the scene, as mi_pt_debug_path takes one: no depth limit ends a hit before the commit
    // (EndsUnshaded), one ray per camera sample whatever "spectralpath" asks for
    SceneViewGuard restore{pt};
    pt->scene.maxDepth = 255;
    pt->scene.nBands = 1;
    pt->scene.bandDelta = MI_NSPEC;
    pt->scene.ignoreRayWeight = 1;   // MetadataIntegrator::IgnoreRayWeight (metadata.h:64): a vignetted sample adds zeros with weight 1
    pt->metaStrategy = strategy;
    return RenderFrame(pt, rp, film_sum, weight_sum, counters);
}

int mi_pt_device_film(mi_pt *pt, void **dev_ptr, uint64_t *n_floats) {
    if (!pt || !dev_ptr || !n_floats) { g_err = "null argument"; return MI_ERR_INVALID; }
    *dev_ptr = pt->film;
    *n_floats = pt->nPix * 32;
    return MI_OK;
}

int mi_pt_pool_info(mi_pt *pt, uint64_t *slots, uint64_t *bytes) {
    if (!pt || !slots || !bytes) { g_err = "null argument"; return MI_ERR_INVALID; }
    *slots = 0; *bytes = 0;
    for (const SubRenderer &sub : pt->subs) { *slots += sub.pool.n; *bytes += sub.poolBytes; }
    return MI_OK;
}

int mi_pt_last_timings(mi_pt *pt, double *seconds, int n) {
    if (!pt || !seconds) { g_err = "null argument"; return MI_ERR_INVALID; }
    for (int i = 0; i < n && i < 8; ++i) seconds[i] = pt->lastSeconds[i];
    return MI_OK;
}

int mi_pt_shade_launch_stats(mi_pt *pt, uint64_t *launches, uint64_t *blocks) {
    if (!pt || !launches || !blocks) { g_err = "null argument"; return MI_ERR_INVALID; }
    *launches = 0; *blocks = 0;
    for (const SubRenderer &sub : pt->subs) { *launches += sub.shadeLaunches; *blocks += sub.shadeBlocks; }
    return MI_OK;
}

int mi_pt_dark_launch_stats(mi_pt *pt, uint64_t *launches, uint64_t *entries, uint64_t *rays, uint64_t *resolve_skipped) {
    if (!pt || !launches || !entries || !rays || !resolve_skipped) { g_err = "null argument"; return MI_ERR_INVALID; }
    *launches = 0; *entries = 0; *rays = 0; *resolve_skipped = 0;
    for (const SubRenderer &sub : pt->subs) {
        *launches += sub.darkLaunches;
        for (const DevStats &r : sub.result.stats) { *entries += r.darkEntries; *rays += r.darkRays; *resolve_skipped += r.misDarkSeen; }
    }
    return MI_OK;
}

int mi_pt_trav_stack_stats(mi_pt *pt, uint64_t out[2]) {
    if (!pt || !out) { g_err = "null argument"; return MI_ERR_INVALID; }
    out[0] = out[1] = 0;
    for (const SubRenderer &sub : pt->subs) { out[0] += sub.stackPushed; out[1] += sub.stackBeyondLds; }
    return MI_OK;
}

int mi_pt_light_distribution(mi_pt *pt, float *func, float *func_int, uint64_t capacity_voxels) {
    if (!pt) { g_err = "null argument"; return MI_ERR_INVALID; }
    const DScene &s = pt->scene;
    if (s.ldType != MI_LD_SPATIAL || s.nLights == 0) { g_err = "mi_pt_light_distribution: the scene has no spatial light distribution"; return MI_ERR_INVALID; }
    const size_t nVox = (size_t)s.nVoxels[0] * s.nVoxels[1] * s.nVoxels[2];
    if (capacity_voxels < nVox) { g_err = "mi_pt_light_distribution: buffer too small"; return MI_ERR_INVALID; }
    HIPCHK(hipSetDevice(pt->device));
    if (func) HIPCHK(hipMemcpy(func, s.ldFunc, nVox * s.nLights * sizeof(float), hipMemcpyDeviceToHost));
    if (func_int) HIPCHK(hipMemcpy(func_int, s.ldFuncInt, nVox * sizeof(float), hipMemcpyDeviceToHost));
    return MI_OK;
}

// Parity tool: one camera sample through the wavefront pipeline with a 256-slot pool, the path's state copied out at the
// kernel boundaries of every iteration (layout of a record: include/mi_pt.h, MI_PATH_RECORD_FLOATS).
int mi_pt_debug_path(mi_pt *pt, int32_t px, int32_t py, int64_t sample, int32_t max_records, float *records, int32_t *n_records) {
    if (!pt || !records || !n_records || max_records < 1) { g_err = "null argument"; return MI_ERR_INVALID; }
    *n_records = 0;
    HIPCHK(hipSetDevice(pt->device));
    ReadQueueBlocksCap(pt);
    SceneViewGuard restore{pt};
    DScene &s = pt->scene;
    if (px < s.sampleBounds[0] || px >= s.sampleBounds[2] || py < s.sampleBounds[1] || py >= s.sampleBounds[3]) { g_err = "pixel outside the sample bounds"; return MI_ERR_INVALID; }
    s.pixelBounds[0] = px; s.pixelBounds[1] = py; s.pixelBounds[2] = px + 1; s.pixelBounds[3] = py + 1;
    s.index32 = 0; s.storePixelSample = 1;
    SubRenderer &sub = pt->subs[0];
    hipStream_t st = sub.stream;
    // the pixel's tile alone: a shard of its own among as many shards as there are tiles, one sample per pixel (256 work items)
    const int tile = ((py - s.sampleBounds[1]) / 16) * TilesAlong(s, 0) + (px - s.sampleBounds[0]) / 16;
    const WorkDesc wd = PlanWork(s, tile, TilesAlong(s, 0) * TilesAlong(s, 1), 1, sample);
    const uint32_t poolN = BLOCK;
    int rc = EnsurePool(sub, poolN, QuadPlanes(s), FloatPlanes(s));
    if (rc != MI_OK) return rc;
    HIPCHK(hipMemsetAsync(sub.pool.i + (size_t)I_FLAGS * poolN, 0, (size_t)poolN * sizeof(int), st));
    HIPCHK(hipMemsetAsync(sub.ctr, 0, sizeof(DevCounters), st));
    HIPCHK(hipMemsetAsync(pt->film, 0, pt->nPix * 32 * sizeof(float), st));
    const dim3 grid(1), block(BLOCK), travGrid(1);
    const Pool &pool = sub.pool;
    std::vector<int> flags(poolN);
    auto F4 = [&](int plane, uint32_t slot, float *dst) { return hipMemcpy(dst, pool.r + pool.RecordIndex(plane, slot), 16, hipMemcpyDeviceToHost); };
    auto I1 = [&](int plane, uint32_t slot, int *dst) { return hipMemcpy(dst, pool.i + pool.ScalarIndex(plane, slot), 4, hipMemcpyDeviceToHost); };
    auto Spec = [&](int set, uint32_t slot, float *dst31) {
        float line[32];
        hipError_t e = hipMemcpy(line, pool.q + pool.QuadIndex(set, slot), 128, hipMemcpyDeviceToHost);
        memcpy(dst31, line, 31 * sizeof(float));
        return e;
    };
    int slot = -1;
    for (int it = 0; it < 4096; ++it) {
        HIPCHK(hipMemsetAsync(&sub.ctr->alive, 0, ITER_CLEAR_BYTES, st));
        hipLaunchKernelGGL(GenerateKernelOf(s), grid, block, 0, st, s, sub.pool, pt->film, sub.ctr, wd);
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(flags.data(), pool.i + (size_t)I_FLAGS * poolN, poolN * sizeof(int), hipMemcpyDeviceToHost));
        slot = -1;
        for (uint32_t k = 0; k < poolN; ++k) if (flags[k] & F_ALIVE) { slot = (int)k; break; }
        if (slot < 0) break;
        if (*n_records >= max_records) break;
        float *r = records + (size_t)(*n_records) * MI_PATH_RECORD_FLOATS;
        for (int k = 0; k < MI_PATH_RECORD_FLOATS; ++k) r[k] = 0.f;
        LaunchTraversal(pt, sub, 0, travGrid);
        LaunchResolve(pt, sub, 0, grid);
        HIPCHK(hipStreamSynchronize(st));
        int bounces = 0, prim = -1, dim = 0;
        float ray0[4], ray1[4], hit[4];
        int word0 = 0;
        HIPCHK(I1(I_FLAGS, slot, &word0)); HIPCHK(I1(I_HITPRIM, slot, &prim));
        bounces = (word0 >> BOUNCE_SHIFT) & 0xff;
        if (s.samplerType >= MI_SAMPLER_ZEROTWO) HIPCHK(I1(I_DIM, slot, &dim)); else dim = (int)((unsigned)word0 >> DIM_SHIFT);
        HIPCHK(F4(R_RAY0, slot, ray0)); HIPCHK(F4(R_RAY1, slot, ray1)); HIPCHK(F4(R_HIT, slot, hit));
        r[0] = (float)bounces; r[1] = (float)prim; r[2] = (float)dim;
        r[4] = ray0[0]; r[5] = ray0[1]; r[6] = ray0[2]; r[7] = prim >= 0 ? hit[0] : ray0[3];
        r[8] = ray1[0]; r[9] = ray1[1]; r[10] = ray1[2]; r[11] = ray1[3];
        if ((rc = LaunchShade(pt, sub, grid)) != MI_OK) return rc;
        LaunchTraversal(pt, sub, 1, travGrid);
        LaunchResolve(pt, sub, 1, grid);
        LaunchTraversal(pt, sub, 2, travGrid);
        LaunchResolve(pt, sub, 2, grid);
        if (s.misAny && (rc = LaunchDarkInLine(pt, sub, travGrid)) != MI_OK) return rc;
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipGetLastError());
        int fl = 0;
        HIPCHK(I1(I_FLAGS, slot, &fl));
        if (s.samplerType >= MI_SAMPLER_ZEROTWO) HIPCHK(I1(I_DIM, slot, &dim)); else dim = (int)((unsigned)fl >> DIM_SHIFT);
        HIPCHK(F4(R_RAY0, slot, ray0)); HIPCHK(F4(R_RAY1, slot, ray1));
        r[3] = (fl & F_ALIVE) ? 0.f : 1.f;
        r[12] = ray0[0]; r[13] = ray0[1]; r[14] = ray0[2]; r[15] = (float)dim;
        r[16] = ray1[0]; r[17] = ray1[1]; r[18] = ray1[2]; r[19] = ray1[3];
        if (fl & F_BETA_ONE) for (int k = 0; k < 31; ++k) r[20 + k] = 1.f;
        else HIPCHK(Spec(Q_BETA, slot, r + 20));
        if (!(fl & F_L_ZERO)) HIPCHK(Spec((fl & F_L_IN_B) ? Q_LB : Q_L, slot, r + 51));
        ++*n_records;
    }
    ReleasePool(sub);   // the next render sizes its own
    HIPCHK(hipMemset(pt->film, 0, pt->nPix * 32 * sizeof(float)));
    return MI_OK;
}

static int TraceRays(mi_pt *pt, const float *rays, int stride, uint32_t n, int any_hit, float *hits) {
    if (!pt || !rays || !hits) { g_err = "null argument"; return MI_ERR_INVALID; }
    if (n == 0) return MI_OK;
    return RunProbe(pt->device, rays, (size_t)n * stride * sizeof(float), hits, (size_t)n * 4 * sizeof(float), [&](void *dr, void *dh) {
        hipLaunchKernelGGL(k_trace, ProbeGrid(n), dim3(BLOCK), 0, 0, pt->scene, (float *)dr, n, any_hit, (float *)dh, stride);
    });
}

int mi_pt_trace(mi_pt *pt, const float *rays, uint32_t n, int any_hit, float *hits) { return TraceRays(pt, rays, 7, n, any_hit, hits); }
int mi_pt_trace_timed(mi_pt *pt, const float *rays, uint32_t n, int any_hit, float *hits) { return TraceRays(pt, rays, 8, n, any_hit, hits); }

static int TraceWavefront(mi_pt *pt, const float *rays, int stride, uint32_t n, int mode, float *hits, float *extra) {
    if (!pt || !rays || !hits) { g_err = "null argument"; return MI_ERR_INVALID; }
    if (mode < 0 || mode > 3) { g_err = "mi_pt_trace_wavefront: mode must be 0 (path rays), 1 (shadow rays), 2 (MIS rays) or 3 (MIS rays as visibility queries)"; return MI_ERR_INVALID; }
    if (mode == 3 && !pt->scene.misAny) { g_err = "mi_pt_trace_wavefront: mode 3 needs a scene without instances and without an alpha mask on an emitter's mesh (others keep the closest-hit form of the MIS rays)"; return MI_ERR_INVALID; }
    if (n == 0) return MI_OK;
    if (n > (1u << 24)) { g_err = "mi_pt_trace_wavefront: at most 16M rays per call"; return MI_ERR_INVALID; }
    // the kernels fix what the render fixes: a shadow ray ends at 1 - ShadowEpsilon (Interaction::SpawnRayTo), a BSDF-sampled
    // ray never ends (SpawnRay)
    for (uint32_t i = 0; i < n && mode == 3; ++i)
        if (!(rays[(size_t)i * stride + 6] > 0)) { g_err = "mi_pt_trace_wavefront: mode 3 rays carry the end of the emitter's span, tMax > 0"; return MI_ERR_INVALID; }
    for (uint32_t i = 0; i < n && (mode == 1 || mode == 2); ++i) {
        const float tMax = rays[(size_t)i * stride + 6];
        if (mode == 1 ? tMax != 1 - kShadowEpsilon : !std::isinf(tMax) || tMax < 0) {
            g_err = mode == 1 ? "mi_pt_trace_wavefront: shadow rays (mode 1) carry tMax = 1 - 0.0001f" : "mi_pt_trace_wavefront: MIS rays (mode 2) carry tMax = +infinity";
            return MI_ERR_INVALID;
        }
    }
    HIPCHK(hipSetDevice(pt->device));
    ReadQueueBlocksCap(pt);
    SubRenderer &sub = pt->subs[0];
    hipStream_t st = sub.stream;
    const DScene &s = pt->scene;
    const uint32_t poolN = (n + SLOT_CHUNKS * BLOCK - 1) / (SLOT_CHUNKS * BLOCK) * (SLOT_CHUNKS * BLOCK);
    int rc = EnsurePool(sub, poolN, QuadPlanes(s), FloatPlanes(s));
    if (rc != MI_OK) return rc;
    struct PoolGuard { SubRenderer &sub; ~PoolGuard() { ReleasePool(sub); } } guard{sub};   // the next render sizes its own
    DevBuf dr, dh, dx;
    HIPCHK(dr.alloc((size_t)n * stride * sizeof(float)));
    HIPCHK(dh.alloc((size_t)n * 4 * sizeof(float)));
    HIPCHK(dx.alloc((size_t)n * 4 * sizeof(float)));
    HIPCHK(hipMemcpy(dr.p, rays, (size_t)n * stride * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(sub.ctr, 0, sizeof(DevCounters), st));
    const dim3 grid(poolN / BLOCK), block(BLOCK);
    const dim3 chunkGrid(grid.x / SLOT_CHUNKS);
    const dim3 travGrid(std::min<unsigned>(grid.x, (unsigned)pt->numCUs * TRAV_BLOCKS_PER_CU));
    hipLaunchKernelGGL(k_trace_load, grid, block, 0, st, sub.pool, sub.ctr, dr.as<float>(), n, mode, s.motions ? s.timePlane : -1, s.camera.shutter_open, stride);
    LaunchTraversal(pt, sub, mode, travGrid, true);   // (mode 2: the closest-hit kernel, whose records this call returns)
    hipLaunchKernelGGL(k_trace_raw, grid, block, 0, st, sub.pool, n, mode, dx.as<float>());
    if (mode < 2) LaunchResolve(pt, sub, mode, mode == 0 ? chunkGrid : grid);   // (modes 2 and 3: k_trace_read resolves the hit)
    hipLaunchKernelGGL(TraceReadKernelOf(pt), grid, block, 0, st, s, sub.pool, n, mode, dh.as<float>(), dx.as<float>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(hits, dh.p, (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToHost));
    if (extra) HIPCHK(hipMemcpy(extra, dx.p, (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<DevStats> stripes(STAT_STRIPES);   // (the stack statistics of this call; the counters of the last render stay as they are)
    HIPCHK(hipMemcpy(stripes.data(), sub.ctr, sizeof(DevStats) * STAT_STRIPES, hipMemcpyDeviceToHost));
    for (SubRenderer &other : pt->subs) other.stackPushed = other.stackBeyondLds = 0;   // (the call ran on the first sub-renderer alone)
    for (const DevStats &r : stripes) { sub.stackPushed += r.stackPushed; sub.stackBeyondLds += r.stackBeyondLds; }
    return MI_OK;
}
int mi_pt_trace_wavefront(mi_pt *pt, const float *rays, uint32_t n, int mode, float *hits, float *extra) { return TraceWavefront(pt, rays, 7, n, mode, hits, extra); }
int mi_pt_trace_wavefront_timed(mi_pt *pt, const float *rays, uint32_t n, int mode, float *hits, float *extra) { return TraceWavefront(pt, rays, 8, n, mode, hits, extra); }

}  // extern "C"
