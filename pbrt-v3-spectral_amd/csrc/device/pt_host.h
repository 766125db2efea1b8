// pt_host.h -- what the host code of the mi_pt_* C ABI (include/mi_pt.h) shares between its units: the renderer (mi_pt) and
// its sub-renderers, the error string, the upload and probe helpers, and the few functions one unit calls in another.
//   pt_create.hip   mi_pt_create / mi_pt_destroy and the entry points that need no GPU
//   pt_render.hip   the pool, the launches of one wavefront iteration, the render driver and the entry points that run it
//   pt_kernels.hip  the kernels, their selection (pt_select.h) and the single-question probes, each under its kernel
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "pt_select.h"

namespace dptk {
extern thread_local std::string g_err;   // mi_pt_last_error (defined in pt_create.hip)
}
using namespace dptk;

#define HIPCHK(x)                                                                         \
    do {                                                                                  \
        hipError_t e_ = (x);                                                              \
        if (e_ != hipSuccess) {                                                           \
            g_err = std::string(#x) + ": " + hipGetErrorString(e_);                       \
            return MI_ERR_HIP;                                                            \
        }                                                                                 \
    } while (0)

constexpr int N_EV = 8;   // events per iteration: kernel-class boundaries + the start of the closest-hit traversal launch
struct SubRenderer {
    Pool pool{};
    DevCounters *ctr = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t evIter[2][N_EV] = {{nullptr}};  // per-iteration kernel boundaries, two alternating sets
    double t[7] = {0};
    int poolQuadPlanes = 0;   // spectral planes the pool was allocated with (spectralpath needs one set more)
    int poolFloatPlanes = P_COUNT;   // float planes likewise (a realistic camera needs one more)
    size_t poolBytes = 0;     // bytes of device memory behind the pool
    unsigned long long iterations = 0;
    DevCounters result{};
    // what the host reads back in every iteration lands here: pinned, so the copy is one command that the device writes
    // straight to host memory (hipHostMalloc at create, freed by mi_pt_destroy)
    struct HostReads {
        DevCursor shadeCount[MAX_CLASSES];   // the shading queues' lengths after the resolve stage of the path rays (ReadShadeCounts)
        unsigned long long drawn;            // DevCounters::nextWork and alive after k_generate (round 5: pageable stack words before; the
        unsigned alive;                      // extend class, which holds this read, 0.4500 -> 0.4489 s per three killeroo frames)
    } *reads = nullptr;
    unsigned long long shadeLaunches = 0, shadeBlocks = 0;   // k_shade launches of the last render and the blocks they covered
    // The dark MIS rays of iteration i are traced beside iteration i + 1 (LaunchDarkTraversal): a stream at the lowest
    // priority, the hand-over from k_shade (evDarkGo), the kernel's own boundaries in two alternating sets (evDark) and its
    // end with the cursors cleared behind it (evDarkDone), which the next k_shade -- the next writer of darkQ and the
    // R_MI planes -- waits for.
    hipStream_t darkStream = nullptr;
    hipEvent_t evDarkGo = nullptr, evDarkDone = nullptr, evDark[2][2] = {{nullptr}};
    bool darkPending = false;            // evDarkDone has been recorded and nothing has waited for it yet
    bool darkTimed[2] = {false, false};  // evDark[k] holds a launch whose time is not in t[5] yet
    unsigned long long darkSeq = 0;      // launches on darkStream so far (picks the set)
    unsigned long long darkLaunches = 0; // k_trav<4> launches of the last render
    unsigned long long stackPushed = 0, stackBeyondLds = 0;   // mi_pt_trav_stack_stats: of the last render or mi_pt_trace_wavefront call
};

struct mi_pt {
    int device = 0;
    DScene scene{};
    std::vector<void *> allocs;   // every device buffer of create (mi_pt_destroy frees them)
    float *film = nullptr;  // [nPix][32]
    float *stageSum = nullptr, *stageW = nullptr;   // [nPix][31] / [nPix] staging of the host hand-over
    size_t nPix = 0;
    int filmW = 0, filmH = 0;
    long long spp = 0;
    std::vector<SubRenderer> subs;
    double lastSeconds[8] = {0};
    uint32_t nTextures = 0;
    std::vector<int> textureTypes;
    bool hasAlphaMasks = false;      // picks the traversal kernels compiled with the alpha-mask test
    bool hasInstances = false;       // ... and with the TransformedPrimitive code (those carry the alpha-mask test too)
    uint32_t nQuadrics = 0;          // n_spheres + n_disks (mi_pt_shape_probe)
    int samplerDims = 0;             // mi_sampler.n_dims: the dimensions the Halton tables hold (mi_pt_sampler_probe)
    std::vector<int> lightTypes;     // mi_light.type of every light (mi_pt_light_probe)
    std::vector<int> materialLobes;  // mi_material.n_bxdfs of every material, -1 - n_bxdfs for one that reads an image texture (mi_pt_bsdf_probe)
    bool hasQuadrics = false;        // the scene has spheres or disks: the quadric lists of rays can overflow (k_resolve_overflow is launched)
    bool hasInfiniteLight = false;   // picks the kernels compiled with the environment-light code
    unsigned shadeClasses[N_SHADE_INSTANCES] = {0};   // per k_shade instance: the shading classes it runs (ShadeInstanceOf)
    int numCUs = 256;
    // k_resolve_shadow and k_resolve_mis walk their queues on grids sized by what the device holds at once (QueueGrid):
    // resident blocks per CU of each, from the occupancy query at create
    int resolveBlocksPerCU[3] = {0};    // [1]: k_resolve_shadow, [2]: k_resolve_mis ([0], k_resolve_extend, walks the pool)
    unsigned queueBlocksCap = 0;        // MIPT_QUEUE_BLOCKS (tests): at most so many blocks for those kernels, 0 = unset
    bool shadeGridPool = false;         // MIPT_SHADE_GRID=pool: every k_shade instance on a pool-sized grid, no read of the class counts
    bool darkInLine = false;            // MIPT_DARK_STREAM=0: k_trav<4> on the main stream after the live MIS stage (the partner for A/B runs and tests)
    // Integrator "metadata" (mi_pt_render_metadata): the ids of the primitives as create copied them, their device copy
    // (made by the first metadata pass: a renderer that only renders radiance holds none) and, during such a pass, its
    // strategy (-1: a radiance render)
    std::vector<mi_prim_meta> primMetaHost;
    const mi_prim_meta *primMeta = nullptr;
    int metaStrategy = -1;
};

template <typename T>
int Upload(mi_pt *pt, const T *src, size_t count, const T **dst) {
    *dst = nullptr;
    if (count == 0 || !src) {
        void *p = nullptr;
        HIPCHK(hipMalloc(&p, 16));
        pt->allocs.push_back(p);
        *dst = (const T *)p;
        return MI_OK;
    }
    void *p = nullptr;
    HIPCHK(hipMalloc(&p, count * sizeof(T) + 16));   // (16 B of slack: the kernels read spectra as 16-B quads)
    pt->allocs.push_back(p);
    HIPCHK(hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
    *dst = (const T *)p;
    return MI_OK;
}

// A run of uploads that stops at the first failure: the later ones do nothing and `rc` keeps the failure's code.
struct Uploads {
    mi_pt *pt;
    int rc = MI_OK;
    template <typename T>
    void operator()(const T *src, size_t count, const T *&dst) {
        if (rc == MI_OK) rc = Upload(pt, src, count, &dst);
    }
};

// A device buffer that create fills on the device, listed in pt->allocs (freed by mi_pt_destroy) as soon as it exists.
template <typename T>
int Alloc(mi_pt *pt, size_t bytes, T **dst, const char *what) {
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();   // the failed hipMalloc must not poison the next call's hipGetLastError
        g_err = std::string("hipMalloc(") + what + ") failed";
        return MI_ERR_NOMEM;
    }
    pt->allocs.push_back(p);
    *dst = (T *)p;
    return MI_OK;
}

// Device temporaries of the entry points: freed on every return path.
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
    template <typename T> T *as() const { return (T *)p; }
};

// The body of an entry point that asks the device one batch of questions: `in` to the device, `launch(dIn, dOut)` (on the null
// stream), `out` back. The entry point has checked its arguments.
template <typename Launch>
int RunProbe(int device, const void *in, size_t inBytes, void *out, size_t outBytes, Launch launch) {
    HIPCHK(hipSetDevice(device));
    DevBuf dIn, dOut;
    HIPCHK(dIn.alloc(inBytes));
    HIPCHK(dOut.alloc(outBytes));
    HIPCHK(hipMemcpy(dIn.p, in, inBytes, hipMemcpyHostToDevice));
    launch(dIn.p, dOut.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, dOut.p, outBytes, hipMemcpyDeviceToHost));
    return MI_OK;
}
// The grid of such a launch: a thread per question.
inline dim3 ProbeGrid(uint32_t n) { return dim3((n + BLOCK - 1) / BLOCK); }

// A call that renders through a view of the scene of its own (mi_pt_render_metadata, mi_pt_debug_path) edits pt->scene in
// place behind one of these: the renderer's DScene and its metaStrategy are back on every return path.
struct SceneViewGuard {
    mi_pt *pt;
    DScene scene = pt->scene;
    int metaStrategy = pt->metaStrategy;
    ~SceneViewGuard() { pt->scene = scene; pt->metaStrategy = metaStrategy; }
};

// pt_render.hip, for pt_create.hip: the time plane of a scene with moving instances (UploadScene), a sub-renderer's pool given
// back (mi_pt_destroy), and the blocks k_shade needs for the queues of `classes` (mi_pt_shade_grid).
int TimePlaneOf(const DScene &s);
void ReleasePool(SubRenderer &sub);
unsigned long long ShadeGridBlocks(const uint32_t *counts, unsigned classes);
