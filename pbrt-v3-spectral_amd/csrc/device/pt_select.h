// pt_select.h -- the kernels that the host units launch. Every function that names a kernel instance is defined beside the
// kernels, in MIPT_PART 0 of pt_kernels.hip (the BSDF probe's in part 4), so the instances exist there and nowhere else;
// pt_create.hip and pt_render.hip launch what these hand them.
#pragma once
#include "d_bsdf.h"
#include "pt_pool.h"

struct mi_pt;

namespace dptk {
using namespace dpt;

// The kernels that are no templates: launched by name.
__global__ void k_build_spatial(DScene s, float *func, float *cdf, float *funcInt, uint32_t nVox);
__global__ void k_pixel_tables(DScene s, float *tab1, float *tab2, unsigned long long nPix);
__global__ void k_film_split(const float *film32, float *filmSum, float *weightSum, size_t nPix);
__global__ void __launch_bounds__(BLOCK) k_trace(DScene s, const float *rays, uint32_t n, int anyHit, float *hits, int stride);
__global__ void __launch_bounds__(BLOCK) k_trace_load(Pool pool, DevCounters *ctr, const float *rays, uint32_t n, int mode, int timePlane, float time, int stride);
__global__ void __launch_bounds__(BLOCK) k_trace_raw(Pool pool, uint32_t n, int mode, float *extra);

using SceneKernel = void (*)(DScene, Pool, DevCounters *);
using GenerateKernel = void (*)(DScene, Pool, float *, DevCounters *, WorkDesc);
using OverflowKernel = void (*)(DScene, Pool, DevCounters *, int);
using MetadataKernel = void (*)(DScene, Pool, const mi_prim_meta *, int);
using TraceReadKernel = void (*)(DScene, Pool, uint32_t, int, float *, float *);

// The k_generate of a scene's camera: a uniform choice per launch.
GenerateKernel GenerateKernelOf(const DScene &s);
// The k_trav instance of ray class `mode` (0 .. 4) for the scene.
SceneKernel TravKernelOf(const mi_pt *pt, int mode);
// The resolve kernel of ray class `mode` (0: path rays, 1: shadow rays, 2: MIS rays) for the scene.
SceneKernel ResolveKernelOf(const mi_pt *pt, int mode);
// The scene's k_resolve_overflow, k_commit_metadata and k_trace_read (by its instances and their motion).
OverflowKernel OverflowKernelOf(const mi_pt *pt);
MetadataKernel MetadataCommitKernelOf(const mi_pt *pt);
TraceReadKernel TraceReadKernelOf(const mi_pt *pt);

// The k_shade instances by their index in MIPT_SHADE_INSTANCES.
struct ShadeInstance {
    int nl;
    unsigned tm;
    // [motion][lens]: [0][1] the LENS twin of an instance that reads image textures, [1][...] the MOTION twins of an instance
    // with the instance code; null: no such twin
    void (*kernel[2][2])(DScene, Pool, DevCounters *, unsigned);
};
constexpr unsigned TM_FULL = TM_ALL & ~TM_INSTANCES, TM_GENERIC = TM_FULL & ~TM_TEXTURED;
constexpr int N_SHADE_INSTANCES = 21;   // the rows of MIPT_SHADE_INSTANCES (pt_kernels.hip does not compile with another count)
const ShadeInstance &ShadeInstanceAt(int i);
int ShadeInstanceOf(unsigned types, int lobes, bool instanced, unsigned hot, bool disks, bool noise, bool projection);

// The forms of instance (nl, tm) as bits (bit f: form f of mi_pt_bsdf_probe is compiled for it), 0 for an instance without a row.
unsigned BsdfProbeForms(int nl, unsigned tm);
// Launches the probe of instance (nl, tm) on the null stream; false: no row, or a form the instance does not compile.
bool LaunchBsdfProbe(int nl, unsigned tm, const DScene &s, int material, int mode, int form, int flags, const float *dq, uint32_t n, float *dout);

}  // namespace dptk
