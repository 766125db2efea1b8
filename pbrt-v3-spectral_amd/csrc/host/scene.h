// scene.h -- the host front end's flat scene: owning storage behind the POD
// mi_scene_desc that crosses the C ABI (include/mi_pt.h). Produced by the .pbrt
// front end (parser.cpp, api.cpp, world_end.cpp) the way pbrtWorldEnd() produces Scene + Integrator in the
// reference (src/core/api.cpp:1617-1737), but as flat arrays because the
// reference's Scene/BVHAccel internals are private.
#pragma once
#include <string>
#include <vector>
#include "../../../include/mi_pt.h"
#include "paramset.h"

namespace mipt {

struct SceneStats {
    int nTriangles = 0, nSpheres = 0, nMeshes = 0, nDisks = 0;
    int interiorNodes = 0, leafNodes = 0;
    int nLights = 0, nMaterials = 0;
};

// LightSource "infinite", and the map of a LightSource "projection" (envmap.cpp)
struct HostEnvMap {
    int width = 0, height = 0, nu = 0, nv = 0;
    std::vector<float> rgb, condFunc, condCdf, condFuncInt, margFunc, margCdf;
    float margFuncInt = 0;
};

// Texture "..." "spectrum" "imagemap": one MIPMap pyramid per distinct TexInfo (imagemap.h:50-76)
struct HostMipMap {
    std::string key;           // filename + filter parameters (the reference's texture cache key)
    int width = 0, height = 0, wrap = 0;
    std::vector<float> texels; // RGB, all levels
    std::vector<uint32_t> levelOffset;
};

struct HostScene {
    // geometry
    std::vector<mi_bvh_node> nodes;
    std::vector<mi_prim> prims;  // BVH leaf order
    std::vector<int32_t> triIndices;
    std::vector<uint32_t> triMesh;
    std::vector<float> P, N, UV;
    std::vector<mi_mesh> meshes;
    std::vector<mi_sphere> spheres;
    std::vector<mi_disk> disks;   // quadric indices continue after the spheres (mi_prim.shape)
    std::vector<mi_material> materials;
    std::vector<mi_light> lights;
    std::vector<HostEnvMap> envStore;   // storage behind desc.envmaps
    std::vector<mi_envmap> envmaps;
    std::vector<HostMipMap> mipStore;   // storage behind desc.mipmaps
    std::vector<mi_mipmap> mipmaps;
    std::vector<mi_texture> textures;
    std::vector<mi_lens> lensStore;       // Camera "realistic": the one record behind desc.lens (empty for a perspective camera)
    std::vector<mi_instance> instances;   // ObjectInstance as TransformedPrimitive (their BVHs follow the world's in `nodes`)
    std::vector<mi_motion> motions;       // MIPT_OBJECT_MOTION=1: the AnimatedTransforms of the moving instances (mi_instance.motion)
    // Integrator "metadata": the ids of every primitive (parallel to prims) and the names behind them
    std::vector<mi_prim_meta> primMeta;
    std::vector<std::string> instanceNames;        // ObjectInstance calls in file order: instance id k + 1
    std::vector<std::string> namedMaterialNames;   // MakeNamedMaterial names in std::map order ...
    std::vector<uint32_t> namedMaterialIds;        // ... and their material ids
    // light distribution
    std::vector<float> ldFunc, ldCdf, ldFuncInt;
    // sampler tables
    std::vector<int32_t> primes, primeSums;
    std::vector<uint16_t> perms;
    std::vector<uint32_t> sobolMatrices;          // Sampler "sobol": the first n_sobol_dims generator matrices
    std::vector<uint64_t> sobolVdc, sobolVdcInv;  // ... and the pixel-index matrices of the film's resolution
    // output
    std::string filmFilename = "pbrt.exr";
    bool spectralFlag = true;
    bool hlbvhOnDevice = false;   // splitmethod "hlbvh": the tree came from the device build
    std::string integratorName = "path", samplerName = "halton", lightStrategy = "spatial";
    std::vector<std::string> warnings, errors;
    SceneStats stats;
    mi_scene_desc desc{};

    void Finalize();  // point desc at the vectors
};

// ---- builders (each cites the reference routine it restates)
// Loop subdivision to the limit surface, src/shapes/loopsubdiv.cpp:149-400.
bool LoopSubdivide(int nLevels, const std::vector<int> &indices, const std::vector<Vec3> &P,
                   std::vector<int> *outIndices, std::vector<Vec3> *outP, std::vector<Vec3> *outN,
                   std::string *err);

// SAH BVH2 build + depth-first flatten, src/accelerators/bvh.cpp:183-402,640-658.
struct BuildPrim { Bounds3 bounds; };
enum class SplitMethod { SAH, Middle, EqualCounts, HLBVH };
// A leaf's count is 16 bits of the node: a leaf of more than kMaxLeafPrims primitives (that many share one centre, or one
// Morton code) makes the builders return false with a message in *err and no tree (the reference CHECKs it away).
constexpr int kMaxLeafPrims = 65535;
bool BuildBVH(const std::vector<Bounds3> &primBounds, int maxPrimsInNode, SplitMethod method,
              std::vector<mi_bvh_node> *nodes, std::vector<int> *orderedPrims, int *interior,
              int *leaves, std::string *err);

// HLBVH, src/accelerators/bvh.cpp:404-638, in the order one thread builds it (bvh.cpp in this directory). The pieces are
// exposed because the device build (mi_bvh_build_hlbvh) shares the upper SAH tree and is tested against the host tree.
bool BuildHLBVH(const std::vector<Bounds3> &primBounds, int maxPrimsInNode, std::vector<mi_bvh_node> *nodes,
                std::vector<int> *orderedPrims, int *interior, int *leaves, std::string *err);
int BuildUpperSAH(uint32_t nTreelets, const float *rootBounds, const int32_t *treeletSizes, std::vector<mi_bvh_node> *upperNodes,
                  std::vector<int> *upperIndex, int32_t *treeletOffset);   // returns the total node count
// The same tree built by libmipt_hip.so's kernels (hlbvh_device.cpp). Built: the tree is there. Unavailable (with `why`): no
// library or no device, the caller builds on the host. Failed (with `why`): the device build ran and refused the input or
// met an error -- that is the scene's error, not a reason to build elsewhere.
enum class DeviceBuild { Built, Unavailable, Failed };
DeviceBuild BuildHLBVHOnDevice(const std::vector<Bounds3> &primBounds, int maxPrimsInNode, int device, std::vector<mi_bvh_node> *nodes,
                        std::vector<int> *orderedPrims, int *interior, int *leaves, double *seconds, std::string *why);

// Halton tables, src/core/lowdiscrepancy.cpp:2490-2504 (+ rng.h PCG32, sampling.h Shuffle).
void ComputeHaltonTables(int nDims, std::vector<int32_t> *primes, std::vector<int32_t> *primeSums,
                         std::vector<uint16_t> *perms);
float RadicalInverseHost(int baseIndex, uint64_t a);  // unscrambled, lowdiscrepancy.cpp:389-424
// Sobol' tables for a film whose sample bounds span `extent` pixels (sobol.h:51-62); false when the resolution is beyond the tables.
bool ComputeSobolTables(int extent, int nDims, HostScene *scene, int *resolution, int *log2Resolution);

// Camera "realistic" (realistic.cpp in this directory; src/cameras/realistic.cpp:126-187, 934-989): the element table from the
// lens file's values (4 per interface, mm), the focused film distance and the exit-pupil boxes. diagonal: Film::diagonal in
// metres. false with *err: what the reference reports as an error or CHECKs away.
bool BuildRealisticLens(std::vector<float> lensData, float apertureDiameter, float filmDistance, float focusDistance,
                        float diagonal, const int fullRes[2], mi_lens *lens, std::vector<std::string> *warnings, std::string *err);

// Light-selection distributions, src/core/lightdistrib.cpp:48-300.
void BuildLightDistribution(HostScene *scene, const std::string &strategy);

// Shape "plymesh" (plymesh.cpp)
struct PLYMeshData {
    std::vector<int> indices;
    std::vector<Vec3> P, N;
    std::vector<Vec2> UV;
};
bool ReadPLYMesh(const std::string &filename, PLYMeshData *out, std::vector<std::string> *warnings, std::string *err);

// ImageTexture<RGBSpectrum, Spectrum>::GetTexture (imagemap.cpp:58-106): read, flip, convertIn, build the pyramid.
// Returns the index into scene->mipStore (cached by TexInfo).
int BuildTextureMipMap(HostScene *scene, const std::string &filename, bool trilinear, bool noFiltering, float maxAniso,
                       int wrap, float scale, bool gamma, bool isFloat = false);
int ConstantFloatMipMap(HostScene *scene, float value);   // ConstantTexture<Float> as a 1x1 pyramid
bool BuildEnvMap(const Spectrum &L, const std::string &texmap, HostEnvMap *store, Spectrum *centre, std::vector<std::string> *errors);
// LightSource "projection": level 0 of the light's MIPMap<RGBSpectrum> (Repeat, after the power-of-two resampling) as an
// environment-map record without a distribution (nu = nv = 0), the file's own resolution (the aspect comes from it) and
// *centre = Spectrum(Lookup((.5, .5), .5f), Illuminant), the map's factor in Power(). false with *err: the file cannot be read.
bool BuildProjectionMap(const std::string &texmap, HostEnvMap *store, int *rx, int *ry, Spectrum *centre, std::string *err);
bool WriteRGBImage(const std::string &filename, int w, int h, const float *filmSum, const float *weightSum, float scale,
                   std::string *written, std::string *err);
// Material compilation (constant textures -> fixed BxDF list),
// src/materials/{matte,plastic,glass,uber,disney,mirror}.cpp.
// Returns false (and appends to errs) for materials this path does not cover.
bool CompileMixMaterial(const mi_material &m1, const mi_material &m2, const Spectrum &amount, mi_material *out,
                        std::vector<std::string> *errs);
bool CompileMaterial(const std::string &type, const TextureParams &mp, mi_material *out,
                     std::vector<std::string> *warnings, std::vector<std::string> *errs);

// .pbrt front end. Overrides < 0 / empty leave the file's values.
struct LoadOverrides {
    int spp = -1, xres = -1, yres = -1, maxDepth = -1;
    float crop[4] = {-1, -1, -1, -1};
    std::string lightStrategy;
};
HostScene *LoadSceneFile(const std::string &path, const LoadOverrides &ov, std::string *err);
HostScene *LoadSceneString(const std::string &text, const std::string &baseDir, const LoadOverrides &ov,
                           std::string *err);

// One loaded scene as a binary file (scene_cache.cpp): the hand-over between the ranks of a multi-GPU job.
bool SaveSceneCache(const HostScene &scene, const std::string &path, std::string *err);
HostScene *LoadSceneCache(const std::string &path, std::string *err);

// Spectral film writer, src/core/film.cpp:226-308 (".dat": text header + 31 planes of float64).
bool WriteSpectralDat(const std::string &filename, int w, int h, const float *filmSum, float scale,
                      std::string *err);
// The name file of an Integrator "metadata" scene beside `filmFilename` (src/core/api.cpp:1631-1686): "<stem>_mesh.txt" for
// strategy mesh, "<stem>_materials.txt" for material, nothing otherwise. *written: the file's name, "" when none was due.
bool WriteMetadataNames(const HostScene &scene, const std::string &filmFilename, std::string *written, std::string *err);

}  // namespace mipt
