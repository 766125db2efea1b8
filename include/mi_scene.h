/*
 * mi_scene.h -- C ABI of the host-side .pbrt front end (libmipt_host.so).
 *
 * It stands where the reference's parse -> pbrtWorldEnd() path stands
 * (src/core/parser.cpp:1094 pbrtParseFile, src/core/api.cpp:1617 pbrtWorldEnd):
 * it reads a scene file and produces the flat mi_scene_desc (include/mi_pt.h)
 * that mi_pt_create() consumes (Camera "perspective" and, ABI v13, Camera "realistic": mi_scene_desc.camera_type and .lens
 * -- lens table, focus and exit-pupil boxes are computed here), plus the spectral ".dat" film writer
 * (src/core/film.cpp:226-308). Pure host C++; no HIP, no GPU needed.
 * Errors never abort: the reference's Error()/Warning() "report and continue"
 * policy (src/core/error.cpp:62-102) is kept; messages are retrievable below.
 */
#ifndef MI_SCENE_H
#define MI_SCENE_H
#include "mi_pt.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_scene mi_scene;

/* Values < 0 (or NULL) keep what the scene file says. crop = {x0,x1,y0,y1}. */
typedef struct mi_scene_overrides {
    int32_t spp, xres, yres, max_depth;
    float crop[4];
    const char *light_strategy;
} mi_scene_overrides;

typedef struct mi_scene_stats {
    int32_t n_triangles, n_spheres, n_meshes, interior_nodes, leaf_nodes, n_lights, n_materials;
    int32_t n_warnings, n_errors;
    int32_t accel_on_device; /* 1: the BVH was built by libmipt_hip.so's kernels (splitmethod "hlbvh" with a GPU present) */
    int32_t n_disks;
} mi_scene_stats;

int mi_scene_load_file(const char *path, const mi_scene_overrides *ov, mi_scene **out);
int mi_scene_load_string(const char *text, const char *base_dir, const mi_scene_overrides *ov, mi_scene **out);
/* A loaded scene as one binary file, for the ranks of a multi-GPU job (one process per GPU): rank 0 parses the .pbrt text
 * and builds the BVH once (the reference's single process does both once, src/core/api.cpp:1617-1737) and saves; the other
 * ranks load the arrays. Same-build, same-host hand-over, written atomically (rename); a truncated or foreign file is an
 * error code. */
int mi_scene_save_cache(const mi_scene *s, const char *path);
int mi_scene_load_cache(const char *path, mi_scene **out);
const mi_scene_desc *mi_scene_get_desc(const mi_scene *s);
void mi_scene_get_stats(const mi_scene *s, mi_scene_stats *out);
/* i-th warning (kind 0) / error (kind 1) message, NULL past the end. */
const char *mi_scene_message(const mi_scene *s, int kind, int i);
const char *mi_scene_film_filename(const mi_scene *s);
/* Integrator "metadata": the names behind the ids of the `mesh` and `material` maps.
 * mi_scene_instance_name: the object name of the i-th ObjectInstance call in file order (instance id i + 1), NULL past the end.
 * mi_scene_named_material: the i-th MakeNamedMaterial name in the order the reference iterates them (std::map order) and,
 * through *id, its material id; NULL past the end.
 * mi_scene_write_metadata_names: what the reference writes at WorldEnd beside the film file `film_filename`
 * (api.cpp:1640-1686) -- strategy `mesh`: "<stem>_mesh.txt", one line "<k> <instance name>" per instance, k from 1;
 * strategy `material`: "<stem>_materials.txt", one line "<id> <name>" per named material; other strategies and other
 * integrators: nothing. <stem> is film_filename up to its last '.'. */
const char *mi_scene_instance_name(const mi_scene *s, int i);
const char *mi_scene_named_material(const mi_scene *s, int i, uint32_t *id);
int mi_scene_write_metadata_names(const mi_scene *s, const char *film_filename);
void mi_scene_free(mi_scene *s);
const char *mi_scene_last_error(void);
/* The permutation table behind the noise textures' Noise() (MI_TEX_FBM / WRINKLED / WINDY), both halves; needs no scene. */
void mi_noise_perm(int32_t out[512]);
/* sizeof(mi_texture) of this build: a binding that mirrors the record checks its own layout against it. */
uint32_t mi_texture_struct_size(void);

/* The host BVH builders on raw bounds, as the front end runs them on a scene's primitives. prim_bounds: n x {min xyz, max xyz}
 * float32; split_method: one of MI_BVH_SPLIT_*; nodes_out: room for nodes_capacity nodes (2 n always suffices); ordered_out:
 * n primitive numbers in leaf order. MI_ERR_UNSUPPORTED (message in mi_scene_last_error) when a leaf would hold more than
 * 65535 primitives -- that many share one centre or one Morton code, and a node's count has 16 bits. */
enum { MI_BVH_SPLIT_SAH = 0, MI_BVH_SPLIT_MIDDLE = 1, MI_BVH_SPLIT_EQUAL = 2, MI_BVH_SPLIT_HLBVH = 3 };
int mi_bvh_build_host(const float *prim_bounds, uint32_t n, int32_t max_prims_in_node, int32_t split_method, mi_bvh_node *nodes_out,
                      uint32_t nodes_capacity, uint32_t *n_nodes, int32_t *ordered_out);
/* buildUpperSAH (src/accelerators/bvh.cpp:534-638) over treelet roots, with the signature of mi_bvh_upper_fn: the callback
 * the front end hands to mi_bvh_build_hlbvh (include/mi_pt.h), and the upper tree of the host HLBVH build. */
int mi_bvh_upper_sah(void *user, uint32_t n_treelets, const float *root_bounds, const int32_t *treelet_sizes, mi_bvh_node *upper_nodes,
                     int32_t *upper_index, uint32_t *n_upper, uint32_t *n_total, int32_t *treelet_offset);

/* Film::WriteImage, spectral branch: "<w> <h> 31\nv3 \n" then 31 planes of w*h
 * float64 (plane-major), values multiplied by `scale`. film_sum is [h*w*31]. */
int mi_film_write_dat(const char *filename, int w, int h, const float *film_sum, float scale);
/* Film::WriteImage, RGB branch ("bool spectralFlag" false; src/core/film.cpp:182-225 + imageio.cpp:81-119):
 * XYZ -> RGB of the summed spectrum, division by the filter-weight sum, clamp, scale. Writes PFM (.pfm),
 * TGA (.tga) or scan-line OpenEXR (.exr: HALF B, G, R, ZIP -- WriteImageEXR, imageio.cpp:163-189); any other extension
 * (PNG) is written as a .pfm beside it. weight_sum is [h*w]. */
int mi_film_write_rgb(const char *filename, int w, int h, const float *film_sum, const float *weight_sum, float scale);
/* Read one back: returns 0 and fills w,h; data (if non-NULL) receives
 * [h*w*31] floats pixel-major. */
int mi_film_read_dat(const char *filename, int *w, int *h, float *data, uint64_t capacity);

/* Integrator-shaped entry: what `integrator->Render(*scene)` (src/core/api.cpp:1707)
 * does for Integrator "path": dlopen()s libmipt_hip.so, creates the device
 * renderer, renders all tiles and writes the film file. A scene with Integrator "metadata"
 * (mi_integrator.kind) gets its name file first, then the map of the file's strategy
 * (mi_pt_render_metadata) through the same film writers. Fails loudly
 * (MI_ERR_NO_DEVICE / MI_ERR_HIP) when the HIP library or a GPU is missing --
 * there is no CPU fallback. */
int mi_integrator_render(const mi_scene *s, int device_ordinal, const char *outfile, mi_counters *counters);

#ifdef __cplusplus
}
#endif
#endif
