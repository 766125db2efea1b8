"""pbrt-v3-spectral_amd -- MI355X-native spectral PathIntegrator hot path.

Python here is plumbing only (ctypes over the two C-ABI libraries):

* ``libmipt_host.so``  -- .pbrt front end -> flat ``mi_scene_desc`` (include/mi_scene.h)
* ``libmipt_hip.so``   -- hand-written HIP wavefront path tracer (include/mi_pt.h)

The host-side mirror of the reference's integrator surface is
:class:`PathIntegrator` with ``Render(scene)`` (reference:
``SamplerIntegrator::Render``, src/core/integrator.cpp:228-342, created by
``CreatePathIntegrator``, src/integrators/path.cpp:190-213).  There is no CPU
fallback: if the HIP library or a GPU is missing, ``PathIntegrator`` raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
NSPEC = 31
LIGHT_PROBE_SAMPLE_FLOATS = 10 + NSPEC   # MI_LIGHT_PROBE_SAMPLE_FLOATS
MAX_BXDFS = 8
PATH_RECORD_FLOATS = 96


# ----------------------------------------------------------------------------
# ctypes mirrors of include/mi_pt.h
class BvhNode(C.Structure):
    _fields_ = [("bmin", C.c_float * 3), ("bmax", C.c_float * 3), ("offset", C.c_int32),
                ("n_prims", C.c_uint16), ("axis", C.c_uint8), ("pad", C.c_uint8)]


class Prim(C.Structure):
    _fields_ = [("shape", C.c_int32), ("material", C.c_int32), ("area_light", C.c_int32), ("instance", C.c_int32)]


class Instance(C.Structure):
    _fields_ = [("i2w", C.c_float * 16), ("w2i", C.c_float * 16), ("root", C.c_uint32), ("motion", C.c_uint32),
                ("instance_id", C.c_uint32), ("pad", C.c_uint32)]


class Motion(C.Structure):
    """mi_motion: the AnimatedTransform of a moving instance (MIPT_OBJECT_MOTION=1)."""
    _fields_ = [("i2w_end", C.c_float * 16), ("w2i_end", C.c_float * 16),
                ("T", (C.c_float * 3) * 2), ("R", (C.c_float * 4) * 2), ("S", (C.c_float * 9) * 2),
                ("transform_start", C.c_float), ("transform_end", C.c_float), ("has_rotation", C.c_int32), ("pad", C.c_int32)]


class Mesh(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("first_vertex", C.c_uint32), ("n_vertices", C.c_uint32),
                ("first_tri", C.c_uint32), ("n_tris", C.c_uint32), ("alpha_tex", C.c_int32), ("shadow_alpha_tex", C.c_int32)]


class Sphere(C.Structure):
    _fields_ = [("o2w", C.c_float * 16), ("w2o", C.c_float * 16), ("radius", C.c_float), ("z_min", C.c_float),
                ("z_max", C.c_float), ("theta_min", C.c_float), ("theta_max", C.c_float), ("phi_max", C.c_float),
                ("reverse_orientation", C.c_int32), ("swaps_handedness", C.c_int32)]


class Disk(C.Structure):
    _fields_ = [("o2w", C.c_float * 16), ("w2o", C.c_float * 16), ("height", C.c_float), ("radius", C.c_float),
                ("inner_radius", C.c_float), ("phi_max", C.c_float), ("reverse_orientation", C.c_int32),
                ("swaps_handedness", C.c_int32), ("kind", C.c_int32), ("pad", C.c_int32)]


class Bxdf(C.Structure):
    _fields_ = [("type", C.c_int32), ("flags", C.c_int32), ("fresnel", C.c_int32), ("scaled", C.c_int32),
                ("p", C.c_float * 8), ("R", C.c_float * NSPEC), ("S", C.c_float * NSPEC),
                ("K", C.c_float * NSPEC), ("scale", C.c_float * NSPEC), ("scale2", C.c_float * NSPEC)]


class LobeTex(C.Structure):
    _fields_ = [("tex_R", C.c_int32), ("tex_S", C.c_int32), ("flags", C.c_uint32), ("rule", C.c_int32)]


class Material(C.Structure):
    _fields_ = [("n_bxdfs", C.c_int32), ("eta", C.c_float), ("kind", C.c_int32), ("textured", C.c_int32),
                ("bxdf", Bxdf * MAX_BXDFS), ("tex", LobeTex * MAX_BXDFS), ("bump_tex", C.c_int32), ("rough_tex", C.c_int32 * 2), ("rough_flags", C.c_uint32), ("sigma_tex", C.c_int32)]


MAX_MIP_LEVELS = 16


class MipMap(C.Structure):
    _fields_ = [("n_levels", C.c_int32), ("wrap", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("texels", C.POINTER(C.c_float)), ("level_offset", C.c_uint32 * MAX_MIP_LEVELS)]


class Texture(C.Structure):
    _fields_ = [("mipmap", C.c_int32), ("filter", C.c_int32), ("max_aniso", C.c_float),
                ("su", C.c_float), ("sv", C.c_float), ("du", C.c_float), ("dv", C.c_float), ("post_scale", C.c_float),
                ("type", C.c_int32), ("aa_none", C.c_int32), ("spec1", C.c_float * NSPEC), ("spec2", C.c_float * NSPEC),
                ("octaves", C.c_int32), ("omega", C.c_float), ("w2t", C.c_float * 16),
                # the opt-in mappings and classes (MIPT_TEXTURES=all)
                ("is_float", C.c_int32), ("mapping", C.c_int32), ("vs", C.c_float * 3), ("vt", C.c_float * 3), ("bilerp", C.c_float * 4)]


TEX_IMAGEMAP, TEX_CHECKERBOARD, TEX_FBM, TEX_WRINKLED, TEX_WINDY, TEX_DOTS, TEX_UV, TEX_BILERP, TEX_CHECKERBOARD3D = range(9)   # mi_tex_type
MAP_UV, MAP_SPHERICAL, MAP_CYLINDRICAL, MAP_PLANAR = range(4)   # mi_tex_mapping


class Light(C.Structure):
    _fields_ = [("type", C.c_int32), ("shape", C.c_int32), ("two_sided", C.c_int32), ("area", C.c_float),
                ("L", C.c_float * NSPEC), ("pos", C.c_float * 3), ("dir", C.c_float * 3),
                ("world_radius", C.c_float), ("world_center", C.c_float * 3), ("envmap", C.c_int32),
                ("l2w", C.c_float * 9), ("w2l", C.c_float * 9), ("cos_total_width", C.c_float), ("cos_falloff_start", C.c_float),
                # the projection light (LIGHT_PROJECTION): screen bounds, lightProjection, hither, the map (-1: none), Power()'s map factor
                ("screen", C.c_float * 4), ("proj", C.c_float * 16), ("hither", C.c_float), ("proj_map", C.c_int32),
                ("proj_centre", C.c_float * NSPEC)]


LIGHT_PROJECTION = 5   # MI_LIGHT_PROJECTION: the light type that has no bit in the k_shade masks (LIGHT_TYPES names those)


class EnvMap(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rgb", C.POINTER(C.c_float)), ("nu", C.c_int32), ("nv", C.c_int32),
                ("cond_func", C.POINTER(C.c_float)), ("cond_cdf", C.POINTER(C.c_float)), ("cond_func_int", C.POINTER(C.c_float)),
                ("marg_func", C.POINTER(C.c_float)), ("marg_cdf", C.POINTER(C.c_float)), ("marg_func_int", C.c_float)]


class LightDistrib(C.Structure):
    _fields_ = [("type", C.c_int32), ("n_voxels", C.c_int32 * 3), ("n_distributions", C.c_uint32),
                ("func", C.POINTER(C.c_float)), ("cdf", C.POINTER(C.c_float)), ("func_int", C.POINTER(C.c_float))]


MAX_LENS_ELEMENTS = 32
EXIT_PUPIL_BOUNDS = 64
CAMERA_PERSPECTIVE, CAMERA_REALISTIC, CAMERA_ORTHOGRAPHIC, CAMERA_ENVIRONMENT = 0, 1, 2, 3


class Lens(C.Structure):
    """mi_lens: Camera "realistic" -- elements[i] = (curvature radius, thickness, eta, aperture radius) in metres, front first."""
    _fields_ = [("n_elements", C.c_int32), ("simple_weighting", C.c_int32), ("no_weighting", C.c_int32),
                ("chromatic_aberration", C.c_int32), ("full_res", C.c_int32 * 2), ("film_distance", C.c_float), ("film_diagonal", C.c_float),
                ("thick_lens_pz", C.c_float * 2), ("thick_lens_fz", C.c_float * 2),
                ("physical_extent", C.c_float * 4), ("elements", (C.c_float * 4) * MAX_LENS_ELEMENTS),
                ("exit_pupil_bounds", (C.c_float * 4) * EXIT_PUPIL_BOUNDS)]


class Camera(C.Structure):
    _fields_ = [("raster_to_camera", C.c_float * 16), ("camera_to_world", C.c_float * 16),
                ("lens_radius", C.c_float), ("focal_distance", C.c_float), ("shutter_open", C.c_float),
                ("shutter_close", C.c_float),
                ("camera_to_world_end", C.c_float * 16), ("transform_start", C.c_float), ("transform_end", C.c_float),
                ("animated", C.c_int32), ("T", (C.c_float * 3) * 2), ("R", (C.c_float * 4) * 2), ("S", (C.c_float * 9) * 2)]


class Film(C.Structure):
    _fields_ = [("full_res", C.c_int32 * 2), ("cropped_bounds", C.c_int32 * 4), ("sample_bounds", C.c_int32 * 4),
                ("filter_radius", C.c_float * 2), ("filter_table", C.c_float * 256), ("scale", C.c_float),
                ("max_sample_luminance", C.c_float)]


class Sampler(C.Structure):
    _fields_ = [("samples_per_pixel", C.c_int64), ("base_scales", C.c_int32 * 2), ("base_exponents", C.c_int32 * 2),
                ("sample_stride", C.c_int32), ("mult_inverse", C.c_int32 * 2), ("sample_at_pixel_center", C.c_int32),
                ("n_dims", C.c_int32), ("primes", C.POINTER(C.c_int32)), ("prime_sums", C.POINTER(C.c_int32)),
                ("perms", C.POINTER(C.c_uint16)), ("n_perms", C.c_uint32),
                ("type", C.c_int32), ("sobol_resolution", C.c_int32), ("sobol_log2_resolution", C.c_int32),
                ("n_sobol_dims", C.c_int32), ("sobol_matrices", C.POINTER(C.c_uint32)),
                ("sobol_vdc", C.POINTER(C.c_uint64)), ("sobol_vdc_inv", C.POINTER(C.c_uint64)),
                ("pixel_dims", C.c_int32), ("x_samples", C.c_int32), ("y_samples", C.c_int32), ("jitter", C.c_int32)]


class Integrator(C.Structure):
    _fields_ = [("max_depth", C.c_int32), ("rr_threshold", C.c_float), ("pixel_bounds", C.c_int32 * 4),
                ("n_ca_bands", C.c_int32), ("kind", C.c_int32), ("metadata_strategy", C.c_int32)]


class PrimMeta(C.Structure):
    _fields_ = [("material_id", C.c_uint32), ("instance_id", C.c_uint32)]


class SceneDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32),
                ("n_nodes", C.c_uint32), ("nodes", C.POINTER(BvhNode)),
                ("n_prims", C.c_uint32), ("prims", C.POINTER(Prim)),
                ("n_tris", C.c_uint32), ("tri_indices", C.POINTER(C.c_int32)), ("tri_mesh", C.POINTER(C.c_uint32)),
                ("n_verts", C.c_uint32), ("P", C.POINTER(C.c_float)), ("N", C.POINTER(C.c_float)),
                ("UV", C.POINTER(C.c_float)),
                ("n_meshes", C.c_uint32), ("meshes", C.POINTER(Mesh)),
                ("n_spheres", C.c_uint32), ("spheres", C.POINTER(Sphere)),
                ("n_materials", C.c_uint32), ("materials", C.POINTER(Material)),
                ("n_lights", C.c_uint32), ("lights", C.POINTER(Light)),
                ("light_distrib", LightDistrib), ("camera", Camera), ("film", Film), ("sampler", Sampler),
                ("integrator", Integrator), ("cie_y", C.c_float * NSPEC),
                ("n_envmaps", C.c_uint32), ("envmaps", C.POINTER(EnvMap)), ("rgb_illum", (C.c_float * NSPEC) * 7),
                ("n_textures", C.c_uint32), ("textures", C.POINTER(Texture)),
                ("n_mipmaps", C.c_uint32), ("mipmaps", C.POINTER(MipMap)),
                ("n_instances", C.c_uint32), ("instances", C.POINTER(Instance)),
                ("prim_meta", C.POINTER(PrimMeta)),
                ("camera_type", C.c_int32), ("lens", C.POINTER(Lens)),
                ("n_disks", C.c_uint32), ("disks", C.POINTER(Disk)),
                ("n_motions", C.c_uint32), ("motions", C.POINTER(Motion)),
                # Camera "environment" (MIPT_CAMERAS=all): the omnistereo parameters
                ("env_ipd", C.c_float), ("env_pole_merge_to", C.c_float), ("env_pole_merge_from", C.c_float),
                ("env_convergence_distance", C.c_float)]


class Counters(C.Structure):
    _fields_ = [("camera_rays", C.c_uint64), ("regular_rays", C.c_uint64), ("shadow_rays", C.c_uint64),
                ("total_paths", C.c_uint64), ("zero_radiance_paths", C.c_uint64), ("path_length_sum", C.c_uint64),
                ("bvh_nodes_visited", C.c_uint64), ("tri_tests", C.c_uint64), ("bad_samples", C.c_uint64),
                ("iterations", C.c_uint64), ("extend_rays", C.c_uint64), ("extend_nodes", C.c_uint64),
                ("extend_tri_tests", C.c_uint64), ("launches", C.c_uint64 * 3)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_ if n != "launches"}


class RenderParams(C.Structure):
    _fields_ = [("shard_index", C.c_int32), ("shard_count", C.c_int32), ("flags", C.c_uint32),
                ("path_pool", C.c_uint32), ("spp_override", C.c_int64), ("sample_begin", C.c_int64),
                ("stream", C.c_void_p)]


class SceneOverrides(C.Structure):
    _fields_ = [("spp", C.c_int32), ("xres", C.c_int32), ("yres", C.c_int32), ("max_depth", C.c_int32),
                ("crop", C.c_float * 4), ("light_strategy", C.c_char_p)]


class SceneStats(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_triangles", "n_spheres", "n_meshes", "interior_nodes", "leaf_nodes",
                                          "n_lights", "n_materials", "n_warnings", "n_errors", "accel_on_device",
                                          "n_disks")]


INTEGRATOR_PATH, INTEGRATOR_METADATA = 0, 1
METADATA_STRATEGIES = ("depth", "material", "mesh", "coordinates")   # mi_metadata_strategy 0..3

RENDER_FILM_ON_DEVICE = 1
RENDER_ACCUMULATE = 2

HOST_LIB = os.path.join(_HERE, "libmipt_host.so")
HIP_LIB = os.environ.get("MIPT_HIP_LIB") or os.path.join(_HERE, "libmipt_hip.so")   # override: kernel tuning builds

_host = None
_hip = None


def host_lib():
    """The .pbrt front-end library (pure host C++)."""
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB):
            raise RuntimeError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % HOST_LIB)
        lib = C.CDLL(HOST_LIB)
        lib.mi_scene_load_file.argtypes = [C.c_char_p, C.POINTER(SceneOverrides), C.POINTER(C.c_void_p)]
        lib.mi_scene_load_string.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(SceneOverrides), C.POINTER(C.c_void_p)]
        lib.mi_scene_save_cache.argtypes = [C.c_void_p, C.c_char_p]
        lib.mi_scene_load_cache.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        lib.mi_scene_get_desc.argtypes = [C.c_void_p]
        lib.mi_scene_get_desc.restype = C.POINTER(SceneDesc)
        lib.mi_scene_get_stats.argtypes = [C.c_void_p, C.POINTER(SceneStats)]
        lib.mi_scene_message.argtypes = [C.c_void_p, C.c_int, C.c_int]
        lib.mi_scene_message.restype = C.c_char_p
        lib.mi_scene_film_filename.argtypes = [C.c_void_p]
        lib.mi_scene_film_filename.restype = C.c_char_p
        lib.mi_scene_instance_name.argtypes = [C.c_void_p, C.c_int]
        lib.mi_scene_instance_name.restype = C.c_char_p
        lib.mi_scene_named_material.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint32)]
        lib.mi_scene_named_material.restype = C.c_char_p
        lib.mi_scene_write_metadata_names.argtypes = [C.c_void_p, C.c_char_p]
        lib.mi_scene_free.argtypes = [C.c_void_p]
        lib.mi_scene_last_error.restype = C.c_char_p
        lib.mi_noise_perm.argtypes = [C.POINTER(C.c_int32)]
        lib.mi_noise_perm.restype = None
        lib.mi_texture_struct_size.argtypes = []
        lib.mi_texture_struct_size.restype = C.c_uint32
        lib.mi_film_write_dat.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_float]
        lib.mi_film_read_dat.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float),
                                         C.c_uint64]
        lib.mi_integrator_render.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.POINTER(Counters)]
        _host = lib
    return _host


def _start_torch_runtime_first():
    """A process that uses torch beside this package (distributed.device_film_tensor, bench.py) runs two copies of the HIP
    runtime: the one torch ships and the one libmipt_hip.so links. They share the GPU when torch's comes up first; in the other
    order torch later finds no device ("No HIP GPUs are available"), whenever that later is -- so the order cannot be left to
    the caller. Where torch is installed, its runtime is started before the library is loaded; without torch the package
    works as before, less the torch hand-overs."""
    try:
        import torch
        if torch.cuda.is_available() and torch.cuda.device_count() > 0:
            torch.cuda.init()
    except Exception:   # (no torch, or one without a usable GPU build: nothing to start, nothing here depends on it)
        pass


def hip_lib():
    """The HIP path (hand-written gfx950 kernels). Raises if it is not built / loadable."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_LIB):
            raise RuntimeError("HIP extension %s is missing; the product path has no CPU fallback" % HIP_LIB)
        _start_torch_runtime_first()
        lib = C.CDLL(HIP_LIB)
        lib.mi_pt_create.argtypes = [C.POINTER(SceneDesc), C.c_int, C.POINTER(C.c_void_p)]
        lib.mi_pt_render.argtypes = [C.c_void_p, C.POINTER(RenderParams), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                     C.POINTER(Counters)]
        lib.mi_pt_render_metadata.argtypes = [C.c_void_p, C.POINTER(RenderParams), C.c_int, C.POINTER(C.c_float),
                                              C.POINTER(C.c_float), C.POINTER(Counters)]
        lib.mi_pt_device_film.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        lib.mi_pt_last_timings.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int]
        lib.mi_pt_pool_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        lib.mi_pt_destroy.argtypes = [C.c_void_p]
        lib.mi_pt_last_error.restype = C.c_char_p
        lib.mi_pt_trace.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.c_int, C.POINTER(C.c_float)]
        lib.mi_pt_camera_rays.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_float)]
        lib.mi_pt_camera_rays_ex.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_uint32, C.c_int32, C.POINTER(C.c_float)]
        lib.mi_pt_math_probe.argtypes = [C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        lib.mi_pt_trace_wavefront.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_uint32, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        lib.mi_pt_trace_timed.argtypes = lib.mi_pt_trace.argtypes
        lib.mi_pt_trace_wavefront_timed.argtypes = lib.mi_pt_trace_wavefront.argtypes
        lib.mi_pt_texture_lookup.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        lib.mi_pt_shape_probe.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        lib.mi_pt_texture_probe.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        lib.mi_pt_light_probe.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        if hasattr(lib, "mi_pt_texture_eval_probe"):   # (as below)
            lib.mi_pt_texture_eval_probe.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        if hasattr(lib, "mi_pt_bsdf_probe"):   # (as below: a parent's library behind MIPT_HIP_LIB has none)
            lib.mi_pt_bsdf_probe.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
            lib.mi_pt_bsdf_probe_forms.argtypes = [C.c_int32, C.POINTER(C.c_uint32)]
        if hasattr(lib, "mi_pt_sampler_probe"):   # (as above)
            lib.mi_pt_sampler_probe.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_float)]
        lib.mi_pt_light_distribution.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint64]
        lib.mi_pt_debug_path.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
        lib.mi_pt_shade_instances.argtypes = [C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
        lib.mi_pt_shade_mask.argtypes = [C.c_char_p, C.POINTER(C.c_uint32)]
        if hasattr(lib, "mi_pt_shade_grid"):   # (an older build behind MIPT_HIP_LIB still renders: A/Bs against a parent's library)
            lib.mi_pt_shade_grid.argtypes = [C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)]
            lib.mi_pt_shade_launch_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        if hasattr(lib, "mi_pt_dark_launch_stats"):
            lib.mi_pt_dark_launch_stats.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint64)] * 4
        if hasattr(lib, "mi_pt_trav_stack_stats"):
            lib.mi_pt_trav_stack_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        lib.mi_pt_shade_plan.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_uint32,
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        _hip = lib
    return _hip


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _check(rc, name):
    """The return code of the HIP library's entry point `name`: RuntimeError with the library's message unless it is MI_OK."""
    if rc != 0:
        raise RuntimeError("%s failed: %s" % (name, hip_lib().mi_pt_last_error().decode()))


class Scene:
    """A parsed .pbrt scene flattened to ``mi_scene_desc`` (reference: pbrtParseFile +
    pbrtWorldEnd up to, not including, ``integrator->Render``; src/core/api.cpp:1617-1707)."""

    def __init__(self, path=None, text=None, base_dir=None, spp=-1, xres=-1, yres=-1, max_depth=-1, crop=None,
                 light_strategy=None, cache=None):
        lib = host_lib()
        if cache is not None:   # a scene another process loaded and saved (Scene.save_cache): no parsing, no BVH build
            h = C.c_void_p()
            if lib.mi_scene_load_cache(os.fsencode(cache), C.byref(h)) != 0:
                raise RuntimeError("scene cache load failed: %s" % lib.mi_scene_last_error().decode())
            self._h = h
            self.desc_ptr = lib.mi_scene_get_desc(h)
            self.desc = self.desc_ptr.contents
            return
        ov = SceneOverrides(spp, xres, yres, max_depth, (C.c_float * 4)(*(crop or (-1, -1, -1, -1))),
                            light_strategy.encode() if light_strategy else None)
        h = C.c_void_p()
        if path is not None:
            rc = lib.mi_scene_load_file(os.fsencode(path), C.byref(ov), C.byref(h))
        else:
            rc = lib.mi_scene_load_string(text.encode(), os.fsencode(base_dir or "."), C.byref(ov), C.byref(h))
        if rc != 0:
            raise RuntimeError("scene load failed: %s" % lib.mi_scene_last_error().decode())
        self._h = h
        self.desc_ptr = lib.mi_scene_get_desc(h)
        self.desc = self.desc_ptr.contents

    def save_cache(self, path):
        """Write the loaded scene (arrays, BVH, tables) as one binary file for the other ranks of a job (Scene(cache=path))."""
        if host_lib().mi_scene_save_cache(self._h, os.fsencode(path)) != 0:
            raise RuntimeError("scene cache save failed: %s" % host_lib().mi_scene_last_error().decode())

    def close(self):
        if getattr(self, "_h", None):
            host_lib().mi_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stats(self):
        st = SceneStats()
        host_lib().mi_scene_get_stats(self._h, C.byref(st))
        return {n: getattr(st, n) for n, _ in SceneStats._fields_}

    def messages(self, kind):
        out, i = [], 0
        while True:
            m = host_lib().mi_scene_message(self._h, kind, i)
            if m is None:
                return out
            out.append(m.decode())
            i += 1

    warnings = property(lambda self: self.messages(0))
    errors = property(lambda self: self.messages(1))

    @property
    def film_filename(self):
        return host_lib().mi_scene_film_filename(self._h).decode()

    @property
    def instance_names(self):
        """Object names of the ObjectInstance calls in file order: the `mesh` map's id k + 1 is instance_names[k]."""
        out = []
        while True:
            m = host_lib().mi_scene_instance_name(self._h, len(out))
            if m is None:
                return out
            out.append(m.decode())

    @property
    def named_material_ids(self):
        """[(name, material id)] of the MakeNamedMaterial names, in the order the reference lists them (sorted by name)."""
        out = []
        while True:
            mid = C.c_uint32()
            m = host_lib().mi_scene_named_material(self._h, len(out), C.byref(mid))
            if m is None:
                return out
            out.append((m.decode(), int(mid.value)))

    def write_metadata_names(self, film_filename):
        """The name file the reference writes beside the film of an Integrator "metadata" scene: <stem>_mesh.txt (strategy
        mesh) or <stem>_materials.txt (strategy material); nothing for the other strategies (mi_scene_write_metadata_names)."""
        if host_lib().mi_scene_write_metadata_names(self._h, os.fsencode(film_filename)) != 0:
            raise RuntimeError("metadata name file: %s" % host_lib().mi_scene_last_error().decode())

    @property
    def film_size(self):
        cb = self.desc.film.cropped_bounds
        return cb[2] - cb[0], cb[3] - cb[1]

    @property
    def spp(self):
        return int(self.desc.sampler.samples_per_pixel)

    def shade_plan(self):
        """The shading plan mi_pt_create would make of this scene (mi_pt_shade_plan; host code of the HIP library, no device):
        {"material_class": [class of material i], "classes": {class: {"instance", "nl", "tm", "lobes", "types"}} for the
        classes in use (MISS_CLASS, the escaped rays', among them; instance indexes shade_instances(), whose (nl, tm) is
        repeated here), "hot": the light and sampler bits of the scene's matte and plastic instances}."""
        lib = hip_lib()
        n_mat = int(self.desc.n_materials)
        mat = (C.c_int32 * max(1, n_mat))()
        cid, cinst, clobes = (C.c_int32 * MAX_CLASSES)(), (C.c_int32 * MAX_CLASSES)(), (C.c_int32 * MAX_CLASSES)()
        ctypes_ = (C.c_uint32 * MAX_CLASSES)()
        n, hot = C.c_uint32(), C.c_uint32()
        rc = lib.mi_pt_shade_plan(self.desc_ptr, mat, n_mat, cid, cinst, clobes, ctypes_, MAX_CLASSES, C.byref(n), C.byref(hot))
        if rc != 0:
            raise RuntimeError("mi_pt_shade_plan failed (%d): %s" % (rc, lib.mi_pt_last_error().decode()))
        table = shade_instances()
        classes = {}
        for k in range(n.value):
            i = int(cinst[k])
            nl, tm = table[i] if 0 <= i < len(table) else (None, None)
            classes[int(cid[k])] = {"instance": i, "nl": nl, "tm": tm, "lobes": int(clobes[k]), "types": int(ctypes_[k])}
        return {"material_class": [int(mat[i]) for i in range(n_mat)], "classes": classes, "hot": int(hot.value)}


class PathIntegrator:
    """Host mirror of ``PathIntegrator`` for ``Integrator "path"``: ``Render(scene)`` runs
    the HIP wavefront pipeline through the C ABI and returns the spectral film sums."""

    def __init__(self, scene, device=0):
        lib = hip_lib()
        self.scene = scene
        h = C.c_void_p()
        rc = lib.mi_pt_create(scene.desc_ptr, device, C.byref(h))
        if rc != 0:
            raise RuntimeError("mi_pt_create failed (%d): %s" % (rc, lib.mi_pt_last_error().decode()))
        self._h = h
        self.counters = Counters()

    def close(self):
        if getattr(self, "_h", None):
            hip_lib().mi_pt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def Render(self, shard_index=0, shard_count=1, spp=0, path_pool=0, download=True, accumulate=False,
               sample_begin=0, film_out=None, weight_out=None):
        """Render sample numbers [sample_begin, sample_begin+spp) of this shard's tiles.
        film_out / weight_out: optional device pointers (ints) that receive the film sums
        (e.g. torch CUDA tensors' data_ptr()) instead of a host download."""
        return self._render(None, shard_index, shard_count, spp, path_pool, download, accumulate, sample_begin, film_out,
                            weight_out)

    def RenderMetadata(self, strategy, shard_index=0, shard_count=1, spp=0, path_pool=0, download=True, accumulate=False,
                       sample_begin=0, film_out=None, weight_out=None):
        """One map of Integrator "metadata" on this renderer's uploaded scene (mi_pt_render_metadata): `strategy` is
        "depth", "material", "mesh" or "coordinates" (or its number). The other arguments and the returned film sums are
        Render()'s; metadata_image() turns them into the map."""
        return self._render(_strategy_number(strategy), shard_index, shard_count, spp, path_pool, download, accumulate,
                            sample_begin, film_out, weight_out)

    def _render(self, strategy, shard_index, shard_count, spp, path_pool, download, accumulate, sample_begin, film_out,
                weight_out):
        lib = hip_lib()

        def call(rp, film, weight):
            if strategy is None:
                name, rc = "mi_pt_render", lib.mi_pt_render(self._h, C.byref(rp), film, weight, C.byref(self.counters))
            else:
                name, rc = "mi_pt_render_metadata", lib.mi_pt_render_metadata(self._h, C.byref(rp), strategy, film, weight,
                                                                             C.byref(self.counters))
            if rc != 0:
                raise RuntimeError("%s failed (%d): %s" % (name, rc, lib.mi_pt_last_error().decode()))

        if film_out is not None:
            rp = RenderParams(shard_index, shard_count, (RENDER_ACCUMULATE if accumulate else 0) | RENDER_FILM_ON_DEVICE,
                              path_pool, spp, sample_begin, None)
            call(rp, C.cast(film_out, C.POINTER(C.c_float)), C.cast(weight_out, C.POINTER(C.c_float)) if weight_out else None)
            return None, None
        w, h = self.scene.film_size
        film = np.zeros((h, w, NSPEC), np.float32) if download else None
        weight = np.zeros((h, w), np.float32) if download else None
        rp = RenderParams(shard_index, shard_count, RENDER_ACCUMULATE if accumulate else 0, path_pool, spp,
                          sample_begin, None)
        call(rp, _fptr(film) if download else None, _fptr(weight) if download else None)
        return film, weight

    def timings(self):
        t = (C.c_double * 8)()
        hip_lib().mi_pt_last_timings(self._h, t, 8)
        return list(t)

    def pool_info(self):
        """(slots, bytes) of the path pool the last render ran on (mi_pt_pool_info)."""
        n, b = C.c_uint64(), C.c_uint64()
        hip_lib().mi_pt_pool_info(self._h, C.byref(n), C.byref(b))
        return int(n.value), int(b.value)

    def shade_launch_stats(self):
        """(launches, blocks) of k_shade in the last render, summed over the sub-renderers (mi_pt_shade_launch_stats)."""
        n, b = C.c_uint64(), C.c_uint64()
        _check(hip_lib().mi_pt_shade_launch_stats(self._h, C.byref(n), C.byref(b)), "mi_pt_shade_launch_stats")
        return int(n.value), int(b.value)

    def dark_launch_stats(self):
        """(launches, entries, rays, resolve_skipped) of the dark MIS rays in the last render (mi_pt_dark_launch_stats)."""
        v = [C.c_uint64() for _ in range(4)]
        _check(hip_lib().mi_pt_dark_launch_stats(self._h, *[C.byref(x) for x in v]), "mi_pt_dark_launch_stats")
        return tuple(int(x.value) for x in v)

    def device_film(self):
        p = C.c_void_p()
        n = C.c_uint64()
        hip_lib().mi_pt_device_film(self._h, C.byref(p), C.byref(n))
        return p.value, int(n.value)

    def trace(self, rays, any_hit=False):
        """rays [n, 7] = o, d, tMax, or [n, 8] with each ray's time in the eighth column (it decides the transform of a
        moving instance; without it a ray takes the shutter-open time)."""
        rays = np.ascontiguousarray(rays, np.float32)
        n = rays.shape[0]
        hits = np.zeros((n, 4), np.float32)
        fn = hip_lib().mi_pt_trace_timed if rays.shape[1] == 8 else hip_lib().mi_pt_trace
        _check(fn(self._h, _fptr(rays), n, 1 if any_hit else 0, _fptr(hits)), "mi_pt_trace")
        return hits

    def camera_rays(self, samples):
        """The camera rays k_generate would make (mi_pt_camera_rays): samples [n, 3] = (px, py, sample number) ->
        [n, 8] = o, d, tMax, time."""
        s = np.ascontiguousarray(samples, np.int32).reshape(-1, 3)
        out = np.zeros((s.shape[0], 8), np.float32)
        _check(hip_lib().mi_pt_camera_rays(self._h, s.ctypes.data_as(C.POINTER(C.c_int32)), s.shape[0], _fptr(out)), "mi_pt_camera_rays")
        return out

    def camera_rays_ex(self, samples, band=0):
        """camera_rays for every camera, with what a realistic camera adds (mi_pt_camera_rays_ex): samples [n, 3] ->
        [n, 21] = o, d, tMax, time, weight, rxOrigin, ryOrigin, rxDirection, ryDirection (the differentials scaled by
        1 / sqrt(spp)); `band`: the "spectralpath" band whose wavelength the lens is traced at."""
        s = np.ascontiguousarray(samples, np.int32).reshape(-1, 3)
        out = np.zeros((s.shape[0], 21), np.float32)
        _check(hip_lib().mi_pt_camera_rays_ex(self._h, s.ctypes.data_as(C.POINTER(C.c_int32)), s.shape[0], int(band), _fptr(out)), "mi_pt_camera_rays_ex")
        return out

    def trace_wavefront(self, rays, mode=0):
        """The rays through the render's own kernels (mi_pt_trace_wavefront): mode 0 path rays (k_trav<0> + resolve),
        1 shadow rays (tMax = 1 - 0.0001f), 2 MIS rays (tMax = inf), 3 MIS rays as visibility queries (tMax = the end of the
        emitter's span; prim = an occluder, -1 or -2 = ambiguous). Returns (hits [n, 4] as trace(), extra [n, 4] int32 view:
        b2 bits, hit instance, raw I_NPEND, raw I_HITPRIM)."""
        rays = np.ascontiguousarray(rays, np.float32)
        n = rays.shape[0]
        hits = np.zeros((n, 4), np.float32)
        extra = np.zeros((n, 4), np.float32)
        fn = hip_lib().mi_pt_trace_wavefront_timed if rays.shape[1] == 8 else hip_lib().mi_pt_trace_wavefront   # (rays [n, 8]: a time per ray)
        _check(fn(self._h, _fptr(rays), n, int(mode), _fptr(hits), _fptr(extra)), "mi_pt_trace_wavefront")
        return hits, extra.view(np.int32)

    def trav_stack_stats(self):
        """(pushed, beyond_lds) of the traversal stacks in the last render or trace_wavefront call (mi_pt_trav_stack_stats):
        the entries k_trav pushed in all, and those of them that went past the stack's LDS part into private memory."""
        v = (C.c_uint64 * 2)()
        _check(hip_lib().mi_pt_trav_stack_stats(self._h, v), "mi_pt_trav_stack_stats")
        return int(v[0]), int(v[1])

    def light_distribution(self):
        """The spatial light-selection tables built at create: (func [nz, ny, nx, n_lights], funcInt [nz, ny, nx])."""
        d = self.scene.desc
        nx, ny, nz = [int(v) for v in d.light_distrib.n_voxels]
        func = np.zeros((nz, ny, nx, d.n_lights), np.float32)
        fint = np.zeros((nz, ny, nx), np.float32)
        _check(hip_lib().mi_pt_light_distribution(self._h, _fptr(func), _fptr(fint), nx * ny * nz), "mi_pt_light_distribution")
        return func, fint

    def debug_path(self, px, py, sample, max_records=64):
        """Vertex-by-vertex state of one camera sample (records of PATH_RECORD_FLOATS floats, include/mi_pt.h)."""
        rec = np.zeros((max_records, PATH_RECORD_FLOATS), np.float32)
        n = C.c_int32()
        _check(hip_lib().mi_pt_debug_path(self._h, int(px), int(py), int(sample), max_records, _fptr(rec), C.byref(n)), "mi_pt_debug_path")
        return rec[: n.value]

    def texture_lookup(self, tex, queries):
        """MIPMap::Lookup on the device: queries [n, 6] = (s, t, dsdx, dtdx, dsdy, dtdy) -> rgb [n, 3]."""
        q = np.ascontiguousarray(queries, np.float32)
        out = np.zeros((q.shape[0], 3), np.float32)
        _check(hip_lib().mi_pt_texture_lookup(self._h, int(tex), q.shape[0], _fptr(q), _fptr(out)), "mi_pt_texture_lookup")
        return out

    def texture_probe(self, tex, queries):
        """A noise texture's value on the device (mi_pt_texture_probe): queries [n, 9] = the interaction's world (p, dpdx, dpdy)
        -> [n], Texture<Float>::Evaluate times post_scale. A texture of another type is an error."""
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, 9)
        out = np.zeros(q.shape[0], np.float32)
        _check(hip_lib().mi_pt_texture_probe(self._h, int(tex), q.shape[0], _fptr(q), _fptr(out)), "mi_pt_texture_probe")
        return out

    def texture_eval_probe(self, tex, mode, queries):
        """Any texture record at given interactions on the device (mi_pt_texture_eval_probe): queries [n, 15] = (p, dpdx, dpdy,
        u, v, dudx, dvdx, dudy, dvdy). mode 0 -> [n, 6] (s, t, dsdx, dtdx, dsdy, dtdy) of the record's 2-D mapping; mode 1 ->
        [n, NSPEC], a spectrum texture's bins or a float texture's value times post_scale in bin 0."""
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, 15)
        out = np.zeros((q.shape[0], 6 if int(mode) == 0 else NSPEC), np.float32)
        _check(hip_lib().mi_pt_texture_eval_probe(self._h, int(tex), int(mode), q.shape[0], _fptr(q), _fptr(out)), "mi_pt_texture_eval_probe")
        return out

    def shape_probe(self, quadric, mode, queries):
        """One quadric of the scene on its own (mi_pt_shape_probe; index space of mi_prim.shape: spheres, then disks).
        mode 0: queries [n, 7] rays (o, d, tMax) -> [n, 16] hit, t, p, n, uv, dpdu, dpdv; mode 1: [n, 5] (ref, u) -> [n, 7]
        p, n, pdf of Shape::Sample(ref, u); mode 2: [n, 6] (ref, wi) -> [n] Shape::Pdf(ref, wi)."""
        n_in, n_out = {0: (7, 16), 1: (5, 7), 2: (6, 1)}[int(mode)]
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, n_in)
        out = np.zeros((q.shape[0], n_out), np.float32)
        _check(hip_lib().mi_pt_shape_probe(self._h, int(quadric), int(mode), q.shape[0], _fptr(q), _fptr(out)), "mi_pt_shape_probe")
        return out[:, 0] if n_out == 1 else out

    def light_probe(self, light, mode, queries):
        """One light of the scene on its own (mi_pt_light_probe). queries: [n, k] float32. mode 0: k = 8 (ref.p, ref.n, u) ->
        [n, LIGHT_PROBE_SAMPLE_FLOATS] wi, pdf, pLight.p, pLight.n, Li[31] of Light::Sample_Li; mode 1: k = 9 (ref.p, ref.n,
        wi) -> [n] Light::Pdf_Li; mode 2: k = 3 (d; infinite light: Le) or k = 6 (n, w; area light: L) -> [n, 31]. A bad light
        index or mode is the library's to refuse: RuntimeError with its message."""
        q = np.ascontiguousarray(queries, np.float32)
        q = q.reshape(len(q), -1)
        light, mode = int(light), int(mode)
        n_out = {0: LIGHT_PROBE_SAMPLE_FLOATS, 1: 1}.get(mode, NSPEC)
        want = {0: 8, 1: 9}.get(mode)
        if mode == 2 and 0 <= light < self.scene.desc.n_lights:   # mi_light_type: 0 = an area light, 3 = the infinite light
            want = {0: 6, 3: 3}.get(int(self.scene.desc.lights[light].type))
        if want is not None and q.shape[1] != want:
            raise ValueError("light_probe mode %d takes %d floats per query for this light" % (mode, want))
        out = np.zeros((q.shape[0], n_out), np.float32)
        _check(hip_lib().mi_pt_light_probe(self._h, int(light), int(mode), q.shape[0], _fptr(q), _fptr(out)), "mi_pt_light_probe")
        return out[:, 0] if n_out == 1 else out

    def sampler_probe(self, group, indices, first_dims):
        """The Halton routines of the shading kernel on their own (mi_pt_sampler_probe): per query the scrambled radical inverse
        of indices[i] in `group` consecutive dimensions from first_dims[i] on. group 5, 2, 1: the grouped routines (32-bit
        indices) -> [n, group]; group 0: the single-dimension routine with its 64-bit loop -> [n, 1]. What the library refuses
        is a RuntimeError with its message."""
        idx = np.ascontiguousarray(indices, np.uint64).reshape(-1)
        dims = np.ascontiguousarray(first_dims, np.int32).reshape(-1)
        if idx.shape != dims.shape:
            raise ValueError("sampler_probe: one first dimension per index")
        out = np.zeros((idx.shape[0], max(int(group), 1)), np.float32)
        _check(hip_lib().mi_pt_sampler_probe(self._h, int(group), idx.shape[0], idx.ctypes.data_as(C.POINTER(C.c_uint64)),
                                             dims.ctypes.data_as(C.POINTER(C.c_int32)), _fptr(out)), "mi_pt_sampler_probe")
        return out

    def bsdf_probe(self, material, instance, mode, form, queries, flags=31):
        """One material of the scene through the BSDF routines of one k_shade instance (mi_pt_bsdf_probe; `instance` indexes
        shade_instances()). queries: [n, 8] float32 wo, wi, u. mode 0: BSDF::f and Pdf for (wo, wi); mode 1: Sample_f(wo, u).
        form: how the 31 bins are formed -- 0 the lobe list bin by bin, 1 four bins at a time, 2 the straight-line form, 3 lobe
        by lobe (bsdf_probe_forms(instance) says which an instance compiles). Returns [n, 36]: f[31], pdf, wi[3], the sampled
        type; for form 2 [n, 38]: then 1 where the query's wave of 64 redid a quad, and 1 where a quotient of the query left
        the fast range. What the library refuses is a RuntimeError with its message."""
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, 8)
        out = np.zeros((q.shape[0], BSDF_PROBE_FLOATS + (2 if int(form) == 2 else 0)), np.float32)
        _check(hip_lib().mi_pt_bsdf_probe(self._h, int(material), int(instance), int(mode), int(form), int(flags), q.shape[0], _fptr(q), _fptr(out)),
               "mi_pt_bsdf_probe")
        return out


BSDF_PROBE_FLOATS = 36   # MI_BSDF_PROBE_FLOATS


def bsdf_probe_forms(instance):
    """The forms of PathIntegrator.bsdf_probe that k_shade instance `instance` compiles, as a tuple (mi_pt_bsdf_probe_forms; no
    device). ValueError for an instance the probe has no instantiation for."""
    m = C.c_uint32()
    if hip_lib().mi_pt_bsdf_probe_forms(int(instance), C.byref(m)) != 0:
        raise ValueError(hip_lib().mi_pt_last_error().decode())
    return tuple(f for f in range(4) if (m.value >> f) & 1)


def math_probe(op, x, y=None, device=0):
    """mi_pt_math_probe: the device's scalar helpers on arrays. x, y: [n, 2] float32; returns [n, 3]."""
    x = np.ascontiguousarray(x, np.float32)
    y = np.ascontiguousarray(x if y is None else y, np.float32)
    out = np.zeros((x.shape[0], 3), np.float32)
    _check(hip_lib().mi_pt_math_probe(device, int(op), x.shape[0], _fptr(x), _fptr(y), _fptr(out)), "mi_pt_math_probe")
    return out


# The shading plan (include/mi_pt.h, "Parity tools for the shading plan"): mirrors of the enums whose values are the bit
# numbers of a k_shade mask -- bit t: BXDF_TYPES[t], bit 16 + f: FRESNEL_TYPES[f], bit 24 + l: LIGHT_TYPES[l].
BXDF_TYPES = ("lambertian_reflection", "oren_nayar", "specular_reflection", "specular_transmission", "fresnel_specular",
              "microfacet_reflection", "microfacet_transmission", "lambertian_transmission", "disney_diffuse", "disney_fake_ss",
              "disney_retro", "disney_sheen", "disney_clearcoat", "fresnel_blend")
FRESNEL_TYPES = ("noop", "dielectric", "disney", "conductor")
LIGHT_TYPES = ("diffuse_area", "point", "distant", "infinite", "spot")
SAMPLER_TYPES = ("halton", "sobol", "random", "02sequence", "stratified")   # mi_sampler_type 0..4 (ZEROTWO: "02sequence")
# (tests/test_shade_plan.py reads the four enums from include/mi_pt.h and compares)
MAX_CLASSES = 16   # shading classes 0..14 of materials (14: the overflow class), MISS_CLASS: the escaped rays'
MISS_CLASS = 15
SHADE_MASK_NAMES = ("TM_DIFFUSE", "TM_PLASTIC", "TM_GLASS", "TM_UBER", "TM_DISNEY", "TM_GENERIC", "TM_FULL", "TM_ALL",
                    "TM_SCALED", "TM_TEXTURED", "TM_INSTANCES", "TM_SAMPLERS", "TM_LIGHTS_ALL", "TM_LIGHTS_NO_ENV")


def shade_mask(name):
    """A k_shade mask by its name in the device code (mi_pt_shade_mask); also an attribute of the package: pt.TM_UBER."""
    m = C.c_uint32()
    if hip_lib().mi_pt_shade_mask(name.encode(), C.byref(m)) != 0:
        raise ValueError(hip_lib().mi_pt_last_error().decode())
    return int(m.value)


def __getattr__(name):   # pt.TM_DIFFUSE, ...: read from the library when first asked (it loads without a GPU)
    if name in SHADE_MASK_NAMES:
        return shade_mask(name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


def lobe_bits(*names):
    """The mask bits of lobe types (BXDF_TYPES) and Fresnel kinds ("fresnel_" + FRESNEL_TYPES) given by name."""
    m = 0
    for n in names:
        if n in BXDF_TYPES:   # ("fresnel_specular" and "fresnel_blend" are lobe types)
            m |= 1 << BXDF_TYPES.index(n)
        elif n.startswith("fresnel_") and n[len("fresnel_"):] in FRESNEL_TYPES:
            m |= 1 << (16 + FRESNEL_TYPES.index(n[len("fresnel_"):]))
        else:
            raise ValueError("%r is neither a lobe type nor a Fresnel kind" % (n,))
    return m


def lobe_names(mask):
    """The names lobe_bits() takes, of the lobe and Fresnel bits set in a mask or type word."""
    return ([n for t, n in enumerate(BXDF_TYPES) if (mask >> t) & 1] +
            ["fresnel_" + n for f, n in enumerate(FRESNEL_TYPES) if (mask >> (16 + f)) & 1])


def shade_instances():
    """[(NL, TM)] of the k_shade instances in launch order (mi_pt_shade_instances; no device)."""
    n = C.c_uint32()
    lib = hip_lib()
    _check(lib.mi_pt_shade_instances(None, None, 0, C.byref(n)), "mi_pt_shade_instances")
    nl, tm = (C.c_int32 * n.value)(), (C.c_uint32 * n.value)()
    _check(lib.mi_pt_shade_instances(nl, tm, n.value, C.byref(n)), "mi_pt_shade_instances")
    return [(int(nl[i]), int(tm[i])) for i in range(n.value)]


def shade_grid(counts, classes):
    """Blocks of one k_shade launch for the shading queues' entry counts (16 of them) and an instance's class mask: each
    class of the mask padded to whole blocks of 256 on its own (mi_pt_shade_grid; no device)."""
    counts = [int(c) for c in counts]
    arr = (C.c_uint32 * len(counts))(*counts)
    blocks = C.c_uint32()
    lib = hip_lib()
    _check(lib.mi_pt_shade_grid(arr, len(counts), int(classes), C.byref(blocks)), "mi_pt_shade_grid")
    return int(blocks.value)


def _strategy_number(strategy):
    if isinstance(strategy, str):
        if strategy not in METADATA_STRATEGIES:
            raise ValueError("metadata strategy %r: one of %s" % (strategy, ", ".join(METADATA_STRATEGIES)))
        return METADATA_STRATEGIES.index(strategy)
    if int(strategy) not in range(len(METADATA_STRATEGIES)):
        raise ValueError("metadata strategy %r out of range" % (strategy,))
    return int(strategy)


class MetadataIntegrator(PathIntegrator):
    """Host mirror of ``MetadataIntegrator`` for ``Integrator "metadata"`` (src/integrators/metadata.cpp): ``Render()``
    gives the film sums of one map -- depth, material id, instance id or world coordinates of each camera sample's closest
    hit. ``strategy=None`` renders the scene file's strategy."""

    def Render(self, shard_index=0, shard_count=1, spp=0, path_pool=0, download=True, accumulate=False,
               sample_begin=0, film_out=None, weight_out=None, strategy=None):
        if strategy is None:
            strategy = int(self.scene.desc.integrator.metadata_strategy)
        return self.RenderMetadata(strategy, shard_index, shard_count, spp, path_pool, download, accumulate, sample_begin,
                                   film_out, weight_out)


def metadata_image(film, weight, strategy):
    """The map of a metadata render: film sums divided by the filter-weight sums (0 where no sample fell). [H, W] for
    depth, material and mesh (every bin holds the value: bin 0 is taken), [H, W, 3] for coordinates (bins 0, 1, 2)."""
    k = _strategy_number(strategy)
    film = np.asarray(film, np.float32)
    w = np.asarray(weight, np.float32)[..., None]
    img = np.divide(film[..., :3], w, out=np.zeros_like(film[..., :3]), where=w != 0)
    return img if METADATA_STRATEGIES[k] == "coordinates" else img[..., 0]


def CreatePathIntegrator(scene, device=0):
    """Factory named after the reference's (src/integrators/path.h:69-71)."""
    return PathIntegrator(scene, device)


def CreateIntegrator(scene, device=0):
    """The integrator the scene file names (MakeIntegrator, src/core/api.cpp:1750-1800): MetadataIntegrator for
    Integrator "metadata", PathIntegrator otherwise."""
    if int(scene.desc.integrator.kind) == INTEGRATOR_METADATA:
        return MetadataIntegrator(scene, device)
    return PathIntegrator(scene, device)


def noise_perm():
    """The permutation table behind the noise textures (mi_noise_perm): [512] int32, the permutation of 0..255 twice."""
    out = np.zeros(512, np.int32)
    host_lib().mi_noise_perm(out.ctypes.data_as(C.POINTER(C.c_int32)))
    return out


def write_dat(filename, film, scale=1.0):
    film = np.ascontiguousarray(film, np.float32)
    h, w, _ = film.shape
    rc = host_lib().mi_film_write_dat(os.fsencode(filename), w, h, _fptr(film), scale)
    if rc != 0:
        raise RuntimeError(host_lib().mi_scene_last_error().decode())


def write_rgb(filename, film, weight, scale=1.0):
    """Film::WriteImage with spectralFlag = false: weighted RGB image as .pfm or .tga (mi_film_write_rgb)."""
    film = np.ascontiguousarray(film, np.float32)
    weight = np.ascontiguousarray(weight, np.float32)
    h, w, _ = film.shape
    lib = host_lib()
    lib.mi_film_write_rgb.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_float]
    if lib.mi_film_write_rgb(os.fsencode(filename), w, h, _fptr(film), _fptr(weight), scale) != 0:
        raise RuntimeError(lib.mi_scene_last_error().decode())


def read_dat(filename):
    w, h = C.c_int(), C.c_int()
    lib = host_lib()
    if lib.mi_film_read_dat(os.fsencode(filename), C.byref(w), C.byref(h), None, 0) != 0:
        raise RuntimeError(lib.mi_scene_last_error().decode())
    out = np.zeros((h.value, w.value, NSPEC), np.float32)
    if lib.mi_film_read_dat(os.fsencode(filename), C.byref(w), C.byref(h), _fptr(out), out.size) != 0:
        raise RuntimeError(lib.mi_scene_last_error().decode())
    return out
