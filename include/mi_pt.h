/*
 * mi_pt.h -- C ABI of the MI355X spectral path-tracing hot path.
 *
 * This is the one boundary the build introduces: host C++ (scene front end,
 * Integrator-shaped class) -> C ABI -> hand-written HIP kernels (gfx950).
 * It replaces, for `Integrator "path"`, the body of the reference's
 *     SamplerIntegrator::Render(const Scene&)       src/core/integrator.cpp:228-342
 *     PathIntegrator::Li(...)                       src/integrators/path.cpp:64-188
 * The reference has no FFI: its integrator contract is the C++ virtual
 *     class Integrator { virtual void Render(const Scene &scene) = 0; }
 *                                                   src/core/integrator.h:53-58
 * and Scene / BVHAccel keep their data private (src/core/scene.h:76-79,
 * src/accelerators/bvh.h:91-94), so the drop-in is at the `.pbrt` file +
 * `Integrator "path"` level: the host front end flattens the scene into the POD
 * description below and calls mi_pt_*.
 *
 * Conventions: plain pointers + counts, host memory unless a flag says device;
 * inputs are copied at mi_pt_create (caller keeps ownership); every entry point
 * returns 0 on success or a negative mi_status, never aborts, never throws;
 * one handle per GPU, calls on one handle are serialised by the caller.
 * Spectrum = float[MI_NSPEC] (31 bins over 395..705 nm, src/core/spectrum.h:48-50).
 */
#ifndef MI_PT_H
#define MI_PT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_NSPEC 31
#define MI_ABI_VERSION 15
#define MI_MAX_BXDFS 8 /* BSDF::MaxBxDFs, src/core/reflection.h:196 */

typedef enum mi_status {
    MI_OK = 0,
    MI_ERR_INVALID = -1,   /* bad argument / malformed description */
    MI_ERR_NO_DEVICE = -2, /* no HIP device / ordinal out of range */
    MI_ERR_HIP = -3,       /* a HIP runtime call failed (see mi_pt_last_error) */
    MI_ERR_UNSUPPORTED = -4,
    MI_ERR_NOMEM = -5
} mi_status;

/* ---- acceleration structure: same 32-byte node as LinearBVHNode
 *      (src/accelerators/bvh.cpp:95-104), depth-first, first child = idx+1. */
typedef struct mi_bvh_node {
    float bmin[3];
    float bmax[3];
    int32_t offset;    /* leaf: first primitive; interior: second child */
    uint16_t n_prims;  /* 0 -> interior */
    uint8_t axis;
    uint8_t pad;
} mi_bvh_node;

/* One GeometricPrimitive (src/core/primitive.h:70-95) in BVH leaf order. */
typedef struct mi_prim {
    int32_t shape;      /* >=0: triangle index; <0: ~quadric index: [0, n_spheres) spheres, then n_disks disks (ignored when `instance` is set) */
    int32_t material;   /* index into materials, -1 = none (interface only) */
    int32_t area_light; /* index into lights, -1 = not emissive */
    int32_t instance;   /* 0: a GeometricPrimitive; k + 1: the TransformedPrimitive of mi_scene_desc.instances[k] (ABI v7) */
} mi_prim;

/* One ObjectInstance (TransformedPrimitive, src/core/primitive.cpp:78-99; api.cpp:1570-1615): the primitives of a named
 * object, kept in the space they were declared in behind a BVH of their own (`root`: that tree's root in
 * mi_scene_desc.nodes, whose interior / leaf offsets are absolute like the world tree's), reached by carrying the ray into
 * that space with WorldToInstance (Transform::operator()(Ray), transform.h:262-277: origin error bound, dt shift of the
 * origin and of tMax) and carrying the SurfaceInteraction back with InstanceToWorld (transform.cpp:262-297). Matrices row
 * major, m[r*4+c]; w2i is the stored inverse of i2w (Transform::mInv), not a recomputation. Objects hold no area lights. */
typedef struct mi_instance {
    float i2w[16], w2i[16];
    uint32_t root;
    uint32_t motion;      /* index + 1 into mi_scene_desc.motions: the instance moves; 0 = static */
    uint32_t instance_id; /* SurfaceInteraction::instanceId of a hit reached through it: the 1-based number of its
                           * ObjectInstance call; 0 for the wrapper of a moving Shape (api.cpp:1363-1430) */
    uint32_t pad;
} mi_instance;

/* The AnimatedTransform of a moving TransformedPrimitive (src/core/transform.cpp:396-411, 1144-1224; object motion, built by
 * the front end only with MIPT_OBJECT_MOTION=1 in the environment). The instance's i2w / w2i are the start member (times <=
 * transform_start), i2w_end / w2i_end the end member with its stored inverse (times >= transform_end). Between the two
 * times a ray of time t is carried by Interpolate(t): m = Translate(Lerp T) * Slerp(dt, R[0], R[1]).ToTransform() *
 * Transform(Lerp S), dt = (t - transform_start) / (transform_end - transform_start), and by that product's own mInv =
 * Inverse(Lerp S) * (the un-transposed quaternion matrix) * Translate(-Lerp T), Inverse being the reference's Gauss-Jordan
 * (transform.cpp:82-136). T, R, S as in mi_camera: R = {x, y, z, w}, R[1] already negated onto the shorter arc; S the upper
 * 3x3 of the scale matrix, row major. has_rotation: Dot(R[0], R[1]) < 0.9995 after that flip (the
 * reference's hasRotation, transform.cpp:411; only the world bound asks). Members that are equal make no record. The
 * version number stays 15: a description without motion records is laid out and read exactly as before (the two words of
 * mi_instance were padding, kept 0; the new array is appended), and a hand-built v15 instance with instance_id 0 still
 * reports its index + 1 where it has no motion record. */
typedef struct mi_motion {
    float i2w_end[16], w2i_end[16];
    float T[2][3], R[2][4], S[2][9];
    float transform_start, transform_end;
    int32_t has_rotation;
    int32_t pad;
} mi_motion;

/* Per TriangleMesh flags (src/shapes/triangle.cpp:54-92). */
#define MI_MESH_HAS_N 1u
#define MI_MESH_HAS_UV 2u
#define MI_MESH_FLIP 4u /* reverseOrientation ^ transformSwapsHandedness */
typedef struct mi_mesh {
    uint32_t flags;
    uint32_t first_vertex, n_vertices;
    uint32_t first_tri, n_tris;
    /* "alpha" / "shadowalpha" float textures (triangle.cpp:331-338,531-570,716-740): index into textures, -1 = none.
     * A hit whose texture value is exactly 0 is no hit ("shadowalpha" for IntersectP only). The value is channel 0 of the
     * texture (float image textures are stored grey), looked up with zero footprint. */
    int32_t alpha_tex, shadow_alpha_tex;
} mi_mesh;

/* Sphere (src/shapes/sphere.h:49-66). Matrices row-major, m[r*4+c]. */
typedef struct mi_sphere {
    float o2w[16], w2o[16];
    float radius, z_min, z_max, theta_min, theta_max, phi_max;
    int32_t reverse_orientation, swaps_handedness;
} mi_sphere;

/* Disk (src/shapes/disk.h, ABI v14): the second kind of quadric. Quadric index n_spheres + k is disks[k]. phi_max in radians
 * (after Radians(Clamp(phimax, 0, 360))); w2o is the stored inverse. `kind` tells the quadrics that share this record's
 * layout apart (0 = disk; the others are not built). */
#define MI_QUADRIC_DISK 0
typedef struct mi_disk {
    float o2w[16], w2o[16];
    float height, radius, inner_radius, phi_max;
    int32_t reverse_orientation, swaps_handedness;
    int32_t kind;
    int32_t pad;
} mi_disk;

/* ---- materials: with constant textures (src/textures/constant.h:49-58) a
 * Material::ComputeScatteringFunctions result is a fixed BxDF list; image textures bind to lobes through mi_lobe_tex. */
typedef enum mi_bxdf_type {
    MI_BXDF_LAMBERTIAN_REFLECTION = 0, /* R */
    MI_BXDF_OREN_NAYAR,                /* R, p[0]=A, p[1]=B */
    MI_BXDF_SPECULAR_REFLECTION,       /* R, fresnel */
    MI_BXDF_SPECULAR_TRANSMISSION,     /* R(=T), p[0]=etaA, p[1]=etaB */
    MI_BXDF_FRESNEL_SPECULAR,          /* R, S(=T), p[0]=etaA, p[1]=etaB */
    MI_BXDF_MICROFACET_REFLECTION,     /* R, p[0]=alphax, p[1]=alphay, fresnel, p[5]=separableG */
    MI_BXDF_MICROFACET_TRANSMISSION,   /* R(=T), p[0]=alphax, p[1]=alphay, p[2]=etaA, p[3]=etaB, p[5]=separableG */
    MI_BXDF_LAMBERTIAN_TRANSMISSION,   /* R(=T) */
    MI_BXDF_DISNEY_DIFFUSE,            /* R */
    MI_BXDF_DISNEY_FAKE_SS,            /* R, p[0]=roughness */
    MI_BXDF_DISNEY_RETRO,              /* R, p[0]=roughness */
    MI_BXDF_DISNEY_SHEEN,              /* R */
    MI_BXDF_DISNEY_CLEARCOAT,          /* p[0]=weight, p[1]=gloss */
    MI_BXDF_FRESNEL_BLEND              /* R(=Rd), S(=Rs), p[0]=alphax, p[1]=alphay (reflection.cpp:279-298,450-475) */
} mi_bxdf_type;

typedef enum mi_fresnel_type {
    MI_FRESNEL_NOOP = 0,
    MI_FRESNEL_DIELECTRIC, /* p[2]=etaI, p[3]=etaT */
    MI_FRESNEL_DISNEY,     /* S=R0, p[2]=metallic, p[3]=eta */
    MI_FRESNEL_CONDUCTOR   /* etaI = 1, S=etaT, K=k per bin (FrConductor, reflection.cpp:71-94) */
} mi_fresnel_type;

/* BxDFType bits, src/core/reflection.h:153-161 */
#define MI_BSDF_REFLECTION 1
#define MI_BSDF_TRANSMISSION 2
#define MI_BSDF_DIFFUSE 4
#define MI_BSDF_GLOSSY 8
#define MI_BSDF_SPECULAR 16
#define MI_BSDF_ALL 31

typedef struct mi_bxdf {
    int32_t type;    /* mi_bxdf_type */
    int32_t flags;   /* BxDFType bits */
    int32_t fresnel; /* mi_fresnel_type (reflection lobes) */
    int32_t scaled;  /* the number of ScaledBxDF wrappers around the lobe (mix materials, reflection.cpp:96-107): 1: f = scale * f;
                        2 (ABI v10, a "mix" of a "mix"): f = scale2 * (scale * f) */
    float p[8];
    float R[MI_NSPEC];
    float S[MI_NSPEC];
    float K[MI_NSPEC];     /* conductor absorption k */
    float scale[MI_NSPEC]; /* ScaledBxDF::scale */
    float scale2[MI_NSPEC]; /* the outer ScaledBxDF's scale when scaled == 2 */
} mi_bxdf;

/* A lobe whose spectrum comes from an image texture (ABI v5). The lobe list of a material stays fixed; at a hit the
 * texture value T = Clamp(Spectrum::FromRGB(mipmap lookup)) (imagemap.h:82-93,113-117; FromRGB's default type is
 * Illuminant, spectrum.h:428-429, so the conversion uses rgb_illum like the environment light's) replaces R (or S), or scales
 * the constant stored there when MI_LOBE_TEX_MUL_* is set (uber: `op * Kd->Evaluate(si).Clamp()`, uber.cpp:71-72;
 * translucent: `r * kd`, translucent.cpp:62), and the lobe is left out of the BSDF at that hit when the spectrum the
 * material tests with IsBlack() is black (`if (!r.IsBlack()) bsdf->Add(...)`, matte.cpp:58-63). */
#define MI_LOBE_TEX_MUL_R 1u
#define MI_LOBE_TEX_MUL_S 2u
typedef enum mi_lobe_rule {
    MI_LOBE_IF_R = 0,      /* present iff the lobe's R (after the multiplier) is not black */
    MI_LOBE_IF_R_OR_S = 1, /* present iff R or S is not black (FresnelSpecular glass.cpp:70-72,78-80; FresnelBlend substrate.cpp:53) */
    MI_LOBE_IF_TEX = 2,    /* present iff the texture value itself is not black (translucent.cpp:59-60,68-69) */
    /* ABI v10 -- "disney" with an image-textured "color" (disney.cpp:485-587). The material adds its lobes whatever the colour
     * is, and three of their spectra are not linear in it. With c = the texture value (clamped), lum = c.y() and
     * Ctint = lum > 0 ? c / lum : 1 (per bin), the lobe's textured channel is:
     *   MI_LOBE_ALWAYS          R = c (or the constant R times c with MI_LOBE_TEX_MUL_R): the diffuse, retro, fake-subsurface and
     *                           diffuse-transmission lobes, whose weights are the constant
     *   MI_LOBE_DISNEY_SHEEN    R = Lerp(p[7], 1, Ctint) * p[6]            (Csheen * (diffuseWeight * sheenWeight))
     *   MI_LOBE_DISNEY_SPEC     R = c, S = Lerp(p[2], Lerp(p[6], 1, Ctint) * p[7], c)   (Cspec0; p[2] = metallic, p[6] = specularTint,
     *                           p[7] = SchlickR0FromEta(eta)) -- the microfacet lobe with the Disney Fresnel term
     *   MI_LOBE_DISNEY_STRANS   R = sqrt(c) * p[6]                          (strans * Sqrt(c))
     * where Lerp(t, a, b) = a * (1 - t) + b * t as Spectrum arithmetic does it (spectrum.h:577-580). */
    MI_LOBE_ALWAYS = 3,
    MI_LOBE_DISNEY_SHEEN = 4,
    MI_LOBE_DISNEY_SPEC = 5,
    MI_LOBE_DISNEY_STRANS = 6,
    /* "metal" with image-textured `eta` / `k` (metal.cpp:119-122: FresnelConductor(1, eta->Evaluate(si), k->Evaluate(si))):
     * tex_S = eta's texture, tex_R = k's -- the lobe's R stays the constant 1 -- either may be -1; always present */
    MI_LOBE_METAL = 7
} mi_lobe_rule;
typedef struct mi_lobe_tex {
    int32_t tex_R, tex_S; /* index into mi_scene_desc.textures, -1 = the constant in mi_bxdf */
    uint32_t flags;       /* MI_LOBE_TEX_MUL_* */
    int32_t rule;         /* mi_lobe_rule */
} mi_lobe_tex;

typedef struct mi_material {
    int32_t n_bxdfs;
    float eta; /* BSDF::eta, src/core/reflection.h:189 */
    int32_t kind; /* informational: 0 matte 1 plastic 2 glass 3 uber 4 disney 5 mirror 6 metal 7 substrate 8 translucent 9 mix */
    int32_t textured; /* != 0: some lobe has tex_R / tex_S >= 0, or bump_tex >= 0 */
    mi_bxdf bxdf[MI_MAX_BXDFS];
    mi_lobe_tex tex[MI_MAX_BXDFS];
    int32_t bump_tex; /* "bumpmap": float image texture displacing the shading geometry (Material::Bump, material.cpp:47-84), -1 = none */
    /* "roughness" / "uroughness" / "vroughness" given as float image textures (plastic.cpp:57-62, uber.cpp:88-96,
     * substrate.cpp:55-60, metal.cpp:66-73, translucent.cpp:70-72): texture of the u / v roughness of the material's
     * microfacet lobes, -1 = the constant alpha in mi_bxdf.p[0] / p[1]. The value at the hit, through RoughnessToAlpha when
     * MI_ROUGH_REMAP is set, replaces that constant in every microfacet / FresnelBlend lobe of the material. */
    int32_t rough_tex[2];
    uint32_t rough_flags;
    /* ABI v10 -- "matte" with `sigma` a float image texture (matte.cpp:55-62): at the hit sig = Clamp(value, 0, 90), and the
     * material's diffuse lobe (compiled as MI_BXDF_OREN_NAYAR) is a LambertianReflection where sig == 0 and an OrenNayar with
     * the A, B of that sig elsewhere (reflection.h:414-420). -1 = the constants of the lobe. */
    int32_t sigma_tex;
} mi_material;
#define MI_ROUGH_REMAP 1u
/* ABI v10 -- "glass" with `uroughness` / `vroughness` float image textures (glass.cpp:60-92): the material holds the lobes of both
 * branches -- lobe 0 the FresnelSpecular one, after it the microfacet reflection / transmission lobes -- and the hit decides:
 * `isSpecular = urough == 0 && vrough == 0` on the values before the remap (a constant axis keeps its raw value in lobe 0's
 * p[6] (u) / p[7] (v)); lobe 0 is part of the BSDF where isSpecular holds, the others where it does not. */
#define MI_ROUGH_GLASS 2u
/* ABI v10 -- "disney" with `roughness` a float image texture (disney.cpp:491, 538-541, 568-573): rough_tex[0] is the map and the
 * value at the hit, rough, replaces p[0] of the DISNEY_FAKE_SS / DISNEY_RETRO lobes and gives the microfacet lobes their alphas:
 * max(.001, sqr(r) / p[4]), max(.001, sqr(r) * p[4]) with p[4] = aspect (from "anisotropic") and r = rough -- or p[7] * rough for the
 * thin surface's transmission lobe, whose p[7] = 0.65 eta - 0.35 (0 elsewhere). */
#define MI_ROUGH_DISNEY 4u

/* ImageTexture<RGBSpectrum, Spectrum> with UVMapping2D (or, opt-in, another TextureMapping2D: mi_tex_mapping) (src/textures/imagemap.h, src/core/texture.cpp:91-99) over a
 * MIPMap<RGBSpectrum> (src/core/mipmap.h). The pyramid is built on the host exactly as the reference builds it (y flip,
 * scale, inverse gamma, power-of-two Lanczos resampling, 2x2 box levels); the render side filters it per hit with the
 * reference's EWA / trilinear lookup from the hit's (u, v) and its screen-space derivatives. */
#define MI_MAX_MIP_LEVELS 16
typedef struct mi_mipmap {
    int32_t n_levels;
    int32_t wrap;           /* 0 repeat, 1 black, 2 clamp (ImageWrap, mipmap.h:50) */
    int32_t width, height;  /* level 0; level l is max(1, width >> l) x max(1, height >> l) */
    const float *texels;    /* RGB triples, all levels back to back, rows from t = 0 */
    uint32_t level_offset[MI_MAX_MIP_LEVELS]; /* first texel of level l */
} mi_mipmap;
typedef enum mi_tex_filter { MI_TEX_EWA = 0, MI_TEX_TRILINEAR = 1, MI_TEX_NONE = 2 /* "noFiltering" */ } mi_tex_filter;
typedef struct mi_texture {   /* spectrum textures: RGB pyramid; float textures: the same with r = g = b (convertIn, imagemap.h:107-110) */
    int32_t mipmap;         /* index into mi_scene_desc.mipmaps */
    int32_t filter;         /* mi_tex_filter */
    float max_aniso;        /* "maxanisotropy" */
    float su, sv, du, dv;   /* UVMapping2D */
    float post_scale;       /* float textures: the looked-up value is multiplied by this (1 for a plain image texture; the
                             * constant operand of a Texture "scale" over an image texture, scale.h:56-58) */
    int32_t type;           /* mi_tex_type */
    int32_t aa_none;        /* checkerboard: "aamode" "none" (point sampled) instead of the closed-form box filter */
    float spec1[MI_NSPEC], spec2[MI_NSPEC]; /* checkerboard: "tex1" / "tex2" (constant spectra) */
    int32_t octaves;        /* noise textures ("fbm", "wrinkled"): "octaves", 0..32 */
    float omega;            /* noise textures ("fbm", "wrinkled"): "roughness" */
    float w2t[16];          /* noise textures and MI_TEX_CHECKERBOARD3D: IdentityMapping3D's WorldToTexture, row major; the spherical
                             * and cylindrical mappings: their WorldToTexture (the inverse of the CTM at the Texture statement) */
    int32_t is_float;       /* the record was declared as a "float" texture (a value), not as a "spectrum" / "color" one */
    /* the opt-in mappings and classes (MIPT_TEXTURES=all; zero in every record made without the switch) */
    int32_t mapping;        /* mi_tex_mapping of a class over a TextureMapping2D; MI_MAP_PLANAR keeps ds, dt in du, dv */
    float vs[3], vt[3];     /* MI_MAP_PLANAR: "vector v1", "vector v2" */
    float bilerp[4];        /* MI_TEX_BILERP: v00, v01, v10, v11 */
} mi_texture;
/* MI_TEX_CHECKERBOARD: Checkerboard2DTexture<Spectrum> over UVMapping2D (src/textures/checkerboard.h:47-86): the value is
 * (1 - a) * spec1 + a * spec2 with a = 0 / 1 inside a check and the box-filtered area fraction across an edge. */
/* MI_TEX_FBM / MI_TEX_WRINKLED / MI_TEX_WINDY: the 3-D noise textures over IdentityMapping3D (src/textures/{fbm,wrinkled,windy}.h,
 * src/core/texture.cpp:157-251), evaluated at the hit point with its world-space footprint dpdx / dpdy. No pyramid: mipmap is -1.
 * A float one yields the value times post_scale, a spectrum one Spectrum(value). Not legal as a mesh's alpha_tex / shadow_alpha_tex.
 * (spec1 / spec2 of such a record are ignored: the device copy carries 0 and 1 there, the compact form Spectrum(value) is expanded from.) */
/* MI_TEX_DOTS / MI_TEX_UV / MI_TEX_BILERP / MI_TEX_CHECKERBOARD3D (the front end makes them only under MIPT_TEXTURES=all):
 *   DOTS (src/textures/dots.h:59-78), float and spectrum: spec1 where the point lies outside the cell's dot, spec2 inside it
 *     (a float record keeps its two operands in spec1[0] / spec2[0]). The reference hands the parameter "inside" to the
 *     constructor's outsideDot (dots.cpp:62-66, 91-95 against dots.h:53-55), so spec1 is "inside" and spec2 is "outside".
 *   UV (uv.h:54-59), spectrum only: FromRGB({s - floor(s), t - floor(t), 0}).
 *   BILERP (bilerp.h:56-62), float only: bilerp[] bilinear in (s, t).
 *   CHECKERBOARD3D (checkerboard.h:118-128), float and spectrum: spec1 / spec2 by the parity of floor(x) + floor(y) + floor(z)
 *     of w2t(p); point sampled. MI_TEX_CHECKERBOARD may now be a float record too: (1 - a) * spec1[0] + a * spec2[0].
 * A float record's value is multiplied by post_scale. None of them is legal as a mesh's alpha_tex / shadow_alpha_tex, and an
 * image texture is only under MI_MAP_UV: the traversal kernels hold neither the mappings nor these classes. */
typedef enum mi_tex_type { MI_TEX_IMAGEMAP = 0, MI_TEX_CHECKERBOARD = 1, MI_TEX_FBM = 2, MI_TEX_WRINKLED = 3, MI_TEX_WINDY = 4,
                           MI_TEX_DOTS = 5, MI_TEX_UV = 6, MI_TEX_BILERP = 7, MI_TEX_CHECKERBOARD3D = 8 } mi_tex_type;
#define MI_TEX_IS_NOISE(type) ((type) >= MI_TEX_FBM && (type) <= MI_TEX_WINDY)
/* TextureMapping2D::Map (src/core/texture.cpp:91-155) of imagemap, checkerboard, dots, uv and bilerp records */
typedef enum mi_tex_mapping { MI_MAP_UV = 0, MI_MAP_SPHERICAL = 1, MI_MAP_CYLINDRICAL = 2, MI_MAP_PLANAR = 3 } mi_tex_mapping;
#define MI_TEX_HAS_MAPPING2D(type) ((type) == MI_TEX_IMAGEMAP || (type) == MI_TEX_CHECKERBOARD || ((type) >= MI_TEX_DOTS && (type) <= MI_TEX_BILERP))
/* "this record needs the hit point": a 3-D class, or a 2-D one under another mapping than uv */
#define MI_TEX_NEEDS_POINT(t) (MI_TEX_IS_NOISE((t).type) || (t).type == MI_TEX_CHECKERBOARD3D || (MI_TEX_HAS_MAPPING2D((t).type) && (t).mapping != MI_MAP_UV))
/* a record only the general texture-evaluating k_shade instances can evaluate: it needs the point or is one of the opt-in classes
 * (a float checkerboard among them) */
#define MI_TEX_IS_GENERAL(t) (MI_TEX_NEEDS_POINT(t) || (t).type >= MI_TEX_DOTS || ((t).type == MI_TEX_CHECKERBOARD && (t).is_float))
#define MI_NOISE_MAX_OCTAVES 32

/* ---- lights */
typedef enum mi_light_type {
    MI_LIGHT_DIFFUSE_AREA = 0, /* src/lights/diffuse.cpp */
    MI_LIGHT_POINT,            /* src/lights/point.cpp */
    MI_LIGHT_DISTANT,          /* src/lights/distant.cpp */
    MI_LIGHT_INFINITE,         /* src/lights/infinite.cpp (environment light; mi_envmap) */
    MI_LIGHT_SPOT              /* src/lights/spot.cpp: pos, L = I, w2l, cos_total_width, cos_falloff_start */
} mi_light_type;
/* src/lights/projection.cpp: the sixth light type, a point light whose intensity is an image seen through a perspective
 * frustum: pos, L = I * scale, w2l (all of WorldToLight's 3x3, scale included), cos_total_width, and the fields from
 * `screen` on. It stands outside the enum because the enum's values are also the bit numbers 24 + type of a k_shade mask,
 * and bits 24..28 are taken: the projection has no mask bit, its code is held by the general instances (TM_HOLDS_PROJECTION)
 * and a scene with such a light is shaded by those alone. */
#define MI_LIGHT_PROJECTION 5

typedef struct mi_light {
    int32_t type;
    int32_t shape;     /* area: >=0 triangle index, <0 ~quadric index (see mi_prim.shape) */
    int32_t two_sided;
    float area;        /* Shape::Area() */
    float L[MI_NSPEC]; /* Lemit / I / L; infinite: Spectrum(Lmap->Lookup((.5,.5), .5), Illuminant), i.e. Power() / (pi r^2) */
    float pos[3];      /* point: pLight */
    float dir[3];      /* distant: wLight (normalised, world) */
    float world_radius;
    float world_center[3];
    int32_t envmap;    /* infinite: index into mi_scene_desc.envmaps */
    float l2w[9], w2l[9]; /* infinite, spot: rotation part of LightToWorld / WorldToLight, row major */
    float cos_total_width, cos_falloff_start; /* spot; projection: cos_total_width (only Power() reads it) */
    /* MI_LIGHT_PROJECTION (appended; read for that type only, 0 in the records of the other lights) */
    float screen[4];     /* screenBounds {pMin.x, pMin.y, pMax.x, pMax.y}: [-aspect, aspect] x [-1, 1] for aspect > 1, else
                          * [-1, 1] x [-1 / aspect, 1 / aspect]; aspect from the file's own resolution, 1 without a map */
    float proj[16];      /* lightProjection = Perspective(fov, hither, yon).m, row major; yon = 1e30f */
    float hither;        /* 1e-3f: directions with wl.z < hither are behind the light */
    int32_t proj_map;    /* index into mi_scene_desc.envmaps of projectionMap's level 0 (a record without a distribution:
                          * nu = nv = 0, null tables), -1 = no map: Projection is Spectrum(1) inside the frustum */
    float proj_centre[MI_NSPEC]; /* Spectrum(projectionMap->Lookup((.5,.5), .5), Illuminant), Spectrum(1) without a map:
                                  * Power() = proj_centre * L * 2 pi (1 - cos_total_width); the render does not read it */
} mi_light;

/* InfiniteAreaLight::Lmap (level 0 of the MIPMap<RGBSpectrum>, after the reference's power-of-two resampling)
 * and its sampling distribution (src/lights/infinite.cpp:43-83, src/core/sampling.h:123-147). The light looks
 * the map up with width 0 (bilinear on level 0, mipmap.h:271-281) and converts the RGB value to a spectrum per
 * lookup (Spectrum(rgb, SpectrumType::Illuminant), spectrum.cpp:98-180 with rgb_illum below). */
typedef struct mi_envmap {
    int32_t width, height;     /* Lmap->Width(), Height() */
    const float *rgb;          /* [height * width * 3] */
    int32_t nu, nv;            /* Distribution2D: nu = 2 * width, nv = 2 * height. A projection light's map
                                * (mi_light.proj_map) has no distribution: nu = nv = 0 and the five tables NULL */
    const float *cond_func;    /* [nv * nu]       pConditionalV[v]->func */
    const float *cond_cdf;     /* [nv * (nu + 1)] pConditionalV[v]->cdf */
    const float *cond_func_int;/* [nv]            pConditionalV[v]->funcInt */
    const float *marg_func;    /* [nv]            pMarginal->func (= cond_func_int) */
    const float *marg_cdf;     /* [nv + 1] */
    float marg_func_int;
} mi_envmap;

/* Light-selection pmf (src/core/lightdistrib.cpp). For UNIFORM / POWER the host
 * supplies one Distribution1D (func[n_lights], cdf[n_lights+1], func_int[1]). For
 * SPATIAL only the voxel resolution is given (func/cdf/func_int NULL,
 * n_distributions 0): mi_pt_create estimates one pmf per voxel on the device with
 * the reference's 128-point Halton estimator (lightdistrib.cpp:232-300), because the
 * estimator needs Light::Sample_Li, which lives on the render side of this ABI. */
typedef enum mi_lightdistrib_type { MI_LD_UNIFORM = 0, MI_LD_POWER, MI_LD_SPATIAL } mi_lightdistrib_type;
typedef struct mi_lightdistrib {
    int32_t type;
    int32_t n_voxels[3]; /* SPATIAL only */
    uint32_t n_distributions;
    const float *func;
    const float *cdf;
    const float *func_int;
} mi_lightdistrib;

/* ---- camera: perspective (src/cameras/perspective.cpp:45-146) or, ABI v13, realistic (src/cameras/realistic.cpp) */
/* MI_CAMERA_ORTHOGRAPHIC (src/cameras/orthographic.cpp) and MI_CAMERA_ENVIRONMENT (src/cameras/environment.cpp, the fork's
 * omnistereo camera) are made by the front end under MIPT_CAMERAS=all only. Orthographic: raster_to_camera =
 * Inverse(Orthographic(0, 1)) * RasterToScreen, lens_radius / focal_distance as parsed. Environment: lens_radius is 0 (no lens
 * dimensions are evaluated), raster_to_camera is the perspective stand-in nothing renders with, and the four env_* fields of
 * mi_scene_desc hold the omnistereo parameters. Both have ray weight 1. */
typedef enum mi_camera_type { MI_CAMERA_PERSPECTIVE = 0, MI_CAMERA_REALISTIC = 1, MI_CAMERA_ORTHOGRAPHIC = 2, MI_CAMERA_ENVIRONMENT = 3 } mi_camera_type;
/* ABI v13 -- Camera "realistic": the lens system as RealisticCamera's constructor leaves it (realistic.cpp:126-187). Plain
 * data. elements[i] = {curvature radius, thickness, eta, aperture radius} of interface i, front (scene side) first, in
 * metres (the file's mm * .001, the diameter halved); curvature radius 0 is the aperture stop, whose aperture is the
 * clamped "aperturediameter". The last thickness is the focused lens-to-film distance (film_distance repeats it): the
 * "filmdistance" parameter, or FocusThickLens("focusdistance") when that is 0. exit_pupil_bounds[k] = {x0, y0, x1, y1}: the
 * bounds of the exit pupil on the rear element's plane seen from film points at radius [k, k + 1) / 64 of the half diagonal
 * (BoundExitPupil, realistic.cpp:753-790). physical_extent = Film::GetPhysicalExtent() {x0, y0, x1, y1} and film_diagonal
 * = Film::diagonal in metres (film.cpp:54, 94-99). */
#define MI_MAX_LENS_ELEMENTS 32
#define MI_EXIT_PUPIL_BOUNDS 64
typedef struct mi_lens {
    int32_t n_elements;
    int32_t simple_weighting;      /* "simpleweighting" (true) */
    int32_t no_weighting;          /* "noweighting": parsed, never read (as in the reference) */
    int32_t chromatic_aberration;  /* "chromaticAberrationEnabled" (false) */
    int32_t full_res[2];           /* Film::fullResolution (= mi_film.full_res): a sample's film point is pFilm / full_res */
    float film_distance;
    float film_diagonal;
    float thick_lens_pz[2], thick_lens_fz[2]; /* ComputeThickLensApproximation's cardinal points, film side [0] and scene
                                               * side [1], traced before focusing; fz[0] - pz[0] is the effective focal length */
    float physical_extent[4];
    float elements[MI_MAX_LENS_ELEMENTS][4];
    float exit_pupil_bounds[MI_EXIT_PUPIL_BOUNDS][4];
} mi_lens;
typedef struct mi_camera {
    float raster_to_camera[16];
    float camera_to_world[16];
    float lens_radius, focal_distance;
    float shutter_open, shutter_close;
    /* ABI v12 -- a moving camera: CameraToWorld as an AnimatedTransform (src/core/transform.cpp:396-411, 1103-1193).
     * camera_to_world is the start transform (at times <= transform_start), camera_to_world_end the end transform (at times
     * >= transform_end); a ray's time is Lerp(time sample, shutter_open, shutter_close) (perspective.cpp:89, 141). `animated`
     * = actuallyAnimated: 0 when the two transforms are equal, and then the fields after it are 0 and every ray takes
     * camera_to_world. Otherwise T, R, S are the two members taken apart by AnimatedTransform::Decompose: translation, the
     * rotation as a quaternion {x, y, z, w} -- R[1] already negated where Dot(R[0], R[1]) < 0 -- and the upper 3x3 of the
     * scale matrix, row major. Between the two times a ray is carried by
     * Translate(Lerp T) * Slerp(dt, R[0], R[1]).ToTransform() * Lerp S with dt = (time - start) / (end - start). */
    float camera_to_world_end[16];
    float transform_start, transform_end;
    int32_t animated;
    float T[2][3], R[2][4], S[2][9];
    /* (ABI v13: the camera's type and a realistic camera's lens system are mi_scene_desc.camera_type and .lens; this record
     * keeps its size. For a realistic camera raster_to_camera is the matrix of a perspective camera with the scene's "fov"
     * (default 90): a defined value nothing renders with; lens_radius is the rear element's aperture radius (> 0: the camera
     * sample's lens dimensions are evaluated) and focal_distance the "focusdistance".) */
} mi_camera;

/* ---- film + reconstruction filter (src/core/film.cpp:50-112, film.h:123-163) */
typedef struct mi_film {
    int32_t full_res[2];
    int32_t cropped_bounds[4]; /* x0,y0,x1,y1 (max exclusive) */
    int32_t sample_bounds[4];  /* Film::GetSampleBounds() */
    float filter_radius[2];
    float filter_table[256];   /* 16x16, Film ctor */
    float scale;
    float max_sample_luminance;
} mi_film;

/* ---- samplers. HALTON (src/samplers/halton.cpp:65-127) and SOBOL (src/samplers/sobol.cpp, lowdiscrepancy.h:229-274) are
 * global samplers: sample (pixel, n) is a pure function of its index, so a parallel render reproduces the reference sample
 * for sample. RANDOM (src/samplers/random.cpp:42-60) draws from one PCG32 stream per film tile in the reference, in the order
 * its thread happens to consume them -- the count per sample depends on the path -- which no parallel schedule can
 * reproduce; here every camera sample owns a PCG32 stream of its own (sequence number = n * pixel count of the sample bounds +
 * pixel index, rng.h:98-105: distinct for every pixel and sample number, also when a pass renders sample numbers beyond
 * samples_per_pixel), consumed in the reference's order: the same estimator on other random numbers. */
/* ZEROTWO ("02sequence" / "lowdiscrepancy", src/samplers/zerotwosequence.cpp:53-69) and STRATIFIED (src/samplers/stratified.cpp:43-71)
 * are PixelSamplers (src/core/sampler.cpp:100-135): at StartPixel they tabulate, for each of `pixel_dims` sampled dimensions, one
 * 1D and one 2D value per sample of the pixel -- randomly scrambled / jittered and shuffled with the sampler's RNG -- and a
 * sample's Get1D / Get2D calls read the next 1D / 2D table until the tables run out, then fall back to that RNG. In the
 * reference the RNG is one stream per film tile, carried through its pixels and samples in the order the thread consumes it
 * (a count that depends on the paths). The convention here, identical on device and oracle, as for RANDOM: the tables of pixel
 * p come from a PCG32 stream of their own (sequence number = pixel index of the sample bounds), generated in the reference's
 * order (all 1D tables, then all 2D tables); the fall-back draws of sample n of pixel p come from the stream
 * (n + 1) * pixel count + pixel index. Same estimator, same stratification, other random numbers. */
typedef enum mi_sampler_type { MI_SAMPLER_HALTON = 0, MI_SAMPLER_SOBOL = 1, MI_SAMPLER_RANDOM = 2, MI_SAMPLER_ZEROTWO = 3, MI_SAMPLER_STRATIFIED = 4 } mi_sampler_type;
#define MI_SOBOL_MATRIX_SIZE 52 /* SobolMatrixSize, src/core/sobolmatrices.h:48 */
typedef struct mi_sampler {
    int64_t samples_per_pixel; /* SOBOL: rounded up to a power of two (sobol.h:52) */
    int32_t base_scales[2], base_exponents[2];
    int32_t sample_stride;
    int32_t mult_inverse[2];
    int32_t sample_at_pixel_center;
    int32_t n_dims;            /* dimensions with tables below */
    const int32_t *primes;     /* [n_dims] (also the bases of the spatial light distribution's probes, whatever the sampler) */
    const int32_t *prime_sums; /* [n_dims] offset of each base's permutation */
    const uint16_t *perms;     /* [n_perms] ComputeRadicalInversePermutations prefix */
    uint32_t n_perms;
    /* ABI v6 */
    int32_t type;              /* mi_sampler_type */
    int32_t sobol_resolution, sobol_log2_resolution; /* RoundUpPow2(max extent of the sample bounds), its log2 */
    int32_t n_sobol_dims;
    const uint32_t *sobol_matrices; /* [n_sobol_dims * 52] SobolMatrices32 */
    const uint64_t *sobol_vdc;      /* [52] VdCSobolMatrices[log2_resolution - 1] */
    const uint64_t *sobol_vdc_inv;  /* [52] VdCSobolMatricesInv[log2_resolution - 1] */
    /* ABI v9: the pixel samplers */
    int32_t pixel_dims;             /* ZEROTWO / STRATIFIED: nSampledDimensions ("integer dimensions", default 4) */
    int32_t x_samples, y_samples;   /* STRATIFIED: samples_per_pixel = x_samples * y_samples */
    int32_t jitter;                 /* STRATIFIED: "bool jitter" */
} mi_sampler;

typedef struct mi_integrator {
    int32_t max_depth;        /* CreatePathIntegrator, src/integrators/path.cpp:193 */
    float rr_threshold;
    int32_t pixel_bounds[4];  /* x0,y0,x1,y1 */
    int32_t n_ca_bands;       /* 1: Integrator "path". >1: Integrator "spectralpath" numCABands -- that many
                               * paths per camera sample on consecutive sampler dimensions, band s supplying
                               * spectrum bins [round(31/n)*s, min(round(31/n)*(s+1), 31))
                               * (src/integrators/spectralpath.cpp:258-318, 366) */
    /* ABI v11 -- Integrator "metadata" (src/integrators/metadata.cpp:52-111): one closest-hit query per camera sample, the
     * answer written into every bin of the sample's spectrum. mi_pt_render renders radiance whatever `kind` says; the maps
     * are rendered by mi_pt_render_metadata. */
    int32_t kind;              /* mi_integrator_kind */
    int32_t metadata_strategy; /* mi_metadata_strategy: the scene file's "string strategy" */
} mi_integrator;
typedef enum mi_integrator_kind { MI_INTEGRATOR_PATH = 0 /* "path" / "spectralpath" */, MI_INTEGRATOR_METADATA = 1 } mi_integrator_kind;
typedef enum mi_metadata_strategy {
    MI_METADATA_DEPTH = 0,      /* all bins: (isect.p - ray.o).Length(), metadata.cpp:62-66 */
    MI_METADATA_MATERIAL = 1,   /* all bins: isect.materialId */
    MI_METADATA_MESH = 2,       /* all bins: isect.instanceId */
    MI_METADATA_COORDINATES = 3 /* bins 0, 1, 2: isect.p.x, .y, .z (world); the other bins 0 */
} mi_metadata_strategy;

/* ABI v11 -- the identifiers the reference's SurfaceInteraction carries, one entry per mi_prim (parallel to
 * mi_scene_desc.prims; mi_prim itself stays 16 bytes). material_id: the construction number of the primitive's Material
 * object (material.h:54: the counter starts at 1; in a `pbrt scene.pbrt` process the scene's default matte is number 2);
 * 0 for a primitive without a material (the reference dereferences a null pointer there, primitive.cpp:125).
 * instance_id: the 1-based number of the ObjectInstance call the primitive was created by (api.cpp:1589-1614,
 * primitive.cpp:89), 0 outside instances -- and 0 in every entry of a scene whose instances are TransformedPrimitives
 * (mi_instance): there the id is the instance's own (mi_instance.instance_id; without one and without a motion record, the
 * hit's instance + 1). */
typedef struct mi_prim_meta {
    uint32_t material_id, instance_id;
} mi_prim_meta;

typedef struct mi_scene_desc {
    uint32_t abi_version; /* MI_ABI_VERSION */
    uint32_t n_nodes;  const mi_bvh_node *nodes;
    uint32_t n_prims;  const mi_prim *prims;
    uint32_t n_tris;   const int32_t *tri_indices; /* 3 per triangle, global vertex ids */
                       const uint32_t *tri_mesh;   /* mesh id per triangle */
    uint32_t n_verts;  const float *P;  /* 3 per vertex, world space */
                       const float *N;  /* 3 per vertex, world space (0 when mesh has none) */
                       const float *UV; /* 2 per vertex */
    uint32_t n_meshes; const mi_mesh *meshes;
    uint32_t n_spheres; const mi_sphere *spheres;
    uint32_t n_materials; const mi_material *materials;
    uint32_t n_lights; const mi_light *lights;
    mi_lightdistrib light_distrib;
    mi_camera camera;
    mi_film film;
    mi_sampler sampler;
    mi_integrator integrator;
    float cie_y[MI_NSPEC]; /* SampledSpectrum::Y, for y() guards */
    uint32_t n_envmaps; const mi_envmap *envmaps;
    float rgb_illum[7][MI_NSPEC]; /* rgbIllum2Spect{White,Cyan,Magenta,Yellow,Red,Green,Blue} (spectrum.h:322-398) */
    uint32_t n_textures; const mi_texture *textures;   /* ABI v5 */
    uint32_t n_mipmaps;  const mi_mipmap *mipmaps;
    uint32_t n_instances; const mi_instance *instances; /* ABI v7 */
    const mi_prim_meta *prim_meta; /* ABI v11: [n_prims], may be NULL (then mi_pt_render_metadata refuses) */
    int32_t camera_type;           /* ABI v13: mi_camera_type of `camera` */
    const mi_lens *lens;           /* ABI v13: MI_CAMERA_REALISTIC: the lens system; NULL for a perspective camera */
    uint32_t n_disks; const mi_disk *disks; /* ABI v14: quadric indices [n_spheres, n_spheres + n_disks) */
    uint32_t n_motions; const mi_motion *motions; /* object motion: the records mi_instance.motion points into */
    /* MI_CAMERA_ENVIRONMENT (appended under an unchanged ABI number; read for that camera type only): "ipd" (0),
     * "poleMergeAngleTo" (90), "poleMergeAngleFrom" (90) -- compared as given against an altitude in radians, as the
     * reference does -- and "convergencedistance" (Infinity: parallel convergence) */
    float env_ipd, env_pole_merge_to, env_pole_merge_from, env_convergence_distance;
} mi_scene_desc;

/* Counters with the reference's STAT names (src/core/integrator.cpp:48,
 * src/core/scene.cpp:40-42, src/integrators/path.cpp:45-46). */
typedef struct mi_counters {
    uint64_t camera_rays;
    uint64_t regular_rays; /* Scene::Intersect calls */
    uint64_t shadow_rays;  /* Scene::IntersectP calls */
    uint64_t total_paths;  /* direct-lighting estimates */
    uint64_t zero_radiance_paths;
    uint64_t path_length_sum;
    uint64_t bvh_nodes_visited; /* build's own traversal, for B_ray */
    uint64_t tri_tests;
    uint64_t bad_samples;  /* NaN / negative / inf guards, integrator.cpp:295-316 */
    uint64_t iterations;   /* wavefront iterations of the last render */
    uint64_t extend_rays, extend_nodes, extend_tri_tests; /* closest-hit (extend) kernel only */
    uint64_t launches[3];  /* kernel launches of the last render: extend, shade, shadow */
} mi_counters;

#define MI_RENDER_FILM_ON_DEVICE 1u /* film_sum / weight_sum are device pointers */
#define MI_RENDER_ACCUMULATE 2u     /* do not clear the device film first */
typedef struct mi_render_params {
    int32_t shard_index, shard_count; /* 16x16 tiles with (tile_id % shard_count == shard_index) */
    uint32_t flags;
    uint32_t path_pool;   /* resident path slots; 0 = default */
    int64_t spp_override; /* 0 = use sampler.samples_per_pixel */
    int64_t sample_begin; /* first Halton sample number of this pass (0 = from the start);
                             a pass renders sample numbers [sample_begin, sample_begin + spp).
                             sample_begin >= 0 and sample_begin + spp <= 2^31 - 1 (a path keeps its sample number
                             in an int); mi_pt_render refuses other values with MI_ERR_INVALID */
    void *stream;         /* hipStream_t or NULL */
} mi_render_params;

typedef struct mi_pt mi_pt;

/* Create a renderer on HIP device `device_ordinal` and upload the scene. */
int mi_pt_create(const mi_scene_desc *scene, int device_ordinal, mi_pt **out);
/* Render. film_sum: [H*W*31] floats, pixel-major (pixel p, bin c at p*31+c) over
 * the cropped pixel bounds = Film::Pixel::L (sum of L*w*filterWeight, NOT
 * normalised, src/core/film.cpp:124-142); weight_sum: [H*W] = filterWeightSum.
 * Either may be NULL. Blocks until done. */
int mi_pt_render(mi_pt *pt, const mi_render_params *params, float *film_sum,
                 float *weight_sum, mi_counters *counters);
/* Integrator "metadata" (src/integrators/metadata.cpp:52-89 inside SamplerIntegrator::Render, integrator.cpp:277-323): one
 * closest-hit query per camera sample of the pass, its answer by `strategy` (mi_metadata_strategy) in the sample's spectrum,
 * which then passes the same guards (a NaN, y() < -1e-5 or an infinite y() blackens the sample and counts as bad; a
 * `coordinates` sample at negative x, y or z is not one of them: SampledSpectrum::y() clamps its weighted sum at 0,
 * spectrum.h:418, so the sample keeps its value, as in the reference) and the same filter as a radiance sample. A miss is
 * L = 0. Film buffers, flags, shards, sample ranges, pool size and stream as in mi_pt_render; the strategy is an argument of
 * the render, so one created renderer serves the radiance render and all four maps (mi_scene_desc.prim_meta goes to the
 * device at the first call). Counters: camera_rays = regular_rays = samples; shadow_rays, total_paths,
 * zero_radiance_paths, path_length_sum = 0; bad_samples = samples the guards blackened. Not with "spectralpath" bands:
 * the pass traces one ray per camera sample. */
int mi_pt_render_metadata(mi_pt *pt, const mi_render_params *params, int strategy, float *film_sum, float *weight_sum,
                          mi_counters *counters);
/* Device pointer of the resident film (layout [H*W][32]: 31 bins + weight) so a
 * collective can reduce in place; element count returned through n_floats. */
int mi_pt_device_film(mi_pt *pt, void **dev_ptr, uint64_t *n_floats);
/* Seconds of the last mi_pt_render: [0] = wall time of the whole render loop; then, from
 * HIP events recorded on the stream each launch goes to, the sum over launches per kernel
 * class: [1]=generate, [2]=extend (closest-hit traversal + its resolve), [3]=shade,
 * [4]=shadow, [5]=mis, [6]=closest-hit traversal kernel alone. The sub-renderers of one
 * render run concurrently, so [1..6] add up to more than [0]. */
int mi_pt_last_timings(mi_pt *pt, double *seconds, int n);
/* The path pool the last render ran on (summed over the renderer's sub-renderers): resident path slots and the device bytes
 * behind them. mi_render_params.path_pool = 0 asks for the default (one slot per camera sample of the shard, 4M .. 96M), which
 * takes at most 65 % of the free device memory and falls back to half, a quarter, ... if the allocation fails: this says what
 * was had. */
int mi_pt_pool_info(mi_pt *pt, uint64_t *slots, uint64_t *bytes);
/* The k_shade launches of the last render and the blocks they covered, summed over the sub-renderers (host-side counts).
 * A render sizes each launch by the shading queues it serves (mi_pt_shade_grid) and skips an instance whose queues are
 * empty; with MIPT_SHADE_GRID=pool in the environment every instance of the plan is launched on pool / 256 + 16 blocks in
 * every iteration. A metadata pass launches none. */
int mi_pt_shade_launch_stats(mi_pt *pt, uint64_t *launches, uint64_t *blocks);
/* The dark MIS rays of the last render, summed over the sub-renderers: BSDF-sampled rays that cannot reach the sampled light,
 * traced and counted because the reference does so, read by nothing. Where the live MIS rays are visibility queries (no
 * object instances, no alpha mask on an emitter's mesh) k_shade lists them in a queue of their own and a traversal launch
 * of their own walks it, beside the next iteration on a second stream (MIPT_DARK_STREAM=0 in the environment, read at
 * every render: in line after the live MIS stage). launches: those launches (host-side count); entries: what they found in
 * the queue; rays: what they traced (= entries); resolve_skipped: dark entries that the resolve kernel of the MIS queue
 * met and skipped -- 0 for such a scene, the dark rays of the others, which keep one queue and launch nothing here. */
int mi_pt_dark_launch_stats(mi_pt *pt, uint64_t *launches, uint64_t *entries, uint64_t *rays, uint64_t *resolve_skipped);
/* The traversal stacks of the last render or mi_pt_trace_wavefront call, summed over the sub-renderers and over every k_trav
 * launch of it: out[0] = the entries pushed in all, out[1] = those of them stored beyond the part of a lane's stack that
 * lives in LDS (MIPT_STACK_LDS entries, 12 by default), i.e. in private memory. A wide-4 record's children are pushed by
 * visiting rank while a lane stays inside the LDS part and one after the other once it leaves it; out[1] > 0 says that
 * rays of the call took the second way. mi_pt_trace_wavefront runs on the first sub-renderer and clears the counts of the
 * others, so after it the sums are that call's alone. */
int mi_pt_trav_stack_stats(mi_pt *pt, uint64_t out[2]);
void mi_pt_destroy(mi_pt *pt);
const char *mi_pt_last_error(void);

/* ---- Traversal-only entry point (parity of the BVH2 kernel on
 * recorded rays). rays: n x {o[3], d[3], tMax} floats (7 per ray);
 * hits: n x {prim (int32 as float bits), t, b0, b1} ; any_hit!=0 -> IntersectP
 * semantics (prim = 0/-1 only). Host pointers. */
int mi_pt_trace(mi_pt *pt, const float *rays, uint32_t n, int any_hit, float *hits);
/* The same with a time per ray: n x {o[3], d[3], tMax, time} (8 floats). The time decides the transform of a moving
 * instance (mi_motion); mi_pt_trace's rays take the shutter-open time. */
int mi_pt_trace_timed(mi_pt *pt, const float *rays, uint32_t n, int any_hit, float *hits);

/* The same question answered by the kernels a render launches (mi_pt_trace runs a plain per-ray routine, k_trace): ray i is
 * loaded into slot i of a path pool and a work list as the pipeline leaves it, traversed by the persistent wavefront kernel
 * of its class (batched state machine, cooperative leaf test, postponed quadrics, instance return entries) and committed by
 * that class's resolve step. Restates BVHAccel::Intersect / IntersectP (src/accelerators/bvh.cpp:662-738).
 *   mode 0: path rays -- k_trav<0>, k_resolve_extend, k_resolve_overflow; closest hit, tMax as given.
 *   mode 1: NEE shadow rays -- k_trav<1>, k_resolve_shadow, k_resolve_overflow; any hit (prim = 0 / -1); d is the
 *           unnormalised vector to the light sample and tMax must be 1 - 0.0001f (Interaction::SpawnRayTo).
 *   mode 2: BSDF-sampled MIS rays -- k_trav<2>, then the quadric step of k_resolve_mis (the same device function; that
 *           kernel consumes the hit in place); closest hit, tMax must be +infinity (Interaction::SpawnRay). (A render of a
 *           scene without instances (and without an alpha mask on an emitter's own mesh) asks these rays as visibility queries bounded by the sampled emitter,
 *           k_trav<3>, and falls back to this closest-hit form for the rays that does not settle; this call always runs
 *           the closest-hit kernel.)
 *   mode 3: the same rays as the visibility queries a render asks (k_trav<3>; only for scenes without instances and
 *           without an alpha mask on an emitter's own mesh): tMax is the end of the span in which the sampled emitter could be hit, the span starts at
 *           tMax (1 - 2^-8), no primitive is left out. hits[4i]: a primitive accepted in front of the span (any one: the
 *           kernel stops at the first), -1 if nothing was accepted up to tMax, -2 if something was accepted only inside the
 *           span (a render traces such a ray again in the reference's order); postponed quadrics are reported, not tested.
 * hits: as mi_pt_trace. extra (may be NULL): n x 4 words {b2 (float), instance of the hit (int32 bits, -1 = none),
 * the count of postponed quadrics as the traversal kernel left it (int32 bits: count | 0x100 on overflow),
 * the hit primitive as the traversal kernel left it, before the quadric step (int32 bits; -2 = the ray was never answered;
 * mode 1, whose kernel keeps one answer word per queue entry: 0 = occluded, -1 = not)}. Host pointers; n <= 2^24. */
int mi_pt_trace_wavefront(mi_pt *pt, const float *rays, uint32_t n, int mode, float *hits, float *extra);
/* The same with a time per ray (8 floats per ray, as mi_pt_trace_timed): it goes into the pool's time plane, where the
 * render's kernels read it. mi_pt_trace_wavefront's rays take the shutter-open time. */
int mi_pt_trace_wavefront_timed(mi_pt *pt, const float *rays, uint32_t n, int mode, float *hits, float *extra);

/* Parity tool for the camera: sample i = {px, py, sample number} (three int32) goes through the device functions k_generate
 * calls -- CameraSampleDims, then CameraRay -- and out receives 8 floats per sample: o[3], d[3], tMax, time. (time is
 * shutter_open for a camera that does not move: such a camera's time sample is never evaluated.) For a realistic camera
 * the ray is the lens camera's at 550 nm and time is the ray's time; a sample that does not get through the lens (weight 0)
 * has o, d and tMax all 0, which this layout cannot tell from a ray -- ask mi_pt_camera_rays_ex for the weight.
 * Host pointers; n <= 2^24. */
int mi_pt_camera_rays(mi_pt *pt, const int32_t *samples, uint32_t n, float *out);
/* The same for every camera, with what a realistic camera adds: band s of Integrator "spectralpath" generates its ray at
 * wavelength 395 + D s + D / 2 nm, D = 10 * round(31 / n_ca_bands) (spectralpath.cpp:234-267 with sampledLambdaStart = 395 and
 * (705 - 395) / 31 = 10 nm per bin, spectrum.h:48-50); band must be 0 for other
 * integrators (550 nm). out receives MI_CAMERA_RAY_EX_FLOATS floats per sample: o[3], d[3], tMax, time (here always
 * Lerp(time sample, shutter_open, shutter_close), whether or not the camera moves), the ray weight
 * (Camera::GenerateRayDifferential's return value, camera.cpp:60-99: 0 when the main ray, or both signs of an offset ray, do
 * not get through the lens; then the other fields are unspecified), and the four differential vectors rxOrigin, ryOrigin,
 * rxDirection, ryDirection after ScaleDifferentials(1 / sqrt(samples per pixel)). Runs the device functions k_generate runs. */
#define MI_CAMERA_RAY_EX_FLOATS 21
int mi_pt_camera_rays_ex(mi_pt *pt, const int32_t *samples, uint32_t n, int32_t band, float *out);

/* Parity tool for the scalar helpers under the shape and sampling code, each run on the device for n inputs (x, y: 2 floats per
 * element; out: 3 floats per element) -- the reference's own tests of them are restated over this entry point and the oracle's:
 *   op 0: NextFloatUp(x0), NextFloatDown(x0)                     pbrt.h:244-268  (OffsetRayOrigin; tests/fp_tests.cpp:29-47)
 *   op 1..4: EFloat(x0, err x1) {+, -, *, /} EFloat(y0, err y1)  efloat.h:48-200 (Sphere::Intersect; tests/fp_tests.cpp:166-260)
 *            -> value, lower bound, upper bound
 *   op 5: FindInterval over the array 0, 1, ..., 9 with the predicate a[i] <= x0, as Distribution1D::SampleDiscrete runs it
 *         (pbrt.h:405-418, sampling.h:91-98; tests/find_interval.cpp:8) -> the interval
 *   op 6: x0 / y0 the two ways the spectral passes divide: DivBy(x0, MakeDivisor(y0)), DivFast(x0, y0, 1 / y0, tracker) with
 *         a tracker reset for this divisor alone, and 1 where that tracker reports a quotient outside the fast range
 * Host pointers; needs no scene. */
int mi_pt_math_probe(int device_ordinal, int op, uint32_t n, const float *x, const float *y, float *out);

/* Parity tool for image textures: MIPMap<RGBSpectrum>::Lookup(st, dstdx, dstdy) (src/core/mipmap.h:281-319) of texture
 * `tex` for n queries on the device. queries: 6 floats each (s, t, dsdx, dtdx, dsdy, dtdy) in texture space, i.e. after
 * the UVMapping2D; rgb: 3 floats per query. */
int mi_pt_texture_lookup(mi_pt *pt, int32_t tex, uint32_t n, const float *queries, float *rgb);

/* Parity tool for the noise textures: Texture<Float>::Evaluate(si) of noise texture `tex` (MI_TEX_FBM / WRINKLED / WINDY) for n
 * queries, through the device functions k_shade calls. queries: 9 floats each -- the interaction's world p, dpdx, dpdy; out: 1
 * float per query, the value times post_scale (no material clamp). MI_ERR_INVALID for any other texture type
 * (mi_pt_texture_lookup answers for image textures). Host pointers. */
int mi_pt_texture_probe(mi_pt *pt, int32_t tex, uint32_t n, const float *queries, float *out);

/* Parity tool for every texture record, the opt-in mappings and classes among them: texture `tex` at n interactions, through
 * the device functions k_shade calls. queries: MI_TEXTURE_EVAL_QUERY_FLOATS floats each -- p[3], dpdx[3], dpdy[3], u, v, dudx,
 * dvdx, dudy, dvdy. n <= 2^24. Host pointers.
 *   mode 0: TextureMapping2D::Map -> 6 floats per query: s, t, dsdx, dtdx, dsdy, dtdy. MI_ERR_INVALID for a record without a 2-D
 *           mapping (the noise textures, MI_TEX_CHECKERBOARD3D).
 *   mode 1: Texture::Evaluate -> MI_NSPEC floats per query. A spectrum record gives its bins, formed as k_shade forms them (the
 *           material's Clamp() included); a float record (is_float) gives its value times post_scale in bin 0 and 0 elsewhere. */
#define MI_TEXTURE_EVAL_QUERY_FLOATS 15
int mi_pt_texture_eval_probe(mi_pt *pt, int32_t tex, int32_t mode, uint32_t n, const float *queries, float *out);

/* Parity tool for the quadrics (ABI v14): quadric `quadric` of the scene (the index space of mi_prim.shape: spheres, then
 * disks) on its own, through the device functions the traversal, shading and light-sampling code call. Host pointers.
 *   mode 0: Shape::Intersect. queries: 7 floats (o[3], d[3], tMax); out: MI_SHAPE_PROBE_HIT_FLOATS floats -- hit, t, p[3],
 *           n[3], uv[2], dpdu[3], dpdv[3] (world space; all 0 on a miss). hit is 1 for a hit, 0 for a miss, and -1 when the
 *           any-hit form of the test (Shape::IntersectP) disagrees with it.
 *   mode 1: Shape::Sample(ref, u). queries: 5 floats (ref[3], u[2]); out: MI_SHAPE_PROBE_SAMPLE_FLOATS floats -- p[3], n[3], pdf
 *           (solid angle).
 *   mode 2: Shape::Pdf(ref, wi). queries: 6 floats (ref[3], wi[3]); out: 1 float.
 * The reference point is a bare one as Shape::SolidAngle builds it (shape.cpp:90-91): no normal, no error bound. */
#define MI_SHAPE_PROBE_HIT_FLOATS 16
#define MI_SHAPE_PROBE_SAMPLE_FLOATS 7
int mi_pt_shape_probe(mi_pt *pt, int32_t quadric, int32_t mode, uint32_t n, const float *queries, float *out);

/* Parity tool for the lights (ABI v15): light `light` of the scene on its own, through the device functions the shading kernel
 * calls for a next-event estimate and for the MIS weight of a BSDF sample. Host pointers. The reference point is built as
 * Shape::SolidAngle builds one (no error bound, wo = +z) with the normal of the query; a zero normal is a bare point.
 *   mode 0: Light::Sample_Li(ref, u). queries: 8 floats (ref.p[3], ref.n[3], u[2]); out: MI_LIGHT_PROBE_SAMPLE_FLOATS floats --
 *           wi[3], pdf, pLight.p[3], pLight.n[3] (zero for every light but an area light), Li[MI_NSPEC]. Where Sample_Li
 *           returns before it has a direction (pdf == 0 on an area light; mapPdf == 0 on the infinite light) all are 0; where
 *           the sample is black (a one-sided emitter seen from behind; a projection light seen from behind it or from outside
 *           its frustum) the Li bins are 0.
 *   mode 1: Light::Pdf_Li(ref, wi). queries: 9 floats (ref.p[3], ref.n[3], wi[3]); out: 1 float. 0 for the delta lights (point,
 *           distant, spot, projection),
 *           Shape::Pdf(ref, wi) for an area light, InfiniteAreaLight::Pdf_Li for the infinite light.
 *   mode 2: Light::Le(ray) of the infinite light -- queries: 3 floats (ray.d) -- and DiffuseAreaLight::L(n, w) of an area
 *           light -- queries: 6 floats (n[3], w[3]); out: MI_NSPEC floats. MI_ERR_INVALID for the delta lights. */
#define MI_LIGHT_PROBE_SAMPLE_FLOATS (10 + MI_NSPEC)
int mi_pt_light_probe(mi_pt *pt, int32_t light, int32_t mode, uint32_t n, const float *queries, float *out);

/* Parity tool for the Halton sampler's device routines: the scrambled radical inverse of `indices[i]` in `group` consecutive
 * dimensions from `first_dims[i]` on, through the routines the shading kernel calls. Host pointers.
 *   group 5, 2, 1: the grouped routines (five dimensions of the direct-lighting estimate, two of the next direction, one of the
 *                  roulette draw), which read the per-dimension records built at create and take 32-bit indices;
 *   group 0:       the single-dimension routine with its 64-bit digit loop (one value per query, any index).
 * out: max(group, 1) floats per query. MI_ERR_INVALID for a dimension below 2 or a group that ends beyond the sampler's tables
 * (mi_sampler.n_dims), and for an index beyond 32 bits with a group other than 0. Neighbouring queries share a wave. */
int mi_pt_sampler_probe(mi_pt *pt, int32_t group, uint32_t n, const uint64_t *indices, const int32_t *first_dims, float *out);

/* Parity tool for the BSDF code: material `material` of the scene through the BSDF routines of shading-kernel instance `instance`
 * (an index into the table mi_pt_shade_instances reports), one query at a time. Host pointers. The frame is the canonical one
 * (ns = ng = +z, ss = +x, ts = +y), every lobe of the material is on and nothing is overridden: what the kernel has at a
 * material without image textures. queries: 8 floats each -- wo[3], wi[3], u[2] (world = local directions).
 *   mode 0: BSDF::f(wo, wi, flags) and BSDF::Pdf(wo, wi, flags); u is not read.
 *   mode 1: BSDF::Sample_f(wo, u, flags); the query's wi is not read.
 * out: MI_BSDF_PROBE_FLOATS floats per query -- f[MI_NSPEC], pdf, wi[3] (mode 0: the query's), the sampled type (mode 0: 0); all
 * zero where Sample_f returns a black value. `form` is the code path that forms the 31 bins:
 *   0: the lobe list (BSDF_f / BSDF_Sample_f) summed bin by bin (EvalBin) -- the definition;
 *   1: the same list four bins at a time (EvalQuad);
 *   2: the straight-line form of the instances with at most two lobes of the simple kinds, with its retry where a quotient leaves
 *      the fast range. out has MI_BSDF_PROBE_STRAIGHT_FLOATS floats per query for this form: the record, then 1 if some quad of
 *      the query's wave (the 64 queries 64 w .. 64 w + 63) took the retry, then 1 if a quotient of this query left the range;
 *   3: summed lobe by lobe (AccumulateF; mode 1: AccumulateSpecular / AccumulateFLocal) -- the instances with more than two
 *      lobes or image textures.
 * MI_ERR_INVALID for a form the instance does not compile (mi_pt_bsdf_probe_forms), a material that reads an image texture (a
 * lobe's spectrum, the roughness, sigma or a bump map) or has more lobes than the instance holds, and an index out of range. A
 * lobe or Fresnel kind outside the instance's mask evaluates to nothing, as in the kernel: the caller picks instances that
 * hold the material's kinds. */
#define MI_BSDF_PROBE_FLOATS (5 + MI_NSPEC)
#define MI_BSDF_PROBE_STRAIGHT_FLOATS (MI_BSDF_PROBE_FLOATS + 2)
int mi_pt_bsdf_probe(mi_pt *pt, int32_t material, int32_t instance, int32_t mode, int32_t form, int32_t flags, uint32_t n,
                     const float *queries, float *out);
/* The forms of mi_pt_bsdf_probe that instance `instance` compiles (bit f: form f). The probe is compiled once per lobe count and
 * set of BSDF bits of the instances' masks; MI_ERR_INVALID for an instance that none of those covers. Touches no device. */
int mi_pt_bsdf_probe_forms(int32_t instance, uint32_t *forms);

/* Parity tool for the spatial light-selection strategy: the per-voxel Distribution1D tables mi_pt_create estimated on
 * the device (SpatialLightDistribution::ComputeDistribution, src/core/lightdistrib.cpp:232-300; the reference fills its
 * hash table lazily, this build tabulates every voxel). Voxel (x, y, z) has index (z * n_voxels[1] + y) * n_voxels[0] + x.
 * func: [n_voxels * n_lights] floats (Distribution1D::func of voxel v at v * n_lights), func_int: [n_voxels]
 * (Distribution1D::funcInt); either may be NULL. capacity_voxels must be >= the voxel count. MI_ERR_INVALID when the
 * scene does not use "lightsamplestrategy" "spatial" (or has no lights). Host pointers. */
int mi_pt_light_distribution(mi_pt *pt, float *func, float *func_int, uint64_t capacity_voxels);

/* ---- Parity tools for the shading plan: which instance of the shading kernel a material is shaded by. The kernel k_shade
 * exists once per (NL, TM): NL lobes at most, and a mask TM outside of which the BxDF, Fresnel, light, sampler, texture and
 * instance code is compiled out (bit t: mi_bxdf_type t; bit 16 + f: mi_fresnel_type f; bit 24 + l: mi_light_type l; the
 * other bits by name, mi_pt_shade_mask). mi_pt_create gives every material a shading class (one per distinct list of lobe
 * types, Fresnel kinds and texturedness, in order of first appearance; the 15th and later lists share class 14, which counts
 * MI_MAX_BXDFS lobes; class 15 is the escaped rays') and every class an instance. These three calls touch no device.
 *
 * The instance table in launch order: nl[i], tm[i] for i < *count; either array may be NULL, otherwise capacity >= *count. */
int mi_pt_shade_instances(int32_t *nl, uint32_t *tm, uint32_t capacity, uint32_t *count);
/* A mask by its name in the device code: "TM_DIFFUSE", "TM_PLASTIC", "TM_GLASS", "TM_UBER", "TM_DISNEY", "TM_GENERIC",
 * "TM_FULL", "TM_ALL" (what an instance is compiled for), "TM_SCALED", "TM_TEXTURED", "TM_INSTANCES", "TM_SAMPLERS",
 * "TM_LIGHTS_ALL", "TM_LIGHTS_NO_ENV" (single properties). MI_ERR_INVALID for another name. */
int mi_pt_shade_mask(const char *name, uint32_t *mask);
/* The grid of one k_shade launch: the blocks of 256 that the shading queues of the classes in `classes` (bit c: class c)
 * fill when each queue is padded to whole blocks on its own -- the sum over those classes of ceil(counts[c] / 256), which is
 * how the kernel maps a block index to (class, block of that queue). counts: the entries of the 16 queues, n_counts = 16
 * (MI_ERR_INVALID otherwise, and for a NULL argument). 0 blocks: the render does not launch the instance. */
int mi_pt_shade_grid(const uint32_t *counts, uint32_t n_counts, uint32_t classes, uint32_t *blocks);
/* The plan mi_pt_create would make for a description (the same routine computes both). material_class: [n_materials]
 * (capacity material_capacity). The classes in use, in rising order, the escaped rays' class last: class_id, the index of
 * its instance, its lobe count (the longest list of its materials) and its type word (the lobe and Fresnel bits present,
 * TM_SCALED if a lobe is a mix's, TM_TEXTURED if a material reads an image texture), each [class_capacity >= 16], *n_classes
 * of them. hot: the light and sampler bits of the scene's matte and plastic instances. Any output may be NULL. */
int mi_pt_shade_plan(const mi_scene_desc *scene, int32_t *material_class, uint32_t material_capacity, int32_t *class_id,
                     int32_t *class_instance, int32_t *class_lobes, uint32_t *class_types, uint32_t class_capacity,
                     uint32_t *n_classes, uint32_t *hot);

/* ---- HLBVH build on the device (Accelerator "bvh" "string splitmethod" "hlbvh"; BVHAccel::HLBVHBuild,
 * src/accelerators/bvh.cpp:404-638): Morton codes, stable radix sort, one LBVH treelet per run of equal top 12 bits
 * (emitLBVH), and the treelets flattened into the depth-first 32-byte node array. The SAH tree over the (at most 4096)
 * treelet roots (buildUpperSAH, bvh.cpp:534-638) is small serial host work: the caller supplies it as `upper`, which
 * receives the treelets' root bounds (6 floats each: min xyz, max xyz) and node counts and returns the upper interior
 * nodes (children given as final indices), their own final indices, the total node count and the final index of each
 * treelet's first node. prim_bounds: n x {min xyz, max xyz}; nodes_out: capacity nodes_capacity (2 n is always enough);
 * ordered_out: n primitive numbers in leaf order. The tree is the one the reference builds on one thread (leaves in
 * Morton order): the host restatement in libmipt_host.so builds the same nodes, bit for bit (mi_bvh_build_host; its
 * mi_bvh_upper_sah is the `upper` the front end passes, include/mi_scene.h). MI_ERR_UNSUPPORTED (message in
 * mi_bvh_last_error) when more than 65535 primitives share one Morton code: they would be one leaf, and a node's count has
 * 16 bits (the reference CHECKs that away, bvh.cpp:646). */
typedef int (*mi_bvh_upper_fn)(void *user, uint32_t n_treelets, const float *root_bounds, const int32_t *treelet_sizes,
                               mi_bvh_node *upper_nodes, int32_t *upper_index, uint32_t *n_upper, uint32_t *n_total,
                               int32_t *treelet_offset);
int mi_bvh_build_hlbvh(int device_ordinal, const float *prim_bounds, uint32_t n, int32_t max_prims_in_node, mi_bvh_upper_fn upper,
                       void *user, mi_bvh_node *nodes_out, uint32_t nodes_capacity, uint32_t *n_nodes, int32_t *ordered_out,
                       double *seconds);
const char *mi_bvh_last_error(void);

/* Parity tool: the state of ONE camera sample (pixel px, py; Halton sample number `sample`) vertex by vertex, for a
 * side-by-side comparison with the oracle's log of the same sample (oracle_path_log) when a film differs. One record of
 * MI_PATH_RECORD_FLOATS floats per path vertex (one wavefront iteration):
 *   [0] bounces  [1] hit primitive (-1: escaped)  [2] sampler dimension before the vertex  [3] 1 if the path ended here
 *   [4..6] incoming ray origin  [7] t of the hit  [8..10] incoming ray direction  [11] etaScale before
 *   [12..14] next ray origin  [15] sampler dimension after  [16..18] next ray direction  [19] etaScale after
 *   [20..50] beta after the vertex  [51..81] L after the vertex's direct lighting has been added
 * The device film is cleared by this call. */
#define MI_PATH_RECORD_FLOATS 96
int mi_pt_debug_path(mi_pt *pt, int32_t px, int32_t py, int64_t sample, int32_t max_records, float *records, int32_t *n_records);

#ifdef __cplusplus
}
#endif
#endif /* MI_PT_H */
