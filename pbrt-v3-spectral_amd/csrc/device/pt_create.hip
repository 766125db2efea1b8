// pt_create.hip -- mi_pt_create and mi_pt_destroy: the checks of a scene description, the tables the host derives from it
// (the wide BVH records, the shading plan), the uploads, the create-time launches and the render state; and the entry points
// that need no GPU (the shading plan and its instances, the error string). Host code only: the kernels it launches are in
// pt_kernels.hip (pt_select.h).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "pt_host.h"

namespace dptk {
thread_local std::string g_err;
}

// Four sub-renderer streams want four hardware queues of their own; the HIP runtime maps
// streams onto GPU_MAX_HW_QUEUES (default 4, shared with the null stream) when it
// initialises, which happens at the first HIP call -- after this library is loaded.
static struct QueueEnv { QueueEnv() { setenv("GPU_MAX_HW_QUEUES", "8", 0); } } g_queueEnv;

namespace {

// -----------------------------------------------------------------------------
// mi_pt_create, step 1: every refusal that depends on the description alone, before anything touches the device
// -----------------------------------------------------------------------------
// a float record of the classes beside the image and noise textures (EvalFloatImageTexture in the general instances): what a
// roughness, sigma or bump parameter may name besides those two
static bool FloatClassRecord(const mi_texture &t) {
    return t.is_float && (t.type == MI_TEX_CHECKERBOARD || t.type == MI_TEX_DOTS || t.type == MI_TEX_BILERP || t.type == MI_TEX_CHECKERBOARD3D);
}
int CheckSceneDesc(const mi_scene_desc *d) {
    if (d->n_prims && !d->n_nodes) { g_err = "primitives without BVH nodes"; return MI_ERR_INVALID; }
    for (uint32_t i = 0; i < d->n_nodes; ++i) {
        const mi_bvh_node &n = d->nodes[i];
        if (n.n_prims > 0) { if (n.offset < 0 || (uint32_t)n.offset + n.n_prims > d->n_prims) { g_err = "BVH leaf out of range"; return MI_ERR_INVALID; } }
        else if (n.offset <= (int)i || (uint32_t)n.offset >= d->n_nodes || i + 1 >= d->n_nodes) { g_err = "BVH child out of range"; return MI_ERR_INVALID; }
        if (n.n_prims > (unsigned)LEAF_COUNT_MASK) { g_err = "a BVH leaf holds more than 16383 primitives"; return MI_ERR_UNSUPPORTED; }
    }
    for (uint32_t i = 0; i < d->n_prims; ++i) {
        const mi_prim &p = d->prims[i];
        if (p.instance != 0) {
            if (p.instance < 0 || (uint32_t)p.instance > d->n_instances || !d->instances) { g_err = "primitive instance index out of range"; return MI_ERR_INVALID; }
            if (d->instances[p.instance - 1].root >= d->n_nodes) { g_err = "instance BVH root out of range"; return MI_ERR_INVALID; }
            continue;
        }
        if (p.shape >= 0 ? (uint32_t)p.shape >= d->n_tris : (uint64_t)(uint32_t)(~p.shape) >= (uint64_t)d->n_spheres + d->n_disks) { g_err = "primitive shape index out of range"; return MI_ERR_INVALID; }
        if (p.material >= (int)d->n_materials || p.area_light >= (int)d->n_lights) { g_err = "primitive material/light index out of range"; return MI_ERR_INVALID; }
    }
    if ((d->n_instances && !d->instances) || (d->n_motions && !d->motions)) { g_err = "instance or motion array missing"; return MI_ERR_INVALID; }
    for (uint32_t k = 0; k < d->n_instances; ++k)   // (every instance, referenced by a primitive or not)
        if (d->instances[k].motion > d->n_motions) { g_err = "instance motion index out of range"; return MI_ERR_INVALID; }
    if ((d->n_spheres && !d->spheres) || (d->n_disks && !d->disks) || (uint64_t)d->n_spheres + d->n_disks > 0x7fffffffull) { g_err = "quadric arrays missing or too large"; return MI_ERR_INVALID; }
    for (uint32_t i = 0; i < d->n_disks; ++i)
        if (d->disks[i].kind != MI_QUADRIC_DISK) { g_err = "mi_disk.kind: only disks (0) are built"; return MI_ERR_UNSUPPORTED; }
    for (uint32_t i = 0; i < d->n_tris * 3; ++i)
        if (d->tri_indices[i] < 0 || (uint32_t)d->tri_indices[i] >= d->n_verts) { g_err = "triangle vertex index out of range"; return MI_ERR_INVALID; }
    for (uint32_t i = 0; i < d->n_tris; ++i)
        if (d->tri_mesh[i] >= d->n_meshes) { g_err = "triangle mesh index out of range"; return MI_ERR_INVALID; }
    for (uint32_t i = 0; i < d->n_meshes; ++i)
        if (d->meshes[i].alpha_tex >= (int)d->n_textures || d->meshes[i].shadow_alpha_tex >= (int)d->n_textures) { g_err = "mi_mesh alpha texture index out of range"; return MI_ERR_INVALID; }
    for (uint32_t i = 0; i < d->n_materials; ++i) {
        const mi_material &m = d->materials[i];
        if (m.n_bxdfs < 0 || m.n_bxdfs > MI_MAX_BXDFS) { g_err = "material lobe count out of range"; return MI_ERR_INVALID; }
        if (m.bump_tex >= (int)d->n_textures || m.bump_tex < -1) { g_err = "mi_material.bump_tex out of range"; return MI_ERR_INVALID; }
        if (m.bump_tex >= 0 && d->textures[m.bump_tex].type == MI_TEX_UV) { g_err = "mi_material.bump_tex names a MI_TEX_UV record, which has no float value"; return MI_ERR_INVALID; }
        for (int k = 0; k < 2; ++k) {   // roughness maps: float image textures with a pyramid behind them, or noise textures (EvalFloatImageTexture)
            const int rt = m.rough_tex[k];
            if (rt < -1 || rt >= (int)d->n_textures) { g_err = "mi_material.rough_tex out of range"; return MI_ERR_INVALID; }
            if (rt >= 0 && !MI_TEX_IS_NOISE(d->textures[rt].type) && !FloatClassRecord(d->textures[rt]) && (d->textures[rt].type != MI_TEX_IMAGEMAP || (uint32_t)d->textures[rt].mipmap >= d->n_mipmaps)) {
                g_err = "mi_material.rough_tex must name an image texture with a mipmap or a noise texture"; return MI_ERR_INVALID;
            }
        }
        // (ABI v10) the sigma map, the lobe rules and the glass switch: what the shading kernels index with them
        if (m.sigma_tex < -1 || m.sigma_tex >= (int)d->n_textures ||
            (m.sigma_tex >= 0 && !MI_TEX_IS_NOISE(d->textures[m.sigma_tex].type) && !FloatClassRecord(d->textures[m.sigma_tex]) &&
             (d->textures[m.sigma_tex].type != MI_TEX_IMAGEMAP || (uint32_t)d->textures[m.sigma_tex].mipmap >= d->n_mipmaps))) {
            g_err = "mi_material.sigma_tex must be -1 or name an image texture with a mipmap or a noise texture"; return MI_ERR_INVALID;
        }
        for (int k = 0; k < m.n_bxdfs; ++k) {
            const mi_lobe_tex &lt = m.tex[k];
            if (lt.rule < MI_LOBE_IF_R || lt.rule > MI_LOBE_METAL) { g_err = "mi_lobe_tex.rule is not a mi_lobe_rule"; return MI_ERR_INVALID; }
            if (lt.tex_R < -1 || lt.tex_R >= (int)d->n_textures || lt.tex_S < -1 || lt.tex_S >= (int)d->n_textures) { g_err = "mi_lobe_tex texture index out of range"; return MI_ERR_INVALID; }
            for (int tx : {lt.tex_R, lt.tex_S})   // (it has no pyramid either: the spectrum evaluation would look one up)
                if (tx >= 0 && d->textures[tx].type == MI_TEX_BILERP) { g_err = "mi_lobe_tex names a MI_TEX_BILERP record, which has no spectrum value"; return MI_ERR_INVALID; }
            if (lt.rule >= MI_LOBE_DISNEY_SHEEN && lt.rule <= MI_LOBE_DISNEY_STRANS && lt.tex_R < 0) { g_err = "a \"disney\" lobe rule needs the colour's texture in tex_R"; return MI_ERR_INVALID; }
        }
        if ((m.rough_flags & MI_ROUGH_GLASS) && (m.n_bxdfs < 1 || m.bxdf[0].type != MI_BXDF_FRESNEL_SPECULAR)) {
            g_err = "MI_ROUGH_GLASS: lobe 0 must be the FresnelSpecular one"; return MI_ERR_INVALID;
        }
    }
    for (uint32_t i = 0; i < d->n_textures; ++i) {
        const mi_texture &t = d->textures[i];
        if (t.type < MI_TEX_IMAGEMAP || t.type > MI_TEX_CHECKERBOARD3D) { g_err = "mi_texture.type is not a mi_tex_type"; return MI_ERR_INVALID; }
        if (t.mapping < MI_MAP_UV || t.mapping > MI_MAP_PLANAR) { g_err = "mi_texture.mapping is not a mi_tex_mapping"; return MI_ERR_INVALID; }
        if (t.mapping != MI_MAP_UV && !MI_TEX_HAS_MAPPING2D(t.type)) { g_err = "mi_texture.mapping set on a record without a 2-D mapping"; return MI_ERR_INVALID; }
        if ((t.type == MI_TEX_UV && t.is_float) || (t.type == MI_TEX_BILERP && !t.is_float)) { g_err = "MI_TEX_UV is a spectrum record and MI_TEX_BILERP a float one"; return MI_ERR_INVALID; }
        if (t.type == MI_TEX_IMAGEMAP && (uint32_t)t.mipmap >= d->n_mipmaps) { g_err = "mi_texture.mipmap out of range"; return MI_ERR_INVALID; }
        // (the octave loops run per lane: bounded here as the front end bounds them)
        if (MI_TEX_IS_NOISE(t.type) && (t.octaves < 0 || t.octaves > MI_NOISE_MAX_OCTAVES)) { g_err = "mi_texture.octaves outside 0..32"; return MI_ERR_INVALID; }
    }
    // the traversal kernels hold no noise code, no other class and no mapping but UVMapping2D: a mask is an image texture under it
    for (uint32_t i = 0; i < d->n_meshes; ++i)
        for (int a : {d->meshes[i].alpha_tex, d->meshes[i].shadow_alpha_tex}) {
            if (a >= 0 && d->textures[a].type != MI_TEX_IMAGEMAP) { g_err = "mi_mesh alpha textures must be image textures"; return MI_ERR_INVALID; }
            if (a >= 0 && d->textures[a].mapping != MI_MAP_UV) { g_err = "mi_mesh alpha textures must be image textures under the uv mapping"; return MI_ERR_INVALID; }
        }
    for (uint32_t i = 0; i < d->n_mipmaps; ++i) {
        const mi_mipmap &m = d->mipmaps[i];
        if (m.n_levels < 1 || m.n_levels > MI_MAX_MIP_LEVELS || !m.texels || m.width < 1 || m.height < 1) { g_err = "malformed mi_mipmap"; return MI_ERR_INVALID; }
    }
    for (uint32_t i = 0; i < d->n_envmaps; ++i) {
        const mi_envmap &e = d->envmaps[i];
        // (a projection light's map is the image alone: nu = nv = 0 and no tables)
        const bool tables = e.cond_func && e.cond_cdf && e.cond_func_int && e.marg_func && e.marg_cdf;
        const bool noTables = !e.cond_func && !e.cond_cdf && !e.cond_func_int && !e.marg_func && !e.marg_cdf;
        if (e.width < 1 || e.height < 1 || !e.rgb || !((e.nu >= 1 && e.nv >= 1 && tables) || (e.nu == 0 && e.nv == 0 && noTables))) {
            g_err = "malformed mi_envmap"; return MI_ERR_INVALID;
        }
    }
    int nInfinite = 0;
    for (uint32_t i = 0; i < d->n_lights; ++i) {
        const mi_light &l = d->lights[i];
        if (l.type == MI_LIGHT_DIFFUSE_AREA && (l.shape >= 0 ? (uint32_t)l.shape >= d->n_tris : (uint64_t)(uint32_t)(~l.shape) >= (uint64_t)d->n_spheres + d->n_disks)) { g_err = "area light shape index out of range"; return MI_ERR_INVALID; }
        if (l.type < MI_LIGHT_DIFFUSE_AREA || l.type > MI_LIGHT_PROJECTION) { g_err = "mi_light.type is not a light type"; return MI_ERR_INVALID; }
        if (l.type == MI_LIGHT_PROJECTION && (l.proj_map < -1 || l.proj_map >= (int)d->n_envmaps)) { g_err = "mi_light.proj_map out of range"; return MI_ERR_INVALID; }
        if (l.type != MI_LIGHT_INFINITE) continue;
        if ((uint32_t)l.envmap >= d->n_envmaps || d->envmaps[l.envmap].nu < 1) { g_err = "infinite light without environment map"; return MI_ERR_INVALID; }
        if (++nInfinite > 4) { g_err = "more than 4 infinite lights"; return MI_ERR_INVALID; }
    }
    const mi_lightdistrib &ld = d->light_distrib;
    if (d->n_lights > 0 && ld.type != MI_LD_SPATIAL && (!ld.func || !ld.cdf || !ld.func_int)) { g_err = "light distribution tables missing"; return MI_ERR_INVALID; }
    if (d->n_lights > 0 && ld.type == MI_LD_SPATIAL) {
        const size_t nVox = (size_t)ld.n_voxels[0] * ld.n_voxels[1] * ld.n_voxels[2];
        if (nVox == 0 || nVox * d->n_lights > (1ull << 31)) { g_err = "spatial light distribution too large for the dense per-voxel table"; return MI_ERR_UNSUPPORTED; }
    }
    if (d->integrator.n_ca_bands < 1 || d->integrator.n_ca_bands > MI_NSPEC) { g_err = "n_ca_bands must be in [1, 31]"; return MI_ERR_INVALID; }
    if (d->camera_type < MI_CAMERA_PERSPECTIVE || d->camera_type > MI_CAMERA_ENVIRONMENT) { g_err = "unknown mi_scene_desc.camera_type"; return MI_ERR_INVALID; }
    if (d->camera_type == MI_CAMERA_REALISTIC) {
        const mi_lens *l = d->lens;
        if (!l || l->n_elements < 1 || l->n_elements > MI_MAX_LENS_ELEMENTS || l->full_res[0] < 1 || l->full_res[1] < 1 || !(l->film_diagonal > 0)) {
            g_err = "realistic camera: mi_scene_desc.lens missing or malformed (1 .. 32 elements, the film's resolution and diagonal)";
            return MI_ERR_INVALID;
        }
    }
    if (d->integrator.max_depth < 0 || d->integrator.max_depth > 255) { g_err = "max_depth must be in [0, 255] (a path's bounce count travels in 8 bits of its state word)"; return MI_ERR_UNSUPPORTED; }
    const mi_sampler &sm = d->sampler;
    if (sm.type < MI_SAMPLER_HALTON || sm.type > MI_SAMPLER_STRATIFIED) { g_err = "unknown mi_sampler.type"; return MI_ERR_INVALID; }
    if (sm.samples_per_pixel < 1) { g_err = "mi_sampler.samples_per_pixel must be positive"; return MI_ERR_INVALID; }
    if (sm.type >= MI_SAMPLER_ZEROTWO) {
        if (sm.pixel_dims < 0 || sm.pixel_dims > 64) { g_err = "mi_sampler.pixel_dims must be in [0, 64]"; return MI_ERR_INVALID; }
        if (sm.samples_per_pixel > (1 << 20)) { g_err = "pixel samplers tabulate every sample of a pixel: at most 2^20 samples per pixel"; return MI_ERR_UNSUPPORTED; }
        if (sm.type == MI_SAMPLER_STRATIFIED && (sm.x_samples < 1 || sm.y_samples < 1 || (int64_t)sm.x_samples * sm.y_samples != sm.samples_per_pixel)) {
            g_err = "stratified sampler: samples_per_pixel must be x_samples * y_samples"; return MI_ERR_INVALID;
        }
        if (sm.type == MI_SAMPLER_ZEROTWO && (sm.samples_per_pixel & (sm.samples_per_pixel - 1)) != 0) { g_err = "02sequence sampler: samples_per_pixel must be a power of two"; return MI_ERR_INVALID; }
    }
    if (sm.type == MI_SAMPLER_SOBOL) {
        if (!sm.sobol_matrices || !sm.sobol_vdc || !sm.sobol_vdc_inv || sm.sobol_log2_resolution < 0 ||
            sm.sobol_log2_resolution > 25 || sm.sobol_resolution != (1 << sm.sobol_log2_resolution)) { g_err = "malformed Sobol' sampler tables"; return MI_ERR_INVALID; }
        if (sm.n_sobol_dims < 6 + 8 * d->integrator.max_depth * d->integrator.n_ca_bands) {
            g_err = "Sobol' matrices cover too few dimensions for max_depth x n_ca_bands";
            return MI_ERR_INVALID;
        }
    }
    if (sm.n_dims < (sm.type == MI_SAMPLER_HALTON ? 6 + 8 * d->integrator.max_depth * d->integrator.n_ca_bands : 5)) {
        g_err = "Halton tables cover too few dimensions for max_depth x n_ca_bands (the reference's prime table ends at 1000)";
        return MI_ERR_INVALID;
    }
    if (d->film.cropped_bounds[2] - d->film.cropped_bounds[0] <= 0 || d->film.cropped_bounds[3] - d->film.cropped_bounds[1] <= 0) { g_err = "empty film"; return MI_ERR_INVALID; }
    return MI_OK;
}

// -----------------------------------------------------------------------------
// mi_pt_create, step 2: the tables the host derives from the checked description (no HIP calls)
// -----------------------------------------------------------------------------

// A leaf's count as the traversal records carry it: | LEAF_SIMPLE when the leaf holds triangles only (`coop`: unless
// MIPT_NO_COOP_LEAVES is set).
unsigned LeafMeta(const mi_scene_desc *d, const mi_bvh_node &leaf, bool coop) {
    bool simple = coop;
    for (uint32_t k = 0; k < leaf.n_prims && simple; ++k) {
        const mi_prim &p = d->prims[leaf.offset + k];
        simple = p.instance == 0 && p.shape >= 0;
    }
    return (unsigned)leaf.n_prims | (simple ? (unsigned)LEAF_SIMPLE : 0u);
}

struct BvhTables {
    int width = 4;                       // MIPT_BVH_WIDTH=2: one record per BVH2 interior node, i.e. the reference's own node-visit counts
    std::vector<float4> wnodes;          // the wide records (none: a wide-4 scene without nodes)
    std::vector<int32_t> instWideRoot;   // wide-4, per instance: the first record of its object's tree
    std::vector<float4> instRootBounds;  // ... and that tree's root box (min, max)
};

// The box of a wide-4 record's slot.
void SetWide4Box(float4 *rec, int slot, const mi_bvh_node &c) {
    float *f = (float *)rec + (slot < 2 ? 0 : 12) + (slot & 1) * 6;
    f[0] = c.bmin[0]; f[1] = c.bmin[1]; f[2] = c.bmin[2]; f[3] = c.bmax[0]; f[4] = c.bmax[1]; f[5] = c.bmax[2];
}

// The links, the counts and the eight octants' visit orders of a wide-4 record.
void FinishWide4Record(float4 *rec, const int link[4], const unsigned cnt[4], int axisRoot, const int groupN[2], const int groupAxis[2]) {
    memcpy(&rec[6], link, 16);
    const unsigned c01 = cnt[0] | (cnt[1] << 16), c23 = cnt[2] | (cnt[3] << 16);
    unsigned ord[2] = {0, 0};
    for (int oct = 0; oct < 8; ++oct) {
        auto neg = [&](int axis) { return ((oct >> axis) & 1) != 0; };
        int seq[4], n = 0;
        bool used[4] = {false, false, false, false};
        for (int pass = 0; pass < 2; ++pass) {
            const int g = (neg(axisRoot) ? 1 : 0) ^ pass;   // near child's group first (bvh.cpp:686-692)
            const int base = 2 * g;
            if (groupN[g] == 2) {
                const bool swap = neg(groupAxis[g]);
                seq[n++] = base + (swap ? 1 : 0);
                seq[n++] = base + (swap ? 0 : 1);
            } else if (groupN[g] == 1) seq[n++] = base;
        }
        for (int k = 0; k < n; ++k) used[seq[k]] = true;
        for (int sl = 0; sl < 4 && n < 4; ++sl) if (!used[sl]) seq[n++] = sl;   // absent slots last (never hit)
        unsigned perm = 0;
        for (int k = 0; k < 4; ++k) perm |= (unsigned)seq[k] << (2 * k);
        ord[oct >> 2] |= perm << (8 * (oct & 3));
    }
    memcpy(&rec[7].x, &c01, 4); memcpy(&rec[7].y, &c23, 4);
    memcpy(&rec[7].z, &ord[0], 4); memcpy(&rec[7].w, &ord[1], 4);
}

// Wide-4 records (OpenNode<4>): one per two-level subtree of the host's BVH2, in depth-first order. Slots 0/1 are the
// left child's children (slot 0 alone = the left child itself when it is a leaf), slots 2/3 the right child's. False,
// and `t` untouched, when a ray's stack could outgrow STACK_LDS + STACK_SPILL entries over them.
bool BuildWide4(const mi_scene_desc *d, bool coop, BvhTables &t) {
    const uint32_t nN = d->n_nodes;
    const mi_bvh_node *nodes = d->nodes;
    std::vector<int32_t> widx(nN, -1);
    std::vector<uint32_t> order;   // BVH2 roots of the records, in record order
    // the trees: the world's (root 0) and one per instanced object (mi_instance.root)
    std::vector<uint32_t> treeRoots(1, 0u);
    for (uint32_t k = 0; k < d->n_instances; ++k)
        if (std::find(treeRoots.begin(), treeRoots.end(), d->instances[k].root) == treeRoots.end()) treeRoots.push_back(d->instances[k].root);
    for (const uint32_t treeRoot : treeRoots) {
        if (nodes[treeRoot].n_prims > 0) {   // a single-leaf tree gets a record of its own: the leaf in slot 0
            widx[treeRoot] = (int32_t)order.size();
            order.push_back(treeRoot);
            continue;
        }
        std::vector<uint32_t> stack;
        stack.push_back(treeRoot);
        while (!stack.empty()) {
            const uint32_t i = stack.back();
            stack.pop_back();
            widx[i] = (int32_t)order.size();
            order.push_back(i);
            uint32_t sub[4];
            int nSub = 0;
            const uint32_t ch[2] = {i + 1, (uint32_t)nodes[i].offset};
            for (int c = 0; c < 2; ++c) {
                if (nodes[ch[c]].n_prims > 0) continue;
                const uint32_t g[2] = {ch[c] + 1, (uint32_t)nodes[ch[c]].offset};
                for (int k = 0; k < 2; ++k) if (nodes[g[k]].n_prims == 0) sub[nSub++] = g[k];
            }
            for (int k = nSub - 1; k >= 0; --k) stack.push_back(sub[k]);   // first slot's subtree next in memory
        }
    }
    const size_t nWide = std::max<size_t>(order.size(), 1);
    std::vector<float4> w(nWide * 8, float4{0, 0, 0, 0});
    std::vector<int> need(nWide, 0);   // stack entries a ray can hold below this record (filled bottom-up)
    for (size_t r = order.size(); r-- > 0;) {   // records in reverse: a child record's stack need is known before its parent's
        const uint32_t i = order[r];
        float4 *rec = &w[r * 8];
        if (nodes[i].n_prims > 0) {   // single-leaf tree: the root itself in slot 0
            int link1[4] = {nodes[i].offset, 0, 0, 0};
            unsigned cnt1[4] = {LeafMeta(d, nodes[i], coop), 0xffffu, 0xffffu, 0xffffu};
            SetWide4Box(rec, 0, nodes[i]);
            const int gN1[2] = {1, 0}, gA1[2] = {0, 0};
            FinishWide4Record(rec, link1, cnt1, 0, gN1, gA1);
            need[r] = 0;
            continue;
        }
        int link[4] = {0, 0, 0, 0};
        unsigned cnt[4] = {0xffffu, 0xffffu, 0xffffu, 0xffffu};
        int gN[2] = {0, 0}, gA[2] = {0, 0}, below = 0, present = 0;
        const uint32_t ch[2] = {i + 1, (uint32_t)nodes[i].offset};
        for (int c = 0; c < 2; ++c) {
            const mi_bvh_node &cn = nodes[ch[c]];
            uint32_t sl[2];
            if (cn.n_prims > 0) { gN[c] = 1; sl[0] = ch[c]; }
            else { gN[c] = 2; gA[c] = cn.axis; sl[0] = ch[c] + 1; sl[1] = (uint32_t)cn.offset; }
            for (int k = 0; k < gN[c]; ++k) {
                const mi_bvh_node &gn = nodes[sl[k]];
                const int slot = 2 * c + k;
                SetWide4Box(rec, slot, gn);
                if (gn.n_prims > 0) { link[slot] = gn.offset; cnt[slot] = LeafMeta(d, gn, coop); }
                else { link[slot] = widx[sl[k]]; cnt[slot] = 0; below = std::max(below, need[widx[sl[k]]]); }
                ++present;
            }
        }
        need[r] = present - 1 + below;
        FinishWide4Record(rec, link, cnt, nodes[i].axis, gN, gA);
    }
    int needAll = need[0];   // the world tree's need, plus -- inside an instance -- the return entry and the object tree's
    for (uint32_t k = 0; k < d->n_instances; ++k) needAll = std::max(needAll, need[0] + 1 + need[widx[d->instances[k].root]]);
    // (pbrt's own 64-entry stack bounds the BVH2 depth; a wide record can hold up to three entries per two levels)
    if (needAll > STACK_LDS + STACK_SPILL) return false;
    t.wnodes = std::move(w);
    t.instWideRoot.assign(std::max<uint32_t>(d->n_instances, 1), 0);
    t.instRootBounds.assign((size_t)std::max<uint32_t>(d->n_instances, 1) * 2, float4{0, 0, 0, 0});
    for (uint32_t k = 0; k < d->n_instances; ++k) {
        const mi_bvh_node &rn = nodes[d->instances[k].root];
        t.instWideRoot[k] = widx[d->instances[k].root];
        t.instRootBounds[2 * k] = float4{rn.bmin[0], rn.bmin[1], rn.bmin[2], 0};
        t.instRootBounds[2 * k + 1] = float4{rn.bmax[0], rn.bmax[1], rn.bmax[2], 0};
    }
    return true;
}

// Wide-2 records: one 64-B record per interior node with both children's boxes.
std::vector<float4> BuildWide2(const mi_scene_desc *d, bool coop) {
    const uint32_t nN = d->n_nodes;
    std::vector<int32_t> widx(nN, -1);
    uint32_t nInterior = 0;
    for (uint32_t i = 0; i < nN; ++i) if (d->nodes[i].n_prims == 0) widx[i] = (int32_t)nInterior++;
    const bool rootLeaf = nN > 0 && d->nodes[0].n_prims > 0;
    std::vector<float4> w((size_t)std::max<uint32_t>(nInterior, 1) * 4, float4{0, 0, 0, 0});
    auto putChild = [&](float4 *rec, int which, uint32_t child, int axis) {
        const mi_bvh_node &c = d->nodes[child];
        int link, meta;
        if (c.n_prims > 0) { link = c.offset; meta = (int)LeafMeta(d, c, coop); }
        else { link = widx[child]; meta = 0; }
        if (which == 0) {
            rec[0] = float4{c.bmin[0], c.bmin[1], c.bmin[2], c.bmax[0]};
            rec[1].x = c.bmax[1]; rec[1].y = c.bmax[2];
            meta |= axis << 16;
            memcpy(&rec[3].x, &link, 4); memcpy(&rec[3].z, &meta, 4);
        } else {
            rec[1].z = c.bmin[0]; rec[1].w = c.bmin[1];
            rec[2] = float4{c.bmin[2], c.bmax[0], c.bmax[1], c.bmax[2]};
            memcpy(&rec[3].y, &link, 4); memcpy(&rec[3].w, &meta, 4);
        }
    };
    if (rootLeaf) {  // single-leaf tree: the root itself is the left "child", no right child
        putChild(&w[0], 0, 0, 0);
        const int absent = 0xffff;
        memcpy(&w[3].w, &absent, 4);
    } else {
        for (uint32_t i = 0; i < nN; ++i) {
            if (d->nodes[i].n_prims != 0) continue;
            float4 *rec = &w[(size_t)widx[i] * 4];
            putChild(rec, 0, i + 1, d->nodes[i].axis);
            putChild(rec, 1, (uint32_t)d->nodes[i].offset, d->nodes[i].axis);
        }
    }
    return w;
}

// The traversal records: wide-4 unless MIPT_BVH_WIDTH=2 asks for wide-2 or the tree is too deep for wide-4; object
// instances are only traversed over wide-4 records.
int BuildBvhTables(const mi_scene_desc *d, bool coop, BvhTables &t) {
    t.width = 4;
    if (const char *e = getenv("MIPT_BVH_WIDTH")) t.width = (atoi(e) == 2) ? 2 : 4;
    if (t.width == 4 && d->n_nodes > 0 && !BuildWide4(d, coop, t)) t.width = 2;
    if (t.width == 2 && d->n_instances > 0) {
        g_err = "object instances are traversed over the two-level BVH records (MIPT_BVH_WIDTH=4), which MIPT_BVH_WIDTH=2 or this scene's tree depth rules out";
        return MI_ERR_UNSUPPORTED;
    }
    if (t.width == 2) t.wnodes = BuildWide2(d, coop);
    return MI_OK;
}

struct ShadingClasses {
    std::vector<int> matClass;                       // per material: its shading class
    unsigned classMask = 1u << MISS_CLASS;           // DScene::classMask
    unsigned shadeClasses[N_SHADE_INSTANCES] = {0};  // mi_pt::shadeClasses
    // what the two above were made from (mi_pt_shade_plan reports it)
    int classLobes[MAX_CLASSES] = {0};       // per class: the longest lobe list
    unsigned classTypes[MAX_CLASSES] = {0};  // per class: lobe types (bits 0..15) and fresnel kinds (bits 16..) present
    int classInstance[MAX_CLASSES] = {0};    // per class in classMask: its k_shade instance
    bool hasInfiniteLight = false, instanced = false;
    unsigned hot = 0;   // the lights and sampler bits of the scene's matte and plastic instances
};

// Shading classes: one per distinct lobe-type list, in order of first appearance; then each class to its k_shade
// instance (ShadeInstanceOf; `hot`: the lights and sampler bits of the scene's matte and plastic instances).
int BuildShadingClasses(const mi_scene_desc *d, bool instanced, unsigned hot, ShadingClasses &sc) {
    sc.matClass.assign(d->n_materials, 0);
    int (&classLobes)[MAX_CLASSES] = sc.classLobes;
    unsigned (&classTypes)[MAX_CLASSES] = sc.classTypes;
    std::vector<std::vector<int>> signatures;
    // (`noise`: some texture needs the hit point or is one of the classes beside image, 2-D spectrum checkerboard and noise --
    // the code the TM_HOLDS_NOISE instances alone hold)
    bool noise = false, projection = false;
    for (uint32_t i = 0; i < d->n_textures; ++i) noise |= MI_TEX_IS_GENERAL(d->textures[i]);
    for (uint32_t i = 0; i < d->n_lights; ++i) projection |= d->lights[i].type == MI_LIGHT_PROJECTION;
    for (uint32_t i = 0; i < d->n_materials; ++i) {
        const mi_material &m = d->materials[i];
        std::vector<int> sig;
        for (int j = 0; j < m.n_bxdfs; ++j) { sig.push_back(m.bxdf[j].type); sig.push_back(m.bxdf[j].fresnel); }
        sig.push_back(m.textured ? 1 : 0);
        size_t c = 0;
        while (c < signatures.size() && signatures[c] != sig) ++c;
        if (c == signatures.size()) signatures.push_back(sig);
        const int cl = sc.matClass[i] = (int)std::min<size_t>(c, MISS_CLASS - 1);
        sc.classMask |= 1u << cl;
        classLobes[cl] = std::max(classLobes[cl], (c >= (size_t)MISS_CLASS - 1) ? MI_MAX_BXDFS : (int)m.n_bxdfs);
        for (int j = 0; j < m.n_bxdfs; ++j) {
            classTypes[cl] |= (1u << m.bxdf[j].type) | (1u << (16 + m.bxdf[j].fresnel));
            if (m.bxdf[j].scaled) classTypes[cl] |= TM_SCALED;
        }
        if (m.textured) classTypes[cl] |= TM_TEXTURED;
    }
    for (int c = 0; c < MAX_CLASSES; ++c) {
        if (!((sc.classMask >> c) & 1u)) continue;
        const int i = ShadeInstanceOf(classTypes[c], classLobes[c], instanced, hot, d->n_disks > 0, noise, projection);
        if (i < 0) { g_err = "no k_shade instance for shading class " + std::to_string(c); return MI_ERR_UNSUPPORTED; }
        sc.classInstance[c] = i;
        sc.shadeClasses[i] |= 1u << c;
    }
    return MI_OK;
}

// The shading plan of a description: what of the scene picks among the instances, then the classes and their instances.
// mi_pt_create (BuildHostTables) and mi_pt_shade_plan both get it here. (The class records are accumulated: sc starts empty.)
int PlanShading(const mi_scene_desc *d, ShadingClasses &sc) {
    sc = ShadingClasses{};
    for (uint32_t i = 0; i < d->n_lights; ++i) sc.hasInfiniteLight |= d->lights[i].type == MI_LIGHT_INFINITE;
    sc.instanced = d->n_instances > 0;
    // the matte and plastic instances exist with and without the environment-light code and with the Halton sampler alone or all three
    sc.hot = (sc.hasInfiniteLight ? TM_LIGHTS_ALL : TM_LIGHTS_NO_ENV) | (d->sampler.type == MI_SAMPLER_HALTON ? 0u : TM_SAMPLERS);
    return BuildShadingClasses(d, sc.instanced, sc.hot, sc);
}

// Whether Triangle::Intersect rejects the triangle (vertices v, positions a, b, c) as degenerate (triangle.cpp:303-314):
// decided once here with the same arithmetic (doubles in Cross).
bool DegenerateTriangle(const mi_scene_desc *d, const int32_t *v, const mi_mesh &m, float4 a, float4 b, float4 c) {
    auto cross = [](const float *u, const float *w, double *o) {
        o[0] = (double)u[1] * w[2] - (double)u[2] * w[1];
        o[1] = (double)u[2] * w[0] - (double)u[0] * w[2];
        o[2] = (double)u[0] * w[1] - (double)u[1] * w[0];
    };
    float uv[3][2] = {{0, 0}, {1, 0}, {1, 1}};
    if (m.flags & MI_MESH_HAS_UV) for (int k = 0; k < 3; ++k) { uv[k][0] = d->UV[2 * v[k]]; uv[k][1] = d->UV[2 * v[k] + 1]; }
    float duv02[2] = {uv[0][0] - uv[2][0], uv[0][1] - uv[2][1]}, duv12[2] = {uv[1][0] - uv[2][0], uv[1][1] - uv[2][1]};
    float dp02[3] = {a.x - c.x, a.y - c.y, a.z - c.z}, dp12[3] = {b.x - c.x, b.y - c.y, b.z - c.z};
    float determinant = duv02[0] * duv12[1] - duv02[1] * duv12[0];
    bool degenerateUV = std::abs(determinant) < 1e-8;
    bool needNg = degenerateUV;
    if (!degenerateUV) {
        float invdet = 1 / determinant;
        float dpdu[3], dpdv[3];
        for (int k = 0; k < 3; ++k) {
            dpdu[k] = (duv12[1] * dp02[k] - duv02[1] * dp12[k]) * invdet;
            dpdv[k] = (-duv12[0] * dp02[k] + duv02[0] * dp12[k]) * invdet;
        }
        double cr[3];
        cross(dpdu, dpdv, cr);
        float cx = (float)cr[0], cy = (float)cr[1], cz = (float)cr[2];
        if (cx * cx + cy * cy + cz * cz == 0) needNg = true;
    }
    if (!needNg) return false;
    float e1[3] = {c.x - a.x, c.y - a.y, c.z - a.z}, e2[3] = {b.x - a.x, b.y - a.y, b.z - a.z};
    double cr[3];
    cross(e1, e2, cr);
    float cx = (float)cr[0], cy = (float)cr[1], cz = (float)cr[2];
    return cx * cx + cy * cy + cz * cz == 0;
}

// Pre-gathered leaf records: positions of each BVH-ordered primitive + flags, three float4 per primitive.
std::vector<float4> BuildPrimRecords(const mi_scene_desc *d, const std::vector<int> &matClass, bool &hasAlphaMasks, bool &hasQuadrics) {
    std::vector<float4> pt3((size_t)d->n_prims * 3);
    for (uint32_t i = 0; i < d->n_prims; ++i) {
        const mi_prim &p = d->prims[i];
        float4 a{0, 0, 0, 0}, b{0, 0, 0, 0}, c{0, 0, 0, 0};
        unsigned flags = 0;
        int shapeIdx = 0;
        if (p.instance != 0) {   // a TransformedPrimitive: no shape of its own
            flags = PRIM_FLAG_INSTANCE;
            shapeIdx = p.instance - 1;
        } else if (p.shape >= 0) {
            const int32_t *v = &d->tri_indices[3 * p.shape];
            const float *P = d->P;
            a = float4{P[3 * v[0]], P[3 * v[0] + 1], P[3 * v[0] + 2], 0};
            b = float4{P[3 * v[1]], P[3 * v[1] + 1], P[3 * v[1] + 2], 0};
            c = float4{P[3 * v[2]], P[3 * v[2] + 1], P[3 * v[2] + 2], 0};
            shapeIdx = p.shape;
            const mi_mesh &m = d->meshes[d->tri_mesh[p.shape]];
            if (DegenerateTriangle(d, v, m, a, b, c)) flags |= PRIM_FLAG_DEGENERATE;
            if (m.alpha_tex >= 0 || m.shadow_alpha_tex >= 0) { flags |= PRIM_FLAG_ALPHA; hasAlphaMasks = true; }
        } else {
            hasQuadrics = true;
            flags |= PRIM_FLAG_SPHERE;
            shapeIdx = ~p.shape;
        }
        flags |= (unsigned)(p.material >= 0 ? matClass[p.material] : MISS_CLASS) << PRIM_CLASS_SHIFT;
        memcpy(&a.w, &flags, 4);
        memcpy(&b.w, &shapeIdx, 4);
        pt3[3 * i] = a; pt3[3 * i + 1] = b; pt3[3 * i + 2] = c;
    }
    return pt3;
}

// Dilated world bounds of the area lights' shapes (dark MIS rays, MIS_EXCL_DARK), two float4 per light (min, max).
std::vector<float4> BuildLightBounds(const mi_scene_desc *d) {
    std::vector<float4> lb((size_t)std::max<uint32_t>(d->n_lights, 1) * 2, float4{-INFINITY, -INFINITY, -INFINITY, 0});
    for (uint32_t i = 0; i < d->n_lights; ++i) {
        const mi_light &l = d->lights[i];
        float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        auto add = [&](float x, float y, float z) { const float p[3] = {x, y, z}; for (int a = 0; a < 3; ++a) { mn[a] = std::min(mn[a], p[a]); mx[a] = std::max(mx[a], p[a]); } };
        bool have = false;
        if (l.type == MI_LIGHT_DIFFUSE_AREA && l.shape >= 0 && (uint32_t)l.shape < d->n_tris) {
            const int32_t *v = &d->tri_indices[3 * l.shape];
            for (int k = 0; k < 3; ++k) add(d->P[3 * v[k]], d->P[3 * v[k] + 1], d->P[3 * v[k] + 2]);
            have = true;
        } else if (l.type == MI_LIGHT_DIFFUSE_AREA && l.shape < 0 && (uint32_t)(~l.shape) < d->n_spheres) {
            const mi_sphere &sp = d->spheres[~l.shape];   // Sphere::ObjectBound through ObjectToWorld (shape.cpp:50)
            for (int c = 0; c < 8; ++c) {
                const float x = (c & 1) ? sp.radius : -sp.radius, y = (c & 2) ? sp.radius : -sp.radius, z = (c & 4) ? sp.z_max : sp.z_min;
                const float *m = sp.o2w;
                const float w = m[12] * x + m[13] * y + m[14] * z + m[15];
                add((m[0] * x + m[1] * y + m[2] * z + m[3]) / w, (m[4] * x + m[5] * y + m[6] * z + m[7]) / w, (m[8] * x + m[9] * y + m[10] * z + m[11]) / w);
            }
            have = true;
        } else if (l.type == MI_LIGHT_DIFFUSE_AREA && l.shape < 0 && (uint64_t)(uint32_t)(~l.shape) < (uint64_t)d->n_spheres + d->n_disks) {
            const mi_disk &k = d->disks[(uint32_t)(~l.shape) - d->n_spheres];   // Disk::ObjectBound (disk.cpp:43-46) through ObjectToWorld
            for (int c = 0; c < 4; ++c) {
                const float x = (c & 1) ? k.radius : -k.radius, y = (c & 2) ? k.radius : -k.radius, z = k.height;
                const float *m = k.o2w;
                const float w = m[12] * x + m[13] * y + m[14] * z + m[15];
                add((m[0] * x + m[1] * y + m[2] * z + m[3]) / w, (m[4] * x + m[5] * y + m[6] * z + m[7]) / w, (m[8] * x + m[9] * y + m[10] * z + m[11]) / w);
            }
            have = true;
        }
        if (have) {
            float scale = 0;
            for (int a = 0; a < 3; ++a) scale = std::max(scale, std::max(std::abs(mn[a]), std::abs(mx[a])) + (mx[a] - mn[a]));
            const float e = 1e-3f * scale;
            lb[2 * i] = float4{mn[0] - e, mn[1] - e, mn[2] - e, 0};
            lb[2 * i + 1] = float4{mx[0] + e, mx[1] + e, mx[2] + e, 0};
        } else {   // not an area light: everything may hit
            lb[2 * i] = float4{-INFINITY, -INFINITY, -INFINITY, 0};
            lb[2 * i + 1] = float4{INFINITY, INFINITY, INFINITY, 0};
        }
    }
    return lb;
}

// The area lights' primitives (DScene::lightPrim), and whether the MIS rays can be asked as visibility queries (k_trav,
// MODE 3): no instances (the traversal kernels compiled for those keep the closest-hit form), no alpha mask on an
// emitter's own mesh, and every area light the shape of exactly one primitive.
std::vector<int> BuildLightPrims(const mi_scene_desc *d, bool &misAny) {
    std::vector<int> lp((size_t)std::max<uint32_t>(d->n_lights, 1), (int)MIS_EXCL_NONE), seen((size_t)std::max<uint32_t>(d->n_lights, 1), 0);
    bool ok = d->n_instances == 0 && d->n_prims < MIS_EXCL_DARK;
    for (uint32_t i = 0; i < d->n_prims; ++i) {
        const int al = d->prims[i].area_light;
        if (al < 0) continue;
        if ((uint32_t)al >= d->n_lights) { ok = false; continue; }
        lp[al] = (int)i;
        if (++seen[al] > 1 || d->prims[i].shape != d->lights[al].shape || d->prims[i].instance != 0) ok = false;
    }
    for (uint32_t i = 0; i < d->n_lights; ++i) {
        const mi_light &l = d->lights[i];
        if (l.type != MI_LIGHT_DIFFUSE_AREA) continue;
        if (!seen[i]) ok = false;
        // an emitter whose own mesh is masked: Shape::Pdf intersects it without the mask (shape.cpp:60), the traversal with it
        if (l.shape >= 0 && (uint32_t)l.shape < d->n_tris) {
            const mi_mesh &m = d->meshes[d->tri_mesh[l.shape]];
            if (m.alpha_tex >= 0 || m.shadow_alpha_tex >= 0) ok = false;
        }
    }
#ifdef MIPT_NO_MIS_ANY
    ok = false;
#endif
    misAny = ok;
    return lp;
}

// The Halton sampler's division magics: ceil(2^64 / p) for p not a power of two; p == 2 is never divided here.
std::vector<uint64_t> BuildPrimeMagics(const mi_sampler &sm) {
    std::vector<uint64_t> magic(sm.n_dims);
    for (int i = 0; i < sm.n_dims; ++i) magic[i] = (~0ull) / (uint64_t)sm.primes[i] + 1;
    return magic;
}

// The Halton records (HaltonDim, d_scene.h) of every sampler dimension, and behind them a copy of the permutations, which
// permOffset reaches from the table's start. invBase and tail are computed here in float, in the expression order of
// ScrambledRadicalInverseBase (d_sampling.h): this file is compiled without contraction on both sides and IEEE division is
// correctly rounded on both, so the two floats are the bits the device's own divisions give.
std::vector<HaltonDim> BuildHaltonDims(const mi_sampler &sm, const std::vector<uint64_t> &magic) {
    const size_t nDims = (size_t)sm.n_dims, permBytes = (size_t)sm.n_perms * sizeof(uint16_t);
    std::vector<HaltonDim> table(nDims + (permBytes + sizeof(HaltonDim) - 1) / sizeof(HaltonDim));
    memset(table.data(), 0, table.size() * sizeof(HaltonDim));
    for (size_t i = 0; i < nDims; ++i) {
        HaltonDim &r = table[i];
        const uint16_t *perm = sm.perms + sm.prime_sums[i];
        r.base = (uint32_t)sm.primes[i];
        r.permOffset = (uint32_t)(nDims * (sizeof(HaltonDim) / sizeof(uint16_t)) + (size_t)sm.prime_sums[i]);
        r.magic = magic[i];
        const float invBase = 1.f / (float)sm.primes[i];
        r.invBase = invBase;
        r.tail = invBase * (float)perm[0] / (1 - invBase);
    }
    if (permBytes) memcpy((void *)(table.data() + nDims), sm.perms, permBytes);
    return table;
}

// The per-pixel Halton index offsets over a 128 x 128 tile (GetIndexForSample, halton.cpp:98-118).
std::vector<uint32_t> BuildPixelOffsets(const mi_sampler &sm) {
    std::vector<uint32_t> table(128 * 128, 0);
    if (sm.sample_stride <= 1) return table;
    auto inverseRadicalInverse = [](uint64_t base, uint64_t inverse, int nDigits) {
        uint64_t index = 0;
        for (int i = 0; i < nDigits; ++i) { uint64_t digit = inverse % base; inverse /= base; index = index * base + digit; }
        return index;
    };
    for (int py = 0; py < 128; ++py)
        for (int px = 0; px < 128; ++px) {
            int64_t offset = 0;
            const int pm[2] = {px, py};
            for (int i = 0; i < 2; ++i) {
                uint64_t dimOffset = inverseRadicalInverse(i == 0 ? 2 : 3, (uint64_t)pm[i], sm.base_exponents[i]);
                offset += (int64_t)(dimOffset * (uint64_t)(sm.sample_stride / sm.base_scales[i]) * (uint64_t)sm.mult_inverse[i]);
            }
            offset %= (int64_t)sm.sample_stride;
            table[py * 128 + px] = (uint32_t)offset;
        }
    return table;
}

// MIPMap::weightLut (mipmap.h:199-206).
std::vector<float> BuildEwaWeights() {
    std::vector<float> lut(128);
    for (int i = 0; i < 128; ++i) {
        float alpha = 2;
        float r2 = float(i) / float(128 - 1);
        lut[i] = std::exp(-alpha * r2) - std::exp(-alpha);
    }
    return lut;
}

struct HostTables {
    BvhTables bvh;
    ShadingClasses classes;
    std::vector<float4> primTri, lightBounds;
    std::vector<int> lightPrim;
    std::vector<uint64_t> primeMagic;
    std::vector<HaltonDim> haltonDims;
    std::vector<uint32_t> pixelOffsets;
    std::vector<float> ewaWeights;
    bool hasAlphaMasks = false, hasQuadrics = false, misAny = false;
};

int BuildHostTables(const mi_scene_desc *d, HostTables &h) {
    const bool coop = getenv("MIPT_NO_COOP_LEAVES") == nullptr;
    int rc = BuildBvhTables(d, coop, h.bvh);
    if (rc != MI_OK) return rc;
    if ((rc = PlanShading(d, h.classes)) != MI_OK) return rc;
    h.primTri = BuildPrimRecords(d, h.classes.matClass, h.hasAlphaMasks, h.hasQuadrics);
    h.lightBounds = BuildLightBounds(d);
    h.lightPrim = BuildLightPrims(d, h.misAny);
    h.primeMagic = BuildPrimeMagics(d->sampler);
    h.haltonDims = BuildHaltonDims(d->sampler, h.primeMagic);
    h.pixelOffsets = BuildPixelOffsets(d->sampler);
    h.ewaWeights = BuildEwaWeights();
    return MI_OK;
}

// -----------------------------------------------------------------------------
// mi_pt_create, step 3: the renderer's fields, the uploads, the create-time kernels and the render state
// -----------------------------------------------------------------------------
void SetSceneFields(mi_pt *pt, const mi_scene_desc *d, const HostTables &h) {
    DScene &s = pt->scene;
    s.bvhWidth = h.bvh.width;
    s.nInstances = d->n_instances;
    s.misAny = h.misAny ? 1 : 0;
    s.classMask = h.classes.classMask;
    s.nNodes = d->n_nodes; s.nPrims = d->n_prims; s.nLights = d->n_lights; s.nMaterials = d->n_materials;
    for (int i = 0; i < MI_NSPEC; ++i) s.cieY[i] = d->cie_y[i];
    s.invSqrtSpp = 1 / std::sqrt((float)d->sampler.samples_per_pixel);
    s.nInfiniteLights = 0;
    for (int k = 0; k < 4; ++k) s.infiniteLights[k] = -1;
    for (uint32_t i = 0; i < d->n_lights; ++i)
        if (d->lights[i].type == MI_LIGHT_INFINITE) s.infiniteLights[s.nInfiniteLights++] = (int)i;
    s.camera = d->camera;
    s.cameraType = d->camera_type;
    s.lens = nullptr;   // (UploadScene: the device copy)
    s.motions = nullptr; s.timePlane = 0;   // (UploadScene, when an instance moves)
    s.lensDiff = 0;
    if (d->camera_type != MI_CAMERA_PERSPECTIVE)   // (k_shade restates the perspective camera's offset rays itself)
        for (uint32_t i = 0; i < d->n_materials; ++i) if (d->materials[i].textured) s.lensDiff = 1;
    s.fullRes[0] = d->film.full_res[0]; s.fullRes[1] = d->film.full_res[1];
    s.envIpd = d->env_ipd; s.envPoleMergeTo = d->env_pole_merge_to; s.envPoleMergeFrom = d->env_pole_merge_from;
    s.envConvergenceDistance = d->env_convergence_distance;
    for (int i = 0; i < 4; ++i) { s.croppedBounds[i] = d->film.cropped_bounds[i]; s.sampleBounds[i] = d->film.sample_bounds[i]; s.pixelBounds[i] = d->integrator.pixel_bounds[i]; }
    s.filterRadius[0] = d->film.filter_radius[0]; s.filterRadius[1] = d->film.filter_radius[1];
    s.maxSampleLuminance = d->film.max_sample_luminance;
    for (int i = 0; i < 2; ++i) { s.baseScales[i] = d->sampler.base_scales[i]; s.baseExponents[i] = d->sampler.base_exponents[i]; s.multInverse[i] = d->sampler.mult_inverse[i]; }
    s.sampleStride = d->sampler.sample_stride;
    s.sampleAtPixelCenter = d->sampler.sample_at_pixel_center;
    s.samplerType = d->sampler.type;
    s.samplesPerPixel = d->sampler.samples_per_pixel;
    s.index32 = 0; s.storePixelSample = 1;
    s.ignoreRayWeight = 0;
    s.pixelDims = d->sampler.pixel_dims; s.xSamples = d->sampler.x_samples; s.ySamples = d->sampler.y_samples; s.jitter = d->sampler.jitter;
    s.sobolResolution = d->sampler.sobol_resolution;
    s.sobolLog2Resolution = d->sampler.sobol_log2_resolution;
    s.maxDepth = d->integrator.max_depth;
    s.rrThreshold = d->integrator.rr_threshold;
    s.nBands = d->integrator.n_ca_bands;
    s.bandDelta = (int)std::round((float)MI_NSPEC / (float)s.nBands);  // spectralpath.cpp:258
    if (d->n_nodes) for (int i = 0; i < 3; ++i) { s.wbMin[i] = d->nodes[0].bmin[i]; s.wbMax[i] = d->nodes[0].bmax[i]; }
    s.ldType = d->light_distrib.type;
    for (int i = 0; i < 3; ++i) s.nVoxels[i] = d->light_distrib.n_voxels[i];
    pt->hasAlphaMasks = h.hasAlphaMasks;
    pt->hasInstances = d->n_instances > 0;
    pt->hasQuadrics = h.hasQuadrics;
    pt->nQuadrics = d->n_spheres + d->n_disks;
    pt->samplerDims = d->sampler.n_dims;
    for (uint32_t i = 0; i < d->n_lights; ++i) pt->lightTypes.push_back(d->lights[i].type);
    for (uint32_t i = 0; i < d->n_materials; ++i) {
        const mi_material &m = d->materials[i];
        const bool tex = m.textured || m.bump_tex >= 0 || m.rough_tex[0] >= 0 || m.rough_tex[1] >= 0 || m.sigma_tex >= 0;
        pt->materialLobes.push_back(tex ? -1 - m.n_bxdfs : m.n_bxdfs);
    }
    pt->hasInfiniteLight = h.classes.hasInfiniteLight;
    memcpy(pt->shadeClasses, h.classes.shadeClasses, sizeof(pt->shadeClasses));
    pt->nTextures = d->n_textures;
    for (uint32_t i = 0; i < d->n_textures; ++i) pt->textureTypes.push_back(d->textures[i].type);
    pt->spp = d->sampler.samples_per_pixel;
    if (d->prim_meta) pt->primMetaHost.assign(d->prim_meta, d->prim_meta + d->n_prims);
}

// The description's arrays and the host tables into device memory. Environment maps and image pyramids go as their
// tables first, then as the records that point at them.
int UploadScene(mi_pt *pt, const mi_scene_desc *d, const HostTables &h) {
    DScene &s = pt->scene;
    Uploads up{pt};
    up((const float4 *)d->nodes, (size_t)d->n_nodes * 2, s.nodes);
    if (!h.bvh.wnodes.empty()) up(h.bvh.wnodes.data(), h.bvh.wnodes.size(), s.wnodes);
    if (!h.bvh.instWideRoot.empty()) {
        up(h.bvh.instWideRoot.data(), h.bvh.instWideRoot.size(), s.instWideRoot);
        up(h.bvh.instRootBounds.data(), h.bvh.instRootBounds.size(), s.instRootBounds);
    }
    up(h.primTri.data(), h.primTri.size(), s.primTri);
    up(d->prims, d->n_prims, s.prims);
    if (d->n_instances) up(d->instances, d->n_instances, s.instances);
    if (d->n_motions) { up(d->motions, d->n_motions, s.motions); s.timePlane = TimePlaneOf(s); }
    up(d->tri_indices, (size_t)d->n_tris * 3, s.triIndices);
    up(d->tri_mesh, d->n_tris, s.triMesh);
    up(d->P, (size_t)d->n_verts * 3, s.P);
    up(d->N, (size_t)d->n_verts * 3, s.N);
    up(d->UV, (size_t)d->n_verts * 2, s.UV);
    up(d->meshes, d->n_meshes, s.meshes);
    up(d->spheres, d->n_spheres, s.spheres);
    up(d->disks, d->n_disks, s.disks);
    s.nSpheres = (int)d->n_spheres;
    up(d->materials, d->n_materials, s.materials);
    up(d->lights, d->n_lights, s.lights);
    up(&d->camera, 1, s.cameraMotion);
    if (d->camera_type == MI_CAMERA_REALISTIC) up(d->lens, 1, s.lens);   // (the by-value record now points at the device copy)
    up(h.lightBounds.data(), h.lightBounds.size(), s.lightBounds);
    up(h.lightPrim.data(), h.lightPrim.size(), s.lightPrim);
    up(d->sampler.primes, d->sampler.n_dims, s.primes);
    up(d->sampler.prime_sums, d->sampler.n_dims, s.primeSums);
    up(d->sampler.perms, d->sampler.n_perms, s.perms);
    up(d->film.filter_table, 256, s.filterTable);
    if (d->sampler.type == MI_SAMPLER_SOBOL) {
        up(d->sampler.sobol_matrices, (size_t)d->sampler.n_sobol_dims * MI_SOBOL_MATRIX_SIZE, s.sobolMatrices);
        up(d->sampler.sobol_vdc, (size_t)MI_SOBOL_MATRIX_SIZE, s.sobolVdc);
        up(d->sampler.sobol_vdc_inv, (size_t)MI_SOBOL_MATRIX_SIZE, s.sobolVdcInv);
    }
    up(h.primeMagic.data(), h.primeMagic.size(), s.primeMagic);
    up(h.haltonDims.data(), h.haltonDims.size(), s.haltonDims);
    up(h.pixelOffsets.data(), h.pixelOffsets.size(), s.pixelOffsetTable);
    std::vector<mi_envmap> envs(d->envmaps, d->envmaps + d->n_envmaps);
    for (mi_envmap &m : envs) {
        const mi_envmap e = m;
        up(e.rgb, (size_t)e.width * e.height * 3, m.rgb);
        up(e.cond_func, (size_t)e.nu * e.nv, m.cond_func);
        up(e.cond_cdf, (size_t)(e.nu + 1) * e.nv, m.cond_cdf);
        up(e.cond_func_int, (size_t)e.nv, m.cond_func_int);
        up(e.marg_func, (size_t)e.nv, m.marg_func);
        up(e.marg_cdf, (size_t)e.nv + 1, m.marg_cdf);
    }
    if (!envs.empty()) up(envs.data(), envs.size(), s.envmaps);
    up(&d->rgb_illum[0][0], (size_t)7 * MI_NSPEC, s.rgbIllum);
    std::vector<mi_mipmap> mips(d->mipmaps, d->mipmaps + d->n_mipmaps);
    for (mi_mipmap &m : mips) {
        size_t nTexels = 0;
        for (int l = 0; l < m.n_levels; ++l) nTexels = std::max<size_t>(nTexels, (size_t)m.level_offset[l] + (size_t)std::max(1, m.width >> l) * std::max(1, m.height >> l));
        const float *texels = m.texels;
        up(texels, nTexels * 3, m.texels);
    }
    if (!mips.empty()) up(mips.data(), mips.size(), s.mipmaps);
    // (a spectrum noise value v reaches the lobes in the checkerboard's compact form: (1 - v) * spec1 + v * spec2 with spec1 = 0,
    // spec2 = 1 is v in every bin -- EvalImageTexture, TexBin)
    std::vector<mi_texture> texs(d->textures, d->textures + d->n_textures);
    for (mi_texture &t : texs)
        if (MI_TEX_IS_NOISE(t.type))
            for (int b = 0; b < MI_NSPEC; ++b) { t.spec1[b] = 0.f; t.spec2[b] = 1.f; }
    if (!texs.empty()) up(texs.data(), texs.size(), s.textures);
    up(h.ewaWeights.data(), h.ewaWeights.size(), s.ewaWeights);
    return up.rc;
}

// The tables that kernels build at create: the pixel samplers' tables (every sampled dimension of every sample of every
// pixel of the sample bounds, 12 bytes each: StartPixel of the reference, done once for all pixels) and the spatial light
// distribution; the other light distributions are uploaded as they are.
int BuildDeviceTables(mi_pt *pt, const mi_scene_desc *d) {
    DScene &s = pt->scene;
    int rc = MI_OK;
    if (d->sampler.type >= MI_SAMPLER_ZEROTWO && d->sampler.pixel_dims > 0) {
        const size_t nPix = (size_t)(s.sampleBounds[2] - s.sampleBounds[0]) * (size_t)(s.sampleBounds[3] - s.sampleBounds[1]);
        const size_t nVal = nPix * (size_t)s.pixelDims * (size_t)s.samplesPerPixel;
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) { (void)hipGetLastError(); freeB = ~(size_t)0; }
        if (nVal * 12 > freeB / 2) { g_err = "the pixel sampler's tables (" + std::to_string(nVal * 12 >> 20) + " MiB) exceed half the free device memory"; return MI_ERR_NOMEM; }
        float *t1 = nullptr, *t2 = nullptr;
        if ((rc = Alloc(pt, nVal * 4 + 16, &t1, "pixel sampler tables")) != MI_OK || (rc = Alloc(pt, nVal * 8 + 16, &t2, "pixel sampler tables")) != MI_OK) return rc;
        s.pixTab1 = t1; s.pixTab2 = t2;
        hipLaunchKernelGGL(k_pixel_tables, dim3((unsigned)((nPix + 127) / 128)), dim3(128), 0, 0, s, t1, t2, (unsigned long long)nPix);
        if (hipDeviceSynchronize() != hipSuccess) { g_err = "k_pixel_tables failed"; return MI_ERR_HIP; }
    }
    Uploads up{pt};
    if (d->n_lights == 0) {
        up((const float *)nullptr, 0, s.ldFunc); up((const float *)nullptr, 0, s.ldCdf); up((const float *)nullptr, 0, s.ldFuncInt);
        return up.rc;
    }
    if (s.ldType != MI_LD_SPATIAL) {
        up(d->light_distrib.func, d->n_lights, s.ldFunc);
        up(d->light_distrib.cdf, d->n_lights + 1, s.ldCdf);
        up(d->light_distrib.func_int, 1, s.ldFuncInt);
        return up.rc;
    }
    const size_t nVox = (size_t)s.nVoxels[0] * s.nVoxels[1] * s.nVoxels[2];
    float *f = nullptr, *c = nullptr, *fi = nullptr;
    if ((rc = Alloc(pt, nVox * d->n_lights * 4, &f, "light distribution")) != MI_OK || (rc = Alloc(pt, nVox * (d->n_lights + 1) * 4, &c, "light distribution")) != MI_OK ||
        (rc = Alloc(pt, nVox * 4, &fi, "light distribution")) != MI_OK) return rc;
    s.ldFunc = f; s.ldCdf = c; s.ldFuncInt = fi;
    hipLaunchKernelGGL(k_build_spatial, dim3((unsigned)((nVox + 127) / 128)), dim3(128), 0, 0, s, f, c, fi, (uint32_t)nVox);
    if (hipDeviceSynchronize() != hipSuccess) { g_err = "k_build_spatial failed"; return MI_ERR_HIP; }
    return MI_OK;
}

// The film, and per sub-renderer (concurrent on their own streams; MIPT_STREAMS overrides their count, 1..8) the
// counters, the stream and the events.
int CreateRenderState(mi_pt *pt, const mi_scene_desc *d) {
    pt->filmW = d->film.cropped_bounds[2] - d->film.cropped_bounds[0];
    pt->filmH = d->film.cropped_bounds[3] - d->film.cropped_bounds[1];
    pt->nPix = (size_t)pt->filmW * pt->filmH;
    int rc = Alloc(pt, pt->nPix * 32 * sizeof(float), &pt->film, "film");
    if (rc != MI_OK) return rc;
    hipMemset(pt->film, 0, pt->nPix * 32 * sizeof(float));
    int nSub = 1;
    if (const char *e = getenv("MIPT_STREAMS")) nSub = std::max(1, std::min(8, atoi(e)));
    pt->subs.resize(nSub);
    for (SubRenderer &sub : pt->subs) {
        if ((rc = Alloc(pt, sizeof(DevCounters), &sub.ctr, "counters")) != MI_OK) return rc;
        if (hipHostMalloc((void **)&sub.reads, sizeof(*sub.reads), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            sub.reads = nullptr;
            g_err = "hipHostMalloc(per-iteration reads) failed";
            return MI_ERR_NOMEM;
        }
        if (hipStreamCreateWithFlags(&sub.stream, hipStreamNonBlocking) != hipSuccess) { g_err = "hipStreamCreate failed"; return MI_ERR_HIP; }
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < N_EV; ++b)
                if (hipEventCreate(&sub.evIter[a][b]) != hipSuccess) { g_err = "hipEventCreate failed"; return MI_ERR_HIP; }
        int prioLeast = 0, prioGreatest = 0;   // (the lowest priority: the dark traversal fills what the main stream leaves idle)
        if (hipDeviceGetStreamPriorityRange(&prioLeast, &prioGreatest) != hipSuccess) { (void)hipGetLastError(); prioLeast = 0; }
        if (hipStreamCreateWithPriority(&sub.darkStream, hipStreamNonBlocking, prioLeast) != hipSuccess) { g_err = "hipStreamCreate failed"; return MI_ERR_HIP; }
        hipEvent_t *darkEvents[] = {&sub.evDarkGo, &sub.evDarkDone, &sub.evDark[0][0], &sub.evDark[0][1], &sub.evDark[1][0], &sub.evDark[1][1]};
        for (int k = 0; k < 6; ++k)   // (the two that only order the streams carry no timestamp)
            if (hipEventCreateWithFlags(darkEvents[k], k < 2 ? hipEventDisableTiming : hipEventDefault) != hipSuccess) { g_err = "hipEventCreate failed"; return MI_ERR_HIP; }
    }
    return MI_OK;
}

// Resident blocks per CU of the two resolve kernels that walk a queue.
int QueryQueueOccupancy(mi_pt *pt) {
    for (int mode = 1; mode < 3; ++mode) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)ResolveKernelOf(pt, mode), BLOCK, 0) != hipSuccess || nb < 1) { g_err = "occupancy query failed"; return MI_ERR_HIP; }
        pt->resolveBlocksPerCU[mode] = nb;
    }
#ifdef MIPT_TRAV_STATS
    {   // the traversal kernels of the scene: the grids above count on 4 blocks per CU closest-hit, 5 any-hit
        for (int mode = 0; mode < 5; ++mode) {
            int nb = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)TravKernelOf(pt, mode), BLOCK, 0) != hipSuccess) nb = -1;
            fprintf(stderr, "TRAVSTAT k_trav<%d> blocks per CU %d\n", mode, nb);
        }
    }
#endif
    return MI_OK;
}

}  // namespace

extern "C" {

const char *mi_pt_last_error(void) { return g_err.c_str(); }

int mi_pt_create(const mi_scene_desc *d, int device_ordinal, mi_pt **out) {
    if (!d || !out) { g_err = "null argument"; return MI_ERR_INVALID; }
    if (d->abi_version != MI_ABI_VERSION) { g_err = "mi_scene_desc ABI version mismatch"; return MI_ERR_INVALID; }
    int nDev = 0;
    if (hipGetDeviceCount(&nDev) != hipSuccess || nDev == 0) { g_err = "no HIP device available (this path has no CPU fallback)"; return MI_ERR_NO_DEVICE; }
    if (device_ordinal < 0 || device_ordinal >= nDev) { g_err = "device ordinal out of range"; return MI_ERR_NO_DEVICE; }
    int rc = CheckSceneDesc(d);
    if (rc != MI_OK) return rc;
    HostTables h;
    if ((rc = BuildHostTables(d, h)) != MI_OK) return rc;
    HIPCHK(hipSetDevice(device_ordinal));
    mi_pt *pt = new mi_pt();
    pt->device = device_ordinal;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess && prop.multiProcessorCount > 0) pt->numCUs = prop.multiProcessorCount;
    SetSceneFields(pt, d, h);
    rc = UploadScene(pt, d, h);
    if (rc == MI_OK) rc = BuildDeviceTables(pt, d);
    if (rc == MI_OK) rc = CreateRenderState(pt, d);
    if (rc == MI_OK) rc = QueryQueueOccupancy(pt);
    if (rc != MI_OK) {   // the one exit of a failed create: whatever was built is registered in pt
        mi_pt_destroy(pt);
        return rc;
    }
    *out = pt;
    return MI_OK;
}

void mi_pt_destroy(mi_pt *pt) {
    if (!pt) return;
    hipSetDevice(pt->device);
    hipDeviceSynchronize();
    for (void *p : pt->allocs) hipFree(p);   // (the film and the sub-renderers' counters among them)
    if (pt->stageSum) hipFree(pt->stageSum);
    if (pt->stageW) hipFree(pt->stageW);
    for (SubRenderer &sub : pt->subs) {
        ReleasePool(sub);
        for (int a = 0; a < 2; ++a) for (int b = 0; b < N_EV; ++b) if (sub.evIter[a][b]) hipEventDestroy(sub.evIter[a][b]);
        if (sub.stream) hipStreamDestroy(sub.stream);
        // (the hipDeviceSynchronize above has joined the dark stream, after a failed create or render as well)
        for (hipEvent_t e : {sub.evDarkGo, sub.evDarkDone, sub.evDark[0][0], sub.evDark[0][1], sub.evDark[1][0], sub.evDark[1][1]}) if (e) hipEventDestroy(e);
        if (sub.darkStream) hipStreamDestroy(sub.darkStream);
        if (sub.reads) hipHostFree(sub.reads);
    }
    delete pt;
}

// Parity tools for the shading plan (include/mi_pt.h): host code only.
int mi_pt_shade_instances(int32_t *nl, uint32_t *tm, uint32_t capacity, uint32_t *count) {
    if (!count) { g_err = "null argument"; return MI_ERR_INVALID; }
    *count = N_SHADE_INSTANCES;
    if ((nl || tm) && capacity < (uint32_t)N_SHADE_INSTANCES) { g_err = "mi_pt_shade_instances: buffer too small"; return MI_ERR_INVALID; }
    for (int i = 0; i < N_SHADE_INSTANCES; ++i) {
        if (nl) nl[i] = ShadeInstanceAt(i).nl;
        if (tm) tm[i] = ShadeInstanceAt(i).tm;
    }
    return MI_OK;
}

int mi_pt_shade_mask(const char *name, uint32_t *mask) {
    if (!name || !mask) { g_err = "null argument"; return MI_ERR_INVALID; }
#define MIPT_MASK_NAME(M_) {#M_, M_}
    static const struct { const char *name; unsigned mask; } kMasks[] = {
        MIPT_MASK_NAME(TM_DIFFUSE), MIPT_MASK_NAME(TM_PLASTIC), MIPT_MASK_NAME(TM_GLASS), MIPT_MASK_NAME(TM_UBER), MIPT_MASK_NAME(TM_DISNEY),
        MIPT_MASK_NAME(TM_GENERIC), MIPT_MASK_NAME(TM_FULL), MIPT_MASK_NAME(TM_ALL), MIPT_MASK_NAME(TM_SCALED), MIPT_MASK_NAME(TM_TEXTURED),
        MIPT_MASK_NAME(TM_INSTANCES), MIPT_MASK_NAME(TM_SAMPLERS), MIPT_MASK_NAME(TM_LIGHTS_ALL), MIPT_MASK_NAME(TM_LIGHTS_NO_ENV)};
#undef MIPT_MASK_NAME
    for (const auto &m : kMasks)
        if (strcmp(m.name, name) == 0) { *mask = m.mask; return MI_OK; }
    g_err = std::string("mi_pt_shade_mask: no mask named ") + name;
    return MI_ERR_INVALID;
}

int mi_pt_shade_grid(const uint32_t *counts, uint32_t n_counts, uint32_t classes, uint32_t *blocks) {
    if (!counts || !blocks) { g_err = "null argument"; return MI_ERR_INVALID; }
    if (n_counts != (uint32_t)MAX_CLASSES) { g_err = "mi_pt_shade_grid: one count per shading class, 16"; return MI_ERR_INVALID; }
    const unsigned long long n = ShadeGridBlocks(counts, classes);
    if (n > 0xffffffffull) { g_err = "mi_pt_shade_grid: more than 2^32 - 1 blocks"; return MI_ERR_INVALID; }
    *blocks = (uint32_t)n;
    return MI_OK;
}

int mi_pt_bsdf_probe_forms(int32_t instance, uint32_t *forms) {
    if (!forms) { g_err = "null argument"; return MI_ERR_INVALID; }
    if (instance < 0 || instance >= N_SHADE_INSTANCES) { g_err = "mi_pt_bsdf_probe_forms: instance index out of range"; return MI_ERR_INVALID; }
    *forms = BsdfProbeForms(ShadeInstanceAt(instance).nl, ShadeInstanceAt(instance).tm);
    if (*forms == 0u) { g_err = "mi_pt_bsdf_probe_forms: the instance has no row in MIPT_BSDF_PROBE_ROWS"; return MI_ERR_INVALID; }
    return MI_OK;
}

int mi_pt_shade_plan(const mi_scene_desc *d, int32_t *material_class, uint32_t material_capacity, int32_t *class_id,
                     int32_t *class_instance, int32_t *class_lobes, uint32_t *class_types, uint32_t class_capacity,
                     uint32_t *n_classes, uint32_t *hot) {
    if (!d) { g_err = "null argument"; return MI_ERR_INVALID; }
    if (d->abi_version != MI_ABI_VERSION) { g_err = "mi_scene_desc ABI version mismatch"; return MI_ERR_INVALID; }
    int rc = CheckSceneDesc(d);
    if (rc != MI_OK) return rc;
    ShadingClasses sc;
    if ((rc = PlanShading(d, sc)) != MI_OK) return rc;
    if (material_class) {
        if (material_capacity < d->n_materials) { g_err = "mi_pt_shade_plan: material buffer too small"; return MI_ERR_INVALID; }
        for (uint32_t i = 0; i < d->n_materials; ++i) material_class[i] = sc.matClass[i];
    }
    if ((class_id || class_instance || class_lobes || class_types) && class_capacity < (uint32_t)MAX_CLASSES) {
        g_err = "mi_pt_shade_plan: class buffers too small"; return MI_ERR_INVALID;
    }
    uint32_t n = 0;
    for (int c = 0; c < MAX_CLASSES; ++c) {
        if (!((sc.classMask >> c) & 1u)) continue;
        if (class_id) class_id[n] = c;
        if (class_instance) class_instance[n] = sc.classInstance[c];
        if (class_lobes) class_lobes[n] = sc.classLobes[c];
        if (class_types) class_types[n] = sc.classTypes[c];
        ++n;
    }
    if (n_classes) *n_classes = n;
    if (hot) *hot = sc.hot;
    return MI_OK;
}

}  // extern "C"
