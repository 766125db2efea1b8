// api.cpp -- the directives of the .pbrt front end for the PathIntegrator hot path: materials and their ids, shapes,
// objects and instances, lights and textures. They fill Api::pending and the scene arrays; WorldEnd (world_end.cpp)
// flattens everything into a HostScene (scene.h) instead of building pbrt's pointer graph. The state is api.h's.
// Behaviour restated from the reference (same directive and parameter names, defaults, "report and continue" policy):
//   state machine, CTM, attributes    src/core/api.cpp:895-1140,1142-1260
//   Shape / Material / lights         src/core/api.cpp:1264-1443,441-548,747-786
// Outside this path's scope and reported as errors, never silently ignored: media, other texture classes and shapes.
#include <cctype>
#include <cstdlib>
#include "api.h"

namespace mipt {
namespace {

bool ShapeMaySetMaterialParameters(const ParamSet &ps) {  // api.cpp:1451-1500
    for (const auto &p : ps.textures)
        if (p.name != "alpha" && p.name != "shadowalpha") return true;
    for (const auto &p : ps.floats)
        if (p.values.size() == 1 && p.name != "radius") return true;
    for (const auto &p : ps.strings)
        if (p.values.size() == 1 && p.name != "filename" && p.name != "type" && p.name != "scheme") return true;
    auto single = [](const auto &items) { for (const auto &p : items) if (p.values.size() == 1) return true; return false; };
    return single(ps.bools) || single(ps.ints) || single(ps.point2s) || single(ps.point3s) || single(ps.vector3s) || single(ps.normals) || single(ps.spectra);
}

// "spectrum <name>" times "spectrum scale": the emission every light is created with
Spectrum ScaledSpectrum(const ParamSet &ps, const char *name) {
    return ps.FindOneSpectrum(name, Spectrum(1.0)) * ps.FindOneSpectrum("scale", Spectrum(1.0));
}
void CopySpectrum(const Spectrum &s, float *out) { for (int i = 0; i < MI_NSPEC; ++i) out[i] = s.c[i]; }
void SetPosition(mi_light *l, const Vec3 &p) { l->pos[0] = p.x; l->pos[1] = p.y; l->pos[2] = p.z; }
void SetLightFrame(mi_light *l, const Transform &lightToWorld) {   // the rotation parts of LightToWorld and WorldToLight
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) { l->l2w[3 * r + c] = lightToWorld.m.m[r][c]; l->w2l[3 * r + c] = lightToWorld.mInv.m[r][c]; }
}
// ObjectToWorld / WorldToObject and the two orientation flags of a quadric's record (Shape ctor, shape.cpp:45-50)
template <typename Quadric> void SetQuadricFrame(Quadric *q, const Transform &ctm, bool reverseOrientation) {
    const Transform w2o = Inverse(ctm);
    std::memcpy(q->o2w, ctm.m.m, sizeof(q->o2w));
    std::memcpy(q->w2o, w2o.m.m, sizeof(q->w2o));
    q->reverse_orientation = reverseOrientation ? 1 : 0;
    q->swaps_handedness = ctm.SwapsHandedness() ? 1 : 0;
}

// What a shape builder made: a range of triangles, or one quadric (its mi_prim.shape code, < 0) with its area and object bound.
struct BuiltShape {
    int firstTri = -1, nTris = 0, quadric = 0;
    float area = 0;
    Bounds3 objectBound;
};

// The primitives `make` creates, kept apart from the world's; the CTM pair and the graphics state are put back after it.
template <typename F> std::vector<PendingPrim> MakeApart(Api &a, F make) {
    const Transform savedStart = a.ctm, savedEnd = a.ctmEnd;
    const GraphicsState savedGs = a.gs;
    std::vector<PendingPrim> world, made;
    world.swap(a.pending);
    make();
    made.swap(a.pending);
    a.pending.swap(world);
    a.ctm = savedStart; a.ctmEnd = savedEnd; a.gs = savedGs;
    return made;
}

// ------------------------------------------------------------------ materials
// `count`: the call stands for a MakeMaterial call of the reference and takes the next material id (lastMaterialId; 0 for
// "none"); false when a recorded shape is re-created, whose id was taken where the reference took it (Shape).
int MakeMaterial(Api &a, const std::string &name, const ParamSet &geom, const ParamSet &mat, bool count = true) {
    if (count) a.lastMaterialId = 0;
    if (name == "" || name == "none") return -1;
    TextureParams mp(geom, mat, a.gs.textures, &a.scene->errors);
    mi_material m;
    std::vector<std::string> errs;
    std::string type = name;
    static const char *known[] = {"matte", "plastic", "glass", "uber", "disney", "mirror", "translucent",
                                  "metal", "substrate", "mix", "hair", "fourier", "subsurface",
                                  "kdsubsurface", "retroreflective"};
    bool isKnown = false;
    for (const char *k : known) if (type == k) isKnown = true;
    if (!isKnown) {  // api.cpp:604-607
        a.Warn("Material \"" + name + "\" unknown. Using \"matte\".");
        type = "matte";
    }
    bool compiled;
    if (type == "mix") {  // api.cpp:573-593 + CreateMixMaterial (mixmat.cpp:66-72)
        auto lookup = [&](const char *param) -> mi_material {
            const std::string nm = mp.FindString(param, "");
            auto it = a.gs.namedMaterials.find(nm);
            if (it == a.gs.namedMaterials.end() || it->second->material < 0) {
                if (count && it == a.gs.namedMaterials.end()) ++a.materialCounter;   // the fallback matte is a MakeMaterial call of its own, before the mix (api.cpp:577-591)
                a.Err("Named material \"" + nm + "\" undefined.  Using \"matte\"");
                mi_material mm;
                std::vector<std::string> e2;
                CompileMaterial("matte", mp, &mm, &a.scene->warnings, &e2);
                return mm;
            }
            return a.scene->materials[it->second->material];
        };
        const mi_material m1 = lookup("namedmaterial1"), m2 = lookup("namedmaterial2");
        compiled = CompileMixMaterial(m1, m2, mp.GetSpectrum("amount", Spectrum(0.5f)), &m, &errs);
    } else
        compiled = CompileMaterial(type, mp, &m, &a.scene->warnings, &errs);
    if (compiled && (m.bump_tex >= 0 || m.rough_tex[0] >= 0 || m.rough_tex[1] >= 0)) m.textured = 1;   // bump-mapped / roughness-mapped vertices take the texture-evaluating shading instances
    if (!compiled) {
        for (auto &e : errs) a.Err(e);
        a.Err("Material \"" + name + "\" replaced by default matte on this path.");
        ParamSet e1, e2;
        TextureParams mp2(e1, e2, a.gs.textures, &a.scene->errors);
        CompileMaterial("matte", mp2, &m, &a.scene->warnings, &errs);
    }
    if (count) a.lastMaterialId = ++a.materialCounter;
    // de-duplicate identical records (a loopsubdiv shape re-creates its material, api.cpp:1502-1513)
    for (size_t i = 0; i < a.scene->materials.size(); ++i)
        if (std::memcmp(&a.scene->materials[i], &m, sizeof(m)) == 0) return (int)i;
    a.scene->materials.push_back(m);
    return (int)a.scene->materials.size() - 1;
}

// The numbers MakeMaterial(name, geom, mat) takes, without making the material: for a shape recorded inside ObjectBegin,
// whose material this front end compiles when the object is first instanced. Returns the material's id.
uint32_t TakeMaterialIds(Api &a, const std::string &name, const ParamSet &geom, const ParamSet &mat) {
    if (name == "" || name == "none") return 0;
    if (name == "mix")   // the fallback mattes of undefined named materials come first (api.cpp:577-591)
        for (const char *param : {"namedmaterial1", "namedmaterial2"})
            if (!a.gs.namedMaterials.count(geom.FindOneString(param, mat.FindOneString(param, "")))) ++a.materialCounter;
    return ++a.materialCounter;
}

// ------------------------------------------------------------------ shapes
// "alpha" / "shadowalpha" of a mesh (triangle.cpp:716-740): a named float texture or the constant 0
int AlphaTexture(Api &a, const ParamSet &params, const char *param) {
    const std::string texName = params.FindTexture(param);
    if (texName != "") {
        auto it = a.gs.textures.floatImageTex.find(texName);
        if (it != a.gs.textures.floatImageTex.end()) {
            if (MI_TEX_IS_NOISE(a.scene->textures[it->second].type)) {   // (it would put the noise into the traversal kernels)
                a.Err("Noise texture \"" + texName + "\" as \"" + param + "\" of a shape is outside the hot-path scope; the shape is left unmasked");
                return -1;
            }
            // (MIPT_TEXTURES=all) the traversal kernels hold neither the 2-D mappings nor the classes beside the image texture: a mask
            // of any of them would put that code there, whether or not it needs the hit point
            if (MI_TEX_IS_GENERAL(a.scene->textures[it->second])) {
                a.Err("Texture \"" + texName + "\" as \"" + param + "\" of a shape is outside the hot-path scope (only a \"uv\"-mapped image texture masks a shape: "
                      "the traversal kernels hold no other mapping or class); the shape is left unmasked");
                return -1;
            }
            return it->second;
        }
        auto c = a.gs.textures.floatTex.find(texName);
        if (c == a.gs.textures.floatTex.end()) { a.Err("Couldn't find float texture \"" + texName + "\" for \"" + param + "\" parameter"); return -1; }
        if (c->second != 0.f) return -1;   // a constant that is never 0 masks nothing
    } else if (params.FindOneFloat(param, 1.f) != 0.f)
        return -1;
    mi_texture t{};
    t.mipmap = ConstantFloatMipMap(a.scene, 0.f);
    t.filter = MI_TEX_TRILINEAR; t.max_aniso = 8.f; t.su = t.sv = 1.f; t.post_scale = 1.f;
    t.is_float = 1;
    a.scene->textures.push_back(t);
    return (int)a.scene->textures.size() - 1;
}

// Append a TriangleMesh (src/shapes/triangle.cpp:54-92): world-space P, N. masks: the shape's parameters when it reads
// "alpha" and "shadowalpha" (in this order: a mask may append a texture). Returns the first triangle's index.
int AddTriangleMesh(Api &a, const std::vector<int> &indices, const std::vector<Vec3> &P, const std::vector<Vec3> *N,
                         const std::vector<Vec2> *UV, const ParamSet *masks) {
    mi_mesh mesh{};
    mesh.alpha_tex = masks ? AlphaTexture(a, *masks, "alpha") : -1;
    mesh.shadow_alpha_tex = masks ? AlphaTexture(a, *masks, "shadowalpha") : -1;
    mesh.first_vertex = (uint32_t)(a.scene->P.size() / 3);
    mesh.n_vertices = (uint32_t)P.size();
    mesh.first_tri = (uint32_t)(a.scene->triIndices.size() / 3);
    mesh.n_tris = (uint32_t)(indices.size() / 3);
    mesh.flags = 0;
    if (N) mesh.flags |= MI_MESH_HAS_N;
    if (UV) mesh.flags |= MI_MESH_HAS_UV;
    if (a.gs.reverseOrientation ^ a.ctm.SwapsHandedness()) mesh.flags |= MI_MESH_FLIP;
    uint32_t meshId = (uint32_t)a.scene->meshes.size();
    for (size_t i = 0; i < P.size(); ++i) {
        Vec3 pw = a.ctm.Point(P[i]);
        a.scene->P.push_back(pw.x); a.scene->P.push_back(pw.y); a.scene->P.push_back(pw.z);
        Vec3 nw(0, 0, 0);
        if (N) nw = a.ctm.Normal((*N)[i]);
        a.scene->N.push_back(nw.x); a.scene->N.push_back(nw.y); a.scene->N.push_back(nw.z);
        Vec2 uv;
        if (UV) uv = (*UV)[i];
        a.scene->UV.push_back(uv.x); a.scene->UV.push_back(uv.y);
    }
    for (size_t i = 0; i < indices.size(); ++i) a.scene->triIndices.push_back(indices[i] + (int)mesh.first_vertex);
    for (uint32_t i = 0; i < mesh.n_tris; ++i) a.scene->triMesh.push_back(meshId);
    a.scene->meshes.push_back(mesh);
    a.scene->stats.nMeshes++;
    a.scene->stats.nTriangles += (int)mesh.n_tris;
    return (int)mesh.first_tri;
}

bool TriangleMeshShape(Api &a, const ParamSet &params, BuiltShape *b) {  // CreateTriangleMeshShape, triangle.cpp:642-740
    const std::vector<int> *vi = ParamSet::Find(params.ints, "indices");
    const std::vector<Vec3> *P = ParamSet::Find(params.point3s, "P");
    const std::vector<Vec2> *uvs = ParamSet::Find(params.point2s, "uv");
    if (!uvs) uvs = ParamSet::Find(params.point2s, "st");
    std::vector<Vec2> tempUVs;
    if (!uvs) {
        const std::vector<float> *fuv = ParamSet::Find(params.floats, "uv");
        if (!fuv) fuv = ParamSet::Find(params.floats, "st");
        if (fuv) {
            for (size_t i = 0; i + 1 < fuv->size(); i += 2) { Vec2 q; q.x = (*fuv)[i]; q.y = (*fuv)[i + 1]; tempUVs.push_back(q); }
            uvs = &tempUVs;
        }
    }
    if (!vi) { a.Err("Vertex indices \"indices\" not provided with triangle mesh shape"); return false; }
    if (!P) { a.Err("Vertex positions \"P\" not provided with triangle mesh shape"); return false; }
    if (uvs) {
        if (uvs->size() < P->size()) {
            a.Err("Not enough of \"uv\"s for triangle mesh. Discarding.");
            uvs = nullptr;
        } else if (uvs->size() > P->size())
            a.Warn("More \"uv\"s provided than will be used for triangle mesh.");
    }
    if (ParamSet::Find(params.vector3s, "S")) a.Warn("trianglemesh \"S\" tangents ignored on this path");
    const std::vector<Vec3> *N = ParamSet::Find(params.normals, "N");
    if (N && N->size() != P->size()) { a.Err("Number of \"N\"s for triangle mesh must match \"P\"s"); N = nullptr; }
    for (int idx : *vi)
        if (idx >= (int)P->size() || idx < 0) { a.Err("trianglemesh has out of-bounds vertex index"); return false; }
    std::vector<int> idx(vi->begin(), vi->begin() + (vi->size() / 3) * 3);
    b->nTris = (int)idx.size() / 3;
    b->firstTri = AddTriangleMesh(a, idx, *P, N, uvs, &params);
    return true;
}

bool PLYMeshShape(Api &a, const ParamSet &params, BuiltShape *b) {  // CreatePLYMesh, plymesh.cpp:149-283
    const std::string fn = a.AbsolutePath(params.FindOneString("filename", ""));
    std::shared_ptr<PLYMeshData> &cached = a.plyCache[fn];
    if (!cached) {
        cached = std::make_shared<PLYMeshData>();
        std::vector<std::string> w;
        std::string e;
        const bool okPly = ReadPLYMesh(fn, cached.get(), &w, &e);
        for (const std::string &m : w) a.Warn(m);
        if (!okPly) { a.Err(e); cached.reset(); a.plyCache.erase(fn); return false; }
    }
    const PLYMeshData &ply = *cached;
    b->nTris = (int)ply.indices.size() / 3;
    b->firstTri = AddTriangleMesh(a, ply.indices, ply.P, ply.N.empty() ? nullptr : &ply.N, ply.UV.empty() ? nullptr : &ply.UV, &params);
    return true;
}

bool LoopSubdivShape(Api &a, const ParamSet &params, BuiltShape *b) {  // CreateLoopSubdiv, loopsubdiv.cpp:402-424
    int nLevels = params.FindOneInt("levels", params.FindOneInt("nlevels", 3));
    const std::vector<int> *vi = ParamSet::Find(params.ints, "indices");
    const std::vector<Vec3> *P = ParamSet::Find(params.point3s, "P");
    if (!vi) { a.Err("Vertex indices \"indices\" not provided for LoopSubdiv shape."); return false; }
    if (!P) { a.Err("Vertex positions \"P\" not provided for LoopSubdiv shape."); return false; }
    (void)params.FindOneString("scheme", "loop");
    std::vector<int> oi;
    std::vector<Vec3> oP, oN;
    std::string e;
    if (!LoopSubdivide(nLevels, *vi, *P, &oi, &oP, &oN, &e)) { a.Err(e); return false; }
    b->nTris = (int)oi.size() / 3;
    b->firstTri = AddTriangleMesh(a, oi, oP, &oN, nullptr, nullptr);   // (no masks: loopsubdiv.cpp reads neither parameter)
    return true;
}

bool SphereShape(Api &a, const ParamSet &params, BuiltShape *b) {  // CreateSphereShape, sphere.cpp:318-328; Sphere ctor sphere.h:52-63
    float radius = params.FindOneFloat("radius", 1.f);
    float zmin = params.FindOneFloat("zmin", -radius);
    float zmax = params.FindOneFloat("zmax", radius);
    float phimax = params.FindOneFloat("phimax", 360.f);
    mi_sphere s{};
    SetQuadricFrame(&s, a.ctm, a.gs.reverseOrientation);
    s.radius = radius;
    s.z_min = Clamp(std::min(zmin, zmax), -radius, radius);
    s.z_max = Clamp(std::max(zmin, zmax), -radius, radius);
    s.theta_min = std::acos(Clamp(std::min(zmin, zmax) / radius, -1, 1));
    s.theta_max = std::acos(Clamp(std::max(zmin, zmax) / radius, -1, 1));
    s.phi_max = Radians(Clamp(phimax, 0, 360));
    b->quadric = ~(int)a.scene->spheres.size();
    b->area = s.phi_max * s.radius * (s.z_max - s.z_min);  // Sphere::Area, sphere.cpp:217
    b->objectBound = Bounds3(Vec3(-s.radius, -s.radius, s.z_min), Vec3(s.radius, s.radius, s.z_max));
    a.scene->spheres.push_back(s);
    a.scene->stats.nSpheres++;
    return true;
}

bool DiskShape(Api &a, const ParamSet &params, BuiltShape *b) {  // CreateDiskShape, disk.cpp:140-150; Disk ctor disk.h:49-58 ("alpha" / "shadowalpha" are not read there)
    mi_disk k{};
    SetQuadricFrame(&k, a.ctm, a.gs.reverseOrientation);
    k.height = params.FindOneFloat("height", 0.f);
    k.radius = params.FindOneFloat("radius", 1.f);
    k.inner_radius = params.FindOneFloat("innerradius", 0.f);
    k.phi_max = Radians(Clamp(params.FindOneFloat("phimax", 360.f), 0, 360));
    k.kind = MI_QUADRIC_DISK;
    b->quadric = ~(kDiskBase + (int)a.scene->disks.size());
    b->area = k.phi_max * 0.5 * (k.radius * k.radius - k.inner_radius * k.inner_radius);  // Disk::Area, disk.cpp:125-127
    b->objectBound = Bounds3(Vec3(-k.radius, -k.radius, k.height), Vec3(k.radius, k.radius, k.height));  // Disk::ObjectBound, disk.cpp:43-46
    a.scene->disks.push_back(k);
    a.scene->stats.nDisks++;
    return true;
}

int MakeAreaLight(Api &a, int shape, float area) {  // CreateDiffuseAreaLight, src/lights/diffuse.cpp:136-147
    if (a.gs.areaLight != "area" && a.gs.areaLight != "diffuse") { a.Warn("Area light \"" + a.gs.areaLight + "\" unknown."); return -1; }
    const ParamSet &ps = a.gs.areaLightParams;
    (void)ps.FindOneInt("samples", ps.FindOneInt("nsamples", 1));
    mi_light l{};
    l.type = MI_LIGHT_DIFFUSE_AREA;
    l.shape = shape;
    l.area = area;
    l.two_sided = ps.FindOneBool("twosided", false) ? 1 : 0;
    CopySpectrum(ScaledSpectrum(ps, "L"), l.L);
    a.scene->lights.push_back(l);
    return (int)a.scene->lights.size() - 1;
}

// A triangle range or a quadric as PendingPrims under the current CTM, each with its area light when one is set.
void AddPrims(Api &a, const BuiltShape &b, int material, uint32_t materialId) {
    PendingPrim pp;
    pp.material = material;
    pp.materialId = materialId; pp.instanceId = a.expandingInstance;
    pp.light = -1;
    if (b.quadric < 0) {
        pp.shape = b.quadric;
        if (a.gs.areaLight != "") {
            pp.light = MakeAreaLight(a, b.quadric, b.area);
            if (a.ctm.HasScale()) a.Warn("Scaling detected in world to light transformation!");
        }
        pp.bounds = a.ctm.Bounds(b.objectBound);  // Shape::WorldBound, shape.cpp:54
        a.pending.push_back(pp);
        return;
    }
    auto vertex = [&](int vi) { return Vec3(a.scene->P[3 * vi], a.scene->P[3 * vi + 1], a.scene->P[3 * vi + 2]); };
    for (int tri = b.firstTri; tri < b.firstTri + b.nTris; ++tri) {
        const int32_t *v = &a.scene->triIndices[3 * tri];
        Vec3 p0 = vertex(v[0]), p1 = vertex(v[1]), p2 = vertex(v[2]);
        pp.shape = tri;
        pp.light = -1;
        if (a.gs.areaLight != "") {
            float area = 0.5 * Cross(p1 - p0, p2 - p0).Length();  // Triangle::Area, triangle.cpp:575-581
            pp.light = MakeAreaLight(a, tri, area);
        }
        pp.bounds = Union(Bounds3(p0, p1), p2);  // Triangle::WorldBound
        a.pending.push_back(pp);
    }
}

// ------------------------------------------------------------------ objects and instances
// AnimatedTransform::MotionBounds (transform.cpp:1196-1208). Without rotation: the union of the two members' bounds, as
// the reference. With rotation the reference bounds every corner's path through the roots of its derivative
// (BoundPointMotion over ~650 lines of generated coefficients); here a bound of our own: the corner c is carried to
// T(dt) + R(dt) S(dt) c, S(dt) c lies on the segment from S0 c to S1 c and is no longer than the longer of the two, a
// rotation keeps that length and no coordinate of a vector exceeds its length -- so every coordinate stays within
// r = max |S_i c| of the translation's own segment. r is computed in double and widened by 1e-4 (the float rounding of
// the interpolated matrix and its quaternion's unit length: ~1e-6), and the two members' exact bounds (the boundary
// rules) are joined in. Looser than the reference's: the world tree may differ, the closest hit does not.
Bounds3 MotionBounds(const Bounds3 &b, const Transform &start, const Transform &end) {
    const Bounds3 ends = Union(start.Bounds(b), end.Bounds(b));
    const AnimatedDecomposition ad = DecomposePair(start, end);
    if (!HasRotation(ad.d[0].R, ad.d[1].R)) return ends;
    double r = 0;
    for (int corner = 0; corner < 8; ++corner) {
        const double c[3] = {(corner & 1) ? b.pMax.x : b.pMin.x, (corner & 2) ? b.pMax.y : b.pMin.y, (corner & 4) ? b.pMax.z : b.pMin.z};
        for (int i = 0; i < 2; ++i) {
            double l2 = 0;
            for (int row = 0; row < 3; ++row) {
                const double v = ad.d[i].S[3 * row] * c[0] + ad.d[i].S[3 * row + 1] * c[1] + ad.d[i].S[3 * row + 2] * c[2];
                l2 += v * v;
            }
            r = std::max(r, std::sqrt(l2));
        }
    }
    const float rf = std::nextafter((float)(r * 1.0001), std::numeric_limits<float>::infinity());
    Bounds3 path;
    for (int a = 0; a < 3; ++a) {
        const float lo = std::min(ad.d[0].T[a], ad.d[1].T[a]) - rf, hi = std::max(ad.d[0].T[a], ad.d[1].T[a]) + rf;
        (a == 0 ? path.pMin.x : a == 1 ? path.pMin.y : path.pMin.z) = std::nextafter(lo, -std::numeric_limits<float>::infinity());
        (a == 0 ? path.pMax.x : a == 1 ? path.pMax.y : path.pMax.z) = std::nextafter(hi, std::numeric_limits<float>::infinity());
    }
    return Union(ends, path);
}

// The TransformedPrimitive of an object: static when the members are equal (AnimatedTransform::actuallyAnimated).
void AddInstance(Api &a, const std::string &object, const Bounds3 &objectBounds, const Transform &start, const Transform &end, uint32_t instanceId) {
    Api::InstanceRec rec;
    rec.object = object; rec.i2w = start; rec.instanceId = instanceId;
    rec.moving = start != end; rec.i2wEnd = end;
    a.instanceRecs.push_back(rec);
    PendingPrim pp;
    pp.shape = 0; pp.material = -1; pp.light = -1;
    pp.instance = (int)a.instanceRecs.size();
    // TransformedPrimitive::WorldBound: MotionBounds, of a static transform its Bounds
    pp.bounds = rec.moving ? MotionBounds(objectBounds, start, end) : start.Bounds(objectBounds);
    a.pending.push_back(pp);
}

// A Shape under an animated CTM outside ObjectBegin (api.cpp:1389-1428): its shapes are made with the identity transform
// and without an area light, and one TransformedPrimitive carries them -- here an instance of an object of its own, with
// instance id 0 and no entry in the instance names.
void MovingShape(Api &a, const std::string &name, const ParamSet &params) {
    if (a.gs.areaLight != "") a.Warn("Ignoring currently set area light when creating animated shape");
    const Transform start = a.ctm, end = a.ctmEnd;
    std::vector<PendingPrim> made = MakeApart(a, [&] {
        a.gs.areaLight = "";
        a.ctm = a.ctmEnd = Transform();
        a.Shape(name, params);
    });
    if (made.empty()) return;   // api.cpp:1399
    const std::string object = std::string("\x01moving shape ") + std::to_string(a.nMovingShapes++);   // (no ObjectBegin can spell it)
    Api::ObjectDef &od = a.objectDefs[object];
    od.created = true; od.wrapper = true;
    od.prims.swap(made);
    for (const PendingPrim &pp : od.prims) od.bounds = Union(od.bounds, pp.bounds);
    a.objectOrder.push_back(object);
    AddInstance(a, object, od.bounds, start, end, 0);
}

// ------------------------------------------------------------------ lights
void PointLight(Api &a, const ParamSet &ps, mi_light *l) {  // CreatePointLight, point.cpp:80-88
    Vec3 from = ps.FindOnePoint3("from", Vec3(0, 0, 0));
    l->type = MI_LIGHT_POINT;
    CopySpectrum(ScaledSpectrum(ps, "I"), l->L);
    SetPosition(l, (Translate(from) * a.ctm).Point(Vec3(0, 0, 0)));
}

void DistantLight(Api &a, const ParamSet &ps, mi_light *l) {  // CreateDistantLight, distant.cpp:94-102
    Vec3 from = ps.FindOnePoint3("from", Vec3(0, 0, 0));
    Vec3 to = ps.FindOnePoint3("to", Vec3(0, 0, 1));
    Vec3 w = Normalize(a.ctm.Vector(from - to));
    l->type = MI_LIGHT_DISTANT;
    CopySpectrum(ScaledSpectrum(ps, "L"), l->L);
    l->dir[0] = w.x; l->dir[1] = w.y; l->dir[2] = w.z;
}

void SpotLight(Api &a, const ParamSet &ps, mi_light *l) {  // CreateSpotLight, spot.cpp:102-122
    float coneangle = ps.FindOneFloat("coneangle", 30.);
    Vec3 from = ps.FindOnePoint3("from", Vec3(0, 0, 0));
    Vec3 to = ps.FindOnePoint3("to", Vec3(0, 0, 1));
    Vec3 dir = Normalize(to - from);
    Vec3 du, dv;
    CoordinateSystem(dir, &du, &dv);
    Transform dirToZ(Matrix4x4(du.x, du.y, du.z, 0., dv.x, dv.y, dv.z, 0., dir.x, dir.y, dir.z, 0., 0, 0, 0, 1.));
    Transform light2world = a.ctm * Translate(Vec3(from.x, from.y, from.z)) * Inverse(dirToZ);
    l->type = MI_LIGHT_SPOT;
    CopySpectrum(ScaledSpectrum(ps, "I"), l->L);
    SetPosition(l, light2world.Point(Vec3(0, 0, 0)));
    SetLightFrame(l, light2world);
    l->cos_total_width = std::cos(Radians(coneangle));
    l->cos_falloff_start = std::cos(Radians(coneangle - ps.FindOneFloat("conedeltaangle", 5.)));
}

void InfiniteLight(Api &a, const ParamSet &ps, mi_light *l) {  // CreateInfiniteLight, infinite.cpp:176-186
    const Spectrum L = ScaledSpectrum(ps, "L");
    const std::string texmap = a.AbsolutePath(ps.FindOneString("mapname", ""));
    (void)ps.FindOneInt("samples", ps.FindOneInt("nsamples", 1));
    HostEnvMap env;
    Spectrum centre;
    std::vector<std::string> errs;
    BuildEnvMap(L, texmap, &env, &centre, &errs);
    for (const std::string &e : errs) a.Err(e);
    l->type = MI_LIGHT_INFINITE;
    l->envmap = (int)a.scene->envStore.size();
    a.scene->envStore.push_back(std::move(env));
    CopySpectrum(centre, l->L);
    SetLightFrame(l, a.ctm);
}

void ProjectionLight(Api &a, const ParamSet &ps, mi_light *l) {  // CreateProjectionLight and the constructor, projection.cpp:45-74, 133-142
    const float fov = ps.FindOneFloat("fov", 45.);
    const std::string texmap = a.AbsolutePath(ps.FindOneString("mapname", ""));
    l->type = MI_LIGHT_PROJECTION;
    CopySpectrum(ScaledSpectrum(ps, "I"), l->L);
    SetPosition(l, a.ctm.Point(Vec3(0, 0, 0)));
    SetLightFrame(l, a.ctm);
    // the map: ReadImage reports a file it cannot read and the light goes on without one
    HostEnvMap map;
    int rx = 0, ry = 0;
    Spectrum centre(1.f);
    std::string ioErr;
    l->proj_map = -1;
    if (!texmap.empty()) {
        if (BuildProjectionMap(texmap, &map, &rx, &ry, &centre, &ioErr)) {
            l->proj_map = (int)a.scene->envStore.size();
            a.scene->envStore.push_back(std::move(map));
        } else
            a.Err("LightSource \"projection\": " + ioErr + "; the light projects no map (a white frustum)");
    }
    CopySpectrum(centre, l->proj_centre);
    const float aspect = l->proj_map >= 0 ? (float(rx) / float(ry)) : 1;
    if (aspect > 1) { l->screen[0] = -aspect; l->screen[1] = -1; l->screen[2] = aspect; l->screen[3] = 1; }
    else { l->screen[0] = -1; l->screen[1] = -1 / aspect; l->screen[2] = 1; l->screen[3] = 1 / aspect; }
    l->hither = 1e-3f;
    const float yon = 1e30f;
    const Transform lightProjection = Perspective(fov, l->hither, yon);
    std::memcpy(l->proj, lightProjection.m.m, sizeof(l->proj));
    const Vec3 wCorner = Normalize(Inverse(lightProjection).Point(Vec3(l->screen[2], l->screen[3], 0)));
    l->cos_total_width = wCorner.z;
}

// ------------------------------------------------------------------ textures
// `t` becomes the scene's next texture and `name` the image texture of its type; the constant of that name and type is forgotten.
void BindImageTexture(Api &a, const std::string &name, bool isFloat, const mi_texture &t) {
    if (isFloat) a.gs.textures.floatTex.erase(name);
    else a.gs.textures.spectrumTex.erase(name);
    (isFloat ? a.gs.textures.floatImageTex : a.gs.textures.imageTex)[name] = (int)a.scene->textures.size();
    a.scene->textures.push_back(t);
    a.scene->textures.back().is_float = isFloat ? 1 : 0;
}

// The TextureMapping2D of a Create*Texture (the block every 2-D class repeats, e.g. checkerboard.cpp:50-71) into `t`: "uv" with
// uscale / vscale / udelta / vdelta; with MIPT_TEXTURES=all also "spherical" and "cylindrical" (WorldToTexture = the inverse of
// the CTM here) and "planar" (v1, v2, udelta, vdelta; no transform). false: the mapping is refused (a reported error).
bool Mapping2D(Api &a, const std::string &name, const ParamSet &ps, mi_texture *t) {
    const std::string mapping = ps.FindOneString("mapping", "uv");
    if (mapping != "uv" && !a.allTextures) {
        a.Err("Texture \"" + name + "\": 2D texture mapping \"" + mapping + "\" is outside the hot-path scope (\"uv\" only)");
        return false;
    }
    t->mapping = MI_MAP_UV;
    t->su = t->sv = 1.f; t->du = t->dv = 0.f;
    if (mapping == "uv") {
        t->su = ps.FindOneFloat("uscale", 1.f); t->sv = ps.FindOneFloat("vscale", 1.f);
        t->du = ps.FindOneFloat("udelta", 0.f); t->dv = ps.FindOneFloat("vdelta", 0.f);
    } else if (mapping == "spherical" || mapping == "cylindrical") {
        t->mapping = mapping == "spherical" ? MI_MAP_SPHERICAL : MI_MAP_CYLINDRICAL;
        std::memcpy(t->w2t, a.ctm.mInv.m, sizeof(t->w2t));
    } else if (mapping == "planar") {
        t->mapping = MI_MAP_PLANAR;
        const Vec3 v1 = ps.FindOneVector3("v1", Vec3(1, 0, 0)), v2 = ps.FindOneVector3("v2", Vec3(0, 1, 0));
        t->vs[0] = v1.x; t->vs[1] = v1.y; t->vs[2] = v1.z;
        t->vt[0] = v2.x; t->vt[1] = v2.y; t->vt[2] = v2.z;
        t->du = ps.FindOneFloat("udelta", 0.f); t->dv = ps.FindOneFloat("vdelta", 0.f);
    } else
        a.Err("2D texture mapping \"" + mapping + "\" unknown");   // then `map.reset(new UVMapping2D)`: the default one
    return true;
}

// (MIPT_TEXTURES=all) the two operands of a "dots" or "checkerboard": constants only, into spec1 / spec2 (a float record's in [0])
bool TwoConstantOperands(Api &a, const std::string &name, const char *cls, bool isFloat, const TextureParams &tp, const char *n1, float d1,
                         const char *n2, float d2, mi_texture *t) {
    if (isFloat) {
        if (tp.GetFloatImageTexture(n1) >= 0 || tp.GetFloatImageTexture(n2) >= 0) {
            a.Err("Texture \"" + name + "\": a \"" + cls + "\" of image textures is outside the hot-path scope (constant " + n1 + " / " + n2 + ")");
            return false;
        }
        t->spec1[0] = tp.GetFloat(n1, d1); t->spec2[0] = tp.GetFloat(n2, d2);
        return true;
    }
    const SpectrumParam p1 = tp.GetSpectrumParam(n1, Spectrum(d1)), p2 = tp.GetSpectrumParam(n2, Spectrum(d2));
    if (p1.tex >= 0 || p2.tex >= 0) {
        a.Err("Texture \"" + name + "\": a \"" + cls + "\" of image textures is outside the hot-path scope (constant " + n1 + " / " + n2 + ")");
        return false;
    }
    CopySpectrum(p1.s, t->spec1);
    CopySpectrum(p2.s, t->spec2);
    return true;
}

// (MIPT_TEXTURES=all) Create{Dots,UV,Bilerp}{Float,Spectrum}Texture, src/textures/{dots,uv,bilerp}.cpp
bool MappedClassTexture(Api &a, const std::string &name, const std::string &texname, bool isFloat, const ParamSet &ps, const TextureParams &tp) {
    if (texname == "bilerp" && !isFloat) {
        a.Err("Texture \"" + name + "\": a spectrum \"bilerp\" is a sum of four spectra, which the two-spectrum form of a texture value on this path cannot carry; "
              "outside the hot-path scope (float \"bilerp\" only)");
        return false;
    }
    if (texname == "uv" && isFloat) return false;   // CreateUVFloatTexture returns nullptr (uv.cpp:41-44): no texture, no message
    mi_texture t{};
    t.mipmap = -1;
    t.post_scale = 1.f; t.max_aniso = 8.f;
    if (!Mapping2D(a, name, ps, &t)) return false;
    if (texname == "dots") {
        t.type = MI_TEX_DOTS;
        // DotsTexture(mapping, outsideDot, insideDot) is handed "inside" first (dots.cpp:62-66, 91-95 against dots.h:53-55):
        // spec1, the value outside the dots, is the parameter "inside"
        if (!TwoConstantOperands(a, name, "dots", isFloat, tp, "inside", 1.f, "outside", 0.f, &t)) return false;
    } else if (texname == "uv")
        t.type = MI_TEX_UV;
    else {
        t.type = MI_TEX_BILERP;
        t.bilerp[0] = ps.FindOneFloat("v00", 0.f); t.bilerp[1] = ps.FindOneFloat("v01", 1.f);
        t.bilerp[2] = ps.FindOneFloat("v10", 0.f); t.bilerp[3] = ps.FindOneFloat("v11", 1.f);
    }
    BindImageTexture(a, name, isFloat, t);
    return true;
}

// (MIPT_TEXTURES=all) CreateCheckerboard{Float,Spectrum}Texture, checkerboard.cpp:40-152, in full: float and spectrum, 2-D over
// any mapping, 3-D over IdentityMapping3D
bool CheckerboardTextureAll(Api &a, const std::string &name, bool isFloat, const ParamSet &ps, const TextureParams &tp) {
    const int dim = ps.FindOneInt("dimension", 2);
    if (dim != 2 && dim != 3) { a.Err(std::to_string(dim) + " dimensional checkerboard texture not supported"); return false; }
    mi_texture t{};
    t.mipmap = -1;
    t.su = t.sv = 1.f; t.post_scale = 1.f; t.max_aniso = 8.f;
    if (!TwoConstantOperands(a, name, "checkerboard", isFloat, tp, "tex1", 1.f, "tex2", 0.f, &t)) return false;
    if (dim == 2) {
        t.type = MI_TEX_CHECKERBOARD;
        if (!Mapping2D(a, name, ps, &t)) return false;
        const std::string aa = ps.FindOneString("aamode", "closedform");
        if (aa == "none") t.aa_none = 1;
        else if (aa != "closedform") a.Warn("Antialiasing mode \"" + aa + "\" not understood by Checkerboard2DTexture; using \"closedform\"");
    } else {
        t.type = MI_TEX_CHECKERBOARD3D;
        std::memcpy(t.w2t, a.ctm.mInv.m, sizeof(t.w2t));   // IdentityMapping3D(tex2world), as NoiseTexture
    }
    BindImageTexture(a, name, isFloat, t);
    return true;
}

// Create{FBm,Wrinkled,Windy}{Float,Spectrum}Texture, src/textures/{fbm,wrinkled,windy}.cpp
bool NoiseTexture(Api &a, const std::string &name, const std::string &texname, bool isFloat, const ParamSet &ps) {
    mi_texture t{};
    t.type = texname == "fbm" ? MI_TEX_FBM : (texname == "wrinkled" ? MI_TEX_WRINKLED : MI_TEX_WINDY);
    t.mipmap = -1;
    t.su = t.sv = 1.f; t.post_scale = 1.f; t.max_aniso = 8.f;
    t.octaves = 8; t.omega = .5f;
    if (t.type != MI_TEX_WINDY) {
        t.octaves = ps.FindOneInt("octaves", 8);
        t.omega = ps.FindOneFloat("roughness", .5f);
        if (t.octaves < 0) { a.Err("Texture \"" + name + "\": \"octaves\" " + std::to_string(t.octaves) + " is negative"); return false; }
        if (t.octaves > MI_NOISE_MAX_OCTAVES) {   // the octave loop runs per lane: keep it bounded
            a.Warn("Texture \"" + name + "\": \"octaves\" " + std::to_string(t.octaves) + " clamped to " + std::to_string(MI_NOISE_MAX_OCTAVES) + " on this path");
            t.octaves = MI_NOISE_MAX_OCTAVES;
        }
    }
    // IdentityMapping3D(tex2world): WorldToTexture = Inverse(tex2world), tex2world = the CTM here (curTransform[0], api.cpp:1233)
    std::memcpy(t.w2t, a.ctm.mInv.m, sizeof(t.w2t));
    // (it binds wherever an image texture of its type binds; the shape masks refuse it, AlphaTexture)
    if (!isFloat) a.gs.textures.scaledImageTex.erase(name);   // (this class alone also forgets a "scale" of the name)
    BindImageTexture(a, name, isFloat, t);
    return true;
}

// CreateCheckerboardSpectrumTexture, checkerboard.cpp:99-150
bool CheckerboardTexture(Api &a, const std::string &name, bool isFloat, const ParamSet &ps, const TextureParams &tp) {
    if (a.allTextures) return CheckerboardTextureAll(a, name, isFloat, ps, tp);
    if (isFloat) { a.Err("Texture \"" + name + "\": float \"checkerboard\" textures are outside the hot-path scope"); return false; }
    if (ps.FindOneInt("dimension", 2) != 2) { a.Err("Texture \"" + name + "\": 3D \"checkerboard\" textures are outside the hot-path scope"); return false; }
    const std::string mapping = ps.FindOneString("mapping", "uv");
    if (mapping != "uv") { a.Err("Texture \"" + name + "\": 2D texture mapping \"" + mapping + "\" is outside the hot-path scope (\"uv\" only)"); return false; }
    const SpectrumParam t1 = tp.GetSpectrumParam("tex1", Spectrum(1.f)), t2 = tp.GetSpectrumParam("tex2", Spectrum(0.f));
    if (t1.tex >= 0 || t2.tex >= 0) { a.Err("Texture \"" + name + "\": a \"checkerboard\" of image textures is outside the hot-path scope (constant tex1 / tex2)"); return false; }
    mi_texture t{};
    t.type = MI_TEX_CHECKERBOARD;
    t.mipmap = -1;
    t.su = ps.FindOneFloat("uscale", 1.f); t.sv = ps.FindOneFloat("vscale", 1.f);
    t.du = ps.FindOneFloat("udelta", 0.f); t.dv = ps.FindOneFloat("vdelta", 0.f);
    t.post_scale = 1.f; t.max_aniso = 8.f;
    const std::string aa = ps.FindOneString("aamode", "closedform");
    if (aa == "none") t.aa_none = 1;
    else if (aa != "closedform") a.Warn("Antialiasing mode \"" + aa + "\" not understood by Checkerboard2DTexture; using \"closedform\"");
    CopySpectrum(t1.s, t.spec1);
    CopySpectrum(t2.s, t.spec2);
    BindImageTexture(a, name, false, t);
    return true;
}

// CreateImage{Float,Spectrum}Texture, imagemap.cpp:152-197
bool ImageMapTexture(Api &a, const std::string &name, bool isFloat, const ParamSet &ps) {
    mi_texture t{};
    if (!Mapping2D(a, name, ps, &t)) return false;
    t.post_scale = 1.f;
    t.max_aniso = ps.FindOneFloat("maxanisotropy", 8.f);
    if (!(t.max_aniso <= 64.f)) {   // an EWA footprint is up to 2 x maxanisotropy texels long: keep the per-lane loop bounded
        a.Warn("Texture \"" + name + "\": \"maxanisotropy\" " + std::to_string(t.max_aniso) + " clamped to 64 on this path");
        t.max_aniso = 64.f;
    }
    const bool trilerp = ps.FindOneBool("trilinear", false), noFilt = ps.FindOneBool("noFiltering", false);
    const std::string wrap = ps.FindOneString("wrap", "repeat");
    const int wrapMode = wrap == "black" ? 1 : (wrap == "clamp" ? 2 : 0);
    const float scale = ps.FindOneFloat("scale", 1.f);
    const std::string filename = ps.FindOneString("filename", "");
    std::string ext = filename.size() >= 4 ? filename.substr(filename.size() - 4) : "";
    for (char &c : ext) c = (char)tolower(c);
    const bool gamma = ps.FindOneBool("gamma", ext == ".tga" || ext == ".png");
    if (ps.FindOneBool("useSPD", false)) a.Warn("Texture \"" + name + "\": \"useSPD\" (display primaries) is not implemented on this path; reflectance conversion used");
    // (MIPMap::Lookup: noFiltering takes the trilinear entry point, mipmap.h:283-288)
    t.filter = noFilt ? MI_TEX_NONE : (trilerp ? MI_TEX_TRILINEAR : MI_TEX_EWA);
    t.mipmap = BuildTextureMipMap(a.scene, a.AbsolutePath(filename), trilerp, noFilt, t.max_aniso, wrapMode, scale, gamma, isFloat);
    BindImageTexture(a, name, isFloat, t);   // (on this path a float image texture can be an "alpha" / "shadowalpha" mask of a mesh)
    return true;
}

void ConstantTexture(Api &a, const std::string &name, bool isFloat, const TextureParams &tp) {
    if (isFloat) a.gs.textures.floatTex[name] = tp.GetFloat("value", 1.f);
    else a.gs.textures.spectrumTex[name] = tp.GetSpectrum("value", Spectrum(1.f));
}

bool ScaleTexture(Api &a, const std::string &name, bool isFloat, const TextureParams &tp) {
    // ScaleTexture of a float image texture and a constant (the usual way to size a bump map): the image texture
    // with the constant as post-lookup factor -- tex1(si) * tex2(si), scale.h:56-58
    const int img1 = isFloat ? tp.GetFloatImageTexture("tex1") : -1, img2 = isFloat ? tp.GetFloatImageTexture("tex2") : -1;
    if (img1 >= 0 || img2 >= 0) {
        if (img1 >= 0 && img2 >= 0) { a.Err("Texture \"" + name + "\": a \"scale\" of two image textures is outside the hot-path scope"); return false; }
        mi_texture t = a.scene->textures[img1 >= 0 ? img1 : img2];
        t.post_scale = t.post_scale * tp.GetFloat(img1 >= 0 ? "tex2" : "tex1", 1.f);
        BindImageTexture(a, name, true, t);
        return true;
    }
    if (!isFloat) {   // spectrum: image texture * constant spectrum -> the lobe keeps the constant and multiplies the texture value in
        const SpectrumParam p1 = tp.GetSpectrumParam("tex1", Spectrum(1.f)), p2 = tp.GetSpectrumParam("tex2", Spectrum(1.f));
        if (p1.tex >= 0 || p2.tex >= 0) {
            if (p1.tex >= 0 && p2.tex >= 0) { a.Err("Texture \"" + name + "\": a \"scale\" of two image textures is outside the hot-path scope"); return false; }
            const SpectrumParam &img = p1.tex >= 0 ? p1 : p2, &cst = p1.tex >= 0 ? p2 : p1;
            a.gs.textures.spectrumTex.erase(name);   // (not BindImageTexture: no record of its own, the name stands for a pair)
            a.gs.textures.scaledImageTex[name] = std::make_pair(img.tex, img.scaled ? img.s * cst.s : cst.s);
            return true;
        }
    }
    if (isFloat) a.gs.textures.floatTex[name] = tp.GetFloat("tex1", 1.f) * tp.GetFloat("tex2", 1.f);
    else a.gs.textures.spectrumTex[name] = tp.GetSpectrum("tex1", Spectrum(1.f)) * tp.GetSpectrum("tex2", Spectrum(1.f));
    return true;
}

void MixTexture(Api &a, const std::string &name, bool isFloat, const TextureParams &tp) {
    const float amt = tp.GetFloat("amount", 0.5f);
    if (isFloat) a.gs.textures.floatTex[name] = (1 - amt) * tp.GetFloat("tex1", 0.f) + amt * tp.GetFloat("tex2", 1.f);
    else a.gs.textures.spectrumTex[name] = (1 - amt) * tp.GetSpectrum("tex1", Spectrum(0.f)) + amt * tp.GetSpectrum("tex2", Spectrum(1.f));
}

}  // namespace

// ------------------------------------------------------------------ the directives (Api's members)
Api::Api(HostScene *s, const LoadOverrides &o) : scene(s), ov(o) {
    if (const char *e = getenv("MIPT_INSTANCES")) expandInstances = std::string(e) == "expand";
    if (const char *e = getenv("MIPT_OBJECT_MOTION")) objectMotion = std::string(e) == "1";
    if (const char *e = getenv("MIPT_TEXTURES")) allTextures = std::string(e) == "all";
    if (const char *e = getenv("MIPT_CAMERAS")) allCameras = std::string(e) == "all";
    // default material: matte with default params (GraphicsState ctor, api.cpp:214-222)
    gs.currentMaterial = NewMaterialInstance("matte", ParamSet());
}

// The Material object of a Material / MakeNamedMaterial directive (and the default matte): one MakeMaterial call, one id.
std::shared_ptr<MaterialInstance> Api::NewMaterialInstance(const std::string &type, const ParamSet &ps) {
    auto mi = std::make_shared<MaterialInstance>();
    mi->name = type; mi->params = ps;
    mi->material = MakeMaterial(*this, type, ps, ParamSet());
    mi->id = lastMaterialId;
    return mi;
}

// `recorded`: the shape of an object is being re-created at an ObjectInstance; *recorded is the material id it took
// where it was declared.
void Api::Shape(const std::string &name, const ParamSet &params, const uint32_t *recorded) {
    if (state != World) { Err("Scene description must be inside world block; \"Shape\" not allowed. Ignoring."); return; }
    // (the reference wraps such a shape in a TransformedPrimitive with an AnimatedTransform, api.cpp:1363-1430: moving
    // primitives need per-ray times in traversal and are outside this path's scope)
    if (CtmIsAnimated() && !recorded) {
        if (objectMotion && !currentInstance) { MovingShape(*this, name, params); return; }
        // (without the switch; and a moving shape inside an object: a TransformedPrimitive inside an instance)
        Err("Shape \"" + name + "\": animated transforms of shapes are outside the hot-path scope; using the start transform");
    }
    const bool known = name == "trianglemesh" || name == "plymesh" || name == "loopsubdiv" || name == "sphere" || name == "disk";
    if (currentInstance) {   // api.cpp:1431-1435
        if (gs.areaLight != "") Warn("Area lights not supported with object instancing");
        // the reference creates the shape and its material here (GetMaterialForShape, api.cpp:1378), so the id is taken here
        // (after MakeShapes has made something, api.cpp:1370-1378: judged here by the shape's name, the shapes this front end
        // builds; a shape whose parameters turn out unusable at the ObjectInstance has taken its number all the same)
        uint32_t id = gs.currentMaterial->id;
        if (known && ShapeMaySetMaterialParameters(params)) id = TakeMaterialIds(*this, gs.currentMaterial->name, params, gs.currentMaterial->params);
        RecordedShape r{name, params, ctm, gs, id};
        r.gs.areaLight = "";
        currentInstance->push_back(std::move(r));
        return;
    }
    if (!known) { Err("Shape \"" + name + "\" is outside the PathIntegrator hot-path scope (SURVEY 2 rows 13-14); skipped."); return; }
    BuiltShape built;
    bool made;
    if (name == "trianglemesh") made = TriangleMeshShape(*this, params, &built);
    else if (name == "plymesh") made = PLYMeshShape(*this, params, &built);
    else if (name == "loopsubdiv") made = LoopSubdivShape(*this, params, &built);
    else if (name == "sphere") made = SphereShape(*this, params, &built);
    else made = DiskShape(*this, params, &built);
    if (!made) return;
    // material (api.cpp:1378, GetMaterialForShape 1502-1513)
    int material;
    uint32_t materialId = gs.currentMaterial->id;
    if (ShapeMaySetMaterialParameters(params)) {
        material = MakeMaterial(*this, gs.currentMaterial->name, params, gs.currentMaterial->params, recorded == nullptr);
        materialId = lastMaterialId;
    } else
        material = gs.currentMaterial->material;
    if (recorded) materialId = *recorded;
    AddPrims(*this, built, material, materialId);
    WarnUnused(params);
}

void Api::ObjectBegin(const std::string &name) {  // api.cpp:1544-1553
    AttributeBegin();
    if (currentInstance) Err("ObjectBegin called inside of instance definition");
    instances[name] = std::vector<RecordedShape>();
    currentInstance = &instances[name];
}

void Api::ObjectEnd() {  // api.cpp:1557-1566
    if (!currentInstance) Err("ObjectEnd called outside of instance definition");
    currentInstance = nullptr;
    AttributeEnd();
}

void Api::ObjectInstance(const std::string &name) {  // api.cpp:1570-1615
    if (currentInstance) { Err("ObjectInstance can't be called inside instance definition"); return; }
    auto it = instances.find(name);
    if (it == instances.end()) { Err("Unable to find instance named \"" + name + "\""); return; }
    // (api.cpp:1594-1610 gives the TransformedPrimitive an AnimatedTransform; see Shape)
    const bool moving = objectMotion && CtmIsAnimated();   // (a moving instance is never expanded)
    if (CtmIsAnimated() && !moving) Err("ObjectInstance \"" + name + "\": animated transforms of instances are outside the hot-path scope; using the start transform");
    const Transform instanceToWorld = ctm;
    if (expandInstances && !moving) {
        if (it->second.empty()) return;   // api.cpp:1588
        instanceNames.push_back(name);
        expandingInstance = (uint32_t)instanceNames.size();   // the copies carry the instance id themselves
        const GraphicsState saved = gs;   // (not MakeApart: the copies are the world's own primitives)
        for (const RecordedShape &r : it->second) {
            ctm = instanceToWorld * r.ctm;
            gs = r.gs;
            Shape(r.name, r.params, &r.materialId);
        }
        expandingInstance = 0;
        ctm = instanceToWorld;
        gs = saved;
        return;
    }
    ObjectDef &od = objectDefs[name];
    if (!od.created) {   // the object's shapes, once, where they were declared
        od.created = true;
        objectOrder.push_back(name);
        od.prims = MakeApart(*this, [&] {
            for (const RecordedShape &r : it->second) {
                ctm = r.ctm; gs = r.gs;
                Shape(r.name, r.params, &r.materialId);
            }
        });
        for (const PendingPrim &pp : od.prims) od.bounds = Union(od.bounds, pp.bounds);
    }
    if (od.prims.empty()) return;   // api.cpp:1580
    instanceNames.push_back(name);   // nObjectInstancesUsed / renderOptions->instanceNames, api.cpp:1589, 1614
    AddInstance(*this, name, od.bounds, instanceToWorld, moving ? ctmEnd : instanceToWorld, (uint32_t)instanceNames.size());
}

void Api::LightSource(const std::string &name, const ParamSet &ps) {  // MakeLight, api.cpp:747-771
    if (state != World) { Err("\"LightSource\" not allowed outside world block. Ignoring."); return; }
    WarnIfAnimated("LightSource");   // api.cpp:1328
    mi_light l{};
    if (name == "point") PointLight(*this, ps, &l);
    else if (name == "distant") DistantLight(*this, ps, &l);
    else if (name == "spot") SpotLight(*this, ps, &l);
    else if (name == "infinite" || name == "exinfinite") InfiniteLight(*this, ps, &l);
    else if (name == "projection") ProjectionLight(*this, ps, &l);
    else { Err("LightSource \"" + name + "\" is outside the hot-path scope (SURVEY 2 row 20); skipped."); return; }
    scene->lights.push_back(l);
    WarnUnused(ps);
}

void Api::Texture(const std::string &name, const std::string &type, const std::string &texname, const ParamSet &ps) {
    // Apart from the image and noise classes every texture on this path evaluates to a constant, so "scale" and "mix" of such
    // textures fold into constants with the reference's arithmetic (src/textures/scale.h:56-58, mix.h:57-61, scale.cpp, mix.cpp).
    const bool isNoise = texname == "fbm" || texname == "wrinkled" || texname == "windy";
    // MIPT_TEXTURES=all: "dots", "uv" and "bilerp" besides; "marble" and "ptex" stay errors, with their reasons
    const bool isMapped = allTextures && (texname == "dots" || texname == "uv" || texname == "bilerp");
    if (allTextures && texname == "marble") {
        Err("Texture class \"marble\" is outside the hot-path scope: its spline mixes FromRGB of colours that need three basis spectra plus white, "
            "more than the two-spectrum form of a texture value on this path carries");
        return;
    }
    if (allTextures && texname == "ptex") {
        Err("Texture class \"ptex\" is outside the hot-path scope: it reads per-face texture files through the Ptex library, which this path does not hold");
        return;
    }
    if (texname != "constant" && texname != "scale" && texname != "mix" && texname != "imagemap" && texname != "checkerboard" && !isNoise && !isMapped) {
        Err("Texture class \"" + texname + "\" is outside the hot-path scope (\"constant\", \"scale\", \"mix\", \"imagemap\", \"checkerboard\", \"fbm\", \"wrinkled\", \"windy\")");
        return;
    }
    ParamSet empty;
    TextureParams tp(ps, empty, gs.textures, &scene->errors);
    const bool isFloat = type == "float", isSpec = type == "color" || type == "spectrum";
    if (!isFloat && !isSpec) { Err("Texture type \"" + type + "\" unknown."); return; }
    WarnIfAnimated("Texture");   // api.cpp:1231, 1249
    bool made = true;
    if (isNoise) made = NoiseTexture(*this, name, texname, isFloat, ps);
    else if (isMapped) made = MappedClassTexture(*this, name, texname, isFloat, ps, tp);
    else if (texname == "checkerboard") made = CheckerboardTexture(*this, name, isFloat, ps, tp);
    else if (texname == "imagemap") made = ImageMapTexture(*this, name, isFloat, ps);
    else if (texname == "constant") ConstantTexture(*this, name, isFloat, tp);
    else if (texname == "scale") made = ScaleTexture(*this, name, isFloat, tp);
    else MixTexture(*this, name, isFloat, tp);
    // (these two classes alone report unused parameters, as they always have: the messages are part of the scene)
    if (made && (isNoise || texname == "imagemap")) WarnUnused(ps);
}

}  // namespace mipt
