// api.h -- internal to csrc/host: the state of the .pbrt front end, shared by its three files -- parser.cpp (text in,
// directive calls out), api.cpp (the directives: they fill `pending` and the scene arrays) and world_end.cpp (WorldEnd
// flattens everything into the HostScene). Nothing else includes it: scene.h is the front end's public face.
#pragma once
#include <map>
#include <memory>
#include "scene.h"

namespace mipt {

struct MaterialInstance {
    std::string name;  // material type
    int material = -1; // index into HostScene::materials, -1 = none
    uint32_t id = 0;   // Material::materialId of the reference's object (Api::materialCounter), 0 = none
    ParamSet params;
};

struct GraphicsState {
    TextureMaps textures;
    std::map<std::string, std::shared_ptr<MaterialInstance>> namedMaterials;
    std::shared_ptr<MaterialInstance> currentMaterial;
    ParamSet areaLightParams;
    std::string areaLight;
    bool reverseOrientation = false;
};

constexpr int kDiskBase = 1 << 30;
struct PendingPrim {
    int shape;  // >=0 tri, <0 ~sphere; a disk: ~(kDiskBase + its number) until WorldEnd knows how many spheres precede the disks
    int material;
    int light;
    Bounds3 bounds;
    int instance = 0;   // k + 1: the TransformedPrimitive of instance k
    uint32_t materialId = 0, instanceId = 0;   // mi_prim_meta
};

// AnimatedTransform::hasRotation (transform.cpp:1103-1110): the two quaternions' dot product, summed in this order.
inline bool HasRotation(const float *R0, const float *R1) {
    return (R0[0] * R1[0] + R0[1] * R1[1] + R0[2] * R1[2]) + R0[3] * R1[3] < 0.9995f;
}

struct Api {
    HostScene *scene;
    LoadOverrides ov;
    std::string baseDir;
    enum { Uninit, Options, World } state = Options;
    // The CTM is a pair (TransformSet, api.cpp:158-190): `ctm` its start member, which everything but the camera is built
    // with, `ctmEnd` its end member. A CTM directive applies to the members whose bit is set in activeBits (ActiveTransform
    // StartTime = 1, EndTime = 2, All = 3; FOR_ACTIVE_TRANSFORMS, api.cpp:426-430); the bits are pushed and popped with the pair.
    Transform ctm, ctmEnd;
    uint32_t activeBits = 3;
    float transformStart = 0.f, transformEnd = 1.f;   // TransformTimes (RenderOptions, api.cpp:168-169)
    struct PushedTransform { Transform start, end; uint32_t bits; };
    std::vector<PushedTransform> transformStack;
    std::vector<GraphicsState> gsStack;
    std::vector<char> pushKinds;
    GraphicsState gs;
    std::map<std::string, std::pair<Transform, Transform>> namedCoordSys;
    // render options (api.cpp:168-196 defaults)
    std::string filterName = "box", filmName = "image", samplerName = "halton", accelName = "bvh",
                integratorName = "path", cameraName = "perspective";
    ParamSet filterParams, filmParams, samplerParams, accelParams, integratorParams, cameraParams;
    Transform cameraToWorld, cameraToWorldEnd;
    std::vector<PendingPrim> pending;
    // Object instancing (api.cpp:1544-1615). As in the reference, an object's primitives are created once, in the space they
    // were declared in, and every ObjectInstance is a TransformedPrimitive in the world's BVH: the world-space box of the
    // object and InstanceToWorld; the object's primitives get a BVH of their own at WorldEnd. (MIPT_INSTANCES=expand
    // re-creates the recorded shapes under InstanceToWorld * (their CTM) instead -- round 1's world-space copies: the same
    // surfaces, hit points that differ from the reference's in rounding.)
    struct RecordedShape { std::string name; ParamSet params; Transform ctm; GraphicsState gs; uint32_t materialId; };
    std::map<std::string, std::vector<RecordedShape>> instances;
    std::vector<RecordedShape> *currentInstance = nullptr;
    // wrapper: the primitives of one moving Shape (api.cpp:1389-1428), behind BVHAccel's default parameters
    struct ObjectDef { std::vector<PendingPrim> prims; Bounds3 bounds; bool created = false; int root = -1; bool wrapper = false; };
    std::map<std::string, ObjectDef> objectDefs;
    std::vector<std::string> objectOrder;                 // objects in the order they were first instanced
    // moving: i2w / i2wEnd are the members of an AnimatedTransform over the TransformTimes (MIPT_OBJECT_MOTION=1)
    struct InstanceRec { std::string object; Transform i2w; uint32_t instanceId = 0; bool moving = false; Transform i2wEnd; };
    std::vector<InstanceRec> instanceRecs;
    bool objectMotion = false;   // MIPT_OBJECT_MOTION=1: shapes and instances under an animated CTM become moving primitives
    bool allTextures = false;    // MIPT_TEXTURES=all: the 2-D mappings beside "uv" and the classes "dots", "uv", "bilerp", float and 3-D "checkerboard"
    bool allCameras = false;     // MIPT_CAMERAS=all: Camera "orthographic" and "environment" are built instead of reported
    int nMovingShapes = 0;
    std::vector<std::string> instanceNames;   // one per ObjectInstance call that created something, in file order
    bool expandInstances = false;
    // Material::materialId (material.h:54): every Material object the reference constructs takes the next number of a counter
    // that starts at 1. In a `pbrt scene.pbrt` process the matte of the static GraphicsState is number 1 (api.cpp:382,
    // 214-222) and the matte of pbrtInit's fresh GraphicsState number 2 (api.cpp:902): the scene's default material, made
    // by the constructor. Then one number per MakeMaterial call that returns a material (api.cpp:552-625). Identical
    // mi_material records are shared (MakeMaterial), so the number belongs to the primitive (mi_prim_meta).
    uint32_t materialCounter = 1, lastMaterialId = 0;
    uint32_t expandingInstance = 0;   // MIPT_INSTANCES=expand: the ObjectInstance call whose copies are being created
    std::map<std::string, std::shared_ptr<PLYMeshData>> plyCache;   // an instanced plymesh is read once
    std::map<std::string, Spectrum> cachedSpectra;                  // paramset.cpp:48, SPD files by name
    bool worldEnded = false;

    Api(HostScene *s, const LoadOverrides &o);
    void Warn(const std::string &m) { scene->warnings.push_back(m); }
    void Err(const std::string &m) { scene->errors.push_back(m); }
    void WarnUnused(const ParamSet &ps) {   // ParamSet::ReportUnused, paramset.cpp:360-372
        std::vector<std::string> unused;
        ps.ReportUnused(&unused);
        for (auto &u : unused) Warn("Parameter \"" + u + "\" not used");
    }
    // FindOneFilename -> AbsolutePath(ResolveFilename()): a relative name is the scene file's neighbour; no name stays no name
    std::string AbsolutePath(const std::string &fn) const { return (!fn.empty() && fn[0] != '/') ? baseDir + "/" + fn : fn; }

    // ---- transforms and attributes
    template <typename F> void ForActiveTransforms(F f) {
        if (activeBits & 1u) ctm = f(ctm);
        if (activeBits & 2u) ctmEnd = f(ctmEnd);
    }
    void ConcatTransform(const Transform &t) { ForActiveTransforms([&](const Transform &c) { return c * t; }); }
    void PushTransform(char kind) { transformStack.push_back(PushedTransform{ctm, ctmEnd, activeBits}); pushKinds.push_back(kind); }
    void PopTransform() {
        ctm = transformStack.back().start; ctmEnd = transformStack.back().end; activeBits = transformStack.back().bits;
        transformStack.pop_back(); pushKinds.pop_back();
    }
    void AttributeBegin() { gsStack.push_back(gs); PushTransform('a'); }
    void AttributeEnd() {
        if (gsStack.empty()) { Err("Unmatched AttributeEnd encountered. Ignoring it."); return; }
        gs = gsStack.back(); gsStack.pop_back();
        PopTransform();
    }
    bool CtmIsAnimated() const { return ctm != ctmEnd; }   // TransformSet::IsAnimated, api.cpp:158-163
    void WarnIfAnimated(const char *func) {                // WARN_IF_ANIMATED_TRANSFORM, api.cpp:431-438
        if (CtmIsAnimated())
            Warn(std::string("Animated transformations set; ignoring for \"") + func + "\" and using the start transform only");
    }

    // ---- the directives the parser calls (api.cpp; WorldEnd: world_end.cpp). Their builders and stages are local to those files.
    std::shared_ptr<MaterialInstance> NewMaterialInstance(const std::string &type, const ParamSet &ps);
    void Shape(const std::string &name, const ParamSet &params, const uint32_t *recorded = nullptr);
    void ObjectBegin(const std::string &name);
    void ObjectEnd();
    void ObjectInstance(const std::string &name);
    void LightSource(const std::string &name, const ParamSet &ps);
    void Texture(const std::string &name, const std::string &type, const std::string &texname, const ParamSet &ps);
    void WorldEnd();
};

// ReadFloatFile, src/core/floatfile.cpp:40-83 (parser.cpp): SPD files and the lens file; messages go to the scene
bool ReadFloatFile(const std::string &filename, std::vector<float> *values, Api *api);

}  // namespace mipt

