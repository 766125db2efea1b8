// world_end.cpp -- WorldEnd of the .pbrt front end: what the directives collected (api.h) becomes the flat HostScene, stage
// by stage -- film, camera, sampler, integrator, sampler tables, accelerators, light preprocessing, names and constants.
// The film's resolution and sample bounds and the integrator's band count and depth reach the later stages as parameters in
// WorldEnd's body. Two records are handed on whole: the sampler tables read and may reset the sampler's type, and the light
// stage reads scene->lightStrategy, which the integrator stage set. (Reference: src/core/api.cpp:1617-1737,1750-1860.)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include "api.h"

namespace mipt {
namespace {

int RoundUpPow2(int n) {   // pbrt.h:386-394, for the counts that occur here
    int p2 = 1;
    while (p2 < n) p2 *= 2;
    return p2;
}

// The T / R / S of both members into the record that interpolates between them (mi_camera, mi_motion).
void CopyDecomposition(const AnimatedDecomposition &ad, float T[2][3], float R[2][4], float S[2][9]) {
    for (int i = 0; i < 2; ++i) {
        std::memcpy(T[i], ad.d[i].T, sizeof(ad.d[i].T));
        std::memcpy(R[i], ad.d[i].R, sizeof(ad.d[i].R));
        std::memcpy(S[i], ad.d[i].S, sizeof(ad.d[i].S));
    }
}

void EvalFilter(const std::string &name, const ParamSet &ps, float radius[2], std::vector<std::string> *warn,
                 std::function<float(float, float)> *fn) {
    // src/filters/{box,triangle,gaussian,mitchell,sinc}.cpp
    if (name == "box") {
        radius[0] = ps.FindOneFloat("xwidth", 0.5f); radius[1] = ps.FindOneFloat("ywidth", 0.5f);
        *fn = [](float, float) { return 1.f; };
    } else if (name == "triangle") {
        radius[0] = ps.FindOneFloat("xwidth", 2.f); radius[1] = ps.FindOneFloat("ywidth", 2.f);
        float rx = radius[0], ry = radius[1];
        *fn = [rx, ry](float x, float y) { return std::max((float)0, rx - std::abs(x)) * std::max((float)0, ry - std::abs(y)); };
    } else if (name == "gaussian") {
        radius[0] = ps.FindOneFloat("xwidth", 2.f); radius[1] = ps.FindOneFloat("ywidth", 2.f);
        float alpha = ps.FindOneFloat("alpha", 2.f);
        float expX = std::exp(-alpha * radius[0] * radius[0]), expY = std::exp(-alpha * radius[1] * radius[1]);
        *fn = [alpha, expX, expY](float x, float y) {
            auto g = [alpha](float d, float expv) { return std::max((float)0, float(std::exp(-alpha * d * d) - expv)); };
            return g(x, expX) * g(y, expY);
        };
    } else if (name == "mitchell") {
        radius[0] = ps.FindOneFloat("xwidth", 2.f); radius[1] = ps.FindOneFloat("ywidth", 2.f);
        float B = ps.FindOneFloat("B", 1.f / 3.f), C = ps.FindOneFloat("C", 1.f / 3.f);
        float irx = 1 / radius[0], iry = 1 / radius[1];
        *fn = [B, C, irx, iry](float x, float y) {
            auto m1 = [B, C](float x) {
                x = std::abs(2 * x);
                if (x > 1)
                    return ((-B - 6 * C) * x * x * x + (6 * B + 30 * C) * x * x + (-12 * B - 48 * C) * x + (8 * B + 24 * C)) * (1.f / 6.f);
                else
                    return ((12 - 9 * B - 6 * C) * x * x * x + (-18 + 12 * B + 6 * C) * x * x + (6 - 2 * B)) * (1.f / 6.f);
            };
            return m1(x * irx) * m1(y * iry);
        };
    } else if (name == "sinc") {
        radius[0] = ps.FindOneFloat("xwidth", 4.); radius[1] = ps.FindOneFloat("ywidth", 4.);
        float tau = ps.FindOneFloat("tau", 3.f);
        float rx = radius[0], ry = radius[1];
        *fn = [tau, rx, ry](float x, float y) {
            auto sinc = [](float x) { x = std::abs(x); if (x < 1e-5) return 1.f; return std::sin(kPi * x) / (kPi * x); };
            auto ws = [&](float x, float r) { x = std::abs(x); if (x > r) return 0.f; float l = sinc(x / tau); return sinc(x) * l; };
            return ws(x, rx) * ws(y, ry);
        };
    } else {
        warn->push_back("Filter \"" + name + "\" unknown.");
        EvalFilter("box", ps, radius, warn, fn);
    }
}

// CreateFilm, film.cpp:313-352; Film ctor film.cpp:50-83
float CreateFilm(Api &a, mi_film &f) {
    float radius[2];
    std::function<float(float, float)> fn;
    EvalFilter(a.filterName, a.filterParams, radius, &a.scene->warnings, &fn);
    if (a.filmName != "image") a.Err("Film \"" + a.filmName + "\" unknown.");
    a.scene->filmFilename = a.filmParams.FindOneString("filename", "");
    if (a.scene->filmFilename == "") a.scene->filmFilename = "pbrt.exr";
    int xres = a.filmParams.FindOneInt("xresolution", 1280);
    int yres = a.filmParams.FindOneInt("yresolution", 720);
    if (a.ov.xres > 0) xres = a.ov.xres;
    if (a.ov.yres > 0) yres = a.ov.yres;
    float crop[4] = {0, 1, 0, 1};
    const std::vector<float> *cr = ParamSet::Find(a.filmParams.floats, "cropwindow");
    if (cr && cr->size() == 4) {
        crop[0] = Clamp(std::min((*cr)[0], (*cr)[1]), 0.f, 1.f);
        crop[1] = Clamp(std::max((*cr)[0], (*cr)[1]), 0.f, 1.f);
        crop[2] = Clamp(std::min((*cr)[2], (*cr)[3]), 0.f, 1.f);
        crop[3] = Clamp(std::max((*cr)[2], (*cr)[3]), 0.f, 1.f);
    } else if (cr)
        a.Err("values supplied for \"cropwindow\". Expected 4.");
    if (a.ov.crop[0] >= 0) for (int i = 0; i < 4; ++i) crop[i] = a.ov.crop[i];
    f.scale = a.filmParams.FindOneFloat("scale", 1.);
    const float diagonal = (float)(a.filmParams.FindOneFloat("diagonal", 35.) * .001);   // Film::diagonal(diagonal * .001), film.cpp:54: a double product rounded to float
    f.max_sample_luminance = a.filmParams.FindOneFloat("maxsampleluminance", kInfinity);
    a.scene->spectralFlag = a.filmParams.FindOneBool("spectralFlag", true);
    f.full_res[0] = xres; f.full_res[1] = yres;
    f.cropped_bounds[0] = (int)std::ceil(xres * crop[0]);
    f.cropped_bounds[1] = (int)std::ceil(yres * crop[2]);
    f.cropped_bounds[2] = (int)std::ceil(xres * crop[1]);
    f.cropped_bounds[3] = (int)std::ceil(yres * crop[3]);
    f.filter_radius[0] = radius[0]; f.filter_radius[1] = radius[1];
    int offset = 0;
    for (int y = 0; y < 16; ++y)
        for (int x = 0; x < 16; ++x, ++offset) {
            float px = (x + 0.5f) * radius[0] / 16;
            float py = (y + 0.5f) * radius[1] / 16;
            f.filter_table[offset] = fn(px, py);
        }
    // GetSampleBounds, film.cpp:85-92
    f.sample_bounds[0] = (int)std::floor(float(f.cropped_bounds[0]) + 0.5f - radius[0]);
    f.sample_bounds[1] = (int)std::floor(float(f.cropped_bounds[1]) + 0.5f - radius[1]);
    f.sample_bounds[2] = (int)std::ceil(float(f.cropped_bounds[2]) - 0.5f + radius[0]);
    f.sample_bounds[3] = (int)std::ceil(float(f.cropped_bounds[3]) - 0.5f + radius[1]);
    return diagonal;
}

// CreateRealisticCamera, src/cameras/realistic.cpp:934-989 (the shutter is the caller's: it is parsed the same way for both
// cameras). An error leaves the scene with the perspective stand-in and the message.
void CreateRealisticCamera(Api &a, const ParamSet &ps, const int fullRes[2], float diagonal, mi_scene_desc *d) {
    const std::string lensFile = a.AbsolutePath(ps.FindOneString("lensfile", ""));
    const float apertureDiameter = ps.FindOneFloat("aperturediameter", 1.0);
    const float focusDistance = ps.FindOneFloat("focusdistance", 10.0);
    const bool simpleWeighting = ps.FindOneBool("simpleweighting", true);
    const bool noWeighting = ps.FindOneBool("noweighting", false);
    if (lensFile == "") { a.Err("No lens description file supplied!"); return; }
    std::vector<float> lensData;
    if (!ReadFloatFile(lensFile, &lensData, &a)) { a.Err("Error reading lens specification file \"" + lensFile + "\"."); return; }
    if (lensData.size() % 4 != 0) {
        if (lensData.size() % 4 == 1) {
            a.Warn("Extra value in lens specification file, this lens file may be for pbrt-v2-spectral. Removing extra value to make it compatible with pbrt-v3-spectral...");
            lensData.erase(lensData.begin());
        } else {
            a.Err("Excess values in lens specification file \"" + lensFile + "\"; must be multiple-of-four values, read " +
                std::to_string((int)lensData.size()) + ".");
            return;
        }
    }
    const float filmDistance = ps.FindOneFloat("filmdistance", 0);
    const bool caFlag = ps.FindOneBool("chromaticAberrationEnabled", false);
    mi_lens lens{};
    std::string err;
    if (!BuildRealisticLens(lensData, apertureDiameter, filmDistance, focusDistance, diagonal, fullRes, &lens, &a.scene->warnings, &err)) {
        a.Err(err);
        return;
    }
    lens.simple_weighting = simpleWeighting ? 1 : 0;
    lens.no_weighting = noWeighting ? 1 : 0;
    lens.chromatic_aberration = caFlag ? 1 : 0;
    if (simpleWeighting)
        a.Warn("\"simpleweighting\" option with RealisticCamera no longer necessarily matches regular camera images. Further, pixel "
             "values will vary a bit depending on the aperture size.");
    a.scene->lensStore.assign(1, lens);
    d->camera_type = MI_CAMERA_REALISTIC;
    // (the camera sample's lens dimensions are evaluated for a camera with a lens: mi_camera)
    d->camera.lens_radius = lens.elements[lens.n_elements - 1][3];
    d->camera.focal_distance = focusDistance;
}

// CreatePerspectiveCamera, perspective.cpp:235-285; ProjectiveCamera ctor camera.h:91-112. Writes d->camera and d->camera_type.
// MIPT_CAMERAS=all: CreateOrthographicCamera (orthographic.cpp:123-164) and CreateEnvironmentCamera (environment.cpp:107-158)
// besides; they read the shutter, the frame and the screen window as the perspective camera does.
void CreateCamera(Api &a, const int fullRes[2], float filmDiagonal, mi_scene_desc *d) {
    const bool ortho = a.allCameras && a.cameraName == "orthographic", env = a.allCameras && a.cameraName == "environment";
    if (a.cameraName != "perspective" && a.cameraName != "realistic" && !ortho && !env)
        a.Err("Camera \"" + a.cameraName + "\" is outside the hot-path scope (SURVEY 2 row 25); using perspective.");
    const ParamSet &ps = a.cameraParams;
    mi_camera &cam = d->camera;
    float shutteropen = ps.FindOneFloat("shutteropen", 0.f);
    float shutterclose = ps.FindOneFloat("shutterclose", 1.f);
    if (shutterclose < shutteropen) { a.Warn("Shutter close time < shutter open. Swapping them."); std::swap(shutterclose, shutteropen); }
    float frame = ps.FindOneFloat("frameaspectratio", float(fullRes[0]) / float(fullRes[1]));
    float screen[4];  // xmin xmax ymin ymax
    if (frame > 1.f) { screen[0] = -frame; screen[1] = frame; screen[2] = -1.f; screen[3] = 1.f; }
    else { screen[0] = -1.f; screen[1] = 1.f; screen[2] = -1.f / frame; screen[3] = 1.f / frame; }
    const std::vector<float> *sw = ParamSet::Find(ps.floats, "screenwindow");
    if (sw) {
        if (sw->size() == 4) for (int i = 0; i < 4; ++i) screen[i] = (*sw)[i];
        else a.Err("\"screenwindow\" should have four values");
    }
    float fov = ps.FindOneFloat("fov", 90.);
    float halffov = ps.FindOneFloat("halffov", -1.f);
    if (halffov > 0.f) fov = 2.f * halffov;
    Transform cameraToScreen = Perspective(fov, 1e-2f, 1000.f);
    Transform screenToRaster = Scale((float)fullRes[0], (float)fullRes[1], 1) *
                               Scale(1 / (screen[1] - screen[0]), 1 / (screen[2] - screen[3]), 1) *
                               Translate(Vec3(-screen[0], -screen[3], 0));
    Transform rasterToScreen = Inverse(screenToRaster);
    // (OrthographicCamera: ProjectiveCamera(CameraToWorld, Orthographic(0, 1), ...), orthographic.h:57-59; "fov" is not read)
    if (ortho) cameraToScreen = Orthographic(0, 1);
    Transform rasterToCamera = Inverse(cameraToScreen) * rasterToScreen;
    std::memcpy(cam.raster_to_camera, rasterToCamera.m.m, sizeof(float) * 16);
    std::memcpy(cam.camera_to_world, a.cameraToWorld.m.m, sizeof(float) * 16);
    // AnimatedTransform(&CameraToWorld[0], transformStartTime, &CameraToWorld[1], transformEndTime) (api.cpp:814-832)
    std::memcpy(cam.camera_to_world_end, a.cameraToWorldEnd.m.m, sizeof(float) * 16);
    cam.transform_start = a.transformStart;
    cam.transform_end = a.transformEnd;
    cam.animated = a.cameraToWorld != a.cameraToWorldEnd ? 1 : 0;
    if (cam.animated) CopyDecomposition(DecomposePair(a.cameraToWorld, a.cameraToWorldEnd), cam.T, cam.R, cam.S);
    cam.lens_radius = ps.FindOneFloat("lensradius", 0.f);
    cam.focal_distance = ps.FindOneFloat("focaldistance", 1e6);
    cam.shutter_open = shutteropen;
    cam.shutter_close = shutterclose;
    d->camera_type = MI_CAMERA_PERSPECTIVE;
    d->env_ipd = 0.f; d->env_pole_merge_to = 90.f; d->env_pole_merge_from = 90.f; d->env_convergence_distance = kInfinity;
    if (ortho) d->camera_type = MI_CAMERA_ORTHOGRAPHIC;
    if (env) {   // "lensradius" and "focaldistance" are parsed and unused (environment.cpp:153-154): no lens dimensions are evaluated
        d->camera_type = MI_CAMERA_ENVIRONMENT;
        cam.lens_radius = 0.f;
        cam.focal_distance = ps.FindOneFloat("focaldistance", 1e30f);
        d->env_ipd = ps.FindOneFloat("ipd", 0.f);
        d->env_pole_merge_to = ps.FindOneFloat("poleMergeAngleTo", 90.f);
        d->env_pole_merge_from = ps.FindOneFloat("poleMergeAngleFrom", 90.f);
        d->env_convergence_distance = ps.FindOneFloat("convergencedistance", kInfinity);
    }
    if (a.cameraName == "realistic") CreateRealisticCamera(a, ps, fullRes, filmDiagonal, d);
    if (a.cameraToWorld.HasScale()) a.Warn("Scaling detected in world-to-camera transformation!");
}

// CreateHaltonSampler + ctor, halton.cpp:65-96,133-140, and the other samplers' Create routines
void CreateSampler(Api &a, const int sampleBounds[4], mi_sampler &s) {
    a.scene->samplerName = a.samplerName;
    s.type = MI_SAMPLER_HALTON;
    if (a.samplerName == "sobol") s.type = MI_SAMPLER_SOBOL;          // CreateSobolSampler, sobol.cpp:66-71
    else if (a.samplerName == "random") s.type = MI_SAMPLER_RANDOM;   // CreateRandomSampler, random.cpp:62-65
    else if (a.samplerName == "02sequence" || a.samplerName == "lowdiscrepancy") s.type = MI_SAMPLER_ZEROTWO;   // api.cpp:859-860
    else if (a.samplerName == "stratified") s.type = MI_SAMPLER_STRATIFIED;
    else if (a.samplerName != "halton")
        a.Err("Sampler \"" + a.samplerName + "\" is not built on this path (SURVEY 2: \"maxmindist\" is outside the hot-path scope); using halton.");
    int nsamp = a.samplerParams.FindOneInt("pixelsamples", s.type == MI_SAMPLER_RANDOM ? 4 : 16);
    if (a.ov.spp > 0) nsamp = a.ov.spp;
    if (s.type == MI_SAMPLER_SOBOL) {   // GlobalSampler(RoundUpPow2(samplesPerPixel)), sobol.h:52-57
        const int p2 = RoundUpPow2(nsamp);
        if (p2 != nsamp) a.Warn("Non power-of-two sample count rounded up to " + std::to_string(p2) + " for SobolSampler.");
        nsamp = p2;
    }
    s.pixel_dims = 0; s.x_samples = s.y_samples = 0; s.jitter = 1;
    if (s.type == MI_SAMPLER_ZEROTWO) {   // ZeroTwoSequenceSampler ctor + CreateZeroTwoSequenceSampler, zerotwosequence.cpp:43-51,77-82
        const int p2 = RoundUpPow2(nsamp);
        if (p2 != nsamp) a.Warn("Pixel samples being rounded up to power of 2 (from " + std::to_string(nsamp) + " to " + std::to_string(p2) + ").");
        nsamp = p2;
        s.pixel_dims = a.samplerParams.FindOneInt("dimensions", 4);
    }
    if (s.type == MI_SAMPLER_STRATIFIED) {   // CreateStratifiedSampler, stratified.cpp:79-86
        s.jitter = a.samplerParams.FindOneBool("jitter", true) ? 1 : 0;
        s.x_samples = a.samplerParams.FindOneInt("xsamples", 4);
        s.y_samples = a.samplerParams.FindOneInt("ysamples", 4);
        if (a.ov.spp > 0) {   // a sample-count override keeps the pixel's grid square-ish: the largest divisor of spp below its root
            int xs = 1;
            for (int k = 1; (long long)k * k <= a.ov.spp; ++k) if (a.ov.spp % k == 0) xs = k;
            s.x_samples = a.ov.spp / xs; s.y_samples = xs;
        }
        if (s.x_samples < 1 || s.y_samples < 1) { a.Err("Sampler \"stratified\": xsamples and ysamples must be positive; using 1."); s.x_samples = std::max(1, s.x_samples); s.y_samples = std::max(1, s.y_samples); }
        nsamp = s.x_samples * s.y_samples;
        s.pixel_dims = a.samplerParams.FindOneInt("dimensions", 4);
    }
    if (s.pixel_dims < 0 || s.pixel_dims > 64) { a.Err("Sampler \"" + a.samplerName + "\": dimensions must be in [0, 64]; using 4."); s.pixel_dims = 4; }
    s.samples_per_pixel = nsamp;
    s.sample_at_pixel_center = a.samplerParams.FindOneBool("samplepixelcenter", false) ? 1 : 0;
    int res[2] = {sampleBounds[2] - sampleBounds[0], sampleBounds[3] - sampleBounds[1]};
    const int kMaxResolution = 128;
    for (int i = 0; i < 2; ++i) {
        int base = (i == 0) ? 2 : 3;
        int scale = 1, exp = 0;
        while (scale < std::min(res[i], kMaxResolution)) { scale *= base; ++exp; }
        s.base_scales[i] = scale;
        s.base_exponents[i] = exp;
    }
    s.sample_stride = s.base_scales[0] * s.base_scales[1];
    auto extendedGCD = [](auto &&self, uint64_t a, uint64_t b, int64_t *x, int64_t *y) -> void {
        if (b == 0) { *x = 1; *y = 0; return; }
        int64_t dd = a / b, xp, yp;
        self(self, b, a % b, &xp, &yp);
        *x = yp;
        *y = xp - (dd * yp);
    };
    auto multInv = [&](int64_t a, int64_t n) {
        int64_t x, y;
        extendedGCD(extendedGCD, a, n, &x, &y);
        int64_t r = x - (x / n) * n;  // Mod(), pbrt.h:317-320
        return (int)((r < 0) ? r + n : r);
    };
    s.mult_inverse[0] = multInv(s.base_scales[1], s.base_scales[0]);
    s.mult_inverse[1] = multInv(s.base_scales[0], s.base_scales[1]);
}

// CreatePathIntegrator, path.cpp:190-213
void CreateIntegrator(Api &a, const int sampleBounds[4], mi_integrator &it) {
    a.scene->integratorName = a.integratorName;
    if (a.integratorName != "path" && a.integratorName != "spectralpath" && a.integratorName != "metadata")
        a.Err("Integrator \"" + a.integratorName + "\" is outside the hot-path scope (SURVEY 2 row 7); using path.");
    it.n_ca_bands = 1;
    it.kind = MI_INTEGRATOR_PATH;
    it.metadata_strategy = MI_METADATA_DEPTH;
    if (a.integratorName == "metadata") {  // CreateMetadataIntegrator, metadata.cpp:91-111
        it.kind = MI_INTEGRATOR_METADATA;
        const std::string st = a.integratorParams.FindOneString("strategy", "depth");
        if (st == "depth") it.metadata_strategy = MI_METADATA_DEPTH;
        else if (st == "material") it.metadata_strategy = MI_METADATA_MATERIAL;
        else if (st == "mesh") it.metadata_strategy = MI_METADATA_MESH;
        else if (st == "coordinates") it.metadata_strategy = MI_METADATA_COORDINATES;
        else a.Warn("Strategy \"" + st + "\" for metadata unknown. Using \"depth\".");
    }
    if (a.integratorName == "spectralpath") {  // CreateSpectralPathIntegrator, spectralpath.cpp:342-376
        it.n_ca_bands = a.integratorParams.FindOneInt("numCABands", 4);
        if (it.n_ca_bands < 1) { a.Err("\"numCABands\" must be at least 1."); it.n_ca_bands = 1; }
        if (it.n_ca_bands != 1)
            a.Warn("Using spectral rendering. For every pixel sample we will trace " + std::to_string(it.n_ca_bands) +
                 "x more rays. Rendering will be " + std::to_string(it.n_ca_bands) + " times slower.");
    }
    it.max_depth = a.integratorParams.FindOneInt("maxdepth", 5);
    if (a.ov.maxDepth >= 0) it.max_depth = a.ov.maxDepth;
    for (int i = 0; i < 4; ++i) it.pixel_bounds[i] = sampleBounds[i];
    const std::vector<int> *pb = ParamSet::Find(a.integratorParams.ints, "pixelbounds");
    if (pb) {
        if (pb->size() != 4) a.Err("Expected four values for \"pixelbounds\" parameter.");
        else {
            it.pixel_bounds[0] = std::max(it.pixel_bounds[0], (*pb)[0]);
            it.pixel_bounds[1] = std::max(it.pixel_bounds[1], (*pb)[2]);
            it.pixel_bounds[2] = std::min(it.pixel_bounds[2], (*pb)[1]);
            it.pixel_bounds[3] = std::min(it.pixel_bounds[3], (*pb)[3]);
            if ((it.pixel_bounds[2] - it.pixel_bounds[0]) * (it.pixel_bounds[3] - it.pixel_bounds[1]) == 0)
                a.Err("Degenerate \"pixelbounds\" specified.");
        }
    }
    it.rr_threshold = a.integratorParams.FindOneFloat("rrthreshold", 1.);
    a.scene->lightStrategy = a.integratorParams.FindOneString("lightsamplestrategy", "spatial");
    if (!a.ov.lightStrategy.empty()) a.scene->lightStrategy = a.ov.lightStrategy;
}

// Halton tables: 5 camera dims + per path and bounce 7 (+1 RR) for bounces 0..maxDepth-1; for Sampler "sobol" its matrices
// as well (a film beyond them takes the sampler back to halton). Reads s->type, writes the dimension counts.
void ComputeSamplerTables(Api &a, const int sampleBounds[4], int nCABands, int maxDepth, mi_sampler *s) {
    int nDims = 5 + nCABands * 8 * (maxDepth + 1) + 8;
    nDims = std::max(64, std::min(nDims, 1000));  // PrimeTableSize = 1000
    ComputeHaltonTables(nDims, &a.scene->primes, &a.scene->primeSums, &a.scene->perms);
    s->n_dims = nDims;
    if (s->type == MI_SAMPLER_SOBOL) {
        const int extent = std::max(sampleBounds[2] - sampleBounds[0], sampleBounds[3] - sampleBounds[1]);
        const int nSobol = std::min(nDims, 1024);   // NumSobolDimensions, sobolmatrices.h:47
        if (!ComputeSobolTables(extent, nSobol, a.scene, &s->sobol_resolution, &s->sobol_log2_resolution)) {
            a.Err("Sampler \"sobol\": film resolution beyond the tabulated pixel-index matrices; using halton.");
            s->type = MI_SAMPLER_HALTON;
        } else s->n_sobol_dims = nSobol;
    }
}

// The primitives of one tree in its leaf order, appended to mi_prim and mi_prim_meta (an object's carry instance 0 and id 0).
void AppendPrims(Api &a, const std::vector<PendingPrim> &from, const std::vector<int> &order) {
    for (int k : order) {
        const PendingPrim &pp = from[k];
        mi_prim p{};
        p.shape = pp.shape; p.material = pp.material; p.area_light = pp.light; p.instance = pp.instance;
        a.scene->prims.push_back(p);
        a.scene->primMeta.push_back(mi_prim_meta{pp.materialId, pp.instanceId});
    }
}

bool BuildWorldTree(Api &a, SplitMethod method, int maxPrims, std::string *err) {
    std::vector<Bounds3> bounds(a.pending.size());
    for (size_t i = 0; i < a.pending.size(); ++i) bounds[i] = a.pending[i].bounds;
    std::vector<int> order;
    bool ok = true;
    const auto tb0 = std::chrono::steady_clock::now();
    if (method == SplitMethod::HLBVH) {
        // on the device when there is one (mi_bvh_build_hlbvh); the host restatement builds the same tree, node for node
        std::string why;
        double secs = 0;
        const char *where = getenv("MIPT_HLBVH");   // "host": do not try the device
        DeviceBuild dev = DeviceBuild::Unavailable;
        if (!(where && std::string(where) == "host"))
            dev = BuildHLBVHOnDevice(bounds, maxPrims, 0, &a.scene->nodes, &order, &a.scene->stats.interiorNodes, &a.scene->stats.leafNodes, &secs, &why);
        const bool onDevice = dev == DeviceBuild::Built;
        if (dev == DeviceBuild::Failed) { ok = false; *err = "Accelerator \"bvh\" \"hlbvh\" (device build): " + why; }
        else if (!onDevice) ok = BuildHLBVH(bounds, maxPrims, &a.scene->nodes, &order, &a.scene->stats.interiorNodes, &a.scene->stats.leafNodes, err);
        a.scene->hlbvhOnDevice = onDevice;
        if (getenv("MIPT_TIMING")) fprintf(stderr, "[mipt] HLBVH on the %s%s%s\n", onDevice ? "device" : "host", onDevice ? "" : ": ", onDevice ? "" : why.c_str());
    } else
        ok = BuildBVH(bounds, maxPrims, method, &a.scene->nodes, &order, &a.scene->stats.interiorNodes, &a.scene->stats.leafNodes, err);
    if (getenv("MIPT_TIMING"))
        fprintf(stderr, "[mipt] BVH build over %zu primitives: %.3f s\n", bounds.size(),
                std::chrono::duration<double>(std::chrono::steady_clock::now() - tb0).count());
    if (ok) AppendPrims(a, a.pending, order);
    return ok;
}

// The objects' own BVHs (MakeAccelerator over the object's primitives at its first ObjectInstance, api.cpp:1583-1590),
// appended to the node and primitive arrays with absolute offsets; ObjectDef::root is where an instance enters.
bool BuildObjectTrees(Api &a, SplitMethod method, int maxPrims, std::string *err) {
    for (const std::string &name : a.objectOrder) {
        Api::ObjectDef &od = a.objectDefs[name];
        if (od.prims.empty()) continue;
        std::vector<Bounds3> ob(od.prims.size());
        for (size_t i = 0; i < od.prims.size(); ++i) ob[i] = od.prims[i].bounds;
        std::vector<mi_bvh_node> onodes;
        std::vector<int> oorder;
        int oi = 0, ol = 0;
        bool ok;
        if (od.wrapper) ok = BuildBVH(ob, 1, SplitMethod::SAH, &onodes, &oorder, &oi, &ol, err);   // std::make_shared<BVHAccel>(prims), api.cpp:1423
        else
            ok = method == SplitMethod::HLBVH ? BuildHLBVH(ob, maxPrims, &onodes, &oorder, &oi, &ol, err)
                                              : BuildBVH(ob, maxPrims, method, &onodes, &oorder, &oi, &ol, err);
        if (!ok) return false;
        const int baseNode = (int)a.scene->nodes.size(), basePrim = (int)a.scene->prims.size();
        for (mi_bvh_node &n : onodes) n.offset += (n.n_prims > 0) ? basePrim : baseNode;
        a.scene->nodes.insert(a.scene->nodes.end(), onodes.begin(), onodes.end());
        AppendPrims(a, od.prims, oorder);
        od.root = baseNode;
        a.scene->stats.interiorNodes += oi;
        a.scene->stats.leafNodes += ol;
    }
    return true;
}

// The quadrics share one index space, spheres first: a disk's number is known now that every sphere has been seen.
void RenumberQuadrics(Api &a) {
    const int nSph = (int)a.scene->spheres.size();
    for (mi_prim &p : a.scene->prims)
        if (p.shape < 0 && ~p.shape >= kDiskBase) p.shape = ~(~p.shape - kDiskBase + nSph);
    for (mi_light &l : a.scene->lights)
        if (l.type == MI_LIGHT_DIFFUSE_AREA && l.shape < 0 && ~l.shape >= kDiskBase) l.shape = ~(~l.shape - kDiskBase + nSph);
}

// The instances that point at the objects' trees, and the AnimatedTransforms of the moving ones.
void CreateInstances(Api &a) {
    for (const Api::InstanceRec &ir : a.instanceRecs) {
        mi_instance mi{};
        std::memcpy(mi.i2w, ir.i2w.m.m, sizeof(float) * 16);
        std::memcpy(mi.w2i, ir.i2w.mInv.m, sizeof(float) * 16);
        mi.root = (uint32_t)a.objectDefs[ir.object].root;
        mi.instance_id = ir.instanceId;
        if (ir.moving) {   // AnimatedTransform(&InstanceToWorld[0], transformStartTime, &InstanceToWorld[1], transformEndTime)
            mi_motion mo{};
            std::memcpy(mo.i2w_end, ir.i2wEnd.m.m, sizeof(float) * 16);
            std::memcpy(mo.w2i_end, ir.i2wEnd.mInv.m, sizeof(float) * 16);
            CopyDecomposition(DecomposePair(ir.i2w, ir.i2wEnd), mo.T, mo.R, mo.S);
            mo.transform_start = a.transformStart; mo.transform_end = a.transformEnd;
            mo.has_rotation = HasRotation(mo.R[0], mo.R[1]) ? 1 : 0;
            a.scene->motions.push_back(mo);
            mi.motion = (uint32_t)a.scene->motions.size();
        }
        a.scene->instances.push_back(mi);
    }
}

// CreateBVHAccelerator, bvh.cpp:740-762. A build that refuses its input (a leaf beyond a node's 16-bit count) is an error of
// the scene, which is left without tree and primitives: reported, never a wrapped count, never another builder's tree.
void BuildAccelerators(Api &a) {
    if (a.accelName != "bvh") a.Err("Accelerator \"" + a.accelName + "\" is outside the hot-path scope (SURVEY 2 row 9); using bvh.");
    std::string sm = a.accelParams.FindOneString("splitmethod", "sah");
    SplitMethod method = SplitMethod::SAH;
    if (sm == "middle") method = SplitMethod::Middle;
    else if (sm == "equal") method = SplitMethod::EqualCounts;
    else if (sm == "hlbvh") method = SplitMethod::HLBVH;
    else if (sm != "sah") a.Warn("BVH split method \"" + sm + "\" unknown.  Using \"sah\".");
    int maxPrims = a.accelParams.FindOneInt("maxnodeprims", 4);
    std::string err;
    const bool ok = BuildWorldTree(a, method, maxPrims, &err) && BuildObjectTrees(a, method, maxPrims, &err);
    if (!ok) {
        a.Err(err);
        a.scene->nodes.clear(); a.scene->prims.clear(); a.scene->primMeta.clear();
        a.scene->hlbvhOnDevice = false;
        a.scene->stats.interiorNodes = a.scene->stats.leafNodes = 0;
    }
    RenumberQuadrics(a);
    if (ok) CreateInstances(a);
}

// Light::Preprocess (distant.h:52-54: the world's bounding sphere) and the light-selection distribution
void PreprocessLights(Api &a) {
    Bounds3 wb;
    if (!a.scene->nodes.empty()) {
        wb.pMin = Vec3(a.scene->nodes[0].bmin[0], a.scene->nodes[0].bmin[1], a.scene->nodes[0].bmin[2]);
        wb.pMax = Vec3(a.scene->nodes[0].bmax[0], a.scene->nodes[0].bmax[1], a.scene->nodes[0].bmax[2]);
    }
    Vec3 c;
    float r;
    wb.BoundingSphere(&c, &r);
    for (auto &l : a.scene->lights) {
        l.world_radius = r;
        l.world_center[0] = c.x; l.world_center[1] = c.y; l.world_center[2] = c.z;
    }
    if (a.scene->lights.empty())
        a.Warn("No light sources defined in scene; rendering a black image.");
    BuildLightDistribution(a.scene, a.scene->lightStrategy);
}

// The names behind the ids (written at WorldEnd by the reference, api.cpp:1654-1681: the instance names in file order, the
// named materials of the graphics state WorldEnd finds, in std::map order), the counts and the colour-matching tables.
void NamesAndConstants(Api &a, mi_scene_desc *d) {
    a.scene->instanceNames = a.instanceNames;
    for (const auto &nm : a.gs.namedMaterials) { a.scene->namedMaterialNames.push_back(nm.first); a.scene->namedMaterialIds.push_back(nm.second->id); }
    a.scene->stats.nLights = (int)a.scene->lights.size();
    a.scene->stats.nMaterials = (int)a.scene->materials.size();
    const float *Y = Spectrum::CIE_Y();
    for (int i = 0; i < MI_NSPEC; ++i) d->cie_y[i] = Y[i];
    for (int k = 0; k < 7; ++k) {
        const float *basis = Spectrum::RGBIllumBasis(k);
        for (int i = 0; i < MI_NSPEC; ++i) d->rgb_illum[k][i] = basis[i];
    }
}

}  // namespace

void Api::WorldEnd() {
    worldEnded = true;
    mi_scene_desc &d = scene->desc;
    const float filmDiagonal = CreateFilm(*this, d.film);
    CreateCamera(*this, d.film.full_res, filmDiagonal, &d);
    CreateSampler(*this, d.film.sample_bounds, d.sampler);
    CreateIntegrator(*this, d.film.sample_bounds, d.integrator);
    ComputeSamplerTables(*this, d.film.sample_bounds, d.integrator.n_ca_bands, d.integrator.max_depth, &d.sampler);
    BuildAccelerators(*this);
    PreprocessLights(*this);
    NamesAndConstants(*this, &d);
    scene->Finalize();
}

void HostScene::Finalize() {
    mi_scene_desc &d = desc;
    d.abi_version = MI_ABI_VERSION;
    mipmaps.clear();
    for (const HostMipMap &h : mipStore) {
        mi_mipmap m{};
        m.n_levels = (int)h.levelOffset.size(); m.wrap = h.wrap; m.width = h.width; m.height = h.height;
        m.texels = h.texels.data();
        for (size_t l = 0; l < h.levelOffset.size() && l < MI_MAX_MIP_LEVELS; ++l) m.level_offset[l] = h.levelOffset[l];
        mipmaps.push_back(m);
    }
    d.n_mipmaps = (uint32_t)mipmaps.size();
    d.mipmaps = mipmaps.empty() ? nullptr : mipmaps.data();
    d.n_textures = (uint32_t)textures.size();
    d.textures = textures.empty() ? nullptr : textures.data();
    envmaps.clear();
    for (const HostEnvMap &e : envStore) {
        mi_envmap m{};
        m.width = e.width; m.height = e.height; m.rgb = e.rgb.data();
        m.nu = e.nu; m.nv = e.nv;
        m.cond_func = e.condFunc.data(); m.cond_cdf = e.condCdf.data(); m.cond_func_int = e.condFuncInt.data();
        m.marg_func = e.margFunc.data(); m.marg_cdf = e.margCdf.data(); m.marg_func_int = e.margFuncInt;
        if (e.nu == 0 && e.nv == 0)   // a projection light's map: the image alone
            m.cond_func = m.cond_cdf = m.cond_func_int = m.marg_func = m.marg_cdf = nullptr;
        envmaps.push_back(m);
    }
    d.n_envmaps = (uint32_t)envmaps.size();
    d.envmaps = envmaps.empty() ? nullptr : envmaps.data();
    d.n_nodes = (uint32_t)nodes.size(); d.nodes = nodes.data();
    d.n_prims = (uint32_t)prims.size(); d.prims = prims.data();
    d.n_tris = (uint32_t)(triIndices.size() / 3); d.tri_indices = triIndices.data(); d.tri_mesh = triMesh.data();
    d.n_verts = (uint32_t)(P.size() / 3); d.P = P.data(); d.N = N.data(); d.UV = UV.data();
    d.n_meshes = (uint32_t)meshes.size(); d.meshes = meshes.data();
    d.n_spheres = (uint32_t)spheres.size(); d.spheres = spheres.data();
    d.n_disks = (uint32_t)disks.size(); d.disks = disks.data();
    d.n_materials = (uint32_t)materials.size(); d.materials = materials.data();
    d.n_lights = (uint32_t)lights.size(); d.lights = lights.data();
    d.n_instances = (uint32_t)instances.size(); d.instances = instances.empty() ? nullptr : instances.data();
    d.n_motions = (uint32_t)motions.size(); d.motions = motions.empty() ? nullptr : motions.data();
    d.prim_meta = primMeta.size() == prims.size() && !primMeta.empty() ? primMeta.data() : nullptr;
    d.lens = (d.camera_type == MI_CAMERA_REALISTIC && !lensStore.empty()) ? lensStore.data() : nullptr;
    d.light_distrib.func = ldFunc.empty() ? nullptr : ldFunc.data();
    d.light_distrib.cdf = ldCdf.empty() ? nullptr : ldCdf.data();
    d.light_distrib.func_int = ldFuncInt.empty() ? nullptr : ldFuncInt.data();
    d.sampler.primes = primes.data();
    d.sampler.prime_sums = primeSums.data();
    d.sampler.perms = perms.data();
    d.sampler.n_perms = (uint32_t)perms.size();
    d.sampler.sobol_matrices = sobolMatrices.empty() ? nullptr : sobolMatrices.data();
    d.sampler.sobol_vdc = sobolVdc.empty() ? nullptr : sobolVdc.data();
    d.sampler.sobol_vdc_inv = sobolVdcInv.empty() ? nullptr : sobolVdcInv.data();
}

}  // namespace mipt
