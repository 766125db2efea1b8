// d_lens.h -- Camera "realistic" on the device (ABI v13: mi_lens): the camera ray of a sample through the lens system.
//   RealisticCamera::TraceLensesFromFilm, IntersectSphericalElement   src/cameras/realistic.cpp:302-392
//   RealisticCamera::SampleExitPupil, GenerateRay                     src/cameras/realistic.cpp:832-851, 899-932
//   Camera::GenerateRayDifferential (the base class's offset rays)    src/core/camera.cpp:60-99
// The element table and the exit-pupil boxes are read from the device copy of mi_lens (DScene::lens), never from
// the by-value DScene: the element loop indexes the table, and an indexed read of a kernel argument moves the whole
// argument block into private memory (compiler notes). The table's addresses are uniform over a
// wave (scalar loads); only the exit-pupil box is picked per lane.
#pragma once
#include "d_sampling.h"
#include "d_bsdf.h"

namespace dpt {

// Transform::operator()(Ray) with Scale(1, 1, -1) (transform.h:247-266): z mirrored and the origin moved along the
// direction by its error bound, as XfRay does it for a general matrix.
DEV Ray LensFlipZ(const Ray &r) {
    const V3 oError = gammaf(3) * V3(absf(r.o.x), absf(r.o.y), absf(-1.f * r.o.z));
    V3 o(r.o.x, r.o.y, -1.f * r.o.z);
    const V3 d(r.d.x, r.d.y, -1.f * r.d.z);
    const float lengthSquared = d.LengthSquared();
    float tMax = r.tMax;
    if (lengthSquared > 0) {
        const float dt = Dot(Abs(d), oError) / lengthSquared;
        o += d * dt;
        tMax -= dt;
    }
    return Ray(o, d, tMax);
}

// Quadratic(Float, ...), pbrt.h:422-438: the roots in double
DEV bool LensQuadratic(float a, float b, float c, float *t0, float *t1) {
    const double discrim = (double)b * (double)b - 4. * (double)a * (double)c;
    if (discrim < 0.) return false;
    const double rootDiscrim = __builtin_sqrt(discrim);
    double q;
    if (b < 0) q = -.5 * ((double)b - rootDiscrim);
    else q = -.5 * ((double)b + rootDiscrim);
    *t0 = (float)(q / (double)a);
    *t1 = (float)((double)c / q);
    if (*t0 > *t1) { const float t = *t0; *t0 = *t1; *t1 = t; }
    return true;
}

DEV bool IntersectSphericalElement(float radius, float zCenter, const Ray &ray, float *t, V3 *n) {
    const V3 o = ray.o - V3(0, 0, zCenter);
    const float A = ray.d.x * ray.d.x + ray.d.y * ray.d.y + ray.d.z * ray.d.z;
    const float B = 2 * (ray.d.x * o.x + ray.d.y * o.y + ray.d.z * o.z);
    const float C = o.x * o.x + o.y * o.y + o.z * o.z - radius * radius;
    float t0, t1;
    if (!LensQuadratic(A, B, C, &t0, &t1)) return false;
    const bool useCloserT = (ray.d.z > 0) ^ (radius < 0);
    *t = useCloserT ? minf(t0, t1) : maxf(t0, t1);
    if (*t < 0) return false;
    *n = o + *t * ray.d;
    *n = Faceforward(Normalize(*n), -ray.d);
    return true;
}

// wavelength in nm: with "chromaticAberrationEnabled" and 400 <= wavelength <= 700 every eta other than 1 is shifted by
// (wavelength - 550) * -.04 / 300, in double as the reference's mixed expression evaluates it (realistic.cpp:352-358).
// (The reference CHECKs t >= 0 at the stop; here such a ray does not get through.)
DEV bool LensTraceFromFilm(const mi_lens *__restrict__ L, const Ray &rCamera, float wavelength, Ray *rOut) {
    float elementZ = 0;
    Ray rLens = LensFlipZ(rCamera);
    const int n = L->n_elements;
    const bool ca = L->chromatic_aberration && wavelength >= 400 && wavelength <= 700;
    for (int i = n - 1; i >= 0; --i) {
        const float curvatureRadius = L->elements[i][0], thickness = L->elements[i][1], eta = L->elements[i][2], apertureRadius = L->elements[i][3];
        elementZ -= thickness;
        float t;
        V3 nrm;
        const bool isStop = curvatureRadius == 0;
        if (isStop) {
            if (rLens.d.z >= 0.f) return false;
            t = (elementZ - rLens.o.z) / rLens.d.z;
            if (!(t >= 0)) return false;
        } else {
            const float zCenter = elementZ + curvatureRadius;
            if (!IntersectSphericalElement(curvatureRadius, zCenter, rLens, &t, &nrm)) return false;
        }
        const V3 pHit = rLens.at(t);
        const float r2 = pHit.x * pHit.x + pHit.y * pHit.y;
        if (r2 > apertureRadius * apertureRadius) return false;
        rLens.o = pHit;
        if (!isStop) {
            V3 w;
            float etaI = eta;
            const float etaPrev = i > 0 ? L->elements[i > 0 ? i - 1 : 0][2] : 0.f;
            float etaT = (i > 0 && etaPrev != 0) ? etaPrev : 1;
            if (ca) {
                if (etaI != 1) etaI = (float)((double)(wavelength - 550) * -.04 / 300. + (double)etaI);
                if (etaT != 1) etaT = (float)((double)(wavelength - 550) * -.04 / 300. + (double)etaT);
            }
            if (!Refract(Normalize(-rLens.d), nrm, etaI / etaT, &w)) return false;
            rLens.d = w;
        }
    }
    *rOut = LensFlipZ(rLens);
    return true;
}

// RealisticCamera::GenerateRay for the film position (pFilmX, pFilmY) in raster space and the lens sample (lu, lv): the ray
// in world space through c2w (CameraToWorld at the ray's time) and the ray's weight, 0 when it does not get through.
DEV float LensGenerateRay(const mi_camera &cam, const mi_lens *__restrict__ L, const float *c2w, float pFilmX, float pFilmY, float lu, float lv,
                          float wavelength, Ray *ray) {
    const float sx = pFilmX / L->full_res[0], sy = pFilmY / L->full_res[1];
    const float fx = lerpf(sx, L->physical_extent[0], L->physical_extent[2]), fy = lerpf(sy, L->physical_extent[1], L->physical_extent[3]);
    const V3 pFilm(-fx, fy, 0);
    // SampleExitPupil
    const float rFilm = __builtin_sqrtf(pFilm.x * pFilm.x + pFilm.y * pFilm.y);
    int rIndex = (int)(rFilm / (L->film_diagonal / 2) * (float)MI_EXIT_PUPIL_BOUNDS);
    rIndex = max(0, min(MI_EXIT_PUPIL_BOUNDS - 1, rIndex));   // (max: the table is indexed with it, whatever the sample was)
    const float bx0 = L->exit_pupil_bounds[rIndex][0], by0 = L->exit_pupil_bounds[rIndex][1], bx1 = L->exit_pupil_bounds[rIndex][2], by1 = L->exit_pupil_bounds[rIndex][3];
    const float exitPupilBoundsArea = (bx1 - bx0) * (by1 - by0);
    const float plx = lerpf(lu, bx0, bx1), ply = lerpf(lv, by0, by1);
    const float sinTheta = (rFilm != 0) ? pFilm.y / rFilm : 0;
    const float cosTheta = (rFilm != 0) ? pFilm.x / rFilm : 1;
    const float rearZ = L->elements[L->n_elements - 1][1];
    const V3 pRear(cosTheta * plx - sinTheta * ply, sinTheta * plx + cosTheta * ply, rearZ);
    const Ray rFilmRay(pFilm, pRear - pFilm);
    Ray r;
    if (!LensTraceFromFilm(L, rFilmRay, wavelength, &r)) return 0.f;
    *ray = XfRay(c2w, r);
    ray->d = Normalize(ray->d);
    const float cosT = Normalize(rFilmRay.d).z;
    const float cos4Theta = (cosT * cosT) * (cosT * cosT);
    if (L->simple_weighting) {
        const float a0 = (L->exit_pupil_bounds[0][2] - L->exit_pupil_bounds[0][0]) * (L->exit_pupil_bounds[0][3] - L->exit_pupil_bounds[0][1]);
        return cos4Theta * exitPupilBoundsArea / a0;
    }
    return (cam.shutter_close - cam.shutter_open) * (cos4Theta * exitPupilBoundsArea) / (rearZ * rearZ);
}

// Camera::GenerateRayDifferential for a realistic camera: the main ray, then the offset rays at pFilm.x + .05 and
// pFilm.y + .05, each once more at - .05 when it does not get through; the sample's weight is 0 when the main ray or both
// signs of an axis are vignetted, so the offset rays are traced whether or not anything reads the differentials.
// diff (may be null): rxOrigin, ryOrigin, rxDirection, ryDirection after ScaleDifferentials(scale).
// MOVING: CameraToWorld is the AnimatedTransform at the ray's time (MovingCameraToWorld), the last step of every ray.
template <bool MOVING>
DEV float LensCameraRay(const DScene &s, float pFilmX, float pFilmY, float lu, float lv, float timeU, float wavelength, Ray *out,
                        float *timeOut, V3 *diff, float scale) {
    const mi_camera &cam = s.camera;
    const mi_lens *__restrict__ L = s.lens;
    const float time = lerpf(timeU, cam.shutter_open, cam.shutter_close);
    if (timeOut) *timeOut = time;
    float m[16];
    if constexpr (MOVING) MovingCameraToWorld(s.cameraMotion, time, m);
    else {
#pragma unroll
        for (int k = 0; k < 16; ++k) m[k] = s.cameraMotion->camera_to_world[k];
    }
    Ray ray;
    const float wt = LensGenerateRay(cam, L, m, pFilmX, pFilmY, lu, lv, wavelength, &ray);
    if (wt == 0) return 0.f;
    *out = ray;
    V3 rxO, rxD, ryO, ryD;
    float wtx = 0.f, wty = 0.f;
#pragma unroll 1
    for (int k = 0; k < 2 && wtx == 0; ++k) {
        const float eps = k ? -.05f : .05f;
        Ray rx;
        wtx = LensGenerateRay(cam, L, m, pFilmX + eps, pFilmY, lu, lv, wavelength, &rx);
        rxO = ray.o + (rx.o - ray.o) / eps;
        rxD = ray.d + (rx.d - ray.d) / eps;
    }
    if (wtx == 0) return 0.f;
#pragma unroll 1
    for (int k = 0; k < 2 && wty == 0; ++k) {
        const float eps = k ? -.05f : .05f;
        Ray ry;
        wty = LensGenerateRay(cam, L, m, pFilmX, pFilmY + eps, lu, lv, wavelength, &ry);
        ryO = ray.o + (ry.o - ray.o) / eps;
        ryD = ray.d + (ry.d - ray.d) / eps;
    }
    if (wty == 0) return 0.f;
    if (diff) {   // RayDifferential::ScaleDifferentials, geometry.h:917-922
        diff[0] = ray.o + (rxO - ray.o) * scale;
        diff[1] = ray.o + (ryO - ray.o) * scale;
        diff[2] = ray.d + (rxD - ray.d) * scale;
        diff[3] = ray.d + (ryD - ray.d) * scale;
    }
    return wt;
}

// The wavelength band s of Integrator "spectralpath" generates its camera ray at (spectralpath.cpp:234-267): the middle of
// the band's bins, with sampledLambdaStart = 395 and (705 - 395) / 31 = 10 nm per bin (spectrum.h:48-50).
DEV float BandWavelength(int bandDelta, int band) {
    const float deltaWaveCA = 10.f * bandDelta;
    return 395 + deltaWaveCA * band + (deltaWaveCA / 2);
}

}  // namespace dpt
