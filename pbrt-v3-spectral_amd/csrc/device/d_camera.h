// d_camera.h -- Camera "orthographic" and Camera "environment" on the device (MIPT_CAMERAS=all: mi_camera_type 2 and 3).
//   OrthographicCamera::GenerateRay, GenerateRayDifferential          src/cameras/orthographic.cpp:44-121
//   EnvironmentCamera::GenerateRay (the fork's omnistereo camera)     src/cameras/environment.cpp:43-105
//   Camera::GenerateRayDifferential (the base class's offset rays)    src/core/camera.cpp:60-99
// Restated as the reference has them, with what a scene author would call surprising (README, "Opt-in cameras"): a lens
// moves every orthographic ray's origin to the lens point alone; the second focal distance of the orthographic offset rays
// comes from the direction the lens has already changed; the pole-merge angles are compared as given against an altitude in
// radians, which is taken from the z of the direction after the axis swap.
// Both cameras have ray weight 1. The routines return the world-space ray and, through `diff`, the offset rays after
// ScaleDifferentials(scale): rxOrigin, ryOrigin, rxDirection, ryDirection -- the layout of LensCameraRay (d_lens.h), so
// k_generate stores them in the same pool planes and the camera probe reports them in the same columns.
#pragma once
#include "d_sampling.h"
#include "d_bsdf.h"

namespace dpt {

static DEV_CALL float asinF(float x) { return (float)asin((double)x); }

// CameraToWorld at the ray's time: the camera's one matrix, or the AnimatedTransform's (MovingCameraToWorld).
template <bool MOVING>
DEV void CameraToWorldAt(const DScene &s, float time, float *m) {
    if constexpr (MOVING) MovingCameraToWorld(s.cameraMotion, time, m);
    else {
#pragma unroll
        for (int k = 0; k < 16; ++k) m[k] = s.cameraMotion->camera_to_world[k];
    }
}

// RayDifferential::ScaleDifferentials, geometry.h:917-922
DEV void ScaleCameraDifferentials(const Ray &ray, const V3 &rxO, const V3 &ryO, const V3 &rxD, const V3 &ryD, float scale, V3 *diff) {
    diff[0] = ray.o + (rxO - ray.o) * scale;
    diff[1] = ray.o + (ryO - ray.o) * scale;
    diff[2] = ray.d + (rxD - ray.d) * scale;
    diff[3] = ray.d + (ryD - ray.d) * scale;
}

// OrthographicCamera::GenerateRayDifferential, then Transform::operator()(RayDifferential) (transform.h:268-281: the main ray
// as a Ray, the offset origins as points, the offset directions as vectors) and ScaleDifferentials.
template <bool MOVING>
DEV void OrthographicCameraRay(const DScene &s, float pFilmX, float pFilmY, float lu, float lv, float timeU, Ray *out, float *timeOut, V3 *diff, float scale) {
    const mi_camera &cam = s.camera;
    const float time = lerpf(timeU, cam.shutter_open, cam.shutter_close);
    if (timeOut) *timeOut = time;
    float m[16];
    CameraToWorldAt<MOVING>(s, time, m);
    const V3 pCamera = XfPoint(cam.raster_to_camera, V3(pFilmX, pFilmY, 0));
    // dxCamera = RasterToCamera(Vector3f(1, 0, 0)), dyCamera = RasterToCamera(Vector3f(0, 1, 0)) (orthographic.h:61-62)
    const V3 dxCamera = XfVector(cam.raster_to_camera, V3(1, 0, 0)), dyCamera = XfVector(cam.raster_to_camera, V3(0, 1, 0));
    Ray ray(pCamera, V3(0, 0, 1));
    V3 rxO, ryO, rxD, ryD;
    if (cam.lens_radius > 0) {
        float dx, dy;
        ConcentricSampleDisk(lu, lv, &dx, &dy);
        const V3 pLens(cam.lens_radius * dx, cam.lens_radius * dy, 0);
        float ft = cam.focal_distance / ray.d.z;
        const V3 pFocus = ray.at(ft);
        ray.o = pLens;   // (the film point's offset is dropped: every ray leaves the lens disk at the origin)
        ray.d = Normalize(pFocus - ray.o);
        ft = cam.focal_distance / ray.d.z;   // (a second time, from the direction the lens changed: orthographic.cpp:102)
        rxO = ryO = pLens;
        rxD = Normalize(((pCamera + dxCamera) + (ft * V3(0, 0, 1))) - rxO);
        ryD = Normalize(((pCamera + dyCamera) + (ft * V3(0, 0, 1))) - ryO);
    } else {
        rxO = ray.o + dxCamera;
        ryO = ray.o + dyCamera;
        rxD = ryD = ray.d;
    }
    *out = XfRay(m, ray);
    if (diff) ScaleCameraDifferentials(*out, XfPoint(m, rxO), XfPoint(m, ryO), XfVector(m, rxD), XfVector(m, ryD), scale, diff);
}

// EnvironmentCamera::GenerateRay up to its CameraToWorld: the ray in camera space.
DEV Ray EnvironmentGenerateRay(const DScene &s, float pFilmX, float pFilmY) {
    const float theta = kPi * pFilmY / (float)s.fullRes[1];
    const float phi = 2 * kPi * pFilmX / (float)s.fullRes[0];
    const float sinTheta = sinF(theta), cosTheta = cosF(theta);
    // (x, y, z) of the spherical direction with y and z swapped: y is up
    Ray ray(V3(0, 0, 0), V3(sinTheta * cosF(phi), cosTheta, sinTheta * sinF(phi)));
    float offset = s.envIpd;
    if (offset != 0.0f) {   // omnistereo
        if (s.envPoleMergeTo > 0.0f) {
            const float altitude = absf(asinF(ray.d.z));
            if (altitude > s.envPoleMergeTo) offset = 0.0f;
            else if (altitude > s.envPoleMergeFrom) {
                const float fac = (altitude - s.envPoleMergeFrom) / (s.envPoleMergeTo - s.envPoleMergeFrom);
                offset *= cosF(fac * kPiOver2);
            }
        }
        const V3 up(0.0f, 1.0f, 0.0f);
        V3 side(0.f, 0.f, 0.f);
        if (!(ray.d.x == up.x && ray.d.y == up.y && ray.d.z == up.z)) side = Normalize(Cross(ray.d, up));
        const V3 stereoOffset = side * offset;
        ray.o += stereoOffset;
        if (s.envConvergenceDistance != kInfinity) ray.d = Normalize((s.envConvergenceDistance * ray.d) - stereoOffset);
    }
    return ray;
}

// Camera::GenerateRayDifferential over EnvironmentCamera::GenerateRay: the ray again at pFilm.x + .05 and at pFilm.y + .05,
// each carried to world space like the main ray (the weight is always 1: the - .05 retry never runs), then ScaleDifferentials.
template <bool MOVING>
DEV void EnvironmentCameraRay(const DScene &s, float pFilmX, float pFilmY, float timeU, Ray *out, float *timeOut, V3 *diff, float scale) {
    const mi_camera &cam = s.camera;
    const float time = lerpf(timeU, cam.shutter_open, cam.shutter_close);
    if (timeOut) *timeOut = time;
    float m[16];
    CameraToWorldAt<MOVING>(s, time, m);
    const Ray ray = XfRay(m, EnvironmentGenerateRay(s, pFilmX, pFilmY));
    *out = ray;
    if (!diff) return;
    const float eps = .05f;
    const Ray rx = XfRay(m, EnvironmentGenerateRay(s, pFilmX + eps, pFilmY));
    const Ray ry = XfRay(m, EnvironmentGenerateRay(s, pFilmX, pFilmY + eps));
    ScaleCameraDifferentials(ray, ray.o + (rx.o - ray.o) / eps, ray.o + (ry.o - ray.o) / eps, ray.d + (rx.d - ray.d) / eps, ray.d + (ry.d - ray.d) / eps, scale, diff);
}

// The camera ray of one of the two kinds (KIND: MI_CAMERA_ORTHOGRAPHIC or MI_CAMERA_ENVIRONMENT), as k_generate and the
// camera probe ask for it.
template <int KIND, bool MOVING>
DEV void OptInCameraRay(const DScene &s, float pFilmX, float pFilmY, float lu, float lv, float timeU, Ray *out, float *timeOut, V3 *diff, float scale) {
    static_assert(KIND == MI_CAMERA_ORTHOGRAPHIC || KIND == MI_CAMERA_ENVIRONMENT, "the cameras of d_camera.h");
    if constexpr (KIND == MI_CAMERA_ORTHOGRAPHIC) OrthographicCameraRay<MOVING>(s, pFilmX, pFilmY, lu, lv, timeU, out, timeOut, diff, scale);
    else EnvironmentCameraRay<MOVING>(s, pFilmX, pFilmY, timeU, out, timeOut, diff, scale);
}

}  // namespace dpt
