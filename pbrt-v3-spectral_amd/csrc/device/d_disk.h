// d_disk.h -- Shape "disk" (ABI v14), the second kind of quadric: plane test, surface interaction and area sampling.
// Restates src/shapes/disk.cpp:48-138 with the base-class Shape::Sample(ref, u) / Shape::Pdf(ref, wi) of
// src/core/shape.cpp:56-87. A quadric index q of the primitive records addresses spheres[q] below DScene::nSpheres and
// disks[q - nSpheres] from there on (QuadricHitT / QuadricInteraction): every place that meets a quadric goes through these.
#pragma once
#include "d_bsdf.h"

namespace dpt {

// The routines marked noinline below are the only out-of-line ones (one body per kernel, reached from the branches a scene without
// disks never takes). They take and return values, never addresses of the caller's variables: such an address would pin the
// caller's interaction records to private memory in every k_shade instance, disks or not.
DEV bool IsDisk(const DScene &s, int q) { return __builtin_expect(q >= s.nSpheres, 0); }

struct DiskHit { float t, px, py, dist2, phi; V3 d; int hit; };        // object space: the hit point is (px, py, height)
struct DiskFrame { V3 p, pError, n, wo, dpdu; };                        // world space
struct DiskTex { V3 dpdv; float u, v; };

// The object-space part Disk::Intersect and IntersectP share (disk.cpp:51-71, 101-121): the ray through
// Transform::operator()(Ray, oErr, dErr) (transform.h:384-396: the origin moves along d by its error bound, tMax stays),
// the plane z = height, the radii and the sweep.
__device__ __attribute__((noinline)) inline DiskHit DiskHitCore(const mi_disk *k, V3 ro, V3 rd, float tMax) {
    DiskHit h;
    h.t = h.px = h.py = h.dist2 = h.phi = 0.f; h.d = V3(0, 0, 0); h.hit = 0;
    V3 oErr;
    V3 o = XfPointErr(k->w2o, ro, &oErr);
    V3 d = XfVector(k->w2o, rd);
    {
        float lengthSquared = d.LengthSquared();
        if (lengthSquared > 0) {
            float dt = Dot(Abs(d), oErr) / lengthSquared;
            o += d * dt;
        }
    }
    if (d.z == 0) return h;
    const float tShapeHit = (k->height - o.z) / d.z;
    if (tShapeHit <= 0 || tShapeHit >= tMax) return h;
    const V3 p = o + d * tShapeHit;
    const float dist2 = p.x * p.x + p.y * p.y;
    if (dist2 > k->radius * k->radius || dist2 < k->inner_radius * k->inner_radius) return h;
    float phi = atan2F(p.y, p.x);
    if (phi < 0) phi += 2 * kPi;
    if (phi > k->phi_max) return h;
    h.t = tShapeHit; h.px = p.x; h.py = p.y; h.dist2 = dist2; h.phi = phi; h.d = d; h.hit = 1;
    return h;
}
// Disk::Intersect's interaction (disk.cpp:73-92) through Transform::operator()(SurfaceInteraction) (transform.cpp:255-288)
__device__ __attribute__((noinline)) inline DiskFrame DiskFrameCore(const mi_disk *k, float px, float py, float dist2, V3 dObj) {
    const float radius = k->radius, innerRadius = k->inner_radius, phiMax = k->phi_max;
    const float rHit = __builtin_sqrtf(dist2);
    const V3 dpdu(-phiMax * py, phiMax * px, 0);
    const float invR = 1.f / rHit;   // Vector3f::operator/ multiplies by the reciprocal (geometry.h:245-249)
    const V3 dpdv((px * (radius - innerRadius)) * invR, (py * (radius - innerRadius)) * invR, (0.f * (radius - innerRadius)) * invR);
    const V3 pHit(px, py, k->height);   // "refine disk intersection point"; pError = 0
    const bool flip = (k->reverse_orientation != 0) ^ (k->swaps_handedness != 0);
    V3 nObj = Normalize(Cross(dpdu, dpdv));
    if (flip) nObj *= -1;
    const float *m = k->o2w, *mi = k->w2o;
    DiskFrame f;
    f.p = XfPointErr2(m, pHit, V3(0, 0, 0), &f.pError);
    f.n = Normalize(XfNormal(mi, nObj));
    f.wo = Normalize(XfVector(m, -dObj));
    f.dpdu = XfVector(m, dpdu);
    return f;
}
// uv and dpdv of the hit (disk.cpp:74-80); dndu = dndv = 0 (disk.cpp:81)
__device__ __attribute__((noinline)) inline DiskTex DiskTexCore(const mi_disk *k, float px, float py, float dist2, float phi) {
    const float radius = k->radius, innerRadius = k->inner_radius;
    const float rHit = __builtin_sqrtf(dist2);
    const float oneMinusV = ((rHit - innerRadius) / (radius - innerRadius));
    const float invR = 1.f / rHit;
    const V3 dpdv((px * (radius - innerRadius)) * invR, (py * (radius - innerRadius)) * invR, (0.f * (radius - innerRadius)) * invR);
    DiskTex t;
    t.u = phi / k->phi_max;
    t.v = 1 - oneMinusV;
    t.dpdv = XfVector(k->o2w, dpdv);
    return t;
}

DEV bool DiskHitT(const mi_disk &k, const V3 &ro, const V3 &rd, float tMax, float *t) {
    const DiskHit h = DiskHitCore(&k, ro, rd, tMax);
    if (!h.hit) return false;
    *t = h.t;
    return true;
}
DEV bool DiskInteraction(const mi_disk &k, const V3 &ro, const V3 &rd, float tMax, SurfaceInteraction *si, float *tHit,
                         float *uvOut = nullptr, V3 *dpdvOut = nullptr) {
    const DiskHit h = DiskHitCore(&k, ro, rd, tMax);
    if (!h.hit) return false;
    const DiskFrame f = DiskFrameCore(&k, h.px, h.py, h.dist2, h.d);
    si->p = f.p; si->pError = f.pError; si->n = f.n; si->wo = f.wo;
    si->dpdu = f.dpdu;
    si->shN = f.n;   // (shading.n = n, then Faceforward(shading.n, n): itself)
    si->shDpdu = f.dpdu;
    if (uvOut || dpdvOut) {
        const DiskTex t = DiskTexCore(&k, h.px, h.py, h.dist2, h.phi);
        if (uvOut) { uvOut[0] = t.u; uvOut[1] = t.v; }
        if (dpdvOut) *dpdvOut = t.dpdv;
    }
    *tHit = h.t;
    return true;
}
DEV float DiskArea(const mi_disk &k) { return k.phi_max * 0.5f * (k.radius * k.radius - k.inner_radius * k.inner_radius); }

// Disk::Sample(u), disk.cpp:129-138 -- the FULL disk of `radius` at `height`, whatever the inner radius and the sweep are --
// inside Shape::Sample(ref, u), shape.cpp:56-70.
struct DiskSampleRec { V3 p, pError, n; float pdf; };
__device__ __attribute__((noinline)) inline DiskSampleRec DiskSampleCore(const mi_disk *k, V3 refP, float u0, float u1) {
    float dx, dy;
    ConcentricSampleDisk(u0, u1, &dx, &dy);
    const V3 pObj(dx * k->radius, dy * k->radius, k->height);
    DiskSampleRec r;
    r.n = Normalize(XfNormal(k->w2o, V3(0, 0, 1)));
    if (k->reverse_orientation) r.n *= -1;
    r.p = XfPointErr2(k->o2w, pObj, V3(0, 0, 0), &r.pError);
    r.pdf = 1 / DiskArea(*k);
    V3 wi = r.p - refP;
    if (wi.LengthSquared() == 0) r.pdf = 0;
    else {
        wi = Normalize(wi);
        r.pdf *= DistanceSquared(refP, r.p) / AbsDot(r.n, -wi);
        if (isinff(r.pdf)) r.pdf = 0.f;
    }
    return r;
}
DEV Interaction DiskSample(const mi_disk &k, const Interaction &ref, float u0, float u1, float *pdf) {
    const DiskSampleRec r = DiskSampleCore(&k, ref.p, u0, u1);
    Interaction it;
    it.p = r.p; it.pError = r.pError; it.n = r.n;
    *pdf = r.pdf;
    return it;
}
// Shape::Pdf(ref, wi), shape.cpp:72-87. *tHit: where the ray meets the disk (a disk light goes the triangle's way in k_shade).
DEV float DiskPdf(const mi_disk &k, float area, const Interaction &ref, const V3 &wi, float *tHit) {
    const Ray ray = SpawnRay(ref, wi);
    const DiskHit h = DiskHitCore(&k, ray.o, ray.d, kInfinity);
    if (!h.hit) return 0;
    const DiskFrame f = DiskFrameCore(&k, h.px, h.py, h.dist2, h.d);
    if (tHit) *tHit = h.t;
    float pdf = DistanceSquared(ref.p, f.p) / (AbsDot(f.n, -wi) * area);
    if (isinff(pdf)) pdf = 0.f;
    return pdf;
}

// ---- the quadric index space (a disk is the rare kind: the compiler keeps its calls, and what they displace, off the spheres' path)
DEV bool QuadricHitT(const DScene &s, int q, const V3 &ro, const V3 &rd, float tMax, float *t) {
    if (IsDisk(s, q)) return DiskHitT(s.disks[q - s.nSpheres], ro, rd, tMax, t);
    return SphereHitT(s.spheres[q], ro, rd, tMax, t);
}
template <bool DISKS = true>
DEV bool QuadricInteraction(const DScene &s, int q, const V3 &ro, const V3 &rd, float tMax, SurfaceInteraction *si, float *t) {
    if (DISKS && IsDisk(s, q)) return DiskInteraction(s.disks[q - s.nSpheres], ro, rd, tMax, si, t);
    return SphereInteraction(s.spheres[q], ro, rd, tMax, si, t);
}

}  // namespace dpt
