// realistic.cpp -- Camera "realistic" at create time (src/cameras/realistic.cpp): the element table, the focused
// lens-to-film distance and the 64 exit-pupil boxes of mi_lens. Float arithmetic in the reference's operation order
// (-ffp-contract=off), so the table and the boxes come out with the reference's bits. Rendering is the device's part;
// the two lens traces here are the host twins of the device's LensTraceFromFilm (d_lens.h).
#include <atomic>
#include <thread>
#include "scene.h"

namespace mipt {
namespace {

struct LRay { Vec3 o, d; };

// Transform::operator()(Ray) with Scale(1, 1, -1) (transform.h:247-266): z mirrored, the origin moved along d by its error bound
LRay FlipZ(const LRay &r) {
    const Vec3 oError = gammaf(3) * Vec3(std::abs(r.o.x), std::abs(r.o.y), std::abs(-1.f * r.o.z));
    Vec3 o(r.o.x, r.o.y, -1.f * r.o.z), d(r.d.x, r.d.y, -1.f * r.d.z);
    const float lengthSquared = d.LengthSquared();
    if (lengthSquared > 0) {
        const float dt = Dot(Vec3(std::abs(d.x), std::abs(d.y), std::abs(d.z)), oError) / lengthSquared;
        o += d * dt;
    }
    return LRay{o, d};
}

bool Quadratic(float a, float b, float c, float *t0, float *t1) {   // pbrt.h:422-438
    const double discrim = (double)b * (double)b - 4 * (double)a * (double)c;
    if (discrim < 0) return false;
    const double rootDiscrim = std::sqrt(discrim);
    double q;
    if (b < 0) q = -.5 * (b - rootDiscrim);
    else q = -.5 * (b + rootDiscrim);
    *t0 = (float)(q / a);
    *t1 = (float)(c / q);
    if (*t0 > *t1) std::swap(*t0, *t1);
    return true;
}

bool Refract(const Vec3 &wi, const Vec3 &n, float eta, Vec3 *wt) {   // reflection.h:92-106
    const float cosThetaI = Dot(n, wi);
    const float sin2ThetaI = std::max(0.f, 1 - cosThetaI * cosThetaI);
    const float sin2ThetaT = eta * eta * sin2ThetaI;
    if (sin2ThetaT >= 1) return false;
    const float cosThetaT = std::sqrt(1 - sin2ThetaT);
    *wt = eta * -wi + (eta * cosThetaI - cosThetaT) * n;
    return true;
}

// realistic.cpp:372-392
bool IntersectSphericalElement(float radius, float zCenter, const LRay &ray, float *t, Vec3 *n) {
    const Vec3 o = ray.o - Vec3(0, 0, zCenter);
    const float A = ray.d.x * ray.d.x + ray.d.y * ray.d.y + ray.d.z * ray.d.z;
    const float B = 2 * (ray.d.x * o.x + ray.d.y * o.y + ray.d.z * o.z);
    const float C = o.x * o.x + o.y * o.y + o.z * o.z - radius * radius;
    float t0, t1;
    if (!Quadratic(A, B, C, &t0, &t1)) return false;
    const bool useCloserT = (ray.d.z > 0) ^ (radius < 0);
    *t = useCloserT ? std::min(t0, t1) : std::max(t0, t1);
    if (*t < 0) return false;
    *n = o + *t * ray.d;
    *n = Normalize(*n);
    if (Dot(*n, -ray.d) < 0.f) *n = -*n;   // Faceforward
    return true;
}

struct Lens {
    int n;
    const float (*e)[4];   // curvature radius, thickness, eta, aperture radius
    float RearZ() const { return e[n - 1][1]; }
    float FrontZ() const { float z = 0; for (int i = 0; i < n; ++i) z += e[i][1]; return z; }
    float RearRadius() const { return e[n - 1][3]; }
};

// TraceLensesFromFilm at 550 nm (realistic.cpp:302-370): what create time traces carries no other wavelength, and at 550 nm
// the chromatic shift is + 0. The reference CHECKs t >= 0 at the stop; here such a ray does not get through.
bool TraceFromFilm(const Lens &L, const LRay &rCamera, LRay *rOut) {
    float elementZ = 0;
    LRay rLens = FlipZ(rCamera);
    for (int i = L.n - 1; i >= 0; --i) {
        const float *el = L.e[i];
        elementZ -= el[1];
        float t;
        Vec3 n;
        const bool isStop = el[0] == 0;
        if (isStop) {
            if (rLens.d.z >= 0.0) return false;
            t = (elementZ - rLens.o.z) / rLens.d.z;
            if (!(t >= 0)) return false;
        } else {
            const float radius = el[0], zCenter = elementZ + el[0];
            if (!IntersectSphericalElement(radius, zCenter, rLens, &t, &n)) return false;
        }
        const Vec3 pHit = rLens.o + rLens.d * t;
        const float r2 = pHit.x * pHit.x + pHit.y * pHit.y;
        if (r2 > el[3] * el[3]) return false;
        rLens.o = pHit;
        if (!isStop) {
            Vec3 w;
            const float etaI = el[2];
            const float etaT = (i > 0 && L.e[i - 1][2] != 0) ? L.e[i - 1][2] : 1;
            if (!Refract(Normalize(-rLens.d), n, etaI / etaT, &w)) return false;
            rLens.d = w;
        }
    }
    if (rOut) *rOut = FlipZ(rLens);
    return true;
}

// TraceLensesFromScene, realistic.cpp:394-442
bool TraceFromScene(const Lens &L, const LRay &rCamera, LRay *rOut) {
    float elementZ = -L.FrontZ();
    LRay rLens = FlipZ(rCamera);
    for (int i = 0; i < L.n; ++i) {
        const float *el = L.e[i];
        float t;
        Vec3 n;
        const bool isStop = el[0] == 0;
        if (isStop) {
            t = (elementZ - rLens.o.z) / rLens.d.z;
            if (!(t >= 0)) return false;
        } else {
            const float radius = el[0], zCenter = elementZ + el[0];
            if (!IntersectSphericalElement(radius, zCenter, rLens, &t, &n)) return false;
        }
        const Vec3 pHit = rLens.o + rLens.d * t;
        const float r2 = pHit.x * pHit.x + pHit.y * pHit.y;
        if (r2 > el[3] * el[3]) return false;
        rLens.o = pHit;
        if (!isStop) {
            Vec3 wt;
            const float etaI = (i == 0 || L.e[i - 1][2] == 0) ? 1 : L.e[i - 1][2];
            const float etaT = (el[2] != 0) ? el[2] : 1;
            if (!Refract(Normalize(-rLens.d), n, etaI / etaT, &wt)) return false;
            rLens.d = wt;
        }
        elementZ += el[1];
    }
    if (rOut) *rOut = FlipZ(rLens);
    return true;
}

void ComputeCardinalPoints(const LRay &rIn, const LRay &rOut, float *pz, float *fz) {   // realistic.cpp:648-654
    const float tf = -rOut.o.x / rOut.d.x;
    *fz = -(rOut.o + rOut.d * tf).z;
    const float tp = (rIn.o.x - rOut.o.x) / rOut.d.x;
    *pz = -(rOut.o + rOut.d * tp).z;
}

float RadicalInverse2(uint64_t a) {   // lowdiscrepancy.h:71-90, lowdiscrepancy.cpp:392
    a = (a << 32) | (a >> 32);
    a = ((a & 0x0000ffff0000ffffull) << 16) | ((a & 0xffff0000ffff0000ull) >> 16);
    a = ((a & 0x00ff00ff00ff00ffull) << 8) | ((a & 0xff00ff00ff00ff00ull) >> 8);
    a = ((a & 0x0f0f0f0f0f0f0f0full) << 4) | ((a & 0xf0f0f0f0f0f0f0f0ull) >> 4);
    a = ((a & 0x3333333333333333ull) << 2) | ((a & 0xccccccccccccccccull) >> 2);
    a = ((a & 0x5555555555555555ull) << 1) | ((a & 0xaaaaaaaaaaaaaaaaull) >> 1);
    return (float)(a * 5.4210108624275222e-20);
}
float RadicalInverse3(uint64_t a) {   // RadicalInverseSpecialized<3>, lowdiscrepancy.cpp:40-58
    const float invBase = (float)1 / (float)3;
    uint64_t reversedDigits = 0;
    float invBaseN = 1;
    while (a) {
        const uint64_t next = a / 3, digit = a - next * 3;
        reversedDigits = reversedDigits * 3 + digit;
        invBaseN *= invBase;
        a = next;
    }
    return std::min(reversedDigits * invBaseN, 0x1.fffffep-1f);
}

// BoundExitPupil, realistic.cpp:753-790 -> {x0, y0, x1, y1}
void BoundExitPupil(const Lens &L, float pFilmX0, float pFilmX1, float *out) {
    float bx0 = std::numeric_limits<float>::max(), by0 = bx0, bx1 = std::numeric_limits<float>::lowest(), by1 = bx1;
    const int nSamples = 1024 * 1024;
    int nExitingRays = 0;
    const float rearRadius = L.RearRadius();
    const float pr0 = -1.5f * rearRadius, pr1 = 1.5f * rearRadius;
    const float rearZ = L.RearZ();
    for (int i = 0; i < nSamples; ++i) {
        const Vec3 pFilm(Lerp((i + 0.5f) / nSamples, pFilmX0, pFilmX1), 0, 0);
        const float u0 = RadicalInverse2((uint64_t)i), u1 = RadicalInverse3((uint64_t)i);
        const Vec3 pRear(Lerp(u0, pr0, pr1), Lerp(u1, pr0, pr1), rearZ);
        // (a point inside the box so far cannot move it: the reference skips its trace too)
        if ((pRear.x >= bx0 && pRear.x <= bx1 && pRear.y >= by0 && pRear.y <= by1) || TraceFromFilm(L, LRay{pFilm, pRear - pFilm}, nullptr)) {
            bx0 = std::min(bx0, pRear.x); by0 = std::min(by0, pRear.y);
            bx1 = std::max(bx1, pRear.x); by1 = std::max(by1, pRear.y);
            ++nExitingRays;
        }
    }
    if (nExitingRays == 0) { out[0] = pr0; out[1] = pr0; out[2] = pr1; out[3] = pr1; return; }
    const float dx = pr1 - pr0;
    const float delta = (float)(2 * std::sqrt(dx * dx + dx * dx) / std::sqrt(nSamples));
    out[0] = bx0 - delta; out[1] = by0 - delta; out[2] = bx1 + delta; out[3] = by1 + delta;
}

}  // namespace

bool BuildRealisticLens(std::vector<float> lensData, float apertureDiameter, float filmDistance, float focusDistance,
                        float diagonal, const int fullRes[2], mi_lens *lens, std::vector<std::string> *warnings, std::string *err) {
    char buf[256];
    if (lensData.empty() || lensData.size() / 4 > MI_MAX_LENS_ELEMENTS) {
        snprintf(buf, sizeof(buf), "Camera \"realistic\": the lens file describes %d element interfaces; 1 to %d are supported.",
                 (int)(lensData.size() / 4), MI_MAX_LENS_ELEMENTS);
        *err = buf;
        return false;
    }
    // RealisticCamera ctor, realistic.cpp:134-148
    lens->n_elements = (int)(lensData.size() / 4);
    for (size_t i = 0; i < lensData.size(); i += 4) {
        if (lensData[i] == 0) {
            if (apertureDiameter > lensData[i + 3]) {
                snprintf(buf, sizeof(buf), "Specified aperture diameter %f is greater than maximum possible %f.  Clamping it.",
                         apertureDiameter, lensData[i + 3]);
                warnings->push_back(buf);
            } else
                lensData[i + 3] = apertureDiameter;
        }
        float *e = lens->elements[i / 4];
        e[0] = lensData[i] * (float).001;
        e[1] = lensData[i + 1] * (float).001;
        e[2] = lensData[i + 2];
        e[3] = lensData[i + 3] * float(.001) / float(2.);
    }
    Lens L{lens->n_elements, lens->elements};
    // Film::diagonal and GetPhysicalExtent, film.cpp:54, 94-99
    lens->film_diagonal = diagonal;
    lens->full_res[0] = fullRes[0]; lens->full_res[1] = fullRes[1];
    {
        const float aspect = (float)fullRes[1] / (float)fullRes[0];
        const float x = std::sqrt(diagonal * diagonal / (1 + aspect * aspect));
        const float y = aspect * x;
        lens->physical_extent[0] = -x / 2; lens->physical_extent[1] = -y / 2;
        lens->physical_extent[2] = x / 2; lens->physical_extent[3] = y / 2;
    }
    {
        // FocusThickLens over ComputeThickLensApproximation, realistic.cpp:656-691. The reference runs it only when no
        // "filmdistance" is given, and then its CHECKs are this scene's errors; with a film distance the cardinal points are
        // recorded where the two rays get through (0 otherwise) and nothing depends on them.
        float pz[2] = {0, 0}, fz[2] = {0, 0};
        const float x = (float)(.001 * diagonal);
        LRay rScene{Vec3(x, 0, L.FrontZ() + 1), Vec3(0, 0, -1)}, rFilm;
        const bool okScene = TraceFromScene(L, rScene, &rFilm);
        if (okScene) ComputeCardinalPoints(rScene, rFilm, &pz[0], &fz[0]);
        else if (filmDistance == 0) {
            *err = "Unable to trace ray from scene to film for thick lens approximation. Is aperture stop extremely small?";
            return false;
        }
        rFilm = LRay{Vec3(x, 0, L.RearZ() - 1), Vec3(0, 0, 1)};
        const bool okFilm = TraceFromFilm(L, rFilm, &rScene);
        if (okFilm) ComputeCardinalPoints(rFilm, rScene, &pz[1], &fz[1]);
        else if (filmDistance == 0) {
            *err = "Unable to trace ray from film to scene for thick lens approximation. Is aperture stop extremely small?";
            return false;
        }
        for (int k = 0; k < 2; ++k) {   // (a system without power has none: 0)
            lens->thick_lens_pz[k] = std::isfinite(pz[k]) ? pz[k] : 0;
            lens->thick_lens_fz[k] = std::isfinite(fz[k]) ? fz[k] : 0;
        }
        if (filmDistance == 0) {
            const float f = fz[0] - pz[0];
            const float z = -focusDistance;
            const float c = (pz[1] - z - pz[0]) * (pz[1] - z - 4 * f - pz[0]);
            if (!(c > 0)) {
                snprintf(buf, sizeof(buf), "Coefficient must be positive. It looks focusDistance: %f is too short for a given lenses configuration", focusDistance);
                *err = buf;
                return false;
            }
            const float delta = 0.5f * (pz[1] - z + pz[0] - std::sqrt(c));
            lens->elements[L.n - 1][1] = lens->elements[L.n - 1][1] + delta;
        } else
            lens->elements[L.n - 1][1] = filmDistance;
    }
    lens->film_distance = lens->elements[L.n - 1][1];
    // exit-pupil boxes (realistic.cpp:171-178): 64 intervals of the film's half diagonal on the build threads
    const int nIntervals = MI_EXIT_PUPIL_BOUNDS;
    unsigned nThreads = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (const char *e = getenv("MIPT_BUILD_THREADS")) nThreads = (unsigned)std::max(1, atoi(e));
    nThreads = std::min(nThreads, (unsigned)nIntervals);
    std::atomic<int> next{0};
    auto work = [&] {
        for (int i = next++; i < nIntervals; i = next++) {
            const float r0 = (float)i / nIntervals * diagonal / 2;
            const float r1 = (float)(i + 1) / nIntervals * diagonal / 2;
            BoundExitPupil(L, r0, r1, lens->exit_pupil_bounds[i]);
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nThreads; ++t) pool.emplace_back(work);
    work();
    for (std::thread &t : pool) t.join();
    return true;
}

}  // namespace mipt
