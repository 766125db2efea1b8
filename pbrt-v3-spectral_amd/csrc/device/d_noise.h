// d_noise.h -- the 3-D noise textures at a path vertex (mi_texture of type MI_TEX_FBM / MI_TEX_WRINKLED / MI_TEX_WINDY).
//   IdentityMapping3D::Map                             src/core/texture.cpp:157-162
//   Noise, Grad, NoiseWeight                           src/core/texture.cpp:164-206
//   SmoothStep, FBm, Turbulence                        src/core/texture.cpp:41-44, 208-251
//   FBmTexture / WrinkledTexture / WindyTexture::Evaluate   src/textures/{fbm,wrinkled,windy}.h
// Float arithmetic in the reference's order (the build contracts nothing). The permutation table is read from global
// memory: 512 bytes, four cache lines that every wave of a noise-textured scene keeps hitting. Noise() and the
// texture's value are calls, like the libm functions (d_math.h): only the general k_shade instances and the probe hold them.
#pragma once
#include "d_scene.h"

namespace dpt {

static __device__ const unsigned char kNoisePerm[512] = {
#include "../host/noise_perm.inc"
};

DEV float NoiseGrad(int x, int y, int z, float dx, float dy, float dz) {
    int h = kNoisePerm[kNoisePerm[kNoisePerm[x] + y] + z];   // x, y, z <= 256 and an entry <= 255: every index <= 511
    h &= 15;
    const float u = h < 8 || h == 12 || h == 13 ? dx : dy;
    const float v = h < 4 || h == 12 || h == 13 ? dy : dz;
    return ((h & 1) ? -u : u) + ((h & 2) ? -v : v);
}
DEV float NoiseWeight(float t) {
    const float t3 = t * t * t;
    const float t4 = t3 * t;
    return 6 * t4 * t - 15 * t4 + 10 * t3;
}
static DEV_CALL float Noise(float x, float y, float z) {
    int ix = (int)floorf(x), iy = (int)floorf(y), iz = (int)floorf(z);
    const float dx = x - ix, dy = y - iy, dz = z - iz;
    ix &= 255; iy &= 255; iz &= 255;
    const float w000 = NoiseGrad(ix, iy, iz, dx, dy, dz);
    const float w100 = NoiseGrad(ix + 1, iy, iz, dx - 1, dy, dz);
    const float w010 = NoiseGrad(ix, iy + 1, iz, dx, dy - 1, dz);
    const float w110 = NoiseGrad(ix + 1, iy + 1, iz, dx - 1, dy - 1, dz);
    const float w001 = NoiseGrad(ix, iy, iz + 1, dx, dy, dz - 1);
    const float w101 = NoiseGrad(ix + 1, iy, iz + 1, dx - 1, dy, dz - 1);
    const float w011 = NoiseGrad(ix, iy + 1, iz + 1, dx, dy - 1, dz - 1);
    const float w111 = NoiseGrad(ix + 1, iy + 1, iz + 1, dx - 1, dy - 1, dz - 1);
    const float wx = NoiseWeight(dx), wy = NoiseWeight(dy), wz = NoiseWeight(dz);
    const float x00 = lerpf(wx, w000, w100);
    const float x10 = lerpf(wx, w010, w110);
    const float x01 = lerpf(wx, w001, w101);
    const float x11 = lerpf(wx, w011, w111);
    const float y0 = lerpf(wy, x00, x10);
    const float y1 = lerpf(wy, x01, x11);
    return lerpf(wz, y0, y1);
}
DEV float SmoothStep(float mn, float mx, float value) {
    const float v = clampf((value - mn) / (mx - mn), 0, 1);
    return v * v * (-2 * v + 3);
}
// the octave count of FBm and Turbulence from the footprint (a zero footprint: Log2 is -inf, every octave)
DEV float NoiseOctaves(const V3 &dpdx, const V3 &dpdy, int maxOctaves) {
    const float len2 = maxf(dpdx.LengthSquared(), dpdy.LengthSquared());
    return clampf(-1 - .5f * Log2F(len2), 0, maxOctaves);
}
DEV float FBm(const V3 &p, const V3 &dpdx, const V3 &dpdy, float omega, int maxOctaves) {
    const float n = NoiseOctaves(dpdx, dpdy, maxOctaves);
    const int nInt = (int)floorf(n);
    float sum = 0, lambda = 1, o = 1;
#pragma unroll 1
    for (int i = 0; i < nInt; ++i) {
        sum += o * Noise(lambda * p.x, lambda * p.y, lambda * p.z);
        lambda *= 1.99f;
        o *= omega;
    }
    const float nPartial = n - nInt;
    sum += o * SmoothStep(.3f, .7f, nPartial) * Noise(lambda * p.x, lambda * p.y, lambda * p.z);
    return sum;
}
DEV float Turbulence(const V3 &p, const V3 &dpdx, const V3 &dpdy, float omega, int maxOctaves) {
    const float n = NoiseOctaves(dpdx, dpdy, maxOctaves);
    const int nInt = (int)floorf(n);
    float sum = 0, lambda = 1, o = 1;
#pragma unroll 1
    for (int i = 0; i < nInt; ++i) {
        sum += o * absf(Noise(lambda * p.x, lambda * p.y, lambda * p.z));
        lambda *= 1.99f;
        o *= omega;
    }
    // the contributions of the clamped octaves
    const float nPartial = n - nInt;
    sum += o * lerpf(SmoothStep(.3f, .7f, nPartial), 0.2f, absf(Noise(lambda * p.x, lambda * p.y, lambda * p.z)));
#pragma unroll 1
    for (int i = nInt; i < maxOctaves; ++i) {
        sum += o * 0.2f;
        o *= omega;
    }
    return sum;
}

// Texture<Float>::Evaluate(si) of noise texture t for an interaction at world p with footprint dpdx / dpdy (without post_scale)
static DEV_CALL float NoiseTextureValue(const mi_texture *t, float px, float py, float pz, float dxx, float dxy, float dxz, float dyx, float dyy,
                                        float dyz) {
    const V3 P = XfPoint(t->w2t, V3(px, py, pz));
    const V3 dpdx = XfVector(t->w2t, V3(dxx, dxy, dxz)), dpdy = XfVector(t->w2t, V3(dyx, dyy, dyz));
    if (t->type == MI_TEX_FBM) return FBm(P, dpdx, dpdy, t->omega, t->octaves);
    if (t->type == MI_TEX_WRINKLED) return Turbulence(P, dpdx, dpdy, t->omega, t->octaves);
    const float windStrength = FBm(.1f * P, .1f * dpdx, .1f * dpdy, .5f, 3);   // MI_TEX_WINDY
    const float waveHeight = FBm(P, dpdx, dpdy, .5f, 6);
    return absf(windStrength) * waveHeight;
}
DEV float NoiseTextureValue(const mi_texture &t, const V3 &p, const V3 &dpdx, const V3 &dpdy) {
    return NoiseTextureValue(&t, p.x, p.y, p.z, dpdx.x, dpdx.y, dpdx.z, dpdy.x, dpdy.y, dpdy.z);
}
}  // namespace dpt
