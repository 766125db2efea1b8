"""The 3-D noise textures "fbm", "wrinkled" and "windy" restated in numpy, in float32 and in float64, for the tests of the
noise-texture path. Each function names the reference lines it follows (src/core/texture.cpp, src/textures/{fbm,wrinkled,
windy}.h, src/core/interaction.cpp, src/core/material.cpp); nothing here calls the product or the oracle. With f = np.float32
every operation rounds to float32 in the reference's order; log is taken in float64 and rounded once, the "correctly rounded"
convention of the device's libm. With f = np.float64 the same formulas give the value the float32 chain approximates; the
literals the reference writes with an `f` suffix stay the float32 numbers in both, they are parameters of the algorithm."""
import os

import numpy as np

import disk_shape as ds

PERM_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "noise_perm.txt")
TEX_FBM, TEX_WRINKLED, TEX_WINDY = 2, 3, 4      # mi_tex_type
_perm = None


def perm():
    """NoisePerm, texture.cpp:50-85: the fixture's 512 integers."""
    global _perm
    if _perm is None:
        with open(PERM_FILE) as fh:
            _perm = np.array(fh.read().split(), np.int64)
        assert _perm.shape == (512,)
    return _perm


def _lit(f, x):
    """A literal with an f suffix: the float32 number, carried in f."""
    return f(np.float32(x))


def lerp(t, a, b):
    """Lerp, pbrt.h:328."""
    f = t.dtype.type
    return (f(1) - t) * a + t * b


def smooth_step(lo, hi, value):
    """SmoothStep, texture.cpp:41-44."""
    f = value.dtype.type
    v = (value - lo) / (hi - lo)
    v = np.where(v < 0, f(0), np.where(v > 1, f(1), v))
    return v * v * (f(-2) * v + f(3))


def grad(x, y, z, dx, dy, dz):
    """Grad, texture.cpp:194-200."""
    p = perm()
    h = p[p[p[x] + y] + z] & 15
    u = np.where((h < 8) | (h == 12) | (h == 13), dx, dy)
    v = np.where((h < 4) | (h == 12) | (h == 13), dy, dz)
    return np.where(h & 1, -u, u) + np.where(h & 2, -v, v)


def noise_weight(t):
    """NoiseWeight, texture.cpp:202-206."""
    f = t.dtype.type
    t3 = t * t * t
    t4 = t3 * t
    return f(6) * t4 * t - f(15) * t4 + f(10) * t3


def noise(x, y, z):
    """Noise(x, y, z), texture.cpp:164-191. floor(x) is a float the int holds exactly (|x| < 2^31), so x - ix is x - floor(x)."""
    f = x.dtype.type
    fx, fy, fz = np.floor(x), np.floor(y), np.floor(z)
    dx, dy, dz = x - fx, y - fy, z - fz
    ix, iy, iz = fx.astype(np.int64) & 255, fy.astype(np.int64) & 255, fz.astype(np.int64) & 255
    one = f(1)
    w000 = grad(ix, iy, iz, dx, dy, dz)
    w100 = grad(ix + 1, iy, iz, dx - one, dy, dz)
    w010 = grad(ix, iy + 1, iz, dx, dy - one, dz)
    w110 = grad(ix + 1, iy + 1, iz, dx - one, dy - one, dz)
    w001 = grad(ix, iy, iz + 1, dx, dy, dz - one)
    w101 = grad(ix + 1, iy, iz + 1, dx - one, dy, dz - one)
    w011 = grad(ix, iy + 1, iz + 1, dx, dy - one, dz - one)
    w111 = grad(ix + 1, iy + 1, iz + 1, dx - one, dy - one, dz - one)
    wx, wy, wz = noise_weight(dx), noise_weight(dy), noise_weight(dz)
    x00, x10 = lerp(wx, w000, w100), lerp(wx, w010, w110)
    x01, x11 = lerp(wx, w001, w101), lerp(wx, w011, w111)
    return lerp(wz, lerp(wy, x00, x10), lerp(wy, x01, x11))


def log2(x):
    """Log2, pbrt.h:338-341: log(x) * invLog2."""
    f = x.dtype.type
    with np.errstate(divide="ignore"):
        lg = np.log(x.astype(np.float64)).astype(f)
    return lg * f(1.442695040888963387004650940071)


def octaves(dpdx, dpdy, max_octaves):
    """`n` of FBm / Turbulence, texture.cpp:211-213, 230-232; a zero footprint takes every octave (Log2(0) = -inf)."""
    f = dpdx.dtype.type
    lx = dpdx[:, 0] * dpdx[:, 0] + dpdx[:, 1] * dpdx[:, 1] + dpdx[:, 2] * dpdx[:, 2]
    ly = dpdy[:, 0] * dpdy[:, 0] + dpdy[:, 1] * dpdy[:, 1] + dpdy[:, 2] * dpdy[:, 2]
    len2 = np.where(lx < ly, ly, lx)
    n = f(-1) - _lit(f, .5) * log2(len2)
    n = np.where(n < 0, f(0), np.where(n > max_octaves, f(max_octaves), n))
    return n, np.floor(n).astype(np.int64)


def _series(f, omega, count):
    """lambda and o before octave i (the same numbers in every lane: lambda *= 1.99f, o *= omega)."""
    lam, o = [f(1)], [f(1)]
    for _ in range(count):
        lam.append(lam[-1] * _lit(f, 1.99))
        o.append(o[-1] * f(omega))
    return np.array(lam, f), np.array(o, f)


def _octave_noise(p, lam):
    return noise(lam * p[:, 0], lam * p[:, 1], lam * p[:, 2])


def fbm(p, dpdx, dpdy, omega, max_octaves):
    """FBm, texture.cpp:208-225."""
    f = p.dtype.type
    n, n_int = octaves(dpdx, dpdy, max_octaves)
    lam, o = _series(f, omega, max_octaves)
    total = np.zeros(len(p), f)
    for i in range(max_octaves):
        a = i < n_int
        if a.any():
            total[a] = total[a] + o[i] * _octave_noise(p[a], lam[i])
    partial = n - n_int.astype(f)
    return total + o[n_int] * smooth_step(_lit(f, .3), _lit(f, .7), partial) * _octave_noise(p, lam[n_int])


def turbulence(p, dpdx, dpdy, omega, max_octaves):
    """Turbulence, texture.cpp:227-251."""
    f = p.dtype.type
    n, n_int = octaves(dpdx, dpdy, max_octaves)
    lam, o = _series(f, omega, max_octaves)
    total = np.zeros(len(p), f)
    for i in range(max_octaves):
        a = i < n_int
        if a.any():
            total[a] = total[a] + o[i] * np.abs(_octave_noise(p[a], lam[i]))
    partial = n - n_int.astype(f)
    total = total + o[n_int] * lerp(smooth_step(_lit(f, .3), _lit(f, .7), partial), np.full(len(p), f(0.2), f), np.abs(_octave_noise(p, lam[n_int])))
    for i in range(max_octaves):
        a = i >= n_int
        total[a] = total[a] + o[i] * _lit(f, .2)
    return total


class Tex:
    """The fields of an mi_texture record (or of a ctypes Texture) that a noise texture reads, in the scalar type f."""

    def __init__(self, rec, f=np.float32):
        self.f = f
        self.type, self.octaves = int(rec.type), int(rec.octaves)
        self.omega, self.post_scale = f(np.float32(rec.omega)), f(np.float32(rec.post_scale))
        self.w2t = np.array(list(rec.w2t), np.float32).reshape(4, 4).astype(f)


def both(rec):
    return Tex(rec, np.float32), Tex(rec, np.float64)


def evaluate(tex, p, dpdx, dpdy):
    """{FBm,Wrinkled,Windy}Texture::Evaluate over IdentityMapping3D::Map (texture.cpp:157-162; fbm.h:55-59, wrinkled.h:56-60,
    windy.h:55-61), times the `scale` constant folded into the record. p, dpdx, dpdy: [n, 3], world space."""
    f = tex.f
    P = ds.xf_point(tex.w2t, np.asarray(p).astype(f))
    dx, dy = ds.xf_vector(tex.w2t, np.asarray(dpdx).astype(f)), ds.xf_vector(tex.w2t, np.asarray(dpdy).astype(f))
    if tex.type == TEX_FBM:
        v = fbm(P, dx, dy, tex.omega, tex.octaves)
    elif tex.type == TEX_WRINKLED:
        v = turbulence(P, dx, dy, tex.omega, tex.octaves)
    else:
        assert tex.type == TEX_WINDY
        t = _lit(f, .1)
        v = np.abs(fbm(t * P, t * dx, t * dy, f(.5), 3)) * fbm(P, dx, dy, f(.5), 6)
    return v * tex.post_scale


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _solve2x2(A, B):
    """SolveLinearSystem2x2, transform.cpp:41-49 -> x0, x1 (0, 0 where it reports failure)."""
    f = B[0].dtype.type
    det = A[0][0] * A[1][1] - A[0][1] * A[1][0]
    with np.errstate(divide="ignore", invalid="ignore"):
        x0 = (A[1][1] * B[0] - A[0][1] * B[1]) / det
        x1 = (A[0][0] * B[1] - A[1][0] * B[0]) / det
    bad = (np.abs(det) < _lit(f, 1e-10)) | np.isnan(x0) | np.isnan(x1)
    return np.where(bad, f(0), x0), np.where(bad, f(0), x1)


def compute_differentials(p, n, rx_o, ry_o, rx_d, ry_d, dpdu=None, dpdv=None):
    """SurfaceInteraction::ComputeDifferentials, interaction.cpp:103-149 -> dpdx, dpdy [n, 3] (zero on the `fail` branch)
    and, with dpdu / dpdv given, (dudx, dvdx, dudy, dvdy) [n, 4] besides."""
    f = p.dtype.type
    d = _dot(n, p)
    with np.errstate(divide="ignore", invalid="ignore"):
        tx = -(_dot(n, rx_o) - d) / _dot(n, rx_d)
        ty = -(_dot(n, ry_o) - d) / _dot(n, ry_d)
        px = rx_o + tx[:, None] * rx_d
        py = ry_o + ty[:, None] * ry_d
    fail = np.isinf(tx) | np.isnan(tx) | np.isinf(ty) | np.isnan(ty)
    zero = np.zeros_like(p)
    dpdx, dpdy = np.where(fail[:, None], zero, px - p), np.where(fail[:, None], zero, py - p)
    if dpdu is None:
        return dpdx, dpdy
    an = np.abs(n)
    first = (an[:, 0] > an[:, 1]) & (an[:, 0] > an[:, 2])
    second = ~first & (an[:, 1] > an[:, 2])
    d0 = np.where(first, 1, 0)
    d1 = np.where(first | second, 2, 1)
    row = np.arange(len(p))
    A = [[dpdu[row, d0], dpdv[row, d0]], [dpdu[row, d1], dpdv[row, d1]]]
    with np.errstate(invalid="ignore"):
        bx = [px[row, d0] - p[row, d0], px[row, d1] - p[row, d1]]
        by = [py[row, d0] - p[row, d0], py[row, d1] - p[row, d1]]
    dudx, dvdx = _solve2x2(A, bx)
    dudy, dvdy = _solve2x2(A, by)
    uv = np.stack([dudx, dvdx, dudy, dvdy], axis=1)
    return dpdx, dpdy, np.where(fail[:, None], f(0), uv)


def bump(tex, p, dpdx, dpdy, duv, sh_dpdu, sh_dpdv, sh_n, ng, flip=False, shift_p=True):
    """Material::Bump (material.cpp:47-84) for a surface with dndu = dndv = 0 under 3-D displacement `tex`, then
    SetShadingGeometry(dpdu, dpdv, ..., false) (interaction.cpp:76-93) -> the new shading normal [n, 3].
    duv: (dudx, dvdx, dudy, dvdy) [n, 4]. shift_p = False leaves p in place in the shifted evaluations (what a uv-only
    Bump would do): the variant the tests tell the right one from."""
    f = tex.f
    p, sh_dpdu, sh_dpdv, sh_n, ng = (np.asarray(a).astype(f) for a in (p, sh_dpdu, sh_dpdv, sh_n, ng))
    duv = np.asarray(duv).astype(f)
    du = _lit(f, .5) * (np.abs(duv[:, 0]) + np.abs(duv[:, 2]))
    du = np.where(du == 0, _lit(f, .0005), du)
    dv = _lit(f, .5) * (np.abs(duv[:, 1]) + np.abs(duv[:, 3]))
    dv = np.where(dv == 0, _lit(f, .0005), dv)
    pu = p + du[:, None] * sh_dpdu if shift_p else p
    pv = p + dv[:, None] * sh_dpdv if shift_p else p
    u_displace = evaluate(tex, pu, dpdx, dpdy)
    v_displace = evaluate(tex, pv, dpdx, dpdy)
    displace = evaluate(tex, p, dpdx, dpdy)
    new_dpdu = sh_dpdu + ((u_displace - displace) / du)[:, None] * sh_n      # (+ displace * dndu, zero here)
    new_dpdv = sh_dpdv + ((v_displace - displace) / dv)[:, None] * sh_n
    ns = ds.normalize(ds.cross(new_dpdu, new_dpdv))
    if flip:
        ns = -ns
    back = _dot(ns, ng) < 0           # Faceforward(shading.n, n)
    return np.where(back[:, None], -ns, ns)
