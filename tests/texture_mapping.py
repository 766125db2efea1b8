"""The 2-D texture mappings and the texture classes "dots", "uv", "bilerp" and "checkerboard" restated in numpy, in float32 and
in float64, for the tests of the opt-in texture path (MIPT_TEXTURES=all). Each function names the reference lines it follows
(src/core/texture.{h,cpp}, src/core/geometry.h, src/textures/{dots,uv,bilerp,checkerboard}.h, src/core/spectrum.cpp); nothing
here calls the product or the oracle. The conventions are noise_texture.py's: with f = np.float32 every operation rounds to
float32 in the reference's order, acos and atan2 are taken in float64 and rounded once (the device's libm convention); with
f = np.float64 the same formulas give the value the float32 chain approximates; literals the reference writes as Float
(Pi, InvPi, .1f, .35f ...) stay the float32 numbers in both. Besides its value every function returns the discrete decisions
it took, so that a test can leave out the queries on which the two precisions decide differently."""
import numpy as np

import disk_shape as ds
import noise_texture as nt

TEX_IMAGEMAP, TEX_CHECKERBOARD, TEX_DOTS, TEX_UV, TEX_BILERP, TEX_CHECKERBOARD3D = 0, 1, 5, 6, 7, 8     # mi_tex_type
MAP_UV, MAP_SPHERICAL, MAP_CYLINDRICAL, MAP_PLANAR = 0, 1, 2, 3                                       # mi_tex_mapping
NSPEC = 31
_lit = nt._lit


class Tex:
    """The fields of an mi_texture record that the mappings and classes read, in the scalar type f."""

    def __init__(self, rec, f=np.float32):
        self.f = f
        self.type, self.mapping, self.aa_none, self.is_float = int(rec.type), int(rec.mapping), int(rec.aa_none), int(rec.is_float)
        c = lambda x: f(np.float32(x))
        self.su, self.sv, self.du, self.dv, self.post_scale = c(rec.su), c(rec.sv), c(rec.du), c(rec.dv), c(rec.post_scale)
        arr = lambda a: np.array(list(a), np.float32).astype(f)
        self.vs, self.vt, self.bilerp = arr(rec.vs), arr(rec.vt), arr(rec.bilerp)
        self.spec1, self.spec2 = arr(rec.spec1), arr(rec.spec2)
        self.w2t = arr(rec.w2t).reshape(4, 4)


def both(rec):
    return Tex(rec, np.float32), Tex(rec, np.float64)


def _libm(fn, f, *a):
    """A libm call: in float64, rounded once to f."""
    with np.errstate(invalid="ignore"):
        return fn(*[x.astype(np.float64) for x in a]).astype(f)


def _dot(a, b):
    return a[:, 0] * b[0] + a[:, 1] * b[1] + a[:, 2] * b[2]


def sphere(tex, p):
    """SphericalMapping2D::sphere, texture.cpp:123-127; SphericalTheta / SphericalPhi, geometry.h:1483-1490.
    -> st [n, 2] and the side of the phi seam (atan2 < 0: phi came from the far side)."""
    f = tex.f
    vec = ds.normalize(ds.xf_point(tex.w2t, p))
    z = vec[:, 2]
    z = np.where(z < -1, f(-1), np.where(z > 1, f(1), z))           # Clamp(v.z, -1, 1)
    theta = _libm(np.arccos, f, z)
    ph = _libm(np.arctan2, f, vec[:, 1], vec[:, 0])
    phi = np.where(ph < 0, ph + f(2) * _lit(f, np.pi), ph)
    return np.stack([theta * _lit(f, 1 / np.pi), phi * _lit(f, .5 / np.pi)], axis=1), ph < 0


def cylinder(tex, p):
    """CylindricalMapping2D::cylinder, texture.h:93-96. The seam lies at atan2 = +-pi."""
    f = tex.f
    vec = ds.normalize(ds.xf_point(tex.w2t, p))
    at = _libm(np.arctan2, f, vec[:, 1], vec[:, 0])
    return np.stack([(_lit(f, np.pi) + at) * _lit(f, .5 / np.pi), vec[:, 2]], axis=1), at < 0


def _wrap(d):
    """texture.cpp:111-119 / 136-145 for one differential's component [1] -> the value and the branch taken."""
    f = d.dtype.type
    with np.errstate(invalid="ignore"):
        hi, lo = d > f(.5), d < _lit(f, -.5)
    return np.where(hi, f(1) - d, np.where(lo, -(d + f(1)), d)), np.where(hi, 1, np.where(lo, -1, 0))


def map2d(tex, p, dpdx, dpdy, uv, duv):
    """TextureMapping2D::Map (texture.cpp:93-155) of the record's mapping. p, dpdx, dpdy [n, 3]; uv [n, 2]; duv [n, 4] =
    (dudx, dvdx, dudy, dvdy). -> [n, 6] (s, t, dsdx, dtdx, dsdy, dtdy) and the decisions [n, k] (seam side, wrap branches)."""
    f = tex.f
    p, dpdx, dpdy, uv, duv = (np.asarray(a).astype(f) for a in (p, dpdx, dpdy, uv, duv))
    n = len(p)
    if tex.mapping == MAP_UV:        # UVMapping2D::Map, texture.cpp:93-99
        out = np.stack([tex.su * uv[:, 0] + tex.du, tex.sv * uv[:, 1] + tex.dv, tex.su * duv[:, 0], tex.sv * duv[:, 1], tex.su * duv[:, 2], tex.sv * duv[:, 3]], axis=1)
        return out, np.zeros((n, 1), np.int64)
    if tex.mapping == MAP_PLANAR:    # PlanarMapping2D::Map, texture.cpp:149-155 (ds, dt ride in du, dv)
        out = np.stack([tex.du + _dot(p, tex.vs), tex.dv + _dot(p, tex.vt), _dot(dpdx, tex.vs), _dot(dpdx, tex.vt), _dot(dpdy, tex.vs), _dot(dpdy, tex.vt)], axis=1)
        return out, np.zeros((n, 1), np.int64)
    fn, delta = (sphere, _lit(f, .1)) if tex.mapping == MAP_SPHERICAL else (cylinder, _lit(f, .01))   # texture.cpp:101-147
    st, side = fn(tex, p)
    stx, sidex = fn(tex, p + delta * dpdx)
    sty, sidey = fn(tex, p + delta * dpdy)
    inv = f(1) / delta                          # Vector2f / Float, geometry.h:121-125
    dx, dy = (stx - st) * inv, (sty - st) * inv
    dtdx, bx = _wrap(dx[:, 1])
    dtdy, by = _wrap(dy[:, 1])
    out = np.stack([st[:, 0], st[:, 1], dx[:, 0], dtdx, dy[:, 0], dtdy], axis=1)
    return out, np.stack([side, sidex, sidey, bx, by], axis=1).astype(np.int64)


def dots(st):
    """DotsTexture::Evaluate, dots.h:59-78 -> inside the dot [n] (bool), the dot's centre [n, 2] and the decisions
    [n, 4]: the cell (two numbers), Noise > 0, inside the radius. Noise(x, y) is Noise(x, y, .5f), texture.h:143."""
    f = st.dtype.type
    half = f(.5)
    s_cell, t_cell = np.floor(st[:, 0] + half), np.floor(st[:, 1] + half)
    n2 = lambda x, y: nt.noise(x, y, np.full_like(x, half))
    present = n2(s_cell + half, t_cell + half) > 0
    radius = _lit(f, .35)
    max_shift = half - radius
    s_center = s_cell + max_shift * n2(s_cell + _lit(f, 1.5), t_cell + _lit(f, 2.8))
    t_center = t_cell + max_shift * n2(s_cell + _lit(f, 4.5), t_cell + _lit(f, 9.8))
    d0, d1 = st[:, 0] - s_center, st[:, 1] - t_center
    within = d0 * d0 + d1 * d1 < radius * radius
    dec = np.stack([s_cell.astype(np.int64), t_cell.astype(np.int64), present.astype(np.int64), (present & within).astype(np.int64)], axis=1)
    return present & within, np.stack([s_center, t_center], axis=1), dec


def checkerboard2d(c, aa_none):
    """Checkerboard2DTexture::Evaluate, checkerboard.h:64-101, for st and differentials c [n, 6] -> the weight of tex2 [n]
    and the decisions [n, 3]: the parity, "the filter lies inside one check", "ds > 1 || dt > 1"."""
    f = c.dtype.type
    s, t = c[:, 0], c[:, 1]
    with np.errstate(invalid="ignore"):
        odd = (np.floor(s).astype(np.int64) + np.floor(t).astype(np.int64)) % 2 != 0
    point = np.where(odd, f(1), f(0))
    if aa_none:
        return point, np.stack([odd, odd, odd], axis=1).astype(np.int64)
    dS = np.maximum(np.abs(c[:, 2]), np.abs(c[:, 4]))
    dT = np.maximum(np.abs(c[:, 3]), np.abs(c[:, 5]))
    s0, s1, t0, t1 = s - dS, s + dS, t - dT, t + dT
    single = (np.floor(s0) == np.floor(s1)) & (np.floor(t0) == np.floor(t1))

    def bump_int(x):
        h = x / f(2)
        fl = np.floor(h)
        return fl + f(2) * np.maximum(h - fl - f(.5), f(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        sint = (bump_int(s1) - bump_int(s0)) / (f(2) * dS)
        tint = (bump_int(t1) - bump_int(t0)) / (f(2) * dT)
    area2 = sint + tint - f(2) * sint * tint
    wide = (dS > 1) | (dT > 1)
    area2 = np.where(wide, f(.5), area2)
    return np.where(single, point, area2), np.stack([odd & single, single, wide & ~single], axis=1).astype(np.int64)


def checkerboard3d(tex, p):
    """Checkerboard3DTexture::Evaluate over IdentityMapping3D, checkerboard.h:118-128, texture.cpp:157-162 -> tex2 is chosen [n]."""
    P = ds.xf_point(tex.w2t, np.asarray(p).astype(tex.f))
    return (np.floor(P[:, 0]).astype(np.int64) + np.floor(P[:, 1]).astype(np.int64) + np.floor(P[:, 2]).astype(np.int64)) % 2 != 0


def from_rgb(rgb, basis):
    """SampledSpectrum::FromRGB(rgb, SpectrumType::Illuminant), spectrum.cpp:140-177, then Clamp(): rgb [n, 3], basis [7, 31] =
    rgbIllum2Spect{White, Cyan, Magenta, Yellow, Red, Green, Blue} -> [n, 31]."""
    f = rgb.dtype.type
    B = np.asarray(basis, np.float32).astype(f)
    r, g, b = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    out = np.zeros((len(rgb), NSPEC), f)
    case_r = (r <= g) & (r <= b)
    case_g = ~case_r & (g <= r) & (g <= b)
    case_b = ~case_r & ~case_g
    # (the white weight, then the secondary's index and weight, then the primary's)
    plans = [(case_r & (g <= b), r, 1, g - r, 6, b - g), (case_r & ~(g <= b), r, 1, b - r, 5, g - b),
             (case_g & (r <= b), g, 2, r - g, 6, b - r), (case_g & ~(r <= b), g, 2, b - g, 4, r - b),
             (case_b & (r <= g), b, 3, r - b, 5, g - r), (case_b & ~(r <= g), b, 3, g - b, 4, r - g)]
    for sel, w0, i1, w1, i2, w2 in plans:
        if sel.any():
            v = np.zeros((int(sel.sum()), NSPEC), f) + w0[sel, None] * B[0]
            v = v + w1[sel, None] * B[i1]
            v = v + w2[sel, None] * B[i2]
            out[sel] = v * _lit(f, .86445)
    return np.maximum(out, f(0))


def evaluate(tex, q, basis=None):
    """Texture::Evaluate of a record of the classes above at the interactions q [n, 15] = (p, dpdx, dpdy, u, v, dudx, dvdx,
    dudy, dvdy). A spectrum record -> [n, 31] with the material's Clamp() (what the lobes read); a float record -> [n], times
    post_scale. Also the decisions [n, k]."""
    f = tex.f
    q = np.asarray(q)
    p, dpdx, dpdy, uv, duv = q[:, 0:3], q[:, 3:6], q[:, 6:9], q[:, 9:11], q[:, 11:15]
    if tex.type == TEX_CHECKERBOARD3D:
        odd = checkerboard3d(tex, p)
        w, dec = np.where(odd, f(1), f(0)), odd[:, None].astype(np.int64)
    else:
        c, dec = map2d(tex, p, dpdx, dpdy, uv, duv)
        if tex.type == TEX_UV:          # uv.h:57-59
            rgb = np.stack([c[:, 0] - np.floor(c[:, 0]), c[:, 1] - np.floor(c[:, 1]), np.zeros(len(c), f)], axis=1)
            return from_rgb(rgb, basis), dec
        if tex.type == TEX_BILERP:      # bilerp.h:59-60
            s, t, b = c[:, 0], c[:, 1], tex.bilerp
            one = f(1)
            return ((one - s) * (one - t) * b[0] + (one - s) * t * b[1] + s * (one - t) * b[2] + s * t * b[3]) * tex.post_scale, dec
        if tex.type == TEX_DOTS:
            inside, _, d2 = dots(c[:, 0:2])
            w = np.where(inside, f(1), f(0))
        else:
            assert tex.type == TEX_CHECKERBOARD
            w, d2 = checkerboard2d(c, tex.aa_none != 0)
        dec = np.concatenate([dec, d2], axis=1)
    if tex.is_float:
        if tex.type in (TEX_DOTS, TEX_CHECKERBOARD3D):      # one operand or the other
            return np.where(w != 0, tex.spec2[0], tex.spec1[0]) * tex.post_scale, dec
        return ((f(1) - w) * tex.spec1[0] + w * tex.spec2[0]) * tex.post_scale, dec
    return np.maximum((f(1) - w)[:, None] * tex.spec1[None, :] + w[:, None] * tex.spec2[None, :], f(0)), dec


def same_decisions(dec32, dec64):
    """The queries on which both precisions took every discrete decision alike."""
    return (dec32 == dec64).all(axis=1)
