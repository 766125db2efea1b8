"""LightSource "projection" restated in numpy, in float32 and in float64: the constructor, Projection, Sample_Li and Power of
src/lights/projection.cpp, with Perspective (transform.cpp:1078-1088), Transform::operator()(Point3f) (transform.h:222-233:
the division by wp is a multiplication by 1 / wp, geometry.h:500-504, and happens unless wp == 1), Bounds2::Inside / Offset
(geometry.h:1218-1222, 818-823) and MIPMap::Lookup (light_restatement.lookup: width 0, level 0, Repeat). Nothing here calls
the product's kernels or the oracle. The inputs are the records of scene.desc: the mi_light, level 0 of its map (the mi_envmap
that has no distribution) and the rgb_illum basis.

With f = np.float32 every operation rounds to float32 in the reference's order; tan is taken in float64 and rounded once (the
convention of light_restatement.py). With f = np.float64 the same formulas give the value the float32 chain approximates.
hither = 1e-3f and yon = 1e30f stay the float32 constants in both: they are parameters.

Decisions are returned beside the values: "behind" (wl.z < hither), "inside" (the screen bounds, inclusive at both ends),
"black" (Projection == 0). A query on which the two precisions decide differently is unsure and decides nothing in a test."""
import math

import numpy as np

import light_restatement as lr
from disk_shape import _cols, normalize

PROJECTION = 5            # MI_LIGHT_PROJECTION
HITHER, YON = np.float32(1e-3), np.float32(1e30)
NSPEC = lr.NSPEC


class Map:
    """Level 0 of projectionMap: the mi_envmap the light's proj_map names (width, height, rgb; no distribution)."""

    def __init__(self, rec, f=np.float32):
        self.f = f
        self.width, self.height = int(rec.width), int(rec.height)
        assert int(rec.nu) == 0 and int(rec.nv) == 0, "a projection map carries no distribution"
        self.rgb = np.ctypeslib.as_array(rec.rgb, shape=(self.width * self.height * 3,)).astype(np.float32).astype(f).reshape(
            self.height, self.width, 3)


class Light:
    """mi_light `index` (type PROJECTION) of a scene description with its map and the rgb_illum basis."""

    def __init__(self, desc, index, f=np.float32):
        rec = desc.lights[index]
        assert int(rec.type) == PROJECTION
        self.f = f

        def a(v):
            return np.array(list(v), np.float32).astype(f)
        self.type = PROJECTION
        self.L, self.pos = a(rec.L), a(rec.pos)
        self.l2w, self.w2l = a(rec.l2w).reshape(3, 3), a(rec.w2l).reshape(3, 3)
        self.cos_total_width = f(np.float32(rec.cos_total_width))
        self.screen, self.proj, self.hither = a(rec.screen), a(rec.proj).reshape(4, 4), f(np.float32(rec.hither))
        self.proj_centre = a(rec.proj_centre)
        self.map = Map(desc.envmaps[rec.proj_map], f) if rec.proj_map >= 0 else None
        self.rgb_illum = np.array([list(r) for r in desc.rgb_illum], np.float32).astype(f)


def both(desc, index):
    return Light(desc, index, np.float32), Light(desc, index, np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the constructor, projection.cpp:45-74
def mat_mul(a, b):
    """Matrix4x4::Mul, transform.h:86-93: four products summed left to right."""
    f = a.dtype.type
    r = np.zeros((4, 4), f)
    for i in range(4):
        for j in range(4):
            r[i, j] = a[i, 0] * b[0, j] + a[i, 1] * b[1, j] + a[i, 2] * b[2, j] + a[i, 3] * b[3, j]
    return r


def perspective(fov, f=np.float32):
    """Perspective(fov, hither, yon): (m, mInv). m = Scale(invTan, invTan, 1) * persp; its inverse the product of the members'
    inverses, persp's by hand (it is what the Gauss-Jordan routine finds, up to rounding that the float64 chain does not see)."""
    n, far = f(HITHER), f(YON)
    persp = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, far / (far - n), -far * n / (far - n)], [0, 0, 1, 0]], f)
    # (Radians(fov) = (Pi / 180) * fov in the scalar type, the half angle's tangent in float64 rounded once)
    rad = (f(math.pi) / f(180)) * f(np.float32(fov))
    inv_tan = f(1) / f(math.tan(float(rad / f(2))))
    scale = np.diag([inv_tan, inv_tan, f(1), f(1)]).astype(f)
    scale_inv = np.diag([f(1) / inv_tan, f(1) / inv_tan, f(1), f(1)]).astype(f)
    a, b = persp[2, 2], persp[2, 3]
    persp_inv = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, f(1) / b, -a / b]], f)
    return mat_mul(scale, persp), mat_mul(persp_inv, scale_inv)


def apply_point(m, p):
    """Transform::operator()(Point3f), transform.h:222-233."""
    f = m.dtype.type
    x, y, z = _cols(p.astype(f))
    out = [m[r, 0] * x + m[r, 1] * y + m[r, 2] * z + m[r, 3] for r in range(4)]
    wp = out[3]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = f(1) / wp
        return np.stack([np.where(wp == 1, out[k], inv * out[k]) for k in range(3)], axis=1)


def screen_bounds(resolution, f=np.float32):
    """[pMin.x, pMin.y, pMax.x, pMax.y] from the file's own resolution (w, h), None without a map."""
    aspect = f(1) if resolution is None else f(np.float32(resolution[0])) / f(np.float32(resolution[1]))
    if aspect > 1:
        return np.array([-aspect, -1, aspect, 1], f)
    return np.array([-1, f(-1) / aspect, 1, f(1) / aspect], f)


def cos_total_width(fov, screen, f=np.float32):
    """The z of Normalize(Inverse(lightProjection)(pMax.x, pMax.y, 0))."""
    _, m_inv = perspective(fov, f)
    corner = apply_point(m_inv, np.array([[screen[2], screen[3], 0]], f))
    return normalize(corner)[0, 2]


# ---------------------------------------------------------------------------------------------------------------------
# Projection, projection.cpp:87-98; Sample_Li, 76-85; Power, 100-106
def projection(light, w):
    """Projection(w) for world directions w [n, 3]: dict(value [n, 31], behind, inside, black, p [n, 2], st [n, 2])."""
    f = light.f
    wl = lr.mul3(light.w2l, w.astype(f))
    behind = wl[:, 2] < light.hither
    p = apply_point(light.proj, wl)
    sc = light.screen
    with np.errstate(invalid="ignore"):
        inside = (p[:, 0] >= sc[0]) & (p[:, 0] <= sc[2]) & (p[:, 1] >= sc[1]) & (p[:, 1] <= sc[3])
    black = behind | ~inside
    ox, oy = p[:, 0] - sc[0], p[:, 1] - sc[1]
    if sc[2] > sc[0]:
        ox = ox / (sc[2] - sc[0])
    if sc[3] > sc[1]:
        oy = oy / (sc[3] - sc[1])
    st = np.stack([ox, oy], axis=1)
    if light.map is None:
        value = np.ones((len(w), NSPEC), f)
    else:
        s, t = np.where(black, f(0.5), ox), np.where(black, f(0.5), oy)   # (a defined lookup where the value is discarded)
        value = lr.from_rgb_illuminant(lr.lookup(light.map, s, t), light.rgb_illum)
    value = np.where(black[:, None], f(0), value)
    return dict(value=value, behind=behind, inside=inside, black=black, p=p[:, :2], st=st, wl=wl)


def sample_li(light, ref_p):
    """Sample_Li(ref): wi, pdf = 1, Li = (I * Projection(-wi)) / DistanceSquared(pLight, ref.p), bin by bin in that order."""
    f = light.f
    ref_p = ref_p.astype(f)
    pl = np.broadcast_to(light.pos, ref_p.shape)
    wi = normalize(pl - ref_p)
    pr = projection(light, -wi)
    d = pl - ref_p
    d2 = lr.dot(d, d)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        li = (light.L[None, :] * pr["value"]) / d2[:, None]
    return dict(wi=wi, pdf=np.ones(len(ref_p), f), p=pl.copy(), Li=li, black=pr["black"], behind=pr["behind"], inside=pr["inside"],
                P=pr["value"], st=pr["st"], d2=d2)


def out_of(r):
    """A sample in the probe's layout [n, SAMPLE_FLOATS]: wi, pdf, pLight.p, pLight.n (0), Li."""
    n = len(r["wi"])
    return np.concatenate([r["wi"], r["pdf"][:, None], r["p"], np.zeros((n, 3), r["wi"].dtype), r["Li"]], axis=1)


def spectrum_y(spec, cie_y):
    """SampledSpectrum::y(), spectrum.h:412-420: the sum in bin order, clamped at 0, times (705 - 395) / (CIE_Y_integral * 31)."""
    f = spec.dtype.type
    yy = f(0)
    for i in range(NSPEC):
        yy = yy + cie_y[i] * spec[i]
    yy = max(yy, f(0))
    return yy * f(np.float32(705 - 395)) / f(np.float32(106.856895) * np.float32(31))


def power(light):
    """Power(): map * I * 2 * Pi * (1.f - cosTotalWidth), left to right; map = Spectrum(Lookup((.5, .5), .5), Illuminant) as the
    record carries it (proj_centre; Spectrum(1) without a map: the trilinear lookup needs the pyramid, which the front end holds)."""
    f = light.f
    return light.proj_centre * light.L * f(2) * f(np.float32(math.pi)) * (f(1) - light.cos_total_width)
