"""The lights of the path integrator restated in numpy, in float32 and in float64: Light::Sample_Li, Pdf_Li, Le and L of the
point, spot, distant, infinite and triangle-emitter lights. Each function names the reference lines it follows
(src/lights/*.cpp, src/core/sampling.h, mipmap.h, spectrum.cpp, shape.cpp, src/shapes/triangle.cpp); nothing here calls the
product or the oracle, and nothing here was written from their sources. The inputs are the records of scene.desc: the
mi_light, the tables of its mi_envmap, the rgb_illum basis and a triangle's vertices.

With f = np.float32 every operation rounds to float32 in the reference's order (numpy does not contract a * b + c); sin, cos,
acos and atan2 are taken in float64 and rounded once, the "correctly rounded" convention of the device's libm and of the
oracle under exact_libm(). With f = np.float64 the same formulas give the value the float32 chain approximates. The float32
constants of the algorithms (gamma(n), the .86445f of FromRGB) stay the float32 ones in both: they are parameters.

Discrete decisions are returned beside the values ("zero": pdf == 0, "black", the spot "branch", the Distribution2D "cell",
"hit"): a query on which the two precisions decide differently is unsure and decides nothing in a test."""
import math

import numpy as np

from disk_shape import EPS, _cols, cross, normalize

AREA, POINT, DISTANT, INFINITE, SPOT = range(5)   # mi_light_type
NSPEC = 31
SAMPLE_FLOATS = 10 + NSPEC                         # MI_LIGHT_PROBE_SAMPLE_FLOATS


def gamma(n):
    """gamma(n), pbrt.h:331-333, in float32."""
    return (np.float32(n) * EPS) / (np.float32(1) - np.float32(n) * EPS)


def _trig(fn, f, *x):
    return fn(*[np.asarray(v, np.float64) for v in x]).astype(f)


def dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def mul3(m, v):
    """Transform::operator()(Vector3f) with the 3x3 part of the matrix, transform.h:251-257."""
    x, y, z = _cols(v)
    return np.stack([m[r, 0] * x + m[r, 1] * y + m[r, 2] * z for r in range(3)], axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# records
def _arr(ptr, n, f):
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(np.float32).astype(f)


class EnvMap:
    """mi_envmap: level 0 of Lmap and the tables of the Distribution2D, as arrays of the scalar type f."""

    def __init__(self, rec, f=np.float32):
        self.f = f
        self.width, self.height, self.nu, self.nv = int(rec.width), int(rec.height), int(rec.nu), int(rec.nv)
        self.rgb = _arr(rec.rgb, self.width * self.height * 3, f).reshape(self.height, self.width, 3)
        self.cond_func = _arr(rec.cond_func, self.nv * self.nu, f).reshape(self.nv, self.nu)
        self.cond_cdf = _arr(rec.cond_cdf, self.nv * (self.nu + 1), f).reshape(self.nv, self.nu + 1)
        self.cond_func_int = _arr(rec.cond_func_int, self.nv, f)
        self.marg_func = _arr(rec.marg_func, self.nv, f)
        self.marg_cdf = _arr(rec.marg_cdf, self.nv + 1, f)
        self.marg_func_int = f(np.float32(rec.marg_func_int))


class Light:
    """mi_light `index` of a scene description, with what it points to: the environment map and the rgb_illum basis of an
    infinite light, the vertices and the orientation flag of a triangle emitter."""

    def __init__(self, desc, index, f=np.float32):
        rec = desc.lights[index]
        self.f = f

        def a(v):
            return np.array(list(v), np.float32).astype(f)
        self.type, self.two_sided = int(rec.type), bool(rec.two_sided)
        self.L, self.pos, self.dir = a(rec.L), a(rec.pos), a(rec.dir)
        self.world_radius = f(np.float32(rec.world_radius))
        self.l2w, self.w2l = a(rec.l2w).reshape(3, 3), a(rec.w2l).reshape(3, 3)
        self.cos_total_width, self.cos_falloff_start = f(np.float32(rec.cos_total_width)), f(np.float32(rec.cos_falloff_start))
        self.rec_area = np.float32(rec.area)
        if self.type == INFINITE:
            self.env = EnvMap(desc.envmaps[rec.envmap], f)
            self.rgb_illum = np.array([list(r) for r in desc.rgb_illum], np.float32).astype(f)
        if self.type == AREA:
            tri = int(rec.shape)
            assert tri >= 0, "a quadric emitter: sphere_shape.py / disk_shape.py restate those"
            mesh = desc.meshes[desc.tri_mesh[tri]]
            assert not (mesh.flags & 1), "per-vertex normals are not restated here"
            self.flip = bool(mesh.flags & 4)   # reverseOrientation ^ transformSwapsHandedness
            idx = [int(desc.tri_indices[3 * tri + k]) for k in range(3)]
            self.tri = np.array([[desc.P[3 * i + c] for c in range(3)] for i in idx], np.float32).astype(f)


def both(desc, index):
    return Light(desc, index, np.float32), Light(desc, index, np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# Distribution1D / Distribution2D, sampling.h:55-147, sampling.cpp:159-172
def distribution1d(func):
    """The constructor, sampling.h:57-69, for every row of func [m, n]: (cdf [m, n + 1], funcInt [m])."""
    f = func.dtype.type
    m, n = func.shape
    cdf = np.zeros((m, n + 1), f)
    for i in range(1, n + 1):
        cdf[:, i] = cdf[:, i - 1] + func[:, i - 1] / f(n)
    func_int = cdf[:, n].copy()
    zero = func_int == 0
    ramp = np.arange(1, n + 1).astype(f) / f(n)
    cdf[:, 1:] = np.where(zero[:, None], ramp[None, :], cdf[:, 1:] / np.where(zero, f(1), func_int)[:, None])
    return cdf, func_int


def find_interval(cdf, u):
    """FindInterval(size, cdf[i] <= u), pbrt.h:405-418, row by row: cdf [k, size], u [k]."""
    k, size = cdf.shape
    rows = np.arange(k)
    first, length = np.zeros(k, np.int64), np.full(k, size, np.int64)
    while (length > 0).any():
        act = length > 0
        half = length >> 1
        middle = first + half
        pred = cdf[rows, np.minimum(middle, size - 1)] <= u
        up = act & pred
        first = np.where(up, middle + 1, first)
        length = np.where(up, length - (half + 1), np.where(act, half, length))
    return np.clip(first - 1, 0, size - 2)


def sample_continuous(func, cdf, func_int, u):
    """Distribution1D::SampleContinuous, sampling.h:71-89, row by row: (x, pdf, offset)."""
    f = cdf.dtype.type
    rows = np.arange(len(u))
    n = func.shape[1]
    off = find_interval(cdf, u)
    c0, c1 = cdf[rows, off], cdf[rows, off + 1]
    du = u - c0
    w = c1 - c0
    du = np.where(w > 0, du / np.where(w > 0, w, f(1)), du)
    pdf = np.where(func_int > 0, func[rows, off] / np.where(func_int > 0, func_int, f(1)), f(0))
    return (off.astype(f) + du) / f(n), pdf, off


def sample_continuous_2d(env, u):
    """Distribution2D::SampleContinuous, sampling.h:127-134: d0, d1, mapPdf and the two offsets."""
    k = len(u)
    u0, u1 = u[:, 0].astype(env.f), u[:, 1].astype(env.f)
    d1, pdf1, v = sample_continuous(np.broadcast_to(env.marg_func, (k, env.nv)), np.broadcast_to(env.marg_cdf, (k, env.nv + 1)),
                                    np.broadcast_to(env.marg_func_int, (k,)), u1)
    d0, pdf0, uo = sample_continuous(env.cond_func[v], env.cond_cdf[v], env.cond_func_int[v], u0)
    return d0, d1, pdf0 * pdf1, uo, v


def pdf_2d(env, p0, p1):
    """Distribution2D::Pdf, sampling.h:135-141: (value, iu, iv)."""
    f = env.f
    iu = np.clip((p0 * f(env.nu)).astype(np.int64), 0, env.nu - 1)
    iv = np.clip((p1 * f(env.nv)).astype(np.int64), 0, env.nv - 1)
    return env.cond_func[iv, iu] / env.marg_func_int, iu, iv


# ---------------------------------------------------------------------------------------------------------------------
# the map: MIPMap::Lookup(st) with width 0 and ImageWrap::Repeat, mipmap.h:247-287; FromRGB(Illuminant), spectrum.cpp:139-172
def lookup(env, s, t):
    f = env.f
    sx, ty = s * f(env.width) - f(0.5), t * f(env.height) - f(0.5)
    s0, t0 = np.floor(sx).astype(np.int64), np.floor(ty).astype(np.int64)
    ds, dt = sx - s0.astype(f), ty - t0.astype(f)

    def texel(ss, tt):
        return env.rgb[tt % env.height, ss % env.width]
    return (((f(1) - ds) * (f(1) - dt))[:, None] * texel(s0, t0) + ((f(1) - ds) * dt)[:, None] * texel(s0, t0 + 1)
            + (ds * (f(1) - dt))[:, None] * texel(s0 + 1, t0) + (ds * dt)[:, None] * texel(s0 + 1, t0 + 1))


def from_rgb_illuminant(rgb, basis):
    """basis: rgbIllum2Spect{White, Cyan, Magenta, Yellow, Red, Green, Blue} [7, 31]."""
    f = rgb.dtype.type
    r, g, b = _cols(rgb)
    WHITE, CYAN, MAGENTA, YELLOW, RED, GREEN, BLUE = range(7)
    first, second = r <= g, g <= b
    c_r = (r <= g) & (r <= b)
    c_g = ~c_r & (g <= r) & (g <= b)
    c_b = ~c_r & ~c_g
    out = np.zeros((len(rgb), NSPEC), f)
    # (selector, w0, i1, w1, i2, w2)
    for sel, w0, i1, w1, i2, w2 in ((c_r & second, r, CYAN, g - r, BLUE, b - g), (c_r & ~second, r, CYAN, b - r, GREEN, g - b),
                                    (c_g & (r <= b), g, MAGENTA, r - g, BLUE, b - r), (c_g & ~(r <= b), g, MAGENTA, b - g, RED, r - b),
                                    (c_b & first, b, YELLOW, r - b, GREEN, g - r), (c_b & ~first, b, YELLOW, g - b, RED, r - g)):
        val = (w0[:, None] * basis[WHITE][None, :] + w1[:, None] * basis[i1][None, :]) + w2[:, None] * basis[i2][None, :]
        out = np.where(sel[:, None], val, out)
    out = out * f(np.float32(0.86445))
    return np.maximum(out, f(0))


def spherical_theta(v):
    f = v.dtype.type
    return _trig(np.arccos, f, np.clip(v[:, 2], f(-1), f(1)))


def spherical_phi(v):
    f = v.dtype.type
    p = _trig(np.arctan2, f, v[:, 1], v[:, 0])
    return np.where(p < 0, p + f(2) * f(math.pi), p)


# ---------------------------------------------------------------------------------------------------------------------
# InfiniteAreaLight, infinite.cpp:91-141
def infinite_le(light, d):
    f = light.f
    w = normalize(mul3(light.w2l, d.astype(f)))
    s, t = spherical_phi(w) * f(0.5 / math.pi), spherical_theta(w) * f(1 / math.pi)
    return from_rgb_illuminant(lookup(light.env, s, t), light.rgb_illum)


def infinite_pdf_li(light, w):
    """Pdf_Li, infinite.cpp:133-141: the transformed direction is NOT normalised (Le's is)."""
    f = light.f
    wi = mul3(light.w2l, w.astype(f))
    theta, phi = spherical_theta(wi), spherical_phi(wi)
    sin_theta = _trig(np.sin, f, theta)
    val, iu, iv = pdf_2d(light.env, phi * f(0.5 / math.pi), theta * f(1 / math.pi))
    zero = sin_theta == 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pdf = np.where(zero, f(0), val / (f(2) * f(math.pi) * f(math.pi) * sin_theta))
    return dict(pdf=pdf, zero=pdf == 0, cell=iv * light.env.nu + iu)


def infinite_sample_li(light, ref_p, u):
    f = light.f
    env = light.env
    d0, d1, map_pdf, uo, v = sample_continuous_2d(env, u)
    none = map_pdf == 0
    theta, phi = d1 * f(math.pi), d0 * f(2) * f(math.pi)
    cos_t, sin_t = _trig(np.cos, f, theta), _trig(np.sin, f, theta)
    sin_p, cos_p = _trig(np.sin, f, phi), _trig(np.cos, f, phi)
    wi = mul3(light.l2w, np.stack([sin_t * cos_p, sin_t * sin_p, cos_t], axis=1))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pdf = np.where(sin_t == 0, f(0), map_pdf / (f(2) * f(math.pi) * f(math.pi) * sin_t))
    p = ref_p.astype(f) + wi * (f(2) * light.world_radius)
    li = from_rgb_illuminant(lookup(env, d0, d1), light.rgb_illum)
    z = none[:, None]
    pdf = np.where(none, f(0), pdf)
    return dict(wi=np.where(z, f(0), wi), pdf=pdf, p=np.where(z, f(0), p), n=np.zeros_like(wi), Li=np.where(z, f(0), li),
                zero=pdf == 0, none=none, d0=d0, d1=d1, map_pdf=map_pdf, offset=v * env.nu + uo)


# ---------------------------------------------------------------------------------------------------------------------
# PointLight (point.cpp:44-53), SpotLight (spot.cpp:51-74), DistantLight (distant.cpp:49-59)
def _dist2(a, b):
    d = a - b
    return dot(d, d)


def point_sample_li(light, ref_p):
    f = light.f
    ref_p = ref_p.astype(f)
    p = np.broadcast_to(light.pos, ref_p.shape)
    wi = normalize(p - ref_p)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        li = light.L[None, :] / _dist2(p, ref_p)[:, None]
    return dict(wi=wi, pdf=np.ones(len(ref_p), f), p=p.copy(), n=np.zeros_like(wi), Li=li, zero=np.zeros(len(ref_p), bool))


def spot_falloff(light, w):
    """SpotLight::Falloff, spot.cpp:63-72: (falloff, branch) -- branch 0 outside the cone, 1 in the band, 2 inside."""
    f = light.f
    wl = normalize(mul3(light.w2l, w))
    cos_theta = wl[:, 2]
    ct, cs = light.cos_total_width, light.cos_falloff_start
    outside = cos_theta < ct
    inside = ~outside & (cos_theta >= cs)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        delta = (cos_theta - ct) / (cs - ct)
    band = (delta * delta) * (delta * delta)
    return np.where(outside, f(0), np.where(inside, f(1), band)), np.where(outside, 0, np.where(inside, 2, 1)), cos_theta


def spot_sample_li(light, ref_p):
    r = point_sample_li(light, ref_p)
    falloff, branch, cos_theta = spot_falloff(light, -r["wi"])
    p = np.broadcast_to(light.pos, r["wi"].shape)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r["Li"] = (light.L[None, :] * falloff[:, None]) / _dist2(p, ref_p.astype(light.f))[:, None]
    r.update(branch=branch, falloff=falloff, cos_theta=cos_theta)
    return r


def distant_sample_li(light, ref_p):
    f = light.f
    ref_p = ref_p.astype(f)
    wi = np.broadcast_to(light.dir, ref_p.shape).copy()
    return dict(wi=wi, pdf=np.ones(len(ref_p), f), p=ref_p + wi * (f(2) * light.world_radius), n=np.zeros_like(wi),
                Li=np.broadcast_to(light.L, (len(ref_p), NSPEC)).copy(), zero=np.zeros(len(ref_p), bool))


# ---------------------------------------------------------------------------------------------------------------------
# the triangle emitter: Triangle::Sample / Area / Intersect (triangle.cpp:188-346, 575-608), Shape::Sample(ref, u) / Pdf(ref, wi)
# (shape.cpp:56-87), DiffuseAreaLight (diffuse.cpp:68-87, diffuse.h:56-58)
def tri_normal(light):
    p0, p1, p2 = light.tri
    n = normalize(cross((p1 - p0)[None, :], (p2 - p0)[None, :]))[0]
    return -n if light.flip else n


def tri_area(light):
    p0, p1, p2 = light.tri
    c = cross((p1 - p0)[None, :], (p2 - p0)[None, :])
    return light.f(0.5) * np.sqrt(dot(c, c))[0]


def tri_sample(light, u):
    """Triangle::Sample(u): (p, n, pdf by area)."""
    f = light.f
    p0, p1, p2 = light.tri
    u0, u1 = u[:, 0].astype(f), u[:, 1].astype(f)
    su0 = np.sqrt(u0)
    b0, b1 = f(1) - su0, u1 * su0
    p = b0[:, None] * p0 + b1[:, None] * p1 + (f(1) - b0 - b1)[:, None] * p2
    n = np.broadcast_to(tri_normal(light), p.shape).copy()
    return p, n, np.full(len(u), f(1) / tri_area(light), f)


def shape_sample(light, ref_p, u):
    """Shape::Sample(ref, u, pdf), shape.cpp:56-70: (p, n, pdf by solid angle)."""
    f = light.f
    ref_p = ref_p.astype(f)
    p, n, pdf = tri_sample(light, u)
    wi = p - ref_p
    same = dot(wi, wi) == 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        wi = normalize(wi)
        pdf = pdf * (_dist2(ref_p, p) / np.abs(dot(n, -wi)))
    pdf = np.where(same | np.isinf(pdf), f(0), pdf)
    return p, n, pdf


def area_sample_li(light, ref_p, u):
    f = light.f
    ref_p = ref_p.astype(f)
    p, n, pdf = shape_sample(light, ref_p, u)
    d = p - ref_p
    none = (pdf == 0) | (dot(d, d) == 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        wi = normalize(d)
    side = dot(n, -wi)
    black = ~none & ~(light.two_sided | (side > 0))
    li = np.where((none | black)[:, None], f(0), np.broadcast_to(light.L, (len(u), NSPEC)))
    z = none[:, None]
    return dict(wi=np.where(z, f(0), wi), pdf=np.where(none, f(0), pdf), p=np.where(z, f(0), p), n=np.where(z, f(0), n), Li=li,
                zero=none, black=black, side=side)


def area_l(light, n, w):
    """DiffuseAreaLight::L(intr, w), diffuse.h:56-58: (spectrum, emits)."""
    f = light.f
    emits = light.two_sided | (dot(n.astype(f), w.astype(f)) > 0)
    return np.where(emits[:, None], np.broadcast_to(light.L, (len(n), NSPEC)), f(0)), emits


def _permute(v, kx, ky, kz):
    rows = np.arange(len(v))
    return np.stack([v[rows, kx], v[rows, ky], v[rows, kz]], axis=1)


def tri_intersect(light, o, d):
    """Triangle::Intersect(ray) with tMax = Infinity and no alpha texture, triangle.cpp:188-346: hit, t, p, n. The (u, v)
    partial derivatives only matter through the degenerate-triangle test, which the cases never meet (asserted)."""
    f = light.f
    p0, p1, p2 = light.tri
    o, d = o.astype(f), d.astype(f)
    ad = np.abs(d)
    kz = np.where(ad[:, 0] > ad[:, 1], np.where(ad[:, 0] > ad[:, 2], 0, 2), np.where(ad[:, 1] > ad[:, 2], 1, 2))   # MaxDimension
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    dp = _permute(d, kx, ky, kz)
    t0, t1, t2 = (_permute(p[None, :] - o, kx, ky, kz) for p in (p0, p1, p2))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        sx, sy, sz = -dp[:, 0] / dp[:, 2], -dp[:, 1] / dp[:, 2], f(1) / dp[:, 2]
        x0, y0 = t0[:, 0] + sx * t0[:, 2], t0[:, 1] + sy * t0[:, 2]
        x1, y1 = t1[:, 0] + sx * t1[:, 2], t1[:, 1] + sy * t1[:, 2]
        x2, y2 = t2[:, 0] + sx * t2[:, 2], t2[:, 1] + sy * t2[:, 2]
        e0, e1, e2 = x1 * y2 - y1 * x2, x2 * y0 - y2 * x0, x0 * y1 - y0 * x1
        if f is np.float32:   # the fall-back to double precision at an edge, triangle.cpp:234-245
            again = (e0 == 0) | (e1 == 0) | (e2 == 0)
            X0, Y0, X1, Y1, X2, Y2 = (v.astype(np.float64) for v in (x0, y0, x1, y1, x2, y2))
            e0 = np.where(again, (Y2 * X1 - X2 * Y1).astype(f), e0)
            e1 = np.where(again, (Y0 * X2 - X0 * Y2).astype(f), e1)
            e2 = np.where(again, (Y1 * X0 - X1 * Y0).astype(f), e2)
        hit = ~(((e0 < 0) | (e1 < 0) | (e2 < 0)) & ((e0 > 0) | (e1 > 0) | (e2 > 0)))
        det = e0 + e1 + e2
        hit &= det != 0
        z0, z1, z2 = t0[:, 2] * sz, t1[:, 2] * sz, t2[:, 2] * sz
        t_scaled = e0 * z0 + e1 * z1 + e2 * z2
        inf = f(np.inf)
        hit &= ~((det < 0) & ((t_scaled >= 0) | (t_scaled < inf * det)))
        hit &= ~((det > 0) & ((t_scaled <= 0) | (t_scaled > inf * det)))
        inv_det = f(1) / det
        b0, b1, b2, t = e0 * inv_det, e1 * inv_det, e2 * inv_det, t_scaled * inv_det
        g2, g3, g5 = f(gamma(2)), f(gamma(3)), f(gamma(5))
        max_zt = np.maximum(np.maximum(np.abs(z0), np.abs(z1)), np.abs(z2))
        max_xt = np.maximum(np.maximum(np.abs(x0), np.abs(x1)), np.abs(x2))
        max_yt = np.maximum(np.maximum(np.abs(y0), np.abs(y1)), np.abs(y2))
        delta_z = g3 * max_zt
        delta_x, delta_y = g5 * (max_xt + max_zt), g5 * (max_yt + max_zt)
        delta_e = f(2) * (g2 * max_xt * max_yt + delta_y * max_xt + delta_x * max_yt)
        max_e = np.maximum(np.maximum(np.abs(e0), np.abs(e1)), np.abs(e2))
        delta_t = f(3) * (g3 * max_e * max_zt + delta_e * max_zt + delta_z * max_e) * np.abs(inv_det)
        hit &= ~(t <= delta_t)
        p = b0[:, None] * p0 + b1[:, None] * p1 + b2[:, None] * p2
    ng = cross((p2 - p0)[None, :], (p1 - p0)[None, :])
    assert dot(ng, ng)[0] != 0, "a degenerate triangle"
    n = normalize(cross((p0 - p2)[None, :], (p1 - p2)[None, :]))[0]
    if light.flip:
        n = -n
    return dict(hit=hit, t=t, p=p, n=np.broadcast_to(n, p.shape))


def shape_pdf(light, ref_p, wi):
    """Shape::Pdf(ref, wi), shape.cpp:72-87. The reference point carries no error bound, so SpawnRay starts at ref.p itself
    (OffsetRayOrigin adds a zero offset and rounds nothing, interaction.h / geometry.h:1449-1467)."""
    f = light.f
    ref_p, wi = ref_p.astype(f), wi.astype(f)
    it = tri_intersect(light, ref_p, wi)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pdf = _dist2(ref_p, it["p"]) / (np.abs(dot(it["n"], -wi)) * tri_area(light))
    pdf = np.where(~it["hit"] | np.isinf(pdf), f(0), pdf)
    return dict(pdf=pdf, zero=pdf == 0, hit=it["hit"])


# ---------------------------------------------------------------------------------------------------------------------
# the three calls of the probe
def sample_li(light, ref_p, u):
    """Light::Sample_Li(ref, u) in the layout of the probe's mode 0 (see out_of)."""
    if light.type == AREA:
        return area_sample_li(light, ref_p, u)
    if light.type == INFINITE:
        return infinite_sample_li(light, ref_p, u)
    if light.type == POINT:
        return point_sample_li(light, ref_p)
    if light.type == SPOT:
        return spot_sample_li(light, ref_p)
    return distant_sample_li(light, ref_p)


def pdf_li(light, ref_p, wi):
    if light.type == AREA:
        return shape_pdf(light, ref_p, wi)
    if light.type == INFINITE:
        return infinite_pdf_li(light, wi)
    z = np.zeros(len(wi), light.f)
    return dict(pdf=z, zero=z == 0)


def out_of(r):
    """A sample_li record as the [n, SAMPLE_FLOATS] array of the probe: wi, pdf, pLight.p, pLight.n, Li."""
    return np.concatenate([r["wi"], r["pdf"][:, None], r["p"], r["n"], r["Li"]], axis=1)


def decisions(light, r):
    """The discrete decisions of a sample_li record, one integer row per query."""
    cols = [r["zero"].astype(np.int64), (r["Li"] == 0).all(axis=1).astype(np.int64)]
    if light.type == SPOT:
        cols.append(r["branch"])
    return np.stack(cols, axis=1)
