"""Shape "sphere" restated in numpy, in float32 and in float64, for the tests of the sphere path, under the rules of
disk_shape.py: each function names the reference lines it follows (src/shapes/sphere.cpp, src/core/efloat.h, src/core/shape.cpp,
src/core/transform.h, src/core/geometry.h, src/core/sampling.cpp); nothing here calls the product or the oracle. With
f = np.float32 every operation rounds to float32 in the reference's order; atan2 / acos / sin / cos are taken in float64 and
rounded once. With f = np.float64 the same formulas give the value the float32 chain approximates; the float32 algorithm
constants -- gamma(3), gamma(5), MachineEpsilon, 1e-5f * radius, the float Pi -- stay the float32 ones.

EFloat (efloat.h:48-200) is a triple of arrays (v, low, high). v has the scalar type f. The bounds are float32 in both
variants: each is formed from values of type f, rounded to float32 and stepped outward by one float32 ulp with np.nextafter
(NextFloatUp / NextFloatDown, pbrt.h:268-296). The widths of the intervals decide which root Sphere::Intersect trusts; like
gamma(3) in the disk file they are a parameter of the algorithm, not a rounding error of the restatement, so the float64
variant keeps them float32-sized around its float64 value."""
import math

import numpy as np

from disk_shape import (EPS, GAMMA3, _cols, bar, cross, normalize, object_ray, xf_normal, xf_point, xf_ray,   # noqa: F401
                        xf_vector)

GAMMA5 = np.float32(5) * EPS / (np.float32(1) - np.float32(5) * EPS)    # gamma(5), pbrt.h:331-333
PI = np.float32(math.pi)                                                # Pi, pbrt.h:139
_UP, _DOWN = np.float32(np.inf), np.float32(-np.inf)


class Sphere:
    """The fields of an mi_sphere record (sphere.h:49-66: thetaMin / thetaMax are the constructor's), matrices as [4, 4]
    arrays of the scalar type f."""

    def __init__(self, rec, f=np.float32):
        self.f = f
        self.o2w = np.array(list(rec.o2w), np.float32).reshape(4, 4).astype(f)
        self.w2o = np.array(list(rec.w2o), np.float32).reshape(4, 4).astype(f)
        self.radius, self.phi_max = f(np.float32(rec.radius)), f(np.float32(rec.phi_max))
        self.z_min, self.z_max = f(np.float32(rec.z_min)), f(np.float32(rec.z_max))
        self.theta_min, self.theta_max = f(np.float32(rec.theta_min)), f(np.float32(rec.theta_max))
        self.reverse, self.swaps = bool(rec.reverse_orientation), bool(rec.swaps_handedness)

    def area(self):
        """Sphere::Area, sphere.cpp:217."""
        return self.phi_max * self.radius * (self.z_max - self.z_min)


def both(rec):
    return Sphere(rec, np.float32), Sphere(rec, np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# EFloat
def _up(x):
    """NextFloatUp of the float32 nearest to x (pbrt.h:268-281: +inf stays, -0 counts as +0)."""
    return np.nextafter(np.asarray(x).astype(np.float32), _UP)


def _down(x):
    """NextFloatDown (pbrt.h:283-296)."""
    return np.nextafter(np.asarray(x).astype(np.float32), _DOWN)


def ef(v, err=None):
    """EFloat(v, err), efloat.h:52-63."""
    v = np.asarray(v)
    if err is None:
        return v, v.astype(np.float32), v.astype(np.float32)
    err = np.asarray(err).astype(v.dtype)
    exact = err == 0
    return v, np.where(exact, v.astype(np.float32), _down(v - err)), np.where(exact, v.astype(np.float32), _up(v + err))


def ef_add(a, b):
    """EFloat::operator+, efloat.h:76-88."""
    return a[0] + b[0], _down(a[1] + b[1]), _up(a[2] + b[2])


def ef_sub(a, b):
    """EFloat::operator-, efloat.h:100-110."""
    return a[0] - b[0], _down(a[1] - b[2]), _up(a[2] - b[1])


def ef_mul(a, b):
    """EFloat::operator*, efloat.h:111-126."""
    prod = [a[1] * b[1], a[2] * b[1], a[1] * b[2], a[2] * b[2]]
    return (a[0] * b[0], _down(np.minimum(np.minimum(prod[0], prod[1]), np.minimum(prod[2], prod[3]))),
            _up(np.maximum(np.maximum(prod[0], prod[1]), np.maximum(prod[2], prod[3]))))


def ef_div(a, b):
    """EFloat::operator/, efloat.h:127-149: everything when the divisor's interval straddles zero."""
    with np.errstate(divide="ignore", invalid="ignore"):
        div = [a[1] / b[1], a[2] / b[1], a[1] / b[2], a[2] / b[2]]
        straddles = (b[1] < 0) & (b[2] > 0)
        low = np.where(straddles, _DOWN, _down(np.minimum(np.minimum(div[0], div[1]), np.minimum(div[2], div[3]))))
        high = np.where(straddles, _UP, _up(np.maximum(np.maximum(div[0], div[1]), np.maximum(div[2], div[3]))))
        return a[0] / b[0], low, high


def ef_sqrt(a):
    """sqrt(EFloat), efloat.h:225-235."""
    with np.errstate(invalid="ignore"):
        return np.sqrt(a[0]), _down(np.sqrt(a[1])), _up(np.sqrt(a[2]))


def quadratic(A, B, C):
    """Quadratic(EFloat A, B, C, t0, t1), efloat.h:267-285: the discriminant and its root in double whatever the scalar
    type, the root's interval MachineEpsilon * root wide. Returns (solved [n], t0, t1), t0.v <= t1.v."""
    f = A[0].dtype.type
    a64, b64, c64 = A[0].astype(np.float64), B[0].astype(np.float64), C[0].astype(np.float64)
    discrim = b64 * b64 - 4. * a64 * c64                                       # :269
    solved = ~(discrim < 0.)                                                   # :270
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        root = np.sqrt(discrim)                                                # :271
        frd = ef(root.astype(f), (np.float64(EPS) * root).astype(np.float32))  # :273
        half = ef(np.full_like(A[0], f(-.5)))
        neg = B[0] < 0                                                         # :277
        qa, qb = ef_mul(half, ef_sub(B, frd)), ef_mul(half, ef_add(B, frd))    # :278-280
        q = tuple(np.where(neg, x, y) for x, y in zip(qa, qb))
        t0, t1 = ef_div(q, A), ef_div(C, q)                                    # :281-282
        swap = t0[0] > t1[0]                                                   # :283
    return solved, tuple(np.where(swap, y, x) for x, y in zip(t0, t1)), tuple(np.where(swap, x, y) for x, y in zip(t0, t1))


# ---------------------------------------------------------------------------------------------------------------------
def _object_ray_err(sphere, o, d):
    """Transform::operator()(Ray, oErr, dErr) with WorldToObject, transform.h:384-396 (disk_shape.object_ray), and the two
    error bounds it hands back: gamma(3) times the sums of the absolute terms (transform.h:222-249, 277-297)."""
    f = sphere.f
    oo, dd = object_ray(sphere, o, d)
    _, o_err = xf_point(sphere.w2o, o, True)
    m = sphere.w2o
    x, y, z = _cols(d)
    d_err = f(GAMMA3) * np.stack([np.abs(m[r, 0] * x) + np.abs(m[r, 1] * y) + np.abs(m[r, 2] * z) for r in range(3)], axis=1)
    return oo, dd, o_err, d_err


def _hit_point(sphere, oo, dd, t):
    """sphere.cpp:80-86: ray(t), re-projected onto the sphere; the pole nudge; phi in [0, 2 pi)."""
    f = sphere.f
    p = oo + dd * t[:, None]                                                           # :80
    scale = sphere.radius / np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] + p[:, 2] * p[:, 2])   # :83
    p = p * scale[:, None]
    pole = (p[:, 0] == 0) & (p[:, 1] == 0)
    p[:, 0] = np.where(pole, f(np.float32(1e-5)) * sphere.radius, p[:, 0])             # :84
    phi = np.arctan2(p[:, 1].astype(np.float64), p[:, 0].astype(np.float64)).astype(f)  # :85
    phi = np.where(phi < 0, phi + f(2) * f(PI), phi)                                   # :86
    clipped = (((sphere.z_min > -sphere.radius) & (p[:, 2] < sphere.z_min)) |
               ((sphere.z_max < sphere.radius) & (p[:, 2] > sphere.z_max)) | (phi > sphere.phi_max))   # :89-90
    return p, phi, clipped


def intersect(sphere, rays):
    """Sphere::Intersect, sphere.cpp:49-155, and what Transform::operator()(SurfaceInteraction) (transform.cpp:255-288)
    makes of it. rays [n, 7] = o, d, tMax. Returns hit [n] and, valid where hit: root (0: t0 answered, 1: t1), t, p, n
    (world, unit, flipped by reverseOrientation ^ transformSwapsHandedness: interaction.cpp:60-65), uv, dpdu, dpdv (world).
    Also t0, t1 (the values of both roots) and solved (the discriminant is not negative). IntersectP (sphere.cpp:158-215) is
    the same verdict."""
    f = sphere.f
    rays = np.asarray(rays)
    o, d, tmax = rays[:, 0:3].astype(f), rays[:, 3:6].astype(f), rays[:, 6].astype(f)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        oo, dd, o_err, d_err = _object_ray_err(sphere, o, d)                          # :56
        ox, oy, oz = [ef(oo[:, k], o_err[:, k]) for k in range(3)]                    # :61
        dx, dy, dz = [ef(dd[:, k], d_err[:, k]) for k in range(3)]                    # :62
        a = ef_add(ef_add(ef_mul(dx, dx), ef_mul(dy, dy)), ef_mul(dz, dz))            # :63
        two = ef(np.full(len(rays), f(2)))
        b = ef_mul(two, ef_add(ef_add(ef_mul(dx, ox), ef_mul(dy, oy)), ef_mul(dz, oz)))   # :64
        rad = ef(np.full(len(rays), sphere.radius))
        c = ef_sub(ef_add(ef_add(ef_mul(ox, ox), ef_mul(oy, oy)), ef_mul(oz, oz)), ef_mul(rad, rad))   # :65
        solved, t0, t1 = quadratic(a, b, c)                                           # :69
        hit = solved & ~((t0[2] > tmax) | (t1[1] <= 0))                               # :72
        second = t0[1] <= 0                                                           # :74
        hit &= ~(second & (t1[2] > tmax))                                             # :76
        t = np.where(second, t1[0], t0[0])
        p, phi, clipped = _hit_point(sphere, oo, dd, t)                               # :80-90
        retry = clipped & ~(t == t1[0]) & ~(t1[2] > tmax)                             # :91-92
        hit &= ~clipped | retry
        p1, phi1, clipped1 = _hit_point(sphere, oo, dd, t1[0])                        # :93-101
        hit &= ~(retry & clipped1)                                                    # :102-104
        root = np.where(second | retry, 1, 0)
        t = np.where(retry, t1[0], t)
        p, phi = np.where(retry[:, None], p1, p), np.where(retry, phi1, phi)
        u = phi / sphere.phi_max                                                      # :108
        theta = np.arccos(np.clip(p[:, 2] / sphere.radius, f(-1), f(1)).astype(np.float64)).astype(f)   # :109
        span = sphere.theta_max - sphere.theta_min
        v = (theta - sphere.theta_min) / span                                         # :110
        z_radius = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1])                     # :113
        inv = f(1) / z_radius
        cos_phi, sin_phi = p[:, 0] * inv, p[:, 1] * inv                               # :115-116
        dpdu = np.stack([-sphere.phi_max * p[:, 1], sphere.phi_max * p[:, 0], np.zeros_like(u)], axis=1)   # :117
        sin_theta = np.sin(theta.astype(np.float64)).astype(f)
        dpdv = span * np.stack([p[:, 2] * cos_phi, p[:, 2] * sin_phi, -sphere.radius * sin_theta], axis=1)   # :118-120
        n_obj = normalize(cross(dpdu, dpdv))                                          # interaction.cpp:55
        if sphere.reverse ^ sphere.swaps:
            n_obj = -n_obj
        return dict(hit=hit, root=root, t=t, p=xf_point(sphere.o2w, p), n=normalize(xf_normal(sphere.w2o, n_obj)),
                    uv=np.stack([u, v], axis=1), dpdu=xf_vector(sphere.o2w, dpdu), dpdv=xf_vector(sphere.o2w, dpdv),
                    t0=t0[0], t1=t1[0], solved=solved)


def uniform_sample_sphere(u, f):
    """UniformSampleSphere, sampling.cpp:98-103."""
    u = np.asarray(u).astype(f)
    z = f(1) - f(2) * u[:, 0]
    r = np.sqrt(np.maximum(f(0), f(1) - z * z))
    phi = (f(2) * f(PI)) * u[:, 1]
    c, s = np.cos(phi.astype(np.float64)).astype(f), np.sin(phi.astype(np.float64)).astype(f)
    return np.stack([r * c, r * s, z], axis=1)


def sample_area(sphere, u):
    """Sphere::Sample(u, pdf), sphere.cpp:219-230: the whole sphere, whatever the clipping parameters."""
    f = sphere.f
    p_obj = sphere.radius * uniform_sample_sphere(u, f)                               # :220
    n = normalize(xf_normal(sphere.w2o, p_obj))                                       # :222
    if sphere.reverse:
        n = -n                                                                        # :223
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = sphere.radius / np.sqrt(p_obj[:, 0] * p_obj[:, 0] + p_obj[:, 1] * p_obj[:, 1] + p_obj[:, 2] * p_obj[:, 2])
    return xf_point(sphere.o2w, p_obj * scale[:, None]), n, f(1) / sphere.area()       # :225-228


def _center(sphere):
    return xf_point(sphere.o2w, np.zeros((1, 3), sphere.f))[0]                        # (*ObjectToWorld)(Point3f(0, 0, 0))


def _dist2(a, b):
    w = a - b
    return w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2]


def inside(sphere, ref):
    """sphere.cpp:237-239 for a bare reference point: OffsetRayOrigin (geometry.h:1495-1509) of a zero normal and a zero
    error bound is the point itself."""
    ref = np.asarray(ref).astype(sphere.f).reshape(1, 3)
    return bool(_dist2(ref, _center(sphere)[None, :])[0] <= sphere.radius * sphere.radius)


def cone_pdf(sphere, ref):
    """sphere.cpp:262-263, 289 (and :303-305 with UniformConePdf, sampling.cpp:109-111)."""
    f = sphere.f
    ref = np.asarray(ref).astype(f).reshape(1, 3)
    with np.errstate(divide="ignore"):
        sin2 = sphere.radius * sphere.radius / _dist2(ref, _center(sphere)[None, :])[0]
        cos_max = np.sqrt(np.maximum(f(0), f(1) - sin2))
        return f(1) / (f(2) * f(PI) * (f(1) - cos_max)), cos_max


def sample(sphere, ref, u):
    """Sphere::Sample(ref, u, pdf), sphere.cpp:232-292, for a bare reference point: uniformly over the area from inside,
    uniformly over the subtended cone from outside. Returns p, n, pdf."""
    f = sphere.f
    u = np.asarray(u).astype(f)
    ref1 = np.asarray(ref).astype(f)
    if inside(sphere, ref1):                                                          # :239
        p, n, pdf_area = sample_area(sphere, u)                                       # :240
        refs = np.broadcast_to(ref1, p.shape)
        wi = p - refs                                                                 # :241
        len2 = wi[:, 0] * wi[:, 0] + wi[:, 1] * wi[:, 1] + wi[:, 2] * wi[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            w = normalize(wi)                                                         # :247
            absdot = np.abs(n[:, 0] * -w[:, 0] + n[:, 1] * -w[:, 1] + n[:, 2] * -w[:, 2])
            pdf = pdf_area * (_dist2(refs, p) / absdot)                               # :248
        pdf = np.where((len2 == 0) | np.isinf(pdf), f(0), pdf)                        # :242-243, 250
        return p, n, pdf
    pc = _center(sphere)
    r = sphere.radius
    wc = normalize((pc - ref1)[None, :])                                              # :255
    x, y, z = wc[0]
    if abs(x) > abs(y):                                                               # CoordinateSystem, geometry.h:1029-1036
        wcx = np.array([[-z, 0, x]], f) * (f(1) / np.sqrt(x * x + z * z))
    else:
        wcx = np.array([[0, z, -y]], f) * (f(1) / np.sqrt(y * y + z * z))
    wcy = cross(wc, wcx)
    pdf, cos_max = cone_pdf(sphere, ref1)                                             # :262-263, 289
    cos_t = (f(1) - u[:, 0]) + u[:, 0] * cos_max                                      # :264
    sin_t = np.sqrt(np.maximum(f(0), f(1) - cos_t * cos_t))                           # :265
    phi = u[:, 1] * f(2) * f(PI)                                                      # :266
    dc = np.sqrt(_dist2(ref1[None, :], pc[None, :])[0])                               # :269
    ds_ = dc * cos_t - np.sqrt(np.maximum(f(0), r * r - dc * dc * sin_t * sin_t))     # :270-272
    cos_a = (dc * dc + r * r - ds_ * ds_) / (f(2) * dc * r)                           # :273
    sin_a = np.sqrt(np.maximum(f(0), f(1) - cos_a * cos_a))                           # :274
    c, s = np.cos(phi.astype(np.float64)).astype(f), np.sin(phi.astype(np.float64)).astype(f)
    n = (sin_a * c)[:, None] * -wcx + (sin_a * s)[:, None] * -wcy + cos_a[:, None] * -wc   # SphericalDirection, geometry.h:1476-1481
    p = pc[None, :] + r * n                                                           # :279
    if sphere.reverse:
        n = -n                                                                        # :286
    return p, n, np.full(len(u), pdf, f)


def pdf(sphere, ref, wi):
    """Sphere::Pdf(ref, wi), sphere.cpp:294-306: the cone's pdf for every direction from outside; Shape::Pdf
    (shape.cpp:72-87) from inside, for a bare reference point (SpawnRay leaves from ref.p itself)."""
    f = sphere.f
    wi = np.asarray(wi).astype(f)
    ref1 = np.asarray(ref).astype(f)
    if not inside(sphere, ref1):
        return np.full(len(wi), cone_pdf(sphere, ref1)[0], f)
    refs = np.broadcast_to(ref1, wi.shape)
    it = intersect(sphere, np.concatenate([refs, wi, np.full((len(wi), 1), np.inf, f)], axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        absdot = np.abs(it["n"][:, 0] * -wi[:, 0] + it["n"][:, 1] * -wi[:, 1] + it["n"][:, 2] * -wi[:, 2])
        val = _dist2(refs, it["p"]) / (absdot * sphere.area())
    val = np.where(np.isinf(val), f(0), val)
    return np.where(it["hit"], val, f(0))


def closest(spheres, rays, instance_w2i=None):
    """The closest hit among `spheres` (Sphere objects of one scalar type) for world rays [n, 7]: (t [n], inf where none;
    index [n], -1 where none; hit verdict per sphere [len(spheres), n]). Each sphere sees the ray with tMax as given, as the
    reference's aggregate would on meeting it first. instance_w2i: the spheres belong to an object seen through that
    WorldToInstance matrix; t is then the instance ray's, which TransformedPrimitive hands back as the world ray's tMax."""
    f = spheres[0].f
    q = xf_ray(np.asarray(instance_w2i, np.float32).reshape(4, 4).astype(f), rays) if instance_w2i is not None else np.asarray(rays)
    best = np.full(len(q), np.inf, f)
    idx = np.full(len(q), -1, np.int64)
    verdicts = []
    for k, sk in enumerate(spheres):
        it = intersect(sk, q)
        verdicts.append(it["hit"])
        closer = it["hit"] & (it["t"] < best)
        best = np.where(closer, it["t"], best)
        idx = np.where(closer, k, idx)
    return best, idx, np.array(verdicts)
