"""Shape "disk" restated in numpy, in float32 and in float64, for the tests of the disk path. Each function names the
reference lines it follows (src/shapes/disk.cpp, src/core/shape.cpp, src/core/transform.h, src/core/sampling.cpp); nothing
here calls the product or the oracle. With f = np.float32 every operation rounds to float32 in the reference's order (numpy
does not contract a * b + c); atan2 / sin / cos are taken in float64 and rounded once, the "correctly rounded" convention of
the device's libm. With f = np.float64 the same formulas give the value the float32 chain approximates; the error-bound
constant gamma(3) stays the float32 one in both, it is a parameter of the algorithm."""
import math

import numpy as np

EPS = np.float32(2.0 ** -24)                                        # MachineEpsilon, pbrt.h:124
GAMMA3 = np.float32(3) * EPS / (np.float32(1) - np.float32(3) * EPS)    # gamma(3), pbrt.h:331-333


class Disk:
    """The fields of an mi_disk record (or of a ctypes Disk), matrices as [4, 4] arrays of the scalar type f."""

    def __init__(self, rec, f=np.float32):
        self.f = f
        self.o2w = np.array(list(rec.o2w), np.float32).reshape(4, 4).astype(f)
        self.w2o = np.array(list(rec.w2o), np.float32).reshape(4, 4).astype(f)
        self.height, self.radius = f(np.float32(rec.height)), f(np.float32(rec.radius))
        self.inner_radius, self.phi_max = f(np.float32(rec.inner_radius)), f(np.float32(rec.phi_max))
        self.reverse, self.swaps = bool(rec.reverse_orientation), bool(rec.swaps_handedness)

    def area(self):
        """Disk::Area, disk.cpp:125-127."""
        return self.phi_max * self.f(0.5) * (self.radius * self.radius - self.inner_radius * self.inner_radius)


def _cols(v):
    return v[:, 0], v[:, 1], v[:, 2]


def xf_point(m, p, want_err=False):
    """Transform::operator()(Point3f[, Vector3f *pError]), transform.h:222-249: left-to-right sums, the homogeneous divide,
    and gamma(3) * the sum of the absolute terms as the error bound."""
    f = m.dtype.type
    x, y, z = _cols(p)
    out = []
    for r in range(4):
        out.append(m[r, 0] * x + m[r, 1] * y + m[r, 2] * z + m[r, 3])
    xp, yp, zp, wp = out
    one = wp == 1
    inv = np.where(one, f(1), f(1) / np.where(one, f(1), wp))
    q = np.stack([np.where(one, xp, inv * xp), np.where(one, yp, inv * yp), np.where(one, zp, inv * zp)], axis=1)
    if not want_err:
        return q
    err = np.stack([np.abs(m[r, 0] * x) + np.abs(m[r, 1] * y) + np.abs(m[r, 2] * z) + np.abs(m[r, 3]) for r in range(3)], axis=1)
    return q, f(GAMMA3) * err


def xf_vector(m, v):
    """Transform::operator()(Vector3f), transform.h:251-257."""
    x, y, z = _cols(v)
    return np.stack([m[r, 0] * x + m[r, 1] * y + m[r, 2] * z for r in range(3)], axis=1)


def xf_normal(m_inv, n):
    """Transform::operator()(Normal3f), transform.h:259-265: the transpose of the inverse."""
    x, y, z = _cols(n)
    return np.stack([m_inv[0, c] * x + m_inv[1, c] * y + m_inv[2, c] * z for c in range(3)], axis=1)


def normalize(v):
    """Normalize(v) = v / v.Length(), Vector3::operator/ multiplying by the reciprocal (geometry.h:245-249, 1024)."""
    f = v.dtype.type
    x, y, z = _cols(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = f(1) / np.sqrt(x * x + y * y + z * z)
        return v * inv[:, None]


def cross(a, b):
    """Cross(v1, v2), geometry.h:985-993: the products in double, rounded once."""
    f = a.dtype.type
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    return np.cross(a64, b64).astype(f)


def object_ray(disk, o, d):
    """Transform::operator()(Ray, oErr, dErr) with WorldToObject, transform.h:384-396: the origin moves along d by its
    error bound, tMax does not change."""
    o_obj, o_err = xf_point(disk.w2o, o, True)
    d_obj = xf_vector(disk.w2o, d)
    dx, dy, dz = _cols(d_obj)
    len2 = dx * dx + dy * dy + dz * dz
    dot = np.abs(dx) * o_err[:, 0] + np.abs(dy) * o_err[:, 1] + np.abs(dz) * o_err[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        dt = np.where(len2 > 0, dot / np.where(len2 > 0, len2, 1), 0).astype(disk.f)
    return o_obj + d_obj * dt[:, None], d_obj


def intersect(disk, rays):
    """Disk::Intersect, disk.cpp:48-97, and what Transform::operator()(SurfaceInteraction) (transform.cpp:255-288) makes
    of it. rays [n, 7] = o, d, tMax. Returns hit [n] and, valid where hit: t, p, n (world, unit, flipped by
    reverseOrientation ^ transformSwapsHandedness: interaction.cpp:60-65), uv, dpdu, dpdv (world). IntersectP
    (disk.cpp:99-123) is the same verdict."""
    f = disk.f
    rays = np.asarray(rays)
    o, d, tmax = rays[:, 0:3].astype(f), rays[:, 3:6].astype(f), rays[:, 6].astype(f)
    oo, dd = object_ray(disk, o, d)
    with np.errstate(divide="ignore", invalid="ignore"):
        parallel = dd[:, 2] == 0                                                   # :58
        t = (disk.height - oo[:, 2]) / np.where(parallel, f(1), dd[:, 2])          # :59
        hit = ~parallel & ~((t <= 0) | (t >= tmax))                               # :60
        p = oo + dd * t[:, None]                                                   # :63  ray(t) = o + d * t
        dist2 = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]                              # :64
        hit &= ~((dist2 > disk.radius * disk.radius) | (dist2 < disk.inner_radius * disk.inner_radius))   # :65
        phi = np.arctan2(p[:, 1].astype(np.float64), p[:, 0].astype(np.float64)).astype(f)   # :69
        phi = np.where(phi < 0, phi + f(2) * f(math.pi), phi)                      # :70
        hit &= ~(phi > disk.phi_max)                                               # :71
        u = phi / disk.phi_max                                                     # :74
        r_hit = np.sqrt(dist2)                                                     # :75
        v = f(1) - (r_hit - disk.inner_radius) / (disk.radius - disk.inner_radius)  # :76-77
        zero = np.zeros_like(u)
        dpdu = np.stack([-disk.phi_max * p[:, 1], disk.phi_max * p[:, 0], zero], axis=1)   # :78
        inv_r = f(1) / r_hit
        span = disk.radius - disk.inner_radius
        dpdv = np.stack([(p[:, 0] * span) * inv_r, (p[:, 1] * span) * inv_r, zero], axis=1)   # :79-80
        p_obj = np.stack([p[:, 0], p[:, 1], np.full_like(u, disk.height)], axis=1)   # :84
        n_obj = normalize(cross(dpdu, dpdv))                                       # interaction.cpp:55
        if disk.reverse ^ disk.swaps:
            n_obj = -n_obj
        out = dict(hit=hit, t=t, p=xf_point(disk.o2w, p_obj), n=normalize(xf_normal(disk.w2o, n_obj)),
                   uv=np.stack([u, v], axis=1), dpdu=xf_vector(disk.o2w, dpdu), dpdv=xf_vector(disk.o2w, dpdv))
    return out


def concentric_sample_disk(u, f):
    """ConcentricSampleDisk, sampling.cpp:113-130."""
    u = np.asarray(u).astype(f)
    ox, oy = f(2) * u[:, 0] - f(1), f(2) * u[:, 1] - f(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        first = np.abs(ox) > np.abs(oy)
        r = np.where(first, ox, oy)
        theta = np.where(first, f(math.pi / 4) * (oy / ox), f(math.pi / 2) - f(math.pi / 4) * (ox / oy))
        c, s = np.cos(theta.astype(np.float64)).astype(f), np.sin(theta.astype(np.float64)).astype(f)
    origin = (ox == 0) & (oy == 0)
    return np.where(origin, f(0), r * c), np.where(origin, f(0), r * s)


def sample_area(disk, u):
    """Disk::Sample(u, pdf), disk.cpp:129-138: the full disk of `radius`, whatever the inner radius and the sweep."""
    f = disk.f
    dx, dy = concentric_sample_disk(u, f)
    p_obj = np.stack([dx * disk.radius, dy * disk.radius, np.full_like(dx, disk.height)], axis=1)
    n = normalize(xf_normal(disk.w2o, np.tile(np.array([[0, 0, 1]], f), (len(dx), 1))))
    if disk.reverse:
        n = -n
    return xf_point(disk.o2w, p_obj), n, f(1) / disk.area()


def sample(disk, ref, u):
    """Shape::Sample(ref, u, pdf), shape.cpp:56-70: to solid angle; 0 on a zero-length wi or an infinite value."""
    f = disk.f
    p, n, pdf_area = sample_area(disk, u)
    ref = np.broadcast_to(np.asarray(ref).astype(f), p.shape)
    wi = p - ref
    len2 = wi[:, 0] * wi[:, 0] + wi[:, 1] * wi[:, 1] + wi[:, 2] * wi[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        w = normalize(wi)
        dist2 = len2                                                               # DistanceSquared(ref.p, intr.p)
        absdot = np.abs(n[:, 0] * -w[:, 0] + n[:, 1] * -w[:, 1] + n[:, 2] * -w[:, 2])
        pdf = pdf_area * (dist2 / absdot)
    pdf = np.where((len2 == 0) | np.isinf(pdf), f(0), pdf)
    return p, n, pdf


def pdf(disk, ref, wi):
    """Shape::Pdf(ref, wi), shape.cpp:72-87, for a bare reference point (no normal, no error bound: SpawnRay leaves from
    ref.p itself)."""
    f = disk.f
    wi = np.asarray(wi).astype(f)
    ref = np.broadcast_to(np.asarray(ref).astype(f), wi.shape)
    rays = np.concatenate([ref, wi, np.full((len(wi), 1), np.inf, f)], axis=1)
    it = intersect(disk, rays)
    to = ref - it["p"]
    with np.errstate(divide="ignore", invalid="ignore"):
        dist2 = to[:, 0] * to[:, 0] + to[:, 1] * to[:, 1] + to[:, 2] * to[:, 2]
        absdot = np.abs(it["n"][:, 0] * -wi[:, 0] + it["n"][:, 1] * -wi[:, 1] + it["n"][:, 2] * -wi[:, 2])
        val = dist2 / (absdot * disk.area())
    val = np.where(np.isinf(val), f(0), val)
    return np.where(it["hit"], val, f(0))


def both(rec):
    return Disk(rec, np.float32), Disk(rec, np.float64)


def bar(a32, a64, sel):
    """The rule of test_realistic_gpu._bars: four times the worst deviation of the float32 restatement from the float64
    one over the selected queries, never below 8 ulp (float32) of the largest component."""
    a, b = np.asarray(a32)[sel].astype(np.float64), np.asarray(a64)[sel]
    if a.size == 0:
        return 0.0
    return float(max(4 * np.abs(a - b).max(), 8 * float(np.spacing(np.float32(np.abs(b).max())))))


def xf_ray(m, rays):
    """Transform::operator()(Ray), transform.h:262-277 -- WorldToInstance of a TransformedPrimitive (primitive.cpp:78-99): the
    origin moves along d by its error bound and tMax shrinks by the same dt. m: [4, 4] of the scalar type."""
    f = m.dtype.type
    rays = np.asarray(rays)
    o, o_err = xf_point(m, rays[:, 0:3].astype(f), True)
    d = xf_vector(m, rays[:, 3:6].astype(f))
    tmax = rays[:, 6].astype(f)
    dx, dy, dz = _cols(d)
    len2 = dx * dx + dy * dy + dz * dz
    dot = np.abs(dx) * o_err[:, 0] + np.abs(dy) * o_err[:, 1] + np.abs(dz) * o_err[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        dt = np.where(len2 > 0, dot / np.where(len2 > 0, len2, 1), 0).astype(f)
    return np.concatenate([o + d * dt[:, None], d, (tmax - dt)[:, None]], axis=1)


def closest(disks, rays, instance_w2i=None):
    """The closest hit among `disks` (Disk objects of one scalar type) for world rays [n, 7]: (t [n], inf where none; index
    [n], -1 where none; hit verdict per disk [len(disks), n]). instance_w2i: the disks belong to an object seen through that
    WorldToInstance matrix; t is then the instance ray's, which TransformedPrimitive hands back as the world ray's tMax."""
    f = disks[0].f
    q = xf_ray(np.asarray(instance_w2i, np.float32).reshape(4, 4).astype(f), rays) if instance_w2i is not None else np.asarray(rays)
    best = np.full(len(q), np.inf, f)
    idx = np.full(len(q), -1, np.int64)
    verdicts = []
    for k, dk in enumerate(disks):
        it = intersect(dk, q)
        verdicts.append(it["hit"])
        closer = it["hit"] & (it["t"] < best)
        best = np.where(closer, it["t"], best)
        idx = np.where(closer, k, idx)
    return best, idx, np.array(verdicts)
