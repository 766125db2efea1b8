"""The shapes, ray families and reference points shared by test_sphere_restatement.py (CPU) and test_sphere_gpu.py: six
spheres, one scene each, and per shape a few thousand rays aimed in object space and taken to world space in float64 with the
record's ObjectToWorld. Nothing here calls the product's kernels or the oracle; the restatement (sphere_shape.py) is asked
where a family needs a hit point or a root to start from."""
import math

import numpy as np

import sphere_shape as ss

HEAD = ('LookAt 0 2.5 9  0 1 0  0 1 0\nCamera "perspective" "float fov" [45]\n'
        'Film "image" "integer xresolution" [%(res)d] "integer yresolution" [%(res)d]\n'
        'Sampler "halton" "integer pixelsamples" [%(spp)d]\n%(integrator)s\n%(accel)sWorldBegin\n')


def text(body, res=32, spp=4, integrator='Integrator "path" "integer maxdepth" [1]', accel=""):
    return HEAD % dict(res=res, spp=spp, integrator=integrator, accel=accel) + body + "WorldEnd\n"


SHAPES = {
    "full": 'Shape "sphere" "float radius" [1.5]',
    "zmin/zmax": 'Shape "sphere" "float radius" [1.5] "float zmin" [-.6] "float zmax" [.9]',
    "phimax": 'Shape "sphere" "float radius" [1.5] "float phimax" [200]',
    "all three": 'Shape "sphere" "float radius" [1.5] "float zmin" [-1] "float zmax" [.5] "float phimax" [300]',
    "rotated, scaled": 'Translate .5 1 -1\nRotate 35 1 2 .5\nScale 1 -2 .5\nShape "sphere" "float radius" [1.5] "float zmin" [-1] "float zmax" [.5] "float phimax" [300]',
    "reversed, small, far": 'ReverseOrientation\nTranslate 40 -25 60\nShape "sphere" "float radius" [1e-2] "float phimax" [270]',
}
PLAIN = 'AttributeBegin\nTranslate -7 -7 -7\nShape "sphere" "float radius" [.25]\nAttributeEnd\n'


def scene(pt, name, plain=True):
    """(scene, index of the probed sphere). With `plain` the scene also holds a small full sphere far from every ray of the
    families, written before the probed shape for every other name: the probed quadric is then 1, not 0."""
    k = list(SHAPES).index(name)
    body = 'AttributeBegin\n%s\nAttributeEnd\n' % SHAPES[name]
    first = plain and k % 2 == 1
    if plain:
        body = PLAIN + body if first else body + PLAIN
    s = pt.Scene(text=text(body))
    assert s.errors == [] and s.desc.n_spheres == (2 if plain else 1) and s.desc.n_disks == 0
    q = 1 if first else 0
    assert float(s.desc.spheres[q].radius) != 0.25
    return s, q


def rays_of(o, d, tmax=np.inf):
    o, d = np.atleast_2d(np.asarray(o, np.float64)), np.atleast_2d(np.asarray(d, np.float64))
    out = np.zeros((max(len(o), len(d)), 7), np.float32)
    out[:, 0:3], out[:, 3:6], out[:, 6] = o, d, tmax
    return out


def origin_noise(rec):
    """gamma(3) |c| / r: the error bound that WorldToObject hands Sphere::Intersect for the ray's origin (transform.h:222-249),
    as a fraction of the radius. The interval of a root is at least that wide, and a root whose upper bound passes tMax is
    rejected (sphere.cpp:72-76): where this is above 1e-4, tMax = t (1 + 1e-4) is a miss in the reference itself."""
    c = np.abs(np.array(list(rec.o2w), np.float64).reshape(4, 4)[:3, 3]).max()
    return float(ss.GAMMA3) * c / float(rec.radius)


class Family:
    def __init__(self, name, rays, expect=None, conditioned=True, exact_t=False, root=None, targets=None):
        self.name, self.rays, self.expect, self.conditioned, self.exact_t, self.root = name, rays, expect, conditioned, exact_t, root
        self.targets = targets          # world-space points the rays aim at (mode 2 reuses them)


def families(rec, rng, n=300):
    """The ray families of one sphere record. expect: True / False where the great majority of the family must hit / miss;
    root: the root that must answer where it hits; conditioned: t, p, n, uv, dpdu, dpdv are compared (else the verdict
    alone); exact_t: t is compared bit for bit with the float32 restatement."""
    m = np.array(list(rec.o2w), np.float64).reshape(4, 4)
    r, zlo, zhi, pm = float(rec.radius), float(rec.z_min), float(rec.z_max), float(rec.phi_max)
    eps = 1e-3
    noise = origin_noise(rec)
    beyond_hits = True if noise < 1e-5 else (False if noise > 1e-3 else None)
    z_clip_lo, z_clip_hi, phi_clip = zlo > -r, zhi < r, pm < 2 * math.pi - 0.1
    rotated = not np.array_equal(m[:3, :3], np.diag(np.diag(m[:3, :3]))) or not np.array_equal(np.diag(m[:3, :3]), np.ones(3))

    def world_p(p_obj):
        return (np.concatenate([p_obj, np.ones((len(p_obj), 1))], axis=1) @ m.T)[:, :3]

    def to_world(p_obj, o_obj):
        p, o = world_p(p_obj), world_p(o_obj)
        return o, p - o

    def surface(z, phi):
        rho = np.sqrt(np.maximum(r * r - z * z, 0))
        return np.stack([rho * np.cos(phi), rho * np.sin(phi), z], axis=1)

    def kept(k):
        return surface(rng.uniform(zlo + 0.01 * r, zhi - 0.01 * r, k), rng.uniform(0.02, pm - 0.02, k))

    def clipped(k):
        """Points of the full sphere that the clipping parameters remove, off every boundary by the margins of `kept`."""
        kinds = [c for c, on in (("lo", z_clip_lo), ("hi", z_clip_hi), ("phi", phi_clip)) if on]
        which = rng.choice(len(kinds), k)
        z, phi = rng.uniform(-0.99 * r, 0.99 * r, k), rng.uniform(0.02, 2 * math.pi - 0.02, k)
        for i, c in enumerate(kinds):
            mine = which == i
            if c == "lo":
                z[mine] = rng.uniform(-0.99 * r, zlo - 0.01 * r, mine.sum())
            elif c == "hi":
                z[mine] = rng.uniform(zhi + 0.01 * r, 0.99 * r, mine.sum())
            else:
                phi[mine] = rng.uniform(pm + 0.02, 2 * math.pi - 0.02, mine.sum())
        return surface(z, phi)

    def unit(k):
        v = rng.normal(size=(k, 3))
        return v / np.linalg.norm(v, axis=1)[:, None]

    def outside_of(t_obj):
        """An origin outside the tangent plane at t_obj: the segment to t_obj meets the sphere there first."""
        return t_obj + (rng.uniform(1, 4, len(t_obj)) * r)[:, None] * (t_obj / r + 0.6 * unit(len(t_obj)))

    def apart(make_a, make_b, k):
        """Pairs of surface points at least 0.3 r apart (the chord between them is no grazing line)."""
        a, b = make_a(4 * k), make_b(4 * k)
        ok = np.linalg.norm(a - b, axis=1) > 0.3 * r
        assert ok.sum() >= k
        return a[ok][:k], b[ok][:k]

    def through(a, b):
        """From outside through a, then b: the origin lies before a on the line a -> b."""
        s = rng.uniform(.5, 2, len(a))[:, None]
        return to_world(a, a - s * (b - a))

    out = []
    any_clip = z_clip_lo or z_clip_hi or phi_clip
    # 1: from outside at the kept surface
    t1_obj = kept(n)
    o, d = to_world(t1_obj, outside_of(t1_obj))
    f1 = Family("1 kept surface from outside", rays_of(o, d), True, exact_t=True, root=0, targets=o + d)
    out.append(f1)
    f2 = None
    if any_clip:
        # 2: in through the clipped part, out through the kept surface: the second root answers
        a, b = apart(clipped, kept, n)
        o, d = through(a, b)
        f2 = Family("2 through a clipped part, out through kept surface", rays_of(o, d), True, exact_t=True, root=1, targets=o + d)
        out.append(f2)
        # 3: clipped on both sides
        a, b = apart(clipped, clipped, n)
        o, d = through(a, b)
        out.append(Family("3 clipped on both sides", rays_of(o, d), False, targets=o + d))
        # 4: either side of each clip boundary
        k = n // 2
        for label, on, zs, phis in (("zmin", z_clip_lo, zlo, None), ("zmax", z_clip_hi, zhi, None), ("phimax", phi_clip, None, pm)):
            if not on:
                continue
            for side, sign in (("inside", 1), ("outside", -1)):
                if phis is None:
                    inward = sign if label == "zmin" else -sign
                    t_obj = surface(np.full(k, zs + inward * eps * r), rng.uniform(0.02, pm - 0.02, k))
                else:
                    t_obj = surface(rng.uniform(zlo + 0.01 * r, zhi - 0.01 * r, k), np.full(k, phis - sign * eps))
                o, d = to_world(t_obj, outside_of(t_obj))
                out.append(Family("4 %s of %s" % (side, label), rays_of(o, d), True if sign > 0 else None,
                                  root=0 if sign > 0 else 1, targets=o + d))
    # 5: origins inside the sphere
    t5_obj = kept(n)
    o_in = unit(n) * (r * rng.uniform(0, 0.9, n) ** (1 / 3))[:, None]
    o, d = to_world(t5_obj, o_in)
    f5 = Family("5 from inside at the kept surface", rays_of(o, d), True, exact_t=True, root=1, targets=o + d)
    out.append(f5)
    if any_clip:
        o, d = to_world(clipped(n // 2), o_in[:n // 2])
        out.append(Family("5 from inside at a clipped part", rays_of(o, d), False, targets=o + d))
    # 6: origins on the surface: the float32 restatement's hit points of family 1
    s32, s64 = ss.both(rec)
    hit1 = ss.intersect(s32, f1.rays)
    on = hit1["p"].astype(np.float64)
    d_out = (world_p(t1_obj + r * (t1_obj / r + 0.6 * unit(n))) - world_p(t1_obj))
    out.append(Family("6 outward from the surface", rays_of(on, d_out)[hit1["hit"]], False, conditioned=False))
    far_obj = apart(lambda k: np.tile(t1_obj, (4, 1))[:k], kept, n)
    d_in = world_p(far_obj[1]) - world_p(far_obj[0])
    o_in6 = ss.intersect(s32, rays_of(*to_world(far_obj[0], outside_of(far_obj[0]))))
    out.append(Family("6 inward from the surface", rays_of(o_in6["p"].astype(np.float64), d_in)[o_in6["hit"]], True, root=1))
    # 7: grazing, inside and outside the tangent line
    k = n // 2
    for label, b_, expect in (("inside", r * (1 - eps), True if not any_clip else None), ("outside", r * (1 + eps), False)):
        u = unit(k)
        w = np.cross(u, unit(k))
        w /= np.linalg.norm(w, axis=1)[:, None]
        pc = b_ * w
        o, d = to_world(pc, pc - (rng.uniform(2, 4, k) * r)[:, None] * u)
        out.append(Family("7 grazing, %s the tangent" % label, rays_of(o, d), expect))
    # 8: along the object z axis: pHit.x == 0 && pHit.y == 0
    k = 40
    h = rng.uniform(2, 4, k) * r * rng.choice([-1, 1], k)
    zero = np.zeros(k)
    o, d = to_world(np.stack([zero, zero, zero], axis=1), np.stack([zero, zero, h], axis=1))
    pole_kept = not (z_clip_lo and z_clip_hi)
    out.append(Family("8 along the z axis", rays_of(o, d), True if not (z_clip_lo or z_clip_hi) else (None if pole_kept else False),
                      conditioned=not rotated))
    # 9: the sphere wholly behind the origin
    out.append(Family("9 sphere behind the origin", rays_of(f1.rays[:, 0:3], -f1.rays[:, 3:6].astype(np.float64)), False))
    # 10: tMax either side of the answering root; and between the roots where the first is clipped
    for fam in (f1, f5):
        t64 = ss.intersect(s64, fam.rays)["t"]
        short, beyond = fam.rays.copy(), fam.rays.copy()
        short[:, 6], beyond[:, 6] = (t64 * (1 - 1e-4)).astype(np.float32), (t64 * (1 + 1e-4)).astype(np.float32)
        out.append(Family("10 tMax short of the root, family %s" % fam.name[0], short, False))
        out.append(Family("10 tMax beyond the root, family %s" % fam.name[0], beyond, beyond_hits, exact_t=True, root=fam.root))
        well = fam.rays.copy()
        well[:, 6] = (t64 * 1.1).astype(np.float32)
        out.append(Family("10 tMax a tenth beyond the root, family %s" % fam.name[0], well, True, exact_t=True, root=fam.root))
    if f2 is not None:
        it = ss.intersect(s64, f2.rays)
        between = f2.rays.copy()
        between[:, 6] = (0.5 * (it["t0"] + it["t1"])).astype(np.float32)
        out.append(Family("10 tMax between the roots, family 2", between, False))
    return out


def reference_points(rec):
    """World-space reference points of modes 1 and 2: (label, point float32, inside?). Sphere::Sample takes the radius as it
    stands and the centre in world space (sphere.cpp:234-239), whatever the transform's scale."""
    c = np.array(list(rec.o2w), np.float64).reshape(4, 4)[:3, 3]
    r = float(rec.radius)
    a = np.array([.48, -.6, .64])
    b = np.array([-.6, .64, .48])
    return [("generic outside", (c + 2.7 * r * a).astype(np.float32), False),
            ("far outside", (c + 200 * r * b).astype(np.float32), False),
            ("inside", (c + r * np.array([.3, -.2, .4])).astype(np.float32), True),
            ("just outside", (c + 1.001 * r * a).astype(np.float32), False),
            ("the centre", c.astype(np.float32), True)]


def sample_points(rng, k=600):
    """600 random u and the four corners of [0, 1 - 2^-24]^2."""
    top = 1 - 2.0 ** -24
    return np.concatenate([rng.random((k, 2)), [[0, 0], [0, top], [top, 0], [top, top]]]).astype(np.float32)


def radical_pairs(n):
    """(RadicalInverse(0, i), RadicalInverse(1, i)), i < n: bases 2 and 3 (lowdiscrepancy.cpp:389-424), in float64 then float32."""
    i = np.arange(n, dtype=np.int64)
    out = np.zeros((n, 2))
    for k, base in enumerate((2, 3)):
        a, inv, v = i.copy(), 1.0, np.zeros(n)
        while a.any():
            inv /= base
            v += (a % base) * inv
            a //= base
        out[:, k] = v
    return np.minimum(out, 1 - 2.0 ** -24).astype(np.float32)
