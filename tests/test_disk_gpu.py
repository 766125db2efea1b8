"""Shape "disk" on the GPU, stage by stage. disk_shape.py restates the disk in float32 and float64; the unchanged oracle knows no
disks, so it is only ever given the twin of a scene (the same text without its disk lines) for camera rays, sampler values and
the hits on everything else. A query whose verdict (hit / miss) differs between the two restatements is "unsure" and decides
nothing; each case asserts on the CPU that at most 1 % of its queries are. Bars: four times the worst float32-vs-float64
deviation of the restatement, never below 8 ulp of the largest component (disk_shape.bar)."""
import math

import numpy as np
import pytest

import disk_shape as ds
import trace_check as tc

pytestmark = pytest.mark.gpu

HEAD = ('LookAt 0 2.5 9  0 1 0  0 1 0\nCamera "perspective" "float fov" [45]\n'
        'Film "image" "integer xresolution" [%(res)d] "integer yresolution" [%(res)d]\n'
        'Sampler "halton" "integer pixelsamples" [%(spp)d]\n%(integrator)s\n%(accel)sWorldBegin\n')
_cache = {}


def _text(body, res=32, spp=4, integrator='Integrator "path" "integer maxdepth" [1]', accel=""):
    return HEAD % dict(res=res, spp=spp, integrator=integrator, accel=accel) + body + "WorldEnd\n"


def _twin_text(text):
    """The same scene without its disks (every disk is written on a line of its own)."""
    lines = text.split("\n")
    assert any('Shape "disk"' in l for l in lines)
    return "\n".join(l for l in lines if 'Shape "disk"' not in l)


def _pair(pt, body, **kw):
    text = _text(body, **kw)
    s, twin = pt.Scene(text=text), pt.Scene(text=_twin_text(text))
    assert s.errors == [] and twin.errors == [] and s.desc.n_disks > 0 and twin.desc.n_disks == 0
    assert twin.desc.n_tris == s.desc.n_tris and twin.desc.n_spheres == s.desc.n_spheres
    return s, twin


def _all_samples(scene):
    sb = list(scene.desc.film.sample_bounds)
    return [(px, py, n) for py in range(sb[1], sb[3]) for px in range(sb[0], sb[2]) for n in range(scene.spp)]


def _rel_l2(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / max((b ** 2).sum(), 1e-30)))


def _rays(o, d, tmax=np.inf):
    o, d = np.atleast_2d(np.asarray(o, np.float64)), np.atleast_2d(np.asarray(d, np.float64))
    n = max(len(o), len(d))
    out = np.zeros((n, 7), np.float32)
    out[:, 0:3], out[:, 3:6], out[:, 6] = o, d, tmax
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1: the probe against the restatement
SHAPES = {
    "full": 'Shape "disk" "float radius" [1.5]',
    "annulus": 'Shape "disk" "float radius" [1.5] "float innerradius" [.6]',
    "phimax 200": 'Shape "disk" "float radius" [1.5] "float phimax" [200]',
    "height .7": 'Shape "disk" "float radius" [1.5] "float height" [.7] "float innerradius" [.4] "float phimax" [300]',
    "rotated, scaled": 'Translate .5 1 -1\nRotate 35 1 2 .5\nScale 1 -2 .5\nShape "disk" "float radius" [1.5] "float innerradius" [.5] "float phimax" [250] "float height" [.3]',
    "reversed": 'ReverseOrientation\nRotate -60 1 0 0\nShape "disk" "float radius" [1.5] "float phimax" [270]',
}


def _probe_rays(rec, rng):
    """World rays aimed from object space: through the interior, the hole, the missing sector, inside and outside the rim by a
    thousandth of the radius, parallel to the plane (d.z = 0 exactly in object space: the world ray is exact too where the
    transform is the identity), starting on the plane, and interior rays with tMax just short of / just beyond the hit."""
    m = np.array(list(rec.o2w), np.float64).reshape(4, 4)
    r, ri, h, pm = float(rec.radius), float(rec.inner_radius), float(rec.height), float(rec.phi_max)

    def to_world(p_obj, o_obj):
        p = np.concatenate([p_obj, np.ones((len(p_obj), 1))], axis=1) @ m.T
        o = np.concatenate([o_obj, np.ones((len(o_obj), 1))], axis=1) @ m.T
        return o[:, :3], (p - o)[:, :3]

    def targets(rad, phi):
        return np.stack([rad * np.cos(phi), rad * np.sin(phi), np.full_like(rad, h)], axis=1)

    n = 400
    origins = lambda k: np.stack([rng.uniform(-3, 3, k), rng.uniform(-3, 3, k), h + rng.choice([-1, 1], k) * rng.uniform(.5, 4, k)], axis=1)
    parts = []
    lo = max(ri, 0.0)
    phi_in = rng.uniform(0.02, pm - 0.02, n)
    parts.append(to_world(targets(rng.uniform(lo + 0.01, r - 0.01, n), phi_in), origins(n)))                 # interior
    if ri > 0:
        parts.append(to_world(targets(rng.uniform(0, ri - 0.01, n // 2), rng.uniform(0, 2 * math.pi, n // 2)), origins(n // 2)))   # the hole
        parts.append(to_world(targets(np.full(n // 4, ri * (1 - 1e-3)), rng.uniform(0.02, pm - 0.02, n // 4)), origins(n // 4)))
        parts.append(to_world(targets(np.full(n // 4, ri * (1 + 1e-3)), rng.uniform(0.02, pm - 0.02, n // 4)), origins(n // 4)))
    if pm < 2 * math.pi - 0.1:
        parts.append(to_world(targets(rng.uniform(lo + 0.01, r - 0.01, n // 2), rng.uniform(pm + 0.02, 2 * math.pi - 0.02, n // 2)), origins(n // 2)))   # the missing sector
        parts.append(to_world(targets(rng.uniform(lo + 0.01, r - 0.01, n // 4), np.full(n // 4, pm - 1e-3)), origins(n // 4)))
        parts.append(to_world(targets(rng.uniform(lo + 0.01, r - 0.01, n // 4), np.full(n // 4, pm + 1e-3)), origins(n // 4)))
    parts.append(to_world(targets(np.full(n // 4, r * (1 - 1e-3)), rng.uniform(0.02, pm - 0.02, n // 4)), origins(n // 4)))   # the rim
    parts.append(to_world(targets(np.full(n // 4, r * (1 + 1e-3)), rng.uniform(0.02, pm - 0.02, n // 4)), origins(n // 4)))
    parts.append(to_world(targets(rng.uniform(r + .1, 3 * r, n // 4), rng.uniform(0, 2 * math.pi, n // 4)), origins(n // 4)))   # outside
    k = n // 4                                                                                              # parallel to the plane
    o_par = np.stack([rng.uniform(-3, 3, k), rng.uniform(-3, 3, k), h + rng.choice([0.0, .25, -.5], k)], axis=1)
    parts.append(to_world(o_par + np.stack([rng.uniform(-1, 1, k), rng.uniform(-1, 1, k), np.zeros(k)], axis=1), o_par))
    o_on = targets(rng.uniform(lo + 0.01, r - 0.01, k), rng.uniform(0.02, pm - 0.02, k))                    # starting on the plane
    parts.append(to_world(o_on + np.stack([rng.uniform(-1, 1, k), rng.uniform(-1, 1, k), rng.choice([-1, 1], k) * rng.uniform(.1, 1, k)], axis=1), o_on))
    o = np.concatenate([p[0] for p in parts])
    d = np.concatenate([p[1] for p in parts])
    rays = _rays(o, d)
    # tMax just short of and just beyond the hit of the interior rays (their t is 1 up to rounding: d = target - origin)
    short, beyond = rays[:n].copy(), rays[:n].copy()
    t64 = ds.intersect(ds.Disk(rec, np.float64), rays[:n])["t"]
    short[:, 6], beyond[:, 6] = (t64 * (1 - 1e-4)).astype(np.float32), (t64 * (1 + 1e-4)).astype(np.float32)
    every = np.concatenate([rays, short, beyond])
    # the rays parallel to the plane and those starting on it decide verdicts only: where the transform is not the identity
    # their d.z or height - o.z is rounding noise, and so is the t both restatements would report
    conditioned = np.ones(len(every), bool)
    conditioned[len(rays) - 2 * k:len(rays)] = False
    return every, n, conditioned


def _check(label, name, got, r32, r64, sel):
    b = ds.bar(r32, r64, sel)
    worst = float(np.abs(got[sel].astype(np.float64) - np.asarray(r64)[sel]).max()) if sel.any() else 0.0
    print("%s: %s worst %.3e / bar %.3e over %d" % (label, name, worst, b, int(sel.sum())))
    assert worst <= b, (label, name, worst, b)


@pytest.mark.parametrize("name", list(SHAPES))
def test_probe_against_the_restatement(pt, name):
    rng = np.random.default_rng(11)
    s = pt.Scene(text=_text('AttributeBegin\n%s\nAttributeEnd\nShape "sphere" "float radius" [.25]\n' % SHAPES[name]))
    assert s.errors == [] and s.desc.n_disks == 1 and s.desc.n_spheres == 1
    rec = s.desc.disks[0]
    if name == "rotated, scaled":
        assert rec.swaps_handedness == 1
    d32, d64 = ds.both(rec)
    q = 1                                                     # quadric 0 is the sphere
    rays, n_interior, conditioned = _probe_rays(rec, rng)
    # ---- mode 0
    r32, r64 = ds.intersect(d32, rays), ds.intersect(d64, rays)
    unsure = r32["hit"] != r64["hit"]
    hit = r64["hit"] & ~unsure
    assert unsure.mean() <= 0.01, unsure.mean()                                          # the conditions, on the CPU
    assert 0.2 < hit.mean() < 0.8 and hit[:n_interior].all()
    assert not r64["hit"][-2 * n_interior:-n_interior].any() and r64["hit"][-n_interior:].all()   # tMax short of / beyond the hit
    integ = pt.CreatePathIntegrator(s)
    dev = integ.shape_probe(q, 0, rays)
    assert np.array_equal(dev[~unsure, 0], r64["hit"][~unsure].astype(np.float32)), name   # 1 / 0, never -1: IntersectP agrees
    assert not dev[dev[:, 0] == 0].any()
    for col, key in ((slice(1, 2), "t"), (slice(2, 5), "p"), (slice(5, 8), "n"), (slice(8, 10), "uv"), (slice(10, 13), "dpdu"), (slice(13, 16), "dpdv")):
        a32, a64 = r32[key].reshape(len(rays), -1), r64[key].reshape(len(rays), -1)
        _check(name, key, dev[:, col], a32, a64, hit & conditioned)
    # n against dpdu x dpdv in world space: a transform that swaps handedness mirrors the cross product, and the flip by
    # reverseOrientation ^ swapsHandedness undoes that: what remains is ReverseOrientation alone
    sel = hit & conditioned
    geo = np.cross(r64["dpdu"][sel], r64["dpdv"][sel])
    assert np.all(np.sign((geo * dev[sel, 5:8]).sum(axis=1)) == (-1 if rec.reverse_orientation else 1))
    # the sphere through the same entry point: t against the closed form of a ray towards its centre
    sp = integ.shape_probe(0, 0, _rays([[0, 0, 5], [3, 0, 0]], [[0, 0, -1], [-1, 0, 0]]))
    assert np.all(sp[:, 0] == 1) and np.allclose(sp[:, 1], [4.75, 2.75], atol=1e-5) and np.allclose(sp[0, 5:8], [0, 0, 1], atol=1e-6)
    # ---- mode 1: Sample(ref, u) from generic points, from a point on the disk's plane and from one on its axis
    m = np.array(list(rec.o2w), np.float64).reshape(4, 4)
    h = float(rec.height)
    refs = [("generic", (np.array([.7, -1.1, h + 2.5, 1]) @ m.T)[:3]), ("on the plane", (np.array([4.0, .5, h, 1]) @ m.T)[:3]),
            ("on the axis", (np.array([0, 0, h - 1.75, 1]) @ m.T)[:3])]
    u = rng.random((600, 2)).astype(np.float32)
    identity = np.array_equal(m, np.eye(4))
    for label, ref in refs:
        if label == "on the plane" and not identity:
            # (under a rotation n . wi of an in-plane direction is rounding noise, exactly 0 in one restatement and not in the
            # other for two samples in five: no verdict to hold the device to. In the disk's own frame it is exactly 0, the
            # pdf infinite and Shape::Sample's answer 0 -- the case the reference's isinf test is there for)
            continue
        ref = ref.astype(np.float32)
        p32, n32, pdf32 = ds.sample(d32, ref, u)
        p64, n64, pdf64 = ds.sample(d64, ref, u)
        got = integ.shape_probe(q, 1, np.concatenate([np.tile(ref, (len(u), 1)), u], axis=1))
        us = (pdf32 == 0) != (pdf64 == 0)
        ok = ~us & (pdf64 > 0)
        assert us.mean() <= 0.01
        assert ok.all() if label != "on the plane" else not ok.any()
        assert np.array_equal(got[~us, 6] == 0, (pdf64 == 0)[~us])
        every = np.ones(len(u), bool)
        _check(name + ", ref " + label, "sampled p", got[:, 0:3], p32, p64, every)
        _check(name + ", ref " + label, "sampled n", got[:, 3:6], n32, n64, every)
        if ok.any():
            # (relative: the pdf spans decades as the direction grazes the disk)
            assert np.all(np.abs(got[ok, 6] / pdf64[ok] - 1) <= max(4 * float(np.abs(pdf32[ok] / pdf64[ok] - 1).max()), 8 * 2.0 ** -23))
    # ---- mode 2: Pdf(ref, wi) towards the solid part, the hole and the missing sector
    ref = refs[0][1].astype(np.float32)
    wi = (rays[:, 0:3] + rays[:, 3:6] - ref).astype(np.float32)                 # towards every target of mode 0
    wi = wi[: len(rays) - 2 * n_interior]
    wi = (wi / np.linalg.norm(wi.astype(np.float64), axis=1)[:, None]).astype(np.float32)
    f32, f64 = ds.pdf(d32, ref, wi), ds.pdf(d64, ref, wi)
    us = (f32 == 0) != (f64 == 0)
    assert us.mean() <= 0.01 and 0.2 < (f64 > 0).mean() < 0.9
    got = integ.shape_probe(q, 2, np.concatenate([np.tile(ref, (len(wi), 1)), wi], axis=1))
    assert np.array_equal(got[~us] == 0, (f64 == 0)[~us])
    ok = ~us & (f64 > 0)
    rel = np.abs(got[ok] / f64[ok] - 1)
    bar = max(4 * float(np.abs(f32[ok] / f64[ok] - 1).max()), 8 * 2.0 ** -23)
    print("%s: Pdf worst relative %.3e / bar %.3e over %d, %d zeros" % (name, rel.max(), bar, int(ok.sum()), int((got == 0).sum())))
    assert rel.max() <= bar


# ---------------------------------------------------------------------------------------------------------------------
# 2: traversal
TRIS = ('Material "matte" "rgb Kd" [.5 .5 .5]\n'
        'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-6 0 -6  6 0 -6  6 0 6  -6 0 6]\n'
        'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-6 0 -4  6 0 -4  6 6 -4  -6 6 -4]\n'
        'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-2 .5 1  -1 2.5 1.5  -3 2 .5]\n')
LIGHT = 'LightSource "point" "point from" [0 8 4] "rgb I" [30 30 30]\n'


def _disk_line(xform, params=""):
    return 'AttributeBegin\n%s\nShape "disk" %s\nAttributeEnd\n' % (xform, params)


TRAVERSAL = {
    "disks among triangles": LIGHT + TRIS + _disk_line("Translate 1 1.5 1\nRotate 20 0 1 0", '"float radius" [1.2] "float innerradius" [.4]') +
                             _disk_line("Translate -1.5 1 2.5\nRotate -70 1 0 0", '"float radius" [1] "float phimax" [250]') +
                             _disk_line("Translate 0 3.5 -1\nRotate 30 1 1 0\nScale 1 -1.5 1", '"float radius" [.9] "float height" [.3]'),
    # more quadrics on one ray than the list of postponed ones holds: k_resolve_overflow runs
    "six coaxial disks": LIGHT + TRIS + "".join(_disk_line("Translate 0 1.5 %g" % z, '"float radius" [%g]' % (1.6 - .2 * k))
                                               for k, z in enumerate((-3, -2, -1, 0, 1, 2))),
    # a disk in the plane of a quad: the two tests give the same t up to their rounding, the order of encounter decides
    "coplanar with a quad": LIGHT + TRIS + 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1.5 .5 1  1.5 .5 1  1.5 3 1  -1.5 3 1]\n' +
                            _disk_line("Translate 0 1.75 1", '"float radius" [2]'),
    "a disk in an instanced object": LIGHT + TRIS + 'ObjectBegin "lamp"\nShape "trianglemesh" "integer indices" [0 1 2] "point P" [-.5 0 0  .5 0 0  0 .8 -.2]\n'
                                     'Shape "disk" "float radius" [.7] "float innerradius" [.2] "float height" [.1]\nObjectEnd\n'
                                     'AttributeBegin\nTranslate 1.5 1.5 1\nRotate 25 0 1 0\nScale 1.5 1 1\nObjectInstance "lamp"\nAttributeEnd\n'
                                     'AttributeBegin\nTranslate -1.5 2 2\nRotate -40 1 0 0\nObjectInstance "lamp"\nAttributeEnd\n',
    "a disk and a sphere": LIGHT + TRIS + 'AttributeBegin\nTranslate -1 1.5 1\nShape "sphere" "float radius" [.8]\nAttributeEnd\n' +
                           _disk_line("Translate 1 1.5 1.5\nRotate 15 0 1 0", '"float radius" [1]') +
                           _disk_line("Translate -1 1.5 2.5", '"float radius" [.5]'),
}


def _camera_rays(ob, twin):
    with ob.exact_libm():
        return ob.camera_rays(twin, _all_samples(twin))


def _restated_closest(s, rays):
    """(t64, index64, unsure) of the closest disk per ray: the world's disks directly, an object's through each instance."""
    d = s.desc
    out = []
    for f in (np.float32, np.float64):
        disks = [ds.Disk(d.disks[k], f) for k in range(d.n_disks)]
        if d.n_instances == 0:
            out.append(ds.closest(disks, rays))
        else:   # (the one scene with instances holds its only disk in the object)
            per = [ds.closest(disks, rays, list(d.instances[k].w2i)) for k in range(d.n_instances)]
            t = np.minimum.reduce([p[0] for p in per])
            idx = np.where(np.isinf(t), -1, 0)
            out.append((t, idx, np.concatenate([p[2] for p in per])))
    (t32, i32, v32), (t64, i64, v64) = out
    return t32, t64, i64, (v32 != v64).any(axis=0)


@pytest.mark.parametrize("name", list(TRAVERSAL))
def test_traversal(pt, ob, name, monkeypatch):
    s, twin = _pair(pt, TRAVERSAL[name])
    d = s.desc
    rays = _camera_rays(ob, twin)
    with ob.exact_libm():
        th, _ = ob.trace(twin, rays)
    t_prim, t_t = th[:, 0].copy().view(np.int32), th[:, 1].astype(np.float64)
    t_t = np.where(t_prim >= 0, t_t, np.inf)
    twin_shape = np.array([twin.desc.prims[i].shape for i in range(twin.desc.n_prims)] + [0], np.int64)
    shape = np.array([d.prims[i].shape for i in range(d.n_prims)] + [0], np.int64)
    t32, t64, i64, unsure = _restated_closest(s, rays)
    tie = np.isfinite(t64) & np.isfinite(t_t) & (np.abs(t64 - t_t) <= 1e-4 * np.maximum(1.0, t_t))
    decided = ~unsure & ~tie
    disk_wins = decided & (t64 < t_t)
    other_wins = decided & (t_t < t64)
    nothing = decided & np.isinf(t64) & np.isinf(t_t)
    assert unsure.mean() <= 0.01 and disk_wins.mean() > 0.03 and other_wins.mean() > 0.2        # the conditions, on the CPU
    if name == "coplanar with a quad":
        assert tie.mean() > 0.02
    # ---- A: k_trace against the closest of (restated disks, the oracle's hit in the twin)
    integ = pt.CreatePathIntegrator(s)
    hits = integ.trace(rays)
    prim, t = hits[:, 0].copy().view(np.int32), hits[:, 1]
    q = ~shape[prim]                                                        # quadric index where the hit is a quadric
    assert np.all(prim[nothing] < 0)
    assert np.all(prim[disk_wins] >= 0) and np.all(shape[prim[disk_wins]] < 0) and np.all(q[disk_wins] >= d.n_spheres)
    if d.n_instances == 0:
        assert np.array_equal(q[disk_wins] - d.n_spheres, i64[disk_wins])
    _check(name, "t of disk hits", t, t32, t64, disk_wins)
    assert np.all(prim[other_wins] >= 0) and np.array_equal(shape[prim[other_wins]], twin_shape[t_prim[other_wins]])
    assert np.array_equal(t[other_wins].view(np.uint32), th[other_wins, 1].view(np.uint32))
    any_hit = integ.trace(rays, any_hit=True)[:, 0].view(np.int32) >= 0
    assert np.array_equal(any_hit[decided], (prim >= 0)[decided])
    # ---- B: the render's own kernels (k_trav<0|1|2>, the resolve steps, k_resolve_overflow) equal k_trace bit for bit on
    # every ray, ties, unsure ones and overflowing lists included
    got, extra = tc.check_wavefront(integ, rays, *tc.device_answers(integ), prim_only=True)
    if name == "six coaxial disks":
        assert ((extra[:, 2] & 0x100) != 0).sum() > 50, "no ray's list of postponed quadrics overflowed"
    if name == "a disk in an instanced object":
        assert (extra[disk_wins, 1] >= 0).all()                                  # reached through an instance
    # ---- C: the other tree shapes find the same hits
    monkeypatch.setenv("MIPT_BVH_WIDTH", "2")
    if d.n_instances:   # (object instances are traversed over the two-level records only: the product refuses, disks or not)
        with pytest.raises(RuntimeError, match="MIPT_BVH_WIDTH"):
            pt.CreatePathIntegrator(s)
        narrow = hits
    else:
        narrow = pt.CreatePathIntegrator(s).trace(rays)
    monkeypatch.delenv("MIPT_BVH_WIDTH")
    h, _ = _pair(pt, TRAVERSAL[name], accel='Accelerator "bvh" "string splitmethod" "hlbvh"\n')
    hl = pt.CreatePathIntegrator(h).trace(rays)
    hl_shape = np.array([h.desc.prims[i].shape for i in range(h.desc.n_prims)] + [0], np.int64)
    for label, other, oshape in (("BVH2", narrow, shape), ("hlbvh", hl, hl_shape)):
        op = other[:, 0].copy().view(np.int32)
        assert np.array_equal(op >= 0, prim >= 0), label
        same = (~tie) & (prim >= 0)
        assert np.array_equal(oshape[op[same]], shape[prim[same]]), label
        assert np.array_equal(other[same, 1].view(np.uint32), t[same].view(np.uint32)), label


# ---------------------------------------------------------------------------------------------------------------------
# helpers of the film tests: the sample positions of the twin, splatted with the box filter (film.h:131-141)
def _film_positions(ob, twin, samples):
    with ob.exact_libm():
        u = np.array([[ob.lib().oracle_sample_dimension(twin.desc_ptr, px, py, n, k) for k in (0, 1)] for px, py, n in samples], np.float32)
    xy = np.array([(px, py) for px, py, _ in samples], np.float32)
    return xy + u


def _splat(scene, p_film, values):
    d = scene.desc
    w, h = scene.film_size
    cb, r = list(d.film.cropped_bounds), np.array(list(d.film.filter_radius), np.float32)
    assert all(v == 1.0 for v in d.film.filter_table), "box filter: every weight is 1"
    film, wsum = np.zeros((h, w, values.shape[1])), np.zeros((h, w), np.float32)
    for i, pf in enumerate(p_film):
        dx, dy = pf[0] - np.float32(0.5), pf[1] - np.float32(0.5)
        x0, x1 = max(int(np.ceil(dx - r[0])), cb[0]) - cb[0], min(int(np.floor(dx + r[0])) + 1, cb[2]) - cb[0]
        y0, y1 = max(int(np.ceil(dy - r[1])), cb[1]) - cb[1], min(int(np.floor(dy + r[1])) + 1, cb[3]) - cb[1]
        film[y0:y1, x0:x1] += values[i]
        wsum[y0:y1, x0:x1] += np.float32(1)
    return film, wsum


# ---------------------------------------------------------------------------------------------------------------------
# 3: maps
def test_metadata_maps_of_a_disk_scene(pt, ob):
    """Depth, coordinates, mesh and material of the camera rays of "disks among triangles": per ray the restated disk hit or
    the oracle's hit in the twin, whichever is closer; pixels that a tie or an unsure ray reaches are left out. Depth and
    coordinates within the summed bars of the samples of a pixel, ids exactly."""
    body = TRAVERSAL["disks among triangles"].replace('Shape "disk" "float radius" [1.2]', 'Material "plastic" "rgb Kd" [.2 .3 .7]\nShape "disk" "float radius" [1.2]')
    s, twin = _pair(pt, body, spp=1, integrator='Integrator "metadata" "string strategy" "depth"')
    d = s.desc
    samples = _all_samples(twin)
    rays = _camera_rays(ob, twin)
    import metadata_scenes as ms
    with ob.exact_libm():
        th, _ = ob.trace(twin, rays)
        t_prim = th[:, 0].copy().view(np.int32)
        t_p = ms.hit_points(ob, twin, rays)
    t_t = np.where(t_prim >= 0, th[:, 1].astype(np.float64), np.inf)
    t32, t64, i64, unsure = _restated_closest(s, rays)
    left_out = unsure | (np.isfinite(t64) & np.isfinite(t_t) & (np.abs(t64 - t_t) <= 1e-4 * np.maximum(1.0, t_t)))
    on_disk = (t64 < t_t) & ~left_out
    on_other = (t_t < t64) & ~left_out
    assert left_out.mean() <= 0.01 and on_disk.mean() > 0.03 and on_other.mean() > 0.2
    # the ids of the disks' primitives and of the twin's
    disk_prim = {~d.prims[i].shape - d.n_spheres: i for i in range(d.n_prims) if d.prims[i].shape < 0}
    vals = {k: np.zeros((len(rays), 3)) for k in ("depth", "coordinates", "mesh", "material")}
    bound = {k: np.zeros(len(rays)) for k in ("depth", "coordinates")}
    for k in range(d.n_disks):
        mine = on_disk & (i64 == k)
        r32, r64 = ds.intersect(ds.Disk(d.disks[k], np.float32), rays), ds.intersect(ds.Disk(d.disks[k], np.float64), rays)
        to32, to64 = r32["p"] - rays[:, :3], r64["p"] - rays[:, :3].astype(np.float64)
        dep32, dep64 = np.sqrt((to32 * to32).sum(axis=1, dtype=np.float32)), np.sqrt((to64 * to64).sum(axis=1))
        vals["depth"][mine] = dep64[mine, None]
        vals["coordinates"][mine] = r64["p"][mine]
        if mine.any():
            bound["depth"][mine] = ds.bar(dep32, dep64, mine)
            bound["coordinates"][mine] = ds.bar(r32["p"], r64["p"], mine)
        vals["material"][mine] = d.prim_meta[disk_prim[k]].material_id
        vals["mesh"][mine] = d.prim_meta[disk_prim[k]].instance_id
    o = np.nonzero(on_other)[0]
    to = t_p[o] - rays[o, :3]
    vals["depth"][o] = np.sqrt(to[:, 0] * to[:, 0] + to[:, 1] * to[:, 1] + to[:, 2] * to[:, 2], dtype=np.float32)[:, None]
    vals["coordinates"][o] = t_p[o]
    prim_of_shape = {d.prims[i].shape: i for i in range(d.n_prims)}                 # the same triangle in the disk scene
    mine = [prim_of_shape[twin.desc.prims[p].shape] for p in t_prim[o]]
    vals["material"][o] = np.array([d.prim_meta[p].material_id for p in mine])[:, None]
    vals["mesh"][o] = np.array([d.prim_meta[p].instance_id for p in mine])[:, None]
    bound["depth"][o] = 8 * np.spacing(np.float32(np.abs(vals["depth"][o]).max()))
    bound["coordinates"][o] = 8 * np.spacing(np.float32(np.abs(vals["coordinates"][o]).max()))
    assert len({d.prim_meta[i].material_id for i in disk_prim.values()}) > 1        # the disks do not share one material id
    p_film = _film_positions(ob, twin, samples)
    keep = _splat(s, p_film, left_out[:, None].astype(np.float64))[0][..., 0] == 0
    integ = pt.MetadataIntegrator(s)
    for strategy in ("depth", "coordinates", "mesh", "material"):
        want, wsum = _splat(s, p_film, vals[strategy])
        film, weight = integ.Render(strategy=strategy)
        c = integ.counters.as_dict()
        assert np.array_equal(weight, wsum) and c["camera_rays"] == len(samples) and c["bad_samples"] == 0
        n = 3 if strategy == "coordinates" else 1
        assert want[keep].any() or strategy == "mesh"      # (no instances here: every mesh id is 0)
        if strategy in ("mesh", "material"):
            assert np.array_equal(film[keep][:, 0], want[keep][:, 0].astype(np.float32)), strategy
        else:
            b = _splat(s, p_film, bound[strategy][:, None])[0]
            diff = np.abs(film[..., :n].astype(np.float64) - want[..., :n])
            print("%s: worst difference %.3e, worst bound %.3e" % (strategy, diff[keep].max(), b[keep].max()))
            assert np.all((diff <= b)[keep]), strategy


# ---------------------------------------------------------------------------------------------------------------------
# 4: emitter film
EMITTER = ('AttributeBegin\nAreaLightSource "diffuse" "rgb L" [3 2 1] %s\nTranslate .3 1.2 0\nRotate %g 0 1 0\n'
           'Shape "disk" "float radius" [2] "float innerradius" [.5] "float phimax" [300]\nAttributeEnd\n'
           'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [50 50 -60  51 50 -60  50 51 -60]\n')


@pytest.mark.parametrize("view", ["one-sided from the front", "one-sided from behind", "two-sided from behind"])   # front: the side an intersection's n points to
def test_emitter_film(pt, ob, view):
    """maxdepth 1, the emitter alone: the film is the sum of filter weight * Le over the samples whose restated ray hits the
    emitting side. An intersection's n is Cross(dpdu, dpdv) as disk.cpp:78-80 writes them, which is -z in object space: the
    camera, on the +z side, sees the front of a disk turned by 180 degrees about y and the back of one turned by 10."""
    two = '"bool twosided" "true"' if view.startswith("two") else ""
    s, twin = _pair(pt, EMITTER % (two, 10 if "behind" in view else 180), integrator='Integrator "path" "integer maxdepth" [1]')
    d = s.desc
    samples = _all_samples(twin)
    rays = _camera_rays(ob, twin)
    r32, r64 = ds.intersect(ds.Disk(d.disks[0], np.float32), rays), ds.intersect(ds.Disk(d.disks[0], np.float64), rays)
    unsure = r32["hit"] != r64["hit"]
    facing = (r64["n"] * -rays[:, 3:6].astype(np.float64)).sum(axis=1) > 0
    emits = r64["hit"] & (facing | (d.lights[0].two_sided != 0))
    assert unsure.sum() == 0 and 0.1 < r64["hit"].mean() < 0.9                                   # the premises, on the CPU
    assert emits.any() == (view != "one-sided from behind")
    le = np.array(list(d.lights[0].L), np.float64)
    p_film = _film_positions(ob, twin, samples)
    want, wsum = _splat(s, p_film, emits[:, None] * le[None, :])
    integ = pt.CreatePathIntegrator(s)
    film, weight = integ.Render()
    c = integ.counters.as_dict()
    assert np.array_equal(weight, wsum) and c["camera_rays"] == len(samples) and c["bad_samples"] == 0
    if emits.any():
        rel = _rel_l2(film, want)
        print("%s: relative L2 %.3e, %d of %d samples see the emitter" % (view, rel, int(emits.sum()), len(samples)))
        assert rel < 1e-6, rel
    else:
        # nothing but the emitter's own matte surface under light samples in its own plane: both cosines are rounding noise.
        # Held to the front view's bar: 1e-6 of what a pixel of the lit film holds (spp samples of Le)
        print("%s: largest film value %.3e" % (view, float(np.abs(film).max())))
        assert float(np.abs(film).max()) <= 1e-6 * float(le.max()) * s.spp


# ---------------------------------------------------------------------------------------------------------------------
# 5: solid-angle pins
def _radical_pairs(n):
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


def _uniform_sphere(u):
    """UniformSampleSphere, sampling.cpp:98-103."""
    z = 1 - 2 * u[:, 0]
    r = np.sqrt(np.maximum(0, 1 - z * z))
    phi = 2 * math.pi * u[:, 1]
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(np.float32)


def test_solid_angle_pins(pt):
    """Disk.SolidAngle (src/tests/shapes.cpp:361-370) with the reference's transform, radius, point and sample count, in the
    form tests/test_shape_pins.py gives Sphere.SolidAngle: mcSolidAngle -- the hit fraction of uniform directions, traced on
    the device, times 4 pi -- against Shape::SolidAngle -- the mean of 1 / pdf over Sample(ref, u) (shape_probe mode 1) of the
    samples whose point is visible -- to 0.001; from the reference's point, a second off-axis one and one on the axis, where
    both equal 2 pi (1 - h / sqrt(h^2 + R^2)) to 0.01. And every sampled direction meets the disk again: Pdf(ref, wi) > 0."""
    R = 1.25
    s = pt.Scene(text=_text('AttributeBegin\nTranslate 1 .5 -.8\nRotate 30 1 0 0\nShape "disk" "float radius" [%g]\nAttributeEnd\n' % R))
    assert s.errors == [] and s.desc.n_disks == 1
    integ = pt.CreatePathIntegrator(s)
    n = 128 * 1024
    u = _radical_pairs(n)
    dirs = _uniform_sphere(u)
    m = np.array(list(s.desc.disks[0].o2w), np.float64).reshape(4, 4)
    hgt = 1.5
    axis = (np.array([0, 0, hgt, 1]) @ m.T)[:3]
    for label, p in (("the reference's point", (.5, -.8, .5)), ("a second point", (2.5, 1.5, 1.0)), ("on the axis", axis)):
        p = np.asarray(p, np.float32)
        occluded = integ.trace(_rays(np.tile(p, (n, 1)), dirs), any_hit=True)[:, 0].view(np.int32) >= 0
        mc = occluded.sum() * 4 * math.pi / n
        sm = integ.shape_probe(0, 1, np.concatenate([np.tile(p, (n, 1)), u], axis=1))
        to = sm[:, 0:3] - p
        blocked = integ.trace(_rays(np.tile(p, (n, 1)), to, 0.999), any_hit=True)[:, 0].view(np.int32) >= 0
        ok = (sm[:, 6] > 0) & ~blocked
        sa = float((1.0 / sm[ok, 6].astype(np.float64)).sum() / n)
        print("%s: uniform directions %.5f, Sample(ref, u) %.5f" % (label, mc, sa))
        assert ok.all()
        assert abs(mc - sa) < .001, (label, mc, sa)
        if label == "on the axis":
            closed = 2 * math.pi * (1 - hgt / math.sqrt(hgt * hgt + R * R))
            assert abs(mc - closed) < .01 and abs(sa - closed) < .01, (mc, sa, closed)
        # Reintersect: the direction of every sample meets the disk, at the sampled point's pdf
        wi = (to / np.linalg.norm(to.astype(np.float64), axis=1)[:, None]).astype(np.float32)
        sub = slice(0, n, 16)
        back = integ.shape_probe(0, 2, np.concatenate([np.tile(p, (len(wi[sub]), 1)), wi[sub]], axis=1))
        assert np.all(back > 0), (label, int((back == 0).sum()))
        assert np.allclose(back, sm[sub, 6], rtol=1e-3)


# ---------------------------------------------------------------------------------------------------------------------
# 6: a lamp over a floor
LAMP_R, LAMP_H = 1.5, 2.0
LAMP_HEAD = ('LookAt 3 1.5 0  0 0 0  0 1 0\nCamera "perspective" "float fov" [0.1]\n'
             'Film "image" "integer xresolution" [4] "integer yresolution" [4]\n'
             'Sampler "halton" "integer pixelsamples" [%(spp)d]\n'
             'Integrator "path" "integer maxdepth" [%(depth)d] "string lightsamplestrategy" "%(strategy)s"\nWorldBegin\n')
FLOOR = ('Material "matte" "rgb Kd" [.5 .5 .5]\n'
         'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-20 0 -20  20 0 -20  20 0 20  -20 0 20]\n')
# The reference's disk has two normals: Disk::Sample gives the sampled point ObjectToWorld(0, 0, 1) (disk.cpp:133), while an
# intersection's n is Cross(dpdu, dpdv) with dpdv pointing outwards (disk.cpp:78-80), which is -z; DiffuseAreaLight::L tests
# whichever it is handed. Under a transform that swaps handedness the interaction's normal is flipped (interaction.cpp:60-65)
# and the sampled one is not: then both are +z. The lamp is such a disk -- mirrored in x, which a disk does not notice -- so
# that "facing down" means the same to the light samples and to the BSDF samples that reach it.
DISK_LAMP = ('AttributeBegin\nAreaLightSource "diffuse" "rgb L" [%(le)s]\nTranslate 0 %(h)g 0\nRotate 90 1 0 0\nScale -1 1 1\n'
             'Shape "disk" "float radius" [%(r)g]\nAttributeEnd\n')


def _fan_lamp(le_scale):
    """The oracle's stand-in: a 64-gon fan in the lamp's plane, facing down, Le scaled by the ratio of the areas."""
    k = 64
    ang = 2 * math.pi * np.arange(k) / k
    pts = ["0 %r 0" % LAMP_H] + ["%r %r %r" % (LAMP_R * math.cos(a), LAMP_H, LAMP_R * math.sin(a)) for a in ang]
    idx = " ".join("0 %d %d" % (1 + i, 1 + (i + 1) % k) for i in range(k))      # (0, p_i, p_i+1): the normal is -y
    return ('AttributeBegin\nAreaLightSource "diffuse" "rgb L" [%r %r %r]\nShape "trianglemesh" "integer indices" [%s] "point P" [%s]\nAttributeEnd\n'
            % (4 * le_scale, 4 * le_scale, 4 * le_scale, idx, " ".join(pts)))


def _lamp_expected(scene):
    d = scene.desc
    mat = d.materials[[d.prims[i].material for i in range(d.n_prims) if d.prims[i].shape == 0][0]]    # the floor's (triangle 0)
    assert mat.n_bxdfs == 1
    kd = np.array(list(mat.bxdf[0].R), np.float64)
    return kd * LAMP_R ** 2 / (LAMP_H ** 2 + LAMP_R ** 2)        # per unit Le: the on-axis form factor of a disk


def _lamp_spp(pt, ob):
    """The smallest power of two at which the oracle's render of the twin with the fan lamp meets the furnace bar."""
    if "lamp spp" not in _cache:
        scale = 2 * math.pi / (64 * math.sin(2 * math.pi / 64))
        for spp in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096):
            t = pt.Scene(text=LAMP_HEAD % dict(spp=spp, depth=1, strategy="uniform") + FLOOR + _fan_lamp(scale) + "WorldEnd\n")
            assert t.errors == [] and t.desc.n_lights == 64
            film, weight, _, _ = ob.render(t)
            le = np.array(list(t.desc.lights[0].L), np.float64) / scale
            mean = (film.astype(np.float64) / weight[..., None]).mean(axis=(0, 1))
            rel = float(np.abs(mean / (_lamp_expected(t) * le) - 1).max())
            if rel < 0.02:
                _cache["lamp spp"] = spp
                break
        assert "lamp spp" in _cache, "the oracle's fan lamp does not meet 0.02 at 4096 spp"
    return _cache["lamp spp"]


def _lamp_scene(pt, spp, strategy, extra="", depth=1):
    s = pt.Scene(text=LAMP_HEAD % dict(spp=spp, depth=depth, strategy=strategy) + FLOOR + DISK_LAMP % dict(le="4 4 4", h=LAMP_H, r=LAMP_R) + extra + "WorldEnd\n")
    assert s.errors == [] and s.desc.n_disks == 1 and s.desc.n_lights == 1
    return s


@pytest.mark.parametrize("strategy", ["uniform", "power", "spatial"])
def test_lamp_over_a_floor(pt, ob, strategy):
    """A one-sided disk light of radius R facing down at height h over a matte floor, direct lighting only, seen through a
    0.1 degree field of view on the axis point: radiance Kd Le R^2 / (h^2 + R^2), to the furnace bar of 0.02."""
    spp = _lamp_spp(pt, ob)
    s = _lamp_scene(pt, spp, strategy)
    film, weight = pt.CreatePathIntegrator(s).Render()
    le = np.array(list(s.desc.lights[0].L), np.float64)
    mean = (film.astype(np.float64) / weight[..., None]).mean(axis=(0, 1))
    rel = float(np.abs(mean / (_lamp_expected(s) * le) - 1).max())
    print("lamp over a floor, %s, %d spp: worst relative error of a bin %.4f" % (strategy, spp, rel))
    assert rel < 0.02, rel


# ---------------------------------------------------------------------------------------------------------------------
# 7: schedules
def test_schedules(pt, ob, monkeypatch):
    """The lamp scene with a mirror and a glass sphere (MIS rays towards the disk light, postponed quadrics on their way):
    a 256-slot pool, two sub-renderers, two passes over sample ranges and two shards equal the plain render -- weights
    exactly, films to 1e-6 relative L2 (the rule of tests/test_render_schedule_gpu.py); so does MIPT_DARK_STREAM=0."""
    extra = ('AttributeBegin\nMaterial "mirror"\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 0.001 -1  -1 0.001 1  -1 2 1  -1 2 -1]\nAttributeEnd\n'
             'AttributeBegin\nMaterial "glass" "float index" [1.5]\nTranslate .4 .3 .3\nShape "sphere" "float radius" [.3]\nAttributeEnd\n')
    head = LAMP_HEAD.replace('[0.1]', '[40]').replace('[4] "integer yresolution" [4]', '[32] "integer yresolution" [32]')
    text = head % dict(spp=4, depth=5, strategy="spatial") + FLOOR + DISK_LAMP % dict(le="4 4 4", h=LAMP_H, r=LAMP_R) + extra + "WorldEnd\n"
    s = pt.Scene(text=text)
    assert s.errors == [] and s.desc.n_disks == 1 and s.desc.n_spheres == 1
    monkeypatch.delenv("MIPT_STREAMS", raising=False)
    monkeypatch.delenv("MIPT_DARK_STREAM", raising=False)
    integ = pt.CreatePathIntegrator(s)
    ref, wref = integ.Render()
    c = integ.counters.as_dict()
    assert ref.any() and c["camera_rays"] == 32 * 32 * 4 and c["shadow_rays"] > 0 and c["bad_samples"] == 0

    def same(film, weight, how):
        rel = _rel_l2(film, ref)
        print("%s: relative L2 %.3e" % (how, rel))
        assert np.array_equal(weight, wref), how
        assert rel < 1e-6, (how, rel)

    film, weight = integ.Render(path_pool=256)
    assert integ.pool_info()[0] == 256
    same(film, weight, "256-slot pool")
    acc, wacc = np.zeros_like(ref), np.zeros_like(wref)
    for r in range(2):
        f, w = integ.Render(shard_index=r, shard_count=2)
        acc += f
        wacc += w
    same(acc, wacc, "two shards")
    integ.Render(spp=2, sample_begin=0, download=False)
    film, weight = integ.Render(spp=2, sample_begin=2, accumulate=True)
    same(film, weight, "two passes")
    monkeypatch.setenv("MIPT_STREAMS", "2")          # (read when the renderer is created)
    two = pt.CreatePathIntegrator(s)
    film, weight = two.Render()
    same(film, weight, "two sub-renderers")
    monkeypatch.delenv("MIPT_STREAMS")
    monkeypatch.setenv("MIPT_DARK_STREAM", "0")
    film, weight = pt.CreatePathIntegrator(s).Render()
    same(film, weight, "MIPT_DARK_STREAM=0")
