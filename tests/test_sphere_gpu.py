"""Shape "sphere" on the GPU, query by query and through the kernels a render runs. sphere_shape.py restates the sphere in
float32 and float64 (test_sphere_restatement.py checks it against closed forms and the oracle where no GPU is needed);
sphere_cases.py holds the six shapes and their ray families. A query whose verdict differs between the two restatements is
"unsure" and decides nothing; each family asserts on the CPU that at most 1 % of its queries are. Bars: four times the worst
float32-vs-float64 deviation of the restatement over the selected queries of ONE family, never below 8 ulp of the largest
component (disk_shape.bar) -- the grazing family's loose bar does not cover for the others."""
import math

import numpy as np
import pytest

import disk_shape as ds
import sphere_cases as sc
import sphere_shape as ss
import trace_check as tc

pytestmark = pytest.mark.gpu

_cache = {}
FIELDS = ((slice(1, 2), "t"), (slice(2, 5), "p"), (slice(5, 8), "n"), (slice(8, 10), "uv"), (slice(10, 13), "dpdu"), (slice(13, 16), "dpdv"))


def _check(label, name, got, r32, r64, sel):
    b = ds.bar(r32, r64, sel)
    worst = float(np.abs(got[sel].astype(np.float64) - np.asarray(r64)[sel]).max()) if sel.any() else 0.0
    print("%s: %s worst %.3e / bar %.3e over %d" % (label, name, worst, b, int(sel.sum())))
    assert worst <= b, (label, name, worst, b)


def _check_rel(label, name, got, f32, f64, sel):
    """The relative bar of test_disk_gpu.py's pdf checks: four times the worst relative float32-vs-float64 deviation, never
    below 8 * 2^-23."""
    if not sel.any():
        return
    rel = float(np.abs(got[sel].astype(np.float64) / f64[sel] - 1).max())
    b = max(4 * float(np.abs(f32[sel].astype(np.float64) / f64[sel] - 1).max()), 8 * 2.0 ** -23)
    print("%s: %s worst relative %.3e / bar %.3e over %d" % (label, name, rel, b, int(sel.sum())))
    assert rel <= b, (label, name, rel, b)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# 1: the probe against the restatement
@pytest.mark.parametrize("name", list(sc.SHAPES))
def test_probe_intersect(pt, name):
    """mi_pt_shape_probe mode 0 on the ray families of sphere_cases.families. The verdict is the restated one wherever the two
    restatements agree and never -1 (SphereHitT -- the pre-test in plain floats and WANT_POINT = false -- and
    SphereInteraction agree on the verdict and on the bits of t); a miss is sixteen zeros; t, p, n, uv, dpdu, dpdv within the
    family's own bar; t bit for bit with the float32 restatement on families 1, 2, 5 and 10; n on the side of dpdu x dpdv
    that ReverseOrientation alone decides."""
    rng = np.random.default_rng(11)
    s, q = sc.scene(pt, name)
    rec = s.desc.spheres[q]
    if name == "rotated, scaled":
        assert rec.swaps_handedness == 1
    s32, s64 = ss.both(rec)
    fams = sc.families(rec, rng)
    rays = np.concatenate([f.rays for f in fams])
    assert 2000 < len(rays) < 8000
    # ---- the conditions, on the CPU
    parts, roots = [], set()
    at = 0
    for f in fams:
        r32, r64 = ss.intersect(s32, f.rays), ss.intersect(s64, f.rays)
        unsure = r32["hit"] != r64["hit"]
        hit = r64["hit"] & ~unsure
        assert unsure.mean() <= 0.01, (name, f.name, unsure.mean())
        if f.expect is not None:
            assert (hit if f.expect else ~r64["hit"]).mean() >= 0.9, (name, f.name, hit.mean())
        if f.root is not None and hit.any():
            assert (r64["root"][hit] == f.root).mean() >= 0.9, (name, f.name)
        roots |= set(np.unique(r64["root"][hit]).tolist())
        parts.append((f, r32, r64, unsure, hit, slice(at, at + len(f.rays))))
        at += len(f.rays)
    assert roots == {0, 1}
    # ---- the device
    integ = pt.CreatePathIntegrator(s)
    dev_all = integ.shape_probe(q, 0, rays)
    assert not (dev_all[:, 0] == -1).any(), "SphereHitT and SphereInteraction disagree on %d rays" % int((dev_all[:, 0] == -1).sum())
    assert not dev_all[dev_all[:, 0] == 0].any()
    for f, r32, r64, unsure, hit, where in parts:
        dev = dev_all[where]
        wrong = np.nonzero((dev[:, 0] != r64["hit"].astype(np.float32)) & ~unsure)[0]
        assert len(wrong) == 0, (name, f.name, len(wrong), f.rays[wrong[0]].tolist())
        label = "%s, %s" % (name, f.name)
        if f.conditioned and hit.any():
            for col, key in FIELDS:
                _check(label, key, dev[:, col], r32[key].reshape(len(dev), -1), r64[key].reshape(len(dev), -1), hit)
            geo = np.cross(r64["dpdu"][hit], r64["dpdv"][hit])
            assert np.all(np.sign((geo * dev[hit, 5:8]).sum(axis=1)) == (-1 if rec.reverse_orientation else 1)), label
        if f.exact_t and hit.any():
            both = hit & r32["hit"]
            differ = int((_bits(dev[both, 1]) != _bits(r32["t"][both])).sum())
            print("%s: t bit for bit with the float32 restatement on %d of %d" % (label, int(both.sum()) - differ, int(both.sum())))
            assert differ == 0, (label, differ)


@pytest.mark.parametrize("name", list(sc.SHAPES))
def test_probe_sample_and_pdf(pt, name):
    """Modes 1 and 2 from five reference points: a generic one outside, one 200 r away (1 - cosThetaMax cancels in float32:
    the bar is vacuous there and pdf is held to the float32 restatement's bits: one sqrt, one subtraction, one division),
    one inside and the centre (both run the area-sampling branch) and one at 1.001 r. Sample(ref, u) over 600 random u and the
    four corners: p, n within the bar, pdf == 0 in the same places, pdf within the relative bar. Pdf(ref, wi) towards the
    targets of mode 0 and back towards the sampled points: from outside it is the sampled pdf bit for bit (the same formula);
    from inside zeros in the same places (directions through the clipped part) and the relative bar."""
    rng = np.random.default_rng(12)
    s, q = sc.scene(pt, name)
    rec = s.desc.spheres[q]
    s32, s64 = ss.both(rec)
    integ = pt.CreatePathIntegrator(s)
    u = sc.sample_points(rng)
    random_u = np.arange(len(u)) < len(u) - 4
    targets = np.concatenate([f.targets[:60] for f in sc.families(rec, rng, n=120) if f.targets is not None])
    for where, ref, is_inside in sc.reference_points(rec):
        label = "%s, ref %s" % (name, where)
        assert ss.inside(s32, ref) == is_inside and ss.inside(s64, ref) == is_inside, label
        p32, n32, pdf32 = ss.sample(s32, ref, u)
        p64, n64, pdf64 = ss.sample(s64, ref, u)
        got = integ.shape_probe(q, 1, np.concatenate([np.tile(ref, (len(u), 1)), u], axis=1))
        us = (pdf32 == 0) != (pdf64 == 0)
        ok = ~us & (pdf64 > 0)
        assert us.mean() <= 0.01 and ok.mean() > 0.9, label
        assert np.array_equal(got[~us, 6] == 0, (pdf64 == 0)[~us]), label
        for part, sel in (("random u", random_u), ("corners", ~random_u)):
            _check(label + ", " + part, "sampled p", got[:, 0:3], p32, p64, sel)
            _check(label + ", " + part, "sampled n", got[:, 3:6], n32, n64, sel)
        _check_rel(label, "sampled pdf", got[:, 6], pdf32, pdf64, ok)
        if where == "far outside":
            assert np.array_equal(_bits(got[:, 6]), _bits(pdf32)), label
        # ---- mode 2
        to = np.concatenate([targets, got[:, 0:3].astype(np.float64)]) - ref.astype(np.float64)
        keep = np.linalg.norm(to, axis=1) > 0
        wi = (to[keep] / np.linalg.norm(to[keep], axis=1)[:, None]).astype(np.float32)
        f32, f64 = ss.pdf(s32, ref, wi), ss.pdf(s64, ref, wi)
        back = integ.shape_probe(q, 2, np.concatenate([np.tile(ref, (len(wi), 1)), wi], axis=1))
        us = (f32 == 0) != (f64 == 0)
        assert us.mean() <= 0.01, (label, us.mean())
        assert np.array_equal(back[~us] == 0, (f64 == 0)[~us]), label
        if not is_inside:
            assert (back > 0).all() and np.all(_bits(back) == _bits(got[0, 6])), label
        else:
            pos = ~us & (f64 > 0)
            assert pos.mean() > 0.2 and (name == "full") == bool((f64 > 0).all()), label
            _check_rel(label, "Pdf", back, f32, f64, pos)
            print("%s: %d zeros of %d" % (label, int((back == 0).sum()), len(back)))


def test_sphere_solid_angle_on_the_device(pt):
    """Sphere.SolidAngle (src/tests/shapes.cpp:331-348) with the device's own Sample: the mean of 1 / pdf over mode 1 with the
    reference's transform, radius, points, sample count and radical-inverse u is 4 pi to 0.01 from the inside point and the
    closed form 2 pi (1 - cos theta_max) to 0.001 from the outside one -- the reference's tolerances."""
    s = pt.Scene(text=sc.text('AttributeBegin\nTranslate 1 .5 -.8\nRotate 30 1 0 0\nShape "sphere" "float radius" [1]\nAttributeEnd\n'))
    assert s.errors == [] and s.desc.n_spheres == 1
    integ = pt.CreatePathIntegrator(s)
    n = 128 * 1024
    u = sc.radical_pairs(n)
    got = {}
    for label, p in (("inside", (1, .9, -.8)), ("outside", (-.25, -1, .8))):
        sm = integ.shape_probe(0, 1, np.concatenate([np.tile(np.asarray(p, np.float32), (n, 1)), u], axis=1))
        assert (sm[:, 6] > 0).mean() > 0.999
        got[label] = float((1.0 / sm[sm[:, 6] > 0, 6].astype(np.float64)).sum() / n)
    d2 = ((np.array([-.25, -1, .8]) - np.array([1, .5, -.8])) ** 2).sum()
    closed = 2 * math.pi * (1 - math.sqrt(1 - 1 / d2))
    print("Sphere.SolidAngle on the device: inside %.5f (4 pi = %.5f), outside %.5f (closed form %.5f)" % (got["inside"], 4 * math.pi, got["outside"], closed))
    assert abs(got["inside"] - 4 * math.pi) < .01 and abs(got["outside"] - closed) < .001


# ---------------------------------------------------------------------------------------------------------------------
# 2: the kernels a render runs
TRIS = ('Material "matte" "rgb Kd" [.5 .5 .5]\n'
        'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-6 0 -6  6 0 -6  6 0 6  -6 0 6]\n'
        'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-6 0 -4  6 0 -4  6 6 -4  -6 6 -4]\n'
        'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-2 .5 1  -1 2.5 1.5  -3 2 .5]\n')
LIGHT = 'LightSource "point" "point from" [0 8 4] "rgb I" [30 30 30]\n'


def _sphere_line(xform, params):
    return 'AttributeBegin\n%s\nShape "sphere" %s\nAttributeEnd\n' % (xform, params)


TRAVERSAL = {
    "partial spheres among triangles": LIGHT + TRIS + _sphere_line("Translate 1 1.5 1\nRotate 20 0 1 0", '"float radius" [1.2] "float zmin" [-.5] "float zmax" [.8]') +
                                       _sphere_line("Translate -1.5 1 2.5\nRotate -70 1 0 0", '"float radius" [1] "float phimax" [250]') +
                                       _sphere_line("Translate 0 3.5 -1\nRotate 30 1 1 0\nScale 1 -1.5 1", '"float radius" [.9] "float zmin" [-.3] "float phimax" [300]'),
    # more quadrics on one ray than the list of postponed ones holds: k_resolve_overflow runs
    "six concentric spheres": LIGHT + TRIS + "".join(_sphere_line("Translate 0 1.6 1\nRotate %g 0 1 0\nRotate -90 1 0 0" % (25 * k),
                                                                  '"float radius" [%g] %s' % (1.6 - .2 * k, '"float phimax" [250]' if k % 2 == 0 else '"float zmax" [%g]' % (.5 * (1.6 - .2 * k))))
                                                     for k in range(6)),
    # a sphere of radius 50 around the camera that touches the back wall from the front: near the point of contact the sphere
    # and the quad give the same t up to their rounding, the order of encounter decides; every camera ray starts inside it
    "a sphere tangent to a quad": LIGHT + TRIS + _sphere_line("Translate 0 3 46", '"float radius" [50]'),
    "a sphere in an instanced object": LIGHT + TRIS + 'ObjectBegin "lamp"\nShape "trianglemesh" "integer indices" [0 1 2] "point P" [-.5 0 0  .5 0 0  0 .8 -.2]\n'
                                       'Shape "sphere" "float radius" [.7] "float zmin" [-.4] "float phimax" [280]\nObjectEnd\n'
                                       'AttributeBegin\nTranslate 1.5 1.5 1\nRotate 25 0 1 0\nScale 1.5 1 .7\nObjectInstance "lamp"\nAttributeEnd\n'
                                       'AttributeBegin\nTranslate -1.5 2 2\nRotate -40 1 0 0\nObjectInstance "lamp"\nAttributeEnd\n',
}


def _twin_text(text):
    """The same scene without its spheres (every sphere is written on a line of its own)."""
    lines = text.split("\n")
    assert any('Shape "sphere"' in l for l in lines)
    return "\n".join(l for l in lines if 'Shape "sphere"' not in l)


def _pair(pt, body, **kw):
    text = sc.text(body, **kw)
    s, twin = pt.Scene(text=text), pt.Scene(text=_twin_text(text))
    assert s.errors == [] and twin.errors == [] and s.desc.n_spheres > 0 and twin.desc.n_spheres == 0
    assert twin.desc.n_tris == s.desc.n_tris and s.desc.n_disks == 0
    return s, twin


def _all_samples(scene):
    sb = list(scene.desc.film.sample_bounds)
    return [(px, py, n) for py in range(sb[1], sb[3]) for px in range(sb[0], sb[2]) for n in range(scene.spp)]


def _centre(s, k=0):
    """The world-space centre of sphere k: through the first instance where the sphere belongs to an object."""
    d = s.desc
    c = np.array(list(d.spheres[k].o2w), np.float64).reshape(4, 4)[:, 3]
    if d.n_instances:
        c = np.linalg.inv(np.array(list(d.instances[0].w2i), np.float64).reshape(4, 4)) @ c
    return c[:3]


def _restated_closest(s, rays):
    """(t32, t64, index64, unsure) of the closest sphere per ray: the world's spheres directly, an object's through each instance."""
    d = s.desc
    out = []
    for f in (np.float32, np.float64):
        spheres = [ss.Sphere(d.spheres[k], f) for k in range(d.n_spheres)]
        if d.n_instances == 0:
            out.append(ss.closest(spheres, rays))
        else:   # (the one scene with instances holds its only sphere in the object)
            per = [ss.closest(spheres, rays, list(d.instances[k].w2i)) for k in range(d.n_instances)]
            t = np.minimum.reduce([p[0] for p in per])
            out.append((t, np.where(np.isinf(t), -1, 0), np.concatenate([p[2] for p in per])))
    (t32, i32, v32), (t64, i64, v64) = out
    return t32, t64, i64, (v32 != v64).any(axis=0)


@pytest.mark.parametrize("name", list(TRAVERSAL))
def test_traversal(pt, ob, name, monkeypatch):
    """The twin's camera rays and 600 rays from the centre of the first sphere. A: mi_pt_trace picks the closer of (restated
    spheres, the oracle's hit in the twin) -- t within the bar where a sphere wins, the oracle's bits where a triangle wins,
    the any-hit form agreeing. B: k_trav<0|1|2> and the resolve steps equal k_trace bit for bit. C: BVH2 and hlbvh find the
    same hits (the instanced scene: the documented BVH2 refusal)."""
    s, twin = _pair(pt, TRAVERSAL[name])
    d = s.desc
    rng = np.random.default_rng(31)
    with ob.exact_libm():
        cam = ob.camera_rays(twin, _all_samples(twin))
    w = rng.normal(size=(600, 3))
    rays = np.concatenate([cam, sc.rays_of(np.tile(_centre(s), (600, 1)), w)])
    from_inside = np.arange(len(rays)) >= len(cam)
    with ob.exact_libm():
        th, _ = ob.trace(twin, rays)
    t_prim, t_t = th[:, 0].copy().view(np.int32), th[:, 1].astype(np.float64)
    t_t = np.where(t_prim >= 0, t_t, np.inf)
    twin_shape = np.array([twin.desc.prims[i].shape for i in range(twin.desc.n_prims)] + [0], np.int64)
    shape = np.array([d.prims[i].shape for i in range(d.n_prims)] + [0], np.int64)
    t32, t64, i64, unsure = _restated_closest(s, rays)
    with np.errstate(invalid="ignore"):
        tie = np.isfinite(t64) & np.isfinite(t_t) & (np.abs(t64 - t_t) <= 1e-4 * np.maximum(1.0, t_t))
    decided = ~unsure & ~tie
    sphere_wins = decided & (t64 < t_t)
    other_wins = decided & (t_t < t64)
    nothing = decided & np.isinf(t64) & np.isinf(t_t)
    print("%s: %d rays, %d unsure, %d ties, a sphere wins %d (%d from inside), a triangle %d" %
          (name, len(rays), int(unsure.sum()), int(tie.sum()), int(sphere_wins.sum()), int((sphere_wins & from_inside).sum()), int(other_wins.sum())))
    assert unsure.mean() <= 0.01 and sphere_wins.mean() > 0.03 and other_wins.mean() > 0.2        # the conditions, on the CPU
    assert (sphere_wins & from_inside).sum() > 100
    if name == "a sphere tangent to a quad":
        assert tie.sum() >= 8
    # ---- A
    integ = pt.CreatePathIntegrator(s)
    hits = integ.trace(rays)
    prim, t = hits[:, 0].copy().view(np.int32), hits[:, 1]
    q = ~shape[prim]                                                        # quadric index where the hit is a quadric
    assert np.all(prim[nothing] < 0)
    assert np.all(prim[sphere_wins] >= 0) and np.all(shape[prim[sphere_wins]] < 0) and np.all(q[sphere_wins] < d.n_spheres)
    if d.n_instances == 0:
        assert np.array_equal(q[sphere_wins], i64[sphere_wins])
    _check(name, "t of sphere hits", t, t32, t64, sphere_wins)
    assert np.all(prim[other_wins] >= 0) and np.array_equal(shape[prim[other_wins]], twin_shape[t_prim[other_wins]])
    assert np.array_equal(t[other_wins].view(np.uint32), th[other_wins, 1].view(np.uint32))
    any_hit = integ.trace(rays, any_hit=True)[:, 0].view(np.int32) >= 0
    assert np.array_equal(any_hit[decided], (prim >= 0)[decided])
    # ---- B
    got, extra = tc.check_wavefront(integ, rays, *tc.device_answers(integ), prim_only=True)
    if name == "six concentric spheres":
        assert ((extra[:, 2].view(np.int32) & 0x100) != 0).sum() > 50, "no ray's list of postponed quadrics overflowed"
    if d.n_instances:
        assert (extra[sphere_wins, 1].view(np.int32) >= 0).all()                 # reached through an instance
    # ---- C
    monkeypatch.setenv("MIPT_BVH_WIDTH", "2")
    if d.n_instances:   # (object instances are traversed over the two-level records only: the product refuses)
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
# 3: MIS rays towards a sphere emitter
EMITTER = ('AttributeBegin\nAreaLightSource "diffuse" "rgb L" [3 2 1]\nTranslate -2 1.7 -1\nShape "sphere" "float radius" [.8]\nAttributeEnd\n')


def test_visibility_spans_around_a_sphere_emitter(pt, ob):
    """mi_pt_trace_wavefront mode 3 (k_trav<3>, the visibility query of a BSDF-sampled MIS ray) on rays towards a sphere
    emitter behind the small triangle of TRIS, the end of the span at the restated t of the sphere (the root inside the span),
    at twice that and at 0.9 of it. The kernel postpones the sphere, so what it answers is decided by the triangles alone,
    which the oracle knows from the twin: a triangle well in front of the span is reported (some primitive >= 0 that is a
    triangle), no triangle up to the end of the span is -1, and nothing else than -1, -2 or a triangle is ever answered."""
    s, twin = _pair(pt, TRIS + EMITTER)
    d = s.desc
    assert d.n_lights == 1 and d.lights[0].shape == ~0
    rng = np.random.default_rng(41)
    n = 2000
    s32, s64 = ss.both(d.spheres[0])
    o = np.stack([rng.uniform(-4, 3, n), rng.uniform(.2, 5, n), rng.uniform(2, 8, n)], axis=1)
    c = _centre(s)
    aim = c + 0.75 * 0.8 * rng.uniform(-1, 1, (n, 3)) / math.sqrt(3)
    dirs = aim - o
    rays = sc.rays_of(o, dirs / np.linalg.norm(dirs, axis=1)[:, None])
    r32, r64 = ss.intersect(s32, rays), ss.intersect(s64, rays)
    assert r32["hit"].all() and r64["hit"].all() and (r64["root"] == 0).all()
    with ob.exact_libm():
        th, _ = ob.trace(twin, rays)
    t_t = np.where(th[:, 0].view(np.int32) >= 0, th[:, 1].astype(np.float64), np.inf)
    shape = np.array([d.prims[i].shape for i in range(d.n_prims)], np.int64)
    integ = pt.CreatePathIntegrator(s)
    for scale in (1 + 2.0 ** -9, 2.0, 0.9):
        q = rays.copy()
        q[:, 6] = (r64["t"] * scale).astype(np.float32)
        end = q[:, 6].astype(np.float64)
        got, extra = integ.trace_wavefront(q, mode=3)
        gp = got[:, 0].view(np.int32)
        assert (extra[:, 3].view(np.int32) != -3).all()
        assert np.all((gp == -1) | (gp == -2) | ((gp >= 0) & (shape[np.maximum(gp, 0)] >= 0)))
        in_front = t_t < end * (1 - 2.0 ** -8) * (1 - 1e-3)
        clear = t_t > end * (1 + 1e-3)
        print("span end at %.4f t: %d with a triangle in front, %d clear, %d answered -2" % (scale, int(in_front.sum()), int(clear.sum()), int((gp == -2).sum())))
        assert in_front.sum() > 20 and clear.sum() > 200
        assert (gp[in_front] >= 0).all() and (gp[clear] == -1).all()
        if scale > 1:   # the sphere lies inside tMax: the kernel met its box and listed it
            assert ((extra[clear, 2].view(np.int32) & 0xff) >= 1).all()


LAMP_R, LAMP_H = .5, 2.0
LAMP_HEAD = ('LookAt 3 1.5 0  0 0 0  0 1 0\nCamera "perspective" "float fov" [0.1]\n'
             'Film "image" "integer xresolution" [4] "integer yresolution" [4]\n'
             'Sampler "halton" "integer pixelsamples" [%(spp)d]\n'
             'Integrator "path" "integer maxdepth" [%(depth)d]\nWorldBegin\n')
FLOOR = ('Material "matte" "rgb Kd" [.5 .5 .5]\n'
         'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-20 0 -20  20 0 -20  20 0 20  -20 0 20]\n')
SPHERE_LAMP = ('AttributeBegin\nAreaLightSource "diffuse" "rgb L" [4 4 4]\nTranslate 0 %g 0\nShape "sphere" "float radius" [%g]\nAttributeEnd\n' % (LAMP_H, LAMP_R))
MIRROR = ('AttributeBegin\nMaterial "mirror"\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 0.001 -3  -1 0.001 3  -1 4 3  -1 4 -3]\nAttributeEnd\n')


def _lamp_scene(pt, spp, depth, extra=""):
    s = pt.Scene(text=LAMP_HEAD % dict(spp=spp, depth=depth) + FLOOR + SPHERE_LAMP + extra + "WorldEnd\n")
    assert s.errors == [] and s.desc.n_spheres == 1 and s.desc.n_lights == 1
    return s


def _bin_means(film, weight):
    return (film.astype(np.float64) / weight[..., None]).mean(axis=(0, 1))


def _material_of(scene, shape):
    d = scene.desc
    mat = d.materials[[d.prims[i].material for i in range(d.n_prims) if d.prims[i].shape == shape][0]]
    assert mat.n_bxdfs == 1
    return np.array(list(mat.bxdf[0].R), np.float64)


def _lamp_expected(scene, mirror):
    """Per unit Le, the radiance a matte floor sends back from the point under a sphere light of radius R whose centre is h
    above it: Kd R^2 / h^2 (the cosine-weighted solid angle of a sphere wholly above the horizon, centre at distance d under
    the angle theta, is pi (R / d)^2 cos theta). The mirror in the plane x = -1 shows the floor point a second such sphere at
    (-2, h, 0), dimmed by Kr (FresnelNoOp, mirror.cpp): Kd Kr R^2 cos theta / d^2 more, which maxdepth 2 collects from
    BSDF-sampled rays alone (the path floor, mirror, light)."""
    kd = _material_of(scene, 0)
    out = kd * LAMP_R ** 2 / LAMP_H ** 2
    if mirror:
        d2 = 4 + LAMP_H ** 2
        out = out + kd * _material_of(scene, 2) * LAMP_R ** 2 * (LAMP_H / math.sqrt(d2)) / d2
    return out


def _lamp_spp(pt, ob):
    """The smallest power of two at which the oracle's render of lamp, mirror and floor meets the furnace bar of 0.02
    against the closed form."""
    if "lamp spp" not in _cache:
        for spp in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192):
            t = _lamp_scene(pt, spp, 2, MIRROR)
            with ob.exact_libm():
                film, weight, _, _ = ob.render(t)
            le = np.array(list(t.desc.lights[0].L), np.float64)
            rel = float(np.abs(_bin_means(film, weight) / (_lamp_expected(t, True) * le) - 1).max())
            if rel < 0.02:
                _cache["lamp spp"] = spp
                break
        assert "lamp spp" in _cache, "the oracle's sphere lamp does not meet 0.02 at 8192 spp"
    return _cache["lamp spp"]


def test_sphere_lamp_with_a_mirror(pt, ob):
    """One sphere light, a mirror and a floor, maxdepth 2, seen through a 0.1 degree field of view on the point under the
    lamp: BSDF-sampled MIS rays from the floor end on the sphere light, and the rays the mirror sends on are the only way
    to its image, so the sphere branch of ResolveMisVisibility and the closest-hit sphere test decide a quarter of the
    film. The device's film against the closed form and against the oracle's film to the furnace bar of 0.02 per bin, at the
    smallest power-of-two spp at which the oracle alone meets that bar on the closed form."""
    spp = _lamp_spp(pt, ob)
    s = _lamp_scene(pt, spp, 2, MIRROR)
    le = np.array(list(s.desc.lights[0].L), np.float64)
    assert (_lamp_expected(s, True) / _lamp_expected(s, False)).min() > 1.2
    integ = pt.CreatePathIntegrator(s)
    film, weight = integ.Render()
    c = integ.counters.as_dict()
    with ob.exact_libm():
        ofilm, oweight, oc, _ = ob.render(s)
    assert np.array_equal(weight, oweight) and c["bad_samples"] == 0 and c["camera_rays"] == 16 * spp
    closed = float(np.abs(_bin_means(film, weight) / (_lamp_expected(s, True) * le) - 1).max())
    rel = float(np.abs(_bin_means(film, weight) / _bin_means(ofilm, oweight) - 1).max())
    print("sphere lamp, mirror and floor, maxdepth 2, %d spp: worst relative error of a bin %.4f against the closed form, %.2e against the oracle"
          % (spp, closed, rel))
    assert closed < 0.02 and rel < 0.02, (closed, rel)
