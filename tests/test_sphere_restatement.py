"""sphere_shape.py, the numpy restatement of Shape "sphere", checked where no GPU is needed: against closed forms in float64,
against the oracle in float32 (verdict and the bits of t; sampled p, n and pdf), and on the reference's own Sphere.SolidAngle
fixture. test_sphere_gpu.py holds the device to it."""
import ctypes as C
import math

import numpy as np
import pytest

import sphere_cases as sc
import sphere_shape as ss

_F = C.POINTER(C.c_float)


def _f(a):
    return a.ctypes.data_as(_F)


def _one(pt, body):
    s = pt.Scene(text=sc.text(body))
    assert s.errors == [] and s.desc.n_spheres == 1
    return s


PLACED = {"at the origin": ("", np.zeros(3), 1.0),
          "translated, scaled by 2": ("Translate .5 -1 2\nScale 2 2 2\n", np.array([.5, -1, 2]), 2.0)}


def _shift(o, c):
    """The bound on what Transform::operator()(Ray, oErr, dErr) takes from t (transform.h:384-396): it moves the origin along
    a unit d by Dot(|d|, oErr) / |d|^2 <= sqrt(3) gamma(3) (|o|_1 + |c|_1), a float32-sized parameter of the algorithm that
    the float64 restatement keeps."""
    return 2 * float(ss.GAMMA3) * (np.abs(o).sum(axis=1) + np.abs(c).sum())


@pytest.mark.parametrize("where", list(PLACED))
def test_closed_forms(pt, where):
    """float64, a unit sphere: t of rays towards the centre, the chord from inside, n = (p - c) / |p - c|, (u, v) at known
    (phi, theta), and the cone pdf 1 / (2 pi (1 - sqrt(1 - r^2 / d^2))). The matrices are exact in float32; the bar is 1e-6 of
    the quantity, for t beside the shift of the origin by its error bound (_shift). The float32-sized intervals decide nothing
    here: every root is far from 0 and from tMax."""
    xf, c, scale = PLACED[where]
    s = _one(pt, 'AttributeBegin\n%sShape "sphere" "float radius" [1]\nAttributeEnd\n' % xf)
    sp = ss.Sphere(s.desc.spheres[0], np.float64)
    rng = np.random.default_rng(5)
    n = 500
    w = rng.normal(size=(n, 3))
    w /= np.linalg.norm(w, axis=1)[:, None]
    # towards the centre from distance D: t = D - R, the point on the segment, n back along the ray
    D = rng.uniform(1.5, 20, n) * scale
    o = c + D[:, None] * w
    it = ss.intersect(sp, np.concatenate([o, -w, np.full((n, 1), np.inf)], axis=1))
    assert it["hit"].all() and (it["root"] == 0).all()
    assert (np.abs(it["t"] - (D - scale)) <= 1e-6 * (D - scale) + _shift(o, c)).all()
    assert np.allclose(it["p"], c + scale * w, rtol=0, atol=1e-6 * scale)
    assert np.allclose(it["n"], w, rtol=0, atol=1e-6)
    # (u, v): phi = atan2(y, x) in [0, 2 pi), theta = acos(z); thetaMin = pi, thetaMax = 0 for a full sphere
    phi = np.arctan2(w[:, 1], w[:, 0])
    phi = np.where(phi < 0, phi + 2 * math.pi, phi)
    assert np.allclose(it["uv"][:, 0], phi / (2 * math.pi), rtol=0, atol=1e-6)
    assert np.allclose(it["uv"][:, 1], (np.arccos(w[:, 2]) - math.pi) / (0 - math.pi), rtol=0, atol=1e-6)
    # dpdu, dpdv are tangent, and dpdu x dpdv points outward (no ReverseOrientation, no swap of handedness)
    assert np.abs((it["dpdu"] * w).sum(axis=1)).max() < 1e-5 * scale and np.abs((it["dpdv"] * w).sum(axis=1)).max() < 1e-5 * scale
    assert ((np.cross(it["dpdu"], it["dpdv"]) * w).sum(axis=1) > 0).all()
    # the chord from inside, along a unit direction: t = -(o' . d) + sqrt((o' . d)^2 - |o'|^2 + R^2)
    op = w * (rng.uniform(0, .95, n) * scale)[:, None]
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    od = (op * d).sum(axis=1)
    chord = -od + np.sqrt(od * od - (op * op).sum(axis=1) + scale * scale)
    it = ss.intersect(sp, np.concatenate([c + op, d, np.full((n, 1), np.inf)], axis=1))
    assert it["hit"].all() and (it["root"] == 1).all()
    assert (np.abs(it["t"] - chord) <= 1e-6 * chord + _shift(c + op, c)).all()
    # the cone pdf: Sphere::Sample takes the radius as written, 1, and the centre in world space
    for dist in (1.5, 3.0, 40.0):
        ref = c + dist * w[0]
        want = 1 / (2 * math.pi * (1 - math.sqrt(1 - 1 / dist ** 2)))
        p, nn, pdf = ss.sample(sp, ref, rng.random((50, 2)))
        # (float32 cancellation in 1 - sin^2 is not there in float64; what remains is the float Pi: 3e-8)
        assert np.allclose(pdf, want, rtol=1e-6) and np.allclose(ss.pdf(sp, ref, -w[:50]), want, rtol=1e-6)
        assert np.allclose(np.linalg.norm(p - c, axis=1), 1, atol=1e-6) and np.allclose(nn, p - c, atol=1e-6)
        # every sampled point lies inside the cone of half angle asin(1 / dist) about the centre, and faces the point
        to = p - ref
        cosang = (to * (c - ref)).sum(axis=1) / (np.linalg.norm(to, axis=1) * dist)
        assert (cosang >= math.sqrt(1 - 1 / dist ** 2) - 1e-6).all() and ((nn * to).sum(axis=1) <= 1e-6).all()


def test_area(pt):
    """Sphere::Area against phiMax * r * (zMax - zMin), the parameters as the scene file states them."""
    for name, want in (("full", 2 * math.pi * 1.5 * 3.0), ("zmin/zmax", 2 * math.pi * 1.5 * 1.5), ("phimax", math.radians(200) * 1.5 * 3.0),
                       ("all three", math.radians(300) * 1.5 * 1.5), ("reversed, small, far", math.radians(270) * 1e-2 * 2e-2)):
        s, q = sc.scene(pt, name, plain=False)
        a32, a64 = [x.area() for x in ss.both(s.desc.spheres[q])]
        assert abs(a64 / want - 1) < 1e-6 and abs(float(a32) / want - 1) < 1e-6, name


def _oracle_samples(ob, s, ref, u):
    out = np.zeros((len(u), 7), np.float32)
    refp, u = np.ascontiguousarray(ref, np.float32), np.ascontiguousarray(u, np.float32)
    lib = ob.lib()
    lib.oracle_shape_sample.argtypes = [C.POINTER(type(s.desc)), C.c_int, _F, C.c_int, _F, _F]
    lib.oracle_shape_sample(s.desc_ptr, ~0, _f(refp), len(u), _f(u), _f(out))
    return out


def _oracle_pdf(ob, s, area, ref, wi):
    lib = ob.lib()
    lib.oracle_shape_pdf.argtypes = [C.POINTER(type(s.desc)), C.c_int, C.c_float, _F, _F]
    lib.oracle_shape_pdf.restype = C.c_float
    refp, wi = np.ascontiguousarray(ref, np.float32), np.ascontiguousarray(wi, np.float32)
    return np.array([lib.oracle_shape_pdf(s.desc_ptr, ~0, float(area), _f(refp), _f(wi[i])) for i in range(len(wi))], np.float32)


@pytest.mark.parametrize("name", list(sc.SHAPES))
def test_float32_restatement_against_the_oracle(pt, ob, name):
    """The six shapes of test_sphere_gpu.py, each alone in a scene. intersect against oracle_trace under correctly rounded
    libm calls: the verdict and the bits of t on every ray of every family. sample / pdf against oracle_shape_sample /
    oracle_shape_pdf from the five reference points: p, n to 1e-3 (of the radius; of 1), pdf to 1e-3 relative -- the bars
    test_shape_pins.py holds these entry points to -- with zeros in the same places; the count of values that are not
    bit-identical is printed."""
    s, q = sc.scene(pt, name, plain=False)
    rec = s.desc.spheres[q]
    s32 = ss.Sphere(rec, np.float32)
    rng = np.random.default_rng(23)
    with ob.exact_libm():
        for fam in sc.families(rec, rng):
            it = ss.intersect(s32, fam.rays)
            th, _ = ob.trace(s, fam.rays)
            o_hit = th[:, 0].view(np.int32) >= 0
            differ = np.nonzero(o_hit != it["hit"])[0]
            assert len(differ) == 0, (name, fam.name, fam.rays[differ[0]].tolist(), len(differ))
            assert np.array_equal(th[o_hit, 1].view(np.uint32), it["t"][o_hit].view(np.uint32)), (name, fam.name)
            any_hit = ob.trace(s, fam.rays, any_hit=True)[0][:, 0].view(np.int32) >= 0
            assert np.array_equal(any_hit, it["hit"]), (name, fam.name)
        u = sc.sample_points(rng, 200)
        r = float(rec.radius)
        targets = np.concatenate([f.targets[:40] for f in sc.families(rec, rng, n=80) if f.targets is not None])
        for label, ref, is_inside in sc.reference_points(rec):
            assert ss.inside(s32, ref) == is_inside, (name, label)
            p, n, pdf = ss.sample(s32, ref, u)
            want = _oracle_samples(ob, s, ref, u)
            assert np.array_equal(want[:, 6] == 0, pdf == 0), (name, label)
            worst = (np.abs(want[:, 0:3] - p).max() / r, np.abs(want[:, 3:6] - n).max(), np.abs(pdf[pdf > 0] / want[pdf > 0, 6] - 1).max())
            loose = int((want.view(np.uint32) != np.concatenate([p, n, pdf[:, None]], axis=1).view(np.uint32)).any(axis=1).sum())
            print("%s, ref %s: Sample worst p %.2e r, n %.2e, pdf %.2e relative; %d of %d not bit-identical" % ((name, label) + worst + (loose, len(u))))
            assert worst[0] <= 1e-3 and worst[1] <= 1e-3 and worst[2] <= 1e-3, (name, label, worst)
            to = np.concatenate([targets, p.astype(np.float64)]) - ref.astype(np.float64)
            keep = np.linalg.norm(to, axis=1) > 0
            wi = (to[keep] / np.linalg.norm(to[keep], axis=1)[:, None]).astype(np.float32)
            mine = ss.pdf(s32, ref, wi)
            theirs = _oracle_pdf(ob, s, s32.area(), ref, wi)
            assert np.array_equal(theirs == 0, mine == 0), (name, label)
            pos = mine > 0
            rel = float(np.abs(mine[pos] / theirs[pos] - 1).max()) if pos.any() else 0.0
            print("%s, ref %s: Pdf worst %.2e relative over %d, %d zeros; %d not bit-identical" %
                  (name, label, rel, int(pos.sum()), int((~pos).sum()), int((mine.view(np.uint32) != theirs.view(np.uint32)).sum())))
            assert rel <= 1e-3, (name, label, rel)


def test_sphere_solid_angle_of_the_restatement(pt):
    """Sphere.SolidAngle (src/tests/shapes.cpp:331-348) on the restatement alone, with the reference's transform, radius, points
    and sample count: the mean of 1 / pdf over Sample(ref, u) (Shape::SolidAngle, shape.cpp:89-103; every sampled point of a
    lone convex shape is visible from outside, and from inside) is 4 pi to 0.01 from the inside point and the cone's
    2 pi (1 - cos theta_max) to 0.001 from the outside one."""
    s = _one(pt, 'AttributeBegin\nTranslate 1 .5 -.8\nRotate 30 1 0 0\nShape "sphere" "float radius" [1]\nAttributeEnd\n')
    s32 = ss.Sphere(s.desc.spheres[0], np.float32)
    n = 128 * 1024
    u = sc.radical_pairs(n)
    _, _, pdf = ss.sample(s32, np.array([1, .9, -.8], np.float32), u)
    inside = float((1.0 / pdf[pdf > 0].astype(np.float64)).sum() / n)
    _, _, pdf = ss.sample(s32, np.array([-.25, -1, .8], np.float32), u)
    outside = float((1.0 / pdf.astype(np.float64)).sum() / n)
    d2 = ((np.array([-.25, -1, .8]) - np.array([1, .5, -.8])) ** 2).sum()
    closed = 2 * math.pi * (1 - math.sqrt(1 - 1 / d2))
    print("Sphere.SolidAngle of the restatement: inside %.5f (4 pi = %.5f), outside %.5f (closed form %.5f)" % (inside, 4 * math.pi, outside, closed))
    assert abs(inside - 4 * math.pi) < .01 and abs(outside - closed) < .001
