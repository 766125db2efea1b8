"""MakeTriRay (d_scene.h): the permutation (kx, ky, kz) and the shear of Triangle::Intersect (triangle.cpp:199-291), formed
once per ray. kz = MaxDimension(|d|) decides with strict comparisons (geometry.h MaxDimension), so a tie between two
components goes to the later axis; the permuted direction is (d[kx], d[ky], d[kz]) with kx = kz + 1, ky = kz + 2 (mod 3).

 * in the traversal kernels: recorded rays through k_trace and k_trav<0>, <1>, <2> on a small mesh, directions led by each
   axis in both signs and the exact ties |dx| == |dy|, |dy| == |dz|, |dx| == |dz|, |dx| == |dy| == |dz| -- hit records
   bit-equal to the oracle's;
 * in k_shade's Shape::Pdf (the light's pdf of a BSDF-sampled direction, before anything is known about what the ray
   hits): two-triangle emitters facing along x, y and z over a matte and a plastic floor, which the plan routes to the two
   hot instances -- exact-mode parity at the bar of tests/test_gpu_parity.py, ray counters equal as integers."""
import itertools

import numpy as np
import pytest

import scenes_text as st
import trace_check as tc
from test_gpu_parity import _parity

pytestmark = pytest.mark.gpu


def _lumpy_cube_scene(pt, seed=3):
    """A cube around the origin, each face 2 x 2 quads (48 triangles), every vertex moved a little so that no triangle lies
    in an axis plane: one mesh, closed, so that a ray from inside meets it in every direction."""
    rng = np.random.default_rng(seed)
    verts, index, idx = [], {}, []

    def vertex(p):
        key = tuple(int(round(v)) for v in p)
        if key not in index:
            index[key] = len(verts)
            verts.append(np.asarray(p, np.float64) * 1.5 + rng.uniform(-.2, .2, 3))
        return index[key]

    for axis in range(3):
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for side in (-2, 2):
            for a in (-2, 0):
                for b in (-2, 0):
                    q = []
                    for da, db in ((0, 0), (2, 0), (2, 2), (0, 2)):
                        p = [0, 0, 0]
                        p[axis], p[u], p[v] = side, a + da, b + db
                        q.append(vertex(p))
                    idx += [q[0], q[1], q[2], q[0], q[2], q[3]]
    body = ('Shape "trianglemesh" "integer indices" [%s] "point P" [%s]\n'
            % (" ".join(map(str, idx)), " ".join(repr(float(np.float32(x))) for p in verts for x in p)))
    s = pt.Scene(text=st._HEAD % dict(res=8, spp=1, depth=1, extra="") + 'LightSource "point" "rgb I" [1 1 1]\n' + body + "WorldEnd\n")
    assert s.errors == [] and s.stats["n_triangles"] == 48
    return s


def _directions(rng):
    """[n, 3] float32 directions and, per direction, the kz the strict comparisons give."""
    d = []
    for axis in range(3):                       # one component leads, both signs
        for sign in (-1.0, 1.0):
            v = rng.uniform(-.9, .9, (40, 3))
            v[:, axis] = sign * rng.uniform(1.0, 2.0, 40)
            d.append(v)
    signs2 = list(itertools.product((-1.0, 1.0), repeat=2))
    for a, b in ((0, 1), (1, 2), (0, 2)):       # |d[a]| == |d[b]| exactly; the third below, above and equal in turn
        c = 3 - a - b
        for sa, sb in signs2:
            for third in (.25, -.6, 1.75, -3.0):
                m = np.float32(rng.uniform(.5, 2.0))
                v = np.zeros((4, 3))
                v[:, a], v[:, b] = sa * m, sb * m
                v[:, c] = third * m * rng.uniform(.9, 1.1, 4)
                d.append(v)
    for s3 in itertools.product((-1.0, 1.0), repeat=3):   # all three equal
        m = rng.uniform(.5, 2.0, 6).astype(np.float32)
        d.append(np.asarray(s3)[None, :] * m[:, None])
    d = np.concatenate(d).astype(np.float32)
    a = np.abs(d)
    kz = np.where(a[:, 0] > a[:, 1], np.where(a[:, 0] > a[:, 2], 0, 2), np.where(a[:, 1] > a[:, 2], 1, 2))
    return d, kz


def test_tri_ray_permutation_in_the_traversal_kernels(pt, ob):
    s = _lumpy_cube_scene(pt)
    rng = np.random.default_rng(29)
    d, kz = _directions(rng)
    n = len(d)
    assert 300 <= n <= 1000
    a = np.abs(d)
    for i, j in ((0, 1), (1, 2), (0, 2)):   # the ties are exact in float32, each with the tied pair leading and not leading
        tie = a[:, i] == a[:, j]
        k = 3 - i - j
        assert (tie & (a[:, k] < a[:, i])).sum() >= 16 and (tie & (a[:, k] > a[:, i])).sum() >= 16
    assert ((a[:, 0] == a[:, 1]) & (a[:, 1] == a[:, 2])).sum() >= 48
    assert all((kz == k).sum() >= 80 for k in range(3))
    o = rng.uniform(-.8, .8, (n, 3)).astype(np.float32)
    o[::5] = 0   # (from the centre, an all-equal direction runs into a corner of the undisturbed cube)
    tmax = np.where(rng.random(n) < .6, np.inf, rng.uniform(.5, 6, n)).astype(np.float32)
    rays = np.concatenate([o, d, tmax[:, None]], axis=1).astype(np.float32)
    integ = pt.CreatePathIntegrator(s)
    closest, occluded = tc.oracle_answers(ob, s)
    want = closest(rays)
    assert np.array_equal(tc.bits(integ.trace(rays)), tc.bits(want))                       # k_trace (TriTest)
    assert np.array_equal(tc.bits(integ.trace(rays, any_hit=True))[:, 0] >= 0, occluded(rays))
    hits, extra = tc.check_wavefront(integ, rays, closest, occluded)                        # k_trav<0>, <2>, <1>
    prim = tc.bits(hits)[:, 0]
    for k in range(3):   # hits and misses (tMax) under every permutation
        assert (prim[kz == k] >= 0).sum() >= 30 and (prim[kz == k] < 0).any()
    assert (prim[np.isinf(tmax)] >= 0).all()   # the mesh is closed


_EMITTERS = """
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [14 13 12] "bool twosided" ["true"]
  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-.4 .5 4.6  .4 .5 4.6  .4 .5 5.4  -.4 .5 5.4]
AttributeEnd
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [12 14 12] "bool twosided" ["true"]
  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [0 -.9 3.1  0 -.9 3.9  0 -.3 3.9  0 -.3 3.1]
AttributeEnd
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [12 13 15] "bool twosided" ["true"]
  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-.5 -.9 7.8  .5 -.9 7.8  .5 -.1 7.8  -.5 -.1 7.8]
AttributeEnd
AttributeBegin
  Material "matte" "rgb Kd" [.6 .55 .5]
  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-3 -1 2  0 -1 2  0 -1 8  -3 -1 8]
AttributeEnd
AttributeBegin
  Material "plastic" "rgb Kd" [.2 .3 .6] "rgb Ks" [.5 .5 .5] "float roughness" [.15]
  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [0 -1 2  3 -1 2  3 -1 8  0 -1 8]
AttributeEnd
WorldEnd
"""
_EMITTER_CENTRES = ((0, .5, 5), (0, -.6, 3.5), (0, -.5, 7.8))   # facing y, x, z


def test_tri_ray_permutation_in_shape_pdf_of_the_hot_instances(pt, ob):
    s = pt.Scene(text=st._HEAD % dict(res=32, spp=4, depth=5, extra="") + _EMITTERS)
    assert s.errors == [] and s.desc.n_lights == 6 and s.stats["n_triangles"] == 10
    # the floor's two materials route to the two hot instances
    plan = s.shade_plan()
    routed = {(c["nl"], c["tm"]) for k, c in plan["classes"].items() if k != pt.MISS_CLASS}
    assert routed == {(2, pt.TM_DIFFUSE | pt.TM_LIGHTS_NO_ENV), (2, pt.TM_PLASTIC | pt.TM_LIGHTS_NO_ENV)}, plan
    # ... and from each half of the floor the emitters lie in directions of every kz
    for half in (-1, 1):
        x, z = np.meshgrid(half * np.linspace(.1, 2.9, 15), np.linspace(2.1, 7.9, 30))
        p = np.stack([x.ravel(), np.full(x.size, -1.0), z.ravel()], -1)
        seen = set()
        for c in _EMITTER_CENTRES:
            a = np.abs(np.asarray(c)[None, :] - p)
            seen |= set(np.where(a[:, 0] > a[:, 1], np.where(a[:, 0] > a[:, 2], 0, 2), np.where(a[:, 1] > a[:, 2], 1, 2)).tolist())
        assert seen == {0, 1, 2}
    film, weight, integ, ofilm, oweight, oc = _parity(pt, ob, s, "triangle emitters along x, y, z over matte and plastic")
    c, o = integ.counters.as_dict(), oc.as_dict()
    for k in ("camera_rays", "regular_rays", "shadow_rays"):
        assert c[k] == o[k], (k, c[k], o[k])
    assert c["camera_rays"] == 32 * 32 * 4 and c["shadow_rays"] > c["camera_rays"] // 4
    assert film[16:].sum() > 0   # the lit floor is in view
