"""Object motion in the front end (MIPT_OBJECT_MOTION=1): moving instances and moving shapes as mi_instance + mi_motion,
what stays a reported error, the scene cache, the world bound of a moving primitive -- and, on the CPU, the two float32
facts the GPU tests rest on. No GPU."""
import numpy as np
import pytest

import camera_motion as cm
import object_motion as om

TRANSLATE = ("Translate -0.5 0.25 1.5", "Translate 1 0.75 2.5")
SCALED = ("Translate -0.5 0.25 1.5\nScale 1 1.5 0.75", "Translate 1 0.75 2.5\nScale 1.25 0.5 1")
ROTATE_90 = ("Translate -0.5 0.25 1.5\nScale 1 1.5 0.75", "Translate 1 0.75 2.5\nRotate 90 0.3 1 0.2\nScale 1.25 0.5 1")
ROTATE_179 = ("Translate -0.5 0.25 1.5\nScale 1 1.5 0.75", "Translate 1 0.75 2.5\nRotate 179 0.3 1 0.2\nScale 1.25 0.5 1")


@pytest.fixture
def on(monkeypatch):
    monkeypatch.setenv("MIPT_OBJECT_MOTION", "1")


def _bits(a):
    return (np.asarray(list(a), np.float32) + np.float32(0)).view(np.uint32)


def test_a_moving_instance_carries_the_decomposed_pair(pt, on):
    s = pt.Scene(text=om.bare_scene(om.mover("instance", *ROTATE_90), times=(0.25, 1.5)))
    assert s.errors == [] and s.warnings == []
    d = s.desc
    assert d.n_instances == 1 and d.n_motions == 1 and s.instance_names == ["mover"]
    inst, mo = d.instances[0], d.motions[0]
    assert inst.motion == 1 and inst.instance_id == 1
    assert mo.transform_start == 0.25 and mo.transform_end == 1.5 and mo.has_rotation == 1
    # each member is the matrix (and the stored inverse) a static instance under the same directives gets
    for member, (m, minv) in zip(ROTATE_90, ((inst.i2w, inst.w2i), (mo.i2w_end, mo.w2i_end))):
        static = pt.Scene(text=om.bare_scene(om.mover("instance", member, member)))
        assert static.errors == [] and static.desc.n_motions == 0
        assert np.array_equal(_bits(m), _bits(static.desc.instances[0].i2w))
        assert np.array_equal(_bits(minv), _bits(static.desc.instances[0].w2i))
    a = om.animated_of(s, 0)
    assert a.animated
    for name, got, want in (("T", mo.T, a.T), ("R", mo.R, a.R), ("S", mo.S, a.S)):
        got = np.array([list(r) for r in got], np.float32)
        dist = cm.ulp_distance(got, np.array(want, np.float32))
        print("%s: %d ulp from camera_motion.decompose" % (name, dist))
        assert dist == 0, (name, got, want)
    assert float(np.dot(np.array(list(mo.R[0]), np.float64), np.array(list(mo.R[1]), np.float64))) >= 0


def test_a_moving_shape_is_an_instance_without_a_number_or_a_name(pt, on):
    block = ('ObjectBegin "still"\n' + om.OCTAHEDRON + 'ObjectEnd\nObjectInstance "still"\n' + om.mover("shape", *TRANSLATE)
             + 'AttributeBegin\nTranslate 3 0 0\nObjectInstance "still"\nAttributeEnd\n')
    s = pt.Scene(text=om.bare_scene(block))
    assert s.errors == [] and s.warnings == []
    d = s.desc
    assert s.instance_names == ["still", "still"] and d.n_instances == 3 and d.n_motions == 1
    assert [(d.instances[k].instance_id, d.instances[k].motion) for k in range(3)] == [(1, 0), (0, 1), (2, 0)]
    # the shapes were made with the identity transform: the object's vertices are the file's
    wrapper = d.instances[1]
    ident = [1.0 if i % 5 == 0 else 0.0 for i in range(16)]
    assert not np.array_equal(_bits(wrapper.i2w), _bits(ident))
    P = np.array([d.P[i] for i in range(3 * d.n_verts)], np.float32).reshape(-1, 3)
    assert d.n_verts == 12 and np.array_equal(P[:6], om.OCTAHEDRON_P) and np.array_equal(P[6:], om.OCTAHEDRON_P)
    # every primitive of an object has instance id 0 in the per-primitive table: the id is the instance's
    assert all(d.prim_meta[i].instance_id == 0 for i in range(d.n_prims))


def test_the_area_light_of_a_moving_shape_is_dropped_with_the_references_warning(pt, on):
    light = 'AreaLightSource "diffuse" "rgb L" [5 5 5]\n'
    s = pt.Scene(text=om.bare_scene(om.mover("shape", *TRANSLATE, before_shape=light)))
    without = pt.Scene(text=om.bare_scene(om.mover("shape", *TRANSLATE)))
    assert s.errors == [] and s.warnings == ["Ignoring currently set area light when creating animated shape"]
    assert s.desc.n_lights == without.desc.n_lights == 1 and s.desc.n_motions == 1
    assert all(s.desc.prims[i].area_light == -1 for i in range(s.desc.n_prims))


@pytest.mark.parametrize("kind", ["instance", "shape"])
def test_equal_members_are_not_animated(pt, on, kind):
    s = pt.Scene(text=om.bare_scene(om.mover(kind, TRANSLATE[0], TRANSLATE[0])))
    assert s.errors == [] and s.desc.n_motions == 0
    assert s.desc.n_instances == (1 if kind == "instance" else 0)


def test_a_moving_shape_inside_an_object_is_still_an_error(pt, on):
    block = 'ObjectBegin "o"\n' + om.pair(*TRANSLATE) + om.OCTAHEDRON + 'ObjectEnd\nObjectInstance "o"\n'
    s = pt.Scene(text=om.bare_scene(block))
    assert s.errors == ['Shape "trianglemesh": animated transforms of shapes are outside the hot-path scope; using the start transform']
    assert s.desc.n_motions == 0


@pytest.mark.parametrize("kind", ["instance", "shape"])
def test_without_the_switch_nothing_moves(pt, monkeypatch, kind):
    monkeypatch.delenv("MIPT_OBJECT_MOTION", raising=False)
    s = pt.Scene(text=om.bare_scene(om.mover(kind, *TRANSLATE)))
    assert len(s.errors) == 1 and "outside the hot-path scope; using the start transform" in s.errors[0]
    assert s.desc.n_motions == 0 and not s.desc.motions
    assert all(s.desc.instances[k].motion == 0 for k in range(s.desc.n_instances))


def test_moving_instances_are_never_expanded(pt, on, monkeypatch):
    monkeypatch.setenv("MIPT_INSTANCES", "expand")
    block = om.mover("instance", *TRANSLATE) + 'AttributeBegin\nTranslate 3 0 0\nObjectInstance "mover"\nAttributeEnd\n'
    s = pt.Scene(text=om.bare_scene(block))
    assert s.errors == [] and s.instance_names == ["mover", "mover"]
    assert s.desc.n_instances == 1 and s.desc.n_motions == 1 and s.desc.instances[0].instance_id == 1


def test_scene_cache_round_trip(pt, on, tmp_path):
    block = om.mover("instance", *ROTATE_90) + om.mover("shape", *SCALED)
    s = pt.Scene(text=om.bare_scene(block, times=(0.25, 1.5)))
    assert s.errors == [] and s.desc.n_motions == 2
    path = str(tmp_path / "scene.cache")
    s.save_cache(path)
    t = pt.Scene(cache=path)
    assert t.desc.n_motions == 2 and t.desc.n_instances == 2 and t.instance_names == ["mover"]
    for k in range(2):
        assert bytes(s.desc.motions[k]) == bytes(t.desc.motions[k])
        assert bytes(s.desc.instances[k]) == bytes(t.desc.instances[k])
    raw = bytearray(open(path, "rb").read())
    off = 8 + 16 + type(s.desc).n_motions.offset
    assert int.from_bytes(raw[off:off + 4], "little") == 2
    raw[off:off + 4] = (3).to_bytes(4, "little")
    bad = str(tmp_path / "bad.cache")
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(RuntimeError):
        pt.Scene(cache=bad)


# ---------------------------------------------------------------------------------------------------------------------
# MotionBounds
OBJ_LO, OBJ_HI = om.OCTAHEDRON_P.min(axis=0), om.OCTAHEDRON_P.max(axis=0)


@pytest.mark.parametrize("kind", ["instance", "shape"])
def test_without_rotation_the_world_bound_is_the_union_of_the_members_bounds(pt, on, kind):
    s = pt.Scene(text=om.bare_scene(om.mover(kind, *SCALED)))
    assert s.errors == [] and s.desc.motions[0].has_rotation == 0
    lo0, hi0 = om.transform_bounds(list(s.desc.instances[0].i2w), OBJ_LO, OBJ_HI)
    lo1, hi1 = om.transform_bounds(list(s.desc.motions[0].i2w_end), OBJ_LO, OBJ_HI)
    lo, hi = om.world_bound(s)
    assert np.array_equal(lo.view(np.uint32), np.minimum(lo0, lo1).view(np.uint32))
    assert np.array_equal(hi.view(np.uint32), np.maximum(hi0, hi1).view(np.uint32))


FAR = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3 0 3 1 1 3 2] "point P" [10 0 0  11 0 0  10 1.5 0  10 0 .5]\n'
FAR_LO, FAR_HI = np.array([10, 0, 0], np.float32), np.array([11, 1.5, .5], np.float32)


@pytest.mark.parametrize("name, members, shape, lo, hi", [("90 degrees", ROTATE_90, om.OCTAHEDRON, OBJ_LO, OBJ_HI),
                                                          ("179 degrees", ROTATE_179, om.OCTAHEDRON, OBJ_LO, OBJ_HI),
                                                          ("90 degrees, vertices 10 units from the object's origin", ROTATE_90, FAR, FAR_LO, FAR_HI)],
                         ids=["90", "179", "90 far from the origin"])
def test_with_rotation_the_world_bound_contains_every_corners_path(pt, on, name, members, shape, lo, hi):
    """The bound is our own: held to the float64 restatement of Interpolate at 2 000 times across the interval."""
    s = pt.Scene(text=om.bare_scene(om.mover("instance", *members, shape=shape)))
    assert s.errors == [] and s.desc.motions[0].has_rotation == 1
    a = om.animated_of(s, 0, np.float64)
    OBJ_LO, OBJ_HI = lo, hi
    corners = np.array([[x, y, z, 1.0] for x in (OBJ_LO[0], OBJ_HI[0]) for y in (OBJ_LO[1], OBJ_HI[1]) for z in (OBJ_LO[2], OBJ_HI[2])])
    pts = []
    for t in np.linspace(0.0, 1.0, 2000):
        m = np.array(a.interpolate(t), np.float64).reshape(4, 4)
        pts.append((corners @ m.T)[:, :3])
    pts = np.concatenate(pts)
    lo, hi = om.world_bound(s)
    assert np.all(pts >= lo.astype(np.float64)) and np.all(pts <= hi.astype(np.float64))
    ext, sampled = (hi - lo).astype(np.float64), pts.max(axis=0) - pts.min(axis=0)
    area = lambda e: 2 * (e[0] * e[1] + e[0] * e[2] + e[1] * e[2])
    print("%s: surface area of the bound over the sampled bound's: %.3f" % (name, area(ext) / area(sampled)))


# ---------------------------------------------------------------------------------------------------------------------
# the float32 facts the GPU tests rest on
def test_the_3x3_gauss_jordan_gives_the_4x4_routines_bits():
    """The device inverts the interpolated scale on its 3x3 block (d_scene.h, InverseScale3)."""
    rng = np.random.default_rng(11)
    cases = [rng.normal(size=9) for _ in range(300)]
    cases += [np.diag(rng.uniform(0.2, 3, 3)).ravel() for _ in range(20)]                 # pure scales: equal maxima, zeros
    cases += [np.array([1, 0, 0, 0, 1, 0, 0, 0, 1.0]), np.array([0, 2, 0, 1, 0, 0, 0, 0, 1.0]), np.array([1, 1, 0, 1, -1, 0, 0, 0, 1.0])]
    for m9 in cases:
        m9 = m9.astype(np.float32)
        m4 = [[m9[3 * r + c] for c in range(3)] + [np.float32(0)] for r in range(3)] + [[np.float32(0)] * 3 + [np.float32(1)]]
        full = cm._inverse(m4, np.float32)
        block = om.inverse3(list(m9), np.float32)
        assert np.array_equal(_bits([full[r][c] for r in range(3) for c in range(3)]), _bits(block)), m9
        assert [float(full[r][3]) for r in range(3)] == [0, 0, 0] and [float(v) for v in full[3]] == [0, 0, 0, 1]


def test_a_translation_interpolates_to_a_translation_and_its_stored_inverse(pt, on):
    """Frozen shutter at 0.5: the product and its mInv are Translate(lerp) and Translate(-lerp), zero signs aside."""
    s = pt.Scene(text=om.bare_scene(om.mover("instance", *TRANSLATE)))
    m, minv = om.matrices_at(s, 0, 0.5)
    v = [np.float32(0.5) * np.float32(a) + np.float32(0.5) * np.float32(b) for a, b in zip((-0.5, 0.25, 1.5), (1, 0.75, 2.5))]
    mid = pt.Scene(text=om.bare_scene(om.mover("instance", *(["Translate %r %r %r" % tuple(float(x) for x in v)] * 2))))
    assert mid.desc.n_motions == 0
    assert cm.same_up_to_zero_signs(m, list(mid.desc.instances[0].i2w))
    assert cm.same_up_to_zero_signs(minv, list(mid.desc.instances[0].w2i))
    assert not cm.same_up_to_zero_signs(m, list(s.desc.instances[0].i2w))


def test_the_restated_inverse_inverts_the_restated_matrix(pt, on):
    s = pt.Scene(text=om.bare_scene(om.mover("instance", *ROTATE_90)))
    for f, tol in ((np.float32, 2e-6), (np.float64, 1e-6)):
        m, minv = om.matrices_at(s, 0, 0.4, f)
        prod = np.array(m, np.float64).reshape(4, 4) @ np.array(minv, np.float64).reshape(4, 4)
        assert np.allclose(prod, np.eye(4), atol=tol)


def test_the_restatement_alone_stays_under_the_unsure_cap(pt, ob, on):
    """The ray families of test_object_motion_gpu.py's per-ray test -- the frame's camera rays, rays grazing the silhouette,
    tMax either side of the hit; one and two moving instances, a sphere in the object, overflowing lists: where the float32
    and the float64 restatement of the instances' matrices (the latter rounded to float32 for the oracle) find different
    primitives a query is unsure, and at most 1 % of a family may be at any time -- checked here without a GPU. At and outside
    the transform times both are the members themselves."""
    import test_object_motion_gpu as g

    def prims(s, twin, rays, time, f):
        om.set_moving(s, twin, time, f)
        with ob.exact_libm():
            h = ob.trace(twin, rays[:, :7])[0]
        return h[:, 0].copy().view(np.int32), h[:, 1]

    for kind, shape, world in (("instance", om.OCTAHEDRON, ""), ("instance", g.WITH_SPHERE, ""), ("shape", om.OCTAHEDRON, g.SHELLS),
                               ("two", om.OCTAHEDRON, "")):
        text = om.lit_scene(world + g._block(kind, shape), times=(g.T0, g.T1))
        s, twin = pt.Scene(text=text), pt.Scene(text=text)
        samples = cm.all_samples(s, 4)
        rays = np.zeros((len(samples), 8), np.float32)
        rays[:, :7] = ob.camera_rays(s, samples)
        rays[:, 7] = g.TIMES[np.arange(len(samples)) % len(g.TIMES)]
        prim32, t32 = np.zeros(len(rays), np.int32), np.zeros(len(rays), np.float32)
        for time in g.TIMES:
            sel = rays[:, 7] == time
            prim32[sel], t32[sel] = prims(s, twin, rays[sel], time, np.float32)
        of_object = np.arange(s.desc.n_prims) >= s.desc.n_prims - (9 if shape is g.WITH_SPHERE else 8)
        families = {"frame": rays, "grazing": om.grazing_rays(s, rays[0, :3], g.TIMES),
                    "tMax either side": g._near_rays(rays, prim32, t32, of_object)[0]}
        for name, fam in families.items():
            for time in g.TIMES:
                sel = fam[:, 7] == time
                assert sel.sum() >= 10, (name, float(time))
                unsure = int((prims(s, twin, fam[sel], time, np.float32)[0] != prims(s, twin, fam[sel], time, np.float64)[0]).sum())
                assert unsure <= 0.01 * sel.sum(), (kind, name, float(time), unsure, int(sel.sum()))
                if time <= g.T0 or time >= g.T1:
                    assert unsure == 0
        hit = of_object[np.maximum(prim32, 0)] & (prim32 >= 0)
        g_prim = np.concatenate([prims(s, twin, families["grazing"][families["grazing"][:, 7] == t], t, np.float32)[0] for t in g.TIMES])
        g_hit = of_object[np.maximum(g_prim, 0)] & (g_prim >= 0)
        print("%s: %d frame rays on a moving object, %.2f of the grazing rays" % (kind, hit.sum(), g_hit.mean()))
