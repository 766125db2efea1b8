"""Shape "disk" in the front end (ABI v14): the mi_disk record, the index space it shares with the spheres, its world
bound, area lights, object instances, what stays an error, and the scene cache. No GPU."""
import math

import numpy as np
import pytest

import disk_shape as ds

HEAD = ('LookAt 0 0 8  0 0 0  0 1 0\nCamera "perspective" "float fov" [40]\n'
        'Film "image" "integer xresolution" [8] "integer yresolution" [8]\n')
TRI = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-3 -3 -1  3 -3 -1  0 3 -1]\n'


def _scene(pt, body, head=HEAD):
    return pt.Scene(text=head + "WorldBegin\n" + body + "WorldEnd\n")


def _f32(x):
    return float(np.float32(x))


def _world_bound(s):
    n = s.desc.nodes[0]
    return np.array(list(n.bmin), np.float32), np.array(list(n.bmax), np.float32)


def test_abi_version_is_15(pt):
    s = _scene(pt, TRI)
    assert s.desc.abi_version == 15
    assert "n_disks" in s.stats and s.stats["n_disks"] == 0 and s.desc.n_disks == 0


def test_parameters_and_defaults(pt):
    s = _scene(pt, 'Shape "disk"\nShape "disk" "float height" [.7] "float radius" [2.5] "float innerradius" [.5] "float phimax" [200]\n')
    assert s.errors == [] and s.warnings == ['No light sources defined in scene; rendering a black image.']
    assert s.stats["n_disks"] == 2 and s.desc.n_disks == 2 and s.stats["n_spheres"] == 0 and s.desc.n_prims == 2
    a, b = s.desc.disks[0], s.desc.disks[1]
    assert (a.height, a.radius, a.inner_radius) == (0.0, 1.0, 0.0) and a.kind == 0
    assert a.phi_max == _f32(np.float32(math.pi / 180) * np.float32(360))      # Radians(360) in float32
    assert (b.height, b.radius, b.inner_radius) == (_f32(.7), 2.5, .5)
    assert b.phi_max == _f32(np.float32(math.pi / 180) * np.float32(200))
    assert a.reverse_orientation == 0 and a.swaps_handedness == 0
    ident = np.eye(4, dtype=np.float32).ravel()
    assert np.array_equal(np.array(list(a.o2w), np.float32), ident) and np.array_equal(np.array(list(a.w2o), np.float32), ident)


@pytest.mark.parametrize("given, clamped", [(-30, 0), (400, 360), (360, 360), (90, 90)])
def test_phimax_is_clamped_to_a_turn(pt, given, clamped):
    s = _scene(pt, 'Shape "disk" "float phimax" [%d]\n' % given)
    assert s.errors == []
    assert s.desc.disks[0].phi_max == _f32(np.float32(math.pi / 180) * np.float32(clamped))


def test_alpha_parameters_are_ignored_as_in_the_reference(pt):
    """CreateDiskShape (disk.cpp:140-150) reads neither "alpha" nor "shadowalpha": no mask, no error, the usual note."""
    s = _scene(pt, 'Texture "a" "float" "constant" "float value" [0]\nShape "disk" "texture alpha" "a" "texture shadowalpha" "a"\n')
    assert s.errors == [] and s.stats["n_disks"] == 1 and s.desc.n_meshes == 0


def test_orientation_flags(pt):
    s = _scene(pt, 'AttributeBegin\nReverseOrientation\nShape "disk"\nAttributeEnd\n'
                   'AttributeBegin\nScale 1 -2 .5\nShape "disk"\nAttributeEnd\n')
    a, b = s.desc.disks[0], s.desc.disks[1]
    assert (a.reverse_orientation, a.swaps_handedness) == (1, 0)
    assert (b.reverse_orientation, b.swaps_handedness) == (0, 1)
    # w2o is the stored inverse
    m, mi = np.array(list(b.o2w), np.float64).reshape(4, 4), np.array(list(b.w2o), np.float64).reshape(4, 4)
    assert np.allclose(m @ mi, np.eye(4), atol=1e-6)


def test_world_bound_under_rotate_and_nonuniform_scale(pt):
    """Shape::WorldBound = ObjectToWorld(ObjectBound) over the box's eight corners (shape.cpp:54, transform.cpp:168-178):
    the union of the transformed corners of [-r, r]^2 x {height}, each carried in float32."""
    s = _scene(pt, 'Translate .5 -1 2\nRotate 35 1 2 .5\nScale 1 2 .5\nShape "disk" "float radius" [1.5] "float height" [.7]\n')
    assert s.errors == [] and s.desc.n_nodes == 1
    k = s.desc.disks[0]
    m = np.array(list(k.o2w), np.float32).reshape(4, 4)
    corners = np.array([[x, y, k.height] for x in (-1.5, 1.5) for y in (-1.5, 1.5)], np.float32)
    w = ds.xf_point(m, corners)
    lo, hi = _world_bound(s)
    assert np.array_equal(lo, w.min(axis=0)) and np.array_equal(hi, w.max(axis=0))
    # the rim of the disk lies inside it (float64, with the slack of the float32 corners)
    phi = np.linspace(0, 2 * math.pi, 721)
    rim = np.stack([1.5 * np.cos(phi), 1.5 * np.sin(phi), np.full_like(phi, float(k.height)), np.ones_like(phi)], axis=1) @ m.astype(np.float64).T
    assert np.all(rim[:, :3] >= lo - 1e-5) and np.all(rim[:, :3] <= hi + 1e-5)


def test_index_space_with_spheres_and_disks_mixed(pt):
    """A negative shape is ~index: [0, n_spheres) spheres, then the disks -- whatever the order in the file."""
    body = ('AttributeBegin\nTranslate -4 0 0\nShape "disk" "float radius" [.25]\nAttributeEnd\n'
            'AttributeBegin\nTranslate -2 0 0\nShape "sphere" "float radius" [.5]\nAttributeEnd\n'
            'AttributeBegin\nTranslate 0 0 0\nShape "disk" "float radius" [.75]\nAttributeEnd\n'
            'AttributeBegin\nTranslate 2 0 0\nShape "sphere" "float radius" [1]\nAttributeEnd\n' + TRI)
    s = _scene(pt, body)
    d = s.desc
    assert s.errors == [] and (d.n_spheres, d.n_disks, d.n_tris, d.n_prims) == (2, 2, 1, 5)
    assert s.stats["n_spheres"] == 2 and s.stats["n_disks"] == 2
    seen = {}
    for i in range(d.n_prims):
        p = d.prims[i]
        if p.shape >= 0:
            continue
        q = ~p.shape
        assert 0 <= q < d.n_spheres + d.n_disks
        seen[q] = (d.spheres[q].radius, d.spheres[q].o2w[3]) if q < d.n_spheres else (d.disks[q - d.n_spheres].radius, d.disks[q - d.n_spheres].o2w[3])
    assert seen == {0: (.5, -2.0), 1: (1.0, 2.0), 2: (.25, -4.0), 3: (.75, 0.0)}


def test_area_and_area_light_binding(pt):
    body = ('AttributeBegin\nAreaLightSource "diffuse" "rgb L" [3 2 1]\nShape "sphere" "float radius" [.5]\nAttributeEnd\n'
            'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [1 2 3] "bool twosided" "true"\nTranslate 0 3 0\n'
            'Shape "disk" "float radius" [2] "float innerradius" [.5] "float phimax" [200]\nAttributeEnd\n'
            'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [1 1 1]\nTranslate 0 -3 0\nShape "disk"\nAttributeEnd\n' + TRI)
    s = _scene(pt, body)
    d = s.desc
    assert s.errors == [] and d.n_lights == 3 and d.n_disks == 2
    lights = [d.lights[i] for i in range(3)]
    assert [l.type for l in lights] == [lights[0].type] * 3
    assert [~l.shape for l in lights] == [0, 1, 2] and [l.two_sided for l in lights] == [0, 1, 0]
    k = ds.Disk(d.disks[0])
    assert lights[1].area == float(k.area())                                   # phiMax * 0.5 * (r^2 - ri^2) in float32
    assert abs(lights[1].area - math.radians(200) * 0.5 * (4 - .25)) < 1e-5
    assert abs(lights[2].area - math.pi) < 1e-6
    # every area light is the shape of exactly one primitive, which names it
    for i in range(d.n_prims):
        p = d.prims[i]
        if p.area_light >= 0:
            assert d.lights[p.area_light].shape == p.shape
    assert sorted(d.prims[i].area_light for i in range(d.n_prims)) == [-1, 0, 1, 2]


@pytest.mark.parametrize("strategy", ["uniform", "power"])
def test_power_distribution_takes_the_disk(pt, strategy):
    """DiffuseAreaLight::Power = (twoSided ? 2 : 1) * L * area * Pi (diffuse.cpp:62-64): `power` weighs the lights by it."""
    body = ('AttributeBegin\nAreaLightSource "diffuse" "rgb L" [1 1 1] "bool twosided" "true"\nShape "disk" "float radius" [2]\nAttributeEnd\n'
            'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [1 1 1]\nTranslate 0 0 -3\nShape "disk"\nAttributeEnd\n')
    s = pt.Scene(text=HEAD + 'Integrator "path" "string lightsamplestrategy" "%s"\nWorldBegin\n' % strategy + body + "WorldEnd\n")
    assert s.errors == []
    func = np.array([s.desc.light_distrib.func[i] for i in range(s.desc.n_lights)], np.float64)
    want = np.array([8.0, 1.0]) if strategy == "power" else np.array([1.0, 1.0])     # 2 * (pi 2^2) * pi against 1 * pi * pi
    assert np.allclose(func / func[1], want, rtol=1e-5)


def test_a_disk_in_an_object_instance(pt):
    body = ('ObjectBegin "lamp"\nShape "disk" "float radius" [.5]\n' + TRI + 'ObjectEnd\n'
            'AttributeBegin\nTranslate 1 0 0\nObjectInstance "lamp"\nAttributeEnd\n'
            'AttributeBegin\nTranslate -1 0 0\nObjectInstance "lamp"\nAttributeEnd\n')
    s = _scene(pt, body)
    d = s.desc
    assert s.errors == [] and d.n_instances == 2 and d.n_disks == 1 and d.n_tris == 1
    shapes = sorted(d.prims[i].shape for i in range(d.n_prims) if d.prims[i].instance == 0)
    assert shapes == [~0, 0]                    # the object's tree holds the disk (quadric 0: no spheres) and the triangle
    assert sum(1 for i in range(d.n_prims) if d.prims[i].instance != 0) == 2


def test_a_disk_under_an_animated_ctm_gives_the_present_error(pt):
    body = 'AttributeBegin\nActiveTransform EndTime\nTranslate 0 1 0\nActiveTransform All\nShape "%s"\nAttributeEnd\n'
    disk, sphere = _scene(pt, body % "disk"), _scene(pt, body % "sphere")
    assert len(disk.errors) == 1 and len(sphere.errors) == 1
    assert disk.errors[0] == sphere.errors[0].replace('"sphere"', '"disk"')
    assert "animated transforms of shapes are outside the hot-path scope; using the start transform" in disk.errors[0]
    assert disk.stats["n_disks"] == 1


@pytest.mark.parametrize("name", ["cylinder", "cone", "paraboloid", "hyperboloid", "curve", "nurbs", "heightfield"])
def test_the_other_shapes_are_still_reported(pt, name):
    s = _scene(pt, 'Shape "%s"\n' % name + TRI)
    assert s.errors == ['Shape "%s" is outside the PathIntegrator hot-path scope (SURVEY 2 rows 13-14); skipped.' % name]
    assert s.desc.n_prims == 1 and s.stats["n_disks"] == 0


def test_scene_cache_round_trip(pt, tmp_path):
    body = ('AttributeBegin\nAreaLightSource "diffuse" "rgb L" [1 2 3]\nRotate 20 1 0 0\nScale 1 2 .5\n'
            'Shape "disk" "float radius" [2] "float innerradius" [.5] "float phimax" [200] "float height" [.7]\nAttributeEnd\n'
            'Shape "sphere"\nAttributeBegin\nReverseOrientation\nTranslate 0 0 -2\nShape "disk"\nAttributeEnd\n' + TRI)
    s = _scene(pt, body)
    path = str(tmp_path / "scene.cache")
    s.save_cache(path)
    t = pt.Scene(cache=path)
    assert t.stats == s.stats and t.desc.n_disks == 2 and t.desc.abi_version == 15
    for i in range(2):
        a, b = s.desc.disks[i], t.desc.disks[i]
        assert bytes(a) == bytes(b)
    assert [t.desc.prims[i].shape for i in range(t.desc.n_prims)] == [s.desc.prims[i].shape for i in range(s.desc.n_prims)]
    assert t.desc.lights[0].shape == s.desc.lights[0].shape == ~1
    # a cache whose disk count disagrees with its array is refused
    raw = bytearray(open(path, "rb").read())
    off = 8 + 16 + type(s.desc).n_disks.offset
    assert int.from_bytes(raw[off:off + 4], "little") == 2
    raw[off:off + 4] = (3).to_bytes(4, "little")
    bad = str(tmp_path / "bad.cache")
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(RuntimeError):
        pt.Scene(cache=bad)
