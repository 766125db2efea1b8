"""The moving camera in the front end: the CTM pair and its active bits, TransformTimes, CameraToWorld as an
AnimatedTransform in mi_camera (ABI v12), what is reported under an animated CTM, and the scene cache."""
import numpy as np

import camera_motion as cm

START = "3 2 8  0 0.5 0  0 1 0"
END = "6 3 5  0.5 0 -1  0.1 1 0"
FILM = 'Film "image" "integer xresolution" [8] "integer yresolution" [8]\n'
WORLD = 'WorldBegin\nLightSource "point" "point from" [0 9 0]\nShape "sphere"\nWorldEnd\n'


def _mat(a):
    return np.array(list(a), np.float32)


def _camera_fields(c):
    return {"camera_to_world": _mat(c.camera_to_world), "camera_to_world_end": _mat(c.camera_to_world_end),
            "transform_start": np.float32(c.transform_start), "transform_end": np.float32(c.transform_end),
            "animated": int(c.animated), "shutter_open": np.float32(c.shutter_open), "shutter_close": np.float32(c.shutter_close),
            "T": np.array([list(r) for r in c.T], np.float32), "R": np.array([list(r) for r in c.R], np.float32),
            "S": np.array([list(r) for r in c.S], np.float32)}


def test_a_moving_camera_is_parsed_into_the_pair_and_its_decomposition(pt):
    moving = pt.Scene(text=cm.moving_camera(START, END, (0.25, 1.5), end_extra="Scale 1 1.25 0.9\n") + FILM + WORLD)
    assert moving.errors == [] and moving.warnings == []
    start = pt.Scene(text=cm.static_camera(START) + FILM + WORLD)
    end = pt.Scene(text="Scale 1 1.25 0.9\n" + cm.static_camera(END) + FILM + WORLD)
    c = moving.desc.camera
    assert c.animated == 1 and c.transform_start == 0.25 and c.transform_end == 1.5
    # each member is computed exactly as the single transform of a static scene
    assert np.array_equal(_mat(c.camera_to_world).view(np.uint32), _mat(start.desc.camera.camera_to_world).view(np.uint32))
    assert np.array_equal(_mat(c.camera_to_world_end).view(np.uint32), _mat(end.desc.camera.camera_to_world).view(np.uint32))
    assert not np.array_equal(_mat(c.camera_to_world), _mat(c.camera_to_world_end))
    s = start.desc.camera
    assert s.animated == 0 and s.transform_start == 0 and s.transform_end == 1   # TransformTimes' defaults
    assert np.array_equal(_mat(s.camera_to_world_end), _mat(s.camera_to_world))
    # T, R, S against the float32 restatement of Decompose. Observed: the polar iteration ends after the same number of
    # steps on both sides (1 and 4 here) and every component is bit-equal; the bar of 4 ulp is the issue's.
    a = cm.animated_of(moving)
    got = _camera_fields(c)
    assert a.animated and a.steps[0] < 100 and a.steps[1] < 100
    for name, want in (("T", a.T), ("R", a.R), ("S", a.S)):
        want = np.array(want, np.float32)
        d = cm.ulp_distance(got[name], want)
        print("%s: %d ulp from the float32 restatement (polar steps %s)" % (name, d, (a.steps,)))
        assert d <= 4, (name, got[name], want)
    # and against the same mathematics in double: the decomposition is a float32 one, so a loose bar
    a64 = cm.animated_of(moving, np.float64)
    for name, want in (("T", a64.T), ("R", a64.R), ("S", a64.S)):
        assert np.allclose(got[name], np.array(want), rtol=0, atol=2e-6), name
    # T R S is the matrix again
    for k, m in enumerate((got["camera_to_world"], got["camera_to_world_end"])):
        x, y, z, w = got["R"][k].astype(np.float64)
        rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                        [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                        [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        m3 = m.reshape(4, 4).astype(np.float64)
        assert np.allclose(rot @ got["S"][k].reshape(3, 3), m3[:3, :3], atol=1e-5)
        assert np.array_equal(got["T"][k], m.reshape(4, 4)[:3, 3])


def test_r1_is_flipped_onto_the_shorter_arc(pt):
    """Two cameras whose quaternions, as Quaternion(Transform) extracts them, have a negative dot product."""
    flipped = None
    for deg in (170, 200, 250, 300):
        text = ('ActiveTransform EndTime\nRotate %d 0 1 0\nActiveTransform All\nLookAt %s\nCamera "perspective"\n' % (deg, START)
                + FILM + WORLD)
        s = pt.Scene(text=text)
        assert s.errors == [] and s.desc.camera.animated == 1
        a = cm.animated_of(s)
        c = s.desc.camera
        r0, r1 = np.array(list(c.R[0]), np.float32), np.array(list(c.R[1]), np.float32)
        assert float(np.dot(r0.astype(np.float64), r1.astype(np.float64))) >= 0     # never the long way round
        assert cm.ulp_distance(r1, np.array(a.R[1], np.float32)) <= 4
        if a.flipped:
            flipped = deg
            raw = np.array(cm.decompose(list(c.camera_to_world_end))[1], np.float32)
            assert cm.ulp_distance(r1, -raw) <= 4 and np.dot(r0, raw) < 0
    assert flipped is not None


def test_equal_members_are_not_animated(pt):
    text = ('TransformTimes 0 2\nActiveTransform StartTime\nLookAt %s\nActiveTransform EndTime\nLookAt %s\nActiveTransform All\n'
            'Camera "perspective"\n' % (START, START)) + FILM + WORLD
    s = pt.Scene(text=text)
    c = s.desc.camera
    assert s.errors == [] and c.animated == 0 and c.transform_end == 2
    assert np.array_equal(_mat(c.camera_to_world), _mat(c.camera_to_world_end))
    assert not np.array(_camera_fields(c)["R"]).any() and not np.array(_camera_fields(c)["S"]).any()


def test_every_ctm_directive_applies_to_the_active_members_only(pt):
    """Each directive once under `ActiveTransform EndTime` after a common LookAt: the start member stays the plain camera, the
    end member is the camera a static scene gets from the same directives."""
    m = "[1 0 0 0  0 1 0 0  0 0 1 0  1 2 3 1]"
    for directive in ("Translate 1 2 3", "Scale 1 2 0.5", "Rotate 20 0 1 1", "LookAt 1 0 4  0 0 0  0 1 0",
                      "ConcatTransform " + m, "Transform " + m, "Identity"):
        text = 'LookAt %s\nActiveTransform EndTime\n%s\nActiveTransform All\nCamera "perspective"\n' % (START, directive)
        s = pt.Scene(text=text + FILM + WORLD)
        plain = pt.Scene(text=cm.static_camera(START, "") + FILM + WORLD)
        both = pt.Scene(text='LookAt %s\n%s\nCamera "perspective"\n' % (START, directive) + FILM + WORLD)
        assert s.errors == [], directive
        c = s.desc.camera
        assert c.animated == 1, directive
        assert np.array_equal(_mat(c.camera_to_world), _mat(plain.desc.camera.camera_to_world)), directive
        assert np.array_equal(_mat(c.camera_to_world_end), _mat(both.desc.camera.camera_to_world)), directive


def _world_vertices(scene):
    return np.array(scene.desc.P[:3 * scene.desc.n_verts], np.float32).reshape(-1, 3)


TRI = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0  1 0 0  0 1 0]\n'
CAM = cm.static_camera(START) + FILM


def test_the_bits_are_pushed_and_popped_with_the_pair(pt):
    """Inside the block only the end member moves; after AttributeEnd / TransformEnd the bits are `All` again, so the next
    Translate moves both members and the triangle sits under a static CTM: no message, and at the translated place."""
    for begin, end in (("AttributeBegin", "AttributeEnd"), ("TransformBegin", "TransformEnd")):
        text = (CAM + 'WorldBegin\nLightSource "point"\n%s\nActiveTransform EndTime\nTranslate 5 0 0\n%s\nTranslate 0 7 0\n' % (begin, end)
                + TRI + 'WorldEnd\n')
        s = pt.Scene(text=text)
        assert s.errors == [] and s.warnings == [], (begin, s.errors, s.warnings)
        assert np.array_equal(_world_vertices(s), np.array([[0, 7, 0], [1, 7, 0], [0, 8, 0]], np.float32))
    # without the pop the second Translate would reach the end member only
    text = CAM + 'WorldBegin\nActiveTransform EndTime\nTranslate 5 0 0\nTranslate 0 7 0\n' + TRI + 'WorldEnd\n'
    s = pt.Scene(text=text)
    assert len(s.errors) == 1 and "animated" in s.errors[0]
    assert np.array_equal(_world_vertices(s), np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32))
    # WorldBegin resets the pair and the bits
    text = ('ActiveTransform EndTime\nTranslate 0 0 2\n' + cm.static_camera(START) + FILM + 'WorldBegin\nTranslate 1 0 0\n'
            + TRI + 'WorldEnd\n')
    s = pt.Scene(text=text)
    assert s.errors == [] and s.desc.camera.animated == 1
    assert np.array_equal(_world_vertices(s)[0], np.array([1, 0, 0], np.float32))


def test_coordsystransform_camera_restores_both_members(pt):
    """A light placed in camera space of a moving camera: both members come back (the CTM is animated again, which the
    LightSource warning shows), and the light sits where the START camera is."""
    text = (cm.moving_camera(START, END) + FILM + 'WorldBegin\nAttributeBegin\nCoordSysTransform "camera"\n'
            'LightSource "point" "rgb I" [1 1 1]\nAttributeEnd\nLightSource "point" "point from" [0 9 0]\n' + TRI + 'WorldEnd\n')
    s = pt.Scene(text=text)
    assert s.errors == []
    assert s.warnings == ['Animated transformations set; ignoring for "LightSource" and using the start transform only']
    assert np.array_equal(np.array(list(s.desc.lights[0].pos), np.float32), np.array([3, 2, 8], np.float32))
    # a named coordinate system stores the pair, too
    text = (CAM + 'WorldBegin\nTransformBegin\nTranslate 1 0 0\nActiveTransform EndTime\nTranslate 0 0 4\nCoordinateSystem "rig"\n'
            'TransformEnd\nCoordSysTransform "rig"\n' + TRI + 'WorldEnd\n')
    s = pt.Scene(text=text)
    assert len(s.errors) == 1 and "animated" in s.errors[0] and "Shape" in s.errors[0]
    assert np.array_equal(_world_vertices(s)[0], np.array([1, 0, 0], np.float32))


def test_shapes_and_instances_under_an_animated_ctm_are_reported(pt):
    moved = 'Translate 2 0 0\nActiveTransform EndTime\nTranslate 0 3 0\nActiveTransform All\n'
    s = pt.Scene(text=CAM + 'WorldBegin\n' + moved + TRI + 'WorldEnd\n')
    assert len(s.errors) == 1 and "animated" in s.errors[0] and "Shape" in s.errors[0]
    assert np.array_equal(_world_vertices(s), np.array([[2, 0, 0], [3, 0, 0], [2, 1, 0]], np.float32))   # the start transform
    text = (CAM + 'WorldBegin\nObjectBegin "o"\n' + TRI + 'ObjectEnd\nAttributeBegin\n' + moved + 'ObjectInstance "o"\nAttributeEnd\n'
            'WorldEnd\n')
    s = pt.Scene(text=text)
    assert len(s.errors) == 1 and "animated" in s.errors[0] and "ObjectInstance" in s.errors[0]
    assert s.desc.n_instances == 1
    i2w = np.array(list(s.desc.instances[0].i2w), np.float32).reshape(4, 4)
    assert np.array_equal(i2w[:3, 3], np.array([2, 0, 0], np.float32))
    assert np.array_equal(_world_vertices(s), np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32))   # kept in object space


def test_lights_and_textures_under_an_animated_ctm_take_the_references_warning(pt):
    moved = 'Translate 2 0 0\nActiveTransform EndTime\nTranslate 0 3 0\nActiveTransform All\n'
    text = (CAM + 'WorldBegin\nAttributeBegin\n' + moved + 'LightSource "point" "point from" [0 0 1]\n'
            'Texture "t" "spectrum" "constant" "rgb value" [.5 .5 .5]\nMakeNamedMedium "m"\nAttributeEnd\n' + TRI + 'WorldEnd\n')
    s = pt.Scene(text=text)
    assert s.errors == []
    w = 'Animated transformations set; ignoring for "%s" and using the start transform only'
    assert [m for m in s.warnings if m.startswith("Animated")] == [w % "LightSource", w % "Texture", w % "MakeNamedMedium"]
    assert np.array_equal(np.array(list(s.desc.lights[0].pos), np.float32), np.array([2, 0, 1], np.float32))


def test_transformtimes_belongs_to_the_options_block(pt):
    s = pt.Scene(text=CAM + 'WorldBegin\nTransformTimes 3 4\n' + TRI + 'WorldEnd\n')
    assert len(s.errors) == 1 and "TransformTimes" in s.errors[0]
    assert s.desc.camera.transform_start == 0 and s.desc.camera.transform_end == 1


def test_the_scene_cache_keeps_every_camera_field(pt, tmp_path):
    s = pt.Scene(text=cm.moving_camera(START, END, (0.25, 1.5), '"float fov" [30] "float shutteropen" [.1] "float shutterclose" [.9]',
                                       end_extra="Scale 1 1.25 0.9\n") + FILM + WORLD)
    assert s.errors == [] and s.desc.camera.animated == 1
    path = str(tmp_path / "scene.cache")
    s.save_cache(path)
    t = pt.Scene(cache=path)
    a, b = _camera_fields(s.desc.camera), _camera_fields(t.desc.camera)
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]).view(np.uint32) if isinstance(a[k], np.ndarray) else a[k],
                              np.asarray(b[k]).view(np.uint32) if isinstance(b[k], np.ndarray) else b[k]), k
    assert np.array_equal(_mat(s.desc.camera.raster_to_camera), _mat(t.desc.camera.raster_to_camera))
    assert a["T"].any() and a["R"].any() and a["S"].any() and a["transform_start"] == np.float32(0.25)
    assert pt.SceneDesc.camera.size == 4 * (16 + 16 + 4 + 16 + 2 + 1 + 6 + 8 + 18)   # the ctypes mirror of mi_camera
