"""Camera "orthographic" and Camera "environment" in the front end (no GPU): the switch MIPT_CAMERAS=all, the record, the
scene cache. Without the switch both stay the reported errors they were; on a build without the two cameras only that
assertion passes, every other test here fails with s.errors != []."""
import ctypes as C

import numpy as np
import pytest

import camera_models as cmod

HEAD = ('%(xform)sCamera "%(camera)s" %(params)s\nFilm "image" "integer xresolution" [%(xres)d] "integer yresolution" [%(yres)d]\n'
        'Sampler "halton" "integer pixelsamples" [4]\nIntegrator "path" "integer maxdepth" [1]\nWorldBegin\n'
        'LightSource "point" "rgb I" [1 1 1]\nShape "sphere" "float radius" [.5]\nWorldEnd\n')
TODAY = 'Camera "%s" is outside the hot-path scope (SURVEY 2 row 25); using perspective.'


def _text(camera, params="", xform="", xres=16, yres=8):
    return HEAD % dict(camera=camera, params=params, xform=xform, xres=xres, yres=yres)


@pytest.fixture
def on(monkeypatch):
    monkeypatch.setenv("MIPT_CAMERAS", "all")


def _raster_to_camera(screen, res):
    """Inverse(Orthographic(0, 1)) * Inverse(Scale(res) * Scale(1 / (x1 - x0), 1 / (y0 - y1), 1) * Translate(-x0, -y1, 0)) in
    closed form: x = x0 + px (x1 - x0) / xres, y = y1 - py (y1 - y0) / yres, z unchanged."""
    x0, x1, y0, y1 = screen
    return np.array([[(x1 - x0) / res[0], 0, 0, x0], [0, (y0 - y1) / res[1], 0, y1], [0, 0, 1, 0], [0, 0, 0, 1]])


@pytest.mark.parametrize("camera", ["orthographic", "environment"])
def test_without_the_switch_both_stay_todays_error(pt, monkeypatch, camera):
    for value in (None, "1", "none"):
        if value is None:
            monkeypatch.delenv("MIPT_CAMERAS", raising=False)
        else:
            monkeypatch.setenv("MIPT_CAMERAS", value)
        s = pt.Scene(text=_text(camera, '"float ipd" [.065]' if camera == "environment" else ""))
        assert s.errors == [TODAY % camera]
        assert s.desc.camera_type == 0 and s.desc.abi_version == 15


@pytest.mark.parametrize("camera", ["orthographic", "environment", "perspective"])
def test_without_the_switch_the_new_fields_hold_the_defaults(pt, monkeypatch, camera):
    monkeypatch.delenv("MIPT_CAMERAS", raising=False)
    d = pt.Scene(text=_text(camera, '"float ipd" [.065]' if camera == "environment" else "")).desc
    assert d.camera_type == 0
    assert (d.env_ipd, d.env_pole_merge_to, d.env_pole_merge_from) == (0, 90, 90) and np.isinf(d.env_convergence_distance)


@pytest.mark.parametrize("camera", ["omni", "realisticEye"])
def test_the_gsl_cameras_stay_errors_with_the_switch(pt, on, camera):
    s = pt.Scene(text=_text(camera))
    assert s.errors == [TODAY % camera] and s.desc.camera_type == 0


def test_orthographic_record(pt, on):
    s = pt.Scene(text=_text("orthographic", '"float fov" [30]'))
    d = s.desc
    assert s.errors == [] and d.camera_type == pt.CAMERA_ORTHOGRAPHIC == 2 and d.abi_version == 15 and not d.lens
    got = np.array(list(d.camera.raster_to_camera), np.float64).reshape(4, 4)
    assert np.allclose(got, _raster_to_camera((-2, 2, -1, 1), (16, 8)), atol=1e-6)         # frame 16 / 8; "fov" is not read
    assert d.camera.lens_radius == 0 and d.camera.focal_distance == 1e6
    assert (d.camera.shutter_open, d.camera.shutter_close, d.camera.animated) == (0, 1, 0)
    assert (d.env_ipd, d.env_pole_merge_to, d.env_pole_merge_from) == (0, 90, 90) and np.isinf(d.env_convergence_distance)
    # screenwindow, frameaspectratio, the lens and the shutter through the code the perspective camera uses
    s = pt.Scene(text=_text("orthographic", '"float screenwindow" [-3 1 -.5 2] "float lensradius" [.3] "float focaldistance" [4] '
                                            '"float shutteropen" [.9] "float shutterclose" [.2]', xres=12, yres=20))
    d = s.desc
    assert s.errors == [] and s.warnings == ["Shutter close time < shutter open. Swapping them."]
    got = np.array(list(d.camera.raster_to_camera), np.float64).reshape(4, 4)
    assert np.allclose(got, _raster_to_camera((-3, 1, -.5, 2), (12, 20)), atol=1e-6)
    assert d.camera.lens_radius == np.float32(.3) and d.camera.focal_distance == 4
    assert (d.camera.shutter_open, d.camera.shutter_close) == (np.float32(.2), np.float32(.9))
    s = pt.Scene(text=_text("orthographic", '"float frameaspectratio" [.5]'))
    got = np.array(list(s.desc.camera.raster_to_camera), np.float64).reshape(4, 4)
    assert np.allclose(got, _raster_to_camera((-1, 1, -2, 2), (16, 8)), atol=1e-6)


def test_environment_record(pt, on):
    s = pt.Scene(text=_text("environment", xres=32, yres=16))
    d = s.desc
    assert s.errors == [] and d.camera_type == pt.CAMERA_ENVIRONMENT == 3 and d.abi_version == 15 and not d.lens
    assert (d.env_ipd, d.env_pole_merge_to, d.env_pole_merge_from) == (0, 90, 90) and np.isinf(d.env_convergence_distance)
    assert d.camera.lens_radius == 0
    s = pt.Scene(text=_text("environment", '"float ipd" [.065] "float poleMergeAngleTo" [1.2] "float poleMergeAngleFrom" [.6] '
                                           '"float convergencedistance" [3] "float lensradius" [.25] "float focaldistance" [2] '
                                           '"float screenwindow" [-1 1 -1 1] "float frameaspectratio" [1]', xres=32, yres=16))
    d = s.desc
    assert s.errors == [] and d.camera_type == 3
    assert (d.env_ipd, d.env_pole_merge_to, d.env_pole_merge_from, d.env_convergence_distance) == (np.float32(.065), np.float32(1.2), np.float32(.6), 3)
    assert d.camera.lens_radius == 0          # parsed and unused: the camera sample's lens dimensions are not evaluated
    cam = cmod.Camera(s)
    assert cam.kind == cmod.ENVIRONMENT and cam.full_res == (32, 16) and cam.ipd == np.float32(.065)


@pytest.mark.parametrize("camera", ["orthographic", "environment"])
def test_the_reference_s_screenwindow_error(pt, on, camera):
    s = pt.Scene(text=_text(camera, '"float screenwindow" [-1 1 -1]'))
    assert s.errors == ['"screenwindow" should have four values'] and s.desc.camera_type in (2, 3)


@pytest.mark.parametrize("camera", ["orthographic", "environment"])
def test_warnings_and_the_animated_pair(pt, on, camera):
    """The HasScale warning and the animated CameraToWorld pair apply as they do to the perspective camera."""
    s = pt.Scene(text=_text(camera, xform="Scale 1 2 1\n"))
    assert s.errors == [] and "Scaling detected in world-to-camera transformation!" in s.warnings
    moving = ('TransformTimes 0 1\nActiveTransform StartTime\nLookAt 0 1 5  0 0 0  0 1 0\nActiveTransform EndTime\n'
              'LookAt 1 1 5  0 0 0  0 1 0\nActiveTransform All\n')
    s = pt.Scene(text=_text(camera, xform=moving))
    twin = pt.Scene(text=cmod.twin_text(_text(camera, xform=moving)))
    assert s.errors == [] and s.desc.camera.animated == 1 and twin.desc.camera.animated == 1
    for name in ("camera_to_world", "camera_to_world_end", "T", "R", "S"):
        assert bytes(getattr(s.desc.camera, name)) == bytes(getattr(twin.desc.camera, name)), name


@pytest.mark.parametrize("camera", ["orthographic", "environment"])
def test_scene_cache_round_trip(pt, on, tmp_path, camera):
    params = ('"float ipd" [.065] "float poleMergeAngleTo" [1.2] "float poleMergeAngleFrom" [.6] "float convergencedistance" [3]'
              if camera == "environment" else '"float lensradius" [.3] "float focaldistance" [4]')
    s = pt.Scene(text=_text(camera, params, xform="LookAt 0 1 5  0 0 0  0 1 0\n"))
    assert s.errors == []
    path = str(tmp_path / "scene.cache")
    s.save_cache(path)
    t = pt.Scene(cache=path)
    a, b = s.desc, t.desc
    assert b.camera_type == a.camera_type == (3 if camera == "environment" else 2) and b.abi_version == 15
    assert bytes(a.camera) == bytes(b.camera)
    for name in ("env_ipd", "env_pole_merge_to", "env_pole_merge_from", "env_convergence_distance"):
        assert getattr(a, name) == getattr(b, name), name
    # the file keeps being refused when its sizes or its camera type disagree with the build: the host library's own check
    raw = bytearray(open(path, "rb").read())
    off = 8 + 16 + type(a).camera_type.offset
    assert int.from_bytes(raw[off:off + 4], "little") == a.camera_type
    forged = bytearray(raw)
    forged[off:off + 4] = (4).to_bytes(4, "little")
    bad = str(tmp_path / "forged.cache")
    open(bad, "wb").write(bytes(forged))
    with pytest.raises(RuntimeError, match="truncated or inconsistent"):
        pt.Scene(cache=bad)
    assert int.from_bytes(raw[12:16], "little") == C.sizeof(pt.SceneDesc)            # magic, ABI, sizeof(mi_scene_desc)
    shorter = bytearray(raw)
    shorter[12:16] = (C.sizeof(pt.SceneDesc) - 16).to_bytes(4, "little")             # the record before the four fields
    open(bad, "wb").write(bytes(shorter))
    with pytest.raises(RuntimeError, match="not a scene cache of this build"):
        pt.Scene(cache=bad)


def test_the_python_mirror_matches_the_record(pt):
    """The four appended floats close mi_scene_desc: the mirror's size is the one the cache header records (checked above) and
    the fields sit behind `motions`."""
    d = pt.SceneDesc
    assert d.env_ipd.offset == d.motions.offset + C.sizeof(C.c_void_p)
    assert C.sizeof(d) == d.env_convergence_distance.offset + 4
