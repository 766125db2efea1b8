"""The numpy restatement of Camera "orthographic" and Camera "environment" (camera_models.py) against closed forms. No GPU.
The scenes are loaded with MIPT_CAMERAS=all: on a build without the two cameras every test here fails with s.errors != []."""
import math

import numpy as np
import pytest

import camera_models as cmod

HEAD = ('%(xform)sCamera "%(camera)s" %(params)s\nFilm "image" "integer xresolution" [%(xres)d] "integer yresolution" [%(yres)d]\n'
        'Sampler "halton" "integer pixelsamples" [%(spp)d]\nIntegrator "path" "integer maxdepth" [1]\nWorldBegin\n'
        'Shape "sphere" "float radius" [.5]\nWorldEnd\n')


def _camera(pt, monkeypatch, camera, params="", xform="", xres=16, yres=8, spp=4):
    monkeypatch.setenv("MIPT_CAMERAS", "all")
    s = pt.Scene(text=HEAD % dict(camera=camera, params=params, xform=xform, xres=xres, yres=yres, spp=spp))
    assert s.errors == [], s.errors
    return cmod.Camera(s)


def _grid(xres, yres, offset=(.25, .75)):
    return np.array([(x + offset[0], y + offset[1]) for y in range(yres) for x in range(xres)], np.float32)


@pytest.mark.parametrize("window", ["default", "screenwindow"])
def test_orthographic_rays_are_parallel_and_evenly_spaced(pt, monkeypatch, window):
    """Without a lens every ray points along +z of the camera (here the identity: world +z), and neighbouring film points
    are the screen window divided by the resolution apart."""
    params = '"float screenwindow" [-3 1 -.5 2]' if window == "screenwindow" else ""
    cam = _camera(pt, monkeypatch, "orthographic", params)
    assert cam.kind == cmod.ORTHOGRAPHIC and cam.lens_radius == 0
    sw = (-3, 1, -.5, 2) if window == "screenwindow" else (-2, 2, -1, 1)       # frame aspect 16 / 8 = 2
    p = _grid(16, 8)
    zero = np.zeros(len(p), np.float32)
    for f in (np.float32, np.float64):
        r = cmod.orthographic(cam, p, None, zero, f)
        assert np.all(r["d"] == np.array([0, 0, 1], f)) and np.all(r["weight"] == 1) and np.all(np.isinf(r["t_max"]))
        o = r["o"].reshape(8, 16, 3).astype(np.float64)
        tol = 1e-6 if f is np.float32 else 1e-12
        assert np.allclose(o[:, 1:, 0] - o[:, :-1, 0], (sw[1] - sw[0]) / 16, atol=tol * 4)
        assert np.allclose(o[1:, :, 1] - o[:-1, :, 1], -(sw[3] - sw[2]) / 8, atol=tol * 4)
        assert np.allclose(o[0, 0, :2], [sw[0] + .25 * (sw[1] - sw[0]) / 16, sw[3] - .75 * (sw[3] - sw[2]) / 8], atol=tol * 4)
        assert np.all(o[..., 2] == 0)


def test_orthographic_offset_origins_differ_by_dx_camera(pt, monkeypatch):
    """rxOrigin - o = dxCamera and ryOrigin - o = dyCamera exactly (1 spp: ScaleDifferentials(1) changes nothing, and the
    window's steps are powers of two), with the offset directions equal to d."""
    cam = _camera(pt, monkeypatch, "orthographic", spp=1)
    p = _grid(16, 8, (.5, .5))
    r = cmod.orthographic(cam, p, None, np.zeros(len(p), np.float32), np.float32)
    assert np.all(r["dx_camera"] == np.array([.25, 0, 0], np.float32)) and np.all(r["dy_camera"] == np.array([0, -.25, 0], np.float32))
    assert np.array_equal(r["diffs"][0] - r["o"], r["dx_camera"]) and np.array_equal(r["diffs"][1] - r["o"], r["dy_camera"])
    assert np.array_equal(r["diffs"][2], r["d"]) and np.array_equal(r["diffs"][3], r["d"])


def test_orthographic_lens_moves_every_origin_to_the_lens_disk(pt, monkeypatch):
    """With a lens the origin is the lens point alone -- inside the disk of the lens radius about the camera's origin,
    whatever the film point -- and the ray passes through pCamera + (0, 0, focalDistance)."""
    cam = _camera(pt, monkeypatch, "orthographic", '"float lensradius" [.3] "float focaldistance" [4]')
    rng = np.random.default_rng(2)
    p = _grid(16, 8)
    u = rng.random((len(p), 2)).astype(np.float32)
    r = cmod.orthographic(cam, p, u, np.zeros(len(p), np.float32), np.float64)
    o, d = r["camera_o"], r["camera_d"]          # (in camera space: the world origin has moved along d by its error bound)
    assert np.all(np.hypot(o[:, 0], o[:, 1]) <= .3 + 1e-6) and np.all(o[:, 2] == 0)
    assert np.hypot(o[:, 0], o[:, 1]).max() > .2 and np.abs(r["o"] - o).max() < 1e-6
    t = 4 / d[:, 2]
    focus = o + d * t[:, None]
    assert np.allclose(focus, r["p_camera"] + np.array([0, 0, 4.0]), atol=1e-6)
    # the offset rays start at the same lens point
    assert np.array_equal(r["diffs"][0], r["diffs"][1])


def test_environment_directions(pt, monkeypatch):
    """Unit length everywhere; pFilm = (0, H / 2) looks along +x and row 0 along +y (the fork's axis swap: y is up)."""
    cam = _camera(pt, monkeypatch, "environment", xres=32, yres=16)
    assert cam.kind == cmod.ENVIRONMENT and cam.ipd == 0 and cam.merge_to == 90 and cam.merge_from == 90 and np.isinf(cam.convergence)
    p = np.concatenate([_grid(32, 16), np.array([[0, 8], [5.5, 0], [31.25, 0]], np.float32)])
    for f, tol in ((np.float32, 2e-7), (np.float64, 1e-7)):     # (float64: Pi is the float32 constant, 8.7e-8 off)
        r = cmod.environment(cam, p, None, np.zeros(len(p), np.float32), f)
        assert np.allclose(np.linalg.norm(r["d"].astype(np.float64), axis=1), 1, atol=tol)
        assert np.allclose(r["d"][-3], [1, 0, 0], atol=tol)
        assert np.array_equal(r["d"][-2], np.array([0, 1, 0], f)) and np.array_equal(r["d"][-1], np.array([0, 1, 0], f))
        assert np.all(r["o"] == 0) and np.all(r["weight"] == 1)
    # the azimuth runs from +x over +z: a quarter of the width looks along +z
    r = cmod.environment(cam, np.array([[8, 8]], np.float32), None, np.zeros(1, np.float32), np.float64)
    assert np.allclose(r["d"][0], [0, 0, 1], atol=1e-7)


def test_omnistereo_origins_lie_on_the_ipd_circle(pt, monkeypatch):
    """ipd set, parallel convergence, default pole-merge angles (90, compared with an altitude in radians: never reached): the
    origins lie on the circle of radius ipd in the plane y = 0, perpendicular to d, and d is the mono camera's (all in camera
    space: CameraToWorld, the identity here, still moves a world origin along d by its error bound)."""
    cam = _camera(pt, monkeypatch, "environment", '"float ipd" [.065]', xres=32, yres=16)
    mono = _camera(pt, monkeypatch, "environment", xres=32, yres=16)
    p = _grid(32, 16)
    zero = np.zeros(len(p), np.float32)
    r, m = cmod.environment(cam, p, None, zero, np.float64), cmod.environment(mono, p, None, zero, np.float64)
    assert np.all(r["branch"] == 0)
    assert np.allclose(np.linalg.norm(r["camera_o"], axis=1), float(np.float32(.065)), atol=1e-9) and np.all(r["camera_o"][:, 1] == 0)
    assert np.allclose((r["camera_o"] * r["camera_d"]).sum(axis=1), 0, atol=1e-9)
    assert np.array_equal(r["camera_d"], m["camera_d"])
    # d == up exactly: no side vector, the origin stays at 0
    top = cmod.environment(cam, np.array([[3.5, 0]], np.float32), None, np.zeros(1, np.float32), np.float32)
    assert top["branch"][0] & 4 and np.all(top["camera_o"] == 0)


def test_pole_merge_fades_the_offset_to_zero(pt, monkeypatch):
    """poleMergeAngleFrom .6, poleMergeAngleTo 1.2 (radians, as the code compares them) against |asin(d.z)| of the swapped
    direction -- the angle off the plane z = 0, not off the horizon: full offset below .6, cos(fac Pi / 2) between, 0 beyond."""
    cam = _camera(pt, monkeypatch, "environment", '"float ipd" [.065] "float poleMergeAngleFrom" [.6] "float poleMergeAngleTo" [1.2]', xres=32, yres=16)
    p = _grid(32, 16)
    r = cmod.environment(cam, p, None, np.zeros(len(p), np.float32), np.float64)
    alt = np.abs(np.arcsin(r["camera_d"][:, 2]))
    beyond, fading, full = alt > 1.2 + 1e-6, (alt > .6 + 1e-6) & (alt < 1.2 - 1e-6), alt < .6 - 1e-6
    assert beyond.sum() > 10 and fading.sum() > 50 and full.sum() > 100
    length = np.linalg.norm(r["camera_o"], axis=1)
    ipd = float(np.float32(.065))
    assert np.all(length[beyond] == 0) and np.all(r["branch"][beyond] & 1 == 1)
    assert np.allclose(length[full], ipd, atol=1e-9)
    assert np.allclose(length[fading], ipd * np.cos((alt[fading] - .6) / .6 * math.pi / 2), atol=1e-7)
    # the horizon towards +z is "beyond" although its elevation is 0: the altitude is taken from z
    z = cmod.environment(cam, np.array([[8, 8]], np.float32), None, np.zeros(1, np.float32), np.float64)
    assert z["branch"][0] & 1 and np.all(z["camera_o"] == 0)


def test_convergence_distance_aims_at_the_mono_point(pt, monkeypatch):
    """With a finite convergence distance the ray from the displaced origin passes through convergencedistance * d0, d0 the
    mono direction, within rounding."""
    cam = _camera(pt, monkeypatch, "environment", '"float ipd" [.065] "float convergencedistance" [3]', xres=32, yres=16)
    mono = _camera(pt, monkeypatch, "environment", xres=32, yres=16)
    p = _grid(32, 16)
    zero = np.zeros(len(p), np.float32)
    for f, tol in ((np.float64, 1e-9), (np.float32, 2e-6)):
        r, m = cmod.environment(cam, p, None, zero, f), cmod.environment(mono, p, None, zero, f)
        target = 3.0 * m["camera_d"].astype(np.float64)
        o, d = r["camera_o"].astype(np.float64), r["camera_d"].astype(np.float64)
        t = ((target - o) * d).sum(axis=1)
        assert np.all(t > 2.9)
        assert np.abs(o + d * t[:, None] - target).max() < tol
        assert np.allclose(np.linalg.norm(o, axis=1), float(np.float32(.065)), atol=1e-7)


def test_time_and_camera_to_world(pt, monkeypatch):
    """time = Lerp(u, shutterOpen, shutterClose) in float32, and the ray is carried by CameraToWorld: a translated camera's
    origins move with it, with the origin's error bound added along d (Transform::operator()(Ray))."""
    cam = _camera(pt, monkeypatch, "orthographic", '"float shutteropen" [.2] "float shutterclose" [.9]', xform="Translate 1 2 3\n")
    p = _grid(16, 8)
    u = np.linspace(0, 1, len(p), endpoint=False).astype(np.float32)
    r = cmod.orthographic(cam, p, None, u, np.float64)
    assert np.array_equal(r["time"], (np.float32(1) - u) * np.float32(.2) + u * np.float32(.9)) and r["time"].dtype == np.float32
    # CameraToWorld = Inverse(Translate(1, 2, 3))
    assert np.allclose(r["o"] - r["p_camera"], [-1, -2, -3], atol=1e-5) and np.all(r["d"] == [0, 0, 1])
    assert np.all(r["o"][:, 2] > -3) and np.all(np.isfinite(r["t_max"]) == False)
