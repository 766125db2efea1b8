"""Camera "realistic" in the front end (no GPU): parameters, the lens table, the focus, the exit-pupil boxes, the scene cache.
realistic_camera.py restates the reference's camera (src/cameras/realistic.cpp) and says which lines each function follows."""
import os

import numpy as np
import pytest

import realistic_camera as rc


def _scene(pt, lens, params="", film='"float diagonal" [35]', res=(32, 32), base_dir=None):
    path = lens if (os.sep in lens or base_dir) else rc.lens_path(lens)
    text = ('LookAt 0 0 5  0 0 0  0 1 0\nCamera "realistic" %s %s\n'
            'Film "image" "integer xresolution" [%d] "integer yresolution" [%d] %s\n'
            'Sampler "halton" "integer pixelsamples" [4]\nWorldBegin\nShape "sphere"\nWorldEnd\n'
            % ('"string lensfile" "%s"' % path if lens else "", params, res[0], res[1], film))
    return pt.Scene(text=text, base_dir=base_dir)


def _lens(scene):
    c = scene.desc.camera
    assert scene.desc.camera_type == 1 and bool(scene.desc.lens)
    return scene.desc.lens.contents


def _table(scene):
    L = _lens(scene)
    return np.array([[L.elements[i][k] for k in range(4)] for i in range(L.n_elements)], np.float32)


def _boxes(scene):
    L = _lens(scene)
    return np.array([[L.exit_pupil_bounds[i][k] for k in range(4)] for i in range(64)], np.float32)


@pytest.fixture(scope="module")
def dgauss(pt):
    s = _scene(pt, "dgauss.dat", '"float aperturediameter" [8] "float focusdistance" [5] "bool chromaticAberrationEnabled" "true"')
    assert s.errors == []
    return s


# ---------------------------------------------------------------------------------------------------------------------
# 1: parsing and the table
def test_defaults_and_the_scaled_table(pt):
    s = _scene(pt, "dgauss.dat", '"float filmdistance" [0.04]', film="")
    assert s.errors == []
    c, L = s.desc.camera, _lens(s)
    assert (L.simple_weighting, L.no_weighting, L.chromatic_aberration) == (1, 0, 0)
    assert (c.shutter_open, c.shutter_close) == (0.0, 1.0) and c.animated == 0
    assert L.n_elements == 11 and list(L.full_res) == [32, 32]
    f32 = np.float32
    raw = np.array([float(v) for line in open(rc.lens_path("dgauss.dat")) if not line.startswith("#") for v in line.split()], f32).reshape(-1, 4)
    t = _table(s)
    # mm -> m, diameter -> radius (realistic.cpp:145-147); the stop takes "aperturediameter" (default 1.0 mm)
    assert np.array_equal(t[:, 0], raw[:, 0] * f32(.001)) and np.array_equal(t[:-1, 1], raw[:-1, 1] * f32(.001))
    assert np.array_equal(t[:, 2], raw[:, 2])
    want_ap = raw[:, 3].copy()
    want_ap[5] = f32(1.0)
    assert raw[5, 0] == 0 and np.array_equal(t[:, 3], want_ap * f32(.001) / f32(2))
    # "filmdistance" sets the last thickness directly, and callers read it
    assert t[-1, 1] == f32(0.04) == f32(L.film_distance)
    # Film "diagonal" defaults to 35 mm: Film::diagonal and GetPhysicalExtent (film.cpp:54, 94-99)
    assert f32(L.film_diagonal) == f32(np.float64(f32(35.)) * .001)
    x = np.sqrt(f32(L.film_diagonal) * f32(L.film_diagonal) / (f32(1) + f32(1) * f32(1)))
    assert list(L.physical_extent) == [-x / 2, -x / 2, x / 2, x / 2]
    # raster_to_camera keeps a defined value, and the camera sample's lens dimensions are on
    assert np.all(np.isfinite(list(c.raster_to_camera))) and any(c.raster_to_camera) and c.lens_radius > 0
    assert any("simpleweighting" in w for w in s.warnings)


def test_every_parameter_is_read(pt):
    s = _scene(pt, "dgauss.dat", '"float aperturediameter" [6] "float focusdistance" [3] "bool simpleweighting" "false" "bool noweighting" "true" '
               '"bool chromaticAberrationEnabled" "true" "float shutteropen" [.75] "float shutterclose" [.25]',
               film='"float diagonal" [20]', res=(48, 32))
    assert s.errors == []
    c, L = s.desc.camera, _lens(s)
    assert (L.simple_weighting, L.no_weighting, L.chromatic_aberration) == (0, 1, 1)
    assert (c.shutter_open, c.shutter_close) == (0.25, 0.75) and any("Swapping" in w for w in s.warnings)
    assert _table(s)[5, 3] == np.float32(6) * np.float32(.001) / np.float32(2)
    assert not any("simpleweighting" in w for w in s.warnings)
    f32 = np.float32
    assert f32(L.film_diagonal) == f32(np.float64(f32(20.)) * .001) != f32(20.) * f32(.001)   # (a double product rounded once)
    aspect = f32(32) / f32(48)
    x = np.sqrt(f32(L.film_diagonal) * f32(L.film_diagonal) / (f32(1) + aspect * aspect))
    y = aspect * x
    assert list(L.physical_extent) == [-x / 2, -y / 2, x / 2, y / 2]
    # focused by FocusThickLens: another focus distance, another film distance
    far = _scene(pt, "dgauss.dat", '"float aperturediameter" [6] "float focusdistance" [30]', film='"float diagonal" [20]', res=(48, 32))
    assert 0 < _lens(far).film_distance < L.film_distance < 0.06


def test_aperture_clamp_warning(pt):
    s = _scene(pt, "dgauss.dat", '"float aperturediameter" [40] "float filmdistance" [0.04]')
    assert s.errors == []
    assert any("Specified aperture diameter 40.000000 is greater than maximum possible 17.100000.  Clamping it." in w for w in s.warnings)
    assert _table(s)[5, 3] == np.float32(17.1) * np.float32(.001) / np.float32(2)


def test_value_count_rules_and_errors(pt, tmp_path):
    rows = "50 5 1.5 20\n-50 2 1 20\n0 45 0 10\n"
    (tmp_path / "plus1.dat").write_text("# v2 style: focal length first\n50.8\n" + rows)
    (tmp_path / "plus2.dat").write_text(rows + "1 2\n")
    s = _scene(pt, str(tmp_path / "plus1.dat"))
    assert s.errors == [] and any("Extra value in lens specification file" in w for w in s.warnings)
    assert _lens(s).n_elements == 3 and _table(s)[0, 0] == np.float32(50) * np.float32(.001)
    ref = _scene(pt, "biconvex.dat")
    assert np.array_equal(_table(s), _table(ref)) and np.array_equal(_boxes(s), _boxes(ref))
    s = _scene(pt, str(tmp_path / "plus2.dat"))
    assert any("must be multiple-of-four values, read 14" in e for e in s.errors) and s.desc.camera_type == 0 and not s.desc.lens
    s = _scene(pt, "")
    assert "No lens description file supplied!" in s.errors
    s = _scene(pt, str(tmp_path / "missing.dat"))
    assert any("Error reading lens specification file" in e and "missing.dat" in e for e in s.errors)
    # a relative name is looked up beside the scene file
    s = _scene(pt, "plus1.dat", base_dir=str(tmp_path))
    assert s.errors == [] and _lens(s).n_elements == 3
    # a focus distance inside the focal length: the reference's CHECK is this scene's error, not an abort
    s = _scene(pt, "biconvex.dat", '"float focusdistance" [0.1]')
    assert any("Coefficient must be positive" in e and "too short" in e for e in s.errors)
    # a stop alone has no focal length to focus with ...
    s = _scene(pt, "stop_only.dat")
    assert any("Coefficient must be positive" in e for e in s.errors)
    # ... and renders with a film distance
    s = _scene(pt, "stop_only.dat", '"float filmdistance" [0.05]')
    assert s.errors == [] and _lens(s).n_elements == 1


@pytest.mark.parametrize("camera", ["orthographic", "environment", "omni", "realisticEye"])
def test_other_cameras_stay_errors(pt, camera):
    s = pt.Scene(text='Camera "%s"\nFilm "image" "integer xresolution" [8] "integer yresolution" [8]\nWorldBegin\nShape "sphere"\nWorldEnd\n' % camera)
    assert any('Camera "%s" is outside the hot-path scope' % camera in e for e in s.errors)
    assert s.desc.camera_type == 0


# ---------------------------------------------------------------------------------------------------------------------
# 2: known-answer optics on the biconvex element
def test_biconvex_focal_length_and_focus(pt):
    """biconvex.dat: R1 = 50 mm, R2 = -50 mm, d = 5 mm, n = 1.5, the stop 2 mm behind the rear vertex.

    The host measures its cardinal points with one ray parallel to the axis at height h = .001 * diagonal (realistic.cpp:659),
    so its focal length differs from the paraxial one by that ray's spherical aberration. Third-order value for a thin lens
    (Jenkins & White, Fundamentals of Optics, eq. 9m) with shape factor q = (R2 + R1) / (R2 - R1) = 0 and position factor
    p = -1 (object at infinity):
        1 / s'_h - 1 / s'_p = h^2 / (8 f^3) * 1 / (n (n - 1)) * [(n + 2) / (n - 1) q^2 + 4 (n + 1) p q + (3 n + 2)(n - 1) p^2 + n^3 / (n - 1)]
                            = h^2 / (8 f^3) * (1 / 0.75) * [3.25 + 6.75] = (5 / 3) h^2 / f^3,
    a longitudinal shift of f^2 times that: LSA = (5 / 3) h^2 / f. The film is 500 mm across here so that h = 0.5 mm: LSA =
    8.19e-6 m, against 3e-7 m of float32 rounding in a ray whose slope is h / f = 0.01 (at the default 35 mm the ray is so
    close to the axis that rounding, 7e-7 m, hides its 4e-8 m of aberration). Measured: f_host - f_formula = -6.51e-6 m
    (the marginal ray focuses short, as it must), film distance - Gaussian value = -7.74e-6 m."""
    n, R1, R2, d, gap, D = 1.5, .050, -.050, .005, .002, 2.0
    s = _scene(pt, "biconvex.dat", '"float focusdistance" [%g]' % D, film='"float diagonal" [500]')
    assert s.errors == []
    L = _lens(s)
    f = 1 / ((n - 1) * (1 / R1 - 1 / R2 + (n - 1) * d / (n * R1 * R2)))
    h = .001 * .5
    lsa = (5. / 3.) * h * h / f
    f_host = L.thick_lens_fz[0] - L.thick_lens_pz[0]
    # Gaussian imaging about the principal planes: H lies f (n - 1) d / (n |R2|) behind the front vertex, H' as far in front
    # of the rear vertex; the object is D in front of the film, so s + HH' + s' = D with 1 / s + 1 / s' = 1 / f
    h1, h2 = f * (n - 1) * d / (n * -R2), f * (n - 1) * d / (n * R1)
    span = D - (d - h1 - h2)
    s_img = (span - np.sqrt(span * span - 4 * f * span)) / 2
    film_distance = s_img - h2 - gap          # from the stop, the last interface, to the film
    print("biconvex: f host %.9f formula %.9f (difference %.3e), film distance host %.9f Gaussian %.9f (difference %.3e), bar %.3e"
          % (f_host, f, f_host - f, L.film_distance, film_distance, L.film_distance - film_distance, lsa))
    assert abs(f_host - f) <= lsa
    assert abs(L.film_distance - film_distance) <= lsa


# ---------------------------------------------------------------------------------------------------------------------
# 3: exit-pupil boxes
@pytest.mark.parametrize("interval", [0, 31, 63])
def test_exit_pupil_boxes(dgauss, interval):
    """The host's box against the float32 restatement over the same 1024^2 points: equal, except that a point whose verdict
    differs between the float32 and float64 restatements may move an edge by at most one sample spacing."""
    host = _boxes(dgauss)[interval]
    ok32, pts, spacing = rc.exit_pupil_points(rc.Lens(dgauss, np.float32), interval)
    ok64, _, _ = rc.exit_pupil_points(rc.Lens(dgauss, np.float64), interval)
    box32 = rc.box_of(pts, ok32, rc.Lens(dgauss))
    unsure = ok32 != ok64
    print("interval %d: %d of %d points get through, %d verdicts differ between float32 and float64; host %s restated %s"
          % (interval, int(ok32.sum()), len(ok32), int(unsure.sum()), host, box32))
    assert ok32.any() and not ok32.all()
    if np.array_equal(host, box32):
        return
    assert unsure.any() and float(np.abs(host.astype(np.float64) - box32).max()) <= spacing
    both = rc.box_of(pts, ok32 | ok64, rc.Lens(dgauss)), rc.box_of(pts, ok32 & ok64, rc.Lens(dgauss))
    assert np.all(host[:2] >= both[0][:2]) and np.all(host[2:] <= both[0][2:])
    assert np.all(host[:2] <= both[1][:2]) and np.all(host[2:] >= both[1][2:])


def test_boxes_when_nothing_gets_through(pt):
    """A film far wider than the lens can serve: the outer intervals keep the whole projected rear bounds."""
    s = _scene(pt, "dgauss.dat", '"float aperturediameter" [4] "float filmdistance" [0.0368]', film='"float diagonal" [400]')
    assert s.errors == []
    t = _table(s)
    rear = np.float32(1.5) * t[-1, 3]
    assert list(_boxes(s)[63]) == [-rear, -rear, rear, rear]
    assert list(_boxes(s)[0]) != [-rear, -rear, rear, rear]


# ---------------------------------------------------------------------------------------------------------------------
# 4: scene cache
def test_scene_cache_round_trip(pt, dgauss, tmp_path):
    path = str(tmp_path / "lens.cache")
    dgauss.save_cache(path)
    back = pt.Scene(cache=path)
    a, b = _lens(dgauss), _lens(back)
    assert back.desc.camera_type == 1 and back.desc.camera.lens_radius == dgauss.desc.camera.lens_radius
    assert bytes(a) == bytes(b)                     # table, boxes, flags, extent, diagonal: the whole record
    assert b.chromatic_aberration == 1 and b.n_elements == 11
    assert np.array_equal(_table(dgauss), _table(back)) and np.array_equal(_boxes(dgauss), _boxes(back))
    # a perspective scene's cache carries no lens
    p = pt.Scene(text='Camera "perspective"\nFilm "image" "integer xresolution" [8] "integer yresolution" [8]\nWorldBegin\nShape "sphere"\nWorldEnd\n')
    p.save_cache(path)
    assert not pt.Scene(cache=path).desc.lens and pt.Scene(cache=path).desc.camera_type == 0
