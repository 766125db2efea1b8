"""Camera "orthographic" and Camera "environment" on the GPU (MIPT_CAMERAS=all), stage by stage. camera_models.py restates the
two cameras in float32 and float64; the unchanged oracle knows the perspective camera only, so it is only ever given the twin
of a scene (the same text with Camera "perspective") for sampler values, and ob.trace for the hits of restated rays. A sample
on which the two restatements take different branches (the pole-merge comparisons, d == up, hit or miss of the restated ray)
is "unsure" and decides nothing; each case asserts on the CPU, before the device is asked, that at most 1 % are. Bars: four
times the worst float32-against-float64 deviation of the restatement over the compared set, never below 8 ulp of the largest
component (camera_models.bar, the rule of disk_shape.bar)."""
import os

import numpy as np
import pytest

import camera_models as cmod
import camera_motion as cm
import metadata_scenes as ms

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _switch(monkeypatch):
    monkeypatch.setenv("MIPT_CAMERAS", "all")
    monkeypatch.delenv("MIPT_STREAMS", raising=False)
    monkeypatch.delenv("MIPT_DARK_STREAM", raising=False)


def _rel_l2(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / max((b ** 2).sum(), 1e-30)))


def _restated(ob, s, twin):
    """The frame's samples, their sampler values from the twin and the two restatements."""
    samples = cmod.all_samples(twin)
    p_film, time_u, p_lens = cmod.sample_values(ob, twin, samples)
    r32, r64, unsure = cmod.both(cmod.Camera(s), p_film, p_lens, time_u)
    return samples, p_film, r32, r64, unsure


def _rays_of(r):
    out = np.zeros((len(r["o"]), 7), np.float32)
    out[:, 0:3], out[:, 3:6], out[:, 6] = r["o"], r["d"], r["t_max"]
    return out


def _splat(scene, p_film, values):
    """FilmTile::AddSample with the box filter (film.h:131-141), as tests/test_disk_gpu.py splats."""
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
# 1: the probe against the restatement
PROBE_HEAD = ('%(xform)sCamera "%(camera)s" %(params)s\nFilm "image" "integer xresolution" [%(xres)d] "integer yresolution" [%(yres)d]\n'
              'Sampler "halton" "integer pixelsamples" [4]\nIntegrator "path" "integer maxdepth" [1]\nWorldBegin\n'
              'LightSource "point" "rgb I" [1 1 1] "point from" [0 5 0]\nShape "sphere" "float radius" [.5]\nWorldEnd\n')
LOOK = "LookAt 1 2 6  0 .5 0  0 1 0\n"
SKEWED = "Translate .5 -1 2\nRotate 35 1 2 .5\nScale 1 2 .5\n"            # rotated and non-uniformly scaled
MOVING = ("TransformTimes .3 .8\nActiveTransform StartTime\nLookAt 1 2 6  0 .5 0  0 1 0\nActiveTransform EndTime\n"
          "Rotate 20 0 1 0\nLookAt 2 2.5 5  0 .5 0  0 1 0\nActiveTransform All\n")
SHUTTER = ' "float shutteropen" [.2] "float shutterclose" [.9]'
ODS = '"float ipd" [.065]'
PROBES = {
    "orthographic": ("orthographic", "", LOOK, 16, 8),
    "orthographic, screenwindow and a non-square frame": ("orthographic", '"float screenwindow" [-3 1 -.5 2] "float frameaspectratio" [.7]', LOOK, 16, 8),
    "orthographic, lens": ("orthographic", '"float lensradius" [.3] "float focaldistance" [4]', LOOK, 16, 8),
    "environment": ("environment", "", LOOK, 32, 16),
    "environment, ods parallel": ("environment", ODS, LOOK, 16, 8),
    "environment, ods pole merge": ("environment", ODS + ' "float poleMergeAngleFrom" [.6] "float poleMergeAngleTo" [1.2]', LOOK, 16, 8),
    "environment, ods convergence": ("environment", ODS + ' "float convergencedistance" [3]', LOOK, 16, 8),
    "orthographic, lens, skewed CameraToWorld": ("orthographic", '"float lensradius" [.3] "float focaldistance" [4]', SKEWED, 16, 8),
    "environment, ods convergence, skewed CameraToWorld": ("environment", ODS + ' "float convergencedistance" [3]', SKEWED, 16, 8),
    "orthographic, lens, animated": ("orthographic", '"float lensradius" [.3] "float focaldistance" [4]' + SHUTTER, MOVING, 16, 8),
    "environment, ods pole merge, animated": ("environment", ODS + ' "float poleMergeAngleFrom" [.6] "float poleMergeAngleTo" [1.2]' + SHUTTER, MOVING, 16, 8),
}
COLUMNS = (("o", slice(0, 3)), ("d", slice(3, 6)), ("rxOrigin", slice(9, 12)), ("ryOrigin", slice(12, 15)), ("rxDirection", slice(15, 18)),
           ("ryDirection", slice(18, 21)))


@pytest.mark.parametrize("name", list(PROBES))
def test_probe_against_the_restatement(pt, ob, name):
    camera, params, xform, xres, yres = PROBES[name]
    s, twin = cmod.pair(pt, PROBE_HEAD % dict(camera=camera, params=params, xform=xform, xres=xres, yres=yres))
    samples, p_film, r32, r64, unsure = _restated(ob, s, twin)
    assert len(samples) == xres * yres * 4 and samples[0] == (0, 0, 0) and samples[-1][1] == yres - 1   # pixel (0, 0) sample 0, the last row
    assert unsure.mean() <= 0.01, unsure.mean()                                                    # the condition, on the CPU
    sure = ~unsure
    c32, c64 = cmod.columns(r32), cmod.columns(r64)
    if "animated" in name:
        assert s.desc.camera.animated == 1
        t = r32["time"]
        assert (t <= np.float32(.3)).any() and (t >= np.float32(.8)).any() and ((t > np.float32(.3)) & (t < np.float32(.8))).sum() > 100
    if "pole merge" in name:
        assert (r64["branch"] & 1).any() and (r64["branch"] & 2).any() and (r64["branch"] & 3 == 0).any()
    if camera == "environment" and "ods" in name and "skewed" not in name and "animated" not in name:
        assert (r64["branch"] & 4).any()                                 # d == up at pixel row 0, sample 0
    integ = pt.CreatePathIntegrator(s)
    dev = integ.camera_rays_ex(samples)
    assert dev.shape == (len(samples), 21)
    assert np.all(dev[:, 8] == 1)                                                                  # the weight, exactly
    assert np.array_equal(dev[:, 7].view(np.uint32), r32["time"].view(np.uint32))                  # the time: the restated float32
    assert np.array_equal(dev[:, 6], c32[:, 6]) and np.all(np.isinf(dev[:, 6]))                    # tMax
    for key, col in COLUMNS:
        b = cmod.bar(c32[:, col], c64[:, col], sure)
        worst = float(np.abs(dev[sure][:, col].astype(np.float64) - c64[sure][:, col]).max())
        exact = int(np.all(dev[sure][:, col] == c32[sure][:, col], axis=1).sum())
        print("%s: %s worst %.3e / bar %.3e over %d, %d bit for bit with the float32 restatement" % (name, key, worst, b, int(sure.sum()), exact))
        assert worst <= b, (name, key, worst, b)
    plain = integ.camera_rays(samples)
    assert plain.shape == (len(samples), 8) and np.array_equal(plain.view(np.uint32), dev[:, :8].view(np.uint32))
    if xform is SKEWED:
        assert "Scaling detected in world-to-camera transformation!" in s.warnings


def test_a_forged_camera_type_is_refused(pt):
    s = pt.Scene(text=PROBE_HEAD % dict(camera="orthographic", params="", xform=LOOK, xres=8, yres=8))
    assert s.errors == [] and s.desc.camera_type == 2
    for forged in (4, -1):
        s.desc.camera_type = forged
        with pytest.raises(RuntimeError, match="camera_type"):
            pt.CreatePathIntegrator(s)
    s.desc.camera_type = 2
    pt.CreatePathIntegrator(s)


# ---------------------------------------------------------------------------------------------------------------------
# 2: maps
def _quad(p0, p1, p2, p3, extra=""):
    pts = " ".join("%g %g %g" % tuple(p) for p in (p0, p1, p2, p3))
    return 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [%s] %s\n' % (pts, extra)


MAP_WORLD = ('WorldBegin\nLightSource "point" "point from" [8 12 14] "rgb I" [200 200 200]\n'
             'Material "matte" "rgb Kd" [.5 .5 .5]\n' + _quad((1, 1, 1), (15, 1, 1), (15, 1, 20), (1, 1, 20)) +
             'Material "plastic" "rgb Kd" [.2 .3 .7]\n' + _quad((2, 2, 5), (5, 2, 5), (5, 6, 5), (2, 6, 5)) +
             'Material "mirror"\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3 0 3 4] "point P" [6 2 8  8.5 2 8  9 4 8.5  7 5.5 8  6 4 7.5]\n'
             'Material "matte" "rgb Kd" [.7 .2 .2]\nAttributeBegin\nTranslate 11 3 10\nShape "sphere" "float radius" [1.2]\nAttributeEnd\n'
             'ObjectBegin "thing"\nMaterial "plastic" "rgb Kd" [.6 .6 .1]\n' + _quad((-1, -0.6, 0.3), (1, -0.6, -0.3), (1, 0.2, -0.3), (-1, 0.2, 0.3)) +
             'Material "matte" "rgb Kd" [.1 .7 .7]\nTranslate 0.2 0.6 0\nShape "sphere" "float radius" [0.5]\nObjectEnd\n'
             'AttributeBegin\nTranslate 12 8 6\nRotate 30 0 1 0\nScale 3 1.4 2.4\nObjectInstance "thing"\nAttributeEnd\nWorldEnd\n')
MAP_CAMERAS = {
    "orthographic": 'LookAt 8 15 28  8 3 8  0 1 0\nCamera "orthographic" "float screenwindow" [-10 10 -7.5 7.5]\n',
    "environment": 'LookAt 10 6.5 9  10 6.5 0  0 1 0\nCamera "environment" "float ipd" [.4] "float convergencedistance" [6]\n',
}


def _hits(ob, twin, r32, r64):
    """Closest hits of the float32 rays and of the float64 rays (rounded to the float32 the tracer takes) in the twin:
    (prim, depth, p) of each, and the samples whose verdict or primitive differs."""
    a, b = cm.hit_values(ob, twin, _rays_of(r32)), cm.hit_values(ob, twin, _rays_of(r64))
    return a, b, a[0] != b[0]


@pytest.mark.parametrize("camera", list(MAP_CAMERAS))
def test_metadata_maps(pt, ob, camera):
    """Integrator "metadata" over triangles, a sphere and an object instance: every sample's restated ray traced in the twin and
    splatted with the box filter. mesh and material exactly, depth and coordinates within the summed bars of a pixel's samples,
    weights exactly; pixels an unsure sample reaches are left out."""
    text = (MAP_CAMERAS[camera] + 'Film "image" "integer xresolution" [32] "integer yresolution" [24]\nSampler "halton" "integer pixelsamples" [1]\n'
            'Integrator "metadata" "string strategy" "depth"\n' + MAP_WORLD)
    s, twin = cmod.pair(pt, text)
    samples, p_film, r32, r64, unsure = _restated(ob, s, twin)
    (prim, dep32, p32), (_, dep64, p64), differ = _hits(ob, twin, r32, r64)
    unsure = unsure | differ
    hit = (prim >= 0) & ~unsure
    assert unsure.mean() <= 0.01 and 0.2 < hit.mean() < 0.95, (unsure.mean(), hit.mean())
    exp = cm.expected_maps(pt, ob, twin, _rays_of(r32), spp=1)
    assert exp.n_samples == len(samples) and exp.sphere_hits > 10 and exp.instance_hits[0] > 10 and all(v == 0 for v in exp.bad.values())
    bound = {"depth": np.zeros(len(samples)), "coordinates": np.zeros(len(samples))}
    bound["depth"][hit] = cmod.bar(dep32, dep64.astype(np.float64), hit)
    bound["coordinates"][hit] = cmod.bar(p32, p64.astype(np.float64), hit)
    keep = _splat(s, p_film, unsure[:, None].astype(np.float64))[0][..., 0] == 0
    integ = pt.MetadataIntegrator(s)
    for strategy in ("depth", "coordinates", "mesh", "material"):
        film, weight = integ.Render(strategy=strategy)
        c = integ.counters.as_dict()
        assert np.array_equal(weight, exp.weight) and c["camera_rays"] == len(samples) and c["bad_samples"] == 0
        want = exp.film[strategy]
        assert want[keep].any()
        if strategy in ("mesh", "material"):
            assert np.array_equal(film[keep], want[keep]), strategy
        else:
            n = 3 if strategy == "coordinates" else 1
            b = _splat(s, p_film, bound[strategy][:, None])[0][..., 0]
            diff = np.abs(film[..., :n].astype(np.float64) - want[..., :n]).max(axis=2)
            print("%s, %s: worst difference %.3e, worst bound %.3e" % (camera, strategy, diff[keep].max(), b[keep].max()))
            assert np.all((diff <= b)[keep]), (camera, strategy)


# ---------------------------------------------------------------------------------------------------------------------
# 3: direct light
LIGHT_POS = (.5, 4, .5)
LIT_WORLD = ('WorldBegin\nLightSource "point" "point from" [%g %g %g] "rgb I" [30 28 26]\n' % LIGHT_POS +
             'Material "matte" "rgb Kd" [.6 .5 .4]\n' + _quad((-6, 0, -6), (6, 0, -6), (6, 0, 6), (-6, 0, 6)) +
             'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-2 1.5 -1  1.5 1.2 -1.5  0 2 2]\nWorldEnd\n')
LIT_CAMERAS = {
    "orthographic": 'LookAt 1 9 3  0 0 0  0 1 0\nCamera "orthographic" "float screenwindow" [-4 4 -4 4]\n',
    "orthographic, lens": 'LookAt 1 9 3  0 0 0  0 1 0\nCamera "orthographic" "float screenwindow" [-4 4 -4 4] "float lensradius" [.4] "float focaldistance" [9]\n',
    "environment": 'LookAt 1 3 2  0 0 0  0 1 0\nCamera "environment" "float ipd" [.3]\n',
}


def _spawn_origin(ob, scene, ray, target):
    """The origin of isect.SpawnRayTo(target) at the ray's closest hit (oracle_spawn_rays, mode 1)."""
    import ctypes as C
    fn = ms._spawn_rays(ob)
    F = C.POINTER(C.c_float)
    out = np.zeros(7, np.float32)
    t = np.asarray(target, np.float32)
    r = np.ascontiguousarray(ray, np.float32)
    assert fn(scene.desc_ptr, r.ctypes.data_as(F), 1, t.ctypes.data_as(F), 1, 0, out.ctypes.data_as(F))
    return out[0:3].copy()


def _direct_light(ob, twin, rays):
    """Per ray: (L [31], lit) of path.cpp's direct lighting at depth 0 under the twin's one point light over matte surfaces:
    Kd / Pi * I / r^2 * |cos| where the light sample's shadow ray -- from the oracle's offset origin towards the light, tMax
    1 - ShadowEpsilon -- is free; `lit` counts the shadow rays the integrator traces (f != 0: wo and wi on one side)."""
    d = twin.desc
    prim, _, p = cm.hit_values(ob, twin, rays)
    light = d.lights[0]
    pos, I = np.array(list(light.pos), np.float32), np.array(list(light.L), np.float64)
    L, lit, shadow = np.zeros((len(rays), 31)), np.zeros(len(rays), bool), []
    P = np.array([d.P[i] for i in range(3 * d.n_verts)], np.float64).reshape(-1, 3)
    normal, kd = {}, {}
    for i in np.nonzero(prim >= 0)[0]:
        k = int(prim[i])
        if k not in normal:
            tri = d.prims[k].shape
            v = [P[d.tri_indices[3 * tri + j]] for j in range(3)]
            n = np.cross(v[1] - v[0], v[2] - v[0])
            normal[k] = n / np.linalg.norm(n)
            mat = d.materials[d.prims[k].material]
            assert mat.n_bxdfs == 1
            kd[k] = np.array(list(mat.bxdf[0].R), np.float64)
        pi = p[i].astype(np.float64)
        wi = pos.astype(np.float64) - pi
        wo = -rays[i, 3:6].astype(np.float64)
        if float(normal[k] @ wi) * float(normal[k] @ wo) <= 0:
            continue                                                   # f = 0: no shadow ray
        lit[i] = True
        origin = _spawn_origin(ob, twin, rays[i], pos)
        shadow.append((i, np.concatenate([origin, pos - origin, [np.float32(1 - .0001)]]).astype(np.float32)))
        r2 = float(wi @ wi)
        L[i] = kd[k] / np.pi * I / r2 * abs(float(normal[k] @ wi)) / np.sqrt(r2)
    if shadow:
        with ob.exact_libm():
            occluded = ob.trace(twin, np.array([r for _, r in shadow], np.float32), any_hit=True)[0][:, 0].view(np.int32) >= 0
        for (i, _), occ in zip(shadow, occluded):
            if occ:
                L[i] = 0
    return L, lit, prim


@pytest.mark.parametrize("camera", list(LIT_CAMERAS))
def test_direct_light(pt, ob, camera):
    """Integrator "path" maxdepth 1, one point light over a matte floor and an occluding triangle. Film relative L2 against
    1e-6 (the bar of test_disk_gpu.py::test_emitter_film), weights equal, camera_rays and shadow_rays exactly."""
    text = (LIT_CAMERAS[camera] + 'Film "image" "integer xresolution" [32] "integer yresolution" [32]\nSampler "halton" "integer pixelsamples" [2]\n'
            'Integrator "path" "integer maxdepth" [1]\n' + LIT_WORLD)
    s, twin = cmod.pair(pt, text)
    samples, p_film, r32, r64, unsure = _restated(ob, s, twin)
    L, lit, prim = _direct_light(ob, twin, _rays_of(r32))
    L64, lit64, prim64 = _direct_light(ob, twin, _rays_of(r64))
    unsure = unsure | (prim != prim64) | (lit != lit64) | ((L.sum(axis=1) > 0) != (L64.sum(axis=1) > 0))
    assert unsure.mean() <= 0.01 and lit.mean() > 0.2 and ((L.sum(axis=1) == 0) & lit).sum() > 5, (unsure.mean(), lit.mean())   # and some are shadowed
    want, wsum = _splat(s, p_film, L)
    keep = _splat(s, p_film, unsure[:, None].astype(np.float64))[0][..., 0] == 0
    integ = pt.CreatePathIntegrator(s)
    film, weight = integ.Render()
    c = integ.counters.as_dict()
    rel = _rel_l2(film[keep], want[keep])
    print("%s: relative L2 %.3e, %d of %d samples lit, %d unsure, shadow rays %d" % (camera, rel, int(lit.sum()), len(samples), int(unsure.sum()), c["shadow_rays"]))
    assert np.array_equal(weight, wsum) and c["bad_samples"] == 0
    assert c["camera_rays"] == len(samples)
    assert abs(c["shadow_rays"] - int(lit[~unsure].sum())) <= int(unsure.sum())     # exactly, over the sure samples
    assert rel < 1e-6, rel


# ---------------------------------------------------------------------------------------------------------------------
# 4: the differentials reach the textures
def _tquad(p0, p1, p2, p3):
    """A textured quad, uv (0,0) (1,0) (1,1) (0,1), whose two triangles both END at corner 0: its uv is (0, 0), so that
    uvHit = b0 uv[0] + b1 uv[1] + b2 (0, 0) follows exactly from the two barycentrics ob.trace reports."""
    pts = " ".join("%g %g %g" % tuple(p) for p in (p0, p1, p2, p3))
    return 'Shape "trianglemesh" "integer indices" [1 2 0 2 3 0] "point P" [%s] "float uv" [0 0 1 0 1 1 0 1]\n' % pts


F = np.float32


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _triangle_shading(d, tri, b0, b1):
    """uvHit, dpdu, dpdv and n of a hit on triangle `tri` in float32, in the reference's operation order
    (Triangle::Intersect, triangle.cpp:293-346)."""
    v = [d.tri_indices[3 * tri + j] for j in range(3)]
    P = [np.array([d.P[3 * k + c] for c in range(3)], F) for k in v]
    uv = [np.array([d.UV[2 * k], d.UV[2 * k + 1]], F) for k in v]
    assert not uv[2].any()
    duv02, duv12, dp02, dp12 = uv[0] - uv[2], uv[1] - uv[2], P[0] - P[2], P[1] - P[2]
    det = duv02[0] * duv12[1] - duv02[1] * duv12[0]
    assert abs(det) >= 1e-8
    invdet = F(1) / det
    dpdu = (duv12[1] * dp02 - duv02[1] * dp12) * invdet
    dpdv = (-duv12[0] * dp02 + duv02[0] * dp12) * invdet
    n = np.cross(dp02.astype(np.float64), dp12.astype(np.float64)).astype(F)           # Cross: in double, rounded
    n = n * (F(1) / np.sqrt(_dot(n, n)))
    return F(b0) * uv[0] + F(b1) * uv[1], dpdu, dpdv, n


def _solve2x2(A, B):
    """SolveLinearSystem2x2, transform.cpp:41-49."""
    det = A[0][0] * A[1][1] - A[0][1] * A[1][0]
    if abs(det) < 1e-10:
        return F(0), F(0)
    x0, x1 = (A[1][1] * B[0] - A[0][1] * B[1]) / det, (A[0][0] * B[1] - A[1][0] * B[0]) / det
    return (F(0), F(0)) if np.isnan(x0) or np.isnan(x1) else (x0, x1)


def _compute_differentials(p, n, dpdu, dpdv, diffs):
    """SurfaceInteraction::ComputeDifferentials, interaction.cpp:103-148, in float32: (dudx, dvdx, dudy, dvdy)."""
    dd = _dot(n, p)
    aux = []
    for ro, rd in ((diffs[0], diffs[2]), (diffs[1], diffs[3])):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -(_dot(n, ro) - dd) / _dot(n, rd)
        if np.isinf(t) or np.isnan(t):
            return F(0), F(0), F(0), F(0)
        aux.append(ro + t * rd)
    if abs(n[0]) > abs(n[1]) and abs(n[0]) > abs(n[2]):
        d0, d1 = 1, 2
    elif abs(n[1]) > abs(n[2]):
        d0, d1 = 0, 2
    else:
        d0, d1 = 0, 1
    A = [[dpdu[d0], dpdv[d0]], [dpdu[d1], dpdv[d1]]]
    out = []
    for q in aux:
        out += list(_solve2x2(A, [q[d0] - p[d0], q[d1] - p[d1]]))
    return out


def _textured_expectation(ob, s, twin, r, p_film, with_differentials):
    """The film of matte, image-textured quads under one light at maxdepth 1, from restated camera rays: per sample
    T / pi * Li * |cos|. T is the oracle's EWA lookup (MIPMap::Lookup + FromRGB, clamped) at the (s, t) and footprint the
    reference hands it, restated in float32 in its operation order: the hit's p (the oracle's) and uv (from the oracle's
    barycentrics), the triangle's dpdu, dpdv and n, SurfaceInteraction::ComputeDifferentials over the restated, scaled
    offset rays, UVMapping2D::Map (texture.cpp:91-99). The radiometry around T is float64."""
    d = twin.desc
    rays = _rays_of(r)
    with ob.exact_libm():
        hits, _ = ob.trace(twin, rays)
        prim = hits[:, 0].copy().view(np.int32)
        p = ms.hit_points(ob, twin, rays)
    tex, light = d.textures[0], d.lights[0]
    su, sv, du, dv = F(tex.su), F(tex.sv), F(tex.du), F(tex.dv)
    I = np.array(list(light.L), np.float64)
    L = np.zeros((len(rays), 31))
    for i in np.nonzero(prim >= 0)[0]:
        uv, dpdu, dpdv, n = _triangle_shading(d, d.prims[int(prim[i])].shape, hits[i, 2], hits[i, 3])
        dst = [F(0)] * 4
        if with_differentials:
            dudx, dvdx, dudy, dvdy = _compute_differentials(p[i], n, dpdu, dpdv, [r["diffs"][k][i] for k in range(4)])
            dst = [su * dudx, sv * dvdx, su * dudy, sv * dvdy]
        with ob.exact_libm():
            _, T = ob.texture_lookup(twin, 0, (su * uv[0] + du, sv * uv[1] + dv), dst[:2], dst[2:])
        pi, n64 = p[i].astype(np.float64), n.astype(np.float64)
        if light.type == 2:                                             # MI_LIGHT_DISTANT: Li = L along wLight
            wi, falloff = np.array(list(light.dir), np.float64), 1.0
        else:
            wi = np.array(list(light.pos), np.float64) - pi
            falloff = 1.0 / float(wi @ wi)
            wi = wi / np.linalg.norm(wi)
        L[i] = np.clip(T.astype(np.float64), 0, None) / np.pi * I * falloff * abs(float(n64 @ wi))
    return _splat(s, p_film, L)[0], int((prim >= 0).sum())


TEX_LINE = 'Texture "img" "spectrum" "imagemap" "string filename" "tex64.png" "float uscale" [%g] "float vscale" [%g]\nMaterial "matte" "texture Kd" "img"\n'
TEXTURED = {
    # straight down at a floor under a distant light along the normal
    "orthographic": ('LookAt 0 6 0  0 0 0  0 0 -1\nCamera "orthographic" "float screenwindow" [-5 5 -5 5]\n',
                     'LightSource "distant" "point from" [0 1 0] "point to" [0 0 0] "rgb L" [3 3 3]\n' + TEX_LINE % (3, 3) +
                     _tquad((-6, 0, -6), (6, 0, -6), (6, 0, 6), (-6, 0, 6))),
    # inside a textured box around a point light
    "environment": ('LookAt .3 .2 .1  .3 .2 -1  0 1 0\nCamera "environment"\n',
                    'LightSource "point" "point from" [-.4 .5 .3] "rgb I" [20 20 20]\n' + TEX_LINE % (2, 2) +
                    _tquad((-3, -2, -3), (3, -2, -3), (3, -2, 3), (-3, -2, 3)) + _tquad((-3, 2, -3), (-3, 2, 3), (3, 2, 3), (3, 2, -3)) +
                    _tquad((-3, -2, -3), (-3, 2, -3), (3, 2, -3), (3, -2, -3)) + _tquad((-3, -2, 3), (3, -2, 3), (3, 2, 3), (-3, 2, 3)) +
                    _tquad((-3, -2, -3), (-3, -2, 3), (-3, 2, 3), (-3, 2, -3)) + _tquad((3, -2, -3), (3, 2, -3), (3, 2, 3), (3, -2, 3))),
}


@pytest.mark.parametrize("camera", list(TEXTURED))
def test_differentials_reach_the_textures(pt, ob, tmp_path, camera):
    """An image-textured Kd (a 64 x 64 map, EWA) behind each camera, maxdepth 1: the EWA footprint comes from the camera's own
    offset rays, which k_generate stores in the pool planes the realistic camera's go to and the LENS twins of the textured
    k_shade instances load. Bar: relative L2 1e-6 of the film, the bar of test_gpu_parity._parity that the textured parity
    tests there (test_image_textures_against_oracle and its neighbours) hold the device to. The same expectation with no
    footprint (a point lookup on the finest level) must miss that bar by a factor of 1000: the test sees the differentials."""
    import scenes_text as st
    st.write_png(os.path.join(str(tmp_path), "tex64.png"), st._texture_image(64, 64, 7))
    head, world = TEXTURED[camera]
    text = (head + 'Film "image" "integer xresolution" [32] "integer yresolution" [%d]\nSampler "halton" "integer pixelsamples" [4]\n'
            'Integrator "path" "integer maxdepth" [1]\nWorldBegin\n' % (32 if camera == "orthographic" else 16) + world + 'WorldEnd\n')
    s, twin = cmod.pair(pt, text, base_dir=str(tmp_path))
    assert s.desc.n_textures == 1 and s.desc.textures[0].filter == twin.desc.textures[0].filter and any(s.desc.materials[i].textured for i in range(s.desc.n_materials))
    samples, p_film, r32, r64, unsure = _restated(ob, s, twin)
    prim32, prim64 = cm.hit_values(ob, twin, _rays_of(r32))[0], cm.hit_values(ob, twin, _rays_of(r64))[0]
    unsure = unsure | (prim32 != prim64)
    assert unsure.mean() <= 0.01
    want, n_hit = _textured_expectation(ob, s, twin, r32, p_film, True)
    point, _ = _textured_expectation(ob, s, twin, r32, p_film, False)
    keep = _splat(s, p_film, unsure[:, None].astype(np.float64))[0][..., 0] == 0
    assert n_hit > 0.9 * len(samples) and want.any() and _rel_l2(point[keep], want[keep]) > 1e-3
    integ = pt.CreatePathIntegrator(s)
    film, weight = integ.Render()
    rel, rel_point = _rel_l2(film[keep], want[keep]), _rel_l2(film[keep], point[keep])
    print("%s: relative L2 %.3e with the camera's differentials, %.3e with a point lookup" % (camera, rel, rel_point))
    assert integ.counters.as_dict()["camera_rays"] == len(samples)
    assert rel_point > 1e-3
    assert rel < 1e-6, rel
    small, wsmall = integ.Render(path_pool=256)          # the planes travel with recycled slots too
    assert np.array_equal(weight, wsmall) and _rel_l2(small, film) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# 5: schedules
DEEP_WORLD = ('WorldBegin\nAttributeBegin\nAreaLightSource "diffuse" "rgb L" [14 13 12]\n' + _quad((-1, 3.9, -1), (1, 3.9, -1), (1, 3.9, 1), (-1, 3.9, 1)) + 'AttributeEnd\n'
              'Material "matte" "rgb Kd" [.6 .55 .5]\n' + _quad((-5, -1, -5), (5, -1, -5), (5, -1, 9), (-5, -1, 9)) + _quad((-5, -1, -4), (5, -1, -4), (5, 5, -4), (-5, 5, -4)) +
              _quad((-5, 5, -5), (5, 5, -5), (5, 5, 9), (-5, 5, 9)) + _quad((5, -1, -5), (5, -1, 9), (5, 5, 9), (5, 5, -5)) + _quad((-5, -1, 9), (5, -1, 9), (5, 5, 9), (-5, 5, 9)) +
              'AttributeBegin\nMaterial "mirror"\n' + _quad((-4, -1, -3), (-4, -1, 3), (-4, 4, 3), (-4, 4, -3)) + 'AttributeEnd\n'
              'AttributeBegin\nMaterial "glass" "float index" [1.5]\nTranslate 1.1 -.2 .6\nShape "sphere" "float radius" [.8]\nAttributeEnd\nWorldEnd\n')
DEEP = {
    "orthographic": ('LookAt 0 2 8  0 1 0  0 1 0\nCamera "orthographic" "float screenwindow" [-5 5 -3 5] "float lensradius" [.2] "float focaldistance" [8]\n', 'Integrator "path" "integer maxdepth" [5]'),
    "environment, spectralpath": ('LookAt 0 1 2.5  0 1 0  0 1 0\nCamera "environment" "float ipd" [.2] "float convergencedistance" [4]\n',
                                  'Integrator "spectralpath" "integer maxdepth" [5] "integer numCABands" [4]'),
}


@pytest.mark.parametrize("camera", list(DEEP))
def test_schedules(pt, camera, monkeypatch):
    """A depth-5 scene (a closed room with a mirror, a glass sphere and an area light): a 256-slot pool, two shards, two passes over sample ranges,
    MIPT_STREAMS=2 and MIPT_DARK_STREAM=0 equal the plain render -- weights exactly, films to 1e-6 relative L2, the rule of
    tests/test_render_schedule_gpu.py."""
    head, integrator = DEEP[camera]
    text = head + 'Film "image" "integer xresolution" [32] "integer yresolution" [24]\nSampler "halton" "integer pixelsamples" [4]\n' + integrator + "\n" + DEEP_WORLD
    s = pt.Scene(text=text)
    assert s.errors == [] and s.desc.camera_type == (2 if camera == "orthographic" else 3) and s.desc.n_spheres == 1
    integ = pt.CreateIntegrator(s)
    ref, wref = integ.Render()
    c = integ.counters.as_dict()
    bands = s.desc.integrator.n_ca_bands
    assert bands == (4 if "spectralpath" in camera else 1)
    assert ref.any() and c["camera_rays"] == 32 * 24 * 4 * bands and c["shadow_rays"] > 0 and c["bad_samples"] == 0   # (one camera ray per band)
    assert c["path_length_sum"] > 1.2 * c["camera_rays"]                 # paths go on past the first vertex

    def same(film, weight, how):
        rel = _rel_l2(film, ref)
        print("%s, %s: relative L2 %.3e" % (camera, how, rel))
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
    film, weight = pt.CreateIntegrator(s).Render()
    same(film, weight, "two sub-renderers")
    monkeypatch.delenv("MIPT_STREAMS")
    monkeypatch.setenv("MIPT_DARK_STREAM", "0")
    film, weight = pt.CreateIntegrator(s).Render()
    same(film, weight, "MIPT_DARK_STREAM=0")


# ---------------------------------------------------------------------------------------------------------------------
# 6: the command line
@pytest.mark.parametrize("camera", list(LIT_CAMERAS))
def test_pbrt_amd_renders_a_file_with_either_camera(pt, tmp_path, camera):
    """`pbrt_amd scene.pbrt --outfile out.dat` in a fresh process with the switch in its environment: exit code 0, no error
    line about the camera, and the .dat file's sums equal the film of the in-process render (1e-6 relative L2: float atomics)."""
    import subprocess
    text = (LIT_CAMERAS[camera] + 'Film "image" "integer xresolution" [32] "integer yresolution" [32]\nSampler "halton" "integer pixelsamples" [2]\n'
            'Integrator "path" "integer maxdepth" [1]\n' + LIT_WORLD)
    path = tmp_path / "scene.pbrt"
    path.write_text(text)
    out = tmp_path / "out.dat"
    exe = os.path.join(os.path.dirname(os.path.abspath(pt.__file__)), "pbrt_amd")
    r = subprocess.run([exe, str(path), "--outfile", str(out)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "outside the hot-path scope" not in r.stdout + r.stderr
    s = pt.Scene(str(path))
    assert s.errors == [] and s.desc.camera_type in (2, 3)
    film, _ = pt.CreateIntegrator(s).Render()
    got = pt.read_dat(str(out))
    assert got.shape == film.shape and film.any() and _rel_l2(got, film) < 1e-6
