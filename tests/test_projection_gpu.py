"""LightSource "projection" on the device: mi_pt_light_probe against projection_light.py over the cases of
projection_cases.py; the probe's refusals; a projector without a map against the point light it is inside its frustum, film
for film; an image projected on a wall against the point-light twin times the restated Projection at each hit; schedules; and
the instances a projection scene launches. Bars: light_cases.check / check_rel -- four times the worst float32-vs-float64
deviation of the restatement over the selected queries of ONE family, never below 8 ulp (absolute) or 8 * 2^-23 (relative). A
query on which the float32 and the float64 restatement decide differently is unsure and decides nothing."""
import numpy as np
import pytest

import light_cases as lc
import light_restatement as lr
import projection_cases as pc
import projection_light as pl
from test_noise_texture_gpu import _pixel_samples, _rel_l2, _tri_vertices

pytestmark = pytest.mark.gpu

RAY_COUNTERS = ("camera_rays", "regular_rays", "shadow_rays", "total_paths", "zero_radiance_paths", "path_length_sum", "bad_samples")


# ---------------------------------------------------------------------------------------------------------------- probe
@pytest.mark.parametrize("xf", list(pc.TRANSFORMS))
@pytest.mark.parametrize("name", list(pc.MAPS))
def test_probe_against_the_restatement(pt, tmp_path, name, xf):
    s, k = pc.light_scene(pt, tmp_path, name, xf)
    l32, l64 = pl.both(s.desc, k)
    fams = pc.families(l64, np.random.default_rng(43))
    integ = pt.CreatePathIntegrator(s)
    got = integ.light_probe(k, 0, np.concatenate([f.q for f in fams]))
    log, at, same, words = [], 0, 0, 0
    try:
        for f in fams:
            g = got[at:at + len(f.q)]
            at += len(f.q)
            _, n = pc.hold("%s, %s" % (name, xf), l32, l64, f, g, log)
            same += n
            words += g.size
        log.append("%s, %s: %d of %d output words equal the float32 restatement bit for bit" % (name, xf, same, words))
    finally:
        print("\n".join(log))


def test_probe_refusals_and_the_renderer_still_renders(pt, tmp_path):
    """Pdf_Li is 0 (mode 1); Le does not exist for a delta light (mode 2), nor light -1 or n_lights: MI_ERR_INVALID."""
    import ctypes as C
    s, k = pc.light_scene(pt, tmp_path, "4x2", "rotated and scaled")
    integ = pt.CreatePathIntegrator(s)
    film, weight = integ.Render()
    assert film.any()
    assert integ.light_probe(k, 1, np.ones((5, 9), np.float32)).tolist() == [0] * 5
    lib = pt.hip_lib()
    q, out = np.zeros((2, 9), np.float32), np.zeros((2, pt.LIGHT_PROBE_SAMPLE_FLOATS), np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for light, mode, what in ((k, 2, "delta light"), (-1, 0, "light index out of range"), (s.desc.n_lights, 0, "light index out of range")):
        assert lib.mi_pt_light_probe(integ._h, light, mode, 2, fp(q), fp(out)) == -1     # MI_ERR_INVALID
        assert what in lib.mi_pt_last_error().decode()
        assert not out.any()
    again, weight2 = integ.Render()
    assert np.array_equal(film, again) and np.array_equal(weight, weight2)


# ------------------------------------------------------------------------------- without a map: a point light in its frustum
ROOM_HEAD = ('LookAt 0 .1 2.8  0 0 1  0 1 0\nCamera "perspective" "float fov" [70]\n'
             'Film "image" "integer xresolution" [32] "integer yresolution" [32]\n'
             'Sampler "halton" "integer pixelsamples" [8]\n'
             'Integrator "%s" "integer maxdepth" [5] "string lightsamplestrategy" "%s"\nWorldBegin\n')
_QUAD = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [%s]\n'
# a closed room x, y in [-1, 1], z in [.4, 3]: with fov 150 (tan 75 deg = 3.73) every point of it is inside the frustum of a
# projector at the origin that looks down +z (at z = .4 the walls stand at |x| / z = 2.5)
ROOM = ('Material "matte" "rgb Kd" [.6 .55 .5]\n' +
        _QUAD % "-1 -1 .4  1 -1 .4  1 1 .4  -1 1 .4" + _QUAD % "-1 -1 3  1 -1 3  1 1 3  -1 1 3" +
        _QUAD % "-1 -1 .4  -1 -1 3  -1 1 3  -1 1 .4" + _QUAD % "1 -1 .4  1 -1 3  1 1 3  1 1 .4" +
        _QUAD % "-1 -1 .4  1 -1 .4  1 -1 3  -1 -1 3" + _QUAD % "-1 1 .4  1 1 .4  1 1 3  -1 1 3" +
        'AttributeBegin\nMaterial "plastic" "rgb Kd" [.3 .5 .3] "rgb Ks" [.3 .3 .3] "float roughness" [.2]\nTranslate .3 -.6 1.4\n'
        'Shape "sphere" "float radius" [.35]\nAttributeEnd\n'
        'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [6 6 5]\n' + _QUAD % "-.3 .98 1.4  .3 .98 1.4  .3 .98 2  -.3 .98 2" + 'AttributeEnd\n')


def _room(pt, integrator, strategy, light):
    s = pt.Scene(text=ROOM_HEAD % (integrator, strategy) + light + ROOM + "WorldEnd\n")
    assert s.errors == [], s.errors
    integ = pt.CreateIntegrator(s)
    film, weight = integ.Render()
    c = integ.counters.as_dict()
    # the eight samples of every pixel one by one: a pass of one sample number puts one sample into each pixel (box filter of
    # half a pixel; the bands of "spectralpath" fill disjoint bins), so no film word is the sum of two contributions
    passes = [integ.Render(spp=1, sample_begin=n) for n in range(8)]
    return s, film, weight, c, np.stack([f for f, _ in passes]), np.stack([w for _, w in passes])


@pytest.mark.parametrize("strategy", ["uniform", "spatial"])
@pytest.mark.parametrize("integrator", ["path", "spectralpath"])
def test_a_projector_without_a_map_is_a_point_light_inside_its_frustum(pt, integrator, strategy):
    """(I * 1) / d^2 and I / d^2 are the same floats and the sample stream is the same: the same ray counts, the same weights and
    the same film, although the two scenes are shaded by different k_shade instances. The film is compared bit for bit sample
    number by sample number (eight passes of one sample per pixel): the film is summed with float atomics, and where the
    samples of a pixel arrive in another order -- the two scenes queue their vertices differently -- the sum of all eight
    rounds differently. Measured on an MI355X, whole 8-spp films against the twin's: `path` 0 of 31 744 words differ under both
    strategies; `spectralpath` 0 to 11 words from one run to the next (relative L2 at most 2.2e-9) with every ray counter equal;
    sample by sample 0 of 253 952 words differ in every run. The whole films are held to 1e-6, the bar of the schedule tests
    for that reordering."""
    s, film, weight, c, per_sample, per_weight = _room(pt, integrator, strategy, 'LightSource "projection" "rgb I" [3 2.5 2] "float fov" [150]\n')
    t, tfilm, tweight, tc, tper_sample, tper_weight = _room(pt, integrator, strategy, 'LightSource "point" "rgb I" [3 2.5 2]\n')
    assert s.desc.lights[0].type == pl.PROJECTION and t.desc.lights[0].type == lr.POINT and s.desc.n_lights == t.desc.n_lights >= 2
    assert film.any() and c["shadow_rays"] > 0
    print("%s, %s: whole film relative L2 %.3e, %d of %d words differ; sample by sample %d of %d words differ"
          % (integrator, strategy, _rel_l2(film, tfilm), int((lc.bits(film) != lc.bits(tfilm)).sum()), film.size,
             int((lc.bits(per_sample) != lc.bits(tper_sample)).sum()), per_sample.size))
    print({n: (c[n], tc[n]) for n in RAY_COUNTERS})
    assert {n: c[n] for n in RAY_COUNTERS} == {n: tc[n] for n in RAY_COUNTERS}
    assert np.array_equal(weight, tweight) and np.array_equal(per_weight, tper_weight)
    assert per_sample.any(axis=(1, 2, 3)).all()
    assert np.array_equal(per_sample, tper_sample)
    assert _rel_l2(film, tfilm) < 1e-6


# ------------------------------------------------------------------------------------------------------ an image on a wall
_wall_cache = {}


def _wall(pt, tmp_path, name, spp=1):
    key = (name, spp)
    if key not in _wall_cache:
        fname, _ = pc.write_map(tmp_path, name)
        text = pc.wall_text(pc.light_text(fname, fov=60))
        twin = pc.wall_text(pc.point_twin())
        if spp != 1:
            text, twin = [x.replace('"integer pixelsamples" [1]', '"integer pixelsamples" [%d]' % spp) for x in (text, twin)]
        s, t = pt.Scene(text=text, base_dir=str(tmp_path)), pt.Scene(text=twin)
        assert s.errors == [] and t.errors == [], (s.errors, t.errors)
        integ = pt.CreateIntegrator(s)
        film, weight = integ.Render()
        c, stats = integ.counters.as_dict(), integ.shade_launch_stats()
        tfilm, tweight = pt.CreateIntegrator(t).Render()
        _wall_cache[key] = (s, t, integ, film, weight, c, stats, tfilm, tweight)
    return _wall_cache[key]


@pytest.mark.parametrize("name", ["4x2", "3x5"])
def test_an_image_on_a_wall(pt, tmp_path, name):
    """One sample through every pixel centre, direct light only: film == twin * P[b](hit), the twin being the same scene with
    a point light of the same I at the projector's place (same shadow, same f |cos| / d^2) and P the restated Projection towards
    the hit, which is Triangle::Intersect's b0 p0 + b1 p1 + b2 p2 from the device's barycentrics."""
    s, t, integ, film, weight, c, _, tfilm, tweight = _wall(pt, tmp_path, name)
    assert np.array_equal(weight, tweight) and (weight == 1).all()
    k = lc.light_of(s, pl.PROJECTION)
    assert list(s.desc.lights[k].pos) == list(t.desc.lights[0].pos)
    rays = integ.camera_rays_ex(_pixel_samples(s))
    hits = integ.trace(np.ascontiguousarray(rays[:, :8]))
    prim = hits[:, 0].view(np.int32)
    hit = prim >= 0
    assert hit.mean() > 0.9
    tri = np.array([s.desc.prims[int(p)].shape if p >= 0 else 0 for p in prim])
    assert (tri >= 0).all() and set(tri[hit]) == {0, 1, 2, 3}          # the wall and the occluder
    P = {}
    for f, light in zip((np.float32, np.float64), pl.both(s.desc, k)):
        b0, b1 = hits[:, 2].astype(f), hits[:, 3].astype(f)
        (p0, p1, p2), _ = _tri_vertices(s, tri, f)
        p = b0[:, None] * p0 + b1[:, None] * p1 + (f(1) - b0 - b1)[:, None] * p2
        P[f] = pl.sample_li(light, p)
    unsure = hit & (P[np.float32]["black"] != P[np.float64]["black"])
    assert unsure.sum() <= 0.02 * len(unsure)
    h, w = weight.shape
    got, twin = film.reshape(h * w, -1), tfilm.reshape(h * w, -1)
    assert twin[hit].any() and not got[~hit].any()
    lit64 = hit & ~P[np.float64]["black"]
    dark = hit & P[np.float64]["black"] & ~unsure
    assert dark.sum() >= 16 and lit64.sum() >= 100, (int(dark.sum()), int(lit64.sum()))
    assert not got[dark].any()                                             # outside the frustum: exactly 0
    shadowed = lit64 & ~unsure & ~twin.any(axis=1)
    assert shadowed.sum() >= 4 and not got[shadowed].any()                 # the occluder's shadow
    e32 = twin * P[np.float32]["P"]
    e64 = twin.astype(np.float64) * P[np.float64]["P"]
    log = []
    try:
        lc.check("wall, map %s" % name, "film", got, e32, e64, lit64 & ~unsure, log)
    finally:
        print("\n".join(log))
    # a shadow ray is traced for every sample whose Li and f are not black, occluded or not
    n_lit, n_unsure = int((lit64 & ~unsure).sum()), int(unsure.sum())
    print("shadow rays %d, samples the restatement lights %d, unsure %d" % (c["shadow_rays"], n_lit, n_unsure))
    assert n_lit <= c["shadow_rays"] <= n_lit + n_unsure
    assert c["camera_rays"] == h * w


# -------------------------------------------------------------------------------------------------- schedules, launches
def test_pool_passes_and_shards_give_the_same_film(pt, tmp_path, monkeypatch):
    s, _, integ, film, weight, _, _, _, _ = _wall(pt, tmp_path, "3x5", spp=4)
    assert film.any()
    small, w = integ.Render(path_pool=256)
    print("pool 256: relative L2 %.3e" % _rel_l2(small, film))
    assert np.array_equal(w, weight) and _rel_l2(small, film) < 1e-6
    integ.Render(spp=1, sample_begin=0, download=False)
    two, w = integ.Render(spp=3, sample_begin=1, accumulate=True)
    print("two passes: relative L2 %.3e" % _rel_l2(two, film))
    assert np.array_equal(w, weight) and _rel_l2(two, film) < 1e-6
    monkeypatch.setenv("MIPT_STREAMS", "2")   # (read when the renderer is created)
    sub = pt.CreateIntegrator(s)
    acc, accw = np.zeros_like(film), np.zeros_like(weight)
    for r in range(2):
        f, w = sub.Render(shard_index=r, shard_count=2)
        acc += f
        accw += w
    print("two shards on two sub-renderers: relative L2 %.3e" % _rel_l2(acc, film))
    assert np.array_equal(accw, weight) and _rel_l2(acc, film) < 1e-6


def test_a_projection_scene_launches_the_general_instances(pt, tmp_path):
    s, t, _, _, _, c, (launches, blocks), _, _ = _wall(pt, tmp_path, "4x2")
    assert launches > 0 and blocks > 0
    plan, twin_plan = s.shade_plan(), t.shade_plan()
    for cls, k in plan["classes"].items():   # every class of the scene, the escaped rays' too
        assert k["tm"] == pt.TM_GENERIC, (cls, hex(k["tm"]))
    assert all(k["tm"] == pt.TM_DIFFUSE | pt.TM_LIGHTS_NO_ENV for k in twin_plan["classes"].values())
    # one instance serves every class of this scene: one k_shade launch per iteration that has something to shade, at the most
    assert len({k["instance"] for k in plan["classes"].values()}) == 1
    assert launches <= c["iterations"]
