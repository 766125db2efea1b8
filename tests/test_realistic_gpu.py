"""Camera "realistic" on the GPU. realistic_camera.py restates the reference's camera in float32 and float64 and says which
lines each function follows; the unchanged oracle supplies every camera sample's values and every closest hit. A sample whose
verdict (through the lens or not) differs between the two restatements belongs to the set U and decides nothing."""
import numpy as np
import pytest

import camera_motion as cm
import metadata_scenes as ms
import realistic_camera as rc

pytestmark = pytest.mark.gpu

LOOKAT = "8 5 30  8 5 0  0 1 0"
DGAUSS = '"float aperturediameter" [8] "float focusdistance" [25]'
_cache = {}


def _rel_l2(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / max((b ** 2).sum(), 1e-30)))


def _meta_scene(pt, params=DGAUSS, camera=None, sampler="halton", **kw):
    text = cm.metadata_scene(camera or rc.camera_block("dgauss.dat", LOOKAT, params), **kw)
    if sampler != "halton":
        text = text.replace('Sampler "halton"', 'Sampler "%s"' % sampler)
    s = pt.Scene(text=text)
    assert s.errors == [] and s.desc.camera_type == 1
    return s


def _restated(ob, scene, samples, band=None):
    r32 = rc.restate(scene, ob, samples, np.float32, band)
    r64 = rc.restate(scene, ob, samples, np.float64, band)
    return r32, r64, (r32["weight"] != 0) != (r64["weight"] != 0)


def _bars(r32, r64, both):
    """The rule of test_camera_motion_gpu._ray_bars, per quantity: four times the worst deviation of the float32 restatement
    from the float64 one, never below 8 ulp of the largest component."""
    def bar(a, b):
        a, b = a[both].astype(np.float64), b[both]
        return float(max(4 * np.abs(a - b).max(), 8 * float(np.spacing(np.float32(np.abs(b).max())))))
    out = dict(o=bar(r32["o"], r64["o"]), d=bar(r32["d"], r64["d"]), weight=bar(r32["weight"], r64["weight"]))
    for k, name in enumerate(("rxo", "ryo", "rxd", "ryd")):
        out[name] = bar(r32["diffs"][k], r64["diffs"][k])
    return out


def _check_rays(dev, r32, r64, unsure, bars, label):
    through64 = r64["weight"] != 0
    both = through64 & (r32["weight"] != 0) & ~unsure
    assert np.array_equal((dev[:, 8] != 0)[~unsure], through64[~unsure]), label
    worst = {}
    cols = dict(o=(dev[:, 0:3], r64["o"]), d=(dev[:, 3:6], r64["d"]), weight=(dev[:, 8], r64["weight"]),
                rxo=(dev[:, 9:12], r64["diffs"][0]), ryo=(dev[:, 12:15], r64["diffs"][1]),
                rxd=(dev[:, 15:18], r64["diffs"][2]), ryd=(dev[:, 18:21], r64["diffs"][3]))
    for name, (got, want) in cols.items():
        worst[name] = float(np.abs(got[both].astype(np.float64) - want[both]).max())
    print("%s: %d of %d through, %d unsure; worst / bar: %s" % (label, int(both.sum()), len(both), int(unsure.sum()),
          ", ".join("%s %.2e / %.2e" % (k, worst[k], bars[k]) for k in cols)))
    for name in cols:
        assert worst[name] <= bars[name], (label, name, worst[name], bars[name])
    assert np.all(np.isinf(dev[both, 6])) and np.all(dev[both, 6] > 0)


# ---------------------------------------------------------------------------------------------------------------------
# 5: rays, weights, differentials
def _ray_case(pt, ob, sampler):
    if ("rays", sampler) not in _cache:
        s = _meta_scene(pt, sampler=sampler, res=(64, 64), spp=4)
        samples = cm.frame_samples(s, 256, spp=4)
        r32, r64, unsure = _restated(ob, s, samples)
        through = r64["weight"] != 0
        # the conditions, on the CPU
        assert unsure.mean() <= 0.01, unsure.mean()
        assert 0.1 <= through.mean() <= 0.9, through.mean()
        both = through & (r32["weight"] != 0) & ~unsure
        _cache[("rays", sampler)] = dict(scene=s, samples=samples, r32=r32, r64=r64, unsure=unsure, bars=_bars(r32, r64, both))
    return _cache[("rays", sampler)]


@pytest.mark.parametrize("sampler", ["halton", "02sequence"])
def test_rays_weights_and_differentials(pt, ob, sampler):
    m = _ray_case(pt, ob, sampler)
    integ = pt.CreatePathIntegrator(m["scene"])
    dev = integ.camera_rays_ex(m["samples"])
    _check_rays(dev, m["r32"], m["r64"], m["unsure"], m["bars"], "double Gauss, " + sampler)
    # the plain parity call answers for the samples that get through with the same ray
    plain = integ.camera_rays(m["samples"])
    ok = dev[:, 8] != 0
    assert np.array_equal(plain[ok, :7].view(np.uint32), dev[ok, :7].view(np.uint32))


def test_weights_without_simple_weighting(pt, ob):
    """(shutterClose - shutterOpen) * cos^4 * boxArea / LensRearZ^2 with a shutter of 0.25 .. 0.75."""
    s = _meta_scene(pt, DGAUSS + ' "bool simpleweighting" "false" "float shutteropen" [.25] "float shutterclose" [.75]', res=(64, 64), spp=4)
    samples = cm.frame_samples(s, 256, spp=4)
    r32, r64, unsure = _restated(ob, s, samples)
    both = (r64["weight"] != 0) & (r32["weight"] != 0) & ~unsure
    dev = pt.CreatePathIntegrator(s).camera_rays_ex(samples)
    _check_rays(dev, r32, r64, unsure, _bars(r32, r64, both), "simpleweighting false")
    simple = _ray_case(pt, ob, "halton")
    ratio = r64["weight"][both] / simple["r64"]["weight"][both]
    L = s.desc.lens.contents
    b0 = np.array(list(L.exit_pupil_bounds[0]), np.float64)
    want = 0.5 * (b0[2] - b0[0]) * (b0[3] - b0[1]) / float(L.film_distance) ** 2
    assert np.allclose(ratio, want, rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------------------
# 6: chromatic bands
CA3 = 'Integrator "spectralpath" "integer numCABands" [3] "integer maxdepth" [1]'


def test_chromatic_bands(pt, ob):
    assert [rc.band_wavelength(3, b) for b in range(3)] == [445.0, 545.0, 645.0]
    s = _meta_scene(pt, DGAUSS + ' "bool chromaticAberrationEnabled" "true"', res=(64, 64), spp=4, integrator=CA3)
    assert s.desc.integrator.n_ca_bands == 3 and s.desc.lens.contents.chromatic_aberration == 1
    samples = cm.frame_samples(s, 256, spp=4)
    bars = _ray_case(pt, ob, "halton")["bars"]
    integ = pt.CreatePathIntegrator(s)
    dev = []
    for band in range(3):
        r32, r64, unsure = _restated(ob, s, samples, band)
        assert unsure.mean() <= 0.01
        dev.append(integ.camera_rays_ex(samples, band=band))
        _check_rays(dev[band], r32, r64, unsure, bars, "band %d at %g nm" % (band, r32["wavelength"]))
    ok = (dev[0][:, 8] != 0) & (dev[1][:, 8] != 0)
    assert ok.sum() > 25 and not np.any(np.all(dev[0][ok, 3:6] == dev[1][ok, 3:6], axis=1))   # band 1's ray is not band 0's
    with pytest.raises(RuntimeError):
        integ.camera_rays_ex(samples, band=3)
    # with the flag off every band's ray is the same ray, bit for bit
    off = _meta_scene(pt, DGAUSS, res=(64, 64), spp=4, integrator=CA3)
    o = pt.CreatePathIntegrator(off)
    first = o.camera_rays_ex(samples, band=0)
    assert (first[:, 8] != 0).sum() > 25
    for band in (1, 2):
        assert np.array_equal(o.camera_rays_ex(samples, band=band).view(np.uint32), first.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 7: maps
FAR = np.array([1e6, 1e6, 1e6, 0, 1, 0, np.inf], np.float32)   # a ray that meets nothing: a vignetted sample adds zeros with weight 1


def _maps(pt, ob):
    if "maps" not in _cache:
        bars = _ray_case(pt, ob, "halton")["bars"]
        s = _meta_scene(pt, res=(48, 48), spp=1)
        samples = cm.all_samples(s, 1)
        r32, r64, unsure = _restated(ob, s, samples)
        through = r32["weight"] != 0
        rays = np.tile(FAR, (len(samples), 1))
        rays[through, :3], rays[through, 3:6] = r32["o"][through], r32["d"][through]
        exp = cm.expected_maps(pt, ob, s, rays, 1)
        prim, depth, p = cm.hit_values(ob, s, rays)
        unstable = unsure.copy()
        bound_depth, bound_p = np.zeros(len(rays)), np.zeros((len(rays), 3))
        for comp in range(6):
            vals = []
            for sign in (-1.0, 1.0):
                q = rays.copy()
                q[through, comp] += np.float32(sign * (bars["o"] if comp < 3 else bars["d"]))
                vals.append(cm.hit_values(ob, s, q))
                unstable |= vals[-1][0] != prim
            with np.errstate(invalid="ignore"):
                bound_depth += 0.5 * np.abs(vals[1][1].astype(np.float64) - vals[0][1])
                bound_p += 0.5 * np.abs(vals[1][2].astype(np.float64) - vals[0][2])
        w, h = s.film_size
        cb, r = list(s.desc.film.cropped_bounds), np.array(list(s.desc.film.filter_radius), np.float32)
        left_out, bd, bp = np.zeros((h, w), bool), np.zeros((h, w)), np.zeros((h, w, 3))
        hit = prim >= 0
        for i, pf in enumerate(r32["p_film"]):
            dx, dy = pf[0] - np.float32(0.5), pf[1] - np.float32(0.5)
            x0, x1 = max(int(np.ceil(dx - r[0])), cb[0]) - cb[0], min(int(np.floor(dx + r[0])) + 1, cb[2]) - cb[0]
            y0, y1 = max(int(np.ceil(dy - r[1])), cb[1]) - cb[1], min(int(np.floor(dy + r[1])) + 1, cb[3]) - cb[1]
            left_out[y0:y1, x0:x1] |= unstable[i]
            if hit[i] and not unstable[i]:
                bd[y0:y1, x0:x1] += bound_depth[i]
                bp[y0:y1, x0:x1] += bound_p[i]
        print("maps: %.2f %% of the pixels left out, %.1f %% of the samples through the lens, %.1f %% hit something"
              % (100 * left_out.mean(), 100 * through.mean(), 100 * hit.mean()))
        assert left_out.mean() <= 0.02 and 0.1 < hit.mean() < 0.9 and 0.1 <= through.mean() <= 0.9
        _cache["maps"] = dict(scene=s, exp=exp, keep=~left_out, bound_depth=bd, bound_p=bp, through=int(through.sum()),
                              integ=pt.MetadataIntegrator(s))
    return _cache["maps"]


@pytest.mark.parametrize("strategy", ms.STRATEGIES)
def test_maps_behind_the_lens(pt, ob, strategy):
    m = _maps(pt, ob)
    exp, keep = m["exp"], m["keep"]
    film, weight = m["integ"].Render(strategy=strategy)
    c = m["integ"].counters.as_dict()
    assert c["camera_rays"] == exp.n_samples and c["bad_samples"] == 0
    assert abs(c["regular_rays"] - m["through"]) <= int((~keep).sum())   # a camera ray that does not get through traces nothing
    assert np.array_equal(weight, exp.weight)                             # ... and is added with weight 1 all the same
    want = exp.film[strategy]
    assert want[keep].any()
    if strategy in ("mesh", "material"):
        assert np.array_equal(film[keep], want[keep])
    else:
        bound = m["bound_depth"][..., None] if strategy == "depth" else m["bound_p"]
        n = bound.shape[2]
        diff = np.abs(film[..., :n].astype(np.float64) - want[..., :n])
        print("%s: worst difference %.3e, worst bound %.3e" % (strategy, diff[keep].max(), bound[keep].max()))
        assert np.all((diff <= 2 * bound)[keep])
        assert np.array_equal(film[..., n:][keep], want[..., n:][keep])


# ---------------------------------------------------------------------------------------------------------------------
# 8: weights in the film
def _emitter_scene(pt, params, integrator, res=32, spp=4):
    text = (rc.camera_block("dgauss.dat", "0 0 5  0 0 0  0 1 0", params) +
            'Film "image" "integer xresolution" [%d] "integer yresolution" [%d]\n'
            'Sampler "halton" "integer pixelsamples" [%d]\n%s\nWorldBegin\n'
            'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [3 2 1]\n'
            'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-.5 -.7 0  .9 -.7 0  .9 .4 0  -.5 .4 0]\n'
            'AttributeEnd\nWorldEnd\n' % (res, res, spp, integrator))
    s = pt.Scene(text=text)
    assert s.errors == [] and s.desc.n_lights == 2   # the quad's two triangles, one-sided, facing the camera
    return s


def _expected_film(ob, scene, bands):
    """Sum of w * Le * [hit] over the restated samples (box filter: weight 1), band b supplying its bins; the sample's weight
    is the last band's. Returns (film, filter-weight sum, camera rays, rays that get through, |U|)."""
    d = scene.desc
    samples = cm.all_samples(scene, scene.spp)
    le = np.array(list(d.lights[0].L), np.float64)
    w, h = scene.film_size
    cb, r = list(d.film.cropped_bounds), np.array(list(d.film.filter_radius), np.float32)
    delta = int(np.round(np.float32(31) / np.float32(bands)))
    L = np.zeros((len(samples), 31))
    through, unsure_any, weight = 0, np.zeros(len(samples), bool), None
    for b in range(bands):
        r32, r64, unsure = _restated(ob, scene, samples, b if bands > 1 else None)
        ok = r32["weight"] != 0
        rays = np.tile(FAR, (len(samples), 1))
        rays[ok, :3], rays[ok, 3:6] = r32["o"][ok], r32["d"][ok]
        with ob.exact_libm():
            hits, _ = ob.trace(scene, rays)
        hit = (hits[:, 0].copy().view(np.int32) >= 0) & ok
        lo, hi = delta * b, min(delta * (b + 1), 31)
        L[:, lo:hi] = hit[:, None] * le[lo:hi]
        through += int(ok.sum())
        unsure_any |= unsure
        weight, p_film = r32["weight"].astype(np.float64), r32["p_film"]
    film, wsum = np.zeros((h, w, 31)), np.zeros((h, w), np.float32)
    for i, pf in enumerate(p_film):
        dx, dy = pf[0] - np.float32(0.5), pf[1] - np.float32(0.5)
        x0, x1 = max(int(np.ceil(dx - r[0])), cb[0]) - cb[0], min(int(np.floor(dx + r[0])) + 1, cb[2]) - cb[0]
        y0, y1 = max(int(np.ceil(dy - r[1])), cb[1]) - cb[1], min(int(np.floor(dy + r[1])) + 1, cb[3]) - cb[1]
        film[y0:y1, x0:x1] += L[i] * weight[i]
        wsum[y0:y1, x0:x1] += np.float32(1)
    return film, wsum, len(samples) * bands, through, int(unsure_any.sum())


def _filter_sum(scene, p_film):
    """The filter-weight sum of samples at the raster positions p_film (box filter: 1 per pixel reached, film.h:131-141)."""
    d = scene.desc
    w, h = scene.film_size
    cb, r = list(d.film.cropped_bounds), np.array(list(d.film.filter_radius), np.float32)
    wsum = np.zeros((h, w), np.float32)
    for pf in p_film:
        dx, dy = pf[0] - np.float32(0.5), pf[1] - np.float32(0.5)
        x0, x1 = max(int(np.ceil(dx - r[0])), cb[0]) - cb[0], min(int(np.floor(dx + r[0])) + 1, cb[2]) - cb[0]
        y0, y1 = max(int(np.ceil(dy - r[1])), cb[1]) - cb[1], min(int(np.floor(dy + r[1])) + 1, cb[3]) - cb[1]
        wsum[y0:y1, x0:x1] += np.float32(1)
    return wsum


@pytest.mark.parametrize("simple", ["true", "false"])
def test_weights_reach_the_film(pt, ob, simple):
    s = _emitter_scene(pt, '"float aperturediameter" [8] "float focusdistance" [5] "bool simpleweighting" "%s" "float shutterclose" [.5]' % simple,
                       'Integrator "path" "integer maxdepth" [0]')
    want, wsum, cams, through, n_unsure = _expected_film(ob, s, 1)
    assert n_unsure == 0 and want.any() and 0.1 * cams < through < 0.9 * cams     # the premises, on the CPU
    integ = pt.CreatePathIntegrator(s)
    film, weight = integ.Render()
    c = integ.counters.as_dict()
    rel = _rel_l2(film, want)
    print("simpleweighting %s: relative L2 %.3e, %d of %d camera rays traced" % (simple, rel, c["regular_rays"], c["camera_rays"]))
    assert np.array_equal(weight, wsum)
    assert c["camera_rays"] == cams and c["regular_rays"] == through and c["bad_samples"] == 0
    assert rel < 1e-6, rel


def test_bands_and_the_last_bands_weight_reach_the_film(pt, ob):
    s = _emitter_scene(pt, '"float aperturediameter" [8] "float focusdistance" [5] "bool chromaticAberrationEnabled" "true"',
                       'Integrator "spectralpath" "integer numCABands" [3] "integer maxdepth" [0]')
    want, wsum, cams, through, n_unsure = _expected_film(ob, s, 3)
    assert n_unsure == 0 and want[..., :10].any() and want[..., 20:].any()
    integ = pt.CreatePathIntegrator(s)
    film, weight = integ.Render()
    c = integ.counters.as_dict()
    rel = _rel_l2(film, want)
    print("three bands: relative L2 %.3e, %d of %d camera rays traced" % (rel, c["regular_rays"], c["camera_rays"]))
    assert np.array_equal(weight, wsum)
    assert c["camera_rays"] == cams and c["regular_rays"] == through
    assert rel < 1e-6, rel


# ---------------------------------------------------------------------------------------------------------------------
# 9: schedules
def test_schedules_with_most_samples_vignetted(pt, ob):
    """A stop of 0.3 mm: the exit-pupil boxes keep their margin of two sample spacings around a pupil that small, and more
    than half of the samples miss it. Every sample must still be flushed, those finished inside k_generate too."""
    s = _meta_scene(pt, '"float aperturediameter" [0.3] "float focusdistance" [25]', res=(64, 64), spp=4,
                    integrator='Integrator "path" "integer maxdepth" [3]')
    probe = cm.frame_samples(s, 256, spp=4)
    assert (rc.restate(s, ob, probe)["weight"] == 0).mean() > 0.5
    integ = pt.PathIntegrator(s)
    n = 64 * 64 * 4
    ref, wref = integ.Render()
    c = integ.counters.as_dict()
    assert ref.any() and c["camera_rays"] == n and c["regular_rays"] > 0
    assert np.array_equal(wref, _filter_sum(s, rc.camera_samples(ob, s, cm.all_samples(s, 4))[0]))   # every sample was flushed
    traced = int((integ.camera_rays_ex(cm.all_samples(s, 4))[:, 8] != 0).sum())
    assert traced < n / 2

    def same(film, weight, how):
        rel = _rel_l2(film, ref)
        print("%s: relative L2 %.3e" % (how, rel))
        assert np.array_equal(weight, wref), how
        assert rel < 1e-6, (how, rel)

    film, weight = integ.Render(path_pool=256)
    assert integ.pool_info()[0] == 256
    same(film, weight, "256-slot pool")
    acc, wacc, cams = np.zeros_like(ref), np.zeros_like(wref), 0
    for r in range(3):
        f, w = integ.Render(shard_index=r, shard_count=3)
        acc += f
        wacc += w
        cams += integ.counters.camera_rays
    assert cams == n
    same(acc, wacc, "three shards")
    integ.Render(spp=2, sample_begin=0, download=False)
    film, weight = integ.Render(spp=2, sample_begin=2, accumulate=True)
    same(film, weight, "two passes")


# ---------------------------------------------------------------------------------------------------------------------
# 10: motion
def test_moving_camera_before_its_start_time(pt, ob):
    """TransformTimes 2 3 and the shutter 0..1: every ray takes the start transform, behind the lens as in front of it."""
    end = "15 7 25  0 4 2  0.2 1 0"
    lens = 'Camera "realistic" "string lensfile" "%s" %s\n' % (rc.lens_path("dgauss.dat"), DGAUSS)
    moving = ('TransformTimes 2 3\nActiveTransform StartTime\nLookAt %s\nActiveTransform EndTime\nLookAt %s\nActiveTransform All\n%s'
              % (LOOKAT, end, lens))
    m = _meta_scene(pt, camera=moving, res=(64, 64), spp=4)
    static = _ray_case(pt, ob, "halton")
    assert m.desc.camera.animated == 1 and static["scene"].desc.camera.animated == 0
    assert list(m.desc.camera.camera_to_world) == list(static["scene"].desc.camera.camera_to_world)
    a = pt.CreatePathIntegrator(m).camera_rays_ex(static["samples"])
    b = pt.CreatePathIntegrator(static["scene"]).camera_rays_ex(static["samples"])
    assert (a[:, 8] != 0).sum() > 25
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_moving_camera_at_interior_times(pt, ob):
    """TransformTimes 0.5 2 with the shutter 0 .. 1.5: most rays lie strictly between the transform times, and CameraToWorld is
    camera_motion's restated AnimatedTransform at each ray's own time, the last step behind the lens trace. Bars by the rule
    of test 5 over these samples."""
    end = "15 7 25  0 4 2  0.2 1 0"
    lens = ('Camera "realistic" "string lensfile" "%s" %s "float shutteropen" [0] "float shutterclose" [1.5]\n'
            % (rc.lens_path("dgauss.dat"), DGAUSS))
    moving = ('TransformTimes 0.5 2\nActiveTransform StartTime\nLookAt %s\nActiveTransform EndTime\nLookAt %s\nActiveTransform All\n%s'
              % (LOOKAT, end, lens))
    s = _meta_scene(pt, camera=moving, res=(64, 64), spp=4)
    assert s.desc.camera.animated == 1
    samples = cm.frame_samples(s, 96, spp=4)
    p_film, tu, p_lens = rc.camera_samples(ob, s, samples)
    times = cm.ray_times(s, tu)
    interior = (times > np.float32(0.5)) & (times < np.float32(2))
    assert interior.mean() > 0.5
    scale = np.float32(1) / np.sqrt(np.float32(s.spp))
    out = {}
    for f in (np.float32, np.float64):
        lens_f, anim = rc.Lens(s, f), cm.animated_of(s, f)
        rows = [rc.generate_ray_differential(lens_f, anim.interpolate(times[i]), p_film[i:i + 1], p_lens[i:i + 1], 550.0, scale)
                for i in range(len(samples))]
        out[f] = dict(weight=np.concatenate([r[0] for r in rows]), o=np.concatenate([r[1] for r in rows]),
                      d=np.concatenate([r[2] for r in rows]), diffs=[np.concatenate([r[3][k] for r in rows]) for k in range(4)])
    r32, r64 = out[np.float32], out[np.float64]
    unsure = (r32["weight"] != 0) != (r64["weight"] != 0)
    both = (r64["weight"] != 0) & (r32["weight"] != 0) & ~unsure
    assert unsure.mean() <= 0.01 and (both & interior).sum() > 25
    dev = pt.CreatePathIntegrator(s).camera_rays_ex(samples)
    assert np.array_equal(dev[:, 7].view(np.uint32), times.view(np.uint32))
    _check_rays(dev, r32, r64, unsure, _bars(r32, r64, both), "moving, %d of %d at interior times" % (int(interior.sum()), len(samples)))
    static = pt.CreatePathIntegrator(_ray_case(pt, ob, "halton")["scene"]).camera_rays_ex(samples)
    moved = both & interior
    assert not np.any(np.all(dev[moved, 0:3] == static[moved, 0:3], axis=1))      # and those are other rays than the start transform's


# ---------------------------------------------------------------------------------------------------------------------
# the differentials reach the textured shading kernels
QUAD = np.array([[-6, -2, -3], [6, -2, -3], [6, 3, -5], [-6, 3, -5]], np.float64)   # uv (0,0) (1,0) (1,1) (0,1): p = P0 + u dpdu + v dpdv
TEX_WORLD = """WorldBegin
LightSource "point" "rgb I" [40 40 40] "point from" [0 3 6]
Texture "img" "spectrum" "imagemap" "string filename" "tex_a.png" "float uscale" [5] "float vscale" [5]
Material "matte" "texture Kd" "img"
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-6 -2 -3  6 -2 -3  6 3 -5  -6 3 -5] "float uv" [0 0 1 0 1 1 0 1]
WorldEnd
"""


def _textured_expectation(ob, scene, with_differentials):
    """The film of a matte, image-textured, tilted quad under one point light at maxdepth 1, from the restated camera rays:
    per sample w * T / pi * I / r^2 * |cos|, T the oracle's EWA lookup (MIPMap::Lookup + FromRGB, clamped) with the footprint
    SurfaceInteraction::ComputeDifferentials (interaction.cpp:99-143) makes of the restated, scaled offset rays and
    UVMapping2D::Map (texture.cpp:91-99) scales; in float64 from the float32 restatement."""
    d = scene.desc
    samples = cm.all_samples(scene, scene.spp)
    r32, r64, unsure = _restated(ob, scene, samples)
    ok = r32["weight"] != 0
    rays = np.tile(FAR, (len(samples), 1))
    rays[ok, :3], rays[ok, 3:6] = r32["o"][ok], r32["d"][ok]
    prim, _, p = cm.hit_values(ob, scene, rays)
    hit = (prim >= 0) & ok
    dpdu, dpdv = QUAD[1] - QUAD[0], QUAD[3] - QUAD[0]
    n = np.cross(dpdu, dpdv)
    n /= np.linalg.norm(n)
    dims = [k for k in range(3) if k != int(np.argmax(np.abs(n)))]
    A = np.array([[dpdu[dims[0]], dpdv[dims[0]]], [dpdu[dims[1]], dpdv[dims[1]]]])
    tex = d.textures[0]
    light, I = np.array(list(d.lights[0].pos), np.float64), np.array(list(d.lights[0].L), np.float64)
    L = np.zeros((len(samples), 31))
    for i in np.nonzero(hit)[0]:
        pi = p[i].astype(np.float64)
        u, v = np.linalg.solve(A, (pi - QUAD[0])[dims])
        dst = np.zeros(4)
        if with_differentials:
            dd = float(n @ pi)
            for k, (ro, rd) in enumerate(((r32["diffs"][0][i], r32["diffs"][2][i]), (r32["diffs"][1][i], r32["diffs"][3][i]))):
                ro, rd = ro.astype(np.float64), rd.astype(np.float64)
                t = -(float(n @ ro) - dd) / float(n @ rd)
                du, dv = np.linalg.solve(A, (ro + t * rd - pi)[dims])
                dst[2 * k], dst[2 * k + 1] = tex.su * du, tex.sv * dv
        _, T = ob.texture_lookup(scene, 0, (tex.su * u + tex.du, tex.sv * v + tex.dv), dst[:2], dst[2:])
        wi = light - pi
        r2 = float(wi @ wi)
        L[i] = np.clip(T.astype(np.float64), 0, None) / np.pi * I / r2 * abs(float(n @ wi)) / np.sqrt(r2) * float(r32["weight"][i])
    w, h = scene.film_size
    cb, r = list(d.film.cropped_bounds), np.array(list(d.film.filter_radius), np.float32)
    film = np.zeros((h, w, 31))
    for i, pf in enumerate(r32["p_film"]):
        dx, dy = pf[0] - np.float32(0.5), pf[1] - np.float32(0.5)
        x0, x1 = max(int(np.ceil(dx - r[0])), cb[0]) - cb[0], min(int(np.floor(dx + r[0])) + 1, cb[2]) - cb[0]
        y0, y1 = max(int(np.ceil(dy - r[1])), cb[1]) - cb[1], min(int(np.floor(dy + r[1])) + 1, cb[3]) - cb[1]
        film[y0:y1, x0:x1] += L[i]
    return film, int(hit.sum()), int(unsure.sum())


def test_textured_lookup_behind_the_lens(pt, ob, tmp_path):
    """The EWA footprint of an image texture behind the double-Gauss lens comes from the lens camera's own offset rays, which
    k_generate stores for k_shade. Bar: relative L2 1e-4 of the film against the expectation above. The shading arithmetic
    (six float32 products, a division, float atomics) stays below 1e-6; the footprint's axes inherit the differentials' float32
    error -- bar / value about 7e-5 / 0.02 for the origins' offsets in test 5, i.e. 4e-3 of the footprint -- and the EWA value
    moves by at most a few per cent of that share as the ellipse grows, 1e-4 of the value. The same expectation with no
    footprint (a point lookup on the finest level) must miss that bar by a factor of 100: the test sees the differentials."""
    import scenes_text as st
    st.write_texture_files(str(tmp_path))
    text = (rc.camera_block("dgauss.dat", "0 0 8  0 0 0  0 1 0", '"float aperturediameter" [8] "float focusdistance" [10]') +
            'Film "image" "integer xresolution" [32] "integer yresolution" [32]\nSampler "halton" "integer pixelsamples" [4]\n'
            'Integrator "path" "integer maxdepth" [1]\n' + TEX_WORLD)
    s = pt.Scene(text=text, base_dir=str(tmp_path))
    assert s.errors == [] and s.desc.n_textures == 1 and any(s.desc.materials[i].textured for i in range(s.desc.n_materials))
    want, n_hit, n_unsure = _textured_expectation(ob, s, True)
    point, _, _ = _textured_expectation(ob, s, False)
    assert n_unsure == 0 and n_hit > 1000 and want.any()
    integ = pt.CreatePathIntegrator(s)
    film, weight = integ.Render()
    rel, rel_point = _rel_l2(film, want), _rel_l2(film, point)
    print("textured quad behind the lens: relative L2 %.3e with the lens differentials, %.3e with a point lookup" % (rel, rel_point))
    assert rel_point > 1e-2
    assert rel < 1e-4, rel
    small, wsmall = integ.Render(path_pool=256)          # the planes travel with recycled slots too
    assert np.array_equal(weight, wsmall) and _rel_l2(small, film) < 1e-6
