"""The moving camera on the GPU (camera_motion.py has the helpers and says where each expected value comes from).

The oracle is unchanged and renders the start transform of any scene, so it is the yardstick wherever the reference's rules
make the moving camera equal to some static one -- every time before the start, every time after the end, an interpolation
that is exact in float -- and the source of every ingredient elsewhere: time samples, camera-space rays, closest hits.
EXACT bar: the oracle with correctly rounded libm calls, counters equal (2 counts of slack), film
relative L2 < 1e-6, every pixel within 2e-4 of the mean."""
import numpy as np
import pytest

import camera_motion as cm
import metadata_scenes as ms
import scenes_text as st

pytestmark = pytest.mark.gpu

START, END = "3 2 8  0 0.5 0  0 1 0", "6 3 5  0.5 0 -1  0.1 1 0"
COUNTER_KEYS = ("regular_rays", "shadow_rays", "total_paths", "zero_radiance_paths", "path_length_sum")


def _rel_l2(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / max((b ** 2).sum(), 1e-30)))


def _exact_bar(name, film, weight, c, oracle, spp):
    ofilm, oweight, oc = oracle
    o = oc.as_dict()
    rel = _rel_l2(film, ofilm)
    l2 = np.sqrt(((film.astype(np.float64) - ofilm) ** 2).mean(axis=2)) / spp
    mean = max(float(ofilm.mean()) / spp, 1e-12)
    print("%s: relative L2 %.3e, worst pixel %.3e of the mean, counter differences %s"
          % (name, rel, l2.max() / mean, [c[k] - o[k] for k in COUNTER_KEYS]))
    assert ofilm.any() and not np.isnan(film).any()
    assert np.array_equal(weight, oweight)
    assert c["camera_rays"] == o["camera_rays"] and c["bad_samples"] == o["bad_samples"] == 0
    for k in COUNTER_KEYS:
        assert abs(c[k] - o[k]) <= 2, (k, c[k], o[k])
    assert rel < 1e-6, rel
    assert l2.max() / mean < 2e-4


def _oracle(ob, scene):
    with ob.exact_libm():
        return ob.render(scene)[:3]


def _device(pt, scene, **render):
    integ = pt.CreateIntegrator(scene)
    film, weight = integ.Render(**render)
    return film, weight, integ.counters.as_dict()


# ---------------------------------------------------------------------------------------------------------------------
# 5: the boundary rules
def test_equal_members_render_as_the_static_camera(pt, ob):
    cam = ('ActiveTransform StartTime\nLookAt %s\nActiveTransform EndTime\nLookAt %s\nActiveTransform All\n'
           'Camera "perspective" "float fov" [45]\n' % (START, START))
    s = pt.Scene(text=cm.lit_scene(cam))
    assert s.errors == [] and s.desc.camera.animated == 0
    static = pt.Scene(text=cm.lit_scene(cm.static_camera(START)))
    film, weight, c = _device(pt, s)
    _exact_bar("equal members", film, weight, c, _oracle(ob, static), 4)


@pytest.mark.parametrize("sampler", ["halton", "sobol", "random", "02sequence", "stratified"])
def test_every_time_before_the_start_takes_the_start_transform(pt, ob, sampler):
    """TransformTimes 2 3, shutter 0..1: time <= startTime for every ray."""
    s = pt.Scene(text=cm.lit_scene(cm.moving_camera(START, END, (2, 3)), sampler=sampler))
    assert s.errors == [] and s.desc.camera.animated == 1 and s.spp == 4
    film, weight, c = _device(pt, s)
    _exact_bar("before the start, " + sampler, film, weight, c, _oracle(ob, s), 4)


def test_every_time_after_the_end_takes_the_end_transform(pt, ob):
    """TransformTimes -2 -1: time >= endTime for every ray; the oracle renders the twin with the members swapped."""
    s = pt.Scene(text=cm.lit_scene(cm.moving_camera(START, END, (-2, -1))))
    twin = pt.Scene(text=cm.lit_scene(cm.moving_camera(END, START, (-2, -1))))
    assert s.errors == [] and twin.errors == [] and s.desc.camera.animated == 1
    assert list(twin.desc.camera.camera_to_world) == list(s.desc.camera.camera_to_world_end)
    film, weight, c = _device(pt, s)
    ofilm = _oracle(ob, twin)
    _exact_bar("after the end", film, weight, c, ofilm, 4)
    assert _rel_l2(film, _oracle(ob, s)[0]) > 0.1   # and that is another picture than the start's


def test_spectralpath_bands_restart_with_the_same_camera_ray(pt, ob):
    s = pt.Scene(text=cm.lit_scene(cm.moving_camera(START, END, (2, 3)),
                                   integrator='Integrator "spectralpath" "integer numCABands" [2] "integer maxdepth" [3]'))
    assert s.errors == [] and s.desc.camera.animated == 1 and s.desc.integrator.n_ca_bands == 2
    film, weight, c = _device(pt, s)
    _exact_bar("spectralpath before the start", film, weight, c, _oracle(ob, s), 4)


# ---------------------------------------------------------------------------------------------------------------------
# 6: an interpolation that is exact in float
HALF = '"float fov" [45] "float shutteropen" [.5] "float shutterclose" [.5]'
LENS = HALF + ' "float lensradius" [.05] "float focaldistance" [7]'
AXIS_START, AXIS_END, AXIS_MID = "0 1 6  0 1 5  0 1 0", "2 3 4  2 3 3  0 1 0", "1 2 5  1 2 4  0 1 0"


def _exact_midpoint(pt, ob, text_of, camera, name, **scene_kw):
    s = pt.Scene(text=text_of(cm.moving_camera(AXIS_START, AXIS_END, (0, 1), camera)), **scene_kw)
    mid = pt.Scene(text=text_of(cm.static_camera(AXIS_MID, camera)), **scene_kw)
    assert s.errors == [] and mid.errors == [] and s.desc.camera.animated == 1
    # the premise, on the CPU: every ray's time is 0.5, strictly between the transform times, and the float32 interpolation
    # there is the static camera at the midpoint, bit for bit up to the sign of zeros
    times = cm.ray_times(s, cm.time_samples(ob, s, cm.frame_samples(s, 256)))
    assert np.all(times == np.float32(0.5)) and s.desc.camera.transform_start < 0.5 < s.desc.camera.transform_end
    a = cm.animated_of(s)
    assert cm.same_up_to_zero_signs(a.interpolate(0.5), list(mid.desc.camera.camera_to_world))
    assert not cm.same_up_to_zero_signs(list(s.desc.camera.camera_to_world), list(mid.desc.camera.camera_to_world))
    film, weight, c = _device(pt, s)
    _exact_bar(name, film, weight, c, _oracle(ob, mid), s.spp)


def test_interpolated_transform_on_the_lit_scene(pt, ob):
    _exact_midpoint(pt, ob, cm.lit_scene, HALF, "midpoint, lit scene")


def test_interpolated_transform_carries_the_differentials(pt, ob, tmp_path):
    """An image-textured quad through a lens: the EWA footprint comes from the camera differentials, which k_shade rebuilds
    with the transform at the ray's time."""
    st.write_texture_files(str(tmp_path))
    _exact_midpoint(pt, ob, cm.textured_scene, LENS, "midpoint, textured quad through a lens", base_dir=str(tmp_path))


# ---------------------------------------------------------------------------------------------------------------------
# 7, 8: a general motion -- a rotation of 34.5 degrees, a translation of 8.8 units, a non-uniform scale of the end member
MOTION = dict(start="8 5 30  8 5 0  0 1 0", end="15 7 25  0 4 2  0.2 1 0", times=(0.5, 2), camera='"float fov" [60]',
              end_extra="Scale 1 1.1 0.95\n")
IDENTITY_CAMERA = 'Camera "perspective" "float fov" [60]\n'
_motion = {}


def _motion_scene(pt, sampler="halton", **kw):
    text = cm.metadata_scene(cm.moving_camera(**MOTION), **kw)
    twin = cm.metadata_scene(IDENTITY_CAMERA, **kw)
    if sampler != "halton":
        text, twin = (t.replace('Sampler "halton"', 'Sampler "%s"' % sampler) for t in (text, twin))
    s, ident = pt.Scene(text=text), pt.Scene(text=twin)
    assert s.errors == [] and ident.errors == [] and s.desc.camera.animated == 1
    assert list(ident.desc.camera.camera_to_world) == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
    return s, ident


def _ray_bars(pt, ob, sampler="halton"):
    """256 samples over the 64 x 64 frame: the samples, their times, the oracle's start-scene rays, the restatements in
    float32 and float64, and the bars for origins and directions: four times the worst deviation of the float32 restatement
    from the float64 one over the interpolated samples (a different but legitimate operation order and contraction on the
    device), never below 8 ulp of the largest component."""
    if sampler not in _motion:
        s, ident = _motion_scene(pt, sampler, res=(64, 64), spp=4)
        samples = cm.frame_samples(s, 256, spp=4)
        times = cm.ray_times(s, cm.time_samples(ob, s, samples))
        cam = ob.camera_rays(ident, samples)
        r32 = cm.restated_rays(cm.animated_of(s), cam, times)
        r64 = cm.restated_rays(cm.animated_of(s, np.float64), cam, times)
        mid = times > np.float32(0.5)
        assert np.all(times < np.float32(2))
        bar_o = max(4 * np.abs(r32[mid, :3] - r64[mid, :3]).max(), 8 * float(np.spacing(np.float32(np.abs(r64[mid, :3]).max()))))
        bar_d = max(4 * np.abs(r32[mid, 3:6] - r64[mid, 3:6]).max(), 8 * float(np.spacing(np.float32(np.abs(r64[mid, 3:6]).max()))))
        _motion[sampler] = dict(scene=s, samples=samples, times=times, start_rays=ob.camera_rays(s, samples), r32=r32, r64=r64,
                                mid=mid, bar_o=float(bar_o), bar_d=float(bar_d))
    return _motion[sampler]


@pytest.mark.parametrize("sampler", ["halton", "02sequence"])
def test_camera_rays_of_a_general_motion(pt, ob, sampler):
    m = _ray_bars(pt, ob, sampler)
    s, mid = m["scene"], m["mid"]
    if sampler == "halton":   # the time sample is dimension 2 of the sample's index
        u = cm.time_samples(ob, s, m["samples"][:32])
        dim2 = [ob.lib().oracle_sample_dimension(s.desc_ptr, px, py, n, 2) for px, py, n in m["samples"][:32]]
        assert np.array_equal(u, np.array(dim2, np.float32))
    assert 0.3 <= mid.mean() <= 0.7, mid.mean()
    # the float32 restatement of the start side is the oracle's camera ray, bit for bit
    assert np.array_equal(m["r32"][~mid].view(np.uint32), m["start_rays"][~mid].view(np.uint32))
    integ = pt.CreatePathIntegrator(s)
    dev = integ.camera_rays(m["samples"])
    assert np.array_equal(dev[:, 7].view(np.uint32), m["times"].view(np.uint32))
    assert np.array_equal(dev[~mid, :7].view(np.uint32), m["start_rays"][~mid].view(np.uint32))
    worst_o = float(np.abs(dev[mid, :3].astype(np.float64) - m["r64"][mid, :3]).max())
    worst_d = float(np.abs(dev[mid, 3:6].astype(np.float64) - m["r64"][mid, 3:6]).max())
    print("%s: origins worst %.3e (bar %.3e), directions worst %.3e (bar %.3e), %d of 256 interpolated; device vs float32 "
          "restatement: %d ulp" % (sampler, worst_o, m["bar_o"], worst_d, m["bar_d"], int(mid.sum()),
                                   cm.ulp_distance(dev[mid, :6], m["r32"][mid, :6])))
    assert worst_o <= m["bar_o"] and worst_d <= m["bar_d"]
    assert np.all(np.isinf(dev[:, 6]))


def _sample_footprints(ob, scene, samples):
    """The pixels of the cropped film each sample is added to (FilmTile::AddSample with the box filter, film.h:131-141), as
    metadata_scenes.Expected works them out."""
    d = scene.desc
    cb, r = list(d.film.cropped_bounds), np.array(list(d.film.filter_radius), np.float32)
    out = []
    for px, py, n in samples:
        u = [np.float32(ob.lib().oracle_sample_dimension(scene.desc_ptr, px, py, n, k)) for k in (0, 1)]
        dx, dy = np.float32(px) + u[0] - np.float32(0.5), np.float32(py) + u[1] - np.float32(0.5)
        x0, x1 = max(int(np.ceil(dx - r[0])), cb[0]), min(int(np.floor(dx + r[0])) + 1, cb[2])
        y0, y1 = max(int(np.ceil(dy - r[1])), cb[1]), min(int(np.floor(dy + r[1])) + 1, cb[3])
        out.append((y0 - cb[1], y1 - cb[1], x0 - cb[0], x1 - cb[0]))
    return out


def _motion_maps(pt, ob):
    """Scene 8 at 64 x 64, 1 spp: the expected maps of the restated float32 rays, the pixels to leave out, the first-order
    bounds of depth and coordinates per pixel, and the pixels all of whose samples lie on the start side."""
    if "maps" not in _motion:
        bars = _ray_bars(pt, ob)
        s, ident = _motion_scene(pt, res=(64, 64), spp=1)
        samples = cm.all_samples(s, 1)
        times = cm.ray_times(s, cm.time_samples(ob, s, samples))
        rays = cm.restated_rays(cm.animated_of(s), ob.camera_rays(ident, samples), times)
        start = times <= np.float32(0.5)
        # on the start side the restated ray IS the oracle's camera ray of the start scene, so there the expected maps are
        # the start scene's expected maps
        assert np.array_equal(rays[start].view(np.uint32), ob.camera_rays(s, samples)[start].view(np.uint32))
        exp = cm.expected_maps(pt, ob, s, rays, 1)
        prim, depth, p = cm.hit_values(ob, s, rays)
        unstable = np.zeros(len(rays), bool)
        bound_depth, bound_p = np.zeros(len(rays)), np.zeros((len(rays), 3))
        for comp in range(6):
            vals = []
            for sign in (-1.0, 1.0):
                q = rays.copy()
                q[:, comp] += np.float32(sign * (bars["bar_o"] if comp < 3 else bars["bar_d"]))
                vals.append(cm.hit_values(ob, s, q))
                unstable |= vals[-1][0] != prim
            with np.errstate(invalid="ignore"):
                bound_depth += 0.5 * np.abs(vals[1][1].astype(np.float64) - vals[0][1])
                bound_p += 0.5 * np.abs(vals[1][2].astype(np.float64) - vals[0][2])
        w, h = s.film_size
        left_out, on_start = np.zeros((h, w), bool), np.ones((h, w), bool)
        bd, bp = np.zeros((h, w)), np.zeros((h, w, 3))
        hit = prim >= 0
        for i, (y0, y1, x0, x1) in enumerate(_sample_footprints(ob, s, samples)):
            left_out[y0:y1, x0:x1] |= unstable[i]
            on_start[y0:y1, x0:x1] &= start[i]
            if hit[i] and not unstable[i]:
                bd[y0:y1, x0:x1] += bound_depth[i]
                bp[y0:y1, x0:x1] += bound_p[i]
        share = left_out.mean()
        print("left out: %.2f %% of the pixels; %.1f %% of the samples hit something; %.1f %% on the start side"
              % (100 * share, 100 * hit.mean(), 100 * start.mean()))
        assert share <= 0.02, share
        assert 0.1 < hit.mean() < 0.9 and 0.3 <= start.mean() <= 0.7
        _motion["maps"] = dict(scene=s, exp=exp, keep=~left_out, on_start=on_start & ~left_out, bound_depth=bd, bound_p=bp,
                               integ=pt.MetadataIntegrator(s))
    return _motion["maps"]


@pytest.mark.parametrize("strategy", ms.STRATEGIES)
def test_maps_of_a_general_motion(pt, ob, strategy):
    m = _motion_maps(pt, ob)
    exp, keep = m["exp"], m["keep"]
    film, weight = m["integ"].Render(strategy=strategy)
    c = m["integ"].counters.as_dict()
    assert c["camera_rays"] == c["regular_rays"] == exp.n_samples and c["bad_samples"] == 0
    assert np.array_equal(weight, exp.weight)
    want = exp.film[strategy]
    assert want[keep].any()
    if strategy in ("mesh", "material"):
        assert np.array_equal(film[keep], want[keep])
    else:
        bound = m["bound_depth"][..., None] if strategy == "depth" else m["bound_p"]
        n = bound.shape[2]
        diff = np.abs(film[..., :n].astype(np.float64) - want[..., :n])
        ok = diff <= 2 * bound
        print("%s: worst difference %.3e, worst bound %.3e, worst ratio %.3f" %
              (strategy, diff[keep].max(), bound[keep].max(), (diff[keep] / np.maximum(2 * bound[keep], 1e-30)).max()))
        assert np.all(ok[keep]), np.argwhere(~ok & keep[..., None])[:8]
        assert np.array_equal(film[..., n:][keep], want[..., n:][keep])   # the other bins: copies of the value (depth), zeros
    on_start = m["on_start"]
    assert on_start.sum() > 0.2 * keep.sum()
    assert np.array_equal(film[on_start].view(np.uint32), want[on_start].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 9: known-answer blur
def test_blur_ramp_of_a_translating_camera(pt):
    """The camera slides along +x from -DELTA / 2 to DELTA / 2 during the shutter in front of an emitter that covers x < 0: a
    pixel column that looks at camera-relative x = X sees the emitter while c(t) + X < 0, i.e. for the fraction
    clamp(1/2 - X / DELTA, 0, 1) of the shutter. 64 x 16 at fov 90 on the short axis and distance 1: 8 pixels per unit, so DELTA = 5 is a ramp of 40 pixels.
    Bar 0.03 Le: 1/125 from the base-5 stratification of the time dimension over 125 samples, 0.5/40 from the pixel
    footprint, rounded up."""
    delta = 5.0
    s = pt.Scene(text=cm.blur_scene(delta))
    still = pt.Scene(text=cm.blur_scene(delta, still=True))
    assert s.errors == [] and still.errors == [] and s.desc.camera.animated == 1 and s.spp == 125 and s.film_size == (64, 16)
    le = np.array(list(s.desc.lights[0].L), np.float64)
    assert le.min() > 0.5
    # camera-relative world x of every column's centre on the plane z = 0, from the camera's own matrices
    cam = still.desc.camera
    r2c = np.array(list(cam.raster_to_camera), np.float64).reshape(4, 4)
    c2w = np.array(list(cam.camera_to_world), np.float64).reshape(4, 4)
    X = np.zeros(64)
    for j in range(64):
        pc = r2c @ np.array([j + 0.5, 8.0, 0.0, 1.0])
        dw = c2w[:3, :3] @ (pc[:3] / pc[3])
        X[j] = dw[0] / -dw[2]          # the camera is at z = 1 and looks down -z
    assert abs(abs(X[0]) - (4 - 1 / 16)) < 1e-4 and abs(X[1] - X[0]) * 8 == pytest.approx(1, abs=1e-4)
    ramp = np.clip(0.5 - X / delta, 0.0, 1.0)
    step = (X < delta / 2).astype(np.float64)   # the camera at rest at the start position
    inside = (ramp > 0) & (ramp < 1)
    assert inside.sum() == 40 and (ramp == 1).sum() >= 4 and (ramp == 0).sum() >= 4
    assert np.abs(step - ramp).max() > 0.4         # the scene without the motion is a step: it misses the bar by far
    film, weight = pt.CreateIntegrator(s).Render()
    assert weight.min() > 0
    img = film.astype(np.float64) / weight[..., None] / le     # per bin, in units of Le
    col = img.mean(axis=(0, 2))
    print("blur ramp: worst column deviation %.4f Le inside the ramp, %.2e outside" %
          (np.abs(col - ramp)[inside].max(), np.abs(col - ramp)[~inside].max()))
    assert np.all(np.abs(col - ramp) <= 0.03)
    assert np.abs(col - ramp)[~inside].max() < 1e-5
    assert np.abs(step - ramp).max() > 0.03


# ---------------------------------------------------------------------------------------------------------------------
# 10: schedule invariance
@pytest.mark.parametrize("what", ["depth", "path"])
def test_schedules_give_the_same_frame(pt, what):
    """64 x 64 x 4 spp behind the moving camera of scene 8: a 256-slot pool, three shards added together and two accumulated
    passes over sample ranges, each against the frame of one pass on the default pool (relative L2 < 1e-6: float atomics)."""
    if what == "depth":
        s, _ = _motion_scene(pt, res=(64, 64), spp=4)
        integ = pt.MetadataIntegrator(s)
        kw = dict(strategy="depth")
    else:
        s, _ = _motion_scene(pt, res=(64, 64), spp=4, integrator='Integrator "path" "integer maxdepth" [3]')
        integ = pt.PathIntegrator(s)
        kw = {}
    n = 64 * 64 * 4
    ref, wref = integ.Render(**kw)
    assert ref.any() and integ.counters.camera_rays == n

    def same(film, weight, how):
        rel = _rel_l2(film, ref)
        print("%s, %s: relative L2 %.3e" % (what, how, rel))
        assert np.array_equal(weight, wref), how
        assert rel < 1e-6, (how, rel)

    film, weight = integ.Render(path_pool=256, **kw)
    assert integ.pool_info()[0] == 256
    same(film, weight, "256-slot pool")
    acc, wacc, cams = np.zeros_like(ref), np.zeros_like(wref), 0
    for r in range(3):
        f, w = integ.Render(shard_index=r, shard_count=3, **kw)
        acc += f
        wacc += w
        cams += integ.counters.camera_rays
    assert cams == n
    same(acc, wacc, "three shards")
    integ.Render(spp=2, sample_begin=0, download=False, **kw)
    film, weight = integ.Render(spp=2, sample_begin=2, accumulate=True, **kw)
    same(film, weight, "two passes")
