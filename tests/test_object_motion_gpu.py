"""Object motion on the GPU (MIPT_OBJECT_MOTION=1; object_motion.py has the helpers).

The oracle is unchanged: it ignores an instance's motion record and renders its i2w / w2i. So it is the yardstick wherever
the reference's rules make the moving primitive equal to a static one: every ray's time before the start (the scene as it
stands), after the end (the twin with the members swapped), and -- the whole path at an interpolated transform -- a shutter
frozen at one time, where the twin is the same scene with the float32 restatement of Interpolate(time) and of its inverse
written into the instance. EXACT bar (test_camera_motion_gpu.py): weights equal, counters within 2, film relative L2 <
1e-6, every pixel within 2e-4 of the mean. Films of 32 x 24 at 4 spp on a path pool of 256 slots: several iterations, slots
reused by new camera samples with other times."""
import numpy as np
import pytest

import camera_motion as cm
import object_motion as om
from test_camera_motion_gpu import _device, _exact_bar, _oracle, _rel_l2

pytestmark = pytest.mark.gpu

# a general pair: the object crosses a third of the frame, turns by 70 degrees and changes its non-uniform scale
GENERAL = ("Translate -1.6 0.4 2.5\nScale 1.2 1.6 1", "Translate 1.4 1.1 3\nRotate 70 0.3 1 0.2\nScale 1.5 0.8 1.3")
TRANSLATION = ("Translate -1.6 0.4 2.5", "Translate 1.4 1.1 3")
SPECTRAL = 'Integrator "spectralpath" "integer numCABands" [2] "integer maxdepth" [3]'
FROZEN = '"float fov" [45] "float shutteropen" [.5] "float shutterclose" [.5]'
POOL = dict(path_pool=256)


@pytest.fixture(autouse=True)
def on(monkeypatch):
    monkeypatch.setenv("MIPT_OBJECT_MOTION", "1")


def _moving(pt, kind, members, **kw):
    s = pt.Scene(text=om.lit_scene(om.mover(kind, *members), **kw))
    assert s.errors == [] and s.desc.n_motions == 1 and s.desc.n_instances == 1
    return s


# ---------------------------------------------------------------------------------------------------------------------
# 1: the boundary rules
@pytest.mark.parametrize("kind", ["instance", "shape"])
@pytest.mark.parametrize("sampler", ["halton", "sobol", "random", "02sequence", "stratified"])
def test_every_time_before_the_start_takes_the_start_member(pt, ob, kind, sampler):
    """TransformTimes 2 3, shutter 0..1: time <= startTime for every ray; the oracle renders the same scene."""
    s = _moving(pt, kind, GENERAL, times=(2, 3), sampler=sampler)
    film, weight, c = _device(pt, s, **POOL)
    _exact_bar("%s before the start, %s" % (kind, sampler), film, weight, c, _oracle(ob, s), 4)


@pytest.mark.parametrize("kind", ["instance", "shape"])
@pytest.mark.parametrize("integrator", ['Integrator "path" "integer maxdepth" [4]', SPECTRAL])
def test_every_time_after_the_end_takes_the_end_member(pt, ob, kind, integrator):
    """TransformTimes -2 -1: time >= endTime for every ray; the oracle renders the twin with the members swapped."""
    s = _moving(pt, kind, GENERAL, times=(-2, -1), integrator=integrator)
    twin = _moving(pt, kind, GENERAL[::-1], times=(-2, -1), integrator=integrator)
    assert list(twin.desc.instances[0].i2w) == list(s.desc.motions[0].i2w_end)
    assert list(twin.desc.instances[0].w2i) == list(s.desc.motions[0].w2i_end)
    film, weight, c = _device(pt, s, **POOL)
    _exact_bar("%s after the end" % kind, film, weight, c, _oracle(ob, twin), 4)
    assert _rel_l2(film, _oracle(ob, s)[0]) > 0.1   # and that is another picture than the start's


@pytest.mark.parametrize("kind", ["instance", "shape"])
def test_spectralpath_bands_restart_with_the_same_time(pt, ob, kind):
    s = _moving(pt, kind, GENERAL, times=(2, 3), integrator=SPECTRAL)
    assert s.desc.integrator.n_ca_bands == 2
    film, weight, c = _device(pt, s, **POOL)
    _exact_bar("%s, spectralpath before the start" % kind, film, weight, c, _oracle(ob, s), 4)


# ---------------------------------------------------------------------------------------------------------------------
# 2: a frozen shutter -- camera, shadow and MIS rays all interpolate at dt = 0.5
def _frozen_pair(pt, ob, kind, members, **kw):
    s = _moving(pt, kind, members, camera=FROZEN, **kw)
    twin = _moving(pt, kind, members, camera=FROZEN, **kw)
    times = cm.ray_times(s, cm.time_samples(ob, s, cm.frame_samples(s, 256)))
    mo = s.desc.motions[0]
    assert np.all(times == np.float32(0.5)) and mo.transform_start < 0.5 < mo.transform_end
    m, minv = om.matrices_at(s, 0, 0.5)
    assert not cm.same_up_to_zero_signs(m, list(s.desc.instances[0].i2w)) and not cm.same_up_to_zero_signs(m, list(mo.i2w_end))
    om.set_instance(twin, 0, m, minv)
    return s, twin


@pytest.mark.parametrize("kind", ["instance", "shape"])
@pytest.mark.parametrize("name, members", [("translation", TRANSLATION), ("rotation and scale", GENERAL)])
def test_the_whole_path_at_an_interpolated_transform(pt, ob, kind, name, members):
    """maxdepth 4 under a point light and an area light: shadow and MIS rays cross the instance at the camera ray's time.
    The twin carries the float32 restatement of the interpolated matrix and of the inverse its product brings (for the
    translation these are Translate(lerp) and its stored inverse: test_object_motion_frontend.py)."""
    s, twin = _frozen_pair(pt, ob, kind, members)
    film, weight, c = _device(pt, s, **POOL)
    oracle = _oracle(ob, twin)
    _exact_bar("%s, %s at dt = 0.5" % (kind, name), film, weight, c, oracle, 4)
    assert _rel_l2(oracle[0], _oracle(ob, s)[0]) > 0.05   # (the start member's picture is another one)


@pytest.mark.parametrize("kind", ["instance", "shape"])
def test_spectralpath_bands_at_an_interpolated_transform(pt, ob, kind):
    """A band that restarts keeps the slot's time: with the shutter frozen at 0.5 every band's path crosses the instance at
    the interpolated transform, or the picture is not the twin's."""
    s, twin = _frozen_pair(pt, ob, kind, GENERAL, integrator=SPECTRAL)
    film, weight, c = _device(pt, s, **POOL)
    _exact_bar("%s, spectralpath at dt = 0.5" % kind, film, weight, c, _oracle(ob, twin), 4)


@pytest.mark.parametrize("kind", ["instance", "shape"])
def test_the_pool_size_does_not_change_a_moving_render(pt, ob, kind):
    """Shutter 0..1 across the interval: every sample has a time of its own. The default pool holds the frame in one
    generation, 256 slots refill a dozen times; the time travels with the slot either way."""
    s = _moving(pt, kind, GENERAL)
    film, weight, c = _device(pt, s)
    film2, weight2, c2 = _device(pt, s, **POOL)
    print("pool 256 against the default: relative L2 %.3e, bit-equal %s" % (_rel_l2(film2, film), np.array_equal(film, film2)))
    # the bar test_render_schedule_gpu.py holds static scenes to across pool sizes (the film's sums come in another order)
    assert np.array_equal(weight, weight2) and c["camera_rays"] == c2["camera_rays"]
    for k in ("regular_rays", "shadow_rays", "total_paths", "zero_radiance_paths", "path_length_sum"):
        assert abs(c[k] - c2[k]) <= 2, k
    assert _rel_l2(film2, film) < 1e-6
    # and the motion is in the picture: neither member's
    assert _rel_l2(film, _oracle(ob, s)[0]) > 0.05


@pytest.mark.parametrize("kind", ["instance", "shape"])
def test_shards_passes_and_sub_renderers_add_up_to_the_single_render(pt, ob, monkeypatch, kind):
    """Two tile shards, each in two passes over sample ranges, on two sub-renderers (MIPT_STREAMS=2; 512 slots: one
    256-slot block each): films, weights and counters summed against the single render of the whole frame, at the bar
    test_render_schedule_gpu.py holds static scenes to (2 counts of slack per render)."""
    s = _moving(pt, kind, GENERAL)
    film, weight, c = _device(pt, s)
    monkeypatch.setenv("MIPT_STREAMS", "2")   # (read when the renderer is created)
    integ = pt.CreateIntegrator(s)
    acc, accw, total = np.zeros_like(film), np.zeros_like(weight), dict.fromkeys(c, 0)
    for r in range(2):
        integ.Render(shard_index=r, shard_count=2, spp=1, sample_begin=0, download=False, path_pool=512)
        first = integ.counters.as_dict()
        f, w = integ.Render(shard_index=r, shard_count=2, spp=3, sample_begin=1, accumulate=True, path_pool=512)
        acc += f
        accw += w
        for k in total:
            total[k] += first[k] + integ.counters.as_dict()[k]
    print("2 shards x 2 passes on 2 sub-renderers against the single render: relative L2 %.3e" % _rel_l2(acc, film))
    assert np.array_equal(accw, weight) and total["camera_rays"] == c["camera_rays"] == 32 * 24 * 4
    for k in ("regular_rays", "shadow_rays", "total_paths", "zero_radiance_paths", "path_length_sum"):
        assert abs(total[k] - c[k]) <= 2 * 4, k
    assert _rel_l2(acc, film) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# 4: the metadata maps of a frozen shutter against the same renderer on the static twin
@pytest.mark.parametrize("kind", ["instance", "shape"])
def test_metadata_maps_at_an_interpolated_transform(pt, ob, kind):
    """One sample per pixel, box filter: a pixel holds the sum of the samples that fell into it (one, sometimes none or
    two), and a sum of small whole numbers is exact. The twin is static (its motion index cleared), so
    the device's own static path -- which test_metadata_gpu.py holds to the oracle -- says what depth, material and
    coordinates are; `mesh` is the instance's number for a moving instance and 0 for a moving shape (a static instance
    without a number of its own reports its index + 1, as the oracle does)."""
    meta = 'Integrator "metadata" "string strategy" "depth"'
    s, twin = _frozen_pair(pt, ob, kind, GENERAL, integrator=meta, spp=1)
    twin.desc.instances[0].motion = 0
    twin.desc.n_motions = 0
    moving, static = pt.MetadataIntegrator(s), pt.MetadataIntegrator(twin)
    seen = None
    for strategy in ("depth", "material", "coordinates", "mesh"):
        film, weight = moving.Render(strategy=strategy, **POOL)
        want, want_weight = static.Render(strategy=strategy, **POOL)
        assert np.array_equal(weight, want_weight) and want.any()
        if strategy == "mesh":
            assert np.array_equal(want, np.round(want)) and want.min() == 0 and want.max() <= 2   # id 1, once or twice
            seen = want[..., 0] >= 1
            if kind == "shape":
                want = np.zeros_like(want)
        assert np.array_equal(film.view(np.uint32), want.view(np.uint32)), (strategy, np.argwhere(film != want)[:8])
    assert 20 < seen.sum() < seen.size   # the object covers part of the frame


# ---------------------------------------------------------------------------------------------------------------------
# 3: per ray -- times before, at, one float either side of and between the transform times
T0, T1 = 0.25, 1.5
TIMES = np.array([-1, np.nextafter(np.float32(T0), np.float32(-9)), T0, np.nextafter(np.float32(T0), np.float32(9)), 0.9,
                  np.nextafter(np.float32(T1), np.float32(-9)), T1, np.nextafter(np.float32(T1), np.float32(9)), 3], np.float32)
WITH_SPHERE = om.OCTAHEDRON + 'Translate 0 .9 0\nShape "sphere" "float radius" [.5]\n'


# five concentric world spheres around the whole scene, the camera inside them: every ray meets their boxes first and postpones
# them, with the scene's two others more quadrics than its list holds, and the overflow path traverses the ray again from the
# world's root -- through the moving instance, whose hit lies in front of the shells
SHELLS = "".join('Shape "sphere" "float radius" [%g]\n' % r for r in (14, 14.1, 14.2, 14.3, 14.4))


GENERAL2 = ("Translate 1.2 -0.2 1.5\nRotate 30 0 0 1", "Translate -1.0 0.6 2.0\nRotate -60 1 0.5 0\nScale 0.8 1.2 1")


def _block(kind, shape):
    if kind == "two":
        return om.two_movers(GENERAL, GENERAL2)
    return om.mover(kind, *GENERAL, shape=shape)


def _near_rays(rays, prim32, t32, of_object):
    """Up to 180 of the rays that hit a moving object, twice each: tMax short of the hit and beyond it -- by one float where
    the time is at or outside the transform times, by 2^-12 of t inside the interval."""
    on = np.nonzero((prim32 >= 0) & of_object[np.maximum(prim32, 0)])[0][:180]
    assert len(on) > 60
    near = np.repeat(rays[on], 2, axis=0)
    exact = (near[:, 7] <= T0) | (near[:, 7] >= T1)
    t = np.repeat(t32[on], 2)
    side = np.tile(np.array([-1, 1], np.float32), len(on))
    near[:, 6] = np.where(exact, np.nextafter(t, np.where(side < 0, np.float32(0), np.float32(np.inf))), t * (np.float32(1) + side * np.float32(2.0 ** -12)))
    return near, on


def _check_rays(ob, s, twin, integ, rays, family):
    """One family of rays [n, 8] through k_trace against the oracle in the twin, time by time. Returns the device's answers,
    the float32 expectation's primitive and t, and how many rays the motion sends elsewhere than the start member does."""
    got = integ.trace(rays)
    got_any = integ.trace(rays, any_hit=True)[:, 0].view(np.int32) >= 0
    prim = got[:, 0].copy().view(np.int32)
    prim32, t32 = np.full(len(rays), -1, np.int32), np.zeros(len(rays), np.float32)
    moved = 0
    for time in np.unique(rays[:, 7]):
        sel = rays[:, 7] == time
        om.set_moving(s, twin, time)
        with ob.exact_libm():
            want, _ = ob.trace(twin, rays[sel, :7])
            want_any = ob.trace(twin, rays[sel, :7], any_hit=True)[0][:, 0].view(np.int32) >= 0
        wprim = want[:, 0].copy().view(np.int32)
        prim32[sel], t32[sel] = wprim, want[:, 1]
        if time <= T0 or time >= T1:
            # (the primitive and t: the oracle's probe works its barycentrics out with the world ray, which says nothing
            # inside an instance)
            assert np.array_equal(got[sel][:, :2].view(np.uint32), want[:, :2].view(np.uint32)), (family, time)
            assert np.array_equal(got_any[sel], want_any), (family, time)
        else:
            # the rule: unsure where the float64 restatement (rounded to float32 for the oracle) finds another primitive or
            # another verdict, held to either, at most 1 %; t within four times the float32 / float64 deviation of the family
            om.set_moving(s, twin, time, np.float64)
            with ob.exact_libm():
                want64, _ = ob.trace(twin, rays[sel, :7])
                any64 = ob.trace(twin, rays[sel, :7], any_hit=True)[0][:, 0].view(np.int32) >= 0
            wprim64 = want64[:, 0].copy().view(np.int32)
            unsure = wprim != wprim64
            both = ~unsure & (wprim >= 0)
            bar = om.rule_bar(want[:, 1], want64[:, 1], both)
            same = prim[sel] == wprim
            worst = float(np.abs(got[sel][both & same, 1].astype(np.float64) - want64[both & same, 1]).max()) if (both & same).any() else 0.0
            print("%s, time %r: %d of %d rays unsure, %d with the float64 answer; t worst %.3e, bar %.3e"
                  % (family, float(time), unsure.sum(), same.size, (~same).sum(), worst, bar))
            assert unsure.sum() <= 0.01 * same.size and (want_any != any64).sum() <= 0.01 * same.size
            assert np.all(same | (prim[sel] == wprim64))
            assert np.all(same[~unsure]) and worst <= bar
            assert np.all((got_any[sel] == want_any) | (got_any[sel] == any64))
        if time > T0:
            om.set_moving(s, twin, -1)
            with ob.exact_libm():
                moved += int((ob.trace(twin, rays[sel, :7])[0][:, 0].view(np.int32) != wprim).sum())
    return got, prim32, t32, moved


@pytest.mark.parametrize("kind, shape, world", [("instance", om.OCTAHEDRON, ""), ("shape", om.OCTAHEDRON, ""), ("instance", WITH_SPHERE, ""),
                                                ("instance", om.OCTAHEDRON, SHELLS), ("shape", om.OCTAHEDRON, SHELLS), ("two", om.OCTAHEDRON, "")],
                         ids=["instance", "shape", "instance with a sphere", "instance, overflowing lists", "shape, overflowing lists",
                              "two instances of one object"])
def test_rays_with_times_of_their_own(pt, ob, kind, shape, world):
    """The probes take a time per ray (rays [n, 8]). Expected: the oracle's answer in the twin that carries the float32
    restatement of every moving instance's matrices at that time. At and outside the transform times these are the members
    themselves and the answers are equal bit for bit. Strictly inside, by the rule (_check_rays). Families: camera rays over
    the frame; rays grazing each object's silhouette at their time (a thousandth and a hundredth of its size inside and
    outside the hull); and rays that hit a moving object again with tMax either side of the hit -- one float at the exact
    times, 2^-12 of t inside the interval, sixty times the deviation there, so that the restatement stays under the cap. The
    render's own kernels then equal the per-ray routine bit for bit at every time."""
    text = om.lit_scene(world + _block(kind, shape), times=(T0, T1))
    s, twin = pt.Scene(text=text), pt.Scene(text=text)
    n_moving = 2 if kind == "two" else 1
    assert s.errors == [] and s.desc.n_motions == n_moving and len(om.moving_instances(s)) == n_moving
    samples = cm.all_samples(s, 4)   # 3 072 rays, 341 per time
    rays = np.zeros((len(samples), 8), np.float32)
    rays[:, :7] = ob.camera_rays(s, samples)
    rays[:, 7] = TIMES[np.arange(len(samples)) % len(TIMES)]
    integ = pt.CreateIntegrator(s)
    got, prim32, t32, moved = _check_rays(ob, s, twin, integ, rays, "frame")
    prim = got[:, 0].copy().view(np.int32)
    graze = om.grazing_rays(s, rays[0, :3], TIMES)
    ggot, gprim, _, _ = _check_rays(ob, s, twin, integ, graze, "grazing")
    of_object = np.arange(s.desc.n_prims) >= s.desc.n_prims - (9 if shape is WITH_SPHERE else 8)
    ghit = of_object[np.maximum(gprim, 0)] & (gprim >= 0)
    assert 0.3 < ghit.mean() < 0.97, ghit.mean()   # those pulled in hit it (unless something stands in front), of those pushed out the silhouette's miss
    near, on = _near_rays(rays, prim32, t32, of_object)
    ngot, nprim, _, _ = _check_rays(ob, s, twin, integ, near, "tMax either side")
    keeps = of_object[np.maximum(nprim, 0)] & (nprim >= 0)
    # short of the hit: not that primitive; 2^-12 beyond it: the object again. (One float beyond decides nothing by itself: the
    # way into the instance shifts the origin and tMax by the origin's error bound, and the device follows the oracle there.)
    inside = (near[1::2, 7] > T0) & (near[1::2, 7] < T1)
    assert np.all(keeps[1::2][inside]) and inside.sum() > 10 and not np.any(keeps[0::2] & (nprim[0::2] == prim32[on]))
    if kind == "two":   # both instances are hit, each at times of its own motion
        inst = integ.trace_wavefront(rays, mode=0)[1][:, 1]
        assert (inst == 0).sum() > 20 and (inst == 1).sum() > 20
    rays = np.concatenate([rays, graze, near])
    got = np.concatenate([got, ggot, ngot])
    prim = got[:, 0].copy().view(np.int32)
    assert moved > 20   # the times matter: with the start member many of these rays hit something else
    # the render's kernels: k_trav<0> + resolve and k_trav<2> + its quadric step against k_trace, bit for bit
    for mode in (0, 2):
        r = rays.copy()
        if mode == 2:
            r[:, 6] = np.inf
            ref = integ.trace(r)
        else:
            ref = got
        hits, extra = integ.trace_wavefront(r, mode=mode)
        assert np.array_equal(hits.view(np.uint32), ref.view(np.uint32)), mode
        if world:   # the lists overflowed, also on rays that end inside the moving object, at times inside the interval
            over = (extra[:, 2] & 0x100) != 0
            inside = (rays[:, 7] > T0) & (rays[:, 7] < T1)
            print("mode %d: %d rays overflowed, %d of them hit through the instance, %d of those strictly inside the interval"
                  % (mode, over.sum(), (over & (extra[:, 1] >= 0)).sum(), (over & (extra[:, 1] >= 0) & inside).sum()))
            assert over.sum() > 50 and (over & (extra[:, 1] >= 0) & inside).sum() > 5
    # k_trav<1>: the shadow form of the rays (an unnormalised direction, tMax = 1 - 0.0001f)
    sh = rays.copy()
    sh[:, 3:6] *= np.float32(12)
    sh[:, 6] = np.float32(1) - np.float32(0.0001)
    ref = integ.trace(sh, any_hit=True)[:, 0].view(np.int32)
    hits, extra = integ.trace_wavefront(sh, mode=1)
    assert np.array_equal(hits[:, 0].view(np.int32) >= 0, ref >= 0) and (ref >= 0).sum() > 50
    if world:
        assert ((extra[:, 2] & 0x100) != 0).sum() > 50
    if shape is WITH_SPHERE:
        shapes = np.array([s.desc.prims[i].shape for i in range(s.desc.n_prims)])
        assert s.desc.n_spheres == 3 and (shapes[prim[prim >= 0]] == ~2).sum() > 10, "no ray hit the moving object's sphere"


# ---------------------------------------------------------------------------------------------------------------------
# 5: the blur ramp
def test_blur_ramp_of_a_moving_edge(pt, ob):
    """A sample sees the quad iff its ray meets the plane z = 0 behind the edge at its own time: x < Lerp(time, -1, 1) in
    float32 (a translation interpolates to a translation). Times and rays are camera_rays_ex's; the radiance of a sample that
    sees the quad is one constant (a matte plane under a distant light, maxdepth 1), taken from the oracle's render of the
    still scene. A pixel of 125 samples then holds count x that constant, up to the rounding of 125 additions (125 x 2^-24 <
    1e-5 relative; the bar is 2e-5). Samples within 1e-5 of the edge are unsure (the hit's x is a handful of float32
    operations on values below 8: 1e-6) and their pixels are left out; at most 1 % may be."""
    delta, res, spp = 2.0, (64, 16), 125
    s = pt.Scene(text=om.ramp_scene(delta, res=res, spp=spp))
    still = pt.Scene(text=om.ramp_scene(delta, still=True, res=res, spp=spp))
    assert s.errors == [] and still.errors == [] and s.desc.n_motions == 1 and still.desc.n_instances == 0
    sfilm, sweight, _ = _oracle(ob, still)
    integ = pt.CreateIntegrator(s)
    samples = cm.all_samples(s, spp)
    r = integ.camera_rays_ex(samples)   # (the one that reports the time in front of a camera that stands still)
    col_x = ((np.float32(0) - r[:, 2]) / r[:, 5] * r[:, 3] + r[:, 0]).reshape(res[1], res[0], spp).mean(axis=(0, 2))
    covered, empty = col_x < -delta / 2 - 0.2, col_x > -delta / 2 + 0.2   # columns of the film the still quad fills / misses
    assert covered.sum() >= 20 and empty.sum() >= 36
    assert not sfilm[:, empty].any()
    lq = sfilm[4, np.argmin(col_x)].astype(np.float64) / sweight[4, np.argmin(col_x)]   # a pixel the still quad covers
    assert lq.min() > 0 and np.allclose(sfilm[:, covered].astype(np.float64) / sweight[:, covered][..., None], lq, rtol=2e-5, atol=0)
    time = r[:, 7]
    assert time.min() >= 0 and time.max() <= 1 and np.unique(time).size > 100
    t_hit = (np.float32(0) - r[:, 2]) / r[:, 5]
    x_hit = r[:, 0] + r[:, 3] * t_hit
    edge = (np.float32(1) - time) * np.float32(-delta / 2) + time * np.float32(delta / 2)
    sees = x_hit < edge
    unsure = np.abs(x_hit.astype(np.float64) - edge) < 1e-5
    print("blur ramp: %d of %d samples within 1e-5 of the edge" % (unsure.sum(), unsure.size))
    assert unsure.sum() <= 0.01 * unsure.size
    count = sees.reshape(res[1], res[0], spp).sum(axis=2)
    skip = unsure.reshape(res[1], res[0], spp).any(axis=2)
    film, weight, c = _device(pt, s, **POOL)
    own = weight == spp   # (a sample on a pixel's very border counts for the neighbour too: some 7 % of the pixels gain one)
    assert own.mean() > 0.9 and c["camera_rays"] == len(samples) and c["bad_samples"] == 0
    use = own & ~skip
    want = count[..., None] * lq
    assert np.allclose(film[use], want[use], rtol=2e-5, atol=0), np.argwhere(~np.isclose(film, want, rtol=2e-5, atol=0))[:8]
    ramp = (count[8] / spp)[np.argsort(col_x)]                     # and it is a ramp: full, a slope of 16 pixels, empty
    assert np.all(ramp[:22] == 1) and np.all(ramp[42:] == 0) and np.all(np.diff(ramp) < 0.06) and 0.35 < ramp[32] < 0.65


@pytest.mark.parametrize("kind", ["instance", "shape", "two"])
def test_metadata_maps_across_the_shutter(pt, ob, kind):
    """Shutter 0..1 over TransformTimes 0.25 1.5: every camera sample has a time of its own, before the start for a quarter
    of them. 32 x 24 at one sample per pixel, box filter. Per sample (camera_rays_ex gives ray and time) the oracle traces
    the ray in the twin that carries the restatement of every moving instance's matrices at that time, in float32 and in
    float64 (rounded for the oracle); depth is |p - o|, coordinates p, material the primitive's id, mesh the number of the
    instance a primitive of the moving object was reached through (0 for a moving shape; with two instances of one object:
    the one whose own scene, the other left out, has the nearer hit). By the rule: a sample is unsure where the two
    restatements find different primitives, at most 1 % may be; depth and coordinates are held to four times the worst
    float32 / float64 deviation over the samples of the interval (never below 8 ulp of the largest value), and bit for bit at
    and before the start time. Pixels that hold exactly their own sample are compared."""
    meta = 'Integrator "metadata" "string strategy" "depth"'
    block = _block(kind, om.OCTAHEDRON)
    text = om.lit_scene(block, times=(T0, T1), res=(32, 24), spp=1, integrator=meta)
    s, twin = pt.Scene(text=text), pt.Scene(text=text)
    assert s.errors == [] and s.desc.n_motions == (2 if kind == "two" else 1)
    integ = pt.MetadataIntegrator(s)
    samples = cm.all_samples(s, 1)
    rays = integ.camera_rays_ex(samples)[:, :8]
    start = rays[:, 7] <= T0
    assert start.sum() > 20 and (~start).sum() > 100
    prim, depth, p = om.expected_hits(ob, s, twin, rays)
    prim64, depth64, p64 = om.expected_hits(ob, s, twin, rays, np.float64)
    unsure = prim != prim64
    print("%s: %d of %d samples unsure" % (kind, unsure.sum(), unsure.size))
    assert unsure.sum() <= 0.01 * unsure.size
    d = s.desc
    of_object = np.arange(d.n_prims) >= d.n_prims - 8   # the object's eight triangles follow the world's primitives
    hit = prim >= 0
    on_object = hit & of_object[np.maximum(prim, 0)]
    assert on_object.sum() > 5
    number = np.ones(len(rays))
    if kind == "shape":
        number[:] = 0
    if kind == "two":   # which instance: each alone in a scene of its own, at its own matrices of the full scene
        alone = []
        for k in range(2):
            one = pt.Scene(text=om.lit_scene(om.two_movers(GENERAL, GENERAL2, only=k), times=(T0, T1), res=(32, 24), spp=1, integrator=meta))
            anim = om.animated_of(s, k)
            dk = np.zeros(len(rays), np.float32)
            for i, r in enumerate(rays):
                om.set_instance(one, 0, *om.matrices_at(s, k, r[7], np.float32, anim))
                a, b, _ = cm.hit_values(ob, one, r[None, :7])
                dk[i] = b[0] if a[0] >= 0 and a[0] >= one.desc.n_prims - 8 else np.inf
            alone.append(dk)
        number = 1.0 + (alone[1] < alone[0])
        assert np.all(np.minimum(alone[0], alone[1])[on_object] == depth[on_object])
        assert (number[on_object] == 1).sum() > 3 and (number[on_object] == 2).sum() > 3
        assert [d.instances[k].instance_id for k in range(2)] == [1, 2]
    mat = np.array([d.prim_meta[i].material_id for i in range(d.n_prims)], np.float32)
    want = {"material": np.where(hit, mat[np.maximum(prim, 0)], 0), "mesh": np.where(on_object, number, 0)}
    both = hit & ~unsure & ~start
    bar_depth = om.rule_bar(depth, depth64, both)
    bar_p = om.rule_bar(p, p64, both)
    shape = (24, 32)
    for strategy in ("depth", "material", "mesh", "coordinates"):
        film, weight = integ.Render(strategy=strategy, **POOL)
        use = ((weight == 1) & ~unsure.reshape(shape)).ravel()
        assert use.mean() > 0.8
        if strategy in ("depth", "coordinates"):
            n = 1 if strategy == "depth" else 3
            got = film.reshape(-1, 31)[:, :n].astype(np.float64)
            ref32 = np.where(hit[:, None], depth[:, None] if n == 1 else p, 0)
            ref64 = np.where(hit[:, None], depth64[:, None] if n == 1 else p64, 0).astype(np.float64)
            bar = bar_depth if n == 1 else bar_p
            worst = float(np.abs(got - ref64)[use & ~start].max())
            print("%s, %s: worst %.3e from the float64 restatement, bar %.3e" % (kind, strategy, worst, bar))
            assert worst <= bar and ref32.any()
            assert np.array_equal(got[use & start].astype(np.float32).view(np.uint32), ref32[use & start].astype(np.float32).view(np.uint32))
            if n == 3:
                assert not film[..., 3:].any()
        else:
            assert np.array_equal(film.reshape(-1, 31)[use, 0], want[strategy][use].astype(np.float32)), strategy
            assert np.array_equal(film[..., 0], film[..., 30])
