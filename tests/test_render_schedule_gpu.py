"""The wavefront driver's operating points against the CPU oracle. Run on the GPU box with `pytest -m gpu`.

The oracle knows nothing of path pools, work runs, passes, shards or sub-renderers, so the device's exact-mode parity with it
(test_gpu_parity._parity: weights equal, camera rays equal, the five counters within 2, film relative L2 < 1e-6, every pixel
within 2e-4 x mean radiance) must hold at every setting of them. test_gpu_parity.py holds the device to the oracle over many
scenes at the driver's defaults, where every scene below 4M camera samples gives each pool slot exactly one path, right after
the pool's state words were cleared. Here the same scenes run through pools of 256 .. a third of the work, so that every slot
is flushed and refilled many times (k_generate's flush, free list, refill and two-ended work list; whatever a finished path
leaves in a slot is what the next one finds), through work runs other than the default, through passes over sample ranges,
shards and several sub-renderers, and through Halton sample numbers whose index does not fit 32 bits.

No tolerance is defined here: the bars are _parity's / _compare's. Every measured figure lands in the metrics file that
test_gpu_parity.py writes (its METRICS list), under a name that carries the schedule."""
import os

import numpy as np
import pytest

from conftest import KILLEROO
import scenes_text as st
from test_gpu_parity import _parity, _compare, _rel_l2, _check_counters, _killeroo_spectralpath, _ZOO_VARIANTS, COUNTER_KEYS, METRICS

pytestmark = pytest.mark.gpu

SMALL_POOLS = (256, 768, 2304)
SAMPLER_TYPE = {"halton": 0, "sobol": 1, "random": 2, "02sequence": 3, "stratified": 4}


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    """One directory with every file the scenes read (textures, alpha mask, environment map)."""
    d = str(tmp_path_factory.mktemp("schedule_assets"))
    st.write_texture_files(d)
    st.write_alpha_png(d)
    st.write_env_pfm(os.path.join(d, "env.pfm"))
    return d


def _zoo_text(sampler, spp=16, res=64):
    """The material zoo under one of the five samplers (stratified: the factorisation of spp the tests name)."""
    txt = st.material_zoo(res=res, spp=spp, depth=6)
    assert 'Sampler "halton"' in txt and '"integer pixelsamples" [%d]' % spp in txt
    txt = txt.replace('Sampler "halton"', 'Sampler "%s"' % sampler)
    if sampler == "stratified":
        xs, ys = {1: (1, 1), 3: (3, 1), 12: (4, 3), 16: (8, 2)}[spp]
        txt = txt.replace('"integer pixelsamples" [%d]' % spp, '"integer xsamples" [%d] "integer ysamples" [%d] "integer dimensions" [3]' % (xs, ys))
    return txt


def _zoo(pt, sampler, spp=16):
    s = pt.Scene(text=_zoo_text(sampler, spp))
    assert s.errors == [] and s.desc.sampler.type == SAMPLER_TYPE[sampler] and s.spp == spp
    return s


def _gaussian_crop_furnace(pt):
    """The wide filter + crop window scene of test_edge_cases_empty_scene_no_lights_crop_filter, at 32 spp."""
    txt = st.furnace_area(res=40, spp=32).replace('Sampler', 'PixelFilter "gaussian" "float xwidth" [2] "float ywidth" [2]\nSampler')
    assert '[40] "integer yresolution" [40]' in txt
    return pt.Scene(text=txt.replace('[40] "integer yresolution" [40]', '[40] "integer yresolution" [40] "float cropwindow" [.2 .8 .1 .9]'))


def _mitchell_zoo(pt):
    txt = st.material_zoo(res=48, spp=8, depth=6)
    for a, b in _ZOO_VARIANTS["mitchell"]:
        assert a in txt
        txt = txt.replace(a, b, 1)
    return pt.Scene(text=txt)


RANDOM_SEEDS = (1, 4, 8, 9, 12, 16, 18, 22)

# name -> (builder(pt, assets), filter weights bit-equal?) -- weights as the scene's own test in test_gpu_parity.py compares them
SCENES = {
    "zoo halton": (lambda pt, d: _zoo(pt, "halton"), True),
    "zoo sobol": (lambda pt, d: _zoo(pt, "sobol"), True),
    "zoo random": (lambda pt, d: _zoo(pt, "random"), True),
    "zoo 02sequence": (lambda pt, d: _zoo(pt, "02sequence"), True),
    "zoo stratified": (lambda pt, d: _zoo(pt, "stratified"), True),
    "textured zoo lens": (lambda pt, d: pt.Scene(text=st.textured_zoo(res=64, spp=16, lens=True), base_dir=d), True),
    "spectralpath 3 bands": (lambda pt, d: _killeroo_spectralpath(pt, 3, spp=8, xres=96, yres=96), True),
    "spectralpath 4 bands": (lambda pt, d: _killeroo_spectralpath(pt, 4, spp=8, xres=96, yres=96), True),
    "infinite light map spatial": (lambda pt, d: pt.Scene(text=st.zoo_with_infinite_light("map", strategy="spatial"), base_dir=d), True),
    "instances lens": (lambda pt, d: pt.Scene(text=st.instanced_scene(lens=True), base_dir=d), True),
    "sphere row": (lambda pt, d: pt.Scene(text=st.sphere_row_scene()), True),
    "mis span": (lambda pt, d: pt.Scene(text=st.mis_span_scene()), True),
    "alpha masks": (lambda pt, d: pt.Scene(text=st.alpha_scene(), base_dir=d), True),
    "disney textured": (lambda pt, d: pt.Scene(text=st.disney_textured_scene(), base_dir=d), True),
    "gaussian crop furnace": (lambda pt, d: _gaussian_crop_furnace(pt), False),
    "zoo mitchell": (lambda pt, d: _mitchell_zoo(pt), False),
}
for _seed in RANDOM_SEEDS:
    SCENES["random scene %d" % _seed] = ((lambda seed: lambda pt, d: pt.Scene(text=st.random_scene(seed), base_dir=d))(_seed), False)

A_SCENES = list(SCENES)
# (for the two-pass test only: its passes are [0,3) + [3,16) and [0,8) + [8,16) under every sampler)
SCENES["spectralpath 3 bands 16 spp"] = (lambda pt, d: _killeroo_spectralpath(pt, 3, spp=16, xres=96, yres=96), True)

# (scene, pool) pairs that may fall short of "every slot reused eight times on average": the 2304-slot pool on the one-band
# random scenes (32 x 32 x 8 = 8 192 camera samples). Every other pair must qualify.
MAY_SKIP = {("random scene %d" % seed, 2304) for seed in (1, 4, 18, 22)}

_CACHE = {}


def _oracle(pt, ob, assets, name):
    """Scene, the oracle's exact-libm render of it and the default-pool device render's iteration count: once per scene."""
    if name not in _CACHE:
        s = SCENES[name][0](pt, assets)
        assert s.errors == [], (name, s.errors)
        with ob.exact_libm():
            ofilm, oweight, oc, _ = ob.render(s)
        film, weight, integ, _, _, _ = _parity(pt, ob, s, name + " | pool default", weights_exact=SCENES[name][1], oracle=(ofilm, oweight, oc))
        _CACHE[name] = (s, (ofilm, oweight, oc), int(integ.counters.iterations), integ.pool_info()[0], film)
    return _CACHE[name]


def test_the_random_scenes_cover_the_features_they_were_picked_for(pt, assets):
    """The eight seeds were picked for what their scenes hold; a change of the generator must not quietly empty the selection."""
    bands, samplers, instances, infinite, textured_lens = set(), set(), 0, 0, 0
    for seed in RANDOM_SEEDS:
        s = pt.Scene(text=st.random_scene(seed), base_dir=assets)
        assert s.errors == [], (seed, s.errors)
        d = s.desc
        bands.add(int(d.integrator.n_ca_bands))
        samplers.add(int(d.sampler.type))
        instances += d.n_instances > 0
        infinite += any(d.lights[i].type == 3 for i in range(d.n_lights))   # MI_LIGHT_INFINITE
        textured_lens += d.camera.lens_radius > 0 and d.n_textures > 0
    assert {2, 3, 4} <= bands, bands
    assert samplers == {0, 1, 2, 3, 4}, samplers
    assert instances >= 2 and infinite >= 2 and textured_lens >= 2, (instances, infinite, textured_lens)


# ---------------------------------------------------------------------------------------------- A: pool sizes
@pytest.mark.parametrize("pool", ["default", 256, 768, 2304, "third"])
@pytest.mark.parametrize("name", A_SCENES)
def test_pool_size_does_not_change_the_render(pt, ob, assets, name, pool):
    """One oracle render per scene; device renders on pools of one block (256 slots), three blocks, nine blocks (neither a
    multiple of k_generate's SLOT_CHUNKS x 256 slots per block), a third of the work and the default -- each at _parity's
    bars. Not vacuous: the pool is the size asked for, a small pool's slots each host eight paths or more on average, and the
    render took more iterations than the default pool's."""
    s, oracle, default_iterations, default_pool, default_film = _oracle(pt, ob, assets, name)
    if pool == "default":
        assert default_iterations > 0 and default_pool >= 256
        return   # (rendered and compared when the scene was first asked for, whichever case came first)
    cam = int(oracle[2].camera_rays)
    if pool == "third":
        # a third of the camera samples: one slot serves all bands of a sample, so with spectralpath the camera rays count
        # each sample n_bands times (a third of the 3-band scene's camera RAYS would be the default pool again)
        slots = max(256, int(round(cam / max(1, int(s.desc.integrator.n_ca_bands)) / 3 / 256)) * 256)
    else:
        slots = pool
        if cam < 8 * slots:
            assert (name, pool) in MAY_SKIP, (name, pool, cam)
            pytest.skip("%s: %d camera rays on %d slots is less than eight paths per slot" % (name, cam, slots))
    film, weight, integ, _, _, _ = _parity(pt, ob, s, "%s | pool %d" % (name, slots), weights_exact=SCENES[name][1],
                                           render=dict(path_pool=slots), oracle=oracle)
    assert integ.pool_info()[0] == slots
    assert integ.counters.iterations > default_iterations, (int(integ.counters.iterations), default_iterations)
    if name == "spectralpath 3 bands":   # round(31 / 3) = 10: bin 30 belongs to no band and stays zero in recycled slots as well
        assert not film[..., 30].any() and film[..., 29].any()
    assert _rel_l2(film, default_film) < 1e-6   # (follows from the two parities; says which side moved when one fails)


# ---------------------------------------------------------------------------------------------- B: shards and sub-renderers
@pytest.mark.parametrize("pool", [768, 0])
@pytest.mark.parametrize("streams", [1, 3])
@pytest.mark.parametrize("name", ["zoo 02sequence", "spectralpath 3 bands"])
def test_small_pools_with_shards_and_sub_renderers(pt, ob, assets, monkeypatch, name, streams, pool):
    """Three tile shards on one and on three sub-renderers (with three, path_pool = 768 is one 256-slot block each): films,
    weights and counters summed over the shards against the oracle's full frame, 2 counts of slack per render."""
    s, oracle, _, _, _ = _oracle(pt, ob, assets, name)
    ofilm, oweight, oc = oracle
    monkeypatch.setenv("MIPT_STREAMS", str(streams))   # (read when the renderer is created)
    integ = pt.CreatePathIntegrator(s)
    acc, accw, c = np.zeros_like(ofilm), np.zeros_like(oweight), dict.fromkeys(("camera_rays", "bad_samples") + COUNTER_KEYS, 0)
    for r in range(3):
        f, w = integ.Render(shard_index=r, shard_count=3, path_pool=pool)
        if pool:
            assert integ.pool_info()[0] == pool
        acc += f
        accw += w
        for k in c:
            c[k] += integ.counters.as_dict()[k]
    _compare("%s | streams %d, 3 shards, pool %s" % (name, streams, pool or "default"), acc, accw, c, ofilm, oweight, oc.as_dict(), s.spp,
             weights_exact=SCENES[name][1], counter_slack=2 * 3)


# ---------------------------------------------------------------------------------------------- C: passes over sample ranges
@pytest.mark.parametrize("first", [3, 8])
@pytest.mark.parametrize("name", ["zoo halton", "zoo sobol", "zoo random", "zoo 02sequence", "zoo stratified", "spectralpath 3 bands 16 spp"])
def test_two_passes_accumulate_to_the_oracles_frame(pt, ob, assets, name, first):
    """Sample numbers [0, first) on the default pool, then [first, spp) accumulated on a 768-slot pool, against the oracle's
    one-pass film (3- and 13-sample passes: work runs of one sample). Counters summed over the passes."""
    s, oracle, _, _, _ = _oracle(pt, ob, assets, name)
    ofilm, oweight, oc = oracle
    spp = s.spp
    assert spp == 16
    integ = pt.CreatePathIntegrator(s)
    integ.Render(spp=first, sample_begin=0, download=False)
    c = integ.counters.as_dict()
    film, weight = integ.Render(spp=spp - first, sample_begin=first, accumulate=True, path_pool=768)
    assert integ.pool_info()[0] == 768
    c = {k: c[k] + v for k, v in integ.counters.as_dict().items()}
    _compare("%s | passes [0,%d) + [%d,%d), pool default + 768" % (name, first, first, spp), film, weight, c, ofilm, oweight, oc.as_dict(),
             spp, weights_exact=SCENES[name][1], counter_slack=2 * 2)


# ---------------------------------------------------------------------------------------------- D: work runs
@pytest.mark.parametrize("spp", [1, 3, 12, 16])
@pytest.mark.parametrize("sampler", ["halton", "stratified"])
def test_work_run_length_does_not_change_the_render(pt, ob, monkeypatch, sampler, spp):
    """MIPT_WORK_RUN caps the run of consecutive samples of a pixel that is handed out together (the largest power of two up
    to the cap that divides spp): caps 1, 4 and 1024, and for 3 and 12 spp the default cap as well (runs of 1 and 4 by the
    divisibility rule), on the default pool and on 768 slots."""
    s = _zoo(pt, sampler, spp)
    with ob.exact_libm():
        ofilm, oweight, oc, _ = ob.render(s)
    monkeypatch.delenv("MIPT_WORK_RUN", raising=False)
    for cap in ([None] if spp in (3, 12) else []) + [1, 4, 1024]:
        if cap is not None:
            monkeypatch.setenv("MIPT_WORK_RUN", str(cap))   # (read at every render)
        for pool in (0, 768):
            film, weight, integ, _, _, _ = _parity(pt, ob, s, "zoo %s %d spp | run cap %s, pool %s" % (sampler, spp, cap or "default", pool or "default"),
                                                   render=dict(path_pool=pool), oracle=(ofilm, oweight, oc))
            if pool:
                assert integ.pool_info()[0] == pool


# ---------------------------------------------------------------------------------------------- E: large sample numbers
def _per_sample_reference(ob, s, x0, x1, y0, y1, begin, n):
    """The film sums of sample numbers [begin, begin + n) of the pixels [x0, x1) x [y0, y1), one oracle Li per sample."""
    ys, xs = np.mgrid[y0:y1, x0:x1]
    samples = np.concatenate([np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, begin + k, np.int64)], axis=1) for k in range(n)])
    assert samples.max() < 2 ** 31
    with ob.exact_libm():
        li, oc = ob.li(s, samples)
    ref = np.zeros((y1 - y0, x1 - x0, li.shape[1]), np.float32)
    np.add.at(ref, (samples[:, 1] - y0, samples[:, 0] - x0), li)
    return ref, oc


def _box_filter_weights(ob, s, x0, x1, y0, y1, begin, n):
    """The filter-weight sums the pass must leave on the whole film, from the oracle's own film positions of its samples
    (dimensions 0 and 1) through FilmTile::AddSample's footprint (film.h:131-141) with the box filter of radius 0.5: one pixel per
    sample, two (or four) for a sample that sits exactly on a pixel border -- px + u rounds up to the border where u is the
    largest float below 1. Global samplers only (the random sampler's values are no function of a dimension number)."""
    assert s.desc.sampler.type in (0, 1)
    w, h = s.film_size
    half = np.float32(.5)
    out = np.zeros((h, w), np.float32)
    sample = ob.lib().oracle_sample_dimension
    for k in range(n):
        for y in range(y0, y1):
            for x in range(x0, x1):
                fx = np.float32(np.float32(x) + np.float32(sample(s.desc_ptr, x, y, begin + k, 0))) - half
                fy = np.float32(np.float32(y) + np.float32(sample(s.desc_ptr, x, y, begin + k, 1))) - half
                out[max(int(np.ceil(fy - half)), 0):min(int(np.floor(fy + half)) + 1, h), max(int(np.ceil(fx - half)), 0):min(int(np.floor(fx + half)) + 1, w)] += 1
    return out


def _check_pass(name, film, weight, c, ref, oc, n, n_pixels, expected_weight=None):
    """A box-filtered pass of n samples per pixel against per-sample oracle sums, on the pixels that hold exactly their own n
    samples (a sample exactly on a pixel border also reaches the neighbour). The weights add up to n per pixel -- plus one for
    every further pixel a border sample reaches, where the oracle's sample positions (expected_weight) hold such samples: the
    Halton pass [T - 1, T + 1) at 64 x 64 has 100 of them (weight sum 8 292 on both sides), the other passes here have none."""
    inner = weight == n
    assert inner.mean() > 0.9, inner.mean()
    extra = 0.0
    if expected_weight is not None:
        assert np.array_equal(weight, expected_weight)
        extra = float(expected_weight.astype(np.float64).sum()) - n * n_pixels
        assert extra >= 0
    assert abs(float(weight.astype(np.float64).sum()) - n * n_pixels - extra) < 1e-3
    o = oc.as_dict()
    rel = _rel_l2(film[inner], ref[inner])
    METRICS.append({"test": name, "mode": "exact", "rel_l2": rel, "pixels": int(inner.sum()),
                    "counter_diff": {k: int(c[k] - o[k]) for k in COUNTER_KEYS}, "counters": {k: int(o[k]) for k in COUNTER_KEYS},
                    "camera_rays": int(o["camera_rays"])})
    assert not np.isnan(film).any()
    _check_counters(c, o, tol=0, slack=2)
    assert rel < 1e-6, (name, rel)


@pytest.mark.parametrize("sampler,begin", [("halton", "T-3"), ("halton", "T-1"), ("halton", 10 ** 6), ("halton", 2 ** 31 - 3),
                                           ("sobol", 10 ** 6), ("sobol", 2 ** 31 - 3), ("random", 10 ** 6), ("random", 2 ** 31 - 3)])
def test_sample_numbers_beyond_the_32_bit_halton_index(pt, ob, sampler, begin):
    """mi_pt_render keeps the Halton index in 32 bits while (last sample + 1) x stride < 2^32. Two-sample passes that begin at
    T - 3 (the last one that stays 32-bit), T - 1 (straddles the limit: the whole pass is 64-bit), 10^6 and 2^31 - 3 (the largest
    sample numbers there are), T = 2^32 / stride; Sobol' and random at the last two (their per-slot sample number is an int)."""
    s = _zoo(pt, sampler)
    if sampler == "halton":
        assert s.desc.sampler.sample_stride == 5184   # 2^6 x 3^4 at 64 x 64
    T = 2 ** 32 // 5184
    B = {"T-3": T - 3, "T-1": T - 1}.get(begin, begin)
    if begin == "T-3":
        assert (B + 2 + 1) * 5184 < 2 ** 32 <= (B + 2 + 2) * 5184
    integ = pt.CreatePathIntegrator(s)
    film, weight = integ.Render(spp=2, sample_begin=B)
    ref, oc = _per_sample_reference(ob, s, 0, 64, 0, 64, B, 2)
    expected = _box_filter_weights(ob, s, 0, 64, 0, 64, B, 2) if sampler != "random" else None
    if begin != "T-1" and expected is not None:
        assert float(expected.sum()) == 2 * 64 * 64   # (no border samples in these passes: the weights add up to the pass's spp per pixel)
    _check_pass("zoo %s | samples [%d, %d)" % (sampler, B, B + 2), film, weight, integ.counters.as_dict(), ref, oc, 2, 64 * 64, expected)


def test_large_sample_numbers_on_a_window_of_the_killeroo_frame(pt, ob):
    """700 x 700: stride 2^7 x 3^5 = 31 104 (a second base-3 exponent, and 64-bit indices from sample number 138 084 on); sample
    numbers from 10^6 on a 32 x 32 window (pixelbounds), against per-sample oracle sums."""
    text = open(KILLEROO).read()
    assert 'Integrator "path"' in text
    text = text.replace('Integrator "path"', 'Integrator "path" "integer pixelbounds" [320 352 300 332]')
    s = pt.Scene(text=text, base_dir=os.path.dirname(KILLEROO), spp=16)
    assert s.errors == [] and s.film_size == (700, 700)
    stride = int(s.desc.sampler.sample_stride)
    assert stride == 31104 and (10 ** 6 + 3) * stride >= 2 ** 32   # (a 64-bit pass)
    integ = pt.CreatePathIntegrator(s)
    film, weight = integ.Render(spp=2, sample_begin=10 ** 6)
    expected = _box_filter_weights(ob, s, 320, 352, 300, 332, 10 ** 6, 2)
    assert np.array_equal(weight, expected) and float(expected.sum()) == 2 * 32 * 32   # (the whole frame: nothing outside the window)
    assert not weight[:300].any() and not weight[332:].any() and not weight[:, :320].any() and not weight[:, 352:].any()
    ref, oc = _per_sample_reference(ob, s, 320, 352, 300, 332, 10 ** 6, 2)
    _check_pass("killeroo 700x700 window | samples [1000000, 1000002)", film[300:332, 320:352], weight[300:332, 320:352],
                integ.counters.as_dict(), ref, oc, 2, 32 * 32)


def test_sample_numbers_that_do_not_fit_an_int_are_refused(pt):
    """include/mi_pt.h: sample_begin >= 0 and sample_begin + spp <= 2^31 - 1."""
    s = _zoo(pt, "halton")
    integ = pt.CreatePathIntegrator(s)
    for kw in (dict(spp=2, sample_begin=2 ** 31 - 2), dict(spp=1, sample_begin=2 ** 31 - 1), dict(spp=2, sample_begin=2 ** 32),
               dict(spp=2, sample_begin=-1), dict(spp=2 ** 31, sample_begin=0)):
        with pytest.raises(RuntimeError, match="sample numbers out of range"):
            integ.Render(**kw)
    film, weight = integ.Render(spp=1, sample_begin=2 ** 31 - 2)   # the last sample number there is
    assert np.isfinite(film).all() and abs(float(weight.sum()) - 64 * 64) < 1e-3
