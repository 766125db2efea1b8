"""Integrator "metadata" on the GPU: the four maps against values worked out from the CPU oracle's entry points
(metadata_scenes.Expected), the pass under other pool sizes, shards and sample ranges, the maps and the radiance from one
renderer, and the command line.

The guards. SamplerIntegrator::Render blackens a sample whose y() is below -1e-5 (integrator.cpp:302-308), and the
`coordinates` map of this scene has samples whose CIE-Y-weighted sum is clearly negative (the quad near x = -40, z = -50:
about -0.02). But SampledSpectrum::y() of this fork clamps that sum at 0 before it scales it (spectrum.h:418), so the
reference's guard does not fire for them, neither does the oracle's (o_bsdf.h) nor the device's (YScale): such a sample keeps
its negative coordinates, and that is what these tests expect -- `coordinates` is zero where the guard fires and bad_samples
is the number of samples for which it does, with y() as the reference computes it: none here. So `exp.guarded` is empty and
every expected bad_samples is 0: no metadata test sees a blackened sample or a non-zero bad_samples (no strategy can form a
NaN, an infinite or, through the clamp, a negative y()); the guards themselves are k_generate's, exercised by the radiance
tests."""
import os
import subprocess

import numpy as np
import pytest

import metadata_scenes as ms

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pbrt-v3-spectral_amd")
_cache = {}


def _setup(pt, ob, spp=1, lens=0.0, light="infinite"):
    """(scene, expected values, renderer) of one variant of the scene, made once. The conditions on the scene are checked
    here, on the CPU, before anything is rendered."""
    key = (spp, lens, light)
    if key not in _cache:
        scene = pt.Scene(text=ms.render_scene(spp=spp, lens=lens, light=light))
        assert scene.errors == [] and scene.film_size == (32, 24) and scene.desc.n_instances == 2
        exp = ms.Expected(pt, ob, scene, spp)
        assert exp.n_samples == 32 * 24 * spp
        assert 0 < exp.n_hits < exp.n_samples                        # part of the frame sees nothing
        assert min(exp.instance_hits) >= 3 and exp.sphere_hits >= 3  # both instances and the world's sphere are seen
        lum = np.array(exp.luminance)
        # every coordinates sample at least 10x away from -1e-5, on one side or the other, and some on each side
        assert np.all((lum >= -1e-6) | (lum <= -1e-4)) and (lum >= -1e-6).any() and (lum <= -1e-4).any()
        _cache[key] = (scene, exp, pt.MetadataIntegrator(scene))
    return _cache[key]


def _rel_l2(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


def _check_counters(c, n_samples, bad):
    assert c["camera_rays"] == n_samples and c["regular_rays"] == n_samples
    assert c["shadow_rays"] == 0 and c["total_paths"] == 0 and c["zero_radiance_paths"] == 0 and c["path_length_sum"] == 0
    assert c["bad_samples"] == bad


@pytest.mark.parametrize("strategy", ms.STRATEGIES)
def test_one_sample_per_pixel_is_bit_equal(pt, ob, strategy):
    scene, exp, integ = _setup(pt, ob)
    film, weight = integ.Render(strategy=strategy)
    assert np.array_equal(weight, exp.weight)
    want = exp.film[strategy]
    assert want.any()
    assert np.array_equal(film.view(np.uint32), want.view(np.uint32)), np.argwhere(film != want)[:8]
    _check_counters(integ.counters.as_dict(), exp.n_samples, exp.bad[strategy])
    if strategy == "coordinates":
        assert not film[exp.guarded].any() and (film[..., 0] < -30).any() and not film[..., 3:].any()
    img = pt.metadata_image(film, weight, strategy)
    assert img.shape == ((24, 32, 3) if strategy == "coordinates" else (24, 32))
    if strategy in ("material", "mesh"):   # ids: whole numbers where one sample fell (a pixel with two holds their mean)
        one = weight == 1
        assert np.array_equal(img[one], np.round(img[one])) and img[one].max() == (11 if strategy == "material" else 2)


def test_the_scene_files_strategy_is_the_default(pt, ob):
    scene, exp, _ = _setup(pt, ob)
    s2 = pt.Scene(text=ms.render_scene(strategy="mesh"))
    integ = pt.CreateIntegrator(s2)
    assert isinstance(integ, pt.MetadataIntegrator)
    film, weight = integ.Render()
    assert np.array_equal(film, exp.film["mesh"]) and np.array_equal(weight, exp.weight)


@pytest.mark.parametrize("strategy", ms.STRATEGIES)
def test_four_samples_per_pixel(pt, ob, strategy):
    scene, exp, integ = _setup(pt, ob, spp=4)
    film, weight = integ.Render(strategy=strategy)
    assert np.array_equal(weight, exp.weight)
    if strategy in ("material", "mesh"):   # sums of small integers are exact in any order
        assert np.array_equal(film, exp.film[strategy])
    else:                                  # the exact-mode film bar
        rel = _rel_l2(film, exp.film[strategy])
        print("4 spp %s: relative L2 %.3e" % (strategy, rel))
        assert rel < 1e-6
    _check_counters(integ.counters.as_dict(), exp.n_samples, exp.bad[strategy])


@pytest.mark.parametrize("strategy", ms.STRATEGIES)
def test_depth_is_measured_from_the_lens_point(pt, ob, strategy):
    """lensradius > 0: ray.o is the point on the lens. (A point light here: the resolve step ends the escaped rays itself.)"""
    scene, exp, integ = _setup(pt, ob, lens=0.3, light="point")
    _, exp0, _ = _setup(pt, ob)
    assert not np.array_equal(exp.film["depth"], exp0.film["depth"])
    film, weight = integ.Render(strategy=strategy)
    assert np.array_equal(weight, exp.weight)
    assert np.array_equal(film.view(np.uint32), exp.film[strategy].view(np.uint32))
    _check_counters(integ.counters.as_dict(), exp.n_samples, exp.bad[strategy])


def test_pool_size_shards_and_passes_give_the_same_maps(pt):
    """64 x 64 x 4 spp: a 256-slot pool (every slot is recycled 64 times), three shards added together and two accumulated
    passes over sample ranges, each against the frame of one pass on the default pool."""
    scene = pt.Scene(text=ms.render_scene(res=(64, 64), spp=4))
    integ = pt.MetadataIntegrator(scene)
    n = 64 * 64 * 4
    for strategy in ms.STRATEGIES:
        ref, wref = integ.Render(strategy=strategy)
        assert ref.any() and integ.counters.camera_rays == n

        def same(film, weight, what):
            assert np.array_equal(weight, wref), what
            if strategy in ("material", "mesh"):
                assert np.array_equal(film, ref), (strategy, what)
            else:
                rel = _rel_l2(film, ref)
                print("%s, %s: relative L2 %.3e" % (strategy, what, rel))
                assert rel < 1e-6, (strategy, what, rel)

        film, weight = integ.Render(strategy=strategy, path_pool=256)
        assert integ.pool_info()[0] == 256 and integ.counters.camera_rays == n
        same(film, weight, "256-slot pool")
        acc, wacc, cams = np.zeros_like(ref), np.zeros_like(wref), 0
        for r in range(3):
            f, w = integ.Render(strategy=strategy, shard_index=r, shard_count=3)
            acc += f
            wacc += w
            cams += integ.counters.camera_rays
        assert cams == n
        same(acc, wacc, "three shards")
        integ.Render(strategy=strategy, spp=2, sample_begin=0, download=False)
        film, weight = integ.Render(strategy=strategy, spp=2, sample_begin=2, accumulate=True)
        same(film, weight, "two passes")


def test_one_renderer_serves_the_radiance_and_the_four_maps(pt, ob):
    """Render(), the four RenderMetadata calls, Render() again on one PathIntegrator of a path scene: every map is the map of
    a fresh MetadataIntegrator, and the second radiance film is the first, bit for bit, with equal counters."""
    _, exp, fresh = _setup(pt, ob)
    scene = pt.Scene(text=ms.render_scene(integrator='Integrator "path" "integer maxdepth" [3]'))
    assert scene.desc.integrator.kind == 0
    integ = pt.PathIntegrator(scene)
    film0, weight0 = integ.Render()
    c0 = integ.counters.as_dict()
    assert film0.any() and c0["shadow_rays"] > 0
    for strategy in ms.STRATEGIES:
        f, w = integ.RenderMetadata(strategy)
        g, wg = fresh.Render(strategy=strategy)
        assert np.array_equal(f.view(np.uint32), g.view(np.uint32)) and np.array_equal(w, wg), strategy
        assert np.array_equal(f, exp.film[strategy])
    film1, weight1 = integ.Render()
    c1 = integ.counters.as_dict()
    assert np.array_equal(film1, film0) and np.array_equal(weight1, weight0)
    assert c1 == c0


def test_a_spectralpath_renderer_gives_maps_between_its_band_renders(pt, ob):
    """The pass traces one ray per camera sample whatever numCABands says (its pool has no stitched-spectrum planes), and the
    band renders before and after it agree bit for bit."""
    _, exp, _ = _setup(pt, ob)
    scene = pt.Scene(text=ms.render_scene(integrator='Integrator "spectralpath" "integer numCABands" [2] "integer maxdepth" [2]'))
    assert scene.errors == [] and scene.desc.integrator.n_ca_bands == 2
    integ = pt.PathIntegrator(scene)
    film0, weight0 = integ.Render()
    c0 = integ.counters.as_dict()
    assert c0["regular_rays"] > 2 * exp.n_samples - 1
    for strategy in ("depth", "mesh"):
        f, w = integ.RenderMetadata(strategy)
        assert np.array_equal(f.view(np.uint32), exp.film[strategy].view(np.uint32)) and np.array_equal(w, exp.weight)
        _check_counters(integ.counters.as_dict(), exp.n_samples, 0)
    film1, weight1 = integ.Render()
    assert np.array_equal(film1, film0) and np.array_equal(weight1, weight0) and integ.counters.as_dict() == c0


def test_command_line_writes_the_map_and_the_name_file(pt, ob, tmp_path):
    _, exp, _ = _setup(pt, ob)
    (tmp_path / "scene.pbrt").write_text(ms.render_scene(strategy="mesh", filename="labels.exr"))
    r = subprocess.run([os.path.join(PKG, "pbrt_amd"), "scene.pbrt"], cwd=str(tmp_path), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(tmp_path)) == ["labels.dat", "labels_mesh.txt", "scene.pbrt"]
    assert (tmp_path / "labels_mesh.txt").read_text() == "1 thing\n2 thing\n"
    film = pt.read_dat(str(tmp_path / "labels.dat"))
    assert np.array_equal(film, exp.film["mesh"])
    assert "Camera rays traced %d" % exp.n_samples in r.stdout
