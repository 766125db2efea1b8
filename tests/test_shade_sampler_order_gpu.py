"""The order in which k_shade draws its sampler dimensions, through whole renders: the grouped Halton calls (five dimensions
for the direct-lighting estimate, two for the next direction, one for the roulette draw) must leave every path where the
reference's Get1D / Get2D sequence leaves it. Exact-mode parity (tests/test_gpu_parity.py: image relative L2 < 1e-6, every pixel
within 2e-4 x mean radiance, filter weights equal) with the ray and path counters equal as integers, on three 32 x 32 windows of
4 samples per pixel:

 1. a floor that is half matte and half plastic under two sphere lights, inside a matte room, at maxdepth 7: paths pass bounce
    3, so the roulette dimension is drawn between the grouped calls;
 2. the same room where the light distribution gives selPdf == 0 for the chosen light: the "power" strategy over lights that
    are all black (a Distribution1D picks a black light only where every light is black) -- UniformSampleOneLight returns
    after the light choice, the dimension counter advances by one instead of five, and every later direction shows it;
 3. scene 1 from sample number 140 000 on: the film is 700 x 700 (Halton stride 2^7 x 3^5 = 31 104), so every index is beyond
    2^32 and the single-dimension routine with its 64-bit loop is taken.

The window is a crop of the 700 x 700 film ("pixelbounds") under a box filter of radius 0.5, so a sample lands in its own pixel
(and in the neighbour where it sits exactly on the border) and the reference is the sum of the oracle's Li per sample
(correctly rounded libm: the arithmetic of the device), which also serves a pass that begins at a later sample number.

The oracle alone passes at this bar on the CPU: its per-sample sums (this file's reference) against its own render of the
window (ob.render, which accumulates tile by tile) have equal counters and filter weights, relative L2 9.8e-9 and the worst
pixel at 1.1e-7 x mean in scene 1, and are equal (a black film) in scene 2. Scene 3 is scene 1 at other sample numbers, which
the oracle's render does not take: there the per-sample sums stand alone (counters of the pass: 43 065 rays, 21 328 shadow rays).
"""
import numpy as np
import pytest

from test_gpu_parity import _rel_l2, _pixel_l2, COUNTER_KEYS, METRICS

pytestmark = pytest.mark.gpu

X0, X1, Y0, Y1 = 334, 366, 380, 412
SPP = 4
WIDE_BEGIN = 140000

SCENE = """
LookAt 0 3.2 -6.5  0 0.4 0  0 1 0
Camera "perspective" "float fov" [38]
Film "image" "integer xresolution" [700] "integer yresolution" [700]
PixelFilter "box" "float xwidth" [0.5] "float ywidth" [0.5]
Sampler "halton" "integer pixelsamples" [%(spp)d]
Integrator "path" "integer maxdepth" [7] "integer pixelbounds" [%(x0)d %(x1)d %(y0)d %(y1)d] "string lightsamplestrategy" "%(strategy)s"
WorldBegin
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [%(l0)s]
  Translate -1.5 3 0.5
  Shape "sphere" "float radius" [.4]
AttributeEnd
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [%(l1)s]
  Translate 1.8 2.4 -0.8
  Shape "sphere" "float radius" [.3]
AttributeEnd
AttributeBegin
  Material "matte" "rgb Kd" [.7 .65 .6]
  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-5 0 -8  -5 0 5  0 0 5  0 0 -8]
AttributeEnd
AttributeBegin
  Material "plastic" "rgb Kd" [.2 .3 .7] "rgb Ks" [.5 .5 .5] "float roughness" [.1]
  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [0 0 -8  0 0 5  5 0 5  5 0 -8]
AttributeEnd
AttributeBegin
  Material "matte" "rgb Kd" [.75 .75 .75]
  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-5 0 5  -5 6 5  5 6 5  5 0 5]
  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-5 0 -8  -5 6 -8  -5 6 5  -5 0 5]
  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [5 0 5  5 6 5  5 6 -8  5 0 -8]
  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-5 6 5  -5 6 -8  5 6 -8  5 6 5]
  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [5 0 -8  5 6 -8  -5 6 -8  -5 0 -8]
AttributeEnd
WorldEnd
"""


def scene(pt, strategy="spatial", lit=True):
    text = SCENE % dict(spp=SPP, x0=X0, x1=X1, y0=Y0, y1=Y1, strategy=strategy,
                        l0="30 28 24" if lit else "0 0 0", l1="14 18 26" if lit else "0 0 0")
    s = pt.Scene(text=text)
    assert s.errors == [] and s.film_size == (700, 700)
    assert int(s.desc.sampler.sample_stride) == 31104 and s.desc.n_lights == 2
    return s


def reference(ob, s, begin):
    """(film sums [700, 700, NSPEC], filter-weight sums [700, 700], counters) of sample numbers [begin, begin + SPP) of the window:
    one oracle Li per sample, added as FilmTile::AddSample adds it (film.h:131-141) under the box filter of radius 0.5 -- to the
    sample's own pixel, and to the neighbour too where the film position sits exactly on a pixel border (px + u rounds up to the
    border where u is the largest float below 1: some twenty of the 4096 samples of a pass)."""
    ys, xs = np.mgrid[Y0:Y1, X0:X1]
    samples = np.concatenate([np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, begin + k, np.int64)], axis=1) for k in range(SPP)])
    with ob.exact_libm():
        li, oc = ob.li(s, samples)
    w, h = s.film_size
    ref, weight = np.zeros((h, w, li.shape[1]), np.float32), np.zeros((h, w), np.float32)
    dimension, half = ob.lib().oracle_sample_dimension, np.float32(.5)
    for (x, y, k), value in zip(samples.tolist(), li):
        fx = np.float32(np.float32(x) + np.float32(dimension(s.desc_ptr, x, y, k, 0))) - half
        fy = np.float32(np.float32(y) + np.float32(dimension(s.desc_ptr, x, y, k, 1))) - half
        rows = slice(max(int(np.ceil(fy - half)), 0), min(int(np.floor(fy + half)) + 1, h))
        cols = slice(max(int(np.ceil(fx - half)), 0), min(int(np.floor(fx + half)) + 1, w))
        ref[rows, cols] += value
        weight[rows, cols] += 1
    return ref, weight, oc


def check(name, film, weight, c, ref, oweight, oc):
    """test_gpu_parity._compare's exact-mode bar on the film, with the counters equal as integers."""
    o = oc.as_dict()
    l2 = _pixel_l2(film, ref, SPP)
    mean = max(float(ref[Y0:Y1, X0:X1].mean()) / SPP, 1e-12)
    m = {"test": name, "mode": "exact", "rel_l2": _rel_l2(film, ref), "pixels": int((oweight > 0).sum()),
         "max_pixel_l2_over_mean": float(l2.max() / mean), "counter_diff": {k: int(c[k] - o[k]) for k in COUNTER_KEYS},
         "counters": {k: int(o[k]) for k in COUNTER_KEYS}, "camera_rays": int(o["camera_rays"])}
    METRICS.append(m)
    print(m)
    assert not np.isnan(film).any()
    assert np.array_equal(weight, oweight) and (oweight[Y0:Y1, X0:X1] >= SPP).all()
    assert c["camera_rays"] == o["camera_rays"] == SPP * (X1 - X0) * (Y1 - Y0)
    for k in COUNTER_KEYS:
        assert c[k] == o[k], (k, c[k], o[k])
    assert c["bad_samples"] == o["bad_samples"] == 0
    assert m["rel_l2"] < 1e-6, m
    assert m["max_pixel_l2_over_mean"] < 2e-4, m
    return m


def test_roulette_between_grouped_calls(pt, ob):
    s = scene(pt)
    ref, oweight, oc = reference(ob, s, 0)
    o = oc.as_dict()
    # paths pass bounce 3 (the roulette test of path.cpp:176 is reached): the mean length at the break is beyond 4
    assert o["path_length_sum"] > 4 * o["camera_rays"] and ref.mean() > 0
    assert (SPP + 1) * 31104 < 2 ** 32   # (32-bit indices: the grouped routines)
    integ = pt.CreatePathIntegrator(s)
    film, weight = integ.Render()
    check("sampler order | matte + plastic floor, maxdepth 7", film, weight, integ.counters.as_dict(), ref, oweight, oc)


def test_black_light_choice_advances_one_dimension(pt, ob):
    s = scene(pt, strategy="power", lit=False)
    ref, oweight, oc = reference(ob, s, 0)
    o = oc.as_dict()
    assert not ref.any() and o["shadow_rays"] == 0   # no estimate is made anywhere: selPdf == 0 at every vertex
    assert o["path_length_sum"] > 4 * o["camera_rays"]
    integ = pt.CreatePathIntegrator(s)
    film, weight = integ.Render()
    check("sampler order | power strategy over black lights", film, weight, integ.counters.as_dict(), ref, oweight, oc)


def test_indices_beyond_32_bits_take_the_single_dimension_routine(pt, ob):
    s = scene(pt)
    assert WIDE_BEGIN * 31104 >= 2 ** 32   # every index of the pass
    ref, oweight, oc = reference(ob, s, WIDE_BEGIN)
    assert oc.as_dict()["path_length_sum"] > 4 * oc.as_dict()["camera_rays"] and ref.mean() > 0
    integ = pt.CreatePathIntegrator(s)
    film, weight = integ.Render(spp=SPP, sample_begin=WIDE_BEGIN)
    check("sampler order | samples [140000, 140004)", film, weight, integ.counters.as_dict(), ref, oweight, oc)
