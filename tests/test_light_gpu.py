"""The device lights, query by query: mi_pt_light_probe (SampleLi / LiBin, InfinitePdfLi / ShapePdf, InfiniteLe as k_shade
calls them) against light_restatement.py over the cases of light_cases.py, against the oracle's probe bit for bit under
exact_libm(), and against the independent statements of test_light_restatement.py on the device's own outputs. A query on
which the float32 and the float64 restatement decide differently is unsure and decides nothing; every family that does not
sit on a decision by construction asserts on the CPU that at most 1 % of its queries are. Bars: light_cases.check /
check_rel -- four times the worst float32-vs-float64 deviation of the restatement over the selected queries of ONE family,
never below 8 ulp (absolute) or 8 * 2^-23 (relative)."""
import numpy as np
import pytest

import light_cases as lc
import light_restatement as lr
import test_light_restatement as cpu

pytestmark = pytest.mark.gpu


def _against_the_oracle(label, ob, s, k, queries, device, exact_words, log):
    """Under exact_libm(): pdf == 0 and black in the same places; the count of output words that differ, which is zero where
    exact_words is set. (Words that differ have passed the bars of light_cases.hold.)"""
    with ob.exact_libm():
        oracle = lc.answer(lambda mode, q: ob.light_probe(s, k, mode, q), queries)
    words = differ = 0
    for mode, fam in queries:
        d, o = device[(mode, fam.name)], oracle[(mode, fam.name)]
        if mode == 0:
            assert np.array_equal(d[:, 3] == 0, o[:, 3] == 0), (label, fam.name, "pdf == 0")
            assert np.array_equal((d[:, 10:] == 0).all(axis=1), (o[:, 10:] == 0).all(axis=1)), (label, fam.name, "black")
        elif mode == 1:
            assert np.array_equal(d == 0, o == 0), (label, fam.name, "Pdf_Li == 0")
        bad = int((lc.bits(d) != lc.bits(o)).sum())
        if exact_words:
            assert bad == 0, (label, mode, fam.name, "%d of %d words differ from the oracle" % (bad, d.size))
        words += d.size
        differ += bad
    log.append("%s: %d of %d output words differ from the oracle under exact_libm" % (label, differ, words))


def _run(label, pt, ob, s, k, queries, exact_words):
    l32, l64 = lr.both(s.desc, k)
    integ = pt.CreatePathIntegrator(s)
    device = lc.answer(lambda mode, q: integ.light_probe(k, mode, q), queries)
    log = []
    try:
        cpu.hold_all(label, l32, l64, queries, device, log)
        _against_the_oracle(label, ob, s, k, queries, device, exact_words, log)
    finally:
        print("\n".join(log))


@pytest.mark.parametrize("name,xf", cpu.INFINITE)
def test_probe_infinite_light(pt, ob, tmp_path, name, xf):
    """Modes 0, 1 and 2 on every family of light_cases.infinite_queries. wi, pdf and Li pass through sin, cos, acos and atan2:
    the count of words that differ from the oracle is printed, and those words are inside the bars."""
    s, k = lc.infinite_scene(pt, tmp_path, name, xf)
    l32, l64 = lr.both(s.desc, k)
    queries = lc.infinite_queries(l32, l64, np.random.default_rng(31))
    _run("%s, %s" % (name, xf), pt, ob, s, k, queries, exact_words=False)


@pytest.mark.parametrize("case", cpu.delta_cases(), ids=lambda c: c[0])
def test_probe_delta_lights(pt, ob, case):
    name, body, kind, cones = case
    s, k = lc.delta_scene(pt, body, kind)
    l32 = lr.Light(s.desc, k) if kind == lr.SPOT else None
    _run(name, pt, ob, s, k, lc.delta_queries(np.random.default_rng(32), cones, l32), exact_words=True)


@pytest.mark.parametrize("name", list(lc.TRIANGLES))
def test_probe_triangle_emitters(pt, ob, name):
    s, k = lc.triangle_scene(pt, name)
    l64 = lr.Light(s.desc, k, np.float64)
    _run(name, pt, ob, s, k, lc.triangle_queries(l64, np.random.default_rng(33)), exact_words=True)


# ---------------------------------------------------------------------------------------------------------------------
# the independent statements on the device's own outputs
@pytest.mark.parametrize("name,xf", [(m, x) for m in lc.MAPS for x in lc.RIGID])
def test_device_pdf_li_integrates_to_one(pt, tmp_path, name, xf):
    s, k = lc.infinite_scene(pt, tmp_path, name, xf)
    integ = pt.CreatePathIntegrator(s)
    total = cpu.integral_of_pdf(lr.Light(s.desc, k, np.float64), lambda w: integ.light_probe(k, 1, lc.pack(lc.REF[None, :], w)))
    print("%s, %s: integral of Pdf_Li on the device: 1 %+.2e" % (name, xf, total - 1))
    assert abs(total - 1) <= 1e-5


@pytest.mark.parametrize("name", list(lc.MAPS))
def test_device_samples_follow_pdf_li(pt, tmp_path, name):
    s, k = lc.infinite_scene(pt, tmp_path, name, "rotated")
    integ = pt.CreatePathIntegrator(s)
    p, cells = cpu.chi_square_of_samples(lr.Light(s.desc, k, np.float64), lambda mode, q: integ.light_probe(k, mode, q))
    print("%s: chi-square p = %.3f over %d cells (device)" % (name, p, cells))
    assert p > 0.01 * 0.2


@pytest.mark.parametrize("name,xf", [(m, x) for m in lc.MAPS for x in lc.RIGID])
def test_device_pdf_and_le_at_a_sampled_direction(pt, tmp_path, name, xf):
    s, k = lc.infinite_scene(pt, tmp_path, name, xf)
    l32, l64 = lr.both(s.desc, k)
    integ = pt.CreatePathIntegrator(s)
    log = []
    try:
        cpu.sample_round_trip("%s, %s (device)" % (name, xf), l32, l64, lambda mode, q: integ.light_probe(k, mode, q), log)
    finally:
        print("\n".join(log))


@pytest.mark.parametrize("name", list(lc.SPOTS))
def test_device_spot_falloff_and_flux(pt, name):
    s, k = lc.delta_scene(pt, lc.spot_text(name), lr.SPOT)
    l32, l64 = lr.both(s.desc, k)
    integ = pt.CreatePathIntegrator(s)
    cpu.spot_falloff_check(name, l32, l64, lambda q: integ.light_probe(k, 0, q))
    cpu.spot_flux_check(name + " (device)", l64, lambda q: integ.light_probe(k, 0, q))


@pytest.mark.parametrize("name", list(lc.TRIANGLES))
def test_device_triangle_solid_angle(pt, name):
    s, k = lc.triangle_scene(pt, name)
    integ = pt.CreatePathIntegrator(s)
    cpu.solid_angle_check(name, lr.Light(s.desc, k, np.float64), lambda q: integ.light_probe(k, 0, q), "device")


# ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_the_renderer_still_renders(pt):
    """A light index of -1 or n_lights, mode 3, and mode 2 on a delta light return MI_ERR_INVALID with a message that names
    the entry point; the integrator renders the same film before and after."""
    body = lc.DELTA["point"] + 'AttributeBegin\nAreaLightSource "diffuse" "rgb L" [5 4 3]\n' + lc.TRIANGLES["one-sided, in a coordinate plane"][1] + "AttributeEnd\n" + lc.BALL
    s = pt.Scene(text=lc.text(body))
    assert s.errors == [] and s.desc.n_lights == 2
    point, area = lc.light_of(s, lr.POINT), lc.light_of(s, lr.AREA)
    integ = pt.CreatePathIntegrator(s)
    film, weight = integ.Render()
    assert film.any()
    q8, q6 = np.zeros((3, 8), np.float32), np.zeros((3, 6), np.float32)
    for light, mode, q, what in ((-1, 0, q8, "light index out of range"), (s.desc.n_lights, 0, q8, "light index out of range"),
                                 (area, 3, q6, "mode must be 0, 1 or 2"), (point, 2, q6, "delta light")):
        with pytest.raises(RuntimeError) as err:
            integ.light_probe(light, mode, q)
        assert "mi_pt_light_probe" in str(err.value) and what in str(err.value), str(err.value)
    assert integ.light_probe(area, 2, np.array([[0, 0, 1, 0, 0, 1]], np.float32)).any()
    assert integ.light_probe(point, 1, np.zeros((2, 9), np.float32)).tolist() == [0, 0]
    again, weight2 = integ.Render()
    assert np.array_equal(film, again) and np.array_equal(weight, weight2)
