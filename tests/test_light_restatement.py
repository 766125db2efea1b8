"""The lights without a GPU: light_restatement.py (numpy, float32 and float64, written from the reference's lights) and the
oracle's probe (oracle_light_probe) are held to independent statements -- the tables rebuilt from their func, closed forms,
the integral of Pdf_Li, a chi-square of the sampled directions, the spot light's flux, the solid angle of a triangle -- and to
each other, query by query, over the cases of light_cases.py. test_light_gpu.py asks the same of the device."""
import math

import numpy as np
import pytest

import light_cases as lc
import light_restatement as lr

INFINITE = [(m, x) for m in lc.MAPS for x in lc.TRANSFORMS]


def _ulp_apart(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def _show(log):
    print("\n".join(log))


# ---------------------------------------------------------------------------------------------------------------------
# the tables
@pytest.mark.parametrize("name", list(lc.MAPS))
def test_distribution_tables_rebuild_from_their_func(pt, tmp_path, name):
    """The float32 restatement of the Distribution1D constructor rebuilds every table of the map from cond_func, bit for bit;
    the marginal's func is the rows' funcInt; a row with funcInt == 0 carries the i / n cdf."""
    s, k = lc.infinite_scene(pt, tmp_path, name, "identity")
    e = lr.EnvMap(s.desc.envmaps[0])
    cdf, func_int = lr.distribution1d(e.cond_func)
    assert np.array_equal(lc.bits(cdf), lc.bits(e.cond_cdf)) and np.array_equal(lc.bits(func_int), lc.bits(e.cond_func_int))
    assert np.array_equal(lc.bits(e.marg_func), lc.bits(e.cond_func_int))
    mcdf, mint = lr.distribution1d(e.marg_func[None, :])
    assert np.array_equal(lc.bits(mcdf[0]), lc.bits(e.marg_cdf)) and lc.bits(mint)[0] == lc.bits(e.marg_func_int)
    ramp = np.arange(e.nu + 1, dtype=np.float32) / np.float32(e.nu)
    dark = np.nonzero(e.cond_func_int == 0)[0]
    for v in dark:
        assert np.array_equal(e.cond_cdf[v], ramp)
    if name.startswith(("black", "one texel")):
        assert len(dark) > 0 and (np.diff(e.marg_cdf) == 0).any(), "the map was to leave a row of the distribution black"
        lit = e.cond_cdf[e.cond_func_int > 0]
        assert (np.diff(lit, axis=1) == 0).any(), "and runs of equal cdf entries in a lit row"
    else:
        assert len(dark) == 0 and (e.cond_func > 0).all()


def test_constant_map_weights_rows_by_sin_theta(pt, tmp_path):
    """infinite.cpp:60-75 on a constant map: the image handed to Distribution2D is y(texel) * sin(pi (v + 1/2) / nv), the sine
    of a float32 argument as line 69 takes it. 4 ulp: one for the host's sinf, the rest for the bilinear weights of the lookup."""
    s, k = lc.infinite_scene(pt, tmp_path, "constant 4x2", "identity")
    e = lr.EnvMap(s.desc.envmaps[0])
    rgb = e.rgb[0, 0]
    assert (e.rgb == rgb).all()
    y = np.float32(0.212671) * rgb[0] + np.float32(0.715160) * rgb[1] + np.float32(0.072169) * rgb[2]   # RGBSpectrum::y, spectrum.h:535-538
    arg = np.float32(math.pi) * (np.arange(e.nv).astype(np.float32) + np.float32(0.5)) / np.float32(e.nv)
    want = y * np.sin(arg.astype(np.float64)).astype(np.float32)
    apart = _ulp_apart(e.cond_func, np.broadcast_to(want[:, None], e.cond_func.shape))
    print("constant map: cond_func within %.1f ulp of y sin(theta)" % apart.max())
    assert apart.max() <= 4


# ---------------------------------------------------------------------------------------------------------------------
# the infinite light against independent statements
def integral_of_pdf(l64, pdf_at):
    """sum over the distribution's cells of Pdf_Li(midpoint) sin(theta) dtheta dphi: the integrand is constant per cell, so
    this is the integral up to rounding."""
    w, weight = lc.cell_midpoints(l64)
    return float((pdf_at(w).astype(np.float64) * weight).sum())


@pytest.mark.parametrize("name,xf", [(m, x) for m in lc.MAPS for x in lc.RIGID])
def test_pdf_li_integrates_to_one(pt, ob, tmp_path, name, xf):
    s, k = lc.infinite_scene(pt, tmp_path, name, xf)
    l32, l64 = lr.both(s.desc, k)
    restated = integral_of_pdf(l64, lambda w: lr.infinite_pdf_li(l64, w)["pdf"])
    oracle = integral_of_pdf(l64, lambda w: ob.light_probe(s, k, 1, lc.pack(lc.REF[None, :], w)))
    print("%s, %s: integral of Pdf_Li: restatement 1 %+.2e, oracle 1 %+.2e" % (name, xf, restated - 1, oracle - 1))
    assert abs(restated - 1) <= 1e-5 and abs(oracle - 1) <= 1e-5


def chi_square_of_samples(l64, probe, n=60000, seed=5):
    """Histogram n mode-0 samples over the distribution's cells; expected counts from mode 1 at the cells' midpoints. The
    level of test_bsdf_sampling_matches_its_pdf: p > 0.01 * 0.2 over the cells that expect more than 5. Cells that expect
    nothing receive nothing."""
    from scipy import stats
    rng = np.random.default_rng(seed)
    u = rng.random((n, 2)).astype(np.float32)
    got = probe(0, lc.pack(lc.REF[None, :], u))
    ok = got[:, 3] > 0
    hist = np.bincount(lc.cell_of(l64, got[ok, 0:3]), minlength=l64.env.nu * l64.env.nv).astype(np.float64)
    w, weight = lc.cell_midpoints(l64)
    expected = probe(1, lc.pack(lc.REF[None, :], w)).astype(np.float64) * weight * n
    assert abs(expected.sum() / n - 1) < 1e-4 and ok.mean() > 0.999
    assert not hist[expected == 0].any(), "samples in cells of zero density"
    mask = expected > 5
    chi2 = ((hist[mask] - expected[mask]) ** 2 / expected[mask]).sum()
    p = float(stats.chi2.sf(chi2, int(mask.sum()) - 1))
    return p, int(mask.sum())


@pytest.mark.parametrize("name", list(lc.MAPS))
def test_sampled_directions_follow_pdf_li(pt, ob, tmp_path, name):
    s, k = lc.infinite_scene(pt, tmp_path, name, "rotated")
    l64 = lr.Light(s.desc, k, np.float64)
    p, cells = chi_square_of_samples(l64, lambda mode, q: ob.light_probe(s, k, mode, q))
    print("%s: chi-square p = %.3f over %d cells" % (name, p, cells))
    assert p > 0.01 * 0.2


def sample_round_trip(label, l32, l64, probe, log, n=2000, seed=6):
    """Mode 1 at a mode-0 sample's wi gives the sampled pdf, and mode 2 its Li. The value expected is the float64
    restatement's sampled pdf / Li; the bar comes from the float32 restatement of the same round trip (Sample_Li, then
    Pdf_Li / Le at the float32 wi), which carries the conditioning of acos near the poles."""
    rng = np.random.default_rng(seed)
    u = rng.random((n, 2)).astype(np.float32)
    ref = np.tile(lc.REF[:3], (n, 1))
    got0 = probe(0, lc.pack(lc.REF[None, :], u))
    s32, s64 = lr.sample_li(l32, ref, u), lr.sample_li(l64, ref, u)
    rt32, rt64 = lr.infinite_pdf_li(l32, s32["wi"]), lr.infinite_pdf_li(l64, s64["wi"])
    sure = (s32["offset"] == s64["offset"]) & (rt32["cell"] == s32["offset"]) & (rt64["cell"] == s64["offset"]) & ~s64["zero"] & ~s32["zero"]
    assert sure.mean() > 0.99, (label, sure.mean())
    got1 = probe(1, lc.pack(lc.REF[None, :], got0[:, 0:3]))
    got2 = probe(2, got0[:, 0:3])
    dev_cell = lr.infinite_pdf_li(l64, got0[:, 0:3].astype(np.float64))["cell"]
    sure &= dev_cell == s64["offset"]
    lc.check_rel(label, "Pdf_Li(wi of the sample) against the sampled pdf", got1, rt32["pdf"], s64["pdf"], sure, log)
    lc.check(label, "Le(wi of the sample) against the sampled Li", got2, lr.infinite_le(l32, s32["wi"]), s64["Li"], sure, log)


@pytest.mark.parametrize("name,xf", [(m, x) for m in lc.MAPS for x in lc.RIGID])
def test_pdf_and_le_at_a_sampled_direction(pt, ob, tmp_path, name, xf):
    s, k = lc.infinite_scene(pt, tmp_path, name, xf)
    l32, l64 = lr.both(s.desc, k)
    log = []
    try:
        sample_round_trip("%s, %s" % (name, xf), l32, l64, lambda mode, q: ob.light_probe(s, k, mode, q), log)
    finally:
        _show(log)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's probe against the restatement, every case
def hold_all(label, l32, l64, queries, answers, log):
    for mode, fam in queries:
        lc.hold(label, l32, l64, mode, fam, answers[(mode, fam.name)], log)


def bit_for_bit(label, l32, queries, answers, columns, log):
    """The words of `columns` (of mode 0; all of modes 1 and 2) equal the float32 restatement's."""
    words, differ = [0, 0, 0], [0, 0, 0]
    for mode, fam in queries:
        got = answers[(mode, fam.name)]
        q = fam.q
        if mode == 0:
            want, got = lr.out_of(lr.sample_li(l32, q[:, :3], q[:, 6:8]))[:, columns], got[:, columns]
        elif mode == 1:
            want = lr.pdf_li(l32, q[:, :3], q[:, 6:9])["pdf"]
        elif l32.type == lr.INFINITE:
            want = lr.infinite_le(l32, q)
        else:
            want = lr.area_l(l32, q[:, :3], q[:, 3:6])[0]
        bad = int((lc.bits(got) != lc.bits(want)).sum())
        assert bad == 0, "%s, mode %d, %s: %d of %d words differ from the float32 restatement" % (label, mode, fam.name, bad, got.size)
        words[mode] += got.size
    log.append("%s: bit for bit with the float32 restatement: %d / %d / %d words of modes 0 / 1 / 2" % ((label,) + tuple(words)))


@pytest.mark.parametrize("name,xf", INFINITE)
def test_oracle_infinite_light_against_the_restatement(pt, ob, tmp_path, name, xf):
    """Every family of light_cases.infinite_queries: the unsure cap, the verdicts and the bars of light_cases.hold with the
    host's libm; with correctly rounded libm calls every output word is the float32 restatement's -- which covers
    Distribution2D's (d0, d1, mapPdf): they do not pass through libm, and wi, pdf and Li are functions of them."""
    s, k = lc.infinite_scene(pt, tmp_path, name, xf)
    l32, l64 = lr.both(s.desc, k)
    queries = lc.infinite_queries(l32, l64, np.random.default_rng(31))
    assert sum(len(f.q) for _, f in queries) < 200000
    log = []
    try:
        hold_all("%s, %s" % (name, xf), l32, l64, queries, lc.answer(lambda mode, q: ob.light_probe(s, k, mode, q), queries), log)
        with ob.exact_libm():
            exact = lc.answer(lambda mode, q: ob.light_probe(s, k, mode, q), queries)
        bit_for_bit("%s, %s, exact libm" % (name, xf), l32, queries, exact, slice(None), log)
    finally:
        _show(log)


def delta_cases():
    out = [("spot, " + n, lc.spot_text(n), lr.SPOT, (c, c - d)) for n, (c, d) in lc.SPOTS.items()]
    return out + [("point", lc.DELTA["point"], lr.POINT, None), ("distant", lc.DELTA["distant"], lr.DISTANT, None)]


@pytest.mark.parametrize("case", delta_cases(), ids=lambda c: c[0])
def test_oracle_delta_lights_against_the_restatement(pt, ob, case):
    name, body, kind, cones = case
    s, k = lc.delta_scene(pt, body, kind)
    l32, l64 = lr.both(s.desc, k)
    queries = lc.delta_queries(np.random.default_rng(32), cones, l32 if kind == lr.SPOT else None)
    answers = lc.answer(lambda mode, q: ob.light_probe(s, k, mode, q), queries)
    log = []
    try:
        hold_all(name, l32, l64, queries, answers, log)
        bit_for_bit(name, l32, queries, answers, slice(None), log)
    finally:
        _show(log)
    with pytest.raises(ValueError):
        ob.light_probe(s, k, 2, np.zeros((1, 6), np.float32))


@pytest.mark.parametrize("name", list(lc.TRIANGLES))
def test_oracle_triangle_emitters_against_the_restatement(pt, ob, name):
    s, k = lc.triangle_scene(pt, name)
    l32, l64 = lr.both(s.desc, k)
    assert lc.bits(lr.tri_area(l32)) == lc.bits(l32.rec_area)
    queries = lc.triangle_queries(l64, np.random.default_rng(33))
    answers = lc.answer(lambda mode, q: ob.light_probe(s, k, mode, q), queries)
    log = []
    try:
        hold_all(name, l32, l64, queries, answers, log)
        bit_for_bit(name, l32, queries, answers, slice(3, 10), log)   # pdf, p, n: no libm, and wi = Normalize(p - ref) besides
    finally:
        _show(log)


# ---------------------------------------------------------------------------------------------------------------------
# the spot light
def spot_falloff_check(name, l32, l64, probe):
    """Outside the band the falloff is 0 or 1 bit for bit: Li is black, or the point light's I / d^2. Inside it is
    ((cos theta - ct) / (cs - ct))^4 and grows with cos theta. probe(q) -> mode-0 output."""
    cone, delta = lc.SPOTS[name]
    assert abs(float(l64.cos_total_width) - math.cos(math.radians(cone))) < 1e-6
    assert abs(float(l64.cos_falloff_start) - math.cos(math.radians(cone - delta))) < 1e-6
    rng = np.random.default_rng(34)
    a, b, axis = lc._frame(np.array(lc.SPOT_TO) - np.array(lc.SPOT_FROM))
    th = np.radians(np.linspace(0.01, min(2 * cone, 179), 4000))
    az = rng.uniform(0, 2 * math.pi, len(th))
    d = np.cos(th)[:, None] * axis + np.sin(th)[:, None] * (np.cos(az)[:, None] * a + np.sin(az)[:, None] * b)
    q = lc.pack(np.array(lc.SPOT_FROM) + 3 * d, np.zeros((len(d), 3)), np.zeros((len(d), 2)))
    got = probe(q)
    r32, r64 = lr.sample_li(l32, q[:, :3], None), lr.sample_li(l64, q[:, :3], None)
    sure = r32["branch"] == r64["branch"]
    assert sure.mean() >= 0.99
    point = lr.point_sample_li(l32, q[:, :3])["Li"]
    out, full, band = sure & (r64["branch"] == 0), sure & (r64["branch"] == 2), sure & (r64["branch"] == 1)
    assert out.any() and full.any() and band.any() == (delta > 0)
    assert not got[out, 10:].any() and np.array_equal(lc.bits(got[full, 10:]), lc.bits(point[full]))
    if delta > 0:
        d2 = ((l64.pos - q[:, :3].astype(np.float64)) ** 2).sum(axis=1)
        f_got = got[:, 10].astype(np.float64) * d2 / float(l64.L[0])
        c = r64["cos_theta"]
        closed = ((c - float(l64.cos_total_width)) / (float(l64.cos_falloff_start) - float(l64.cos_total_width))) ** 4
        log = []
        try:
            lc.check("spot " + name, "falloff in the band against the closed form", f_got, r32["falloff"], closed, band, log)
        finally:
            _show(log)
        order = np.argsort(r32["cos_theta"][band], kind="stable")
        assert (np.diff(r32["falloff"][band][order]) >= 0).all()
        assert (np.diff(f_got[band][np.argsort(c[band])]) >= -lc.bar(r32["falloff"], closed, band)).all()


@pytest.mark.parametrize("name", list(lc.SPOTS))
def test_spot_falloff(pt, ob, name):
    s, k = lc.delta_scene(pt, lc.spot_text(name), lr.SPOT)
    l32, l64 = lr.both(s.desc, k)
    spot_falloff_check(name, l32, l64, lambda q: ob.light_probe(s, k, 0, q))


def spot_flux(l64, probe, rows, cols=128):
    """Midpoint quadrature of Li d^2 (bin 0) over the sphere of directions around the light, on a rows x cols grid of
    (theta, phi) about the light's axis (the integrand varies with theta alone, so the rows carry the resolution);
    probe(q) -> mode-0 output, or None for the float64 restatement's falloff."""
    a, b, axis = lc._frame(np.array(lc.SPOT_TO) - np.array(lc.SPOT_FROM))
    th = math.pi * (np.arange(rows) + 0.5) / rows
    ph = 2 * math.pi * (np.arange(cols) + 0.5) / cols
    T, P = np.meshgrid(th, ph, indexing="ij")
    d = (np.cos(T)[..., None] * axis + np.sin(T)[..., None] * (np.cos(P)[..., None] * a + np.sin(P)[..., None] * b)).reshape(-1, 3)
    weight = (np.sin(T) * (math.pi / rows) * (2 * math.pi / cols)).reshape(-1)
    if probe is None:
        return float((lr.spot_falloff(l64, -d)[0] * weight).sum() * l64.L[0])
    q = lc.pack(np.array(lc.SPOT_FROM) + 3 * d, np.zeros((len(d), 3)), np.zeros((len(d), 2)))
    d2 = ((l64.pos - q[:, :3].astype(np.float64)) ** 2).sum(axis=1)
    return float((probe(q)[:, 10].astype(np.float64) * d2 * weight).sum())


def spot_flux_check(name, l64, probe):
    """The flux is I 2 pi [(1 - cs) + (cs - ct) / 5]. The probe answers a 1024 x 128 grid (131 072 queries: 0.18 degrees per
    row, five rows across the narrow cone's band). Tolerance: the quadrature's own error on that grid, taken as the
    difference between the float64 restatement's sums on the 512 x 128 and the 1024 x 128 grids -- the midpoint rule's error
    at least halves per halving of the step (first order across a jump of the integrand, as on the rim of the cone without a
    band; second order elsewhere), so the finer grid's error is at most that difference -- plus 1e-6 of the flux for the
    float32 Li. Without a band (cs == ct) the integrand jumps from I to 0 on the rim, and the difference of two grids says
    nothing about a jump: the row that holds the rim counts wholly or not at all, an error of at most half that row,
    I 2 pi sin(theta_t) (pi / 1024) / 2, which is added."""
    cs, ct = float(l64.cos_falloff_start), float(l64.cos_total_width)
    closed = float(l64.L[0]) * 2 * math.pi * ((1 - cs) + (cs - ct) / 5)
    coarse, fine = spot_flux(l64, None, 512), spot_flux(l64, None, 1024)
    tol = abs(coarse - fine) + 1e-6 * closed
    if cs == ct:
        tol += float(l64.L[0]) * 2 * math.pi * math.sqrt(1 - ct * ct) * (math.pi / 1024) / 2
    got = spot_flux(l64, probe, 1024)
    print("spot %s: flux %.6f, closed form %.6f, off by %.2e, tolerance %.2e (restatement off by %.2e)" % (name, got, closed, abs(got - closed), tol, abs(fine - closed)))
    assert abs(fine - closed) <= tol and abs(got - closed) <= tol


@pytest.mark.parametrize("name", list(lc.SPOTS))
def test_spot_flux(pt, ob, name):
    s, k = lc.delta_scene(pt, lc.spot_text(name), lr.SPOT)
    spot_flux_check(name, lr.Light(s.desc, k, np.float64), lambda q: ob.light_probe(s, k, 0, q))


def test_power_table_carries_the_reference_formulas(pt):
    """Light::Power() of the spot, point and distant lights (spot.cpp:74-76, point.cpp:55, distant.cpp:61-63) through
    SampledSpectrum::y() (spectrum.h:415-421) in the "power" light-selection table, to 4 ulp."""
    body = lc.spot_text("wide") + lc.DELTA["point"] + lc.DELTA["distant"] + lc.BALL
    s = pt.Scene(text=lc.text(body).replace('"integer maxdepth" [2]', '"integer maxdepth" [2] "string lightsamplestrategy" "power"'))
    assert s.errors == [] and s.desc.n_lights == 3 and s.desc.light_distrib.type == 1 and s.desc.light_distrib.n_distributions == 1
    cie_y = np.array(list(s.desc.cie_y), np.float32)
    f = np.float32
    pi = f(math.pi)

    def y(c):
        yy = f(0)
        for i in range(lr.NSPEC):
            yy = yy + cie_y[i] * c[i]
        return max(yy, f(0)) * f(705 - 395) / f(np.float32(106.856895) * f(lr.NSPEC))
    for i in range(3):
        l = lr.Light(s.desc, i)
        if l.type == lr.SPOT:
            power = l.L * f(2) * pi * (f(1) - f(0.5) * (l.cos_falloff_start + l.cos_total_width))
        elif l.type == lr.POINT:
            power = f(4) * pi * l.L
        else:
            assert l.type == lr.DISTANT and l.world_radius > 0
            power = l.L * pi * l.world_radius * l.world_radius
        got = np.float32(s.desc.light_distrib.func[i])
        print("power of light %d (type %d): %.7g, formula %.7g" % (i, l.type, got, y(power)))
        assert got > 0 and _ulp_apart(got, y(power)) <= 4


# ---------------------------------------------------------------------------------------------------------------------
# the triangle emitter's solid angle
def solid_angle(tri, p):
    """Van Oosterom and Strackee: tan(omega / 2) = |a . (b x c)| / (1 + a.b + b.c + c.a) for the unit vectors to the vertices."""
    a, b, c = (lc.unit(v - p) for v in tri)
    num = abs(float(np.dot(a, np.cross(b, c))))
    den = 1 + float(np.dot(a, b)) + float(np.dot(b, c)) + float(np.dot(c, a))
    return 2 * math.atan2(num, den)


def solid_angle_count(l64, p):
    """The smallest power-of-two count of radical-inverse u, up to 2^17, at which the mean of 1 / pdf over Sample(ref, u) of
    the float64 restatement meets 0.002 relative, and the solid angle; None if there is none."""
    omega = solid_angle(l64.tri, p)
    u = lc.radical_pairs(2 ** 17)
    pdf = lr.shape_sample(l64, np.tile(p, (len(u), 1)), u)[2]
    inv = np.where(pdf > 0, 1 / np.where(pdf > 0, pdf, 1), 0)
    for e in range(4, 18):
        if abs(inv[:2 ** e].mean() / omega - 1) <= 0.002:
            return 2 ** e, omega
    return None, omega


def triangle_outside_points(l64):
    c = l64.tri.mean(axis=0)
    n = lr.tri_normal(l64)
    t = lc.unit(l64.tri[1] - l64.tri[0])
    return [c + 2.0 * n + 0.7 * t, c - 1.2 * n - 0.4 * t, c + 0.3 * n + 2.5 * t]


def solid_angle_check(name, l64, probe, who):
    """From three outside points: the mean of 1 / pdf over the radical-inverse u of Shape::SolidAngle is the closed-form solid
    angle to 0.002 at the count the float64 restatement needs (asserted to exist), plus 1e-5 for the float32 pdf (a relative
    error of a few 2^-24 per sample)."""
    for p in triangle_outside_points(l64):
        p = p.astype(np.float32).astype(np.float64)
        n, omega = solid_angle_count(l64, p)
        assert n is not None, (name, p.tolist(), "no count up to 2^17 meets 0.002")
        u = lc.radical_pairs(n)
        got = probe(lc.pack(np.concatenate([p, [0, 0, 0]])[None, :], u))
        assert (got[:, 3] > 0).all()
        mean = float((1 / got[:, 3].astype(np.float64)).mean())
        print("%s: solid angle %.6e, mean of 1 / pdf over %d samples %.6e (%s)" % (name, omega, n, mean, who))
        assert abs(mean / omega - 1) <= 0.002 + 1e-5


@pytest.mark.parametrize("name", list(lc.TRIANGLES))
def test_triangle_solid_angle(pt, ob, name):
    s, k = lc.triangle_scene(pt, name)
    solid_angle_check(name, lr.Light(s.desc, k, np.float64), lambda q: ob.light_probe(s, k, 0, q), "oracle")
