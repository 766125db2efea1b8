"""LightSource "projection" in the front end: the mi_light record and its map, what stays a reported error, the `power`
light distribution, the scene cache, the shading plan; and statements about Projection that the numpy restatement
(projection_light.py) has to satisfy on its own. No GPU."""
import os

import numpy as np
import pytest

import light_cases as lc
import light_restatement as lr
import projection_cases as pc
import projection_light as pl

XFS = list(pc.TRANSFORMS)


def _ulps(a, b):
    return abs(float(a) - float(b)) / float(np.spacing(np.float32(abs(b))))


# -------------------------------------------------------------------------------------------------------------- records
@pytest.mark.parametrize("xf", XFS)
@pytest.mark.parametrize("name", list(pc.MAPS))
def test_the_light_record(pt, tmp_path, name, xf):
    s, k = pc.light_scene(pt, tmp_path, name, xf)
    rec = s.desc.lights[k]
    assert rec.type == 5 == pt.LIGHT_PROJECTION and s.errors == []
    assert list(rec.pos) == (list(pc.POS) if xf != "identity" else [0, 0, 0])   # LightToWorld(0, 0, 0): the translation, exactly
    _, _, res, level0 = pc.MAPS[name]
    want = pl.screen_bounds(res, np.float32)
    assert np.array_equal(np.array(list(rec.screen), np.float32), want), (list(rec.screen), want)
    if name == "4x2":
        assert list(rec.screen) == [-2, -1, 2, 1]        # aspect > 1
    if name == "2x4":
        assert list(rec.screen) == [-1, -2, 1, 2]        # aspect < 1
    if name == "none":
        assert list(rec.screen) == [-1, -1, 1, 1]        # aspect = 1
    assert rec.hither == float(pl.HITHER)
    c64 = pl.cos_total_width(pc.FOV, pl.screen_bounds(res, np.float64), np.float64)
    assert _ulps(rec.cos_total_width, c64) <= 4, (rec.cos_total_width, c64)
    m64, _ = pl.perspective(pc.FOV, np.float64)
    got = np.array(list(rec.proj), np.float64).reshape(4, 4)
    assert np.abs(got - m64).max() <= 4 * 2.0 ** -23 * np.abs(m64).max() and np.array_equal(got == 0, m64 == 0)
    # the 3x3 of the CTM and of its stored inverse
    if xf == "identity":
        assert np.array_equal(np.array(list(rec.w2l)).reshape(3, 3), np.eye(3))
    else:
        prod = np.array(list(rec.l2w), np.float64).reshape(3, 3) @ np.array(list(rec.w2l), np.float64).reshape(3, 3)
        assert np.abs(prod - np.eye(3)).max() < 1e-6
        assert abs(np.linalg.det(np.array(list(rec.l2w), np.float64).reshape(3, 3)) - 1.0) < 1e-5   # Scale 1 2 .5 keeps the volume ...
        assert np.linalg.norm(np.array(list(rec.l2w), np.float64).reshape(3, 3), axis=0).round(4).tolist() == [1, 2, .5]   # ... not the lengths
    # the map
    if name == "none":
        assert rec.proj_map == -1 and s.desc.n_envmaps == 0
        assert list(rec.proj_centre) == [1.0] * 31
    else:
        assert rec.proj_map == 0 and s.desc.n_envmaps == 1
        e = s.desc.envmaps[0]
        assert (e.width, e.height) == level0 and (e.nu, e.nv) == (0, 0)
        assert not e.cond_func and not e.cond_cdf and not e.cond_func_int and not e.marg_func and not e.marg_cdf
        m = pl.Map(e)
        assert np.isfinite(m.rgb).all() and (m.rgb >= 0).any()
        centre = np.array(list(rec.proj_centre))
        assert (centre > 0).all() and np.isfinite(centre).all()
    if name == "4x2":   # a power of two: level 0 is the file, top row first, no flip
        _, img = pc.write_map(tmp_path, name)
        assert np.array_equal(pl.Map(s.desc.envmaps[0]).rgb, img)
    if name == "2x4":   # PNG: ReadImage hands out value / 255.f as it is (imageio.cpp:270-280; the inverse gamma is ImageTexture's)
        _, img = pc.write_map(tmp_path, name)
        assert np.array_equal(pl.Map(s.desc.envmaps[0]).rgb, img.astype(np.float32) / np.float32(255))


def test_intensity_is_I_times_scale(pt, tmp_path):
    params = '"rgb I" [3 2 1] "rgb scale" [.5 2 4]'
    body = 'LightSource "projection" %s\nLightSource "point" %s\n' % (params, params) + lc.BALL
    s = pt.Scene(text=lc.text(body))
    assert s.errors == [] and s.desc.n_lights == 2
    proj, point = s.desc.lights[0], s.desc.lights[1]
    assert proj.type == 5 and point.type == lr.POINT
    assert list(proj.L) == list(point.L) and any(proj.L)
    default = pt.Scene(text=lc.text('LightSource "projection"\n' + lc.BALL))   # I = 1, scale = 1, fov = 45, no map
    assert default.errors == [] and list(default.desc.lights[0].L) == [1.0] * 31
    m64, _ = pl.perspective(45.0, np.float64)
    assert abs(default.desc.lights[0].proj[0] / m64[0, 0] - 1) < 1e-6


def test_a_file_that_cannot_be_read_is_one_error_and_a_light_without_a_map(pt, tmp_path):
    body = pc.light_text("no_such_map.pfm") + lc.BALL
    s = pt.Scene(text=lc.text(body), base_dir=str(tmp_path))
    assert len(s.errors) == 1 and "no_such_map.pfm" in s.errors[0], s.errors
    assert s.desc.n_lights == 1 and s.desc.n_envmaps == 0
    rec = s.desc.lights[0]
    assert rec.type == 5 and rec.proj_map == -1 and list(rec.screen) == [-1, -1, 1, 1] and list(rec.proj_centre) == [1.0] * 31
    ok = pt.Scene(text=lc.text(pc.light_text() + lc.BALL))
    assert bytes(ok.desc.lights[0]) == bytes(rec)   # the light a scene without "mapname" builds


def test_goniometric_is_still_reported_beside_a_projection_that_is_built(pt):
    body = 'LightSource "goniometric" "rgb I" [1 1 1]\n' + pc.light_text() + lc.BALL
    s = pt.Scene(text=lc.text(body))
    assert len(s.errors) == 1 and 'LightSource "goniometric"' in s.errors[0] and "outside the hot-path scope" in s.errors[0]
    assert s.desc.n_lights == 1 and s.desc.lights[0].type == 5


def test_an_animated_ctm_takes_the_start_transform_with_the_warning(pt):
    body = ('ActiveTransform EndTime\nTranslate 5 0 0\nActiveTransform All\nTranslate 1 2 3\n' + pc.light_text() + lc.BALL)
    s = pt.Scene(text=lc.text(body))
    assert s.desc.n_lights == 1 and s.desc.lights[0].type == 5
    assert list(s.desc.lights[0].pos) == [1, 2, 3]
    assert any('"LightSource"' in w and "start transform" in w for w in s.warnings), s.warnings


# ---------------------------------------------------------------------------------------------------------------- power
@pytest.mark.parametrize("name", ["4x2", "none"])
def test_power_strategy_takes_the_restated_power(pt, tmp_path, name):
    fname, _ = pc.write_map(tmp_path, name)
    body = lc.DELTA["point"] + "AttributeBegin\n" + pc.TRANSFORMS["rotated and scaled"] + pc.light_text(fname) + "AttributeEnd\n" + lc.BALL
    text = lc.text(body).replace('Integrator "path"', 'Integrator "path" "string lightsamplestrategy" "power"')
    s = pt.Scene(text=text, base_dir=str(tmp_path))
    assert s.errors == [] and s.desc.n_lights == 2 and s.desc.light_distrib.type == 1   # MI_LD_POWER
    point, proj = lc.light_of(s, lr.POINT), lc.light_of(s, pl.PROJECTION)
    func = np.array([s.desc.light_distrib.func[i] for i in range(2)], np.float32)
    want = {}
    for f in (np.float32, np.float64):
        cie = np.array(list(s.desc.cie_y), np.float32).astype(f)
        p_point = f(4) * f(np.float32(np.pi)) * lr.Light(s.desc, point, f).L          # point.cpp:55
        p_proj = pl.power(pl.Light(s.desc, proj, f))
        want[f] = np.array([pl.spectrum_y(p_point, cie) if i == point else pl.spectrum_y(p_proj, cie) for i in range(2)], f)
    log = []
    lc.check_rel("power, map %s" % name, "func", func, want[np.float32], want[np.float64], np.ones(2, bool), log)
    print("\n".join(log))
    assert func[proj] > 0 and func[point] > 0
    if name == "none":   # Spectrum(1) * I * 2 pi (1 - cosTotalWidth) against the point light's 4 pi I with the same I
        assert abs(func[proj] / func[point] - (1 - s.desc.lights[proj].cos_total_width) / 2) < 1e-6


# ---------------------------------------------------------------------------------------------------------------- cache
def test_scene_cache_keeps_the_light_and_its_map(pt, tmp_path):
    s, k = pc.light_scene(pt, tmp_path, "3x5", "rotated and scaled")
    path = os.path.join(str(tmp_path), "projection.cache")
    s.save_cache(path)
    r = pt.Scene(cache=path)
    assert r.desc.n_lights == 1 and r.desc.n_envmaps == 1
    assert bytes(r.desc.lights[0]) == bytes(s.desc.lights[0])
    a, b = s.desc.envmaps[0], r.desc.envmaps[0]
    assert (a.width, a.height, a.nu, a.nv) == (b.width, b.height, b.nu, b.nv) == (4, 8, 0, 0)
    assert pl.Map(a).rgb.tobytes() == pl.Map(b).rgb.tobytes()
    assert not b.cond_func and not b.marg_cdf
    # a cache of the build before this light (its magic number, its mi_light) is refused, not misread
    raw = bytearray(open(path, "rb").read())
    assert bytes(raw[:8]) == b"MIPTSC10"
    for label, patch in (("the earlier magic", {6: ord("0"), 7: ord("9")}), ("another ABI number", {8: raw[8] - 1})):
        old = bytearray(raw)
        for at, v in patch.items():
            old[at] = v
        stale = os.path.join(str(tmp_path), "stale.cache")
        with open(stale, "wb") as f:
            f.write(bytes(old))
        with pytest.raises(RuntimeError, match="not a scene cache of this build"):
            pt.Scene(cache=stale)


# ----------------------------------------------------------------------------------------------------------------- plan
TRI = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-3 -3 -1  3 -3 -1  0 3 -1]\n'
PLAN_BODY = '%s' + 'Material "matte"\n' + TRI + 'Material "plastic"\n' + TRI + 'Material "glass"\n' + TRI + 'Material "uber" "rgb Kr" [.3 .3 .3]\n' + TRI


def _routes(s):
    plan = s.shade_plan()
    mats = []
    for i in range(s.desc.n_prims):
        if s.desc.prims[i].material not in mats:
            mats.append(s.desc.prims[i].material)
    classes = [plan["material_class"][m] for m in mats]
    return [(plan["classes"][c]["nl"], plan["classes"][c]["tm"]) for c in classes], plan


def test_classes_of_a_projection_scene_go_to_the_general_instances(pt):
    point, _ = _routes(pt.Scene(text=lc.text(PLAN_BODY % lc.DELTA["point"])))
    cold = pt.TM_LIGHTS_ALL | pt.TM_SAMPLERS
    assert point == [(2, pt.TM_DIFFUSE | pt.TM_LIGHTS_NO_ENV), (2, pt.TM_PLASTIC | pt.TM_LIGHTS_NO_ENV), (2, pt.TM_GLASS | cold),
                     (4, pt.TM_UBER | cold)]            # the parent's routes
    s = pt.Scene(text=lc.text(PLAN_BODY % pc.light_text()))
    assert s.errors == []
    proj, plan = _routes(s)
    assert proj == [(2, pt.TM_GENERIC), (2, pt.TM_GENERIC), (2, pt.TM_GENERIC), (4, pt.TM_GENERIC)]
    for c, k in plan["classes"].items():   # every class, the escaped rays' too: an instance that holds the projection's code
        assert k["tm"] | pt.TM_INSTANCES | pt.TM_TEXTURED == pt.TM_ALL, (c, hex(k["tm"]))
    # one projection light beside others moves the classes too; with object instances everything is on TM_ALL already
    mixed, _ = _routes(pt.Scene(text=lc.text(PLAN_BODY % (lc.DELTA["point"] + pc.light_text()))))
    assert mixed == proj
    inst, _ = _routes(pt.Scene(text=lc.text((PLAN_BODY % pc.light_text()) + 'ObjectBegin "o"\n' + TRI + 'ObjectEnd\nObjectInstance "o"\n')))
    assert set(tm for _, tm in inst) == {pt.TM_ALL}


def test_no_instance_was_added(pt):
    assert len(pt.shade_instances()) == 21


# ------------------------------------------------------------------------------------ Projection, on the restatement itself
def _lights(pt, tmp_path, name, xf):
    s, k = pc.light_scene(pt, tmp_path, name, xf)
    return pl.both(s.desc, k)


@pytest.mark.parametrize("xf", XFS)
def test_projection_is_zero_behind_the_light(pt, tmp_path, xf):
    l32, l64 = _lights(pt, tmp_path, "4x2", xf)
    rng = np.random.default_rng(5)
    local = np.concatenate([lc.uniform_directions(rng, 400) * [1, 1, 0] + [0, 0, -1e-6], -np.abs(lc.uniform_directions(rng, 400))])
    local = local[local[:, 2] < 0]
    w = lc.unit(local @ l64.l2w.T)
    for light in (l32, l64):
        r = pl.projection(light, w.astype(light.f))
        assert r["behind"].all() and not r["value"].any()
        front = pl.projection(light, lc.unit(np.array([[0.01, 0.02, 1.0]]) @ l64.l2w.T).astype(light.f))
        assert not front["behind"][0] and front["value"].all()


@pytest.mark.parametrize("name", ["4x2", "2x4", "none"])
def test_projection_is_zero_outside_the_bounds_and_not_on_them(pt, tmp_path, name):
    """In the light's own frame (identity CTM) with wl = (px z / invTan, py z / invTan, z), z a power of two: the
    projection gives p back up to the rounding of two multiplications, so the edge is found by walking p itself."""
    l32, l64 = _lights(pt, tmp_path, name, "identity")
    for light in (l32, l64):
        f = light.f
        sc = light.screen
        for axis, edge, outward in ((0, sc[0], -1), (0, sc[2], 1), (1, sc[1], -1), (1, sc[3], 1)):
            p = np.zeros((3, 2), f)
            p[:, 1 - axis] = f(0.25)
            p[:, axis] = [np.nextafter(edge, f(-outward) * f(np.inf)), edge, np.nextafter(edge, f(outward) * f(np.inf))]
            # Bounds2::Inside is inclusive at both ends: on the edge and one float inside it is lit, one float outside is not
            sc_ = light.screen
            inside = (p[:, 0] >= sc_[0]) & (p[:, 0] <= sc_[2]) & (p[:, 1] >= sc_[1]) & (p[:, 1] <= sc_[3])
            assert inside.tolist() == [True, True, False]
            # and Projection decides the same from a direction that projects onto exactly those p: with invTan replaced by 1
            # the perspective matrix's first two rows are the identity, so wl = (p.x, p.y, 1) projects to p (wp == 1: no division)
            unit_light = pl.Light.__new__(pl.Light)
            unit_light.__dict__.update(light.__dict__)
            unit_light.proj = light.proj.copy()
            unit_light.proj[0, 0] = unit_light.proj[1, 1] = f(1)
            wl = np.concatenate([p, np.ones((3, 1), f)], axis=1)
            r = pl.projection(unit_light, wl)
            assert np.array_equal(r["p"], p)
            assert r["inside"].tolist() == [True, True, False] and (~r["behind"]).all()
            assert r["value"][0].any() and r["value"][1].any() and not r["value"][2].any()


def test_the_bright_column_of_the_4x2_map_lands_where_offset_says(pt, tmp_path):
    """Column 2 of four is bright: its centre is st.s = 2.5 / 4, p.x = 0.5 of the screen's [-2, 2]; bilinear blending with it
    ends at the centres of the columns beside it, beyond which the dim texels are alone (Repeat blends column 0 with column 3)."""
    for light in _lights(pt, tmp_path, "4x2", "identity"):
        f = light.f
        inv_tan = float(light.proj[0, 0])
        px = np.linspace(-1.95, 1.95, 79)
        py = np.full_like(px, 0.5)
        wl = np.stack([px / inv_tan, py / inv_tan, np.ones_like(px)], axis=1).astype(f)
        r = pl.projection(light, wl)
        assert np.abs(r["st"][:, 0] - (px + 2) / 4).max() < 1e-6 and np.abs(r["st"][:, 1] - 0.75).max() < 1e-6
        y = r["value"].sum(axis=1)
        s = (px + 2) / 4
        bright = np.abs(s - 0.625) < 0.03                    # around the centre of column 2
        dim = (s < 0.375 + 0.01) | (s > 0.875 - 0.01)         # up to the centre of column 1, from the centre of column 3 on
        assert bright.sum() >= 4 and dim.sum() >= 40
        assert y[bright].min() > 5 * y[dim].max()
        assert np.argmax(y) in np.nonzero((s > 0.5) & (s < 0.75))[0]


@pytest.mark.parametrize("xf", XFS)
@pytest.mark.parametrize("name", list(pc.MAPS))
def test_float32_and_float64_agree_on_all_but_one_percent(pt, tmp_path, name, xf):
    """The in / out decision of every query family that is not built on an edge: at most 1 % unsure; and the float32 values
    follow the float64 ones."""
    l32, l64 = _lights(pt, tmp_path, name, xf)
    total = 0
    for fam in pc.families(l64, np.random.default_rng(43)):
        r32, r64 = pl.sample_li(l32, fam.q[:, :3]), pl.sample_li(l64, fam.q[:, :3])
        unsure = r32["black"] != r64["black"]
        total += len(fam.q)
        if not fam.rim:
            assert unsure.mean() <= 0.01, (fam.name, float(unsure.mean()))
        lit = ~unsure & ~r64["black"]
        if fam.name in ("inside the frustum", "texel centres", "texel borders", "near and far"):
            assert lit.mean() >= 0.99, fam.name
        if fam.name == "outside the screen bounds":
            assert r64["black"].all() and not r64["behind"].any()
        if lit.any():
            a, b = r32["Li"][lit].astype(np.float64), r64["Li"][lit]
            big = b > 1e-3 * b.max(axis=1, keepdims=True)
            assert np.abs(a[big] / b[big] - 1).max() < 2e-3, fam.name
    assert 1500 <= total <= 2600
    d2 = pl.sample_li(l64, pc.families(l64, np.random.default_rng(43))[-1].q[:, :3])["d2"]
    assert d2.min() < 2e-4 and d2.max() > 5e7
