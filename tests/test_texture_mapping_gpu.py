"""MIPT_TEXTURES=all on the GPU: the mappings "spherical", "cylindrical", "planar" and the classes "dots", "uv", "bilerp", float and
3-D "checkerboard". The frozen oracle knows none of them, so the method is the noise textures' (test_noise_texture_gpu.py):
the device answers single queries through mi_pt_texture_eval_probe and is held to texture_mapping.py, the float32 / float64
numpy restatement, with disk_shape.bar -- four times the worst float32-to-float64 deviation of the restatement over the group,
never below 8 ulp -- over the queries on which both precisions take the same discrete decisions (at most 2 % of a group may
be left out; in the one group built on the decision boundaries the device has to take one of the two sides); an image
texture under a mapping is the existing MIPMap lookup (held to the oracle elsewhere) at the probed st; whole renders are held
to a twin render (a constant, or a uniform image, in the texture's place) times the restated value at each pixel's hit."""
import numpy as np
import pytest

import disk_shape as ds
import noise_texture as nt
import scenes_text as st
import sphere_shape as ss
import test_noise_texture_gpu as nz
import texture_mapping as tm
import texture_mapping_cases as tc

pytestmark = pytest.mark.gpu

_cache = {}


@pytest.fixture(autouse=True)
def _switch(monkeypatch):
    monkeypatch.setenv("MIPT_TEXTURES", "all")


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("texture_mapping_gpu"))
    st.write_texture_files(d)
    tc.write_grey_image(d)
    return d


def _basis(scene):
    return np.array([list(row) for row in scene.desc.rgb_illum], np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# 6, 7: the probe against the restatement
def _probe_scene(pt, images):
    if "probe" not in _cache:
        text, index = tc.scene_text()
        s = pt.Scene(text=text, base_dir=images)
        assert s.errors == [], s.errors
        _cache["probe"] = (s, pt.CreateIntegrator(s), index, tc.groups())
    return _cache["probe"]


def _hold_columns(name, dev, v32, v64, judged, capped):
    """Per column: |device - float64 restatement| <= bar over the judged queries; the others take one of the two sides."""
    n = len(dev)
    dev, v32, v64 = (a.reshape(n, -1) for a in (dev, v32, v64))
    assert np.isfinite(dev).all(), name
    share = 1 - judged.mean()
    if capped:
        assert share <= .02, (name, share)
    worst_rel = 0.
    for k in range(dev.shape[1] if dev.shape[1] <= 6 else 1):
        cols = slice(k, k + 1) if dev.shape[1] <= 6 else slice(None)        # (a spectrum's bins share one bar)
        bar = ds.bar(v32[:, cols], v64[:, cols], judged)
        err = np.abs(dev[:, cols].astype(np.float64) - v64[:, cols])
        worst = float(err[judged].max()) if judged.any() else 0.
        worst_rel = max(worst_rel, worst / bar if bar > 0 else 0.)
        assert worst <= bar, (name, k, worst, bar)
        if not judged.all():
            side = np.minimum(err, np.abs(dev[:, cols].astype(np.float64) - v32[:, cols].astype(np.float64)))[~judged]
            assert side.max() <= bar, (name, k, float(side.max()), bar)
    print("%-76s n %4d  unjudged %5.2f %%  worst deviation / bar %.3f" % (name, n, 100 * share, worst_rel))


@pytest.mark.parametrize("i", range(len(tc.CASES)), ids=[c[0] for c in tc.CASES])
def test_probe_against_the_restatement(pt, images, i):
    s, integ, index, groups = _probe_scene(pt, images)
    tex = index[i]
    rec = s.desc.textures[tex]
    image = rec.type == tm.TEX_IMAGEMAP
    varied = False
    for name, q in groups.items():
        label = "%s, %s" % (tc.CASES[i][0], name)
        if rec.type != tm.TEX_CHECKERBOARD3D:
            v32, v64, judged = tc.restate(rec, q, _basis(s), 0)
            st_dev = integ.texture_eval_probe(tex, 0, q)
            _hold_columns(label + ", mode 0", st_dev, v32, v64, judged, name != tc.NEAR)
        value = integ.texture_eval_probe(tex, 1, q)
        if not image:
            v32, v64, judged = tc.restate(rec, q, _basis(s), 1)
            if rec.is_float:
                assert not value[:, 1:].any()
                value = value[:, 0]
            _hold_columns(label + ", mode 1", value, v32, v64, judged, name != tc.NEAR)
            continue
        # 7: an image texture under a mapping is MIPMap::Lookup at the mapped st, converted as EvalImageTexture converts it
        rgb = integ.texture_lookup(tex, st_dev)
        assert np.isfinite(rgb).all()
        varied |= bool(rgb.max() > rgb.min())      # (a footprint wider than the image reads the one texel of the last level)
        if rec.is_float:
            want = np.zeros_like(value)
            want[:, 0] = rgb[:, 0] * np.float32(rec.post_scale)
        else:
            assert np.array_equal(rgb[:, 0], rgb[:, 1]) and np.array_equal(rgb[:, 0], rgb[:, 2])       # grey
            want = tm.from_rgb(rgb.astype(np.float32), _basis(s))
        print("%-76s n %4d  worst |mode 1 - converted lookup| %.3e" % (label, len(q), float(np.abs(value - want).max())))
        assert np.array_equal(value, want), label
    assert varied or not image


def test_probe_refuses_what_it_cannot_answer(pt, images):
    s, integ, index, _ = _probe_scene(pt, images)
    q = np.zeros((3, 15), np.float32)
    q[:, 0] = 1
    three_d = index[[c[0] for c in tc.CASES].index("3-D checkerboard")]
    assert integ.texture_eval_probe(three_d, 1, q).shape == (3, 31)
    for tex, mode in ((three_d, 0), (-1, 1), (s.desc.n_textures, 1), (0, 2), (0, -1)):
        with pytest.raises(RuntimeError):
            integ.texture_eval_probe(tex, mode, q)
    with pytest.raises(RuntimeError):
        integ.texture_probe(0, np.zeros((1, 9), np.float32))        # mi_pt_texture_probe keeps its contract: noise only


# ---------------------------------------------------------------------------------------------------------------------
# 8: whole renders
KD = {
    "uv": 'Texture "kd" "spectrum" "uv" "float uscale" [3] "float vscale" [2] "float udelta" [.25]',
    "dots": 'Texture "kd" "spectrum" "dots" "float uscale" [6] "float vscale" [5] "rgb inside" [.8 .1 .1] "rgb outside" [.1 .2 .9]',
    "3-D checkerboard": 'Texture "kd" "spectrum" "checkerboard" "integer dimension" [3] "rgb tex1" [.9 .9 .2] "rgb tex2" [.1 .3 .1]',
    "planar checkerboard": 'Texture "kd" "spectrum" "checkerboard" "string mapping" "planar" "vector v1" [1.5 0 .5] "vector v2" [0 2 .3] "rgb tex1" [.9 .9 .9] "rgb tex2" [.2 .1 .3]',
    "spherical image": 'Texture "kd" "spectrum" "imagemap" "string filename" "grey.pfm" "string mapping" "spherical"',
}
UNIFORM_GREY = np.float32(.5)
TWIN_IMAGE = 'Texture "kd" "spectrum" "imagemap" "string filename" "uniform/grey.pfm"'


def _render_pair(pt, images, texture, twin_texture, **kw):
    key = (texture, twin_texture, tuple(sorted(kw.items())))
    if key not in _cache:
        s, twin = pt.Scene(text=nz._colour_text(texture, **kw), base_dir=images), pt.Scene(text=nz._colour_text(twin_texture, **kw), base_dir=images)
        assert s.errors == [] and twin.errors == [], (s.errors, twin.errors)
        integ = pt.CreateIntegrator(s)
        film, weight = integ.Render()
        tfilm, tweight = pt.CreateIntegrator(twin).Render()
        assert np.array_equal(weight, tweight)
        _cache[key] = (s, twin, integ, film, tfilm, weight)
    return _cache[key]


def _queries(scene, rays, hits, f):
    """What k_shade hands the texture at each camera ray's hit: nz._surface's p, dpdx, dpdy and (dudx, dvdx, dudy, dvdy), and the
    hit's (u, v) -- of the world triangles, of the instance's triangles (in the instance's space) and of the sphere."""
    surf = nz._surface(scene, rays, hits, f)
    d = scene.desc
    uv = np.zeros((len(rays), 2), f)
    prim = hits[:, 0].copy().view(np.int32)
    shape = np.array([d.prims[k].shape if k >= 0 else 0 for k in prim])
    cls = surf["classes"]
    if cls["quad"].any():
        uv[cls["quad"]] = nz._tri_point(scene, shape[cls["quad"]], rays[cls["quad"], 0:7], f)[4]
    if cls["instance"].any():
        w2i = np.array(list(d.instances[0].w2i), np.float64).astype(f).reshape(4, 4)
        local = np.concatenate([ds.xf_ray(w2i, rays[r:r + 1, 0:7]) for r in np.flatnonzero(cls["instance"])])
        uv[cls["instance"]] = nz._tri_point(scene, shape[cls["instance"]], local, f)[4]
    if cls["sphere"].any():
        uv[cls["sphere"]] = ss.intersect(ss.Sphere(d.spheres[0], f), rays[cls["sphere"], 0:7])["uv"]
    q = np.concatenate([surf["p"], surf["dpdx"], surf["dpdy"], uv, surf["duv"]], axis=1)
    return surf, np.where(surf["hit"][:, None], q, f(1))      # (a missed pixel: any harmless point)


def _check_render(pt, images, case, integrator=nz.PATH):
    image = case == "spherical image"
    if image:
        import os
        os.makedirs(os.path.join(images, "uniform"), exist_ok=True)
        tc.write_grey_image(os.path.join(images, "uniform"), uniform=UNIFORM_GREY)
    s, twin, integ, film, tfilm, weight = _render_pair(pt, images, KD[case], TWIN_IMAGE if image else nz.CONSTANT_KD, integrator=integrator)
    rays, hits = nz._camera_and_hits(integ, s)
    lists = nz._samples_of_pixels(s, rays, weight)
    (a, q32), (b, q64) = _queries(s, rays, hits, np.float32), _queries(s, rays, hits, np.float64)
    tex = [i for i in range(s.desc.n_textures)][-1]
    rec = s.desc.textures[tex]
    hit = a["hit"]
    if image:
        # the value is the device's own MIPMap lookup (held to the oracle by the existing suite) at the restated st, grey -> FromRGB
        t32, t64 = tm.both(rec)
        c32, d32 = tm.map2d(t32, q32[:, 0:3], q32[:, 3:6], q32[:, 6:9], q32[:, 9:11], q32[:, 11:15])
        c64, d64 = tm.map2d(t64, q64[:, 0:3], q64[:, 3:6], q64[:, 6:9], q64[:, 9:11], q64[:, 11:15])
        look = lambda c: tm.from_rgb(integ.texture_lookup(tex, c.astype(np.float32)).astype(np.float64), _basis(s))
        v32, v64 = look(c32), look(c64)
        same = tm.same_decisions(d32, d64)
        kd = tm.from_rgb(np.full((1, 3), UNIFORM_GREY, np.float64), _basis(s))[0]
    else:
        (v32, d32), (v64, d64) = tm.evaluate(tm.Tex(rec, np.float32), q32, _basis(s)), tm.evaluate(tm.Tex(rec, np.float64), q64, _basis(s))
        same = tm.same_decisions(d32, d64)
        kd = nz._kd_of(twin)
    nb = kd.size
    assert (kd > 0).all() and film.shape[2] >= nb and not film[:, :, nb:].any()
    film, tfilm = film.reshape(len(rays), -1)[:, :nb].astype(np.float64), tfilm.reshape(len(rays), -1)[:, :nb].astype(np.float64)
    undecided = hit & ~same
    print("%s: samples on which the two precisions decide differently: %d of %d hits" % (case, undecided.sum(), hit.sum()))
    assert undecided.sum() <= .02 * hit.sum()
    gain, gain_tol = np.zeros((len(rays), nb)), np.zeros((len(rays), nb))
    for name, sel in a["classes"].items():
        assert sel.sum() >= 40, (name, sel.sum())
        bar = ds.bar(v32, v64, sel & same)
        print("%-9s samples %4d, value in [%.3f, %.3f], bar %.3e" % (name, sel.sum(), v64[sel].min(), v64[sel].max(), bar))
        gain[sel] = v64[sel] / kd
        gain_tol[sel] = bar / kd
        if image:       # the twin's own lookup is a weighted mean of equal texels: the texel up to a few ulp
            gain_tol[sel] += 8 * float(np.finfo(np.float32).eps) * gain[sel]
    # where the precisions decide differently the device takes one of the two sides
    gain_tol[undecided] += np.abs(v32[undecided].astype(np.float64) - v64[undecided]) / kd
    nz._hold_film(case, film, tfilm, lists, gain, gain_tol, a["classes"])
    # the texture shows: the picture is not the twin's, and the value varies over every shape
    assert nz._rel_l2(film, tfilm) > 1e-2
    for name, sel in a["classes"].items():
        assert np.ptp(v64[sel].sum(axis=1)) > .05 * np.abs(v64[sel].sum(axis=1)).max(), name
    missed = np.array([not any(hit[j] for j in l) for l in lists])
    assert missed.any() and np.array_equal(film[missed], tfilm[missed])
    assert np.isfinite(film).all()


@pytest.mark.parametrize("case", list(KD))
def test_colour_whole_render(pt, images, case):
    _check_render(pt, images, case)


def test_colour_whole_render_spectralpath(pt, images):
    _check_render(pt, images, "dots", integrator=nz.SPECTRAL)


# ---------------------------------------------------------------------------------------------------------------------
# 9: bump
# (trilinear: that lookup is continuous in st, so the float32 and float64 restatements of a difference quotient of displacements stay
# together; EWA's weight table and integer ellipse bounds step at the 1e-3 level, which the division by du ~ 1e-2 turns into a bar as
# wide as the effect -- measured: bar 8e-3 against ratios in [.71, 1.14])
BUMP = ('Texture "w" "float" "imagemap" "string filename" "rough.pfm" "string mapping" "cylindrical" "bool trilinear" "true"\n'
        'Texture "b" "float" "scale" "texture tex1" "w" "float tex2" [.5]')


def _bump_text(bumped):
    mat = 'Material "matte" "rgb Kd" [.6 .6 .6]' + (' "texture bumpmap" "b"\n' if bumped else "\n")
    return (nz.HEAD % dict(times="", res=32, spp=1, integrator=nz.PATH) + "TransformBegin\n" + nz.TEXTURE_CTM + BUMP + "\nTransformEnd\n" + mat +
            "AttributeBegin\n" + nz.BUMP_QUAD + "AttributeEnd\nWorldEnd\n")


def _bump_ratio(integ, tex, rec, surf, f, shift_p):
    """Material::Bump (material.cpp:47-84) on the flat quad (dndu = dndv = 0) with the cylindrical-mapped image as displacement
    -> |ns' . wi| / |ns . wi|. The displacement at a point is the device's MIPMap lookup at the restated st (precision f)."""
    t = tm.Tex(rec, f)
    p, ng, dpdx, dpdy, duv = surf["p"], surf["n"], surf["dpdx"], surf["dpdy"], surf["duv"]
    zero2, zero4 = np.zeros((len(p), 2), f), np.zeros((len(p), 4), f)

    def displacement(at):
        c, _ = tm.map2d(t, at, dpdx, dpdy, zero2, zero4)
        return integ.texture_lookup(tex, c.astype(np.float32))[:, 0].astype(f) * t.post_scale
    du = nt._lit(f, .5) * (np.abs(duv[:, 0]) + np.abs(duv[:, 2]))
    du = np.where(du == 0, nt._lit(f, .0005), du)
    dv = nt._lit(f, .5) * (np.abs(duv[:, 1]) + np.abs(duv[:, 3]))
    dv = np.where(dv == 0, nt._lit(f, .0005), dv)
    pu = p + du[:, None] * surf["dpdu"] if shift_p else p
    pv = p + dv[:, None] * surf["dpdv"] if shift_p else p
    d0, d_u, d_v = displacement(p), displacement(pu), displacement(pv)
    new_dpdu = surf["dpdu"] + ((d_u - d0) / du)[:, None] * ng
    new_dpdv = surf["dpdv"] + ((d_v - d0) / dv)[:, None] * ng
    ns = ds.normalize(ds.cross(new_dpdu, new_dpdv))
    dot = lambda x, y: x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1] + x[:, 2] * y[:, 2]
    ns = np.where((dot(ns, ng) < 0)[:, None], -ns, ns)
    wi = nz.LIGHT_POS.astype(f)[None, :] - p
    return np.abs(dot(ns, wi)) / np.abs(dot(ng, wi))


def test_bump_whole_render(pt, images):
    s, twin = pt.Scene(text=_bump_text(True), base_dir=images), pt.Scene(text=_bump_text(False), base_dir=images)
    assert s.errors == [] and twin.errors == [], s.errors
    integ = pt.CreateIntegrator(s)
    film, weight = integ.Render()
    tfilm, _ = pt.CreateIntegrator(twin).Render()
    tex = s.desc.materials[s.desc.prims[0].material].bump_tex
    rec = s.desc.textures[tex]
    assert (rec.type, rec.mapping, rec.post_scale) == (tm.TEX_IMAGEMAP, tm.MAP_CYLINDRICAL, .5)
    rays, hits = nz._camera_and_hits(integ, s)
    lists = nz._samples_of_pixels(s, rays, weight)
    a, b = nz._surface(s, rays, hits, np.float32, instance_mesh=-2), nz._surface(s, rays, hits, np.float64, instance_mesh=-2)
    film, tfilm = film.reshape(len(rays), -1)[:, :31].astype(np.float64), tfilm.reshape(len(rays), -1)[:, :31].astype(np.float64)
    sel = a["hit"] & (tfilm[:, 0] > 0)
    assert sel.sum() >= 300
    cut = lambda x: {k: (v[sel] if isinstance(v, np.ndarray) else v) for k, v in x.items()}
    r32, r64 = _bump_ratio(integ, tex, rec, cut(a), np.float32, True), _bump_ratio(integ, tex, rec, cut(b), np.float64, True)
    bar = ds.bar(r32, r64, slice(None))
    still = _bump_ratio(integ, tex, rec, cut(b), np.float64, False)
    apart = np.abs(still - r64) > 10 * bar
    print("bump: samples %d, bar %.3e, ratio in [%.3f, %.3f], |shifted - unshifted| > 10 bars on %d" % (sel.sum(), bar, r64.min(), r64.max(), apart.sum()))
    assert apart.sum() >= sel.sum() / 2
    gain, gain_tol = np.ones((len(rays), 31)), np.zeros((len(rays), 31))
    gain[sel], gain_tol[sel] = r64[:, None], bar
    nz._hold_film("bump", film, tfilm, lists, gain, gain_tol, dict(quad=sel))


# ---------------------------------------------------------------------------------------------------------------------
# 10: schedules; routing
def test_pool_passes_and_shards_give_the_same_film(pt, images):
    s = pt.Scene(text=nz._colour_text(KD["dots"], spp=4), base_dir=images)
    assert s.errors == []
    integ = pt.CreateIntegrator(s)
    film, weight = integ.Render()
    assert film.any()
    small, w = integ.Render(path_pool=256)
    print("pool 256: relative L2 %.3e" % nz._rel_l2(small, film))
    assert np.array_equal(w, weight) and nz._rel_l2(small, film) < 1e-6
    integ.Render(spp=1, sample_begin=0, download=False)
    two, w = integ.Render(spp=3, sample_begin=1, accumulate=True)
    print("two passes: relative L2 %.3e" % nz._rel_l2(two, film))
    assert np.array_equal(w, weight) and nz._rel_l2(two, film) < 1e-6
    acc, accw = np.zeros_like(film), np.zeros_like(weight)
    for r in range(2):
        f, w = integ.Render(shard_index=r, shard_count=2)
        acc += f
        accw += w
    print("two shards: relative L2 %.3e" % nz._rel_l2(acc, film))
    assert np.array_equal(accw, weight) and nz._rel_l2(acc, film) < 1e-6


def test_every_binding_renders(pt, images):
    """The front-end tests' scene of bindings (colours of five material families, a scaled colour, sigma, bump, the roughness maps)
    passes mi_pt_create's validation and renders a finite picture that its textures shape."""
    import texture_mapping_scenes as ts
    s = pt.Scene(text=ts.text("bindings"), base_dir=images)
    assert s.errors == [], s.errors
    film, _ = pt.CreateIntegrator(s).Render()
    assert np.isfinite(film).all() and film.any()
    flat = pt.Scene(text=ts.text("bindings").replace('"texture sigma" "df" "texture bumpmap" "bs"', "").replace('"texture roughness" "cf"', '"float roughness" [.2]'),
                    base_dir=images)
    assert flat.errors == []
    assert nz._rel_l2(film, pt.CreateIntegrator(flat).Render()[0]) > 1e-4


def test_such_a_scene_launches_the_general_instances(pt, images):
    s, _, integ, _, _, _ = _render_pair(pt, images, KD["dots"], nz.CONSTANT_KD, integrator=nz.PATH)
    launches, blocks = integ.shade_launch_stats()
    assert launches > 0 and blocks > 0
    plan = s.shade_plan()
    textured = [plan["classes"][c] for c in set(plan["material_class"]) if plan["classes"][c]["types"] & pt.TM_TEXTURED]
    assert textured and all(k["tm"] == pt.TM_ALL for k in textured)
