"""MIPT_TEXTURES=all in the front end: the 2-D mappings "spherical", "cylindrical" and "planar", the classes "dots", "uv",
"bilerp", the float and the 3-D "checkerboard" -- the mi_texture records they make, where they bind, what stays a reported
error and why, the shading plan and the scene cache. Without the switch every scene text here gives the messages it gave
before the switch existed (golden/texture_mapping_messages_without_switch.json, recorded from the parent commit). No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import scenes_text as st
import texture_mapping as tm
import texture_mapping_scenes as ts

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "texture_mapping_messages_without_switch.json")


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("texture_mapping"))
    st.write_texture_files(d)
    return d


@pytest.fixture
def switch(monkeypatch):
    monkeypatch.setenv("MIPT_TEXTURES", "all")


def _scene(pt, name, images):
    return pt.Scene(text=ts.text(name), base_dir=images)


def _m(rec):
    return np.array(list(rec), np.float32).reshape(4, 4)


def _ctm():
    """The CTM of texture_mapping_scenes.CTM in float64: Translate * Rotate(35, (1, 2, .5)) * Scale."""
    a = np.array([1, 2, .5]) / np.linalg.norm([1, 2, .5])
    th = np.radians(35.)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = np.eye(4)
    R[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T, S = np.eye(4), np.diag([1.5, .6, 2.5, 1.])
    T[:3, 3] = [.3, -1.2, .7]
    return T @ R @ S


def _spec(pt, rgb):
    """The constant spectrum an "rgb" parameter makes, through the product's own constant-texture path."""
    s = pt.Scene(text=ts.HEAD + 'WorldBegin\nMaterial "matte" "rgb Kd" [%g %g %g]\n' % tuple(rgb) + ts.TRI + "WorldEnd\n")
    return list(s.desc.materials[s.desc.prims[0].material].bxdf[0].R)


# -------------------------------------------------------------------------------------------------------------- layout
def test_the_python_record_has_the_library_s_size(pt):
    assert C.sizeof(pt.Texture) == pt.host_lib().mi_texture_struct_size()


def test_abi_version_is_unchanged(pt, switch, images):
    assert _scene(pt, "classes", images).desc.abi_version == 15


# ------------------------------------------------------------------------------------------------------------- records
def test_classes_make_their_records(pt, switch, images):
    s = _scene(pt, "classes", images)
    assert s.errors == [], s.errors
    t = s.desc.textures
    assert s.desc.n_textures == 7            # the float "uv" makes no texture (CreateUVFloatTexture returns nullptr) and no message
    u, d, df, b, cf, c3, c3f = (t[i] for i in range(7))
    f32 = lambda x: float(np.float32(x))
    assert (u.type, u.is_float, u.mapping, u.su, u.sv, u.du, u.dv, u.mipmap) == (tm.TEX_UV, 0, tm.MAP_UV, 2, 1, 0, .25, -1)
    assert (d.type, d.is_float, d.mapping, d.su, d.sv) == (tm.TEX_DOTS, 0, tm.MAP_UV, 6, 5)
    # the operand swap of dots.cpp:62-66 / 91-95: "inside" is the constructor's outsideDot, the value outside the dots (spec1)
    assert list(d.spec1) == _spec(pt, [.8, .1, .1]) and list(d.spec2) == _spec(pt, [.1, .2, .9])
    assert (df.type, df.is_float, df.spec1[0], df.spec2[0], df.post_scale) == (tm.TEX_DOTS, 1, f32(.7), f32(.2), 1)
    assert (b.type, b.is_float, b.du, list(b.bilerp)) == (tm.TEX_BILERP, 1, .5, [f32(.1), f32(.2), f32(.3), f32(.9)])
    assert (cf.type, cf.is_float, cf.aa_none, cf.su, cf.sv, cf.spec1[0], cf.spec2[0]) == (tm.TEX_CHECKERBOARD, 1, 1, 4, 3, f32(.4), f32(.05))
    assert (c3.type, c3.is_float, c3.mapping) == (tm.TEX_CHECKERBOARD3D, 0, tm.MAP_UV)
    assert list(c3.spec1) == _spec(pt, [.9, .9, .2]) and list(c3.spec2) == _spec(pt, [.1, .1, .1])
    assert (c3f.type, c3f.is_float, c3f.aa_none, c3f.spec1[0], c3f.spec2[0]) == (tm.TEX_CHECKERBOARD3D, 1, 0, f32(.3), f32(.6))   # ignores aamode
    # WorldToTexture of the 3-D checkerboard: the inverse of the CTM at the statement
    for rec in (c3, c3f):
        assert np.abs(_m(rec.w2t).astype(np.float64) @ _ctm() - np.eye(4)).max() < 1e-6
    m = s.desc.materials[s.desc.prims[0].material]
    assert m.textured == 1 and m.tex[0].tex_R == 1


def test_mappings_make_their_records(pt, switch, images):
    s = _scene(pt, "mappings", images)
    assert s.errors == [], s.errors
    assert s.desc.n_textures == 7
    isph, icyl, ipl, cp, dsph, ucyl, bp = (s.desc.textures[i] for i in range(7))
    f32 = lambda x: float(np.float32(x))
    assert (isph.type, isph.mapping, isph.is_float) == (tm.TEX_IMAGEMAP, tm.MAP_SPHERICAL, 0) and isph.mipmap >= 0
    assert (icyl.type, icyl.mapping, icyl.is_float) == (tm.TEX_IMAGEMAP, tm.MAP_CYLINDRICAL, 1) and icyl.mipmap >= 0
    for rec in (isph, icyl, dsph, ucyl):        # w2t is the inverse of the CTM at the statement
        assert np.abs(_m(rec.w2t).astype(np.float64) @ _ctm() - np.eye(4)).max() < 1e-6
    assert (ipl.type, ipl.mapping) == (tm.TEX_IMAGEMAP, tm.MAP_PLANAR)
    assert list(ipl.vs) == [.5, 0, .25] and list(ipl.vt) == [0, 2, 0] and (ipl.du, ipl.dv) == (f32(.1), f32(.2))
    # planar ignores the CTM: the vectors are the parameters as written, no transform is kept
    assert not np.array(list(ipl.w2t)).any() and not np.array(list(cp.w2t)).any()
    assert (cp.type, cp.mapping, list(cp.vs), list(cp.vt), cp.du, cp.dv) == (tm.TEX_CHECKERBOARD, tm.MAP_PLANAR, [1, 0, 0], [0, 1, 0], 0, 0)
    assert (dsph.type, dsph.mapping) == (tm.TEX_DOTS, tm.MAP_SPHERICAL) and (ucyl.type, ucyl.mapping) == (tm.TEX_UV, tm.MAP_CYLINDRICAL)
    assert (bp.type, bp.mapping, list(bp.bilerp)) == (tm.TEX_BILERP, tm.MAP_PLANAR, [0, 1, 0, 1])


@pytest.mark.parametrize("name", ["unknown mapping", "unknown mapping of an image"])
def test_unknown_mapping_is_the_reference_s_error_and_a_default_uv_mapping(pt, switch, images, name):
    s = _scene(pt, name, images)
    assert s.errors == ['2D texture mapping "conformal" unknown']
    t = s.desc.textures[0]
    assert s.desc.n_textures == 1 and (t.mapping, t.su, t.sv, t.du, t.dv) == (tm.MAP_UV, 1, 1, 0, 0)     # `new UVMapping2D`, uscale unread
    assert s.desc.materials[s.desc.prims[0].material].tex[0].tex_R == 0


# ------------------------------------------------------------------------------------------------------ still reported
@pytest.mark.parametrize("name, needles", [
    ("spectrum bilerp", ['spectrum "bilerp"', "sum of four spectra", "two-spectrum form"]),
    ("marble", ['"marble"', "three basis spectra plus white", "two-spectrum form"]),
    ("ptex", ['"ptex"', "Ptex library"]),
    ("dimension 4", ["4 dimensional checkerboard texture not supported"]),
    ("dots of textures", ['"dots" of image textures', "constant inside / outside"]),
    ("float checkerboard of textures", ['"checkerboard" of image textures', "constant tex1 / tex2"]),
])
def test_what_stays_an_error_carries_its_reason(pt, switch, images, name, needles):
    s = _scene(pt, name, images)
    assert len(s.errors) == 1 and all(n in s.errors[0] for n in needles), s.errors
    made = {"dots of textures": 1, "float checkerboard of textures": 1}.get(name, 0)
    assert s.desc.n_textures == made and s.desc.n_tris == 1


@pytest.mark.parametrize("name, param", [("alpha dots", "alpha"), ("shadowalpha spherical image", "shadowalpha"), ("alpha 3-D checkerboard", "alpha")])
def test_masks_are_refused(pt, switch, images, name, param):
    s = _scene(pt, name, images)
    assert len(s.errors) == 1 and ('as "%s" of a shape is outside the hot-path scope' % param) in s.errors[0] and "left unmasked" in s.errors[0], s.errors
    assert "traversal kernels" in s.errors[0]
    assert s.desc.n_meshes == 1 and s.desc.meshes[0].alpha_tex == -1 and s.desc.meshes[0].shadow_alpha_tex == -1 and s.desc.n_tris == 1


# ------------------------------------------------------------------------------------------------------------ bindings
def test_they_bind_where_image_textures_bind(pt, switch, images):
    s = _scene(pt, "bindings", images)
    assert s.errors == [], s.errors
    names = ["d", "u", "c3", "b", "bs", "cf", "df", "ic"]
    idx = {n: i for i, n in enumerate(names)}
    assert s.desc.n_textures == len(names)
    assert s.desc.textures[idx["bs"]].type == tm.TEX_BILERP and s.desc.textures[idx["bs"]].post_scale == float(np.float32(.05))
    mats = [s.desc.materials[s.desc.prims[i].material] for i in range(6)]
    matte, plastic, uber, disney, mirror, scaled = mats
    # a spectrum "scale" with a constant: the constant stays in the lobe, the texture is multiplied in (MI_LOBE_TEX_MUL_R = 1)
    assert scaled.tex[0].tex_R == idx["d"] and scaled.tex[0].flags & 1 and list(scaled.bxdf[0].R) == _spec(pt, [.5, .25, .125])
    assert all(m.textured == 1 for m in mats)
    assert (matte.tex[0].tex_R, matte.sigma_tex, matte.bump_tex) == (idx["d"], idx["df"], idx["bs"])
    assert plastic.tex[0].tex_R == idx["u"] and idx["c3"] in [plastic.tex[i].tex_R for i in range(plastic.n_bxdfs)] + [plastic.tex[i].tex_S for i in range(plastic.n_bxdfs)]
    assert plastic.rough_tex[0] == idx["cf"]
    assert list(uber.rough_tex) == [idx["cf"], idx["ic"]] and idx["d"] in [uber.tex[i].tex_R for i in range(uber.n_bxdfs)]
    assert disney.rough_tex[0] == idx["cf"] and any(disney.tex[i].tex_R == idx["c3"] for i in range(disney.n_bxdfs))
    assert idx["u"] in [mirror.tex[i].tex_R for i in range(mirror.n_bxdfs)]


# ---------------------------------------------------------------------------------------------------------------- plan
def _routes(s):
    plan = s.shade_plan()
    mats = []
    for i in range(s.desc.n_prims):
        if s.desc.prims[i].material not in mats:
            mats.append(s.desc.prims[i].material)
    return [(plan["classes"][plan["material_class"][m]]["nl"], plan["classes"][plan["material_class"][m]]["tm"]) for m in mats]


def test_textured_classes_go_to_the_general_instances(pt, switch, images):
    s = _scene(pt, "plan", images)
    assert s.errors == []
    assert _routes(s) == [(2, pt.TM_FULL), (2, pt.TM_FULL), (2, pt.TM_DIFFUSE | pt.TM_LIGHTS_NO_ENV)]
    s = _scene(pt, "bindings", images)
    plan = s.shade_plan()
    textured = [plan["classes"][c] for c in set(plan["material_class"]) if plan["classes"][c]["types"] & pt.TM_TEXTURED]
    assert textured and all(k["tm"] == pt.TM_FULL for k in textured)
    s = _scene(pt, "plan with instances", images)
    assert s.errors == [] and set(_routes(s)) == {(2, pt.TM_ALL)}
    # an image texture under another mapping is enough: the hot textured instances hold UVMapping2D alone
    s = _scene(pt, "mappings", images)
    assert _routes(s) == [(2, pt.TM_FULL)]
    assert len(pt.shade_instances()) == 21


def test_the_device_library_refuses_records_in_the_wrong_slot(pt, switch, images):
    """mi_pt_create's checks of the description (reached here through mi_pt_shade_plan, host code): a float-only record in a
    spectrum slot, a spectrum-only one as bump map, a new record as a mask, a mapping out of range."""
    def broken(change, needle):
        s = _scene(pt, "bindings", images)
        s.shade_plan()
        change(s.desc)
        with pytest.raises(RuntimeError, match=needle):
            s.shade_plan()
    def kd_bilerp(d): d.materials[d.prims[0].material].tex[0].tex_R = 3
    def bump_uv(d): d.materials[d.prims[0].material].bump_tex = 1
    def rough_uv(d): d.materials[d.prims[1].material].rough_tex[0] = 1
    def mask_dots(d): d.meshes[0].alpha_tex = 6
    def mask_mapped_image(d): d.meshes[0].shadow_alpha_tex = 7
    def bad_mapping(d): d.textures[0].mapping = 4
    def mapping_on_3d(d): d.textures[2].mapping = 1
    for change, needle in ((kd_bilerp, "MI_TEX_BILERP"), (bump_uv, "MI_TEX_UV"), (rough_uv, "rough_tex"), (mask_dots, "alpha textures must be image textures"),
                           (mask_mapped_image, "under the uv mapping"), (bad_mapping, "not a mi_tex_mapping"), (mapping_on_3d, "without a 2-D mapping")):
        broken(change, needle)


# ---------------------------------------------------------------------------------------------------------------- cache
@pytest.mark.parametrize("name", ["classes", "mappings", "bindings"])
def test_scene_cache_round_trip(pt, switch, images, tmp_path, name):
    s = _scene(pt, name, images)
    path = os.path.join(str(tmp_path), "textures.cache")
    s.save_cache(path)
    r = pt.Scene(cache=path)
    assert r.desc.n_textures == s.desc.n_textures > 0 and list(r.errors) == list(s.errors)
    for i in range(s.desc.n_textures):
        assert bytes(r.desc.textures[i]) == bytes(s.desc.textures[i])
    assert bytes(r.desc.materials[0]) == bytes(s.desc.materials[0])


def test_scene_cache_of_another_record_size_is_rejected(pt, switch, images, tmp_path):
    """mi_texture grew under an unchanged ABI number, cache magic and cache header (existing tests pin all three), so a cache
    ends with sizeof(mi_texture): a file that names another size there is refused, and so is a file without that word, which
    is how a file of the build before ends."""
    import struct
    for name in ("classes", "plan"):
        s = _scene(pt, name, images)
        path = os.path.join(str(tmp_path), "t.cache")
        s.save_cache(path)
        raw = bytearray(open(path, "rb").read())
        size = C.sizeof(pt.Texture)
        assert struct.unpack_from("<I", raw, len(raw) - 4)[0] == size
        for stale in (raw[:-4] + struct.pack("<I", size - 48), raw[:-4]):
            with open(path, "wb") as f:
                f.write(bytes(stale))
            with pytest.raises(RuntimeError, match="not a scene cache of this build"):
                pt.Scene(cache=path)
        with open(path, "wb") as f:
            f.write(bytes(raw))
        assert pt.Scene(cache=path).desc.n_textures == s.desc.n_textures


# -------------------------------------------------------------------------------------------------- without the switch
@pytest.mark.parametrize("name", sorted(ts.FRONTEND))
@pytest.mark.parametrize("env", [None, "", "1", "ALL"], ids=["unset", "empty", "1", "ALL"])
def test_without_the_switch_the_messages_are_the_parent_s(pt, monkeypatch, images, name, env):
    if env is None:
        monkeypatch.delenv("MIPT_TEXTURES", raising=False)
    else:
        monkeypatch.setenv("MIPT_TEXTURES", env)        # only the exact value "all" turns the feature on
    with open(GOLDEN) as fh:
        want = json.load(fh)[name]
    s = _scene(pt, name, images)
    assert list(s.errors) == want["errors"] and list(s.warnings) == want["warnings"] and s.desc.n_textures == want["n_textures"]
    for i in range(s.desc.n_textures):
        t = s.desc.textures[i]
        assert t.mapping == 0 and not any(t.vs) and not any(t.vt) and not any(t.bilerp)
