"""Texture "fbm" / "wrinkled" / "windy" in the front end: the permutation table, the mi_texture record, where a noise texture
binds, what stays a reported error, the shading plan and the scene cache; and the numpy restatement's own sanity. No GPU."""
import os

import numpy as np
import pytest

import noise_texture as nt
import scenes_text as st

HEAD = ('LookAt 0 0 8  0 0 0  0 1 0\nCamera "perspective" "float fov" [40]\n'
        'Film "image" "integer xresolution" [8] "integer yresolution" [8]\n')
TRI = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-3 -3 -1  3 -3 -1  0 3 -1]\n'
LIGHT = 'LightSource "point" "point from" [0 4 4]\n'
NO_LIGHT = 'No light sources defined in scene; rendering a black image.'
CLASSES = {"fbm": nt.TEX_FBM, "wrinkled": nt.TEX_WRINKLED, "windy": nt.TEX_WINDY}


def _scene(pt, body, head=HEAD, base_dir=None):
    return pt.Scene(text=head + "WorldBegin\n" + body + "WorldEnd\n", base_dir=base_dir)


def _mat(s, prim=0):
    return s.desc.materials[s.desc.prims[prim].material]


def _m(rec):
    return np.array(list(rec), np.float32).reshape(4, 4)


# ---------------------------------------------------------------------------------------------------------------- table
def test_permutation_table_is_the_fixture(pt):
    p = pt.noise_perm()
    assert p.shape == (512,) and p.dtype == np.int32
    assert np.array_equal(p, nt.perm())
    assert np.array_equal(p[:256], p[256:])
    assert np.array_equal(np.sort(p[:256]), np.arange(256))


# ---------------------------------------------------------------------------------------------------- restatement sanity
@pytest.mark.parametrize("f", [np.float32, np.float64])
def test_noise_is_zero_on_the_lattice(f):
    pts = np.array([[0, 0, 0], [1, 2, 3], [-1, -2, -3], [-255, 256, 257], [300, -700, 1024], [255, 255, 255], [-256, 511, 70000]], f)
    assert np.array_equal(nt.noise(pts[:, 0], pts[:, 1], pts[:, 2]), np.zeros(len(pts), f))


def test_noise_has_period_256_in_float64():
    rng = np.random.default_rng(3)
    p = rng.uniform(-4, 4, (500, 3))
    p = np.round(p * 1024) / 1024          # (so that x + 256 is exact)
    a = nt.noise(p[:, 0], p[:, 1], p[:, 2])
    assert np.abs(a).max() > .5
    for shift in ([256, 0, 0], [0, -256, 0], [512, 256, -768]):
        q = p + np.array(shift, np.float64)
        assert np.array_equal(nt.noise(q[:, 0], q[:, 1], q[:, 2]), a)


@pytest.mark.parametrize("f", [np.float32, np.float64])
def test_zero_octaves_keep_the_partial_term_only(f):
    rng = np.random.default_rng(4)
    p = rng.uniform(-30, 30, (200, 3)).astype(f)
    d = (rng.normal(size=(200, 3)) * 1e-3).astype(f)
    zero = np.zeros_like(d)
    for dx, dy in ((d, d), (zero, zero), (1e4 * d, d)):
        assert np.array_equal(nt.fbm(p, dx, dy, f(.5), 0), np.zeros(200, f))
        assert np.array_equal(nt.turbulence(p, dx, dy, f(.5), 0), np.full(200, f(0.2), f))


def test_float32_restatement_follows_the_float64_one():
    """The figures of the prototype: 20 000 queries, |p| <= 300, footprints 1e-6 .. 10."""
    rng = np.random.default_rng(1)
    n = 20000
    p = rng.uniform(-300, 300, (n, 3))
    fp = 10 ** rng.uniform(-6, 1, (n, 1))
    dx, dy = rng.normal(size=(n, 3)) * fp, rng.normal(size=(n, 3)) * fp
    a32 = [a.astype(np.float32) for a in (p, dx, dy)]
    a64 = [a.astype(np.float64) for a in a32]
    d = np.abs(nt.fbm(*a32, np.float32(.5), 8) - nt.fbm(*a64, .5, 8))
    assert d.max() < 1e-3 and np.median(d) < 5e-5
    d1 = np.abs(nt.fbm(*a32, np.float32(1), 8) - nt.fbm(*a64, 1., 8))
    assert d1.max() < 5e-2
    assert np.array_equal(nt.fbm(*a32, np.float32(.5), 0), nt.fbm(*a64, .5, 0).astype(np.float32))


# -------------------------------------------------------------------------------------------------------------- parsing
@pytest.mark.parametrize("cls", ["fbm", "wrinkled", "windy"])
@pytest.mark.parametrize("typ", ["float", "spectrum", "color"])
def test_each_class_and_type_with_defaults(pt, cls, typ):
    s = _scene(pt, 'Texture "n" "%s" "%s"\n' % (typ, cls) + TRI)
    assert s.errors == [] and s.warnings == [NO_LIGHT]
    assert s.desc.n_textures == 1 and s.desc.n_mipmaps == 0
    t = s.desc.textures[0]
    assert t.type == CLASSES[cls] and t.mipmap == -1
    assert (t.octaves, t.omega, t.post_scale) == (8, .5, 1.)
    assert np.array_equal(_m(t.w2t), np.eye(4, dtype=np.float32))


def test_parameters_and_the_inverse_of_the_ctm(pt):
    s = _scene(pt, 'AttributeBegin\nTranslate .5 -1 2\nRotate 35 1 2 .5\nScale 1 2 .5\n'
                   'Texture "a" "float" "fbm" "integer octaves" [3] "float roughness" [.7]\n'
                   'Texture "b" "spectrum" "wrinkled" "integer octaves" [0] "float roughness" [1]\n'
                   'CoordinateSystem "here"\nAttributeEnd\n'
                   'Texture "c" "float" "windy" "integer octaves" [3] "float roughness" [.7]\n' + TRI)
    assert s.errors == []
    assert s.warnings == ['Parameter "octaves" not used', 'Parameter "roughness" not used', NO_LIGHT]   # windy reads neither
    a, b, c = (s.desc.textures[i] for i in range(3))
    assert (a.type, a.octaves, a.omega) == (nt.TEX_FBM, 3, float(np.float32(.7)))
    assert (b.type, b.octaves, b.omega) == (nt.TEX_WRINKLED, 0, 1.)
    assert (c.type, c.octaves, c.omega) == (nt.TEX_WINDY, 8, .5) and np.array_equal(_m(c.w2t), np.eye(4, dtype=np.float32))
    assert np.array_equal(_m(a.w2t), _m(b.w2t))
    # tex2world in float64 from the directives; w2t is its inverse
    th = np.radians(35.)
    ax = np.array([1, 2, .5]) / np.linalg.norm([1, 2, .5])
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(4)
    R[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T = np.eye(4)
    T[:3, 3] = [.5, -1, 2]
    t2w = T @ R @ np.diag([1, 2, .5, 1])
    assert np.allclose(_m(a.w2t).astype(np.float64) @ t2w, np.eye(4), atol=2e-6)


def test_unused_parameter_warning(pt):
    s = _scene(pt, 'Texture "a" "float" "fbm" "float scale" [2] "integer octaves" [4]\n' + TRI)
    assert s.errors == [] and s.warnings == ['Parameter "scale" not used', NO_LIGHT]
    assert s.desc.textures[0].octaves == 4


def test_octaves_are_clamped_to_32_and_negative_ones_refused(pt):
    s = _scene(pt, 'Texture "a" "float" "fbm" "integer octaves" [40]\nTexture "b" "spectrum" "wrinkled" "integer octaves" [32]\n' + TRI)
    assert s.errors == []
    assert s.warnings == ['Texture "a": "octaves" 40 clamped to 32 on this path', NO_LIGHT]
    assert s.desc.textures[0].octaves == 32 and s.desc.textures[1].octaves == 32
    s = _scene(pt, 'Texture "a" "float" "wrinkled" "integer octaves" [-1]\nMaterial "matte" "texture sigma" "a"\n' + TRI)
    assert len(s.errors) == 2 and '"octaves" -1' in s.errors[0] and "Couldn't find float texture" in s.errors[1]
    assert s.desc.n_textures == 0


# -------------------------------------------------------------------------------------------------------------- binding
def test_matte_kd(pt):
    s = _scene(pt, 'Texture "n" "spectrum" "fbm"\nMaterial "matte" "texture Kd" "n"\n' + TRI)
    assert s.errors == []
    m = _mat(s)
    assert m.textured == 1 and m.tex[0].tex_R == 0 and m.tex[0].tex_S == -1
    assert m.bump_tex == -1 and list(m.rough_tex) == [-1, -1] and m.sigma_tex == -1


def test_plastic_kd_and_roughness(pt):
    s = _scene(pt, 'Texture "n" "spectrum" "windy"\nTexture "r" "float" "wrinkled" "integer octaves" [2]\n'
                   'Material "plastic" "texture Kd" "n" "texture roughness" "r"\n' + TRI)
    assert s.errors == []
    m = _mat(s)
    assert m.textured == 1 and m.tex[0].tex_R == 0 and list(m.rough_tex) == [1, 1] and m.bump_tex == -1 and m.sigma_tex == -1
    assert s.desc.textures[1].type == nt.TEX_WRINKLED and s.desc.textures[1].octaves == 2


def test_bumpmap_through_scale(pt):
    s = _scene(pt, 'Texture "w" "float" "wrinkled"\nTexture "b" "float" "scale" "texture tex1" "w" "float tex2" [.05]\n'
                   'Material "matte" "texture bumpmap" "b"\n' + TRI)
    assert s.errors == []
    m = _mat(s)
    assert m.textured == 1 and m.bump_tex == 1 and m.tex[0].tex_R == -1 and m.sigma_tex == -1
    b = s.desc.textures[1]
    assert b.type == nt.TEX_WRINKLED and b.post_scale == float(np.float32(.05)) and b.mipmap == -1 and b.octaves == 8
    assert s.desc.textures[0].post_scale == 1.


def test_spectrum_scale_with_a_constant(pt):
    s = _scene(pt, 'Texture "n" "spectrum" "fbm"\nTexture "k" "spectrum" "scale" "texture tex1" "n" "rgb tex2" [.5 .5 .5]\n'
                   'Material "matte" "texture Kd" "k"\n' + TRI)
    assert s.errors == []
    m = _mat(s)
    assert m.textured == 1 and m.tex[0].tex_R == 0 and (m.tex[0].flags & 1) == 1      # MI_LOBE_TEX_MUL_R


def test_matte_sigma(pt):
    s = _scene(pt, 'Texture "g" "float" "fbm"\nMaterial "matte" "texture sigma" "g"\n' + TRI)
    assert s.errors == []
    m = _mat(s)
    assert m.textured == 1 and m.sigma_tex == 0 and m.tex[0].tex_R == -1 and m.bump_tex == -1 and list(m.rough_tex) == [-1, -1]


def test_disney_color_and_roughness(pt):
    s = _scene(pt, 'Texture "n" "spectrum" "wrinkled"\nTexture "r" "float" "windy"\n'
                   'Material "disney" "texture color" "n" "texture roughness" "r"\n' + TRI)
    assert s.errors == []
    m = _mat(s)
    assert m.textured == 1 and m.rough_tex[0] == 1 and m.bump_tex == -1 and m.sigma_tex == -1
    assert any(m.tex[i].tex_R == 0 for i in range(m.n_bxdfs))


# ------------------------------------------------------------------------------------------------------- still reported
@pytest.mark.parametrize("param", ["alpha", "shadowalpha"])
def test_noise_as_a_mask_is_reported(pt, param):
    s = _scene(pt, 'Texture "w" "float" "fbm"\n' + TRI.rstrip("\n") + ' "texture %s" "w"\n' % param)
    assert len(s.errors) == 1 and "Noise texture \"w\"" in s.errors[0] and param in s.errors[0]
    assert s.desc.n_meshes == 1 and s.desc.meshes[0].alpha_tex == -1 and s.desc.meshes[0].shadow_alpha_tex == -1
    assert s.desc.n_tris == 1


@pytest.mark.parametrize("body, needle", [
    ('Texture "n" "spectrum" "fbm"\nTexture "c" "spectrum" "checkerboard" "texture tex1" "n"\n', "\"checkerboard\" of image textures"),
    ('Texture "n" "spectrum" "fbm"\nTexture "c" "spectrum" "mix" "texture tex1" "n"\n', "Image texture \"n\" on parameter \"tex1\""),
    ('Texture "n" "float" "fbm"\nTexture "c" "float" "mix" "texture tex2" "n"\n', "Float image texture \"n\" on parameter \"tex2\""),
    ('Texture "n" "float" "fbm"\nTexture "o" "float" "windy"\nTexture "c" "float" "scale" "texture tex1" "n" "texture tex2" "o"\n', "\"scale\" of two image textures"),
    ('Texture "n" "spectrum" "fbm"\nTexture "o" "spectrum" "windy"\nTexture "c" "spectrum" "scale" "texture tex1" "n" "texture tex2" "o"\n',
     "\"scale\" of two image textures"),
])
def test_noise_inside_another_texture_is_reported(pt, body, needle):
    s = _scene(pt, body + TRI)
    assert len(s.errors) == 1 and needle in s.errors[0], s.errors
    assert s.desc.n_tris == 1


@pytest.mark.parametrize("cls", ["marble", "dots", "bilerp", "uv", "ptex"])
def test_other_classes_stay_reported(pt, cls):
    s = _scene(pt, 'Texture "x" "spectrum" "%s"\n' % cls + TRI)
    assert len(s.errors) == 1 and ('Texture class "%s" is outside the hot-path scope' % cls) in s.errors[0]
    assert all('"%s"' % k in s.errors[0] for k in ("fbm", "wrinkled", "windy", "imagemap", "checkerboard"))
    assert s.desc.n_textures == 0 and s.desc.n_tris == 1


# ----------------------------------------------------------------------------------------------------------------- plan
PLAN_BODY = LIGHT + '%s\nMaterial "matte" "texture Kd" "n"\n' + TRI + 'Material "plastic" "texture Kd" "n"\n' + TRI + 'Material "matte"\n' + TRI


def _routes(pt, s):
    plan = s.shade_plan()
    mats = []
    for i in range(s.desc.n_prims):          # the materials in the order the shapes name them
        if s.desc.prims[i].material not in mats:
            mats.append(s.desc.prims[i].material)
    classes = [plan["material_class"][m] for m in mats]
    return [(plan["classes"][c]["nl"], plan["classes"][c]["tm"]) for c in classes]


def test_textured_classes_of_a_noise_scene_go_to_the_general_instances(pt, tmp_path):
    st.write_texture_files(str(tmp_path))
    hot = pt.TM_LIGHTS_ALL | pt.TM_SAMPLERS
    img = _scene(pt, PLAN_BODY % 'Texture "n" "spectrum" "imagemap" "string filename" "tex_c.pfm"', base_dir=str(tmp_path))
    assert img.errors == []
    assert _routes(pt, img) == [(2, pt.TM_DIFFUSE | pt.TM_TEXTURED | hot), (2, pt.TM_PLASTIC | pt.TM_TEXTURED | hot), (2, pt.TM_DIFFUSE | pt.TM_LIGHTS_NO_ENV)]
    for cls in CLASSES:
        noise = _scene(pt, PLAN_BODY % ('Texture "n" "spectrum" "%s"' % cls))
        assert noise.errors == []
        assert _routes(pt, noise) == [(2, pt.TM_FULL), (2, pt.TM_FULL), (2, pt.TM_DIFFUSE | pt.TM_LIGHTS_NO_ENV)]
    # one noise texture anywhere in the scene: the image-textured classes move too (the hot textured instances hold no noise code)
    both = _scene(pt, (PLAN_BODY % 'Texture "n" "spectrum" "imagemap" "string filename" "tex_c.pfm"') +
                  'Texture "g" "float" "fbm"\nMaterial "matte" "texture sigma" "g"\n' + TRI, base_dir=str(tmp_path))
    assert both.errors == []
    assert _routes(pt, both) == [(2, pt.TM_FULL), (2, pt.TM_FULL), (2, pt.TM_DIFFUSE | pt.TM_LIGHTS_NO_ENV), (2, pt.TM_FULL)]
    # with object instances the plan is the parent's: everything on TM_ALL already
    inst = _scene(pt, (PLAN_BODY % 'Texture "n" "spectrum" "fbm"') + 'ObjectBegin "o"\n' + TRI + 'ObjectEnd\nObjectInstance "o"\n')
    assert set(_routes(pt, inst)) == {(2, pt.TM_ALL)}


def test_no_instance_was_added(pt):
    assert len(pt.shade_instances()) == 21


# ---------------------------------------------------------------------------------------------------------------- cache
def test_scene_cache_keeps_the_texture_records(pt, tmp_path):
    s = _scene(pt, 'Translate 1 2 3\nScale 2 2 .5\nTexture "n" "spectrum" "fbm" "integer octaves" [5] "float roughness" [.3]\n'
                   'Texture "w" "float" "wrinkled"\nTexture "b" "float" "scale" "texture tex1" "w" "float tex2" [.05]\n'
                   'Material "matte" "texture Kd" "n" "texture bumpmap" "b"\n' + TRI)
    assert s.errors == []
    path = os.path.join(str(tmp_path), "noise.cache")
    s.save_cache(path)
    r = pt.Scene(cache=path)
    assert r.desc.n_textures == s.desc.n_textures == 3
    for i in range(3):
        assert bytes(r.desc.textures[i]) == bytes(s.desc.textures[i])
    assert r.desc.textures[0].octaves == 5 and r.desc.textures[2].post_scale == float(np.float32(.05))
    assert _mat(r).bump_tex == 2 and _mat(r).tex[0].tex_R == 0
