"""texture_mapping.py, the numpy restatement of the 2-D mappings and the classes "dots", "uv", "bilerp" and "checkerboard", held
to facts that need no renderer; and the cap on unjudged queries: over every capped group of the GPU tests' query sets the
float32 and float64 restatements disagree on a discrete decision (checkerboard parity, the dot's cell, Noise > 0, inside the
radius, the side of the phi seam and the wrap of a differential) in at most 2 % of the queries. No GPU."""
import numpy as np
import pytest

import texture_mapping as tm
import texture_mapping_cases as tc


class Rec:
    """A bare mi_texture stand-in."""

    def __init__(self, **kw):
        self.type, self.mapping, self.aa_none, self.is_float = tm.TEX_UV, tm.MAP_UV, 0, 0
        self.su = self.sv = self.post_scale = 1.
        self.du = self.dv = 0.
        self.vs, self.vt, self.bilerp = [1, 0, 0], [0, 1, 0], [0, 1, 0, 1]
        self.spec1, self.spec2 = [0.] * 31, [1.] * 31
        self.w2t = list(np.eye(4).reshape(-1))
        self.__dict__.update(kw)


PRECISIONS = [np.float32, np.float64]


@pytest.mark.parametrize("f", PRECISIONS)
def test_spherical_st_of_the_six_axis_points(f):
    t = tm.Tex(Rec(mapping=tm.MAP_SPHERICAL), f)
    p = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f) * f(2.5)
    st, _ = tm.sphere(t, p)
    want = np.array([[.5, 0], [.5, .5], [.5, .25], [.5, .75], [0, 0], [1, 0]])      # (theta / pi, phi / 2 pi)
    assert np.abs(st - want).max() <= 4 * np.finfo(np.float32).eps


@pytest.mark.parametrize("f", PRECISIONS)
def test_cylindrical_st_of_the_axis_points(f):
    t = tm.Tex(Rec(mapping=tm.MAP_CYLINDRICAL), f)
    p = np.array([[1, 0, 0], [0, 1, 0], [0, -1, 0], [3, 0, 4]], f)
    st, _ = tm.cylinder(t, p)
    assert np.abs(st - np.array([[.5, 0], [.75, 0], [.25, 0], [.5, .8]])).max() <= 4 * np.finfo(np.float32).eps


@pytest.mark.parametrize("f", PRECISIONS)
def test_planar_with_default_vectors_is_the_uv_mapping_on_a_quad_whose_uv_is_its_xy(f):
    rng = np.random.default_rng(1)
    n = 200
    xy = rng.uniform(-2, 2, (n, 2)).astype(np.float32)
    p = np.concatenate([xy, rng.uniform(-1, 1, (n, 1)).astype(np.float32)], axis=1)       # z does not matter
    dpdx, dpdy = rng.normal(size=(n, 3)).astype(np.float32) * 1e-2, rng.normal(size=(n, 3)).astype(np.float32) * 1e-2
    duv = np.concatenate([dpdx[:, 0:2], dpdy[:, 0:2]], axis=1)                            # (dudx, dvdx, dudy, dvdy) = d(xy)
    planar, _ = tm.map2d(tm.Tex(Rec(mapping=tm.MAP_PLANAR), f), p, dpdx, dpdy, xy * 0, duv * 0)
    uv, _ = tm.map2d(tm.Tex(Rec(), f), p * 0, dpdx * 0, dpdy * 0, xy, duv)
    assert np.array_equal(planar, uv)


@pytest.mark.parametrize("f", PRECISIONS)
@pytest.mark.parametrize("mapping, x", [(tm.MAP_SPHERICAL, 2.), (tm.MAP_CYLINDRICAL, -2.)])
def test_a_footprint_across_the_phi_seam_gives_the_wrapped_differential(f, mapping, x):
    """The raw forward difference of a coordinate that jumps by 1 across the seam is about -+1 / delta; the reference folds a
    component [1] above .5 to 1 - d and one below -.5 to -(d + 1) (texture.cpp:111-119). For the spherical mapping [1] is phi, so
    the fold acts on the jump; for the cylindrical one [1] is z of the normalised vector and the jump sits in [0], which is never folded -- restated as written."""
    t = tm.Tex(Rec(mapping=mapping), f)
    delta = np.float64(np.float32(.1 if mapping == tm.MAP_SPHERICAL else .01))
    p = np.array([[x, -.01 * np.sign(x), .3]], f)        # just below the seam, phi near 2 pi (s near 1 for the cylinder)
    step = np.array([[0, .05 * np.sign(x) / delta, 0]], f)      # p + delta * step lies at +-.04: across
    out, dec = tm.map2d(t, p, step, -step, np.zeros((1, 2)), np.zeros((1, 4)))
    fn = tm.sphere if mapping == tm.MAP_SPHERICAL else tm.cylinder
    st0, st1 = fn(t, p)[0].astype(np.float64), fn(t, p + f(delta) * step)[0].astype(np.float64)
    raw = (st1 - st0) / delta
    if mapping == tm.MAP_SPHERICAL:
        assert raw[0, 1] < -.5 and dec[0, 0] != dec[0, 1]             # phi fell by almost 2 pi: the raw difference is about -1 / delta
        assert abs(out[0, 3] - (-(raw[0, 1] + 1))) < 1e-4 and dec[0, 3] == -1
        assert abs(out[0, 2] - raw[0, 0]) < 1e-4                        # [0] is left alone
    else:
        assert abs(raw[0, 0]) > .5 and abs(out[0, 2] - raw[0, 0]) < 1e-3      # the jump sits in [0], which is never folded
        assert dec[0, 3] == 0 and abs(out[0, 3] - raw[0, 1]) < 1e-4 and abs(raw[0, 1]) < .5      # the normalised z hardly moves


@pytest.mark.parametrize("f", PRECISIONS)
def test_the_wrap_branches(f):
    d = np.array([.5, .6, -.5, -.6, 3, -3, 0], f)
    v, branch = tm._wrap(d)
    assert list(branch) == [0, 1, 0, -1, 1, -1, 0]
    assert np.allclose(v, [.5, .4, -.5, -.4, -2, 2, 0], atol=1e-6)


@pytest.mark.parametrize("f", PRECISIONS)
def test_every_dot_centre_lies_within_015_of_its_cell_centre(f):
    rng = np.random.default_rng(2)
    st = rng.uniform(-40, 40, (4000, 2)).astype(f)
    inside, centre, dec = tm.dots(st)
    cell = dec[:, 0:2].astype(np.float64)
    assert np.abs(centre - cell).max() <= .15 + 1e-6          # maxShift * |Noise| with |Noise| <= 1
    assert np.abs(centre - cell).max() > .05                   # and the shift is there
    assert .1 < dec[:, 2].mean() < .9 and 0 < inside.mean() < dec[:, 2].mean()
    assert np.abs(st - cell).max() <= .5 + 1e-6               # the cell is the nearest integer point
    r2 = ((st - centre) ** 2).sum(axis=1)
    assert (r2[inside] < .35 ** 2 + 1e-6).all()


@pytest.mark.parametrize("f", PRECISIONS)
def test_uv_texture_rgb_lies_in_0_1(f):
    rng = np.random.default_rng(3)
    n = 2000
    uv = np.concatenate([rng.uniform(-50, 50, (n - 6, 2)), [[0, 0], [1, -1], [-1e-9, 1e-9], [2, 3], [-.5, .5], [7.999999, -7.999999]]]).astype(np.float32)
    rec = Rec(su=3., sv=-2., du=.1, dv=.7)
    c, _ = tm.map2d(tm.Tex(rec, f), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), uv, np.zeros((n, 4)))
    rgb = np.stack([c[:, 0] - np.floor(c[:, 0]), c[:, 1] - np.floor(c[:, 1])], axis=1)
    assert (rgb >= 0).all() and (rgb < 1).all() if f == np.float64 else (rgb >= 0).all() and (rgb <= 1).all()
    basis = np.random.default_rng(4).uniform(0, 1, (7, 31))
    q = np.concatenate([np.zeros((n, 9)), uv, np.zeros((n, 4))], axis=1)
    v, _ = tm.evaluate(tm.Tex(rec, f), q, basis)
    assert v.shape == (n, 31) and (v >= 0).all() and np.isfinite(v).all()
    # FromRGB of (r, g, 0): blue is the least, so white gets 0 and the value is yellow * min(r, g) + red or green * the rest
    k = 5
    r, g = rgb[k].astype(np.float64)
    B = basis.astype(np.float32).astype(np.float64)
    want = (B[3] * min(r, g) + (B[4] * (r - g) if r > g else B[5] * (g - r))) * np.float64(np.float32(.86445))
    assert np.abs(v[k] - want).max() < 1e-5


def test_checkerboards():
    for f in PRECISIONS:
        c = np.array([[.5, .5, 0, 0, 0, 0], [1.5, .5, 0, 0, 0, 0], [-.5, .5, 0, 0, 0, 0], [1., .5, .25, .1, 0, 0], [.3, .3, 5, .1, 0, 0]], f)
        w, _ = tm.checkerboard2d(c, False)
        assert list(w[:3]) == [0, 1, 1] and abs(w[3] - .5) < 1e-6 and w[4] == .5
        w, _ = tm.checkerboard2d(c, True)
        assert list(w) == [0, 1, 1, 1, 0]
        t = tm.Tex(Rec(type=tm.TEX_CHECKERBOARD3D), f)
        assert list(tm.checkerboard3d(t, np.array([[.5, .5, .5], [1.5, .5, .5], [-.5, .5, .5], [1.5, 1.5, .5], [-.5, -.5, -.5]]))) == [False, True, True, False, True]


# ---------------------------------------------------------------------------------------------------------------- the cap
@pytest.fixture(scope="module")
def probe_scene(pt, tmp_path_factory):
    import os
    import scenes_text as st
    d = str(tmp_path_factory.mktemp("texture_mapping_cases"))
    st.write_texture_files(d)
    tc.write_grey_image(d)
    old = os.environ.get("MIPT_TEXTURES")
    os.environ["MIPT_TEXTURES"] = "all"
    try:
        text, index = tc.scene_text()
        s = pt.Scene(text=text, base_dir=d)
    finally:
        if old is None:
            del os.environ["MIPT_TEXTURES"]
        else:
            os.environ["MIPT_TEXTURES"] = old
    assert s.errors == [], s.errors
    return s, index


@pytest.mark.parametrize("i", range(len(tc.CASES)), ids=[c[0] for c in tc.CASES])
def test_the_precisions_disagree_on_at_most_2_percent_of_a_group(probe_scene, i):
    s, index = probe_scene
    rec = s.desc.textures[index[i]]
    basis = np.array([list(row) for row in s.desc.rgb_illum], np.float32)
    image = i >= len(tc.CASES) - tc.IMAGE_CASES
    for name, q in tc.groups().items():
        for mode in ([0] if image else [0, 1]):
            if mode == 0 and rec.type == tm.TEX_CHECKERBOARD3D:
                continue
            v32, v64, judged = tc.restate(rec, q, basis, mode)
            assert np.isfinite(v32).all() and np.isfinite(v64).all()
            share = 1 - judged.mean()
            print("%-34s %-42s mode %d  unjudged %5.2f %%" % (tc.CASES[i][0], name, mode, 100 * share))
            if name != tc.NEAR:
                assert share <= .02, (name, mode, share)
