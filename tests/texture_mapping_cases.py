"""The probe scene and the query sets of the texture-mapping tests: every case is one texture of one scene, every group one
[n, 15] float32 array of interactions (p, dpdx, dpdy, u, v, dudx, dvdx, dudy, dvdy). test_texture_mapping_restatement.py checks
on the CPU that the two precisions of the restatement disagree on a discrete decision in at most 2 % of each capped group;
test_texture_mapping_gpu.py holds the device to the restatement over the same queries."""
import numpy as np

import texture_mapping as tm
import texture_mapping_scenes as ts

IMAGE_CASES = 3     # the last cases are image textures (mode 0 against the restatement, mode 1 against texture_lookup)
# (name, declaration, under the CTM)
CASES = [
    ("uv, uv mapping", 'Texture "%s" "spectrum" "uv" "float uscale" [2] "float vscale" [3] "float udelta" [.25] "float vdelta" [-.5]', False),
    ("uv, spherical", 'Texture "%s" "spectrum" "uv" "string mapping" "spherical"', False),
    ("uv, spherical, CTM", 'Texture "%s" "spectrum" "uv" "string mapping" "spherical"', True),
    ("uv, cylindrical", 'Texture "%s" "spectrum" "uv" "string mapping" "cylindrical"', False),
    ("uv, cylindrical, CTM", 'Texture "%s" "spectrum" "uv" "string mapping" "cylindrical"', True),
    ("uv, planar", 'Texture "%s" "spectrum" "uv" "string mapping" "planar" "float udelta" [.25]', False),
    ("uv, planar v1 v2, CTM", 'Texture "%s" "spectrum" "uv" "string mapping" "planar" "vector v1" [.5 0 .25] "vector v2" [0 2 -1] "float udelta" [.1] "float vdelta" [.2]', True),
    ("dots, uv mapping", 'Texture "%s" "spectrum" "dots" "float uscale" [6] "float vscale" [5] "rgb inside" [.8 .1 .1] "rgb outside" [.1 .2 .9]', False),
    ("float dots, planar", 'Texture "%s" "float" "dots" "string mapping" "planar" "float inside" [.7] "float outside" [.2]', False),
    ("dots, spherical, CTM", 'Texture "%s" "spectrum" "dots" "string mapping" "spherical"', True),
    ("bilerp, uv mapping", 'Texture "%s" "float" "bilerp" "float v00" [.1] "float v01" [.2] "float v10" [.3] "float v11" [.9]', False),
    ("bilerp, cylindrical", 'Texture "%s" "float" "bilerp" "string mapping" "cylindrical" "float v00" [1] "float v01" [0] "float v10" [.5] "float v11" [2]', False),
    ("float checkerboard", 'Texture "%s" "float" "checkerboard" "float uscale" [4] "float vscale" [3] "float tex1" [.4] "float tex2" [.05]', False),
    ("float checkerboard, aamode none", 'Texture "%s" "float" "checkerboard" "float uscale" [4] "float vscale" [3] "float tex1" [.4] "float tex2" [.05] "string aamode" "none"', False),
    ("checkerboard, planar", 'Texture "%s" "spectrum" "checkerboard" "string mapping" "planar" "rgb tex1" [.9 .9 .9] "rgb tex2" [.2 .1 .3]', False),
    ("checkerboard, spherical, CTM", 'Texture "%s" "spectrum" "checkerboard" "string mapping" "spherical" "float uscale" [8]', True),
    ("3-D checkerboard", 'Texture "%s" "spectrum" "checkerboard" "integer dimension" [3] "rgb tex1" [.9 .9 .2] "rgb tex2" [.1 .1 .1]', False),
    ("float 3-D checkerboard, CTM", 'Texture "%s" "float" "checkerboard" "integer dimension" [3] "float tex1" [.3] "float tex2" [.6]', True),
    ("scaled float dots", 'Texture "%s_" "float" "dots" "float uscale" [3]\nTexture "%s" "float" "scale" "texture tex1" "%s_" "float tex2" [.25]', False),
    ("grey image, spherical, CTM", 'Texture "%s" "spectrum" "imagemap" "string filename" "grey.pfm" "string mapping" "spherical"', True),
    ("grey image, planar, trilinear", 'Texture "%s" "spectrum" "imagemap" "string filename" "grey.pfm" "string mapping" "planar" "bool trilinear" "true" "vector v1" [.2 0 0] "vector v2" [0 .3 .1]', False),
    ("float image, cylindrical", 'Texture "%s" "float" "imagemap" "string filename" "rough.pfm" "string mapping" "cylindrical"', False),
]
NEAR = "decisions within 2^-20 of their boundary"       # the group outside the cap


def write_grey_image(base_dir, uniform=None):
    """A non-power-of-two grey PFM (r = g = b): an image texture's value is then linear in the texel. uniform: every texel that value."""
    import os
    rng = np.random.default_rng(5)
    g = rng.uniform(.05, .95, (10, 12)).astype(np.float32) if uniform is None else np.full((8, 8), uniform, np.float32)   # (8 x 8: never resampled)
    with open(os.path.join(base_dir, "grey.pfm"), "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (g.shape[1], g.shape[0]))
        f.write(np.repeat(g[:, :, None], 3, axis=2).tobytes())


def scene_text():
    body, index, n = "", [], 0
    for i, (_, decl, ctm) in enumerate(CASES):
        name = "t%d" % i
        line = (decl % ((name,) * decl.count("%s"))) + "\n"
        n += line.count("Texture ")
        index.append(n - 1)
        body += "TransformBegin\n%s%sTransformEnd\n" % (ts.CTM, line) if ctm else line
    return ts.HEAD + "WorldBegin\n" + ts.LIGHT + body + ts.TRI + "WorldEnd\n", index


def _footprints(rng, n, lo=-6., hi=-1.):
    scale = 10 ** rng.uniform(lo, hi, (n, 1))
    return rng.normal(size=(n, 3)) * scale, rng.normal(size=(n, 3)) * scale


def _uv(rng, n, zero=False):
    uv = rng.uniform(-2, 3, (n, 2))
    duv = np.zeros((n, 4)) if zero else rng.normal(size=(n, 4)) * 10 ** rng.uniform(-6, -1, (n, 1))
    return uv, duv


def groups():
    """{group: [n, 15] float32}: about 4 000 queries."""
    rng = np.random.default_rng(31)
    g = {}

    def put(name, p, dx, dy, uv, duv):
        g[name] = np.concatenate([p, dx, dy, uv, duv], axis=1).astype(np.float32)

    put("|p| <= 3", rng.uniform(-3, 3, (700, 3)), *_footprints(rng, 700), *_uv(rng, 700))
    put("|p| <= 300", rng.uniform(-300, 300, (700, 3)), *_footprints(rng, 700, -4, 0), *_uv(rng, 700))
    # the axis of the spherical and cylindrical mappings (z) and the other two, both directions, and the plane of the poles' opposite
    axis = np.zeros((450, 3))
    axis[np.arange(450), np.arange(450) % 3] = rng.choice([-1., 1.], 450) * 10 ** rng.uniform(-2, 2, 450)
    put("on the axes", axis, *_footprints(rng, 450), *_uv(rng, 450))
    # within 1e-6 (in angle) of the phi seam of either mapping: the half planes y = 0, x > 0 and y = 0, x < 0
    e = rng.uniform(-1e-6, 1e-6, 500)
    r = 10 ** rng.uniform(-1, 1.5, 500) * np.where(np.arange(500) % 2 == 0, 1., -1.)
    seam = np.stack([r * np.cos(e), r * np.sin(e), rng.uniform(-5, 5, 500)], axis=1)
    put("within 1e-6 of the phi seam", seam, *_footprints(rng, 500, -5, -2), *_uv(rng, 500))
    # a footprint that straddles the seam: it starts on one side and ends well on the other
    e = rng.choice([-1., 1.], 300) * rng.uniform(.01, .1, 300)
    r = 10 ** rng.uniform(-1, 1, 300) * np.where(np.arange(300) % 2 == 0, 1., -1.)
    p = np.stack([r * np.cos(e), r * np.sin(e), rng.uniform(-2, 2, 300)], axis=1)
    across = np.stack([rng.normal(size=300) * 1e-3, -np.sign(e) * np.abs(r) * np.sign(r) * 30 * np.abs(e), rng.normal(size=300) * 1e-3], axis=1)   # (mostly along y)
    put("a footprint across the phi seam", p, across, -.5 * across, *_uv(rng, 300))
    put("footprint 0", rng.uniform(-30, 30, (400, 3)), np.zeros((400, 3)), np.zeros((400, 3)), *_uv(rng, 400, zero=True))
    p = rng.uniform(-3, 3, (400, 3))
    dx, dy = rng.normal(size=(400, 3)), rng.normal(size=(400, 3))
    norm = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    length = np.linalg.norm(p, axis=1, keepdims=True) * rng.uniform(3, 30, (400, 1))
    uv, duv = _uv(rng, 400)
    put("footprint longer than |p|", p, norm(dx) * length, norm(dy) * length, uv, duv * 1e3)
    # st within 2^-20 of an integer or of a half-integer (the dots' cell edge), for the scales the cases use
    base = np.concatenate([rng.integers(-4, 5, 150).astype(np.float64), rng.integers(-4, 5, 150) + .5,
                           (rng.integers(-12, 13, 80) + .5) / 6, (rng.integers(-12, 13, 80) + .5) / 5, rng.integers(-8, 9, 70) / 4., rng.integers(-8, 9, 70) / 3.])
    n = len(base)
    coord = lambda: rng.permutation(base) + rng.choice([-1., 1.], n) * rng.uniform(0, 1, n) * 2. ** -20
    pxyz = np.stack([coord(), coord(), coord()], axis=1)
    put(NEAR, pxyz, *_footprints(rng, n, -6, -3), pxyz[:, :2], _uv(rng, n)[1] * 1e-2)
    assert 3500 <= sum(len(v) for v in g.values()) <= 4500
    return g


def restate(rec, q, basis, mode):
    """Both precisions of mode 0 (the mapping, [n, 6]) or mode 1 (the value: [n, 31] or [n]) with the queries on which they
    decided alike. -> v32, v64, judged [n]."""
    a, b = tm.both(rec)
    if mode == 0:
        (v32, d32), (v64, d64) = (tm.map2d(t, q[:, 0:3], q[:, 3:6], q[:, 6:9], q[:, 9:11], q[:, 11:15]) for t in (a, b))
    else:
        (v32, d32), (v64, d64) = tm.evaluate(a, q, basis), tm.evaluate(b, q, basis)
    return v32, v64, tm.same_decisions(d32, d64)
