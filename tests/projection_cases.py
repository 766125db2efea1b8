"""The projection lights, their maps and the query families shared by test_projection_frontend.py (CPU) and
test_projection_gpu.py: four lights (maps of 4x2, 2x4 and 3x5 texels and none), each under an identity and a rotate +
non-uniform-scale CTM, the reference points of the light probe, and the wall scene. Nothing here calls the product's
kernels; the restatement (projection_light.py) is asked where a family aims at a screen position."""
import math
import os

import numpy as np

import light_cases as lc
import projection_light as pl
import scenes_text as st

INTENSITY = "30 25 20"
POS = (1.0, 2.0, -1.0)
TRANSFORMS = {"identity": "", "rotated and scaled": "Translate %g %g %g\nRotate 35 1 2 .5\nScale 1 2 .5\n" % POS}
FOV = 60.0


def _map_4x2(rng):
    """Dim texels and one bright column (column 2): four columns, two rows."""
    img = (rng.random((2, 4, 3)) * 0.08 + 0.02).astype(np.float32)
    img[:, 2] = [[4.0, 3.0, 1.5], [2.0, 5.0, 3.0]]
    return img


def _map_2x4(rng):
    """Eight-bit texels (a PNG: the reader applies the inverse gamma), two columns, four rows."""
    return rng.integers(20, 256, (4, 2, 3)).astype(np.uint8)


def _map_3x5(rng):
    """Not a power of two: the MIPMap resamples it to 4x8."""
    return (rng.random((5, 3, 3)) * 2 + 0.05).astype(np.float32)


# name -> (file name or None, image maker, the file's resolution (w, h), level 0's resolution)
MAPS = {"4x2": ("map_4x2.pfm", _map_4x2, (4, 2), (4, 2)), "2x4": ("map_2x4.png", _map_2x4, (2, 4), (2, 4)),
        "3x5": ("map_3x5.pfm", _map_3x5, (3, 5), (4, 8)), "none": (None, None, None, None)}


def write_map(base_dir, name):
    """Writes the map's file into base_dir; returns (file name, the image as written)."""
    fname, make, _, _ = MAPS[name]
    if fname is None:
        return None, None
    img = make(np.random.default_rng(41))
    path = os.path.join(str(base_dir), fname)
    if fname.endswith(".png"):
        st.write_png(path, img)
    else:
        lc.write_pfm(path, img)
    return fname, img


def light_text(mapname=None, fov=FOV, intensity=INTENSITY, extra=""):
    return ('LightSource "projection" "rgb I" [%s] "float fov" [%g]%s%s\n'
            % (intensity, fov, ' "string mapname" "%s"' % mapname if mapname else "", extra))


def light_scene(pt, base_dir, map_name, xf_name, fov=FOV):
    """A scene with the one projection light (index 0) and a ball; the file is written into base_dir."""
    fname, _ = write_map(base_dir, map_name)
    body = "AttributeBegin\n" + TRANSFORMS[xf_name] + light_text(fname, fov) + "AttributeEnd\n" + lc.BALL
    s = pt.Scene(text=lc.text(body), base_dir=str(base_dir))
    assert s.errors == [] and s.desc.n_lights == 1 and s.desc.lights[0].type == pl.PROJECTION
    return s, 0


# ---------------------------------------------------------------------------------------------------------------------
# the reference points of the probe, aimed in the light's frame (float64) and carried to the world
def _world_points(l64, local_dir, dist):
    """World points at distance `dist` (world units) from the light, in the world direction of the light-frame direction."""
    w = lc.unit(np.asarray(local_dir, np.float64) @ l64.l2w.T)
    return l64.pos[None, :] + np.asarray(dist, np.float64).reshape(-1, 1) * w


def _local_dir(l64, px, py):
    """The light-frame direction whose projection is the screen point (px, py): p = invTan * (x, y) / z."""
    inv_tan = l64.proj[0, 0]
    px, py = np.broadcast_arrays(np.asarray(px, np.float64), np.asarray(py, np.float64))
    return np.stack([px / inv_tan, py / inv_tan, np.ones_like(px)], axis=1)


def _queries(points):
    """Probe queries [n, 8]: ref.p, ref.n = 0, u = 0 (a delta light reads neither)."""
    return lc.pack(points, np.zeros((len(points), 5)))


def _beside32(x):
    x = np.float32(x)
    return [float(np.nextafter(x, np.float32(-np.inf))), float(x), float(np.nextafter(x, np.float32(np.inf)))]


def families(l64, rng, n_inside=1200):
    """[Family] of mode-0 queries for one projection light; about 2 000 queries. `rim`: the family sits on a decision (a screen
    edge, wl.z == hither) by construction."""
    x0, y0, x1, y1 = [float(v) for v in l64.screen]
    fams = []
    u = rng.random((n_inside, 2))
    px, py = x0 + (0.01 + 0.98 * u[:, 0]) * (x1 - x0), y0 + (0.01 + 0.98 * u[:, 1]) * (y1 - y0)
    fams.append(lc.Family("inside the frustum", _queries(_world_points(l64, _local_dir(l64, px, py), rng.uniform(0.5, 5, n_inside)))))
    # outside, in front of the light: between one and two half widths off the centre
    k = 120
    ang = rng.uniform(0, 2 * math.pi, k)
    r = rng.uniform(1.05, 2.0, k)
    ox, oy = r * np.cos(ang), r * np.sin(ang)
    scale = np.maximum(np.abs(ox) / x1, np.abs(oy) / y1)
    grow = np.where(scale < 1.05, 1.05 / scale, 1.0)
    fams.append(lc.Family("outside the screen bounds", _queries(_world_points(l64, _local_dir(l64, ox * grow, oy * grow), rng.uniform(0.5, 5, k)))))
    # the four edges: on them and one float32 either side, at a few places along each
    along = np.linspace(0.07, 0.93, 14)
    pts = []
    for edge in _beside32(x0) + _beside32(x1):
        pts.append(_local_dir(l64, np.full(len(along), edge), y0 + along * (y1 - y0)))
    for edge in _beside32(y0) + _beside32(y1):
        pts.append(_local_dir(l64, x0 + along * (x1 - x0), np.full(len(along), edge)))
    pts = np.concatenate(pts)
    fams.append(lc.Family("on and beside the screen edges", _queries(_world_points(l64, pts, rng.uniform(0.5, 5, len(pts)))), rim=True))
    # behind the light and around wl.z == hither: wl = d / |l2w d| for a light-frame direction d
    az = np.linspace(0, 2 * math.pi, 24, endpoint=False) + 0.05
    rows = []
    for rel in (-1e-2, -1e-5, -1e-7, 0.0, 1e-7, 1e-5, 1e-2):
        z = np.full(len(az), float(l64.hither) * (1 + rel))
        for _ in range(4):   # z = hither (1 + rel) |l2w d| with d = (cos, sin, z): a fixed point
            d = np.stack([np.cos(az), np.sin(az), z], axis=1)
            z = float(l64.hither) * (1 + rel) * np.linalg.norm(d @ l64.l2w.T, axis=1)
        rows.append(np.stack([np.cos(az), np.sin(az), z], axis=1))
    rows.append(np.stack([np.cos(az), np.sin(az), -np.abs(rng.normal(size=len(az))) - 0.1], axis=1))
    rows = np.concatenate(rows)
    fams.append(lc.Family("behind the light and around hither", _queries(_world_points(l64, rows, rng.uniform(0.5, 5, len(rows)))), rim=True))
    # texel centres and the texel borders inside the map (its outer borders are the screen edges)
    w, h = (l64.map.width, l64.map.height) if l64.map is not None else (4, 4)
    cs, ct = (np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h
    bs, bt = np.arange(1, w) / w, np.arange(1, h) / h
    for label, ss, tt in (("texel centres", cs, ct), ("texel borders", np.concatenate([bs, cs]), np.concatenate([bt, ct]))):
        s_, t_ = [g.reshape(-1) for g in np.meshgrid(ss, tt)]
        if label == "texel borders":   # (drop the centre-centre pairs: those are the other family)
            on = (np.isin(s_, bs) | np.isin(t_, bt))
            s_, t_ = s_[on], t_[on]
        loc = _local_dir(l64, x0 + s_ * (x1 - x0), y0 + t_ * (y1 - y0))
        fams.append(lc.Family(label, _queries(_world_points(l64, loc, rng.uniform(0.5, 5, len(loc))))))
    # very near and very far: d^2 from 1e-4 to 1e8
    k = 200
    u = rng.random((k, 2))
    px, py = x0 + (0.02 + 0.96 * u[:, 0]) * (x1 - x0), y0 + (0.02 + 0.96 * u[:, 1]) * (y1 - y0)
    dist = 10 ** np.concatenate([np.linspace(-2, 4, k - 2), [-2, 4]])
    fams.append(lc.Family("near and far", _queries(_world_points(l64, _local_dir(l64, px, py), dist))))
    return fams


def hold(label, l32, l64, fam, got, log):
    """One family's mode-0 answers against the two restatements: the unsure cap (families not built on an edge), Li == 0 where
    the float32 restatement has it wherever the two agree, and the values within the family's own bars. Returns (unsure, the
    count of output words equal to the float32 restatement's)."""
    q = fam.q
    label = "%s, %s" % (label, fam.name)
    r32, r64 = pl.sample_li(l32, q[:, :3]), pl.sample_li(l64, q[:, :3])
    unsure = r32["black"] != r64["black"]
    if not fam.rim:
        assert unsure.mean() <= 0.01, (label, "unsure", float(unsure.mean()))
    black = (got[:, 10:] == 0).all(axis=1)
    sure = ~unsure
    wrong = np.nonzero(sure & (black != r32["black"]))[0]
    assert len(wrong) == 0, (label, "Li == 0", len(wrong), q[wrong[0]].tolist())
    o32, o64 = pl.out_of(r32), pl.out_of(r64)
    assert np.array_equal(got[:, 3], np.ones(len(q), np.float32)), (label, "pdf")
    assert not got[:, 7:10].any(), (label, "pLight.n")
    every = np.ones(len(q), bool)
    lc.check(label, "wi", got[:, 0:3], o32[:, 0:3], o64[:, 0:3], every, log)
    lc.check(label, "pLight.p", got[:, 4:7], o32[:, 4:7], o64[:, 4:7], every, log)
    lit = sure & ~r64["black"]
    if lit.any():
        g, a, b = got[lit, 10:].reshape(-1), o32[lit, 10:].reshape(-1), o64[lit, 10:].reshape(-1)
        pos = (b > 0) & (a > 0) & np.isfinite(a)   # (a bin the Illuminant conversion clamps to 0 on one side only decides nothing)
        lc.check_rel(label, "Li", g, a, b, pos, log)
    same = int((lc.bits(got) == lc.bits(o32)).sum())
    log.append("%s: %d of %d output words are the float32 restatement's, %d of %d queries unsure" % (label, same, got.size, int(unsure.sum()), len(q)))
    return unsure, same


# ---------------------------------------------------------------------------------------------------------------------
# the wall: a matte quad lit by the projector, an occluder in the beam
WALL_HEAD = ('LookAt 0 0 6  0 0 0  0 1 0\nCamera "perspective" "float fov" [50]\n'
             'Film "image" "integer xresolution" [16] "integer yresolution" [16] "string filename" "wall.exr"\n'
             'PixelFilter "box" "float xwidth" [.5] "float ywidth" [.5]\n'
             'Sampler "halton" "integer pixelsamples" [1] "bool samplepixelcenter" "true"\n'
             'Integrator "path" "integer maxdepth" [1]\nWorldBegin\n')
WALL = ('AttributeBegin\nMaterial "matte" "rgb Kd" [.7 .6 .5]\n'
        'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-4 -4 0  4 -4 0  4 4 0  -4 4 0]\nAttributeEnd\n'
        'AttributeBegin\nMaterial "matte" "rgb Kd" [.2 .2 .2]\n'
        'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [.2 -.9 1.5  1.1 -.9 1.5  1.1 .3 1.5  .2 .3 1.5]\nAttributeEnd\n')
# the projector stands in front of the wall (z = 4), a little off the axis, and looks down -z: Rotate 180 about y
WALL_LIGHT_XF = "Translate .3 -.2 4\nRotate 180 0 1 0\nRotate 10 0 0 1\n"


def wall_text(light):
    """light: the LightSource statement (a projection light, or the point twin `point_twin()`), given in the projector's frame."""
    return WALL_HEAD + "AttributeBegin\n" + WALL_LIGHT_XF + light + "AttributeEnd\n" + WALL + "WorldEnd\n"


def point_twin(intensity=INTENSITY):
    return 'LightSource "point" "rgb I" [%s]\n' % intensity
