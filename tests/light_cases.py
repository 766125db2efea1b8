"""The lights, environment maps and query families shared by test_light_restatement.py (CPU) and test_light_gpu.py: scenes
with one light each, and per light the reference points, u pairs and directions of the light probe (mi_pt_light_probe). Nothing
here calls the product's kernels or the oracle; the restatement (light_restatement.py) is asked where a family needs a table
entry or a sampled point to aim at.

A Family with `rim` set sits on a discrete decision by construction (a direction exactly on a cell border of the
Distribution2D, a point exactly on a cone of the spot light, a point in the plane of a slanted triangle): float32 and float64
legitimately decide either way there, so the 1 % cap on unsure queries is not asked of it and the tests hold it to the bits of
the float32 restatement, or to the value of either neighbour, instead."""
import math

import numpy as np

import light_restatement as lr

ONE_MINUS_EPS = np.float32(1) - np.float32(2.0 ** -24)   # 0x1.fffffep-1

HEAD = ('LookAt 0 2.5 9  0 1 0  0 1 0\nCamera "perspective" "float fov" [45]\n'
        'Film "image" "integer xresolution" [16] "integer yresolution" [16]\n'
        'Sampler "halton" "integer pixelsamples" [4]\nIntegrator "path" "integer maxdepth" [2]\nWorldBegin\n')
BALL = 'AttributeBegin\nMaterial "matte"\nShape "sphere" "float radius" [2]\nAttributeEnd\n'


def text(body):
    return HEAD + body + "WorldEnd\n"


def light_of(scene, kind):
    """Index of the scene's only light of mi_light_type `kind`."""
    found = [i for i in range(scene.desc.n_lights) if scene.desc.lights[i].type == kind]
    assert len(found) == 1, (kind, found)
    return found[0]


class Family:
    def __init__(self, name, q, rim=False):
        self.name, self.q, self.rim = name, np.ascontiguousarray(q, np.float32), rim


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def uniform_directions(rng, n):
    return unit(rng.normal(size=(n, 3)))


def pack(*cols):
    """Columns (arrays [n, k] or rows broadcast to n) side by side as float32 queries."""
    n = max(len(c) for c in cols if np.ndim(c) == 2)
    return np.concatenate([np.broadcast_to(np.asarray(c, np.float64), (n, np.shape(c)[-1])) for c in cols], axis=1).astype(np.float32)


def radical_pairs(n):
    """(RadicalInverse(0, i), RadicalInverse(1, i)), i < n, as Shape::SolidAngle draws them (shape.cpp:94)."""
    i = np.arange(n, dtype=np.uint64)
    b2 = np.zeros(n)
    f, k = 0.5, i.copy()
    while k.any():
        b2 += f * (k & np.uint64(1)).astype(np.float64)
        k >>= np.uint64(1)
        f *= 0.5
    b3 = np.zeros(n)
    f, k = 1 / 3.0, i.copy()
    while k.any():
        b3 += f * (k % np.uint64(3)).astype(np.float64)
        k //= np.uint64(3)
        f /= 3.0
    return np.minimum(np.stack([b2, b3], axis=1).astype(np.float32), ONE_MINUS_EPS)


# ---------------------------------------------------------------------------------------------------------------------
# the infinite light
def _map_constant(rng):
    return np.tile(np.array([0.7, 0.9, 1.2], np.float32), (2, 4, 1))


def _map_random(rng):
    return (rng.random((8, 16, 3)) ** 3 * 4 + 0.01).astype(np.float32)


def _map_black_rows(rng):
    """Rows 1 and 2 and columns 4 and 5 are black. (The light's distribution is filtered out of the map at twice its
    resolution with a bilinear lookup a quarter texel off the texel centres, infinite.cpp:64-75, so one black row of the map
    leaves no row of the distribution black; two neighbouring ones leave one: funcInt == 0 there and the i / n cdf.)"""
    img = (rng.random((4, 8, 3)) + 0.2).astype(np.float32)
    img[1:3] = 0
    img[:, 4:6] = 0
    return img


def _map_one_texel(rng):
    img = np.zeros((4, 8, 3), np.float32)
    img[1, 3] = [5, 4, 2]
    return img


MAPS = {"constant 4x2": _map_constant, "random 16x8": _map_random, "black rows and columns 8x4": _map_black_rows,
        "one texel 8x4": _map_one_texel}
TRANSFORMS = {"identity": "", "rotated": "Rotate -90 1 0 0\nRotate 37 0 0 1\n", "mirrored": "Scale -1 1 1\n",
              "non-uniform scale": "Scale 1 2 .5\n"}
RIGID = ("identity", "rotated", "mirrored")


def write_pfm(path, img):
    h, w, _ = img.shape
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n-1.0\n" % (w, h))
        f.write(np.ascontiguousarray(img[::-1], "<f4").tobytes())


def infinite_scene(pt, tmp_path, map_name, xf_name):
    img = MAPS[map_name](np.random.default_rng(21))
    write_pfm(str(tmp_path / "env.pfm"), img)
    body = 'AttributeBegin\n%sLightSource "infinite" "string mapname" "env.pfm"\nAttributeEnd\n' % TRANSFORMS[xf_name] + BALL
    s = pt.Scene(text=text(body), base_dir=str(tmp_path))
    assert s.errors == [] and s.desc.n_lights == 1 and s.desc.n_envmaps == 1
    e = s.desc.envmaps[0]
    assert (e.width, e.height) == (img.shape[1], img.shape[0]) and (e.nu, e.nv) == (2 * e.width, 2 * e.height)
    return s, 0


def _beside(x):
    """x, one float32 below and one above, kept inside [0, 1)."""
    x = np.asarray(x, np.float32)
    out = np.concatenate([x, np.nextafter(x, np.float32(-1)), np.nextafter(x, np.float32(2))])
    return np.clip(out, np.float32(0), ONE_MINUS_EPS)


def infinite_u_families(light, rng):
    """u pairs for mode 0 (light: the float32 record). Every family is [n, 2]."""
    env = light.env
    fams = [Family("random u", rng.random((2000, 2)).astype(np.float32)),
            Family("corners", np.array([[0, 0], [0, ONE_MINUS_EPS], [ONE_MINUS_EPS, 0], [ONE_MINUS_EPS, ONE_MINUS_EPS]], np.float32), rim=True)]
    # (u on a cdf entry puts the sample on a texel border of the map: next to a black texel Li == 0 is a decision -- rim.
    # The first and the last entry are the poles, where pdf ~ 1 / sin(theta) is ill-conditioned: a family of their own.)
    for label, entries in (("u1 on marg_cdf", env.marg_cdf[1:-1]), ("u1 on marg_cdf, the poles", env.marg_cdf[[0, -1]])):
        u1 = _beside(entries)
        fams.append(Family(label, np.stack([np.full(len(u1), np.float32(0.37)), u1], axis=1), rim=True))
    # one row of cond_cdf: the lit row with the most runs of equal entries; u1 in the middle of that row's interval
    lit = np.nonzero(env.cond_func_int > 0)[0]
    runs = [(int((np.diff(env.cond_cdf[v]) == 0).sum()), -abs(int(v) - env.nv // 2), int(v)) for v in lit]
    v = max(runs)[2]
    mid = np.float32(0.5) * (env.marg_cdf[v] + env.marg_cdf[v + 1])
    u0 = _beside(env.cond_cdf[v])
    fams.append(Family("u0 on cond_cdf[%d]" % v, np.stack([u0, np.full(len(u0), mid)], axis=1), rim=True))
    tied = np.nonzero(np.diff(env.cond_cdf[v]) == 0)[0]
    if len(tied):
        u0 = _beside(env.cond_cdf[v][tied])
        fams.append(Family("u0 in a run of equal cdf entries", np.stack([u0, np.full(len(u0), mid)], axis=1), rim=True))
    tied = np.nonzero(np.diff(env.marg_cdf) == 0)[0]
    if len(tied):
        u1 = _beside(env.marg_cdf[tied])
        fams.append(Family("u1 in a run of equal cdf entries", np.stack([np.full(len(u1), np.float32(0.61)), u1], axis=1), rim=True))
    fams.append(Family("u1 = 0 (d1 == 0)", np.stack([rng.random(64).astype(np.float32), np.zeros(64, np.float32)], axis=1)))
    return fams, v


def to_world(light64, local):
    """Light-frame vectors in world space (LightToWorld, float64), normalised."""
    return unit(np.asarray(local, np.float64) @ light64.l2w.T)


def infinite_direction_families(light64, rng):
    """World directions for modes 1 and 2, aimed in the light's frame."""
    nu, nv = light64.env.nu, light64.env.nv
    fams = [Family("uniform directions", to_world(light64, uniform_directions(rng, 2000)))]
    az = np.linspace(0, 2 * math.pi, 16, endpoint=False)
    ring = np.stack([1e-4 * np.cos(az), 1e-4 * np.sin(az), np.ones(16)], axis=1)
    fams.append(Family("the poles", to_world(light64, [[0, 0, 1], [0, 0, -1]]), rim=True))
    # (1e-4 from a pole cos(theta) is 1 - 5e-9: it rounds to 1 or to 1 - 2^-24, so theta is 0 or 3.5e-4 -- a decision)
    fams.append(Family("near the poles", to_world(light64, np.concatenate([ring, ring * [1, 1, -1]])), rim=True))
    seam, exact = [], []
    for z in (-0.9, -0.3, 0.0, 0.4, 0.8):
        r = math.sqrt(1 - z * z)
        for x in (r, -r):
            exact += [[x, 0.0, z], [x, -0.0, z]]
            seam += [[x, 1e-7 * x, z], [x, -1e-7 * x, z]]
    fams.append(Family("on the seam", to_world(light64, exact), rim=True))
    fams.append(Family("beside the seam", to_world(light64, seam), rim=True))
    on, beside = [], []
    for i in range(nu):   # the borders phi = 2 pi i / nu, at a few polar angles
        for th in np.linspace(0.07, math.pi - 0.07, 5) + 0.013 * (i + 1):   # (off the borders in theta)
            for dphi, into in ((0, on), (-1e-4, beside), (1e-4, beside), (-1e-3, beside), (1e-3, beside)):
                ph = 2 * math.pi * i / nu + dphi
                into.append([math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th)])
    for j in range(1, nv):   # the borders theta = pi j / nv, at a few azimuths
        for ph in np.linspace(0.1, 2 * math.pi - 0.3, 5) + 0.017 * j:
            for dth, into in ((0, on), (-1e-4, beside), (1e-4, beside), (-1e-3, beside), (1e-3, beside)):
                th = math.pi * j / nv + dth
                into.append([math.sin(th) * math.cos(ph), math.sin(th) * math.sin(ph), math.cos(th)])
    fams.append(Family("on the cell borders", to_world(light64, on), rim=True))
    fams.append(Family("beside the cell borders", to_world(light64, beside)))
    return fams


def cell_midpoints(light64):
    """Directions (world, float64, unit) at the midpoints of the distribution's cells in the light's frame, with the solid
    angle factor of each: sum over cells of pdf * sin(theta) * (2 pi / nu) * (pi / nv) is the integral of Pdf_Li."""
    nu, nv = light64.env.nu, light64.env.nv
    ph, th = np.meshgrid(2 * math.pi * (np.arange(nu) + 0.5) / nu, math.pi * (np.arange(nv) + 0.5) / nv)
    local = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=-1).reshape(-1, 3)
    return to_world(light64, local), (np.sin(th) * (2 * math.pi / nu) * (math.pi / nv)).reshape(-1)


def cell_of(light64, wi):
    """The cell (iv * nu + iu) of world directions, in float64, for histograms."""
    return lr.infinite_pdf_li(light64, np.asarray(wi, np.float64))["cell"]


# ---------------------------------------------------------------------------------------------------------------------
# the delta lights
SPOT_FROM, SPOT_TO = (1.0, 2.0, -1.0), (0.5, -1.0, 0.3)
SPOTS = {"wide": (60, 20), "narrow": (5, 1), "no band": (40, 0)}
DELTA = {"point": 'LightSource "point" "rgb I" [30 25 20] "point from" [1 2 -1]\n',
         "distant": 'LightSource "distant" "rgb L" [3 2.5 2] "point from" [1 2 -1] "point to" [.5 -1 .3]\n'}


def spot_text(name):
    cone, delta = SPOTS[name]
    return ('LightSource "spot" "rgb I" [30 25 20] "point from" [%g %g %g] "point to" [%g %g %g] "float coneangle" [%g] '
            '"float conedeltaangle" [%g]\n' % (SPOT_FROM + SPOT_TO + (cone, delta)))


def delta_scene(pt, body, kind):
    s = pt.Scene(text=text(body + BALL))
    assert s.errors == [] and s.desc.n_lights == 1
    return s, light_of(s, kind)


def _frame(axis):
    axis = unit(axis)
    a = np.cross(axis, [0.0, 0.0, 1.0] if abs(axis[2]) < 0.9 else [1.0, 0.0, 0.0])
    a = unit(a)
    return a, np.cross(axis, a), axis


def reference_point_families(rng, cones=None, l32=None):
    """Reference points (with a normal: the probe takes one) around the light at SPOT_FROM. cones: the spot's (total width,
    falloff start) in degrees -- rings at those angles from the axis, +- 1e-3 rad, and on the rim (+- 0 and 1e-6 rad)."""
    p = np.array(SPOT_FROM)
    d = uniform_directions(rng, 600)
    fams = [Family("sphere around the light", pack(p + 3 * d, -d)),
            Family("distance 1e-3", pack(p + 1e-3 * d[:40], -d[:40])),
            Family("distance 1e4", pack(p + 1e4 * d[:40], np.zeros((40, 3))))]
    if cones is not None:
        a, b, axis = _frame(np.array(SPOT_TO) - p)
        az = np.linspace(0, 2 * math.pi, 24, endpoint=False) + 0.1
        for label, offsets, rim in (("rings beside the cones", (-1e-3, 1e-3), False), ("on the cones", (0.0, -1e-6, 1e-6), True)):
            pts = []
            for deg in cones:
                for off in offsets:
                    th = math.radians(deg) + off
                    pts.append(p + 3 * (math.cos(th) * axis + math.sin(th) * (np.cos(az)[:, None] * a + np.sin(az)[:, None] * b)))
            pts = np.concatenate(pts)
            fams.append(Family(label, pack(pts, np.zeros_like(pts)), rim=rim))
        if l32 is not None:   # points whose float32 cos(theta) IS a cone's cosine: the two comparisons of Falloff at equality
            th = np.radians(np.repeat(np.asarray(cones, np.float64), 20000))
            az = rng.uniform(0, 2 * math.pi, len(th))
            d = np.cos(th)[:, None] * axis + np.sin(th)[:, None] * (np.cos(az)[:, None] * a + np.sin(az)[:, None] * b)
            pts = (p + rng.uniform(0.5, 4, (len(th), 1)) * d).astype(np.float32)
            cos32 = lr.spot_sample_li(l32, pts)["cos_theta"]
            on = np.concatenate([np.nonzero(cos32 == c)[0][:60] for c in (l32.cos_total_width, l32.cos_falloff_start)])
            assert len(on) >= 20, "no point found with cos(theta) exactly on a cone"
            fams.append(Family("cos(theta) exactly a cone's cosine", pack(pts[on], np.zeros((len(on), 3))), rim=True))
    return fams


# ---------------------------------------------------------------------------------------------------------------------
# triangle emitters
_TRI = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [%s]\n'
TRIANGLES = {
    "one-sided, in a coordinate plane": ('AreaLightSource "diffuse" "rgb L" [5 4 3]\n', _TRI % "-1 -1 0  2 -1 0  0 1.5 0"),
    "two-sided, slanted": ('AreaLightSource "diffuse" "rgb L" [5 4 3] "bool twosided" "true"\nTranslate .5 1 -1\nRotate 35 1 2 .5\n',
                           _TRI % "-1 -1 0  2 -1 0  0 1.5 0"),
    "reversed, slanted": ('AreaLightSource "diffuse" "rgb L" [5 4 3]\nReverseOrientation\nTranslate -1 .5 2\nRotate 70 0 1 1\n',
                          _TRI % "-1 -1 0  2 -1 0  0 1.5 0"),
    "needle 1:1e4": ('AreaLightSource "diffuse" "rgb L" [5 4 3]\nRotate 25 1 1 0\n', _TRI % "0 0 0  1 0 0  0 1e-4 0"),
}


def triangle_scene(pt, name):
    head, shape = TRIANGLES[name]
    s = pt.Scene(text=text("AttributeBegin\n" + head + shape + "AttributeEnd\n"))
    assert s.errors == [] and s.desc.n_lights == 1 and s.desc.n_tris == 1
    return s, 0


def triangle_point_families(light64, rng):
    """Reference points [n, 6] (p, n) for a triangle emitter; light64: the float64 record."""
    p0, p1, p2 = light64.tri
    c = (p0 + p1 + p2) / 3
    n = lr.tri_normal(light64)
    size = max(np.linalg.norm(p1 - p0), np.linalg.norm(p2 - p0))
    t1 = unit(p1 - p0)
    t2 = np.cross(n, t1)
    k = 12
    jitter = rng.uniform(-1, 1, (k, 2)) @ np.stack([t1, t2]) * size
    up = rng.uniform(0.5, 3, (k, 1)) * n
    fams = [Family("in front", pack(c + jitter + up, np.tile(-n, (k, 1)))),
            Family("behind", pack(c + jitter - up, np.zeros((k, 3)))),
            Family("distance 1e-4", pack(c + 1e-4 * unit(up + 0.3 * jitter / size), np.zeros((k, 3)))),
            Family("distance 1e4", pack(c + 1e4 * unit(up + 0.3 * jitter / size), np.zeros((k, 3))))]
    az = np.linspace(0, 2 * math.pi, k, endpoint=False) + 0.2
    plane = c + 3 * size * (np.cos(az)[:, None] * t1 + np.sin(az)[:, None] * t2)
    fams.append(Family("in the triangle's plane", pack(plane, np.zeros((k, 3))), rim=True))
    return fams


def triangle_edge_targets(light64):
    """Points just inside and just outside each edge (relative to the centroid): ([n, 3] beside, [m, 3] on the rim)."""
    p = light64.tri
    c = p.mean(axis=0)
    beside, rim = [], []
    for a in range(3):
        for t in (0.1, 0.35, 0.5, 0.8):
            e = (1 - t) * p[a] + t * p[(a + 1) % 3]
            for s, into in ((1e-3, beside), (-1e-3, beside), (1e-7, rim), (-1e-7, rim), (0.0, rim)):
                into.append(e + s * (c - e))
    return np.array(beside), np.array(rim)


# ---------------------------------------------------------------------------------------------------------------------
# the query sets of one light, and how an answer to them is held to the restatement
REF = np.array([0.3, 0.2, 0.1, 0, 0, 0], np.float32)   # a bare point inside the scene, for the lights that ignore it


def infinite_queries(l32, l64, rng):
    """[(mode, Family)] for an infinite light; the queries are in the probe's layout."""
    out = []
    ufams, _ = infinite_u_families(l32, rng)
    for f in ufams:
        out.append((0, Family(f.name, pack(REF[None, :], f.q), f.rim)))
    dfams = infinite_direction_families(l64, rng)
    sampled = lr.sample_li(l64, np.tile(REF[:3], (len(ufams[0].q), 1)), ufams[0].q)
    keep = ~sampled["zero"]
    dfams.append(Family("towards the sampled directions", sampled["wi"][keep]))
    for f in dfams:
        out.append((1, Family(f.name, pack(REF[None, :], f.q), f.rim)))
        out.append((2, Family(f.name, f.q, f.rim)))
    return out


def delta_queries(rng, cones=None, l32=None):
    out = [(0, Family(f.name, pack(f.q, np.zeros((len(f.q), 2))), f.rim)) for f in reference_point_families(rng, cones, l32)]
    pts = out[0][1].q[:200, :6]
    out.append((1, Family("Pdf_Li of a delta light", pack(pts, uniform_directions(rng, 200)))))
    return out


def _angle_to_edges(tri, ref, pts):
    """The smallest angle, seen from ref, between pts and the lines of the triangle's edges (float64)."""
    best = np.full(len(pts), np.inf)
    for a in range(3):
        e0, e1 = tri[a], tri[(a + 1) % 3]
        d = unit(e1 - e0)
        off = pts - e0
        perp = off - (off @ d)[:, None] * d
        best = np.minimum(best, np.linalg.norm(perp, axis=1) / np.linalg.norm(pts - ref, axis=1))
    return best


def triangle_queries(l64, rng):
    out = []
    u = np.concatenate([rng.random((200, 2)).astype(np.float32),
                        np.array([[0, 0], [0, ONE_MINUS_EPS], [ONE_MINUS_EPS, 0], [ONE_MINUS_EPS, ONE_MINUS_EPS]], np.float32)])
    beside, rim = triangle_edge_targets(l64)
    for f in triangle_point_families(l64, rng):
        refs = np.repeat(f.q, len(u), axis=0)
        us = np.tile(u, (len(f.q), 1))
        out.append((0, Family(f.name, pack(refs, us), f.rim)))
        p = lr.tri_sample(l64, us)[0]
        corner = np.tile(np.arange(len(u)) >= 200, len(f.q))
        for label, pts, sel, is_rim in (("the sampled points", p, ~corner, f.rim), ("the sampled corners", p, corner, True),
                                        ("points beside the edges", np.tile(beside, (len(f.q), 1)), None, f.rim),
                                        ("points on the edges", np.tile(rim, (len(f.q), 1)), None, True)):
            r = np.repeat(f.q, len(pts) // len(f.q), axis=0) if sel is None else refs
            to = pts - r[:, :3].astype(np.float64)
            ok = np.linalg.norm(to, axis=1) > 0
            if sel is not None:
                ok &= sel
            # a target closer to an edge than 1e-5 rad, seen from the reference point, is beyond what a float32 direction
            # resolves (the needle's short side, the triangle seen from 1e4 away): on the edge, for these purposes
            close = _angle_to_edges(l64.tri, r[:, :3].astype(np.float64), pts) < 1e-5
            for part, suffix, rim_part in ((ok & ~close, "", is_rim), (ok & close, " (closer than float32 resolves)", True)):
                if part.any():
                    out.append((1, Family("%s, towards %s%s" % (f.name, label, suffix), pack(r[part], unit(to[part])), rim_part)))
    n = lr.tri_normal(l64)
    w = uniform_directions(rng, 500)
    out.append((2, Family("L(n, w), uniform w", pack(np.tile(n, (len(w), 1)), w))))
    a, b, _ = _frame(n)
    az = np.linspace(0, 2 * math.pi, 32, endpoint=False)
    w = np.cos(az)[:, None] * a + np.sin(az)[:, None] * b
    out.append((2, Family("L(n, w), w across n", pack(np.tile(n, (len(w), 1)), w), rim=True)))
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bar(a32, a64, sel):
    """disk_shape.bar: four times the worst float32-vs-float64 deviation of the restatement over the selected queries of one
    family, never below 8 ulp (float32) of the largest component."""
    a, b = np.asarray(a32)[sel].astype(np.float64), np.asarray(a64)[sel]
    if a.size == 0:
        return 0.0
    return float(max(4 * np.abs(a - b).max(), 8 * float(np.spacing(np.float32(np.abs(b).max())))))


def check(label, name, got, r32, r64, sel, log):
    if not sel.any():
        return
    b = bar(r32, r64, sel)
    worst = float(np.abs(got[sel].astype(np.float64) - np.asarray(r64)[sel]).max())
    log.append("%s: %s worst %.3e / bar %.3e over %d" % (label, name, worst, b, int(sel.sum())))
    assert worst <= b, log[-1]


def check_rel(label, name, got, f32, f64, sel, log):
    """_check_rel of test_sphere_gpu.py: four times the worst relative float32-vs-float64 deviation, never below 8 * 2^-23."""
    if not sel.any():
        return
    rel = float(np.abs(got[sel].astype(np.float64) / f64[sel] - 1).max())
    b = max(4 * float(np.abs(f32[sel].astype(np.float64) / f64[sel] - 1).max()), 8 * 2.0 ** -23)
    log.append("%s: %s worst relative %.3e / bar %.3e over %d" % (label, name, rel, b, int(sel.sum())))
    assert rel <= b, log[-1]


def hold(label, l32, l64, mode, fam, got, log):
    """One family's answers `got` (from the oracle's or the device's probe) against the two restatements: the unsure cap, the
    verdicts, the values within the family's own bars. Appends its "worst / bar" lines to log."""
    q = fam.q
    label = "%s, mode %d, %s" % (label, mode, fam.name)
    if mode == 0:
        r32, r64 = lr.sample_li(l32, q[:, :3], q[:, 6:8]), lr.sample_li(l64, q[:, :3], q[:, 6:8])
        d32, d64 = lr.decisions(l32, r32), lr.decisions(l64, r64)
        unsure = (d32 != d64).any(axis=1)
        if not fam.rim:
            assert unsure.mean() <= 0.01, (label, "unsure", float(unsure.mean()))
        dg = np.stack([(got[:, 3] == 0).astype(np.int64), (got[:, 10:] == 0).all(axis=1).astype(np.int64)], axis=1)
        same32, same64 = (dg == d32[:, :2]).all(axis=1), (dg == d64[:, :2]).all(axis=1)
        if l32.type == lr.SPOT:
            # the branch shows in Li: black outside the cone (and in the band where the falloff is exactly 0), the point light's
            # (I * 1) / d^2 bit for bit inside the inner cone (and in the band where the falloff is exactly 1)
            full = (bits(got[:, 10:]) == bits(lr.point_sample_li(l32, q[:, :3])["Li"])).all(axis=1)
            for r, same in ((r32, same32), (r64, same64)):
                same &= np.where(r["branch"] == 0, dg[:, 1] == 1, np.where(r["branch"] == 2, full, (dg[:, 1] == 1) == (r["falloff"] == 0)))
                same &= ~full | (r["branch"] == 2) | (r["falloff"] == 1)
        wrong = np.nonzero(np.where(unsure, ~(same32 | same64), ~same64))[0]
        assert len(wrong) == 0, (label, "verdicts", len(wrong), q[wrong[0]].tolist(), dg[wrong[0]].tolist(), d64[wrong[0]].tolist())
        nothing = (d64[:, 0] == 1) & (d64[:, 1] == 1) & ~unsure & (l32.type in (lr.AREA, lr.INFINITE))
        if l32.type == lr.INFINITE:
            nothing &= r64["none"]
        assert not got[nothing].any(), (label, "a sample that has no direction is all zeros")
        sel = ~unsure & ~((d64[:, 0] == 1) & (d64[:, 1] == 1))
        o32, o64 = lr.out_of(r32), lr.out_of(r64)
        finite = np.isfinite(o32[:, 3])
        assert np.array_equal(np.isinf(got[sel, 3]), ~finite[sel]), (label, "pdf overflows where the float32 restatement's does")
        for cols, name in ((slice(0, 3), "wi"), (slice(4, 7), "pLight.p"), (slice(7, 10), "pLight.n"), (slice(10, None), "Li")):
            check(label, name, got[:, cols], o32[:, cols], o64[:, cols], sel & np.isfinite(o32[:, cols]).all(axis=1), log)
        check_rel(label, "pdf", got[:, 3], o32[:, 3], o64[:, 3], sel & finite & (o64[:, 3] > 0) & (o32[:, 3] > 0), log)
        return unsure
    if mode == 1:
        r32, r64 = lr.pdf_li(l32, q[:, :3], q[:, 6:9]), lr.pdf_li(l64, q[:, :3], q[:, 6:9])
        unsure = r32["zero"] != r64["zero"]
        if "cell" in r32:
            unsure |= r32["cell"] != r64["cell"]
        if not fam.rim:
            assert unsure.mean() <= 0.01, (label, "unsure", float(unsure.mean()))
        pos = ~unsure & ~r64["zero"] & np.isfinite(r32["pdf"])
        b = max(4 * float(np.abs(r32["pdf"][pos].astype(np.float64) / r64["pdf"][pos] - 1).max()) if pos.any() else 0.0, 8 * 2.0 ** -23)
        if not fam.rim:
            assert np.array_equal((got == 0)[~unsure], r64["zero"][~unsure]), (label, "pdf == 0")
            check_rel(label, "Pdf_Li", got, r32["pdf"], r64["pdf"], pos, log)
            return unsure
        # on a decision: the answer of either restatement or, on a border of the Distribution2D, of a neighbouring cell --
        # within the relative bar of the family's sure queries
        cand = [r32["pdf"].astype(np.float64), r64["pdf"]]
        if "cell" in r64:
            e = l64.env
            iv, iu = r64["cell"] // e.nu, r64["cell"] % e.nu
            for dv in (-1, 0, 1):
                for du in (-1, 0, 1):
                    other = e.cond_func[np.clip(iv + dv, 0, e.nv - 1), (iu + du) % e.nu]
                    with np.errstate(divide="ignore", invalid="ignore"):
                        cand.append(np.where(r64["zero"], 0.0, r64["pdf"] * other / e.cond_func[iv, iu]))
        g = got.astype(np.float64)
        ok = (bits(got) == bits(r32["pdf"])) | ((g == 0) & (r32["zero"] | r64["zero"]))
        for c in cand:
            with np.errstate(divide="ignore", invalid="ignore"):
                ok |= np.abs(g / c - 1) <= b
            ok |= (g == 0) & (c == 0)
        log.append("%s: on a decision: %d of %d the float32 restatement's bits, all of them an answer of either side (bar %.3e)"
                   % (label, int((bits(got) == bits(r32["pdf"])).sum()), len(q), b))
        assert ok.all(), (log[-1], int((~ok).sum()), q[np.nonzero(~ok)[0][0]].tolist())
        return unsure
    if l32.type == lr.INFINITE:
        le32, le64 = lr.infinite_le(l32, q), lr.infinite_le(l64, q)
        check(label, "Le", got, le32, le64, np.ones(len(q), bool), log)
        return np.zeros(len(q), bool)
    (v32, e32), (v64, e64) = lr.area_l(l32, q[:, :3], q[:, 3:6]), lr.area_l(l64, q[:, :3], q[:, 3:6])
    unsure = e32 != e64
    if not fam.rim:
        assert unsure.mean() <= 0.01, (label, "unsure", float(unsure.mean()))
    assert np.array_equal(bits(got)[~unsure], bits(v32)[~unsure]), (label, "L(n, w)")
    either = (bits(got) == bits(v32)).all(axis=1) | (got == 0).all(axis=1)
    assert either.all(), label
    log.append("%s: L(n, w) bit for bit on %d, %d unsure" % (label, int((~unsure).sum()), int(unsure.sum())))
    return unsure


def answer(probe, queries):
    """One probe call per mode over every family's queries: {(mode, family name): output}."""
    out = {}
    for mode in (0, 1, 2):
        fams = [f for m, f in queries if m == mode]
        if not fams:
            continue
        got = probe(mode, np.concatenate([f.q for f in fams]))
        at = 0
        for f in fams:
            out[(mode, f.name)] = got[at:at + len(f.q)]
            at += len(f.q)
    return out
