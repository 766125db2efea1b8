"""Texture "fbm" / "wrinkled" / "windy" on the GPU. noise_texture.py restates the textures in float32 and float64; the unchanged
oracle knows no noise, so whole renders are held to the device's own render of a twin scene (the same text with a constant
in the texture's place: ground the existing suite holds to the oracle) times the restated texture value at each pixel's hit.
There is no hit / miss verdict and so no "unsure" class: a bar is four times the worst float32-vs-float64 deviation of the
restatement over the group, never below 8 ulp of the largest value (disk_shape.bar). FBm is continuous in every input, so
its bars are rounding bars. Turbulence is not: where the octave count n crosses an integer k the reference's sum jumps by
0.2 * omega^(k-1) * (1 - omega) (the clamped octaves' terms start one octave later), so in the group that puts n within 1e-6
of an integer the two restatements land on either side and the bar is as wide as the jump (0.4 at omega .5): it says only
that the device takes one of the two sides. Measured on an MI355X: the device returned the float32 restatement's value bit
for bit in every group of every case (worst deviation = a quarter of the bar).
A film pixel holds one sample (1 spp, box filter), except that the first Halton points of a 32 x 32 film lie exactly on pixel
borders and are added to the pixel before as well (57 of 1024 pixels hold two samples): the whole-render tests work out
which samples each pixel holds from the rays and check the film's weights against that, take a two-sample pixel's twin
apart with the neighbour's own pixel, and hold every pixel to the sum over its samples."""
import numpy as np
import pytest

import disk_shape as ds
import noise_texture as nt
import object_motion as om
import sphere_shape as ss

pytestmark = pytest.mark.gpu

_cache = {}


def _rel_l2(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.sqrt(((a - b) ** 2).sum() / max((b ** 2).sum(), 1e-30)))


# ---------------------------------------------------------------------------------------------------------------------
# 1: the probe against the restatement
PARAMS = [(8, .5), (0, .3), (3, .5), (12, .5), (8, 1)]
CTM = 'Translate .3 -1.2 .7\nRotate 35 1 2 .5\nScale 1.5 .6 2.5\n'
CASES = ([("fbm", o, r, False) for o, r in PARAMS] + [("wrinkled", o, r, False) for o, r in PARAMS] + [("windy", 8, .5, False)] +
         [(c, 8, .5, True) for c in ("fbm", "wrinkled", "windy")])


def _case_name(case):
    return "%s %d %g%s" % (case[0], case[1], case[2], " under a CTM" if case[3] else "")


def _probe_scene(pt):
    """Every case as a float texture of one scene (texture i is case i)."""
    if "probe" not in _cache:
        body = ""
        for cls, octaves, rough, ctm in CASES:
            par = "" if cls == "windy" else ' "integer octaves" [%d] "float roughness" [%g]' % (octaves, rough)
            line = 'Texture "t%d" "float" "%s"%s\n' % (len(body), cls, par)
            body += "TransformBegin\n%s%sTransformEnd\n" % (CTM, line) if ctm else line
        text = ('LookAt 0 0 8  0 0 0  0 1 0\nCamera "perspective" "float fov" [40]\nFilm "image" "integer xresolution" [8] "integer yresolution" [8]\n'
                'WorldBegin\nLightSource "point" "point from" [0 4 4]\n' + body +
                'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-3 -3 -1  3 -3 -1  0 3 -1]\nWorldEnd\n')
        s = pt.Scene(text=text)
        assert s.errors == [] and s.desc.n_textures == len(CASES)
        _cache["probe"] = (s, pt.CreateIntegrator(s))
    return _cache["probe"]


def _footprints(rng, n, lo=-6, hi=1):
    scale = 10 ** rng.uniform(lo, hi, (n, 1))
    return rng.normal(size=(n, 3)) * scale, rng.normal(size=(n, 3)) * scale


def _probe_groups():
    """{group: [n, 9] float32 queries (p, dpdx, dpdy)}: about 4 000 in all. Coordinates are the texture's own where the
    texture stands under the identity; under the CTM they are merely other points."""
    if "groups" in _cache:
        return _cache["groups"]
    rng = np.random.default_rng(20)
    g = {}

    def put(name, p, dx, dy):
        g[name] = np.concatenate([p, dx, dy], axis=1).astype(np.float32)

    put("|p| <= 3", rng.uniform(-3, 3, (600, 3)), *_footprints(rng, 600))
    put("|p| <= 300", rng.uniform(-300, 300, (600, 3)), *_footprints(rng, 600))
    ints = rng.integers(-600, 600, (400, 3)).astype(np.float64)
    ints[:40] = rng.choice([-256., -255., -1., 0., 255., 256., 257., 511., 512.], (40, 3))
    put("integer coordinates", ints, *_footprints(rng, 400))
    small = rng.integers(-4, 5, (200, 3)) + rng.choice([-1., 1.], (200, 3)) * rng.uniform(0, 1, (200, 3)) * 2. ** -20
    large = rng.integers(-300, 300, (200, 3)).astype(np.float32)
    large = np.nextafter(large, np.where(rng.random((200, 3)) < .5, -np.inf, np.inf).astype(np.float32))
    put("within 2^-20 of an integer", np.concatenate([small, large.astype(np.float64)]), *_footprints(rng, 400))
    put("footprint 0", rng.uniform(-30, 30, (400, 3)), np.zeros((400, 3)), np.zeros((400, 3)))
    put("footprint so large that n = 0", rng.uniform(-30, 30, (300, 3)), *_footprints(rng, 300, 1, 3))
    k = np.repeat(np.arange(1, 9), 50)
    delta = rng.uniform(-1e-6, 1e-6, len(k))
    length = 2. ** (-(k + delta) - 1)                       # -1 - .5 log2(length^2) = k + delta
    dirs = rng.normal(size=(len(k), 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    put("octave count next to 1 .. 8", rng.uniform(-30, 30, (len(k), 3)), dirs * length[:, None], .3 * dirs[:, [1, 2, 0]] * length[:, None])
    dx, dy = _footprints(rng, 500, -5, -1)
    put("dpdy longer than dpdx", rng.uniform(-30, 30, (250, 3)), dx[:250], 10 * dy[:250] * np.linalg.norm(dx[:250], axis=1, keepdims=True) / np.linalg.norm(dy[:250], axis=1, keepdims=True))
    put("dpdx longer than dpdy", rng.uniform(-30, 30, (250, 3)), dx[250:], .1 * dy[250:] * np.linalg.norm(dx[250:], axis=1, keepdims=True) / np.linalg.norm(dy[250:], axis=1, keepdims=True))
    assert 3500 <= sum(len(v) for v in g.values()) <= 4500
    _cache["groups"] = g
    return g


def _restated(rec, q):
    a, b = nt.both(rec)
    return nt.evaluate(a, q[:, 0:3], q[:, 3:6], q[:, 6:9]), nt.evaluate(b, q[:, 0:3], q[:, 3:6], q[:, 6:9])


def _hold(name, dev, v32, v64):
    """|device - float64 restatement| against the rule's bar over the group."""
    bar = ds.bar(v32, v64, slice(None))
    worst = float(np.abs(dev.astype(np.float64) - v64).max()) if len(dev) else 0.
    print("%-44s n %5d  bar %.3e  worst %.3e  largest |value| %.3e" % (name, len(dev), bar, worst, float(np.abs(v64).max()) if len(dev) else 0.))
    assert np.isfinite(dev).all()
    assert worst <= bar, (name, worst, bar)


@pytest.mark.parametrize("i", range(len(CASES)), ids=[_case_name(c) for c in CASES])
def test_probe_against_the_restatement(pt, i):
    s, integ = _probe_scene(pt)
    rec = s.desc.textures[i]
    assert rec.type == {"fbm": nt.TEX_FBM, "wrinkled": nt.TEX_WRINKLED, "windy": nt.TEX_WINDY}[CASES[i][0]]
    octaves = 6 if CASES[i][0] == "windy" else CASES[i][1]
    for name, q in _probe_groups().items():
        # (the reference converts lambda * p to int: it stays below 2^30 at the last octave)
        w2t = np.array(list(rec.w2t), np.float64).reshape(4, 4)
        assert np.abs(q[:, 0:3].astype(np.float64) @ w2t[:3, :3].T + w2t[:3, 3]).max() * 1.99 ** octaves < 2. ** 30
        v32, v64 = _restated(rec, q)
        dev = integ.texture_probe(i, q)
        if name == "footprint so large that n = 0":      # only the partial term, faded out: 0, and 0.2 per clamped octave
            a = nt.Tex(rec, np.float64)
            assert (nt.octaves(ds.xf_vector(a.w2t, q[:, 3:6].astype(np.float64)), ds.xf_vector(a.w2t, q[:, 6:9].astype(np.float64)), octaves)[0] == 0).all()
        _hold(_case_name(CASES[i]) + ", " + name, dev, v32, v64)


def test_probe_refuses_other_textures_and_bad_indices(pt, tmp_path):
    import scenes_text as st
    st.write_texture_files(str(tmp_path))
    s = pt.Scene(text='LookAt 0 0 8  0 0 0  0 1 0\nCamera "perspective"\nFilm "image" "integer xresolution" [8] "integer yresolution" [8]\nWorldBegin\n'
                      'LightSource "point" "point from" [0 4 4]\nTexture "i" "spectrum" "imagemap" "string filename" "tex_c.pfm"\n'
                      'Texture "c" "spectrum" "checkerboard"\nTexture "n" "float" "fbm"\nMaterial "matte" "texture Kd" "i"\n'
                      'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-3 -3 -1  3 -3 -1  0 3 -1]\nWorldEnd\n', base_dir=str(tmp_path))
    assert s.errors == []
    integ = pt.CreateIntegrator(s)
    q = np.zeros((4, 9), np.float32)
    assert integ.texture_probe(2, q).shape == (4,)
    for bad in (0, 1, 3, -1):
        with pytest.raises(RuntimeError):
            integ.texture_probe(bad, q)
    with pytest.raises(RuntimeError):
        integ.texture_lookup(2, np.zeros((1, 6), np.float32))       # mi_pt_texture_lookup keeps its job: image textures only


# ---------------------------------------------------------------------------------------------------------------------
# the hit of every pixel's camera ray, restated: p, the geometric n, dpdx, dpdy
HEAD = ('%(times)sLookAt 0 0 8  0 0 0  0 1 0\nCamera "perspective" "float fov" [40]\n'
        'Film "image" "integer xresolution" [%(res)d] "integer yresolution" [%(res)d]\n'
        'Sampler "halton" "integer pixelsamples" [%(spp)d]\n%(integrator)s\nWorldBegin\n'
        'LightSource "point" "point from" [1 3 6] "rgb I" [40 40 40]\n')
LIGHT_POS = np.array([1., 3., 6.])
PATH = 'Integrator "path" "integer maxdepth" [1]'
SPECTRAL = 'Integrator "spectralpath" "integer maxdepth" [1]'
QUAD = ('Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-3.2 -2.6 -1.5  -.2 -2.6 -.4  -.2 .4 -.9  -3.2 .4 -2] '
        '"float uv" [0 0 1 0 1 1 0 1]\n')
UNIT_QUAD = 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1 -1 0  1 -1 0  1 1 0  -1 1 0] "float uv" [0 0 1 0 1 1 0 1]\n'
INSTANCE_CTM = 'Translate 1.6 -1.4 -.5\nRotate 30 0 1 1\nScale 1.4 .8 1\n'
INSTANCE_CTM_END = 'Translate 1.9 -1.2 -.3\nRotate 50 0 1 1\nScale 1.2 .9 1\n'
TEXTURE_CTM = 'Translate .3 -.2 .1\nRotate 25 1 1 0\nScale 3.5 2.5 3\n'
NOISE_KD = 'Texture "kd" "spectrum" "fbm" "integer octaves" [6] "float roughness" [.6]'
CONSTANT_KD = 'Texture "kd" "spectrum" "constant" "rgb value" [1 1 1]'


def _colour_text(texture, integrator=PATH, res=32, spp=1, moving=False):
    """Scene 2: a tilted quad (mesh 0), a sphere and an ObjectInstance of a quad (mesh 1) under rotate + non-uniform scale, all
    matte with Kd = texture "kd", which is declared under a CTM of its own."""
    inst = om.pair(INSTANCE_CTM, INSTANCE_CTM_END) if moving else INSTANCE_CTM
    return (HEAD % dict(times="TransformTimes 0 1\n" if moving else "", res=res, spp=spp, integrator=integrator) +
            "TransformBegin\n" + TEXTURE_CTM + texture + "\nTransformEnd\n" + 'Material "matte" "texture Kd" "kd"\n' + QUAD +
            'AttributeBegin\nTranslate 1.4 1.3 -.3\nRotate 20 1 0 0\nShape "sphere" "float radius" [1.1]\nAttributeEnd\n'
            'ObjectBegin "q"\n' + UNIT_QUAD + 'ObjectEnd\nAttributeBegin\n' + inst + 'ObjectInstance "q"\nAttributeEnd\nWorldEnd\n')


def _pixel_samples(scene):
    sb = list(scene.desc.film.sample_bounds)
    return np.array([(px, py, 0) for py in range(sb[1], sb[3]) for px in range(sb[0], sb[2])], np.int32)


def _tri_vertices(scene, tri, f):
    d = scene.desc
    idx = np.array([[d.tri_indices[3 * t + k] for k in range(3)] for t in tri])
    P = np.array([d.P[i] for i in range(3 * d.n_verts)], np.float32).reshape(-1, 3).astype(f)
    UV = np.array([d.UV[i] for i in range(2 * d.n_verts)], np.float32).reshape(-1, 2).astype(f)
    return [P[idx[:, k]] for k in range(3)], [UV[idx[:, k]] for k in range(3)]


def _barycentrics(p0, p1, p2, o, d):
    """b0, b1, b2 of Triangle::Intersect (triangle.cpp:199-291) for a ray known to hit: the permutation, the shear, the edge
    functions (in double where one of them is zero), each divided by their sum."""
    f = o.dtype.type
    ad = np.abs(d)
    kz = np.where(ad[:, 0] > ad[:, 1], np.where(ad[:, 0] > ad[:, 2], 0, 2), np.where(ad[:, 1] > ad[:, 2], 1, 2))
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    row = np.arange(len(o))
    perm = lambda v: (v[row, kx], v[row, ky], v[row, kz])
    dx, dy, dz = perm(d)
    sx, sy = -dx / dz, -dy / dz
    t = []
    for q in (p0, p1, p2):
        x, y, z = perm(q - o)
        t.append((x + sx * z, y + sy * z))
    (x0, y0), (x1, y1), (x2, y2) = t
    e0, e1, e2 = x1 * y2 - y1 * x2, x2 * y0 - y2 * x0, x0 * y1 - y0 * x1
    zero = (e0 == 0) | (e1 == 0) | (e2 == 0)
    if zero.any():
        w = lambda a: a.astype(np.float64)
        e0 = np.where(zero, (w(y2) * w(x1) - w(x2) * w(y1)).astype(f), e0)
        e1 = np.where(zero, (w(y0) * w(x2) - w(x0) * w(y2)).astype(f), e1)
        e2 = np.where(zero, (w(y1) * w(x0) - w(x1) * w(y0)).astype(f), e2)
    inv = f(1) / (e0 + e1 + e2)
    return e0 * inv, e1 * inv, e2 * inv


def _tri_point(scene, tri, rays, f, device_b=None):
    """Triangle::Intersect's hit point, geometric normal and (dpdu, dpdv) (triangle.cpp:199-345) for rays [n, 7] given in the
    space the vertices are kept in. device_b: the device's (b0, b1), which the float32 barycentrics are printed against."""
    (p0, p1, p2), (uv0, uv1, uv2) = _tri_vertices(scene, tri, f)
    b0, b1, b2 = _barycentrics(p0, p1, p2, rays[:, 0:3].astype(f), rays[:, 3:6].astype(f))
    if device_b is not None and f == np.float32:
        off = (b0 != device_b[:, 0]) | (b1 != device_b[:, 1])
        print("barycentrics restated in float32: %d of %d differ from the device's, by at most %.2e"
              % (off.sum(), len(off), float(max(np.abs(b0 - device_b[:, 0]).max(), np.abs(b1 - device_b[:, 1]).max()))))
    p = b0[:, None] * p0 + b1[:, None] * p1 + b2[:, None] * p2
    dp02, dp12 = p0 - p2, p1 - p2
    n = ds.normalize(ds.cross(dp02, dp12))
    duv02, duv12 = uv0 - uv2, uv1 - uv2
    det = duv02[:, 0] * duv12[:, 1] - duv02[:, 1] * duv12[:, 0]
    assert (np.abs(det) >= 1e-8).all()
    inv = f(1) / det
    dpdu = (duv12[:, 1:2] * dp02 - duv02[:, 1:2] * dp12) * inv[:, None]
    dpdv = (-duv12[:, 0:1] * dp02 + duv02[:, 0:1] * dp12) * inv[:, None]
    uv = b0[:, None] * uv0 + b1[:, None] * uv1 + b2[:, None] * uv2
    return p, n, dpdu, dpdv, uv


def _surface(scene, rays, hits, f, instance_mesh=1):
    """What k_shade has at each camera ray's hit: world p, geometric n, dpdx, dpdy; for triangles the world (dpdu, dpdv) and
    the differentials of (u, v) besides. rays: camera_rays_ex rows; hits: trace rows. -> dict of [n, ...] arrays, `hit` [n]."""
    d = scene.desc
    n = len(rays)
    prim = hits[:, 0].copy().view(np.int32)
    hit = prim >= 0
    p, ng = np.zeros((n, 3), f), np.zeros((n, 3), f)
    dpdu, dpdv = np.zeros((n, 3), f), np.zeros((n, 3), f)
    shape = np.array([d.prims[k].shape if k >= 0 else 0 for k in prim])
    is_tri = hit & (shape >= 0)
    mesh = np.array([d.tri_mesh[t] if ok else -1 for t, ok in zip(shape, is_tri)])
    world_tri, inst_tri, sphere = is_tri & (mesh != instance_mesh), is_tri & (mesh == instance_mesh), hit & (shape < 0)
    if world_tri.any():
        p[world_tri], ng[world_tri], dpdu[world_tri], dpdv[world_tri], _ = _tri_point(scene, shape[world_tri], rays[world_tri, 0:7], f, hits[world_tri, 2:4])
    if inst_tri.any():
        assert d.n_instances == 1
        rows = np.flatnonzero(inst_tri)
        moving = d.instances[0].motion > 0
        anim = om.animated_of(scene, 0, f) if moving else None
        mats = []
        for r in rows:     # (a moving instance: the matrices of Interpolate(the ray's time))
            if moving:
                i2w, w2i = om.matrices_at(scene, 0, rays[r, 7], f, anim)
            else:
                i2w, w2i = list(d.instances[0].i2w), list(d.instances[0].w2i)
            mats.append((np.array(i2w, np.float64).astype(f).reshape(4, 4), np.array(w2i, np.float64).astype(f).reshape(4, 4)))
        local = np.concatenate([ds.xf_ray(w2i, rays[r:r + 1, 0:7]) for r, (_, w2i) in zip(rows, mats)])   # TransformedPrimitive::Intersect
        pi, ni, du, dv, _ = _tri_point(scene, shape[inst_tri], local, f, hits[inst_tri, 2:4])
        for j, (r, (i2w, w2i)) in enumerate(zip(rows, mats)):    # Transform::operator()(SurfaceInteraction), transform.cpp:255-288
            p[r] = ds.xf_point(i2w, pi[j:j + 1])[0]
            ng[r] = ds.normalize(ds.xf_normal(w2i, ni[j:j + 1]))[0]
            dpdu[r], dpdv[r] = ds.xf_vector(i2w, du[j:j + 1])[0], ds.xf_vector(i2w, dv[j:j + 1])[0]
    if sphere.any():
        assert d.n_spheres == 1
        h = ss.intersect(ss.Sphere(d.spheres[0], f), rays[sphere, 0:7])
        assert h["hit"].all()
        p[sphere], ng[sphere], dpdu[sphere], dpdv[sphere] = h["p"], h["n"], h["dpdu"], h["dpdv"]
    diff = [rays[:, 9 + 3 * k:12 + 3 * k].astype(f) for k in range(4)]       # rxOrigin, ryOrigin, rxDirection, ryDirection
    with np.errstate(invalid="ignore", divide="ignore"):
        dpdx, dpdy, duv = nt.compute_differentials(p, ng, diff[0], diff[1], diff[2], diff[3], dpdu, dpdv)
    return dict(hit=hit, tri=is_tri, p=p, n=ng, dpdx=dpdx, dpdy=dpdy, dpdu=dpdu, dpdv=dpdv, duv=duv,
                classes=dict(quad=world_tri, instance=inst_tri, sphere=sphere))


def _camera_and_hits(integ, scene):
    rays = integ.camera_rays_ex(_pixel_samples(scene))
    assert (rays[:, 8] == 1).all()
    return rays, integ.trace(np.ascontiguousarray(rays[:, :8]))


def _kd_of(scene):
    m = scene.desc.materials[scene.desc.prims[0].material]
    return np.array(list(m.bxdf[0].R), np.float64)


def _render_pair(pt, texture, twin_texture, **kw):
    key = (texture, twin_texture, tuple(sorted(kw.items())))
    if key not in _cache:
        s, twin = pt.Scene(text=_colour_text(texture, **kw)), pt.Scene(text=_colour_text(twin_texture, **kw))
        assert s.errors == [] and twin.errors == [], (s.errors, twin.errors)
        integ = pt.CreateIntegrator(s)
        film, weight = integ.Render()
        stats = integ.shade_launch_stats()
        tfilm, tweight = pt.CreateIntegrator(twin).Render()
        assert np.array_equal(weight, tweight)
        _cache[key] = (s, twin, integ, film, tfilm, weight, stats)
    return _cache[key]


def _noise_index(scene):
    k = [i for i in range(scene.desc.n_textures) if scene.desc.textures[i].type >= nt.TEX_FBM]
    assert len(k) == 1
    return k[0]


def _raster(scene, rays):
    """The film position (raster x, y, float64) of each pinhole camera ray: the inverse of PerspectiveCamera::GenerateRay."""
    cam = scene.desc.camera
    assert cam.lens_radius == 0 and cam.animated == 0
    r2c = np.array(list(cam.raster_to_camera), np.float64).reshape(4, 4)
    c2w = np.array(list(cam.camera_to_world), np.float64).reshape(4, 4)
    dcam = rays[:, 3:6].astype(np.float64) @ np.linalg.inv(c2w)[:3, :3].T
    z0 = r2c[2, 3] / r2c[3, 3]
    pcam = np.concatenate([dcam * (z0 / dcam[:, 2:3]), np.ones((len(rays), 1))], axis=1)
    ras = pcam @ np.linalg.inv(r2c).T
    return ras[:, 0] / ras[:, 3], ras[:, 1] / ras[:, 3]


def _samples_of_pixels(scene, rays, weight):
    """Which samples the box filter (radius .5) adds to which pixel (film.cpp:114-156): a sample's own pixel and, where the
    Halton point lies exactly on a pixel border (its first samples do, a few per cent of a 32 x 32 film), the pixel before
    it too. -> per pixel the list of its samples. The film's own weight sums (1 per sample) must say the same."""
    assert tuple(scene.desc.film.filter_radius) == (.5, .5)
    sb = list(scene.desc.film.sample_bounds)
    res = sb[2] - sb[0]
    assert sb[0] == 0 and sb[1] == 0 and sb[3] == res and len(rays) == res * res
    x, y = _raster(scene, rays)
    own = np.arange(res * res)
    assert np.array_equal(np.floor(x + 1e-4).astype(int), own % res) and np.array_equal(np.floor(y + 1e-4).astype(int), own // res)
    onx, ony = np.abs(x - np.round(x)) < 1e-4, np.abs(y - np.round(y)) < 1e-4
    lists = [[i] for i in own]
    for i in own:
        px, py = i % res, i // res
        for ddx, ddy, on in ((1, 0, onx[i]), (0, 1, ony[i]), (1, 1, onx[i] and ony[i])):
            if on and px - ddx >= 0 and py - ddy >= 0:
                lists[(py - ddy) * res + px - ddx].append(i)
    assert np.array_equal(np.array([len(l) for l in lists], np.float32), weight.reshape(-1))
    return lists


def _twin_per_sample(tfilm, lists):
    """The twin's radiance of each sample from its film sums: a pixel with one sample holds it; a pixel with two, one of which
    is known from that sample's own pixel, holds the other as the difference. -> [n, bins] and which are known."""
    n = len(lists)
    T, known = np.zeros_like(tfilm), np.zeros(n, bool)
    for i, l in enumerate(lists):
        if len(l) == 1:
            T[i], known[i] = tfilm[i], True
    for i, l in enumerate(lists):
        if len(l) == 2 and known[l[1]]:
            T[i], known[i] = tfilm[i] - T[l[1]], True
    return T, known


def _hold_film(name, film, tfilm, lists, gain, gain_tol, of_class):
    """film[pixel] == sum over the pixel's samples of gain[sample] * twin's radiance of that sample, within the samples'
    gain_tol times that radiance plus 8 ulp of the sums involved. At most 2 % of the pixels hold a sample the twin's film
    does not tell apart; they are counted, not judged."""
    T, known = _twin_per_sample(tfilm, lists)
    judged = np.array([all(known[j] for j in l) for l in lists])
    assert judged.mean() >= .98, judged.mean()
    want, tol = np.zeros_like(film), np.zeros_like(film)
    for i, l in enumerate(lists):
        if judged[i]:
            for j in l:
                want[i] += gain[j] * T[j]
                tol[i] += gain_tol[j] * np.abs(T[j])
    ulp = np.spacing(np.maximum(np.maximum(np.abs(want), tfilm), 1e-30).astype(np.float32)).astype(np.float64)
    err = np.abs(film - want)
    for cls, sel in of_class.items():
        k = judged & sel
        scale = np.maximum(np.abs(T[k]), 1e-30)
        print("%s, %-9s pixels %4d (two samples: %3d)  worst |film - expected| / twin %.3e, allowed there %.3e"
              % (name, cls, k.sum(), sum(len(lists[i]) > 1 for i in np.flatnonzero(k)), float((err[k] / scale).max()),
                 float(((tol[k] + 8 * ulp[k]) / scale).reshape(-1)[np.argmax((err[k] / scale).reshape(-1))])))
    bad = judged[:, None] & (err > tol + 8 * ulp)
    assert not bad.any(), (name, int(bad.sum()), float((err - tol - 8 * ulp)[bad].max()))
    return judged


def _check_colour(pt, integrator=PATH, moving=False):
    """film[px, b] == max(v, 0) * twin[px, b] / Kd_twin[b], v the texture restated at the hit of the pixel's sample (and the
    same sum over two samples where a pixel holds two)."""
    s, twin, integ, film, tfilm, weight, _ = _render_pair(pt, NOISE_KD, CONSTANT_KD, integrator=integrator, moving=moving)
    assert s.desc.n_instances == 1 and (s.desc.instances[0].motion > 0) == moving
    rays, hits = _camera_and_hits(integ, s)
    lists = _samples_of_pixels(s, rays, weight)
    a, b = _surface(s, rays, hits, np.float32), _surface(s, rays, hits, np.float64)
    rec = s.desc.textures[_noise_index(s)]
    t32, t64 = nt.both(rec)
    v32, v64 = nt.evaluate(t32, a["p"], a["dpdx"], a["dpdy"]), nt.evaluate(t64, b["p"], b["dpdx"], b["dpdy"])
    hit = a["hit"]
    kd = _kd_of(twin)
    nb = kd.size
    assert (kd > 0).all() and film.shape[2] >= nb and not film[:, :, nb:].any()
    film, tfilm = film.reshape(len(rays), -1)[:, :nb].astype(np.float64), tfilm.reshape(len(rays), -1)[:, :nb].astype(np.float64)
    # the texture takes both signs over the picture: a fifth of the hit pixels each (v <= 0 loses the lobe)
    assert (v64[hit] > 0).sum() >= hit.sum() / 5 and (v64[hit] <= 0).sum() >= hit.sum() / 5, ((v64[hit] > 0).sum(), hit.sum())
    gain, gain_tol = np.zeros((len(rays), nb)), np.zeros((len(rays), nb))
    for name, sel in a["classes"].items():
        assert sel.sum() >= 40, (name, sel.sum())
        bar = ds.bar(v32, v64, sel)
        print("%-9s samples %4d, lit %4d, v in [%.3f, %.3f], bar %.3e" % (name, sel.sum(), (sel & (tfilm > 0).any(axis=1)).sum(), v64[sel].min(), v64[sel].max(), bar))
        assert (sel & (tfilm > 0).any(axis=1)).sum() >= 20
        gain[sel] = np.maximum(v64[sel], 0)[:, None] / kd
        gain_tol[sel] = bar / kd
    judged = _hold_film("colour", film, tfilm, lists, gain, gain_tol, a["classes"])
    dark = np.array([all(hit[j] and v64[j] < -gain_tol[j, 0] for j in l) for l in lists]) & judged
    assert dark.sum() >= hit.sum() / 10 and not film[dark].any()          # the lobe is gone: black
    missed = np.array([not any(hit[j] for j in l) for l in lists])
    assert missed.any() and np.array_equal(film[missed], tfilm[missed])   # missed pixels are the twin's
    assert np.isfinite(film).all()


def test_colour_whole_render(pt):
    _check_colour(pt)


def test_colour_whole_render_spectralpath(pt):
    _check_colour(pt, integrator=SPECTRAL)


def test_colour_whole_render_with_a_moving_instance(pt, monkeypatch):
    monkeypatch.setenv("MIPT_OBJECT_MOTION", "1")
    _check_colour(pt, moving=True)


# ---------------------------------------------------------------------------------------------------------------------
# 3: bump, whole render
BUMP = 'Texture "w" "float" "wrinkled" "integer octaves" [5]\nTexture "b" "float" "scale" "texture tex1" "w" "float tex2" [.05]'
BUMP_QUAD = ('Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-3 -2.6 -1.5  3 -2.6 -.4  3 2.6 -.9  -3 2.6 -2] '
             '"float uv" [0 0 1 0 1 1 0 1]\n')
SMOOTH_MESH = ('Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-3 -2.6 -1.5  3 -2.6 -.4  3 2.6 -.9  -3 2.6 -2] '
               '"float uv" [0 0 1 0 1 1 0 1] "normal N" [-.3 -.2 1  .3 -.2 1  .3 .2 1  -.3 .2 1]\n')
BUMP_SPHERE = 'Translate 0 0 -1\nRotate 20 1 0 0\nShape "sphere" "float radius" [2.5]\n'


def _bump_text(shape, bumped, res=32):
    mat = 'Material "matte" "rgb Kd" [.6 .6 .6]' + (' "texture bumpmap" "b"\n' if bumped else "\n")
    return (HEAD % dict(times="", res=res, spp=1, integrator=PATH) + "TransformBegin\n" + TEXTURE_CTM + BUMP + "\nTransformEnd\n" + mat +
            "AttributeBegin\n" + shape + "AttributeEnd\nWorldEnd\n")


def _bump_pair(pt, shape):
    if ("bump", shape) not in _cache:
        s, twin = pt.Scene(text=_bump_text(shape, True)), pt.Scene(text=_bump_text(shape, False))
        assert s.errors == [] and twin.errors == []
        integ = pt.CreateIntegrator(s)
        film, weight = integ.Render()
        tfilm, _ = pt.CreateIntegrator(twin).Render()
        _cache[("bump", shape)] = (s, integ, film, tfilm, weight)
    return _cache[("bump", shape)]


def _bump_ratio(s, surf, f, shift_p):
    """|ns' . wi| / |ns . wi| per pixel: ns the flat quad's normal, ns' the bumped one, wi towards the point light."""
    t = nt.Tex(s.desc.textures[s.desc.materials[s.desc.prims[0].material].bump_tex], f)
    p, ng = surf["p"], surf["n"]
    ns = nt.bump(t, p, surf["dpdx"], surf["dpdy"], surf["duv"], surf["dpdu"], surf["dpdv"], ng, ng, shift_p=shift_p)
    wi = LIGHT_POS.astype(f)[None, :] - p
    dot = lambda a, b: a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]
    return np.abs(dot(ns, wi)) / np.abs(dot(ng, wi))


def test_bump_whole_render(pt):
    s, integ, film, tfilm, weight = _bump_pair(pt, BUMP_QUAD)
    assert s.desc.textures[s.desc.materials[s.desc.prims[0].material].bump_tex].post_scale == float(np.float32(.05))
    rays, hits = _camera_and_hits(integ, s)
    lists = _samples_of_pixels(s, rays, weight)
    a, b = _surface(s, rays, hits, np.float32, instance_mesh=-2), _surface(s, rays, hits, np.float64, instance_mesh=-2)
    film, tfilm = film.reshape(len(rays), -1)[:, :31].astype(np.float64), tfilm.reshape(len(rays), -1)[:, :31].astype(np.float64)
    sel = a["hit"] & (tfilm[:, 0] > 0)
    assert sel.sum() >= 300
    cut = lambda x: {k: (v[sel] if isinstance(v, np.ndarray) else v) for k, v in x.items()}
    r32, r64 = _bump_ratio(s, cut(a), np.float32, True), _bump_ratio(s, cut(b), np.float64, True)
    bar = ds.bar(r32, r64, slice(None))
    # the test tells a p shifted by du * dpdu from a p left in place: the two restated variants lie far apart
    still = _bump_ratio(s, cut(b), np.float64, False)
    apart = np.abs(still - r64) > 10 * bar
    print("bump: samples %d, bar %.3e, ratio in [%.3f, %.3f], |shifted - unshifted| > 10 bars on %d" % (sel.sum(), bar, r64.min(), r64.max(), apart.sum()))
    assert apart.sum() >= sel.sum() / 2
    gain, gain_tol = np.ones((len(rays), 31)), np.zeros((len(rays), 31))
    gain[sel], gain_tol[sel] = r64[:, None], bar
    _hold_film("bump", film, tfilm, lists, gain, gain_tol, dict(quad=sel))


@pytest.mark.parametrize("shape", [BUMP_SPHERE, SMOOTH_MESH], ids=["sphere", "mesh with vertex normals"])
def test_bump_on_curved_shading_geometry(pt, shape):
    s, integ, film, tfilm, _ = _bump_pair(pt, shape)
    assert np.isfinite(film).all() and film.any()
    assert _rel_l2(film, tfilm) > 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# 4: roughness and sigma
def _map_text(material, textures, res=16):
    return (HEAD % dict(times="", res=res, spp=1, integrator=PATH) + "TransformBegin\n" + TEXTURE_CTM + textures + "\nTransformEnd\n" + material + "\n" +
            BUMP_QUAD + "WorldEnd\n")


@pytest.mark.parametrize("name, textures, material, twin_material, field", [
    ("plastic roughness", 'Texture "r" "float" "wrinkled" "integer octaves" [4] "float roughness" [.4]',
     'Material "plastic" "rgb Kd" [.3 .3 .3] "rgb Ks" [.6 .6 .6] "texture roughness" "r"',
     'Material "plastic" "rgb Kd" [.3 .3 .3] "rgb Ks" [.6 .6 .6] "float roughness" [.3]', "rough"),
    ("matte sigma", 'Texture "g" "float" "fbm" "integer octaves" [4]\nTexture "r" "float" "scale" "texture tex1" "g" "float tex2" [60]',
     'Material "matte" "rgb Kd" [.6 .6 .6] "texture sigma" "r"', 'Material "matte" "rgb Kd" [.6 .6 .6] "float sigma" [20]', "sigma"),
])
def test_roughness_and_sigma_maps(pt, name, textures, material, twin_material, field):
    s, twin = pt.Scene(text=_map_text(material, textures)), pt.Scene(text=_map_text(twin_material, textures))
    assert s.errors == [] and twin.errors == []
    m = s.desc.materials[s.desc.prims[0].material]
    tex = m.rough_tex[0] if field == "rough" else m.sigma_tex
    assert tex >= 0 and s.desc.textures[tex].type >= nt.TEX_FBM
    integ = pt.CreateIntegrator(s)
    film, _ = integ.Render()
    tfilm, _ = pt.CreateIntegrator(twin).Render()
    assert np.isfinite(film).all() and film.any()
    assert _rel_l2(film, tfilm) > 1e-3
    # the bound texture at the restated hit of ten pixels
    rays, hits = _camera_and_hits(integ, s)
    a, b = _surface(s, rays, hits, np.float32, instance_mesh=-2), _surface(s, rays, hits, np.float64, instance_mesh=-2)
    rows = np.flatnonzero(a["hit"])[::max(1, a["hit"].sum() // 10)][:10]
    assert len(rows) == 10
    q = np.concatenate([a["p"][rows], a["dpdx"][rows], a["dpdy"][rows]], axis=1).astype(np.float32)
    v32, v64 = _restated(s.desc.textures[tex], q)
    _hold(name + ", ten hits", integ.texture_probe(tex, q), v32, v64)


# ---------------------------------------------------------------------------------------------------------------------
# 5: schedules, 6: routing
def test_pool_passes_and_shards_give_the_same_film(pt):
    s = pt.Scene(text=_colour_text(NOISE_KD, spp=4))
    assert s.errors == []
    integ = pt.CreateIntegrator(s)
    film, weight = integ.Render()
    assert film.any()
    small, w = integ.Render(path_pool=256)
    print("pool 256: relative L2 %.3e" % _rel_l2(small, film))
    assert np.array_equal(w, weight) and _rel_l2(small, film) < 1e-6
    integ.Render(spp=1, sample_begin=0, download=False)
    two, w = integ.Render(spp=3, sample_begin=1, accumulate=True)
    print("two passes: relative L2 %.3e" % _rel_l2(two, film))
    assert np.array_equal(w, weight) and _rel_l2(two, film) < 1e-6
    acc, accw = np.zeros_like(film), np.zeros_like(weight)
    for r in range(2):
        f, w = integ.Render(shard_index=r, shard_count=2)
        acc += f
        accw += w
    print("two shards: relative L2 %.3e" % _rel_l2(acc, film))
    assert np.array_equal(accw, weight) and _rel_l2(acc, film) < 1e-6


def test_noise_scene_launches_the_general_instances(pt):
    s, _, integ, film, _, _, stats = _render_pair(pt, NOISE_KD, CONSTANT_KD, integrator=PATH, moving=False)
    launches, blocks = stats
    assert launches > 0 and blocks > 0
    plan = s.shade_plan()
    textured = [plan["classes"][c] for c in set(plan["material_class"]) if plan["classes"][c]["types"] & pt.TM_TEXTURED]
    assert textured and all(k["tm"] == pt.TM_ALL for k in textured)           # (object instances: the instance code too)
    flat = pt.Scene(text=_bump_text(BUMP_QUAD, True))
    plan = flat.shade_plan()
    textured = [plan["classes"][c] for c in set(plan["material_class"]) if plan["classes"][c]["types"] & pt.TM_TEXTURED]
    assert textured and all(k["tm"] == pt.TM_FULL for k in textured)
