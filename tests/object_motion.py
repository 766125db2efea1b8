"""Helpers of the object-motion tests (test_object_motion_frontend.py, test_object_motion_gpu.py).

With MIPT_OBJECT_MOTION=1 a Shape or an ObjectInstance under an animated CTM becomes a moving TransformedPrimitive: an
mi_instance with an mi_motion record. camera_motion.py restates the reference's AnimatedTransform over float32 and float64;
here is what a moving primitive needs besides: the inverse that Interpolate's product carries (Transform::operator*,
transform.cpp:244-246, over Inverse(Matrix4x4), 82-136), Transform::operator()(Bounds3f) (231-242), and the scene texts.
The unchanged oracle ignores the motion record and renders an instance's i2w / w2i, so it renders any moving scene at
whatever pair of matrices a test writes there."""
import numpy as np

import camera_motion as cm

START_CAMERA = "3 2 8  0 0.5 0  0 1 0"

# an octahedron: eight triangles, so the object's tree has interior nodes
OCTAHEDRON = ('Shape "trianglemesh" "integer indices" [0 2 4  2 1 4  1 3 4  3 0 4  2 0 5  1 2 5  3 1 5  0 3 5] '
              '"point P" [.8 0 0  -.8 0 0  0 .8 0  0 -.8 0  0 0 .8  0 0 -.8]\n')
OCTAHEDRON_P = np.array([.8, 0, 0, -.8, 0, 0, 0, .8, 0, 0, -.8, 0, 0, 0, .8, 0, 0, -.8], np.float32).reshape(6, 3)
MOVER_MATERIAL = 'Material "matte" "rgb Kd" [.7 .3 .2]\n'


def pair(start, end):
    """Directives of the start member, then of the end member."""
    return 'ActiveTransform StartTime\n%s\nActiveTransform EndTime\n%s\nActiveTransform All\n' % (start, end)


def mover(kind, start, end, shape=OCTAHEDRON, before_shape=""):
    """The moving object: an ObjectInstance ("instance") or a Shape ("shape") under the CTM pair."""
    if kind == "instance":
        return ('ObjectBegin "mover"\n%s%sObjectEnd\nAttributeBegin\n%sObjectInstance "mover"\nAttributeEnd\n'
                % (MOVER_MATERIAL, shape, pair(start, end)))
    assert kind == "shape"
    return 'AttributeBegin\n%s%s%s%sAttributeEnd\n' % (pair(start, end), MOVER_MATERIAL, before_shape, shape)


def lit_scene(block, times=(0, 1), camera='"float fov" [45]', sampler="halton", spp=4, res=(32, 24),
              integrator='Integrator "path" "integer maxdepth" [4]'):
    """camera_motion.lit_scene (a point light and an area light over matte, plastic and glass) behind a camera that stands
    still, with `block` added to the world."""
    text = cm.lit_scene(cm.static_camera(START_CAMERA, camera), res=res, spp=spp, sampler=sampler, integrator=integrator)
    assert text.count("WorldEnd\n") == 1
    return 'TransformTimes %g %g\n' % times + text.replace("WorldEnd\n", block + "WorldEnd\n")


def bare_scene(block, times=(0, 1)):
    """Nothing but `block` in the world (the world tree's root bound is then the block's)."""
    return ('TransformTimes %g %g\n%sFilm "image" "integer xresolution" [8] "integer yresolution" [8]\nWorldBegin\n'
            'LightSource "point" "point from" [0 9 0]\n%sWorldEnd\n' % (times[0], times[1], cm.static_camera(START_CAMERA), block))


# ---------------------------------------------------------------------------------------------------------------------
def inverse3(m9, f=np.float32):
    """The device's form of Inverse for a matrix bordered by (0, 0, 0, 1): the same Gauss-Jordan with full pivoting on the
    3x3 block alone."""
    a = [[f(m9[3 * r + c]) for c in range(3)] for r in range(3)]
    done, reduced = [], [False] * 3
    for _ in range(3):
        best, pr, pc = f(0), 0, 0
        for r in range(3):
            if reduced[r]:
                continue
            for c in range(3):
                if not reduced[c] and abs(a[r][c]) >= best:
                    best, pr, pc = abs(a[r][c]), r, c
        reduced[pc] = True
        a[pr], a[pc] = a[pc], a[pr]
        done.append((pr, pc))
        scale = f(1.0 / float(a[pc][pc]))
        a[pc][pc] = f(1)
        a[pc] = [v * scale for v in a[pc]]
        for r in range(3):
            if r != pc:
                factor = a[r][pc]
                a[r][pc] = f(0)
                a[r] = [a[r][c] - a[pc][c] * factor for c in range(3)]
    for pr, pc in reversed(done):
        if pr != pc:
            for r in range(3):
                a[r][pr], a[r][pc] = a[r][pc], a[r][pr]
    return [a[r][c] for r in range(3) for c in range(3)]


def interpolated_inverse(anim, time):
    """mInv of Interpolate(time) strictly between the transform times: Inverse(scale) * (ToTransform's un-transposed matrix *
    Translate(-trans)), row major."""
    f = anim.f
    time = f(time)
    assert anim.animated and anim.t0 < time < anim.t1
    dt = (time - anim.t0) / (anim.t1 - anim.t0)
    tr = [(f(1) - dt) * anim.T[0][i] + dt * anim.T[1][i] for i in range(3)]
    x, y, z, w = anim.slerp(dt)
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, x * w, y * w, z * w
    one, two, zero = f(1), f(2), f(0)
    q = [[one - two * (yy + zz), two * (xy + wz), two * (xz - wy), zero],
         [two * (xy - wz), one - two * (xx + zz), two * (yz + wx), zero],
         [two * (xz + wy), two * (yz - wx), one - two * (xx + yy), zero],
         [zero, zero, zero, one]]
    ti = [[one, zero, zero, -tr[0]], [zero, one, zero, -tr[1]], [zero, zero, one, -tr[2]], [zero, zero, zero, one]]
    sc = [[(f(1) - dt) * anim.S[0][3 * r + c] + dt * anim.S[1][3 * r + c] for c in range(3)] + [zero] for r in range(3)]
    sc.append([zero, zero, zero, one])
    m = cm._mul(cm._inverse(sc, f), cm._mul(q, ti))
    return [m[r][c] for r in range(4) for c in range(4)]


def animated_of(scene, k, f=np.float32):
    """The AnimatedTransform of moving instance k of a loaded scene."""
    inst = scene.desc.instances[k]
    assert inst.motion > 0
    mo = scene.desc.motions[inst.motion - 1]
    return cm.Animated(list(inst.i2w), list(mo.i2w_end), mo.transform_start, mo.transform_end, f)


def matrices_at(scene, k, time, f=np.float32, anim=None):
    """(InstanceToWorld, WorldToInstance) of instance k at `time` with Interpolate's boundary rules: the members bring their
    stored inverses. anim: animated_of(scene, k, f), where it is at hand."""
    inst = scene.desc.instances[k]
    mo = scene.desc.motions[inst.motion - 1]
    a = anim or animated_of(scene, k, f)
    time = f(time)
    if time <= a.t0:
        return [f(v) for v in inst.i2w], [f(v) for v in inst.w2i]
    if time >= a.t1:
        return [f(v) for v in mo.i2w_end], [f(v) for v in mo.w2i_end]
    return a.interpolate(time), interpolated_inverse(a, time)


def set_instance(scene, k, i2w, w2i):
    """Write a pair of matrices into instance k of the description (host memory): what the oracle then renders."""
    inst = scene.desc.instances[k]
    for i in range(16):
        inst.i2w[i] = float(np.float32(i2w[i]))
        inst.w2i[i] = float(np.float32(w2i[i]))


# ---------------------------------------------------------------------------------------------------------------------
def transform_bounds(m16, lo, hi, f=np.float32):
    """Transform::operator()(Bounds3f), transform.cpp:231-242: the union of the eight transformed corners."""
    m = [f(v) for v in m16]
    pts = []
    for cz in (lo[2], hi[2]):
        for cy in (lo[1], hi[1]):
            for cx in (lo[0], hi[0]):
                x, y, z = f(cx), f(cy), f(cz)
                p = [m[4 * r] * x + m[4 * r + 1] * y + m[4 * r + 2] * z + m[4 * r + 3] for r in range(4)]
                assert p[3] == 1
                pts.append(p[:3])
    pts = np.array(pts, np.float64 if f is np.float64 else np.float32)
    return pts.min(axis=0), pts.max(axis=0)


def world_bound(scene):
    n = scene.desc.nodes[0]
    return np.array(list(n.bmin), np.float32), np.array(list(n.bmax), np.float32)


def ramp_scene(delta, still=False, res=(64, 16), spp=125):
    """camera_motion.blur_scene restated for a moving object: a pinhole camera that stands still at z = 1 looking down -z
    (shutter 0..1), and a matte quad in the plane z = 0 whose edge travels along +x from -delta / 2 to delta / 2 between
    times 0 and 1, under a distant light along -z. maxdepth 1, box filter, Halton. still: the quad stays at the start."""
    quad = ('Material "matte" "rgb Kd" [.5 .5 .5]\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] '
            '"point P" [-50 -50 0  0 -50 0  0 50 0  -50 50 0]\n')
    x0, x1 = -delta / 2, delta / 2
    move = 'Translate %r 0 0\n' % x0 if still else pair('Translate %r 0 0' % x0, 'Translate %r 0 0' % x1)
    return ('%sFilm "image" "integer xresolution" [%d] "integer yresolution" [%d]\n'
            'PixelFilter "box" "float xwidth" [.5] "float ywidth" [.5]\n'
            'Sampler "halton" "integer pixelsamples" [%d]\nIntegrator "path" "integer maxdepth" [1]\nWorldBegin\n'
            'LightSource "distant" "point from" [0 0 1] "point to" [0 0 0] "rgb L" [3 3 3]\n'
            'AttributeBegin\n%s%sAttributeEnd\nWorldEnd\n'
            % (cm.static_camera("0 0 1  0 0 0  0 1 0", '"float fov" [90]'), res[0], res[1], spp, move, quad))


def two_movers(pair_a, pair_b, only=None):
    """Two ObjectInstances of one object under two CTM pairs (only: just that one of them, for telling their hits apart)."""
    out = 'ObjectBegin "mover"\n%s%sObjectEnd\n' % (MOVER_MATERIAL, OCTAHEDRON)
    for k, pr in enumerate((pair_a, pair_b)):
        if only is None or only == k:
            out += 'AttributeBegin\n%sObjectInstance "mover"\nAttributeEnd\n' % pair(*pr)
    return out


def moving_instances(scene):
    return [k for k in range(scene.desc.n_instances) if scene.desc.instances[k].motion > 0]


def set_moving(scene, twin, time, f=np.float32, anims=None):
    """Every moving instance of `twin` (a second load of `scene`) at the restatement of its matrices at `time`."""
    for k in moving_instances(scene):
        set_instance(twin, k, *matrices_at(scene, k, time, f, anims[k] if anims else None))


def expected_hits(ob, scene, twin, rays8, f=np.float32):
    """Per ray [n, 8] = o, d, tMax, time: (prim, depth, p) of the closest hit the oracle finds in `twin` (a second load of
    the scene) with every moving instance at the restatement, over scalar type f, of its matrices at the ray's time (rounded
    to float32 where f is float64: the oracle traces in float32)."""
    anims = {k: animated_of(scene, k, f) for k in moving_instances(scene)}
    prim, depth, p = np.zeros(len(rays8), np.int32), np.zeros(len(rays8), np.float32), np.zeros((len(rays8), 3), np.float32)
    for i, r in enumerate(rays8):
        set_moving(scene, twin, r[7], f, anims)
        a, b, c = cm.hit_values(ob, twin, r[None, :7])
        prim[i], depth[i], p[i] = a[0], b[0], c[0]
    return prim, depth, p


def rule_bar(v32, v64, both):
    """The project's bar for a family of outputs (test_camera_motion_gpu._ray_bars): four times the worst deviation of the
    float32 restatement from the float64 one over the queries both answer alike, never below 8 ulp of the largest value."""
    v32, v64 = np.asarray(v32, np.float64), np.asarray(v64, np.float64)
    if not np.any(both):
        return 0.0
    dev = float(np.abs(v32[both] - v64[both]).max())
    return max(4 * dev, 8 * float(np.spacing(np.float32(np.abs(v64[both]).max()))))


def grazing_rays(scene, origin, times, eps=(1e-3, 1e-2)):
    """Rays from `origin` at the silhouette of every moving instance's octahedron at each time: through its six vertices and
    twelve edge midpoints carried to the world by the float64 restatement, pulled in and pushed out of the hull by eps."""
    P = OCTAHEDRON_P.astype(np.float64)
    pts = list(P) + [(P[i] + P[j]) / 2 for i in range(6) for j in range(i + 1, 6) if np.dot(P[i], P[j]) == 0]
    assert len(pts) == 18
    rays = []
    o = np.asarray(origin, np.float64)
    for k in moving_instances(scene):
        anim = animated_of(scene, k, np.float64)
        for t in times:
            m = np.array(matrices_at(scene, k, t, np.float64, anim)[0], np.float64).reshape(4, 4)
            for q in pts:
                for e in eps:
                    for sign in (-1, 1):
                        w = (m @ np.append(q * (1 + sign * e), 1.0))[:3]
                        d = (w - o) / np.linalg.norm(w - o)
                        rays.append(list(o) + list(d) + [np.inf, t])
    return np.array(rays, np.float32)
