"""Camera "orthographic" and Camera "environment" restated in numpy (MIPT_CAMERAS=all), for test_camera_models_restatement.py,
test_cameras_frontend.py and test_cameras_gpu.py.

  OrthographicCamera::GenerateRayDifferential                    src/cameras/orthographic.cpp:70-121
  EnvironmentCamera::GenerateRay (the fork's omnistereo camera)  src/cameras/environment.cpp:43-105
  Camera::GenerateRayDifferential (the base class's offset rays) src/core/camera.cpp:60-99
  Transform::operator()(Ray / RayDifferential)                   src/core/transform.h:251-281
  RayDifferential::ScaleDifferentials                            src/core/geometry.h:917-922

Written once over a scalar type: np.float32 follows the reference's float operation order with libm calls correctly rounded
(as the device evaluates them), np.float64 is the same mathematics in double from the same float32 inputs -- the camera
record, the sample values and the float32 constants Pi, Pi/2 and .05f are data. The unchanged oracle knows the perspective
camera only: it is given a *twin* (the same text with Camera "perspective") for sampler values and for tracing restated rays.

Every routine takes arrays of n samples and returns arrays of the scalar type. `branch` (environment) names the path a sample
took through the comparisons of the omnistereo code, so that a test can set aside the samples on which the two restatements
disagree: bit 0 altitude > poleMergeTo, bit 1 fading, bit 2 d == up."""
import re

import numpy as np

import camera_motion as cm

ORTHOGRAPHIC, ENVIRONMENT = 2, 3
PI32, PI_OVER_2_32, PI_OVER_4_32 = np.float32(3.14159265358979323846), np.float32(1.57079632679489661923), np.float32(0.78539816339744830961)
EPS32 = np.float32(.05)


def _libm(fn, x, f):
    """A float libm call, correctly rounded: evaluated in double and rounded once."""
    with np.errstate(invalid="ignore"):   # (the branch not taken of a np.where: 0 / 0 of equal pole-merge angles)
        return fn(np.asarray(x, np.float64)).astype(f)


def _normalize(v):
    """Normalize(v) = v / v.Length(), a vector divided by a float multiplying by the reciprocal (geometry.h:245-249)."""
    f = v.dtype.type
    length = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = f(1) / length
        return v * inv[:, None]


def _cross(a, b):
    """Cross in double, rounded to the scalar type (geometry.h:966-972)."""
    f = a.dtype.type
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    return np.stack([a64[:, 1] * b64[:, 2] - a64[:, 2] * b64[:, 1], a64[:, 2] * b64[:, 0] - a64[:, 0] * b64[:, 2],
                     a64[:, 0] * b64[:, 1] - a64[:, 1] * b64[:, 0]], axis=1).astype(f)


def _gamma3(f):
    eps = np.float32(2.0 ** -24)
    return f((np.float32(3) * eps) / (np.float32(1) - np.float32(3) * eps))


def _matrices(m, n, f):
    """[n, 4, 4] of the scalar type from one 16-vector or n of them."""
    m = np.asarray(m, np.float64)
    if m.ndim == 1:
        m = np.tile(m, (n, 1))
    return m.reshape(n, 4, 4).astype(f)


def xf_point(M, p):
    """Transform::operator()(Point3f) of an affine matrix (w = 1), and its absolute error bound (transform.h:199-231)."""
    f = p.dtype.type
    out, err = [], []
    for r in range(3):
        a, b, c, t = M[:, r, 0] * p[:, 0], M[:, r, 1] * p[:, 1], M[:, r, 2] * p[:, 2], M[:, r, 3]
        out.append(a + b + c + t)
        err.append(_gamma3(f) * (np.abs(a) + np.abs(b) + np.abs(c) + np.abs(t)))
    return np.stack(out, axis=1), np.stack(err, axis=1)


def xf_vector(M, v):
    return np.stack([M[:, r, 0] * v[:, 0] + M[:, r, 1] * v[:, 1] + M[:, r, 2] * v[:, 2] for r in range(3)], axis=1)


def xf_ray(M, o, d, t_max):
    """Transform::operator()(Ray): the origin moves along d by its error bound, tMax shrinks by the same dt."""
    p, err = xf_point(M, o)
    v = xf_vector(M, d)
    l2 = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        dt = (np.abs(v[:, 0]) * err[:, 0] + np.abs(v[:, 1]) * err[:, 1] + np.abs(v[:, 2]) * err[:, 2]) / l2
    move = l2 > 0
    dt = np.where(move, dt, 0).astype(p.dtype)
    return np.where(move[:, None], p + v * dt[:, None], p), v, np.where(move, t_max - dt, t_max)


def concentric_sample_disk(u, f):
    """ConcentricSampleDisk, sampling.cpp:113-130."""
    u = np.asarray(u, np.float32).astype(f)
    ox, oy = f(2) * u[:, 0] - f(1), f(2) * u[:, 1] - f(1)
    wide = np.abs(ox) > np.abs(oy)
    with np.errstate(divide="ignore", invalid="ignore"):
        theta = np.where(wide, f(PI_OVER_4_32) * (oy / ox), f(PI_OVER_2_32) - f(PI_OVER_4_32) * (ox / oy))
    r = np.where(wide, ox, oy)
    theta = np.where((ox == 0) & (oy == 0), 0, theta).astype(f)
    out = np.stack([r * _libm(np.cos, theta, f), r * _libm(np.sin, theta, f)], axis=1)
    out[(ox == 0) & (oy == 0)] = 0
    return out


class Camera:
    """The fields of a scene's description the two cameras read."""

    def __init__(self, scene):
        d = scene.desc
        c = d.camera
        self.kind = int(d.camera_type)
        self.raster_to_camera = [float(v) for v in c.raster_to_camera]
        self.camera_to_world = [float(v) for v in c.camera_to_world]
        self.lens_radius, self.focal_distance = np.float32(c.lens_radius), np.float32(c.focal_distance)
        self.shutter = (np.float32(c.shutter_open), np.float32(c.shutter_close))
        self.full_res = (int(d.film.full_res[0]), int(d.film.full_res[1]))
        self.ipd, self.merge_to = np.float32(d.env_ipd), np.float32(d.env_pole_merge_to)
        self.merge_from, self.convergence = np.float32(d.env_pole_merge_from), np.float32(d.env_convergence_distance)
        self.scale = np.float32(1) / np.sqrt(np.float32(d.sampler.samples_per_pixel))   # ScaleDifferentials(1 / sqrt(spp))
        self.animated = bool(c.animated)
        self._anim = {}
        self._scene = scene

    def times(self, time_u):
        """Lerp(u, shutterOpen, shutterClose), float32 (orthographic.cpp:64, environment.cpp:54)."""
        u = np.asarray(time_u, np.float32)
        return (np.float32(1) - u) * self.shutter[0] + u * self.shutter[1]

    def camera_to_world_at(self, times, f):
        """[n, 4, 4]: CameraToWorld at each ray's time (camera_motion.Animated for an animated pair)."""
        n = len(times)
        if not self.animated:
            return _matrices(self.camera_to_world, n, f)
        if f not in self._anim:
            self._anim[f] = cm.animated_of(self._scene, f)
        return _matrices(np.array([[float(v) for v in self._anim[f].interpolate(t)] for t in times]), n, f)


def _scaled(o, d, rx_o, ry_o, rx_d, ry_d, scale):
    return [o + (rx_o - o) * scale, o + (ry_o - o) * scale, d + (rx_d - d) * scale, d + (ry_d - d) * scale]


def orthographic(cam, p_film, p_lens, time_u, f=np.float32):
    """OrthographicCamera::GenerateRayDifferential, CameraToWorld, ScaleDifferentials: dict(o, d, t_max, time, weight, diffs)."""
    p_film = np.asarray(p_film, np.float32)
    n = len(p_film)
    times = cam.times(time_u)
    C2W, R2C = cam.camera_to_world_at(times, f), _matrices(cam.raster_to_camera, n, f)
    pf = np.concatenate([p_film.astype(f), np.zeros((n, 1), f)], axis=1)
    p_camera, _ = xf_point(R2C, pf)
    dx_camera = xf_vector(R2C, np.tile(np.array([1, 0, 0], f), (n, 1)))
    dy_camera = xf_vector(R2C, np.tile(np.array([0, 1, 0], f), (n, 1)))
    z = np.tile(np.array([0, 0, 1], f), (n, 1))
    o, d = p_camera, z
    if cam.lens_radius > 0:
        p_lens2 = f(cam.lens_radius) * concentric_sample_disk(p_lens, f)
        ft = f(cam.focal_distance) / d[:, 2]
        p_focus = o + d * ft[:, None]
        o = np.concatenate([p_lens2, np.zeros((n, 1), f)], axis=1)      # the lens point alone
        d = _normalize(p_focus - o)
        ft = f(cam.focal_distance) / d[:, 2]                              # a second time, from the direction the lens changed
        rx_o = ry_o = o
        rx_d = _normalize(((p_camera + dx_camera) + ft[:, None] * z) - rx_o)
        ry_d = _normalize(((p_camera + dy_camera) + ft[:, None] * z) - ry_o)
    else:
        rx_o, ry_o, rx_d, ry_d = o + dx_camera, o + dy_camera, d, d
    wo, wd, t_max = xf_ray(C2W, o, d, np.full(n, np.inf, f))
    diffs = _scaled(wo, wd, xf_point(C2W, rx_o)[0], xf_point(C2W, ry_o)[0], xf_vector(C2W, rx_d), xf_vector(C2W, ry_d), f(cam.scale))
    return dict(o=wo, d=wd, t_max=t_max, time=times, weight=np.ones(n, f), diffs=diffs, branch=np.zeros(n, np.int32),
                p_camera=p_camera, dx_camera=dx_camera, dy_camera=dy_camera, camera_o=o, camera_d=d)


def environment_camera_ray(cam, p_film, f=np.float32):
    """EnvironmentCamera::GenerateRay up to CameraToWorld: (o, d, branch, offset) in camera space."""
    p_film = np.asarray(p_film, np.float32).astype(f)
    n = len(p_film)
    theta = f(PI32) * p_film[:, 1] / f(cam.full_res[1])
    phi = f(2) * f(PI32) * p_film[:, 0] / f(cam.full_res[0])
    sin_t, cos_t = _libm(np.sin, theta, f), _libm(np.cos, theta, f)
    d = np.stack([sin_t * _libm(np.cos, phi, f), cos_t, sin_t * _libm(np.sin, phi, f)], axis=1)    # y and z swapped: y is up
    o = np.zeros((n, 3), f)
    branch = np.zeros(n, np.int32)
    offset = np.full(n, f(cam.ipd), f)
    if cam.ipd != 0:
        if cam.merge_to > 0:
            altitude = np.abs(_libm(np.arcsin, d[:, 2], f))              # radians, from the swapped direction's z
            beyond = altitude > f(cam.merge_to)                           # against the parameter as given
            fading = ~beyond & (altitude > f(cam.merge_from))
            with np.errstate(divide="ignore", invalid="ignore"):
                fac = (altitude - f(cam.merge_from)) / (f(cam.merge_to) - f(cam.merge_from))
            fade = _libm(np.cos, fac * f(PI_OVER_2_32), f)
            offset = np.where(beyond, f(0), np.where(fading, offset * fade, offset)).astype(f)
            branch |= beyond.astype(np.int32) | (fading.astype(np.int32) << 1)
        up = np.tile(np.array([0, 1, 0], f), (n, 1))
        is_up = np.all(d == up, axis=1)
        side = np.where(is_up[:, None], f(0), _normalize(_cross(d, up))).astype(f)
        branch |= is_up.astype(np.int32) << 2
        stereo = side * offset[:, None]
        o = o + stereo
        if np.isfinite(cam.convergence):
            d = _normalize(f(cam.convergence) * d - stereo)
    return o, d, branch, offset


def environment(cam, p_film, p_lens, time_u, f=np.float32):
    """Camera::GenerateRayDifferential over EnvironmentCamera::GenerateRay, then ScaleDifferentials."""
    p_film = np.asarray(p_film, np.float32)
    n = len(p_film)
    times = cam.times(time_u)
    C2W = cam.camera_to_world_at(times, f)
    inf = np.full(n, np.inf, f)
    co, cd, branch, offset = environment_camera_ray(cam, p_film, f)
    o, d, t_max = xf_ray(C2W, co, cd, inf)
    inv_eps = f(1) / f(EPS32)
    shifted = []
    for axis in (0, 1):
        q = p_film.copy()
        q[:, axis] = q[:, axis] + EPS32                                   # sshift.pFilm += eps, in float32
        so, sd, sb, _ = environment_camera_ray(cam, q, f)
        branch = branch | (sb << (3 * (axis + 1)))
        ro, rd, _ = xf_ray(C2W, so, sd, inf)
        shifted.append((o + (ro - o) * inv_eps, d + (rd - d) * inv_eps))
    diffs = _scaled(o, d, shifted[0][0], shifted[1][0], shifted[0][1], shifted[1][1], f(cam.scale))
    return dict(o=o, d=d, t_max=t_max, time=times, weight=np.ones(n, f), diffs=diffs, branch=branch, camera_o=co, camera_d=cd, offset=offset)


def generate(cam, p_film, p_lens, time_u, f=np.float32):
    return (orthographic if cam.kind == ORTHOGRAPHIC else environment)(cam, p_film, p_lens, time_u, f)


def both(cam, p_film, p_lens, time_u):
    """(r32, r64, unsure): the two restatements and the samples on which they took different branches."""
    r32, r64 = generate(cam, p_film, p_lens, time_u, np.float32), generate(cam, p_film, p_lens, time_u, np.float64)
    return r32, r64, r32["branch"] != r64["branch"]


def columns(r):
    """The 21 columns of mi_pt_camera_rays_ex: o, d, tMax, time, weight, rxOrigin, ryOrigin, rxDirection, ryDirection."""
    return np.concatenate([r["o"], r["d"], r["t_max"][:, None], r["time"][:, None].astype(r["o"].dtype), r["weight"][:, None]] + r["diffs"], axis=1)


def bar(a32, a64, sel):
    """disk_shape.bar: four times the worst float32-against-float64 deviation over the selected queries, never below 8 ulp
    (float32) of the largest component."""
    a, b = np.asarray(a32)[sel].astype(np.float64), np.asarray(a64)[sel]
    if a.size == 0:
        return 0.0
    return float(max(4 * np.abs(a - b).max(), 8 * float(np.spacing(np.float32(np.abs(b).max())))))


# ---------------------------------------------------------------------------------------------------------------------
# scenes and sampler values
def twin_text(text):
    """The same scene behind Camera "perspective": what the unchanged oracle is given (sampler values, ob.trace)."""
    out, n = re.subn(r'Camera "(orthographic|environment)"', 'Camera "perspective"', text)
    assert n == 1
    return out


def pair(pt, text, **kw):
    """(scene, twin): loaded with and without the camera; the switch must be set in the environment by the caller."""
    s, twin = pt.Scene(text=text, **kw), pt.Scene(text=twin_text(text), **kw)
    assert s.errors == [] and twin.errors == [], (s.errors, twin.errors)
    assert s.desc.camera_type in (ORTHOGRAPHIC, ENVIRONMENT) and twin.desc.camera_type == 0
    assert list(s.desc.film.sample_bounds) == list(twin.desc.film.sample_bounds) and s.spp == twin.spp
    return s, twin


def all_samples(scene):
    sb = list(scene.desc.film.sample_bounds)
    return [(px, py, n) for py in range(sb[1], sb[3]) for px in range(sb[0], sb[2]) for n in range(scene.spp)]


def sample_values(ob, twin, samples):
    """(p_film [n, 2], time_u [n], p_lens [n, 2]) of GetCameraSample (sampler.cpp:46-52) from the oracle's sampler: dimensions
    0, 1 (film offset), 2 (time), 3, 4 (lens)."""
    fn = ob.lib().oracle_sample_dimension
    with ob.exact_libm():
        u = np.array([[fn(twin.desc_ptr, int(px), int(py), int(n), k) for k in range(5)] for px, py, n in samples], np.float32)
    xy = np.array([(px, py) for px, py, _ in samples], np.float32)
    return xy + u[:, 0:2], u[:, 2].copy(), u[:, 3:5].copy()
