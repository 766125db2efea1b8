"""Helpers of the realistic-camera tests (test_realistic_frontend.py, test_realistic_gpu.py).

The reference's lens camera (src/cameras/realistic.cpp) restated in numpy over a scalar type, vectorised over rays:
np.float32 follows the reference's float operation order, np.float64 is the same mathematics in double and gives the bars.
Both take the element table, the exit-pupil boxes and the film data from the scene's mi_lens, and a camera sample's five
values from the unchanged oracle's sampler. Beside each function: the reference lines it restates."""
import ctypes as C
import os

import numpy as np

import camera_motion as cm

LENS_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lenses")
_EPS = np.float32(2.0 ** -24)
GAMMA3 = (np.float32(3) * _EPS) / (np.float32(1) - np.float32(3) * _EPS)    # gamma(3), pbrt.h:292-294


def lens_path(name):
    return os.path.join(LENS_DIR, name)


class Lens:
    """The scene's mi_lens as arrays of scalar type f."""

    def __init__(self, scene, f=np.float32):
        c = scene.desc.camera
        assert scene.desc.camera_type == 1 and bool(scene.desc.lens)
        L = scene.desc.lens.contents
        self.f = f
        self.n = int(L.n_elements)
        self.el = np.array([[L.elements[i][k] for k in range(4)] for i in range(self.n)], np.float32).astype(f)
        self.boxes = np.array([[L.exit_pupil_bounds[i][k] for k in range(4)] for i in range(64)], np.float32).astype(f)
        self.extent = np.array(list(L.physical_extent), np.float32).astype(f)
        self.diagonal = f(np.float32(L.film_diagonal))
        self.full_res = (int(L.full_res[0]), int(L.full_res[1]))
        self.simple = bool(L.simple_weighting)
        self.ca = bool(L.chromatic_aberration)
        self.shutter = (f(np.float32(c.shutter_open)), f(np.float32(c.shutter_close)))
        self.rear_z = self.el[self.n - 1, 1]


def _flip_z(o, d, f):
    """Transform::operator()(Ray) with Scale(1, 1, -1), transform.h:247-266: the mirrored ray, its origin moved along the
    direction by the origin's error bound (gamma(3) is the float32 constant in both scalar types: it is part of the method)."""
    g = f(GAMMA3)
    oz, dz = f(-1) * o[:, 2], f(-1) * d[:, 2]
    ex, ey, ez = g * np.abs(o[:, 0]), g * np.abs(o[:, 1]), g * np.abs(oz)
    l2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + dz * dz
    with np.errstate(divide="ignore", invalid="ignore"):
        dt = np.where(l2 > 0, (np.abs(d[:, 0]) * ex + np.abs(d[:, 1]) * ey + np.abs(dz) * ez) / l2, f(0))
    no = np.stack([o[:, 0] + d[:, 0] * dt, o[:, 1] + d[:, 1] * dt, oz + dz * dt], 1)
    return no, np.stack([d[:, 0], d[:, 1], dz], 1)


def _normalize(v, f):
    """Normalize: v / Length() multiplies by the reciprocal (geometry.h:245-249)."""
    inv = f(1) / np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    return v * inv[:, None]


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _spherical(radius, z_center, o, d, f):
    """IntersectSphericalElement, realistic.cpp:372-392 with Quadratic, pbrt.h:422-438 (its roots in double)."""
    oc = o.copy()
    oc[:, 2] = o[:, 2] - z_center
    A = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    B = f(2) * (d[:, 0] * oc[:, 0] + d[:, 1] * oc[:, 1] + d[:, 2] * oc[:, 2])
    Cc = oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1] + oc[:, 2] * oc[:, 2] - radius * radius
    a64, b64, c64 = A.astype(np.float64), B.astype(np.float64), Cc.astype(np.float64)
    disc = b64 * b64 - 4.0 * a64 * c64
    ok = disc >= 0
    with np.errstate(divide="ignore", invalid="ignore"):
        root = np.sqrt(np.where(ok, disc, 0.0))
        q = np.where(b64 < 0, -.5 * (b64 - root), -.5 * (b64 + root))
        t0, t1 = (q / a64).astype(f), (c64 / q).astype(f)
    lo, hi = np.minimum(t0, t1), np.maximum(t0, t1)
    closer = (d[:, 2] > 0) ^ bool(radius < 0)
    t = np.where(closer, lo, hi)
    ok = ok & ~(t < 0) & ~np.isnan(t)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        n = _normalize(oc + t[:, None] * d, f)
        n = np.where((_dot(n, -d) < 0)[:, None], -n, n)   # Faceforward
    return ok, t, n


def _refract(wi, n, eta, f):
    """Refract, reflection.h:92-106."""
    cos_i = _dot(n, wi)
    sin2_i = np.maximum(f(0), f(1) - cos_i * cos_i)
    sin2_t = eta * eta * sin2_i
    ok = ~(sin2_t >= 1)
    with np.errstate(invalid="ignore"):
        cos_t = np.sqrt(f(1) - sin2_t)
    wt = eta * -wi + ((eta * cos_i - cos_t)[:, None]) * n
    return ok, wt


def _eta_shift(eta, wavelength, f):
    """realistic.cpp:352-358: `(wavelength - 550) * -.04 / (300) + eta`, a double expression rounded to Float."""
    if eta == 1:
        return eta
    return f(np.float64(f(wavelength) - f(550)) * -.04 / 300 + np.float64(eta))


def trace_from_film(lens, o, d, wavelength=550.0):
    """TraceLensesFromFilm, realistic.cpp:302-370 -> (through [n], o [n, 3], d [n, 3]) in camera space."""
    f = lens.f
    o, d = _flip_z(np.asarray(o, f), np.asarray(d, f), f)
    alive = np.ones(len(o), bool)
    element_z = f(0)
    ca = lens.ca and 400 <= wavelength <= 700
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(lens.n - 1, -1, -1):
            radius, thickness, eta, aperture = lens.el[i]
            element_z = element_z - thickness
            if radius == 0:
                ok = ~(d[:, 2] >= 0)
                t = (element_z - o[:, 2]) / d[:, 2]
                ok &= t >= 0
                n = None
            else:
                ok, t, n = _spherical(radius, element_z + radius, o, d, f)
            p = o + d * t[:, None]
            r2 = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]
            ok &= ~(r2 > aperture * aperture)
            alive &= ok
            o = np.where(alive[:, None], p, o)
            if radius != 0:
                eta_i = eta
                eta_t = lens.el[i - 1, 2] if (i > 0 and lens.el[i - 1, 2] != 0) else f(1)
                if ca:
                    eta_i, eta_t = _eta_shift(eta_i, wavelength, f), _eta_shift(eta_t, wavelength, f)
                ok, w = _refract(_normalize(-d, f), n, eta_i / eta_t, f)
                alive &= ok
                d = np.where(alive[:, None], w, d)
    o, d = _flip_z(o, d, f)
    return alive, o, d


def trace_from_scene(lens, o, d):
    """TraceLensesFromScene, realistic.cpp:394-442 (with the table as it stands: call it on an unfocused Lens to restate
    ComputeThickLensApproximation)."""
    f = lens.f
    o, d = _flip_z(np.asarray(o, f), np.asarray(d, f), f)
    alive = np.ones(len(o), bool)
    front = f(0)
    for i in range(lens.n):
        front = front + lens.el[i, 1]
    element_z = -front
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for i in range(lens.n):
            radius, thickness, eta, aperture = lens.el[i]
            if radius == 0:
                t = (element_z - o[:, 2]) / d[:, 2]
                ok = t >= 0
                n = None
            else:
                ok, t, n = _spherical(radius, element_z + radius, o, d, f)
            p = o + d * t[:, None]
            ok &= ~(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1] > aperture * aperture)
            alive &= ok
            o = np.where(alive[:, None], p, o)
            if radius != 0:
                eta_i = f(1) if (i == 0 or lens.el[i - 1, 2] == 0) else lens.el[i - 1, 2]
                eta_t = eta if eta != 0 else f(1)
                ok, w = _refract(_normalize(-d, f), n, eta_i / eta_t, f)
                alive &= ok
                d = np.where(alive[:, None], w, d)
            element_z = element_z + thickness
    o, d = _flip_z(o, d, f)
    return alive, o, d


def _lerp(t, a, b, f):
    return (f(1) - t) * a + t * b


def generate_ray(lens, c2w, p_film, p_lens, wavelength=550.0):
    """RealisticCamera::GenerateRay, realistic.cpp:899-932, with SampleExitPupil, 832-851: p_film [n, 2] raster positions,
    p_lens [n, 2] -> (weight [n], o [n, 3], d [n, 3] in world space through the row-major c2w). Weight 0: vignetted."""
    f = lens.f
    p_film, p_lens = np.asarray(p_film, np.float32).astype(f), np.asarray(p_lens, np.float32).astype(f)
    sx, sy = p_film[:, 0] / f(lens.full_res[0]), p_film[:, 1] / f(lens.full_res[1])
    fx = _lerp(sx, lens.extent[0], lens.extent[2], f)
    fy = _lerp(sy, lens.extent[1], lens.extent[3], f)
    px, py = -fx, fy
    r_film = np.sqrt(px * px + py * py)
    r_index = np.minimum(63, (r_film / (lens.diagonal / f(2)) * f(64)).astype(np.int64))
    box = lens.boxes[r_index]
    area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
    lx, ly = _lerp(p_lens[:, 0], box[:, 0], box[:, 2], f), _lerp(p_lens[:, 1], box[:, 1], box[:, 3], f)
    with np.errstate(invalid="ignore", divide="ignore"):
        sin_t = np.where(r_film != 0, py / r_film, f(0))
        cos_t = np.where(r_film != 0, px / r_film, f(1))
    p_rear = np.stack([cos_t * lx - sin_t * ly, sin_t * lx + cos_t * ly, np.full(len(px), lens.rear_z, f)], 1)
    o = np.stack([px, py, np.zeros(len(px), f)], 1)
    d = p_rear - o
    ok, lo, ld = trace_from_film(lens, o, d, wavelength)
    wo, wd = np.zeros_like(lo), np.zeros_like(ld)
    for i in np.nonzero(ok)[0]:
        a, b, _ = cm.transform_ray(c2w, lo[i], ld[i], np.inf, f)
        wo[i], wd[i] = a, b
    with np.errstate(invalid="ignore", divide="ignore"):
        wd = _normalize(wd, f)
    cos_theta = _normalize(d, f)[:, 2]
    cos4 = (cos_theta * cos_theta) * (cos_theta * cos_theta)
    if lens.simple:
        b0 = lens.boxes[0]
        w = cos4 * area / ((b0[2] - b0[0]) * (b0[3] - b0[1]))
    else:
        w = (lens.shutter[1] - lens.shutter[0]) * (cos4 * area) / (lens.rear_z * lens.rear_z)
    return np.where(ok, w, f(0)), wo, wd


def generate_ray_differential(lens, c2w, p_film, p_lens, wavelength=550.0, scale=1.0):
    """Camera::GenerateRayDifferential, camera.cpp:60-99, then ScaleDifferentials(scale), geometry.h:917-922 ->
    (weight, o, d, [rxOrigin, ryOrigin, rxDirection, ryDirection])."""
    f = lens.f
    p_film = np.asarray(p_film, np.float32)
    w, o, d = generate_ray(lens, c2w, p_film, p_lens, wavelength)
    out_w = w.copy()
    diffs = []
    for axis in (0, 1):
        got = np.zeros(len(w), bool)
        ro, rd = np.zeros_like(o), np.zeros_like(d)
        for eps in (np.float32(.05), np.float32(-.05)):
            shifted = p_film.copy()
            shifted[:, axis] = shifted[:, axis] + eps
            wx, xo, xd = generate_ray(lens, c2w, shifted, p_lens, wavelength)
            take = ~got & (wx != 0)
            inv = f(1) / f(eps)
            ro[take] = (o + (xo - o) * inv)[take]
            rd[take] = (d + (xd - d) * inv)[take]
            got |= take
        out_w = np.where(got, out_w, f(0))
        diffs.append((ro, rd))
    s = f(np.float32(scale))
    (rxo, rxd), (ryo, ryd) = diffs
    scaled = [o + (rxo - o) * s, o + (ryo - o) * s, d + (rxd - d) * s, d + (ryd - d) * s]
    return out_w, o, d, scaled


def band_wavelength(n_bands, band):
    """spectralpath.cpp:234-267: sampledLambdaStart + deltaWaveCA * s + deltaWaveCA / 2 in float, with sampledLambdaStart =
    395 and deltaWave = (705 - 395) / 31 = 10 (integer division of the three int constants, spectrum.h:48-50)."""
    delta_index = int(np.round(np.float32(31) / np.float32(n_bands)))
    delta = np.float32(10) * np.float32(delta_index)
    return float(np.float32(395) + delta * np.float32(band) + delta / np.float32(2))


def radical_inverse_2_3(n):
    """RadicalInverse(0, i) and RadicalInverse(1, i) for i < n (lowdiscrepancy.cpp:389-424 over 40-58) in float32."""
    i = np.arange(n, dtype=np.uint64)
    rev = np.zeros(n, np.uint64)
    for b in range(64):
        rev |= ((i >> np.uint64(b)) & np.uint64(1)) << np.uint64(63 - b)
    u0 = (rev.astype(np.float64) * 5.4210108624275222e-20).astype(np.float32)
    inv_base = np.float32(1) / np.float32(3)
    a, digits, inv_n = i.copy(), np.zeros(n, np.uint64), np.ones(n, np.float32)
    while a.any():
        live = a != 0
        nxt = a // np.uint64(3)
        digits = np.where(live, digits * np.uint64(3) + (a - nxt * np.uint64(3)), digits)
        inv_n = np.where(live, inv_n * inv_base, inv_n)
        a = nxt
    u1 = np.minimum(digits.astype(np.float32) * inv_n, np.float32(1) - np.float32(2.0 ** -24))
    return u0, u1


def exit_pupil_points(lens, interval, n=1024 * 1024):
    """The film points and rear-plane points BoundExitPupil tries for one radial interval (realistic.cpp:753-770), always
    placed in float32 -- both restatements trace the same rays -- and which of them get through in the scalar type of `lens`:
    (through [n], pRear [n, 2] float32, sample spacing)."""
    f32 = np.float32
    diag = f32(lens.diagonal)
    r0 = f32(interval) / f32(64) * diag / f32(2)
    r1 = f32(interval + 1) / f32(64) * diag / f32(2)
    rear_radius = f32(lens.el[lens.n - 1, 3])
    lo, hi = f32(-1.5) * rear_radius, f32(1.5) * rear_radius
    t = (np.arange(n, dtype=np.float32) + f32(0.5)) / f32(n)
    x = (f32(1) - t) * r0 + t * r1
    u0, u1 = radical_inverse_2_3(n)
    rx, ry = (f32(1) - u0) * lo + u0 * hi, (f32(1) - u1) * lo + u1 * hi
    o = np.stack([x, np.zeros(n, f32), np.zeros(n, f32)], 1)
    p = np.stack([rx, ry, np.full(n, f32(lens.rear_z), f32)], 1)
    ok = np.zeros(n, bool)
    for a in range(0, n, 1 << 18):
        b = a + (1 << 18)
        ok[a:b] = trace_from_film(lens, o[a:b], (p - o)[a:b])[0]
    side = hi - lo
    spacing = float(f32(2) * np.sqrt(side * side + side * side) / f32(1024))
    return ok, p[:, :2], spacing


def box_of(points, through, lens):
    """BoundExitPupil's box of the points that got through (realistic.cpp:771-789), expanded; the whole projected rear
    bounds when none did."""
    f32 = np.float32
    rear_radius = f32(lens.el[lens.n - 1, 3])
    lo, hi = f32(-1.5) * rear_radius, f32(1.5) * rear_radius
    if not through.any():
        return np.array([lo, lo, hi, hi], f32)
    side = hi - lo
    delta = f32(2) * np.sqrt(side * side + side * side) / f32(1024)
    p = points[through]
    return np.array([p[:, 0].min() - delta, p[:, 1].min() - delta, p[:, 0].max() + delta, p[:, 1].max() + delta], f32)


# ---------------------------------------------------------------------------------------------------------------------
# Scene texts and camera samples
def camera_block(lens, lookat="0 0 5  0 0 0  0 1 0", params=""):
    return 'LookAt %s\nCamera "realistic" "string lensfile" "%s" %s\n' % (lookat, lens_path(lens), params)


def camera_samples(ob, scene, samples):
    """GetCameraSample's five values of each (px, py, n) from the oracle's sampler (sampler.cpp:46-52: pFilm = pixel +
    Get2D, time = Get1D, pLens = Get2D) -> (pFilm [n, 2], time sample [n], pLens [n, 2]) in float32."""
    lib = cm._bind(ob)
    out = np.zeros(6, np.float32)
    p_film, tu, p_lens = np.zeros((len(samples), 2), np.float32), np.zeros(len(samples), np.float32), np.zeros((len(samples), 2), np.float32)
    for i, (px, py, n) in enumerate(samples):
        lib.oracle_sampler_calls(scene.desc_ptr, int(px), int(py), int(n), 2, out.ctypes.data_as(C.POINTER(C.c_float)))
        p_film[i] = (np.float32(px) + out[0], np.float32(py) + out[1])
        tu[i] = out[2]
        p_lens[i] = (out[3], out[4])
    return p_film, tu, p_lens


def restate(scene, ob, samples, f=np.float32, band=None):
    """The restated GenerateRayDifferential of the listed samples (static camera: CameraToWorld is the start member) ->
    dict(weight, o, d, diffs [4], p_film)."""
    lens = Lens(scene, f)
    p_film, _, p_lens = camera_samples(ob, scene, samples)
    nb = int(scene.desc.integrator.n_ca_bands)
    wl = 550.0 if band is None or nb <= 1 else band_wavelength(nb, band)
    scale = np.float32(1) / np.sqrt(np.float32(scene.spp))
    w, o, d, diffs = generate_ray_differential(lens, list(scene.desc.camera.camera_to_world), p_film, p_lens, wl, scale)
    return dict(weight=w, o=o, d=d, diffs=diffs, p_film=p_film, wavelength=wl)
