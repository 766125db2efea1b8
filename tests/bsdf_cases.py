"""Query sets for the BSDF tests (test_bsdf_gpu.py on the device, test_oracle_pins.py on the oracle): rows of eight float32 --
wo[3], wi[3], u[2] -- in the canonical shading frame (ns = ng = +z, ss = +x, ts = +y), seeded. No GPU, no library.

Every vector is normalised in float64 and then rounded to float32, except where a case says "exactly". Mode 0 of the probes
(BSDF::f, BSDF::Pdf) reads wo and wi, mode 1 (BSDF::Sample_f) reads wo and u, so one row serves both."""
import itertools

import numpy as np

MAX_BXDFS = 8   # MI_MAX_BXDFS

# BxDFType bits (MI_BSDF_*)
BSDF_REFLECTION, BSDF_TRANSMISSION, BSDF_DIFFUSE, BSDF_GLOSSY, BSDF_SPECULAR, BSDF_ALL = 1, 2, 4, 8, 16, 31
FLAGS = {
    "all": BSDF_ALL,
    "non-specular": BSDF_ALL & ~BSDF_SPECULAR,   # the value EstimateDirect passes
    "reflection": BSDF_ALL & ~BSDF_TRANSMISSION,
    "transmission": BSDF_ALL & ~BSDF_REFLECTION,
}


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _sphere(rng, n):
    z = rng.uniform(-1, 1, n)
    phi = rng.uniform(0, 2 * np.pi, n)
    s = np.sqrt(1 - z * z)
    return _unit(np.stack([s * np.cos(phi), s * np.sin(phi), z], 1))


def random_queries(n=2048, seed=20240531):
    """n (wo, wi, u): directions uniform over the sphere, u uniform over the unit square."""
    rng = np.random.default_rng(seed)
    return np.concatenate([_sphere(rng, n), _sphere(rng, n), rng.random((n, 2)).astype(np.float32)], 1)


def reflect_z(wo):
    """Reflect(wo, (0, 0, 1)) in float32, operation by operation as d_bsdf.h has it: -wo + 2 * Dot(wo, n) * n."""
    wo = np.asarray(wo, np.float32)
    zero, one, two = np.float32(0), np.float32(1), np.float32(2)
    dot = wo[0] * zero + wo[1] * zero + wo[2] * one
    k = two * dot
    return np.array([-wo[0] + k * zero, -wo[1] + k * zero, -wo[2] + k * one], np.float32)


def _edge_wo():
    """wo.z in {0 exactly, +-1e-7, +-1e-4, +-1e-3, +-0.5, +-1 exactly} at the azimuths 0 and pi / 2 (exactly on the x and y
    axes) and 0.3."""
    out = []
    for z in (0.0, 1e-7, -1e-7, 1e-4, -1e-4, 1e-3, -1e-3, .5, -.5, 1.0, -1.0):
        s = np.sqrt(1 - z * z)
        for az in ("x", .3, "y"):
            if az == "x":
                v = (s, 0.0, z)
            elif az == "y":
                v = (0.0, s, z)
            else:
                v = (s * np.cos(az), s * np.sin(az), z)
            w = np.array(v, np.float64).astype(np.float32)   # (already of length one in float64; z = 0 and |z| = 1 stay exact)
            if not any(np.array_equal(w, o) for o in out):
                out.append(w)
    return out


def _edge_u():
    """(0.5, 0.5): the origin of ConcentricSampleDisk; (0, 0); (1 - 2^-24, 1 - 2^-24); and u0 = k / ncomp exactly, with its two
    float neighbours, for every ncomp <= MAX_BXDFS -- where the component choice of Sample_f changes."""
    top = np.float32(1) - np.float32(2.0 ** -24)
    out = [(np.float32(.5), np.float32(.5)), (np.float32(0), np.float32(0)), (top, top)]
    seen = set()
    for n in range(1, MAX_BXDFS + 1):
        for k in range(n):
            b = np.float32(k) / np.float32(n)
            for v in (np.nextafter(b, np.float32(-1)), b, np.nextafter(b, np.float32(2))):
                if 0 <= v < 1 and float(v) not in seen:
                    seen.add(float(v))
                    out.append((v, np.float32(.37)))
    return out


def edge_queries(seed=7):
    """The cross product of the edge lists as either mode sees it, at most 2048 rows: every (wo, wi) pair and every (wo, u)
    pair occurs -- mode 0 does not read u and mode 1 does not read wi, so a row carries one of each: for a wo, row k takes
    u[k] and wi kind k mod 6. The wi kinds: Reflect(wo, z) computed as the device computes it, -wo (a zero half vector),
    (-wo.x, -wo.y, wo.z), a grazing direction, one in the lower hemisphere, a random one."""
    rng = np.random.default_rng(seed)
    us = _edge_u()
    rows = []
    for wo in _edge_wo():
        kinds = [reflect_z(wo), -wo, np.array([-wo[0], -wo[1], wo[2]], np.float32),
                 _unit([np.cos(1.1), np.sin(1.1), 1e-4]), _unit([.3, -.4, -.75])]
        for k, u in enumerate(us):
            wi = kinds[k % 6] if k % 6 < 5 else _sphere(rng, 1)[0]
            rows.append(np.concatenate([wo, wi, np.array(u, np.float32)]))
    q = np.unique(np.array(rows, np.float32).view(np.uint32), axis=0).view(np.float32)   # (bitwise: -0 and +0 are different rows)
    assert len(q) <= 2048
    return q


def all_queries():
    return np.concatenate([random_queries(), edge_queries()])


# ---- the straight-line form's retry (form 2 of the probe), one wave of 64 queries
# The quotients of the lobes an instance with the straight-line passes can hold are ((R a) b) c / d with d = 4 cos_o cos_i of a
# microfacet reflection (or |cos| of a specular lobe). With a divisor inside DivBy's fast range (1e-18 < |d| < 1e18) no material
# of the catalogue reaches a quotient outside (1e-30, 1e30): D G F R / d stays below 1e12 / 1e-18 and, for a non-zero
# numerator, above 1e-12 / 4. What does leave the range is the divisor: both directions within 4e-10 of the horizon give
# 4 cos_o cos_i = 6.4e-19 < 1e-18, the lane's tracker starts out of range (DivTrack::Reset) and the wave redoes the quad.
RETRY_LANE = 17
RETRY_WO = (1.0, 0.0, 4e-10)    # (of length one in float32 as they stand)
RETRY_WI = (-1.0, 0.0, 4e-10)


def retry_waves(seed=99):
    """(wave with the lane, wave without): 64 queries each in mode 0. The other lanes: wo and wi in the upper hemisphere, at
    least 0.05 above the horizon (divisors and quotients well inside the range). The second wave has, in the lane's place, a
    wi below the surface: no reflection lobe contributes, the lane's slots are unused (A = 0, d = 1) and its only quotients
    are exact zeros."""
    rng = np.random.default_rng(seed)

    def upper(n):
        v = _sphere(rng, n).astype(np.float64)
        v[:, 2] = np.abs(v[:, 2]) * .95 + .05
        return _unit(v)

    wave = np.concatenate([upper(64), upper(64), rng.random((64, 2)).astype(np.float32)], 1)
    hit, calm = wave.copy(), wave.copy()
    hit[RETRY_LANE, :3] = np.array(RETRY_WO, np.float32)
    hit[RETRY_LANE, 3:6] = np.array(RETRY_WI, np.float32)
    calm[RETRY_LANE, 5] = -calm[RETRY_LANE, 5]
    return hit, calm
