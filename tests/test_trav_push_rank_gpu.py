"""k_trav's push step on a wide-4 record (OpenNode<4>): the hit children that are not taken go to the stack place their
visiting rank gives (LDS stores from fixed registers) while the lane's stack stays inside its LDS part, and through the
sequential loop once an entry would go past it into private memory. Both paths must leave the stack as the reference's
visiting order wants it: every comparison here is on the bit patterns of the oracle's hit records, through k_trace and
through k_trav<0>, <2> and <1>, and `trav_stack_stats()` proves which of the two paths the rays of a call took.

 * a deep scene (a geometric string of slivers: the BVH is a chain, and a ray along it holds more entries than the LDS
   part has) -- both paths in every launch;
 * the stacked sheets of test_gpu_parity (records with all four children hit) -- more than one entry per ray;
 * the same sheets seen from the front -- never past the LDS part."""
import numpy as np
import pytest

import scenes_text as st
import trace_check as tc
from test_gpu_parity import _stacked_sheets_scene

pytestmark = pytest.mark.gpu

N_SLIVERS = 4096
ALONG_SHARE, SHEET_SHARE = 0.003, 0.6
SHEET_AT = np.array([-10.0, -10.0, -5.0])
GROWTH = 26.0 / N_SLIVERS   # x_i = exp(GROWTH i): 1 .. e^26 (the cube of a coordinate stays far inside float32)


def _string_of_slivers(pt):
    """4096 thin triangles strung along the diagonal (1, 1, 1), sliver i at distance exp(GROWTH i) and of a size in proportion,
    each across the diagonal. The SAH's twelve buckets then hold nearly every centroid in the first one, level after level:
    the tree is a chain that peels a few hundred slivers off the sparse end at a time, and a ray along the string from the
    dense end finds the far sibling's box hit at every level."""
    rng = np.random.default_rng(3)
    axis = np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    u = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)
    v = np.cross(axis, u)
    x = np.exp(GROWTH * np.arange(N_SLIVERS))
    P, idx = [], []
    for i in range(N_SLIVERS):
        c = x[i] * axis
        rad = 0.3 * GROWTH * x[i]   # (well inside the gap to the neighbours, GROWTH x_i)
        ph = rng.uniform(0, 2 * np.pi)
        for k in range(3):
            a = ph + 2 * np.pi * k / 3
            P.append(c + rad * (np.cos(a) * u + np.sin(a) * v) + 0.02 * rad * rng.uniform(-1, 1) * axis)
        idx += [3 * i, 3 * i + 1, 3 * i + 2]
    # beside the string's dense end: two sheets of 12 x 12 quads, half a unit apart. A ray through them finds several boxes of a
    # record hit, in the any-hit kernels too, and holds a few entries, all in LDS.
    for z in (0.0, -0.5):
        for cy in range(12):
            for cx in range(12):
                b = len(P)
                q = SHEET_AT + np.array([cx - 6.0, cy - 6.0, z])
                P += [q, q + [1, 0, 0], q + [1, 1, 0], q + [0, 1, 0]]
                idx += [b, b + 1, b + 2, b, b + 2, b + 3]
    P = np.asarray(P, np.float32)
    body = ('Shape "trianglemesh" "integer indices" [%s] "point P" [%s]\n'
            % (" ".join(map(str, idx)), " ".join(repr(float(c)) for p in P for c in p)))
    s = pt.Scene(text=st._HEAD % dict(res=8, spp=1, depth=1, extra="") + 'LightSource "point" "rgb I" [1 1 1]\n' + body + "WorldEnd\n")
    centres = P[:3 * N_SLIVERS].reshape(N_SLIVERS, 3, 3).astype(np.float64).mean(axis=1)
    return s, centres, x, (axis, u, v)


def _string_rays(centres, x, frame, n=20000, seed=29, along_share=ALONG_SHARE, sheet_share=SHEET_SHARE):
    """Rays at slivers, t = 1 at the sliver aimed at. `along_share` of them run along the string -- half from on it, half from
    anywhere near it, beyond either end included -- at far targets: the octants + + + and - - -, and stacks far beyond the
    LDS part (an any-hit ray, which takes a record's children as they lie, pushes hundreds of entries there: hence few
    of them). The others cross the string from beside it at a neighbour's distance: the six mixed octants, shallow stacks.
    `sheet_share` of the rays go through the two sheets beside the dense end, from all around them: every octant, a few
    entries a ray in every kernel. Half unbounded, the others end between a fifth of the way and three times the way to the
    target, so the lanes of a wave differ in depth."""
    axis, u, v = frame
    rng = np.random.default_rng(seed)
    j = rng.integers(0, N_SLIVERS, n)
    pick = rng.random(n)
    kind = np.where(pick < along_share / 2, 0, np.where(pick < along_share, 2, 1))
    k = np.where(kind == 1, np.clip(j + rng.integers(-3, 4, n), 0, N_SLIVERS - 1), rng.integers(0, N_SLIVERS, n))
    along = x[j] * np.where(kind == 1, 1 + GROWTH * rng.uniform(-2, 2, n), rng.uniform(0.0, 1.5, n))
    ends = rng.random(n)
    along = np.where((kind != 1) & (ends < .1), -0.5 * x[j], np.where((kind != 1) & (ends > .9), x[-1] * rng.uniform(1.01, 2, n), along))
    side = np.where(kind == 0, GROWTH * 0.1, np.where(kind == 1, 0.5, rng.uniform(0, 0.5, n))) * np.abs(along) * rng.uniform(0, 1, n)
    ang = rng.uniform(0, 2 * np.pi, n)
    o = along[:, None] * axis + side[:, None] * (np.cos(ang)[:, None] * u + np.sin(ang)[:, None] * v)
    tgt = centres[k]
    sheet = rng.random(n) < sheet_share
    o[sheet] = SHEET_AT + rng.uniform(-9, 9, (int(sheet.sum()), 3))
    tgt[sheet] = SHEET_AT + np.stack([rng.uniform(-6, 6, int(sheet.sum())), rng.uniform(-6, 6, int(sheet.sum())), np.full(int(sheet.sum()), -0.25)], -1)
    o = o.astype(np.float32)
    d = (tgt - o.astype(np.float64)).astype(np.float32)
    tmax = np.where(rng.random(n) < .5, np.inf, rng.uniform(.2, 3, n)).astype(np.float32)
    return np.concatenate([o, d, tmax[:, None]], axis=1).astype(np.float32)


def _octants(rays):
    d = rays[:, 3:6]
    return (d[:, 0] < 0).astype(int) | ((d[:, 1] < 0).astype(int) << 1) | ((d[:, 2] < 0).astype(int) << 2)


def _wavefront_modes(integ, rays, closest, occluded):
    """trace_check.check_wavefront's comparisons (modes 0, 2, 1), one call at a time, with the stack statistics of each call."""
    stats = {}
    for mode, rr in ((0, rays), (2, tc.unbounded(rays))):
        got, extra = integ.trace_wavefront(rr, mode=mode)
        stats[mode] = integ.trav_stack_stats()
        assert (tc.bits(extra)[:, 3] != -2).all(), "a ray was never answered by k_trav<%d>" % mode
        assert np.array_equal(tc.bits(got), tc.bits(closest(rr))), mode
    sh = tc.shadow_form(rays)
    got, extra = integ.trace_wavefront(sh, mode=1)
    stats[1] = integ.trav_stack_stats()
    assert (tc.bits(extra)[:, 3] != -2).all(), "a ray was never answered by k_trav<1>"
    assert np.array_equal(tc.bits(got)[:, 0] >= 0, np.asarray(occluded(sh), bool))
    assert (tc.bits(got)[:, 1:] == 0).all()
    return stats


def test_deep_stacks_take_both_push_paths_in_one_launch(pt, ob):
    s, centres, x, frame = _string_of_slivers(pt)
    assert s.errors == [] and s.stats["n_triangles"] == N_SLIVERS + 2 * 12 * 12 * 2
    rays = _string_rays(centres, x, frame)
    assert (np.bincount(_octants(rays), minlength=8) > 200).all()   # every octant's visiting order is used
    assert .4 < np.isinf(rays[:, 6]).mean() < .6
    closest, occluded = tc.oracle_answers(ob, s)
    want = closest(rays)
    assert (want.view(np.int32)[:, 0] >= 0).mean() > .5
    integ = pt.CreatePathIntegrator(s)
    assert np.array_equal(integ.trace(rays).view(np.int32), want.view(np.int32))
    stats = _wavefront_modes(integ, rays, closest, occluded)
    print("deep scene: (pushed, beyond LDS) per mode", stats)
    for mode in (0, 2, 1):
        pushed, beyond = stats[mode]
        # entries past the LDS part (the sequential loop ran), and more below it (the rank stores ran), in the same launch
        assert beyond > 0 and pushed - beyond > beyond, (mode, pushed, beyond)


def test_records_with_all_four_children_hit(pt, ob):
    s = _stacked_sheets_scene(pt)
    rng = np.random.default_rng(41)
    n = 24000
    # from in front of and from behind the sheets, origins and targets on all sides of each other: eight octants
    o = np.stack([rng.uniform(-6, 6, n), rng.uniform(-6, 6, n), np.where(rng.random(n) < .5, rng.uniform(-2, 4.5, n), rng.uniform(5.5, 12, n))], -1).astype(np.float32)
    tgt = np.stack([rng.uniform(-3, 3, n), rng.uniform(-3, 3, n), np.full(n, 5.0)], -1).astype(np.float32)
    d = tgt - o
    tmax = np.where(rng.random(n) < .7, np.inf, rng.uniform(.5, 3, n)).astype(np.float32)
    rays = np.concatenate([o, d, tmax[:, None]], axis=1).astype(np.float32)
    assert (np.bincount(_octants(rays), minlength=8) > 200).all()
    closest, occluded = tc.oracle_answers(ob, s)
    want = closest(rays)
    assert (want.view(np.int32)[:, 0] >= 0).mean() > .5
    integ = pt.CreatePathIntegrator(s)
    assert np.array_equal(integ.trace(rays).view(np.int32), want.view(np.int32))
    stats = _wavefront_modes(integ, rays, closest, occluded)
    print("stacked sheets: (pushed, beyond LDS) per mode", stats)
    for mode in (0, 2, 1):
        assert stats[mode][0] > n, (mode, stats[mode])   # more than one entry a ray: records with several children hit


def test_shallow_scene_never_leaves_the_lds_part(pt, ob):
    """The stacked sheets from one side, as a camera would see them: a tree a few records deep. (Killeroo's camera rays do
    reach beyond twelve entries: 5 entries of 76 304.)"""
    s = _stacked_sheets_scene(pt)
    integ = pt.CreatePathIntegrator(s)
    rng = np.random.default_rng(7)
    n = 20000
    o = np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), np.zeros(n)], -1).astype(np.float32)
    tgt = np.stack([rng.uniform(-3.5, 3.5, n), rng.uniform(-3.5, 3.5, n), np.full(n, 5.0)], -1).astype(np.float32)
    rays = np.concatenate([o, tgt - o, np.full((n, 1), np.inf, np.float32)], axis=1).astype(np.float32)
    closest, occluded = tc.oracle_answers(ob, s)
    stats = _wavefront_modes(integ, rays, closest, occluded)
    print("sheets from the front: (pushed, beyond LDS) per mode", stats)
    for mode in (0, 2, 1):
        assert stats[mode][0] > 0 and stats[mode][1] == 0, (mode, stats[mode])
