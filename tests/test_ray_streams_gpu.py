"""Direct-lighting estimates whose BSDF-sampled (MIS) ray is dark -- it cannot reach the sampled area light -- against the CPU
oracle. Run on the GPU box with `pytest -m gpu`.

A dark ray is traced and counted (the reference traces it), but nothing reads its answer, so the state machine treats its
estimate as one without a MIS ray: the shadow ray's commit closes it (CommitShadowVerdict), or k_shade itself when there is no
shadow ray either; k_trav<3> / k_trav<2> answer MIS_ANSWER_DARK and k_resolve_mis skips the entry. What can go wrong is a
wrongly closed estimate (zero_radiance_paths, the film), a lost or re-traced ray (regular_rays, shadow_rays) or an estimate
that stays open (total_paths, the film of the path's later vertices).

No tolerance is defined here: every render goes through test_gpu_parity._parity in the exact mode (weights equal, camera rays
equal, the five counters within 2, film relative L2 < 1e-6, every pixel within 2e-4 x mean radiance)."""
import pytest

import scenes_text as st
from test_gpu_parity import _parity

pytestmark = pytest.mark.gpu

_DARK_HEAD = """
LookAt 0 2.5 -6  0 0.6 0  0 1 0
Camera "perspective" "float fov" [42]
Film "image" "integer xresolution" [%(res)d] "integer yresolution" [%(res)d]
Sampler "halton" "integer pixelsamples" [%(spp)d]
Integrator "path" "integer maxdepth" [5]
WorldBegin
AttributeBegin
  AreaLightSource "diffuse" "rgb L" [60 56 50]
  Translate 0 3 0
  Shape "sphere" "float radius" [.2]
AttributeEnd
%(more)s
Material "matte" "rgb Kd" [.6 .6 .6]
Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-4 0 -4  4 0 -4  4 0 4  -4 0 4]
"""
# The occluder: a matte table top at y = 1.4 between the floor and the light. The floor under it has occluded shadow rays
# (and dark MIS rays: zero radiance, closed by the shadow resolve); the table's underside, reached by the floor's bounce rays,
# has the light behind its surface: f is black, no shadow ray, a dark MIS ray -- closed in k_shade.
_TABLE = ('Material "matte" "rgb Kd" [.7 .5 .3]\n'
          'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1.2 1.4 -1.2  1.2 1.4 -1.2  1.2 1.4 1.2  -1.2 1.4 1.2]\n')
_SECOND_LIGHT = ('AttributeBegin\n  AreaLightSource "diffuse" "rgb L" [20 24 30]\n  Translate 2.5 1.2 1\n'
                 '  Shape "sphere" "float radius" [.3]\nAttributeEnd')
# the same table as an object instance: the scene's MIS rays then go through the closest-hit kernel (k_trav<2>, INST)
_TABLE_INSTANCE = 'ObjectBegin "table"\n%sObjectEnd\nObjectInstance "table"\n' % _TABLE


def dark_scene(res=32, spp=4, two_lights=False, instanced=False, occluder=True):
    body = _DARK_HEAD % dict(res=res, spp=spp, more=_SECOND_LIGHT if two_lights else "")
    if occluder:
        body += _TABLE_INSTANCE if instanced else _TABLE
    return body + "WorldEnd\n"


def _check(pt, ob, monkeypatch, text, what, pool=0, shade_grid=None, queue_blocks=None, oracle=None):
    for var, val in (("MIPT_SHADE_GRID", shade_grid), ("MIPT_QUEUE_BLOCKS", queue_blocks)):
        monkeypatch.delenv(var, raising=False)
        if val is not None:
            monkeypatch.setenv(var, str(val))
    s = pt.Scene(text=text)
    assert s.errors == [], (what, s.errors)
    _, _, integ, ofilm, oweight, oc = _parity(pt, ob, s, "%s | pool %s, shade grid %s, queue blocks %s" % (what, pool or "default", shade_grid or "queues", queue_blocks or "default"),
                                              render=dict(path_pool=pool), oracle=oracle)
    if pool:
        assert integ.pool_info()[0] == pool
    c = integ.counters
    # (_parity allows two counts; these two are integers that no arithmetic of the device can move)
    assert int(c.total_paths) == int(oc.total_paths), (what, int(c.total_paths), int(oc.total_paths))
    assert int(c.zero_radiance_paths) == int(oc.zero_radiance_paths), (what, int(c.zero_radiance_paths), int(oc.zero_radiance_paths))
    return integ, (ofilm, oweight, oc)


@pytest.mark.parametrize("two_lights", [False, True])
def test_dark_mis_rays_close_no_estimate(pt, ob, monkeypatch, two_lights):
    """A matte floor under a small sphere light with an occluder, 32 x 32 x 4 spp: most MIS rays are dark. The default pool (one
    k_shade launch per iteration holds every vertex), 768 slots (many iterations, queues that shrink) and one block per
    queue-walking kernel, each against one oracle render. With two lights the rays that are not dark carry I_MISLIGHT.
    Not vacuous: a third and more of the estimates add nothing (the floor under the table, the table's underside)."""
    text = dark_scene(two_lights=two_lights)
    integ, oracle = _check(pt, ob, monkeypatch, text, "dark rays, %d light(s)" % (2 if two_lights else 1))
    oc = oracle[2]
    assert int(oc.zero_radiance_paths) * 10 > int(oc.total_paths), (int(oc.zero_radiance_paths), int(oc.total_paths))
    assert int(oc.zero_radiance_paths) < int(oc.total_paths)
    _check(pt, ob, monkeypatch, text, "dark rays, %d light(s)" % (2 if two_lights else 1), pool=768, oracle=oracle)
    _check(pt, ob, monkeypatch, text, "dark rays, %d light(s)" % (2 if two_lights else 1), pool=768, shade_grid="pool", queue_blocks=1, oracle=oracle)


def test_dark_mis_rays_through_the_closest_hit_kernel(pt, ob, monkeypatch):
    """The same scene with the table as an object instance: no visibility form of the MIS rays (DScene::misAny is off), so
    k_trav<2> traces the dark rays to their closest hit, answers MIS_ANSWER_DARK and stores no hit record."""
    text = dark_scene(instanced=True)
    s = pt.Scene(text=text)
    assert s.errors == [] and s.desc.n_instances == 1
    _, oracle = _check(pt, ob, monkeypatch, text, "dark rays, instanced occluder")
    _check(pt, ob, monkeypatch, text, "dark rays, instanced occluder", pool=256, queue_blocks=3, oracle=oracle)


def test_every_mis_ray_dark_or_absent(pt, ob, monkeypatch):
    """Queues that are all or mostly without a consumer. No occluder: the floor's MIS rays are dark but for the few inside
    the light's cone. A point light only: no MIS ray anywhere. No light at all: no estimate rays (and nothing to see)."""
    _check(pt, ob, monkeypatch, dark_scene(occluder=False), "dark rays, no occluder", pool=512)
    _check(pt, ob, monkeypatch, st.furnace_point(res=17, spp=4, depth=4), "point light only", pool=256)
    dark_world = st.furnace_point(res=16, spp=2, depth=4, n_lights=0)
    integ, _ = _check(pt, ob, monkeypatch, dark_world, "no light", pool=256)
    assert int(integ.counters.shadow_rays) == 0


def test_estimates_without_a_shadow_ray(pt, ob, monkeypatch):
    """A one-sided quad emitter that faces away from half of the geometry (the zoo's ceiling light shines down; here the floor
    AND a ceiling above the emitter are lit by it): above it Li is black, so the estimate has no shadow ray, and its MIS ray
    -- dark or not -- must close it alone."""
    text = (st._HEAD % dict(res=24, spp=4, depth=4, extra="") +
            'AttributeBegin\n  AreaLightSource "diffuse" "rgb L" [12 12 12]\n'
            '  Shape "trianglemesh" "integer indices" [0 2 1 0 3 2] "point P" [-.5 0 3.5  .5 0 3.5  .5 0 4.5  -.5 0 4.5]\nAttributeEnd\n'
            'Material "matte" "rgb Kd" [.5 .5 .5]\n'
            'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3  4 6 5 4 7 6] '
            '"point P" [-3 -1.5 1  3 -1.5 1  3 -1.5 7  -3 -1.5 7   -3 1.5 1  3 1.5 1  3 1.5 7  -3 1.5 7]\nWorldEnd\n')
    _, oracle = _check(pt, ob, monkeypatch, text, "one-sided emitter")
    oc = oracle[2]
    assert int(oc.shadow_rays) < int(oc.total_paths)   # estimates without a shadow ray exist
    _check(pt, ob, monkeypatch, text, "one-sided emitter", pool=256, shade_grid="pool", oracle=oracle)


@pytest.mark.parametrize("res,pool", [(16, 256), (17, 512)])
def test_whole_and_partial_blocks(pt, ob, monkeypatch, res, pool):
    """Inside the emissive furnace sphere at 1 spp: 16 x 16 on a 256-slot pool is a MIS queue of exactly one block, 17 x 16
    (here 17 x 17 = 289) on 512 slots a second, partial one. Every MIS ray reaches the light: none is dark."""
    _check(pt, ob, monkeypatch, st.furnace_area(res=res, spp=1, depth=8), "furnace %d" % res, pool=pool)
