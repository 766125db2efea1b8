"""The dark MIS rays in a queue of their own (Pool::darkQ), traced by a kernel of their own (k_trav<4>) on a stream of their
own beside the next iteration, against the CPU oracle and against the same kernel in line. Run on the GPU box with
`pytest -m gpu`.

Where the live MIS rays are visibility queries (DScene::misAny: no object instances, no alpha mask on an emitter's mesh)
k_shade lists a dark ray -- one that cannot reach the sampled light, test_ray_streams_gpu.py -- in darkQ and not in misQ.
Nothing reads what its traversal finds, so the launch leaves the chain of dependent launches: iteration i's dark rays are
traced on a second stream while the main stream runs the shadow and live MIS stages and k_generate, k_trav<0> and
k_resolve_extend of iteration i + 1, and the next k_shade waits for its end. MIPT_DARK_STREAM=0 (read at every render) runs
the same kernel on the main stream after the live MIS stage.

What can go wrong and where it would show: a dark ray lost, traced twice or traced after its record was overwritten
(regular_rays, bvh_nodes_visited, tri_tests: the walk of a ray is a function of its record alone, so the three sums must
not depend on when the kernel runs); a cursor cleared under a running kernel, or not cleared (the same three, and
dark_launch_stats' entries against rays); a live ray sent to the dark queue or the reverse (total_paths,
zero_radiance_paths, the film); a scene that must keep one queue and lost it (the instanced table).

Small pools make the hazard frequent: on 256 and 768 slots a 32 x 32 x 4 spp render takes dozens of iterations, each with a
dark traversal in flight beside the next one's launches.

No tolerance is defined here: every render goes through test_gpu_parity._parity in the exact mode (weights equal, camera rays
equal, the five counters within 2, film relative L2 < 1e-6, every pixel within 2e-4 x mean radiance); between the two modes
the six counters below are equal as integers and the films within the 1e-6 that test_queue_grid_gpu.py asks between two
schedules of one render (float atomics: accumulation order)."""
import pytest

import scenes_text as st
from test_gpu_parity import _parity, _rel_l2
from test_ray_streams_gpu import dark_scene

pytestmark = pytest.mark.gpu

EQUAL = ("regular_rays", "shadow_rays", "total_paths", "zero_radiance_paths", "bvh_nodes_visited", "tri_tests")

# a one-sided quad emitter that faces the floor (test_ray_streams_gpu.test_estimates_without_a_shadow_ray's): a triangle's
# pdf is 0 for a direction that misses it, so a MIS ray exists only where it reaches the light -- every one is live
_QUAD_EMITTER = (st._HEAD % dict(res=24, spp=4, depth=4, extra="") +
                 'AttributeBegin\n  AreaLightSource "diffuse" "rgb L" [12 12 12]\n'
                 '  Shape "trianglemesh" "integer indices" [0 2 1 0 3 2] "point P" [-.5 0 3.5  .5 0 3.5  .5 0 4.5  -.5 0 4.5]\nAttributeEnd\n'
                 'Material "matte" "rgb Kd" [.5 .5 .5]\n'
                 'Shape "trianglemesh" "integer indices" [0 1 2 0 2 3  4 6 5 4 7 6] '
                 '"point P" [-3 -1.5 1  3 -1.5 1  3 -1.5 7  -3 -1.5 7   -3 1.5 1  3 1.5 1  3 1.5 7  -3 1.5 7]\nWorldEnd\n')

TEXTS = {
    "dark": lambda: dark_scene(),
    "two lights": lambda: dark_scene(two_lights=True),
    "no occluder": lambda: dark_scene(occluder=False),
    "instanced": lambda: dark_scene(instanced=True),
    "all live": lambda: _QUAD_EMITTER,
    "no light": lambda: st.furnace_point(res=16, spp=2, depth=4, n_lights=0),
}
_oracles = {}


def _scene(pt, ob, name):
    """The scene and its one oracle render (shared by every device render of it, never changed)."""
    s = pt.Scene(text=TEXTS[name]())
    assert s.errors == [], (name, s.errors)
    if name not in _oracles:
        with ob.exact_libm():
            ofilm, oweight, oc, _ = ob.render(s)
        _oracles[name] = (ofilm, oweight, oc)
    return s, _oracles[name]


def _render(pt, ob, monkeypatch, name, mode, pool=0, twice=False):
    """One device render of scene `name` at _parity's bars with MIPT_DARK_STREAM=`mode`: film, counters, dark launch stats.
    `twice`: a second render on the same integrator, which must repeat the first."""
    monkeypatch.setenv("MIPT_DARK_STREAM", mode)
    s, oracle = _scene(pt, ob, name)
    film, _, integ, _, _, _ = _parity(pt, ob, s, "%s | dark stream %s, pool %s" % (name, mode, pool or "default"), render=dict(path_pool=pool), oracle=oracle)
    c = integ.counters.as_dict()
    stats = integ.dark_launch_stats()
    if pool:
        assert integ.pool_info()[0] == pool
    if twice:
        film2, _ = integ.Render(path_pool=pool)
        c2 = integ.counters.as_dict()
        assert {k: c2[k] for k in EQUAL} == {k: c[k] for k in EQUAL}, (name, mode, c, c2)
        assert integ.dark_launch_stats() == stats
        assert _rel_l2(film2, film) < 1e-6
    print("%s mode %s pool %s: iterations %d, regular rays %d, dark (launches, entries, rays, skipped by resolve) %s" %
          (name, mode, integ.pool_info()[0], c["iterations"], c["regular_rays"], stats))
    return film, c, stats


def _both(pt, ob, monkeypatch, name, pool=0, twice=False, split=True):
    """Scene `name` in line (0) and beside the next iteration (1): one render. `split`: the scene has the queue of its own.
    Returns the counters and the dark launch stats."""
    film0, c0, stats0 = _render(pt, ob, monkeypatch, name, "0", pool, twice)
    film1, c1, stats1 = _render(pt, ob, monkeypatch, name, "1", pool, twice)
    assert {k: c1[k] for k in EQUAL} == {k: c0[k] for k in EQUAL}, (name, {k: (c0[k], c1[k]) for k in EQUAL if c0[k] != c1[k]})
    assert _rel_l2(film1, film0) < 1e-6
    assert stats1 == stats0, (name, stats0, stats1)
    launches, entries, rays, skipped = stats1
    assert entries == rays, (name, stats1)   # every entry of the queue was traced, once
    if split:   # one launch per iteration that shades, and k_resolve_mis met no dark entry
        assert 0 < launches <= c1["iterations"] and skipped == 0, (name, stats1, c1["iterations"])
        assert rays <= c1["regular_rays"]
    else:       # one queue, as before: no launch, and the resolve kernel skips the dark entries
        assert launches == 0 and entries == 0, (name, stats1)
    return c1, stats1


@pytest.mark.parametrize("pool", [256, 768, 0])
def test_dark_rays_beside_the_next_iteration(pt, ob, monkeypatch, pool):
    """The floor under the sphere light with the table, 32 x 32 x 4 spp. 256 and 768 slots: dozens of iterations, each dark
    traversal beside the next iteration's generate, extend and resolve. Not vacuous: the scene has dark rays, and the small
    pools need more iterations than the 4096 / pool refills."""
    c, (launches, entries, rays, _) = _both(pt, ob, monkeypatch, "dark", pool)
    assert rays > 0
    if pool:
        assert c["iterations"] > 4096 // pool and launches > 4096 // pool


def test_two_lights_and_no_occluder(pt, ob, monkeypatch):
    """Two lights: the live rays carry I_MISLIGHT, the dark ones of either light share the queue. No occluder: the floor's MIS
    rays are dark but for the few inside the light's cone."""
    for name in ("two lights", "no occluder"):
        _, (_, _, rays, _) = _both(pt, ob, monkeypatch, name, 512)
        assert rays > 0


def test_instanced_table_keeps_one_queue(pt, ob, monkeypatch):
    """The table as an object instance: DScene::misAny is off, the dark rays stay in misQ for k_trav<2>, no launch of the dark
    kernel in either mode, and k_resolve_mis skips them."""
    s, _ = _scene(pt, ob, "instanced")
    assert s.desc.n_instances == 1
    _, (_, _, _, skipped) = _both(pt, ob, monkeypatch, "instanced", 256, split=False)
    assert skipped > 0


def test_empty_dark_queue(pt, ob, monkeypatch):
    """Every MIS ray live (a quad emitter facing the floor), and no light at all: launches that find nothing."""
    c, (_, entries, _, _) = _both(pt, ob, monkeypatch, "all live", 256)
    assert entries == 0 and c["regular_rays"] > 0
    c, (_, entries, _, _) = _both(pt, ob, monkeypatch, "no light", 256)
    assert entries == 0 and c["shadow_rays"] == 0


def test_two_sub_renderers(pt, ob, monkeypatch):
    """MIPT_STREAMS=2 (read when the renderer is created): each sub-renderer has its own dark stream, queue and cursors."""
    monkeypatch.setenv("MIPT_STREAMS", "2")
    _, (_, _, rays, _) = _both(pt, ob, monkeypatch, "dark", 512)
    assert rays > 0


def test_two_renders_on_one_integrator(pt, ob, monkeypatch):
    """The second render starts from the first one's streams and events: it must find the dark stream joined and the cursors
    clear, and repeat the first render's counters."""
    _both(pt, ob, monkeypatch, "dark", 768, twice=True)


def test_one_block_per_queue_walking_kernel(pt, ob, monkeypatch):
    """MIPT_QUEUE_BLOCKS=1: k_resolve_shadow and k_resolve_mis on one block each, the longest they can run beside the dark
    traversal."""
    monkeypatch.setenv("MIPT_QUEUE_BLOCKS", "1")
    _both(pt, ob, monkeypatch, "dark", 768)
