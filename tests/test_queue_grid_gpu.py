"""The resolve kernels that walk a queue (k_resolve_shadow, k_resolve_mis) on grids smaller than their queues, and the paths
that k_resolve_extend ends itself (an escaped ray, a vertex at the depth limit), against the CPU oracle. Run on the GPU box
with `pytest -m gpu`.

The two kernels run on a grid sized by what the device holds at once and walk their queues in steps of the grid. At the sizes
of a test scene that grid is larger than any queue, so every block makes at most one trip -- MIPT_QUEUE_BLOCKS (read at every
render) caps the grid: with 1 and 3 blocks a block makes many trips, and on a 768-slot pool the grid of 3 is at times larger
than the work. The oracle knows nothing of grids: exact-mode parity (test_gpu_parity._parity: weights equal, camera rays
equal, the five counters within 2, film relative L2 < 1e-6, every pixel within 2e-4 x mean radiance) must hold at every cap.

No tolerance is defined here: the bars are _parity's."""
import pytest

import scenes_text as st
from test_gpu_parity import _parity, _rel_l2
from test_render_schedule_gpu import SCENES, _oracle, _zoo_text, assets  # noqa: F401  (assets: the module's fixture)

pytestmark = pytest.mark.gpu

# total_paths counts the direct-lighting estimates, nearly each of which queues a shadow ray: more than 256 per iteration on
# average means a one-block grid walked its queue in several trips. One pair cannot reach that average whatever the kernels
# do: the sphere row's paths are long (maxdepth 12) and few of a 768-slot pool's are at a vertex with an estimate in one
# iteration -- 40 490 estimates in 186 iterations, 218 per iteration (measured). Its
# first iterations, with all 768 slots on new camera rays, still make several trips; the default-pool case of the scene
# (3 115 per iteration) carries the proof.
AVERAGE_BELOW_ONE_BLOCK = {("sphere row", 768)}

GRID_SCENES = ("zoo halton",        # the most shading classes and k_shade instances
               "sphere row",        # quadric lists and the overflow queues
               "instances lens",    # the INST kernels
               "mis span")          # k_trav<3>, ambiguous MIS rays


@pytest.mark.parametrize("pool", [0, 768])
@pytest.mark.parametrize("cap", [None, 1, 3])
@pytest.mark.parametrize("name", GRID_SCENES)
def test_queue_grid_cap_does_not_change_the_render(pt, ob, assets, monkeypatch, name, cap, pool):  # noqa: F811
    """MIPT_QUEUE_BLOCKS unset, 1 and 3 on the default pool and on 768 slots, each at _parity's bars against one oracle render
    per scene. Not vacuous: with one block, more than 256 direct-lighting estimates per iteration on average, so launches
    walked their queue in more than one trip (AVERAGE_BELOW_ONE_BLOCK: the one pair that cannot show it this way)."""
    monkeypatch.delenv("MIPT_QUEUE_BLOCKS", raising=False)
    s, oracle, default_iterations, _, default_film = _oracle(pt, ob, assets, name)   # (renders at the defaults when first asked)
    if cap is None and pool == 0:
        assert default_iterations > 0
        return
    if cap is not None:
        monkeypatch.setenv("MIPT_QUEUE_BLOCKS", str(cap))
    film, weight, integ, _, _, _ = _parity(pt, ob, s, "%s | queue blocks %s, pool %s" % (name, cap or "default", pool or "default"),
                                           weights_exact=SCENES[name][1], render=dict(path_pool=pool), oracle=oracle)
    if pool:
        assert integ.pool_info()[0] == pool
    c = integ.counters
    print("%s cap %s pool %s: total_paths %d, iterations %d" % (name, cap, pool, c.total_paths, c.iterations))
    if cap == 1 and (name, pool) not in AVERAGE_BELOW_ONE_BLOCK:
        assert c.total_paths > 256 * c.iterations, (int(c.total_paths), int(c.iterations))
    assert _rel_l2(film, default_film) < 1e-6


@pytest.mark.parametrize("cap", [None, 1, 3])
def test_a_queue_of_exactly_one_block(pt, ob, monkeypatch, cap):
    """16 x 16 x 1 spp inside the emissive furnace sphere on a 256-slot pool: every camera ray hits the one material, so the
    first iteration's queues hold whole blocks of 256 entries and no partial one."""
    s = pt.Scene(text=st.furnace_area(res=16, spp=1, depth=8))
    assert s.errors == []
    monkeypatch.delenv("MIPT_QUEUE_BLOCKS", raising=False)
    if cap is not None:
        monkeypatch.setenv("MIPT_QUEUE_BLOCKS", str(cap))
    _, _, integ, _, _, oc = _parity(pt, ob, s, "furnace 16x16 1spp | queue blocks %s, pool 256" % (cap or "default"), render=dict(path_pool=256))
    assert integ.pool_info()[0] == 256 and int(oc.camera_rays) == 256


def _interface_zoo(pt):
    """The material zoo seen through a quad without a material (an interface: the path goes on through it, path.cpp:108-113)."""
    txt = _zoo_text("halton")
    quad = ('AttributeBegin\n  Material "none"\n  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] '
            '"point P" [-1.5 0 -5  1.5 0 -5  1.5 2.5 -5  -1.5 2.5 -5]\nAttributeEnd\nWorldEnd')
    assert txt.count("WorldEnd") == 1
    return pt.Scene(text=txt.replace("WorldEnd", quad))


def _zoo_depth(pt, depth):
    txt = _zoo_text("halton")
    assert '"integer maxdepth" [6]' in txt
    return pt.Scene(text=txt.replace('"integer maxdepth" [6]', '"integer maxdepth" [%d]' % depth))


FINISHED_SCENES = {
    "zoo halton maxdepth 1": lambda pt, d: _zoo_depth(pt, 1),
    "zoo halton maxdepth 2": lambda pt, d: _zoo_depth(pt, 2),
    "infinite light map spatial": SCENES["infinite light map spatial"][0],   # escaped rays that still owe the environment's light after a specular bounce
    "spectralpath 3 bands": SCENES["spectralpath 3 bands"][0],               # a finished band restarts
    "zoo behind an interface": lambda pt, d: _interface_zoo(pt),
}


@pytest.mark.parametrize("name", list(FINISHED_SCENES))
def test_paths_that_end_at_a_miss_or_at_the_depth_limit(pt, ob, assets, monkeypatch, name):  # noqa: F811
    """Escaped rays with and without an environment to show, vertices at maxdepth with and without an emission check, an
    interface primitive in front of the geometry: films and all counters (total_paths, zero_radiance_paths and
    path_length_sum among them) at _parity's bars, on the default grid and with one block per queue-walking kernel."""
    s = FINISHED_SCENES[name](pt, assets)
    assert s.errors == [], (name, s.errors)
    if name == "zoo behind an interface":
        assert any(s.desc.prims[i].material < 0 for i in range(s.desc.n_prims))
    with ob.exact_libm():
        ofilm, oweight, oc, _ = ob.render(s)
    monkeypatch.delenv("MIPT_QUEUE_BLOCKS", raising=False)
    _parity(pt, ob, s, name + " | finished paths", oracle=(ofilm, oweight, oc))
    monkeypatch.setenv("MIPT_QUEUE_BLOCKS", "1")
    _parity(pt, ob, s, name + " | finished paths, queue blocks 1", oracle=(ofilm, oweight, oc))
