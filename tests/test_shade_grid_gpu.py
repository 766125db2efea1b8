"""k_shade on grids sized by its class queues, and instances with empty queues left out, against the CPU oracle. Run on the
GPU box with `pytest -m gpu`.

After the resolve stage of the path rays the host reads the 16 shading-queue counts and launches every k_shade instance on
the blocks its queues fill (mi_pt_shade_grid; tests/test_shade_grid.py holds that number to the kernel's prologue).
MIPT_SHADE_GRID=pool (read at every render) brings the former shape back: every instance of the plan on pool / 256 + 16
blocks in every iteration, no read. The oracle knows nothing of grids: exact-mode parity (test_gpu_parity._parity: weights
equal, camera rays equal, the five counters within 2, film relative L2 < 1e-6, every pixel within 2e-4 x mean radiance) must
hold in both modes, and the two modes must give one render: every counter equal, films within the 1e-6 that
test_queue_grid_gpu.py asks between two grids.

What can go wrong and where it would show: a grid of ceil(sum / 256) instead of the sum of the ceilings drops vertices when
several classes of one instance hold a partial block each (the zoo on 768 slots: three classes share an instance); a read
placed before k_resolve_overflow misses what that kernel appends (the sphere row's quadric lists overflow); an off-by-one at
whole blocks (the furnace on 256 slots: queues of exactly 256); counts of another sub-renderer (MIPT_STREAMS=2).

No tolerance is defined here: the bars are _parity's."""
import numpy as np
import pytest

import scenes_text as st
from test_gpu_parity import _parity, _rel_l2
from test_metadata_gpu import _setup as _metadata_setup
from test_render_schedule_gpu import SCENES, _oracle, _zoo_text, assets  # noqa: F401  (assets: the module's fixture)

pytestmark = pytest.mark.gpu

BLOCK, MAX_CLASSES = 256, 16


def _instances(s):
    """{k_shade instance: its classes} of the scene's shading plan."""
    inst = {}
    for c, k in s.shade_plan()["classes"].items():
        inst.setdefault(k["instance"], []).append(c)
    return inst


def _render(pt, ob, monkeypatch, s, oracle, what, mode, pool, weights_exact=True):
    """One device render at _parity's bars with MIPT_SHADE_GRID unset (mode None) or set to `mode`: film, counters, launch stats."""
    monkeypatch.delenv("MIPT_SHADE_GRID", raising=False)
    if mode is not None:
        monkeypatch.setenv("MIPT_SHADE_GRID", mode)
    film, _, integ, _, _, _ = _parity(pt, ob, s, "%s | shade grid %s, pool %s" % (what, mode or "queues", pool or "default"),
                                      weights_exact=weights_exact, render=dict(path_pool=pool), oracle=oracle)
    launches, blocks = integ.shade_launch_stats()
    c = integ.counters.as_dict()
    print("%s mode %s pool %s: iterations %d, k_shade launches %d, blocks %d" % (what, mode, integ.pool_info()[0], c["iterations"], launches, blocks))
    return film, c, launches, blocks, integ.pool_info()[0]


def _both_modes(pt, ob, monkeypatch, s, oracle, what, pool, weights_exact=True):
    """The render in both modes: each at parity, all counters equal, the films within 1e-6; the launch stats of the pool mode
    are what the former LaunchShade did. Returns the stats of the queue-sized mode."""
    film, c, launches, blocks, slots = _render(pt, ob, monkeypatch, s, oracle, what, None, pool, weights_exact)
    pfilm, pc, planches, pblocks, pslots = _render(pt, ob, monkeypatch, s, oracle, what, "pool", pool, weights_exact)
    assert slots == pslots and (not pool or slots == pool)
    assert c == pc, {k: (c[k], pc[k]) for k in c if c[k] != pc[k]}
    assert _rel_l2(film, pfilm) < 1e-6
    n_inst = len(_instances(s))
    assert planches > 0 and planches % n_inst == 0 and planches <= c["iterations"] * n_inst
    assert pblocks == planches * (slots // BLOCK + MAX_CLASSES)
    # queue-sized: never more launches, and each covers at most its entries / 256 + one partial block per class
    assert 0 < launches <= planches
    assert blocks <= (c["camera_rays"] + c["regular_rays"]) // BLOCK + launches * MAX_CLASSES
    return c, launches, blocks, slots, n_inst


@pytest.mark.parametrize("pool", [0, 768])
def test_zoo_in_both_modes(pt, ob, assets, monkeypatch, pool):  # noqa: F811
    """The material zoo (14 classes on 7 instances, up to three classes per instance) on the default pool and on 768 slots.
    On 768 slots, not vacuous: instances with empty queues were skipped (fewer launches than iterations x instances), and
    the blocks stay below what the counters allow -- every queue entry is a path ray that was traced (camera_rays +
    regular_rays bounds their number), a launch adds at most one partial block per class it serves, and an iteration of a
    768-slot pool holds at most 3 blocks' worth of entries in all."""
    monkeypatch.delenv("MIPT_SHADE_GRID", raising=False)
    s, oracle, _, _, default_film = _oracle(pt, ob, assets, "zoo halton")
    c, launches, blocks, slots, n_inst = _both_modes(pt, ob, monkeypatch, s, oracle, "zoo halton", pool)
    inst = _instances(s)
    assert n_inst == 7 and max(len(v) for v in inst.values()) == 3
    n_classes = sum(len(v) for v in inst.values())
    assert blocks <= c["iterations"] * (slots // BLOCK + n_classes)
    if pool == 768:
        assert launches < c["iterations"] * n_inst, (launches, c["iterations"])
        # a launch serves at most 3 classes here: 3 + 3 blocks at the very most, against the pool mode's 3 + 16
        assert blocks <= launches * (768 // BLOCK + 3) < launches * (768 // BLOCK + MAX_CLASSES)


def test_sphere_row_in_both_modes(pt, ob, assets, monkeypatch):  # noqa: F811
    """Quadric lists past their four entries: k_resolve_overflow appends to the shading queues after k_resolve_extend, and
    the counts must be read after it."""
    monkeypatch.delenv("MIPT_SHADE_GRID", raising=False)
    s, oracle, _, _, _ = _oracle(pt, ob, assets, "sphere row")
    _both_modes(pt, ob, monkeypatch, s, oracle, "sphere row", 768, weights_exact=SCENES["sphere row"][1])


def test_furnace_of_whole_blocks_in_both_modes(pt, ob, monkeypatch):
    """16 x 16 x 1 spp inside the emissive furnace sphere on a 256-slot pool: the first iteration's queue holds exactly one
    whole block."""
    s = pt.Scene(text=st.furnace_area(res=16, spp=1, depth=8))
    assert s.errors == []
    with ob.exact_libm():
        ofilm, oweight, oc, _ = ob.render(s)
    assert int(oc.camera_rays) == 256
    _both_modes(pt, ob, monkeypatch, s, (ofilm, oweight, oc), "furnace 16x16 1spp", 256)


def test_two_sub_renderers_size_their_own_launches(pt, ob, assets, monkeypatch):  # noqa: F811
    monkeypatch.delenv("MIPT_SHADE_GRID", raising=False)
    s, oracle, _, _, default_film = _oracle(pt, ob, assets, "zoo halton")
    monkeypatch.setenv("MIPT_STREAMS", "2")   # (read when the renderer is created)
    film, c, launches, blocks, slots = _render(pt, ob, monkeypatch, s, oracle, "zoo halton, 2 sub-renderers", None, 768)
    assert slots == 2 * BLOCK
    assert _rel_l2(film, default_film) < 1e-6
    assert 0 < launches < c["iterations"] * len(_instances(s))
    assert blocks <= launches * (BLOCK // BLOCK + 3)   # one block's worth of entries per sub-renderer, at most 3 classes per launch


def test_spectralpath_bands(pt, ob, assets, monkeypatch):  # noqa: F811
    monkeypatch.delenv("MIPT_SHADE_GRID", raising=False)
    s, oracle, _, _, default_film = _oracle(pt, ob, assets, "spectralpath 3 bands")
    film, c, launches, blocks, _ = _render(pt, ob, monkeypatch, s, oracle, "spectralpath 3 bands", None, 0,
                                           weights_exact=SCENES["spectralpath 3 bands"][1])
    assert launches > 0 and _rel_l2(film, default_film) < 1e-6


def test_a_metadata_pass_launches_no_k_shade(pt, ob, monkeypatch):
    """The depth map of the metadata scene, bit for bit what the oracle's entry points give, and no k_shade launch (so no
    read of the class counts either: LaunchShade makes both)."""
    monkeypatch.delenv("MIPT_SHADE_GRID", raising=False)
    scene, exp, integ = _metadata_setup(pt, ob)
    film, weight = integ.Render(strategy="depth")
    assert np.array_equal(weight, exp.weight)
    assert exp.film["depth"].any() and np.array_equal(film.view(np.uint32), exp.film["depth"].view(np.uint32))
    assert integ.shade_launch_stats() == (0, 0)
