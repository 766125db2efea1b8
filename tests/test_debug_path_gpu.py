"""mi_pt_debug_path (PathIntegrator.debug_path) and the pool it borrows. Run on the GPU box with `pytest -m gpu`.

debug_path steps one camera sample through the render's own launches (LaunchTraversal, LaunchResolve, LaunchShade, the dark
rays in line) on a 256-slot pool of its own and hands that pool back; trace_wavefront does the same with a pool sized by its
rays. Two things are held here: every path it logs is the oracle's path (path_rule.paths_agree, the rule of
tools/diag/path_compare.py), and a renderer that lent its pool to either call says so and renders afterwards as a fresh one."""
import numpy as np
import pytest

import scenes_text as st
from path_rule import paths_agree

pytestmark = pytest.mark.gpu


def _zoo(pt):
    """16 x 16, 1 spp, depth 6: 256 paths over several k_shade instances, with shadow, MIS and dark rays."""
    s = pt.Scene(text=st.material_zoo(res=16, spp=1, depth=6))
    assert s.errors == [] and s.film_size == (16, 16) and s.spp == 1
    return s


def _sphere_row(pt):
    """8 x 8, 2 spp: quadrics in rows longer than a ray's list of them, hence k_resolve_overflow."""
    s = pt.Scene(text=st.sphere_row_scene(), xres=8, yres=8, spp=2)
    assert s.errors == [] and s.film_size == (8, 8) and s.spp == 2 and s.desc.n_spheres > 4
    return s


@pytest.mark.parametrize("scene", [_zoo, _sphere_row], ids=["material zoo 16x16", "sphere row 8x8"])
def test_every_logged_path_is_the_oracles(pt, ob, scene):
    """Every camera sample of the frame, device log against oracle log under correctly rounded libm calls: no path may
    differ (_parity allows these scene families 2 counts in 65 536 samples; none is expected in 256 or 128)."""
    s = scene(pt)
    w, h = s.film_size
    integ = pt.CreatePathIntegrator(s)
    differing, vertices = [], 0
    with ob.exact_libm():
        for y in range(h):
            for x in range(w):
                for k in range(s.spp):
                    d, o = integ.debug_path(x, y, k), ob.path_log(s, x, y, k)
                    vertices += len(o)
                    if not paths_agree(d, o):
                        differing.append((x, y, k, len(d), len(o)))
    print("%d paths, %d oracle vertices, %d differ" % (w * h * s.spp, vertices, len(differing)))
    assert vertices > w * h * s.spp   # (not vacuous: paths of more than one vertex)
    assert differing == []


def test_a_lent_pool_is_given_back_in_full(pt):
    """After debug_path and after trace_wavefront the renderer holds no pool and says so, slots and bytes; the next render
    at the default path_pool then sizes its pool as a fresh renderer does and renders the same film (1 spp under the box
    filter: one sample per pixel, so the film does not depend on the order of the adds)."""
    s = _zoo(pt)
    fresh = pt.CreatePathIntegrator(s)
    want_film, want_weight = fresh.Render()
    want_pool = fresh.pool_info()
    assert want_pool[0] >= 256 and want_pool[1] > 0 and want_film.any()

    integ = pt.CreatePathIntegrator(s)
    integ.Render()
    assert integ.pool_info() == want_pool
    assert len(integ.debug_path(8, 8, 0)) >= 1
    assert integ.pool_info() == (0, 0)
    integ.Render()
    assert integ.pool_info() == want_pool
    rays = np.array([[0, 3, -8, 0, -.3, 1, np.inf], [0, 3, -8, .1, -.3, 1, np.inf], [0, 3, -8, -.1, -.25, 1, np.inf],
                     [0, 3, -8, .2, -.35, 1, np.inf], [0, 3, -8, 0, 1, 0, np.inf]], np.float32)
    hits, _ = integ.trace_wavefront(rays, mode=0)
    assert hits.shape == (5, 4)
    assert integ.pool_info() == (0, 0)
    film, weight = integ.Render()
    assert integ.pool_info() == want_pool
    assert np.array_equal(film, want_film) and np.array_equal(weight, want_weight)
