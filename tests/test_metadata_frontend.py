"""Integrator "metadata" in the front end (no GPU): parsing, the material and instance ids of every primitive against the
reference's counters written out by hand, the name lists and name files, the scene cache."""
import json
import os
import subprocess
import sys

import pytest

import metadata_scenes as ms
from conftest import ROOT


def _scene(pt, strategy_params, extra_integrator=""):
    return pt.Scene(text=ms.id_scene('Integrator "metadata" %s %s' % (strategy_params, extra_integrator)))


@pytest.mark.parametrize("k,name", list(enumerate(ms.STRATEGIES)))
def test_each_strategy_parses(pt, k, name):
    s = _scene(pt, '"string strategy" ["%s"]' % name)
    assert s.errors == []
    assert s.desc.integrator.kind == pt.INTEGRATOR_METADATA == 1 and s.desc.integrator.metadata_strategy == k
    assert pt.METADATA_STRATEGIES[k] == name


def test_default_strategy_is_depth_and_unknown_falls_back_with_the_reference_warning(pt):
    s = _scene(pt, "")
    assert s.errors == [] and s.desc.integrator.kind == 1 and s.desc.integrator.metadata_strategy == 0
    s = _scene(pt, '"string strategy" ["normals"]')
    assert s.errors == [] and s.desc.integrator.kind == 1 and s.desc.integrator.metadata_strategy == 0
    assert 'Strategy "normals" for metadata unknown. Using "depth".' in s.warnings   # metadata.cpp:105-110


def test_pixelbounds_are_honoured_and_path_scenes_keep_kind_zero(pt):
    s = _scene(pt, '"string strategy" ["mesh"]', '"integer pixelbounds" [2 6 1 5]')
    assert s.errors == [] and list(s.desc.integrator.pixel_bounds) == [2, 1, 6, 5]
    s = pt.Scene(text=ms.id_scene('Integrator "path" "integer maxdepth" [3]'))
    assert s.errors == [] and s.desc.integrator.kind == pt.INTEGRATOR_PATH == 0 and s.desc.integrator.max_depth == 3
    assert bool(s.desc.prim_meta)   # the ids are there for every scene: a path scene can be asked for maps at render time
    s = pt.Scene(text=ms.id_scene('Integrator "bdpt"'))
    assert any("outside the hot-path scope" in e for e in s.errors) and s.desc.integrator.kind == 0


def test_material_and_instance_ids_follow_the_reference_counters(pt):
    s = pt.Scene(text=ms.id_scene())
    assert s.errors == []
    d = s.desc
    assert d.n_instances == 3
    assert ms.world_prim_ids(s) == ms.ID_SCENE_EXPECTED
    # the two textually identical Material directives share one mi_material record and keep their own ids
    by_x = {}
    for i in range(d.n_prims):
        p = d.prims[i]
        if p.instance == 0 and p.shape >= 0:
            by_x[int(round(d.P[3 * d.tri_indices[3 * p.shape]] / 10.0)) * 10] = i
    e, f = by_x[40], by_x[50]
    assert d.prims[e].material == d.prims[f].material
    assert (d.prim_meta[e].material_id, d.prim_meta[f].material_id) == (7, 8)
    # ... as do the two shapes with the same parameters of their own
    assert d.prims[by_x[60]].material == d.prims[by_x[70]].material
    assert d.prims[by_x[100]].material == -1 and d.prim_meta[by_x[100]].material_id == 0   # Material "none"
    # 13 ids, 9 records: default matte, Kd .3, zinc (and the default plastic after it: the same record), amber, blend, Kd .2,
    # the shapes' own Kd, mirror, the object's matte
    assert d.n_materials == 9 == s.stats["n_materials"]


def test_mix_fallbacks_and_recorded_shapes_take_their_ids_in_the_reference_order(pt):
    s = pt.Scene(text=ms.id_scene_fallbacks())
    assert s.errors and all("undefined.  Using \"matte\"" in e for e in s.errors)
    assert ms.world_prim_ids(s) == ms.ID_SCENE_FALLBACKS_EXPECTED
    assert s.named_material_ids == [("ghost", 5), ("zinc", 3)]


def test_expanded_instances_carry_the_same_ids(pt, tmp_path):
    """MIPT_INSTANCES=expand is read when a scene is loaded: a child process loads the same text and reports its ids."""
    script = tmp_path / "ids.py"
    script.write_text(
        "import sys, json\nsys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import pbrt_v3_spectral_amd as pt, metadata_scenes as ms\n"
        "s = pt.Scene(text=ms.id_scene())\n"
        "f = pt.Scene(text=ms.id_scene_fallbacks())\n"
        "print(json.dumps([s.desc.n_instances, s.errors, sorted(ms.world_prim_ids(s).items()), s.instance_names, sorted(ms.world_prim_ids(f).items())]))\n"
        % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, str(script)], env=dict(os.environ, MIPT_INSTANCES="expand"), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    n_instances, errors, ids, names, fallback_ids = json.loads(r.stdout.strip().splitlines()[-1])
    assert {k: tuple(v) for k, v in fallback_ids} == ms.ID_SCENE_FALLBACKS_EXPECTED
    assert n_instances == 0 and errors == []
    assert {k: tuple(v) for k, v in ids} == ms.ID_SCENE_EXPECTED
    assert names == ms.ID_SCENE_INSTANCES


def test_names_and_name_files(pt, tmp_path):
    for strategy, suffix, lines in [("mesh", "_mesh.txt", ["%d %s" % (k + 1, n) for k, n in enumerate(ms.ID_SCENE_INSTANCES)]),
                                    ("material", "_materials.txt", ["%d %s" % (i, n) for n, i in ms.ID_SCENE_NAMED])]:
        s = _scene(pt, '"string strategy" ["%s"]' % strategy)
        assert s.instance_names == ms.ID_SCENE_INSTANCES and s.named_material_ids == ms.ID_SCENE_NAMED
        out = tmp_path / strategy
        out.mkdir()
        s.write_metadata_names(str(out / "frame.01.exr"))   # the stem ends at the LAST '.'
        assert sorted(os.listdir(out)) == ["frame.01" + suffix]
        assert (out / ("frame.01" + suffix)).read_text() == "".join(l + "\n" for l in lines)
    for strategy in ("depth", "coordinates"):
        out = tmp_path / strategy
        out.mkdir()
        _scene(pt, '"string strategy" ["%s"]' % strategy).write_metadata_names(str(out / "frame.exr"))
        assert os.listdir(out) == []
    out = tmp_path / "path"
    out.mkdir()
    pt.Scene(text=ms.id_scene('Integrator "path"')).write_metadata_names(str(out / "frame.exr"))
    assert os.listdir(out) == []


def test_scene_cache_keeps_the_integrator_the_ids_and_the_names(pt, tmp_path):
    s = _scene(pt, '"string strategy" ["coordinates"]')
    path = str(tmp_path / "scene.bin")
    s.save_cache(path)
    c = pt.Scene(cache=path)
    assert (c.desc.integrator.kind, c.desc.integrator.metadata_strategy) == (1, 3)
    assert c.desc.n_prims == s.desc.n_prims and bool(c.desc.prim_meta)
    ids = lambda sc: [(sc.desc.prim_meta[i].material_id, sc.desc.prim_meta[i].instance_id) for i in range(sc.desc.n_prims)]
    assert ids(c) == ids(s) and ms.world_prim_ids(c) == ms.ID_SCENE_EXPECTED
    assert c.instance_names == ms.ID_SCENE_INSTANCES and c.named_material_ids == ms.ID_SCENE_NAMED


def test_metadata_integrator_needs_a_gpu(pt):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the renderer is created")
    s = _scene(pt, '"string strategy" ["depth"]')
    with pytest.raises(RuntimeError, match="no HIP device|no CPU fallback|mi_pt_create failed"):
        pt.MetadataIntegrator(s)
    with pytest.raises(RuntimeError, match="no HIP device|no CPU fallback|mi_pt_create failed"):
        pt.CreateIntegrator(s)
