"""Accelerator "bvh" "string splitmethod" "hlbvh" (BVHAccel::HLBVHBuild, src/accelerators/bvh.cpp:404-638).

CPU: the host restatement builds a valid tree (every primitive in exactly one leaf, every node's box
containing its children's, leaf sizes below maxnodeprims) whose closest hits on recorded rays are those of the SAH tree.
GPU: the device build (mi_bvh_build_hlbvh: Morton codes, stable split sort, one lane per treelet for emitLBVH, flatten)
returns the same node array and primitive order as the host restatement, bit for bit; the render under it matches the oracle.

Below the whole-scene tests the build is taken stage by stage on raw bounds (mi_bvh_build_host / mi_bvh_build_hlbvh, no scene
text), one family of synthetic boxes per thing that can go wrong: sizes about the wave, the block and the sort tile, and n = 1, 2
(with maxnodeprims 1, 4 and the clamp at 255, negative coordinates and zeros of both signs); more than 1024 sort tiles (the
scan's carry); primitives that share one Morton code (sort stability, leaves above maxnodeprims); centroid bounds flat on
every choice of axes; exactly 4096 treelets with singletons beside a crowded one.
CPU: the host build equals tests/hlbvh_reference.py, a numpy restatement written from the reference alone, treelet by treelet.
GPU: the device build equals the host build byte for byte, and its order the stable sort of the reference's codes.
A leaf of more than 65 535 primitives (the node's 16-bit count; the reference CHECKs it away) is an error of both builders and of
the scene, never a wrapped count; leaves of 300 ... 16 383 triangles trace like the oracle through every traversal variant, and
16 384 is the renderer's refusal."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor
import sys

import numpy as np
import pytest

from conftest import KILLEROO, ROOT
import hlbvh_reference as hr
import scenes_text as st
import trace_check as tc


def _nodes(s):
    d = s.desc
    raw = np.ctypeslib.as_array(d.nodes, (d.n_nodes,))   # structured: bmin, bmax, offset, n_prims, axis, pad
    return raw


def _check_tree(s, max_prims):
    nodes = _nodes(s)
    n = len(nodes)
    bmin, bmax = np.array(nodes["bmin"]), np.array(nodes["bmax"])
    offset, nprims = np.array(nodes["offset"]), np.array(nodes["n_prims"])
    seen = np.zeros(s.desc.n_prims, int)
    next_leaf = 0
    stack = sorted({0} | {int(s.desc.instances[k].root) for k in range(s.desc.n_instances)})   # the world's tree and the objects'
    while stack:   # depth first: first child = i + 1, second = offset
        i = stack.pop()
        if nprims[i] > 0:
            next_leaf += int(nprims[i])           # (treelets keep Morton order inside; the SAH tree above reorders the treelets)
            seen[offset[i]:offset[i] + nprims[i]] += 1
            continue
        a, b = i + 1, int(offset[i])
        assert i < a < n and a < b < n
        for c in (a, b):
            assert (bmin[c] >= bmin[i]).all() and (bmax[c] <= bmax[i]).all()
        stack.append(b)
        stack.append(a)
    assert (seen == 1).all() and next_leaf == s.desc.n_prims
    leaves = nprims[nprims > 0]
    return int((nprims == 0).sum()), len(leaves), int(leaves.max())


def _with_hlbvh(text, maxprims=None):
    extra = ' "integer maxnodeprims" [%d]' % maxprims if maxprims else ""
    return text.replace("WorldBegin", 'Accelerator "bvh" "string splitmethod" "hlbvh"%s\nWorldBegin' % extra, 1)


def _rays(rng, s, n):
    d = s.desc
    lo = np.array([d.nodes[0].bmin[i] for i in range(3)], np.float32)
    hi = np.array([d.nodes[0].bmax[i] for i in range(3)], np.float32)
    o = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    dr = rng.normal(size=(n, 3)).astype(np.float32)
    return np.concatenate([o, dr, np.full((n, 1), np.inf, np.float32)], axis=1).astype(np.float32)


def test_host_hlbvh_is_a_valid_tree_with_the_sah_trees_hits(pt, ob, monkeypatch):
    monkeypatch.setenv("MIPT_HLBVH", "host")
    text = open(KILLEROO).read()
    base = os.path.dirname(KILLEROO)
    sah = pt.Scene(text=text, base_dir=base, spp=1)
    hl = pt.Scene(text=_with_hlbvh(text), base_dir=base, spp=1)
    assert hl.errors == [] and not any("hlbvh" in w for w in hl.warnings) and hl.stats["accel_on_device"] == 0
    interior, leaves, biggest = _check_tree(hl, 4)
    assert interior == hl.stats["interior_nodes"] and leaves == hl.stats["leaf_nodes"] and interior == leaves - 1
    assert biggest < 4 or biggest <= 255      # emitLBVH: leaves of fewer than maxPrimsInNode primitives (more only when the code bits run out)
    # the same geometry: closest hits (t, barycentrics) on recorded rays equal the SAH tree's, primitive for primitive
    rng = np.random.default_rng(3)
    rays = _rays(rng, sah, 20000)
    a, _ = ob.trace(sah, rays)
    b, _ = ob.trace(hl, rays)
    assert np.array_equal(a[:, 1:].view(np.int32), b[:, 1:].view(np.int32))
    hit = a.view(np.int32)[:, 0] >= 0
    assert np.array_equal(hit, b.view(np.int32)[:, 0] >= 0) and hit.mean() > 0.3
    # (primitive numbers differ -- another leaf order -- but they name the same shapes)
    pa = np.array([sah.desc.prims[int(i)].shape for i in a.view(np.int32)[hit, 0]])
    pb = np.array([hl.desc.prims[int(i)].shape for i in b.view(np.int32)[hit, 0]])
    assert np.array_equal(pa, pb)
    # and the render under it is the SAH render up to the order the leaves are met in
    small_sah = pt.Scene(text=text, base_dir=base, spp=2, xres=64, yres=64)
    small_hl = pt.Scene(text=_with_hlbvh(text), base_dir=base, spp=2, xres=64, yres=64)
    fa, wa, ca, _ = ob.render(small_sah, n_threads=4)
    fb, wb, cb, _ = ob.render(small_hl, n_threads=4)
    assert ca.camera_rays == cb.camera_rays and np.array_equal(wa, wb)
    assert np.sqrt(((fa.astype(np.float64) - fb) ** 2).sum() / (fa.astype(np.float64) ** 2).sum()) < 1e-3


def test_host_hlbvh_on_random_scenes_and_maxnodeprims(pt, ob, tmp_path, monkeypatch):
    monkeypatch.setenv("MIPT_HLBVH", "host")
    st.write_texture_files(str(tmp_path))
    st.write_alpha_png(str(tmp_path))
    for seed in range(6):
        s = pt.Scene(text=_with_hlbvh(st.random_scene(seed), maxprims=2 + seed % 3), base_dir=str(tmp_path))
        assert s.errors == []
        _check_tree(s, 2 + seed % 3)
        f, w, c, _ = ob.render(s, n_threads=4)
        assert np.isfinite(f).all()


@pytest.mark.gpu
def test_device_hlbvh_equals_the_host_tree_node_for_node(pt, ob, tmp_path, monkeypatch):
    """mi_bvh_build_hlbvh against the host restatement: killeroo (66 533 primitives), fuzz scenes, and the 10 000 002-triangle
    scene (build time reported; target < 0.5 s)."""
    st.write_texture_files(str(tmp_path))
    st.write_alpha_png(str(tmp_path))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_procedural_scene as mps
    big = tmp_path / "proc.pbrt"
    with open(big, "w") as fh:
        mps.write_scene(fh, 10_000_000, 64, 1, 7, 5)
    cases = [("killeroo", dict(text=_with_hlbvh(open(KILLEROO).read()), base_dir=os.path.dirname(KILLEROO), spp=1))]
    cases += [("random %d" % k, dict(text=_with_hlbvh(st.random_scene(k), maxprims=2 + k % 3), base_dir=str(tmp_path))) for k in range(4)]
    cases.append(("procedural 10M", dict(text=_with_hlbvh(open(big).read()), base_dir=str(tmp_path))))
    for name, kw in cases:
        monkeypatch.setenv("MIPT_HLBVH", "host")
        host = pt.Scene(**kw)
        monkeypatch.delenv("MIPT_HLBVH")
        dev = pt.Scene(**kw)
        assert host.stats["accel_on_device"] == 0 and dev.stats["accel_on_device"] == 1, name
        assert dev.desc.n_nodes == host.desc.n_nodes and dev.desc.n_prims == host.desc.n_prims, name
        assert np.array_equal(_nodes(dev).view(np.uint8), _nodes(host).view(np.uint8)), name
        pd = np.ctypeslib.as_array(dev.desc.prims, (dev.desc.n_prims,))
        ph = np.ctypeslib.as_array(host.desc.prims, (host.desc.n_prims,))
        assert np.array_equal(pd.view(np.uint8), ph.view(np.uint8)), name


@pytest.mark.gpu
def test_render_under_the_device_built_hlbvh_matches_the_oracle(pt, ob):
    """The HIP path traversing a device-built HLBVH against the oracle traversing the same tree: exact-mode parity."""
    text = _with_hlbvh(open(KILLEROO).read())
    s = pt.Scene(text=text, base_dir=os.path.dirname(KILLEROO), spp=4, xres=200, yres=200)
    assert s.stats["accel_on_device"] == 1
    integ = pt.CreatePathIntegrator(s)
    film, weight = integ.Render()
    with ob.exact_libm():
        ofilm, oweight, oc, _ = ob.render(s)
    c, o = integ.counters.as_dict(), oc.as_dict()
    for k in ("camera_rays", "regular_rays", "shadow_rays", "total_paths", "zero_radiance_paths", "path_length_sum"):
        assert abs(c[k] - o[k]) <= 2, (k, c[k], o[k])
    assert np.array_equal(weight, oweight)
    d = film.astype(np.float64) - ofilm
    assert np.sqrt((d ** 2).sum() / (ofilm.astype(np.float64) ** 2).sum()) < 1e-6


# ------------------------------------------------------------------ the build stage by stage, on raw bounds
# mi_bvh_build_host (libmipt_host.so) and mi_bvh_build_hlbvh (libmipt_hip.so) take the same n x 6 float32 array, so the
# inputs below need no scene text: synthetic boxes from seeded generators, one family per thing that can go wrong.
NODE_DT = np.dtype([("bmin", "<f4", 3), ("bmax", "<f4", 3), ("offset", "<i4"), ("n_prims", "<u2"), ("axis", "u1"), ("pad", "u1")])
SPLIT_SAH, SPLIT_MIDDLE, SPLIT_EQUAL, SPLIT_HLBVH = 0, 1, 2, 3     # MI_BVH_SPLIT_*, include/mi_scene.h
MI_ERR_UNSUPPORTED = -4
TILE = 1024                                                        # HB_TILE of hlbvh.hip: elements per block of the split sort


def _host_build(pt, bounds, max_prims, method=SPLIT_HLBVH):
    """-> (status, nodes [NODE_DT], order [int32], message)"""
    lib = pt.host_lib()
    lib.mi_bvh_build_host.argtypes = [C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p]
    b = np.ascontiguousarray(bounds, np.float32).reshape(-1, 6)
    nodes = np.zeros(2 * len(b) + 1, NODE_DT)
    order = np.full(len(b), -1, np.int32)
    n_nodes = C.c_uint32(12345)
    rc = lib.mi_bvh_build_host(b.ctypes.data, len(b), max_prims, method, nodes.ctypes.data, len(nodes), C.byref(n_nodes), order.ctypes.data)
    return rc, nodes[:n_nodes.value], order, lib.mi_scene_last_error().decode()


def _device_build(pt, bounds, max_prims):
    """mi_bvh_build_hlbvh with the front end's own upper-tree callback (mi_bvh_upper_sah) -> (status, nodes, order, message)"""
    hip, host = pt.hip_lib(), pt.host_lib()
    hip.mi_bvh_build_hlbvh.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                       C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_double)]
    hip.mi_bvh_last_error.restype = C.c_char_p
    b = np.ascontiguousarray(bounds, np.float32).reshape(-1, 6)
    nodes = np.zeros(2 * len(b) + 1, NODE_DT)
    order = np.full(len(b), -1, np.int32)
    n_nodes, secs = C.c_uint32(12345), C.c_double(0)
    rc = hip.mi_bvh_build_hlbvh(0, b.ctypes.data, len(b), max_prims, C.cast(host.mi_bvh_upper_sah, C.c_void_p), None, nodes.ctypes.data, len(nodes),
                                C.byref(n_nodes), order.ctypes.data, C.byref(secs))
    return rc, nodes[:n_nodes.value], order, hip.mi_bvh_last_error().decode()


def _boxes(centre, half):
    """Boxes [centre - half, centre + half] in float32. Where both are small dyadic numbers the sums are exact, and so is
    the centroid .5f * min + .5f * max = centre."""
    c, h = np.asarray(centre, np.float32), np.asarray(half, np.float32)
    return np.concatenate([c - h, c + h], axis=1).astype(np.float32)


def _dyadic(rng, shape, lo, hi, step):
    return (rng.integers(int(round(lo / step)), int(round(hi / step)) + 1, shape) * step).astype(np.float32)


def _tails(n):
    """Uniform random boxes about the origin (negative coordinates). A quarter of them stand on the plane z = 0 with
    min z = -0.0 or +0.0, and some have a zero max x: leaves and interior nodes whose extreme is a zero of either sign,
    where std::min / std::max keep the first of the two and fminf / fmaxf order them."""
    rng = np.random.default_rng(1000 + n)
    b = _boxes(rng.uniform(-10, 10, (n, 3)), rng.uniform(0, 1, (n, 3)))
    k = rng.random(n)
    floor = k < .25
    b[floor, 2] = np.where(rng.random(floor.sum()) < .5, np.float32(-0.0), np.float32(0.0))
    b[floor, 5] = rng.uniform(0, .5, floor.sum())
    wall = (k >= .25) & (k < .35)
    b[wall, 3] = np.where(rng.random(wall.sum()) < .5, np.float32(-0.0), np.float32(0.0))
    b[wall, 0] = -rng.uniform(0, .5, wall.sum())
    return b


def _lattice(n, side=64):
    """n boxes with centroids on a side^3 lattice (n / side^3 of them per point, with one code each) and jittered extents."""
    rng = np.random.default_rng(n)
    return _boxes(rng.integers(0, side, (n, 3)), _dyadic(rng, (n, 3), 1 / 64, .5, 1 / 64))


def _equal_identical():
    return np.tile(np.array([[-1.5, 2, 3, -1, 2.25, 4]], np.float32), (300, 1))


def _equal_lattice8():
    rng = np.random.default_rng(8)
    return _boxes(rng.integers(0, 2, (5000, 3)) * 4 - 2, _dyadic(rng, (5000, 3), 1 / 64, 1, 1 / 64))


def _equal_cluster():
    rng = np.random.default_rng(9)
    b = np.concatenate([_boxes(rng.uniform(-5, 5, (3000, 3)), rng.uniform(0, .3, (3000, 3))),
                        _boxes(np.tile(np.array([[1.25, -2.5, .75]], np.float32), (400, 1)), _dyadic(rng, (400, 3), 1 / 64, 1, 1 / 64))])
    return b[rng.permutation(len(b))]


def _flat(axes):
    """600 boxes whose centroids agree exactly on the axes named (one: a plane, two: a line, three: a point)."""
    rng = np.random.default_rng(70 + sum(1 << a for a in axes))
    c = rng.uniform(-4, 4, (600, 3)).astype(np.float32)
    h = rng.uniform(0, .5, (600, 3)).astype(np.float32)
    for a in axes:
        c[:, a] = (-2.5, 0.0, 3.75)[a]
        h[:, a] = _dyadic(rng, 600, 0, 1, 1 / 64)
    return _boxes(c, h)


def _full_treelet_table():
    """Three boxes in every cell of the 16^3 grid of the top 12 code bits, centroids spanning [0, 1]^3 exactly, so that all
    4096 treelets exist; then 40 cells are thinned to one box (singleton treelets) and the cell beside the first of them
    is filled up to 2000."""
    rng = np.random.default_rng(4096)
    cell = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3)
    cells = np.repeat(cell, 3, axis=0)
    single = rng.choice(4096, 40, replace=False)
    keep = np.ones(len(cells), bool)
    keep[np.concatenate([3 * single + 1, 3 * single + 2])] = False
    crowd = cell[single[0]].copy()
    crowd[0] += 1 if crowd[0] < 15 else -1
    cells = np.concatenate([cells[keep], np.tile(crowd, (1997, 1))])
    c = (cells + _dyadic(rng, cells.shape, 1 / 8, 7 / 8, 1 / 64)) / np.float32(16)
    c = np.concatenate([c, [[0, 0, 0], [1, 1, 1]]]).astype(np.float32)     # (cells 0,0,0 and 15,15,15 are not among the thinned: checked by the treelet count)
    b = _boxes(c, _dyadic(rng, c.shape, 0, 1 / 32, 1 / 256))
    return b[rng.permutation(len(b))]


def _one_cell(k):
    """k boxes with centroids inside one cell of the 1024^3 Morton grid, and two far boxes that span the grid."""
    rng = np.random.default_rng(k)
    return np.concatenate([_boxes(rng.uniform(.1, .9, (k, 3)), rng.uniform(0, .2, (k, 3))),
                           _boxes([[-1000, -1000, -1000], [1000, 1000, 1000]], [[1, 1, 1], [1, 1, 1]])])


TAIL_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)     # the wave, the block, the tile, +-1; four tiles + 1
SCAN_SIZES = (TILE * 1024 + 1, 2 * TILE * 1024 + TILE + 1)                 # 1025 tiles: k_scan_single's second round with one live element; 2050
FAMILIES = {}                                                              # name -> (generator, its arguments, maxnodeprims)
for _n in TAIL_SIZES:
    for _mp in (1, 4, 255):
        FAMILIES["tails-%d-maxprims%d" % (_n, _mp)] = (_tails, (_n,), _mp)
for _n in SCAN_SIZES:
    FAMILIES["scan-carry-%d" % _n] = (_lattice, (_n,), 255)
FAMILIES["equal-300-identical"] = (_equal_identical, (), 4)
FAMILIES["equal-5000-on-8-points"] = (_equal_lattice8, (), 4)
FAMILIES["equal-3000-plus-400-on-one-centre"] = (_equal_cluster, (), 4)
for _axes in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)):
    FAMILIES["flat-" + "".join("xyz"[a] for a in _axes)] = (_flat, (_axes,), 4)
FAMILIES["full-treelet-table"] = (_full_treelet_table, (), 4)
_CACHE = {}


def _family(pt, name):
    """(bounds, maxnodeprims, the host build's nodes, its order): made once, shared by the CPU and the GPU test, never written to."""
    if name not in _CACHE:
        gen, args, mp = FAMILIES[name]
        b = gen(*args)
        rc, nodes, order, msg = _host_build(pt, b, mp)
        assert rc == 0, msg
        for a in (b, nodes, order):
            a.setflags(write=False)
        _CACHE[name] = (b, mp, nodes, order)
    return _CACHE[name]


def _check_flat_tree(nodes, order, n):
    """_check_tree without the walk: every primitive in exactly one leaf, every non-root node the child of exactly one
    interior node, first child = i + 1 < second child, every child's box inside its parent's."""
    N = len(nodes)
    off, npr = nodes["offset"].astype(np.int64), nodes["n_prims"].astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(n))
    leaf, inner = np.flatnonzero(npr > 0), np.flatnonzero(npr == 0)
    assert len(inner) == len(leaf) - 1
    by = leaf[np.argsort(off[leaf], kind="stable")]
    assert off[by[0]] == 0 and (off[by[1:]] == off[by[:-1]] + npr[by[:-1]]).all() and off[by[-1]] + npr[by[-1]] == n
    first, second = inner + 1, off[inner]
    assert (first < second).all() and (second < N).all()
    assert np.array_equal(np.sort(np.concatenate([first, second])), np.arange(1, N))
    for c in (first, second):
        assert (nodes["bmin"][c] >= nodes["bmin"][inner]).all() and (nodes["bmax"][c] <= nodes["bmax"][inner]).all()
    assert (nodes["pad"] == 0).all() and (nodes["axis"] <= 2).all() and (nodes["axis"][leaf] == 0).all()


def _subtree_cover(nodes):
    """{(first position, count) of the primitives below a node: the node}; no two nodes cover the same run."""
    off, npr = nodes["offset"].tolist(), nodes["n_prims"].tolist()
    lo, cnt = [0] * len(off), [0] * len(off)
    for i in range(len(off) - 1, -1, -1):
        if npr[i] > 0:
            lo[i], cnt[i] = off[i], npr[i]
        else:
            lo[i], cnt[i] = min(lo[i + 1], lo[off[i]]), cnt[i + 1] + cnt[off[i]]
    cover = {(lo[i], cnt[i]): i for i in range(len(off))}
    assert len(cover) == len(off)
    return cover


@pytest.mark.parametrize("name", list(FAMILIES))
def test_host_hlbvh_equals_the_numpy_restatement_of_the_reference(pt, name):
    """The host build against tests/hlbvh_reference.py (written from the reference's bvh.cpp:404-532 alone): the primitive
    order is the stable sort by the reference's codes; every treelet, found in the flat array by the primitives it covers,
    has the reference's nodes in the reference's order -- counts, children, first primitives and axes exactly, bounds as
    float values (a zero may differ in sign: std::min / std::max keep the first of -0.0 and +0.0, np.minimum / np.maximum
    need not; the tails family has such nodes); what is left over is the upper tree's treelets - 1 interior nodes; the
    whole array is a tree over all primitives; and a leaf has fewer than maxnodeprims primitives unless they share one code."""
    b, mp, nodes, order = _family(pt, name)
    n = len(b)
    ref = hr.build(b, mp)
    assert np.array_equal(order, ref.order)
    _check_flat_tree(nodes, order, n)
    cover = _subtree_cover(nodes)
    n_treelets = len(ref.starts) - 1
    in_treelet = np.zeros(len(nodes), bool)
    for t in range(n_treelets):
        want = ref.treelet(t)
        root = cover[(int(ref.starts[t]), int(ref.starts[t + 1] - ref.starts[t]))]
        got = nodes[root:root + len(want)]
        assert len(got) == len(want) and not in_treelet[root:root + len(want)].any(), (name, t)
        in_treelet[root:root + len(want)] = True
        is_leaf = want["n_prims"] > 0
        assert np.array_equal(got["n_prims"], want["n_prims"]), (name, t)
        assert np.array_equal(got["offset"], np.where(is_leaf, want["second"], want["second"] + root)), (name, t)
        assert np.array_equal(got["axis"], want["axis"]), (name, t)
        assert np.array_equal(got["bmin"], want["bmin"]) and np.array_equal(got["bmax"], want["bmax"]), (name, t)
    assert (~in_treelet).sum() == n_treelets - 1 and (nodes["n_prims"][~in_treelet] == 0).all()
    sc = ref.codes[ref.order]
    big = np.flatnonzero(nodes["n_prims"] >= min(mp, 255))
    first, last = nodes["offset"][big], nodes["offset"][big] + nodes["n_prims"][big].astype(np.int64) - 1
    assert (sc[first] == sc[last]).all()
    # the families are what their names say
    if name.startswith("scan-carry"):
        assert -(-n // TILE) > 1024 and len(nodes) < 100000
    if name == "equal-300-identical":
        assert len(nodes) == 1 and nodes["n_prims"][0] == 300
    if name == "equal-5000-on-8-points":
        assert len(np.unique(ref.codes)) == 8 and nodes["n_prims"].max() > 255
    if name == "equal-3000-plus-400-on-one-centre":
        assert nodes["n_prims"].max() >= 400
    if name.startswith("flat-"):
        c = np.float32(.5) * b[:, :3] + np.float32(.5) * b[:, 3:]
        flat = [a for a in range(3) if c[:, a].min() == c[:, a].max()]
        assert flat == ["xyz".index(ch) for ch in name[5:]]
        per_axis = [ref.codes & np.uint32(0x9249249 << a) for a in range(3)]
        assert all((per_axis[a] == 0).all() == (a in flat) for a in range(3))
    if name == "full-treelet-table":
        sizes = np.diff(ref.starts)
        assert n_treelets == 4096 and (sizes == 1).sum() >= 38 and sizes.max() == 2000
    if name.startswith("tails-") and n >= 1023:
        zero_min = (nodes["bmin"][:, 2] == 0) & (nodes["n_prims"] != 1)
        assert zero_min.sum() > 5 and len(np.unique(np.signbit(nodes["bmin"][zero_min, 2]))) == 2


def test_maxnodeprims_beyond_255_is_255(pt):
    b, _, nodes, order = _family(pt, "tails-4097-maxprims255")
    rc, nodes2, order2, msg = _host_build(pt, b, 100000)
    assert rc == 0 and np.array_equal(nodes2.view(np.uint8), nodes.view(np.uint8)) and np.array_equal(order2, order)


def _coincident(k):
    """k boxes of different extents about one centre (plus nothing else): no builder can separate them."""
    rng = np.random.default_rng(k)
    return _boxes(np.tile(np.array([[.5, -1.25, 2]], np.float32), (k, 1)), _dyadic(rng, (k, 3), 1 / 64, 1, 1 / 64))


def test_a_leaf_of_more_than_65535_primitives_is_an_error_of_the_host_builders(pt):
    """LinearBVHNode::nPrimitives has 16 bits and the reference CHECKs larger leaves away (bvh.cpp:646). 65 535 primitives
    in one leaf are a tree; 65 536 (a count that wraps to 0: an interior node) and 70 000 are an error with a message and
    without a tree, from the HLBVH build (one Morton code) and from the SAH / middle / equal-counts build (one centre)."""
    rc, nodes, order, msg = _host_build(pt, _coincident(65535), 4, SPLIT_SAH)
    assert rc == 0 and len(nodes) == 1 and nodes["n_prims"][0] == 65535
    rc, nodes, order, msg = _host_build(pt, _one_cell(65535), 4)
    assert rc == 0 and nodes["n_prims"].max() == 65535
    _check_flat_tree(nodes, order, 65537)
    for bounds, methods in ((_coincident(65536), (SPLIT_SAH, SPLIT_HLBVH)), (_coincident(70000), (SPLIT_SAH, SPLIT_MIDDLE, SPLIT_EQUAL, SPLIT_HLBVH)),
                            (_one_cell(65536), (SPLIT_HLBVH,)), (_one_cell(70000), (SPLIT_HLBVH,))):
        for method in methods:
            rc, nodes, order, msg = _host_build(pt, bounds, 4, method)
            assert rc == MI_ERR_UNSUPPORTED and len(nodes) == 0, (len(bounds), method)
            assert "65535" in msg and str(len(bounds) if len(bounds) in (65536, 70000) else len(bounds) - 2) in msg, msg
    rc, nodes, order, msg = _host_build(pt, _one_cell(70000), 4, SPLIT_SAH)      # (different centres: SAH separates them)
    assert rc == 0 and nodes["n_prims"].max() <= 4


def _shared_centre_mesh(k, seed, extra=6):
    """Shape text of k random triangles whose bounding boxes all have the centre (0, 0, 5 -> moved by a Translate) -- on every
    axis one vertex at -e, one at +e and the third between, so .5f * min + .5f * max is exactly 0 -- and `extra` ordinary
    triangles around them, so that the tree has interior nodes."""
    rng = np.random.default_rng(seed)
    e = rng.uniform(.2, 1, (k, 3)).astype(np.float32)
    P = np.zeros((k, 3, 3), np.float32)
    for a in range(3):
        who = np.argsort(rng.random((k, 3)), axis=1)          # which vertex is at -e, which at +e, which between
        rows = np.arange(k)
        P[rows, who[:, 0], a] = -e[:, a]
        P[rows, who[:, 1], a] = e[:, a]
        P[rows, who[:, 2], a] = (rng.uniform(-1, 1, k) * e[:, a]).astype(np.float32)
    far = (rng.uniform(-3, 3, (extra, 1, 3)) + rng.uniform(-.7, .7, (extra, 3, 3))).astype(np.float32)
    far[:, :, rng.integers(0, 3)] += np.where(rng.random((extra, 1)) < .5, -3, 3)
    P = np.concatenate([P, far]).reshape(-1, 3)
    return ('Shape "trianglemesh" "integer indices" [%s] "point P" [%s]\n'
            % (" ".join(map(str, range(len(P)))), " ".join(repr(float(v)) for v in P.ravel())))


def _shared_centre_scene(pt, k, hlbvh, seed=5):
    text = st._HEAD % dict(res=8, spp=1, depth=1, extra="") + 'LightSource "point" "rgb I" [1 1 1]\n' + _shared_centre_mesh(k, seed) + "WorldEnd\n"
    return pt.Scene(text=_with_hlbvh(text) if hlbvh else text)


@pytest.mark.parametrize("hlbvh", [False, True], ids=["sah", "hlbvh"])
def test_a_scene_with_70000_triangles_about_one_centre_has_the_error(pt, monkeypatch, hlbvh):
    """The front end: "reported as an error, never silently dropped" -- no tree, no primitives, the message in Scene.errors."""
    monkeypatch.setenv("MIPT_HLBVH", "host")
    s = _shared_centre_scene(pt, 70000, hlbvh, seed=6)
    assert s.stats["n_triangles"] == 70006
    assert len(s.errors) == 1 and "a leaf would hold 70000 primitives" in s.errors[0] and "more than 65535" in s.errors[0]
    assert s.desc.n_nodes == 0 and s.desc.n_prims == 0 and s.stats["leaf_nodes"] == 0 and s.stats["accel_on_device"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FAMILIES))
def test_device_hlbvh_on_raw_bounds_equals_the_host_build(pt, name):
    """mi_bvh_build_hlbvh(..., mi_bvh_upper_sah, ...) on the arrays of the CPU test: node array and primitive order byte-equal
    to mi_bvh_build_host's, and the order equal to numpy's stable sort of the reference's codes -- which names the sort
    (k_split_count / k_scan_single / k_split_scatter) when it is the sort that is wrong."""
    b, mp, nodes, order = _family(pt, name)
    rc, dnodes, dorder, msg = _device_build(pt, b, mp)
    assert rc == 0, msg
    assert np.array_equal(dorder, np.argsort(hr.morton_codes(b), kind="stable")), "the sort"
    assert np.array_equal(dorder, order)
    assert len(dnodes) == len(nodes) and np.array_equal(dnodes.view(np.uint8), nodes.view(np.uint8))


@pytest.mark.gpu
def test_device_hlbvh_refuses_a_leaf_of_more_than_65535_primitives(pt, monkeypatch):
    """70 000 boxes in one Morton cell: k_emit_lbvh keeps the node a leaf (count clamped, never wrapped) and flags it,
    mi_bvh_build_hlbvh returns MI_ERR_UNSUPPORTED with a message, and the next build is none the worse. 65 535 are a tree.
    The front end reports the device's refusal as the scene's error and builds no other tree instead."""
    rc, nodes, order, msg = _device_build(pt, _one_cell(70000), 4)
    assert rc == MI_ERR_UNSUPPORTED and len(nodes) == 0 and "70000" in msg and "65535" in msg, (rc, msg)
    b, mp, hnodes, horder = _family(pt, "tails-4097-maxprims4")
    rc, nodes, order, msg = _device_build(pt, b, mp)
    assert rc == 0 and np.array_equal(order, horder) and np.array_equal(nodes.view(np.uint8), hnodes.view(np.uint8)), msg
    edge = _one_cell(65535)
    rc, nodes, order, msg = _device_build(pt, edge, 4)
    hrc, hnodes, horder, _ = _host_build(pt, edge, 4)
    assert rc == 0 and hrc == 0 and nodes["n_prims"].max() == 65535, msg
    assert np.array_equal(order, horder) and np.array_equal(nodes.view(np.uint8), hnodes.view(np.uint8))
    monkeypatch.delenv("MIPT_HLBVH", raising=False)
    s = _shared_centre_scene(pt, 70000, True, seed=6)
    assert len(s.errors) == 1 and "device build" in s.errors[0] and "70000" in s.errors[0], s.errors
    assert s.desc.n_nodes == 0 and s.desc.n_prims == 0 and s.stats["accel_on_device"] == 0


# ------------------------------------------------------------------ large leaves through the traversal kernels
_LEAF_RAYS = {}


def _large_leaf_case(pt, ob, k, hlbvh):
    """The scene (built on the host: the same tree with or without a device), 20 000 rays from inside the world's box, and
    the oracle's answers to them -- once per (k, split method), shared by the three traversal variants."""
    key = (k, hlbvh)
    if key not in _LEAF_RAYS:
        os.environ["MIPT_HLBVH"] = "host"
        try:
            s = _shared_centre_scene(pt, k, hlbvh)
        finally:
            del os.environ["MIPT_HLBVH"]
        rng = np.random.default_rng(k)
        rays = _rays(rng, s, 20000)
        aimed = rng.random(20000) < .5                   # half of them at the cluster, which is a small part of the world's box
        rays[aimed, 3:6] = rng.uniform(-.6, .6, (int(aimed.sum()), 3)).astype(np.float32) - rays[aimed, 0:3]
        def oracle(r, any_hit):      # (oracle_trace takes the rays one after another; eight slices of them side by side)
            with ThreadPoolExecutor(8) as pool:
                return np.concatenate(list(pool.map(lambda part: ob.trace(s, part, any_hit=any_hit)[0], np.array_split(r, 8))))
        closest, anyhit, shadow = oracle(rays, False), oracle(rays, True), oracle(tc.shadow_form(rays), True)
        _LEAF_RAYS[key] = (s, rays, closest, anyhit, shadow.view(np.int32)[:, 0] >= 0)
    return _LEAF_RAYS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"MIPT_BVH_WIDTH": "2"}, {"MIPT_NO_COOP_LEAVES": "1"}], ids=["wide4", "wide2", "no-coop-leaves"])
@pytest.mark.parametrize("hlbvh", [False, True], ids=["sah", "hlbvh"])
@pytest.mark.parametrize("k", [300, 5000, 16383])
def test_a_leaf_of_hundreds_to_16383_triangles_traces_like_the_oracle(pt, ob, monkeypatch, k, hlbvh, env):
    """Triangles whose boxes share one centre end in ONE leaf under every split method (bvh.cpp:289-300; one Morton code):
    256 ... 16 383 primitives, the range between what maxnodeprims allows and what the traversal records hold
    (LEAF_COUNT_MASK). mi_pt_trace closest-hit and any-hit, and the render's own kernels (k_trav's cooperative leaf test
    in 64-pair rounds, the BVH2 records, the one-primitive-per-pass leaf path), bit-equal to the oracle's records."""
    s, rays, closest, anyhit, shadow = _large_leaf_case(pt, ob, k, hlbvh)
    assert s.errors == [] and s.stats["n_triangles"] == k + 6
    leaves = _nodes(s)["n_prims"]
    assert leaves.max() == k and (leaves > 0).sum() > 1
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    integ = pt.CreatePathIntegrator(s)
    assert np.array_equal(integ.trace(rays).view(np.int32), closest.view(np.int32))
    assert np.array_equal(integ.trace(rays, any_hit=True).view(np.int32), anyhit.view(np.int32))
    tc.check_wavefront(integ, rays, lambda r: closest, lambda r: shadow)      # (the rays are unbounded: modes 0 and 2 ask the same question)
    prim = closest.view(np.int32)[:, 0]
    in_leaf = prim[prim >= 0]
    assert (prim >= 0).mean() > .2 and len(np.unique(in_leaf)) > min(k, 2000) // 4       # (the winners are spread over the leaf)
    integ.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hlbvh", [False, True], ids=["sah", "hlbvh"])
def test_a_leaf_of_16384_triangles_is_refused_by_the_renderer(pt, monkeypatch, hlbvh):
    monkeypatch.setenv("MIPT_HLBVH", "host")
    s = _shared_centre_scene(pt, 16384, hlbvh)
    assert s.errors == [] and _nodes(s)["n_prims"].max() == 16384
    with pytest.raises(RuntimeError, match="more than 16383"):
        pt.CreatePathIntegrator(s)
