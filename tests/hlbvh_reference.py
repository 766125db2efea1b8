"""BVHAccel::HLBVHBuild up to its treelets (src/accelerators/bvh.cpp:404-532) in numpy, written from the reference's text
and from nothing else of this project: the second opinion beside the host restatement (csrc/host/bvh.cpp) and the kernels
(csrc/device/hlbvh.hip), which share one author and one reading.

    centroids      .5f * pMin + .5f * pMax in float32                                  bvh.cpp:51-56
    codes          Bounds3::Offset in the centroids' bounds (divide only where pMax > pMin), times 1024, truncated,
                   1024 -> 1023, three-way bit interleave                               geometry.h:802-808, bvh.cpp:107-137, 414-422
    order          RadixSort is a stable sort by the 30-bit code: np.argsort(kind="stable")   bvh.cpp:139-181
    treelets       runs of equal top 12 bits                                           bvh.cpp:428-447
    emitLBVH       an explicit stack instead of the recursion; the nodes in the order the recursion creates them (a node,
                   its first subtree, its second subtree); leaves take their primitives in Morton order, which is what ONE
                   thread hands out with orderedPrimsOffset                            bvh.cpp:474-532
The reference builds no flat array before buildUpperSAH has run, and this file stops where that begins: what it returns is
per treelet, `second` counted from the treelet's own root. A test finds each treelet in a flattened tree by the primitives
it covers."""
import numpy as np

NODE = np.dtype([("bmin", np.float32, 3), ("bmax", np.float32, 3), ("second", np.int64), ("n_prims", np.int64), ("axis", np.uint8)])
TREELET_MASK = 0x3FFC0000


def _left_shift3(x):
    x = x.astype(np.uint32)
    x = np.where(x == 1 << 10, x - 1, x).astype(np.uint32)
    x = (x | (x << 16)) & 0x30000FF
    x = (x | (x << 8)) & 0x300F00F
    x = (x | (x << 4)) & 0x30C30C3
    x = (x | (x << 2)) & 0x9249249
    return x.astype(np.uint32)


def morton_codes(bounds):
    """bounds [n, 6] float32 (min xyz, max xyz) -> the 30-bit codes of the primitives, in primitive order."""
    b = np.ascontiguousarray(bounds, np.float32).reshape(-1, 6)
    half = np.float32(.5)
    c = half * b[:, :3] + half * b[:, 3:]
    assert c.dtype == np.float32
    lo, hi = c.min(axis=0), c.max(axis=0)
    o = c - lo
    for a in range(3):
        if hi[a] > lo[a]:
            o[:, a] = o[:, a] / (hi[a] - lo[a])
    v = o * np.float32(1024)
    assert v.dtype == np.float32 and (v >= 0).all() and (v <= 1024).all()
    q = v.astype(np.uint32)          # (uint32_t)float: truncation
    return (_left_shift3(q[:, 2]) << 2) | (_left_shift3(q[:, 1]) << 1) | _left_shift3(q[:, 0])


def _emit(codes, first, count, max_prims, out):
    """emitLBVH over sorted codes [first, first + count): appends (second or first primitive, n_prims, axis) in creation order."""
    base = len(out)
    stack = [(first, count, 29 - 12, -1)]
    while stack:
        f, n, bit, parent = stack.pop()
        while not (bit == -1 or n < max_prims) and ((int(codes[f]) >> bit) & 1) == ((int(codes[f + n - 1]) >> bit) & 1):
            bit -= 1                                   # no split at this bit: the same primitives, the next bit
        me = len(out) - base
        if parent >= 0:
            out[base + parent][0] = me
        if bit == -1 or n < max_prims:
            out.append([f, n, 0])
            continue
        mask = 1 << bit
        s, e = 0, n - 1
        while s + 1 != e:
            mid = (s + e) // 2
            if (int(codes[f + s]) & mask) == (int(codes[f + mid]) & mask):
                s = mid
            else:
                e = mid
        out.append([-1, 0, bit % 3])
        stack.append((f + e, n - e, bit - 1, me))      # the second child: created after the whole first subtree
        stack.append((f, e, bit - 1, -1))              # the first child: the next node


class Reference:
    """codes [n] (primitive order), order [n] (primitive numbers in leaf order), starts [T + 1] (treelet t covers sorted
    positions starts[t] : starts[t + 1]), node_starts [T + 1] and nodes (NODE records; treelet t's are
    nodes[node_starts[t] : node_starts[t + 1]], depth first, `second` relative to the treelet's root; a leaf's `second`
    is its first position in `order`)."""

    def treelet(self, t):
        return self.nodes[self.node_starts[t]:self.node_starts[t + 1]]


def build(bounds, max_prims_in_node):
    b = np.ascontiguousarray(bounds, np.float32).reshape(-1, 6)
    n = len(b)
    max_prims = min(255, int(max_prims_in_node))      # BVHAccel::BVHAccel, bvh.cpp:185
    ref = Reference()
    ref.codes = morton_codes(b)
    ref.order = np.argsort(ref.codes, kind="stable")
    sc = ref.codes[ref.order]
    top = sc & np.uint32(TREELET_MASK)
    ref.starts = np.concatenate([[0], np.flatnonzero(top[1:] != top[:-1]) + 1, [n]]).astype(np.int64)
    recs, node_starts = [], [0]
    for t in range(len(ref.starts) - 1):
        _emit(sc, int(ref.starts[t]), int(ref.starts[t + 1] - ref.starts[t]), max_prims, recs)
        node_starts.append(len(recs))
    ref.node_starts = np.array(node_starts, np.int64)
    nodes = np.zeros(len(recs), NODE)
    r = np.array(recs, np.int64).reshape(-1, 3)
    nodes["second"], nodes["n_prims"], nodes["axis"] = r[:, 0], r[:, 1], r[:, 2]
    # leaf bounds: the leaves, in creation order, cut the sorted primitives into consecutive runs
    leaf = np.flatnonzero(nodes["n_prims"] > 0)
    firsts = nodes["second"][leaf]
    assert firsts[0] == 0 and (firsts[1:] == firsts[:-1] + nodes["n_prims"][leaf][:-1]).all() and firsts[-1] + nodes["n_prims"][leaf][-1] == n
    ob = b[ref.order]
    nodes["bmin"][leaf] = np.minimum.reduceat(ob[:, :3], firsts, axis=0)
    nodes["bmax"][leaf] = np.maximum.reduceat(ob[:, 3:], firsts, axis=0)
    # interior bounds: InitInterior's Union of the children (bvh.cpp:72-78); a child has a larger index than its parent
    bmin, bmax = nodes["bmin"], nodes["bmax"]
    owner = np.repeat(np.arange(len(node_starts) - 1), np.diff(ref.node_starts))
    for k in np.flatnonzero(nodes["n_prims"] == 0)[::-1]:
        c1 = ref.node_starts[owner[k]] + nodes["second"][k]
        bmin[k] = np.minimum(bmin[k + 1], bmin[c1])
        bmax[k] = np.maximum(bmax[k + 1], bmax[c1])
    ref.nodes = nodes
    return ref
