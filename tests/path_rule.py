"""When a device path log (PathIntegrator.debug_path) and the oracle's (oracle_binding.path_log) count as the same path.
Shared by tools/diag/path_compare.py ("all" mode) and tests/test_debug_path_gpu.py. Record layout: include/mi_pt.h."""
import numpy as np


def paths_agree(d, o):
    """d, o: [vertices, PATH_RECORD_FLOATS] float32. True when
    - both hold the same number of vertices,
    - words 0..19 of every vertex are bit-equal, but for [12:15] and [16:20] of the last vertex (a path's last vertex spawns no
      ray that anything reads: what the two sides leave there differs),
    - the device's L = [51:82] is finite and non-negative and within rtol 1e-4, atol 1e-7 of the oracle's."""
    if len(d) != len(o):
        return False
    dg, og = d[:, :20].copy(), o[:, :20].copy()
    if len(d):
        dg[-1, 12:15] = og[-1, 12:15] = 0
        dg[-1, 16:20] = og[-1, 16:20] = 0
    if not np.array_equal(dg.view(np.uint32), og.view(np.uint32)):
        return False
    dl, ol = d[:, 51:82], o[:, 51:82]
    return bool(np.isfinite(dl).all() and not (dl < 0).any() and np.allclose(dl, ol, rtol=1e-4, atol=1e-7))
