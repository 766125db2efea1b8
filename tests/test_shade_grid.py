"""The grid of a k_shade launch (mi_pt_shade_grid: host code of the HIP library, no device) against the kernel's prologue.

k_shade finds its work from blockIdx.x alone: it walks the classes of its mask in rising order and subtracts each queue's
ceil(n / 256) blocks until the index fits (pt_kernels.hip, the head of k_shade). The host (pt_render.hip) sizes the launch from the same 16
counts, so the two must agree block for block: a grid one block short drops up to 256 vertices of the last class, and
ceil(sum / 256) instead of the sum of the ceilings drops them whenever two classes each hold a partial block. The prologue
is restated here in Python and the library's answer is held to it."""
import ctypes as C
import itertools

import pytest

BLOCK = 256
BITS = (0, 3, 7, 15)                     # the first class, two in the middle, the escaped rays' class
COUNTS = (0, 1, 255, 256, 257, 513)      # empty, one entry, one short of a block, a whole block, one over, two blocks and one
OTHERS = 300                             # what every class outside BITS holds: a mask without them must not see it


def _prologue(counts, classes, blk):
    """(class, block within its queue) of block index `blk`, or None when it lies past the queues: k_shade's walk."""
    for c in range(16):
        if not (classes >> c) & 1:
            continue
        nb = (counts[c] + BLOCK - 1) // BLOCK
        if blk < nb:
            return c, blk
        blk -= nb
    return None


def _masks():
    for k in range(1, len(BITS) + 1):
        for bits in itertools.combinations(BITS, k):
            yield sum(1 << b for b in bits)


def test_grid_is_what_the_prologue_walks(pt):
    masks = list(_masks())
    assert len(masks) == 15
    for four in itertools.product(COUNTS, repeat=len(BITS)):
        counts = [OTHERS] * 16
        for b, n in zip(BITS, four):
            counts[b] = n
        for mask in masks:
            blocks = pt.shade_grid(counts, mask)
            where = (four, hex(mask), blocks)
            assert blocks == sum((counts[c] + BLOCK - 1) // BLOCK for c in range(16) if (mask >> c) & 1), where
            seen = {}
            for blk in range(blocks):   # every block of the grid has work ...
                hit = _prologue(counts, mask, blk)
                assert hit is not None and counts[hit[0]] > hit[1] * BLOCK, where + (blk, hit)
                seen[hit[0]] = seen.get(hit[0], 0) + 1
            assert _prologue(counts, mask, blocks) is None, where   # ... and the first one past it has none
            # every entry of every class of the mask is under a block
            assert seen == {c: (counts[c] + BLOCK - 1) // BLOCK for c in range(16) if (mask >> c) & 1 and counts[c]}, where


def test_empty_queues_need_no_launch(pt):
    for mask in _masks():
        counts = [OTHERS] * 16
        for b in BITS:
            counts[b] = 0
        assert pt.shade_grid(counts, mask) == 0
    assert pt.shade_grid([OTHERS] * 16, 0) == 0
    assert pt.shade_grid([0] * 16, 0xffff) == 0


def test_sum_of_ceilings_not_ceiling_of_sum(pt):
    counts = [0] * 16
    counts[0] = counts[3] = counts[7] = 1
    assert pt.shade_grid(counts, 0b10001001) == 3
    assert pt.shade_grid([0xffffffff] * 16, 0x0003) == 2 * (1 << 24)   # (the sum is formed wider than a count)


def test_bad_arguments_are_refused(pt):
    lib = pt.hip_lib()
    invalid = lib.mi_pt_shade_instances(None, None, 0, None)   # the library's code for a null argument
    assert invalid != 0
    counts, blocks = (C.c_uint32 * 16)(), C.c_uint32(77)
    assert lib.mi_pt_shade_grid(None, 16, 1, C.byref(blocks)) == invalid
    assert lib.mi_pt_shade_grid(counts, 16, 1, None) == invalid
    for n in (0, 1, 15, 17, 32):
        assert lib.mi_pt_shade_grid(counts, n, 1, C.byref(blocks)) == invalid, n
        assert lib.mi_pt_last_error()
    assert blocks.value == 77   # a refused call writes nothing
    assert lib.mi_pt_shade_grid(counts, 16, 1, C.byref(blocks)) == 0 and blocks.value == 0
    with pytest.raises(RuntimeError):
        pt.shade_grid([1] * 15, 1)
    with pytest.raises(RuntimeError):
        pt.shade_grid([1] * 17, 1)
