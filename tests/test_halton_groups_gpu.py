"""The Halton routines of the shading kernel, query by query (PathIntegrator.sampler_probe, mi_pt_sampler_probe): the grouped
routines -- five dimensions of the direct-lighting estimate, two of the next direction, one of the roulette draw; per-dimension
records, digit loops interleaved, 32-bit indices -- and the single-dimension routine with its 64-bit loop, bit for bit against
the oracle's ScrambledRadicalInverse (oracle_scrambled_radical_inverse).

First dimensions 2 .. 60, and 995 (five) / 998 (two) / 999 (one), where a group ends at the tables' last dimension. Indices, for
the bases of every group: 0, 1, b - 1, b, b^k - 1 and b^k for every k that fits 32 bits, 2^32 - 1; 4096 seeded random 32-bit
indices per routine; and 2^32, 2^40 + 12345, 2^63 - 1 through the 64-bit loop. The queries of a launch are shuffled, so the
lanes of a wave hold different first dimensions and digit counts: the interleaved loops run with some chains finished and
others not. About 5 x 10^4 values from the grouped routines and as many from the single-dimension routine."""
import numpy as np
import pytest

import scenes_text as st

pytestmark = pytest.mark.gpu

FIRST_DIMS = list(range(2, 61))
N_DIMS = 1000
WIDE = (2 ** 32, 2 ** 40 + 12345, 2 ** 63 - 1)


@pytest.fixture(scope="module")
def halton(pt, ob):
    s = pt.Scene(text=st.furnace_point(res=8, spp=1, depth=124))   # (8 dimensions per bounce: the deepest path the 1000 dimensions hold)
    assert s.errors == [] and s.desc.sampler.n_dims == N_DIMS
    primes = [int(s.desc.sampler.primes[i]) for i in range(N_DIMS)]
    assert primes[2] == 5 and primes[999] == 7919
    integ = pt.CreatePathIntegrator(s)
    fn, ptr, cache = ob.lib().oracle_scrambled_radical_inverse, s.desc_ptr, {}

    def oracle(dim, index):
        key = (int(dim), int(index))
        if key not in cache:
            cache[key] = np.float32(fn(ptr, key[0], key[1]))
        return cache[key]
    return integ, primes, oracle


def _edge_indices(bases):
    idx = {0, 1, 2 ** 32 - 1}
    for b in bases:
        idx.update((b - 1, b))
        p = b
        while p < 2 ** 32:
            idx.update((p - 1, p))
            p *= b
        if p - 1 < 2 ** 32:
            idx.add(p - 1)
    assert all(0 <= i < 2 ** 32 for i in idx)
    return sorted(idx)


def _queries(primes, group, last_first_dim, seed):
    """(indices, first dimensions) of the routine that draws `group` dimensions: the edge indices of each group's bases, 4096
    random indices over the first dimensions in turn, shuffled."""
    firsts = FIRST_DIMS + [last_first_dim]
    assert last_first_dim + group == N_DIMS
    idx, dims = [], []
    for d in firsts:
        e = _edge_indices(primes[d:d + group])
        idx += e
        dims += [d] * len(e)
    rng = np.random.RandomState(seed)
    idx += [int(v) for v in rng.randint(0, 2 ** 32, size=4096, dtype=np.uint64)]
    dims += [firsts[i % len(firsts)] for i in range(4096)]
    order = rng.permutation(len(idx))
    return np.array(idx, np.uint64)[order], np.array(dims, np.int32)[order]


def _digits(index, base):
    n = 0
    while index:
        index //= base
        n += 1
    return n


def _expected(oracle, idx, dims, group):
    return np.array([[oracle(d + k, i) for k in range(group)] for i, d in zip(idx.tolist(), dims.tolist())], np.float32)


def _assert_bits(got, want, idx, dims):
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, [(int(idx[q]), int(dims[q]) + int(k), float(got[q, k]), float(want[q, k])) for q, k in bad[:8]]


@pytest.mark.parametrize("group,last,seed", [(5, 995, 11), (2, 998, 12), (1, 999, 13)])
def test_grouped_routines_match_the_oracle_bit_for_bit(halton, group, last, seed):
    integ, primes, oracle = halton
    idx, dims = _queries(primes, group, last, seed)
    # the first wave: several first dimensions, and chains of several lengths side by side
    assert len(set(dims[:64].tolist())) > 8
    assert len({_digits(int(i), primes[int(d)]) for i, d in zip(idx[:64], dims[:64])}) > 3
    got = integ.sampler_probe(group, idx, dims)
    assert got.shape == (len(idx), group)
    want = _expected(oracle, idx, dims, group)
    assert (want >= 0).all() and (want < 1).all()
    _assert_bits(got, want, idx, dims)
    # the single-dimension routine at the same (index, dimension) pairs
    flat_idx, flat_dims = np.repeat(idx, group), (dims[:, None] + np.arange(group, dtype=np.int32)[None, :]).reshape(-1)
    _assert_bits(integ.sampler_probe(0, flat_idx, flat_dims), want.reshape(-1, 1), flat_idx, flat_dims)


def test_single_dimension_routine_beyond_32_bits(halton):
    integ, primes, oracle = halton
    dims = np.array(sorted(set(d + k for d in FIRST_DIMS for k in range(5)) | set(range(995, 1000))), np.int32)
    idx = np.array([w for w in WIDE for _ in dims], np.uint64)
    dims = np.tile(dims, len(WIDE))
    order = np.random.RandomState(14).permutation(len(idx))
    idx, dims = idx[order], dims[order]
    _assert_bits(integ.sampler_probe(0, idx, dims), _expected(oracle, idx, dims, 1), idx, dims)


def test_what_the_probe_refuses(halton):
    integ = halton[0]
    for group, index, dim, what in ((5, 1, 996, "dimensions"), (2, 1, 999, "dimensions"), (1, 1, 1000, "dimensions"), (0, 1, 1, "dimensions"),
                                    (5, 2 ** 32, 2, "32-bit"), (1, 2 ** 40, 2, "32-bit"), (3, 1, 2, "group")):
        with pytest.raises(RuntimeError) as err:
            integ.sampler_probe(group, [index], [dim])
        assert "mi_pt_sampler_probe" in str(err.value) and what in str(err.value), str(err.value)
