"""The reference's tests of the scalar helpers under this path, restated -- against the oracle here, and (GPU-marked twins)
against the device's own copies through `mi_pt_math_probe`:

  FloatingPoint.NextUpDownFloat   src/tests/fp_tests.cpp:29-47     NextFloatUp / NextFloatDown (OffsetRayOrigin, EFloat)
  EFloat.{Add,Sub,Mul,Div}        src/tests/fp_tests.cpp:166-260   interval arithmetic under Sphere::Intersect's quadratic
  FindInterval.Basics             src/tests/find_interval.cpp:8    the search inside Distribution1D::SampleDiscrete

and, with no counterpart in the reference, the divisions of the spectral passes (d_math.h DivBy, d_bsdf.h DivFast / DivTrack;
mi_pt_math_probe op 6) against IEEE division and a float32 emulation of the algorithm.

(EFloat.Abs / EFloat.Sqrt exercise operations Sphere::Intersect does not use: Quadratic takes the root of the discriminant in
double, efloat.h:271-290. tests/bounds.cpp covers Bounds iterators, Distance and Union, none of which is on the render path:
the BVH build's use of Union is pinned by the reference's node counts, tests/test_frontend.py.)
The reference draws its operands from its PCG32 stream; containment does not depend on which operands, so these use numpy's
seeded generator with the reference's distributions (exponent uniform in [-6, 6]; no error / <= 1024 ulp / <= 2^20 ulp / up to
4 |v|) and its adversarial choice of the precise value (an end of the interval two times in three)."""
import ctypes as C

import numpy as np
import pytest

_F = C.POINTER(C.c_float)


def _oracle_probe(ob):
    lib = ob.lib()
    lib.oracle_math_probe.argtypes = [C.c_int, C.c_uint32, _F, _F, _F]

    def probe(op, x, y=None):
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(x if y is None else y, np.float32)
        out = np.zeros((len(x), 3), np.float32)
        lib.oracle_math_probe(op, len(x), x.ctypes.data_as(_F), y.ctypes.data_as(_F), out.ctypes.data_as(_F))
        return out
    return probe


def _device_probe(pt):
    return lambda op, x, y=None: pt.math_probe(op, x, y)


def _next_up_down(probe):
    inf = np.float32(np.inf)
    special = np.array([[-0.0, 0], [0.0, 0], [inf, 0], [-inf, 0]], np.float32)
    r = probe(0, special)
    assert r[0, 0] > 0 and r[1, 1] < 0                         # NextFloatUp(-0.f) > 0, NextFloatDown(0.f) < 0
    assert r[2, 0] == inf and r[2, 1] < inf                    # up(inf) == inf, down(inf) < inf
    assert r[3, 1] == -inf and r[3, 0] > -inf
    rng = np.random.default_rng(1)
    f = rng.integers(0, 1 << 32, 100000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    f = f[np.isfinite(f)]
    r = probe(0, np.stack([f, np.zeros_like(f)], 1))
    assert np.array_equal(r[:, 0], np.nextafter(f, inf)) and np.array_equal(r[:, 1], np.nextafter(f, -inf))


def _efloats(rng, n):
    """getFloat, tests/fp_tests.cpp:108-136: (value, error bound) pairs and the interval they stand for."""
    val = (10.0 ** rng.uniform(-6, 6, n)).astype(np.float32)
    kind = rng.integers(0, 4, n)
    bits = val.view(np.uint32).astype(np.uint64)
    small = (bits + rng.integers(0, 1024, n).astype(np.uint64)).astype(np.uint32).view(np.float32)
    big = (bits + rng.integers(0, 1 << 20, n).astype(np.uint64)).astype(np.uint32).view(np.float32)
    err = np.select([kind == 0, kind == 1, kind == 2], [np.zeros(n, np.float32), np.abs(small - val), np.abs(big - val)],
                    (4 * rng.random(n).astype(np.float32)) * np.abs(val)).astype(np.float32)
    v = (np.where(rng.random(n) < .5, -1, 1) * val).astype(np.float32)
    inf = np.float32(np.inf)
    low = np.where(err == 0, v, np.nextafter((v - err).astype(np.float32), -inf))    # EFloat(v, err), efloat.h:52-62
    high = np.where(err == 0, v, np.nextafter((v + err).astype(np.float32), inf))
    return np.stack([v, err], 1), low.astype(np.float64), high.astype(np.float64)


def _precise(rng, low, high):
    """getPrecise, tests/fp_tests.cpp:140-158."""
    t = rng.random(len(low)).astype(np.float32).astype(np.float64)
    mid = np.clip((1 - t) * low + t * high, low, high)
    return np.select([(k := rng.integers(0, 3, len(low))) == 0, k == 1], [low, high], mid)


def _efloat_ops(probe, n=200000):
    rng = np.random.default_rng(7)
    a, alo, ahi = _efloats(rng, n)
    b, blo, bhi = _efloats(rng, n)
    pa, pb = _precise(rng, alo, ahi), _precise(rng, blo, bhi)
    with np.errstate(all="ignore"):
        for op, fn in ((1, np.add), (2, np.subtract), (3, np.multiply), (4, np.divide)):
            r = probe(op, a, b).astype(np.float64)
            want = fn(pa, pb).astype(np.float32).astype(np.float64)   # `float preciseResult = precise[0] op precise[1]`
            ok = np.ones(n, bool)
            if op == 4:   # the denominator's interval must not straddle zero nor be wide against its centre (fp_tests.cpp:249-252)
                ok = ~((blo * bhi < 0) | ((bhi - blo) / 2 > .25 * np.abs(blo)))
                assert ok.mean() > .3
            assert (want[ok] >= r[ok, 1]).all() and (want[ok] <= r[ok, 2]).all(), op
            assert np.array_equal(r[:, 0], fn(a[:, 0], b[:, 0]).astype(np.float32).astype(np.float64), equal_nan=True)   # the value itself is the plain float result


def _find_interval(probe):
    q = lambda v: int(probe(5, np.array([[v, 0]], np.float32))[0, 0])
    assert q(-1) == 0 and q(100) == 8            # clamped to [0, size - 2]
    for i in range(9):
        assert q(i) == i and q(i + .5) == i
        if i > 0:
            assert q(i - .5) == i - 1


# ---- op 6: the divisions of the spectral passes (d_math.h DivBy, d_bsdf.h DivFast / DivTrack)
_LO_D, _HI_D, _LO_Q, _HI_Q = np.float32(1e-18), np.float32(1e18), np.float32(1e-30), np.float32(1e30)   # the literals of d_math.h


def division_operands(n=1 << 20, seed=5):
    """n pairs (x, d) of float32. Half: magnitudes log-uniform over [2^-120, 2^120], random signs. The other half next to the
    guards of DivBy: |d| within 8 ulp of 1e-18f and of 1e18f, and (x, d) whose quotient lies within about 8 ulp of 1e-30f and of
    1e30f (x = fl(q d) for such a q). In front, every pair of 0, -0, subnormals, +-inf, NaN and four ordinary values."""
    rng = np.random.default_rng(seed)

    def logu(k, lo=-120., hi=120.):
        return (np.exp2(rng.uniform(lo, hi, k)) * rng.choice([-1., 1.], k)).astype(np.float32)

    def near(v, k):   # within 8 ulp of +-v
        b = np.full(k, np.float32(v).view(np.uint32), np.int64) + rng.integers(-8, 9, k)
        return b.astype(np.uint32).view(np.float32) * rng.choice([-1., 1.], k).astype(np.float32)

    h, e = n // 2, n // 8
    x, d = [logu(h)], [logu(h)]
    for v in (_LO_D, _HI_D):
        d.append(near(v, e))
        x.append(logu(e, -40., 40.))
    for v, (lo, hi) in ((_LO_Q, (-20., 55.)), (_HI_Q, (-55., 20.))):   # (d well inside the fast range, x = q d representable)
        dd, qq = logu(e, lo, hi), near(v, e)
        d.append(dd)
        x.append((qq.astype(np.float64) * dd.astype(np.float64)).astype(np.float32))
    x, d = np.concatenate(x), np.concatenate(d)
    tiny = np.float32(1e-45)
    special = np.array([0., -0., tiny, -tiny, np.float32(1.1e-38), np.float32(-5e-39), np.inf, -np.inf, np.nan, 1., -3., 7e-31, 2.5e29], np.float32)
    sx, sd = np.meshgrid(special, special, indexing="ij")
    x[:sx.size], d[:sd.size] = sx.ravel(), sd.ravel()
    return x, d


def _round_sum_to_float32(p, q):
    """fl32(p + q) for float64 p (exact) and float32 q: the float64 sum rounded again, corrected where the float64 sum sits
    exactly half way between two float32 and is not itself exact (TwoSum's error term says which side the true sum lies)."""
    with np.errstate(all="ignore"):
        q = q.astype(np.float64)
        s = p + q
        bb = s - p
        err = (p - (s - bb)) + (q - bb)
        f = s.astype(np.float32)
        other = np.nextafter(f, np.where(s > f, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        tie = np.isfinite(s) & (err != 0) & (f.astype(np.float64) != s) & ((f.astype(np.float64) + other.astype(np.float64)) / 2 == s)
        # (the cast rounded the tie to even; the true sum lies on err's side of s: the float32 nearest to the next double there)
        up = np.nextafter(s, np.inf).astype(np.float32)
        down = np.nextafter(s, -np.inf).astype(np.float32)
        f = np.where(tie, np.where(err > 0, up, down), f)
    return f


def divby_emulation(x, d):
    """(DivBy, DivFast, Bad()) of d_math.h / d_bsdf.h for float32 arrays, in float32 arithmetic: the products of two 24-bit
    significands and the remainder x - q d are exact in float64, the last sum is rounded once (_round_sum_to_float32)."""
    with np.errstate(all="ignore"):
        one = np.float32(1)
        r = one / d
        ad = np.abs(d)
        fast = (ad > _LO_D) & (ad < _HI_D)
        q = x * r
        rem = (x.astype(np.float64) - q.astype(np.float64) * d.astype(np.float64)).astype(np.float32)   # fma(-q, d, x)
        q1 = _round_sum_to_float32(rem.astype(np.float64) * r.astype(np.float64), q)                     # fma(rem, r, q)
        aq = np.abs(q1)
        x2 = np.float32(2) * np.abs(x)   # (the numerator's guard: below it the remainder would be a subnormal float)
        inside = (aq > _LO_Q) & (aq < _HI_Q) & (x2 > _LO_Q)
        plain = x / d
        div_by = np.where(fast & inside, q1, plain)
        u = aq.view(np.uint32)
        t = np.minimum(u, x2.view(np.uint32))
        bad = ~fast | (u >= _HI_Q.view(np.uint32)) | ((t != 0) & (t <= _LO_Q.view(np.uint32)))
        q1 = np.copysign(q1, q)   # (DivFast's result: a zero takes the sign of x * r)
    return div_by, q1, bad, fast, inside


def _one_ulp_quotients(x, d, div_by):
    """(off, plain): where DivBy is not the IEEE quotient x / d bitwise (NaN for NaN counts as equal), and that quotient."""
    with np.errstate(all="ignore"):
        plain = x / d
    return ~((div_by.view(np.uint32) == plain.view(np.uint32)) | (np.isnan(div_by) & np.isnan(plain))), plain


def check_divisions(x, d, div_by, div_fast, bad):
    """What op 6 must show, for results from the device or from the emulation -- all but the two claims that the algorithm
    are checks of their own (check_boundary_claim, check_fast_is_exact). Returns the number of 1-ulp quotients."""
    off, plain = _one_ulp_quotients(x, d, div_by)
    with np.errstate(all="ignore"):
        ad = np.abs(d)
        fast = (ad > _LO_D) & (ad < _HI_D)
        # DivBy is x / d bitwise, or exactly one ulp away, the latter on at most 2^-18 of the operands
        assert (np.abs(div_by[off].view(np.int32).astype(np.int64) - plain[off].view(np.int32).astype(np.int64)) == 1).all(), (x[off][:4], d[off][:4], div_by[off][:4], plain[off][:4])
        assert off.sum() <= 2.0 ** -18 * len(x), off.sum()
        # outside the fast range of the divisor or the quotient, and on special values: the plain division
        aq = np.abs(plain)
        special = ~np.isfinite(x) | ~np.isfinite(d) | (x == 0) | (d == 0)
        # (DivBy tests its own candidate, at most an ulp from x / d: off the range for sure when x / d is, by more than an ulp)
        out_q = ~((aq >= np.nextafter(_LO_Q, np.float32(0))) & (aq <= np.nextafter(_HI_Q, np.float32(np.inf))))
        tiny_x = ~(np.float32(2) * np.abs(x) > _LO_Q)   # (the numerator's guard: such a remainder would be a subnormal float)
        assert not off[~fast | special | out_q | tiny_x].any()
        # DivTrack::Bad() is DivBy's own test -- the quotient's range (the hex constants against the float literals) and the
        # numerator's guard 2 |x| > 1e-30f -- a non-fast divisor included; an exact zero passes (d_bsdf.h: "0 * r is the quotient 0 / d")
        aqf = np.abs(div_fast)
        want_bad = ~fast | (~((aqf > _LO_Q) & (aqf < _HI_Q) & ~tiny_x) & (aqf != 0))
        assert np.array_equal(bad, want_bad), np.flatnonzero(bad != want_bad)[:8]
        # where the tracker holds DivFast has DivBy's value
        assert (div_fast[~bad] == div_by[~bad]).all()
    return int(off.sum())


def check_boundary_claim(x, d, div_by):
    """Where DivBy is one ulp off, float64(x) / float64(d) lies within 2^-20 ulp of a float32 rounding boundary: the cause
    d_math.h documents ("~2^-23 ulp"), with a factor 8 of margin."""
    off, plain = _one_ulp_quotients(x, d, div_by)
    exact = x[off].astype(np.float64) / d[off].astype(np.float64)
    boundary = (div_by[off].astype(np.float64) + plain[off].astype(np.float64)) / 2
    ulp = np.abs(div_by[off].astype(np.float64) - plain[off].astype(np.float64))
    dist = np.abs(exact - boundary) / ulp
    assert (dist <= 2.0 ** -20).all(), "(x, d, distance from the boundary in ulp): %s" % [(float(a), float(b), float(c)) for a, b, c in zip(x[off], d[off], dist)]


def check_fast_is_exact(x, d, div_by, div_fast, bad):
    """DivFast is DivBy bit for bit wherever Bad() is 0."""
    differ = ~bad & (div_fast.view(np.uint32) != div_by.view(np.uint32))
    assert not differ.any(), "(x, d, DivFast, DivBy): %s" % [(float(a), float(b), float(c), float(e)) for a, b, c, e in zip(x[differ][:8], d[differ][:8], div_fast[differ][:8], div_by[differ][:8])]


def test_division_emulation_holds_the_bounds():
    """The algorithm itself, emulated in float32 on the operands of the device test: DivBy is the IEEE quotient but for exactly
    one ulp on at most 2^-18 of the operands, and bitwise the IEEE quotient off the fast ranges, for numerators below the guard
    and on special values; Bad() is DivBy's own test, or a divisor off the fast range; DivFast has DivBy's value wherever Bad()
    is 0. (The device test compares the device with this emulation bit for bit.)"""
    x, d = division_operands()
    div_by, div_fast, bad, fast, inside = divby_emulation(x, d)
    n_off = check_divisions(x, d, div_by, div_fast, bad)
    print("DivBy one ulp from x / d on %d of %d operand pairs (cap %d)" % (n_off, len(x), int(2.0 ** -18 * len(x))))
    assert (fast & inside).mean() > .3 and (~fast).mean() > .1 and (fast & ~inside).mean() > .05   # every branch is well populated


def test_division_emulation_one_ulp_only_next_to_a_rounding_boundary():
    """Where DivBy is one ulp off, the float64 quotient lies within 2^-20 ulp of a rounding boundary. This is what the guard on
    the numerator (2 |x| > 1e-30f) is for: the remainder fma(-q, d, x) is about 2^-24 |x|, a subnormal float for |x| < 2^-101 and
    then no longer exact. Without the guard 4 of these 2^20 pairs were one ulp off at 1.5e-5 to 3.4e-3 ulp from the boundary,
    e.g. x = -2.5827939e-36, d = 4.03556142e-14, all of them among the 23 702 fast-path pairs with such a numerator."""
    x, d = division_operands()
    assert ((np.abs(x) < 2.0 ** -101) & (x != 0)).sum() > 20000
    check_boundary_claim(x, d, divby_emulation(x, d)[0])


def test_division_emulation_fast_form_is_divby_bit_for_bit():
    """DivFast is DivBy bit for bit wherever Bad() is 0, the sign of a zero included: the correction step fma(rem, r, q) alone
    turns x = -0 over d > 0 into +0 (rem * r = +0 added to q = -0), so DivFast gives its result the sign of q = x * r, which a
    non-zero result has anyway. The pair (x, d) = (-0, 1) of these operands shows it."""
    x, d = division_operands()
    div_by, div_fast, bad, _, _ = divby_emulation(x, d)
    k = np.flatnonzero((x == 0) & np.signbit(x) & (d == 1))
    assert len(k) == 1 and not bad[k[0]] and np.signbit(div_fast[k[0]]) and np.signbit(div_by[k[0]])
    check_fast_is_exact(x, d, div_by, div_fast, bad)


@pytest.mark.gpu
def test_divisions_on_the_device(pt):
    """mi_pt_math_probe op 6 over 2^20 operand pairs: the device's DivBy, DivFast and Bad() are the emulation's bit for bit and hold
    the same expectations themselves."""
    import test_gpu_parity
    x, d = division_operands()
    z = np.zeros_like(x)
    out = pt.math_probe(6, np.stack([x, z], 1), np.stack([d, z], 1))
    div_by, div_fast, bad = out[:, 0].copy(), out[:, 1].copy(), out[:, 2] == 1
    n_off = check_divisions(x, d, div_by, div_fast, bad)
    print("device DivBy one ulp from x / d on %d of %d operand pairs" % (n_off, len(x)))
    test_gpu_parity.METRICS.append({"test": "test_divisions_on_the_device", "pairs": len(x), "divby_off_by_one_ulp": n_off, "cap": int(2.0 ** -18 * len(x))})
    e_by, e_fast, e_bad, _, _ = divby_emulation(x, d)
    eq = lambda a, b: (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    assert eq(div_by, e_by).all(), np.flatnonzero(~eq(div_by, e_by))[:8]
    assert np.array_equal(bad, e_bad)
    assert eq(div_fast, e_fast)[~bad].all(), np.flatnonzero(~eq(div_fast, e_fast) & ~bad)[:8]
    check_boundary_claim(x, d, div_by)
    check_fast_is_exact(x, d, div_by, div_fast, bad)


def test_next_float_up_down(ob):
    _next_up_down(_oracle_probe(ob))


def test_efloat_operations_contain_the_precise_result(ob):
    _efloat_ops(_oracle_probe(ob))


def test_find_interval_basics(ob):
    _find_interval(_oracle_probe(ob))


@pytest.mark.gpu
def test_scalar_helpers_on_the_device(pt, ob):
    """The same three reference tests over the device's NextFloatUp / NextFloatDown, EFloat and SampleDiscrete
    (mi_pt_math_probe), and the device's results equal to the oracle's bit for bit on the same operands."""
    dev, orc = _device_probe(pt), _oracle_probe(ob)
    _next_up_down(dev)
    _efloat_ops(dev)
    _find_interval(dev)
    rng = np.random.default_rng(11)
    a, _, _ = _efloats(rng, 50000)
    b, _, _ = _efloats(rng, 50000)
    for op in (1, 2, 3, 4):
        assert np.array_equal(dev(op, a, b).view(np.int32), orc(op, a, b).view(np.int32)), op
