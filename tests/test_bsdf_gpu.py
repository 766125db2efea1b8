"""The device BSDF (d_bsdf.h), query by query: PathIntegrator.bsdf_probe (mi_pt_bsdf_probe) against the oracle's BSDF
(oracle_bsdf_n, correctly rounded libm) over the query sets of bsdf_cases.py -- 2048 random (wo, wi, u) and the edge set: wo on
and next to the horizon and the pole, wi the exact mirror direction / -wo / grazing / below the surface, u on the component
boundaries of Sample_f and at the origin of the concentric map -- under four lobe-type filters, in both modes.

Every untextured material of the catalogue (shade_plan_scenes.PLAIN, one scene) goes through every k_shade instance that can
shade it -- the instance holds its lobe count, lobe types, Fresnel kinds and TM_SCALED -- in every form of the 31 bins that
instance compiles: the lobe list bin by bin (form 0, the definition), four bins at a time (EvalQuad, 1), the straight-line form
of the hot instances with its retry (2), lobe by lobe (AccumulateF, 3). Instances whose masks differ only in light, sampler or
instance bits share one instantiation of the probe (those bits do not reach d_bsdf.h; test_shade_plan.py holds the mapping):
the sweep runs one of them and test_instances_of_one_instantiation_agree the others.

  pdf, wi, the sampled type, whether f is black     bitwise the oracle's (NaN where it has NaN)
  the 31 bins of form 0                             bitwise the oracle's; where a lobe's value is a quotient (microfacet
                                                    reflection, specular lobes: DivBy, d_math.h) at most 1 ulp off, in at most
                                                    max(4, 2^-18 x bins compared) bins of the whole module
  forms 1, 2, 3                                     bitwise form 0 of the same instance

Out of reach of this probe: image-textured lobes, roughness / sigma overrides and bump-mapped frames. The two hot
`... | TM_TEXTURED` instances receive only textured materials in a render; the probe runs them with untextured ones, so the
texture paths of every instance stay untested here (test_shade_instances_gpu.py renders them)."""
import numpy as np
import pytest

import bsdf_cases as bc
import shade_plan_scenes as sp

pytestmark = pytest.mark.gpu

DIV_LOBES = ("microfacet_reflection", "specular_reflection", "specular_transmission", "fresnel_specular")   # the kinds LobeDiv forms


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    """Bitwise equal, or NaN on both sides (the payload of a NaN is not part of the contract)."""
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def _ulps(a, b):
    """Distance in units of the last place between finite floats of one sign (else a large number)."""
    ia, ib = _bits(a).astype(np.int64), _bits(b).astype(np.int64)
    ok = np.isfinite(a) & np.isfinite(b) & ((ia >> 31) == (ib >> 31))
    return np.where(ok, np.abs(ia - ib), 1 << 40)


def material_bits(pt, m):
    t = 0
    for j in range(m.n_bxdfs):
        t |= (1 << m.bxdf[j].type) | (1 << (16 + m.bxdf[j].fresnel)) | (pt.TM_SCALED if m.bxdf[j].scaled else 0)
    return t


def probe_key(pt, nl, tm):
    """What the probe is instantiated per: the lobe count and the bits of the mask d_bsdf.h reads."""
    return nl, tm & (pt.lobe_bits(*pt.BXDF_TYPES) | pt.lobe_bits(*("fresnel_" + f for f in pt.FRESNEL_TYPES)) | pt.TM_SCALED | pt.TM_TEXTURED)


def instances_for(pt, m):
    """{probe key: [instance indices]} of the instances that can shade material m."""
    out = {}
    for i, (nl, tm) in enumerate(pt.shade_instances()):
        if m.n_bxdfs <= nl and material_bits(pt, m) & ~tm == 0:
            out.setdefault(probe_key(pt, nl, tm), []).append(i)
    return out


@pytest.fixture(scope="module")
def world(pt):
    s = pt.Scene(text=sp.scene_text(list(sp.PLAIN), res=8, spp=1))
    assert s.errors == [], s.errors
    assert s.desc.n_materials >= len(sp.PLAIN)
    assert not any(s.desc.materials[i].textured for i in range(s.desc.n_materials))
    return s, pt.CreatePathIntegrator(s, 0)


@pytest.fixture(scope="module")
def sweep(pt, ob, world):
    """Every launch of the module, once: per material, filter and mode the oracle's records, then every instantiation and form
    against them. Returns the lists of what went wrong (empty when all is well) and the counts."""
    s, integ = world
    q = bc.all_queries()
    r = {"oracle": [], "bins": [], "forms": [], "ulp_bins": 0, "bins_compared": 0, "launches": 0, "ulp_examples": []}

    def where(mi, inst, form, mode, fname, rows):
        k = int(rows[0])
        return "material %d, instance %d, form %d, mode %d, %s: %d queries, first %d = %s" % (mi, inst, form, mode, fname, len(rows), k, q[k].tolist())

    with ob.exact_libm():
        for mi in range(s.desc.n_materials):
            m = s.desc.materials[mi]
            has_div = any(pt.BXDF_TYPES[m.bxdf[j].type] in DIV_LOBES for j in range(m.n_bxdfs))
            keys = instances_for(pt, m)
            assert keys, mi   # (the general instances take everything)
            for fname, flags in bc.FLAGS.items():
                for mode in (0, 1):
                    want = ob.bsdf_n(s, mi, mode, q, flags)
                    for key, members in keys.items():
                        inst = members[0]
                        forms = pt.bsdf_probe_forms(inst)
                        got = {f: integ.bsdf_probe(mi, inst, mode, f, q, flags) for f in forms}
                        r["launches"] += len(forms)
                        g0 = got[0]
                        # pdf, wi, the sampled type, blackness
                        bad = ~_same(g0[:, 31:36], want[:, 31:36]).all(1) | ((g0[:, :31] == 0).all(1) != (want[:, :31] == 0).all(1))
                        if bad.any():
                            r["oracle"].append(where(mi, inst, 0, mode, fname, np.flatnonzero(bad)) +
                                               " device %s oracle %s" % (g0[np.flatnonzero(bad)[0], 31:36].tolist(), want[np.flatnonzero(bad)[0], 31:36].tolist()))
                        # the bins
                        same = _same(g0[:, :31], want[:, :31])
                        r["bins_compared"] += same.size
                        off = ~same
                        if off.any():
                            near = _ulps(g0[:, :31], want[:, :31]) <= 1
                            wrong = off & ~(near & has_div)
                            if wrong.any():
                                k = int(np.flatnonzero(wrong.any(1))[0])
                                r["bins"].append(where(mi, inst, 0, mode, fname, np.flatnonzero(wrong.any(1))) +
                                                 " device %s oracle %s" % (g0[k, :31][wrong[k]].tolist(), want[k, :31][wrong[k]].tolist()))
                            n_ulp = int((off & ~wrong).sum())
                            r["ulp_bins"] += n_ulp
                            if n_ulp and len(r["ulp_examples"]) < 8:
                                k = int(np.flatnonzero((off & ~wrong).any(1))[0])
                                r["ulp_examples"].append(where(mi, inst, 0, mode, fname, [k]))
                        # the other forms against form 0
                        for f in forms[1:]:
                            diff = ~_same(got[f][:, :36], g0).all(1)
                            if diff.any():
                                k = int(np.flatnonzero(diff)[0])
                                r["forms"].append(where(mi, inst, f, mode, fname, np.flatnonzero(diff)) +
                                                  " form %d %s form 0 %s" % (f, got[f][k, :36].tolist(), g0[k].tolist()))
    return r


def _report(items):
    return "%d cases, the first: %s" % (len(items), "\n".join(items[:5]))


def test_pdf_direction_type_and_blackness_are_the_oracles(sweep):
    assert sweep["launches"] > 1000
    assert not sweep["oracle"], _report(sweep["oracle"])


def test_bins_are_the_oracles_up_to_the_documented_quotients(sweep):
    """Bitwise, but for 1 ulp where a bin went through DivBy -- d_math.h: off by one ulp for about 2^-22 of operands; the cap is
    16 times that per bin (several quotients can meet in one bin)."""
    import test_gpu_parity
    cap = max(4, int(2.0 ** -18 * sweep["bins_compared"]))
    print("bins compared %d, off by one ulp %d (cap %d)" % (sweep["bins_compared"], sweep["ulp_bins"], cap))
    test_gpu_parity.METRICS.append({"test": "test_bins_are_the_oracles_up_to_the_documented_quotients", "bins_compared": sweep["bins_compared"],
                                    "bins_off_by_one_ulp": sweep["ulp_bins"], "cap": cap, "examples": sweep["ulp_examples"]})
    assert not sweep["bins"], _report(sweep["bins"])
    assert sweep["ulp_bins"] <= cap, (sweep["ulp_bins"], cap, sweep["ulp_examples"])


def test_every_form_is_form_0_bit_for_bit(sweep):
    """EvalQuad, the straight-line form and the lobe-by-lobe sums promise "the same additions as EvalBin's": no allowance."""
    assert not sweep["forms"], _report(sweep["forms"])


def test_instances_of_one_instantiation_agree(pt, world):
    """Instances that differ in light, sampler or instance bits only run the same probe kernel; and a material that several
    instantiations can shade gets the same record from all of them (form 0, both modes)."""
    s, integ = world
    q = bc.all_queries()
    for mi in range(s.desc.n_materials):
        keys = instances_for(pt, s.desc.materials[mi])
        for mode in (0, 1):
            first = None
            for members in keys.values():
                for inst in members:
                    got = integ.bsdf_probe(mi, inst, mode, 0, q)
                    if first is None:
                        first = got
                    assert _same(got, first).all(), (mi, inst, mode)


def _simple_instances(pt):
    return [i for i in range(len(pt.shade_instances())) if 2 in pt.bsdf_probe_forms(i)]


def test_the_retry_is_taken_and_reported(pt, world):
    """One wave of 64 queries through form 2 of every instance with the straight-line passes. With the lane of
    bsdf_cases.RETRY_LANE out of DivBy's fast range (the divisor 4 cos_o cos_i = 6.4e-19) every lane reports the retry, that lane
    alone reports Bad(), and the records are form 0's bit for bit; the same wave with a below-the-surface wi in that lane -- its
    only quotients exact zeros over 1 -- reports neither. The matte instances compile no division: nothing to retry."""
    s, integ = world
    plastic = next(i for i in range(s.desc.n_materials) if [pt.BXDF_TYPES[s.desc.materials[i].bxdf[j].type] for j in range(s.desc.materials[i].n_bxdfs)]
                   == ["lambertian_reflection", "microfacet_reflection"] and not s.desc.materials[i].bxdf[0].scaled)
    rough_glass = next(i for i in range(s.desc.n_materials) if [pt.BXDF_TYPES[s.desc.materials[i].bxdf[j].type] for j in range(s.desc.materials[i].n_bxdfs)]
                       == ["microfacet_reflection"] and s.desc.materials[i].kind == 2)
    matte = next(i for i in range(s.desc.n_materials) if s.desc.materials[i].n_bxdfs == 1 and pt.BXDF_TYPES[s.desc.materials[i].bxdf[0].type] == "oren_nayar")
    hit, calm = bc.retry_waves()
    seen = {"divides": 0, "matte": 0}
    for inst in _simple_instances(pt):
        nl, tm = pt.shade_instances()[inst]
        divides = bool(tm & pt.lobe_bits("microfacet_reflection"))
        mat = next((c for c in (plastic, rough_glass, matte) if inst in sum(instances_for(pt, s.desc.materials[c]).values(), [])), None)
        assert mat is not None and (mat != matte) == divides, (inst, hex(tm))
        seen["divides" if divides else "matte"] += 1
        a, a0 = integ.bsdf_probe(mat, inst, 0, 2, hit), integ.bsdf_probe(mat, inst, 0, 0, hit)
        b, b0 = integ.bsdf_probe(mat, inst, 0, 2, calm), integ.bsdf_probe(mat, inst, 0, 0, calm)
        assert _same(a[:, :36], a0).all() and _same(b[:, :36], b0).all(), inst
        lane = np.arange(64) == bc.RETRY_LANE
        if divides:
            assert np.isfinite(a0[bc.RETRY_LANE, :31]).all() and (a0[bc.RETRY_LANE, :31] > 0).all(), a0[bc.RETRY_LANE]   # (the lane's f is a value, not a zero)
            assert (a[:, 36] == 1).all() and np.array_equal(a[:, 37] == 1, lane), (inst, a[:, 36:])
        else:
            assert (a[:, 36:] == 0).all(), (inst, a[:, 36:])
        assert (b[:, 36:] == 0).all(), (inst, b[:, 36:])
        assert (b0[bc.RETRY_LANE, :31] == 0).all() and (b0[~lane, :31] > 0).all()   # (the lane's lobes dropped out; the others divide)
        # two waves in one launch: the report is per wave
        both = integ.bsdf_probe(mat, inst, 0, 2, np.concatenate([calm, hit]))
        assert (both[:64, 36] == 0).all() and (both[64:, 36] == (1 if divides else 0)).all(), inst
    assert seen["divides"] >= 5 and seen["matte"] >= 4, seen


def test_what_the_probe_refuses(pt, world, tmp_path):
    s, integ = world
    q = bc.random_queries(4)
    inst = pt.shade_instances()
    generic2, generic8 = inst.index((2, pt.TM_GENERIC)), inst.index((pt.MAX_BXDFS, pt.TM_GENERIC))
    for args, what in (((0, generic2, 0, 2), "form"),        # a form the instance lacks: no straight-line passes with every kind compiled
                       ((0, generic2, 0, 3), "form"),        # ... and no lobe-by-lobe sums at two lobes
                       ((0, generic8, 0, 2), "form"),
                       ((0, generic2, 0, 4), "form"), ((0, generic2, 0, -1), "form"),
                       ((0, len(inst), 0, 0), "instance index out of range"), ((0, -1, 0, 0), "instance index out of range"),
                       ((s.desc.n_materials, generic2, 0, 0), "material index out of range"), ((-1, generic2, 0, 0), "material index out of range"),
                       ((0, generic2, 2, 0), "mode")):
        with pytest.raises(RuntimeError, match=what):
            integ.bsdf_probe(args[0], args[1], args[2], args[3], q)
    five = next(i for i in range(s.desc.n_materials) if s.desc.materials[i].n_bxdfs == 5)
    with pytest.raises(RuntimeError, match="more lobes"):
        integ.bsdf_probe(five, generic2, 0, 0, q)
    assert integ.bsdf_probe(0, generic2, 0, 0, np.zeros((0, 8), np.float32)).shape == (0, 36)   # n = 0: nothing to do, no error
    assert integ.bsdf_probe(0, inst.index((2, pt.TM_GLASS | pt.TM_LIGHTS_ALL | pt.TM_SAMPLERS)), 0, 2, np.zeros((0, 8), np.float32)).shape == (0, 38)
    # a material that reads an image texture
    import scenes_text as st
    st.write_texture_files(str(tmp_path))
    ts = pt.Scene(text=sp.scene_text(["matte tex", "plastic rough tex", "matte"], res=8, spp=1), base_dir=str(tmp_path))
    assert ts.errors == [], ts.errors
    tinteg = pt.CreatePathIntegrator(ts, 0)
    full2 = inst.index((2, pt.TM_FULL))
    refused = 0
    for mi in range(ts.desc.n_materials):
        m = ts.desc.materials[mi]
        if m.textured or m.rough_tex[0] >= 0 or m.rough_tex[1] >= 0:
            refused += 1
            with pytest.raises(RuntimeError, match="image texture"):
                tinteg.bsdf_probe(mi, full2, 0, 0, q)
        else:
            tinteg.bsdf_probe(mi, full2, 0, 0, q)
    assert refused >= 2
