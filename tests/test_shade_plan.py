"""The shading plan (mi_pt_shade_plan: host code of the HIP library, no device) against the contract of d_bsdf.h: "a lobe
outside the mask cannot occur (the host picks the kernel from the lobes the class holds)". A k_shade instance compiles out
what its mask TM lacks, and a class routed to an instance without one of its bits renders a little darker and nothing else
shows -- so the routing itself is held here, from scene text through the real front end, for every material family in the
variants that change its lobe list (shade_plan_scenes.MATERIALS), under every sampler, with and without an infinite light,
with and without an ObjectInstance.

The last tests close the loop with tests/test_shade_instances_gpu.py: every instance of the library has a row there, the
rows' plans hold, and the rows of an instance name every lobe and Fresnel kind found routable to it here."""
import itertools

import pytest

import scenes_text as st
import shade_plan_scenes as sp
import test_shade_instances_gpu as rows

CONTEXTS = list(itertools.product(sp.SAMPLERS, (None, "const"), (False, True)))


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    d = tmp_path_factory.mktemp("shade_plan")
    st.write_texture_files(str(d))
    st.write_env_pfm(str(d / "env.pfm"))
    return d


def _scene(pt, assets, names, **kw):
    kw.setdefault("res", 4)
    kw.setdefault("spp", 4)
    s = pt.Scene(text=sp.scene_text(names, **kw), base_dir=str(assets))
    assert s.errors == [], (names, s.errors)
    return s


def _masks(pt):
    lobes = pt.lobe_bits(*pt.BXDF_TYPES)
    fresnels = pt.lobe_bits(*("fresnel_" + f for f in pt.FRESNEL_TYPES))
    disney = pt.lobe_bits("disney_diffuse", "disney_fake_ss", "disney_retro", "disney_sheen", "disney_clearcoat", "fresnel_disney")
    return lobes, fresnels, disney


def check_plan(pt, s, plan, instances, what):
    """The mask contract for every class of a plan."""
    d = s.desc
    lobes, fresnels, disney = _masks(pt)
    sampler = pt.SAMPLER_TYPES[d.sampler.type]
    assert pt.MISS_CLASS in plan["classes"], what   # the escaped rays are shaded too
    assert len(plan["material_class"]) == d.n_materials
    assert set(plan["material_class"]) | {pt.MISS_CLASS} == set(plan["classes"]), what
    for c, k in plan["classes"].items():
        where = (what, c, k)
        assert 0 <= k["instance"] < len(instances), where
        nl, tm = instances[k["instance"]]
        assert (nl, tm) == (k["nl"], k["tm"])
        assert (k["types"] & (lobes | fresnels | pt.TM_SCALED | pt.TM_TEXTURED)) & ~tm == 0, where
        assert k["types"] & ~(lobes | fresnels | pt.TM_SCALED | pt.TM_TEXTURED) == 0, where   # (a type word has no other bits)
        assert nl >= k["lobes"], where
        for i in range(d.n_lights):
            assert (tm >> (24 + d.lights[i].type)) & 1, where + (pt.LIGHT_TYPES[d.lights[i].type],)
        if sampler != "halton":
            assert tm & pt.TM_SAMPLERS, where
        if d.n_instances > 0:
            assert tm & pt.TM_INSTANCES, where
        if (k["types"] & pt.TM_TEXTURED) and (k["types"] & disney):
            assert nl == pt.MAX_BXDFS, where
    # the class records are those of the materials: the longest lobe list, the union of the types
    for c in set(plan["material_class"]):
        members = [d.materials[i] for i in range(d.n_materials) if plan["material_class"][i] == c]
        types = 0
        for m in members:
            for j in range(m.n_bxdfs):
                types |= (1 << m.bxdf[j].type) | (1 << (16 + m.bxdf[j].fresnel)) | (pt.TM_SCALED if m.bxdf[j].scaled else 0)
            types |= pt.TM_TEXTURED if m.textured else 0
        assert plan["classes"][c]["types"] == types, (what, c)
        longest = max(m.n_bxdfs for m in members)
        assert plan["classes"][c]["lobes"] == (pt.MAX_BXDFS if c == pt.MISS_CLASS - 1 else longest), (what, c)


def _signature(m):
    return tuple((m.bxdf[j].type, m.bxdf[j].fresnel) for j in range(m.n_bxdfs)) + (bool(m.textured),)


def test_the_instance_table_and_the_masks_come_from_the_library(pt):
    inst = pt.shade_instances()
    assert len(inst) == len(set(inst)) >= 21
    assert all(nl in (2, 4, pt.MAX_BXDFS) for nl, _ in inst)
    lobes, fresnels, _ = _masks(pt)
    assert pt.TM_ALL == 0xffffffff and pt.TM_FULL == pt.TM_ALL & ~pt.TM_INSTANCES and pt.TM_GENERIC == pt.TM_FULL & ~pt.TM_TEXTURED
    singles = (pt.TM_SCALED, pt.TM_TEXTURED, pt.TM_INSTANCES, pt.TM_SAMPLERS)
    assert all(bin(b).count("1") == 1 for b in singles) and len(set(singles)) == 4
    assert pt.TM_LIGHTS_ALL == sum(1 << (24 + t) for t in range(len(pt.LIGHT_TYPES)))
    assert pt.TM_LIGHTS_NO_ENV == pt.TM_LIGHTS_ALL & ~(1 << (24 + pt.LIGHT_TYPES.index("infinite")))
    for b in singles + (pt.TM_LIGHTS_ALL,):
        assert b & (lobes | fresnels) == 0
    for family in ("TM_DIFFUSE", "TM_PLASTIC", "TM_GLASS", "TM_UBER", "TM_DISNEY"):   # lobe and Fresnel bits only
        assert getattr(pt, family) & ~(lobes | fresnels) == 0 and getattr(pt, family) != 0
    assert pt.TM_DIFFUSE & ~pt.TM_PLASTIC == 0 and pt.TM_PLASTIC & ~pt.TM_UBER == 0
    with pytest.raises(ValueError, match="no mask named"):
        pt.shade_mask("TM_NONE")
    with pytest.raises(AttributeError):
        pt.TM_NONE


def test_the_enum_mirrors_are_those_of_the_header(pt):
    """BXDF_TYPES, FRESNEL_TYPES, LIGHT_TYPES and SAMPLER_TYPES give the mask bits their names: same names, same order as
    the enums of include/mi_pt.h."""
    import os
    import re
    from conftest import ROOT
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi_pt.h")).read(), flags=re.S)

    def enum(name, prefix):
        body = re.search(r"typedef enum %s \{(.*?)\}" % name, txt, flags=re.S).group(1)
        names = []
        for k, item in enumerate(x.strip() for x in body.split(",") if x.strip()):
            m = re.fullmatch(r"(%s[A-Z0-9_]+)(?:\s*=\s*(\d+))?" % prefix, item)
            assert m and (m.group(2) is None or int(m.group(2)) == k), item   # values count up from 0
            names.append(m.group(1)[len(prefix):].lower())
        return tuple(names)

    assert enum("mi_bxdf_type", "MI_BXDF_") == pt.BXDF_TYPES
    assert enum("mi_fresnel_type", "MI_FRESNEL_") == pt.FRESNEL_TYPES
    assert enum("mi_light_type", "MI_LIGHT_") == pt.LIGHT_TYPES
    assert tuple("02sequence" if n == "zerotwo" else n for n in enum("mi_sampler_type", "MI_SAMPLER_")) == pt.SAMPLER_TYPES
    assert pt.lobe_bits("fresnel_blend", "fresnel_noop") == (1 << pt.BXDF_TYPES.index("fresnel_blend")) | (1 << 16)
    with pytest.raises(ValueError):
        pt.lobe_bits("fresnel_none")


def test_a_malformed_description_is_refused_through_the_error_string(pt, assets):
    import ctypes as C
    lib = pt.hip_lib()
    assert lib.mi_pt_shade_plan(None, None, 0, None, None, None, None, 0, None, None) == -1
    assert b"null" in lib.mi_pt_last_error()
    s = _scene(pt, assets, ["matte"])
    n = C.c_uint32()
    buf = (C.c_int32 * 16)()
    assert lib.mi_pt_shade_plan(s.desc_ptr, None, 0, buf, None, None, None, 4, C.byref(n), None) == -1   # class buffers of 4
    assert b"too small" in lib.mi_pt_last_error()
    assert lib.mi_pt_shade_plan(s.desc_ptr, buf, 1, None, None, None, None, 0, None, None) == -1          # 2 materials into 1
    assert lib.mi_pt_shade_plan(s.desc_ptr, None, 0, None, None, None, None, 0, C.byref(n), None) == 0 and n.value == 2
    version = s.desc.abi_version
    s.desc.abi_version = version + 1
    try:
        with pytest.raises(RuntimeError, match="ABI version"):
            s.shade_plan()
    finally:
        s.desc.abi_version = version
    assert lib.mi_pt_shade_instances(None, None, 0, None) == -1
    assert lib.mi_pt_shade_instances(buf, None, 3, C.byref(n)) == -1 and n.value == len(pt.shade_instances())


@pytest.fixture(scope="module")
def routable(pt, assets):
    """Per instance index: the lobe, Fresnel and TM_SCALED bits of every class the catalogue routes to it, over all contexts
    (one scene per material and context; the plans are checked as they are made)."""
    instances = pt.shade_instances()
    lobes, fresnels, _ = _masks(pt)
    found = {}
    for name in sp.MATERIALS:
        for sampler, infinite, instanced in CONTEXTS:
            s = _scene(pt, assets, [name], sampler=sampler, infinite=infinite, instanced=instanced)
            assert pt.SAMPLER_TYPES[s.desc.sampler.type] == sampler and (s.desc.n_instances > 0) == instanced
            assert any(s.desc.lights[i].type == pt.LIGHT_TYPES.index("infinite") for i in range(s.desc.n_lights)) == bool(infinite)
            assert {s.desc.lights[i].type for i in range(s.desc.n_lights)} >= {0, 1, 2, 4}
            plan = s.shade_plan()
            check_plan(pt, s, plan, instances, (name, sampler, infinite, instanced))
            hot = (pt.TM_LIGHTS_ALL if infinite else pt.TM_LIGHTS_NO_ENV) | (0 if sampler == "halton" else pt.TM_SAMPLERS)
            assert plan["hot"] == hot
            for c, k in plan["classes"].items():
                found[k["instance"]] = found.get(k["instance"], 0) | (k["types"] & (lobes | fresnels | pt.TM_SCALED))
    return found


def test_every_material_family_under_every_context_keeps_the_mask_contract(pt, routable):
    """(The checks run in the fixture, scene by scene.) Not vacuous: every instance of the library is reached by some
    material of the catalogue under some context."""
    assert set(routable) == set(range(len(pt.shade_instances())))


def test_the_catalogue_has_the_lobe_lists_it_is_named_for(pt, assets):
    """The variants do change the lobe list: lobe counts by name, through the front end."""
    def lobes_of(name):
        s = _scene(pt, assets, [name])
        used = {s.desc.prims[i].material for i in range(s.desc.n_prims)}
        assert len(used) == 1
        return s.desc.materials[used.pop()]

    counts = {"matte": 1, "matte sigma": 1, "matte black": 0, "plastic": 2, "plastic Kd black": 1, "plastic Ks black": 1, "glass": 1,
              "glass rough": 2, "glass rough Kr black": 1, "mirror": 1, "metal": 1, "substrate": 1, "translucent": 4, "translucent Kd black": 2,
              "translucent Ks black": 2, "translucent reflect black": 2, "translucent transmit black": 2, "disney": 3, "disney thin": 5,
              "disney spectrans": 4, "disney clearcoat": 4, "disney sheen": 4, "disney metallic": 1, "disney all": 8, "uber": 0, "uber dsrto": 5,
              "uber dsrt": 4, "uber o": 1, "uber do": 2, "mix matte matte": 2, "mix plastic mirror": 3, "mix uber5 matte": 6, "mix of mixes": 5,
              "mix of mixes 8": 8, "glass rough map": 3, "uber5 tex": 5, "disney tex": 3, "disney metallic tex": 1, "disney all tex": 8,
              "mix of mixes tex": 5, "mix of mixes 8 tex": 8}
    for name, n in counts.items():
        assert lobes_of(name).n_bxdfs == n, name
    for parts in ("d", "ds", "dsr", "dsrt", "sro"):
        assert lobes_of("uber " + parts).n_bxdfs == len(parts)
    assert all(lobes_of(n).textured for n in sp.TEXTURED) and not any(lobes_of(n).textured for n in sp.PLAIN)
    assert max(lobes_of("mix of mixes").bxdf[j].scaled for j in range(5)) == 2


def test_materials_with_equal_signatures_share_a_class(pt, assets):
    names = ["matte", "plastic Ks black", "plastic", "translucent transmit black", "matte tex", "matte bump", "glass", "glass Kr black", "matte sigma"]
    s = _scene(pt, assets, names)
    plan = s.shade_plan()
    d = s.desc
    assert d.n_materials >= len(names)   # (distinct records: the parameters differ)
    sigs = [_signature(d.materials[i]) for i in range(d.n_materials)]
    for i, j in itertools.combinations(range(d.n_materials), 2):
        assert (plan["material_class"][i] == plan["material_class"][j]) == (sigs[i] == sigs[j]), (i, j)
    assert len(set(sigs)) == 5 < d.n_materials   # [L], [L, MR], [L] textured, [FS], [ON]
    first = []   # classes are numbered in order of first appearance
    for c in plan["material_class"]:
        if c not in first:
            first.append(c)
    assert first == list(range(len(first)))
    check_plan(pt, s, plan, pt.shade_instances(), "shared classes")


# 16 materials whose signatures differ from each other and from the default matte's (material 0 of every scene): with it, a
# scene of the first n of them has n + 1 signatures
DISTINCT = ("matte sigma", "plastic", "glass", "mirror", "metal", "substrate", "translucent", "disney", "uber dr", "uber dt", "uber sr",
            "glass rough", "uber dsr", "disney metallic", "uber dsrto", "disney thin")


@pytest.mark.parametrize("textured", [False, True])
@pytest.mark.parametrize("instanced", [False, True])
def test_overflow_17_signatures(pt, assets, instanced, textured):
    """The 15th, 16th and 17th signature share class 14, which counts MI_MAX_BXDFS lobes and holds the union of their types;
    it routes to an eight-lobe instance that fits. The default matte, material 0 of every scene, is the first signature and
    DISTINCT[k] the (k + 2)th; textured: the 16th is an image-textured matte, one lobe."""
    names = list(DISTINCT)
    if textured:
        names[14] = "matte tex"
    s = _scene(pt, assets, names, instanced=instanced)
    d = s.desc
    sigs = [_signature(d.materials[i]) for i in range(d.n_materials)]
    assert d.n_materials == 17 and len(set(sigs)) == 17
    plan = s.shade_plan()
    assert plan["material_class"] == list(range(14)) + [14, 14, 14]
    k = plan["classes"][14]
    want = pt.TM_TEXTURED if textured else 0
    for m in (14, 15, 16):
        for t, f in sigs[m][:-1]:
            want |= (1 << t) | (1 << (16 + f))
    assert k["types"] & ~pt.TM_SCALED == want and k["lobes"] == pt.MAX_BXDFS
    assert max(d.materials[m].n_bxdfs for m in (14, 15, 16)) < pt.MAX_BXDFS   # (the count is the class's, not a material's)
    assert k["nl"] == pt.MAX_BXDFS
    assert k["tm"] == (pt.TM_ALL if instanced else pt.TM_FULL if textured else pt.TM_GENERIC)
    check_plan(pt, s, plan, pt.shade_instances(), "overflow")


def test_14_and_15_signatures_sit_on_the_two_sides_of_the_boundary(pt, assets):
    """14 signatures: classes 0..13, each with its own lobe count and instance. The 15th opens class 14 -- alone in it, one
    lobe, and still counted as MI_MAX_BXDFS lobes on an eight-lobe instance."""
    assert DISTINCT[13] == "disney metallic"
    s14 = _scene(pt, assets, DISTINCT[:13])
    plan = s14.shade_plan()
    assert s14.desc.n_materials == 14 and plan["material_class"] == list(range(14)) and 14 not in plan["classes"]
    assert all(plan["classes"][c]["lobes"] == s14.desc.materials[c].n_bxdfs for c in range(14))
    s15 = _scene(pt, assets, DISTINCT[:14])
    plan = s15.shade_plan()
    assert s15.desc.n_materials == 15 and plan["material_class"] == list(range(15))
    assert s15.desc.materials[14].n_bxdfs == 1 and plan["classes"][14]["lobes"] == pt.MAX_BXDFS
    # (a metallic Disney lobe alone: of the eight-lobe instances, the Disney one fits it)
    assert (plan["classes"][14]["nl"], plan["classes"][14]["tm"]) == (pt.MAX_BXDFS, pt.TM_DISNEY | pt.TM_LIGHTS_ALL | pt.TM_SAMPLERS)
    # the same material one place earlier is an ordinary class of one lobe on a two-lobe instance
    s = _scene(pt, assets, DISTINCT[:12] + DISTINCT[13:14])
    k = s.shade_plan()["classes"][13]
    assert (k["lobes"], k["nl"], k["tm"]) == (1, 2, pt.TM_GENERIC)
    for sc in (s14, s15, s):
        check_plan(pt, sc, sc.shade_plan(), pt.shade_instances(), "boundary")


def test_routes_that_the_special_rules_decide(pt, assets):
    """The rules of ShadeInstanceOf by name: what a reader of the table expects, pinned."""
    inst = pt.shade_instances()

    def route(name, **kw):
        s = _scene(pt, assets, [name], **kw)
        plan = s.shade_plan()
        used = {s.desc.prims[i].material for i in range(s.desc.n_prims)}
        (c,) = {plan["material_class"][m] for m in used}
        return plan["classes"][c]["nl"], plan["classes"][c]["tm"]

    LS = pt.TM_LIGHTS_ALL | pt.TM_SAMPLERS
    assert route("matte") == (2, pt.TM_DIFFUSE | pt.TM_LIGHTS_NO_ENV)
    assert route("matte", infinite="const", sampler="random") == (2, pt.TM_DIFFUSE | LS)
    assert route("plastic", sampler="stratified") == (2, pt.TM_PLASTIC | pt.TM_LIGHTS_NO_ENV | pt.TM_SAMPLERS)
    assert route("glass", sampler="sobol") == (2, pt.TM_GLASS | LS)          # (the hot bits go to matte and plastic only)
    assert route("translucent") == route("uber dsro") == (4, pt.TM_UBER | LS)    # four lobes fit
    assert route("uber dsrto") == (pt.MAX_BXDFS, pt.TM_GENERIC)               # five do not
    assert route("disney") == route("disney all") == (pt.MAX_BXDFS, pt.TM_DISNEY | LS)
    assert route("disney metallic") == (2, pt.TM_GENERIC)
    assert route("mix of mixes") == (pt.MAX_BXDFS, pt.TM_GENERIC) and route("mix plastic mirror") == (4, pt.TM_GENERIC)
    assert route("matte tex") == (2, pt.TM_DIFFUSE | pt.TM_TEXTURED | LS) and route("plastic bump") == (2, pt.TM_PLASTIC | pt.TM_TEXTURED | LS)
    assert route("mirror tex") == (2, pt.TM_FULL) and route("uber tex") == (4, pt.TM_FULL) and route("uber5 tex") == (pt.MAX_BXDFS, pt.TM_FULL)
    assert route("disney metallic tex") == route("disney tex") == (pt.MAX_BXDFS, pt.TM_FULL)   # textured Disney: eight, whatever the count
    assert route("matte", instanced=True) == route("mirror tex", instanced=True) == (2, pt.TM_ALL)
    assert route("disney metallic tex", instanced=True) == route("uber dsr", instanced=True) == (pt.MAX_BXDFS, pt.TM_ALL)
    assert all(x in inst for x in (route("matte"), route("uber5 tex")))


# ------------------------------------------------------------------ closure with the GPU table
def test_every_instance_has_a_row_and_every_row_an_instance(pt):
    """A new or renamed k_shade instance fails here, without a GPU, until tests/test_shade_instances_gpu.py has a scene for it."""
    inst = pt.shade_instances()
    keyed = {}
    for name, row in rows.ROWS.items():
        key = (row["nl"], rows.row_mask(pt, row))
        assert key in inst, "row %r names k_shade<%d, %#x>, which the library does not have" % ((name,) + key)
        keyed.setdefault(inst.index(key), []).append(name)
    missing = [(i,) + inst[i] for i in range(len(inst)) if i not in keyed]
    assert not missing, "k_shade instances without a row in tests/test_shade_instances_gpu.py (index, NL, TM): %s" % [(i, nl, hex(tm)) for i, nl, tm in missing]


def test_every_instance_has_a_bsdf_probe_instantiation(pt):
    """A new k_shade instance fails here, without a GPU, until MIPT_BSDF_PROBE_ROWS (pt_kernels.hip) has a row for its lobe
    count and BSDF bits: tests/test_bsdf_gpu.py reaches the BSDF code of an instance through that row alone. The forms of a row
    are those its instance's spectral passes are compiled as (ShadeSimpleSpectra, ShadeAccum)."""
    not_simple = pt.lobe_bits("fresnel_conductor", "fresnel_disney", "fresnel_blend", "disney_clearcoat", "disney_diffuse", "disney_retro") | pt.TM_TEXTURED | pt.TM_SCALED
    for i, (nl, tm) in enumerate(pt.shade_instances()):
        forms = pt.bsdf_probe_forms(i)   # (ValueError: no row)
        want = (0, 1) + ((2,) if nl <= 2 and not tm & not_simple else ()) + ((3,) if nl > 2 or tm & pt.TM_TEXTURED else ())
        assert forms == want, (i, nl, hex(tm), forms)
    with pytest.raises(ValueError, match="out of range"):
        pt.bsdf_probe_forms(len(pt.shade_instances()))
    with pytest.raises(ValueError, match="out of range"):
        pt.bsdf_probe_forms(-1)


@pytest.mark.parametrize("name", list(rows.ROWS))
def test_the_rows_plans_hold(pt, assets, monkeypatch, name):
    """What each GPU row asserts from the plan before it renders, here without a device; and the contract for its scene."""
    monkeypatch.delenv("MIPT_INSTANCES", raising=False)
    row = rows.ROWS[name]
    s = rows.load_row(pt, row, assets)
    inst = pt.shade_instances()
    index = rows.check_row_plan(pt, s, row, inst)
    check_plan(pt, s, s.shade_plan(), inst, name)
    tm = inst[index][1]
    want = {"halton"} if not (tm & pt.TM_SAMPLERS) else None
    if want:
        assert pt.SAMPLER_TYPES[s.desc.sampler.type] in want
    # an infinite light in the scene exactly when the instance is compiled with that code, row by row
    has_infinite = any(s.desc.lights[i].type == pt.LIGHT_TYPES.index("infinite") for i in range(s.desc.n_lights))
    assert has_infinite == bool(row["infinite"]) == bool((tm >> (24 + pt.LIGHT_TYPES.index("infinite"))) & 1)
    assert {s.desc.lights[i].type for i in range(s.desc.n_lights)} >= {0, 1, 2, 4}
    w, h = s.film_size
    assert 24 <= w <= 32 and s.spp == 16 and 5 <= s.desc.integrator.max_depth <= 6
    if row["zoo"]:
        plan = s.shade_plan()
        hidden = [m for m in range(s.desc.n_materials) if m not in rows.visible_materials(s)]
        assert sorted(plan["material_class"][m] for m in hidden)[:14] == list(range(14))   # the 14 signatures in front


def test_the_rows_of_an_instance_name_everything_routable_to_it(pt, routable):
    inst = pt.shade_instances()
    declared = {}
    for row in rows.ROWS.values():
        i = inst.index((row["nl"], rows.row_mask(pt, row)))
        declared[i] = declared.get(i, 0) | rows.row_types(pt, row)
    for i, bits in sorted(routable.items()):
        lacking = bits & ~declared.get(i, 0)
        assert not lacking, "k_shade instance %d <%d, %#x>: no row exercises %s%s" % (
            i, inst[i][0], inst[i][1], pt.lobe_names(lacking), " (scaled)" if lacking & pt.TM_SCALED else "")
