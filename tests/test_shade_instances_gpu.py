"""Every k_shade instance against the CPU oracle, each on a scene built for it. Run on the GPU box with `pytest -m gpu`.

k_shade is compiled once per (NL, TM) of MIPT_SHADE_INSTANCES (pt_kernels.hip); the host routes every shading class of a
scene to one of them (mi_pt_shade_plan). A lobe or Fresnel kind outside an instance's mask is compiled out of it and
evaluates to nothing, so an instance is tested only by a scene whose classes route to it. ROWS names such a scene for
every instance: the materials (shade_plan_scenes.MATERIALS) on small spheres over a lit ground, the sampler and the lights
the mask stands for (an infinite light in every row whose mask has that bit). Each row first asserts, from
Scene.shade_plan(), that its materials do route to its instance and that the lobe and Fresnel kinds routed there are the ones
the row declares -- the table says what each instance is tested with --, then that every material is seen by the camera,
then renders at test_gpu_parity._parity's exact bars (weights equal, camera rays equal, the five counters within 2, film
relative L2 < 1e-6, every pixel within 2e-4 x mean radiance).

No tolerance is defined here: the bars are _parity's. (The one other figure, 0.05 between an instanced render and the
render of the same scene with its instances expanded into world shapes, is test_object_instances_against_oracle's, as is
the comparison: the two scenes have different trees and float paths and agree statistically.)

test_shade_plan.py (no GPU) checks that every instance of the library has a row here and that the rows of an instance
declare every lobe and Fresnel kind the front end can route to it."""
import numpy as np
import pytest

import scenes_text as st
import shade_plan_scenes as sp
from test_gpu_parity import _parity, _rel_l2

pytestmark = pytest.mark.gpu

L = ("TM_LIGHTS_ALL",)
LS = ("TM_LIGHTS_ALL", "TM_SAMPLERS")

# zoo: the 13 hidden materials in front of scenes_text.material_zoo() -- with the default matte, 14 signatures none of the
# zoo's materials has, so that every one of those lands in the overflow class
ZOO_DUMMIES = ("uber dr", "uber dt", "uber sr", "uber st", "uber rt", "uber drt", "uber srt", "uber dst", "uber dsrt", "uber do",
               "uber so", "uber ro", "uber dsrto")   # (the zoo's own uber is Kd, Ks, Kr under an opacity: another list)


def _row(nl, tm, materials, kinds, sampler="halton", infinite=None, instanced=False, ground=True, zoo=False, hidden=(), scaled=False):
    """nl, tm: the instance (tm: names of pt.TM_* masks, or-ed). materials: catalogue names, the first one also the ground's
    and the emitter's. kinds: the lobe types and Fresnel kinds (pt.lobe_bits names) routed to the instance by this scene;
    scaled: a mix's lobes among them. zoo: the scene is material_zoo() behind `hidden` (the overflow class)."""
    return dict(nl=nl, tm=tm, materials=tuple(materials), kinds=tuple(kinds), sampler=sampler, infinite=infinite, instanced=instanced,
                ground=ground, zoo=zoo, hidden=tuple(hidden), scaled=scaled)


DIFFUSE_KINDS = ("lambertian_reflection", "oren_nayar", "fresnel_noop")
PLASTIC_KINDS = ("lambertian_reflection", "microfacet_reflection", "fresnel_noop", "fresnel_dielectric")
GENERIC2_KINDS = ("lambertian_reflection", "oren_nayar", "specular_transmission", "fresnel_specular", "microfacet_reflection",
                  "microfacet_transmission", "lambertian_transmission", "fresnel_blend", "fresnel_noop", "fresnel_disney", "fresnel_conductor")
GLASS_KINDS = ("specular_reflection", "specular_transmission", "fresnel_specular", "microfacet_reflection", "microfacet_transmission",
               "fresnel_noop", "fresnel_dielectric")
UBER_KINDS = ("lambertian_reflection", "specular_reflection", "specular_transmission", "microfacet_reflection", "microfacet_transmission",
              "lambertian_transmission", "fresnel_noop", "fresnel_dielectric")
DISNEY_KINDS = ("microfacet_reflection", "microfacet_transmission", "lambertian_transmission", "disney_diffuse", "disney_fake_ss",
                "disney_retro", "disney_sheen", "disney_clearcoat", "fresnel_noop", "fresnel_disney")
ZOO_KINDS = ("lambertian_reflection", "oren_nayar", "specular_reflection", "specular_transmission", "fresnel_specular", "microfacet_reflection",
             "microfacet_transmission", "lambertian_transmission", "disney_diffuse", "disney_fake_ss", "disney_retro", "disney_sheen",
             "disney_clearcoat", "fresnel_blend", "fresnel_noop", "fresnel_dielectric", "fresnel_disney", "fresnel_conductor")
UNTEXTURED_2 = ("matte", "matte sigma", "plastic", "glass", "glass rough", "mirror", "metal", "substrate", "translucent Ks black",
                "translucent reflect black", "disney metallic", "uber do", "mix matte matte")
# (the materials a mix names are materials of the scene too and take classes: few enough mixes to stay below the overflow)
TEXTURED_2 = ("matte tex", "plastic tex", "glass tex", "mirror bump", "metal tex", "substrate tex", "uber bump", "mix matte tex matte",
              "mix matte bump mirror")
ALL2_KINDS = GENERIC2_KINDS + ("specular_reflection", "fresnel_dielectric")

ROWS = {
    # ---- the hot instances: matte and plastic, by the scene's lights and sampler
    "matte, infinite light, halton": _row(2, ("TM_DIFFUSE",) + L, ("matte", "matte sigma", "plastic Ks black", "matte black"), DIFFUSE_KINDS, infinite="map"),
    "matte, halton": _row(2, ("TM_DIFFUSE", "TM_LIGHTS_NO_ENV"), ("matte sigma", "matte", "matte black"), DIFFUSE_KINDS),
    "matte, infinite light, sobol": _row(2, ("TM_DIFFUSE",) + LS, ("matte", "matte sigma", "plastic Ks black"), DIFFUSE_KINDS, sampler="sobol", infinite="const"),
    "matte, stratified": _row(2, ("TM_DIFFUSE", "TM_LIGHTS_NO_ENV", "TM_SAMPLERS"), ("matte sigma", "matte"), DIFFUSE_KINDS, sampler="stratified"),
    "plastic, infinite light, halton": _row(2, ("TM_PLASTIC",) + L, ("plastic", "plastic Kd black", "translucent transmit black", "glass rough Kt black"),
                                            PLASTIC_KINDS, infinite="const"),
    "plastic, halton": _row(2, ("TM_PLASTIC", "TM_LIGHTS_NO_ENV"), ("plastic", "plastic Kd black", "translucent transmit black"), PLASTIC_KINDS),
    "plastic, infinite light, 02sequence": _row(2, ("TM_PLASTIC",) + LS, ("plastic", "plastic Kd black", "glass rough Kt black"), PLASTIC_KINDS,
                                                sampler="02sequence", infinite="map"),
    "plastic, random": _row(2, ("TM_PLASTIC", "TM_LIGHTS_NO_ENV", "TM_SAMPLERS"), ("plastic", "plastic Kd black", "translucent transmit black"),
                            PLASTIC_KINDS, sampler="random"),
    # ---- the other untextured instances
    "two lobes, generic": _row(2, ("TM_GENERIC",), ("mix matte matte", "metal", "metal spectra", "substrate", "translucent Ks black", "translucent reflect black",
                                                     "disney metallic", "uber dr", "uber do", "mix matte metal", "mix glass substrate"), ALL2_KINDS, infinite="const", scaled=True),
    "glass and mirror": _row(2, ("TM_GLASS",) + LS, ("mirror", "glass", "glass Kr black", "glass rough", "glass rough Kr black", "translucent Kd black",
                                                    "uber sr", "uber r", "uber t", "uber st"), GLASS_KINDS, infinite="map"),
    "uber": _row(4, ("TM_UBER",) + LS, ("uber dsr", "translucent", "uber dst", "uber drt", "uber srt", "uber dsrt", "uber dsro", "uber srto", "uber dto"),
                 UBER_KINDS, infinite="const"),
    "disney": _row(8, ("TM_DISNEY",) + LS, ("disney", "disney thin", "disney spectrans", "disney clearcoat", "disney sheen", "disney all"), DISNEY_KINDS,
                   infinite="map"),
    "four lobes, generic": _row(4, ("TM_GENERIC",), ("mix plastic mirror", "mix disney matte", "mix of mix small", "mix plastic metal"),
                                ("lambertian_reflection", "oren_nayar", "specular_reflection", "microfacet_reflection", "disney_diffuse", "disney_retro",
                                 "fresnel_noop", "fresnel_dielectric", "fresnel_disney", "fresnel_conductor"), infinite="map", scaled=True),
    "eight lobes, generic: mixes of mixes": _row(8, ("TM_GENERIC",), ("mix of mixes", "mix of mixes 8", "mix translucent metal"),
                                                 ("lambertian_reflection", "specular_reflection", "fresnel_specular", "microfacet_reflection", "microfacet_transmission",
                                                  "lambertian_transmission", "fresnel_blend", "fresnel_noop", "fresnel_dielectric", "fresnel_conductor"),
                                                 infinite="const", scaled=True),
    "eight lobes, generic: five-lobe uber": _row(8, ("TM_GENERIC",), ("uber dsrto", "mix uber5 matte"),
                                                 ("lambertian_reflection", "specular_reflection", "specular_transmission", "microfacet_reflection", "fresnel_noop",
                                                  "fresnel_dielectric"), infinite="map", scaled=True),
    # ---- the instances that evaluate image textures
    "matte, textured": _row(2, ("TM_DIFFUSE", "TM_TEXTURED") + LS, ("matte tex", "matte sigma tex", "matte bump"), DIFFUSE_KINDS, infinite="map"),
    "plastic, textured": _row(2, ("TM_PLASTIC", "TM_TEXTURED") + LS, ("plastic tex", "plastic Ks tex", "plastic rough tex", "plastic bump", "translucent bump"),
                              PLASTIC_KINDS, infinite="const"),
    "two lobes, textured": _row(2, ("TM_FULL",), ("substrate tex", "glass tex", "glass bump", "mirror tex", "mirror bump", "metal tex", "metal rough tex",
                                                  "substrate bump", "uber bump", "mix matte tex matte", "mix matte bump mirror"),
                                ("lambertian_reflection", "specular_reflection", "fresnel_specular", "microfacet_reflection", "fresnel_blend", "fresnel_noop",
                                 "fresnel_dielectric", "fresnel_conductor"), infinite="map", scaled=True),
    "four lobes, textured": _row(4, ("TM_FULL",), ("uber tex", "glass rough map", "translucent tex", "mix plastic tex mirror"),
                                 ("lambertian_reflection", "specular_reflection", "fresnel_specular", "microfacet_reflection", "microfacet_transmission",
                                  "lambertian_transmission", "fresnel_noop", "fresnel_dielectric"), infinite="const", scaled=True),
    "eight lobes, textured, not disney": _row(8, ("TM_FULL",), ("uber5 tex", "mix uber5 tex matte", "mix of mixes tex", "mix of mixes 8 tex"),
                                              ("lambertian_reflection", "specular_reflection", "specular_transmission", "fresnel_specular", "microfacet_reflection",
                                               "microfacet_transmission", "lambertian_transmission", "fresnel_blend", "fresnel_noop", "fresnel_dielectric",
                                               "fresnel_conductor"), infinite="const", scaled=True),
    "textured disney of four lobes or fewer": _row(8, ("TM_FULL",), ("disney tex", "disney metallic tex", "disney spectrans tex", "disney clearcoat tex",
                                                                      "disney sheen tex", "disney rough tex", "mix disney tex matte"),
                                                   ("lambertian_reflection", "microfacet_reflection", "microfacet_transmission", "disney_diffuse", "disney_retro",
                                                    "disney_sheen", "disney_clearcoat", "fresnel_noop", "fresnel_disney"), infinite="const", scaled=True),
    "textured disney of more lobes": _row(8, ("TM_FULL",), ("disney thin tex", "disney all tex"), DISNEY_KINDS, infinite="map"),
    # ---- scenes with an ObjectInstance: the two fully general instances (also rendered expanded, test_instanced_rows_expanded)
    "instanced, two lobes": _row(2, ("TM_ALL",), UNTEXTURED_2, ALL2_KINDS, instanced=True, infinite="const", scaled=True),
    "instanced, two lobes, textured": _row(2, ("TM_ALL",), TEXTURED_2,
                                           ("lambertian_reflection", "specular_reflection", "fresnel_specular", "microfacet_reflection",
                                            "fresnel_blend", "fresnel_noop", "fresnel_dielectric", "fresnel_conductor"), instanced=True, infinite="map",
                                           scaled=True),
    "instanced, more lobes": _row(8, ("TM_ALL",), ("uber dsr", "translucent", "uber dsrto", "disney", "disney all", "disney sheen", "mix plastic mirror",
                                                   "mix of mix small", "mix of mixes 8", "mix translucent metal"), tuple(k for k in ZOO_KINDS if k != "fresnel_specular"), instanced=True,
                                  infinite="map", scaled=True),
    "instanced, more lobes, textured": _row(8, ("TM_ALL",), ("uber tex", "glass rough map", "translucent tex", "uber5 tex", "disney tex", "disney metallic tex",
                                                             "disney all tex", "mix disney tex matte", "mix of mixes 8 tex"),
                                            tuple(k for k in ZOO_KINDS if k != "oren_nayar"), instanced=True, infinite="const", scaled=True),
    # ---- the overflow class: the material zoo behind 14 other signatures. (The instanced one is not among the scenes rendered
    # expanded as well: without its object instance it is the first one's scene and one sphere more, routed like it.)
    "overflow": _row(8, ("TM_GENERIC",), (), ZOO_KINDS, zoo=True, hidden=ZOO_DUMMIES, infinite="const", scaled=True),
    "overflow, a textured material in the class": _row(8, ("TM_FULL",), (), ZOO_KINDS, zoo=True, hidden=ZOO_DUMMIES + ("matte tex",), infinite="map",
                                                       scaled=True),
    "overflow, instanced": _row(8, ("TM_ALL",), (), ZOO_KINDS, zoo=True, hidden=ZOO_DUMMIES, instanced=True, infinite="const", scaled=True),
}

RES, SPP, DEPTH = 24, 16, 5
ZOO_RES = 32


def row_mask(pt, row):
    m = 0
    for n in row["tm"]:
        m |= getattr(pt, n)
    return m


def row_types(pt, row):
    """The lobe, Fresnel and TM_SCALED bits of the type words the row declares (texturedness: check_row_plan, from the mask)."""
    return pt.lobe_bits(*row["kinds"]) | (pt.TM_SCALED if row["scaled"] else 0)


def row_text(row):
    if row["zoo"]:
        zoo = st.zoo_with_infinite_light(row["infinite"], res=ZOO_RES, spp=SPP, depth=6, strategy="power")   # ("const" / "map": beside the zoo's lights)
        head = sp.TEXTURES if any(n in sp.TEXTURED for n in row["hidden"]) else ""
        for k, n in enumerate(row["hidden"]):
            head += 'AttributeBegin\n%s\nTranslate %g -50 -90\nShape "sphere" "float radius" [.01]\nAttributeEnd\n' % (sp.MATERIALS[n], 2 * k)
        assert zoo.count("WorldBegin\n") == 1 and zoo.count("WorldEnd") == 1
        zoo = zoo.replace("WorldBegin\n", "WorldBegin\n" + head)
        if row["instanced"]:   # (a use of one more sphere of the zoo's last material, in front of the others)
            zoo = zoo.replace("WorldEnd", 'Material "plastic" "rgb Kd" [.1 .2 .6] "rgb Ks" [.5 .5 .5] "float roughness" [.08]\n' + sp.INSTANCE % (0, .3, -4.6) + "WorldEnd")
        return zoo
    m = row["materials"]
    return sp.scene_text(m[1:], sampler=row["sampler"], infinite=row["infinite"], instanced=row["instanced"], res=RES, spp=SPP, depth=DEPTH, ground=m[0])


def load_row(pt, row, base_dir):
    s = pt.Scene(text=row_text(row), base_dir=str(base_dir))
    assert s.errors == [], s.errors
    return s


def visible_materials(s):
    """Material indices of the primitives meant to be seen: not an emitter's, not a hidden sphere's (radius .01)."""
    d = s.desc
    out = set()
    for i in range(d.n_prims):
        p = d.prims[i]
        if p.area_light >= 0 or p.material < 0:
            continue
        if p.shape < 0 and abs(d.spheres[~p.shape].radius - .01) < 1e-6:
            continue
        out.add(int(p.material))
    return out


def check_row_plan(pt, s, row, instances):
    """The row's instance exists, the materials in view all route to it, and what is routed there is what the row declares.
    Returns the instance index."""
    want = (row["nl"], row_mask(pt, row))
    assert want in instances, "no k_shade<%d, %#x>" % want
    index = instances.index(want)
    plan = s.shade_plan()
    seen = visible_materials(s)
    classes = {plan["material_class"][m] for m in seen}
    assert {plan["classes"][c]["instance"] for c in classes} == {index}, (index, {c: plan["classes"][c] for c in classes})
    routed = 0
    for c in classes:
        routed |= plan["classes"][c]["types"]
    lobes = pt.lobe_bits(*pt.BXDF_TYPES) | pt.lobe_bits(*("fresnel_" + f for f in pt.FRESNEL_TYPES)) | pt.TM_SCALED
    assert routed & lobes == row_types(pt, row), (sorted(pt.lobe_names(routed)), bool(routed & pt.TM_SCALED), sorted(row["kinds"]))
    assert bool(routed & pt.TM_TEXTURED) == bool(want[1] & pt.TM_TEXTURED) or want[1] == pt.TM_ALL
    if row["zoo"]:   # every material in view sits in the overflow class
        assert classes == {pt.MISS_CLASS - 1} and plan["classes"][pt.MISS_CLASS - 1]["lobes"] == pt.MAX_BXDFS
    return index


def _samples_per_material(s, integ, pool):
    """Camera samples whose closest hit has each material: one metadata pass per sample number (one sample per pixel, so a
    pixel of weight 1 holds one sample's id, the box filter's), ids to material indices through the primitives."""
    d = s.desc
    by_id = {int(d.prim_meta[i].material_id): int(d.prims[i].material) for i in range(d.n_prims) if d.prims[i].material >= 0}
    count = {}
    for k in range(s.spp):
        film, weight = integ.RenderMetadata("material", spp=1, sample_begin=k, path_pool=pool)
        ids = film[..., 0][weight == 1.0]
        for v, n in zip(*np.unique(ids, return_counts=True)):
            if int(v) in by_id:
                count[by_id[int(v)]] = count.get(by_id[int(v)], 0) + int(n)
    return count


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    d = tmp_path_factory.mktemp("shade_instances")
    st.write_texture_files(str(d))
    st.write_env_pfm(str(d / "env.pfm"))
    return d


@pytest.mark.parametrize("name", list(ROWS))
def test_instance_against_oracle(pt, ob, assets, monkeypatch, name):
    """The row's plan, its materials in view (each the closest hit of at least 8 camera samples), then exact-mode parity."""
    monkeypatch.delenv("MIPT_INSTANCES", raising=False)
    row = ROWS[name]
    s = load_row(pt, row, assets)
    assert (s.desc.n_instances > 0) == row["instanced"]
    check_row_plan(pt, s, row, pt.shade_instances())
    w, h = s.film_size
    pool = w * h * s.spp
    count = _samples_per_material(s, pt.CreatePathIntegrator(s), pool)   # (conditions on the scene first, then the render)
    for m in visible_materials(s):
        assert count.get(m, 0) >= 8, (name, m, count)
    film, weight, integ, ofilm, oweight, oc = _parity(pt, ob, s, "shade instance | " + name, render=dict(path_pool=pool))
    assert integ.pool_info()[0] <= pool


@pytest.mark.parametrize("name", [n for n in ROWS if ROWS[n]["instanced"] and not ROWS[n]["zoo"]])
def test_instanced_rows_expanded(pt, ob, assets, monkeypatch, name):
    """The instanced scenes once more with MIPT_INSTANCES=expand (read when the scene is loaded): no object instances, so the
    same materials go through the specialised instances -- asserted from the plan --, and the film is the instanced scene's
    oracle film statistically (another tree, another float path: test_object_instances_against_oracle's comparison and
    figure) and its own oracle film at _parity's bars."""
    monkeypatch.delenv("MIPT_INSTANCES", raising=False)
    row = ROWS[name]
    s = load_row(pt, row, assets)
    with ob.exact_libm():
        ofilm, _, _, _ = ob.render(s)
    monkeypatch.setenv("MIPT_INSTANCES", "expand")
    flat = load_row(pt, row, assets)
    assert flat.desc.n_instances == 0 and s.desc.n_instances > 0
    plan, instances = flat.shade_plan(), pt.shade_instances()
    used = {plan["classes"][plan["material_class"][m]]["instance"] for m in visible_materials(flat)}
    assert used and all(not (instances[i][1] & pt.TM_INSTANCES) for i in used), used
    assert len(used) > 1   # (several specialised instances share the work of the general one)
    w, h = flat.film_size
    film, _, _, _, _, _ = _parity(pt, ob, flat, "shade instance | " + name + ", expanded", render=dict(path_pool=w * h * flat.spp))
    assert _rel_l2(film, ofilm) < 0.05
