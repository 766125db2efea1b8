"""Diagnostic (needs a GPU): one line per scene of a fixed corpus with the SHA-256 of what the device rendered.

Two builds of the HIP library whose digests agree over the corpus compute the same bits: the build under test is whatever
MIPT_HIP_LIB names (default: the package's own library). Each entry is rendered as four passes of one sample per pixel
(spp=1, sample_begin=0..3) and the digest covers the four films, the four weight images and the counters of each pass. At
one sample per pixel under the box filter a pixel receives one add, so the film does not depend on the order of the adds;
the tool asserts the box filter and leaves out a scene with another one.

Usage: film_digest.py [--json FILE]
The corpus, each entry at most 32 x 32 pixels: every row of test_shade_instances_gpu.ROWS; the rows whose instance reads image
textures once more behind a realistic camera (the LENS twins of k_shade); the two textured instanced rows with their object
instance moving, behind the perspective and the realistic camera (the MOTION twins, loaded under MIPT_OBJECT_MOTION=1 in a
child process of its own); material_zoo under Integrator "path" and "spectralpath"; sphere_row_scene; the textured quad of
test_realistic_gpu behind the double-Gauss lens; a moving octahedron of tests/object_motion.py; and RenderMetadata of all
four strategies on the zoo, an instanced row and the moving scene (k_commit_metadata builds its hit vertex with k_shade's
routine). Each line also shows shade_launch_stats() of the last pass and the k_shade instances of the classes in view
(index in shade_instances(), +L the LENS twin, +M the MOTION twin); the last line counts the distinct ones."""
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
TESTS = os.path.join(ROOT, "tests")
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)

VARIANTS = {"default": {}, "motion": {"MIPT_OBJECT_MOTION": "1"}}
PASSES = 4
LENS_CAMERA = '"float aperturediameter" [8] "float focusdistance" [7.5]'
MOVE = ("Translate -.1 0 0", "Translate .1 .05 0")


def corpus(variant):
    """[(name, scene text, metadata strategies or None)] of the variant."""
    import metadata_scenes as ms
    import object_motion as om
    import realistic_camera as rc
    import scenes_text as st
    import shade_plan_scenes as sp
    import test_realistic_gpu as trg
    import test_shade_instances_gpu as tsi

    head = sp.HEAD.split("Film")[0].lstrip("\n")   # the rows' LookAt and Camera lines
    lens_head = rc.camera_block("dgauss.dat", head.split("\n")[0][len("LookAt "):], LENS_CAMERA)

    def behind_lens(text):
        assert text.count(head) == 1
        return text.replace(head, lens_head)

    def moving(text):
        assert text.count('  ObjectInstance "extra"\n') == 1
        return "TransformTimes 0 1\n" + text.replace('  ObjectInstance "extra"\n', om.pair(*MOVE) + '  ObjectInstance "extra"\n')

    rows = {name: tsi.row_text(row) for name, row in tsi.ROWS.items()}
    mover = om.lit_scene(om.mover("instance", "Translate -1 0 0", "Translate 1 .5 0"))
    out = []
    if variant == "default":
        for name, text in rows.items():
            out.append(("row/" + name, text, None))
        for name, row in tsi.ROWS.items():
            if "TM_TEXTURED" in row["tm"] or (not row["zoo"] and any(n in sp.TEXTURED for n in row["materials"])):
                out.append(("lens/" + name, behind_lens(rows[name]), None))
        zoo = st.material_zoo(res=16, depth=6)
        out.append(("zoo/path", zoo, None))
        assert zoo.count('Integrator "path"') == 1
        out.append(("zoo/spectralpath", zoo.replace('Integrator "path"', 'Integrator "spectralpath"'), None))
        out.append(("sphere_row_scene", st.sphere_row_scene(res=32), None))
        out.append(("realistic/textured quad", rc.camera_block("dgauss.dat", "0 0 8  0 0 0  0 1 0", '"float aperturediameter" [8] "float focusdistance" [10]') +
                    'Film "image" "integer xresolution" [32] "integer yresolution" [32]\nSampler "halton" "integer pixelsamples" [4]\n'
                    'Integrator "path" "integer maxdepth" [1]\n' + trg.TEX_WORLD, None))
        out.append(("metadata/zoo", zoo, ms.STRATEGIES))
        out.append(("metadata/instanced row", rows["instanced, two lobes"], ms.STRATEGIES))
    else:
        for name in ("instanced, two lobes, textured", "instanced, more lobes, textured"):
            out.append(("motion/" + name, moving(rows[name]), None))
            out.append(("motion, lens/" + name, moving(behind_lens(rows[name])), None))
        out.append(("motion/object_motion.lit_scene", mover, None))
        out.append(("metadata/object_motion.lit_scene", mover, ms.STRATEGIES))
    return out


def is_box_filter(scene):
    film = scene.desc.film
    return tuple(film.filter_radius) == (0.5, 0.5) and all(v == 1.0 for v in film.filter_table)


def instances_in_view(pt, tsi, scene):
    """The k_shade instances a render of the scene launches: those of the classes of the materials in view and of the
    escaped rays, as the LENS / MOTION twin where LaunchShade takes it."""
    plan = scene.shade_plan()
    d = scene.desc
    table = pt.shade_instances()
    lens = d.camera_type != 0 and any(d.materials[i].textured for i in range(d.n_materials))
    motion = d.n_motions > 0
    classes = {plan["material_class"][m] for m in tsi.visible_materials(scene)} | {pt.MISS_CLASS}
    out = set()
    for c in classes:
        if c in plan["classes"]:
            i = plan["classes"][c]["instance"]
            tm = table[i][1]
            out.add("%d%s%s" % (i, "+L" if lens and tm & pt.TM_TEXTURED else "", "+M" if motion and tm & pt.TM_INSTANCES else ""))
    return sorted(out)


def child(variant):
    """Renders the variant's entries in this process and prints {name: {...}} as JSON."""
    import pbrt_v3_spectral_amd as pt
    import realistic_camera as rc
    import scenes_text as st
    import test_shade_instances_gpu as tsi

    result = {}
    workdir = tempfile.mkdtemp(prefix="film_digest_")
    try:
        st.write_texture_files(workdir)
        st.write_env_pfm(os.path.join(workdir, "env.pfm"))
        for name, text, strategies in corpus(variant):
            scene = pt.Scene(text=text, base_dir=workdir)
            assert scene.errors == [], (name, scene.errors)
            w, h = scene.film_size
            assert w <= 32 and h <= 32, (name, w, h)
            if not is_box_filter(scene):
                result[name] = {"left_out": "not the box filter"}
                continue
            integ = pt.CreatePathIntegrator(scene)
            parts = {"film": hashlib.sha256(), "weight": hashlib.sha256(), "counters": hashlib.sha256()}
            counters = []
            for strategy in strategies or (None,):
                for k in range(PASSES):
                    if strategy is None:
                        film, weight = integ.Render(spp=1, sample_begin=k)
                    else:
                        film, weight = integ.RenderMetadata(strategy, spp=1, sample_begin=k)
                    parts["film"].update(film.tobytes())
                    parts["weight"].update(weight.tobytes())
                    counters.append(integ.counters.as_dict())
                    parts["counters"].update(json.dumps(counters[-1], sort_keys=True).encode())
            sub = {k: v.hexdigest() for k, v in parts.items()}
            result[name] = {"digest": hashlib.sha256("".join(sub[k] for k in sorted(sub)).encode()).hexdigest(), "parts": sub,
                            "counters": counters, "shade_launch_stats": list(integ.shade_launch_stats()),
                            "instances": instances_in_view(pt, tsi, scene)}
            integ.close()
            scene.close()
    finally:
        shutil.rmtree(workdir, ignore_errors=True)
    json.dump(result, sys.stdout)


def main(argv):
    if len(argv) == 2 and argv[0] == "--child":
        return child(argv[1])
    result = {}
    for variant, env in VARIANTS.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", variant], env=dict(os.environ, **env),
                           stdout=subprocess.PIPE, check=True)
        result.update(json.loads(r.stdout))
    seen = set()
    for name, e in result.items():
        if "left_out" in e:
            print("%-64s left out: %s" % (name, e["left_out"]))
            continue
        seen.update(e["instances"])
        print("%-64s %s  k_shade launches %d, blocks %d, instances %s" % (name, e["digest"], e["shade_launch_stats"][0],
                                                                        e["shade_launch_stats"][1], " ".join(e["instances"])))
    print("%d entries, %d distinct k_shade instances in view: %s" % (len(result), len(seen), " ".join(sorted(seen, key=lambda v: (int(v.split("+")[0]), v)))))
    if len(argv) == 2 and argv[0] == "--json":
        with open(argv[1], "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
