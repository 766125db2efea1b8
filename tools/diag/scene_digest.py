"""Diagnostic (no GPU): one line per scene of a fixed corpus with the SHA-256 of its scene cache and its message counts.

The scene cache (scene_cache.cpp) serialises everything the .pbrt front end produces -- the descriptor, every array, the
warnings and the errors, in order -- so two builds of the front end whose digests agree over the corpus produce the same
scenes. The descriptor's pointer fields (process addresses) are zeroed in the file before it is hashed.

Usage: scene_digest.py [--json FILE]
The corpus: scenes/*.pbrt, every builder of tests/scenes_text.py (random_scene for seeds 0-19), the scene texts of the other
test helper modules, and a few texts of this file's own for the directives those leave out (tests/disk_shape.py and
tests/noise_texture.py hold reference maths and no scene text: "own/disks" and "own/noise" stand in for them; a text that
does not parse is recorded by the hash of its error message, counts -1). Every scene is loaded under the
default environment; the scenes with instances, animated transforms and "hlbvh" once more under MIPT_INSTANCES=expand,
MIPT_OBJECT_MOTION=1 and MIPT_HLBVH=host. Each environment runs in a child process of its own. Everything is loaded from a
temporary directory through relative names, so no message or texture key carries the directory's name."""
import ctypes as C
import glob
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

# name -> (the environment of the child process, which scene texts it loads)
VARIANTS = {
    "default": ({}, lambda text: True),
    "expand": ({"MIPT_INSTANCES": "expand"}, lambda text: "ObjectInstance" in text),
    "motion": ({"MIPT_OBJECT_MOTION": "1"}, lambda text: "ActiveTransform" in text),
    "hlbvh-host": ({"MIPT_HLBVH": "host"}, lambda text: '"hlbvh"' in text),
}
HEADER_BYTES = 24   # magic, ABI version and three struct sizes precede mi_scene_desc in the file (scene_cache.cpp)

HEAD = ('LookAt 0 2 -8  0 0.5 0  0 1 0\nCamera "perspective" "float fov" [40]\n'
        'Film "image" "integer xresolution" [16] "integer yresolution" [12]\n%sWorldBegin\n')
TRI = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [0 0 0 1 0 0 0 1 0]\n'
HLBVH = 'Accelerator "bvh" "string splitmethod" "hlbvh"\n'
PLY = ("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\n"
       "element face 2\nproperty list uchar int vertex_indices\nend_header\n"
       "-1 0 -1\n1 0 -1\n1 0 1\n-1 0 1\n3 0 1 2\n3 0 2 3\n")
TETRA = '"integer indices" [0 1 2 0 2 3 0 3 1 1 3 2] "point P" [0 0 0  .9 0 0  .45 0 .8  .45 .9 .3]'


def own_texts():
    """The directives and the report-and-continue branches the test modules' scenes leave out."""
    w = lambda body, options="": HEAD % options + body + "WorldEnd\n"
    yield "own/disks", w('Shape "disk"\nShape "disk" "float height" [.7] "float radius" [2.5] "float innerradius" [.5] "float phimax" [200]\n'
                         'Shape "sphere"\nAttributeBegin\nAreaLightSource "diffuse" "rgb L" [1 1 1] "bool twosided" "true"\nScale 1 -2 .5\n'
                         'Shape "disk" "float radius" [2] "float bogus" [1]\nAttributeEnd\n'
                         'AttributeBegin\nAreaLightSource "diffuse"\nReverseOrientation\nTranslate 0 0 -2\nShape "sphere" "float zmin" [-.3]\nAttributeEnd\n'
                         'ObjectBegin "lamp"\nShape "disk" "float radius" [.5]\n' + TRI + 'ObjectEnd\nTranslate 3 0 0\nObjectInstance "lamp"\n')
    yield "own/noise", w('Translate 1 2 3\nScale 2 2 .5\nTexture "n" "spectrum" "fbm" "integer octaves" [5] "float roughness" [.3] "float bogus" [1]\n'
                         'Texture "w" "float" "wrinkled"\nTexture "b" "float" "scale" "texture tex1" "w" "float tex2" [.05]\n'
                         'Texture "y" "spectrum" "windy"\nTexture "k" "spectrum" "scale" "texture tex1" "n" "rgb tex2" [.5 .5 .5]\n'
                         'Texture "big" "float" "fbm" "integer octaves" [40]\nTexture "neg" "float" "wrinkled" "integer octaves" [-1]\n'
                         'Material "plastic" "texture Kd" "k" "texture Ks" "y" "texture bumpmap" "b" "texture roughness" "big"\n' + TRI +
                         TRI.rstrip("\n") + ' "texture alpha" "w"\n' + 'LightSource "point"\n')
    yield "own/textures", w('Texture "c" "float" "constant" "float value" [.25]\nTexture "cs" "spectrum" "constant" "rgb value" [.2 .4 .6]\n'
                            'Texture "m" "float" "mix" "texture tex1" "c" "float tex2" [.75] "float amount" [.3]\n'
                            'Texture "ms" "color" "mix" "texture tex1" "cs" "rgb tex2" [.9 .9 .1]\n'
                            'Texture "s" "float" "scale" "texture tex1" "c" "texture tex2" "m"\n'
                            'Texture "ss" "spectrum" "scale" "texture tex1" "cs" "texture tex2" "ms"\n'
                            'Texture "img" "spectrum" "imagemap" "string filename" "tex_a.png" "float maxanisotropy" [100] "bool useSPD" "true" "float bogus" [1]\n'
                            'Texture "img" "spectrum" "constant" "rgb value" [.5 .5 .5]\n'
                            'Texture "chk" "spectrum" "checkerboard" "string aamode" "fancy" "texture tex1" "cs"\n'
                            'Texture "chk3" "spectrum" "checkerboard" "integer dimension" [3]\nTexture "chkf" "float" "checkerboard"\n'
                            'Texture "sph" "spectrum" "imagemap" "string mapping" "spherical"\nTexture "q" "vector" "constant"\n'
                            'Texture "m" "spectrum" "marble"\nTexture "gone" "spectrum" "imagemap" "string filename" "missing.png"\n'
                            'Texture "z" "float" "constant" "float value" [0]\nTexture "one" "float" "constant" "float value" [1]\n'
                            'Material "uber" "texture Kd" "ss" "texture Ks" "chk" "texture sigma" "s"\n'
                            + TRI.rstrip("\n") + ' "texture alpha" "z" "texture shadowalpha" "one"\n'
                            + TRI.rstrip("\n") + ' "texture alpha" "nowhere" "float shadowalpha" [0]\nLightSource "distant"\n')
    yield "own/meshes", w('Shape "plymesh" "string filename" "quad.ply"\nAttributeBegin\nTranslate 0 1 0\nShape "plymesh" "string filename" "quad.ply" "float alpha" [0]\nAttributeEnd\n'
                          'Shape "plymesh" "string filename" "missing.ply"\nShape "plymesh"\n'
                          'Shape "loopsubdiv" "integer levels" [2] ' + TETRA + '\nShape "loopsubdiv" "integer nlevels" [1]\n'
                          'Shape "trianglemesh" ' + TETRA + ' "float st" [0 0 1 0 1 1 0 1] "vector S" [1 0 0] "normal N" [0 1 0]\n'
                          'Shape "trianglemesh" ' + TETRA + ' "point2 uv" [0 0 1 0] "rgb Kd" [.9 .1 .1]\n'
                          'Shape "trianglemesh" "integer indices" [0 1 7] "point P" [0 0 0 1 0 0 0 1 0]\nShape "trianglemesh" "point P" [0 0 0]\n'
                          'Shape "cone"\nObjectBegin "ply"\nShape "plymesh" "string filename" "quad.ply"\nShape "hyperboloid"\nObjectEnd\n'
                          'Translate 2 0 0\nObjectInstance "ply"\nObjectInstance "nobody"\nLightSource "spot" "float bogus" [1]\nLightSource "goniometric"\n',
                          HLBVH)
    yield "own/materials", w('Material "mix" "string namedmaterial1" "a" "string namedmaterial2" "b"\n' + TRI +
                             'Material "velvet"\n' + TRI + 'Material "hair"\n' + TRI + 'Material ""\n' + TRI +
                             'MakeNamedMaterial "nt"\nMakeNamedMaterial "p" "string type" "plastic"\nMakeNamedMaterial "p" "string type" "mirror"\n'
                             'NamedMaterial "p"\n' + TRI + 'NamedMaterial "q"\nAreaLightSource "laser"\n' + TRI +
                             'AttributeEnd\nTransformEnd\nAttributeBegin\nTransformBegin\nCoordinateSystem "here"\nCoordSysTransform "there"\n'
                             'CoordSysTransform "camera"\nMediumInterface "a" "b"\nMakeNamedMedium "fog" "string type" "homogeneous"\n'
                             'Camera "perspective"\n' + TRI + 'ObjectEnd\nObjectBegin "a"\nObjectBegin "b"\nObjectInstance "a"\n' + TRI + 'ObjectEnd\n',
                             'Shape "sphere"\nLightSource "point"\nPixelFilter "lanczos"\nSampler "maxmindist"\nAccelerator "kdtree"\n'
                             'Integrator "bdpt" "integer pixelbounds" [0 4 0]\nFilm "rgb" "float cropwindow" [0 1]\n')
    yield "own/options", w('LightSource "point" "blackbody I" [5500 2] "spectrum scale" "grey.spd" "point from" [0 3 0]\n'
                           'LightSource "distant" "spectrum L" "missing.spd" "xyz scale" [.3 .3 .3]\nInclude "part.pbrt"\nInclude "missing.pbrt"\n',
                           'Scale -1 1 1\nTransform [1 0 0 0 0 1 0 0 0 0 1 0 0 0 5 1]\nConcatTransform [1 0 0 0 0 1 0 0 0 0 1 0 0 0 -5 1]\n'
                           'Camera "perspective" "float halffov" [25] "float screenwindow" [-1 1 -1] "float shutteropen" [1] "float shutterclose" [0] "float frameaspectratio" [.5]\n'
                           'PixelFilter "sinc" "float tau" [2]\nSampler "sobol" "integer pixelsamples" [6]\n'
                           'Film "image" "float cropwindow" [.75 .25 .2 .9] "float diagonal" [50] "float scale" [2] "float maxsampleluminance" [10] "bool spectralFlag" "false" "string filename" "o.exr"\n'
                           'Integrator "spectralpath" "integer numCABands" [3] "integer pixelbounds" [2 9 2 2] "float rrthreshold" [.5] "string lightsamplestrategy" "uniform"\n'
                           'Accelerator "bvh" "string splitmethod" "middle" "integer maxnodeprims" [2]\n')
    for sampler in ('"02sequence" "integer pixelsamples" [5] "integer dimensions" [70]', '"stratified" "integer xsamples" [0] "bool jitter" "false"',
                    '"random"', '"lowdiscrepancy" "bool samplepixelcenter" "true"'):
        yield "own/sampler " + sampler.split('"')[1], w(TRI, 'Sampler %s\nAccelerator "bvh" "string splitmethod" "equal"\nIntegrator "metadata" "string strategy" "uvw"\n' % sampler)
    # the tokenizer's string escapes: every one it knows, a file name spelt with them, then one it does not know and an open string
    yield "own/escapes", w('MakeNamedMaterial "a\\tb\\n\\r\\b\\f \\\\ \\\' \\"q\\"" "string type" "matte"\nNamedMaterial "a\\tb"\n'
                           'Texture "t" "spectrum" "imagemap" "string filename" "tex\\\\\\"_a.png"\n' + TRI)
    yield "own/bad escape", w('Material "ma\\qtte"\n' + TRI)
    yield "own/open string", w('Material "matte\n' + TRI)
    yield "own/no light, gaussian", w(TRI, 'PixelFilter "gaussian" "float alpha" [1.5]\nAccelerator "bvh" "string splitmethod" "octree"\n')


def corpus(workdir):
    """[(name, scene text or None, path or None)] with the files the texts name written into workdir (the current directory)."""
    import camera_motion as cm
    import light_cases as lc
    import metadata_scenes as ms
    import object_motion as om
    import projection_cases as pc
    import realistic_camera as rc
    import scenes_text as st
    import shade_plan_scenes as sp
    import sphere_cases as sc

    st.write_texture_files(workdir)
    st.write_alpha_png(workdir)
    st.write_env_pfm(os.path.join(workdir, "env.pfm"))
    for name in pc.MAPS:
        pc.write_map(workdir, name)
    shutil.copytree(rc.LENS_DIR, os.path.join(workdir, "lenses"))
    shutil.copytree(os.path.join(ROOT, "scenes"), os.path.join(workdir, "scenes"))
    with open(os.path.join(workdir, "quad.ply"), "w") as f:
        f.write(PLY)
    with open(os.path.join(workdir, "grey.spd"), "w") as f:
        f.write("# wavelength value\n400 .5\n700 .25\n550\n")
    with open(os.path.join(workdir, "part.pbrt"), "w") as f:
        f.write('AttributeBegin\nMaterial "mirror"\n' + TRI + 'AttributeEnd\n')

    out = [("scenes/" + os.path.basename(p), None, os.path.join("scenes", os.path.basename(p)))
           for p in sorted(glob.glob(os.path.join(workdir, "scenes", "*.pbrt")))]
    add = lambda name, text: out.append((name, text, None))

    # tests/scenes_text.py
    for fn in (st.furnace_point, st.furnace_area, st.furnace_uber, st.material_zoo, st.textured_zoo, st.alpha_scene, st.bump_scene,
               st.sphere_row_scene, st.roughness_scene, st.metal_textured_scene, st.sigma_textured_scene, st.glass_rough_scene,
               st.nested_mix_scene, st.disney_textured_scene, st.instanced_scene, st.mis_span_scene):
        add("scenes_text/" + fn.__name__, fn())
    add("scenes_text/furnace_point 3 lights", st.furnace_point(n_lights=3))
    add("scenes_text/textured_zoo lens", st.textured_zoo(lens=True))
    add("scenes_text/sphere_row_scene instanced", st.sphere_row_scene(instanced=True))
    add("scenes_text/instanced_scene hlbvh", st.instanced_scene().replace("WorldBegin", HLBVH + "WorldBegin", 1))
    for kind in ("const", "map", "only_env"):
        add("scenes_text/zoo_with_infinite_light " + kind, st.zoo_with_infinite_light(kind))
    for seed in range(20):
        add("scenes_text/random_scene %d" % seed, st.random_scene(seed))
    # tests/metadata_scenes.py
    add("metadata/id_scene", ms.id_scene())
    add("metadata/id_scene path", ms.id_scene('Integrator "path"'))
    add("metadata/id_scene_fallbacks", ms.id_scene_fallbacks())
    for strategy in ms.STRATEGIES:
        add("metadata/render_scene " + strategy, ms.render_scene(strategy, light="point" if strategy == "mesh" else "infinite"))
    add("metadata/render_scene lens", ms.render_scene(lens=0.5, spp=4))
    # tests/shade_plan_scenes.py: every catalogue material once, in groups of six, through every sampler
    names = list(sp.MATERIALS)
    samplers = list(sp.SAMPLERS)
    for k in range(0, len(names), 6):
        group = names[k:k + 6]
        add("shade_plan/%s .. %s" % (group[0], group[-1]),
            sp.scene_text(group, sampler=samplers[(k // 6) % len(samplers)], infinite=(None, "const", "map")[(k // 6) % 3],
                          instanced=(k // 6) % 2 == 1, ground=group[0], hidden=group[-1:]))
    # tests/camera_motion.py
    still = cm.static_camera("3 2 8  0 0.5 0  0 1 0")
    moving = cm.moving_camera("3 2 8  0 0.5 0  0 1 0", "2 3 7  0.5 0.5 0  0 1 0", times=(0.25, 2))
    scaled = cm.moving_camera("3 2 8  0 0.5 0  0 1 0", "2 3 7  0.5 0.5 0  0 1 0", end_extra="Scale 1.5 1 1\n")
    for tag, cam in (("still", still), ("moving", moving), ("moving scaled", scaled)):
        add("camera_motion/lit_scene " + tag, cm.lit_scene(cam, sampler=("halton", "sobol", "stratified")[len(tag) % 3]))
    add("camera_motion/textured_scene", cm.textured_scene(cm.moving_camera("0 0 6  0 0 0  0 1 0", "1 0 6  0 0 0  0 1 0", camera='"float fov" [45] "float lensradius" [.05] "float focaldistance" [6]')))
    add("camera_motion/metadata_scene", cm.metadata_scene(cm.moving_camera("8 5 30  8 5 0  0 1 0", "9 5 30  8 5 0  0 1 0", camera='"float fov" [60]'), strategy="coordinates"))
    add("camera_motion/blur_scene", cm.blur_scene(0.5))
    add("camera_motion/blur_scene still", cm.blur_scene(0.5, still=True))
    # tests/object_motion.py
    slide = ("Translate -1 0 0", "Translate 1 .5 0")
    spin = ("Translate 0 1 0\nRotate 10 0 1 0", "Translate 0 1 0\nRotate 130 0 1 0\nScale 1 2 1")
    for kind in ("instance", "shape"):
        add("object_motion/lit_scene %s slide" % kind, om.lit_scene(om.mover(kind, *slide)))
        add("object_motion/bare_scene %s spin" % kind, om.bare_scene(om.mover(kind, *spin), times=(0.5, 1.5)))
    add("object_motion/shape sphere, area light", om.bare_scene(om.mover("shape", *spin, shape='Shape "sphere" "float radius" [.5]\n', before_shape='AreaLightSource "diffuse"\n')))
    add("object_motion/shape inside object", om.bare_scene('ObjectBegin "o"\n' + om.mover("shape", *slide) + 'ObjectEnd\nObjectInstance "o"\n'))
    add("object_motion/light and texture under motion", om.bare_scene(om.pair(*slide) + 'LightSource "point"\nTexture "c" "float" "constant"\nMakeNamedMaterial "m" "string type" "matte"\n' + TRI))
    add("object_motion/two_movers", om.bare_scene(om.two_movers(slide, spin)))
    add("object_motion/two_movers hlbvh", om.bare_scene(om.two_movers(slide, spin)).replace("WorldBegin", HLBVH + "WorldBegin", 1))
    add("object_motion/ramp_scene", om.ramp_scene(0.5))
    add("object_motion/ramp_scene still", om.ramp_scene(0.5, still=True))
    # tests/sphere_cases.py
    for k, name in enumerate(sc.SHAPES):
        body = 'AttributeBegin\n%s\nAttributeEnd\n' % sc.SHAPES[name]
        add("sphere_cases/" + name, sc.text(sc.PLAIN + body if k % 2 else body + sc.PLAIN, accel=HLBVH if k == 3 else ""))
    # tests/projection_cases.py
    for map_name in pc.MAPS:
        for xf_name in pc.TRANSFORMS:
            body = "AttributeBegin\n" + pc.TRANSFORMS[xf_name] + pc.light_text(pc.MAPS[map_name][0]) + "AttributeEnd\n" + lc.BALL
            add("projection/light %s, %s" % (map_name, xf_name), lc.text(body))
    add("projection/wall", pc.wall_text(pc.light_text(pc.MAPS["3x5"][0], extra=' "float bogus" [1]')))
    add("projection/wall missing map", pc.wall_text(pc.light_text("missing.pfm")))
    add("projection/wall point twin", pc.wall_text(pc.point_twin()))
    # tests/realistic_camera.py with the lens files of tests/golden/lenses
    for lens in sorted(os.listdir(rc.LENS_DIR)):
        for tag, params in (("", ""), (" ca", '"float aperturediameter" [4] "float focusdistance" [2] "bool chromaticAberrationEnabled" "true" "bool simpleweighting" "false"')):
            block = rc.camera_block(lens, params=params).replace(rc.LENS_DIR, "lenses")
            add("realistic/%s%s" % (lens, tag), cm.lit_scene(block, integrator='Integrator "spectralpath" "integer numCABands" [%d]' % (3 if tag else 1)))
    add("realistic/missing lens file", cm.lit_scene(rc.camera_block("nothing.dat").replace(rc.LENS_DIR, "lenses")))
    add("realistic/no lens file", cm.lit_scene('Camera "realistic"\n'))
    out.extend((name, text, None) for name, text in own_texts())
    assert len({name for name, _, _ in out}) == len(out)
    return out


def pointer_ranges(struct, base=0):
    """(offset, size) of every pointer-valued field of the ctypes structure, nested structures and arrays included."""
    for name, typ in struct._fields_:
        yield from _pointers_of(typ, base + getattr(struct, name).offset)


def _pointers_of(typ, offset):
    if issubclass(typ, C._Pointer) or typ in (C.c_void_p, C.c_char_p):
        yield offset, C.sizeof(typ)
    elif issubclass(typ, C.Structure):
        yield from pointer_ranges(typ, offset)
    elif issubclass(typ, C.Array):
        for k in range(typ._length_):
            yield from _pointers_of(typ._type_, offset + k * C.sizeof(typ._type_))


def child(variant):
    """Loads the variant's scenes in this process and prints {name: [digest, warnings, errors]} as JSON."""
    import pbrt_v3_spectral_amd as pt
    wanted = VARIANTS[variant][1]
    masks = list(pointer_ranges(pt.SceneDesc, HEADER_BYTES))
    result = {}
    with tempfile.TemporaryDirectory() as workdir:
        os.chdir(workdir)
        for name, text, path in corpus(workdir):
            key = name if variant == "default" else "%s [%s]" % (name, variant)
            if text is None:
                with open(path) as f:
                    if not wanted(f.read()):
                        continue
                scene = pt.Scene(path)
            elif wanted(text):
                try:
                    scene = pt.Scene(text=text, base_dir=".")
                except RuntimeError as e:   # a parse error ends the load: the message is the result
                    result[key] = [hashlib.sha256(str(e).encode()).hexdigest(), -1, -1]
                    continue
            else:
                continue
            scene.save_cache("scene.cache")
            with open("scene.cache", "rb") as f:
                image = bytearray(f.read())
            for offset, size in masks:
                image[offset:offset + size] = bytes(size)
            result[key] = [hashlib.sha256(image).hexdigest(), len(scene.warnings), len(scene.errors)]
            scene.close()
        os.chdir(ROOT)
    assert "torch" not in sys.modules and pt._hip is None
    json.dump(result, sys.stdout)


def main(argv):
    if len(argv) == 2 and argv[0] == "--child":
        return child(argv[1])
    result = {}
    for variant, (env, _) in VARIANTS.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", variant], env=dict(os.environ, **env),
                           stdout=subprocess.PIPE, check=True)
        result.update(json.loads(r.stdout))
    for name, (digest, warnings, errors) in result.items():
        print("%-60s %s  %d warnings, %d errors" % (name, digest, warnings, errors))
    if len(argv) == 2 and argv[0] == "--json":
        with open(argv[1], "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
