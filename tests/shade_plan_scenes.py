"""Materials and scene texts for the shading-plan tests (test_shade_plan.py on the CPU, test_shade_instances_gpu.py on the
device): every material family the front end accepts, in the parameter variants that change its lobe list, plain and with an
image texture or bump map, by name. A scene is made of catalogue names -- one primitive per material -- under a context: a
sampler, with or without an infinite light, with or without an ObjectInstance.

An entry is the .pbrt text that makes the material current: a Material line, or MakeNamedMaterial lines and a NamedMaterial
line for a mix. The textured entries use the textures of TEXTURES, whose files scenes_text.write_texture_files() writes."""
import itertools

TEXTURES = """
Texture "colour" "spectrum" "imagemap" "string filename" "tex_c.pfm" "float uscale" [2] "float vscale" [2]
Texture "colour2" "spectrum" "imagemap" "string filename" "tex_b.tga" "bool trilinear" ["true"]
Texture "bumps" "float" "imagemap" "string filename" "tex_a.png" "float uscale" [3] "float vscale" [3] "float scale" [.04]
Texture "rough" "float" "imagemap" "string filename" "rough.pfm"
Texture "sig" "float" "imagemap" "string filename" "tex_a.png" "float scale" [30]
"""

PLAIN = {
    "matte": 'Material "matte" "rgb Kd" [.5 .4 .3]',
    "matte sigma": 'Material "matte" "rgb Kd" [.3 .5 .4] "float sigma" [25]',
    "matte black": 'Material "matte" "rgb Kd" [0 0 0]',   # no lobe at all
    "plastic": 'Material "plastic" "rgb Kd" [.1 .2 .6] "rgb Ks" [.5 .5 .5] "float roughness" [.08]',
    "plastic Kd black": 'Material "plastic" "rgb Kd" [0 0 0] "rgb Ks" [.5 .5 .5] "float roughness" [.1]',
    "plastic Ks black": 'Material "plastic" "rgb Kd" [.4 .2 .6] "rgb Ks" [0 0 0]',
    "glass": 'Material "glass" "float index" [1.5]',
    "glass Kr black": 'Material "glass" "rgb Kr" [0 0 0] "rgb Kt" [.9 .9 1]',
    "glass Kt black": 'Material "glass" "rgb Kr" [.9 1 .9] "rgb Kt" [0 0 0]',
    "glass rough": 'Material "glass" "float index" [1.4] "float uroughness" [.1] "float vroughness" [.2] "rgb Kt" [.9 .9 1]',
    "glass rough Kr black": 'Material "glass" "float uroughness" [.1] "float vroughness" [.1] "rgb Kr" [0 0 0]',
    "glass rough Kt black": 'Material "glass" "float uroughness" [.2] "float vroughness" [.1] "rgb Kt" [0 0 0]',
    "mirror": 'Material "mirror" "rgb Kr" [.8 .8 .8]',
    "metal": 'Material "metal" "float roughness" [.2]',
    "metal spectra": 'Material "metal" "spectrum eta" [400 1.5 550 0.9 700 0.3] "spectrum k" [400 2.0 550 2.6 700 4.1] '
                     '"float uroughness" [.05] "float vroughness" [.3]',
    "substrate": 'Material "substrate" "rgb Kd" [.5 .2 .1] "rgb Ks" [.3 .3 .3] "float uroughness" [.1] "float vroughness" [.25]',
    "translucent": 'Material "translucent" "rgb Kd" [.5 .5 .3] "rgb Ks" [.3 .3 .3] "rgb reflect" [.6 .6 .6] "rgb transmit" [.4 .4 .4] "float roughness" [.15]',
    "translucent Kd black": 'Material "translucent" "rgb Kd" [0 0 0] "rgb Ks" [.3 .3 .3] "rgb reflect" [.6 .6 .6] "rgb transmit" [.4 .4 .4]',
    "translucent Ks black": 'Material "translucent" "rgb Kd" [.5 .5 .3] "rgb Ks" [0 0 0] "rgb reflect" [.6 .6 .6] "rgb transmit" [.4 .4 .4]',
    "translucent reflect black": 'Material "translucent" "rgb Kd" [.5 .5 .3] "rgb Ks" [.3 .3 .3] "rgb reflect" [0 0 0] "rgb transmit" [.7 .7 .7]',
    "translucent transmit black": 'Material "translucent" "rgb Kd" [.5 .5 .3] "rgb Ks" [.3 .3 .3] "rgb reflect" [.6 .6 .6] "rgb transmit" [0 0 0]',
    "disney": 'Material "disney" "rgb color" [.2 .5 .3] "float roughness" [.3]',
    "disney thin": 'Material "disney" "rgb color" [.7 .6 .2] "float roughness" [.2] "bool thin" ["true"] "float flatness" [.3] "float difftrans" [.8]',
    "disney spectrans": 'Material "disney" "rgb color" [.7 .6 .5] "float spectrans" [.6] "float roughness" [.2]',
    "disney clearcoat": 'Material "disney" "rgb color" [.5 .2 .2] "float clearcoat" [.6] "float roughness" [.4]',
    "disney sheen": 'Material "disney" "rgb color" [.2 .2 .6] "float sheen" [.7] "float sheentint" [.3]',
    "disney metallic": 'Material "disney" "rgb color" [.8 .6 .3] "float metallic" [1] "float roughness" [.3] "float anisotropic" [.3]',   # one lobe
    "disney all": 'Material "disney" "rgb color" [.7 .6 .2] "float metallic" [.3] "float spectrans" [.5] "float roughness" [.2] "bool thin" ["true"] '
                  '"float flatness" [.3] "float difftrans" [.8] "float sheen" [.5] "float clearcoat" [.6]',   # eight lobes
}

# "uber" with each of Kd, Ks, Kr, Kt present (d, s, r, t) and an opacity below one (o: a specular transmission lobe in
# front of the others): "uber dsrto" is the five-lobe one, "uber" alone has no lobe. (An opacity of one is the default's:
# "rgb opacity" [1 1 1] is a spectrum a little below one in some bins, and that lobe appears.)
_UBER = {"d": ('"rgb Kd" [.3 .1 .1]', '"rgb Kd" [0 0 0]'), "s": ('"rgb Ks" [.4 .4 .4] "float roughness" [.05]', '"rgb Ks" [0 0 0]'),
         "r": ('"rgb Kr" [.2 .2 .2]', '"rgb Kr" [0 0 0]'), "t": ('"rgb Kt" [.3 .3 .2]', '"rgb Kt" [0 0 0]'),
         "o": ('"rgb opacity" [.8 .8 .8]', '')}
for _n in range(6):
    for _parts in itertools.combinations("dsrto", _n):
        PLAIN[("uber " + "".join(_parts)).strip()] = 'Material "uber" ' + " ".join(_UBER[k][0 if k in _parts else 1] for k in "dsrto").strip()


def _mix(name, a, b, amount="[.7 .5 .3]"):
    return 'Material "mix" "string namedmaterial1" "%s" "string namedmaterial2" "%s" "rgb amount" %s' % (a, b, amount)


def _named(name, entry):
    """MakeNamedMaterial text of a catalogue Material line."""
    assert entry.startswith('Material "')
    head, rest = entry.split(" ", 2)[1:]
    return 'MakeNamedMaterial "%s" "string type" %s %s' % (name, head, rest)


def _mix_entry(tag, a, b, table):
    """A mix of the catalogue entries a and b (plain Material lines of `table`)."""
    return "\n".join([_named(tag + ".1", table[a]), _named(tag + ".2", table[b]), _mix(tag, tag + ".1", tag + ".2")])


def _mix_of_mixes(tag, a, b, c, d, table):
    """mix(mix(a, b), mix(c, d)); d = None: mix(mix(a, b), c)."""
    out = [_named(tag + ".a", table[a]), _named(tag + ".b", table[b]), _named(tag + ".c", table[c])]
    out.append('MakeNamedMaterial "%s.ab" "string type" "mix" "string namedmaterial1" "%s.a" "string namedmaterial2" "%s.b" "rgb amount" [.6 .6 .4]' % (tag, tag, tag))
    if d is None:
        return "\n".join(out + [_mix(tag, tag + ".ab", tag + ".c")])
    out.append(_named(tag + ".d", table[d]))
    out.append('MakeNamedMaterial "%s.cd" "string type" "mix" "string namedmaterial1" "%s.c" "string namedmaterial2" "%s.d" "rgb amount" [.3 .5 .5]' % (tag, tag, tag))
    return "\n".join(out + [_mix(tag, tag + ".ab", tag + ".cd")])


PLAIN.update({
    "mix matte matte": _mix_entry("mmm", "matte", "matte sigma", PLAIN),                  # two scaled diffuse lobes
    "mix plastic mirror": _mix_entry("mpm", "plastic", "mirror", PLAIN),                  # three
    "mix matte metal": _mix_entry("mme", "matte", "metal", PLAIN),                        # two, a conductor
    "mix plastic metal": _mix_entry("mpe", "plastic", "metal", PLAIN),                    # three, a conductor
    "mix glass substrate": _mix_entry("mgs", "glass", "substrate", PLAIN),                # two
    "mix uber5 matte": _mix_entry("mum", "uber dsrto", "matte", PLAIN),                   # six
    "mix disney matte": _mix_entry("mdm", "disney", "matte", PLAIN),                      # four, Disney's among them
    "mix translucent metal": _mix_entry("mtm", "translucent", "metal spectra", PLAIN),    # five
    "mix of mixes": _mix_of_mixes("mom", "plastic", "mirror", "matte", "glass", PLAIN),   # five, twice scaled
    "mix of mix small": _mix_of_mixes("mos", "matte", "mirror", "matte sigma", None, PLAIN),   # three
    "mix of mixes 8": _mix_of_mixes("mo8", "translucent", "substrate", "plastic", "metal", PLAIN),   # eight
})

TEXTURED = {
    "matte tex": 'Material "matte" "texture Kd" "colour"',
    "matte sigma tex": 'Material "matte" "rgb Kd" [.5 .5 .4] "texture sigma" "sig"',
    "matte bump": 'Material "matte" "rgb Kd" [.5 .4 .3] "texture bumpmap" "bumps"',
    "plastic tex": 'Material "plastic" "texture Kd" "colour" "rgb Ks" [.3 .3 .3] "float roughness" [.15]',
    "plastic Ks tex": 'Material "plastic" "rgb Kd" [.2 .2 .5] "texture Ks" "colour2"',
    "plastic rough tex": 'Material "plastic" "rgb Kd" [.2 .4 .5] "rgb Ks" [.4 .4 .4] "texture roughness" "rough"',
    "plastic bump": 'Material "plastic" "rgb Kd" [.1 .2 .6] "rgb Ks" [.5 .5 .5] "texture bumpmap" "bumps"',
    "glass tex": 'Material "glass" "texture Kt" "colour2" "rgb Kr" [.9 .9 .9]',
    "glass rough map": 'Material "glass" "texture uroughness" "rough" "float vroughness" [.1]',
    "glass bump": 'Material "glass" "float index" [1.5] "texture bumpmap" "bumps"',
    "mirror tex": 'Material "mirror" "texture Kr" "colour"',
    "mirror bump": 'Material "mirror" "rgb Kr" [.8 .8 .8] "texture bumpmap" "bumps"',
    "metal tex": 'Material "metal" "texture eta" "colour" "texture k" "colour2" "float roughness" [.08]',
    "metal rough tex": 'Material "metal" "texture roughness" "rough"',
    "substrate tex": 'Material "substrate" "texture Kd" "colour2" "texture Ks" "colour" "float uroughness" [.2] "float vroughness" [.1]',
    "substrate bump": 'Material "substrate" "rgb Kd" [.5 .2 .1] "rgb Ks" [.3 .3 .3] "texture bumpmap" "bumps"',
    "translucent tex": 'Material "translucent" "texture Kd" "colour" "rgb Ks" [.2 .2 .2] "rgb reflect" [.4 .5 .4] "rgb transmit" [.5 .4 .5]',
    "translucent bump": 'Material "translucent" "rgb Kd" [.5 .5 .3] "rgb Ks" [.3 .3 .3] "rgb reflect" [.6 .6 .6] "rgb transmit" [0 0 0] "texture bumpmap" "bumps"',
    "uber tex": 'Material "uber" "texture Kd" "colour" "texture Ks" "colour2" "rgb Kr" [.1 .1 .1] "float roughness" [.2]',
    "uber5 tex": 'Material "uber" "texture Kd" "colour" "rgb Ks" [.4 .4 .4] "rgb Kr" [.2 .2 .2] "rgb Kt" [.3 .3 .2] "rgb opacity" [.8 .8 .8]',
    "uber bump": 'Material "uber" "rgb Kd" [.3 .1 .1] "rgb Ks" [0 0 0] "rgb Kr" [.2 .2 .2] "texture bumpmap" "bumps"',
    "disney tex": 'Material "disney" "texture color" "colour" "float roughness" [.4] "float speculartint" [.6]',
    "disney thin tex": 'Material "disney" "texture color" "colour" "bool thin" ["true"] "float flatness" [.4] "float difftrans" [.8] "float eta" [1.4]',
    "disney spectrans tex": 'Material "disney" "texture color" "colour2" "float spectrans" [.7] "float roughness" [.2]',
    "disney clearcoat tex": 'Material "disney" "texture color" "colour2" "float clearcoat" [.5] "float anisotropic" [.4]',
    "disney sheen tex": 'Material "disney" "texture color" "colour" "float sheen" [.7] "float sheentint" [.3]',
    "disney metallic tex": 'Material "disney" "texture color" "colour" "float metallic" [1] "float roughness" [.3]',   # one lobe
    "disney rough tex": 'Material "disney" "rgb color" [.7 .4 .2] "texture roughness" "rough" "float sheen" [.4]',
    "disney all tex": 'Material "disney" "texture color" "colour" "float metallic" [.3] "float spectrans" [.5] "float roughness" [.2] "bool thin" ["true"] '
                      '"float flatness" [.3] "float difftrans" [.8] "float sheen" [.5] "float clearcoat" [.6]',
}
_BOTH = dict(PLAIN, **TEXTURED)
TEXTURED.update({
    "mix plastic tex mirror": _mix_entry("xpm", "plastic tex", "mirror", _BOTH),                 # three
    "mix matte tex matte": _mix_entry("xmm", "matte tex", "matte", _BOTH),                       # two
    "mix matte bump mirror": _mix_entry("xbm", "matte bump", "mirror", _BOTH),                   # the first material's bump map counts
    "mix disney tex matte": _mix_entry("xdm", "disney tex", "matte", _BOTH),                     # four, textured Disney's among them
    "mix uber5 tex matte": _mix_entry("xum", "uber5 tex", "matte", _BOTH),                       # six
    "mix of mixes tex": _mix_of_mixes("xom", "plastic tex", "mirror", "matte", "glass", _BOTH),  # five
    "mix of mixes 8 tex": _mix_of_mixes("xo8", "translucent", "substrate tex", "plastic", "metal", _BOTH),   # eight
})
MATERIALS = dict(PLAIN, **TEXTURED)

SAMPLERS = {
    "halton": 'Sampler "halton" "integer pixelsamples" [%d]',
    "sobol": 'Sampler "sobol" "integer pixelsamples" [%d]',
    "random": 'Sampler "random" "integer pixelsamples" [%d]',
    "02sequence": 'Sampler "02sequence" "integer pixelsamples" [%d]',
    "stratified": 'Sampler "stratified" "integer xsamples" [4] "integer ysamples" [%d]',   # (spp / 4 rows of four)
}


def sampler_line(sampler, spp):
    assert spp % 4 == 0 or sampler != "stratified"
    return SAMPLERS[sampler] % (spp // 4 if sampler == "stratified" else spp)


LIGHTS = """
AttributeBegin
  %s
  AreaLightSource "diffuse" "rgb L" [18 17 15]
  Translate 0 5 -1
  Shape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-1.2 0 -1.2  1.2 0 -1.2  1.2 0 1.2  -1.2 0 1.2]
AttributeEnd
LightSource "point" "rgb I" [6 6 8] "point from" [-4 3 -3]
LightSource "distant" "rgb L" [.4 .4 .5] "point from" [0 10 -4] "point to" [0 0 0]
LightSource "spot" "rgb I" [40 36 30] "point from" [3 4 -4] "point to" [0.5 0 -1] "float coneangle" [30] "float conedeltaangle" [8]
"""
INFINITE = {"const": 'LightSource "infinite" "rgb L" [.4 .5 .7]\n',
            "map": 'AttributeBegin\nRotate -90 1 0 0\nRotate 30 0 0 1\nLightSource "infinite" "rgb L" [.6 .6 .6] "string mapname" "env.pfm"\nAttributeEnd\n'}

HEAD = """
LookAt 0 3.2 -7  0 0.4 -0.5  0 1 0
Camera "perspective" "float fov" [36]
Film "image" "integer xresolution" [%(res)d] "integer yresolution" [%(res)d]
%(sampler)s
Integrator "path" "integer maxdepth" [%(depth)d] "string lightsamplestrategy" "power"
WorldBegin
"""

_QUAD_UV = '"float uv" [0 0 1 0 1 1 0 1]'
# an object used once, off to the side but in the light: the scene then has object instances (every class takes a TM_ALL
# instance), and its own material is one of the scene's
INSTANCE = """
ObjectBegin "extra"
  Shape "sphere" "float radius" [.3]
ObjectEnd
AttributeBegin
  Translate %g %g %g
  ObjectInstance "extra"
AttributeEnd
"""


def _slots(n):
    """Centres of n small spheres (radius .32) in rows across the ground in front of the camera, back rows raised."""
    per_row = 6
    out = []
    for i in range(n):
        row, col = divmod(i, per_row)
        in_row = min(per_row, n - row * per_row)
        out.append(((col - (in_row - 1) / 2) * .8, .33 + .18 * row, -2.2 + .9 * row))
    return out


def scene_text(names, sampler="halton", infinite=None, instanced=False, res=24, spp=16, depth=5, ground=None, hidden=(), textures=None):
    """One sphere per catalogue name in `names`, in view, on a ground quad of the material `ground` (None: no ground), lit
    by an area, a point, a distant and a spot light and, with infinite = "const" / "map", an infinite light as well.
    hidden: catalogue names declared first on tiny spheres far behind the camera, where no path arrives (they only take
    shading classes). instanced: one ObjectInstance of a sphere with the last visible material."""
    every = list(hidden) + ([ground] if ground else []) + list(names)
    if textures is None:
        textures = any(n in TEXTURED for n in every)
    t = HEAD % dict(res=res, depth=depth, sampler=sampler_line(sampler, spp))
    if textures:
        t += TEXTURES
    t += LIGHTS % MATERIALS[every[0]] + (INFINITE[infinite] if infinite else "")   # (the emitter's quad has a material too: the first one)
    for k, n in enumerate(hidden):
        t += 'AttributeBegin\n%s\nTranslate %g -50 -90\nShape "sphere" "float radius" [.01]\nAttributeEnd\n' % (MATERIALS[n], 2 * k)
    if ground:
        t += ('AttributeBegin\n%s\nShape "trianglemesh" "integer indices" [0 1 2 0 2 3] "point P" [-7 0 -7  7 0 -7  7 0 7  -7 0 7] %s\nAttributeEnd\n'
              % (MATERIALS[ground], _QUAD_UV))
    slots = _slots(len(names) + (1 if instanced else 0))
    for n, (x, y, z) in zip(names, slots):
        t += 'AttributeBegin\n%s\nTranslate %g %g %g\nRotate 40 0 1 0\nShape "sphere" "float radius" [.32]\nAttributeEnd\n' % (MATERIALS[n], x, y, z)
    if instanced:
        t += "AttributeBegin\n" + MATERIALS[names[-1]] + INSTANCE % slots[-1] + "AttributeEnd\n"
    return t + "WorldEnd\n"
