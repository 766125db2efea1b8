"""Scene texts of the opt-in texture mappings and classes (MIPT_TEXTURES=all), shared by the front-end tests, the fixture of
the messages these texts give without the switch (golden/texture_mapping_messages_without_switch.json) and the GPU tests."""
HEAD = ('LookAt 0 0 8  0 0 0  0 1 0\nCamera "perspective" "float fov" [40]\n'
        'Film "image" "integer xresolution" [8] "integer yresolution" [8]\n')
TRI = 'Shape "trianglemesh" "integer indices" [0 1 2] "point P" [-3 -3 -1  3 -3 -1  0 3 -1]\n'
LIGHT = 'LightSource "point" "point from" [0 4 4]\n'
CTM = 'Translate .3 -1.2 .7\nRotate 35 1 2 .5\nScale 1.5 .6 2.5\n'
IMAGE = '"string filename" "tex_c.pfm"'
FLOAT_IMAGE = '"string filename" "rough.pfm"'

# every body stands between WorldBegin and WorldEnd; image files are scenes_text.write_texture_files' (base_dir)
FRONTEND = {
    "classes": LIGHT + "TransformBegin\n" + CTM +
               'Texture "u" "spectrum" "uv" "float uscale" [2] "float vdelta" [.25]\n'
               'Texture "d" "spectrum" "dots" "rgb inside" [.8 .1 .1] "rgb outside" [.1 .2 .9] "float uscale" [6] "float vscale" [5]\n'
               'Texture "df" "float" "dots" "float inside" [.7] "float outside" [.2]\n'
               'Texture "b" "float" "bilerp" "float v00" [.1] "float v01" [.2] "float v10" [.3] "float v11" [.9] "float udelta" [.5]\n'
               'Texture "cf" "float" "checkerboard" "float tex1" [.4] "float tex2" [.05] "float uscale" [4] "float vscale" [3] "string aamode" "none"\n'
               'Texture "c3" "spectrum" "checkerboard" "integer dimension" [3] "rgb tex1" [.9 .9 .2] "rgb tex2" [.1 .1 .1]\n'
               'Texture "c3f" "float" "checkerboard" "integer dimension" [3] "float tex1" [.3] "float tex2" [.6] "string aamode" "none"\n'
               'Texture "fu" "float" "uv"\n'
               "TransformEnd\n" + 'Material "matte" "texture Kd" "d"\n' + TRI,
    "mappings": LIGHT + "TransformBegin\n" + CTM +
                'Texture "is" "spectrum" "imagemap" ' + IMAGE + ' "string mapping" "spherical"\n'
                'Texture "ic" "float" "imagemap" ' + FLOAT_IMAGE + ' "string mapping" "cylindrical"\n'
                'Texture "ip" "spectrum" "imagemap" ' + IMAGE + ' "string mapping" "planar" "vector v1" [.5 0 .25] "vector v2" [0 2 0] "float udelta" [.1] "float vdelta" [.2]\n'
                'Texture "cp" "spectrum" "checkerboard" "string mapping" "planar" "rgb tex1" [.9 .9 .9] "rgb tex2" [.2 .2 .2]\n'
                'Texture "ds" "spectrum" "dots" "string mapping" "spherical"\n'
                'Texture "uc" "spectrum" "uv" "string mapping" "cylindrical"\n'
                'Texture "bp" "float" "bilerp" "string mapping" "planar"\n'
                "TransformEnd\n" + 'Material "matte" "texture Kd" "is"\n' + TRI,
    "unknown mapping": LIGHT + 'Texture "d" "spectrum" "dots" "string mapping" "conformal" "float uscale" [3]\nMaterial "matte" "texture Kd" "d"\n' + TRI,
    "unknown mapping of an image": LIGHT + 'Texture "i" "spectrum" "imagemap" ' + IMAGE + ' "string mapping" "conformal"\nMaterial "matte" "texture Kd" "i"\n' + TRI,
    "spectrum bilerp": LIGHT + 'Texture "b" "spectrum" "bilerp"\n' + TRI,
    "marble": LIGHT + 'Texture "m" "spectrum" "marble"\n' + TRI,
    "ptex": LIGHT + 'Texture "p" "spectrum" "ptex" "string filename" "none.ptx"\n' + TRI,
    "dimension 4": LIGHT + 'Texture "c" "spectrum" "checkerboard" "integer dimension" [4]\n' + TRI,
    "dots of textures": LIGHT + 'Texture "i" "spectrum" "imagemap" ' + IMAGE + '\nTexture "d" "spectrum" "dots" "texture inside" "i"\n' + TRI,
    "float checkerboard of textures": LIGHT + 'Texture "i" "float" "imagemap" ' + FLOAT_IMAGE + '\nTexture "c" "float" "checkerboard" "texture tex2" "i"\n' + TRI,
    "alpha dots": LIGHT + 'Texture "d" "float" "dots"\n' + TRI.rstrip("\n") + ' "texture alpha" "d"\n',
    "shadowalpha spherical image": LIGHT + 'Texture "i" "float" "imagemap" ' + FLOAT_IMAGE + ' "string mapping" "spherical"\n' + TRI.rstrip("\n") + ' "texture shadowalpha" "i"\n',
    "alpha 3-D checkerboard": LIGHT + 'Texture "c" "float" "checkerboard" "integer dimension" [3]\n' + TRI.rstrip("\n") + ' "texture alpha" "c"\n',
    "bindings": LIGHT +
                'Texture "d" "spectrum" "dots"\nTexture "u" "spectrum" "uv"\nTexture "c3" "spectrum" "checkerboard" "integer dimension" [3]\n'
                'Texture "b" "float" "bilerp"\nTexture "bs" "float" "scale" "texture tex1" "b" "float tex2" [.05]\n'
                'Texture "cf" "float" "checkerboard" "float tex1" [.3] "float tex2" [.1]\nTexture "df" "float" "dots" "float inside" [10] "float outside" [40]\n'
                'Texture "ic" "float" "imagemap" ' + FLOAT_IMAGE + ' "string mapping" "cylindrical"\n'
                'Material "matte" "texture Kd" "d" "texture sigma" "df" "texture bumpmap" "bs"\n' + TRI +
                'Material "plastic" "texture Kd" "u" "texture Ks" "c3" "texture roughness" "cf"\n' + TRI +
                'Material "uber" "texture Kd" "d" "texture uroughness" "cf" "texture vroughness" "ic"\n' + TRI +
                'Material "disney" "texture color" "c3" "texture roughness" "cf"\n' + TRI +
                'Material "mirror" "texture Kr" "u"\n' + TRI +
                'Texture "sd" "spectrum" "scale" "texture tex1" "d" "rgb tex2" [.5 .25 .125]\nMaterial "matte" "texture Kd" "sd"\n' + TRI,
    "plan": LIGHT + 'Texture "n" "spectrum" "dots"\nMaterial "matte" "texture Kd" "n"\n' + TRI + 'Material "plastic" "texture Kd" "n"\n' + TRI + 'Material "matte"\n' + TRI,
    "plan with instances": LIGHT + 'Texture "n" "spectrum" "uv" "string mapping" "planar"\nMaterial "matte" "texture Kd" "n"\n' + TRI +
                           'ObjectBegin "o"\n' + TRI + 'ObjectEnd\nObjectInstance "o"\n',
}


def text(name):
    return HEAD + "WorldBegin\n" + FRONTEND[name] + "WorldEnd\n"
