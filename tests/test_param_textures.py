"""Bitmaps on specular colours, roughness and mask opacity — the parts that need no GPU: the XML loader (which parameter fills which key,
averages, `channel`, refusals), the flat scene container's optional block, and the layout of ppg_material_textures.  The scene builders at
the end are shared with tests/test_param_textures_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ppg_host
from ppg_host import mitsuba_xml
from conftest import GOLDEN, PKG, ROOT

f32 = np.float32

XML = """<?xml version="1.0"?>
<scene version="0.5.0">
  <integrator type="guided_path"> <string name="budgetType" value="spp"/> <float name="budget" value="4"/> </integrator>
  <sensor type="perspective">
    <float name="fov" value="45"/>
    <transform name="toWorld"> <lookAt origin="0, 0, -5" target="0, 0, 0" up="0, 1, 0"/> </transform>
    <film type="hdrfilm"> <integer name="width" value="16"/> <integer name="height" value="12"/> <rfilter type="box"/> </film>
  </sensor>
  <texture type="bitmap" id="named"> <string name="filename" value="t.pfm"/> <string name="filterType" value="nearest"/> </texture>
  %s
  <shape type="rectangle"> <bsdf type="diffuse"/> <emitter type="area"> <rgb name="radiance" value="1"/> </emitter> </shape>
</scene>
"""
TEXELS = np.array([[[0.25, 0.5, 0.75], [0.75, 0.5, 0.25]], [[0.125, 0.25, 0.5], [0.375, 0.25, 0.5]]], f32)  # 2 x 2, average (0.375, 0.375, 0.5)
AVERAGE = (0.375, 0.375, 0.5)
INLINE = '<texture name="%s" type="bitmap"> <string name="filename" value="t.pfm"/> <string name="filterType" value="nearest"/> </texture>'
REF = '<ref name="%s" id="named"/>'


QUAD_OBJ = "v -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nf 1/1 2/2 3/3 4/4\n"  # [-1, 1]^2 facing +z, uv = [0, 1]^2
OBJ_SHAPE = '<shape type="obj"> <string name="filename" value="quad.obj"/> %s %s </shape>'  # (transform, bsdf)


REF_DATA = "/root/reference/mitsuba/data"
needs_ref = pytest.mark.skipif(not os.path.exists(os.path.join(REF_DATA, "microfacet", "beckmann.dat")), reason="Mitsuba data tables not mounted")


def _load(tmp_path, bsdf, strict=True, write=True, data_dir=None):
    from ppg_host import imageio
    if write:
        imageio.write_pfm(str(tmp_path / "t.pfm"), TEXELS)
    (tmp_path / "quad.obj").write_text(QUAD_OBJ)
    p = tmp_path / "s.xml"
    p.write_text(XML % (OBJ_SHAPE % ("", bsdf)))
    desc, _, info = ppg_host.load_scene(str(p), strict=strict, data_dir=data_dir)
    return desc, desc.materials[int(desc.tri_material[0])], info


# (plug-in, its parameters, the textured parameter, the material key of the slot, the record's field)
PARAMETERS = [
    ("conductor", '<string name="material" value="none"/>', "specularReflectance", "texture", "reflectance"),
    ("roughconductor", '<string name="material" value="none"/>', "specularReflectance", "texture", "reflectance"),
    ("dielectric", "", "specularReflectance", "texture", "reflectance"),
    ("thindielectric", "", "specularReflectance", "texture", "reflectance"),
    ("roughdielectric", "", "specularReflectance", "texture", "reflectance"),
    ("plastic", "", "specularReflectance", "specular_texture", "specular"),
    ("dielectric", "", "specularTransmittance", "specular_texture", "specular"),
    ("thindielectric", "", "specularTransmittance", "specular_texture", "specular"),
    ("roughdielectric", "", "specularTransmittance", "specular_texture", "specular"),
    ("roughconductor", '<string name="material" value="none"/>', "alpha", "alpha_texture", "alpha"),
    ("roughdielectric", "", "alpha", "alpha_texture", "alpha"),
]


@pytest.mark.parametrize("how", ["inline", "ref"])
@pytest.mark.parametrize("plugin,params,name,key,field", PARAMETERS)
def test_each_parameter_loads_and_fills_its_key(tmp_path, plugin, params, name, key, field, how):
    tex = (INLINE if how == "inline" else REF) % name
    desc, m, info = _load(tmp_path, '<bsdf type="%s"> %s %s </bsdf>' % (plugin, params, tex))
    assert not info["warnings"]
    assert m[key] == 0 and len(desc.textures) == 1
    assert [k for k in mitsuba_xml.TEXTURE_KEYS if k in m] == [key]
    assert np.array_equal(desc.textures[0]["rgb"], TEXELS) and desc.textures[0]["nearest"]
    if field == "alpha":  # eval(its).average() of the texture's average
        assert m["alpha"] == float((f32(0.375) + f32(0.375) + f32(0.5)) / f32(3))
    else:
        assert tuple(m[field]) == AVERAGE
    assert desc.texcoords is not None and np.isfinite(desc.texcoords[:4]).all()  # the mesh's texture coordinates are kept for a material with any slot


def test_mask_opacity(tmp_path):
    desc, m, _ = _load(tmp_path, '<bsdf type="mask"> %s <bsdf type="diffuse"/> </bsdf>' % (INLINE % "opacity"))
    assert m["opacity_texture"] == 0 and tuple(m["opacity"]) == AVERAGE and m["type"] == 0
    desc, m, _ = _load(tmp_path, '<bsdf type="mask"> %s <bsdf type="twosided"> <bsdf type="diffuse"/> </bsdf> </bsdf>' % (REF % "opacity"))
    assert m["opacity_texture"] == 0 and m["twosided"] and tuple(m["opacity"]) == AVERAGE


@needs_ref  # (roughplastic is converted with Mitsuba's own rough-transmittance tables, data/microfacet/*.dat)
@pytest.mark.parametrize("how", ["inline", "ref"])
def test_roughplastic_specular_reflectance(tmp_path, how):
    tex = (INLINE if how == "inline" else REF) % "specularReflectance"
    desc, m, info = _load(tmp_path, '<bsdf type="roughplastic"> <float name="alpha" value="0.2"/> %s </bsdf>' % tex, data_dir=REF_DATA)
    assert not info["warnings"] and m["type"] == 9
    assert m["specular_texture"] == 0 and len(desc.textures) == 1 and tuple(m["specular"]) == AVERAGE
    assert [k for k in mitsuba_xml.TEXTURE_KEYS if k in m] == ["specular_texture"]


def test_a_texture_shared_by_two_parameters_is_stored_once(tmp_path):
    bsdf = '<bsdf type="roughdielectric"> %s %s %s </bsdf>' % (INLINE % "specularReflectance", REF % "specularTransmittance", INLINE % "alpha")
    desc, m, _ = _load(tmp_path, bsdf)
    assert len(desc.textures) == 1 and (m["texture"], m["specular_texture"], m["alpha_texture"]) == (0, 0, 0)
    plastic = '<bsdf type="plastic"> %s %s </bsdf>' % (INLINE % "diffuseReflectance", REF % "specularReflectance")
    desc, m, _ = _load(tmp_path, plastic)
    assert len(desc.textures) == 1 and (m["texture"], m["specular_texture"]) == (0, 0)
    assert tuple(m["reflectance"]) == AVERAGE and tuple(m["specular"]) == AVERAGE


@pytest.mark.parametrize("bsdf,needle", [
    ('<bsdf type="roughplastic"> %s </bsdf>' % (INLINE % "alpha"), "roughplastic: a texture on 'alpha'"),
    ('<bsdf type="roughconductor"> <string name="material" value="none"/> %s </bsdf>' % (INLINE % "alphaU"), "alphaU"),
    ('<bsdf type="roughdielectric"> %s </bsdf>' % (REF % "alphaV"), "alphaV"),
    ('<bsdf type="plastic"> <texture name="specularReflectance" type="checkerboard"/> </bsdf>', "checkerboard"),
    ('<bsdf type="dielectric"> <texture name="specularReflectance" type="bitmap"/> </bsdf>', "texture on 'specularReflectance': bitmap texture without filename"),
    ('<bsdf type="plastic"> <texture name="specularReflectance" type="bitmap"> <string name="filename" value="t.pfm"/> <string name="channel" value="q"/> </texture> </bsdf>',
     "channel 'q'"),
    ('<bsdf type="diffuse"> <texture name="reflectance" type="scale"/> </bsdf>', "scale"),
])
def test_refusals_name_the_parameter(tmp_path, bsdf, needle):
    with pytest.raises(mitsuba_xml.SceneError) as ei:
        _load(tmp_path, bsdf)
    assert needle in str(ei.value)


def test_a_missing_file_raises_in_strict_mode_and_falls_back_in_lenient_mode(tmp_path):
    bsdf = '<bsdf type="mask"> %s <bsdf type="diffuse"/> </bsdf>' % (INLINE % "opacity")
    with pytest.raises(mitsuba_xml.SceneError) as ei:
        _load(tmp_path, bsdf, write=False)
    assert "texture on 'opacity'" in str(ei.value) and "not found" in str(ei.value)
    desc, m, info = _load(tmp_path, bsdf, strict=False, write=False)
    assert "opacity_texture" not in m and tuple(m["opacity"]) == (0.5, 0.5, 0.5) and not desc.textures
    assert any("opacity" in w and "default" in w for w in info["warnings"])


PATTERN = np.array([[1, 0, 0, 1], [0, 0, 1, 0], [1, 1, 0, 0], [0, 1, 1, 1]], f32)  # the cut-out of the GPU tests: row 0 = v in [0, 1/4)


def test_the_pattern_has_no_symmetry():
    for q in (PATTERN.T, PATTERN[::-1], PATTERN[:, ::-1], PATTERN[::-1, ::-1], PATTERN.T[::-1], PATTERN.T[:, ::-1], PATTERN[::-1, ::-1].T):
        assert not np.array_equal(q, PATTERN)


def write_rgba_png(path):
    """4 x 4 RGBA: alpha = PATTERN, red = its transpose, green = its complement, blue = a constant"""
    from PIL import Image
    a = np.zeros((4, 4, 4), np.uint8)
    a[..., 0] = 255 * PATTERN.T
    a[..., 1] = 255 * (1 - PATTERN)
    a[..., 2] = 128
    a[..., 3] = 255 * PATTERN
    Image.fromarray(a, "RGBA").save(path)


def test_channel_selects_one_channel_as_a_monochrome_texture(tmp_path):
    write_rgba_png(str(tmp_path / "t.png"))
    tex = '<texture name="opacity" type="bitmap"> <string name="filename" value="t.png"/> <string name="channel" value="%s"/> </texture>'
    want = dict(a=PATTERN, r=PATTERN.T, g=1 - PATTERN)
    for ch in "arg":
        desc, m, _ = _load(tmp_path, '<bsdf type="mask"> %s <bsdf type="diffuse"/> </bsdf>' % (tex % ch))
        rgb = desc.textures[m["opacity_texture"]]["rgb"]
        assert rgb.dtype == f32 and np.array_equal(rgb, np.repeat(want[ch][:, :, None], 3, 2)), ch  # 0 and 255 decode to 0 and 1 under any gamma
    desc, m, _ = _load(tmp_path, '<bsdf type="mask"> %s <bsdf type="diffuse"/> </bsdf>' % (tex % "b"))
    blue = desc.textures[m["opacity_texture"]]["rgb"]
    assert np.all(blue == ppg_host.scenes.srgb8_table()[128])  # a colour channel goes through the file's sRGB curve ...
    # ... alpha never does (bitmap.cpp:258-263): 128 / 255
    from PIL import Image
    a = np.full((2, 2, 4), 128, np.uint8)
    Image.fromarray(a, "RGBA").save(str(tmp_path / "t.png"))
    desc, m, _ = _load(tmp_path, '<bsdf type="mask"> %s <bsdf type="diffuse"/> </bsdf>' % (tex % "a"))
    assert np.all(desc.textures[m["opacity_texture"]]["rgb"] == f32(128) / f32(255))
    # a channel the file lacks
    Image.fromarray(a[..., :3].copy(), "RGB").save(str(tmp_path / "t.png"))
    with pytest.raises(mitsuba_xml.SceneError) as ei:
        _load(tmp_path, '<bsdf type="mask"> %s <bsdf type="diffuse"/> </bsdf>' % (tex % "a"))
    assert "no channel 'a'" in str(ei.value) and "r, g, b" in str(ei.value)


# ---------------------------------------------------------------------------------------------- container
def test_a_scene_with_slots_round_trips_through_the_container(tmp_path):
    desc = slots_box(textured=True)
    path = str(tmp_path / "a.ppgs")
    ppg_host.save_scene(desc, path)
    back = ppg_host.load_scene_file(path)
    keys = ("texture", "bump", "specular_texture", "alpha_texture", "opacity_texture")
    assert [{k: m.get(k) for k in keys} for m in back.materials] == [{k: m.get(k) for k in keys} for m in desc.materials]
    assert any(m.get("opacity_texture") is not None for m in back.materials) and any(m.get("alpha_texture") is not None for m in back.materials)
    again = str(tmp_path / "b.ppgs")
    ppg_host.save_scene(back, again)
    assert open(again, "rb").read() == open(path, "rb").read()
    # the C++ driver echoes a scene with `--ppgs` (load, then save): the block survives it
    exe = os.path.join(PKG, "bin", "ppg_render")
    echoed = str(tmp_path / "c.ppgs")
    r = subprocess.run([exe, "-q", "--ppgs", echoed, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert open(echoed, "rb").read() == open(path, "rb").read()
    # a truncated block is refused by both readers
    open(str(tmp_path / "d.ppgs"), "wb").write(open(path, "rb").read()[:-8])
    with pytest.raises(ValueError):
        ppg_host.load_scene_file(str(tmp_path / "d.ppgs"))
    r = subprocess.run([exe, "-q", "--ppgs", echoed, str(tmp_path / "d.ppgs")], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0


def test_a_scene_without_slots_serialises_as_before(tmp_path):
    golden = os.path.join(GOLDEN, "cbox_16x12_pinhole.ppgs")
    desc = ppg_host.load_scene_file(golden)
    assert not ppg_host.bindings.has_parameter_textures(desc)
    out = str(tmp_path / "resaved.ppgs")
    ppg_host.save_scene(desc, out)
    assert open(out, "rb").read() == open(golden, "rb").read()
    plain = slots_box(textured=False)  # textures on no new slot: header bit 9 stays clear
    ppg_host.save_scene(plain, out)
    blocks = np.frombuffer(open(out, "rb").read()[4:28], np.uint32)[5]
    assert not (blocks & 512)


# ---------------------------------------------------------------------------------------------- ABI
def test_material_textures_layout(tmp_path):
    from ppg_host import bindings as b
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppg.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(ppg_material_textures), '
                   'offsetof(ppg_material_textures, specular), offsetof(ppg_material_textures, alpha), offsetof(ppg_material_textures, opacity), '
                   'offsetof(ppg_material_textures, _reserved), sizeof(ppg_material)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    T = b.MaterialTextures
    assert got == [C.sizeof(T), T.specular.offset, T.alpha.offset, T.opacity.offset, T._reserved.offset, C.sizeof(b.Material)]
    assert got == [16, 0, 4, 8, 12, 80] and ppg_host.scenes.C_MATERIAL_TEXTURES_BYTES == 16


def test_the_oracle_refuses_a_scene_with_slots_by_name(oracle_lib):
    e = ppg_host.Engine(oracle_lib, "ppgo_", budgetType="spp", budget=4)
    with pytest.raises(NotImplementedError, match="opacity_texture"):
        e.set_scene(slots_box(textured=True))


# ---------------------------------------------------------------------------------------------- scenes shared with the GPU tests
def const_texture(rgb, w=2, h=2, **kw):
    return dict(dict(rgb=np.broadcast_to(np.asarray(rgb, f32), (h, w, 3)).copy(), nearest=True), **kw)


def rtrans_slice(distribution, alpha, eta):
    g = np.load(os.path.join(GOLDEN, "rtrans_slices.npz"))
    for i, (d, a, e) in enumerate(g["cases"]):
        if (str(d), float(a), float(e)) == (distribution, alpha, eta):
            return g["slice%d" % i]
    raise KeyError((distribution, alpha, eta))


CU_ETA, CU_K = (0.2, 0.92, 1.1), (3.9, 2.45, 2.14)  # copper-like
# Per material: the BSDF, then per textured-capable field (material key of the slot) the values of the quads A and B.  Roughness values are
# ones for which (c + c + c) / 3 == c in float32.
SLOT_FIELD = dict(texture="reflectance", specular_texture="specular", alpha_texture="alpha", opacity_texture="opacity")
MATERIALS = [
    ("conductor", dict(type=3, eta=CU_ETA, k=CU_K), dict(texture=((0.9, 0.8, 0.7), (0.5, 0.7, 0.9)))),
    ("roughconductor", dict(type=4, eta=CU_ETA, k=CU_K), dict(texture=((0.8, 0.9, 0.7), (0.9, 0.6, 0.5)), alpha_texture=(0.25, 0.125))),
    ("plastic", dict(type=5, eta=1.49), dict(texture=((0.6, 0.3, 0.1), (0.1, 0.3, 0.6)), specular_texture=((0.9, 0.8, 1.0), (0.5, 1.0, 0.7)))),
    ("roughplastic", dict(type=9, eta=1.49, alpha=0.2, distribution="beckmann", rtrans=0),
     dict(texture=((0.2, 0.5, 0.7), (0.7, 0.5, 0.2)), specular_texture=((0.8, 0.9, 1.0), (1.0, 0.6, 0.8)))),
    ("dielectric", dict(type=6, eta=1.5), dict(texture=((0.9, 1.0, 0.8), (1.0, 0.7, 0.9)), specular_texture=((0.7, 0.9, 1.0), (1.0, 0.9, 0.6)))),
    ("thindielectric", dict(type=7, eta=1.5), dict(texture=((1.0, 0.9, 0.8), (0.8, 0.9, 1.0)), specular_texture=((0.9, 0.7, 0.8), (0.6, 0.8, 0.9)))),
    ("roughdielectric", dict(type=8, eta=1.5, distribution="beckmann"),
     dict(texture=((0.9, 0.9, 0.8), (0.8, 1.0, 0.9)), specular_texture=((0.8, 0.9, 0.9), (0.9, 0.8, 1.0)), alpha_texture=(0.125, 0.25))),
    ("mask-diffuse", dict(type=0), dict(texture=((0.7, 0.6, 0.5), (0.4, 0.6, 0.8)), opacity_texture=((0.25, 0.5, 0.75), (0.75, 0.25, 0.5)))),
    ("mask-twosided-roughconductor", dict(type=4, eta=CU_ETA, k=CU_K, twosided=True),
     dict(texture=((0.9, 0.7, 0.8), (0.7, 0.9, 0.8)), alpha_texture=(0.25, 0.125), opacity_texture=((0.5, 0.75, 0.25), (0.25, 0.5, 0.75)))),
]


def _value(v):
    return (v, v, v) if np.isscalar(v) else tuple(v)


def _field(key, v):
    return float(v) if key == "alpha_texture" else tuple(float(f32(x)) for x in v)


def slots_box(textured, mode="constant", texcoords=False, width=48, height=40):
    """A closed 2 x 2 x 2 box (diffuse walls) with an area emitter under the ceiling, two masked quads one above the other below the emitter —
    shadow rays and BSDF-sampled rays from below cross both — and, for each of the other materials, a quad A and a quad B standing in the box.
    mode "constant"  one material per BSDF, the values of A on every textured-capable field: as constants (textured=False) or as 2 x 2
                     all-equal nearest textures on every slot (textured=True)
         "shared"    one material per BSDF, each slot a 2 x 1 nearest texture (A, B); needs texcoords: quad A's lie in u < 1/2, quad B's in u > 1/2
         "own"       a material per quad, each slot a texture that reads that quad's value at those texture coordinates and has the AVERAGE of
                     the shared one (2 x 2: the quad's value in row 0, the other one in row 1; every v lies in row 0) — the plug-ins' sampling
                     weights come from the averages, so the two scenes only agree when those agree
    """
    quads = []  # (vertices, material name, emitter, A or B)

    def wall(v, name="wall", em=-1, which="A"):
        quads.append((v, name, em, which))
    wall([(-1, -1, -1), (-1, -1, 1), (1, -1, 1), (1, -1, -1)])    # floor (y = -1), facing up
    wall([(-1, 1, -1), (1, 1, -1), (1, 1, 1), (-1, 1, 1)])        # ceiling
    wall([(-1, -1, 1), (-1, 1, 1), (1, 1, 1), (1, -1, 1)])        # back (z = 1)
    wall([(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1)])    # front (behind the camera)
    wall([(-1, -1, -1), (-1, 1, -1), (-1, 1, 1), (-1, -1, 1)])    # left
    wall([(1, -1, -1), (1, -1, 1), (1, 1, 1), (1, 1, -1)])        # right
    wall([(-0.3, 0.98, -0.3), (0.3, 0.98, -0.3), (0.3, 0.98, 0.3), (-0.3, 0.98, 0.3)], "light", 0)
    # the two masks below the emitter, A and B halves side by side
    for name, y in (("mask-diffuse", 0.6), ("mask-twosided-roughconductor", 0.3)):
        wall([(-0.6, y, -0.5), (-0.6, y, 0.5), (0.0, y, 0.5), (0.0, y, -0.5)], name, -1, "A")
        wall([(0.0, y, -0.5), (0.0, y, 0.5), (0.6, y, 0.5), (0.6, y, -0.5)], name, -1, "B")
    # the others: tilted quads standing on the floor in a row, A in front of B
    others = [m[0] for m in MATERIALS if not m[0].startswith("mask")]
    for i, name in enumerate(others):
        x0 = -0.95 + i * (1.9 / len(others))
        x1 = x0 + 1.9 / len(others) - 0.04
        for which, z in (("A", 0.1), ("B", 0.7)):
            wall([(x0, -0.95, z), (x1, -0.95, z), (x1, -0.35, z + 0.25), (x0, -0.35, z + 0.25)], name, -1, which)
    textures, materials, names = [], [dict(type=0, reflectance=(0.7, 0.7, 0.7)), dict(type=0, reflectance=(0.0, 0.0, 0.0))], ["wall", "light"]

    def add_texture(t):
        textures.append(t)
        return len(textures) - 1
    for name, base, slots in MATERIALS:
        for which in ("A", "B") if mode == "own" else ("A",):
            m = dict(base)
            for key, (a, b) in slots.items():
                a, b = _value(a), _value(b)
                mine, other = (a, b) if which == "A" else (b, a)
                if mode == "constant":
                    m[SLOT_FIELD[key]] = _field(key, a[0] if key == "alpha_texture" else a)
                    if textured:
                        m[key] = add_texture(const_texture(a))
                else:
                    avg = tuple((f32(x) + f32(y)) / f32(2) for x, y in zip(a, b))  # Texture::getAverage of either texture
                    m[SLOT_FIELD[key]] = _field(key, (avg[0] + avg[1] + avg[2]) / f32(3) if key == "alpha_texture" else avg)
                    if mode == "shared":
                        m[key] = add_texture(dict(rgb=np.array([[a, b]], f32), nearest=True))
                    else:
                        m[key] = add_texture(dict(rgb=np.array([[mine, mine], [other, other]], f32), nearest=True))
            if name.startswith("mask") and "opacity" not in m:
                m["opacity"] = (0.5, 0.5, 0.5)
            materials.append(m)
            names.append(name + (which if mode == "own" else ""))
    cam = ppg_host.perspective_camera((0.0, 0.1, -0.98), (0.0, -0.15, 0.0), (0, 1, 0), 75.0, "x", 1e-2, 100.0, width, height)
    pos, idx, tmat, tem, uvs = [], [], [], [], []
    for verts, name, em, which in quads:
        base = len(pos)
        pos.extend(verts)
        idx.extend([(base, base + 1, base + 2), (base, base + 2, base + 3)])
        key = name + which if (mode == "own" and name not in ("wall", "light")) else name
        tmat.extend([names.index(key)] * 2)
        tem.extend([em] * 2)
        u0 = 0.05 if which == "A" else 0.55  # the quad's corners inside ONE texel of a 2-wide texture, and inside row 0 of a 2-high one
        uvs.extend([(u0, 0.05), (u0 + 0.4, 0.05), (u0 + 0.4, 0.45), (u0, 0.45)])
    desc = ppg_host.SceneDesc(np.array(pos, f32), np.array(idx, np.uint32), np.array(tmat, np.uint32), np.array(tem, np.int32), materials,
                              [dict(radiance=(30.0, 28.0, 24.0))], cam, rtrans=rtrans_slice("beckmann", 0.2, 1.49)[None, :].astype(f32),
                              texcoords=np.array(uvs, f32) if texcoords else None, textures=textures)
    return desc
