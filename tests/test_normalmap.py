"""Mitsuba's normalmap and null BSDFs and the scale texture — the parts that need no GPU (include/ppg.h PPG_MAT_NORMALMAP, PPG_BSDF_NULL):

  * the float64 restatement of the shading frame (tests/normalmap_ref.py) against itself in float32: the figure the GPU test's tolerance
    is 4 x of, and the share of rays it leaves out;
  * the Python loader: every acceptance and every refusal of the three plug-ins, by its message; the folded texels of `scale`;
  * the round trips through the flat scene file and the XML writer;
  * the bindings' refusals;
  * ppg_set_scene's refusals through the host build stage (tests/normalmap_build_check.hip, csrc/ppg_scene_build.h, no device).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ppg_host
from ppg_host import imageio, mitsuba_xml
from ppg_host.bindings import Material
from conftest import ROOT

import normalmap_ref as R

f32 = np.float32
SceneError = mitsuba_xml.SceneError


# ------------------------------------------------------------------------------------------------ 1. the restatement and its figure
@pytest.mark.parametrize("key", ["normal_map", "bump"])
def test_the_float32_restatement_stays_within_its_figure_of_the_float64_one(key):
    """FRAME_FIGURE is this test's own measurement (printed); 4 x it is what tests/test_normalmap_gpu.py allows the hook.  The rays left
    out — near a triangle edge, a texel border under `nearest`, a cell border of the bump map's gradient — stay below 1 % per case."""
    worst = 0.0
    for case in R.CASES:
        desc, rays = R.scene(case, key), R.rays(case)
        a, b = R.frames(desc, rays, np.float32), R.frames(desc, rays, np.float64)
        hits = int(b["hit"].sum())
        excluded = 1.0 - b["keep"].sum() / hits
        dev = R.deviation(a, b)
        print(key, case, "rays that hit", hits, "left out", excluded, "float32 against float64", dev)
        assert hits > 0.7 * R.N_RAYS and excluded <= R.MAX_EXCLUDED
        assert set(np.unique(b["tri"][b["hit"]])) == set(range(6))  # every triangle of the three quads
        for w in ("ps", "pt", "pn"):
            assert np.isfinite(b[w][b["hit"]]).all() and np.allclose(np.linalg.norm(b[w][b["keep"]], axis=1), 1.0, atol=1e-12)
        assert np.abs(np.einsum("ij,ij->i", b["ps"], b["pn"])[b["keep"]]).max() < 1e-12
        worst = max(worst, dev)
    print(key, "largest", worst, "figure", R.FRAME_FIGURE[key], "allowance", R.ALLOWANCE * R.FRAME_FIGURE[key])
    assert 0.5 * R.FRAME_FIGURE[key] <= worst <= R.FRAME_FIGURE[key]  # the constant IS the measurement, rounded up


def test_the_normal_map_of_the_frame_tests():
    """4 x 3 unit normals tilted up to 60 degrees, one below the horizon, and no lookup of the tests decodes to (nearly) the zero vector,
    where Mitsuba's frame is NaN"""
    n = 2.0 * R.normal_texels().astype(np.float64) - 1.0
    assert n.shape == (3, 4, 3) and np.allclose(np.linalg.norm(n, axis=2), 1.0, atol=1e-6)
    assert (n[..., 2] < 0).sum() == 1 and np.degrees(np.arccos(n[..., 2][n[..., 2] > 0])).max() <= 60.0
    for case in R.CASES:
        desc = R.scene(case)
        fr = R.frames(desc, R.rays(case), np.float64)
        rgb, _ = R.tex_eval(np.asarray(desc.textures[0]["rgb"]), desc.textures[0], fr["uv"][:, 0], fr["uv"][:, 1], np.float64)
        assert np.linalg.norm(2.0 * rgb[fr["hit"]] - 1.0, axis=1).min() > 0.3
    # without `vt` the quad's uv is the barycentrics and the tangent its first edge
    desc = R.scene("bilinear-repeat")
    fr = R.frames(desc, R.rays("bilinear-repeat"), np.float64)
    mid = fr["hit"] & ((fr["tri"] == 2) | (fr["tri"] == 3))
    assert mid.any() and np.all(fr["uv"][mid] >= 0) and np.all(fr["uv"][mid].sum(1) <= 1)


def test_the_flip_is_the_bump_maps_alone():
    """bumpmap.cpp:157-158 turns a normal that points against the geometric one; normalmap.cpp does not: with the texel below the horizon
    the restated normal-mapped frame keeps n . geoN < 0 on some rays"""
    desc = R.scene("nearest-repeat")
    fr = R.frames(desc, R.rays("nearest-repeat"), np.float64)
    flat = fr["keep"] & (fr["tri"] < 4)  # the quads with their face normal (0, 0, 1)
    assert (fr["pn"][flat][:, 2] < 0).any()
    bump = R.frames(R.scene("bilinear-repeat", "bump"), R.rays("bilinear-repeat"), np.float64)
    assert np.all(bump["pn"][bump["keep"] & (bump["tri"] < 4)][:, 2] > 0)


def test_depth_count_of_null_surfaces():
    assert [R.seen_through(k, 2) for k in range(4)] == [True, True, False, False]
    assert [R.seen_through(k, 3) for k in range(4)] == [True, True, True, False]
    assert all(R.seen_through(k, -1) for k in range(6))


# ------------------------------------------------------------------------------------------------ 2. the loader
XML = """<?xml version="1.0"?>
<scene version="0.5.0">
  <integrator type="guided_path"> <string name="budgetType" value="spp"/> <float name="budget" value="4"/> </integrator>
  <sensor type="perspective">
    <float name="fov" value="45"/>
    <transform name="toWorld"> <lookAt origin="0, 0, -5" target="0, 0, 0" up="0, 1, 0"/> </transform>
    <film type="hdrfilm"> <integer name="width" value="16"/> <integer name="height" value="12"/> <rfilter type="box"/> </film>
  </sensor>
  <texture type="bitmap" id="named"> <string name="filename" value="t.pfm"/> <float name="gamma" value="1"/> </texture>
  <texture type="scale" id="named-scale"> <float name="scale" value="0.5"/> <ref id="named"/> </texture>
  <texture type="checkerboard" id="checks"/>
  %s
  <shape type="rectangle"> <bsdf type="diffuse"/> <emitter type="area"> <rgb name="radiance" value="1"/> </emitter> </shape>
</scene>
"""
TEXELS = np.array([[[0.25, 0.5, 0.75], [0.7, 0.5, 0.3]], [[0.125, 0.3, 0.5], [0.375, 0.2, 0.6]]], f32)
QUAD_OBJ = "v -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nf 1/1 2/2 3/3 4/4\n"
OBJ_SHAPE = '<shape type="obj"> <string name="filename" value="quad.obj"/> %s </shape>'
BITMAP = '<texture type="bitmap"> <string name="filename" value="t.pfm"/> <float name="gamma" value="1.0"/> %s </texture>'
DIFFUSE = '<bsdf type="diffuse"> <rgb name="reflectance" value="0.25, 0.5, 0.75"/> </bsdf>'


def _load(tmp_path, shapes, strict=True):
    imageio.write_pfm(str(tmp_path / "t.pfm"), TEXELS)
    (tmp_path / "quad.obj").write_text(QUAD_OBJ)
    p = tmp_path / "s.xml"
    p.write_text(XML % shapes)
    desc, _, info = ppg_host.load_scene(str(p), strict=strict)
    return desc, desc.materials[int(desc.tri_material[0])], info


def _on_quad(tmp_path, bsdf, strict=True):
    return _load(tmp_path, OBJ_SHAPE % bsdf, strict)


def _normalmap(inner=DIFFUSE, texture=BITMAP % ""):
    return '<bsdf type="normalmap"> %s %s </bsdf>' % (texture, inner)


def test_normalmap_is_read_where_bumpmap_stands(tmp_path):
    desc, m, info = _on_quad(tmp_path, _normalmap())
    assert m["type"] == 0 and m["normal_map"] == 0 and "bump" not in m and not info["warnings"]
    assert np.array_equal(desc.textures[0]["rgb"], TEXELS) and desc.texcoords is not None
    M = Material.from_dict(m)
    assert M.flags == 32 and M.texture == 1 << 16
    # around mask(twosided(x)), by <ref>, and with a reflectance bitmap beside it
    masked = '<bsdf type="mask"> <rgb name="opacity" value="0.4"/> <bsdf type="twosided"> <bsdf type="conductor"> <string name="material" value="none"/> </bsdf> </bsdf> </bsdf>'
    _, m, _ = _on_quad(tmp_path, _normalmap(masked, '<ref id="named"/>'))
    M = Material.from_dict(m)
    assert M.type == 2 and M.flags == (32 | 4 | 1) and M.texture == 1 << 16 and m["opacity"] == pytest.approx((0.4, 0.4, 0.4))
    textured = '<bsdf type="diffuse"> <ref name="reflectance" id="named"/> </bsdf>'
    _, m, _ = _on_quad(tmp_path, _normalmap(textured, BITMAP % '<string name="filterType" value="nearest"/>'))
    assert m["texture"] != m["normal_map"] and {m["texture"], m["normal_map"]} == {0, 1}
    # around a coat and around a blend
    coat = '<bsdf type="coating"> <float name="intIOR" value="1.5"/> %s </bsdf>' % DIFFUSE
    _, m, _ = _on_quad(tmp_path, _normalmap(coat))
    assert m["normal_map"] == 0 and m["coating"]["kind"] == "coating"
    blend = '<bsdf type="blendbsdf"> <float name="weight" value="0.3"/> %s %s </bsdf>' % (DIFFUSE, DIFFUSE)
    _, m, _ = _on_quad(tmp_path, _normalmap(blend))
    assert m["normal_map"] == 0 and m["blend"]["kind"] == "blendbsdf"


NORMALMAP_REFUSALS = [
    ("no-gamma", _normalmap(texture='<texture type="bitmap"> <string name="filename" value="t.pfm"/> </texture>'),
     "When using a bitmap texture as a normal map, please explicitly specify the 'gamma' parameter of the bitmap plugin"),
    ("normalmap-normalmap", _normalmap(_normalmap()), "normalmap(normalmap(...)) is not supported"),
    ("normalmap-bumpmap", _normalmap('<bsdf type="bumpmap"> %s %s </bsdf>' % (BITMAP % "", DIFFUSE)), "normalmap(bumpmap(...)) is not supported"),
    ("bumpmap-normalmap", '<bsdf type="bumpmap"> %s %s </bsdf>' % (BITMAP % "", _normalmap()), "bumpmap(normalmap(...)) is not supported"),
    ("no-bsdf", '<bsdf type="normalmap"> %s </bsdf>' % (BITMAP % ""), "normalmap: A child BSDF instance is required"),
    ("two-bsdfs", '<bsdf type="normalmap"> %s %s %s </bsdf>' % (BITMAP % "", DIFFUSE, DIFFUSE), "normalmap: Only a single nested BSDF can be added!"),
    ("no-texture", '<bsdf type="normalmap"> %s </bsdf>' % DIFFUSE, "normalmap: A normal map texture must be specified"),
    ("two-textures", '<bsdf type="normalmap"> %s %s %s </bsdf>' % (BITMAP % "", BITMAP % "", DIFFUSE), "normalmap: Only a single normal texture can be specified!"),
    ("procedural", _normalmap(texture='<ref id="checks"/>'), "texture type 'checkerboard' on normalmap is not supported (bitmap only)"),
    ("blend-child", '<bsdf type="blendbsdf"> <float name="weight" value="0.3"/> %s %s </bsdf>' % (DIFFUSE, _normalmap()),
     "blendbsdf(normalmap) is not supported: the nesting order is bumpmap(mask(twosided(blendbsdf(..))))"),
    ("inside-a-coat", '<bsdf type="coating"> %s </bsdf>' % _normalmap(), "coating(normalmap) is not supported: the nesting order is bumpmap(mask(twosided(coating(..))))"),
    ("inside-a-roughcoating", '<bsdf type="roughcoating"> %s </bsdf>' % _normalmap(),
     "roughcoating(normalmap) is not supported: the nesting order is bumpmap(mask(twosided(coating(..))))"),
    ("normalmap-null", _normalmap('<bsdf type="null"/>'), "normalmap(null) is not supported"),
]


@pytest.mark.parametrize("k", range(len(NORMALMAP_REFUSALS)), ids=[r[0] for r in NORMALMAP_REFUSALS])
def test_normalmap_refusals(tmp_path, k):
    _, bsdf, says = NORMALMAP_REFUSALS[k]
    with pytest.raises(SceneError) as err:
        _on_quad(tmp_path, bsdf)
    assert says in str(err.value), str(err.value)


def test_a_lenient_load_drops_a_normal_map_it_cannot_read(tmp_path):
    for bsdf in (NORMALMAP_REFUSALS[0][1], NORMALMAP_REFUSALS[1][1], NORMALMAP_REFUSALS[8][1]):
        _, m, info = _on_quad(tmp_path, bsdf, strict=False)
        assert m["type"] == 0 and tuple(m["reflectance"]) == (0.25, 0.5, 0.75)
        assert any("dropped around its nested bsdf" in w for w in info["warnings"]), info["warnings"]
    _, m, info = _on_quad(tmp_path, NORMALMAP_REFUSALS[6][1], strict=False)  # (no texture at all: the adapter goes)
    assert m["type"] == 0 and "normal_map" not in m and any("dropped around its nested bsdf" in w for w in info["warnings"])


@pytest.mark.parametrize("shape", ["disk", "cylinder"])
def test_a_normal_map_on_a_disk_or_cylinder_is_refused(tmp_path, shape):
    """(on a sphere the refusal is ppg_set_scene's: tests/normalmap_build_check.hip)"""
    with pytest.raises(SceneError) as err:
        _load(tmp_path, OBJ_SHAPE % DIFFUSE + '<shape type="%s"> <float name="radius" value="0.5"/> %s </shape>' % (shape, _normalmap()))
    assert "%s: textured BSDFs are only supported on triangle meshes (not on spheres, disks or cylinders)" % shape in str(err.value)


def test_null_is_read(tmp_path):
    desc, m, info = _on_quad(tmp_path, '<bsdf type="null"/>')
    assert m == dict(type=13) and not info["warnings"]
    assert Material.from_dict(m).type == 13 == Material.BSDF["null"] and Material.from_dict(m).flags == 0
    # its usual use: the invisible carrier of an area emitter
    desc, m, _ = _on_quad(tmp_path, '<bsdf type="null"/> <emitter type="area"> <rgb name="radiance" value="3, 2, 1"/> </emitter>')
    assert m["type"] == 13 and int(desc.tri_emitter[0]) >= 0
    assert tuple(desc.emitters[int(desc.tri_emitter[0])]["radiance"]) == (3.0, 2.0, 1.0)


NULL = '<bsdf type="null"/>'
NULL_REFUSALS = [
    ("twosided", '<bsdf type="twosided"> %s </bsdf>' % NULL, "twosided(null): only BRDFs can be two-sided (twosided.cpp:84-88)"),
    ("mask", '<bsdf type="mask"> %s </bsdf>' % NULL, "mask(null) is not supported"),
    ("bumpmap", '<bsdf type="bumpmap"> %s %s </bsdf>' % (BITMAP % "", NULL), "bumpmap(null) is not supported"),
    ("coating", '<bsdf type="coating"> %s </bsdf>' % NULL, "coating(null): a coat on the null BSDF is not supported"),
    ("roughcoating", '<bsdf type="roughcoating"> %s </bsdf>' % NULL, "roughcoating(null): a coat on the null BSDF is not supported"),
    ("blend-child", '<bsdf type="blendbsdf"> <float name="weight" value="0.3"/> %s %s </bsdf>' % (DIFFUSE, NULL), "blendbsdf(null): a null child is not supported"),
    ("mixture-child", '<bsdf type="mixturebsdf"> <string name="weights" value="0.3, 0.4"/> %s %s </bsdf>' % (NULL, DIFFUSE), "mixturebsdf(null): a null child is not supported"),
]


@pytest.mark.parametrize("k", range(len(NULL_REFUSALS)), ids=[r[0] for r in NULL_REFUSALS])
def test_null_refusals(tmp_path, k):
    _, bsdf, says = NULL_REFUSALS[k]
    with pytest.raises(SceneError) as err:
        _on_quad(tmp_path, bsdf)
    assert says in str(err.value), str(err.value)


@pytest.mark.parametrize("shape", ["sphere", "disk", "cylinder"])
def test_null_on_an_analytic_shape_is_refused(tmp_path, shape):
    with pytest.raises(SceneError) as err:
        _load(tmp_path, OBJ_SHAPE % DIFFUSE + '<shape type="%s"> <float name="radius" value="0.5"/> %s </shape>' % (shape, NULL))
    assert "%s: the null BSDF is only supported on triangle meshes (not on spheres, disks or cylinders)" % shape in str(err.value)


def test_the_unsupported_list_still_begins_as_it_did_and_names_the_new_plugins(tmp_path):
    with pytest.raises(SceneError) as err:
        _on_quad(tmp_path, '<bsdf type="ward"/>')
    text = str(err.value)
    assert "is not supported yet (diffuse, roughdiffuse, difftrans, phong," in text
    assert " null," in text and "normalmap(...)" in text and "bumpmap(...)" in text


def test_the_cpp_loader_reads_null_and_keeps_refusing_normalmap(tmp_path):
    """host/scene_xml.h: the same record as the Python loader's for <bsdf type="null"/>; twosided(null) and mask(null) refused; normalmap (it
    reads no bitmaps) refused strictly and dropped leniently, as before"""
    from test_microfacet_general import MESH_VT, _cpp, _material_records, _scene
    body = MESH_VT % NULL
    r, flat = _cpp(tmp_path, body)
    assert r.returncode == 0, r.stderr
    desc, _, _ = ppg_host.load_scene(_scene(tmp_path, body))
    assert _material_records(flat) == b"".join(bytes(Material.from_dict(m)) for m in desc.materials)
    assert any(m["type"] == 13 for m in desc.materials)
    for bsdf, says in (('<bsdf type="twosided"> %s </bsdf>' % NULL, "twosided(null): only BRDFs can be two-sided (twosided.cpp:84-88)"),
                       ('<bsdf type="mask"> %s </bsdf>' % NULL, "mask(null) is not supported")):
        r, _ = _cpp(tmp_path, MESH_VT % bsdf)
        assert r.returncode != 0 and says in r.stderr, r.stderr
    imageio.write_pfm(str(tmp_path / "t.pfm"), TEXELS)
    r, _ = _cpp(tmp_path, MESH_VT % _normalmap())
    assert r.returncode != 0 and "bsdf type 'normalmap' is not supported yet (diffuse, roughdiffuse, difftrans, phong," in r.stderr and " null," in r.stderr
    r, flat = _cpp(tmp_path, MESH_VT % _normalmap(), "--lenient")
    assert r.returncode == 0 and flat is not None, r.stderr


# ------------------------------------------------------------------------------------------------ 3. the scale texture
def _scale(factor, nested=BITMAP % "", name=None):
    return '<texture type="scale"%s> %s %s </texture>' % ("" if name is None else ' name="%s"' % name, factor, nested)


HALF = '<float name="scale" value="0.3"/>'


def test_scale_folds_the_factor_into_the_texels_in_float32(tmp_path):
    desc, m, info = _on_quad(tmp_path, '<bsdf type="diffuse"> %s </bsdf>' % _scale(HALF, name="reflectance"))
    assert not info["warnings"]
    t = desc.textures[m["texture"]]
    want = TEXELS * f32(0.3)
    assert t["rgb"].dtype == np.float32 and np.array_equal(t["rgb"].view(np.uint32), want.view(np.uint32))
    # the record's average scales with it
    assert np.allclose(m["reflectance"], TEXELS.reshape(-1, 3).mean(0, dtype=np.float64) * 0.3, rtol=1e-6)
    assert np.allclose(t["average"], want.reshape(-1, 3).mean(0, dtype=np.float64), rtol=0, atol=0)
    # the lookup's parameters are the bitmap's
    nested = BITMAP % '<string name="wrapMode" value="clamp"/> <float name="uscale" value="2"/> <string name="filterType" value="nearest"/>'
    desc, m, _ = _on_quad(tmp_path, '<bsdf type="diffuse"> %s </bsdf>' % _scale(HALF, nested, "reflectance"))
    t = desc.textures[m["texture"]]
    assert (t["wrap_u"], t["wrap_v"], t["nearest"], tuple(t["uv_scale"])) == ("clamp", "clamp", True, (2.0, 1.0))


def test_scale_of_scale_folds_both_factors_and_a_spectrum_folds_per_channel(tmp_path):
    inner = _scale('<float name="scale" value="0.7"/>')
    desc, m, _ = _on_quad(tmp_path, '<bsdf type="diffuse"> %s </bsdf>' % _scale(HALF, inner, "reflectance"))
    want = (TEXELS * f32(0.7)) * f32(0.3)  # the inner one first
    assert np.array_equal(desc.textures[m["texture"]]["rgb"].view(np.uint32), want.view(np.uint32))
    desc, m, _ = _on_quad(tmp_path, '<bsdf type="diffuse"> %s </bsdf>' % _scale('<rgb name="scale" value="0.5, 0.25, 1.5"/>', name="reflectance"))
    want = TEXELS * np.array([0.5, 0.25, 1.5], f32)
    assert np.array_equal(desc.textures[m["texture"]]["rgb"].view(np.uint32), want.view(np.uint32))
    desc, m, _ = _on_quad(tmp_path, '<bsdf type="diffuse"> %s </bsdf>' % _scale('<spectrum name="scale" value="0.4"/>', name="reflectance"))
    assert np.array_equal(desc.textures[m["texture"]]["rgb"].view(np.uint32), (TEXELS * f32(0.4)).view(np.uint32))


def test_scale_is_accepted_wherever_a_bitmap_is(tmp_path):
    # by <ref>, to a scale that itself refers to a bitmap
    desc, m, _ = _on_quad(tmp_path, '<bsdf type="diffuse"> <ref name="reflectance" id="named-scale"/> </bsdf>')
    assert np.array_equal(desc.textures[m["texture"]]["rgb"], TEXELS * f32(0.5))
    # on a specular colour, a roughness, an opacity
    desc, m, _ = _on_quad(tmp_path, '<bsdf type="plastic"> %s </bsdf>' % _scale(HALF, name="specularReflectance"))
    assert np.array_equal(desc.textures[m["specular_texture"]]["rgb"], TEXELS * f32(0.3))
    desc, m, _ = _on_quad(tmp_path, '<bsdf type="roughconductor"> <string name="material" value="none"/> %s </bsdf>' % _scale(HALF, name="alpha"))
    assert np.array_equal(desc.textures[m["alpha_texture"]]["rgb"], TEXELS * f32(0.3))
    desc, m, _ = _on_quad(tmp_path, '<bsdf type="mask"> %s %s </bsdf>' % (_scale(HALF, name="opacity"), DIFFUSE))
    assert np.array_equal(desc.textures[m["opacity_texture"]]["rgb"], TEXELS * f32(0.3))
    # around a bump map, whose gradient scales with it: the documented use
    desc, m, _ = _on_quad(tmp_path, '<bsdf type="bumpmap"> %s %s </bsdf>' % (_scale('<float name="scale" value="4"/>'), DIFFUSE))
    bump = desc.textures[m["bump"]]
    assert np.array_equal(bump["rgb"], TEXELS * f32(4.0))
    plain = dict(bump, rgb=TEXELS)
    u, v = np.array([0.4, 0.55]), np.array([0.45, 0.6])
    g4, g1 = R.tex_gradient_lum(bump["rgb"], bump, u, v, np.float64), R.tex_gradient_lum(TEXELS, plain, u, v, np.float64)
    assert np.all(g1[0] != 0) and np.allclose(g4[0], 4 * g1[0], rtol=1e-6) and np.allclose(g4[1], 4 * g1[1], rtol=1e-6)
    # inside a normalmap: simply folded
    desc, m, _ = _on_quad(tmp_path, _normalmap(texture=_scale(HALF)))
    assert np.array_equal(desc.textures[m["normal_map"]]["rgb"], TEXELS * f32(0.3))
    # two uses of one scaled texture share it
    both = OBJ_SHAPE % ('<bsdf type="diffuse"> %s </bsdf>' % _scale(HALF, name="reflectance")) + OBJ_SHAPE % _normalmap(texture=_scale(HALF))
    desc, _, _ = _load(tmp_path, both)
    assert len(desc.textures) == 2  # the bitmap and its scaled copy


SCALE_REFUSALS = [
    ("zero", _scale('<float name="scale" value="0"/>', name="reflectance"), "scale: the scale factor must be finite and > 0"),
    ("negative", _scale('<float name="scale" value="-2"/>', name="reflectance"), "scale: the scale factor must be finite and > 0"),
    ("infinite", _scale('<float name="scale" value="inf"/>', name="reflectance"), "scale: the scale factor must be finite and > 0"),
    ("nan", _scale('<float name="scale" value="nan"/>', name="reflectance"), "scale: the scale factor must be finite and > 0"),
    ("a-black-channel", _scale('<rgb name="scale" value="0.5, 0, 0.5"/>', name="reflectance"), "scale: the scale factor must be finite and > 0"),
    ("no-nested", _scale(HALF, "", "reflectance"), "scale: The scale plugin needs a nested texture!"),
    ("two-nested", _scale(HALF, BITMAP % "" + BITMAP % "", "reflectance"), "scale: exactly one nested texture is required (found 2)"),
    ("procedural", _scale(HALF, '<texture type="checkerboard"/>', "reflectance"), "scale: texture type 'checkerboard' inside a scale texture is not supported"),
    ("procedural-by-ref", _scale(HALF, '<ref id="checks"/>', "reflectance"), "scale: texture type 'checkerboard' inside a scale texture is not supported"),
    ("constant-value", _scale(HALF + '<rgb name="value" value="0.5"/>', "", "reflectance"), "scale: a constant 'value' inside a scale texture is not supported"),
    ("wrap-one", _scale(HALF, BITMAP % '<string name="wrapMode" value="one"/>', "reflectance"),
     "scale around a bitmap with wrap mode 'one' is not supported: the constant outside the image would not scale"),
    ("wrap-one-v", _scale(HALF, BITMAP % '<string name="wrapModeV" value="one"/>', "reflectance"),
     "scale around a bitmap with wrap mode 'one' is not supported: the constant outside the image would not scale"),
]


@pytest.mark.parametrize("k", range(len(SCALE_REFUSALS)), ids=[r[0] for r in SCALE_REFUSALS])
def test_scale_refusals(tmp_path, k):
    _, texture, says = SCALE_REFUSALS[k]
    with pytest.raises(SceneError) as err:
        _on_quad(tmp_path, '<bsdf type="diffuse"> %s </bsdf>' % texture)
    assert says in str(err.value), str(err.value)


def test_a_procedural_texture_stays_refused_by_its_old_message(tmp_path):
    with pytest.raises(SceneError, match="texture type 'checkerboard' on reflectance is not supported \\(bitmap only\\)"):
        _on_quad(tmp_path, '<bsdf type="diffuse"> <ref name="reflectance" id="checks"/> </bsdf>')


# ------------------------------------------------------------------------------------------------ 4. round trips
def _records(desc):
    return [bytes(Material.from_dict(m)) for m in ppg_host.bindings.expand_blends(desc.materials)]


def test_flat_scene_file_carries_the_flag_and_the_type(tmp_path):
    desc = R.scene("nearest-clamp")
    desc.materials = list(desc.materials) + [dict(type="null"), dict(type=0, reflectance=(0.5, 0.5, 0.5), bump=0), dict(type=4, normal_map=0, texture=0, twosided=True)]
    p = str(tmp_path / "s.ppgs")
    ppg_host.save_scene(desc, p)
    back = ppg_host.load_scene_file(p)
    assert _records(back) == _records(desc)
    assert back.materials[0]["normal_map"] == 0 and "bump" not in back.materials[0]
    assert back.materials[6]["type"] == 13
    assert back.materials[7]["bump"] == 0 and "normal_map" not in back.materials[7]
    assert back.materials[8]["normal_map"] == 0 and back.materials[8]["texture"] == 0
    assert np.array_equal(back.textures[0]["rgb"], desc.textures[0]["rgb"])


def test_xml_writer_round_trip(tmp_path):
    """the writer emits <bsdf type="null"/> and <bsdf type="normalmap"> around everything else, the map as a float image — a `scale` the
    loader folded stays folded —; the loader reads the same records back"""
    scaled = _scale('<float name="scale" value="0.9"/>', BITMAP % '<string name="wrapModeU" value="clamp"/> <float name="voffset" value="0.25"/> <string name="filterType" value="nearest"/>')
    masked = '<bsdf type="mask"> <rgb name="opacity" value="0.4"/> <bsdf type="twosided"> %s </bsdf> </bsdf>' % DIFFUSE
    shapes = OBJ_SHAPE % _normalmap(masked, scaled) + OBJ_SHAPE % (NULL + '<emitter type="area"> <rgb name="radiance" value="3, 2, 1"/> </emitter>') \
        + OBJ_SHAPE % _normalmap('<bsdf type="plastic"/>')
    desc, _, _ = _load(tmp_path, shapes)
    out = tmp_path / "written"
    path = mitsuba_xml.save_scene_xml(desc, dict(budgetType="spp", budget=4), str(out))
    text = open(path).read()
    assert '<bsdf type="null"' in text and text.count('<bsdf type="normalmap"') == 2 and 'type="scale"' not in text
    back, _, info = ppg_host.load_scene(path)
    used = lambda d: sorted(set(bytes(Material.from_dict(d.materials[int(i)])) for i in d.tri_material))  # noqa: E731
    a = {int(i): desc.materials[int(i)] for i in desc.tri_material}
    b = {int(i): back.materials[int(i)] for i in back.tri_material}

    def record(d, m):  # the record without the texture's position in the list, and the texture it names
        M = Material.from_dict(m)
        t = d.textures[m["normal_map"]] if m.get("normal_map") is not None else None
        key = None if t is None else (t["rgb"].tobytes(), t["wrap_u"], t["wrap_v"], bool(t["nearest"]), tuple(t["uv_scale"]), tuple(t["uv_offset"]))
        M.texture = 1 << 16 if t is not None else 0
        return bytes(M), key
    assert sorted(record(desc, m) for m in a.values()) == sorted(record(back, m) for m in b.values())
    assert len(used(back)) == 4 and any(m.get("type") == 13 for m in b.values())
    scaled_map = [t for t in back.textures if t["nearest"]][0]
    assert np.array_equal(scaled_map["rgb"].view(np.uint32), (TEXELS * f32(0.9)).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 5. the bindings
def test_bindings_refuse_bump_and_normal_map_together():
    with pytest.raises(ValueError) as err:
        Material.from_dict(dict(type=0, bump=0, normal_map=1))
    assert "bump" in str(err.value) and "normal_map" in str(err.value)
    M = Material.from_dict(dict(type="diffuse", normal_map=2, texture=0))
    assert M.flags == 32 and M.texture == (3 << 16 | 1)
    assert Material.from_dict(dict(type="null")).type == 13 and Material.from_dict(dict(type=13)).type == 13
    assert Material.from_dict(dict(type=0, bump=2)).flags == 0


def test_the_oracle_refuses_both(oracle_lib):
    from conftest import make_oracle
    e = make_oracle(oracle_lib, threads=1, budgetType="spp", budget=4)
    for last in (dict(type="null"), dict(type=0, normal_map=0)):
        desc = ppg_host.cbox_scene(8, 6)
        desc.materials = list(desc.materials) + [last]
        desc.textures = [dict(rgb=TEXELS)]
        with pytest.raises(NotImplementedError, match="normalmap adapter and the null BSDF"):
            e.set_scene(desc)
    with pytest.raises(NotImplementedError):
        e.debug_shading_frame(np.zeros((1, 8), f32))


# ------------------------------------------------------------------------------------------------ 6. ppg_set_scene's refusals, on the host
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_ppg_set_scene_refusals_through_the_host_build_stage(tmp_path):
    """tests/normalmap_build_check.hip: buildScene() without a context or a device, its host code under the address and undefined-behaviour
    sanitizers, as a child process"""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail("hipcc not found (set HIPCC)")
    exe = str(tmp_path / "normalmap_build_check")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "normalmap_build_check.hip")])
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)
    print(run.stdout)
    print(run.stderr)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "all checks passed" in run.stdout and "FAILED" not in run.stdout
    assert run.stdout.count("ok refused") == 21 and run.stdout.count("ok accepted") == 10
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
