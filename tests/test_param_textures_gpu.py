"""Bitmaps on specular colours, roughness and mask opacity on the GPU (include/ppg.h ppg_set_material_textures).  The CPU oracle does not know
these slots, so the pins reduce the new code to what the oracle already pins — a constant texture renders what the constant renders, a shared
texture what per-quad textures render — and to closed forms: a specular colour seen in a mirror, cut-outs seen directly and as shadows."""
import os
import subprocess

import numpy as np
import pytest

import ppg_host
from conftest import IMPROVED, PKG
from test_param_textures import OBJ_SHAPE, PATTERN, QUAD_OBJ, XML, slots_box, write_rgba_png
from test_rfilter_gpu import _tree_equal

f32 = np.float32
pytestmark = pytest.mark.gpu
W, H = 48, 40

# 31 samples per pixel = iterations of 1, 2, 4, 8 and 16 passes.  The IMPROVED preset combines the last four iterations by inverse variance,
# and the variance estimate of an iteration of ONE sample per pixel divides by N - 1 = 0 (GP:1303-1311): a budget of 16 or less — four
# iterations — renders NaN on the GPU and in the oracle alike.  31 is the smallest budget of this preset that gives a picture.
CONFIGS = {
    "nee-always-depth-6": dict(IMPROVED, budgetType="spp", budget=31, nee="always", maxDepth=6, rrDepth=5, seed=11),
    "kickstart-unbounded": dict(IMPROVED, budgetType="spp", budget=31, nee="kickstart", maxDepth=-1, rrDepth=4, seed=12),
}


def hip(**props):
    return ppg_host.Engine.hip(**props)


def _render(desc, **props):
    e = hip(**props)
    e.set_scene(desc)
    e.render()
    out = e.read_film(), e.read_variance(), e.read_sdtree()
    e.close()
    return out


def _same(a, b):
    assert np.isfinite(a[0]).all() and a[0].mean() > 1e-3
    assert np.array_equal(a[0], b[0]), "film: %d pixels differ, max %g" % ((a[0] != b[0]).any(2).sum(), np.abs(a[0] - b[0]).max())
    assert np.array_equal(a[1], b[1])
    _tree_equal(a[2], b[2])


# ---------------------------------------------------------------------------------------------- 1, 2: reductions
@pytest.mark.parametrize("config", list(CONFIGS))
def test_a_constant_texture_is_the_constant(config):
    """Every textured-capable parameter of nine BSDFs as a constant, and as a 2 x 2 all-equal nearest texture on every slot (no texture
    coordinates: uv = the barycentrics, the frame that of an untextured hit).  All three lookup sites, bin 13 against the common kernel,
    k_tail (unbounded depth) and the sampling weights from the record's averages."""
    plain, textured = slots_box(False), slots_box(True)
    assert not ppg_host.bindings.has_parameter_textures(plain) and ppg_host.bindings.has_parameter_textures(textured)
    _same(_render(textured, **CONFIGS[config]), _render(plain, **CONFIGS[config]))


def test_the_right_texel_at_the_right_place():
    """With texture coordinates: quads A and B of a material inside the two texels of one shared 2 x 1 texture per slot, against a material per
    quad whose textures hold that quad's value where its texture coordinates lie (and have the shared texture's average).  Two masked quads
    below the emitter: shadow rays and BSDF-sampled rays cross both."""
    shared, own = slots_box(True, "shared", texcoords=True), slots_box(True, "own", texcoords=True)
    assert len(own.materials) == 2 * len(shared.materials) - 2
    a, b = _render(shared, **CONFIGS["nee-always-depth-6"]), _render(own, **CONFIGS["nee-always-depth-6"])
    _same(a, b)
    swapped = slots_box(True, "shared", texcoords=True)  # (the test can fail: A and B exchanged in every shared texture)
    for t in swapped.textures:
        t["rgb"] = np.ascontiguousarray(t["rgb"][:, ::-1])
    c = _render(swapped, **CONFIGS["nee-always-depth-6"])
    assert not np.array_equal(c[0], a[0])


# ---------------------------------------------------------------------------------------------- 3, 4: closed forms
def _camera():
    return ppg_host.perspective_camera((0, 0, 1), (0, 0, 0), (0, 1, 0), 90.0, "x", 1e-2, 100.0, W, H)


def _view_uv(cam, p):
    """texture coordinates that map the view's footprint on the plane z = 0 to [0, 1]^2: (u, v) = the film position that sees (p.x, p.y, 0)"""
    c2w = np.asarray(cam["camera_to_world"], np.float64)
    q = c2w[:3, :3].T @ (np.array([p[0], p[1], 0.0]) - c2w[:3, 3])
    tan_x = 1.0  # fov 90 degrees across the width
    tan_y = tan_x * H / W
    return 0.5 * (1 - q[0] / q[2] / tan_x), 0.5 * (1 - q[1] / q[2] / tan_y)


def _plane_scene(quads, materials, textures, environment=None, delta=None):
    """quads: (z, material index); each spans [-2, 2]^2 at height z, facing +z, with the texture coordinates of the floor point below it"""
    cam = _camera()
    pos, idx, tmat, uvs = [], [], [], []
    for z, mat in quads:
        base = len(pos)
        verts = [(-2, -2, z), (2, -2, z), (2, 2, z), (-2, 2, z)]
        pos.extend(verts)
        uvs.extend(_view_uv(cam, v) for v in verts)
        idx.extend([(base, base + 1, base + 2), (base, base + 2, base + 3)])
        tmat.extend([mat] * 2)
    return ppg_host.SceneDesc(np.array(pos, f32), np.array(idx, np.uint32), np.array(tmat, np.uint32), np.full(len(tmat), -1, np.int32), materials, [], cam,
                              environment=environment, texcoords=np.array(uvs, f32), textures=textures, delta_emitters=delta or [])


def _interior(edges_x, edges_y):
    """pixels farther than one pixel from a texel edge (edges in pixels)"""
    keep = np.ones((H, W), bool)
    for e in edges_x:
        keep[:, [e - 1, e]] = False
    for e in edges_y:
        keep[[e - 1, e], :] = False
    return keep


BASE_INTERIOR = _interior((12, 24, 36), (10, 20, 30))
LE = np.array([2.0, 1.5, 0.75], f32)
SIMPLE = dict(budgetType="spp", budget=7, sppPerPass=1, seed=3)


def _upsample(tex, tx, ty):
    return tex[ty[:, None], tx[None, :]]


def _close(img, want, keep, left_out=0.3):
    assert 1 - keep.mean() <= left_out + 1e-9  # at most 30 % of the pixels are left out (the mirror's uv-transformed variant: see there)
    err = np.abs(img - want)[keep]
    assert np.all(err <= 1e-5 * np.abs(want)[keep]), "max relative error %g" % (err / np.maximum(np.abs(want)[keep], 1e-30)).max()


@pytest.mark.parametrize("variant", ["plain", "uv-transform"])
def test_specular_colour_seen_in_a_mirror(variant):
    """straight down on a mirror (conductor, material none) whose specularReflectance is a 4 x 4 nearest texture of 16 colours, under a constant
    environment: every pixel is L * its texel (all samples of a pixel are identical)"""
    rng = np.random.RandomState(5)
    colours = (0.2 + 0.75 * rng.rand(4, 4, 3)).astype(f32)
    assert len({tuple(c) for c in colours.reshape(-1, 3)}) == 16
    tex = dict(rgb=colours, nearest=True)
    px, py = np.arange(W), np.arange(H)
    if variant == "plain":
        tx, ty = px * 4 // W, py * 4 // H
        keep = BASE_INTERIOR
        assert abs((1 - keep.mean()) - 0.256) < 1e-3
    else:  # the same uv transform as every texture: u * 2 mirrored, v + 1/4 clamped
        tex.update(uv_scale=(2.0, 1.0), uv_offset=(0.0, 0.25), wrap_u="mirror", wrap_v="clamp")
        tx = px * 8 // W
        tx = np.where(tx >= 4, 7 - tx, tx)
        ty = np.minimum(py * 4 // H + 1, 3)
        # Texel edges every 6 columns but for the mirror's fold, rows as before but for the clamped last one: "farther than one pixel from an
        # edge" leaves out 12 columns and 4 rows = 32.5 %.  The 30 % allowed cannot be met here: under uscale = 2 a row of 48 pixels has six
        # real edges, 25 % in the columns alone.  The exclusion rule is kept and the share it gives is asserted instead.
        keep = _interior((6, 12, 18, 30, 36, 42), (10, 20))
        assert abs((1 - keep.mean()) - 0.325) < 1e-3
    desc = _plane_scene([(0.0, 0)], [dict(type=2, reflectance=tuple(float(v) for v in colours.reshape(-1, 3).mean(0)), texture=0)], [tex],
                        environment=tuple(float(v) for v in LE))
    img = _render(desc, maxDepth=2, nee="never", **SIMPLE)[0]
    want = _upsample(colours, tx, ty) * LE
    _close(img, want, keep, left_out=0.3 if variant == "plain" else 0.325)


def _cutout_direct(pattern_tex):
    mats = [dict(type=0, reflectance=(0.0, 0.0, 0.0), opacity=tuple(float(v) for v in pattern_tex["rgb"].reshape(-1, 3).mean(0)), opacity_texture=0)]
    return _plane_scene([(0.0, 0)], mats, [pattern_tex], environment=tuple(float(v) for v in LE))


def _pattern_texture(p):
    return dict(rgb=np.repeat(np.asarray(p, f32)[:, :, None], 3, 2).copy(), nearest=True)


def test_cutout_seen_directly():
    """a masked black diffuse quad fills the view in front of a constant environment: opaque texels are 0, open ones L, exactly.
    (bsdfSamplingFraction = 1: a mask is a smooth / null hybrid, so once the SD-tree is built the integrator picks its BSDF with that
    probability and weights the pass-through by its inverse, GP:1672-1676 — with 0.5 a pixel is a mean of 0 and 2 L, right only on average.)"""
    img = _render(_cutout_direct(_pattern_texture(PATTERN)), maxDepth=4, nee="never", bsdfSamplingFraction=1.0, **SIMPLE)[0]
    opaque = _upsample(PATTERN, np.arange(W) * 4 // W, np.arange(H) * 4 // H) > 0
    assert BASE_INTERIOR.mean() >= 0.7
    assert np.all(img[BASE_INTERIOR & opaque] == 0)
    assert np.array_equal(img[BASE_INTERIOR & ~opaque], np.broadcast_to(LE, img.shape)[BASE_INTERIOR & ~opaque])


RHO, IRRADIANCE = np.array([0.6, 0.5, 0.4], f32), np.array([3.0, 2.5, 2.0], f32)


def _cutout_shadow(pattern):
    """a diffuse floor seen from above, a directional emitter travelling along -z, the cut-out ABOVE THE CAMERA between light and floor"""
    t = _pattern_texture(pattern)
    mats = [dict(type=0, reflectance=tuple(float(v) for v in RHO)),
            dict(type=0, reflectance=(0.0, 0.0, 0.0), opacity=tuple(float(v) for v in t["rgb"].reshape(-1, 3).mean(0)), opacity_texture=0)]
    light = dict(type="directional", intensity=tuple(float(v) for v in IRRADIANCE), direction=(0.0, 0.0, -1.0))
    return _plane_scene([(0.0, 0), (2.0, 1)], mats, [t], delta=[light])


# maxDepth = 3, not 2: a shadow segment may pass maxDepth - depth - 1 null surfaces (GP:1966, Scene::evalTransmittance's maxInteractions), which
# at the first hit of a maxDepth = 2 render is none — every cut-out then shadows like a solid sheet, as in the reference.  The third vertex adds
# nothing: the cut-out's own BSDF is black, and nothing can be hit beyond it.
SHADOW_PROPS = dict(maxDepth=3, nee="always", **SIMPLE)


def test_cutout_as_a_shadow_and_its_orientation():
    """shadow rays through the cut-out (shadow_transmittance): a floor pixel is rho / pi * irradiance under an open texel, 0 under an opaque one.
    The transposed pattern gives another picture: a lookup with u and v exchanged cannot pass."""
    img = _render(_cutout_shadow(PATTERN), **SHADOW_PROPS)[0]
    opaque = _upsample(PATTERN, np.arange(W) * 4 // W, np.arange(H) * 4 // H)[..., None]
    want = (1 - opaque) * (RHO * f32(1 / np.pi) * IRRADIANCE)
    assert np.all(img[BASE_INTERIOR & (opaque[..., 0] > 0)] == 0)
    _close(img, want, BASE_INTERIOR)
    other = _render(_cutout_shadow(PATTERN.T), **SHADOW_PROPS)[0]
    assert not np.array_equal(other, img)
    want_t = (1 - _upsample(PATTERN.T, np.arange(W) * 4 // W, np.arange(H) * 4 // H)[..., None]) * (RHO * f32(1 / np.pi) * IRRADIANCE)
    _close(other, want_t, BASE_INTERIOR)


# ---------------------------------------------------------------------------------------------- 5: channel
def test_opacity_from_the_alpha_channel_of_a_png(tmp_path):
    """<texture type="bitmap" channel="a"> of an RGBA PNG on a mask's opacity, through the XML loader: the picture of the same scene with the
    pattern as a float image; channel "r" (the transposed pattern) gives another one"""
    from ppg_host import imageio
    write_rgba_png(str(tmp_path / "cut.png"))
    imageio.write_pfm(str(tmp_path / "cut.pfm"), np.repeat(PATTERN[:, :, None], 3, 2))
    shape = """<emitter type="constant"> <rgb name="radiance" value="2, 1.5, 0.75"/> </emitter>
      """ + OBJ_SHAPE % ('<transform name="toWorld"> <scale value="2.2"/> </transform>', """<bsdf type="mask">
          <texture name="opacity" type="bitmap"> <string name="filename" value="%s"/> <string name="filterType" value="nearest"/> %s </texture>
          <bsdf type="diffuse"> <rgb name="reflectance" value="0"/> </bsdf> </bsdf>""")
    (tmp_path / "quad.obj").write_text(QUAD_OBJ)
    films = {}
    for name, fn, extra in (("a", "cut.png", '<string name="channel" value="a"/>'), ("float", "cut.pfm", ""), ("r", "cut.png", '<string name="channel" value="r"/>')):
        p = tmp_path / (name + ".xml")
        p.write_text(XML.replace('<shape type="rectangle"> <bsdf type="diffuse"/> <emitter type="area"> <rgb name="radiance" value="1"/> </emitter> </shape>', "") % (shape % (fn, extra)))
        desc, _, _ = ppg_host.load_scene(str(p), width=W, height=H)
        assert desc.materials[int(desc.tri_material[0])]["opacity_texture"] is not None
        films[name] = _render(desc, maxDepth=4, nee="never", **SIMPLE)[0]
    assert np.array_equal(films["a"], films["float"])
    assert set(np.unique(films["a"].reshape(-1, 3), axis=0)[:, 0]) >= {0.0, 2.0}  # both kinds of texel are in the picture
    assert not np.array_equal(films["r"], films["a"])


# ---------------------------------------------------------------------------------------------- 6: validation
def test_invalid_slots_are_refused_by_name():
    from ppg_host.bindings import MaterialTextures, PPGError
    desc = slots_box(True)
    names = ["wall", "light"] + [m[0] for m in __import__("test_param_textures").MATERIALS]
    n = len(desc.materials)
    e = hip(budgetType="spp", budget=3, sppPerPass=1, maxDepth=4)

    def set_scene_keeping_the_list(eng, d):  # Engine.set_scene always sends the description's own list first: here the hand-made one stays
        send, eng.set_material_textures = eng.set_material_textures, lambda slots: None
        try:
            eng.set_scene(d)
        finally:
            eng.set_material_textures = send

    def slots(**per_material):
        out = [MaterialTextures() for _ in range(n)]
        for name, kw in per_material.items():
            for k, v in kw.items():
                setattr(out[names.index(name.replace("_", "-"))], k, v)
        return out
    nt = len(desc.textures)
    cases = [
        (slots()[:-1], "entries"),                                        # a list of another length
        (slots(plastic=dict(specular=nt + 1)), "material %d: texture slot specular: index" % names.index("plastic")),
        (slots(conductor=dict(specular=1)), "material %d: texture slot specular" % names.index("conductor")),   # a type that does not read it
        (slots(plastic=dict(alpha=1)), "material %d: texture slot alpha" % names.index("plastic")),
        (slots(dielectric=dict(opacity=1)), "material %d: texture slot opacity" % names.index("dielectric")),   # no PPG_MAT_MASK
        (slots(roughplastic=dict(alpha=1)), "slot alpha: roughplastic"),
        (slots(wall=dict(_reserved=7)), "material 0: texture slot _reserved"),
    ]
    for lst, msg in cases:
        e.set_material_textures(lst)
        with pytest.raises(PPGError) as ex:
            set_scene_keeping_the_list(e, desc)
        assert ex.value.code == -1 and msg in str(ex.value), (msg, str(ex.value))
    # a textured material on an analytic sphere
    ball = slots_box(True)
    del ball.materials[names.index("plastic")]["texture"]  # (only the new slot: the old one has its own refusal)
    ball.spheres = [dict(center=(0.0, 0.0, 0.0), radius=0.1, material=names.index("plastic"), emitter=-1)]
    with pytest.raises(PPGError) as ex:
        e.set_scene(ball)
    assert ex.value.code == -1 and "sphere" in str(ex.value) and "material %d" % names.index("plastic") in str(ex.value)
    # after a refused ppg_set_scene: clear the list, set a scene without slots, render
    e.set_material_textures([])
    plain = slots_box(False)
    set_scene_keeping_the_list(e, plain)
    e.render()
    assert np.array_equal(e.read_film(), _render(plain, budgetType="spp", budget=3, sppPerPass=1, maxDepth=4)[0])
    e.begin_render()
    with pytest.raises(PPGError, match="ppg_begin_render") as ex:  # not while a render is open
        e.set_material_textures([])
    assert ex.value.code == -3
    e.end_render()
    e.close()


# ---------------------------------------------------------------------------------------------- 7: no slots, no change
def test_without_slots_the_call_changes_nothing():
    """a FULL scene with a reflectance texture and a bump map: the call never made, made with an all-zero list, and a list of a previous scene
    cleared again"""
    from ppg_host.bindings import MaterialTextures
    rng = np.random.RandomState(2)
    desc = ppg_host.cbox_scene(W, H)
    desc.textures = [dict(rgb=(0.2 + 0.7 * rng.rand(8, 8, 3)).astype(f32)), dict(rgb=np.repeat(rng.rand(8, 8, 1), 3, 2).astype(f32))]
    desc.materials[1].update(reflectance=tuple(float(v) for v in desc.textures[0]["rgb"].reshape(-1, 3).mean(0)), texture=0)
    desc.materials[0].update(bump=1)
    desc.materials[2] = dict(type=4, reflectance=(0.9, 0.8, 0.7), eta=(0.2, 0.9, 1.1), k=(3.9, 2.4, 2.1), alpha=0.2)
    props = dict(CONFIGS["kickstart-unbounded"])
    n = hip(**props)  # ppg_set_material_textures never called on this context
    n.set_material_textures = lambda slots: None
    n.set_scene(desc)
    n.render()
    never = n.read_film(), n.read_variance(), n.read_sdtree()
    n.close()
    e = hip(**props)
    e.set_material_textures([MaterialTextures() for _ in desc.materials])
    e.set_material_textures = lambda slots: None  # (set_scene would replace the all-zero list by the empty one)
    e.set_scene(desc)
    e.render()
    _same((e.read_film(), e.read_variance(), e.read_sdtree()), never)
    e.close()
    g = hip(**props)
    g.set_scene(slots_box(True))     # a previous scene's list ...
    g.set_scene(desc)                # ... cleared by the description without slots
    g.render()
    _same((g.read_film(), g.read_variance(), g.read_sdtree()), never)
    g.close()


# ---------------------------------------------------------------------------------------------- 8: hosts agree
HOST_XML = """<?xml version="1.0"?>
<scene version="0.5.0">
  <integrator type="guided_path"> <string name="budgetType" value="spp"/> <float name="budget" value="15"/> <integer name="sppPerPass" value="1"/>
    <integer name="maxDepth" value="4"/> <string name="nee" value="always"/> <integer name="sTreeThreshold" value="4000"/> </integrator>
  <sensor type="perspective"> <float name="fov" value="90"/> <string name="fovAxis" value="x"/>
    <transform name="toWorld"> <lookAt origin="0, 0, 1" target="0, 0, 0" up="0, 1, 0"/> </transform>
    <film type="hdrfilm"> <integer name="width" value="48"/> <integer name="height" value="40"/> <rfilter type="box"/> </film> </sensor>
  <emitter type="directional"> <vector name="direction" x="0" y="0" z="-1"/> <rgb name="irradiance" value="3, 2.5, 2"/> </emitter>
  <shape type="rectangle"> <transform name="toWorld"> <scale value="2"/> </transform> <bsdf type="diffuse"> <rgb name="reflectance" value="0.6, 0.5, 0.4"/> </bsdf> </shape>
  <shape type="obj"> <string name="filename" value="quad.obj"/> <transform name="toWorld"> <scale value="2"/> <translate z="2"/> </transform>
    <bsdf type="mask"> <texture name="opacity" type="bitmap"> <string name="filename" value="cut.pfm"/> <string name="filterType" value="nearest"/> </texture>
      <bsdf type="diffuse"> <rgb name="reflectance" value="0"/> </bsdf> </bsdf> </shape>
  <shape type="obj"> <string name="filename" value="quad.obj"/>
    <transform name="toWorld"> <scale value="0.5"/> <rotate x="1" angle="-35"/> <translate x="0.2" y="0.1" z="0.3"/> </transform>
    <bsdf type="roughconductor"> <string name="material" value="none"/> <string name="distribution" value="ggx"/>
      <texture name="alpha" type="bitmap"> <string name="filename" value="rough.pfm"/> <string name="filterType" value="nearest"/> </texture> </bsdf> </shape>
</scene>
"""


def test_hosts_agree(tmp_path):
    """the cut-out shadow plus a roughness-mapped roughconductor, converted with `python -m ppg_host ... --ppgs`: bin/ppg_render (one rank, and
    through its reducer with --rank 0 --world 1) and Engine.hip give the same film; two ranks sharing the GPU give it too.  (Two ppg_render
    processes cannot share one device — RCCL refuses a communicator with two ranks on the same GPU — so the two ranks are the two processes
    of tests/test_two_ranks_one_gpu.py, with this scene file.)"""
    import sys
    from ppg_host import imageio
    from test_cpp_host import read_pfm
    from test_two_ranks_one_gpu import _launch
    imageio.write_pfm(str(tmp_path / "cut.pfm"), np.repeat(PATTERN[:, :, None], 3, 2))
    rough = np.repeat(np.array([[0.05, 0.4], [0.3, 0.1]], f32)[:, :, None], 3, 2)
    imageio.write_pfm(str(tmp_path / "rough.pfm"), rough)
    (tmp_path / "quad.obj").write_text(QUAD_OBJ)
    (tmp_path / "scene.xml").write_text(HOST_XML)
    path = str(tmp_path / "scene.ppgs")
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "ppg_host", str(tmp_path / "scene.xml"), "--ppgs", path], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    desc = ppg_host.load_scene_file(path)
    assert sorted(k for m in desc.materials for k in m if k.endswith("_texture")) == ["alpha_texture", "opacity_texture"]
    props = dict(budgetType="spp", budget=15.0, sppPerPass=1, maxDepth=4, nee="always", sTreeThreshold=4000)
    want = ppg_host.GuidedPathTracer(engine=hip(**props)).render(desc)
    assert np.isfinite(want).all() and want.mean() > 1e-3
    exe = os.path.join(PKG, "bin", "ppg_render")
    for extra in ([], ["--rank", "0", "--world", "1", "--nccl-id", str(tmp_path / "id"), "--run-tag", "t"]):
        out = str(tmp_path / "out.pfm")
        r = subprocess.run([exe, "-q", "-o", out] + extra + [path], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(read_pfm(out), want)
    ranks = _launch(tmp_path, dict(scene=path, res=[W, H], tile=8, props=props), timeout=240)
    for k in ranks:
        assert np.array_equal(k["film"], want)
