"""Scene-XML subset loader, OBJ reader, colour conversion, image writers (SURVEY.md §8(b) row "Scene XML subset",
§8(f3)/(f4)).  CPU only; the end-to-end CLI run on the GPU is in test_gpu_parity.py."""
import os
import sys

import numpy as np
import pytest

import ppg_host
from ppg_host import mitsuba_xml, spectrum
from ppg_host.imageio import read_exr, write_exr, write_pfm
from ppg_host.scenes import CBOX_EMITTER_RGB, CBOX_RGB

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF_CBOX = os.path.join(GOLDEN, "cbox", "cbox.xml")                 # the reference's scenes/cbox/cbox.xml + meshes/*.obj, as shipped
MITSUBA_DATA = os.path.join(GOLDEN, "mitsuba_data")                  # Mitsuba's data/ior/{Ag,Au,Cu,W}.{eta,k}.spd, as shipped


def test_spectrum_values_reproduce_the_committed_cbox_constants():
    # scenes/cbox/cbox.xml: the "light" reflectance and the emitter's radiance (4 samples each); incl. the reversed
    # interpolation of spectrum.cpp:693-706 that lowers the emitter's R by 11 %
    assert np.allclose(spectrum.parse("spectrum", "400:0.78, 500:0.78, 600:0.78, 700:0.78"), CBOX_RGB["light"], rtol=2e-6)
    em = spectrum.parse("spectrum", "400:0, 500:16, 600:31.2, 700:36.8")
    assert np.allclose(em, CBOX_EMITTER_RGB, rtol=2e-6)
    assert np.array_equal(spectrum.parse("spectrum", "0.5"), np.full(3, 0.5, np.float32))
    assert np.array_equal(spectrum.parse("rgb", "0.1, 0.2, 0.3"), np.array([0.1, 0.2, 0.3], np.float32))
    assert np.allclose(spectrum.parse("rgb", "#ff8000"), [1.0, 128 / 255.0, 0.0])
    assert np.allclose(spectrum.parse("srgb", "0.5, 0.5, 0.5"), 0.21404114, atol=1e-6)
    with pytest.raises(ValueError):
        spectrum.parse("blackbody", "5000")


def test_reference_cbox_xml_equals_the_procedural_restatement():
    desc, props, info = ppg_host.load_scene(REF_CBOX)
    assert props == dict(strictNormals=1, maxDepth=10, rrDepth=10, budgetType="spp", budget=127.0)  # cbox.xml:8-24
    assert (info["width"], info["height"], info["sample_count"]) == (512, 512, 128) and not info["warnings"]
    ref = ppg_host.cbox_scene(512, 512)
    assert desc.n_triangles == 36 and len(desc.emitters) == 1
    key = lambda s: {tuple(np.sort(t.reshape(-1))) for t in np.round(s.positions[s.indices.astype(int)], 2)}  # noqa: E731
    assert key(desc) == key(ref)
    assert np.array_equal(desc.camera["camera_to_world"], ref.camera["camera_to_world"])
    assert np.array_equal(desc.camera["sample_to_camera"], ref.camera["sample_to_camera"])
    got = sorted(tuple(np.float32(v) for v in m["reflectance"]) for m in desc.materials)
    want = sorted({tuple(np.float32(v) for v in m["reflectance"]) for m in ref.materials})
    assert np.allclose(got, want, rtol=2e-6)
    assert np.allclose(desc.emitters[0]["radiance"], CBOX_EMITTER_RGB, rtol=2e-6)
    # vertex normals: present in two OBJs, generated (trimesh.cpp:631-671) for the planar ones — all equal the face normal
    tri = desc.positions[desc.indices.astype(int)]
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]); fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    for k in range(3):
        assert np.abs(np.sum(desc.normals[desc.indices[:, k]] * fn, 1) - 1).max() < 1e-5
    # the emitter is the luminaire, rotated by 180 degrees about x and translated (cbox.xml:66-70): it hangs below the ceiling
    # and faces UP ("edited by us to have an upside-down light source", cbox.xml:3-4) — same winding as the restatement
    lum = desc.positions[desc.indices[desc.tri_emitter >= 0].reshape(-1)]
    assert np.allclose(lum[:, 1], 1020 - 548.79999, atol=1e-3) and fn[desc.tri_emitter >= 0][:, 1].min() > 0.999
    rt = ref.positions[ref.indices.astype(int)]
    rn = np.cross(rt[:, 1] - rt[:, 0], rt[:, 2] - rt[:, 0]); rn /= np.linalg.norm(rn, axis=1, keepdims=True)
    centre = lambda t: tuple(np.round(t.mean(1), 1).reshape(-1))  # noqa: E731
    by_centre = {tuple(np.round(c, 1)): n for c, n in zip(rt.mean(1), rn)}
    for c, n in zip(tri.mean(1), fn):
        assert np.dot(by_centre[tuple(np.round(c, 1))], n) > 0.999


SCENE = """<?xml version="1.0"?>
<scene version="0.5.0">
  <default name="spp" value="12"/>
  <integrator type="guided_path">
    <string name="budgetType" value="spp"/> <float name="budget" value="$spp"/>
    <integer name="sTreeThreshold" value="4000"/> <boolean name="strictNormals" value="true"/>
    <string name="nee" value="$nee"/> <integer name="someVorbaThing" value="3"/>
  </integrator>
  <sensor type="perspective">
    <float name="fov" value="45"/> <string name="fovAxis" value="y"/>
    <transform name="toWorld"> <lookAt origin="0, 1, -5" target="0, 1, 0" up="0, 1, 0"/> </transform>
    <sampler type="independent"> <integer name="sampleCount" value="64"/> </sampler>
    <film type="hdrfilm"> <integer name="width" value="40"/> <integer name="height" value="30"/> <rfilter type="box"/> </film>
  </sensor>
  <bsdf type="diffuse" id="grey"> <rgb name="reflectance" value="0.4, 0.5, 0.6"/> </bsdf>
  <bsdf type="twosided" id="two"> <bsdf type="diffuse"> <spectrum name="reflectance" value="0.25"/> </bsdf> </bsdf>
  <shape type="obj"> <string name="filename" value="meshes/thing.obj"/>
    <transform name="toWorld"> <scale x="2" y="1" z="1"/> <rotate y="1" angle="90"/> <translate x="1" y="2" z="3"/> </transform>
    <ref id="grey"/> </shape>
  <shape type="rectangle">
    <transform name="toWorld"> <scale value="0.5"/> <matrix value="1 0 0 0  0 0 -1 4  0 1 0 0  0 0 0 1"/> </transform>
    <ref id="two"/> <emitter type="area"> <rgb name="radiance" value="10, 9, 8"/> </emitter> </shape>
  <shape type="rectangle"> <bsdf type="conductor"> <string name="material" value="none"/> </bsdf> </shape>
  %s
</scene>
"""
OBJ = """# a quad given as one 4-gon with negative indices (resolved against the vertex count when the mesh is created, like
# obj.cpp:573-578 — hence all vertices first), then a triangle with v/vt/vn corners; one line continued with a backslash
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 0 0 1
v 1 0 1 \\
 
v 0 1 1
vn 0 0 1
vt 0.5 0.5
f -7 -6 -5 -4
f 5/1/1 6/1/1 7/1/1
"""


def _write(tmp_path, extra=""):
    os.makedirs(tmp_path / "meshes", exist_ok=True)
    (tmp_path / "meshes" / "thing.obj").write_text(OBJ)
    p = tmp_path / "s.xml"
    p.write_text(SCENE % extra)
    return str(p)


def test_loader_subset_semantics(tmp_path):
    desc, props, info = ppg_host.load_scene(_write(tmp_path), defines=dict(nee="kickstart"))
    assert props == dict(budgetType="spp", budget=12.0, sTreeThreshold=4000, strictNormals=1, nee="kickstart")  # $spp default, -D nee
    assert any("someVorbaThing" in w for w in info["warnings"])
    assert (info["width"], info["height"]) == (40, 30)
    with pytest.raises(mitsuba_xml.SceneError, match=r"\$nee"):
        ppg_host.load_scene(_write(tmp_path))
    # OBJ: fan triangulation (0,1,2),(0,2,3) of the 4-gon + the extra triangle; then scale → rotate(y, 90) → translate
    assert desc.n_triangles == 3 + 2 + 2
    P = desc.positions[desc.indices[:3].astype(int)]

    def xf(p):  # (x, y, z) → scale x by 2 → rotate 90 deg about y: (z, y, -x) → + (1, 2, 3)
        x, y, z = 2 * p[0], p[1], p[2]
        return np.array([z + 1, y + 2, -x + 3], np.float32)
    quad = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)]
    assert np.allclose(P[0], [xf(np.array(quad[k], float)) for k in (0, 1, 2)], atol=1e-6)
    assert np.allclose(P[1], [xf(np.array(quad[k], float)) for k in (0, 2, 3)], atol=1e-6)
    assert np.allclose(P[2], [xf(np.array(q, float)) for q in ((0, 0, 1), (1, 0, 1), (0, 1, 1))], atol=1e-6)
    # normals: the file's vn (0,0,1) goes through the inverse transpose: scale 2 in x does not tilt it; rotate → (1,0,0).
    # The 4-gon has no normals in the file: this mesh mixes both, so the whole mesh reports normals (zero = "none" in Mitsuba
    # for those corners is NOT reproduced: the loader keeps per-mesh semantics — mesh has normals ⇒ corners without get 0)
    n_tri = desc.normals[desc.indices[2].astype(int)]
    assert np.allclose(n_tri, [[1, 0, 0]] * 3, atol=1e-6)
    # rectangle: [-1,1]^2 scaled by 0.5, then the matrix (y ← -z + 4, z ← y): a quad at y = 4 spanning x,z in [-0.5, 0.5]
    R = desc.positions[desc.indices[3:5].reshape(-1).astype(int)]
    assert np.allclose(R[:, 1], 4) and np.allclose(np.abs(R[:, [0, 2]]), 0.5)
    assert np.allclose(desc.normals[desc.indices[3].astype(int)], [[0, -1, 0]] * 3, atol=1e-6)  # (0,0,1) → (0,-1,0): faces down
    assert list(desc.tri_emitter) == [-1, -1, -1, 0, 0, -1, -1]
    assert desc.emitters == [dict(radiance=(10.0, 9.0, 8.0))]
    mats = [desc.materials[i] for i in desc.tri_material]
    assert mats[0] == dict(type=0, reflectance=tuple(float(np.float32(v)) for v in (0.4, 0.5, 0.6)))
    assert mats[3] == dict(type=1, reflectance=(0.25, 0.25, 0.25)) and mats[5]["type"] == 2 and mats[5]["reflectance"] == (1.0, 1.0, 1.0)
    # camera: fov 45 about y at 4:3, lookAt
    want = ppg_host.perspective_camera((0, 1, -5), (0, 1, 0), (0, 1, 0), 45, "y", 1e-2, 1e4, 40, 30)
    assert np.allclose(desc.camera["camera_to_world"], want["camera_to_world"], atol=1e-6)
    assert np.array_equal(desc.camera["sample_to_camera"], want["sample_to_camera"])


@pytest.mark.parametrize("extra,needle", [
    ('<shape type="cylinder"/>', "cylinder"),
    ('<shape type="rectangle"><bsdf type="ward"/></shape>', "ward"),
    ('<shape type="rectangle"><bsdf type="conductor"><string name="material" value="Au"/></bsdf></shape>', "Au"),
    ('<emitter type="sunsky"/>', "sunsky"),
    ('<shape type="rectangle"><bsdf type="diffuse"><texture name="reflectance" type="checkerboard"/></bsdf></shape>', "checkerboard"),
    ('<shape type="rectangle"><bsdf type="diffuse"><texture name="reflectance" type="bitmap"/></bsdf></shape>', "without filename"),
    ('<shape type="rectangle"><bsdf type="dielectric"><texture name="specularReflectance" type="bitmap"/></bsdf></shape>', "texture on"),
    ('<shape type="obj"><string name="filename" value="meshes/missing.obj"/></shape>', "not found"),
])
def test_unsupported_plugins_are_named(tmp_path, extra, needle):
    with pytest.raises(mitsuba_xml.SceneError, match=needle):
        ppg_host.load_scene(_write(tmp_path, extra), defines=dict(nee="never"))


def test_lenient_mode_and_wrong_integrator(tmp_path):
    p = _write(tmp_path, '<shape type="rectangle"><bsdf type="ward"/></shape>')
    desc, _, info = ppg_host.load_scene(p, defines=dict(nee="never"), strict=False)
    assert any("ward" in w for w in info["warnings"]) and desc.n_triangles == 9
    q = tmp_path / "pt.xml"
    q.write_text(open(p).read().replace('type="guided_path"', 'type="path"'))
    with pytest.raises(mitsuba_xml.SceneError, match="guided_path"):
        ppg_host.load_scene(str(q), defines=dict(nee="never"))


def test_generated_vertex_normals_of_a_cube():
    # shared corner vertices: every corner sees three faces with a total angle of 90 degrees each (two 45-degree triangle
    # corners or one 90-degree one) ⇒ the angle-weighted normal is the normalised diagonal (trimesh.cpp:631-671)
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = np.array([(q[0], q[a], q[a + 1]) for q in quads for a in (1, 2)], np.uint32)
    n = mitsuba_xml.compute_normals(v, tris)
    want = (v * 2 - 1) / np.sqrt(3)
    assert np.abs(np.abs(n) - np.abs(want)).max() < 1e-6 and np.allclose(np.abs(np.sum(n * want, 1)), 1, atol=1e-6)
    assert np.array_equal(mitsuba_xml.compute_normals(v, tris, flip=True), -n)
    # a degenerate triangle contributes nothing; an isolated vertex gets the reference's bogus (1, 0, 0)
    v2 = np.vstack([v, [[5, 5, 5]]]).astype(np.float32)
    t2 = np.vstack([tris, [[0, 0, 1]]]).astype(np.uint32)
    n2 = mitsuba_xml.compute_normals(v2, t2)
    assert np.array_equal(n2[:8], n) and np.array_equal(n2[8], [1, 0, 0])


def test_scene_xml_round_trip(tmp_path):
    for desc in (ppg_host.cbox_scene(64, 48), ppg_host.room_scene(32, 18, n_boxes=3, tess=1)):
        props = dict(budgetType="spp", budget=31.0, maxDepth=10, rrDepth=10, strictNormals=1, nee="kickstart", dTreeThreshold=0.02)
        back, props2, info = ppg_host.load_scene(ppg_host.save_scene_xml(desc, props, str(tmp_path)))
        assert props2 == props and not info["warnings"]
        key = lambda s: sorted(tuple(t.reshape(-1)) + (tuple(float(np.float32(v)) for v in s.materials[m]["reflectance"]), int(e))  # noqa: E731
                               for t, m, e in zip(s.positions[s.indices.astype(int)], s.tri_material, s.tri_emitter))
        assert key(back) == key(desc)
        assert back.normals is None and len(back.emitters) == len(desc.emitters)
        for k in ("camera_to_world", "sample_to_camera"):
            assert np.array_equal(back.camera[k], desc.camera[k])


def test_exr_and_pfm_writers(tmp_path):
    rng = np.random.RandomState(0)
    img = rng.rand(7, 11, 3).astype(np.float32) * 10
    p = str(tmp_path / "a.exr")
    write_exr(p, img, {"log": "line 1\nline 2", "generatedBy": "test"})
    back, attrs = read_exr(p)
    assert np.array_equal(back, img) and attrs["log"] == "line 1\nline 2" and attrs["generatedBy"] == "test"
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import exr_min  # the independent reader used to mine the reference's shipped EXRs
    a2, ch = exr_min.read_exr(p)
    assert np.array_equal(ch["R"], img[..., 0]) and np.array_equal(ch["B"], img[..., 2]) and a2["log"][0] == "string"
    q = str(tmp_path / "a.pfm")
    write_pfm(q, img)
    raw = open(q, "rb").read()
    assert raw.startswith(b"PF\n11 7\n-1.0\n")
    assert np.array_equal(np.frombuffer(raw[len(b"PF\n11 7\n-1.0\n"):], "<f4").reshape(7, 11, 3)[::-1], img)


def test_cli_converts_to_the_flat_scene_of_the_cpp_driver(tmp_path):
    from ppg_host.__main__ import main
    xml = ppg_host.save_scene_xml(ppg_host.cbox_scene(32, 32), dict(budgetType="spp", budget=8.0, maxDepth=5), str(tmp_path))
    out = str(tmp_path / "flat.ppgs")
    assert main([xml, "--ppgs", out, "-q", "-P", "rrDepth=3"]) == 0
    raw = open(out, "rb").read()
    assert raw[:4] == b"PPGS" and np.frombuffer(raw, "<u4", 6, 4).tolist()[1:5] == [36, 4, 1, 0]  # vertices merge per mesh (obj.cpp:600-608)
    assert set(open(out + ".props").read().split()) == {"budgetType=spp", "budget=8.0", "maxDepth=5", "rrDepth=3"}


def test_glossy_plugins_parse_like_their_constructors(tmp_path):
    extra = """
    <shape type="rectangle"><bsdf type="roughconductor"> <string name="material" value="none"/> <string name="distribution" value="ggx"/>
        <float name="alpha" value="0.15"/> </bsdf></shape>
    <shape type="rectangle"><bsdf type="twosided"><bsdf type="roughconductor"> <string name="distribution" value="ggx"/>
        <rgb name="eta" value="0.2, 0.9, 1.1"/> <rgb name="k" value="3.9, 2.4, 2.1"/> <rgb name="specularReflectance" value="0.5, 0.6, 0.7"/>
        </bsdf></bsdf></shape>
    <shape type="rectangle"><bsdf type="plastic"> <rgb name="diffuseReflectance" value="0.1, 0.2, 0.3"/> <boolean name="nonlinear" value="true"/> </bsdf></shape>
    <shape type="rectangle"><bsdf type="dielectric"> <string name="intIOR" value="water"/> <float name="extIOR" value="1.0"/> </bsdf></shape>
    <shape type="rectangle"><bsdf type="conductor"> <float name="extEta" value="2"/> <spectrum name="eta" value="1.0"/> <spectrum name="k" value="3.0"/> </bsdf></shape>
    """
    desc, _, _ = ppg_host.load_scene(_write(tmp_path, extra), defines=dict(nee="never"))
    m = [desc.materials[i] for i in desc.tri_material[7::2]]
    f = lambda *v: tuple(float(np.float32(x)) for x in v)  # noqa: E731
    air = np.float32(1.000277)
    assert m[0] == dict(type=4, reflectance=f(1, 1, 1), eta=f(0, 0, 0), k=tuple(float(np.float32(1) / air) for _ in range(3)), alpha=0.15)
    assert m[1]["twosided"] and m[1]["type"] == 4 and m[1]["alpha"] == 0.1 and m[1]["reflectance"] == f(0.5, 0.6, 0.7)  # alpha default, microfacet.h:99-100
    assert "distribution" not in m[1] and "distribution" not in m[0]                                                     # both ask for ggx
    assert np.allclose(m[1]["eta"], np.float32([0.2, 0.9, 1.1]) / air, rtol=1e-7)  # divided by extEta = air (roughconductor.cpp:183-186)
    assert m[2] == dict(type=5, reflectance=f(0.1, 0.2, 0.3), specular=f(1, 1, 1), eta=float(np.float32(1.49 / 1.000277)), nonlinear=True)  # polypropylene / air
    assert m[3] == dict(type=6, reflectance=f(1, 1, 1), specular=f(1, 1, 1), eta=float(np.float32(1.333)))
    assert m[4] == dict(type=3, reflectance=f(1, 1, 1), eta=f(0.5, 0.5, 0.5), k=f(1.5, 1.5, 1.5))
    for bad, needle in (('<bsdf type="roughconductor"><string name="distribution" value="ggx"/></bsdf>', "data/ior"),
                        ('<bsdf type="roughconductor"><string name="material" value="none"/><string name="distribution" value="phong"/></bsdf>', "phong"),
                        ('<bsdf type="roughconductor"><string name="material" value="none"/><string name="distribution" value="ggx"/>'
                         '<float name="alphaU" value="0.1"/><float name="alphaV" value="0.3"/></bsdf>', "anisotropic"),
                        ('<bsdf type="dielectric"><string name="intIOR" value="unobtainium"/></bsdf>', "unobtainium"),
                        ('<bsdf type="twosided"><bsdf type="dielectric"/></bsdf>', "two-sided"),
                        ('<bsdf type="twosided"><bsdf type="roughdielectric"/></bsdf>', "two-sided"),
                        ('<bsdf type="roughdielectric"><float name="intIOR" value="1.0"/><float name="extIOR" value="1.0"/></bsdf>', "differ")):
        with pytest.raises(mitsuba_xml.SceneError, match=needle):
            ppg_host.load_scene(_write(tmp_path, '<shape type="rectangle">%s</shape>' % bad), defines=dict(nee="never"))


def test_full_material_set_survives_the_xml_round_trip(tmp_path):
    from ppg_host.bindings import Material
    scene = ppg_host.cbox_scene(16, 16)
    scene.materials = list(scene.materials) + [
        dict(type="roughconductor", alpha=0.2, eta=(0.143, 0.375, 1.442), k=(3.983, 2.386, 1.603), reflectance=(1, 1, 1)),
        dict(type="conductor", eta=(0.2, 0.92, 1.1), k=(3.9, 2.45, 2.14), reflectance=(0.95, 0.95, 0.95), twosided=True),
        dict(type="plastic", reflectance=(0.2, 0.35, 0.7), specular=(1, 0.9, 0.8), eta=1.49, nonlinear=True),
        dict(type="dielectric", eta=1.5, reflectance=(1, 1, 1), specular=(0.98, 0.99, 0.98)),
        dict(type="mirror", reflectance=(0.7, 0.8, 0.9)), dict(type=1, reflectance=(0.3, 0.3, 0.3)),
        dict(type="thindielectric", eta=1.33, reflectance=(1, 1, 1), specular=(0.9, 0.9, 1.0)),
        dict(type="diffuse", reflectance=(0.2, 0.3, 0.4), twosided=True, opacity=(0.5, 0.6, 0.7)),
        dict(type="plastic", reflectance=(0.2, 0.3, 0.4), eta=1.4, opacity=(0.25, 0.25, 0.25)),
        dict(type="roughconductor", alpha=0.3, eta=(0.2, 0.9, 1.1), k=(3.9, 2.4, 2.1), reflectance=(1, 1, 1), distribution="beckmann"),
        dict(type="roughdielectric", alpha=0.25, eta=1.5, reflectance=(1, 1, 1), specular=(0.9, 0.95, 1.0)),
        dict(type="roughdielectric", alpha=0.1, eta=1.33, reflectance=(0.9, 0.9, 0.9), specular=(1, 1, 1), distribution="beckmann", opacity=(0.5, 0.5, 0.5))]
    tm = scene.tri_material.copy(); tm[2:26:2] = np.arange(5, 17); scene.tri_material = tm
    back, _, info = ppg_host.load_scene(ppg_host.save_scene_xml(scene, dict(budgetType="spp", budget=8.0), str(tmp_path)))
    assert not info["warnings"]
    per_tri = lambda s: sorted((tuple(np.sort(t.reshape(-1))), bytes(Material.from_dict(s.materials[m])))  # noqa: E731
                               for t, m in zip(s.positions[s.indices.astype(int)], s.tri_material))
    assert per_tri(back) == per_tri(scene)


def test_environment_emitter_in_xml_and_flat_file(tmp_path):
    import struct
    scene = ppg_host.cbox_scene(16, 16)
    scene.environment = (0.25, 0.5, 1.0)
    back, _, _ = ppg_host.load_scene(ppg_host.save_scene_xml(scene, dict(budgetType="spp", budget=8.0), str(tmp_path)))
    assert back.environment == (0.25, 0.5, 1.0)
    p = str(tmp_path / "e.ppgs")
    ppg_host.save_scene(back, p)
    raw = open(p, "rb").read()
    assert struct.unpack_from("<6I", raw, 4)[5] == 1 and struct.unpack_from("<3f", raw, len(raw) - 12) == (0.25, 0.5, 1.0)
    with pytest.raises(mitsuba_xml.SceneError, match="envmap"):
        ppg_host.load_scene(_write(tmp_path, '<emitter type="envmap"/>'), defines=dict(nee="never"))


def test_sphere_shapes_follow_the_reference_constructor(tmp_path):
    """Sphere::Sphere (sphere.cpp:108-131): `center` / `radius`, and a toWorld whose (uniform) scale is moved into the radius while
    rotation and translation stay in the object-to-world transform — the rotation orients the (theta, phi) tangent frame."""
    import struct
    xml = _write(tmp_path, """
    <shape type="sphere"><point name="center" x="1" y="2" z="3"/><float name="radius" value="0.5"/></shape>
    <shape type="sphere"><boolean name="flipNormals" value="true"/><transform name="toWorld"><scale x="100" y="100" z="100"/></transform>
        <emitter type="area"><rgb name="radiance" value="0.3, 0.3, 0.3"/></emitter></shape>
    <shape type="sphere"><float name="radius" value="2"/><transform name="toWorld"><rotate y="1" angle="90"/><scale value="3"/><translate x="5" y="6" z="7"/></transform>
        <bsdf type="dielectric"/></shape>""")
    desc, _, info = ppg_host.load_scene(xml, defines=dict(nee="never"))
    a, b, c = desc.spheres
    assert a["center"] == (1.0, 2.0, 3.0) and a["radius"] == 0.5 and not a["flip_normals"] and a["emitter"] == -1
    assert np.array_equal(np.reshape(a["to_world"], (3, 3)), np.eye(3))
    assert b["center"] == (0.0, 0.0, 0.0) and abs(b["radius"] - 100.0) < 1e-4 and b["flip_normals"]
    assert np.allclose(np.reshape(b["to_world"], (3, 3)), np.eye(3), atol=1e-6)
    assert desc.emitters[b["emitter"]]["radiance"] == pytest.approx((0.3, 0.3, 0.3)) and b["emitter"] == len(desc.emitters) - 1
    assert desc.materials[b["material"]] == dict(type=0, reflectance=(0.0, 0.0, 0.0))   # under an emitter: all-absorbing (shape.cpp:51-56)
    assert desc.materials[a["material"]] == dict(type=0, reflectance=(0.5, 0.5, 0.5))   # otherwise Mitsuba's 0.5 Lambertian (shape.cpp:57-64)
    assert np.allclose(c["center"], (5, 6, 7)) and abs(c["radius"] - 6.0) < 1e-5 and desc.materials[c["material"]]["type"] == 6
    R = np.reshape(c["to_world"], (3, 3))                                   # rotate 90 deg about y: x -> -z, z -> x
    assert np.allclose(R, [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], atol=1e-6)
    # flat file: block bit 2, then ppg_sphere records of 64 bytes
    p = str(tmp_path / "s.ppgs")
    ppg_host.save_scene(desc, p)
    raw = open(p, "rb").read()
    assert struct.unpack_from("<6I", raw, 4)[5] & 4
    n = struct.unpack_from("<I", raw, len(raw) - 4 - 3 * 64)[0]
    rec = struct.unpack_from("<4f9fIii", raw, len(raw) - 64)
    assert n == 3 and rec[:4] == pytest.approx((5, 6, 7, 6.0)) and rec[13:] == (c["material"], -1, 0)
    # XML round trip keeps spheres and the emitter numbering
    back, _, _ = ppg_host.load_scene(ppg_host.save_scene_xml(desc, dict(budgetType="spp", budget=8.0), str(tmp_path / "rt")))
    key = lambda sp: tuple(np.round(sp["center"], 3))  # noqa: E731
    for sp in desc.spheres:
        (q,) = [x for x in back.spheres if key(x) == key(sp)]
        assert abs(q["radius"] - sp["radius"]) < 1e-4 and bool(q["flip_normals"]) == bool(sp["flip_normals"]) and np.allclose(q["to_world"], sp["to_world"], atol=1e-6)
        assert (q["emitter"] < 0) == (sp["emitter"] < 0)
        if sp["emitter"] >= 0:
            assert back.emitters[q["emitter"]]["radiance"] == pytest.approx(desc.emitters[sp["emitter"]]["radiance"])
    with pytest.raises(mitsuba_xml.SceneError, match="radius"):
        ppg_host.load_scene(_write(tmp_path, '<shape type="sphere"><float name="radius" value="0"/></shape>'), defines=dict(nee="never"))


def test_lenient_loading_skips_missing_meshes(tmp_path):
    xml = _write(tmp_path, '<shape type="obj"><string name="filename" value="meshes/not-there.obj"/></shape>')
    with pytest.raises(mitsuba_xml.SceneError, match="not found"):
        ppg_host.load_scene(xml, defines=dict(nee="never"))
    desc, _, info = ppg_host.load_scene(xml, defines=dict(nee="never"), strict=False)
    assert any("not-there.obj" in w for w in info["warnings"]) and desc.n_triangles > 0


def test_max_smooth_angle_rebuilds_the_topology(tmp_path):
    """obj.cpp:336-343 → TriMesh::rebuildTopology (trimesh.cpp:468-608): the file's normals are dropped, vertices re-merged, and smooth
    normals stop at creases sharper than the angle.  A cube with shared corners: 30 deg → every face gets its own four vertices and a
    flat normal; 100 deg (more than the cube's 90) → the eight corners stay shared and their normals are the diagonals."""
    v = [(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    (tmp_path / "meshes").mkdir(exist_ok=True)
    (tmp_path / "meshes" / "cube.obj").write_text("".join("v %d %d %d\n" % q for q in v) + "vn 0 0 1\n" + "".join("f " + " ".join("%d//1" % (i + 1) for i in q) + "\n" for q in quads))
    p = str(tmp_path / "meshes" / "cube.obj")
    flat, smooth = mitsuba_xml.load_obj(p, max_smooth_angle=30.0)[0], mitsuba_xml.load_obj(p, max_smooth_angle=100.0)[0]
    assert len(flat["positions"]) == 24 and len(smooth["positions"]) == 8 and len(flat["indices"]) == len(smooth["indices"]) == 12
    P, I = flat["positions"], flat["indices"]
    fn = np.cross(P[I[:, 1]] - P[I[:, 0]], P[I[:, 2]] - P[I[:, 0]]); fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    for k in range(3):
        assert np.allclose(flat["normals"][I[:, k]], fn, atol=1e-6)                    # flat per face (the file's bogus "vn 0 0 1" is gone)
    assert np.allclose(np.abs(smooth["normals"]), 1 / np.sqrt(3), atol=1e-5)            # corner diagonals
    xml = _write(tmp_path, '<shape type="obj"><string name="filename" value="meshes/cube.obj"/><float name="maxSmoothAngle" value="30"/></shape>')
    desc, _, _ = ppg_host.load_scene(xml, defines=dict(nee="never"))
    base, _, _ = ppg_host.load_scene(_write(tmp_path), defines=dict(nee="never"))
    assert desc.n_triangles == base.n_triangles + 12
    with pytest.raises(mitsuba_xml.SceneError, match="same time"):
        ppg_host.load_scene(_write(tmp_path, '<shape type="obj"><string name="filename" value="meshes/cube.obj"/><float name="maxSmoothAngle" value="30"/>'
                                             '<boolean name="faceNormals" value="true"/></shape>'), defines=dict(nee="never"))


def test_cube_shape(tmp_path):
    """shapes/cube.cpp: 24 vertices (each face its own four, so the normals are flat), 12 triangles wound outward; toWorld may stretch it
    (normals through the inverse transpose); flipNormals negates the normals and leaves the winding."""
    xml = _write(tmp_path, '<shape type="cube"><transform name="toWorld"><scale x="2" y="0.5" z="1"/><translate x="10"/></transform></shape>')
    desc, _, _ = ppg_host.load_scene(xml, defines=dict(nee="never"))
    base, _, _ = ppg_host.load_scene(_write(tmp_path), defines=dict(nee="never"))
    assert desc.n_triangles == base.n_triangles + 12
    tri = desc.indices[-12:]
    P, N = desc.positions, desc.normals
    assert P[tri].reshape(-1, 3).min(0).tolist() == [8.0, -0.5, -1.0] and P[tri].reshape(-1, 3).max(0).tolist() == [12.0, 0.5, 1.0]
    fn = np.cross(P[tri[:, 1]] - P[tri[:, 0]], P[tri[:, 2]] - P[tri[:, 0]]); fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    centre = np.float32([10, 0, 0])
    assert np.all(np.sum(fn * (P[tri].mean(1) - centre), 1) > 0)                       # wound outward
    for k in range(3):
        assert np.allclose(N[tri[:, k]], fn, atol=1e-6)                                  # flat normals = the geometric ones, also when stretched
    flipped, _, _ = ppg_host.load_scene(_write(tmp_path, '<shape type="cube"><boolean name="flipNormals" value="true"/></shape>'), defines=dict(nee="never"))
    t2 = flipped.indices[-12:]
    f2 = np.cross(flipped.positions[t2[:, 1]] - flipped.positions[t2[:, 0]], flipped.positions[t2[:, 2]] - flipped.positions[t2[:, 0]])
    assert np.all(np.sum(f2 * flipped.normals[t2[:, 0]], 1) < 0)


def write_serialized(path, meshes, version=4):
    """Mitsuba's .serialized container (trimesh.cpp:1130-1190): per mesh {u16 0x041C, u16 version, zlib{flags, [name\\0], u64 nv, u64 nt,
    positions, [normals], [uvs], indices}}, then the offset table and the mesh count."""
    import struct
    import zlib
    out, offsets = b"", []
    for m in meshes:
        dbl = m.get("double", False)
        dt = "<f8" if dbl else "<f4"
        flags = (0x2000 if dbl else 0x1000) | (1 if m.get("normals") is not None else 0) | (2 if m.get("uvs") is not None else 0)
        body = struct.pack("<I", flags) + ((m.get("name", "mesh").encode() + b"\0") if version == 4 else b"")
        body += struct.pack("<QQ", len(m["positions"]), len(m["indices"]))
        body += np.asarray(m["positions"], dt).tobytes()
        if m.get("normals") is not None:
            body += np.asarray(m["normals"], dt).tobytes()
        if m.get("uvs") is not None:
            body += np.asarray(m["uvs"], dt).tobytes()
        body += np.asarray(m["indices"], "<u4").tobytes()
        offsets.append(len(out))
        out += struct.pack("<HH", 0x041C, version) + zlib.compress(body)
    out += b"".join(struct.pack("<Q" if version == 4 else "<I", o) for o in offsets) + struct.pack("<I", len(meshes))
    open(path, "wb").write(out)


def _two_meshes():
    rng = np.random.RandomState(8)
    quad = dict(name="quad", positions=np.float32([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]), indices=np.uint32([[0, 1, 2], [0, 2, 3]]),
                normals=np.float32([[0, 0, 1]] * 4), uvs=np.float32([[0, 0], [1, 0], [1, 1], [0, 1]]))
    P = rng.rand(9, 3).astype(np.float32)
    fan = dict(name="fan", positions=P, indices=np.uint32([[0, k, k + 1] for k in range(1, 8)]), double=True)
    return quad, fan


@pytest.mark.parametrize("version", [3, 4])
def test_serialized_meshes(tmp_path, version):
    """shapes/serialized.cpp + TriMesh::loadCompressed: both format versions, float and double payloads, the offset table (shapeIndex),
    stored normals kept / generated when absent, toWorld with a mirror (winding swapped, serialized.cpp:197-202), flipNormals."""
    quad, fan = _two_meshes()
    (tmp_path / "meshes").mkdir(exist_ok=True)
    p = str(tmp_path / "meshes" / "two.serialized")
    write_serialized(p, [quad, fan], version)
    a = mitsuba_xml.load_serialized(p)
    assert np.array_equal(a["positions"], quad["positions"]) and np.array_equal(a["indices"], quad["indices"]) and np.array_equal(a["normals"], quad["normals"])
    b = mitsuba_xml.load_serialized(p, shape_index=1)
    assert np.array_equal(b["positions"], fan["positions"]) and np.array_equal(b["indices"], fan["indices"])
    assert np.array_equal(b["normals"], mitsuba_xml.compute_normals(fan["positions"], fan["indices"], False))     # none stored: generated
    mirror = np.diag(np.float32([-1, 1, 1, 1]))
    c = mitsuba_xml.load_serialized(p, mirror)
    assert np.array_equal(c["indices"], quad["indices"][:, [1, 0, 2]]) and np.array_equal(c["positions"][:, 0], -quad["positions"][:, 0])
    d = mitsuba_xml.load_serialized(p, flip_normals=True)
    assert np.array_equal(d["normals"], -quad["normals"])
    e = mitsuba_xml.load_serialized(p, shape_index=1, face_normals=True)
    assert e["normals"] is None
    xml = _write(tmp_path, '<shape type="serialized"><string name="filename" value="meshes/two.serialized"/><integer name="shapeIndex" value="1"/>'
                           '<transform name="toWorld"><scale value="2"/></transform><bsdf type="conductor"><string name="material" value="none"/></bsdf></shape>')
    desc, _, _ = ppg_host.load_scene(xml, defines=dict(nee="never"))
    assert np.allclose(desc.positions[-9:], 2 * fan["positions"]) and desc.materials[desc.tri_material[-1]]["type"] == 2
    with pytest.raises(mitsuba_xml.SceneError, match="out of range"):
        mitsuba_xml.load_serialized(p, shape_index=5)
    open(str(tmp_path / "bad.serialized"), "wb").write(b"\x00\x01\x02\x03rubbish")
    with pytest.raises(mitsuba_xml.SceneError, match="invalid file format"):
        mitsuba_xml.load_serialized(str(tmp_path / "bad.serialized"))


def write_ply(path, P, faces, fmt="ascii", normals=None, double=False):
    import struct
    props = [("x", 0), ("y", 1), ("z", 2)] + ([("nx", 3), ("ny", 4), ("nz", 5)] if normals is not None else [])
    V = np.hstack([P, normals]) if normals is not None else np.asarray(P)
    head = "ply\nformat %s 1.0\ncomment written by the test\nelement vertex %d\n" % (fmt, len(V))
    head += "".join("property %s %s\n" % ("double" if double else "float", n) for n, _ in props) + "property uchar red\n"
    head += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(faces)
    with open(path, "wb") as f:
        f.write(head.encode())
        if fmt == "ascii":
            for v in V:
                f.write((" ".join(repr(float(x)) for x in v) + " 200\n").encode())
            for fc in faces:
                f.write(("%d %s\n" % (len(fc), " ".join(str(i) for i in fc))).encode())
        else:
            bo = "<" if fmt == "binary_little_endian" else ">"
            for v in V:
                f.write(struct.pack(bo + "%d%sB" % (len(v), "d" if double else "f"), *[float(x) for x in v], 200))
            for fc in faces:
                f.write(struct.pack(bo + "B%di" % len(fc), len(fc), *fc))


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
def test_ply_meshes(tmp_path, fmt):
    """shapes/ply.cpp: the three encodings, extra properties skipped, quads split as (0, 1, 2), (3, 0, 2), normals kept or generated."""
    P = np.float32([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1]])
    faces = [(0, 1, 2, 3), (0, 1, 4), (1, 2, 4)]
    (tmp_path / "meshes").mkdir(exist_ok=True)
    p = str(tmp_path / "meshes" / "m.ply")
    write_ply(p, P, faces, fmt, double=(fmt == "binary_big_endian"))
    m = mitsuba_xml.load_ply(p)
    assert m["indices"].tolist() == [[0, 1, 2], [3, 0, 2], [0, 1, 4], [1, 2, 4]] and np.array_equal(m["positions"], P)
    assert np.array_equal(m["normals"], mitsuba_xml.compute_normals(P, m["indices"], False))
    N = np.float32([[0, 0, 1]] * 5)
    write_ply(p, P, faces, fmt, normals=N)
    assert np.array_equal(mitsuba_xml.load_ply(p, flip_normals=True)["normals"], -N)
    xml = _write(tmp_path, '<shape type="ply"><string name="filename" value="meshes/m.ply"/><transform name="toWorld"><translate z="5"/></transform></shape>')
    desc, _, _ = ppg_host.load_scene(xml, defines=dict(nee="never"))
    assert np.allclose(desc.positions[-5:], P + np.float32([0, 0, 5]))
    write_ply(p, P, [(0, 1, 2, 3, 4)], fmt)
    with pytest.raises(mitsuba_xml.SceneError, match="triangle and quad"):
        mitsuba_xml.load_ply(p)


def test_blackbody_spectra(tmp_path):
    """<blackbody> (scenehandler.cpp:534-547, spectrum.cpp:483-495): Planck's law through the CIE matching functions.  The chromaticities
    land on the published Planckian locus (6500 K: x 0.3135, y 0.3237; 5000 K: 0.3451, 0.3516; 3000 K: 0.4369, 0.4041); the magnitude is
    spectral radiance in W m^-2 nm^-1 sr^-1 weighted by y-bar, `scale` multiplies it."""
    from ppg_host import spectrum
    M = np.linalg.inv(spectrum._XYZ_TO_RGB)
    for T, xy in ((6500, (0.3135, 0.3237)), (5000, (0.3451, 0.3516)), (3000, (0.4369, 0.4041))):
        XYZ = M @ spectrum.blackbody_to_rgb(T).astype(np.float64)
        assert abs(XYZ[0] / XYZ.sum() - xy[0]) < 3e-4 and abs(XYZ[1] / XYZ.sum() - xy[1]) < 3e-4
    assert np.allclose(spectrum.blackbody_to_rgb(5000, 1e-4), spectrum.blackbody_to_rgb(5000) * np.float32(1e-4), rtol=1e-6)
    xml = _write(tmp_path, '<shape type="rectangle"><emitter type="area"><blackbody name="radiance" temperature="4500K" scale="0.001"/></emitter></shape>')
    desc, _, _ = ppg_host.load_scene(xml, defines=dict(nee="never"))
    assert np.allclose(desc.emitters[-1]["radiance"], spectrum.blackbody_to_rgb(4500, 0.001), rtol=1e-6)
    r, g, b = desc.emitters[-1]["radiance"]
    assert r > g > b > 0                                    # a warm white


def test_spectrum_from_a_file(tmp_path):
    """<spectrum filename="x.spd"/> (scenehandler.cpp:557-567): the file's "wavelength value" samples go the same way as an inline list."""
    from ppg_host import spectrum
    pairs = [(400, 0.1), (500, 0.8), (600, 0.5), (700, 0.2)]
    (tmp_path / "meshes").mkdir(exist_ok=True)
    (tmp_path / "meshes" / "paint.spd").write_text("# measured\n" + "".join("%g %g\n" % p for p in pairs) + "\n")
    xml = _write(tmp_path, '<shape type="rectangle"><bsdf type="diffuse"><spectrum name="reflectance" filename="meshes/paint.spd"/></bsdf></shape>')
    desc, _, _ = ppg_host.load_scene(xml, defines=dict(nee="never"))
    assert np.allclose(desc.materials[desc.tri_material[-1]]["reflectance"], spectrum.interpolated_to_rgb(pairs), rtol=1e-6)
    with pytest.raises(mitsuba_xml.SceneError, match="not found"):
        ppg_host.load_scene(_write(tmp_path, '<shape type="rectangle"><bsdf type="diffuse"><spectrum name="reflectance" filename="nope.spd"/></bsdf></shape>'), defines=dict(nee="never"))


def test_named_conductor_materials_come_from_the_mitsuba_data_directory(tmp_path):
    """conductor.cpp:160-186 / roughconductor.cpp:174-186: `material` names data/ior/<name>.{eta,k}.spd, integrated against the CIE curves
    without zero extension or clamping; Mitsuba's default is copper.  Gold gives the familiar (0.143, 0.375, 1.442) / (3.98, 2.39, 1.60)."""
    data = MITSUBA_DATA
    xml = _write(tmp_path, '<shape type="rectangle"><bsdf type="roughconductor"><string name="material" value="Au"/><string name="distribution" value="ggx"/></bsdf></shape>'
                           '<shape type="rectangle"><bsdf type="conductor"/></shape>'
                           '<shape type="rectangle"><bsdf type="conductor"><string name="material" value="Ag"/><float name="extEta" value="1.33"/></bsdf></shape>')
    desc, _, _ = ppg_host.load_scene(xml, defines=dict(nee="never"), data_dir=data)
    au, cu, ag = desc.materials[-3:]
    assert np.allclose(au["eta"], (0.143, 0.375, 1.442), atol=5e-3) and np.allclose(au["k"], (3.983, 2.386, 1.603), atol=5e-3)
    assert np.allclose(cu["eta"], (0.2, 0.92, 1.1), atol=2e-2) and np.allclose(cu["k"], (3.9, 2.45, 2.14), atol=3e-2)
    plain, _, _ = ppg_host.load_scene(_write(tmp_path, '<shape type="rectangle"><bsdf type="conductor"><string name="material" value="Ag"/></bsdf></shape>'),
                                      defines=dict(nee="never"), data_dir=data)
    assert np.allclose(np.float32(ag["eta"]) * np.float32(1.33), np.float32(plain.materials[-1]["eta"]) * np.float32(1.000277), rtol=1e-5)
    with pytest.raises(mitsuba_xml.SceneError, match="data/ior"):
        ppg_host.load_scene(xml, defines=dict(nee="never"), data_dir=str(tmp_path))


LENIENT_EXTRA = """
    <bsdf type="bumpmap"><texture type="scale"><float name="scale" value="0.01"/></texture>
        <bsdf type="twosided" id="inner"><bsdf type="diffuse"><texture name="reflectance" type="bitmap"><string name="filename" value="t.jpg"/></texture></bsdf></bsdf></bsdf>
    <shape type="rectangle"><ref id="inner"/></shape>
    <shape type="rectangle"><bsdf type="bumpmap"><texture type="bitmap"><string name="filename" value="b.png"/></texture>
        <bsdf type="roughconductor"><string name="material" value="none"/><string name="distribution" value="ggx"/></bsdf></bsdf></shape>
    <emitter type="sunsky"><float name="hour" value="9"/></emitter>
"""


def test_lenient_loading_of_kitchen_style_constructs(tmp_path):
    """What the reference's KITCHEN scene needs from a lenient load: an id on a bsdf NESTED in a bumpmap is a named object of its own
    (the shapes reference the inner twosided, not the bump adapter); textures whose files are missing fall back to the plug-in's default
    value; a bump map that cannot be loaded is dropped around its nested bsdf; the sunsky emitter is skipped without a Mitsuba source tree
    for the sky model's tables — each with a warning.  Strict loading names the first unsupported construct."""
    xml = _write(tmp_path, LENIENT_EXTRA)
    with pytest.raises(mitsuba_xml.SceneError, match="bumpmap|texture|bitmap|sunsky"):
        ppg_host.load_scene(xml, defines=dict(nee="never"))
    desc, _, info = ppg_host.load_scene(xml, defines=dict(nee="never"), strict=False)
    w = "\n".join(info["warnings"])
    assert "texture on 'reflectance' ignored" in w and "bump map dropped" in w and "emitter 'sunsky' skipped" in w
    a, b = desc.materials[desc.tri_material[-4]], desc.materials[desc.tri_material[-1]]
    assert a["type"] == 1 and tuple(a["reflectance"]) == (0.5, 0.5, 0.5)          # the inner twosided diffuse with diffuse's default reflectance
    assert b["type"] == 4 and b.get("distribution") is None
