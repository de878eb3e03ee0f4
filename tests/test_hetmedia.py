"""Heterogeneous participating media without a GPU (include/ppg.h ppg_set_media_volumes):
  * the numpy restatement (tests/hetmedium_ref.py) against closed forms, its float32 / float64 figures and its share of undecided items;
  * the Python loader: .vol files, <medium type="heterogeneous"> over const and grid volumes, inline and by reference, and every refusal by
    its message;
  * the bindings: struct sizes and offsets against the header's, the flattening of medium dicts into the side list;
  * ppg_set_scene's validation and derived tables through the host build stage (tests/hetmedia_build_check.hip, no device).
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ppg_host
from ppg_host import bindings as B
from ppg_host import mitsuba_xml
from conftest import ROOT

import hetmedium_ref as R

SceneError = mitsuba_xml.SceneError
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ 1. the restatement
def test_figures_are_the_measured_ones_and_few_items_are_undecided():
    fig = R.figures()
    for q in R.QUANTITIES:
        assert float("%.2g" % fig[q]) == R.FIGURES[q], (q, fig[q])
    lookups, tracking, differ = R.undecided_shares()
    print("undecided: lookups", lookups, "tracking", tracking, "decided items on which float32 draws another count", differ)
    assert lookups <= 0.01 and tracking <= 0.01 and differ == 0.0
    items, _ = R.lookup_items()
    assert len(items) == 4096
    for k, (_, medium) in enumerate(R.TRACK_MEDIA):  # about 3 expected steps per segment
        r = R.evaluate_track(medium, R.track_items(k, medium), f64)
        assert 1.0 < r["draws"].mean() < 12.0


@pytest.mark.parametrize("dtype", [f32, f64], ids=["float32", "float64"])
def test_trilinear_interpolation_reproduces_an_affine_field(dtype):
    """a field a + b . u sampled at the nodes of a 5 x 4 x 3 grid, under a rotated and scaled to_world, at random points inside"""
    rs = np.random.RandomState(3)
    lo, hi = np.array([-1.0, 0.5, 2.0]), np.array([1.5, 2.0, 2.75])
    zz, yy, xx = np.meshgrid(np.linspace(0, 1, 3), np.linspace(0, 1, 4), np.linspace(0, 1, 5), indexing="ij")
    coef = (0.2, 0.3, 0.15, 0.25)
    data = (coef[0] + coef[1] * xx + coef[2] * yy + coef[3] * zz).astype(f32)
    v = dict(data=data, min=tuple(lo), max=tuple(hi), to_world=R.SKEW_TO_WORLD)
    u = rs.uniform(0.01, 0.99, (2000, 3))
    tw = np.asarray(R.SKEW_TO_WORLD, f64)
    p = (lo + u * (hi - lo)) @ tw[:3, :3].T + tw[:3, 3]
    got, _ = R.lookup(R.derive_volume(v, 1, dtype), p.astype(dtype))
    want = coef[0] + u @ np.asarray(coef[1:])
    # float32 texels and, in float32, a few roundings of coordinates of a few units: 4 of them carried through slopes below 1 per cell
    tol = 2e-7 if dtype is f64 else 4e-6
    assert np.abs(got[:, 0] - want).max() < tol
    rgb = dict(v, data=np.stack([data, data * 0.5, 1 - data], -1))
    got3, _ = R.lookup(R.derive_volume(rgb, 3, dtype), p.astype(dtype))
    assert np.abs(got3 - np.stack([want, want * 0.5, 1 - want], -1)).max() < tol
    # outside the nodes the lookup answers 0
    far, _ = R.lookup(R.derive_volume(v, 1, dtype), (p + 50.0).astype(dtype))
    assert np.all(far == 0)


def test_tracked_survival_of_a_linear_ramp_is_the_exponential_of_its_integral():
    """2 * 10^5 keys along one ray through the ramp grid: the share of runs without a collision (sampleDistance failing) lies within 5
    binomial standard errors of exp(-scale int rho), and so does evalTransmittance's mean — each run is such a trial"""
    n = 200000
    scale = 3.0
    M = R.derive_medium(dict(type="heterogeneous", density=R.ramp_grid(), albedo=dict(value=0.5), scale=scale), f64)
    o = np.tile([-0.5, 0.4, 0.6], (n, 1))
    d = np.tile([1.0, 0.0, 0.0], (n, 1))
    key = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(12345)) & np.uint64(0xffffffff)
    s = R.sample_distance(M, o, d, np.full(n, np.inf), key, np.zeros(n, np.uint64))
    want = np.exp(-scale * 0.5)  # rho rises from 0.2 to 0.8 over the unit box: its integral is 0.5
    se = np.sqrt(want * (1 - want) / n)
    survived = 1.0 - s["success"].mean()
    print("survival", survived, "closed form", want, "standard error", se)
    assert abs(survived - want) <= 5 * se
    assert np.all(s["t"][s["success"] != 0] >= 0.5) and np.all(s["t"][s["success"] != 0] < 1.5)  # the box starts 0.5 along the ray
    e = R.eval_transmittance(M, o, d, np.full(n, np.inf), key, s["dim"])
    assert set(np.unique(e["value"])) <= {0.0, 0.5, 1.0}
    assert abs(e["value"].mean() - want) <= 5 * np.sqrt(want * (1 - want) / (2 * n))
    # sigma_s = albedo * density at t, transmittance = 1 / density at t
    hit = s["success"] != 0
    rho = scale * (0.2 + 0.6 * (s["t"][hit] - 0.5))
    assert np.abs(s["sigma_s"][hit, 0] - 0.5 * rho).max() < 1e-6 and np.abs(s["transmittance"][hit] * rho - 1).max() < 1e-6


def test_a_const_density_reduces_to_the_exponential_law():
    """no collision is ever rejected: the first draw alone places the event, t = -log(1 - u) * invMaxDensity, on a ray of any direction
    without a zero component; with one, the default box refuses the ray"""
    n = 50000
    M = R.derive_medium(dict(type="heterogeneous", density=dict(value=0.75), albedo=dict(value=(0.9, 0.5, 0.2)), scale=2.0), f64)
    key = np.arange(n, dtype=np.uint64) * np.uint64(7919)
    o, d = np.tile([0.3, -0.2, 0.1], (n, 1)), np.tile(np.array([1.0, 2.0, -2.0]) / 3.0, (n, 1))
    maxt = np.full(n, 1.0)
    s = R.sample_distance(M, o, d, maxt, key, np.zeros(n, np.uint64))
    u = R.rand(key, np.zeros(n, np.uint64)).astype(f64)
    t = -np.log(1 - u) * float(M["inv_max_density"])  # (the float32 1 / maxDensity that heterogeneous.cpp:242 keeps)
    assert np.array_equal(s["success"] != 0, t < 1.0) and np.all(s["draws"] == np.where(t < 1.0, 2, 1))
    assert np.abs(s["t"] - np.where(t < 1.0, t, 0.0)).max() < 1e-12
    assert abs((s["success"] == 0).mean() - np.exp(-1.5)) <= 5 * np.sqrt(np.exp(-1.5) * (1 - np.exp(-1.5)) / n)
    assert np.allclose(s["sigma_s"][s["success"] != 0], np.asarray((0.9, 0.5, 0.2), f32).astype(f64) * 1.5) and np.allclose(s["transmittance"][s["success"] != 0], 1 / 1.5)
    flat = R.sample_distance(M, o, np.tile([0.0, 0.6, 0.8], (n, 1)), maxt, key, np.zeros(n, np.uint64))
    assert not flat["success"].any() and not flat["draws"].any()
    assert np.all(R.eval_transmittance(M, o, np.tile([0.0, 0.6, 0.8], (n, 1)), maxt, key, np.zeros(n, np.uint64))["value"] == 1)


def test_the_restated_sampler_is_the_projects():
    from commit_ref import ppg_rand
    keys, dims = np.array([0, 1, 0xdeadbeef, 0xffffffff, 12345], np.uint64), np.array([0, 7, 4096, 0x3fffffff, 99], np.uint64)
    assert [float(v) for v in R.rand(keys, dims)] == [float(ppg_rand(int(k), int(d))) for k, d in zip(keys, dims)]


# ------------------------------------------------------------------------------------------------ 2. the loader
XML = """<scene version="0.5.0">
  <integrator type="guided_path"/>
  <sensor type="perspective"> <float name="fov" value="40"/> %(sensor)s
    <film type="hdrfilm"> <integer name="width" value="8"/> <integer name="height" value="8"/> <rfilter type="box"/> </film> </sensor>
  %(top)s
  %(shapes)s
  <shape type="rectangle"> <bsdf type="diffuse"/> <emitter type="area"> <rgb name="radiance" value="1"/> </emitter> </shape>
</scene>
"""
CONST = '<volume name="density" type="constvolume"> <float name="value" value="0.5"/> </volume> <volume name="albedo" type="constvolume"> <rgb name="value" value="0.9, 0.5, 0.2"/> </volume>'


def _het(body, attrs='name="interior"'):
    return '<medium type="heterogeneous" %s> %s </medium>' % (attrs, body)


def _load(tmp_path, sensor="", top="", shapes="", strict=True):
    p = tmp_path / "s.xml"
    p.write_text(XML % dict(sensor=sensor, top=top, shapes=shapes))
    desc, _, info = ppg_host.load_scene(str(p), strict=strict)
    return desc, info


def _grid(channels=1, seed=1):
    shape = (3, 4, 5) if channels == 1 else (3, 4, 5, 3)
    return np.random.RandomState(seed).uniform(0, 1, shape).astype(f32)


def test_vol_files_round_trip(tmp_path):
    for channels in (1, 3):
        data = _grid(channels)
        p = str(tmp_path / ("f%d.vol" % channels))
        ppg_host.write_vol(p, data, (-1, -2, -3), (1, 2.5, 3), encoding="float32")
        raw = open(p, "rb").read()
        assert raw[:4] == b"VOL\x03" and len(raw) == 48 + data.size * 4
        assert list(np.frombuffer(raw, "<i4", 5, 4)) == [1, 5, 4, 3, channels]
        v = ppg_host.read_vol(p)
        assert v["encoding"] == "float32" and v["min"] == (-1.0, -2.0, -3.0) and v["max"] == (1.0, 2.5, 3.0)
        assert v["data"].dtype == f32 and np.array_equal(v["data"].view(np.uint32), data.view(np.uint32))
        # the reference's order: ((z * ry + y) * rx + x) * channels + c
        assert np.frombuffer(raw, "<f4", 1, 48 + 4 * (((2 * 4 + 1) * 5 + 3) * channels + channels - 1))[0] == data[(2, 1, 3) if channels == 1 else (2, 1, 3, channels - 1)]
    # uint8: every code becomes i / 255.0f, the reference's m_densityMap, bit for bit
    codes = np.arange(256, dtype=np.uint8).reshape(4, 8, 8)
    p = str(tmp_path / "u.vol")
    ppg_host.write_vol(p, codes, (0, 0, 0), (1, 1, 1), encoding="uint8")
    v = ppg_host.read_vol(p)
    want = np.arange(256, dtype=f32) / f32(255.0)
    assert v["encoding"] == "uint8" and np.array_equal(v["data"].reshape(-1).view(np.uint32), want.view(np.uint32))
    ppg_host.write_vol(p, want.reshape(4, 8, 8), (0, 0, 0), (1, 1, 1), encoding="uint8")  # floats are rounded to the nearest code
    assert open(p, "rb").read()[48:] == codes.tobytes()
    with pytest.raises(ValueError, match="encoding 'float16' is not supported"):
        ppg_host.write_vol(p, want.reshape(4, 8, 8), (0, 0, 0), (1, 1, 1), encoding="float16")


def test_a_heterogeneous_medium_on_a_shape_and_by_reference(tmp_path):
    ppg_host.write_vol(str(tmp_path / "smoke.vol"), _grid(1), (0, 0, 0), (1, 1, 1))
    ppg_host.write_vol(str(tmp_path / "colour.vol"), _grid(3, 2), (0, 0, 0), (2, 2, 2), encoding="uint8")
    smoke = ('<volume name="density" type="gridvolume"> <string name="filename" value="smoke.vol"/> <boolean name="sendData" value="true"/>'
             ' <transform name="toWorld"> <scale value="2"/> <translate x="1" y="0" z="-1"/> </transform> </volume>'
             '<volume name="albedo" type="gridvolume"> <string name="filename" value="colour.vol"/> <point name="min" x="-1" y="-1" z="-1"/> <point name="max" x="1" y="1" z="1"/> </volume>'
             '<float name="scale" value="12.5"/> <string name="method" value="woodcock"/> <float name="stepSize" value="0.01"/>'
             '<phase type="hg"> <float name="g" value="0.6"/> </phase>')
    shapes = ('<shape type="cube"> <bsdf type="null"/> <ref name="interior" id="smoke"/> </shape>'
              '<shape type="rectangle"> <bsdf type="null"/> <ref name="interior" id="smoke"/> <ref name="exterior" id="haze"/> </shape>')
    desc, info = _load(tmp_path, top=_het(smoke, 'id="smoke"') + _het(CONST, 'id="haze"'), shapes=shapes, sensor=_het(CONST, ""))
    assert not info["warnings"] and len(desc.media) == 3 and desc.camera_medium == 3
    words = np.asarray(desc.tri_media)
    assert (words[:12] == B.media_word(interior=0)).all() and (words[12:14] == B.media_word(interior=0, exterior=1)).all() and not words[14:].any()
    m = desc.media[0]
    assert sorted(m) == ["albedo", "density", "g", "phase", "scale", "type"] and m["type"] == "heterogeneous" and m["scale"] == 12.5 and (m["phase"], m["g"]) == ("hg", 0.6)
    assert np.array_equal(m["density"]["data"], _grid(1)) and m["density"]["min"] == (0.0, 0.0, 0.0) and m["density"]["max"] == (1.0, 1.0, 1.0)
    assert np.allclose(m["density"]["to_world"], [[2, 0, 0, 1], [0, 2, 0, 0], [0, 0, 2, -1], [0, 0, 0, 1]])
    assert m["albedo"]["data"].shape == (3, 4, 5, 3) and m["albedo"]["min"] == (-1.0, -1.0, -1.0) and m["albedo"]["max"] == (1.0, 1.0, 1.0) and m["albedo"]["to_world"] is None
    assert np.array_equal(m["albedo"]["data"], (np.rint(_grid(3, 2).astype(f64) * 255).astype(np.uint8).astype(f32) / f32(255.0)))
    haze = desc.media[1]
    assert haze == dict(type="heterogeneous", density=dict(value=0.5), albedo=dict(value=(pytest.approx(0.9), 0.5, pytest.approx(0.2))), scale=1.0)
    # ... and the side list the engine sends: the shared <ref> is one medium, its two grids two volumes
    volumes, entries, _ = B.flatten_media_volumes(desc.media)
    assert len(volumes) == 6 and [(e.medium, e.density, e.albedo) for e in entries] == [(0, 0, 1), (1, 2, 3), (2, 4, 5)]
    assert (volumes[0].kind, volumes[0].channels, list(volumes[0].res)) == (B.Volume.GRID, 1, [5, 4, 3]) and volumes[1].channels == 3
    assert (volumes[2].kind, volumes[2].channels, volumes[3].channels) == (B.Volume.CONST, 1, 3) and abs(entries[0].scale - 12.5) < 1e-6
    medium = B.Medium.from_dict(m)
    assert list(medium.sigma_a) == [0, 0, 0] and list(medium.sigma_s) == [0, 0, 0] and (medium.strategy, medium.phase) == (0, 1) and abs(medium.g - 0.6) < 1e-6


def _vol_header(tmp_path, name, enc=1, channels=1, version=3, magic=b"VOL", cut=0):
    data = np.zeros(8 * channels, f32).tobytes()
    raw = magic + bytes([version]) + np.asarray([enc, 2, 2, 2, channels], "<i4").tobytes() + np.asarray([0, 0, 0, 1, 1, 1], "<f4").tobytes() + data
    (tmp_path / name).write_bytes(raw[:len(raw) - cut])
    return '<volume name="%%s" type="gridvolume"> <string name="filename" value="%s"/> </volume>' % name


ALBEDO = '<volume name="albedo" type="constvolume"> <rgb name="value" value="0.5"/> </volume>'
DENSITY = '<volume name="density" type="constvolume"> <float name="value" value="0.5"/> </volume>'
REFUSALS = [
    ("sigmaA and sigmaS", lambda t: _het('<rgb name="sigmaA" value="1"/> <rgb name="sigmaS" value="1"/>' + CONST),
     "medium type 'heterogeneous' is not supported (homogeneous media only) with 'sigmaA' / 'sigmaS': these belong to homogeneous media; give `density` and `albedo` volumes"),
    ("no density", lambda t: _het(ALBEDO), "medium type 'heterogeneous': No density specified!"),
    ("no albedo", lambda t: _het(DENSITY), "medium type 'heterogeneous': No albedo specified!"),
    ("simpson", lambda t: _het(CONST + '<string name="method" value="simpson"/>'), "medium type 'heterogeneous': method 'simpson' is not supported (woodcock)"),
    ("unknown method", lambda t: _het(CONST + '<string name="method" value="marching"/>'), "Unsupported integration method 'marching'"),
    ("float16", lambda t: _het(ALBEDO + _vol_header(t, "h.vol", enc=2) % "density"), "gridvolume (density) 'h.vol': encoding float16 is not supported (float32, uint8)"),
    ("quantized directions", lambda t: _het(ALBEDO + _vol_header(t, "q.vol", enc=4, channels=3) % "density"), "encoding quantized directions is not supported"),
    ("hgridvolume", lambda t: _het(ALBEDO + '<volume name="density" type="hgridvolume"/>'), "volume type 'hgridvolume' (density) is not supported (constvolume, gridvolume)"),
    ("volcache", lambda t: _het(DENSITY + '<volume name="albedo" type="volcache"/>'), "volume type 'volcache' (albedo) is not supported (constvolume, gridvolume)"),
    ("orientation", lambda t: _het(CONST + '<volume name="orientation" type="constvolume"> <vector name="value" x="0" y="1" z="0"/> </volume>'),
     "an 'orientation' volume (anisotropic media) is not supported"),
    ("one-channel albedo grid", lambda t: _het(DENSITY + _vol_header(t, "a1.vol") % "albedo"), "gridvolume 'a1.vol' has 1 channel: an albedo volume must have 3"),
    ("three-channel density grid", lambda t: _het(ALBEDO + _vol_header(t, "d3.vol", channels=3) % "density"), "gridvolume 'd3.vol' has 3 channels: a density volume must have 1"),
    ("missing file", lambda t: _het(ALBEDO + '<volume name="density" type="gridvolume"> <string name="filename" value="nowhere.vol"/> </volume>'), "gridvolume (density) 'nowhere.vol': "),
    ("no filename", lambda t: _het(ALBEDO + '<volume name="density" type="gridvolume"/>'), "gridvolume (density) without filename"),
    ("bad signature", lambda t: _het(ALBEDO + _vol_header(t, "m.vol", magic=b"VOX") % "density"), "bad header: not a .vol file"),
    ("bad version", lambda t: _het(ALBEDO + _vol_header(t, "v.vol", version=2) % "density"), "bad header: file format version 2 (3 is supported)"),
    ("unknown encoding", lambda t: _het(ALBEDO + _vol_header(t, "e.vol", enc=7) % "density"), "bad header: unknown encoding 7"),
    ("two channels", lambda t: _het(ALBEDO + _vol_header(t, "c.vol", channels=2) % "density"), "bad header: 2 x 2 x 2 cells, 2 channels (1 or 3 are supported)"),
    ("truncated data", lambda t: _het(ALBEDO + _vol_header(t, "t.vol", cut=4) % "density"), "bad header: the file holds 28 data bytes, 2 x 2 x 2 x 1 float32 texels need 32"),
    ("spectrum as a density", lambda t: _het(ALBEDO + '<volume name="density" type="constvolume"> <rgb name="value" value="0.5"/> </volume>'),
     "the constvolume for density must hold a float value (got <rgb>)"),
    ("anisotropic phase", lambda t: _het(CONST + '<phase type="microflake"/>'), "phase function type 'microflake' is not supported (isotropic, hg)"),
]


@pytest.mark.parametrize("name,body,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_loader_refuses_by_name(tmp_path, name, body, message):
    with pytest.raises(SceneError) as err:
        _load(tmp_path, shapes='<shape type="cube"> <bsdf type="null"/> %s </shape>' % body(tmp_path))
    assert message in str(err.value)


def test_a_lenient_load_drops_what_it_cannot_render_with_a_warning(tmp_path):
    shapes = "".join('<shape type="cube"> <bsdf type="null"/> %s </shape>' % body(tmp_path) for _, body, _ in REFUSALS) + '<shape type="cube"> <bsdf type="null"/> %s </shape>' % _het(CONST)
    desc, info = _load(tmp_path, top='<medium type="heterogeneous" id="het"/>', sensor='<ref id="het"/>', shapes=shapes, strict=False)
    assert len(desc.media) == 1 and desc.camera_medium == 0 and desc.media[0]["type"] == "heterogeneous"
    words = np.asarray(desc.tri_media)
    assert (words[12 * len(REFUSALS):12 * len(REFUSALS) + 12] == B.media_word(interior=0)).all() and not words[:12 * len(REFUSALS)].any()
    w = "\n".join(info["warnings"])
    assert "medium dropped (id 'het'): medium type 'heterogeneous': No density specified!" in w
    for _, _, message in REFUSALS:
        assert "medium dropped (interior of a cube shape): " in w and message in w, message


# ------------------------------------------------------------------------------------------------ 3. the bindings
def test_ctypes_mirrors_have_the_layout_of_the_headers(tmp_path):
    fields = dict(ppg_volume=["kind", "channels", "value", "res", "aabb_min", "aabb_max", "to_world", "_reserved", "data"],
                  ppg_medium_volumes=["medium", "density", "albedo", "scale", "_reserved"],
                  ppg_media_volumes=["n_volumes", "n_entries", "volumes", "entries", "_reserved"],
                  ppg_debug_volume_item=["volume", "p"], ppg_debug_volume_out=["value"],
                  ppg_debug_hetmedium_item=["medium", "o", "d", "maxt", "key", "dim"],
                  ppg_debug_hetmedium_out=["success", "t", "sigma_s", "transmittance", "draws", "eval_transmittance", "eval_draws"])
    mirrors = dict(ppg_volume=B.Volume, ppg_medium_volumes=B.MediumVolumes, ppg_media_volumes=B.MediaVolumes, ppg_debug_volume_item=B.DebugVolumeItem,
                   ppg_debug_volume_out=B.DebugVolumeOut, ppg_debug_hetmedium_item=B.DebugHetmediumItem, ppg_debug_hetmedium_out=B.DebugHetmediumOut)
    body = ""
    for name, names in fields.items():
        t = name if not name.startswith("ppg_debug") else "struct " + name
        body += 'printf("%%zu", sizeof(%s));\n' % t + "".join('printf(" %%zu", offsetof(%s, %s));\n' % (t, n) for n in names) + 'printf("\\n");\n'
    body += 'printf("%d %d %d %d\\n", PPG_VOLUME_CONST, PPG_VOLUME_GRID, (int)PPG_HETMEDIUM_MAX_MEAN_STEPS, (int)sizeof(ppg_medium));\n'
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppg.h"\n#include "ppg_testhooks.h"\nint main(void) {\n' + body + 'return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    lines = [[int(v) for v in line.split()] for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]
    for (name, names), got in zip(fields.items(), lines):
        cls = mirrors[name]
        assert got == [C.sizeof(cls)] + [getattr(cls, n).offset for n in names], name
    assert [l[0] for l in lines[:7]] == [136, 32, 40, 16, 12, 40, 36]
    assert lines[0][1:] == [0, 4, 8, 20, 32, 44, 56, 120, 128] and lines[2][1:] == [0, 4, 8, 16, 24]  # as the header documents them
    assert lines[7] == [B.Volume.CONST, B.Volume.GRID, 4096, 64]  # (ppg_medium stays as it was)
    assert B.DEBUG_VOLUME_ITEM_DTYPE.itemsize == 16 == R.LOOKUP_ITEM_DTYPE.itemsize and B.DEBUG_VOLUME_OUT_DTYPE.itemsize == 12
    assert B.DEBUG_HETMEDIUM_ITEM_DTYPE == R.TRACK_ITEM_DTYPE and B.DEBUG_HETMEDIUM_ITEM_DTYPE.itemsize == 40 and B.DEBUG_HETMEDIUM_OUT_DTYPE.itemsize == 36


def test_medium_dicts_flatten_into_the_side_list():
    grid = dict(data=_grid(1), min=(0, 0, 0), max=(1, 2, 3), to_world=R.SKEW_TO_WORLD)
    media = [dict(sigma_a=1.0, sigma_s=1.0), dict(type="heterogeneous", density=grid, albedo=dict(value=0.5), scale=3.0),
             dict(type="heterogeneous", density=grid, albedo=dict(data=_grid(3), min=(0, 0, 0), max=(1, 1, 1)))]
    volumes, entries, keep = B.flatten_media_volumes(media)
    assert [(e.medium, e.density, e.albedo, e.scale) for e in entries] == [(1, 0, 1, 3.0), (2, 0, 2, 1.0)] and len(volumes) == 3  # (the shared grid is one volume)
    v = volumes[0]
    assert (v.kind, v.channels, list(v.res), list(v.aabb_max)) == (1, 1, [5, 4, 3], [1.0, 2.0, 3.0]) and np.allclose(np.asarray(v.to_world[:]).reshape(4, 4), R.SKEW_TO_WORLD)
    assert np.array_equal(np.ctypeslib.as_array(v.data, (60,)), _grid(1).reshape(-1))
    assert list(volumes[1].value) == [0.5, 0.5, 0.5] and volumes[1].channels == 3 and list(volumes[2].to_world) == list(np.eye(4).reshape(-1))
    assert B.flatten_media_volumes([dict(sigma_a=1.0, sigma_s=1.0)])[:2] == ([], [])
    for bad, message in ((dict(type="heterogeneous", density=dict(value=0.5), albedo=dict(value=0.5), sigma_a=1.0), "'sigma_a' belongs to homogeneous media"),
                         (dict(type="heterogeneous", albedo=dict(value=0.5)), "state `density` and `albedo` volumes")):
        with pytest.raises(ValueError, match=message):
            B.Medium.from_dict(bad)
    with pytest.raises(ValueError, match="a const density takes one number"):
        B.flatten_media_volumes([dict(type="heterogeneous", density=dict(value=(0.1, 0.2, 0.3)), albedo=dict(value=0.5))])


def test_the_oracle_library_and_the_scene_writers_refuse_heterogeneous_media(oracle_lib, tmp_path):
    from conftest import ORACLE_SO
    desc = ppg_host.cbox_scene(8, 8)
    desc.media, desc.camera_medium = [dict(type="heterogeneous", density=dict(value=0.5), albedo=dict(value=0.5))], 1
    e = ppg_host.Engine(ORACLE_SO, "ppgo_", budgetType="spp", budget=4)
    with pytest.raises(NotImplementedError, match="ppgo_: participating media are not implemented here"):
        e.set_scene(desc)
    with pytest.raises(NotImplementedError, match="participating media"):
        e.set_media_volumes([], [])
    e.close()
    with pytest.raises(NotImplementedError, match=r"save_scene: participating media"):
        ppg_host.save_scene(desc, str(tmp_path / "het.ppgs"))
    with pytest.raises(NotImplementedError, match="save_scene_xml: participating media"):
        ppg_host.save_scene_xml(desc, {}, str(tmp_path))


# ------------------------------------------------------------------------------------------------ 4. the build stage
def test_ppg_set_scene_validation_and_tables_through_the_host_build_stage(tmp_path):
    """tests/hetmedia_build_check.hip: buildScene() without a context or a device, its host code under the address and undefined-behaviour
    sanitizers, as a child process"""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail("hipcc not found (set HIPCC)")
    exe = str(tmp_path / "hetmedia_build_check")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "hetmedia_build_check.hip")])
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)
    print(run.stdout)
    print(run.stderr)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "all checks passed" in run.stdout and "FAILED" not in run.stdout
    assert run.stdout.count("ok refused") == 34 and run.stdout.count("ok ") == 50
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
