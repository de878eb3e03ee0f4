"""Point, spot and directional emitters (include/ppg.h ppg_set_delta_emitters; mitsuba/src/emitters/point.cpp, spot.cpp, directional.cpp),
the parts that need no GPU: both scene loaders, their agreement field for field, their errors, and the .ppgs block that carries the list."""
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

f32 = np.float32
EXE = os.path.join(ROOT, "practical-path-guiding_amd", "bin", "ppg_render")

SCENE = """<?xml version="1.0"?>
<scene version="0.5.0">
  <integrator type="guided_path"> <string name="budgetType" value="spp"/> <float name="budget" value="4"/> %s </integrator>
  <sensor type="perspective">
    <float name="fov" value="40"/>
    <transform name="toWorld"> <lookAt origin="1, 2, -5" target="0, 0, 0" up="0, 1, 0"/> </transform>
    <film type="hdrfilm"> <integer name="width" value="33"/> <integer name="height" value="21"/> <rfilter type="box"/> </film>
  </sensor>
  %s
  <shape type="rectangle"> <bsdf type="diffuse"/> </shape>
</scene>
"""
NEE = '<string name="nee" value="always"/>'
SPOT_XF = '<transform name="toWorld"> <lookAt origin="1, 4, 2" target="0.5, 0, 1" up="0, 0, 1"/> </transform>'
DIR_XF = '<transform name="toWorld"> <rotate x="1" angle="150"/> <rotate y="1" angle="20"/> </transform>'

# every accepted form, each with more than one light so that the order shows
GOOD = {
    "point_position": '<emitter type="point"> <point name="position" x="0.1" y="2.5" z="-3"/> <rgb name="intensity" value="1, 2, 3"/> </emitter>',
    "point_toworld": '<emitter type="point"> <transform name="toWorld"> <rotate y="1" angle="30"/> <translate x="0.1" y="2.5" z="-3"/> </transform> </emitter>',
    "spot": '<emitter type="spot"> %s <float name="cutoffAngle" value="25"/> <float name="beamWidth" value="15"/> <spectrum name="intensity" value="7"/> </emitter>' % SPOT_XF,
    "spot_defaults": '<emitter type="spot"/> <emitter type="spot"> <float name="cutoffAngle" value="33"/> </emitter>',
    "directional_direction": '<emitter type="directional"> <vector name="direction" x="1" y="-2" z="0.5"/> <rgb name="irradiance" value="3, 2, 1"/> </emitter>',
    "directional_toworld": '<emitter type="directional"> %s </emitter>' % DIR_XF,
    "mixed": '<emitter type="directional"/> <emitter type="point"> <point name="position" x="1" y="1" z="1"/> </emitter> <emitter type="spot"> %s </emitter>'
             '<emitter type="constant"> <rgb name="radiance" value="0.25"/> </emitter>' % SPOT_XF,
}
# (emitters, the word the message must hold)
BAD = {
    "point_position_and_toworld": ('<emitter type="point"> <point name="position" x="0" y="1" z="0"/> <transform name="toWorld"> <translate x="1"/> </transform> </emitter>', "position"),
    "directional_direction_and_toworld": ('<emitter type="directional"> <vector name="direction" x="0" y="-1" z="0"/> %s </emitter>' % DIR_XF, "direction"),
    "directional_scaled": ('<emitter type="directional"> <transform name="toWorld"> <scale value="2"/> </transform> </emitter>', "scale"),
    "spot_cutoff_below_beam": ('<emitter type="spot"> <float name="cutoffAngle" value="10"/> <float name="beamWidth" value="15"/> </emitter>', "cutoffAngle"),
    "spot_texture_property": ('<emitter type="spot"> <rgb name="texture" value="1, 0, 0"/> </emitter>', "texture"),
    "spot_texture_child": ('<emitter type="spot"> <texture type="bitmap" name="texture"> <string name="filename" value="x.png"/> </texture> </emitter>', "texture"),
    "sampling_weight": ('<emitter type="point"> <float name="samplingWeight" value="2"/> </emitter>', "samplingWeight"),
    "collimated": ('<emitter type="collimated"/>', "collimated"),
}


def _write(tmp_path, emitters, integrator=NEE):
    p = tmp_path / "s.xml"
    p.write_text(SCENE % (integrator, emitters))
    return str(p)


def _load(tmp_path, emitters, integrator=NEE, **kw):
    from ppg_host import load_scene
    return load_scene(_write(tmp_path, emitters, integrator), **kw)


def _rad(deg):
    """degToRad (util.h:297) in the reference's float arithmetic"""
    return float(f32(f32(deg) * f32(f32(math.pi) / f32(180))))


def test_point_takes_position_or_the_translation_of_toworld(tmp_path):
    desc, _, info = _load(tmp_path, GOOD["point_position"] + GOOD["point_toworld"])
    a, b = desc.delta_emitters
    assert a == dict(type="point", intensity=(1.0, 2.0, 3.0), position=(float(f32(0.1)), 2.5, -3.0))
    assert b == dict(type="point", intensity=(1.0, 1.0, 1.0), position=(float(f32(0.1)), 2.5, -3.0))  # default intensity: the loaders' D65 (area's default radiance)
    assert not any("next-event" in w for w in info["warnings"])
    assert desc.emitters == [] and desc.environment is None


def test_spot_takes_its_frame_from_toworld_and_its_angles_in_degrees(tmp_path):
    desc, _, _ = _load(tmp_path, GOOD["spot"])
    (s,) = desc.delta_emitters
    assert s["type"] == "spot" and s["position"] == (1.0, 4.0, 2.0)
    assert s["cutoff_angle"] == _rad(25) and s["beam_width"] == _rad(15)
    assert np.allclose(s["intensity"], 7.0)
    R = np.asarray(s["to_local"]).reshape(3, 3)
    axis = np.array([0.5, 0, 1.0]) - np.array([1.0, 4, 2])
    axis /= np.linalg.norm(axis)
    assert np.allclose(R @ axis, (0, 0, 1), atol=1e-6)            # the world-to-light rotation takes the axis to +z
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-6)


def test_spot_defaults(tmp_path):
    """spot.cpp:68-74: intensity 1, cutoffAngle 20, beamWidth = 3/4 of the cutoff angle; identity frame: the axis is +z"""
    desc, _, _ = _load(tmp_path, GOOD["spot_defaults"])
    a, b = desc.delta_emitters
    assert a["intensity"] == (1.0, 1.0, 1.0) and a["position"] == (0.0, 0.0, 0.0)
    assert a["cutoff_angle"] == _rad(20) and a["beam_width"] == _rad(15)
    assert a["to_local"] == [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    assert b["cutoff_angle"] == _rad(33) and b["beam_width"] == _rad(f32(33) * f32(3) / f32(4))


def test_directional_takes_direction_or_the_z_axis_of_toworld(tmp_path):
    desc, _, _ = _load(tmp_path, GOOD["directional_direction"] + GOOD["directional_toworld"])
    a, b = desc.delta_emitters
    assert a["type"] == "directional" and a["intensity"] == (3.0, 2.0, 1.0)
    assert np.allclose(a["direction"], np.array([1, -2, 0.5]) / math.sqrt(5.25), atol=1e-7)
    assert b["intensity"] == (1.0, 1.0, 1.0)
    cx, sx, cy, sy = math.cos(math.radians(150)), math.sin(math.radians(150)), math.cos(math.radians(20)), math.sin(math.radians(20))
    assert np.allclose(b["direction"], (sy * cx, -sx, cy * cx), atol=1e-6)  # Ry(20) Rx(150) (0, 0, 1)
    assert abs(np.linalg.norm(b["direction"]) - 1) < 1e-6


def test_order_is_kept_and_the_environment_emitter_stays_what_it_is(tmp_path):
    desc, _, _ = _load(tmp_path, GOOD["mixed"])
    assert [e["type"] for e in desc.delta_emitters] == ["directional", "point", "spot"]
    assert desc.delta_emitters[0]["direction"] == (0.0, 0.0, 1.0)
    assert np.allclose(desc.environment, 0.25)


@pytest.mark.parametrize("case", sorted(BAD))
def test_python_loader_refuses(tmp_path, case):
    from ppg_host.mitsuba_xml import SceneError
    emitters, word = BAD[case]
    with pytest.raises(SceneError, match=word):
        _load(tmp_path, emitters)


def test_unsupported_emitter_error_names_the_new_types(tmp_path):
    from ppg_host.mitsuba_xml import SceneError
    with pytest.raises(SceneError, match="`point`, `spot` and `directional`"):
        _load(tmp_path, BAD["collimated"][0])


def test_lenient_still_skips_a_collimated(tmp_path):
    desc, _, info = _load(tmp_path, BAD["collimated"][0] + GOOD["point_position"], strict=False)
    assert len(desc.delta_emitters) == 1
    assert any("collimated" in w and "skipped" in w for w in info["warnings"])


@pytest.mark.parametrize("integrator", ["", '<string name="nee" value="kickstart"/>', '<string name="nee" value="never"/>'])
def test_warning_when_nee_is_not_always(tmp_path, integrator):
    _, _, info = _load(tmp_path, GOOD["point_position"], integrator)
    assert any("next-event estimation only" in w for w in info["warnings"])
    _, _, info = _load(tmp_path, "", integrator)  # no such lights: no warning
    assert not any("next-event estimation only" in w for w in info["warnings"])


def test_scene_file_round_trip_keeps_the_list(tmp_path):
    import ppg_host
    from ppg_host.scenes import load_scene_file, save_scene
    lights, _, _ = _load(tmp_path, GOOD["mixed"] + GOOD["spot"] + GOOD["directional_toworld"])
    desc = ppg_host.cbox_scene(16, 12)
    desc.delta_emitters = lights.delta_emitters
    p = tmp_path / "l.ppgs"
    save_scene(desc, str(p))
    back = load_scene_file(str(p))
    assert back.delta_emitters == lights.delta_emitters and len(back.delta_emitters) == 5
    raw = p.read_bytes()
    assert np.frombuffer(raw[24:28], np.uint32)[0] & 256
    golden = open(os.path.join(GOLDEN, "cbox_16x12_pinhole.ppgs"), "rb").read()
    assert len(raw) == len(golden) + 4 + 5 * 84 and raw[28:len(golden)] == golden[28:]  # the block is appended: uint32 n, n x 84 bytes
    assert np.frombuffer(raw[len(golden):len(golden) + 4], np.uint32)[0] == 5


def test_scene_file_without_such_lights_is_unchanged(tmp_path):
    """bit 8 clear and the bytes the format had before (a fixture written by an earlier version), with an empty list and with a description
    from before the list existed"""
    import ppg_host
    from ppg_host.scenes import load_scene_file, save_scene
    golden = open(os.path.join(GOLDEN, "cbox_16x12_pinhole.ppgs"), "rb").read()
    desc = ppg_host.cbox_scene(16, 12)
    p = tmp_path / "p.ppgs"
    save_scene(desc, str(p))
    assert p.read_bytes() == golden
    assert load_scene_file(str(p)).delta_emitters == []
    del desc.delta_emitters
    save_scene(desc, str(p))
    assert p.read_bytes() == golden


def test_binding_struct_is_the_header_struct():
    from ppg_host.bindings import C, DeltaEmitter
    from ppg_host.scenes import C_DELTA_EMITTER_BYTES
    assert C.sizeof(DeltaEmitter) == C_DELTA_EMITTER_BYTES == 84
    hdr = open(os.path.join(ROOT, "include", "ppg.h")).read()
    body = hdr[hdr.index("typedef struct ppg_delta_emitter {"):hdr.index("} ppg_delta_emitter;")]
    import re
    names = re.findall(r"\b(type|intensity|position|to_local|direction|cutoff_angle|beam_width)\b(?=\[|,|;)", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [n for n, _ in DeltaEmitter._fields_]
    with pytest.raises(ValueError, match="unknown type"):
        DeltaEmitter.from_dict(dict(type="collimated", intensity=(1, 1, 1)))
    with pytest.raises(ValueError, match="unknown parameters"):
        DeltaEmitter.from_dict(dict(type="point", intensity=(1, 1, 1), radius=1))


def test_xml_writer_round_trips_the_list(tmp_path):
    import ppg_host
    from ppg_host.mitsuba_xml import save_scene_xml
    lights, _, _ = _load(tmp_path, GOOD["mixed"])
    desc = ppg_host.cbox_scene(16, 12)
    desc.delta_emitters = lights.delta_emitters
    back, _, _ = ppg_host.load_scene(save_scene_xml(desc, dict(budgetType="spp", budget=4, nee="always"), str(tmp_path)))
    assert [e["type"] for e in back.delta_emitters] == ["directional", "point", "spot"]
    for a, b in zip(back.delta_emitters, lights.delta_emitters):
        assert set(a) == set(b)
        for k in a:
            if k != "type":
                assert np.allclose(a[k], b[k], rtol=1e-6, atol=1e-6), k


# ---------------------------------------------------------------------------------------------- the C++ loader, through ppg_render's conversion
@pytest.mark.parametrize("case", sorted(GOOD))
def test_cpp_loader_equals_the_python_loader(hip_lib_path, tmp_path, case):
    from ppg_host.scenes import load_scene_file
    desc, _, _ = _load(tmp_path, GOOD[case])
    cpp = tmp_path / "cpp.ppgs"
    r = subprocess.run([EXE, str(tmp_path / "s.xml"), "--ppgs", str(cpp)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    c = load_scene_file(str(cpp))
    assert len(desc.delta_emitters) >= 1 and c.delta_emitters == desc.delta_emitters  # field for field, to the bit
    assert c.environment == desc.environment
    assert "next-event estimation only" not in r.stderr + r.stdout


@pytest.mark.parametrize("case", sorted(BAD))
def test_cpp_loader_refuses_what_the_python_loader_refuses(hip_lib_path, tmp_path, case):
    emitters, word = BAD[case]
    r = subprocess.run([EXE, _write(tmp_path, emitters), "--ppgs", str(tmp_path / "x.ppgs")], capture_output=True, text=True)
    assert r.returncode != 0 and word in r.stderr, r.stderr


def test_cpp_loader_lenient_and_warning(hip_lib_path, tmp_path):
    from ppg_host.scenes import load_scene_file
    xml = _write(tmp_path, BAD["collimated"][0] + GOOD["point_position"], '<string name="nee" value="kickstart"/>')
    cpp = tmp_path / "cpp.ppgs"
    r = subprocess.run([EXE, xml, "--lenient", "--ppgs", str(cpp)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert len(load_scene_file(str(cpp)).delta_emitters) == 1
    out = r.stderr + r.stdout
    assert "collimated" in out and "skipped" in out and "next-event estimation only" in out
    r = subprocess.run([EXE, xml, "--ppgs", str(cpp)], capture_output=True, text=True)
    assert r.returncode != 0 and "`point`, `spot` and `directional`" in r.stderr
