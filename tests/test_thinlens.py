"""Thin-lens camera and focalLength (include/ppg.h ppg_set_lens; mitsuba/src/sensors/thinlens.cpp, librender/sensor.cpp), the parts that
need no GPU: both scene loaders, their agreement, and the .ppgs block that carries the lens."""
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
  <integrator type="guided_path"> <string name="budgetType" value="spp"/> <float name="budget" value="4"/> </integrator>
  <sensor type="%s">
    %s
    <transform name="toWorld"> %s </transform>
    <film type="hdrfilm"> <integer name="width" value="33"/> <integer name="height" value="21"/> <rfilter type="box"/> </film>
  </sensor>
  <shape type="rectangle"> <bsdf type="diffuse"/> <emitter type="area"> <rgb name="radiance" value="1, 2, 3"/> </emitter> </shape>
</scene>
"""
LOOKAT = '<lookAt origin="1, 2, -5" target="0, 0, 0" up="0, 1, 0"/>'


def _load(tmp_path, sensor, body, xf=LOOKAT):
    from ppg_host import load_scene
    p = tmp_path / "s.xml"
    p.write_text(SCENE % (sensor, body, xf))
    return load_scene(str(p)), str(p)


def _same_camera(a, b):
    for k in ("sample_to_camera", "camera_to_world"):
        assert np.array_equal(np.asarray(a[k], f32), np.asarray(b[k], f32)), k
    assert (f32(a["near_clip"]), f32(a["far_clip"]), a["width"], a["height"]) == (f32(b["near_clip"]), f32(b["far_clip"]), b["width"], b["height"])


def test_thinlens_sensor_gives_lens_and_the_perspective_camera(tmp_path):
    (desc, _, info), _ = _load(tmp_path, "thinlens", '<float name="fov" value="40"/> <float name="apertureRadius" value="0.2"/> '
                                                     '<float name="focusDistance" value="4.5"/> <float name="farClip" value="100"/>')
    assert desc.lens == dict(aperture_radius=float(f32(0.2)), focus_distance=4.5)
    (pin, _, _), _ = _load(tmp_path, "perspective", '<float name="fov" value="40"/> <float name="farClip" value="100"/>')
    assert pin.lens is None
    _same_camera(desc.camera, pin.camera)
    assert not any("thinlens" in w for w in info["warnings"])


def test_thinlens_needs_an_aperture_radius(tmp_path):
    from ppg_host.mitsuba_xml import SceneError
    with pytest.raises(SceneError, match="apertureRadius"):
        _load(tmp_path, "thinlens", '<float name="fov" value="40"/>')


def test_zero_aperture_becomes_epsilon_with_a_warning(tmp_path):
    (desc, _, info), _ = _load(tmp_path, "thinlens", '<float name="fov" value="40"/> <float name="apertureRadius" value="0"/> '
                                                     '<float name="focusDistance" value="2"/>')
    assert desc.lens["aperture_radius"] == float(f32(1e-4))
    assert any("zero aperture radius" in w for w in info["warnings"])


def test_focus_distance_defaults_to_far_clip(tmp_path):
    (desc, _, _), _ = _load(tmp_path, "thinlens", '<float name="fov" value="40"/> <float name="apertureRadius" value="0.1"/> '
                                                  '<float name="farClip" value="250"/>')
    assert desc.lens["focus_distance"] == 250.0
    (desc, _, _), _ = _load(tmp_path, "thinlens", '<float name="fov" value="40"/> <float name="apertureRadius" value="0.1"/>')
    assert desc.lens["focus_distance"] == 1e4


def test_scale_in_the_lens_transform_is_refused(tmp_path):
    from ppg_host.mitsuba_xml import SceneError
    with pytest.raises(SceneError, match="scale"):
        _load(tmp_path, "thinlens", '<float name="fov" value="40"/> <float name="apertureRadius" value="0.1"/>', '<scale value="2"/>' + LOOKAT)
    (desc, _, _), _ = _load(tmp_path, "perspective", '<float name="fov" value="40"/>', '<scale value="2"/>' + LOOKAT)  # (the pinhole takes one)
    assert desc.lens is None


def _dfov(mm):
    """sensor.cpp:264-276 restated: 2 * 180/pi * atan(sqrt(36^2 + 24^2) / (2 mm)), float32 where the reference is"""
    a = f32(np.arctan(f32(np.sqrt(f32(1872))) / (f32(2) * f32(mm))))
    return float(f32(2 * 180 / math.pi * float(a)))


@pytest.mark.parametrize("sensor", ["perspective", "thinlens"])
def test_focal_length_is_the_equivalent_diagonal_fov(tmp_path, sensor):
    lens = '<float name="apertureRadius" value="0.1"/>' if sensor == "thinlens" else ""
    (a, _, _), _ = _load(tmp_path, sensor, '<string name="focalLength" value="35mm"/>' + lens)
    assert abs(_dfov(35) - 2 * math.degrees(math.atan(math.sqrt(36 ** 2 + 24 ** 2) / 70))) < 1e-4
    (b, _, _), _ = _load(tmp_path, sensor, '<float name="fov" value="%r"/> <string name="fovAxis" value="diagonal"/>' % _dfov(35) + lens)
    _same_camera(a.camera, b.camera)
    # neither fov nor focalLength: 50mm
    (c, _, _), _ = _load(tmp_path, sensor, lens)
    (d, _, _), _ = _load(tmp_path, sensor, '<float name="fov" value="%r"/> <string name="fovAxis" value="diagonal"/>' % _dfov(50) + lens)
    _same_camera(c.camera, d.camera)
    assert not np.array_equal(a.camera["sample_to_camera"], c.camera["sample_to_camera"])


@pytest.mark.parametrize("sensor", ["perspective", "thinlens"])
def test_fov_together_with_focal_length_is_refused(tmp_path, sensor):
    from ppg_host.mitsuba_xml import SceneError
    with pytest.raises(SceneError, match="focalLength"):
        _load(tmp_path, sensor, '<float name="fov" value="40"/> <string name="focalLength" value="35mm"/> <float name="apertureRadius" value="0.1"/>')


def test_other_sensors_are_still_refused(tmp_path):
    from ppg_host.mitsuba_xml import SceneError
    with pytest.raises(SceneError, match="orthographic"):
        _load(tmp_path, "orthographic", "")


def test_scene_file_round_trip_keeps_the_lens(tmp_path):
    import ppg_host
    from ppg_host.scenes import load_scene_file, save_scene
    desc = ppg_host.cbox_scene(16, 12)
    desc.lens = dict(aperture_radius=0.05, focus_distance=3.25)
    p = tmp_path / "l.ppgs"
    save_scene(desc, str(p))
    back = load_scene_file(str(p))
    assert back.lens == dict(aperture_radius=float(f32(0.05)), focus_distance=3.25)
    blocks = np.frombuffer(p.read_bytes()[24:28], np.uint32)[0]
    assert blocks & 128 and p.read_bytes()[-8:] == np.array([0.05, 3.25], f32).tobytes()


def test_scene_file_without_a_lens_is_unchanged(tmp_path):
    """bit 7 clear, and the bytes the format had before the lens existed (a fixture written by the previous version)"""
    import ppg_host
    from ppg_host.scenes import load_scene_file, save_scene
    desc = ppg_host.cbox_scene(16, 12)
    p = tmp_path / "p.ppgs"
    save_scene(desc, str(p))
    assert p.read_bytes() == open(os.path.join(GOLDEN, "cbox_16x12_pinhole.ppgs"), "rb").read()
    assert not np.frombuffer(p.read_bytes()[24:28], np.uint32)[0] & 128
    assert load_scene_file(str(p)).lens is None
    del desc.lens  # a description from before the lens existed
    save_scene(desc, str(p))
    assert p.read_bytes() == open(os.path.join(GOLDEN, "cbox_16x12_pinhole.ppgs"), "rb").read()


def test_xml_writer_round_trips_the_lens(tmp_path):
    import ppg_host
    from ppg_host.mitsuba_xml import save_scene_xml
    desc = ppg_host.cbox_scene(16, 12)
    desc.lens = dict(aperture_radius=0.05, focus_distance=3.25)
    xml = save_scene_xml(desc, dict(budgetType="spp", budget=4), str(tmp_path))
    back, _, _ = ppg_host.load_scene(xml)
    assert back.lens == dict(aperture_radius=float(f32(0.05)), focus_distance=3.25)
    desc.lens = None
    back, _, _ = ppg_host.load_scene(save_scene_xml(desc, dict(budgetType="spp", budget=4), str(tmp_path)))
    assert back.lens is None


@pytest.mark.parametrize("body", ['<float name="fov" value="40"/> <float name="apertureRadius" value="0.2"/> <float name="focusDistance" value="4.5"/>',
                                  '<string name="focalLength" value="35mm"/> <float name="apertureRadius" value="0"/>',
                                  '<float name="apertureRadius" value="0.01"/> <float name="farClip" value="70"/>'])
def test_cpp_loader_equals_the_python_loader_on_a_thinlens(hip_lib_path, tmp_path, body):
    from ppg_host.scenes import load_scene_file
    (desc, _, info), xml = _load(tmp_path, "thinlens", body)
    cpp = tmp_path / "cpp.ppgs"
    r = subprocess.run([EXE, xml, "--ppgs", str(cpp)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    c = load_scene_file(str(cpp))
    assert c.lens == desc.lens
    assert np.allclose(c.camera["sample_to_camera"], desc.camera["sample_to_camera"], rtol=1e-6, atol=1e-6)
    _same_camera(dict(c.camera, sample_to_camera=0), dict(desc.camera, sample_to_camera=0))
    assert ("zero aperture radius" in r.stderr + r.stdout) == any("zero aperture radius" in w for w in info["warnings"])


def test_cpp_loader_equals_the_python_loader_on_a_focal_length(hip_lib_path, tmp_path):
    from ppg_host.scenes import load_scene_file
    (desc, _, _), xml = _load(tmp_path, "perspective", '<string name="focalLength" value="28mm"/>')
    cpp = tmp_path / "cpp.ppgs"
    subprocess.run([EXE, xml, "--ppgs", str(cpp)], check=True, capture_output=True)
    c = load_scene_file(str(cpp))
    assert c.lens is None and desc.lens is None
    assert np.allclose(c.camera["sample_to_camera"], desc.camera["sample_to_camera"], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("body,what", [('<float name="fov" value="40"/>', "apertureRadius"),
                                       ('<float name="fov" value="40"/> <string name="focalLength" value="35mm"/> <float name="apertureRadius" value="0.1"/>', "focalLength"),
                                       ('<float name="fov" value="40"/> <float name="apertureRadius" value="0.1"/>', "scale")])
def test_cpp_loader_refuses_what_the_python_loader_refuses(hip_lib_path, tmp_path, body, what):
    from ppg_host.mitsuba_xml import SceneError
    xf = '<scale value="2"/>' + LOOKAT if what == "scale" else LOOKAT
    with pytest.raises(SceneError):
        _load(tmp_path, "thinlens", body, xf)
    r = subprocess.run([EXE, str(tmp_path / "s.xml"), "--ppgs", str(tmp_path / "x.ppgs")], capture_output=True, text=True)
    assert r.returncode != 0 and what in r.stderr
