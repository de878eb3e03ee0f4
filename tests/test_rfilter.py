"""Film reconstruction filters other than box (include/ppg.h ppg_set_rfilter), the parts that need no GPU: the discretised filter table
against a numpy restatement of ReconstructionFilter::configure (mitsuba/src/libcore/rfilter.cpp:37-55, src/rfilters/*.cpp), both scene
loaders, and the .ppgs block that carries the filter."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

f32 = np.float32
EXE = os.path.join(ROOT, "practical-path-guiding_amd", "bin", "ppg_render")


def np_eval(d, x):
    """eval(x) of the Mitsuba filter `d`, float32 (the Gaussian's exp and Lanczos' pi * x in double, as there)"""
    t = d["type"]
    x = f32(x)
    if t == "box":
        r = f32(d.get("radius", 0.5)) + f32(1e-5)
        return f32(1) if abs(x) <= r else f32(0)
    if t == "tent":
        return max(f32(0), f32(1) - abs(x / f32(1)))
    if t == "gaussian":
        s = f32(d.get("stddev", 0.5))
        r = f32(4) * s
        alpha = f32(-1) / (f32(2) * s * s)
        return max(f32(0), f32(np.exp(np.float64(alpha * x * x))) - f32(np.exp(np.float64(alpha * r * r))))
    if t in ("mitchell", "catmullrom"):
        B, C = (f32(d.get("B", 1 / 3)), f32(d.get("C", 1 / 3))) if t == "mitchell" else (f32(0), f32(0.5))
        x = abs(x)
        x2 = x * x
        x3 = x2 * x
        if x < 1:
            return f32(1) / f32(6) * ((f32(12) - f32(9) * B - f32(6) * C) * x3 + (f32(-18) + f32(12) * B + f32(6) * C) * x2 + (f32(6) - f32(2) * B))
        if x < 2:
            return f32(1) / f32(6) * ((-B - f32(6) * C) * x3 + (f32(6) * B + f32(30) * C) * x2 + (f32(-12) * B - f32(48) * C) * x + (f32(8) * B + f32(24) * C))
        return f32(0)
    r = f32(d.get("lobes", 3))
    x = abs(x)
    if x < f32(1e-4):
        return f32(1)
    if x > r:
        return f32(0)
    x1 = f32(np.pi * np.float64(x))
    x2 = x1 / r
    sin = lambda v: f32(np.sin(np.float64(v)))  # (sinf: correctly rounded)
    return (sin(x1) * sin(x2)) / (x1 * x2)


def np_radius(d):
    t = d["type"]
    return {"box": lambda: f32(d.get("radius", 0.5)) + f32(1e-5), "tent": lambda: f32(1), "gaussian": lambda: f32(4) * f32(d.get("stddev", 0.5)),
            "mitchell": lambda: f32(2), "catmullrom": lambda: f32(2), "lanczos": lambda: f32(d.get("lobes", 3))}[t]()


def np_table(d):
    r = np_radius(d)
    vals = np.zeros(32, f32)
    s = f32(0)
    for i in range(31):
        vals[i] = np_eval(d, (r * f32(i)) / f32(31))
        s = f32(s + vals[i])
    s = f32(s * (f32(2) * r / f32(31)))
    norm = f32(1) / s
    vals[:31] = vals[:31] * norm
    return vals, r, int(np.ceil(r - f32(0.5)))


FILTERS = [{"type": "box", "radius": 1.5}, {"type": "box", "radius": 0.3}, {"type": "tent"}, {"type": "gaussian"}, {"type": "gaussian", "stddev": 0.3},
           {"type": "gaussian", "stddev": 0.8}, {"type": "mitchell"}, {"type": "mitchell", "B": 0.0, "C": 0.5}, {"type": "catmullrom"},
           {"type": "lanczos"}, {"type": "lanczos", "lobes": 2}]


@pytest.mark.parametrize("d", FILTERS, ids=lambda d: "-".join(str(v) for v in d.values()))
def test_table_matches_numpy_restatement(hip_lib_path, d):
    import ppg_host.bindings as b
    table, r, border = b.rfilter_table(d)
    want, r_want, border_want = np_table(d)
    assert r == r_want and border == border_want
    ulp = np.spacing(np.maximum(np.abs(want), np.abs(table)))
    assert (np.abs(table - want) <= ulp).all(), (table, want)
    assert table[31] == 0
    if d["type"] in ("mitchell", "catmullrom", "lanczos"):
        assert (table < 0).any()  # the negative lobes are in the table


def test_default_box_and_bad_filters(hip_lib_path):
    import ppg_host.bindings as b
    table, r, border = b.rfilter_table(None)
    assert r == f32(0.5) + f32(1e-5) and border == 1 and np.allclose(table[:31], table[0])
    for bad in ({"type": "lanczos", "lobes": 4}, {"type": "gaussian", "stddev": 0.9}, {"type": "box", "radius": 3.6}, {"type": "box", "radius": 0.0},
                {"type": "gaussian", "stddev": -1.0}, {"type": "lanczos", "lobes": 0}):
        with pytest.raises(b.PPGError):
            b.rfilter_table(bad)
    with pytest.raises(ValueError):
        b.RFilter.from_dict({"type": "blackman"})
    with pytest.raises(ValueError):
        b.RFilter.from_dict({"type": "tent", "radius": 2.0})


SCENE = """<?xml version="1.0"?>
<scene version="0.5.0">
  <integrator type="guided_path"> <string name="budgetType" value="spp"/> <float name="budget" value="4"/> </integrator>
  <sensor type="perspective">
    <float name="fov" value="45"/>
    <transform name="toWorld"> <lookAt origin="0, 0, -5" target="0, 0, 0" up="0, 1, 0"/> </transform>
    <film type="hdrfilm"> <integer name="width" value="33"/> <integer name="height" value="21"/> %s </film>
  </sensor>
  <shape type="rectangle"> <bsdf type="diffuse"/> <emitter type="area"> <rgb name="radiance" value="1, 2, 3"/> </emitter> </shape>
</scene>
"""

XML_CASES = [('<rfilter type="box"/>', None),
             ('<rfilter type="box"> <float name="radius" value="0.5"/> </rfilter>', None),
             ('<rfilter type="box"> <float name="radius" value="1.5"/> </rfilter>', {"type": "box", "radius": 1.5}),
             ('<rfilter type="tent"/>', {"type": "tent"}),
             ('<rfilter type="gaussian"/>', {"type": "gaussian", "stddev": 0.5}),
             ('<rfilter type="gaussian"> <float name="stddev" value="0.3"/> </rfilter>', {"type": "gaussian", "stddev": float(f32(0.3))}),
             ('<rfilter type="mitchell"/>', {"type": "mitchell", "B": float(f32(1 / 3)), "C": float(f32(1 / 3))}),
             ('<rfilter type="mitchell"> <float name="B" value="0"/> <float name="C" value="0.5"/> </rfilter>', {"type": "mitchell", "B": 0.0, "C": 0.5}),
             ('<rfilter type="catmullrom"/>', {"type": "catmullrom"}),
             ('<rfilter type="lanczos"/>', {"type": "lanczos", "lobes": 3}),
             ('<rfilter type="lanczos"> <integer name="lobes" value="2"/> </rfilter>', {"type": "lanczos", "lobes": 2})]


@pytest.mark.parametrize("xml,want", XML_CASES, ids=[str(i) for i in range(len(XML_CASES))])
def test_both_loaders_parse_the_filter(hip_lib_path, tmp_path, xml, want):
    from ppg_host import load_scene
    from ppg_host.scenes import load_scene_file, save_scene
    p = tmp_path / "s.xml"
    p.write_text(SCENE % xml)
    desc, _, info = load_scene(str(p))
    assert desc.rfilter == want
    assert not any("rfilter" in w for w in info["warnings"])
    # .ppgs: written by the Python side and by the C++ loader (ppg_render --ppgs), read back by both
    py, cpp = tmp_path / "py.ppgs", tmp_path / "cpp.ppgs"
    save_scene(desc, str(py))
    subprocess.run([EXE, str(p), "--ppgs", str(cpp)], check=True, capture_output=True)
    for f in (py, cpp):
        assert load_scene_file(str(f)).rfilter == want
        blocks = np.frombuffer(f.read_bytes()[24:28], np.uint32)[0]
        assert bool(blocks & 64) == (want is not None)
    if want is not None:
        assert py.read_bytes()[-24:] == cpp.read_bytes()[-24:]  # the same ppg_rfilter block


def test_box_scene_file_is_unchanged(hip_lib_path, tmp_path):
    """a box-filtered scene writes no bit 6: its bytes are those of a scene without any filter block"""
    from ppg_host import load_scene
    from ppg_host.scenes import save_scene
    p = tmp_path / "s.xml"
    p.write_text(SCENE % '<rfilter type="box"/>')
    desc, _, _ = load_scene(str(p))
    a, b = tmp_path / "a.ppgs", tmp_path / "b.ppgs"
    save_scene(desc, str(a))
    desc.rfilter = {"type": "gaussian"}
    save_scene(desc, str(b))
    assert len(b.read_bytes()) == len(a.read_bytes()) + 24 and b.read_bytes()[:24] == a.read_bytes()[:24]
    del desc.rfilter  # a description from before the filter existed
    save_scene(desc, str(b))
    assert a.read_bytes() == b.read_bytes()


@pytest.mark.parametrize("xml", ['<rfilter type="blackman"/>', '<rfilter type="gaussian"> <float name="radius" value="2"/> </rfilter>',
                                 '<rfilter type="gaussian"> <float name="stddev" value="-1"/> </rfilter>',
                                 '<rfilter type="lanczos"> <integer name="lobes" value="5"/> </rfilter>',
                                 '<rfilter type="box"> <float name="radius" value="abc"/> </rfilter>'])
def test_both_loaders_refuse_bad_filters(hip_lib_path, tmp_path, xml):
    from ppg_host import load_scene
    from ppg_host.mitsuba_xml import SceneError
    p = tmp_path / "s.xml"
    p.write_text(SCENE % xml)
    with pytest.raises(SceneError):
        load_scene(str(p))
    r = subprocess.run([EXE, str(p), "--ppgs", str(tmp_path / "x.ppgs")], capture_output=True, text=True)
    assert r.returncode != 0 and "rfilter" in r.stderr


def test_missing_rfilter_keeps_box_with_warning(hip_lib_path, tmp_path):
    from ppg_host import load_scene
    p = tmp_path / "s.xml"
    p.write_text(SCENE % "")
    desc, _, info = load_scene(str(p))
    assert desc.rfilter is None and any("no <rfilter>" in w for w in info["warnings"])


def test_sharded_render_refuses_a_filtered_scene():
    from ppg_host.distributed import check_shardable
    from ppg_host.scenes import cbox_scene
    s = cbox_scene(8, 8)
    check_shardable(s)
    s.rfilter = {"type": "gaussian"}
    with pytest.raises(ValueError, match="sharded filtered renders are not supported yet"):
        check_shardable(s)
