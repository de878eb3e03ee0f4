"""Analytic disks and cylinders (ppg_set_shapes), the parts that need no GPU: both scene loaders, the flat scene file, the XML writer, the
refusals and the layout of ppg_shape.  The constructors of Mitsuba's disk and cylinder plug-ins are restated here in float64 numpy."""
import ctypes as C
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT

import ppg_host
from ppg_host import mitsuba_xml
from ppg_host import bindings as b

XML = os.path.join(GOLDEN, "shapes", "shapes.xml")
BIN = os.path.join(PKG, "bin", "ppg_render")


@pytest.fixture(scope="module")
def ppg_render():
    if not os.path.exists(BIN):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "__graft_entry__.py")])
    return BIN


# ---- the transforms of tests/golden/shapes/shapes.xml, in float64 (values as floats, as a loader reads them) ----
def f(v):
    return float(np.float32(v))


def translate(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (f(x), f(y), f(z))
    return m


def scale(x, y=None, z=None):
    y, z = (x, x) if y is None else (y, z)
    return np.diag([f(x), f(y), f(z), 1.0])


def rotate(axis, deg):
    """rotation by `deg` degrees about `axis` (Rodrigues' formula)"""
    a = np.array([f(v) for v in axis])
    a = a / np.linalg.norm(a)
    th = math.radians(f(deg))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    return m


def chain(*ms):
    """elements of a <transform> in document order: later ones are applied after earlier ones"""
    out = np.eye(4)
    for m in ms:
        out = m @ out
    return out


def frame_of(n):
    """an orthonormal frame (s, t, n) as Mitsuba's Frame(n) builds it"""
    if abs(n[0]) > abs(n[1]):
        t = np.array([n[2], 0.0, -n[0]]) / math.hypot(n[0], n[2])
    else:
        t = np.array([0.0, n[2], -n[1]]) / math.hypot(n[1], n[2])
    return np.cross(t, n), t


def cylinder_record(p0, p1, radius, to_world):
    """the cylinder plug-in's constructor: translate(p0) * fromFrame(Frame(axis)) * scale(r, r, len), toWorld in front, scale taken out"""
    p0, p1 = np.array([f(v) for v in p0]), np.array([f(v) for v in p1])
    d = p1 - p0
    length = np.linalg.norm(d)
    s, t = frame_of(d / length)
    fr = np.eye(4)
    fr[:3, 0], fr[:3, 1], fr[:3, 2] = s, t, d / length
    m = to_world @ translate(*p0) @ fr @ scale(radius, radius, length)
    r, ln = np.linalg.norm(m[:3, 0]), np.linalg.norm(m[:3, 2])
    m = m @ np.diag([1 / r, 1 / r, 1 / ln, 1.0])
    return m[:3, :].reshape(-1), r, ln


EXPECTED = [
    dict(type="disk", to_world=chain(scale(0.7), rotate((1, 0.2, 0), 35), rotate((0, 1, 0), -20), translate(0.4, 0.1, 0.6))[:3, :].reshape(-1),
         flip_normals=False, emitter=-1),
    dict(type="disk", to_world=chain(scale(0.35), rotate((1, 0, 0), 90), translate(0, 1.4, 0.2))[:3, :].reshape(-1), flip_normals=True, emitter=0),
    dict(zip(("to_world", "radius", "length"),
             cylinder_record((-0.5, 0.1, 0.2), (0.3, 0.9, -0.1), 0.15, chain(rotate((0.3, 1, 0.1), 50), scale(1.3), translate(-0.2, 0, 0.3)))),
         type="cylinder", flip_normals=False, emitter=-1),
    dict(zip(("to_world", "radius", "length"), cylinder_record((0, 0, 0), (0, 0, 1), 0.05, chain(rotate((0, 0, 1), 30), translate(-0.9, 0.2, 0)))),
         type="cylinder", flip_normals=True, emitter=1),
]


def close(a, b_, rel=1e-6):
    a, b_ = np.asarray(a, np.float64), np.asarray(b_, np.float64)
    return bool(np.all(np.abs(a - b_) <= rel * max(1.0, float(np.abs(b_).max()))))


def same_records(xs, ys):
    assert len(xs) == len(ys)
    for x, y in zip(xs, ys):
        assert bytes(b.Shape.from_dict(x)) == bytes(b.Shape.from_dict(y)), (x, y)


def test_python_loader_records_equal_the_constructors():
    desc, _, _ = ppg_host.load_scene(XML)
    assert len(desc.shapes) == 4 and len(desc.emitters) == 2 and desc.n_triangles == 2
    for got, want in zip(desc.shapes, EXPECTED):
        assert got["type"] == want["type"] and got["flip_normals"] == want["flip_normals"] and got["emitter"] == want["emitter"]
        assert close(got["to_world"], want["to_world"]), (got["to_world"], want["to_world"])
        if want["type"] == "cylinder":
            assert abs(got["radius"] - want["radius"]) <= 1e-6 * want["radius"] and abs(got["length"] - want["length"]) <= 1e-6 * want["length"]
            R = np.asarray(got["to_world"]).reshape(3, 4)[:, :3]
            assert np.allclose(R @ R.T, np.eye(3), atol=1e-6)  # the scale is gone: a rotation is left
    # the emitting shapes carry the all-absorbing BSDF Mitsuba gives a shape under an emitter, the others their own
    assert [desc.materials[s["material"]]["reflectance"] for s in desc.shapes][1] == (0.0, 0.0, 0.0)
    assert desc.emitters[0]["radiance"] == (12.0, 11.0, 9.0) and desc.emitters[1]["radiance"] == (3.0, 4.0, 5.0)


def _shape_block(path):
    """the bytes of a flat scene file's shape block (bit 10: the last block) and the header's block word"""
    buf = open(path, "rb").read()
    blocks = struct.unpack_from("<6I", buf, 4)[5]
    if not blocks & 1024:
        return blocks, b""
    # the block is the file's last one: uint32 n, n x 80 bytes
    for n in range(1, 1 + (len(buf) - 28) // 80):
        off = len(buf) - 4 - 80 * n
        if off >= 28 and struct.unpack_from("<I", buf, off)[0] == n and all(struct.unpack_from("<i", buf, off + 4 + 80 * k)[0] in (0, 1) for k in range(n)):
            return blocks, buf[off:]
    raise AssertionError("no shape block found")


def test_cpp_loader_writes_the_same_shape_block(ppg_render, tmp_path):
    r = subprocess.run([ppg_render, "--ppgs", str(tmp_path / "cpp.ppgs"), "-q", XML], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    desc, _, _ = ppg_host.load_scene(XML)
    ppg_host.save_scene(desc, str(tmp_path / "py.ppgs"))
    (bc, cpp), (bp, py) = _shape_block(str(tmp_path / "cpp.ppgs")), _shape_block(str(tmp_path / "py.ppgs"))
    assert bc & 1024 and bp & 1024 and len(py) == 4 + 80 * 4
    assert cpp == py
    # ... and the C++ reader takes the Python file, shape block included: reading and writing it again leaves the block as it is
    r = subprocess.run([ppg_render, "--ppgs", str(tmp_path / "again.ppgs"), "-q", str(tmp_path / "py.ppgs")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert _shape_block(str(tmp_path / "again.ppgs"))[1] == py
    same_records(ppg_host.load_scene_file(str(tmp_path / "cpp.ppgs")).shapes, desc.shapes)


def test_flat_file_round_trip_and_files_without_the_block(tmp_path):
    desc, _, _ = ppg_host.load_scene(XML)
    p = str(tmp_path / "a.ppgs")
    ppg_host.save_scene(desc, p)
    back = ppg_host.load_scene_file(p)
    same_records(back.shapes, desc.shapes)
    q = str(tmp_path / "b.ppgs")
    ppg_host.save_scene(back, q)
    assert open(p, "rb").read() == open(q, "rb").read()  # lossless
    # a scene without shapes: no bit 10, not a byte more than before, and it loads with an empty list
    plain = ppg_host.cbox_scene(16, 16)
    ppg_host.save_scene(plain, str(tmp_path / "plain.ppgs"))
    buf = open(str(tmp_path / "plain.ppgs"), "rb").read()
    assert not struct.unpack_from("<6I", buf, 4)[5] & 1024
    assert ppg_host.load_scene_file(str(tmp_path / "plain.ppgs")).shapes == []
    desc.shapes = []
    ppg_host.save_scene(desc, str(tmp_path / "none.ppgs"))
    assert len(open(str(tmp_path / "none.ppgs"), "rb").read()) == len(open(p, "rb").read()) - (4 + 80 * 4)
    # a truncated block and an unknown shape type are refused
    good = open(p, "rb").read()
    (tmp_path / "cut.ppgs").write_bytes(good[:-40])
    (tmp_path / "type.ppgs").write_bytes(good[:-80] + struct.pack("<i", 7) + good[-76:])
    for name in ("cut.ppgs", "type.ppgs"):
        with pytest.raises(ValueError):
            ppg_host.load_scene_file(str(tmp_path / name))


def test_xml_writer_round_trip(tmp_path):
    desc, props, _ = ppg_host.load_scene(XML)
    path = mitsuba_xml.save_scene_xml(desc, props, str(tmp_path))
    back, _, _ = ppg_host.load_scene(path)
    same_records(back.shapes, desc.shapes)  # the identity on the records: same order, same emitters, every float the same
    assert back.emitters == desc.emitters and back.n_triangles == desc.n_triangles


SCENE = """<scene version="0.6.0">
<integrator type="guided_path"><string name="budgetType" value="spp"/><float name="budget" value="4"/></integrator>
<sensor type="perspective"><transform name="toWorld"><lookAt origin="0, 0, -4" target="0, 0, 0" up="0, 1, 0"/></transform>
<film type="hdrfilm"><integer name="width" value="8"/><integer name="height" value="8"/><rfilter type="box"/></film></sensor>
<shape type="rectangle"/>
%s
</scene>
"""
REFUSALS = {
    "sheared disk": ('<shape type="disk"><transform name="toWorld"><matrix value="1 0.3 0 0  0 1 0 0  0 0 1 0  0 0 0 1"/></transform></shape>',
                     "disk: 'toWorld' transformation contains shear!"),
    "non-uniformly scaled disk": ('<shape type="disk"><transform name="toWorld"><scale x="1" y="1.5" z="1"/></transform></shape>',
                                  "disk: 'toWorld' transformation contains a non-uniform scale!"),
    "cylinder with p0 == p1": ('<shape type="cylinder"><point name="p0" x="1" y="2" z="3"/><point name="p1" x="1" y="2" z="3"/></shape>',
                               "cylinder: p0 and p1 coincide"),
    "cylinder under a non-uniform toWorld": ('<shape type="cylinder"><transform name="toWorld"><scale x="1" y="2" z="1"/></transform></shape>',
                                             "cylinder: 'toWorld' transformation contains a non-uniform scale!"),
    "cylinder sheared by a non-uniform toWorld": ('<shape type="cylinder"><point name="p1" x="1" y="0" z="1"/><transform name="toWorld"><scale x="1" y="1" z="3"/>'
                                                  '</transform></shape>', "cylinder: 'toWorld' transformation contains"),
    "textured BSDF on a disk": ('<shape type="disk"><bsdf type="diffuse"><texture type="bitmap" name="reflectance"><string name="filename" value="tex.pfm"/>'
                                '</texture></bsdf></shape>', "disk: textured BSDFs are only supported on triangle meshes"),
    "cylinder that states nothing": ('<shape type="cylinder"/>', "cylinder: none of p0, p1, radius, toWorld is given"),
    "hair": ('<shape type="hair"/>', "is not supported (obj, ply, serialized, rectangle, cube, sphere, disk, cylinder)"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals_of_both_loaders(case, ppg_render, tmp_path):
    body, message = REFUSALS[case]
    from ppg_host import imageio
    imageio.write_pfm(str(tmp_path / "tex.pfm"), np.full((2, 2, 3), 0.5, np.float32))
    xml = tmp_path / "s.xml"
    xml.write_text(SCENE % body)
    with pytest.raises(mitsuba_xml.SceneError) as e:
        ppg_host.load_scene(str(xml))
    assert message in str(e.value), str(e.value)
    r = subprocess.run([ppg_render, "--ppgs", str(tmp_path / "x.ppgs"), "-q", str(xml)], capture_output=True, text=True)
    # (the C++ loader reads no bitmaps at all: it refuses the textured value before it gets to the shape)
    cpp_message = "textured 'reflectance' is not supported" if case == "textured BSDF on a disk" else message
    assert r.returncode != 0 and cpp_message in r.stderr, r.stderr


def test_a_cylinder_stretched_along_its_axis_is_a_longer_cylinder(tmp_path):
    """(a toWorld that scales the axis and the circle differently leaves a cylinder: only its length changes, as in Mitsuba)"""
    xml = tmp_path / "s.xml"
    xml.write_text(SCENE % '<shape type="cylinder"><float name="radius" value="0.5"/><transform name="toWorld"><scale x="2" y="2" z="3"/></transform></shape>')
    desc, _, _ = ppg_host.load_scene(str(xml))
    assert desc.shapes[0]["radius"] == 1.0 and desc.shapes[0]["length"] == 3.0
    assert np.array_equal(np.asarray(desc.shapes[0]["to_world"]).reshape(3, 4), np.eye(4)[:3])


def test_shapes_aimed_with_lookat_load_alike_in_both_loaders(ppg_render, tmp_path):
    """a round lamp aimed with <lookAt>: object z looks from `origin` at `target`; both loaders, byte for byte, and the float64 restatement"""
    xml = tmp_path / "s.xml"
    xml.write_text(SCENE % ('<shape type="disk"><transform name="toWorld"><scale value="0.4"/><lookAt origin="1, 2, 0.5" target="0.2, 0, 0.1" up="0, 1, 0.1"/>'
                            '</transform><emitter type="area"><rgb name="radiance" value="5"/></emitter></shape>'
                            '<shape type="cylinder"><float name="radius" value="0.2"/><transform name="toWorld"><lookat origin="-1, 1, 0" target="0, 0, 1"/>'
                            '</transform></shape>'))
    desc, _, _ = ppg_host.load_scene(str(xml))
    o, tg, up = np.array([f(1), f(2), f(0.5)]), np.array([f(0.2), 0.0, f(0.1)]), np.array([0.0, 1.0, f(0.1)])
    d = (tg - o) / np.linalg.norm(tg - o)
    left = np.cross(up, d) / np.linalg.norm(np.cross(up, d))
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = left, np.cross(d, left), d, o
    assert close(desc.shapes[0]["to_world"], (m @ scale(0.4))[:3].reshape(-1))
    axis = np.asarray(desc.shapes[1]["to_world"]).reshape(3, 4)[:, 2]
    assert close(axis, np.array([1.0, -1.0, 1.0]) / math.sqrt(3)) and desc.shapes[1]["radius"] == f(0.2) and abs(desc.shapes[1]["length"] - 1) < 1e-6
    r = subprocess.run([ppg_render, "--ppgs", str(tmp_path / "cpp.ppgs"), "-q", str(xml)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ppg_host.save_scene(desc, str(tmp_path / "py.ppgs"))
    assert _shape_block(str(tmp_path / "cpp.ppgs"))[1] == _shape_block(str(tmp_path / "py.ppgs"))[1] != b""


def test_ctypes_mirror_has_the_layout_of_the_header(tmp_path):
    fields = ["type", "to_world", "radius", "length", "material", "emitter", "flip_normals", "_reserved"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppg.h"\n#include "ppg_testhooks.h"\nint main(void) { printf("%zu %zu %zu", sizeof(ppg_shape), '
                   'sizeof(struct ppg_debug_hit), sizeof(struct ppg_debug_direct));\n'
                   + "".join('printf(" %%zu", offsetof(ppg_shape, %s));\n' % n for n in fields)
                   + 'printf(" %zu %zu %zu %zu", offsetof(struct ppg_debug_hit, wi), offsetof(struct ppg_debug_hit, emitter), offsetof(struct ppg_debug_direct, pdf), '
                   'offsetof(struct ppg_debug_direct, value)); printf(" %d %d\\n", PPG_SHAPE_DISK, PPG_SHAPE_CYLINDER); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(b.Shape), C.sizeof(b.DebugHit), C.sizeof(b.DebugDirect)] + [getattr(b.Shape, n).offset for n in fields]
    want += [b.DebugHit.wi.offset, b.DebugHit.emitter.offset, b.DebugDirect.pdf.offset, b.DebugDirect.value.offset]
    want += [b.Shape.TYPES.index("disk"), b.Shape.TYPES.index("cylinder")]
    assert got == want
    assert got[0] == 80 and got[0] % 16 == 0 and got[1:3] == [80, 64]
    assert b.DEBUG_HIT_DTYPE.itemsize == 80 and b.DEBUG_DIRECT_DTYPE.itemsize == 64
    from ppg_host.scenes import C_SHAPE_BYTES
    assert C_SHAPE_BYTES == 80


def test_the_oracle_refuses_scenes_with_shapes(oracle_lib):
    from conftest import make_oracle
    desc, _, _ = ppg_host.load_scene(XML)
    e = make_oracle(oracle_lib, budgetType="spp", budget=4)
    with pytest.raises(NotImplementedError, match="disks and cylinders"):
        e.set_scene(desc)
