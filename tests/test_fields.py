"""Feature buffers of the first hit (include/ppg.h ppg_render_fields), the parts that need no GPU: the boundary's structure and names
against the header, the multichannel / field integrators of the scene XML, the EXR layers, the command line's argument errors."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ppg_host
from conftest import ROOT
from ppg_host import bindings as b
from ppg_host import mitsuba_xml
from ppg_host.imageio import read_exr, write_exr
from test_mitsuba_xml import SCENE, _write

HEADER = os.path.join(ROOT, "include", "ppg.h")


def test_ctypes_mirror_of_ppg_fields_has_the_layout_of_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppg.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(ppg_fields), '
                   'offsetof(ppg_fields, n_fields), offsetof(ppg_fields, field), offsetof(ppg_fields, undefined), offsetof(ppg_fields, spp), '
                   'offsetof(ppg_fields, first_sample), PPG_MAX_FIELDS); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = [C.sizeof(b.Fields), b.Fields.n_fields.offset, b.Fields.field.offset, b.Fields.undefined.offset, b.Fields.spp.offset, b.Fields.first_sample.offset,
            b.MAX_FIELDS]
    assert got == want and got[0] == 4 + 8 * 4 + 8 * 12 + 8


def test_field_names_are_the_headers_enum():
    src = open(HEADER).read()
    enum = dict((n, int(v)) for n, v in re.findall(r"PPG_FIELD_([A-Z_]+) = (\d+)", src))
    assert len(enum) == 8 and sorted(enum.values()) == list(range(8))
    mitsuba = dict(POSITION="position", REL_POSITION="relPosition", DISTANCE="distance", GEO_NORMAL="geoNormal", SH_NORMAL="shNormal", UV="uv",
                   ALBEDO="albedo", PRIM_INDEX="primIndex")  # field.cpp:72-91
    assert {mitsuba[k]: v for k, v in enum.items()} == b.FIELD_NAMES
    with pytest.raises(ValueError, match="position, relPosition, distance, geoNormal, shNormal, uv, albedo, primIndex"):
        b.field_code("shapeIndex")
    assert "ppg_render_fields" in src and "ppg_debug_camera_rays" in open(os.path.join(ROOT, "include", "ppg_testhooks.h")).read()


def _multichannel(tmp_path, inner):
    """tests/test_mitsuba_xml.py's scene with its guided_path integrator wrapped (or replaced) by `inner` inside a multichannel one"""
    p = _write(tmp_path)
    text = open(p).read()
    mo = re.search(r'<integrator type="guided_path">.*?</integrator>', text, re.S)
    q = tmp_path / "mc.xml"
    q.write_text(text[:mo.start()] + '<integrator type="multichannel">' + inner.replace("GUIDED", mo.group(0)) + "</integrator>" + text[mo.end():])
    return str(q)


FIELD = '<integrator type="field"> <string name="field" value="%s"/> %s </integrator>'


def test_multichannel_scenes_give_their_fields(tmp_path):
    desc, props, info = ppg_host.load_scene(_write(tmp_path), defines=dict(nee="never"))
    assert info["fields"] == []  # a plain scene
    inner = (FIELD % ("albedo", "") + "GUIDED" + FIELD % ("shNormal", '<float name="undefined" value="-1"/>') +
             FIELD % ("distance", '<rgb name="undefined" value="0.25, 0.5, 1"/>') + FIELD % ("primIndex", '<spectrum name="undefined" value="2"/>'))
    desc2, props2, info2 = ppg_host.load_scene(_multichannel(tmp_path, inner), defines=dict(nee="never"))
    assert info2["fields"] == [("albedo", (0.0, 0.0, 0.0)), ("shNormal", (-1.0, -1.0, -1.0)), ("distance", (0.25, 0.5, 1.0)), ("primIndex", (2.0, 2.0, 2.0))]
    assert props2 == props and desc2.n_triangles == desc.n_triangles  # the guided_path inside is read as the plain one is
    assert ppg_host.load_scene(_multichannel(tmp_path, "GUIDED"), defines=dict(nee="never"))[2]["fields"] == []


@pytest.mark.parametrize("inner,needle", [
    (FIELD % ("normal", "") + "GUIDED", "Invalid 'field' parameter. Must be one of 'position', 'relPosition', 'distance', 'geoNormal', 'shNormal', 'primIndex', 'shapeIndex', or 'uv'!"),
    (FIELD % ("shapeIndex", "") + "GUIDED", "shapeIndex"),
    ("GUIDED" + "GUIDED", "guided_path"),
    (FIELD % ("albedo", ""), "guided_path"),
    ("GUIDED" + '<integrator type="path"/>', "guided_path"),
], ids=["bad-name", "shapeIndex", "two-guided", "no-guided", "other-integrator"])
def test_multichannel_refusals(tmp_path, inner, needle):
    with pytest.raises(mitsuba_xml.SceneError, match=re.escape(needle)):
        ppg_host.load_scene(_multichannel(tmp_path, inner), defines=dict(nee="never"))


def _parent_write_exr(path, rgb, attributes=None):
    """write_exr as it stood before it took layers: the golden for a file without any"""
    import struct
    attr = lambda name, typ, payload: name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(payload)) + payload  # noqa: E731
    img = np.ascontiguousarray(rgb, np.float32)
    H, W, _ = img.shape
    chans = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", 2, 0, 1, 1) for n in ("B", "G", "R")) + b"\0"
    box = struct.pack("<4i", 0, 0, W - 1, H - 1)
    hdr = struct.pack("<II", 20000630, 2) + attr("channels", "chlist", chans) + attr("compression", "compression", b"\0")
    hdr += attr("dataWindow", "box2i", box) + attr("displayWindow", "box2i", box) + attr("lineOrder", "lineOrder", b"\0")
    hdr += attr("pixelAspectRatio", "float", struct.pack("<f", 1.0)) + attr("screenWindowCenter", "v2f", struct.pack("<2f", 0.0, 0.0))
    hdr += attr("screenWindowWidth", "float", struct.pack("<f", 1.0))
    for k, v in (attributes or {}).items():
        hdr += attr(k, "string", str(v).encode("utf-8", "replace"))
    hdr += b"\0"
    line = 12 * W
    first = len(hdr) + 8 * H
    with open(path, "wb") as f:
        f.write(hdr + struct.pack("<%dQ" % H, *[first + y * (8 + line) for y in range(H)]))
        for y in range(H):
            f.write(struct.pack("<ii", y, line) + img[y, :, 2].tobytes() + img[y, :, 1].tobytes() + img[y, :, 0].tobytes())


def test_exr_layers_round_trip_and_the_plain_file_is_unchanged(tmp_path):
    rng = np.random.RandomState(4)
    rgb = rng.rand(13, 17, 3).astype(np.float32)
    layers = {"shNormal": (rng.rand(13, 17, 3) * 2 - 1).astype(np.float32), "albedo": rng.rand(13, 17, 3).astype(np.float32),
              "Zfirst": rng.rand(13, 17, 3).astype(np.float32)}
    layers["albedo"][3, 5] = [np.nan, np.inf, -0.0]
    p = str(tmp_path / "l.exr")
    write_exr(p, rgb, {"log": "a\nb"}, layers=layers)
    got, attrs, lay = read_exr(p, layers=True)
    assert got.tobytes() == rgb.tobytes() and attrs["log"] == "a\nb" and sorted(lay) == sorted(layers)
    for k in layers:
        assert lay[k].tobytes() == layers[k].tobytes(), k
    # the file's channel list is alphabetical (bytewise, as OpenEXR sorts it): B G R Zfirst.* albedo.* shNormal.*
    buf = open(p, "rb").read()
    names = [n.decode() for n in re.findall(rb"([A-Za-z.]+)\0\x02\0\0\0\0\0\0\0\x01\0\0\0\x01\0\0\0", buf)]
    assert names == ["B", "G", "R", "Zfirst.B", "Zfirst.G", "Zfirst.R", "albedo.B", "albedo.G", "albedo.R", "shNormal.B", "shNormal.G", "shNormal.R"]
    assert len(read_exr(p)) == 2 and np.array_equal(read_exr(p)[0], rgb)  # the default reads as before
    # without layers the bytes are those of the function as it stood
    q, g = str(tmp_path / "plain.exr"), str(tmp_path / "golden.exr")
    write_exr(q, rgb, {"log": "x", "generatedBy": "y"})
    _parent_write_exr(g, rgb, {"log": "x", "generatedBy": "y"})
    assert open(q, "rb").read() == open(g, "rb").read()
    write_exr(q, rgb, None, layers={})
    _parent_write_exr(g, rgb)
    assert open(q, "rb").read() == open(g, "rb").read()


@pytest.mark.parametrize("args,needle", [
    (["--fields", "albedo,normal"], "unknown field 'normal'"),
    (["--fields", "shapeIndex"], "unknown field 'shapeIndex'"),
    (["--fields", "albedo", "-o", "out.pfm"], "PFM"),
    (["--fields", "albedo", "--fields-spp", "0"], "--fields-spp"),
    (["--fields", "albedo", "--fields-spp", "65537"], "--fields-spp"),
], ids=["unknown", "shapeIndex", "pfm", "spp-0", "spp-big"])
def test_command_line_argument_errors(tmp_path, capsys, args, needle):
    from ppg_host.__main__ import main
    with pytest.raises(SystemExit) as ex:
        main([_write(tmp_path)] + args)
    assert ex.value.code == 2 and needle in capsys.readouterr().err


def test_the_oracle_engine_refuses_both_by_name(oracle_lib):
    o = ppg_host.Engine(oracle_lib, "ppgo_", budgetType="spp", budget=4)
    o.set_scene(ppg_host.cbox_scene(8, 8))
    with pytest.raises(NotImplementedError, match="ppg_render_fields"):
        o.render_fields(["albedo"])
    with pytest.raises(NotImplementedError, match="ppg_debug_camera_rays"):
        o.debug_camera_rays()


def test_command_line_refuses_a_pfm_for_a_multichannel_scene(tmp_path, capsys):
    from ppg_host.__main__ import main
    p = _multichannel(tmp_path, FIELD % ("albedo", "") + "GUIDED")
    with pytest.raises(SystemExit) as ex:
        main([p, "-D", "nee=never", "-o", str(tmp_path / "o.pfm")])
    assert ex.value.code == 2 and "PFM" in capsys.readouterr().err
