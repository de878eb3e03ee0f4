"""The .ppgs container (host/scene_file.h, ppg_host/scenes.py): one scene that carries all fourteen optional blocks goes through both
writers and both readers and stays the same bytes; every truncation of it is refused by both readers.  tests/scene_file_check.cpp does
the C++ half in-process, compiled with the address and undefined-behaviour sanitizers and run as a child process."""
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

CXX = os.environ.get("CXX", "c++")
BIN = os.path.join(PKG, "bin", "ppg_render")
f32 = np.float32


@pytest.fixture(scope="module")
def ppg_render():
    if not os.path.exists(BIN):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "__graft_entry__.py")])
    return BIN


def full_scene():
    """cbox_scene(8, 6) with every optional block of the format"""
    import ppg_host
    d = ppg_host.cbox_scene(8, 6)
    nv = len(d.positions)
    d.normals = np.tile(np.asarray([[0.0, 1.0, 0.0]], f32), (nv, 1))
    d.environment = (0.25, 0.5, 0.75)
    d.rtrans = np.asarray([[0.9, 0.8, 0.7, 0.6, 0.5], [0.95, 0.85, 0.75, 0.65, 0.55]], f32)
    d.spheres = [dict(center=(100.0, 50.0, 100.0), radius=25.0, material=1, emitter=-1, flip_normals=True)]
    d.envmap = dict(rgb=np.arange(18, dtype=f32).reshape(3, 2, 3) / 8, scale=2.0, to_world=[0, 0, 1, 0, 1, 0, -1, 0, 0])
    d.texcoords = (np.arange(2 * nv, dtype=f32).reshape(nv, 2) / 16)
    d.textures = [dict(rgb=np.full((2, 2, 3), 0.5, f32), uv_scale=(2.0, 3.0), uv_offset=(0.25, 0.5), wrap_u="mirror", wrap_v="clamp", nearest=True),
                  dict(rgb=np.arange(12, dtype=f32).reshape(1, 4, 3) / 16)]
    d.rfilter = dict(type="gaussian", stddev=0.75)
    d.lens = dict(aperture_radius=4.0, focus_distance=900.0)
    d.delta_emitters = [dict(type="point", intensity=(1.0, 2.0, 3.0), position=(278.0, 300.0, 280.0)),
                        dict(type="spot", intensity=(4.0, 5.0, 6.0), position=(100.0, 500.0, 100.0), to_local=[1, 0, 0, 0, 0, 1, 0, -1, 0],
                             cutoff_angle=0.5, beam_width=0.375),
                        dict(type="directional", intensity=(0.5, 0.25, 0.125), direction=(0.0, -1.0, 0.0))]
    d.shapes = [dict(type="disk", to_world=[50, 0, 0, 400, 0, 0, 50, 1, 0, -50, 0, 100], material=2),
                dict(type="cylinder", to_world=[1, 0, 0, 150, 0, 1, 0, 0, 0, 0, 1, 400], radius=30.0, length=120.0, material=3, flip_normals=True)]
    d.materials = list(d.materials) + [
        dict(type="roughconductor", alpha=0.25, alpha_v=0.125, specular_texture=1, eta=(0.2, 0.9, 1.1), k=(3.9, 2.4, 2.2), reflectance=(1.0, 1.0, 1.0)),
        dict(type=0, reflectance=(0.5, 0.25, 0.125), texture=0,
             coating=dict(kind="roughcoating", eta=1.5, thickness=0.5, sigma_a=(0.1, 0.2, 0.3), alpha=0.125, distribution="ggx", slice=1)),
        dict(type=0, opacity=(0.5, 0.5, 0.5), opacity_texture=0, blend=dict(kind="mixturebsdf", children=[1, 2], weights=(0.25, 0.5)))]
    return d


def _flags(raw):
    return struct.unpack_from("<6I", raw, 4)[5]


@pytest.fixture(scope="module")
def full_file(tmp_path_factory):
    import ppg_host
    path = str(tmp_path_factory.mktemp("scene_file") / "a.ppgs")
    ppg_host.save_scene(full_scene(), path)
    return path


def test_both_writers_and_both_readers_keep_the_fourteen_blocks_byte_for_byte(ppg_render, full_file, tmp_path):
    import ppg_host
    a = open(full_file, "rb").read()
    assert _flags(a) == 0x3fff
    b, c, d = (str(tmp_path / n) for n in ("b.ppgs", "c.ppgs", "d.ppgs"))
    r = subprocess.run([ppg_render, "-q", "--ppgs", b, full_file], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ppg_host.save_scene(ppg_host.load_scene_file(full_file), c)
    ppg_host.save_scene(ppg_host.load_scene_file(b), d)
    for other in (b, c, d):
        assert open(other, "rb").read() == a, other


def test_the_python_reader_refuses_every_proper_prefix(full_file, tmp_path):
    import ppg_host
    a = open(full_file, "rb").read()
    p = str(tmp_path / "cut.ppgs")
    for n in range(len(a)):
        with open(p, "wb") as f:
            f.write(a[:n])
        with pytest.raises(ValueError):
            ppg_host.load_scene_file(p)


def test_the_driver_refuses_prefixes(ppg_render, full_file, tmp_path):
    a = open(full_file, "rb").read()
    p = str(tmp_path / "cut.ppgs")
    for n in sorted(set(range(0, len(a), 37)) | set(range(len(a) - 65, len(a)))):
        with open(p, "wb") as f:
            f.write(a[:n])
        r = subprocess.run([ppg_render, p], capture_output=True, text=True)
        assert r.returncode == 2 and "cannot load scene" in r.stderr, (n, r.returncode, r.stderr)


@pytest.fixture(scope="module")
def check_output(full_file, tmp_path_factory):
    if not shutil.which(CXX):
        pytest.fail("no host C++ compiler found (set CXX)")
    exe = str(tmp_path_factory.mktemp("scene_file_check") / "scene_file_check")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(PKG, "host"), "-o", exe, os.path.join(ROOT, "tests", "scene_file_check.cpp")])
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe, full_file], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)
    print(run.stdout)
    print(run.stderr)
    return run


def test_the_cpp_container_under_the_sanitizers(check_output, full_file):
    out = check_output.stdout
    assert check_output.returncode == 0, out[-4000:] + check_output.stderr[-4000:]
    assert "all checks passed" in out and "FAILED" not in out
    assert "runtime error" not in check_output.stderr and "AddressSanitizer" not in check_output.stderr
    n = os.path.getsize(full_file)
    assert "rewritten: %d bytes, identical" % n in out
    assert "prefixes refused: %d of %d" % (n, n) in out
    assert "huge counts refused: 3 of 3" in out  # spheres, delta emitters, shapes
    assert "unknown block refused" in out


def test_a_coat_list_without_a_coat_writes_no_block(ppg_render, tmp_path):
    """SceneData::trimSideLists behind the XML loader: the loader collects a microfacet entry and a coat entry per material; the coat list
    is all kind == 0 and leaves no block, the microfacet list has one live entry and is written whole, one entry per material."""
    import ppg_host
    from ppg_host.scenes import C_MICROFACET_BYTES
    d = ppg_host.cbox_scene(8, 6)
    d.materials = list(d.materials)
    d.materials[1] = dict(type="roughconductor", alpha=0.25, sample_visible=False, eta=(0.2, 0.9, 1.1), k=(3.9, 2.4, 2.2), reflectance=(1.0, 1.0, 1.0))
    xml = ppg_host.save_scene_xml(d, dict(budgetType="spp", budget=4), str(tmp_path))
    out = str(tmp_path / "out.ppgs")
    r = subprocess.run([ppg_render, "-q", "--ppgs", out, xml], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    nv, nt, nm, ne, has_n, flags = struct.unpack_from("<6I", raw, 4)
    assert flags == 1 << 11 and nm == 5 and not has_n
    assert len(raw) == 28 + nv * 12 + nt * 20 + nm * 80 + ne * 16 + 144 + nm * C_MICROFACET_BYTES
    assert [m.get("sample_visible") for m in ppg_host.load_scene_file(out).materials] == [None, False, None, None, None]
