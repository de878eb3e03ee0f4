"""The C++ host side above the C-ABI (practical-path-guiding_amd/host): class GuidedPathTracerHIP + the ppg_render driver."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import CBOX_PROPS, PKG, ROOT

BIN = os.path.join(PKG, "bin", "ppg_render")


@pytest.fixture(scope="module")
def ppg_render():
    if not os.path.exists(BIN):
        subprocess.check_call([sys.executable, os.path.join(ROOT, "__graft_entry__.py")])
    return BIN


def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"PF"
        w, h = map(int, f.readline().split())
        assert float(f.readline()) < 0  # little endian
        data = np.frombuffer(f.read(), "<f4").reshape(h, w, 3)
    return data[::-1]  # PFM is bottom-up


def test_driver_builds_and_rejects_bad_input(ppg_render, tmp_path):
    r = subprocess.run([ppg_render, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "usage" in r.stdout
    r = subprocess.run([ppg_render, str(tmp_path / "missing.ppgs")], capture_output=True, text=True)
    assert r.returncode == 2 and "cannot load scene" in r.stderr
    r = subprocess.run([ppg_render, "--cbox", "8x8", "-D", "spatialFilter=gauss"], capture_output=True, text=True)
    assert r.returncode == 3 and ("spatialFilter" in r.stderr or "HIP device" in r.stderr)  # unknown enum value / no GPU here


def test_truncated_and_corrupt_scene_files_are_refused(ppg_render, tmp_path):
    """A flat scene file whose header or texture block claims more than the file holds (truncated download, corrupt sizes): both
    readers refuse it — "cannot load scene" / ValueError — instead of sizing an allocation by the claim."""
    import struct
    import ppg_host
    s = ppg_host.cbox_scene(16, 16)
    s.textures = [dict(rgb=np.full((4, 4, 3), 0.5, np.float32))]
    s.texcoords = np.zeros((len(s.positions), 2), np.float32)
    good = tmp_path / "good.ppgs"
    ppg_host.save_scene(s, str(good))
    buf = good.read_bytes()
    assert len(ppg_host.load_scene_file(str(good)).textures) == 1
    cases = {"cut.ppgs": buf[:len(buf) // 2], "short-texture.ppgs": buf[:-7],
             "huge-count.ppgs": buf[:4] + struct.pack("<I", 0x7fffffff) + buf[8:]}
    tex_hdr = len(buf) - (8 + 16 + 12 + 4 + 4 * 4 * 3 * 4)            # width, height of the one texture
    cases["huge-texture.ppgs"] = buf[:tex_hdr] + struct.pack("<2I", 0x7fff, 0x7fff) + buf[tex_hdr + 8:]
    cases["zero-texture.ppgs"] = buf[:tex_hdr] + struct.pack("<2I", 0, 4) + buf[tex_hdr + 8:]
    for name, data in cases.items():
        p = tmp_path / name
        p.write_bytes(data)
        with pytest.raises(ValueError):
            ppg_host.load_scene_file(str(p))
        r = subprocess.run([ppg_render, str(p)], capture_output=True, text=True)
        assert r.returncode == 2 and "cannot load scene" in r.stderr, (name, r.returncode, r.stderr)


def test_scene_file_round_trip(tmp_path):
    import struct
    import ppg_host
    s = ppg_host.cbox_scene(40, 30)
    p = tmp_path / "cbox.ppgs"
    ppg_host.save_scene(s, str(p))
    buf = p.read_bytes()
    assert buf[:4] == b"PPGS"
    nv, nt, nm, ne, has_n, _ = struct.unpack_from("<6I", buf, 4)
    assert (nv, nt, nm, ne, has_n) == (72, 36, 5, 1, 0)
    off = 28
    assert np.array_equal(np.frombuffer(buf, np.float32, nv * 3, off).reshape(-1, 3), s.positions)
    expect = 28 + nv * 12 + nt * 12 + nt * 4 + nt * 4 + nm * 80 + ne * 16 + (16 + 16) * 4 + 16
    assert len(buf) == expect
    w, h = struct.unpack_from("<2i", buf, len(buf) - 8)
    assert (w, h) == (40, 30)


@pytest.mark.gpu
def test_cpp_driver_equals_python_path(ppg_render, tmp_path):
    import ppg_host
    scene = ppg_host.cbox_scene(96, 64)
    path = str(tmp_path / "cbox.ppgs")
    ppg_host.save_scene(scene, path)
    for extra in ({}, dict(sampleCombination="inversevar", bsdfSamplingFractionLoss="kl", spatialFilter="stochastic", directionalFilter="box",
                           sTreeThreshold=4000, sppPerPass=1)):
        props = dict(CBOX_PROPS, budget=60, seed=5, **extra)
        out = str(tmp_path / "out.pfm")
        args = [ppg_render, "-o", out]
        for k, v in props.items():
            args += ["-D", "%s=%s" % (k, v)]
        r = subprocess.run(args + [path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        its = [int(m) for m in re.findall(r"ITERATION \d+, (\d+) passes", r.stdout)]
        e = ppg_host.Engine.hip(**props)
        gpt = ppg_host.GuidedPathTracer(engine=e)
        img = gpt.render(scene)
        assert its == [it["passes"] for it in gpt.iterations]
        assert "Distribution statistics" in r.stdout and "Total passes" in r.stdout  # the reference's log lines (GP:1176-1186, 1325)
        assert np.array_equal(read_pfm(out), img)
    # the built-in procedural CBOX (own C++ camera maths) renders the same picture up to the camera matrix's last bit
    out2 = str(tmp_path / "cbox.pfm")
    r = subprocess.run([ppg_render, "--cbox", "96x64", "-q", "-o", out2] + sum([["-D", "%s=%s" % kv] for kv in dict(CBOX_PROPS, budget=60, seed=5).items()], []),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    a, b = read_pfm(out2), ppg_host.GuidedPathTracer(engine=ppg_host.Engine.hip(**dict(CBOX_PROPS, budget=60, seed=5))).render(scene)
    assert abs(a.mean() / b.mean() - 1) < 0.05


def test_plugin_core_reports_errors_instead_of_crashing(ppg_render, tmp_path):
    """ppg::PluginCore (host/plugin_core.h) is what mitsuba_plugin/guided_path_hip.cpp is made of below the Mitsuba types; the stand-alone
    driver runs it with --plugin-core.  A context that cannot be created (unknown enum value; here also: no GPU) is an error message and a
    return code — never a NULL context handed on to ppg_set_scene, which is what round 3's shim did when Log(EError) did not throw."""
    r = subprocess.run([ppg_render, "--cbox", "8x8", "--plugin-core", "-D", "spatialFilter=gauss", "-o", str(tmp_path / "x.pfm")], capture_output=True, text=True)
    assert r.returncode == 3 and r.stderr.startswith("error: ") and ("spatialFilter" in r.stderr or "HIP device" in r.stderr)
    assert not (tmp_path / "x.pfm").exists()


@pytest.mark.gpu
def test_plugin_core_control_flow_dumps_and_cancel(ppg_render, tmp_path):
    """The plug-in's control flow, compiled and run (its source had never been): properties → create → scene → ONE ppg_render()
    → film equals the phase-by-phase C++ host bit for bit; dumpSDTree through it writes "<dest>-NN.sdt" for every iteration but the last
    (GP:1191-1195) — byte-equal to what the phase-driven host writes with an explicit prefix —; cancel() before render() and from another
    thread while it renders both end it with `false` (GP:1584) and without a crash."""
    props = dict(CBOX_PROPS, budget=60, seed=5, sampleCombination="inversevar", bsdfSamplingFractionLoss="kl", spatialFilter="stochastic",
                 directionalFilter="box", sTreeThreshold=4000, sppPerPass=1, dumpSDTree="true")
    defs = sum([["-D", "%s=%s" % kv] for kv in props.items()], [])
    a, b = tmp_path / "a" / "img.pfm", tmp_path / "b" / "img.pfm"
    a.parent.mkdir(); b.parent.mkdir()
    r = subprocess.run([ppg_render, "--cbox", "64x48", "-q", "--plugin-core", "-o", str(a)] + defs, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([ppg_render, "--cbox", "64x48", "-q", "-o", str(b), "-D", "dumpPrefix=%s" % (b.parent / "img")] + defs, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(read_pfm(str(a)), read_pfm(str(b)))
    dumps_a = sorted(f.name for f in a.parent.glob("img-*.sdt"))
    assert dumps_a == ["img-%02d.sdt" % k for k in range(len(dumps_a))] and len(dumps_a) >= 3  # 60 passes: iterations 0..4, the last one is final
    for name in dumps_a:
        assert (a.parent / name).read_bytes() == (b.parent / name).read_bytes() and (a.parent / name).stat().st_size > 64
    # dumpSDTree off: nothing is written
    c = tmp_path / "c" / "img.pfm"
    c.parent.mkdir()
    defs_off = sum([["-D", "%s=%s" % kv] for kv in dict(props, dumpSDTree="false").items()], [])
    r = subprocess.run([ppg_render, "--cbox", "64x48", "-q", "--plugin-core", "-o", str(c)] + defs_off, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and not list(c.parent.glob("*.sdt")) and np.array_equal(read_pfm(str(c)), read_pfm(str(a)))
    # Integrator::cancel(): before render() has a context, and in the middle of a long render
    d = tmp_path / "d.pfm"
    r = subprocess.run([ppg_render, "--cbox", "64x48", "--plugin-core", "--cancel-after-ms", "0", "-o", str(d)] + defs_off, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "(cancelled)" in r.stdout and not d.exists()
    long_defs = sum([["-D", "%s=%s" % kv] for kv in dict(props, dumpSDTree="false", budget=200000).items()], [])
    r = subprocess.run([ppg_render, "--cbox", "256x256", "--plugin-core", "--cancel-after-ms", "400", "-o", str(d)] + long_defs, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "(cancelled)" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert read_pfm(str(d)).shape == (256, 256, 3)  # whatever the film held when the render stopped


@pytest.mark.gpu
def test_cpp_rccl_reducer_single_rank(ppg_render, tmp_path):
    """`ppg_render --rank 0 --world 1 --nccl-id FILE`: the C++ RCCL reducer with a real communicator (ncclCommInitRank, packed all-reduces
    of images / SD-tree sums / film each with its status word; per round of the optimiser the records sent to the owners of their D-trees
    by grouped ncclSend / ncclRecv and the owners' state all-gathered — include/ppg.h "Sharded optimiser").  On one rank every exchange is
    the identity, so the picture must equal the un-sharded render bit for bit — for both film combinations and with the sampling-fraction
    optimiser on.  The id file carries the run's tag and is gone once the communicator exists."""
    import ppg_host
    scene = ppg_host.cbox_scene(96, 64)
    path = str(tmp_path / "cbox.ppgs")
    ppg_host.save_scene(scene, path)
    for extra in ({}, dict(sampleCombination="inversevar", bsdfSamplingFractionLoss="kl", directionalFilter="box")):
        props = dict(CBOX_PROPS, budget=60, seed=9, **extra)
        defs = sum([["-D", "%s=%s" % kv] for kv in props.items()], [])
        a, b = str(tmp_path / "a.pfm"), str(tmp_path / "b.pfm")
        r = subprocess.run([ppg_render, "-q", "-o", a] + defs + [path], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        (tmp_path / "id").write_bytes(b"stale file of an earlier run")
        r = subprocess.run([ppg_render, "-o", b, "--rank", "0", "--world", "1", "--nccl-id", str(tmp_path / "id"), "--run-tag", "run-%d" % len(extra)] + defs + [path],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert not (tmp_path / "id").exists()
        assert "RCCL communicator: rank 0 of 1" in r.stdout
        n = int(re.search(r"RCCL: (\d+) collectives", r.stdout).group(1))
        assert n >= 2 * len(re.findall(r"ITERATION", r.stdout))
        assert np.array_equal(read_pfm(a), read_pfm(b))
    # a wall-clock budget, sharded: every decision taken by a clock is rank 0's, broadcast (ppg_set_stop_hook, Reducer::broadcast) — the render
    # runs its iterations 1, 2, 4, ... until the second is up and ends normally
    r = subprocess.run([ppg_render, "-o", a, "--rank", "0", "--world", "1", "--nccl-id", str(tmp_path / "id2"), "-D", "budgetType=seconds",
                        "-D", "budget=1", path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    its = [int(m) for m in re.findall(r"ITERATION \d+, (\d+) passes", r.stdout)]
    assert len(its) >= 3 and its == [1 << k for k in range(len(its))] and np.isfinite(read_pfm(a)).all()


@pytest.mark.gpu
def test_scene_xml_through_both_drivers(ppg_render, tmp_path):
    """Mitsuba scene XML → (a) `python -m ppg_host` → EXR with the render log attached, (b) --ppgs + .props → the C++
    driver; both equal a direct render of the loaded scene."""
    import ppg_host
    from ppg_host.__main__ import main
    from ppg_host.imageio import read_exr
    props = dict(CBOX_PROPS, budget=28.0, nee="kickstart", sTreeThreshold=3000)
    props["strictNormals"] = 1
    xml = ppg_host.save_scene_xml(ppg_host.cbox_scene(80, 60), props, str(tmp_path), name="box")
    desc, loaded, _ = ppg_host.load_scene(xml)
    assert loaded == {k: (float(v) if k == "budget" else v) for k, v in props.items()}
    want = ppg_host.GuidedPathTracer(**loaded).render(desc)
    exr = str(tmp_path / "box.exr")
    assert main([xml, "-o", exr, "-q"]) == 0
    img, attrs = read_exr(exr)
    assert np.array_equal(img, want)
    assert attrs["log"].count("Total passes") == 3 and "Distribution statistics" in attrs["log"] and "Msamples/s" in attrs["log"]
    flat = str(tmp_path / "box.ppgs")
    assert main([xml, "--ppgs", flat, "-q"]) == 0
    out = str(tmp_path / "box.pfm")
    r = subprocess.run([ppg_render, "-q", "-o", out, flat], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(read_pfm(out), want)
    # (c) the C++ driver reading the XML itself (host/scene_xml.h)
    out2 = str(tmp_path / "box2.pfm")
    r = subprocess.run([ppg_render, "-q", "-o", out2, xml], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(read_pfm(out2), want)


def _read_ppgs(path):
    import struct
    buf = open(path, "rb").read()
    assert buf[:4] == b"PPGS"
    nv, nt, nm, ne, has_n, blocks = struct.unpack_from("<6I", buf, 4)
    has_env, has_rt = blocks & 1, blocks & 2
    off = 28
    def take(dtype, count):
        nonlocal off
        a = np.frombuffer(buf, dtype, count, off); off += a.nbytes
        return a
    out = dict(positions=take(np.float32, 3 * nv).reshape(-1, 3))
    out["normals"] = take(np.float32, 3 * nv).reshape(-1, 3) if has_n else None
    out["indices"] = take(np.uint32, 3 * nt).reshape(-1, 3)
    out["tri_material"] = take(np.uint32, nt); out["tri_emitter"] = take(np.int32, nt)
    out["materials"] = [bytes(take(np.uint8, 80)) for _ in range(nm)]
    out["emitters"] = take(np.float32, 4 * ne).reshape(-1, 4)
    out["s2c"] = take(np.float32, 16); out["c2w"] = take(np.float32, 16)
    out["clip"] = take(np.float32, 2); out["size"] = take(np.int32, 2)
    out["env"] = take(np.float32, 3) if has_env else None
    has_sph, has_em = blocks & 4, blocks & 8
    out["rtrans"] = None
    if has_rt:
        n, samples = take(np.uint32, 2)
        out["rtrans"] = take(np.float32, int(n) * (int(samples) + 1)).reshape(int(n), int(samples) + 1)
    out["spheres"] = []
    if has_sph:
        (n,) = take(np.uint32, 1)
        for _ in range(int(n)):
            f = take(np.float32, 13); i = take(np.int32, 3)
            out["spheres"].append(dict(center=tuple(f[:3]), radius=float(f[3]), to_world=f[4:13].copy(), material=int(i[0]), emitter=int(i[1]), flip_normals=int(i[2])))
    out["envmap"] = None
    if has_em:
        w, h = (int(v) for v in take(np.uint32, 2))
        scale = float(take(np.float32, 1)[0]); R = take(np.float32, 9).copy()
        out["envmap"] = dict(rgb=take(np.float32, w * h * 3).reshape(h, w, 3), scale=scale, to_world=R)
    assert off == len(buf)
    return out


def _cpp_load(ppg_render, xml, tmp_path, *extra):
    out = str(tmp_path / "cpp.ppgs")
    r = subprocess.run([ppg_render, "--ppgs", out, "-q", *extra, xml], capture_output=True, text=True)
    return r, (_read_ppgs(out) if r.returncode == 0 else None)


def test_cpp_scene_xml_loader_equals_the_python_loader(ppg_render, tmp_path):
    """host/scene_xml.h against ppg_host/mitsuba_xml.py on a scene using every supported element: transforms, $params, ref ids, nested BSDFs,
    all material plug-ins incl. mask / twosided, spectra, an n-gon OBJ with normals, generated vertex normals, a rectangle, an area
    and a constant emitter.  (No GPU needed: `ppg_render --ppgs` converts only.)"""
    import ppg_host
    from ppg_host.bindings import Material
    from test_mitsuba_xml import _write
    extra = """
    <bsdf type="mask" id="m1"><rgb name="opacity" value="0.3, 0.4, 0.5"/><bsdf type="twosided"><bsdf type="roughconductor">
        <string name="material" value="none"/><string name="distribution" value="ggx"/><float name="alpha" value="0.2"/></bsdf></bsdf></bsdf>
    <shape type="rectangle"><ref id="m1"/></shape>
    <shape type="rectangle"><bsdf type="plastic"><spectrum name="diffuseReflectance" value="400:0.1, 500:0.5, 600:0.3, 700:0.2"/></bsdf></shape>
    <shape type="rectangle"><bsdf type="dielectric"><string name="intIOR" value="water"/></bsdf></shape>
    <shape type="rectangle"><bsdf type="thindielectric"/></shape>
    <shape type="rectangle"><bsdf type="roughdielectric"><string name="intIOR" value="diamond"/><float name="alpha" value="0.05"/></bsdf></shape>
    <shape type="rectangle"><bsdf type="roughdielectric"><string name="distribution" value="ggx"/><rgb name="specularTransmittance" value="0.9, 0.8, 0.7"/></bsdf></shape>
    <shape type="rectangle"><bsdf type="conductor"><rgb name="eta" value="0.2, 0.9, 1.1"/><rgb name="k" value="3.9, 2.4, 2.1"/></bsdf></shape>
    <shape type="obj"><string name="filename" value="meshes/cube.obj"/><transform name="toWorld"><rotate x="1" y="1" angle="33"/><translate x="3"/></transform></shape>
    <emitter type="constant"><srgb name="radiance" value="0.5, 0.6, 0.7"/></emitter>
    <shape type="rectangle"><emitter type="area"><blackbody name="radiance" temperature="4500K" scale="0.001"/></emitter></shape>
    <shape type="rectangle"><bsdf type="diffuse"><spectrum name="reflectance" filename="meshes/paint.spd"/></bsdf></shape>
    <shape type="sphere"><point name="center" x="1" y="2" z="3"/><float name="radius" value="0.5"/><ref id="m1"/></shape>
    <shape type="cube"><boolean name="flipNormals" value="true"/><transform name="toWorld"><scale x="2" y="0.5" z="1"/><rotate y="1" angle="30"/><translate x="-4"/></transform></shape>
    <shape type="sphere"><boolean name="flipNormals" value="true"/><float name="radius" value="2"/>
        <transform name="toWorld"><rotate x="1" y="1" angle="33"/><scale value="3"/><translate x="5" y="6" z="7"/></transform>
        <emitter type="area"><rgb name="radiance" value="0.3, 0.4, 0.5"/></emitter></shape>
    """
    xml = _write(tmp_path, extra)
    # a cube with shared vertices and no normals: TriMesh::computeNormals generates them
    v = [(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    (tmp_path / "meshes" / "cube.obj").write_text("".join("v %d %d %d\n" % p for p in v) + "".join("f %d %d %d %d\n" % tuple(i + 1 for i in q) for q in quads))
    (tmp_path / "meshes" / "paint.spd").write_text("# measured\n400 0.1\n500 0.8\n600 0.5\n700 0.2\n")
    r, c = _cpp_load(ppg_render, xml, tmp_path, "-D", "nee=kickstart")
    assert r.returncode == 0, r.stderr
    desc, props, _ = ppg_host.load_scene(xml, defines=dict(nee="kickstart"))
    assert np.array_equal(c["indices"], desc.indices) and np.array_equal(c["tri_material"], desc.tri_material) and np.array_equal(c["tri_emitter"], desc.tri_emitter)
    assert np.allclose(c["positions"], desc.positions, rtol=1e-6, atol=1e-6) and np.allclose(c["normals"], desc.normals, rtol=1e-5, atol=1e-6)
    assert len(c["spheres"]) == len(desc.spheres) == 2 and len(desc.emitters) >= 3
    for a, b in zip(c["spheres"], desc.spheres):
        assert np.allclose(a["center"], b["center"], rtol=1e-6) and abs(a["radius"] - b["radius"]) < 1e-5 * b["radius"] and np.allclose(a["to_world"], b["to_world"], atol=1e-6)
        assert (a["material"], a["emitter"], a["flip_normals"]) == (b["material"], b["emitter"], int(b["flip_normals"]))
    py_mats = [bytes(Material.from_dict(m)) for m in desc.materials]
    assert len(c["materials"]) == len(py_mats)
    for a, b in zip(c["materials"], py_mats):
        fa, fb = np.frombuffer(a, np.float32), np.frombuffer(b, np.float32)
        ia, ib = np.frombuffer(a, np.int32), np.frombuffer(b, np.int32)
        assert ia[0] == ib[0] and ia[14] == ib[14]                      # type, flags
        assert np.allclose(fa[1:14], fb[1:14], rtol=2e-6) and np.allclose(fa[16:19], fb[16:19], rtol=2e-6)
    assert np.allclose(c["emitters"][:, :3], [e["radiance"] for e in desc.emitters]) and np.allclose(c["env"], desc.environment, rtol=1e-6)
    assert np.allclose(c["c2w"], np.asarray(desc.camera["camera_to_world"]).reshape(-1), atol=1e-6)
    assert np.allclose(c["s2c"], np.asarray(desc.camera["sample_to_camera"]).reshape(-1), rtol=1e-6, atol=1e-9)
    assert list(c["size"]) == [40, 30]
    got = dict(l.split("=", 1) for l in open(str(tmp_path / "cpp.ppgs.props")).read().split())
    assert got == {k: ("true" if v is True else str(v)) if not isinstance(v, float) else got[k] for k, v in dict(props, strictNormals="true").items()} and float(got["budget"]) == 12.0


@pytest.mark.skipif(not os.path.exists("/root/reference/mitsuba/data/microfacet/ggx.dat"), reason="Mitsuba data tables not mounted")
def test_cpp_roughplastic_slices_equal_the_python_loader(ppg_render, tmp_path):
    """host/rough_transmittance.h against ppg_host/rtrans.py: same table, same reduction, same float arithmetic ⇒ the same bits."""
    import ppg_host
    from test_mitsuba_xml import _write
    data = "/root/reference/mitsuba/data"
    xml = _write(tmp_path, """
    <shape type="rectangle"><bsdf type="roughplastic"><string name="distribution" value="ggx"/><float name="alpha" value="0.13"/>
        <string name="intIOR" value="water"/><rgb name="diffuseReflectance" value="0.1, 0.2, 0.3"/><boolean name="nonlinear" value="true"/></bsdf></shape>
    <shape type="rectangle"><bsdf type="twosided"><bsdf type="roughplastic"><float name="alpha" value="0.35"/></bsdf></bsdf></shape>
    <shape type="rectangle"><bsdf type="roughplastic"><string name="distribution" value="ggx"/><float name="alpha" value="0.13"/>
        <string name="intIOR" value="water"/></bsdf></shape>""")
    r, c = _cpp_load(ppg_render, xml, tmp_path, "-D", "nee=never", "--data-dir", data)
    assert r.returncode == 0, r.stderr
    desc, _, _ = ppg_host.load_scene(xml, defines=dict(nee="never"), data_dir=data)
    assert c["rtrans"].shape == desc.rtrans.shape == (2, 101) and np.array_equal(c["rtrans"], desc.rtrans)
    from ppg_host.bindings import Material
    for a, m in zip(c["materials"], desc.materials):
        b = bytes(Material.from_dict(m))
        assert np.frombuffer(a, np.int32)[[0, 14, 15]].tolist() == np.frombuffer(b, np.int32)[[0, 14, 15]].tolist()   # type, flags, rtrans slice
        assert np.allclose(np.frombuffer(a, np.float32)[1:11], np.frombuffer(b, np.float32)[1:11], rtol=2e-6)
    env = dict(os.environ); env.pop("PPG_MITSUBA_DATA", None)
    r = subprocess.run([ppg_render, "--ppgs", str(tmp_path / "x.ppgs"), "-q", "-D", "nee=never", xml], capture_output=True, text=True, env=env)
    assert r.returncode == 2 and "data/microfacet" in r.stderr
    # the flat file carries the slices: ppg_render reads back what it wrote
    r2 = subprocess.run([ppg_render, "--ppgs", str(tmp_path / "again.ppgs"), "-q", str(tmp_path / "cpp.ppgs")], capture_output=True, text=True)
    assert r2.returncode == 0, r2.stderr
    assert open(str(tmp_path / "again.ppgs"), "rb").read() == open(str(tmp_path / "cpp.ppgs"), "rb").read()


def test_cpp_envmap_readers_equal_the_python_loader(ppg_render, tmp_path):
    """host/hdr_image.h against ppg_host/imageio.py: PFM, Radiance RGBE (flat and run-length encoded), uncompressed EXR and — where
    the reference tree is mounted — one of its ZIP-compressed half-float EXR files, all through <emitter type="envmap">."""
    import ppg_host
    from ppg_host import imageio
    from test_envmap import _write_hdr
    from test_mitsuba_xml import _write
    rng = np.random.RandomState(5)
    img = (rng.rand(6, 40, 3) ** 3 * 50).astype(np.float32)
    img[2, 5:30] = img[2, 5]
    (tmp_path / "meshes").mkdir(exist_ok=True)
    imageio.write_pfm(str(tmp_path / "m.pfm"), img); imageio.write_exr(str(tmp_path / "m.exr"), img)
    _write_hdr(str(tmp_path / "flat.hdr"), img, False); _write_hdr(str(tmp_path / "rle.hdr"), img, True)
    files = ["m.pfm", "m.exr", "flat.hdr", "rle.hdr"]
    ref_exr = "/root/reference/scenes/cbox/cbox.exr"
    if os.path.exists(ref_exr):
        files.append(ref_exr)
    for fn in files:
        xml = _write(tmp_path, '<emitter type="envmap"><string name="filename" value="%s"/><float name="scale" value="1.5"/>'
                               '<transform name="toWorld"><rotate x="1" y="2" z="3" angle="40"/></transform></emitter>' % fn)
        r, c = _cpp_load(ppg_render, xml, tmp_path, "-D", "nee=never")
        assert r.returncode == 0, r.stderr
        desc, _, _ = ppg_host.load_scene(xml, defines=dict(nee="never"))
        assert np.array_equal(c["envmap"]["rgb"], desc.envmap["rgb"]), fn
        assert c["envmap"]["scale"] == desc.envmap["scale"] == 1.5 and np.allclose(c["envmap"]["to_world"], desc.envmap["to_world"], atol=1e-6)
    r, _ = _cpp_load(ppg_render, _write(tmp_path, '<emitter type="envmap"><string name="filename" value="nope.hdr"/></emitter>'), tmp_path, "-D", "nee=never")
    assert r.returncode == 2 and "not found" in r.stderr


def test_cpp_max_smooth_angle_equals_the_python_loader(ppg_render, tmp_path):
    """rebuildTopology in host/scene_xml.h against ppg_host/mitsuba_xml.py: a bumpy height field with texture coordinates and a sharp ridge,
    thresholds on both sides of its dihedral angles — same vertex numbering, same generated normals."""
    import ppg_host
    from test_mitsuba_xml import _write
    rng = np.random.RandomState(6)
    n = 7
    h = rng.rand(n, n) * 0.15
    h[:, n // 2] += 0.8                                           # the ridge
    lines = []
    for i in range(n):
        for j in range(n):
            lines.append("v %r %r %r" % (float(i), float(h[i, j]), float(j)))
    for i in range(n):
        for j in range(n):
            lines.append("vt %r %r" % (i / (n - 1), j / (n - 1)))
    for i in range(n - 1):
        for j in range(n - 1):
            a, b, c, d = i * n + j + 1, (i + 1) * n + j + 1, (i + 1) * n + j + 2, i * n + j + 2
            lines.append("f %d/%d %d/%d %d/%d %d/%d" % (a, a, b, b, c, c, d, d))
    (tmp_path / "meshes").mkdir(exist_ok=True)
    (tmp_path / "meshes" / "field.obj").write_text("\n".join(lines) + "\n")
    for angle in (5, 25, 60, 179):
        xml = _write(tmp_path, '<shape type="obj"><string name="filename" value="meshes/field.obj"/><float name="maxSmoothAngle" value="%d"/>'
                               '<transform name="toWorld"><rotate x="1" angle="20"/><scale value="0.5"/></transform></shape>' % angle)
        r, c = _cpp_load(ppg_render, xml, tmp_path, "-D", "nee=never")
        assert r.returncode == 0, r.stderr
        desc, _, _ = ppg_host.load_scene(xml, defines=dict(nee="never"))
        assert np.array_equal(c["indices"], desc.indices), angle
        assert np.allclose(c["positions"], desc.positions, rtol=1e-6, atol=1e-6) and np.allclose(c["normals"], desc.normals, rtol=1e-5, atol=2e-6)
    n5 = len(ppg_host.mitsuba_xml.load_obj(str(tmp_path / "meshes" / "field.obj"), max_smooth_angle=5.0)[0]["positions"])
    n179 = len(ppg_host.mitsuba_xml.load_obj(str(tmp_path / "meshes" / "field.obj"), max_smooth_angle=179.0)[0]["positions"])
    assert n179 == n * n and n5 > 2 * n * n                     # everything smooth vs. most vertices split


def test_cpp_serialized_loader_equals_the_python_loader(ppg_render, tmp_path):
    import ppg_host
    from test_mitsuba_xml import _two_meshes, _write, write_serialized
    (tmp_path / "meshes").mkdir(exist_ok=True)
    for version in (3, 4):
        write_serialized(str(tmp_path / "meshes" / "two.serialized"), list(_two_meshes()), version)
        xml = _write(tmp_path, '<shape type="serialized"><string name="filename" value="meshes/two.serialized"/><boolean name="flipNormals" value="true"/>'
                               '<transform name="toWorld"><scale x="-1"/><rotate y="1" angle="25"/></transform></shape>'
                               '<shape type="serialized"><string name="filename" value="meshes/two.serialized"/><integer name="shapeIndex" value="1"/>'
                               '<float name="maxSmoothAngle" value="20"/></shape>')
        r, c = _cpp_load(ppg_render, xml, tmp_path, "-D", "nee=never")
        assert r.returncode == 0, r.stderr
        desc, _, _ = ppg_host.load_scene(xml, defines=dict(nee="never"))
        assert np.array_equal(c["indices"], desc.indices) and np.allclose(c["positions"], desc.positions, rtol=1e-6, atol=1e-6)
        assert np.allclose(c["normals"], desc.normals, rtol=1e-5, atol=2e-6)
    r, _ = _cpp_load(ppg_render, _write(tmp_path, '<shape type="serialized"><string name="filename" value="meshes/two.serialized"/><integer name="shapeIndex" value="7"/></shape>'),
                     tmp_path, "-D", "nee=never")
    assert r.returncode == 2 and "out of range" in r.stderr


def test_cpp_ply_loader_equals_the_python_loader(ppg_render, tmp_path):
    import ppg_host
    from test_mitsuba_xml import _write, write_ply
    rng = np.random.RandomState(9)
    P = rng.rand(12, 3).astype(np.float32)
    faces = [(0, 1, 2, 3), (4, 5, 6), (7, 8, 9, 10), (1, 5, 11), (2, 6, 10, 11)]
    (tmp_path / "meshes").mkdir(exist_ok=True)
    for fmt, normals, double in (("ascii", None, False), ("binary_little_endian", rng.randn(12, 3).astype(np.float32), False), ("binary_big_endian", None, True)):
        write_ply(str(tmp_path / "meshes" / "m.ply"), P, faces, fmt, normals, double)
        xml = _write(tmp_path, '<shape type="ply"><string name="filename" value="meshes/m.ply"/><transform name="toWorld"><rotate x="1" angle="35"/><scale x="2" y="1" z="0.5"/></transform></shape>'
                               '<shape type="ply"><string name="filename" value="meshes/m.ply"/><float name="maxSmoothAngle" value="40"/><boolean name="flipNormals" value="true"/></shape>')
        r, c = _cpp_load(ppg_render, xml, tmp_path, "-D", "nee=never")
        assert r.returncode == 0, r.stderr
        desc, _, _ = ppg_host.load_scene(xml, defines=dict(nee="never"))
        assert np.array_equal(c["indices"], desc.indices) and np.allclose(c["positions"], desc.positions, rtol=1e-6, atol=1e-6)
        assert np.allclose(c["normals"], desc.normals, rtol=1e-5, atol=2e-6), fmt


@pytest.mark.skipif(not os.path.exists("/root/reference/scenes/spaceship/spaceship.xml"), reason="reference scenes not mounted (development container only)")
def test_cpp_loader_on_the_reference_spaceship_scene(ppg_render, tmp_path):
    """Both loaders on the reference's bundled SPACESHIP scene (84 of its 86 OBJ meshes are in the checkout): the same quarter of a million
    triangles in the same order, the same materials, rough-transmittance slices, emitters, sphere and camera."""
    import ppg_host
    from ppg_host.bindings import Material
    xml, data = "/root/reference/scenes/spaceship/spaceship.xml", "/root/reference/mitsuba/data"
    r, c = _cpp_load(ppg_render, xml, tmp_path, "--lenient", "--data-dir", data)
    assert r.returncode == 0, r.stderr
    desc, props, info = ppg_host.load_scene(xml, strict=False, data_dir=data)
    assert len(c["indices"]) == desc.n_triangles == 257486
    assert np.array_equal(c["indices"], desc.indices) and np.array_equal(c["tri_material"], desc.tri_material) and np.array_equal(c["tri_emitter"], desc.tri_emitter)
    assert np.allclose(c["positions"], desc.positions, rtol=1e-6, atol=1e-6) and np.allclose(c["normals"], desc.normals, rtol=1e-4, atol=1e-5)
    assert np.array_equal(c["rtrans"], desc.rtrans)
    for a, m in zip(c["materials"], desc.materials):
        b = bytes(Material.from_dict(m))
        assert np.frombuffer(a, np.int32)[[0, 14, 15]].tolist() == np.frombuffer(b, np.int32)[[0, 14, 15]].tolist()
        assert np.allclose(np.frombuffer(a, np.float32)[1:14], np.frombuffer(b, np.float32)[1:14], rtol=2e-6)
    assert len(c["spheres"]) == 1 and c["spheres"][0]["radius"] == pytest.approx(100.0) and c["spheres"][0]["flip_normals"] == 1
    assert np.allclose(c["emitters"][:, :3], [e["radiance"] for e in desc.emitters])
    assert np.allclose(c["c2w"], np.asarray(desc.camera["camera_to_world"]).reshape(-1), atol=1e-6) and list(c["size"]) == [640, 360]


def test_cpp_named_conductors_equal_the_python_loader(ppg_render, tmp_path):
    import ppg_host
    from ppg_host.bindings import Material
    from test_mitsuba_xml import MITSUBA_DATA as data, _write
    xml = _write(tmp_path, '<shape type="rectangle"><bsdf type="conductor"><string name="material" value="Au"/></bsdf></shape>'
                           '<shape type="rectangle"><bsdf type="roughconductor"><float name="extEta" value="1.33"/></bsdf></shape>'
                           '<shape type="rectangle"><bsdf type="conductor"><string name="material" value="W"/><rgb name="k" value="1, 2, 3"/></bsdf></shape>')
    r, c = _cpp_load(ppg_render, xml, tmp_path, "-D", "nee=never", "--data-dir", data)
    assert r.returncode == 0, r.stderr
    desc, _, _ = ppg_host.load_scene(xml, defines=dict(nee="never"), data_dir=data)
    assert len(c["materials"]) == len(desc.materials)
    for a, m in zip(c["materials"], desc.materials):
        b = bytes(Material.from_dict(m))
        assert np.frombuffer(a, np.int32)[0] == np.frombuffer(b, np.int32)[0]
        assert np.allclose(np.frombuffer(a, np.float32)[1:14], np.frombuffer(b, np.float32)[1:14], rtol=1e-5)
    env = dict(os.environ); env.pop("PPG_MITSUBA_DATA", None)
    r = subprocess.run([ppg_render, "--ppgs", str(tmp_path / "x.ppgs"), "-q", "-D", "nee=never", xml], capture_output=True, text=True, env=env)
    assert r.returncode == 2 and "data/ior" in r.stderr


@pytest.mark.skipif(not os.path.exists("/root/reference/mitsuba/src/emitters/sunsky/skymodeldata.h"), reason="Mitsuba source tree not mounted (development container only)")
def test_cpp_sunsky_bake_equals_the_python_loader(ppg_render, tmp_path):
    """`sunsky` in the C++ host (host/sunsky.h): the same bake as ppg_host/sunsky.py — Hosek-Wilkie sky + Preetham sun rasterised into the
    latitude-longitude radiance map the envmap emitter takes, tables parsed from the operator's Mitsuba tree — for the plug-in's defaults
    and for KITCHEN's settings (kitchen-improved.xml: its own sun position, scale, turbidity)."""
    import ppg_host
    from test_mitsuba_xml import _write
    for extra in ('<emitter type="sunsky"/>',
                  '<emitter type="sunsky"><float name="hour" value="9.5"/><float name="turbidity" value="4.5"/><float name="scale" value="2"/>'
                  '<integer name="resolution" value="128"/><float name="sunRadiusScale" value="3"/><rgb name="albedo" value="0.1, 0.3, 0.5"/>'
                  '<transform name="toWorld"><rotate y="1" angle="40"/></transform></emitter>'):
        xml = _write(tmp_path, extra)
        r, c = _cpp_load(ppg_render, xml, tmp_path, "-D", "nee=never", "--data-dir", "/root/reference/mitsuba/data")
        assert r.returncode == 0, r.stderr
        desc, _, _ = ppg_host.load_scene(xml, defines=dict(nee="never"), data_dir="/root/reference/mitsuba/data")
        a, b = c["envmap"]["rgb"], np.asarray(desc.envmap["rgb"])
        assert a.shape == b.shape and b.shape[1] == 2 * b.shape[0]
        assert np.allclose(c["envmap"]["to_world"], desc.envmap["to_world"], atol=1e-6) and c["envmap"]["scale"] == 1.0
        sun = b.max(-1) > 50 * np.median(b.max(-1)[: b.shape[0] // 2])                       # the pixels of the sun's disc
        assert 1 <= sun.sum() < 400 and np.array_equal(sun, a.max(-1) > 50 * np.median(a.max(-1)[: a.shape[0] // 2]))
        assert np.allclose(a, b, rtol=2e-5, atol=1e-7)                                       # libm vs numpy transcendentals: a few ulp
        assert abs(a.sum() / b.sum() - 1) < 1e-6


def test_cpp_lenient_loading_equals_the_python_loader(ppg_render, tmp_path):
    import ppg_host
    from ppg_host.bindings import Material
    from test_mitsuba_xml import LENIENT_EXTRA, _write
    xml = _write(tmp_path, LENIENT_EXTRA)
    r, _ = _cpp_load(ppg_render, xml, tmp_path, "-D", "nee=never")
    assert r.returncode == 2 and ("bumpmap" in r.stderr or "textured" in r.stderr or "sunsky" in r.stderr)
    r, c = _cpp_load(ppg_render, xml, tmp_path, "-D", "nee=never", "--lenient")
    assert r.returncode == 0, r.stderr
    desc, _, info = ppg_host.load_scene(xml, defines=dict(nee="never"), strict=False)
    assert np.array_equal(c["tri_material"], desc.tri_material) and len(c["materials"]) == len(desc.materials)
    for a, m in zip(c["materials"], desc.materials):
        b = bytes(Material.from_dict(m))
        assert np.frombuffer(a, np.int32)[[0, 14]].tolist() == np.frombuffer(b, np.int32)[[0, 14]].tolist()
        assert np.allclose(np.frombuffer(a, np.float32)[1:14], np.frombuffer(b, np.float32)[1:14], rtol=2e-6)


def test_cpp_scene_xml_loader_errors(ppg_render, tmp_path):
    from test_mitsuba_xml import _write
    for extra, needle in (('<shape type="cylinder"/>', "cylinder"), ('<shape type="rectangle"><bsdf type="ward"/></shape>', "ward"),
                          ('<emitter type="sunsky"/>', "sunsky"), ('<shape type="obj"><string name="filename" value="meshes/missing.obj"/></shape>', "not found")):
        r, _ = _cpp_load(ppg_render, _write(tmp_path, extra), tmp_path, "-D", "nee=never")
        assert r.returncode == 2 and needle in r.stderr, r.stderr
    r, _ = _cpp_load(ppg_render, _write(tmp_path), tmp_path)
    assert r.returncode == 2 and "$nee" in r.stderr          # undefined parameter
    r, c = _cpp_load(ppg_render, _write(tmp_path, '<shape type="rectangle"><bsdf type="ward"/></shape>'), tmp_path, "-D", "nee=never", "--lenient")
    assert r.returncode == 0 and len(c["indices"]) == 9


def test_cpp_loader_reads_the_reference_cbox(ppg_render, tmp_path):
    import ppg_host
    from test_mitsuba_xml import REF_CBOX
    r, c = _cpp_load(ppg_render, REF_CBOX, tmp_path)
    assert r.returncode == 0, r.stderr
    desc, _, _ = ppg_host.load_scene(REF_CBOX)
    assert np.array_equal(c["indices"], desc.indices) and np.allclose(c["positions"], desc.positions, atol=1e-4)
    assert np.allclose(c["normals"], desc.normals, atol=1e-5)
    mats = np.array([np.frombuffer(m, np.float32)[1:4] for m in c["materials"]])
    assert np.allclose(mats, [m["reflectance"] for m in desc.materials], rtol=5e-6)   # spectrum → RGB, incl. the reversed interpolation
    assert np.allclose(c["emitters"][0, :3], desc.emitters[0]["radiance"], rtol=5e-6)


def test_bsdf_by_id_for_the_mitsuba_plugin_shim(tmp_path):
    """mitsuba_plugin/guided_path_hip.cpp cannot reach the nested BSDF of a twosided / mask / bumpmap adapter through Mitsuba's API; it asks
    host/scene_xml.h for the <bsdf> element with the object's id (ppg::xml::bsdfById, exposed as `ppg_render --bsdf-id`): ids on nested
    elements are named objects of their own, unknown ids are reported."""
    import json
    xml = tmp_path / "s.xml"
    xml.write_text("""<scene version="0.5.0"><integrator type="guided_path"/><sensor type="perspective"><float name="fov" value="40"/>
        <film type="hdrfilm"><rfilter type="box"/></film></sensor>
        <bsdf type="bumpmap"><texture type="scale"/><bsdf type="twosided" id="inner"><bsdf type="diffuse"><rgb name="reflectance" value="0.2,0.3,0.4"/></bsdf></bsdf></bsdf>
        <bsdf type="mask" id="holes"><rgb name="opacity" value="0.25"/><bsdf type="roughconductor"><string name="material" value="none"/><float name="alpha" value="0.2"/>
            <string name="distribution" value="ggx"/></bsdf></bsdf>
        <shape type="rectangle"><ref id="inner"/></shape></scene>""")
    exe = os.path.join(ROOT, "practical-path-guiding_amd", "bin", "ppg_render")
    a = json.loads(subprocess.run([exe, str(xml), "--bsdf-id", "inner"], check=True, capture_output=True, text=True).stdout)
    assert a["type"] == 1 and np.allclose(a["reflectance"], [0.2, 0.3, 0.4])
    b = json.loads(subprocess.run([exe, str(xml), "--bsdf-id", "holes"], check=True, capture_output=True, text=True).stdout)
    assert b["type"] == 4 and b["flags"] & 4 and abs(b["alpha"] - 0.2) < 1e-6
    r = subprocess.run([exe, str(xml), "--bsdf-id", "nope"], capture_output=True, text=True)
    assert r.returncode == 2 and "no bsdf 'nope'" in r.stderr
    # a flat plug-in WITHOUT an id: the shim hands its Properties to the loader as the <bsdf> element they came from
    # (ppg::xml::bsdfFromProperties, `--bsdf-plugin` / `--bsdf-param name:tag:value`) — same material as the same element in a scene file
    xml2 = tmp_path / "s2.xml"
    xml2.write_text(xml.read_text().replace('<shape type="rectangle">', '<bsdf type="roughconductor" id="flat"><string name="material" value="none"/>'
                                            '<float name="alpha" value="0.15"/><string name="distribution" value="ggx"/><rgb name="specularReflectance" value="0.9, 0.8, 0.7"/></bsdf>'
                                            '<shape type="rectangle">', 1))
    want = json.loads(subprocess.run([exe, str(xml2), "--bsdf-id", "flat"], check=True, capture_output=True, text=True).stdout)
    got = json.loads(subprocess.run([exe, "--bsdf-plugin", "roughconductor", "--bsdf-param", "material:string:none", "--bsdf-param", "alpha:float:0.15",
                                     "--bsdf-param", "distribution:string:ggx", "--bsdf-param", "specularReflectance:rgb:0.9, 0.8, 0.7"],
                                    check=True, capture_output=True, text=True).stdout)
    assert got == want and got["type"] == 4 and abs(got["alpha"] - 0.15) < 1e-6 and np.allclose(got["reflectance"], [0.9, 0.8, 0.7])
    d = json.loads(subprocess.run([exe, "--bsdf-plugin", "dielectric", "--bsdf-param", "intIOR:string:water"], check=True, capture_output=True, text=True).stdout)
    assert abs(d["eta"] - 1.3330 / 1.000277) < 1e-5
    r = subprocess.run([exe, "--bsdf-plugin", "ward"], capture_output=True, text=True)
    assert r.returncode == 2 and "ward" in r.stderr
