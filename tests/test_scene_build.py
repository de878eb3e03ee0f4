"""buildScene() (csrc/ppg_scene_build.h), the pure stage of ppg_set_scene, on the host alone: tests/scene_build_check.hip is compiled with the
address and undefined-behaviour sanitizers on its host code and run as a child process — no context, no device, nothing loaded into this
interpreter.  The program builds one scene that fills every host table at once (66 triangles, and the same cut to 64 and to 0), one refused
scene per kind of index the function trusts — each at its first invalid value, with its exact message — and pairs of defects whose winner is
the order of ppg_set_scene's checks.  It prints a checksum of every table: a change of the function that is meant to keep the tables shows
there (the values are libm's and the compiler's as well, so they are compared between two builds, never with a constant)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail("hipcc not found (set HIPCC)")
    exe = str(tmp_path_factory.mktemp("scene_build") / "scene_build_check")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "scene_build_check.hip")])
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)
    print(run.stdout)
    print(run.stderr)
    return run


def test_every_check_of_the_program_passes_under_the_sanitizers(check_output):
    assert check_output.returncode == 0, check_output.stdout[-4000:] + check_output.stderr[-4000:]
    assert "all checks passed" in check_output.stdout and "FAILED" not in check_output.stdout
    assert "runtime error" not in check_output.stderr and "AddressSanitizer" not in check_output.stderr


def test_the_accepted_scenes_fill_every_table(check_output):
    lines = check_output.stdout.splitlines()
    heads = [l for l in lines if l.startswith("accepted ")]
    assert [h.split()[1] for h in heads] == ["66", "64", "0"]
    tables = {}
    scene = None
    for l in lines:
        if l.startswith("accepted "):
            scene = l.split()[1]
        elif l.startswith("  ") and scene:
            name, count, digest = l.split()
            tables[scene, name] = (int(count), digest)
    for name in ("tris", "accel", "accelSmall", "normals", "uvs", "nodes", "nodes4q", "topCut", "mats", "ems", "mfd", "coat", "blend", "texels0", "texels1",
                 "textures", "envTexels", "envCdfRows", "envCdfCols", "envRowWeights", "emSel", "emArea", "emInfo", "emTris", "emNormals", "delta", "shapes",
                 "spheres", "rtrans"):
        assert tables["66", name][0] > 0, name
    # 66 triangles are past the small-scene rule (no record is grouped by axis), 64 are within it
    assert "small_n 0 0 0" in heads[0] and "small_n 0 0 64" in heads[1]
    # the tables that do not depend on the triangles are the same in all three
    for name in ("mats", "mfd", "coat", "blend", "textures", "envCdfCols", "delta", "shapes", "spheres", "rtrans"):
        assert tables["66", name] == tables["64", name] == tables["0", name], name
    assert tables["0", "tris"][0] == 0 and tables["0", "nodes4q"][0] == 1
