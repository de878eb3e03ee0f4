"""Loading a dumped SD-tree, the part that needs no GPU (include/ppg.h "Loading a dumped SD-tree").
The import stage csrc/ppg_sdt_load.h on the host alone: tests/sdt_load_check.cpp is compiled with the address and undefined-behaviour
sanitizers and run as a child process — files built in memory, the trees that can be written out by hand, and every refusal, one case each.
ppg_host.read_sdt against the oracle's own view of the tree it dumped; the command line's default for --sdtree-iter."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import CBOX_PROPS, ROOT, make_oracle

CXX = os.environ.get("CXX", "c++")
HEADER = os.path.join(ROOT, "practical-path-guiding_amd", "csrc", "ppg_sdt_load.h")

REFUSALS = ["truncated-header", "trailing-bytes", "truncated-nodes", "numnodes-0", "numnodes-absurd", "numnodes-wraps", "numnodes-65537", "child-beyond",
            "child-not-above", "child-twice", "node-unreferenced", "sum-negative", "sum-nan", "sum-inf", "mean-nan", "box-inf", "box-nan",
            "other-aabb-inside", "other-aabb-larger", "other-aabb-shifted", "out-of-order", "overlapping", "same-leaf-twice", "stree-nodes",
            "sampling-nodes", "dtree-depth-21", "stree-depth-95-box"]


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    if not shutil.which(CXX):
        pytest.fail("no host C++ compiler found (set CXX)")
    exe = str(tmp_path_factory.mktemp("sdt_load") / "sdt_load_check")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "sdt_load_check.cpp")])
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)
    print(run.stdout)
    print(run.stderr)
    return run


def test_every_check_of_the_program_passes_under_the_sanitizers(check_output):
    assert check_output.returncode == 0, check_output.stdout[-4000:] + check_output.stderr[-4000:]
    assert "all checks passed" in check_output.stdout and "FAILED" not in check_output.stdout
    assert "runtime error" not in check_output.stderr and "AddressSanitizer" not in check_output.stderr


def test_every_refusal_was_exercised_and_names_its_place(check_output):
    lines = dict(re.findall(r"^refused (\S+)\s+(-\d+  .*)$", check_output.stdout, re.M))
    assert sorted(lines) == sorted(REFUSALS), sorted(set(REFUSALS) ^ set(lines))
    for name, rest in lines.items():
        code, msg = rest.split("  ", 1)
        assert int(code) == (-5 if name in ("stree-nodes", "sampling-nodes", "stree-depth-95-box") else -1), (name, rest)
        if name not in ("truncated-header", "stree-nodes", "sampling-nodes", "stree-depth-95-box"):
            assert re.match(r"leaf \d+ at offset \d+: ", msg), (name, msg)
    assert "the tree was trained on another scene" in lines["other-aabb-inside"]


def test_the_header_needs_no_device_toolchain():
    text = open(HEADER).read()
    includes = re.findall(r"^\s*#\s*include\s*[<\"]([^>\"]+)[>\"]", text, re.M)
    assert includes and all(not i.startswith("hip") and not i.startswith("ppg") and "/ppg" not in i for i in includes), includes
    assert "ppg_ctx" not in text


def _leaves_depth_first(tree):
    """S-tree leaves, child 0 before child 1 (STreeNode::forEachLeaf, GP:796-813)."""
    out, stack = [], [0]
    while stack:
        i = stack.pop()
        c0, c1 = (int(v) for v in tree["children"][i])
        if c0 == 0:
            out.append(i)
        else:
            stack += [c1, c0]
    return out


def test_read_sdt_agrees_with_the_oracles_own_view_of_its_dump(oracle_lib, tmp_path):
    import ppg_host
    e = make_oracle(oracle_lib, budget=12, seed=1, **CBOX_PROPS)
    # budget 12 = 3 passes: iteration 0 trains with one, iteration 1 is final with two (renderSPP) — and a final iteration records nothing, so the
    # tree a whole render() leaves is empty.  The dump is taken where the dumpSDTree property takes it: at the end of the training iteration.
    e.set_scene(ppg_host.cbox_scene(24, 24)); e.begin_render()
    e.begin_iteration(False); e.render_passes(1); e.build_sdtree()
    path = str(tmp_path / "o.sdt")
    e.dump_sdtree(path)
    f = ppg_host.read_sdt(path)
    t = e.read_sdtree()
    e.end_iteration(); e.begin_iteration(True); e.render_passes(2); e.build_sdtree(); e.end_iteration(); e.end_render()
    s = t["sampling"]
    kept = [i for i in _leaves_depth_first(t) if s["stat_weight"][i] > 0]
    assert len(kept) >= 1 and len(f["leaves"]) == len(kept) and max(l["num_nodes"] for l in f["leaves"]) > 1
    assert f["camera"].shape == (4, 4) and abs(f["camera"][0, 3] - 278) < 1e-3
    for leaf, i in zip(f["leaves"], kept):
        o, n = int(s["offset"][i]), int(s["num_nodes"][i])
        assert leaf["num_nodes"] == n and leaf["weight"] == int(s["stat_weight"][i])
        assert leaf["node_children"].dtype == np.uint16 and np.array_equal(leaf["node_children"], s["node_children"][o:o + n])
        assert leaf["node_sums"].dtype == np.float32 and np.array_equal(leaf["node_sums"].view(np.uint32), s["node_sums"][o:o + n].view(np.uint32))
        assert np.all(leaf["size"] > 0) and np.all(leaf["p"] >= t["aabb_min"]) and np.all(leaf["p"] + leaf["size"] <= t["aabb_max"] + 1e-3)
    # the framing is checked: a cut file is an error, not a short list
    cut = str(tmp_path / "cut.sdt")
    open(cut, "wb").write(open(path, "rb").read()[:-7])
    with pytest.raises(ValueError, match="truncated"):
        ppg_host.read_sdt(cut)


def test_cli_takes_the_iteration_from_the_name_the_dump_property_gives():
    """endIteration (ppg_hip.hip; GP:1417-1422) writes "<dest>-%02d.sdt" with m_iter and increments it afterwards: the context that wrote
    -NN went on with NN + 1."""
    from ppg_host.__main__ import parse_args, sdtree_iter_from_name
    assert sdtree_iter_from_name("/some/where/kitchen-06.sdt") == 7 and sdtree_iter_from_name("out-00.sdt") == 1
    assert sdtree_iter_from_name("out-6.sdt") is None and sdtree_iter_from_name("out-06.sdt.bak") is None and sdtree_iter_from_name("tree.sdt") is None
    a = parse_args(["scene.xml", "--sdtree", "renders/cbox-02.sdt"])[1]
    assert a.sdtree_iter == 3 and a.sdtree_passes is None and not a.guide_only
    a = parse_args(["scene.xml", "--sdtree", "renders/cbox-02.sdt", "--sdtree-iter", "5", "--guide-only"])[1]
    assert a.sdtree_iter == 5 and a.guide_only
    a = parse_args(["scene.xml", "--sdtree", "tree.sdt", "--sdtree-iter", "0", "--sdtree-passes", "0"])[1]
    assert a.sdtree_iter == 0 and a.sdtree_passes == 0


@pytest.mark.parametrize("argv,part", [
    (["scene.xml", "--sdtree", "tree.sdt"], "--sdtree-iter is required"),
    (["scene.xml", "--guide-only"], "need --sdtree"),
    (["scene.xml", "--sdtree", "a-01.sdt", "--sdtree-iter", "31"], "0 .. 30"),
])
def test_cli_refuses_what_it_cannot_resolve(argv, part, capsys):
    from ppg_host.__main__ import parse_args
    with pytest.raises(SystemExit) as ei:
        parse_args(argv)
    assert ei.value.code == 2 and part in capsys.readouterr().err


def test_guide_only_needs_a_tree():
    import ppg_host
    with pytest.raises(ValueError):
        ppg_host.GuidedPathTracer(engine=object(), guide_only=True)


def test_the_ctypes_mirror_of_the_options_has_the_headers_layout(tmp_path):
    import ctypes as C
    from ppg_host import bindings as b
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppg.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(ppg_sdtree_load), '
                   'offsetof(ppg_sdtree_load, passes_rendered), offsetof(ppg_sdtree_load, _reserved)); return 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(b.SDTreeLoad), b.SDTreeLoad.passes_rendered.offset, b.SDTreeLoad._reserved.offset] == [16, 4, 8]
