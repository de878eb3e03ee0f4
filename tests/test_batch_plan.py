"""The decisions of renderBatch (csrc/ppg_batch_plan.h) on the host alone: tests/batch_plan_check.cpp is compiled with the address and
undefined-behaviour sanitizers and run as a child process — no context, no device, nothing loaded into this interpreter.  The program compares
planBatch with the inline rule it replaced over the full product of the facts, asserts the invariants of a plan on every case, compares
planBounces with the loop it replaced over a seeded sweep of survival curves and on the cases whose answer can be derived by hand, and pins the
layout of the pinned read-back block.  No picture can show a scheduling mistake (every schedule renders the same bits): this can."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CXX = os.environ.get("CXX", "c++")


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    if not shutil.which(CXX):
        pytest.fail("no host C++ compiler found (set CXX)")
    exe = str(tmp_path_factory.mktemp("batch_plan") / "batch_plan_check")
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(ROOT, "tests", "batch_plan_check.cpp")])
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)
    print(run.stdout)
    print(run.stderr)
    return run


def test_every_check_of_the_program_passes_under_the_sanitizers(check_output):
    assert check_output.returncode == 0, check_output.stdout[-4000:] + check_output.stderr[-4000:]
    assert "all checks passed" in check_output.stdout and "FAILED" not in check_output.stdout
    assert "runtime error" not in check_output.stderr and "AddressSanitizer" not in check_output.stderr


def test_the_plan_equals_the_inline_rule_on_the_full_product_of_the_facts(check_output):
    m = re.search(r"planBatch: (\d+) cases compared with the inline rule, (\d+) differing", check_output.stdout)
    assert m, check_output.stdout[-2000:]
    # 9 booleans x bounded / unbounded x 3 path counts x 3 spatial filters x 3 nee modes x 2 split depths x 2 defer depths x 2 thresholds x 3 tree sizes
    assert int(m.group(1)) == 512 * 2 * 3 * 3 * 3 * 2 * 2 * 2 * 3
    assert int(m.group(2)) == 0


def test_the_bounce_predictor_equals_the_inline_loop(check_output):
    m = re.search(r"planBounces: (\d+) curves compared with the inline rule, (\d+) differing", check_output.stdout)
    assert m, check_output.stdout[-2000:]
    assert int(m.group(1)) == 200000 and int(m.group(2)) == 0


def test_the_header_needs_no_device_toolchain():
    text = open(os.path.join(ROOT, "practical-path-guiding_amd", "csrc", "ppg_batch_plan.h")).read()
    includes = re.findall(r"^\s*#\s*include\s*[<\"]([^>\"]+)[>\"]", text, re.M)
    assert includes and all(not i.startswith("hip") and not i.startswith("ppg") for i in includes), includes
    assert "ppg_ctx" not in text
