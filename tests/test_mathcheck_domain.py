"""The domain predicate of include/ppg_mathcheck.h — "every C++ step is defined for this input" — under the undefined-behaviour sanitizer:
tests/mathcheck_domain_check.cpp is compiled with it (float-to-integer conversions included) and run as a child process, nothing is loaded into
this interpreter.  It evaluates every op on a stride through all float patterns, on every pattern near the edges of the domains and
branches, and on the special values; an input the predicate admits and C++ does not define ends the program."""
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
    exe = str(tmp_path_factory.mktemp("mathcheck") / "mathcheck_domain_check")
    subprocess.check_call([CXX, "-std=c++14", "-O1", "-g", "-Wall", "-Werror", "-Wno-unused-function", "-ffp-contract=off",
                           "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "mathcheck_domain_check.cpp")])
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, env=env)
    print(run.stdout)
    print(run.stderr)
    return run


def test_every_input_of_a_domain_is_defined_cxx(check_output):
    assert check_output.returncode == 0, check_output.stdout[-4000:] + check_output.stderr[-4000:]
    assert "all checks passed" in check_output.stdout and "FAILED" not in check_output.stdout
    assert "runtime error" not in check_output.stderr


def test_the_sweep_is_not_vacuous(check_output):
    m = re.search(r"mathcheck: (\d+) inputs evaluated inside their domains, (\d+) outside and skipped", check_output.stdout)
    assert m, check_output.stdout[-2000:]
    assert int(m.group(1)) > 10_000_000 and int(m.group(2)) > 100_000  # ten one-argument ops x a million patterns; sincos, tan, adam refuse most
