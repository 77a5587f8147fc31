"""pa::eq_any (csrc/pa_eq_any.h, the equality prefilter of the lane-major scan) on the host: tests/native/eq_any_check.cpp
is compiled with the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer and run as a child process.

For every width nb in 1..32 it compares eq_any with a per-doc decode on random lanes and on planted ones: one match in
every doc position (doc 0, doc 31 and every doc whose field straddles a word boundary among them), runs of 2..5
adjacent matches, every doc one bit off the value (with and without one match among them), v - 1 / v + 1 neighbours,
dictId 0 and 2^nb - 1, no match at all, all docs matching. Required: no false negative (a tile would be skipped
wrongly) and, as the zero-field test is exact, no false positive either.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "eq_any_check.cpp")
CSRC = os.path.join(ROOT, "pinot_amd", "csrc")


def _host_compiler():
    """The host compiler of the build (hipcc's clang++), else the system's C++ compiler."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for c in (os.path.join(os.path.dirname(os.path.dirname(hipcc)), "llvm", "bin", "clang++"), shutil.which("g++"),
              shutil.which("c++")):
        if c and os.path.exists(c):
            yield c


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("eq_any") / "eq_any_check")
    errors = []
    for cxx in _host_compiler():
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
               "-I", CSRC, SRC, "-o", exe]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode == 0:
            break
        errors.append("%s: %s" % (cxx, p.stderr[-2000:]))
    else:
        pytest.fail("no host compiler built the check:\n" + "\n".join(errors))
    return subprocess.run([exe], capture_output=True, text=True, timeout=300)


def test_eq_any_matches_the_per_doc_decode(report):
    assert report.returncode == 0, (report.stdout[-3000:], report.stderr[-3000:])
    assert "ERROR" not in report.stderr and "runtime error" not in report.stderr, report.stderr[-3000:]
    lines = dict((int(m.group(1)), tuple(int(x) for x in m.groups()[1:])) for m in
                 re.finditer(r"^nb=(\d+) cases=(\d+) false_neg=(\d+) false_pos=(\d+)$", report.stdout, re.M))
    assert sorted(lines) == list(range(1, 33)), sorted(lines)
    for nb, (cases, neg, pos) in lines.items():
        assert cases >= 1000, (nb, cases)
        assert neg == 0, (nb, neg)
        assert pos == 0, (nb, pos)
