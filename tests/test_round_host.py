"""pa::i128_to_double and pa::sum_pair_to_i128 (csrc/pa_round.h, the final rounding of the integer accumulators in
compact_final_kernel) on the host: tests/native/round_check.cpp is compiled with the host compiler under
AddressSanitizer + UndefinedBehaviorSanitizer and run as a child process.

It compares the header's double bit for bit with the compiler's (double)(__int128) and the (high, low) recombination
with ((__int128)hs << 32) + ls: m * 2^k + r around every rounding decision (below, at and above the tie, even and odd
significands, the carry of an all-ones significand into the next binade), both signs, the powers of two and their
neighbours up to 2^127, the int64 extremes sign-extended, partial sums whose low part has crossed 2^32, 2^63 and
2^64 - 1 under high parts of both signs, totals that cancel, and more than 2 * 10^6 random values of every width up to
96 bits. Required: no mismatch at all, and no sanitizer report.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "round_check.cpp")
CSRC = os.path.join(ROOT, "pinot_amd", "csrc")

# the designed sets and the least number of cases each must report (round_check.cpp: 4 m * 43 k * up to 6 r * 2 signs
# less the r that fall outside [0, 2^k) at k = 1; 4 * 43 * 2 * 2 ties; ...)
MIN_CASES = {"designed_rounding": 2000, "ties": 688, "landmarks": 45, "recombination": 2 * 23 * 12 + 2 * 93,
             "random_pairs": 1200000, "random_widths": 1000000}


def _host_compiler():
    """The host compiler of the build (hipcc's clang++), else the system's C++ compiler."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for c in (os.path.join(os.path.dirname(os.path.dirname(hipcc)), "llvm", "bin", "clang++"), shutil.which("g++"),
              shutil.which("c++")):
        if c and os.path.exists(c):
            yield c


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("round") / "round_check")
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


def test_rounding_and_recombination_match_int128(report):
    assert report.returncode == 0, (report.stdout[-3000:], report.stderr[-3000:])
    assert "ERROR" not in report.stderr and "runtime error" not in report.stderr, report.stderr[-3000:]
    assert "MISMATCH" not in report.stderr, report.stderr[-3000:]
    lines = dict((m.group(1), (int(m.group(2)), int(m.group(3)))) for m in
                 re.finditer(r"^(\w+) cases=(\d+) mismatches=(\d+)$", report.stdout, re.M))
    total = lines.pop("TOTAL")
    assert sorted(lines) == sorted(MIN_CASES), sorted(lines)
    for name, (cases, bad) in lines.items():
        assert cases >= MIN_CASES[name], (name, cases)
        assert bad == 0, (name, bad)
    assert total == (sum(c for c, _ in lines.values()), 0), total
    assert total[0] >= 10 ** 6 + MIN_CASES["designed_rounding"] + MIN_CASES["ties"]
