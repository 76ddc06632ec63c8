"""CPU: the bit vector helpers of rnamotif_amd/csrc/rm_scan_core.h that the search kernel's pre-filters are made of,
compiled for the host by tests/hostsim/bitvec_check.cpp.

rmd_or_window( v, x, lo, hi, vec_bits ) must equal, bit for bit, the loop it replaces in the look-ahead chain and in
pass A' --  r = 0; for d in lo..hi: r |= rmd_bits64( v, x + d ) if 0 <= x + d and x + d + 96 <= vec_bits else all ones --
for vectors of 128, 192 and 8256 bits of densities 0, 0.02, 0.5 and 1, every x from -70 to vec_bits + 70, ranges of
hi - lo in {-1, 0, 1, 17, 31, 32, 63, 64, 65, 127, 300} with lo negative, zero and positive.

(The program checks nothing about the bases as bit planes: that part of the change was measured and taken out,
DESIGN.md 4.)  The vectors lie in heap blocks of exactly their size: the same program built with -fsanitize=address,undefined
reports a read outside them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "_build", "bitvec_check")


@pytest.fixture(scope="module")
def checker():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "hostsim", "bitvec_check.cpp")
    newest = max(os.path.getmtime(f) for f in (src, os.path.join(H, "rm_scan_core.h"), os.path.join(H, "rm_dev_program.h")))
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < newest:
        subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + H, "-o", BIN, src], check=True)
    return BIN


@pytest.fixture(scope="module")
def report(checker):
    """the program's lines as dictionaries, and what it wrote about mismatches"""
    p = subprocess.run([checker], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode in (0, 1), p.stderr.decode()
    lines = [line.split() for line in p.stdout.decode().splitlines()]
    return [dict(zip(w[0::2], map(int, w[1::2]))) for w in lines], p.stderr.decode()


def test_or_window_equals_the_loop(report):
    f, err = report
    # 3 sizes x 4 densities x ( vec_bits + 141 ) values of x x 5 values of lo x 11 widths
    assert f[0]["or_window"] == 4 * 5 * 11 * sum(n + 141 for n in (128, 192, 8256)), f
    assert f[0]["mismatches"] == 0, err
