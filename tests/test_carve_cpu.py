"""CPU: where the scratch arrays of the calls over device records lie (rnamotif_amd/csrc/rm_hitpost.h, carved with
rm_scanner_impl.h's Carver), printed by tests/hostsim/carve_check.cpp.  The expected offsets are the chains of running
offsets the library computed by hand before it had the carver, written out here once more."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "_build", "carve_check")
HW_CHUNK = 1 << 17
PRUNE_WG = 256
PRUNE_CASES = [(n, row) for n in (1, 129, 1 << 17) for row in (1, 7)]


def align256(x):
    return (x + 255) & ~255


@pytest.fixture(scope="module")
def carved():
    """the checker's lines by their first words"""
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "hostsim", "carve_check.cpp")
    newest = max(os.path.getmtime(f) for f in (src, os.path.join(H, "rm_hitpost.h"), os.path.join(H, "rm_scanner_impl.h")))
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < newest:
        # (the headers compile like rm_scanner.cpp: g++ with the ROCm headers)
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                        "-I" + os.path.join(ROOT, "include"), "-I" + H, "-o", BIN, src], check=True)
    args = [str(HW_CHUNK)] + [str(v) for case in PRUNE_CASES for v in case]
    p = subprocess.run([BIN] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0, p.stderr.decode()
    out = {}
    for line in p.stdout.decode().splitlines():
        w = line.split()
        if w[0] == "win":
            out["win"] = [int(v) for v in w[1:]]
        else:
            out[(int(w[1]), int(w[2]))] = [int(v) for v in w[3:]]
    return out


def test_window_scratch(carved):
    """lo[ chunk ] | len[ chunk + 1 ] | off[ chunk + 1 ] | src[ chunk ] | bad[ HB_SLOTS ] | letters[ 256 ] on the device,
    off[ chunk + 1 ] | lo[ chunk ] | bad[ HBH_SLOTS ] | letters[ 256 ] page-locked: the named refusal words of
    rm_hitpost.h, which fit the 256 bytes an array has at least."""
    o_len = align256(HW_CHUNK * 4)
    o_off = o_len + align256((HW_CHUNK + 1) * 8)
    o_src = o_off + align256((HW_CHUNK + 1) * 8)
    o_bad = o_src + align256(HW_CHUNK * 8)
    o_tab = o_bad + 256
    h_lo = align256((HW_CHUNK + 1) * 8)
    h_bad = h_lo + align256(HW_CHUNK * 4)
    h_tab = h_bad + 256
    assert carved["win"] == [HW_CHUNK, 0, o_len, o_off, o_src, o_bad, o_tab, o_tab + 256, 0, h_lo, h_bad, h_tab, h_tab + 256]


@pytest.mark.parametrize("n,row", PRUNE_CASES)
def test_prune_scratch(carved, n, row):
    """hdr[ n ][ 4 ] | rows[ n ][ row ] | bflag[ n ] | part[ parts ] | part_x[ parts ] | blocks[ n ]"""
    parts = (n + PRUNE_WG - 1) // PRUNE_WG
    o_rows = align256(n * 16)
    o_bflag = o_rows + align256(n * row * 4)
    o_part = o_bflag + align256(n)
    o_part_x = o_part + align256(parts * 8)
    o_blocks = o_part_x + align256(parts * 8)
    total = o_blocks + align256(n * 8)
    assert carved[(n, row)] == [parts, 0, o_rows, o_bflag, o_part, o_part_x, o_blocks, total]
