"""CPU: the owners of device memory, page-locked memory, streams and events (rnamotif_amd/csrc/rm_hip_own.h) against a
counting fake of the runtime, tests/hostsim/own_check.cpp: room() and exact(), the empty state after a failure, moves,
a stream's synchronise-then-destroy, and a first use that is built in locals and moved in -- failed at every call it
makes.  The same program built with -fsanitize=address,undefined runs all of it clean."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "hostsim", "own_check.cpp")
BUILDS = {"plain": [], "sanitized": ["-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def own_check(request):
    out = os.path.join(ROOT, "tests", "_build", "own_check" + ("" if request.param == "plain" else "_san"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    newest = max(os.path.getmtime(f) for f in (SRC, os.path.join(H, "rm_hip_own.h")))
    if not os.path.exists(out) or os.path.getmtime(out) < newest:
        # (the header compiles like rm_scanner.cpp: g++ with the ROCm headers; the program links no ROCm library)
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-result", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                        "-I" + H] + BUILDS[request.param] + ["-o", out, SRC], check=True)
    return out


def test_owners(own_check):
    p = subprocess.run([own_check], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    err = p.stderr.decode()
    assert p.returncode == 0, err[-3000:]
    assert p.stdout.decode().strip() == "own_check: ok"
    assert "AddressSanitizer" not in err and "runtime error" not in err, err[-3000:]
