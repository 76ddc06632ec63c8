"""CPU: the rule of a scan's tail enqueued ahead of the count -- plan_tail() and tail_verdict() of
rnamotif_amd/csrc/rm_tail_plan.h -- over its edges, by tests/hostsim/tail_plan_check.cpp: no earlier scan, the least a tail is
planned for, the quarter above the most records seen, a hit buffer below that margin, every switch that turns it off; a count of
exactly the plan and one more, the hit buffer's last record and one more, every repeat condition, the ordering's flag, 0, 1 and 2
records; and a scanner's sequence of scans through both.  The same program built with -fsanitize=address,undefined runs clean."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "hostsim", "tail_plan_check.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def tail_plan_check(request):
    out = os.path.join(ROOT, "tests", "_build", "tail_plan_check" + ("" if request.param == "plain" else "_san"))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    newest = max(os.path.getmtime(f) for f in (SRC, os.path.join(H, "rm_tail_plan.h")))
    if not os.path.exists(out) or os.path.getmtime(out) < newest:
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + H] + BUILDS[request.param] + ["-o", out, SRC], check=True)
    return out


def test_tail_plan(tail_plan_check):
    p = subprocess.run([tail_plan_check], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    out, err = p.stdout.decode(), p.stderr.decode()
    assert p.returncode == 0, (out[-3000:], err[-3000:])
    assert out.strip() == "tail_plan_check: ok"
    assert "AddressSanitizer" not in err and "runtime error" not in err, err[-3000:]

