"""CPU: the start positions out of the start vector by one prefix sum a wave (the pre-filter of the search kernel that walks
nothing), by tests/hostsim/start_compact_check.cpp: over random words of every density, 0 .. 16 bits a lane, the prefix sum
hands on the same set of start positions per wave as the rounds of ballots it replaces, each exactly once, 64 at a time;
and once more built with -fsanitize=address,undefined, the wave's buffer in a heap block of exactly its 128 places."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "start_compact_check.cpp")


def build(name, flags):
    out = os.path.join(ROOT, "tests", "_build", name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not (os.path.exists(out) and os.path.getmtime(out) >= os.path.getmtime(SRC)):
        subprocess.run(["g++"] + flags + ["-std=c++17", "-o", out, SRC], check=True)
    return out


def run(checker, seed):
    p = subprocess.run([checker, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, (p.stdout.decode(), p.stderr.decode())
    w = p.stdout.decode().split()
    return {w[i]: int(w[i + 1]) for i in range(1, len(w) - 1, 2)}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_prefix_sum_hands_on_what_the_ballots_hand_on(seed):
    f = run(build("start_compact_check", ["-O2"]), seed)
    # 17 densities x 200 waves; every position once, in hand-offs of 64
    assert f["differ"] == 0 and f["waves"] == 17 * 200 and f["positions"] > 1_000_000, f
    assert f["rounds"] * 64 >= f["positions"] > (f["rounds"] - f["waves"]) * 64, f


def test_checker_under_sanitizers():
    f = run(build("start_compact_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]), 1)
    assert f["differ"] == 0 and f["positions"] > 1_000_000, f
