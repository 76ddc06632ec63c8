"""CPU: the launch shape that leaves another scanner's drain kernel room (option beside, rm_launch_plan.cpp) over the
descriptors, databases and option sets of tests/test_launch_plan.py on a device of 256 CUs, and the count of scans in
flight that decides who plans that way (rm_flight_count.h) from eight threads, plain and under the sanitizers."""
import os
import subprocess

import numpy as np
import pytest

from test_launch_plan import CUS, DESCRS, H, OPTS, ROOT, cases, databases, descr_path

BUILD = os.path.join(ROOT, "tests", "_build")
BIN = os.path.join(BUILD, "beside_plan_check")
CU_LDS = 160 * 1024
KEY = ("tile_t", "dminlen", "strands", "group", "qcap", "concat", "flush", "n_tiles")


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """case id -> {"solo" | "b0" | "b1": fields of the layout key and the plan}, for every case of test_launch_plan.cases()"""
    os.makedirs(BUILD, exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "hostsim", "beside_plan_check.cpp")]
    srcs += [os.path.join(H, f) for f in ("rm_launch_plan.cpp", "rm_regex.cpp", "rm_compile.cpp", "rm_parse.cpp", "rm_score.cpp",
                                          "rm_efndata.cpp", "rm_efn2data.cpp", "rm_fasta.cpp", "rm_driver.cpp", "rm_cli.cpp",
                                          "rm_dump.cpp", "rm_pack.cpp", "rm_stream.cpp", "rm_dev_program.cpp")]
    newest = max(os.path.getmtime(s) for s in srcs + [os.path.join(H, f) for f in ("rm_launch_plan.h", "rm_kernels.h", "rm_diag.h", "rm_dev_program.h")])
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < newest:
        subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                        "-I" + os.path.join(ROOT, "include"), "-I" + H, "-o", BIN] + srcs + ["-lm"], check=True)
    tmp = str(tmp_path_factory.mktemp("beside"))
    files = {}
    for name, (lens, ranges, asc) in databases().items():
        np.asarray(lens, dtype=np.int32).tofile(os.path.join(tmp, name + ".len"))
        rng = "-"
        if ranges is not None:
            rng = os.path.join(tmp, name + ".rng")
            np.asarray(ranges, dtype=np.int32).tofile(rng)
        files[name] = (os.path.join(tmp, name + ".len"), rng, int(asc))
    env = dict(os.environ, EFNDATA=os.path.join(ROOT, "rnamotif_amd", "efndata"))
    got = {}
    for d in DESCRS:
        lines = []
        for (dd, b, o) in cases():
            if dd != d:
                continue
            env_o, sets = OPTS[o]
            opts = dict(sets)
            opts.update({k.replace("RNAMOTIF_", "").lower(): v for k, v in env_o.items()})
            lines.append("%s|%s|%s %s %s %d %s" % (d, b, o, *files[b], ",".join("%s=%s" % kv for kv in opts.items()) or "-"))
        cf = os.path.join(tmp, "cases.txt")
        with open(cf, "w") as f:
            f.write("\n".join(lines) + "\n")
        p = subprocess.run([BIN, cf, "-descr", descr_path(d, tmp)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
        assert p.returncode == 0, p.stderr.decode()
        for line in p.stdout.decode().splitlines():
            w = line.split()
            assert w[2] != "ERR", line
            got.setdefault(w[0], {})[w[1]] = {k: int(v) for k, v in (x.split("=") for x in w[2:])}
    assert sorted(got) == sorted("%s|%s|%s" % c for c in cases())
    return got


def test_beside_off_is_the_solo_plan(plans):
    """beside = 0 and the default (-1, which plan_launch reads as off) reproduce the plan field for field."""
    for cid, p in plans.items():
        assert p["b0"] == p["solo"], cid
        assert p["solo"]["beside"] == 0, cid


def test_beside_leaves_the_drain_kernel_room(plans):
    """beside = 1, the instance that walks nothing: at most four workgroups a CU and five that do not fit one, LDS left
    for two to four drain waves a CU, and the instance, the tile and the layout key of the solo plan.  Every other
    instance: the solo plan."""
    n_beside = 0
    for cid, p in plans.items():
        solo, b1 = p["solo"], p["b1"]
        if not solo["nothing"]:
            assert b1 == solo, cid
            continue
        n_beside += 1
        assert b1["beside"] == 1, cid
        assert b1["grid"] <= 4 * CUS and b1["grid"] == min(solo["grid"], 4 * CUS), cid
        assert 5 * b1["lds"] > CU_LDS and b1["lds"] % 64 == 0 and b1["lds"] >= solo["lds"], cid
        per_cu = b1["drain_grid"] // CUS
        assert b1["drain_grid"] == per_cu * CUS and 2 <= per_cu <= 4, cid
        assert 4 * b1["lds"] + per_cu * (b1["drain_lds"] + 64) <= CU_LDS, cid
        same = KEY + ("inst", "tile_bytes", "lean", "grouped", "pooled", "nib", "drain_lds", "listed", "nothing", "light")
        assert {k: b1[k] for k in same} == {k: solo[k] for k in same}, cid
    assert n_beside >= 20       # (trna.descr and bulge.descr over every database, and the option sets that force the instance)


def test_beside_on_trna(plans):
    """The headline: 32 832 bytes a workgroup, 1024 workgroups, two drain waves a CU (a third finds LDS beside
    4 x 32 832 bytes but not beside the workgroups' 1152 bytes of static LDS as well)."""
    b1 = plans["trna|mb100|base"]["b1"]
    assert (b1["grid"], b1["lds"], b1["drain_grid"]) == (1024, 32832, 512)
    assert plans["trna|one6000|base"]["b1"]["grid"] == 2


@pytest.mark.parametrize("flags", [[], ["-fsanitize=thread"], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "tsan", "asan_ubsan"])
def test_flight_count_from_eight_threads(flags):
    """rm_flight_count.h through rma_scan_begin()'s guard, early returns included: a program of its own, run directly."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "flight_count_check" + "".join("_" + f.split("=")[-1].replace(",", "_") for f in flags[:1]))
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread"] + flags + ["-I" + H, "-o", exe,
                    os.path.join(ROOT, "tests", "hostsim", "flight_count_check.cpp")], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode()
    assert b" 0 violations" in p.stdout, p.stdout.decode()
