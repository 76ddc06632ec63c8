"""CPU: the launch shapes of scans (rnamotif_amd/csrc/rm_launch_plan.cpp, the functions rm_scanner.cpp calls)
for the golden descriptors over databases of every shape and the option sets the GPU tests use, on a device of
256 CUs.  tests/golden/launch_plan.txt pins, for each case, the layout key, the number of tiles, a hash of the
three tile arrays and the launch plan; it was recorded from the scanner on an MI355X."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from rnamotif_amd import DBG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "tests", "_build", "launch_plan_check")
PINNED = os.path.join(GOLDEN, "launch_plan.txt")
CUS = 256

WIDE = "descr\n\th5(minlen=20,maxlen=110,mispair=1)\n\t\tss(minlen=3,maxlen=8)\n\th3\n"     # a helix of 64 to 127 pairs
DESCRS = {"trna": "descr/trna.descr", "pk1": "descr/pk1.descr", "ire": "test/ire.descr", "mp.ends": "test/mp.ends.descr",
          "qu+tr": "test/qu+tr.descr", "pk_j1+2": "test/pk_j1+2.descr", "bulge": "test/bulge.descr", "dp.wide": None}


def descr_path(name, tmpdir):
    if DESCRS[name] is None:
        path = os.path.join(tmpdir, name + ".descr")
        with open(path, "w") as f:
            f.write(WIDE)
        return path
    return os.path.join(GOLDEN, DESCRS[name])


def _real_lengths():
    lens, n = [], -1
    with gzip.open(os.path.join(GOLDEN, "test", "gbrna.111.0.fastn.gz"), "rb") as f:
        for line in f:
            if line.startswith(b">"):
                lens.append(0)
            else:
                lens[-1] += sum(1 for c in line if chr(c).isalpha())
    return lens


def databases():
    """name -> (entry lengths, start-position ranges or None, entries ascending in the packed arrays)"""
    short = [60 + (i * 7919) % 900 for i in range(4096)]
    return {"mb100": ([1_000_000] * 100, None, True),
            "real44": (_real_lengths() * 44, None, True),           # the reference's test database x 44: 179 k entries
            "short": (short, None, True),
            "one6000": ([6000], None, True),                        # (the general instance's smaller tiles)
            "long": ([2 ** 31 - 1], None, True),
            "ranges": ([50_000] * 8, [(1000 * i, 30_000 + 5000 * i) for i in range(8)], True),
            "unasc": ([2000] * 100, None, False)}


# option set -> (environment when the scanner is created, rma_scanner_set_option() afterwards)
OPTS = {"base": ({}, {}), "pool0": ({}, {"pool": 0}), "drain0": ({}, {"drain": 0}),
        "flush0": ({}, {"flush": 0}), "flush1": ({}, {"flush": 1}), "flush-1": ({}, {"flush": -1}),
        "short0": ({}, {"short": 0}), "short1": ({}, {"short": 1}), "short2": ({}, {"short": 2}),
        "dbg16": ({}, {"dbg": DBG["GENERAL"]}), "dbg2048": ({}, {"dbg": DBG["POOL_DROP"]}), "dbg8388608": ({}, {"dbg": DBG["LIST_ALL"]}),
        "dbg2097152": ({}, {"dbg": DBG["WHOLE_ITEMS"]}), "glist7": ({}, {"glist": 7}),
        "qcap64": ({"RNAMOTIF_QCAP": "64"}, {}), "tile4096": ({"RNAMOTIF_TILE": "4096"}, {}),
        "efn0": ({}, {"efn_light": 0}), "efn1": ({}, {"efn_light": 1})}


def cases():
    """(descriptor, database, option set) in the order of the pinned table"""
    out = [(d, b, "base") for d in DESCRS for b in databases()]
    out += [(d, b, o) for o in OPTS if o != "base" for d in ("trna", "mp.ends", "bulge", "pk1")
            for b in ("mb100", "real44", "short", "one6000")]
    out += [("trna", "long", o) for o in OPTS if o != "base"]
    return out


@pytest.fixture(scope="module")
def checker():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "hostsim", "launch_plan_check.cpp")]
    srcs += [os.path.join(H, f) for f in ("rm_launch_plan.cpp", "rm_regex.cpp", "rm_compile.cpp", "rm_parse.cpp", "rm_score.cpp",
                                          "rm_efndata.cpp", "rm_efn2data.cpp", "rm_fasta.cpp", "rm_driver.cpp", "rm_cli.cpp",
                                          "rm_dump.cpp", "rm_pack.cpp", "rm_stream.cpp", "rm_dev_program.cpp")]
    newest = max(os.path.getmtime(s) for s in srcs + [os.path.join(H, f) for f in ("rm_launch_plan.h", "rm_kernels.h", "rm_diag.h", "rm_dev_program.h")])
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < newest:
        # (rm_launch_plan.cpp compiles like rm_scanner.cpp: g++ with the ROCm headers, for rm_kernels.h)
        subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                        "-I" + os.path.join(ROOT, "include"), "-I" + H, "-o", BIN] + srcs + ["-lm"], check=True)
    return BIN


@pytest.fixture(scope="module")
def table(checker, tmp_path_factory):
    """what the checker prints for every case, in the order of cases()"""
    tmp = str(tmp_path_factory.mktemp("plan"))
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
        p = subprocess.run([checker, cf, "-descr", descr_path(d, tmp)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=env, timeout=600)
        assert p.returncode == 0, p.stderr.decode()
        for line in p.stdout.decode().splitlines():
            got[line.split(" ", 1)[0]] = line
    return ["%s|%s|%s" % c for c in cases()], got


def test_plans_equal_the_recorded_ones(table):
    """Every case: layout key, tiles, the tile arrays' hash and the launch plan as the scanner chose them."""
    ids, got = table
    with open(PINNED) as f:
        pinned = {line.split(" ", 1)[0]: line.rstrip("\n") for line in f}
    assert sorted(pinned) == sorted(ids)
    bad = [(pinned[i], got.get(i)) for i in ids if got.get(i) != pinned[i]]
    assert not bad, "%d of %d cases differ, first: %s" % (len(bad), len(ids), bad[0])


def test_tile_lines(table):
    """A few tiles' lines word by word (RMK_META_SEQ, COMP, Z0, SLEN, OFF_LO, OFF_HI, POS_HI, PAD): the first and last
    of the entry of 2^31 - 1 bases, the last of 100 entries of 1 Mbase, and concatenation tiles that span entries."""
    _, got = table
    fields = {k: dict(w.split("=", 1) for w in got[k].split()[1:]) for k in
              ("trna|long|base", "trna|mb100|base", "trna|real44|base", "pk_j1+2|real44|base")}
    assert fields["trna|long|base"]["m0"] == "0:0,0,0,2147483647,0,0,2147483647,0"
    assert fields["trna|long|base"]["mN"] == "541201:0,1,2147481600,2147483647,0,0,2147483647,0"
    assert fields["trna|mb100|base"]["mN"] == "25399:99,1,999936,1000000,99000000,0,2147483647,0"
    assert fields["trna|real44|base"]["span"] == "0:0,0,0,102429184,0,0,2147483647,31"
    assert fields["pk_j1+2|real44|base"]["mN"] == "66685:178939,0,102428160,102429184,0,0,2147483647,9"
