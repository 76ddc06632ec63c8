"""CPU: the cases of tests/test_flush_vectors_gpu.py run the code they are there for.  tests/hostsim/flush_cases_check.cpp
builds each descriptor's device program and launch plans with the host sources the scanner uses (as
tests/test_launch_plan.py does) and prints the look-ahead chain and the search instance of every case:

  * wide_loop.descr: three groups -- a leaf, a group that is none with a range of lengths of 64 or more (the chain's
    `len` window in chunks), a leaf whose helix has more than one length (the `t` window);
  * two_leaves.descr: two leaves with different core slots and a group between them;
  * trna.descr, bulge.descr: a chain with a leaf;
  * every descriptor, both databases: RNAMOTIF_SHORT = 0 launches RMK_LEAN_FLUSH at every tile size; 1 the groups of
    small tiles (option `flush` does not apply there); 2 launches RMK_LEAN_CONCAT_FLUSH at the default tile size (and
    bulge.descr at 2048) for all but wide_loop.descr, whose window the layout over the concatenation does not take."""
import os
import subprocess

import numpy as np
import pytest

import flush_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "_build", "flush_cases_check")


@pytest.fixture(scope="module")
def checker():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "hostsim", "flush_cases_check.cpp")]
    srcs += [os.path.join(H, f) for f in ("rm_launch_plan.cpp", "rm_regex.cpp", "rm_compile.cpp", "rm_parse.cpp", "rm_score.cpp",
                                          "rm_efndata.cpp", "rm_efn2data.cpp", "rm_fasta.cpp", "rm_driver.cpp", "rm_cli.cpp",
                                          "rm_dump.cpp", "rm_pack.cpp", "rm_stream.cpp", "rm_dev_program.cpp")]
    newest = max(os.path.getmtime(s) for s in srcs + [os.path.join(H, f) for f in ("rm_launch_plan.h", "rm_kernels.h", "rm_diag.h", "rm_dev_program.h")])
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < newest:
        subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                        "-I" + os.path.join(ROOT, "include"), "-I" + H, "-o", BIN] + srcs + ["-lm"], check=True)
    return BIN


@pytest.fixture(scope="module")
def dumps(checker, workdir, tmp_path_factory):
    """descriptor -> (the chain's line, its groups, {case id: fields})"""
    tmp = str(tmp_path_factory.mktemp("flush_cases"))
    for name, text in FC.WRITTEN.items():
        with open(os.path.join(workdir, name), "w") as f:
            f.write(text)
    lines = []
    for which, seqs in FC.databases().items():
        path = os.path.join(tmp, which + ".i32")
        np.asarray([len(s) for s in seqs], dtype=np.int32).tofile(path)
        for short in FC.SHORT:
            for tile in FC.TILE:
                opts = "flush=1,short=%s" % short + (",tile=%s" % tile if tile else "")
                lines.append("%s/%s/%s %s %s" % (which, short, tile or "default", path, opts))
    cases = os.path.join(tmp, "cases.txt")
    with open(cases, "w") as f:
        f.write("\n".join(lines) + "\n")
    env = dict(os.environ, EFNDATA=os.path.join(ROOT, "rnamotif_amd", "efndata"))
    out = {}
    for name in FC.NAMES:
        p = subprocess.run([checker, cases, "-descr", name], cwd=workdir, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        assert p.returncode == 0, p.stderr.decode()
        fields = lambda words: {k: (int(v) if v.lstrip("-").isdigit() else v) for k, v in (w.split("=") for w in words)}
        chain, sibs, got = None, [], {}
        for line in p.stdout.decode().splitlines():
            w = line.split()
            if w[0] == "chain":
                chain = fields(w[1:])
            elif w[0] == "sib":
                sibs.append(fields(w[1:]))
            else:
                assert w[0] == "case" and w[2] != "ERR", line
                got[w[1]] = fields(w[2:])
        assert len(got) == len(lines), name
        out[name] = (chain, sibs, got)
    return out


def test_wide_loop_has_a_group_wider_than_a_word(dumps):
    chain, sibs, _ = dumps["wide_loop.descr"]
    assert chain["on"] == 1 and chain["n"] == 3, (chain, sibs)
    assert [s["leaf"] for s in sibs] == [1, 0, 1], sibs
    assert sibs[1]["len_hi"] - sibs[1]["len_lo"] >= 64, sibs       # (the `len` window over the next group's vector, in chunks)
    assert sibs[2]["tmax"] > 0 and sibs[0]["lmax"] > sibs[0]["lmin"], sibs


def test_two_leaves_have_two_core_slots(dumps):
    chain, sibs, _ = dumps["two_leaves.descr"]
    assert chain["on"] == 1 and chain["n"] == 3, (chain, sibs)
    assert [s["leaf"] for s in sibs] == [1, 0, 1], sibs
    assert {sibs[0]["core_slot"], sibs[2]["core_slot"]} == {0, 1}, sibs
    assert (sibs[0]["hmin"], sibs[0]["lmin"], sibs[0]["lmax"]) != (sibs[2]["hmin"], sibs[2]["lmin"], sibs[2]["lmax"]), sibs


@pytest.mark.parametrize("name", FC.NAMES)
def test_the_flush_instances_are_launched(dumps, name):
    chain, sibs, got = dumps[name]
    assert chain["on"] == 1 and any(s["leaf"] for s in sibs), (chain, sibs)
    for cid, f in got.items():
        which, short, tile = cid.split("/")
        if short == "1":
            assert f["inst"] == "lean_group" and f["grouped"] == 1 and f["nothing"] == 0, (cid, f)
        else:
            assert f["inst"] == ("lean_concat_flush" if f["concat"] else "lean_flush") and f["nothing"] == 1, (cid, f)
            assert f["concat"] == 0 or short == "2", (cid, f)
    # Tiles over the concatenation are laid where the other pooled instance would fit the tile (choose_layout): at the
    # default tile size for the descriptors whose window is short enough for it -- not wide_loop.descr's 113 bases.
    for which in ("short", "long"):
        assert got[which + "/0/default"]["inst"] == got[which + "/0/512"]["inst"] == "lean_flush"
        if name != "wide_loop.descr":
            assert got[which + "/2/default"]["inst"] == "lean_concat_flush", got[which + "/2/default"]
    if name == "bulge.descr":
        assert got["long/2/2048"]["inst"] == "lean_concat_flush"
