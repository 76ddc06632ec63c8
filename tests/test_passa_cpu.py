"""CPU: what the search kernel that walks nothing does behind its pre-filter, by tests/hostsim/passa_check.cpp with the
rules as rm_scan_core.h states them for host and device (the cases: tests/passa_cases.py).

  * the end window: every record of the oracle has its bit in E at the end of the first element's group, and where E is
    decided it says what the rule says base by base; where there is no end window the program says so;
  * pass A' on quads of lanes gives every item the (keep, hm0, hm1) of the sequential loop it replaces -- outer helices of
    1, 2, 3 and 4 lengths, a head_pre of one value and of a range, masks wanted and not wanted;
  * the checker once more, built with -fsanitize=address,undefined, over the short entries."""
import os
import subprocess

import pytest

import passa_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
HOST = ("rm_regex.cpp", "rm_compile.cpp", "rm_parse.cpp", "rm_score.cpp", "rm_efndata.cpp", "rm_efn2data.cpp", "rm_fasta.cpp",
        "rm_driver.cpp", "rm_cli.cpp", "rm_dump.cpp", "rm_pack.cpp", "rm_stream.cpp", "rm_dev_program.cpp")
ORACLE = ("rm_oracle_scan.c", "rm_oracle_efn.c", "rm_oracle_efn2.c")
ENV = dict(os.environ, EFNDATA=os.path.join(ROOT, "rnamotif_amd", "efndata"))


def build(name, flags):
    """tests/_build/NAME from the checker, the scanner's host sources and the oracle's, all with the same flags"""
    out = os.path.join(ROOT, "tests", "_build", name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "hostsim", "passa_check.cpp")] + [os.path.join(H, f) for f in HOST]
    csrcs = [os.path.join(ROOT, "oracle", f) for f in ORACLE]
    deps = srcs + csrcs + [os.path.join(H, f) for f in ("rm_scan_core.h", "rm_dev_program.h")]
    if os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(d) for d in deps):
        return out
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + H, "-I" + os.path.join(ROOT, "oracle")]
    objs = []
    for c in csrcs:
        objs.append(out + "." + os.path.basename(c) + ".o")
        subprocess.run(["gcc"] + flags + ["-Wno-unused-function", "-c", c, "-o", objs[-1]] + inc, check=True)
    subprocess.run(["g++"] + flags + ["-std=c++17", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + inc + ["-o", out] + srcs + objs + ["-lm"],
                   check=True)
    return out


def run(checker, dbfile, name, cwd, env=ENV):
    p = subprocess.run([checker, dbfile, "-descr", name], cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, (name, p.stdout.decode(), p.stderr.decode())
    fields = {}
    for line in p.stdout.decode().splitlines():
        w = line.split()
        if w[0] == "records":
            fields.update(records=int(w[1]), checked=int(w[3]), lost=int(w[5]), wrong=int(w[7]), set=int(w[9]), decided=int(w[11]))
        elif w[0] == "items":
            fields.update(items=int(w[1]), differ=int(w[3]), kept=int(w[5]), masked=int(w[7]))
        else:
            fields.update({k: int(v) for k, v in (x.split("=") for x in w[1:])})
    return fields


@pytest.fixture(scope="module")
def files(workdir, tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("passa"))
    for name, text in PC.WRITTEN.items():
        with open(os.path.join(workdir, name), "w") as f:
            f.write(text)
    out = {}
    for which, seqs in PC.databases().items():
        out[which] = os.path.join(tmp, which + ".txt")
        with open(out[which], "wb") as f:
            f.write(b"\n".join(seqs) + b"\n")
    return out


@pytest.fixture(scope="module")
def results(files, workdir):
    checker = build("passa_check", ["-O2"])
    return {name: run(checker, files["long"], name, workdir) for name in PC.NAMES}


@pytest.mark.parametrize("name", PC.NAMES)
def test_end_window_loses_no_candidate(results, name):
    f = results[name]
    assert f["records"] > 0, f                  # (the oracle finds something)
    assert f["lost"] == 0 and f["wrong"] == 0, f
    if name == "tail_no_leaf.descr":
        assert f["on"] == 0 and f["checked"] == 0, f        # (the interior ends with a helix that is no leaf: the program says so)
    else:
        # every record, in the entry as one tile and in tiles of 96 and 512; E decides, and clears most end positions
        assert f["on"] == 1 and f["checked"] == 3 * f["records"] and f["d_hi"] - f["d_lo"] < 24, f
        assert 0 < f["set"] < f["decided"] / 2, f


def test_end_window_ranges(results):
    # trna.descr: outer helix 6 .. 7, T arm 4 .. 5 pairs around 7 bases, nothing behind it: 6 + 8 + 7 - 1 .. 7 + 8 + 7 + 1 - 1
    assert (results["trna.descr"]["d_lo"], results["trna.descr"]["d_hi"]) == (20, 22)
    # tail_2x2.descr: 4 .. 5, ss 1 .. 3, 4 .. 5 pairs around 4 .. 5 bases: 4 + 1 + 8 + 4 - 1 .. 5 + 3 + 8 + 5 + 1 - 1
    assert (results["tail_2x2.descr"]["d_lo"], results["tail_2x2.descr"]["d_hi"]) == (16, 21)
    # two_leaves.descr: 4 .. 6, ss 1, 5 pairs around 3 .. 5 bases
    assert (results["two_leaves.descr"]["d_lo"], results["two_leaves.descr"]["d_hi"]) == (17, 21)


@pytest.mark.parametrize("name", PC.NAMES)
def test_quads_equal_the_sequential_loop(results, name):
    f = results[name]
    assert f["differ"] == 0 and f["items"] > 100_000 and 0 < f["kept"] < f["items"], f
    assert f["tail"] == 1 or f["head"] == 1, f


def test_quads_cases_cover_lengths_offsets_and_masks(results):
    r = results
    assert {r[n]["lengths"] for n in ("outer_one.descr", "trna.descr", "two_leaves.descr", "outer_four.descr")} == {1, 2, 3, 4}
    assert r["trna.descr"]["pre"] == 1 and r["head_range.descr"]["pre"] == 3
    assert r["trna.descr"]["tail"] == 1 and r["trna.descr"]["head"] == 1
    # masks wanted (the head helix next to a leaf, one offset: some item keeps a mask that restricts) and not wanted
    for n in ("trna.descr", "two_leaves.descr", "outer_four.descr"):
        assert r[n]["head_next"] == 1 and r[n]["masked"] > 0, (n, r[n])
    for n in ("wide_loop.descr", "head_range.descr", "tail_no_leaf.descr"):
        assert r[n]["masked"] == 0, (n, r[n])


def test_checker_under_sanitizers(files, workdir):
    checker = build("passa_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    # (the descriptor front end frees nothing at exit: what is looked for here are reads and writes out of bounds and undefined arithmetic)
    env = dict(ENV, ASAN_OPTIONS="detect_leaks=0")
    for name in PC.NAMES:
        f = run(checker, files["short"], name, workdir, env)
        assert f["lost"] == 0 and f["wrong"] == 0 and f["differ"] == 0 and f["items"] > 10_000, (name, f)
