"""CPU: how the energy kernel gets at the bases of a call (rm_seq_window.h's one fetch of a window,
rme_cand_t::fill_cache() in two passes), compiled for the host by tests/hostsim/efn_window_check.cpp and held to the
base-by-base rule, to the uncached bc()/bp() and to the oracle's energies on every candidate of the reference's test
database -- once as it is and once under the address and undefined-behaviour sanitizers, the packed words in heap
blocks of exactly their size (a stand-alone program: nothing is preloaded)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
SRCS = [os.path.join(ROOT, "tests", "hostsim", "efn_window_check.cpp")]
SRCS += [os.path.join(H, f) for f in ("rm_regex.cpp", "rm_compile.cpp", "rm_parse.cpp", "rm_score.cpp", "rm_efndata.cpp",
                                      "rm_efn2data.cpp", "rm_fasta.cpp", "rm_driver.cpp", "rm_cli.cpp", "rm_dump.cpp",
                                      "rm_pack.cpp", "rm_stream.cpp", "rm_dev_program.cpp")]
SRCS += [os.path.join(ROOT, "oracle", f) for f in ("rm_oracle_scan.c", "rm_oracle_efn.c", "rm_oracle_efn2.c")]
HDRS = [os.path.join(H, f) for f in ("rm_seq_window.h", "rm_efn_core.h", "rm_efn2_core.h", "rm_dev_program.h", "rm_pack.h")]
VARIANTS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                           "-static-libasan", "-static-libubsan"]}   # (the runtimes inside the program)


@pytest.fixture(scope="module")
def checkers():
    os.makedirs(BUILD, exist_ok=True)
    newest = max(os.path.getmtime(s) for s in SRCS + HDRS)
    bins, jobs = {}, []
    for name, flags in VARIANTS.items():
        bins[name] = os.path.join(BUILD, "efn_window_check_" + name)
        if not os.path.exists(bins[name]) or os.path.getmtime(bins[name]) < newest:
            jobs.append(subprocess.Popen(["g++", "-std=c++17", "-pthread"] + flags +
                                         ["-I" + os.path.join(ROOT, "include"), "-I" + H, "-I" + os.path.join(ROOT, "oracle"),
                                          "-o", bins[name]] + SRCS + ["-lm"]))
    for j in jobs:
        assert j.wait() == 0
    return bins


def _run(binary, args, cwd):
    env = dict(os.environ, EFNDATA=os.path.join(ROOT, "rnamotif_amd", "efndata"),
               ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([binary] + args, cwd=cwd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=1800)
    out = p.stdout.decode() + p.stderr.decode()
    assert p.returncode == 0, out[-3000:]
    return out


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_cloverleaf_windows_and_caches(checkers, workdir, variant):
    """(i) every start and length of a window on both strands, on entries shorter than a word, at the pack's first and
    last entry, with letters under the mask first, last and inside; (ii) all 1351 cloverleaf candidates of the
    database (trna.descr with its efn() site): none left out, every one short enough for the cache."""
    out = _run(checkers[variant], ["-descr", "trna.efn.descr", "gbrna.111.0.fastn"], workdir)
    m = re.search(r"windows: (\d+) checked \((\d+) over copies of their own words\), letters under the mask: (\d+) first, (\d+) last, (\d+) inner", out)
    assert m and int(m.group(1)) > 30000 and int(m.group(2)) > 10000 and min(int(m.group(k)) for k in (3, 4, 5)) > 0, out
    m = re.search(r"(\d+) candidates, (\d+) sites \((\d+) cached, (\d+) longer than the cache, (\d+) rejected\), 0 mismatches", out)
    assert m, out
    cands, sites, cached, longer, rejected = (int(g) for g in m.groups())
    assert cands == 1351 and sites == 1351 and cached == 1351 and longer == 0 and rejected == 0


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_efn2_and_own_pair_sets(checkers, workdir, gbrna, tmp_path, variant):
    """The same through rme2_site_energy (efn2() of the cloverleaves), and on hairpins paired by the descriptor's own
    pair set with g:a pairs, whose helices efn's walk can reject."""
    out = _run(checkers[variant], ["-descr", os.path.join(ROOT, "tests", "data", "trna.efn2.descr"), "gbrna.111.0.fastn"], workdir)
    # (two sites a candidate: the descriptor scores efn() next to efn2())
    assert re.search(r"1351 candidates, 2702 sites \(2702 cached, 0 longer than the cache, 0 rejected\), 0 mismatches", out), out
    small = tmp_path / "small.fastn"
    with open(gbrna, "rb") as f:
        small.write_bytes(b"".join(f.readlines()[:1500]))
    out = _run(checkers[variant], ["-descr", os.path.join(ROOT, "tests", "data", "hairpin.nostdbp.descr"), str(small)], workdir)
    m = re.search(r"(\d+) candidates, (\d+) sites \((\d+) cached, .* 0 mismatches", out)
    assert m and int(m.group(1)) > 0 and int(m.group(3)) > 0, out
