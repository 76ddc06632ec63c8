"""CPU: the premises of tests/test_scan_end_gpu.py, by the oracle and the device program's dump alone (tests/scan_end_cases.py
holds the cases): every count the GPU test relies on, the flags and order bits of every descriptor, the widths of the ordering's
key over the database of the clamped order field, the order words the lean kernels leave before the ordering, and that the
host's sort_hits() leaves the oracle's records as they are.  tests/hostsim/order_plan_check.cpp, which prints the dump, runs
here plain and under the sanitizers, a program of its own."""
import os
import subprocess

import numpy as np
import pytest

import scan_end_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
HOST_SRCS = ("rm_regex.cpp", "rm_compile.cpp", "rm_parse.cpp", "rm_score.cpp", "rm_efndata.cpp", "rm_efn2data.cpp", "rm_fasta.cpp",
             "rm_driver.cpp", "rm_cli.cpp", "rm_dump.cpp", "rm_pack.cpp", "rm_stream.cpp", "rm_dev_program.cpp")
HDR = 5


def _build_dump(flags, suffix):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "order_plan_check" + suffix)
    srcs = [os.path.join(ROOT, "tests", "hostsim", "order_plan_check.cpp")] + [os.path.join(H, f) for f in HOST_SRCS]
    newest = max(os.path.getmtime(s) for s in srcs + [os.path.join(H, "rm_dev_program.h")])
    if not os.path.exists(exe) or os.path.getmtime(exe) < newest:
        subprocess.run(["g++", "-std=c++17", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
                        "-I" + H] + flags + ["-o", exe] + srcs + ["-lm"], check=True)
    return exe


def _dump(exe, path):
    """({field: value} of the first line, [(ord_stride, ord_nlen) per search level])"""
    # (the front end frees nothing of a descriptor before it exits, like the reference's: no leak report)
    env = dict(os.environ, EFNDATA=os.path.join(ROOT, "rnamotif_amd", "efndata"), ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, "-descr", path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    lines = p.stdout.decode().splitlines()
    w = lines[0].split()
    head = {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)}
    levels = []
    for line in lines[1:]:
        w = line.split()
        assert w[0] == "level" and w[4] == "ord_stride" and w[6] == "ord_nlen", line
        levels.append((int(w[5]), int(w[7])))
    return head, levels


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return SC.write_all(tmp_path_factory.mktemp("scan_end"))


@pytest.fixture(scope="module")
def dumps(paths):
    exe = _build_dump(["-O2"], "")
    return {name: _dump(exe, path) for name, path in paths.items()}


_WANT = {}


def oracle(built, paths, name, key, entries):
    """the oracle's records of descriptor name over entries(), once per (name, key)"""
    import rnamotif_amd as R
    from oracle_binding import oracle_scan
    if (name, key) not in _WANT:
        d = R.Descriptor(["-descr", paths[name]])
        _WANT[(name, key)] = (d, oracle_scan(d, entries()))
    return _WANT[(name, key)]


def _parts(w, k):
    """lengths of the k single strands behind the first element of record w"""
    return [int(w[HDR + 4 * (1 + i) + 1]) for i in range(k)]


def _sorted_as_is(want):
    import rnamotif_amd as R
    assert np.array_equal(R.sort_hits(want.copy()), want)


def test_flags_and_order_bits(dumps):
    assert sorted(dumps) == sorted(SC.FLAGS)
    for name, (lean_ok, ord_ok, ord_bits, winsize, n_efn, efn_big) in SC.FLAGS.items():
        h, levels = dumps[name]
        assert (h["lean_ok"], h["ord_ok"], h["w_winsize"], h["n_efn"], h["efn_big"]) == (lean_ok, ord_ok, winsize, n_efn, efn_big), (name, h)
        assert h["ord_bits"] in (ord_bits if isinstance(ord_bits, range) else (ord_bits,)), (name, h)
    # the weights of SS6's levels as walk_number() has them: 21^4 .. 21, 1 for the two last
    m = SC.SS6_MAXLEN
    assert [s for s, _ in dumps["ss6.descr"][1]][1:] == [m ** 4, m ** 3, m ** 2, m, 1, 1]
    assert all(n == 1 for _, n in dumps["ss6.descr"][1])
    # DEEP: the walks outnumber 2^31, so its order words are counts; its hit records are the widest here
    assert dumps["deep.descr"][0]["hit_stride"] == HDR + 4 * 19 + 4 and len(dumps["deep.descr"][1]) == 16


def test_dump_under_the_sanitizers(paths, dumps):
    exe = _build_dump(["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "_asan_ubsan")
    for name, path in paths.items():
        assert _dump(exe, path) == dumps[name], name


def test_hit_buffer_edge_counts(built, paths):
    """L - 3 windows an entry: the three databases around the cap, the one that grows it again and the small ones, by
    construction and by the oracle"""
    for count, _ in SC.SS4_FRESH + SC.SS4_GROWN:
        seqs = SC.ss4_entries(count)
        assert SC.ss4_count(seqs) == count
        assert min(len(s) for s in seqs) < 4 and (count < 8 or len(seqs) >= 8)
        d, want = oracle(built, paths, "ss4_one.descr", count, lambda: seqs)
        assert want.shape[0] == count and not d.both_strands
        assert np.all(want[:, 4] == 0)
        _sorted_as_is(want)
    assert [c for c, _ in SC.SS4_FRESH] == [SC.HIT_CAP - 1, SC.HIT_CAP, SC.HIT_CAP + 1]
    # (the first regrow left room for count + 1024 records: the second one's database is beyond that, the third scan's within)
    assert SC.SS4_GROWN[0][0] > 3 * SC.HIT_CAP > SC.SS4_FRESH[2][0] + 1024 and SC.SS4_GROWN[1][0] == SC.SS4_FRESH[2][0]
    seqs = SC.ss4_entries(SC.SS4_BOTH_WINDOWS)
    d, want = oracle(built, paths, "ss4_both.descr", 0, lambda: seqs)
    assert d.both_strands and want.shape[0] == SC.HIT_CAP + 2 == SC.ss4_count(seqs, 2)
    _sorted_as_is(want)


@pytest.mark.parametrize("name,entries", [("pk.descr", SC.pk_entries), ("dense.descr", SC.dense_entries)])
def test_regrow_counts(built, paths, name, entries):
    """one regrow, not two: between 2^17 and 2^18 records"""
    _, want = oracle(built, paths, name, 0, entries)
    assert SC.HIT_CAP < want.shape[0] < 2 * SC.HIT_CAP
    assert len(set(want[:, 1].tolist())) == 2
    _sorted_as_is(want)


@pytest.mark.parametrize("name", ["hairpin_efn.descr", "hairpin_efn2.descr"])
def test_energy_counts(built, paths, name):
    """more records than a pass of either energy kernel takes on EFN_CUS CUs, and a quarter more; energies that differ"""
    d, want = oracle(built, paths, name, 0, SC.hairpin_entries)
    assert d.n_efn_sites == 1
    assert want.shape[0] > SC.efn_need(SC.EFN_CUS, True) > SC.efn_need(SC.EFN_CUS, False)
    assert want.shape[0] < 4 * SC.HIT_CAP
    assert len(np.unique(want[:, d.efn_off])) > 50
    _sorted_as_is(want)


def test_order_words_of_ss6(built, paths, dumps):
    """Case 4: 2 ( 1 + C( 16, 5 ) + C( 19, 5 ) ) records, and among the words the kernels leave (walk_number) some of 2^20 and
    more, all within ord_bits"""
    _, want = oracle(built, paths, "ss6.descr", 0, SC.ss6_entries)
    m = SC.SS6_MAXLEN
    assert want.shape[0] == 2 * sum(SC.compositions(d, 6, m) for d in (6, 17, 20)) == 2 * (1 + 4368 + 11628)
    words = [SC.walk_number(_parts(w, 6), m) for w in want]
    assert max(words) >= 1 << SC.W_ORD and max(words) < 1 << dumps["ss6.descr"][0]["ord_bits"]
    assert min(words) == 0
    # (the walk takes the alternatives in the order of these numbers: within a start position the oracle's records ascend in them)
    for k in range(1, len(words)):
        if tuple(want[k, :4]) == tuple(want[k - 1, :4]):
            assert words[k] > words[k - 1] and want[k, 4] == want[k - 1, 4] + 1
    _sorted_as_is(want)


def test_clamped_key(built, paths, dumps):
    """Case 5: entry, strand, position and rank take 17 + 1 + 22 + 8 bits of SS6's key and leave the order word 16 -- with the
    field at 20 bits and at 31 --, which SS6's words outgrow and SMALL's do not (17 + 1 + 22 + 5: 19 bits left of 20)"""
    seqs = SC.clamp_entries()
    assert len(seqs) == SC.CLAMP_SHORT + 1 and all(len(s) == 1 for s in seqs[:-1]) and len(seqs[-1]) == SC.CLAMP_LONG
    assert set(seqs[-1]) <= set(b"acg")
    bits = SC.key_bits(seqs, dumps["ss6.descr"][0]["w_winsize"])
    assert bits == (17, 1, 22, 8)
    left = 64 - sum(bits)
    assert left == 16 and sum(bits) + SC.W_ORD > 64 and left >= 4
    _, want = oracle(built, paths, "ss6.descr", "clamp", lambda: seqs)
    m = SC.SS6_MAXLEN
    assert want.shape[0] == 6 * (SC.compositions(20, 6, m) + SC.compositions(10, 6, m))
    assert set(want[:, 0].tolist()) == {SC.CLAMP_SHORT}
    starts = sorted(set(want[want[:, 1] == 0][:, 2].tolist()))
    assert starts[0] < 600 and starts[-1] > SC.CLAMP_LONG - 600 and any(abs(s - (1 << 20)) < 600 for s in starts)
    assert want[:, 2].max() >= 1 << 21
    assert max(SC.walk_number(_parts(w, 6), m) for w in want) >= 1 << left
    _sorted_as_is(want)
    bits = SC.key_bits(seqs, dumps["small.descr"][0]["w_winsize"])
    assert bits == (17, 1, 22, 5) and sum(bits) + SC.W_ORD > 64
    _, small = oracle(built, paths, "small.descr", "clamp", lambda: seqs)
    assert small.shape[0] == 6 * SC.compositions(10, 3, 6) == 162
    assert dumps["small.descr"][0]["ord_bits"] <= 64 - sum(bits)
    _sorted_as_is(small)


def test_piece_overflow_counts(built, paths):
    """Case 6: one start position, one end of the head helix and more than 2^12 records -- the dense site --, and a sparse
    database of three sites with fewer"""
    _, dense = oracle(built, paths, "deep.descr", "dense", SC.deep_dense_entries)
    assert dense.shape[0] == SC.compositions(SC.DEEP_DENSE_D, SC.DEEP_PARTS, SC.DEEP_MAXLEN) == 43747
    assert 10 * (1 << SC.PIECE_ORDER_BITS) < dense.shape[0] < SC.HIT_CAP
    assert len(set(map(tuple, dense[:, :4].tolist()))) == 1          # (entry, strand, start, rank: one item)
    assert len(set(map(tuple, dense[:, HDR + 4:HDR + 4 + 2].tolist()))) == 1    # (the head helix: one 5' strand ...)
    assert len(set(map(tuple, dense[:, HDR + 12:HDR + 12 + 2].tolist()))) == 1  # (... and one 3' strand)
    assert np.array_equal(dense[:, 4], np.arange(dense.shape[0]))
    _sorted_as_is(dense)
    _, sparse = oracle(built, paths, "deep.descr", "sparse", SC.deep_sparse_entries)
    per = [SC.compositions(d, SC.DEEP_PARTS, SC.DEEP_MAXLEN) for d in SC.DEEP_SPARSE_D]
    assert per == [11, 1, 66] and sparse.shape[0] == sum(per)
    assert [int((sparse[:, 0] == i).sum()) for i in range(3)] == per
    _sorted_as_is(sparse)


def test_single_records(built, paths, dumps):
    """Case 7: one record, order word 0, on a lean instance with numbered walks, on one with counted walks, on a general one"""
    kinds = []
    for k, (name, seqs) in enumerate(SC.single_cases()):
        _, want = oracle(built, paths, name, ("single", k), lambda: seqs)
        assert want.shape[0] == 1 and want[0, 4] == 0, name
        kinds.append((dumps[name][0]["lean_ok"], dumps[name][0]["ord_ok"]))
        _sorted_as_is(want)
    assert kinds == [(1, 1), (1, 0), (0, 0)]
    # ONE: the record's first single strand has ONE_TAKEN bases where the walk began with ONE_FIRST; the level has a weight
    _, want = _WANT[("one.descr", ("single", 0))]
    interior = int(want[0, HDR + 4 * 6] - (want[0, HDR] + 3))      # (between the strands of the outer helix, elements 0 and 6)
    assert int(want[0, HDR + 4 + 1]) == SC.ONE_TAKEN and min(5, interior - 11) == SC.ONE_FIRST
    stride, nlen = dumps["one.descr"][1][1]
    assert (SC.ONE_FIRST - SC.ONE_TAKEN) * nlen * stride > 0
