"""CPU: the windows of hit records that Replay.device() cuts out of a device database's text (rnamotif_amd/csrc/
rm_hitwin.h, shared by the kernels of rm_hitwin_dev.hip and the host) against the host's own ways of rebuilding a
hit's text, through tests/hostsim/hit_windows_check.cpp:

  * the letter and span rule equal PackFile::window over the reader-normalised text, both strands;
  * Replayer::replay_windows prints exactly the bytes Replayer::replay (whole strands, revcomp()) and
    Replayer::replay_packed print, and its `accepted` agrees with the number printed;
  * hitwin_span's checks (entry, strand, every element and context inside the entry, in 64 bits) equal a
    statement of them in Python.

The entries are the reference's test database with raw bytes mixed in -- upper case, U, IUPAC letters, '-', NUL,
0xff -- as text on a GPU may hold them; the records are the oracle's scan of the normalised entries."""
import os
import subprocess

import numpy as np
import pytest

import pins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "tests", "_build", "hit_windows_check")
ODD = np.frombuffer(b"acgtuACGTUacgtacgtnNrRyYwWsSkKmMbBdDhHvV-.*\n\x00\xff\x80 ", dtype=np.uint8)
LOOSE = {"literal_n": 'parms\n\tiupac = 0;\ndescr\n\tss(minlen=4,maxlen=5,seq="^nnac")\n',
         "backref": 'descr\n\th5(minlen=2,maxlen=3)\n\t\tss(minlen=5,maxlen=7,seq="^\\(a[cg]\\)g\\1")\n\th3\n'}


@pytest.fixture(scope="module")
def checker():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "hostsim", "hit_windows_check.cpp")]
    srcs += [os.path.join(H, f) for f in ("rm_regex.cpp", "rm_compile.cpp", "rm_parse.cpp", "rm_score.cpp", "rm_efndata.cpp",
                                          "rm_efn2data.cpp", "rm_fasta.cpp", "rm_driver.cpp", "rm_cli.cpp", "rm_dump.cpp",
                                          "rm_pack.cpp", "rm_stream.cpp", "rm_dev_program.cpp")]
    newest = max(os.path.getmtime(s) for s in srcs + [os.path.join(H, f) for f in ("rm_hitwin.h", "rm_driver.h")])
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < newest:
        subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + H, "-o", BIN]
                       + srcs + ["-lm"], check=True)
    return BIN


def normalise(raw: bytes) -> bytes:
    """The readers' letters of raw bytes, as Replay.device() reads them."""
    import rnamotif_amd as R
    return bytes(R.reader_letter(b) for b in raw)


def odd_entries(gbrna, seed=5, rate=0.01, limit=None):
    """The reference's test database (its first `limit` entries), the letters in mixed case, some t as u, and a few odd
    bytes at random positions; plus entries of 0, 1 and 33 odd bytes."""
    import rnamotif_amd as R
    rng = np.random.default_rng(seed)
    out = []
    for k, (_, _, s) in enumerate(R.read_fasta(gbrna)[:limit]):
        a = np.frombuffer(s, dtype=np.uint8).copy()
        if k % 3 == 0:
            a = np.frombuffer(s.upper(), dtype=np.uint8).copy()
        if k % 3 == 1:
            a[a == ord("t")] = ord("u")
        at = rng.random(a.size) < rate
        a[at] = ODD[rng.integers(0, ODD.size, size=int(at.sum()))]
        out.append(a.tobytes())
    out += [ODD[rng.integers(0, ODD.size, size=n)].tobytes() for n in (0, 1, 33)]
    return out


def _write_entries(path, entries):
    with open(path, "wb") as f:
        f.write(np.asarray([len(entries)] + [len(e) for e in entries], dtype=np.int32).tobytes())
        f.write(b"".join(entries))


def _run(checker, tmp, mode, entries, records, argv, cwd=None):
    ent, rec = os.path.join(tmp, "entries.bin"), os.path.join(tmp, "records.bin")
    _write_entries(ent, entries)
    np.ascontiguousarray(records, dtype=np.int32).tofile(rec)
    env = dict(os.environ, EFNDATA=os.path.join(ROOT, "rnamotif_amd", "efndata"))
    p = subprocess.run([checker, mode, ent, rec, tmp if mode == "replay" else "-"] + argv, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=env, cwd=cwd, timeout=600)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout.decode()


def _cases(workdir):
    """(name, rnamotif arguments, working directory)"""
    out = [("trna", ["-descr", os.path.join(GOLDEN, "descr", "trna.descr")], None),
           ("score.2", ["-descr", "score.2.descr"], workdir),
           ("trna.strict", pins.STRICT_ARGS + ["-descr", "trna.strict.descr"], workdir),
           ("getbest.strict", pins.STRICT_ARGS + ["-descr", "getbest.strict.descr"], workdir)]
    for name, text in LOOSE.items():
        path = os.path.join(workdir, "loose_%s.descr" % name)
        with open(path, "w") as f:
            f.write(text)
        out.append(("loose_" + name, ["-descr", os.path.basename(path)], workdir))
    return out


@pytest.mark.parametrize("case", range(6), ids=["trna", "score.2", "trna.strict", "getbest.strict", "loose_literal_n", "loose_backref"])
def test_windows_replay_as_whole_strands(built, checker, gbrna, workdir, tmp_path, case):
    import rnamotif_amd as R
    from oracle_binding import oracle_scan
    name, argv, cwd = _cases(workdir)[case]
    old = os.getcwd()
    os.chdir(cwd or old)
    try:
        d = R.Descriptor(argv)
    finally:
        os.chdir(old)
    entries = odd_entries(gbrna)
    recs = oracle_scan(d, [normalise(e) for e in entries])
    assert recs.shape[0] > 0, name
    # the records as the scan gave them, and shuffled (a subset in any order prints in the order given)
    rng = np.random.default_rng(case)
    for records in (recs, recs[rng.permutation(recs.shape[0])]):
        out = _run(checker, str(tmp_path), "replay", entries, records, argv, cwd=cwd)
        f = dict(zip(out.split()[0::2], map(int, out.split()[1::2])))
        assert f["records"] == records.shape[0] and f["mismatches"] == 0, out
        assert f["accepted"] == f["hits"], out
        want = (tmp_path / "replay.out").read_bytes()
        assert (tmp_path / "packed.out").read_bytes() == want
        assert (tmp_path / "windows.out").read_bytes() == want
        if name == "trna":
            assert f["hits"] > 0 and want.count(b"\n>") + want.startswith(b">") == f["hits"]


def _span_py(w, n_elems, ctx_off, lctx, rctx, slen):
    """hitwin_span restated: (code, lo, hi, which)"""
    seq, comp = int(w[0]), int(w[1])
    if seq < 0 or seq >= len(slen):
        return (1, 0, 0, -1)
    if comp not in (0, 1):
        return (2, 0, 0, -1)
    n = slen[seq]
    lo, hi = n, 0
    items = [(e, 5 + 4 * e) for e in range(n_elems)]
    if lctx:
        items.append((n_elems, ctx_off))
    if rctx:
        items.append((n_elems + 1, ctx_off + 2))
    for e, k in items:
        off, ln = int(w[k]), int(w[k + 1])
        if off < 0 or ln < 0 or off + ln > n:
            return (3, 0, 0, e)
        if ln > 0:
            lo, hi = min(lo, off), max(hi, off + ln)
    return (0, lo, hi, -1)


@pytest.mark.parametrize("strict", [False, True])
def test_span_checks(built, checker, workdir, tmp_path, strict):
    import rnamotif_amd as R
    argv = (pins.STRICT_ARGS if strict else []) + ["-descr", "trna.strict.descr" if strict else "trna.descr"]
    old = os.getcwd()
    os.chdir(workdir)
    try:
        d = R.Descriptor(argv)
    finally:
        os.chdir(old)
    rng = np.random.default_rng(9)
    slen = [0, 1, 33, 2 ** 31 - 1, 500, 90]
    entries = [b"a" * n for n in slen[:3]] + [b""] + [b"c" * n for n in slen[4:]]
    m = 4000
    recs = np.zeros((m, d.hit_stride), dtype=np.int32)
    recs[:, 0] = rng.choice([-1, 0, 1, 2, 3, 4, 5, 6, 2 ** 31 - 1], size=m, p=[.02, .1, .1, .1, .3, .2, .14, .02, .02])
    recs[:, 1] = rng.choice([0, 1, 2, -1], size=m, p=[.48, .48, .02, .02])
    big = np.array([0, 1, 2, 5, 40, 89, 90, 2 ** 30, 2 ** 31 - 2, 2 ** 31 - 1, -1, -2 ** 31], dtype=np.int64)
    pw = np.array([.1, .1, .1, .2, .2, .1, .05, .03, .03, .03, .03, .03])
    for k in range(5, d.hit_stride):
        recs[:, k] = big[rng.choice(big.size, size=m, p=pw / pw.sum())].astype(np.int32)
    # the entry of 2^31 - 1 bases is declared, not held: only its length is read
    slen_decl = [len(e) for e in entries]
    slen_decl[3] = 2 ** 31 - 1
    ent = os.path.join(str(tmp_path), "entries.bin")
    with open(ent, "wb") as f:
        f.write(np.asarray([len(entries)] + slen_decl, dtype=np.int32).tobytes())
    rec = os.path.join(str(tmp_path), "records.bin")
    recs.tofile(rec)
    env = dict(os.environ, EFNDATA=os.path.join(ROOT, "rnamotif_amd", "efndata"))
    p = subprocess.run([checker, "span", ent, rec, "-"] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env,
                       cwd=workdir, timeout=600)
    assert p.returncode == 0, p.stderr.decode()
    got = [tuple(map(int, line.split())) for line in p.stdout.decode().splitlines()]
    want = [_span_py(w, d.n_elems, d.ctx_off, strict, strict, slen_decl) for w in recs]
    assert got == want
    assert {g[0] for g in got} == {0, 1, 2, 3}


def test_descriptor_loose(built, tmp_path):
    import rnamotif_amd as R
    assert R.Descriptor(["-descr", os.path.join(GOLDEN, "descr", "trna.descr")]).loose == 0
    for name, text in LOOSE.items():
        path = tmp_path / (name + ".descr")
        path.write_text(text)
        assert R.Descriptor(["-descr", str(path)]).loose == 1, name


def test_header_declares_the_device_replay():
    text = open(os.path.join(ROOT, "include", "rnamotif_amd.h")).read()
    assert "int\trma_replay_device( rma_replay_t *rp, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits," in text
    assert "rma_program_loose(" in text


def test_reader_letters(built):
    import rnamotif_amd as R
    want = {b: (b | 0x20) for b in range(256) if chr(b).isascii() and chr(b).isalpha()}
    want[ord("u")] = want[ord("U")] = ord("t")
    assert bytes(R.reader_letter(b) for b in range(256)) == bytes(want.get(b, ord("n")) for b in range(256))
    tab = R.alphabet_letters("acgU")
    assert tab[:4] == b"acgt" and tab[4:] == b"n" * 252
    assert R.alphabet_letters("NRy-")[:4] == b"nryn"
