"""CPU: hit records as rnamotif prints them -- the '>sid sdef' line and the hit line of HitPrinter::print -- as
rnamotif_amd/csrc/rm_hitprint.h states them for the host and for the kernels of rm_hitprint_dev.hip, run on the host
through tests/hostsim/hit_print_check.cpp.  The test holds the rule to the host printer, whose output is pinned to the
reference's:

  * per case of test_hit_align_cpu.py: the oracle's records of the reference's test database through the host replay
    into a file; the header and the rule's bytes of the accepted records, with the replay's own score columns, are
    that file byte for byte, and its md5 is the reference's raw stdout's where tests/pins.py has one;
  * rows made by hand -- names of 1, 12, 13 and 99 bytes, the default name, with and without a definition, strand 1 at
    both ends of an entry, an offset and a length wider than %7d and %4d, score columns of 8 and of 40 bytes -- each
    against HitPrinter::print through Replay.batch;
  * the checker itself refuses (exit status 3) a record whose hitprint_size() is not the length of what the segments
    and hitprint_byte() produce, so every row above holds that too; a record that is not accepted has size 0;
  * the record check gives hitwin_span's codes, and HP_TEXT for a text_len outside its row."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import pins
from test_hit_align_cpu import CASES as ALIGN_CASES
from test_hit_align_cpu import DOT, _descr, hit_lines, records_of
from test_hit_structures_cpu import Program, program_of
from test_hit_windows_cpu import _span_py, _write_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "_build", "hit_print_check")
HDR = 5
HP_TEXT = 5         # rm_hitprint.h: HS_HELIX + 1

# The cases of test_hit_align_cpu.py, and trna with its score section: the workdir's trna.descr is the reference's
# test/trna.descr, which has none (every column is "   0.000"); trna.efn.descr there is descr/trna.descr, whose SCORE is
# sprintf( '%8.3f %8.3f', bits(...), efn(...) ) -- a string column that differs from record to record.
CASES = dict(ALIGN_CASES, **{"trna.efn": (["-descr", "trna.efn.descr"], None, pins.SLACK["trna.efn.descr"][0])})

# the reference's raw stdout per case (tests/pins.py), where it is pinned
MD5 = {"trna": pins.SLACK["trna.descr"][1], "trna.efn": pins.SLACK["trna.efn.descr"][1], "pk1": pins.SLACK["pk1.descr"][1], "qu+tr": pins.SLACK["qu+tr.descr"][1],
       "score.2": pins.SLACK["score.2.descr"][1], "trna.context": pins.STRICT["trna"][1], "dot": None}

# rows made by hand: no score section (the column is %8.3lf of 0.0, 8 bytes) and a string SCORE of 40 bytes
HAND = "descr\n\th5( len=3 )\n\t\tss( minlen=0, maxlen=4 )\n\th3\n"
HAND40 = HAND + "score\n\t{ SCORE = sprintf( '%s%s', '0123456789abcdefghij', 'ABCDEFGHIJ9876543210' ); }\n"


@pytest.fixture(scope="module")
def print_checker():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "hostsim", "hit_print_check.cpp")
    deps = [src] + [os.path.join(H, f) for f in ("rm_hitprint.h", "rm_hitalign.h", "rm_hitstruct.h", "rm_hitwin.h", "rm_score_fmt.h")]
    deps.append(os.path.join(ROOT, "include", "rnamotif_amd_program.h"))
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(f) for f in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + H, "-o", BIN, src], check=True)
    return BIN


def _write_inputs(tmp, d, entries, records, text_len, text_bytes):
    tmp = str(tmp)
    prog, ent, rec, sco = (os.path.join(tmp, f) for f in ("program.bin", "entries.bin", "records.bin", "scores.bin"))
    with open(prog, "wb") as f:
        f.write(C.string_at(d.program, C.sizeof(Program)))
    if entries and isinstance(entries[0], (bytes, bytearray)):
        _write_entries(ent, entries)
    else:                                   # (lengths alone: the record check)
        with open(ent, "wb") as f:
            f.write(np.asarray([len(entries)] + list(entries), dtype=np.int32).tobytes())
    records = np.ascontiguousarray(records, dtype=np.int32)
    records.tofile(rec)
    text_bytes = np.ascontiguousarray(text_bytes, dtype=np.uint8)
    assert text_bytes.ndim == 2 and text_bytes.shape[0] == len(records)
    with open(sco, "wb") as f:
        f.write(np.asarray([len(records), text_bytes.shape[1]], dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(text_len, dtype=np.int32).tobytes())
        f.write(text_bytes.tobytes())
    return prog, ent, rec, sco


def host_print(checker, tmp, d, entries, records, sids, sdefs, text_len, text_bytes, accept=None, expect=0):
    """The rule on the host: (off int64 [n+1], the bytes); with expect=1 the words of the refusal.  text_bytes: uint8
    [n, W], the score columns; text_len int32 [n]; accept: bool [n] or None (all)."""
    prog, ent, rec, sco = _write_inputs(tmp, d, entries, records, text_len, text_bytes)
    nam, out, acc = (os.path.join(str(tmp), f) for f in ("names.bin", "printed.bin", "accept.bin"))
    run = b"".join(a + b for a, b in zip(sids, sdefs))
    off = np.zeros(2 * len(sids) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for pair in zip(sids, sdefs) for x in pair])
    with open(nam, "wb") as f:
        f.write(off.tobytes())
        f.write(run)
    argv = [checker, "print", prog, ent, rec, nam, sco, out]
    if accept is not None:
        np.ascontiguousarray(accept, dtype=np.uint8).tofile(acc)
        argv.append(acc)
    p = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == expect, p.stderr.decode()
    if expect:
        return p.stderr.decode()
    raw = open(out, "rb").read()
    n = int(np.frombuffer(raw, dtype=np.int64, count=1)[0])
    assert n == len(records)
    o = np.frombuffer(raw, dtype=np.int64, count=n + 1, offset=8)
    data = raw[8 * (n + 2):]
    assert o[0] == 0 and o[-1] == len(data) and (np.diff(o) >= 0).all()
    return o, data


def host_check(checker, tmp, d, slens, records, text_len, width):
    """hitprint_check of every record: [(code, which)]"""
    n = len(records)
    prog, ent, rec, sco = _write_inputs(tmp, d, list(slens), records, text_len, np.zeros((n, width), dtype=np.uint8))
    q = subprocess.run([checker, "check", prog, ent, rec, "-", sco, "-"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert q.returncode == 0, q.stderr.decode()
    return [tuple(map(int, line.split())) for line in q.stdout.decode().splitlines()]


def field_lens(w, d, p):
    lens = [int(x) for x in w[HDR + 1:HDR + 4 * d.n_elems:4]]
    return ([int(w[d.ctx_off + 1])] if p.has_lctx else []) + lens + ([int(w[d.ctx_off + 3])] if p.has_rctx else [])


def score_columns(lines, recs, sids, slens, d, p):
    """The score column of every hit line, cut out by the lengths of what stands around it: %-12s of the name and a
    blank in front, " %d %7d %4d" and the fields behind.  (Lengths alone are taken from the record: the bytes around
    the column are compared with the rule's like every other byte.)  Returns (text_len int32 [n], text_bytes uint8 [n, W])."""
    cols = []
    for ln, w in zip(lines, recs):
        e, comp = int(w[0]), int(w[1])
        offset = int(slens[e]) - int(w[HDR]) if comp else int(w[HDR]) + 1
        total = sum(int(x) for x in w[HDR + 1:HDR + 4 * d.n_elems:4])
        tail = len(b" %d %7d %4d" % (comp, offset, total)) + sum(1 + max(k, 1) for k in field_lens(w, d, p))
        cols.append(ln[max(len(sids[e]), 12) + 1:len(ln) - tail])
    width = max([len(c) for c in cols] + [1])
    text = np.zeros((len(cols), width), dtype=np.uint8)
    for h, c in enumerate(cols):
        text[h, :len(c)] = np.frombuffer(c, dtype=np.uint8)
    return np.asarray([len(c) for c in cols], dtype=np.int32), text


def header_of(d):
    import rnamotif_amd as R
    buf = C.create_string_buffer(1 << 16)
    m = R.lib().rma_print_header(d._h, buf, len(buf))
    assert 0 < m < len(buf)
    return buf.raw[:m]


_results = {}


def case_result(name, gbrna, workdir, tmp_factory):
    """A case of test_hit_align_cpu.py: the replay's file, its accepted records in order and their score columns."""
    if name in _results:
        return _results[name]
    import rnamotif_amd as R
    from oracle_binding import oracle_scan
    argv, limit, _ = CASES[name]
    tmp = tmp_factory.mktemp("print_" + name.replace("+", "_"))
    if name == "dot":
        with open(os.path.join(workdir, "dot.descr"), "w") as f:
            f.write(DOT)
    d = _descr(argv, cwd=workdir)
    p = program_of(d)
    fasta = R.read_fasta(gbrna)[:limit]
    sids, sdefs, entries = [r[0] for r in fasta], [r[1] for r in fasta], [r[2] for r in fasta]
    recs = oracle_scan(d, entries)
    out = os.path.join(str(tmp), "hits.out")
    rp = R.Replay(d, out)
    n_printed = rp.batch(sids, sdefs, entries, recs)
    rp.close()
    text = open(out, "rb").read()
    lines = hit_lines(text)
    assert len(lines) == n_printed
    slens = [len(e) for e in entries]
    rows = records_of(lines, recs, sids, slens, d, p)
    text_len, text_bytes = score_columns(lines, recs[rows], sids, slens, d, p)
    r = {"d": d, "p": p, "entries": entries, "sids": sids, "sdefs": sdefs, "all": recs, "rows": rows, "recs": recs[rows], "text": text,
         "text_len": text_len, "text_bytes": text_bytes, "tmp": tmp}
    _results[name] = r
    return r


@pytest.mark.parametrize("name", sorted(CASES))
def test_lines_are_the_replays(built, print_checker, gbrna, workdir, tmp_path_factory, name):
    r = case_result(name, gbrna, workdir, tmp_path_factory)
    n = len(r["recs"])
    assert n >= 1 and (CASES[name][2] is None or n == CASES[name][2])
    off, data = host_print(print_checker, r["tmp"], r["d"], r["entries"], r["recs"], r["sids"], r["sdefs"], r["text_len"], r["text_bytes"])
    head = header_of(r["d"])
    assert head.count(b"\n") == 3 and head.startswith(b"#RM scored\n#RM descr ") and b"\n#RM dfile " in head
    assert head + data == r["text"]
    if MD5[name] is not None:
        assert hashlib.md5(head + data).hexdigest() == MD5[name]
    # a record's bytes are its two lines
    for h in (0, n // 2, n - 1):
        two = data[off[h]:off[h + 1]]
        assert two.startswith(b">" + r["sids"][int(r["recs"][h][0])] + b" ") and two.count(b"\n") == 2 and two.endswith(b"\n")
    assert (r["text_len"] >= 8).all()
    if name == "trna.efn":
        # a string SCORE made by sprintf(), with blanks inside and another one for nearly every record
        assert (r["text_len"] >= 17).all() and len({row.tobytes() for row in r["text_bytes"]}) > n // 2
        assert all(b" " in row.tobytes().strip(b"\0").strip() for row in r["text_bytes"][:20])
    if name == "dot":
        assert b" . " in data or b" .\n" in data
    if name == "trna.context":
        assert r["p"].has_lctx and r["p"].has_rctx


def test_not_accepted_is_size_zero(built, print_checker, gbrna, workdir, tmp_path_factory):
    r = case_result("qu+tr", gbrna, workdir, tmp_path_factory)
    n = len(r["recs"])
    args = (print_checker, r["tmp"], r["d"], r["entries"], r["recs"], r["sids"], r["sdefs"], r["text_len"], r["text_bytes"])
    off, data = host_print(*args)
    for mask in (np.ones(n, dtype=bool), np.zeros(n, dtype=bool), np.arange(n) % 3 != 1):
        o, got = host_print(*args, accept=mask)
        assert np.array_equal(np.diff(o), np.where(mask, np.diff(off), 0))
        assert got == b"".join(data[off[h]:off[h + 1]] for h in range(n) if mask[h])


def _hand(d, rows):
    """records of HAND: (entry, strand, offset of the h5, length of the ss)"""
    recs = np.zeros((len(rows), d.hit_stride), dtype=np.int32)
    for h, (e, comp, at, ss) in enumerate(rows):
        recs[h, 0], recs[h, 1] = e, comp
        for k, (o, ln) in enumerate(((at, 3), (at + 3, ss), (at + 3 + ss, 3))):
            recs[h, HDR + 4 * k], recs[h, HDR + 4 * k + 1] = o, ln
    return recs


@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    """The rows made by hand through HitPrinter::print, for a score column of 8 and of 40 bytes."""
    import rnamotif_amd as R
    tmp = tmp_path_factory.mktemp("print_hand")
    # (letters as the readers deliver them: Replay.batch prints the bytes it is given)
    big = b"acgt" * 2_600_000                     # more than 10^7 bases
    entries = [b"acgtnacgtryk" * 4, b"ggggaaaacccc" * 3, b"tttt" * 10, b"acgt" * 11, b"cagt" * 9, big]
    sids = [b"a", b"twelve_bytes", b"thirteen_byte", b"n" * 99, b"4", b"big"]
    sdefs = [b"", b"a definition, with blanks", b"", b"x", b"", b"ten million bases and more"]
    assert [len(s) for s in sids[:4]] == [1, 12, 13, 99] and sids[4] == b"%d" % 4
    m = len(big)
    rows = [(0, 0, 0, 2), (0, 0, len(entries[0]) - 8, 2),           # strand 0 at the first and at the last base
            (0, 1, 0, 4), (0, 1, len(entries[0]) - 6, 0),           # strand 1 at the first and at the last base; an empty ss
            (1, 0, 5, 1), (1, 1, 7, 3), (2, 0, 1, 0), (3, 1, 2, 4), (4, 0, 0, 4), (4, 1, 3, 2),
            (5, 0, m - 10_500, 10_001), (5, 0, 0, 1), (5, 1, 17, 12_345), (5, 1, m - 6, 0)]
    out = {}
    for key, text in (("8", HAND), ("40", HAND40)):
        path = os.path.join(str(tmp), "hand%s.descr" % key)
        with open(path, "w") as f:
            f.write(text)
        d = R.Descriptor(["-descr", path])
        recs = _hand(d, rows)
        file = os.path.join(str(tmp), "hand%s.out" % key)
        rp = R.Replay(d, file)
        assert rp.batch(sids, sdefs, entries, recs) == len(rows)
        rp.close()
        out[key] = (d, recs, open(file, "rb").read())
    return {"tmp": tmp, "entries": entries, "sids": sids, "sdefs": sdefs, "rows": rows, "cases": out}


@pytest.mark.parametrize("key", ["8", "40"])
def test_rows_made_by_hand(built, print_checker, hand, key):
    d, recs, text = hand["cases"][key]
    p = program_of(d)
    lines = hit_lines(text)
    assert len(lines) == len(recs)
    slens = [len(e) for e in hand["entries"]]
    text_len, text_bytes = score_columns(lines, recs, hand["sids"], slens, d, p)
    assert (text_len == int(key)).all()
    assert text_bytes[0].tobytes() == (b"   0.000" if key == "8" else b"0123456789abcdefghijABCDEFGHIJ9876543210")
    off, data = host_print(print_checker, hand["tmp"], d, hand["entries"], recs, hand["sids"], hand["sdefs"], text_len, text_bytes)
    assert header_of(d) + data == text
    # what the rows are there for
    two = [data[off[h]:off[h + 1]].split(b"\n") for h in range(len(recs))]
    assert two[0][0] == b">a " and two[0][1].startswith(b"a" + b" " * 12)
    assert two[4][0] == b">twelve_bytes a definition, with blanks" and two[4][1].startswith(b"twelve_bytes ")
    assert two[6][1].startswith(b"thirteen_byte ") and two[7][1].startswith(b"n" * 99 + b" ")
    nums = [ln[1].split()[-6:] for ln in two]
    assert nums[10][:3] == [b"0", b"%d" % (slens[5] - 10_500 + 1), b"10007"] and len(nums[10][1]) == 8
    assert nums[12][:3] == [b"1", b"%d" % (slens[5] - 17), b"12351"]
    assert nums[2][:2] == [b"1", b"%d" % slens[0]] and nums[3][:3] == [b"1", b"6", b"6"] and nums[3][4] == b"."
    assert nums[1][1] == b"%d" % (slens[0] - 8 + 1) and two[1][1].endswith(b" " + hand["entries"][0][-3:])


def test_record_check(built, print_checker, workdir, tmp_path):
    d = _descr(pins.STRICT_ARGS + ["-descr", "trna.strict.descr"], cwd=workdir)
    p = program_of(d)
    rng = np.random.default_rng(29)
    slen = [0, 1, 33, 2 ** 31 - 1, 500, 90]
    m, width = 4000, 24
    recs = np.zeros((m, d.hit_stride), dtype=np.int32)
    recs[:, 0] = rng.choice([-1, 0, 1, 2, 3, 4, 5, 6, 2 ** 31 - 1], size=m, p=[.01, .02, .02, .05, .4, .3, .18, .01, .01])
    recs[:, 1] = rng.choice([0, 1, 2, -1], size=m, p=[.49, .49, .01, .01])
    big = np.array([0, 1, 2, 5, 40, 2 ** 30, 2 ** 31 - 2, 2 ** 31 - 1, -1, -2 ** 31], dtype=np.int64)
    pw = np.array([.3, .3, .2, .1, .04, .01, .01, .02, .01, .01])
    for k in range(HDR, d.hit_stride):
        recs[:, k] = big[rng.choice(big.size, size=m, p=pw / pw.sum())].astype(np.int32)
    text_len = rng.choice([0, 8, width, width + 1, -1, 2 ** 31 - 1], size=m, p=[.2, .4, .3, .04, .03, .03]).astype(np.int32)
    got = host_check(print_checker, tmp_path, d, slen, recs, text_len, width)
    want = []
    for w, tl in zip(recs, text_len):
        code, _, _, which = _span_py(w, d.n_elems, d.ctx_off, p.has_lctx, p.has_rctx, slen)
        want.append((code, which) if code else (0 if 0 <= tl <= width else HP_TEXT, -1))
    assert got == want
    assert {g[0] for g in got} == {0, 1, 2, 3, HP_TEXT}
    # a bad entry, a bad strand and an element outside its entry, one at a time, and what the print mode says of one
    d2 = _descr(["-descr", "qu+tr.descr"], cwd=workdir)
    base = np.zeros((4, d2.hit_stride), dtype=np.int32)
    base[1, 0], base[2, 1], base[3, HDR + 4 * 2:HDR + 4 * 2 + 2] = 7, 2, (28, 3)
    assert host_check(print_checker, tmp_path, d2, [30] * 7, base, np.full(4, 8, dtype=np.int32), 8) == [(0, -1), (1, -1), (2, -1), (3, 2)]
    words = host_print(print_checker, tmp_path, d2, [b"a" * 30] * 7, base[[0, 3]], [b"s"] * 7, [b""] * 7, np.full(2, 8, dtype=np.int32),
                       np.full((2, 8), ord("0"), dtype=np.uint8), expect=1)
    assert "record 1 is bad: 3 2" in words


def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "rnamotif_amd.h")).read()
    for name in ("rma_names_create", "rma_names_destroy", "rma_hit_print_size", "rma_hit_print", "rma_print_header"):
        assert "\t%s( " % name in text
    rule = open(os.path.join(H, "rm_hitprint.h")).read()
    for words in ("rm_score.cpp:1909", "find_motif.c:1869-1896", "hitwin_span", "%-12s", " %d %7d %4d", "buf[ 2048 ]"):
        assert words in rule
