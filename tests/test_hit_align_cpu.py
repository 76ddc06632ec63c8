"""CPU: hit records as an alignment -- the byte matrix whose rows are the sequence lines of `rmfmt -a` -- as
rnamotif_amd/csrc/rm_hitalign.h states it for the host and for the kernels of rm_hitalign_dev.hip, run on the host
through tests/hostsim/hit_align_check.cpp over the oracle's records of the reference's test database.  The test
holds the rule to the tool and the tool to the reference's:

  * per case: the oracle's records through the host replay (which prints the accepted ones), the text through
    rnamotif_amd/bin/rmfmt -a and, where it has been built, oracle/_ref/rmfmt -a: byte-identical; the sequence lines
    of hit h are lines(h) of the checker's row h over the records of the printed hits; the hit counts are pins.py's;
  * tests/golden/tools/*.rmfmt.a.ref, the reference tool's own output, reproduced from the hits of *.rm.out;
  * over the table: a right-aligned column with a gap, a left-aligned one with a gap, a '.';
  * pos: every letter is its strand's letter at pos, a column's letters are one run on the side its direction says,
    and a row's letters in column order are the hit's printed fields;
  * given widths larger than needed shift nothing but gaps, widths one too small are refused, naming the column;
  * the record check against _span_py of test_hit_windows_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pins
from test_hit_structures_cpu import TYPES, Program, program_of
from test_hit_windows_cpu import _span_py, _write_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "tests", "_build", "hit_align_check")
TOOL = os.path.join(ROOT, "rnamotif_amd", "bin", "rmfmt")
REF_TOOL = os.path.join(ROOT, "oracle", "_ref", "rmfmt")
HDR = 5
LINE = 70
RIGHT = ("h3", "t2", "q2", "q4")

# an ss( minlen=0 ) that is empty in some hits: printed as '.'
DOT = ("descr\n\th5( minlen=3, maxlen=5 )\n\t\tss( minlen=0, maxlen=1 )\n\t\th5( minlen=3, maxlen=4 )\n"
       "\t\t\tss( minlen=4, maxlen=6 )\n\t\th3\n\t\tss( minlen=0, maxlen=1 )\n\th3\n")
# name -> (rnamotif arguments, entries of the database taken, the number of hits pinned in pins.py or None)
CASES = {
    "trna": (["-descr", "trna.descr"], None, pins.SLACK["trna.descr"][0]),
    "pk1": (["-descr", "pk1.descr"], None, pins.SLACK["pk1.descr"][0]),
    "qu+tr": (["-descr", "qu+tr.descr"], None, pins.SLACK["qu+tr.descr"][0]),
    "score.2": (["-descr", "score.2.descr"], None, pins.SLACK["score.2.descr"][0]),
    "trna.context": (pins.STRICT_ARGS + ["-descr", "trna.strict.descr"], None, pins.STRICT["trna"][0]),
    "dot": (["-descr", "dot.descr"], 60, None),
}
assert (pins.SLACK["trna.descr"][0], pins.SLACK["pk1.descr"][0], pins.SLACK["qu+tr.descr"][0]) == (1351, 193, 9)


@pytest.fixture(scope="module")
def align_checker():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "hostsim", "hit_align_check.cpp")
    deps = [src, os.path.join(H, "rm_hitalign.h"), os.path.join(H, "rm_hitstruct.h"), os.path.join(H, "rm_hitwin.h"),
            os.path.join(ROOT, "include", "rnamotif_amd_program.h")]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(f) for f in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + H, "-o", BIN, src], check=True)
    return BIN


def _descr(argv, cwd=None):
    import rnamotif_amd as R
    old = os.getcwd()
    os.chdir(cwd or old)
    try:
        return R.Descriptor(argv)
    finally:
        os.chdir(old)


def host_alignment(checker, tmp, d, entries, records, widths=None, fill=None, expect=0):
    """The rule on the host: dict of widths int32 [n_cols], right bool [n_cols], rows uint8 [n, W], pos int32 [n, W];
    with expect=1 the words of the refusal."""
    tmp = str(tmp)
    prog, ent, rec, out = (os.path.join(tmp, f) for f in ("program.bin", "entries.bin", "records.bin", "alignment.bin"))
    with open(prog, "wb") as f:
        f.write(C.string_at(d.program, C.sizeof(Program)))
    _write_entries(ent, entries)
    np.ascontiguousarray(records, dtype=np.int32).tofile(rec)
    argv = [checker, "fill", prog, ent, rec, out, "-" if widths is None else ",".join(str(int(w)) for w in widths)]
    if fill is not None:
        argv.append(bytes(fill).decode("latin-1"))
    p = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == expect, p.stderr.decode()
    if expect:
        return p.stderr.decode()
    raw = open(out, "rb").read()
    n, w = (int(x) for x in np.frombuffer(raw, dtype=np.int64, count=2))
    nc = int(np.frombuffer(raw, dtype=np.int32, count=1, offset=16)[0])
    assert n == len(records)
    at = 20
    wid = np.frombuffer(raw, dtype=np.int32, count=nc, offset=at)
    at += 4 * nc
    right = np.frombuffer(raw, dtype=np.uint8, count=nc, offset=at).astype(np.bool_)
    at += nc
    rows = np.frombuffer(raw, dtype=np.uint8, count=n * w, offset=at).reshape(n, w)
    at += n * w
    pos = np.frombuffer(raw[at:], dtype=np.int32, count=n * w).reshape(n, w)
    assert at + 4 * n * w == len(raw) and w == int(wid.sum()) + nc - 1
    return {"widths": wid, "right": right, "rows": rows, "pos": pos}


def lines_of(row):
    b = row.tobytes()
    return [b[i:i + LINE] for i in range(0, len(b), LINE)]


def run_tool(exe, text):
    p = subprocess.run([exe, "-a"], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, LC_ALL="C"))
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout


def alignment_hits(out):
    """the hits of `rmfmt -a`'s output: per hit its sequence lines"""
    hits = []
    for ln in out.split(b"\n"):
        if ln.startswith(b">"):
            hits.append([])
        elif ln:
            hits[-1].append(ln)
    return hits


def hit_lines(text):
    return [ln for ln in text.split(b"\n") if ln and ln[:1] not in (b"#", b">")]


def records_of(lines, recs, sids, slens, d, p):
    """The records the printed hits came from, in order: a hit line names its entry, strand, where its first element
    starts and how long every field is, and the elements of a record lie end to end; the replay prints in the order
    of the records, so each hit's record is the next one that has these values."""
    ne, ctx = d.n_elems, d.ctx_off
    n_cols = ne + int(p.has_lctx) + int(p.has_rctx)
    rows, at = [], 0
    for ln in lines:
        f = ln.split()
        fields = f[-n_cols:]
        comp, offset = int(f[-n_cols - 3]), int(f[-n_cols - 2])
        lens = [0 if x == b"." else len(x) for x in fields]
        while True:
            w = recs[at]        # (an IndexError here: a printed hit without a record)
            e = int(w[0])
            off0 = int(slens[e]) - offset if comp else offset - 1
            got = [int(x) for x in w[HDR + 1:HDR + 4 * ne:4]]
            if p.has_lctx:
                got = [int(w[ctx + 1])] + got
            if p.has_rctx:
                got = got + [int(w[ctx + 3])]
            if sids[e] == f[0] and int(w[1]) == comp and int(w[HDR]) == off0 and got == lens:
                break
            at += 1
        rows.append(at)
        at += 1
    return np.asarray(rows, dtype=np.int64)


_results = {}


def case_result(name, checker, gbrna, workdir, tmp_factory):
    if name in _results:
        return _results[name]
    import rnamotif_amd as R
    from oracle_binding import oracle_scan
    argv, limit, _ = CASES[name]
    tmp = tmp_factory.mktemp("align_" + name.replace("+", "_"))
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
    n_cols = d.n_elems + int(p.has_lctx) + int(p.has_rctx)
    lines = hit_lines(text)
    assert len(lines) == n_printed
    rows = records_of(lines, recs, sids, [len(e) for e in entries], d, p)
    accepted = recs[rows]
    r = {"d": d, "p": p, "entries": entries, "sids": sids, "recs": accepted, "text": text, "lines": lines, "n_cols": n_cols,
         "tool": run_tool(TOOL, text), "al": host_alignment(checker, tmp, d, entries, accepted), "tmp": tmp}
    _results[name] = r
    return r


def _strand(seq, comp):
    if not comp:
        return seq
    return bytes({ord("a"): ord("t"), ord("c"): ord("g"), ord("g"): ord("c"), ord("t"): ord("a")}.get(b, ord("n")) for b in seq[::-1])


@pytest.mark.parametrize("name", sorted(CASES))
def test_rows_are_rmfmt_a(built, align_checker, gbrna, workdir, tmp_path_factory, name):
    r = case_result(name, align_checker, gbrna, workdir, tmp_path_factory)
    n = len(r["recs"])
    assert n >= 1
    if CASES[name][2] is not None:
        assert n == CASES[name][2]
    if os.path.exists(REF_TOOL):
        assert run_tool(REF_TOOL, r["text"]) == r["tool"]
    hits = alignment_hits(r["tool"])
    assert len(hits) == n
    al = r["al"]
    for h in range(n):
        assert hits[h] == lines_of(al["rows"][h]), (name, h)
    # the directions are getfmt()'s, read off the '#RM descr' line
    names = [ln for ln in r["text"].split(b"\n") if ln.startswith(b"#RM descr")][0].split()[2:]
    assert len(names) == r["n_cols"] == len(al["widths"]) == len(r["d"].names())
    assert [x.decode() for x in names] == r["d"].names()
    assert list(al["right"]) == [x[:2].decode() in RIGHT for x in names]
    if name == "trna.context":
        assert names[0] == b"ctx" and names[-1] == b"ctx" and al["widths"][0] >= 1 and al["widths"][-1] >= 1
    if name == "qu+tr":
        assert {x[:2] for x in names} >= {b"t2", b"q2", b"q4"}
    if name == "dot":
        lens = r["recs"][:, HDR + 1:HDR + 4 * r["d"].n_elems:4]
        assert (lens == 0).any(axis=1).any() and (lens[:, 1] == 1).any()


def _columns(al):
    off = np.concatenate([[0], np.cumsum(al["widths"].astype(np.int64) + 1)])[:-1]
    return [(int(off[c]), int(off[c] + al["widths"][c])) for c in range(len(al["widths"]))]


def test_the_table_covers_gaps_on_both_sides_and_a_dot(built, align_checker, gbrna, workdir, tmp_path_factory):
    right_gap = left_gap = dot = 0
    for name in sorted(CASES):
        r = case_result(name, align_checker, gbrna, workdir, tmp_path_factory)
        al = r["al"]
        for c, (a, b) in enumerate(_columns(al)):
            gaps = int((al["rows"][:, a:b] == ord("-")).sum())
            if al["right"][c]:
                right_gap += gaps
            else:
                left_gap += gaps
        dot += int((al["rows"] == ord(".")).sum())
    assert right_gap >= 1 and left_gap >= 1 and dot >= 1, (right_gap, left_gap, dot)


@pytest.mark.parametrize("name", sorted(CASES))
def test_pos(built, align_checker, gbrna, workdir, tmp_path_factory, name):
    r = case_result(name, align_checker, gbrna, workdir, tmp_path_factory)
    al, cols = r["al"], _columns(r["al"])
    seps = [b for _, b in cols[:-1]]
    strands = {}
    for h, w in enumerate(r["recs"]):
        row, pos = al["rows"][h], al["pos"][h]
        key = (int(w[0]), int(w[1]))
        if key not in strands:
            strands[key] = np.frombuffer(_strand(r["entries"][key[0]], key[1]), dtype=np.uint8)
        letter = pos >= 0
        # every letter byte is its strand's letter at pos (the window letter at pos - lo)
        assert np.array_equal(row[letter], strands[key][pos[letter]]), h
        assert (row[seps] == ord("|")).all() and (pos[seps] == -1).all()
        assert np.isin(row[~letter], np.frombuffer(b"-|.", dtype=np.uint8)).all()
        fields = r["lines"][h].split()[-r["n_cols"]:]
        for c, (a, b) in enumerate(cols):
            at = np.flatnonzero(letter[a:b])
            f = fields[c]
            if f == b".":
                assert at.size == 0 and (row[a:b] == ord(".")).sum() == 1
                assert row[b - 1 if al["right"][c] else a] == ord(".")
                continue
            # one run, on the side the direction says, of consecutive positions, spelling the printed field
            assert at.size == len(f) and at[-1] - at[0] + 1 == at.size, (h, c)
            assert (at[-1] == b - a - 1) if al["right"][c] else (at[0] == 0), (h, c)
            assert (np.diff(pos[a:b][at]) == 1).all()
            assert row[a:b][at].tobytes() == f, (h, c)
        assert b" ".join(fields).replace(b" ", b"").replace(b".", b"") == row[letter].tobytes()


def test_given_widths(built, align_checker, gbrna, workdir, tmp_path_factory):
    for name in ("qu+tr", "dot"):
        r = case_result(name, align_checker, gbrna, workdir, tmp_path_factory)
        al, d = r["al"], r["d"]
        extra = np.arange(len(al["widths"]), dtype=np.int32) % 3
        assert (extra > 0).any() and (extra == 0).any()
        wide = host_alignment(align_checker, r["tmp"], d, r["entries"], r["recs"], widths=al["widths"] + extra)
        assert np.array_equal(wide["widths"], al["widths"] + extra)
        for c, ((a, b), (a2, b2)) in enumerate(zip(_columns(al), _columns(wide))):
            k = int(extra[c])
            inner = slice(a2 + k, b2) if al["right"][c] else slice(a2, b2 - k)
            outer = slice(a2, a2 + k) if al["right"][c] else slice(b2 - k, b2)
            assert np.array_equal(wide["rows"][:, inner], al["rows"][:, a:b]) and np.array_equal(wide["pos"][:, inner], al["pos"][:, a:b])
            assert (wide["rows"][:, outer] == ord("-")).all() and (wide["pos"][:, outer] == -1).all()
        # the widths of a subset hold for the subset, and the whole set's widths hold for it too
        some = r["recs"][::2]
        sub = host_alignment(align_checker, r["tmp"], d, r["entries"], some)
        assert (sub["widths"] <= al["widths"]).all()
        shared = host_alignment(align_checker, r["tmp"], d, r["entries"], some, widths=al["widths"])
        assert np.array_equal(shared["rows"], al["rows"][::2]) and np.array_equal(shared["pos"], al["pos"][::2])
        # one too small, column by column
        for c in (0, len(al["widths"]) // 2, len(al["widths"]) - 1):
            small = al["widths"].copy()
            small[c] -= 1
            words = host_alignment(align_checker, r["tmp"], d, r["entries"], r["recs"], widths=small, expect=1)
            assert "column %d: width %d given, the records need %d" % (c, small[c], al["widths"][c]) in words
        # other fill bytes change those bytes alone
        other = host_alignment(align_checker, r["tmp"], d, r["entries"], r["recs"], fill=b"~/o")
        assert np.array_equal(other["pos"], al["pos"])
        table = np.arange(256, dtype=np.uint8)
        table[[ord("-"), ord("|"), ord(".")]] = [ord("~"), ord("/"), ord("o")]
        assert np.array_equal(other["rows"], table[al["rows"]])


@pytest.mark.parametrize("name", ["trna", "pk1", "score.2"])
def test_golden_files(built, align_checker, gbrna, workdir, tmp_path_factory, name):
    """tests/golden/tools/NAME.rmfmt.a.ref is the reference's rmfmt -a on NAME.rm.out, the hits of a dozen entries"""
    r = case_result(name, align_checker, gbrna, workdir, tmp_path_factory)
    text = open(os.path.join(GOLDEN, "tools", name + ".rm.out"), "rb").read()
    want = open(os.path.join(GOLDEN, "tools", name + ".rmfmt.a.ref"), "rb").read()
    assert run_tool(TOOL, text) == want
    lines = hit_lines(text)
    assert lines and lines == r["lines"][:len(lines)]
    recs = r["recs"][:len(lines)]
    al = host_alignment(align_checker, r["tmp"], r["d"], r["entries"], recs)
    hits = alignment_hits(want)
    assert len(hits) == len(recs)
    for h in range(len(recs)):
        assert hits[h] == lines_of(al["rows"][h]), (name, h)


@pytest.mark.parametrize("name", ["trna.descr", "qu+tr.descr", "trna.strict.descr"])
def test_record_check(built, align_checker, workdir, tmp_path, name):
    strict = "strict" in name
    d = _descr((pins.STRICT_ARGS if strict else []) + ["-descr", name], cwd=workdir)
    p = program_of(d)
    rng = np.random.default_rng(13)
    slen = [0, 1, 33, 2 ** 31 - 1, 500, 90]
    m = 6000
    recs = np.zeros((m, d.hit_stride), dtype=np.int32)
    recs[:, 0] = rng.choice([-1, 0, 1, 2, 3, 4, 5, 6, 2 ** 31 - 1], size=m, p=[.01, .02, .02, .05, .4, .3, .18, .01, .01])
    recs[:, 1] = rng.choice([0, 1, 2, -1], size=m, p=[.49, .49, .01, .01])
    big = np.array([0, 1, 2, 5, 40, 2 ** 30, 2 ** 31 - 2, 2 ** 31 - 1, -1, -2 ** 31], dtype=np.int64)
    pw = np.array([.3, .3, .2, .1, .04, .01, .01, .02, .01, .01])
    for k in range(HDR, d.hit_stride):
        recs[:, k] = big[rng.choice(big.size, size=m, p=pw / pw.sum())].astype(np.int32)
    # (strands of one helix with unequal lengths everywhere: not refused, as rmfmt does not refuse them)
    tmp = str(tmp_path)
    prog, ent, rec = (os.path.join(tmp, f) for f in ("program.bin", "entries.bin", "records.bin"))
    with open(prog, "wb") as f:
        f.write(C.string_at(d.program, C.sizeof(Program)))
    with open(ent, "wb") as f:
        f.write(np.asarray([len(slen)] + slen, dtype=np.int32).tobytes())
    recs.tofile(rec)
    q = subprocess.run([align_checker, "check", prog, ent, rec, "-"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert q.returncode == 0, q.stderr.decode()
    got = [tuple(map(int, line.split())) for line in q.stdout.decode().splitlines()]
    want = [(c, which) for c, _, _, which in (_span_py(w, d.n_elems, d.ctx_off, p.has_lctx, p.has_rctx, slen) for w in recs)]
    assert got == want
    assert {g[0] for g in got} == {0, 1, 2, 3}


def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "rnamotif_amd.h")).read()
    assert "int\trma_hit_alignment_shape( rma_scanner_t *sc, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits," in text
    assert "int\trma_hit_alignment( rma_scanner_t *sc, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits," in text
    rule = open(os.path.join(H, "rm_hitalign.h")).read()
    for words in ("find_motif.c:1869-1896", "rmfmt.c:418-425", "rmfmt.c:531-554", "hitwin_span", "NOT required"):
        assert words in rule
    assert [TYPES[t] for t in (3, 7, 10, 12)] == list(RIGHT)
