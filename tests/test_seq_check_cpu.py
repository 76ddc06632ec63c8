"""CPU: the loose seq= expressions on one record as rnamotif_amd/csrc/rm_seqcheck.h states them for the host and for
rma_seqcheck_kernel -- advance() without its recursion, on an explicit stack of frames -- run on the host through
tests/hostsim/seq_check.cpp against re_step() / re_mm_step() of rm_regex.cpp (the checker compares, record by record) and
against Python's `re` (this file compares):

  * every string of length 0 to 7 over acgn (21 845) under each expression of TABLE, every string of length 0 to 5 over
    acgnry under the three iupac = 0 cases of tests/test_loose_seq.py; the strings lie end to end in one entry, so the
    byte behind an element is the next string's first: the rule must take the element's end for the end of the string;
  * hand-made records of a lone ss over six entries of 40 to 90 bases: one for every entry, strand, start and length in
    [minlen, maxlen] (window_records), with the plants the elements' ends need;
  * refusals, the budget, the header.

tests/test_seq_check.py runs the same window records through the kernel."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "tests", "_build", "seq_check")
FRONT_END = ["rm_regex", "rm_compile", "rm_parse", "rm_score", "rm_seqcheck", "rm_efndata", "rm_efn2data", "rm_fasta", "rm_driver",
             "rm_cli", "rm_dump", "rm_pack", "rm_stream"]
HDR = 5         # RMA_HIT_HDR

# ed form (seq=), Python's form, anchored (re.match) or floating (re.search)
TABLE = [
    (r"^\(a[cg]\)g\1", r"(a[cg])g\1", True),
    (r"\(ac\)g\1", r"(ac)g\1", False),
    (r"^\(ac\)\1*g", r"(ac)(?:\1)*g", True),
    (r"^\(a\)\(c\)..\2\1", r"(a)(c)..\2\1", True),
    (r"^\(a*\)c\1$", r"(a*)c\1$", True),
    (r"^\(.*\)\1$", r"(.*)\1$", True),
    (r"\(.\)\1\1", r"(.)\1\1", False),
    (r"^a*\(c*\)g*\1a*$", r"a*(c*)g*\1a*$", True),
    (r"^\(a\{1,2\}\)c\{0,1\}\1", r"(a{1,2})c{0,1}\1", True),
    (r"\([ac]g\).*\1$", r"([ac]g).*\1$", False),
    (r"^.*\(g.\).*\1.*$", r".*(g.).*\1.*$", True),
    (r"^\(\(a\)c\)\2\1", r"((a)c)\2\1", True),
    (r"^[^a]*\(a.\)\1*$", r"[^a]*(a.)(?:\1)*$", True),
    # two more, for \{lo,hi\} and \{lo,\}, which the compiler takes on a class and on a dot: the ninth expression in classes
    # (the same strings match), and a square of at least two letters
    (r"^\([a]\{1,2\}\)[c]\{0,1\}\1", r"(a{1,2})c{0,1}\1", True),
    (r"^\(.\{2,\}\)\1$", r"(.{2,})\1$", True),
]
# how many of the 21 845 strings each matches
MATCHES = [42, 57, 363, 80, 4, 85, 4976, 172, 1706, 600, 2632, 21, 1632, 1706, 4 ** 2 + 4 ** 3]
# The descriptor compiler refuses this one as an element's seq=, whatever minlen / maxlen of at most 12 go with it:
# mm_seqlen() of the reference reads the literal where the low count of a CCHR | RNGE is (mm_regexp.c:111-117; rm_regex.cpp
# walks the same bytes), so a\{1,2\} implies a minimal length of 'a' = 97 bases and the element fails with
# "minlen > maxlen".  Twelve of the thirteen remain.
REFUSED_BY_COMPILER = {r"^\(a\{1,2\}\)c\{0,1\}\1": "minlen > maxlen"}
# name -> (parms, minlen, maxlen, seq=, mismatch): the cases of tests/test_loose_seq.py with iupac = 0
IUPAC0 = {
    "literal_n": ("iupac = 0;", 4, 5, "^nnac", 0),
    "literal_r_class": ("iupac = 0;", 3, 4, "^[ar]n[^y]", 0),
    "literal_mismatch": ("iupac = 0;", 4, 4, "^nrac$", 1),
}
CASES = ["table%02d" % k for k in range(len(TABLE)) if TABLE[k][0] not in REFUSED_BY_COMPILER] + sorted(IUPAC0)
BACKREF_CASES = [c for c in CASES if c.startswith("table")]


def case_of(name):
    """(parms, minlen, maxlen, seq=, mismatch, python expression or None, anchored)"""
    if name in IUPAC0:
        parms, lo, hi, seq, mm = IUPAC0[name]
        return parms, lo, hi, seq, mm, (None if mm else seq.lstrip("^")), True
    ed, py, anchored = TABLE[int(name[5:])]
    return "", 2, 7, ed, 0, py, anchored


def descr_text(name, hairpin=False, score=""):
    parms, lo, hi, seq, mm, _, _ = case_of(name)
    elem = 'ss(minlen=%d,maxlen=%d,seq="%s"%s)' % (lo, hi, seq, ",mismatch=%d" % mm if mm else "")
    body = "\th5(minlen=2,maxlen=3)\n\t\t" + elem + "\n\th3\n" if hairpin else "\t" + elem + "\n"
    return ("parms\n\t" + parms + "\n" if parms else "") + "descr\n" + body + score


def descr_args(name, tmp, hairpin=False, score=""):
    path = os.path.join(str(tmp), name + (".hp" if hairpin else "") + ".descr")
    with open(path, "w") as f:
        f.write(descr_text(name, hairpin, score))
    return ["-descr", path]


def expected(name, sub):
    """(keep, the mismatch word or None) of Python's statement of the case on an element's text"""
    _, _, _, seq, mm, py, anchored = case_of(name)
    if py is None:
        # "^nrac$" with one mismatch: the letters compared one by one (mm_advance, mm_regexp.c:369)
        n = sum(a != b for a, b in zip(sub, "nrac"))
        return len(sub) == 4 and n <= 1, n
    return (re.match(py, sub) if anchored else re.search(py, sub)) is not None, None


def build_checker(sanitize=False):
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    out = BIN + ("_san" if sanitize else "")
    src = os.path.join(ROOT, "tests", "hostsim", "seq_check.cpp")
    units = [os.path.join(H, u + ".cpp") for u in FRONT_END]
    deps = [src] + units + [os.path.join(H, f) for f in os.listdir(H) if f.endswith(".h")] + [os.path.join(ROOT, "include", "rnamotif_amd_program.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(f) for f in deps):
        flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread"] + flags + ["-I" + os.path.join(ROOT, "include"), "-I" + H, "-o", out, src] + units,
                       check=True)
    return out


@pytest.fixture(scope="module")
def seq_checker():
    return build_checker()


def run_checker(checker, tmp, argv, entries, recs, budget=0):
    """seq_check over these entries and records: (refusal or None, the image's sizes, [(outcome, element, steps)], the fixed
    rows, status, stdout)."""
    import rnamotif_amd as R
    tmp = str(tmp)
    ent, rec = os.path.join(tmp, "entries.bin"), os.path.join(tmp, "records.bin")
    with open(ent, "wb") as f:
        f.write(np.asarray([len(entries)] + [len(e) for e in entries], dtype=np.int32).tobytes())
        f.write(b"".join(entries))
    recs = np.ascontiguousarray(recs, dtype=np.int32)
    recs.tofile(rec)
    p = subprocess.run([checker, ent, rec, str(budget)] + list(argv), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600,
                       env=dict(os.environ, EFNDATA=os.environ.get("EFNDATA", R.EFNDATA_DIR), ASAN_OPTIONS="detect_leaks=0"))
    out = p.stdout.decode()
    assert p.returncode in (0, 1), p.stderr.decode()[-2000:]
    lines = out.split("\n")
    if lines[0].startswith("REFUSED "):
        return lines[0][8:], None, [], None, p.returncode, out
    assert lines[0].startswith("IMAGE "), out[:200]
    image = {k: int(v) for k, v in (w.split("=") for w in lines[0].split()[1:])}
    rows, fixed = [], []
    for ln in lines[1:]:
        if ln[:2] in ("K ", "D ", "S "):
            w = ln.split(" ")
            rows.append((w[0], int(w[1]), int(w[2])))
            fixed.append([int(x) for x in w[3:]])
    fixed = np.asarray(fixed, dtype=np.int32).reshape(len(rows), recs.shape[1] if recs.ndim == 2 else -1)
    return None, image, rows, fixed, p.returncode, out


def revcomp(s):
    """mk_rcmp (rnamot.c:193-216) of the readers' letters"""
    tr = bytes((ord("n") if chr(c) not in "acgt" else c) for c in range(256)).translate(bytes.maketrans(b"acgt", b"tgca"))
    return s.translate(tr)[::-1]


def reader_letters(raw):
    """what the readers make of an entry's bytes: a letter in lower case, u as t, anything else n"""
    import rnamotif_amd as R
    return bytes(R.reader_letter(b) for b in raw)


def raw_entries():
    """Six entries of 40 to 90 bases as a database's text holds them: acgt, a few n, r and y, entries 1 and 4 in upper case;
    planted: acgac at base 0 of entry 0 and at the end of entry 1 (on strand 1: gtcgt at the end and at base 0), and again
    inside entry 2 -- the record acga of it must be dropped under \\(ac\\)g\\1 though a c follows -- and the material of the
    iupac = 0 cases."""
    rng = np.random.default_rng(4177)
    lens = [40, 57, 64, 71, 83, 90]
    plants = [b"aggag", b"acacacg", b"accgca", b"nnac", b"rnac", b"rna", b"anc", b"ynac", b"nracc", b"arac", b"gaga", b"gtcgt", b"acgtacgt", b"cccc"]
    out = []
    for k, n in enumerate(lens):
        s = bytearray(np.frombuffer(b"acgt", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes())
        for i in rng.integers(0, n, size=3):
            s[i] = ord("nry"[int(rng.integers(0, 3))])
        for _ in range(5):
            p = plants[int(rng.integers(0, len(plants)))]
            at = int(rng.integers(0, n - len(p)))
            s[at:at + len(p)] = p
        if k == 0:
            s[:5] = b"acgac"
        if k == 1:
            s[-5:] = b"acgac"
        if k == 2:
            s[20:27] = b"tacgact"
        if k == 3:
            s[:5] = b"gtcgt"
        if k == 4:
            s[-5:] = b"gtcgt"
        out.append(bytes(s).upper() if k in (1, 4) else bytes(s))
    return out


def window_records(entries, lo, hi, stride):
    """A record of a lone ss for every entry, strand, start and length in [lo, hi]: a header, then off, len, 0, 0."""
    rows = []
    for k, e in enumerate(entries):
        for comp in (0, 1):
            for off in range(len(e) + 1):
                for rank, n in enumerate(range(hi, lo - 1, -1)):
                    if off + n <= len(e):
                        r = [0] * stride
                        r[:HDR + 2] = [k, comp, off, rank, 0, off, n]
                        rows.append(r)
    return np.asarray(rows, dtype=np.int32)


def window_expectation(name, entries, recs):
    """keep and the fixed rows by Python's statement of the case"""
    strands = [(e, revcomp(e)) for e in entries]
    keep = np.zeros(len(recs), dtype=bool)
    fixed = recs.copy()
    for h, r in enumerate(recs):
        sub = strands[r[0]][r[1]][r[HDR]:r[HDR] + r[HDR + 1]].decode()
        keep[h], n_mm = expected(name, sub)
        if keep[h] and n_mm is not None:
            fixed[h, HDR + 3] = n_mm
    return keep, fixed


_windows = {}


def window_case(name, checker, tmp_factory):
    """A case's window records through the checker, once for the session (and for tests/test_seq_check.py)."""
    import rnamotif_amd as R
    if name not in _windows:
        tmp = tmp_factory.mktemp("seq_" + name)
        argv = descr_args(name, tmp)
        d = R.Descriptor(argv)
        _, lo, hi = case_of(name)[:3]
        raw = raw_entries()
        entries = [reader_letters(e) for e in raw]
        recs = window_records(entries, lo, hi, d.hit_stride)
        refused, image, rows, fixed, status, out = run_checker(checker, tmp, argv, entries, recs)
        _windows[name] = {"argv": argv, "d": d, "raw": raw, "entries": entries, "recs": recs, "refused": refused, "image": image, "rows": rows,
                          "fixed": fixed, "status": status, "out": out}
    return _windows[name]


def strings_over(alphabet, most):
    return [b""] + [bytes(t) for n in range(1, most + 1) for t in itertools.product(alphabet, repeat=n)]


def string_records(strings, stride):
    """the strings end to end in one entry, and a record for each: its element is the string"""
    recs = np.zeros((len(strings), stride), dtype=np.int32)
    lens = np.asarray([len(s) for s in strings], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    recs[:, 2] = off
    recs[:, HDR] = off
    recs[:, HDR + 1] = lens
    return [b"".join(strings)], recs


def test_the_compiler_refuses_what_the_list_says(built, tmp_path):
    import rnamotif_amd as R
    for k, (ed, _, _) in enumerate(TABLE):
        argv = descr_args("table%02d" % k, tmp_path)
        if ed in REFUSED_BY_COMPILER:
            for lo, hi in ((0, 7), (1, 12), (2, 7), (3, 3)):
                (tmp_path / "r.descr").write_text('descr\n\tss(minlen=%d,maxlen=%d,seq="%s")\n' % (lo, hi, ed))
                with pytest.raises(R.RnamotifError, match=REFUSED_BY_COMPILER[ed]):
                    R.Descriptor(["-descr", str(tmp_path / "r.descr")])
        else:
            assert R.Descriptor(argv).loose == 1
    assert len(BACKREF_CASES) >= 10


@pytest.mark.parametrize("name", BACKREF_CASES)
def test_every_short_string(built, seq_checker, tmp_path, name):
    """the rule, re_step and Python's re on every string of length 0 to 7 over acgn"""
    import rnamotif_amd as R
    argv = descr_args(name, tmp_path)
    d = R.Descriptor(argv)
    strings = strings_over(b"acgn", 7)
    assert len(strings) == 21845
    entries, recs = string_records(strings, d.hit_stride)
    refused, image, rows, fixed, status, out = run_checker(seq_checker, tmp_path, argv, entries, recs)
    assert refused is None, refused
    assert status == 0, [ln for ln in out.split("\n") if ln.startswith("MISMATCH")]
    assert len(rows) == len(strings) and all(r[0] in "KD" for r in rows)
    keep = np.array([r[0] == "K" for r in rows])
    want = np.array([expected(name, s.decode())[0] for s in strings])
    bad = np.flatnonzero(keep != want)
    assert bad.size == 0, [(strings[i], bool(keep[i])) for i in bad[:5]]
    assert int(keep.sum()) == MATCHES[int(name[5:])]
    assert np.array_equal(fixed, recs)
    print("%s: %d of %d match, image %s, most steps %d" % (name, keep.sum(), len(strings), image, max(r[2] for r in rows)))


@pytest.mark.parametrize("name", sorted(IUPAC0))
def test_every_short_string_iupac0(built, seq_checker, tmp_path, name):
    """the three iupac = 0 cases on every string of length 0 to 5 over acgnry; the mismatch word is re_mm_step's n_mm"""
    import rnamotif_amd as R
    argv = descr_args(name, tmp_path)
    d = R.Descriptor(argv)
    strings = strings_over(b"acgnry", 5)
    entries, recs = string_records(strings, d.hit_stride)
    refused, image, rows, fixed, status, out = run_checker(seq_checker, tmp_path, argv, entries, recs)
    assert refused is None, refused
    assert status == 0, [ln for ln in out.split("\n") if ln.startswith("MISMATCH")]
    keep = np.array([r[0] == "K" for r in rows])
    want = [expected(name, s.decode()) for s in strings]
    assert np.array_equal(keep, np.array([w[0] for w in want]))
    assert keep.any() and not keep.all()
    rows_want = recs.copy()
    if case_of(name)[4]:
        for h in np.flatnonzero(keep):
            rows_want[h, HDR + 3] = want[h][1]
        assert set(fixed[keep, HDR + 3].tolist()) == {0, 1}
    assert np.array_equal(fixed, rows_want)


@pytest.mark.parametrize("name", CASES)
def test_window_records(built, seq_checker, tmp_path_factory, name):
    r = window_case(name, seq_checker, tmp_path_factory)
    assert r["refused"] is None, r["refused"]
    assert r["status"] == 0, [ln for ln in r["out"].split("\n") if ln.startswith("MISMATCH")]
    recs = r["recs"]
    keep = np.array([x[0] == "K" for x in r["rows"]])
    want, rows_want = window_expectation(name, r["entries"], recs)
    assert len(keep) == len(recs) and np.array_equal(keep, want)
    assert np.array_equal(r["fixed"], rows_want)
    assert keep.any() and not keep.all()
    print("%s: %d records, %d kept" % (name, len(recs), keep.sum()))
    # both strands, an element at base 0 and one that ends at the entry's last base, kept and dropped
    lens = np.array([len(e) for e in r["entries"]])
    for comp in (0, 1):
        on = recs[:, 1] == comp
        assert (on & (recs[:, HDR] == 0)).any() and (on & (recs[:, HDR] + recs[:, HDR + 1] == lens[recs[:, 0]])).any()


def test_plants_at_the_ends_and_behind_the_element(built, seq_checker, tmp_path_factory):
    r = window_case("table01", seq_checker, tmp_path_factory)       # \(ac\)g\1, floating
    recs, keep = r["recs"], np.array([x[0] == "K" for x in r["rows"]])
    lens = [len(e) for e in r["entries"]]

    def at(seq, comp, off, n):
        h = np.flatnonzero((recs[:, 0] == seq) & (recs[:, 1] == comp) & (recs[:, HDR] == off) & (recs[:, HDR + 1] == n))
        assert h.size == 1
        return bool(keep[h[0]])

    # acgac at base 0 and at the last base, strand 0; gtcgt is acgac on strand 1
    assert at(0, 0, 0, 5) and at(1, 0, lens[1] - 5, 5)
    assert at(3, 1, lens[3] - 5, 5) and at(4, 1, 0, 5)
    # entry 2 holds acgac at 21: the element acga is dropped -- the c behind it is not the element's
    assert r["entries"][2][21:26] == b"acgac"
    assert at(2, 0, 21, 5) and not at(2, 0, 21, 4) and at(2, 0, 20, 7) and not at(2, 0, 22, 5)


def test_refusals(built, tmp_path):
    import rnamotif_amd as R
    # not loose: no expressions
    q = R.SeqCheck(R.Descriptor(["-descr", os.path.join(GOLDEN, "descr", "trna.descr")]))
    assert q.info["expressions"] == 0 and q.info["ops"] == 0 and q.info["waves_per_workgroup"] == 4
    q.close()
    q.close()
    score = "score\n\t{ SCORE = 1; }\n"
    d = R.Descriptor(descr_args("literal_n", tmp_path, hairpin=True, score=score))
    q = R.SeqCheck(d)
    assert q.info["expressions"] == 1 and q.info["ops"] == 4 and q.info["frames"] == 0
    words = ("the score section cannot run on the device: the descriptor is loose (element 1's seq= is tested by a necessary condition only): "
             "its records are not yet the reference's candidates")
    with pytest.raises(R.RnamotifError) as e:
        R.ScoreProgram(d)
    assert str(e.value) == words and R.ScoreProgram.reason(d) == words
    assert R.ScoreProgram.reason(d, checked=True) is None
    p = R.ScoreProgram(d, checked=True)
    assert p.checked
    p.close()
    # every other refusal stays
    s = R.Descriptor(["-descr", os.path.join(GOLDEN, "test", "sprintf.descr")])
    assert "sprintf()" in R.ScoreProgram.reason(s) and R.ScoreProgram.reason(s, checked=True) == R.ScoreProgram.reason(s)
    d2 = R.Descriptor(descr_args("table00", tmp_path, hairpin=True, score="score\n\t{ if( NAME == \"e\" ) REJECT; }\n"))
    assert "loose" in R.ScoreProgram.reason(d2) and "NAME" in R.ScoreProgram.reason(d2, checked=True)
    # the frames of the image: the most repeating ops of one expression
    assert R.SeqCheck(R.Descriptor(descr_args("table10", tmp_path))).info["frames"] == 3


def test_limits_are_refused_at_open(built, tmp_path):
    import rnamotif_amd as R
    # 21 loose elements
    text = "parms\n\tiupac = 0;\ndescr\n" + "".join('\tss(minlen=4,maxlen=5,seq="^nnac")\n' for _ in range(21))
    (tmp_path / "many.descr").write_text(text)
    with pytest.raises(R.RnamotifError, match="more than 20 elements have a loose seq="):
        R.SeqCheck(R.Descriptor(["-descr", str(tmp_path / "many.descr")]))


def test_budget(built, seq_checker, tmp_path):
    """^.*\\(g.\\).*\\1.*$ over a 60-base element of g and a with 64 steps: the records that need more stop, and those
    are the ones the rule itself counts beyond 64 with room to run"""
    import rnamotif_amd as R
    name = "table10"
    argv = descr_args(name, tmp_path)
    d = R.Descriptor(argv)
    # one g among 59 a: no second "g." for the back reference, and every position of the first .* is tried
    long = b"a" * 30 + b"g" + b"a" * 29
    entries = [b"gcgc" + long + b"tttt"]
    recs = np.zeros((4, d.hit_stride), dtype=np.int32)
    for h, (off, n) in enumerate(((0, 4), (4, 6), (4, 60), (2, 64))):
        recs[h, 2], recs[h, HDR], recs[h, HDR + 1] = off, off, n
    _, _, free, _, status, _ = run_checker(seq_checker, tmp_path, argv, entries, recs)
    assert status == 0 and all(r[0] in "KD" for r in free)
    steps = [r[2] for r in free]
    assert steps[0] <= 64 < steps[2], steps
    _, _, rows, fixed, status, _ = run_checker(seq_checker, tmp_path, argv, entries, recs, budget=64)
    assert status == 0
    for h in range(4):
        if steps[h] > 64:
            assert rows[h] == ("S", 0, 65)
        else:
            assert rows[h] == free[h]
    assert min(h for h in range(4) if rows[h][0] == "S") == min(h for h in range(4) if steps[h] > 64)
    assert np.array_equal(fixed, recs)
    print("steps without a budget:", steps)


def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "rnamotif_amd.h")).read()
    for words in ("typedef struct rma_seqcheck\trma_seqcheck_t;",
                  "int\trma_seqcheck_open( const rma_descr_t *d, rma_seqcheck_t **out, char *err, size_t errlen );",
                  "void\trma_seqcheck_close( rma_seqcheck_t *sq );", "void\trma_seqcheck_info( const rma_seqcheck_t *sq, int32_t info[ 8 ] );",
                  "int\trma_seqcheck_hits( rma_scanner_t *sc, const rma_seqcheck_t *sq, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,",
                  "int\trma_score_open_checked( const rma_descr_t *d, rma_score_t **out, char *err, size_t errlen );", "csrc/rm_seqcheck.h"):
        assert words in text


def test_exports(built):
    import ctypes
    lib = ctypes.CDLL(built["lib"])
    for n in ("rma_seqcheck_open", "rma_seqcheck_close", "rma_seqcheck_info", "rma_seqcheck_hits", "rma_score_open_checked"):
        assert hasattr(lib, n), n


def test_checker_under_sanitizers(built, tmp_path_factory):
    """the rule's host instance, built with -fsanitize=address,undefined as the stand-alone program it is, on one case"""
    san = build_checker(sanitize=True)
    _windows.pop("table10", None)
    r = window_case("table10", san, tmp_path_factory)
    _windows.pop("table10", None)
    assert r["refused"] is None and r["status"] == 0 and len(r["rows"]) == len(r["recs"])
