"""CPU: the score section with =~, !~ and mismatches( string, pattern ) -- an image opened with RMA_SCORE_MATCH (8) -- as
rnamotif_amd/csrc/rm_score_core.h states it for the host and for rma_score_match_kernel / rma_score_match_text_kernel, run
on the host through tests/hostsim/score_match_check.cpp ( rms_run_t< *, true > over planes of stride 1 ) against
ScoreVM::run and HitPrinter::print:

  * own descriptors, one construct each (OWN_MATCH), over the oracle's records of the first 30 entries of the reference's
    test database, under flags 8 and 8 | 2: outcome, kind, the bits of the score and (with text) the column of every
    record.  Not vacuous: every =~ program is written so that the host VM's outcome tells whether its condition held -- a
    REJECT on one side, an odd SCORE for a match and an even one for none on the other -- and at least 50 records are on
    either side; every mismatches() program takes at least three values.  Both are counted on the host VM's side;
  * the matcher through the program: 24 patterns, each over every string of up to 5 letters of acgt -- the 1364 that are
    not empty as entries whose one ss element is the whole entry, "" as a constant of the same program -- with =~ and
    mismatches() through the rule equal to re_step() and re_mm_step();
  * refusals and stops with their words, the flags, and images of programs without a pattern, which bit 8 leaves alone."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from test_score_device_cpu import FRONT_END, GOLDEN, GOLDEN_CASES, H, HP, ROOT, counts, descr_args, entries_of, own_args, scan_case  # noqa: F401
from test_score_text_cpu import GOLDEN_TEXT, run_text_checker, text_args

BIN = os.path.join(ROOT, "tests", "_build", "score_match_check")
CHECKED, TEXT, MATCH = 1, 2, 8

LOOSE = ("parms\n\twc += gu;\ndescr\n\th5( tag='a', minlen=4, maxlen=6, mispair=1 )\n\t\tss( tag='l', minlen=4, maxlen=6, seq=\"\\(.\\)\\1\" )\n"
         "\th3( tag='a' )\nscore\n")

# name -> (descriptor, what a REJECT says of the program's condition: "match", "none" or None (it never rejects), needs text?)
# An accepted record's SCORE is odd where the condition held and even where it did not.
OWN_MATCH = {
    "anchored": (HP + "\t{ if( ss( tag='l' ) =~ \"^ga\" ) REJECT; SCORE = 2; }\n", "match", False),
    "unanchored": (HP + "\t{ m = 0; if( h5( tag='a' ) =~ \"gg\" ) m = 1; SCORE = m; }\n", None, False),
    "$ and .": (HP + "\t{ if( ss( tag='l' ) =~ \"g.a$\" ) REJECT; SCORE = 2; }\n", "match", False),
    "star": (HP + "\t{ m = 0; if( h5( tag='a' ) =~ \"^g*c\" ) m = 1; SCORE = m; }\n", None, False),
    "range": (HP + "\t{ m = 0; if( h5( tag='a' ) =~ \"[ag]\\{2,3\\}c\" ) m = 1; SCORE = m + 10; }\n", None, False),
    "class and negated class": (HP + "\t{ if( h3( tag='a' ) =~ \"^[ag][^ag]\" ) REJECT; SCORE = 4; }\n", "match", False),
    "back reference": (HP + "\t{ m = 0; if( h5( tag='a' ) =~ \"\\(..\\).*\\1\" ) m = 1; SCORE = m; }\n", None, False),
    "starred back reference": (HP + "\t{ m = 0; if( ss( tag='l' ) =~ \"^\\(.\\)\\1*[^a]\" ) m = 1; SCORE = m; }\n", None, False),
    "word brackets": (HP + "\t{ m = 0; if( ss( tag='l' ) =~ \"\\<g.*a\\>\" ) m = 1; SCORE = m; }\n", None, False),
    "!~": (HP + "\t{ if( ss( tag='l' ) !~ \"a.*a\" ) REJECT; SCORE = 1; }\n", "none", False),
    "inside && and ||": (HP + "\t{ m = 0; if( LEN > 14 && ss( tag='l' ) =~ \"^g\" || h5( tag='a' ) =~ \"cc\" ) m = 1; SCORE = m; }\n", None, False),
    "in a loop": (HP + "\t{ m = 0; for( i = 1; i <= 3; i++ ){ if( se( index=i ) =~ \"gc\" ) m = 1; } SCORE = m; }\n", None, False),
    "pos= and len=": (HP + "\t{ if( h5( tag='a', pos=2, len=3 ) =~ \"^[cg][cg]\" ) REJECT; SCORE = 2; }\n", "match", False),
    "substr": (HP + "\t{ m = 0; if( substr( ss( tag='l' ), 2, 3 ) =~ \"a.$\" ) m = 1; SCORE = m; }\n", None, False),
    "a string constant": (HP + "\t{ m = 0; if( \"gattaca\" =~ \"t\\{2\\}\" && ss( tag='l' ) =~ \"^g\" ) m = 1; if( \"gattaca\" =~ \"^a\" ) REJECT; SCORE = m; }\n", None, False),
    "a variable": (HP + "\t{ s = ss( tag='l' ); m = 0; if( s =~ \"c\" ) m = 1; SCORE = m; }\n", None, False),
    "a + b": (HP + "\t{ s = h5( tag='a' ) + ss( tag='t' ); m = 0; if( s =~ \"g[ct].$\" ) m = 1; SCORE = m; }\n", None, True),
    "sprintf": (HP + "\t{ s = sprintf( '%s-%d', ss( tag='l' ), LEN ); if( s =~ \"a-1[0-5]$\" ) REJECT; SCORE = 2; }\n", "match", True),
    "an empty left string": (HP + "\t{ e = \"\"; if( e =~ \"a\" ) REJECT; m = 0; if( e =~ \"^$\" && ss( tag='l' ) =~ \"^g\" ) m = 1; SCORE = m; }\n", None, False),
    "an empty pattern": (HP + "\t{ m = 0; if( ss( tag='l' ) =~ \"\" || ss( tag='l' ) =~ \"^g\" ) m = 1; SCORE = m + 2 * mismatches( ss( tag='l' ), \"\" ); }\n", None, False),
    "a loose descriptor": (LOOSE + "\t{ if( ss( tag='l' ) =~ \"^g\" ) REJECT; SCORE = 2; }\n", "match", False),
}
# name -> (descriptor, needs text?): SCORE is the builtin's value
OWN_MISMATCHES = {
    "fixed length": (HP + "\t{ SCORE = mismatches( ss( tag='l' ), \"gaa\" ); }\n", False),
    "anchored": (HP + "\t{ SCORE = mismatches( h5( tag='a' ), \"^gc[ag]c\" ); }\n", False),
    "with a star": (HP + "\t{ SCORE = mismatches( ss( tag='l' ), \"ga*c.g\" ); }\n", False),
    "with a group": (HP + "\t{ SCORE = mismatches( h5( tag='a' ), \"\\(g.\\)c\\1\" ); }\n", False),
    "with $": (HP + "\t{ SCORE = mismatches( ss( tag='l' ), \"ga[^c].$\" ); }\n", False),
    "of a made string": (HP + "\t{ SCORE = mismatches( ss( tag='t' ) + h3( tag='a' ), \"^a\\{2\\}gc\" ); }\n", True),
}
PATTERNS = ["a", "^a", "a$", "^$", ".", "a.c", "a*", "^a*c", "ca*t", "[ac]g", "[^ac]", "^[a-g]*$", "a\\{2\\}", "a\\{1,2\\}c", "g\\{2,\\}", "\\(a\\)\\1",
            "\\(..\\).*\\1", "^\\(.\\)\\1*$", "\\(a*\\)c\\1", "\\<a", "a\\>", "\\<ac\\>", ".*\\(..\\).*\\1", "\\(.\\)\\(.\\)\\2\\1"]
STRINGS = "descr\n\tss( tag='s', minlen=1, maxlen=5 )\nscore\n"
BUDGET = (HP + "\t{ s = ss( tag='l' ) + h5( tag='a' ); s = s + s; s = s + \"t\" + s; if( s =~ \".*\\(..\\).*\\1\" ) REJECT; SCORE = 1; }\n")
# name -> (descriptor or file under tests/golden, flags beside 8, words of the refusal)
REFUSED_MATCH = {
    "a pattern from a variable": (HP + "\t{ p = \"^g\"; if( ss( tag='l' ) =~ p ) REJECT; }\n", 0, "the pattern of =~ / !~ is not one string constant"),
    "a pattern from sprintf()": (HP + "\t{ if( ss( tag='l' ) =~ sprintf( '^%s', 'g' ) ) REJECT; }\n", TEXT, "the pattern of =~ / !~ is not one string constant"),
    "a pattern from an element": (HP + "\t{ SCORE = mismatches( ss( tag='l' ), ss( tag='t' ) ); }\n", 0, "the pattern of mismatches( string, pattern ) is not one string constant"),
    "an unmatched \\(": (HP + "\t{ if( ss( tag='l' ) =~ \"\\(ga\" ) REJECT; }\n", 0, "the pattern '\\(ga' of =~ / !~ is no regular expression (regerr 42)"),
    "\\{3,2\\}": (HP + "\t{ SCORE = mismatches( ss( tag='l' ), \"a\\{3,2\\}\" ); }\n", 0, "the pattern 'a\\{3,2\\}' of mismatches( string, pattern ) is no regular expression (regerr 46)"),
    "33 expressions": (HP + "\t{ n = 0;\n" + "".join("\t  if( ss( tag='l' ) =~ \"g\\{%d\\}\" ) n = n + 1;\n" % k for k in range(1, 34)) + "\t  SCORE = n; }\n", 0,
                       "more than 32 patterns"),
    "NAME": (HP + "\t{ if( NAME =~ \"e\" ) REJECT; }\n", 0, "NAME"),
    "getbest": ("test/getbest.descr", 0, "HOLD / RELEASE"),
}


def build_match_checker():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "hostsim", "score_match_check.cpp")
    units = [os.path.join(H, u + ".cpp") for u in FRONT_END]
    deps = [src] + units + [os.path.join(H, f) for f in os.listdir(H) if f.endswith(".h")] + [os.path.join(ROOT, "include", "rnamotif_amd_program.h")]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(f) for f in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + H,
                        "-o", BIN, src] + units, check=True)
    return BIN


@pytest.fixture(scope="module")
def match_checker():
    return build_match_checker()


def vm_counts(out):
    """the checker's count of the host VM's side: (accepted, rejected, stopped, {int SCORE: records})"""
    ln = [x for x in out.split("\n") if x.startswith("VM ")][-1].split()
    a, r, s = (int(w.split("=")[1]) for w in ln[1:4])
    scores = {int(k): int(v) for k, v in (kv.split(":") for kv in ln[4].split("=")[1].split(",") if kv)} if len(ln) > 4 else {}
    return a, r, s, scores


def run_match_checker(checker, tmp, argv, entries, recs, flags, heap=256, stride=64, budget=0):
    """score_match_check run: as run_text_checker (the two print the same lines), the host VM's counts in place of BITS"""
    refused, image, rows, status, out, _ = run_text_checker(checker, tmp, argv, entries, recs, flags=flags, heap=heap, stride=stride, budget=budget)
    return refused, image, rows, status, out, (vm_counts(out) if refused is None else None)


def own_flags(needs_text):
    return (MATCH | TEXT,) if needs_text else (MATCH, MATCH | TEXT)


def is_loose(name):
    return name == "a loose descriptor"


@pytest.mark.parametrize("name", sorted(OWN_MATCH))
def test_own_match_descriptors(built, match_checker, gbrna, tmp_path, name):
    text, rejects, needs_text = OWN_MATCH[name]
    argv = own_args(text, tmp_path, name)
    d, entries, recs = scan_case(argv, gbrna, 30)
    for flags in own_flags(needs_text):
        flags |= CHECKED if is_loose(name) else 0
        refused, image, rows, status, out, vm = run_match_checker(match_checker, tmp_path, argv, entries, recs, flags)
        assert refused is None, refused
        assert status == 0, [ln for ln in out.split("\n") if ln.startswith("MISMATCH")]
        a, r, s, scores = vm
        held = sum(n for v, n in scores.items() if v % 2) + (r if rejects == "match" else 0)
        not_held = sum(n for v, n in scores.items() if v % 2 == 0) + (r if rejects == "none" else 0)
        print("%s, flags %d: %d records, the condition held on %d and not on %d; image %s" % (name, flags, len(recs), held, not_held, image))
        assert len(rows) == len(recs) == a + r and s == 0 and counts(rows)["S"] == 0
        assert (rejects is not None) == (r > 0) and held + not_held == len(recs)
        assert held >= 50 and not_held >= 50, (held, not_held)
        assert image["flags"] & 2 and image["expr"] >= 1 and bool(image["flags"] & 1) == bool(flags & TEXT)
        if flags & TEXT:
            assert all(x[3] == len(x[4]) >= 8 for x in rows if x[0] == "A")


@pytest.mark.parametrize("name", sorted(OWN_MISMATCHES))
def test_own_mismatches_descriptors(built, match_checker, gbrna, tmp_path, name):
    text, needs_text = OWN_MISMATCHES[name]
    argv = own_args(text, tmp_path, name)
    d, entries, recs = scan_case(argv, gbrna, 30)
    for flags in own_flags(needs_text):
        refused, image, rows, status, out, vm = run_match_checker(match_checker, tmp_path, argv, entries, recs, flags)
        assert refused is None, refused
        assert status == 0, [ln for ln in out.split("\n") if ln.startswith("MISMATCH")]
        a, r, s, scores = vm
        print("%s, flags %d: %d records, values %s" % (name, flags, len(recs), scores))
        assert len(rows) == len(recs) == a and r == 0 and s == 0 and len(scores) >= 3, scores


@pytest.fixture(scope="module")
def strings_case(built, tmp_path_factory):
    """every string of 1 to 5 letters of acgt as an entry, and the record of each whose one element is the whole entry"""
    import rnamotif_amd as R
    from oracle_binding import oracle_scan
    tmp = tmp_path_factory.mktemp("score_match_strings")
    entries = ["".join(t).encode() for n in range(1, 6) for t in itertools.product("acgt", repeat=n)]
    d = R.Descriptor(own_args(STRINGS + "\t{ SCORE = 1; }\n", tmp, "scan"))
    recs = oracle_scan(d, entries)
    lens = np.array([len(e) for e in entries])
    whole = recs[(recs[:, 1] == 0) & (recs[:, 5] == 0) & (recs[:, 6] == lens[recs[:, 0]])]
    assert len(entries) == 1364 and len(whole) == 1364 and sorted(whole[:, 0].tolist()) == list(range(1364))
    return tmp, entries, whole


@pytest.mark.parametrize("k", range(len(PATTERNS)))
def test_the_matcher_through_the_program(match_checker, strings_case, k):
    tmp, entries, recs = strings_case
    pat = PATTERNS[k]
    text = STRINGS + ("\t{ SCORE = 2 * mismatches( ss( tag='s' ), \"%s\" ) + ( ss( tag='s' ) =~ \"%s\" ) + 1000 * ( 2 * mismatches( \"\", \"%s\" ) + ( \"\" =~ \"%s\" ) ); }\n"
                      % (pat, pat, pat, pat))
    argv = own_args(text, tmp, "pattern %d" % k)
    ent, rec = os.path.join(str(tmp), "entries.bin"), os.path.join(str(tmp), "records.bin")
    if not os.path.exists(ent):
        with open(ent, "wb") as f:
            f.write(np.asarray([len(entries)] + [len(e) for e in entries], dtype=np.int32).tobytes())
            f.write(b"".join(entries))
        np.ascontiguousarray(recs, dtype=np.int32).tofile(rec)
    import rnamotif_amd as R
    p = subprocess.run([match_checker, "strings", pat, ent, rec, "0", str(MATCH), "256", "0"] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600,
                       env=dict(os.environ, EFNDATA=os.environ.get("EFNDATA", R.EFNDATA_DIR)))
    out = p.stdout.decode()
    last = [ln for ln in out.split("\n") if ln.startswith("STRINGS ")]
    assert p.returncode == 0 and last, out[-1500:] + p.stderr.decode()[-500:]
    a, r, s, scores = vm_counts(out)
    print("%s: %s, %d values" % (pat, last[0], len(scores)))
    assert last[0] == "STRINGS checked=1364 bad=0" and a == 1364 and "MISMATCH" not in out
    assert "expr=4 " in out.split("\n")[0]


@pytest.mark.parametrize("name", sorted(REFUSED_MATCH))
def test_refusals(built, match_checker, tmp_path, name):
    import rnamotif_amd as R
    what, more, words = REFUSED_MATCH[name]
    argv = ["-descr", os.path.join(GOLDEN, what)] if what.endswith(".descr") else own_args(what, tmp_path, name)
    refused, _, _, status, _, _ = run_match_checker(match_checker, tmp_path, argv, [b"acgt"], np.zeros((0, 1), dtype=np.int32), MATCH | more)
    assert status == 0 and refused is not None and words in refused, refused
    assert name in ("NAME", "getbest") or ".descr:" in refused        # (file and line)
    d = R.Descriptor(argv)
    assert R.ScoreProgram.reason(d, text=bool(more & TEXT), match=True) == refused
    with pytest.raises(R.RnamotifError) as e:
        R.ScoreProgram(d, text=bool(more & TEXT), match=True)
    assert words in str(e.value)


def test_32_expressions_open(built, match_checker, tmp_path):
    text = HP + "\t{ n = 0;\n" + "".join("\t  if( ss( tag='l' ) =~ \"g\\{%d\\}\" ) n = n + 1;\n" % k for k in range(1, 33)) + "\t  SCORE = n; }\n"
    refused, image, _, status, _, _ = run_match_checker(match_checker, tmp_path, own_args(text, tmp_path, "32"), [b"acgt"], np.zeros((0, 1), dtype=np.int32), MATCH)
    assert refused is None and image["expr"] == 32 and image["frames"] == 1


def test_match_on_an_int_stops(built, match_checker, gbrna, tmp_path):
    """the host VM's own word for it, in one word"""
    argv = own_args(HP + "\t{ x = LEN; if( x =~ \"1\" ) REJECT; SCORE = 1; }\n", tmp_path, "int")
    d, entries, recs = scan_case(argv, gbrna, 30)
    refused, image, rows, status, out, vm = run_match_checker(match_checker, tmp_path, argv, entries, recs, MATCH)
    assert refused is None and status == 0, out[-500:]
    assert len(rows) == len(recs) > 0 and all(r[0] == "S" and r[5].endswith(".descr:9 typemismatch.") for r in rows) and vm[2] == len(recs)


def test_the_budget_stops_a_backtracking_pattern(built, match_checker, gbrna, tmp_path):
    """.*\\(..\\).*\\1 over a string of some forty letters the record makes: the matcher's ops count against the record's
    budget with the instructions, and a record over it stops with the budget's words, which the host VM has not"""
    argv = own_args(BUDGET, tmp_path, "budget")
    d, entries, recs = scan_case(argv, gbrna, 30)
    refused, image, rows, status, out, vm = run_match_checker(match_checker, tmp_path, argv, entries, recs, MATCH | TEXT, budget=100)
    assert refused is None and status == 0 and image["inst"] < 100, out[-500:]
    c = counts(rows)
    print(len(recs), c, image)
    # (a record whose string repeats a pair early is matched, and rejected, inside the budget)
    assert c["S"] >= 50 and c["S"] + c["R"] + c["A"] == len(recs) and vm[2] == 0
    assert all("more than 100 instructions for one record (option score_budget)." in r[5] and ".descr:9 " in r[5] for r in rows if r[0] == "S")
    # with the default budget every record is judged, and the two sides agree
    refused, image, rows, status, out, vm = run_match_checker(match_checker, tmp_path, argv, entries, recs, MATCH | TEXT)
    assert status == 0 and counts(rows)["S"] == 0


def test_flags(built, tmp_path):
    import rnamotif_amd as R
    ire = R.Descriptor(["-descr", os.path.join(GOLDEN, "test", "ire.descr")])
    trna = R.Descriptor(["-descr", os.path.join(GOLDEN, "descr", "trna.descr")])
    mat = R.Descriptor(own_args(OWN_MATCH["anchored"][0], tmp_path, "anchored"))
    mm = R.Descriptor(own_args(OWN_MISMATCHES["fixed length"][0], tmp_path, "mm"))
    err, h = C.create_string_buffer(2048), C.c_void_p()

    def opened(d, flags):
        rc = R.lib().rma_score_open_flags(d._h, flags, C.byref(h), err, 2048)
        if rc == 0:
            R.lib().rma_score_close(h)
            return None
        assert not h.value
        return err.value.decode()
    for flags in range(16):
        if flags & 4:
            assert "flags" in opened(ire, flags)
            continue
        # the flag alone opens what opened and refuses, in the same words, what was refused for another reason
        assert opened(ire, flags) is None
        assert opened(trna, flags) == opened(trna, flags & ~MATCH) and (opened(trna, flags) is None) == bool(flags & TEXT)
        assert (opened(mat, flags) is None) == bool(flags & MATCH) == (opened(mm, flags) is None)
    assert "=~ and !~ operators need the host's regular expressions" in R.ScoreProgram.reason(mat)
    assert "=~ and !~" in R.ScoreProgram.reason(mat, True, True)
    assert "mismatches( string, pattern ) needs the host's regular expressions" in R.ScoreProgram.reason(mm, text=True)
    assert R.ScoreProgram.reason(mat, match=True) is None and R.ScoreProgram.reason(mm, False, False, True) is None
    p = R.ScoreProgram(mat, match=True)
    assert p.match and not p.text and not p.checked and p.info()["instructions"] > 0
    p.close()
    p = R.ScoreProgram(ire, True, True)
    assert p.checked and p.text and not p.match
    p.close()
    text = open(os.path.join(ROOT, "include", "rnamotif_amd.h")).read()
    assert "#define RMA_SCORE_MATCH   8u" in text and "#define RMA_SCORE_TEXT    2u" in text


@pytest.mark.parametrize("name", sorted(GOLDEN_CASES) + ["text:" + n for n in sorted(GOLDEN_TEXT)])
def test_old_images_are_unchanged(built, match_checker, tmp_path, name):
    """bit 8 alone changes nothing of a program without a pattern but the flag: no table, not a byte more"""
    if name.startswith("text:"):
        argv, base = text_args(name[5:])[0], TEXT
    else:
        argv, base = descr_args(name), 0
    none = np.zeros((0, 1), dtype=np.int32)
    r0, i0, _, s0, _, _ = run_match_checker(match_checker, tmp_path, argv, [b"acgt"], none, base)
    r8, i8, _, s8, _, _ = run_match_checker(match_checker, tmp_path, argv, [b"acgt"], none, base | MATCH)
    assert r0 is None and r8 is None and s0 == 0 and s8 == 0, (r0, r8)
    for key in ("bytes", "inst", "vars", "stack", "deepest", "pool", "pairsets", "wave_bytes", "bits_L", "table"):
        assert i0[key] == i8[key], key
    assert i8["flags"] == i0["flags"] | 2 and i8["expr"] == i0["expr"] == 0 and i8["frames"] == -1
