"""CPU: generated score programs, programs of every workgroup shape and programs at the image's limits (tests/score_programs.py)
through the host checkers -- score_check, score_text_check, score_match_check, which run the rule of rm_score_core.h against
ScoreVM::run and HitPrinter::print record by record -- over the oracle's records of the first 30 entries of the reference's
test database (4625 records of HP, 5077 of CTX with -context):

  * N = 200 seeds a family (plain, text, match, match_text), sizes 0 .. 3 in turn: every program that opens agrees on every
    record -- outcome, kind, the bits of SCORE, the score column, the words of a stop;
  * the corpus is not empty (counts of this corpus, asserted below as bounds):
        family      open  refused  no stop  accept and reject  stop on some records  waves 4 / 3 / 2 / 1
        plain        200     0       151          153                 49              50 / 49 /  50 / 51
        text         200     0       168          152                 32              43 / 38 /  69 / 50
        match        200     0       145          129                 55              20 / 40 /  90 / 50
        match_text   200     0       152          132                 48              18 / 41 /  91 / 50
    every feature of score_programs.features_of( family ) is used by at least 10 programs; no program is refused, so the
    listed set of refusals is empty;
  * sized( family, waves ): 16 programs whose IMAGE line gives exactly 4, 3, 2 and 1 waves for each of the four kernels;
  * limits(): the stack, the variables, LDS (through the stack and through the matcher's frames), instructions, the string
    pool, pair sets and expressions, each at its limit (it runs, accepts and rejects) and one beyond (refused with its words);
  * the element stack at RMS_ESTK, by nesting and by calls that leave their element: the rule stops where the host VM does;
    a $ read behind a reference nested in pos=;
  * `$` behind an explicit left context (found by seed 1 of this corpus);
  * all of it, with 50 seeds a family, through score_match_check built with -fsanitize=address,undefined as the stand-alone
    program it is: the rule stays inside its planes, its element stack and its heap.

The file takes about 80 s, 35 s of them under the sanitizers.  What a mutated rule does to it
(scratch copies of rm_score_core.h, never committed) is in DESIGN.md's score section."""
import collections
import os
import subprocess

import pytest

import score_programs as SP
from test_score_device_cpu import CTX, FRONT_END, H, HP, ROOT, counts, scan_case

N = 200
N_SAN = 50
# the words a generated program may be refused with: none -- the generator is written to ScoreVM::hit_independent
REFUSALS = ()
SAN = os.path.join(ROOT, "tests", "_build", "score_match_check_san")


@pytest.fixture(scope="module")
def checkers(built):
    return SP.build_checkers()


@pytest.fixture(scope="module")
def records(built, gbrna, tmp_path_factory):
    """uses -context? -> (entries, the oracle's records): the records are the descriptor's, whatever its score section"""
    tmp = tmp_path_factory.mktemp("score_programs_scan")
    out = {}
    for ctx, base, extra in ((False, HP, []), (True, CTX, ["-context"])):
        argv = extra + ["-descr", SP.write_descr(base + "\t{ SCORE = 1; }\n", tmp, "scan%d" % ctx)]
        d, entries, recs = scan_case(argv, gbrna, 30)
        assert len(recs) > 1000 and (recs[:, 1] == 0).sum() > 100 and (recs[:, 1] == 1).sum() > 100
        out[ctx] = (entries, recs)
    return out


def run(checker, family, text, extra, records, tmp, san=None):
    argv = list(extra) + ["-descr", SP.write_descr(text, tmp, "program")]
    entries, recs = records[bool(extra)]
    return SP.run_family(checker, family, tmp, argv, entries, recs, checker_of_family=san)


def mismatches(out):
    return [ln for ln in out.split("\n") if ln.startswith("MISMATCH")]


@pytest.fixture(scope="module")
def corpus(checkers, records, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("score_programs")
    res = {}
    for family in SP.FAMILIES:
        for seed in range(N):
            text, extra, feats = SP.generate(seed, family, seed % 4)
            refused, image, rows, status, out = run(checkers[family], family, text, extra, records, tmp)
            res[(family, seed)] = {"text": text, "features": feats, "refused": refused, "image": image, "counts": counts(rows), "status": status,
                                   "bad": mismatches(out), "n": len(rows)}
    return res


@pytest.mark.parametrize("family", SP.FAMILIES)
def test_rule_and_host_vm_agree_on_generated_programs(corpus, family):
    for seed in range(N):
        r = corpus[(family, seed)]
        if r["refused"] is None:
            assert r["status"] == 0 and not r["bad"], (family, seed, r["bad"][:1], r["text"])


@pytest.mark.parametrize("family", SP.FAMILIES)
def test_the_corpus_is_not_empty(corpus, records, family):
    rs = [corpus[(family, seed)] for seed in range(N)]
    opened = [r for r in rs if r["refused"] is None]
    refusals = collections.Counter(r["refused"] for r in rs if r["refused"] is not None)
    no_stop = sum(r["counts"]["S"] == 0 for r in opened)
    both = sum(r["counts"]["A"] > 0 and r["counts"]["R"] > 0 for r in opened)
    some = sum(0 < r["counts"]["S"] < r["n"] for r in opened)
    waves = collections.Counter(SP.waves_of(r["image"]) for r in opened)
    feats = collections.Counter(f for r in opened for f in r["features"])
    print("%s: %d open, %d refused, %d without a stop, %d accept and reject, %d stop on some records, waves %s" %
          (family, len(opened), len(rs) - len(opened), no_stop, both, some, [waves[w] for w in (4, 3, 2, 1)]))
    print("  features: %s" % {f: feats[f] for f in SP.features_of(family)})
    assert all(r["n"] == len(records["-context" in r["text"] or "ctx(" in r["text"]][1]) for r in opened)
    assert len(opened) >= 0.8 * N
    for words in refusals:
        assert any(w in words for w in REFUSALS), words       # (a syntax error or "too many labels" ends the checker: run() fails)
    assert no_stop >= 0.6 * len(opened)
    assert both >= 0.5 * len(opened)
    assert 0.15 * len(opened) <= some <= 0.35 * len(opened)
    for f in SP.features_of(family):
        assert feats[f] >= 10, f
    for w in (1, 2, 3, 4):
        assert waves[w] >= 10, (w, waves)


def test_generate_is_deterministic():
    for family in SP.FAMILIES:
        assert SP.generate(7, family, 3) == SP.generate(7, family, 3) and SP.generate(7, family, 3)[0] != SP.generate(8, family, 3)[0]


@pytest.mark.parametrize("waves", [4, 3, 2, 1])
@pytest.mark.parametrize("family", SP.FAMILIES)
def test_sized_programs(checkers, records, tmp_path, family, waves):
    refused, image, rows, status, out = run(checkers[family], family, SP.sized(family, waves), [], records, tmp_path)
    assert refused is None, refused
    c = counts(rows)
    print(family, waves, image, c)
    assert SP.waves_of(image) == waves and 512 + image["bytes"] + waves * image["wave_bytes"] <= 65536
    assert status == 0 and not mismatches(out)
    assert len(rows) == len(records[False][1]) and c["S"] == 0 and c["A"] >= 100 and c["R"] >= 100
    assert len({(r[2], r[4]) for r in rows if r[0] == "A"}) >= 3, "one SCORE for every record"
    assert bool(image.get("expr", 0)) == bool(SP.FLAGS[family] & 8)


LIMITS = SP.limits()


@pytest.mark.parametrize("k", range(len(LIMITS)), ids=[x[0] for x in LIMITS])
def test_limits(built, checkers, records, tmp_path, k):
    import rnamotif_amd as R
    name, family, text, words, want = LIMITS[k]
    refused, image, rows, status, out = run(checkers[family], family, text, [], records, tmp_path)
    if words is not None:
        assert refused is not None and words in refused and status == 0, (refused, image)
        d = R.Descriptor(["-descr", os.path.join(str(tmp_path), "program.descr")])
        assert R.ScoreProgram.reason(d, text=bool(SP.FLAGS[family] & 2), match=bool(SP.FLAGS[family] & 8)) == refused
        return
    assert refused is None, refused
    c = counts(rows)
    print(name, image, c)
    for key, v in want.items():
        assert image[key] == v, (key, image)
    assert SP.waves_of(image) >= 1 and status == 0 and not mismatches(out)
    assert c["S"] == 0 and c["A"] >= 100 and c["R"] >= 100 and len({r[2] for r in rows if r[0] == "A"}) >= 3


ESTK = SP.element_stack()


@pytest.mark.parametrize("k", range(len(ESTK)), ids=[x[0] for x in ESTK])
def test_element_stack(checkers, records, tmp_path, k):
    """whatever the host VM does at the element stack's edge, the rule does the same, words included (the checker compares them)"""
    name, text, stops = ESTK[k]
    refused, image, rows, status, out = run(checkers["plain"], "plain", text, [], records, tmp_path)
    assert refused is None and status == 0 and not mismatches(out), (refused, mismatches(out)[:1])
    c = counts(rows)
    print(name, image, c)
    if stops:
        assert c["S"] == len(rows) and all(r[5].endswith("element stack overflow.") for r in rows)
    else:
        assert c["S"] == 0 and c["A"] >= 100 and c["R"] >= 100


DOLLAR = {
    "the last element": (CTX + "\t{ s = se( index=4, pos=2, len=$-2 ); if( LEN % 3 == 0 ) REJECT; SCORE = length( s ); }\n", True),
    "by its tag": (CTX + "\t{ s = h3( tag='a', pos=$, len=1 ); SCORE = length( s ); }\n", True),
    # (of any other element $ is the length of the element behind it: the helix's 5' strand reads the loop's)
    "an element in front of it": (CTX + "\t{ s = h5( tag='a', pos=1, len=$-3 ); if( LEN % 3 == 0 ) REJECT; SCORE = length( s ); }\n", False),
}


@pytest.mark.parametrize("name", sorted(DOLLAR))
def test_dollar_behind_an_explicit_context(checkers, records, tmp_path, name):
    """$ reads rm_descr by an index of rm_xdescr (sic, as the reference does).  Behind an explicit left context the last element's
    index is one past rm_descr: the reference reads what follows its array, the rule stops with the words of a $ outside a
    reference, and since seed 1 of the plain corpus showed the two apart, so does the host VM"""
    text, stops = DOLLAR[name]
    for family in ("plain", "match_text"):
        refused, image, rows, status, out = run(checkers[family], family, text, ["-context"], records, tmp_path)
        assert refused is None and status == 0 and not mismatches(out), (refused, mismatches(out)[:1])
        c = counts(rows)
        if stops:
            assert c["S"] == len(rows) > 1000 and all(r[5].endswith("'$' used outside a structure element reference.") for r in rows)
        else:
            assert c["S"] == 0 and c["A"] >= 100 and c["R"] >= 100 and len({r[2] for r in rows if r[0] == "A"}) == 3


def build_sanitized_checker():
    """score_match_check, which runs the rule of all four families, with -fsanitize=address,undefined: a stand-alone program"""
    src = os.path.join(ROOT, "tests", "hostsim", "score_match_check.cpp")
    units = [os.path.join(H, u + ".cpp") for u in FRONT_END] + [os.path.join(ROOT, "tests", "hostsim", "asan_options.cpp")]
    deps = [src] + units + [os.path.join(H, f) for f in os.listdir(H) if f.endswith(".h")] + [os.path.join(ROOT, "include", "rnamotif_amd_program.h")]
    os.makedirs(os.path.dirname(SAN), exist_ok=True)
    if not os.path.exists(SAN) or os.path.getmtime(SAN) < max(os.path.getmtime(f) for f in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g",
                        "-I" + os.path.join(ROOT, "include"), "-I" + H, "-o", SAN, src] + units, check=True)
    return SAN


def test_under_sanitizers(built, records, tmp_path):
    """the rule's host instance over the sized and limit programs, the element stack's edge and 50 seeds a family: a read or write
    outside the planes, the element stack or the heap ends the checker (run_family fails on its status), and the two sides
    still agree"""
    san = build_sanitized_checker()
    cases = [(family, SP.sized(family, w), []) for family in SP.FAMILIES for w in (4, 3, 2, 1)]
    cases += [(family, text, []) for name, family, text, words, want in LIMITS]
    cases += [("plain", text, []) for name, text, stops in ESTK] + [("text", DOLLAR[name][0], ["-context"]) for name in sorted(DOLLAR)]
    cases += [(family,) + SP.generate(seed, family, seed % 4)[:2] for family in SP.FAMILIES for seed in range(N_SAN)]
    ran = 0
    for family, text, extra in cases:
        refused, image, rows, status, out = run(san, family, text, extra, records, tmp_path, san=san)
        assert status == 0 and not mismatches(out), (family, mismatches(out)[:1], text)
        ran += refused is None
    print("%d programs, %d of them ran" % (len(cases), ran))
    assert ran >= 16 + 9 + 4 + 3 + 4 * N_SAN * 0.8
