"""CPU: the score section's MAIN program on one record as rnamotif_amd/csrc/rm_score_core.h states it for the host and for
rma_score_kernel, run on the host through tests/hostsim/score_check.cpp against ScoreVM::run, over the oracle's
records of the first entries of the reference's test database:

  * golden cases -- ire, ire.1, mp.ends, mp1.ends, mp.consec.not.ok, score.0 .. score.3, bulge, efn, each also with the
    reference's strict arguments (-sh -context -Dctx_maxlen=5): for every record the same outcome, and for an accepted
    record the same kind of SCORE and the same bits of its double (the checker compares; the same IEEE operations run
    in the same order);
  * not vacuous: every case whose program can reject accepts a record and rejects one over the entries taken (the
    counts of entries were chosen by running the oracle here); a case whose program never rejects, over the whole
    database, is listed as accept-only and held to accepting everything;
  * own descriptors, one construct each (OWN);
  * refusals with their words (REFUSED), stops with the host VM's words (STOPS).

A rejected record has no SCORE to compare: on the host the variable keeps what an earlier record left in it."""
import os
import subprocess

import numpy as np
import pytest

import pins
from test_hit_windows_cpu import normalise, odd_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "tests", "_build", "score_check")
FRONT_END = ["rm_regex", "rm_compile", "rm_parse", "rm_score", "rm_score_image", "rm_efndata", "rm_efn2data", "rm_fasta", "rm_driver",
             "rm_cli", "rm_dump", "rm_pack", "rm_stream"]

# name -> (file under tests/golden, entries of the database taken, can the program reject?)
# (the first entry count at which the oracle's records, plain and strict, hold an accepted and a rejected record: bulge
# 107, mp.consec.not.ok and score.2 264, mp.ends and mp1.ends 15, score.1 168, score.3 86.  efn.descr and score.0.descr
# reject nothing over all 4067 entries -- 445 / 327 and 108762 / 60338 records: accept-only.  ire.descr and ire.1.descr
# never reject over the whole database either, for want of anything to judge: the oracle finds NO candidate of theirs in
# its 4067 entries (2 264 722 bases), on either strand, plain or strict -- BASELINE.md's table has the same 0.  They are
# listed with the accept-only cases (None: and held to having no record at all, so that a database that gives them
# records is noticed); test_ire_over_synthetic_records holds the two programs to records they do have.)
GOLDEN_CASES = {
    "ire": ("test/ire.descr", 120, None),
    "ire.1": ("test/ire.1.descr", 120, None),
    "mp.ends": ("test/mp.ends.descr", 20, True),
    "mp1.ends": ("descr/mp1.ends.descr", 20, True),
    "mp.consec.not.ok": ("descr/mp.consec.not.ok.descr", 270, True),
    "score.0": ("descr/score.0.descr", 10, False),
    "score.1": ("test/score.1.descr", 170, True),
    "score.2": ("test/score.2.descr", 270, True),
    "score.3": ("descr/score.3.descr", 90, True),
    "bulge": ("test/bulge.descr", 110, True),
    "efn": ("test/efn.descr", 120, False),
}
ALL_GOLDEN = sorted(GOLDEN_CASES) + [n + ".strict" for n in sorted(GOLDEN_CASES)]
# ire.descr and ire.1.descr over entries 0, 5 and 7 of synthetic_records(10), BASELINE.md's syn10M: 7 records, 3 accepted;
# strict 2 records, 1 accepted
SYNTHETIC = {"ire.syn": "test/ire.descr", "ire.1.syn": "test/ire.1.descr"}
ALL_SYNTHETIC = sorted(SYNTHETIC) + [n + ".strict" for n in sorted(SYNTHETIC)]

HP = ("parms\n\twc += gu;\ndescr\n\th5( tag='a', minlen=4, maxlen=6, mispair=1 )\n\t\tss( tag='l', minlen=4, maxlen=6, seq=\"ga\", mismatch=1 )\n"
      "\th3( tag='a' )\n\tss( tag='t', len=2 )\nscore\n")
TRIP = ("descr\n\tt1( tag='1', minlen=3, maxlen=4, mispair=1 )\n\t\tss( minlen=3, maxlen=5 )\n\tt2( tag='1' )\n\t\tss( minlen=3, maxlen=5 )\n"
        "\tt3( tag='1' )\nscore\n")
QUAD = ("descr\n\tq1( tag='1', minlen=2, maxlen=3, mispair=1 )\n\t\tss( minlen=3, maxlen=4 )\n\tq2( tag='1' )\n\t\tss( minlen=3, maxlen=4 )\n"
        "\tq3( tag='1' )\n\t\tss( minlen=3, maxlen=4 )\n\tq4( tag='1' )\nscore\n")
CTX = ("parms\n\twc += gu;\ndescr\n\tctx( tag='L', minlen=2, maxlen=3 )\n\th5( tag='a', minlen=4, maxlen=6, mispair=1 )\n"
       "\t\tss( tag='l', minlen=4, maxlen=6 )\n\th3( tag='a' )\nscore\n")
# name -> (descriptor, arguments in front of -descr, entries taken, can the program reject?)
OWN = {
    "string variable": (HP + "\t{ s = ss( tag='l' ); t = h5( tag='a', pos=1, len=2 ); if( s < \"c\" ) REJECT; if( t == \"gg\" ) REJECT;\n"
                             "\t  SCORE = length( s ); }\n", [], 30, True),
    "substr": (HP + "\t{ s = substr( ss( tag='l' ), 2, 2 ); if( s == \"aa\" ) REJECT; u = substr( s, 2, 1 );\n"
                    "\t  if( u >= \"g\" ) SCORE = 1; else SCORE = 2; }\n", [], 30, True),
    "in": (HP + "\t{ if( h5( tag='a', pos=1, len=1 ):h3( tag='a', pos=$, len=1 ) in { \"g:c\", \"c:g\" } ) SCORE = 1;\n"
                "\t  else if( h5( tag='a', pos=2, len=2 ):h3( tag='a', pos=$-2, len=2 ):ss( tag='l', pos=1, len=2 ) in { \"g:c:a\", \"c:g:a\", \"a:t:g\", \"g:c:g\", \"t:a:t\", \"g:t:c\" } )\n"
                "\t\tSCORE = 2;\n\t  else REJECT; }\n", [], 30, True),
    "$": (HP + "\t{ s = h3( tag='a', pos=$-1, len=2 ); if( s == \"cc\" || s == \"gg\" ) REJECT; SCORE = length( h5( tag='a', pos=2, len=$-2 ) ); }\n", [], 30, True),
    "nested references": (HP + "\t{ if( h5( tag='a', pos=length( ss( tag='l', pos=$-3 ) ) - 2, len=length( ss( tag='t' ) ) ) < \"c\" ) REJECT;\n"
                               "\t  SCORE = length( h5( tag='a', pos=length( ss( tag='l' ) ) - 2 ) ); }\n", [], 30, True),
    "loc": (HP + "\t{ SCORE = loc( ss( tag='l' ) ) * 2 - loc( h5[ 1, 2 ] ); if( loc( h3( tag='a' ) ) > 700 ) REJECT; }\n", [], 30, True),
    "mismatches": (HP + "\t{ SCORE = mismatches( ss( tag='l' ) ); if( SCORE > 0 && LEN % 2 == 0 ) REJECT; }\n", [], 30, True),
    "mispairs": (HP + "\t{ SCORE = mispairs( h5( tag='a' ) ) + 2 * mispairs( se( index=3 ) ); if( SCORE > 0 && LEN % 2 == 0 ) REJECT; }\n", [], 30, True),
    "paired duplex": (HP + "\t{ if( !paired( h5( tag='a', pos=2, len=2 ) ) ) REJECT; SCORE = paired( h3( tag='a', pos=1, len=1 ) ) + 2 * paired( h5[ 1, 4, 9 ] ); }\n",
                      [], 30, True),
    "paired triplex": (TRIP + "\t{ if( !paired( t1( tag='1', pos=1, len=2 ) ) ) REJECT; SCORE = paired( t3( tag='1', pos=2, len=-1 ) ); }\n", [], 200, True),
    "paired 4-plex": (QUAD + "\t{ if( !paired( q1( tag='1', pos=1, len=2 ) ) ) REJECT; SCORE = paired( q3( tag='1', pos=1, len=1 ) ); }\n", [], 200, False),
    "%": (HP + "\t{ x = LEN % 4; y = 17; y %= 5; if( x == 1 ) REJECT; SCORE = x * 10 + y; }\n", [], 30, True),
    "++ and --": (HP + "\t{ i = LEN % 3; n = 0; if( i++ ) n = n + 1; j = 2; while( j-- ) n = n + 100; if( n == 200 ) REJECT; SCORE = n + i + j; }\n", [], 30, True),
    "int op float": (HP + "\t{ x = 7; y = 2.5; a = x * y; b = y * x; if( LEN * 0.5 > 8 ) REJECT; SCORE = b + a / 3 - x / y + 0.1 * LEN - LEN / 3.0; }\n",
                     [], 30, True),
    "&& on a float": (HP + "\t{ f = 0.5 * ( LEN % 2 ); g = 0.0; if( f && LEN > 17 ) REJECT; if( g || f && LEN > 0 ) SCORE = f; else SCORE = 2.5; }\n", [], 30, True),
    "loops": (HP + "\t{ n = 0; for( i = 1; i <= NSE; i++ ){ if( i == 2 ) continue; n = n + mispairs( se( index=i ) ); if( n > 0 ) break; }\n"
                   "\t  j = 0; while( j < 3 ){ j = j + 1; if( j == 2 ) break; } if( n > 0 ) REJECT; SCORE = j * 10 + i + LEN; }\n", [], 30, True),
    "COMP POS LEN": (HP + "\t{ if( COMP == 1 && POS % 2 == 0 ) REJECT; SCORE = POS + LEN * 1000 + SLEN % 7; }\n", [], 30, True),
    "explicit left context": (CTX + "\t{ s = se( index=1 ); if( length( s ) < 3 ) REJECT; if( s < \"c\" ) REJECT;\n"
                                    "\t  SCORE = mispairs( h5( index=2 ) ) + 10 * length( s ) + 100 * loc( ctx( tag='L' ) ); }\n", ["-context"], 30, True),
}
# name -> (descriptor or file under tests/golden, words of the refusal)
REFUSED = {
    "getbest": ("test/getbest.descr", "HOLD / RELEASE"),
    "score.4": ("descr/score.4.descr", "variable 'tmpr' may be read with an earlier hit's value"),
    "trna": ("descr/trna.descr", "bits()"),
    "sprintf": ("test/sprintf.descr", "sprintf()"),
    "=~": (HP + "\t{ if( ss( tag='l' ) =~ \"^ga\" ) REJECT; }\n", "=~ and !~"),
    "bits": (HP + "\t{ SCORE = bits( h5( tag='a' ), h3( tag='a' ) ); }\n", "bits()"),
    "NAME": (HP + "\t{ if( NAME == \"e\" ) REJECT; }\n", "NAME"),
    "mismatches( string, pattern )": (HP + "\t{ SCORE = mismatches( ss( tag='l' ), \"ga\" ); }\n", "mismatches( string, pattern )"),
    # (the code generator loads the operand of a prefix ++ / -- as a value, on which the host VM fails with "type mismatch":
    # the analysis refuses the program; the postfix forms are an own descriptor above)
    "prefix ++": (HP + "\t{ i = 1; if( ++i ) REJECT; }\n", "increment of something that is not a variable"),
    "prefix --": (HP + "\t{ i = 1; while( --i ) i = 0; }\n", "increment of something that is not a variable"),
    "loose": ("parms\n\tiupac = 0;\ndescr\n\th5( minlen=4, maxlen=6 )\n\t\tss( minlen=4, maxlen=5, seq=\"^nnac\" )\n\th3\nscore\n\t{ SCORE = 1; }\n", "loose"),
}
# name -> (descriptor, the host VM's words, must some record also be accepted?)
STOPS = {
    "division by zero": (HP + "\t{ x = LEN % 3; SCORE = 10 / x; }\n", "integer division by zero.", True),
    "pos beyond the match": (HP + "\t{ s = h5( tag='a', pos=6, len=1 ); SCORE = 1; }\n", "bad pos 6, must be <= ", True),
    "type mismatch": (HP + "\t{ x = \"a\"; SCORE = x + 1; }\n", "type mismatch.", False),
    "undefined variable": (HP + "\t{ if( zz > 1 ) REJECT; SCORE = 1; }\n", "variable 'zz' is undefined.", False),
    "string +": (HP + "\t{ s = ss( tag='l' ) + \"a\"; SCORE = 1; }\n", "string + string", False),
}


def build_checker():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "hostsim", "score_check.cpp")
    units = [os.path.join(H, u + ".cpp") for u in FRONT_END]
    deps = [src] + units + [os.path.join(H, f) for f in os.listdir(H) if f.endswith(".h")] + [os.path.join(ROOT, "include", "rnamotif_amd_program.h")]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(f) for f in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + H,
                        "-o", BIN, src] + units, check=True)
    return BIN


@pytest.fixture(scope="module")
def score_checker():
    return build_checker()


def run_checker(checker, tmp, argv, entries, recs, budget=0, cwd=None):
    """score_check over these entries and records: (refusal or None, the image's sizes, [(outcome, kind, bits, words)],
    status, stdout)."""
    import rnamotif_amd as R
    tmp = str(tmp)
    ent, rec = os.path.join(tmp, "entries.bin"), os.path.join(tmp, "records.bin")
    with open(ent, "wb") as f:
        f.write(np.asarray([len(entries)] + [len(e) for e in entries], dtype=np.int32).tobytes())
        f.write(b"".join(entries))
    np.ascontiguousarray(recs, dtype=np.int32).tofile(rec)
    p = subprocess.run([checker, ent, rec, str(budget)] + list(argv), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=cwd,
                       env=dict(os.environ, EFNDATA=os.environ.get("EFNDATA", R.EFNDATA_DIR)))
    out = p.stdout.decode()
    assert p.returncode in (0, 1), p.stderr.decode()
    lines = out.split("\n")
    if lines[0].startswith("REFUSED "):
        return lines[0][8:], None, [], p.returncode, out
    assert lines[0].startswith("IMAGE "), out[:200]
    image = {k: int(v) for k, v in (w.split("=") for w in lines[0].split()[1:])}
    rows = []
    for ln in lines[1:]:
        if ln[:2] in ("A ", "R ", "S "):
            w = ln.split(" ", 3)
            rows.append((w[0], int(w[1]), int(w[2], 16), w[3] if len(w) > 3 else ""))
    return None, image, rows, p.returncode, out


def plain(name):
    return name[:-7] if name.endswith(".strict") else name


def descr_args(name, tmp=None):
    """the arguments of a golden or synthetic case"""
    path = SYNTHETIC[plain(name)] if plain(name) in SYNTHETIC else GOLDEN_CASES[plain(name)][0]
    return (pins.STRICT_ARGS if name.endswith(".strict") else []) + ["-descr", os.path.join(GOLDEN, path)]


def synthetic_entries():
    import rnamotif_amd as R
    if "syn" not in _entries:
        e = R.synthetic_records(8)
        _entries["syn"] = [e[0], e[5], e[7]]
    return _entries["syn"]


def own_args(text, tmp, name, extra=()):
    path = os.path.join(str(tmp), "".join(c if c.isalnum() else "_" for c in name) + ".descr")
    with open(path, "w") as f:
        f.write(text)
    return list(extra) + ["-descr", path]


_entries = {}


def entries_of(gbrna, limit, odd=True):
    """The first `limit` entries of the reference's test database as the readers deliver them; odd: in mixed case, with u
    for t and a few odd bytes (test_hit_windows_cpu.odd_entries), which the exact sequences of the golden cases do not survive."""
    import rnamotif_amd as R
    if (limit, odd) not in _entries:
        _entries[(limit, odd)] = [normalise(e) for e in (odd_entries(gbrna, limit=limit) if odd else [s for _, _, s in R.read_fasta(gbrna)[:limit]])]
    return _entries[(limit, odd)]


def scan_case(argv, gbrna, limit, odd=True):
    import rnamotif_amd as R
    from oracle_binding import oracle_scan
    d = R.Descriptor(argv)
    entries = entries_of(gbrna, limit, odd)
    return d, entries, oracle_scan(d, entries)


_golden = {}


def golden_result(name, checker, gbrna, tmp_factory):
    """A golden case through the checker, once for the module (and for tests/test_score_device.py)."""
    if name not in _golden:
        tmp = tmp_factory.mktemp("score_" + name.replace("+", "_"))
        argv = descr_args(name, tmp)
        if plain(name) in SYNTHETIC:
            import rnamotif_amd as R
            from oracle_binding import oracle_scan
            d, entries = R.Descriptor(argv), synthetic_entries()
            recs = oracle_scan(d, entries)
        else:
            d, entries, recs = scan_case(argv, gbrna, GOLDEN_CASES[plain(name)][1], odd=False)
        refused, image, rows, status, out = run_checker(checker, tmp, argv, entries, recs)
        _golden[name] = {"argv": argv, "d": d, "entries": entries, "recs": recs, "refused": refused, "image": image, "rows": rows,
                         "status": status, "out": out}
    return _golden[name]


def counts(rows):
    return {o: sum(1 for r in rows if r[0] == o) for o in "ARS"}


@pytest.mark.parametrize("name", ALL_GOLDEN)
def test_golden_cases(built, score_checker, gbrna, tmp_path_factory, name):
    r = golden_result(name, score_checker, gbrna, tmp_path_factory)
    assert r["refused"] is None, r["refused"]
    c = counts(r["rows"])
    print("%s: %d records, %s, image %s" % (name, len(r["recs"]), c, r["image"]))
    assert r["status"] == 0, [ln for ln in r["out"].split("\n") if ln.startswith("MISMATCH")]
    assert len(r["rows"]) == len(r["recs"]) and c["S"] == 0
    # the limits of rm_score_image.h are generous
    assert r["image"]["inst"] <= 4096 // 4 and r["image"]["stack"] <= 64 // 2 and r["image"]["vars"] <= 64 // 2


@pytest.mark.parametrize("name", ALL_GOLDEN)
def test_golden_cases_are_not_vacuous(built, score_checker, gbrna, tmp_path_factory, name):
    r = golden_result(name, score_checker, gbrna, tmp_path_factory)
    c = counts(r["rows"])
    print("%s: %d records, %s" % (name, len(r["recs"]), c))
    if GOLDEN_CASES[plain(name)][2]:
        assert c["A"] >= 1 and c["R"] >= 1, c
    elif GOLDEN_CASES[plain(name)][2] is None:
        assert c == {"A": 0, "R": 0, "S": 0}, c
    else:
        assert c["A"] >= 1 and c["R"] == 0, c


@pytest.mark.parametrize("name", ALL_SYNTHETIC)
def test_ire_over_synthetic_records(built, score_checker, gbrna, tmp_path_factory, name):
    r = golden_result(name, score_checker, gbrna, tmp_path_factory)
    c = counts(r["rows"])
    print("%s: %d records, %s" % (name, len(r["recs"]), c))
    assert r["refused"] is None and r["status"] == 0, r["out"][-300:]
    assert len(r["rows"]) == len(r["recs"]) and c["S"] == 0 and c["A"] >= 1 and c["R"] >= 1, c
    assert {x[1] for x in r["rows"] if x[0] == "A"} == {2}


def test_accept_only_cases_never_reject(built, score_checker, gbrna, tmp_path_factory):
    """score.0 assigns a string and accepts; efn.descr's threshold is never passed; ire.descr and ire.1.descr have no candidate:
    over the whole database nothing is rejected."""
    for name in sorted(n for n in ALL_GOLDEN if not GOLDEN_CASES[plain(n)][2]):
        argv = descr_args(name, None)
        d, entries, recs = scan_case(argv, gbrna, None, odd=False)
        tmp = tmp_path_factory.mktemp("score_all")
        refused, image, rows, status, out = run_checker(score_checker, tmp, argv, entries, recs)
        assert refused is None and status == 0 and counts(rows) == {"A": len(recs), "R": 0, "S": 0}
        assert len(recs) == 0 if GOLDEN_CASES[plain(name)][2] is None else len(recs) > 100


@pytest.mark.parametrize("name", sorted(OWN))
def test_own_descriptors(built, score_checker, gbrna, tmp_path, name):
    text, extra, limit, rejects = OWN[name]
    argv = own_args(text, tmp_path, name, extra)
    d, entries, recs = scan_case(argv, gbrna, limit)
    refused, image, rows, status, out = run_checker(score_checker, tmp_path, argv, entries, recs)
    assert refused is None, refused
    c = counts(rows)
    print("%s: %d records, %s, kinds %s, image %s" % (name, len(recs), c, sorted({r[1] for r in rows if r[0] == "A"}), image))
    assert status == 0, [ln for ln in out.split("\n") if ln.startswith("MISMATCH")]
    assert len(rows) == len(recs) > 0 and c["S"] == 0 and c["A"] >= 1
    assert (c["R"] >= 1) == rejects, c
    scores = {r[2] for r in rows if r[0] == "A"}
    if name not in ("paired 4-plex", "substr"):
        assert len(scores) >= 2, "one SCORE for every record"
    if name == "COMP POS LEN":
        assert set(np.unique(recs[:, 1]).tolist()) == {0, 1}
    if name == "explicit left context":
        assert d.ctx_off and (recs[:, d.ctx_off + 1] == 3).any() and (recs[:, d.ctx_off + 1] < 3).any()


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals(built, score_checker, gbrna, tmp_path, name):
    import rnamotif_amd as R
    what, words = REFUSED[name]
    argv = ["-descr", os.path.join(GOLDEN, what)] if what.endswith(".descr") else own_args(what, tmp_path, name)
    refused, _, _, status, _ = run_checker(score_checker, tmp_path, argv, [b"acgt"], np.zeros((0, 1), dtype=np.int32))
    assert status == 0 and refused is not None and words in refused, refused
    # the call itself, with the same words
    d = R.Descriptor(argv)
    assert R.ScoreProgram.reason(d) == refused
    with pytest.raises(R.RnamotifError) as e:
        R.ScoreProgram(d)
    assert words in str(e.value)
    if name == "loose":
        assert d.loose > 0


def test_a_program_that_opens(built):
    import rnamotif_amd as R
    d = R.Descriptor(["-descr", os.path.join(GOLDEN, "test", "ire.descr")])
    assert R.ScoreProgram.reason(d) is None
    p = R.ScoreProgram(d)
    p.close()
    p.close()
    # no score section at all: it opens
    assert R.ScoreProgram.reason(R.Descriptor(["-descr", os.path.join(GOLDEN, "descr", "hlx.gf.if.descr")])) is None


@pytest.mark.parametrize("name", sorted(STOPS))
def test_stops(built, score_checker, gbrna, tmp_path, name):
    text, words, accepts = STOPS[name]
    argv = own_args(text, tmp_path, name)
    d, entries, recs = scan_case(argv, gbrna, 30)
    refused, image, rows, status, out = run_checker(score_checker, tmp_path, argv, entries, recs)
    assert refused is None, refused
    c = counts(rows)
    print("%s: %d records, %s" % (name, len(recs), c))
    # (the checker holds the words of every stop to the host VM's fail(); string + stops in the rule alone)
    assert status == 0, [ln for ln in out.split("\n") if ln.startswith("MISMATCH")]
    stopped = [r for r in rows if r[0] == "S"]
    assert stopped and all(words in r[3] for r in stopped), stopped[:2]
    assert all(".descr:" in r[3] for r in stopped)
    assert (c["A"] >= 1) == accepts, c


def test_budget_stops_a_finite_loop(built, score_checker, gbrna, tmp_path):
    text = HP + "\t{ n = 0; for( i = 0; i < 3000; i++ ) n = n + i % 7; SCORE = n; }\n"
    argv = own_args(text, tmp_path, "budget")
    d, entries, recs = scan_case(argv, gbrna, 5)
    recs = recs[:8]
    _, _, rows, status, out = run_checker(score_checker, tmp_path, argv, entries, recs, budget=1000)
    assert status == 0 and rows and all(r[0] == "S" and "more than 1000 instructions" in r[3] for r in rows)
    _, _, rows, status, out = run_checker(score_checker, tmp_path, argv, entries, recs)
    assert status == 0 and all(r[0] == "A" and r[1] == 1 for r in rows)


def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "rnamotif_amd.h")).read()
    for words in ("int\trma_score_open( const rma_descr_t *d, rma_score_t **out, char *err, size_t errlen );", "void\trma_score_close( rma_score_t *sp );",
                  "int\trma_score_hits( rma_scanner_t *sc, const rma_score_t *sp, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,",
                  "csrc/rm_score_core.h", "score_budget"):
        assert words in text
