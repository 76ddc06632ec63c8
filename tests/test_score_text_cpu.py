"""CPU: the score section with text -- sprintf(), bits(), string +, a string in SCORE -- as rnamotif_amd/csrc/rm_score_core.h
states it for the host and for rma_score_text_kernel, run on the host through tests/hostsim/score_text_check.cpp:

  * the formatter alone (rm_score_fmt.h) against snprintf: a million doubles from a fixed seed, each at every precision
    from 0 to 18 under changing flags and widths, ties, subnormals, negative zero, values just under 2^63, every energy
    word; %d %i %u %o %x %X and %s under every combination -- equal inside the domain, refused outside;
  * golden programs -- descr/trna.descr, test/sprintf.descr, test/sprintf.strict.descr, descr/rs2_gaps.descr, plain and
    with the strict arguments -- over the oracle's records of the first entries of the reference's test database: for
    every record the outcome of ScoreVM::run, its kind, and the score column HitPrinter::print writes, byte for byte;
  * own descriptors, one construct each (OWN_TEXT) -- the grammar takes only element references on the left of `in`, so
    a made string reaches that operator from no descriptor: it is compared, cut and measured; stops with their words (STOPS_TEXT); refusals that stay (REFUSED_TEXT).

The entry counts of GOLDEN_TEXT were chosen by running the oracle here, over all 4067 entries (where the rule and the host
VM agree on every record: rs2_gaps 1 474 016 records, 2183 accepted; sprintf and sprintf.strict 28 972 / 139, with the strict
arguments 17 120 / 82; trna 1351 / 1351 and 184 / 184): the first count, in steps of 10, at which the case, plain and strict,
holds an accepted record -- rs2_gaps in entry 0, sprintf in entry 16, trna in entry 85 -- and, where the program calls
bits() (trna.descr alone), a call over a window with fewer than four distinct letters: the first is in entry 2824, 28 of
the 1351.  With the strict arguments none of trna.descr's 184 records in the whole database has such a window, so that
case is held to the rest; the own descriptors "bits with pos" and "bits in arithmetic" read short windows."""
import os
import subprocess

import numpy as np
import pytest

import pins
from test_score_device_cpu import FRONT_END, GOLDEN, H, HP, ROOT, counts, entries_of, own_args, scan_case

BIN = os.path.join(ROOT, "tests", "_build", "score_text_check")
TEXT, CHECKED = 2, 1

# name -> (file under tests/golden, entries of the database taken)
GOLDEN_TEXT = {
    "trna": ("descr/trna.descr", 2830),
    "sprintf": ("test/sprintf.descr", 20),
    "sprintf.strict": ("test/sprintf.strict.descr", 20),
    "rs2_gaps": ("descr/rs2_gaps.descr", 10),
}
ALL_GOLDEN_TEXT = sorted(GOLDEN_TEXT) + [n + "+strict" for n in sorted(GOLDEN_TEXT)]

# name -> (descriptor, what every accepted record's column must be like: a regular expression over the field)
OWN_TEXT = {
    "%d with flags": (HP + "\t{ SCORE = sprintf( '%+5d|%-6d|%06d|% d|%.4d|%5.3d', LEN, POS, LEN - 20, LEN, LEN, COMP ); }\n", rb"^ *[+]\d+\|\d+ *\|-?\d+\| \d+\|\d{4}\| +\d{3}$"),
    "%i %u %o %x %X": (HP + "\t{ SCORE = sprintf( '%i %u %#o %#x %08X %-#6x|', 0 - LEN, 0 - LEN, LEN, POS, POS, COMP ); }\n", rb"^-\d+ 42949672\d\d 0[0-7]+ 0x[0-9a-f]+ [0-9A-F]{8} (0x1|0)  +\|$"),
    "%f with flags": (HP + "\t{ x = 1.0 * LEN / 7.0 - 2.5; SCORE = sprintf( '%f|%+.0f|%-9.2f|%09.4f|% .1f|%#.0f|%.18f', x, x, x, x, x, x, x ); }\n", rb"^-?\d\.\d{6}\|[+-]\d\|"),
    "%s of slices": (HP + "\t{ SCORE = sprintf( '%s|%6s|%-6s|%.2s|%5.1s', ss( tag='l' ), h5( tag='a', pos=1, len=3 ), ss( tag='t' ), h3( tag='a' ), 'xyz' ); }\n",
                     rb"^[a-z]{4,6}\| {3}[a-z]{3}\|[a-z]{2} {4}\|[a-z]{2}\|    x$"),
    "%n and %%": (HP + "\t{ i = 5; SCORE = sprintf( 'a%nb%%c%dd', i, 0, LEN ); }\n", rb"^ *ab%c\d+d$"),
    "s = a + b": (HP + "\t{ s = ss( tag='l' ) + '-' + h5( tag='a', pos=1, len=2 ); SCORE = s; }\n", rb"^ *[a-z]{4,6}-[a-z]{2}$"),
    "+=": (HP + "\t{ s = 'x'; s += ss( tag='t' ); s += s; SCORE = s; }\n", rb"^  x[a-z]{2}x[a-z]{2}$"),
    "a made string compared": (HP + "\t{ s = h5( tag='a', pos=1, len=1 ) + h3( tag='a', pos=$, len=1 ); if( s == 'gc' || s > 'ta' ) REJECT; t = sprintf( '%s', s );\n"
                                    "\t  if( t != s ) REJECT; SCORE = t; }\n", rb"^ {6}[a-z]{2}$"),
    "substr length in": (HP + "\t{ s = ss( tag='l' ) + ss( tag='t' ); u = substr( s, 2, 3 ); n = length( s ) * 10 + length( u );\n"
                              "\t  a = substr( s, 1, 1 ) + ''; b = substr( s, length( s ), 1 ) + ''; if( a == b ) REJECT;\n"
                              "\t  SCORE = sprintf( '%s %d', u, n ); }\n", rb"^ *[a-z]{3} [6-8]3$"),
    "a short string SCORE": (HP + "\t{ SCORE = substr( ss( tag='l' ), 1, 3 ) + ''; }\n", rb"^ {5}[a-z]{3}$"),
    "a long string SCORE": (HP + "\t{ SCORE = sprintf( '%s %s %s', h5( tag='a' ), ss( tag='l' ), h3( tag='a' ) ); }\n", rb"^[a-z]{4,6} [a-z]{4,6} [a-z]{4,6}$"),
    "bits with pos": (HP + "\t{ SCORE = sprintf( '%6.3f %6.3f', bits( h5( tag='a', pos=2 ), ss( tag='l', pos=3 ) ), bits( ss( tag='l', pos=1 ), h3( tag='a', pos=2 ) ) ); }\n",
                      rb"^ *-?\d\.\d{3}  *-?\d\.\d{3}$"),
    "bits in arithmetic": (HP + "\t{ b = bits( h5( tag='a' ), h3( tag='a' ) ); if( b < 1.5 ) REJECT; SCORE = b * 2 - LEN / 10.0; }\n", rb"^ *-?\d+\.\d{3}$"),
    "an int SCORE": (HP + "\t{ s = sprintf( '%d', LEN ); if( length( s ) != 2 || LEN % 3 == 0 ) REJECT; SCORE = LEN * 3; }\n", rb"^ {6}\d\d$"),
    "no SCORE": (HP + "\t{ s = 'a' + 'b'; if( s != 'ab' ) REJECT; }\n", rb"^   0\.000$"),
}
# name -> (descriptor, words of the stop, heap, stride, must some record be accepted?)
STOPS_TEXT = {
    "the heap": (HP + "\t{ s = 'ab'; while( length( s ) < 1000 ) s = s + s; SCORE = 1; }\n", "a string of 128 bytes does not fit a record's heap: 124 of its 128 bytes are in use (option score_heap).", 128, 64, False),
    "text_stride": (HP + "\t{ SCORE = sprintf( '%s %s', h5( tag='a' ), ss( tag='l' ) ); }\n", "a row of the text has room for 10 (text_stride).", 256, 10, True),
    "%c": (HP + "\t{ SCORE = sprintf( '%c', LEN ); }\n", "'c' unsupported format.", 256, 64, False),
    "%e by a variable format": (HP + "\t{ f = '%'; f += 'e'; SCORE = sprintf( f, 1.5 ); }\n", "'e' format: its digits are the host's C library's", 256, 64, False),
    "a wrong argument type": (HP + "\t{ SCORE = sprintf( '%d', 1.5 ); }\n", "'d' format requires int arg.", 256, 64, False),
    "a string for %f": (HP + "\t{ SCORE = sprintf( '%f', 'a' ); }\n", "'f' format requires float arg.", 256, 64, False),
    "an int for %s": (HP + "\t{ SCORE = sprintf( '%s', 1 ); }\n", "'s' format requires string/seq arg.", 256, 64, False),
    "a missing argument": (HP + "\t{ SCORE = sprintf( '%d %d', 1 ); }\n", "No such argument 2.", 256, 64, False),
    "a length modifier": (HP + "\t{ SCORE = sprintf( '%ld', 1 ); }\n", "'d' format with something else than flags, a width and a precision.", 256, 64, False),
    "a precision above 18": (HP + "\t{ SCORE = sprintf( '%.19f', 1.5 ); }\n", "a precision of 19, the device writes at most 18", 256, 64, False),
    "%f of an infinity": (HP + "\t{ x = 1.0; for( i = 0; i < 11; i++ ) x = x * 1.0e30; SCORE = sprintf( '%f', x ); }\n", "'f' format of a float that is not finite or not below 2^63.", 256, 64, False),
    "*": (HP + "\t{ SCORE = sprintf( '%*d', 1, 2 ); }\n", "sprintf: '*' and '$' in formats are not supported by this build.", 256, 64, False),
    "no conversion": (HP + "\t{ SCORE = sprintf( 'a%5.2', 1 ); }\n", "sprintf: bad format '%5.2'.", 256, 64, False),
    "no format": (HP + "\t{ SCORE = sprintf( LEN, 1 ); }\n", "sprintf: first argument must be a format string.", 256, 64, False),
    "a non-finite SCORE": (HP + "\t{ x = 1.0; if( LEN % 2 ) for( i = 0; i < 11; i++ ) x = x * 1.0e30; SCORE = x; }\n", "SCORE is not finite or not below 2^63", 256, 64, True),
    "bits pos": (HP + "\t{ SCORE = bits( h5( tag='a', pos=7 ), h3( tag='a' ) ); }\n", "bits: bad pos1 7, must be <= ", 256, 64, False),
    "bits order": (HP + "\t{ SCORE = bits( h3( tag='a' ), h5( tag='a' ) ); }\n", "bits: bad 2nd descr index 3, must follow 1st descr index 1.", 256, 64, False),
}
# bits() beyond L needs a descriptor whose elements may be longer than the table: L is capped at 1024
LONG = ("descr\n\th5( tag='a', minlen=4, maxlen=6 )\n\t\tss( tag='l', minlen=900, maxlen=1100 )\n\th3( tag='a' )\nscore\n"
        "\t{ SCORE = bits( h5( tag='a' ), h3( tag='a' ) ); }\n")
# name -> (descriptor or file under tests/golden, words of the refusal)
REFUSED_TEXT = {
    "getbest": ("test/getbest.descr", "HOLD / RELEASE"),
    "=~": (HP + "\t{ if( ss( tag='l' ) =~ \"^ga\" ) REJECT; }\n", "=~ and !~"),
    "NAME": (HP + "\t{ SCORE = sprintf( '%s', NAME ); }\n", "NAME"),
    "mismatches( string, pattern )": (HP + "\t{ SCORE = mismatches( ss( tag='l' ), \"ga\" ); }\n", "mismatches( string, pattern )"),
    "prefix ++": (HP + "\t{ i = 1; if( ++i ) REJECT; }\n", "increment of something that is not a variable"),
    "a constant %g": (HP + "\t{ SCORE = sprintf( '%d %8.3g', LEN, 1.5 ); }\n", "holds %g"),
    "a constant %e alone": (HP + "\t{ SCORE = sprintf( '%e' ); }\n", "holds %e"),
}


def build_text_checker():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "hostsim", "score_text_check.cpp")
    units = [os.path.join(H, u + ".cpp") for u in FRONT_END]
    deps = [src] + units + [os.path.join(H, f) for f in os.listdir(H) if f.endswith(".h")] + [os.path.join(ROOT, "include", "rnamotif_amd_program.h")]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(f) for f in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + H,
                        "-o", BIN, src] + units, check=True)
    return BIN


@pytest.fixture(scope="module")
def text_checker():
    return build_text_checker()


def run_text_checker(checker, tmp, argv, entries, recs, flags=TEXT, heap=256, stride=64, budget=0):
    """score_text_check over these entries and records: (refusal or None, the image's sizes, [(outcome, kind, bits, length,
    column, words)], status, stdout, (calls of bits(), those over fewer than four distinct letters))."""
    import rnamotif_amd as R
    tmp = str(tmp)
    ent, rec = os.path.join(tmp, "entries.bin"), os.path.join(tmp, "records.bin")
    with open(ent, "wb") as f:
        f.write(np.asarray([len(entries)] + [len(e) for e in entries], dtype=np.int32).tobytes())
        f.write(b"".join(entries))
    np.ascontiguousarray(recs, dtype=np.int32).tofile(rec)
    p = subprocess.run([checker, "run", ent, rec, str(budget), str(flags), str(heap), str(stride)] + list(argv), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, EFNDATA=os.environ.get("EFNDATA", R.EFNDATA_DIR)))
    out = p.stdout.decode()
    assert p.returncode in (0, 1), p.stderr.decode()[-2000:]
    lines = out.split("\n")
    if lines[0].startswith("REFUSED "):
        return lines[0][8:], None, [], p.returncode, out, (0, 0)
    assert lines[0].startswith("IMAGE "), out[:200]
    image = {k: int(v) for k, v in (w.split("=") for w in lines[0].split()[1:])}
    rows, bits = [], (0, 0)
    for ln in lines[1:]:
        if ln[:2] in ("A ", "R ", "S "):
            w = ln.split(" ", 5)
            rows.append((w[0], int(w[1]), int(w[2], 16), int(w[3]), b"" if w[4] == "-" else bytes.fromhex(w[4]), w[5] if len(w) > 5 else ""))
        elif ln.startswith("BITS "):
            bits = tuple(int(x) for x in ln.split()[1:])
    return None, image, rows, p.returncode, out, bits


def text_args(name):
    base = name[:-7] if name.endswith("+strict") else name
    return (pins.STRICT_ARGS if name.endswith("+strict") else []) + ["-descr", os.path.join(GOLDEN, GOLDEN_TEXT[base][0])], GOLDEN_TEXT[base][1]


_golden = {}


def golden_text_result(name, checker, gbrna, tmp_factory):
    """A golden case through the checker, once for the module (and for tests/test_score_text.py)."""
    if name not in _golden:
        tmp = tmp_factory.mktemp("score_text_" + name.replace("+", "_"))
        argv, limit = text_args(name)
        d, entries, recs = scan_case(argv, gbrna, limit, odd=False)
        refused, image, rows, status, out, bits = run_text_checker(checker, tmp, argv, entries, recs)
        _golden[name] = {"argv": argv, "d": d, "entries": entries, "recs": recs, "refused": refused, "image": image, "rows": rows, "status": status,
                         "out": out, "bits": bits}
    return _golden[name]


def test_formatter_against_snprintf(text_checker):
    p = subprocess.run([text_checker, "fmt", "20240607", "1000000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    out = p.stdout.decode()
    print(out[-1500:])
    last = dict(w.split("=") for w in out.strip().split("\n")[-1].split()[1:])
    assert p.returncode == 0 and int(last["bad"]) == 0, out[-1500:]
    # a million values at 19 precisions, less those outside the domain, which must be refused
    assert int(last["checked"]) + int(last["refused"]) >= 20 * 1000000 and int(last["checked"]) >= 17 * 1000000 and int(last["refused"]) >= 1000000


@pytest.mark.parametrize("name", ALL_GOLDEN_TEXT)
def test_golden_programs(built, text_checker, gbrna, tmp_path_factory, name):
    r = golden_text_result(name, text_checker, gbrna, tmp_path_factory)
    assert r["refused"] is None, r["refused"]
    c = counts(r["rows"])
    print("%s: %d records, %s, bits %s, image %s" % (name, len(r["recs"]), c, r["bits"], r["image"]))
    assert r["status"] == 0, [ln for ln in r["out"].split("\n") if ln.startswith("MISMATCH")]
    assert len(r["rows"]) == len(r["recs"]) and c["S"] == 0 and c["A"] >= 1
    accepted = [x for x in r["rows"] if x[0] == "A"]
    assert {x[1] for x in accepted} == {3} and all(x[3] == len(x[4]) >= 8 and x[2] == 0 for x in accepted)
    if name.startswith("trna"):
        assert r["image"]["flags"] == 1 and r["image"]["bits_L"] > 50 and r["bits"][0] == len(r["recs"]) and (r["bits"][1] >= 1 or name == "trna+strict"), r["bits"]
        assert all(len(x[4]) == 17 for x in accepted)


def test_golden_programs_are_refused_without_text(built, text_checker, gbrna, tmp_path):
    for name in sorted(GOLDEN_TEXT):
        argv, _ = text_args(name)
        refused, _, _, status, _, _ = run_text_checker(text_checker, tmp_path, argv, [b"acgt"], np.zeros((0, 1), dtype=np.int32), flags=0)
        assert status == 0 and refused is not None and ("sprintf()" in refused or "bits()" in refused), refused


@pytest.mark.parametrize("name", sorted(OWN_TEXT))
def test_own_descriptors(built, text_checker, gbrna, tmp_path, name):
    import re
    text, column = OWN_TEXT[name]
    argv = own_args(text, tmp_path, name)
    d, entries, recs = scan_case(argv, gbrna, 30)
    refused, image, rows, status, out, bits = run_text_checker(text_checker, tmp_path, argv, entries, recs)
    assert refused is None, refused
    c = counts(rows)
    accepted = [r for r in rows if r[0] == "A"]
    print("%s: %d records, %s, kinds %s, bits %s, e.g. %r" % (name, len(recs), c, sorted({r[1] for r in accepted}), bits, accepted[0][4] if accepted else None))
    assert status == 0, [ln for ln in out.split("\n") if ln.startswith("MISMATCH")]
    assert len(rows) == len(recs) > 0 and c["S"] == 0 and c["A"] >= 1
    assert all(re.match(column, r[4], re.S) and r[3] == len(r[4]) >= 8 for r in accepted), [r[4] for r in accepted if not re.match(column, r[4], re.S)][:3]
    assert len({r[4] for r in accepted}) >= (1 if name == "no SCORE" else 2), "one column for every record"
    kind = {"bits in arithmetic": 2, "an int SCORE": 1, "no SCORE": 0}.get(name, 3)
    assert {r[1] for r in accepted} == {kind}
    if name in ("a made string compared", "substr length in", "bits in arithmetic", "an int SCORE"):
        assert c["R"] >= 1, c
    if name.startswith("bits"):
        assert bits[0] >= len(recs) and bits[1] >= 1, bits
    if name == "%s of slices":
        assert set(np.unique(recs[:, 1]).tolist()) == {0, 1} and len({r[4] for k, r in enumerate(rows) if r[0] == "A" and recs[k, 1] == 1}) >= 2
    if name == "a short string SCORE":
        assert all(len(r[4]) == 8 for r in accepted)
    if name == "a long string SCORE":
        assert all(len(r[4]) > 8 for r in accepted)
    # without a row the same programs deliver numbers, and stop on a string
    _, _, rows0, status0, _, _ = run_text_checker(text_checker, tmp_path, argv, entries, recs, stride=0)
    assert status0 == 0 and len(rows0) == len(rows)
    for a, b in zip(rows, rows0):
        if a[0] == "A" and a[1] == 3:
            assert b[0] == "S" and "SCORE holds a string" in b[5]
        else:
            assert b[:3] == a[:3] and b[3] == 0


@pytest.mark.parametrize("name", sorted(STOPS_TEXT))
def test_stops(built, text_checker, gbrna, tmp_path, name):
    text, words, heap, stride, accepts = STOPS_TEXT[name]
    argv = own_args(text, tmp_path, name)
    d, entries, recs = scan_case(argv, gbrna, 30)
    refused, image, rows, status, out, _ = run_text_checker(text_checker, tmp_path, argv, entries, recs, heap=heap, stride=stride)
    assert refused is None, refused
    c = counts(rows)
    print("%s: %d records, %s" % (name, len(recs), c))
    assert status == 0, [ln for ln in out.split("\n") if ln.startswith("MISMATCH")]
    stopped = [r for r in rows if r[0] == "S"]
    assert stopped and all(words in r[5] for r in stopped), stopped[:2]
    # (the ACCEPT at MAIN's end, where the column is written, has no line of the descriptor's)
    assert all(".descr:" in r[5] for r in stopped) or name in ("text_stride", "a non-finite SCORE")
    assert (c["A"] >= 1) == accepts, c


def test_bits_beyond_the_table(built, text_checker, tmp_path):
    """windows of more bases than a table that ends at 1024 has rows for: the stop names both"""
    import re
    rng = np.random.default_rng(5)
    loop = bytes(rng.choice(np.frombuffer(b"acgt", dtype=np.uint8), 1100))
    entries = [b"ggcatc" + loop[:950] + b"gatgcc" + b"a" * 10, b"ttggcatc" + loop + b"gatgccaa"]
    argv = own_args(LONG, tmp_path, "long")
    import rnamotif_amd as R
    from oracle_binding import oracle_scan
    recs = oracle_scan(R.Descriptor(argv), entries)
    refused, image, rows, status, out, bits = run_text_checker(text_checker, tmp_path, argv, entries, recs)
    assert refused is None and status == 0 and image["bits_L"] == 1024 and image["table"] == 1024 * 1025 // 2
    c = counts(rows)
    print(len(recs), c, rows[-1][5])
    assert c["A"] >= 1 and c["S"] >= 1 and c["R"] == 0
    assert all(re.search(r"bits\(\) over 1\d\d\d bases, the table of its logarithms ends at 1024\.$", r[5]) for r in rows if r[0] == "S")


@pytest.mark.parametrize("name", sorted(REFUSED_TEXT))
def test_refusals_that_stay(built, text_checker, tmp_path, name):
    import rnamotif_amd as R
    what, words = REFUSED_TEXT[name]
    argv = ["-descr", os.path.join(GOLDEN, what)] if what.endswith(".descr") else own_args(what, tmp_path, name)
    for flags in (TEXT, TEXT | CHECKED):
        refused, _, _, status, _, _ = run_text_checker(text_checker, tmp_path, argv, [b"acgt"], np.zeros((0, 1), dtype=np.int32), flags=flags)
        assert status == 0 and refused is not None and words in refused, refused
    d = R.Descriptor(argv)
    assert R.ScoreProgram.reason(d, False, True) == refused == R.ScoreProgram.reason(d, checked=True, text=True)
    with pytest.raises(R.RnamotifError) as e:
        R.ScoreProgram(d, text=True)
    assert words in str(e.value)


def test_programs_that_open_with_text(built):
    import rnamotif_amd as R
    d = R.Descriptor(["-descr", os.path.join(GOLDEN, "descr", "trna.descr")])
    assert "bits()" in R.ScoreProgram.reason(d) and R.ScoreProgram.reason(d, text=True) is None
    p = R.ScoreProgram(d, text=True)
    assert p.text and not p.checked and p.info()["instructions"] > 0
    p.close()
    # a program without text opens with the flag as well, and a loose one needs checked with it as without
    assert R.ScoreProgram.reason(R.Descriptor(["-descr", os.path.join(GOLDEN, "test", "ire.descr")]), text=True) is None
    err = __import__("ctypes").create_string_buffer(512)
    h = __import__("ctypes").c_void_p()
    assert R.lib().rma_score_open_flags(d._h, 4, __import__("ctypes").byref(h), err, 512) != 0 and b"flags" in err.value and not h.value


def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "rnamotif_amd.h")).read()
    for words in ("#define RMA_SCORE_CHECKED 1u", "#define RMA_SCORE_TEXT    2u",
                  "int\trma_score_open_flags( const rma_descr_t *d, unsigned flags, rma_score_t **out, char *err, size_t errlen );",
                  "int\trma_score_hits_text( rma_scanner_t *sc, const rma_score_t *sp, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits,",
                  "score_heap"):
        assert words in text
