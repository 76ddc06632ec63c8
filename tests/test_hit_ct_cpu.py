"""CPU: hit records as rm2ct writes them -- the connect records of `rm2ct` and `rm2ct -t rnaviz` -- as
rnamotif_amd/csrc/rm_hitct.h states them for the host and for the kernels of rm_hitct_dev.hip, run on the host through
tests/hostsim/hit_ct_check.cpp.  The test holds the rule to bin/rm2ct (pinned to the reference's by test_tools.py) and,
where `built` has made it, to the reference's own oracle/_ref/rm2ct, byte for byte, in both types:

  * per duplex case of test_hit_print_cpu.py: both tools over the host replay's file against the rule's bytes of the
    same records; qu+tr is refused with the tool's words and the tool's exit status;
  * rows made by hand, the tools fed with the rule of rm_hitprint.h's lines for the same rows: nb of 0, 1, 9, 10, 99,
    100, 999, 1000 and 10 001 (one ss of a record made by hand: the checker and the kernels take a record's lengths
    as they are, so no descriptor's maxlen caps it), strand 1 at both ends of an entry down to hn = 1, an offset of 7
    and of 10 digits, an empty element between two helices, both contexts, a tagged pseudoknot, p5/p3, a record that is
    not accepted;
  * energy columns for rnaviz: %8.3f values, "      -0", a 19-digit number, letters, blanks, an empty column; 2000
    seeded random decimals of the rule's grammar against printf( "%.3f", (float) atof( s ) ) of the C library; each
    HC_NUMBER form;
  * the checker itself refuses (exit status 3) a record whose hitct_size() is not the length of what the lines and
    hitct_byte() produce, so every row above holds that too."""
import os
import subprocess

import numpy as np
import pytest

from test_hit_print_cpu import CASES, HAND, HDR, _write_inputs, case_result, header_of, host_print, print_checker  # noqa: F401
from test_hit_structures_cpu import program_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "_build", "hit_ct_check")
TOOL = os.path.join(ROOT, "rnamotif_amd", "bin", "rm2ct")
REF_TOOL = os.path.join(ROOT, "oracle", "_ref", "rm2ct")
TYPES = ("rnamotif", "rnaviz")
HC_NEWLINE, HC_LINE, HC_NUMBER = 6, 7, 8        # rm_hitct.h: behind HP_TEXT
DUPLEX = ("trna", "trna.efn", "pk1", "score.2", "trna.context", "dot")

# descriptors of the rows made by hand
TWO = HAND + "\tss( minlen=0, maxlen=4 )\n\th5( len=3 )\n\t\tss( minlen=0, maxlen=4 )\n\th3\n"
PK = ("descr\n\th5( tag='a', len=3 )\n\tss( minlen=0, maxlen=4 )\n\th5( tag='b', len=3 )\n\tss( minlen=0, maxlen=4 )\n"
      "\th3( tag='a' )\n\tss( minlen=0, maxlen=4 )\n\th3( tag='b' )\n")
P53 = "descr\n\tp5( len=3 )\n\t\tss( minlen=3, maxlen=6 )\n\tp3\n"


@pytest.fixture(scope="module")
def ct_checker():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "hostsim", "hit_ct_check.cpp")
    deps = [src] + [os.path.join(H, f) for f in ("rm_hitct.h", "rm_hitprint.h", "rm_hitalign.h", "rm_hitstruct.h", "rm_hitwin.h", "rm_score_fmt.h")]
    deps.append(os.path.join(ROOT, "include", "rnamotif_amd_program.h"))
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(f) for f in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + H, "-o", BIN, src], check=True)
    return BIN


def host_ct(checker, tmp, d, entries, records, sids, sdefs, text_len, text_bytes, type, accept=None, expect=0, ent_file=None):
    """The rule on the host: (off int64 [n+1], the bytes); with expect=1 the words of the refusal.  Arguments as
    test_hit_print_cpu.host_print takes them; ent_file: an entries file that is there already."""
    prog, ent, rec, sco = _write_inputs(tmp, d, entries, records, text_len, text_bytes)
    nam, out, acc = (os.path.join(str(tmp), f) for f in ("names.bin", "ct.bin", "accept.bin"))
    off = np.zeros(2 * len(sids) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for pair in zip(sids, sdefs) for x in pair])
    with open(nam, "wb") as f:
        f.write(off.tobytes())
        f.write(b"".join(a + b for a, b in zip(sids, sdefs)))
    argv = [checker, "ct", type, " ".join(d.names()), prog, ent_file or ent, rec, nam, sco, out]
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


def tools():
    return [TOOL] + ([REF_TOOL] if os.path.exists(REF_TOOL) else [])


def rm2ct(tool, type, text):
    """(exit status, stdout, stderr) of the tool over rnamotif's output `text`"""
    p = subprocess.run([tool] + (["-t", "rnaviz"] if type == "rnaviz" else []), input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600, env=dict(os.environ, LC_ALL="C"))
    return p.returncode, p.stdout, p.stderr


@pytest.mark.parametrize("type", TYPES)
@pytest.mark.parametrize("name", DUPLEX)
def test_records_are_the_tools(built, ct_checker, gbrna, workdir, tmp_path_factory, name, type):
    r = case_result(name, gbrna, workdir, tmp_path_factory)
    off, data = host_ct(ct_checker, r["tmp"], r["d"], r["entries"], r["recs"], r["sids"], r["sdefs"], r["text_len"], r["text_bytes"], type)
    assert len(r["recs"]) >= 1 and len(data) > 0
    for tool in tools():
        rc, out, _ = rm2ct(tool, type, r["text"])
        assert rc == 0 and out == data, tool
    # a record's bytes are its header line and a line per base
    for h in (0, len(r["recs"]) - 1):
        lines = data[off[h]:off[h + 1]].split(b"\n")
        assert lines[-1] == b"" and int(lines[0].split()[0]) == len(lines) - 2
    if name == "trna.context":
        assert b"   -1 " in data
    if name == "trna.efn" and type == "rnaviz":
        assert len({ln.split()[3] for ln in data.split(b"\n") if b" dG = " in ln}) > 10


def test_triple_and_quad_are_refused(built, ct_checker, gbrna, workdir, tmp_path_factory):
    r = case_result("qu+tr", gbrna, workdir, tmp_path_factory)
    for type in TYPES:
        words = host_ct(ct_checker, r["tmp"], r["d"], r["entries"], r["recs"], r["sids"], r["sdefs"], r["text_len"], r["text_bytes"], type, expect=1)
        for tool in tools():
            rc, out, err = rm2ct(tool, type, r["text"])
            # (the reference's tool puts a time stamp and its source line in front of the words)
            assert rc == 1 and out == b"" and (err.decode() == words if tool == TOOL else words[len("rm2ct: "):].rstrip() in err.decode())
    assert words.startswith("rm2ct: can't make CT file for ") and words.endswith(" helices.\n")


def _rows(d, p, rows):
    """records by hand: (entry, strand, offset of the first element, lengths of the elements[, left context, right context])"""
    recs = np.zeros((len(rows), d.hit_stride), dtype=np.int32)
    for h, (e, comp, at, lens, *ctx) in enumerate(rows):
        recs[h, 0], recs[h, 1] = e, comp
        assert len(lens) == d.n_elems
        o = at
        for k, ln in enumerate(lens):
            recs[h, HDR + 4 * k], recs[h, HDR + 4 * k + 1] = o, ln
            o += ln
        if ctx:
            recs[h, d.ctx_off:d.ctx_off + 4] = (at - ctx[0], ctx[0], o, ctx[1])
    return recs


def _descr_of(tmp, name, text, argv=()):
    import rnamotif_amd as R
    path = os.path.join(str(tmp), name + ".descr")
    with open(path, "w") as f:
        f.write(text)
    return R.Descriptor(list(argv) + ["-descr", path])


def columns(cols, width=None):
    """score columns from their bytes: (text_len int32 [n], text_bytes uint8 [n, W])"""
    width = width or max([len(c) for c in cols] + [1])
    text = np.zeros((len(cols), width), dtype=np.uint8)
    for h, c in enumerate(cols):
        text[h, :len(c)] = np.frombuffer(c, dtype=np.uint8)
    return np.asarray([len(c) for c in cols], dtype=np.int32), text


ENTRIES = [b"acgtnacgtryk" * 4, b"ggggaaaacccc" * 3, b"acgt" * 2_600_000]
SIDS = [b"a", b"thirteen_byte", b"big"]
SDEFS = [b"", b"a definition, with blanks", b"ten million bases and more"]
NB = (0, 1, 9, 10, 99, 100, 999, 1000, 10_001)


def hand_sets(tmp):
    """name -> (descriptor, records, score columns): the rows the module's docstring lists"""
    m, s0 = len(ENTRIES[2]), len(ENTRIES[0])
    sets = {}
    d = _descr_of(tmp, "hand", HAND)
    rows = [(2, k % 2, 1000 * k, (min(nb // 3, 3), nb - 2 * min(nb // 3, 3), min(nb // 3, 3))) for k, nb in enumerate(NB)]
    assert [sum(r[3]) for r in rows] == list(NB)
    # strand 1 at both ends of an entry: at the 5' end of the strand hn counts down from slen, at the 3' end to 1; strand
    # 0 likewise; an offset of 7 digits (8 with strand 0 near the end)
    rows += [(0, 1, 0, (3, 4, 3)), (0, 1, s0 - 8, (3, 2, 3)), (0, 0, 0, (3, 2, 3)), (0, 0, s0 - 6, (3, 0, 3)),
             (2, 0, 1_234_560, (3, 4, 3)), (2, 1, m - 1_234_567, (3, 4, 3)), (1, 0, 5, (3, 1, 3)), (1, 1, 7, (3, 3, 3))]
    sets["hand"] = (d, _rows(d, program_of(d), rows), [b"   0.000"] * len(rows))
    d = _descr_of(tmp, "two", TWO)
    rows = [(0, 0, 2, (3, 2, 3, 0, 3, 4, 3)), (1, 1, 1, (3, 0, 3, 0, 3, 0, 3)), (0, 1, 4, (3, 4, 3, 2, 3, 1, 3))]
    sets["two"] = (d, _rows(d, program_of(d), rows), [b"   1.500", b"  -2.250", b"   0.000"])
    d = _descr_of(tmp, "ctx", HAND, ["-context", "-Dctx_maxlen=5"])
    p = program_of(d)
    assert p.has_lctx and p.has_rctx and d.names()[0] == "ctx" and d.names()[-1] == "ctx"
    rows = [(0, 0, 5, (3, 2, 3), 5, 5), (0, 1, 3, (3, 4, 3), 3, 0), (1, 0, 0, (3, 1, 3), 0, 4), (1, 1, 2, (3, 0, 3), 2, 5)]
    sets["ctx"] = (d, _rows(d, p, rows), [b"   0.000"] * len(rows))
    d = _descr_of(tmp, "pk", PK)
    assert [x[:2] for x in d.names()] == ["h5", "ss", "h5", "ss", "h3", "ss", "h3"] and "tag='a'" in d.names()[0]
    rows = [(0, 0, 1, (3, 2, 3, 4, 3, 1, 3)), (1, 1, 0, (3, 0, 3, 0, 3, 0, 3))]
    sets["pk"] = (d, _rows(d, program_of(d), rows), [b"  -7.125", b"   3.000"])
    d = _descr_of(tmp, "p53", P53)
    assert [x[:2] for x in d.names()] == ["p5", "ss", "p3"]
    rows = [(0, 0, 2, (3, 4, 3)), (1, 1, 3, (3, 6, 3))]
    sets["p53"] = (d, _rows(d, program_of(d), rows), [b"   0.000"] * 2)
    # energy columns: what atof() makes of the text behind the name
    d = sets["hand"][0]
    cols = [b"  -12.345", b"   0.0005", b"      -0", b"1234567890123456789", b"0.1234567890123456789", b"abcdefgh", b"        ", b"",
            b"  +3.25 x", b"-.5", b"7.", b"-", b"0x", b" \t 16777217"]
    rows = [(k % 2, k % 2, 3 + k, (3, k % 5, 3)) for k in range(len(cols))]
    sets["energy"] = (d, _rows(d, program_of(d), rows), cols)
    return sets


@pytest.fixture(scope="module")
def hand_ct(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ct_hand")
    return tmp, hand_sets(tmp)


@pytest.mark.parametrize("type", TYPES)
@pytest.mark.parametrize("key", ["hand", "two", "ctx", "pk", "p53", "energy"])
def test_rows_made_by_hand(built, ct_checker, print_checker, hand_ct, key, type):
    tmp, sets = hand_ct
    d, recs, cols = sets[key]
    text_len, text_bytes = columns(cols)
    args = (tmp, d, ENTRIES, recs, SIDS, SDEFS, text_len, text_bytes)
    _, printed = host_print(print_checker, *args)
    off, data = host_ct(ct_checker, *args, type)
    for tool in tools():
        rc, out, _ = rm2ct(tool, type, header_of(d) + printed)
        assert rc == 0 and out == data, tool
    recs_ct = [data[off[h]:off[h + 1]].split(b"\n")[:-1] for h in range(len(recs))]
    first = 3 if type == "rnaviz" else 0            # the words in front of the name
    if key == "hand":
        assert [int(r[0].split()[0]) for r in recs_ct[:len(NB)]] == list(NB) and [len(r) - 1 for r in recs_ct[:len(NB)]] == list(NB)
        assert recs_ct[0] == [(b"    0 dG = 0.000 \"big 0 1 0\"" if type == "rnaviz" else b"   0 big 0 1 0")]
        assert recs_ct[8][-1].split()[0] == b"10001" and recs_ct[8][-1].split()[3] == b"0"
        s0, m = len(ENTRIES[0]), len(ENTRIES[2])
        hn = [[int(ln.split()[-1]) for ln in r[1:]] for r in recs_ct]
        assert hn[9][0] == s0 and hn[10][-1] == 1 and hn[11][0] == 1 and hn[12][-1] == s0
        assert hn[13][0] == 1_234_561 and hn[14][0] == 1_234_567 and len(b"%d" % hn[13][0]) == 7
        # the helix: h5[ k ] with h3[ len - 1 - k ], numbered from 1
        assert [int(ln.split()[4]) for ln in recs_ct[9][1:]] == [10, 9, 8, 0, 0, 0, 0, 3, 2, 1]
    if key == "two":
        # an empty element between two helices: no line, and the numbers run on
        assert [int(ln.split()[4]) for ln in recs_ct[1][1:]] == [6, 5, 4, 3, 2, 1, 12, 11, 10, 9, 8, 7]
    if key == "ctx":
        pn = [int(ln.split()[4]) for ln in recs_ct[0][1:]]
        assert pn[:5] == [-1] * 5 and pn[-5:] == [-1] * 5 and pn[5:8] == [13, 12, 11] and int(recs_ct[0][0].split()[0]) == 18
    if key == "pk":
        assert [int(ln.split()[4]) for ln in recs_ct[1][1:]] == [9, 8, 7, 12, 11, 10, 3, 2, 1, 6, 5, 4]
    if key == "p53":
        # p5[ k ] with p3[ k ], the partner numbered from 0 as the tool has it
        assert [int(ln.split()[4]) for ln in recs_ct[0][1:]] == [7, 8, 9, 0, 0, 0, 0, 0, 1, 2]
    if key == "energy" and type == "rnaviz":
        got = [r[0].split()[first] for r in recs_ct]
        assert got == [b"-12.345", b"0.001", b"-0.000", b"1234567939550609408.000", b"0.123", b"0.000", b"0.000", b"1.000",
                       b"3.250", b"-0.500", b"7.000", b"0.000", b"0.000", b"16777216.000"]


@pytest.mark.parametrize("type", TYPES)
def test_ten_digit_offset(built, ct_checker, print_checker, tmp_path, type):
    """An entry of more than 10^9 bases, its file sparse: only the bases the two records print are written."""
    import rnamotif_amd as R
    d = _descr_of(tmp_path, "hand", HAND)
    slen = 1_000_000_100
    ent = os.path.join(str(tmp_path), "sparse.bin")
    tail = b"acgtgcatta" * 5
    with open(ent, "wb") as f:
        f.write(np.asarray([1, slen], dtype=np.int32).tobytes())
        f.seek(8 + slen - len(tail))
        f.write(tail)
    rows = [(0, 0, slen - 20, (3, 4, 3)), (0, 1, 5, (3, 2, 3))]
    recs = _rows(d, program_of(d), rows)
    text_len, text_bytes = columns([b"   0.000"] * 2)
    prog, _, rec, sco = _write_inputs(tmp_path, d, [slen], recs, text_len, text_bytes)
    nam, out = os.path.join(str(tmp_path), "names.bin"), os.path.join(str(tmp_path), "printed.bin")
    with open(nam, "wb") as f:
        f.write(np.asarray([0, 1, 1], dtype=np.int64).tobytes() + b"x")
    subprocess.run([print_checker, "print", prog, ent, rec, nam, sco, out], check=True, timeout=600)
    raw = open(out, "rb").read()
    printed = raw[8 * 4:]
    off, data = host_ct(ct_checker, tmp_path, d, [slen], recs, [b"x"], [b""], text_len, text_bytes, type, ent_file=ent)
    for tool in tools():
        rc, got, _ = rm2ct(tool, type, header_of(d) + printed)
        assert rc == 0 and got == data, tool
    hn = [int(ln.split()[-1]) for ln in data[:off[1]].split(b"\n")[1:-1]]
    assert hn == list(range(slen - 19, slen - 9)) and len(str(hn[0])) == 10
    assert int(data[off[1]:].split(b"\n")[1].split()[-1]) == slen - 5


def test_not_accepted_is_no_bytes(built, ct_checker, hand_ct):
    tmp, sets = hand_ct
    d, recs, cols = sets["energy"]
    n = len(recs)
    text_len, text_bytes = columns(cols)
    args = (ct_checker, tmp, d, ENTRIES, recs, SIDS, SDEFS, text_len, text_bytes, "rnaviz")
    off, data = host_ct(*args)
    for mask in (np.zeros(n, dtype=bool), np.arange(n) % 3 != 1):
        o, got = host_ct(*args, accept=mask)
        assert np.array_equal(np.diff(o), np.where(mask, np.diff(off), 0))
        assert got == b"".join(data[off[h]:off[h + 1]] for h in range(n) if mask[h])
    # a record that is not printed is not read by the tool: its column may be anything
    text_len, text_bytes = columns([b"1e5"] + cols[1:])
    mask = np.arange(n) != 0
    o, got = host_ct(ct_checker, tmp, d, ENTRIES, recs, SIDS, SDEFS, text_len, text_bytes, "rnaviz", accept=mask)
    assert got == data[off[1]:]


def random_decimals(seed, count):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        nd = int(rng.integers(1, 20))
        digits = "".join(str(int(x)) for x in rng.integers(0, 10, size=nd))
        if rng.random() < .5:
            digits = str(int(rng.integers(1, 10))) + digits[1:]
        point = int(rng.integers(0, nd + 1)) if rng.random() < .8 else nd
        s = digits[:point] + ("." + digits[point:] if point < nd or rng.random() < .1 else "")
        lead = "0" * int(rng.integers(0, 3)) if rng.random() < .2 else ""
        s = " " * int(rng.integers(0, 4)) + str(rng.choice(["", "", "-", "+"])) + lead + s
        out.append(s + str(rng.choice(["", " 0 12", "x", " "])))
    return out


def test_energy_is_the_c_librarys(ct_checker):
    texts = random_decimals(31, 2000)
    # ties and neighbours of ties of the float grid, which a single rounding would get wrong or right by luck
    texts += ["16777217", "16777217.0000000001", "16777219", "0.0005", "0.00049999999999", "1.0005", "2.5005", "9007199254740993", "0.1", ".", "-", "", "9999999999999999999",
              "-9223372036854775808", "9223372036854775807", "9223371487098961920"]
    p = subprocess.run([ct_checker, "energy"], input=("\n".join(texts) + "\n").encode(), stdout=subprocess.PIPE, timeout=600)
    assert p.returncode == 0
    rows = [ln.split("\t") for ln in p.stdout.decode().splitlines()]
    assert len(rows) == len(texts)
    bad = [(t, r) for t, r in zip(texts, rows) if r[0] != r[1]]
    assert not bad, bad[:5]
    assert len({r[0] for r in rows}) > 1500 and any(r[0].startswith("-") for r in rows) and any(len(r[0]) > 20 for r in rows)


@pytest.mark.parametrize("text", ["1e5", "2.5E-3", "inf", "-Infinity", "nan", "0x1p3", "0X.8", "12345678901234567890", "0.00000000000000000001"])
def test_forms_that_are_not_restated(built, ct_checker, hand_ct, text):
    p = subprocess.run([ct_checker, "energy"], input=(text + "\n").encode(), stdout=subprocess.PIPE, timeout=600)
    assert p.stdout.decode().split("\t")[0] == "HC_NUMBER"
    tmp, sets = hand_ct
    d, recs, _ = sets["p53"]
    text_len, text_bytes = columns([b"   0.000", b"  " + text.encode()])
    args = (ct_checker, tmp, d, ENTRIES, recs, SIDS, SDEFS, text_len, text_bytes)
    assert "record 1 is bad: %d\n" % HC_NUMBER in host_ct(*args, "rnaviz", expect=1)
    host_ct(*args, "rnamotif")          # the energy is rnaviz's alone


def test_lines_the_tool_would_not_see(built, ct_checker, hand_ct):
    tmp, sets = hand_ct
    d, recs, _ = sets["p53"]
    text_len, text_bytes = columns([b"   0.000", b"  1\n2"])
    assert "record 1 is bad: %d\n" % HC_NEWLINE in host_ct(ct_checker, tmp, d, ENTRIES, recs, SIDS, SDEFS, text_len, text_bytes, "rnamotif", expect=1)
    d, _, _ = sets["hand"]
    p = program_of(d)
    # "big" + 10 blanks, the column, " 0 %7d %4d", three fields, the newline: 49 999 bytes pass, 50 000 do not
    for ss, expect in ((49_952, 0), (49_953, 1)):
        recs = _rows(d, p, [(2, 0, 10, (3, ss, 3))])
        line = 13 + 8 + len(" 0 %7d %4d" % (11, ss + 6)) + 4 + 4 + ss + 1 + 1
        assert line == (49_999 if not expect else 50_000)
        got = host_ct(ct_checker, tmp, d, ENTRIES, recs, SIDS, SDEFS, *columns([b"   0.000"]), "rnaviz", expect=expect)
        assert ("record 0 is bad: %d\n" % HC_LINE in got) if expect else (len(got[1]) > 49_952 * 20)


def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "rnamotif_amd.h")).read()
    for name in ("rma_hit_ct_size", "rma_hit_ct"):
        assert "\t%s( " % name in text
    assert "RMA_CT_RNAMOTIF = 0, RMA_CT_RNAVIZ = 1" in text
    rule = open(os.path.join(H, "rm_hitct.h")).read()
    for words in ("rm2ct.c:232-297", "rm2ct.c:432-471", "hitct_line_len", "hitct_size", "hitct_byte", "HC_NUMBER", "%5d dG = %.3f"):
        assert words in rule
