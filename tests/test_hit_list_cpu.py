"""CPU: hit records as rmfmt lists them -- sorted, every field padded to its widest instance, long elements
abbreviated -- as rnamotif_amd/csrc/rm_hitlist.h states it for the host and for the kernels of rm_hitlist_dev.hip, run on
the host through tests/hostsim/hit_list_check.cpp with std::sort under rmlist_less.  The rule is held, byte for byte, to
bin/rmfmt and, where oracle/_ref/rmfmt has been built, to the reference's tool, both fed the host printer's output for
the same records under LC_ALL=C, with no flag, -l and -la:

  * per case of test_hit_print_cpu.py: most have one numeric column (mode 1), trna.efn two fields (mode 2), dot empty
    elements, trna.context contexts;
  * rows made by hand (SCENES): numeric against byte order, negatives, -0.000 beside 0.000, 1e3, integers of 25 digits
    that differ in the last one, a column that is no number, equal scores and positions with different element
    boundaries, exact duplicates, elements of 20, 21 and 100 letters in left- and right-justified columns, names with
    none, one and two '|' and one of 40 bytes; -smax one byte below and exactly at the temp bytes.
    bin/rmfmt reads scores through a double, which cannot tell the two integers of 25 digits apart, so for that scene it
    is held to the same lines in any order, and the order to the reference's tool and to sort(1) itself;
  * rmlist_less on 200 random records with heavy ties is a strict weak order and agrees with sort(1), run with the
    command rmfmt.c writes, on every adjacent pair of its output;
  * every refusal with its words, and the checker's own exit status 3 for a line that is not line_len bytes long."""
import os
import subprocess

import numpy as np
import pytest

from test_hit_print_cpu import CASES, _write_inputs, case_result, header_of, host_print, print_checker  # noqa: F401 (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "_build", "hit_list_check")
RMFMT = os.path.join(ROOT, "rnamotif_amd", "bin", "rmfmt")
REF_RMFMT = os.path.join(ROOT, "oracle", "_ref", "rmfmt")
HDR = 5
FLAGS = ([], ["-l"], ["-la"])
ENV = dict(os.environ, LC_ALL="C")

# three elements of free lengths: h5 and ss are left-justified columns, h3 a right-justified one
LONG = "descr\n\th5( minlen=1, maxlen=120 )\n\tss( minlen=0, maxlen=120 )\n\th3\n"


@pytest.fixture(scope="module")
def list_checker():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "hostsim", "hit_list_check.cpp")
    deps = [src] + [os.path.join(H, f) for f in ("rm_hitlist.h", "rm_hitprint.h", "rm_hitalign.h", "rm_hitstruct.h", "rm_hitwin.h", "rm_score_fmt.h")]
    deps.append(os.path.join(ROOT, "include", "rnamotif_amd_program.h"))
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(f) for f in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + H, "-o", BIN, src], check=True)
    return BIN


def host_list(checker, tmp, d, entries, records, sids, sdefs, text_len, text_bytes, name_mode=0, smax=0, accept=None, widths=None,
              letters=None, expect=0, what="list"):
    """The rule on the host.  list: {lines, L, perm, widths, mode, temp_bytes}; order: {mode, index, less, temp};
    with expect != 0 the words on stderr."""
    prog, ent, rec, sco = _write_inputs(tmp, d, entries, records, text_len, text_bytes)
    nam, out, acc, let = (os.path.join(str(tmp), f) for f in ("names.bin", "listed.bin", "accept.bin", "letters.bin"))
    off = np.zeros(2 * len(sids) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for pair in zip(sids, sdefs) for x in pair])
    with open(nam, "wb") as f:
        f.write(off.tobytes())
        f.write(b"".join(a + b for a, b in zip(sids, sdefs)))
    if accept is not None:
        np.ascontiguousarray(accept, dtype=np.uint8).tofile(acc)
    argv = [checker, what, prog, ent, rec, nam, sco, out, str(name_mode), str(smax), acc if accept is not None else "-",
            ",".join(str(int(w)) for w in widths) if widths is not None else "-"]
    if letters is not None:
        with open(let, "wb") as f:
            f.write(bytes(letters))
        argv.append(let)
    p = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == expect, p.stderr.decode()
    if expect:
        return p.stderr.decode()
    raw = open(out, "rb").read()
    if what == "order":
        n = int(np.frombuffer(raw, dtype=np.int64, count=1)[0])
        mode = int(np.frombuffer(raw, dtype=np.int32, count=1, offset=8)[0])
        index = np.frombuffer(raw, dtype=np.int64, count=n, offset=16)
        less = np.frombuffer(raw, dtype=np.uint8, count=n * n, offset=16 + 8 * n).reshape(n, n).astype(bool)
        temp = raw[16 + 8 * n + n * n:].splitlines(keepends=True)
        assert len(temp) == n
        return {"mode": mode, "index": index, "less": less, "temp": temp}
    m, L, temp_bytes = (int(x) for x in np.frombuffer(raw, dtype=np.int64, count=3))
    mode, n_segs = (int(x) for x in np.frombuffer(raw, dtype=np.int32, count=2, offset=24))
    w = np.frombuffer(raw, dtype=np.int32, count=n_segs, offset=32)
    perm = np.frombuffer(raw, dtype=np.int64, count=m, offset=32 + 4 * n_segs)
    lines = raw[32 + 4 * n_segs + 8 * m:]
    assert len(lines) == m * L and (m == 0 or lines[L - 1::L] == b"\n" * m)
    return {"lines": lines, "L": L, "perm": perm, "widths": w, "mode": mode, "temp_bytes": temp_bytes}


def rmfmt(tool, text, flags):
    p = subprocess.run([tool] + list(flags), input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=ENV, timeout=600)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout


def tools():
    return [RMFMT] + ([REF_RMFMT] if os.path.exists(REF_RMFMT) else [])


def head_of(text):
    """the '#RM' lines in front of the first hit"""
    return text[:text.index(b">")]


@pytest.mark.parametrize("name", sorted(CASES))
def test_listing_is_rmfmts(built, list_checker, gbrna, workdir, tmp_path_factory, name):
    r = case_result(name, gbrna, workdir, tmp_path_factory)
    modes = set()
    for nm, flags in enumerate(FLAGS):
        got = host_list(list_checker, r["tmp"], r["d"], r["entries"], r["recs"], r["sids"], r["sdefs"], r["text_len"], r["text_bytes"], name_mode=nm)
        assert len(got["perm"]) == len(r["recs"]) and sorted(got["perm"]) == list(range(len(r["recs"])))
        for tool in tools():
            assert head_of(r["text"]) + got["lines"] == rmfmt(tool, r["text"], flags), (tool, flags)
        modes.add(got["mode"])
    assert modes == ({2} if name == "trna.efn" else {1})
    if name == "dot":
        assert b" . " in got["lines"]


# ---- rows made by hand
NAMES = [b"a|b|c", b"a|b|", b"a|", b"|a", b"a", b"gi|12345|gb|X0123456.1|LOCUS_OF_40_BYTES"]
assert len(NAMES[5]) == 40
ENTRY = (b"acgtnacgtryk" * 30)[:340]


def recs_of(d, rows):
    """records of LONG: (entry, strand, first base, (h5, ss, h3 lengths))"""
    recs = np.zeros((len(rows), d.hit_stride), dtype=np.int32)
    for h, (e, comp, at, lens) in enumerate(rows):
        recs[h, 0], recs[h, 1] = e, comp
        for k, ln in enumerate(lens):
            recs[h, HDR + 4 * k], recs[h, HDR + 4 * k + 1] = at, ln
            at += ln
    return recs


def columns(cols):
    width = max(len(c) for c in cols)
    text = np.zeros((len(cols), width), dtype=np.uint8)
    for h, c in enumerate(cols):
        text[h, :len(c)] = np.frombuffer(c, dtype=np.uint8)
    return np.asarray([len(c) for c in cols], dtype=np.int32), text


def _spread(n, lens=(3, 2, 3)):
    return [(h % 6, h % 2, 3 * (h % 5), lens) for h in range(n)]


SCORES = [b"   9.500", b"  10.250", b"  -3.000", b"  -0.000", b"   0.000", b"     1e3", b"   2.000", b" -10.250", b"  -9.500", b"0.5",
          b"00.50", b".5", b"1.", b"    1E-2", b"   10.25", b"   100", b" 99.999"]
BIG = [b"1234567890123456789012345", b"1234567890123456789012346", b"1234567890123456789012344", b"-1234567890123456789012345",
       b"-1234567890123456789012346", b"999999999999999999999999", b"12345678901234567890123450"]
SPLITS = [(3, 2, 3), (4, 2, 2), (2, 2, 4), (1, 6, 1), (4, 0, 4), (3, 1, 4), (2, 4, 2), (5, 2, 1), (1, 2, 5), (4, 1, 3), (3, 3, 2), (2, 3, 3)]
LENS = [(20, 21, 2), (21, 20, 100), (100, 3, 21), (3, 100, 20), (5, 0, 5), (1, 1, 1), (100, 100, 100), (19, 22, 21)]
SCENES = {
    # numeric order, not byte order; negatives; the two zeros; 1e3 is a number and reads as 1
    "numeric": (_spread(34), SCORES * 2),
    "25 digits": (_spread(14), BIG * 2),
    "no number": (_spread(12), [b"abc", b"x1", b"9.5", b"-", b"1e", b"abc"] * 2),
    # the last resort everywhere: one score, one position, one length, another split
    "splits": ([(4, 1, 7, s) for s in SPLITS], [b"   1.000"] * len(SPLITS)),
    "duplicates": ([(4, 0, 5, (3, 2, 3)), (2, 1, 0, (3, 2, 3)), (4, 0, 5, (3, 2, 3))] * 8, [b"   7.000"] * 24),
    "long": ([(h % 6, h % 2, h, LENS[h % len(LENS)]) for h in range(16)], [b"%8.3f" % (h % 3) for h in range(16)]),
    "two fields": (_spread(12), [b"%8.3f %8.3f" % (h % 3, -h % 4) for h in range(12)]),
}
assert all(10 <= len(rows) <= 100 and len(rows) == len(cols) for rows, cols in SCENES.values())


@pytest.fixture(scope="module")
def long_descr(built, tmp_path_factory):
    import rnamotif_amd as R
    path = os.path.join(str(tmp_path_factory.mktemp("list_hand")), "long.descr")
    with open(path, "w") as f:
        f.write(LONG)
    return R.Descriptor(["-descr", path])


def scene(print_checker, tmp, d, key):
    """A scene's inputs and what the host printer's rule prints for them."""
    rows, cols = SCENES[key]
    recs = recs_of(d, rows)
    text_len, text_bytes = columns(cols)
    entries, sdefs = [ENTRY] * len(NAMES), [b"", b"a definition"] * 3
    off, data = host_print(print_checker, tmp, d, entries, recs, NAMES, sdefs, text_len, text_bytes)
    return (d, entries, recs, NAMES, sdefs, text_len, text_bytes), header_of(d) + data


def sort_1(temp, mode, k=1):
    """sort(1) on the temp lines with the command rmfmt.c:263-273 writes"""
    keys = ["-k", "2rn,2", "-k", "1,1", "-k", "3n,3", "-k", "4n,4", "-k", "5n,5"] if mode == 1 else \
        ["-k", "1,1"] + [x for f in (k + 2, k + 3, k + 4) for x in ("-k", "%dn,%d" % (f, f))]
    p = subprocess.run(["sort"] + keys, input=b"".join(temp), stdout=subprocess.PIPE, env=ENV, check=True)
    return p.stdout.splitlines(keepends=True)


@pytest.mark.parametrize("key", sorted(SCENES))
def test_rows_made_by_hand(list_checker, print_checker, long_descr, tmp_path, key):
    args, text = scene(print_checker, tmp_path, long_descr, key)
    for nm, flags in enumerate(FLAGS):
        got = host_list(list_checker, tmp_path, *args, name_mode=nm)
        assert got["mode"] == (2 if key in ("no number", "two fields") else 1)
        for tool in tools():
            want = rmfmt(tool, text, flags)
            if key == "25 digits" and tool == RMFMT:
                # (its doubles do not tell 1234567890123456789012345 from ...346: the same lines, in its own order)
                assert sorted((head_of(text) + got["lines"]).splitlines()) == sorted(want.splitlines())
                continue
            assert head_of(text) + got["lines"] == want, (tool, flags)
        # the order is sort(1)'s
        o = host_list(list_checker, tmp_path, *args, name_mode=nm, what="order")
        by_index = dict(zip((int(i) for i in o["index"]), o["temp"]))
        assert [by_index[int(h)] for h in got["perm"]] == sort_1(o["temp"], got["mode"], 2 if key == "two fields" else 1)
    perm, L = got["perm"], got["L"]
    rows = [got["lines"][i * L:(i + 1) * L] for i in range(len(perm))]
    if key == "duplicates":
        # identical lines come in the order of their indices
        for i in range(len(perm) - 1):
            assert rows[i] != rows[i + 1] or perm[i] < perm[i + 1]
        assert sum(rows[i] == rows[i + 1] for i in range(len(perm) - 1)) == 22
    if key == "splits":
        assert len(set(rows)) == len(rows) and len({r.split()[:5][-1] for r in rows}) == 1
    if key == "long":
        # (20 letters stand as they are and are the widest: 21 letters take 16 bytes, 100 take 17.)  Without the records
        # of 20: the widest instance of h5 and of h3 is an abbreviated one
        assert list(got["widths"][5:]) == [20, 20, 20] and b"...(100)..." in got["lines"] and b"...(21)..." in got["lines"]
        short = host_list(list_checker, tmp_path, args[0], args[1], args[2][[2, 4, 5, 10]], *args[3:5], args[5][[2, 4, 5, 10]], args[6][[2, 4, 5, 10]])
        assert list(short["widths"][5:]) == [17, 3, 16]
    if key == "numeric":
        first = [r.split()[1] for r in rows]
        assert first[:2] == [b"100", b"100"] and first[-1] == b"-10.250" and got["widths"][0] == len(b"X0123456.1")   # -la of these names
        whole = host_list(list_checker, tmp_path, *args)
        assert whole["widths"][0] == 40


def test_smax_is_a_greater_than(list_checker, print_checker, long_descr, tmp_path):
    args, text = scene(print_checker, tmp_path, long_descr, "numeric")
    for nm, flags in enumerate(FLAGS):
        t = host_list(list_checker, tmp_path, *args, name_mode=nm)["temp_bytes"]
        at = host_list(list_checker, tmp_path, *args, name_mode=nm, smax=t)
        below = host_list(list_checker, tmp_path, *args, name_mode=nm, smax=t - 1)
        assert at["mode"] == 1 and below["mode"] == 0 and list(below["perm"]) == list(range(len(args[2]))) and list(at["perm"]) != list(below["perm"])
        for tool in tools():
            assert head_of(text) + at["lines"] == rmfmt(tool, text, flags + ["-smax", str(t)])
            assert head_of(text) + below["lines"] == rmfmt(tool, text, flags + ["-smax", str(t - 1)])


@pytest.mark.parametrize("mode", [1, 2])
def test_order_is_a_strict_weak_order_and_sorts(list_checker, long_descr, tmp_path, mode):
    rng = np.random.default_rng(41 + mode)
    n = 200
    rows = [(int(rng.integers(3, 5)), int(rng.integers(0, 2)), int(rng.integers(0, 2)), SPLITS[int(rng.integers(0, 2))]) for _ in range(n)]
    pool = SCORES[2:5] if mode == 1 else [b"abc", b"x1", b"9.5"]
    text_len, text_bytes = columns([pool[int(rng.integers(0, len(pool)))] for _ in range(n)])
    o = host_list(list_checker, tmp_path, long_descr, [ENTRY] * 6, recs_of(long_descr, rows), NAMES, [b""] * 6, text_len, text_bytes, name_mode=1,
                  what="order")
    less, temp = o["less"], o["temp"]
    assert o["mode"] == mode and less.shape == (n, n) and len(set(temp)) < n // 2       # heavy ties
    assert not less.diagonal().any() and not (less & less.T).any()
    assert (less | less.T | np.eye(n, dtype=bool)).all()                                 # the index decides: a total order
    reach = less.astype(np.int32) @ less.astype(np.int32)
    assert not ((reach > 0) & ~less).any()                                               # transitive
    where = {}
    for i, t in enumerate(temp):
        where.setdefault(t, i)
    out = sort_1(temp, mode)
    assert sorted(out) == sorted(temp)
    for a, b in zip(out, out[1:]):
        assert a == b or less[where[a], where[b]]


def test_refusals(list_checker, long_descr, tmp_path):
    d = long_descr
    recs = recs_of(d, _spread(4))
    entries, sdefs = [ENTRY] * 6, [b""] * 6

    def refused(cols, expect=1, recs=recs, names=NAMES, **kw):
        text_len, text_bytes = columns(cols)
        return host_list(list_checker, tmp_path, d, entries, recs, names, sdefs, text_len, text_bytes, expect=expect, **kw)

    ok = [b"   1.000"] * 4
    bad = recs.copy()
    bad[1, HDR + 4 * 2:HDR + 4 * 2 + 2] = (len(ENTRY) - 1, 3)
    assert "record 1 is bad: 3 2" in refused(ok, recs=bad)
    words = refused([b"1.0", b"2.0", b"1.0 2.0", b"3"])
    assert "records 0 and 2: 1 and 2 score fields" in words and "n_sfields" in words and "does not restate" in words and "nothing listed" in words
    # (a record that is not printed does not count)
    assert refused([b"1.0", b"2.0", b"1.0 2.0", b"3"], expect=0, accept=[1, 1, 0, 1])["mode"] == 1
    words = refused([b"1.0", b"  \t ", b"1.0", b"3"])
    assert "record 1: an empty score column" in words and "sfields[ 0 ]" in words and "does not restate" in words
    assert "record 0: an empty score column" in refused([b"", b"", b"", b""])
    assert "record 2: a newline in its score column" in refused([b"1.0", b"2.0", b"1\n0", b"3"])
    many = b" ".join([b"1"] * 193)                       # 1 + 193 + 3 + 3 fields
    assert refused([many] * 4, expect=0)["mode"] == 2
    assert "record 0: a line of more than 200 fields (MAXFIELDS)" in refused([many + b" 1"] * 4)
    # the hit line: %-12s of a|b|c, a blank, the column, " 0 %7d %4d" and three fields of 3, 2 and 3 letters, a newline
    room = 50000 - (12 + 1 + len(b" 0 %7d %4d" % (1, 8)) + 4 + 3 + 4 + 1)
    assert refused([b"1" * (room - 1)] * 4, expect=0, recs=recs[:1].repeat(4, axis=0))["mode"] == 1
    assert "record 0: a hit line of 50000 bytes or more (LINE_SIZE)" in refused([b"1" * room] * 4, recs=recs[:1].repeat(4, axis=0))
    for names, nm, e in (([b"a", b"", b"c", b"d", b"e", b"f"], 0, 1), ([b"a", b"b", b"c d", b"d", b"e", b"f"], 0, 2),
                         ([b"a", b"b", b"c", b"d\te", b"e", b"f"], 2, 3), ([b"|", b"b", b"c", b"d", b"e", b"f"], 1, 0),
                         ([b"a", b"b", b"c", b"d", b"e", b"x||"], 2, 5)):
        assert "entry %d: its name is empty, trims to nothing or has a blank" % e in refused(ok, names=names, name_mode=nm)
    assert refused(ok, expect=0, names=[b"|", b"b", b"c", b"d", b"e", b"x||"])["mode"] == 1     # whole: nothing to trim
    table = bytearray(b"n" * 256)
    for c in b"abcdefghijklmnopqrstuvwxyz":
        table[c] = table[c - 32] = c
    table[ord("g")] = ord(" ")
    assert "the letters map byte 103 to a blank, a tab or a newline" in refused(ok, letters=table)
    table[ord("g")] = ord("G")
    assert b"G" in refused(ok, expect=0, letters=table)["lines"]
    # the checker holds every line to line_len: a width below the widest instance makes a longer line
    w = list(refused(ok, expect=0)["widths"])
    assert "line_len" in refused(ok, expect=3, widths=w[:5] + [w[5] - 1] + w[6:])
    assert refused(ok, expect=0, widths=[x + 1 for x in w])["L"] == sum(w) + 2 * len(w)


def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "rnamotif_amd.h")).read()
    for name in ("rma_hit_list_shape", "rma_hit_list"):
        assert "\t%s( " % name in text
    assert "RMA_LIST_WHOLE = 0, RMA_LIST_LOCUS = 1, RMA_LIST_ACC = 2" in text
    rule = open(os.path.join(H, "rm_hitlist.h")).read()
    for words in ("rmfmt.c:122-353", "rmfmt.c:188-217", "rmfmt.c:431-461", "-k 2rn,2 -k 1,1 -k 3n,3 -k 4n,4 -k 5n,5", "fcmprs", "MAXFIELDS", "LINE_SIZE"):
        assert words in rule
