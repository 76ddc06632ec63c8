"""CPU: the per-base structure of hit records -- element and pair mates of every base of a record's window -- as
rnamotif_amd/csrc/rm_hitstruct.h states it for the host and for the fill kernel of rm_hitstruct_dev.hip, run on the
host through tests/hostsim/hit_structures_check.cpp over the oracle's records of the reference's test database:

  * duplex descriptors against the reference's own tool: the records printed by the host replay and piped through
    rm2ct; the .ct partner of every base of every printed hit is mate[:, 0] + 1, its letter is base, and elem
    follows the fields of the hit's line;
  * parallel, triple and quad helices, which rm2ct cannot judge, against the matcher's geometry restated here, and
    against the pair sets of the program blob: with mispair=0, pairfrac=1 and both ends paired every matched pair,
    triple or quad is a member of its element's set;
  * on every case: mates symmetric, inside the window, in the same helix; context bases numbered n_elems, n_elems+1;
  * the record check against a statement of it in Python, unequal strand lengths and sums past 2^31 included.

The entries are odd_entries() of test_hit_windows_cpu.py: the database with raw bytes mixed in."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pins
from test_hit_windows_cpu import _span_py, _write_entries, normalise, odd_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "tests", "_build", "hit_structures_check")
HDR = 5
BACKWARDS = ("h3", "t2", "q2", "q4")
TYPES = ["ctx", "ss", "h5", "h3", "p5", "p3", "t1", "t2", "t3", "q1", "q2", "q3", "q4", "se"]      # enum rma_type

# variants with every position of a helix paired: no mispairs, both ends paired; pairfrac= may not stand beside mispair=,
# so it is left at its default, which the test reads back from the program as 1
ALL_PAIRED = {
    "phlx.gf.if": "descr\n\tp5( minlen=3, maxlen=7, mispair=0, ends='pp' )\n\t\tss( minlen=4, maxlen=7 )\n\tp3\n",
    "trip": "descr\n\tt1( tag=\"1\", minlen=4, maxlen=7, mispair=0, ends='pp' )\n\t\tss( minlen=3, maxlen=10 )\n"
            "\tt2( tag=\"1\" )\n\t\tss( minlen=3, maxlen=10 )\n\tt3( tag=\"1\" )\n",
    "quad": "descr\n\tq1( tag=\"1\", minlen=3, maxlen=5, mispair=0, ends='pp' )\n\t\tss( minlen=4, maxlen=10 )\n"
            "\tq2( tag=\"1\" )\n\t\tss( minlen=4, maxlen=10 )\n\tq3( tag=\"1\" )\n\t\tss( minlen=4, maxlen=10 )\n\tq4( tag=\"1\" )\n",
    # (qu+tr.descr itself with mispair=0 has no candidate in the whole database: 4-plexes from 2 bases, triplexes from 3,
    # loops from 3 and 1 have two)
    "qu+tr": "descr\n\tq1( tag=\"1\", minlen=2, maxlen=5, mispair=0, ends='pp' )\n\t\tss( minlen=3, maxlen=10 )\n"
             "\tq2( tag=\"1\" )\n\t\tss( minlen=3, maxlen=10 )\n\tq3( tag=\"1\" )\n\t\tss( minlen=3, maxlen=10 )\n\tq4( tag=\"1\" )\n"
             "\tss( minlen=1, maxlen=10 )\n"
             "\tt1( tag=\"2\", minlen=3, maxlen=7, mispair=0, ends='pp' )\n\t\tss( minlen=3, maxlen=10 )\n"
             "\tt2( tag=\"2\" )\n\t\tss( minlen=3, maxlen=10 )\n\tt3( tag=\"2\" )\n",
}


# ---- include/rnamotif_amd_program.h, mirrored: what the tests read of the blob behind Descriptor.program
class _Atom(C.Structure):
    _fields_ = [("mask", C.c_uint8), ("lo", C.c_uint8), ("hi", C.c_uint8), ("kind", C.c_uint8)]


class _Regex(C.Structure):
    _fields_ = [("anchored", C.c_int32), ("dollar", C.c_int32), ("n_atoms", C.c_int32), ("fixed_len", C.c_int32),
                ("loose", C.c_int32), ("atoms", _Atom * 128)]


class _Pairset(C.Structure):
    _fields_ = [("n_bases", C.c_int32), ("mat2", C.c_uint32), ("mat3", C.c_uint32 * 4), ("mat4", C.c_uint32 * 20)]


class _Elem(C.Structure):
    _fields_ = [("type", C.c_int32), ("proper", C.c_int32), ("ends", C.c_int32), ("strict", C.c_int32), ("index", C.c_int32),
                ("searchno", C.c_int32), ("next", C.c_int32), ("prev", C.c_int32), ("inner", C.c_int32), ("outer", C.c_int32),
                ("n_mates", C.c_int32), ("mates", C.c_int32 * 3), ("n_scopes", C.c_int32), ("scope", C.c_int32),
                ("scopes", C.c_int32 * 8), ("minlen", C.c_int32), ("maxlen", C.c_int32), ("minglen", C.c_int32),
                ("maxglen", C.c_int32), ("minilen", C.c_int32), ("maxilen", C.c_int32), ("mismatch", C.c_int32),
                ("mispair", C.c_int32), ("pairfrac", C.c_double), ("pairset", C.c_int32), ("re", C.c_int32)]


class _SitePos(C.Structure):
    _fields_ = [("elem", C.c_int32), ("l2r", C.c_int32), ("offset", C.c_int32)]


class _Site(C.Structure):
    _fields_ = [("n_pos", C.c_int32), ("pos", _SitePos * 4), ("pairset", C.c_int32)]


class _EfnSite(C.Structure):
    _fields_ = [("idx", C.c_int32), ("pos", C.c_int32), ("idx2", C.c_int32), ("pos2", C.c_int32), ("kind", C.c_int32)]


class Program(C.Structure):
    _fields_ = [("magic", C.c_uint32), ("size", C.c_uint32), ("n_elems", C.c_int32), ("n_searches", C.c_int32),
                ("searches", C.c_int32 * 100), ("dminlen", C.c_int32), ("dmaxlen", C.c_int32), ("windowsize", C.c_int32),
                ("strict_helices", C.c_int32), ("chk_both_strs", C.c_int32), ("has_lctx", C.c_int32), ("has_rctx", C.c_int32),
                ("lctx", _Elem), ("rctx", _Elem), ("elems", _Elem * 100), ("n_sites", C.c_int32), ("sites", _Site * 16),
                ("n_pairsets", C.c_int32), ("pairsets", _Pairset * 118), ("n_regexes", C.c_int32), ("regexes", _Regex * 102),
                ("n_efn_sites", C.c_int32), ("efn_sites", _EfnSite * 16), ("efn_usestdbp", C.c_int32), ("efn_stdbp", C.c_int32)]


def program_of(d):
    """The program blob of a compiled descriptor (valid while d lives)."""
    p = Program.from_address(d.program)
    assert p.magic == 0x524d4131 and p.size == C.sizeof(Program)
    return p


def helices(p):
    """per element: (its helix's elements in descriptor order, its place among them) or None"""
    out = []
    for e in range(p.n_elems):
        el = p.elems[e]
        if TYPES[el.type] in ("ss", "ctx") or el.n_mates == 0:
            out.append(None)
            continue
        strands = sorted([e] + [el.mates[m] for m in range(el.n_mates)])
        out.append((strands, strands.index(e)))
    return out


@pytest.fixture(scope="module")
def checker():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "hostsim", "hit_structures_check.cpp")
    deps = [src, os.path.join(H, "rm_hitstruct.h"), os.path.join(H, "rm_hitwin.h"), os.path.join(ROOT, "include", "rnamotif_amd_program.h")]
    if not os.path.exists(BIN) or os.path.getmtime(BIN) < max(os.path.getmtime(f) for f in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + H, "-o", BIN, src], check=True)
    return BIN


def _inputs(tmp, d, entries, records, declared=None):
    prog, ent, rec = (os.path.join(tmp, f) for f in ("program.bin", "entries.bin", "records.bin"))
    with open(prog, "wb") as f:
        f.write(C.string_at(d.program, C.sizeof(Program)))
    if declared is None:
        _write_entries(ent, entries)
    else:
        with open(ent, "wb") as f:
            f.write(np.asarray([len(declared)] + list(declared), dtype=np.int32).tobytes())
    np.ascontiguousarray(records, dtype=np.int32).tofile(rec)
    return prog, ent, rec


def host_structures(checker, tmp, d, entries, records):
    """The rule on the host: dict of off int64 [n+1], lo int32 [n], base uint8 [T], elem int16 [T], mate int32 [T, 3]."""
    prog, ent, rec = _inputs(tmp, d, entries, records)
    out = os.path.join(tmp, "structures.bin")
    p = subprocess.run([checker, "fill", prog, ent, rec, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()
    raw = open(out, "rb").read()
    n = int(np.frombuffer(raw, dtype=np.int64, count=1)[0])
    assert n == len(records)
    at = 8
    off = np.frombuffer(raw, dtype=np.int64, count=n + 1, offset=at)
    at += 8 * (n + 1)
    lo = np.frombuffer(raw, dtype=np.int32, count=n, offset=at)
    at += 4 * n
    t = int(off[-1])
    base = np.frombuffer(raw, dtype=np.uint8, count=t, offset=at)
    at += t
    elem = np.frombuffer(raw, dtype=np.int16, count=t, offset=at)
    at += 2 * t
    mate = np.frombuffer(raw, dtype=np.int32, count=3 * t, offset=at).reshape(t, 3)
    assert at + 12 * t == len(raw)
    return {"off": off, "lo": lo, "base": base, "elem": elem, "mate": mate}


def restated(p, w, lo, length):
    """elem and mate of one record's window, written out here from the matcher's geometry"""
    ne, hx = p.n_elems, helices(p)
    ext = [(int(w[HDR + 4 * e]), int(w[HDR + 4 * e + 1])) for e in range(ne)]
    ctx = HDR + 4 * ne
    if p.has_lctx:
        ext.append((int(w[ctx]), int(w[ctx + 1])))
    else:
        ext.append((0, 0))
    ext.append((int(w[ctx + 2]), int(w[ctx + 3])) if p.has_rctx else (0, 0))
    elem = np.full(length, -1, dtype=np.int64)
    mate = np.full((length, 3), -1, dtype=np.int64)
    for i in range(length):
        pos = lo + i
        for e, (o, n) in enumerate(ext):
            if n > 0 and o <= pos < o + n:
                elem[i] = e
                break
        e = int(elem[i])
        if e < 0 or e >= ne or hx[e] is None:
            continue
        strands, me = hx[e]
        o, n = ext[e]
        k = pos - o
        # the index along the strand's direction: h3, t2, q2, q4 are read from their 3' end
        j = n - 1 - k if TYPES[p.elems[e].type] in BACKWARDS else k
        others = [s for s in strands if s != e]
        for c, s in enumerate(others):
            so = ext[s][0]
            mate[i, c] = so + (n - 1 - j if TYPES[p.elems[s].type] in BACKWARDS else j) - lo
    return elem, mate


def check_properties(p, recs, st):
    """what holds for every case: lo and the window's length by the span rule, mates symmetric, inside the window,
    in the same helix; contexts numbered behind the elements"""
    ne, hx = p.n_elems, helices(p)
    for h, w in enumerate(recs):
        a, b = int(st["off"][h]), int(st["off"][h + 1])
        elem, mate = st["elem"][a:b].astype(np.int64), st["mate"][a:b].astype(np.int64)
        want_elem, want_mate = restated(p, w, int(st["lo"][h]), b - a)
        assert np.array_equal(elem, want_elem), h
        assert np.array_equal(mate, want_mate), h
        for i in range(b - a):
            e = int(elem[i])
            ms = [int(x) for x in mate[i] if x >= 0]
            if e < 0 or e >= ne or hx[e] is None:
                assert not ms
                continue
            assert len(ms) == len(hx[e][0]) - 1 and list(mate[i][:len(ms)]) == ms
            for j in ms:
                assert 0 <= j < b - a, (h, i)
                assert i in mate[j], (h, i, j)
                assert int(elem[j]) in hx[e][0] and int(elem[j]) != e, (h, i, j)


def _descr(argv, cwd=None):
    import rnamotif_amd as R
    old = os.getcwd()
    os.chdir(cwd or old)
    try:
        return R.Descriptor(argv)
    finally:
        os.chdir(old)


def _oracle_records(d, entries):
    from oracle_binding import oracle_scan
    return oracle_scan(d, [normalise(e) for e in entries])


# hlx.gu.iu.descr (h5 ss h3, no bounds but the window's) has 3.3 million candidates in 300 entries: a dozen entries give
# thousands, every shape of the other two descriptors' helices among them
DUPLEX = [("trna.descr", 300), ("pk1.descr", 300), ("hlx.gu.iu.descr", 12)]


@pytest.mark.parametrize("name,limit", DUPLEX, ids=[n for n, _ in DUPLEX])
def test_duplex_against_rm2ct(built, checker, gbrna, tmp_path, name, limit):
    import rnamotif_amd as R
    d = _descr(["-descr", os.path.join(GOLDEN, "descr", name)])
    p = program_of(d)
    assert not p.has_lctx and not p.has_rctx
    entries = odd_entries(gbrna, limit=limit)
    recs = _oracle_records(d, entries)
    if name.startswith("hlx"):
        recs = recs[::max(1, recs.shape[0] // 4000)]      # (evenly over both strands and all entries)
    assert recs.shape[0] > 0
    st = host_structures(checker, str(tmp_path), d, entries, recs)
    check_properties(p, recs[:200], st)
    # the records printed by the host replay
    out = str(tmp_path / "hits.out")
    rp = R.Replay(d, out)
    n_printed = rp.batch([b"e%d" % i for i in range(len(entries))], [b""] * len(entries), [normalise(e) for e in entries], recs)
    rp.close()
    assert n_printed > 0
    tools = [os.path.join(ROOT, "rnamotif_amd", "bin", "rm2ct")]
    ref = os.path.join(ROOT, "oracle", "_ref", "rm2ct")
    if os.path.exists(ref):
        tools.append(ref)
    cts = [subprocess.run([t, out], stdout=subprocess.PIPE, check=True, timeout=600).stdout for t in tools]
    assert all(c == cts[0] for c in cts)
    ct = cts[0].decode().splitlines()
    hit_lines = [ln for ln in open(out).read().splitlines() if ln and ln[0] not in "#>"]
    assert len(hit_lines) == n_printed
    # every printed hit, in order: its record is the next one with these element lengths on this entry and strand
    ne = d.n_elems
    lens_of = recs[:, HDR + 1:HDR + 4 * ne:4]
    at, row, compared = 0, 0, 0
    for ln in hit_lines:
        f = ln.split()
        fields = f[-ne:]
        entry, comp = int(f[0][1:]), int(f[-ne - 3])
        lens = [0 if x == "." else len(x) for x in fields]
        while not (recs[at, 0] == entry and recs[at, 1] == comp and list(lens_of[at]) == lens):
            at += 1             # (an IndexError here: a printed hit without a record)
        a, b = int(st["off"][at]), int(st["off"][at + 1])
        nb = int(ct[row].split()[0])
        assert nb == b - a == sum(lens)
        body = [x.split() for x in ct[row + 1:row + 1 + nb]]
        assert [int(x[0]) for x in body] == list(range(1, nb + 1))
        assert "".join(x[1] for x in body) == st["base"][a:b].tobytes().decode() == "".join(x for x in fields if x != ".")
        assert [int(x[4]) for x in body] == [int(m) + 1 for m in st["mate"][a:b, 0]], ln
        assert (st["mate"][a:b, 1:] == -1).all()
        assert list(st["elem"][a:b]) == [e for e, n in enumerate(lens) for _ in range(n)]
        row += 1 + nb
        at += 1
        compared += 1
    assert row == len(ct) and compared == n_printed


def _tuple_ok(ps, codes):
    ix = 0
    for c in codes:
        ix = ix * 5 + c
    if len(codes) == 2:
        return (ps.mat2 >> ix) & 1
    mat = ps.mat3 if len(codes) == 3 else ps.mat4
    return (mat[ix >> 5] >> (ix & 31)) & 1


# trip.descr and qu+tr.descr have no candidate in the first thousand entries: they take the whole database
MULTI = [("phlx.gf.if", 300), ("trip", None), ("quad", 300), ("qu+tr", None)]


@pytest.mark.parametrize("name,limit", MULTI, ids=[n for n, _ in MULTI])
def test_parallel_triple_quad(built, checker, gbrna, tmp_path, name, limit):
    entries = odd_entries(gbrna, limit=limit)
    # the descriptor as the reference ships it: the restatement and the properties
    d = _descr(["-descr", os.path.join(GOLDEN, "descr", name + ".descr")])
    p = program_of(d)
    recs = _oracle_records(d, entries)
    assert recs.shape[0] > 0, name
    recs = recs[::max(1, recs.shape[0] // 300)]
    st = host_structures(checker, str(tmp_path), d, entries, recs)
    check_properties(p, recs, st)
    kinds = {TYPES[p.elems[e].type] for e in set(int(x) for x in st["elem"]) if e >= 0}
    assert kinds >= {"phlx.gf.if": {"p5", "p3"}, "trip": {"t1", "t2", "t3"}, "quad": {"q1", "q2", "q3", "q4"},
                     "qu+tr": {"q1", "q2", "q3", "q4", "t1", "t2", "t3"}}[name]
    # every position paired: each matched tuple is in the element's pair set
    path = tmp_path / (name + ".paired.descr")
    path.write_text(ALL_PAIRED[name])
    d2 = _descr(["-descr", str(path)])
    p2 = program_of(d2)
    for e in range(p2.n_elems):
        if helices(p2)[e] is not None:
            assert p2.elems[e].mispair <= 0 and p2.elems[e].pairfrac == 1.0 and p2.elems[e].ends == 3, e
    recs2 = _oracle_records(d2, entries)
    assert recs2.shape[0] > 0, name
    recs2 = recs2[::max(1, recs2.shape[0] // 300)]
    st2 = host_structures(checker, str(tmp_path), d2, entries, recs2)
    check_properties(p2, recs2, st2)
    code = {ord("a"): 0, ord("c"): 1, ord("g"): 2, ord("t"): 3}
    hx, tuples = helices(p2), 0
    for h in range(recs2.shape[0]):
        a, b = int(st2["off"][h]), int(st2["off"][h + 1])
        base, elem, mate = st2["base"][a:b], st2["elem"][a:b], st2["mate"][a:b]
        for i in range(b - a):
            e = int(elem[i])
            if e < 0 or e >= p2.n_elems or hx[e] is None or hx[e][1] != 0:
                continue
            strands = hx[e][0]
            # the pair set the matcher reads: the 5' strand's (match_phlx, match_triplex), for a 4-plex the second
            # strand's (match_4plex is handed q2 as its first element, oracle/rm_oracle_scan.c:1100)
            ps = p2.pairsets[p2.elems[strands[1] if len(strands) == 4 else e].pairset]
            assert ps.n_bases == len(strands)
            letters = [int(base[i])] + [int(base[int(m)]) for m in mate[i][:len(strands) - 1]]
            assert _tuple_ok(ps, [code.get(x, 4) for x in letters]), (name, h, i, bytes(letters))
            tuples += 1
    assert tuples > 0


def test_contexts(built, checker, gbrna, workdir, tmp_path):
    d = _descr(pins.STRICT_ARGS + ["-descr", "trna.strict.descr"], cwd=workdir)
    p = program_of(d)
    assert p.has_lctx and p.has_rctx
    entries = odd_entries(gbrna, limit=300)
    recs = _oracle_records(d, entries)
    assert recs.shape[0] > 0
    st = host_structures(checker, str(tmp_path), d, entries, recs)
    check_properties(p, recs, st)
    ne, ctx = d.n_elems, d.ctx_off
    seen = set()
    for h, w in enumerate(recs):
        a, b = int(st["off"][h]), int(st["off"][h + 1])
        elem = st["elem"][a:b]
        ll, rl = int(w[ctx + 1]), int(w[ctx + 3])
        assert (elem[:ll] == ne).all() and (elem[b - a - rl:] == ne + 1).all()
        assert ((elem[ll:b - a - rl] >= 0) & (elem[ll:b - a - rl] < ne)).all()
        assert (st["mate"][a:b][(elem >= ne)] == -1).all()
        seen |= {int(x) for x in elem}
    assert {ne, ne + 1} <= seen


def check_py(w, p, n_elems, ctx_off, slen):
    """hitstruct_check restated: (code, which)"""
    code, _, _, which = _span_py(w, n_elems, ctx_off, p.has_lctx, p.has_rctx, slen)
    if code:
        return (code, which)
    hx = helices(p)
    for e in range(n_elems):
        if hx[e] is None or hx[e][1] == 0:
            continue
        if int(w[HDR + 4 * e + 1]) != int(w[HDR + 4 * hx[e][0][0] + 1]):
            return (4, e)
    return (0, -1)


@pytest.mark.parametrize("name", ["trna.descr", "qu+tr.descr", "trna.strict.descr"])
def test_record_check(built, checker, workdir, tmp_path, name):
    strict = "strict" in name
    d = _descr((pins.STRICT_ARGS if strict else []) + ["-descr", name if strict else os.path.join(GOLDEN, "descr", name)], cwd=workdir)
    p = program_of(d)
    rng = np.random.default_rng(11)
    slen = [0, 1, 33, 2 ** 31 - 1, 500, 90]
    m = 6000
    recs = np.zeros((m, d.hit_stride), dtype=np.int32)
    recs[:, 0] = rng.choice([-1, 0, 1, 2, 3, 4, 5, 6, 2 ** 31 - 1], size=m, p=[.01, .02, .02, .05, .4, .3, .18, .01, .01])
    recs[:, 1] = rng.choice([0, 1, 2, -1], size=m, p=[.49, .49, .01, .01])
    # few values, so that the strands of a helix often agree; sums past 2^31 among them
    big = np.array([0, 1, 2, 5, 40, 2 ** 30, 2 ** 31 - 2, 2 ** 31 - 1, -1, -2 ** 31], dtype=np.int64)
    pw = np.array([.3, .3, .2, .1, .04, .01, .01, .02, .01, .01])
    for k in range(HDR, d.hit_stride):
        recs[:, k] = big[rng.choice(big.size, size=m, p=pw / pw.sum())].astype(np.int32)
    # a third of them with every helix consistent, so that records pass and single strands fail
    hx = helices(p)
    for h in range(0, m, 3):
        for e in range(d.n_elems):
            if hx[e] is not None and hx[e][1] != 0 and rng.random() < 0.97:
                recs[h, HDR + 4 * e + 1] = recs[h, HDR + 4 * hx[e][0][0] + 1]
    prog, ent, rec = _inputs(str(tmp_path), d, None, recs, declared=slen)
    q = subprocess.run([checker, "check", prog, ent, rec, "-"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert q.returncode == 0, q.stderr.decode()
    got = [tuple(map(int, line.split())) for line in q.stdout.decode().splitlines()]
    want = [check_py(w, p, d.n_elems, d.ctx_off, slen) for w in recs]
    assert got == want
    assert {g[0] for g in got} == {0, 1, 2, 3, 4}


def test_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "rnamotif_amd.h")).read()
    assert "int\trma_hit_structures_size( rma_scanner_t *sc, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits," in text
    assert "int\trma_hit_structures( rma_scanner_t *sc, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits," in text
    rule = open(os.path.join(H, "rm_hitstruct.h")).read()
    for words in ("the LOWEST", "match_wchlx", "match_phlx", "oracle/rm_oracle_scan.c:411-420", "oracle/rm_oracle_scan.c:447-457",
                  "hitwin_span"):
        assert words in rule
