"""CPU: rmprune's rule over hit records as rnamotif_amd/csrc/rm_prune.h states it for the host and for the kernels of
rm_prune_dev.hip, run on the host through tests/hostsim/prune_check.cpp over the oracle's records of the reference's
test database:

  * the rule equals the tool: the records printed by the host replay and piped through rnamotif_amd/bin/rmprune leave
    exactly what records[keep] print -- duplex, pseudoknot, triple, quad and parallel helices, a left context (which
    shifts every element), an empty element printed as "." (which shifts those behind it), a tagged and an untagged
    spelling of one hairpin;
  * the tool's output is the reference's own tool's (md5 pins in tests/golden/prune_pins.json, data only;
    RNAMOTIF_PIN_REF=1 with oracle/_ref built records them again);
  * the equality is not vacuous: every case keeps a hit, every case that can drop drops one, and over the file the
    checker counts drops via DOWN and via LEFT;
  * runs and blocks: 999, 1000, 1001 and 2001 records of one entry, names that merge entries, strands 0,1,0,1 in one
    run, shuffled rows, duplicates, 0, 1 and 2 records;
  * the table of strand groups built from mates[] equals read_descr()'s, restated here from the '#RM descr' line,
    for every descriptor of tests/golden/descr that compiles.

A descriptor without a duplex can never be pruned: relation() judges p5, t1 and q1 by equality of all strands' spans,
so it says SAME or DIFF and never DOWN or LEFT, whatever the length ranges -- the reference's own tool keeps every hit
of phlx.gf.if, trip, quad and qu+tr over the whole database.  Those four are cases that can only keep (and are held
to keeping everything); for each kind of helix there is a sibling case with a duplex next to it that does drop
("phlx+hlx", "trip+hlx", "quad+hlx").  Every case with a duplex must drop.  trna.strict.descr is compiled with
-context but without -sh: with strict helices no hit is an unzipped version of another (none of its 136 hits in the
whole database is dropped), without them the left context shifts the elements of hits that are."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import pins
from test_hit_structures_cpu import Program, program_of
from test_hit_windows_cpu import normalise, odd_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "tests", "_build", "prune_check")
TOOL = os.path.join(ROOT, "rnamotif_amd", "bin", "rmprune")
REF_TOOL = os.path.join(ROOT, "oracle", "_ref", "rmprune")
PINS = os.path.join(GOLDEN, "prune_pins.json")
RECORD = os.environ.get("RNAMOTIF_PIN_REF") == "1"
HDR = 5

HLX = "\th5( minlen=3, maxlen=6 )\n\t\tss( minlen=3, maxlen=6 )\n\th3\n\tss( minlen=1, maxlen=3 )\n"
HAIRPIN = "descr\n\th5( %sminlen=4, maxlen=8 )\n\t\tss( minlen=3, maxlen=6 )\n\th3%s\n"
OWN = {
    "phlx+hlx": "descr\n" + HLX + "\tp5( minlen=3, maxlen=4 )\n\t\tss( minlen=4, maxlen=7 )\n\tp3\n",
    "trip+hlx": "descr\n" + HLX + "\tt1( tag=\"1\", minlen=3, maxlen=5, mispair=1 )\n\t\tss( minlen=3, maxlen=8 )\n\tt2( tag=\"1\" )\n"
                "\t\tss( minlen=3, maxlen=8 )\n\tt3( tag=\"1\" )\n",
    "quad+hlx": "descr\n" + HLX + "\tq1( tag=\"1\", minlen=2, maxlen=3, mispair=1 )\n\t\tss( minlen=3, maxlen=6 )\n\tq2( tag=\"1\" )\n"
                "\t\tss( minlen=3, maxlen=6 )\n\tq3( tag=\"1\" )\n\t\tss( minlen=3, maxlen=6 )\n\tq4( tag=\"1\" )\n",
    "dot": "descr\n\th5( minlen=3, maxlen=5 )\n\t\tss( minlen=0, maxlen=1 )\n\t\th5( minlen=3, maxlen=4 )\n"
           "\t\t\tss( minlen=4, maxlen=6 )\n\t\th3\n\t\tss( minlen=0, maxlen=1 )\n\th3\n",
    "hairpin.untagged": HAIRPIN % ("", ""),
    "hairpin.tagged": HAIRPIN % ('tag="a", ', '( tag="a" )'),
}
# name -> (entries of the database taken, has the descriptor a duplex, so that the tool can drop at all?)
# (pk1's first dropped hit is in entry 421; trip.descr and qu+tr.descr have their first candidates past the thousandth)
CASES = {"trna": (300, True), "pk1": (450, True), "trip": (None, False), "quad": (300, False), "qu+tr": (None, False),
         "phlx.gf.if": (300, False), "phlx+hlx": (60, True), "trip+hlx": (300, True), "quad+hlx": (300, True),
         "trna.context": (300, True), "dot": (60, True), "hairpin.untagged": (40, True), "hairpin.tagged": (40, True)}
CONTEXT_ARGS = ["-context", "-Dctx_maxlen=5"]


@pytest.fixture(scope="module")
def prune_checker():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    src = os.path.join(ROOT, "tests", "hostsim", "prune_check.cpp")
    deps = [src, os.path.join(H, "rm_prune.h"), os.path.join(H, "rm_hitstruct.h"), os.path.join(H, "rm_hitwin.h"),
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


def descr_of(name, workdir, tmp):
    if name in OWN:
        path = os.path.join(str(tmp), name + ".descr")
        with open(path, "w") as f:
            f.write(OWN[name])
        return _descr(["-descr", path])
    if name == "trna.context":
        return _descr(CONTEXT_ARGS + ["-descr", "trna.strict.descr"], cwd=workdir)
    return _descr(["-descr", os.path.join(GOLDEN, "descr", name + ".descr")])


def host_mask(checker, tmp, d, slens, recs, groups=None):
    """The rule on the host: (bool mask [n], {"down", "left", "blocks", "groups"})."""
    tmp = str(tmp)
    prog, ent, rec, grp = (os.path.join(tmp, f) for f in ("program.bin", "lengths.bin", "records.bin", "groups.bin"))
    with open(prog, "wb") as f:
        f.write(C.string_at(d.program, C.sizeof(Program)))
    np.asarray([len(slens)] + list(slens), dtype=np.int32).tofile(ent)
    np.ascontiguousarray(recs, dtype=np.int32).tofile(rec)
    if groups is not None:
        np.ascontiguousarray(groups, dtype=np.int32).tofile(grp)
    p = subprocess.run([checker, "mask", prog, ent, rec, grp if groups is not None else "-"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()
    mask, counts = p.stdout.decode().split("\n")[:2]
    assert len(mask) == len(recs)
    w = counts.split()
    return np.frombuffer(mask.encode(), dtype=np.uint8) == ord("1"), {w[i]: int(w[i + 1]) for i in range(0, 8, 2)}


def printed(d, entries, recs, sids, path):
    """The records through the host replay, as rnamotif prints them; every record must reach the printer."""
    import rnamotif_amd as R
    rp = R.Replay(d, str(path))
    n = rp.batch(sids, [b""] * len(entries), entries, np.ascontiguousarray(recs, dtype=np.int32))
    rp.close()
    assert n == len(recs), "the score section rejected records: printed hits and records do not correspond"
    return open(str(path), "rb").read()


def run_tool(exe, text):
    p = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=dict(os.environ, LC_ALL="C"))
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout


def split(text):
    """(the #RM lines, the hits as (definition line, hit line))"""
    lines = text.split(b"\n")
    head = [ln for ln in lines if ln.startswith(b"#RM")]
    body = [ln for ln in lines if ln and not ln.startswith(b"#")]
    assert len(body) % 2 == 0 and all(ln.startswith(b">") for ln in body[::2])
    return head, list(zip(body[::2], body[1::2]))


def sids_of(n):
    return [b"e%d" % i for i in range(n)]


def check_against_tool(checker, tmp, d, entries, recs, sids=None, groups=None):
    """The rule's mask against the tool on the printed records; returns (mask, counts, the tool's input and output)."""
    sids = sids or sids_of(len(entries))
    keep, counts = host_mask(checker, tmp, d, [len(e) for e in entries], recs, groups)
    text = printed(d, entries, recs, sids, os.path.join(str(tmp), "all.out"))
    out = run_tool(TOOL, text)
    want = printed(d, entries, recs[keep], sids, os.path.join(str(tmp), "kept.out"))
    head, hits = split(out)
    want_head, want_hits = split(want)
    assert hits == want_hits
    assert head == want_head == split(text)[0] and len(head) == (3 if len(recs) else 0)
    assert out == want
    return keep, counts, text, out


_results = {}


def case_result(name, checker, gbrna, workdir, tmp_factory):
    if name not in _results:
        tmp = tmp_factory.mktemp("prune_" + name.replace("+", "_"))
        d = descr_of(name, workdir, tmp)
        entries = [normalise(e) for e in odd_entries(gbrna, limit=CASES[name][0])]
        from oracle_binding import oracle_scan
        recs = oracle_scan(d, entries)
        keep, counts, text, out = check_against_tool(checker, tmp, d, entries, recs)
        _results[name] = {"d": d, "entries": entries, "recs": recs, "keep": keep, "counts": counts, "text": text, "out": out}
    return _results[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_rule_equals_the_tool(built, prune_checker, gbrna, workdir, tmp_path_factory, name):
    r = case_result(name, prune_checker, gbrna, workdir, tmp_path_factory)
    n, kept = len(r["recs"]), int(r["keep"].sum())
    print("%s: %d records, %d kept, %s" % (name, n, kept, r["counts"]))
    assert n > 0 and kept >= 1
    assert n - kept == r["counts"]["down"] + r["counts"]["left"]
    if name == "trna.context":
        p = program_of(r["d"])
        assert p.has_lctx and (r["recs"][:, r["d"].ctx_off + 1] > 0).any()
    if name == "dot":
        lens = r["recs"][:, HDR + 1:HDR + 4 * r["d"].n_elems:4]
        assert (lens[:, 1] == 0).any() and (lens[:, 1] == 1).any() and b" . " in r["text"]


def _pin(key, make):
    all_pins = json.load(open(PINS)) if os.path.exists(PINS) else {}
    if RECORD:
        assert os.path.exists(REF_TOOL), "RNAMOTIF_PIN_REF=1 needs oracle/_ref (oracle/Makefile, target ref)"
        all_pins[key] = make()
        with open(PINS, "w") as f:
            json.dump(all_pins, f, indent=0, sort_keys=True)
            f.write("\n")
    assert key in all_pins, "no pin %r in tests/golden/prune_pins.json (RNAMOTIF_PIN_REF=1 with oracle/_ref built records it)" % key
    return all_pins[key]


@pytest.mark.parametrize("name", sorted(CASES))
def test_tool_matches_the_references_tool(built, prune_checker, gbrna, workdir, tmp_path_factory, name):
    r = case_result(name, prune_checker, gbrna, workdir, tmp_path_factory)
    # (the '#RM dfile' line names a path of this run: the pins are of everything else)
    def body(text):
        return b"\n".join(ln for ln in text.split(b"\n") if not ln.startswith(b"#RM dfile"))
    pin = _pin("rmprune on the printed records of " + name,
               lambda: {"input": hashlib.md5(body(r["text"])).hexdigest(),
                        "stdout": hashlib.md5(body(run_tool(REF_TOOL, r["text"]))).hexdigest()})
    assert hashlib.md5(body(r["text"])).hexdigest() == pin["input"]
    assert hashlib.md5(body(r["out"])).hexdigest() == pin["stdout"]


def test_the_equality_is_not_vacuous(built, prune_checker, gbrna, workdir, tmp_path_factory):
    down = left = 0
    for name in sorted(CASES):
        r = case_result(name, prune_checker, gbrna, workdir, tmp_path_factory)
        n_in, n_out = len(split(r["text"])[1]), len(split(r["out"])[1])
        print("%-18s the tool keeps %d of %d; %s" % (name, n_out, n_in, r["counts"]))
        assert n_out >= 1, name
        duplex = b" h5" in split(r["text"])[0][1]
        assert duplex == CASES[name][1], name
        if duplex:
            assert n_out < n_in, name
        else:
            assert n_out == n_in, name      # (nothing to judge by but equality: the module's text)
        down += r["counts"]["down"]
        left += r["counts"]["left"]
    assert down >= 1 and left >= 1, (down, left)


@pytest.fixture(scope="module")
def trna2(built, gbrna):
    """trna over 300 entries and their reverse complements: records on both strands"""
    d = _descr(["-descr", os.path.join(GOLDEN, "descr", "trna.descr")])
    seqs = [normalise(e) for e in odd_entries(gbrna, limit=300)]
    rc = [bytes(b if b in b"acgt" else ord("n") for b in s[::-1].translate(bytes.maketrans(b"acgt", b"tgca"))) for s in seqs]
    entries = seqs + rc
    from oracle_binding import oracle_scan
    recs = oracle_scan(d, entries)
    assert (recs[:, 1] == 0).sum() > 8 and (recs[:, 1] == 1).sum() > 8
    return d, entries, recs


def related_pair(checker, tmp, d, entries, recs):
    """(a, b, x): two neighbouring records of one entry and strand of which the rule drops one when they are alone, and
    a third of that entry and strand that is related to neither"""
    idx = [i for i in range(len(recs) - 1) if recs[i, 0] == recs[i + 1, 0] and recs[i, 1] == recs[i + 1, 1]][:400]
    pairs = np.concatenate([recs[[i, i + 1]] for i in idx]).copy()
    pairs[:, 0] = np.repeat(np.arange(len(idx)), 2)             # every pair an entry, hence a run, of its own
    slens = [len(entries[int(recs[i, 0])]) for i in idx]
    keep, _ = host_mask(checker, tmp, d, slens, pairs)
    slens = [len(e) for e in entries]
    for k in (k for k in range(len(idx)) if not keep[2 * k:2 * k + 2].all()):
        a, b = recs[idx[k]], recs[idx[k] + 1]
        for x in recs[(recs[:, 0] == a[0]) & (recs[:, 1] == a[1])]:
            if (host_mask(checker, tmp, d, slens, np.stack([b, x, x]))[0].all() and host_mask(checker, tmp, d, slens, np.stack([x, x, a]))[0].all()
                    and host_mask(checker, tmp, d, slens, np.stack([x, a, b, x]))[0].sum() == 3):
                return a, b, x
    raise AssertionError("no entry with a related pair and an unrelated third record")


def test_blocks_and_runs(prune_checker, trna2, tmp_path):
    d, entries, recs = trna2
    a, b, x = related_pair(prune_checker, tmp_path, d, entries, recs)
    alone, c, _, _ = check_against_tool(prune_checker, tmp_path, d, entries, np.stack([x, a, b]))
    assert alone.tolist().count(False) == 1 and alone[0] and c["blocks"] == 1
    for n in (999, 1000, 1001, 2001):
        # a and b the last two of the first thousand / the thousandth and the one after it / ...
        for at in sorted({n - 2, 998, 999} & set(range(n - 1))):
            run = np.stack([x] * at + [a, b] + [x] * (n - at - 2))
            keep, c, _, _ = check_against_tool(prune_checker, tmp_path, d, entries, run)
            assert c["blocks"] == (n + 999) // 1000, (n, at)
            apart = (at + 1) % 1000 == 0          # a the last record of a block, b the first of the next
            if apart:
                assert keep[at] and keep[at + 1], "records %d and %d saw each other" % (at + 1, at + 2)
            else:
                assert not (keep[at] and keep[at + 1]), (n, at)
            assert keep.sum() == n - (not apart)
    # shuffled rows, duplicates, 0, 1 and 2 records
    rng = np.random.default_rng(3)
    for what, rows in (("shuffled", recs[rng.permutation(len(recs))][:700]), ("duplicates", np.stack([x] * 4 + [a] * 3)),
                       ("none", recs[:0]), ("one", recs[3:4]), ("two", np.stack([a, b])), ("all", recs)):
        keep, c, _, _ = check_against_tool(prune_checker, tmp_path, d, entries, rows)
        if what == "duplicates":
            assert keep.all() and c["down"] == c["left"] == 0
        if what == "two":
            assert keep.sum() == 1
        if what == "none":
            assert keep.size == 0 and c["blocks"] == 0


def test_names_merge_entries_into_a_run(prune_checker, trna2, tmp_path):
    import rnamotif_amd as R
    d, entries, recs = trna2
    half = len(entries) // 2
    assert R.prune_groups([b"x.1", b"x.2", b"y"]).tolist() == [0, 0, 1] and R.prune_groups([b"x.1", b"x.2", b"y"]).dtype == np.int32
    assert R.prune_groups(["  a b", "a.7", "ab", b"\ta", ""]).tolist() == [0, 0, 1, 0, 2]
    # an entry with hits on strand 0 whose reverse complement (entry + half) has them on strand 1
    e = next(int(e) for e in np.unique(recs[recs[:, 1] == 0, 0]) if e < half and ((recs[:, 0] == e + half) & (recs[:, 1] == 1)).sum() > 1
             and ((recs[:, 0] == e) & (recs[:, 1] == 0)).sum() > 1)
    s0 = recs[(recs[:, 0] == e) & (recs[:, 1] == 0)]
    s1 = recs[(recs[:, 0] == e + half) & (recs[:, 1] == 1)]
    other = next(int(o) for o in np.unique(recs[:, 0]) if o not in (e, e + half))
    rows = np.concatenate([s0, s1, s0, s1, recs[recs[:, 0] == other]])          # strands 0,1,0,1 in one run, then y
    sids = sids_of(len(entries))
    sids[e], sids[e + half], sids[other] = b"x.1", b"x.2", b"y"
    groups = R.prune_groups(sids)
    assert groups[e] == groups[e + half] != groups[other]
    merged, c, _, _ = check_against_tool(prune_checker, tmp_path, d, entries, rows, sids=sids, groups=groups)
    assert c["blocks"] == 2
    # the names kept apart, the same rows are four runs and one: the first_comp quirk shows in the difference
    apart, c2 = host_mask(prune_checker, tmp_path, d, [len(x) for x in entries], rows)
    assert c2["blocks"] == 5
    print("merged keeps %d, apart %d of %d" % (merged.sum(), apart.sum(), len(rows)))


def _read_descr(words):
    """read_descr() of the tool, from the words of the '#RM descr' line behind '#RM descr': per field (kind, group)"""
    names = ["ctx", "ss", "h5", "h3", "p5", "p3", "t1", "t2", "t3", "q1", "q2", "q3", "q4"]
    n = len(words)
    kind = [next((k for k, nm in enumerate(names) if nm[:2] == w[:2]), -1) for w in words]
    group = [[] for _ in range(n)]
    tag = [w[w.index("("):] if "(" in w else None for w in words]
    for d in range(n):
        if kind[d] == 1 or tag[d] is None or group[d]:
            continue
        g = [d] + [d1 for d1 in range(d + 1, n) if tag[d1] == tag[d]]
        g = g[:4]
        for m in g:
            group[m] = g
    stk = []
    for d in range(n):
        if kind[d] == 1 or group[d]:
            continue
        if kind[d] in (2, 4):
            stk.append(d)
        elif stk:
            d5 = stk.pop()
            group[d5] = group[d] = [d5, d]
    return [(kind[d], group[d]) for d in range(n)]


def test_table_equals_read_descr(built, prune_checker, workdir, tmp_path):
    import rnamotif_amd as R
    cases = []
    folder = os.path.join(GOLDEN, "descr")
    for name in sorted(f for f in os.listdir(folder) if f.endswith(".descr")):
        try:
            _descr(["-descr", name], cwd=folder)
        except R.RnamotifError:
            continue
        # the descriptor without its score section, which could reject the made-up record below: the same elements
        text = open(os.path.join(folder, name)).read().split("\n")
        cut = next((i for i, ln in enumerate(text) if ln.strip() == "score"), len(text))
        with open(str(tmp_path / name), "w") as f:
            f.write("\n".join(text[:cut]) + "\n")
        cases.append((name, _descr(["-descr", str(tmp_path / name)], cwd=folder)))
    cases.append(("trna.context", descr_of("trna.context", workdir, tmp_path)))
    for name in sorted(OWN):
        cases.append((name, descr_of(name, workdir, tmp_path)))
    assert len(cases) >= 60
    kinds = set()
    for name, d in cases:
        out = str(tmp_path / "header.out")
        rp = R.Replay(d, out)
        # (the header comes with the first hit: a made-up record of 8 bases an element will do)
        w = np.zeros((1, d.hit_stride), dtype=np.int32)
        w[0, HDR:HDR + 4 * d.n_elems:4] = 8 + 8 * np.arange(d.n_elems)
        w[0, HDR + 1:HDR + 4 * d.n_elems:4] = 8
        w[0, d.ctx_off:d.ctx_off + 4] = [0, 8, 8 + 8 * d.n_elems, 8]
        rp.batch([b"e0"], [b""], [b"acgtgcat" * (d.n_elems + 2)], w)
        rp.close()
        line = next(ln for ln in open(out).read().splitlines() if ln.startswith("#RM descr"))
        want = _read_descr(line.split()[2:])
        prog = str(tmp_path / "program.bin")
        with open(prog, "wb") as f:
            f.write(C.string_at(d.program, C.sizeof(Program)))
        p = subprocess.run([prune_checker, "table", prog], stdout=subprocess.PIPE, check=True)
        got = [(int(ln.split()[0]), [int(x) for x in ln.split()[1:]]) for ln in p.stdout.decode().splitlines()]
        # an element the tool cannot name (kind -1) does not occur; ss and contexts have no group
        assert got == want, name
        kinds |= {k for k, _ in got}
    assert kinds >= set(range(13))


def test_header_declares_the_call():
    text = open(os.path.join(ROOT, "include", "rnamotif_amd.h")).read()
    assert "int\trma_prune_hits( rma_scanner_t *sc, const rma_db_t *db, const int32_t *d_hits, int64_t n_hits," in text
    assert "csrc/rm_prune.h" in text
    rule = open(os.path.join(H, "rm_prune.h")).read()
    for words in ("WHERE THE LENGTH IS 0", "rmprune.cpp:150-209", "hitwin_span", "first record with", "PRUNE_BLOCK = 1000"):
        assert words in rule
