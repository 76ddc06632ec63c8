"""The oracle (oracle/rm_oracle_scan.c) and the HIP scanner held to the reference's own matcher on the generated
descriptors the kernels are tested on.  find_motif.c, regexp.c and mm_regexp.c compile as they lie behind a driver
of this repository's own (oracle/ref_find_motif_drv.c -> oracle/_ref/find_motif_drv, built by oracle/Makefile
where the reference's sources are): it sets the reference's globals from the program blob
(tests/hostsim/program_dump.cpp writes it, with the seq= strings the C ABI does not expose), and its RM_score()
prints every candidate the reference finds, in the reference's call order:

    entry strand  {matchoff matchlen n_mispairs n_mismatches} per element  lctx off len  rctx off len

That listing's md5 and line count are pinned in tests/golden/ref_pins.json (tests/ref_pins.py; key = options,
md5 of the descriptor text, md5 of the sequences, so a changed generator is a missing pin), and the tests run
from the pins: RNAMOTIF_PIN_REF=1 with oracle/_ref built records them again.

CPU: the same listing made of oracle_scan()'s records equals the pin, and R.sort_hits() leaves those records as
they were emitted, order word 0, 1, ... (the oracle's order word is already its emission counter within (entry,
strand, start, rank), so this holds start and rank to the reference's call order).  GPU: the listing made of
Scanner.scan()'s records -- sorted on the device by (entry, strand, start, rank, order), DESIGN.md section 1 -- equals
the pin: kernel and sort against the reference's call order with nothing of this repository in between.

Cases: the generators and entry builders of tests/test_gpu_parity.py (imported) with the seeds of its tests (nested
1000+0..159, general 5000+0..39 plain and -sh -context, drain 7000+0..39, the stress entries: empty, shorter than
minlen, of maxlen + 1), its 4-plex / long seq= / long-helix descriptors, four of the reference's own descriptors
over its test database, and 300 + 300 fresh seeds.  A case is left out (skipped, with the reason) only where the
descriptor does not compile, its window exceeds the bound of the GPU test of the same generator, or the
reference's candidate count exceeds that test's cap.  -sh cases run the reference with fm_window[] first filled
with UNDEF (the pin) and with zeros (find_motif.c:129 never initialises it); "zfill_same" in the pin says whether
the two listings were equal.

Recorded: 977 cases listed, 887 pinned (the other 90 do not compile or exceed the window bound), 617 of them with
candidates, 7 above the cap; fresh ranges: 600 seeds, 63 left out (57 do not compile, 6 above the cap), 537
compared, 374 with candidates.  No mismatch between the reference and the oracle.  3 of the 153 -sh cases differ
under the two fills (FILL_DEPENDENT below).
GPU leg: 145 cases, each one scan of at most 90 000 bases (the test database: 4067 entries, 2.3 Mbases).  No time of its
own on the MI355X is recorded for it; the limit per test, 120 s, is taken from the GPU suite's recorded time
(GPUTEST_r04.json: some 650 tests of this size in 262 s), generously.
"""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import rnamotif_amd as R
from oracle_binding import oracle_scan
from ref_pins import RECORD, md5, pinned
from test_gpu_parity import (Q1_VARIANTS, WIDE_DESCRS, _drain_entries, _long_seq_case, _nested_sequence, _planted_sequence, _q1_case,
                             _random_descriptor, _random_general_descriptor, _stress_entries, _wide_sequences)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
REF = os.path.join(ROOT, "oracle", "_ref", "find_motif_drv")
DUMP = os.path.join(ROOT, "tests", "_build", "program_dump")
GOLDEN = os.path.join(ROOT, "tests", "golden")
STRICT = ["-sh", "-context", "-Dctx_maxlen=4"]
LONG_SEQ = ["anchored", "floating", "mismatch", "helix", "ranges"]
GBRNA = {"trna.descr": [], "pk1.descr": [], "qu+tr.descr": [], "mp.ends.strict.descr": ["-sh", "-context", "-Dctx_maxlen=5"]}
N_FRESH = 300


def build_program_dump():
    """tests/_build/program_dump, built where it is missing or older than its sources"""
    srcs = [os.path.join(ROOT, "tests", "hostsim", "program_dump.cpp")] + [os.path.join(H, f + ".cpp") for f in (
        "rm_regex", "rm_compile", "rm_parse", "rm_score", "rm_efndata", "rm_efn2data", "rm_fasta", "rm_driver", "rm_cli",
        "rm_dump", "rm_pack", "rm_stream")]
    if not os.path.exists(DUMP) or os.path.getmtime(DUMP) < max(os.path.getmtime(s) for s in srcs):
        os.makedirs(os.path.dirname(DUMP), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + H, "-o", DUMP] + srcs, check=True)
    return DUMP


@pytest.fixture(scope="module")
def program_dump(built):
    """needed only where pins are recorded"""
    return build_program_dump() if RECORD else None


# ---------------------------------------------------------------------------------------------- the cases
def _gbrna_sequences():
    import gzip
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "gbrna.111.0.fastn")
        with gzip.open(os.path.join(GOLDEN, "test", "gbrna.111.0.fastn.gz"), "rb") as f, open(path, "wb") as g:
            g.write(f.read())
        return [r[2] for r in R.read_fasta(path)]


def _compile(tmp, text, extra):
    path = os.path.join(str(tmp), "case.descr")
    with open(path, "w") as f:
        f.write(text)
    try:
        return R.Descriptor(list(extra) + ["-descr", path])
    except R.RnamotifError:
        return None


class Case:
    """kind and seed -> options, descriptor text, compiled descriptor (None: does not compile), a function that gives
    the entries, and the window bound and candidate cap of the GPU test the case is taken from (None: it has none)"""

    def __init__(self, kind, seed, tmp):
        self.kind, self.seed, self.extra, self.bound, self.cap = kind, seed, [], None, None
        rng = None
        if kind in ("nested", "drain", "stress-lean", "fresh-nested"):
            rng = np.random.default_rng({"nested": 1000, "drain": 7000, "stress-lean": 1000, "fresh-nested": 30000}[kind] + seed)
            self.text = _random_descriptor(rng)
        elif kind in ("general", "general-sh", "stress-general", "fresh-general"):
            rng = np.random.default_rng((20000 if kind == "fresh-general" else 5000) + seed)
            self.text = _random_general_descriptor(rng)
            if kind == "general-sh" or (kind == "fresh-general" and seed % 2):
                self.extra = STRICT
        elif kind == "q1":
            self.text, seqs = _q1_case(seed)
        elif kind == "long-seq":
            self.text, seqs = _long_seq_case(LONG_SEQ[seed])
        elif kind == "wide":
            self.text = WIDE_DESCRS[seed][0]
        elif kind == "gbrna":
            name = sorted(GBRNA)[seed]
            self.text = open(os.path.join(GOLDEN, "test", name)).read()
            self.extra = GBRNA[name]
        else:
            raise ValueError(kind)
        self.d = d = _compile(tmp, self.text, self.extra)
        if kind == "nested":
            self.bound, self.cap = 600, 400_000
            self.entries = lambda: (lambda s: [s, s[:257]])(_nested_sequence(rng))
        elif kind in ("general", "general-sh"):
            self.bound, self.cap = 160, 300_000
            self.entries = lambda: (lambda s: [s, s[:301]])(_planted_sequence(rng, 6_000))
        elif kind == "drain":
            self.bound, self.cap = 200, 300_000
            self.entries = lambda: _drain_entries(_planted_sequence(rng, 20_000), d, rng)
        elif kind in ("stress-lean", "stress-general"):
            self.bound, self.cap = 160, 300_000
            self.entries = lambda: _stress_entries(_planted_sequence(rng, 5_000), d)
        elif kind in ("fresh-nested", "fresh-general"):
            self.bound, self.cap = (600, 400_000) if kind == "fresh-nested" else (160, 300_000)
            self.entries = lambda: (lambda s: [s, s[:301]])(_planted_sequence(rng, int(rng.integers(6_000, 20_001))))
        elif kind in ("q1", "long-seq"):
            self.entries = lambda: seqs
        elif kind == "wide":
            self.entries = _wide_sequences
        elif kind == "gbrna":
            self.entries = _gbrna_sequences

    def left_out(self):
        """why the case is left out before its pin is looked at, or None"""
        if self.d is None:
            return "does not compile"
        if self.bound is not None and self.d.maxlen > self.bound:
            return "window exceeds the bound of the GPU test of this generator"
        assert not self.d.loose, "a loose seq= among the cases: its records are a superset by design (tests/test_loose_seq.py)"
        return None


def _listing(recs, n_elems):
    """(md5, lines) of the canonical listing of hit records"""
    cols = np.concatenate([recs[:, :2], recs[:, 5:5 + 4 * n_elems + 4]], axis=1)
    h = hashlib.md5()
    for a in range(0, cols.shape[0], 20_000):
        h.update(("\n".join(" ".join(map(str, r)) for r in cols[a:a + 20_000].tolist()) + "\n").encode())
    return h.hexdigest(), int(cols.shape[0])


def _run_ref(case, seqs, tmp):
    """the reference's listing: md5 and lines (-sh: under both fills of fm_window[])"""
    tmp = str(tmp)
    prog, db = os.path.join(tmp, "case.prog"), os.path.join(tmp, "case.seqs")
    subprocess.run([DUMP, prog] + list(case.extra) + ["-descr", os.path.join(tmp, "case.descr")], check=True, timeout=300)
    with open(db, "wb") as f:
        f.write(b"".join(s + b"\n" for s in seqs))

    def run(flags):
        p = subprocess.Popen([REF] + flags + [prog, db], stdout=subprocess.PIPE)
        h, n = hashlib.md5(), 0
        for chunk in iter(lambda: p.stdout.read(1 << 20), b""):
            h.update(chunk)
            n += chunk.count(b"\n")
        assert p.wait(timeout=3600) == 0
        return h.hexdigest(), n
    m, n = run([])
    pin = {"md5": m, "n": n}
    if "-sh" in case.extra:
        pin["zfill_same"] = run(["-z"]) == (m, n)
    return pin


def _pin(case, seqs, tmp):
    key = "find_motif_drv %s %s %s" % (" ".join(case.extra) or "-", md5(case.text.encode()), md5(b"\n".join(seqs)))
    return pinned(key, lambda: _run_ref(case, seqs, tmp))


CASES = ([("nested", s) for s in range(160)] + [("general", s) for s in range(40)] + [("general-sh", s) for s in range(40)] +
         [("drain", s) for s in range(40)] + [("stress-lean", s) for s in range(40)] + [("stress-general", s) for s in range(40)] +
         [("q1", s) for s in range(len(Q1_VARIANTS))] + [("long-seq", s) for s in range(len(LONG_SEQ))] +
         [("wide", s) for s in range(len(WIDE_DESCRS))] + [("gbrna", s) for s in range(len(GBRNA))] +
         [("fresh-nested", s) for s in range(N_FRESH)] + [("fresh-general", s) for s in range(N_FRESH)])
# the GPU leg: every tenth nested seed, every general seed in both modes, the named variants
# the -sh descriptors whose listing depends on the first contents of fm_window[]: the pin is the UNDEF fill
FILL_DEPENDENT = [("general-sh", 23), ("fresh-general", 231), ("fresh-general", 249)]
GPU_CASES = [(k, s) for k, s in CASES if k in ("general", "general-sh", "q1", "long-seq", "wide", "gbrna") or
             (k in ("nested", "fresh-nested") and s % 10 == 0) or (k, s) in FILL_DEPENDENT]


def _ids(cases):
    return ["%s-%d" % c for c in cases]


@pytest.mark.parametrize("kind,seed", CASES, ids=_ids(CASES))
def test_oracle_records_equal_reference_pins(built, program_dump, tmp_path, kind, seed):
    case = Case(kind, seed, tmp_path)
    if case.left_out():
        pytest.skip("left out: " + case.left_out())
    seqs = case.entries()
    pin = _pin(case, seqs, tmp_path)
    if case.cap is not None and pin["n"] > case.cap:
        pytest.skip("left out: the reference's %d candidates exceed the cap of the GPU test of this generator" % pin["n"])
    recs = oracle_scan(case.d, seqs)
    assert _listing(recs, case.d.n_elems) == (pin["md5"], pin["n"]), (case.extra, case.text)
    # the order the reference called RM_score() in is the order of the boundary's sort key
    assert np.array_equal(R.sort_hits(recs), recs), (case.extra, case.text)


def test_reference_descriptors_have_their_pinned_hit_counts(built, program_dump, tmp_path):
    """The instrument against what is already pinned to the reference by md5 (tests/pins.py): where the score section
    rejects nothing the driver's count is the number of hits of the reference's run.  (mp.ends.strict.descr rejects
    helices whose first pair is made: its 46 hits are among the candidates, which says little; what holds the driver
    there is its gbrna case above, listing against listing.)"""
    import pins
    seqs = _gbrna_sequences()
    for i, name in enumerate(sorted(GBRNA)):
        want = pins.STRICT[name[:-len(".strict.descr")]][0] if name.endswith(".strict.descr") else pins.SLACK[name][0]
        sub = tmp_path / str(i)
        sub.mkdir()
        case = Case("gbrna", i, sub)
        n = _pin(case, seqs, sub)["n"]
        assert (n >= want) if "REJECT" in case.text else (n == want), name


def test_a_changed_mispair_count_fails_the_comparison(built, program_dump, tmp_path):
    case = Case("q1", 0, tmp_path)
    seqs = case.entries()
    pin = _pin(case, seqs, tmp_path)
    recs = oracle_scan(case.d, seqs)
    assert recs.shape[0] > 0 and _listing(recs, case.d.n_elems) == (pin["md5"], pin["n"])
    recs[recs.shape[0] // 2, 5 + 2] += 1
    assert _listing(recs, case.d.n_elems) != (pin["md5"], pin["n"])


def test_fresh_ranges_compare_enough(built, program_dump, tmp_path):
    """At most one fresh seed in five is left out, and at least half of the compared ones have candidates -- counted
    from the pins, that is from the reference alone."""
    left, compared, with_hits, fills_differ = {}, 0, 0, []
    for kind in ("fresh-nested", "fresh-general"):
        for seed in range(N_FRESH):
            case = Case(kind, seed, tmp_path)
            why = case.left_out()
            if why is None:
                seqs = case.entries()
                pin = _pin(case, seqs, tmp_path)
                if pin["n"] > case.cap:
                    why = "candidates"
                elif not pin.get("zfill_same", True):
                    fills_differ.append((kind, seed))
            if why is not None:
                left[why] = left.get(why, 0) + 1
            else:
                compared += 1
                with_hits += pin["n"] > 0
    n_left = sum(left.values())
    print("fresh ranges: %d seeds, %d left out %r, %d compared, %d with candidates; -sh cases that differ under a zero fill: %r"
          % (2 * N_FRESH, n_left, left, compared, with_hits, fills_differ))
    assert n_left * 5 <= 2 * N_FRESH
    assert with_hits * 2 >= compared


@pytest.mark.gpu
@pytest.mark.timeout(120)
@pytest.mark.parametrize("kind,seed", GPU_CASES, ids=_ids(GPU_CASES))
def test_gpu_records_equal_reference_pins(built, tmp_path, kind, seed):
    case = Case(kind, seed, tmp_path)
    if case.left_out():
        pytest.skip("left out: " + case.left_out())
    seqs = case.entries()
    pin = _pin(case, seqs, tmp_path)
    if case.cap is not None and pin["n"] > case.cap:
        pytest.skip("left out: the reference's %d candidates exceed the cap of the GPU test of this generator" % pin["n"])
    sc = R.Scanner(case.d)          # (a descriptor the device build refuses fails here: the pins are about what it runs)
    recs = sc.scan(sc.database(seqs))
    assert _listing(recs, case.d.n_elems) == (pin["md5"], pin["n"]), (case.extra, case.text)
