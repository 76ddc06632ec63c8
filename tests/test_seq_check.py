"""GPU: the loose seq= expressions on the device (Scanner.seq_check, rma_seqcheck_hits: rma_seqcheck_kernel of
rm_seqcheck_dev.hip) against the same rule, rm_seqcheck.h, run on the host through tests/hostsim/seq_check.cpp, against
Python's `re` and against the host replay:

  * the window records of tests/test_seq_check_cpu.py (which holds the rule to re_step / re_mm_step) over a database whose
    text holds n, r, y and upper case: keep and the fixed rows equal the checker's and Python's; 37 rows are repeated
    behind them, so that the last wave is ragged whatever the count;
  * the records of a real scan, the expression inside a hairpin over tests/test_loose_seq.py's database: keep equals the
    `accepted` mask of Replay.device(..., accepted=True) -- no score section, so what is printed is the candidates;
  * rows in any order and 2^17 + 65 of them; alphabet= tokens and a letters table;
  * failed calls -- a bad record, an element past its entry's end, a record beyond a budget of 64 -- fail with their words,
    name the lowest index and leave the output tensors, prefilled with a sentinel, as they were;
  * refusals before the call; the score section behind it; a descriptor that is not loose.

torch is imported before the product library: one HIP runtime serves the process."""
import ctypes as C
import os

import torch  # noqa: F401  (first: its HIP runtime is the process's)

import numpy as np
import pytest

import rnamotif_amd as R
from test_loose_seq import _database
from test_seq_check_cpu import (BACKREF_CASES, CASES, HDR, case_of, descr_args, expected, raw_entries, reader_letters, revcomp, run_checker,  # noqa: F401
                                seq_checker, window_case, window_expectation, window_records)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ragged(seqs, lead=3):
    flat = b"x" * lead + b"".join(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64) + lead
    return torch.frombuffer(bytearray(flat), dtype=torch.uint8).to(DEV), off


def _open(d, seqs):
    sc = R.Scanner(d, device=0)
    text, off = _ragged(seqs)
    return sc, sc.database_from_tensor(text, offsets=off)


def _checked(sc, db, rows, **kw):
    r = sc.seq_check(db, rows, **kw)
    n = rows.shape[0]
    assert r.keep.dtype == torch.bool and tuple(r.keep.shape) == (n,) and r.keep.device == rows.device
    if kw.get("fixed", True):
        assert r.hits.dtype == torch.int32 and tuple(r.hits.shape) == tuple(rows.shape) and r.hits.device == rows.device
    else:
        assert r.hits is None
    torch.cuda.synchronize()
    return r.keep.cpu().numpy(), r.hits.cpu().numpy() if r.hits is not None else None


@pytest.mark.parametrize("name", CASES)
def test_kernel_against_the_rule_and_re(built, seq_checker, tmp_path_factory, name):
    w = window_case(name, seq_checker, tmp_path_factory)
    assert w["refused"] is None and w["status"] == 0
    recs = w["recs"]
    idx = np.concatenate([np.arange(len(recs)), np.arange(37)])
    rows = recs[idx]
    assert len(rows) > 256 and len(rows) % 64 != 0
    sc, db = _open(w["d"], w["raw"])
    keep, fixed = _checked(sc, db, torch.from_numpy(rows).to(DEV))
    want, rows_want = window_expectation(name, w["entries"], recs)
    rule = np.array([x[0] == "K" for x in w["rows"]])
    assert np.array_equal(keep, rule[idx]) and np.array_equal(keep, want[idx])
    assert np.array_equal(fixed, w["fixed"][idx]) and np.array_equal(fixed, rows_want[idx])
    assert keep.any() and not keep.all()
    # keep alone
    only, none = _checked(sc, db, torch.from_numpy(rows).to(DEV), fixed=False)
    assert np.array_equal(only, keep)
    info = sc._seq_check.info
    print("%s: %d records, %d kept, %s" % (name, len(rows), keep.sum(), info))
    assert info["private_bytes"] == 0 and info["expressions"] == 1
    db.close()
    sc.close()


@pytest.fixture(scope="module")
def loose_db(tmp_path_factory):
    """tests/test_loose_seq.py's database as its file holds it: every fifth entry in upper case"""
    seqs = _database(str(tmp_path_factory.mktemp("loose") / "db.fastn"))
    return [s.upper() if k % 5 == 0 else s for k, s in enumerate(seqs)], seqs


def _replayed(d, db, rows, path, letters=None):
    rp = R.Replay(d, str(path))
    n, mask = rp.device(db, rows, letters=letters, accepted=True)
    rp.close()
    lines = [ln for ln in open(str(path), "rb").read().split(b"\n") if ln and not ln.startswith(b"#") and not ln.startswith(b">")]
    assert n == int(mask.sum()) == len(lines)
    return mask, lines


@pytest.mark.parametrize("name", CASES)
def test_records_of_a_real_scan(built, loose_db, tmp_path, name):
    """(over this database every case, the three iupac = 0 ones included, keeps some records of its scan and drops some: the
    oracle's records through the checker say so -- from 1 of 295 for ^\\(\\(a\\)c\\)\\2\\1 to 659 of 2526)"""
    raw, seqs = loose_db
    d = R.Descriptor(descr_args(name, tmp_path, hairpin=True))
    assert d.loose == 1
    sc, db = _open(d, raw)
    hits = sc.scan_tensor(db)
    keep, fixed = _checked(sc, db, hits)
    mask, lines = _replayed(d, db, hits, tmp_path / "out.txt")
    assert np.array_equal(keep, mask)
    print("%s: %d records, %d candidates" % (name, len(keep), keep.sum()))
    assert keep.any() and not keep.all()
    # the element's text by Python's statement, too
    recs = hits.cpu().numpy()
    strands = [(s, revcomp(s)) for s in seqs]
    want = np.array([expected(name, strands[r[0]][r[1]][r[HDR + 4]:r[HDR + 4] + r[HDR + 5]].decode())[0] for r in recs])
    assert np.array_equal(keep, want)
    assert np.array_equal(fixed[~keep], recs[~keep]) and np.array_equal(np.delete(fixed, HDR + 7, axis=1), np.delete(recs, HDR + 7, axis=1))
    db.close()
    sc.close()


@pytest.fixture(scope="module")
def floating(built, seq_checker, tmp_path_factory):
    """\\(ac\\)g\\1 over the window records: a scanner, a database and the checker's answer"""
    w = window_case("table01", seq_checker, tmp_path_factory)
    sc, db = _open(w["d"], w["raw"])
    hits = torch.from_numpy(w["recs"]).to(DEV)
    yield {"w": w, "sc": sc, "db": db, "hits": hits, "keep": np.array([x[0] == "K" for x in w["rows"]]), "fixed": w["fixed"]}
    db.close()
    sc.close()


def _rows_equal(f, idx):
    at = torch.as_tensor(idx, dtype=torch.int64, device=DEV)
    keep, fixed = _checked(f["sc"], f["db"], f["hits"][at])
    idx = np.asarray(idx, dtype=np.int64)
    assert np.array_equal(keep, f["keep"][idx]) and np.array_equal(fixed, f["fixed"][idx])
    return keep


def test_rows_in_any_order(floating):
    n = floating["hits"].shape[0]
    rng = np.random.default_rng(11)
    _rows_equal(floating, rng.permutation(n))
    _rows_equal(floating, np.repeat(rng.permutation(n)[:300], 3))
    for k in (0, 1, 63, 64, 65):
        _rows_equal(floating, np.arange(k) + 5)


def test_more_rows_than_a_chunk(floating):
    n = floating["hits"].shape[0]
    idx = np.random.default_rng(12).integers(0, n, size=(1 << 17) + 65)
    keep = _rows_equal(floating, idx)
    assert keep[: 1 << 17].any() and keep[1 << 17:].size == 65 and len(set(idx.tolist())) < len(idx)


def test_alphabet_tokens_and_letters_table(floating, seq_checker, tmp_path):
    w = floating["w"]
    # tokens: 0-3 are acgu, anything else 4 -- the readers' n
    ent = [bytes(c if chr(c) in "acgt" else ord("n") for c in e) for e in w["entries"]]
    lut = np.full(256, 4, dtype=np.uint8)
    lut[np.frombuffer(b"acgt", dtype=np.uint8)] = np.arange(4, dtype=np.uint8)
    tokens = torch.from_numpy(lut[np.frombuffer(b"".join(ent), dtype=np.uint8)]).to(DEV)
    sc = R.Scanner(w["d"], device=0)
    db = sc.database_from_tensor(tokens, lengths=[len(s) for s in ent], alphabet="acgu")
    keep, fixed = _checked(sc, db, floating["hits"])
    want, rows_want = window_expectation("table01", ent, w["recs"])
    assert np.array_equal(keep, want) and np.array_equal(fixed, rows_want) and keep.any()
    db.close()
    sc.close()
    # the readers' letters with a and c exchanged: other strings, other records kept
    tab = bytearray(R.reader_letter(b) for b in range(256))
    for x, y in ((b"a", b"c"), (b"A", b"C"), (b"c", b"a"), (b"C", b"A")):
        tab[x[0]] = R.reader_letter(y[0])
    swapped = [e.translate(bytes.maketrans(b"ac", b"ca")) for e in w["entries"]]
    keep, fixed = _checked(floating["sc"], floating["db"], floating["hits"], letters=bytes(tab))
    want, rows_want = window_expectation("table01", swapped, w["recs"])
    # (on strand 1 the table's letter is complemented: the swapped entries' reverse complement)
    assert np.array_equal(keep, want) and np.array_equal(fixed, rows_want)
    assert not np.array_equal(keep, floating["keep"])
    with pytest.raises(R.RnamotifError, match="the letter 0"):
        floating["sc"].seq_check(floating["db"], floating["hits"], letters=bytes(256))
    with pytest.raises(ValueError, match="256 bytes"):
        floating["sc"].seq_check(floating["db"], floating["hits"], letters=b"acgt")


def _raw_call(sc, db, rows, keep, fixed, budget=0):
    err = C.create_string_buffer(4096)
    rc = R.lib().rma_seqcheck_hits(sc._h, sc._seq_check._h, db._h, rows.data_ptr(), rows.shape[0], None, budget, keep.data_ptr(),
                                   fixed if isinstance(fixed, int) else fixed.data_ptr(), torch.cuda.current_stream(DEV).cuda_stream, err, 4096)
    torch.cuda.synchronize()
    return rc, err.value.decode()


def _sentinels(rows):
    return torch.full((rows.shape[0],), 7, dtype=torch.uint8, device=DEV), torch.full(tuple(rows.shape), -9, dtype=torch.int32, device=DEV)


def _untouched(out):
    return bool((out[0] == 7).all()) and bool((out[1] == -9).all())


def test_failed_calls_write_nothing(floating, seq_checker, tmp_path):
    sc, db, hits = floating["sc"], floating["db"], floating["hits"]
    n_seq = db.n_seqs
    # an entry out of range: the replay's refusal, naming the lowest index
    bad = hits.clone()
    bad[300, 0] = n_seq + 5
    bad[17, 0] = -1
    out = _sentinels(bad)
    rc, words = _raw_call(sc, db, bad, *out)
    assert rc != 0 and words.startswith("record 17: entry -1 outside [0, %d)" % n_seq) and _untouched(out), words
    with pytest.raises(R.RnamotifError, match="record 17: entry"):
        sc.seq_check(db, bad)
    # an element that passes its entry's end
    bad = hits.clone()
    slen = len(floating["w"]["entries"][int(bad[500, 0])])
    bad[500, HDR + 1] = slen - int(bad[500, HDR]) + 1
    bad[900, HDR] = -2
    rc, words = _raw_call(sc, db, bad, *out)
    assert rc != 0 and words.startswith("record 500: element 0 at offset %d, length %d, outside entry" % (int(bad[500, HDR]), int(bad[500, HDR + 1]))), words
    assert _untouched(out)
    # the same call, good: everything is written
    rc, words = _raw_call(sc, db, hits, *out)
    assert rc == 0 and np.array_equal(out[0].cpu().numpy().astype(bool), floating["keep"]) and np.array_equal(out[1].cpu().numpy(), floating["fixed"])


def test_budget_stops_the_call(built, seq_checker, tmp_path):
    """tests/test_seq_check_cpu.py's budget case: records 2 and 3 need 155 and 231 steps"""
    name = "table10"
    argv = descr_args(name, tmp_path)
    d = R.Descriptor(argv)
    entries = [b"gcgc" + b"a" * 30 + b"g" + b"a" * 29 + b"tttt"]
    recs = np.zeros((4, d.hit_stride), dtype=np.int32)
    for h, (off, n) in enumerate(((0, 4), (4, 6), (4, 60), (2, 64))):
        recs[h, 2], recs[h, HDR], recs[h, HDR + 1] = off, off, n
    _, _, free, _, status, _ = run_checker(seq_checker, tmp_path, argv, entries, recs)
    _, _, rows, _, _, _ = run_checker(seq_checker, tmp_path, argv, entries, recs, budget=64)
    first = min(h for h in range(4) if rows[h][0] == "S")
    assert status == 0 and first == 2
    sc, db = _open(d, entries)
    hits = torch.from_numpy(recs).to(DEV)
    sc.seq_check(db, hits[:1])          # (makes the scanner's handle)
    out = _sentinels(hits)
    rc, words = _raw_call(sc, db, hits, *out, budget=64)
    assert rc != 0 and words.startswith("rma_seqcheck_hits: record %d: element 0: " % first) and "budget of 64 steps" in words, words
    assert _untouched(out)
    with pytest.raises(R.RnamotifError, match="record 2: element 0: .*budget of 64 steps"):
        sc.seq_check(db, hits, budget=64)
    # the records in front of it alone pass with 64 steps; all of them with the default
    keep, _ = _checked(sc, db, hits[:first], budget=64)
    assert np.array_equal(keep, np.array([r[0] == "K" for r in free[:first]]))
    keep, fixed = _checked(sc, db, hits)
    assert np.array_equal(keep, np.array([r[0] == "K" for r in free])) and np.array_equal(fixed, recs)
    db.close()
    sc.close()


def test_refusals_before_the_call(floating):
    sc, db, hits, w = floating["sc"], floating["db"], floating["hits"], floating["w"]
    out = _sentinels(hits)
    # the fixed rows may not overlap the records: the same memory, and a part of it
    rc, words = _raw_call(sc, db, hits, out[0], hits.data_ptr())
    assert rc != 0 and "overlap" in words and _untouched(out), words
    two = torch.cat([hits, hits])
    rc, words = _raw_call(sc, db, two[: hits.shape[0]], out[0], two.data_ptr() + (hits.shape[0] - 1) * hits.shape[1] * 4)
    assert rc != 0 and "overlap" in words and _untouched(out), words
    with pytest.raises(ValueError, match="is on cpu"):
        sc.seq_check(db, hits.cpu())
    with pytest.raises(TypeError, match="int32"):
        sc.seq_check(db, hits.to(torch.int64))
    with pytest.raises(ValueError, match="shape"):
        sc.seq_check(db, hits[:, :-1])
    with pytest.raises(ValueError, match="budget"):
        sc.seq_check(db, hits, budget=-1)
    # a host-made database: the replay's words from the call, a ValueError before it
    hdb = sc.database(w["entries"])
    rc, words = _raw_call(sc, hdb, hits, *out)
    assert rc != 0 and "was not made by rma_db_create_device() or has been destroyed" in words and _untouched(out), words
    with pytest.raises(ValueError, match="not made by database_from_tensor"):
        sc.seq_check(hdb, hits)
    hdb.close()
    text, off = _ragged(w["raw"])
    gone = sc.database_from_tensor(text, offsets=off)
    gone.close()
    with pytest.raises(ValueError, match="closed"):
        sc.seq_check(gone, hits)
    # a handle of another descriptor
    other = R.SeqCheck(R.Descriptor(["-descr", os.path.join(ROOT, "tests", "golden", "descr", "trna.descr")]))
    with pytest.raises(R.RnamotifError, match="another descriptor"):
        sc.seq_check(db, hits, check=other)
    other.close()
    with pytest.raises(ValueError, match="open SeqCheck"):
        sc.seq_check(db, hits, check=other)


def test_the_score_section_follows(built, loose_db, tmp_path):
    raw, seqs = loose_db
    text = ("parms\n\tiupac = 0;\ndescr\n\th5(tag='a',minlen=2,maxlen=3)\n\t\tss(tag='l',minlen=4,maxlen=4,seq=\"^nrac$\",mismatch=1)\n\th3(tag='a')\n"
            "score\n\t{ SCORE = mismatches( ss( tag='l' ) ) * 10 + length( h5( tag='a' ) ); if( SCORE == 2 ) REJECT; }\n")
    (tmp_path / "s.descr").write_text(text)
    d = R.Descriptor(["-descr", str(tmp_path / "s.descr")])
    with pytest.raises(R.RnamotifError, match="the descriptor is loose \\(element 1's seq= is tested by a necessary condition only\\)"):
        R.ScoreProgram(d)
    prog = R.ScoreProgram(d, checked=True)
    sc, db = _open(d, raw)
    hits = sc.scan_tensor(db)
    r = sc.seq_check(db, hits)
    cand = r.hits[r.keep]
    s = sc.score(db, cand, prog)
    torch.cuda.synchronize()
    mask, lines = _replayed(d, db, hits, tmp_path / "out.txt")
    keep, acc = r.keep.cpu().numpy(), s.accept.cpu().numpy()
    got = np.zeros(len(keep), dtype=bool)
    got[np.flatnonzero(keep)[acc]] = True
    print("%d records, %d candidates, %d hits" % (len(keep), keep.sum(), got.sum()))
    assert np.array_equal(got, mask)
    assert keep.sum() > got.sum() > 0 and not keep.all()
    for k, h in enumerate(np.flatnonzero(acc)):
        assert s.text(int(h)) == lines[k][12:21], (h, lines[k])
    prog.close()
    db.close()
    sc.close()


def test_a_descriptor_that_is_not_loose(built):
    """trna.descr: no expressions -- the records are checked, every keep is 1 and the fixed rows are the input rows.  (A
    database of a few hundred bases has no candidate of trna.descr's: the scan is over 200 000 synthetic bases, 11 records,
    and hand-made rows over the six small entries stand in for more.)"""
    d = R.Descriptor(["-descr", os.path.join(ROOT, "tests", "golden", "descr", "trna.descr")])
    assert d.loose == 0
    sc = R.Scanner(d, device=0)
    seqs = R.synthetic_records(1, length=200_000)
    text, off = _ragged(seqs)
    db = sc.database_from_tensor(text, offsets=off)
    hits = sc.scan_tensor(db)
    keep, fixed = _checked(sc, db, hits)
    assert len(keep) > 0 and keep.all() and np.array_equal(fixed, hits.cpu().numpy())
    assert sc._seq_check.info["expressions"] == 0
    db.close()
    raw = raw_entries()
    text, off = _ragged(raw)
    db = sc.database_from_tensor(text, offsets=off)
    rng = np.random.default_rng(3)
    rows = np.zeros((1000, d.hit_stride), dtype=np.int32)
    rows[:, 0] = rng.integers(0, len(raw), size=1000)
    rows[:, 1] = rng.integers(0, 2, size=1000)
    for e in range(d.n_elems):
        rows[:, HDR + 4 * e] = rng.integers(0, 30, size=1000)
        rows[:, HDR + 4 * e + 1] = rng.integers(0, 10, size=1000)
    rows[:, HDR + 2::4][:, :d.n_elems] = rng.integers(0, 3, size=(1000, d.n_elems))
    keep, fixed = _checked(sc, db, torch.from_numpy(rows).to(DEV))
    assert keep.all() and np.array_equal(fixed, rows)
    bad = rows.copy()
    bad[77, HDR + 1] = 400
    with pytest.raises(R.RnamotifError, match="record 77: element 0"):
        sc.seq_check(db, torch.from_numpy(bad).to(DEV))
    db.close()
    sc.close()
