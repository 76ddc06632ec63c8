"""GPU: the score section on the device (Scanner.score, rma_score_hits: rma_score_kernel of rm_score_dev.hip) against the
host replay and against the same rule, rm_score_core.h, run on the host through tests/hostsim/score_check.cpp:

  * the golden cases of tests/test_score_device_cpu.py (which holds the rule to ScoreVM::run) and ire.descr / ire.1.descr
    over synthetic records, on the records of the GPU scan: accept equals the `accepted` mask of
    Replay.device(..., accepted=True), text(h) of every accepted record equals bytes 12-20 of its printed line, score and
    kind equal the checker's bit for bit;
  * rows: shuffled, duplicated and subset rows of records on both strands; 0, 1, 63, 64 and 65 rows; 2^17 + 1 rows, made
    by indexing a small scan's records, which crosses a chunk of the call;
  * databases: database_from_tensor(alphabet=), database_from_fasta_tensor, a letters table;
  * the budget: a for loop of 3000 rounds stops with score_budget at 1000, naming the record, and runs through with the
    default -- the loop ends by itself whatever the budget does;
  * failed calls -- a bad record, a stopped record, a host-made database, a program of another descriptor -- fail with
    their words and leave the three output tensors, prefilled with a sentinel, as they were.

torch is imported before the product library: one HIP runtime serves the process."""
import ctypes as C
import os

import torch  # noqa: F401  (first: its HIP runtime is the process's)

import numpy as np
import pytest

import rnamotif_amd as R
from test_score_device_cpu import (ALL_GOLDEN, ALL_SYNTHETIC, GOLDEN_CASES, HP, OWN, SYNTHETIC, STOPS, descr_args, entries_of, own_args,  # noqa: F401
                                   plain, run_checker, score_checker, synthetic_entries)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

DEV = torch.device("cuda", 0)


def _ragged(seqs, lead=3):
    flat = b"x" * lead + b"".join(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64) + lead
    return torch.frombuffer(bytearray(flat), dtype=torch.uint8).to(DEV), off


def _open(d, seqs):
    sc = R.Scanner(d, device=0)
    text, off = _ragged(seqs)
    db = sc.database_from_tensor(text, offsets=off)
    return sc, db, sc.scan_tensor(db)


def _replayed(d, db, rows, path, letters=None):
    """(the accepted mask, the printed hit lines) of the host path"""
    rp = R.Replay(d, str(path))
    n, mask = rp.device(db, rows, letters=letters, accepted=True)
    rp.close()
    lines = [ln for ln in open(str(path), "rb").read().split(b"\n") if ln and not ln.startswith(b"#") and not ln.startswith(b">")]
    assert n == int(mask.sum()) == len(lines)
    return mask, lines


def _scored(sc, db, rows, prog, letters=None):
    s = sc.score(db, rows, prog, letters=letters)
    n = rows.shape[0]
    assert s.accept.dtype == torch.bool and s.score.dtype == torch.float64 and s.kind.dtype == torch.int8
    assert tuple(s.accept.shape) == tuple(s.score.shape) == tuple(s.kind.shape) == (n,) and s.accept.device == rows.device
    torch.cuda.synchronize()
    return s, s.accept.cpu().numpy(), s.score.cpu().numpy().view(np.uint64), s.kind.cpu().numpy()


def _expected(rows):
    """(accept, bits, kind) of the checker's lines"""
    acc = np.array([r[0] == "A" for r in rows], dtype=bool)
    return acc, np.array([r[2] for r in rows], dtype=np.uint64), np.array([r[1] for r in rows], dtype=np.int8)


def _against_both(d, sc, db, hits, prog, checker, tmp, argv, seqs, letters=None, check=True):
    recs = hits.cpu().numpy()
    s, acc, bits, kind = _scored(sc, db, hits, prog, letters=letters)
    mask, lines = _replayed(d, db, hits, tmp / "dev.txt", letters=letters)
    assert np.array_equal(acc, mask)
    for k, h in enumerate(np.flatnonzero(acc)):
        assert s.text(int(h)) == lines[k][12:21], (h, lines[k])
    if check:
        refused, image, rows, status, out = run_checker(checker, tmp, argv, seqs, recs)
        assert refused is None and status == 0 and len(rows) == len(recs)
        want = _expected(rows)
        assert np.array_equal(acc, want[0]) and np.array_equal(bits, want[1]) and np.array_equal(kind, want[2])
    return recs, acc


@pytest.mark.parametrize("name", ALL_GOLDEN + ALL_SYNTHETIC)
def test_golden_cases(built, score_checker, gbrna, tmp_path, name):
    argv = descr_args(name)
    d = R.Descriptor(argv)
    seqs = synthetic_entries() if plain(name) in SYNTHETIC else entries_of(gbrna, GOLDEN_CASES[plain(name)][1], odd=False)
    sc, db, hits = _open(d, seqs)
    prog = R.ScoreProgram(d)
    recs, acc = _against_both(d, sc, db, hits, prog, score_checker, tmp_path, argv, seqs)
    print("%s: %d records, %d accepted" % (name, len(recs), acc.sum()))
    if plain(name) in SYNTHETIC or GOLDEN_CASES[plain(name)][2]:
        assert acc.any() and not acc.all()
    elif GOLDEN_CASES[plain(name)][2] is None:
        assert len(recs) == 0           # (no candidate in the test database: a scan that finds one is noticed)
    else:
        assert acc.all()
    prog.close()
    db.close()
    sc.close()


@pytest.fixture(scope="module")
def hairpins(built, score_checker, gbrna, tmp_path_factory):
    """the string-variable descriptor over 30 entries: records on both strands, and the checker's lines for them"""
    tmp = tmp_path_factory.mktemp("score_rows")
    argv = own_args(OWN["string variable"][0], tmp, "rows")
    d = R.Descriptor(argv)
    seqs = entries_of(gbrna, 30)
    sc, db, hits = _open(d, seqs)
    prog = R.ScoreProgram(d)
    recs = hits.cpu().numpy()
    refused, image, rows, status, out = run_checker(score_checker, tmp, argv, seqs, recs)
    assert refused is None and status == 0 and len(rows) == len(recs) > 1000
    assert (recs[:, 1] == 0).sum() > 100 and (recs[:, 1] == 1).sum() > 100
    yield {"d": d, "argv": argv, "seqs": seqs, "sc": sc, "db": db, "hits": hits, "prog": prog, "want": _expected(rows)}
    prog.close()
    db.close()
    sc.close()


def _rows_equal(h, idx):
    at = torch.as_tensor(idx, dtype=torch.int64, device=DEV)
    s, acc, bits, kind = _scored(h["sc"], h["db"], h["hits"][at], h["prog"])
    want = h["want"]
    idx = np.asarray(idx, dtype=np.int64)
    assert np.array_equal(acc, want[0][idx]) and np.array_equal(bits, want[1][idx]) and np.array_equal(kind, want[2][idx])
    return acc


def test_rows_in_any_order(hairpins):
    n = hairpins["hits"].shape[0]
    rng = np.random.default_rng(11)
    acc = _rows_equal(hairpins, np.arange(n))
    assert acc.any() and not acc.all()
    _rows_equal(hairpins, rng.permutation(n))
    _rows_equal(hairpins, np.repeat(rng.permutation(n)[:300], 3))
    _rows_equal(hairpins, np.sort(rng.permutation(n)[:777])[::-1].copy())
    for k in (0, 1, 63, 64, 65):
        _rows_equal(hairpins, np.arange(k) + 5)


def test_out_tensors(hairpins):
    """out=: the caller's three tensors are written and returned; wrong ones are refused before the call"""
    h = hairpins
    rows = h["hits"][:200]
    out = (torch.zeros(200, dtype=torch.bool, device=DEV), torch.full((200,), -1.0, dtype=torch.float64, device=DEV),
           torch.full((200,), 5, dtype=torch.int8, device=DEV))
    s = h["sc"].score(h["db"], rows, h["prog"], out=out)
    torch.cuda.synchronize()
    assert s.accept is out[0] and s.score is out[1] and s.kind is out[2]
    assert np.array_equal(out[0].cpu().numpy(), h["want"][0][:200]) and np.array_equal(out[1].cpu().numpy().view(np.uint64), h["want"][1][:200])
    assert np.array_equal(out[2].cpu().numpy(), h["want"][2][:200])
    for bad in ((out[0][:199], out[1], out[2]), (out[0], out[1].to(torch.float32), out[2]), (out[0], out[1], out[2].cpu())):
        with pytest.raises(ValueError, match="out: "):
            h["sc"].score(h["db"], rows, h["prog"], out=bad)


def test_more_rows_than_a_chunk(hairpins):
    n = hairpins["hits"].shape[0]
    idx = (np.arange((1 << 17) + 1) * 7) % n
    acc = _rows_equal(hairpins, idx)
    assert acc[: 1 << 17].any() and idx[-1] != idx[0]


def test_alphabet_tokens(built, score_checker, gbrna, tmp_path):
    argv = own_args(OWN["in"][0], tmp_path, "alphabet")
    d = R.Descriptor(argv)
    seqs = entries_of(gbrna, 30)
    lut = np.full(256, 4, dtype=np.uint8)
    lut[np.frombuffer(b"acgt", dtype=np.uint8)] = np.arange(4, dtype=np.uint8)
    tokens = torch.from_numpy(lut[np.frombuffer(b"".join(seqs), dtype=np.uint8)]).to(DEV)
    sc = R.Scanner(d, device=0)
    db = sc.database_from_tensor(tokens, lengths=[len(s) for s in seqs], alphabet="acgu")
    hits = sc.scan_tensor(db)
    prog = R.ScoreProgram(d)
    # (the entries are the readers' letters already: token 4 is n)
    recs, acc = _against_both(d, sc, db, hits, prog, score_checker, tmp_path, argv, seqs)
    assert acc.any() and not acc.all()
    prog.close()
    db.close()
    sc.close()


def test_fasta_tensor(built, score_checker, gbrna, tmp_path):
    argv = own_args(OWN["$"][0], tmp_path, "fasta")
    d = R.Descriptor(argv)
    raw = open(gbrna, "rb").read()
    text = raw[:raw.index(b"\n>", 60_000) + 1]
    sc = R.Scanner(d, device=0)
    db = sc.database_from_fasta_tensor(torch.frombuffer(bytearray(text), dtype=torch.uint8).to(DEV))
    hits = sc.scan_tensor(db)
    prog = R.ScoreProgram(d)
    seqs = entries_of(gbrna, db.n_seqs, odd=False)
    recs, acc = _against_both(d, sc, db, hits, prog, score_checker, tmp_path, argv, seqs)
    assert db.n_seqs > 10 and acc.any() and not acc.all()
    prog.close()
    db.close()
    sc.close()


def test_letters_table(hairpins, score_checker, tmp_path):
    h = hairpins
    # the readers' letters with a and c exchanged: other strings, other outcomes
    tab = bytearray(R.reader_letter(b) for b in range(256))
    for x, y in ((b"a", b"c"), (b"A", b"C"), (b"c", b"a"), (b"C", b"A")):
        tab[x[0]] = R.reader_letter(y[0])
    tab = bytes(tab)
    seqs = [s.translate(bytes.maketrans(b"ac", b"ca")) for s in h["seqs"]]
    recs, acc = _against_both(h["d"], h["sc"], h["db"], h["hits"], h["prog"], score_checker, tmp_path, h["argv"], seqs, letters=tab)
    assert acc.any() and not acc.all() and not np.array_equal(acc, h["want"][0])
    with pytest.raises(R.RnamotifError, match="the letter 0"):
        h["sc"].score(h["db"], h["hits"], h["prog"], letters=bytes(256))
    with pytest.raises(ValueError, match="256 bytes"):
        h["sc"].score(h["db"], h["hits"], h["prog"], letters=b"acgt")


def test_budget(built, gbrna, tmp_path):
    text = HP + "\t{ n = 0; for( i = 0; i < 3000; i++ ) n = n + i % 7; SCORE = n; }\n"
    d = R.Descriptor(own_args(text, tmp_path, "budget"))
    sc, db, hits = _open(d, entries_of(gbrna, 5))
    rows = hits[:70]
    prog = R.ScoreProgram(d)
    sc.set_option("score_budget", 1000)
    with pytest.raises(R.RnamotifError, match=r"record 0: .*budget\.descr:\d+ more than 1000 instructions"):
        sc.score(db, rows, prog)
    sc.set_option("score_budget", 1 << 20)
    s, acc, bits, kind = _scored(sc, db, rows, prog)
    assert acc.all() and (kind == 1).all() and (s.score.cpu().numpy() == sum(i % 7 for i in range(3000))).all()
    prog.close()
    db.close()
    sc.close()


def _raw_call(sc, prog, db, rows, out):
    err = C.create_string_buffer(4096)
    rc = R.lib().rma_score_hits(sc._h, prog._h, db._h, rows.data_ptr(), rows.shape[0], None, out[0].data_ptr(), out[1].data_ptr(),
                                out[2].data_ptr(), torch.cuda.current_stream(DEV).cuda_stream, err, 4096)
    torch.cuda.synchronize()
    return rc, err.value.decode()


def _sentinels(n):
    return (torch.full((n,), 7, dtype=torch.uint8, device=DEV), torch.full((n,), -12.5, dtype=torch.float64, device=DEV),
            torch.full((n,), 9, dtype=torch.int8, device=DEV))


def _untouched(out):
    return bool((out[0] == 7).all()) and bool((out[1] == -12.5).all()) and bool((out[2] == 9).all())


def test_failed_calls_write_nothing(hairpins, score_checker, gbrna, tmp_path):
    h = hairpins
    sc, db, hits, prog = h["sc"], h["db"], h["hits"], h["prog"]
    n = hits.shape[0]
    # a bad record: the replay's refusal, naming its index
    bad = hits.clone()
    bad[3, 0] = db.n_seqs + 5
    bad[40, 1] = 2
    out = _sentinels(n)
    rc, words = _raw_call(sc, prog, db, bad, out)
    assert rc != 0 and words.startswith("record 3: entry %d outside [0, %d)" % (db.n_seqs + 5, db.n_seqs)) and _untouched(out), words
    with pytest.raises(R.RnamotifError, match="record 3: entry"):
        sc.score(db, bad, prog)
    # a program of another descriptor (one whose descr section differs: the same elements under another score section are
    # the same program to the scanner, and such an image is taken)
    other = R.Descriptor(own_args(OWN["paired triplex"][0], tmp_path, "other"))
    oprog = R.ScoreProgram(other)
    rc, words = _raw_call(sc, oprog, db, hits, out)
    assert rc != 0 and "another descriptor" in words and _untouched(out), words
    oprog.close()
    # a host-made database: the replay's words
    hdb = sc.database(h["seqs"])
    rc, words = _raw_call(sc, prog, hdb, hits, out)
    assert rc != 0 and "was not made by rma_db_create_device() or has been destroyed" in words and _untouched(out), words
    with pytest.raises(ValueError, match="not made by database_from_tensor"):
        sc.score(hdb, hits, prog)
    hdb.close()
    # the same call, good: everything is written
    rc, words = _raw_call(sc, prog, db, hits, out)
    assert rc == 0 and np.array_equal(out[0].cpu().numpy().astype(bool), h["want"][0]) and np.array_equal(out[2].cpu().numpy(), h["want"][2])
    # wrong tensors are refused before the call
    with pytest.raises(TypeError, match="int32"):
        sc.score(db, hits.to(torch.int64), prog)
    with pytest.raises(ValueError, match="shape"):
        sc.score(db, hits[:, :-1], prog)
    with pytest.raises(ValueError, match="is on cpu"):
        sc.score(db, hits.cpu(), prog)


def test_a_stopped_record_fails_the_call(built, score_checker, gbrna, tmp_path):
    argv = own_args(STOPS["division by zero"][0], tmp_path, "stop")
    d = R.Descriptor(argv)
    seqs = entries_of(gbrna, 30)
    sc, db, hits = _open(d, seqs)
    prog = R.ScoreProgram(d)
    recs = hits.cpu().numpy()
    refused, image, rows, status, out = run_checker(score_checker, tmp_path, argv, seqs, recs)
    first = next(k for k, r in enumerate(rows) if r[0] == "S")
    assert status == 0 and first > 0 and any(r[0] == "A" for r in rows)
    sent = _sentinels(len(recs))
    rc, words = _raw_call(sc, prog, db, hits, sent)
    assert rc != 0 and words.startswith("rma_score_hits: record %d: " % first) and rows[first][3] in words and "integer division by zero." in words, words
    assert _untouched(sent)
    # the records in front of it alone are scored
    s, acc, bits, kind = _scored(sc, db, hits[:first], prog)
    assert acc.all() and np.array_equal(bits, _expected(rows[:first])[1])
    prog.close()
    db.close()
    sc.close()
