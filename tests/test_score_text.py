"""GPU: the score section with text on the device (Scanner.score(..., text=True), rma_score_hits_text: rma_score_text_kernel of
rm_score_dev.hip) against the same rule, rm_score_core.h, run on the host through tests/hostsim/score_text_check.cpp (which
tests/test_score_text_cpu.py holds to ScoreVM::run and HitPrinter::print), and against the host replay:

  * the golden programs and the own descriptors of tests/test_score_text_cpu.py on the records of the GPU scan: accept,
    kind, the bits of the double, the score column and its length equal the checker's lines;
  * descr/trna.descr against Replay.device(): the score column of every line it prints equals HitScores.text( h ), accept
    equals its mask;
  * rows in any order; 2^17 + 3 rows made by repeating indices, which cross a chunk of the call and take a fresh heap; a
    letters table; a database made by database_from_fasta_tensor;
  * failed calls -- a stop, a bad record, a text_stride too small -- leave the five outputs, prefilled, as they were;
  * a program opened without text through the text call, a program with text through rma_score_hits().

torch is imported before the product library: one HIP runtime serves the process."""
import ctypes as C
import os

import torch  # noqa: F401  (first: its HIP runtime is the process's)

import numpy as np
import pytest

import rnamotif_amd as R
from test_score_device_cpu import GOLDEN, HP, OWN, entries_of, own_args, run_checker, score_checker  # noqa: F401
from test_score_text_cpu import ALL_GOLDEN_TEXT, OWN_TEXT, STOPS_TEXT, run_text_checker, text_args, text_checker  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

DEV = torch.device("cuda", 0)
W = 64


def _ragged(seqs, lead=3):
    flat = b"x" * lead + b"".join(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64) + lead
    return torch.frombuffer(bytearray(flat), dtype=torch.uint8).to(DEV), off


def _open(d, seqs):
    sc = R.Scanner(d, device=0)
    text, off = _ragged(seqs)
    db = sc.database_from_tensor(text, offsets=off)
    return sc, db, sc.scan_tensor(db)


def _scored(sc, db, rows, prog, letters=None, width=W):
    """(the HitScores, accept, bits, kind, [the column of every record])"""
    s = sc.score(db, rows, prog, letters=letters, text=True, text_width=width)
    n = rows.shape[0]
    assert s.text_bytes.dtype == torch.uint8 and tuple(s.text_bytes.shape) == (n, width) and s.text_len.dtype == torch.int32 and tuple(s.text_len.shape) == (n,)
    torch.cuda.synchronize()
    tb, tl = s.text_bytes.cpu().numpy(), s.text_len.cpu().numpy()
    return s, s.accept.cpu().numpy(), s.score.cpu().numpy().view(np.uint64), s.kind.cpu().numpy(), [tb[h, :tl[h]].tobytes() for h in range(n)]


def _expected(rows):
    return (np.array([r[0] == "A" for r in rows], dtype=bool), np.array([r[2] for r in rows], dtype=np.uint64), np.array([r[1] for r in rows], dtype=np.int8),
            [r[4] for r in rows])


def _equal(got, want, idx=None):
    _, acc, bits, kind, cols = got
    if idx is None:
        idx = np.arange(len(acc))
    assert np.array_equal(acc, want[0][idx]) and np.array_equal(bits, want[1][idx]) and np.array_equal(kind, want[2][idx])
    assert cols == [want[3][i] for i in idx]


def _against_checker(sc, db, hits, prog, checker, tmp, argv, seqs, letters=None):
    recs = hits.cpu().numpy()
    got = _scored(sc, db, hits, prog, letters=letters)
    refused, image, rows, status, out, bits = run_text_checker(checker, tmp, argv, seqs, recs, flags=2 if prog.text else 0)
    assert refused is None and status == 0 and len(rows) == len(recs)
    _equal(got, _expected(rows))
    s = got[0]
    for h in (0, len(recs) // 2, len(recs) - 1):
        assert s.text(h) == b" " + rows[h][4] if rows[h][0] == "A" else s.text(h) == b" "
    return recs, got, rows


@pytest.mark.parametrize("name", ALL_GOLDEN_TEXT)
def test_golden_programs(built, text_checker, gbrna, tmp_path, name):
    argv, limit = text_args(name)
    d = R.Descriptor(argv)
    seqs = entries_of(gbrna, limit, odd=False)
    sc, db, hits = _open(d, seqs)
    prog = R.ScoreProgram(d, text=True)
    recs, got, rows = _against_checker(sc, db, hits, prog, text_checker, tmp_path, argv, seqs)
    print("%s: %d records, %d accepted, %s" % (name, len(recs), got[1].sum(), prog.info()))
    assert got[1].any() and set(got[3][got[1]].tolist()) == {3}
    prog.close()
    db.close()
    sc.close()


@pytest.mark.parametrize("name", sorted(OWN_TEXT))
def test_own_descriptors(built, text_checker, gbrna, tmp_path, name):
    argv = own_args(OWN_TEXT[name][0], tmp_path, name)
    d = R.Descriptor(argv)
    seqs = entries_of(gbrna, 30)
    sc, db, hits = _open(d, seqs)
    prog = R.ScoreProgram(d, text=True)
    recs, got, rows = _against_checker(sc, db, hits, prog, text_checker, tmp_path, argv, seqs)
    assert got[1].any()
    prog.close()
    db.close()
    sc.close()


def test_trna_against_the_replay(built, gbrna, tmp_path):
    """the chain the benchmark's descriptor takes: scan_tensor -> score( text=True ) on the device, against Replay.device()"""
    d = R.Descriptor(["-descr", os.path.join(GOLDEN, "descr", "trna.descr")])
    seqs = R.synthetic_records(2, length=400_000)
    sc, db, hits = _open(d, seqs)
    prog = R.ScoreProgram(d, text=True)
    s, acc, bits, kind, cols = _scored(sc, db, hits, prog)
    path = str(tmp_path / "dev.txt")
    rp = R.Replay(d, path)
    n, mask = rp.device(db, hits, accepted=True)
    rp.close()
    lines = [ln for ln in open(path, "rb").read().split(b"\n") if ln and not ln.startswith(b"#") and not ln.startswith(b">")]
    assert n == int(mask.sum()) == len(lines) > 20 and np.array_equal(acc, np.asarray(mask.cpu() if hasattr(mask, "cpu") else mask, dtype=bool))
    recs = hits.cpu().numpy()
    for k, h in enumerate(np.flatnonzero(acc)):
        t = s.text(int(h))
        assert len(t) == 18 and lines[k][12:12 + len(t)] == t and lines[k][12 + len(t):].startswith(b" %d " % recs[h, 1]), (h, lines[k], t)
    assert (kind[acc] == 3).all() and (bits == 0).all() and len(set(cols)) > 20
    prog.close()
    db.close()
    sc.close()


@pytest.fixture(scope="module")
def made(built, text_checker, gbrna, tmp_path_factory):
    """a program that makes strings of the record's own bases, on both strands, and the checker's lines for its records"""
    tmp = tmp_path_factory.mktemp("score_text_rows")
    text = HP + ("\t{ s = ss( tag='l' ) + '-' + h5( tag='a', pos=1, len=2 ); if( substr( s, 1, 1 ) == 'g' ) REJECT;\n"
                 "\t  SCORE = sprintf( '%s %5.2f %d', s, bits( h5( tag='a' ), h3( tag='a' ) ), LEN ); }\n")
    argv = own_args(text, tmp, "rows")
    d = R.Descriptor(argv)
    seqs = entries_of(gbrna, 30)
    sc, db, hits = _open(d, seqs)
    prog = R.ScoreProgram(d, text=True)
    recs = hits.cpu().numpy()
    refused, image, rows, status, out, bits = run_text_checker(text_checker, tmp, argv, seqs, recs)
    assert refused is None and status == 0 and len(rows) == len(recs) > 1000
    assert (recs[:, 1] == 0).sum() > 100 and (recs[:, 1] == 1).sum() > 100
    yield {"d": d, "argv": argv, "seqs": seqs, "sc": sc, "db": db, "hits": hits, "prog": prog, "want": _expected(rows), "rows": rows}
    prog.close()
    db.close()
    sc.close()


def _rows_equal(h, idx):
    at = torch.as_tensor(idx, dtype=torch.int64, device=DEV)
    got = _scored(h["sc"], h["db"], h["hits"][at], h["prog"])
    _equal(got, h["want"], np.asarray(idx, dtype=np.int64))
    return got[1]


def test_rows_in_any_order(made):
    n = made["hits"].shape[0]
    rng = np.random.default_rng(12)
    acc = _rows_equal(made, np.arange(n))
    assert acc.any() and not acc.all()
    _rows_equal(made, rng.permutation(n))
    _rows_equal(made, np.repeat(rng.permutation(n)[:300], 3))
    for k in (0, 1, 63, 64, 65):
        _rows_equal(made, np.arange(k) + 5)


def test_more_rows_than_a_chunk(made):
    """2^17 + 3 rows: the last three are a launch of their own, with the first heaps of the scratch"""
    n = made["hits"].shape[0]
    idx = (np.arange((1 << 17) + 3) * 7) % n
    at = torch.as_tensor(idx, dtype=torch.int64, device=DEV)
    s = made["sc"].score(made["db"], made["hits"][at], made["prog"], text=True, text_width=W)
    torch.cuda.synchronize()
    want = made["want"]
    assert np.array_equal(s.accept.cpu().numpy(), want[0][idx]) and np.array_equal(s.kind.cpu().numpy(), want[2][idx])
    wl = np.array([len(c) for c in want[3]], dtype=np.int32)
    wb = np.zeros((n, W), dtype=np.uint8)
    for k, c in enumerate(want[3]):
        wb[k, :len(c)] = np.frombuffer(c, dtype=np.uint8)
    assert np.array_equal(s.text_len.cpu().numpy(), wl[idx]) and np.array_equal(s.text_bytes.cpu().numpy(), wb[idx])   # (zeros behind the length: not written)
    assert want[0][idx[-3:]].any() and idx[-1] != idx[0]


def test_letters_table(made, text_checker, tmp_path):
    h = made
    tab = bytearray(R.reader_letter(b) for b in range(256))
    for x, y in ((b"a", b"c"), (b"A", b"C"), (b"c", b"a"), (b"C", b"A")):
        tab[x[0]] = R.reader_letter(y[0])
    seqs = [s.translate(bytes.maketrans(b"ac", b"ca")) for s in h["seqs"]]
    recs, got, rows = _against_checker(h["sc"], h["db"], h["hits"], h["prog"], text_checker, tmp_path, h["argv"], seqs, letters=bytes(tab))
    assert got[1].any() and got[4] != h["want"][3]


def test_fasta_tensor(built, text_checker, gbrna, tmp_path):
    argv = own_args(OWN_TEXT["%s of slices"][0], tmp_path, "fasta")
    d = R.Descriptor(argv)
    raw = open(gbrna, "rb").read()
    text = raw[:raw.index(b"\n>", 60_000) + 1]
    sc = R.Scanner(d, device=0)
    db = sc.database_from_fasta_tensor(torch.frombuffer(bytearray(text), dtype=torch.uint8).to(DEV))
    hits = sc.scan_tensor(db)
    prog = R.ScoreProgram(d, text=True)
    recs, got, rows = _against_checker(sc, db, hits, prog, text_checker, tmp_path, argv, entries_of(gbrna, db.n_seqs, odd=False))
    assert db.n_seqs > 10 and got[1].any()
    prog.close()
    db.close()
    sc.close()


def _raw_call(sc, prog, db, rows, out, stride=W):
    err = C.create_string_buffer(4096)
    rc = R.lib().rma_score_hits_text(sc._h, prog._h, db._h, rows.data_ptr(), rows.shape[0], None, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                     out[3].data_ptr(), stride, out[4].data_ptr(), torch.cuda.current_stream(DEV).cuda_stream, err, 4096)
    torch.cuda.synchronize()
    return rc, err.value.decode()


def _sentinels(n, stride=W):
    return (torch.full((n,), 7, dtype=torch.uint8, device=DEV), torch.full((n,), -12.5, dtype=torch.float64, device=DEV),
            torch.full((n,), 9, dtype=torch.int8, device=DEV), torch.full((n, stride), 0x55, dtype=torch.uint8, device=DEV),
            torch.full((n,), -3, dtype=torch.int32, device=DEV))


def _untouched(out):
    return (bool((out[0] == 7).all()) and bool((out[1] == -12.5).all()) and bool((out[2] == 9).all()) and bool((out[3] == 0x55).all())
            and bool((out[4] == -3).all()))


def test_failed_calls_write_nothing(made, gbrna, tmp_path):
    h = made
    sc, db, hits, prog = h["sc"], h["db"], h["hits"], h["prog"]
    n = hits.shape[0]
    out = _sentinels(n)
    # a bad record
    bad = hits.clone()
    bad[3, 0] = db.n_seqs + 5
    rc, words = _raw_call(sc, prog, db, bad, out)
    assert rc != 0 and words.startswith("record 3: entry %d outside [0, %d)" % (db.n_seqs + 5, db.n_seqs)) and _untouched(out), words
    # a text_stride too small for the longest column
    longest = max(len(c) for c in h["want"][3])
    first = next(k for k, c in enumerate(h["want"][3]) if len(c) > 14)
    small = _sentinels(n, 14)
    rc, words = _raw_call(sc, prog, db, hits, small, stride=14)
    assert longest > 14 and rc != 0 and words.startswith("rma_score_hits_text: record %d: " % first) and _untouched(small), words
    assert "the score column has %d bytes, a row of the text has room for 14 (text_stride)." % len(h["want"][3][first]) in words and "nothing written" in words
    with pytest.raises(R.RnamotifError, match="text_stride"):
        sc.score(db, hits, prog, text=True, text_width=14)
    # a stop: the heap
    sc.set_option("score_heap", 8)
    rc, words = _raw_call(sc, prog, db, hits, out)
    assert rc != 0 and "does not fit a record's heap" in words and "(option score_heap)" in words and _untouched(out), words
    sc.set_option("score_heap", 256)
    # bad arguments
    rc, words = _raw_call(sc, prog, db, hits, out, stride=0)
    assert rc != 0 and "bad arguments" in words and _untouched(out)
    # the same call, good: everything is written, bytes behind a row's length are not
    rc, words = _raw_call(sc, prog, db, hits, out)
    assert rc == 0, words
    tl, tb = out[4].cpu().numpy(), out[3].cpu().numpy()
    assert np.array_equal(out[0].cpu().numpy().astype(bool), h["want"][0]) and np.array_equal(out[2].cpu().numpy(), h["want"][2])
    assert [tb[k, :tl[k]].tobytes() for k in range(n)] == h["want"][3] and all((tb[k, tl[k]:] == 0x55).all() for k in range(n))
    assert (tl[~h["want"][0]] == 0).all() and (tl[h["want"][0]] >= 8).all()
    with pytest.raises(ValueError, match="out: "):
        sc.score(db, hits, prog, text=True, out=out[:3])


@pytest.mark.parametrize("name", ["the heap", "%c", "a missing argument", "a non-finite SCORE"])
def test_a_stopped_record_fails_the_call(built, text_checker, gbrna, tmp_path, name):
    text, words, heap, stride, accepts = STOPS_TEXT[name]
    argv = own_args(text, tmp_path, name)
    d = R.Descriptor(argv)
    seqs = entries_of(gbrna, 30)
    sc, db, hits = _open(d, seqs)
    sc.set_option("score_heap", heap)
    prog = R.ScoreProgram(d, text=True)
    recs = hits.cpu().numpy()
    refused, image, rows, status, out, _ = run_text_checker(text_checker, tmp_path, argv, seqs, recs, heap=heap, stride=stride)
    first = next(k for k, r in enumerate(rows) if r[0] == "S")
    sent = _sentinels(len(recs), stride)
    rc, said = _raw_call(sc, prog, db, hits, sent, stride=stride)
    assert rc != 0 and said.startswith("rma_score_hits_text: record %d: " % first) and rows[first][5] in said and words in said, said
    assert _untouched(sent)
    if first > 0:
        got = _scored(sc, db, hits[:first], prog)
        _equal(got, _expected(rows[:first]))
    prog.close()
    db.close()
    sc.close()


def test_a_program_without_text_through_the_text_call(built, text_checker, score_checker, gbrna, tmp_path):
    """the numeric programs get their score column too: %8d and %8.3lf from the same formatter"""
    for name in ("string variable", "int op float"):
        argv = own_args(OWN[name][0], tmp_path, name)
        d = R.Descriptor(argv)
        seqs = entries_of(gbrna, 30)
        sc, db, hits = _open(d, seqs)
        prog = R.ScoreProgram(d)
        recs, got, rows = _against_checker(sc, db, hits, prog, text_checker, tmp_path, argv, seqs)
        plain = sc.score(db, hits, prog)
        torch.cuda.synchronize()
        assert np.array_equal(plain.accept.cpu().numpy(), got[1]) and np.array_equal(plain.score.cpu().numpy().view(np.uint64), got[2])
        for h in np.flatnonzero(got[1])[:200]:
            assert got[0].text(int(h)) == plain.text(int(h)) and len(got[4][h]) == 8
        assert got[1].any() and set(got[3][got[1]].tolist()) == {1 if name == "string variable" else 2}
        prog.close()
        db.close()
        sc.close()


def test_a_text_program_through_the_numeric_call(built, text_checker, gbrna, tmp_path):
    """rma_score_hits() on a program with text: numbers where SCORE is one, the old stop on a string"""
    argv = own_args(OWN_TEXT["bits in arithmetic"][0], tmp_path, "numeric")
    d = R.Descriptor(argv)
    seqs = entries_of(gbrna, 30)
    sc, db, hits = _open(d, seqs)
    prog = R.ScoreProgram(d, text=True)
    s = sc.score(db, hits, prog)
    torch.cuda.synchronize()
    refused, image, rows, status, out, _ = run_text_checker(text_checker, tmp_path, argv, seqs, hits.cpu().numpy(), stride=0)
    want = _expected(rows)
    assert status == 0 and s.text_bytes is None and np.array_equal(s.accept.cpu().numpy(), want[0]) and want[0].any() and not want[0].all()
    assert np.array_equal(s.score.cpu().numpy().view(np.uint64), want[1]) and np.array_equal(s.kind.cpu().numpy(), want[2])
    prog.close()
    db.close()
    sc.close()
    argv = own_args(OWN_TEXT["s = a + b"][0], tmp_path, "string")
    d = R.Descriptor(argv)
    sc, db, hits = _open(d, seqs)
    prog = R.ScoreProgram(d, text=True)
    with pytest.raises(R.RnamotifError, match=r"rma_score_hits: record 0: .*SCORE holds a string: the device delivers an int or a float"):
        sc.score(db, hits, prog)
    prog.close()
    db.close()
    sc.close()
