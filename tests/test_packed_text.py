"""GPU: a packed database's text made in HBM from its words (Database.device_text, Scanner.database_from_pack(text=True),
rma_db_text_attach*, the kernels of rm_dbtext_dev.hip) against Pack.seq() on the host:

  * the entries of test_packed_text_cpu.py -- 0 .. 4097 bases, exceptions at the seams of slots, mask words and runs --
    plus 300 entries of 0..70 bases (many a wave) and one of 70 001 (many groups), 2 % of the letters from nryswkmbdhv:
    read_text(i) is Pack.seq(i) for a whole pack, a slice of one, entries in any order with one twice, and a database
    of host strings with and without exceptions; Database.packed() is unchanged by the call;
  * the chain over a database made from a pack with text=True: print_hits, list_hits, ct_hits, align and prune give,
    byte for byte, what they give on database_from_fasta_tensor() of the FASTA bytes the pack was read from, names left
    to their defaults on both, and print_hits what Replay.batch() prints of the same records on the host; before
    device_text() every one of them still raises the words it had;
  * the refusals with their words, the database scanning and without text after each; a scan in flight.

torch is imported before the product library: one HIP runtime serves the process."""
import os

import numpy as np
import pytest
import torch

import rnamotif_amd as R
from test_packed_text_cpu import AMBIGUOUS, make_records

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

DEV = torch.device("cuda", 0)
NOT_FROM_TENSOR = r"the database was not made by database_from_tensor\(\)"

HAIRPIN = ("parms\n\twc += gu;\ndescr\n\th5( tag='a', minlen=5, maxlen=6 )\n\t\tss( tag='l', minlen=4, maxlen=6 )\n\th3( tag='a' )\n"
           "\tss( tag='t', len=2 )\nscore\n\t{ SCORE = sprintf( '%s %s %s', h5( tag='a' ), ss( tag='l' ), h3( tag='a' ) ); }\n")


@pytest.fixture(scope="module")
def descr(built, tmp_path_factory):
    path = tmp_path_factory.mktemp("packed_text_descr") / "hairpin.descr"
    path.write_text(HAIRPIN)
    return R.Descriptor(["-descr", str(path)])


@pytest.fixture(scope="module")
def scanner(descr):
    return R.Scanner(descr, device=0)


@pytest.fixture(scope="module")
def big(built, tmp_path_factory):
    """The pack of every shape, written once: (Pack, records)."""
    path = str(tmp_path_factory.mktemp("packed_text") / "big.rmdb")
    recs = make_records(many=300, long=70001)
    R.Pack.write(path, recs)
    return R.Pack(path), recs


def exceptions_of(seq):
    return bytes(c for c in seq if c not in b"acgt")


def same_words(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_whole_pack(scanner, big):
    pk, recs = big
    db = scanner.database_from_pack(pk, text=True)
    assert db.n_seqs == len(recs) and db._text is not None
    assert [pk.seq(i) for i in range(pk.count)] == [r[2] for r in recs]
    for i in range(db.n_seqs):
        assert db.read_text(i) == pk.seq(i), i
    assert db.sids == [r[0] for r in recs] and db.sdefs == [r[1] for r in recs]
    db.close()


def test_slice_any_order_and_host_strings(scanner, big):
    pk, recs = big
    # a slice: the defaults are what the database was made with
    count = len(recs) - 5
    db = scanner.database_from_pack(pk, first=3, count=count)
    before = db.packed()
    assert db.device_text() is db and same_words(before, db.packed())
    for i in range(count):
        assert db.read_text(i) == pk.seq(3 + i), i
    assert db.sids[0] == recs[3][0]
    db.close()
    # entries in any order, one twice, with ranges
    entries = [5, 2, 2, 9, len(recs) - 1, 12, 11]
    db = scanner.database_from_pack(pk, entries=entries, ranges=[(0, 10 ** 6)] * len(entries))
    before = db.packed()
    db.device_text()
    assert same_words(before, db.packed())
    assert [db.read_text(i) for i in range(len(entries))] == [pk.seq(e) for e in entries]
    assert db.sids == [recs[e][0] for e in entries]
    db.close()
    # host strings: the caller's exceptions, or n
    seqs = [r[2] for r in recs[:40]]
    db = scanner.database(seqs)
    db.device_text(exceptions=[exceptions_of(s) for s in seqs])
    assert [db.read_text(i) for i in range(len(seqs))] == seqs
    assert not hasattr(db, "sids")
    db.close()
    db = scanner.database(seqs)
    db.device_text()
    table = bytes(c if c in b"acgt" else ord("n") for c in range(256))
    assert [db.read_text(i) for i in range(len(seqs))] == [s.translate(table) for s in seqs]
    db.close()


def fasta_bytes(recs):
    out = []
    for sid, sdef, seq in recs:
        out.append(b">" + sid + b" " + sdef + b"\n")
        out += [seq[i:i + 60] + b"\n" for i in range(0, len(seq), 60)]
    return b"".join(out)


def written(p, path, **kw):
    with open(str(path), "wb") as f:
        p.write(f, **kw)
    return open(str(path), "rb").read()


def test_chain_is_the_fasta_databases(descr, scanner, tmp_path):
    sc = scanner
    recs = [r for r in make_records(seed=11, many=60) if len(r[2]) > 0]
    text = fasta_bytes(recs)
    fa = tmp_path / "cases.fa"
    fa.write_bytes(text)
    pk = R.Pack.read([str(fa)])
    assert [pk.record(i)[::2] for i in range(pk.count)] == [r[::2] for r in recs]
    prog = R.ScoreProgram(descr, text=True)
    ref = sc.database_from_fasta_tensor(torch.frombuffer(bytearray(text), dtype=torch.uint8).to(DEV))
    db = sc.database_from_pack(pk)
    hits = sc.scan_tensor(db)
    assert torch.equal(hits, sc.scan_tensor(ref)) and hits.shape[0] > 100

    def chain(d):
        s = sc.score(d, hits, prog, text=True)
        kept = hits[s.accept].contiguous()
        a = sc.align(d, kept)
        return {"print": written(sc.print_hits(d, hits, s), tmp_path / "print.out"),
                "list": written(sc.list_hits(d, hits, s), tmp_path / "list.out"),
                "ct": written(sc.ct_hits(d, hits, s), tmp_path / "ct.out"),
                "align": a.rows.cpu().numpy().tobytes() + a.widths.tobytes(),
                "prune": sc.prune(d, kept).cpu().numpy().tobytes()}

    # before the call: the words every one of them had
    zero = R.HitScores(torch.zeros(hits.shape[0], dtype=torch.bool, device=DEV), None, None,
                       torch.zeros((hits.shape[0], 64), dtype=torch.uint8, device=DEV), torch.zeros(hits.shape[0], dtype=torch.int32, device=DEV))
    for call in (lambda: sc.score(db, hits, prog, text=True), lambda: sc.print_hits(db, hits, zero), lambda: sc.list_hits(db, hits, zero),
                 lambda: sc.ct_hits(db, hits, zero), lambda: sc.align(db, hits),
                 lambda: sc.hit_structures(db, hits), lambda: sc.seq_check(db, hits)):
        with pytest.raises(ValueError, match=NOT_FROM_TENSOR):
            call()
    # (prune() reads the entries' lengths alone and never asked for text: it answers as it will with it)
    pruned = sc.prune(db, hits).cpu().numpy()
    rp = R.Replay(descr, str(tmp_path / "no.out"))
    with pytest.raises(ValueError, match=NOT_FROM_TENSOR):
        rp.device(db, hits)
    rp.close()
    before = db.packed()
    db.device_text()
    assert same_words(before, db.packed()) and db.sids == ref.sids and db.sdefs == ref.sdefs
    assert np.array_equal(sc.prune(db, hits).cpu().numpy(), pruned)
    got, want = chain(db), chain(ref)
    for what in want:
        assert got[what] == want[what] and len(want[what]) > 0, what
    # ... and what the host replay prints of the same records
    rp = R.Replay(descr, str(tmp_path / "host.out"))
    rp.batch([r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs], hits.cpu().numpy())
    rp.close()
    assert got["print"] == open(str(tmp_path / "host.out"), "rb").read()
    # the hits read exceptions: their own letters on strand 0, n on strand 1
    lines = [l.split() for l in got["print"].split(b"\n") if l and not l.startswith((b">", b"#"))]
    fields = {c: b"".join(b"".join(l[-4:]) for l in lines if l[-7] == c) for c in (b"0", b"1")}
    assert set(fields[b"0"]) & set(AMBIGUOUS.replace(b"n", b"")) and b"n" in fields[b"1"]
    assert not set(fields[b"1"]) - set(b"acgtn")
    assert torch.equal(sc.scan_tensor(db), hits)
    db.close()
    ref.close()


def test_refusals(scanner, big, tmp_path):
    sc = scanner
    pk, recs = big
    n = 40
    seqs = [r[2] for r in recs[:n]]
    exc = [exceptions_of(s) for s in seqs]
    e = next(i for i, x in enumerate(exc) if len(x) >= 2)          # the least entry with exceptions to take away
    later = next(i for i, x in enumerate(exc) if i > e and x)
    db = sc.database(seqs)
    want = sc.scan(db)

    def refused(words, **kw):
        with pytest.raises(R.RnamotifError, match=words):
            db.device_text(**kw)
        assert db._text is None and np.array_equal(sc.scan(db), want)
        with pytest.raises(R.RnamotifError, match="has no text in device memory"):
            db.read_text(0)

    def changed(i, x, j=None, y=None):
        out = list(exc)
        out[i] = x
        if j is not None:
            out[j] = y
        return out

    have, mask = len(exc[e]), len(exc[e])
    refused(rf"rma_db_text_attach: entry {e}: its mask has {mask} bases set, its exceptions are {have - 1}$",
            exceptions=changed(e, exc[e][:-1], later, exc[later] + b"n"))
    refused(rf"rma_db_text_attach: entry {e}: its mask has {mask} bases set, its exceptions are {have + 1}$", exceptions=changed(e, exc[e] + b"n"))
    refused(rf"rma_db_text_attach: entry {e}: exception 1 is byte 0x61: a lower-case letter other than a, c, g and t stands at a masked position$",
            exceptions=changed(e, exc[e][:1] + b"a" + exc[e][2:], later, b"N" + exc[later][1:]))
    refused(rf"rma_db_text_attach: entry {later}: exception 0 is byte 0x4e: ", exceptions=changed(later, b"N" + exc[later][1:]))
    # a pack entry of another length, and one outside the pack
    other = next(i for i in range(n) if len(seqs[i]) != len(seqs[0]))
    refused(rf"rma_db_text_attach_pack: entry 0 of the database has {len(seqs[0])} bases, entry {other} of the pack {len(seqs[other])}$",
            pack=pk, entries=[other] + list(range(1, n)))
    refused(rf"rma_db_text_attach_pack: entry 1 of the database is entry {pk.count} of the pack, which has {pk.count} entries$",
            pack=pk, entries=[0, pk.count] + list(range(2, n)))
    # a scan begun before and ended after: refused, not raced
    sc.scan_begin(db)
    with pytest.raises(R.RnamotifError, match="rma_db_text_attach: a scan of the database is in flight: end it first$"):
        db.device_text(exceptions=exc)
    assert np.array_equal(sc.scan_end(), want) and db._text is None
    # the call itself, then a second one
    db.device_text(exceptions=exc)
    assert [db.read_text(i) for i in range(n)] == seqs
    for kw in ({"exceptions": exc}, {"pack": pk, "first": 0}, {}):
        with pytest.raises(R.RnamotifError, match=r"rma_db_text_attach(_pack)?: the database already has its text in device memory"):
            db.device_text(**kw)
    assert [db.read_text(i) for i in range(n)] == seqs and np.array_equal(sc.scan(db), want)
    # a closed database
    db.close()
    with pytest.raises(ValueError, match="the database is closed"):
        db.device_text(exceptions=exc)
    with pytest.raises(ValueError, match="the database is closed"):
        db.read_text(0)
    # a database made from device text has its text
    flat = b"".join(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    dev = sc.database_from_tensor(torch.frombuffer(bytearray(flat), dtype=torch.uint8).to(DEV), offsets=off)
    with pytest.raises(R.RnamotifError, match=r"rma_db_text_attach: the database already has its text in device memory"):
        dev.device_text()
    assert dev.read_text(n - 1) == seqs[n - 1] and np.array_equal(sc.scan(dev), want)
    dev.close()


def test_destroyed_database_is_refused_by_the_call(scanner):
    """The C call on a handle rma_db_destroy() has had: words, not a read through it."""
    import ctypes as C
    db = scanner.database([b"acgtnacgt"])
    h = db._h
    db.close()
    err = C.create_string_buffer(512)
    assert R.lib().rma_db_text_attach(h, None, None, None, err, 512) == 1
    assert b"has been destroyed or was never made" in err.value
