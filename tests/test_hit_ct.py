"""GPU: hit records as rm2ct writes them, on the device (Scanner.ct_hits, rma_hit_ct_size, rma_hit_ct: the size and fill
kernels of rm_hitct_dev.hip) against the same rule, rm_hitct.h, run on the host through tests/hostsim/hit_ct_check.cpp --
byte for byte in bytes and offsets, in both types -- and against bin/rm2ct over what print_hits() writes:

  * the duplex cases of test_hit_ct_cpu.py over the reference's test database, scanned and scored on the device, a few
    hundred records each; the rows made by hand there, the entry of more than 10^9 bases among them;
  * end to end for trna with its score section: ct_hits(...).write() is `rm2ct [-t rnaviz]` of print_hits(...).write();
  * the shapes at which the kernels can go wrong: nb of 0, 1, 63, 64, 65, 128, 129 and 10 001 in one batch, accepted and
    not accepted records mixed, one record and none, 2^17 + 3 records (the chunk seam and the carried offset), a strided
    row selection made contiguous;
  * refusals with their words, the outputs left as they were;
  * the fill call ordered behind and ahead of the work on the caller's stream.

torch is imported before the product library: one HIP runtime serves the process."""
import ctypes
import os
import re

import torch  # noqa: F401  (first: its HIP runtime is the process's)

import numpy as np
import pytest

import rnamotif_amd as R
from test_hit_ct_cpu import (DUPLEX, ENTRIES, NB, SDEFS, SIDS, TOOL, TYPES, _descr_of, _rows, columns, ct_checker, hand_sets,  # noqa: F401
                             host_ct, rm2ct)
from test_hit_print import Case, _descr, _written, fasta, trna  # noqa: F401
from test_hit_print_cpu import HAND
from test_hit_structures_cpu import HDR, program_of

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

DEV = torch.device("cuda", 0)
CHUNK = 1 << 17


def _same(p, off, data, what=""):
    torch.cuda.synchronize()
    assert p.off.dtype == torch.int64 and p.bytes.dtype == torch.uint8, what
    assert np.array_equal(p.off.cpu().numpy(), off), what
    assert p.bytes.cpu().numpy().tobytes() == data, what


def _db(d, seqs, lead=3):
    """a scanner and the device database of these entries, not scanned"""
    sc = R.Scanner(d, device=0)
    flat = b"x" * lead + b"".join(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64) + lead
    db = sc.database_from_tensor(torch.frombuffer(bytearray(flat), dtype=torch.uint8).to(DEV), offsets=off)
    return sc, db


def _scores(cols, accept=None, width=None):
    """HitScores of records whose score columns are these bytes"""
    text_len, text_bytes = columns(cols, width)
    n = len(cols)
    acc = np.ones(n, dtype=bool) if accept is None else np.asarray(accept, dtype=bool)
    return R.HitScores(torch.from_numpy(acc).to(DEV), torch.zeros(n, dtype=torch.float64, device=DEV), torch.zeros(n, dtype=torch.int8, device=DEV),
                       torch.from_numpy(text_bytes).to(DEV), torch.from_numpy(text_len).to(DEV))


class Hand:
    """the entries of test_hit_ct_cpu.py's rows on the device, for one descriptor"""

    def __init__(self, d):
        self.d = d
        self.sc, self.db = _db(d, ENTRIES)
        self.names = R.EntryNames(self.sc, self.db, SIDS, SDEFS)

    def both(self, checker, tmp, recs, cols, accept=None, what=""):
        hits = torch.from_numpy(np.ascontiguousarray(recs)).to(DEV)
        s = _scores(cols, accept)
        text_len, text_bytes = columns(cols)
        for type in TYPES:
            p = self.sc.ct_hits(self.db, hits, s, names=self.names, type=type)
            _same(p, *host_ct(checker, tmp, self.d, ENTRIES, recs, SIDS, SDEFS, text_len, text_bytes, type, accept=accept), (what, type))
        return p

    def close(self):
        self.names.close()
        self.db.close()
        self.sc.close()


@pytest.mark.parametrize("name", DUPLEX)
def test_cases(built, ct_checker, fasta, workdir, tmp_path, name):
    c = Case(name, fasta, workdir)
    hits = c.hits[:400].contiguous()
    assert int(hits.shape[0]) >= 1
    s = c.sc.score(c.db, hits, c.prog, text=True)
    assert bool(s.accept.any())
    for type in TYPES:
        p = c.sc.ct_hits(c.db, hits, s, names=c.names, type=type)
        off, data = host_ct(ct_checker, tmp_path, c.d, c.seqs, hits.cpu().numpy(), c.sids, c.sdefs, s.text_len.cpu().numpy(),
                            s.text_bytes.cpu().numpy(), type, accept=s.accept.cpu().numpy())
        _same(p, off, data, (name, type))
        first = int(np.flatnonzero(s.accept.cpu().numpy())[0])
        assert p.record(first) == data[off[first]:off[first + 1]] and len(p.record(first)) > 0
    c.close()


def test_end_to_end_is_the_tools(built, trna, tmp_path):
    c = trna
    s = c.sc.score(c.db, c.hits, c.prog, text=True)
    printed = _written(c.sc.print_hits(c.db, c.hits, s, names=c.names), tmp_path / "hits.out")
    assert printed.startswith(b"#RM scored\n")
    for type in TYPES:
        rc, want, _ = rm2ct(TOOL, type, printed)
        p = c.sc.ct_hits(c.db, c.hits, s, names=c.names, type=type)
        with open(str(tmp_path / "device.ct"), "wb") as f:
            n = p.write(f)
        got = open(str(tmp_path / "device.ct"), "rb").read()
        assert rc == 0 and n == len(got) and got == want and len(want) > 0, type
    # a strided row selection made contiguous, as the chain produces it
    rows = c.hits[1::3].contiguous()
    s = c.sc.score(c.db, rows, c.prog, text=True)
    printed = _written(c.sc.print_hits(c.db, rows, s, names=c.names), tmp_path / "rows.out")
    for type in TYPES:
        assert c.sc.ct_hits(c.db, rows, s, names=c.names, type=type).bytes.cpu().numpy().tobytes() == rm2ct(TOOL, type, printed)[1]


@pytest.mark.parametrize("key", ["hand", "two", "ctx", "pk", "p53", "energy"])
def test_rows_made_by_hand(built, ct_checker, tmp_path, key):
    d, recs, cols = hand_sets(tmp_path)[key]
    h = Hand(d)
    h.both(ct_checker, tmp_path, recs, cols, what=key)
    h.close()


def test_ten_digit_offset(built, ct_checker, tmp_path):
    """An entry of more than 10^9 bases: the last column has ten digits.  The host's entries file is sparse."""
    d = _descr_of(tmp_path, "hand", HAND)
    slen = 1_000_000_100
    tail = b"acgtgcatta" * 5
    ent = os.path.join(str(tmp_path), "sparse.bin")
    with open(ent, "wb") as f:
        f.write(np.asarray([1, slen], dtype=np.int32).tobytes())
        f.seek(8 + slen - len(tail))
        f.write(tail)
    text = torch.zeros(slen, dtype=torch.uint8, device=DEV)
    text[slen - len(tail):] = torch.frombuffer(bytearray(tail), dtype=torch.uint8).to(DEV)
    sc = R.Scanner(d, device=0)
    db = sc.database_from_tensor(text, offsets=np.asarray([0, slen], dtype=np.int64))
    names = R.EntryNames(sc, db, [b"x"], [b""])
    recs = _rows(d, program_of(d), [(0, 0, slen - 20, (3, 4, 3)), (0, 1, 5, (3, 2, 3))])
    cols = [b"   0.000"] * 2
    text_len, text_bytes = columns(cols)
    for type in TYPES:
        p = sc.ct_hits(db, torch.from_numpy(recs).to(DEV), _scores(cols), names=names, type=type)
        off, data = host_ct(ct_checker, tmp_path, d, [slen], recs, [b"x"], [b""], text_len, text_bytes, type, ent_file=ent)
        _same(p, off, data, type)
        assert data[:off[1]].split(b"\n")[1].split()[-1] == b"%d" % (slen - 19)
    names.close()
    db.close()
    sc.close()


def test_shapes(built, ct_checker, tmp_path):
    d = _descr_of(tmp_path, "hand", HAND)
    p = program_of(d)
    h = Hand(d)
    nbs = (0, 1, 63, 64, 65, 128, 129, 10_001, 64, 0, 129, 2)
    rows = [(2, k % 2, 977 * k, (min(nb // 3, 3), nb - 2 * min(nb // 3, 3), min(nb // 3, 3))) for k, nb in enumerate(nbs)]
    recs = _rows(d, p, rows)
    cols = [b"%8.3f" % (k - 3.5) for k in range(len(rows))]
    h.both(ct_checker, tmp_path, recs, cols, what="all")
    for mask in ([1, 0, 1, 1, 0, 0, 1, 1, 0, 1, 0, 1], [0, 1, 0, 0, 1, 1, 0, 0, 1, 0, 1, 0], [0] * 12):
        got = h.both(ct_checker, tmp_path, recs, cols, accept=np.asarray(mask, dtype=bool), what=mask)
        width = (got.off[1:] - got.off[:-1]).cpu().numpy()
        assert ((width > 0) == np.asarray(mask, dtype=bool)).all()
    # one record and none
    one = h.both(ct_checker, tmp_path, recs[7:8], cols[7:8], what="one")
    assert tuple(one.off.shape) == (2,) and int(one.off[1]) == one.bytes.numel() > 10_001 * 20
    none = h.sc.ct_hits(h.db, torch.from_numpy(recs[:0]).to(DEV), _scores([]), names=h.names)
    torch.cuda.synchronize()
    assert tuple(none.off.shape) == (1,) and int(none.off[0]) == 0 and none.bytes.numel() == 0
    h.close()


def test_chunk_seam(built, ct_checker, tmp_path):
    """2^17 + 3 records of a three-base hairpin: the second chunk's offsets run on from the first's."""
    d = _descr_of(tmp_path, "hand", HAND)
    h = Hand(d)
    n = CHUNK + 3
    k = np.arange(n)
    recs = np.zeros((n, d.hit_stride), dtype=np.int32)
    recs[:, 0], recs[:, 1] = 2, k % 2
    at = (k * 7919) % 10_000_000
    for e in range(3):
        recs[:, HDR + 4 * e], recs[:, HDR + 4 * e + 1] = at + e, 1
    cols = [b"%8.3f" % ((i % 1000) / 8 - 60) for i in range(n)]
    text_len, text_bytes = columns(cols)
    hits = torch.from_numpy(recs).to(DEV)
    s = _scores(cols)
    for type in TYPES:
        p = h.sc.ct_hits(h.db, hits, s, names=h.names, type=type)
        torch.cuda.synchronize()
        off = p.off.cpu().numpy()
        lo, hi = CHUNK - 3, CHUNK + 3
        o6, d6 = host_ct(ct_checker, tmp_path, d, ENTRIES, recs[lo:hi], SIDS, SDEFS, text_len[lo:hi], text_bytes[lo:hi], type)
        assert np.array_equal(off[lo:hi + 1] - off[lo], o6)
        assert p.bytes[int(off[lo]):int(off[hi])].cpu().numpy().tobytes() == d6
        # by total length: every record is a header line and three lines of the same widths but for hn's digits
        oall, dall = host_ct(ct_checker, tmp_path, d, ENTRIES, recs, SIDS, SDEFS, text_len, text_bytes, type)
        assert int(off[-1]) == len(dall) == p.bytes.numel() and np.array_equal(off, oall)
        assert p.record(n - 1) == dall[oall[n - 1]:]
    h.close()


def test_stream_order(built, ct_checker, tmp_path):
    d, recs, cols = hand_sets(tmp_path)["hand"]
    h = Hand(d)
    hits = torch.from_numpy(recs).to(DEV)
    s = _scores(cols)
    want = h.sc.ct_hits(h.db, hits, s, names=h.names, type="rnaviz")
    torch.cuda.synchronize()
    text = h.db._text
    good = text.clone()
    text.fill_(ord("n"))                # (the text spoilt: letters read of it now are all n)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    filler = torch.zeros(64 << 20, dtype=torch.int32, device=DEV)
    with torch.cuda.stream(side):
        late = torch.zeros_like(hits)
        filler.add_(1)                  # (something to wait behind)
        text.copy_(good)                # the kernels that write the text and the records, then the call right behind
        late.copy_(hits)
        p = h.sc.ct_hits(h.db, late, s, names=h.names, type="rnaviz")
        total = p.bytes.sum()           # ... and a consumer right behind the call
    side.synchronize()
    assert torch.equal(p.bytes, want.bytes) and torch.equal(p.off, want.off)
    assert int(total) == int(want.bytes.sum())
    h.close()


def test_refusals(built, ct_checker, workdir, tmp_path):
    d, recs, cols = hand_sets(tmp_path)["energy"]
    h = Hand(d)
    sc, db = h.sc, h.db
    n = len(recs)
    hits = torch.from_numpy(recs).to(DEV)
    s = _scores(cols, width=24)
    good = sc.ct_hits(db, hits, s, names=h.names, type="rnaviz")
    torch.cuda.synchronize()
    total, width = int(good.bytes.numel()), 24
    words_of = " ".join(d.names()).encode()
    L = R.lib()
    buf = ctypes.create_string_buffer(1024)

    def call(rows=hits, text_len=s.text_len, text_bytes=s.text_bytes, tot=total, type=1, names=h.names._h, letters=None, words=words_of, scanner=sc._h, dbh=db._h):
        out = (torch.full((total + 64,), 77, dtype=torch.uint8, device=DEV), torch.full((n + 9,), -77, dtype=torch.int64, device=DEV))
        torch.cuda.synchronize()
        first = (scanner, dbh, names, rows.data_ptr(), n, None, text_bytes.data_ptr(), width, text_len.data_ptr(), type, words, letters)
        size = ctypes.c_int64(-1)
        rc0 = L.rma_hit_ct_size(*first, ctypes.byref(size), None, buf, 1024)
        said = buf.value.decode()
        rc = L.rma_hit_ct(*first, tot, out[0].data_ptr(), out[1].data_ptr(), None, buf, 1024)
        torch.cuda.synchronize()
        return rc0, said, int(size.value), rc, buf.value.decode(), out

    def untouched(out):
        return bool((out[0] == 77).all()) and bool((out[1] == -77).all())

    def refused(pattern, **kw):
        rc0, said, size, rc, err, out = call(**kw)
        assert rc0 == 1 and size == 0 and re.search(pattern, said), said
        assert rc == 1 and re.search(pattern, err) and untouched(out), err

    rc0, _, size, rc, _, out = call()
    assert rc0 == 0 and size == total and rc == 0 and torch.equal(out[0][:total], good.bytes) and torch.equal(out[1][:n + 1], good.off)
    assert bool((out[0][total:] == 77).all()) and bool((out[1][n + 1:] == -77).all())
    # before any record is looked at
    q = _descr(["-descr", "qu+tr.descr"], cwd=workdir)
    scq, dbq = _db(q, ENTRIES)
    namesq = R.EntryNames(scq, dbq, SIDS, SDEFS)
    rowsq = torch.zeros((n, q.hit_stride), dtype=torch.int32, device=DEV)
    refused(r"rma_hit_ct(_size)?: can't make CT file for (quad|triple) helices\.$", rows=rowsq, scanner=scq._h, dbh=dbq._h, names=namesq._h,
            words=" ".join(q.names()).encode())
    with pytest.raises(R.RnamotifError, match="can't make CT file for (quad|triple) helices"):
        scq.ct_hits(dbq, rowsq, s, names=namesq)
    namesq.close()
    dbq.close()
    scq.close()
    refused("type 2: RMA_CT_RNAMOTIF or RMA_CT_RNAVIZ", type=2)
    for bad_name in (b"", b"a b", b"a\tb", b"a\nb"):
        blank = R.EntryNames(sc, db, [SIDS[0], bad_name, SIDS[2]], SDEFS)
        refused("entry 1: its name is empty or has a blank, a tab, a newline", names=blank._h)
        with pytest.raises(R.RnamotifError, match="entry 1: its name is empty or has a blank"):
            sc.ct_hits(db, hits, s, names=blank)
        blank.close()
    table = bytearray(b"n" * 256)
    table[ord("n")] = ord(".")
    refused(r"the letters map byte %d to %d, which is no ASCII letter" % (ord("n"), ord(".")), letters=bytes(table))
    # naming the lowest record
    forged = [(2, 0, len(ENTRIES), r"record 2: entry %d outside \[0, %d\)" % (len(ENTRIES), len(ENTRIES))),
              (3, 1, 2, "record 3: strand 2, not 0 or 1"),
              (1, HDR + 4 * 2, len(ENTRIES[1]) + 1, "record 1: element 2 at offset %d, length .* outside entry" % (len(ENTRIES[1]) + 1))]
    for row, col, value, words in forged:
        bad = hits.clone()
        bad[row, col] = value
        refused(words + ".*nothing written", rows=bad)
        with pytest.raises(R.RnamotifError, match=words):
            sc.ct_hits(db, bad, s, names=h.names)
    for value in (width + 1, -1):
        lens = s.text_len.clone()
        lens[4], lens[9] = value, value
        refused(r"record 4: a score column of %d bytes, outside the \[0, %d\] of text_width: nothing written" % (value, width), text_len=lens)
    tb = s.text_bytes.clone()
    tb[5, 2], tb[11, 0] = 10, 10                      # (record 11's column is one byte long)
    refused("record 5: a newline in its score column: nothing written", text_bytes=tb)
    long_rows = hits.clone()
    long_rows[6, 0], long_rows[6, HDR] = 2, 10
    long_rows[6, HDR + 4], long_rows[6, HDR + 5] = 13, 49_960
    long_rows[6, HDR + 8] = 13 + 49_960
    refused(r"record 6: a hit line of 50000 bytes or more \(rm2ct's line buffer\): nothing written", rows=long_rows)
    for text in (b"1e5", b"inf", b"nan", b"0x1p3", b"12345678901234567890"):
        tb = s.text_bytes.clone()
        lens = s.text_len.clone()
        tb[8, :len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(DEV)
        lens[8] = len(text)
        refused(r"record 8: the text behind its name is .* \(HC_NUMBER\): nothing written", text_bytes=tb, text_len=lens)
        rc0, _, size, rc, _, out = call(text_bytes=tb, text_len=lens, type=0, tot=-1)      # rnamotif does not read it
        assert rc0 == 0 and size > 0
    with pytest.raises(R.RnamotifError, match=r"record 8: .*HC_NUMBER"):
        sc.ct_hits(db, hits, R.HitScores(s.accept, s.score, s.kind, tb, lens), names=h.names, type="rnaviz")
    # a total that is not the size call's
    for tot in (total - 1, total + 1):
        rc0, _, size, rc, err, out = call(tot=tot)
        assert rc0 == 0 and rc == 1 and ("have %d bytes, not the %d of `total`: nothing written" % (total, tot)) in err and untouched(out), err
    with pytest.raises(ValueError, match="type: 'rnamotif' or 'rnaviz'"):
        sc.ct_hits(db, hits, s, names=h.names, type="ct")
    # a good call still works
    again = sc.ct_hits(db, hits, s, names=h.names, type="rnaviz")
    assert torch.equal(again.bytes, good.bytes) and torch.equal(again.off, good.off)
    h.close()
