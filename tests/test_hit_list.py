"""GPU: hit records as rmfmt lists them, on the device (Scanner.list_hits, rma_hit_list_shape, rma_hit_list: the measure,
compact, sort and fill kernels of rm_hitlist_dev.hip) against the same rule, rm_hitlist.h, run on the host through
tests/hostsim/hit_list_check.cpp -- byte for byte in lines, perm, widths and mode -- and against bin/rmfmt (and
oracle/_ref/rmfmt where it has been built) fed what print_hits(...).write() gives for the same records:

  * the cases of test_hit_print_cpu.py over the reference's test database, in all three name modes; the scenes made by
    hand of test_hit_list_cpu.py;
  * permuted input gives identical lines in modes 1 and 2, and with a small smax the listing follows the input;
  * masks that are all true, all false and mixed; hits[ s.accept ] after prune;
  * 0, 1, 63, 64 and 65 printed records; 2^17 + 1 rows of a small set repeated, whose duplicates sort by index, whose
    widest name and widest abbreviated field stand only in the second chunk and whose record 2^17 has a column unlike
    record 0's;
  * a listing whose line length is no multiple of 4 and one above 256;
  * the C ABI's refusals with outputs prefilled with sentinels, and a good call afterwards.

torch is imported before the product library: one HIP runtime serves the process."""
import ctypes
import re

import torch  # noqa: F401  (first: its HIP runtime is the process's)

import numpy as np
import pytest

import rnamotif_amd as R
from test_hit_list_cpu import ENTRY, FLAGS, NAMES, SCENES, columns, host_list, list_checker, long_descr, recs_of, rmfmt, tools  # noqa: F401
from test_hit_print import CHUNK, DEV, Case, _open, _written, fasta, trna  # noqa: F401
from test_hit_print_cpu import CASES
from test_hit_structures_cpu import HDR

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

MODES = ("whole", "locus", "acc")


def _host(checker, tmp, c, hits, s, accept="scores", **kw):
    acc = s.accept.cpu().numpy() if isinstance(accept, str) else accept
    return host_list(checker, tmp, c.d, c.seqs, hits.cpu().numpy(), c.sids, c.sdefs, s.text_len.cpu().numpy(), s.text_bytes.cpu().numpy(),
                     accept=acc, **kw)


def _same(hl, want, what=""):
    torch.cuda.synchronize()
    m, L = len(want["perm"]), want["L"]
    assert hl.lines.dtype == torch.uint8 and hl.perm.dtype == torch.int64 and tuple(hl.lines.shape) == (m, L) and tuple(hl.perm.shape) == (m,), what
    assert hl.mode == want["mode"] and list(hl.widths) == list(want["widths"]), what
    assert np.array_equal(hl.perm.cpu().numpy(), want["perm"]), what
    assert hl.lines.cpu().numpy().tobytes() == want["lines"], what


def _is_rmfmts(c, hits, s, hl, flags, tmp, **kw):
    """the listing written is what the tools make of the records printed"""
    printed = _written(c.sc.print_hits(c.db, hits, s, names=c.names, **kw), tmp / "printed.out")
    mine = _written(hl, tmp / "listed.out")
    for tool in tools():
        assert mine == rmfmt(tool, printed, flags), (tool, flags)


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases(built, list_checker, fasta, workdir, tmp_path, name):
    c = Case(name, fasta, workdir)
    s = c.sc.score(c.db, c.hits, c.prog, text=True)
    for nm, flags in enumerate(FLAGS):
        hl = c.sc.list_hits(c.db, c.hits, s, names=c.names, name=MODES[nm])
        _same(hl, _host(list_checker, tmp_path, c, c.hits, s, name_mode=nm), (name, nm))
        assert hl.mode == (2 if name == "trna.efn" else 1) and int(hl.lines.shape[0]) == int(s.accept.sum()) >= 1
        _is_rmfmts(c, c.hits, s, hl, flags, tmp_path)
    assert hl.line(0) == hl.lines[0].cpu().numpy().tobytes() and hl.line(0).endswith(b"\n") and hl.header.startswith(b"#RM scored\n")
    c.close()


class Hand:
    """A database of the entries made by hand and their names"""

    def __init__(self, d):
        self.d = d
        self.seqs, self.sids, self.sdefs = [ENTRY] * len(NAMES), NAMES, [b"", b"a definition"] * 3
        self.sc, self.db, _ = _open(d, self.seqs)
        self.names = R.EntryNames(self.sc, self.db, self.sids, self.sdefs)

    def scores(self, cols, accept=None):
        text_len, text_bytes = columns(cols)
        n = len(cols)
        acc = np.ones(n, dtype=bool) if accept is None else np.asarray(accept, dtype=bool)
        return R.HitScores(torch.from_numpy(acc).to(DEV), torch.zeros(n, dtype=torch.float64, device=DEV), torch.full((n,), 3, dtype=torch.int8, device=DEV),
                           torch.from_numpy(text_bytes).to(DEV), torch.from_numpy(text_len).to(DEV))

    def close(self):
        self.names.close()
        self.db.close()
        self.sc.close()


@pytest.fixture(scope="module")
def hand(built, long_descr):
    h = Hand(long_descr)
    yield h
    h.close()


@pytest.mark.parametrize("key", sorted(SCENES))
def test_scenes(list_checker, hand, tmp_path, key):
    rows, cols = SCENES[key]
    hits = torch.from_numpy(recs_of(hand.d, rows)).to(DEV)
    s = hand.scores(cols)
    for nm, flags in enumerate(FLAGS):
        hl = hand.sc.list_hits(hand.db, hits, s, names=hand.names, name=MODES[nm])
        _same(hl, _host(list_checker, tmp_path, hand, hits, s, name_mode=nm), (key, nm))
        if key != "25 digits":          # (bin/rmfmt's doubles: test_hit_list_cpu.py)
            _is_rmfmts(hand, hits, s, hl, flags, tmp_path)


def test_permuted_input_and_smax(built, list_checker, fasta, workdir, trna, tmp_path):
    plain = Case("pk1", fasta, workdir)
    for c, mode in ((plain, 1), (trna, 2)):
        hits = c.hits[:600].contiguous()
        n = int(hits.shape[0])
        s = c.sc.score(c.db, hits, c.prog, text=True)
        base = c.sc.list_hits(c.db, hits, s, names=c.names)
        assert base.mode == mode and int(base.lines.shape[0]) > 8
        perm = torch.from_numpy(np.random.default_rng(9).permutation(n)).to(DEV)
        rows = hits[perm].contiguous()
        t = c.sc.score(c.db, rows, c.prog, text=True)
        moved = c.sc.list_hits(c.db, rows, t, names=c.names)
        _same(moved, _host(list_checker, tmp_path, c, rows, t), "permuted")
        assert torch.equal(moved.lines, base.lines) and not torch.equal(moved.perm, base.perm)
        # more temp bytes than smax: the input's order
        small = c.sc.list_hits(c.db, rows, t, names=c.names, smax=100)
        _same(small, _host(list_checker, tmp_path, c, rows, t, smax=100), "smax")
        assert small.mode == 0 and torch.equal(small.perm, torch.nonzero(t.accept).flatten()) and not torch.equal(small.lines, base.lines)
        _is_rmfmts(c, rows, t, small, ["-smax", "100"], tmp_path)
    plain.close()


def test_masks_and_after_prune(built, list_checker, trna, tmp_path):
    c = trna
    rows = c.hits[:300].contiguous()
    m = int(rows.shape[0])
    s = c.sc.score(c.db, rows, c.prog, text=True)
    rng = np.random.default_rng(5)
    for what, mask in (("all", np.ones(m, dtype=bool)), ("none", np.zeros(m, dtype=bool)), ("mixed", rng.random(m) < 0.4)):
        # (a rejected record has an empty column: the masks pick among the accepted ones)
        mask = mask & s.accept.cpu().numpy() if what != "none" else mask
        t = R.HitScores(torch.from_numpy(mask).to(DEV), s.score, s.kind, s.text_bytes, s.text_len)
        hl = c.sc.list_hits(c.db, rows, t, names=c.names, name="locus")
        _same(hl, _host(list_checker, tmp_path, c, rows, t, accept=mask, name_mode=1), what)
        assert int(hl.lines.shape[0]) == int(mask.sum())
        if what == "none":
            # nothing listed writes nothing, not even the header, as rmfmt of empty input does
            assert hl.lines.numel() == 0 and _written(hl, tmp_path / "none.out") == b""
        else:
            _is_rmfmts(c, rows, t, hl, ["-l"], tmp_path)
    # the chain: score, prune what is accepted, list what is kept
    acc = c.hits[c.sc.score(c.db, c.hits, c.prog, text=True).accept].contiguous()
    kept = acc[c.sc.prune(c.db, acc)].contiguous()
    assert 0 < int(kept.shape[0]) <= int(acc.shape[0])
    t = c.sc.score(c.db, kept, c.prog, text=True)
    assert bool(t.accept.all())
    hl = c.sc.list_hits(c.db, kept, t, names=c.names)
    _same(hl, _host(list_checker, tmp_path, c, kept, t), "pruned")
    _is_rmfmts(c, kept, t, hl, [], tmp_path)


def test_counts(built, list_checker, hand, tmp_path):
    rows = [(h % 5, h % 2, h % 7, (3, 2, 3)) for h in range(70)]
    cols = [b"%8.3f" % (h % 11) for h in range(70)]
    for n, printed in ((0, 0), (1, 1), (1, 0), (70, 63), (70, 64), (70, 65)):
        hits = torch.from_numpy(recs_of(hand.d, rows[:n])).to(DEV)
        accept = np.arange(n) < printed if n > 1 else np.ones(n, dtype=bool) * printed
        s = hand.scores(cols[:n], accept) if n else R.HitScores(*(torch.zeros(sh, dtype=t, device=DEV) for sh, t in
                                                                   (((0,), torch.bool), ((0,), torch.float64), ((0,), torch.int8), ((0, 8), torch.uint8), ((0,), torch.int32))))
        hl = hand.sc.list_hits(hand.db, hits, s, names=hand.names)
        _same(hl, _host(list_checker, tmp_path, hand, hits, s, accept=np.asarray(accept, dtype=bool)), (n, printed))
        assert int(hl.lines.shape[0]) == printed
    # 2^17 + 1 rows: a small set repeated, then one record of the entry with the widest name, with an element of 100
    # letters and a column of its own
    small = recs_of(hand.d, rows[:5])
    last = recs_of(hand.d, [(5, 1, 9, (100, 2, 3))])
    many = np.concatenate([small[np.arange(CHUNK) % 5], last])
    cols = [b"   1.000", b"   2.500", b"   1.000", b"  -4.000", b"   2.500"]
    text_len, text_bytes = columns([cols[h % 5] for h in range(8)] + [b"  77.125"])
    idx = np.concatenate([np.arange(CHUNK) % 5, [8]])
    s = R.HitScores(torch.ones(CHUNK + 1, dtype=torch.bool, device=DEV), torch.zeros(CHUNK + 1, dtype=torch.float64, device=DEV),
                    torch.full((CHUNK + 1,), 3, dtype=torch.int8, device=DEV), torch.from_numpy(text_bytes[idx]).to(DEV), torch.from_numpy(text_len[idx]).to(DEV))
    hits = torch.from_numpy(many).to(DEV)
    hl = hand.sc.list_hits(hand.db, hits, s, names=hand.names)
    want = _host(list_checker, tmp_path, hand, hits, s)
    _same(hl, want, "2^17 + 1")
    perm = hl.perm.cpu().numpy()
    # (the score block is as wide as the widest token, 6 bytes: the column's own padding is split away)
    assert perm[0] == CHUNK and hl.line(0).startswith(NAMES[5] + b" 77.125 1 ") and b"...(100)..." in hl.line(0)
    assert hl.widths[0] == 40 and hl.widths[5] == 17 and hl.mode == 1
    # the duplicates: each of the five records' lines in one run, by index
    rest = perm[1:]
    same = rest[1:] % 5 == rest[:-1] % 5
    assert (np.diff(rest)[same] == 5).all() and int((~same).sum()) == 4 and sorted(rest[np.r_[True, ~same]]) == [0, 1, 2, 3, 4]
    first = hand.sc.list_hits(hand.db, hits[:CHUNK], R.HitScores(s.accept[:CHUNK], s.score[:CHUNK], s.kind[:CHUNK], s.text_bytes[:CHUNK], s.text_len[:CHUNK]),
                              names=hand.names)
    assert first.widths[0] < 40 and first.widths[5] == 3 and int(first.lines.shape[1]) < int(hl.lines.shape[1])


def test_line_lengths(built, list_checker, trna, tmp_path):
    c = trna
    hits = c.hits[:200].contiguous()
    s = c.sc.score(c.db, hits, c.prog, text=True)
    seen = set()
    for k in (1, 2, 3, 4, 300):
        names = R.EntryNames(c.sc, c.db, [b"s" * k] * len(c.sids), c.sdefs)
        hl = c.sc.list_hits(c.db, hits, s, names=names)
        want = host_list(list_checker, tmp_path, c.d, c.seqs, hits.cpu().numpy(), [b"s" * k] * len(c.sids), c.sdefs, s.text_len.cpu().numpy(),
                         s.text_bytes.cpu().numpy(), accept=s.accept.cpu().numpy())
        _same(hl, want, k)
        seen.add(int(hl.lines.shape[1]))
        names.close()
    assert len(seen) == 5 and any(L % 4 for L in seen) and max(seen) > 256


def test_c_abi_refusals(built, list_checker, fasta, workdir, trna, tmp_path):
    c = trna
    sc, db = c.sc, c.db
    hits = c.hits[:500].contiguous()
    n = int(hits.shape[0])
    s = sc.score(db, hits, c.prog, text=True)
    good = sc.list_hits(db, hits, s, names=c.names)
    torch.cuda.synchronize()
    m, ll, width = int(good.lines.shape[0]), int(good.lines.shape[1]), int(s.text_bytes.shape[1])
    assert m > 8
    L = R.lib()
    buf = ctypes.create_string_buffer(1024)

    def call(rows=hits, text_bytes=s.text_bytes, text_len=s.text_len, n_lines=m, line_len=ll, dbh=db._h, names=c.names._h):
        out = (torch.full(((m + 1) * (ll + 1) + 64,), 77, dtype=torch.uint8, device=DEV), torch.full((m + 9,), -77, dtype=torch.int64, device=DEV))
        torch.cuda.synchronize()
        rc = L.rma_hit_list(sc._h, dbh, names, rows.data_ptr(), n, s.accept.data_ptr(), text_bytes.data_ptr(), width, text_len.data_ptr(), 0, 0, None,
                            n_lines, line_len, out[0].data_ptr(), out[1].data_ptr(), None, buf, 1024)
        torch.cuda.synchronize()
        return rc, out

    def untouched(out):
        return bool((out[0] == 77).all()) and bool((out[1] == -77).all())

    def shape(rows=hits, text_bytes=s.text_bytes, text_len=s.text_len):
        got = (ctypes.c_int64(-1), ctypes.c_int64(-1), np.full(107, -1, dtype=np.int32), ctypes.c_int32(-1))
        rc = L.rma_hit_list_shape(sc._h, db._h, c.names._h, rows.data_ptr(), n, s.accept.data_ptr(), text_bytes.data_ptr(), width, text_len.data_ptr(), 0, 0,
                                  ctypes.byref(got[0]), ctypes.byref(got[1]), got[2].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(got[3]),
                                  None, buf, 1024)
        return rc, got

    rc, out = call()
    assert rc == 0 and torch.equal(out[0][:m * ll].reshape(m, ll), good.lines) and torch.equal(out[1][:m], good.perm)
    assert bool((out[0][m * ll:] == 77).all()) and bool((out[1][m:] == -77).all())
    rc, got = shape()
    assert rc == 0 and (got[0].value, got[1].value, got[3].value) == (m, ll, good.mode) and list(got[2][:len(good.widths)]) == list(good.widths)

    def refused(words, **kw):
        rc, out = call(**kw)
        assert rc == 1 and re.search(words, buf.value.decode()) and untouched(out), buf.value
        if not ({"n_lines", "line_len", "dbh", "names"} & set(kw)):
            rc, got = shape(**kw)
            assert rc == 1 and re.search(words, buf.value.decode()) and got[0].value == -1 and (got[2] == -1).all(), buf.value

    # a forged record
    first = int(torch.nonzero(s.accept)[0])
    bad = hits.clone()
    bad[3, 1] = 2
    refused("record 3: strand 2, not 0 or 1: nothing listed", rows=bad)
    slen0 = len(c.seqs[int(hits[1, 0])])
    bad = hits.clone()
    bad[1, HDR + 4 * 4] = slen0 + 1
    refused("record 1: element 4 at offset %d, length .* outside entry" % (slen0 + 1), rows=bad)
    with pytest.raises(R.RnamotifError, match="record 1: element 4"):
        sc.list_hits(db, bad, s, names=c.names)
    # records whose numbers of score fields differ: one column loses its second field
    later = int(torch.nonzero(s.accept)[5])
    cols = s.text_bytes.clone()
    cols[later, 9:] = ord(" ")
    refused(r"records %d and %d: 2 and 1 score fields: .*n_sfields.*does not restate it: nothing listed" % (first, later), text_bytes=cols)
    # a text_len outside its row
    lens = s.text_len.clone()
    lens[7], lens[300] = width + 1, width + 1
    refused(r"record 7: a score column of %d bytes, outside the \[0, %d\] of text_width: nothing listed" % (width + 1, width), text_len=lens)
    # a shape that is not the listing's
    for kw in ({"n_lines": m - 1}, {"line_len": ll + 1}, {"line_len": ll - 1}):
        refused(r"has %d lines of %d bytes, not the %d lines of %d bytes given: nothing listed" % (m, ll, kw.get("n_lines", m), kw.get("line_len", ll)), **kw)
    # another database's names, a host database
    sc2, db2, _ = _open(c.d, c.seqs[:50])
    other = R.EntryNames(sc, db2)
    refused("names were made for another database", names=other._h)
    other.close()
    db2.close()
    sc2.close()
    host = sc.database(c.seqs)
    refused(r"not made by rma_db_create_device\(\) or has been destroyed", dbh=host._h)
    with pytest.raises(ValueError, match="not made by database_from_tensor"):
        sc.list_hits(host, hits, s, names=c.names)
    host.close()
    # what the host knows when the call is made: a name with a blank in it, letters that are blanks
    blank = R.EntryNames(sc, db, [b"a b"] + c.sids[1:], c.sdefs)
    refused("entry 0: its name is empty, trims to nothing or has a blank", names=blank._h)
    blank.close()
    with pytest.raises(R.RnamotifError, match="the letters map byte 103 to a blank, a tab or a newline"):
        sc.list_hits(db, hits, s, names=c.names, letters=bytes(32 if b == 103 else 110 for b in range(256)))
    with pytest.raises(ValueError, match="name: 'whole', 'locus' or 'acc'"):
        sc.list_hits(db, hits, s, names=c.names, name="-l")
    # a good call still gives the same bytes
    again = sc.list_hits(db, hits, s, names=c.names)
    assert torch.equal(again.lines, good.lines) and torch.equal(again.perm, good.perm) and again.mode == good.mode == 2
