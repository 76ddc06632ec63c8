"""GPU: hit records as rnamotif prints them, on the device (Scanner.print_hits, EntryNames, rma_hit_print_size,
rma_hit_print: the size and fill kernels of rm_hitprint_dev.hip) against the same rule, rm_hitprint.h, run on the host
through tests/hostsim/hit_print_check.cpp -- byte for byte in bytes and offsets -- and against the file Replay.device()
writes for the same records and names:

  * the cases of test_hit_print_cpu.py over the reference's test database, scanned, scored and printed on the device;
  * rows in a permuted order and repeated, accepted_only with masks that are all true, all false and mixed;
  * 0, 1 and 2^17 + 1 rows: the offsets run on over the chunks;
  * a database made from FASTA text prints the file's own names with names=None; tokens with alphabet= and an explicit
    letters table agree with Replay.device() on the same arguments;
  * refusals with their words, the outputs left as they were; nothing printed writes nothing, not even the header.

torch is imported before the product library: one HIP runtime serves the process."""
import ctypes
import os
import re

import torch  # noqa: F401  (first: its HIP runtime is the process's)

import numpy as np
import pytest

import rnamotif_amd as R
from test_hit_align_cpu import DOT
from test_hit_print_cpu import CASES, host_print, print_checker  # noqa: F401
from test_hit_structures_cpu import GOLDEN, HDR

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

DEV = torch.device("cuda", 0)
CHUNK = 1 << 17


def _descr(argv, cwd=None):
    old = os.getcwd()
    os.chdir(cwd or old)
    try:
        return R.Descriptor(argv)
    finally:
        os.chdir(old)


def _open(d, seqs, lead=3):
    sc = R.Scanner(d, device=0)
    flat = b"x" * lead + b"".join(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64) + lead
    text = torch.frombuffer(bytearray(flat), dtype=torch.uint8).to(DEV)
    db = sc.database_from_tensor(text, offsets=off)
    return sc, db, sc.scan_tensor(db)


def _replay_file(d, db, hits, path, sids=None, sdefs=None, letters=None):
    """What Replay.device() writes for these records and names, and its mask of the records printed."""
    rp = R.Replay(d, str(path))
    _, mask = rp.device(db, hits, sids, sdefs, letters=letters, accepted=True)
    rp.close()
    return open(str(path), "rb").read(), mask


def _written(p, path, header=True):
    with open(str(path), "wb") as f:
        n = p.write(f, header=header)
    data = open(str(path), "rb").read()
    assert n == len(data)
    return data


def _same(p, off, data, what=""):
    torch.cuda.synchronize()
    assert p.off.dtype == torch.int64 and p.bytes.dtype == torch.uint8, what
    assert np.array_equal(p.off.cpu().numpy(), off), what
    assert p.bytes.cpu().numpy().tobytes() == data, what


@pytest.fixture(scope="module")
def fasta(gbrna):
    return R.read_fasta(gbrna)


class Case:
    def __init__(self, name, fasta, workdir):
        argv, limit, _ = CASES[name]
        if name == "dot":
            with open(os.path.join(workdir, "dot.descr"), "w") as f:
                f.write(DOT)
        self.d = _descr(argv, cwd=workdir)
        rows = fasta[:limit]
        self.sids, self.sdefs, self.seqs = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
        self.sc, self.db, self.hits = _open(self.d, self.seqs)
        self.prog = R.ScoreProgram(self.d, text=True)
        self.names = R.EntryNames(self.sc, self.db, self.sids, self.sdefs)

    def host(self, checker, tmp, hits, s, accept="scores"):
        acc = s.accept.cpu().numpy() if isinstance(accept, str) else accept
        return host_print(checker, tmp, self.d, self.seqs, hits.cpu().numpy(), self.sids, self.sdefs, s.text_len.cpu().numpy(),
                          s.text_bytes.cpu().numpy(), accept=acc)

    def close(self):
        self.names.close()
        self.prog.close()
        self.db.close()
        self.sc.close()


@pytest.fixture(scope="module")
def trna(fasta, workdir):
    """trna with its score section (trna.efn.descr: SCORE = sprintf( '%8.3f %8.3f', bits(...), efn(...) )): a string
    column made on the device that differs from record to record, so that a row of text_bytes taken for another shows."""
    c = Case("trna.efn", fasta, workdir)
    s = c.sc.score(c.db, c.hits, c.prog, text=True)
    torch.cuda.synchronize()
    rows = s.text_bytes[s.accept].cpu().numpy()
    assert int((s.kind[s.accept] == 3).all()) and len({r.tobytes() for r in rows}) > rows.shape[0] // 2
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases(built, print_checker, fasta, workdir, tmp_path, name):
    c = Case(name, fasta, workdir)
    n = int(c.hits.shape[0])
    assert n >= 1
    s = c.sc.score(c.db, c.hits, c.prog, text=True)
    p = c.sc.print_hits(c.db, c.hits, s, names=c.names)
    off, data = c.host(print_checker, tmp_path, c.hits, s)
    _same(p, off, data, name)
    want, mask = _replay_file(c.d, c.db, c.hits, tmp_path / "replay.out", c.sids, c.sdefs)
    assert np.array_equal(mask, s.accept.cpu().numpy()) and mask.any()
    if CASES[name][2] is not None:
        assert int(mask.sum()) == CASES[name][2]
    assert p.header + data == want
    assert _written(p, tmp_path / "device.out") == want
    assert _written(p, tmp_path / "bare.out", header=False) == data
    first = int(np.flatnonzero(mask)[0])
    assert p.record(first) == data[off[first]:off[first + 1]] and p.record(first).startswith(b">")
    if not mask.all():
        assert p.record(int(np.flatnonzero(~mask)[0])) == b""
    # every record, the rejected ones with the empty column they have
    every = c.sc.print_hits(c.db, c.hits, s, names=c.names, accepted_only=False)
    _same(every, *c.host(print_checker, tmp_path, c.hits, s, accept=None), name)
    assert bool((every.off[1:] > every.off[:-1]).all())
    c.close()


def test_orders_and_masks(built, print_checker, trna, tmp_path):
    c = trna
    n = int(c.hits.shape[0])
    rng = np.random.default_rng(5)
    perm = torch.from_numpy(rng.permutation(n)).to(DEV)
    for what, rows in (("permuted", c.hits[perm]), ("repeated", c.hits[torch.tensor([2, 2, 0, n - 1, 2, n - 1, 2], device=DEV)])):
        s = c.sc.score(c.db, rows, c.prog, text=True)
        p = c.sc.print_hits(c.db, rows, s, names=c.names)
        off, data = c.host(print_checker, tmp_path, rows, s)
        _same(p, off, data, what)
        want, _ = _replay_file(c.d, c.db, rows, tmp_path / (what + ".out"), c.sids, c.sdefs)
        assert p.header + data == want
    rows = c.hits[perm][:300].contiguous()
    m = int(rows.shape[0])
    s = c.sc.score(c.db, rows, c.prog, text=True)
    for what, mask in (("all", np.ones(m, dtype=bool)), ("none", np.zeros(m, dtype=bool)), ("mixed", rng.random(m) < 0.4)):
        t = R.HitScores(torch.from_numpy(mask).to(DEV), s.score, s.kind, s.text_bytes, s.text_len)
        p = c.sc.print_hits(c.db, rows, t, names=c.names)
        _same(p, *c.host(print_checker, tmp_path, rows, t, accept=mask), what)
        width = (p.off[1:] - p.off[:-1]).cpu().numpy()
        assert ((width == 0) == ~mask).all(), what
        if what == "none":
            # nothing printed writes nothing, not even the header, as rnamotif does without a hit
            assert p.bytes.numel() == 0 and _written(p, tmp_path / "none.out") == b"" and p.header.startswith(b"#RM scored\n")


def test_edge_counts(built, print_checker, trna, tmp_path):
    c = trna
    for n in (0, 1):
        rows = c.hits[:n].contiguous()
        s = c.sc.score(c.db, rows, c.prog, text=True)
        p = c.sc.print_hits(c.db, rows, s, names=c.names, accepted_only=False)
        _same(p, *c.host(print_checker, tmp_path, rows, s, accept=None), n)
        assert tuple(p.off.shape) == (n + 1,) and int(p.off[0]) == 0 and (p.bytes.numel() > 0) == (n == 1)
    # 2^17 + 1 rows of a small record set: the second chunk's offsets run on from the first's
    # (ordered so that record 0 and record 2^17, the first of the second chunk, are printed and have different score
    # columns: a column read from the chunk's row instead of the call's would print record 2^17 with record 0's)
    base = c.hits[:1000].contiguous()
    m = int(base.shape[0])
    sb = c.sc.score(c.db, base, c.prog, text=True)
    acc, cols = sb.accept.cpu().numpy(), sb.text_bytes.cpu().numpy()
    a = int(np.flatnonzero(acc)[0])
    b = int(np.flatnonzero(acc & (cols != cols[a]).any(axis=1))[0])
    k = CHUNK % m
    assert m == 1000 and k not in (0, a)
    order = np.arange(m)
    order[[0, a]] = order[[a, 0]]
    at = int(np.flatnonzero(order == b)[0])
    order[[k, at]] = order[[at, k]]
    small = base[torch.from_numpy(order).to(DEV)].contiguous()
    idx = torch.arange(CHUNK + 1, device=DEV) % m
    many = small[idx]
    s = c.sc.score(c.db, many, c.prog, text=True)
    assert bool(s.accept[0]) and bool(s.accept[CHUNK]) and not torch.equal(s.text_bytes[CHUNK], s.text_bytes[0])
    big = c.sc.print_hits(c.db, many, s, names=c.names)
    one = c.sc.print_hits(c.db, small, c.sc.score(c.db, small, c.prog, text=True), names=c.names)
    torch.cuda.synchronize()
    lens = one.off[1:] - one.off[:-1]
    assert int((lens > 0).sum()) > 8
    want_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=DEV), torch.cumsum(lens[idx], 0)])
    assert torch.equal(big.off, want_off)
    total, reps = int(one.off[-1]), (CHUNK + 1) // m
    assert big.bytes.numel() == int(want_off[-1]) and reps * m <= CHUNK
    assert torch.equal(big.bytes[:reps * total].reshape(reps, total), one.bytes[None, :].expand(reps, total))
    tail = CHUNK + 1 - reps * m
    assert tail == k + 1 and torch.equal(big.bytes[reps * total:], one.bytes[:int(one.off[tail])])
    # a second chunk of a thousand records, each with its own column: the set once more, rotated by k
    idx2 = torch.arange(CHUNK + m, device=DEV) % m
    s2 = c.sc.score(c.db, small[idx2], c.prog, text=True)
    big2 = c.sc.print_hits(c.db, small[idx2], s2, names=c.names)
    torch.cuda.synchronize()
    assert int(big2.off[CHUNK]) == int(want_off[CHUNK]) and torch.equal(big2.bytes[:int(big2.off[CHUNK])], big.bytes[:int(big.off[CHUNK])])
    cut = int(one.off[k])
    assert torch.equal(big2.bytes[int(big2.off[CHUNK]):], torch.cat([one.bytes[cut:], one.bytes[:cut]]))
    last = big.record(CHUNK)
    column = bytes(s.text_bytes[CHUNK, :int(s.text_len[CHUNK])].cpu().numpy().tobytes())
    assert last == one.record(k) and last != one.record(0) and (b" " + column + b" ") in last and column == cols[b][:len(column)].tobytes()


def test_fasta_database_prints_its_own_names(built, fasta, workdir, tmp_path):
    d = _descr(CASES["pk1"][0], cwd=workdir)
    rows = fasta[:400]
    text = b"".join(b">" + sid + (b" " + sdef if sdef else b"") + b"\n" + seq + b"\n" for sid, sdef, seq in rows)
    sc = R.Scanner(d, device=0)
    db = sc.database_from_fasta_tensor(torch.frombuffer(bytearray(text), dtype=torch.uint8).to(DEV))
    assert db.sids == [r[0] for r in rows] and any(db.sdefs)
    hits = sc.scan_tensor(db)
    prog = R.ScoreProgram(d, text=True)
    s = sc.score(db, hits, prog, text=True)
    p = sc.print_hits(db, hits, s)
    want, mask = _replay_file(d, db, hits, tmp_path / "replay.out", db.sids, db.sdefs)
    assert mask.any() and _written(p, tmp_path / "device.out") == want
    # ... and the entries' numbers where the caller asks for names of its own
    own = R.EntryNames(sc, db, sids=[b"%d" % i for i in range(db.n_seqs)], sdefs=[b""] * db.n_seqs)
    q = sc.print_hits(db, hits, s, names=own)
    plain, _ = _replay_file(d, db, hits, tmp_path / "plain.out")
    assert _written(q, tmp_path / "numbers.out") == plain and plain != want
    own.close()
    # one missing name among given ones is that entry's own, as a missing list is every entry's
    first = int(np.flatnonzero(mask)[0])
    e = int(hits[first, 0])
    some = R.EntryNames(sc, db, sids=[None if i == e else b"x" for i in range(db.n_seqs)], sdefs=[None if i == e else b"y" for i in range(db.n_seqs)])
    assert sc.print_hits(db, hits, s, names=some).record(first) == p.record(first)
    assert p.record(first).startswith(b">" + db.sids[e] + b" " + db.sdefs[e] + b"\n")
    some.close()
    # the default table is kept with the database: the same one serves the next call, and goes with the database
    kept = db._default_names
    assert sc.print_hits(db, hits, s).record(first) == p.record(first) and db._default_names is kept and kept._h
    prog.close()
    db.close()
    assert not kept._h
    sc.close()


def test_tokens_with_an_alphabet(built, fasta, workdir, tmp_path):
    d = _descr(CASES["trna"][0], cwd=workdir)
    seqs = [r[2] for r in fasta[:300]]
    width, lens = max(len(s) for s in seqs), [len(s) for s in seqs]
    letters = np.full((len(seqs), width + 13), ord("g"), dtype=np.uint8)
    for i, s in enumerate(seqs):
        letters[i, 5:5 + len(s)] = np.frombuffer(s, dtype=np.uint8)
    lut = np.full(256, 4, dtype=np.uint8)
    lut[np.frombuffer(b"acgt", dtype=np.uint8)] = np.arange(4, dtype=np.uint8)
    tokens = torch.from_numpy(lut[letters]).to(DEV)[:, 5:5 + width]     # rows at a stride of width + 13
    sc = R.Scanner(d, device=0)
    db = sc.database_from_tensor(tokens, lengths=lens, alphabet="acgu")
    hits = sc.scan_tensor(db)
    prog = R.ScoreProgram(d, text=True)
    # names=None on a database without names: the entry's number, no definition, as Replay.device() has them
    want, mask = _replay_file(d, db, hits, tmp_path / "replay.out")
    assert mask.any()
    for what, table in (("alphabet", None), ("letters", R.alphabet_letters("acgu"))):
        s = sc.score(db, hits, prog, letters=table, text=True)
        p = sc.print_hits(db, hits, s, letters=table)
        assert _written(p, tmp_path / (what + ".out")) == want, what
    again, _ = _replay_file(d, db, hits, tmp_path / "again.out", letters=R.alphabet_letters("acgu"))
    assert again == want
    # a closed database
    db.close()
    with pytest.raises(ValueError, match="closed"):
        sc.print_hits(db, hits, s)
    with pytest.raises(ValueError, match="closed"):
        R.EntryNames(sc, db)
    prog.close()
    sc.close()


def test_refusals(built, trna, tmp_path):
    c = trna
    sc, db, d = c.sc, c.db, c.d
    hits = c.hits[:500].contiguous()
    n = int(hits.shape[0])
    s = sc.score(db, hits, c.prog, text=True)
    good = sc.print_hits(db, hits, s, names=c.names)
    torch.cuda.synchronize()
    total, width = int(good.bytes.numel()), int(s.text_bytes.shape[1])
    assert total > 0
    with pytest.raises(ValueError, match="no text"):
        sc.print_hits(db, hits, R.HitScores(s.accept, s.score, s.kind), names=c.names)      # (what score() without text=True returns)
    with pytest.raises(TypeError, match="not a HitScores"):
        sc.print_hits(db, hits, None, names=c.names)
    with pytest.raises(ValueError, match="hits is on cpu"):
        sc.print_hits(db, hits.cpu(), s, names=c.names)
    host = sc.database(c.seqs)
    with pytest.raises(ValueError, match="not made by database_from_tensor"):
        sc.print_hits(host, hits, s, names=c.names)
    # names: another database's, a wrong count, a NUL inside, a sid of 2048 bytes
    sc2, db2, _ = _open(d, c.seqs[:50])
    other = R.EntryNames(sc, db2)
    with pytest.raises(R.RnamotifError, match="names were made for another database"):
        sc.print_hits(db, hits, s, names=other)
    other.close()
    with pytest.raises(R.RnamotifError, match="names of %d entries, the database has %d" % (len(c.sids) - 1, len(c.sids))):
        R.EntryNames(sc, db, c.sids[:-1], c.sdefs[:-1])
    with pytest.raises(R.RnamotifError, match="entry 1: its name has a NUL at byte 2 of 5"):
        R.EntryNames(sc, db, [c.sids[0], b"ab\0cd"] + c.sids[2:], c.sdefs)
    with pytest.raises(R.RnamotifError, match="entry 0: its definition has a NUL at byte 0 of 1"):
        R.EntryNames(sc, db, c.sids, [b"\0"] + c.sdefs[1:])
    with pytest.raises(R.RnamotifError, match="entry 2: its name has 2048 bytes"):
        R.EntryNames(sc, db, c.sids[:2] + [b"s" * 2048] + c.sids[3:], c.sdefs)
    with pytest.raises(R.RnamotifError, match="not made by rma_db_create_device"):
        R.EntryNames(sc, host)
    long_names = R.EntryNames(sc, db, [b"s" * 2047] * len(c.sids), c.sdefs)
    p = sc.print_hits(db, hits[:3], sc.score(db, hits[:3], c.prog, text=True), names=long_names, accepted_only=False)
    assert p.record(0).startswith(b">" + b"s" * 2047 + b" ") and (b"\n" + b"s" * 2047 + b" ") in p.record(0)
    long_names.close()

    # the C ABI, outputs prefilled with a sentinel
    L = R.lib()
    buf = ctypes.create_string_buffer(1024)

    def call(rows, text_len, tot, dbh=db._h, names=c.names._h, text_width=width):
        out = (torch.full((total + 64,), 77, dtype=torch.uint8, device=DEV), torch.full((n + 9,), -77, dtype=torch.int64, device=DEV))
        torch.cuda.synchronize()
        rc = L.rma_hit_print(sc._h, dbh, names, rows.data_ptr(), n, None, s.accept.data_ptr(), s.text_bytes.data_ptr(), text_width,
                             text_len.data_ptr(), tot, out[0].data_ptr(), out[1].data_ptr(), None, buf, 1024)
        torch.cuda.synchronize()
        return rc, out

    def untouched(out):
        return bool((out[0] == 77).all()) and bool((out[1] == -77).all())

    rc, out = call(hits, s.text_len, total)
    assert rc == 0 and torch.equal(out[0][:total], good.bytes) and torch.equal(out[1][:n + 1], good.off)
    assert bool((out[0][total:] == 77).all()) and bool((out[1][n + 1:] == -77).all())
    size = ctypes.c_int64(-1)
    rc = L.rma_hit_print_size(sc._h, db._h, c.names._h, hits.data_ptr(), n, s.accept.data_ptr(), s.text_len.data_ptr(), ctypes.byref(size), None, buf, 1024)
    assert rc == 0 and size.value == total
    slen0 = len(c.seqs[int(hits[1, 0])])
    forged = [(2, 0, len(c.seqs), r"record 2: entry %d outside \[0, %d\)" % (len(c.seqs), len(c.seqs))),
              (3, 1, 2, "record 3: strand 2, not 0 or 1"),
              (1, HDR + 4 * 4, slen0 + 1, "record 1: element 4 at offset %d, length .* outside entry" % (slen0 + 1))]
    for row, col, value, words in forged:
        bad = hits.clone()
        bad[row, col] = value
        rc, out = call(bad, s.text_len, total)
        assert rc == 1 and re.search(words, buf.value.decode()) and "nothing printed" in buf.value.decode(), buf.value
        assert untouched(out), words
        rc = L.rma_hit_print_size(sc._h, db._h, c.names._h, bad.data_ptr(), n, None, s.text_len.data_ptr(), ctypes.byref(size), None, buf, 1024)
        assert rc == 1 and re.search(words, buf.value.decode()) and size.value == 0
        with pytest.raises(R.RnamotifError, match=words):
            sc.print_hits(db, bad, s, names=c.names)
    # a text_len above text_width (and below 0), the lowest such record named
    for value in (width + 1, -1):
        lens = s.text_len.clone()
        lens[7], lens[300] = value, value
        rc, out = call(hits, lens, total)
        words = r"record 7: a score column of %d bytes, outside the \[0, %d\] of text_width: nothing printed" % (value, width)
        assert rc == 1 and re.search(words, buf.value.decode()) and untouched(out), buf.value
        # (through print_hits the size call, which knows no row width, meets a negative length first)
        with pytest.raises(R.RnamotifError, match=words if value > 0 else "record 7: a score column of -1 bytes: nothing printed"):
            sc.print_hits(db, hits, R.HitScores(s.accept, s.score, s.kind, s.text_bytes, lens), names=c.names)
    # a total that is not the size call's
    for tot in (total - 1, total + 1):
        rc, out = call(hits, s.text_len, tot)
        assert rc == 1 and ("have %d bytes, not the %d of `total`: nothing printed" % (total, tot)) in buf.value.decode() and untouched(out), buf.value
    # databases the replay refuses, names of another database
    for h in (host._h,):
        rc, out = call(hits, s.text_len, total, dbh=h)
        assert rc == 1 and b"not made by rma_db_create_device() or has been destroyed" in buf.value and untouched(out)
    other = R.EntryNames(sc, db2)
    rc, out = call(hits, s.text_len, total, names=other._h)
    assert rc == 1 and b"names were made for another database" in buf.value and untouched(out)
    other.close()
    db2.close()
    sc2.close()
    host.close()
    # a good call still works
    again = sc.print_hits(db, hits, s, names=c.names)
    assert torch.equal(again.bytes, good.bytes) and torch.equal(again.off, good.off)
