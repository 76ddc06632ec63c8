"""GPU: hit records laid into the columns of an alignment on the device (Scanner.align, rma_hit_alignment_shape,
rma_hit_alignment: the widths and fill kernels of rm_hitalign_dev.hip) against the same rule, rm_hitalign.h, run on the
host through tests/hostsim/hit_align_check.cpp -- byte for byte in rows, pos and widths:

  * 0, 1, 63, 64, 65 and 257 records, the wave and workgroup edges of both kernels; both strands, the strand 1 hits
    of entries with upper case, u and non-letters;
  * rows shorter than, as long as and longer than two lane passes of 64, so that a pass straddles columns and the
    row's end; a descriptor of more elements than one register per lane holds, with a '.' field;
  * letters= from alphabet=, contexts, all three fill bytes changed, pos=True and pos=False, rows in reversed and in
    repeated order, given widths;
  * 2^17 + 1 rows, the one record with the widest element last: the widths are over all chunks;
  * al.pos against hit_structures' tensors;
  * refusals with their words, nothing written; stream order without a synchronisation.

torch is imported before the product library: one HIP runtime serves the process."""
import ctypes
import os
import re

import torch  # noqa: F401  (first: its HIP runtime is the process's)

import numpy as np
import pytest

import pins
import rnamotif_amd as R
from test_hit_align_cpu import align_checker, host_alignment  # noqa: F401
from test_hit_structures_cpu import GOLDEN, HDR
from test_hit_windows_cpu import normalise, odd_entries

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

DEV = torch.device("cuda", 0)
CHUNK = 1 << 17


@pytest.fixture(scope="module")
def gb(gbrna):
    return [r[2] for r in R.read_fasta(gbrna)]


def _descr(argv, cwd=None):
    old = os.getcwd()
    os.chdir(cwd or old)
    try:
        return R.Descriptor(argv)
    finally:
        os.chdir(old)


def _golden(name):
    return _descr(["-descr", os.path.join(GOLDEN, "descr", name + ".descr")])


def _own(tmp_path, name, text):
    path = tmp_path / (name + ".descr")
    path.write_text(text)
    return _descr(["-descr", str(path)])


def _open(d, seqs, lead=3):
    sc = R.Scanner(d, device=0)
    flat = b"x" * lead + b"".join(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64) + lead
    text = torch.frombuffer(bytearray(flat), dtype=torch.uint8).to(DEV)
    db = sc.database_from_tensor(text, offsets=off)
    return sc, db, sc.scan_tensor(db)


def _strand(raw, comp):
    s = normalise(raw)
    if comp:
        s = s[::-1].translate(bytes.maketrans(b"acgt", b"tgca"))
        s = bytes(b if b in b"acgt" else ord("n") for b in s)
    return s


def _same(al, want, what=""):
    torch.cuda.synchronize()
    rows = al.rows.cpu().numpy()
    assert np.array_equal(al.widths, want["widths"]), (what, al.widths, want["widths"])
    assert al.widths.dtype == np.int32 and np.array_equal(al.right, want["right"]), what
    assert rows.dtype == np.uint8 and rows.shape == want["rows"].shape, (what, rows.shape, want["rows"].shape)
    assert np.array_equal(rows, want["rows"]), what
    if al.pos is not None:
        pos = al.pos.cpu().numpy()
        assert pos.dtype == np.int32 and pos.shape == want["pos"].shape and np.array_equal(pos, want["pos"]), what
    return rows


@pytest.fixture(scope="module")
def trna_both(gbrna):
    """trna.descr over entries with upper case, u and non-letters, and their reverse complements: hits on both strands"""
    d = _golden("trna")
    seqs = odd_entries(gbrna, limit=300)
    seqs = seqs + [_strand(s, 1) for s in seqs]
    sc, db, hits = _open(d, seqs)
    assert d.both_strands and int((hits[:, 1] == 0).sum()) > 8 and int((hits[:, 1] == 1).sum()) > 8
    yield d, seqs, sc, db, hits
    db.close()
    sc.close()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_record_counts(built, align_checker, trna_both, tmp_path, n):
    d, seqs, sc, db, hits = trna_both
    m = int(hits.shape[0])
    # (spread over all records, again from the start when they run out: the strand 1 hits are those of the later entries)
    rows = hits[(torch.arange(n, device=DEV) * max(1, m // max(n, 1))) % m]
    al = sc.align(db, rows, pos=True)
    want = host_alignment(align_checker, tmp_path, d, seqs, rows.cpu().numpy())
    got = _same(al, want, n)
    assert tuple(al.rows.shape) == (n, int(al.widths.sum()) + d.n_elems - 1) and al.pos.dtype == torch.int32
    assert al.names == d.names() and len(al.names) == d.n_elems and al.col.shape == (al.rows.shape[1],)
    if n == 0:
        assert (al.widths == 0).all() and al.rows.shape[1] == d.n_elems - 1
        return
    assert (al.widths >= 1).all()
    assert al.lines(n - 1) == [got[n - 1].tobytes()[i:i + 70] for i in range(0, got.shape[1], 70)]
    assert (got[:, al.col < 0] == ord("|")).all() and ((al.col >= 0).sum() == al.widths.sum())
    if n >= 63:
        assert {0, 1} <= set(int(x) for x in rows[:, 1].cpu())
        assert (got == ord("-")).any()
    # pos=False: the same rows, no positions
    plain = sc.align(db, rows)
    assert plain.pos is None and torch.equal(plain.rows, al.rows)


def test_row_lengths_and_fill_bytes(built, align_checker, gb, tmp_path):
    # a record gets a wave, a pass 64 bytes of its row: rows shorter than a pass, of exactly one, and of nearly two (the
    # longest loop these entries have is 116; the row of more than two passes is the next test's)
    d = _own(tmp_path, "widths", "descr\n\th5( len=2 )\n\t\tss( minlen=1, maxlen=140 )\n\th3\n")
    seqs = gb[:12]
    sc, db, hits = _open(d, seqs)
    loop = hits[:, HDR + 4 * 1 + 1]
    seen = set()
    for longest in (20, 58, 116):
        rows = hits[loop <= longest]
        rows = torch.cat([rows[::11], rows[rows[:, HDR + 4 * 1 + 1] == longest][:2]])
        al = sc.align(db, rows, pos=True, fill=b"~/o")
        want = host_alignment(align_checker, tmp_path, d, seqs, rows.cpu().numpy(), fill=b"~/o")
        got = _same(al, want, longest)
        assert al.rows.shape[1] == longest + 6 and list(al.right) == [False, False, True]
        assert (got == ord("~")).any() and (got[:, [2, longest + 3]] == ord("/")).all()
        assert not np.isin(got, np.frombuffer(b"-|.", dtype=np.uint8)).any()
        seen.add(int(al.rows.shape[1]))
    assert seen == {26, 64, 122}
    db.close()
    sc.close()


def test_more_elements_than_a_register_and_a_dot(built, align_checker, gb, tmp_path):
    chain = "".join("\tss( minlen=0, maxlen=1 )\n" if k % 29 == 3 else "\tss( len=1 )\n" for k in range(70))
    d = _own(tmp_path, "chain", "descr\n" + chain + "\th5( minlen=3, maxlen=4 )\n\t\tss( minlen=3, maxlen=5 )\n\th3\n")
    assert d.n_elems == 73
    seqs = gb[:6]
    sc, db, hits = _open(d, seqs)
    assert hits.shape[0] > 0
    hits = hits[::3].contiguous()
    al = sc.align(db, hits, pos=True)
    got = _same(al, host_alignment(align_checker, tmp_path, d, seqs, hits.cpu().numpy()), "chain")
    assert bool(al.right[72]) and not al.right[:72].any() and al.widths[70] == 4 and al.widths[72] == 4
    # 155 bytes a row: more than two lane passes, the last one cut by the row's end
    assert al.rows.shape[1] > 128 and al.rows.shape[1] % 64 != 0
    # the '.' of an empty element, the gaps of both directions in columns of the second register
    assert (hits[:, HDR + 4 * 3 + 1] == 0).any() and (hits[:, HDR + 4 * 3 + 1] == 1).any()
    assert (got[:, al.col == 3] == ord(".")).any() and (got[:, al.col == 70] == ord("-")).any() and (got[:, al.col == 72] == ord("-")).any()
    db.close()
    sc.close()


def test_tokens_with_an_alphabet(built, align_checker, gb, tmp_path):
    d = _golden("trna")
    seqs = gb[:300]
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
    assert hits.shape[0] > 0
    # token i is letter "acgu"[i] (u as t), token 4 -- every letter that is not acgt -- is n
    as_letters = [bytes(b if b in b"acgt" else ord("n") for b in s) for s in seqs]
    want = host_alignment(align_checker, tmp_path, d, as_letters, hits.cpu().numpy())
    _same(sc.align(db, hits, pos=True), want, "alphabet")
    _same(sc.align(db, hits, letters=R.alphabet_letters("acgu")), want, "letters")
    db.close()
    sc.close()


def test_contexts_orders_and_given_widths(built, align_checker, gbrna, workdir, tmp_path):
    d = _descr(pins.STRICT_ARGS + ["-descr", "trna.strict.descr"], cwd=workdir)
    seqs = odd_entries(gbrna, limit=300)
    sc, db, hits = _open(d, seqs)
    n = int(hits.shape[0])
    assert n > 4
    al = sc.align(db, hits, pos=True)
    want = host_alignment(align_checker, tmp_path, d, seqs, hits.cpu().numpy())
    _same(al, want, "context")
    assert len(al.widths) == d.n_elems + 2 and al.names[0] == "ctx" and al.names[-1] == "ctx" and al.widths[0] >= 1
    # reversed and repeated rows, under the columns of the whole set
    for what, rows in (("reversed", hits.flip(0)), ("repeated", hits[torch.tensor([2, 2, 0, n - 1, 2, n - 1], device=DEV)])):
        got = sc.align(db, rows, widths=al.widths, pos=True)
        _same(got, host_alignment(align_checker, tmp_path, d, seqs, rows.cpu().numpy(), widths=al.widths), what)
    assert torch.equal(sc.align(db, hits.flip(0)).rows, al.rows.flip(0))
    # wider columns than needed
    wide = al.widths + (np.arange(len(al.widths), dtype=np.int32) % 3)
    _same(sc.align(db, hits, widths=wide, pos=True), host_alignment(align_checker, tmp_path, d, seqs, hits.cpu().numpy(), widths=wide), "wide")
    db.close()
    sc.close()


def test_more_records_than_a_chunk(built, gb):
    d = _golden("trna")
    sc, db, hits = _open(d, gb[:300])
    # the column whose widest field the fewest records have; those records out of the body, one of them last
    lens = hits[:, HDR + 1:HDR + 4 * d.n_elems:4]
    top = lens.max(dim=0).values
    count = (lens == top[None, :]).sum(dim=0)
    count[lens.min(dim=0).values == top] = hits.shape[0] + 1
    c = int(count.argmin())
    widest = lens[:, c] == top[c]
    body, last = hits[~widest], hits[widest][:1]
    assert body.shape[0] > 8 and last.shape[0] == 1
    k = CHUNK // body.shape[0] + 1
    many = torch.cat([body.repeat(k, 1)[:CHUNK], last])
    assert many.shape[0] == CHUNK + 1
    al = sc.align(db, many, pos=True)
    small = sc.align(db, body)
    assert al.widths[c] == int(top[c]) > small.widths[c]
    want = np.maximum(small.widths, sc.align(db, last).widths)
    assert np.array_equal(al.widths, want)
    one = sc.align(db, torch.cat([body, last]), widths=want, pos=True)
    torch.cuda.synchronize()
    m = body.shape[0]
    # the first repeat, the repeats around record 2^17, and the last record
    for r in (0, 1, k - 2):
        assert torch.equal(al.rows[r * m:(r + 1) * m], one.rows[:m]) and torch.equal(al.pos[r * m:(r + 1) * m], one.pos[:m]), r
    tail = CHUNK - (k - 1) * m
    assert torch.equal(al.rows[(k - 1) * m:CHUNK], one.rows[:tail]) and torch.equal(al.pos[(k - 1) * m:CHUNK], one.pos[:tail])
    assert torch.equal(al.rows[CHUNK], one.rows[m]) and torch.equal(al.pos[CHUNK], one.pos[m])
    db.close()
    sc.close()


def test_pos_indexes_hit_structures(built, gbrna):
    d = _golden("pk1")
    seqs = odd_entries(gbrna, limit=300)
    sc, db, hits = _open(d, seqs)
    assert hits.shape[0] > 0
    al, st = sc.align(db, hits, pos=True), sc.hit_structures(db, hits)
    torch.cuda.synchronize()
    letter = al.pos >= 0
    at = (st.off[:-1, None] + al.pos.to(torch.int64) - st.lo[:, None].to(torch.int64))[letter]
    assert torch.equal(al.rows[letter], st.base[at])
    # every base of every window appears once, in its element's column
    assert int(letter.sum()) == int(st.off[-1])
    col = torch.from_numpy(al.col.astype(np.int64)).to(DEV)[None, :].expand_as(al.pos)[letter]
    assert torch.equal(col, st.elem[at].to(torch.int64))
    db.close()
    sc.close()


def test_stream_order(built, gb):
    d = _golden("trna")
    sc, db, hits = _open(d, gb[:300])
    want = sc.align(db, hits, pos=True)
    torch.cuda.synchronize()
    text = db._text
    good = text.clone()
    text.fill_(ord("n"))                # (the text spoilt: rows made of it now are all n)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    filler = torch.zeros(64 << 20, dtype=torch.int32, device=DEV)
    with torch.cuda.stream(side):
        late = torch.zeros_like(hits)
        filler.add_(1)                  # (something to wait behind)
        text.copy_(good)                # the kernels that write the text and the records, then the call right behind
        late.copy_(hits)
        al = sc.align(db, late, pos=True)
        total = al.rows.sum()           # ... and a consumer right behind the call
    side.synchronize()
    assert torch.equal(al.rows, want.rows) and torch.equal(al.pos, want.pos)
    assert int(total) == int(want.rows.sum())
    db.close()
    sc.close()


def test_refusals(built, gb):
    d = _golden("trna")
    seqs = gb[:300]
    sc, db, hits = _open(d, seqs)
    n = int(hits.shape[0])
    assert n > 4
    with pytest.raises(ValueError, match="hits is on cpu"):
        sc.align(db, hits.cpu())
    with pytest.raises(TypeError, match="int64"):
        sc.align(db, hits.to(torch.int64))
    with pytest.raises(ValueError, match=r"\[n, %d\]" % d.hit_stride):
        sc.align(db, hits[:, :-1])
    with pytest.raises(TypeError, match="not a torch.Tensor"):
        sc.align(db, hits.cpu().numpy())
    host = sc.database(seqs)
    with pytest.raises(ValueError, match="not made by database_from_tensor"):
        sc.align(host, hits)
    good = sc.align(db, hits, pos=True)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="one per column, %d, not %d" % (d.n_elems, d.n_elems - 1)):
        sc.align(db, hits, widths=good.widths[:-1])

    # the C ABI, outputs prefilled with a sentinel
    L = R.lib()
    width = int(good.rows.shape[1])
    buf = ctypes.create_string_buffer(1024)
    i32p = ctypes.POINTER(ctypes.c_int32)

    def call(rows, widths, dbh=db._h):
        w = np.ascontiguousarray(widths, dtype=np.int32)
        out = (torch.full((n, width + 8), 77, dtype=torch.uint8, device=DEV), torch.full((n, width + 8), -77, dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        rc = L.rma_hit_alignment(sc._h, dbh, rows.data_ptr(), rows.shape[0], w.ctypes.data_as(i32p), None, None, out[0].data_ptr(),
                                 out[1].data_ptr(), None, buf, 1024)
        torch.cuda.synchronize()
        return rc, out

    def untouched(out):
        return bool((out[0] == 77).all()) and bool((out[1] == -77).all())

    rc, out = call(hits, good.widths)
    flat = (out[0].reshape(-1), out[1].reshape(-1))
    assert rc == 0 and torch.equal(flat[0][:n * width].reshape(n, width), good.rows) and torch.equal(flat[1][:n * width].reshape(n, width), good.pos)
    assert bool((flat[0][n * width:] == 77).all()) and bool((flat[1][n * width:] == -77).all())
    slen0 = len(seqs[int(hits[1, 0])])
    forged = [(2, 0, len(seqs), r"record 2: entry %d outside \[0, %d\)" % (len(seqs), len(seqs))),
              (3, 1, 2, "record 3: strand 2, not 0 or 1"),
              (1, HDR + 4 * 4, slen0 + 1, "record 1: element 4 at offset %d, length .* outside entry" % (slen0 + 1))]
    for row, col, value, words in forged:
        bad = hits.clone()
        bad[row, col] = value
        rc, out = call(bad, good.widths)
        assert rc == 1 and re.search(words, buf.value.decode()) and "nothing written" in buf.value.decode(), buf.value
        assert untouched(out), words
        with pytest.raises(R.RnamotifError, match=words):
            sc.align(db, bad)
    # strands of one helix with unequal lengths are not refused: rmfmt does not refuse them
    odd = hits.clone()
    odd[0, HDR + 4 * 0 + 1] -= 1
    assert sc.align(db, odd).rows.shape[0] == n
    for c in (0, d.n_elems // 2, d.n_elems - 1):
        small = good.widths.copy()
        small[c] -= 1
        words = "column %d: width %d given, the records need %d" % (c, small[c], good.widths[c])
        rc, out = call(hits, small)
        assert rc == 1 and words in buf.value.decode() and "nothing written" in buf.value.decode() and untouched(out), buf.value
        with pytest.raises(R.RnamotifError, match=words):
            sc.align(db, hits, widths=small)
    for h in (host._h, None):
        rc, out = call(hits, good.widths, dbh=h)
        assert rc == 1 and b"not made by rma_db_create_device() or has been destroyed" in buf.value and untouched(out)
    nc, wb = ctypes.c_int32(-1), ctypes.c_int64(-1)
    need = np.full(102, -1, dtype=np.int32)
    rc = L.rma_hit_alignment_shape(sc._h, host._h, hits.data_ptr(), n, ctypes.byref(nc), need.ctypes.data_as(i32p), None, ctypes.byref(wb), None, buf, 1024)
    assert rc == 1 and b"not made by rma_db_create_device() or has been destroyed" in buf.value
    rc = L.rma_hit_alignment_shape(sc._h, db._h, hits.data_ptr(), n, ctypes.byref(nc), need.ctypes.data_as(i32p), None, ctypes.byref(wb), None, buf, 1024)
    assert rc == 0 and nc.value == d.n_elems and wb.value == width and np.array_equal(need[:nc.value], good.widths) and (need[nc.value:] == 0).all()
    host.close()
    # a good call still works, then a closed database
    assert torch.equal(sc.align(db, hits).rows, good.rows)
    db.close()
    with pytest.raises(ValueError, match="closed"):
        sc.align(db, hits)
    sc.close()
