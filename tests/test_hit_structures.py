"""GPU: hit records expanded into per-base tensors on the device (Scanner.hit_structures, rma_hit_structures: the
fill kernel of rm_hitstruct_dev.hip) against the same rule, rm_hitstruct.h, run on the host through
tests/hostsim/hit_structures_check.cpp -- bit for bit:

  * duplex, pseudoknot, triple, quad and context descriptors, both strands, databases from tokens on strided rows
    and from FASTA text; the letters are the windows Replay.device() replays;
  * any rows in any order: subsets, duplicates, no record, one record, a record with an empty window;
  * more records than a chunk; windows shorter than, as long as and longer than the 64 lanes a record gets; a
    descriptor of more elements than one lane pass holds;
  * under a non-default stream right behind the kernel that wrote the records;
  * refusals with their words.  A forged record is caught by the check kernels before the fill kernel runs: the
    outputs keep the sentinel they were filled with.

torch is imported before the product library: one HIP runtime serves the process."""
import ctypes
import os
import re

import torch  # noqa: F401  (first: its HIP runtime is the process's)

import numpy as np
import pytest

import pins
import rnamotif_amd as R
from test_hit_structures_cpu import GOLDEN, HDR, checker, helices, host_structures, program_of  # noqa: F401
from test_hit_windows_cpu import normalise, odd_entries

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

DEV = torch.device("cuda", 0)
CHUNK = 1 << 17
KEYS = ("off", "lo", "base", "elem", "mate")


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


def _ragged(seqs, lead=3):
    flat = b"x" * lead + b"".join(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64) + lead
    return torch.frombuffer(bytearray(flat), dtype=torch.uint8).to(DEV), off


def _open(d, seqs):
    sc = R.Scanner(d, device=0)
    text, off = _ragged(seqs)
    db = sc.database_from_tensor(text, offsets=off)
    return sc, db, sc.scan_tensor(db)


def _got(st):
    torch.cuda.synchronize()
    return {k: getattr(st, k).cpu().numpy() for k in KEYS}


def _same(got, want, what=""):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k)


def _strand(raw, comp):
    s = normalise(raw)
    if comp:
        s = s[::-1].translate(bytes.maketrans(b"acgt", b"tgca"))
        s = bytes(b if b in b"acgt" else ord("n") for b in s)
    return s


def _check_letters(got, recs, seqs):
    for h, w in enumerate(recs):
        a, b = int(got["off"][h]), int(got["off"][h + 1])
        lo = int(got["lo"][h])
        assert got["base"][a:b].tobytes() == _strand(seqs[int(w[0])], int(w[1]))[lo:lo + b - a], h


CASES = {"trna": ("trna", 300), "pk1": ("pk1", 300), "trip": ("trip", None), "quad": ("quad", 300), "qu+tr": ("qu+tr", None)}


@pytest.mark.parametrize("case", sorted(CASES) + ["context"])
def test_parity_with_the_host_rule(built, checker, gbrna, workdir, tmp_path, case):
    if case == "context":
        d = _descr(pins.STRICT_ARGS + ["-descr", "trna.strict.descr"], cwd=workdir)
        seqs = odd_entries(gbrna, limit=300)
    else:
        d = _golden(CASES[case][0])
        # (trip.descr and qu+tr.descr have their first candidates past the thousandth entry)
        seqs = odd_entries(gbrna, limit=CASES[case][1])
    if case == "trna":
        # both strands: what entry e has on strand 0 its reverse complement has on strand 1
        seqs = seqs + [_strand(s, 1) for s in seqs]
    sc, db, hits = _open(d, seqs)
    recs = hits.cpu().numpy()
    assert recs.shape[0] > 0, case
    got = _got(sc.hit_structures(db, hits))
    _same(got, host_structures(checker, str(tmp_path), d, seqs, recs), case)
    _check_letters(got, recs, seqs)
    if case == "trna":
        assert d.both_strands and (recs[:, 1] == 0).sum() > 8 and (recs[:, 1] == 1).sum() > 8
    if case == "context":
        assert {d.n_elems, d.n_elems + 1} <= set(int(x) for x in got["elem"])
    assert (got["mate"][:, 0] >= 0).any()
    db.close()
    sc.close()


def test_tokens_on_strided_rows(built, checker, gb, tmp_path):
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
    got = _got(sc.hit_structures(db, hits))
    # token i is letter "acgu"[i] (u as t), token 4 -- every letter that is not acgt -- is n
    as_letters = [bytes(b if b in b"acgt" else ord("n") for b in s) for s in seqs]
    _same(got, host_structures(checker, str(tmp_path), d, as_letters, hits.cpu().numpy()))
    db.close()
    sc.close()


def test_fasta_tensor(built, checker, gbrna, gb, tmp_path):
    d = _golden("trna")
    raw = open(gbrna, "rb").read()
    cut = raw.index(b"\n>", 300_000) + 1
    text = torch.frombuffer(bytearray(raw[:cut]), dtype=torch.uint8).to(DEV)
    sc = R.Scanner(d, device=0)
    db = sc.database_from_fasta_tensor(text)
    hits = sc.scan_tensor(db)
    assert hits.shape[0] > 0 and db.n_seqs > 100
    got = _got(sc.hit_structures(db, hits))
    _same(got, host_structures(checker, str(tmp_path), d, gb[:db.n_seqs], hits.cpu().numpy()))
    db.close()
    sc.close()


def test_arbitrary_rows(built, checker, gb, tmp_path):
    d = _golden("trna")
    seqs = gb[:300]
    sc, db, hits = _open(d, seqs)
    n = hits.shape[0]
    assert n > 20
    g = torch.Generator().manual_seed(4)
    perm = torch.randperm(n, generator=g).to(DEV)
    dup = torch.tensor([5, 5, 0, n - 1, 5, n - 1, 0], device=DEV)
    empty = hits[:3].clone()
    empty[1, HDR + 1:HDR + 4 * d.n_elems:4] = 0        # every element of length 0: nothing covers anything
    for what, rows in (("shuffled", hits[perm][:n // 2]), ("duplicates", hits[dup]), ("one", hits[7:8]), ("empty window", empty)):
        got = _got(sc.hit_structures(db, rows))
        _same(got, host_structures(checker, str(tmp_path), d, seqs, rows.cpu().numpy()), what)
    assert got["off"][1] == got["off"][2] and got["off"][3] > got["off"][2]
    st = sc.hit_structures(db, hits[:0])
    torch.cuda.synchronize()
    assert st.off.tolist() == [0] and st.off.dtype == torch.int64 and tuple(st.mate.shape) == (0, 3)
    assert st.lo.numel() == 0 and st.base.numel() == 0 and st.elem.numel() == 0
    assert st.base.dtype == torch.uint8 and st.elem.dtype == torch.int16 and st.mate.dtype == torch.int32 and st.lo.dtype == torch.int32
    # padded(): plain torch over the same tensors
    st = sc.hit_structures(db, hits[:9])
    base, elem, mate, mask = st.padded(fill=(0, -2, -3))
    off = st.off.cpu().numpy()
    assert tuple(base.shape) == (9, int(np.diff(off).max())) and tuple(mate.shape) == tuple(base.shape) + (3,)
    for h in range(9):
        m = int(off[h + 1] - off[h])
        assert mask[h].sum().item() == m and mask[h, :m].all()
        assert torch.equal(base[h, :m], st.base[off[h]:off[h + 1]]) and torch.equal(elem[h, :m], st.elem[off[h]:off[h + 1]])
        assert torch.equal(mate[h, :m], st.mate[off[h]:off[h + 1]])
        assert (base[h, m:] == 0).all() and (elem[h, m:] == -2).all() and (mate[h, m:] == -3).all()
    db.close()
    sc.close()


def test_more_records_than_a_chunk(built, gb):
    d = _golden("trna")
    sc, db, hits = _open(d, gb[:300])
    n = hits.shape[0]
    k = (CHUNK + 5000) // n + 2
    many = hits.repeat(k, 1)
    assert many.shape[0] > CHUNK + n
    one, st = sc.hit_structures(db, hits), sc.hit_structures(db, many)
    torch.cuda.synchronize()
    lens = one.off[1:] - one.off[:-1]
    per = int(one.off[-1])
    assert torch.equal(st.off[1:] - st.off[:-1], lens.repeat(k)) and int(st.off[-1]) == k * per and int(st.off[0]) == 0
    assert torch.equal(st.lo, one.lo.repeat(k))
    # the first repeat, the last one, and the repeats around record 2^17
    seam = CHUNK // n
    for r in (0, k - 1, seam - 1, seam, seam + 1):
        a, b = r * per, (r + 1) * per
        assert torch.equal(st.base[a:b], one.base) and torch.equal(st.elem[a:b], one.elem) and torch.equal(st.mate[a:b], one.mate), r
    db.close()
    sc.close()


def test_window_widths_and_many_elements(built, checker, gb, tmp_path):
    # a record gets a wave: windows shorter than its 64 lanes, of 64, of 65 and of nearly two passes
    path = tmp_path / "widths.descr"
    path.write_text("descr\n\th5( len=2 )\n\t\tss( minlen=1, maxlen=140 )\n\th3\n")
    d = _descr(["-descr", str(path)])
    seqs = gb[:12]
    sc, db, hits = _open(d, seqs)
    hits = hits[::7].contiguous()
    got = _got(sc.hit_structures(db, hits))
    _same(got, host_structures(checker, str(tmp_path), d, seqs, hits.cpu().numpy()), "widths")
    widths = set(int(x) for x in np.diff(got["off"]))
    assert {5, 63, 64, 65} <= widths and max(widths) > 100
    db.close()
    sc.close()
    # more elements than the 64 one lane pass holds, a helix among those of the second pass, elements of length 0
    chain = "".join("\tss( minlen=0, maxlen=1 )\n" if k % 29 == 3 else "\tss( len=1 )\n" for k in range(66))
    path = tmp_path / "chain.descr"
    path.write_text("descr\n" + chain + "\th5( minlen=3, maxlen=4 )\n\t\tss( minlen=3, maxlen=5 )\n\th3\n")
    d = _descr(["-descr", str(path)])
    assert d.n_elems == 69
    seqs = gb[:6]
    sc, db, hits = _open(d, seqs)
    assert hits.shape[0] > 0
    hits = hits[::3].contiguous()
    got = _got(sc.hit_structures(db, hits))
    _same(got, host_structures(checker, str(tmp_path), d, seqs, hits.cpu().numpy()), "chain")
    assert {66, 68} <= set(int(x) for x in got["elem"]) and (got["mate"][got["elem"] == 68, 0] >= 0).all()
    assert (hits[:, HDR + 4 * 3 + 1] == 0).any() and (hits[:, HDR + 4 * 3 + 1] == 1).any()
    db.close()
    sc.close()


def test_stream_order(built, gb):
    d = _golden("trna")
    sc, db, hits = _open(d, gb[:300])
    want = sc.hit_structures(db, hits)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    filler = torch.zeros(64 << 20, dtype=torch.int32, device=DEV)
    with torch.cuda.stream(side):
        late = torch.zeros_like(hits)
        filler.add_(1)              # (something to wait behind)
        late.copy_(hits)            # the kernel that writes the records, then the call right behind it
        st = sc.hit_structures(db, late)
        total = st.mate.sum()       # ... and a consumer right behind the call
    side.synchronize()
    for k in KEYS:
        assert torch.equal(getattr(st, k), getattr(want, k)), k
    assert int(total) == int(want.mate.sum())
    db.close()
    sc.close()


def test_refusals(built, gb):
    d = _golden("trna")
    seqs = gb[:300]
    sc, db, hits = _open(d, seqs)
    n = hits.shape[0]
    assert n > 4
    with pytest.raises(ValueError, match="hits is on cpu"):
        sc.hit_structures(db, hits.cpu())
    with pytest.raises(TypeError, match="int64"):
        sc.hit_structures(db, hits.to(torch.int64))
    with pytest.raises(ValueError, match=r"\[n, %d\]" % d.hit_stride):
        sc.hit_structures(db, hits[:, :-1])
    with pytest.raises(TypeError, match="not a torch.Tensor"):
        sc.hit_structures(db, hits.cpu().numpy())
    host = sc.database(seqs)
    with pytest.raises(ValueError, match="not made by database_from_tensor"):
        sc.hit_structures(host, hits)

    # the C ABI, outputs prefilled with a sentinel
    L = R.lib()
    good = sc.hit_structures(db, hits)
    torch.cuda.synchronize()
    total = int(good.off[-1])
    buf = ctypes.create_string_buffer(1024)

    def call(rows, total_arg, dbh=db._h):
        out = (torch.full((n + 1,), -77, dtype=torch.int64, device=DEV), torch.full((n,), -77, dtype=torch.int32, device=DEV),
               torch.full((total + 64,), 77, dtype=torch.uint8, device=DEV), torch.full((total + 64,), -77, dtype=torch.int16, device=DEV),
               torch.full((total + 64, 3), -77, dtype=torch.int32, device=DEV))
        torch.cuda.synchronize()
        rc = L.rma_hit_structures(sc._h, dbh, rows.data_ptr(), rows.shape[0], None, total_arg, *[t.data_ptr() for t in out],
                                  None, buf, 1024)
        torch.cuda.synchronize()
        return rc, out

    def untouched(out):
        return all(bool((t == (77 if t.dtype == torch.uint8 else -77)).all()) for t in out)

    rc, out = call(hits, total)
    assert rc == 0 and torch.equal(out[0], good.off) and torch.equal(out[4][:total], good.mate) and torch.equal(out[2][:total], good.base)
    assert bool((out[2][total:] == 77).all()) and bool((out[4][total:] == -77).all()) and bool((out[3][total:] == -77).all())
    hx = helices(program_of(d))
    e3 = next(e for e in range(d.n_elems) if hx[e] is not None and hx[e][1] == 1)
    e5 = hx[e3][0][0]
    slen0 = len(seqs[int(hits[1, 0])])
    forged = [(2, 0, len(seqs), r"record 2: entry %d outside \[0, %d\)" % (len(seqs), len(seqs))),
              (3, 1, 2, "record 3: strand 2, not 0 or 1"),
              (1, HDR + 4 * 4, slen0 + 1, "record 1: element 4 at offset %d, length .* outside entry" % (slen0 + 1)),
              (n - 1, HDR + 4 * e3 + 1, int(hits[n - 1, HDR + 4 * e5 + 1]) - 1,
               "record %d: element %d has length .* element %d of the same helix" % (n - 1, e3, e5))]
    for row, col, value, words in forged:
        bad = hits.clone()
        bad[row, col] = value
        rc, out = call(bad, total)
        assert rc == 1 and re.search(words, buf.value.decode()) and "nothing written" in buf.value.decode(), buf.value
        assert untouched(out), words
        with pytest.raises(R.RnamotifError, match=words):
            sc.hit_structures(db, bad)
    rc, out = call(hits, total + 1)
    assert rc == 1 and ("have %d bytes, not the %d" % (total, total + 1)) in buf.value.decode() and untouched(out)
    for h in (host._h, None):
        rc, out = call(hits, total, dbh=h)
        assert rc == 1 and b"not made by rma_db_create_device() or has been destroyed" in buf.value and untouched(out)
    size = ctypes.c_int64(-1)
    rc = L.rma_hit_structures_size(sc._h, host._h, hits.data_ptr(), n, None, ctypes.byref(size), buf, 1024)
    assert rc == 1 and b"not made by rma_db_create_device() or has been destroyed" in buf.value
    rc = L.rma_hit_structures_size(sc._h, db._h, hits.data_ptr(), n, None, ctypes.byref(size), buf, 1024)
    assert rc == 0 and size.value == total
    host.close()
    # a good call still works, then a closed database
    assert torch.equal(sc.hit_structures(db, hits).mate, good.mate)
    db.close()
    with pytest.raises(ValueError, match="closed"):
        sc.hit_structures(db, hits)
    sc.close()
