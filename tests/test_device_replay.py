"""GPU: candidates of databases made from text in HBM, replayed from that text (Replay.device, rma_replay_device):
the windows come from the device (rm_hitwin_dev.hip), the score program and the printer are the host's.

  * every pinned descriptor (tests/pins.py) over the reference's test database as one CUDA tensor prints the
    reference's own output;
  * raw bytes (upper case, U, IUPAC letters, '-', NUL, 0xff) print what Replay.batch prints for the same entries
    normalised by the readers' rule, at every byte alignment, for plain, score, context and loose descriptors;
  * alphabet= tokens, row subsets in any order, more records than one chunk;
  * refusals before anything is printed.  A malformed record is refused on the device, before any text is read.

torch is imported before the product library: one HIP runtime serves the process."""
import contextlib
import hashlib
import os

import torch  # noqa: F401  (first: its HIP runtime is the process's)

import numpy as np
import pytest

import pins
import rnamotif_amd as R
from test_hit_windows_cpu import LOOSE, normalise, odd_entries

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESCR = os.path.join(ROOT, "tests", "golden", "descr")
DEV = torch.device("cuda", 0)


@contextlib.contextmanager
def _cwd(d):
    old = os.getcwd()
    os.chdir(d)
    try:
        yield
    finally:
        os.chdir(old)


@pytest.fixture(scope="module")
def gb(gbrna):
    return R.read_fasta(gbrna)


def _ragged(seqs, lead=0):
    flat = b"x" * lead + b"".join(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64) + lead
    t = torch.frombuffer(bytearray(flat), dtype=torch.uint8) if flat else torch.empty(0, dtype=torch.uint8)
    return t.to(DEV), off


def _device_output(descr, seqs, path, sids=None, sdefs=None, lead=0, rows=None, accepted=False, **kw):
    """scan_tensor + Replay.device over seqs on the GPU: (bytes printed, n_printed[, mask], records)"""
    sc = R.Scanner(descr, device=0)
    text, off = _ragged(seqs, lead)
    db = sc.database_from_tensor(text, offsets=off, **kw)
    hits = sc.scan_tensor(db)
    if rows is not None:
        hits = rows(hits)
    rp = R.Replay(descr, path)
    got = rp.device(db, hits, sids=sids, sdefs=sdefs, accepted=accepted)
    rp.close()
    db.close()
    sc.close()
    with open(path, "rb") as f:
        return f.read(), got, hits.cpu().numpy()


def _host_output(descr, seqs, records, path, sids=None, sdefs=None):
    sids = sids if sids is not None else [b"%d" % i for i in range(len(seqs))]
    sdefs = sdefs if sdefs is not None else [b""] * len(seqs)
    rp = R.Replay(descr, path)
    n = rp.batch(sids, sdefs, seqs, records)
    rp.close()
    with open(path, "rb") as f:
        return f.read(), n


def _pin_case(workdir, gb, argv, pin, tmp_path):
    with _cwd(workdir):
        d = R.Descriptor(argv)
        out, n, _ = _device_output(d, [r[2] for r in gb], str(tmp_path / "out.txt"), sids=[r[0] for r in gb],
                                   sdefs=[r[1] for r in gb])
    nhits, md5 = pin
    assert out.count(b"\n>") + (1 if out.startswith(b">") else 0) == nhits
    assert hashlib.md5(out).hexdigest() == md5


@pytest.mark.parametrize("name", sorted(pins.SLACK))
def test_pinned_output(built, workdir, gb, tmp_path, name):
    _pin_case(workdir, gb, ["-descr", name], pins.SLACK[name], tmp_path)


@pytest.mark.parametrize("name", sorted(pins.STRICT))
def test_pinned_strict_output(built, workdir, gb, tmp_path, name):
    _pin_case(workdir, gb, pins.STRICT_ARGS + ["-descr", name + ".strict.descr"], pins.STRICT[name], tmp_path)


def _odd_set(gbrna):
    rng = np.random.default_rng(3)
    extra = [_odd_bytes(rng, n) for n in (0, 1, 33, 1_000_000)]
    return odd_entries(gbrna, limit=600) + extra


def _odd_bytes(rng, n):
    pool = np.frombuffer(b"acgtuACGTUacgtacgtnNrRyYwWsSkKmMbBdDhHvV-.*\n\x00\xff\x80 ", dtype=np.uint8)
    return pool[rng.integers(0, len(pool), size=n)].tobytes()


@pytest.mark.parametrize("case", ["trna", "score.2", "trna.strict", "loose_literal_n", "loose_backref"])
def test_raw_bytes_equal_host_replay(built, workdir, gbrna, tmp_path, case):
    argv = {"trna": ["-descr", os.path.join(DESCR, "trna.descr")], "score.2": ["-descr", "score.2.descr"],
            "trna.strict": pins.STRICT_ARGS + ["-descr", "trna.strict.descr"]}.get(case)
    if argv is None:
        path = os.path.join(workdir, case + ".descr")
        with open(path, "w") as f:
            f.write(LOOSE[case[len("loose_"):]])
        argv = ["-descr", os.path.basename(path)]
    seqs = _odd_set(gbrna)
    norm = [normalise(s) for s in seqs]
    with _cwd(workdir):
        d = R.Descriptor(argv)
        if case.startswith("loose"):
            assert d.loose > 0
        printed = []
        for lead in range(4):
            got, n, recs = _device_output(d, seqs, str(tmp_path / "dev.txt"), lead=lead)
            assert recs.shape[0] > 0
            want, m = _host_output(d, norm, recs, str(tmp_path / "host.txt"))
            assert got == want and n == m
            printed.append(n)
    assert printed[0] > 0 or case == "loose_backref"


def test_alphabet_tokens_on_strided_rows(built, gb, tmp_path):
    d = R.Descriptor(["-descr", os.path.join(DESCR, "trna.descr")])
    seqs = [r[2] for r in gb[:800]]
    width = max(len(s) for s in seqs)
    lens = [len(s) for s in seqs]
    letters = np.full((len(seqs), width + 13), ord("g"), dtype=np.uint8)
    for i, s in enumerate(seqs):
        letters[i, 5:5 + len(s)] = np.frombuffer(s, dtype=np.uint8)
    lut = np.full(256, 4, dtype=np.uint8)
    lut[np.frombuffer(b"acgt", dtype=np.uint8)] = np.arange(4, dtype=np.uint8)
    tokens = torch.from_numpy(lut[letters]).to(DEV)[:, 5:5 + width]     # rows at a stride of width + 13
    sc = R.Scanner(d, device=0)
    db = sc.database_from_tensor(tokens, lengths=lens, alphabet="acgu")
    hits = sc.scan_tensor(db)
    rp = R.Replay(d, str(tmp_path / "dev.txt"))
    n = rp.device(db, hits)
    rp.close()
    db.close()
    assert n > 0
    # token i is letter "acgu"[i] (u as t), token 4 -- every letter that is not acgt -- is n
    as_letters = [bytes(b if b in b"acgt" else ord("n") for b in s) for s in seqs]
    want, m = _host_output(d, as_letters, hits.cpu().numpy(), str(tmp_path / "host.txt"))
    assert open(str(tmp_path / "dev.txt"), "rb").read() == want and n == m
    sc.close()


def test_subset_and_accepted(built, workdir, gb, tmp_path):
    with _cwd(workdir):
        d = R.Descriptor(["-descr", "trna.efn.descr"])
    seqs = [r[2] for r in gb]
    sc = R.Scanner(d, device=0)
    text, off = _ragged(seqs)
    db = sc.database_from_tensor(text, offsets=off)
    hits = sc.scan_tensor(db)
    assert d.n_efn_sites > 0 and hits.shape[0] > 100
    # the records whose energy is below the median, reversed
    e = hits[:, d.efn_off]
    sub = hits[e < e.median()].flip(0)
    rp = R.Replay(d, str(tmp_path / "dev.txt"))
    n, acc = rp.device(db, sub, accepted=True)
    rp.close()
    recs = sub.cpu().numpy()
    want, m = _host_output(d, seqs, recs, str(tmp_path / "host.txt"))
    assert open(str(tmp_path / "dev.txt"), "rb").read() == want and n == m
    assert acc.dtype == np.bool_ and acc.shape == (recs.shape[0],) and int(acc.sum()) == n
    # record by record: the host replay of that record alone (the program holds nothing from one to the next)
    rp = R.Replay(d, str(tmp_path / "one.txt"))
    for h in range(recs.shape[0]):
        one = recs[h:h + 1].copy()
        k = int(one[0, 0])
        one[0, 0] = 0
        assert rp.batch([b"%d" % k], [b""], [seqs[k]], one) == int(acc[h]), h
    rp.close()
    db.close()
    sc.close()


def test_more_records_than_a_chunk(built, gb, tmp_path):
    d = R.Descriptor(["-descr", os.path.join(DESCR, "trna.descr")])
    seqs = [r[2] for r in gb]
    sc = R.Scanner(d, device=0)
    text, off = _ragged(seqs)
    db = sc.database_from_tensor(text, offsets=off)
    hits = sc.scan_tensor(db)
    k = 200_000 // hits.shape[0] + 2
    many = hits.repeat(k, 1)
    assert many.shape[0] > 200_000
    rp = R.Replay(d, str(tmp_path / "dev.txt"))
    n, acc = rp.device(db, many, accepted=True)
    rp.close()
    want, m = _host_output(d, seqs, many.cpu().numpy(), str(tmp_path / "host.txt"))
    assert open(str(tmp_path / "dev.txt"), "rb").read() == want and n == m and int(acc.sum()) == n
    db.close()
    sc.close()


def test_refusals(built, gb, tmp_path):
    d = R.Descriptor(["-descr", os.path.join(DESCR, "trna.descr")])
    seqs = [r[2] for r in gb[:600]]
    sc = R.Scanner(d, device=0)
    text, off = _ragged(seqs)
    db = sc.database_from_tensor(text, offsets=off)
    hits = sc.scan_tensor(db)
    assert hits.shape[0] > 3
    path = str(tmp_path / "out.txt")

    def refused(make, exc, words, on=None):
        rp = R.Replay(d, path)
        with pytest.raises(exc, match=words):
            rp.device(on if on is not None else db, make())
        rp.close()
        assert os.path.getsize(path) == 0, words

    def bad(row, col, value):
        def make():
            h = hits.clone()
            h[row, col] = value
            return h
        return make
    ctx = d.ctx_off
    refused(bad(2, 0, len(seqs)), R.RnamotifError, r"record 2: entry %d outside \[0, %d\)" % (len(seqs), len(seqs)))
    refused(bad(3, 0, -1), R.RnamotifError, "record 3: entry -1")
    refused(bad(1, 1, 2), R.RnamotifError, "record 1: strand 2, not 0 or 1")
    refused(bad(0, R.RMA_HIT_HDR + 4 * 3 + 1, 2 ** 31 - 1), R.RnamotifError, "record 0: element 3 at offset .* length 2147483647")
    refused(bad(1, R.RMA_HIT_HDR + 4 * 5, -7), R.RnamotifError, "record 1: element 5 at offset -7")
    refused(bad(hits.shape[0] - 1, R.RMA_HIT_HDR, 2 ** 31 - 1), R.RnamotifError, "record %d: element 0" % (hits.shape[0] - 1))
    assert ctx == R.RMA_HIT_HDR + 4 * d.n_elems
    refused(lambda: hits.cpu(), ValueError, "hits is on cpu")
    refused(lambda: hits.to(torch.int64), TypeError, "int64")
    refused(lambda: hits[:, :-1], ValueError, r"\[n, %d\]" % d.hit_stride)
    refused(lambda: hits.cpu().numpy(), TypeError, "not a torch.Tensor")
    host = sc.database(seqs)
    refused(lambda: hits, ValueError, "not made by database_from_tensor", on=host)
    host.close()
    # another descriptor's replay: records of the wrong width
    other = R.Descriptor(["-descr", os.path.join(DESCR, "pk1.descr")])
    rp = R.Replay(other, path)
    with pytest.raises(ValueError, match=r"\[n, %d\]" % other.hit_stride):
        rp.device(db, hits)
    rp.close()
    assert os.path.getsize(path) == 0
    # the C ABI: a database made on the host, a null one
    import ctypes
    buf = ctypes.create_string_buffer(1024)
    rp = R.Replay(d, path)
    host = sc.database(seqs)
    printed = ctypes.c_int64()
    for h in (host._h, None):
        rc = R.lib().rma_replay_device(rp._h, h, hits.data_ptr(), hits.shape[0], None, None, None, None, ctypes.byref(printed),
                                       None, buf, 1024)
        assert rc == 1 and b"not made by rma_db_create_device() or has been destroyed" in buf.value
    rc = R.lib().rma_replay_device(rp._h, db._h, hits.data_ptr(), -1, None, None, None, None, ctypes.byref(printed), None, buf, 1024)
    assert rc == 1 and b"-1 records" in buf.value
    rp.close()
    host.close()
    # nothing was printed, and a good call still works on the same replay
    rp = R.Replay(d, path)
    n = rp.device(db, hits)
    rp.close()
    assert n > 0
    # a closed database
    db.close()
    refused(lambda: hits, ValueError, "closed")
    sc.close()
