"""GPU: databases packed on the device from text already in HBM (Scanner.database_from_tensor,
rma_db_create_device) hold the words the host packer makes of the same bytes, and scans of them return the
same records, on the host (scan) and left on the device (scan_tensor).  Needs an MI355X: -m gpu.

torch is imported before the product library: one HIP runtime serves the process, torch's (INTEGRATION.md,
"Databases from device memory")."""
import ctypes
import os

import torch  # noqa: F401  (first: its HIP runtime is the process's)

import numpy as np
import pytest

import rnamotif_amd as R

# (each test well under a minute on the MI355X; the bound keeps the file under about two)
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(60)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESCR = os.path.join(ROOT, "tests", "golden", "descr")
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def trna(built):
    os.environ.setdefault("EFNDATA", R.EFNDATA_DIR)
    sc = R.Scanner(R.Descriptor(["-descr", os.path.join(DESCR, "trna.descr")]), device=0)
    yield sc
    sc.close()


@pytest.fixture(scope="module")
def gb_seqs(gbrna):
    return [r[2] for r in R.read_fasta(gbrna)]


def _ragged(seqs, lead=0):
    """The entries one after the other on the GPU (after `lead` bytes of 'x'), and their offsets."""
    flat = b"x" * lead + b"".join(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64) + lead
    t = torch.frombuffer(bytearray(flat), dtype=torch.uint8) if flat else torch.empty(0, dtype=torch.uint8)
    return t.to(DEV), off


def _same_words(a, b):
    pa, pb = a.packed(), b.packed()
    for name, x, y in zip(("codes", "amask", "base_off", "slen"), pa, pb):
        assert x.dtype == y.dtype and x.shape == y.shape, name
        assert np.array_equal(x, y), f"{name}: first difference at {int(np.argmax(x != y))}"


def _odd_bytes(rng, n):
    pool = np.frombuffer(b"acgtuACGTUacgtacgtnNrRyYwWsSkKmMbBdDhHvV-.*\n\x00\xff\x80 ", dtype=np.uint8)
    return pool[rng.integers(0, len(pool), size=n)].tobytes()


def test_words_equal_host_packer(trna):
    rng = np.random.default_rng(11)
    seqs = [_odd_bytes(rng, n) for n in (0, 1, 15, 16, 31, 32, 33, 1000, 0, 7, 1_000_000, 64, 3)]
    seqs.append(rng.integers(0, 256, size=4099, dtype=np.uint8).tobytes())     # every byte value
    host = trna.database(seqs)
    for lead in (0, 1, 3):
        text, off = _ragged(seqs, lead)
        # the entries at every alignment, from the storage's start and from a view's
        dev = trna.database_from_tensor(text, offsets=off, wait=True) if lead != 3 else \
            trna.database_from_tensor(text[lead:], offsets=off - lead, wait=True)
        _same_words(dev, host)
        assert dev.bases == host.bases
        dev.close()
    host.close()


def test_recycled_block_is_overwritten(trna):
    """The block of a destroyed database goes to the next one of about its size, uncleared: every word of
    the new one, padding bits included, is written by the kernel."""
    rng = np.random.default_rng(12)
    lens = [1_500_000, 33, 1, 100_001, 0, 63]
    seqs = [_odd_bytes(rng, n) for n in lens]
    # the same number of words, every bit of them set where it can be: 'n' (mask) and 't' (code 3)
    dirty = trna.database([b"nt" * (((n + 31) // 32) * 16) for n in lens])
    dirty.close()
    text, off = _ragged(seqs)
    dev = trna.database_from_tensor(text, offsets=off, wait=True)
    host = trna.database(seqs)
    _same_words(dev, host)
    dev.close()
    host.close()


def _scanner(name, text=None):
    os.environ.setdefault("EFNDATA", R.EFNDATA_DIR)
    if text is None:
        return R.Scanner(R.Descriptor(["-descr", os.path.join(DESCR, name)]), device=0)
    return R.Scanner(R.Descriptor(["-descr", text]), device=0)


def _records_agree(sc, host, dev, at_least=1):
    want = sc.scan(host)
    got = sc.scan(dev)
    assert want.shape[0] >= at_least, want.shape
    assert got.shape == want.shape and np.array_equal(got, want)
    t = sc.scan_tensor(dev)
    assert t.device == DEV and t.dtype == torch.int32 and tuple(t.shape) == want.shape
    assert np.array_equal(t.cpu().numpy(), want)
    return want.shape[0]


@pytest.mark.parametrize("name", ["trna.descr", "pk1.descr", "qu+tr.descr"])
def test_records_equal_host_database(gb_seqs, name):
    sc = _scanner(name)
    host = sc.database(gb_seqs)
    # the device text in mixed case, u for t here and there: the same words
    mixed = [s.upper() if i % 3 == 0 else (s.replace(b"t", b"u") if i % 3 == 1 else s) for i, s in enumerate(gb_seqs)]
    text, off = _ragged(mixed)
    dev = sc.database_from_tensor(text, offsets=off)
    _records_agree(sc, host, dev)
    dev.close()
    host.close()
    sc.close()


def test_records_with_ranges(gb_seqs):
    sc = _scanner("trna.descr")
    ranges = [(i % 7 * 10, max(i % 7 * 10, len(s) - i % 5 * 20)) for i, s in enumerate(gb_seqs)]
    host = sc.database(gb_seqs, ranges=ranges)
    text, off = _ragged(gb_seqs)
    dev = sc.database_from_tensor(text, offsets=off, ranges=ranges)
    assert dev.bases == host.bases
    _records_agree(sc, host, dev)
    dev.close()
    host.close()
    sc.close()


def test_records_of_a_loose_descriptor(tmp_path):
    """seq= with letters the words cannot decide alone (tests/test_loose_seq.py): the scan's superset of
    candidates, the same from either database."""
    from test_loose_seq import _database
    seqs = _database(str(tmp_path / "db.fastn"))
    path = tmp_path / "x.descr"
    path.write_text('parms\n\tiupac = 0;\ndescr\n\tss(minlen=4,maxlen=5,seq="^nnac")\n')
    sc = _scanner(None, str(path))
    host = sc.database(seqs)
    text, off = _ragged(seqs)
    dev = sc.database_from_tensor(text, offsets=off)
    _records_agree(sc, host, dev)
    dev.close()
    host.close()
    sc.close()


def test_input_forms(trna, gb_seqs):
    seqs = gb_seqs[:600]
    host = trna.database(seqs)
    want = trna.scan(host)
    assert want.shape[0] > 0
    width = max(len(s) for s in seqs)
    lens = [len(s) for s in seqs]
    rows = np.full((len(seqs), width + 13), ord("g"), dtype=np.uint8)
    for i, s in enumerate(seqs):
        rows[i, 5:5 + len(s)] = np.frombuffer(s, dtype=np.uint8)
    big = torch.from_numpy(rows).to(DEV)
    # [N, L] with lengths, the rest of each row 'g'
    plain = big[:, 5:5 + width].contiguous()
    forms = [(plain, {"lengths": lens}), (big[:, 5:5 + width], {"lengths": torch.tensor(lens)})]
    # values 0..3 for acgu (4 for any other letter) with alphabet="acgu"
    codes = np.full(rows.shape, 2, dtype=np.uint8)
    lut = np.full(256, 4, dtype=np.uint8)
    lut[np.frombuffer(b"acgt", dtype=np.uint8)] = np.arange(4, dtype=np.uint8)
    codes[:, 5:] = lut[rows[:, 5:]]
    forms.append((torch.from_numpy(codes).to(DEV)[:, 5:5 + width], {"lengths": lens, "alphabet": "acgu"}))
    for text, kw in forms:
        dev = trna.database_from_tensor(text, **kw)
        _same_words(dev, host)
        got = trna.scan(dev)
        assert np.array_equal(got, want)
        dev.close()
    host.close()
    # no entries: an empty tensor, or none of a tensor's bytes
    for text, kw in ((torch.empty(0, dtype=torch.uint8, device=DEV), {"offsets": [0]}),
                     (big[0], {"lengths": []})):
        dev = trna.database_from_tensor(text, **kw)
        assert dev.bases == 0 and dev.n_seqs == 0
        assert trna.scan(dev).shape == (0, trna.descr.hit_stride)
        assert tuple(trna.scan_tensor(dev).shape) == (0, trna.descr.hit_stride)
        assert all(a.size == 0 for a in dev.packed())
        dev.close()


def test_stream_order(trna, gb_seqs):
    """The text written on a side stream, that stream current, no synchronise: the packing runs behind it."""
    host = trna.database(gb_seqs)
    want = trna.scan(host)
    flat = np.frombuffer(b"".join(gb_seqs), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum([len(s) for s in gb_seqs])]).astype(np.int64)
    src = torch.from_numpy(flat.copy()).pin_memory()
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize(DEV)
    with torch.cuda.stream(side):
        text = torch.full((len(flat),), ord("n"), dtype=torch.uint8, device=DEV)
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(20_000_000)      # (the side stream busy for a while before the bytes arrive)
        text.copy_(src, non_blocking=True)
        text.add_(1).sub_(1)
        dev = trna.database_from_tensor(text, offsets=off)
        out = trna.scan_tensor(dev)
        got = out.cpu().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(trna.scan(dev), want)
    dev.close()
    host.close()


def _hip():
    return ctypes.CDLL("libamdhip64.so.7")


def _raw_create(sc, ptr, text_bytes, start, slen, table=None):
    L = R.lib()
    start = np.ascontiguousarray(start, dtype=np.int64)
    slen = np.ascontiguousarray(slen, dtype=np.int32)
    h = ctypes.c_void_p()
    err = ctypes.create_string_buffer(1024)
    rc = L.rma_db_create_device(sc._h, ptr, text_bytes, start.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                slen.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None, None, len(slen), table, None,
                                ctypes.byref(h), err, 1024)
    if rc == 0:
        L.rma_db_destroy(h)
    return rc, err.value.decode()


def test_refusals_before_any_launch(trna, gb_seqs):
    with pytest.raises(ValueError, match="is on cpu: the scanner is on cuda:0"):
        trna.database_from_tensor(torch.zeros(64, dtype=torch.uint8))
    text = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = text.data_ptr()
    rc, err = _raw_create(trna, p, 4096, [0, 4000], [10, 97])
    assert rc == 1 and "entry 1: bytes [4000, 4097) lie past the text's 4096 bytes" in err
    rc, err = _raw_create(trna, p, 4096, [0, 8], [10, -1])
    assert rc == 1 and "entry 1: negative length" in err
    rc, err = _raw_create(trna, p, 4096, [-8], [4])
    assert rc == 1 and "entry 0: negative start" in err
    # host memory: unregistered and page-locked
    host = np.zeros(4096, dtype=np.uint8)
    rc, err = _raw_create(trna, host.ctypes.data, 4096, [0], [100])
    assert rc == 1 and "the text" in err and ("not device memory" in err or "host memory" in err)
    pinned = torch.zeros(4096, dtype=torch.uint8).pin_memory()
    rc, err = _raw_create(trna, pinned.data_ptr(), 4096, [0], [100])
    assert rc == 1 and "page-locked host memory" in err
    # a declared extent past the allocation the runtime knows
    base, size = ctypes.c_void_p(), ctypes.c_size_t()
    hip = _hip()
    assert hip.hipMemGetAddressRange(ctypes.byref(base), ctypes.byref(size), ctypes.c_void_p(p)) == 0
    past = base.value + size.value - p
    rc, err = _raw_create(trna, p, past + 4096, [past - 8], [16])
    assert rc == 1 and "outside its allocation" in err
    # a table of codes above 4
    rc, err = _raw_create(trna, p, 4096, [0], [10], table=bytes([5] * 256))
    assert rc == 1 and "table[ 0 ] = 5" in err
    # records into host memory
    db = trna.database(gb_seqs[:600])
    dst = np.zeros(64, dtype=np.int32)
    err = ctypes.create_string_buffer(1024)
    trna.scan_begin(db)
    n = trna.scan_end_on_device()
    assert n > 0
    rc = R.lib().rma_scan_records_to_device(trna._h, dst.ctypes.data, n * trna.descr.hit_stride, None, err, 1024)
    assert rc == 1 and "the destination" in err.value.decode()
    out = torch.zeros((n, trna.descr.hit_stride), dtype=torch.int32, device=DEV)
    rc = R.lib().rma_scan_records_to_device(trna._h, out.data_ptr(), out.numel() - 1, None, err, 1024)
    assert rc == 1 and "room for %d" % (out.numel() - 1) in err.value.decode()
    db.close()


def test_wrong_device(trna):
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU: no other device to refuse")
    other = torch.zeros(64, dtype=torch.uint8, device=torch.device("cuda", 1))
    with pytest.raises(ValueError, match="is on cuda:1: the scanner is on cuda:0"):
        trna.database_from_tensor(other)
    rc, err = _raw_create(trna, other.data_ptr(), 64, [0], [10])
    assert rc == 1 and "memory of device 1, the scanner is on device 0" in err
