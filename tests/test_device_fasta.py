"""GPU: databases made of FASTA text already in HBM (Scanner.database_from_fasta_tensor, rma_db_create_device_fasta)
hold the entries, names and words the host route makes of the same file (Pack.read + database_from_pack), refuse
what the parallel reader hands to the serial reader, and scan and replay as databases made of cut text do.  Needs an
MI355X: -m gpu.

torch is imported before the product library: one HIP runtime serves the process, torch's (INTEGRATION.md,
"Databases from device memory")."""
import contextlib
import hashlib
import os

import torch  # noqa: F401  (first: its HIP runtime is the process's)

import numpy as np
import pytest

import pins
import rnamotif_amd as R
from test_stream import CASES

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(60)]

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
def trna(built):
    os.environ.setdefault("EFNDATA", R.EFNDATA_DIR)
    sc = R.Scanner(R.Descriptor(["-descr", os.path.join(DESCR, "trna.descr")]), device=0)
    yield sc
    sc.close()


@pytest.fixture(scope="module")
def gb_text(gbrna):
    with open(gbrna, "rb") as f:
        return f.read()


def _on_gpu(data: bytes, offset=0, tail=b""):
    """data in HBM as a view `offset` bytes into its storage, which goes on with `tail` behind the view."""
    whole = b"\n" * offset + data + tail
    t = torch.frombuffer(bytearray(whole), dtype=torch.uint8).to(DEV) if whole else torch.empty(0, dtype=torch.uint8, device=DEV)
    return t[offset:offset + len(data)]


def _same_words(a, b):
    pa, pb = a.packed(), b.packed()
    for name, x, y in zip(("codes", "amask", "base_off", "slen"), pa, pb):
        assert x.dtype == y.dtype and x.shape == y.shape, name
        assert np.array_equal(x, y), f"{name}: first difference at {int(np.argmax(x != y))}"


def _host_route(sc, data: bytes, tmp_path, name="host.fa"):
    """(database, sids, sdefs) of the same bytes as a file through Pack.read"""
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    pk = R.Pack.read([path])
    recs = [pk.record(i) for i in range(pk.count)]
    pk.close()
    return sc.database([r[2] for r in recs]), [r[0] for r in recs], [r[1] for r in recs]


def _declined(data: bytes, tmp_path, name="probe.fa"):
    """Pack.read_entries -- the parallel reader alone -- returns None for text it hands to the serial reader."""
    if not data:
        return False
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(data)
    index = R.database_index([path])
    return index is None or R.Pack.read_entries([path], list(range(len(index)))) is None


def _held_to_host(sc, data: bytes, tmp_path, offset=0, tail=b""):
    dev = sc.database_from_fasta_tensor(_on_gpu(data, offset, tail))
    host, sids, sdefs = _host_route(sc, data, tmp_path)
    try:
        assert dev.n_seqs == host.n_seqs and dev.bases == host.bases
        _same_words(dev, host)
        assert dev.sids == sids and dev.sdefs == sdefs
    finally:
        host.close()
    return dev


def test_reference_database_equals_host_route(trna, gb_text, tmp_path):
    dev = _held_to_host(trna, gb_text, tmp_path)
    assert dev.n_seqs == 4067
    dev.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_reader_cases(trna, tmp_path, name):
    data = CASES[name]
    if _declined(data, tmp_path):
        with pytest.raises(R.RnamotifError, match=r"entry \d+ at byte \d+"):
            trna.database_from_fasta_tensor(_on_gpu(data))
    else:
        _held_to_host(trna, data, tmp_path).close()


def test_refusals_name_the_entry(trna):
    for data, words in ((CASES["unnamed_mid"], "entry 1 at byte 10: unnamed entry"), (CASES["not_gt"], "entry 0 at byte 0: the text does not begin"),
                        (CASES["long_def"], "entry 0 at byte 0: definition line too long"), (CASES["nul_def"], "entry 0 at byte 0: NUL"),
                        (b">a\nAC\n>b\nACGTA\n", "entry 1 at byte 6: sequence too long")):
        with pytest.raises(R.RnamotifError, match=words):
            trna.database_from_fasta_tensor(_on_gpu(data), maxslen=4)
    # (maxslen as Pack.read takes it: -N 4 reads four letters)
    trna.database_from_fasta_tensor(_on_gpu(b">a\nACGT\n"), maxslen=4).close()


def _seam_text():
    """Text whose '>' , '\\n', last byte of a definition line and lone letters fall on, before and behind the seams of
    the chunks, with a definition line over three chunks, an entry over many, thousands of one-letter entries in one
    chunk, empty entries back to back, and one chunk more than the scan's second level needs."""
    chunk, block, _ = R.fasta_device_shape()
    rng = np.random.default_rng(31)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    parts, size = [], 0

    def add(b):
        nonlocal size
        parts.append(b)
        size += len(b)

    def letters(n):
        return acgt[rng.integers(0, 4, size=n)].tobytes()

    def pad_to(pos, k):
        """letters (in lines of 70) until the text is `pos` bytes long; k names the entry"""
        add(b">pad%d filler\n" % k)
        room = pos - size
        assert room >= 2, (pos, size)
        body = bytearray(letters(room))
        body[69::70] = b"\n" * len(body[69::70])
        body[-1:] = b"\n"
        add(bytes(body))

    k = 0
    for d in (-1, 0, 1):                # a '>' at a seam
        k += 1
        pad_to(k * 2 * chunk + d, k)
        add(b">gt%d at the seam\nAC\n" % (d + 1))
    for d in (-1, 0, 1):                # the '\n' that ends a definition line at a seam (and so its last byte before it)
        k += 1
        head = b">nl%d ends" % (d + 1)
        pad_to(k * 2 * chunk + d - len(head), k)
        add(head + b"\nGGA\n")
    for d in (-1, 0, 1):                # a lone letter at a seam, blanks and digits around it
        k += 1
        pad_to(k * 2 * chunk + d - 10, k)
        add(b">lone\n 12 T 34 \n")
    k += 1
    pad_to(k * 2 * chunk - 2, k)         # a definition line from the end of one chunk over the next into a third
    add(b">span " + b"d" * (chunk + 10) + b" > still the definition\nACGTN\n")
    add(b">many over many chunks\n" + letters(5 * chunk + 17) + b"\n")
    k = (size + 2 * chunk - 1) // (2 * chunk) + 1
    pad_to(k * 2 * chunk, k)
    add(b"".join(b">%d\nA\n" % i for i in range(3000)))                                   # one-letter entries
    add(b">e1\n>e2 x\n>e3\n\n>e4\n")                                                       # empty entries
    # enough chunks for the second level of the scan, and one more
    want = (block + 1) * chunk + 5
    while size < want:
        add(b">fill%d\n" % size + letters(min(200_000, max(want - size, 1))) + b"\n")
    return b"".join(parts)


def test_chunk_and_scan_seams(trna, tmp_path):
    chunk, block, cap = R.fasta_device_shape()
    data = _seam_text()
    assert len(data) > (block + 1) * chunk
    for d in range(3):
        assert data[(d + 1) * 2 * chunk + d - 1] == ord(">") and data[(d + 4) * 2 * chunk + d - 1] == ord("\n")
        assert data[(d + 7) * 2 * chunk + d - 1] == ord("T")
    at = data.index(b">span ")
    assert at // chunk + 2 == data.index(b"\n", at) // chunk
    dev = _held_to_host(trna, data, tmp_path)
    assert dev.n_seqs > 3000
    dev.close()


def test_overlong_definition_line(trna, tmp_path):
    """A definition line longer than the bytes of it that are looked at is refused without being copied whole, the '>'
    in it starting nothing; and the entry numbers behind a line with '>' in it count entries, not '>'."""
    chunk, _, cap = R.fasta_device_shape()
    pre = b">a x\n" + b"ACGT" * ((chunk - 40) // 4) + b"\n"
    data = pre + b">b " + b"d>" * (chunk + 50) + b"\nACGT\n>\nAC\n"
    with pytest.raises(R.RnamotifError, match="entry 1 at byte %d: definition line too long" % len(pre)):
        trna.database_from_fasta_tensor(_on_gpu(data))
    # with the long line's entry made regular the unnamed entry behind it is the one refused: entry 2, not 1 + the
    # '>' of the long line
    with pytest.raises(R.RnamotifError, match="entry 2 at byte %d: unnamed" % (len(pre) + 9 + 5)):
        trna.database_from_fasta_tensor(_on_gpu(pre + b">b d>d>d\nACGT\n>\nAC\n"))


def test_alignment_and_extent(trna, gb_text, tmp_path):
    data = gb_text[:300_001]
    data = data[:data.rindex(b"\n>")] + b"\n"
    host, sids, sdefs = _host_route(trna, data, tmp_path)
    for offset in (0, 1, 2, 3):
        dev = trna.database_from_fasta_tensor(_on_gpu(data, offset))
        _same_words(dev, host)
        assert dev.sids == sids
        dev.close()
    # a view that ends before its storage does: what lies behind it is not the text's
    for offset in (0, 3):
        dev = trna.database_from_fasta_tensor(_on_gpu(data, offset, tail=b">x\nAAAA" * 50))
        assert dev.n_seqs == host.n_seqs
        _same_words(dev, host)
        dev.close()
    host.close()


def test_recycled_buffers_are_overwritten(trna, tmp_path):
    rng = np.random.default_rng(12)
    lens = [1_500_000, 33, 1, 100_001, 0, 63]
    pool = np.frombuffer(b"acgtuACGTUnNrRyY", dtype=np.uint8)
    seqs = [pool[rng.integers(0, pool.size, size=n)].tobytes() for n in lens]
    data = b"".join(b">s%d d\n" % i + s + b"\n" for i, s in enumerate(seqs))
    # the same sizes with every bit of the words and every byte of the clean text set, then given back
    dirty = trna.database_from_fasta_tensor(_on_gpu(b"".join(b">s%d d\n" % i + b"\xff" * 0 + b"nt" * ((n + 1) // 2) + b"\n" for i, n in enumerate(lens))))
    dirty.close()
    dev = _held_to_host(trna, data, tmp_path)
    dev.close()


def _scanner(workdir, name):
    os.environ.setdefault("EFNDATA", R.EFNDATA_DIR)
    with _cwd(workdir):
        d = R.Descriptor(["-descr", name])
    return d, R.Scanner(d, device=0)


@pytest.mark.parametrize("name", ["trna.descr", "pk1.descr", "qu+tr.descr"])
def test_end_to_end(built, workdir, gb_text, gbrna, tmp_path, name):
    d, sc = _scanner(workdir, name)
    host = sc.database([r[2] for r in R.read_fasta(gbrna)])
    want = sc.scan(host)
    text = _on_gpu(gb_text)
    dev = sc.database_from_fasta_tensor(text)
    # the text is free once the call has returned
    text.zero_()
    got = sc.scan(dev)
    assert got.shape == want.shape and np.array_equal(got, want)
    hits = sc.scan_tensor(dev)
    assert np.array_equal(hits.cpu().numpy(), want)
    out = str(tmp_path / "out.txt")
    with _cwd(workdir):
        rp = R.Replay(d, out)
        rp.device(dev, hits, sids=dev.sids, sdefs=dev.sdefs)
        rp.close()
    with open(out, "rb") as f:
        printed = f.read()
    nhits, md5 = pins.SLACK[name]
    assert printed.count(b"\n>") + (1 if printed.startswith(b">") else 0) == nhits
    assert hashlib.md5(printed).hexdigest() == md5
    dev.close()
    host.close()
    sc.close()


def test_shared_context_and_the_cache(trna, gb_text, gbrna):
    seqs = [r[2] for r in R.read_fasta(gbrna)]
    dev = trna.database_from_fasta_tensor(_on_gpu(gb_text))
    other = R.Scanner(R.Descriptor(["-descr", os.path.join(DESCR, "pk1.descr")]), device=0)
    other.attach(dev)
    host = other.database(seqs)
    assert np.array_equal(other.scan(dev), other.scan(host))
    want = host.packed()
    bases = dev.bases
    dev.close()
    # the clean text is back in the cache: a database of cut text of its size finds room, and has the same words
    flat = torch.frombuffer(bytearray(b"".join(seqs)), dtype=torch.uint8).to(DEV)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    again = trna.database_from_tensor(flat, offsets=off, wait=True)
    assert again.bases == bases
    for x, y in zip(again.packed(), want):
        assert np.array_equal(x, y)
    again.close()
    host.close()
    other.close()


def test_empty_text(trna):
    dev = trna.database_from_fasta_tensor(torch.empty(0, dtype=torch.uint8, device=DEV))
    assert dev.n_seqs == 0 and dev.bases == 0 and dev.sids == [] and trna.scan(dev).shape[0] == 0
    dev.close()
