"""Helpers of tests/test_large_db_gpu.py: databases of billions of bases laid out in HBM, the slices and oracle
runs they are held to, and where a record lies in the packed arrays.  Plain functions (no fixtures).

Layouts are lists of entry lengths; an entry's base_off is the running sum of ceil(slen / 32) * 32, as both
packers lay them out, and the text holds the entries one after the other without padding."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLICE_BASES = 1 << 29          # slices are scanned where the rest of the suite holds the scan to the oracle
_COMP = bytes.maketrans(b"acgtnACGTN", b"tgcanTGCAN")


def padded(lens):
    return (np.asarray(lens, dtype=np.int64) + 31) // 32 * 32


def base_offsets(lens):
    p = padded(lens)
    return np.concatenate([[0], np.cumsum(p)[:-1]]).astype(np.int64)


def byte_offsets(lens):
    """n + 1 offsets of the entries in the text."""
    return np.concatenate([[0], np.cumsum(np.asarray(lens, dtype=np.int64))]).astype(np.int64)


def revcomp(s: bytes) -> bytes:
    return s.translate(_COMP)[::-1]


def letter_table(torch, device):
    """256 byte values -> letters: mostly acgt, one value in 64 an ambiguity letter (n, N, r, y)."""
    lut = np.frombuffer(b"acgt", dtype=np.uint8)[np.arange(256) % 4].copy()
    lut[[63, 127, 191, 255]] = np.frombuffer(b"nNry", dtype=np.uint8)
    return torch.from_numpy(lut).to(device)


def random_text(torch, device, nbytes, seed, chunk=1 << 26):
    """nbytes of letters on the device from a seeded torch generator, made a chunk at a time."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    lut = letter_table(torch, device)
    out = torch.empty(nbytes, dtype=torch.uint8, device=device)
    for a in range(0, nbytes, chunk):
        b = min(nbytes, a + chunk)
        r = torch.randint(0, 256, (b - a,), dtype=torch.uint8, device=device, generator=g)
        out[a:b] = lut[r.long()]
        del r
    return out


def put(torch, text, at, seg: bytes):
    text[at:at + len(seg)] = torch.frombuffer(bytearray(seg), dtype=torch.uint8).to(text.device)


def hit_pair(seg: bytes, tail: int):
    """seg (a candidate's whole span on strand 0) followed by its reverse complement, the two overlapping in the
    candidate's last `tail` bases, which no test constrains (the last ss of trna.descr): the strand-0 candidate
    and the strand-1 one both cover the bases [len(seg) - tail, len(seg)) of the pair."""
    return seg + revcomp(seg)[tail:]


def slices(lens, limit=SLICE_BASES):
    """[first, last) runs of entries, each of at most `limit` padded bases (an entry longer than that alone)."""
    p = padded(lens)
    out, a, acc = [], 0, 0
    for i, x in enumerate(p):
        if acc + x > limit and i > a:
            out.append((a, i))
            a, acc = i, 0
        acc += int(x)
    if a < len(p):
        out.append((a, len(p)))
    return out


def sliced_records(sc, make_db, lens, limit=SLICE_BASES):
    """The records of every slice, entry numbers of the whole database: make_db(first, last) builds a slice."""
    parts = []
    for a, b in slices(lens, limit):
        db = make_db(a, b)
        h = sc.scan(db)
        db.close()
        h[:, 0] += a
        parts.append(h)
    return np.concatenate(parts) if parts else None


def sorted_unique(h):
    key = h[:, :5]
    order = np.lexsort(key.T[::-1])
    assert np.array_equal(order, np.arange(len(order))), "records are not in (seq, comp, szero, rank, order) order"
    assert len(np.unique(key, axis=0)) == len(key)


def spans(h, n_elems, lens, base_off):
    """Each record's bases in the packed arrays: [lo, hi) from its entry's base_off, its strand and the
    elements' matchoff / matchlen (positions on the record's strand)."""
    off = h[:, 5:5 + 4 * n_elems:4].astype(np.int64)
    ln = h[:, 6:6 + 4 * n_elems:4].astype(np.int64)
    s_lo = off.min(axis=1)
    s_hi = (off + ln).max(axis=1)
    e = h[:, 0]
    slen = np.asarray(lens, dtype=np.int64)[e]
    comp = h[:, 1] == 1
    lo = np.where(comp, slen - s_hi, s_lo)
    hi = np.where(comp, slen - s_lo, s_hi)
    bo = np.asarray(base_off, dtype=np.int64)[e]
    return bo + lo, bo + hi


def entry_records(h, e):
    r = h[h[:, 0] == e].copy()
    r[:, 0] = 0
    return r


def oracle_entries(descr, seqs_by_entry, whole):
    """The oracle's records of each entry (a database of that one entry) against the scan's, renumbered.
    Returns the number compared."""
    from oracle_binding import oracle_scan
    n = 0
    for e, s in seqs_by_entry.items():
        want = oracle_scan(descr, [s])
        got = entry_records(whole, e)
        assert got.shape == want.shape and np.array_equal(got, want), f"entry {e}: {got.shape} records, the oracle {want.shape}"
        n += want.shape[0]
    return n


def piece_records(h, lo, hi):
    """Records whose start position lies in [lo, hi) (the search of those lies wholly inside a piece)."""
    return h[(h[:, 2] >= lo) & (h[:, 2] < hi)]
