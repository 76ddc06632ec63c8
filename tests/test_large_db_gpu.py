"""GPU: databases past 2^31 and 2^32 bases, and entries up to 2^31 - 1 bases, held to three references: the same
entries scanned as slices of at most 2^29 bases (where the rest of the suite holds the scan to the oracle), the
oracle on the entries at the boundaries, and the host packer's words.  Needs an MI355X: -m gpu.

A. about 4.5 Gbase of entries of about 1 Mbase, one entry across base 2^31 of the packed arrays, one across
   base 2^32 (it also starts at an odd text byte just below 2^32), each with a planted candidate on either
   strand over the boundary base; a run of 300 empty entries past base 2^32.
B. one entry of 2^31 - 1 bases (the longest text_entries takes), candidates planted within the last window of
   each strand; then the same entry followed by 2^22 short entries, which leaves the device hit sort's key no
   room for its order word, so that the host sorts.
C. about 2.3 Gbase of 1.5 million entries of 50 to 3000 bases: past the concatenation gate (2^30 padded bases),
   its slices on this side of it; and databases on either side of the gate itself.
D. entry layouts that send the device packer to its global-memory path (more than 256 entries in one
   workgroup's 8192 bases).

torch is imported before the product library: one HIP runtime serves the process, torch's."""
import os

import torch  # noqa: F401  (first: its HIP runtime is the process's)

import numpy as np
import pytest

import rnamotif_amd as R
import large_db as L

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda", 0)
BOUNDS = (1 << 31, 1 << 32)
BEFORE = 75_008                 # a boundary lies this far into its entry (a multiple of 32)
B_LEN = 150_001                 # the entries across the boundaries: short enough for the oracle
GIB = 1 << 30


def _need(gib):
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < gib * GIB:
        pytest.skip(f"{free / GIB:.1f} GiB of device memory free, {gib} GiB needed")


def _scanner(workdir, name):
    os.environ.setdefault("EFNDATA", R.EFNDATA_DIR)
    path = os.path.join(ROOT, "tests", "data", name) if name == "trna.efn2.descr" else os.path.join(workdir, name)
    return R.Scanner(R.Descriptor(["-descr", path]), device=0)


def _same_words(a, b, what=""):
    for name, x, y in zip(("codes", "amask", "base_off", "slen"), a.packed(), b.packed()):
        assert x.dtype == y.dtype and x.shape == y.shape, what + name
        assert np.array_equal(x, y), f"{what}{name}: first difference at {int(np.argmax(x != y))}"


# ---------------------------------------------------------------- A. long entries past 2^32 bases

def _layout_a(rng, total=4_500_000_000):
    """Entry lengths: about 1 Mbase each, the boundary entries placed BEFORE bases ahead of BOUNDS, a filler ahead
    of each that leaves the running text-minus-padding lag odd (the entry's first byte odd), 300 empty entries
    after the last boundary entry."""
    lens, b, lag, special = [], 0, 0, []
    for B in BOUNDS:
        tb = B - BEFORE
        while tb - b > 1_100_000:
            n = 1_000_000 - int(rng.integers(0, 8))
            lens.append(n)
            b += (n + 31) // 32 * 32
            lag += (n + 31) // 32 * 32 - n
        pf = 0 if lag % 2 else 1
        lens.append(tb - b - pf)
        b, lag = tb, lag + pf
        special.append(len(lens))
        lens.append(B_LEN)
        b += (B_LEN + 31) // 32 * 32
        lag += (B_LEN + 31) // 32 * 32 - B_LEN
    empties = len(lens)
    lens += [0] * 300
    while b < total:
        n = 1_000_000 - int(rng.integers(0, 8))
        lens.append(n)
        b += (n + 31) // 32 * 32
    return lens, special, empties


class TestLongEntries:
    @pytest.fixture(scope="class")
    def a(self, built, workdir):
        _need(12)
        lens, special, empties = _layout_a(np.random.default_rng(31))
        off, bo = L.byte_offsets(lens), L.base_offsets(lens)
        assert [int(bo[i]) + BEFORE for i in special] == list(BOUNDS)
        i2 = special[1]
        assert off[i2] % 2 == 1 and off[i2] < BOUNDS[1] < off[i2 + 1]      # starts at an odd byte below 2^32, ends above
        text = L.random_text(torch, DEV, int(off[-1]), seed=31)
        seg = _segment(os.path.join(ROOT, "tests", "golden", "descr", "trna.descr"))
        pair = L.hit_pair(seg, 4)
        for i in special:
            L.put(torch, text, int(off[i]) + BEFORE - (len(seg) - 2), pair)
        sc = _scanner(workdir, "trna.efn.descr")
        dev = sc.database_from_tensor(text, offsets=off, wait=True)
        seqs = [text[int(off[i]):int(off[i + 1])].cpu().numpy().tobytes() for i in range(len(lens))]
        bound = {i: seqs[i] for i in special}
        host = sc.database(seqs)
        del seqs
        st = {"lens": lens, "off": off, "bo": bo, "special": special, "empties": empties, "text": text,
              "dev": dev, "host": host, "bound": bound}
        del text
        yield st
        dev.close()
        host.close()
        sc.close()
        st.clear()      # (the last reference to the text: its memory goes back to the device)
        torch.cuda.empty_cache()

    def test_words(self, a):
        assert a["dev"].bases == a["host"].bases and int(a["bo"][-1]) + L.padded(a["lens"])[-1] > 4_400_000_000
        _same_words(a["dev"], a["host"])

    @pytest.mark.parametrize("name", ["trna.efn.descr", "mp.ends.descr", "ire.descr", "pk1.descr", "qu+tr.descr",
                                      "trna.efn2.descr"])
    def test_records(self, a, workdir, name):
        sc = _scanner(workdir, name)
        text, off, lens = a["text"], a["off"], a["lens"]
        whole = sc.scan(a["dev"])
        L.sorted_unique(whole)
        assert np.array_equal(sc.scan(a["host"]), whole)
        # the slices
        sl = L.sliced_records(sc, lambda i, j: sc.database_from_tensor(text, offsets=off[i:j + 1]), lens)
        assert sl.shape == whole.shape and np.array_equal(sl, whole)
        # the oracle on the boundary entries
        L.oracle_entries(sc.descr, a["bound"], whole)
        if name.startswith("trna"):
            lo, hi = L.spans(whole, sc.descr.n_elems, lens, a["bo"])
            for B in BOUNDS:
                for comp in (0, 1):
                    assert ((lo <= B) & (B < hi) & (whole[:, 1] == comp)).any(), (B, comp)
        sc.close()

    @pytest.mark.parametrize("name", ["trna.efn.descr", "pk1.descr"])
    def test_modes_and_ranges(self, a, workdir, name):
        sc = _scanner(workdir, name)
        dev, text, off, lens = a["dev"], a["text"], a["off"], a["lens"]
        whole = sc.scan(dev)
        t = sc.scan_tensor(dev)
        assert np.array_equal(t.cpu().numpy(), whole)
        del t
        sc.set_option("host_sort", 1)
        assert np.array_equal(sc.scan(dev), whole)
        sc.set_option("host_sort", 0)
        for v in (0, 1):
            sc.set_option("flush", v)
            assert np.array_equal(sc.scan(dev), whole), ("flush", v)
        sc.set_option("flush", -1)
        # start positions of the boundary entries only, cut near the boundary
        special = a["special"]
        parts = []
        for k in range(2):
            ranges = [(0, 0)] * len(lens)
            for i in special:
                c = BEFORE - 40
                ranges[i] = (0, c) if k == 0 else (c, lens[i])
            db = sc.database_from_tensor(text, offsets=off, ranges=ranges)
            parts.append(sc.scan(db))
            db.close()
        got = np.concatenate(parts)
        got = got[np.lexsort(got[:, :5].T[::-1])]
        want = whole[np.isin(whole[:, 0], special)]
        assert want.shape[0] > 0 and np.array_equal(got, want)
        sc.close()

    def test_empty_run_and_rows_past_2_32(self, a, workdir):
        """(D) the run of empty entries past base 2^32: the records are those of the database without them, entry
        numbers mapped back (the entries after the run included); rows of a 2-D strided view of the same text,
        starting past byte 2^32, some of them empty in runs of 300."""
        text, off, lens, empties = a["text"], a["off"], a["lens"], a["empties"]
        sc = _scanner(workdir, "trna.efn.descr")
        keep = np.array([i for i in range(len(lens)) if lens[i] > 0], dtype=np.int64)
        assert len(keep) == len(lens) - 300 and lens[empties - 1] > 0 and keep[-1] > empties + 300
        # (an empty entry has no bytes: the non-empty ones are the same byte ranges one after the other)
        dense = sc.database_from_tensor(text, offsets=np.append(off[keep], off[-1]))
        whole = sc.scan(a["dev"])
        want = sc.scan(dense)
        dense.close()
        sc.close()
        want[:, 0] = keep[want[:, 0]]
        assert (want[:, 0] > empties).any()
        assert want.shape == whole.shape and np.array_equal(want, whole)
        rng = np.random.default_rng(41)
        rows, width, stride = 2000, 3000, 7001
        rl = rng.integers(0, width + 1, size=rows)
        rl[100:400] = 0
        rl[1500:1800] = 0
        rl[-300:] = 0
        grid = text.as_strided((rows, width), (stride, 1), (1 << 32) + 3)
        _check_layout(workdir, lambda sc: sc.database_from_tensor(grid, lengths=rl),
                      [grid[i, :int(rl[i])].cpu().numpy().tobytes() for i in range(rows)])


# ---------------------------------------------------------------- D. layouts of the packer's global-memory path

HAIRPIN = "descr\n\th5(minlen=4,maxlen=6)\n\tss(minlen=3,maxlen=8)\n\th3\n"


def _check_layout(workdir, make_dev, seqs):
    """The device database make_dev(scanner) has the host packer's words for seqs, and under the concatenation,
    grouped and tile-by-tile instances the records of the same entries without the empty ones."""
    path = os.path.join(workdir, "large_db_hairpin.descr")
    with open(path, "w") as f:
        f.write(HAIRPIN)
    sc = R.Scanner(R.Descriptor(["-descr", path]), device=0)
    dev = make_dev(sc)
    host = sc.database(seqs)
    _same_words(dev, host)
    keep = np.array([i for i, s in enumerate(seqs) if s], dtype=np.int32)
    dense = sc.database([seqs[i] for i in keep])
    n = 0
    for v in (2, 1, 0):
        sc.set_option("short", v)
        want = sc.scan(dense)
        want[:, 0] = keep[want[:, 0]]
        got = sc.scan(dev)
        assert got.shape == want.shape and np.array_equal(got, want), ("short", v)
        assert np.array_equal(sc.scan(host), want), ("short", v)
        n = want.shape[0]
    sc.set_option("short", -1)
    assert n > 0
    for db in (dev, host, dense):
        db.close()
    sc.close()


def _letters(rng, n):
    return np.frombuffer(b"acgt", dtype=np.uint8)[rng.integers(0, 4, size=n)]


@pytest.mark.parametrize("form", ["runs", "twenty"])
def test_packer_global_path(built, workdir, form):
    rng = np.random.default_rng(51 if form == "runs" else 52)
    if form == "runs":
        # runs of more than 256 empty entries at the start, in the middle and at the end
        lens = [0] * 300 + list(rng.integers(1, 2000, size=500)) + [0] * 700 + list(rng.integers(1, 40, size=400)) + [0] * 260
    else:
        # many entries of 1 to 32 bases, most of them 20-mers: the first word of a span often in an earlier entry
        lens = list(np.where(rng.random(200_000) < 0.8, 20, rng.integers(0, 33, size=200_000)))
    lens = [int(x) for x in lens]
    flat = _letters(rng, sum(lens))
    off = L.byte_offsets(lens)
    seqs = [flat[off[i]:off[i + 1]].tobytes() for i in range(len(lens))]
    text = torch.from_numpy(np.concatenate([np.frombuffer(b"x", dtype=np.uint8), flat])).to(DEV)
    _check_layout(workdir, lambda sc: sc.database_from_tensor(text[1:], offsets=off), seqs)


# ---------------------------------------------------------------- B. the longest entry the API takes

def _segment(path):
    """The shortest strand-0 candidate of the descriptor at `path` in seeded random text: its whole span."""
    from oracle_binding import oracle_scan
    d = R.Descriptor(["-descr", path])
    s = np.frombuffer(b"acgt", dtype=np.uint8)[np.random.default_rng(1).integers(0, 4, 200_000)].tobytes()
    h = oracle_scan(d, [s])
    h = h[h[:, 1] == 0]
    lo, hi = L.spans(h, d.n_elems, [len(s)], [0])
    k = int(np.argmin(hi - lo))
    d.close()
    return s[int(lo[k]):int(hi[k])]


def _piece_filter(r, lo_cut, hi_cut, n, maxlen, g=200):
    """Records of a piece of n positions on one strand whose search lies wholly inside it: a margin only on the
    side where the piece was cut from the entry (the other side is the entry's own end, in both scans)."""
    lo = g if lo_cut else 0
    hi = n - maxlen - g if hi_cut else n
    return r[(r[:, 2] >= lo) & (r[:, 2] < hi)]


@pytest.mark.parametrize("name", ["trna.efn.descr", "pk1.descr"])
def test_longest_entry(built, workdir, name):
    """One entry of 2^31 - 1 bases: its first and last 200 kbase against the oracle, with candidates planted so
    that a start position within the last maxlen bases of each strand is compared (there, start + window passes
    INT_MAX).  Then the same entry followed by 2^22 short entries: 23 + 1 + 31 bits of entry, strand and position
    leave the device hit sort's key less than its 4 bits of order word, so the host sorts, and the long entry runs
    in a database of short mean entry length -- grouped and tile-by-tile layouts (short forced to 1 and 0)."""
    _need(8)
    slen = (1 << 31) - 1
    n_short, short_len = 1 << 22, 100
    sc = _scanner(workdir, name)
    d = sc.descr
    seg = _segment(os.path.join(ROOT, "tests", "golden", "descr" if name.startswith("trna") else "test",
                                "trna.descr" if name.startswith("trna") else name))
    n = len(seg)
    assert n + 3 < d.maxlen       # (start slen - n - 2: past slen - maxlen + 1, where the window's sums wrapped)
    text = L.random_text(torch, DEV, slen + n_short * short_len, seed=61)
    L.put(torch, text, slen - n - 2, seg)                       # strand 0: start slen - n - 2
    L.put(torch, text, 2, L.revcomp(seg))                       # strand 1: start slen - n - 2 as well
    if name.startswith("trna"):
        pair = L.hit_pair(seg, 4)                               # (a candidate on either strand over one base)
        L.put(torch, text, 1000, pair)
        L.put(torch, text, slen - 100_000, pair)
    with pytest.raises(ValueError, match="2\\*\\*31 bases or more"):
        R.text_entries(text, lengths=[slen + 1])
    piece = 200_000
    S = (slen - piece) // 32 * 32
    first = text[:piece].cpu().numpy().tobytes()
    last = text[S:slen].cpu().numpy().tobytes()
    alone = sc.database_from_tensor(text[:slen], lengths=[slen], wait=True)
    # the words of both ends against the host packer's
    codes, amask, _, _ = alone.packed()
    for at, s in ((0, first), (S, last)):
        h = sc.database([s])
        hc, ha, _, _ = h.packed()
        h.close()
        w = at // 32
        assert np.array_equal(amask[w:w + ha.size], ha) and np.array_equal(codes[2 * w:2 * w + hc.size], hc), at
    del codes, amask
    big = sc.scan(alone)
    L.sorted_unique(big)
    sc.set_option("host_sort", 1)
    assert np.array_equal(sc.scan(alone), big)
    sc.set_option("host_sort", 0)
    alone.close()
    # every record inside the entry
    lo, hi = L.spans(big, d.n_elems, [slen], [0])
    assert (big[:, 2] >= 0).all() and (lo >= 0).all() and (hi <= slen).all()
    # the ends against the oracle
    from oracle_binding import oracle_scan
    pos_cols = [2] + [5 + 4 * e for e in range(d.n_elems)]
    n_cmp = 0
    for which, s in (("first", first), ("last", last)):
        want = oracle_scan(d, [s])
        got, ref = [], []
        for comp in (0, 1):
            # first piece: strand 0 cut at its high end, strand 1 at its low end; the last piece the other way round
            lo_cut = (which == "first") == (comp == 1)
            shift = (0 if comp == 0 else slen - len(s)) if which == "first" else (S if comp == 0 else 0)
            r = big[big[:, 1] == comp].copy()
            r[:, pos_cols] -= shift
            got.append(_piece_filter(r, lo_cut, not lo_cut, len(s), d.maxlen))
            ref.append(_piece_filter(want[want[:, 1] == comp], lo_cut, not lo_cut, len(s), d.maxlen))
        # the planted candidates within the last maxlen start positions of each strand are among those compared
        end = got[0] if which == "last" else got[1]
        assert (end[:, 2] == len(s) - n - 2).any(), which
        got, ref = np.concatenate(got), np.concatenate(ref)
        assert got.shape == ref.shape and np.array_equal(got, ref), which
        n_cmp += ref.shape[0]
    assert n_cmp > 10
    # the long entry and 2^22 short ones
    lens = [slen] + [short_len] * n_short
    assert (len(lens) - 1).bit_length() + 1 + slen.bit_length() + d.maxlen.bit_length() > 60    # order word < 4 bits
    rest = sc.database_from_tensor(text[slen:], lengths=lens[1:])
    tail = sc.scan(rest)
    rest.close()
    tail[:, 0] += 1
    assert tail.shape[0] > 0
    many = sc.database_from_tensor(text, lengths=lens)
    for v in (-1, 1, 0):
        sc.set_option("short", v)
        whole = sc.scan(many)
        assert np.array_equal(whole[whole[:, 0] == 0], big), ("short", v)
        assert np.array_equal(whole[whole[:, 0] > 0], tail), ("short", v)
    sc.set_option("short", -1)
    many.close()
    sc.close()
    del text, whole
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- C. short entries past the concatenation gate

class TestShortEntries:
    @pytest.fixture(scope="class")
    def c(self, built, workdir):
        _need(8)
        rng = np.random.default_rng(71)
        lens = [int(x) for x in rng.integers(50, 3001, size=1_500_000)]
        off, bo = L.byte_offsets(lens), L.base_offsets(lens)
        text = L.random_text(torch, DEV, int(off[-1]), seed=71)
        sc = _scanner(workdir, "trna.descr")
        dev = sc.database_from_tensor(text, offsets=off, wait=True)
        flat = text.cpu().numpy()
        seqs = [flat[off[i]:off[i + 1]].tobytes() for i in range(len(lens))]
        del flat
        host = sc.database(seqs)
        # about 20 entries for the oracle: those across bases 2^29, 2^30, 2^31 and a spread of others
        ends = bo + L.padded(lens)
        pick = {int(np.searchsorted(ends, B, side="right")) for B in (1 << 29, 1 << 30, 1 << 31)}
        pick |= {int(x) for x in rng.choice(len(lens), size=17, replace=False)}
        sample = {i: seqs[i] for i in sorted(pick)}
        del seqs
        st = {"lens": lens, "off": off, "bo": bo, "text": text, "dev": dev, "host": host, "sample": sample,
              "ends": ends}
        del text
        yield st
        dev.close()
        host.close()
        sc.close()
        st.clear()      # (the last reference to the text: its memory goes back to the device)
        torch.cuda.empty_cache()

    def test_words(self, c):
        assert c["dev"].bases == c["host"].bases and int(c["ends"][-1]) > (1 << 31) + (1 << 27)
        _same_words(c["dev"], c["host"])

    @pytest.mark.parametrize("name", ["trna.descr", "mp.ends.descr"])
    def test_modes(self, c, workdir, name):
        sc = _scanner(workdir, name)
        text, off, lens = c["text"], c["off"], c["lens"]
        ref = L.sliced_records(sc, lambda i, j: sc.database_from_tensor(text, offsets=off[i:j + 1]), lens)
        L.sorted_unique(ref)
        assert ref.shape[0] > 1000
        for opt, v in (("default", None), ("short", 0), ("short", 1), ("short", 2), ("host_sort", 1)):
            if v is not None:
                sc.set_option(opt, v)
            got = sc.scan(c["dev"])
            assert got.shape == ref.shape and np.array_equal(got, ref), (opt, v)
            if v is not None:
                sc.set_option(opt, -1 if opt == "short" else 0)
        assert np.array_equal(sc.scan(c["host"]), ref)
        L.oracle_entries(sc.descr, c["sample"], ref)
        sc.close()

    def test_gate_edge(self, c, workdir):
        """The last prefix of the entries below 2^30 padded bases (concatenation tiles allowed) and the first at
        or above (refused): either way, in every instance, the slices' records."""
        sc = _scanner(workdir, "trna.descr")
        text, off, lens, ends = c["text"], c["off"], c["lens"], c["ends"]
        k = int(np.searchsorted(ends, 1 << 30, side="left"))       # ends[k - 1] < 2^30 <= ends[k]
        assert ends[k - 1] < (1 << 30) <= ends[k]
        ref = L.sliced_records(sc, lambda i, j: sc.database_from_tensor(text, offsets=off[i:j + 1]), lens[:k + 1])
        for m in (k, k + 1):
            db = sc.database_from_tensor(text, offsets=off[:m + 1])
            want = ref[ref[:, 0] < m]
            for v in (-1, 2, 1, 0):
                sc.set_option("short", v)
                got = sc.scan(db)
                assert got.shape == want.shape and np.array_equal(got, want), (m, v)
            sc.set_option("short", -1)
            db.close()
        sc.close()
