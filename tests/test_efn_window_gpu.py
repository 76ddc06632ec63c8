"""GPU: the energy kernels fetch a call's window in one go (rm_seq_window.h) and pair it from LDS
(rme_cand_t::fill_cache).  A database of a few dozen kilobases in which cloverleaves of the reference's test database
begin at every residue of a 32-base word on both strands, some with an n inside the call: the records of
Scanner.scan, energies included, are the oracle's word for word, with the energy kernel in both its forms and the
search kernel in both of its; so are those of a call longer than the cache and of the instance with the large stacks."""
import itertools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = 5                 # RMA_HIT_HDR: seq, comp, ... then ( offset, length, .. ) of every element
COMP = bytes.maketrans(b"acgtn", b"tgcan")


def _revcomp(s):
    return s.translate(COMP)[::-1]


def _span(d, w):
    """first strand position and length of a record's match"""
    first = int(w[HDR])
    last = int(w[HDR + 4 * (d.n_elems - 1)] + w[HDR + 4 * (d.n_elems - 1) + 1])
    return first, last - first


@pytest.fixture(scope="module")
def cloverleaves(gbrna):
    """(descriptor, entries, oracle's records): built and checked on the CPU."""
    import rnamotif_amd as R
    from oracle_binding import oracle_scan
    os.environ.setdefault("EFNDATA", R.EFNDATA_DIR)
    d = R.Descriptor(["-descr", os.path.join(ROOT, "tests", "golden", "descr", "trna.descr")])
    assert d.n_efn_sites >= 1
    src = [r[2] for r in R.read_fasta(gbrna)[:400]]
    found = oracle_scan(d, src)
    assert found.shape[0] >= 12
    windows = []
    for w in found[:12]:
        strand = src[w[0]] if w[1] == 0 else _revcomp(src[w[0]])
        p, n = _span(d, w)
        windows.append(strand[p:p + n])
    rng = np.random.default_rng(96)
    lut = np.frombuffer(b"acgt", dtype=np.uint8)
    filler = lambda n: lut[rng.integers(0, 4, size=n)].tobytes()       # noqa: E731
    seqs = []
    for k in range(32):
        # strand 0: the call begins at strand position k; strand 1: k bases in front of it on that strand, and
        # ( 7 k ) mod 32 -- every residue once -- behind it, which are the bases in front of it in memory
        seqs.append(filler(k) + windows[k % 12] + filler(9))
        seqs.append(_revcomp(filler(k) + windows[(k + 5) % 12] + filler((7 * k) % 32)))
    # an n inside the call, where the descriptor still matches: every place of three windows tried with the oracle
    with_n = []
    for win in windows[:3]:
        for q in range(len(win)):
            s = filler(11) + win[:q] + b"n" + win[q + 1:] + filler(6)
            hit = oracle_scan(d, [s])
            if any(w[1] == 0 and _span(d, w)[0] <= 11 + q < sum(_span(d, w)) for w in hit):
                with_n.append(s)
    assert len(with_n) >= 3, "trna.descr matches no window with an n in it"
    with_n = with_n[::max(1, len(with_n) // 12)][:12]
    seqs += with_n + [_revcomp(s) for s in with_n[:4]]
    want = oracle_scan(d, seqs)
    # the conditions on the inputs, by the oracle alone
    res = {0: set(), 1: set()}
    n_inside = 0
    for w in want:
        p, n = _span(d, w)
        slen = len(seqs[w[0]])
        res[int(w[1])].add((p if w[1] == 0 else slen - p - n) % 32)          # where its first base lies in memory
        strand = seqs[w[0]] if w[1] == 0 else _revcomp(seqs[w[0]])
        n_inside += b"n" in strand[p:p + n]
    assert res[0] == set(range(32)) and res[1] == set(range(32)), res
    assert n_inside >= 1
    assert sum(len(s) for s in seqs) < 40_000
    return d, seqs, want


def _all_forms(sc, db, want, what):
    for light, flush in itertools.product((0, 1), (1, 0)):
        sc.set_option("efn_light", light)
        sc.set_option("flush", flush)
        got = sc.scan(db)
        assert got.shape == want.shape and np.array_equal(got, want), (what, "efn_light", light, "flush", flush)


def test_every_residue_both_strands(built, cloverleaves, monkeypatch):
    import rnamotif_amd as R
    d, seqs, want = cloverleaves
    monkeypatch.setenv("RNAMOTIF_SHORT", "0")      # (entries tile by tile, not in groups: `flush` 1 is the search kernel that walks nothing)
    sc = R.Scanner(d)
    db = sc.database(seqs)
    _all_forms(sc, db, want, "trna.descr")
    db.close()
    sc.close()


def test_efn2_beside_efn(built, cloverleaves, monkeypatch):
    """the same entries with efn2() scored next to efn(): rme2_site_energy fills its cache by the same two passes"""
    import rnamotif_amd as R
    from oracle_binding import oracle_scan
    _, seqs, _ = cloverleaves
    d = R.Descriptor(["-descr", os.path.join(ROOT, "tests", "data", "trna.efn2.descr")])
    assert d.efn2data and d.n_efn_sites == 2
    want = oracle_scan(d, seqs)
    assert want.shape[0] >= 64
    monkeypatch.setenv("RNAMOTIF_SHORT", "0")
    sc = R.Scanner(d)
    db = sc.database(seqs)
    _all_forms(sc, db, want, "trna.efn2.descr")
    db.close()
    sc.close()


def test_call_longer_than_the_cache(built, tmp_path):
    """hairpins of 48 to 55 base pairs, efn() and efn2() over 100 bases and more: codes and partners on demand"""
    import rnamotif_amd as R
    from oracle_binding import oracle_scan
    (tmp_path / "long.descr").write_text("parms\n\twc += gu;\ndescr\n\th5(minlen=48,maxlen=55)\n\t\tss(minlen=4,maxlen=6)\n\th3\n"
                                         "score\n\t{ e2 = efn2( h5[1], h3[3] ); SCORE = efn( h5[1], h3[3] ); }\n")
    d = R.Descriptor(["-descr", str(tmp_path / "long.descr")])
    rng = np.random.default_rng(7)
    lut = np.frombuffer(b"acgt", dtype=np.uint8)
    rnd = lambda n: lut[rng.integers(0, 4, size=n)].tobytes()          # noqa: E731
    seqs = []
    for k, (hl, loop) in enumerate(((48, 4), (50, 5), (55, 6), (52, 4))):
        stem = rnd(hl)
        s = rnd(13 + 5 * k) + stem + rnd(loop) + _revcomp(stem) + rnd(21)
        seqs += [s, s[:20] + b"n" + s[21:]]
    want = oracle_scan(d, seqs)
    assert want.shape[0] >= 4 and min(_span(d, w)[1] for w in want) > 96
    sc = R.Scanner(d)
    db = sc.database(seqs)
    _all_forms(sc, db, want, "long.descr")
    db.close()
    sc.close()


def test_instance_with_the_large_stacks(built, tmp_path):
    """test_gpu_parity.py's seventeen hairpins side by side (rmd_program_t::efn_big), here at every residue"""
    import rnamotif_amd as R
    from oracle_binding import oracle_scan
    text = ("parms\n\twc += gu;\ndescr\n" +
            "".join("\th5(tag='h%d',minlen=2,maxlen=3)\n\t\tss(len=3)\n\th3(tag='h%d')\n\tss(minlen=1,maxlen=2)\n" % (i, i) for i in range(17)) +
            "score\n\t{ e2 = efn2( h5['h0'], h3['h16'] ); SCORE = efn( h5['h0'], h3['h16'] ); }\n")
    (tmp_path / "many.descr").write_text(text)
    d = R.Descriptor(["-descr", str(tmp_path / "many.descr")])
    rng = np.random.default_rng(31)
    lut = np.frombuffer(b"acgt", dtype=np.uint8)
    flank = lambda n: lut[rng.integers(0, 4, size=n)].tobytes()        # noqa: E731
    units = [b"gcaaagca", b"ggcttagtca", b"gtaaaaca", b"cgagacgaa", b"ggaaatca"]
    seqs = []
    for k in range(8):
        body = b"".join(units[int(i)] for i in rng.integers(0, len(units), size=17))
        seqs.append(flank(40 + 5 * k) + body + flank(30))
    want = oracle_scan(d, seqs)
    assert want.shape[0] >= 8
    sc = R.Scanner(d)
    db = sc.database(seqs)
    _all_forms(sc, db, want, "many.descr")
    assert np.all(np.abs(want[:, d.efn_off + 1]) < 16000)
    db.close()
    sc.close()
