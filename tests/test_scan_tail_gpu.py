"""GPU: a scan's tail -- energies, ordering, the records' way back -- enqueued by rma_scan_begin() behind the scan's kernels,
ahead of the count (rm_tail_plan.h, launch_tail() and scan_end() of rm_scanner.cpp, the device-count forms of the energy kernels
and of DevHitSort::run()).  Default options: dbg and timing turn the tail ahead off, so what a scan's end did is read from
Scanner.last_end() -- (host waits, records of the tail ahead taken, search launches, energy launches).

Every scan is compared word for word with the oracle and with the same scanner at spec_tail 0.  A scanner's first scan has no
tail ahead (2 waits); from the second on the end waits once and takes the records when the scan found no more than was planned
for -- a quarter above the most records of the scans before, 1024 at least -- and nothing has to be repeated; otherwise it does
the tail again (two energy launches) and the records are the same.  The cases are tests/scan_end_cases.py's, with their premises."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (first: its HIP runtime is the process's)

import scan_end_cases as SC
from test_gpu_parity import _descr, _env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL_MIN = 1024             # records a tail ahead is planned for at least (RMA_TAIL_MIN, rm_tail_plan.h)


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return SC.write_all(tmp_path_factory.mktemp("scan_tail"))


_WANT = {}


def _oracle(d, key, seqs):
    """the oracle's records, once per key"""
    from oracle_binding import oracle_scan
    if key not in _WANT:
        _WANT[key] = oracle_scan(d, seqs)
        _WANT[key].setflags(write=False)
    return _WANT[key]


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def scan(sc, db, want, what):
    """Scanner.scan() with the tail ahead where the rule allows it: the oracle's records; what the end did"""
    got = sc.scan(db)
    end = sc.last_end()
    print(what, "records", got.shape[0], "last_end", end)
    assert _same(got, want), (what, got.shape, want.shape, end)
    return end


def scan_off(sc, db, want, what):
    """the same scanner at spec_tail 0: the same records, and no tail was taken"""
    sc.set_option("spec_tail", 0)
    got = sc.scan(db)
    end = sc.last_end()
    sc.set_option("spec_tail", -1)
    assert _same(got, want), (what, "spec_tail 0", got.shape, want.shape)
    assert end[1] == 0, (what, "spec_tail 0", end)


def _trna_case(workdir, gbrna, name="trna.efn.descr", chosen_by="trna.descr"):
    """A few kilobases of the reference's test database with records of trna.descr, chosen as test_scan_end_gpu.py's first case
    chooses them (chosen_by: the descriptor whose records choose the entries); the descriptor is descr/trna.descr
    (trna.efn.descr of the work directory), whose score section calls efn() -- what bench.py scans with -- or the one named."""
    import rnamotif_amd as R
    d_by = _descr(workdir, chosen_by)
    entries = [r[2] for r in R.read_fasta(gbrna)[:400]]
    found = _oracle(d_by, (chosen_by, 400), entries)
    with_hits = sorted(set(found[:, 0].tolist()))[:6]
    assert len(with_hits) >= 2
    seqs = [entries[i] for i in with_hits] + entries[:3]
    assert sum(map(len, seqs)) < 40_000
    d = R.Descriptor(["-descr", name]) if os.sep in name else _descr(workdir, name)
    return d, seqs, _oracle(d, os.path.basename(name), seqs)


def test_three_scans(built, workdir, gbrna):
    """(1) trna.descr on one scanner: no tail ahead in the first scan, taken in the second and third, one energy launch each"""
    import rnamotif_amd as R
    d, seqs, want = _trna_case(workdir, gbrna)
    assert want.shape[0] >= 2 and d.n_efn_sites == 1
    sc = R.Scanner(d)
    db = sc.database(seqs)
    assert scan(sc, db, want, "first") == (2, 0, 1, 1)
    assert scan(sc, db, want, "second") == (1, 1, 1, 1)
    assert scan(sc, db, want, "third") == (1, 1, 1, 1)
    assert sc.last_kernel_ms()[2] > 0
    scan_off(sc, db, want, "trna")
    assert scan(sc, db, want, "after spec_tail 0") == (1, 1, 1, 1)
    db.close()
    sc.close()


def test_a_miss(built, paths):
    """(2) few records, then more than 1.25 x as many and more than the least a tail is planned for: the tail is done again, two
    energy launches; the same database again: taken.  The second run of the energies over the same records changes none."""
    import rnamotif_amd as R
    d = R.Descriptor(["-descr", paths["hairpin_efn.descr"]])
    few, many = [SC.random_bases(11, 900)], [SC.random_bases(12, 9_000), SC.random_bases(13, 70)]
    want_few, want_many = _oracle(d, "hairpin-few", few), _oracle(d, "hairpin-many", many)
    assert 2 <= want_few.shape[0] < TAIL_MIN and want_many.shape[0] > max(TAIL_MIN, want_few.shape[0] * 5 // 4)
    assert len(np.unique(want_many[:, d.efn_off])) > 20
    sc = R.Scanner(d)
    db_few, db_many = sc.database(few), sc.database(many)
    assert scan(sc, db_few, want_few, "few") == (2, 0, 1, 1)
    assert scan(sc, db_many, want_many, "many: a miss") == (2, 0, 1, 2)
    assert scan(sc, db_many, want_many, "many again") == (1, 1, 1, 1)
    assert scan(sc, db_few, want_few, "few again") == (1, 1, 1, 1)
    scan_off(sc, db_many, want_many, "many")
    for light in (0, 1):        # (both energy kernels with the count on the device)
        sc.set_option("efn_light", light)
        assert scan(sc, db_many, want_many, ("efn_light", light)) == (1, 1, 1, 1)
    db_few.close()
    db_many.close()
    sc.close()


def test_few_records_after_many(built, paths):
    """(3) 0, 1 and 2 records after a scan with thousands: none and one keep their own ways out -- a single record's order word
    is 0 --, two are taken"""
    import rnamotif_amd as R
    d = R.Descriptor(["-descr", paths["one.descr"]])
    sc = R.Scanner(d)
    many = [b"aaa"] + [SC.ONE_SITE] * 3_000
    want = _oracle(d, "one-many", many)
    assert want.shape[0] == 3_000
    db = sc.database(many)
    assert scan(sc, db, want, "many") == (2, 0, 1, 0)
    db.close()
    for count, taken in ((2, 1), (1, 0), (0, 0), (2, 1)):
        seqs = [b"aaa", b"a" * 100] + [SC.ONE_SITE] * count
        want = _oracle(d, ("one", count), seqs)
        assert want.shape[0] == count
        db = sc.database(seqs)
        end = scan(sc, db, want, ("few", count))
        assert end == (2 if count == 1 else 1, taken, 1, 0), (count, end)
        if count == 1:
            assert want[0, 4] == 0 and int(sc.scan_tensor(db)[0, 4]) == 0
        assert sc.last_kernel_ms()[2] == 0
        scan_off(sc, db, want, ("few", count))
        db.close()
    sc.close()


@pytest.mark.parametrize("n", [2, 3, 255, 256, 257, 1023, 1024, 1025, 8191, 8192, 8193])
def test_ordering_sizes(built, paths, n):
    """The ordering at the sizes where its sort takes another way -- one and two workgroups of the counting kernel's 32 pairs,
    a chunk of 1024 staged keys and one key more or less, the last size of the counting kernel and rocPRIM's first --,
    against the oracle's stable order.  At spec_tail 0 the ordering sorts exactly n pairs; with the tail ahead after it the
    plan is n + n / 4 (1024 at least) pairs of which those behind the n records are padding, all with the same key; and
    a scan of 2 records under that plan sorts 2 records among padding only."""
    import rnamotif_amd as R
    d = R.Descriptor(["-descr", paths["ss4_one.descr"]])
    seqs = [b"ac", SC.random_bases(n, n + 3), b"a"]
    want = _oracle(d, ("ss4-sizes", n), seqs)
    assert want.shape[0] == n
    two = [SC.random_bases(2, 5)]
    want_two = _oracle(d, ("ss4-sizes", "two"), two)
    assert want_two.shape[0] == 2
    sc = R.Scanner(d)
    db, db_two = sc.database(seqs), sc.database(two)
    sc.set_option("spec_tail", 0)
    assert _same(sc.scan(db), want) and sc.last_end()[1] == 0
    sc.set_option("spec_tail", -1)
    assert scan(sc, db, want, ("ahead", n)) == (1, 1, 1, 0)
    assert scan(sc, db_two, want_two, ("two among padding", n)) == (1, 1, 1, 0)
    db.close()
    db_two.close()
    sc.close()


def test_hit_buffer_edge(built, paths):
    """(4) The hit buffer's edge with a tail planned for all of it: 2^17 - 1 records on a fresh scanner (no tail ahead), then 2^17
    -- the buffer's and the plan's last record: taken --, then 2^17 + 1: the search is repeated into a larger buffer and the
    tail done again.  On the scanner that grew, the three again: one launch each, taken."""
    import rnamotif_amd as R
    d = R.Descriptor(["-descr", paths["ss4_one.descr"]])
    sc = R.Scanner(d)
    dbs = {}
    for count in (SC.HIT_CAP - 1, SC.HIT_CAP, SC.HIT_CAP + 1):
        seqs = SC.ss4_entries(count)
        want = _oracle(d, ("ss4", count), seqs)
        assert want.shape[0] == count
        dbs[count] = (sc.database(seqs), want)
    assert scan(sc, *dbs[SC.HIT_CAP - 1], "2^17 - 1, fresh") == (2, 0, 1, 0)
    assert scan(sc, *dbs[SC.HIT_CAP], "2^17") == (1, 1, 1, 0)
    end = scan(sc, *dbs[SC.HIT_CAP + 1], "2^17 + 1")
    assert end[1:] == (0, 2, 0), end
    for count in (SC.HIT_CAP - 1, SC.HIT_CAP, SC.HIT_CAP + 1):
        assert scan(sc, *dbs[count], ("grown", count)) == (1, 1, 1, 0)
    scan_off(sc, *dbs[SC.HIT_CAP + 1], "2^17 + 1")
    ten = sc.scan_tensor(dbs[SC.HIT_CAP][0]).cpu().numpy()
    assert _same(ten, dbs[SC.HIT_CAP][1]) and sc.last_end() == (1, 1, 1, 0)
    for db, _ in dbs.values():
        db.close()
    sc.close()


def test_order_words_beyond_the_key_field(built, paths):
    """(4) SS6's order words take 22 bits: the first scan is ordered on the host and widens the field, the second has its tail
    ahead and is taken.  Over the database of the clamped key the field cannot be widened: every tail ahead raises the flag and
    is done again, ordered on the host; SMALL fits and is taken."""
    import rnamotif_amd as R
    d = R.Descriptor(["-descr", paths["ss6.descr"]])
    seqs = SC.ss6_entries()
    want = _oracle(d, "ss6", seqs)
    assert want.shape[0] > 30_000 and want[:, 4].max() > 10_000
    sc = R.Scanner(d)
    db = sc.database(seqs)
    assert scan(sc, db, want, "ss6 first")[1:] == (0, 1, 0)
    assert scan(sc, db, want, "ss6 second") == (1, 1, 1, 0)
    scan_off(sc, db, want, "ss6")
    db.close()
    sc.close()
    seqs = SC.clamp_entries()
    want = _oracle(d, "ss6-clamp", seqs)
    assert want.shape[0] == 70_524
    sc = R.Scanner(d)
    db = sc.database(seqs)
    assert scan(sc, db, want, "ss6 clamped, first")[1:] == (0, 1, 0)
    end = scan(sc, db, want, "ss6 clamped, second: the flag")
    assert end[1:] == (0, 1, 0) and end[0] >= 2, end
    db.close()
    sc.close()
    d = R.Descriptor(["-descr", paths["small.descr"]])
    want = _oracle(d, "small-clamp", seqs)
    assert want.shape[0] == 162
    sc = R.Scanner(d)
    db = sc.database(seqs)
    assert scan(sc, db, want, "small first") == (2, 0, 1, 0)
    assert scan(sc, db, want, "small second") == (1, 1, 1, 0)
    scan_off(sc, db, want, "small")
    db.close()
    sc.close()


def test_piece_overflow(built, paths):
    """(4) DEEP: 78 records, then one piece of one item with 43 747 -- beyond the plan and beyond the piece's order words: the
    search is repeated with whole items and the tail done again; from then on one launch and taken."""
    import rnamotif_amd as R
    d = R.Descriptor(["-descr", paths["deep.descr"]])
    sparse, dense = SC.deep_sparse_entries(), SC.deep_dense_entries()
    want_sparse, want_dense = _oracle(d, "deep-sparse", sparse), _oracle(d, "deep-dense", dense)
    sc = R.Scanner(d)
    db_s, db_d = sc.database(sparse), sc.database(dense)
    assert scan(sc, db_s, want_sparse, "sparse") == (2, 0, 1, 0)
    assert scan(sc, db_d, want_dense, "dense")[1:] == (0, 2, 0)
    assert scan(sc, db_d, want_dense, "dense again") == (1, 1, 1, 0)
    assert scan(sc, db_s, want_sparse, "sparse again") == (1, 1, 1, 0)
    scan_off(sc, db_d, want_dense, "dense")
    db_s.close()
    db_d.close()
    sc.close()


@pytest.mark.parametrize("name,entries,env,opts,launches", [
    ("pk.descr", SC.pk_entries, {"RNAMOTIF_QCAP": "64", "RNAMOTIF_SPILL": "0"}, {}, 3),       # queue need, then the regrow
    ("dense.descr", SC.dense_entries, {}, {"flush": 1, "glist": 1}, 3),                       # list need, then the regrow
], ids=["general-queue", "lean-list"])
def test_a_repeat_under_a_tail_ahead(built, paths, name, entries, env, opts, launches):
    """(4) A scan without records, so that the next has its tail ahead; then between 2^17 and 2^18 records with a queue of 64 and
    no spill area (general instance) or a list of one item (the instance that walks nothing): the launches
    test_scan_end_gpu.py's case 2 states, the tail done again; the same database again repeats nothing and is taken."""
    import rnamotif_amd as R
    d = R.Descriptor(["-descr", paths[name]])
    seqs = entries()
    want = _oracle(d, name, seqs)
    assert SC.HIT_CAP < want.shape[0] < 2 * SC.HIT_CAP
    with _env(**env):
        sc = R.Scanner(d)
    for k, v in opts.items():
        sc.set_option(k, v)
    none = [b"a" * 200]
    want_none = _oracle(d, (name, "none"), none)
    assert want_none.shape[0] == 0
    db0 = sc.database(none)
    assert scan(sc, db0, want_none, "none")[1] == 0
    db0.close()
    db = sc.database(seqs)
    end = scan(sc, db, want, (name, "first"))
    assert end[1:3] == (0, launches), end
    assert scan(sc, db, want, (name, "second")) == (1, 1, 1, 0)
    scan_off(sc, db, want, name)
    db.close()
    sc.close()


@pytest.mark.parametrize("name", ["pk1.descr", os.path.join(ROOT, "tests", "data", "trna.efn2.descr")], ids=["pk1", "efn2"])
def test_general_instance_and_efn2(built, workdir, gbrna, name):
    """(5) pk1.descr -- the general instance, no drain kernel in front of the tail -- and a descriptor with an efn2() site"""
    import rnamotif_amd as R
    d, seqs, want = _trna_case(workdir, gbrna, name, "pk1.descr" if name == "pk1.descr" else "trna.descr")
    sc = R.Scanner(d)
    db = sc.database(seqs)
    assert want.shape[0] >= 2
    first = scan(sc, db, want, "first")
    assert first[:3] == (2, 0, 1) and first[3] == (1 if d.n_efn_sites else 0)
    assert scan(sc, db, want, "second") == (1, 1, 1, first[3])
    scan_off(sc, db, want, name)
    db.close()
    sc.close()


def test_two_scanners_in_turns(built, workdir, gbrna):
    """(6) Two scanners over one database, six steps in the order bench.py issues the calls: a step's begin, then the end of the
    step before.  Every step's records; from the third step on one wait, taken, and a launch shape that leaves the other
    scanner's drain kernel room."""
    import rnamotif_amd as R
    d, seqs, want = _trna_case(workdir, gbrna)
    scs = [R.Scanner(d), R.Scanner(d)]
    db = scs[0].database(seqs)
    for s in scs:
        s.attach(db)
    ends = []
    pend = None
    for i in range(6):
        s = scs[i & 1]
        s.scan_begin(db)
        if pend is not None:
            got = pend.scan_end(copy=False)
            assert _same(got, want), ("step", i - 1)
            ends.append((pend.last_end(), pend.last_launch()[3]))
        pend = s
    got = pend.scan_end(copy=False)
    assert _same(got, want), ("step", 5)
    ends.append((pend.last_end(), pend.last_launch()[3]))
    print(ends)
    for i, (end, beside) in enumerate(ends):
        if i < 2:
            assert end == (2, 0, 1, 1), (i, end)
        else:
            assert end == (1, 1, 1, 1) and beside == 1, (i, end, beside)
    db.close()
    for s in scs:
        s.close()


def test_device_consumers(built, workdir, gbrna):
    """(7) scan_end_on_device() and scan_tensor() after a tail ahead give the ordered records, and a consumer on the device
    prints from them what it prints from the records of a scan without one"""
    import rnamotif_amd as R
    d, seqs, want = _trna_case(workdir, gbrna)
    dev = torch.device("cuda", 0)
    sc = R.Scanner(d, device=0)
    flat = b"".join(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    db = sc.database_from_tensor(torch.frombuffer(bytearray(flat), dtype=torch.uint8).to(dev), offsets=off)
    first = sc.scan_tensor(db)
    assert sc.last_end()[1] == 0 and _same(first.cpu().numpy(), want)
    ahead = sc.scan_tensor(db)
    assert sc.last_end() == (1, 1, 1, 1) and _same(ahead.cpu().numpy(), want)
    sc.scan_begin(db)
    assert sc.scan_end_on_device() == want.shape[0] and sc.last_end() == (1, 1, 1, 1)
    prog = R.ScoreProgram(d, text=True)
    out = []
    for hits in (first, ahead):
        s = sc.score(db, hits, prog, text=True)
        p = sc.print_hits(db, hits, s)
        torch.cuda.synchronize()
        out.append((p.off.cpu().numpy(), p.bytes.cpu().numpy().tobytes()))
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1] and len(out[0][1]) > 0
    prog.close()
    db.close()
    sc.close()


def test_scan_device(built, workdir, gbrna, paths):
    """(8) scan_device() times the kernels apart: never a tail ahead, one energy launch, and an energy kernel's time only where
    there were records"""
    import rnamotif_amd as R
    d, seqs, want = _trna_case(workdir, gbrna)
    sc = R.Scanner(d)
    db, db0 = sc.database(seqs), sc.database([b"a" * 3_000])
    scan(sc, db, want, "a scan before")
    n, _, efn_ms = sc.scan_device(db)
    assert n == want.shape[0] and sc.last_end()[1:] == (0, 1, 1) and efn_ms > 0 and sc.last_kernel_ms()[2] > 0
    n, _, efn_ms = sc.scan_device(db0)
    assert n == 0 and sc.last_end()[1:] == (0, 1, 0) and efn_ms == 0 and sc.last_kernel_ms()[2] == 0
    got = sc.scan(db0)          # (a tail ahead over no records: its energy kernel had nothing to do)
    assert got.shape[0] == 0 and sc.last_end() == (1, 0, 1, 1) and sc.last_kernel_ms()[2] == 0
    assert scan(sc, db, want, "records again") == (1, 1, 1, 1) and sc.last_kernel_ms()[2] > 0
    db.close()
    db0.close()
    sc.close()
