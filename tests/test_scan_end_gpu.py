"""GPU: what runs behind the search kernel, at the sizes where it takes another branch -- search_finish() and scan_end()
(rm_scanner.cpp), DevHitSort::run() (rm_hitsort_dev.hip), the stride loop of efn_body (rm_scan_kernel.h) -- against the oracle,
word for word: the edge of the hit buffer and its regrow (count-then-emit) on lean and general instances, alone and in one scan
with a queue or list repeat; energies over more records than a pass of either energy kernel takes; order words beyond the
ordering's key field (host ordering, the field widened for the next scan) and a key whose other fields clamp it; a piece of an
item beyond 2^12 candidates (the scanner goes over to whole items); one record, and none, after scans that grew the buffers.

Every scan is observed: launches of the search kernel are the "[dbg] queued items:" lines of a dbg bit that only counts, and
"[timing] ordered" against "[timing] ordering" says where the records were ordered.  The cases and their premises are
tests/scan_end_cases.py's, proved on the CPU by tests/test_scan_end_cpu.py; what only a device can show -- launch counts, the
ordering's side, records against the grid -- is asserted here, so a premise that fails fails the test.

Oracle's counts (tests/test_scan_end_cpu.py): PK 194 682 records, DENSE 190 410, the hairpins 377 690 each (efn and efn2) over
1 050 071 bases, SS6 31 994 and over the database of the clamped key 70 524 (SMALL 162), DEEP 43 747 dense and 78 sparse."""
import numpy as np
import pytest
import torch  # noqa: F401  (first: its HIP runtime is the process's)

import scan_end_cases as SC
from test_gpu_parity import _env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return SC.write_all(tmp_path_factory.mktemp("scan_end"))


_WANT = {}


def _oracle(d, key, seqs):
    """the oracle's records, once per key"""
    from oracle_binding import oracle_scan
    if key not in _WANT:
        _WANT[key] = oracle_scan(d, seqs)
        _WANT[key].setflags(write=False)
    return _WANT[key]


def _descriptor(paths, name):
    import rnamotif_amd as R
    return R.Descriptor(["-descr", paths[name]])


def _scanner(d):
    """a scanner that says what it does: a line per launch of the search kernel, the laps of scan_end()"""
    import rnamotif_amd as R
    sc = R.Scanner(d)
    sc.set_option("dbg", R.DBG["COUNT_QUEUED"])
    sc.set_option("timing", 1)
    return sc


def observe(capfd, call):
    """(what call() returns, launches of the search kernel, "device" | "host" | None: where the records were ordered --
    None: nowhere, there were none or one)"""
    capfd.readouterr()
    out = call()
    err = capfd.readouterr().err
    on_device, on_host = "[timing] ordered" in err, "[timing] ordering" in err
    assert not (on_device and on_host), err
    return out, err.count("[dbg] queued items:"), "device" if on_device else "host" if on_host else None


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def check_scan(capfd, sc, db, want, launches, side, what, tensor_side="same"):
    """Scanner.scan() gives the oracle's records after so many launches, ordered on that side; so does the same scanner with
    host_sort = 1, and scan_tensor() (records left on the device), both without a repeat: the buffers are there by then.
    launches None: one at most (a database without a start position launches nothing)."""
    n = want.shape[0]
    got, k, s = observe(capfd, lambda: sc.scan(db))
    assert _same(got, want), (what, got.shape, want.shape)
    assert (k <= 1 if launches is None else k == launches), (what, "launches", k)
    assert s == (side if n >= 2 else None), (what, "ordered on", s)
    sc.set_option("host_sort", 1)
    host, k, s = observe(capfd, lambda: sc.scan(db))
    sc.set_option("host_sort", 0)
    assert _same(host, want), (what, "host_sort")
    assert k <= 1 and s == ("host" if n >= 1 else None), (what, "host_sort", k, s)
    ten, k, s = observe(capfd, lambda: sc.scan_tensor(db).cpu().numpy())
    assert _same(ten, want), (what, "scan_tensor")
    assert k <= 1 and s == ((side if tensor_side == "same" else tensor_side) if n >= 2 else None), (what, "scan_tensor", k, s)


def test_the_observer_itself(built, workdir, gbrna, capfd):
    """trna.descr over a few kilobases of the reference's test database: the oracle's records, one launch, ordered on the device"""
    import rnamotif_amd as R
    from test_gpu_parity import _descr
    d = _descr(workdir, "trna.descr")
    entries = [r[2] for r in R.read_fasta(gbrna)[:400]]
    found = _oracle(d, "trna400", entries)
    with_hits = sorted(set(found[:, 0].tolist()))[:6]
    assert len(with_hits) >= 2
    seqs = [entries[i] for i in with_hits] + entries[:3]
    want = _oracle(d, "trna", seqs)
    assert want.shape[0] >= 2 and sum(map(len, seqs)) < 40_000
    sc = _scanner(d)
    db = sc.database(seqs)
    got, launches, side = observe(capfd, lambda: sc.scan(db))
    assert _same(got, want) and (launches, side) == (1, "device")
    sc.set_option("host_sort", 1)
    got, launches, side = observe(capfd, lambda: sc.scan(db))
    assert _same(got, want) and (launches, side) == (1, "host")
    db.close()
    sc.close()


def test_hit_buffer_edge(built, paths, capfd):
    """Case 1.  2^17 - 1, 2^17 and 2^17 + 1 records on fresh scanners: 1, 1 and 2 launches.  The scanner that grew: three times
    the cap (grows again), the first database again (no repeat), then 3 records, 1 -- order word 0 -- and none."""
    d = _descriptor(paths, "ss4_one.descr")
    sc = None
    for count, launches in SC.SS4_FRESH:
        seqs = SC.ss4_entries(count)
        want = _oracle(d, ("ss4", count), seqs)
        assert want.shape[0] == count
        if sc is not None:
            sc.close()
        sc = _scanner(d)
        db = sc.database(seqs)
        check_scan(capfd, sc, db, want, launches, "device", ("fresh", count))
        db.close()
    for count, launches in SC.SS4_GROWN:
        seqs = SC.ss4_entries(count)
        want = _oracle(d, ("ss4", count), seqs)
        assert want.shape[0] == count
        db = sc.database(seqs)
        check_scan(capfd, sc, db, want, launches, "device", ("grown", count))
        if count == 1:
            assert sc.scan(db)[0, 4] == 0 and int(sc.scan_tensor(db)[0, 4]) == 0
        db.close()
    sc.close()


def test_hit_buffer_edge_both_strands(built, paths, capfd):
    """2^17 + 2 records, half of them on the other strand: 2 launches, then 1"""
    d = _descriptor(paths, "ss4_both.descr")
    seqs = SC.ss4_entries(SC.SS4_BOTH_WINDOWS)
    want = _oracle(d, "ss4_both", seqs)
    assert want.shape[0] == SC.HIT_CAP + 2
    sc = _scanner(d)
    db = sc.database(seqs)
    check_scan(capfd, sc, db, want, 2, "device", "first")
    check_scan(capfd, sc, db, want, 1, "device", "second")
    db.close()
    sc.close()


@pytest.mark.parametrize("name,entries,env,opts,first", [
    ("pk.descr", SC.pk_entries, {}, {}, 2),
    ("pk.descr", SC.pk_entries, {"RNAMOTIF_QCAP": "64", "RNAMOTIF_SPILL": "0"}, {}, 3),       # queue need, then the regrow
    ("dense.descr", SC.dense_entries, {}, {}, 2),
    ("dense.descr", SC.dense_entries, {}, {"flush": 1, "glist": 1}, 3),                       # list need, then the regrow
], ids=["general", "general-queue", "lean", "lean-list"])
def test_regrow_and_a_second_reason(built, paths, capfd, name, entries, env, opts, first):
    """Case 2.  Between 2^17 and 2^18 records: a fresh scanner repeats the search once for the hit buffer -- and once more before
    that where the first pass had no room for its items: a queue of 64 without a spill area (general instance), a list of one
    item behind the search kernel that walks nothing (lean) --; its second scan of the database repeats nothing."""
    d = _descriptor(paths, name)
    seqs = entries()
    want = _oracle(d, name, seqs)
    assert SC.HIT_CAP < want.shape[0] < 2 * SC.HIT_CAP
    with _env(**env):
        sc = _scanner(d)
    for k, v in opts.items():
        sc.set_option(k, v)
    db = sc.database(seqs)
    check_scan(capfd, sc, db, want, first, "device", (name, env, opts, "first"))
    check_scan(capfd, sc, db, want, 1, "device", (name, env, opts, "second"))
    db.close()
    sc.close()


@pytest.mark.parametrize("name", ["hairpin_efn.descr", "hairpin_efn2.descr"])
def test_energies_beyond_one_grid_pass(built, paths, capfd, name):
    """Case 3.  More records than the lanes of either energy kernel's grid, and a quarter more: every lane strides on to a second
    candidate (window and LDS row of its first one behind it), some to none.  The first scan has regrown the hit buffer."""
    d = _descriptor(paths, name)
    seqs = SC.hairpin_entries()
    want = _oracle(d, name, seqs)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = want.shape[0]
    assert n > SC.efn_need(cus, True), "%d records do not reach 1.25 x %d CUs x %d: the light energy kernel makes one pass" % (n, cus, SC.EFN_LIGHT_PER_CU)
    assert n > SC.efn_need(cus, False), "%d records do not reach 1.25 x %d CUs x %d: the staged energy kernel makes one pass" % (n, cus, SC.EFN_BLOCK)
    assert len(np.unique(want[:, d.efn_off])) > 50
    sc = _scanner(d)
    db = sc.database(seqs)
    launches = 2
    for light in (0, 1):
        sc.set_option("efn_light", light)
        check_scan(capfd, sc, db, want, launches, "device", (name, "efn_light", light))
        launches = 1
    db.close()
    sc.close()


def test_order_words_beyond_the_key_field(built, paths, capfd):
    """Case 4.  SS6's order words take 22 bits, the key's field has 20: the first scan of a fresh scanner is ordered on the host
    and widens the field, the second on the device.  A fresh scanner whose first call is scan_tensor(): the host's order, copied
    back into the hit buffer."""
    d = _descriptor(paths, "ss6.descr")
    seqs = SC.ss6_entries()
    want = _oracle(d, "ss6", seqs)
    assert want.shape[0] > 30_000 and want[:, 4].max() > 10_000
    sc = _scanner(d)
    db = sc.database(seqs)
    got, launches, side = observe(capfd, lambda: sc.scan(db))
    assert side == "host", "the first scan's order words fit %d bits: ordered on the %s" % (SC.W_ORD, side)
    assert _same(got, want) and launches == 1
    check_scan(capfd, sc, db, want, 1, "device", "second")
    db.close()
    sc.close()
    sc = _scanner(d)
    db = sc.database(seqs)
    ten, launches, side = observe(capfd, lambda: sc.scan_tensor(db).cpu().numpy())
    assert (launches, side) == (1, "host") and _same(ten, want)
    ten, launches, side = observe(capfd, lambda: sc.scan_tensor(db).cpu().numpy())
    assert (launches, side) == (1, "device") and _same(ten, want)
    db.close()
    sc.close()


def test_order_field_clamped(built, paths, capfd):
    """Case 5.  2^16 + 1 entries of one base and one of 2^21 + 999: entry, strand, position and rank leave the order word 16 bits
    of the key, whatever the field's own width: SS6 is ordered on the host in every scan, SMALL -- 6 bits -- on the device."""
    seqs = SC.clamp_entries()
    d = _descriptor(paths, "ss6.descr")
    want = _oracle(d, "ss6-clamp", seqs)
    assert want.shape[0] == 70_524
    sc = _scanner(d)
    db = sc.database(seqs)
    check_scan(capfd, sc, db, want, 1, "host", "ss6 first")
    check_scan(capfd, sc, db, want, 1, "host", "ss6 second")
    db.close()
    sc.close()
    d = _descriptor(paths, "small.descr")
    want = _oracle(d, "small-clamp", seqs)
    assert want.shape[0] == 162
    sc = _scanner(d)
    db = sc.database(seqs)
    check_scan(capfd, sc, db, want, 1, "device", "small first")
    check_scan(capfd, sc, db, want, 1, "device", "small second")
    db.close()
    sc.close()


def test_piece_overflow(built, paths, capfd):
    """Case 6.  DEEP's order words are counts.  One piece of one item with 43 747 candidates: the scan is repeated with whole
    items, and the scanner stays with them."""
    import rnamotif_amd as R
    d = _descriptor(paths, "deep.descr")
    sparse, dense = SC.deep_sparse_entries(), SC.deep_dense_entries()
    want_sparse, want_dense = _oracle(d, "deep-sparse", sparse), _oracle(d, "deep-dense", dense)
    assert want_dense.shape[0] > 10 << SC.PIECE_ORDER_BITS and 2 <= want_sparse.shape[0] < 1 << SC.PIECE_ORDER_BITS
    sc = _scanner(d)
    db_s, db_d = sc.database(sparse), sc.database(dense)
    check_scan(capfd, sc, db_s, want_sparse, 1, "device", "sparse")
    got, launches, side = observe(capfd, lambda: sc.scan(db_d))
    assert launches == 2, "%d launch(es), search and drain workgroups %s: no piece of an item found 2^%d candidates" % (
        launches, sc.last_launch()[::2], SC.PIECE_ORDER_BITS)
    assert _same(got, want_dense) and side == "device"
    check_scan(capfd, sc, db_d, want_dense, 1, "device", "dense again")
    check_scan(capfd, sc, db_s, want_sparse, 1, "device", "sparse again")
    sc.set_option("dbg", R.DBG["COUNT_QUEUED"] | R.DBG["WHOLE_ITEMS"])
    check_scan(capfd, sc, db_d, want_dense, 1, "device", "dense, whole items forced")
    db_s.close()
    db_d.close()
    sc.close()


@pytest.mark.parametrize("k", range(3), ids=["lean-numbered", "lean-counted", "general"])
def test_single_record(built, paths, capfd, k):
    """Case 7.  One site, one record, nothing to order: its order word is 0, on the host and left on the device."""
    name, seqs = SC.single_cases()[k]
    d = _descriptor(paths, name)
    want = _oracle(d, ("single", k), seqs)
    assert want.shape[0] == 1 and want[0, 4] == 0
    sc = _scanner(d)
    db = sc.database(seqs)
    check_scan(capfd, sc, db, want, 1, None, name)
    check_scan(capfd, sc, db, want, 1, None, (name, "second"))
    db.close()
    sc.close()
