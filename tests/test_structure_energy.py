"""GPU: efn() and efn2() of structures in device tensors (Scanner.structure_energies, rma_structure_energies: the check
and energy kernels of rm_structenergy_dev.hip) against the reference's drivers (the pins of the 783 + 40 structures of
tests/structure_energy.py) and, bit for bit, against the same rule and cores built for the host
(tests/hostsim/struct_energy_check.cpp):

  * every family in a call of its own and all of them in one shuffled batch -- 3 and 30 helices side by side, so both
    instances of the energy kernel run -- each with one workgroup (the grid-stride loops) and with the default grid;
  * batches of 1, 63, 64, 65 and 257 structures, hairpins of 96 and 97 bases (the LDS cache's last and the first
    structure read from the tensors), 15 and 16 helices (the last of the usual stacks, the first of the large ones),
    50 helices accepted and 51 refused with the outputs untouched;
  * hits of a scan expanded by hit_structures() and handed over as they are: the energies are the records' own words;
  * a letters table, one output only, missing tables, no structures, and scans that loading tables leaves alone.

torch is imported before the product library: one HIP runtime serves the process."""
import ctypes as C
import os

import torch  # noqa: F401  (first: its HIP runtime is the process's)

import numpy as np
import pytest

import rnamotif_amd as R
import structure_descr as S
import structure_energy as E

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
PLAIN = "descr\n\th5( len=3 )\n\t\tss( len=4 )\n\th3\n"          # no efn() / efn2(): the scanner has no tables of its own


@pytest.fixture(scope="module")
def families():
    return E.all_families()


@pytest.fixture(scope="module")
def host(families, tmp_path_factory):
    """{name: (efn, efn2)} of every structure of the families, from the host build -- computed once"""
    binary, _ = E.build_checker(sanitized=False)
    cases = [c for f in families.values() for c in f[0]]
    rows = E.host_batch(binary, str(tmp_path_factory.mktemp("host") / "b.txt"), *E.batch_of([c[1:] for c in cases]))
    assert rows[0] != "refused"
    return {"checker": binary, "dir": str(tmp_path_factory.mktemp("hostb")), **{c[0]: r[:2] for c, r in zip(cases, rows)}}


@pytest.fixture(scope="module")
def scanner(built, tmp_path_factory):
    path = tmp_path_factory.mktemp("plain") / "plain.descr"
    path.write_text(PLAIN)
    d = R.Descriptor(["-descr", str(path)])
    sc = R.Scanner(d, device=0)
    sc.load_energy_tables()
    yield sc
    sc.close()
    d.close()


def _dev(off, base, pair):
    return torch.from_numpy(off).to(DEV), torch.from_numpy(base.copy()).to(DEV), torch.from_numpy(pair).to(DEV)


def _energies(sc, structs, **kw):
    e, e2 = sc.structure_energies(*_dev(*E.batch_of(structs)), **kw)
    torch.cuda.synchronize()
    return (e.cpu().numpy() if e is not None else None), (e2.cpu().numpy() if e2 is not None else None)


def _host_of(host, structs):
    rows = E.host_batch(host["checker"], os.path.join(host["dir"], "b.txt"), *E.batch_of(structs))
    assert rows[0] != "refused", rows
    return np.array([r[0] for r in rows], dtype=np.int32), np.array([r[1] for r in rows], dtype=np.int32)


@pytest.mark.parametrize("wgs", [1, 0], ids=["one-workgroup", "default-grid"])
@pytest.mark.parametrize("family", ["efn_random", "efn2_closed", "directed", "large", "noncanonical", "all-shuffled"])
def test_families(scanner, families, host, family, wgs):
    if family == "all-shuffled":
        both = [(c, p) for f in families.values() for c, p in zip(*f)]
        order = np.random.default_rng(20261020).permutation(len(both))
        cases, pins = [both[k][0] for k in order], [both[k][1] for k in order]
        helices = {S._count(s, p)[1] for _, s, p in cases}
        assert {3, 30} <= helices
    else:
        cases, pins = families[family]
    scanner.set_option("struct_wgs", wgs)
    try:
        e, e2 = _energies(scanner, [c[1:] for c in cases])
    finally:
        scanner.set_option("struct_wgs", 0)
    bad = [(name, seq, pairs, "kernel efn %d efn2 %d" % (e[k], e2[k]), "drivers efn %r efn2 %r" % pins[k], "host %r" % (host[name],))
           for k, (name, seq, pairs) in enumerate(cases)
           if not S.energies_match(int(e2[k]), int(e[k]), pins[k], S.efn2_defined(seq, pairs)) or (int(e[k]), int(e2[k])) != host[name]]
    assert not bad, "%d disagreements, the first: %r" % (len(bad), bad[0])


@pytest.mark.parametrize("copies", [1, 63, 64, 65, 257])
def test_batch_sizes(scanner, families, host, copies):
    name, seq, pairs = families["efn_random"][0][3]
    e, e2 = _energies(scanner, [(seq, pairs)] * copies)
    assert e.shape == e2.shape == (copies,)
    assert (e == host[name][0]).all() and (e2 == host[name][1]).all()


def test_cache_and_instance_boundaries(scanner, host):
    structs = [E.hairpin(E.CACHE), E.hairpin(E.CACHE + 1), E.chain(E.SMALL_HELICES), E.chain(E.SMALL_HELICES + 1), E.chain(E.MAX_HELICES)]
    assert [len(s) for s, _ in structs[:2]] == [96, 97]
    assert [S._count(s, p)[1] for s, p in structs[2:]] == [15, 16, 50]
    want = _host_of(host, structs)
    for wgs in (1, 0):
        scanner.set_option("struct_wgs", wgs)
        try:
            got = _energies(scanner, structs)
            # (each alone as well: the batch with 16 helices launches both instances, the one of 15 only the usual one)
            alone = [_energies(scanner, [s]) for s in structs]
        finally:
            scanner.set_option("struct_wgs", 0)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (wgs, got, want)
        assert [int(a[0][0]) for a in alone] == list(want[0]) and [int(a[1][0]) for a in alone] == list(want[1]), wgs
    assert (want[0] < 0).all() and (want[1] < 0).all()          # (finite, every one)


def _call(sc, off, base, pair, e, e2, stride=1):
    err = C.create_string_buffer(4096)
    rc = R.lib().rma_structure_energies(sc._h, off.data_ptr(), base.data_ptr(), pair.data_ptr(), stride, int(off.shape[0]) - 1,
                                        int(base.shape[0]), None, e.data_ptr(), e2.data_ptr(),
                                        torch.cuda.current_stream(DEV).cuda_stream, err, 4096)
    torch.cuda.synchronize()
    return rc, err.value.decode()


def test_refusals_leave_the_outputs_untouched(scanner):
    good = E.hairpin(12)
    cases = [([good, E.chain(E.MAX_HELICES + 1), good], None, r"structure 1: 51 helices, more than 50: nothing written"),
             ([good, good, good], (12 + 5, 12), r"structure 1: base 5 pairs with 12, outside its 12 bases"),
             ([good, good, good], (24 + 5, 5), r"structure 2: base 5 pairs with itself"),
             ([good, good, good], (5, 6), r"structure 0: base 5 pairs with 6, which pairs with -1")]
    for structs, change, words in cases:
        off, base, pair = E.batch_of(structs)
        if change:
            pair[change[0]] = change[1]
        off, base, pair = _dev(off, base, pair)
        e = torch.full((len(structs),), -77, dtype=torch.int32, device=DEV)
        e2 = torch.full((len(structs),), -78, dtype=torch.int32, device=DEV)
        rc, msg = _call(scanner, off, base, pair, e, e2)
        assert rc != 0 and words in msg, msg
        assert (e == -77).all() and (e2 == -78).all(), msg
        with pytest.raises(R.RnamotifError, match=words.split(":")[0]):
            scanner.structure_energies(off, base, pair)
    # offsets: a decreasing off, a last one that is not the total; more bases than the logarithm tables have entries
    off, base, pair = E.batch_of([good, good, good])
    for at, v, words in ((2, 11, "structure 1: off decreases from 12 to 11"), (3, 35, "structure 2: off[ n ] is 35, not the 36")):
        o = off.copy()
        o[at] = v
        with pytest.raises(R.RnamotifError, match=words.replace("[", r"\[").replace("]", r"\]")):
            scanner.structure_energies(*_dev(o, base, pair))
    n = E.MAX_BASES + 1
    long_one = (torch.tensor([0, n], dtype=torch.int64, device=DEV), torch.full((n,), ord("a"), dtype=torch.uint8, device=DEV),
                torch.full((n,), -1, dtype=torch.int32, device=DEV))
    with pytest.raises(R.RnamotifError, match="structure 0: 8192 bases, more than 8191"):
        scanner.structure_energies(*long_one)
    e, e2 = scanner.structure_energies(long_one[0] - torch.tensor([0, 1], device=DEV), long_one[1][:-1], long_one[2][:-1])
    assert e.tolist() == [0] and e2.tolist() == [0]


def test_results_that_are_not_refusals(scanner):
    inf = (E.EFN_INF, E.EFN2_INF)
    off = np.array([0, 0, 8, 8, 12, 17], dtype=np.int64)
    pair = np.array([2, 3, 0, 1, -1, -1, -1, -1] + [-1, 2, 1, -1] + [-1] * 5, dtype=np.int32)
    base = np.frombuffer(b"gcgcaaaa" + b"agca" + b"acgua", dtype=np.uint8)
    e, e2 = scanner.structure_energies(*_dev(off, base, pair))
    assert list(zip(e.tolist(), e2.tolist())) == [inf, inf, inf, inf, (0, 0)]
    # no structures: nothing to do
    e, e2 = scanner.structure_energies(torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.uint8, device=DEV),
                                       torch.zeros(0, dtype=torch.int32, device=DEV))
    assert e.shape == e2.shape == (0,)


def test_letters_strides_and_single_outputs(scanner, families, host):
    cases = families["directed"][0][:30] + families["noncanonical"][0][:10]
    structs = [c[1:] for c in cases]
    off, base, pair = _dev(*E.batch_of(structs))
    want = (np.array([host[c[0]][0] for c in cases]), np.array([host[c[0]][1] for c in cases]))
    # tokens 0..4 through a letters table against the letters themselves
    lut = np.full(256, 9, dtype=np.uint8)
    for k, ch in enumerate(b"acgun"):
        lut[ch] = k
    tokens = torch.from_numpy(lut).to(DEV)[base.long()]
    letters = bytes(b"ACGUx"[b] if b < 5 else ord("a") for b in range(256))
    e, e2 = scanner.structure_energies(off, tokens, pair, letters=letters)
    assert np.array_equal(e.cpu().numpy(), want[0]) and np.array_equal(e2.cpu().numpy(), want[1])
    # partners as column 0 of a [T, 3] tensor, read in place, and as a strided 1-D view
    wide = torch.full((pair.shape[0], 3), -5, dtype=torch.int32, device=DEV)
    wide[:, 0] = pair
    for view in (wide, wide[:, 0], torch.stack([pair, pair], dim=1).reshape(-1)[::2]):
        e, e2 = scanner.structure_energies(off, base, view)
        assert np.array_equal(e.cpu().numpy(), want[0]) and np.array_equal(e2.cpu().numpy(), want[1]), view.stride()
    # one output only
    e, e2 = scanner.structure_energies(off, base, pair, efn2=False)
    assert e2 is None and np.array_equal(e.cpu().numpy(), want[0])
    e, e2 = scanner.structure_energies(off, base, pair, efn=False)
    assert e is None and np.array_equal(e2.cpu().numpy(), want[1])


def test_missing_tables_are_an_error_and_loading_changes_no_scan(built, families, host):
    d = R.Descriptor(["-descr", os.path.join(S.ROOT, "tests", "data", "hairpin.efn2.descr")])
    sc = R.Scanner(d, device=0)
    seqs = R.synthetic_records(1, length=20000)
    db = sc.database(seqs)
    before = sc.scan(db).copy()
    assert before.shape[0] > 0
    cases = families["efn2_closed"][0][:8]
    args = _dev(*E.batch_of([c[1:] for c in cases]))
    with pytest.raises(R.RnamotifError, match=r"no efn\(\) tables"):
        sc.structure_energies(*args)
    e, e2 = sc.structure_energies(*args, efn=False)             # (efn2's tables are the descriptor's)
    assert e2.tolist() == [host[c[0]][1] for c in cases]
    sc.scan_begin(db)
    with pytest.raises(R.RnamotifError, match="a scan is in flight"):
        sc.load_energy_tables(efn2=False)
    assert np.array_equal(sc.scan_end(), before)
    sc.load_energy_tables(efn2=False)
    e, e2 = sc.structure_energies(*args)
    assert e.tolist() == [host[c[0]][0] for c in cases] and e2.tolist() == [host[c[0]][1] for c in cases]
    assert np.array_equal(sc.scan(db), before)
    sc.load_energy_tables()
    assert np.array_equal(sc.scan(db), before)
    db.close()
    sc.close()
    d.close()


def test_hits_of_a_scan_hand_their_structures_over(built, tmp_path):
    """20 structures of `directed`, each scanned by its own descriptor as tests/test_efn_structures.py scans it; the
    records expanded by hit_structures(); off, base and the mate tensor -- column 0, stride 3 -- passed on as they are.
    Every record's window is the whole candidate, so the energies are the record's own efn2 and efn words, on both strands."""
    directed = S.families()["directed"]
    rng = np.random.default_rng(20261021)
    strands, n_records = set(), 0
    for name, seq, pairs in directed[::max(1, len(directed) // 20)][:20]:
        path = tmp_path / "s.descr"
        path.write_text(S.descriptor_of(seq, pairs))
        d = R.Descriptor(["-descr", str(path)])
        sc = R.Scanner(d, device=0)
        entries, planted = S.entries_of(seq, rng)
        text = torch.frombuffer(bytearray(b"".join(entries)), dtype=torch.uint8).to(DEV)
        db = sc.database_from_tensor(text, offsets=np.concatenate([[0], np.cumsum([len(s) for s in entries])]).astype(np.int64))
        hits = sc.scan_tensor(db)
        recs = hits.cpu().numpy()
        assert all(S.record_at(recs, *at).shape[0] == 1 for at in planted), name
        st = sc.hit_structures(db, hits)
        assert st.mate.shape[1] == 3 and st.mate.stride(0) == 3
        e, e2 = st.energies(sc)
        assert e.tolist() == recs[:, d.efn_off + 1].tolist() and e2.tolist() == recs[:, d.efn_off].tolist(), name
        e, e2 = sc.structure_energies(st.off, st.base, st.mate[:, 0])
        assert e.tolist() == recs[:, d.efn_off + 1].tolist() and e2.tolist() == recs[:, d.efn_off].tolist(), name
        strands |= set(recs[:, 1].tolist())
        n_records += recs.shape[0]
        db.close()
        sc.close()
        d.close()
    assert strands == {0, 1} and n_records >= 80
