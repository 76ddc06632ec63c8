"""CPU: rma_structure_energies' rule (rnamotif_amd/csrc/rm_structenergy.h) compiled for the host by
tests/hostsim/struct_energy_check.cpp -- the check of a batch and efn() / efn2() of its structures through the cores
rm_efn_core.h / rm_efn2_core.h, straight from (seq, pairs) with no descriptor in between: with the int16 table image
the kernel stages, without and with the cache of codes and partners, with the instance of the cores the helix count
picks.  The 783 structures of structure_descr.families() must give what the reference's efn_drv / efn2_drv gave
(tests/golden/ref_pins.json), the 40 of the family `noncanonical` what they gave for those
(tests/golden/structure_energy_pins.json); every refusal names its structure and reason; random pair tables with
crossing pairs give both infinities; and the same program built with -fsanitize=address,undefined runs all of it clean.
tests/test_structure_energy.py runs the same structures through the kernels."""
import numpy as np
import pytest

import structure_descr as S
import structure_energy as E


@pytest.fixture(scope="module")
def checker():
    return E.build_checker()


@pytest.fixture(scope="module")
def families():
    return E.all_families()


def _disagreements(rows, cases, pins):
    return [(name, seq, pairs, "efn %d efn2 %d" % (r[0], r[1]), "drivers efn %r efn2 %r" % pin)
            for r, (name, seq, pairs), pin in zip(rows, cases, pins)
            if not S.energies_match(r[1], r[0], pin, S.efn2_defined(seq, pairs))]


@pytest.mark.parametrize("san", [0, 1], ids=["plain", "sanitized"])
def test_families_agree_with_the_drivers(checker, families, tmp_path, san):
    """all 783 + 40 structures in one batch; efn2 is 9999999 where efn2_defined is false"""
    assert sum(len(c) for c, _ in families.values()) == 783 + 40
    cases = [c for f in families.values() for c in f[0]]
    pins = [p for f in families.values() for p in f[1]]
    rows = E.host_batch(checker[san], str(tmp_path / "b.txt"), *E.batch_of([c[1:] for c in cases]))
    assert rows[0] != "refused", rows
    bad = _disagreements(rows, cases, pins)
    assert not bad, "%d disagreements, the first: %r" % (len(bad), bad[0])
    # the helix count is elements_of's; the large family, and it alone, takes the instance with the large stacks
    for r, (name, seq, pairs) in zip(rows, cases):
        assert r[2] == S._count(seq, pairs)[1] and r[3] == 0, name
    large = {c[0] for c in families["large"][0]}
    assert {name for r, (name, _, _) in zip(rows, cases) if r[2] > E.SMALL_HELICES} == large


def test_noncanonical_is_what_it_claims(families):
    cases, pins = families["noncanonical"]
    assert len(cases) == 40
    for name, seq, pairs in cases:
        odd = [seq[i] + seq[j] for i, j in pairs if seq[i] + seq[j] not in E._CANONICAL]
        assert 1 <= len(odd) <= 3, name
    # both kinds of efn2 are there, and some letter n is paired
    assert {S.efn2_defined(s, p) for _, s, p in cases} == {True, False}
    assert any("n" in seq[i] + seq[j] for _, seq, pairs in cases for i, j in pairs)


def _one(seq_len, pair):
    return np.array([0, seq_len], dtype=np.int64), np.frombuffer(b"a" * seq_len, dtype=np.uint8), np.asarray(pair, dtype=np.int32)


def test_refusals_name_index_and_reason(checker, tmp_path):
    path = str(tmp_path / "b.txt")
    good = E.hairpin(12)
    off, base, pair = E.batch_of([good, good, good])

    def with_pairs(change):
        p = pair.copy()
        change(p[12:24])                     # (structure 1)
        return E.host_batch(checker[0], path, off, base, p)

    def put(i, v):
        return lambda p: p.__setitem__(i, v)

    assert with_pairs(put(5, 12)) == ("refused", 1, "pair_range", 5)           # one past the structure's last base
    assert with_pairs(put(5, -2)) == ("refused", 1, "pair_range", 5)
    assert with_pairs(put(5, 5)) == ("refused", 1, "pair_self", 5)
    assert with_pairs(put(5, 6)) == ("refused", 1, "pair_asym", 5)             # 6 does not return it
    assert with_pairs(put(0, -1)) == ("refused", 1, "pair_asym", 11)           # 11 still points at 0
    assert with_pairs(put(5, -1))[0] != "refused"
    # the lowest bad structure is the one named
    p = pair.copy()
    p[24 + 5] = 5
    p[12 + 4] = 4
    assert E.host_batch(checker[0], path, off, base, p) == ("refused", 1, "pair_self", 4)
    # offsets
    for change, want in (((0, 1), ("refused", 0, "off_first", 0)), ((2, 11), ("refused", 1, "off_decreases", 0)),
                         ((3, 35), ("refused", 2, "off_last", 0)), ((3, 37), ("refused", 2, "off_outside", 0))):
        o = off.copy()
        o[change[0]] = change[1]
        assert E.host_batch(checker[0], path, o, base, pair) == want, change
    # 50 helices accepted, 51 refused; 8191 bases accepted, 8192 refused
    for n, ok in ((E.MAX_HELICES, True), (E.MAX_HELICES + 1, False)):
        got = E.host_batch(checker[0], path, *E.batch_of([good, E.chain(n)]))
        assert (got[1][2] == n) if ok else (got == ("refused", 1, "helices", n))
    for n, ok in ((E.MAX_BASES, True), (E.MAX_BASES + 1, False)):
        got = E.host_batch(checker[0], path, *_one(n, [-1] * n))
        assert (got[0][:2] == (0, 0)) if ok else (got == ("refused", 0, "too_long", 0))


def test_results_that_are_not_refusals(checker, tmp_path):
    """no bases, crossing pairs and a pair (i, i+1) give both infinities; an unpaired structure is worth nothing"""
    inf = (E.EFN_INF, E.EFN2_INF)
    off = np.array([0, 0, 8, 8, 12, 17], dtype=np.int64)
    pair = np.array([2, 3, 0, 1, -1, -1, -1, -1] + [-1, 2, 1, -1] + [-1] * 5, dtype=np.int32)
    rows = E.host_batch(checker[0], str(tmp_path / "b.txt"), off, np.frombuffer(b"gcgcaaaa" + b"agca" + b"acgua", dtype=np.uint8), pair)
    assert [r[:2] for r in rows] == [inf, inf, inf, inf, (0, 0)]
    assert [r[3] for r in rows] == [0, 1, 0, 1, 0]


@pytest.mark.parametrize("san", [0, 1], ids=["plain", "sanitized"])
def test_fuzz(checker, san):
    """10 000 random symmetric pair tables of 2 to 200 bases, with crossing pairs wherever four bases allow them: each
    is accepted, flagged by the check exactly when a quadratic search finds a crossing (or a pair (i, i+1)) and then
    worth both infinities; and 10 000 random nested structures of any letters, which go through the cores -- cache or
    not, either instance -- to one value.  (Why crossing is found by the check and not left to the cores:
    rm_structenergy.h.)"""
    out = E.run_checker(checker[san], "cross", 20261018, 10000)
    assert out.startswith("10000 structures: ") and int(out.split()[2]) >= 9900, out
    out = E.run_checker(checker[san], "nested", 20261019, 10000)
    assert out.startswith("10000 structures: ") and int(out.split()[7]) >= 5000, out
