"""CPU: efn() and efn2() of arbitrary nested structures -- each the single candidate of the descriptor
tests/structure_descr.py writes for it -- through the oracle (which must give what the reference's own efn_drv /
efn2_drv gave, tests/golden/ref_pins.json) and through the device cores rm_efn_core.h / rm_efn2_core.h compiled for
the host (tests/hostsim/hostsim_check.cpp: with the int16 table image the kernel stages, with and without the per-lane
cache of codes and partners, with the large stacks where the descriptor asks for them), which must give what the
oracle gives.  Four families: the 296 + 400 random structures of the two oracle tests, the directed structures and the
large ones.  tests/test_efn_structures.py runs the same structures through the kernels."""
import os
import re
import subprocess

import numpy as np
import pytest

import structure_descr as S
from test_hostsim import hostsim      # noqa: F401  (the fixture that builds tests/_build/hostsim_check)

CHUNK = 50
FAMILIES = S.families()
CHUNKS = [(f, lo) for f, cases in FAMILIES.items() for lo in range(0, len(cases), CHUNK)]


@pytest.fixture(scope="module")
def pins():
    return {f: S.pins(f, cases) for f, cases in FAMILIES.items()}


def test_descriptor_of_cuts_the_3prime_run_of_two_helices():
    # ((.(...)))  : the 3' run ")))" belongs to two helices
    seq, pairs = "ggacaaaguc", [(0, 9), (1, 8), (3, 7)]
    assert [e[:2] + e[3:] for e in S.elements_of(seq, pairs)] == [("h5", 0, 2), ("ss", None, 1), ("h5", 1, 1), ("ss", None, 3),
                                                                ("h3", 1, 1), ("h3", 0, 2)]
    text = S.descriptor_of(seq, pairs)
    assert "\th5(tag='h0',len=2)\n\tss(len=1)\n\th5(tag='h1',len=1)\n\tss(len=3)\n\th3(tag='h1')\n\th3(tag='h0')\n" in text
    assert "sprintf( '%8.3f %8.3f', efn2( h5[1], h3[6] ), efn( h5[1], h3[6] ) )" in text


def test_the_families_are_what_they_claim():
    """every directed and large structure has its feature; the features cover the list of the module's docstring"""
    directed, large = S.directed(), S.large()
    for name, seq, pairs, pred in directed + large:
        assert pred(seq, pairs), name
    sizes = {l[3] for _, s, p, _ in directed for l in S.loops_of(s, p) if l[0] == "hairpin"}
    assert {1, 2, 3, 4, 31, 32, 60, 150} <= sizes
    for kind in ("bulge", "interior"):
        totals = {l[3] + l[4] for _, s, p, _ in directed for l in S.loops_of(s, p) if l[0] == kind}
        assert {31, 32, 60} <= totals and totals & {150, 151}
    assert len(FAMILIES["efn_random"]) == 296 and len(FAMILIES["efn2_closed"]) == 400
    # the reference leaves the exterior loop of some undefined (structure_descr.efn2_defined): both kinds are there
    assert {S.efn2_defined(s, p) for _, s, p, _ in directed} == {True, False}


@pytest.mark.parametrize("family,lo", CHUNKS, ids=["%s-%d" % c for c in CHUNKS])
def test_oracle_equals_drivers_and_host_cores_equal_oracle(built, hostsim, pins, tmp_path, family, lo):    # noqa: F811
    import rnamotif_amd as R
    from oracle_binding import oracle_scan
    env = dict(os.environ, EFNDATA=S.EFNDATA)
    rng = np.random.default_rng(1000 + lo)
    bad = []
    for k, (name, seq, pairs) in enumerate(FAMILIES[family][lo:lo + CHUNK]):
        pin = pins[family][lo + k]
        path = tmp_path / "s.descr"
        path.write_text(S.descriptor_of(seq, pairs))
        d = R.Descriptor(["-descr", str(path)])             # (no structure may fail to compile)
        assert d.n_efn_sites == 2 and d.minlen == d.maxlen == len(seq), name
        entries, planted = S.entries_of(seq, rng)
        recs = oracle_scan(d, entries)
        for entry, strand, start in planted:
            row = S.record_at(recs, entry, strand, start)
            assert row.shape[0] == 1, (name, entry, row.shape)
            e2, e = int(row[0, d.efn_off]), int(row[0, d.efn_off + 1])
            if not S.energies_match(e2, e, pin, S.efn2_defined(seq, pairs)):
                bad.append((name, seq, pairs, (entry, strand, start), "oracle efn2 %d efn %d" % (e2, e), "drivers efn %r efn2 %r" % pin))
        d.close()
        fa = tmp_path / "s.fastn"
        fa.write_bytes(b"".join(b">e%d x\n%s\n" % (i, s) for i, s in enumerate(entries)))
        p = subprocess.run([hostsim, "-descr", str(path), str(fa)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        m = re.search(rb"(\d+) candidates, 0 mismatching strands \((\d+) efn2 energies compared\) \((\d+) efn energies compared\)", p.stdout)
        if p.returncode != 0 or not m or not (int(m.group(1)) == int(m.group(2)) == int(m.group(3)) >= len(planted)):
            bad.append((name, seq, pairs, p.stdout[-300:], p.stderr[-600:]))
        # (the cores' instance with the large stacks is the one under test where the kernel would launch it)
        assert (b"(large energy stacks)" in p.stdout) == (family == "large"), name
    assert not bad, "%d disagreements, the first: %r" % (len(bad), bad[0])
