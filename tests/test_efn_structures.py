"""GPU: the energy kernel (rm_scan_kernel.h efn_body: the LDS int16 table image, the per-lane cache of codes and
partners for calls of up to 96 bases and the walk from the hit record for longer ones, the interval stacks that
replace recursion, the instance with the large stacks) on arbitrary nested structures: the four families of
tests/structure_descr.py, each structure the single candidate of its own descriptor, scanned as a small database --
alone, behind a flank (the window across a boundary of the packed words and at the entry's last base), between two
flanks, and as its reverse complement.  Records equal the oracle's bit for bit; the energies of the planted
candidates equal what the reference's efn_drv / efn2_drv gave for the structure (tests/golden/ref_pins.json; the
drivers themselves are not needed here)."""
import numpy as np
import pytest

import structure_descr as S

CHUNK = 50
FAMILIES = S.families()
CHUNKS = [(f, lo) for f, cases in FAMILIES.items() for lo in range(0, len(cases), CHUNK)]


@pytest.fixture(scope="module")
def pins():
    return {f: S.pins(f, cases) for f, cases in FAMILIES.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("family,lo", CHUNKS, ids=["%s-%d" % c for c in CHUNKS])
def test_kernel_energies_of_structures(built, pins, tmp_path, family, lo):
    import rnamotif_amd as R
    from oracle_binding import oracle_scan
    rng = np.random.default_rng(1000 + lo)
    bad = []
    for k, (name, seq, pairs) in enumerate(FAMILIES[family][lo:lo + CHUNK]):
        pin = pins[family][lo + k]
        path = tmp_path / "s.descr"
        path.write_text(S.descriptor_of(seq, pairs))
        d = R.Descriptor(["-descr", str(path)])
        entries, planted = S.entries_of(seq, rng)
        sc = R.Scanner(d)                      # (a refusal here is a finding: no structure is skipped)
        db = sc.database(entries)
        got = sc.scan(db)
        want = oracle_scan(d, entries)
        if got.shape != want.shape or not np.array_equal(got, want):
            bad.append((name, seq, pairs, "records differ from the oracle's", got.shape, want.shape))
        else:
            for entry, strand, start in planted:
                row = S.record_at(got, entry, strand, start)
                if row.shape[0] != 1:
                    bad.append((name, seq, pairs, (entry, strand, start), "%d records" % row.shape[0]))
                    continue
                e2, e = int(row[0, d.efn_off]), int(row[0, d.efn_off + 1])
                if not S.energies_match(e2, e, pin, S.efn2_defined(seq, pairs)):
                    bad.append((name, seq, pairs, (entry, strand, start), "kernel efn2 %d efn %d" % (e2, e), "drivers efn %r efn2 %r" % pin))
        db.close()
        sc.close()
        d.close()
    assert not bad, "%d disagreements, the first: %r" % (len(bad), bad[0])
