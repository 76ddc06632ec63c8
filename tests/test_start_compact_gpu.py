"""GPU: the search kernel that walks nothing (RMK_LEAN_FLUSH, RMK_LEAN_CONCAT_FLUSH) with the start positions taken out of the
start vector by one prefix sum a wave: records equal to the oracle's.

Descriptors and databases: tests/passa_cases.py, and one database more -- an entry of 20 000 bases with two runs of n beside
entries of 95 .. 129 bases --, so that under the default tile there are whole tiles (a wave's 1024 positions a step with
more survivors than its buffer holds at once, and with none), a partial last tile and the reverse strand's alignment, all
in one scan.  Two sequences that trna.descr matches are planted in the long entry: at its start, across
the end of the default plan's first tile, next to a run of n, and as the reverse complement.  tests/test_start_compact_cpu.py
shows on the CPU that the prefix sum hands on what the rounds of ballots handed on.  Option `flush` = 1 under
RNAMOTIF_SHORT = 0 and 2 and RNAMOTIF_TILE = 512 and the default.  Every database is scanned twice."""
import os

import numpy as np
import pytest

import passa_cases as PC

pytestmark = pytest.mark.gpu


# two matches of trna.descr, found by the oracle in the long entries of tests/flush_cases.py
PLANT = (b"tatagcaatgtgatgtgggggtaggtagcggtaattgttatcacgtgccacgccggccaatgcggaagttgttgctgtgggag",
         b"caagttgaacttcgtggttgttgggcattcgtcggctgaagggcggagtgatttttccctttagggagcttggaat")


def mixed_database():
    rng = np.random.default_rng(20261)
    lut = np.frombuffer(b"acgt", dtype=np.uint8)
    a = lut[rng.integers(0, 4, size=20_000)].copy()
    rc = bytes(reversed(PLANT[0].translate(bytes.maketrans(b"acgt", b"tgca"))))
    for at, text in ((3, PLANT[0]), (7_900, PLANT[0]), (7_990, PLANT[1]), (12_000, rc), (15_080, PLANT[0]), (19_900, PLANT[1])):
        a[at:at + len(text)] = np.frombuffer(text, dtype=np.uint8)
    a[7_860:7_893] = ord("n")
    a[15_000:15_070] = ord("n")
    return [lut[rng.integers(0, 4, size=n)].tobytes() for n in (95, 96, 97)] + [a.tobytes()] + \
           [lut[rng.integers(0, 4, size=n)].tobytes() for n in (127, 128, 129)]


@pytest.fixture(scope="module")
def cases(built, workdir):
    """name -> (descriptor, {database: (entries, the oracle's records)}), the oracle run once"""
    import rnamotif_amd as R
    from oracle_binding import oracle_scan
    for name, text in PC.WRITTEN.items():
        with open(os.path.join(workdir, name), "w") as f:
            f.write(text)
    dbs = dict(PC.databases(), mixed=mixed_database())
    out = {}
    cwd = os.getcwd()
    os.chdir(workdir)
    try:
        for name in PC.NAMES:
            d = R.Descriptor(["-descr", name])
            out[name] = (d, {k: (v, oracle_scan(d, v)) for k, v in dbs.items()})
    finally:
        os.chdir(cwd)
    return out


@pytest.mark.parametrize("name", PC.NAMES)
def test_start_positions_by_prefix_sum_equal_the_oracle(cases, name):
    import rnamotif_amd as R
    d, dbs = cases[name]
    # (on the CPU first: the long entries and the database added here hold something to find)
    for which in ("long", "mixed"):
        assert dbs[which][1].shape[0] > 0, (name, which)
    keys = ("RNAMOTIF_SHORT", "RNAMOTIF_TILE")
    old = {k: os.environ.get(k) for k in keys}
    try:
        for short in PC.SHORT:
            for tile in PC.TILE:
                os.environ["RNAMOTIF_SHORT"] = short
                os.environ.pop("RNAMOTIF_TILE", None)
                if tile:
                    os.environ["RNAMOTIF_TILE"] = tile
                sc = R.Scanner(d)          # (the environment is read when the scanner is created)
                sc.set_option("flush", 1)
                for which, (seqs, want) in dbs.items():
                    db = sc.database(seqs)
                    for _ in range(2):
                        got = sc.scan(db)
                        assert got.shape == want.shape and np.array_equal(got, want), (name, short, tile, which)
                    db.close()
                sc.close()
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
