"""GPU: the search kernel that walks nothing (RMK_LEAN_FLUSH, RMK_LEAN_CONCAT_FLUSH) after its look-ahead chain takes
its window ORs by doubling shifts (rmd_or_window) and reads the cores' vectors without a test and a wait each: records
equal to the oracle's.

Descriptors and databases: tests/flush_cases.py -- trna.descr, bulge.descr, a chain with a group wider than a word
behind a leaf, a chain with two shapes of leaf; entries whose vectors end at the edge of a read, long entries with runs
of n.  tests/test_flush_vectors_cases.py shows on the CPU that the chains have these shapes and which instance every
case launches.  Option `flush` = 1 under RNAMOTIF_SHORT = 0, 1 and 2 and RNAMOTIF_TILE = 512, 2048 and the default, so
that vectors end inside and outside entries.  Every case is scanned twice."""
import os

import numpy as np
import pytest

import flush_cases as FC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(built, workdir):
    """name -> (descriptor, {database: (entries, the oracle's records)}), the oracle run once"""
    import rnamotif_amd as R
    from oracle_binding import oracle_scan
    for name, text in FC.WRITTEN.items():
        with open(os.path.join(workdir, name), "w") as f:
            f.write(text)
    dbs = FC.databases()
    out = {}
    cwd = os.getcwd()
    os.chdir(workdir)
    try:
        for name in FC.NAMES:
            d = R.Descriptor(["-descr", name])
            out[name] = (d, {k: (v, oracle_scan(d, v)) for k, v in dbs.items()})
    finally:
        os.chdir(cwd)
    return out


@pytest.mark.parametrize("name", FC.NAMES)
def test_flush_instances_equal_the_oracle(cases, name):
    import rnamotif_amd as R
    d, dbs = cases[name]
    # (on the CPU first: the inputs hold something to find)
    assert dbs["long"][1].shape[0] > 0, name
    keys = ("RNAMOTIF_SHORT", "RNAMOTIF_TILE")
    old = {k: os.environ.get(k) for k in keys}
    try:
        for short in FC.SHORT:
            for tile in FC.TILE:
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
