"""GPU: the search kernel that walks nothing (RMK_LEAN_FLUSH, RMK_LEAN_CONCAT_FLUSH) with the look-ahead chain's end window
on its end positions and pass A' on quads of lanes: records equal to the oracle's.

Descriptors and databases: tests/passa_cases.py -- trna.descr; chains with two and three outer lengths; a tail stem-loop
with two helix and two loop lengths and single strand behind it; a tail that is no leaf (no end window); a range of single
strand in front of the first interior helix; outer helices of one and of four lengths; entries of 95 .. 129 bases, whose
end positions lie at the vectors' and the entries' edges, and long ones with runs of n.  tests/test_passa_cpu.py shows on
the CPU what each descriptor exercises.  Option `flush` = 1 under RNAMOTIF_SHORT = 0 and 2 and RNAMOTIF_TILE = 512 and the
default.  Every database is scanned twice."""
import os

import numpy as np
import pytest

import passa_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(built, workdir):
    """name -> (descriptor, {database: (entries, the oracle's records)}), the oracle run once"""
    import rnamotif_amd as R
    from oracle_binding import oracle_scan
    for name, text in PC.WRITTEN.items():
        with open(os.path.join(workdir, name), "w") as f:
            f.write(text)
    dbs = PC.databases()
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
def test_end_window_and_quads_equal_the_oracle(cases, name):
    import rnamotif_amd as R
    d, dbs = cases[name]
    # (on the CPU first: the inputs hold something to find)
    assert dbs["long"][1].shape[0] > 0, name
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
