"""GPU: the launch shape that leaves another scanner's drain kernel room (option beside) -- the same records as the solo
shape, word for word; two scanners taking eight steps in turns under default options, each step's records those of its
database alone; who plans beside and when (Scanner.last_launch()); the repeat launch of a list that overflowed keeps
the shape.  trna.descr over (a) 5 Mbase of synthetic records: 1270 tiles, more than four workgroups a CU on 256 CUs, so
the beside grid is really capped and drain waves really share CUs with four search workgroups; (b) the reference's
test database: the instance over the concatenation of short entries, 1351 candidates (the oracle's count, as bench.py
has it); (c) one record of 6000 bases: 2 tiles, a grid below every cap."""
import os

import torch  # noqa: F401  (first: its HIP runtime is the process's)

import numpy as np
import pytest

import rnamotif_amd as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

os.environ.setdefault("EFNDATA", R.EFNDATA_DIR)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRNA = os.path.join(ROOT, "tests", "golden", "descr", "trna.descr")
REAL_DB = os.path.join(ROOT, "tests", "golden", "test", "gbrna.111.0.fastn.gz")
CU_LDS = 160 * 1024


@pytest.fixture(scope="module")
def world(built):
    """descriptor, CUs, the three databases (on device 0, laid out for whoever attaches) and their records under the solo shape"""
    d = R.Descriptor(["-descr", TRNA])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    seqs = {"a": R.synthetic_records(5), "b": [r[2] for r in R.read_fasta(REAL_DB)], "c": R.synthetic_records(1, length=6000)}
    sc = R.Scanner(d, device=0)
    sc.set_option("beside", 0)
    dbs = {k: sc.database(v) for k, v in seqs.items()}
    solo, shape = {}, {}
    for k, db in dbs.items():
        solo[k] = sc.scan(db).copy()
        shape[k] = sc.last_launch()
        assert shape[k][3] == 0
    assert solo["b"].shape[0] == 1351 and solo["a"].shape[0] > 100
    assert shape["a"][0] > 4 * cus or cus != 256       # (on an MI355X the solo grid of (a) is above the beside cap)
    yield {"d": d, "cus": cus, "dbs": dbs, "solo": solo, "shape": shape}
    sc.close()


def _beside_shape(ll, solo_ll, cus):
    grid, lds, drain_grid, beside = ll
    assert beside == 1
    assert grid == min(solo_ll[0], 4 * cus)
    assert 5 * lds > CU_LDS and lds % 64 == 0 and lds >= solo_ll[1]
    assert drain_grid % cus == 0 and 2 <= drain_grid // cus <= 4


@pytest.mark.parametrize("which", ["a", "b", "c"])
def test_records_under_beside_equal_the_solo_ones(world, which):
    sc = R.Scanner(world["d"], device=0)
    sc.set_option("beside", 1)
    got = sc.scan(world["dbs"][which])
    _beside_shape(sc.last_launch(), world["shape"][which], world["cus"])
    assert got.shape == world["solo"][which].shape and np.array_equal(got, world["solo"][which])
    if which == "b":
        assert got.shape[0] == 1351
    sc.close()


def test_two_scanners_in_turns(world):
    """Eight steps, databases (a) and (b) alternating, step i + 1 begun before step i is ended, default options: from
    the second step on a scan begins while the other scanner's is in flight and plans beside."""
    scs = [R.Scanner(world["d"], device=0) for _ in range(2)]
    for s in scs:
        for k in "ab":
            s.attach(world["dbs"][k])
    order = "abbaabab"          # (either scanner gets both databases, and both orders of the two follow each other)
    pend, got, shapes = None, [], []
    for i, k in enumerate(order):
        s = scs[i & 1]
        s.scan_begin(world["dbs"][k])
        shapes.append(s.last_launch())
        if pend is not None:
            got.append(pend.scan_end().copy())
        pend = s
    got.append(pend.scan_end().copy())
    for i, k in enumerate(order):
        assert got[i].shape == world["solo"][k].shape and np.array_equal(got[i], world["solo"][k]), (i, k)
        if i == 0:
            assert shapes[i] == world["shape"][k]
        else:
            _beside_shape(shapes[i], world["shape"][k], world["cus"])
    for s in scs:
        s.close()


def test_who_plans_beside(world):
    a, c = world["dbs"]["a"], world["dbs"]["c"]
    s0, s1 = R.Scanner(world["d"], device=0), R.Scanner(world["d"], device=0)
    # a lone scanner: the solo shape
    s0.scan(c)
    assert s0.last_launch() == world["shape"]["c"]
    # the scanner that begins while the other has a scan in flight plans beside; the first did not
    s0.scan_begin(a)
    s1.scan_begin(a)
    assert s0.last_launch() == world["shape"]["a"]
    _beside_shape(s1.last_launch(), world["shape"]["a"], world["cus"])
    # a begin that is refused -- this scanner's scan is in flight already -- leaves the count where it was: one in flight
    # after s1 is ended (s0's), none after s0 is
    with pytest.raises(R.RnamotifError):
        s1.scan_begin(c)
    r1 = s1.scan_end().copy()
    with pytest.raises(R.RnamotifError):
        s0.scan_begin(c)
    s1.scan_begin(c)
    assert s1.last_launch()[3] == 1
    s1.scan_end()
    r0 = s0.scan_end().copy()
    assert np.array_equal(r0, world["solo"]["a"]) and np.array_equal(r1, world["solo"]["a"])
    # ... and so does one refused for a database of another device.  That needs a second GPU: on a machine with one this
    # case does not run here.  The refusal returns before rma_scan_begin() has made its guard or touched the mark, the same
    # place as the one above; tests/hostsim/flight_count_check.cpp runs that return (how == 0) on the CPU.
    if torch.cuda.device_count() > 1:
        other = R.Scanner(world["d"], device=1)
        with pytest.raises(R.RnamotifError):
            other.scan_begin(a)
        with pytest.raises(R.RnamotifError):
            s0.scan_begin(other.database(R.synthetic_records(1, length=6000)))
        other.close()
    # both ended: a lone scan is solo again, on either scanner
    for s in (s1, s0):
        s.scan(c)
        assert s.last_launch() == world["shape"]["c"]
    # a scanner closed with its scan in flight leaves the count too
    s1.scan_begin(c)
    s1.close()
    s0.scan(c)
    assert s0.last_launch() == world["shape"]["c"]
    s0.close()


def test_repeat_launch_keeps_the_beside_shape(world):
    """A list of seven items overflows on (a): search_finish() makes room and launches again, in the shape the scan began with."""
    sc = R.Scanner(world["d"], device=0)
    sc.set_option("beside", 1)
    sc.set_option("glist", 7)
    got = sc.scan(world["dbs"]["a"])
    _beside_shape(sc.last_launch(), world["shape"]["a"], world["cus"])
    assert np.array_equal(got, world["solo"]["a"])
    sc.close()
