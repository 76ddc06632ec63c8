"""GPU: life cycles of scanners, databases and communicators -- what their destroy functions and the owners of
rnamotif_amd/csrc/rm_hip_own.h must get right for a process that makes and closes them again and again:

  * a scanner closed with a scan in flight, then its database: a new pair of the same inputs scans as before;
  * three rounds of every call over records (prune, hit_structures, energies, align, score) between creating and closing
    a scanner and a database: round 3's tensors equal round 1's;
  * load_energy_tables twice on one scanner: the same structure energies before and after the second load;
  * a communicator of one rank created, counted, used and closed twice in one process.

Legitimate use of the API only.  torch is imported before the product library: one HIP runtime serves the process."""
import os

import torch  # noqa: F401  (first: its HIP runtime is the process's)

import numpy as np
import pytest

import rnamotif_amd as R
from test_score_device_cpu import OWN, entries_of, own_args

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

os.environ.setdefault("EFNDATA", R.EFNDATA_DIR)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRNA = os.path.join(ROOT, "tests", "golden", "descr", "trna.descr")
DEV = torch.device("cuda", 0)


def _ragged(seqs):
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return torch.frombuffer(bytearray(b"".join(seqs)), dtype=torch.uint8).to(DEV), off


@pytest.fixture(scope="module")
def synthetic(built):
    return R.synthetic_records(4, length=250_000)


def _round(d, seqs, prog_of):
    """every call over records between creating and closing a scanner and a database: their tensors, on the host"""
    sc = R.Scanner(d, device=0)
    text, off = _ragged(seqs)
    db = sc.database_from_tensor(text, offsets=off)
    hits = sc.scan_tensor(db)
    assert hits.shape[0] >= 1
    keep = sc.prune(db, hits)
    st = sc.hit_structures(db, hits)
    sc.load_energy_tables()
    efn, efn2 = st.energies(sc)
    al = sc.align(db, hits, pos=True)
    out = [hits, keep, st.off, st.lo, st.base, st.elem, st.mate, efn, efn2, al.rows, al.pos]
    prog = prog_of(d)
    if prog is not None:
        s = sc.score(db, hits, prog)
        out += [s.accept, s.score, s.kind]
        prog.close()
    torch.cuda.synchronize()
    out = [t.cpu() for t in out]
    sc.close()
    db.close()
    return out


def _three_rounds(d, seqs, prog_of):
    first = _round(d, seqs, prog_of)
    _round(d, seqs, prog_of)
    third = _round(d, seqs, prog_of)
    assert len(first) == len(third)
    for a, b in zip(first, third):
        assert a.dtype == b.dtype and torch.equal(a, b)
    return first


def test_three_rounds_of_every_call(synthetic):
    """trna.descr (its score section prints: no program for the device) over 1 Mbase"""
    d = R.Descriptor(["-descr", TRNA])
    assert R.ScoreProgram.reason(d) is not None
    first = _three_rounds(d, synthetic, lambda d: None)
    assert first[0].shape[0] >= 1 and first[1].any()


def test_three_rounds_with_a_score_section(built, gbrna, tmp_path):
    """the string-variable hairpin of tests/test_score_device.py over its 30 entries: score() as well"""
    d = R.Descriptor(own_args(OWN["string variable"][0], tmp_path, "lifecycle"))
    first = _three_rounds(d, entries_of(gbrna, 30), R.ScoreProgram)
    assert len(first) == 14 and first[11].any() and not first[11].all()


def test_close_with_a_scan_in_flight(synthetic):
    d = R.Descriptor(["-descr", TRNA])
    sc = R.Scanner(d, device=0)
    db = sc.database(synthetic)
    want = sc.scan(db)
    assert want.shape[0] >= 1
    sc.scan_begin(db)
    sc.close()              # (ends the scan, waits for its kernels, frees what they wrote)
    db.close()
    sc = R.Scanner(d, device=0)
    db = sc.database(synthetic)
    got = sc.scan(db)
    assert got.shape == want.shape and np.array_equal(got, want)
    sc.close()
    db.close()


def test_energy_tables_loaded_twice(synthetic):
    d = R.Descriptor(["-descr", TRNA])
    sc = R.Scanner(d, device=0)
    text, off = _ragged(synthetic)
    db = sc.database_from_tensor(text, offsets=off)
    hits = sc.scan_tensor(db)
    assert hits.shape[0] >= 1
    st = sc.hit_structures(db, hits)
    sc.load_energy_tables()
    e1, f1 = sc.structure_energies(st.off, st.base, st.mate)
    sc.load_energy_tables()
    e2, f2 = sc.structure_energies(st.off, st.base, st.mate)
    torch.cuda.synchronize()
    assert torch.equal(e1, e2) and torch.equal(f1, f2)
    assert (e1 != 16000).any() and (f1 != 9999999).any()      # (finite energies: the tables are read)
    sc.close()
    db.close()


def test_comm_twice(synthetic):
    d = R.Descriptor(["-descr", TRNA])
    sc = R.Scanner(d, device=0)
    db = sc.database(synthetic)
    want = sc.scan(db)
    index = [9, 3, 5, 1]
    relabelled = want.copy()
    relabelled[:, 0] = np.asarray(index, dtype=np.int32)[want[:, 0]]
    for _ in range(2):
        comm = R.Comm(0, 1, 0)
        assert comm.count() == 1
        sc.scan_begin(db)
        n = sc.scan_end_on_device()
        assert n == want.shape[0] >= 1
        got, counts = comm.gather(sc, index)
        assert counts == [n] and np.array_equal(got, relabelled)
        comm.close()
    sc.close()
    db.close()
