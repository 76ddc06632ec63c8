"""GPU: rmprune's rule over hit records on the device (Scanner.prune, rma_prune_hits: the kernels of rm_prune_dev.hip)
against the same rule, rm_prune.h, run on the host through tests/hostsim/prune_check.cpp -- bit for bit:

  * the descriptor cases of tests/test_prune_cpu.py (which holds the rule to the rmprune tool), databases from
    database_from_tensor and once from database_from_fasta_tensor with groups=prune_groups(db.sids);
  * end to end on the device: Replay.device(db, hits) piped through bin/rmprune equals Replay.device(db, hits[keep]);
  * the shapes where the kernels can go wrong, made by row selection and repetition: groups of 1, 2, 63, 64, 65 and
    129 records (the lanes' chunks), blocks of 1000 and 1001, 3 000 blocks of one record, more blocks than the rezip
    kernel's 65 536 workgroups (the grid-stride path), record counts that are no multiple of the 256 a workgroup of
    the per-record kernels takes;
  * no record; a non-default stream right behind the kernel that wrote the records; hits[keep] into hit_structures();
  * refusals with their words; a forged record is named by index and keep stays at the sentinel it was filled with.

torch is imported before the product library: one HIP runtime serves the process."""
import ctypes
import os
import re
import subprocess

import torch  # noqa: F401  (first: its HIP runtime is the process's)

import numpy as np
import pytest

import rnamotif_amd as R
from test_hit_windows_cpu import normalise, odd_entries
from test_prune_cpu import CASES, GOLDEN, HDR, TOOL, descr_of, host_mask, prune_checker, split  # noqa: F401

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

DEV = torch.device("cuda", 0)


def _ragged(seqs, lead=3):
    flat = b"x" * lead + b"".join(seqs)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64) + lead
    return torch.frombuffer(bytearray(flat), dtype=torch.uint8).to(DEV), off


def _open(d, seqs):
    sc = R.Scanner(d, device=0)
    text, off = _ragged(seqs)
    db = sc.database_from_tensor(text, offsets=off)
    return sc, db, sc.scan_tensor(db)


def _rc(s):
    return bytes(b if b in b"acgt" else ord("n") for b in s[::-1].translate(bytes.maketrans(b"acgt", b"tgca")))


def _mask(sc, db, rows, groups=None):
    keep = sc.prune(db, rows, groups=groups)
    assert keep.dtype == torch.bool and tuple(keep.shape) == (rows.shape[0],) and keep.device == rows.device
    torch.cuda.synchronize()
    return keep.cpu().numpy()


@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_with_the_host_rule(built, prune_checker, gbrna, workdir, tmp_path, name):
    d = descr_of(name, workdir, tmp_path)
    seqs = [normalise(e) for e in odd_entries(gbrna, limit=CASES[name][0])]
    if name == "trna":
        seqs = seqs + [_rc(s) for s in seqs]            # records on both strands
    sc, db, hits = _open(d, seqs)
    recs = hits.cpu().numpy()
    assert recs.shape[0] > 0, name
    want, counts = host_mask(prune_checker, tmp_path, d, [len(s) for s in seqs], recs)
    got = _mask(sc, db, hits)
    print("%s: %d records, %d kept, %s" % (name, len(recs), want.sum(), counts))
    assert np.array_equal(got, want), name
    if CASES[name][1]:
        assert not want.all() and want.any()
    if name == "trna":
        assert (recs[:, 1] == 0).sum() > 8 and (recs[:, 1] == 1).sum() > 8
    db.close()
    sc.close()


def test_fasta_tensor_with_name_groups(built, prune_checker, gbrna, tmp_path):
    d = descr_of("trna", None, tmp_path)
    raw = open(gbrna, "rb").read()
    cut = raw.index(b"\n>", 300_000) + 1
    text = raw[:cut]
    sc = R.Scanner(d, device=0)
    db = sc.database_from_fasta_tensor(torch.frombuffer(bytearray(text), dtype=torch.uint8).to(DEV))
    hits = sc.scan_tensor(db)
    assert hits.shape[0] > 0 and db.n_seqs > 100
    groups = R.prune_groups(db.sids)
    assert groups.dtype == np.int32 and len(groups) == db.n_seqs
    slens = [len(r[2]) for r in R.read_fasta(gbrna)[:db.n_seqs]]
    recs = hits.cpu().numpy()
    want, _ = host_mask(prune_checker, tmp_path, d, slens, recs, groups)
    assert np.array_equal(_mask(sc, db, hits, groups=groups), want)
    # entries merged in fours: other runs, other blocks
    merged = (np.arange(db.n_seqs) // 4).astype(np.int32)
    want4, c4 = host_mask(prune_checker, tmp_path, d, slens, recs, merged)
    assert np.array_equal(_mask(sc, db, hits, groups=merged), want4)
    assert c4["blocks"] == len(set(merged[recs[:, 0]]))
    db.close()
    sc.close()


@pytest.fixture(scope="module")
def trna(built, gbrna):
    d = R.Descriptor(["-descr", os.path.join(GOLDEN, "descr", "trna.descr")])
    seqs = [normalise(e) for e in odd_entries(gbrna, limit=300)]
    seqs = seqs + [_rc(s) for s in seqs]
    sc, db, hits = _open(d, seqs)
    yield d, seqs, sc, db, hits
    db.close()
    sc.close()


def test_end_to_end_on_the_device(trna, tmp_path):
    d, seqs, sc, db, hits = trna
    keep = sc.prune(db, hits)
    outs = []
    for what, rows in (("all", hits), ("kept", hits[keep])):
        path = str(tmp_path / (what + ".out"))
        rp = R.Replay(d, path)
        n = rp.device(db, rows)
        rp.close()
        assert n == rows.shape[0]
        outs.append(open(path, "rb").read())
    p = subprocess.run([TOOL], input=outs[0], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and p.stdout == outs[1]
    n_all, n_kept = len(split(outs[0])[1]), len(split(outs[1])[1])
    assert 0 < n_kept < n_all == hits.shape[0]
    # ... and into hit_structures(): the windows of the kept records are those rows of all records' windows
    st_all, st = sc.hit_structures(db, hits), sc.hit_structures(db, hits[keep])
    torch.cuda.synchronize()
    lens = (st_all.off[1:] - st_all.off[:-1])[keep]
    assert torch.equal(st.off[1:] - st.off[:-1], lens) and torch.equal(st.lo, st_all.lo[keep]) and int(st.off[-1]) == int(lens.sum())
    k0 = int(torch.nonzero(keep)[0])
    a, b = int(st_all.off[k0]), int(st_all.off[k0 + 1])
    assert torch.equal(st.base[:b - a], st_all.base[a:b]) and torch.equal(st.mate[:b - a], st_all.mate[a:b])


def _family(prune_checker, tmp, d, seqs, recs):
    """(a, b, x) of test_prune_cpu.related_pair: a and b related, x of their entry and strand related to neither"""
    from test_prune_cpu import related_pair
    return related_pair(prune_checker, tmp, d, seqs, recs)


def test_shapes(trna, prune_checker, tmp_path):
    d, seqs, sc, db, hits = trna
    recs = hits.cpu().numpy()
    slens = [len(s) for s in seqs]
    a, b, x = _family(prune_checker, tmp_path, d, seqs, recs)
    e = int(a[0])
    far = recs[recs[:, 0] != e]
    shapes = {}
    # groups of g records: the family a, b repeated inside one leader's span, fenced by records of other entries
    for g in (1, 2, 63, 64, 65, 129):
        shapes["group %d" % g] = np.concatenate([far[:3], np.stack(([a, b] * g)[:g]), far[3:5], np.stack(([b, a, a] * g)[:g]), far[5:7]])
    for n in (1000, 1001):
        shapes["block %d" % n] = np.stack(([a, b, b, a, x] * n)[:n])
        shapes["block %d, x first" % n] = np.stack([x] * (n - 2) + [a, b])
    # blocks of one record: two entries in turn
    other = far[far[:, 0] == far[0, 0]][0]
    shapes["3000 blocks of one"] = np.stack([a, other] * 1500)
    shapes["70001 blocks of one"] = np.stack([a, other] * 35000 + [a])
    # counts around the per-record kernels' 256 and seams of blocks in the middle of a workgroup
    for n in (255, 256, 257, 2 * 256 + 1):
        shapes["%d records" % n] = np.concatenate([recs] * (n // len(recs) + 1))[:n]
    shapes["all, three times"] = np.concatenate([recs, recs[::-1], recs])
    dropped = 0
    for what, rows in shapes.items():
        want, c = host_mask(prune_checker, tmp_path, d, slens, rows)
        got = _mask(sc, db, torch.from_numpy(np.ascontiguousarray(rows)).to(DEV))
        assert np.array_equal(got, want), (what, int((got != want).sum()), np.nonzero(got != want)[0][:8])
        dropped += int((~want).sum())
        if what.startswith("block 1001"):
            assert c["blocks"] == 2
        if "blocks of one" in what:
            assert c["blocks"] == len(rows) and want.all()
    assert dropped > 100


def test_no_record_and_stream_order(trna):
    d, seqs, sc, db, hits = trna
    keep = sc.prune(db, hits[:0])
    assert keep.dtype == torch.bool and keep.numel() == 0
    want = sc.prune(db, hits)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    filler = torch.zeros(64 << 20, dtype=torch.int32, device=DEV)
    with torch.cuda.stream(side):
        late = torch.zeros_like(hits)
        filler.add_(1)              # (something to wait behind)
        late.copy_(hits)            # the kernel that writes the records, then the call right behind it
        got = sc.prune(db, late)
        total = got.sum()           # ... and a consumer right behind the call
    side.synchronize()
    assert torch.equal(got, want) and int(total) == int(want.sum())


def test_refusals(trna):
    d, seqs, sc, db, hits = trna
    n = hits.shape[0]
    with pytest.raises(ValueError, match="hits is on cpu"):
        sc.prune(db, hits.cpu())
    with pytest.raises(TypeError, match="int64"):
        sc.prune(db, hits.to(torch.int64))
    with pytest.raises(ValueError, match=r"\[n, %d\]" % d.hit_stride):
        sc.prune(db, hits[:, :-1])
    with pytest.raises(TypeError, match="not a torch.Tensor"):
        sc.prune(db, hits.cpu().numpy())
    with pytest.raises(ValueError, match="groups: one per entry, %d, not 3" % len(seqs)):
        sc.prune(db, hits, groups=[0, 1, 2])
    # a host database of the same entries will do: only the lengths are read
    host = sc.database(seqs)
    assert torch.equal(sc.prune(host, hits), sc.prune(db, hits))
    host.close()
    with pytest.raises(ValueError, match="closed"):
        sc.prune(host, hits)
    # forged records through the C ABI, keep prefilled with a sentinel
    L = R.lib()
    buf = ctypes.create_string_buffer(1024)
    slen1 = len(seqs[int(hits[1, 0])])
    forged = [(2, 0, len(seqs), r"record 2: entry %d outside \[0, %d\)" % (len(seqs), len(seqs))),
              (3, 1, 2, "record 3: strand 2, not 0 or 1"),
              (1, HDR + 4 * 4, slen1 + 1, "record 1: element 4 at offset %d, length .* outside entry" % (slen1 + 1))]
    for row, col, value, words in forged:
        bad = hits.clone()
        bad[row, col] = value
        keep = torch.full((n,), 77, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        rc = L.rma_prune_hits(sc._h, db._h, bad.data_ptr(), n, None, keep.data_ptr(), None, buf, 1024)
        torch.cuda.synchronize()
        assert rc == 1 and re.search(words, buf.value.decode()) and "nothing judged" in buf.value.decode(), buf.value
        assert bool((keep == 77).all()), words
        with pytest.raises(R.RnamotifError, match=words):
            sc.prune(db, bad)
    keep = torch.full((n + 8,), 77, dtype=torch.uint8, device=DEV)
    rc = L.rma_prune_hits(sc._h, db._h, hits.data_ptr(), n, None, keep.data_ptr(), None, buf, 1024)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(keep[:n].bool(), sc.prune(db, hits)) and bool((keep[n:] == 77).all()) and bool((keep[:n] <= 1).all())
    rc = L.rma_prune_hits(sc._h, db._h, hits.cpu().data_ptr(), n, None, keep.data_ptr(), None, buf, 1024)
    assert rc == 1 and b"the records" in buf.value
