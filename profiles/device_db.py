"""Databases from device memory (Scanner.database_from_tensor): one JSON line.

Two texts already in HBM: 100 Mbase as 100 entries of 1 Mbase, and the reference's test database 44 times
over (179 k entries of ~557 bases) as one ragged 1-D tensor.  For each, after a warm-up:
  pack_ms        database_from_tensor(wait=True), median: the small tables up, the pack kernel, its event
  pack_GBps      (1 byte read + 0.375 written per base) / pack_ms
  host_ms        rma_db_create of the same bytes (host pack + upload), median
and for trna.descr over the 100 Mbase text: database_from_tensor + scan against database(seqs) + scan.
The times are HIP events on torch's current stream around calls that end in a synchronise; the pack
kernel's own time is in a rocprofv3 --kernel-trace --stats run of this script (rma_pack_text_kernel).

usage: python profiles/device_db.py [--reps N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch  # first: its HIP runtime serves the process

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rnamotif_amd as R  # noqa: E402

DEV = torch.device("cuda", 0)


def _timed(fn, reps):
    """Median ms of fn() between two events on torch's current stream, fn ending in a synchronise."""
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(DEV)
        a.record()
        r = fn()
        b.record()
        torch.cuda.synchronize(DEV)
        out.append(a.elapsed_time(b))
        if r is not None and hasattr(r, "close"):
            r.close()
    return statistics.median(out)


def _case(sc, seqs, reps):
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    flat = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    text = torch.from_numpy(flat.copy()).to(DEV)
    off = np.concatenate([[0], np.cumsum(lens)])
    bases = int(lens.sum())
    for _ in range(2):
        sc.database_from_tensor(text, offsets=off, wait=True).close()
        sc.database(seqs).close()
    pack = _timed(lambda: sc.database_from_tensor(text, offsets=off, wait=True), reps)
    host = _timed(lambda: sc.database(seqs), max(3, reps // 3))
    return text, off, {"entries": len(seqs), "bases": bases, "pack_ms": round(pack, 4),
                       "pack_GBps": round(bases * 1.375 / pack / 1e6, 1), "host_ms": round(host, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    args = ap.parse_args()
    os.environ.setdefault("EFNDATA", R.EFNDATA_DIR)
    sc = R.Scanner(R.Descriptor(["-descr", os.path.join(ROOT, "tests", "golden", "descr", "trna.descr")]), device=0)
    sc.warmup()
    long_seqs = R.synthetic_records(100, length=1_000_000)
    gb = [r[2] for r in R.read_fasta(os.path.join(ROOT, "tests", "golden", "test", "gbrna.111.0.fastn.gz"))] * 44
    res = {"what": "device_db"}
    text, off, res["long_100x1M"] = _case(sc, long_seqs, args.reps)
    _, _, res["short_gbrna_x44"] = _case(sc, gb, args.reps)

    def dev_scan():
        db = sc.database_from_tensor(text, offsets=off)
        n = sc.scan(db).shape[0]
        db.close()
        return n

    def host_scan():
        db = sc.database(long_seqs)
        n = sc.scan(db).shape[0]
        db.close()
        return n

    n_dev, n_host = dev_scan(), host_scan()
    assert n_dev == n_host and n_dev > 0, (n_dev, n_host)
    res["trna_100M"] = {"candidates": n_dev, "from_tensor_scan_ms": round(_timed(dev_scan, 5), 2),
                        "host_db_scan_ms": round(_timed(host_scan, 3), 2)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sc.close()


if __name__ == "__main__":
    main()
