"""Hit records as an alignment on the device (Scanner.align, rma_hit_alignment): one JSON line.

trna.descr over the synthetic 100 x 1 Mbase database bench.py uses (iid uniform acgt, seed 20240601), as one 1-D
uint8 tensor on the GPU: database_from_tensor, scan_tensor, then for the same records
  events_ms   HIP events on the caller's stream around rma_hit_alignment() into tensors made beforehand: the record
              check, the widths and fill kernels (rm_hitwin_dev.hip, rm_hitalign_dev.hip) and the one host wait for
              the widths between them
  call_ms     wall clock of Scanner.align(): rma_hit_alignment_shape, torch's allocations, the call above
  text_ms     wall clock of the route without it: the records replayed from the device and printed (Replay.device),
              the text piped through bin/rmfmt -a, the FASTA parsed back into an [n, W] array and uploaded
Medians.  The fill kernel's own time is not taken here: it comes from a rocprofv3 --kernel-trace run of this script
(rma_hit_align_kernel), to be set next to the bytes it writes divided by the rate rma_pack_text_kernel reaches in
the same run -- that kernel packs the 100 Mbase of text when the database is made.

usage: python profiles/hit_align.py [--reps N] [--out FILE]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch  # first: its HIP runtime serves the process

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rnamotif_amd as R  # noqa: E402

DEV = torch.device("cuda", 0)
RMFMT = os.path.join(ROOT, "rnamotif_amd", "bin", "rmfmt")


def _wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(DEV)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(DEV)
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def text_route(d, db, hits, path):
    """records -> host -> printed -> rmfmt -a -> parsed -> uploaded; returns the uint8 tensor [n, W]"""
    rp = R.Replay(d, path)
    rp.device(db, hits)
    rp.close()
    out = subprocess.run([RMFMT, "-a", path], stdout=subprocess.PIPE, check=True).stdout
    rows, cur = [], None
    for ln in out.split(b"\n"):
        if ln.startswith(b">"):
            if cur is not None:
                rows.append(b"".join(cur))
            cur = []
        elif ln:
            cur.append(ln)
    if cur is not None:
        rows.append(b"".join(cur))
    a = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), -1) if rows else np.zeros((0, 0), dtype=np.uint8)
    return torch.from_numpy(a.copy()).to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    args = ap.parse_args()
    os.environ.setdefault("EFNDATA", R.EFNDATA_DIR)
    d = R.Descriptor(["-descr", os.path.join(ROOT, "tests", "golden", "descr", "trna.descr")])
    sc = R.Scanner(d, device=0)
    sc.warmup()
    seqs = R.synthetic_records(100, length=1_000_000)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    text = torch.from_numpy(np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()).to(DEV)
    db = sc.database_from_tensor(text, offsets=off, wait=True)
    hits = sc.scan_tensor(db)
    # the accepted records: what the text route prints is what the device route aligns
    rp = R.Replay(d, os.devnull)
    _, mask = rp.device(db, hits, accepted=True)
    rp.close()
    hits = hits[torch.from_numpy(mask).to(DEV)].contiguous()
    al = sc.align(db, hits, pos=True)
    torch.cuda.synchronize(DEV)
    n, width = int(hits.shape[0]), int(al.rows.shape[1])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "hits.out")
        same = bool(torch.equal(text_route(d, db, hits, path), al.rows))
        text_ms = _wall(lambda: text_route(d, db, hits, path), max(3, args.reps // 4))
    call_ms = _wall(lambda: sc.align(db, hits, pos=True), args.reps)
    err = C.create_string_buffer(4096)
    stream = torch.cuda.current_stream(DEV)
    widths = np.ascontiguousarray(al.widths, dtype=np.int32)
    ev = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(DEV)
        a.record(stream)
        rc = R.lib().rma_hit_alignment(sc._h, db._h, hits.data_ptr(), n, widths.ctypes.data_as(C.POINTER(C.c_int32)), None, None,
                                       al.rows.data_ptr(), al.pos.data_ptr(), stream.cuda_stream, err, 4096)
        assert rc == 0, err.value
        b.record(stream)
        b.synchronize()
        ev.append(a.elapsed_time(b))
    h = hashlib.sha256()
    for f in ("rm_hitalign_dev.hip", "rm_hitalign.h"):
        h.update(open(os.path.join(ROOT, "rnamotif_amd", "csrc", f), "rb").read())
    res = {"what": "hit_align", "descr": "trna.descr", "database": "100 x 1 Mbase synthetic, one uint8 tensor", "records": n,
           "row_bytes": width, "bytes_written": n * width * 5, "rows_equal_rmfmt_a": same, "events_ms": round(statistics.median(ev), 4),
           "events_ms_min": round(min(ev), 4), "call_ms": round(call_ms, 3), "text_route_ms": round(text_ms, 3), "reps": args.reps,
           "kernel_sha256": h.hexdigest()[:16], "measured": "one MI355X, medians; events_ms by HIP events, the others wall clock"}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    db.close()
    sc.close()


if __name__ == "__main__":
    main()
