"""Hit structures as device tensors (Scanner.hit_structures, rma_hit_structures): one JSON line.

trna.descr over the synthetic 100 x 1 Mbase database bench.py uses (iid uniform acgt, seed 20240601), as one 1-D
uint8 tensor on the GPU: database_from_tensor, scan_tensor, then for the same records
  events_ms   HIP events on the caller's stream around rma_hit_structures() into tensors made beforehand: the span,
              helix-check, scan and fill kernels (rm_hitwin_dev.hip, rm_hitstruct_dev.hip) and the one host wait
              for the count between them
  call_ms     wall clock of Scanner.hit_structures(): rma_hit_structures_size, torch's allocations, the call above
  replay_ms   wall clock of Replay.device() over the same records, for comparison: the text route's first step
Medians.  The kernels' own times are in a rocprofv3 --kernel-trace --stats run of this script
(rma_hit_span_kernel, rma_hit_helix_kernel, rma_hit_struct_kernel, rocPRIM's scan).

usage: python profiles/hit_structures.py [--reps N] [--out FILE]"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import sys
import time

import torch  # first: its HIP runtime serves the process

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rnamotif_amd as R  # noqa: E402

DEV = torch.device("cuda", 0)


def _wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(DEV)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(DEV)
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


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
    st = sc.hit_structures(db, hits)
    torch.cuda.synchronize(DEV)
    n, total = int(hits.shape[0]), int(st.off[-1])
    call_ms = _wall(lambda: sc.hit_structures(db, hits), args.reps)
    # the C call alone between two events, into the tensors of the first call
    err = C.create_string_buffer(4096)
    stream = torch.cuda.current_stream(DEV)
    ev = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(DEV)
        a.record(stream)
        rc = R.lib().rma_hit_structures(sc._h, db._h, hits.data_ptr(), n, None, total, st.off.data_ptr(), st.lo.data_ptr(),
                                        st.base.data_ptr(), st.elem.data_ptr(), st.mate.data_ptr(), stream.cuda_stream, err, 4096)
        assert rc == 0, err.value
        b.record(stream)
        b.synchronize()
        ev.append(a.elapsed_time(b))
    rp = R.Replay(d, os.devnull)
    rp.device(db, hits)
    replay_ms = _wall(lambda: rp.device(db, hits), args.reps)
    rp.close()
    h = hashlib.sha256()
    for f in ("rm_hitstruct_dev.hip", "rm_hitstruct.h"):
        h.update(open(os.path.join(ROOT, "rnamotif_amd", "csrc", f), "rb").read())
    res = {"what": "hit_structures", "descr": "trna.descr", "database": "100 x 1 Mbase synthetic, one uint8 tensor", "records": n,
           "window_bytes": total, "bytes_written": 8 * (n + 1) + 4 * n + total * (1 + 2 + 12), "events_ms": round(statistics.median(ev), 4),
           "events_ms_min": round(min(ev), 4), "call_ms": round(call_ms, 3), "replay_device_ms": round(replay_ms, 3), "reps": args.reps,
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
