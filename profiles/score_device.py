"""profiles/score_device.py -- the score section on the device against the path that existed before it.

For mp.ends.descr and ire.descr over synthetic_records(100) (100 x 1 Mbase), on the records of the GPU scan:
  * Scanner.score(): the call between HIP events and by wall clock (the call waits once, so both cover the kernel, the
    wait and the copies into the result tensors);
  * Replay.device(..., accepted=True) writing to /dev/null on the same records: windows cut on the device, copied to
    the host, ScoreVM::run and the printer there.
Writes profiles/score_device_mi355x.json: both times per descriptor (best and median of --reps), the record counts, the
accepted counts of both paths (which must agree) and the image's and kernel's register and LDS figures.
Not a test.  Usage: python profiles/score_device.py [--records 100] [--reps 20]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rnamotif_amd as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--records", type=int, default=100)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_device_mi355x.json"))
args = ap.parse_args()

dev = torch.device("cuda", 0)
seqs = R.synthetic_records(args.records)
text = torch.frombuffer(bytearray(b"".join(seqs)), dtype=torch.uint8).to(dev)
result = {"device": torch.cuda.get_device_name(0), "database": "synthetic_records(%d)" % args.records, "reps": args.reps, "cases": {}}
for name in ("mp.ends", "ire"):
    d = R.Descriptor(["-descr", os.path.join(ROOT, "tests", "golden", "test", name + ".descr")])
    sc = R.Scanner(d, device=0)
    db = sc.database_from_tensor(text, lengths=[len(s) for s in seqs])
    hits = sc.scan_tensor(db)
    prog = R.ScoreProgram(d)
    s = sc.score(db, hits, prog)            # (first call: scratch, the image's upload, the code object)
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        s = sc.score(db, hits, prog)
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    host = []
    rp = R.Replay(d, "/dev/null")
    n_host, mask = rp.device(db, hits, accepted=True)
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_host, mask = rp.device(db, hits, accepted=True)
        host.append((time.perf_counter() - t0) * 1e3)
    rp.close()
    n_dev = int(s.accept.sum())
    case = {"records": int(hits.shape[0]), "accepted_device": n_dev, "accepted_host": int(n_host),
            "masks_equal": bool((s.accept.cpu().numpy() == mask).all()),
            "score_events_ms": {"best": min(ev), "median": statistics.median(ev)},
            "score_wall_ms": {"best": min(wall), "median": statistics.median(wall)},
            "replay_device_wall_ms": {"best": min(host), "median": statistics.median(host)},
            "kernel": prog.info()}
    result["cases"][name] = case
    print(name, json.dumps(case))
    prog.close()
    db.close()
    sc.close()
with open(args.out, "w") as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write("\n")
