"""profiles/seq_check.py -- the loose seq= expressions on the device against the path that existed before the call.

For backref_floating of tests/test_loose_seq.py -- ss(minlen=6,maxlen=9,seq="\\(ac\\)g\\1") -- inside a hairpin, over
synthetic_records(100) (100 x 1 Mbase) as profiles/device_replay.py makes them, on the records of the GPU scan:
  * Scanner.seq_check(): the call between HIP events on the stream and by wall clock (the call waits once, so both cover
    the kernel, the wait and the copies into the result tensors), after a warm-up call;
  * Replay.device(..., accepted=True) writing to /dev/null on the same records: windows cut on the device, copied to
    the host, the expression applied and the printer run there.  The descriptor has no score section: what the replay
    prints is the candidates, and its mask must equal keep.
Writes profiles/seq_check_mi355x.json: both times (best and median of --reps), the record and candidate counts, and the
image's and kernel's figures from rma_seqcheck_info -- private bytes, registers, LDS of a workgroup and the workgroups
of 4 waves that fit a CU's 160 KB of LDS by it.
Not a test.  Usage: python profiles/seq_check.py [--records 100] [--reps 20]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rnamotif_amd as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--records", type=int, default=100)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_check_mi355x.json"))
args = ap.parse_args()

dev = torch.device("cuda", 0)
seqs = R.synthetic_records(args.records)
text = torch.frombuffer(bytearray(b"".join(seqs)), dtype=torch.uint8).to(dev)
descr = 'descr\n\th5(minlen=2,maxlen=3)\n\t\tss(minlen=6,maxlen=9,seq="\\(ac\\)g\\1")\n\th3\n'
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "backref_floating.descr")
    with open(path, "w") as f:
        f.write(descr)
    d = R.Descriptor(["-descr", path])
sc = R.Scanner(d, device=0)
db = sc.database_from_tensor(text, lengths=[len(s) for s in seqs])
hits = sc.scan_tensor(db)
r = sc.seq_check(db, hits)              # (first call: scratch, the image's upload, the code object)
torch.cuda.synchronize()
ev, wall = [], []
for _ in range(args.reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    r = sc.seq_check(db, hits)
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
info = sc._seq_check.info
result = {"device": torch.cuda.get_device_name(0), "database": "synthetic_records(%d)" % args.records, "reps": args.reps,
          "descriptor": descr, "records": int(hits.shape[0]), "candidates_device": int(r.keep.sum()), "candidates_host": int(n_host),
          "masks_equal": bool((r.keep.cpu().numpy() == mask).all()),
          "seq_check_events_ms": {"best": min(ev), "median": statistics.median(ev)},
          "seq_check_wall_ms": {"best": min(wall), "median": statistics.median(wall)},
          "replay_device_wall_ms": {"best": min(host), "median": statistics.median(host)},
          "kernel": info, "workgroups_per_cu_by_lds": (160 * 1024) // max(info["workgroup_lds_bytes"], 1)}
print(json.dumps(result))
with open(args.out, "w") as f:
    json.dump(result, f, indent=1, sort_keys=True)
    f.write("\n")
db.close()
sc.close()
