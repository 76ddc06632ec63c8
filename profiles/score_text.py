"""profiles/score_text.py -- the score section with text on the device against the path such descriptors took before it.

For descr/trna.descr (SCORE = sprintf( '%8.3f %8.3f', bits(...), efn(...) )) over synthetic_records(100) (100 x 1 Mbase), on the
records of the GPU scan:
  * Scanner.score( ..., text=True ): the call between HIP events and by wall clock (the call waits once, so both cover
    the kernel, the wait and the copies into the five result tensors);
  * Replay.device(..., accepted=True) writing to /dev/null on the same records: windows cut on the device, copied to
    the host, ScoreVM::run and the printer there.
The two alternate, --reps times each, after a warm-up of both.  Writes profiles/score_text_mi355x.json: both times (best
and median), the record and accepted counts of both paths (which must agree) and the image's and kernel's figures.  No
ratio is promised: the number is for the record.
Not a test.  Usage: python profiles/score_text.py [--records 100] [--reps 20]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_text_mi355x.json"))
args = ap.parse_args()

os.environ.setdefault("EFNDATA", R.EFNDATA_DIR)
dev = torch.device("cuda", 0)
seqs = R.synthetic_records(args.records)
text = torch.frombuffer(bytearray(b"".join(seqs)), dtype=torch.uint8).to(dev)
d = R.Descriptor(["-descr", os.path.join(ROOT, "tests", "golden", "descr", "trna.descr")])
sc = R.Scanner(d, device=0)
db = sc.database_from_tensor(text, lengths=[len(s) for s in seqs])
hits = sc.scan_tensor(db)
prog = R.ScoreProgram(d, text=True)
rp = R.Replay(d, "/dev/null")
s = sc.score(db, hits, prog, text=True)          # (first calls: scratch, the image's and the table's upload, the code object)
n_host, mask = rp.device(db, hits, accepted=True)
torch.cuda.synchronize()
ev, wall, host = [], [], []
for _ in range(args.reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    s = sc.score(db, hits, prog, text=True)
    b.record()
    torch.cuda.synchronize()
    wall.append((time.perf_counter() - t0) * 1e3)
    ev.append(a.elapsed_time(b))
    t0 = time.perf_counter()
    n_host, mask = rp.device(db, hits, accepted=True)
    host.append((time.perf_counter() - t0) * 1e3)
rp.close()
accepted = int(s.accept.sum())
assert accepted == n_host, (accepted, n_host)
result = {"device": torch.cuda.get_device_name(0), "database": "synthetic_records(%d)" % args.records, "descriptor": "descr/trna.descr",
          "reps": args.reps, "records": int(hits.shape[0]), "accepted": accepted, "replay_accepted": int(n_host),
          "score_text_event_ms": {"best": min(ev), "median": statistics.median(ev)},
          "score_text_wall_ms": {"best": min(wall), "median": statistics.median(wall)},
          "replay_device_wall_ms": {"best": min(host), "median": statistics.median(host)},
          "a_column": s.text(int(torch.nonzero(s.accept)[0])).decode() if accepted else None,
          "score_heap": 256, "text_width": int(s.text_bytes.shape[1]), "image": prog.info()}
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps(result))
