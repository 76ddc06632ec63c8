"""profiles/hit_print.py -- rnamotif's output lines made on the device against the path that made them before.

For descr/trna.descr over synthetic_records(100) (100 x 1 Mbase), on the records of the GPU scan, both into a file:
  * the new chain: Scanner.score( ..., text=True ) + Scanner.print_hits( ..., names=EntryNames ) + HitPrint.write():
    the score and print kernels, the two waits, one device-to-host copy of the bytes and the write;
  * Replay.device() on the same records and names: windows cut on the device, copied to the host, ScoreVM::run and
    HitPrinter::print there, into its file.
The two alternate, --reps times each, after a warm-up of both; wall clock, medians.  The two files must be
byte-identical: that is asserted, the ratio is not -- the number is for the record.  The chain's parts are timed too
(score, print_hits, write: each by wall clock behind a synchronisation).  Writes profiles/hit_print_mi355x.json.  For the
kernels' own times run it under `rocprofv3 --kernel-trace --stats -- python profiles/hit_print.py --reps 5 --out /dev/null`.
Not a test.  Usage: python profiles/hit_print.py [--records 100] [--reps 10]"""
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
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hit_print_mi355x.json"))
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
sids = [b"synthetic_%03d" % i for i in range(len(seqs))]
sdefs = [b"%d bases" % len(s) for s in seqs]
names = R.EntryNames(sc, db, sids, sdefs)
tmp = tempfile.mkdtemp(prefix="hit_print_")
new_path, old_path = os.path.join(tmp, "device.out"), os.path.join(tmp, "replay.out")


def chain(parts=None):
    t0 = time.perf_counter()
    s = sc.score(db, hits, prog, text=True)
    if parts is not None:
        torch.cuda.synchronize()
    t1 = time.perf_counter()
    p = sc.print_hits(db, hits, s, names=names)
    if parts is not None:
        torch.cuda.synchronize()
    t2 = time.perf_counter()
    with open(new_path, "wb") as f:
        p.write(f)
    t3 = time.perf_counter()
    if parts is not None:
        parts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
    return s, p


def replay():
    rp = R.Replay(d, old_path)
    n = rp.device(db, hits, sids, sdefs)
    rp.close()
    return n


s, p = chain()          # (first calls: scratch, the image's and the table's upload, the code objects)
n_host = replay()
torch.cuda.synchronize()
new, old, parts = [], [], []
for _ in range(args.reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s, p = chain()
    new.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    n_host = replay()
    old.append((time.perf_counter() - t0) * 1e3)
    chain(parts)
a, b = open(new_path, "rb").read(), open(old_path, "rb").read()
assert a == b, "the two files differ"
accepted = int(s.accept.sum())
assert accepted == n_host, (accepted, n_host)
result = {"what": "hit_print", "device": torch.cuda.get_device_name(0), "database": "synthetic_records(%d)" % args.records,
          "descriptor": "descr/trna.descr", "reps": args.reps, "records": int(hits.shape[0]), "printed": accepted, "output_bytes": len(a),
          "identical_output": a == b,
          "score_print_write_wall_ms": {"best": min(new), "median": statistics.median(new)},
          "replay_device_wall_ms": {"best": min(old), "median": statistics.median(old)},
          "parts_median_ms": {"score_text": statistics.median(x[0] for x in parts), "print_hits": statistics.median(x[1] for x in parts),
                              "copy_and_write": statistics.median(x[2] for x in parts)},
          "measured": "wall clock, medians; the parts in a run of their own with a synchronisation behind each"}
if args.out != "/dev/null":
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps(result))
names.close()
