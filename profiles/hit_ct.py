"""profiles/hit_ct.py -- rm2ct's connect records made on the device against the path that made them before.

For descr/trna.descr over synthetic_records(100) (100 x 1 Mbase), on the records of the GPU scan, scored once, the
accepted records as they are and repeated to about 10^5, in both types, both into a file:
  * the new call: Scanner.ct_hits( ..., names=EntryNames, type= ) + HitCt.write(): the size and fill kernels, the wait
    for the total, one device-to-host copy of the bytes and the write;
  * what there was for the same records: Scanner.print_hits() + HitPrint.write() into a pipe that bin/rm2ct reads, its
    output into a file.
The two alternate, --reps times each per size, after a warm-up of both; wall clock behind a synchronisation, medians.
The two files must be byte-identical: that is asserted, the ratio is not.  The call's halves are timed too, each by wall
clock behind a synchronisation: rma_hit_ct_size() alone (the size kernels and the wait) and ct_hits() without the copy
to the host; the fill is the difference.  For the kernels' own times run
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o hc -- python profiles/hit_ct.py --device-only --out /dev/null
Writes profiles/hit_ct_mi355x.json.  Not a test.
Usage: python profiles/hit_ct.py [--sizes 0,100000] [--reps 10] [--device-only]     (size 0: the scan's accepted records)"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rnamotif_amd as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="0,100000")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--device-only", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hit_ct_mi355x.json"))
args = ap.parse_args()

os.environ.setdefault("EFNDATA", R.EFNDATA_DIR)
RM2CT = os.path.join(ROOT, "rnamotif_amd", "bin", "rm2ct")
ENV = dict(os.environ, LC_ALL="C")
dev = torch.device("cuda", 0)
seqs = R.synthetic_records(100)
text = torch.frombuffer(bytearray(b"".join(seqs)), dtype=torch.uint8).to(dev)
d = R.Descriptor(["-descr", os.path.join(ROOT, "tests", "golden", "descr", "trna.descr")])
sc = R.Scanner(d, device=0)
db = sc.database_from_tensor(text, lengths=[len(s) for s in seqs])
prog = R.ScoreProgram(d, text=True)
found = sc.scan_tensor(db)
scored = sc.score(db, found, prog, text=True)
keep = torch.nonzero(scored.accept).flatten()
names = R.EntryNames(sc, db, [b"synthetic_%03d" % i for i in range(len(seqs))], [b"%d bases" % len(s) for s in seqs])
words = " ".join(d.names()).encode()
tmp = tempfile.mkdtemp(prefix="hit_ct_")
new_path, old_path = os.path.join(tmp, "device.ct"), os.path.join(tmp, "rm2ct.ct")


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(xs):
    xs = list(xs)
    return {"best": min(xs), "median": statistics.median(xs)}


rows = []
for size in args.sizes.split(","):
    n = int(size) or int(keep.numel())
    idx = keep[torch.arange(n, device=dev) % keep.numel()]
    hits = found[idx].contiguous()
    s = R.HitScores(scored.accept[idx].contiguous(), scored.score[idx].contiguous(), scored.kind[idx].contiguous(),
                    scored.text_bytes[idx].contiguous(), scored.text_len[idx].contiguous())
    for type in ("rnamotif", "rnaviz"):
        def device():
            ct = sc.ct_hits(db, hits, s, names=names, type=type)
            with open(new_path, "wb") as f:
                ct.write(f)

        def host():
            p = sc.print_hits(db, hits, s, names=names)
            with open(old_path, "wb") as out:
                tool = subprocess.Popen([RM2CT] + (["-t", "rnaviz"] if type == "rnaviz" else []), stdin=subprocess.PIPE, stdout=out, env=ENV)
                p.write(tool.stdin)
                tool.stdin.close()
                assert tool.wait() == 0

        def size_only():
            total = C.c_int64(0)
            err = C.create_string_buffer(1024)
            rc = R.lib().rma_hit_ct_size(sc._h, db._h, names._h, hits.data_ptr(), n, s.accept.data_ptr(), s.text_bytes.data_ptr(), int(s.text_bytes.shape[1]),
                                         s.text_len.data_ptr(), 1 if type == "rnaviz" else 0, words, None, C.byref(total),
                                         torch.cuda.current_stream().cuda_stream, err, 1024)
            assert rc == 0, err.value

        device()            # (first calls: scratch, the table's upload, the code objects)
        if not args.device_only:
            host()
        new, old, halves = [], [], []
        for _ in range(args.reps):
            new.append(wall(device))
            if not args.device_only:
                old.append(wall(host))
            halves.append((wall(size_only), wall(lambda: sc.ct_hits(db, hits, s, names=names, type=type))))
        row = {"records": n, "type": type, "reps": args.reps, "output_bytes": os.path.getsize(new_path), "ct_hits_write_wall_ms": median(new),
               "halves_median_ms": {"size_call": statistics.median(x[0] for x in halves), "ct_hits_on_the_device": statistics.median(x[1] for x in halves),
                                    "fill_by_difference": statistics.median(x[1] - x[0] for x in halves)}}
        if not args.device_only:
            a, b = open(new_path, "rb").read(), open(old_path, "rb").read()
            assert a == b, "the two files differ at %d records, %s" % (n, type)
            row["identical_output"] = True
            row["print_hits_pipe_rm2ct_wall_ms"] = median(old)
            row["ratio_of_medians"] = statistics.median(old) / statistics.median(new)
        rows.append(row)
        print(json.dumps(row), flush=True)

result = {"what": "hit_ct", "device": torch.cuda.get_device_name(0), "database": "synthetic_records(100)", "descriptor": "descr/trna.descr",
          "scan_records": int(found.shape[0]), "accepted": int(keep.numel()), "sizes": rows,
          "measured": "wall clock behind a synchronisation, medians; the two paths alternate; the halves in runs of their own"}
if args.out != "/dev/null":
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps(result))
names.close()
