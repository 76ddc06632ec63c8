"""profiles/hit_list.py -- rmfmt's listing made on the device against the path that made it before.

For descr/trna.descr over synthetic_records(100) (100 x 1 Mbase), on the records of the GPU scan, scored once, at about
10^3, 10^5 and 10^6 records (the larger sets by repeating rows; 10^6 twice: as rmfmt takes it, in input order because its
temp lines exceed -smax, and with -smax raised on both sides), both into a file:
  * the new call: Scanner.list_hits( ..., names=EntryNames ) + HitList.write(): the measure, compact, sort and fill
    kernels, the two waits, one device-to-host copy of the lines and the write;
  * what there was for the same listing: Scanner.print_hits() + HitPrint.write() into a pipe that bin/rmfmt reads, its
    output into a file.
The two alternate, --reps times each per size (fewer for the larger sizes), after a warm-up of both; wall clock behind
a synchronisation, medians.  The two files must be byte-identical: that is asserted, the ratio is not.  The call's
phases are timed too, each by wall clock behind a synchronisation: rma_hit_list_shape() alone (one measure pass and
its wait), list_hits() with smax=1 (both measure passes and the fill, no sort) and the whole call; the sort is the
difference of the last two.  For the kernels' own times run
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o hl -- python profiles/hit_list.py --sizes 100000 --device-only --out /dev/null
and hand the kernel statistics it leaves to a second, untraced run with --kernel-stats DIR/.../hl_kernel_stats.csv.
Writes profiles/hit_list_mi355x.json.  Not a test.
Usage: python profiles/hit_list.py [--sizes 1000,100000,1000000,1000000s] [--reps 10] [--device-only] [--kernel-stats CSV]"""
import argparse
import csv
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
ap.add_argument("--sizes", default="1000,100000,1000000,1000000s")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--device-only", action="store_true")
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hit_list_mi355x.json"))
args = ap.parse_args()

os.environ.setdefault("EFNDATA", R.EFNDATA_DIR)
RMFMT = os.path.join(ROOT, "rnamotif_amd", "bin", "rmfmt")
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
tmp = tempfile.mkdtemp(prefix="hit_list_")
new_path, old_path = os.path.join(tmp, "device.out"), os.path.join(tmp, "rmfmt.out")


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median(xs):
    xs = list(xs)
    return {"best": min(xs), "median": statistics.median(xs)}


sizes = []
for size in args.sizes.split(","):
    # (NNNs: with -smax raised on both sides, so that a listing of more than 30 000 000 temp bytes is sorted too)
    n, smax = int(size.rstrip("s")), (1 << 40) if size.endswith("s") else None
    idx = keep[torch.arange(n, device=dev) % keep.numel()]
    hits = found[idx].contiguous()
    s = R.HitScores(scored.accept[idx].contiguous(), scored.score[idx].contiguous(), scored.kind[idx].contiguous(),
                    scored.text_bytes[idx].contiguous(), scored.text_len[idx].contiguous())

    def device():
        hl = sc.list_hits(db, hits, s, names=names, smax=smax)
        with open(new_path, "wb") as f:
            hl.write(f)
        return hl

    def host():
        p = sc.print_hits(db, hits, s, names=names)
        with open(old_path, "wb") as out:
            tool = subprocess.Popen([RMFMT] + (["-smax", str(smax)] if smax else []), stdin=subprocess.PIPE, stdout=out, env=ENV)
            p.write(tool.stdin)
            tool.stdin.close()
            assert tool.wait() == 0

    def shape_only():
        import ctypes as C
        n_lines, line_len, mode, widths = C.c_int64(0), C.c_int64(0), C.c_int32(0), (C.c_int32 * 107)()
        err = C.create_string_buffer(1024)
        rc = R.lib().rma_hit_list_shape(sc._h, db._h, names._h, hits.data_ptr(), n, s.accept.data_ptr(), s.text_bytes.data_ptr(),
                                        int(s.text_bytes.shape[1]), s.text_len.data_ptr(), 0, 0, C.byref(n_lines), C.byref(line_len), widths, C.byref(mode),
                                        torch.cuda.current_stream().cuda_stream, err, 1024)
        assert rc == 0, err.value

    reps = max(2, args.reps if n <= 10_000 else args.reps // 2 if n <= 200_000 else args.reps // 4)
    device()            # (first calls: scratch, the table's upload, the code objects, the sort's work area)
    if not args.device_only:
        host()
    new, old, phases = [], [], []
    for _ in range(reps):
        new.append(wall(device))
        if not args.device_only:
            old.append(wall(host))
        phases.append((wall(shape_only), wall(lambda: sc.list_hits(db, hits, s, names=names, smax=1)), wall(lambda: sc.list_hits(db, hits, s, names=names, smax=smax))))
    hl = device()
    row = {"records": n, "smax": smax or 30000000, "reps": reps, "mode": hl.mode, "line_len": int(hl.lines.shape[1]), "output_bytes": os.path.getsize(new_path),
           "list_hits_write_wall_ms": median(new),
           "phases_median_ms": {"shape_call_one_measure_pass": statistics.median(x[0] for x in phases),
                                "list_hits_without_sort": statistics.median(x[1] for x in phases),
                                "list_hits": statistics.median(x[2] for x in phases),
                                "sort_by_difference": statistics.median(x[2] - x[1] for x in phases)}}
    if not args.device_only:
        a, b = open(new_path, "rb").read(), open(old_path, "rb").read()
        assert a == b, "the two files differ at %d records" % n
        row["identical_output"] = True
        row["print_hits_pipe_rmfmt_wall_ms"] = median(old)
        row["ratio_of_medians"] = statistics.median(old) / statistics.median(new)
    sizes.append(row)
    print(json.dumps(row), flush=True)

result = {"what": "hit_list", "device": torch.cuda.get_device_name(0), "database": "synthetic_records(100)", "descriptor": "descr/trna.descr",
          "scan_records": int(found.shape[0]), "accepted": int(keep.numel()), "sizes": sizes,
          "measured": "wall clock behind a synchronisation, medians; the two paths alternate; the phases in runs of their own"}
if args.kernel_stats:
    # rocprofv3's kernel statistics of a traced, device-only run: the listing's kernels and the library's they use
    with open(args.kernel_stats) as f:
        rows = list(csv.DictReader(f))
    mine = [r for r in rows if any(w in r.get("Name", "") for w in ("hit_list", "merge_sort", "block_sort", "block_merge", "scan", "hit_carry"))]
    result["kernels_traced_run"] = [{"name": r["Name"][:120], "calls": int(r.get("Calls", 0)), "total_us": float(r.get("TotalDurationNs", 0)) / 1e3,
                                     "average_us": float(r.get("AverageNs", 0)) / 1e3} for r in mine]
if args.out != "/dev/null":
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps(result))
names.close()
