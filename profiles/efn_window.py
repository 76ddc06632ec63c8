"""The energy kernel's time on bench.py's workload (trna.descr over 100 Mbase, 5 837 cloverleaves): one scan alone,
twelve scans, by rma_scanner_last_kernel_ms()[2] -- in both forms of the kernel -- and the step of two scanners in
turns (beside_try.py's loop).  Builds go in turns through RNAMOTIF_AMD_LIB, one process a build and round:
    RNAMOTIF_AMD_LIB=.../librnamotif_amd.so python profiles/efn_window.py TAG OUT.jsonl
appends one JSON line to OUT.jsonl; profiles/efn_window_mi355x.json is those lines put together."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rnamotif_amd as R  # noqa: E402

tag, out = sys.argv[1], sys.argv[2]
os.environ.setdefault("EFNDATA", R.EFNDATA_DIR)
d = R.Descriptor(["-descr", os.path.join(ROOT, "tests", "golden", "descr", "trna.descr")])
seqs = R.synthetic_records(100)
scs = [R.Scanner(d), R.Scanner(d)]
db = scs[0].database(seqs)
for s in scs:
    s.attach(db)


def turns(n):
    pend = None
    for i in range(n):
        s = scs[i & 1]
        s.scan_begin(db)
        if pend is not None:
            pend.scan_end(copy=False)
        pend = s
    return pend.scan_end(copy=False).shape[0]


row = {"lib": tag}
for light in (1, 0):
    scs[0].set_option("efn_light", light)
    for rep in range(3):
        scs[0].scan_device(db)
    ks = []
    for rep in range(12):
        scs[0].scan_device(db)
        ks.append(round(scs[0].last_kernel_ms()[2], 4))
    row["efn_light_ms" if light else "efn_staged_ms"] = {"median": statistics.median(ks), "min": min(ks), "max": max(ks), "all": ks}
scs[0].set_option("efn_light", -1)
turns(20)
ms = []
for rep in range(5):
    t0 = time.perf_counter()
    cand = turns(200)
    ms.append(round((time.perf_counter() - t0) / 200 * 1e3, 4))
row["ms_per_step_in_turns"] = ms
row["candidates"] = cand
print(json.dumps(row), flush=True)
with open(out, "a") as f:
    f.write(json.dumps(row) + "\n")
