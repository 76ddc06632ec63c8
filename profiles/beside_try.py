"""Two scanners taking the steps in turns (bench.py's step): ms a step by the search kernel's workgroups per CU
(search_wgs), the drain kernel's waves per CU (drain_waves) and the shape that guarantees the drain kernel room
(beside), next to one scan's kernels alone under the same switches -- the table of DESIGN.md 4, "What runs beside what".
A library from before option beside (RNAMOTIF_AMD_LIB) runs the rows it knows: the two builds go in turns that way.
python profiles/beside_try.py TAG OUT.json"""
import json
import os
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
has_beside = hasattr(R.lib(), "rma_scanner_last_launch")


def run(n):
    pend = None
    for i in range(n):
        s = scs[i & 1]
        s.scan_begin(db)
        if pend is not None:
            pend.scan_end(copy=False)
        pend = s
    return pend.scan_end(copy=False).shape[0]


CFG = [(0, 6, 0), (4, 3, 0), (4, 4, 0), (4, 2, 0)]
if has_beside:
    CFG += [(0, 6, 1), (0, 3, 1), (0, 6, -1)]
CFG += [(0, 6, 0)]
rows = []
for wgs, dw, be in CFG:
    for s in scs:
        s.set_option("search_wgs", wgs)
        s.set_option("drain_waves", dw)
        if has_beside:
            s.set_option("beside", be)
    run(6)
    ms = []
    for rep in range(3):
        t0 = time.perf_counter()
        n = 200
        cand = run(n)
        ms.append(round((time.perf_counter() - t0) / n * 1e3, 4))
    ll = scs[1].last_launch() if has_beside else None
    # one scan alone with the same switches (beside = -1 resolves to 0 there)
    ks = []
    for rep in range(3):
        scs[0].scan_device(db)
        k = scs[0].last_kernel_ms()
        ks.append([round(k[0], 4), round(k[1], 4), round(k[2], 4)])
    row = {"lib": tag, "search_wgs": wgs, "drain_waves": dw, "beside": be, "ms_per_step_in_turns": ms,
           "solo_search_drain_efn_ms": ks, "last_launch_in_turns": ll, "candidates": cand}
    rows.append(row)
    print(json.dumps(row), flush=True)
with open(out, "w") as f:
    json.dump(rows, f, indent=1)
