"""From a rocprofv3 --kernel-trace csv of profiles/turns_trace.py (two scanners in turns): what ran beside what, as one
JSON line -- the search and the drain kernel's mean times, the share of drain launches that lie inside a search kernel
of the OTHER scanner's queue (whole, and by the share of their time), the gap from a search kernel's end to the next
one's start, and the mean times of the kernels on the chain behind the drain kernel (energies, ordering).
python3 profiles/beside_trace.py <dir with *_kernel_trace.csv> [launches to skip at the start]"""
import csv
import glob
import json
import statistics
import sys

d = sys.argv[1]
skip = int(sys.argv[2]) if len(sys.argv) > 2 else 200
f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))[0]
ev = []
for r in csv.DictReader(open(f)):
    n = r["Kernel_Name"]
    kind = "S" if "rma_search" in n else "D" if "rma_drain" in n else "E" if "rma_efn" in n else n.split("(")[0].split("<")[0]
    ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind, r.get("Queue_Id", "?")))
ev.sort()
ev = ev[skip:]
S = [e for e in ev if e[2] == "S"]
D = [e for e in ev if e[2] == "D"]


def mean_us(rows):
    return round(statistics.mean((e - s) / 1e3 for s, e, _, _ in rows), 1) if rows else None


inside = covered = 0.0
for s, e, _, q in D:
    cov = 0
    for s2, e2, _, q2 in S:
        if q2 != q:
            cov = max(cov, min(e, e2) - max(s, s2))
    covered += max(cov, 0) / max(e - s, 1)
    inside += cov >= e - s
gaps = [(S[i + 1][0] - S[i][1]) / 1e3 for i in range(len(S) - 1)]
others = {}
for s, e, k, _ in ev:
    if k not in ("S", "D"):
        others.setdefault(k, []).append((s, e, k, 0))
print(json.dumps({
    "search_launches": len(S), "search_mean_us": mean_us(S), "drain_mean_us": mean_us(D),
    "drain_launches_wholly_inside_other_search": round(inside / max(len(D), 1), 3),
    "drain_time_share_inside_other_search": round(covered / max(len(D), 1), 3),
    "search_end_to_next_start_us": {"median": round(statistics.median(gaps), 1), "mean": round(statistics.mean(gaps), 1)} if gaps else None,
    "step_us_by_search_starts": round((S[-1][0] - S[0][0]) / 1e3 / max(len(S) - 1, 1), 1) if len(S) > 1 else None,
    "other_kernels_mean_us": {k: mean_us(v) for k, v in sorted(others.items())}}))
