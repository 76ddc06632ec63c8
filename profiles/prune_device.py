"""rmprune's rule on the device (Scanner.prune, rma_prune_hits) against what a caller did without it: one JSON line
per case.

  events_ms   HIP events on the caller's stream around rma_prune_hits() into a tensor made beforehand: the keys, scan,
              list and rezip kernels of rm_prune_dev.hip and the one host wait (the check, the number of blocks)
  host_ms     the route without the call, wall clock: the records copied to the host, the same rule on one core
              (tests/hostsim/prune_check.cpp, its files written and read included), the mask copied up
  ratio       host_ms / events_ms

The kernels' own times come from a run under `rocprofv3 --kernel-trace --stats -- python profiles/prune_device.py`,
a run of its own.

cases: trna over 100 x 1 Mbase synthetic; a permissive hairpin whose blocks are full (1000 records in one group).

usage: python profiles/prune_device.py [--reps N] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch  # first: its HIP runtime serves the process

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rnamotif_amd as R  # noqa: E402

DEV = torch.device("cuda", 0)
CHECK = os.path.join(ROOT, "tests", "_build", "prune_check")
HAIRPIN = "descr\n\th5( minlen=3, maxlen=30 )\n\t\tss( minlen=3, maxlen=40 )\n\th3\n"


def checker():
    src = os.path.join(ROOT, "tests", "hostsim", "prune_check.cpp")
    if not os.path.exists(CHECK):
        os.makedirs(os.path.dirname(CHECK), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "rnamotif_amd", "csrc"),
                        "-o", CHECK, src], check=True)
    return CHECK


def measure(name, d, sc, db, hits, slens, reps, tmp):
    n = int(hits.shape[0])
    keep = sc.prune(db, hits)
    torch.cuda.synchronize(DEV)
    err = C.create_string_buffer(4096)
    stream = torch.cuda.current_stream(DEV)
    ev = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(DEV)
        a.record(stream)
        rc = R.lib().rma_prune_hits(sc._h, db._h, hits.data_ptr(), n, None, keep.data_ptr(), stream.cuda_stream, err, 4096)
        assert rc == 0, err.value
        b.record(stream)
        b.synchronize()
        ev.append(a.elapsed_time(b))
    prog, ent, rec = (os.path.join(tmp, f) for f in ("program.bin", "lengths.bin", "records.bin"))
    with open(prog, "wb") as f:
        f.write(C.string_at(d.program, int(np.frombuffer(C.string_at(d.program, 8), dtype=np.uint32)[1])))       # (word 1: its size)
    np.asarray([len(slens)] + list(slens), dtype=np.int32).tofile(ent)
    host, counts, mask = [], "", None
    for _ in range(max(3, reps // 4)):
        torch.cuda.synchronize(DEV)
        t0 = time.perf_counter()
        hits.cpu().numpy().tofile(rec)
        p = subprocess.run([checker(), "mask", prog, ent, rec, "-"], stdout=subprocess.PIPE, check=True)
        line, counts = p.stdout.decode().split("\n")[:2]
        mask = torch.from_numpy(np.frombuffer(line.encode(), dtype=np.uint8) == ord("1")).to(DEV)
        torch.cuda.synchronize(DEV)
        host.append((time.perf_counter() - t0) * 1e3)
    assert torch.equal(mask, keep), name
    e, h = statistics.median(ev), statistics.median(host)
    return {"what": "prune_device", "case": name, "records": n, "kept": int(keep.sum()), "counts": counts, "events_ms": round(e, 4),
            "events_ms_min": round(min(ev), 4), "host_ms": round(h, 3), "ratio": round(h / e, 2), "reps": reps,
            "measured": "one MI355X, medians; events_ms by HIP events, host_ms wall clock"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="", help="also write the JSON lines to this file")
    args = ap.parse_args()
    os.environ.setdefault("EFNDATA", R.EFNDATA_DIR)
    tmp = tempfile.mkdtemp()
    lines = []
    # trna over 100 x 1 Mbase
    d = R.Descriptor(["-descr", os.path.join(ROOT, "tests", "golden", "descr", "trna.descr")])
    sc = R.Scanner(d, device=0)
    sc.warmup()
    seqs = R.synthetic_records(100, length=1_000_000)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    text = torch.from_numpy(np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()).to(DEV)
    db = sc.database_from_tensor(text, offsets=off, wait=True)
    lines.append(measure("trna, 100 x 1 Mbase synthetic", d, sc, db, sc.scan_tensor(db), [len(s) for s in seqs], args.reps, tmp))
    db.close()
    sc.close()
    # a permissive hairpin over a short perfect hairpin repeated: every record of an entry inside the first one's span
    path = os.path.join(tmp, "hairpin.descr")
    with open(path, "w") as f:
        f.write(HAIRPIN)
    d = R.Descriptor(["-descr", path])
    sc = R.Scanner(d, device=0)
    arm = b"gcgcgcatatatgcgcgcatatatgcgcgc"
    rc = arm[::-1].translate(bytes.maketrans(b"acgt", b"tgca"))
    seqs = [arm + b"ttttcttttc"[:4 + k % 6] + rc for k in range(64)]
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    text = torch.from_numpy(np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()).to(DEV)
    db = sc.database_from_tensor(text, offsets=off, wait=True)
    hits = sc.scan_tensor(db)
    # whole blocks: the records of an entry whose span lies inside the first one's, repeated up to 1000 an entry
    recs = hits.cpu().numpy()
    rows = []
    for e in range(len(seqs)):
        r = recs[recs[:, 0] == e]
        lead = r[np.argmax(2 * r[:, 6] + r[:, 10])] if len(r) else None         # (the widest: 2 x the helix + the loop)
        if lead is None:
            continue
        rows.append(np.concatenate([lead[None], np.concatenate([r] * (1000 // max(len(r), 1) + 1))])[:1000])
    full = torch.from_numpy(np.ascontiguousarray(np.concatenate(rows))).to(DEV)
    lines.append(measure("hairpin, %d blocks of 1000" % len(rows), d, sc, db, full, [len(s) for s in seqs], max(3, args.reps // 4), tmp))
    db.close()
    sc.close()
    for ln in lines:
        print(json.dumps(ln))
    if args.out:
        with open(args.out, "w") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
