"""The text of a packed database made in HBM (Database.device_text): one JSON line.

A pack of N entries of 1 Mbase, 0.1 % of the letters n or IUPAC (--entries 100, and 1000 for a gigabase).  After a
warm-up, medians of --reps:
  call_ms      Database.device_text() on a fresh database_from_pack() of the pack: the exceptions up, the rank
               directory, the check, the fill, its one wait -- a host clock around a call that ends in a synchronise
  fill_ms      the fill kernel alone (HIP events around it inside the call: rma_db_text_fill_ms)
  copy_ms      a device-to-device copy of as many bytes as the fill writes, in this process (HIP events): the
               yardstick for a kernel that reads 3 bits and writes 8 a base
  old_ms       today's route to the same text on the same pack: Pack.seq() of every entry, one upload,
               database_from_tensor(wait=True) -- a host clock, --old-reps of them
and the ratios fill_ms / copy_ms and old_ms / call_ms.

usage: python profiles/packed_text.py [--entries N] [--reps N] [--old-reps N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch  # first: its HIP runtime serves the process

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import rnamotif_amd as R  # noqa: E402

DEV = torch.device("cuda", 0)
MBASE = 1_000_000


def make_pack(path, entries, seed=5):
    rng = np.random.default_rng(seed)
    acgt, amb = np.frombuffer(b"acgt", dtype=np.uint8), np.frombuffer(b"nryswkmbdhv", dtype=np.uint8)
    recs = []
    for i in range(entries):
        s = acgt[rng.integers(0, 4, MBASE)]
        at = rng.choice(MBASE, MBASE // 1000, replace=False)
        s[at] = amb[rng.integers(0, len(amb), len(at))]
        recs.append((b"e%d" % i, b"", s.tobytes()))
    R.Pack.write(path, recs)
    return R.Pack(path)


def case(sc, pk, reps, old_reps):
    bases = pk.bases
    text_bytes = sum((n + 15) // 16 * 16 for n in pk.lengths())
    call, fill = [], []
    for r in range(reps + 2):          # (two warm-ups: the kernels' code objects, the block cache)
        db = sc.database_from_pack(pk)
        torch.cuda.synchronize(DEV)
        t = time.perf_counter()
        db.device_text()
        dt = (time.perf_counter() - t) * 1e3
        if r >= 2:
            call.append(dt)
            fill.append(float(R.lib().rma_db_text_fill_ms(db._h)))
        if r == 0:
            assert all(db.read_text(i) == pk.seq(i) for i in (0, pk.count - 1))
        db.close()
    src = torch.randint(0, 255, (text_bytes,), dtype=torch.uint8, device=DEV)
    dst = torch.empty_like(src)
    copy = []
    for r in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(DEV)
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize(DEV)
        if r >= 2:
            copy.append(a.elapsed_time(b))
    del src, dst
    old = []
    for r in range(old_reps + 1):
        torch.cuda.synchronize(DEV)
        t = time.perf_counter()
        seqs = [pk.seq(i) for i in range(pk.count)]
        off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
        text = torch.frombuffer(bytearray(b"".join(seqs)), dtype=torch.uint8).to(DEV)
        db = sc.database_from_tensor(text, offsets=off, wait=True)
        torch.cuda.synchronize(DEV)
        if r >= 1:
            old.append((time.perf_counter() - t) * 1e3)
        db.close()
        del text, seqs
    m = {k: statistics.median(v) for k, v in (("call_ms", call), ("fill_ms", fill), ("copy_ms", copy), ("old_ms", old))}
    out = {"entries": pk.count, "bases": bases, "text_bytes": text_bytes}
    out.update({k: round(v, 4) for k, v in m.items()})
    out["fill_GBps"] = round((bases * 0.375 + text_bytes) / m["fill_ms"] / 1e6, 1)
    out["copy_GBps"] = round(2 * text_bytes / m["copy_ms"] / 1e6, 1)
    out["fill_over_copy"] = round(m["fill_ms"] / m["copy_ms"], 3)
    out["old_over_call"] = round(m["old_ms"] / m["call_ms"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, nargs="+", default=[100])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--old-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d = R.Descriptor(["-descr", os.path.join(ROOT, "tests", "golden", "descr", "trna.descr")])
    sc = R.Scanner(d, device=0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "old_reps": a.old_reps, "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        for n in a.entries:
            pk = make_pack(os.path.join(tmp, f"p{n}.rmdb"), n)
            res["cases"].append(case(sc, pk, a.reps, a.old_reps))
            pk.close()
            print(json.dumps(res["cases"][-1]), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
