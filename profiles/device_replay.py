"""Replay of a device database from its text in HBM (Replay.device, rma_replay_device): one JSON line.

trna.descr over the synthetic 100 x 1 Mbase database bench.py uses (iid uniform acgt, seed 20240601), as one
1-D uint8 tensor on the GPU: database_from_tensor, scan_tensor, then for the same records
  device_ms       Replay.device(db, hits): span kernel, scan, gather kernel, the copies, the host replay
  workaround_ms   text.cpu() + Replay.batch(the entries, hits.cpu()): every base across PCIe
  replay_ms       Replay.pack over the same entries packed on the host: the same replay (one_hit: score program
                  and printer) over windows the host rebuilds from packed bits
  device_part_ms  device_ms - replay_ms: only a bound -- replay_ms holds host work of its own -- the device
                  part is measured by the kernel trace below
The three outputs are byte for byte equal (asserted).  Times are medians of wall clock around the calls alone,
on one replay handle (its buffers made by an earlier call), each ending in a synchronise.  The kernels' own times are in a rocprofv3 --kernel-trace --stats run of this script
(rma_hit_span_kernel, rma_hit_gather_kernel, rocPRIM's scan).

usage: python profiles/device_replay.py [--reps N] [--out FILE] [--tmp DIR]"""
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


def _timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(DEV)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(DEV)
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    ap.add_argument("--tmp", default="", help="directory for the printed output (default: a temporary one)")
    args = ap.parse_args()
    os.environ.setdefault("EFNDATA", R.EFNDATA_DIR)
    tmp = args.tmp or tempfile.mkdtemp()
    os.makedirs(tmp, exist_ok=True)
    d = R.Descriptor(["-descr", os.path.join(ROOT, "tests", "golden", "descr", "trna.descr")])
    sc = R.Scanner(d, device=0)
    sc.warmup()
    seqs = R.synthetic_records(100, length=1_000_000)
    sids = [b"syn%04d" % i for i in range(len(seqs))]
    sdefs = [b"synthetic"] * len(seqs)
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    text = torch.from_numpy(np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()).to(DEV)
    db = sc.database_from_tensor(text, offsets=off, wait=True)
    hits = sc.scan_tensor(db)
    torch.cuda.synchronize(DEV)
    n_rec = int(hits.shape[0])
    pk_path = os.path.join(tmp, "syn.rmpack")
    R.Pack.write(pk_path, list(zip(sids, sdefs, seqs)))
    pk = R.Pack(pk_path)
    recs = hits.cpu().numpy()
    outs = {}
    # the outputs, once each, byte for byte equal
    rp = R.Replay(d, os.path.join(tmp, "device.txt"))
    outs["device"] = rp.device(db, hits, sids=sids, sdefs=sdefs)
    rp.close()
    host = text.cpu().numpy().tobytes()
    rp = R.Replay(d, os.path.join(tmp, "workaround.txt"))
    outs["workaround"] = rp.batch(sids, sdefs, [host[off[i]:off[i + 1]] for i in range(len(seqs))], recs)
    rp.close()
    rp = R.Replay(d, os.path.join(tmp, "pack.txt"))
    outs["pack"] = rp.pack(pk, recs)
    rp.close()
    texts = [open(os.path.join(tmp, f), "rb").read() for f in ("device.txt", "workaround.txt", "pack.txt")]
    assert texts[0] == texts[1] == texts[2] and outs["device"] == outs["workaround"] == outs["pack"], outs
    # the calls alone, each kind on one replay handle of its own (its buffers made by the first call above)
    rp = R.Replay(d, os.devnull)
    rp.device(db, hits, sids=sids, sdefs=sdefs)
    dev_ms = _timed(lambda: rp.device(db, hits, sids=sids, sdefs=sdefs), args.reps)

    def workaround():
        h = text.cpu().numpy().tobytes()
        rp.batch(sids, sdefs, [h[off[i]:off[i + 1]] for i in range(len(seqs))], hits.cpu().numpy())
    work_ms = _timed(workaround, max(3, args.reps // 2))
    rep_ms = _timed(lambda: rp.pack(pk, recs), args.reps)
    rp.close()
    window_bytes = 0
    for w in recs:
        offs = [(w[5 + 4 * e], w[6 + 4 * e]) for e in range(d.n_elems)]
        lo = min(o for o, n in offs if n > 0)
        hi = max(o + n for o, n in offs if n > 0)
        window_bytes += hi - lo
    res = {"what": "device_replay", "descr": "trna.descr", "database": "100 x 1 Mbase synthetic, one uint8 tensor",
           "records": n_rec, "printed": outs["device"], "output_bytes": len(texts[0]),
           "window_bytes": int(window_bytes), "record_bytes": n_rec * d.hit_stride * 4, "text_bytes": int(off[-1]),
           "device_ms": round(dev_ms, 3), "workaround_ms": round(work_ms, 3), "replay_ms": round(rep_ms, 3),
           "device_part_ms": round(dev_ms - rep_ms, 3), "identical_output": True, "reps": args.reps,
           "measured": "wall clock on an MI355X, medians"}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    pk.close()
    db.close()
    sc.close()


if __name__ == "__main__":
    main()
