"""Databases from FASTA text in HBM (Scanner.database_from_fasta_tensor): one JSON line.

Two FASTA texts: the synthetic 100 entries of 1 Mbase in lines of 60 letters, and the reference's test database 44
times over (179 k entries).  For each, after a warm-up:
  device_ms   database_from_fasta_tensor(text on the GPU), median wall time: the call synchronises
  host_ms     the host route of the same bytes as a file: Pack.read on 16 threads + database_from_pack(wait=True)
The kernels' own times come from a run of their own under the profiler,
  rocprofv3 --kernel-trace --stats -d DIR --output-format csv -- python profiles/device_fasta.py --trace
whose *kernel_stats.csv goes to --stats: per kernel the mean time of a call and a yardstick, the bytes the kernel
moves divided by the rate rma_pack_text_kernel reaches in that same run (1 byte read + 0.375 written per base).  The
trace run makes, per text, the same number of databases, so a kernel's mean is over both texts, as is the yardstick.

usage: python profiles/device_fasta.py [--reps N] [--trace] [--stats CSV] [--out FILE]"""
import argparse
import csv
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


def _fasta(seqs, width=60):
    parts = []
    for i, s in enumerate(seqs):
        a = np.frombuffer(s, dtype=np.uint8)
        full = a.size // width * width
        body = np.concatenate([a[:full].reshape(-1, width), np.full((full // width, 1), 10, dtype=np.uint8)], axis=1).tobytes()
        tail = a[full:].tobytes()
        parts.append(b">s%d entry %d of the measurement\n" % (i, i) + body + (tail + b"\n" if tail else b""))
    return b"".join(parts)


def _median_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(DEV)
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize(DEV)
        out.append((time.perf_counter() - t) * 1e3)
        r.close()
    return statistics.median(out)


def _moved(data: bytes):
    """bytes each kernel reads + writes for this text, and what the pack kernel moves"""
    a = np.frombuffer(data, dtype=np.uint8) | 0x20
    letters = int(np.count_nonzero((a >= ord("a")) & (a <= ord("z"))))
    # (letters of definition lines are counted too: a fraction of a percent of these texts)
    return {"rma_fasta_summarise_kernel": len(data), "rma_fasta_apply_kernel": len(data) + letters, "rma_pack_text_kernel": letters * 1.375}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--trace", action="store_true", help="a few calls per text and nothing else: the run to profile")
    ap.add_argument("--stats", default="", help="kernel_stats.csv of a --trace run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    os.environ.setdefault("EFNDATA", R.EFNDATA_DIR)
    sc = R.Scanner(R.Descriptor(["-descr", os.path.join(ROOT, "tests", "golden", "descr", "trna.descr")]), device=0)
    texts = {"long_100x1M": _fasta(R.synthetic_records(100, length=1_000_000)),
             "short_gbrna_x44": _fasta([r[2] for r in R.read_fasta(os.path.join(ROOT, "tests", "golden", "test", "gbrna.111.0.fastn.gz"))] * 44)}
    res = {"what": "device_fasta", "chunk": R.fasta_device_shape()[0]}
    moved = {}
    for name, data in texts.items():
        for k, v in _moved(data).items():
            moved[k] = moved.get(k, 0) + v
        text = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV)
        if args.trace:
            for _ in range(5):
                sc.database_from_fasta_tensor(text).close()
            continue
        with tempfile.NamedTemporaryFile(suffix=".fa") as f:
            f.write(data)
            f.flush()

            def host():
                pk = R.Pack.read([f.name], threads=16)
                db = sc.database_from_pack(pk, wait=True)
                pk.close()
                return db

            for _ in range(2):
                sc.database_from_fasta_tensor(text).close()
                host().close()
            dev = sc.database_from_fasta_tensor(text)
            res[name] = {"bytes": len(data), "entries": dev.n_seqs, "bases": dev.bases}
            dev.close()
            res[name]["device_ms"] = round(_median_ms(lambda: sc.database_from_fasta_tensor(text), args.reps), 3)
            res[name]["host_ms"] = round(_median_ms(host, max(3, args.reps // 3)), 2)
    if args.stats:
        mean_us = {}
        with open(args.stats) as f:
            for row in csv.DictReader(f):
                for k in ("rma_fasta_summarise_kernel", "rma_fasta_scan_blocks_kernel", "rma_fasta_scan_top_kernel", "rma_fasta_apply_kernel",
                          "rma_fasta_headers_kernel", "rma_pack_text_kernel"):
                    if k in row["Name"]:
                        mean_us[k] = float(row["AverageNs"]) / 1e3
        # both texts count alike in a kernel's mean: bytes per call = the mean over the two texts
        rate = moved["rma_pack_text_kernel"] / 2 / mean_us["rma_pack_text_kernel"]      # bytes per microsecond
        res["kernels_mean_us"] = {k: round(v, 2) for k, v in mean_us.items()}
        res["pack_kernel_GBps"] = round(rate / 1e3, 1)
        res["yardstick_us"] = {k: round(moved[k] / 2 / rate, 2) for k in ("rma_fasta_summarise_kernel", "rma_fasta_apply_kernel")}
    sc.close()
    if not args.trace:
        line = json.dumps(res)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
