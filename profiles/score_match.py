"""What =~ in a score section costs on the device (Scanner.score with ScoreProgram(d, match=True)): one JSON line.

An own descriptor whose MAIN judges a loop and a helix strand by =~ (WITH), over the records the scan finds in the first
entries of the reference's test database (tests/golden/test/gbrna.111.0.fastn.gz), rows repeated to --records:
  match_ms    Scanner.score( db, hits, ScoreProgram( WITH, match=True ) ): rma_score_match_kernel
  plain_ms    Scanner.score( db, hits, ScoreProgram( WITHOUT ) ), the same program with its match lines removed:
              rma_score_kernel -- the difference is what the matcher costs
  replay_ms   Replay.device( db, hits, accepted=True ) of WITH: windows to the host, one thread of the host VM -- what a
              program with =~ had before
match_ms and plain_ms are HIP events around the call on the caller's stream (the call itself waits once), replay_ms
is wall clock around the call ending in a synchronise; each after warm-up calls, the median of --reps.  A library
whose ScoreProgram has no `match` measures plain_ms and replay_ms alone: run at the parent commit with --out, they are
the bar, and --parent FILE takes them from there into the line this commit writes.

usage: python profiles/score_match.py [--records N] [--reps N] [--commit ID] [--parent FILE] [--out FILE]"""
import argparse
import gzip
import inspect
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
HP = ("parms\n\twc += gu;\ndescr\n\th5( tag='a', minlen=4, maxlen=6, mispair=1 )\n\t\tss( tag='l', minlen=4, maxlen=6, seq=\"ga\", mismatch=1 )\n"
      "\th3( tag='a' )\n\tss( tag='t', len=2 )\nscore\n")
MATCH_LINES = ("\t  if( ss( tag='l' ) =~ \"^g.*a$\" ) SCORE = SCORE + 100;\n"
               "\t  if( h5( tag='a' ) =~ \"\\(.\\)\\1\" ) REJECT;\n")
WITH = HP + "\t{ SCORE = LEN + mispairs( h5( tag='a' ) );\n" + MATCH_LINES + "\t}\n"
WITHOUT = HP + "\t{ SCORE = LEN + mispairs( h5( tag='a' ) );\n\t}\n"


def _events(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(DEV)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize(DEV)
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out)


def _wall(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(DEV)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(DEV)
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--entries", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--commit", default="", help="the commit this library was built from")
    ap.add_argument("--parent", default="", help="a line this script wrote at the parent commit: its plain_ms and replay_ms are the bar")
    ap.add_argument("--out", default="", help="also write the JSON line to this file")
    args = ap.parse_args()
    os.environ.setdefault("EFNDATA", R.EFNDATA_DIR)
    tmp = tempfile.mkdtemp()
    fasta = os.path.join(tmp, "gbrna.fastn")
    with gzip.open(os.path.join(ROOT, "tests", "golden", "test", "gbrna.111.0.fastn.gz"), "rb") as f, open(fasta, "wb") as g:
        g.write(f.read())
    seqs = [s for _, _, s in R.read_fasta(fasta)[:args.entries]]
    paths = {}
    for name, text in (("with", WITH), ("without", WITHOUT)):
        paths[name] = os.path.join(tmp, name + ".descr")
        with open(paths[name], "w") as f:
            f.write(text)
    d_with, d_without = R.Descriptor(["-descr", paths["with"]]), R.Descriptor(["-descr", paths["without"]])
    sc = R.Scanner(d_without, device=0)
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    text = torch.from_numpy(np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()).to(DEV)
    db = sc.database_from_tensor(text, offsets=off)
    found = sc.scan_tensor(db)
    torch.cuda.synchronize(DEV)
    n_found = int(found.shape[0])
    idx = torch.arange(args.records, device=DEV, dtype=torch.int64) % n_found
    hits = found[idx].contiguous()
    res = {"what": "score_match", "commit": args.commit, "database": "the first %d entries of gbrna.111.0.fastn" % len(seqs), "found": n_found,
           "records": int(hits.shape[0]), "reps": args.reps, "measured": "on an MI355X, medians (min in *_min_ms)"}
    plain = R.ScoreProgram(d_without)
    out_plain = sc.score(db, hits, plain)
    med, low = _events(lambda: sc.score(db, hits, plain), args.reps)
    res.update(plain_ms=round(med, 3), plain_min_ms=round(low, 3), plain_info=plain.info(), plain_accepted=int(out_plain.accept.sum()))
    plain.close()
    has_match = "match" in inspect.signature(R.ScoreProgram.__init__).parameters
    # the scanner of the descriptor with =~: the same descr section, a program of its own
    sc2 = R.Scanner(d_with, device=0)
    db2 = sc2.database_from_tensor(text, offsets=off)
    rp = R.Replay(d_with, os.devnull)
    n_acc, mask = rp.device(db2, hits, accepted=True)
    med, low = _wall(lambda: rp.device(db2, hits, accepted=True), max(3, args.reps // 3))
    rp.close()
    res.update(replay_ms=round(med, 3), replay_min_ms=round(low, 3), replay_accepted=int(n_acc))
    if has_match:
        prog = R.ScoreProgram(d_with, match=True)
        s = sc2.score(db2, hits, prog)
        torch.cuda.synchronize(DEV)
        acc = s.accept.cpu().numpy()
        assert int(acc.sum()) == int(n_acc) and np.array_equal(acc, np.asarray(mask.cpu() if hasattr(mask, "cpu") else mask, dtype=bool)), "the kernel and the replay differ"
        assert 0 < int(acc.sum()) < len(acc)
        med, low = _events(lambda: sc2.score(db2, hits, prog), args.reps)
        res.update(match_ms=round(med, 3), match_min_ms=round(low, 3), match_info=prog.info(), match_accepted=int(acc.sum()))
        prog.close()
    if args.parent:
        p = json.loads(open(args.parent).read().strip().split("\n")[-1])
        res["parent"] = {k: p[k] for k in ("commit", "records", "plain_ms", "plain_min_ms", "plain_info", "replay_ms", "replay_min_ms", "replay_accepted") if k in p}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    db2.close()
    sc2.close()
    db.close()
    sc.close()


if __name__ == "__main__":
    main()
