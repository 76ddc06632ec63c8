"""Structures per second of Scanner.structure_energies (rma_structure_energies: the check and energy kernels of
rm_structenergy_dev.hip) on the family efn_random of tests/structure_descr.py -- 296 structures of 12 to 119 bases --
repeated to about a million structures.  One JSON line per case, all of them in profiles/structure_energy_mi355x.json.

  call_ms     HIP events on the caller's stream around one rma_structure_energies() into tensors made beforehand: the
              upload of the codes, the check kernel, the one host wait for its two words and the energy kernel.  The
              median of --reps calls behind two warm-up calls; min and max beside it are the spread.
  per_s       structures / call_ms
  cases       efn alone, efn2 alone, both (both walk the same LDS cache; efn2's tables are read from global memory)
  host        the same cores built for the host (tests/hostsim/struct_energy_check.cpp at -O2, mode `time`): one core,
              the 296 structures over and over, for scale -- not the reference's drivers, which read a .ct file per call

The kernels' own times come from a run under `rocprofv3 --kernel-trace --stats -- python profiles/structure_energy.py`,
a run of its own.  A run without a GPU fails: there is nothing to fall back on.

usage: python profiles/structure_energy.py [--structures N] [--reps N] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

import torch  # first: its HIP runtime serves the process

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rnamotif_amd as R  # noqa: E402
import structure_descr as S  # noqa: E402
import structure_energy as E  # noqa: E402

DEV = torch.device("cuda", 0)
PLAIN = "descr\n\th5( len=3 )\n\t\tss( len=4 )\n\th3\n"
HOST_BIN = os.path.join(ROOT, "tests", "_build", "struct_energy_check_o2")


def host_ns(off, base, pair, tmp, reps):
    if not os.path.exists(HOST_BIN) or os.path.getmtime(HOST_BIN) < os.path.getmtime(E.SRC):
        os.makedirs(os.path.dirname(HOST_BIN), exist_ok=True)
        srcs = [os.path.join(E.H, f + ".cpp") for f in ("rm_regex", "rm_compile", "rm_parse", "rm_score", "rm_efndata", "rm_efn2data", "rm_fasta",
                                                        "rm_driver", "rm_cli", "rm_dump", "rm_pack", "rm_stream", "rm_dev_program")]
        subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + E.H, "-o", HOST_BIN, E.SRC] + srcs, check=True)
    path = os.path.join(tmp, "b.txt")
    E.write_batch(path, off, base, pair)
    out = E.run_checker(HOST_BIN, "time", path, reps)
    m = re.search(r"efn ([0-9.]+) ns a structure, efn2 ([0-9.]+) ns", out)
    return float(m.group(1)), float(m.group(2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--structures", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structure_energy_mi355x.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "no GPU: nothing is measured without one"
    structs = [(s, p) for s, p in S.efn_random()]
    off1, base1, pair1 = E.batch_of(structs)
    times = max(1, a.structures // len(structs))
    n, t1 = times * len(structs), int(off1[-1])
    off = (off1[None, :-1] + (np.arange(times, dtype=np.int64) * t1)[:, None]).reshape(-1)
    off = np.concatenate([off, [times * t1]]).astype(np.int64)
    d_off = torch.from_numpy(off).to(DEV)
    d_base = torch.from_numpy(base1.copy()).to(DEV).repeat(times)
    d_pair = torch.from_numpy(pair1).to(DEV).repeat(times)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "plain.descr")
        with open(path, "w") as f:
            f.write(PLAIN)
        d = R.Descriptor(["-descr", path])
        sc = R.Scanner(d, device=0)
        sc.load_energy_tables()
        want = sc.structure_energies(*(torch.from_numpy(x.copy()).to(DEV) for x in (off1, base1, pair1)))
        e, e2 = torch.empty(n, dtype=torch.int32, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
        err = C.create_string_buffer(4096)
        stream = torch.cuda.current_stream(DEV)
        lines = []
        for case, pe, pe2 in (("efn", e, None), ("efn2", None, e2), ("both", e, e2)):
            ms = []
            for rep in range(a.reps + 2):
                s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(DEV)
                s0.record(stream)
                rc = R.lib().rma_structure_energies(sc._h, d_off.data_ptr(), d_base.data_ptr(), d_pair.data_ptr(), 1, n, n // len(structs) * t1,
                                                    None, pe.data_ptr() if pe is not None else None, pe2.data_ptr() if pe2 is not None else None,
                                                    stream.cuda_stream, err, 4096)
                assert rc == 0, err.value
                s1.record(stream)
                s1.synchronize()
                if rep >= 2:
                    ms.append(s0.elapsed_time(s1))
            # the timed calls computed what one call over the 296 computes
            for got, ref in ((pe, want[0]), (pe2, want[1])):
                assert got is None or torch.equal(got.view(times, -1), ref[None, :].expand(times, -1)), case
            med = statistics.median(ms)
            lines.append({"what": "structure_energy", "case": case, "structures": n, "bases": times * t1, "reps": a.reps,
                          "call_ms": round(med, 4), "call_ms_min": round(min(ms), 4), "call_ms_max": round(max(ms), 4),
                          "per_s": round(n / med * 1e3)})
            print(json.dumps(lines[-1]), flush=True)
        ns = host_ns(off1, base1, pair1, tmp, 200)
        lines.append({"what": "structure_energy_host", "case": "one CPU core, cores at -O2", "structures": len(structs),
                      "efn_ns": ns[0], "efn2_ns": ns[1], "efn_per_s": round(1e9 / ns[0]), "efn2_per_s": round(1e9 / ns[1])})
        print(json.dumps(lines[-1]), flush=True)
        sc.close()
        d.close()
    with open(a.out, "w") as f:
        for l in lines:
            f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
