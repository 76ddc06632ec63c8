"""What the two tests of rma_structure_energies share (tests/test_structure_energy_cpu.py on the host build of
rnamotif_amd/csrc/rm_structenergy.h, tests/test_structure_energy.py on the kernels): structures as the batch the call
takes, the family `noncanonical` with its pins (tests/golden/structure_energy_pins.json, from the reference's efn_drv
and efn2_drv like tests/golden/ref_pins.json), and the host checker tests/hostsim/struct_energy_check.cpp.

A plain module, like structure_descr.py."""
import json
import os
import subprocess

import numpy as np

import structure_descr as S
from ref_pins import RECORD, REF, md5

ROOT = S.ROOT
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
PINS = os.path.join(ROOT, "tests", "golden", "structure_energy_pins.json")
SRC = os.path.join(ROOT, "tests", "hostsim", "struct_energy_check.cpp")
BIN = os.path.join(ROOT, "tests", "_build", "struct_energy_check")
BIN_SAN = BIN + "_san"
EFN_INF, EFN2_INF = 16000, 9999999          # RMA_EFN_INFINITY, RMA_EFN2_INFINITY
MAX_BASES, MAX_HELICES, SMALL_HELICES, CACHE = 8191, 50, 15, 96

_pins = None


def pinned(key, make):
    """ref_pins.pinned() over this module's own file: the pin `key`; with RNAMOTIF_PIN_REF=1 (and oracle/_ref built)
    make() runs the reference's programs and the pin is written afresh."""
    global _pins
    if _pins is None:
        _pins = json.load(open(PINS)) if os.path.exists(PINS) else {}
    if RECORD:
        assert os.path.isdir(REF), "RNAMOTIF_PIN_REF=1 needs oracle/_ref (oracle/Makefile, target ref)"
        _pins[key] = json.loads(json.dumps(make()))
        with open(PINS, "w") as f:
            json.dump(_pins, f, indent=0, sort_keys=True)
            f.write("\n")
    assert key in _pins, "no pin %r in tests/golden/structure_energy_pins.json (RNAMOTIF_PIN_REF=1 with oracle/_ref built records it)" % key
    return _pins[key]


# ---------------------------------------------------------------- the family of pairs no pair set would allow
_CANONICAL = {"au", "ua", "cg", "gc", "gu", "ug"}


def noncanonical():
    """[(name, seq, pairs)]: 40 random structures of efn_random's generator with one to three pairs relettered to
    pairs that are neither Watson-Crick nor G-U (a.a, c.u, n.g, ...).  A descriptor could not produce them (its pair
    set would leave the bases unpaired); the drivers and rma_structure_energies take the pairs as given."""
    from test_efn_oracle import _random_structure
    rng = np.random.default_rng(20261018)
    out = []
    while len(out) < 40:
        seq, pairs = _random_structure(rng, int(rng.integers(12, 120)))
        if not pairs:
            continue
        seq = list(seq)
        for k in rng.choice(len(pairs), size=min(len(pairs), int(rng.integers(1, 4))), replace=False):
            while True:
                a, b = "acgun"[int(rng.integers(0, 5))], "acgun"[int(rng.integers(0, 5))]
                if a + b not in _CANONICAL:
                    break
            seq[pairs[k][0]], seq[pairs[k][1]] = a, b
        out.append(("noncanonical %d" % len(out), "".join(seq), sorted(pairs)))
    return out


def noncanonical_pins(cases):
    """S.pins() for the family: [(efn_drv's kcal/mol, efn2_drv's 1/100 kcal/mol or None)].  The rule for a driver that
    leaves its arrays is structure_descr.efn2_defined's, unchanged: efn2_drv is not run where the exterior walk of
    RM_efn2 would index outside its arrays -- a matter of where the helices stand, not of their letters -- and efn2 must
    be 9999999 there.  Inside their arrays both drivers have a table entry for every letter, n included."""
    sp = [(s, p) for _, s, p in cases]
    cts = md5("".join(S.ct_text(s, p) for s, p in sp).encode())
    pin = pinned("efn_drv energy and efn2_drv dG, noncanonical structures",
                 lambda: {"input": cts, "energy": S._efn_drv(sp), "dG": S._efn2_drv(sp)})
    assert pin["input"] == cts, "not the structures the pin of noncanonical was made from"
    assert len(pin["energy"]) == len(pin["dG"]) == len(cases)
    return list(zip(pin["energy"], pin["dG"]))


def all_families():
    """S.families() and `noncanonical`, with their pins: {family: ([(name, seq, pairs)], [pin])}"""
    fam = {f: (cases, S.pins(f, cases)) for f, cases in S.families().items()}
    nc = noncanonical()
    fam["noncanonical"] = (nc, noncanonical_pins(nc))
    return fam


# ---------------------------------------------------------------- structures as the call takes them
def batch_of(structs):
    """(off int64 [n+1], base uint8 [T], pair int32 [T]) of [(seq, pairs)], pairs as (i, j) tuples"""
    off = np.zeros(len(structs) + 1, dtype=np.int64)
    base, pair = [], []
    for k, (seq, pairs) in enumerate(structs):
        off[k + 1] = off[k] + len(seq)
        base.append(np.frombuffer(seq.encode(), dtype=np.uint8))
        pair.append(np.asarray(S.partners(seq, pairs), dtype=np.int32))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dtype=dt)     # noqa: E731
    return off, cat(base, np.uint8), cat(pair, np.int32)


def hairpin(total, stem=4):
    """a hairpin of `total` bases"""
    seq, dots = S._hp("gcgc"[:stem], "a" * (total - 2 * stem))
    return seq, S._pairs_of(dots)


def chain(helices):
    """`helices` hairpins of three pairs side by side: that many helices"""
    seq, dots = S._cat("a", *[S._hp("gcc", "gaaa") for _ in range(helices)])
    return seq, S._pairs_of(dots)


# ---------------------------------------------------------------- the host checker
def _compile(out, extra):
    srcs = [os.path.join(H, f + ".cpp") for f in ("rm_regex", "rm_compile", "rm_parse", "rm_score", "rm_efndata", "rm_efn2data",
                                                  "rm_fasta", "rm_driver", "rm_cli", "rm_dump", "rm_pack", "rm_stream", "rm_dev_program")]
    return subprocess.Popen(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread"] + extra +
                            ["-I" + os.path.join(ROOT, "include"), "-I" + H, "-o", out, SRC] + srcs)


def build_checker(sanitized=True):
    """tests/_build/struct_energy_check and, with `sanitized`, the same program under -fsanitize=address,undefined,
    compiled side by side when they are older than what they are made of."""
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    newest = max(os.path.getmtime(f) for f in [SRC] + [os.path.join(H, h) for h in ("rm_structenergy.h", "rm_efn_core.h", "rm_efn2_core.h")])
    jobs = [_compile(out, extra) for out, extra in ((BIN, []), (BIN_SAN, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]))[:2 if sanitized else 1]
            if not os.path.exists(out) or os.path.getmtime(out) < newest]
    for j in jobs:
        assert j.wait() == 0
    return BIN, BIN_SAN


def run_checker(binary, *args, timeout=600):
    p = subprocess.run([binary, S.EFNDATA] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0, (p.returncode, p.stdout[-300:], p.stderr[-2000:])
    return p.stdout.decode()


def write_batch(path, off, base, pair):
    with open(path, "w") as f:
        f.write("%d %d\n%s\n%s\n%s\n" % (len(off) - 1, len(base), " ".join(str(int(o)) for o in off),
                                        bytes(base).decode() if len(base) else "-", " ".join(str(int(p)) for p in pair)))


def host_batch(binary, path, off, base, pair):
    """the checker over one batch: ("refused", s, reason, which) or [(efn, efn2, helices, inf)]"""
    write_batch(path, off, base, pair)
    lines = run_checker(binary, "batch", path).splitlines()
    if lines and lines[0].startswith("refused"):
        w = lines[0].split()
        return ("refused", int(w[1]), w[2], int(w[3]))
    rows = [tuple(int(v) for v in l.split()) for l in lines]
    assert [r[0] for r in rows] == list(range(len(off) - 1))
    return [r[1:] for r in rows]
