"""CPU: the text of a packed database as rnamotif_amd/csrc/rm_dbtext.h states it for the host and for the kernels of
rm_dbtext_dev.hip, run on the host through tests/hostsim/dbtext_check.cpp the way the kernels run it -- the rank
directory, the per-entry check, the fill slot by slot in groups of 64 -- and held to PackFile::unpack:

  * entries of 0, 1, 15, 16, 17, 31, 32, 33, 2047, 2048, 2049 and 4097 bases; exceptions at base 0, at the last base, on
    either side of a slot seam, a mask-word seam and a 2048-base run seam; an entry of nothing but exceptions; entries
    with none between entries with some; in the pack's order, in reverse with entries twice, without exceptions (n),
    and with every padding bit of the mask set;
  * the same once more with the checker built with -fsanitize=address,undefined as a stand-alone program;
  * the rule's index arithmetic with base_off and exc_off above 2^32 and p = 2^31 - 2 against Python integers."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "hostsim", "dbtext_check.cpp")

LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 2047, 2048, 2049, 4097]
AMBIGUOUS = b"nryswkmbdhv"
SEAMS = [0, 15, 16, 31, 32, 63, 64, 2047, 2048, 4096]      # of slots, mask words and runs; base 0 and the last base


def make_records(seed=7, frac=0.02, many=0, long=0):
    """(sid, sdef, seq) records: the lengths above with `frac` ambiguous letters, an entry with exceptions exactly at
    the seams, entries of nothing but exceptions, entries with none; then `many` entries of 0..70 bases and, with
    `long`, one of that many bases."""
    rng = np.random.default_rng(seed)
    acgt, amb = np.frombuffer(b"acgt", dtype=np.uint8), np.frombuffer(AMBIGUOUS, dtype=np.uint8)

    def entry(n, f):
        s = acgt[rng.integers(0, 4, n)]
        m = rng.random(n) < f
        s[m] = amb[rng.integers(0, len(amb), int(m.sum()))]
        return s

    seqs = [entry(n, frac) for n in LENGTHS]
    s = entry(4097, 0.0)
    s[SEAMS] = amb[rng.integers(0, len(amb), len(SEAMS))]
    seqs.append(s)
    seqs += [entry(33, 0.0), entry(100, 1.0), entry(2048, 0.0), entry(2049, 1.0), entry(17, 0.0), entry(2049, frac)]
    seqs += [entry(int(rng.integers(0, 71)), frac) for _ in range(many)]
    if long:
        seqs.append(entry(long, frac))
    n = len(seqs)
    return [(b"e%d" % i, b"entry %d of %d" % (i, n), s.tobytes()) for i, s in enumerate(seqs)]


def build(name, flags):
    out = os.path.join(ROOT, "tests", "_build", name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    deps = [SRC] + [os.path.join(H, f) for f in ("rm_dbtext.h", "rm_pack.h", "rm_pack.cpp", "rm_fasta.h", "rm_fasta.cpp")]
    if not (os.path.exists(out) and os.path.getmtime(out) >= max(os.path.getmtime(f) for f in deps)):
        subprocess.run(["g++"] + flags + ["-std=c++17", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + H, "-o", out, SRC,
                        os.path.join(H, "rm_pack.cpp"), os.path.join(H, "rm_fasta.cpp")], check=True)
    return out


VARIANTS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module")
def pack_path(built, tmp_path_factory):
    import rnamotif_amd as R
    path = str(tmp_path_factory.mktemp("packed_text") / "cases.rmdb")
    recs = make_records(many=40)
    R.Pack.write(path, recs)
    return path, recs


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_rule_is_unpack_on_every_entry(pack_path, variant):
    path, recs = pack_path
    p = subprocess.run([build("dbtext_check_" + variant, VARIANTS[variant]), "pack", path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, (p.stdout.decode(), p.stderr.decode())
    w = p.stdout.decode().split()
    n = len(recs)
    twice = sum(1 for i in range(n) if i % 3 == 0)
    slots = sum((len(r[2]) + 15) // 16 for r in recs)
    slots_twice = sum((len(r[2]) + 15) // 16 for i, r in enumerate(recs) if i % 3 == 0)
    assert w[0] == "ok" and int(w[1]) == 4 * n + twice and int(w[2]) == 4 * slots + slots_twice, w
    # both ways to a rank were taken: groups of 64 slots inside one entry and groups over several
    groups = 3 * ((slots + 63) // 64) + (slots + slots_twice + 63) // 64
    assert int(w[3]) > 0 and int(w[4]) > 0 and int(w[3]) + int(w[4]) == groups, w


def test_pack_holds_the_cases(pack_path):
    """What the generated entries are there for, seen in the pack itself."""
    import rnamotif_amd as R
    path, recs = pack_path
    pk = R.Pack(path)
    assert pk.lengths()[:len(LENGTHS)] == LENGTHS
    seam = pk.seq(len(LENGTHS))
    assert [p for p in range(len(seam)) if seam[p:p + 1] not in (b"a", b"c", b"g", b"t")] == SEAMS
    assert all(pk.seq(i) == r[2] for i, r in enumerate(recs))
    every = pk.seq(len(LENGTHS) + 2)
    assert len(every) == 100 and not set(every) & set(b"acgt")


@pytest.mark.parametrize("base_off,p,exc_base,dir_run,in_run,below", [
    ((1 << 33) + 96, (1 << 31) - 2, (1 << 34) + 12345, (1 << 32) + 7, 2047, 15),
    ((1 << 32) + 32, 0, -(1 << 32) - 5, (1 << 33), 0, 0),
    (0, 33, 0, 0, 1, 1),
])
def test_index_arithmetic_is_64_bit(base_off, p, exc_base, dir_run, in_run, below):
    out = subprocess.run([build("dbtext_check_plain", VARIANTS["plain"]), "index"] + [str(x) for x in (base_off, p, exc_base, dir_run, in_run, below)],
                         stdout=subprocess.PIPE, check=True).stdout.decode().split()
    mw = base_off // 32 + p // 32
    want = [base_off // 16 + p // 16, mw, mw // 64, mw - mw % 64, exc_base + dir_run + in_run + below, (p + 15) // 16 * 16]
    assert [int(x) for x in out] == want
