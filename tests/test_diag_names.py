"""CPU: the names of the scan's diagnostic bits and counter slots (rnamotif_amd/csrc/rm_diag.h).

  * the RMK_DBG_* bits of the header, rnamotif_amd.DBG and the switches table of DESIGN.md say the same;
  * the RMK_C_* slots, as the compiler sees them (tests/hostsim/diag_slots.cpp), are the numbers the kernels and the
    scanner used as literals before the header existed -- a renumbering shows here;
  * no source under rnamotif_amd/csrc tests `dbg` against, or offsets a counter pointer by, a decimal literal."""
import os
import re
import subprocess

from rnamotif_amd import DBG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "_build", "diag_slots")

# Index from the start of the counter block (rma_scanner::d_counters).  The kernels wrote `hb.ticket + n` for slot
# n + 1; the scanner read `d_counters + 1 + n`, `h_ctr[ n ]` or, in the report, `lv[ n - 16 ]`.
SLOTS = {
    "COUNT": 0, "TICKET": 1, "QUEUED": 2, "QUEUE_NEED": 3, "PIECE_OVERFLOW": 3, "PHASE": 4,
    # general instances: ticket + 15 + 2 * kk, ticket + 16 + 2 * kk, kk < 32
    "GEN_LEVEL": 16,
    # lean search instances: ticket + 15 .. 22, 23 + log2, 60 + level, 76 + level, 92, 93
    "POP_ROUNDS": 16, "POP_LANES": 17, "STEPS": 18, "STEP_LANES": 19, "POP_CYCLES": 20, "STEP_CYCLES": 21,
    "STEP_LONGEST": 22, "WAVE_MOST": 23, "STEP_LOG2": 24, "LEVEL_CYCLES": 61,
    "LEVEL_STEPS": 77, "EMIT_CYCLES": 93, "EMITTED": 94,
    # ... their timeline: ticket + 87 .. 91
    "TL_WGS": 88, "TL_START": 89, "TL_DRY_SUM": 90, "TL_DONE_MAX": 91, "TL_DONE_SUM": 92,
    # drain kernel: ticket + 17, 18, 20, 21, 22, 23 + log2, 60 + bin, 76 + bin, 93, DRAIN_LAP( 94 .. 97 ), 98; 23 + bin, 55
    "DRAIN_ITEMS": 18, "DRAIN_STEPS": 19, "DRAIN_CYCLES": 21, "DRAIN_LONGEST": 22, "DRAIN_MOST_STEPS": 23,
    "DRAIN_LOG2": 24, "DRAIN_EMIT_ITEMS": 61, "DRAIN_EMIT_CYCLES": 77, "DRAIN_LANES": 94,
    "DRAIN_LAP": 95, "DRAIN_ROUNDS": 99, "DRAIN_DONE": 24, "DRAIN_START": 56,
    # the list: ticket + ( RMK_GCTL - 1 ), ticket + RMK_GCTL, ticket + ( RMK_GCTL + 1 ); RMK_GCTL + 3 words copied back
    "LIST_RESERVED": 100, "LIST_TAKEN": 101, "FLUSH_QUEUE_NEED": 102, "COPIED": 103,
}

# words of the binned ranges (RMK_CN_*): the loop bounds of the report
EXTENTS = {"PHASES": 6, "GEN_LEVELS": 32, "LOG2_BINS": 32, "LEVEL_BINS": 16, "EMIT_BINS": 16, "DRAIN_LAPS": 4}


def header():
    with open(os.path.join(H, "rm_diag.h")) as f:
        return f.read()


def test_dbg_bits_header_python_and_design_agree():
    bits = {m.group(1): int(m.group(2)) for m in re.finditer(r"^\s*RMK_DBG_(\w+)\s*=\s*(\d+)", header(), re.M)}
    assert bits == DBG
    assert len(set(bits.values())) == len(bits) == 27
    assert all(v > 0 and v & (v - 1) == 0 for v in bits.values())
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        text = f.read()
    table = text[text.index("### Launch-shape and diagnostic switches"):]
    rows = [line for line in table[:table.index("\n\n")].splitlines() if line.startswith("| `RNAMOTIF_DBG` bits")]
    assert len(rows) == 3
    listed = {m.group(2): int(m.group(1)) for row in rows for m in re.finditer(r"(\d+) `(\w+)` ", row.split("|")[3])}
    assert listed == bits


def test_counter_slots_are_the_pinned_ones():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + H, "-o", BIN,
                    "-DSLOTS=" + " ".join(["SLOT( %s )" % n for n in SLOTS] + ["EXTENT( %s )" % n for n in EXTENTS]),
                    os.path.join(ROOT, "tests", "hostsim", "diag_slots.cpp")], check=True)
    out = subprocess.run([BIN], stdout=subprocess.PIPE, check=True).stdout.decode().split()
    got = dict(zip(out[0::2], map(int, out[1::2])))
    assert got.pop("N_COUNTERS") == 128 and got.pop("GCTL") == 100
    assert got == dict(SLOTS, **{"N_" + n: v for n, v in EXTENTS.items()})
    assert set(re.findall(r"^\s*RMK_C_(\w+)\s*=", header(), re.M)) == set(SLOTS)
    assert set(re.findall(r"^\s*RMK_CN_(\w+)\s*=", header(), re.M)) == set(EXTENTS)


def test_no_decimal_literals_next_to_dbg_or_ticket():
    bad = []
    for name in sorted(os.listdir(H)):
        if name.endswith((".h", ".cpp", ".hip")):
            with open(os.path.join(H, name)) as f:
                for n, line in enumerate(f, 1):
                    if re.search(r"dbg\s*&\s*\(?\s*\d", line) or re.search(r"ticket\s*\+\s*\(?\s*\d", line):
                        bad.append("%s:%d: %s" % (name, n, line.strip()))
    assert not bad, "\n".join(bad)
