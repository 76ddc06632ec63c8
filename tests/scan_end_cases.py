"""The cases of tests/test_scan_end_gpu.py, shared with the CPU test that proves their premises (tests/test_scan_end_cpu.py):
what runs behind the search kernel -- search_finish() and scan_end() of rm_scanner.cpp, DevHitSort::run() of
rm_hitsort_dev.hip, the stride loop of efn_body (rm_scan_kernel.h) -- at the sizes where it takes another branch.

Descriptors (the flags are rmd_program_t's, printed by tests/hostsim/order_plan_check.cpp and held in FLAGS below):

  * SS4_ONE, SS4_BOTH -- ss(len=4) on one strand and on both: L - 3 candidates an entry of L bases (2 ( L - 3 )), none for
    an entry shorter than 4 bases: a count known by construction, for the edge of the hit buffer (HIT_CAP);
  * PK -- a pseudoknot (general instance) over random sequence, about four records a base;
  * DENSE -- h5(len=4) around three ss(1..12) on random sequence, lean, window short enough for the pooled instance and
    with it the search kernel that walks nothing (option flush);
  * HAIRPIN_EFN2 (tests/data/hairpin.efn2.descr) and HAIRPIN_EFN, the same with efn(): about 0.36 records a base of random sequence;
  * SS6 -- h5(len=3) around six ss(1..21): lean, ord_ok 1, order words of 22 bits (21^5 walks), window 132 (8 bits of rank);
  * SMALL -- h5(len=3) around three ss(1..6): ord_bits 6, window 24;
  * DEEP -- h5(len=3) around a stem-loop of 3 .. 6 pairs (the head helix), a stem-loop of five pairs (a leaf of the look-ahead chain:
    pass A' tests head and leaf together and leaves its items the head's ends as masks, so the drain kernel's list gets them in
    pieces, rm_scan_kernel.h pool_sub_count) and eleven ss(1..8): lean, ord_ok 0 (the weight, 7 ends x 4 lengths x 8^10, exceeds
    2^31): order words are counts of a walk, or of a piece;
  * ONE -- h5(len=3) around ss(1..5), a stem-loop with a loop of 3 .. 7 and ss(len=2): lean, ord_ok 1; at its site the walk tries
    five bases for the first single strand, the match has one, so the kernels leave an order word that is not 0;
  * PK_ONE -- PK with single strands of different ranges, so that a site matches on one strand only.

Poly-a databases: a pairs with nothing under wc, so a helix forms only where g...c is planted, and the single strands
between the planted strands take every composition of the a's between them: C( D - 1, k - 1 ) records for k strands over D bases
less those with a part beyond its maxlen."""
import os
from math import comb

import numpy as np

HIT_CAP = 1 << 17           # records of a fresh scanner's hit buffer (rnamotif_amd/csrc/rm_scanner.cpp:249)
W_ORD = 20                  # bits of the order word in the ordering's key until a scan outgrows them (DevHitSort::w_ord, rm_hitsort_dev.h:23)
PIECE_ORDER_BITS = 12       # candidates a piece of an item may find (rnamotif_amd/csrc/rm_kernels.h:92)
EFN_BLOCK = 256             # candidates a workgroup of the staged energy kernel takes a pass, one workgroup a CU (launch_efn)
EFN_LIGHT_PER_CU = 1024     # ... and the light kernel's: 16 waves of 64 a CU

SS4_ONE = "parms\n\tchk_both_strs = 0;\ndescr\n\tss(minlen=4,maxlen=4)\n"
SS4_BOTH = "descr\n\tss(minlen=4,maxlen=4)\n"
PK = ("descr\n\th5(tag='1',len=2)\n\tss(minlen=1,maxlen=8)\n\th5(tag='2',len=2)\n\tss(minlen=1,maxlen=8)\n\th3(tag='1')\n"
      "\tss(minlen=1,maxlen=8)\n\th3(tag='2')\n")
PK_ONE = PK.replace("ss(minlen=1,maxlen=8)\n\th5(tag='2'", "ss(minlen=1,maxlen=2)\n\th5(tag='2'").replace(
    "ss(minlen=1,maxlen=8)\n\th3(tag='2')", "ss(minlen=3,maxlen=8)\n\th3(tag='2')")
DENSE = "descr\n\th5(len=4)\n\t\tss(minlen=1,maxlen=12)\n\t\tss(minlen=1,maxlen=12)\n\t\tss(minlen=1,maxlen=12)\n\th3\n"
HAIRPIN_EFN2 = ("parms\n\twc += gu;\ndescr\n\th5( minlen=4, maxlen=6 )\n\t\tss( minlen=3, maxlen=8 )\n\th3\n"
                "score\n\t{ SCORE = efn2( h5[1], h3[3] ); }\n")
HAIRPIN_EFN = HAIRPIN_EFN2.replace("efn2(", "efn(")
SS6_MAXLEN = 21
SS6 = "descr\n\th5(len=3)\n" + "\t\tss(minlen=1,maxlen=%d)\n" % SS6_MAXLEN * 6 + "\th3\n"
ONE = "descr\n\th5(len=3)\n\t\tss(minlen=1,maxlen=5)\n\t\th5(len=3)\n\t\t\tss(minlen=3,maxlen=7)\n\t\th3\n\t\tss(len=2)\n\th3\n"
SMALL = "descr\n\th5(len=3)\n" + "\t\tss(minlen=1,maxlen=6)\n" * 3 + "\th3\n"
DEEP = ("descr\n\th5(len=3)\n\t\th5(minlen=3,maxlen=6)\n\t\t\tss(len=3)\n\t\th3\n\t\th5(len=5)\n\t\t\tss(len=4)\n\t\th3\n" +
        "\t\tss(minlen=1,maxlen=8)\n" * 11 + "\th3\n")
WRITTEN = {"ss4_one.descr": SS4_ONE, "ss4_both.descr": SS4_BOTH, "pk.descr": PK, "pk_one.descr": PK_ONE, "dense.descr": DENSE,
           "hairpin_efn2.descr": HAIRPIN_EFN2, "hairpin_efn.descr": HAIRPIN_EFN, "ss6.descr": SS6, "one.descr": ONE, "small.descr": SMALL, "deep.descr": DEEP}

# name -> (lean_ok, ord_ok, ord_bits or a range of them, w_winsize, n_efn, efn_big): what the cases need of the device program
FLAGS = {
    "ss4_one.descr": (1, 1, 0, 4, 0, 0), "ss4_both.descr": (1, 1, 0, 4, 0, 0),
    "pk.descr": (0, 0, 0, 32, 0, 0), "pk_one.descr": (0, 0, 0, 26, 0, 0),
    "dense.descr": (1, 1, range(0, W_ORD + 1), 44, 0, 0),
    "hairpin_efn2.descr": (1, 1, range(0, W_ORD + 1), 20, 1, 0), "hairpin_efn.descr": (1, 1, range(0, W_ORD + 1), 20, 1, 0),
    "ss6.descr": (1, 1, range(W_ORD + 1, 32), 132, 0, 0),       # case 4: more bits than the key's field has at first
    "one.descr": (1, 1, range(1, W_ORD + 1), 26, 0, 0),
    "small.descr": (1, 1, range(0, 17), 24, 0, 0),              # case 5: fits the bits the clamped field has left
    "deep.descr": (1, 0, 0, 123, 0, 0),
}


def write_all(directory):
    """the descriptors as files of directory; name -> path"""
    paths = {}
    for name, text in WRITTEN.items():
        paths[name] = os.path.join(str(directory), name)
        with open(paths[name], "w") as f:
            f.write(text)
    return paths


def random_bases(seed, n):
    lut = np.frombuffer(b"acgt", dtype=np.uint8)
    return lut[np.random.default_rng(seed).integers(0, 4, size=n)].tobytes()


# ---------------------------------------------------------------- case 1: the edge of the hit buffer
def ss4_entries(count, seed=1):
    """Entries of random sequence with count windows of four bases in all (sum of L - 3), some of them shorter than four bases"""
    lens = [2, 60_001, 3, 1, 4, 30_011, 0, 7]
    have = sum(max(n - 3, 0) for n in lens)
    if have > count:                      # (the small databases: one entry takes them all)
        lens = [2, count + 3, 3, 1] if count > 0 else [3, 2, 1]
        have = count
    while count - have > 0:
        n = min(count - have, 150_001)
        lens.append(n + 3)
        have += n
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"acgt", dtype=np.uint8)
    return [lut[rng.integers(0, 4, size=n)].tobytes() for n in lens]


def ss4_count(seqs, strands=1):
    return strands * sum(max(len(s) - 3, 0) for s in seqs)


# the scans of case 1: (count, launches of the search kernel; None: one at most, there may be no start position to launch for) --
# each on a fresh scanner, then in this order on the last of them, the one that grew
SS4_FRESH = ((HIT_CAP - 1, 1), (HIT_CAP, 1), (HIT_CAP + 1, 2))
SS4_GROWN = ((3 * HIT_CAP + 5, 2), (HIT_CAP + 1, 1), (3, 1), (1, 1), (0, None))
SS4_BOTH_WINDOWS = HIT_CAP // 2 + 1         # 2^17 + 2 records on both strands


# ---------------------------------------------------------------- case 2: regrow on a general instance, two repeat reasons
def pk_entries():
    """random sequence for PK: the oracle finds 2^17 .. 2^18 records (tests/test_scan_end_cpu.py)"""
    return [random_bases(202, n) for n in (30_001, 5, 13_003, 61, 4_999)]


def dense_entries():
    """random sequence for DENSE: 2^17 .. 2^18 records"""
    return [random_bases(203, n) for n in (9_001, 33, 4_003)]


# ---------------------------------------------------------------- case 3: energies beyond one grid pass
EFN_CUS = 256               # the device the database is sized for


def hairpin_entries():
    """a megabase of random sequence: more than 1.25 x 256 x 1024 records of the hairpin descriptors"""
    return [random_bases(204, n) for n in (400_003, 61, 350_001, 7, 299_999)]


def efn_need(cus, light):
    """records beyond which the energy kernel's lanes take a second candidate, and a quarter more"""
    return int(1.25 * cus * (EFN_LIGHT_PER_CU if light else EFN_BLOCK))


# ---------------------------------------------------------------- cases 4, 5, 7: planted sites in poly-a
def ss_site(d, before=40, after=40):
    """ggg, d times a, ccc in poly-a: a descriptor of k single strands in h5(len=3) finds the compositions of d into k parts
    within their lengths, on either strand"""
    return b"a" * before + b"ggg" + b"a" * d + b"ccc" + b"a" * after


def ss6_entries():
    """Sites of 6 (a single record a strand), 17 and 20 a's: compositions of 20 into six parts have first parts of 1 .. 15,
    the walk tries 15 first, so order words reach 14 x 21^4 > 2^20 (walk_number)"""
    return [ss_site(6), b"a" * 300 + ss_site(17)[40:], b"aa", ss_site(20, 7, 300)]


def compositions(d, k, maxlen):
    """compositions of d into k parts of 1 .. maxlen (inclusion and exclusion over the parts that are too long)"""
    return sum((-1) ** j * comb(k, j) * comb(d - j * maxlen - 1, k - 1) for j in range(k + 1) if d - j * maxlen >= k)


def walk_number(parts, maxlen, minlen=1):
    """The order word the lean kernels leave for the candidate of single strands of the lengths parts in h5(len=3), before the
    ordering renumbers it (wave_emit_body, rm_scan_kernel.h:142): per level but the last ( first end tried - end taken ) x the
    level's weight, the first end tried being the longest the level's maxlen and the levels behind it allow (rmd_lean_open)."""
    k = len(parts)
    left = sum(parts)
    word = 0
    for i, n in enumerate(parts[:-1]):
        first = min(maxlen, left - minlen * (k - 1 - i))
        word += (first - n) * (maxlen - minlen + 1) ** (k - 2 - i)
        left -= n
    return word


CLAMP_SHORT = (1 << 16) + 1
CLAMP_LONG = (1 << 21) + 999


def clamp_entries():
    """case 5: 2^16 + 1 entries of one base, then poly-a of 2^21 + 999 bases with sites of 20 a's (SS6) and of 10 (SMALL, SS6) at
    its start, in its middle and at its end"""
    long = bytearray(b"a" * CLAMP_LONG)
    for d, first in ((20, 3), (10, 500)):        # (the two kinds half a kilobase apart: no window holds strands of both)
        site = b"ggg" + b"a" * d + b"ccc"
        for at in (first, (1 << 20) + 17 + first, len(long) - len(site) - first):
            long[at:at + len(site)] = site
    return [b"acgt"[i % 4:i % 4 + 1] for i in range(CLAMP_SHORT)] + [bytes(long)]


def bits_of(x):
    return int(x).bit_length()      # (rma::bits_of)


def key_bits(seqs, w_winsize):
    """(entry, strand, position, rank) bits of the ordering's key as scan_end() asks for them: of the last entry's number, the
    longest entry and the window"""
    return bits_of(len(seqs) - 1), 1, bits_of(max(len(s) for s in seqs)), bits_of(w_winsize)


# ---------------------------------------------------------------- case 6: a piece of an item beyond 2^12 candidates
DEEP_PARTS, DEEP_MAXLEN = 11, 8


def deep_site(d, before=50, after=50):
    """ggg, the head stem-loop ccc aaa ggg, the leaf gcgcg aaaa cgcgc, d times a, ccc: DEEP finds the compositions of d into eleven
    parts of 1 .. 8, all from one start position and one end of the head helix, that is from one piece of one item"""
    return b"a" * before + b"ggg" + b"cccaaaggg" + b"gcgcgaaaacgcgc" + b"a" * d + b"ccc" + b"a" * after


DEEP_DENSE_D = 19           # 43 747 records


def deep_dense_entries():
    return [b"a" * 700, deep_site(DEEP_DENSE_D, 1000, 2000)]


DEEP_SPARSE_D = (12, 11, 13)


def deep_sparse_entries():
    """11 + 1 + 66 records"""
    return [deep_site(12), deep_site(11, 3, 9), deep_site(13)]


# ---------------------------------------------------------------- case 7: a single record on each instance
# ONE's site: the interior has 16 bases, the levels behind the first single strand need 11 of them, so the walk tries min( 5, 16 - 11 )
# for it first and finds the stem-loop only behind 1: ( 5 - 1 ) x the level's weight is the word the kernels leave
ONE_SITE = b"a" * 30 + b"ggg" + b"a" + b"ccc" + b"aaaaaaa" + b"ggg" + b"aa" + b"ccc" + b"a" * 30
ONE_FIRST, ONE_TAKEN = 5, 1


def single_cases():
    """(descriptor, entries): one site, one record"""
    return [("one.descr", [b"aaa", ONE_SITE]),
            ("deep.descr", [deep_site(11)]),
            ("pk_one.descr", [b"a" * 30 + b"gg" + b"a" + b"cc" + b"a" + b"cc" + b"aaa" + b"gg" + b"a" * 30])]
