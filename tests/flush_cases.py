"""The cases of tests/test_flush_vectors_gpu.py, shared with the CPU test that proves them (tests/test_flush_vectors_cases.py).

Descriptors: trna.descr; bulge.descr; WIDE_LOOP -- two leaves of the look-ahead chain with a single strand of 4 .. 70
bases between them, so that the chain has a group whose range of lengths is wider than a word, behind a leaf whose
helix has two lengths (tmax 1) --; TWO_LEAVES -- two stem-loops of different shape, both leaves: two core slots.
(A stem-loop is a leaf of the chain when helix lengths x loop lengths x p_pair ^ minlen <= 0.25, rm_dev_program.cpp:
helices of four pairs and more under wc + gu.)

Databases: entries of 95, 96, 97, 127, 128 and 129 bases -- the vectors end within a dword of where a read of 96 bits
must stop --, and three entries of 20 000 bases with runs of n that begin on multiples of 512 next to one of 50 000."""
import numpy as np

WIDE_LOOP = """parms
	wc += gu;
descr
	h5(minlen=4,maxlen=5)
		ss(len=2)
		h5(len=4)
			ss(minlen=4,maxlen=5)
		h3
		ss(minlen=4,maxlen=70)
		h5(minlen=4,maxlen=5)
			ss(len=5)
		h3
	h3
"""
TWO_LEAVES = """parms
	wc += gu;
descr
	h5(minlen=4,maxlen=6)
		ss(len=2)
		h5(len=4)
			ss(minlen=4,maxlen=6)
		h3
		ss(minlen=1,maxlen=3)
		h5(len=5)
			ss(minlen=3,maxlen=5)
		h3
		ss(len=1)
	h3
"""
WRITTEN = {"wide_loop.descr": WIDE_LOOP, "two_leaves.descr": TWO_LEAVES}
NAMES = ["trna.descr", "bulge.descr", "wide_loop.descr", "two_leaves.descr"]
# RNAMOTIF_SHORT (tiles per entry; groups of small tiles, where option flush does not apply; tiles over the concatenation: the
# second flush instance, where the layout takes it -- tests/test_flush_vectors_cases.py) x RNAMOTIF_TILE (512 and 2048 start
# positions, the default)
SHORT = ("0", "1", "2")
TILE = ("512", "2048", None)


def databases():
    rng = np.random.default_rng(20251)
    lut = np.frombuffer(b"acgt", dtype=np.uint8)
    short = [lut[rng.integers(0, 4, size=n)].tobytes() for n in (95, 96, 97, 127, 128, 129)]
    long = []
    for k in range(3):
        a = lut[rng.integers(0, 4, size=20_000)].copy()
        for i, at in enumerate(range(512 * (k + 1), 20_000, 512 * 3)):
            a[at:at + (1, 3, 33, 70)[i % 4]] = ord("n")
        long.append(a.tobytes())
    long.append(lut[rng.integers(0, 4, size=50_000)].tobytes())
    return {"short": short, "long": long}
