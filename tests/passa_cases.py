"""The cases of tests/test_passa_quads_gpu.py, shared with the CPU test of the same rules (tests/test_passa_cpu.py).

Descriptors: trna.descr; two_leaves.descr and wide_loop.descr of tests/flush_cases.py; and five written here, each a chain
with leaves (helices of four pairs and more under wc + gu, tests/flush_cases.py):

  * TAIL_2X2 -- the tail stem-loop has two helix lengths and two loop lengths and ss(minlen=1,maxlen=3) behind it: the
    end window spans every term of its range;
  * TAIL_NO_LEAF -- the interior ends with h5(len=3) around ss(minlen=4,maxlen=11), which is no leaf: no end window;
  * HEAD_RANGE -- one to three bases of single strand in front of the first interior helix: pass A' tries the head
    helix at each offset and wants no masks;
  * OUTER_ONE, OUTER_FOUR -- an outer helix of one length and of four: one round of a quad half used, two rounds.

Databases: those of tests/flush_cases.py."""
import flush_cases as FC

_HEAD = "parms\n\twc += gu;\ndescr\n"
TAIL_2X2 = _HEAD + """	h5(minlen=4,maxlen=5)
		ss(len=2)
		h5(len=4)
			ss(minlen=4,maxlen=6)
		h3
		ss(minlen=1,maxlen=3)
		h5(minlen=4,maxlen=5)
			ss(minlen=4,maxlen=5)
		h3
		ss(minlen=1,maxlen=3)
	h3
"""
TAIL_NO_LEAF = _HEAD + """	h5(minlen=4,maxlen=5)
		ss(len=2)
		h5(len=4)
			ss(minlen=3,maxlen=5)
		h3
		ss(minlen=1,maxlen=3)
		h5(len=3)
			ss(minlen=4,maxlen=11)
		h3
	h3
"""
HEAD_RANGE = _HEAD + """	h5(minlen=4,maxlen=5)
		ss(minlen=1,maxlen=3)
		h5(len=4)
			ss(minlen=4,maxlen=6)
		h3
		ss(len=2)
		h5(len=4)
			ss(minlen=3,maxlen=5)
		h3
	h3
"""
OUTER_ONE = _HEAD + """	h5(len=4)
		ss(len=2)
		h5(len=4)
			ss(minlen=4,maxlen=6)
		h3
		ss(len=1)
		h5(len=4)
			ss(minlen=4,maxlen=5)
		h3
	h3
"""
OUTER_FOUR = OUTER_ONE.replace("\th5(len=4)\n\t\tss(len=2)", "\th5(minlen=4,maxlen=7)\n\t\tss(len=2)")
WRITTEN = dict(FC.WRITTEN, **{"tail_2x2.descr": TAIL_2X2, "tail_no_leaf.descr": TAIL_NO_LEAF, "head_range.descr": HEAD_RANGE,
                              "outer_one.descr": OUTER_ONE, "outer_four.descr": OUTER_FOUR})
NAMES = ["trna.descr", "two_leaves.descr", "wide_loop.descr", "tail_2x2.descr", "tail_no_leaf.descr", "head_range.descr",
         "outer_one.descr", "outer_four.descr"]
# RNAMOTIF_SHORT (tiles per entry; tiles over the concatenation: the second flush instance) x RNAMOTIF_TILE
SHORT = ("0", "2")
TILE = ("512", None)
databases = FC.databases
