"""Nested structures as descriptors, and the four families of structures the energy tests run.

Any nested structure is the single candidate of a descriptor of fixed lengths over its own sequence: each maximal
stack becomes h5(tag,len=k) ... h3(tag), each unpaired run ss(len=m), with `wc += gu` and efn2() / efn() over the
first to the last element.  That hands the energy kernels (rm_efn_core.h, rm_efn2_core.h inside the energy kernel of
rm_scan_kernel.h), their host build (tests/hostsim) and the oracle the structures the reference's own drivers
(oracle/_ref/efn_drv, efn2_drv) are run on; what the drivers print is pinned in tests/golden/ref_pins.json
(tests/ref_pins.py).

Families: `efn_random` and `efn2_closed` are the structures of tests/test_efn_oracle.py and tests/test_efn2_oracle.py
(same generators, same seeds, same pins); `directed` has one structure or more for every line of the two cores that
those 696 leave unreached, each with a predicate that says the feature is there; `large` has 16 to 30 helices under
100 elements, for the energy kernel's instance with the large stacks (rmd_program_t::efn_big).

A plain module: tests/test_efn_structures_cpu.py and tests/test_efn_structures.py import it."""
import os
import re
import subprocess
import tempfile

import numpy as np

from ref_pins import md5, pinned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EFNDATA = os.path.join(ROOT, "rnamotif_amd", "efndata")
EFN_DRV = os.path.join(ROOT, "oracle", "_ref", "efn_drv")
EFN2_DRV = os.path.join(ROOT, "oracle", "_ref", "efn2_drv")
EFN2_UNDEFINED = 9999999                 # RMA_EFN2_INFINITY


# ---------------------------------------------------------------- structure -> descriptor
def partners(seq, pairs):
    bp = [-1] * len(seq)
    for i, j in pairs:
        assert 0 <= i < j < len(seq) and bp[i] == -1 and bp[j] == -1, (i, j)
        bp[i], bp[j] = j, i
    return bp


def elements_of(seq, pairs):
    """[(type, helix number or None, first base, length)] in 5' to 3' order.  A pair (i, j) continues the previous
    helix only if (i-1, j+1) is a pair, so a 3' run that spans two helices is cut in two."""
    bp = partners(seq, pairs)
    helix = [None] * len(seq)
    n = 0
    for i, j in enumerate(bp):
        if j > i:
            if i > 0 and bp[i - 1] == j + 1:
                helix[i] = helix[i - 1]
            else:
                helix[i] = n
                n += 1
            helix[j] = helix[i]
    elems = []
    for i, j in enumerate(bp):
        key = ("ss", None) if j < 0 else ("h5" if j > i else "h3", helix[i])
        if elems and (elems[-1][0], elems[-1][1]) == key:
            elems[-1][3] += 1
        else:
            elems.append([key[0], key[1], i, 1])
    return [tuple(e) for e in elems]


def descriptor_of(seq, pairs):
    """Descriptor text whose only candidate over `seq` is the structure `pairs` (0-based (i, j), nested);
    score: '%8.3f %8.3f' of efn2() and efn() from the first to the last element (energy sites 0 and 1)."""
    elems = elements_of(seq, pairs)
    lines = ["parms", "\twc += gu;", "descr"]
    for t, h, _, ln in elems:
        if t == "ss":
            lines.append("\tss(len=%d)" % ln)
        elif t == "h5":
            lines.append("\th5(tag='h%d',len=%d)" % (h, ln))
        else:
            lines.append("\th3(tag='h%d')" % h)
    first, last = "%s[1]" % elems[0][0], "%s[%d]" % (elems[-1][0], len(elems))
    lines += ["score", "\t{ SCORE = sprintf( '%%8.3f %%8.3f', efn2( %s, %s ), efn( %s, %s ) ); }" % (first, last, first, last)]
    return "\n".join(lines) + "\n"


def ct_text(seq, pairs):
    """the structure as the drivers read it (the .ct text of the two oracle tests)"""
    from test_efn_oracle import _ct
    return _ct(seq, pairs)


def loops_of(seq, pairs):
    """The loops of a nested structure: ("hairpin", i, j, size), ("bulge" | "interior", i, j, size1, size2),
    ("multi", i, j, branches inside, unpaired) for every pair (i, j) that closes one, and ("exterior", [(i, j), ...])."""
    bp = partners(seq, pairs)

    def branches(lo, hi):
        out, k = [], lo
        while k <= hi:
            if bp[k] > k:
                out.append((k, bp[k]))
                k = bp[k] + 1
            else:
                k += 1
        return out

    loops = [("exterior", branches(0, len(seq) - 1))]
    for i, j in sorted(pairs):
        br = branches(i + 1, j - 1)
        if not br:
            loops.append(("hairpin", i, j, j - i - 1))
        elif len(br) == 1:
            s1, s2 = br[0][0] - i - 1, j - br[0][1] - 1
            if s1 + s2:
                loops.append(("bulge" if 0 in (s1, s2) else "interior", i, j, s1, s2))
        else:
            loops.append(("multi", i, j, len(br), j - i - 1 - sum(q - p + 1 for p, q in br)))
    return loops


def efn2_defined(seq, pairs):
    """Whether RM_efn2 stays inside its arrays (efn2.c:1313-1345).  A structure closed by its first and last base
    always does.  Otherwise the exterior walk looks for the first helix from base 1 on and for the next right
    behind the last; its test for an unpaired base, rm_basepr[ip] == 0, skips only a base paired with base 0, so
    the structure is defined only if every such search lands on a paired base at once or after that one base."""
    bp = partners(seq, pairs)
    n = len(seq)
    if bp[0] == n - 1:
        return True
    i, helices = 0, 0
    while i < n - 1:
        if bp[i] != -1:
            helices += 1
            i = bp[i]
        i += 1
    p = 1
    for _ in range(helices):
        while p < n and bp[p] == 0:
            p += 1
        if p >= n or bp[p] < p:
            return False
        p = bp[p] + 1
    return True


# ---------------------------------------------------------------- the two existing families
def efn_random():
    """the 296 structures of test_efn_oracle.py::test_against_reference_efn_drv"""
    from test_efn_oracle import _random_structure
    rng = np.random.default_rng(5)
    return [c for c in (_random_structure(rng, int(rng.integers(12, 120))) for t in range(300)) if c[1]]


def efn2_closed():
    """the 400 structures of test_efn2_oracle.py::test_random_closed_structures_match_efn2_drv"""
    from test_efn2_oracle import _closed_structure
    rng = np.random.default_rng(20240602)
    return [_closed_structure(rng, int(rng.integers(9, 120))) for _ in range(400)]


# ---------------------------------------------------------------- building blocks
_COMP = {"a": "u", "c": "g", "g": "c", "u": "a"}


def _rc(s):
    return "".join(_COMP[c] for c in reversed(s))


def _rnd(rng, n, letters="acgu"):
    return "".join(letters[int(x)] for x in rng.integers(0, len(letters), size=n))


def _pairs_of(dots):
    stack, pairs = [], []
    for i, c in enumerate(dots):
        if c == "(":
            stack.append(i)
        elif c == ")":
            pairs.append((stack.pop(), i))
    assert not stack
    return sorted(pairs)


def _hp(stem, loop, stem3=None):
    """(sequence, dot-bracket) of a hairpin; stem3: the 3' strand where it is not the plain complement (g-u pairs)"""
    stem3 = _rc(stem) if stem3 is None else stem3
    assert len(stem3) == len(stem)
    return stem + loop + stem3, "(" * len(stem) + "." * len(loop) + ")" * len(stem)


def _wrap(stem, left, inner, right, stem3=None):
    """a helix around `inner` with `left` / `right` unpaired between"""
    stem3 = _rc(stem) if stem3 is None else stem3
    return (stem + left + inner[0] + right + stem3,
            "(" * len(stem) + "." * len(left) + inner[1] + "." * len(right) + ")" * len(stem))


def _cat(*parts):
    """structures and plain strings (unpaired) side by side"""
    seq, dots = "", ""
    for p in parts:
        if isinstance(p, str):
            seq, dots = seq + p, dots + "." * len(p)
        else:
            seq, dots = seq + p[0], dots + p[1]
    return seq, dots


def _has(kind, *sizes):
    return lambda seq, pairs: any(l[0] == kind and tuple(l[3:]) == sizes for l in loops_of(seq, pairs))


def _table_keys(name):
    """the loops of efndata/tloop.dat or triloop.dat, closing pair included, in lower case"""
    with open(os.path.join(EFNDATA, name)) as f:
        return [m.group(1).lower() for m in (re.match(r"\s*([ACGU]+)\s+-?[0-9.]+", l) for l in f.readlines()[2:]) if m]


def _hairpin_in(name):
    def pred(seq, pairs):
        keys = set(_table_keys(name))
        return any(l[0] == "hairpin" and seq[l[1]:l[2] + 1] in keys for l in loops_of(seq, pairs))
    return pred


def _efn_polyc(size):
    """ef_hploop starts its scan for an all-C loop at base i + i (efn.c:1511): it can count `size` C only for a
    hairpin closed from base 0 or 1"""
    def pred(seq, pairs):
        for l in loops_of(seq, pairs):
            if l[0] == "hairpin" and l[3] == size:
                i, j, c = l[1], l[2], 0
                for k in range(i + i, j):
                    if seq[k] != "c":
                        break
                    c += 1
                if c == size:
                    return True
        return False
    return pred


def _all_c(size):
    return lambda seq, pairs: any(l[0] == "hairpin" and l[3] == size and set(seq[l[1] + 1:l[2]]) == {"c"} for l in loops_of(seq, pairs))


def _gu_after_gg(seq, pairs):
    return any(l[0] == "hairpin" and l[1] > 1 and seq[l[1] - 2:l[1] + 1] == "ggg" and seq[l[2]] == "u" for l in loops_of(seq, pairs))


def _n_in_loop(seq, pairs):
    bp = partners(seq, pairs)
    return any(c == "n" and bp[i] < 0 for i, c in enumerate(seq))


def _n_next_to_pair(seq, pairs):
    bp = partners(seq, pairs)
    return any(c == "n" and bp[i] < 0 and any(0 <= k < len(seq) and bp[k] >= 0 for k in (i - 1, i + 1)) for i, c in enumerate(seq))


def _exterior(first, gaps, tail=None):
    """exterior helices: the first starts at base `first`, the others `gaps` bases behind their neighbours, and
    `tail` bases (None: any number) follow the last"""
    def pred(seq, pairs):
        br = loops_of(seq, pairs)[0][1]
        return (br[0][0] == first and [b[0] - a[1] - 1 for a, b in zip(br, br[1:])] == list(gaps) and
                (tail is None or len(seq) - 1 - br[-1][1] == tail))
    return pred


# ---------------------------------------------------------------- directed
def directed():
    """[(name, seq, pairs, predicate)]: what the 696 random structures leave unreached in rm_efn_core.h and
    rm_efn2_core.h (a gcov build of tests/hostsim/hostsim_check.cpp over them tells), one structure or more each."""
    rng = np.random.default_rng(20251018)
    inner = _hp("gcac", "gaaa")
    out = []

    def add(name, s, pred):
        seq, dots = s
        pairs = _pairs_of(dots)
        assert pred(seq, pairs), name
        out.append((name, seq, pairs, pred))

    # loops beyond the tables' 30 entries: the logarithm tables (rme_loginc: rounded; rme2_loginc: truncated)
    for n in (31, 32, 60, 150):
        add("hairpin of %d" % n, _cat("a", _hp("ggcac", _rnd(rng, n)), "a"), _has("hairpin", n))
        add("bulge of %d, 5' side" % n, _cat("a", _wrap("gcuc", _rnd(rng, n), inner, ""), "a"), _has("bulge", n, 0))
        add("bulge of %d, 3' side" % n, _wrap("gguc", "", inner, _rnd(rng, n)), _has("bulge", 0, n))
    for a, b in ((1, 30), (30, 1), (10, 21), (16, 16), (2, 30), (30, 30), (20, 40), (75, 75), (1, 149), (100, 50), (149, 2)):
        add("interior loop of %d + %d" % (a, b), _cat("a", _wrap("gcuc", _rnd(rng, a), inner, _rnd(rng, b)), "a"), _has("interior", a, b))
    # special hairpins
    for key in _table_keys("tloop.dat")[:2] + _table_keys("tloop.dat")[-1:]:
        add("tetraloop %s" % key, _cat("a", _hp("cac" + key[0], key[1:5], key[5] + "gug"), "a"), _hairpin_in("tloop.dat"))
    add("all-C hairpin of 3", _cat("a", _hp("gcag", "ccc"), "a"), _all_c(3))
    add("all-C hairpin of 6", _cat("a", _hp("gcag", "cccccc"), "a"), _all_c(6))
    add("all-C hairpin of 3 closed from base 1", _cat("a", _hp("g", "ccc"), "a"), _efn_polyc(3))
    add("all-C hairpin of 5 closed from base 1", _cat("a", _hp("g", "ccccc"), "a"), _efn_polyc(5))
    add("hairpin of 3 closed from base 0, c c c a g", _hp("c", "cca"), _efn_polyc(3))
    add("hairpin of 4 closed from base 0, c c c c a g", _cat(_hp("c", "ccca"), "a"), _efn_polyc(4))
    add("G-U closure behind two G, hairpin of 4", _cat("a", _hp("cggg", "gaaa", "uccg"), "a"), _gu_after_gg)
    add("G-U closure behind two G, hairpin of 3", _hp("cggg", "aaa", "uccg"), _gu_after_gg)
    add("G-U closure behind two G, hairpin of 40", _cat("a", _hp("cggg", _rnd(rng, 40), "uccg")), _gu_after_gg)
    add("hairpin of 1", _cat("a", _hp("ggc", "a"), "a"), _has("hairpin", 1))
    add("hairpin of 2", _cat("a", _hp("ggc", "ua"), "a"), _has("hairpin", 2))
    add("hairpin of 2, closed", _hp("gc", "cc"), _has("hairpin", 2))
    add("N inside a hairpin", _cat("a", _hp("ggc", "ganaa"), "a"), _n_in_loop)
    add("N next to the closing pairs of a hairpin of 4", _cat("a", _hp("ggc", "naan"), "a"), _n_next_to_pair)
    add("N next to the closing pairs of a hairpin of 3", _hp("ggc", "nan"), _n_next_to_pair)
    add("N in an interior loop of 1 + 1", _wrap("ggc", "n", inner, "a"), _n_next_to_pair)
    add("N in an interior loop of 2 + 2", _wrap("ggc", "na", inner, "an"), _n_next_to_pair)
    add("N in an interior loop of 1 + 2", _wrap("ggc", "n", inner, "na"), _n_next_to_pair)
    add("N in a bulge", _wrap("ggc", "n", inner, ""), _n_next_to_pair)
    add("N dangling on an exterior helix", _cat("n", _hp("ggc", "gaaa"), "n"), _n_next_to_pair)
    add("N in a multi-branch loop", _wrap("ggc", "n", _cat(inner, "n", _hp("cgu", "uuuu")), "n"), _n_next_to_pair)
    # 1 + 2 and 2 + 1 interior loops between u-g and g-u pairs in every position (asint1x2's rows 4 and 5)
    for a, b in ((1, 2), (2, 1)):
        for o5, o3, i5, i3 in (("u", "g", "g", "c"), ("g", "u", "g", "c"), ("c", "g", "u", "g"), ("c", "g", "g", "u"), ("u", "g", "g", "u")):
            add("interior loop of %d + %d between %s-%s and %s-%s" % (a, b, o5, o3, i5, i3),
                _cat("a", _wrap("gc" + o5, _rnd(rng, a), _hp(i5 + "ca", "gaaa", "ug" + i3), _rnd(rng, b), o3 + "gc"), "a"),
                lambda s, p, a=a, b=b, o5=o5, o3=o3, i5=i5, i3=i3: any(
                    l[0] == "interior" and l[3:] == (a, b) and s[l[1]] + s[l[2]] == o5 + o3 and s[l[1] + a + 1] + s[l[2] - b - 1] == i5 + i3
                    for l in loops_of(s, p)))
    # exterior helices against the ends and each other
    h1, h2, h3 = _hp("ggc", "gaaa"), _hp("cug", "uuca"), _hp("gau", "aaaa", "guc")
    add("exterior helix flush with both ends", h1, _exterior(0, [], 0))
    add("exterior helix from base 0, one base behind", _cat(h1, "a"), _exterior(0, [], 1))
    add("exterior helix from base 1 to the last base", _cat("a", h1), _exterior(1, [], 0))
    add("exterior helix from base 2", _cat("ac", h1, "a"), _exterior(2, [], 1))
    add("two exterior helices flush, from base 1", _cat("a", h1, h2, "a"), _exterior(1, [0], 1))
    add("two exterior helices flush, from base 1 to the last base", _cat("u", h2, h1), _exterior(1, [0], 0))
    add("three exterior helices flush, from base 1", _cat("c", h1, h2, h3, "ag"), _exterior(1, [0, 0], 2))
    add("two exterior helices flush, from base 0", _cat(h1, h2, "a"), _exterior(0, [0], 1))
    add("two exterior helices flush, from base 0 to the last base", _cat(h2, h3), _exterior(0, [0], 0))
    add("three exterior helices flush, from base 0", _cat(h3, h1, h2, "u"), _exterior(0, [0, 0], 1))
    add("two exterior helices one base apart, from base 1", _cat("a", h1, "a", h2, "a"), _exterior(1, [1], 1))
    add("two exterior helices one base apart, from base 0", _cat(h1, "u", h2), _exterior(0, [1], 0))
    add("two exterior helices two bases apart", _cat("a", h1, "ca", h2, "c"), _exterior(1, [2], 1))
    # multi-branch loops of more than 6 unpaired bases (mbl_log)
    add("multi-branch loop of 8 unpaired", _wrap("gcgc", "aaa", _cat(h1, "aaa", h2), "aa"), _has("multi", 2, 8))
    add("multi-branch loop of 7 unpaired, one gap", _wrap("gcgc", "", _cat(h1, "acaacaa", h2), ""), _has("multi", 2, 7))
    add("multi-branch loop of 40 unpaired", _wrap("gcgc", _rnd(rng, 12), _cat(h1, _rnd(rng, 13), h2, h3), _rnd(rng, 15)), _has("multi", 3, 40))
    return out


# ---------------------------------------------------------------- large
def _count(seq, pairs):
    el = elements_of(seq, pairs)
    return len(el), sum(1 for e in el if e[0] == "h5")


def large():
    """[(name, seq, pairs, predicate)]: 16 to 30 helices and fewer than 100 elements -- descriptors for which
    rmd_build sets efn_big (a call over more than 15 helices)"""
    rng = np.random.default_rng(20251019)

    def stem(k):
        s = _rnd(rng, k)
        t = "".join(("u" if c == "g" else "g") if c in "gu" and rng.random() < 0.2 else _COMP[c] for c in reversed(s))
        return s, t

    def hairpin():
        s, t = stem(int(rng.integers(2, 5)))
        return _hp(s, _rnd(rng, int(rng.integers(3, 7))), t)

    def chain(n, first):
        return _cat(_rnd(rng, first), *[hairpin() for _ in range(n)], _rnd(rng, int(rng.integers(0, 3))))

    def multi(n, gaps):
        parts = []
        for k in range(n):
            parts += [_rnd(rng, int(rng.integers(0, gaps + 1))), hairpin()]
        s, t = stem(3)
        return _wrap(s, "", _cat(*parts), _rnd(rng, int(rng.integers(0, gaps + 1))), t)

    def nested(n, both):
        cur = hairpin()
        for _ in range(n - 1):
            s, t = stem(int(rng.integers(1, 4)))
            l, r = int(rng.integers(1, 4)), int(rng.integers(1, 4))
            if not both:                              # bulges only: one element a loop
                l, r = (l, 0) if rng.random() < 0.5 else (0, r)
            cur = _wrap(s, _rnd(rng, l), cur, _rnd(rng, r), t)
        return cur

    def tree(depth):
        if depth == 0:
            return hairpin()
        s, t = stem(int(rng.integers(2, 4)))
        return _wrap(s, "", _cat(tree(depth - 1), _rnd(rng, int(rng.integers(0, 3))), tree(depth - 1)), "", t)

    made = [("chain of 16 hairpins from base 1", chain(16, 1)), ("chain of 30 hairpins from base 1", chain(30, 1)),
            ("chain of 24 hairpins from base 0", chain(24, 0)), ("chain of 20 hairpins from base 3", chain(20, 3)),
            ("multi-branch loop of 15 hairpins", multi(15, 2)), ("multi-branch loop of 16 hairpins", multi(16, 1)),
            ("multi-branch loop of 29 hairpins", multi(29, 0)), ("multi-branch loop of 22 hairpins", multi(22, 2)),
            ("16 helices nested", nested(16, True)), ("30 helices nested", nested(30, False)), ("22 helices nested", nested(22, True)),
            ("binary tree of 31 helices", tree(4)),
            ("two trees of 15 helices side by side", _cat("a", tree(3), tree(3), "a")),
            ("multi-branch loops inside a chain", _cat("g", multi(7, 1), multi(8, 2), "c"))]
    out = []
    for name, (seq, dots) in made:
        pairs = _pairs_of(dots)
        pred = lambda s, p: _count(s, p)[0] < 100 and 16 <= _count(s, p)[1] <= 31       # noqa: E731
        assert pred(seq, pairs), (name, _count(seq, pairs))
        out.append((name, seq, pairs, pred))
    return out


# ---------------------------------------------------------------- what the drivers say
def _efn_drv(cases):
    energies = []
    with tempfile.TemporaryDirectory() as tmp:
        for seq, pairs in cases:
            f = os.path.join(tmp, "s.ct")
            with open(f, "w") as fp:
                fp.write(ct_text(seq, pairs))
            p = subprocess.run([EFN_DRV, f], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, EFNDATA=EFNDATA), timeout=60)
            assert p.returncode == 0, (seq, pairs, p.stderr.decode())
            energies.append(float([l for l in p.stdout.decode().splitlines() if l.startswith("energy")][0].split("=")[1]))
    return energies


def _efn2_drv(cases):
    from test_efn2_oracle import _efn2_drv as run
    defined = [c for c in cases if efn2_defined(*c)]
    got = iter(run("".join(ct_text(s, p) for s, p in defined).encode()))
    dg = [next(got) if efn2_defined(*c) else None for c in cases]
    assert len([x for x in dg if x is not None]) == len(defined)
    return dg


def families():
    """{family: [(name, seq, pairs)]} of all four families, in a fixed order"""
    return {"efn_random": [("efn_random %d" % k, s, p) for k, (s, p) in enumerate(efn_random())],
            "efn2_closed": [("efn2_closed %d" % k, s, p) for k, (s, p) in enumerate(efn2_closed())],
            "directed": [c[:3] for c in directed()],
            "large": [c[:3] for c in large()]}


def pins(family, cases):
    """[(efn_drv's energy in kcal/mol or None, efn2_drv's dG in 1/100 kcal/mol or None)] for the structures of a
    family.  None: no pin -- the existing families have one driver's each; in the new ones efn2_drv is not run
    where RM_efn2 leaves its arrays (efn2_defined), and efn2() must say 9999999 there."""
    cts = md5("".join(ct_text(s, p) for _, s, p in cases).encode())
    sp = [(s, p) for _, s, p in cases]
    if family == "efn_random":
        pin = pinned("efn_drv energy, random structures of default_rng(5)", lambda: {"input": cts, "energy": _efn_drv(sp)})
        efn, efn2 = pin["energy"], [None] * len(cases)
    elif family == "efn2_closed":
        pin = pinned("efn2_drv dG, closed structures of default_rng(20240602)", lambda: {"input": cts, "dG": _efn2_drv(sp)})
        efn, efn2 = [None] * len(cases), pin["dG"]
    else:
        pin = pinned("efn_drv energy and efn2_drv dG, %s structures" % family,
                     lambda: {"input": cts, "energy": _efn_drv(sp), "dG": _efn2_drv(sp)})
        efn, efn2 = pin["energy"], pin["dG"]
    assert pin["input"] == cts, "not the structures the pin of %s was made from" % family
    assert len(efn) == len(efn2) == len(cases)
    return list(zip(efn, efn2))


def energies_match(e2, e, pin, defined):
    """the comparison rules of test_efn_oracle.py (efn_drv prints kcal/mol with three decimals) and
    test_efn2_oracle.py (efn2_drv prints %5.2f: exact below 900 kcal/mol), on a record's two energy words"""
    want, want2 = pin
    ok = want is None or abs(0.01 * e - want) < 0.0051
    if want2 is not None:
        ok = ok and (e2 == want2 if abs(e2) < 90000 else abs(e2 - want2) <= 1)
    elif not defined:
        ok = ok and e2 == EFN2_UNDEFINED
    return ok


# ---------------------------------------------------------------- a structure as a small database
def as_db_text(seq):
    """the letters as the database readers deliver them: lower case, u as t"""
    return seq.replace("u", "t").encode()


def entries_of(seq, rng):
    """The entries a structure is scanned in, and where it was planted: [(entry, strand, start)].
    0: the sequence alone; 1: behind a flank, so that the window ends at the entry's last base and lies across
    base 96 of the entry, a boundary of the packed words (32 bases a word); 2: between two flanks, across base 128;
    3: the reverse complement alone, where the structure is the strand-1 candidate."""
    lut = np.frombuffer(b"acgt", dtype=np.uint8)
    flank = lambda n: lut[rng.integers(0, 4, size=n)].tobytes()        # noqa: E731
    s = as_db_text(seq)
    a = 96 - max(1, min(len(s), 62) // 2)
    rc = s.translate(bytes.maketrans(b"acgt", b"tgca"))[::-1]
    return ([s, flank(a) + s, flank(127) + s + flank(int(rng.integers(1, 40))), rc],
            [(0, 0, 0), (1, 0, a), (2, 0, 127), (3, 1, 0)])


def record_at(recs, entry, strand, start):
    """the rows of `recs` at (entry, strand, start)"""
    return recs[(recs[:, 0] == entry) & (recs[:, 1] == strand) & (recs[:, 2] == start)]
