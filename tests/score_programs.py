"""Score sections made to order, shared by tests/test_score_programs_cpu.py and tests/test_score_programs_gpu.py (no test here):

  * generate( seed, family, size ) -- a random but well-formed MAIN over the hairpin descriptor HP (a share of seeds over CTX
    with -context), written to the rules of ScoreVM::hit_independent (rm_score.cpp): every variable is assigned at the top of
    MAIN and keeps one type in every assignment; the leftmost operand of an arithmetic expression has the type of the variable
    it is stored to (do_arith leaves the left operand's type, so `f = ( 2 + f )` would store an int to a float variable and is
    refused); a postfix ++ / -- is a statement or a condition, never a value that is stored; SCORE is assigned last, with one
    type per program.  The generator keeps a bound of every int and float variable, so that no int overflows (the host VM's
    ints are C ints), of every string's length (substr() stays inside, a string SCORE fits a row of 64 bytes) and of the heap a
    record's made strings take (a lane's heap is never collected).  A minority of programs hold one statement that stops some
    records and not others;
  * sized( family, waves ) -- a program whose image leaves room for exactly `waves` waves in a workgroup, which reads and
    writes every variable, reaches its deepest stack with values that all end in SCORE, and both accepts and rejects;
  * limits() -- programs at and one beyond every limit of rm_score_image.h.

family: plain (flags 0, rma_score_kernel), text (2, ..._text_), match (8, ..._match_), match_text (10, ..._match_text_)."""
import os
import random

from test_score_device_cpu import CTX, HP
from test_score_match_cpu import PATTERNS

FAMILIES = ("plain", "text", "match", "match_text")
FLAGS = {"plain": 0, "text": 2, "match": 8, "match_text": 10}
W = 64          # a row of the score column in every run of these programs
HEAP = 256      # RMS_DEFAULT_HEAP, the scanner's score_heap as it is opened

COMMON = ["int variable", "float variable", "string variable", "+", "-", "*", "/", "%", "compound assignment", "++", "--", "int comparison",
          "float comparison", "string comparison", "&&", "||", "if", "else", "for", "while", "nested loops", "break", "continue", "REJECT",
          "tag=", "index=", "pos=", "len=", "$", "$-k", "pos= expression", "length", "substr", "mispairs", "mismatches( elem )", "paired", "loc", "in",
          "LEN", "POS", "COMP", "SLEN", "NSE"]
TEXT_ONLY = ["made string variable", "string +", "string +=", "substr of a made string", "sprintf", "%d", "%i", "%u", "%o", "%x", "%X", "%s", "%f", "bits",
             "string SCORE", "string reassigned in a loop"]
MATCH_ONLY = ["=~", "!~", "mismatches( string, pattern )", "match in a loop"]


def features_of(family):
    return COMMON + (TEXT_ONLY if FLAGS[family] & 2 else []) + (MATCH_ONLY if FLAGS[family] & 8 else [])


# patterns whose backtracking over a string of a few dozen letters stays far inside a record's budget of 2^20 steps
HEAVY = {".*\\(..\\).*\\1", "\\(..\\).*\\1", "\\(.\\)\\(.\\)\\2\\1"}


class _Gen:
    def __init__(self, seed, family, size):
        self.r = random.Random(seed)
        self.family, self.size = family, size
        self.text, self.match = bool(FLAGS[family] & 2), bool(FLAGS[family] & 8)
        self.used = set()
        self.ctx = self.r.random() < 0.15
        if self.ctx:        # (type, tag, shortest match or None: only read whole, longest match)
            self.elems = [("ctx", "L", None, 3), ("h5", "a", 4, 6), ("ss", "l", 4, 6), ("h3", "a", 4, 6)]
        else:
            self.elems = [("h5", "a", 4, 6), ("ss", "l", 4, 6), ("h3", "a", 4, 6), ("ss", "t", 2, 2)]
        self.ib, self.fb, self.sb = {}, {}, {}      # bounds: |int|, |float|, (shortest, longest) string
        self.made = set()                           # string variables that hold made strings
        self.heap = 0
        self.leak = 0
        self.deep = 1 if size == 0 else 2
        self.n_expr = 0
        self.mult = 1                               # rounds of the loops around the statement being written
        self.specials = set()

    # ---- element references
    def ref(self, whole=False, helix=False, tagged=None):
        """(text, shortest, longest) of an element reference that no record stops"""
        r = self.r
        cand = [(k, e) for k, e in enumerate(self.elems) if (not helix or e[0] in ("h5", "h3")) and (tagged is None or e[1] == tagged)]
        k, (ty, tag, lo, hi) = r.choice(cand)
        if r.random() < 0.6:
            self.used.add("tag=")
            head = "%s( tag='%s'" % (ty, tag)
        else:
            self.used.add("index=")
            head = "%s( index=%d" % (r.choice([ty, "se"]) if ty != "ctx" else "se", k + 1)
        if whole or lo is None or r.random() < 0.35:
            return head + " )", (lo if lo is not None else 0), hi
        form = r.randrange(6)
        if self.ctx and form in (2, 3, 4) or form == 4 and lo < 3 or form == 5 and self.size == 0:
            form = 0        # ($ reads rm_descr by an index of rm_xdescr: with an explicit context it is another element's length)
        if form == 0:
            p = r.randint(1, lo)
            n = r.randint(1, lo - p + 1)
            self.used.update(("pos=", "len="))
            return "%s, pos=%d, len=%d )" % (head, p, n), n, n
        if form == 1:
            p = r.randint(1, lo)
            self.used.add("pos=")
            return "%s, pos=%d )" % (head, p), lo - p + 1, hi - p + 1
        if form == 2:
            self.used.update(("pos=", "len=", "$"))
            return "%s, pos=$, len=1 )" % head, 1, 1
        if form == 3:
            k = r.randint(1, lo - 1)
            n = r.randint(1, k + 1)
            self.used.update(("pos=", "len=", "$-k"))
            return "%s, pos=$-%d, len=%d )" % (head, k, n), n, n
        if form == 4:
            self.used.update(("pos=", "len=", "$-k"))
            return "%s, pos=2, len=$-2 )" % head, lo - 2, hi - 2
        self.used.update(("pos=", "pos= expression"))
        self.special("LEN")
        e = r.choice(["1 + LEN %% %d" % min(lo, 3), "length( %s ) - %d" % (self.ref(whole=True, tagged="l")[0], 3), "COMP + 1"])
        if "COMP" in e:
            self.special("COMP")
        if lo < 3 and "length" in e:
            e = "1 + COMP"
            self.special("COMP")
        top = 3 if "length" in e or "LEN" in e else 2
        top = min(top, lo)
        if lo >= 4 and not self.ctx and r.random() < 0.5:
            # ($ behind a reference nested in pos=: the outer element's slot of the element stack is read after the inner one's was used)
            self.used.update(("len=", "$-k"))
            return "%s, pos=%s, len=$-3 )" % (head, e), lo - 3, hi - 3
        return "%s, pos=%s )" % (head, e), lo - top + 1, hi

    def special(self, name):
        if self.size == 0 and name not in self.specials and len(self.specials) >= (1 if self.match else 2):
            name = "LEN"        # (a small image names few variables)
        self.used.add(name)
        self.specials.add(name)
        return name

    def leaks(self, n=1):
        """mispairs(), mismatches( elem ), paired(), loc() and bits() leave their element on the element stack (only an element
        read as a string is popped, by STRF): a record has RMS_ESTK = 20 slots of it.  False: no room for another call here"""
        if self.leak + n * self.mult > 16:
            return False
        self.leak += n * self.mult
        return True

    # ---- int expressions: (text, bound)
    def int_leaf(self, small=False):
        r = self.r
        c = r.randrange(14 if not small else 11)
        if c == 0 or c == 1:
            v = r.randint(0, 9)
            return str(v), v
        if c == 2:
            return self.special("LEN"), 24
        if c == 3:
            return self.special("COMP"), 1
        if c == 4:
            return self.special("NSE"), 4
        if c == 5:
            k = r.randint(2, 9)
            return "( %s %% %d )" % (self.special(r.choice(["POS", "SLEN"])), k), k
        if c == 6:
            self.used.add("length")
            t, lo, hi = self.ref() if r.random() < 0.6 or not self.sb else self.svar()
            return "length( %s )" % t, hi
        if c in (7, 8, 9, 10) and not self.leaks():
            return self.special("LEN"), 24
        if c == 7:
            self.used.add("mispairs")
            return "mispairs( %s )" % self.ref(whole=True, helix=True)[0], 6
        if c == 8:
            self.used.add("mismatches( elem )")
            return "mismatches( %s )" % self.ref(whole=True, tagged="l")[0], 6
        if c == 9:
            self.used.add("paired")
            return "paired( %s( tag='a', pos=%d, len=%d ) )" % (r.choice(["h5", "h3"]), r.randint(1, 3), r.randint(1, 2)), 1
        if c == 10:
            k = r.randint(2, 11)
            self.used.add("loc")
            return "( loc( %s ) %% %d )" % (self.ref(whole=True)[0], k), k
        if self.match and c == 11 and self.room_for_expr():
            self.used.add("mismatches( string, pattern )")
            pat = r.choice(PATTERNS)
            return "mismatches( %s, \"%s\" )" % (self.str_for_match(pat), pat), 20 * len(pat) + 64
        if not self.ib:
            return "3", 3
        v = r.choice(sorted(self.ib))
        return v, self.ib[v]

    def int_expr(self, depth, small=False):
        r = self.r
        if depth <= 0 or r.random() < 0.25:
            return self.int_leaf(small)
        a, ba = self.int_expr(depth - 1, small)
        op = r.choice("++--**/%")
        self.used.add(op)
        if op in "+-":
            if r.random() < 0.06:
                t, b = "%s %s %s" % (a, op, r.choice(["0.5", "2.5", "1.0e1"])), ba + 10
            else:
                b, bb = self.int_expr(depth - 1, small)
                t, b = "%s %s %s" % (a, op, b), ba + bb
        elif op == "*":
            b, bb = self.int_leaf(small=True)
            if bb > 30:
                b, bb = str(r.randint(2, 9)), 9
            t, b = "%s * %s" % (a, b), ba * max(bb, 1)
        else:
            d = r.choice([str(r.randint(1, 7)), "( %s %% %d + 1 )" % (self.special("LEN"), r.randint(2, 4))])
            t, b = "%s %s %s" % (a, op, d), ba
        if b > 10 ** 7:
            self.used.add("%")
            return "( %s ) %% 1009" % t, 1009
        return "( %s )" % t, b

    # ---- float expressions: the leftmost operand is a float
    def float_leaf(self):
        r = self.r
        c = r.randrange(5 if self.text else 4)
        if c == 0:
            v = r.choice(["0.5", "1.5", "2.25", "0.1", "3.0", "1.0e-3", "7.75"])
            return v, 8.0
        if c == 1:
            t, b = self.int_leaf(small=True)
            return "1.0 * ( %s )" % t, float(b)
        if c == 4 and not self.leaks(2):
            return "0.75", 1.0
        if c == 4:
            self.used.add("bits")
            if self.ctx:
                return "bits( h5( tag='a' ), h3( tag='a' ) )", 8.0
            return r.choice(["bits( h5( tag='a' ), h3( tag='a' ) )", "bits( h5( tag='a', pos=2 ), ss( tag='l', pos=3 ) )",
                             "bits( ss( tag='l', pos=1 ), h3( tag='a', pos=2 ) )"]), 8.0
        if not self.fb:
            return "1.25", 2.0
        v = r.choice(sorted(self.fb))
        return v, self.fb[v]

    def float_expr(self, depth):
        r = self.r
        if depth <= 0 or r.random() < 0.25:
            return self.float_leaf()
        a, ba = self.float_expr(depth - 1)
        op = r.choice("++--**/")
        self.used.add(op)
        if op in "+-":
            if r.random() < 0.3:
                b, bb = self.int_leaf(small=True)
            else:
                b, bb = self.float_expr(depth - 1)
            t, b = "%s %s %s" % (a, op, b), ba + bb
        elif op == "*":
            b, bb = self.float_leaf() if r.random() < 0.7 else self.int_leaf(small=True)
            t, b = "%s * %s" % (a, b), ba * max(bb, 1.0)
        else:
            d = r.choice(["3.0", "0.7", "7.0", "( %s %% 3 + 1 )" % self.special("LEN")])
            t, b = "%s / %s" % (a, d), ba * 2.0
        if b > 1.0e9:
            return self.float_leaf()
        return "( %s )" % t, b

    # ---- strings: (text, shortest, longest)
    def svar(self):
        v = self.r.choice(sorted(self.sb))
        return (v,) + self.sb[v]

    def takes_heap(self, n):
        cost = (n + 8) * self.mult
        if self.heap + cost > HEAP - 40:
            return False
        self.heap += cost
        return True

    def str_expr(self, depth=1, longest=40):
        r = self.r
        c = r.randrange(9 if self.text else 5)
        if c <= 1 or depth <= 0:
            return self.ref()
        if c == 2:
            n = r.randint(0, 3)
            return "'%s'" % "".join(r.choice("acgt") for _ in range(n)), n, n
        if c == 3 and self.sb:
            return self.svar()
        if c == 4:
            if self.made and r.random() < 0.5:
                v = r.choice(sorted(self.made))
                t, lo, hi = (v,) + self.sb[v]
            else:
                t, lo, hi = self.str_expr(depth - 1) if self.text and r.random() < 0.5 or not self.sb else self.svar()
            if lo >= 1 and self.takes_heap(hi):
                p = r.randint(1, lo)
                n = r.randint(1, lo - p + 1)
                self.used.add("substr")
                if t in self.made:
                    self.used.add("substr of a made string")
                return "substr( %s, %d, %d )" % (t, p, n), n, n
            return self.ref()
        if c in (5, 6):
            a, alo, ahi = self.str_expr(depth - 1)
            b, blo, bhi = self.str_expr(0) if r.random() < 0.6 else ("'-'", 1, 1)
            if ahi + bhi <= longest and self.takes_heap(ahi + bhi):
                self.used.add("string +")
                return "%s + %s" % (a, b), alo + blo, ahi + bhi
            return self.ref()
        if c >= 7:
            t = self.sprintf(longest)
            if t is not None:
                return t
        return self.ref()

    def sprintf(self, longest):
        """(text, shortest, longest) of a sprintf() whose result has at most `longest` bytes, or None"""
        r = self.r
        fmt, args, lo, hi = "", [], 0, 0
        for _ in range(r.randint(1, 4)):
            conv = r.choice("diuoxXsf")
            flags = "".join(f for f in "-+ 0#" if r.random() < 0.2)
            if conv == "s":
                flags = flags.replace("0", "").replace("#", "").replace("+", "").replace(" ", "")
            width = r.choice(["", "", str(r.randint(1, 12))])
            prec = ""
            if conv == "f":
                prec = r.choice(["", ".0", ".1", ".3", ".%d" % r.randint(0, 18)])
                a, b = self.float_leaf() if r.random() < 0.5 or not self.fb else self.fvar()
                a = "( %s )" % a
                if b > 1.0e9:
                    continue
                natural = 12 + (6 if prec == "" else int(prec[1:])) + 2
                least = 1
            elif conv == "s":
                prec = r.choice(["", "", ".%d" % r.randint(1, 5)])
                a, slo, shi = self.str_expr(0)
                natural, least = shi, (0 if prec else slo)
            else:
                prec = r.choice(["", "", ".%d" % r.randint(1, 6)])
                a, b = self.int_expr(1, small=True)
                natural, least = 13, 1
            n = max(natural, int(width) if width else 0)
            lit = r.choice(["", " ", "|", "-", ":", " x"])
            if hi + n + len(lit) > longest:
                continue
            fmt += "%" + flags + width + prec + conv + lit
            args.append(a)
            lo, hi = lo + least + len(lit), hi + n + len(lit)
            self.used.update(("%" + conv,))
        if not args or not self.takes_heap(hi):
            return None
        self.used.add("sprintf")
        return "sprintf( '%s', %s )" % (fmt, ", ".join(args)), lo, hi

    def fvar(self):
        v = self.r.choice(sorted(self.fb))
        return v, self.fb[v]

    # ---- conditions
    def room_for_expr(self):
        # (an expression in a loop is one expression of the image; its steps count against the record's budget)
        if self.n_expr >= 12 or self.mult > 16:
            return False
        self.n_expr += 1
        return True

    def str_for_match(self, pat):
        if pat in HEAVY or self.mult > 1:
            return self.ref()[0]
        return self.str_expr(1, longest=24)[0]

    def cond(self, depth=1, varying=False):
        r = self.r
        if depth > 0 and r.random() < 0.35:
            op = r.choice(["&&", "||"])
            self.used.add(op)
            return "%s %s %s" % (self.cond(depth - 1, varying), op, self.cond(depth - 1, varying))
        c = r.randrange(9 if self.match else 7)
        if c == 0 or c == 1:
            self.used.add("int comparison")
            if varying or r.random() < 0.5:
                k = r.randint(2, 4)
                self.used.add("%")
                return "%s %% %d == %d" % (self.special("LEN"), k, r.randrange(k))
            return "%s %s %s" % (self.int_expr(1)[0], r.choice(["<", "<=", ">", ">=", "==", "!="]), self.int_expr(1)[0])
        if c == 2:
            self.used.add("float comparison")
            return "%s %s %s" % (self.float_expr(1)[0], r.choice(["<", "<=", ">", ">="]), self.float_expr(1)[0])
        if c == 3:
            self.used.add("string comparison")
            return "%s %s %s" % (self.ref()[0] if varying else self.str_expr(1)[0], r.choice(["<", "<=", ">", ">=", "==", "!="]),
                                 r.choice(["'c'", "'g'", "'ga'", "'t'", "'cg'"]) if varying or r.random() < 0.6 else self.str_expr(0)[0])
        if c == 4:
            self.used.add("in")
            sets = ["\"g:c\", \"c:g\"", "\"g:c\", \"c:g\", \"a:t\"", "\"a:t\", \"t:a\", \"g:t\"", "\"g:c\""]
            self.used.update(("pos=", "len=", "tag="))
            if self.ctx:
                return "h5( tag='a', pos=1, len=1 ):h3( tag='a', pos=%d, len=1 ) in { %s }" % (r.randint(1, 4), r.choice(sets))
            self.used.add("$")
            return "h5( tag='a', pos=%d, len=1 ):h3( tag='a', pos=$%s, len=1 ) in { %s }" % ((1, "", r.choice(sets)) if r.random() < 0.5 else (2, "-1", r.choice(sets)))
        if c in (5, 6) and not self.leaks():
            c = 0
        if c == 0 or c == 1:
            self.used.update(("int comparison", "%"))
            k = r.randint(2, 4)
            return "%s %% %d == %d" % (self.special("LEN"), k, r.randrange(k))
        if c == 5:
            self.used.add("paired")
            return "%spaired( %s( tag='a', pos=%d, len=%d ) )" % (r.choice(["", "!"]), r.choice(["h5", "h3"]), r.randint(1, 3), r.randint(1, 2))
        if c == 6:
            self.used.update(("int comparison", "mispairs"))
            return "mispairs( %s ) %s 0" % (self.ref(whole=True, helix=True)[0], r.choice([">", "=="]))
        if not self.room_for_expr():
            self.used.add("int comparison")
            return "%s > 14" % self.special("LEN")
        op = r.choice(["=~", "=~", "!~"])
        self.used.add(op)
        if self.mult > 1:
            self.used.add("match in a loop")
        pat = r.choice(PATTERNS)
        return "%s %s \"%s\"" % (self.str_for_match(pat), op, pat)

    # ---- statements
    def assign(self, depth_left):
        r = self.r
        kinds = ["int"] * 3 + (["float"] * 2 if self.fb else []) + (["string"] * 2 if self.sb else [])
        kind = r.choice(kinds)
        in_loop = self.mult > 1
        if kind == "int":
            v = r.choice(sorted(x for x in self.ib if x not in "ijk"))      # (a loop's own variable is only read)
            c = r.randrange(5)
            if c == 0:
                op = r.choice(["++", "--"])
                self.used.add(op)
                self.ib[v] += self.mult
                return "%s%s;" % (v, op)
            if c == 1:
                self.used.add("compound assignment")
                op = r.choice(["+=", "-=", "*=", "/=", "%="])
                self.used.add(op[0])
                if op in ("+=", "-="):
                    t, b = self.int_expr(1, small=True)
                    b = min(b, 10 ** 6)
                    self.ib[v] += b * self.mult
                    if self.ib[v] > 10 ** 8:
                        self.ib[v] = 1009
                        return "%s = ( %s ) %% 1009;" % (v, v)
                    return "%s %s %s;" % (v, op, t)
                if op == "*=":
                    if in_loop or self.ib[v] > 10 ** 6:
                        self.ib[v] = 1009 * 3
                        return "%s %%= 1009; %s *= 3;" % (v, v)
                    k = r.randint(2, 5)
                    self.ib[v] *= k
                    return "%s *= %d;" % (v, k)
                return "%s %s %s;" % (v, op, r.choice([str(r.randint(2, 7)), "( %s %% 3 + 1 )" % self.special("LEN")]))
            t, b = self.int_expr(self.deep)
            if in_loop or b > 10 ** 7:
                self.used.add("%")
                self.ib[v] = max(self.ib[v], 1009)
                return "%s = %s %% 1009;" % (v, t)
            self.ib[v] = max(self.ib[v], b)
            return "%s = %s;" % (v, t)
        if kind == "float":
            v = r.choice(sorted(self.fb))
            if in_loop:
                if r.random() < 0.5:
                    self.used.update(("compound assignment", "+"))
                    self.fb[v] += 8.0 * self.mult
                    return "%s += %s;" % (v, r.choice(["0.25", "1.5", "0.1"]))
                self.used.update(("*", "+"))
                self.fb[v] = max(self.fb[v], 64.0)
                return "%s = %s * 0.5 + %s;" % (v, v, self.float_leaf_no_var()[0])
            t, b = self.float_expr(self.deep)
            self.fb[v] = max(self.fb[v], b)
            return "%s = %s;" % (v, t)
        v = r.choice(sorted(self.sb))
        lo, hi = self.sb[v]
        if self.text and v in self.made and r.random() < 0.4:
            t, tlo, thi = self.str_expr(0, longest=6) if r.random() < 0.6 else ("'a'", 1, 1)
            if not t.startswith("sprintf") and hi + thi * self.mult <= 40 and self.takes_heap(hi + thi * self.mult):
                self.sb[v] = (lo, hi + thi * self.mult)
                if in_loop:
                    self.used.add("string reassigned in a loop")
                if r.random() < 0.5:
                    self.used.update(("string +=", "compound assignment"))
                    return "%s += %s;" % (v, t)
                self.used.add("string +")
                return "%s = %s + %s;" % (v, v, t)
        if v in self.made or not self.text:
            t, tlo, thi = self.str_expr(1, longest=30)
            if in_loop:
                self.used.add("string reassigned in a loop")
        else:
            t, tlo, thi = self.ref()
        if "substr( %s," % v in t:        # (in a loop the second round would cut what the first one left)
            t, tlo, thi = self.ref()
        self.sb[v] = (min(lo, tlo), max(hi, thi))
        return "%s = %s;" % (v, t)

    def float_leaf_no_var(self):
        while True:
            t, b = self.float_leaf()
            if t not in self.fb:
                return t, b

    def block(self, n, loops_left, loop_var=None):
        return " ".join(self.statement(loops_left, loop_var) for _ in range(n))

    def statement(self, loops_left, loop_var):
        r = self.r
        c = r.random()
        if c < 0.40:
            return self.assign(loops_left)
        if c < 0.60:
            self.used.add("if")
            s = "if( %s ){ %s }" % (self.cond(1), self.assign(loops_left) if r.random() < 0.6 else self.block(2, loops_left, loop_var))
            if r.random() < 0.4:
                self.used.add("else")
                s += " else { %s }" % self.assign(loops_left)
            return s
        if c < 0.74 and loop_var is not None:
            w = r.choice(["break", "continue"])
            self.used.update((w, "if"))
            return "if( %s ) %s;" % (self.cond(0), w)
        if c < 0.80:
            self.used.update(("REJECT", "if"))
            return "if( %s ) REJECT;" % self.cond(1, varying=True)
        if loops_left > 0 and self.mult <= 16:
            lv = "ijk"[3 - loops_left] if self.size else "i"
            trips = r.randint(2, 4)
            if loop_var is not None:
                self.used.add("nested loops")
            outer = self.mult
            self.mult *= trips
            self.ib[lv] = max(self.ib.get(lv, 0), trips + 1)
            body = self.block(r.randint(1, 3), loops_left - 1, lv)
            self.mult = outer
            top = r.choice([str(trips), "%s %% %d + 1" % (self.special("LEN"), trips), "NSE" if trips == 4 else str(trips)])
            if top == "NSE":
                self.special("NSE")
            form = r.randrange(3)
            if form == 0:
                self.used.update(("for", "++"))
                return "for( %s = 0; %s < %s; %s++ ){ %s }" % (lv, lv, top, lv, body)
            self.used.add("while")
            if form == 1:
                self.used.add("+")
                return "%s = 0; while( %s < %s ){ %s = %s + 1; %s }" % (lv, lv, top, lv, lv, body)
            self.used.add("--")
            return "%s = %d; while( %s-- ){ %s }" % (lv, trips, lv, body)
        return self.assign(loops_left)

    def stop_statement(self):
        r = self.r
        v = sorted(x for x in self.ib if x not in "ijk")[0]
        c = r.randrange(4)
        if c == 0:
            return "%s = 10 / ( %s %% 3 );" % (v, self.special("LEN")), "division by zero"
        if c == 1:
            return "%s %%= ( %s %% 2 );" % (v, self.special("LEN")), "division by zero"
        if c == 2:
            return "if( h5( tag='a', pos=6, len=1 ) == 'g' ) %s = %s + 1;" % (v, v), "bad pos"
        return "if( substr( ss( tag='l' ), 2, %s %% 3 - 1 ) == 'a' ) %s = %s + 1;" % (self.special("LEN"), v, v), "substr: bad len"

    def program(self):
        r = self.r
        small = self.size == 0
        tiny = small and self.match        # (the matcher's planes are a wave's too: four waves have room for a few slots each)
        n_int, n_float, n_str = (1, 0, 0) if tiny else (1, r.randint(0, 1), r.randint(0, 1)) if small else (r.randint(1, 3), r.randint(1, 2), r.randint(1, 2))
        score = r.choice(["int", "int", "float"] + (["string"] * 2 if self.text else []))
        ints, floats, strs = ["n%d" % k for k in range(n_int)], ["f%d" % k for k in range(n_float)], ["s%d" % k for k in range(n_str)]
        self.used.update(("int variable", "float variable", "string variable"))
        top = []
        for v in ints:
            t, b = self.int_expr(1)
            self.ib[v] = b
            top.append("%s = %s;" % (v, t))
        for v in floats:
            t, b = self.float_expr(1)
            self.fb[v] = b
            top.append("%s = %s;" % (v, t))
        for k, v in enumerate(strs):
            if self.text and (k == 0 or r.random() < 0.5):
                t, lo, hi = self.str_expr(1, longest=20)
                self.made.add(v)
                self.used.add("made string variable")
            else:
                t, lo, hi = self.ref()
            self.sb[v] = (lo, hi)
            top.append("%s = %s;" % (v, t))
        loop_vars = "i" if small else "ijk"
        for lv in loop_vars:
            self.ib[lv] = 0
        top.append(" ".join("%s = 0;" % lv for lv in loop_vars))
        # the extra variables a size asks for: all of them written here and read below
        want = {0: 0, 1: 20, 2: 32, 3: 50}[self.size] - (3 if self.text else 0) - (5 if self.match else 0)
        body = self.block(r.randint(2, 3), 1) if tiny else self.block(r.randint(3, 5), 1) if small else self.block(r.randint(4, 8), 3)
        stop = None
        if r.random() < 0.27:
            stop = self.stop_statement()
        reject = "if( %s ) REJECT;" % self.cond(0, varying=True) if r.random() < 0.8 else ""
        if reject:
            self.used.update(("REJECT", "if"))
        have = n_int + n_float + n_str + len(loop_vars) + 1 + len(self.specials | {"LEN"}) + 8 + (8 if self.match and self.n_expr else 0)
        pads = ["x%d" % k for k in range(max(0, want - have))]
        fold = ""
        if pads:
            top.append(" ".join("%s = %d + %s %% %d;" % (v, k, self.special("LEN"), k % 5 + 2) for k, v in enumerate(pads)))
            depth = min(len(pads), 6)
            nest = "".join("%s + ( " % v for v in pads[:depth]) + self.special("LEN") + " )" * depth
            fold = "%s = ( %s + %s + %s ) %% 1009;" % (ints[0], ints[0], " + ".join(pads), nest)
            self.ib[ints[0]] = max(self.ib[ints[0]], 1009)
            self.used.update(("+", "%"))
        if score == "int":
            t, b = self.int_expr(self.deep)
            last = "SCORE = %s + %s %% 1009;" % (t if b < 10 ** 7 else "0", ints[0])
        elif score == "float":
            last = "SCORE = %s + %s %% 1009;" % (self.float_expr(self.deep)[0], ints[0])
        else:
            self.used.add("string SCORE")
            self.heap = min(self.heap, HEAP - 120)
            t = self.sprintf(40) if r.random() < 0.6 else None
            if t is None:
                t = self.str_expr(1, longest=30)
            self.used.update(("sprintf", "%d", "%s"))
            last = "SCORE = sprintf( '%%s %%d', %s, %s %% 1009 );" % (t[0], ints[0])
        # (the stop is written once: in front of the body or behind it)
        before = stop is not None and r.random() < 0.5
        once = top + ([stop[0]] if before else []) + [body] + ([stop[0]] if stop is not None and not before else [])
        text = (CTX if self.ctx else HP) + "\t{ " + "\n\t  ".join(p for p in once + [reject, fold, last] if p) + " }\n"
        feats = set(self.used)
        if stop:
            feats.add("stop: " + stop[1])
        return text, feats


def wrap(text):
    """the same descriptor with short lines: the parser's line buffer is no part of what is tested"""
    head, main = text.split("score\n", 1)
    out = []
    for ln in main.replace("; ", ";\n\t  ").split("\n"):
        while len(ln) > 150:
            for sep in (" + ", " && ", " || ", ", ", " "):
                at = ln.rfind(sep, 20, 150)
                if at > 0:
                    break
            if at <= 0:
                break
            out.append(ln[:at + len(sep) - 1])
            ln = "\t    " + ln[at + len(sep) - 1:].lstrip(" ")
        out.append(ln)
    return head + "score\n" + "\n".join(out)


def generate(seed, family, size):
    """(the descriptor's text, the arguments in front of -descr, the features MAIN uses)"""
    g = _Gen(seed, family, size)
    text, feats = g.program()
    return wrap(text), (["-context"] if g.ctx else []), feats


# ---------------------------------------------------------------- programs of a wanted shape
def nest(depth, inner):
    """1 + ( 2 + ( ... ( inner ) ) ): the operand stack is `depth` slots deeper at `inner` than at the 1"""
    return "".join("%d + ( " % (k % 9 + 1) for k in range(depth)) + inner + " )" * depth


# family -> waves -> (variables, nesting, lean): ( stack + variables ) * 768 + 1280 bytes a wave (rms_wave_bytes), the matcher's
# planes behind them in the match kernels -- 18 + 4 * frames slots of 256 bytes (rmq_wave_bytes) --, 65536 - 512 - the image's
# bytes of room (score_waves).  The full program names n + 5 variables (and s with text) and its stack is nesting + 10 slots; four
# waves of a match kernel have room for a dozen slots each beside the matcher's, so that program is a lean one: one variable
# (and s), no loop, and patterns without a repeating op (no frame).  The image's sizes are the checker's IMAGE line, asserted by the tests.
SIZED = {
    "plain": {4: (2, 1, False), 3: (5, 4, False), 2: (12, 8, False), 1: (24, 12, False)},
    "text": {4: (2, 0, False), 3: (5, 3, False), 2: (12, 7, False), 1: (24, 11, False)},
    "match": {4: (1, 0, True), 3: (2, 0, False), 2: (6, 5, False), 1: (20, 10, False)},
    "match_text": {4: (1, 0, True), 3: (1, 0, False), 2: (6, 4, False), 1: (20, 9, False)},
}


def sized(family, waves):
    """the text of a descriptor over HP whose image has room for exactly `waves` waves"""
    n, depth, lean = SIZED[family][waves]
    vs = ["v%d" % k for k in range(n)]
    text, match = bool(FLAGS[family] & 2), bool(FLAGS[family] & 8)
    size = "length( ss( tag='l' ) )" if lean else "LEN"
    lines = [" ".join("%s = %s %% %d + %d;" % (v, size, k % 5 + 2, k) for k, v in enumerate(vs))]
    if text:
        lines.append("s = ss( tag='l' ) + '-' + h5( tag='a', pos=1, len=2 );")
    if lean:
        v = vs[0]
        lines.append("if( %s =~ \"^g[ac]\" ) %s = %s + 1; %s = %s + 3 * mismatches( h5( tag='a' ), \"gc.c\" );" % ("s" if text else "ss( tag='l' )", v, v, v, v))
        lines.append("if( %s %% 3 == 0 ) REJECT;" % v)
        total = v
    else:
        lines.append("m = 0;")
        if match:
            lines.append("if( %s =~ \"^g*a*[ct]\" ) m = 1; m = m + mismatches( h5( tag='a' ), \"\\(g.\\)c\\1\" );" % ("s" if text else "ss( tag='l' )"))
        # every variable is read and written twice over, each from its neighbour
        step = " ".join("%s = %s + %s %% 7;" % (v, v, vs[(k + 1) % n] if n > 1 else "m") for k, v in enumerate(vs))
        lines.append("for( i = 0; i < 2; i++ ){ " + step + " }")
        # the deepest stack, every slot of it a value that ends in d
        lines.append("d = %s;" % nest(depth, "%s + LEN * mispairs( h5( tag='a' ) )" % vs[0]))
        lines.append("if( ( d + %s ) %% 3 == 0 ) REJECT;" % vs[-1])
        total = " + ".join(["d", "m"] + ["%s * %d" % (v, k % 3 + 1) for k, v in enumerate(vs)])
    lines.append("SCORE = sprintf( '%%d %%s', %s, s );" % total if text else "SCORE = %s;" % total)
    return wrap(HP + "\t{ " + "\n\t  ".join(lines) + " }\n")


# ---------------------------------------------------------------- programs at the image's limits
def _ifs(n, fill):
    return "".join("\t  if( LEN %% %d == 1 ) n = n + %d;\n" % (k % 7 + 2, k % 9 + 1) for k in range(n)) + "".join("\t  %s;\n" % f for f in fill)


def inst_program(n, fill=()):
    return HP + "\t{ n = 0;\n" + _ifs(n, fill) + "\t  if( n % 5 == 0 ) REJECT; SCORE = n; }\n"


def vars_program(n, named=()):
    """n int variables written and read; `named`: specials MAIN reads beside them"""
    vs = ["v%d" % k for k in range(n)]
    return HP + ("\t{ " + " ".join("%s = LEN %% %d + %d;" % (v, k % 5 + 2, k) for k, v in enumerate(vs)) + "\n\t  SCORE = " + " + ".join(vs + list(named)) + ";\n"
                 "\t  if( SCORE % 3 == 0 ) REJECT; }\n")


def stack_program(depth, n_vars=0):
    vs = ["v%d" % k for k in range(n_vars)]
    return HP + ("\t{ " + " ".join("%s = LEN %% %d + %d;" % (v, k % 5 + 2, k) for k, v in enumerate(vs)) + "\n\t  SCORE = " + nest(depth, " + ".join(["LEN"] + vs)) + ";\n"
                 "\t  if( SCORE % 3 == 0 ) REJECT; }\n")


def frames_program(frames, depth, n_vars):
    """a pattern of `frames` repeating ops beside a stack and variables: the matcher's planes decide whether a wave fits"""
    pat = "^" + "".join("acgt"[k % 4] + "*" for k in range(frames)) + "$"
    vs = ["v%d" % k for k in range(n_vars)]
    return HP + ("\t{ " + " ".join("%s = LEN %% %d + %d;" % (v, k % 5 + 2, k) for k, v in enumerate(vs)) + "\n\t  m = 0; if( ss( tag='l' ) =~ \"%s\" ) m = 1;\n" % pat +
                 "\t  SCORE = m + " + nest(depth, " + ".join(["LEN"] + vs)) + ";\n\t  if( SCORE % 3 == 0 ) REJECT; }\n")


def pool_program(n_bytes):
    """string constants of n_bytes bytes in all, beside what the image pools anyway"""
    chunks, k = [], 0
    while n_bytes > 0:
        n = min(n_bytes, 100)
        chunks.append(("".join("acgt"[(k >> (2 * j)) & 3] for j in range(4)) + "".join("acgt"[(i * 7 + i // 5) % 4] for i in range(n)))[:n])
        n_bytes -= n
        k += 1
    return HP + ("\t{ n = 0;\n" + "".join("\t  if( ss( tag='l' ) < \"%s\" ) n = n + %d;\n" % (c, 1 << (k % 8)) for k, c in enumerate(chunks)) +
                 "\t  if( n % 3 == 0 ) REJECT; SCORE = n; }\n")


def pairset_program(n):
    pairs = ["%s:%s" % (a, b) for a in "acgt" for b in "acgt"]
    sets = ["\"%s\", \"%s\"" % (pairs[k % 16], pairs[(k % 16 + 1 + k // 16) % 16]) for k in range(n)]
    return HP + ("\t{ n = 0;\n" + "".join("\t  if( h5( tag='a', pos=1, len=1 ):h3( tag='a', pos=$, len=1 ) in { %s } ) n = n + %d;\n" % (s, k % 7 + 1) for k, s in enumerate(sets)) +
                 "\t  if( LEN % 3 == 0 ) REJECT; SCORE = n; }\n")


def expr_program(n):
    return HP + "\t{ n = 0;\n" + "".join("\t  if( %s =~ \"%s\\{%d\\}\" ) n = n + %d;\n" % (("ss( tag='l' )", "h5( tag='a' )")[k % 2], "acgt"[k % 4], k % 3 + 1, k) for k in range(1, n + 1)) + "\t  if( LEN % 3 == 0 ) REJECT; SCORE = n; }\n"


def estk_program(depth):
    """element references nested in pos=, `depth` of them open at the innermost: ss( tag='t' ) has two bases, so every pos= is 1 or 2"""
    e = "ss( tag='t' )"
    for _ in range(depth - 1):
        e = "ss( tag='t', pos=length( %s ) )" % e
    return HP + "\t{ n = length( %s ); if( LEN %% 3 == 0 ) REJECT; SCORE = n * 10 + LEN; }\n" % e


# ---------------------------------------------------------------- through the checkers
def build_checkers():
    """family -> the host checker that runs its rule against ScoreVM::run and HitPrinter::print"""
    from test_score_device_cpu import build_checker
    from test_score_match_cpu import build_match_checker
    from test_score_text_cpu import build_text_checker
    m = build_match_checker()
    return {"plain": build_checker(), "text": build_text_checker(), "match": m, "match_text": m}


def write_descr(text, tmp, name):
    path = os.path.join(str(tmp), name + ".descr")
    with open(path, "w") as f:
        f.write(text)
    return path


def run_family(checker, family, tmp, argv, entries, recs, checker_of_family=None):
    """A program through its family's checker (checker_of_family: a build of score_match_check, which runs all four):
    (refusal or None, the image's sizes, [(outcome, kind, bits, length of the column, column, words)], status, stdout)."""
    from test_score_device_cpu import run_checker
    from test_score_text_cpu import run_text_checker
    if family == "plain" and checker_of_family is None:
        refused, image, rows, status, out = run_checker(checker, tmp, argv, entries, recs)
        return refused, image, [(r[0], r[1], r[2], 0, b"", r[3]) for r in rows], status, out
    refused, image, rows, status, out, _ = run_text_checker(checker_of_family or checker, tmp, argv, entries, recs, flags=FLAGS[family], heap=HEAP,
                                                            stride=W if FLAGS[family] & 2 else 0)
    return refused, image, rows, status, out


def waves_of(image):
    """score_waves() of rm_score_dev.hip from a checker's IMAGE line (wave_bytes has the matcher's planes in it)"""
    room = 64 * 1024 - 512 - image["bytes"]
    return min(4, room // image["wave_bytes"]) if room >= image["wave_bytes"] else 0


def limits():
    """[(name, family, the descriptor's text, the words of its refusal or None where it opens, {what its IMAGE line must say})]"""
    fills = ["n++", "n++", "n = n * 2 + 1"]
    out = [
        ("stack of 62", "plain", stack_program(59), None, {"deepest": 62, "stack": 64}),
        ("stack of 63", "plain", stack_program(60), "MAIN's operand stack can reach 63 slots, the image allows 62", None),
        ("64 variables", "plain", vars_program(62, ["LEN"]), None, {"vars": 64}),
        ("65 variables named", "plain", vars_program(63, ["LEN"]), "MAIN names 65 variables, the image holds 64", None),
        ("65 variables written", "plain", vars_program(64), "more than 64 variables written", None),
        ("one wave just fits", "plain", stack_program(34, 34), None, {"wave_bytes": 59648}),
        ("one wave does not fit", "plain", stack_program(35, 34), "a wave's 60416 bytes of stack and variables leave no room for one wave in 65536 bytes of LDS", None),
        ("one wave just fits with 24 frames", "match", frames_program(24, 10, 20), None, {"frames": 24, "wave_bytes": 60416}),
        ("one wave does not fit with 25 frames", "match", frames_program(25, 10, 20),
         "bytes of its matcher's 25 frames leave no room for one wave in 65536 bytes of LDS", None),
        ("4096 instructions", "plain", inst_program(290, fills), None, {"inst": 4096}),
        ("4097 instructions", "plain", inst_program(290, ["n = n * 2 + 1"] * 2), "MAIN has 4097 instructions, the image holds 4096", None),
        ("8192 bytes of strings", "plain", pool_program(8191), None, {"pool": 8192}),
        ("8193 bytes of strings", "plain", pool_program(8192), "8193 bytes of strings, the image holds 8192", None),
        ("64 pair sets", "plain", pairset_program(62), None, {"pairsets": 64}),
        ("65 pair sets", "plain", pairset_program(63), "65 pair sets, the image holds 64", None),
        ("32 expressions", "match", expr_program(32), None, {"expr": 32}),
        ("32 expressions with text", "match_text", expr_program(32), None, {"expr": 32}),
    ]
    return [(name, family, wrap(text), refused, image) for name, family, text, refused, image in out]


# the element stack's edge: (name, the descriptor's text, does a record stop?)
def element_stack():
    """RMS_ESTK is 20.  Only an element read as a string leaves the stack again, so nested references fill it as deep as they are
    nested, and mispairs() / loc() / paired() / mismatches( elem ) / bits() fill it by one (two) a call, for the rest of the record."""
    def calls(n):
        return HP + ("\t{ n = 0;\n" + "".join("\t  n = n + mispairs( h5( tag='a' ) ) + %d;\n" % k for k in range(n)) + "\t  if( LEN % 3 == 0 ) REJECT; SCORE = n; }\n")
    dollar = HP + "\t{ s = h5( tag='a', pos=length( ss( tag='t' ) ), len=$-2 ); if( LEN % 3 == 0 ) REJECT; SCORE = length( s ) * 100 + LEN; }\n"
    return [("20 references nested", wrap(estk_program(20)), False), ("21 references nested", wrap(estk_program(21)), True),
            ("$ behind a nested reference", dollar, False),
            ("20 calls that leave their element", calls(20), False), ("21 calls that leave their element", calls(21), True)]
