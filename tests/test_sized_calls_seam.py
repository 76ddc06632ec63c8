"""GPU: the calls that size an output on the device and then fill it -- Scanner.hit_structures, print_hits and ct_hits
(rma_hit_structures, rma_hit_print, rma_hit_ct with their _size calls) -- refused behind the chunk seam.  2^17 + 3 rows
made by indexing a few records of a three-base hairpin scan: the smallest call with a second chunk, whose fill runs the
sizes a second time into spare refusal words.  For each call:

  * a malformed row in the second chunk is named by its index in the call, not in its chunk;
  * a `total` that is not the size call's is refused with the outputs left as they were;
  * a text_len outside its row in the second chunk is named likewise (print and .ct);
  * right after each refusal the same scanner makes of the unmodified rows what it made before: the refusal words, the
    spare ones and the carried total leave nothing behind.

torch is imported before the product library: one HIP runtime serves the process."""
import ctypes
import re

import torch  # noqa: F401  (first: its HIP runtime is the process's)

import numpy as np
import pytest

import rnamotif_amd as R
from test_hit_ct_cpu import _descr_of, columns
from test_hit_print_cpu import HAND

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

DEV = torch.device("cuda", 0)
CHUNK = 1 << 17
N = CHUNK + 3
CALLS = ("structures", "print", "ct")
NOTHING = {"structures": "nothing written", "print": "nothing printed", "ct": "nothing written"}
NOUN = {"structures": "the windows", "print": "the lines", "ct": "the .ct records"}
SEQS = [b"acgtnacgtryk" * 4, b"ggggaaaacccc" * 3, b"gggaaaccc" * 4]
WIDTH = 8


class Seam:
    """the rows, their score columns and what each call makes of them, computed once"""

    def __init__(self, tmp):
        self.d = _descr_of(tmp, "hand", HAND)
        self.sc = R.Scanner(self.d, device=0)
        off = np.concatenate([[0], np.cumsum([len(s) for s in SEQS])]).astype(np.int64)
        self.db = self.sc.database_from_tensor(torch.frombuffer(bytearray(b"".join(SEQS)), dtype=torch.uint8).to(DEV), offsets=off)
        self.names = R.EntryNames(self.sc, self.db, [b"one", b"two", b"three"], [b"", b"a definition", b""])
        found = self.sc.scan_tensor(self.db)
        m = min(7, int(found.shape[0]))
        assert m >= 3
        few = found[:m].contiguous()
        idx = torch.arange(N, device=DEV) % m
        self.rows = few[idx].contiguous()
        text_len, text_bytes = columns([b"%8.3f" % (k - 2.5) for k in range(m)], WIDTH)
        self.scores = self._scores(torch.from_numpy(text_bytes).to(DEV)[idx].contiguous(), torch.from_numpy(text_len).to(DEV)[idx].contiguous())
        self.good = {call: self.run(call) for call in CALLS}
        torch.cuda.synchronize()
        # the rows' results are the few records' own, repeated: offsets that run on over the seam
        s = self._scores(torch.from_numpy(text_bytes).to(DEV), torch.from_numpy(text_len).to(DEV))
        for call in CALLS:
            one, big = self.run(call, few, s), self.good[call]
            lens = (one.off[1:] - one.off[:-1])[idx]
            assert int(big.off[0]) == 0 and torch.equal(big.off[1:], torch.cumsum(lens, 0)) and int(big.off[-1]) == self.total(call) > 0, call
        self.words = " ".join(self.d.names()).encode()
        self.buf = ctypes.create_string_buffer(1024)

    @staticmethod
    def _scores(text_bytes, text_len):
        n = int(text_len.shape[0])
        return R.HitScores(torch.ones(n, dtype=torch.bool, device=DEV), torch.zeros(n, dtype=torch.float64, device=DEV),
                           torch.zeros(n, dtype=torch.int8, device=DEV), text_bytes, text_len)

    def run(self, call, rows=None, scores=None):
        rows = self.rows if rows is None else rows
        scores = self.scores if scores is None else scores
        if call == "structures":
            return self.sc.hit_structures(self.db, rows)
        if call == "print":
            return self.sc.print_hits(self.db, rows, scores, names=self.names)
        return self.sc.ct_hits(self.db, rows, scores, names=self.names, type="rnaviz")

    @staticmethod
    def tensors(call, r):
        return (r.off, r.lo, r.base, r.elem, r.mate) if call == "structures" else (r.bytes, r.off)

    def total(self, call):
        return int(self.good[call].off[-1])

    def fill(self, call, total, rows=None, text_len=None):
        """the fill call itself, its outputs prefilled with a sentinel: (rc, the words, the outputs untouched)"""
        rows = self.rows if rows is None else rows
        s = self.scores
        tl = s.text_len if text_len is None else text_len
        room = self.total(call) + 64
        L = R.lib()
        if call == "structures":
            out = (torch.full((N + 1,), -77, dtype=torch.int64, device=DEV), torch.full((N,), -77, dtype=torch.int32, device=DEV),
                   torch.full((room,), 77, dtype=torch.uint8, device=DEV), torch.full((room,), -77, dtype=torch.int16, device=DEV),
                   torch.full((room, 3), -77, dtype=torch.int32, device=DEV))
        else:
            out = (torch.full((room,), 77, dtype=torch.uint8, device=DEV), torch.full((N + 9,), -77, dtype=torch.int64, device=DEV))
        torch.cuda.synchronize()
        if call == "structures":
            rc = L.rma_hit_structures(self.sc._h, self.db._h, rows.data_ptr(), N, None, total, *[t.data_ptr() for t in out], None, self.buf, 1024)
        elif call == "print":
            rc = L.rma_hit_print(self.sc._h, self.db._h, self.names._h, rows.data_ptr(), N, None, s.accept.data_ptr(), s.text_bytes.data_ptr(), WIDTH,
                                 tl.data_ptr(), total, out[0].data_ptr(), out[1].data_ptr(), None, self.buf, 1024)
        else:
            rc = L.rma_hit_ct(self.sc._h, self.db._h, self.names._h, rows.data_ptr(), N, s.accept.data_ptr(), s.text_bytes.data_ptr(), WIDTH,
                              tl.data_ptr(), 1, self.words, None, total, out[0].data_ptr(), out[1].data_ptr(), None, self.buf, 1024)
        torch.cuda.synchronize()
        self.filled = out
        return rc, self.buf.value.decode(), all(bool((t == (77 if t.dtype == torch.uint8 else -77)).all()) for t in out)

    def filled_as_before(self, call):
        """the last fill call's outputs: what the scanner made before, the room behind it at its sentinel"""
        for got, want in zip(self.filled, self.tensors(call, self.good[call])):
            m = int(want.shape[0])
            if not torch.equal(got[:m], want) or not bool((got[m:] == (77 if got.dtype == torch.uint8 else -77)).all()):
                return False
        return True

    def as_before(self, call):
        """the same scanner on the unmodified rows, right behind a refusal"""
        again = self.run(call)
        torch.cuda.synchronize()
        return all(torch.equal(a, b) for a, b in zip(self.tensors(call, again), self.tensors(call, self.good[call])))

    def close(self):
        self.names.close()
        self.db.close()
        self.sc.close()


@pytest.fixture(scope="module")
def seam(built, tmp_path_factory):
    f = Seam(tmp_path_factory.mktemp("seam"))
    yield f
    f.close()


@pytest.mark.parametrize("call", CALLS)
def test_malformed_row_in_the_second_chunk(seam, call):
    n_seq = len(SEQS)
    bad = seam.rows.clone()
    bad[CHUNK + 1, 0] = n_seq
    words = r"record %d: entry %d outside \[0, %d\): %s$" % (CHUNK + 1, n_seq, n_seq, NOTHING[call])
    with pytest.raises(R.RnamotifError, match=words):
        seam.run(call, bad)
    assert seam.as_before(call)
    rc, said, untouched = seam.fill(call, seam.total(call), rows=bad)
    assert rc == 1 and re.search(words, said) and untouched, said
    assert seam.as_before(call)


@pytest.mark.parametrize("call", CALLS)
def test_wrong_total(seam, call):
    total = seam.total(call)
    rc, said, untouched = seam.fill(call, total + 1)
    words = "%s of the %d records have %d bytes, not the %d of `total`: %s" % (NOUN[call], N, total, total + 1, NOTHING[call])
    assert rc == 1 and said.endswith(words) and untouched, said
    assert seam.as_before(call)
    rc, said, untouched = seam.fill(call, total)
    assert rc == 0 and not untouched and seam.filled_as_before(call), said


@pytest.mark.parametrize("call", ("print", "ct"))
def test_text_length_outside_its_row(seam, call):
    lens = seam.scores.text_len.clone()
    lens[CHUNK + 2] = WIDTH + 1
    rc, said, untouched = seam.fill(call, seam.total(call), text_len=lens)
    words = r"record %d: a score column of %d bytes, outside the \[0, %d\] of text_width: %s$" % (CHUNK + 2, WIDTH + 1, WIDTH, NOTHING[call])
    assert rc == 1 and re.search(words, said) and untouched, said
    assert seam.as_before(call)
    s = seam.scores
    with pytest.raises(R.RnamotifError, match=words):
        seam.run(call, scores=R.HitScores(s.accept, s.score, s.kind, s.text_bytes, lens))
    assert seam.as_before(call)
