"""GPU: the four score kernels of rm_score_dev.hip (rma_score_kernel, ..._text_, ..._match_, ..._match_text_) on the programs of
tests/score_programs.py, against the rule of rm_score_core.h run on the host through the checkers (which
tests/test_score_programs_cpu.py holds to ScoreVM::run and HitPrinter::print on the same programs):

  * sized( family, waves ): every kernel in workgroups of 4, 3, 2 and 1 waves -- info() says so -- over 0, 1, 63, 64, 65 and
    2^17 + 1 rows; the text kernels with score_heap at its default and the score column of every row;
  * limits() that open, and the element stack's edge: the deepest stack, 64 variables, a wave that just fits LDS (by its stack
    and by its matcher's frames), 4096 instructions, a full string pool, 64 pair sets, 32 expressions;
  * the first 40 seeds a family whose records all run through: accept, kind, the bits of SCORE and, in the text kernels, the
    length and every byte of the score column equal the checker's rows;
  * the first 6 seeds a family with a stopped record: the call fails naming the first one with the checker's words and leaves
    the outputs, prefilled, as they were; the records in front of it are judged as the rule judges them.

One scanner, database and scan per descriptor (HP; CTX with -context) serve the module: the records are the descriptor's,
whatever its score section, and so is the program a ScoreProgram is compared by.  torch is imported before the product library:
one HIP runtime serves the process."""
import ctypes as C

import torch  # noqa: F401  (first: its HIP runtime is the process's)

import numpy as np
import pytest

import rnamotif_amd as R
import score_programs as SP
from test_score_device_cpu import CTX, HP, entries_of
from test_score_programs_cpu import ESTK, LIMITS, checkers  # noqa: F401
from test_score_text import DEV, _open, _raw_call, _sentinels, _untouched

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

W = SP.W
N_RUN, N_STOP = 40, 6


@pytest.fixture(scope="module")
def world(built, gbrna, tmp_path_factory):
    """uses -context? -> the scanner, the database and the scan's records of the first 30 entries"""
    tmp = tmp_path_factory.mktemp("score_programs_gpu")
    seqs = entries_of(gbrna, 30)
    out = {}
    for ctx, base, extra in ((False, HP, []), (True, CTX, ["-context"])):
        d = R.Descriptor(extra + ["-descr", SP.write_descr(base + "\t{ SCORE = 1; }\n", tmp, "scan%d" % ctx)])
        sc, db, hits = _open(d, seqs)
        recs = hits.cpu().numpy()
        assert len(recs) > 1000 and (recs[:, 1] == 0).sum() > 100 and (recs[:, 1] == 1).sum() > 100
        out[ctx] = {"sc": sc, "db": db, "hits": hits, "recs": recs, "seqs": seqs, "tmp": tmp}
    yield out
    for w in out.values():
        w["db"].close()
        w["sc"].close()


class Case:
    """a program opened for its family's kernel, and the checker's rows for the world's records"""
    def __init__(self, world, checker, family, text, extra, name):
        self.w = world[bool(extra)]
        self.family, self.text = family, bool(SP.FLAGS[family] & 2)
        self.argv = list(extra) + ["-descr", SP.write_descr(text, self.w["tmp"], name)]
        refused, self.image, self.rows, status, out = SP.run_family(checker, family, self.w["tmp"], self.argv, self.w["seqs"], self.w["recs"])
        assert refused is None and status == 0 and len(self.rows) == len(self.w["recs"]), (refused, out[-300:])
        self.stopped = [k for k, r in enumerate(self.rows) if r[0] == "S"]
        self.prog = None

    def open(self):
        self.prog = R.ScoreProgram(R.Descriptor(self.argv), text=self.text, match=bool(SP.FLAGS[self.family] & 8))
        info = self.prog.info()
        assert info["waves_per_workgroup"] == SP.waves_of(self.image) and info["workgroup_lds_bytes"] <= 65536 and info["private_bytes"] == 0, info
        return info

    def close(self):
        if self.prog is not None:
            self.prog.close()

    def want(self, idx):
        rows = [self.rows[i] for i in idx]
        acc = np.array([r[0] == "A" for r in rows], dtype=bool)
        bits = np.array([r[2] for r in rows], dtype=np.uint64)
        kind = np.array([r[1] for r in rows], dtype=np.int8)
        tl = np.array([len(r[4]) for r in rows], dtype=np.int32)
        tb = np.zeros((len(rows), W), dtype=np.uint8)
        for k, r in enumerate(rows):
            tb[k, :len(r[4])] = np.frombuffer(r[4], dtype=np.uint8)
        return acc, bits, kind, tl, tb

    def equal(self, idx):
        """Scanner.score of these rows of the scan's records against the checker's rows of them, bit for bit"""
        idx = np.asarray(idx, dtype=np.int64)
        at = torch.as_tensor(idx, dtype=torch.int64, device=DEV)
        s = self.w["sc"].score(self.w["db"], self.w["hits"][at], self.prog, text=self.text, text_width=W)
        torch.cuda.synchronize()
        acc, bits, kind, tl, tb = self.want(idx)
        assert np.array_equal(s.accept.cpu().numpy(), acc) and np.array_equal(s.kind.cpu().numpy(), kind)
        assert np.array_equal(s.score.cpu().numpy().view(np.uint64), bits)
        if self.text:
            assert np.array_equal(s.text_len.cpu().numpy(), tl) and np.array_equal(s.text_bytes.cpu().numpy(), tb)      # (zeros behind the length: not written)
        return acc


@pytest.mark.parametrize("waves", [4, 3, 2, 1])
@pytest.mark.parametrize("family", SP.FAMILIES)
def test_every_kernel_in_every_workgroup_shape(world, checkers, family, waves):
    c = Case(world, checkers[family], family, SP.sized(family, waves), [], "sized")
    info = c.open()
    print(family, waves, info)
    assert info["waves_per_workgroup"] == waves and not c.stopped
    n = len(c.rows)
    acc = c.equal(np.arange(n))
    assert acc.sum() >= 100 and (~acc).sum() >= 100
    for k in (0, 1, 63, 64, 65):
        c.equal(np.arange(k) + 5)
    c.equal((np.arange((1 << 17) + 1) * 7 + 3) % n)
    c.close()


RUNNING = [x for x in LIMITS if x[3] is None]


@pytest.mark.parametrize("k", range(len(RUNNING)), ids=[x[0] for x in RUNNING])
def test_programs_at_the_limits(world, checkers, k):
    name, family, text, _, want = RUNNING[k]
    c = Case(world, checkers[family], family, text, [], "limit")
    info = c.open()
    print(name, info)
    for key, v in want.items():
        assert c.image[key] == v
    n = len(c.rows)
    acc = c.equal(np.arange(n))
    assert not c.stopped and acc.sum() >= 100 and (~acc).sum() >= 100
    c.equal((np.arange(257) * 11 + 1) % n)
    c.close()


def _fails_at_the_first_stop(c):
    """the call fails naming the first stopped record with the checker's words, nothing is written, the rows in front of it run"""
    w, first, n = c.w, c.stopped[0], len(c.rows)
    if c.text:
        sent = _sentinels(n, W)
        rc, said = _raw_call(w["sc"], c.prog, w["db"], w["hits"], sent, stride=W)
        who = "rma_score_hits_text"
        untouched = _untouched(sent)
    else:
        sent = (torch.full((n,), 7, dtype=torch.uint8, device=DEV), torch.full((n,), -12.5, dtype=torch.float64, device=DEV),
                torch.full((n,), 9, dtype=torch.int8, device=DEV))
        err = C.create_string_buffer(4096)
        rc = R.lib().rma_score_hits(w["sc"]._h, c.prog._h, w["db"]._h, w["hits"].data_ptr(), n, None, sent[0].data_ptr(), sent[1].data_ptr(), sent[2].data_ptr(),
                                    torch.cuda.current_stream(DEV).cuda_stream, err, 4096)
        torch.cuda.synchronize()
        said, who = err.value.decode(), "rma_score_hits"
        untouched = bool((sent[0] == 7).all()) and bool((sent[1] == -12.5).all()) and bool((sent[2] == 9).all())
    assert rc != 0 and said.startswith("%s: record %d: " % (who, first)) and c.rows[first][5] in said and "nothing written" in said, (said, c.rows[first])
    assert untouched
    c.equal(np.arange(first))


@pytest.mark.parametrize("k", range(len(ESTK)), ids=[x[0] for x in ESTK])
def test_the_element_stack_at_its_edge(world, checkers, k):
    name, text, stops = ESTK[k]
    c = Case(world, checkers["plain"], "plain", text, [], "estk")
    c.open()
    assert bool(c.stopped) == stops
    if stops:
        assert c.rows[0][5].endswith("element stack overflow.")
        _fails_at_the_first_stop(c)
    else:
        acc = c.equal(np.arange(len(c.rows)))
        assert acc.any() and not acc.all()
    c.close()


_chosen = {}


def chosen(world, checkers, family):  # noqa: F811
    """(the first N_RUN seeds of the family without a stopped record, the first N_STOP with one), each as a Case"""
    if family not in _chosen:
        run, stop, seed = [], [], 0
        while (len(run) < N_RUN or len(stop) < N_STOP) and seed < 400:
            text, extra, _ = SP.generate(seed, family, seed % 4)
            c = Case(world, checkers[family], family, text, extra, "seed")
            c.seed = seed
            if c.stopped and len(stop) < N_STOP:
                stop.append(c)
            elif not c.stopped and len(run) < N_RUN:
                run.append(c)
            seed += 1
        assert len(run) == N_RUN and len(stop) == N_STOP
        _chosen[family] = (run, stop)
    return _chosen[family]


def _reopen(c, name):
    """the checker's words name the descriptor file: the program is opened from the one the checker read, written again"""
    text = SP.generate(c.seed, c.family, c.seed % 4)[0]
    assert c.argv[-1] == SP.write_descr(text, c.w["tmp"], "seed")
    return c.open()


@pytest.mark.parametrize("k", range(N_RUN))
@pytest.mark.parametrize("family", SP.FAMILIES)
def test_generated_programs(world, checkers, family, k):
    c = chosen(world, checkers, family)[0][k]
    info = _reopen(c, "seed")
    acc = c.equal(np.arange(len(c.rows)))
    print("%s seed %d: %d waves, %d of %d records accepted" % (family, c.seed, info["waves_per_workgroup"], acc.sum(), len(acc)))
    c.close()


@pytest.mark.parametrize("k", range(N_STOP))
@pytest.mark.parametrize("family", SP.FAMILIES)
def test_generated_programs_that_stop(world, checkers, family, k):
    c = chosen(world, checkers, family)[1][k]
    _reopen(c, "seed")
    print("%s seed %d: record %d of %d stops: %s" % (family, c.seed, c.stopped[0], len(c.rows), c.rows[c.stopped[0]][5]))
    _fails_at_the_first_stop(c)
    c.close()
