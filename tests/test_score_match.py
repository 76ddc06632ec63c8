"""GPU: the score section with =~, !~ and mismatches( string, pattern ) on the device (Scanner.score with
ScoreProgram(d, match=True): rma_score_match_kernel and rma_score_match_text_kernel of rm_score_dev.hip) against the same
rule, rm_score_core.h, run on the host through tests/hostsim/score_match_check.cpp (which tests/test_score_match_cpu.py
holds to ScoreVM::run, re_step() and re_mm_step()), and against the host replay:

  * six own descriptors of tests/test_score_match_cpu.py -- a plain one, one with text, a back reference, a loop,
    mismatches(), a loose descriptor through seq_check and checked=True -- on the records of the GPU scan of the first 30
    entries of the reference's test database: accept, kind and the bits of the score (with text: the column and its
    length) equal the checker's lines, and hits[accept] are the records Replay.device(..., accepted=True) prints;
  * record counts at the seams of a wave, a workgroup and a chunk of the call;
  * a program whose planes leave room for fewer than four waves, with a pattern of nine repeating ops;
  * a record over its budget fails the call and leaves the outputs as they were;
  * programs opened without the flag run the kernels they ran, with the registers and LDS they had at the parent commit.

torch is imported before the product library: one HIP runtime serves the process."""
import ctypes as C
import json
import os

import torch  # noqa: F401  (first: its HIP runtime is the process's)

import numpy as np
import pytest

import rnamotif_amd as R
from test_score_device_cpu import GOLDEN, HP, ROOT, entries_of, own_args
from test_score_match_cpu import BUDGET, CHECKED, MATCH, OWN_MATCH, OWN_MISMATCHES, TEXT, match_checker, run_match_checker  # noqa: F401
from test_score_text import DEV, W, _equal, _expected, _open, _scored

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

CASES = {
    "anchored": OWN_MATCH["anchored"],
    "a + b": OWN_MATCH["a + b"],
    "back reference": OWN_MATCH["back reference"],
    "in a loop": OWN_MATCH["in a loop"],
    "mismatches": (OWN_MISMATCHES["with a star"][0], None, False),
    "a loose descriptor": OWN_MATCH["a loose descriptor"],
}
FIXTURE = os.path.join(GOLDEN, "score_match", "parent_kernel_attributes.json")
KEYS = ("registers", "private_bytes", "static_lds_bytes", "waves_per_workgroup", "workgroup_lds_bytes")


def _numbers(s):
    torch.cuda.synchronize()
    return s.accept.cpu().numpy(), s.score.cpu().numpy().view(np.uint64), s.kind.cpu().numpy()


def _numbers_equal(got, want, idx=None):
    idx = np.arange(len(got[0])) if idx is None else idx
    assert np.array_equal(got[0], want[0][idx]) and np.array_equal(got[1], want[1][idx]) and np.array_equal(got[2], want[2][idx])


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_against_rule_and_replay(built, match_checker, gbrna, tmp_path, name):
    text, rejects, needs_text = CASES[name]
    loose = name == "a loose descriptor"
    argv = own_args(text, tmp_path, name)
    d = R.Descriptor(argv)
    seqs = entries_of(gbrna, 30)
    sc, db, hits = _open(d, seqs)
    prog = R.ScoreProgram(d, checked=loose, text=needs_text, match=True)
    info = prog.info()
    assert prog.match and info["private_bytes"] == 0 and info["waves_per_workgroup"] == 4, info
    rows_in, at = hits, np.arange(hits.shape[0])
    if loose:
        assert d.loose > 0
        r = sc.seq_check(db, hits)
        at = np.flatnonzero(r.keep.cpu().numpy())
        rows_in = r.hits[r.keep].contiguous()
        assert 0 < len(at) < hits.shape[0]
    recs = rows_in.cpu().numpy()
    flags = MATCH | (TEXT if needs_text else 0) | (CHECKED if loose else 0)
    refused, image, rows, status, out, vm = run_match_checker(match_checker, tmp_path, argv, seqs, recs, flags, stride=W if needs_text else 0)
    assert refused is None and status == 0 and len(rows) == len(recs) > 1000
    want = _expected(rows)
    if needs_text:
        got = _scored(sc, db, rows_in, prog)
        _equal(got, want)
        acc = got[1]
    else:
        got = _numbers(sc.score(db, rows_in, prog))
        _numbers_equal(got, want)
        acc = got[0]
    print("%s: %d records, %d accepted, %s" % (name, len(recs), acc.sum(), info))
    assert acc.any() and acc.all() == (rejects is None)
    # the records the host replay prints: for a loose descriptor it drops those that are no candidates itself
    rp = R.Replay(d, str(tmp_path / "replay.txt"))
    n, mask = rp.device(db, hits, accepted=True)
    rp.close()
    mask = np.asarray(mask.cpu() if hasattr(mask, "cpu") else mask, dtype=bool)
    mine = np.zeros(hits.shape[0], dtype=bool)
    mine[at[acc]] = True
    assert n == int(mine.sum()) and np.array_equal(mask, mine)
    prog.close()
    db.close()
    sc.close()


@pytest.fixture(scope="module")
def made(built, match_checker, gbrna, tmp_path_factory):
    """a program with matches of the record's own bases and of a string it makes, a mismatches() and a string SCORE"""
    tmp = tmp_path_factory.mktemp("score_match_rows")
    text = HP + ("\t{ s = ss( tag='l' ) + '-' + h5( tag='a', pos=1, len=2 ); if( s =~ \"^g.*-c\" ) REJECT; if( h5( tag='a' ) !~ \"\\(.\\).*\\1\" ) REJECT;\n"
                 "\t  SCORE = sprintf( '%s %d', s, mismatches( s, \"a*ga\" ) ); }\n")
    argv = own_args(text, tmp, "rows")
    d = R.Descriptor(argv)
    seqs = entries_of(gbrna, 30)
    sc, db, hits = _open(d, seqs)
    prog = R.ScoreProgram(d, text=True, match=True)
    recs = hits.cpu().numpy()
    refused, image, rows, status, out, vm = run_match_checker(match_checker, tmp, argv, seqs, recs, MATCH | TEXT, stride=W)
    assert refused is None and status == 0 and len(rows) == len(recs) > 1000 and image["expr"] == 3
    yield {"sc": sc, "db": db, "hits": hits, "prog": prog, "want": _expected(rows)}
    prog.close()
    db.close()
    sc.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, (1 << 17) + 2])
def test_record_counts_at_the_seams(made, n):
    """a wave, a workgroup of four, and 2^17 + 1 records, a chunk of the call and one more: every row as in the full batch"""
    n_hits = made["hits"].shape[0]
    idx = (np.arange(n) * 7 + 3) % n_hits
    at = torch.as_tensor(idx, dtype=torch.int64, device=DEV)
    s = made["sc"].score(made["db"], made["hits"][at], made["prog"], text=True, text_width=W)
    torch.cuda.synchronize()
    want = made["want"]
    assert want[0].any() and not want[0].all()
    assert np.array_equal(s.accept.cpu().numpy(), want[0][idx]) and np.array_equal(s.kind.cpu().numpy(), want[2][idx])
    assert np.array_equal(s.score.cpu().numpy().view(np.uint64), want[1][idx])
    wl = np.array([len(c) for c in want[3]], dtype=np.int32)
    wb = np.zeros((n_hits, W), dtype=np.uint8)
    for k, c in enumerate(want[3]):
        wb[k, :len(c)] = np.frombuffer(c, dtype=np.uint8)
    assert np.array_equal(s.text_len.cpu().numpy(), wl[idx]) and np.array_equal(s.text_bytes.cpu().numpy(), wb[idx])


def test_workgroups_of_fewer_than_four_waves(built, match_checker, gbrna, tmp_path):
    """19 variables and a pattern of nine repeating ops: a wave's planes and its matcher's 54 slots leave room for one or two"""
    names = ["v%d" % k for k in range(16)]
    text = HP + ("\t{ " + " ".join("%s = %d;" % (v, k) for k, v in enumerate(names)) + "\n"
                 "\t  s = ss( tag='l' ) + h5( tag='a' ); m = 0; if( s =~ \"^a*c*g*t*a*c*g*t*a*$\" ) m = 1;\n"
                 "\t  SCORE = m + 2 * ( " + " + ".join(names) + " ); }\n")
    argv = own_args(text, tmp_path, "few waves")
    d = R.Descriptor(argv)
    seqs = entries_of(gbrna, 30)
    sc, db, hits = _open(d, seqs)
    prog = R.ScoreProgram(d, text=True, match=True)
    info = prog.info()
    print(info)
    assert info["waves_per_workgroup"] in (1, 2), info
    recs = hits.cpu().numpy()
    refused, image, rows, status, out, vm = run_match_checker(match_checker, tmp_path, argv, seqs, recs, MATCH | TEXT, stride=0)
    assert refused is None and status == 0 and image["frames"] == 9 and info["workgroup_lds_bytes"] <= 64 * 1024
    got = _numbers(sc.score(db, hits, prog))
    _numbers_equal(got, _expected(rows))
    odd = (got[1].view(np.float64) % 2 == 1)
    assert len(recs) > 4 * 128 and odd.any() and not odd.all()
    prog.close()
    db.close()
    sc.close()


def test_a_record_over_its_budget_fails_the_call(built, match_checker, gbrna, tmp_path):
    argv = own_args(BUDGET, tmp_path, "budget")
    d = R.Descriptor(argv)
    seqs = entries_of(gbrna, 30)
    sc, db, hits = _open(d, seqs)
    prog = R.ScoreProgram(d, text=True, match=True)
    recs = hits.cpu().numpy()
    refused, image, rows, status, out, vm = run_match_checker(match_checker, tmp_path, argv, seqs, recs, MATCH | TEXT, stride=0, budget=100)
    first = next(k for k, r in enumerate(rows) if r[0] == "S")
    n = len(recs)
    sent = (torch.full((n,), 7, dtype=torch.uint8, device=DEV), torch.full((n,), -12.5, dtype=torch.float64, device=DEV),
            torch.full((n,), 9, dtype=torch.int8, device=DEV))
    sc.set_option("score_budget", 100)
    err = C.create_string_buffer(4096)
    rc = R.lib().rma_score_hits(sc._h, prog._h, db._h, hits.data_ptr(), n, None, sent[0].data_ptr(), sent[1].data_ptr(), sent[2].data_ptr(),
                                torch.cuda.current_stream(DEV).cuda_stream, err, 4096)
    torch.cuda.synchronize()
    said = err.value.decode()
    assert rc != 0 and said.startswith("rma_score_hits: record %d: " % first) and rows[first][5] in said, said
    assert "more than 100 instructions for one record (option score_budget)." in said and "nothing written" in said
    assert bool((sent[0] == 7).all()) and bool((sent[1] == -12.5).all()) and bool((sent[2] == 9).all())
    # the records in front of it are judged as the rule judges them, and with the budget back all of them are
    if first > 0:
        _numbers_equal(_numbers(sc.score(db, hits[:first], prog)), _expected(rows[:first]))
    sc.set_option("score_budget", 1 << 20)
    refused, image, rows, status, out, vm = run_match_checker(match_checker, tmp_path, argv, seqs, recs, MATCH | TEXT, stride=0)
    _numbers_equal(_numbers(sc.score(db, hits, prog)), _expected(rows))
    prog.close()
    db.close()
    sc.close()


def test_programs_without_the_flag_run_what_they_ran(built):
    """info() of ire.descr and trna.descr, plain and with text, against the values recorded from the parent commit on an
    MI355X (tests/golden/score_match/parent_kernel_attributes.json names the commit): the two kernels are not touched"""
    if not os.path.exists(FIXTURE):
        pytest.skip("tests/golden/score_match/parent_kernel_attributes.json, the parent commit's values, is absent")
    parent = json.load(open(FIXTURE))
    for name, path in (("ire", "test/ire.descr"), ("trna", "descr/trna.descr")):
        d = R.Descriptor(["-descr", os.path.join(GOLDEN, path)])
        for kind, text in (("plain", False), ("text", True)):
            want = parent["programs"][name][kind]
            if want is None:
                assert R.ScoreProgram.reason(d, text=text) is not None
                continue
            for match in (False, True):        # (neither has a pattern: the flag changes nothing)
                p = R.ScoreProgram(d, text=text, match=match)
                got = p.info()
                p.close()
                for k in KEYS:
                    assert got[k] == want[k], (parent["commit"], name, kind, match, k, got[k], want[k])
