"""CPU: the rule Scanner.database_from_fasta_tensor() reads FASTA text by (rnamotif_amd/csrc/rm_fasta_dev.h, shared by the
kernels of rm_fasta_dev.hip and the host) against the parallel reader, through tests/hostsim/fasta_index_check.cpp:

  * summarise -> scan -> apply over chunks of 1, 3, 7, 64 and FD_CHUNK bytes finds the entries FastaStream finds --
    the offset of every '>', the end of every definition line, the letters, lengths, names and definitions -- and
    refuses exactly the texts, at exactly the entry, that FastaStream hands to the serial reader;
  * the chunk summaries compose associatively;
  * the Python method refuses what is not FASTA bytes on the scanner's GPU, with words, before the C call."""
import os
import subprocess

import numpy as np
import pytest

from test_stream import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "rnamotif_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
CHUNKS = "1,3,7,64,0"       # (0: the kernels' own chunk size)
DEFAULT_LIM = 30000001      # what rma_pack_read makes of maxslen = 0


def _build(name, flags):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    srcs = [os.path.join(ROOT, "tests", "hostsim", "fasta_index_check.cpp")] + [os.path.join(H, f) for f in ("rm_fasta.cpp", "rm_pack.cpp", "rm_stream.cpp")]
    newest = max(os.path.getmtime(s) for s in srcs + [os.path.join(H, f) for f in ("rm_fasta_dev.h", "rm_stream.h", "rm_pack.h")])
    if not os.path.exists(out) or os.path.getmtime(out) < newest:
        subprocess.run(["g++", "-std=c++17", "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + H] + flags + ["-o", out] + srcs, check=True)
    return out


@pytest.fixture(scope="module")
def checker():
    return _build("fasta_index_check", ["-O2"])


def _run(binary, args, timeout=600):
    p = subprocess.run([binary] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert p.returncode == 0, (p.stdout + p.stderr).decode("utf-8", "replace")[-2000:]
    return p.stdout.decode()


def generated_texts(count=300, seed=20):
    """FASTA as files do not usually hold it: lines of any length from 1 up, CR-LF, '>' inside definition lines and in
    the middle of sequence lines, entries without letters, no newline at the end, digits and bytes of 128 and above
    among the letters; now and then what the readers refuse (an unnamed entry, a NUL in a definition line)."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGTUacgtunNrRyYkKmM", dtype=np.uint8)
    junk = np.frombuffer(b"0123456789 \t*-.\x00\x80\xff\xc3", dtype=np.uint8)
    out = []
    for t in range(count):
        eol = b"\r\n" if t % 5 == 1 else b"\n"
        parts = []
        for e in range(int(rng.integers(1, 9))):
            name = b"s%d_%d" % (t, e)
            kind = int(rng.integers(0, 40))
            if kind == 0:
                head = b">" + b" " * int(rng.integers(0, 3))                     # unnamed
            elif kind == 1:
                head = b">" + name + b" de\x00f"                                 # NUL in the definition
            elif kind < 10:
                head = b">" + name + b" one > two >three"                        # '>' in the definition line
            elif kind < 14:
                head = b">" + name                                               # no definition
            else:
                head = (b"> " if kind % 2 else b">") + name + b"\t a definition " + bytes(rng.integers(33, 127, size=int(rng.integers(0, 30)), dtype=np.uint8)).replace(b">", b"x")
            parts.append(head + eol)
            lines = int(rng.integers(0, 6))                                      # (0: an entry without letters)
            for _ in range(lines):
                n = int(rng.integers(1, 90))
                line = letters[rng.integers(0, letters.size, size=n)].copy()
                dirty = rng.random(n) < 0.05
                line[dirty] = junk[rng.integers(0, junk.size, size=int(dirty.sum()))]
                parts.append(line.tobytes() + eol)
                if rng.random() < 0.05:                                          # an entry begins in mid line
                    parts[-1] = parts[-1][: -len(eol)] + b">mid%d y" % t + eol
        text = b"".join(parts)
        if t % 4 == 2:
            text = text.rstrip(b"\r\n")                                          # no newline at the end
        out.append(text)
    return out


def _write(tmp, texts):
    paths = []
    for k, text in enumerate(texts):
        p = os.path.join(str(tmp), "t%04d.fa" % k)
        with open(p, "wb") as f:
            f.write(text)
        paths.append(p)
    return paths


def test_cases_of_the_reader_tests(checker, tmp_path):
    names = sorted(CASES)
    paths = _write(tmp_path, [CASES[n] for n in names])
    for lim in (DEFAULT_LIM, 4):         # (4: every entry of 4 letters or more is one the reader hands over)
        out = _run(checker, ["files", lim, CHUNKS] + paths)
        assert "%d files identical at 5 chunk sizes" % len(names) in out, out


def test_reference_database(checker, gbrna):
    out = _run(checker, ["files", DEFAULT_LIM, CHUNKS, gbrna])
    assert "1 files identical at 5 chunk sizes" in out, out


def test_generated_texts(checker, tmp_path):
    texts = generated_texts()
    assert sum(b"\r\n" in t for t in texts) > 20 and sum(not t.endswith(b"\n") for t in texts) > 20
    paths = _write(tmp_path, texts)
    out = _run(checker, ["files", DEFAULT_LIM, CHUNKS] + paths)
    assert "%d files identical at 5 chunk sizes" % len(texts) in out, out
    out = _run(checker, ["files", 60, "7,0"] + paths)
    assert "%d files identical at 2 chunk sizes" % len(texts) in out, out


def test_under_the_sanitizers(tmp_path):
    san = _build("fasta_index_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    names = sorted(CASES)
    paths = _write(tmp_path, [CASES[n] for n in names] + generated_texts(count=60, seed=21))
    out = _run(san, ["files", DEFAULT_LIM, CHUNKS] + paths)
    assert "%d files identical" % len(paths) in out, out
    assert "triples associative" in _run(san, ["compose", 2000, 3])


def test_summaries_compose_associatively(checker):
    assert "200000 triples associative" in _run(checker, ["compose", 200000, 1])


def test_constants_are_exported(built):
    import rnamotif_amd as R
    chunk, block, cap = R.fasta_device_shape()
    text = open(os.path.join(H, "rm_fasta_dev.h")).read()
    assert "FD_CHUNK = %d;" % chunk in text and "FD_SCAN_BLOCK = %d;" % block in text
    assert chunk % 1024 == 0 and cap > 20000


def test_header_declares_the_route():
    text = open(os.path.join(ROOT, "include", "rnamotif_amd.h")).read()
    assert "int\trma_db_create_device_fasta( rma_scanner_t *sc, const void *text, int64_t text_bytes, int32_t maxslen," in text
    assert "int\trma_db_entry_name( const rma_db_t *db, int32_t i, const char **sid, const char **sdef );" in text
    assert "synchronises" in text


class _FakeScanner:
    """database_from_fasta_tensor's checks run before anything of the scanner but its device is touched."""
    device = 0
    _h = None


def test_python_refusals(built):
    import torch
    import rnamotif_amd as R
    f = R.Scanner.database_from_fasta_tensor
    sc = _FakeScanner()
    with pytest.raises(TypeError, match="not a torch.Tensor"):
        f(sc, b">a\nACGT\n")
    with pytest.raises(TypeError, match="uint8 or int8"):
        f(sc, torch.zeros(8, dtype=torch.int32))
    with pytest.raises(ValueError, match="2 dimensions"):
        f(sc, torch.zeros((2, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="stride 2"):
        f(sc, torch.zeros(8, dtype=torch.uint8)[::2])
    with pytest.raises(ValueError, match="is on cpu"):
        f(sc, torch.zeros(8, dtype=torch.uint8))
