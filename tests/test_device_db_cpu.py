"""CPU: how Scanner.database_from_tensor reads its input forms -- text_entries() turns a byte tensor and its
offsets / lengths into (start, slen) from the first byte of the tensor's storage -- and the table alphabet=
makes from the readers' letters (rma_letter_codes).  The device half is tests/test_device_db.py."""
import numpy as np
import pytest
import torch


def _entries(text, **kw):
    import rnamotif_amd as R
    start, slen = R.text_entries(text, **kw)
    assert start.dtype == np.int64 and slen.dtype == np.int32
    return start.tolist(), slen.tolist()


def test_offsets_and_lengths_agree():
    t = torch.arange(100, dtype=torch.uint8)
    assert _entries(t, offsets=[0, 3, 3, 10, 100]) == ([0, 3, 3, 10], [3, 0, 7, 90])
    assert _entries(t, lengths=[3, 0, 7, 90]) == ([0, 3, 3, 10], [3, 0, 7, 90])
    assert _entries(t, lengths=torch.tensor([3, 0, 7])) == ([0, 3, 3], [3, 0, 7])
    assert _entries(t) == ([0], [100])
    assert _entries(t, offsets=[5]) == ([], [])
    # a view: starts count from the storage's first byte
    v = t[17:60]
    assert _entries(v, offsets=np.array([0, 10, 43])) == ([17, 27], [10, 33])
    assert _entries(v, lengths=[40]) == ([17], [40])
    assert _entries(t.view(torch.int8)[1:], lengths=[2, 2]) == ([1, 3], [2, 2])


def test_rows_and_strides():
    big = torch.zeros((6, 50), dtype=torch.uint8)
    assert _entries(big) == ([0, 50, 100, 150, 200, 250], [50] * 6)
    assert _entries(big, lengths=[0, 1, 2, 3, 4, 50]) == ([0, 50, 100, 150, 200, 250], [0, 1, 2, 3, 4, 50])
    v = big[:, 5:5 + 20]
    assert _entries(v, lengths=[20, 0, 1, 19, 7, 3]) == ([5, 55, 105, 155, 205, 255], [20, 0, 1, 19, 7, 3])
    every_other = big[1::2, 10:30]
    assert _entries(every_other) == ([60, 160, 260], [20, 20, 20])
    assert _entries(torch.zeros((0, 8), dtype=torch.uint8)) == ([], [])
    # (a row of one byte has no inner stride to speak of)
    assert _entries(big[:, 3:4]) == ([3, 53, 103, 153, 203, 253], [1] * 6)


@pytest.mark.parametrize("make,kw,words", [
    (lambda: torch.zeros(10, dtype=torch.int32), {}, "uint8 or int8"),
    (lambda: torch.zeros(10, dtype=torch.float32), {}, "uint8 or int8"),
    (lambda: torch.zeros((2, 2, 2), dtype=torch.uint8), {}, "3 dimensions"),
    (lambda: torch.zeros(20, dtype=torch.uint8)[::2], {}, "stride 2"),
    (lambda: torch.zeros((8, 8), dtype=torch.uint8).t(), {}, "inner stride 8"),
    (lambda: torch.zeros(10, dtype=torch.uint8), {"offsets": [0, 11]}, "inside the text's 10 bytes"),
    (lambda: torch.zeros(10, dtype=torch.uint8), {"offsets": [0, 6, 4]}, "ascending"),
    (lambda: torch.zeros(10, dtype=torch.uint8), {"offsets": [-1, 4]}, "ascending"),
    (lambda: torch.zeros(10, dtype=torch.uint8), {"offsets": []}, "n\\+1 values"),
    (lambda: torch.zeros(10, dtype=torch.uint8), {"lengths": [6, 5]}, "11 bytes in all"),
    (lambda: torch.zeros(10, dtype=torch.uint8), {"lengths": [6, -1]}, "non-negative"),
    (lambda: torch.zeros(10, dtype=torch.uint8), {"lengths": [1], "offsets": [0, 1]}, "not both"),
    (lambda: torch.zeros(10, dtype=torch.uint8), {"lengths": [[1, 2]]}, "1-D sequence of integers"),
    (lambda: torch.zeros(10, dtype=torch.uint8), {"lengths": [1.5]}, "1-D sequence of integers"),
    (lambda: torch.zeros((3, 4), dtype=torch.uint8), {"lengths": [1, 2]}, "one per row, 3, not 2"),
    (lambda: torch.zeros((3, 4), dtype=torch.uint8), {"lengths": [1, 5, 2]}, "0 to the row length 4"),
    (lambda: torch.zeros((3, 4), dtype=torch.uint8), {"lengths": [1, -1, 2]}, "0 to the row length 4"),
    (lambda: torch.zeros((3, 4), dtype=torch.uint8), {"offsets": [0, 4]}, "per-row lengths"),
])
def test_input_form_errors(make, kw, words):
    import rnamotif_amd as R
    with pytest.raises((TypeError, ValueError), match=words):
        R.text_entries(make(), **kw)


def test_not_a_tensor():
    import rnamotif_amd as R
    with pytest.raises(TypeError, match="not a torch.Tensor"):
        R.text_entries(b"acgt")


def test_letter_table_and_alphabet(built):
    import ctypes
    import rnamotif_amd as R
    buf = ctypes.create_string_buffer(256)
    R.lib().rma_letter_codes(buf)
    lut = buf.raw
    want = {ord(c): v for c, v in zip("acgtuACGTU", [0, 1, 2, 3, 3, 0, 1, 2, 3, 3])}
    assert all(lut[b] == want.get(b, 4) for b in range(256))
    tab = R.alphabet_table("acgu")
    assert tab[:4] == bytes([0, 1, 2, 3]) and tab[4:] == bytes([4] * 252)
    tab = R.alphabet_table("NACGT")
    assert tab[:5] == bytes([4, 0, 1, 2, 3])
    assert R.alphabet_table("".join(chr(c) for c in range(256))) == lut


@pytest.mark.parametrize("bad", ["", "x" * 257, "acĀ", 5, None, b"acgt"])
def test_bad_alphabet(built, bad):
    import rnamotif_amd as R
    with pytest.raises(ValueError, match="alphabet"):
        R.alphabet_table(bad)
