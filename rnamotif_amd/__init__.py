"""rnamotif_amd -- MI355X-native scan path of rnamotif behind a C ABI.

Thin ctypes mirror of include/rnamotif_amd.h.  The work is done by
``librnamotif_amd.so`` (host front end in C++, search and efn kernels in HIP for
gfx950); this module only moves pointers.  There is no CPU implementation of the
scan in this package: if the library is missing or no GPU is usable the calls
fail loudly.

Reference boundary (see the header for the full table):
  rma_descr_compile  <- RM_init/yyparse/SE_link/RM_linkscore (rnamot.c:49-98)
  rma_scanner_create <- RM_fm_init (find_motif.c:109)
  rma_scan           <- RM_find_motif (find_motif.c:164), both strands
  rma_replay_*       <- RM_score + print_match (score.c:608, find_motif.c:1826)
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RNAMOTIF_AMD_LIB") or os.path.join(_HERE, "librnamotif_amd.so")    # (the variable: build variants, profiles/variants.sh)
EFNDATA_DIR = os.path.join(_HERE, "efndata")
CLI_PATH = os.path.join(_HERE, "bin", "rnamotif")

RMA_HIT_HDR = 5
_ERRLEN = 4096

# The bits of Scanner.set_option("dbg", ...) and RNAMOTIF_DBG: RMK_DBG_* of csrc/rm_diag.h, which says what each does
# (tests/test_diag_names.py holds the two together).
DBG = {
    # path selectors
    "GENERAL": 16, "POOL_DROP": 2048, "WHOLE_ITEMS": 2097152, "NO_FORKS": 4194304, "LIST_ALL": 8388608,
    # ablation switches
    "NO_PASS_B": 1, "NO_BITPAR": 4, "NO_LITERAL": 8, "NO_ROWS": 64, "NO_VOTE": 128, "NO_SPLIT": 256,
    "NO_STEP_CHAIN": 512, "NO_HEAD_TEST": 4096, "NO_Q1_FILTER": 8192, "NO_TRI_FILTER": 16384, "NO_CHAIN": 32768,
    "STOP_ROWS": 65536, "STOP_CHAIN": 131072, "NO_HEAD_NEXT": 262144, "NO_START_VEC": 33554432,
    "TICKET_PER_TILE": 67108864, "HEAD_ALL_ENDS": 134217728, "DRAIN_DROP": 268435456,
    # instrumentation
    "COUNT_QUEUED": 2, "CYCLES": 32, "TIMELINE": 1048576, "DRAIN_DONE": 536870912,
}


class RnamotifError(RuntimeError):
    pass


_lib = None


def lib() -> C.CDLL:
    """Load librnamotif_amd.so (built in-tree by __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RnamotifError(
            f"{LIB_PATH} is missing: build it with `make -C rnamotif_amd/csrc` "
            "(hipcc --offload-arch=gfx950); there is no fallback implementation")
    L = C.CDLL(LIB_PATH)
    vp, i32p, i64p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    cpp = C.POINTER(C.c_char_p)
    L.rma_version.restype = C.c_char_p
    L.rma_device_count.restype = C.c_int
    L.rma_descr_compile.argtypes = [C.c_int, cpp, C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.rma_descr_free.argtypes = [vp]
    L.rma_descr_program.argtypes = [vp]
    L.rma_descr_program.restype = vp
    L.rma_descr_efndata.argtypes = [vp]
    L.rma_descr_efn2data.argtypes = [vp]
    L.rma_descr_efn2data.restype = vp
    L.rma_scanner_set_efn2data.argtypes = [vp, vp, C.c_char_p, C.c_size_t]
    L.rma_descr_efndata.restype = vp
    L.rma_descr_minlen.argtypes = [vp]
    L.rma_descr_maxlen.argtypes = [vp]
    L.rma_program_info.argtypes = [vp, i32p]
    L.rma_program_info.restype = None
    L.rma_scanner_create.argtypes = [vp, vp, C.c_int, C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.rma_scanner_destroy.argtypes = [vp]
    L.rma_scanner_set_option.argtypes = [vp, C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]
    L.rma_scanner_warmup.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.rma_db_attach.argtypes = [vp, vp, C.c_char_p, C.c_size_t]
    L.rma_db_wait.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.rma_db_create_packed_async.argtypes = [vp, vp, C.c_int32, C.c_int32, C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.rma_pack_pin.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.rma_scan_begin.argtypes = [vp, vp, C.c_char_p, C.c_size_t]
    L.rma_scan_end.argtypes = [vp, C.POINTER(i32p), i64p, C.c_char_p, C.c_size_t]
    L.rma_scan_end_on_device.argtypes = [vp, C.POINTER(vp), i64p, C.c_char_p, C.c_size_t]
    L.rma_comm_unique_id.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.rma_comm_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.rma_comm_destroy.argtypes = [vp]
    L.rma_comm_create_on.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.rma_comm_count.argtypes = [vp, C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
    L.rma_gather_hits.argtypes = [vp, vp, i32p, C.c_int32, C.c_int, C.POINTER(i32p), i64p, i64p, C.c_char_p, C.c_size_t]
    L.rma_db_create.argtypes = [vp, cpp, i32p, C.c_int32, C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.rma_db_destroy.argtypes = [vp]
    L.rma_db_create_ranges.argtypes = [vp, cpp, i32p, i32p, i32p, C.c_int32, C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.rma_db_create_packed.argtypes = [vp, vp, C.c_int32, C.c_int32, C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.rma_pack_write.argtypes = [C.c_char_p, cpp, cpp, cpp, i32p, C.c_int32, C.c_char_p, C.c_size_t]
    L.rma_pack_read.argtypes = [cpp, C.c_int32, C.c_char_p, C.c_int32, C.c_int32, C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.rma_database_index.argtypes = [cpp, C.c_int32, C.c_char_p, C.c_int32, C.POINTER(i64p), i32p, C.c_char_p, C.c_size_t]
    L.rma_pack_read_entries.argtypes = [cpp, C.c_int32, C.c_char_p, C.c_int32, C.c_int32, i32p, C.c_int32, C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.rma_free.argtypes = [vp]
    L.rma_db_create_packed_ranges.argtypes = [vp, vp, i32p, i32p, i32p, C.c_int32, C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.rma_replay_pack.argtypes = [vp, vp, C.c_int32, i32p, C.c_int64, i64p, C.c_char_p, C.c_size_t]
    L.rma_sort_hits.argtypes = [i32p, C.c_int64, C.c_int32, i32p, C.c_char_p, C.c_size_t]
    L.rma_pack_open.argtypes = [C.c_char_p, C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.rma_pack_close.argtypes = [vp]
    L.rma_pack_count.argtypes = [vp]
    L.rma_pack_count.restype = C.c_int32
    L.rma_pack_bases.argtypes = [vp]
    L.rma_pack_bases.restype = C.c_int64
    L.rma_pack_sid.argtypes = [vp, C.c_int32]
    L.rma_pack_sid.restype = vp
    L.rma_pack_sdef.argtypes = [vp, C.c_int32]
    L.rma_pack_sdef.restype = vp
    L.rma_pack_slen.argtypes = [vp, C.c_int32]
    L.rma_pack_slen.restype = C.c_int32
    L.rma_pack_seq.argtypes = [vp, C.c_int32, C.c_char_p]
    L.rma_db_bases.argtypes = [vp]
    L.rma_db_bases.restype = C.c_int64
    L.rma_scan.argtypes = [vp, vp, C.POINTER(i32p), i64p, C.c_char_p, C.c_size_t]
    L.rma_scanner_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float), C.c_char_p, C.c_size_t]
    if hasattr(L, "rma_scanner_last_launch"):       # (RNAMOTIF_AMD_LIB may name a build from before the call: comparisons in turns)
        L.rma_scanner_last_launch.argtypes = [vp, C.POINTER(C.c_int)]
    if hasattr(L, "rma_scanner_last_end"):
        L.rma_scanner_last_end.argtypes = [vp, C.POINTER(C.c_int)]
    L.rma_scan_device.argtypes = [vp, vp, i64p, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                  C.c_char_p, C.c_size_t]
    L.rma_replay_open.argtypes = [vp, C.c_char_p, C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.rma_replay_batch.argtypes = [vp, cpp, cpp, cpp, i32p, C.c_int32, i32p, C.c_int64, i64p,
                                   C.c_char_p, C.c_size_t]
    L.rma_replay_close.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.rma_db_create_device.argtypes = [vp, vp, C.c_int64, i64p, i32p, i32p, i32p, C.c_int32, C.c_char_p, vp,
                                       C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.rma_db_create_device_fasta.argtypes = [vp, vp, C.c_int64, C.c_int32, vp, C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.rma_db_entry_name.argtypes = [vp, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
    L.rma_db_entries.argtypes = [vp]
    L.rma_db_entries.restype = C.c_int32
    L.rma_fasta_device_shape.argtypes = [i32p]
    L.rma_fasta_device_shape.restype = None
    L.rma_letter_codes.argtypes = [C.c_char_p]
    L.rma_letter_codes.restype = None
    L.rma_db_mask_words.argtypes = [vp]
    L.rma_db_mask_words.restype = C.c_int64
    L.rma_db_read_packed.argtypes = [vp, vp, vp, vp, vp, C.c_char_p, C.c_size_t]
    L.rma_db_text_attach.argtypes = [vp, C.c_char_p, i64p, vp, C.c_char_p, C.c_size_t]
    L.rma_db_text_attach_pack.argtypes = [vp, vp, i32p, C.c_int32, vp, C.c_char_p, C.c_size_t]
    L.rma_db_read_text.argtypes = [vp, C.c_int32, C.c_char_p, C.c_char_p, C.c_size_t]
    L.rma_db_text_fill_ms.argtypes = [vp]
    L.rma_db_text_fill_ms.restype = C.c_float
    L.rma_scan_records_to_device.argtypes = [vp, vp, C.c_int64, vp, C.c_char_p, C.c_size_t]
    L.rma_replay_device.argtypes = [vp, vp, vp, C.c_int64, C.c_char_p, cpp, cpp, vp, i64p, vp, C.c_char_p, C.c_size_t]
    L.rma_hit_structures_size.argtypes = [vp, vp, vp, C.c_int64, vp, i64p, C.c_char_p, C.c_size_t]
    L.rma_hit_structures.argtypes = [vp, vp, vp, C.c_int64, C.c_char_p, C.c_int64, vp, vp, vp, vp, vp, vp, C.c_char_p, C.c_size_t]
    L.rma_hit_alignment_shape.argtypes = [vp, vp, vp, C.c_int64, i32p, i32p, vp, i64p, vp, C.c_char_p, C.c_size_t]
    L.rma_hit_alignment.argtypes = [vp, vp, vp, C.c_int64, i32p, C.c_char_p, C.c_char_p, vp, vp, vp, C.c_char_p, C.c_size_t]
    L.rma_descr_names.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.rma_descr_names.restype = C.c_size_t
    L.rma_prune_hits.argtypes = [vp, vp, vp, C.c_int64, i32p, vp, vp, C.c_char_p, C.c_size_t]
    L.rma_scanner_load_energy_tables.argtypes = [vp, C.c_char_p, C.c_int, C.c_char_p, C.c_size_t]
    L.rma_structure_energies.argtypes = [vp, vp, vp, vp, C.c_int32, C.c_int64, C.c_int64, C.c_char_p, vp, vp, vp, C.c_char_p, C.c_size_t]
    L.rma_score_open.argtypes = [vp, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
    L.rma_score_close.argtypes = [vp]
    L.rma_score_close.restype = None
    L.rma_score_info.argtypes = [vp, C.POINTER(C.c_int32)]
    L.rma_score_info.restype = None
    L.rma_score_hits.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_char_p, vp, vp, vp, vp, C.c_char_p, C.c_size_t]
    L.rma_score_open_checked.argtypes = [vp, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
    L.rma_score_open_flags.argtypes = [vp, C.c_uint, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
    L.rma_score_hits_text.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_char_p, vp, vp, vp, vp, C.c_int32, vp, vp, C.c_char_p, C.c_size_t]
    L.rma_seqcheck_open.argtypes = [vp, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
    L.rma_seqcheck_close.argtypes = [vp]
    L.rma_seqcheck_close.restype = None
    L.rma_seqcheck_info.argtypes = [vp, C.POINTER(C.c_int32)]
    L.rma_seqcheck_info.restype = None
    L.rma_seqcheck_hits.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_char_p, C.c_int32, vp, vp, vp, C.c_char_p, C.c_size_t]
    L.rma_program_loose.argtypes = [vp]
    L.rma_program_loose.restype = C.c_int
    L.rma_names_create.argtypes = [vp, vp, cpp, i64p, cpp, i64p, C.c_int32, C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.rma_names_destroy.argtypes = [vp]
    L.rma_names_destroy.restype = None
    L.rma_hit_print_size.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp, i64p, vp, C.c_char_p, C.c_size_t]
    L.rma_hit_print.argtypes = [vp, vp, vp, vp, C.c_int64, C.c_char_p, vp, vp, C.c_int32, vp, C.c_int64, vp, vp, vp, C.c_char_p, C.c_size_t]
    L.rma_hit_list_shape.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp, C.c_int32, vp, C.c_int32, C.c_int64, i64p, i64p,
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, C.c_char_p, C.c_size_t]
    L.rma_hit_list.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp, C.c_int32, vp, C.c_int32, C.c_int64, C.c_char_p, C.c_int64, C.c_int64,
                               vp, vp, vp, C.c_char_p, C.c_size_t]
    L.rma_print_header.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.rma_hit_ct_size.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp, C.c_int32, vp, C.c_int32, C.c_char_p, C.c_char_p, i64p, vp, C.c_char_p, C.c_size_t]
    L.rma_hit_ct.argtypes = [vp, vp, vp, vp, C.c_int64, vp, vp, C.c_int32, vp, C.c_int32, C.c_char_p, C.c_char_p, C.c_int64, vp, vp, vp,
                             C.c_char_p, C.c_size_t]
    _lib = L
    return L


def _check(rc: int, err) -> None:
    if rc != 0:
        raise RnamotifError(err.value.decode("utf-8", "replace").rstrip())


def fasta_device_shape() -> Tuple[int, int, int]:
    """(bytes per chunk, chunks per scan block, bytes of a definition line looked at) of database_from_fasta_tensor."""
    a = (C.c_int32 * 3)()
    lib().rma_fasta_device_shape(a)
    return int(a[0]), int(a[1]), int(a[2])


def _cstr_array(items: Sequence[bytes]):
    arr = (C.c_char_p * max(len(items), 1))()
    for i, s in enumerate(items):
        arr[i] = s
    return arr


class Descriptor:
    """A compiled descriptor: ``Descriptor(["-descr", "trna.descr"])``.

    ``argv`` is the rnamotif command line without the program name.  For
    descriptors whose score section calls efn() the energy tables are read from
    ``efn_datadir`` / $EFNDATA as in the reference; $EFNDATA defaults to the
    tables shipped with the package.
    """

    def __init__(self, argv: Sequence[str]):
        os.environ.setdefault("EFNDATA", EFNDATA_DIR)
        L = lib()
        args = [b"rnamotif"] + [a.encode() for a in argv]
        arr = _cstr_array(args)
        h = C.c_void_p()
        err = C.create_string_buffer(_ERRLEN)
        _check(L.rma_descr_compile(len(args), arr, C.byref(h), err, _ERRLEN), err)
        self._h = h
        self.program = L.rma_descr_program(h)
        self.efndata = L.rma_descr_efndata(h)
        self.efn2data = L.rma_descr_efn2data(h)
        info = (C.c_int32 * 8)()
        L.rma_program_info(self.program, info)
        (self.n_elems, self.n_searches, self.hit_stride, self.ctx_off, self.efn_off,
         self.n_efn_sites, self.both_strands, self.windowsize) = list(info)
        self.minlen = L.rma_descr_minlen(h)
        self.maxlen = L.rma_descr_maxlen(h)
        # elements whose seq= the scan tests loosely (back references, iupac = 0 letters): the records of a scan are
        # then a superset of rnamotif's candidates until they are replayed (rma_program_loose)
        self.loose = L.rma_program_loose(self.program)

    def names(self) -> List[str]:
        """The fields of the '#RM descr' line, one per printed column: "h5(tag='1')", "ss", ... (contexts included)."""
        L = lib()
        n = L.rma_descr_names(self._h, None, 0)
        buf = C.create_string_buffer(n + 1)
        L.rma_descr_names(self._h, buf, n + 1)
        return buf.value.decode().split()

    def search_order(self) -> List[int]:
        """Element index heading each search level (rm_searches[k]->s_descr->s_index)."""
        hdr = (C.c_int32 * (4 + self.n_searches)).from_address(self.program)   # magic, size, n_elems, n_searches, searches[]
        return [int(x) for x in hdr[4:4 + self.n_searches]]

    def close(self) -> None:
        if self._h:
            lib().rma_descr_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Database:
    """Sequences packed 2 bit + ambiguity mask, resident in HBM."""

    def __init__(self, scanner: "Scanner", seqs: Optional[Sequence[bytes]] = None, pack: Optional["Pack"] = None,
                 first: int = 0, count: Optional[int] = None, ranges: Optional[Sequence[Tuple[int, int]]] = None,
                 entries: Optional[Sequence[int]] = None, wait: bool = True):
        L = lib()
        self.scanner = scanner
        # (what device_text() defaults to: the pack the words came from and which of its entries)
        self._made_of = (pack, int(first), None if entries is None else [int(e) for e in entries])
        self._text, self.alphabet = None, None
        h = C.c_void_p()
        err = C.create_string_buffer(_ERRLEN)
        if pack is not None and entries is not None:
            # any entries of a packed database, each with a range of start positions (rma_db_create_packed_ranges)
            n = len(entries)
            assert ranges is None or len(ranges) == n
            self.n_seqs = n
            ent = (C.c_int32 * max(n, 1))(*[int(e) for e in entries])
            lo = (C.c_int32 * max(n, 1))(*[int(r[0]) for r in ranges]) if ranges is not None else None
            hi = (C.c_int32 * max(n, 1))(*[int(r[1]) for r in ranges]) if ranges is not None else None
            _check(L.rma_db_create_packed_ranges(scanner._h, pack._h, ent, lo, hi, n, C.byref(h), err, _ERRLEN), err)
        elif pack is not None:
            # entries [first, first+count) of a packed database, uploaded as they are
            count = pack.count - first if count is None else count
            self.n_seqs = count
            if wait:
                _check(L.rma_db_create_packed(scanner._h, pack._h, first, count, C.byref(h), err, _ERRLEN), err)
            else:
                # the copies run on the device's upload stream; the pack stays as it is until a scan has ended
                self._pack = pack
                _check(L.rma_db_create_packed_async(scanner._h, pack._h, first, count, C.byref(h), err, _ERRLEN), err)
        else:
            self.n_seqs = len(seqs)
            arr = _cstr_array(seqs)
            lens = (C.c_int32 * max(len(seqs), 1))(*[len(s) for s in seqs])
            if ranges is not None:
                # only start positions lo <= szero < hi of each strand of entry i (rma_db_create_ranges)
                lo = (C.c_int32 * max(len(seqs), 1))(*[int(r[0]) for r in ranges])
                hi = (C.c_int32 * max(len(seqs), 1))(*[int(r[1]) for r in ranges])
                _check(L.rma_db_create_ranges(scanner._h, arr, lens, lo, hi, len(seqs), C.byref(h), err, _ERRLEN), err)
            else:
                _check(L.rma_db_create(scanner._h, arr, lens, len(seqs), C.byref(h), err, _ERRLEN), err)
        self._h = h
        self.bases = L.rma_db_bases(h)

    def packed(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """The words in HBM, read back (verification): (codes uint32 [2 w], amask uint32 [w], base_off int64 [n],
        slen int32 [n]), w the mask words."""
        L = lib()
        w = int(L.rma_db_mask_words(self._h))
        codes = np.zeros(2 * w, dtype=np.uint32)
        amask = np.zeros(w, dtype=np.uint32)
        base_off = np.zeros(self.n_seqs, dtype=np.int64)
        slen = np.zeros(self.n_seqs, dtype=np.int32)
        err = C.create_string_buffer(_ERRLEN)
        _check(L.rma_db_read_packed(self._h, codes.ctypes.data, amask.ctypes.data, base_off.ctypes.data,
                                    slen.ctypes.data, err, _ERRLEN), err)
        return codes, amask, base_off, slen

    def device_text(self, pack: Optional["Pack"] = None, first: Optional[int] = None, entries: Optional[Sequence[int]] = None,
                    exceptions: Optional[Sequence[bytes]] = None) -> "Database":
        """Give a database of packed words its text in HBM, made there from the words (rma_db_text_attach*): one byte
        per base of device memory until the database is closed.  From then on score(), seq_check(), prune(),
        hit_structures(), align(), print_hits(), list_hits(), ct_hits() and Replay.device() take it as they take a
        database made by database_from_tensor(); its words and scans are unchanged.

        Default: the pack and the first / entries the database was made with; entry i of the database is entry
        entries[i] (else first + i) of pack, and .sids / .sdefs become the pack's names.  A database made of host
        strings has no pack: exceptions is one bytes per entry, the letters at its masked positions in order
        (lower case, not a, c, g or t), or None: every masked base reads n.  Runs behind torch's current stream and
        waits once.  Refused with words (RnamotifError), the database as it was: a database that has text already, a
        scan in flight, exceptions that are not the mask's number or no such letters, a pack entry of another length."""
        if getattr(self, "_h", None) is None or not self._h:
            raise ValueError("the database is closed")
        L = lib()
        made = getattr(self, "_made_of", (None, 0, None))
        if pack is None and exceptions is None:
            pack = made[0]
        if pack is not None and exceptions is not None:
            raise ValueError("device_text: a pack or exceptions, not both")
        stream = None
        try:
            import torch
            if torch.cuda.is_available():
                stream = torch.cuda.current_stream(torch.device("cuda", self.scanner.device)).cuda_stream
        except ImportError:
            pass
        err = C.create_string_buffer(_ERRLEN)
        if pack is not None:
            if entries is None and first is None:
                first, entries = made[1], made[2]
            ent = None
            if entries is not None:
                if len(entries) != self.n_seqs:
                    raise ValueError(f"entries: one per entry, {self.n_seqs}, not {len(entries)}")
                ent = (C.c_int32 * max(len(entries), 1))(*[int(e) for e in entries])
            _check(L.rma_db_text_attach_pack(self._h, pack._h, ent, int(first or 0), stream, err, _ERRLEN), err)
            self.sids, self.sdefs = [], []
            sid, sdef = C.c_char_p(), C.c_char_p()
            for i in range(self.n_seqs):
                L.rma_db_entry_name(self._h, i, C.byref(sid), C.byref(sdef))
                self.sids.append(sid.value)
                self.sdefs.append(sdef.value)
        elif exceptions is not None:
            if len(exceptions) != self.n_seqs:
                raise ValueError(f"exceptions: one per entry, {self.n_seqs}, not {len(exceptions)}")
            exc = b"".join(bytes(x) for x in exceptions)
            off = np.zeros(self.n_seqs + 1, dtype=np.int64)
            np.cumsum([len(x) for x in exceptions], out=off[1:])
            buf = C.create_string_buffer(exc, len(exc) + 1)
            _check(L.rma_db_text_attach(self._h, buf, off.ctypes.data_as(C.POINTER(C.c_int64)), stream, err, _ERRLEN), err)
        else:
            _check(L.rma_db_text_attach(self._h, None, None, stream, err, _ERRLEN), err)
        self._text = "owned"    # (as database_from_fasta_tensor(): the calls over records ask for a database with text)
        return self

    def read_text(self, i: int) -> bytes:
        """Entry i's text in HBM, read back (verification): the readers' letters, one byte per base."""
        if getattr(self, "_h", None) is None or not self._h:
            raise ValueError("the database is closed")
        L = lib()
        if not 0 <= int(i) < self.n_seqs:
            raise IndexError(f"entry {i} of {self.n_seqs}")
        err = C.create_string_buffer(_ERRLEN)
        slens = self.__dict__.get("_slens")
        if slens is None:       # (the entries' lengths, read back once)
            slens = np.zeros(max(self.n_seqs, 1), dtype=np.int32)
            _check(L.rma_db_read_packed(self._h, None, None, None, slens.ctypes.data, err, _ERRLEN), err)
            self._slens = slens
        n = int(slens[int(i)])
        buf = C.create_string_buffer(n + 1)
        _check(L.rma_db_read_text(self._h, int(i), buf, err, _ERRLEN), err)
        return buf.raw[:n]

    def wait(self) -> None:
        """Until the upload is complete (wait=False databases)."""
        err = C.create_string_buffer(_ERRLEN)
        _check(lib().rma_db_wait(self._h, err, _ERRLEN), err)

    def close(self) -> None:
        # (the table of default names Scanner.print_hits() made for this database goes first: it waits for its readers)
        names = self.__dict__.pop("_default_names", None)
        if names is not None:
            names.close()
        if self._h:
            lib().rma_db_destroy(self._h)
            self._h = None
        self._text = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def text_entries(text, offsets=None, lengths=None):
    """The entries of a byte tensor as (start, slen): int64 / int32 numpy arrays, start in bytes from the first
    byte of the tensor's storage.  Only the tensor's metadata is read (a CPU tensor will do).

    1-D uint8/int8 tensor: `offsets` (n+1 ascending, entry i = text[offsets[i]:offsets[i+1]]) or `lengths` (the
    entries one after the other), neither: one entry, the whole tensor.  2-D [N, L]: row i is entry i, its first
    `lengths[i]` bytes (default L); rows may lie at any stride(0), the bytes of a row one after the other."""
    import torch
    if not isinstance(text, torch.Tensor):
        raise TypeError(f"text is a {type(text).__name__}, not a torch.Tensor")
    if text.dtype not in (torch.uint8, torch.int8):
        raise TypeError(f"text is {text.dtype}: uint8 or int8 bytes are needed")

    def ints(x, what):
        if isinstance(x, torch.Tensor):
            x = x.detach().cpu().numpy()
        a = np.asarray(x)
        if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
            raise ValueError(f"{what}: a 1-D sequence of integers is needed")
        return a.astype(np.int64)

    so = int(text.storage_offset())
    if text.ndim == 1:
        if offsets is not None and lengths is not None:
            raise ValueError("offsets or lengths, not both")
        if text.numel() > 1 and text.stride(0) != 1:
            raise ValueError(f"text has stride {text.stride(0)}: the bytes of an entry one after the other are needed")
        size = int(text.numel())
        if offsets is not None:
            off = ints(offsets, "offsets")
            if off.size == 0:
                raise ValueError("offsets: n+1 values are needed (0 for no entry)")
            slen = np.diff(off)
            if off[0] < 0 or off[-1] > size or (slen < 0).any():
                raise ValueError(f"offsets: an ascending sequence inside the text's {size} bytes is needed")
            start = off[:-1]
        else:
            slen = ints(lengths, "lengths") if lengths is not None else np.array([size], dtype=np.int64)
            if (slen < 0).any() or int(slen.sum()) > size:
                raise ValueError(f"lengths: non-negative, {int(slen.sum())} bytes in all, the text has {size}")
            start = np.concatenate([[0], np.cumsum(slen)[:-1]]).astype(np.int64)
        start = start + so
    elif text.ndim == 2:
        if offsets is not None:
            raise ValueError("offsets are for a 1-D text; a 2-D text takes per-row lengths")
        rows, width = int(text.shape[0]), int(text.shape[1])
        if width > 1 and text.stride(1) != 1:
            raise ValueError(f"text has inner stride {text.stride(1)}: the bytes of a row one after the other are needed")
        if lengths is None:
            slen = np.full(rows, width, dtype=np.int64)
        else:
            slen = ints(lengths, "lengths")
            if slen.size != rows:
                raise ValueError(f"lengths: one per row, {rows}, not {slen.size}")
            if (slen < 0).any() or (slen > width).any():
                raise ValueError(f"lengths: 0 to the row length {width}")
        start = so + np.arange(rows, dtype=np.int64) * int(text.stride(0))
    else:
        raise ValueError(f"text has {text.ndim} dimensions: 1 (entries concatenated) or 2 (one entry per row)")
    if slen.size and slen.max() > 0x7fffffff:
        raise ValueError("an entry of 2**31 bases or more")
    return np.ascontiguousarray(start, dtype=np.int64), np.ascontiguousarray(slen, dtype=np.int32)


def alphabet_table(alphabet: str) -> bytes:
    """The 256-byte table of database_from_tensor(alphabet=...): value i is the letter alphabet[i] (its code as the
    readers take it, 4 for a letter that is not acgtu), every other value ambiguous (4)."""
    if not isinstance(alphabet, str) or not 0 < len(alphabet) <= 256:
        raise ValueError(f"alphabet: a string of 1 to 256 letters is needed, not {alphabet!r}")
    if any(ord(ch) > 255 for ch in alphabet):
        raise ValueError(f"alphabet: letters are single bytes, not {alphabet!r}")
    codes = C.create_string_buffer(256)
    lib().rma_letter_codes(codes)
    tab = bytearray([4] * 256)
    for i, ch in enumerate(alphabet):
        tab[i] = codes.raw[ord(ch)]
    return bytes(tab)


def reader_letter(b: int) -> int:
    """The letter the readers make of a byte (dbutil.c:112-113): an ASCII letter in lower case, u as t; every
    other byte is n here (the readers drop it; a device database keeps it, ambiguous)."""
    if 65 <= b <= 90:
        b += 32
    if 97 <= b <= 122:
        return ord("t") if b == ord("u") else b
    return ord("n")


def alphabet_letters(alphabet: str) -> bytes:
    """The 256 letters Replay.device() reads a database_from_tensor(alphabet=...) text as: value i is
    alphabet[i] as the readers take it, every other value n."""
    alphabet_table(alphabet)        # (the same checks)
    tab = bytearray(b"n" * 256)
    for i, ch in enumerate(alphabet):
        tab[i] = reader_letter(ord(ch))
    return bytes(tab)


def prune_groups(sids) -> np.ndarray:
    """One id per entry for Scanner.prune(groups=...): int32, two ids equal iff the entries' names are equal as the
    rmprune tool takes them from a hit's '>' line (getname): leading blanks skipped, the name up to the first '.'
    or blank.  sids: the entries' names, bytes or str (db.sids of database_from_fasta_tensor())."""
    ids, seen = [], {}
    for sid in sids:
        b = sid.encode() if isinstance(sid, str) else bytes(sid)
        q = 0
        while q < len(b) and b[q:q + 1].isspace():
            q += 1
        e = q
        while e < len(b) and b[e:e + 1] != b"." and not b[e:e + 1].isspace():
            e += 1
        ids.append(seen.setdefault(b[q:e], len(seen)))
    return np.asarray(ids, dtype=np.int32)


def _record_args(db, hits, device, stride, whose, text_hint, letters=None):
    """What every call over records on the GPU does first.  db: open and, with text_hint (what to do instead), made
    from a tensor; hits: an int32 CUDA tensor [n, stride] on `device` (None: the device of db's scanner), records of
    the descriptor of `whose` ("scanner", "replay"); letters: 256 bytes, default db's alphabet= (calls that read text).
    Returns (hits contiguous, n, the torch device, torch's current stream on it, letters)."""
    import torch
    if getattr(db, "_h", None) is None or not db._h:
        raise ValueError("the database is closed")
    if text_hint is not None and getattr(db, "_text", None) is None:
        raise ValueError("the database was not made by database_from_tensor(): " + text_hint)
    if not isinstance(hits, torch.Tensor):
        raise TypeError(f"hits is a {type(hits).__name__}, not a torch.Tensor")
    if device is None:
        device = db.scanner.device
    if hits.device.type != "cuda" or (hits.device.index if hits.device.index is not None else torch.cuda.current_device()) != device:
        raise ValueError(f"hits is on {hits.device}: the database is on cuda:{device}")
    if hits.dtype != torch.int32:
        raise TypeError(f"hits is {hits.dtype}: int32 records are needed")
    if hits.ndim != 2 or int(hits.shape[1]) != stride:
        raise ValueError(f"hits has shape {tuple(hits.shape)}: [n, {stride}] records of this {whose}'s descriptor are needed")
    if text_hint is not None:
        if letters is None and db.alphabet is not None:
            letters = alphabet_letters(db.alphabet)
        if letters is not None and len(letters) != 256:
            raise ValueError(f"letters: 256 bytes are needed, not {len(letters)}")
    dev = torch.device("cuda", device)
    return hits.contiguous(), int(hits.shape[0]), dev, torch.cuda.current_stream(dev), letters


class ScoreProgram:
    """The MAIN program of a descriptor's score section as an image the GPU runs, one record per lane
    (rma_score_open; Scanner.score() takes it).  Raises RnamotifError with the reason where the program cannot be
    judged record by record on the device: HOLD / RELEASE or a variable carried from one hit to the next, sprintf(),
    bits() (without text=True), mismatches( string, pattern ), =~ / !~ (without match=True), a read of NAME, a loose
    descriptor (without checked=True), an image beyond the limits of csrc/rm_score_image.h.  The descriptor itself is not touched: the image is made from a private copy.
    checked=True (rma_score_open_checked) opens a loose descriptor too: the caller promises to score only
    r.hits[r.keep] of r = Scanner.seq_check(db, hits), the records that are rnamotif's candidates, as fixed rows.
    text=True (rma_score_open_flags with RMA_SCORE_TEXT) opens a program with sprintf(), bits(), string + and a string
    in SCORE: the rule then makes strings in a heap of option "score_heap" bytes a record, writes printf's %d %s %f
    with the host's bytes and reads bits()'s logarithms from a table made here; %e %E %g %G in a constant format is
    refused.  Scanner.score(..., text=True) delivers the score column of such a program.
    match=True (RMA_SCORE_MATCH, with either of the others) opens a program with =~, !~ and mismatches( string, pattern )
    whose patterns are string constants: each is compiled here, once, and applied to every record's string by the
    reference's matcher in LDS (csrc/rm_seqcheck.h), its steps counted against option "score_budget".  A pattern from a
    variable, an element reference or sprintf(), one the reference's compile() rejects, more than 32 patterns are
    refused; NAME and HOLD / RELEASE stay refused.  info() reports the kernel that would run: a program without a
    pattern runs what it runs without the flag."""

    def __init__(self, descr: Descriptor, checked: bool = False, text: bool = False, match: bool = False):
        h = C.c_void_p()
        err = C.create_string_buffer(_ERRLEN)
        L = lib()
        if text or match:
            _check(L.rma_score_open_flags(descr._h, (1 if checked else 0) | (2 if text else 0) | (8 if match else 0), C.byref(h), err, _ERRLEN), err)
        else:
            _check((L.rma_score_open_checked if checked else L.rma_score_open)(descr._h, C.byref(h), err, _ERRLEN), err)
        self._h = h
        self.descr = descr
        self.checked = bool(checked)
        self.text = bool(text)
        self.match = bool(match)

    @staticmethod
    def reason(descr: Descriptor, checked: bool = False, text: bool = False, match: bool = False) -> Optional[str]:
        """Why ScoreProgram(descr, checked, text, match) would refuse, or None where it opens."""
        try:
            ScoreProgram(descr, checked, text, match).close()
        except RnamotifError as e:
            return str(e)
        return None

    def info(self) -> dict:
        """The image's and its kernel's sizes (rma_score_info); the last three are -1 where no GPU answers."""
        a = (C.c_int32 * 10)()
        lib().rma_score_info(self._h, a)
        return dict(zip(("image_bytes", "instructions", "variables", "stack_slots", "wave_lds_bytes", "waves_per_workgroup",
                         "workgroup_lds_bytes", "private_bytes", "static_lds_bytes", "registers"), (int(x) for x in a)))

    def close(self) -> None:
        if self._h:
            lib().rma_score_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SeqCheck:
    """The seq= expressions of a descriptor that its scan tests loosely (descr.loose > 0: back references, \\< \\>,
    letters that are not acgt with iupac = 0) as an image the GPU applies to records, one record per lane
    (rma_seqcheck_open; Scanner.seq_check() takes it).  A descriptor that is not loose opens with no expressions.
    Raises RnamotifError with the reason beyond the limits of csrc/rm_seqcheck.h."""

    def __init__(self, descr: Descriptor):
        h = C.c_void_p()
        err = C.create_string_buffer(_ERRLEN)
        _check(lib().rma_seqcheck_open(descr._h, C.byref(h), err, _ERRLEN), err)
        self._h = h
        self.descr = descr

    @property
    def info(self) -> dict:
        """The image's and its kernel's sizes (rma_seqcheck_info); the last two are -1 where no GPU answers."""
        a = (C.c_int32 * 8)()
        lib().rma_seqcheck_info(self._h, a)
        return dict(zip(("expressions", "ops", "frames", "image_bytes", "waves_per_workgroup", "workgroup_lds_bytes",
                         "private_bytes", "registers"), (int(x) for x in a)))

    def close(self) -> None:
        if self._h:
            lib().rma_seqcheck_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SeqChecked:
    """Scanner.seq_check()'s result, tensors on the scanner's device, ready on torch's current stream.

    keep  torch.bool [n]          the record passes every loose seq= expression: it is a candidate of rnamotif's
    hits  int32 [n, hit_stride]   the records with the mismatch counts the expressions fix (None with fixed=False);
                                  hits[keep] are the rows the score section, prune(), align() ... go on with"""

    def __init__(self, keep, hits):
        self.keep, self.hits = keep, hits


class HitScores:
    """Scanner.score()'s result, tensors on the scanner's device, ready on torch's current stream.

    accept  torch.bool [n]   the record is a hit: MAIN accepts it
    score   float64 [n]      its SCORE, an int as its exact double; 0.0 for a rejected record
    kind    int8 [n]         0: no SCORE, 1: an int, 2: a float, 3: a string (score 0.0); 0 for a rejected record
    with Scanner.score(..., text=True):
    text_bytes  uint8 [n, W]  the score column HitPrinter::print writes behind the blank after the name: %8d of an int
                              SCORE, %8.3lf of a float or of none, %8s of a string; bytes behind text_len are not written
    text_len    int32 [n]     its length, 0 for a rejected record"""

    def __init__(self, accept, score, kind, text_bytes=None, text_len=None):
        self.accept, self.score, self.kind = accept, score, kind
        self.text_bytes, self.text_len = text_bytes, text_len

    def text(self, h: int) -> bytes:
        """What HitPrinter::print puts behind the name for record h, the blank and the score column: " %8d" of an int
        SCORE, " %8.3lf" of a float, " %8.3lf" of 0.0 where there is none and, with text_bytes, " %8s" of a string."""
        if self.text_bytes is not None:
            return b" " + bytes(self.text_bytes[h, :int(self.text_len[h])].cpu().numpy().tobytes())
        k = int(self.kind[h])
        v = float(self.score[h])
        if k == 1:
            return b" %8d" % int(v)
        return (" %8.3f" % (v if k == 2 else 0.0)).encode()


class HitStructures:
    """Scanner.hit_structures()'s result: the windows of n records, base by base, as tensors on the scanner's device.

    off   int64 [n+1]  window h is [off[h], off[h+1]) of the per-base tensors
    lo    int32 [n]    its first position on the hit's strand
    base  uint8 [T]    the letters as Replay.device() reads them
    elem  int16 [T]    the descriptor element of each base (n_elems / n_elems + 1: left / right context, -1: none)
    mate  int32 [T, 3] window-relative indices of the bases it is matched with, -1 padding"""

    def __init__(self, off, lo, base, elem, mate):
        self.off, self.lo, self.base, self.elem, self.mate = off, lo, base, elem, mate

    def padded(self, fill=(ord("n"), -1, -1)):
        """([n, Lmax] base, elem, [n, Lmax, 3] mate, bool mask) with Lmax the longest window; fill: the values of
        (base, elem, mate) past a window's end.  Plain torch operations, no kernel of this package."""
        import torch
        n = int(self.lo.shape[0])
        lens = self.off[1:] - self.off[:-1]
        width = int(lens.max()) if n else 0
        col = torch.arange(width, device=self.off.device, dtype=torch.int64)
        mask = col[None, :] < lens[:, None]
        at = (self.off[:-1, None] + col[None, :])[mask]
        base = torch.full((n, width), int(fill[0]), dtype=self.base.dtype, device=self.base.device)
        elem = torch.full((n, width), int(fill[1]), dtype=self.elem.dtype, device=self.elem.device)
        mate = torch.full((n, width, 3), int(fill[2]), dtype=self.mate.dtype, device=self.mate.device)
        base[mask] = self.base[at]
        elem[mask] = self.elem[at]
        mate[mask] = self.mate[at]
        return base, elem, mate, mask

    def energies(self, scanner: "Scanner", letters: Optional[bytes] = None, efn: bool = True, efn2: bool = True):
        """Scanner.structure_energies() of these windows, each taken whole: column 0 of mate read in place."""
        return scanner.structure_energies(self.off, self.base, self.mate, letters=letters, efn=efn, efn2=efn2)


class HitAlignment:
    """Scanner.align()'s result: n records laid into the columns of an alignment, as `rmfmt -a` lays their printed form.

    rows     uint8 [n, W] on the scanner's device: the fields in column order, each padded to its column's width
             with the gap byte, one separator byte between columns
    pos      int32 [n, W] or None: for a letter byte the position on the hit's strand it came from (the coordinate
             of HitStructures.lo), -1 for gap, separator and empty-field bytes
    widths   np.int32 [n_cols]; col_off np.int64 [n_cols], the first byte of each column; right np.bool_ [n_cols],
             True for the right-aligned columns (h3, t2, q2, q4); names, the '#RM descr' fields
    col      np.int16 [W]: the column of each byte of a row, -1 for a separator
    fill     the gap, separator and empty-field bytes"""
    LINE = 70       # rmfmt.c: WBSIZE

    def __init__(self, rows, pos, widths, right, names, fill):
        self.rows, self.pos, self.fill, self.names = rows, pos, bytes(fill), list(names)
        self.widths = np.asarray(widths, dtype=np.int32)
        self.right = np.asarray(right, dtype=np.bool_)
        n_cols = self.widths.size
        self.col_off = np.zeros(n_cols, dtype=np.int64)
        if n_cols:
            self.col_off[1:] = np.cumsum(self.widths[:-1].astype(np.int64) + 1)
        w = int(self.widths.sum(dtype=np.int64)) + max(n_cols - 1, 0)
        self.col = np.full(w, -1, dtype=np.int16)
        for c in range(n_cols):
            self.col[self.col_off[c]:self.col_off[c] + self.widths[c]] = c

    def lines(self, h: int) -> List[bytes]:
        """Row h as rmfmt -a writes it: its bytes cut into lines of 70 (the sequence lines, without the '>' line)."""
        row = bytes(self.rows[h].cpu().numpy().tobytes())
        return [row[i:i + self.LINE] for i in range(0, len(row), self.LINE)]


class EntryNames:
    """The names and definitions of a database's entries as a table on the GPU (rma_names_create), for
    Scanner.print_hits().  db: a database made by database_from_tensor() or database_from_fasta_tensor(); sids / sdefs:
    one bytes per entry, defaults as Replay.device() -- the entry's number in decimal and b"" -- and for a database made
    from FASTA text its own db.sids / db.sdefs; a None among given names is that entry's default.  Uploaded once, behind the database, without a wait.  Refused with words
    (RnamotifError): a count that is not the database's, a NUL inside a name or definition, a sid of 2048 bytes or more."""

    def __init__(self, scanner: "Scanner", db: "Database", sids: Optional[Sequence[bytes]] = None, sdefs: Optional[Sequence[bytes]] = None):
        if getattr(db, "_h", None) is None or not db._h:
            raise ValueError("the database is closed")
        n = None
        lens = []
        for what, names in (("sids", sids), ("sdefs", sdefs)):
            if names is None:
                lens.append(None)
                continue
            names = [None if x is None else bytes(x) for x in names]        # (None: that entry's default)
            if n is not None and len(names) != n:
                raise ValueError(f"sids and sdefs: {n} and {len(names)}")
            n = len(names)
            lens.append((names, np.ascontiguousarray([0 if x is None else len(x) for x in names] or [0], dtype=np.int64)))
        if n is None:
            n = db.n_seqs
        i64p = C.POINTER(C.c_int64)
        h = C.c_void_p()
        err = C.create_string_buffer(_ERRLEN)
        args = []
        for item in lens:
            args += [None, None] if item is None else [_cstr_array(item[0]), item[1].ctypes.data_as(i64p)]
        _check(lib().rma_names_create(scanner._h, db._h, args[0], args[1], args[2], args[3], n, C.byref(h), err, _ERRLEN), err)
        self._h = h
        self.scanner, self.db, self.n = scanner, db, n

    def close(self) -> None:
        if self._h:
            lib().rma_names_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HitPrint:
    """Scanner.print_hits()'s result: what rnamotif writes for n records, as bytes on the scanner's device.

    bytes   uint8 [T]     the '>sid sdef' line and the hit line of every printed record, in the order given
    off     int64 [n+1]   record h is bytes[off[h]:off[h+1]], empty where it is not printed
    header  bytes         the three '#RM' lines rnamotif writes in front of its first hit"""

    def __init__(self, data, off, header: bytes):
        self.bytes, self.off, self.header = data, off, header

    def record(self, h: int) -> bytes:
        """The two lines of record h (one copy), b"" for a record that is not printed."""
        a, b = (int(x) for x in self.off[h:h + 2].cpu())
        return bytes(self.bytes[a:b].cpu().numpy().tobytes())

    def write(self, fp, header: bool = True) -> int:
        """All the bytes to the binary file fp, one device-to-host copy; with header, the '#RM' lines first when at
        least one record is printed -- nothing at all otherwise, as rnamotif writes nothing without a hit.  Returns the
        bytes written."""
        data = self.bytes.cpu().numpy().tobytes()
        if not data:
            return 0
        if header:
            fp.write(self.header)
        fp.write(data)
        return len(data) + (len(self.header) if header else 0)


class HitCt:
    """Scanner.ct_hits()'s result: what rm2ct writes for n records, as bytes on the scanner's device.

    bytes   uint8 [T]     the connect record of every printed record, in the order given: a header line, a line per base
    off     int64 [n+1]   record h is bytes[off[h]:off[h+1]], empty where it is not printed"""

    def __init__(self, data, off):
        self.bytes, self.off = data, off

    def record(self, h: int) -> bytes:
        """The connect record of record h (one copy), b"" for a record that is not printed."""
        a, b = (int(x) for x in self.off[h:h + 2].cpu())
        return bytes(self.bytes[a:b].cpu().numpy().tobytes())

    def write(self, fp) -> int:
        """All the bytes to the binary file fp, one device-to-host copy; no '#RM' lines: rm2ct writes none.  Returns the
        bytes written."""
        data = self.bytes.cpu().numpy().tobytes()
        fp.write(data)
        return len(data)


class HitList:
    """Scanner.list_hits()'s result: rmfmt's listing of the printed records, as bytes on the scanner's device.

    lines   uint8 [m, L]  line r of the listing, its newline included: every line has the same length
    perm    int64 [m]     line r is record perm[r] of the hits given
    mode    int           1: sorted by score, best first; 2: by name and position; 0: input order (more than smax bytes)
    widths  int32 [5+c]   the widths of the name, the score block, comp, offset, len and the c element columns
    header  bytes         the three '#RM' lines rmfmt copies from rnamotif's output"""

    def __init__(self, lines, perm, mode: int, widths, header: bytes):
        self.lines, self.perm, self.mode, self.widths, self.header = lines, perm, mode, widths, header

    def line(self, r: int) -> bytes:
        """Line r (one copy)."""
        return bytes(self.lines[r].cpu().numpy().tobytes())

    def write(self, fp, header: bool = True) -> int:
        """The listing to the binary file fp, one device-to-host copy; with header, the '#RM' lines first.  Nothing at
        all when nothing is listed, as rmfmt of empty input writes nothing.  Returns the bytes written."""
        data = self.lines.cpu().numpy().tobytes() if int(self.lines.shape[0]) else b""
        if not data:
            return 0
        if header:
            fp.write(self.header)
        fp.write(data)
        return len(data) + (len(self.header) if header else 0)


class Scanner:
    """The motif program on one GPU (RM_fm_init + RM_find_motif)."""

    def __init__(self, descr: Descriptor, device: int = 0):
        L = lib()
        self.descr = descr
        h = C.c_void_p()
        err = C.create_string_buffer(_ERRLEN)
        _check(L.rma_scanner_create(descr.program, descr.efndata, device, C.byref(h), err, _ERRLEN), err)
        self._h = h
        self.device = device
        if descr.efn2data:
            _check(L.rma_scanner_set_efn2data(h, descr.efn2data, err, _ERRLEN), err)

    def database(self, seqs: Sequence[bytes], ranges: Optional[Sequence[Tuple[int, int]]] = None) -> Database:
        return Database(self, seqs, ranges=ranges)

    def database_from_pack(self, pack: "Pack", first: int = 0, count: Optional[int] = None,
                           entries: Optional[Sequence[int]] = None,
                           ranges: Optional[Sequence[Tuple[int, int]]] = None, wait: bool = True, text: bool = False) -> Database:
        """Entries of a packed database, uploaded as they are.  text=True: Database.device_text() at once -- the
        database's text made in HBM from the words (1 byte per base of device memory until it is closed), so that
        the calls over hit records on the GPU take it."""
        db = Database(self, pack=pack, first=first, count=count, entries=entries, ranges=ranges, wait=wait)
        if text:
            db.device_text()
        return db

    def database_from_tensor(self, text, offsets=None, lengths=None, ranges: Optional[Sequence[Tuple[int, int]]] = None,
                             alphabet: Optional[str] = None, wait: bool = False) -> Database:
        """A database of bytes already on this scanner's GPU, packed there (rma_db_create_device): the same words
        database() makes of the same bytes.  text and the entries in it as text_entries() takes them; ranges as
        database(); alphabet: value i of the text is letter alphabet[i] (default: the bytes are letters).  The
        packing runs behind the work queued on torch's current stream; the database keeps the tensor until it is
        closed.  Records of its scans are candidates as rma_scan returns them; Replay.device() scores and prints
        them from the text on the GPU."""
        import torch
        if not isinstance(text, torch.Tensor):
            raise TypeError(f"text is a {type(text).__name__}, not a torch.Tensor")
        if text.device.type != "cuda" or (text.device.index if text.device.index is not None else torch.cuda.current_device()) != self.device:
            raise ValueError(f"text is on {text.device}: the scanner is on cuda:{self.device}")
        start, slen = text_entries(text, offsets, lengths)
        n = len(slen)
        lo = hi = None
        if ranges is not None:
            if len(ranges) != n:
                raise ValueError(f"ranges: one per entry, {n}, not {len(ranges)}")
            lo = np.ascontiguousarray([int(r[0]) for r in ranges], dtype=np.int32)
            hi = np.ascontiguousarray([int(r[1]) for r in ranges], dtype=np.int32)
        table = alphabet_table(alphabet) if alphabet is not None else None
        storage = text.untyped_storage()
        stream = torch.cuda.current_stream(text.device).cuda_stream
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        h = C.c_void_p()
        err = C.create_string_buffer(_ERRLEN)
        _check(lib().rma_db_create_device(self._h, storage.data_ptr(), storage.nbytes(), start.ctypes.data_as(i64p),
                                          slen.ctypes.data_as(i32p), lo.ctypes.data_as(i32p) if lo is not None else None,
                                          hi.ctypes.data_as(i32p) if hi is not None else None, n, table, stream,
                                          C.byref(h), err, _ERRLEN), err)
        db = Database.__new__(Database)
        db.scanner, db.n_seqs, db._h, db._text = self, n, h, text
        db.start, db.slen, db.alphabet = start, slen, alphabet
        db.bases = lib().rma_db_bases(h)
        if wait:
            db.wait()
        return db

    def database_from_fasta_tensor(self, text, maxslen: int = 0) -> Database:
        """A database of FASTA text already on this scanner's GPU -- the bytes of a file, '>' lines and line breaks
        included -- cut into entries and packed there (rma_db_create_device_fasta): the entries, names and words
        Pack.read() + database_from_pack() make of the same file.  text: a 1-D contiguous uint8 / int8 tensor on the
        scanner's device (a view with a storage offset will do); maxslen as Pack.read().  The call synchronises
        and the tensor is free once it returns: the database keeps the letters (1 byte per base of HBM until it is
        closed).  .sids / .sdefs are the entries' names and definitions, ready for
        Replay.device(db, hits, sids=db.sids, sdefs=db.sdefs).  Text the readers have a diagnostic for is refused
        (RnamotifError naming the entry)."""
        import torch
        if not isinstance(text, torch.Tensor):
            raise TypeError(f"text is a {type(text).__name__}, not a torch.Tensor")
        if text.dtype not in (torch.uint8, torch.int8):
            raise TypeError(f"text is {text.dtype}: the bytes of a FASTA file are uint8 or int8")
        if text.dim() != 1:
            raise ValueError(f"text has {text.dim()} dimensions: the bytes of a FASTA file are a 1-D tensor")
        if not text.is_contiguous():
            raise ValueError(f"text has stride {text.stride(0)}: a contiguous tensor is needed")
        if text.device.type != "cuda" or (text.device.index if text.device.index is not None else torch.cuda.current_device()) != self.device:
            raise ValueError(f"text is on {text.device}: the scanner is on cuda:{self.device}")
        if int(maxslen) < 0:
            raise ValueError(f"maxslen is {maxslen}")
        L = lib()
        stream = torch.cuda.current_stream(text.device).cuda_stream
        h = C.c_void_p()
        err = C.create_string_buffer(_ERRLEN)
        _check(L.rma_db_create_device_fasta(self._h, text.data_ptr() if text.numel() else None, text.numel(), int(maxslen),
                                            stream, C.byref(h), err, _ERRLEN), err)
        db = Database.__new__(Database)
        db.scanner, db._h, db.alphabet = self, h, None
        db._text = "owned"      # (Replay.device asks for a database with text on the device: this one owns its text)
        db.n_seqs = int(L.rma_db_entries(h))
        db.bases = L.rma_db_bases(h)
        db.sids, db.sdefs = [], []
        sid, sdef = C.c_char_p(), C.c_char_p()
        for i in range(db.n_seqs):
            L.rma_db_entry_name(h, i, C.byref(sid), C.byref(sdef))
            db.sids.append(sid.value)
            db.sdefs.append(sdef.value)
        return db

    def scan_tensor(self, db: Database):
        """scan(db) with the records left on the GPU: an int32 tensor [n, hit_stride] on the scanner's device, the
        same records in the same order, ready on torch's current stream.  Candidates before the score section, a
        superset of rnamotif's when descr.loose > 0, until Replay.device() replays them or seq_check() says which to keep."""
        import torch
        self.scan_begin(db)
        n = self.scan_end_on_device()
        dev = torch.device("cuda", self.device)
        out = torch.empty((n, self.descr.hit_stride), dtype=torch.int32, device=dev)
        if n > 0:
            err = C.create_string_buffer(_ERRLEN)
            _check(lib().rma_scan_records_to_device(self._h, out.data_ptr(), out.numel(),
                                                    torch.cuda.current_stream(dev).cuda_stream, err, _ERRLEN), err)
        return out

    def hit_structures(self, db: Database, hits, letters: Optional[bytes] = None) -> HitStructures:
        """The secondary structure of records of a database made by database_from_tensor() or
        database_from_fasta_tensor(), as tensors on the GPU (rma_hit_structures; the rule is csrc/rm_hitstruct.h's):
        per base of each record's window -- the bases its elements and contexts cover, what Replay.device() reads --
        its letter, its descriptor element and the bases it is matched with.  hits: int32 CUDA tensor [n, hit_stride]
        on the scanner's device, scan_tensor()'s output or any rows of it in any order (hits[mask] of
        Replay.device(..., accepted=True) for the accepted ones).  letters as Replay.device().  The tensors are torch's
        and ready on torch's current stream; the call waits once, for the total length.  A malformed record is refused
        (RnamotifError naming its index) before anything is written."""
        import torch
        hits, n, dev, cur, letters = _record_args(db, hits, self.device, self.descr.hit_stride, "scanner",
                                                  "replay it with batch() or pack()", letters)
        L = lib()
        err = C.create_string_buffer(_ERRLEN)
        stream = cur.cuda_stream
        total = C.c_int64(0)
        if n:
            _check(L.rma_hit_structures_size(self._h, db._h, hits.data_ptr(), n, stream, C.byref(total), err, _ERRLEN), err)
        t = int(total.value)
        st = HitStructures(torch.empty(n + 1, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
                           torch.empty(t, dtype=torch.uint8, device=dev), torch.empty(t, dtype=torch.int16, device=dev),
                           torch.empty((t, 3), dtype=torch.int32, device=dev))
        _check(L.rma_hit_structures(self._h, db._h, hits.data_ptr() if n else None, n, letters, t, st.off.data_ptr(),
                                    st.lo.data_ptr() if n else None, st.base.data_ptr() if t else None,
                                    st.elem.data_ptr() if t else None, st.mate.data_ptr() if t else None, stream, err, _ERRLEN), err)
        # (the records are read by kernels queued behind this stream: torch keeps their memory until those have run)
        hits.record_stream(cur)
        return st

    def align(self, db: Database, hits, letters: Optional[bytes] = None, widths=None, fill: bytes = b"-|.", pos: bool = False) -> HitAlignment:
        """Records of a database made by database_from_tensor() or database_from_fasta_tensor() as an alignment on the
        GPU (rma_hit_alignment; the rule is csrc/rm_hitalign.h's): a uint8 matrix [n, W] whose row h, cut into lines
        of 70, is what `rmfmt -a` writes for the printed form of record h among these records.  Every descriptor
        element (and context) is a column as wide as its longest instance over the records; shorter instances are
        padded with fill[0], the 3' strands h3, t2, q2, q4 on their left so that paired bases share a column; fill[1]
        separates columns and fill[2] stands for an empty element.  hits and letters as hit_structures().  widths:
        one per column, at least what the records need (RnamotifError naming the column otherwise) -- the .widths of
        another call, or the maximum of several, so that batches share their columns; default: what these records
        need.  pos=True adds the position on the hit's strand of every letter byte.  The tensors are torch's and
        ready on torch's current stream; the call waits for the record check and the widths.  A malformed record is
        refused (RnamotifError naming its index) before anything is written."""
        import torch
        hits, n, dev, cur, letters = _record_args(db, hits, self.device, self.descr.hit_stride, "scanner",
                                                  "print its hits and use bin/rmfmt -a", letters)
        fill = bytes(fill)
        if len(fill) != 3:
            raise ValueError(f"fill: 3 bytes (gap, separator, empty) are needed, not {len(fill)}")
        L = lib()
        err = C.create_string_buffer(_ERRLEN)
        stream = cur.cuda_stream
        i32p = C.POINTER(C.c_int32)
        n_cols, row_bytes = C.c_int32(0), C.c_int64(0)
        need, right = np.zeros(102, dtype=np.int32), np.zeros(102, dtype=np.uint8)
        # (given widths: the shape of no record, for the columns and their directions; the fill call holds the widths
        # to the records)
        _check(L.rma_hit_alignment_shape(self._h, db._h, hits.data_ptr() if n and widths is None else None, n if widths is None else 0,
                                         C.byref(n_cols), need.ctypes.data_as(i32p), right.ctypes.data, C.byref(row_bytes), stream,
                                         err, _ERRLEN), err)
        nc = int(n_cols.value)
        if widths is None:
            w = need[:nc].copy()
        else:
            w = np.ascontiguousarray(np.asarray(widths), dtype=np.int32)
            if w.ndim != 1 or w.size != nc:
                raise ValueError(f"widths: one per column, {nc}, not {w.size if w.ndim == 1 else tuple(w.shape)}")
            if (w < 0).any():
                raise ValueError("widths: a negative width")
        al = HitAlignment(None, None, w, right[:nc], self.descr.names(), fill)
        width = int(al.col.size)
        al.rows = torch.empty((n, width), dtype=torch.uint8, device=dev)
        if pos:
            al.pos = torch.empty((n, width), dtype=torch.int32, device=dev)
        if n:
            _check(L.rma_hit_alignment(self._h, db._h, hits.data_ptr(), n, w.ctypes.data_as(i32p), letters, fill,
                                       al.rows.data_ptr() if width else None, al.pos.data_ptr() if pos and width else None,
                                       stream, err, _ERRLEN), err)
            # (the records are read by kernels queued behind this stream: torch keeps their memory until those have run)
            hits.record_stream(cur)
        return al

    def prune(self, db: Database, hits, groups=None):
        """Which of these records the rmprune tool would keep, decided on the GPU (rma_prune_hits; the rule is
        csrc/rm_prune.h's): a torch.bool tensor [n] on the scanner's device, ready on torch's current stream, False
        where a record is only an "unzipped" version of another -- the tool's decisions on the printed form of the
        same records in the same order.  The order given is the order judged: pass hits[accepted] of
        Replay.device(..., accepted=True) to prune what would be printed, then hit_structures(db, hits[keep]).
        hits: int32 CUDA tensor [n, hit_stride] on the scanner's device; db: the database the records are of (only
        its entry lengths are read); groups: an int per entry, equal for entries the tool takes as one name
        (prune_groups(db.sids)), default: every entry its own.  The call waits once, for the record check.  A
        malformed record is refused (RnamotifError naming its index)."""
        import torch
        hits, n, dev, stream, _ = _record_args(db, hits, self.device, self.descr.hit_stride, "scanner", None)
        g = None
        if groups is not None:
            g = np.ascontiguousarray(np.asarray(groups), dtype=np.int32)
            if g.ndim != 1 or g.size != db.n_seqs:
                raise ValueError(f"groups: one per entry, {db.n_seqs}, not {g.size if g.ndim == 1 else tuple(g.shape)}")
        keep = torch.empty(n, dtype=torch.bool, device=dev)
        if n:
            err = C.create_string_buffer(_ERRLEN)
            _check(lib().rma_prune_hits(self._h, db._h, hits.data_ptr(), n,
                                        g.ctypes.data_as(C.POINTER(C.c_int32)) if g is not None else None,
                                        keep.data_ptr(), stream.cuda_stream, err, _ERRLEN), err)
            # (the records are read by a kernel queued on this stream: torch keeps their memory until it has run)
            hits.record_stream(stream)
        return keep

    def score(self, db: Database, hits, program: ScoreProgram, letters: Optional[bytes] = None, out=None, text: bool = False,
              text_width: int = 64) -> HitScores:
        """The score section's MAIN on each of these records, on the GPU (rma_score_hits; the rule is
        csrc/rm_score_core.h's, what ScoreVM::run does on the host): a HitScores -- which records are hits, and the
        SCORE of each -- so that hits[scores.accept] goes on to prune(), hit_structures(), align() without a trip to
        the host.  hits: int32 CUDA tensor [n, hit_stride] on the scanner's device, any rows of a scan's records in any
        order; db: the database_from_tensor() / database_from_fasta_tensor() database they are of; program:
        ScoreProgram(descr) of this scanner's descriptor; letters as Replay.device() takes them.  out: (accept, score,
        kind) tensors to write instead of new ones.  The call waits once.  A malformed record, and a record on which
        MAIN stops -- type mismatch, undefined variable, bad pos or len, integer division by zero, string + string,
        more than option "score_budget" (2^20) instructions ... -- raise RnamotifError naming the lowest such record;
        nothing is written then.  text=True (rma_score_hits_text): the result also has text_bytes [n, text_width] and
        text_len [n], the score column of every record as HitPrinter::print writes it, so that a program whose SCORE is
        a string (kind 3; ScoreProgram(descr, text=True)) is served too; a column longer than text_width stops its
        record.  out may then hold five tensors."""
        import torch
        hits, n, dev, stream, letters = _record_args(db, hits, self.device, self.descr.hit_stride, "scanner",
                                                    "its records are scored by Replay.batch() or pack()", letters)
        if not isinstance(program, ScoreProgram) or not program._h:
            raise ValueError("program: an open ScoreProgram is needed")
        if text and (not isinstance(text_width, int) or text_width < 1):
            raise ValueError(f"text_width: a positive int is needed, not {text_width!r}")
        if out is None:
            out = (torch.empty(n, dtype=torch.bool, device=dev), torch.zeros(n, dtype=torch.float64, device=dev),
                   torch.zeros(n, dtype=torch.int8, device=dev))
            if text:
                out += (torch.zeros((n, text_width), dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
        if len(out) != (5 if text else 3):
            raise ValueError("out: (accept, score, kind%s) are needed" % (", text_bytes, text_len" if text else ""))
        for t, dt, what in zip(out, (torch.bool, torch.float64, torch.int8), ("accept", "score", "kind")):
            if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != (n,) or t.device != dev or not t.is_contiguous():
                raise ValueError(f"out: {what} must be a contiguous {dt} tensor [{n}] on {dev}")
        if text:
            for t, dt, shape, what in ((out[3], torch.uint8, (n, text_width), "text_bytes"), (out[4], torch.int32, (n,), "text_len")):
                if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
                    raise ValueError(f"out: {what} must be a contiguous {dt} tensor {list(shape)} on {dev}")
        if n and text:
            err = C.create_string_buffer(_ERRLEN)
            _check(lib().rma_score_hits_text(self._h, program._h, db._h, hits.data_ptr(), n, letters, out[0].data_ptr(),
                                             out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), text_width, out[4].data_ptr(),
                                             stream.cuda_stream, err, _ERRLEN), err)
            hits.record_stream(stream)
        elif n:
            err = C.create_string_buffer(_ERRLEN)
            _check(lib().rma_score_hits(self._h, program._h, db._h, hits.data_ptr(), n, letters, out[0].data_ptr(),
                                        out[1].data_ptr(), out[2].data_ptr(), stream.cuda_stream, err, _ERRLEN), err)
            # (the records are read by a kernel queued behind this stream: torch keeps their memory until it has run)
            hits.record_stream(stream)
        return HitScores(*out)

    def _print_args(self, db: Database, hits, scores, names, accepted_only: bool, letters):
        """What print_hits() and list_hits() check first: the records, the score columns, the names (None: the
        database's default table) and the header."""
        import torch
        hits, n, dev, cur, letters = _record_args(db, hits, self.device, self.descr.hit_stride, "scanner",
                                                  "its hits are printed by Replay.batch() or pack()", letters)
        if not isinstance(scores, HitScores):
            raise TypeError(f"scores is a {type(scores).__name__}, not a HitScores")
        if scores.text_bytes is None or scores.text_len is None:
            raise ValueError("scores has no text: the score column of every line is needed, score(..., text=True) delivers it")
        tb, tl, acc = scores.text_bytes, scores.text_len, scores.accept
        if tb.dtype != torch.uint8 or tb.ndim != 2 or int(tb.shape[0]) != n or tb.device != dev or not tb.is_contiguous():
            raise ValueError(f"scores.text_bytes must be a contiguous uint8 tensor [{n}, W] on {dev}")
        if tl.dtype != torch.int32 or tuple(tl.shape) != (n,) or tl.device != dev or not tl.is_contiguous():
            raise ValueError(f"scores.text_len must be a contiguous int32 tensor [{n}] on {dev}")
        if accepted_only and (acc.dtype != torch.bool or tuple(acc.shape) != (n,) or acc.device != dev or not acc.is_contiguous()):
            raise ValueError(f"scores.accept must be a contiguous bool tensor [{n}] on {dev}")
        if names is not None and (not isinstance(names, EntryNames) or not names._h):
            raise ValueError("names: an open EntryNames is needed")
        L = lib()
        head = C.create_string_buffer(1 << 16)
        m = L.rma_print_header(self.descr._h, head, len(head))
        if m < 0 or m >= len(head):
            raise RnamotifError(f"rma_print_header: {m}")
        if names is None:
            # the default table, made on the first such call and kept with the database until it is closed
            names = getattr(db, "_default_names", None)
            if names is None or not names._h:
                names = db._default_names = EntryNames(self, db)
        return hits, n, dev, cur, letters, tb, tl, acc, names, head.raw[:m]

    def print_hits(self, db: Database, hits, scores: HitScores, names: Optional[EntryNames] = None, accepted_only: bool = True,
                   letters: Optional[bytes] = None) -> HitPrint:
        """These records as rnamotif prints them, on the GPU (rma_hit_print; the rule is csrc/rm_hitprint.h's, what
        HitPrinter::print does on the host): a HitPrint whose bytes, behind its header, are what Replay.device() writes
        for the same records and names -- one device-to-host copy and a write away from rnamotif's stdout.  hits, db and
        letters as score() takes them; scores: score(db, hits, program, text=True) of the same records, whose text_bytes
        are the score column of every line (a HitScores without text is refused); names: EntryNames(scanner, db, sids,
        sdefs), default: a table of the default names, made on the first such call and kept with the database until it
        is closed; accepted_only: print scores.accept's records
        (False: every record, a rejected one with the empty score column it has).  The tensors are torch's and ready on
        torch's current stream; the call waits once, for the total length.  A malformed record and a text_len outside
        its row are refused (RnamotifError naming the record) before anything is written.  Score programs the device
        refuses -- HOLD / RELEASE, NAME, carried variables -- keep Replay.device()."""
        import torch
        hits, n, dev, cur, letters, tb, tl, acc, names, head = self._print_args(db, hits, scores, names, accepted_only, letters)
        L = lib()
        nh = names._h
        width = int(tb.shape[1])
        err = C.create_string_buffer(_ERRLEN)
        stream = cur.cuda_stream
        total = C.c_int64(0)
        accept = acc.data_ptr() if accepted_only and n else None
        _check(L.rma_hit_print_size(self._h, db._h, nh, hits.data_ptr() if n else None, n, accept, tl.data_ptr() if n else None,
                                    C.byref(total), stream, err, _ERRLEN), err)
        t = int(total.value)
        p = HitPrint(torch.empty(t, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev), head)
        _check(L.rma_hit_print(self._h, db._h, nh, hits.data_ptr() if n else None, n, letters, accept,
                               tb.data_ptr() if n and width else None, width, tl.data_ptr() if n else None, t,
                               p.bytes.data_ptr() if t else None, p.off.data_ptr(), stream, err, _ERRLEN), err)
        # (the inputs are read by kernels queued behind this stream: torch keeps their memory until those have run)
        for x in (hits, tb, tl) + ((acc,) if accepted_only else ()):
            x.record_stream(cur)
        return p

    def ct_hits(self, db: Database, hits, scores: HitScores, names: Optional[EntryNames] = None, accepted_only: bool = True,
                type: str = "rnamotif", letters: Optional[bytes] = None) -> HitCt:
        """These records as rm2ct writes them, on the GPU (rma_hit_ct; the rule is csrc/rm_hitct.h's): a HitCt whose bytes
        are what `rm2ct` (type="rnamotif") or `rm2ct -t rnaviz` ("rnaviz") writes for print_hits(...).write() of the same
        arguments -- per printed record a header line and a line per base: its number, its letter, its neighbours, its
        partner and its place in the entry.  The partner is the tool's, paired by the words of the '#RM descr' line:
        counted from 0 in p5/p3, -1 in a context -- where hit_structures' mate[:, 0] + 1 differs.  Everything else as
        print_hits() takes it.  The call waits once, for the total length; the fill is queued behind torch's current
        stream.  Refused (RnamotifError) before a record is looked at: a descriptor with a triple or quad helix, with
        the tool's words; a name that is empty or has a blank in it; letters that are no ASCII letters.  Refused naming
        the record, nothing written: a malformed record, a newline in a score column, a hit line of 50 000 bytes or
        more and, for rnaviz, a text behind the name that atof() reads as inf, nan, a 0x or exponent form, or that has
        more than 19 digits."""
        import torch
        types = {"rnamotif": 0, "rnaviz": 1}
        if type not in types:
            raise ValueError(f"type: 'rnamotif' or 'rnaviz', not {type!r}")
        hits, n, dev, cur, letters, tb, tl, acc, names, _ = self._print_args(db, hits, scores, names, accepted_only, letters)
        L = lib()
        width = int(tb.shape[1])
        err = C.create_string_buffer(_ERRLEN)
        stream = cur.cuda_stream
        accept = acc.data_ptr() if accepted_only and n else None
        total = C.c_int64(0)
        first = (self._h, db._h, names._h, hits.data_ptr() if n else None, n, accept, tb.data_ptr() if n and width else None, width,
                 tl.data_ptr() if n else None, types[type], " ".join(self.descr.names()).encode(), letters)
        _check(L.rma_hit_ct_size(*first, C.byref(total), stream, err, _ERRLEN), err)
        t = int(total.value)
        out = HitCt(torch.empty(t, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.int64, device=dev))
        _check(L.rma_hit_ct(*first, t, out.bytes.data_ptr() if t else None, out.off.data_ptr(), stream, err, _ERRLEN), err)
        # (the inputs are read by kernels queued behind this stream: torch keeps their memory until those have run)
        for x in (hits, tb, tl) + ((acc,) if accepted_only else ()):
            x.record_stream(cur)
        return out

    def list_hits(self, db: Database, hits, scores: HitScores, names: Optional[EntryNames] = None, accepted_only: bool = True,
                  letters: Optional[bytes] = None, name: str = "whole", smax: Optional[int] = None) -> HitList:
        """These records as rmfmt lists them, on the GPU (rma_hit_list; the rule is csrc/rm_hitlist.h's): a HitList
        whose lines, behind its header, are what `rmfmt` (name="whole"), `rmfmt -l` ("locus") or `rmfmt -la` ("acc")
        writes for print_hits(...).write() of the same arguments -- the hits best score first where the score column is
        one number, else by name and position, every field padded to its widest instance, long elements abbreviated.
        smax: rmfmt's -smax, default 30 000 000: a listing whose temp lines have more bytes keeps the input order.
        Everything else as print_hits() takes it.  The call waits twice, for the listing's shape each time; the sort and
        the fill are queued behind torch's current stream.  Refused (RnamotifError naming the record or the entry)
        before anything is written: a malformed record, records whose score columns do not all have the same number
        (at least one) of fields, a newline in a score column, a name that is empty or has a blank in it."""
        import torch
        modes = {"whole": 0, "locus": 1, "acc": 2}
        if name not in modes:
            raise ValueError(f"name: 'whole', 'locus' or 'acc', not {name!r}")
        hits, n, dev, cur, letters, tb, tl, acc, names, head = self._print_args(db, hits, scores, names, accepted_only, letters)
        L = lib()
        width = int(tb.shape[1])
        err = C.create_string_buffer(_ERRLEN)
        stream = cur.cuda_stream
        accept = acc.data_ptr() if accepted_only and n else None
        n_lines, line_len, mode = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        widths = np.zeros(107, dtype=np.int32)
        first = (self._h, db._h, names._h, hits.data_ptr() if n else None, n, accept, tb.data_ptr() if n and width else None, width,
                 tl.data_ptr() if n else None, modes[name], int(smax) if smax is not None else 0)
        _check(L.rma_hit_list_shape(*first, C.byref(n_lines), C.byref(line_len), widths.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(mode),
                                    stream, err, _ERRLEN), err)
        m, ll = int(n_lines.value), int(line_len.value)
        out = HitList(torch.empty((m, ll), dtype=torch.uint8, device=dev), torch.empty(m, dtype=torch.int64, device=dev), int(mode.value),
                      widths[:ll - int(widths.sum())].copy(), head)      # (a line: the widths, a blank or the newline behind each)
        _check(L.rma_hit_list(*first, letters, m, ll, out.lines.data_ptr() if m else None, out.perm.data_ptr() if m else None,
                              stream, err, _ERRLEN), err)
        # (the inputs are read by kernels queued behind this stream: torch keeps their memory until those have run)
        for x in (hits, tb, tl) + ((acc,) if accepted_only else ()):
            x.record_stream(cur)
        return out

    def seq_check(self, db: Database, hits, check: Optional[SeqCheck] = None, letters: Optional[bytes] = None, budget: int = 0,
                  fixed: bool = True) -> SeqChecked:
        """The loose seq= expressions of the descriptor applied to the element text of each of these records, on the
        GPU (rma_seqcheck_hits; the rule is csrc/rm_seqcheck.h's, what the replay does on the host): a SeqChecked, so
        that r.hits[r.keep] -- rnamotif's candidates -- go on to score() with ScoreProgram(descr, checked=True),
        prune(), hit_structures(), align() without a trip to the host.  For a descriptor that is not loose every
        record is kept.  hits: int32 CUDA tensor [n, hit_stride] on the scanner's device, any rows of a scan's records
        in any order; db: the database_from_tensor() / database_from_fasta_tensor() database they are of; check:
        SeqCheck(descr) of this scanner's descriptor (default: one made on first use and kept by the scanner);
        letters as Replay.device() takes them; budget: the ops one record may visit, 0 for 2^20; fixed=False: no rows,
        only keep.  The call waits once.  A malformed record, and a record that needs more than the budget, raise
        RnamotifError naming the lowest such record; nothing is written then."""
        import torch
        hits, n, dev, stream, letters = _record_args(db, hits, self.device, self.descr.hit_stride, "scanner",
                                                    "its records are checked by Replay.batch() or pack()", letters)
        if check is None:
            check = getattr(self, "_seq_check", None)
            if check is None or not check._h:
                check = self._seq_check = SeqCheck(self.descr)
        if not isinstance(check, SeqCheck) or not check._h:
            raise ValueError("check: an open SeqCheck is needed")
        if int(budget) < 0:
            raise ValueError(f"budget is {budget}")
        keep = torch.empty(n, dtype=torch.bool, device=dev)
        rows = torch.empty((n, self.descr.hit_stride), dtype=torch.int32, device=dev) if fixed else None
        if n:
            err = C.create_string_buffer(_ERRLEN)
            _check(lib().rma_seqcheck_hits(self._h, check._h, db._h, hits.data_ptr(), n, letters, int(budget), keep.data_ptr(),
                                           rows.data_ptr() if fixed else None, stream.cuda_stream, err, _ERRLEN), err)
            # (the records are read by a kernel queued behind this stream: torch keeps their memory until it has run)
            hits.record_stream(stream)
        return SeqChecked(keep, rows)

    def load_energy_tables(self, dir: str = EFNDATA_DIR, efn: bool = True, efn2: bool = True) -> None:
        """The tables of efn() and / or efn2() from a directory onto the scanner's GPU (rma_scanner_load_energy_tables),
        for structure_energies() of a scanner whose descriptor has no such call in its score section.  No scan changes."""
        which = (1 if efn else 0) | (2 if efn2 else 0)
        if which:
            err = C.create_string_buffer(_ERRLEN)
            _check(lib().rma_scanner_load_energy_tables(self._h, os.fsencode(dir), which, err, _ERRLEN), err)

    def structure_energies(self, off, base, pair, letters: Optional[bytes] = None, efn: bool = True, efn2: bool = True):
        """efn() and efn2() of a batch of structures in tensors on the scanner's GPU (rma_structure_energies; the rule is
        csrc/rm_structenergy.h's), as the reference's efn_drv and efn2_drv give them for a .ct file: (efn, efn2), int32
        tensors [n] in 1/100 kcal/mol, None for an energy not asked for; 16000 / 9999999 where the energy is infinite
        (also: no bases, crossing pairs, a pair (i, i+1)).  off: int64 [n+1], structure s is [off[s], off[s+1]) of
        base and pair; base: uint8 / int8 [T] letters (letters: 256 bytes, byte -> letter, default the readers');
        pair: int32, [T] -- any stride -- or [T, k] whose column 0 is read in place: the index inside its structure
        of the base each base pairs with, or -1, as HitStructures.mate.  Pairs are taken as given.  The tables are
        the descriptor's or those of load_energy_tables().  The tensors are ready on torch's current stream; the call
        waits once, for the check of every structure.  A malformed structure is refused (RnamotifError naming the
        lowest bad index and the reason) before anything is written."""
        import torch
        for name, t, dtypes in (("off", off, (torch.int64,)), ("base", base, (torch.uint8, torch.int8)), ("pair", pair, (torch.int32,))):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{name} is a {type(t).__name__}, not a torch.Tensor")
            if t.device.type != "cuda" or (t.device.index if t.device.index is not None else torch.cuda.current_device()) != self.device:
                raise ValueError(f"{name} is on {t.device}: the scanner is on cuda:{self.device}")
            if t.dtype not in dtypes:
                raise TypeError(f"{name} is {t.dtype}: {' or '.join(str(d) for d in dtypes)} is needed")
        if off.ndim != 1 or off.numel() < 1:
            raise ValueError(f"off has shape {tuple(off.shape)}: [n + 1] offsets are needed")
        if base.ndim != 1 or pair.ndim not in (1, 2) or int(pair.shape[0]) != int(base.shape[0]) or (pair.ndim == 2 and int(pair.shape[1]) < 1):
            raise ValueError(f"base has shape {tuple(base.shape)}, pair {tuple(pair.shape)}: [T] letters and [T] or [T, k] partners are needed")
        if letters is not None and len(letters) != 256:
            raise ValueError(f"letters: 256 bytes are needed, not {len(letters)}")
        off, base = off.contiguous(), base.contiguous()
        n, total = int(off.shape[0]) - 1, int(base.shape[0])
        stride = int(pair.stride(0)) if total > 1 else 1
        if total > 1 and stride < 1:
            pair = pair.contiguous()
            stride = int(pair.stride(0))
        dev = torch.device("cuda", self.device)
        cur = torch.cuda.current_stream(dev)
        e = torch.empty(n, dtype=torch.int32, device=dev) if efn else None
        e2 = torch.empty(n, dtype=torch.int32, device=dev) if efn2 else None
        if n:
            err = C.create_string_buffer(_ERRLEN)
            _check(lib().rma_structure_energies(self._h, off.data_ptr(), base.data_ptr() if total else None,
                                                pair.data_ptr() if total else None, stride, n, total, letters,
                                                e.data_ptr() if efn else None, e2.data_ptr() if efn2 else None,
                                                cur.cuda_stream, err, _ERRLEN), err)
            # (the tensors are read by kernels queued on this stream: torch keeps their memory until those have run)
            for t in (off, base, pair):
                t.record_stream(cur)
        return e, e2

    def set_option(self, name: str, value: int) -> None:
        """A launch-shape / diagnostic switch between scans (rma_scanner_set_option); the RNAMOTIF_*
        environment is read once, when the scanner is created."""
        err = C.create_string_buffer(_ERRLEN)
        _check(lib().rma_scanner_set_option(self._h, name.encode(), int(value), err, _ERRLEN), err)

    def forget_last(self) -> None:
        """The last scan's records are no longer there for Comm.gather (a round in which this rank has no entries)."""
        self.set_option("forget_last", 1)

    def warmup(self) -> None:
        err = C.create_string_buffer(_ERRLEN)
        _check(lib().rma_scanner_warmup(self._h, err, _ERRLEN), err)

    def attach(self, db: Database) -> None:
        """Lay db out for this scanner ahead of its first scan of it (rma_db_attach)."""
        err = C.create_string_buffer(_ERRLEN)
        _check(lib().rma_db_attach(self._h, db._h, err, _ERRLEN), err)

    def scan_begin(self, db: Database) -> None:
        """The search kernel on its way (rma_scan_begin); scan_end() returns the records."""
        err = C.create_string_buffer(_ERRLEN)
        _check(lib().rma_scan_begin(self._h, db._h, err, _ERRLEN), err)

    def scan_end(self, copy: bool = True) -> np.ndarray:
        """The records of the scan begun with scan_begin(), as scan() returns them.  With copy=False the array is a view of
        the scanner's own buffer, valid until THIS scanner's next scan_begin() (or scan()): from its second scan on a scanner's
        begin already writes that buffer, or replaces it -- read the records before beginning the scanner's next scan."""
        L = lib()
        hits = C.POINTER(C.c_int32)()
        n = C.c_int64()
        err = C.create_string_buffer(_ERRLEN)
        _check(L.rma_scan_end(self._h, C.byref(hits), C.byref(n), err, _ERRLEN), err)
        return self._records(hits, n.value, copy)

    def scan_end_on_device(self) -> int:
        """End the scan in flight leaving the ordered records in HBM (for Comm.gather); their number."""
        d = C.c_void_p()
        n = C.c_int64()
        err = C.create_string_buffer(_ERRLEN)
        _check(lib().rma_scan_end_on_device(self._h, C.byref(d), C.byref(n), err, _ERRLEN), err)
        return n.value

    def _records(self, hits, n: int, copy: bool) -> np.ndarray:
        stride = self.descr.hit_stride
        if n == 0:
            return np.zeros((0, stride), dtype=np.int32)
        a = np.ctypeslib.as_array(hits, shape=(n * stride,)).reshape(n, stride)
        return a.copy() if copy else a

    def scan(self, db: Database, copy: bool = True) -> np.ndarray:
        """All candidates of db in reference order: int32 array [n, hit_stride].  With
        copy=False the array is a view of the scanner's own buffer, valid until its next scan begins (scan(), scan_begin()).
        When descr.loose > 0 the records are a superset of rnamotif's candidates until replayed."""
        L = lib()
        hits = C.POINTER(C.c_int32)()
        n = C.c_int64()
        err = C.create_string_buffer(_ERRLEN)
        _check(L.rma_scan(self._h, db._h, C.byref(hits), C.byref(n), err, _ERRLEN), err)
        return self._records(hits, n.value, copy)

    def scan_device(self, db: Database) -> Tuple[int, float, float]:
        """Device part only: (candidates, search kernel ms, efn kernel ms)."""
        L = lib()
        n = C.c_int64()
        ms1, ms2 = C.c_float(), C.c_float()
        err = C.create_string_buffer(_ERRLEN)
        _check(L.rma_scan_device(self._h, db._h, C.byref(n), C.byref(ms1), C.byref(ms2), err, _ERRLEN), err)
        return n.value, ms1.value, ms2.value

    def last_kernel_ms(self) -> Tuple[float, float, float]:
        """(search kernel, drain kernel, efn kernel) of the last search in ms; 0 for a kernel that did not run."""
        ms = (C.c_float * 3)()
        err = C.create_string_buffer(_ERRLEN)
        _check(lib().rma_scanner_last_kernel_ms(self._h, ms, err, _ERRLEN), err)
        return ms[0], ms[1], ms[2]

    def last_launch(self) -> Tuple[int, int, int, int]:
        """(search workgroups, bytes of dynamic LDS a workgroup, drain workgroups, beside) of the last search launch
        (rma_scanner_last_launch); beside is 1 when the shape leaves another scanner's drain kernel room."""
        out = (C.c_int * 4)()
        lib().rma_scanner_last_launch(self._h, out)
        return out[0], out[1], out[2], out[3]

    def last_end(self) -> Tuple[int, int, int, int]:
        """(host waits, 1 if the records of the tail enqueued at scan_begin were taken, search launches, energy launches)
        of the last scan ended (rma_scanner_last_end)."""
        out = (C.c_int * 4)()
        lib().rma_scanner_last_end(self._h, out)
        return out[0], out[1], out[2], out[3]

    def close(self) -> None:
        if getattr(self, "_seq_check", None) is not None:
            self._seq_check.close()
            self._seq_check = None
        if self._h:
            lib().rma_scanner_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Replay:
    """Score program + hit printer over candidate records (host side)."""

    def __init__(self, descr: Descriptor, out_path: str = "-"):
        L = lib()
        h = C.c_void_p()
        err = C.create_string_buffer(_ERRLEN)
        _check(L.rma_replay_open(descr._h, out_path.encode(), C.byref(h), err, _ERRLEN), err)
        self._h = h
        self.descr = descr

    def batch(self, sids: Sequence[bytes], sdefs: Sequence[bytes], seqs: Sequence[bytes],
              hits: np.ndarray) -> int:
        L = lib()
        hits = np.ascontiguousarray(hits, dtype=np.int32)
        lens = (C.c_int32 * max(len(seqs), 1))(*[len(s) for s in seqs])
        printed = C.c_int64()
        err = C.create_string_buffer(_ERRLEN)
        _check(L.rma_replay_batch(self._h, _cstr_array(sids), _cstr_array(sdefs), _cstr_array(seqs), lens,
                                  len(seqs), hits.ctypes.data_as(C.POINTER(C.c_int32)), hits.shape[0],
                                  C.byref(printed), err, _ERRLEN), err)
        return printed.value

    def pack(self, pack: "Pack", hits: np.ndarray, first: int = 0) -> int:
        """Candidates over a packed database (word 0 of a record: entry number minus first)."""
        L = lib()
        hits = np.ascontiguousarray(hits, dtype=np.int32)
        printed = C.c_int64()
        err = C.create_string_buffer(_ERRLEN)
        _check(L.rma_replay_pack(self._h, pack._h, first, hits.ctypes.data_as(C.POINTER(C.c_int32)), hits.shape[0],
                                 C.byref(printed), err, _ERRLEN), err)
        return printed.value

    def device(self, db: Database, hits, sids: Optional[Sequence[bytes]] = None, sdefs: Optional[Sequence[bytes]] = None,
               letters: Optional[bytes] = None, accepted: bool = False):
        """Candidates of a database made by Scanner.database_from_tensor(), replayed from its text on the GPU
        (rma_replay_device): only each record's window -- the bases its elements and contexts cover -- is cut out
        on the device and copied to the host.  hits: int32 CUDA tensor [n, hit_stride] on the database's device,
        scan_tensor()'s output or rows of it, printed in the order given.  sids / sdefs: one per entry (default:
        the entry's number, "").  letters: 256 bytes, byte -> letter; default: the database's alphabet= (value i
        -> alphabet[i] as the readers take it, anything else n), else the readers' letters.  Runs behind the work
        queued on torch's current stream.  Returns the number printed, or (that number, np.bool_ mask of the
        records printed) with accepted=True."""
        hits, n, _, cur, letters = _record_args(db, hits, None, self.descr.hit_stride, "replay",
                                                "replay it with batch() or pack()", letters)
        for what, names in (("sids", sids), ("sdefs", sdefs)):
            if names is not None and len(names) != db.n_seqs:
                raise ValueError(f"{what}: one per entry, {db.n_seqs}, not {len(names)}")
        mask = np.zeros(max(n, 1), dtype=np.uint8)
        printed = C.c_int64()
        err = C.create_string_buffer(_ERRLEN)
        stream = cur.cuda_stream
        _check(lib().rma_replay_device(self._h, db._h, hits.data_ptr() if n else None, n, letters,
                                       _cstr_array(sids) if sids is not None else None,
                                       _cstr_array(sdefs) if sdefs is not None else None, stream, C.byref(printed),
                                       mask.ctypes.data, err, _ERRLEN), err)
        if accepted:
            return printed.value, mask[:n].astype(np.bool_)
        return printed.value

    def close(self) -> None:
        if self._h:
            err = C.create_string_buffer(_ERRLEN)
            rc = lib().rma_replay_close(self._h, err, _ERRLEN)
            self._h = None
            _check(rc, err)


class Comm:
    """The native gather of a multi-GPU search (rma_comm_*, rma_gather_hits): RCCL behind the C ABI.
    One per process.  `broadcast(buf: bytearray)` hands rank 0's 128-byte id to every rank -- with
    torch.distributed: a broadcast of a uint8 tensor (rnamotif_amd/distributed.py does that)."""

    def __init__(self, rank: int, world: int, device: int, broadcast=None):
        L = lib()
        ident = C.create_string_buffer(128)
        err = C.create_string_buffer(_ERRLEN)
        if world > 1:
            if rank == 0:
                _check(L.rma_comm_unique_id(ident, err, _ERRLEN), err)
            raw = bytearray(ident.raw)
            broadcast(raw)
            ident = C.create_string_buffer(bytes(raw), 128)
        h = C.c_void_p()
        _check(L.rma_comm_create(ident, rank, world, device, C.byref(h), err, _ERRLEN), err)
        self._h = h
        self.rank, self.world = rank, world

    def gather(self, scanner: Scanner, global_index: Sequence[int], root: int = 0):
        """The records of every rank's last scan (left in HBM) to `root`: (records [n, stride] on root --
        rank by rank, each part in order -- else empty, counts per rank)."""
        L = lib()
        idx = np.ascontiguousarray(np.asarray(global_index, dtype=np.int32))
        hits = C.POINTER(C.c_int32)()
        n = C.c_int64()
        counts = (C.c_int64 * self.world)()
        err = C.create_string_buffer(_ERRLEN)
        _check(L.rma_gather_hits(self._h, scanner._h, idx.ctypes.data_as(C.POINTER(C.c_int32)), len(idx), root,
                                 C.byref(hits), C.byref(n), counts, err, _ERRLEN), err)
        return scanner._records(hits, n.value, True), [int(c) for c in counts]

    def count(self) -> int:
        """The number of ranks the transport itself reports (RCCL: ncclCommCount)."""
        n = C.c_int()
        err = C.create_string_buffer(_ERRLEN)
        _check(lib().rma_comm_count(self._h, C.byref(n), err, _ERRLEN), err)
        return n.value

    def close(self) -> None:
        if self._h:
            lib().rma_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sort_hits(hits: np.ndarray) -> np.ndarray:
    """Hit records [n, stride] (from several scans, word 0 the database-wide entry number) in the
    reference's output order, order word renumbered: rma_sort_hits()."""
    h = np.ascontiguousarray(hits, dtype=np.int32)
    if h.ndim != 2:
        raise ValueError("hit records are [n, stride]")
    out = np.empty_like(h)
    err = C.create_string_buffer(512)
    i32p = C.POINTER(C.c_int32)
    _check(lib().rma_sort_hits(h.ctypes.data_as(i32p), h.shape[0], h.shape[1], out.ctypes.data_as(i32p), err, len(err)), err)
    return out


def read_fasta(path: str) -> List[Tuple[bytes, bytes, bytes]]:
    """(sid, sdef, seq) per record with the reference reader's normalisation
    (dbutil.c:42-128: every alpha character kept, lower case, u -> t).  Used by
    tests and the benchmark; the CLI has its own C++ reader."""
    import gzip
    op = gzip.open if path.endswith(".gz") else open
    recs: List[Tuple[bytes, bytes, bytes]] = []
    sid = sdef = None
    chunks: List[bytes] = []
    table = bytes(((c | 0x20) if (65 <= c <= 90) else c) for c in range(256)).replace(b"u", b"t")
    keep = bytes(c for c in range(256) if chr(c).isalpha() and c < 128)
    drop = bytes(c for c in range(256) if c not in keep)
    with op(path, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                if sid is not None:
                    recs.append((sid, sdef, b"".join(chunks)))
                hdr = line[1:].strip().split(None, 1)
                sid = hdr[0] if hdr else b""
                sdef = hdr[1].rstrip() if len(hdr) > 1 else b""
                chunks = []
            else:
                chunks.append(line.translate(table, drop))
        if sid is not None:
            recs.append((sid, sdef, b"".join(chunks)))
    return recs


class Pack:
    """A packed database on disk (rma_pack_*): what the readers deliver, in the
    layout the scanner keeps in HBM."""

    def __init__(self, path: Optional[str] = None, _handle=None):
        L = lib()
        h = _handle if _handle is not None else C.c_void_p()
        if _handle is None:
            err = C.create_string_buffer(_ERRLEN)
            _check(L.rma_pack_open(path.encode(), C.byref(h), err, _ERRLEN), err)
        self._h = h
        self.count = int(L.rma_pack_count(h))
        self.bases = int(L.rma_pack_bases(h))

    @staticmethod
    def read(paths: Sequence[str], fmt: str = "", maxslen: int = 0, threads: int = 0) -> "Pack":
        """Sequence files (or packed databases) read the way rnamotif reads them, into memory
        (rma_pack_read): -fmt, -N and every quirk of the reference's readers included."""
        L = lib()
        h = C.c_void_p()
        err = C.create_string_buffer(_ERRLEN)
        arr = _cstr_array([p.encode() for p in paths])
        _check(L.rma_pack_read(arr, len(paths), fmt.encode() if fmt else None, maxslen, threads, C.byref(h), err, _ERRLEN), err)
        return Pack(_handle=h)

    @staticmethod
    def read_entries(paths: Sequence[str], entries: Sequence[int], fmt: str = "", maxslen: int = 0, threads: int = 0) -> Optional["Pack"]:
        """Only the entries with these numbers (ascending; numbered over all files as database_index()
        counts them), read and packed (rma_pack_read_entries); None when the files can only be read whole."""
        L = lib()
        h = C.c_void_p()
        err = C.create_string_buffer(_ERRLEN)
        arr = _cstr_array([p.encode() for p in paths])
        ent = (C.c_int32 * max(len(entries), 1))(*[int(e) for e in entries])
        rc = L.rma_pack_read_entries(arr, len(paths), fmt.encode() if fmt else None, maxslen, threads, ent, len(entries), C.byref(h), err, _ERRLEN)
        if rc == 2:
            return None
        _check(rc, err)
        return Pack(_handle=h)

    def pin(self) -> None:
        """Page-lock the packed words: uploads from this pack are DMA, asynchronous (rma_pack_pin)."""
        err = C.create_string_buffer(_ERRLEN)
        _check(lib().rma_pack_pin(self._h, err, _ERRLEN), err)

    def lengths(self) -> List[int]:
        L = lib()
        return [int(L.rma_pack_slen(self._h, i)) for i in range(self.count)]

    @staticmethod
    def write(path: str, records: Sequence[Tuple[bytes, bytes, bytes]]) -> None:
        """records: (sid, sdef, seq) as read_fasta() returns them."""
        L = lib()
        n = len(records)
        sids = _cstr_array([r[0] for r in records])
        sdefs = _cstr_array([r[1] for r in records])
        seqs = _cstr_array([r[2] for r in records])
        slens = (C.c_int32 * max(n, 1))(*[len(r[2]) for r in records])
        err = C.create_string_buffer(_ERRLEN)
        _check(L.rma_pack_write(path.encode(), sids, sdefs, seqs, slens, n, err, _ERRLEN), err)

    def record(self, i: int) -> Tuple[bytes, bytes, bytes]:
        L = lib()
        n = int(L.rma_pack_slen(self._h, i))
        if n < 0:
            raise IndexError(i)
        buf = C.create_string_buffer(n + 1)
        L.rma_pack_seq(self._h, i, buf)
        return (C.string_at(L.rma_pack_sid(self._h, i)), C.string_at(L.rma_pack_sdef(self._h, i)), buf.raw[:n])

    def seq(self, i: int) -> bytes:
        """Entry i's sequence text, unpacked on the host: the readers' letters."""
        return self.record(i)[2]

    def close(self) -> None:
        if self._h:
            lib().rma_pack_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def database_index(paths: Sequence[str], fmt: str = "", threads: int = 0) -> Optional[List[int]]:
    """The entries of the sequence files, in order, each with an upper bound of its length -- without
    reading the database (rma_database_index); None when the files can only be read whole."""
    L = lib()
    ext = C.POINTER(C.c_int64)()
    n = C.c_int32()
    err = C.create_string_buffer(_ERRLEN)
    arr = _cstr_array([p.encode() for p in paths])
    rc = L.rma_database_index(arr, len(paths), fmt.encode() if fmt else None, threads, C.byref(ext), C.byref(n), err, _ERRLEN)
    if rc == 2:
        return None
    _check(rc, err)
    out = [int(ext[i]) for i in range(n.value)]
    L.rma_free(ext)
    return out


def synthetic_records(k: int, length: int = 1_000_000, seed: int = 20240601) -> List[bytes]:
    """BASELINE.md / SURVEY.md section 8d synthetic database: k records of
    iid uniform acgt from numpy default_rng(seed); the first 10 records of the
    default parameters are the survey's syn10M."""
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"acgt", dtype=np.uint8)
    return [lut[rng.integers(0, 4, size=length)].tobytes() for _ in range(k)]


def write_synthetic_fasta(path: str, k: int, length: int = 1_000_000, seed: int = 20240601) -> str:
    """The synthetic database as a FASTA file in the layout SURVEY.md section 8d
    fixes (ids syn%04d, upper case, 50 columns); k=10 gives the survey's syn10M
    (md5 d33c2542e515346e1d0fdfc9edcc5658).  Returns the md5 of the file."""
    import hashlib
    h = hashlib.md5()
    with open(path, "wb") as f:
        for i, s in enumerate(synthetic_records(k, length, seed)):
            head = b">syn%04d synthetic uniform ACGT seed=%d len=%d\n" % (i, seed, length)
            a = np.frombuffer(s.upper(), dtype=np.uint8)
            full = (len(a) // 50) * 50
            body = np.concatenate([a[:full].reshape(-1, 50),
                                   np.full((full // 50, 1), 10, dtype=np.uint8)], axis=1).tobytes()
            if full < len(a):
                body += a[full:].tobytes() + b"\n"
            f.write(head)
            f.write(body)
            h.update(head)
            h.update(body)
    return h.hexdigest()
