"""FASTQ file <-> .fqz5 file on the GPU: the container
fqzcomp5 writes, produced and read by this library alone.

    compress_file(src, dst, level[, src2=])  FASTQ text -> HBM -> fqz5_fastq_index /
                                     blocks / gather (fastq.hip) -> the
                                     section coder with the level's trial
                                     (sections.encode_run) -> whole blocks
                                     (fqz5_blocks_assemble) -> file
    decompress_file(src, dst[, dst2=])  file -> HBM -> fqz5_block_parse ->
                                     sections decoded -> fqz5_fastq_format
                                     (_pairs: deinterleaved to two files)
    compress_paired_bytes / decompress_paired_bytes: the same for R1/R2
    pairs (encode_interleaved / decode_deinterleaved, fqzcomp5.c:3211,
    :4049): records interleaved R1, R2, R1, ... with READ2 on the R2 ones.
    extract_file(src, dst, first, count[, dst2=]) / extract_bytes: records
                                     [first, first + count) (dst2: pairs)
                                     through the block index: read_index ->
                                     cover -> only the covering blocks read,
                                     checked against the index and decoded
                                     -> fqz5_fastq_format_range (the text of
                                     the wanted records, laid out on the
                                     device); with_qual=False: no quality
                                     section decoded, FASTA text
    find_names(src, names) / extract_names_file(src, dst, names[, dst2=]) /
    extract_names_bytes: records by read name, in one pass over the file:
                                     every block read and checked, only its
                                     name section decoded, the names matched
                                     against the query table on the device
                                     (fqz5_names_match) -> sequence and
                                     quality decoded for the blocks with hits
                                     only -> fqz5_fastq_format_list (the hit
                                     records' text, in file order)
    find_seqs(src, patterns) / extract_seqs_file(src, dst, patterns[, dst2=]) /
    extract_seqs_bytes: records by sequence content, the same pass with the
                                     sequence section as the key: decoded for
                                     every block and scanned on the device for
                                     the patterns (fqz5_seqs_match) -> names
                                     and quality decoded for the blocks with
                                     hits only -> fqz5_fastq_format_list
    stats(src)                       read QC statistics in one pass: sequence
                                     and quality sections decoded, histogrammed
                                     on the device (fqz5_stats_add); no names,
                                     no text, only the tables come back
    filter_records(src, Filter(...)) / filter_file(src, dst, flt[, dst2=]) /
    filter_bytes: records by read metrics (length, N count, mean quality,
                                     low-quality share, GC, complexity), the
                                     same pass with the sections the criteria
                                     need as keys; summed and picked on the
                                     device (fqz5_filter_match) -> the other
                                     sections decoded for the blocks with kept
                                     records only -> fqz5_fastq_format_list

File layout (fqzcomp5.c:2563-2630, :2959-2969): "FQZ5\\1\\1\\0\\0", u64 index
offset, the blocks, then "FQZ5IDX\\0", u32 nblocks and per block {u64 file
offset, u32 bases, u32 records}.  The reference reads the index only for
--inspect; here read_index / cover / extract_file use it for record ranges
(files without one are walked by their block size fields).  Encoding follows
a single-threaded (-t1) reference run: the codec trial runs over the blocks
in file order, so the file equals the reference CLI's `-<level> -t1` output
byte for byte.

Scope: 4-line FASTQ, wrapped (multi-line) FASTQ as kseq_read reads it
(kseq.h:194-216; fastq.hip's record chain) and FASTA with any line wrapping
(text starting with '>': blocks without a quality section, decoded to
output_fasta's one-line text, fqzcomp5.c:2258-2264, :3503-3517).  Files of
any size stream through in windows of whole records (see below), on one or
several ranks; over several ranks a window of 4-line FASTQ or FASTA is read
once (each rank its share), a window holding wrapped FASTQ whole by every
rank.  Refused with an error (there is no host parse): the two layouts of
kseq's that fastq.hip does not follow (a lone '\\r' line before a block's
first kept byte, kseq.h:141; bytes between records, :180-186).
"""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

from . import lib as _lib
from . import sections as S

MAGIC = b"FQZ5\x01\x01\x00\x00"                 # fqzcomp5.c:156
INDEX_MAGIC = b"FQZ5IDX\x00"                    # :158


class FastqRec(C.Structure):
    """fqz5_fastq_rec (include/fqz5_fastq.h)"""
    _fields_ = [("name", C.c_uint64), ("comment", C.c_uint64), ("seq", C.c_uint64),
                ("qual", C.c_uint64), ("name_len", C.c_uint32), ("comment_len", C.c_uint32),
                ("seq_len", C.c_uint32), ("fasta", C.c_uint32), ("end", C.c_uint64)]


_bound = False


def _load():
    global _bound
    so = _lib.load()
    if not _bound:
        so.fqz5_fastq_index.restype = C.c_int
        so.fqz5_fastq_index.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                        C.POINTER(C.c_uint64), C.c_void_p]
        so.fqz5_fastq_index_any.restype = C.c_int
        so.fqz5_fastq_index_any.argtypes = so.fqz5_fastq_index.argtypes
        so.fqz5_fastq_record_ends.restype = C.c_int
        so.fqz5_fastq_record_ends.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p,
                                              C.c_uint64, C.POINTER(C.c_uint64)]
        so.fqz5_fastq_blocks.restype = C.c_int
        so.fqz5_fastq_blocks.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int]
        so.fqz5_fastq_gather.restype = C.c_int
        so.fqz5_fastq_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.POINTER(C.c_uint64)]
        so.fqz5_fastq_format.restype = C.c_int
        so.fqz5_fastq_format.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_uint64, C.c_int, C.c_void_p,
                                         C.c_uint64, C.POINTER(C.c_uint64)]
        so.fqz5_fastq_format_pairs.restype = C.c_int
        so.fqz5_fastq_format_pairs.argtypes = so.fqz5_fastq_format.argtypes + [
            C.POINTER(C.c_uint64)]
        so.fqz5_fastq_format_range.restype = C.c_int
        so.fqz5_fastq_format_range.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64,
                                               C.c_int, C.c_int, C.c_void_p, C.c_uint64,
                                               C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        so.fqz5_fastq_format_list.restype = C.c_int
        so.fqz5_fastq_format_list.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                              C.c_int, C.c_int, C.c_void_p, C.c_uint64,
                                              C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        so.fqz5_names_table_build.restype = C.c_void_p
        so.fqz5_names_table_build.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_int]
        so.fqz5_names_table_free.restype = None
        so.fqz5_names_table_free.argtypes = [C.c_void_p]
        so.fqz5_names_table_find.restype = C.c_int64
        so.fqz5_names_table_find.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64]
        so.fqz5_names_match_window.restype = C.c_uint32
        so.fqz5_names_match_window.argtypes = []
        so.fqz5_names_match.restype = C.c_int
        so.fqz5_names_match.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int,
                                        C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        so.fqz5_seqs_table_build.restype = C.c_void_p
        so.fqz5_seqs_table_build.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int]
        so.fqz5_seqs_table_free.restype = None
        so.fqz5_seqs_table_free.argtypes = [C.c_void_p]
        so.fqz5_seqs_table_anchor.restype = C.c_uint32
        so.fqz5_seqs_table_anchor.argtypes = [C.c_void_p]
        so.fqz5_seqs_match_tile.restype = C.c_uint32
        so.fqz5_seqs_match_tile.argtypes = []
        so.fqz5_seqs_scan_host.restype = C.c_int
        so.fqz5_seqs_scan_host.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_void_p,
                                           C.c_uint64, C.c_void_p, C.c_void_p]
        so.fqz5_seqs_match.restype = C.c_int
        so.fqz5_seqs_match.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                       C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                                       C.c_void_p]
        so.fqz5_stats_new.restype = C.c_void_p
        so.fqz5_stats_new.argtypes = [C.c_uint32, C.c_int]
        so.fqz5_stats_free.restype = None
        so.fqz5_stats_free.argtypes = [C.c_void_p]
        so.fqz5_stats_words.restype = C.c_uint64
        so.fqz5_stats_words.argtypes = [C.c_uint32, C.c_int]
        so.fqz5_stats_tile.restype = C.c_uint32
        so.fqz5_stats_tile.argtypes = []
        so.fqz5_stats_add.restype = C.c_int
        so.fqz5_stats_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                      C.c_uint64, C.c_void_p, C.c_void_p]
        so.fqz5_stats_read.restype = C.c_int
        so.fqz5_stats_read.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        so.fqz5_stats_host.restype = C.c_int
        so.fqz5_stats_host.argtypes = [C.c_uint32, C.c_int, C.c_char_p, C.c_char_p, C.c_uint64,
                                       C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                       C.c_void_p]
        so.fqz5_filter_tile.restype = C.c_uint32
        so.fqz5_filter_tile.argtypes = []
        so.fqz5_filter_match.restype = C.c_int
        so.fqz5_filter_match.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                         C.c_uint64, C.c_int, C.c_int, C.c_void_p,
                                         C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p]
        so.fqz5_filter_host.restype = C.c_int
        so.fqz5_filter_host.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_uint64, C.c_void_p,
                                        C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p]
        so.fqz5_trim_cuts.restype = C.c_int
        so.fqz5_trim_cuts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                      C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p]
        so.fqz5_trim_gather.restype = C.c_int
        so.fqz5_trim_gather.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        so.fqz5_trim_host.restype = C.c_int
        so.fqz5_trim_host.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p, C.c_uint64,
                                      C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
        so.fqz5_dedup_table_bytes.restype = C.c_uint64
        so.fqz5_dedup_table_bytes.argtypes = [C.c_uint64]
        so.fqz5_dedup_table_new.restype = C.c_void_p
        so.fqz5_dedup_table_new.argtypes = [C.c_uint64]
        so.fqz5_dedup_table_free.restype = None
        so.fqz5_dedup_table_free.argtypes = [C.c_void_p]
        so.fqz5_dedup_table_slots.restype = C.c_uint64
        so.fqz5_dedup_table_slots.argtypes = [C.c_void_p]
        so.fqz5_dedup_table_reset.restype = C.c_int
        so.fqz5_dedup_table_reset.argtypes = [C.c_void_p]
        so.fqz5_dedup_table_slot.restype = C.c_int
        so.fqz5_dedup_table_slot.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        so.fqz5_dedup_keys.restype = C.c_int
        so.fqz5_dedup_keys.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int,
                                       C.c_int, C.c_void_p]
        so.fqz5_dedup_insert_keys.restype = C.c_int
        so.fqz5_dedup_insert_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                              C.c_void_p]
        so.fqz5_dedup_match.restype = C.c_int
        so.fqz5_dedup_match.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                        C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_void_p,
                                        C.POINTER(C.c_uint64), C.c_void_p]
        so.fqz5_dedup_levels.restype = C.c_int
        so.fqz5_dedup_levels.argtypes = [C.c_void_p, C.c_void_p]
        so.fqz5_dedup_keys_host.restype = C.c_int
        so.fqz5_dedup_keys_host.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int,
                                            C.c_int, C.c_void_p]
        so.fqz5_dedup_host_new.restype = C.c_void_p
        so.fqz5_dedup_host_new.argtypes = []
        so.fqz5_dedup_host_free.restype = None
        so.fqz5_dedup_host_free.argtypes = [C.c_void_p]
        so.fqz5_dedup_host_add.restype = C.c_int
        so.fqz5_dedup_host_add.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int,
                                           C.c_void_p, C.c_void_p]
        so.fqz5_dedup_host_levels.restype = C.c_int
        so.fqz5_dedup_host_levels.argtypes = [C.c_void_p, C.c_void_p]
        _bound = True
    return so


# $FQZ5_FILE_TRACE: host wall time per stage of compress_file /
# decompress_file on stderr (read, upload, parse, gather, codec, assemble,
# download, write; extract_file: index, read, upload, decode, format,
# download, write; find_names / extract_names_file: index, read, upload,
# names (the blocks parsed and CRC-checked, their name sections decoded),
# match, decode, format, download, write; find_seqs / extract_seqs_file: the
# same with seqs, the sequence sections decoded, in place of names, after
# table, the patterns expanded and their table built, and before result, the
# hits mapped back to the caller's patterns; stats: index, read, upload,
# decode, stats, the histogram kernels, and result, the tables' download;
# filter_records / filter_file: index, read, upload, keys (the blocks parsed
# and CRC-checked, their key sections decoded; parse where the criteria need no
# section), filter (the sums and pick kernels), decode, format, download,
# write; trim_records / trim_file: the same with trim, the cuts, the key
# streams' compaction and the filter's kernels, in place of filter, and the
# remaining streams' compaction inside format); dedup_records / dedup_file /
# duplication: the filter's with table, the device table made, after index,
# dedup (the key, insert and pick kernels) in place of filter, and for
# duplication levels, the pass over the table, at the end);
# the stages end with what the library synchronises
_TRACE = {}


class _stage:
    def __init__(self, name: str):
        self.name = name

    def __enter__(self):
        import time
        self.t = time.perf_counter()

    def __exit__(self, *a):
        import time
        _TRACE[self.name] = _TRACE.get(self.name, 0.0) + time.perf_counter() - self.t


def _trace_dump(what: str) -> None:
    import os
    import sys
    if os.environ.get("FQZ5_FILE_TRACE") and _TRACE:
        print(f"[fqz5file] {what}: " + ", ".join(f"{k} {1e3 * v:.1f} ms" for k, v in _TRACE.items()),
              file=sys.stderr, flush=True)
    _TRACE.clear()


def _check(rc, what):
    if rc < 0:
        raise _lib.NativeError(f"{what}: {_lib.last_error()}")
    return rc


def _index_text(text_d, at: int, n: int, wrapped: bool = False):
    """fqz5_fastq_index of text_d[at:at+n]: (records as bytes on the
    device, their load_seqs_kseq sizes, count, is FASTA).  wrapped: any
    layout kseq reads, wrapped FASTQ included (fqz5_fastq_index_any; the
    multi-rank windows, which count records in lines, keep 4-line FASTQ)."""
    import torch
    so = _load()
    part = text_d[at:at + n]
    # records <= lines / 4 (wrapped: / 3, a record without bases), FASTA
    # records <= lines (+1 for a last line without '\n')
    lpr = 1 if n and int(part[0].item()) == ord(">") else (3 if wrapped else 4)
    max_rec = (int((part == 10).sum().item()) + 1) // lpr + 1 if n else 1
    recs = torch.empty(max_rec * C.sizeof(FastqRec), dtype=torch.uint8, device=text_d.device)
    rsz = np.zeros(max_rec, np.uint32)
    nrec = C.c_uint64(0)
    _lib.after_torch(text_d.device)
    fn = so.fqz5_fastq_index_any if wrapped else so.fqz5_fastq_index
    fasta = _check(fn(text_d.data_ptr() + at, n, recs.data_ptr(), max_rec,
                      C.byref(nrec), rsz.ctypes.data), "fqz5_fastq_index") == 1
    nrec = int(nrec.value)
    if at and nrec:                     # offsets into the whole text
        v = recs[:nrec * C.sizeof(FastqRec)].view(torch.int64).view(nrec, -1)
        v[:, :4] += at
        v[:, 6] += at                   # (end)
    return recs[:nrec * C.sizeof(FastqRec)], rsz[:nrec], nrec, fasta


def _seq_lens_of(recs, rids) -> np.ndarray:
    """Sequence lengths of the records `rids` (the device record table)."""
    import torch
    if not len(rids):
        return np.zeros(0, np.uint32)
    w = C.sizeof(FastqRec)
    tab = recs.view(-1, w)
    idx = torch.as_tensor(np.asarray(rids, np.int64), device=recs.device)
    return tab[idx, 40:44].contiguous().view(torch.int32).flatten().cpu().numpy().astype(np.uint32)


def _fasta_blocks(recs, starts, fasta: bool) -> list[bool]:
    """load_seqs_kseq's per-block rule (fqzcomp5.c:574-578, :805-809): a
    block is FASTA (no quality section) when its first record has no
    quality, i.e. in FASTQ text when that record's sequence is empty."""
    if fasta:
        return [True] * len(starts)
    return [bool(x == 0) for x in _seq_lens_of(recs, starts)]


def _gather(text_d, recs, first, fasta: bool, pair_flags: bool):
    """The blocks [first[k], first[k+1]) of the records as a sections.Run,
    every section input gathered in HBM.  pair_flags: READ2 on the odd
    records (load_seqs_interleaved, fqzcomp5.c:763) instead of from the names."""
    return _gather_ranges(text_d, recs, [(int(first[k]), int(first[k + 1]))
                                         for k in range(len(first) - 1)], fasta, pair_flags)


def _blocks(so, sizes: np.ndarray, blk_size: int) -> np.ndarray:
    n = len(sizes)
    first = np.zeros(n + 2, np.uint64)
    sz = np.ascontiguousarray(sizes, np.uint32)
    nb = _check(so.fqz5_fastq_blocks(sz.ctypes.data, n, blk_size, first.ctypes.data, n + 1),
                "fqz5_fastq_blocks")
    return first[:nb + 1]


def parse_fastq(text_d, blk_size: int):
    """FASTQ (or FASTA) text (a device uint8 tensor) -> a sections.Run of
    its blocks, every section input gathered in HBM.  FASTA blocks have no
    quality section (fqzcomp5.c:2237-2264)."""
    so = _load()
    recs, rsz, nrec, fasta = _index_text(text_d, 0, int(text_d.numel()), wrapped=True)
    run = _gather(text_d, recs, _blocks(so, rsz, blk_size), fasta, False)
    del recs
    return run


def parse_paired(text_d, len1: int, blk_size: int):
    """Two files' text in one device buffer (R1 in [0, len1), R2 after it)
    -> the Run of their interleaved records (load_seqs_interleaved,
    fqzcomp5.c:627-848): records R1[0], R2[0], R1[1], ...; a block ends
    before the pair that would take it past blk_size; READ2 on R2 records.
    R2 ending before R1 is an error; R2 records past R1's end are not read."""
    import torch
    so = _load()
    r1, rs1, n1, fa1 = _index_text(text_d, 0, len1, wrapped=True)
    r2, rs2, n2, fa2 = _index_text(text_d, len1, int(text_d.numel()) - len1, wrapped=True)
    if n2 < n1:
        raise _lib.NativeError("unpaired read detected: R2 file ended before R1")
    if n1 and fa1 != fa2:
        raise _lib.NativeError("paired files: one FASTA, one FASTQ")
    w = C.sizeof(FastqRec)
    recs = torch.stack([r1.view(n1, w), r2[:n1 * w].view(n1, w)], 1).reshape(-1) if n1 else r1
    del r1, r2
    pair = rs1.astype(np.uint64) + rs2[:n1].astype(np.uint64)
    if n1 and int(pair.max()) >= 2 ** 32:
        raise _lib.NativeError("paired record larger than 4 GB")
    first = _blocks(so, pair.astype(np.uint32), blk_size) * 2
    run = _gather(text_d, recs, first, fa1, True)
    del recs
    return run


def container(blocks: list[bytes], bases: list[int], nrec: list[int]) -> bytes:
    """The file: header with the index offset, the blocks, the index
    (write_header / write_index, fqzcomp5.c:2563-2630, :2959-2969)."""
    out = [MAGIC, b"\0" * 8]
    off = 16
    idx = []
    for blk, nb, nr in zip(blocks, bases, nrec):
        idx.append(struct.pack("<QII", off, nb, nr))
        out.append(blk)
        off += len(blk)
    if blocks:
        out.append(INDEX_MAGIC + struct.pack("<I", len(blocks)) + b"".join(idx))
    out[1] = struct.pack("<Q", off)
    return b"".join(out)


def _pinned(n: int):
    import torch
    return torch.empty(max(n, 1), dtype=torch.uint8, pin_memory=True)[:n]


def _index(offs, bases, nrec) -> bytes:
    return INDEX_MAGIC + struct.pack("<I", len(offs)) + b"".join(
        struct.pack("<QII", o, nb, nr) for o, nb, nr in zip(offs, bases, nrec))


# ---------------------------------------------------------------------------
# streaming and multi-GPU encode
#
# The reference reads its input block by block (load_seqs_kseq per block,
# fqzcomp5.c:3051, dispatched at :3077) and writes each block behind the
# last, the index at the end (:3108-3115, write_index :2606).  Here the text
# comes in windows of whole records (a FASTQ window ends after 4k lines, a
# FASTA window before a header line); the last block of a window that is not
# the end of the input may be incomplete, so it is not coded: the next window
# starts at its first record.  The codec trial's state carries from window
# to window, so the blocks and their methods are those of one pass over the
# whole input.
#
# Over several ranks (group = a torch.distributed group, one process per
# GPU), every rank reads and parses every window (the block split needs the
# records in order), the window's blocks are split contiguously over the
# ranks, each rank codes its own blocks and its share of the trial blocks'
# work candidates (sections.encode_window), and the blocks are written with
# positioned writes at offsets from an all-gather of the block sizes and an
# exclusive scan; rank 0 writes the header and the index.
# ---------------------------------------------------------------------------
DEFAULT_WINDOW = 2_000_000_000
# Device bytes the encode of a window takes per input byte, by level (the
# arenas' pool peak over the input size, bench.py's arena_bytes.peak): the
# candidates' outputs and the fqz / sequence-model event tables of the trial
# blocks dominate.
FOOTPRINT = {1: 24, 2: 24, 3: 40, 4: 40, 5: 64, 6: 64, 7: 64, 8: 64, 9: 64}


def window_bytes_for(level: int, blk: int, ws: int = 1, hbm: int | None = None) -> int:
    """The encode window: as much input as fits 0.8 x HBM at the level's
    footprint on every rank (each codes about window / ws of it), at least
    two blocks per rank and one over (the last block of a window waits for
    the next), at most 8 GB per rank."""
    if hbm is None:
        import torch
        hbm = torch.cuda.get_device_properties(torch.cuda.current_device()).total_memory \
            if torch.cuda.is_available() else 64 << 30
    per_rank = int(0.8 * hbm) // FOOTPRINT.get(level, 64)
    per_rank = min(per_rank, 8_000_000_000)
    return max(ws * per_rank, 2 * ws * blk + blk)


class _Src:
    """One input read sequentially (plain or gzip; a path or bytes), holding
    the unread text from the start of the next window on (`buf`).

    A plain file is memory-mapped: `buf` is a view of the mapping and the
    window's text goes to the device straight from the page cache in 32 MB
    parts on several threads (fill(device=...)), with no host copy of the
    text to make, fault in and free (the copy ran at ~4.3 GB/s, and freeing
    a 1 GB window's copy took ~90 ms).  gzip and bytes sources keep a host
    buffer."""

    def __init__(self, path: str | None = None, data: bytes | None = None):
        import gzip
        import io
        import os
        self.path, self.gz = path, False
        self.mm = None
        if data is not None:
            self.f = io.BytesIO(data)
            self.size = len(data)
        else:
            with open(path, "rb") as f:
                magic = f.read(2)
            self.gz = magic == b"\x1f\x8b"
            self.f = gzip.open(path, "rb") if self.gz else open(path, "rb")
            self.size = None if self.gz else os.fstat(self.f.fileno()).st_size
            if not self.gz and self.size:
                import mmap
                self.mm = mmap.mmap(self.f.fileno(), 0, access=mmap.ACCESS_READ)
        self.pos = 0                          # bytes read so far (plain / bytes)
        self.base = 0                         # mapped: file offset of buf's start
        self._buf = bytearray()
        self.dev = None                       # fill(device=...): the buffer on the device
        self.eof = False

    @property
    def buf(self):
        if self.mm is not None:
            return memoryview(self.mm)[self.base:self.pos]
        return self._buf

    def fill(self, want: int, device=None) -> None:
        """The buffer up to `want` bytes (or the end of the input).  device
        (a mapped file): also self.dev, the whole buffer on the device
        (otherwise self.dev is None and the caller uploads)."""
        self.dev = None
        if self.mm is not None:
            end = min(self.base + max(want, 0), self.size)
            if end > self.pos:
                self.pos = end
            self.eof = self.pos >= self.size
            if device is not None and self.pos > self.base:
                self.dev = self._upload(device)
            return
        need = want - len(self._buf)
        if need <= 0 or self.eof:
            return
        if self.size is None:                 # gzip: chunks
            while len(self._buf) < want and not self.eof:
                c = self.f.read(min(want - len(self._buf), 1 << 28))
                if not c:
                    self.eof = True
                    break
                self._buf += c
            return
        at = len(self._buf)                   # bytes: into a buffer of the exact size
        left = self.size - self.pos
        want = at + min(need, left)
        nb = bytearray(want)
        nb[:at] = self._buf
        self._buf = nb
        got = self.f.readinto(memoryview(self._buf)[at:want])
        self.pos += got
        if at + got < want:
            del self._buf[at + got:]
        if self.pos >= self.size:
            self.eof = True

    def _upload(self, device):
        """buf on the device: 32 MB parts copied from the mapping by several
        threads (the copies fault the page-cache pages in and release the
        GIL)."""
        import warnings
        from concurrent.futures import ThreadPoolExecutor
        import torch
        a, b = self.base, self.pos
        dev = torch.empty(b - a, dtype=torch.uint8, device=device)
        mv = memoryview(self.mm)
        step = 32 << 20
        parts = [(o, min(o + step, b)) for o in range(a, b, step)]

        def one(p):
            o, e = p
            with warnings.catch_warnings():   # (a read-only mapping: torch only reads it)
                warnings.simplefilter("ignore")
                src = torch.frombuffer(mv[o:e], dtype=torch.uint8)
            dev[o - a:e - a].copy_(src)
        try:
            if len(parts) == 1:
                one(parts[0])
            else:
                with ThreadPoolExecutor(max_workers=min(16, len(parts))) as ex:
                    list(ex.map(one, parts))
        finally:
            del mv
        return dev

    def advance(self, n: int) -> None:
        if self.mm is not None:
            self.base += n
        else:
            del self._buf[:n]

    def close(self) -> None:
        if self.mm is not None:
            self.mm.close()
            self.mm = None
        self.f.close()


class _Sink:
    """Positioned writes into the output file (or a bytearray).  A pipe, FIFO
    or terminal (/dev/stdout) cannot take pwrite (ESPIPE): there the writes
    go out sequentially, any that arrive ahead of the stream position held
    until the bytes before them have been written."""

    def __init__(self, path: str | None, create: bool):
        import os
        import stat
        self.path, self.mem, self.fd = path, None, None
        self.seq, self.pos, self.held = False, 0, {}
        if path is None:
            self.mem = bytearray()
        else:
            flags = os.O_WRONLY | (os.O_CREAT | os.O_TRUNC if create else 0)
            self.fd = os.open(path, flags, 0o644)
            self.seq = not stat.S_ISREG(os.fstat(self.fd).st_mode)

    def _write_seq(self, off: int, mv) -> None:
        import os
        if off != self.pos:
            if off < self.pos:
                raise ValueError("sequential output: a write before the stream position")
            self.held[off] = bytes(mv)
            return
        while True:
            while len(mv):
                k = os.write(self.fd, mv)
                mv = mv[k:]
                self.pos += k
            nxt = self.held.pop(self.pos, None)
            if nxt is None:
                return
            mv = memoryview(nxt)

    def write_at(self, off: int, data) -> None:
        import os
        mv = memoryview(data).cast("B")
        if self.mem is not None:
            if len(self.mem) < off + len(mv):
                self.mem.extend(b"\0" * (off + len(mv) - len(self.mem)))
            self.mem[off:off + len(mv)] = mv
            return
        if self.seq:
            self._write_seq(off, mv)
            return
        if len(mv) >= (64 << 20):
            # large writes in 32 MB parts on several threads (the page-cache
            # copy runs at ~4 GB/s on one core; pwrite releases the GIL)
            from concurrent.futures import ThreadPoolExecutor
            step = 32 << 20
            parts = [(o, min(o + step, len(mv))) for o in range(0, len(mv), step)]

            def one(p):
                a, b = p
                part, at = mv[a:b], off + a
                while len(part):
                    k = os.pwrite(self.fd, part, at)
                    part, at = part[k:], at + k
            with ThreadPoolExecutor(max_workers=min(16, len(parts))) as ex:
                list(ex.map(one, parts))
            return
        while len(mv):
            k = os.pwrite(self.fd, mv, off)
            mv, off = mv[k:], off + k

    def close(self) -> None:
        import os
        if self.fd is not None:
            held, self.held = self.held, {}
            os.close(self.fd)
            self.fd = None
            if held:
                raise ValueError("sequential output: a gap before the held writes")


def _allgather_obj(x, group):
    return S.xchg(x, group)


def _barrier(group):
    S.barrier(group)


def _complete_records(text_d, n: int, eof: bool):
    """Record ends of text_d[:n] (exclusive offsets, increasing; a list or a
    uint64 array) that are known to be complete, and whether the text is
    FASTA.  FASTQ: after each record (fqz5_fastq_record_ends: 4-line or
    wrapped); FASTA: before every header line after the first; at the end of
    the input, the end of the text closes the last record."""
    import torch
    if n == 0:
        return [], False
    t = text_d[:n]
    fasta = int(t[0].item()) == ord(">")
    if fasta:
        starts = ((t[1:] == ord(">")) & (t[:-1] == 10)).nonzero().flatten() + 1
        ends = starts.cpu().tolist()
    else:
        # 4-line records, or kseq's wrapped ones (fqz5_fastq_record_ends)
        cap = int((t == 10).sum().item()) // 3 + 2
        buf = np.zeros(cap, np.uint64)
        cnt = C.c_uint64(0)
        _lib.after_torch()
        _check(_load().fqz5_fastq_record_ends(text_d.data_ptr(), n, int(bool(eof)), buf.ctypes.data,
                                              cap, C.byref(cnt)), "fqz5_fastq_record_ends")
        # (an array: the window needs the count and one end, not 3M Python ints)
        ends = buf[:int(cnt.value)]
        if eof and (not len(ends) or int(ends[-1]) != n):
            ends = np.append(ends, np.uint64(n))
        return ends, fasta
    if eof and (not ends or ends[-1] != n):
        ends.append(n)
    del torch
    return ends, fasta


def _rec_start(recs, r: int) -> int:
    """Text offset of record r's header line (its name field less one)."""
    import torch
    w = C.sizeof(FastqRec)
    return int(recs[r * w:r * w + 8].view(torch.int64).item()) - 1


class _Window:
    """One window of the input, parsed: record table, block starts (records),
    the blocks to code now, and the text to consume after them."""
    pass


def _next_window(srcs: list, blk: int, wbytes: int, device: str):
    """Parse the next window of whole records from the source(s); returns a
    _Window or None at the end of the input.  Grows the window until it holds
    one complete block (or the rest of the input)."""
    import torch
    so = _load()
    paired = len(srcs) == 2
    want = wbytes
    while True:
        with _stage("read"):                  # (the parts go up as they are read)
            for s in srcs:
                s.fill(want, device)
        devs, ends = [], []
        for s in srcs:
            with _stage("upload"):
                if getattr(s, "dev", None) is not None and int(s.dev.numel()) == len(s.buf):
                    d = s.dev
                    s.dev = None
                    H2D[0] += int(d.numel())
                elif len(s.buf):
                    cpu = torch.frombuffer(s.buf, dtype=torch.uint8)
                    d = cpu.to(device)            # blocking (pageable): done before the parse
                    H2D[0] += int(cpu.numel())
                    del cpu
                else:
                    d = torch.empty(0, dtype=torch.uint8, device=device)
            devs.append(d)
            with _stage("record_ends"):
                ends.append(_complete_records(d, int(d.numel()), s.eof)[0])
        k = min(len(e) for e in ends) if paired else len(ends[0])
        r1_done = srcs[0].eof and k == len(ends[0])      # all of R1 in the window
        if paired and not r1_done and srcs[1].eof and k == len(ends[1]):
            raise _lib.NativeError("unpaired read detected: R2 file ended before R1")
        if k == 0:
            if r1_done:
                return None
            want *= 2
            continue
        cut = [int(e[k - 1]) for e in ends]
        if paired:
            text_d = torch.cat([devs[0][:cut[0]], devs[1][:cut[1]]])
            len1 = cut[0]
        else:
            text_d, len1 = devs[0][:cut[0]], None
        del devs
        if len1 is None:
            with _stage("parse"):
                recs, rsz, nrec, fasta = _index_text(text_d, 0, int(text_d.numel()), wrapped=True)
                first = _blocks(so, rsz, blk)
        else:
            r1, rs1, n1, fa1 = _index_text(text_d, 0, len1, wrapped=True)
            r2, rs2, n2, fa2 = _index_text(text_d, len1, int(text_d.numel()) - len1, wrapped=True)
            if n2 < n1:
                raise _lib.NativeError("unpaired read detected: R2 file ended before R1")
            if n1 and fa1 != fa2:
                raise _lib.NativeError("paired files: one FASTA, one FASTQ")
            w = C.sizeof(FastqRec)
            recs = (torch.stack([r1.view(n1, w), r2[:n1 * w].view(n1, w)], 1).reshape(-1)
                    if n1 else r1)
            del r1, r2
            pair = rs1.astype(np.uint64) + rs2[:n1].astype(np.uint64)
            if n1 and int(pair.max()) >= 2 ** 32:
                raise _lib.NativeError("paired record larger than 4 GB")
            first = _blocks(so, pair.astype(np.uint32), blk) * 2
            fasta = fa1
        nb = len(first) - 1
        keep = nb if r1_done else nb - 1
        if keep <= 0:
            want *= 2
            continue
        W = _Window()
        W.text_d, W.recs, W.first, W.fasta, W.pairs = text_d, recs, first[:keep + 1], fasta, paired
        W.final = bool(r1_done and keep == nb)   # the input ends with this window
        if keep < nb:                          # the next window starts at block `keep`
            r = int(first[keep])
            W.consume = [_rec_start(recs, r)] + \
                ([_rec_start(recs, r + 1) - len1] if paired else [])
        else:
            W.consume = [len(srcs[0].buf)] + ([len(srcs[1].buf)] if paired else [])
        return W


# ---------------------------------------------------------------------------
# Windows read once over the ranks (plain files, several ranks).  The window
# [P, P + Wn) of each input is cut into one byte range per rank; each rank
# reads and uploads only its range (and the byte before it), counts its
# newlines on the GPU, and after one exchange of the counts knows which of
# its line starts are record starts (FASTQ: every 4th line from the window
# start; FASTA: a '>' line).  It parses the records that start in its range
# (fqz5_fastq_index), and a second exchange gives every rank every record's
# start, load_seqs_kseq size, name-section and sequence bytes: the block
# split (fqz5_fastq_blocks) is then computed alike on every rank.  A block
# belongs to the rank holding its first record; a rank then gathers its own
# blocks (and the trial blocks whose work candidates it shares) from the text
# it already holds, reading from the file only the bytes it lacks (the end of
# its last block, other ranks' trial blocks).  Reference: load_seqs_kseq's
# split, fqzcomp5.c:423-623; dispatch :3051-3120.
# ---------------------------------------------------------------------------
H2D = [0]          # input text bytes this process uploaded (tests, bench)


def _upload(buf, device: str):
    import torch
    a = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else buf
    H2D[0] += int(a.size)
    if not a.size:
        return torch.empty(0, dtype=torch.uint8, device=device)
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


class _PosFile:
    """A plain input file read at positions."""

    def __init__(self, path: str):
        import os
        self.fd = os.open(path, os.O_RDONLY)
        self.size = os.fstat(self.fd).st_size

    def read(self, a: int, b: int) -> np.ndarray:
        import os
        out = np.empty(max(b - a, 0), np.uint8)
        got = 0
        while got < out.size:
            c = os.pread(self.fd, out.size - got, a + got)
            if not c:
                raise _lib.NativeError("input file shrank while being read")
            out[got:got + len(c)] = np.frombuffer(c, np.uint8)
            got += len(c)
        return out

    def close(self) -> None:
        import os
        os.close(self.fd)


def _allgather_np(x, group):
    return _allgather_obj(x, group)


def _record_end(f: _PosFile, s: int, fasta: bool) -> int:
    """End (exclusive) of the record starting at file offset s: FASTQ after
    its 4th line, FASTA before the next '>' line; the end of the file closes
    the last record."""
    need, at, piece = 4, s, 1 << 16
    while at < f.size:
        b = f.read(at, min(f.size, at + piece))
        if fasta:
            hit = np.flatnonzero((b[:-1] == 10) & (b[1:] == ord(">")))
            if hit.size:
                return at + int(hit[0]) + 1
            at += max(b.size - 1, 1)
        else:
            nl = np.flatnonzero(b == 10)
            if nl.size >= need:
                return at + int(nl[need - 1]) + 1
            need -= nl.size
            at += b.size
        piece *= 2
    return f.size


class _Scan:
    """One input's window scanned over the ranks (see above)."""
    pass


def _scan(f: _PosFile, P: int, Wn: int, device: str, group, fasta=None) -> _Scan:
    import torch
    ws, rk = S._world(group)
    lo, hi = P + rk * Wn // ws, P + (rk + 1) * Wn // ws
    # bytes [lo - 1, hi): the byte before the range decides whether lo
    # starts a line (a newline stands in before the window start)
    h = f.read(max(lo - 1, P), hi)
    if lo == P:
        h = np.concatenate([np.array([10], np.uint8), h])
    t = _upload(h, device)
    n = hi - lo
    nl = (t[:n] == 10) if n else torch.zeros(0, dtype=torch.bool, device=device)
    head = int(t[1].item()) if rk == 0 and t.numel() > 1 else -1
    cnt = int(nl.sum().item()) if n else 0
    got = _allgather_np((cnt, head), group)
    if fasta is None:
        fasta = got[0][1] == ord(">")
    base = sum(c for c, _ in got[:rk])
    # four: this range reads as 4-line FASTQ (every line 4k a '@' line, every
    # line 4k + 2 a '+' line), where kseq's record is exactly those 4 lines;
    # wrapped FASTQ (or blank lines among the records) fails it and the
    # window is read whole instead (_next_window_ranks)
    four = True
    if n:
        if fasta:
            st = nl & (t[1:n + 1] == ord(">"))
        else:
            # (an '@' line: blank lines after the last record start none)
            line = torch.cumsum(nl.to(torch.int64), 0) + (base - 1)
            st = nl & (line % 4 == 0) & (t[1:n + 1] == ord("@"))
            four = not bool((nl & (line % 4 == 2) & (t[1:n + 1] != ord("+"))).any().item()) \
                and not bool((nl & (line % 4 == 0) & (t[1:n + 1] != ord("@"))).any().item())
        starts = (st.nonzero().flatten() + lo).cpu().numpy().astype(np.int64)
    else:
        starts = np.zeros(0, np.int64)
    firsts = _allgather_np(int(starts[0]) if starts.size else -1, group)
    # the end of this rank's last record: the next rank's first start, or
    # (the window's last record) found by reading on
    nxt = [x for x in firsts[rk + 1:] if x >= 0]
    sc = _Scan()
    sc.fasta = fasta
    sc.lo = int(starts[0]) if starts.size else hi
    nrec = -1
    if starts.size and four:
        end = nxt[0] if nxt else _record_end(f, int(starts[-1]), fasta)
        text = t[int(starts[0]) - (lo - 1):]
        if end > hi:
            text = torch.cat([text, _upload(f.read(hi, end), device)])
        else:
            text = text[:end - int(starts[0])]
        sc.hi = end
        try:
            recs, rsz, nrec, fa = _index_text(text, 0, int(text.numel()))
        except _lib.NativeError:
            four = False              # (every rank still takes the exchanges below)
        four = four and nrec == starts.size
    if starts.size and four:
        w = C.sizeof(FastqRec)
        u = recs.view(nrec, w)[:, 32:44].contiguous().view(torch.int32).view(nrec, 3).cpu().numpy()
        nsz = (u[:, 0] + np.where(u[:, 1] > 0, u[:, 1] + 1, 0) + 1).astype(np.uint64)
        slen = u[:, 2].astype(np.uint64)
    else:
        text, sc.hi = t[:0], hi
        rsz = np.zeros(0, np.uint32)
        nsz = slen = np.zeros(0, np.uint64)
        if not four:
            starts = np.zeros(0, np.int64)
    del t, nl
    sc.text = text                       # this rank's records' text, [lo, hi) of the file
    parts = _allgather_np((starts, rsz.astype(np.uint32), nsz, slen, sc.hi, four), group)
    sc.four = all(p[5] for p in parts)
    if not sc.four:
        return sc
    sc.start = np.concatenate([p[0] for p in parts]).astype(np.int64)
    sc.rsz = np.concatenate([p[1] for p in parts]).astype(np.uint32)
    sc.nsz = np.concatenate([p[2] for p in parts]).astype(np.uint64)
    sc.slen = np.concatenate([p[3] for p in parts]).astype(np.uint64)
    counts = [len(p[0]) for p in parts]
    sc.rank_of = np.repeat(np.arange(ws), counts)
    ends = [p[4] for p in parts if len(p[0])]
    sc.end = np.append(sc.start[1:], ends[-1] if ends else P).astype(np.int64)   # per record
    sc.n = int(sc.start.size)
    return sc


def _need_text(f: _PosFile, sc: _Scan, ranges, device: str):
    """The text of the byte ranges (file order, disjoint) as one device
    buffer: the parts this rank holds from its scan sliced, the rest read."""
    import torch
    pieces = []
    for a, e in ranges:
        x0, x1 = max(a, sc.lo), min(e, sc.hi)
        if x0 < x1:
            if a < x0:
                pieces.append(_upload(f.read(a, x0), device))
            pieces.append(sc.text[x0 - sc.lo:x1 - sc.lo])
            if x1 < e:
                pieces.append(_upload(f.read(x1, e), device))
        else:
            pieces.append(_upload(f.read(a, e), device))
    if not pieces:
        return torch.empty(0, dtype=torch.uint8, device=device)
    return torch.cat(pieces) if len(pieces) > 1 else pieces[0]


def _merge(ranges):
    out = []
    for a, e in ranges:
        if out and out[-1][1] == a:
            out[-1] = (out[-1][0], e)
        else:
            out.append((a, e))
    return out


class _RankWindow:
    """A window read once over the ranks: the per-block fields every rank
    knows, and gather() for the blocks this rank codes or tries."""

    def __init__(self, files, pos, scans, k, first, keep, final, group, device):
        ws, rk = S._world(group)
        self.files, self.pos, self.scans, self.device = files, pos, scans, device
        self.paired = len(files) == 2
        self.first, self.nb, self.final = first, keep, final
        mul = 2 if self.paired else 1
        fa = scans[0].fasta
        self.text_fasta = fa
        self.fasta, self.name_bytes, self.seq_bytes, self.nrec, self.owner = [], [], [], [], []
        for b in range(keep):
            a, e = int(first[b]) // mul, int(first[b + 1]) // mul
            self.fasta.append(fa or int(scans[0].slen[a]) == 0)
            self.name_bytes.append(int(sum(int(s.nsz[a:e].sum()) for s in scans)))
            self.seq_bytes.append(int(sum(int(s.slen[a:e].sum()) for s in scans)))
            self.nrec.append((e - a) * mul)
            self.owner.append(int(scans[0].rank_of[a]))
        self.owner = np.array(self.owner, np.int64)
        # the next window starts at block `keep` (R1 and R2 at the same pair)
        if keep < len(first) - 1:
            r = int(first[keep]) // mul
            self.next_pos = [int(s.start[r]) for s in scans]
        else:
            self.next_pos = [int(s.end[k - 1]) if k else p for s, p in zip(scans, pos)]

    def gather(self, need):
        """A sections.Run of the blocks `need` (in that order)."""
        import torch
        mul = 2 if self.paired else 1
        texts, lens = [], []
        for f, sc in zip(self.files, self.scans):
            rng = []
            for b in need:
                a, e = int(self.first[b]) // mul, int(self.first[b + 1]) // mul
                rng.append((int(sc.start[a]), int(sc.end[e - 1])))
            t = _need_text(f, sc, _merge(rng), self.device)
            texts.append(t)
            lens.append(int(t.numel()))
        nrecs = [self.nrec[b] for b in need]
        loc = np.concatenate([[0], np.cumsum(nrecs)]).astype(np.int64)
        if not self.paired:
            text_d = texts[0]
            recs, _, nrec, _ = _index_text(text_d, 0, lens[0])
        else:
            text_d = torch.cat(texts) if lens[1] else texts[0]
            r1, _, n1, _ = _index_text(text_d, 0, lens[0])
            r2, _, n2, _ = _index_text(text_d, lens[0], lens[1])
            if n1 != n2:
                raise _lib.NativeError("window gather: R1 and R2 record counts differ")
            w = C.sizeof(FastqRec)
            recs = torch.stack([r1.view(n1, w), r2.view(n2, w)], 1).reshape(-1) if n1 else r1
            nrec = 2 * n1
        if nrec != int(loc[-1]):
            raise _lib.NativeError("window gather: record count differs from the scan")
        run = _gather_ranges(text_d, recs, [(int(loc[j]), int(loc[j + 1]))
                                            for j in range(len(need))],
                             self.text_fasta, self.paired)
        for j, b in enumerate(need):          # the scan's sizes are the ones coded
            i = run.blk_sec0[j]
            if (run.spans[i][2] - run.spans[i][1], run.spans[i + 1][2] - run.spans[i + 1][1]) != \
                    (self.name_bytes[b], self.seq_bytes[b]):
                raise _lib.NativeError("window gather: section sizes differ from the scan")
        return run

    def advance(self):
        self.pos[:] = self.next_pos


WRAPPED = object()


def _next_window_ranks(files, pos, blk: int, wbytes: int, device: str, group):
    """The next window of the inputs at file offsets `pos`, read once over
    the ranks; None at the end of the input; WRAPPED when the window is not
    4-line FASTQ (or FASTA), whose record starts the line count cannot give:
    wrapped FASTQ, whose kseq records (kseq.h:194-216) only a walk from a
    known record start finds (the caller then reads the window whole on
    every rank, _LocalWindow)."""
    so = _load()
    paired = len(files) == 2
    want = wbytes
    if pos[0] >= files[0].size:
        return None
    while True:
        wn = [min(want, f.size - p) for f, p in zip(files, pos)]
        eof = [p + w >= f.size for f, p, w in zip(files, pos, wn)]
        scans = [_scan(files[0], pos[0], wn[0], device, group)]
        if paired:
            scans.append(_scan(files[1], pos[1], wn[1], device, group))
        if not all(sc.four for sc in scans):
            return WRAPPED
            if scans[0].n and scans[1].n and scans[0].fasta != scans[1].fasta:
                raise _lib.NativeError("paired files: one FASTA, one FASTQ")
        k = min(s.n for s in scans)
        r1_done = eof[0] and k == scans[0].n
        if paired and not r1_done and eof[1] and k == scans[1].n:
            raise _lib.NativeError("unpaired read detected: R2 file ended before R1")
        if k == 0:
            if r1_done:
                return None
            want *= 2
            continue
        if paired:
            pair = scans[0].rsz[:k].astype(np.uint64) + scans[1].rsz[:k].astype(np.uint64)
            if int(pair.max()) >= 2 ** 32:
                raise _lib.NativeError("paired record larger than 4 GB")
            first = _blocks(so, pair.astype(np.uint32), blk) * 2
        else:
            first = _blocks(so, scans[0].rsz[:k], blk)
        nb = len(first) - 1
        keep = nb if r1_done else nb - 1
        if keep <= 0:
            want *= 2
            continue
        return _RankWindow(files, pos, scans, k, first, keep, bool(r1_done and keep == nb),
                           group, device)


class _LocalWindow:
    """A window every rank reads whole (one rank, or gzip / in-memory
    input): the same per-block fields as _RankWindow."""

    def __init__(self, W, srcs, ws):
        so = _load()
        self.W, self.srcs = W, srcs
        nb = len(W.first) - 1
        self.nb, self.final = nb, W.final
        self.fasta = _fasta_blocks(W.recs, [int(W.first[b]) for b in range(nb)], W.fasta)
        self.name_bytes, self.seq_bytes, self.nrec = [], [], []
        for b in range(nb):
            a, e = int(W.first[b]), int(W.first[b + 1])
            sz = (C.c_uint64 * 3)()
            _lib.after_torch()
            _check(so.fqz5_fastq_gather(W.text_d.data_ptr(), W.recs.data_ptr(), a, e, None,
                                        None, None, None, None, sz), "fqz5_fastq_gather")
            self.name_bytes.append(int(sz[0]))
            self.seq_bytes.append(int(sz[1]))
            self.nrec.append(e - a)
        self.owner = (np.arange(nb) * ws) // nb

    def gather(self, need):
        W = self.W
        return _gather_ranges(W.text_d, W.recs, [(int(W.first[b]), int(W.first[b + 1]))
                                                 for b in need], W.fasta, W.pairs)

    def advance(self):
        for s, c in zip(self.srcs, self.W.consume):
            s.advance(c)


def _code_window(W, sink: _Sink, level: int, pos: int, index: list, av, state, group) -> int:
    """Code the window's blocks over the ranks and write them at file
    offset `pos` on (see above); appends their index entries and returns
    the offset after them."""
    ws, rk = S._world(group)
    nb = W.nb
    # per block the sections in encode_block order (no quality section in a
    # FASTA block)
    per = [2 if f else 3 for f in W.fasta]
    sec0 = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    ids, ins = [], []
    for b in range(nb):
        ids += [S.SEC_NAME, S.SEC_SEQ] + ([] if W.fasta[b] else [S.SEC_QUAL])
        ins += [W.name_bytes[b], W.seq_bytes[b]] + ([] if W.fasta[b] else [W.seq_bytes[b]])
    ids = np.array(ids, np.int32)
    ins = np.array(ins, np.uint32)
    blk_owner = np.asarray(W.owner, np.int64)
    owner = np.repeat(blk_owner, per)
    sched = S.trial_schedule(ids, av, state)
    need = sorted({b for b in range(nb)
                   if blk_owner[b] == rk or sched[sec0[b]:sec0[b + 1]].any()})
    # the needed blocks' section inputs, gathered in HBM
    with _stage("gather"):
        run = W.gather(need)
    secs = [None] * int(sec0[-1])
    local = run.enc_secs()
    for j, b in enumerate(need):
        for q in range(per[b]):
            secs[sec0[b] + q] = local[run.blk_sec0[j] + q]
    with _stage("codec"):
        res, meth, _ = S.encode_window(secs, ids, ins, owner, av, state, group,
                                       bounded=level >= 7, final=W.final,
                                       bounds_first=5 <= level < 7)
    mine = [j for j, b in enumerate(need) if blk_owner[b] == rk]
    full_res = [None] * len(local)
    for j, b in enumerate(need):
        for q in range(per[b]):
            full_res[run.blk_sec0[j] + q] = res[sec0[b] + q]
    for j in mine:
        for q in range(per[need[j]]):
            r = full_res[run.blk_sec0[j] + q]
            if r is None or r.status != 0:
                raise _lib.NativeError("section coding failed: " + _lib.last_error())
    sizes = []
    if mine:
        with _stage("assemble"):
            run.assemble(full_res, mine)
        sizes = [int(run.blk_off[i + 1] - run.blk_off[i]) for i in range(len(mine))]
    all_sizes = _allgather_obj(sizes, group)
    # blocks in file order: rank-contiguous, so rank-major order
    flat = [z for zs in all_sizes for z in zs]
    assert len(flat) == nb
    starts = np.concatenate([[0], np.cumsum(flat)]).astype(np.int64) + pos
    if mine:
        end = int(run.blk_off[len(mine)])
        with _stage("download"):
            host = _pinned(end)
            host.copy_(run.blk_buf[:end])
        b0 = need[mine[0]]
        with _stage("write"):
            sink.write_at(int(starts[b0]), host.numpy())
        del host
    for b in range(nb):
        index.append((int(starts[b]), W.seq_bytes[b], W.nrec[b]))
    return int(starts[-1])


def _encode_stream(srcs: list, sink: _Sink, level: int, blk_size: int | None, device: str,
                   group=None, window_bytes: int | None = None) -> int:
    """The sources' FASTQ -> .fqz5 written through `sink` (see above);
    returns the file size."""
    ws, rk = S._world(group)
    blk = blk_size or S.BLOCK_SIZE[level]
    # a window holds several blocks per rank, so that every GPU has blocks
    # whose serial chains run side by side
    wbytes = window_bytes or window_bytes_for(level, blk, ws)
    av = S.masks(level, full=True)
    state = S.new_state()
    pos = 16                                  # file offset of the next block
    index = []
    # several ranks on plain files: each reads its share of every window once
    files = [_PosFile(s.path) for s in srcs] \
        if ws > 1 and all(s.path and not s.gz for s in srcs) else None
    opened = list(files or [])
    at = [0] * len(srcs)
    try:
        while True:
            with _stage("window"):
                W = _next_window_ranks(files, at, blk, wbytes, device, group) if files else None
                if W is WRAPPED:
                    # wrapped FASTQ: from here on every rank reads each window
                    # whole and walks its records (fqz5_fastq_record_ends); the
                    # mapped sources start at the window's offsets
                    for s_, a in zip(srcs, at):
                        s_.base = s_.pos = a
                        s_.eof = False
                    files = None
                if not files:
                    w0 = _next_window(srcs, blk, wbytes, device)
                    W = _LocalWindow(w0, srcs, ws) if w0 is not None else None
            if W is None:
                break
            with _stage("code_window"):
                pos = _code_window(W, sink, level, pos, index, av, state, group)
            with _stage("advance"):
                W.advance()
                del W
    finally:
        for f in opened:
            f.close()
    if rk == 0:
        if index:
            idx = _index([o for o, _, _ in index], [b for _, b, _ in index],
                         [n for _, _, n in index])
            sink.write_at(pos, idx)
        else:
            idx = b""
        sink.write_at(0, MAGIC + struct.pack("<Q", pos))
        total = pos + len(idx)
    else:
        total = 0
    _trace_dump(f"encode -{level}")
    return int(_allgather_obj(total, group)[0])


def _gather_ranges(text_d, recs, ranges, fasta: bool, pair_flags: bool):
    """Blocks given as record ranges [a, b) (not necessarily adjacent) as a
    sections.Run, every section input gathered in HBM."""
    import torch
    so = _load()
    sizes = []
    for a, b in ranges:
        sz = (C.c_uint64 * 3)()
        _lib.after_torch()
        _check(so.fqz5_fastq_gather(text_d.data_ptr(), recs.data_ptr(), a, b, None, None, None,
                                    None, None, sz), "fqz5_fastq_gather")
        sizes.append((int(sz[0]), int(sz[1])))
    tot_n = sum(a for a, _ in sizes)
    tot_s = sum(b for _, b in sizes)
    name_d = torch.empty(max(tot_n, 1), dtype=torch.uint8, device=text_d.device)
    seq_d = torch.empty(max(tot_s, 1), dtype=torch.uint8, device=text_d.device)
    qual_d = None if fasta else torch.empty(max(tot_s, 1), dtype=torch.uint8, device=text_d.device)
    bfa = _fasta_blocks(recs, [a for a, _ in ranges], fasta)
    lens, flags, nr, sr = [], [], [], []
    no = so_ = 0
    for (a, b), (zn, zs) in zip(ranges, sizes):
        ln = np.zeros(max(b - a, 1), np.uint32)
        fl = np.zeros(max(b - a, 1), np.uint32)
        sz = (C.c_uint64 * 3)()
        _lib.after_torch()
        _check(so.fqz5_fastq_gather(text_d.data_ptr(), recs.data_ptr(), a, b,
                                    name_d.data_ptr() + no, seq_d.data_ptr() + so_,
                                    None if fasta else qual_d.data_ptr() + so_, ln.ctypes.data,
                                    fl.ctypes.data, sz),
               "fqz5_fastq_gather")
        if pair_flags:
            fl[:] = 0
            fl[1::2] = 128                  # FQZ_FREAD2 (a range starts at an R1 record)
        lens.append(ln[:b - a])
        flags.append(fl[:b - a])
        nr.append((no, no + zn))
        sr.append((so_, so_ + zs))
        no += zn
        so_ += zs
    return S.Run.from_device(name_d, seq_d, qual_d, nr, sr, lens, flags, bfa)


def compress_bytes(text: bytes, level: int = 3, blk_size: int | None = None,
                   device: str = "cuda", window_bytes: int | None = None) -> bytes:
    """fqzcomp5 -<level> (-t1 semantics) of FASTQ text, on the GPU."""
    sink = _Sink(None, True)
    _encode_stream([_Src(data=text)], sink, level, blk_size, device, None, window_bytes)
    return bytes(sink.mem)


def compress_paired_bytes(text1: bytes, text2: bytes, level: int = 3,
                          blk_size: int | None = None, device: str = "cuda",
                          window_bytes: int | None = None) -> bytes:
    """fqzcomp5 -<level> in1 in2 out (-t1 semantics): the two files'
    records interleaved (encode_interleaved, fqzcomp5.c:3211-3440)."""
    sink = _Sink(None, True)
    _encode_stream([_Src(data=text1), _Src(data=text2)], sink, level, blk_size, device, None,
                   window_bytes)
    return bytes(sink.mem)


def compress_file(src: str, dst: str, level: int = 3, blk_size: int | None = None,
                  device: str = "cuda", src2: str | None = None, group=None,
                  window_bytes: int | None = None) -> int:
    """fqzcomp5 -<level> src [src2] dst on the GPU(s): the input streamed in
    windows of whole records, each window's complete blocks coded and written
    behind the last (see above); src2: the R2 file of a pair, interleaved
    with src (fqzcomp5 in1 in2 out).  group: a torch.distributed group, one
    process per GPU, every rank calling with the same arguments; the file
    equals the single-process one byte for byte.  Returns the file size."""
    ws, rk = S._world(group)
    # every rank fails together (S.ranks_fail_together): the body's last
    # exchange is the final barrier, taken on every path
    with S.ranks_fail_together(group):
        if rk == 0:
            _Sink(dst, True).close()              # create / truncate before anyone writes
        _barrier(group)
        sink = _Sink(dst, False)
        srcs = [_Src(src)] + ([_Src(src2)] if src2 else [])
        try:
            n = _encode_stream(srcs, sink, level, blk_size, device, group, window_bytes)
        finally:
            sink.close()
            for s in srcs:
                s.close()
        _barrier(group)
        return n


V11, V10, VOLD = 0, 1, 2                        # read_header's results (fqzcomp5.c:2577)
MAGIC_V10 = b"FQZ5\x01\x00\x00\x00"             # :155


class Blocks(list):
    """Block byte ranges of a container, with its version: V11 (CRC field in
    every block), V10 or VOLD (none; VOLD files have no file header either)."""
    version = V11

    def __init__(self, ranges=(), version: int = V11):
        super().__init__(ranges)
        self.version = version


def _version_of(head: bytes, size: int):
    """read_header (fqzcomp5.c:2578-2603): (version, first block offset,
    index offset or 0).  A file with neither magic is the old headerless
    format: blocks from offset 0 to the end, no index.  Fewer than 8 bytes
    (an empty file included) is an error, as read_header's short fread of
    the magic is (:2581-2582)."""
    if len(head) < 8 or size < 8:
        raise ValueError("not an .fqz5 file: shorter than the 8-byte magic")
    if head[:8] in (MAGIC, MAGIC_V10):
        if len(head) < 16:
            raise ValueError("truncated .fqz5: no index offset after the magic")
        (idx,) = struct.unpack_from("<Q", head, 8)
        if idx > size or (idx and idx < 16):
            raise ValueError("truncated .fqz5: index offset past the end of the file")
        return (V11 if head[:8] == MAGIC else V10), 16, idx
    return VOLD, 0, 0


def _walk(read4, start: int, end: int, version: int) -> Blocks:
    """The block_size walk of decode (fqzcomp5.c:3769-3797) from `start` up
    to `end` (the index or the end of the file); a block that runs past it is
    an error (the reference's read fails there)."""
    hd = 12 if version == V11 else 8
    p, out = start, Blocks(version=version)
    while p < end:
        h = read4(p) if p + 4 <= end else b""
        if len(h) < 4:
            raise ValueError("truncated .fqz5: a block header runs past the end")
        (bsz,) = struct.unpack("<I", h)
        if p + 4 + bsz > end or bsz + 4 < hd:
            raise ValueError("truncated .fqz5: a block runs past the end of the file")
        out.append((p, p + 4 + bsz))
        p += 4 + bsz
    return out


def _blocks_of(data) -> Blocks:
    """Block byte ranges of a .fqz5 held in memory (any version the
    reference reads)."""
    data = memoryview(data).cast("B")
    version, start, idx = _version_of(bytes(data[:16]), len(data))
    return _walk(lambda p: bytes(data[p:p + 4]), start, idx if idx else len(data), version)


def block_fields(data, s: int, e: int, version: int = V11) -> dict:
    """The header fields of the block data[s:e] read on the host, as
    decode_block reads them (fqzcomp5.c:2290-2420): record count, the name,
    sequence and quality sections' sizes, the lengths section.  Raises
    ValueError when a field points past the block or the sizes disagree
    (the decoders write u_len bytes into outputs sized by these fields)."""
    d = memoryview(data).cast("B")

    def get(fmt, at):
        z = struct.calcsize(fmt)
        if at + z > e:
            raise ValueError("corrupt block: header runs past the block")
        return struct.unpack_from(fmt, d, at), at + z

    (bsz, nrec), p = get("<II", s)
    if version == V11:
        _crc, p = get("<I", p)
    if s + 4 + bsz != e:
        raise ValueError("corrupt block: block size field")
    (nu, _st, nc), p = get("<IBI", p)
    p += nc

    def varint(at, end):
        # var_get_u32 as the reference's lengths walk reads it
        # (fqzcomp5.c:2384-2404; csrc/rans_format.hpp varint_get): the bytes
        # it reads, not the header's own count, set the offsets
        if at >= end:
            raise ValueError("corrupt block: bad length varint")
        v = n = 0
        while True:
            c = d[at + n]
            n += 1
            v = ((v << 7) | (c & 0x7f)) & 0xffffffff
            if not (c & 0x80 and n < 6 and at + n < end):
                return v, at + n

    (nb,), p = get("<B", p)
    lens_sum = None
    if nb:
        fixed, p = varint(p, min(e, p + 5))
        lens_sum = fixed * nrec
    else:
        (_lz,), p = get("<I", p)
        lens_sum = 0
        end = min(e, p + 5 * nrec)
        for _ in range(nrec):
            x, p = varint(p, end)
            lens_sum += x
    (_s1, su, sc), p = get("<BII", p)
    p += sc
    (_s2, qu, qc), p = get("<BII", p)
    p += qc
    if p > e:
        raise ValueError("corrupt block: a section runs past the block")
    fasta = qu == 0 and qc == 0
    if not fasta and qu != su:
        raise ValueError("corrupt block: quality and sequence sizes differ")
    if lens_sum != su:
        raise ValueError("corrupt block: record lengths do not sum to the bases")
    return dict(nrec=nrec, name_ulen=nu, seq_ulen=su, qual_ulen=qu, fasta=fasta)


def check_blocks(data, ranges=None) -> list[dict]:
    """block_fields of every block (host only)."""
    if ranges is None:
        ranges = _blocks_of(data)
    v = getattr(ranges, "version", V11)
    return [block_fields(data, s, e, v) for s, e in ranges]


def _parse_checked(data, buf, ranges):
    """The blocks `ranges` of a container (host view `data`, device copy
    `buf`) checked and parsed: their header fields on the host
    (check_blocks), then fqz5_blocks_parse_v on the device with the CRC of
    every block.  Returns the BlockViews, the record lengths and whether each
    block is FASTA."""
    version = getattr(ranges, "version", V11)
    try:
        check_blocks(data, ranges)
    except ValueError as err:
        raise _lib.NativeError(str(err)) from None
    views, lens = [], []
    nrecs = [struct.unpack_from("<I", data, s + 4)[0] for s, _ in ranges]
    parsed = S.parse_blocks([buf.data_ptr() + s for s, _ in ranges], [e - s for s, e in ranges],
                            nrecs, version)
    for v, ln in parsed:
        if not v.crc_ok:
            raise _lib.NativeError("block CRC mismatch")
        # the decoders write u_len bytes into outputs sized by the block's
        # own fields: refuse fields that disagree (decode_block allocates
        # from them, fqzcomp5.c:2433-2519)
        if int(ln.astype(np.uint64).sum()) != v.seq_ulen:
            raise _lib.NativeError("corrupt block: record lengths do not sum to the bases")
        if not (v.qual_ulen == 0 and v.qual_size == 9) and v.qual_ulen != v.seq_ulen:
            raise _lib.NativeError("corrupt block: quality and sequence sizes differ")
        views.append(v)
        lens.append(ln)
    # FASTA: a quality section of u_len 0 and c_len 0 (decode_block,
    # fqzcomp5.c:2477-2483); the text is then output_fasta's (:3503-3517)
    fasta = [v.qual_ulen == 0 and v.qual_size == 9 for v in views]
    return views, lens, fasta


def _group(items, size_of, wb: int) -> list[list]:
    """`items` in order, in groups of at most `wb` bytes by size_of(item): an
    item joins the current group unless that group has items and would pass
    `wb` with it, so an item larger than `wb` stands alone."""
    groups, cur, tot = [], [], 0
    for it in items:
        z = size_of(it)
        if cur and tot + z > wb:
            groups.append(cur)
            cur, tot = [], 0
        cur.append(it)
        tot += z
    if cur:
        groups.append(cur)
    return groups


class _ReadWindow:
    """Adjacent blocks of a container as read and uploaded together: the host
    view `data`, its device copy `buf`, the blocks' byte ranges within them
    (`ranges`, a Blocks) and their numbers in the file (`blocks`, windows of
    the index).  parse() adds what _parse_checked gives: `views`, `lens`,
    `fasta`."""

    def __init__(self, data, buf, ranges, blocks=None):
        self.data, self.buf, self.ranges, self.blocks = data, buf, ranges, blocks
        self.base = buf.data_ptr()

    def parse(self) -> None:
        """_parse_checked of the window.  A call of its own, so that its time
        (the block parse, the CRCs) falls into the stage the caller is in."""
        self.views, self.lens, self.fasta = _parse_checked(self.data, self.buf, self.ranges)
        self.rls = [ln.ctypes.data_as(C.POINTER(C.c_uint32)) for ln in self.lens]

    def field(self, j: int, sec: int):
        """(offset in block j, compressed size, decoded size) of its section `sec`."""
        v = self.views[j]
        return {S.SEC_NAME: (v.name_off, v.name_size, v.name_ulen),
                S.SEC_SEQ: (v.seq_off, v.seq_size, v.seq_ulen),
                S.SEC_QUAL: (v.qual_off, v.qual_size, v.qual_ulen)}[sec]

    def section(self, j: int, sec: int, dst: int, bases=None):
        """The section `sec` of block j to decode to the device address `dst`;
        bases: for SEC_QUAL the block's decoded bases, which the quality
        decoder reads."""
        off, size, ulen = self.field(j, sec)
        return S.Section(self.base + self.ranges[j][0] + off, dst, size, ulen, 0, sec, self.rls[j],
                         None, len(self.lens[j]), bases)

    def decode(self, secs) -> None:
        if any(r.status != 0 for r in S.decode(secs)):
            raise _lib.NativeError("section decoding failed: " + _lib.last_error())

    def release(self) -> None:
        self.data = self.buf = None


def _layout(fmts, pairs: bool, device: str):
    """The text of blocks laid out one after the other in one device buffer,
    in two passes over fmts, per block a callable fmt(out, cap) -> (the text's
    size, the size of its R1 part): the sizes (out None), then the text into
    the one buffer.  Returns (the text,), with pairs (the R1 text, the R2
    text) of output_fastq_deinterleaved (fqzcomp5.c:3612-3676)."""
    import torch
    sizes = [fmt(None, 0) for fmt in fmts]
    text = torch.empty(max(sum(z for z, _ in sizes), 1), dtype=torch.uint8, device=device)
    _lib.after_torch(device)
    at, r1, r2 = 0, [], []
    for fmt, (z, k) in zip(fmts, sizes):
        fmt(text.data_ptr() + at, z)
        r1.append((at, at + k))
        r2.append((at + k, at + z))
        at += z
    if not pairs:
        return (text[:at],)
    cat = lambda rs: torch.cat([text[x:y] for x, y in rs]) if rs else text[:0]
    return cat(r1), cat(r2)


def _decode_blocks(win, with_qual: bool, device: str):
    """Every block of the parsed window decoded into one device buffer, per
    block its names, bases and (unless FASTA or with_qual False) qualities:
    (the buffer, per block the three offsets in it)."""
    import torch
    nsz = [v.name_ulen for v in win.views]
    ssz = [v.seq_ulen for v in win.views]
    out_d = torch.empty(sum(nsz) + 2 * sum(ssz) + 1, dtype=torch.uint8, device=device)
    secs, places = [], []
    o = out_d.data_ptr()
    for j, (v, fa) in enumerate(zip(win.views, win.fasta)):
        po = (o, o + v.name_ulen, o + v.name_ulen + v.seq_ulen)
        secs.append(win.section(j, S.SEC_NAME, po[0]))
        secs.append(win.section(j, S.SEC_SEQ, po[1]))
        if not fa and with_qual:
            secs.append(win.section(j, S.SEC_QUAL, po[2], po[1]))
        else:
            po = (po[0], po[1], None)
        places.append(po)
        o += v.name_ulen + 2 * v.seq_ulen
    win.decode(secs)
    return out_d, places


def _format_blocks(win, places, plus_name: bool, device: str, pairs: bool, slices):
    """The text of the window's decoded blocks (`places`: _decode_blocks'),
    see _decode."""
    so = _load()

    def fmt_of(j):
        head = (places[j][0], win.views[j].name_ulen, places[j][1], places[j][2],
                win.lens[j].ctypes.data, len(win.lens[j]))

        def fmt(out, cap):
            size, s1 = C.c_uint64(0), C.c_uint64(0)
            if slices is not None:
                rc = so.fqz5_fastq_format_range(*head, *slices[j], int(plus_name), int(pairs), out,
                                                cap, C.byref(size), C.byref(s1) if pairs else None)
            elif pairs:
                rc = so.fqz5_fastq_format_pairs(*head, int(plus_name), out, cap, C.byref(size),
                                                C.byref(s1))
            else:
                rc = so.fqz5_fastq_format(*head, int(plus_name), out, cap, C.byref(size))
            _check(rc, "fqz5_fastq_format")
            return int(size.value), int(s1.value)
        return fmt
    return _layout([fmt_of(j) for j in range(len(win.views))], pairs, device)


def _decode(win, plus_name: bool, device: str, pairs: bool = False):
    """The blocks of a parsed window -> (the FASTQ text of every block in one
    device buffer,); pairs: (the R1 text, the R2 text), even records of every
    block to R1 and odd ones to R2.  (The whole-file callers, which time the
    call; the range path records its stages around the two steps.)"""
    out_d, places = _decode_blocks(win, True, device)
    return _format_blocks(win, places, plus_name, device, pairs, None)


def _whole(data, device: str):
    """A container held in memory as one parsed window, None without blocks."""
    import torch
    ranges = _blocks_of(data)
    if not ranges:
        return None
    win = _ReadWindow(data, torch.frombuffer(bytearray(data), dtype=torch.uint8).to(device), ranges)
    win.parse()
    return win


def decompress_bytes(data: bytes, plus_name: bool = False, device: str = "cuda") -> bytes:
    """fqzcomp5 -d of a .fqz5 (its blocks parsed, CRC-checked and decoded on
    the GPU, the FASTQ text formatted there)."""
    win = _whole(data, device)
    return _decode(win, plus_name, device)[0].cpu().numpy().tobytes() if win else b""


def decompress_paired_bytes(data: bytes, plus_name: bool = False,
                            device: str = "cuda") -> tuple[bytes, bytes]:
    """fqzcomp5 -d in out1 out2: the records deinterleaved into R1 / R2."""
    win = _whole(data, device)
    if not win:
        return b"", b""
    t1, t2 = _decode(win, plus_name, device, pairs=True)
    return t1.cpu().numpy().tobytes(), t2.cpu().numpy().tobytes()


def _file_blocks(f, size: int) -> Blocks:
    """Block byte ranges of a .fqz5 file (any version the reference reads),
    walking the block size fields up to the index; checked against the file
    size."""
    f.seek(0)
    version, start, idx = _version_of(f.read(16), size)

    def read4(p):
        f.seek(p)
        return f.read(4)
    return _walk(read4, start, idx if idx else size, version)


def _block_text_size(f, s: int, e: int, plus_name: bool, version: int = V11) -> int:
    """The FASTQ (or FASTA) text size of block [s, e) of an open .fqz5, from
    its headers alone (a few small reads): output_fastq writes '@' name '\n'
    seq '\n' '+' [name] '\n' qual '\n' per record (fqzcomp5.c:3441-3480),
    output_fasta '>' name '\n' seq '\n' (:3503-3517); the name section
    decodes to each name and a '\0'."""
    hd = 12 if version == V11 else 8
    f.seek(s)
    h = f.read(hd + 9)
    if len(h) < hd + 9:
        raise ValueError("truncated .fqz5: a block header runs past the end")
    nrec, = struct.unpack_from("<I", h, 4)
    name_ulen, = struct.unpack_from("<I", h, hd)
    c_len, = struct.unpack_from("<I", h, hd + 5)
    p = s + hd + 9 + c_len
    f.seek(p)
    nb = f.read(1)
    if not nb:
        raise ValueError("truncated .fqz5: lengths past the block")
    if nb[0]:
        vl = f.read(5)
        n = 1
        while n < len(vl) and vl[n - 1] & 0x80:
            n += 1
        p += 1 + n
    else:
        # [0][u32][a varint per record]: walk them (read in one go)
        f.seek(p + 5)
        v = f.read(min(5 * nrec, max(e - p - 5, 0)))
        k = 0
        for _ in range(nrec):
            while k < len(v) and v[k] & 0x80:
                k += 1
            k += 1
        p += 5 + k
    f.seek(p)
    sh = f.read(9)
    if len(sh) < 9:
        raise ValueError("truncated .fqz5: sequence header past the block")
    seq_ulen, seq_clen = struct.unpack_from("<II", sh, 1)
    f.seek(p + 9 + seq_clen)
    qh = f.read(9)
    if len(qh) < 9:
        raise ValueError("truncated .fqz5: quality header past the block")
    qual_ulen, qual_clen = struct.unpack_from("<II", qh, 1)
    names = name_ulen - nrec
    if qual_ulen == 0 and qual_clen == 0:                    # FASTA
        return names + seq_ulen + 2 * nrec
    return names * (2 if plus_name else 1) + 2 * seq_ulen + 6 * nrec


def decompress_file(src: str, dst: str, plus_name: bool = False, device: str = "cuda",
                    dst2: str | None = None, group=None, window_bytes: int | None = None) -> int:
    """fqzcomp5 -d src dst [dst2] on the GPU(s): blocks read and decoded in
    windows of at most `window_bytes` of compressed data (the reference
    decodes block by block, fqzcomp5.c:3754-3800), the text written behind
    the last.  dst2: deinterleave, R1 records to dst and R2 records to dst2
    (fqzcomp5 -d in out1 out2).  group: one process per GPU, the blocks split
    contiguously over the ranks; every window's text goes out as soon as it
    is decoded (host memory stays one window): at its offset from the block
    headers' text sizes (one output), or into a per-rank spill file copied
    into place at the end (R1/R2: the split of a block's text between the two
    files needs its decoded names).  Returns the text bytes written."""
    import os
    ws, rk = S._world(group)
    with S.ranks_fail_together(group):
        outs = [dst] + ([dst2] if dst2 is not None else [])
        if ws > 1 and any(d.endswith(".gz") for d in outs):
            raise ValueError("gzip output needs a single process")
        size = os.path.getsize(src)
        single = ws == 1
        spill = not single and dst2 is not None
        with open(src, "rb") as f:
            with _stage("index"):
                ranges = _file_blocks(f, size)
            nb = len(ranges)
            mine = [b for b in range(nb) if (b * ws) // max(nb, 1) == rk] if nb else []
            groups = _group(mine, lambda b: ranges[b][1] - ranges[b][0],
                            window_bytes or DEFAULT_WINDOW)
            gz = [d.endswith(".gz") for d in outs]
            streams, sinks, at = [], [], 0
            plain = []                        # single process: plain outputs by positioned writes
            with _stage("open"):
                if single:
                    import gzip
                    streams = [gzip.GzipFile(filename="", mode="wb", compresslevel=6, mtime=0,
                                             fileobj=open(d, "wb")) if z else None
                               for d, z in zip(outs, gz)]
                    plain = [None if z else _Sink(d, True) for d, z in zip(outs, gz)]
                elif spill:
                    streams = [open(f"{d}.part{rk}", "wb") for d in outs]
                else:
                    # one output: every block's text size from its headers, so this
                    # rank's text starts at the sum over the blocks before its first
                    sizes = [_block_text_size(f, s, e, plus_name, ranges.version)
                             for s, e in ranges]
                    at = sum(sizes[:mine[0]]) if mine else 0
                    if rk == 0:
                        _Sink(dst, True).close()
                    _barrier(group)
                    sinks = [_Sink(dst, False)]
            written = [0 for _ in outs]
            try:
                for gb in groups:
                    a, e = ranges[gb[0]][0], ranges[gb[-1]][1]
                    with _stage("read"):
                        host = _pinned(e - a)
                        f.seek(a)
                        mv = memoryview(host.numpy())
                        got = 0
                        while got < e - a:
                            k = f.readinto(mv[got:])
                            if not k:
                                raise OSError(f"{src}: short read")
                            got += k
                        hv = host.numpy()
                    with _stage("upload"):
                        buf = host.to(device)      # blocking: block parsing runs on the library's streams
                    with _stage("decode"):
                        win = _ReadWindow(hv, buf, Blocks([(ranges[b][0] - a, ranges[b][1] - a)
                                                       for b in gb], ranges.version))
                        win.parse()
                        texts = _decode(win, plus_name, device, pairs=dst2 is not None)
                    for j, t in enumerate(texts):
                        with _stage("download"):
                            out = _pinned(int(t.numel()))
                            out.copy_(t)
                        with _stage("write"):
                            if sinks:
                                want = sum(sizes[b] for b in gb)
                                if int(t.numel()) != want:
                                    raise _lib.NativeError(
                                        "decoded text size differs from the block headers'")
                                sinks[j].write_at(at + written[j], out.numpy())
                            elif plain and plain[j] is not None:
                                plain[j].write_at(written[j], out.numpy())
                            else:
                                streams[j].write(memoryview(out.numpy()))
                            written[j] += int(t.numel())
                        del out
                    with _stage("free"):
                        del buf, host, texts, win
            finally:
                with _stage("close"):
                    for sk in plain:
                        if sk is not None:
                            sk.close()
                    for st in streams:
                        if st is None:
                            continue
                        if isinstance(st, __import__("gzip").GzipFile):
                            raw = st.fileobj          # (close() drops the reference)
                            st.close()
                            raw.close()
                        else:
                            st.close()
                    for sk in sinks:
                        sk.close()
        _trace_dump("decode")
        if single:
            return sum(written)
        all_w = _allgather_obj(written, group)
        if spill:
            # the spill files into place at their offsets from the ranks' sizes
            for j, d in enumerate(outs):
                if rk == 0:
                    _Sink(d, True).close()
            _barrier(group)
            for j, d in enumerate(outs):
                off = sum(w[j] for w in all_w[:rk])
                sink = _Sink(d, False)
                part = f"{d}.part{rk}"
                try:
                    with open(part, "rb") as pf:
                        for c in iter(lambda: pf.read(1 << 26), b""):
                            sink.write_at(off, c)
                            off += len(c)
                finally:
                    sink.close()
                    os.unlink(part)
        _barrier(group)
        return sum(sum(w) for w in all_w)


def _write_out(path: str, data) -> None:
    """Decoded text to `path`; gzip-compressed when the name ends in ".gz"
    (gzopen(name, "wb"), zlib's default level, fqzcomp5.c:5113-5160)."""
    if path.endswith(".gz"):
        import gzip
        # no file name and mtime 0 in the header, as zlib's gzopen writes it
        with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", compresslevel=6,
                                                    mtime=0, fileobj=raw) as f:
            f.write(data)
    else:
        with open(path, "wb") as f:
            f.write(data)


# ---------------------------------------------------------------------------
# Record ranges through the block index
#
# The index at the end of the file (write_index, fqzcomp5.c:2606-2630) gives
# every block's file offset and record count, so the blocks that hold records
# [first, first + count) follow from prefix sums of the counts, and only those
# blocks are read, checked and decoded (whole: a block's rANS streams, its
# adaptive models and its tok3 names have no prefix decode).  Their text is
# laid out on the device for the wanted records only
# (fqz5_fastq_format_range).  The reference writes the index and reads it
# only for --inspect; a file without one (v1.0 files written without, the
# old headerless format) is walked block header by block header instead.
# ---------------------------------------------------------------------------
class Index(list):
    """Blocks of a container as (start, end, nrec): the block's byte range
    in the file and its record count; `version` as for Blocks, `indexed`
    whether the file's own index gave them (else the block headers did)."""

    def __init__(self, blocks=(), version: int = V11, indexed: bool = True):
        super().__init__(blocks)
        self.version, self.indexed = version, indexed


class _PosBytes:
    """A container held in memory, read at positions (as _PosFile)."""

    def __init__(self, data):
        self.mv = memoryview(data).cast("B")
        self.size = len(self.mv)

    def read(self, a: int, b: int) -> np.ndarray:
        return np.frombuffer(self.mv[a:max(a, b)], np.uint8).copy()

    def close(self) -> None:
        pass


def _reader(src):
    """(reader, whether to close it): src a path, bytes, or a reader."""
    import os
    if isinstance(src, (str, os.PathLike)):
        return _PosFile(os.fspath(src)), True
    if hasattr(src, "read") and hasattr(src, "size"):
        return src, False
    return _PosBytes(src), False


def _run(opened, what: str, fn):
    """fn(reader) for `opened`, a (reader, whether to close it) as _reader
    gives: the reader closed behind it, then the $FQZ5_FILE_TRACE line of the
    entry point `what`."""
    rd, close = opened
    try:
        res = fn(rd)
    finally:
        if close:
            rd.close()
    _trace_dump(what)
    return res


def read_index(src) -> Index:
    """The blocks of a .fqz5 (a path, the file's bytes, or a positioned
    reader) as an Index.  With an index offset in the header this is one
    positioned read of the index and touches no block; the index is checked
    structurally (magic, size, offsets from 16 strictly increasing up to the
    index) and a failure raises ValueError("corrupt index: ...").  Without
    one the block size fields are walked (_walk) and each block's record
    count comes from its header."""
    rd, close = _reader(src)
    try:
        size = rd.size
        version, start, idx = _version_of(bytes(rd.read(0, min(16, size))), size)
        if idx:
            if idx == size == 16:
                return Index(version=version)              # an empty body: no index is written
            raw = bytes(rd.read(idx, size))                # the one read
            if len(raw) < 12 or raw[:8] != INDEX_MAGIC:
                raise ValueError("corrupt index: bad magic")
            (n,) = struct.unpack_from("<I", raw, 8)
            if 12 + 16 * n > len(raw):
                raise ValueError("corrupt index: more entries than the file holds")
            ent = [struct.unpack_from("<QII", raw, 12 + 16 * k) for k in range(n)]
            offs = [e[0] for e in ent]
            if (offs[0] != 16) if n else (idx != 16):
                raise ValueError("corrupt index: the first block is not at offset 16")
            if any(b <= a for a, b in zip(offs, offs[1:])):
                raise ValueError("corrupt index: block offsets do not increase")
            if n and offs[-1] >= idx:
                raise ValueError("corrupt index: a block offset past the index")
            ends = offs[1:] + [idx]
            return Index([(o, e, ent[k][2]) for k, (o, e) in enumerate(zip(offs, ends))],
                         version, True)
        cnt = {}

        def read4(p):
            h = bytes(rd.read(p, min(p + 8, size)))
            if len(h) == 8:
                cnt[p] = struct.unpack_from("<I", h, 4)[0]
            return h[:4]
        blocks = _walk(read4, start, size, version)
        return Index([(s, e, cnt[s]) for s, e in blocks], version, False)
    finally:
        if close:
            rd.close()


def cover(index, first: int, count: int) -> list[tuple[int, int, int]]:
    """The blocks holding records [first, first + count) of the file, as
    (block, first record within it, records from it), in file order.  The
    range is clipped to the file's records; one starting at or past their
    end covers nothing.  Python ints throughout: files hold more than 2^32
    records."""
    import bisect
    if first < 0 or count < 0:
        raise ValueError("cover: negative record range")
    ends, tot = [], 0
    for _, _, n in index:
        tot += int(n)
        ends.append(tot)
    last = min(first + count, tot)
    out = []
    b = bisect.bisect_right(ends, first)          # the first block ending after `first`
    while b < len(ends) and first < last:
        b0 = ends[b] - int(index[b][2])
        k = min(last, ends[b]) - first
        if k:
            out.append((b, first - b0, k))
        first += k
        b += 1
    return out


def _check_entry(index, b: int, hv, a: int) -> None:
    """Block b as read (hv holds the file from offset a on) against its index
    entry: the size and record count in its header are the index's."""
    s, t, n = index[b]
    bsz, nrec = struct.unpack_from("<II", hv, s - a) if t - s >= 8 else (None, None)
    if bsz != t - s - 4 or nrec != n:
        raise _lib.NativeError(
            f"index disagrees with block {b}: size {bsz} records {nrec} in its header, "
            f"size {t - s - 4} records {n} in the index")


def _windows(rd, index, groups, device: str):
    """The blocks of the container behind `rd`, window by window: per group
    of `groups` (adjacent block numbers of `index`) one read, the blocks
    checked against their index entries, one upload; yields the _ReadWindow,
    unparsed.  One window's host and device buffers are alive at a time: a
    window is released before the next is read."""
    import torch
    for grp in groups:
        a, e = index[grp[0]][0], index[grp[-1]][1]
        with _stage("read"):
            hv = rd.read(a, e)
            if len(hv) != e - a:
                raise _lib.NativeError("index disagrees with the file: a block past its end")
        for b in grp:
            _check_entry(index, b, hv, a)
        with _stage("upload"):
            buf = torch.from_numpy(np.ascontiguousarray(hv)).to(device)   # blocking
        win = _ReadWindow(hv, buf, Blocks([(index[b][0] - a, index[b][1] - a) for b in grp],
                                      index.version), grp)
        del hv, buf
        yield win
        win.release()
        del win


def _index_windows(rd, index, device: str, window_bytes: int | None):
    """_windows over every block of the index, at most `window_bytes` each."""
    groups = _group(range(len(index)), lambda b: index[b][1] - index[b][0],
                    window_bytes or DEFAULT_WINDOW)
    return _windows(rd, index, groups, device)


def _extract_windows(rd, first: int, count: int, plus_name: bool, device: str, pairs: bool,
                     with_qual: bool, window_bytes: int | None):
    """The text of records [first, first + count) (pairs: of pairs) of the
    container behind `rd`, window by window: device tensors (pairs: the R1
    and the R2 text).  Every covering block is decoded whole and its text laid
    out by fqz5_fastq_format_range for the wanted records only; with_qual
    False: the quality sections are not decoded and the text is
    output_fasta's ('>' name, sequence)."""
    mul = 2 if pairs else 1
    with _stage("index"):
        index = read_index(rd)
        cov = cover(index, mul * first, mul * count)
    groups = _group(cov, lambda c: index[c[0]][1] - index[c[0]][0], window_bytes or DEFAULT_WINDOW)
    wins = _windows(rd, index, [[b for b, _, _ in grp] for grp in groups], device)
    for grp, win in zip(groups, wins):
        with _stage("decode"):
            win.parse()
            out_d, places = _decode_blocks(win, with_qual, device)
        with _stage("format"):
            texts = _format_blocks(win, places, plus_name, device, pairs,
                                   [(rf, rc) for _, rf, rc in grp])
        del out_d
        yield texts
        del texts


def extract_bytes(data, first: int, count: int, plus_name: bool = False, device: str = "cuda",
                  with_qual: bool = True) -> bytes:
    """Records [first, first + count) of a .fqz5 held in memory, as the
    text decompress_bytes gives for them: only the blocks that hold them
    (read_index, cover) are uploaded, checked and decoded.  with_qual False:
    the quality sections are not decoded and the text is FASTA ('>' name,
    sequence), as for a FASTA block either way."""
    out = [t[0].cpu().numpy().tobytes()
           for t in _extract_windows(_PosBytes(data), first, count, plus_name, device, False,
                                     with_qual, None)]
    _trace_dump("extract")
    return b"".join(out)


def _write_texts(outs, windows) -> list[int]:
    """The windows' texts (per window one device tensor per output) to the
    files `outs`: plain outputs by positioned writes as the windows come,
    gzip ones held and written whole.  Returns the bytes written per output."""
    sinks = [None if d.endswith(".gz") else _Sink(d, True) for d in outs]
    held = [[] for _ in outs]
    written = [0 for _ in outs]
    try:
        for texts in windows:
            for j, t in enumerate(texts):
                with _stage("download"):
                    out = _pinned(int(t.numel()))
                    out.copy_(t)
                with _stage("write"):
                    if sinks[j] is not None:
                        sinks[j].write_at(written[j], out.numpy())
                    else:
                        held[j].append(out.numpy().tobytes())
                    written[j] += int(t.numel())
                del out
    finally:
        for sk in sinks:
            if sk is not None:
                sk.close()
    with _stage("write"):
        for d, sk, h in zip(outs, sinks, held):
            if sk is None:
                _write_out(d, b"".join(h))
    return written


def extract_file(src: str, dst: str, first: int, count: int, plus_name: bool = False,
                 device: str = "cuda", dst2: str | None = None, with_qual: bool = True,
                 window_bytes: int | None = None) -> int:
    """Records [first, first + count) of the .fqz5 file src to dst, reading
    and decoding only the blocks that hold them: the index (one positioned
    read; the block headers of a file without one), then the covering blocks
    in windows of at most `window_bytes` of compressed data, each block
    checked against its index entry, CRC-checked and decoded whole, its text
    laid out on the GPU for the wanted records only.  dst2: first and count
    are in pairs, records 2 first .. 2 (first + count) deinterleaved to dst
    (R1) and dst2 (R2) as decompress_file(dst2=) does.  with_qual False: no
    quality section is decoded and the text is FASTA.  A ".gz" destination is
    gzip-compressed.  One process; returns the text bytes written."""
    pairs = dst2 is not None
    return sum(_run((_PosFile(src), True), "extract", lambda rd: _write_texts(
        [dst] + ([dst2] if pairs else []),
        _extract_windows(rd, first, count, plus_name, device, pairs, with_qual, window_bytes))))


# ---------------------------------------------------------------------------
# Lookup by read name
#
# A caller holds read names, not record numbers.  Names are in no order the
# index knows, so every block's name section is decoded, in one pass over the
# file: each window of blocks is read once, checked against the index,
# uploaded, parsed and CRC-checked whole (the CRC covers the block, and a
# skipped check could turn damage into a silent miss); then only its SEC_NAME
# sections go to the section decoder, and fqz5_names_match (name_match.hip)
# finds each block's records whose key is in the query table, on the device.
# Only the compacted hits come back to the host.  The extractors then decode
# the sequence (and quality) sections of the blocks with hits alone and lay
# out the text of the hit records with fqz5_fastq_format_list.  Output is in
# file order; a name several records carry yields all of them.  One process;
# no name index is kept between calls; "/1" and "/2" are part of a name.
# ---------------------------------------------------------------------------
class NameHits:
    """The result of a lookup by name: `records` (np.uint64) the file record
    numbers that matched, ascending (pairs: with their mates); `query`
    (np.int64) per record the index into the caller's names of the name it
    carries (the first occurrence of a name given twice), -1 for a mate taken
    only as partner; `missing` the names no record matched, in the caller's
    order; `written` the text bytes written (extract_names_file)."""

    def __init__(self, records, query, missing, written: int = 0):
        self.records, self.query, self.missing, self.written = records, query, missing, written


def read_name_list(path) -> list[bytes]:
    """A list of read names, one per line: the line end ('\\n', "\\r\\n") is
    dropped and empty lines are skipped; nothing else is stripped (a leading
    '@' stays part of the name)."""
    with open(path, "rb") as f:
        return [x for x in (ln.rstrip(b"\r\n") for ln in f) if x]


def _as_bytes(given, what: str):
    """The caller's names or patterns (`what` names them in errors) one by
    one as bytes: str ones are UTF-8; an empty one or one with a NUL byte is
    a ValueError."""
    for i, x in enumerate(given):
        b = x.encode() if isinstance(x, str) else bytes(x)
        if not b:
            raise ValueError(f"{what} {i} is empty")
        if b"\0" in b:
            raise ValueError(f"{what} {i} holds a NUL byte")
        yield b


def _queries(names):
    """The caller's names as (the names as given, the distinct names as
    bytes in order of first occurrence, for each of those the index of that
    first occurrence).  str names are UTF-8; an empty name is a ValueError."""
    given = list(names)
    qs, first, seen = [], [], set()
    for i, b in enumerate(_as_bytes(given, "read name")):
        if b not in seen:
            seen.add(b)
            qs.append(b)
            first.append(i)
    return given, qs, first


def _name_hits(given, first, records, qidx, written: int = 0) -> NameHits:
    """NameHits from the matcher's output: qidx per record the index of the
    distinct query it carries (0xFFFFFFFF: none, a mate)."""
    records = np.asarray(records, np.uint64)
    qidx = np.asarray(qidx, np.uint32)
    none = qidx == 0xFFFFFFFF
    fa = np.asarray(first, np.int64)
    query = np.full(len(qidx), -1, np.int64)
    if len(fa):
        query[~none] = fa[qidx[~none].astype(np.int64)]
    found = set(np.unique(qidx[~none]).tolist())
    missing = [given[i] for q, i in enumerate(first) if q not in found]
    return NameHits(records, query, missing, written)


class _Native:
    """A handle `p` of the library `so`, freed by its function FREE on close
    or on leaving the `with`."""
    p, FREE = None, ""

    def close(self) -> None:
        if self.p:
            getattr(self.so, self.FREE)(self.p)
            self.p = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class _NameTable(_Native):
    """fqz5_name_table of the distinct queries (freed on exit)."""
    FREE = "fqz5_names_table_free"

    def __init__(self, queries: list[bytes], tag_bits: int = 32):
        self.so = _load()
        blob = b"".join(q + b"\0" for q in queries)
        self.p = self.so.fqz5_names_table_build(blob, len(blob), len(queries), tag_bits)
        if not self.p:
            raise _lib.NativeError("fqz5_names_table_build: " + _lib.last_error())

    def find(self, key: bytes) -> int:
        return int(self.so.fqz5_names_table_find(self.p, key, len(key)))


def _key_windows(rd, keys: tuple, stages: tuple, match, pairs: bool, extract: bool,
                 plus_name: bool, with_qual: bool, device: str, window_bytes: int | None,
                 block_hook=None):
    """One pass over the container behind `rd` (see above), window by window,
    for a lookup whose keys are the sections `keys` ((SEC_NAME,): by read
    name, (SEC_SEQ,): by sequence content, the filter by read metrics: none,
    (SEC_SEQ,) or (SEC_SEQ, SEC_QUAL), a quality section after the bases its
    decoder reads): every block is read, checked and CRC-checked and the key
    sections of the window's blocks decoded in one call (none without keys);
    match(the block's device addresses by section, its BlockView, its record
    lengths, hits) leaves the block's compacted hits (record indices, query
    indices) in the device tensor `hits` and returns their number; the other
    sections are decoded for the blocks with hits alone.  A block without
    qualities under a SEC_QUAL key is an error that names it.  stages: the
    trace's names of the key stage and the match stage.  Yields (file record
    numbers of the window's hits, their query indices, the hits' text as
    device tensors or None without `extract`; pairs: R1 and R2 text).
    block_hook (the trimmer's): called before the format for every block with
    hits, once all its sections are decoded, as block_hook(the block's device
    addresses by section, which it may replace, its BlockView, its record
    lengths); it returns the record lengths the text is laid out with."""
    import functools
    import torch
    so = _load()
    with _stage("index"):
        index = read_index(rd)
    rec0 = [0]
    for _, _, n in index:
        rec0.append(rec0[-1] + int(n))            # (Python ints: more than 2^32 records)
    for win in _index_windows(rd, index, device, window_bytes):
        with _stage(stages[0] if keys else "parse"):
            win.parse()
            views, lens, fasta = win.views, win.lens, win.fasta
            if S.SEC_QUAL in keys and any(fasta):
                raise _lib.NativeError(f"block {win.blocks[fasta.index(True)]} has no qualities "
                                       "for a quality criterion")
            kulen = [win.field(j, sec)[2] for j in range(len(views)) for sec in keys]
            koff = np.concatenate([[0], np.cumsum(kulen)]).astype(np.int64)
            key_d = torch.empty(int(koff[-1]) + 1, dtype=torch.uint8, device=device)
            ptr = [{sec: key_d.data_ptr() + int(koff[j * len(keys) + i])
                    for i, sec in enumerate(keys)} for j in range(len(views))]

            def section(j, sec):          # (the quality decoder reads the block's decoded bases)
                return win.section(j, sec, ptr[j][sec],
                                   ptr[j][S.SEC_SEQ] if sec == S.SEC_QUAL else None)
            if keys:
                win.decode([section(j, sec) for j in range(len(views)) for sec in keys])
        recs, qidx, sels = [], [], {}
        with _stage(stages[1]):
            hits = torch.empty((2, max(max(len(ln) for ln in lens), 1)), dtype=torch.int32,
                               device=device)
            for j, ln in enumerate(lens):
                _lib.after_torch(device)          # (the last block's hits have been copied)
                n = match(ptr[j], views[j], ln, hits)
                if not n:
                    continue
                got = hits[:, :n].cpu().numpy().view(np.uint32)      # the compacted hits alone
                recs.append(got[0].astype(np.uint64) + np.uint64(rec0[win.blocks[j]]))
                qidx.append(got[1].copy())
                if extract:
                    sels[j] = hits[0, :n].clone()
        recs = np.concatenate(recs) if recs else np.zeros(0, np.uint64)
        qidx = np.concatenate(qidx) if qidx else np.zeros(0, np.uint32)
        if not extract:
            yield recs, qidx, None
            del key_d
            continue
        with _stage("decode"):
            rest, o = [], 0
            for j in sels:
                for sec in (S.SEC_NAME, S.SEC_SEQ, S.SEC_QUAL):
                    if sec in keys or (sec == S.SEC_QUAL and (fasta[j] or not with_qual)):
                        continue
                    rest.append((j, sec, o))
                    o += win.field(j, sec)[2]
            out_d = torch.empty(o + 1, dtype=torch.uint8, device=device)
            for j, sec, at in rest:
                ptr[j][sec] = out_d.data_ptr() + at
            if rest:
                win.decode([section(j, sec) for j, sec, _ in rest])
        with _stage("format"):
            flens = lens
            if block_hook is not None:
                flens = {j: block_hook(ptr[j], views[j], lens[j]) for j in sels}

            def fmt(j, out, cap):
                size, s1 = C.c_uint64(0), C.c_uint64(0)
                _check(so.fqz5_fastq_format_list(
                    ptr[j][S.SEC_NAME], views[j].name_ulen, ptr[j][S.SEC_SEQ],
                    ptr[j].get(S.SEC_QUAL) if with_qual else None, flens[j].ctypes.data,
                    len(lens[j]), sels[j].data_ptr(), int(sels[j].numel()), int(plus_name),
                    int(pairs), out, cap, C.byref(size), C.byref(s1)), "fqz5_fastq_format_list")
                return int(size.value), int(s1.value)
            _lib.after_torch(device)
            texts = _layout([functools.partial(fmt, j) for j in sels], pairs, device)
        yield recs, qidx, texts
        del key_d, out_d, texts


def _lookup(rd, keys: tuple, stages: tuple, match, pairs, extract, plus_name, with_qual, device,
            window_bytes, sink, block_hook=None):
    """_key_windows run to its end: (the hits' file record numbers, their
    query indices, the bytes sink(windows of texts) wrote with `extract`)."""
    recs, qidx = [], []

    def windows():
        for r, q, texts in _key_windows(rd, keys, stages, match, pairs, extract, plus_name,
                                        with_qual, device, window_bytes, block_hook):
            recs.append(r)
            qidx.append(q)
            yield texts
    if extract:
        written = sink(windows())
    else:
        written = 0
        for _ in windows():
            pass
    return (np.concatenate(recs) if recs else [], np.concatenate(qidx) if qidx else [], written)


def _find(rd, names, whole, pairs, extract, plus_name, with_qual, device, window_bytes, sink):
    """The lookup by name over `rd`; sink(windows of texts) consumes the
    hits' text (extract) and returns the bytes written."""
    given, qs, first = _queries(names)
    if not qs:
        return _name_hits(given, first, [], [], sink(iter(())) if extract else 0)
    so = _load()
    with _NameTable(qs) as tab:
        def match(ptr, v, ln, hits):
            n = C.c_uint64(0)
            _check(so.fqz5_names_match(tab.p, ptr[S.SEC_NAME], v.name_ulen, len(ln), int(whole),
                                       int(pairs), hits[0].data_ptr(), hits[1].data_ptr(),
                                       C.byref(n)),
                   "fqz5_names_match")
            return int(n.value)
        recs, qidx, written = _lookup(rd, (S.SEC_NAME,), ("names", "match"), match, pairs, extract,
                                      plus_name, with_qual, device, window_bytes, sink)
    return _name_hits(given, first, recs, qidx, written)


def find_names(src, names, whole: bool = False, pairs: bool = False, device: str = "cuda",
               window_bytes: int | None = None) -> NameHits:
    """The records of a .fqz5 (a path, the file's bytes, or a positioned
    reader) that carry one of `names` (bytes or str): every block is read,
    checked and CRC-checked, its name section alone decoded and matched on
    the GPU (see above); no sequence or quality section is decoded.  A
    record's key is its name up to the first ' ' or '\\t' (kseq's name), with
    `whole` the entire header line; keys are compared byte for byte.  pairs:
    a hit on record 2k or 2k + 1 selects both mates."""
    return _run(_reader(src), "find_names", lambda rd: _find(
        rd, names, whole, pairs, False, False, True, device, window_bytes, None))


def _bytes_sink(out: list):
    """The sink of the extractors to bytes: every window's text appended to
    `out`; returns the bytes held."""
    def sink(windows):
        for (t,) in windows:
            out.append(t.cpu().numpy().tobytes())
        return sum(len(x) for x in out)
    return sink


def extract_names_bytes(data, names, whole: bool = False, plus_name: bool = False,
                        with_qual: bool = True, device: str = "cuda") -> bytes:
    """The records of a .fqz5 held in memory that carry one of `names`, in
    file order, as the text decompress_bytes gives for them (with_qual
    False: FASTA text, no quality section decoded).  See find_names."""
    out = []
    _find(_PosBytes(data), names, whole, False, True, plus_name, with_qual, device, None,
          _bytes_sink(out))
    _trace_dump("extract_names")
    return b"".join(out)


def extract_names_file(src: str, dst: str, names, whole: bool = False, plus_name: bool = False,
                       device: str = "cuda", dst2: str | None = None, with_qual: bool = True,
                       window_bytes: int | None = None) -> NameHits:
    """The records of the .fqz5 file src that carry one of `names` to dst, in
    file order (never query order): one pass over the file in windows of at
    most `window_bytes` of compressed data; every block is read once, checked
    against its index entry and CRC-checked, and its name section decoded and
    matched on the GPU; the sequence and quality sections are decoded for the
    blocks with hits only, and the hits' text is laid out on the GPU
    (fqz5_fastq_format_list).  dst2: the records are interleaved pairs, a hit
    on either mate takes both, R1 records to dst and R2 records to dst2.
    with_qual False: no quality section is decoded and the text is FASTA.  A
    ".gz" destination is gzip-compressed.  One process; returns the NameHits
    (`written`: the text bytes written)."""
    outs = [dst] + ([dst2] if dst2 is not None else [])
    return _run((_PosFile(src), True), "extract_names", lambda rd: _find(
        rd, names, whole, dst2 is not None, True, plus_name, with_qual, device, window_bytes,
        lambda w: sum(_write_texts(outs, w))))


# ---------------------------------------------------------------------------
# Lookup by sequence content
#
# "The reads that contain this adapter / barcode / primer / k-mer list": the
# pass of the lookup by name with the sequence section as the key.  Every
# block is read once, checked against the index and CRC-checked; only its
# SEC_SEQ section goes to the section decoder (it decodes on its own), and
# fqz5_seqs_match (seq_match.hip) scans the bases for the patterns on the
# device.  The extractors decode the name (and quality) sections of the
# blocks with hits alone.  A record hits when its sequence line holds a
# pattern as a contiguous substring, byte for byte; revcomp also searches
# each pattern's reverse complement, which this layer expands into queries of
# its own (the kernel knows nothing of strands).  Not built: mismatches or
# edit distance, IUPAC expansion, case folding, the positions of occurrences,
# several ranks, a k-mer index kept between calls.
# ---------------------------------------------------------------------------
class SeqHits:
    """The result of a lookup by sequence: `records` (np.uint64) the file
    record numbers that hold a pattern, ascending (pairs: with their mates);
    `query` (np.int64) per record the index into the caller's patterns of the
    first one, in list order, that occurs in it (forward before reverse
    complement for one pattern), -1 for a mate taken only as partner;
    `reverse` (bool) whether that occurrence is the pattern's reverse
    complement; `missing` the caller's patterns that occur in no record (on
    either strand with revcomp), in the caller's order; `written` the text
    bytes written (extract_seqs_file)."""

    def __init__(self, records, query, reverse, missing, written: int = 0):
        self.records, self.query, self.reverse = records, query, reverse
        self.missing, self.written = missing, written


def read_pattern_list(path) -> list[bytes]:
    """A list of patterns, one per line, line ends ('\\n', "\\r\\n") dropped and
    empty lines skipped.  A FASTA file (its first such line starts with '>')
    gives its sequences, the lines of a wrapped one joined."""
    with open(path, "rb") as f:
        lines = [x for x in (ln.rstrip(b"\r\n") for ln in f) if x]
    if not lines or not lines[0].startswith(b">"):
        return lines
    out, cur = [], None
    for ln in lines:
        if ln.startswith(b">"):
            if cur:
                out.append(cur)
            cur = b""
        else:
            cur += ln
    if cur:
        out.append(cur)
    return out


_COMPLEMENT = bytes.maketrans(b"ACGTacgtNn", b"TGCAtgcaNn")


def _seq_queries(patterns, revcomp: bool):
    """The caller's patterns as (the patterns as given, the distinct internal
    queries, for each of those (index of the caller's pattern it first stands
    for, whether as its reverse complement)).  The queries come in the order
    fwd(0), rc(0), fwd(1), rc(1), ...; one equal to an earlier query is
    dropped (a palindrome has no rc of its own).  str patterns are UTF-8; an
    empty pattern, one with a NUL byte and, with revcomp, one with a byte
    outside ACGTNacgtn is a ValueError."""
    given = list(patterns)
    qs, origin, seen = [], [], set()
    for i, b in enumerate(_as_bytes(given, "pattern")):
        forms = [(b, False)]
        if revcomp:
            if b.translate(None, b"ACGTacgtNn"):
                raise ValueError(f"pattern {i} holds a byte without a complement (not ACGTN)")
            forms.append((b.translate(_COMPLEMENT)[::-1], True))
        for f, rev in forms:
            if f not in seen:
                seen.add(f)
                qs.append(f)
                origin.append((i, rev))
    return given, qs, origin


def _seq_hits(given, qs, origin, revcomp: bool, records, qidx, seen, written: int = 0) -> SeqHits:
    """SeqHits from the matcher's output: qidx per record the index of the
    lowest query it holds (0xFFFFFFFF: none, a mate), seen per query whether
    it occurs in any record."""
    records = np.asarray(records, np.uint64)
    qidx = np.asarray(qidx, np.uint32)
    none = qidx == 0xFFFFFFFF
    query = np.full(len(qidx), -1, np.int64)
    reverse = np.zeros(len(qidx), bool)
    if len(origin):
        at = qidx[~none].astype(np.int64)
        query[~none] = np.asarray([i for i, _ in origin], np.int64)[at]
        reverse[~none] = np.asarray([r for _, r in origin], bool)[at]
    where = {q: k for k, q in enumerate(qs)}
    missing, done = [], set()
    for x, b in zip(given, _as_bytes(given, "pattern")):
        if b in done:
            continue
        done.add(b)
        forms = [b] + ([b.translate(_COMPLEMENT)[::-1]] if revcomp else [])
        if not any(seen[where[f]] for f in forms):
            missing.append(x)
    return SeqHits(records, query, reverse, missing, written)


class _SeqTable(_Native):
    """fqz5_seq_table of the distinct queries (freed on exit)."""
    FREE = "fqz5_seqs_table_free"

    def __init__(self, queries: list[bytes], tag_bits: int = 32, anchor: int = 0):
        self.so = _load()
        blob = b"".join(q + b"\0" for q in queries)
        self.p = self.so.fqz5_seqs_table_build(blob, len(blob), len(queries), tag_bits, anchor)
        if not self.p:
            raise _lib.NativeError("fqz5_seqs_table_build: " + _lib.last_error())
        self.anchor = int(self.so.fqz5_seqs_table_anchor(self.p))

    def scan_host(self, seq: bytes, lens, nq: int):
        """fqz5_seqs_scan_host: (hit per record, seen per query)."""
        lens = np.ascontiguousarray(lens, np.uint32)
        hit = np.zeros(len(lens), np.uint32)
        seen = np.zeros(nq, np.uint8)
        _check(self.so.fqz5_seqs_scan_host(self.p, seq, len(seq), lens.ctypes.data, len(lens),
                                           hit.ctypes.data, seen.ctypes.data), "fqz5_seqs_scan_host")
        return hit, seen


def _find_seqs(rd, patterns, revcomp, pairs, extract, plus_name, with_qual, device, window_bytes,
               sink):
    """The lookup by sequence over `rd`; sink(windows of texts) consumes the
    hits' text (extract) and returns the bytes written."""
    with _stage("table"):
        given, qs, origin = _seq_queries(patterns, revcomp)
    if not qs:
        return _seq_hits(given, qs, origin, revcomp, [], [], [], sink(iter(())) if extract else 0)
    import torch
    so = _load()
    with _stage("table"):
        tab = _SeqTable(qs)
    with tab:
        seen = torch.zeros(len(qs), dtype=torch.uint8, device=device)

        def match(ptr, v, ln, hits):
            n = C.c_uint64(0)
            _check(so.fqz5_seqs_match(tab.p, ptr[S.SEC_SEQ], v.seq_ulen, ln.ctypes.data, len(ln),
                                      int(pairs), hits[0].data_ptr(), hits[1].data_ptr(),
                                      C.byref(n), seen.data_ptr()), "fqz5_seqs_match")
            return int(n.value)
        recs, qidx, written = _lookup(rd, (S.SEC_SEQ,), ("seqs", "match"), match, pairs, extract,
                                      plus_name, with_qual, device, window_bytes, sink)
        seen = seen.cpu().numpy()
    with _stage("result"):
        return _seq_hits(given, qs, origin, revcomp, recs, qidx, seen, written)


def find_seqs(src, patterns, revcomp: bool = False, pairs: bool = False, device: str = "cuda",
              window_bytes: int | None = None) -> SeqHits:
    """The records of a .fqz5 (a path, the file's bytes, or a positioned
    reader) whose sequence holds one of `patterns` (bytes or str) as a
    contiguous substring: every block is read, checked and CRC-checked, its
    sequence section alone decoded and scanned on the GPU (see above); no name
    or quality section is decoded.  Bytes are compared as they are (case
    matters, 'N' is an ordinary byte); an occurrence never spans two records.
    revcomp: each pattern's reverse complement (A<->T, C<->G, N; other bytes
    are a ValueError) is searched as well.  pairs: a hit on record 2k or
    2k + 1 selects both mates."""
    return _run(_reader(src), "find_seqs", lambda rd: _find_seqs(
        rd, patterns, revcomp, pairs, False, False, True, device, window_bytes, None))


def extract_seqs_bytes(data, patterns, revcomp: bool = False, plus_name: bool = False,
                       with_qual: bool = True, device: str = "cuda") -> bytes:
    """The records of a .fqz5 held in memory whose sequence holds one of
    `patterns`, in file order, as the text decompress_bytes gives for them
    (with_qual False: FASTA text, no quality section decoded).  See
    find_seqs."""
    out = []
    _find_seqs(_PosBytes(data), patterns, revcomp, False, True, plus_name, with_qual, device, None,
               _bytes_sink(out))
    _trace_dump("extract_seqs")
    return b"".join(out)


def extract_seqs_file(src: str, dst: str, patterns, revcomp: bool = False, plus_name: bool = False,
                      device: str = "cuda", dst2: str | None = None, with_qual: bool = True,
                      window_bytes: int | None = None) -> SeqHits:
    """The records of the .fqz5 file src whose sequence holds one of
    `patterns` to dst, in file order: one pass over the file in windows of at
    most `window_bytes` of compressed data; every block is read once, checked
    against its index entry and CRC-checked, and its sequence section decoded
    and scanned on the GPU; the name and quality sections are decoded for the
    blocks with hits only, and the hits' text is laid out on the GPU
    (fqz5_fastq_format_list).  dst2: the records are interleaved pairs, a hit
    on either mate takes both, R1 records to dst and R2 records to dst2.
    with_qual False: no quality section is decoded and the text is FASTA.  A
    ".gz" destination is gzip-compressed.  One process; returns the SeqHits
    (`written`: the text bytes written)."""
    outs = [dst] + ([dst2] if dst2 is not None else [])
    return _run((_PosFile(src), True), "extract_seqs", lambda rd: _find_seqs(
        rd, patterns, revcomp, dst2 is not None, True, plus_name, with_qual, device, window_bytes,
        lambda w: sum(_write_texts(outs, w))))


# ---------------------------------------------------------------------------
# File statistics
#
# "What is in this file?": read and base counts, the length distribution and
# Nx, base composition and GC content, the quality distribution and quality
# by cycle, without decoding a name, laying out text or downloading anything
# but the final tables.  One pass over the file in windows, as the lookups
# walk it: every block is read, checked against its index entry, parsed and
# CRC-checked; one section decode per window holds the SEC_SEQ section of
# every block and the SEC_QUAL section of every block that has one (FASTA
# blocks have none; their records count in the length and base tables only);
# fqz5_stats_add (stats.hip) then histograms each block's bases and qualities
# into one device accumulator, which comes back once at the end.  The length
# distribution is built here from the lengths the block headers give and kept
# sparse.  One process.  Not built: several ranks, per-tile or flowcell
# statistics from the names, k-mer or duplication levels, adapter content.
# ---------------------------------------------------------------------------
STATS_CYCLES_MAX = 1 << 16


def _stats_unpack(flat: np.ndarray, cycles: int, mates: int) -> dict:
    """The tables of fqz5_stats_read / fqz5_stats_host (include/fqz5_fastq.h)
    as arrays with a leading axis of `mates`."""
    t = np.asarray(flat, np.uint64).reshape(mates, 873 + 262 * cycles)
    cb = 873 + 6 * cycles
    return {"records": t[:, 0].copy(), "bases": t[:, 1].copy(), "qual_records": t[:, 2].copy(),
            "empty": t[:, 3].copy(), "base_counts": t[:, 4:260].copy(),
            "qual_counts": t[:, 260:516].copy(), "read_qual": t[:, 516:772].copy(),
            "read_gc": t[:, 772:873].copy(),
            "cycle_base": t[:, 873:cb].reshape(mates, cycles, 6).copy(),
            "cycle_qual": t[:, cb:].reshape(mates, cycles, 256).copy()}


def _stats_host(seq: bytes, qual, lens, cycles: int, mates: int, out=None, per_record=False):
    """fqz5_stats_host of one block added to `out` (a new zeroed table by
    default): (the flat table, record_qsum, record_gc)."""
    so = _load()
    lens = np.ascontiguousarray(lens, np.uint32)
    if out is None:
        out = np.zeros(int(so.fqz5_stats_words(cycles, mates)), np.uint64)
    qs = np.zeros(len(lens), np.uint64) if per_record else None
    gc = np.zeros(len(lens), np.uint32) if per_record else None
    _check(so.fqz5_stats_host(cycles, mates, bytes(seq), None if qual is None else bytes(qual),
                              len(seq), lens.ctypes.data, len(lens), out.ctypes.data, len(out),
                              qs.ctypes.data if per_record else None,
                              gc.ctypes.data if per_record else None), "fqz5_stats_host")
    return out, qs, gc


class _StatsAcc(_Native):
    """fqz5_stats, the device accumulator (freed on exit)."""
    FREE = "fqz5_stats_free"

    def __init__(self, cycles: int, mates: int):
        self.so = _load()
        self.cycles, self.mates = cycles, mates
        self.p = self.so.fqz5_stats_new(cycles, mates)
        if not self.p:
            raise _lib.NativeError("fqz5_stats_new: " + _lib.last_error())

    def add(self, d_seq: int, d_qual, seq_len: int, lens, d_qsum=None, d_gc=None) -> int:
        """fqz5_stats_add's return code (callers raise)."""
        lens = np.ascontiguousarray(lens, np.uint32)
        return self.so.fqz5_stats_add(self.p, d_seq, d_qual, seq_len, lens.ctypes.data, len(lens),
                                      d_qsum, d_gc)

    def read(self) -> np.ndarray:
        out = np.zeros(int(self.so.fqz5_stats_words(self.cycles, self.mates)), np.uint64)
        _check(self.so.fqz5_stats_read(self.p, out.ctypes.data, len(out)), "fqz5_stats_read")
        return out


def _merge_lengths(a, b):
    """Two sparse length distributions (values ascending, counts) as one."""
    v, inv = np.unique(np.concatenate([a[0], b[0]]), return_inverse=True)
    c = np.zeros(len(v), np.uint64)
    np.add.at(c, inv, np.concatenate([a[1], b[1]]))
    return v, c


class Stats:
    """The result of stats(): every table has a leading axis of `mates` (1,
    or 2 with pairs: record r of the file belongs to mate r & 1), counts are
    np.uint64.

    records, bases, qual_records (records of blocks that have qualities),
    empty (records of length 0): [mates].
    lengths: per mate (distinct record lengths ascending, their counts).
    base_counts [mates, 256]: each sequence byte, case kept; qual_counts
    [mates, 256]: each quality (the quality line's byte - 33).
    cycles: C = min(the caller's cap, the longest record of the file);
    cycle_base [mates, C, 6]: at position c the records longer than c by their
    base there: A, C, G, T, N, other (case folded); cycle_qual [mates, C, 256]:
    likewise by quality.
    read_qual [mates, 256]: records with qualities and length L > 0 by
    floor(sum of qualities / L); read_gc [mates, 101]: records of length L > 0
    by floor(100 * G/C bases / L).
    record_len (u32), record_gc (u32), record_qsum (u64, 0 without
    qualities): per record in file order with per_record, else None."""

    def __init__(self, mates: int, tables: dict, lengths, cycles: int, record_len=None,
                 record_gc=None, record_qsum=None):
        self.mates, self.cycles, self.lengths = mates, cycles, lengths
        for k, v in tables.items():
            setattr(self, k, v)
        self.record_len, self.record_gc, self.record_qsum = record_len, record_gc, record_qsum

    def nx(self, x: float, mate: int = 0) -> int:
        """The Nx length: the largest v such that the records of length >= v
        hold at least x % of the mate's bases (N50: nx(50)); 0 without bases."""
        v, c = self.lengths[mate]
        total = sum(int(a) * int(b) for a, b in zip(v, c))
        cum = 0
        for a, b in zip(v[::-1], c[::-1]):
            cum += int(a) * int(b)
            if total and cum * 100 >= x * total:
                return int(a)
        return 0


def _stats(rd, cycles: int, mates: int, per_record: bool, device: str, window_bytes) -> Stats:
    import torch
    with _stage("index"):
        index = read_index(rd)
    none = (np.zeros(0, np.uint32), np.zeros(0, np.uint64))
    lengths = [none] * mates
    rlen, rgc, rqs = [], [], []
    with _StatsAcc(cycles, mates) as acc:
        for win in _index_windows(rd, index, device, window_bytes):
            with _stage("decode"):
                win.parse()
                views, lens, fasta = win.views, win.lens, win.fasta
                # per block its bases, then (unless FASTA) its qualities
                at = np.concatenate([[0], np.cumsum([v.seq_ulen * (1 if fa else 2)
                                                     for v, fa in zip(views, fasta)])])
                out_d = torch.empty(int(at[-1]) + 1, dtype=torch.uint8, device=device)
                secs = []
                for j, (v, fa) in enumerate(zip(views, fasta)):
                    d_seq = out_d.data_ptr() + int(at[j])
                    secs.append(win.section(j, S.SEC_SEQ, d_seq))
                    if not fa:
                        secs.append(win.section(j, S.SEC_QUAL, d_seq + v.seq_ulen, d_seq))
                win.decode(secs)
            with _stage("stats"):
                nw = sum(len(ln) for ln in lens)
                if per_record:
                    qs_d = torch.empty(nw + 1, dtype=torch.int64, device=device)
                    gc_d = torch.empty(nw + 1, dtype=torch.int32, device=device)
                _lib.after_torch(device)
                r0 = 0
                for j, (v, ln, fa) in enumerate(zip(views, lens, fasta)):
                    d_seq = out_d.data_ptr() + int(at[j])
                    _check(acc.add(d_seq, None if fa else d_seq + v.seq_ulen, v.seq_ulen, ln,
                                   qs_d.data_ptr() + 8 * r0 if per_record else None,
                                   gc_d.data_ptr() + 4 * r0 if per_record else None),
                           "fqz5_stats_add")
                    r0 += len(ln)
                for m in range(mates):
                    for ln in lens:
                        v, c = np.unique(ln[m::mates], return_counts=True)
                        lengths[m] = _merge_lengths(lengths[m], (v, c.astype(np.uint64)))
                if per_record:
                    rlen.extend(lens)
                    rqs.append(qs_d[:nw].cpu().numpy().view(np.uint64))
                    rgc.append(gc_d[:nw].cpu().numpy().view(np.uint32))
            del out_d
        with _stage("result"):
            flat = acc.read()
    with _stage("result"):
        longest = max((int(v[-1]) for v, _ in lengths if len(v)), default=0)
        c = min(cycles, longest)
        tab = _stats_unpack(flat, cycles, mates)
        tab["cycle_base"] = tab["cycle_base"][:, :c].copy()
        tab["cycle_qual"] = tab["cycle_qual"][:, :c].copy()
        cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
        return Stats(mates, tab, lengths, c,
                     *((cat(rlen, np.uint32), cat(rgc, np.uint32), cat(rqs, np.uint64))
                       if per_record else ()))


def stats(src, cycles: int = 1024, pairs: bool = False, per_record: bool = False,
          device: str = "cuda", window_bytes: int | None = None) -> Stats:
    """Read QC statistics of a .fqz5 (a path, the file's bytes, or a
    positioned reader) as a Stats, histogrammed on the GPU (see above): one
    pass in windows of at most `window_bytes` of compressed data; every block
    is read once, checked against its index entry and CRC-checked, and its
    sequence and quality sections decoded; no name section is decoded, no
    text is formatted and only the tables come back.  cycles: the cap on the
    per-cycle tables, 1..65536.  pairs: the records are interleaved pairs and
    every table is kept per mate (a block with an odd record count is an
    error).  per_record: also each record's length, G/C count and quality sum,
    in file order.  One process."""
    if not 1 <= cycles <= STATS_CYCLES_MAX:
        raise ValueError(f"stats: cycles {cycles} not in 1..{STATS_CYCLES_MAX}")
    return _run(_reader(src), "stats", lambda rd: _stats(
        rd, cycles, 2 if pairs else 1, per_record, device, window_bytes))


# ---------------------------------------------------------------------------
# Filter by read metrics
#
# "The reads worth keeping": long enough, mean quality high enough, not full
# of N, not too many low-quality bases, sane GC, not low-complexity (what
# fastp, seqkit seq -m/-Q and vsearch --fastq_filter do first).  The pass is
# the lookups' (_key_windows) with a set of key sections the criteria decide:
# none for length criteria alone (the lengths come from the block headers),
# SEC_SEQ for a base criterion, SEC_SEQ and SEC_QUAL for a quality criterion
# (the quality decoder reads the block's bases).  The key sections of a
# window's blocks are decoded in one call, fqz5_filter_match (filter.hip) sums
# each block's records and picks on the device, and the remaining sections are
# decoded in one further call for the blocks with hits alone.  The rule is
# exact integer arithmetic (include/fqz5_fastq.h); a pair is kept only when
# both mates pass.  One process.  Not built: expected-error (maxee) filters,
# several ranks (trimming, clipping and the adapter cut: "Trim and clip" below).
# ---------------------------------------------------------------------------
class _FilterSpec(C.Structure):
    """fqz5_filter_spec (include/fqz5_fastq.h)"""
    _fields_ = [("set", C.c_uint32), ("min_mean_q", C.c_uint32), ("low_q", C.c_uint32),
                ("max_low_pct", C.c_uint32), ("gc_min_pct", C.c_uint32), ("gc_max_pct", C.c_uint32),
                ("min_complexity_pct", C.c_uint32), ("min_len", C.c_uint64),
                ("max_len", C.c_uint64), ("max_n", C.c_uint64)]


class _FilterSums(C.Structure):
    """fqz5_filter_sums: addresses of n, gc, diff (u32), qsum (u64), lowq (u32)"""
    _fields_ = [(k, C.c_void_p) for k in ("n", "gc", "diff", "qsum", "lowq")]


class Filter:
    """The criteria of filter_records / filter_file; one left None is off.
    Integers throughout, the rule exact (include/fqz5_fastq.h): a record of
    length L passes when
      min_len, max_len       min_len <= L <= max_len
      max_n                  its bytes in "Nn" <= max_n
      min_mean_q             the sum of its qualities >= min_mean_q * L
      low_q, max_low_pct     100 * (its qualities < low_q) <= max_low_pct * L
                             (given together)
      gc_pct = (lo, hi)      lo * L <= 100 * (its bytes in "GCgc") <= hi * L
      min_complexity_pct     100 * (its positions that differ from their
                             right-hand neighbour) >= min_complexity_pct *
                             max(L - 1, 0)
    A quality is the quality line's byte - 33.  ValueError: a negative value,
    a percentage over 100, lo > hi, low_q without max_low_pct or the reverse,
    min_len > max_len."""

    def __init__(self, min_len=None, max_len=None, max_n=None, min_mean_q=None, low_q=None,
                 max_low_pct=None, gc_pct=None, min_complexity_pct=None):
        import operator
        lo, hi = (None, None) if gc_pct is None else gc_pct
        vals = {"min_len": min_len, "max_len": max_len, "max_n": max_n, "min_mean_q": min_mean_q,
                "low_q": low_q, "max_low_pct": max_low_pct, "gc_pct lo": lo, "gc_pct hi": hi,
                "min_complexity_pct": min_complexity_pct}
        for k, v in vals.items():
            if v is None:
                continue
            vals[k] = v = operator.index(v)
            if v < 0:
                raise ValueError(f"Filter: {k} is negative")
            if (k.endswith("_pct") or k.startswith("gc_pct")) and v > 100:
                raise ValueError(f"Filter: {k} is a percentage over 100")
        if gc_pct is not None and (vals["gc_pct lo"] is None or vals["gc_pct hi"] is None):
            raise ValueError("Filter: gc_pct is (lo, hi)")
        if gc_pct is not None and vals["gc_pct lo"] > vals["gc_pct hi"]:
            raise ValueError("Filter: gc_pct has lo > hi")
        if (low_q is None) != (max_low_pct is None):
            raise ValueError("Filter: low_q and max_low_pct go together")
        if min_len is not None and max_len is not None and vals["min_len"] > vals["max_len"]:
            raise ValueError("Filter: min_len > max_len")
        self.min_len, self.max_len, self.max_n = vals["min_len"], vals["max_len"], vals["max_n"]
        self.min_mean_q, self.low_q = vals["min_mean_q"], vals["low_q"]
        self.max_low_pct, self.min_complexity_pct = vals["max_low_pct"], vals["min_complexity_pct"]
        self.gc_pct = None if gc_pct is None else (vals["gc_pct lo"], vals["gc_pct hi"])

    def spec(self) -> _FilterSpec:
        """The criteria as the library takes them (values past a field's range
        clipped to it: no record is that long, no quality sum that large)."""
        f = _FilterSpec()
        u32, u64 = (1 << 32) - 1, (1 << 64) - 1
        for k, (name, top) in enumerate((("min_len", u64), ("max_len", u64), ("max_n", u64),
                                         ("min_mean_q", u32), ("low_q", u32), (None, 0),
                                         ("min_complexity_pct", u32))):
            v = getattr(self, name) if name else None
            if v is not None:
                f.set |= 1 << k
                setattr(f, name, min(v, top))
        if self.low_q is not None:
            f.max_low_pct = self.max_low_pct
        if self.gc_pct is not None:
            f.set |= 1 << 5
            f.gc_min_pct, f.gc_max_pct = self.gc_pct
        return f

    def keys(self) -> tuple:
        """The sections the criteria are judged on (see above)."""
        if self.min_mean_q is not None or self.low_q is not None:
            return (S.SEC_SEQ, S.SEC_QUAL)
        if self.max_n is not None or self.gc_pct is not None or self.min_complexity_pct is not None:
            return (S.SEC_SEQ,)
        return ()


class FilterHits:
    """The result of a filter: `records` (np.uint64) the file record numbers
    selected, ascending (pairs: both mates); `total` the units seen (records,
    with pairs pairs); `failed` (np.uint64[7]) the units that failed, by the
    lowest criterion they fail in the order of REASONS (with invert these are
    the units selected); `written` the text bytes written (filter_file)."""
    REASONS = ("min_len", "max_len", "max_n", "min_mean_q", "low_q", "gc_pct",
               "min_complexity_pct")

    def __init__(self, records, total: int, failed, written: int = 0):
        self.records, self.total, self.failed, self.written = records, total, failed, written


def _filter_host(flt: Filter, seq, qual, lens, pairs: bool = False, invert: bool = False):
    """fqz5_filter_host of one block: (keep per record, failed[7], the sums
    n, gc, diff, qsum, lowq)."""
    so = _load()
    lens = np.ascontiguousarray(lens, np.uint32)
    keep = np.zeros(len(lens), np.uint8)
    failed = np.zeros(7, np.uint64)
    sums = [np.zeros(len(lens), np.uint64 if k == 3 else np.uint32) for k in range(5)]
    spec = flt.spec()
    _check(so.fqz5_filter_host(C.byref(spec), None if seq is None else bytes(seq),
                               None if qual is None else bytes(qual),
                               len(seq) if seq is not None else int(lens.astype(np.uint64).sum()),
                               lens.ctypes.data, len(lens), int(pairs), int(invert),
                               keep.ctypes.data, failed.ctypes.data,
                               C.byref(_FilterSums(*(a.ctypes.data for a in sums)))),
           "fqz5_filter_host")
    return keep, failed, sums


def _filter(rd, flt: Filter, pairs, invert, extract, plus_name, with_qual, device, window_bytes,
            sink) -> FilterHits:
    """The filter over `rd`; sink(windows of texts) consumes the selected
    records' text (extract) and returns the bytes written."""
    if not isinstance(flt, Filter):
        raise TypeError("the criteria are a Filter")
    so = _load()
    spec, failed, total = flt.spec(), np.zeros(7, np.uint64), [0]

    def match(ptr, v, ln, hits):
        n = C.c_uint64(0)
        _check(so.fqz5_filter_match(C.byref(spec), ptr.get(S.SEC_SEQ), ptr.get(S.SEC_QUAL),
                                    v.seq_ulen, ln.ctypes.data, len(ln), int(pairs), int(invert),
                                    hits[0].data_ptr(), C.byref(n), failed.ctypes.data, None),
               "fqz5_filter_match")
        total[0] += len(ln) // (2 if pairs else 1)
        return int(n.value)
    recs, _, written = _lookup(rd, flt.keys(), ("keys", "filter"), match, pairs, extract, plus_name,
                               with_qual, device, window_bytes, sink)
    return FilterHits(np.asarray(recs, np.uint64), total[0], failed, written)


def filter_records(src, flt: Filter, pairs: bool = False, invert: bool = False,
                   device: str = "cuda", window_bytes: int | None = None) -> FilterHits:
    """The records of a .fqz5 (a path, the file's bytes, or a positioned
    reader) that pass the criteria `flt`, judged on the GPU (see above): every
    block is read, checked and CRC-checked; only the sections the criteria
    need are decoded (none for length criteria alone) and no name section.
    pairs: records 2k and 2k + 1 are one unit, kept only when both mates pass
    (a block with an odd record count is an error).  invert: exactly the units
    that do not pass.  A quality criterion on a block without qualities is an
    error."""
    return _run(_reader(src), "filter_records", lambda rd: _filter(
        rd, flt, pairs, invert, False, False, True, device, window_bytes, None))


def filter_bytes(data, flt: Filter, plus_name: bool = False, with_qual: bool = True,
                 invert: bool = False, device: str = "cuda") -> bytes:
    """The records of a .fqz5 held in memory that pass `flt`, in file order,
    as the text decompress_bytes gives for them (with_qual False: FASTA
    text).  See filter_records."""
    out = []
    _filter(_PosBytes(data), flt, False, invert, True, plus_name, with_qual, device, None,
            _bytes_sink(out))
    _trace_dump("filter")
    return b"".join(out)


def filter_file(src: str, dst: str, flt: Filter, plus_name: bool = False, device: str = "cuda",
                dst2: str | None = None, with_qual: bool = True, invert: bool = False,
                window_bytes: int | None = None) -> FilterHits:
    """The records of the .fqz5 file src that pass `flt` to dst, in file
    order: one pass over the file in windows of at most `window_bytes` of
    compressed data; every block is read once, checked against its index entry
    and CRC-checked, the sections the criteria need decoded and judged on the
    GPU; the remaining sections are decoded for the blocks with selected
    records only, and their text is laid out on the GPU
    (fqz5_fastq_format_list).  dst2: the records are interleaved pairs, a pair
    is kept only when both mates pass, R1 records to dst and R2 records to
    dst2.  with_qual False: the text is FASTA, and no quality section is
    decoded unless a criterion needs it.  invert: the records that do not
    pass.  A ".gz" destination is gzip-compressed.  One process; returns the
    FilterHits (`written`: the text bytes written)."""
    outs = [dst] + ([dst2] if dst2 is not None else [])
    return _run((_PosFile(src), True), "filter", lambda rd: _filter(
        rd, flt, dst2 is not None, invert, True, plus_name, with_qual, device, window_bytes,
        lambda w: sum(_write_texts(outs, w))))


# ---------------------------------------------------------------------------
# Trim and clip
#
# "Clip fixed bases, trim low-quality ends, cut the 3' adapter, strip N ends,
# crop, then filter what is left" (fastp, cutadapt): the pass of the filter,
# with the records changed before they are judged and written.  The keys are
# the sections the cut points are judged on (none for clip and crop alone,
# SEC_SEQ for adapters or trim_n, SEC_SEQ and SEC_QUAL for a quality cutoff)
# together with the filter's.  Per block fqz5_trim_cuts (trim.hip) finds every
# record's kept interval on the device, fqz5_trim_gather compacts the key
# streams to those intervals into buffers of their own, and from there they are
# ordinary streams with new lengths: fqz5_filter_match judges them (an empty
# Filter selects every record) and fqz5_fastq_format_list lays out their text,
# both unchanged.  Sections that were no key are decoded for the blocks with
# selected records as in every lookup and compacted before the format
# (_key_windows' block_hook).  Names are never trimmed, and a record trimmed to
# nothing is still a record; only the Filter drops records (its min_len is the
# "too short after trimming" rule).  The rule is exact integer arithmetic
# (include/fqz5_fastq.h).  One process.  Not built: poly-G / poly-X tails, 5'
# and linked adapters, indels in the adapter match, wildcards and case folding,
# paired-overlap adapter detection, several ranks, writing .fqz5 directly.
# ---------------------------------------------------------------------------
TRIM_ADAPTERS, TRIM_ADAPTER_MAX = 16, 128


class _TrimSpec(C.Structure):
    """fqz5_trim_spec (include/fqz5_fastq.h)"""
    _fields_ = [("set", C.c_uint32), ("q5", C.c_uint32), ("q3", C.c_uint32),
                ("min_overlap", C.c_uint32), ("max_err_pct", C.c_uint32),
                ("n_adapters", C.c_uint32 * 2), ("head", C.c_uint64), ("tail", C.c_uint64),
                ("max_len", C.c_uint64)]


class _TrimAdapters(C.Structure):
    """fqz5_trim_adapters"""
    _fields_ = [("len", C.c_uint32 * (2 * TRIM_ADAPTERS)),
                ("bytes", (C.c_uint8 * TRIM_ADAPTER_MAX) * (2 * TRIM_ADAPTERS))]


class Trim:
    """The steps of trim_records / trim_file, applied to every record in this
    order; one left None (False, no adapters) is off.  Integers throughout,
    the rule exact (include/fqz5_fastq.h); a quality is the quality line's
    byte - 33:
      head, tail     fixed bases off the 5' and the 3' end
      q5, q3         the low-quality 5' / 3' end by the running-sum rule of BWA
                     and cutadapt, each judged on what the clip left
      adapters       3' adapters (bytes or str): the record is cut at the first
                     position where one matches over min(its length, what is
                     left of the read) >= min_overlap bases with at most
                     max_err_pct percent of them mismatches (no indels, bytes
                     compared as they are); adapters2: those of the odd
                     records of interleaved pairs
      trim_n         N and n off both ends
      max_len        at most that many bases from the 5' end of what is left
    ValueError: a negative value, a cutoff over 93, max_err_pct over 100,
    min_overlap below 1, an empty adapter or one longer than 128 bytes, more
    than 16 adapters per mate, adapters2 without adapters, min_overlap or
    max_err_pct given without adapters."""

    def __init__(self, head=None, tail=None, q5=None, q3=None, adapters=None, adapters2=None,
                 min_overlap=3, max_err_pct=10, trim_n=False, max_len=None):
        import operator
        vals = {"head": head, "tail": tail, "q5": q5, "q3": q3, "min_overlap": min_overlap,
                "max_err_pct": max_err_pct, "max_len": max_len}
        for k, v in vals.items():
            if v is None:
                continue
            vals[k] = v = operator.index(v)
            if v < 0:
                raise ValueError(f"Trim: {k} is negative")
            if k in ("q5", "q3") and v > 93:
                raise ValueError(f"Trim: {k} is a cutoff over 93")
        if vals["max_err_pct"] is None or vals["max_err_pct"] > 100:
            raise ValueError("Trim: max_err_pct is a percentage up to 100")
        if vals["min_overlap"] is None or vals["min_overlap"] < 1:
            raise ValueError("Trim: min_overlap is at least 1")
        mates = []
        for what, given in (("adapters", adapters), ("adapters2", adapters2)):
            if isinstance(given, (bytes, bytearray, str)):
                given = [given]
            got = list(_as_bytes(given or (), "adapter"))
            if given is not None and not got:
                raise ValueError(f"Trim: {what} is empty")
            if len(got) > TRIM_ADAPTERS:
                raise ValueError(f"Trim: more than {TRIM_ADAPTERS} {what}")
            for a in got:
                if not 1 <= len(a) <= TRIM_ADAPTER_MAX:
                    raise ValueError(f"Trim: an adapter of {len(a)} bytes (1 to "
                                     f"{TRIM_ADAPTER_MAX})")
            mates.append(got)
        if mates[1] and not mates[0]:
            raise ValueError("Trim: adapters2 without adapters")
        if not mates[0] and (vals["min_overlap"] != 3 or vals["max_err_pct"] != 10):
            raise ValueError("Trim: min_overlap and max_err_pct go with adapters")
        self.head, self.tail, self.q5, self.q3 = vals["head"], vals["tail"], vals["q5"], vals["q3"]
        self.min_overlap, self.max_err_pct = vals["min_overlap"], vals["max_err_pct"]
        self.max_len, self.trim_n = vals["max_len"], bool(trim_n)
        self.adapters, self.adapters2 = mates

    def spec(self):
        """(fqz5_trim_spec, fqz5_trim_adapters) as the library takes them
        (values past a field's range clipped to it: no record is that long)."""
        t, ad = _TrimSpec(), _TrimAdapters()
        u32, u64 = (1 << 32) - 1, (1 << 64) - 1
        if self.head is not None or self.tail is not None:
            t.set |= 1
            t.head, t.tail = min(self.head or 0, u64), min(self.tail or 0, u64)
        if self.q5 is not None:
            t.set |= 2
            t.q5 = self.q5
        if self.q3 is not None:
            t.set |= 4
            t.q3 = self.q3
        if self.adapters:
            t.set |= 8
            t.min_overlap, t.max_err_pct = min(self.min_overlap, u32), self.max_err_pct
            t.n_adapters[0], t.n_adapters[1] = len(self.adapters), len(self.adapters2)
            for j, a in enumerate(self.adapters + self.adapters2):
                ad.len[j] = len(a)
                C.memmove(ad.bytes[j], a, len(a))
        if self.trim_n:
            t.set |= 16
        if self.max_len is not None:
            t.set |= 32
            t.max_len = min(self.max_len, u64)
        return t, ad

    def keys(self) -> tuple:
        """The sections the cut points are judged on (see above)."""
        if self.q5 is not None or self.q3 is not None:
            return (S.SEC_SEQ, S.SEC_QUAL)
        if self.adapters or self.trim_n:
            return (S.SEC_SEQ,)
        return ()


class TrimHits:
    """The result of a trim: `records` (np.uint64) the file record numbers
    selected (all of them without a Filter), ascending; `total` the units seen
    (records, with pairs pairs); `failed` (np.uint64[7]) the units the Filter
    failed, as in FilterHits, judged on the trimmed records; `written` the
    text bytes written; `bases_in`, `bases_out` the bases before and after
    trimming; `trimmed[k]`, `removed[k]` (np.uint64[5]) the records step k of
    STEPS shortened and the bases it took off; `adapter_hits` (np.uint64, one
    per adapter, adapters2's after adapters') the records each adapter cut:
    all counted over every record seen, before any selection.  per_record:
    `starts`, `lengths` (np.uint32) per file record where its kept interval
    starts and how long it is."""
    STEPS = ("clip", "quality", "adapter", "trim_n", "crop")

    def __init__(self, records, total: int, failed, counts, n_adapters: int, written: int = 0,
                 starts=None, lengths=None):
        self.records, self.total, self.failed, self.written = records, total, failed, written
        self.bases_in, self.bases_out = int(counts[0]), int(counts[1])
        self.trimmed, self.removed = counts[2:7].copy(), counts[7:12].copy()
        self.adapter_hits = counts[12:12 + n_adapters].copy()
        self.starts, self.lengths = starts, lengths


def _trim_host(trim: Trim, seq, qual, lens, pairs: bool = False, compact: bool = False):
    """fqz5_trim_host of one block: (starts, new lengths, the counts'
    words[, the compacted bases, the compacted qualities])."""
    so = _load()
    lens = np.ascontiguousarray(lens, np.uint32)
    start, new = np.zeros(len(lens), np.uint32), np.zeros(len(lens), np.uint32)
    counts = np.zeros(12 + 2 * TRIM_ADAPTERS, np.uint64)
    total = int(lens.astype(np.uint64).sum())
    oseq = np.zeros(total + 1, np.uint8) if compact and seq is not None else None
    oqual = np.zeros(total + 1, np.uint8) if compact and qual is not None else None
    t, ad = trim.spec()
    _check(so.fqz5_trim_host(C.byref(t), C.byref(ad), None if seq is None else bytes(seq),
                             None if qual is None else bytes(qual),
                             len(seq) if seq is not None else total, lens.ctypes.data, len(lens),
                             int(pairs), start.ctypes.data, new.ctypes.data, counts.ctypes.data,
                             None if oseq is None else oseq.ctypes.data,
                             None if oqual is None else oqual.ctypes.data), "fqz5_trim_host")
    if not compact:
        return start, new, counts
    kept = int(new.astype(np.uint64).sum())
    return (start, new, counts, None if oseq is None else oseq[:kept].tobytes(),
            None if oqual is None else oqual[:kept].tobytes())


class _TrimBlock:
    """One block's cuts on the device: `start` (tensor), `new` (the new
    lengths, host), and the streams compacted so far (`ptr` by section; the
    tensors in `held` live as long as the block's addresses do)."""

    def __init__(self, start, new):
        self.start, self.new, self.total = start, new, int(new.astype(np.uint64).sum())
        self.ptr, self.held = {}, []

    def gather(self, so, sec, src: int, seq_ulen: int, ln, device) -> None:
        import torch
        dst = torch.empty(self.total + 1, dtype=torch.uint8, device=device)
        got = C.c_uint64(0)
        _check(so.fqz5_trim_gather(src, seq_ulen, ln.ctypes.data, self.start.data_ptr(),
                                   self.new.ctypes.data, len(ln), dst.data_ptr(), self.total,
                                   C.byref(got)), "fqz5_trim_gather")
        self.held.append(dst)
        self.ptr[sec] = dst.data_ptr()


def _trim(rd, trim: Trim, flt, pairs, invert, extract, per_record, plus_name, with_qual, device,
          window_bytes, sink) -> TrimHits:
    """The trim over `rd`; sink(windows of texts) consumes the selected
    records' text (extract) and returns the bytes written."""
    import torch
    if not isinstance(trim, Trim):
        raise TypeError("the steps are a Trim")
    if flt is not None and not isinstance(flt, Filter):
        raise TypeError("the criteria are a Filter")
    so = _load()
    (tspec, tad), fspec = trim.spec(), (flt or Filter()).spec()
    tkeys, fkeys = trim.keys(), (flt.keys() if flt is not None else ())
    keys = max(tkeys, fkeys, key=len)             # (each a prefix of (SEC_SEQ, SEC_QUAL))
    failed, total = np.zeros(7, np.uint64), [0]
    counts = np.zeros(12 + 2 * TRIM_ADAPTERS, np.uint64)
    starts, lengths = [], []

    def match(ptr, v, ln, hits):
        start = torch.empty(max(len(ln), 1), dtype=torch.int32, device=device)
        new = np.zeros(len(ln), np.uint32)
        _check(so.fqz5_trim_cuts(C.byref(tspec), C.byref(tad),
                                 ptr.get(S.SEC_SEQ) if S.SEC_SEQ in tkeys else None,
                                 ptr.get(S.SEC_QUAL) if S.SEC_QUAL in tkeys else None,
                                 v.seq_ulen, ln.ctypes.data, len(ln), int(pairs), start.data_ptr(),
                                 new.ctypes.data, counts.ctypes.data), "fqz5_trim_cuts")
        blk = ptr["trim"] = _TrimBlock(start, new)
        for sec in keys if extract else fkeys:    # (the streams the filter or the text needs)
            blk.gather(so, sec, ptr[sec], v.seq_ulen, ln, device)
        n = C.c_uint64(0)
        _check(so.fqz5_filter_match(C.byref(fspec), blk.ptr.get(S.SEC_SEQ),
                                    blk.ptr.get(S.SEC_QUAL), blk.total, new.ctypes.data, len(ln),
                                    int(pairs), int(invert), hits[0].data_ptr(), C.byref(n),
                                    failed.ctypes.data, None), "fqz5_filter_match")
        total[0] += len(ln) // (2 if pairs else 1)
        if per_record:
            starts.append(start[:len(ln)].cpu().numpy().view(np.uint32))
            lengths.append(new)
        return int(n.value)

    def hook(ptr, v, ln):
        blk = ptr["trim"]
        for sec in (S.SEC_SEQ, S.SEC_QUAL):       # those decoded after the match
            if sec in ptr and sec not in blk.ptr:
                blk.gather(so, sec, ptr[sec], v.seq_ulen, ln, device)
        ptr.update(blk.ptr)
        return blk.new
    recs, _, written = _lookup(rd, keys, ("keys", "trim"), match, pairs, extract, plus_name,
                               with_qual, device, window_bytes, sink, hook)
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.uint32)   # noqa: E731
    return TrimHits(np.asarray(recs, np.uint64), total[0], failed, counts,
                    len(trim.adapters) + len(trim.adapters2), written,
                    cat(starts) if per_record else None, cat(lengths) if per_record else None)


def trim_records(src, trim: Trim, flt: Filter | None = None, pairs: bool = False,
                 per_record: bool = False, device: str = "cuda",
                 window_bytes: int | None = None) -> TrimHits:
    """The cuts `trim` makes in the records of a .fqz5 (a path, the file's
    bytes, or a positioned reader), found on the GPU (see above), and the
    records whose trimmed form passes `flt` (all without one): every block is
    read, checked and CRC-checked; only the sections the steps and the
    criteria need are decoded (none for clip and crop alone) and no name
    section; nothing is written.  pairs: records 2k and 2k + 1 are mates, each
    trimmed on its own (the odd ones with adapters2), kept only when both pass
    `flt`.  A quality cutoff on a block without qualities is an error."""
    return _run(_reader(src), "trim_records", lambda rd: _trim(
        rd, trim, flt, pairs, False, False, per_record, False, True, device, window_bytes, None))


def trim_bytes(data, trim: Trim, flt: Filter | None = None, plus_name: bool = False,
               with_qual: bool = True, device: str = "cuda") -> bytes:
    """The records of a .fqz5 held in memory, trimmed, those that then pass
    `flt`, in file order, as FASTQ text (with_qual False: FASTA text).  A
    Trim() with nothing set and no Filter gives decompress_bytes' text.  See
    trim_records."""
    out = []
    _trim(_PosBytes(data), trim, flt, False, False, True, False, plus_name, with_qual, device, None,
          _bytes_sink(out))
    _trace_dump("trim")
    return b"".join(out)


def trim_file(src: str, dst: str, trim: Trim, flt: Filter | None = None, plus_name: bool = False,
              dst2: str | None = None, with_qual: bool = True, invert: bool = False,
              window_bytes: int | None = None, device: str = "cuda") -> TrimHits:
    """The records of the .fqz5 file src, trimmed, to dst in file order: one
    pass over the file in windows of at most `window_bytes` of compressed
    data, as filter_file makes it, the cut points found and the streams
    compacted on the GPU before the Filter judges them and the text is laid
    out.  flt: only the records whose trimmed form passes are written (invert:
    those that do not).  dst2: the records are interleaved pairs, each mate
    trimmed on its own (the odd ones with adapters2), a pair kept only when
    both trimmed mates pass, R1 records to dst and R2 records to dst2.
    with_qual False: the text is FASTA.  A ".gz" destination is
    gzip-compressed.  One process; returns the TrimHits."""
    outs = [dst] + ([dst2] if dst2 is not None else [])
    return _run((_PosFile(src), True), "trim", lambda rd: _trim(
        rd, trim, flt, dst2 is not None, invert, True, False, plus_name, with_qual, device,
        window_bytes, lambda w: sum(_write_texts(outs, w))))


# ---------------------------------------------------------------------------
# Duplicates
#
# "Drop the reads seen before" (fastp --dedup, seqkit rmdup -s, clumpify
# dedupe): the pass of the filter with the sequence section as the only key,
# and the first record pass whose verdict depends on every earlier record of
# the file.  A unit (a record, with pairs the records 2k and 2k + 1) is kept
# when no earlier unit has the same key; the key is 128 bits summed from the
# unit's bases on the device, so two units are duplicates when their keys are
# equal: equal sequences always, unequal ones with probability about 2^-128 per
# pair (include/fqz5_fastq.h).  A device table with at least twice the file's
# units in slots (the unit count comes from the block index) lives across
# blocks and windows; per block fqz5_dedup_match (dedup.hip) sums the keys,
# inserts them wait-free under the units' file numbers and selects the units
# whose number is their key's smallest.  _key_windows hands blocks over in file
# order, so every earlier unit is in the table when a block is judged and
# "keep the first occurrence" needs no second pass.  No name section is decoded
# before the hits' text is laid out, and no quality section for a block whose
# records are all duplicates.  One process.  Not built: deduplication after a
# Trim or Filter in the same pass, keys that include the qualities or a UMI
# from the name, mismatch-tolerant duplicates, the most duplicated sequences
# themselves, several ranks.
# ---------------------------------------------------------------------------
DEDUP_LEVELS = 1025
DEDUP_TABLE_SHARE = 0.5                         # of the device's free memory: max_table_bytes


class DedupHits:
    """The result of a deduplication: `records` (np.uint64) the file record
    numbers selected, ascending (pairs: both mates); `total` the units seen
    (records, with pairs pairs); `distinct` the different keys among them (the
    units kept without invert); `written` the text bytes written; `first`
    (np.uint64, per_record) for every unit the file record number of the first
    unit with its key (pairs: of that unit's first mate)."""

    def __init__(self, records, total: int, distinct: int, written: int = 0, first=None):
        self.records, self.total, self.distinct = records, total, distinct
        self.written, self.first = written, first


class Duplication:
    """Duplication levels of a whole file, exact (every unit counted, not an
    estimate from the first 100 000 reads as FastQC's): `total` the units,
    `distinct` the different keys, `levels` (np.uint64[1025]) at c the keys
    that c units carry for c < 1024 and at 1024 those that 1024 and more
    carry, `max_count` the most units one key has, `remaining` the share of
    units left after deduplication (distinct / total; 1.0 for no units)."""

    def __init__(self, total: int, distinct: int, levels, max_count: int):
        self.total, self.distinct, self.levels, self.max_count = total, distinct, levels, max_count
        self.remaining = distinct / total if total else 1.0


class _DedupTable(_Native):
    """fqz5_dedup_table for `units` units on the device (freed on exit)."""
    FREE = "fqz5_dedup_table_free"

    def __init__(self, units: int):
        self.so = _load()
        self.p = self.so.fqz5_dedup_table_new(units)
        if not self.p:
            raise _lib.NativeError("fqz5_dedup_table_new: " + _lib.last_error())

    def levels(self) -> np.ndarray:
        out = np.zeros(DEDUP_LEVELS + 2, np.uint64)
        _check(self.so.fqz5_dedup_levels(self.p, out.ctypes.data), "fqz5_dedup_levels")
        return out


class _DedupHostTable(_Native):
    """fqz5_dedup_host_table (freed on exit)."""
    FREE = "fqz5_dedup_host_free"

    def __init__(self):
        self.so = _load()
        self.p = self.so.fqz5_dedup_host_new()
        if not self.p:
            raise _lib.NativeError("fqz5_dedup_host_new: " + _lib.last_error())

    def levels(self) -> np.ndarray:
        out = np.zeros(DEDUP_LEVELS + 2, np.uint64)
        _check(self.so.fqz5_dedup_host_levels(self.p, out.ctypes.data), "fqz5_dedup_host_levels")
        return out


def _dedup_host(seq, lens, pairs: bool = False, revcomp: bool = False, invert: bool = False,
                table: _DedupHostTable | None = None, first_unit: int = 0):
    """fqz5_dedup_keys_host of one block and fqz5_dedup_host_add of its keys
    as the units first_unit .. into `table` (None: a table of its own): (the
    keys, np.uint64[units, 2]; keep per unit; per unit the first unit with its
    key)."""
    import contextlib
    so = _load()
    lens = np.ascontiguousarray(lens, np.uint32)
    seq = bytes(seq)
    units = len(lens) // (2 if pairs else 1)
    keys = np.zeros((units, 2), np.uint64)
    _check(so.fqz5_dedup_keys_host(seq, len(seq), lens.ctypes.data, len(lens), int(pairs),
                                   int(revcomp), keys.ctypes.data), "fqz5_dedup_keys_host")
    keep, first = np.zeros(units, np.uint8), np.zeros(units, np.uint64)
    with (_DedupHostTable() if table is None else contextlib.nullcontext(table)) as t:
        _check(so.fqz5_dedup_host_add(t.p, keys.ctypes.data, units, first_unit, int(invert),
                                      keep.ctypes.data, first.ctypes.data), "fqz5_dedup_host_add")
    return keys, keep, first


def _dedup(rd, pairs, revcomp, invert, extract, per_record, plus_name, with_qual, device,
           window_bytes, sink, max_table_bytes=None, levels: bool = False):
    """The deduplication over `rd`; sink(windows of texts) consumes the
    selected records' text (extract) and returns the bytes written.  Returns
    the DedupHits, with `levels` (the pass over the table after the last
    block) the pair (DedupHits, fqz5_dedup_levels' words)."""
    import torch
    so = _load()
    mates = 2 if pairs else 1
    with _stage("index"):
        units = sum(int(n) // mates for _, _, n in read_index(rd))
    need = int(so.fqz5_dedup_table_bytes(units))
    if max_table_bytes is None:
        max_table_bytes = int(DEDUP_TABLE_SHARE * torch.cuda.mem_get_info(device)[0])
    if not need or need > max_table_bytes:
        raise _lib.NativeError(f"dedup: a table of {need or 'more than 2^36'} bytes for {units} "
                               f"units exceeds max_table_bytes = {max_table_bytes}")
    with _stage("table"):
        tab = _DedupTable(units)
    with tab:
        unit0, first = [0], []

        def match(ptr, v, ln, hits):
            n, k = C.c_uint64(0), len(ln) // mates
            d_first = torch.empty(max(k, 1), dtype=torch.int64, device=device) if per_record else None
            _lib.after_torch(device)
            _check(so.fqz5_dedup_match(tab.p, ptr[S.SEC_SEQ], v.seq_ulen, ln.ctypes.data, len(ln),
                                       int(pairs), int(revcomp), int(invert), unit0[0],
                                       hits[0].data_ptr(), C.byref(n),
                                       d_first.data_ptr() if per_record else None),
                   "fqz5_dedup_match")
            unit0[0] += k
            if per_record:
                first.append(d_first[:k].cpu().numpy().view(np.uint64) * np.uint64(mates))
            return int(n.value)
        recs, _, written = _lookup(rd, (S.SEC_SEQ,), ("keys", "dedup"), match, pairs, extract,
                                   plus_name, with_qual, device, window_bytes, sink)
        total, picked = unit0[0], len(recs) // mates
        hits = DedupHits(np.asarray(recs, np.uint64), total, total - picked if invert else picked,
                         written, (np.concatenate(first) if first else np.zeros(0, np.uint64))
                         if per_record else None)
        if not levels:
            return hits
        with _stage("levels"):
            return hits, tab.levels()


def dedup_records(src, pairs: bool = False, revcomp: bool = False, invert: bool = False,
                  per_record: bool = False, device: str = "cuda",
                  window_bytes: int | None = None, max_table_bytes: int | None = None) -> DedupHits:
    """The records of a .fqz5 (a path, the file's bytes, or a positioned
    reader) that are the first of their sequence in the file, judged on the
    GPU (see above): every block is read, checked and CRC-checked, its
    sequence section alone decoded.  Two units are duplicates when their
    128-bit keys are equal: equal sequences always (bytes as they are, no case
    folding), unequal ones with probability about 2^-128 per pair.  pairs:
    records 2k and 2k + 1 are one unit, a duplicate when both mates are (a
    block with an odd record count is an error).  revcomp: a sequence and its
    reverse complement are the same; with pairs, a pair and the pair with its
    mates swapped (no base is complemented).  invert: exactly the units that
    are not the first.  per_record: `first` per unit.  max_table_bytes: the
    most device memory the table may take (default: half of what is free); a
    table beyond it is an error that names the size."""
    return _run(_reader(src), "dedup_records", lambda rd: _dedup(
        rd, pairs, revcomp, invert, False, per_record, False, True, device, window_bytes, None,
        max_table_bytes))


def dedup_bytes(data, revcomp: bool = False, invert: bool = False, plus_name: bool = False,
                with_qual: bool = True, device: str = "cuda", window_bytes: int | None = None,
                max_table_bytes: int | None = None) -> bytes:
    """The records of a .fqz5 held in memory that are the first of their
    sequence, in file order, as the text decompress_bytes gives for them
    (with_qual False: FASTA text).  See dedup_records."""
    out = []
    _dedup(_PosBytes(data), False, revcomp, invert, True, False, plus_name, with_qual, device,
           window_bytes, _bytes_sink(out), max_table_bytes)
    _trace_dump("dedup")
    return b"".join(out)


def dedup_file(src: str, dst: str, dst2: str | None = None, with_qual: bool = True,
               plus_name: bool = False, revcomp: bool = False, invert: bool = False,
               device: str = "cuda", window_bytes: int | None = None,
               max_table_bytes: int | None = None) -> DedupHits:
    """The records of the .fqz5 file src that are the first of their sequence
    to dst, in file order: one pass over the file in windows of at most
    `window_bytes` of compressed data; every block is read once, checked
    against its index entry and CRC-checked, its sequence section decoded and
    judged on the GPU against a table of every earlier unit; the name and
    quality sections are decoded for the blocks with selected records only,
    and their text is laid out on the GPU (fqz5_fastq_format_list).  dst2: the
    records are interleaved pairs, a pair is one unit, R1 records to dst and R2
    records to dst2.  with_qual False: the text is FASTA and no quality
    section is decoded.  invert: the duplicates instead.  A ".gz" destination
    is gzip-compressed.  One process; returns the DedupHits (`written`: the
    text bytes written).  See dedup_records."""
    outs = [dst] + ([dst2] if dst2 is not None else [])
    return _run((_PosFile(src), True), "dedup", lambda rd: _dedup(
        rd, dst2 is not None, revcomp, invert, True, False, plus_name, with_qual, device,
        window_bytes, lambda w: sum(_write_texts(outs, w)), max_table_bytes))


def duplication(src, pairs: bool = False, revcomp: bool = False, device: str = "cuda",
                window_bytes: int | None = None,
                max_table_bytes: int | None = None) -> Duplication:
    """The duplication levels of a .fqz5 (a path, the file's bytes, or a
    positioned reader): the pass of dedup_records with nothing extracted, then
    one pass over the table on the GPU.  Exact over the whole file, every unit
    counted: not FastQC's estimate from the first 100 000 reads.  See
    Duplication and dedup_records."""
    def run(rd):
        h, lv = _dedup(rd, pairs, revcomp, False, False, False, False, True, device, window_bytes,
                       None, max_table_bytes, levels=True)
        return Duplication(h.total, int(lv[DEDUP_LEVELS]), lv[:DEDUP_LEVELS].copy(),
                           int(lv[DEDUP_LEVELS + 1]))
    return _run(_reader(src), "duplication", run)
