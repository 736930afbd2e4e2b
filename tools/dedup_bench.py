#!/usr/bin/env python3
"""The deduplication against a whole-file decode and against the filter
("Duplicates"): the input of tools/filter_bench.py (the
benchmark's -3 Illumina text at a tenth of its size in ten 10 MB blocks),
compressed once; then

  (a) decompress_file of the whole file (what a user does today before
      deduplicating elsewhere),
  (b) filter_records with one base criterion (max_n): the same pass, the same
      key section and the same tile walk without keys or table; the filter's
      code is the parent commit's, so this is the yardstick,
  (c) dedup_records,
  (d) dedup_file on a second input with about half its reads duplicated (every
      odd record takes the bases and qualities of an earlier even one),
  (e) duplication,

each the median of 5 runs after one warmup, with the $FQZ5_FILE_TRACE stages
(median per stage).  The selections of (c) and (d), the levels of (e) and the
text (d) writes are checked against an exact deduplication by a Python dict on
the sequence lines of the decompressed text; "dedup_file_exact" in the result
says whether (d)'s text was exactly the kept records'.

The kernels on their own, through the library's seams on device arrays, host
wall time of the synchronous call (median of 5): fqz5_dedup_keys over all the
file's bases as one block beside fqz5_filter_match with max_n over the same
arrays (its sums kernel, pick and compaction), and fqz5_dedup_insert_keys of
4 Mi random keys into an empty table of 8 Mi slots.  Not part of bench.py.

    python tools/dedup_bench.py [--out profiles/dedup_l3.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FASTQ_REC = 358            # bench.py's bytes of text per synthetic 150 bp record
RUNS = 5
INSERT_KEYS = 1 << 22


def exact(seq_lines):
    """(kept record numbers, count per distinct sequence) by a dict."""
    first, kept = {}, []
    for r, s in enumerate(seq_lines):
        if s not in first:
            first[s] = 0
            kept.append(r)
        first[s] += 1
    return kept, list(first.values())


def levels_of(counts):
    out = np.zeros(1025, np.uint64)
    for c in counts:
        out[min(c, 1024)] += 1
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=0.1)
    ap.add_argument("--blk", type=int, default=10_000_000)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()

    import torch
    from fqzcomp5_amd import fqz5file as Z
    from fqzcomp5_amd import lib, synth
    stages = []

    def grab(what):                       # the stages of each call, instead of stderr
        stages.append(dict(Z._TRACE))
        Z._TRACE.clear()
    Z._trace_dump = grab
    med = statistics.median

    def timed(fn):
        fn()                                                # warmup
        del stages[:]
        ts = []
        for _ in range(RUNS):
            t = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t)
        return ts, [dict(s) for s in stages]

    with tempfile.TemporaryDirectory() as d:
        src, fqz, half, hfqz, out = (os.path.join(d, n) for n in (
            "in.fastq", "in.fqz5", "half.fastq", "half.fqz5", "out.fastq"))
        reads = synth.illumina(int(args.gb * 1e9 / FASTQ_REC), seed=1)
        text_bytes = synth.write_fastq(reads, src)
        size = Z.compress_file(src, fqz, args.level, blk_size=args.blk)
        index = Z.read_index(fqz)
        with open(src, "rb") as f:
            lines = f.read().split(b"\n")[:-1]
        nrec = len(lines) // 4
        rng = np.random.default_rng(1)
        hl = list(lines)
        for r in range(1, nrec, 2):                         # every odd record: an earlier even one's
            j = 2 * int(rng.integers(0, (r + 1) // 2))
            hl[4 * r + 1], hl[4 * r + 3] = hl[4 * j + 1], hl[4 * j + 3]
        with open(half, "wb") as f:
            f.write(b"".join(x + b"\n" for x in hl))
        del hl
        hsize = Z.compress_file(half, hfqz, args.level, blk_size=args.blk)

        whole, whole_st = timed(lambda: Z.decompress_file(fqz, out))
        assert os.path.getsize(out) == text_bytes
        with open(out, "rb") as f:
            seq_lines = f.read().split(b"\n")[1::4]
        keep_c, counts_c = exact(seq_lines)
        bases = sum(len(s) for s in seq_lines)
        got = []
        b, b_st = timed(lambda: got.append(Z.filter_records(fqz, Z.Filter(max_n=150))))
        c, c_st = timed(lambda: got.append(Z.dedup_records(fqz)))
        h = got[-1]
        ok_c = (h.records.tolist() == keep_c and h.total == nrec and h.distinct == len(counts_c))
        e, e_st = timed(lambda: got.append(Z.duplication(fqz)))
        du = got[-1]
        ok_e = ((du.levels == levels_of(counts_c)).all() and du.distinct == len(counts_c)
                and du.max_count == max(counts_c))

        Z.decompress_file(hfqz, out)
        del stages[:]
        with open(out, "rb") as f:
            hlines = f.read().split(b"\n")[:-1]
        keep_d, counts_d = exact(hlines[1::4])
        want = b"".join(x + b"\n" for r in keep_d for x in hlines[4 * r:4 * r + 4])
        del hlines
        dd, d_st = timed(lambda: got.append(Z.dedup_file(hfqz, out)))
        h = got[-1]
        with open(out, "rb") as f:
            ok_d = (f.read() == want and h.written == len(want) and h.records.tolist() == keep_d)
        kept_d, written_d = len(keep_d), len(want)
        del want

        # the kernels on their own, through the seams, on device arrays
        so = Z._load()
        seq_d = torch.frombuffer(bytearray(b"".join(seq_lines)), dtype=torch.uint8).cuda()
        lens = np.asarray([len(s) for s in seq_lines], np.uint32)
        keys_d = torch.empty(2 * nrec, dtype=torch.int64, device="cuda")
        rec_d = torch.empty(nrec, dtype=torch.int32, device="cuda")
        spec, failed, nhit = Z.Filter(max_n=150).spec(), np.zeros(7, np.uint64), C.c_uint64(0)
        lib.after_torch()

        def call(fn, *a):
            def run():
                assert fn(*a) == 0, lib.last_error()
            return med(timed(run)[0])
        t_keys = {}
        for name, pairs, rc in (("plain", 0, 0), ("revcomp", 0, 1), ("pairs", 1, 0),
                                ("pairs_revcomp", 1, 1)):
            n = nrec - (nrec & 1 if pairs else 0)
            t_keys[name] = call(so.fqz5_dedup_keys, seq_d.data_ptr(), int(lens[:n].sum()),
                                lens.ctypes.data, n, pairs, rc, keys_d.data_ptr())
        t_sums = call(so.fqz5_filter_match, C.byref(spec), seq_d.data_ptr(), None, bases,
                      lens.ctypes.data, nrec, 0, 0, rec_d.data_ptr(), C.byref(nhit),
                      failed.ctypes.data, None)
        rk = torch.from_numpy(rng.integers(0, 1 << 63, 2 * INSERT_KEYS, dtype=np.int64)).cuda()
        slot_d = torch.empty(INSERT_KEYS, dtype=torch.int32, device="cuda")
        lib.after_torch()
        with Z._DedupTable(INSERT_KEYS) as tab:
            def insert():
                assert so.fqz5_dedup_table_reset(tab.p) == 0
                t = time.perf_counter()
                assert so.fqz5_dedup_insert_keys(tab.p, rk.data_ptr(), INSERT_KEYS, 0,
                                                 slot_d.data_ptr()) == 0, lib.last_error()
                return time.perf_counter() - t
            insert()
            t_ins = med([insert() for _ in range(RUNS)])
            t_again = []                                    # the same keys again: every one a duplicate
            for _ in range(RUNS):
                t = time.perf_counter()
                assert so.fqz5_dedup_insert_keys(tab.p, rk.data_ptr(), INSERT_KEYS, INSERT_KEYS,
                                                 slot_d.data_ptr()) == 0
                t_again.append(time.perf_counter() - t)
            lv = np.zeros(Z.DEDUP_LEVELS + 2, np.uint64)    # (held: the calls write into it)
            t_lv = call(so.fqz5_dedup_levels, tab.p, lv.ctypes.data)
            assert int(lv[Z.DEDUP_LEVELS]) == INSERT_KEYS and int(lv[RUNS + 1]) == INSERT_KEYS
        del stages[:]

    def stage_ms(runs):
        keys = list(runs[0])
        return {k: round(1e3 * med([r.get(k, 0.0) for r in runs]), 3) for k in keys}

    def case(ts, sts, **more):
        return dict(more, median_s=round(med(ts), 5), runs=[round(x, 5) for x in ts],
                    stages_ms=stage_ms(sts))

    ms_b, ms_c = stage_ms(b_st), stage_ms(c_st)
    res = {
        "tool": "tools/dedup_bench.py",
        "input": f"synth.illumina seed 1, {text_bytes} bytes of FASTQ, -{args.level}, "
                 f"blk_size {args.blk}",
        "text_bytes": text_bytes, "fqz5_bytes": size, "blocks": len(index), "records": nrec,
        "base_bytes": bases,
        "a_decompress_file": case(whole, whole_st),
        "b_filter_records_max_n": case(b, b_st, criteria="max_n=150"),
        "c_dedup_records": case(c, c_st, kept=len(keep_c), distinct=len(counts_c)),
        "d_dedup_file_half": case(dd, d_st, fqz5_bytes=hsize, kept=kept_d, written=written_d),
        "e_duplication": case(e, e_st, distinct=du.distinct, max_count=du.max_count),
        "dedup_records_exact": bool(ok_c),
        "dedup_file_exact": bool(ok_d),
        "dedup_file_records": {"in": nrec, "kept_by_dedup_file": int(len(h.records)),
                               "kept_by_exact_host_dedup": kept_d},
        "duplication_exact": bool(ok_e),
        "dedup_stage": {"ms_per_call": ms_c["dedup"],
                        "ms_per_block": round(ms_c["dedup"] / len(index), 3),
                        "filter_stage_ms_per_call": ms_b["filter"],
                        "filter_stage_ms_per_block": round(ms_b["filter"] / len(index), 3),
                        "dedup_over_filter": round(ms_c["dedup"] / ms_b["filter"], 3),
                        "keys_stage_ms": ms_c["keys"],
                        "note": "host wall time of fqz5_dedup_match per block (the record ends' "
                                "and the tiles' first records' upload, the key, fold, insert and "
                                "pick kernels, the compaction and its synchronisation) and the "
                                "download of the selected indices; keys_stage_ms: the window's "
                                "blocks parsed, CRC-checked and their sequence sections decoded"},
        "kernels": {"note": "host wall time of one synchronous call on device arrays, median of 5; "
                            "each holds its uploads, launches and the final synchronisation",
                    "dedup_keys_s": {k: round(v, 6) for k, v in t_keys.items()},
                    "dedup_keys_bases_per_s": {k: round(bases / v) for k, v in t_keys.items()},
                    "filter_match_max_n_s": round(t_sums, 6),
                    "filter_match_max_n_bases_per_s": round(bases / t_sums),
                    "insert_keys": INSERT_KEYS, "insert_slots": 2 * INSERT_KEYS,
                    "insert_distinct_s": round(t_ins, 6),
                    "insert_distinct_units_per_s": round(INSERT_KEYS / t_ins),
                    "insert_duplicates_s": round(med(t_again), 6),
                    "insert_duplicates_units_per_s": round(INSERT_KEYS / med(t_again)),
                    "levels_s": round(t_lv, 6),
                    "levels_slots_per_s": round(2 * INSERT_KEYS / t_lv)},
        "ratio_a_over_c": round(med(whole) / med(c), 2),
        "ratio_c_over_b": round(med(c) / med(b), 2),
        "ratio_a_over_d": round(med(whole) / med(dd), 2),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
