#!/usr/bin/env python3
"""File statistics against a whole-file decode ("File
statistics"): the input of tools/seqs_bench.py (the benchmark's -3 Illumina
text at a tenth of its size in ten 10 MB blocks), compressed once; then

  (a) decompress_file of the whole file,
  (b) stats of it (cycles 1024),
  (c) stats with per_record=True,

each the median of 5 runs after one warmup, with the $FQZ5_FILE_TRACE stages
(median per stage) and the base bytes per second the stats stage implies.
The result of (c) is checked against numpy on the input text.  --kind ont
takes synth.ont reads instead, --level another level.  Not part of bench.py.

    python tools/stats_bench.py [--out profiles/stats_l3.json]
"""
from __future__ import annotations

import argparse
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
ONT_REC = 29_000           # about the text of one synth.ont read
RUNS = 5


def numpy_tables(lines, cycles: int) -> dict:
    """The definitions over the whole text at once (one mate)."""
    seq = np.frombuffer(b"".join(lines[1::4]), np.uint8)
    qual = np.frombuffer(b"".join(lines[3::4]), np.uint8) - np.uint8(33)
    lens = np.asarray([len(s) for s in lines[1::4]], np.int64)
    assert lens.min() > 0
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    c = int(min(cycles, lens.max()))
    pos = np.arange(len(seq)) - np.repeat(start, lens)
    low = pos < c
    cls = np.full(256, 5, np.int64)
    for k, b in enumerate(b"ACGTN"):
        cls[b] = cls[b | 0x20] = k
    gc = np.zeros(256, np.int64)
    gc[list(b"GCgc")] = 1
    rgc = np.add.reduceat(gc[seq], start)
    rqs = np.add.reduceat(qual.astype(np.int64), start)
    return {"records": len(lens), "bases": int(lens.sum()), "cycles": c,
            "base_counts": np.bincount(seq, minlength=256),
            "qual_counts": np.bincount(qual, minlength=256),
            "cycle_base": np.bincount(pos[low] * 6 + cls[seq[low]], minlength=6 * c).reshape(c, 6),
            "cycle_qual": np.bincount(pos[low] * 256 + qual[low], minlength=256 * c).reshape(c, 256),
            "read_gc": np.bincount(100 * rgc // lens, minlength=101),
            "read_qual": np.bincount(rqs // lens, minlength=256),
            "record_len": lens, "record_gc": rgc, "record_qsum": rqs}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=0.1)
    ap.add_argument("--blk", type=int, default=10_000_000)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--kind", choices=("illumina", "ont"), default="illumina")
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()

    from fqzcomp5_amd import fqz5file as Z
    from fqzcomp5_amd import synth
    stages = []

    def grab(what):                       # the stages of each call, instead of stderr
        stages.append(dict(Z._TRACE))
        Z._TRACE.clear()
    Z._trace_dump = grab

    med = statistics.median
    with tempfile.TemporaryDirectory() as d:
        src, fqz, out = (os.path.join(d, n) for n in ("in.fastq", "in.fqz5", "out.fastq"))
        if args.kind == "illumina":
            reads = synth.illumina(int(args.gb * 1e9 / FASTQ_REC), seed=1)
        else:
            reads = synth.ont(int(args.gb * 1e9 / ONT_REC), seed=1, with_names=True)
        text_bytes = synth.write_fastq(reads, src)
        size = Z.compress_file(src, fqz, args.level, blk_size=args.blk)
        index = Z.read_index(fqz)
        with open(src, "rb") as f:
            lines = f.read().split(b"\n")[:-1]
        exp = numpy_tables(lines, 1024)
        del lines

        def timed(fn):
            fn()                                            # warmup
            del stages[:]
            ts = []
            for _ in range(RUNS):
                t = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t)
            return ts, [dict(s) for s in stages]

        whole, whole_st = timed(lambda: Z.decompress_file(fqz, out))
        assert os.path.getsize(out) == text_bytes
        got = []
        plain, plain_st = timed(lambda: got.append(Z.stats(fqz)))
        per, per_st = timed(lambda: got.append(Z.stats(fqz, per_record=True)))
        for st in (got[0], got[-1]):
            assert int(st.records[0]) == exp["records"] == int(st.qual_records[0])
            assert int(st.bases[0]) == exp["bases"] and st.cycles == exp["cycles"]
            for k in ("base_counts", "qual_counts", "cycle_base", "cycle_qual", "read_gc",
                      "read_qual"):
                assert (getattr(st, k)[0] == exp[k]).all(), f"{k} differs from numpy on the text"
        for k in ("record_len", "record_gc", "record_qsum"):
            assert (getattr(got[-1], k) == exp[k]).all(), f"{k} differs from numpy on the text"
        n50 = got[0].nx(50)

    def stage_ms(runs):
        keys = list(runs[0])
        return {k: round(1e3 * med([r.get(k, 0.0) for r in runs]), 3) for k in keys}

    def case(ts, st):
        return {"median_s": round(med(ts), 5), "runs": [round(x, 5) for x in ts],
                "stages_ms": stage_ms(st)}

    ms = stage_ms(plain_st)
    res = {
        "tool": "tools/stats_bench.py",
        "input": f"synth.{args.kind} seed 1, {text_bytes} bytes of FASTQ, -{args.level}, "
                 f"blk_size {args.blk}",
        "text_bytes": text_bytes, "fqz5_bytes": size, "blocks": len(index),
        "records": exp["records"], "base_bytes": exp["bases"], "cycles": exp["cycles"], "n50": n50,
        "a_decompress_file": case(whole, whole_st),
        "b_stats": case(plain, plain_st),
        "c_stats_per_record": case(per, per_st),
        "stats_stage": {"ms_per_call": ms["stats"], "ms_per_block": round(ms["stats"] / len(index), 3),
                        "decode_ms": ms["decode"],
                        "stats_over_decode": round(ms["stats"] / ms["decode"], 3),
                        "base_and_quality_bytes_per_s": round(2 * exp["bases"] / (ms["stats"] / 1e3)),
                        "note": "host wall time of fqz5_stats_add per block (the record ends' and "
                                "the tiles' first records' upload, the three kernels, the "
                                "synchronisation) and the host's merge of the length counts"},
        "checked": "every table of (b) and (c) and the per-record arrays of (c) equal numpy's on "
                   "the input text",
        "ratio_a_over_b": round(med(whole) / med(plain), 2),
        "ratio_a_over_c": round(med(whole) / med(per), 2),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
