#!/usr/bin/env python3
"""The filter by read metrics against a whole-file decode and against the
statistics ("Filter by read metrics"): the input of
tools/stats_bench.py (the benchmark's -3 Illumina text at a tenth of its size
in ten 10 MB blocks), compressed once; then

  (a) decompress_file of the whole file (what a user does today before
      filtering elsewhere),
  (b) stats of it (the same decode without selection),
  (c) filter_records with a quality and an N criterion,
  (d) filter_file keeping roughly half the reads (min_mean_q at the median of
      the reads' mean quality),
  (e) filter_records with min_len alone,

each the median of 5 runs after one warmup, with the $FQZ5_FILE_TRACE stages
(median per stage).  The selections of (c), (d) and (e), the reason counts and
the text (d) writes are checked against numpy on the input text.  --kind ont
takes synth.ont reads instead, --level another level.  Not part of bench.py.

    python tools/filter_bench.py [--out profiles/filter_l3.json]
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


def numpy_sums(lines) -> dict:
    """Per record its length, N count and quality sum, over the whole text at
    once."""
    seq = np.frombuffer(b"".join(lines[1::4]), np.uint8)
    qual = np.frombuffer(b"".join(lines[3::4]), np.uint8) - np.uint8(33)
    lens = np.asarray([len(s) for s in lines[1::4]], np.int64)
    assert lens.min() > 0
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    return {"len": lens, "n": np.add.reduceat(((seq | 0x20) == ord("n")).astype(np.int64), start),
            "qsum": np.add.reduceat(qual.astype(np.int64), start)}


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
        exp = numpy_sums(lines)
        nrec = len(exp["len"])
        # (c): a quality and an N criterion; (d): the median mean quality, about half the reads
        q_c = int(np.percentile(exp["qsum"] // exp["len"], 20))
        q_d = int(np.median(-(-exp["qsum"] // exp["len"])))
        n_c = 0 if (exp["n"] > 0).any() else 1
        l_e = int(exp["len"].min())
        f_c = Z.Filter(min_mean_q=q_c, max_n=n_c)
        f_d = Z.Filter(min_mean_q=q_d)
        f_e = Z.Filter(min_len=l_e)
        fail_n = exp["n"] > n_c
        fail_q = ~fail_n & (exp["qsum"] < q_c * exp["len"])
        keep_c = np.flatnonzero(~fail_n & ~fail_q)
        keep_d = np.flatnonzero(exp["qsum"] >= q_d * exp["len"])

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
        st, st_st = timed(lambda: Z.stats(fqz))
        c, c_st = timed(lambda: got.append(Z.filter_records(fqz, f_c)))
        h = got[-1]
        assert (h.records == keep_c.astype(np.uint64)).all() and h.total == nrec
        assert h.failed.tolist() == [0, 0, int(fail_n.sum()), int(fail_q.sum()), 0, 0, 0]
        dd, d_st = timed(lambda: got.append(Z.filter_file(fqz, out, f_d)))
        h = got[-1]
        assert (h.records == keep_d.astype(np.uint64)).all()
        want = b"".join(x + b"\n" for r in keep_d.tolist() for x in lines[4 * r:4 * r + 4])
        with open(out, "rb") as f:
            assert f.read() == want and h.written == len(want)
        kept_d, written_d = len(keep_d), len(want)
        del want, lines
        e, e_st = timed(lambda: got.append(Z.filter_records(fqz, f_e)))
        h = got[-1]
        assert len(h.records) == nrec and not h.failed.any() and int(h.records[-1]) == nrec - 1

    def stage_ms(runs):
        keys = list(runs[0])
        return {k: round(1e3 * med([r.get(k, 0.0) for r in runs]), 3) for k in keys}

    def case(ts, sts, **more):
        return dict(more, median_s=round(med(ts), 5), runs=[round(x, 5) for x in ts],
                    stages_ms=stage_ms(sts))

    bases = int(exp["len"].sum())
    ms_b, ms_c = stage_ms(st_st), stage_ms(c_st)
    res = {
        "tool": "tools/filter_bench.py",
        "input": f"synth.{args.kind} seed 1, {text_bytes} bytes of FASTQ, -{args.level}, "
                 f"blk_size {args.blk}",
        "text_bytes": text_bytes, "fqz5_bytes": size, "blocks": len(index), "records": nrec,
        "base_bytes": bases,
        "a_decompress_file": case(whole, whole_st),
        "b_stats": case(st, st_st),
        "c_filter_records_quality_and_n": case(c, c_st, criteria=f"min_mean_q={q_c}, max_n={n_c}",
                                               kept=len(keep_c)),
        "d_filter_file_half": case(dd, d_st, criteria=f"min_mean_q={q_d}", kept=kept_d,
                                   written=written_d),
        "e_filter_records_min_len": case(e, e_st, criteria=f"min_len={l_e}", kept=nrec),
        "filter_stage": {"ms_per_call": ms_c["filter"],
                         "ms_per_block": round(ms_c["filter"] / len(index), 3),
                         "stats_stage_ms": ms_b["stats"],
                         "filter_over_stats": round(ms_c["filter"] / ms_b["stats"], 3),
                         "base_and_quality_bytes_per_s": round(2 * bases / (ms_c["filter"] / 1e3)),
                         "note": "host wall time of fqz5_filter_match per block (the record ends' "
                                 "and the tiles' first records' upload, the sums and pick kernels, "
                                 "the compaction and its synchronisation) and the download of the "
                                 "selected indices"},
        "checked": "the records and reason counts of (c), (d) and (e) and the text (d) writes "
                   "equal numpy's on the input text",
        "ratio_a_over_c": round(med(whole) / med(c), 2),
        "ratio_a_over_d": round(med(whole) / med(dd), 2),
        "ratio_b_over_c": round(med(st) / med(c), 2),
        "ratio_a_over_e": round(med(whole) / med(e), 2),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
