#!/usr/bin/env python3
"""Lookup by sequence content against a whole-file decode (DESIGN.md section
4, "Lookup by sequence"): the input of tools/names_bench.py (the benchmark's
-3 Illumina text at a tenth of its size in ten 10 MB blocks), compressed
once; then, with 16 patterns of 20 bases drawn from reads of block 5 plus 16
that occur nowhere, revcomp=True,

  (a) decompress_file of the whole file,
  (b) find_seqs of the 32 patterns,
  (c) extract_seqs_file of the 32 patterns,
  (d) find_seqs of 10 000 patterns of 31 bases (half of them drawn from
      reads all over the file, half random), revcomp=True,

each the median of 5 runs after one warmup, with the $FQZ5_FILE_TRACE stages
(median per stage), the match stage per block and the base bytes per second
it implies.  Not part of bench.py.

    python tools/seqs_bench.py [--out profiles/extract_seqs_l3.json]
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FASTQ_REC = 358            # bench.py's bytes of text per synthetic 150 bp record
RUNS = 5
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=0.1)
    ap.add_argument("--blk", type=int, default=10_000_000)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--many", type=int, default=10_000)
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
        text_bytes = synth.write_fastq(synth.illumina(int(args.gb * 1e9 / FASTQ_REC), seed=1), src)
        size = Z.compress_file(src, fqz, args.level, blk_size=args.blk)
        index = Z.read_index(fqz)
        with open(src, "rb") as f:
            lines = f.read().split(b"\n")[:-1]
        seqs = lines[1::4]
        base_bytes = sum(len(s) for s in seqs)
        first = [0]
        for _, _, n in index:
            first.append(first[-1] + n)
        rng = random.Random(1)
        mid = len(index) // 2

        def piece(r, n):
            at = rng.randint(0, len(seqs[r]) - n)
            return seqs[r][at:at + n]

        def absent(n):
            return bytes(rng.choice(b"ACGT") for _ in range(n))
        from_mid = sorted(rng.sample(range(first[mid], first[mid + 1]), 16))
        few = [piece(r, 20) for r in from_mid] + [absent(20) for _ in range(16)]
        assert len(set(few)) == 32
        from_all = sorted(rng.sample(range(len(seqs)), args.many // 2))
        many = list(dict.fromkeys([piece(r, 31) for r in from_all] +
                                  [absent(31) for _ in range(args.many - args.many // 2)]))

        def want(pats):                   # the records that hold one, on either strand
            both = pats + [p.translate(COMP)[::-1] for p in pats]
            return [r for r, s in enumerate(seqs) if any(p in s for p in both)]

        def text_of(recs):
            return b"".join(x + b"\n" for r in recs for x in lines[4 * r:4 * r + 4])

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
        hits = []
        find, find_st = timed(lambda: hits.append(Z.find_seqs(fqz, few, revcomp=True)))
        rec_few = want(few)
        assert hits[-1].records.tolist() == rec_few and set(from_mid) <= set(rec_few)
        assert len(hits[-1].missing) >= 14 and not set(hits[-1].missing) & set(few[:16])
        ext, ext_st = timed(lambda: Z.extract_seqs_file(fqz, out, few, revcomp=True))
        assert open(out, "rb").read() == text_of(rec_few), "extracted text differs from the input"
        big, big_st = timed(lambda: hits.append(Z.find_seqs(fqz, many, revcomp=True)))
        rec_many = set(hits[-1].records.tolist())            # (checked by the drawn reads alone)
        assert set(from_all) <= rec_many and not set(hits[-1].missing) & set(many[:len(from_all)])
        blocks_few = sorted({sum(r >= f for f in first[1:]) for r in rec_few})

    def stage_ms(runs):
        keys = list(runs[0])
        return {k: round(1e3 * med([r.get(k, 0.0) for r in runs]), 3) for k in keys}

    def case(ts, st):
        return {"median_s": round(med(ts), 5), "runs": [round(x, 5) for x in ts],
                "stages_ms": stage_ms(st)}

    def match_of(st, queries):
        ms = stage_ms(st)["match"]
        return {"queries": queries, "ms_per_call": ms, "ms_per_block": round(ms / len(index), 3),
                "base_bytes_per_s": round(base_bytes / (ms / 1e3))}

    res = {
        "tool": "tools/seqs_bench.py",
        "input": f"synth.illumina seed 1, {text_bytes} bytes of FASTQ, -{args.level}, "
                 f"blk_size {args.blk}",
        "text_bytes": text_bytes, "fqz5_bytes": size, "blocks": len(index),
        "records": len(seqs), "base_bytes": base_bytes,
        "a_decompress_file": case(whole, whole_st),
        "b_find_seqs_32": dict(case(find, find_st), records=len(rec_few)),
        "c_extract_seqs_32": dict(case(ext, ext_st), records=len(rec_few),
                                  blocks_with_hits=blocks_few),
        "d_find_seqs_many": dict(case(big, big_st), patterns=len(many), records=len(rec_many)),
        "match_stage": {"b": match_of(find_st, len(Z._seq_queries(few, True)[1])),
                        "d": match_of(big_st, len(Z._seq_queries(many, True)[1])),
                        "note": "host wall time of fqz5_seqs_match per block (the record ends' "
                                "upload, k_seq_match, compaction, the count's download) and the "
                                "download of the compacted hits"},
        "ratio_a_over_b": round(med(whole) / med(find), 2),
        "ratio_a_over_c": round(med(whole) / med(ext), 2),
        "ratio_a_over_d": round(med(whole) / med(big), 2),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
