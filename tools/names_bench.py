#!/usr/bin/env python3
"""Lookup by read name against a whole-file decode (DESIGN.md section 4,
"Lookup by read name"): the input of tools/extract_bench.py (the benchmark's
-3 Illumina text at a tenth of its size in ten 10 MB blocks), compressed
once; then

  (a) decompress_file of the whole file,
  (b) find_names of 1 000 names spread over every block,
  (c) extract_names_file of those 1 000 names,
  (d) extract_names_file of 1 000 names that all lie in block 5,

each the median of 5 runs after one warmup, with the $FQZ5_FILE_TRACE stages
(median per stage), the match stage per block and the name bytes per second
it implies.  Not part of bench.py.

    python tools/names_bench.py [--out profiles/extract_names_l3.json]
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
RUNS, COUNT = 5, 1000


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=0.1)
    ap.add_argument("--blk", type=int, default=10_000_000)
    ap.add_argument("--level", type=int, default=3)
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
        heads = lines[0::4]
        ids = [h[1:].split(b" ", 1)[0] for h in heads]
        name_bytes = sum(len(h) for h in heads)             # each line less '@', plus its '\0'
        first = [0]
        for _, _, n in index:
            first.append(first[-1] + n)
        rng = random.Random(1)
        mid = len(index) // 2
        spread = [ids[r] for r in sorted(rng.sample(range(len(ids)), COUNT))]
        one = [ids[r] for r in sorted(rng.sample(range(first[mid], first[mid + 1]), COUNT))]

        def want(names):
            keep = set(names)
            return [r for r, x in enumerate(ids) if x in keep]

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
        find, find_st = timed(lambda: hits.append(Z.find_names(fqz, spread)))
        assert hits[-1].records.tolist() == want(spread) and not hits[-1].missing
        ext, ext_st = timed(lambda: Z.extract_names_file(fqz, out, spread))
        assert open(out, "rb").read() == text_of(want(spread)), "extracted text differs from the input"
        blk, blk_st = timed(lambda: hits.append(Z.extract_names_file(fqz, out, one)))
        rec_one = want(one)
        assert open(out, "rb").read() == text_of(rec_one), "extracted text differs from the input"
        blocks_one = sorted({sum(r >= f for f in first[1:]) for r in rec_one})

    def stage_ms(runs):
        keys = list(runs[0])
        return {k: round(1e3 * med([r.get(k, 0.0) for r in runs]), 3) for k in keys}

    def case(ts, st):
        return {"median_s": round(med(ts), 5), "runs": [round(x, 5) for x in ts],
                "stages_ms": stage_ms(st)}

    match_ms = stage_ms(find_st)["match"]
    res = {
        "tool": "tools/names_bench.py",
        "input": f"synth.illumina seed 1, {text_bytes} bytes of FASTQ, -{args.level}, "
                 f"blk_size {args.blk}",
        "text_bytes": text_bytes, "fqz5_bytes": size, "blocks": len(index),
        "records": len(ids), "name_section_bytes": name_bytes, "names": COUNT,
        "a_decompress_file": case(whole, whole_st),
        "b_find_names_spread": case(find, find_st),
        "c_extract_names_spread": dict(case(ext, ext_st), records=len(want(spread))),
        "d_extract_names_one_block": dict(case(blk, blk_st), records=len(rec_one),
                                          blocks_with_hits=blocks_one),
        "match_stage": {"ms_per_call": match_ms, "ms_per_block": round(match_ms / len(index), 3),
                        "name_bytes_per_s": round(name_bytes / (match_ms / 1e3)),
                        "note": "host wall time of fqz5_names_match per block (terminator "
                                "search, k_name_match, compaction, the count's download) and "
                                "the download of the compacted hits"},
        "ratio_a_over_b": round(med(whole) / med(find), 2),
        "ratio_a_over_d": round(med(whole) / med(blk), 2),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
