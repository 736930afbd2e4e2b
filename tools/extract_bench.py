#!/usr/bin/env python3
"""Record-range extraction against a whole-file decode (DESIGN.md section 4,
"Record ranges"): the benchmark's -3 Illumina text at a tenth of its size in
ten 10 MB blocks, compressed once; then

  * decompress_file of the whole file,
  * extract_file of 1 000 records from the middle of the middle block,

each the median of 5 runs after one warmup, with the extraction's
$FQZ5_FILE_TRACE stages (median per stage) and, from a fresh process, the
first extraction of a process (which creates the GPU context) next to its
second.  Not part of bench.py.

    python tools/extract_bench.py [--out profiles/extract_l3.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FASTQ_REC = 358            # bench.py's bytes of text per synthetic 150 bp record
RUNS, COUNT = 5, 1000


def _child(src: str, first: int) -> None:
    """A fresh process: its first extraction and its second."""
    import torch
    torch.cuda.init()
    from fqzcomp5_amd import fqz5file as Z
    out = []
    with tempfile.TemporaryDirectory() as d:
        for _ in range(2):
            t = time.perf_counter()
            Z.extract_file(src, os.path.join(d, "o.fastq"), first, COUNT)
            out.append(time.perf_counter() - t)
    print(json.dumps({"first_call_s": out[0], "second_call_s": out[1]}))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=0.1)
    ap.add_argument("--blk", type=int, default=10_000_000)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return _child(args.child[0], int(args.child[1]))

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
        t = time.perf_counter()
        size = Z.compress_file(src, fqz, args.level, blk_size=args.blk)
        t_comp = time.perf_counter() - t
        index = Z.read_index(fqz)
        mid = len(index) // 2
        first = sum(n for _, _, n in index[:mid]) + (index[mid][2] - COUNT) // 2
        assert Z.cover(index, first, COUNT) == [(mid, (index[mid][2] - COUNT) // 2, COUNT)]

        def timed(fn):
            fn()                                            # warmup
            del stages[:]
            ts = []
            for _ in range(RUNS):
                t = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t)
            return ts

        whole = timed(lambda: Z.decompress_file(fqz, out))
        assert os.path.getsize(out) == text_bytes
        whole_stages = [dict(s) for s in stages]
        part = timed(lambda: Z.extract_file(fqz, out, first, COUNT))
        part_stages = [dict(s) for s in stages]
        # the extracted text is the input's lines
        want = []
        with open(src, "rb") as f:
            for k, line in enumerate(f):
                if k >= 4 * (first + COUNT):
                    break
                if k >= 4 * first:
                    want.append(line)
        assert open(out, "rb").read() == b"".join(want), "extracted text differs from the input"
        fresh = json.loads(subprocess.run(
            [sys.executable, os.path.abspath(__file__), "--child", fqz, str(first)],
            check=True, capture_output=True, text=True, timeout=600).stdout.strip().splitlines()[-1])

    def stage_ms(runs):
        keys = list(runs[0])
        return {k: round(1e3 * med([r.get(k, 0.0) for r in runs]), 3) for k in keys}

    res = {
        "tool": "tools/extract_bench.py",
        "input": f"synth.illumina seed 1, {text_bytes} bytes of FASTQ, -{args.level}, "
                 f"blk_size {args.blk}",
        "text_bytes": text_bytes, "fqz5_bytes": size, "blocks": len(index),
        "block_records": [n for _, _, n in index],
        "compress_s": round(t_comp, 4),
        "decompress_file_s": {"median": round(med(whole), 5), "runs": [round(x, 5) for x in whole]},
        "decompress_file_stages_ms": stage_ms(whole_stages),
        "extract": {"block": mid, "first": first, "count": COUNT,
                    "block_bytes": index[mid][1] - index[mid][0]},
        "extract_file_s": {"median": round(med(part), 5), "runs": [round(x, 5) for x in part]},
        "extract_file_stages_ms": stage_ms(part_stages),
        "ratio_whole_over_extract": round(med(whole) / med(part), 2),
        "fresh_process": {k: round(v, 5) for k, v in fresh.items()},
    }
    print("[fqz5file] extract: " + ", ".join(f"{k} {v:.1f} ms"
                                             for k, v in res["extract_file_stages_ms"].items()),
          file=sys.stderr)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
