#!/usr/bin/env python3
"""Trim and clip against a whole-file decode and against the filter
("Trim and clip"): the input of tools/filter_bench.py
(the benchmark's -3 Illumina text at a tenth of its size in ten 10 MB
blocks), compressed once; then

  (a) decompress_file of the whole file (what a user does today before
      trimming elsewhere),
  (b) filter_file with min_mean_q=25,
  (c) trim_records with q3 alone,
  (d) trim_file with q3, one adapter and Filter(min_len=...),
  (e) trim_file with clip alone,

and stats of the file (the same decode as (c) without cuts), each the median
of 5 runs after one warmup, with the $FQZ5_FILE_TRACE stages (median per
stage).  The lengths (c) reports, and the counters, the selection and the
text (d) writes, are checked against the rule in plain Python
(tests/trim_ref.py) on the input text: (c) on every record, (d) on every
16th record (the adapter match in Python loops is slow) and on its totals of
records.  One further line times fqz5_trim_cuts and fqz5_trim_gather alone on
device arrays of the same number of bases cut into 150-base and into
15 000-base records (what a wave per record costs on long reads), checked
against fqz5_trim_host.  Not part of bench.py.

    python tools/trim_bench.py [--out profiles/trim_l3.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

FASTQ_REC = 358            # bench.py's bytes of text per synthetic 150 bp record
RUNS = 5
ADAPTER = b"AGATCGGAAGAGC"
SAMPLE = 16


def kernel_line(Z, lib, rec_len: int, bases: int, spec: dict) -> dict:
    """fqz5_trim_cuts and fqz5_trim_gather (bases and qualities) on device
    arrays of `bases` random bases in records of rec_len: median wall ms."""
    import torch
    so = Z._load()
    rng = np.random.default_rng(rec_len)
    n = bases // rec_len
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n * rec_len)]
    qual = rng.integers(2, 42, n * rec_len).astype(np.uint8)
    qual.reshape(n, rec_len)[:, -rec_len // 10:] = rng.integers(2, 14, (n, rec_len // 10))
    lens = np.full(n, rec_len, np.uint32)
    d_seq, d_qual = torch.from_numpy(seq).cuda(), torch.from_numpy(qual).cuda()
    d_out = torch.empty(n * rec_len + 1, dtype=torch.uint8, device="cuda")
    start = torch.empty(n, dtype=torch.int32, device="cuda")
    new, counts = np.zeros(n, np.uint32), np.zeros(12 + 2 * Z.TRIM_ADAPTERS, np.uint64)
    t, ad = Z.Trim(**spec).spec()
    got = C.c_uint64(0)

    def cuts():
        Z._check(so.fqz5_trim_cuts(C.byref(t), C.byref(ad), d_seq.data_ptr(), d_qual.data_ptr(),
                                   n * rec_len, lens.ctypes.data, n, 0, start.data_ptr(),
                                   new.ctypes.data, counts.ctypes.data), "fqz5_trim_cuts")

    def gather():
        for src in (d_seq, d_qual):
            Z._check(so.fqz5_trim_gather(src.data_ptr(), n * rec_len, lens.ctypes.data,
                                         start.data_ptr(), new.ctypes.data, n, d_out.data_ptr(),
                                         n * rec_len, C.byref(got)), "fqz5_trim_gather")
    out = {}
    lib.after_torch()
    for name, fn in (("cuts", cuts), ("gather_two_streams", gather)):
        fn()
        ts = []
        for _ in range(RUNS):
            t0 = time.perf_counter()
            fn()                                            # (both calls end synchronised)
            ts.append(time.perf_counter() - t0)
        out[name + "_ms"] = round(1e3 * statistics.median(ts), 3)
    hstart, hnew, _ = Z._trim_host(Z.Trim(**spec), seq.tobytes(), qual.tobytes(), lens)
    assert (hnew == new).all() and (start.cpu().numpy().view(np.uint32) == hstart).all()
    out.update(records=n, record_len=rec_len, bases=n * rec_len,
               bases_out=int(new.astype(np.uint64).sum()),
               cuts_bases_per_s=round(n * rec_len / (out["cuts_ms"] / 1e3)))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=0.1)
    ap.add_argument("--blk", type=int, default=10_000_000)
    ap.add_argument("--level", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON result here")
    args = ap.parse_args()

    import trim_ref as R
    from fqzcomp5_amd import fqz5file as Z
    from fqzcomp5_amd import lib, synth
    stages = []

    def grab(what):                       # the stages of each call, instead of stderr
        stages.append(dict(Z._TRACE))
        Z._TRACE.clear()
    Z._trace_dump = grab

    med = statistics.median
    with tempfile.TemporaryDirectory() as d:
        src, fqz, out = (os.path.join(d, n) for n in ("in.fastq", "in.fqz5", "out.fastq"))
        reads = synth.illumina(int(args.gb * 1e9 / FASTQ_REC), seed=1)
        text_bytes = synth.write_fastq(reads, src)
        size = Z.compress_file(src, fqz, args.level, blk_size=args.blk)
        index = Z.read_index(fqz)
        with open(src, "rb") as f:
            names, records = R.fastq_records(f.read())
        nrec = len(records)
        bases = sum(len(s) for s, _ in records)
        spec_c = {"q3": 20}
        spec_d = {"q3": 20, "adapters": [ADAPTER]}
        spec_e = {"head": 5, "tail": 5}
        min_len = 100

        def timed(fn):
            fn()                                            # warmup
            del stages[:]
            ts = []
            for _ in range(RUNS):
                t = time.perf_counter()
                fn()
                ts.append(time.perf_counter() - t)
            return ts, [dict(s) for s in stages]

        got = []
        whole, whole_st = timed(lambda: Z.decompress_file(fqz, out))
        assert os.path.getsize(out) == text_bytes
        st, st_st = timed(lambda: Z.stats(fqz))
        b, b_st = timed(lambda: got.append(Z.filter_file(fqz, out, Z.Filter(min_mean_q=25))))
        kept_b = len(got[-1].records)
        c, c_st = timed(lambda: got.append(Z.trim_records(fqz, Z.Trim(**spec_c), per_record=True)))
        h = got[-1]
        want = R.trim(records, spec_c)
        assert h.lengths.tolist() == want.lengths and h.starts.tolist() == want.starts
        assert h.removed.tolist() == want.removed and h.trimmed.tolist() == want.trimmed
        assert (h.bases_in, h.bases_out) == (bases, want.bases_out) and len(h.records) == nrec
        trimmed_c, out_c = want.trimmed[1], want.bases_out
        dd, d_st = timed(lambda: got.append(
            Z.trim_file(fqz, out, Z.Trim(**spec_d), Z.Filter(min_len=min_len))))
        h = got[-1]
        with open(out, "rb") as f:
            lines = f.read().split(b"\n")[:-1]
        assert len(lines) == 4 * len(h.records) and h.written == sum(len(x) + 1 for x in lines)
        where = {int(r): k for k, r in enumerate(h.records.tolist())}
        checked = 0
        for r in range(0, nrec, SAMPLE):
            a, e, _, _ = R.cut(records[r], spec_d)
            assert (r in where) == (e - a >= min_len), r
            if r in where:
                k = 4 * where[r]
                s, q = records[r]
                assert lines[k:k + 4] == [b"@" + names[r], s[a:e], b"+",
                                          bytes(x + 33 for x in q[a:e])], r
            checked += 1
        assert h.total == nrec and int(h.failed[0]) == nrec - len(h.records)
        assert h.bases_in == bases and h.removed[1] == want.removed[1]      # (the quality step is (c)'s)
        kept_d, written_d, hits_d = len(h.records), h.written, int(h.adapter_hits[0])
        del lines, where
        e, e_st = timed(lambda: got.append(Z.trim_file(fqz, out, Z.Trim(**spec_e))))
        h = got[-1]
        assert h.bases_out == sum(max(len(s) - 10, 0) for s, _ in records) and len(h.records) == nrec
        with open(out, "rb") as f:
            text_e = f.read()
        assert text_e[:4000] == R.text(names[:40], R.trim(records[:40], spec_e).records)[:4000]
        assert len(text_e) == h.written == text_bytes - 2 * (bases - h.bases_out)
        del text_e
    short = kernel_line(Z, lib, 150, 42_000_000, spec_d)
    long_ = kernel_line(Z, lib, 15_000, 42_000_000, spec_d)

    def stage_ms(runs):
        keys = list(runs[0])
        return {k: round(1e3 * med([r.get(k, 0.0) for r in runs]), 3) for k in keys}

    def case(ts, sts, **more):
        return dict(more, median_s=round(med(ts), 5), runs=[round(x, 5) for x in ts],
                    stages_ms=stage_ms(sts))

    ms_c = stage_ms(c_st)
    res = {
        "tool": "tools/trim_bench.py",
        "input": f"synth.illumina seed 1, {text_bytes} bytes of FASTQ, -{args.level}, "
                 f"blk_size {args.blk}",
        "text_bytes": text_bytes, "fqz5_bytes": size, "blocks": len(index), "records": nrec,
        "base_bytes": bases,
        "a_decompress_file": case(whole, whole_st),
        "stats": case(st, st_st),
        "b_filter_file": case(b, b_st, criteria="min_mean_q=25", kept=kept_b),
        "c_trim_records_q3": case(c, c_st, steps="q3=20, per_record", trimmed=trimmed_c,
                                  bases_out=out_c),
        "d_trim_file_q3_adapter_min_len": case(
            dd, d_st, steps=f"q3=20, adapters=[{ADAPTER.decode()}]", criteria=f"min_len={min_len}",
            kept=kept_d, written=written_d, adapter_hits=hits_d),
        "e_trim_file_clip": case(e, e_st, steps="head=5, tail=5", kept=nrec),
        "trim_stage": {"ms_per_call": ms_c["trim"],
                       "ms_per_block": round(ms_c["trim"] / len(index), 3),
                       "note": "host wall time per block of fqz5_trim_cuts (the record ends' upload, "
                               "the cuts kernel, the new lengths' and counters' download), the "
                               "starts' download (per_record), and the empty fqz5_filter_match with "
                               "the download of the selected indices"},
        "kernels_150_base_records": short,
        "kernels_15000_base_records": long_,
        "checked": f"(c) every record's start and length and the counters, (d) every {SAMPLE}th "
                   f"record's selection and text ({checked} records) and its totals, (e) its totals "
                   "and first records' text: all equal tests/trim_ref.py on the input text; the "
                   "kernel lines equal fqz5_trim_host",
        "ratio_c_over_stats": round(med(c) / med(st), 2),
        "ratio_d_over_a": round(med(dd) / med(whole), 2),
        "ratio_d_over_b": round(med(dd) / med(b), 2),
        "ratio_e_over_a": round(med(e) / med(whole), 2),
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
