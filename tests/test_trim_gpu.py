"""Trim and clip the records of an .fqz5 (fqz5file.trim_records / trim_bytes /
trim_file): one pass over the file, the cut points found and the streams
compacted on the GPU, a Filter judged on the trimmed records, the text laid
out from the compacted streams.

Expected values never come from the code under test: 4-line input decodes to
itself (tests/test_fqz5file_gpu.py::test_golden_files_vs_cli), so the expected
text is the rule restated in plain Python (trim_ref) applied to the text that
was compressed, and the selection filter_ref's rule on the trimmed records."""
import gzip
import os
import random

import numpy as np
import pytest

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib, synth

import filter_ref as F
import trim_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "fastq")
AD1 = [b"AGATCGGAAGAGCACACGTC", b"CTGTCTCTTATACACATCT"]
AD2 = [b"AGATCGGAAGAGCGTCGTGT"]

# steps that shorten some of the golden file's seven records and not all
# (clip shortens every record that is not empty, and none of them has an N: both
# steps alone are judged on the synthetic reads, which have empty records)
GOLD_SPECS = {
    "quality": {"q5": 28, "q3": 12},
    "adapter": {"adapters": [b"GTAGGTACGG", b"AGGGTT"], "min_overlap": 6, "max_err_pct": 0},
    "crop": {"max_len": 36},
    "mixed": {"q3": 12, "adapters": [b"GTAGGTACGG"], "trim_n": True, "max_len": 50},
}
SMALL_SPECS = {
    "clip": {"head": 3, "tail": 200},
    "quality": {"q5": 30, "q3": 20},
    "adapter": {"adapters": AD1, "min_overlap": 4},
    "trim_n": {"trim_n": True},
    "crop": {"max_len": 120},
    "all": {"head": 3, "tail": 2, "q5": 30, "q3": 20, "adapters": AD1, "min_overlap": 4,
            "max_err_pct": 12, "trim_n": True, "max_len": 120},
}


@pytest.fixture(scope="module", autouse=True)
def _need():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())


def _plant(text: bytes, seed: int, adapters, empties=()) -> bytes:
    """The text with an adapter spliced into a seeded third of its reads at a
    random position (the read keeps its length, so near the end the adapter is
    cut off), a low-quality tail written into another third, and N ends and
    shorter reads in some of the rest; the records `empties` are emptied."""
    rng = random.Random(seed)
    names, records = R.fastq_records(text)
    out = []
    for i, (s, q) in enumerate(records):
        s, q = (bytearray(), bytearray()) if i in empties else (bytearray(s), bytearray(q))
        L = len(s)
        kind = rng.randrange(3)
        if not L:
            pass
        elif kind == 0:
            ad = rng.choice(adapters)
            at = rng.randint(L // 3, L - 4)
            s[at:] = (ad + bytes(rng.choice(b"ACGT") for _ in range(L)))[:L - at]
        elif kind == 1:
            k = rng.randint(1, min(60, L))
            q[L - k:] = bytes(rng.randint(2, 12) for _ in range(k))
        else:
            if rng.randrange(2):
                k = rng.randint(1, 5)
                s[:k], s[L - 2:] = b"N" * k, b"nN"
            if rng.randrange(3) == 0:
                cut = rng.randint(20, 120)
                s, q = s[:cut], q[:cut]
        out.append((bytes(s), bytes(q)))
    return R.text(names, out)


@pytest.fixture(scope="module")
def gold():
    """(names, records, text, .fqz5 bytes) of regression_srr1238539.fastq at -3
    in blocks of 2, 2, 2 and 1 records."""
    text = open(os.path.join(GOLD, "regression_srr1238539.fastq"), "rb").read()
    z = Z.compress_bytes(text, 3, blk_size=240)
    assert [n for _, _, n in Z.read_index(z)] == [2, 2, 2, 1]
    names, records = R.fastq_records(text)
    assert R.text(names, records) == text
    return names, records, text, z


@pytest.fixture(scope="module")
def small():
    """(names, records, text, .fqz5 bytes) of 300 synthetic reads with planted
    adapters and tails, in several blocks."""
    reads = synth.illumina(300, seed=61)
    # (records 1 and 2 are empty; a block's first record must not be, or the
    # block is coded as FASTA: test_fqz5file_gpu.py::test_fasta_rule_per_block_vs_reference)
    text = _plant(synth.fastq_chunk(reads, 0, reads.num_records).tobytes(), 5, AD1, (1, 2))
    names, records = R.fastq_records(text)
    assert len(records) == 300 and R.text(names, records) == text
    z = Z.compress_bytes(text, 3, blk_size=12_000)
    assert len(Z.read_index(z)) >= 4
    return names, records, text, z


def _counters(h, want, n, keep=None, written=None, what=None):
    assert h.trimmed.dtype == h.removed.dtype == h.adapter_hits.dtype == np.uint64
    assert (h.bases_in, h.bases_out) == (want.bases_in, want.bases_out), what
    assert h.trimmed.tolist() == want.trimmed and h.removed.tolist() == want.removed, what
    assert h.adapter_hits.tolist() == want.adapter_hits, what
    assert h.records.dtype == np.uint64
    assert h.records.tolist() == [i for i in range(n) if keep is None or keep[i]], what
    if written is not None:
        assert h.written == written, what


def _trim(records, spec, pairs=False):
    """trim_ref's result, with the number of records it shortened."""
    want = R.trim(records, spec, pairs)
    want.shortened = sum(n != len(s) for n, (s, _) in zip(want.lengths, records))
    return want


def _some_not_all(want, spec_name, n):
    """From the reference alone: the case trims some records and not all."""
    short = want.shortened
    assert 0 < short < n, (spec_name, short)
    if spec_name in R.STEPS:
        assert want.trimmed[R.STEPS.index(spec_name)] == short
    elif spec_name == "all":
        assert all(0 < t < n for t in want.trimmed), want.trimmed


@pytest.mark.parametrize("name", list(GOLD_SPECS))
def test_golden_sources_and_windows(gold, tmp_path, name):
    names, records, text, z = gold
    spec = GOLD_SPECS[name]
    want = _trim(records, spec)
    _some_not_all(want, name, 7)
    exp = R.text(names, want.records)
    src, dst = str(tmp_path / "g.fqz5"), str(tmp_path / "o.fastq")
    open(src, "wb").write(z)
    trim = Z.Trim(**spec)
    assert Z.trim_bytes(z, trim) == exp
    for wb in (None, 1):                                   # one window; a window per block
        for what in (z, src):
            h = Z.trim_records(what, trim, per_record=True, window_bytes=wb)
            _counters(h, want, 7, what=(name, wb))
            assert h.starts.dtype == h.lengths.dtype == np.uint32
            assert h.starts.tolist() == want.starts and h.lengths.tolist() == want.lengths
            assert h.total == 7 and not h.failed.any() and h.written == 0
        h = Z.trim_file(src, dst, trim, window_bytes=wb)
        _counters(h, want, 7, written=len(exp))
        assert open(dst, "rb").read() == exp and h.starts is None


@pytest.mark.parametrize("name", list(SMALL_SPECS))
def test_synthetic_blocks(small, name):
    names, records, text, z = small
    spec = SMALL_SPECS[name]
    want = _trim(records, spec)
    _some_not_all(want, name, 300)
    assert Z.trim_bytes(z, Z.Trim(**spec)) == R.text(names, want.records)
    h = Z.trim_records(z, Z.Trim(**spec), per_record=True)
    _counters(h, want, 300, what=name)
    assert h.starts.tolist() == want.starts and h.lengths.tolist() == want.lengths
    if name == "adapter":
        assert all(want.adapter_hits)


def test_text_options_and_windows(small, tmp_path):
    """plus_name, with_qual False, a .gz destination, several windows."""
    names, records, text, z = small
    src, dst, dgz = (str(tmp_path / x) for x in ("s.fqz5", "o.fastq", "o.fastq.gz"))
    open(src, "wb").write(z)
    wb = 2 * max(t - s for s, t, _ in Z.read_index(z))
    for name in ("clip", "adapter", "all"):                # no key, the bases, bases and qualities
        spec = SMALL_SPECS[name]
        trim, want = Z.Trim(**spec), R.trim(records, spec)
        assert Z.trim_bytes(z, trim, plus_name=True) == R.text(names, want.records, plus_name=True)
        fasta = R.text(names, want.records, with_qual=False)
        assert Z.trim_bytes(z, trim, with_qual=False) == fasta
        exp = R.text(names, want.records)
        for w in (None, wb, 1):
            h = Z.trim_file(src, dst, trim, window_bytes=w)
            _counters(h, want, 300, written=len(exp), what=(name, w))
            assert open(dst, "rb").read() == exp
        h = Z.trim_file(src, dst, trim, plus_name=True, with_qual=False, window_bytes=wb)
        assert open(dst, "rb").read() == fasta and h.written == len(fasta)
        h = Z.trim_file(src, dgz, trim)
        assert gzip.open(dgz, "rb").read() == exp and h.written == len(exp)


def test_nothing_set_is_the_decoder(gold, small):
    for names, records, text, z in (gold, small):
        assert Z.trim_bytes(z, Z.Trim()) == Z.decompress_bytes(z) == text
        assert Z.trim_bytes(z, Z.Trim(), plus_name=True) == Z.decompress_bytes(z, plus_name=True)
        h = Z.trim_records(z, Z.Trim())
        assert h.bases_in == h.bases_out == sum(len(s) for s, _ in records)
        assert not h.trimmed.any() and not h.removed.any() and len(h.adapter_hits) == 0
        assert h.records.tolist() == list(range(len(records)))
    # records trimmed to nothing are still records
    names, records, text, z = gold
    empty = b"".join(b"@" + n + b"\n\n+\n\n" for n in names)
    assert Z.trim_bytes(z, Z.Trim(max_len=0)) == empty
    assert Z.trim_bytes(z, Z.Trim(head=1000)) == empty
    e = Z.compress_bytes(b"", 3)                            # a container without a block
    h = Z.trim_records(e, Z.Trim(q3=20), per_record=True)
    assert h.total == 0 and h.bases_in == 0 and len(h.starts) == 0 and len(h.records) == 0
    assert Z.trim_bytes(e, Z.Trim(q3=20)) == b""
    with pytest.raises(TypeError):
        Z.trim_records(z, {"head": 1})
    with pytest.raises(TypeError):
        Z.trim_records(z, Z.Trim(head=1), {"min_len": 1})


@pytest.mark.parametrize("name", ["clip", "adapter", "all"])
def test_filter_judges_the_trimmed_reads(small, tmp_path, name):
    names, records, text, z = small
    spec = {"head": 3, "tail": 40} if name == "clip" else SMALL_SPECS[name]
    want = R.trim(records, spec)
    crit = {"min_len": 100, "min_mean_q": 16}
    keep, failed, total = F.rule(want.records, crit)
    untrimmed = F.rule(records, crit)[0]
    assert 10 < sum(keep) < 290 and keep != untrimmed      # the trim changes the verdicts
    src, dst = str(tmp_path / "s.fqz5"), str(tmp_path / "o.fastq")
    open(src, "wb").write(z)
    trim, flt = Z.Trim(**spec), Z.Filter(**crit)
    for invert in (False, True):
        k = [x != invert for x in keep]
        exp = R.text(names, want.records, k)
        h = Z.trim_file(src, dst, trim, flt, invert=invert, window_bytes=1)
        _counters(h, want, 300, k, len(exp), what=(name, invert))      # counted before the selection
        assert h.failed.tolist() == failed and h.total == total
        assert open(dst, "rb").read() == exp
    assert Z.trim_bytes(z, trim, flt) == R.text(names, want.records, keep)
    h = Z.trim_records(z, trim, flt, per_record=True)
    _counters(h, want, 300, keep)
    assert h.lengths.tolist() == want.lengths and h.failed.tolist() == failed
    # a length criterion alone (with clip alone no section is a key)
    k2 = F.rule(want.records, {"min_len": 110})[0]
    assert Z.trim_records(z, trim, Z.Filter(min_len=110)).records.tolist() == \
        [i for i, x in enumerate(k2) if x]


def _reads(n: int, seed: int, name, adapters) -> bytes:
    rng = random.Random(seed)
    out = []
    for k in range(n):
        L = rng.randint(30, 90)
        out += [b"@" + name(k), bytes(rng.choice(b"ACGTACGTN") for _ in range(L)), b"+",
                bytes(rng.randint(40, 73) for _ in range(L))]
    return _plant(b"".join(x + b"\n" for x in out), seed + 100, adapters)


def test_pairs(tmp_path):
    """Interleaved pairs: each mate trimmed on its own, the odd records with
    adapters2; a pair is kept only when both trimmed mates pass; R1 records go
    to dst, R2 records to dst2."""
    n = 40
    t1 = _reads(n, 1, lambda k: b"frag%d/1" % k, AD1)
    t2 = _reads(n, 2, lambda k: b"frag%d/2" % k, AD2)
    z = Z.compress_paired_bytes(t1, t2, 3, blk_size=2000)
    index = Z.read_index(z)
    assert len(index) >= 3 and all(c % 2 == 0 for _, _, c in index)
    (n1, r1), (n2, r2) = R.fastq_records(t1), R.fastq_records(t2)
    inames = [x for pair in zip(n1, n2) for x in pair]
    inter = [x for pair in zip(r1, r2) for x in pair]
    spec = {"q3": 20, "adapters": AD1, "adapters2": AD2, "min_overlap": 5, "trim_n": True}
    want = R.trim(inter, spec, pairs=True)
    assert want.adapter_hits[2] > 0 and sum(want.adapter_hits[:2]) > 0
    assert want.lengths != R.trim(inter, spec).lengths     # mate 2's adapters matter
    assert 0 < want.trimmed[2] < 2 * n
    crit = {"min_len": 30, "min_mean_q": 15}
    trim, flt = Z.Trim(**spec), Z.Filter(**crit)
    single = F.rule(want.records, crit)[0]
    src, d1, d2 = (str(tmp_path / x) for x in ("p.fqz5", "o1.fastq", "o2.fastq.gz"))
    open(src, "wb").write(z)
    for invert in (False, True):
        keep, failed, total = F.rule(want.records, crit, pairs=True, invert=invert)
        if not invert:
            assert 4 < sum(keep) // 2 < 36 and sum(single) > sum(keep)   # (pairs that lose one mate)
        h = Z.trim_file(src, d1, trim, flt, dst2=d2, invert=invert, window_bytes=1)
        _counters(h, want, 2 * n, keep)
        assert h.failed.tolist() == failed and h.total == total == n
        e1 = R.text(inames[0::2], want.records[0::2], keep[0::2])
        e2 = R.text(inames[1::2], want.records[1::2], keep[1::2])
        assert open(d1, "rb").read() == e1 and gzip.open(d2, "rb").read() == e2
        assert h.written == len(e1) + len(e2)
    h = Z.trim_records(z, trim, pairs=True, per_record=True)
    _counters(h, want, 2 * n)
    assert h.lengths.tolist() == want.lengths and h.starts.tolist() == want.starts
    with pytest.raises(lib.NativeError, match="odd record count"):
        Z.trim_records(Z.compress_bytes(b"\n".join(t1.split(b"\n")[:4]) + b"\n", 3), trim,
                       pairs=True)


def test_sections_handed_to_the_decoder(gold, monkeypatch):
    """The key sections of a window in one call, the rest for the blocks with
    selected records in one further call; names only ever there."""
    names, records, text, z = gold
    calls, real = [], Z.S.decode

    def decode(secs):
        calls.append([s.sec for s in secs])
        return real(secs)
    monkeypatch.setattr(Z.S, "decode", decode)
    N, Q, B = Z.S.SEC_NAME, Z.S.SEC_QUAL, Z.S.SEC_SEQ

    def run(fn, *a, **kw):
        del calls[:]
        out = fn(*a, **kw)
        return out, list(calls)
    h, got = run(Z.trim_records, z, Z.Trim(head=3, max_len=20))
    assert got == [] and h.bases_out == 7 * 20
    h, got = run(Z.trim_records, z, Z.Trim(trim_n=True))
    assert got == [[B] * 4]
    h, got = run(Z.trim_records, z, Z.Trim(q3=12), Z.Filter(min_len=30))
    assert got == [[B, Q] * 4]
    h, got = run(Z.trim_records, z, Z.Trim(head=3), Z.Filter(min_mean_q=20))
    assert got == [[B, Q] * 4]
    out, got = run(Z.trim_bytes, z, Z.Trim(head=3))
    assert got == [[N, B, Q] * 4] and out == R.text(names, R.trim(records, {"head": 3}).records)
    out, got = run(Z.trim_bytes, z, Z.Trim(trim_n=True), with_qual=False)
    assert got == [[B] * 4, [N] * 4]
    out, got = run(Z.trim_bytes, z, Z.Trim(trim_n=True))
    assert got == [[B] * 4, [N, Q] * 4]
    out, got = run(Z.trim_bytes, z, Z.Trim(q3=12), Z.Filter(min_len=52))   # record 2: block 1 alone
    assert got == [[B, Q] * 4, [N]]
    want = R.trim(records, {"q3": 12})
    assert out == R.text(names, want.records, [n >= 52 for n in want.lengths]) and out


def test_fasta_input():
    rng = random.Random(8)
    recs = []
    for k in range(60):
        s = bytearray(rng.choice(b"ACGTN") for _ in range(rng.randint(30, 200)))
        if k % 2:
            at = rng.randint(0, len(s) - 4)
            s[at:] = AD1[0][:len(s) - at]
        recs.append((b"contig%d len" % k, bytes(s)))
    text = b"".join(b">" + h + b"\n" + s + b"\n" for h, s in recs)
    z = Z.compress_bytes(text, 3, blk_size=1500)
    assert len(Z.read_index(z)) >= 3 and Z.decompress_bytes(z) == text
    for trim in (Z.Trim(q3=20), Z.Trim(q5=1, adapters=AD1)):
        for call in (Z.trim_records, Z.trim_bytes):
            with pytest.raises(lib.NativeError, match="block 0 has no qualities"):
                call(z, trim)
    names, records = [h for h, _ in recs], [(s, None) for _, s in recs]
    for spec in ({"adapters": AD1, "trim_n": True}, {"head": 10, "max_len": 50}):
        want = R.trim(records, spec)
        assert 0 < sum(n != len(s) for n, (s, _) in zip(want.lengths, records)) <= 60
        assert Z.trim_bytes(z, Z.Trim(**spec)) == R.text(names, want.records)
        _counters(Z.trim_records(z, Z.Trim(**spec)), want, 60)
    want = R.trim(records, {"adapters": AD1})
    assert 0 < want.trimmed[2] < 60


def test_a_damaged_block(gold):
    names, records, text, z = gold
    for spec in ({"head": 2}, {"q3": 12}):                  # also where no section is decoded
        for b, (_, e, _) in enumerate(Z.read_index(z)):
            bad = bytearray(z)
            bad[e - 3] ^= 0x20
            for call in (Z.trim_records, Z.trim_bytes):
                with pytest.raises(lib.NativeError, match="block CRC mismatch"):
                    call(bytes(bad), Z.Trim(**spec))
