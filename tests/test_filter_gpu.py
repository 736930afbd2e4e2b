"""Filter the records of an .fqz5 by read metrics (fqz5file.filter_records /
filter_bytes / filter_file): one pass over the file, every block checked, only
the sections the criteria need decoded before the pick on the GPU, the
remaining sections for the blocks with selected records alone.

Expected values never come from the code under test: 4-line input decodes to
itself (tests/test_fqz5file_gpu.py::test_golden_files_vs_cli), so the selection
is the rule restated in plain Python (filter_ref) on the text that was
compressed, and the text the selected records' own lines."""
import gzip
import os
import random
import struct

import numpy as np
import pytest

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib, synth

import filter_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "fastq")

# criteria that split the golden file's seven records, by the sections they need
LENGTHS = {"min_len": 36, "max_len": 50}
BASES = {"min_complexity_pct": 50, "gc_pct": (49, 52), "max_n": 0}
QUALS = {"min_mean_q": 21}
MIXED = {"min_len": 35, "low_q": 20, "max_low_pct": 39, "min_complexity_pct": 48}
CRITERIA = [LENGTHS, BASES, QUALS, MIXED]


@pytest.fixture(scope="module", autouse=True)
def _need():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())


def _text(texts, keep, plus_name=False, fasta=False) -> bytes:
    out = []
    for t, k in zip(texts, keep):
        if not k:
            continue
        h, s, p, q = t.split(b"\n")[:4]
        out += [b">" + h[1:], s] if fasta else [h, s, b"+" + h[1:] if plus_name else p, q]
    return b"".join(x + b"\n" for x in out)


def _same(h, records, crit, pairs=False, invert=False, written=None, what=None):
    keep, failed, total = R.rule(records, crit, pairs, invert)
    assert h.records.dtype == np.uint64 and h.failed.dtype == np.uint64, what
    assert h.records.tolist() == [i for i, k in enumerate(keep) if k], what
    assert h.failed.tolist() == failed and h.total == total, what
    if written is not None:
        assert h.written == written, what
    return keep


@pytest.fixture(scope="module")
def gold():
    """(records, each record's text, .fqz5 bytes, index) of
    regression_srr1238539.fastq at -3 in blocks of 2, 2, 2 and 1 records
    (tests/test_stats_gpu.py::gold)."""
    text = open(os.path.join(GOLD, "regression_srr1238539.fastq"), "rb").read()
    z = Z.compress_bytes(text, 3, blk_size=240)
    index = Z.read_index(z)
    assert [n for _, _, n in index] == [2, 2, 2, 1] and index.indexed
    records, texts = R.fastq_records(text)
    assert b"".join(texts) == text
    return records, texts, z, index


@pytest.fixture(scope="module")
def small():
    """(records, texts, .fqz5 bytes) of 300 synthetic reads in several blocks."""
    reads = synth.illumina(300, seed=61)
    text = synth.fastq_chunk(reads, 0, reads.num_records).tobytes()
    records, texts = R.fastq_records(text)
    assert len(records) == 300 and b"".join(texts) == text
    z = Z.compress_bytes(text, 3, blk_size=12_000)
    assert len(Z.read_index(z)) >= 4
    return records, texts, z


def test_the_criteria_decide(gold):
    records = gold[0]
    kept = [sum(R.rule(records, c)[0]) for c in CRITERIA]
    assert kept == [4, 4, 4, 3]


@pytest.mark.parametrize("crit", CRITERIA, ids=["lengths", "bases", "quals", "mixed"])
def test_golden_sources_and_windows(gold, tmp_path, crit):
    records, texts, z, _ = gold
    src, dst = str(tmp_path / "g.fqz5"), str(tmp_path / "o.fastq")
    open(src, "wb").write(z)
    (idx,) = struct.unpack_from("<Q", z, 8)
    bare = z[:8] + struct.pack("<Q", 0) + z[16:idx]       # a file without an index
    assert not Z.read_index(bare).indexed
    flt = Z.Filter(**crit)
    keep = R.rule(records, crit)[0]
    want = _text(texts, keep)
    assert 0 < len(want) < len(b"".join(texts))
    for wb in (None, 1):                                   # one window; a window per block
        for what in (z, src, bare):
            _same(Z.filter_records(what, flt, window_bytes=wb), records, crit, what=wb)
        h = Z.filter_file(src, dst, flt, window_bytes=wb)
        _same(h, records, crit, written=len(want))
        assert open(dst, "rb").read() == want
    for what in (z, bare):
        assert Z.filter_bytes(what, flt) == want


def test_text_options(gold, tmp_path):
    """plus_name, with_qual False (also where the qualities were decoded as a
    key), a .gz destination."""
    records, texts, z, _ = gold
    src, dst, dgz = (str(tmp_path / x) for x in ("g.fqz5", "o.fastq", "o.fastq.gz"))
    open(src, "wb").write(z)
    for crit in CRITERIA:
        flt, keep = Z.Filter(**crit), R.rule(records, crit)[0]
        assert Z.filter_bytes(z, flt, plus_name=True) == _text(texts, keep, plus_name=True)
        assert Z.filter_bytes(z, flt, with_qual=False) == _text(texts, keep, fasta=True)
        h = Z.filter_file(src, dst, flt, plus_name=True, with_qual=False, window_bytes=1)
        assert open(dst, "rb").read() == _text(texts, keep, fasta=True)
        h = Z.filter_file(src, dgz, flt)
        assert gzip.open(dgz, "rb").read() == _text(texts, keep) and h.written == len(_text(texts, keep))


@pytest.mark.parametrize("crit", CRITERIA, ids=["lengths", "bases", "quals", "mixed"])
def test_invert_partitions_the_file(gold, tmp_path, crit):
    records, texts, z, _ = gold
    flt = Z.Filter(**crit)
    keep = R.rule(records, crit)[0]
    a, b = Z.filter_records(z, flt), Z.filter_records(z, flt, invert=True)
    _same(b, records, crit, invert=True)
    assert sorted(a.records.tolist() + b.records.tolist()) == list(range(7))
    assert a.failed.tolist() == b.failed.tolist() and int(a.failed.sum()) == len(b.records)
    assert Z.filter_bytes(z, flt, invert=True) == _text(texts, [not k for k in keep])
    src, dst = str(tmp_path / "g.fqz5"), str(tmp_path / "o.fastq")
    open(src, "wb").write(z)
    h = Z.filter_file(src, dst, flt, invert=True, window_bytes=1)
    assert open(dst, "rb").read() == _text(texts, [not k for k in keep])
    assert h.written == len(b"".join(texts)) - len(_text(texts, keep))


def test_nothing_and_everything(gold):
    records, texts, z, _ = gold
    assert Z.filter_bytes(z, Z.Filter()) == b"".join(texts)          # no criterion: every record
    assert Z.filter_bytes(z, Z.Filter(), invert=True) == b""
    assert Z.filter_bytes(z, Z.Filter(min_mean_q=41)) == b""
    h = Z.filter_records(z, Z.Filter(min_mean_q=41, max_len=20))
    assert h.records.tolist() == [] and h.failed.tolist() == [0, 7, 0, 0, 0, 0, 0] and h.total == 7
    e = Z.compress_bytes(b"", 3)                            # a container without a block
    h = Z.filter_records(e, Z.Filter(min_len=1), pairs=True)
    assert h.records.tolist() == [] and h.total == 0 and not h.failed.any()
    assert Z.filter_bytes(e, Z.Filter(min_mean_q=1)) == b""
    with pytest.raises(TypeError):
        Z.filter_records(z, {"min_len": 1})


def test_synthetic_blocks(small, tmp_path):
    records, texts, z = small
    lens = sorted(len(s) for s, _ in records)
    qmean = sorted(sum(q) // max(len(q), 1) for _, q in records)
    crits = [{"min_mean_q": qmean[150]}, {"max_n": 0, "gc_pct": (40, 55)},
             {"min_len": lens[40], "low_q": qmean[150], "max_low_pct": 50, "min_complexity_pct": 70}]
    wb = 2 * max(t - s for s, t, _ in Z.read_index(z))
    src, dst = str(tmp_path / "s.fqz5"), str(tmp_path / "o.fastq")
    open(src, "wb").write(z)
    for crit in crits:
        keep = R.rule(records, crit)[0]
        assert 10 < sum(keep) < 290, crit
        h = Z.filter_file(src, dst, Z.Filter(**crit), window_bytes=wb)
        _same(h, records, crit, written=len(_text(texts, keep)), what=crit)
        assert open(dst, "rb").read() == _text(texts, keep)
        _same(Z.filter_records(z, Z.Filter(**crit), invert=True), records, crit, invert=True)


def _reads(n: int, seed: int, name, lens, quals) -> bytes:
    rng = random.Random(seed)
    out = []
    for k in range(n):
        L = rng.randint(*lens)
        out += [b"@" + name(k), bytes(rng.choice(b"ACGTACGTN") for _ in range(L)), b"+",
                bytes(rng.randint(*quals) for _ in range(L))]
    return b"".join(x + b"\n" for x in out)


def test_pairs(tmp_path):
    """Interleaved pairs: a pair is kept only when both mates pass; R1 records
    go to dst, R2 records to dst2."""
    n = 40
    t1 = _reads(n, 1, lambda k: b"frag%d/1" % k, (30, 60), (45, 73))
    t2 = _reads(n, 2, lambda k: b"frag%d/2" % k, (30, 60), (40, 73))
    z = Z.compress_paired_bytes(t1, t2, 3, blk_size=2000)
    index = Z.read_index(z)
    assert len(index) >= 3 and all(c % 2 == 0 for _, _, c in index)
    (r1, x1), (r2, x2) = R.fastq_records(t1), R.fastq_records(t2)
    inter = [x for pair in zip(r1, r2) for x in pair]
    itext = [x for pair in zip(x1, x2) for x in pair]
    crit = {"min_len": 36, "max_n": 6, "min_mean_q": 24}
    flt = Z.Filter(**crit)
    keep = R.rule(inter, crit, pairs=True)[0]
    single = R.rule(inter, crit)[0]
    assert 4 < sum(keep) // 2 < 36 and sum(single) > sum(keep)      # (some pairs lose one mate only)
    src, d1, d2 = (str(tmp_path / x) for x in ("p.fqz5", "o1.fastq", "o2.fastq"))
    open(src, "wb").write(z)
    for invert in (False, True):
        k = R.rule(inter, crit, pairs=True, invert=invert)[0]
        h = Z.filter_file(src, d1, flt, dst2=d2, invert=invert, window_bytes=1)
        _same(h, inter, crit, pairs=True, invert=invert)
        assert open(d1, "rb").read() == _text(x1, k[0::2])
        assert open(d2, "rb").read() == _text(x2, k[1::2])
        assert h.written == len(_text(itext, k))
        _same(Z.filter_records(z, flt, pairs=True, invert=invert), inter, crit, True, invert)
    _same(Z.filter_records(z, flt), inter, crit)
    assert Z.filter_bytes(z, flt) == _text(itext, single)


def test_sections_handed_to_the_decoder(gold, monkeypatch):
    """The key sections of a window in one call, the rest for the blocks with
    selected records in one further call; names only ever there."""
    records, texts, z, _ = gold
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
    # lengths alone: no key section; without hits no decode call at all
    h, got = run(Z.filter_records, z, Z.Filter(**LENGTHS))
    assert got == [] and h.records.tolist() == [0, 1, 3, 4]
    out, got = run(Z.filter_bytes, z, Z.Filter(min_len=1000))
    assert got == [] and out == b""
    out, got = run(Z.filter_bytes, z, Z.Filter(min_len=55))          # record 2: block 1 alone
    assert got == [[N, B, Q]] and out == texts[2]
    out, got = run(Z.filter_bytes, z, Z.Filter(**LENGTHS), with_qual=False)
    assert got == [[N, B] * 3]                              # blocks 0, 1 and 2
    # base criteria: never a quality section before the hit blocks' call
    keep = R.rule(records, BASES)[0]
    assert [i for i, k in enumerate(keep) if k] == [2, 3, 4, 6]    # blocks 1, 2 and 3
    h, got = run(Z.filter_records, z, Z.Filter(**BASES))
    assert got == [[B] * 4]
    out, got = run(Z.filter_bytes, z, Z.Filter(**BASES))
    assert got == [[B] * 4, [N, Q] * 3] and out == _text(texts, keep)
    out, got = run(Z.filter_bytes, z, Z.Filter(min_complexity_pct=60))   # records 3 and 6
    assert got == [[B] * 4, [N, Q] * 2] and out == texts[3] + texts[6]
    out, got = run(Z.filter_bytes, z, Z.Filter(min_complexity_pct=60), with_qual=False)
    assert got == [[B] * 4, [N] * 2]
    out, got = run(Z.filter_bytes, z, Z.Filter(min_complexity_pct=100, max_n=0))
    assert got == [[B] * 4, [N, Q]] and out == texts[6]
    h, got = run(Z.filter_records, z, Z.Filter(max_n=0, gc_pct=(90, 100)))
    assert got == [[B] * 4] and h.records.tolist() == []
    # quality criteria: bases and qualities are keys, names for the hit blocks alone
    h, got = run(Z.filter_records, z, Z.Filter(**QUALS))
    assert got == [[B, Q] * 4] and h.records.tolist() == [0, 2, 5, 6]
    out, got = run(Z.filter_bytes, z, Z.Filter(min_mean_q=24))       # records 2 and 6
    assert got == [[B, Q] * 4, [N] * 2] and out == texts[2] + texts[6]
    out, got = run(Z.filter_bytes, z, Z.Filter(min_mean_q=41))
    assert got == [[B, Q] * 4] and out == b""
    # a window per block: one key call per window
    h, got = run(Z.filter_records, z, Z.Filter(**QUALS), window_bytes=1)
    assert got == [[B, Q]] * 4


def test_fasta_input():
    rng = random.Random(8)
    recs = [(b"contig%d len" % k, bytes(rng.choice(b"ACGTN") for _ in range(rng.randint(30, 200))))
            for k in range(60)]
    text = b"".join(b">" + h + b"\n" + s + b"\n" for h, s in recs)
    z = Z.compress_bytes(text, 3, blk_size=1500)
    assert len(Z.read_index(z)) >= 3 and Z.decompress_bytes(z) == text
    for flt in (Z.Filter(min_mean_q=1), Z.Filter(low_q=1, max_low_pct=100),
                Z.Filter(min_len=1, min_mean_q=0)):
        for call in (Z.filter_records, Z.filter_bytes):
            with pytest.raises(lib.NativeError, match="block 0 has no qualities"):
                call(z, flt)
    records = [(s, None) for _, s in recs]
    for crit in ({"min_len": 100}, {"max_n": 20, "gc_pct": (35, 45)}, {"min_complexity_pct": 80}):
        keep = _same(Z.filter_records(z, Z.Filter(**crit)), records, crit)
        assert 0 < sum(keep) < 60
        want = b"".join(b">" + h + b"\n" + s + b"\n" for (h, s), k in zip(recs, keep) if k)
        assert Z.filter_bytes(z, Z.Filter(**crit)) == want


def test_damage_a_wrong_index_and_an_odd_block(gold):
    records, texts, z, index = gold
    for crit in (LENGTHS, QUALS):                           # also where no section is decoded
        flt = Z.Filter(**crit)
        for b, (_, e, _) in enumerate(index):
            bad = bytearray(z)
            bad[e - 3] ^= 0x20
            for call in (Z.filter_records, Z.filter_bytes):
                with pytest.raises(lib.NativeError, match="block CRC mismatch"):
                    call(bytes(bad), flt)
        (idx,) = struct.unpack_from("<Q", z, 8)
        off = bytearray(z)
        struct.pack_into("<I", off, idx + 12 + 16 * 3 + 12, 2)       # block 3's record count
        with pytest.raises(lib.NativeError, match="index disagrees with block 3"):
            Z.filter_records(bytes(off), flt)
        with pytest.raises(lib.NativeError, match="odd record count"):
            Z.filter_records(z, flt, pairs=True)
        _same(Z.filter_records(z, flt), records, crit)


def test_the_lookups_decode_lists_still_hold(gold, monkeypatch):
    """_key_windows now takes a set of key sections: the lookups by name and
    by sequence hand the decoder the lists they handed it before.  Their own
    tests (test_extract_names_gpu.py, test_extract_seqs_gpu.py::
    test_sections_handed_to_the_decoder) pin those lists and run in this suite
    as they are; this restates the shape of what they pin beside the filter's."""
    import test_extract_names_gpu as tn
    import test_extract_seqs_gpu as ts
    assert callable(tn.test_sections_handed_to_the_decoder)
    assert callable(ts.test_sections_handed_to_the_decoder)
    records, texts, z, _ = gold
    calls, real = [], Z.S.decode

    def decode(secs):
        calls.append([s.sec for s in secs])
        return real(secs)
    monkeypatch.setattr(Z.S, "decode", decode)
    N, Q, B = Z.S.SEC_NAME, Z.S.SEC_QUAL, Z.S.SEC_SEQ
    name = texts[2].split(b"\n")[0][1:].split(b" ")[0]
    assert Z.extract_names_bytes(z, [name]) == texts[2]
    assert calls == [[N] * 4, [B, Q]]                      # block 1 alone
    del calls[:]
    assert Z.find_names(z, [name]).records.tolist() == [2]
    assert calls == [[N] * 4]
    del calls[:]
    assert Z.extract_seqs_bytes(z, [records[2][0]]) == texts[2]
    assert calls == [[B] * 4, [N, Q]]
    del calls[:]
    assert Z.extract_seqs_bytes(z, [records[2][0]], with_qual=False) == \
        _text(texts, [k == 2 for k in range(7)], fasta=True)
    assert calls == [[B] * 4, [N]]
