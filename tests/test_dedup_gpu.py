"""Drop the duplicate reads of an .fqz5 (fqz5file.dedup_records / dedup_bytes /
dedup_file / duplication): one pass over the file, every block's sequence
section decoded and keyed on the GPU, a device table across blocks and windows,
the other sections decoded for the blocks with selected records alone.

Expected values never come from the code under test: 4-line input decodes to
itself, so the selection is the exact deduplication by a dict on the sequences
of the text that was compressed (dedup_ref), and the text the selected
records' own lines.  Every input is first checked to have different keys for
different units."""
import gzip
import random

import numpy as np
import pytest

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib

import dedup_ref as R

pytestmark = pytest.mark.gpu
PER_BLOCK = 400                                             # records of a block of `single`
MODES = [(False, False), (False, True), (True, False), (True, True)]


@pytest.fixture(scope="module", autouse=True)
def _need():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())


def _fastq(names, seqs, rng):
    return [b"@" + n + b"\n" + s + b"\n+\n" + bytes(rng.randint(35, 73) for _ in s) + b"\n"
            for n, s in zip(names, seqs)]


def _text(texts, keep, fasta=False, plus_name=False) -> bytes:
    out = []
    for t, k in zip(texts, keep):
        if not k:
            continue
        h, s, p, q = t.split(b"\n")[:4]
        out += [b">" + h[1:], s] if fasta else [h, s, b"+" + h[1:] if plus_name else p, q]
    return b"".join(x + b"\n" for x in out)


def _windows(z) -> int:
    """A window size that puts two blocks in a window."""
    return 2 * max(e - s for s, e, _ in Z.read_index(z))


@pytest.fixture(scope="module")
def single():
    """2400 reads of 100 bases in six blocks of 400, three windows of two
    blocks: duplicates within block 0, from block 0 into blocks 1, 2 and 5
    (another window), one other strand, and block 4 a copy of block 0 whole.
    (sequences, each record's text, the text, .fqz5 bytes, window_bytes)"""
    rng = random.Random(71)
    n = 6 * PER_BLOCK
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(100)) for _ in range(n)]
    for _ in range(150):
        a, b = sorted(rng.sample(range(PER_BLOCK, 4 * PER_BLOCK), 2))
        seqs[b] = seqs[a]
    seqs[7] = seqs[3]
    seqs[450] = seqs[10]
    seqs[2000 + 300] = seqs[20]
    seqs[900] = R.revcomp(seqs[30])
    seqs[901] = seqs[30].lower()
    seqs[4 * PER_BLOCK:5 * PER_BLOCK] = seqs[:PER_BLOCK]
    texts = _fastq([b"r%05d" % k for k in range(n)], seqs, rng)
    text = b"".join(texts)
    z = Z.compress_bytes(text, 3, blk_size=207 * PER_BLOCK)    # name + 1 + bases + qualities
    assert [c for _, _, c in Z.read_index(z)] == [PER_BLOCK] * 6
    assert Z.decompress_bytes(z) == text
    for rc in (False, True):
        assert R.distinct_keys(seqs, False, rc)
    return seqs, texts, text, z, _windows(z)


@pytest.fixture(scope="module")
def paired():
    """1200 pairs in blocks of 100 pairs: pairs repeated within and across
    blocks, some with their mates swapped, some with one mate alone repeated.
    (interleaved sequences, R1 texts, R2 texts, .fqz5 bytes, window_bytes)"""
    rng = random.Random(73)
    n = 1200
    s1 = [bytes(rng.choice(b"ACGT") for _ in range(100)) for _ in range(n)]
    s2 = [bytes(rng.choice(b"ACGT") for _ in range(100)) for _ in range(n)]
    for k in range(300):
        a, b = sorted(rng.sample(range(n), 2))
        if k % 3 == 0:
            s1[b], s2[b] = s1[a], s2[a]
        elif k % 3 == 1:
            s1[b], s2[b] = s2[a], s1[a]
        else:
            s1[b] = s1[a]
    x1 = _fastq([b"f%05d/1" % k for k in range(n)], s1, rng)
    x2 = _fastq([b"f%05d/2" % k for k in range(n)], s2, rng)
    z = Z.compress_paired_bytes(b"".join(x1), b"".join(x2), 3, blk_size=209 * 200)
    index = Z.read_index(z)
    assert len(index) >= 6 and all(c % 2 == 0 for _, _, c in index)
    inter = [s for p in zip(s1, s2) for s in p]
    for rc in (False, True):
        assert R.distinct_keys(inter, True, rc)
    return inter, x1, x2, z, _windows(z)


@pytest.mark.parametrize("pairs,rc", MODES)
def test_records_against_the_exact_answer(single, paired, pairs, rc):
    seqs, z, wb = (paired[0], paired[3], paired[4]) if pairs else (single[0], single[3], single[4])
    mates = 2 if pairs else 1
    for invert in (False, True):
        keep, first, counts = R.dedup(seqs, pairs, rc, invert)
        h = Z.dedup_records(z, pairs, rc, invert, per_record=True, window_bytes=wb)
        assert h.records.dtype == np.uint64 and h.first.dtype == np.uint64
        assert h.records.tolist() == [r for r, k in enumerate(keep) if k], (pairs, rc, invert)
        assert h.first.tolist() == [mates * f for f in first]
        assert (h.total, h.distinct, h.written) == (len(seqs) // mates, len(counts), 0)
        assert 0 < len(h.records) < len(seqs)
        one = Z.dedup_records(z, pairs, rc, invert)         # one window: the same
        assert one.records.tolist() == h.records.tolist() and one.first is None
        assert (one.total, one.distinct) == (h.total, h.distinct)
    if not pairs:                                           # the other strand is dropped, case is kept
        got = Z.dedup_records(z, revcomp=rc).records.tolist()
        assert (900 in got) == (not rc) and 901 in got and 7 not in got and 2300 not in got


def test_bytes_are_the_kept_records_text(single):
    seqs, texts, text, z, wb = single
    for rc in (False, True):
        for invert in (False, True):
            keep = R.dedup(seqs, False, rc, invert)[0]
            want = _text(texts, keep)
            assert 0 < len(want) < len(text)
            assert Z.dedup_bytes(z, rc, invert, window_bytes=wb) == want
    keep = R.dedup(seqs)[0]
    assert Z.dedup_bytes(z) == _text(texts, keep)
    assert Z.dedup_bytes(z, plus_name=True) == _text(texts, keep, plus_name=True)
    assert Z.dedup_bytes(z, with_qual=False, window_bytes=wb) == _text(texts, keep, fasta=True)


def test_files(single, paired, tmp_path):
    """dedup_file: one destination, a .gz one, and dst2 for interleaved pairs
    (the split filter_file makes of the same pairs)."""
    seqs, texts, text, z, wb = single
    src, dst, dgz = (str(tmp_path / x) for x in ("s.fqz5", "o.fastq", "o.fastq.gz"))
    open(src, "wb").write(z)
    keep, _, counts = R.dedup(seqs)
    want = _text(texts, keep)
    for w in (None, wb):
        h = Z.dedup_file(src, dst, window_bytes=w)
        assert open(dst, "rb").read() == want
        assert (h.written, h.total, h.distinct) == (len(want), len(seqs), len(counts))
        assert h.records.tolist() == [r for r, k in enumerate(keep) if k]
    h = Z.dedup_file(src, dgz, with_qual=False, window_bytes=wb)
    assert gzip.open(dgz, "rb").read() == _text(texts, keep, fasta=True)
    inter, x1, x2, zp, wbp = paired
    srcp, d1, d2 = (str(tmp_path / x) for x in ("p.fqz5", "o1.fastq", "o2.fastq"))
    open(srcp, "wb").write(zp)
    for rc in (False, True):
        for invert in (False, True):
            k = R.dedup(inter, True, rc, invert)[0]
            h = Z.dedup_file(srcp, d1, d2, revcomp=rc, invert=invert, window_bytes=wbp)
            assert open(d1, "rb").read() == _text(x1, k[0::2])
            assert open(d2, "rb").read() == _text(x2, k[1::2])
            assert h.written == len(_text(x1, k[0::2])) + len(_text(x2, k[1::2]))
            assert h.records.tolist() == [r for r, kk in enumerate(k) if kk]
    # every pair passes an empty Filter: filter_file's split of all pairs, then the kept ones
    f1, f2 = str(tmp_path / "f1.fastq"), str(tmp_path / "f2.fastq")
    Z.filter_file(srcp, f1, Z.Filter(), dst2=f2)
    k = R.dedup(inter, True)[0]
    Z.dedup_file(srcp, d1, d2)
    pick = lambda path, kk: b"".join(                       # noqa: E731
        b"".join(x + b"\n" for x in ls) for ls, keep in zip(
            zip(*[iter(open(path, "rb").read().split(b"\n")[:-1])] * 4), kk) if keep)
    assert open(d1, "rb").read() == pick(f1, k[0::2])
    assert open(d2, "rb").read() == pick(f2, k[1::2])


def test_sections_handed_to_the_decoder(single, monkeypatch):
    """The sequence sections of a window in one call; names and qualities for
    the blocks with kept records alone: none for block 4, all duplicates."""
    seqs, texts, text, z, wb = single
    calls, real = [], Z.S.decode

    def decode(secs):
        calls.append([s.sec for s in secs])
        return real(secs)
    monkeypatch.setattr(Z.S, "decode", decode)
    N, Q, B = Z.S.SEC_NAME, Z.S.SEC_QUAL, Z.S.SEC_SEQ
    keep = R.dedup(seqs)[0]
    assert not any(keep[4 * PER_BLOCK:5 * PER_BLOCK]) and any(keep[5 * PER_BLOCK:])
    assert Z.dedup_bytes(z, window_bytes=wb) == _text(texts, keep)
    assert calls == [[B] * 2, [N, Q] * 2, [B] * 2, [N, Q] * 2, [B] * 2, [N, Q]]
    del calls[:]
    Z.dedup_records(z)
    assert calls == [[B] * 6]
    del calls[:]
    Z.dedup_bytes(z, with_qual=False)
    assert calls == [[B] * 6, [N] * 5]


def test_fasta_input():
    rng = random.Random(8)
    pool = [bytes(rng.choice(b"ACGTN") for _ in range(rng.randint(30, 200))) for _ in range(40)]
    recs = [(b"contig%d len" % k, rng.choice(pool)) for k in range(90)]
    text = b"".join(b">" + h + b"\n" + s + b"\n" for h, s in recs)
    z = Z.compress_bytes(text, 3, blk_size=1500)
    assert len(Z.read_index(z)) >= 3 and Z.decompress_bytes(z) == text
    seqs = [s for _, s in recs]
    assert R.distinct_keys(seqs)
    keep, _, counts = R.dedup(seqs)
    assert 0 < sum(keep) < 90
    want = b"".join(b">" + h + b"\n" + s + b"\n" for (h, s), k in zip(recs, keep) if k)
    assert Z.dedup_bytes(z, window_bytes=1) == want
    d = Z.duplication(z)
    assert (d.total, d.distinct, d.max_count) == (90, len(counts), max(counts))


def test_a_file_without_duplicates():
    rng = random.Random(9)
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(rng.randint(0, 120))) + b"A%dC" % k
            for k in range(500)]
    assert len(set(seqs)) == 500 and R.distinct_keys(seqs)
    text = b"".join(_fastq([b"u%d" % k for k in range(500)], seqs, rng))
    z = Z.compress_bytes(text, 3, blk_size=20_000)
    assert len(Z.read_index(z)) >= 4
    assert Z.dedup_bytes(z, window_bytes=1) == text
    assert Z.dedup_bytes(z, invert=True) == b""
    d = Z.duplication(z, window_bytes=1)
    assert d.distinct == d.total == 500 and d.max_count == 1 and d.remaining == 1.0
    assert d.levels[1] == 500 and int(d.levels.sum()) == 500
    e = Z.compress_bytes(b"", 3)                            # a container without a block
    h = Z.dedup_records(e, pairs=True, per_record=True)
    assert (h.records.tolist(), h.total, h.distinct, h.first.tolist()) == ([], 0, 0, [])
    d = Z.duplication(e)
    assert (d.total, d.distinct, d.max_count, d.remaining) == (0, 0, 0, 1.0)


@pytest.mark.parametrize("pairs,rc", MODES)
def test_duplication_levels(single, paired, pairs, rc):
    seqs, z, wb = (paired[0], paired[3], paired[4]) if pairs else (single[0], single[3], single[4])
    hist, distinct, top = R.levels(R.dedup(seqs, pairs, rc)[2])
    total = len(seqs) // (2 if pairs else 1)
    for w in (None, wb):
        d = Z.duplication(z, pairs, rc, window_bytes=w)
        assert d.levels.dtype == np.uint64 and d.levels.tolist() == hist
        assert (d.total, d.distinct, d.max_count) == (total, distinct, top)
        assert d.remaining == distinct / total
        assert sum(c * int(x) for c, x in enumerate(d.levels)) == total
    assert top >= 2 and distinct < total


def test_errors(single):
    seqs, texts, text, z, wb = single
    need = 32 * 8192                                        # 2400 units: 8192 slots of 32 bytes
    for call in (Z.dedup_records, Z.dedup_bytes, Z.duplication):
        with pytest.raises(lib.NativeError, match=f"a table of {need} bytes for 2400 units"):
            call(z, max_table_bytes=1)
    assert len(Z.dedup_records(z, max_table_bytes=need).records) == sum(R.dedup(seqs)[0])
    odd = Z.compress_bytes(b"".join(texts[:7]), 3)
    with pytest.raises(lib.NativeError, match="odd record count"):
        Z.dedup_records(odd, pairs=True)
    bad = bytearray(z)
    bad[Z.read_index(z)[2][1] - 3] ^= 0x20
    with pytest.raises(lib.NativeError, match="block CRC mismatch"):
        Z.dedup_records(bytes(bad))
