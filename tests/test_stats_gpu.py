"""Read QC statistics of an .fqz5 (fqz5file.stats): one pass over the file,
every block checked, the sequence and quality sections decoded and
histogrammed on the GPU; no name is decoded and only the tables come back.

Expected values never come from the code under test: 4-line input decodes to
itself (tests/test_fqz5file_gpu.py::test_golden_files_vs_cli), so they are the
definitions restated with numpy (stats_ref.rule) on the text that was
compressed."""
import os
import random
import struct

import numpy as np
import pytest

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib, synth

import stats_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "fastq")


@pytest.fixture(scope="module", autouse=True)
def _need():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())


def _same(st, records, cycles, mates=1, what=None, per_record=False):
    """A Stats against the rule over the records the file was made from."""
    full = R.rule(records, cycles, mates)
    lens = [len(s) for s, _ in records]
    c = min(cycles, max(lens, default=0))
    assert st.cycles == c and st.mates == mates, what
    exp = dict(full, cycle_base=full["cycle_base"][:, :c], cycle_qual=full["cycle_qual"][:, :c])
    R.same(st.__dict__, exp, what)
    for m in range(mates):
        v, n = np.unique(lens[m::mates], return_counts=True)
        assert st.lengths[m][0].tolist() == v.tolist() and st.lengths[m][1].tolist() == n.tolist()
        assert st.lengths[m][1].dtype == np.uint64
        for x in (10, 50, 90):
            assert st.nx(x, m) == R.nx(lens[m::mates], x), (what, x)
    if not per_record:
        assert st.record_len is None and st.record_gc is None and st.record_qsum is None
        return
    assert (st.record_len.dtype, st.record_gc.dtype, st.record_qsum.dtype) == \
        (np.uint32, np.uint32, np.uint64)
    assert st.record_len.tolist() == lens
    assert (st.record_gc == full["record_gc"]).all() and (st.record_qsum == full["record_qsum"]).all()


@pytest.fixture(scope="module")
def gold():
    """(records, .fqz5 bytes, index) of regression_srr1238539.fastq at -3 in
    blocks of 2, 2, 2 and 1 records (tests/test_extract_gpu.py::gold)."""
    text = open(os.path.join(GOLD, "regression_srr1238539.fastq"), "rb").read()
    z = Z.compress_bytes(text, 3, blk_size=240)
    index = Z.read_index(z)
    assert [n for _, _, n in index] == [2, 2, 2, 1] and index.indexed
    return R.fastq_records(text), z, index


def test_golden_every_table(gold, tmp_path):
    records, z, _ = gold
    src = str(tmp_path / "g.fqz5")
    open(src, "wb").write(z)
    longest = max(len(s) for s, _ in records)
    for wb in (None, 1):                                   # one window; a window per block
        for what in (z, src):
            _same(Z.stats(what, window_bytes=wb), records, 1024, what=wb)
        _same(Z.stats(z, cycles=10, window_bytes=wb, per_record=True), records, 10, per_record=True)
    for cycles in (1, longest - 1, longest, longest + 1):
        _same(Z.stats(z, cycles=cycles), records, cycles, what=cycles)
    st = Z.stats(z)
    assert int(st.records[0]) == 7 == int(st.qual_records[0]) and int(st.empty[0]) == 0
    assert int(st.bases[0]) == int(st.base_counts.sum()) == int(st.qual_counts.sum())
    # a file without an index is walked by its block headers
    (idx,) = struct.unpack_from("<Q", z, 8)
    bare = z[:8] + struct.pack("<Q", 0) + z[16:idx]
    assert not Z.read_index(bare).indexed
    _same(Z.stats(bare), records, 1024)
    for cycles in (0, -1, (1 << 16) + 1):
        with pytest.raises(ValueError, match="cycles"):
            Z.stats(z, cycles=cycles)
    # an odd block under pairs
    with pytest.raises(lib.NativeError, match="odd record count"):
        Z.stats(z, pairs=True)


def test_sections_handed_to_the_decoder(gold, monkeypatch):
    """Per window exactly one decode, holding the sequence and quality
    sections only: never a name section."""
    records, z, _ = gold
    calls, real = [], Z.S.decode

    def decode(secs):
        calls.append([s.sec for s in secs])
        return real(secs)
    monkeypatch.setattr(Z.S, "decode", decode)
    Q, B = Z.S.SEC_QUAL, Z.S.SEC_SEQ
    _same(Z.stats(z), records, 1024)
    assert calls == [[B, Q] * 4]
    del calls[:]
    _same(Z.stats(z, window_bytes=1, per_record=True), records, 1024, per_record=True)
    assert calls == [[B, Q]] * 4
    assert Z.S.SEC_NAME not in sum(calls, [])


def test_damage_and_a_wrong_index(gold):
    records, z, index = gold
    for b, (_, e, _) in enumerate(index):
        bad = bytearray(z)
        bad[e - 3] ^= 0x20
        with pytest.raises(lib.NativeError, match="block CRC mismatch"):
            Z.stats(bytes(bad))
    (idx,) = struct.unpack_from("<Q", z, 8)
    off = bytearray(z)
    struct.pack_into("<I", off, idx + 12 + 16 * 3 + 12, 2)       # block 3's record count
    with pytest.raises(lib.NativeError, match="index disagrees with block 3"):
        Z.stats(bytes(off))
    _same(Z.stats(z), records, 1024)


def _reads(n: int, seed: int, name, lens, quals) -> bytes:
    rng = random.Random(seed)
    out = []
    for k in range(n):
        L = rng.randint(*lens)
        out += [b"@" + name(k), bytes(rng.choice(b"ACGTN") for _ in range(L)), b"+",
                bytes(rng.randint(*quals) for _ in range(L))]
    return b"".join(x + b"\n" for x in out)


def test_pairs():
    """Interleaved pairs whose mates differ in length range and quality range:
    per-mate tables are each input file's own, one mate their sum."""
    n = 40
    t1 = _reads(n, 1, lambda k: b"frag%d/1" % k, (70, 90), (60, 73))
    t2 = _reads(n, 2, lambda k: b"frag%d/2" % k, (30, 50), (35, 50))
    z = Z.compress_paired_bytes(t1, t2, 3, blk_size=2000)
    index = Z.read_index(z)
    assert len(index) >= 3 and all(c % 2 == 0 for _, _, c in index)
    r1, r2 = R.fastq_records(t1), R.fastq_records(t2)
    inter = [x for pair in zip(r1, r2) for x in pair]
    st = Z.stats(z, pairs=True, cycles=80, per_record=True)
    _same(st, inter, 80, mates=2, per_record=True)
    e1, e2 = R.rule(r1, 80), R.rule(r2, 80)
    for k in R.FIELDS:
        assert (getattr(st, k)[0] == e1[k][0]).all() and (getattr(st, k)[1] == e2[k][0]).all(), k
    assert not st.qual_counts[0, :27].any() and not st.qual_counts[1, 18:].any()
    one = Z.stats(z, cycles=80)
    _same(one, inter, 80)
    for k in R.FIELDS:
        assert (getattr(one, k)[0] == getattr(st, k).sum(0)).all(), k


@pytest.mark.parametrize("level", [3, 5])
def test_illumina_blocks_and_windows(level):
    """2 000 reads in several blocks read in at least three windows."""
    reads = synth.illumina(2000, seed=52)
    text = synth.fastq_chunk(reads, 0, reads.num_records).tobytes()
    records = R.fastq_records(text)
    assert len(records) == 2000
    z = Z.compress_bytes(text, level, blk_size=40_000)
    index = Z.read_index(z)
    assert len(index) >= 5                                 # two blocks a window at the most:
    wb = 2 * max(t - s for s, t, _ in index)               # three windows or more
    _same(Z.stats(z, window_bytes=wb, per_record=True), records, 1024, per_record=True)
    _same(Z.stats(z, cycles=100), records, 100)


def test_long_reads():
    """Records far longer than a tile, the cap below every read."""
    T = int(Z._load().fqz5_stats_tile())
    reads = synth.ont(24, seed=7, median=6 * T, with_names=True)
    text = synth.fastq_chunk(reads, 0, reads.num_records).tobytes()
    records = R.fastq_records(text)
    lens = [len(s) for s, _ in records]
    assert len(records) == 24 and min(lens) > 200 and max(lens) > 4 * T and sum(lens) < 2_000_000
    z = Z.compress_bytes(text, 3, blk_size=300_000)
    assert len(Z.read_index(z)) >= 2
    st = Z.stats(z, cycles=200, per_record=True)
    _same(st, records, 200, per_record=True)
    assert (st.cycle_qual.sum(2) == 24).all() and st.nx(50) == R.nx(lens, 50)
    assert st.nx(50) > T


def test_fasta_input():
    rng = random.Random(8)
    recs = [(b"contig%d len" % k, bytes(rng.choice(b"ACGTN") for _ in range(rng.randint(30, 200))))
            for k in range(60)]
    text = b"".join(b">" + h + b"\n" + s + b"\n" for h, s in recs)
    z = Z.compress_bytes(text, 3, blk_size=1500)
    assert len(Z.read_index(z)) >= 3 and Z.decompress_bytes(z) == text
    st = Z.stats(z, cycles=64, per_record=True)
    _same(st, [(s, None) for _, s in recs], 64, per_record=True)
    assert int(st.qual_records[0]) == 0 and int(st.records[0]) == 60
    assert not st.qual_counts.any() and not st.cycle_qual.any() and not st.read_qual.any()
    assert not st.record_qsum.any() and int(st.base_counts.sum()) == sum(len(s) for _, s in recs)


def test_no_records():
    """compress_bytes(b"") gives a container without a block: C is 0 and the
    tables are empty or zero."""
    z = Z.compress_bytes(b"", 3)
    assert len(Z.read_index(z)) == 0
    for pairs in (False, True):
        st = Z.stats(z, pairs=pairs, per_record=True)
        assert st.cycles == 0 and st.cycle_base.shape == (1 + pairs, 0, 6)
        assert st.cycle_qual.shape == (1 + pairs, 0, 256) and st.nx(50) == 0
        assert not st.records.any() and not st.base_counts.any() and not st.read_gc.any()
        assert len(st.record_len) == 0 and len(st.lengths[0][0]) == 0
