"""The host side of record-range extraction (fqzcomp5_amd/fqz5file.py):
read_index reads the container's block index (write_index,
fqzcomp5.c:2606-2630: "FQZ5IDX\\0", u32 nblocks, {u64 offset, u32 bases, u32
records} per block) or, without one, walks the block headers; cover maps a
record range onto the blocks that hold it.  No GPU: the blocks here are fake
byte strings that carry only a block's first two fields (size, records)."""
import os
import struct

import pytest

from fqzcomp5_amd import fqz5file as Z

HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLE = os.path.join(HERE, "golden", "fastq", "sample.fqz5")
NREC = [3, 1, 4, 7]
PAYLOAD = [40, 13, 64, 29]


def _fake_blocks():
    """Byte strings that start as a block does: u32 size of what follows,
    u32 records; then filler."""
    return [struct.pack("<II", 4 + p, n) + bytes([65 + k]) * p
            for k, (n, p) in enumerate(zip(NREC, PAYLOAD))]


def _file(magic=Z.MAGIC):
    blocks = _fake_blocks()
    data = Z.container(blocks, [10 * n for n in NREC], NREC)
    return magic + data[8:], blocks


def _expected(data):
    """_blocks_of's byte ranges with each block header's record count."""
    return [(s, e, struct.unpack_from("<I", data, s + 4)[0]) for s, e in Z._blocks_of(data)]


def _no_index(data):
    """The file without its index: offset field 0, the index bytes dropped."""
    (idx,) = struct.unpack_from("<Q", data, 8)
    return data[:8] + struct.pack("<Q", 0) + data[16:idx]


def test_read_index_round_trip(tmp_path):
    data, blocks = _file()
    want = _expected(data)
    assert [n for _, _, n in want] == NREC and len(want) == len(blocks)
    assert want[0][0] == 16 and [e - s for s, e, _ in want] == [len(b) for b in blocks]
    got = Z.read_index(data)
    assert list(got) == want and got.version == Z.V11 and got.indexed
    p = tmp_path / "a.fqz5"
    p.write_bytes(data)
    assert list(Z.read_index(str(p))) == want          # a path reads the same


def test_read_index_walk_fallback(tmp_path):
    data, _ = _file()
    want = _expected(data)
    bare = _no_index(data)
    got = Z.read_index(bare)
    assert list(got) == want and not got.indexed and got.version == Z.V11
    p = tmp_path / "b.fqz5"
    p.write_bytes(bare)
    assert list(Z.read_index(str(p))) == want
    # the old headerless format: blocks from offset 0 to the end of the file
    old = Z.read_index(bare[16:])
    assert old.version == Z.VOLD and list(old) == [(s - 16, e - 16, n) for s, e, n in want]


def test_read_index_v10_magic():
    data, _ = _file(Z.MAGIC_V10)
    got = Z.read_index(data)
    assert got.version == Z.V10 and list(got) == _expected(data)
    bare = Z.read_index(_no_index(data))
    assert bare.version == Z.V10 and list(bare) == list(got)


def test_read_index_sample_fqz5():
    """The reference's own v1.0 fixture."""
    data = open(SAMPLE, "rb").read()
    got = Z.read_index(data)
    assert got.version == Z.V10 and list(got) == _expected(data)
    assert [(s, e) for s, e, _ in got] == list(Z._blocks_of(data))
    assert list(Z.read_index(SAMPLE)) == list(got)


def test_read_index_touches_no_block(tmp_path, monkeypatch):
    """With an index offset: the header, then one positioned read of the index."""
    data, _ = _file()
    (idx,) = struct.unpack_from("<Q", data, 8)
    p = tmp_path / "c.fqz5"
    p.write_bytes(data)
    reads, real = [], os.pread

    def pread(fd, n, off):
        reads.append((off, n))
        return real(fd, n, off)
    monkeypatch.setattr(os, "pread", pread)
    Z.read_index(str(p))
    assert reads == [(0, 16), (idx, len(data) - idx)]


def test_read_index_empty_body():
    assert list(Z.read_index(Z.container([], [], []))) == []
    assert list(Z.read_index(Z.MAGIC + struct.pack("<Q", 0))) == []


def _patched(data, at, fmt, value):
    b = bytearray(data)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


def test_index_validation():
    data, _ = _file()
    (idx,) = struct.unpack_from("<Q", data, 8)
    ent = lambda k: idx + 12 + 16 * k                   # entry k's offset field
    (off2,) = struct.unpack_from("<Q", data, ent(2))
    bad = {
        "magic": data[:idx] + b"FQZ5IDY\0" + data[idx + 8:],
        "nblocks": _patched(data, idx + 8, "<I", len(NREC) + 1),
        "huge nblocks": _patched(data, idx + 8, "<I", 0xffffffff),
        "first offset": _patched(data, ent(0), "<Q", 20),
        "equal offsets": _patched(data, ent(1), "<Q", off2),
        "decreasing": _patched(data, ent(2), "<Q", 17),
        "last offset at the index": _patched(data, ent(3), "<Q", idx),
        "last offset past the index": _patched(data, ent(3), "<Q", idx + 40),
        "cut inside the index": data[:idx + 20],
        "cut at the index": data[:idx + 4],
    }
    for what, d in bad.items():
        with pytest.raises(ValueError, match="corrupt index"):
            Z.read_index(d)
            pytest.fail(what + ": a list came back")
    assert len(Z.read_index(data)) == len(NREC)         # (the unpatched file reads)


def _brute(nrec, first, count):
    """(block, record in block) of every record of the range, one by one."""
    recs = [(b, r) for b, n in enumerate(nrec) for r in range(n)]
    return recs[first:first + count]


def _spread(cov):
    return [(b, r) for b, rf, rc in cov for r in range(rf, rf + rc)]


def test_cover_against_brute_force():
    nrec = [3, 1, 4]
    index = Z.Index([(16 + 100 * k, 116 + 100 * k, n) for k, n in enumerate(nrec)])
    for first in range(10):
        for count in range(10):
            cov = Z.cover(index, first, count)
            assert _spread(cov) == _brute(nrec, first, count), (first, count)
            assert all(rc > 0 for _, _, rc in cov)
            assert [b for b, _, _ in cov] == sorted({b for b, _, _ in cov})


def test_cover_clipping_and_errors():
    index = Z.Index([(16, 116, 3), (116, 216, 1), (216, 316, 4)])
    assert Z.cover(index, 0, 8) == [(0, 0, 3), (1, 0, 1), (2, 0, 4)]
    assert Z.cover(index, 0, 10 ** 20) == [(0, 0, 3), (1, 0, 1), (2, 0, 4)]   # clipped
    assert Z.cover(index, 6, 100) == [(2, 2, 2)]
    assert Z.cover(index, 2, 3) == [(0, 2, 1), (1, 0, 1), (2, 0, 1)]
    assert Z.cover(index, 8, 1) == [] and Z.cover(index, 9, 5) == []          # at / past the total
    assert Z.cover(index, 10 ** 20, 1) == []
    assert Z.cover(index, 3, 0) == []
    assert Z.cover(Z.Index(), 0, 5) == [] and Z.cover([], 0, 0) == []
    for first, count in ((-1, 2), (0, -1), (-3, -3)):
        with pytest.raises(ValueError):
            Z.cover(index, first, count)


def test_cover_beyond_32_bits():
    """Prefix sums in Python ints: a file of more than 2^32 records."""
    n = 0xfffffff0
    index = Z.Index([(16, 20, n), (20, 24, n), (24, 28, 7)])
    assert Z.cover(index, 2 * n + 1, 3) == [(2, 1, 3)]
    assert Z.cover(index, n - 1, n + 2) == [(0, n - 1, 1), (1, 0, n), (2, 0, 1)]
