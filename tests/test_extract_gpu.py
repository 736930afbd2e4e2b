"""Record ranges out of an .fqz5 through its block index
(fqz5file.extract_bytes / extract_file, fastq.hip's fqz5_fastq_format_range):
only the blocks that hold the records are read and decoded, and their text is
laid out on the GPU for the wanted records alone.

Expected text never comes from the code under test: for 4-line input the full
decode equals the input (tests/test_fqz5file_gpu.py::test_golden_files_vs_cli),
so records [a, b) are lines 4a .. 4b of the text that was compressed."""
import ctypes as C
import os
import struct

import numpy as np
import pytest
import torch

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib, synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "fastq")


@pytest.fixture(scope="module", autouse=True)
def _need():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())


def _lines(text: bytes) -> list[bytes]:
    return text.split(b"\n")[:-1]


def _fastq(lines, a: int, b: int, plus_name: bool = False) -> bytes:
    """Records [a, b) of 4-line text (b clipped by the slice)."""
    out = []
    for k in range(4 * a, min(4 * b, len(lines)), 4):
        plus = b"+" + lines[k][1:] if plus_name else lines[k + 2]
        out += [lines[k], lines[k + 1], plus, lines[k + 3]]
    return b"".join(x + b"\n" for x in out)


def _fasta(lines, a: int, b: int) -> bytes:
    """The same records in output_fasta's form: '>' name, sequence."""
    out = []
    for k in range(4 * a, min(4 * b, len(lines)), 4):
        out += [b">" + lines[k][1:], lines[k + 1]]
    return b"".join(x + b"\n" for x in out)


# ---------------------------------------------------------------------------
# the golden file in >= 4 blocks
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    """(lines, .fqz5 bytes, index) of regression_srr1238539.fastq at -3.  Its
    7 records count 91, 91, 123, 113, 85, 81 and 81 bytes in the block split
    (name.l + 1 + bases + qualities, fqzcomp5.c:471-479), so blocks of at most
    240 bytes hold 2, 2, 2 and 1 of them."""
    text = open(os.path.join(GOLD, "regression_srr1238539.fastq"), "rb").read()
    z = Z.compress_bytes(text, 3, blk_size=240)
    index = Z.read_index(z)
    assert len(index) >= 4 and index.indexed
    assert sum(n for _, _, n in index) == len(_lines(text)) // 4 == 7
    assert [n for _, _, n in index][:3] == [2, 2, 2]      # the ranges below rely on it
    return _lines(text), z, index


def test_golden_ranges(gold):
    lines, z, index = gold
    total = len(lines) // 4
    ranges = {
        "first record": (0, 1),
        "everything": (0, total),
        "last record": (total - 1, 1),
        "ends at block 1's last record": (1, 3),
        "starts at block 1's first record": (2, 1),
        "crosses one boundary": (3, 2),
        "whole block 1, parts of blocks 0 and 2": (1, 4),
        "nothing": (3, 0),
        "first = total": (total, 2),
        "past the end": (5, 40),
    }
    assert Z.cover(index, 1, 4) == [(0, 1, 1), (1, 0, 2), (2, 0, 1)]
    assert Z.cover(index, 3, 2) == [(1, 1, 1), (2, 0, 1)]
    for what, (a, n) in ranges.items():
        got = Z.extract_bytes(z, a, n)
        assert got == _fastq(lines, a, a + n), what
    assert Z.extract_bytes(z, total, 2) == b"" and Z.extract_bytes(z, 3, 0) == b""
    assert Z.extract_bytes(z, 0, total) == b"".join(x + b"\n" for x in lines)


def test_golden_plus_name_and_fasta_form(gold):
    lines, z, _ = gold
    want = _fastq(lines, 3, 5, plus_name=True)
    assert want.count(b"\n+SRR1238539.") == 2
    assert Z.extract_bytes(z, 3, 2, plus_name=True) == want
    assert Z.extract_bytes(z, 3, 2, with_qual=False) == _fasta(lines, 3, 5)
    assert Z.extract_bytes(z, 1, 4, with_qual=False, plus_name=True) == _fasta(lines, 1, 5)


def test_with_qual_false_decodes_no_quality(gold, monkeypatch):
    """The quality sections are not handed to the section decoder at all."""
    lines, z, _ = gold
    seen = []
    real = Z.S.decode

    def decode(secs):
        seen.extend(s.sec for s in secs)
        return real(secs)
    monkeypatch.setattr(Z.S, "decode", decode)
    assert Z.extract_bytes(z, 3, 2, with_qual=False) == _fasta(lines, 3, 5)
    assert seen and Z.S.SEC_QUAL not in seen and len(seen) == 4     # names, bases of 2 blocks
    del seen[:]
    assert Z.extract_bytes(z, 3, 2) == _fastq(lines, 3, 5)
    assert seen.count(Z.S.SEC_QUAL) == 2


# ---------------------------------------------------------------------------
# scan and tile boundaries inside one block
# ---------------------------------------------------------------------------
def _one_block(reads, level):
    text = synth.fastq_chunk(reads, 0, reads.num_records).tobytes()
    z = Z.compress_bytes(text, level)
    index = Z.read_index(z)
    assert len(index) == 1 and index[0][2] == reads.num_records
    return _lines(text), z


def _name_starts(lines) -> np.ndarray:
    """Offset of every record's name in the block's name section (each
    record: its header line less '@', and a terminator); the last entry is
    the section's size."""
    return np.concatenate([[0], np.cumsum([len(x) for x in lines[0::4]])])


def test_tiles_illumina():
    """One block of 20 000 reads: ~1 MB of names, so the name terminators come
    from many delimiter-search tiles (FQ_TILE = 256 threads x 16 bytes x 16
    steps = 65 536 bytes, fastq.hip), and 20 000 records take several tiles of
    the scans (rocPRIM has no tuned scan entry for gfx950 and uses
    default_scan_config_base: 256 threads x 8 items = 2 048 64-bit values a
    tile, 4 096 32-bit ones)."""
    lines, z = _one_block(synth.illumina(20000, seed=51, with_names=True), 1)
    starts = _name_starts(lines)
    assert starts[20000] > 4 * 65536
    later = int(np.searchsorted(starts, 65536))           # its name starts in the second tile
    assert 0 < later < 19990 and starts[later] >= 65536 > starts[later - 1]
    for a, n in ((0, 1), (19999, 1), (9999, 3), (later, 2), (later - 1, 3), (2047, 3), (4095, 2)):
        assert Z.extract_bytes(z, a, n) == _fastq(lines, a, a + n), (a, n)
    assert Z.extract_bytes(z, 19998, 9, with_qual=False) == _fasta(lines, 19998, 20000)


def test_tiles_ont():
    """Variable lengths, reads far longer than a wave's 64 lanes and not
    multiples of 64."""
    r = synth.ont(300, seed=52, with_names=True)
    lens = r.lens.tolist()
    assert len(set(lens)) > 100 and max(lens) > 6400 and any(x % 64 for x in lens)
    lines, z = _one_block(r, 3)
    single = next(k for k in range(130, 300) if lens[k] % 64 and lens[k] > 640)
    for a, n in ((single, 1), (0, 3), (296, 4)):
        assert Z.extract_bytes(z, a, n) == _fastq(lines, a, a + n), (a, n)


# ---------------------------------------------------------------------------
# FASTA
# ---------------------------------------------------------------------------
def test_fasta_blocks():
    """Wrapped FASTA whose first record has no sequence: the text is
    output_fasta's one line per sequence (fqzcomp5.c:3503-3517)."""
    text = (b">r0 empty\n>r1 one\nACGTACGT\nACG\n>r2\nGGGTTTAAAC\nCC\nT\n>r3 x y\nTTGA\n"
            b">r4 last\nACGTTGCA\nAC\n")
    recs, cur = [], None
    for ln in _lines(text):                      # the parsed input, joined
        if ln.startswith(b">"):
            cur = [ln, b""]
            recs.append(cur)
        else:
            cur[1] += ln
    one = [h + b"\n" + s + b"\n" for h, s in recs]
    assert len(one) == 5 and one[0] == b">r0 empty\n\n"
    for blk in (None, 24):                       # one block; several
        z = Z.compress_bytes(text, 3, blk_size=blk)
        assert (len(Z.read_index(z)) > 2) == (blk is not None)
        for a, n in ((0, 1), (1, 2), (4, 1), (0, 5)):
            want = b"".join(one[a:a + n])
            assert Z.extract_bytes(z, a, n) == want, (blk, a, n)
            assert Z.extract_bytes(z, a, n, with_qual=False) == want, (blk, a, n)


# ---------------------------------------------------------------------------
# pairs
# ---------------------------------------------------------------------------
def test_pairs(tmp_path):
    t1 = open(os.path.join(GOLD, "paired_R1_nosuffix.fastq"), "rb").read()
    t2 = open(os.path.join(GOLD, "paired_R2_nosuffix.fastq"), "rb").read()
    l1, l2 = _lines(t1), _lines(t2)
    npairs = len(l1) // 4
    z = Z.compress_paired_bytes(t1, t2, 3, blk_size=100_000)
    index = Z.read_index(z)
    assert len(index) >= 3 and sum(n for _, _, n in index) == 2 * npairs
    assert all(n % 2 == 0 for _, _, n in index)
    src = str(tmp_path / "p.fqz5")
    open(src, "wb").write(z)
    edge = index[0][2] // 2                      # the first pair of block 1
    cases = {"inside block 0": (5, 7), "across a boundary": (edge - 2, 5),
             "clipped at the end": (npairs - 3, 10)}
    for what, (a, n) in cases.items():
        d1, d2 = str(tmp_path / "o1.fastq"), str(tmp_path / "o2.fastq")
        wrote = Z.extract_file(src, d1, a, n, dst2=d2)
        g1, g2 = open(d1, "rb").read(), open(d2, "rb").read()
        assert g1 == _fastq(l1, a, a + n) and g2 == _fastq(l2, a, a + n), what
        assert wrote == len(g1) + len(g2) and g1
    assert len(Z.cover(index, 2 * (edge - 2), 10)) == 2


def test_extract_file_outputs(gold, tmp_path):
    """One output, plain and gzip, in one window and a window per block."""
    import gzip
    lines, z, index = gold
    src = str(tmp_path / "g.fqz5")
    open(src, "wb").write(z)
    want = _fastq(lines, 1, 6)
    for wb in (None, 1):
        dst, dgz = str(tmp_path / "o.fastq"), str(tmp_path / "o.fastq.gz")
        assert Z.extract_file(src, dst, 1, 5, window_bytes=wb) == len(want)
        assert open(dst, "rb").read() == want
        assert Z.extract_file(src, dgz, 1, 5, window_bytes=wb) == len(want)
        assert gzip.open(dgz, "rb").read() == want
    assert Z.extract_file(src, dst, 7, 3) == 0 and open(dst, "rb").read() == b""


# ---------------------------------------------------------------------------
# v1.0 files and files without an index
# ---------------------------------------------------------------------------
def test_v10_sample():
    data = open(os.path.join(GOLD, "sample.fqz5"), "rb").read()
    lines = _lines(open(os.path.join(GOLD, "sample.fastq"), "rb").read())
    total = len(lines) // 4
    assert Z.read_index(data).version == Z.V10 and total == 5
    for k in range(total):
        assert Z.extract_bytes(data, k, 1) == _fastq(lines, k, k + 1), k
    assert Z.extract_bytes(data, 0, total) == _fastq(lines, 0, total)


def test_no_index_walk(gold):
    lines, z, index = gold
    (idx,) = struct.unpack_from("<Q", z, 8)
    bare = z[:8] + struct.pack("<Q", 0) + z[16:idx]
    walked = Z.read_index(bare)
    assert not walked.indexed and list(walked) == list(index)
    for a, n in ((0, 7), (1, 4), (3, 2), (6, 1), (7, 1)):
        assert Z.extract_bytes(bare, a, n) == Z.extract_bytes(z, a, n) == _fastq(lines, a, a + n)


# ---------------------------------------------------------------------------
# only the covering blocks are touched
# ---------------------------------------------------------------------------
def test_other_blocks_untouched(gold, tmp_path, monkeypatch):
    lines, z, index = gold
    (idx,) = struct.unpack_from("<Q", z, 8)
    s0, e0, _ = index[0]
    bad = bytearray(z)
    bad[e0 - 3] ^= 0x20                          # a payload byte of block 0
    bad = bytes(bad)
    # records 4 and 5 are block 2
    assert Z.cover(index, 4, 2) == [(2, 0, 2)]
    assert Z.extract_bytes(bad, 4, 2) == _fastq(lines, 4, 6)
    assert Z.extract_bytes(bad, 5, 1) == _fastq(lines, 5, 6)
    with pytest.raises(lib.NativeError, match="block CRC mismatch"):
        Z.extract_bytes(bad, 1, 4)
    with pytest.raises(lib.NativeError, match="block CRC mismatch"):
        Z.decompress_bytes(bad)
    src, dst = str(tmp_path / "bad.fqz5"), str(tmp_path / "o.fastq")
    open(src, "wb").write(bad)
    reads, real = [], os.pread

    def pread(fd, n, off):
        reads.append((off, off + n))
        return real(fd, n, off)
    monkeypatch.setattr(os, "pread", pread)
    assert Z.extract_file(src, dst, 4, 2) == len(_fastq(lines, 4, 6))
    monkeypatch.undo()
    assert open(dst, "rb").read() == _fastq(lines, 4, 6)
    s2, e2, _ = index[2]
    allowed = [(0, 16), (idx, len(z)), (s2, e2)]
    assert reads and all(any(a >= lo and b <= hi for lo, hi in allowed) for a, b in reads), reads
    assert any(a >= s2 and b <= e2 for a, b in reads)


def test_index_against_block(gold):
    lines, z, index = gold
    (idx,) = struct.unpack_from("<Q", z, 8)
    at = idx + 12 + 16 * 1 + 12                  # block 1's record count in the index
    (n1,) = struct.unpack_from("<I", z, at)
    assert n1 == index[1][2] == 2
    for wrong in (n1 + 1, n1 - 1):
        bad = bytearray(z)
        struct.pack_into("<I", bad, at, wrong)
        bad = bytes(bad)
        with pytest.raises(lib.NativeError, match="index disagrees with block 1"):
            Z.extract_bytes(bad, 2, 1)
        assert Z.extract_bytes(bad, 0, 2) == _fastq(lines, 0, 2)
    # a block offset that is not a block's start: the size field disagrees
    bad = bytearray(z)
    struct.pack_into("<Q", bad, idx + 12 + 16 * 2, index[2][0] + 1)
    with pytest.raises(lib.NativeError, match="index disagrees with block"):
        Z.extract_bytes(bytes(bad), 2, 1)


# ---------------------------------------------------------------------------
# fqz5_fastq_format_range against fqz5_fastq_format's bytes
# ---------------------------------------------------------------------------
class _Sections:
    """The decoded sections of one 6-record block, as the decoders leave
    them: names with a terminator each, bases, qualities - 33 (device), the
    lengths (host)."""

    def __init__(self, lines):
        n = len(lines) // 4
        names = b"".join(lines[4 * k][1:] + b"\0" for k in range(n))
        seq = b"".join(lines[4 * k + 1] for k in range(n))
        qual = bytes(c - 33 for k in range(n) for c in lines[4 * k + 3])
        up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
        self.names, self.seq, self.qual = up(names), up(seq), up(qual)
        self.lens = np.array([len(lines[4 * k + 1]) for k in range(n)], np.uint32)
        self.n = n

    def args(self, qual: bool):
        return (self.names.data_ptr(), int(self.names.numel()), self.seq.data_ptr(),
                self.qual.data_ptr() if qual else None, self.lens.ctypes.data, self.n)

    def whole(self, qual: bool, plus_name: bool, pairs: bool):
        """fqz5_fastq_format(_pairs) of the block: (text, r1 size)."""
        so = Z._load()
        out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        size, r1 = C.c_uint64(0), C.c_uint64(0)
        lib.after_torch()
        if pairs:
            rc = so.fqz5_fastq_format_pairs(*self.args(qual), int(plus_name), out.data_ptr(), 4096,
                                            C.byref(size), C.byref(r1))
        else:
            rc = so.fqz5_fastq_format(*self.args(qual), int(plus_name), out.data_ptr(), 4096,
                                      C.byref(size))
        assert rc == 0, lib.last_error()
        return out[:size.value].cpu().numpy().tobytes(), int(r1.value)

    def part(self, qual, plus_name, pairs, a, n, cap=4096, n_all=None):
        """fqz5_fastq_format_range: (rc, size from the size-only call, text, r1 size)."""
        so = Z._load()
        out = torch.full((4096,), 0x7e, dtype=torch.uint8, device="cuda")
        size, size0, r1 = C.c_uint64(0), C.c_uint64(77), C.c_uint64(0)
        head = self.args(qual)[:5] + (self.n if n_all is None else n_all,)
        lib.after_torch()
        rc0 = so.fqz5_fastq_format_range(*head, a, n, int(plus_name), int(pairs), None, 0,
                                         C.byref(size0), None)
        rc = so.fqz5_fastq_format_range(*head, a, n, int(plus_name), int(pairs), out.data_ptr(), cap,
                                        C.byref(size), C.byref(r1))
        host = out.cpu().numpy().tobytes()
        if rc == 0:
            assert rc0 == 0 and size0.value == size.value
            assert host[size.value:] == b"\x7e" * (4096 - size.value)   # nothing past the text
        return rc, int(size0.value), host[:size.value], int(r1.value)


@pytest.fixture(scope="module")
def six():
    text = open(os.path.join(GOLD, "regression_srr1238539.fastq"), "rb").read()
    lines = _lines(text)[:24]
    assert len({len(lines[4 * k + 1]) for k in range(6)}) > 3          # lengths differ
    return lines, _Sections(lines)


@pytest.mark.parametrize("qual,plus_name", [(True, False), (True, True), (False, False)])
def test_format_range_every_slice(six, qual, plus_name):
    lines, sec = six
    whole, _ = sec.whole(qual, plus_name, False)
    per = 4 if qual else 2
    recs = [b"".join(x + b"\n" for x in _lines(whole)[per * k:per * k + per]) for k in range(6)]
    assert b"".join(recs) == whole
    # (the whole-block formatter itself against the input's lines)
    assert whole == (_fastq(lines, 0, 6, plus_name) if qual else _fasta(lines, 0, 6))
    paired, r1 = sec.whole(qual, plus_name, True)
    assert paired == b"".join(recs[0::2]) + b"".join(recs[1::2])
    assert r1 == sum(len(x) for x in recs[0::2])
    for a in range(7):
        for n in range(7 - a):
            rc, size0, got, _ = sec.part(qual, plus_name, False, a, n)
            assert rc == 0 and got == b"".join(recs[a:a + n]), (a, n)
            assert size0 == len(got)
            rc, _, got, g1 = sec.part(qual, plus_name, True, a, n)
            even = b"".join(recs[k] for k in range(a, a + n) if k % 2 == 0)
            odd = b"".join(recs[k] for k in range(a, a + n) if k % 2)
            assert rc == 0 and got == even + odd and g1 == len(even), (a, n)
    rc, _, got, g1 = sec.part(qual, plus_name, True, 0, 6)
    assert (got, g1) == (paired, r1)


def test_format_range_limits(six):
    lines, sec = six
    for a, n in ((0, 7), (6, 1), (3, 4), (7, 0), (2 ** 63, 2 ** 63), (1, 2 ** 64 - 1)):
        rc, _, _, _ = sec.part(True, False, False, a, n)
        assert rc == -1 and "past the block" in lib.last_error(), (a, n)
    # more records claimed than the names have terminators
    rc, _, _, _ = sec.part(True, False, False, 5, 2, n_all=7)
    assert rc == -1 and "fewer names" in lib.last_error()
    # the text does not fit out_cap
    full = len(_fastq(lines, 2, 5))
    rc, _, _, _ = sec.part(True, False, False, 2, 3, cap=full - 1)
    assert rc == -1 and "out_cap" in lib.last_error()
    rc, _, got, _ = sec.part(True, False, False, 2, 3, cap=full)
    assert rc == 0 and got == _fastq(lines, 2, 5)
