"""Records by read name out of an .fqz5 (fqz5file.find_names /
extract_names_bytes / extract_names_file): one pass over the file, every
block checked, only the name sections decoded and matched on the GPU, the
other sections decoded for the blocks with hits alone.

Expected values never come from the code under test: 4-line input decodes to
itself (tests/test_fqz5file_gpu.py::test_golden_files_vs_cli), so the records
that carry a name are found in the text that was compressed."""
import gzip
import os
import random
import re
import struct

import numpy as np
import pytest

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


def _ids(lines) -> list[bytes]:
    return [re.split(b"[ \t]", x[1:], maxsplit=1)[0] for x in lines[0::4]]


def _records(lines, names, whole=False, pairs=False) -> list[int]:
    """The records whose key is one of `names` (pairs: and their mates)."""
    want = set(names)
    keys = [x[1:] for x in lines[0::4]] if whole else _ids(lines)
    hit = [k in want for k in keys]
    return [r for r in range(len(keys))
            if hit[r] or (pairs and (r ^ 1) < len(keys) and hit[r ^ 1])]


def _text(lines, recs, plus_name=False, fasta=False) -> bytes:
    out = []
    for r in recs:
        h, s, p, q = lines[4 * r:4 * r + 4]
        if fasta:
            out += [b">" + h[1:], s]
        else:
            out += [h, s, b"+" + h[1:] if plus_name else p, q]
    return b"".join(x + b"\n" for x in out)


@pytest.fixture(scope="module")
def gold():
    """(lines, .fqz5 bytes, index) of regression_srr1238539.fastq at -3 in
    blocks of 2, 2, 2 and 1 records (tests/test_extract_gpu.py::gold)."""
    text = open(os.path.join(GOLD, "regression_srr1238539.fastq"), "rb").read()
    z = Z.compress_bytes(text, 3, blk_size=240)
    index = Z.read_index(z)
    assert [n for _, _, n in index] == [2, 2, 2, 1] and index.indexed
    return _lines(text), z, index


def test_golden_by_name(gold):
    lines, z, _ = gold
    ids = _ids(lines)
    assert ids[0] == b"SRR1238539.1" and len(set(ids)) == 7
    cases = {
        "records 0 and 6": [ids[0], ids[6]],
        "two ids of one block": [ids[3], ids[2]],
        "all, in reverse order": ids[::-1],
        "one present, one absent": [b"SRR1238539.8", ids[4]],
        "as str, given twice": [ids[5].decode(), ids[5], ids[1]],
    }
    for what, names in cases.items():
        asb = [x.encode() if isinstance(x, str) else x for x in names]
        recs = _records(lines, asb)
        assert Z.extract_names_bytes(z, names) == _text(lines, recs), what
        h = Z.find_names(z, names)
        assert h.records.dtype == np.uint64 and h.records.tolist() == recs, what
        assert h.query.dtype == np.int64
        assert h.query.tolist() == [asb.index(ids[r]) for r in recs], what
        assert h.missing == [x for k, x in enumerate(names)
                             if asb[k] not in ids and asb.index(asb[k]) == k], what
    assert Z.find_names(z, [b"SRR1238539.8", ids[4]]).missing == [b"SRR1238539.8"]
    assert Z.find_names(z, [b"nope", b"SRR1238539", b"SRR1238539.10"]).records.tolist() == []
    assert Z.extract_names_bytes(z, ids[::-1]) == b"".join(x + b"\n" for x in lines)
    assert Z.extract_names_bytes(z, []) == b""


def test_golden_forms(gold):
    lines, z, _ = gold
    ids = _ids(lines)
    names = [ids[5], ids[1], ids[2]]
    recs = [1, 2, 5]
    assert Z.extract_names_bytes(z, names, plus_name=True) == _text(lines, recs, plus_name=True)
    assert Z.extract_names_bytes(z, names, with_qual=False) == _text(lines, recs, fasta=True)
    # whole: the header line is the key, the bare id of a line with a comment is not
    full = [lines[4 * r][1:] for r in (4, 0)]
    assert full[0] == b"SRR1238539.5 5/1"
    assert Z.extract_names_bytes(z, full + [ids[3]], whole=True) == _text(lines, [0, 4])
    h = Z.find_names(z, full + [ids[3]], whole=True)
    assert (h.records.tolist(), h.query.tolist(), h.missing) == ([0, 4], [1, 0], [ids[3]])
    # without whole a full line matches nothing (no id holds a space)
    assert Z.extract_names_bytes(z, full) == b""
    with pytest.raises(ValueError, match="empty"):
        Z.find_names(z, [ids[0], b""])


def test_sections_handed_to_the_decoder(gold, monkeypatch):
    """The first decode sees the name sections of every block only; bases and
    qualities are handed over for the blocks with hits alone, and never by
    find_names."""
    lines, z, _ = gold
    ids = _ids(lines)
    calls, real = [], Z.S.decode

    def decode(secs):
        calls.append([s.sec for s in secs])
        return real(secs)
    monkeypatch.setattr(Z.S, "decode", decode)
    N, Q, B = Z.S.SEC_NAME, Z.S.SEC_QUAL, Z.S.SEC_SEQ
    assert Z.extract_names_bytes(z, [ids[2]]) == _text(lines, [2])
    assert calls == [[N] * 4, [B, Q]]                      # block 1 alone
    del calls[:]
    assert Z.extract_names_bytes(z, [ids[6], ids[0]], with_qual=False) == \
        _text(lines, [0, 6], fasta=True)
    assert calls == [[N] * 4, [B, B]]                      # blocks 0 and 3, no qualities
    del calls[:]
    assert Z.find_names(z, ids).records.tolist() == list(range(7))
    assert calls == [[N] * 4]
    del calls[:]
    assert Z.extract_names_bytes(z, [b"absent"]) == b""
    assert calls == [[N] * 4]


def test_files_windows_gzip_and_no_index(gold, tmp_path):
    lines, z, index = gold
    ids = _ids(lines)
    src = str(tmp_path / "g.fqz5")
    open(src, "wb").write(z)
    names = [ids[6], b"absent", ids[1], ids[2]]
    want = _text(lines, [1, 2, 6])
    for wb in (None, 1):                                   # one window; a window per block
        dst, dgz = str(tmp_path / "o.fastq"), str(tmp_path / "o.fastq.gz")
        h = Z.extract_names_file(src, dst, names, window_bytes=wb)
        assert open(dst, "rb").read() == want and h.written == len(want)
        assert (h.records.tolist(), h.query.tolist(), h.missing) == ([1, 2, 6], [2, 3, 0], [b"absent"])
        h = Z.extract_names_file(src, dgz, names, window_bytes=wb)
        assert gzip.open(dgz, "rb").read() == want and h.written == len(want)
        assert Z.find_names(src, names, window_bytes=wb).records.tolist() == [1, 2, 6]
    h = Z.extract_names_file(src, dst, [])
    assert h.written == 0 and open(dst, "rb").read() == b"" and h.records.tolist() == []
    # names from a list file
    lst = tmp_path / "names.txt"
    lst.write_bytes(b"\r\n".join(names) + b"\r\n")
    assert Z.extract_names_file(src, dst, Z.read_name_list(str(lst))).written == len(want)
    # a file without an index is walked by its block headers
    (idx,) = struct.unpack_from("<Q", z, 8)
    bare = z[:8] + struct.pack("<Q", 0) + z[16:idx]
    assert not Z.read_index(bare).indexed
    assert Z.extract_names_bytes(bare, names) == want
    assert Z.find_names(bare, names).records.tolist() == [1, 2, 6]


def test_damage_in_a_block_without_hits(gold):
    """Every block is checked: damage in block 0 fails a lookup whose names
    all lie in block 2."""
    lines, z, index = gold
    ids = _ids(lines)
    _, e0, _ = index[0]
    bad = bytearray(z)
    bad[e0 - 3] ^= 0x20
    bad = bytes(bad)
    for call in (Z.extract_names_bytes, Z.find_names):
        with pytest.raises(lib.NativeError, match="block CRC mismatch"):
            call(bad, [ids[4], ids[5]])
    # the index is checked against every block as well
    (idx,) = struct.unpack_from("<Q", z, 8)
    off = bytearray(z)
    struct.pack_into("<I", off, idx + 12 + 16 * 3 + 12, 2)       # block 3's record count
    with pytest.raises(lib.NativeError, match="index disagrees with block 3"):
        Z.find_names(bytes(off), [ids[0]])


def _reads(n: int, seed: int, name) -> bytes:
    rng = random.Random(seed)
    out = []
    for k in range(n):
        L = rng.randint(40, 90)
        out += [b"@" + name(k), bytes(rng.choice(b"ACGT") for _ in range(L)), b"+",
                bytes(rng.randint(35, 73) for _ in range(L))]
    return b"".join(x + b"\n" for x in out)


def test_pairs(tmp_path):
    """Interleaved pairs: mates that share an id both match it; with ids that
    differ, a hit on one mate takes the other as partner (query -1)."""
    n = 40
    t1, t2 = _reads(n, 1, lambda k: b"frag%d" % k), _reads(n, 2, lambda k: b"frag%d" % k)
    l1, l2 = _lines(t1), _lines(t2)
    z = Z.compress_paired_bytes(t1, t2, 3, blk_size=2000)
    index = Z.read_index(z)
    assert len(index) >= 3 and all(c % 2 == 0 for _, _, c in index)
    src, d1, d2 = (str(tmp_path / x) for x in ("p.fqz5", "o1.fastq", "o2.fastq"))
    open(src, "wb").write(z)
    names = [b"frag31", b"frag0", b"frag17", b"frag40"]
    h = Z.extract_names_file(src, d1, names, dst2=d2)
    assert open(d1, "rb").read() == _text(l1, [0, 17, 31])
    assert open(d2, "rb").read() == _text(l2, [0, 17, 31])
    assert h.records.tolist() == [0, 1, 34, 35, 62, 63] and h.query.tolist() == [1, 1, 2, 2, 0, 0]
    assert h.missing == [b"frag40"] and h.written == len(_text(l1, [0, 17, 31]) + _text(l2, [0, 17, 31]))
    # one output: the interleaved records that carry the name, both mates
    inter = [x for k in range(n) for x in l1[4 * k:4 * k + 4] + l2[4 * k:4 * k + 4]]
    assert Z.extract_names_bytes(z, [b"frag5"]) == _text(inter, [10, 11])
    # mates told apart by a suffix
    u1, u2 = _reads(n, 3, lambda k: b"m%d/1 c" % k), _reads(n, 4, lambda k: b"m%d/2 c" % k)
    k1, k2 = _lines(u1), _lines(u2)
    z = Z.compress_paired_bytes(u1, u2, 3, blk_size=2000)
    open(src, "wb").write(z)
    names = [b"m7/2", b"m7/1", b"m20/1", b"m33/2", b"m33"]
    h = Z.extract_names_file(src, d1, names, dst2=d2)
    assert open(d1, "rb").read() == _text(k1, [7, 20, 33])
    assert open(d2, "rb").read() == _text(k2, [7, 20, 33])
    assert h.records.tolist() == [14, 15, 40, 41, 66, 67]
    assert h.query.tolist() == [1, 0, 2, -1, -1, 3] and h.missing == [b"m33"]
    p = Z.find_names(src, names, pairs=True)
    assert (p.records.tolist(), p.query.tolist()) == (h.records.tolist(), h.query.tolist())
    s = Z.find_names(src, names)
    assert s.records.tolist() == [14, 15, 40, 67] and s.query.tolist() == [1, 0, 2, 3]
    inter = [x for k in range(n) for x in k1[4 * k:4 * k + 4] + k2[4 * k:4 * k + 4]]
    assert _records(inter, names, pairs=True) == h.records.tolist()
    assert Z.extract_names_bytes(z, names) == _text(inter, [14, 15, 40, 67])


def test_illumina_blocks_and_windows(tmp_path):
    """20 000 reads (~1 MB of names) in one block, and in several blocks read
    in at least three windows: 500 random ids."""
    reads = synth.illumina(20000, seed=51, with_names=True)
    text = synth.fastq_chunk(reads, 0, reads.num_records).tobytes()
    lines = _lines(text)
    ids = _ids(lines)
    rng = random.Random(3)
    names = [ids[r] for r in rng.sample(range(20000), 500)] + [b"A00123:45:HXXXXXXX:9:1:1:1"]
    recs = _records(lines, names)
    assert len(recs) >= 500
    want = _text(lines, recs)
    z = Z.compress_bytes(text, 1)
    assert len(Z.read_index(z)) == 1
    assert Z.extract_names_bytes(z, names) == want
    h = Z.find_names(z, names)
    assert h.records.tolist() == recs and h.missing == names[-1:]
    assert [names[q] for q in h.query.tolist()] == [ids[r] for r in recs]
    z = Z.compress_bytes(text, 1, blk_size=1_000_000)
    index = Z.read_index(z)
    assert len(index) >= 5                                 # two blocks a window at the most:
    wb = 2 * max(t - s for s, t, _ in index)               # three windows or more
    src, dst = str(tmp_path / "i.fqz5"), str(tmp_path / "o.fastq")
    open(src, "wb").write(z)
    h = Z.extract_names_file(src, dst, names, window_bytes=wb)
    assert open(dst, "rb").read() == want and h.written == len(want)
    assert h.records.tolist() == recs and h.missing == names[-1:]
