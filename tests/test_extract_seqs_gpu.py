"""Records by sequence content out of an .fqz5 (fqz5file.find_seqs /
extract_seqs_bytes / extract_seqs_file): one pass over the file, every block
checked, only the sequence sections decoded and scanned on the GPU, the other
sections decoded for the blocks with hits alone.

Expected values never come from the code under test: 4-line input decodes to
itself (tests/test_fqz5file_gpu.py::test_golden_files_vs_cli), so the records
that hold a pattern are found with Python's `in` on the sequence lines of the
text that was compressed, by this rule per record: for i ascending, p_i in
seq -> (i, forward), else rc(p_i) in seq -> (i, reverse)."""
import gzip
import os
import random
import struct

import numpy as np
import pytest

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib, synth

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "fastq")
COMP = {65: 84, 67: 71, 71: 67, 84: 65, 97: 116, 99: 103, 103: 99, 116: 97, 78: 78, 110: 110}


@pytest.fixture(scope="module", autouse=True)
def _need():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())


def _lines(text: bytes) -> list[bytes]:
    return text.split(b"\n")[:-1]


def _rc(b: bytes) -> bytes:
    return bytes(COMP[c] for c in reversed(b))


def _rule(seqs, patterns, revcomp=False, pairs=False):
    """(records, query, reverse, missing) by the rule above."""
    pats = [p.encode() if isinstance(p, str) else p for p in patterns]
    own = []
    for s in seqs:
        got = None
        for i, p in enumerate(pats):
            if p in s:
                got = (i, False)
            elif revcomp and _rc(p) in s:
                got = (i, True)
            if got:
                break
        own.append(got)
    n = len(seqs)
    recs = [r for r in range(n) if own[r] or (pairs and (r ^ 1) < n and own[r ^ 1])]
    missing = [patterns[k] for k, p in enumerate(pats) if pats.index(p) == k and
               not any(p in s or (revcomp and _rc(p) in s) for s in seqs)]
    return (recs, [own[r][0] if own[r] else -1 for r in recs],
            [bool(own[r] and own[r][1]) for r in recs], missing)


def _text(lines, recs, plus_name=False, fasta=False) -> bytes:
    out = []
    for r in recs:
        h, s, p, q = lines[4 * r:4 * r + 4]
        if fasta:
            out += [b">" + h[1:], s]
        else:
            out += [h, s, b"+" + h[1:] if plus_name else p, q]
    return b"".join(x + b"\n" for x in out)


def _same(h, exp, what=None):
    assert h.records.dtype == np.uint64 and h.query.dtype == np.int64 and h.reverse.dtype == bool
    assert (h.records.tolist(), h.query.tolist(), h.reverse.tolist(), h.missing) == exp, what


@pytest.fixture(scope="module")
def gold():
    """(lines, .fqz5 bytes, index) of regression_srr1238539.fastq at -3 in
    blocks of 2, 2, 2 and 1 records (tests/test_extract_gpu.py::gold)."""
    text = open(os.path.join(GOLD, "regression_srr1238539.fastq"), "rb").read()
    z = Z.compress_bytes(text, 3, blk_size=240)
    index = Z.read_index(z)
    assert [n for _, _, n in index] == [2, 2, 2, 1] and index.indexed
    return _lines(text), z, index


def _holders(seqs, p: bytes, revcomp: bool = True) -> list[int]:
    return [k for k, s in enumerate(seqs) if p in s or (revcomp and _rc(p) in s)]


def _own(seqs, r: int, n: int, at: int = 3) -> bytes:
    """n bases of record r that no other record holds on either strand."""
    p = seqs[r][at:at + n]
    assert len(p) == n and set(p) <= set(b"ACGTN") and _holders(seqs, p) == [r]
    return p


ABSENT = b"ACGTTGCAACGTTGCAACGT"


@pytest.fixture(scope="module")
def pats(gold):
    """Patterns from the file's own sequence lines.  Records 0 to 5 are
    telomere repeats (every piece of records 0, 1, 4 and 5 also lies in the
    longer record 2); record 3 ends in bases of its own, record 6 is a GATC
    repeat.  `tel` lies in records 0..5, `tail3` in 3, `r6` in 6 (which also
    holds its reverse complement), `long2` in 2 alone."""
    seqs = gold[0][1::4]
    assert len(seqs) == 7
    P = {"tel": b"TTAGGGTTAGGGTT", "tail3": seqs[3][-20:], "r6": seqs[6][3:17], "long2": seqs[2][:50]}
    assert _holders(seqs, P["tel"]) == [0, 1, 2, 3, 4, 5] == _holders(seqs, P["tel"], False)
    assert _holders(seqs, P["tail3"]) == [3] and _holders(seqs, _rc(P["tail3"]), False) == []
    assert _holders(seqs, P["r6"], False) == [6] == _holders(seqs, _rc(P["r6"]), False)
    assert _holders(seqs, P["long2"]) == [2] and _holders(seqs, ABSENT) == []
    return P


def test_golden_by_sequence(gold, pats):
    lines, z, _ = gold
    seqs = lines[1::4]
    tel, tail3, r6, long2 = (pats[k] for k in ("tel", "tail3", "r6", "long2"))
    cases = {
        "records 3 and 6": [tail3, r6],
        "two of one block, in reverse order": [tail3, long2],
        "the repeat last: it takes what the others left": [r6, long2, tail3, tel],
        "the repeat first": [tel, r6, long2, tail3],
        "one present, one absent": [ABSENT, r6],
        "as str, given twice": [long2.decode(), long2, tail3],
        "a whole sequence line, which a longer record holds too": [seqs[4]],
        "the longest line, that line plus one base, another less one": [seqs[2], seqs[2] + b"A",
                                                                        seqs[3][1:]],
        "only as reverse complement": [_rc(tail3), _rc(long2)],
        "pattern 1 the reverse complement of pattern 0": [tail3, _rc(tail3), r6],
    }
    for what, ps in cases.items():
        for revcomp in (False, True):
            exp = _rule(seqs, ps, revcomp)
            assert Z.extract_seqs_bytes(z, ps, revcomp=revcomp) == _text(lines, exp[0]), what
            _same(Z.find_seqs(z, ps, revcomp=revcomp), exp, what)
    ps = [_rc(tail3), r6, _rc(long2)]
    _same(Z.find_seqs(z, ps, revcomp=True), ([2, 3, 6], [2, 0, 1], [True, True, False], []))
    _same(Z.find_seqs(z, ps), ([6], [1], [False], [ps[0], ps[2]]))
    # a record that holds two patterns reports the first listed; the other was seen
    _same(Z.find_seqs(z, [tel, tail3, ABSENT]),
          ([0, 1, 2, 3, 4, 5], [0] * 6, [False] * 6, [ABSENT]))
    _same(Z.find_seqs(z, [tail3, tel]), ([0, 1, 2, 3, 4, 5], [1, 1, 1, 0, 1, 1], [False] * 6, []))
    # forward is preferred to reverse for one pattern
    _same(Z.find_seqs(z, [_rc(r6)], revcomp=True), ([6], [0], [False], []))
    h = Z.find_seqs(z, [b"AC"], revcomp=True)
    _same(h, _rule(seqs, [b"AC"], True))
    assert h.reverse.tolist().count(True) >= 3 and h.reverse.tolist().count(False) >= 1
    assert Z.extract_seqs_bytes(z, [b"A", b"C", b"G", b"T"]) == b"".join(x + b"\n" for x in lines)
    assert Z.extract_seqs_bytes(z, []) == b""
    with pytest.raises(ValueError, match="without a complement"):
        Z.find_seqs(z, [tel, b"ACGR"], revcomp=True)
    assert Z.find_seqs(z, [b"ACGR"]).records.tolist() == []


def test_golden_forms(gold, pats):
    lines, z, _ = gold
    ps = [pats["r6"], _rc(pats["tail3"]), pats["long2"]]
    assert Z.extract_seqs_bytes(z, ps, revcomp=True, plus_name=True) == \
        _text(lines, [2, 3, 6], plus_name=True)
    assert Z.extract_seqs_bytes(z, ps, revcomp=True, with_qual=False) == \
        _text(lines, [2, 3, 6], fasta=True)
    assert Z.extract_seqs_bytes(z, ps, with_qual=False) == _text(lines, [2, 6], fasta=True)


def test_sections_handed_to_the_decoder(gold, pats, monkeypatch):
    """The first decode sees the sequence sections of every block only; names
    and qualities are handed over for the blocks with hits alone, and never by
    find_seqs."""
    lines, z, _ = gold
    calls, real = [], Z.S.decode

    def decode(secs):
        calls.append([s.sec for s in secs])
        return real(secs)
    monkeypatch.setattr(Z.S, "decode", decode)
    N, Q, B = Z.S.SEC_NAME, Z.S.SEC_QUAL, Z.S.SEC_SEQ
    assert Z.extract_seqs_bytes(z, [pats["long2"]]) == _text(lines, [2])
    assert calls == [[B] * 4, [N, Q]]                      # block 1 alone
    del calls[:]
    assert Z.extract_seqs_bytes(z, [pats["r6"], pats["tail3"]], with_qual=False) == \
        _text(lines, [3, 6], fasta=True)
    assert calls == [[B] * 4, [N, N]]                      # blocks 1 and 3, no qualities
    del calls[:]
    assert Z.extract_seqs_bytes(z, [pats["tel"]]) == _text(lines, range(6))
    assert calls == [[B] * 4, [N, Q] * 3]                  # blocks 0, 1 and 2
    del calls[:]
    assert Z.find_seqs(z, [b"G"]).records.tolist() == list(range(7))
    assert Z.find_seqs(z, [pats["tail3"]], revcomp=True, pairs=True).records.tolist() == [2, 3]
    assert calls == [[B] * 4, [B] * 4]
    del calls[:]
    assert Z.extract_seqs_bytes(z, [ABSENT]) == b""
    assert calls == [[B] * 4]


def test_files_windows_gzip_and_no_index(gold, pats, tmp_path):
    lines, z, index = gold
    seqs = lines[1::4]
    src = str(tmp_path / "g.fqz5")
    open(src, "wb").write(z)
    ps = [pats["r6"], ABSENT, _rc(pats["tail3"]), pats["long2"]]
    want = _text(lines, [2, 3, 6])
    for wb in (None, 1):                                   # one window; a window per block
        dst, dgz = str(tmp_path / "o.fastq"), str(tmp_path / "o.fastq.gz")
        h = Z.extract_seqs_file(src, dst, ps, revcomp=True, window_bytes=wb)
        assert open(dst, "rb").read() == want and h.written == len(want)
        _same(h, ([2, 3, 6], [3, 2, 0], [False, True, False], [ABSENT]))
        h = Z.extract_seqs_file(src, dgz, ps, revcomp=True, window_bytes=wb)
        assert gzip.open(dgz, "rb").read() == want and h.written == len(want)
        _same(Z.find_seqs(src, ps, revcomp=True, window_bytes=wb), _rule(seqs, ps, True))
        # seen in one window only, behind a lower pattern in another: not missing
        _same(Z.find_seqs(src, [pats["tel"], pats["tail3"], ABSENT], window_bytes=wb),
              ([0, 1, 2, 3, 4, 5], [0] * 6, [False] * 6, [ABSENT]))
    h = Z.extract_seqs_file(src, dst, [])
    assert h.written == 0 and open(dst, "rb").read() == b"" and h.records.tolist() == []
    # patterns from a list file
    lst = tmp_path / "patterns.fa"
    lst.write_bytes(b"".join(b">p%d\r\n%s\r\n%s\r\n" % (k, p[:7], p[7:]) for k, p in enumerate(ps)))
    assert Z.read_pattern_list(str(lst)) == ps
    h = Z.extract_seqs_file(src, dst, Z.read_pattern_list(str(lst)), revcomp=True)
    assert h.written == len(want)
    # a file without an index is walked by its block headers
    (idx,) = struct.unpack_from("<Q", z, 8)
    bare = z[:8] + struct.pack("<Q", 0) + z[16:idx]
    assert not Z.read_index(bare).indexed
    assert Z.extract_seqs_bytes(bare, ps, revcomp=True) == want


def test_damage_in_a_block_without_hits(gold, pats):
    """Every block is checked: damage in block 0 fails a search whose
    patterns all lie in blocks 1 and 3."""
    lines, z, index = gold
    ps = [pats["tail3"], pats["r6"]]
    _, e0, _ = index[0]
    bad = bytearray(z)
    bad[e0 - 3] ^= 0x20
    bad = bytes(bad)
    for call in (Z.extract_seqs_bytes, Z.find_seqs):
        with pytest.raises(lib.NativeError, match="block CRC mismatch"):
            call(bad, ps)
    assert Z.find_seqs(z, ps).records.tolist() == [3, 6]
    (idx,) = struct.unpack_from("<Q", z, 8)
    off = bytearray(z)
    struct.pack_into("<I", off, idx + 12 + 16 * 3 + 12, 2)       # block 3's record count
    with pytest.raises(lib.NativeError, match="index disagrees with block 3"):
        Z.find_seqs(bytes(off), ps)


def _reads(n: int, seed: int, name) -> bytes:
    rng = random.Random(seed)
    out = []
    for k in range(n):
        L = rng.randint(40, 90)
        out += [b"@" + name(k), bytes(rng.choice(b"ACGT") for _ in range(L)), b"+",
                bytes(rng.randint(35, 73) for _ in range(L))]
    return b"".join(x + b"\n" for x in out)


def test_pairs(tmp_path):
    """Interleaved pairs: a hit on one mate takes the other as partner
    (query -1); R1 records go to dst, R2 records to dst2."""
    n = 40
    t1, t2 = _reads(n, 1, lambda k: b"frag%d/1" % k), _reads(n, 2, lambda k: b"frag%d/2" % k)
    l1, l2 = _lines(t1), _lines(t2)
    z = Z.compress_paired_bytes(t1, t2, 3, blk_size=2000)
    index = Z.read_index(z)
    assert len(index) >= 3 and all(c % 2 == 0 for _, _, c in index)
    src, d1, d2 = (str(tmp_path / x) for x in ("p.fqz5", "o1.fastq", "o2.fastq"))
    open(src, "wb").write(z)
    inter = [x for k in range(n) for x in l1[4 * k:4 * k + 4] + l2[4 * k:4 * k + 4]]
    seqs = inter[1::4]
    # R2 of pair 31 (reverse strand), R1 of pair 0, both mates of pair 17, an absent one
    pats = [_rc(_own(seqs, 63, 20)), _own(seqs, 0, 20), _own(seqs, 34, 20), _own(seqs, 35, 20),
            b"ACGTTGCAACGTTGCAACGTTGCA"]
    h = Z.extract_seqs_file(src, d1, pats, revcomp=True, dst2=d2)
    assert open(d1, "rb").read() == _text(l1, [0, 17, 31])
    assert open(d2, "rb").read() == _text(l2, [0, 17, 31])
    _same(h, ([0, 1, 34, 35, 62, 63], [1, -1, 2, 3, -1, 0],
              [False, False, False, False, False, True], pats[4:]))
    assert h.written == len(_text(l1, [0, 17, 31]) + _text(l2, [0, 17, 31]))
    _same(h, _rule(seqs, pats, True, pairs=True))
    _same(Z.find_seqs(src, pats, revcomp=True, pairs=True), _rule(seqs, pats, True, pairs=True))
    _same(Z.find_seqs(src, pats, revcomp=True), _rule(seqs, pats, True))
    # one output: the interleaved records that hold a pattern
    assert Z.extract_seqs_bytes(z, pats, revcomp=True) == _text(inter, [0, 34, 35, 63])


@pytest.mark.parametrize("level", [3, 5])
def test_illumina_blocks_and_windows(tmp_path, level):
    """2 000 reads in several blocks read in at least three windows: 30
    patterns of 20 bases from the reads (half of them given as reverse
    complement), a short one that many reads hold, one absent."""
    reads = synth.illumina(2000, seed=52)
    text = synth.fastq_chunk(reads, 0, reads.num_records).tobytes()
    lines = _lines(text)
    seqs = lines[1::4]
    assert len(seqs) == 2000
    rng = random.Random(4)
    pats = []
    for k, r in enumerate(rng.sample(range(2000), 30)):
        at = rng.randint(0, len(seqs[r]) - 20)
        p = seqs[r][at:at + 20]
        assert set(p) <= set(b"ACGTN")
        pats.append(_rc(p) if k % 2 else p)
    pats += [b"ACGTTGCAACGTTGCAACGTTGCA", b"GATTACA"]
    exp = _rule(seqs, pats, True)
    assert 40 <= len(exp[0]) < 1500 and any(exp[2]) and not all(exp[2]) and exp[3] == pats[30:31]
    want = _text(lines, exp[0])
    z = Z.compress_bytes(text, level, blk_size=40_000)
    index = Z.read_index(z)
    assert len(index) >= 5                                 # two blocks a window at the most:
    wb = 2 * max(t - s for s, t, _ in index)               # three windows or more
    src, dst = str(tmp_path / "i.fqz5"), str(tmp_path / "o.fastq")
    open(src, "wb").write(z)
    h = Z.extract_seqs_file(src, dst, pats, revcomp=True, window_bytes=wb)
    assert open(dst, "rb").read() == want and h.written == len(want)
    _same(h, exp)
    _same(Z.find_seqs(z, pats, revcomp=True), exp)
    assert Z.extract_seqs_bytes(z, pats[:30]) == _text(lines, _rule(seqs, pats[:30])[0])


def test_fasta_input():
    rng = random.Random(8)
    recs = [(b"contig%d len" % k, bytes(rng.choice(b"ACGT") for _ in range(rng.randint(30, 200))))
            for k in range(60)]
    text = b"".join(b">" + h + b"\n" + s + b"\n" for h, s in recs)
    z = Z.compress_bytes(text, 3, blk_size=1500)
    assert len(Z.read_index(z)) >= 3 and Z.decompress_bytes(z) == text
    seqs = [s for _, s in recs]
    pats = [seqs[41][5:25], _rc(seqs[7][0:18]), seqs[59][-16:], b"ACGTTGCAACGTTGCAACGT"]
    exp = _rule(seqs, pats, True)
    assert exp[0] == [7, 41, 59] and exp[2] == [True, False, False]
    _same(Z.find_seqs(z, pats, revcomp=True), exp)
    want = b"".join(b">" + recs[r][0] + b"\n" + recs[r][1] + b"\n" for r in exp[0])
    assert Z.extract_seqs_bytes(z, pats, revcomp=True) == want
    assert Z.extract_seqs_bytes(z, pats, revcomp=True, with_qual=False) == want
