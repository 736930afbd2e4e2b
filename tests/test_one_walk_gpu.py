"""The read passes over an .fqz5 walk the file in the same windows:
extract_file over all records, find_names, find_seqs and stats read the
header and the index and then the same block ranges in the same order, for
every window size.  Seen from outside, through the positioned reads of the
file (os.pread)."""
import os
import struct

import pytest

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "fastq")


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    """(path, lines, index) of the first 6 records of
    regression_srr1238539.fastq at -3 in 3 blocks of 2 records
    (tests/test_extract_gpu.py::gold's split)."""
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())
    text = open(os.path.join(GOLD, "regression_srr1238539.fastq"), "rb").read()
    lines = text.split(b"\n")[:24]
    z = Z.compress_bytes(b"".join(x + b"\n" for x in lines), 3, blk_size=240)
    index = Z.read_index(z)
    assert [n for _, _, n in index] == [2, 2, 2] and index.indexed
    src = str(tmp_path_factory.mktemp("walk") / "three.fqz5")
    open(src, "wb").write(z)
    return src, lines, index


@pytest.mark.parametrize("which", ["one per window", "two largest", "default"])
def test_four_passes_same_windows(three, tmp_path, monkeypatch, which):
    src, lines, index = three
    size = os.path.getsize(src)
    (idx,) = struct.unpack_from("<Q", open(src, "rb").read(16), 8)
    sizes = sorted(t - s for s, t, _ in index)
    wb = {"one per window": 1, "two largest": sizes[-1] + sizes[-2], "default": None}[which]
    name = lines[8][1:].split(b" ")[0]                     # record 2's
    pat = lines[17][:12]                                   # the start of record 4's bases
    dst = str(tmp_path / "o.fastq")
    passes = {
        "extract_file": lambda: Z.extract_file(src, dst, 0, 6, window_bytes=wb),
        "find_names": lambda: Z.find_names(src, [name], window_bytes=wb),
        "find_seqs": lambda: Z.find_seqs(src, [pat], window_bytes=wb),
        "stats": lambda: Z.stats(src, window_bytes=wb),
    }
    real, seen = os.pread, {}
    for what, run in passes.items():
        reads = []

        def pread(fd, n, off):
            reads.append((off, off + n))
            return real(fd, n, off)
        monkeypatch.setattr(os, "pread", pread)
        res = run()
        monkeypatch.undo()
        assert reads[:2] == [(0, 16), (idx, size)], what
        seen[what] = (reads[2:], res)
    assert seen["extract_file"][1] == len(b"".join(x + b"\n" for x in lines))
    assert seen["find_names"][1].records.tolist() == [2]
    assert 4 in seen["find_seqs"][1].records.tolist()
    assert int(seen["stats"][1].records[0]) == 6
    walk = seen["extract_file"][0]
    for what, (reads, _) in seen.items():
        assert reads == walk, (what, reads, walk)
    # the windows tile the blocks, in file order
    assert walk[0][0] == index[0][0] and walk[-1][1] == index[-1][1] == idx
    assert all(a[1] == b[0] for a, b in zip(walk, walk[1:]))
    starts = [s for s, _, _ in index]
    assert all(a in starts for a, _ in walk)
    assert len(walk) == {"one per window": 3, "two largest": 2, "default": 1}[which]
