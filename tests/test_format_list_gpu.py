"""fqz5_fastq_format_list (fastq.hip): the text of an ascending list of a
decoded block's records, laid out on the device, against the bytes
fqz5_fastq_format (or _pairs) writes for those records, on the 6-record
block of tests/test_extract_gpu.py::test_format_range_every_slice."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib
from test_extract_gpu import GOLD, _Sections, _fasta, _fastq, _lines

pytestmark = pytest.mark.gpu
CAP = 4096


@pytest.fixture(scope="module", autouse=True)
def _need():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())


@pytest.fixture(scope="module")
def six():
    text = open(os.path.join(GOLD, "regression_srr1238539.fastq"), "rb").read()
    lines = _lines(text)[:24]
    assert len({len(lines[4 * k + 1]) for k in range(6)}) > 3          # lengths differ
    return lines, _Sections(lines)


def _part(sec, qual, plus_name, pairs, sel, cap=CAP):
    """fqz5_fastq_format_list of records `sel`: (rc, size of the size-only
    call, text, r1 size)."""
    so = Z._load()
    out = torch.full((CAP,), 0x7e, dtype=torch.uint8, device="cuda")
    d_sel = torch.from_numpy(np.asarray(list(sel) + [0], np.int32)).cuda()   # (never empty)
    size, size0, r1 = C.c_uint64(0), C.c_uint64(77), C.c_uint64(0)
    lib.after_torch()
    rc0 = so.fqz5_fastq_format_list(*sec.args(qual), d_sel.data_ptr(), len(sel), int(plus_name),
                                    int(pairs), None, 0, C.byref(size0), None)
    rc = so.fqz5_fastq_format_list(*sec.args(qual), d_sel.data_ptr(), len(sel), int(plus_name),
                                   int(pairs), out.data_ptr(), cap, C.byref(size), C.byref(r1))
    host = out.cpu().numpy().tobytes()
    if rc == 0:
        assert rc0 == 0 and size0.value == size.value            # the size-only call agrees
        assert host[size.value:] == b"\x7e" * (CAP - size.value)  # nothing past the text
    return rc, int(size0.value), host[:size.value], int(r1.value)


@pytest.mark.parametrize("qual,plus_name", [(True, False), (True, True), (False, False)])
def test_format_list_every_subset(six, qual, plus_name):
    lines, sec = six
    whole, _ = sec.whole(qual, plus_name, False)
    assert whole == (_fastq(lines, 0, 6, plus_name) if qual else _fasta(lines, 0, 6))
    per = 4 if qual else 2
    recs = [b"".join(x + b"\n" for x in _lines(whole)[per * k:per * k + per]) for k in range(6)]
    assert b"".join(recs) == whole
    paired, r1 = sec.whole(qual, plus_name, True)
    assert paired == b"".join(recs[0::2]) + b"".join(recs[1::2])
    for mask in range(64):
        sel = [k for k in range(6) if mask >> k & 1]
        rc, size0, got, g1 = _part(sec, qual, plus_name, False, sel)
        assert rc == 0 and got == b"".join(recs[k] for k in sel), sel
        assert size0 == len(got) == g1
        rc, size0, got, g1 = _part(sec, qual, plus_name, True, sel)
        even = b"".join(recs[k] for k in sel if k % 2 == 0)
        odd = b"".join(recs[k] for k in sel if k % 2)
        assert rc == 0 and got == even + odd and g1 == len(even) and size0 == len(got), sel
    rc, _, got, g1 = _part(sec, qual, plus_name, True, range(6))
    assert (got, g1) == (paired, r1)


def test_format_list_limits(six):
    lines, sec = six
    # n_sel = 0: nothing to do, nothing written
    rc, size0, got, g1 = _part(sec, True, False, False, [])
    assert (rc, size0, got, g1) == (0, 0, b"", 0)
    for bad in ([3, 2], [0, 1, 5, 4], [2, 2], [6], [0, 3, 6], [0, 2 ** 31 - 1]):
        for pairs in (False, True):
            rc, _, _, _ = _part(sec, True, False, pairs, bad)
            assert rc == -1 and "does not ascend or reaches past" in lib.last_error(), bad
    rc, _, _, _ = _part(sec, True, False, False, [0, 1, 2, 3, 4, 5, 5])
    assert rc == -1 and "more records listed" in lib.last_error()
    # the text does not fit out_cap
    sel = [1, 3, 4]
    want = b"".join(_fastq(lines, k, k + 1) for k in sel)
    rc, _, _, _ = _part(sec, True, False, False, sel, cap=len(want) - 1)
    assert rc == -1 and "out_cap" in lib.last_error()
    rc, _, got, _ = _part(sec, True, False, False, sel, cap=len(want))
    assert rc == 0 and got == want
    # the range path is as it was
    rc, _, got, _ = sec.part(True, False, False, 1, 3)
    assert rc == 0 and got == _fastq(lines, 1, 4)
