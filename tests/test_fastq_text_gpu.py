"""The FASTQ text kernels of fastq.hip against kseq_ref, the plain
restatement of the reference's reader (pinned to the reference CLI by
test_fastq_text_cases.py), field by field and byte by byte, on the texts of
fastq_text_cases: the record table (fqz5_fastq_index, fqz5_fastq_index_any),
the record ends, the gathered sections with lengths and READ2 flags, the
names' delimiter search across a tile, and the refusals.  Raw ctypes calls on
torch device tensors, at aligned and unaligned device pointers.

The fuzz counts (FUZZ in fastq_text_cases) are what fits in about three seconds
a layout on an MI355X."""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

import fastq_text_cases as T
import kseq_ref as K
from fqzcomp5_amd import fqz5file as Z
from fqzcomp5_amd import lib

pytestmark = pytest.mark.gpu

REC = np.dtype([("name", "<u8"), ("comment", "<u8"), ("seq", "<u8"), ("qual", "<u8"),
                ("name_len", "<u4"), ("comment_len", "<u4"), ("seq_len", "<u4"), ("fasta", "<u4"),
                ("end", "<u8")])
FILL = 0xA5
GUARD = 64


@pytest.fixture(scope="module", autouse=True)
def _need():
    if not lib.device_ok():
        pytest.fail("no GPU: " + lib.last_error())
    assert REC.itemsize == C.sizeof(Z.FastqRec)


def _dev(text: bytes, off: int = 0):
    """The text in device memory, `off` bytes past an aligned allocation:
    (the tensor that owns it, the device pointer)."""
    buf = torch.full((len(text) + off + 32,), 0x0a, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    if text:
        buf[off:off + len(text)] = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()
    return buf, buf.data_ptr() + off


def _index(fn, text: bytes, off: int = 0, max_rec: int = None, dev=None):
    """(return value, records as a structured array, h_rec_size, the record
    table on the device, the text on the device)."""
    so = Z._load()
    dev = dev or _dev(text, off)
    if max_rec is None:
        max_rec = text.count(b"\n") + 2
    recs = torch.full(((max_rec + 1) * REC.itemsize,), FILL, dtype=torch.uint8, device="cuda")
    rsz = np.full(max_rec + 1, 0xA5A5A5A5, np.uint32)
    nrec = C.c_uint64(0)
    lib.after_torch()
    rc = getattr(so, fn)(dev[1], len(text), recs.data_ptr(), max_rec, C.byref(nrec), rsz.ctypes.data)
    n = int(nrec.value)
    if rc < 0:
        return rc, None, None, recs, dev
    host = recs.cpu().numpy()
    assert n <= max_rec
    assert (host[max_rec * REC.itemsize:] == FILL).all(), "records written past max_rec"
    assert (rsz[max_rec:] == 0xA5A5A5A5).all(), "sizes written past max_rec"
    return rc, host[:n * REC.itemsize].view(REC), rsz[:n], recs, dev


def _same_table(what, rc, got, rsz, text):
    """The record count, the return value, every field of every record and
    h_rec_size against the model: the first differing record and field."""
    want_rc, want, sizes = K.fields(text)
    assert rc == want_rc, f"{what}: returned {rc} ({lib.last_error() if rc < 0 else ''}), the model {want_rc}"
    for r in range(min(len(got), len(want))):
        for f in K.FIELDS:
            assert int(got[f][r]) == want[r][f], \
                f"{what}: record {r} field {f}: {int(got[f][r])}, the model {want[r][f]}"
        assert int(rsz[r]) == sizes[r], f"{what}: record {r} h_rec_size: {int(rsz[r])}, the model {sizes[r]}"
    assert len(got) == len(want), f"{what}: {len(got)} records, the model {len(want)}"
    return want


def _offsets_for(name):
    return T.PTR_OFFSETS if name in T.TILES else (0, 15)


# ----------------------------------------------------------------------------
# index
# ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.MUST_EQUAL))
def test_index(name):
    text = T.MUST_EQUAL[name]
    for off in _offsets_for(name):
        fns = ["fqz5_fastq_index_any"] + (["fqz5_fastq_index"] if T.LAYOUT[name] != "ml" else [])
        for fn in fns:
            rc, got, rsz, _, _ = _index(fn, text, off)
            _same_table(f"{name} {fn} pointer+{off}", rc, got, rsz, text)
            if name in T.TILES:
                # every newline of the text, from the fields alone
                nl = np.stack([got["seq"] - 1, got["seq"] + got["seq_len"], got["qual"] - 1,
                               got["end"] - 1], axis=1).reshape(-1)
                want = np.asarray(T.tile_newlines(text), np.uint64)
                assert len(nl) == len(want)
                bad = np.flatnonzero(nl != want)
                assert not len(bad), f"{name} pointer+{off}: newline {bad[0]} at {want[bad[0]]} read as {nl[bad[0]]}"


def test_index_ml_refused_by_index():
    # fqz5_fastq_index itself takes 4-line FASTQ and FASTA only
    for name in ("ml_wrap_63_lf", "ml_skipped", "ml_four_empty_tail"):
        rc, *_ = _index("fqz5_fastq_index", T.MUST_EQUAL[name])
        assert rc == -1 and lib.last_error(), name


@pytest.mark.parametrize("lay", list(T.FUZZ))
def test_fuzz(lay):
    """Index, gather and (FASTQ) record ends of every fuzz text."""
    t0 = time.perf_counter()
    texts = T.fuzz_texts(lay)
    for k, text in enumerate(texts):
        off = (0, 1, 8, 15)[k % 4]
        what = f"{lay} fuzz {k} {text!r}"
        rc, got, rsz, recs_d, dev = _index("fqz5_fastq_index_any", text, off)
        _same_table(what, rc, got, rsz, text)
        if K.layout(text) != 2:
            rc, got, rsz, _, _ = _index("fqz5_fastq_index", text, off, dev=dev)
            _same_table(what + " (index)", rc, got, rsz, text)
        mrecs, _ = K.read_all(text)
        _gather_same(what, dev, recs_d, mrecs, 0, len(mrecs), rc == 1)
        if lay != "fa":
            for eof in (0, 1):
                _ends_same(what, text, eof, dev)
    print(f"\n{lay}: {len(texts)} fuzz texts in {time.perf_counter() - t0:.2f} s")


# ----------------------------------------------------------------------------
# record ends
# ----------------------------------------------------------------------------
def _ends(text: bytes, eof: int, dev=None, max_ends: int = None):
    so = Z._load()
    dev = dev or _dev(text)
    cap = text.count(b"\n") + 3 if max_ends is None else max_ends
    out = np.full(cap + 1, 0xA5A5A5A5A5A5A5A5, np.uint64)
    n = C.c_uint64(0)
    lib.after_torch()
    rc = so.fqz5_fastq_record_ends(dev[1], len(text), eof, out.ctypes.data, cap, C.byref(n))
    if rc < 0:
        return None
    assert (out[int(n.value):] == 0xA5A5A5A5A5A5A5A5).all()
    return [int(x) for x in out[:int(n.value)]]


def _ends_same(what, text, eof, dev=None):
    got, want = _ends(text, eof, dev), K.ends(text, bool(eof))
    assert got == want, f"{what}: record ends with eof={eof}: {got} ({lib.last_error() if got is None else ''}), " \
                        f"the model {want}"
    return got


@pytest.mark.parametrize("name", [n for n in T.MUST_EQUAL if T.LAYOUT[n] != "fa"])
def test_record_ends(name):
    text = T.MUST_EQUAL[name]
    _, fields, _ = K.fields(text)
    for eof in (0, 1):
        got = _ends_same(name, text, eof)
        if T.LAYOUT[name] == "fq4":          # the ends are the records' end fields
            assert got[:len(fields)] == [F["end"] for F in fields][:len(got)]
            assert len(got) >= len(fields) - (0 if eof else 1)
    if len(text) > T.SHORT:
        return
    # the text cut at every byte of its last two records
    first = fields[-2]["name"] - 1 if len(fields) > 1 else 0
    for cut in range(first, len(text)):
        dev = _dev(text[:cut])
        for eof in (0, 1):
            _ends_same(f"{name} cut at {cut} {text[:cut]!r}", text[:cut], eof, dev)


def test_record_ends_not_fastq():
    for name in ("fa_lines_lf", "fa_bare_gt_last"):
        assert _ends(T.MUST_EQUAL[name], 1) is None and lib.last_error()
    text = T.MUST_EQUAL["fq4_flags"]
    assert _ends(text, 1, max_ends=7) is None and "max_ends" in lib.last_error()
    assert len(_ends(text, 1, max_ends=8)) == 8


# ----------------------------------------------------------------------------
# gather
# ----------------------------------------------------------------------------
def _gather(dev, recs_d, a, b, names_cap, seq_cap, with_names=True, with_qual=True, host=True):
    """(return value, names, bases, qualities, h_len, h_flag, sizes): the
    buffers whole, pre-filled, GUARD bytes longer than the capacity."""
    so = Z._load()
    n = max(b - a, 0)
    bufs = [torch.full((cap + GUARD,), FILL, dtype=torch.uint8, device="cuda") for cap in
            (names_cap, seq_cap, seq_cap)]
    hl = np.full(n + 2, 0xA5A5A5A5, np.uint32)
    hf = np.full(n + 2, 0xA5A5A5A5, np.uint32)
    sizes = (C.c_uint64 * 4)(7, 7, 7, 0xA5)
    lib.after_torch()
    rc = so.fqz5_fastq_gather(dev[1], recs_d.data_ptr(), a, b,
                              bufs[0].data_ptr() if with_names else None,
                              bufs[1].data_ptr() if with_names else None,
                              bufs[2].data_ptr() if with_qual else None,
                              hl.ctypes.data if host else None, hf.ctypes.data if host else None, sizes)
    assert sizes[3] == 0xA5
    return rc, [x.cpu().numpy().tobytes() for x in bufs], hl, hf, list(sizes)[:3]


def _gather_same(what, dev, recs_d, mrecs, a, b, fasta):
    names, seq, qual, lens, flags = K.block(mrecs[a:b])
    want_sizes = [len(names), len(seq), 0 if fasta else len(seq)]
    what = f"{what} gather [{a}, {b})"
    rc, bufs, hl, hf, sizes = _gather(dev, recs_d, a, b, len(names), len(seq), with_qual=not fasta)
    assert rc == 0, f"{what}: {lib.last_error()}"
    assert sizes == want_sizes, f"{what}: sizes {sizes}, the model {want_sizes}"
    n = b - a
    for r in range(n):
        assert int(hl[r]) == lens[r], f"{what}: record {a + r} h_len {int(hl[r])}, the model {lens[r]}"
        assert int(hf[r]) == flags[r], f"{what}: record {a + r} h_flag {int(hf[r])}, the model {flags[r]}"
    assert (hl[n:] == 0xA5A5A5A5).all() and (hf[n:] == 0xA5A5A5A5).all()
    for label, got, want in (("names", bufs[0], names), ("bases", bufs[1], seq),
                             ("qualities - 33", bufs[2], b"" if fasta else qual)):
        if got[:len(want)] != want:
            at = next(i for i in range(len(want)) if got[i] != want[i])
            raise AssertionError(f"{what}: {label} byte {at}: {got[at]}, the model {want[at]} "
                                 f"({got[max(at - 8, 0):at + 8]!r} / {want[max(at - 8, 0):at + 8]!r})")
        assert got[len(want):] == bytes([FILL]) * (len(got) - len(want)), \
            f"{what}: {label}: bytes written past the section"
    return want_sizes


@pytest.mark.parametrize("name", [n for n in T.MUST_EQUAL if n not in T.TILES or n == "tile_dense"])
def test_gather(name):
    text = T.MUST_EQUAL[name]
    mrecs, _ = K.read_all(text)
    n = len(mrecs)
    for off in (0, 15):
        rc, got, _, recs_d, dev = _index("fqz5_fastq_index_any", text, off)
        assert rc >= 0 and len(got) == n
        fasta = rc == 1
        ranges = [(0, n)] + ([(n // 2, n), (1, n - 1)] if n > 1 else [])
        for a, b in ranges:
            want_sizes = _gather_same(f"{name} pointer+{off}", dev, recs_d, mrecs, a, b, fasta)
            # the sizes-only call: d_names NULL, nothing else is written
            rc, bufs, hl, hf, sizes = _gather(dev, recs_d, a, b, 8, 8, with_names=False, with_qual=not fasta)
            assert rc == 0 and sizes == want_sizes
            assert all(x == bytes([FILL]) * len(x) for x in bufs)
            assert (hl == 0xA5A5A5A5).all() and (hf == 0xA5A5A5A5).all()
        # a == b: an empty block
        for a in (0, n // 2, n):
            rc, bufs, hl, hf, sizes = _gather(dev, recs_d, a, a, 8, 8, with_qual=not fasta)
            assert rc == 0 and sizes == [0, 0, 0]
            assert all(x == bytes([FILL]) * len(x) for x in bufs)


def test_gather_flags():
    text = T.FLAGS_TEXT
    mrecs, _ = K.read_all(text)
    rc, got, _, recs_d, dev = _index("fqz5_fastq_index_any", text)
    assert rc == 0 and len(got) == len(T.FLAGS_WANT)
    _, _, _, hf, _ = _gather(dev, recs_d, 0, len(got), 256, 64)
    assert tuple(int(x) for x in hf[:len(got)]) == T.FLAGS_WANT
    # a record equal to record a - 1 that is first in the range is not flagged
    a = T.FLAGS_REPEAT
    assert mrecs[a].name_bytes == mrecs[a - 1].name_bytes and T.FLAGS_WANT[a] == 128
    _, _, _, hf, _ = _gather(dev, recs_d, a, len(got), 256, 64)
    assert tuple(int(x) for x in hf[:len(got) - a]) == (0,) + T.FLAGS_WANT[a + 1:]
    _gather_same("flags", dev, recs_d, mrecs, a, len(got), False)


# ----------------------------------------------------------------------------
# names over a tile: find_delims looks for '\0' across a tile edge
# ----------------------------------------------------------------------------
@functools.lru_cache(None)
def _section():
    """About 70 KB of names (with a run of empty ones, many '\\0' in a 16-byte
    group, around the tile edge), a few bases and qualities each."""
    rng = np.random.default_rng(170)
    names, seqs, quals = [], [], []
    total = 0
    while total < 70_000:
        k = len(names)
        # lengths 0..40, and a run of empty names (many '\0' in a 16-byte group) at the tile edge
        n = 0 if T.TILE - 200 < total < T.TILE + 200 and k % 3 else int(rng.integers(0, 41))
        names.append(bytes(rng.choice(np.frombuffer(b"abcXYZ:/ 12", np.uint8), n)))
        L = int(rng.integers(0, 5))
        seqs.append(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), L)))
        quals.append(bytes(rng.integers(0, 41, L).astype(np.uint8)))
        total += n + 1
    return names, seqs, quals


@pytest.mark.parametrize("off", T.PTR_OFFSETS)
@pytest.mark.parametrize("fastq,plus_name", [(True, False), (True, True), (False, False)])
def test_format_names_over_a_tile(off, fastq, plus_name):
    so = Z._load()
    names, seqs, quals = _section()
    sect = b"".join(x + b"\0" for x in names)
    assert len(sect) > T.TILE + 4000
    want = b"".join((b"@" + nm + b"\n" + s + b"\n+" + (nm if plus_name else b"") + b"\n"
                     + bytes(q + 33 for q in ql) + b"\n") if fastq else (b">" + nm + b"\n" + s + b"\n")
                    for nm, s, ql in zip(names, seqs, quals))
    d_names = _dev(sect, off)
    d_seq, d_qual = _dev(b"".join(seqs), 3), _dev(b"".join(quals), 5)
    lens = np.asarray([len(s) for s in seqs], np.uint32)
    out = torch.full((len(want) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    size0, size = C.c_uint64(0), C.c_uint64(0)
    lib.after_torch()
    args = (d_names[1], len(sect), d_seq[1], d_qual[1] if fastq else None, lens.ctypes.data, len(names),
            int(plus_name))
    assert so.fqz5_fastq_format(*args, None, 0, C.byref(size0)) == 0, lib.last_error()
    assert so.fqz5_fastq_format(*args, out.data_ptr(), len(want), C.byref(size)) == 0, lib.last_error()
    assert size0.value == size.value == len(want)
    host = out.cpu().numpy().tobytes()
    if host[:len(want)] != want:
        at = next(i for i in range(len(want)) if host[i] != want[i])
        raise AssertionError(f"text byte {at} (record {want[:at].count(b'@' if fastq else b'>') - 1}): "
                             f"{host[max(at - 20, 0):at + 20]!r} / {want[max(at - 20, 0):at + 20]!r}")
    assert host[len(want):] == bytes([FILL]) * GUARD
    # one terminator too few: refused
    assert so.fqz5_fastq_format(d_names[1], len(sect) - 1, *args[2:], None, 0, C.byref(size0)) == -1
    assert "fewer names" in lib.last_error()


# ----------------------------------------------------------------------------
# refusals
# ----------------------------------------------------------------------------
def _valid_after():
    """A valid call straight after a refusal succeeds."""
    text = T.MUST_EQUAL["fq4_crlf"]
    rc, got, rsz, _, _ = _index("fqz5_fastq_index_any", text)
    _same_table("a valid call after a refusal", rc, got, rsz, text)


@pytest.mark.parametrize("case", T.REFUSALS, ids=[r[0] for r in T.REFUSALS])
def test_refusals(case):
    name, text, api, code, reason = case
    rc, *_ = _index("fqz5_fastq_index", text)
    assert rc == -1 and lib.last_error(), f"{name}: fqz5_fastq_index took it ({reason})"
    _valid_after()
    rc, got, rsz, _, _ = _index("fqz5_fastq_index_any", text)
    if api == "index":
        _same_table(name, rc, got, rsz, text)
        return
    assert rc == -1 and lib.last_error(), f"{name}: fqz5_fastq_index_any took it ({reason})"
    _valid_after()
    if text[:1] != b">":
        assert _ends(text, 1) is None and lib.last_error(), name
        _valid_after()


def _number(msg: str, word: str) -> int:
    tail = msg.split(word + " ", 1)[1]
    return int(tail.split()[0])


def test_refusals_name_the_first_bad_one():
    ok = b"@r c\nACGT\n+\nIIII\n"
    bad = b"@bad\nACGT\n+\nIII\n"                    # qualities too short: in both layouts' eyes
    recs = [ok] * 400
    recs[5] = recs[300] = bad                          # (in different workgroups of k_fq_records)
    text = b"".join(recs)
    for fn in ("fqz5_fastq_index", "fqz5_fastq_index_any"):
        rc, *_ = _index(fn, text)
        assert rc == -1 and _number(lib.last_error(), "record") == 5, (fn, lib.last_error())
    _valid_after()
    # FASTA: the first line that starts a FASTQ record
    lines = [b">h%d" % k if k % 2 == 0 else b"ACGT" for k in range(700)]
    lines[11] = lines[601] = b"@CGT"
    rc, *_ = _index("fqz5_fastq_index_any", b"\n".join(lines) + b"\n")
    assert rc == -1 and _number(lib.last_error(), "line") == 11, lib.last_error()
    _valid_after()
    # wrapped: the first record kseq does not read as one
    wr = [b"@w%d\nAC\nGT\n+\nII\nII\n" % k for k in range(400)]
    wr[5] = wr[300] = b"@w\nAC\nGT\n+\nII\nIII\n"
    rc, *_ = _index("fqz5_fastq_index_any", b"".join(wr))
    assert rc == -1 and _number(lib.last_error(), "record") == 5, lib.last_error()
    _valid_after()


def test_max_rec_one_too_small():
    for name in ("fq4_flags", "fa_header_only", "ml_qual_starts"):
        text = T.MUST_EQUAL[name]
        n = len(K.read_all(text)[0])
        rc, got, rsz, _, _ = _index("fqz5_fastq_index_any", text, max_rec=n)
        _same_table(name, rc, got, rsz, text)
        rc, _, _, recs_d, _ = _index("fqz5_fastq_index_any", text, max_rec=n - 1)
        assert rc == -1 and "max_rec" in lib.last_error(), name
        assert (recs_d.cpu().numpy() == FILL).all(), f"{name}: records written by a refused call"
        _valid_after()
