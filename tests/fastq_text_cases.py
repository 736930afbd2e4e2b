"""Seeded FASTQ / FASTA texts for the tests of fastq.hip against kseq_ref:
every text here is small (most under 200 bytes; the delimiter-tile texts are
two or three 64 KiB tiles) and deterministic.

MUST_EQUAL   name -> text the reference reads and fastq.hip must read the same
             way, field by field.  tests/golden/make_golden_fastq_text.py codes
             each with the reference CLI and asserts that it took it.
LAYOUT       name -> "fq4" (4-line FASTQ), "fa" (FASTA) or "ml" (wrapped)
TILES        the names of the delimiter-tile texts (every newline position is
             known by construction: tile_newlines())
FUZZ         layout -> (seed, count): fuzz_texts(layout) draws them
REFUSALS     the closed list of texts fastq.hip refuses, each with its reason
"""
import numpy as np

from wrapped_cases import wrap

TILE = 65536                 # FQ_TILE of fastq.hip
PTR_OFFSETS = (0, 1, 8, 15)  # device pointer offsets from an aligned allocation


# --------------------------------------------------------------------------
# delimiter tiles: 4-line FASTQ whose newline positions are known
# --------------------------------------------------------------------------
def _fill(rng, n: int, alpha: bytes) -> bytes:
    return bytes(rng.choice(np.frombuffer(alpha, np.uint8), n)) if n else b""


def _rec4(rng, name: bytes, n: int) -> bytes:
    return b"@" + name + b"\n" + _fill(rng, n, b"ACGT") + b"\n+\n" + _fill(rng, n, b"#5AFJ") + b"\n"


def _tile_total(total: int, seed: int) -> bytes:
    """4-line records of about 100 bases, the last sized so that the text is
    exactly `total` bytes."""
    rng = np.random.default_rng(seed)
    out, at, r = [], 0, 0
    while total - at > 600:
        rec = _rec4(rng, b"t%d" % r, int(rng.integers(60, 140)))
        out.append(rec)
        at += len(rec)
        r += 1
    left = total - at                       # "@z\n" n "\n+\n" n "\n" = 7 + 2n, "@zz": 8 + 2n
    name = b"z" if left % 2 else b"zz"
    out.append(_rec4(rng, name, (left - 6 - len(name)) // 2))
    text = b"".join(out)
    assert len(text) == total
    return text


def _tile_edge(nl_at: int, seed: int) -> bytes:
    """One record whose sequence line's '\n' is byte `nl_at`."""
    return _rec4(np.random.default_rng(seed), b"e", nl_at - 3)


def _tile_bare(seed: int) -> bytes:
    """Short records up to just before a tile edge, then one record whose
    sequence line covers the whole of tile 1: a tile without a newline."""
    rng = np.random.default_rng(seed)
    out, at = [], 0
    while at < TILE - 400:
        out.append(_rec4(rng, b"b%d" % len(out), 100))
        at += len(out[-1])
    out.append(_rec4(rng, b"long", 2 * TILE - at))
    return b"".join(out)


def _tile_dense(seed: int) -> bytes:
    """A region where every record is "@\\n\\n+\\n\\n" (16-byte groups with
    many delimiters) across the first tile edge, ordinary records around it."""
    rng = np.random.default_rng(seed)
    head = b"".join(_rec4(rng, b"d%d" % k, 70) for k in range(420))
    assert TILE - 3000 < len(head) < TILE - 100          # (the region crosses the tile edge)
    return head + b"@\n\n+\n\n" * 700 + _rec4(rng, b"tail", 33)


def _tiles() -> dict:
    out = {"tile_len_%d" % n: _tile_total(n, 100 + k)
           for k, n in enumerate((4095, 4096, 4097, 65535, 65536, 65537, 131073))}
    out["tile_nl_last_byte"] = _tile_edge(TILE - 1, 120)
    out["tile_nl_first_byte"] = _tile_edge(TILE, 121)
    out["tile_no_newline"] = _tile_bare(122)
    out["tile_dense"] = _tile_dense(123)
    return out


def tile_newlines(text: bytes):
    """The newline positions of a 4-line text from the lengths of its lines."""
    out, at = [], -1
    for line in text.split(b"\n")[:-1]:
        at += len(line) + 1
        out.append(at)
    return out


# --------------------------------------------------------------------------
# 4-line edges
# --------------------------------------------------------------------------
def _fq4() -> dict:
    ok = b"@ok c\nACGT\n+\nIIII\n"
    out = {}
    for c in (9, 11, 12, 13, 32):
        out["fq4_name_end_%d" % c] = b"@nm" + bytes([c]) + b"cm x\nACGT\n+\nI5I5\n" + ok
    out["fq4_empty_name"] = ok + b"@\nAC\n+\nII\n" + ok
    out["fq4_at_space_x"] = ok + b"@ x\nAC\n+\nII\n"
    out["fq4_two_spaces"] = b"@n  c d\nACG\n+\nIII\n" + ok
    out["fq4_tab_comment"] = b"@n\tc\td\nACG\n+\nIII\n" + ok
    out["fq4_comment_lone_cr"] = b"@n \r\nACG\n+\nIII\n" + ok
    out["fq4_name_cr_cr"] = b"@n\r\r\nACG\n+\nIII\n" + ok
    out["fq4_crlf"] = b"@a c\r\nACGT\r\n+\r\nIIII\r\n@b\r\nAC\r\n+b\r\n5I\r\n"
    out["fq4_lone_cr_seq_qual"] = ok + b"@r\n\r\n+\n\r\n" + ok
    out["fq4_empty_seq_qual"] = ok + b"@e\n\n+\n\n" + ok
    out["fq4_empty_first"] = b"@e\n\n+\n\n" + ok
    out["fq4_no_final_nl"] = ok + b"@l\nACG\n+\nI5I"
    out["fq4_no_final_nl_cr"] = ok + b"@l\nACG\r\n+\r\nI5I\r"
    for k in (1, 2, 3):
        out["fq4_trailing_%d" % k] = ok + b"@t\nAC\n+\n5I\n" + b"\n" * k
    out["fq4_qual_starts"] = b"@q1\nACG\n+\n@II\n@q2\nACG\n+\n+II\n@q3\nACG\n+\n>II\n"
    out["fq4_seq_has_marks"] = b"@q1\nA@>+\n+\nIIII\n@q2 @ > +\nAC\n+@q2\nII\n"
    out["fq4_flags"] = FLAGS_TEXT
    out["fq4_copy_lens"] = _copy_lens("fq4", 160)
    return out


# READ2 flags (fqzcomp5.c:518-527), in this order: name "ab" with comment
# "c/2" is flagged; name "a" with comment "/2" is not (name.l > 1); name "/2"
# is; a first "x" is not, the "x" after it is (equal names), and is not when a
# block starts at it (FLAGS_REPEAT); equal lengths with different bytes are not
FLAGS_TEXT = b"".join(b"@" + h + b"\nAC\n+\nII\n" for h in
                      (b"ab c/2", b"a /2", b"/2", b"x", b"x", b"xa 1", b"xb 1", b"xb 1"))
FLAGS_WANT = (128, 0, 128, 0, 128, 0, 0, 128)
FLAGS_REPEAT = 4
COPY_LENS = (0, 1, 63, 64, 65, 129)      # around the 64-lane copy loops of k_fq_gather


def _copy_lens(lay: str, seed: int) -> bytes:
    """Names, comments and sequences of every length in COPY_LENS."""
    rng = np.random.default_rng(seed)
    out = []
    for k, n in enumerate(COPY_LENS):
        for part in range(3):
            ln = [3, 2, 5]
            ln[part] = n
            name, com, seq = _fill(rng, ln[0], b"abc:/12"), _fill(rng, ln[1], b"xyz 12"), _fill(rng, ln[2], b"ACGT")
            if com[:1] == b" " or com[-1:] == b" ":
                com = b"c" + com[1:-1] + b"c" if len(com) > 1 else b"c"
            head = name + (b" " + com if com else b"")
            if lay == "fa":
                out.append(b">" + head + b"\n" + seq + b"\n")
            elif lay == "fq4":
                out.append(b"@" + head + b"\n" + seq + b"\n+\n" + _fill(rng, len(seq), b"#5AFJ") + b"\n")
            else:
                out.append(b"@" + head + b"\n" + wrap(seq, 50) + b"+\n" + wrap(_fill(rng, len(seq), b"#5AFJ"), 50))
    return b"".join(out)


# --------------------------------------------------------------------------
# FASTA edges
# --------------------------------------------------------------------------
FA_LENS = (0, 1, 63, 64, 65, 127, 128, 129)


def _fa_lines(nl: bytes, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    out = []
    for n in FA_LENS:                       # the line alone, then followed by a second line
        a, b = _fill(rng, n, b"ACGT"), _fill(rng, n, b"ACGTN")
        out.append(b">s%d" % n + nl + a + nl)
        out.append(b">d%d x" % n + nl + a + nl + b + nl + b"GG" + nl)
    return b"".join(out)


def _fa() -> dict:
    out = {"fa_lines_lf": _fa_lines(b"\n", 130), "fa_lines_crlf": _fa_lines(b"\r\n", 131)}
    out["fa_empty_lines"] = b">a\n\n\nAC\n\n\nGT\n\n>b\n\nA\n\n\n"
    out["fa_header_only"] = b">h1\n>h2 c\n>h3\nAC\n>h4\n"
    out["fa_lone_cr_first"] = b">a\n\r\nACG\n>b\nAC\n\r\nGT\n\r\n>c\n\n\r\n\r\nA\n"
    out["fa_cr_cr"] = b">a\n\r\r\nAC\n>b\nAC\r\r\nGT\n"
    out["fa_cr_mid_line"] = b">a\nA\rC\nG\rT\r\n>b\n\rA\n"
    out["fa_crlf"] = b">a c\r\nACGT\r\nAC\r\n\r\nGG\r\n>b\r\n>c\r\nA\r\n"
    out["fa_no_final_nl_x_cr"] = b">a\nAC\nX\r"
    out["fa_no_final_nl"] = b">a\nAC\n>b\nGT"
    out["fa_last_lone_cr"] = b">a y\nATCTC\n>:\r\nAG\r\n\r"
    out["fa_last_lone_cr_only"] = b">a\nAC\n>b\n\r"
    out["fa_bare_gt_last"] = b">1a\nAC\n> x\nGG\n>"
    out["fa_bare_gt_only_after_header"] = b">1a\n>"
    out["fa_gt_in_line"] = b">a\nAC>GT\nA>\n>b\nG@+\n"
    out["fa_header_no_nl"] = b">a\nAC\n>last c"
    out["fa_copy_lens"] = _copy_lens("fa", 161)
    return out


# --------------------------------------------------------------------------
# wrapped edges
# --------------------------------------------------------------------------
def _ml_wrap(width: int, nl: bytes, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    out = []
    for r, n in enumerate((width, width + 1, 2 * width, 2 * width + 1, 129, 1)):
        out.append(b"@w%d c" % r + nl + wrap(_fill(rng, n, b"ACGTN"), width, nl) + b"+" + nl
                   + wrap(_fill(rng, n, b"#5AFJ"), width, nl))
    return b"".join(out)


def _ml_lonecr(seed: int) -> bytes:
    """The kept lone-'\\r' forms of wrapped_cases.lonecr at 1 to 130 bases."""
    rng = np.random.default_rng(seed)
    out = []
    r = 0
    for n in (1, 2, 63, 64, 65, 66, 129, 130):
        for kind in range(6):
            seq, qual = _fill(rng, n, b"ACGTN"), _fill(rng, n, b"#,:FIJ")
            nl = b"\r\n" if r % 4 == 3 else b"\n"
            head = b"@cr%d" % r + nl
            if kind == 0:
                sq, qq = b"\r\n" + wrap(seq[1:], 60, nl), b"\r\n" + wrap(qual[1:], 60, nl)
            elif kind == 1:
                sq, qq = wrap(seq, 60, nl), b"\r\n" + wrap(qual[1:], 60, nl)
            elif kind == 2:
                sq, qq = b"\n\n\r\n" + wrap(seq[1:], 60, nl), wrap(qual, 60, nl)
            elif kind == 3:
                sq, qq = b"\r\n\r\n" + wrap(seq[1:], 60, nl), b"\n\r\n\r\n" + wrap(qual[1:], 60, nl)
            elif kind == 4:
                sq, qq = wrap(seq, 60, nl), wrap(qual, 60, nl)
            else:
                sq, qq = wrap(seq, 60, nl) + b"\r\n", wrap(qual, 60, nl) + b"\r\n"
            if n == 1 and kind in (0, 3):
                sq, qq = b"\r\n", b"\r\n"
            if n == 1 and kind in (1, 2):        # (wrap(b"") is an empty line: drop it)
                sq = b"\n\n\r\n" if kind == 2 else sq
                qq = b"\r\n" if kind == 1 else qq
            out.append(head + sq + b"+" + nl + qq)
            r += 1
    return b"".join(out)


def _ml() -> dict:
    out = {}
    for w in (1, 63, 64, 65):
        out["ml_wrap_%d_lf" % w] = _ml_wrap(w, b"\n", 140 + w)
        out["ml_wrap_%d_crlf" % w] = _ml_wrap(w, b"\r\n", 240 + w)
    out["ml_qual_starts"] = b"@a\nAC\nGT\n+\n@I\n+I\n@b\nACG\nT\n+\n+\n@I5\n"
    out["ml_empty_lines"] = b"@a\n\nAC\n\nGT\n\n+\nII\n\nI\n\nI\n@b\nA\nC\n+\n\nI\n\n\nI\n"
    out["ml_lonecr"] = _ml_lonecr(150)
    out["ml_skipped"] = (b"# text first\n\nmore\r\n+ plus\n@a\nAC\nGT\n+\nII\nII\njunk\n\n+\n\r\n"
                         b"@b\nA\n+\nI\n@c\nAC\nG\n+\nIII\ntrailing text\n\r\n\n")
    out["ml_mixed_4line"] = b"@a\nACGT\n+\nIIII\n@b\nAC\nGT\n+\nII\nII\n@c x\nAC\n+\nII\n"
    out["ml_no_final_nl"] = b"@a\nAC\nGT\n+\nIII\nI"
    out["ml_four_empty_tail"] = b"@a\nAC\n+\nII\n\n\n\n\n"
    out["ml_copy_lens"] = _copy_lens("ml", 162)
    return out


# --------------------------------------------------------------------------
# the seeded grammar fuzz: at most 6 records per text, small alphabets that
# include '\r', '@', '+', '>', space and tab; the refused classes below are
# left out by construction
# --------------------------------------------------------------------------
# counts: what index, gather and record ends of every text take about three
# seconds for on an MI355X, the model's own time included (measured: 2800
# 4-line texts in 2.91 s, 4000 FASTA texts in 2.78 s, 2000 wrapped texts in
# 2.74 s)
FUZZ = {"fq4": (1001, 2800), "fa": (1002, 4000), "ml": (1003, 2000)}
_MARK = b"@+>"


def _pick(rng, alpha: bytes, lo: int, hi: int) -> bytes:
    return _fill(rng, int(rng.integers(lo, hi + 1)), alpha)


def _header(rng, first: bytes, nl: bytes) -> bytes:
    h = first + _pick(rng, b"ab/2:@+>", 0, 3)
    if rng.integers(0, 3):
        h += _pick(rng, b" \t\r\v\f", 1, 2) + _pick(rng, b"c/2 \t\r@+>", 0, 4)
    return h + nl


def _body(rng, alpha: bytes, n: int, first_free: bool) -> bytes:
    """n bytes of `alpha`; the first is none of '@', '+', '>' unless
    first_free, and the last is no '\\r' (the line end decides about that)."""
    b = bytearray(_fill(rng, n, alpha))
    if n and not first_free and b[0] in _MARK:
        b[0] = 65
    if n and b[-1] == 13:
        b[-1] = 67
    return bytes(b)


def _fuzz_fq4(rng) -> bytes:
    out = []
    nrec = int(rng.integers(1, 7))
    for r in range(nrec):
        nl = b"\r\n" if rng.integers(0, 4) == 0 else b"\n"
        n = int(rng.integers(0, 6))
        s = _body(rng, b"ACGTN\r@+> ", n, False)
        q = _body(rng, b"!5I~@+>\r ", n, True)
        if n == 0:
            # an empty line; or a lone '\r' on both (kept: one base, one quality)
            sl = ql = b"\r\n" if rng.integers(0, 4) == 0 else b"\n"
        else:
            sl, ql = s + nl, q + nl
        out.append(_header(rng, b"@", nl) + sl + b"+" + _pick(rng, b"ab@ ", 0, 2) + nl + ql)
    text = b"".join(out)
    tail = int(rng.integers(0, 6))
    if tail <= 3:
        return text + b"\n" * tail
    if tail == 4 and not text.endswith(b"\n\n") and not text.endswith(b"+\n\r\n"):
        return text[:-1]                                 # no final '\n'
    return text


def _fuzz_fa(rng) -> bytes:
    out = []
    nrec = int(rng.integers(1, 7))
    for r in range(nrec):
        nl = b"\r\n" if rng.integers(0, 4) == 0 else b"\n"
        out.append(_header(rng, b">", nl))
        for _ in range(int(rng.integers(0, 5))):
            k = int(rng.integers(0, 8))
            if k == 0:
                out.append(b"\n")
            elif k == 1:
                out.append(b"\r\n")
            elif k == 2:
                out.append(_body(rng, b"ACGT\r> @+N", int(rng.integers(1, 4)), False) + b"\r\r\n")
            else:
                out.append(_body(rng, b"ACGT\r> @+N", int(rng.integers(1, 6)), False) + nl)
    text = b"".join(out)
    tail = int(rng.integers(0, 8))
    if tail == 0:                                        # no final '\n'
        return text[:-1] if len(text) > 2 else text      # (">" alone holds no record at all)
    if tail == 1:
        return text + b">"                               # a bare '>': no record
    if tail == 2:
        return text + b"\r"                              # a lone '\r' at the very end
    if tail == 3:
        return text + b"X\r"
    return text


def _fuzz_lines(rng, payload: bytes, nl: bytes, first_free: bool, lone_cr: bool) -> bytes:
    """`payload` over lines of random widths, empty lines among them; with
    lone_cr the block's first kept byte is a lone-'\\r' line's '\\r'."""
    out = []
    if lone_cr:
        out.append(b"\n" * int(rng.integers(0, 2)) + b"\r\n")
    at = 0
    while at < len(payload):
        w = int(rng.integers(1, 4))
        b = bytearray(payload[at:at + w])
        if not first_free and b[0] in _MARK:
            b[0] = 65
        if b[-1] == 13:
            b[-1] = 67
        out.append(bytes(b) + nl)
        at += w
        if at < len(payload) and rng.integers(0, 5) == 0:
            out.append(b"\r\n" if out and rng.integers(0, 2) else b"\n")
    return b"".join(out)


def _fuzz_junk(rng) -> bytes:
    return b"".join(_pick(rng, b"xy+ \t\r", 0, 3) + b"\n" for _ in range(int(rng.integers(0, 3))))


def _fuzz_ml(rng) -> bytes:
    out = [_fuzz_junk(rng)]
    nrec = int(rng.integers(1, 7))
    for r in range(nrec):
        nl = b"\r\n" if rng.integers(0, 4) == 0 else b"\n"
        n = int(rng.integers(0, 8))
        cs, cq = (int(rng.integers(0, 4)) == 0, int(rng.integers(0, 4)) == 0) if n else (False, False)
        seq = _fuzz_lines(rng, _fill(rng, n - cs, b"ACGTN\r@> "), nl, False, cs)
        qual = _fuzz_lines(rng, _fill(rng, n - cq, b"!5I~@+>\r "), nl, True, cq)
        if n == 0:
            seq, qual = b"\n" * int(rng.integers(0, 3)), b"\n"
        out.append(_header(rng, b"@", nl) + seq + b"+" + _pick(rng, b"ab@ ", 0, 2) + nl + qual)
        out.append(_fuzz_junk(rng))
    text = b"".join(out)
    if rng.integers(0, 4) == 0 and not text.endswith(b"\n\n") and not text.endswith(b"+\n"):
        last = text[:-1].rfind(b"\n") + 1
        if text[last:-1] not in (b"", b"\r"):            # (keep an empty or lone-'\r' last line whole)
            return text[:-1]
    return text


_FUZZERS = {"fq4": _fuzz_fq4, "fa": _fuzz_fa, "ml": _fuzz_ml}


def fuzz_texts(layout: str, count: int = None) -> list:
    seed, n = FUZZ[layout]
    rng = np.random.default_rng(seed)
    return [_FUZZERS[layout](rng) for _ in range(n if count is None else count)]


# --------------------------------------------------------------------------
def _must_equal():
    texts, layout = {}, {}
    for lay, group in (("fq4", _tiles()), ("fq4", _fq4()), ("fa", _fa()), ("ml", _ml())):
        for name, t in group.items():
            assert name not in texts
            texts[name] = t
            layout[name] = lay
    return texts, layout


MUST_EQUAL, LAYOUT = _must_equal()
TILES = tuple(n for n in MUST_EQUAL if n.startswith("tile_"))
N_MUST_EQUAL = 68
SHORT = 400                  # "short" texts: golden keeps their decoded text, record ends are cut

# --------------------------------------------------------------------------
# The closed list of refusals: (name, text, what calls it, kseq's return code
# or None when kseq reads it, reason)
#   api "any": fqz5_fastq_index_any refuses it; "index": fqz5_fastq_index
#   alone does (index_any reads it)
# --------------------------------------------------------------------------
_OK4 = b"@ok c\nACGT\n+\nIIII\n"
REFUSALS = (
    ("kseq_minus2_long_qual", _OK4 + b"@a\nAC\n+\nIII\n", "any", -2,
     "qualities longer than the bases: kseq_read returns -2"),
    ("kseq_minus2_short_qual", _OK4 + b"@a\nACGT\n+\nII\n", "any", -2,
     "qualities shorter than the bases at the end of the text: kseq_read returns -2"),
    ("no_plus_line", _OK4 + b"@a\nACGT\n@b\nAC\n+\nII\n", "any", None,
     "a FASTQ record with no '+' line (kseq returns it without qualities)"),
    ("at_mid_line_in_skipped", _OK4 + b"junk x@y\n" + _OK4, "any", None,
     "'@' in the middle of a line inside skipped bytes: kseq starts a record there"),
    ("gt_mid_line_in_skipped", b"junk x>y\n" + _OK4, "any", None,
     "'>' in the middle of a line inside skipped bytes: kseq starts a record there"),
    ("fasta_line_starts_at", b">a\nAC\n@b\nGT\n", "any", None,
     "a FASTA line that starts with '@' (kseq starts a record there)"),
    ("fasta_line_starts_plus", b">a\nAC\n+\nII\n", "any", None,
     "a FASTA line that starts with '+' (kseq reads qualities after it)"),
    ("stray_lines_after_4line", _OK4 + b"stray\n", "index", None,
     "stray non-empty lines after 4-line records: fqz5_fastq_index alone refuses"),
    ("no_quality_line", _OK4 + b"@e\n\n+\n", "any", None,
     "an empty record that the text ends after its '+' line, with no quality line at all: the "
     "reference reads it (no bases, no qualities), fastq.hip refuses"),
    ("bare_at_last", _OK4 + b"@", "any", None,
     "FASTQ text ending in a bare '@': the reference ignores the '@', fastq.hip refuses"),
)
N_REFUSALS = 10              # and "max_rec one too small", which is a call, not a text
