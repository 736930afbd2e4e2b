"""A plain, byte-level restatement of the reference's FASTQ / FASTA reader,
for the tests of fqzcomp5_amd/csrc/fastq.hip: kseq_read (kseq.h:93-218) over
a bytes object, load_seqs_kseq's per-record rules (fqzcomp5.c:469-527), the
text offsets every record was read from (so that the fields of
fqz5_fastq_rec, include/fqz5_fastq.h, can be stated), fqz5_fastq_record_ends
as its header documents it, and output_fastq / output_fasta
(fqzcomp5.c:3441-3517) of the records read.

One byte at a time, no numpy: the point is to be easy to check against the
reference's source, not to be fast.  kseq's 16 KiB stream buffer is not
modelled: nothing kseq_read returns depends on where a refill falls.
"""
from __future__ import annotations

SPACE = b" \t\n\v\f\r"                      # C isspace()
KEEP_CR_SEQ, KEEP_CR_QUAL = 1 << 8, 1 << 9  # fqz5_fastq_rec.fasta, wrapped records


class Rec:
    """One record kseq_read returned, and where its parts lie in the text."""

    def __init__(self):
        self.hdr = 0              # offset of the '@' / '>'
        self.name = b""           # kseq's name.s, comment.s, seq.s, qual.s
        self.comment = b""
        self.seq = b""
        self.qual = b""
        self.name_off = 0         # first name byte
        self.comment_off = 0      # first comment byte; the header's '\n' without one
        self.seq_off = 0          # the line after the header line
        self.seq_first = None     # first kept sequence byte (None: no bases)
        self.plus = None          # offset of the '+' (None: a record without qualities)
        self.qual_off = None      # the line after the '+' line
        self.stop = 0             # FASTA: the next header's offset or len
        self.end = 0              # after the record's last line, <= len
        self.cr_seq = False       # the first base is a lone-'\r' line's '\r'
        self.cr_qual = False      # the same for the qualities
        self.no_qual_line = False # the text ends after the '+' line

    # load_seqs_kseq (fqzcomp5.c:472, :491-516)
    @property
    def record_size(self) -> int:
        return len(self.name) + 1 + len(self.seq) + len(self.qual)

    @property
    def name_bytes(self) -> bytes:
        return self.name + (b" " + self.comment if self.comment else b"") + b"\0"

    @property
    def qual33(self) -> bytes:
        return bytes((q - 33) & 255 for q in self.qual)


class Kseq:
    """kseq_t over `text`: read() is kseq_read."""

    def __init__(self, text: bytes):
        self.t = text
        self.pos = 0
        self.last_char = 0
        self.hdr = 0
        self.rec = None           # the record of the last read() >= 0
        self.short = False        # the last -2: fewer qualities than bases
        self.bare = False         # the text ends in a bare '@' / '>' (read() returned -1 there)

    def getc(self) -> int:                              # ks_getc (:67-79)
        if self.pos >= len(self.t):
            return -1
        self.pos += 1
        return self.t[self.pos - 1]

    def getuntil(self, delim: str, s: bytearray, append: bool):
        """ks_getuntil2 (:93-144): (return value, the delimiter met or 0)."""
        if not append:
            del s[:]
        if self.pos >= len(self.t):                     # nothing read, end of file (:137):
            return -1, 0                                # before the '\r' strip (:141)
        i = self.pos
        while i < len(self.t):
            if (self.t[i] == 10) if delim == "line" else (self.t[i] in SPACE):
                break
            i += 1
        s += self.t[self.pos:i]
        dret = self.t[i] if i < len(self.t) else 0
        self.pos = min(i + 1, len(self.t))
        if delim == "line" and len(s) > 1 and s[-1] == 13:
            del s[-1]
        return len(s), dret

    def read(self) -> int:                              # kseq_read (:178-218)
        t = self.t
        if self.last_char == 0:                         # jump to the next header line
            while True:
                c = self.getc()
                if c < 0 or c == 62 or c == 64:
                    break
            if c < 0:
                return c
            self.last_char = c
            self.hdr = self.pos - 1
        R = Rec()
        R.hdr = self.hdr
        R.name_off = self.pos
        name, comment, seq, qual = bytearray(), bytearray(), bytearray(), bytearray()
        r, c = self.getuntil("space", name, False)
        if r < 0:
            self.bare = True
            return r
        d = R.name_off + len(name)                      # the delimiter's offset (len at the end)
        R.comment_off = d if d >= len(t) or t[d] == 10 else d + 1
        if c != 10:
            self.getuntil("line", comment, False)
        R.seq_off = self.pos
        while True:
            c = self.getc()
            if c < 0 or c == 62 or c == 43 or c == 64:
                break
            if c == 10:
                continue
            if R.seq_first is None:
                R.seq_first = self.pos - 1
            first = not seq
            seq.append(c)
            at = self.pos
            self.getuntil("line", seq, True)
            if first and c == 13 and self.pos <= at + 1 and t[at:at + 1] != b"\r":
                R.cr_seq = True                         # the line was a lone '\r': kept (:141)
        if c == 62 or c == 64:
            self.last_char = c
            self.hdr = self.pos - 1
        R.stop = self.pos - 1 if c >= 0 else len(t)
        R.name, R.comment, R.seq = bytes(name), bytes(comment), bytes(seq)
        if c != 43:                                     # FASTA
            R.end = R.stop
            self.rec = R
            return len(seq)
        R.plus = self.pos - 1
        while True:                                     # skip the rest of the '+' line
            c = self.getc()
            if c < 0 or c == 10:
                break
        if c == -1:
            self.short = True
            return -2
        R.qual_off = self.pos
        while True:
            at = self.pos
            was = len(qual)
            r, _ = self.getuntil("line", qual, True)
            if r < 0 and at == R.qual_off:
                R.no_qual_line = True
            if r >= 0:
                if was == 0 and bytes(qual) == b"\r" and t[at:at + 2] in (b"\r\n", b"\r"):
                    R.cr_qual = True
            if not (r >= 0 and len(qual) < len(seq)):
                break
        self.last_char = 0
        R.end = self.pos
        R.qual = bytes(qual)
        if len(seq) != len(qual):
            self.short = len(qual) < len(seq)
            return -2
        self.rec = R
        return len(seq)


def read_all(text: bytes):
    """Every record of `text` and kseq_read's last return value (-1: a clean
    end of file, -2: truncated quality string)."""
    ks, recs = Kseq(text), []
    while True:
        r = ks.read()
        if r < 0:
            return recs, r
        recs.append(ks.rec)


def flags(recs) -> list:
    """load_seqs_kseq's READ2 flags (fqzcomp5.c:518-527) of the records of one
    block: the name (with its comment) ends in "/2" and name.l > 1, or equals
    the block's previous name."""
    out, last = [], None
    for R in recs:
        nb = R.name_bytes[:-1]
        f = 0
        if len(R.name) > 1 and nb[-2:] == b"/2":
            f = 128
        if last is not None and nb == last:
            f = 128
        out.append(f)
        last = nb
    return out


def block(recs):
    """One block's section inputs: (names, bases, qualities - 33, lengths,
    READ2 flags)."""
    return (b"".join(R.name_bytes for R in recs), b"".join(R.seq for R in recs),
            b"".join(R.qual33 for R in recs), [len(R.seq) for R in recs], flags(recs))


def render(recs, plus_name: bool = False) -> bytes:
    """What the reference's decoder writes for one block of these records:
    output_fasta when the block's first record has no qualities
    (fqzcomp5.c:575-578), else output_fastq."""
    if not recs:
        return b""
    out = []
    fasta = len(recs[0].qual) == 0
    for R in recs:
        nb = R.name_bytes[:-1]
        if fasta:
            out.append(b">" + nb + b"\n" + R.seq + b"\n")
        else:
            out.append(b"@" + nb + b"\n" + R.seq + b"\n+" + (nb if plus_name else b"") + b"\n"
                       + R.qual + b"\n")
    return b"".join(out)


def _strip(line: bytes) -> bytes:
    return line[:-1] if len(line) > 1 and line[-1] == 13 else line


def four_line_groups(lines) -> bool:
    """Every complete group of four lines is a 4-line FASTQ record: '@' line,
    one sequence line that starts with none of '@', '+', '>', '+' line, one
    quality line of the sequence's length (a trailing '\r' off both)."""
    for g in range(0, len(lines) - len(lines) % 4, 4):
        h, s, p, q = lines[g:g + 4]
        if h[:1] != b"@" or p[:1] != b"+" or s[:1] in (b"@", b"+", b">"):
            return False
        if len(_strip(s)) != len(_strip(q)):
            return False
    return True


def _kept(lines) -> bool:
    """Some line holds a byte kseq would keep (more than a trailing '\\r')."""
    return any(len(l) - (1 if l[-1:] == b"\r" else 0) > 0 for l in lines)


def lines_of(text: bytes, eof: bool):
    """The text's lines without their '\n'; a last line without one counts
    only at the end of the input."""
    ls = text.split(b"\n")
    last = ls.pop()
    if eof and last:
        ls.append(last)
    return ls


def layout(text: bytes) -> int:
    """How fastq.hip files the text: 1 FASTA (the first byte is '>'), 0 4-line
    FASTQ (groups of four lines, at most three empty lines after them), 2
    wrapped FASTQ (anything else kseq reads)."""
    if text[:1] == b">":
        return 1
    ls = lines_of(text, True)
    if four_line_groups(ls) and all(x == b"" for x in ls[len(ls) - len(ls) % 4:]):
        return 0
    return 2


def fields(text: bytes):
    """(return value of fqz5_fastq_index_any, the fqz5_fastq_rec fields of
    every record as dicts, the records' load_seqs_kseq sizes)."""
    recs, code = read_all(text)
    assert code == -1, code
    kind = layout(text)
    out = []
    for R in recs:
        assert (R.plus is None) == (kind == 1), "FASTA and FASTQ records in one text"
        if kind == 1:
            qual, fasta = R.stop, 1
        else:
            qual = R.qual_off
            fasta = 0 if kind == 0 else 2 | (KEEP_CR_SEQ if R.cr_seq else 0) | (KEEP_CR_QUAL if R.cr_qual else 0)
        out.append(dict(name=R.name_off, comment=R.comment_off, seq=R.seq_off, qual=qual,
                        name_len=len(R.name), comment_len=len(R.comment), seq_len=len(R.seq),
                        fasta=fasta, end=R.end))
    return (1 if kind == 1 else 0), out, [R.record_size for R in recs]


FIELDS = ("name", "comment", "seq", "qual", "name_len", "comment_len", "seq_len", "fasta", "end")


def ends(text: bytes, eof: bool):
    """fqz5_fastq_record_ends: the ends (exclusive offsets) of the complete
    FASTQ records of `text`.  At the end of the input every record counts and
    the text end closes the list.  Otherwise only whole lines count; 4-line
    text gives every complete group of four lines, wrapped text every record
    whose successor's header line has been seen (the bytes after a record
    belong to it until then).  None: not FASTQ text kseq reads, or one of
    the two texts kseq reads and fastq.hip refuses: a bare '@' or '>' as the
    last byte, and an empty record that the text ends after its '+' line."""
    if eof:
        ks, recs = Kseq(text), []
        while True:
            code = ks.read()
            if code < 0:
                break
            recs.append(ks.rec)
        if code != -1 or ks.bare or any(R.plus is None or R.no_qual_line for R in recs):
            return None
        if not recs and _kept(lines_of(text, True)):
            return None
        out = [R.end for R in recs]
        if text and (not out or out[-1] != len(text)):
            out.append(len(text))
        return out
    whole = text[:text.rfind(b"\n") + 1]
    ls = lines_of(whole, False)
    if four_line_groups(ls):
        out, at = [], 0
        for k, l in enumerate(ls[:len(ls) - len(ls) % 4]):
            at += len(l) + 1
            if k % 4 == 3:
                out.append(at)
        return out
    if not any(c in (62, 64) for c in whole):
        return None if _kept(ls) else []   # no header line: only empty lines are no records
    ks, out = Kseq(whole), []
    while True:
        r = ks.read()
        if r == -1:
            break
        if r == -2:                        # cut off inside the qualities, or too many of them
            if ks.short:
                break
            return None
        if ks.rec.plus is None:            # cut off before the '+' line, or a record without one
            if ks.rec.stop == len(whole):
                break
            return None
        out.append(ks.rec.end)
    # the last record stays open until a later header line has been seen
    if out and not any(c in (62, 64) for c in whole[out[-1]:]):
        out.pop()
    return out
