"""kseq_ref (the plain restatement of kseq_read and load_seqs_kseq the GPU
tests of fastq.hip compare with) pinned to the reference CLI: for every
must-equal text of fastq_text_cases, the model's records rendered as
output_fastq / output_fasta are what the reference decoded
(tests/golden/fastq_text.json, from make_golden_fastq_text.py); the model
ends every such text with -1 and every refusal with its stated code; and
the offsets it reports slice the text to the bytes it returned."""
import hashlib
import json
import os

import pytest

import fastq_text_cases as T
import kseq_ref as K

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                   "fastq_text.json")))


def md5(b: bytes) -> str:
    return hashlib.md5(b).hexdigest()


def test_counts():
    # nothing is filtered at run time: both sets are closed
    assert len(T.MUST_EQUAL) == T.N_MUST_EQUAL == len(GOLD["cases"]) == 68
    assert set(T.MUST_EQUAL) == set(GOLD["cases"]) == set(T.LAYOUT)
    assert len(T.REFUSALS) == T.N_REFUSALS == 10
    assert {n: len(GOLD["fuzz"][n]["dec_md5"]) for n in GOLD["fuzz"]} == {n: c for n, (_, c) in T.FUZZ.items()}
    assert {n: GOLD["fuzz"][n]["seed"] for n in GOLD["fuzz"]} == {n: s for n, (s, _) in T.FUZZ.items()}
    assert len(T.TILES) == 11
    assert sorted(len(T.MUST_EQUAL["tile_len_%d" % n]) for n in (4095, 4096, 4097, 65535, 65536, 65537, 131073)) \
        == [4095, 4096, 4097, 65535, 65536, 65537, 131073]


@pytest.mark.parametrize("name", list(T.MUST_EQUAL))
def test_model_is_the_reference(name):
    text, g = T.MUST_EQUAL[name], GOLD["cases"][name]
    assert md5(text) == g["in_md5"], "the case module and the fixture differ: rerun the maker"
    recs, code = K.read_all(text)
    assert code == -1 and recs
    out = K.render(recs)
    if "dec" in g:
        assert out == g["dec"].encode("latin-1")
    assert (len(out), md5(out)) == (g["dec_len"], g["dec_md5"])
    assert (len(text) <= T.SHORT) == ("dec" in g)
    assert K.layout(text) == {"fq4": 0, "fa": 1, "ml": 2}[T.LAYOUT[name]]


@pytest.mark.parametrize("lay", list(T.FUZZ))
def test_fuzz_is_the_reference(lay):
    texts, g = T.fuzz_texts(lay), GOLD["fuzz"][lay]
    assert len(texts) == g["count"] == T.FUZZ[lay][1]
    assert md5(b"\0".join(texts)) == g["in_md5"], "seed and count do not give the committed texts"
    for k, text in enumerate(texts):
        recs, code = K.read_all(text)
        assert code == -1 and recs, (k, text)
        assert len(recs) <= 6
        assert md5(K.render(recs))[:12] == g["dec_md5"][k], (k, text)
        if lay != "ml":                       # (wrapped fuzz may come out as 4-line text)
            assert K.layout(text) == {"fq4": 0, "fa": 1}[lay], (k, text)
        _offsets(text)


def _unwrap(b: bytes) -> bytes:
    return b.replace(b"\n", b"").replace(b"\r", b"")


def _offsets(text: bytes):
    """The fields the model states slice the text to what kseq returned."""
    rc, fields, sizes = K.fields(text)
    recs, _ = K.read_all(text)
    assert len(fields) == len(recs) == len(sizes)
    prev_end = 0
    for F, R, size in zip(fields, recs, sizes):
        assert text[F["name"]:F["name"] + F["name_len"]] == R.name
        assert text[F["comment"]:F["comment"] + F["comment_len"]] == R.comment
        assert text[F["name"] - 1:F["name"]] == (b">" if rc else b"@")
        assert size == len(R.name) + 1 + len(R.seq) + len(R.qual)
        assert prev_end <= F["name"] - 1 < F["seq"] <= F["qual"] <= F["end"] <= len(text)
        kind = F["fasta"] & 0xff
        assert (kind == 1) == (rc == 1)
        if kind == 0:
            assert text[F["seq"]:F["seq"] + F["seq_len"]] == R.seq
            assert text[F["qual"]:F["qual"] + F["seq_len"]] == R.qual
            assert text[F["end"] - 1:F["end"]] == b"\n" or F["end"] == len(text)
        elif kind == 1:
            assert R.qual == b""
            assert _unwrap(text[F["seq"]:F["qual"]]) == _unwrap(R.seq)
            assert F["qual"] == F["end"] and text[F["end"]:F["end"] + 1] in (b">", b"")
        else:
            assert _unwrap(text[F["seq"]:R.plus]) == _unwrap(R.seq)
            assert _unwrap(text[F["qual"]:F["end"]]) == _unwrap(R.qual)
            assert bool(F["fasta"] & K.KEEP_CR_SEQ) == (R.seq[:1] == b"\r" and text[R.seq_first:R.seq_first + 2]
                                                        in (b"\r\n", b"\r"))
            assert len(R.seq) == len(R.qual)
        prev_end = F["end"]
    return rc, fields


@pytest.mark.parametrize("name", list(T.MUST_EQUAL))
def test_offsets_slice_the_text(name):
    text = T.MUST_EQUAL[name]
    rc, fields = _offsets(text)
    if name in T.TILES:
        # every newline of a 4-line text follows from the fields
        nl = []
        for F in fields:
            plus = F["seq"] + F["seq_len"] + 1
            nl += [F["seq"] - 1, plus - 1, F["qual"] - 1, F["end"] - 1]
        assert nl == T.tile_newlines(text) == [i for i, c in enumerate(text) if c == 10]
    e = K.ends(text, True)
    if rc == 1:
        assert e is None
    else:
        assert e[-1] == len(text) and e[:len(fields)] == [F["end"] for F in fields]
        part = K.ends(text, False)
        assert part == e[:len(part)] and len(part) >= len(fields) - 1


def test_hand_cases_of_the_issue():
    # the two confirmed differences, as the reference reads them
    recs, code = K.read_all(T.MUST_EQUAL["fa_last_lone_cr"])
    assert code == -1 and [R.seq for R in recs] == [b"ATCTC", b"AG\r"]
    recs, code = K.read_all(T.MUST_EQUAL["fa_bare_gt_last"])
    assert code == -1 and [(R.name, R.comment, R.seq) for R in recs] == [(b"1a", b"", b"AC"), (b"", b"x", b"GG")]
    assert recs[1].end == len(T.MUST_EQUAL["fa_bare_gt_last"]) - 1
    # X '\r' at the end still drops the '\r'
    assert K.read_all(T.MUST_EQUAL["fa_no_final_nl_x_cr"])[0][0].seq == b"ACX"
    # end never exceeds len
    _, f, _ = K.fields(T.MUST_EQUAL["fq4_no_final_nl"])
    assert f[-1]["end"] == len(T.MUST_EQUAL["fq4_no_final_nl"])
    # READ2 flags (fqzcomp5.c:518-527)
    recs, _ = K.read_all(b"@ab c/2\nA\n+\nI\n@a /2\nA\n+\nI\n@/2\nA\n+\nI\n@x\nA\n+\nI\n@x\nA\n+\nI\n@y\nA\n+\nI\n")
    assert K.flags(recs) == [128, 0, 128, 0, 128, 0]
    assert K.flags(recs[4:]) == [0, 0]                     # the block's first record has no previous name
    frecs, _ = K.read_all(T.FLAGS_TEXT)
    assert tuple(K.flags(frecs)) == T.FLAGS_WANT and K.flags(frecs[T.FLAGS_REPEAT:])[0] == 0
    assert recs[0].name_bytes == b"ab c/2\0" and recs[0].qual33 == bytes([ord("I") - 33])
    assert K.Rec().qual33 == b"" and K.read_all(b"@a\n\r\n+\n\r\n")[0][0].qual33 == bytes([(13 - 33) & 255])


@pytest.mark.parametrize("case", T.REFUSALS, ids=[r[0] for r in T.REFUSALS])
def test_refusals_are_stated(case):
    name, text, api, code, reason = case
    assert api in ("any", "index") and reason
    recs, got = K.read_all(text)
    assert got == (-1 if code is None else code)
    if code is None and api == "any" and name not in ("bare_at_last", "no_quality_line"):
        # kseq reads on, but not as FASTQ records alone / FASTA records alone
        mixed = len({R.plus is None for R in recs}) == 2
        mid_line = any(R.hdr and text[R.hdr - 1] != 10 for R in recs)
        at_in_fasta = text[:1] == b">" and any(text[R.hdr] == 64 or R.plus is not None for R in recs)
        assert mixed or mid_line or at_in_fasta
    if name == "bare_at_last":
        assert [R.name for R in recs] == [b"ok"]            # the reference ignores the '@'
    if name == "no_quality_line":
        assert (recs[-1].name, recs[-1].seq, recs[-1].qual, recs[-1].qual_off) == (b"e", b"", b"", len(text))
    if name in ("bare_at_last", "no_quality_line"):
        assert K.ends(text, True) is None                    # ends() states both
    if api == "index":
        assert K.layout(text) == 2 and all(R.plus is not None for R in recs)
