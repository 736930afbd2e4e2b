"""The case table of test_rans_variants_gpu.py (rans_variant_cases.py) against
the oracle alone, no GPU: every input round-trips, the oracle's streams reach
both sides of every table-placement threshold of the decoder and of the
encoder, and each class's own input selects that class."""
from collections import defaultdict

import pytest

import rans_variant_cases as V
from oracle import binding


def test_every_case_round_trips_through_the_oracle():
    ora = binding.oracle()
    cases = V.all_cases() + V.transform_cases()
    assert len(set(cases)) == len(cases)
    for c in cases:
        assert ora.rans_uncompress(V.stream(c)) == V.data(c.A, c.kind, c.n), c


@pytest.mark.skipif(not binding.have_ref(), reason="the reference was not built")
def test_the_reference_makes_the_same_streams():
    ref = binding.ref()
    for c in V.class_cases() + V.transform_cases():
        assert ref.rans_compress(V.data(c.A, c.kind, c.n), c.order) == V.stream(c), c


def test_case_table_holds_every_alphabet_and_length():
    """Every alphabet size flat and skewed at three lengths and four orders,
    with exactly that many symbols, byte 0 among them; every class's input
    at every length."""
    cases = V.all_cases()
    for A in V.ALPHABETS:
        for o in V.ORDERS:
            for n in V.ALPHABET_LENGTHS:
                assert {V.Case(A, "flat", n, o), V.Case(A, "skew", n, o)} <= set(cases)
        d = V.data(A, "flat", 4097)
        assert len(set(d)) == A and 0 in set(d)
    for A, kind, o in (*V.DEC_CLASS_INPUT.values(), *V.ENC_CLASS_INPUT.values()):
        assert {V.Case(A, kind, n, o) for n in V.LENGTHS} <= set(cases)


def test_each_class_input_selects_its_class():
    """A class's input at CLASS_N bytes runs that class (first in dec_jobs;
    a compressed order-1 table adds its order-0 chain behind it), and over
    all lengths every class but the opt-in O1REG* occurs."""
    for name, (A, kind, o) in V.DEC_CLASS_INPUT.items():
        assert V.dec_jobs(V.stream(V.Case(A, kind, V.CLASS_N, o)))[0] == name
    for name, (A, kind, o) in V.ENC_CLASS_INPUT.items():
        assert V.enc_job(V.Case(A, kind, V.CLASS_N, o)) == name
    # the hedged batches' lengths: 777 is under one group of every body (and
    # under the 1000 bytes that keep 32 states), 1024 and 2048 are group edges
    for n in (1024, 2048, V.CLASS_N):
        got = set()
        for A, kind, o in V.DEC_CLASS_INPUT.values():
            got.update(V.dec_jobs(V.stream(V.Case(A, kind, n, o))))
        want = set(V.DEC_CLASS_INPUT)
        if n == 1024:
            # 1024 bytes over 128 symbols are stored uncoded
            want -= {"O1_GLOBAL", "X32_O1_SPLIT", "X32_O1_GLOBAL"}
        elif n == 2048:
            want -= {"X32_O1_GLOBAL"}
        assert want <= got, (n, want - got)


def test_streams_reach_both_sides_of_every_decoder_threshold():
    """The (rows, shift) pairs of the oracle's order-1 streams, 4 states and
    32, hold every pair of rans_variant_cases.THRESHOLDS (the literal list of
    both sides of each threshold of kernels.h:129-153), and dec_jobs names
    the body listed there for every stream of that pair.  The reference's
    rans_compute_shift produced every pair, so none is dropped: 12 bits at 2
    and 3 rows needs the `runs` kind with a switch every ~200 bytes
    (rans_variant_cases.data), the others come from `runs` at 12 bits and
    `walk` at 10."""
    seen = {k: {V.dec_jobs(V.stream(c))[0] for c in cs} for k, cs in V.o1_pairs().items()}
    assert len(V.THRESHOLDS) == 12
    for (rows, bits), name in V.THRESHOLDS:
        assert seen.get((4, rows, bits)) == {name}, (rows, bits)
        assert seen.get((32, rows, bits)) == {V.x32_name(name)}, (rows, bits)
    # every pair the table makes is placed one way
    assert all(len(names) == 1 for names in seen.values())


def test_encoder_alphabets_on_both_sides_of_the_lds_table():
    """Order-1 alphabets of 64 and 65 symbols (byte 0 counted), the last
    whose 16-byte entries fit the encoder's LDS table and the first that
    takes the compact one (kernels.h ENC_TAB_LDS_MAX, enc_tab_compact), with
    4 states and with 32."""
    seen = defaultdict(set)
    for c in V.all_cases():
        d = V.data(c.A, c.kind, c.n)
        if c.order & 1 and len(d) >= 8:
            seen[32 if c.order & 4 and len(d) > 1000 else 4].add((len(set(d) | {0}), V.enc_job(c)))
    assert {(64, "E2W_O1"), (65, "E1W_O1_COMPACT")} <= seen[4]
    assert {(64, "E32_O1"), (65, "E32_O1_COMPACT")} <= seen[32]
    assert {V.enc_job(c) for c in V.all_cases()} - {None} == set(V.ENC_CLASS_INPUT)
