"""LZP streams for the host unlzp's tests (fqz5_unlzp_host) and for its
comparison with the kernel (fqz5_unlzp): hand-built streams with the bytes
they decode to, the oracle's streams of tests/lzp_cases.py, and damaged
streams with the capacity they are decoded into.

In the hand-built streams only a 233 / 234 byte consults the table, so what
each decodes to follows from the format alone.  P9 is 9 literals after which
position 9 has the context "ABCD" of position 4: the token at 9 is predicted,
from position 4.  (A hash keeps its last byte's low 4 bits, so the contexts in
between, which end in other letters, cannot take that table entry.)"""
from lzp_cases import cases

P9 = b"ABCDXABCD"


def hand_built():
    """(name, stream, decoded)"""
    return [
        ("empty", b"", b""),
        ("literals", b"HELLO, WORLD", b"HELLO, WORLD"),
        # markers where the table has nothing: literals themselves
        ("marker_empty_start", bytes([233, 234, 233]), bytes([233, 234, 233])),
        ("marker_empty_mid", b"ABC\xe9D", b"ABC\xe9D"),
        ("marker_empty_last", b"A\xe9", b"A\xe9"),
        ("marker2_empty_last", b"A\xea", b"A\xea"),
        ("escaped_after_233", P9 + bytes([233, 0, 233]) + b"Z", P9 + b"\xe9Z"),
        ("escaped_after_234", P9 + bytes([234, 0, 0, 234]) + b"Z", P9 + b"\xeaZ"),
        ("escaped_plain_byte", P9 + bytes([233, 0]) + b"Q", P9 + b"Q"),
        ("match_1byte_len", P9 + bytes([233, 5]), P9 + b"XABCD"),
        ("match_2byte_len_small", P9 + bytes([234, 0, 5]), P9 + b"XABCD"),
        ("match_2byte_len_65535", P9 + bytes([234, 255, 255]), P9 + b"XABCD" * 13107),
        ("match_then_literals", P9 + bytes([233, 3]) + b"tail", P9 + b"XABtail"),
        # overlapping matches: the source is op - 1, op - 2, op - 3
        ("period1", b"AAAAA" + bytes([233, 10]), b"A" * 15),
        ("period2", b"ABABAB" + bytes([233, 9]), b"ABABAB" + b"ABABABABA"),
        ("period3", b"ABCABCA" + bytes([233, 10]), b"ABCABCA" + b"BCABCABCAB"),
        ("period1_long", b"AAAAA" + bytes([234, 1, 44]), b"A" * 305),
        # sources inside positions 0..3, whose hashes start from 0: zeros hash
        # to 0 (position 2 is predicted from position 1), and the context
        # 0 0 A B of position 8 hashes as the context A B of position 2
        ("source_at_1", b"\0\0" + bytes([233, 7]), b"\0" * 9),
        ("source_at_2", b"ABCD\0\0AB" + bytes([233, 3]), b"ABCD\0\0ABCD\0"),
    ]


def oracle_streams(ora):
    """(name, stream, decoded) of every case of lzp_cases, coded by the oracle"""
    return [("lzp_cases/" + name, ora.lzp(data), data) for name, data in cases()]


def damaged():
    """(name, stream, cap): each must fail, and write nothing past cap"""
    whole = P9 + bytes([233, 5])                       # decodes to 14 bytes
    lits = b"HELLO, WORLD"
    return [
        ("ends_after_marker_233", P9 + bytes([233]), 64),
        ("ends_after_marker_234", P9 + bytes([234]), 64),
        ("ends_after_one_of_two_length_bytes", P9 + bytes([234, 1]), 64),
        ("ends_before_escaped_literal_233", P9 + bytes([233, 0]), 64),
        ("ends_before_escaped_literal_234", P9 + bytes([234, 0, 0]), 64),
        ("match_one_over_cap", whole, 13),
        ("match_far_over_cap", P9 + bytes([234, 255, 255]), 9 + 65534),
        ("literal_one_over_cap", lits, len(lits) - 1),
        ("escaped_literal_one_over_cap", P9 + bytes([233, 0, 233]), 9),
        ("cap_zero", b"A", 0),
    ]
