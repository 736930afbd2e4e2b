"""Generate the golden vectors of the sequence model's edge cases from the
compiled reference (oracle/_ref/libfqz5ref.so: fqzcomp5.c's own encode_seq /
decode_seq, which take any context size of 1..14 although its command line
offers only 10..14).

Inputs are regenerated from tests/seq_edge_cases.py (seeded); this script
stores per case the output length and md5 (seq_edges.json) and the bytes of
the streams of up to KEEP bytes (seq_edges.bin) for the decode tests.
Run from the repo root: python tests/golden/make_golden_seq_edges.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from seq_edge_cases import cases  # noqa: E402
from oracle import binding  # noqa: E402

KEEP = 40000


def main():
    ref = binding.seq_ref()
    out, blob = [], bytearray()
    for c in cases():
        z = ref.encode(c.seq, c.lens, c.both, c.k)
        rec = {"case": c.name, "k": c.k, "both": c.both, "n": len(c.seq), "len": len(z),
               "md5": hashlib.md5(z).hexdigest(), "off": None}
        if len(z) <= KEEP:
            rec["off"] = len(blob)
            blob += z
        assert ref.decode(z, c.lens, c.both, c.k, len(c.seq)) == c.seq, c.name
        out.append(rec)
    assert len(blob) < (1 << 20)
    json.dump(out, open(os.path.join(HERE, "seq_edges.json"), "w"), indent=0)
    open(os.path.join(HERE, "seq_edges.bin"), "wb").write(bytes(blob))
    print(len(out), "vectors,", len(blob), "bytes of streams,",
          sorted({r["len"] % 16 for r in out}), "residues mod 16")


if __name__ == "__main__":
    main()
