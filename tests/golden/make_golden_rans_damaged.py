#!/usr/bin/env python3
"""What the compiled reference (oracle/_ref/libhtsref.so) does with every
damaged rANS 4x16 stream of tests/rans_damage_cases.py.  Run here:

    make -C oracle && python tests/golden/make_golden_rans_damaged.py

Written: rans_damaged.json.  Per case the name, the stream's md5, the caller's
capacity and either null (rans_uncompress_to_4x16 returned NULL), [length,
md5] of what it decoded, or "stale": outcomes only, no stream and no decoded
bytes.  "stale" is a case whose outcome is no function of the stream.  The
reference's order-1 decoders keep their tables in thread-local memory that
the next call finds as it was left; a context row without frequencies is
skipped (rANS_static4x16pr.c:611), and the 32-state decoder goes on after its
table parser failed (rANS_static32x16pr.c:604), so such a stream decodes from
what an earlier call left there.  Every case is decoded twice, each time
after sound streams that fill those tables, of other data the second time
(poison); where the two differ the case stays in the corpus as "stale", and
the GPU tests ask of it what the oracle gives (its tables start zeroed, and
it refuses an order-1 table without a row for context 0).  Per mutation class the number
of cases the reference refuses ("null"), decodes to other bytes than the
undamaged stream's ("other"), to the same bytes ("same"), and the stale ones;
"excluded" is the number of generated cases left out (none).
The damage is real: every class has a refused case, and some case decodes to
other bytes."""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import rans_damage_cases as rd  # noqa: E402
from oracle import binding  # noqa: E402


def outcome(codec, stream, cap):
    r = codec.rans_uncompress_to(stream, cap)
    return None if r is None else [len(r), rd.md5(r)]


def poison(which):
    """Sound order-1 streams of all 256 symbols, 4 and 32 states, 10- and
    12-bit tables: decoding them leaves every context row of the reference's
    tables filled, with other rows for `which` 0 and 1."""
    import numpy as np
    ora = binding.oracle()
    r = np.random.default_rng(4000 + which)
    out = []
    for conc in (0.05, 5.0):
        d = np.concatenate([np.arange(256), r.choice(256, 70001, p=r.dirichlet(np.full(256, conc)))])
        d = d.astype(np.uint8).tobytes()
        out += [(ora.rans_compress(d, o), len(d)) for o in (1, 5)]
    return out


def build(codec, again=None):
    """again: decode every case twice, each time after poison()."""
    corpus = rd.corpus()
    fill = [poison(0), poison(1)] if again else []
    sound = {}                      # base name -> outcome of the undamaged stream
    cases, classes = [], {}
    for name, mc, stream, cap in corpus:
        for ps, pn in fill[0] if again else []:
            assert codec.rans_uncompress_to(ps, pn) is not None
        o = outcome(codec, stream, cap)
        if again:
            for ps, pn in fill[1]:
                assert again.rans_uncompress_to(ps, pn) is not None
            if outcome(again, stream, cap) != o:
                o = "stale"
        if mc == "base":
            assert o is not None and o != "stale", name
            sound[rd.base_of(name)] = o
        cases.append([name, rd.md5(stream), cap, o])
        c = classes.setdefault(mc, {"cases": 0, "null": 0, "other": 0, "same": 0, "stale": 0})
        c["cases"] += 1
        c["stale" if o == "stale" else "null" if o is None else "same" if o == sound[rd.base_of(name)] else "other"] += 1
    return {"count": len(cases), "excluded": 0, "classes": classes, "cases": cases}


def main():
    fx = build(binding.ref(), binding.ref())
    for mc, c in fx["classes"].items():
        assert mc == "base" or c["null"] > 0, (mc, c)
    assert sum(c["other"] for c in fx["classes"].values()) > 0
    with open(os.path.join(HERE, "rans_damaged.json"), "w") as f:
        json.dump(fx, f, indent=0)
        f.write("\n")
    print(fx["count"], "cases;", json.dumps(fx["classes"]))


if __name__ == "__main__":
    main()
