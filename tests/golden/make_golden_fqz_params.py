"""Generate the golden vectors of tests/fqz_param_cases.py from the compiled
reference (oracle/_ref/libhtsref.so): fqz_compress with caller-supplied
parameters, with reversal (vers 3) and with empty records.

Inputs are regenerated from the seeded cases; this script stores for every
(case, strat) the expected output length and md5, the md5 of what the call
left in the caller's parameter block (gp_md5, see gp_digest), the record
lengths as the call left them where it changed them, whether the reference
decodes its own stream, and the full bytes of the smaller streams
(fqz_params.bin) for decode tests.
Run from the repo root: python tests/golden/make_golden_fqz_params.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from fqz_param_cases import cases, gp_digest  # noqa: E402
from oracle import binding  # noqa: E402

SMALL = 25000


def main():
    ref = binding.ref()
    out, blob = [], bytearray()
    for c in cases():
        for st in c.strats:
            gp = c.gp()
            comp = ref.fqz_compress(c.q, c.lens.copy(), c.flags.copy(), st, c.seq, c.vers, gp)
            rec = {"case": c.name, "strat": st, "len": len(comp),
                   "md5": hashlib.md5(comp).hexdigest(), "gp_md5": gp_digest(gp), "off": None,
                   "last_len": ref.last_lens[-1] if ref.last_lens else None}
            assert all(f < 65536 for f in ref.last_flags), c.name
            if len(comp) <= SMALL:
                rec["off"] = len(blob)
                blob += comp
            try:
                back = ref.fqz_decompress(comp, ref.last_lens, c.flags & 0xffff, c.seq)
            except RuntimeError:
                back = None
            rec["decodes"] = back is not None
            assert back is None or back == c.q, (c.name, st)
            out.append(rec)
    json.dump(out, open(os.path.join(HERE, "fqz_params.json"), "w"), indent=0)
    open(os.path.join(HERE, "fqz_params.bin"), "wb").write(bytes(blob))
    print(len(out), "vectors,", len(blob), "bytes of small outputs")


if __name__ == "__main__":
    main()
