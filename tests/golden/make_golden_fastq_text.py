"""What the reference CLI decodes for every must-equal text of
tests/fastq_text_cases.py (the hand-made and tile texts and the seeded fuzz):
each is coded with oracle/_ref/fqzcomp5 -1 -t1 and decoded with -d, and
fastq_text.json keeps the md5 of the input and the length and md5 of the
decoded text (for the short hand-made texts the decoded text itself).  A text
the reference does not take stops the run: it is changed or removed in the
case module, never skipped in a test.
python tests/golden/make_golden_fastq_text.py"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "fqzcomp5")
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import fastq_text_cases as T  # noqa: E402


def md5(b: bytes) -> str:
    return hashlib.md5(b).hexdigest()


def decode(wd: str, text: bytes, what: str) -> bytes:
    src, z, dec = (os.path.join(wd, n) for n in ("in.fq", "o.fqz5", "dec"))
    open(src, "wb").write(text)
    for p in (z, dec):
        if os.path.exists(p):
            os.remove(p)
    r = subprocess.run([REF, "-1", "-t1", src, z], capture_output=True)
    assert r.returncode == 0 and os.path.getsize(z) > 0, (what, text[:80], r.stderr[-300:])
    r = subprocess.run([REF, "-d", "-t1", z, dec], capture_output=True)
    assert r.returncode == 0, (what, text[:80], r.stderr[-300:])
    out = open(dec, "rb").read()
    assert out, (what, "the reference decoded nothing", text[:80])
    return out


if __name__ == "__main__":
    cases, fuzz = {}, {}
    with tempfile.TemporaryDirectory() as wd:
        for name, text in T.MUST_EQUAL.items():
            d = decode(wd, text, name)
            cases[name] = dict(in_md5=md5(text), dec_len=len(d), dec_md5=md5(d))
            if len(text) <= T.SHORT:
                cases[name]["dec"] = d.decode("latin-1")
        for lay, (seed, count) in T.FUZZ.items():
            texts = T.fuzz_texts(lay)
            fuzz[lay] = dict(seed=seed, count=count, in_md5=md5(b"\0".join(texts)),
                             dec_md5=[md5(decode(wd, t, "%s fuzz %d" % (lay, k)))[:12]
                                      for k, t in enumerate(texts)])
    json.dump(dict(cases=cases, fuzz=fuzz), open(os.path.join(HERE, "fastq_text.json"), "w"),
              indent=0, sort_keys=True)
    print(len(cases), "texts,", {k: v["count"] for k, v in fuzz.items()}, "fuzz texts")
