"""Child of test_rans_variants_gpu.py::test_o1_register_decoder_in_a_child_process.

Decodes the oracle's order-1, 4-state streams of the case table's alphabets of
up to 16 symbols on the GPU, one launch per alphabet size, first one copy per
job and then hedged, and prints one JSON line: the cases decoded, those whose
bytes differ from the input, and fqz5_rans_variant_counts.  It sets nothing:
started with $FQZ5_O1REG=1 the streams that fit run dec4_o1reg_body (at most
64 (context, symbol) pairs, 8 rows at 12 bits or 16 at 10), the others and
every stream of a process started without it the table decoders."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]


def main():
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    import rans_variant_cases as V
    from fqzcomp5_amd import lib
    if not lib.device_ok():
        raise SystemExit("no GPU: " + lib.last_error())
    so = lib.load()
    so.fqz5_set_host_decode(0)
    cases = [c for c in V.all_cases() if c.order == 1 and c.A <= 16 and c.n]
    bad = []
    for hedge in (0, 1):
        so.fqz5_set_hedge(hedge)
        for A in sorted({c.A for c in cases}):
            batch = [c for c in cases if c.A == A]
            src = [torch.frombuffer(bytearray(V.stream(c)), dtype=torch.uint8).cuda() for c in batch]
            dst = [torch.zeros(c.n, dtype=torch.uint8, device="cuda") for c in batch]
            lib.after_torch()
            jobs = [lib.RansJob(a.data_ptr(), b.data_ptr(), a.numel(), b.numel(), 0, 0, 0, 0)
                    for a, b in zip(src, dst)]
            lib.uncompress_batch_dev(jobs)
            for c, j, b in zip(batch, jobs, dst):
                if j.status != 0 or bytes(b.cpu().numpy()) != V.data(c.A, c.kind, c.n):
                    bad.append([hedge, *c])
    dec, hedged, _ = lib.rans_variant_counts()
    print(json.dumps({"cases": len(cases), "bad": bad, "dec": dec, "hedged": hedged}))


if __name__ == "__main__":
    main()
