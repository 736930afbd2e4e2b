"""Inputs for the lane-group form of the 32-state rANS encoder chain
(k_enc_chain_x32g), shared by test_x32_groups_gpu.py and its child process.

A 32-state job of n = 32*m + r bytes runs T steps: m (r = 0) or m + 1 at
order 4, and m + r at order 5, where state 31 owns the tail.  The values of m
put T at and around the 32-step checkpoint (32, 33) and the lane group's
256-step staged chunk (255, 256, 257, 512); r = 1 and 31 give state 31 its
longer run.  1024 is the smallest: the reference codes inputs of up to 1000
bytes with 4 states.

Run as a program it is the child: it encodes every case with host encode off
and the group threshold at 0 and prints one JSON line, the md5 of each stream
and fqz5_rans_variant_counts.  Started with $FQZ5_X32_GROUPS=0 the library
keeps every chain on k_enc_chain whatever the threshold."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

import rans_variant_cases as V

M = (32, 33, 255, 256, 257, 512)
R = (0, 1, 31)
LENGTHS = tuple(32 * m + r for m in M for r in R)
# (alphabet, kind): 2 symbols, 5 (the LZP3 streams' shape), and at order 5 the
# first alphabet whose order-1 table is compact (rans_variant_cases.ENC_LDS_LAST_A)
INPUTS = ((2, "skew"), (2, "walk"), (5, "skew"), (5, "walk"))
COMPACT = (V.ENC_LDS_LAST_A + 1, "walk")
LZP3 = (5, "walk")
BIG_N = (1 << 20) + 37


def cases(order):
    inputs = INPUTS + ((COMPACT,) if order & 1 else ())
    return [V.Case(A, kind, n, order) for A, kind in inputs for n in LENGTHS]


def grouped_name(c):
    """The lane-group body that codes a case once every 32-state chain is
    grouped; None for a case the old names keep (4 states)."""
    name = V.enc_job(c)
    return "E32G" + name[3:] if name and name.startswith("E32_") else None


def encode(batch):
    """fqz5_rans_compress_batch of device inputs, one launch: the streams."""
    import torch
    from fqzcomp5_amd import lib
    datas = [V.data(c.A, c.kind, c.n) for c in batch]
    caps = [lib.compress_bound(c.n, c.order) for c in batch]
    src = [torch.frombuffer(bytearray(d), dtype=torch.uint8).cuda() for d in datas]
    dst = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for cap in caps]
    lib.after_torch()
    jobs = [lib.RansJob(a.data_ptr(), b.data_ptr(), a.numel(), b.numel(), c.order, 0, 0, 0)
            for a, b, c in zip(src, dst, batch)]
    lib.compress_batch_dev(jobs)
    assert all(j.status == 0 for j in jobs)
    return [bytes(b[:j.out_size].cpu().numpy()) for b, j in zip(dst, jobs)]


def main():
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    from fqzcomp5_amd import lib
    if not lib.device_ok():
        raise SystemExit("no GPU: " + lib.last_error())
    lib.set_host_encode(0)
    lib.set_x32_group_min(0)
    md5 = {}
    for order in (4, 5):
        batch = cases(order)
        for c, s in zip(batch, encode(batch)):
            md5["%d %s %d %d" % c] = hashlib.md5(s).hexdigest()
    big = V.Case(*LZP3, BIG_N, 5)
    md5["big"] = hashlib.md5(encode([big])[0]).hexdigest()
    print(json.dumps({"md5": md5, "enc": lib.rans_variant_counts()[2]}))


if __name__ == "__main__":
    main()
