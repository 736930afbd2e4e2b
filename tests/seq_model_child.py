"""Child of test_seq_edges_gpu.py::test_per_event_model_pass_in_a_child_process.

Encodes the run-length and tile cases of seq_edge_cases.py on the GPU against
the golden lengths and md5s and prints one JSON line: the cases encoded,
those whose bytes differ, and fqz5_seq_path_counts.  It sets nothing: started
with $FQZ5_SEQ_MODEL_EVENTS set, launch_seq_model runs k_seq_model (a lane
per sorted event, the heads walk their runs); without it k_seq_model_runs."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]


def main():
    import seq_edge_cases as E
    from fqzcomp5_amd import lib
    if not lib.device_ok():
        raise SystemExit("no GPU: " + lib.last_error())
    gold = {r["case"]: r for r in json.load(open(os.path.join(HERE, "golden", "seq_edges.json")))}
    cases = [c for c in E.cases() if c.name.startswith(("run1_", "runx_", "span"))]
    bad = []
    for c in cases:
        z = lib.seq_encode(c.seq, c.lens, c.both, c.k)
        if (len(z), hashlib.md5(z).hexdigest()) != (gold[c.name]["len"], gold[c.name]["md5"]):
            bad.append(c.name)
    print(json.dumps({"cases": len(cases), "bad": bad, "counts": lib.seq_path_counts()}))


if __name__ == "__main__":
    main()
