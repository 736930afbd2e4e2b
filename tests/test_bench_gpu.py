"""bench.py's plain run and --dump-outputs on a small workload (-1, 30 MB,
three 10 MB blocks): the plain run times `--steps` steps of the headline
workload and nothing else; the dump holds what the last step computed (the
blocks whole, since they fit the sample size: their md5 is the line's; the
decoded bytes as the seeded sample: equal to the same positions of the
input) and is the same from run to run."""
import contextlib
import hashlib
import io
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--level", "1", "--gb", "0.03"]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("cpu_baseline", "level5", "level5_illumina", "crc32", "dropin_cli")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    import bench
    out = []
    for tag in ("a", "b"):
        d = str(tmp_path_factory.mktemp("dump_" + tag))
        so, se = io.StringIO(), io.StringIO()
        with contextlib.redirect_stdout(so), contextlib.redirect_stderr(se):
            bench.main(ARGS + ["--dump-outputs", d])
        lines = so.getvalue().strip().splitlines()
        assert len(lines) == 1, lines
        out.append((json.loads(lines[0]), d, se.getvalue()))
    return out


def test_plain_line(runs):
    line, _, err = runs[0]
    for k in HEADLINE:
        assert k in line, k
    for k in FULL_ONLY:
        assert k not in line, k
    assert line["steps"] == 2 and line["warmup"] == 1
    assert err.count("[bench] -1 step:") == 2          # the timed steps; warmup logs none
    assert line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "MB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["config"]["roundtrip_ok"] is True
    assert line["config"]["blocks_rank0"] == 3


def test_dump_is_the_steps_output(runs):
    import bench
    from fqzcomp5_amd import sections as S, synth
    line, d, _ = runs[0]
    files = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert sorted(files) == ["block_byte_sums", "block_sizes", "blocks", "decoded",
                             "decoded_section_byte_sums", "section_methods", "section_sizes"]
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    # encode: the blocks fit the sample size, so they are written whole
    nbytes = line["config"]["fqz5_block_bytes_rank0"]
    assert nbytes <= bench.DUMP_SAMPLE
    assert files["block_sizes"].sum() == nbytes and len(files["block_sizes"]) == 3
    blk = files["blocks"].astype(np.uint8)
    assert hashlib.md5(blk.tobytes()).hexdigest() == line["config"]["blocks_md5_by_rank"][0]
    off = np.concatenate([[0], np.cumsum(files["block_sizes"])]).astype(np.int64)
    assert [int(blk[a:b].sum(dtype=np.int64)) for a, b in zip(off[:-1], off[1:])] \
        == files["block_byte_sums"].tolist()
    assert len(files["section_methods"]) == len(files["section_sizes"]) == 9
    assert sorted(set(files["section_methods"].astype(int).tolist())) \
        == line["config"]["methods_chosen"]
    # decode: every block's names, bases and qualities in block order
    reads = bench.make_reads(0.03, 1, "illumina")
    names, noff = synth.all_names(reads)
    soff = np.concatenate([[0], np.cumsum(reads.lens.astype(np.int64))])
    secs = []
    for a, b in synth.split_blocks(reads, S.BLOCK_SIZE[1]):
        secs += [names[noff[a]:noff[b]], reads.seq[soff[a]:soff[b]], reads.qual[soff[a]:soff[b]]]
    assert [int(s.sum(dtype=np.int64)) for s in secs] \
        == files["decoded_section_byte_sums"].tolist()
    whole = np.concatenate(secs)
    assert len(whole) > bench.DUMP_SAMPLE              # written as the seeded sample
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, len(whole),
                                                                  bench.DUMP_SAMPLE))
    assert np.array_equal(files["decoded"], whole[idx].astype(np.float32))


def test_dump_repeats(runs):
    (_, da, _), (_, db, _) = runs
    assert sorted(os.listdir(da)) == sorted(os.listdir(db))
    for f in os.listdir(da):
        a, b = np.load(os.path.join(da, f)), np.load(os.path.join(db, f))
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), f
