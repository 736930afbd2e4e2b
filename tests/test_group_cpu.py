"""fqz5file._group, the one rule by which every read pass (decompress_file,
extract_file, the lookups by name and by sequence, stats) groups blocks into
windows of at most `window_bytes` of compressed data: an item joins the
current group unless that group has items and would pass the limit with it.
No GPU: explicit size lists, and the block sizes of a six-block container
made of fake blocks as tests/test_extract_cpu.py makes them."""
import struct

from fqzcomp5_amd import fqz5file as Z


def _sizes(sizes, wb):
    """The groups of `sizes` themselves (items 0..n-1 sized sizes[k])."""
    return [[sizes[k] for k in g] for g in Z._group(range(len(sizes)), lambda k: sizes[k], wb)]


def _by_rule(sizes, wb):
    """The rule stated item by item: close the group when it has items and
    the next would take it past wb."""
    groups = []
    for k, z in enumerate(sizes):
        if groups and sum(sizes[j] for j in groups[-1]) + z <= wb:
            groups[-1].append(k)
        else:
            groups.append([k])
    return groups


def test_empty_and_one_per_group():
    assert Z._group([], lambda x: x, 10) == []
    assert Z._group(iter(()), lambda x: x, 1) == []
    assert _sizes([5, 1, 7, 1], 1) == [[5], [1], [7], [1]]
    assert _sizes([1, 1, 1], 1) == [[1], [1], [1]]


def test_item_larger_than_the_window_stands_alone():
    assert _sizes([3, 50, 2, 2], 10) == [[3], [50], [2, 2]]
    assert _sizes([50, 2, 2], 10) == [[50], [2, 2]]
    assert _sizes([2, 2, 50], 10) == [[2, 2], [50]]
    assert _sizes([50, 60], 10) == [[50], [60]]


def test_group_closes_exactly_at_the_limit():
    assert _sizes([4, 3, 3], 10) == [[4, 3, 3]]                 # sums to wb: together
    assert _sizes([4, 3, 4], 10) == [[4, 3], [4]]               # wb + 1: split
    assert _sizes([4, 3, 3, 1], 10) == [[4, 3, 3], [1]]
    assert _sizes([10, 10], 10) == [[10], [10]]
    assert _sizes([0, 10, 0, 1], 10) == [[0, 10, 0], [1]]


def test_order_kept_every_item_once():
    items = [("f", 7), ("a", 2), ("q", 9), ("b", 1), ("z", 4), ("c", 4), ("k", 12), ("d", 3)]
    for wb in (1, 5, 9, 10, 11, 16, 100):
        groups = Z._group(items, lambda it: it[1], wb)
        assert [it for g in groups for it in g] == items, wb
        assert all(g for g in groups), wb
        assert all(sum(z for _, z in g) <= wb or len(g) == 1 for g in groups), wb
        # no group could have taken the next group's first item
        assert all(sum(z for _, z in g) + h[0][1] > wb for g, h in zip(groups, groups[1:])), wb
    cover = [(3, 1, 1), (4, 0, 2), (5, 0, 1)]                   # (extract_file groups cover triples)
    assert Z._group(cover, lambda c: 10, 20) == [cover[:2], cover[2:]]


def test_six_block_container():
    """The block sizes a container's index gives, at the window sizes the GPU
    tests use: one block per window (1), everything in one (the default), twice
    the largest block, a third of the file."""
    payload = [113, 97, 140, 121, 88, 61]
    nrec = [2, 2, 2, 2, 2, 1]
    blocks = [struct.pack("<II", 4 + p, n) + bytes([65 + k]) * p
              for k, (n, p) in enumerate(zip(nrec, payload))]
    data = Z.container(blocks, [10 * n for n in nrec], nrec)
    index = Z.read_index(data)
    sizes = [t - s for s, t, _ in index]
    assert sizes == [8 + p for p in payload]
    for wb in (1, Z.DEFAULT_WINDOW, 2 * max(sizes), len(data) // 3, sum(sizes), sum(sizes) - 1):
        want = _by_rule(sizes, wb)
        got = Z._group(range(len(index)), lambda b: index[b][1] - index[b][0], wb)
        assert got == want, wb
    assert _by_rule(sizes, 1) == [[0], [1], [2], [3], [4], [5]]
    assert _by_rule(sizes, Z.DEFAULT_WINDOW) == [[0, 1, 2, 3, 4, 5]]
    assert _by_rule(sizes, 2 * max(sizes)) == [[0, 1], [2, 3], [4, 5]]
