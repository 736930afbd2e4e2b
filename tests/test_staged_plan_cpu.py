"""The staged try's role walk (fqz5_staged_plan) against a Python model of
metrics_method (fqzcomp5.c:1899-1946) over random section-id sequences and
random incoming trial states: a call can start anywhere in a file."""
import ctypes as C

import numpy as np
import pytest

from fqzcomp5_amd import sections as S

REVIEW, TRIAL, DECIDED = 100, 3, -99999
STAGED = (S.SEC_SEQ, S.SEC_QUAL)


def _methods(mask):
    return [m for m in range(S.M_LAST) if mask >> m & 1]


def _random_state(rng, av):
    """(state, what): per kind fresh, mid-trial with 1-2 sections left, the
    window complete and undecided, decided, or decided with review at 0-2."""
    st = S.new_state()
    what = []
    for k in range(4):
        ss = st.sec[k]
        c = int(rng.integers(0, 5))
        ms = _methods(int(av[k])) or [1]
        if c in (1, 2):                       # sums of the window's earlier sections
            ss.review = REVIEW
            ss.trial = int(rng.integers(1, 3)) if c == 1 else 0
            for m in ms:
                ss.usize[m] = (TRIAL - ss.trial) * 1000
                ss.csize[m] = int(rng.integers(100, 900))
        elif c >= 3:
            ss.trial = DECIDED
            ss.review = int(rng.integers(3, REVIEW + 1)) if c == 3 else int(rng.integers(0, 3))
            ss.method_used = int(rng.choice(ms))
        what.append(c)
    return st, what


def _pick(ss):
    best, best_m = 1e30, 0
    for m in range(S.M_LAST):
        if ss.usize[m] and best > (ss.csize[m] + 1.0) / ss.usize[m]:
            best, best_m = (ss.csize[m] + 1.0) / ss.usize[m], m
    return best_m


def _model(ids, st):
    """metrics_method's counters: per section "trial", "decide" or "keep"."""
    rv = [st.sec[k].review for k in range(4)]
    tr = [st.sec[k].trial for k in range(4)]
    out = []
    for k in ids:
        if rv[k] <= 0:
            rv[k], tr[k] = REVIEW, TRIAL
        if tr[k] > 0:
            tr[k] -= 1
            out.append("trial")
        elif tr[k] > DECIDED:
            tr[k] = DECIDED
            out.append("decide")
        else:
            rv[k] -= 1
            out.append("keep")
    return out


@pytest.mark.parametrize("seed", range(40))
def test_plan_against_model(seed):
    rng = np.random.default_rng(seed)
    av = S.masks(int(rng.choice([3, 5])), True)
    n = int(rng.integers(1, 260))
    if rng.integers(0, 2):                    # whole blocks in file order
        ids = np.tile(np.array([0, 1, 2, 3], np.int32), n // 4 + 1)[:n]
    else:
        ids = rng.integers(0, 4, n).astype(np.int32)
    st, _ = _random_state(rng, av)
    before = bytes(st)
    roles, masks, win = S.staged_plan(ids, av, st)
    assert bytes(st) == before                # the state is not modified
    sched = S.trial_schedule(ids, av, st)
    steps = _model(ids, st)

    # trial rows are the schedule's, with the schedule's methods
    for i in range(n):
        assert (steps[i] == "trial") == bool(sched[i]) or not av[ids[i]]
        if steps[i] == "trial":
            assert masks[i] == sched[i] == av[ids[i]]
            assert roles[i] == (S.ROLE_TRIAL if ids[i] in STAGED else S.ROLE_OTHER)
        else:
            assert roles[i] != S.ROLE_TRIAL
        if ids[i] not in STAGED:
            assert roles[i] == S.ROLE_OTHER and win[i] == -1
            assert masks[i] == sched[i]

    for k in STAGED:
        rows = [i for i in range(n) if ids[i] == k]
        ss = st.sec[k]
        mid = ss.review > 0 and 0 < ss.trial          # sections of an open window to come
        # a call that starts inside a window: its remaining sections are
        # trial sections, and nothing follows before it is complete
        if mid:
            head = rows[:ss.trial]
            assert all(roles[i] == S.ROLE_TRIAL and win[i] == 0 for i in head)
        windows = {}
        for i in rows:
            if roles[i] == S.ROLE_TRIAL:
                windows.setdefault(int(win[i]), []).append(i)
        for w, wr in windows.items():
            assert wr == sorted(wr) and len(wr) <= TRIAL
        for i in rows:
            if roles[i] == S.ROLE_FOLLOW:
                # the governing window: in the call, earlier, and complete
                wr = windows[int(win[i])]
                assert max(wr) < i
                whole = ss.trial if (mid and win[i] == 0) else TRIAL
                assert len(wr) == whole
                assert masks[i] == 0
                # no section of the kind between the window and here tries anything
                assert all(roles[j] == S.ROLE_FOLLOW for j in rows if max(wr) < j < i)
            if roles[i] == S.ROLE_SETTLED:
                assert win[i] == -1 and not any(max(wr) < i for wr in windows.values())

    # a settled section's method is the one the replay gives it, whatever
    # the sizes of this call's candidates
    sizes = rng.integers(1, 1000, (n, S.M_LAST)).astype(np.uint32)
    ins = np.full(n, 1000, np.uint32)
    st2 = S._copy_state(st)
    meth = S.trial_replay(ids, ins, sizes, av, st2)
    for i in range(n):
        if roles[i] == S.ROLE_SETTLED:
            assert masks[i] == 1 << int(meth[i]), i
    for k in STAGED:
        ss = st.sec[k]
        first = next((i for i in range(n) if ids[i] == k), None)
        if first is not None and steps[first] == "decide":
            assert masks[first] == 1 << _pick(ss)      # the pick over the state's sums


def test_plan_fresh_file():
    """A fresh state, whole blocks: three trial blocks, 101 follow blocks,
    the re-trial at block 104, and follow sections of its window after it."""
    ids = np.tile(np.array([0, 1, 2, 3], np.int32), 112)
    av = S.masks(3)
    roles, masks, win = S.staged_plan(ids, av, S.new_state())
    for k in STAGED:
        r = roles[ids == k]
        w = win[ids == k]
        assert list(r[:3]) == [S.ROLE_TRIAL] * 3 and list(r[104:107]) == [S.ROLE_TRIAL] * 3
        assert (r[3:104] == S.ROLE_FOLLOW).all() and (r[107:] == S.ROLE_FOLLOW).all()
        assert (w[:104] == 0).all() and (w[104:] == 1).all()


def test_plan_decided_state():
    """A decided state (a later window of a file): every section is settled
    on the state's method until the re-trial."""
    av = S.masks(3)
    st = S.new_state()
    for k in range(4):
        st.sec[k].trial = DECIDED
        st.sec[k].review = 5
        st.sec[k].method_used = _methods(int(av[k]))[-1] if av[k] else 0
    ids = np.tile(np.array([0, 1, 2, 3], np.int32), 12)
    roles, masks, win = S.staged_plan(ids, av, st)
    for k in STAGED:
        r, m = roles[ids == k], masks[ids == k]
        assert list(r) == [S.ROLE_SETTLED] * 5 + [S.ROLE_TRIAL] * 3 + [S.ROLE_FOLLOW] * 4
        assert (m[:5] == 1 << st.sec[k].method_used).all() and (m[5:8] == av[k]).all()
