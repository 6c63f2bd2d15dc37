"""Where the deferred updates of the inversions' 16-column panel chain are issued (csrc/bcr_chain_schedule.h: the table kChainSchedule,
expanded by bcr_chain_body.h and restated event by event, in program order, by oicc_debug_bcr_chain_schedule), on the host alone.

A column c of a panel is a dependent sequence (pivot read, rsq, two Goldschmidt steps, l, strip store, the v_readlane hop onto column
c + 1); the updates av[c2] = fma(-l(k), m(k, c2), av[c2]) with c2 >= k + 2 are independent of it and sit in the gaps between its steps,
anywhere between column k's strip store and column c2's pivot read.  Whatever the placement, the bits of the factor depend on it
only through the order in which an entry takes its updates, so that order and the lifetimes of the strips are what is asserted here.

The bound per gap: scripts/micro/chain_issue.hip measured the placements; the one kept puts two updates into each of the two
v_readlane shadows of a column (behind the pivot's and behind the hop's: 24.6 cycles each, six issue slots) and at most one behind a
dependent fp64 step, whose latency is an issue slot or two; three or four in a shadow measured no better.  So no gap holds more than
2 updates, and no column more than 8 (105 updates over the 14 columns 1 .. 14).
"""
import numpy as np

from openimucameracalibrator_amd import _abi, _lib

PIVOT, STORE, LOAD, UPDATE, HOP = range(5)
MAX_PER_GAP = 2
MAX_PER_COLUMN = 8


def events():
    b = _lib.load_bcr_plan()
    n = b.chain_schedule(None, 0)
    assert 0 < n < 4096
    rows = np.zeros((n, 6), dtype=np.int32)
    assert b.chain_schedule(rows.ctypes.data_as(_abi.c_i32p), n) == n
    return [tuple(int(v) for v in r) for r in rows]


def position(ev, type_, **kw):
    names = dict(column=1, gap=2, k=3, c2=4, aux=5)
    hits = [i for i, e in enumerate(ev) if e[0] == type_ and all(e[names[a]] == v for a, v in kw.items())]
    assert len(hits) == 1, (type_, kw, hits)
    return hits[0]


def test_every_pair_once_and_the_hops_marked():
    ev = events()
    pairs = [(e[3], e[4]) for e in ev if e[0] in (UPDATE, HOP)]
    assert sorted(pairs) == [(k, c2) for k in range(15) for c2 in range(k + 1, 16)] and len(pairs) == 120
    for e in ev:
        if e[0] in (UPDATE, HOP):
            assert (e[0] == HOP) == (e[4] == e[3] + 1), e          # c2 = k + 1 is the v_readlane hop and nothing else is
    assert [e[1] for e in ev if e[0] == PIVOT] == list(range(16))  # the columns in order, one pivot read each
    assert [e[1] for e in ev if e[0] == HOP] == list(range(15))


def test_an_entry_takes_its_updates_in_column_order_before_its_pivot_is_read():
    ev = events()
    for c2 in range(1, 16):
        at = [(i, e[3]) for i, e in enumerate(ev) if e[0] in (UPDATE, HOP) and e[4] == c2]
        assert [k for _, k in at] == list(range(c2)), (c2, at)     # increasing k; the hop, k = c2 - 1, last
        assert ev[at[-1][0]][0] == HOP
        assert at[-1][0] < position(ev, PIVOT, column=c2), c2


def test_updates_follow_their_column_and_its_strip_store():
    ev = events()
    for i, e in enumerate(ev):
        if e[0] == UPDATE:
            k, c2 = e[3], e[4]
            store = position(ev, STORE, column=k)
            load = position(ev, LOAD, k=k, c2=c2)
            assert store < load < i, e                               # l(k) stored, then m(k, c2) read back, then used
            assert ev[load][5] == 16 * k + c2 and ev[store][5] == 16 * k
            assert position(ev, PIVOT, column=k) < store and k + 1 <= e[1] <= c2 - 1, e
        if e[0] == HOP:
            assert position(ev, PIVOT, column=e[3]) < i < position(ev, PIVOT, column=e[4])
    assert sum(1 for e in ev if e[0] == LOAD) == 105 and sum(1 for e in ev if e[0] == STORE) == 14


def test_no_strip_is_rewritten_before_its_last_reader():
    """Every lane stores: column k's store covers the doubles [16 k, 16 k + 64), its own strip and the next three.  A strip's reads
    must see its own column's store and nothing later."""
    ev = events()
    top = 0
    for i, e in enumerate(ev):
        if e[0] == STORE:
            assert e[4] - e[5] == 64 and e[5] == 16 * e[3]
            top = max(top, e[4])
        if e[0] == LOAD:
            writers = [j for j, w in enumerate(ev) if w[0] == STORE and w[5] <= e[5] < w[4]]
            before = [j for j in writers if j < i]
            assert before and ev[before[-1]][3] == e[3], e             # the last store that touched it is column k's own ...
            assert all(j < i for j in writers), e                      # ... and no store touches it afterwards (within the panel)
    assert top == 272                                                  # kChainStripDoubles: the doubles a wave's strips take
    # the next panel starts over at strip 0: by then every read of this panel is behind (LDS operations of a wave execute in order)
    assert max(i for i, e in enumerate(ev) if e[0] == LOAD) < position(ev, PIVOT, column=15)


def test_the_gaps_are_balanced():
    ev = events()
    per_gap, per_col = {}, {}
    for e in ev:
        if e[0] == UPDATE:
            assert 0 <= e[2] < 8
            per_gap[(e[1], e[2])] = per_gap.get((e[1], e[2]), 0) + 1
            per_col[e[1]] = per_col.get(e[1], 0) + 1
    assert max(per_gap.values()) <= MAX_PER_GAP, per_gap
    assert sorted(per_col) == list(range(1, 15)) and max(per_col.values()) <= MAX_PER_COLUMN and min(per_col.values()) >= 7, per_col
    # multipliers in flight: a column's and the next one's, 16 doubles at the most
    assert max(sum(1 for e in ev if e[0] == LOAD and e[1] == c) for c in range(14)) <= MAX_PER_COLUMN
