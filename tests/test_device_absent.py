"""The closed form of the timeout `every e1=A[c1] -> not B[c2] for W` on interleaved device batches
(sm_app_process_device_events, fast_path 11: kernels/seqpath.hip fast_absent, absent_dev.h) against the CPU oracle fed
the same events. Every A row passing c1 is emitted with timestamp ts + W at the first row (any row, a heartbeat or a row
of the unread stream included) whose playback clock reaches that time, unless a B row of its partition instance passing
c2 arrives before; the product carries the open partials and the instances' creation ordinals across batches and
advances the playback clock. Every case compares the e1 ordinals of the whole stream, in order, and the delivered events
(values, timestamps, visible refs, order) with the oracle's, and checks the path taken. Inputs: 20 000 events or fewer,
3 streams and heartbeat rows, 50 keys or fewer."""
import numpy as np
import pytest

from test_device_mseq import NAMES, Run, events, oracle_out, send_rows

pytestmark = pytest.mark.gpu

BY_SYMBOL = {"A": "symbol", "B": "symbol"}


def text(a="A", b="B", keys=None, wait="5 milliseconds", c1="[price>20]", c2="[price>45]", select="e1.timestamp as i",
         kt="int", playback=True, having=""):
    schema = "".join(f"define stream {s} (symbol {kt}, price double, volume long, timestamp long); " for s in NAMES)
    q = (f"@info(name='q') from every e1={a}{c1} -> not {b}{c2} for {wait} select {select} {having} "
         "insert into OutputStream;")
    head = ("@app:playback " if playback else "") + schema
    if keys is None:
        return head + q
    return head + "partition with (" + ", ".join(f"{x} of {s}" for s, x in keys.items()) + f") begin {q} end;"


def e1_of(out):
    return np.array([r[2][0] for r in out["streams"].get("OutputStream", [])], dtype=np.int64)


def due_of(out, ts):
    """The position at which each expected output fires: the first row whose clock reaches its timestamp."""
    d = np.array([r[0] for r in out["streams"].get("OutputStream", [])], dtype=np.int64)
    return np.searchsorted(np.maximum.accumulate(ts), d, side="left")


class AbsRun(Run):
    """Run with the device matches read as single words: e1's ordinal."""

    def piece(self, sid, cols, ts, lo, hi, ords=None):
        t = self.torch
        up = lambda a: t.from_numpy(np.ascontiguousarray(a[lo:hi])).to(self.dev)
        tsid, tts, tcols = up(sid), up(ts), [up(c) for c in cols]
        t.cuda.synchronize()
        self.app.process_device_events(tsid, tts, tcols, ordinal_base=lo)
        self.keep = (tsid, tts, tcols)
        self.paths.append(int(self.app.get_stat("fast_path:q")))
        assert self.app.get_stat("match_arity:q") == 1
        got = self.app.device_rows_host("q").view(np.int32).astype(np.int64) + lo
        self.tuples.append(got)
        return got


def run(app_text, sid, cols, ts, ranges, **options):
    r = AbsRun(app_text, **options)
    for lo, hi in ranges:
        r.piece(sid, cols, ts, lo, hi)
    got, out, state = r.finish()
    return got, out, r.paths, state


def pieces(n, size, upto=None):
    upto = n if upto is None else min(upto, n)
    r = [(lo, min(lo + size, upto)) for lo in range(0, upto, size)]
    return r + ([(upto, n)] if upto < n else [])


def check(t, sid, cols, ts, ranges, floor=300, **options):
    exp_out = oracle_out(t, sid, cols, ts)
    exp = e1_of(exp_out)
    assert len(exp) >= floor
    got, out, paths, state = run(t, sid, cols, ts, ranges, **options)
    assert set(paths) == {11} and state == 0
    np.testing.assert_array_equal(got, exp)
    assert out == exp_out  # values, timestamps, visible refs and order of the delivered events
    return exp_out


# ---- 1. batches

@pytest.mark.parametrize("keyed", [True, False])
def test_one_batch_and_ragged_pieces(keyed):
    """One batch; pieces of 1023, 1025, 8191 and 8193 rows. Due points fall on heartbeat rows, on rows of the unread
    stream and in a later piece than their e1."""
    sid, cols, ts = events(K=50 if keyed else 1)
    t = text(keys=BY_SYMBOL if keyed else None)
    n = len(ts)
    exp_out = check(t, sid, cols, ts, [(0, n)])
    p = due_of(exp_out, ts)
    assert (sid[p] == -1).sum() >= 10 and (sid[p] == 2).sum() >= 10
    for size in (1023, 1025, 8191, 8193):
        firsts = np.arange(size, n, size)
        if size < 2000:  # (8191 and 8193 cut the stream twice only)
            assert (np.searchsorted(firsts, e1_of(exp_out), "right") < np.searchsorted(firsts, p, "right")).any()
        check(t, sid, cols, ts, pieces(n, size))


@pytest.mark.parametrize("keyed", [True, False])
def test_pieces_of_1_and_37_rows(keyed):
    sid, cols, ts = events(n=6000, K=10 if keyed else 1)
    t = text(keys=BY_SYMBOL if keyed else None)
    check(t, sid, cols, ts, pieces(len(ts), 37, 2500), floor=100)
    check(t, sid, cols, ts, pieces(len(ts), 1, 300), floor=100)


@pytest.mark.parametrize("keyed", [True, False])
def test_cuts_between_an_e1_and_its_due_point_and_its_cancelling_row(keyed):
    """Also a cut in front of a due point: the partial fires on the next batch's first row."""
    sid, cols, ts = events(K=50 if keyed else 1)
    sym, price = cols[0], cols[1]
    t = text(keys=BY_SYMBOL if keyed else None, wait="40 milliseconds" if keyed else "5 milliseconds")
    W = 40 if keyed else 5
    exp_out = oracle_out(t, sid, cols, ts)
    e1, p = e1_of(exp_out), due_of(exp_out, ts)
    k = int(np.argmax(p - e1 > 3) + len(e1) // 3)
    k = int(np.nonzero(p[k:] - e1[k:] > 3)[0][0]) + k
    cut1 = int(e1[k]) + 2  # between an emitted e1 and its due point
    assert e1[k] < cut1 <= p[k]
    # a cancelled e1 and its cancelling row, behind cut1
    emitted = set(e1.tolist())
    cut2 = None
    for i in np.nonzero((sid == 0) & (price > 20))[0]:
        if i <= p[k] or int(i) in emitted:
            continue
        j = np.nonzero((sid == 1) & (price > 45) & (np.arange(len(sid)) > i) & ((sym == sym[i]) | (not keyed)))[0]
        if len(j) and ts[j[0]] < ts[i] + W and j[0] - i > 2:
            cut2 = int(i) + 1
            break
    assert cut2 is not None and cut1 < cut2
    cut3 = int(p[(p > cut2 + 1) & (p - e1 > 1)][0])  # a due point as the next batch's first row
    assert cut2 < cut3 < len(ts)
    check(t, sid, cols, ts, [(0, cut1), (cut1, cut2), (cut2, cut3), (cut3, len(ts))], floor=100)


def test_a_jump_in_time_makes_many_keys_due_at_one_position():
    """After a quiet stretch one row jumps ahead: the partials of at least 20 instances fall due at its position and come
    out in the order the instances were created, some of them by rows of B. Also cut in front of the jump."""
    sid, cols, ts = events(n=8000, K=50)
    ts = ts.copy()
    ts[4000:] = ts[3999] + 1000 + (ts[4000:] - ts[4000])
    ts[3700:4000] = ts[3699]  # the clock stands still: no partial of these rows is due before the jump
    t = text(keys=BY_SYMBOL, wait="40 milliseconds")
    exp_out = oracle_out(t, sid, cols, ts)
    e1, p = e1_of(exp_out), due_of(exp_out, ts)
    at = e1[p == 4000]
    keys = cols[0][at]
    assert len(np.unique(keys)) >= 20
    read = np.nonzero(np.isin(sid, [0, 1]))[0]
    first = {int(k): int(read[cols[0][read] == k][0]) for k in np.unique(keys)}
    assert sum(sid[first[int(k)]] == 1 for k in np.unique(keys)) >= 3  # created by a B row
    order = [first[int(k)] for k in keys]
    assert order == sorted(order) and len(set(order)) >= 20
    for ranges in ([(0, len(ts))], [(0, 4000), (4000, len(ts))], [(0, 3950), (3950, 4001), (4001, len(ts))]):
        got, out, paths, state = run(t, sid, cols, ts, ranges)
        assert set(paths) == {11} and state == 0
        np.testing.assert_array_equal(got, e1)
        assert out == exp_out


# ---- 2. keys and forms

@pytest.mark.parametrize("remap", [-1, 1])
def test_long_keys_negative_and_wide(remap):
    sid, cols, ts = events(K=50)
    sym = (cols[0].astype(np.int64) - 25) * (1 << 40) + 7
    cols = (sym, cols[1], cols[2], cols[3])
    t = text(keys=BY_SYMBOL, kt="long")
    check(t, sid, cols, ts, pieces(len(ts), 7000), **({} if remap < 0 else {"key_remap": remap}))


def test_per_stream_keys():
    """A rows are keyed by symbol, B rows by volume."""
    sid, cols, ts = events(K=50)
    cols = (cols[0], cols[1], cols[2] % 50, cols[3])
    check(text(keys={"A": "symbol", "B": "volume"}), sid, cols, ts, pieces(len(ts), 6001))


@pytest.mark.parametrize("keyed", [True, False])
def test_the_same_stream_cancels(keyed):
    sid, cols, ts = events(K=50 if keyed else 1)
    t = text("A", "A", keys={"A": "symbol"} if keyed else None, wait="40 milliseconds" if keyed else "2 milliseconds",
             c2="[price>45]" if keyed else "[price>55]")
    check(t, sid, cols, ts, pieces(len(ts), 6001), floor=100)


@pytest.mark.parametrize("keyed", [True, False])
def test_no_filters_and_more_select_values(keyed):
    sid, cols, ts = events(K=50 if keyed else 1)
    t = text(keys=BY_SYMBOL if keyed else None, wait="2 milliseconds", c1="", c2="[price > 30.0 and volume != 1000]",
             select="e1.timestamp as i, e1.price as p, e1.volume + 1 as v, 7 as c")
    check(t, sid, cols, ts, pieces(len(ts), 9000))


@pytest.mark.parametrize("keyed", [True, False])
def test_snapshot_restore_between_pieces(keyed):
    sid, cols, ts = events(K=50 if keyed else 1)
    t = text(keys=BY_SYMBOL if keyed else None, wait="40 milliseconds" if keyed else "5 milliseconds")
    exp_out = oracle_out(t, sid, cols, ts)
    e1, p = e1_of(exp_out), due_of(exp_out, ts)
    k = int(np.nonzero((e1 > 9000) & (p - e1 > 2))[0][0])
    cut = int(e1[k]) + 1  # behind an e1 whose due point lies further on
    assert ((e1 < cut) & (p >= cut)).sum() >= (3 if keyed else 1) and len(e1) >= 100
    a = AbsRun(t)
    first = a.piece(sid, cols, ts, 0, cut)
    snap = a.app.snapshot()
    a.app.close()
    b = AbsRun(t)
    b.app.restore(snap)
    second = b.piece(sid, cols, ts, cut, len(ts))
    b.app.close()
    assert a.paths == [11] and b.paths == [11]
    np.testing.assert_array_equal(np.concatenate([first, second]), e1)


def test_device_project_and_timing_labels():
    sid, cols, ts = events(K=50)
    t = text(keys=BY_SYMBOL, select="e1.timestamp as i, e1.price as p")
    rows = oracle_out(t, sid, cols, ts)["streams"]["OutputStream"]
    r = AbsRun(t, fast_timing=1)
    got = []
    for lo, hi in pieces(len(ts), 7000):
        r.piece(sid, cols, ts, lo, hi)
        vals, nulls, ots = r.app.device_project("q")
        r.torch.cuda.synchronize()
        assert not nulls.any()
        got += [[t_, v[0], float(np.array([v[1]], np.int64).view(np.float64)[0])]
                for t_, v in zip(ots.cpu().tolist(), vals.cpu().tolist())]
    for label in ("absent_facts", "absent_pack", "absent_sort", "absent_next", "absent_state", "absent_count",
                  "absent_scan", "absent_emit", "absent_order", "absent_project", "absent_carry"):
        assert r.app.get_stat(f"kernel_calls:{label}") == 1, label
    assert set(r.paths) == {11}
    r.app.close()
    assert got == [[row[0], row[1][0], row[1][1]] for row in rows] and len(rows) >= 300


# ---- 3. outside the envelope: the NFA kernel, as before

def test_c2_reading_e1_a_having_and_no_playback():
    sid, cols, ts = events(n=6000, K=10)
    ranges = [(0, 2500), (2500, 6000)]
    for t in (text(keys=BY_SYMBOL, c2="[price>e1.price]"),
              text(keys=BY_SYMBOL, having="having i > 100")):
        exp_out = oracle_out(t, sid, cols, ts)
        assert len(exp_out["streams"]["OutputStream"]) >= 100
        r = AbsRun(t)
        paths = []
        for lo, hi in ranges:
            up = lambda a: r.torch.from_numpy(np.ascontiguousarray(a[lo:hi])).to(r.dev)
            r.app.process_device_events(up(sid), up(ts), [up(c) for c in cols], ordinal_base=lo)
            paths.append(int(r.app.get_stat("fast_path:q")))
        assert 11 not in paths and r.app.outputs() == exp_out
        r.app.close()
    from siddhi_amd.testing import EngineError
    with pytest.raises(EngineError, match="playback"):
        AbsRun(text(keys=BY_SYMBOL, playback=False))


# ---- 4. hand-over

@pytest.mark.parametrize("keyed", [True, False])
def test_staged_sends_before_and_after_device_events(keyed):
    sid, cols, ts = events(n=6000, K=10 if keyed else 1, heartbeats=0.0)
    t = text(keys=BY_SYMBOL if keyed else None, wait="40 milliseconds" if keyed else "5 milliseconds")
    exp_out = oracle_out(t, sid, cols, ts)
    e1, p = e1_of(exp_out), due_of(exp_out, ts)
    n = len(ts)
    assert len(e1) >= 100
    # staged, then device: the NFA kernel holds the state
    r = AbsRun(t)
    send_rows(r.app, sid, cols, ts, 0, 40)
    tail = r.piece(sid, cols, ts, 40, n)
    assert r.paths == [5]
    _, out, state = r.finish()
    assert state == 1 and out == exp_out
    np.testing.assert_array_equal(tail, e1[p >= 40])
    # device, staged, device: the flush replays the carried e1 rows into the NFA, which keeps the query
    k = int(np.nonzero((p - e1 > 2) & (e1 > n // 2))[0][0])
    a = int(e1[k]) + 1
    b = a + 40
    assert ((e1 < a) & (p >= a)).any()  # a handed-over partial falls due
    r = AbsRun(t)
    first = r.piece(sid, cols, ts, 0, a)
    assert r.paths == [11] and r.app.get_stat("nfa_state:q") == 0
    send_rows(r.app, sid, cols, ts, a, b)
    r.app.flush()
    assert r.app.get_stat("nfa_state:q") == 1
    last = r.piece(sid, cols, ts, b, n)
    assert r.paths == [11, 5]
    _, out, state = r.finish()
    assert state == 1 and out == exp_out
    np.testing.assert_array_equal(first, e1[p < a])
    np.testing.assert_array_equal(last, e1[p >= b])


@pytest.mark.parametrize("keyed", [True, False])
def test_a_read_row_below_the_clock_hands_over(keyed):
    """The second piece has a read row below the clock: FAST_NON_MONOTONE, the NFA kernel takes the query over for good
    with the carried partials. Before that row the stream has a stretch longer than W without cancelling rows, and the
    step back is smaller than W, so neither lastArrivalTime nor a cancelled partial's timer can change an output."""
    sid, cols, ts = events(K=50 if keyed else 1)
    W = 40 if keyed else 5
    sid, price, ts = sid.copy(), cols[1].copy(), ts.copy()
    lo = 9000
    hi = int(np.searchsorted(ts, ts[lo] + W + 2)) + 1
    quiet = np.arange(lo, hi)
    price[quiet] = np.minimum(price[quiet], 40.0)  # no cancelling row
    i = hi + int(np.nonzero(sid[hi:] == 0)[0][0])
    assert ts[i] - (W // 2) < ts[i - 1]
    ts[i] -= W // 2
    assert ts[i] < np.maximum.accumulate(ts)[i]
    cols = (cols[0], price, cols[2], cols[3])
    t = text(keys=BY_SYMBOL if keyed else None, wait=f"{W} milliseconds")
    exp_out = oracle_out(t, sid, cols, ts)
    e1 = e1_of(exp_out)
    assert len(e1) >= 300
    got, out, paths, state = run(t, sid, cols, ts, [(0, 8000), (8000, 14000), (14000, 20000)])
    assert paths == [11, 5, 5] and state == 1
    np.testing.assert_array_equal(got, e1)
    assert out == exp_out
