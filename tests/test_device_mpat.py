"""The closed form of the pattern over two streams, `every e1=A[c1] -> e2=B[c2] within T` (streams of one schema), on
interleaved device batches (sm_app_process_device_events, fast_path 9: kernels/seqpath.hip fast_pat_ms, mpat_dev.h)
against the CPU oracle fed the same events. Every A event passing c1 waits for the first later B event of its partition
instance that passes c2, inside T; one e2 may complete many partials, oldest e1 first; the product carries the open
partials' e1 rows across batches. Every case compares the (e1, e2) ordinals of the whole stream, pair for pair and in
order, with the oracle's, checks the path taken, and asserts a floor of expected outputs that the oracle alone reaches.
Inputs: 20 000 events or fewer, 3 streams and heartbeat rows, 50 keys or fewer."""
import ctypes
import struct

import numpy as np
import pytest

from test_device_mseq import (NAMES, Run, events, oracle_on_read_rows, oracle_out, run, send_rows, straddling, tuples_of,
                              unread_rows_going_back)

pytestmark = pytest.mark.gpu

C2 = "price > e1.price"
C2_COMPOUND = "price > e1.price - 25.0 and volume != e1.volume"
T_KEYED, T_FLAT = 150, 10  # ms: about three events of a key out of 50, about ten events of the flat stream


def text(a="A", b="B", keys=None, within=T_KEYED, c2=C2, select=None, kt="int", c1="[price>20]"):
    schema = "".join(f"define stream {s} (symbol {kt}, price double, volume long, timestamp long); " for s in NAMES)
    w = "" if within is None else f" within {within} milliseconds"
    sel = select or "select e1.timestamp as i1, e2.timestamp as i2"
    q = f"@info(name='q') from every e1={a}{c1} -> e2={b}[{c2}]{w} {sel} insert into OutputStream;"
    if keys is None:
        return schema + q
    return schema + "partition with (" + ", ".join(f"{x} of {s}" for s, x in keys.items()) + f") begin {q} end;"


BY_SYMBOL = {"A": "symbol", "B": "symbol"}
PER_STREAM = {"A": "symbol", "B": "volume"}


def case(kind, K=50, **kw):
    """(text, sid, cols, ts) of a form: flat, keyed by symbol, or B keyed by its volume."""
    if kind == "flat":
        sid, cols, ts = events(K=1)
        return text(keys=None, **dict({"within": T_FLAT}, **kw)), sid, cols, ts
    sid, cols, ts = events(K=K)
    if kind == "per_stream":
        cols = (cols[0], cols[1], cols[2] % 50, cols[3])
        return text(keys=PER_STREAM, **kw), sid, cols, ts
    return text(keys=BY_SYMBOL, **kw), sid, cols, ts


def cuts_inside_pairs(exp, n, extra=()):
    """Pieces cut between e1 and e2 of expected pairs (one in each third of the stream), plus `extra` cuts."""
    far = exp[exp[:, 1] - exp[:, 0] > 1]
    cuts = {int(far[len(far) // 4, 1]), int(far[len(far) // 2, 1]), int(far[3 * len(far) // 4, 1])} | set(extra)
    cuts = sorted(c for c in cuts if 0 < c < n)
    return list(zip([0] + cuts, cuts + [n]))


# ---- 1. batches

@pytest.mark.parametrize("kind", ["flat", "symbol", "per_stream"])
def test_one_batch_and_ragged_pieces(kind):
    """One batch; then pieces of 1, 1023, 1025, 8191 and 8193 rows and cuts between an expected pair's e1 and e2."""
    t, sid, cols, ts = case(kind)
    exp_out = oracle_out(t, sid, cols, ts)
    exp = tuples_of(exp_out, 2)
    n = len(ts)
    assert len(exp) >= 300
    ranges = cuts_inside_pairs(exp, n, extra=(1, 1024, 2049) + tuple(range(2500, n, 500)))
    assert {hi - lo for lo, hi in ranges} >= {1, 1023, 1025} and straddling(exp, ranges) >= 20
    got, out, paths, state = run(t, sid, cols, ts, [(0, n)])
    assert paths == [9] and state == 0
    np.testing.assert_array_equal(got, exp)
    assert out == exp_out
    got, out, paths, state = run(t, sid, cols, ts, ranges)
    assert set(paths) == {9} and state == 0
    np.testing.assert_array_equal(got, exp)
    assert out == exp_out  # values, timestamps, visible refs and order of the delivered events
    # exactly 8191 and 8193 rows
    ranges = [(0, 8191), (8191, 8191 + 8193), (8191 + 8193, n)]
    got, _, paths, _ = run(t, sid, cols, ts, ranges)
    assert paths == [9, 9, 9]
    np.testing.assert_array_equal(got, exp)


def test_many_small_pieces():
    t, sid, cols, ts = case("symbol")
    exp = tuples_of(oracle_out(t, sid, cols, ts), 2)
    n = len(ts)
    ranges = [(lo, min(lo + 37, 3000)) for lo in range(0, 3000, 37)] + [(3000, n)]
    assert straddling(exp, ranges) >= 20
    got, _, paths, _ = run(t, sid, cols, ts, ranges)
    assert set(paths) == {9}
    np.testing.assert_array_equal(got, exp)


# ---- 2. rows that must be ignored, conditions, windows

@pytest.mark.parametrize("keyed", [True, False])
def test_heartbeats_and_unread_rows_between_members(keyed):
    sid, cols, ts = events(K=50 if keyed else 1, heartbeats=0.3)
    t = text(keys=BY_SYMBOL if keyed else None, within=T_KEYED if keyed else T_FLAT)
    exp = tuples_of(oracle_out(t, sid, cols, ts), 2)
    assert len(exp) >= 30
    between = [sid[a + 1:b] for a, b in exp]
    assert any((x == -1).any() for x in between) and any((x == 2).any() for x in between)
    ranges = cuts_inside_pairs(exp, len(ts))
    got, _, paths, _ = run(t, sid, cols, ts, ranges)
    assert set(paths) == {9}
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("kind", ["flat", "symbol"])
@pytest.mark.parametrize("c2,within", [(C2_COMPOUND, None), ("price > 45", None), (C2, 0), (C2_COMPOUND, 0)])
def test_compound_c2_many_partials_per_e2_and_within_0(c2, within, kind):
    """within None: the form's default window. `price > 45` does not read e1: one e2 completes many partials."""
    kw = {"c2": c2} if within is None else {"c2": c2, "within": within, "K": 3}  # (3 keys: enough pairs within 0 ms)
    t, sid, cols, ts = case(kind, **kw)
    exp = tuples_of(oracle_out(t, sid, cols, ts), 2)
    assert len(exp) >= 30
    if c2 == "price > 45":
        assert np.unique(exp[:, 1], return_counts=True)[1].max() >= 4
    ranges = cuts_inside_pairs(exp, len(ts)) if within is None else [(0, 7000), (7000, 7001), (7001, len(ts))]
    got, _, paths, _ = run(t, sid, cols, ts, ranges)
    assert set(paths) == {9}
    np.testing.assert_array_equal(got, exp)


def test_other_direction_and_third_stream_as_e1():
    sid, cols, ts = events(K=50)
    for a, b in (("B", "A"), ("C", "A")):
        t = text(a, b, {a: "symbol", b: "symbol"})
        exp = tuples_of(oracle_out(t, sid, cols, ts), 2)
        assert len(exp) >= 30
        got, _, paths, _ = run(t, sid, cols, ts, cuts_inside_pairs(exp, len(ts)))
        assert set(paths) == {9}
        np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("keyed", [True, False])
def test_unread_rows_going_back_in_time_between_e1_and_e2(keyed):
    """Three batches: 1025 rows (one more than a tile) of A that leave open partials, 65 rows of C and heartbeats whose
    event times decrease and lie before the first batch's, and 1025 rows of B, in time order after the first batch, that
    complete the partials. The batch without a read row neither reports decreasing time nor moves the carried time: every
    batch stays on the closed form, and the pairs, all of which straddle the middle batch, are the oracle's on the
    read rows."""
    n1 = 1025
    rng = np.random.default_rng(23)
    a_sid = np.zeros(n1, np.int32)
    a_sid[::16] = -1
    step = np.arange(n1, dtype=np.int64) // 16
    sid = np.concatenate([a_sid, np.ones(n1, np.int32)])
    sym = rng.integers(0, 5 if keyed else 1, 2 * n1).astype(np.int32)
    price = np.concatenate([21.0 + np.round(rng.random(n1) * 19.0, 1), 30.0 + np.round(rng.random(n1) * 30.0, 1)])
    vol = rng.integers(0, 2000, 2 * n1).astype(np.int64)
    ts = 1000 + np.concatenate([step, step[-1] + step])  # the third batch starts at the first one's last event time
    sid, cols, ts = unread_rows_going_back(sid, (sym, price, vol), ts, n1)
    ranges = [(0, n1), (n1, n1 + 65), (n1 + 65, len(ts))]
    assert (np.diff(ts[n1:n1 + 65]) < 0).all() and ts[n1] < ts[0] and ts[n1 + 65] == ts[n1 - 1]
    assert not np.isin(sid[n1:n1 + 65], [0, 1]).any()
    t = text(keys=BY_SYMBOL if keyed else None)  # (T_KEYED: longer than the stream)
    exp = tuples_of(oracle_on_read_rows(t, sid, cols, ts, [0, 1]), 2)
    across = straddling(exp, ranges)
    assert across == len(exp) >= 900  # (960 A rows pass c1; a B row with a higher price follows each inside T)
    got, _, paths, state = run(t, sid, cols, ts, ranges)
    assert paths == [9, 9, 9] and state == 0
    np.testing.assert_array_equal(got, exp)
    assert straddling(got, ranges) >= across


# ---- 3. keys and ordinals

@pytest.mark.parametrize("remap", ["auto", "off", "on"])
def test_long_keys_negative_and_wide(remap):
    """LONG keys, negative values, a span above 2^20: dense ids by themselves (the first batch's span), the key values
    (option key_remap = 0: more sort passes), or dense ids from the start."""
    sid, cols, ts = events(K=40)
    sym = (cols[0].astype(np.int64) - 20) * 3_000_011
    assert sym.min() < 0 and sym.max() - sym.min() > 1 << 20
    cols = (sym, cols[1], cols[2], cols[3])
    t = text(keys=BY_SYMBOL, kt="long")
    exp = tuples_of(oracle_out(t, sid, cols, ts), 2)
    assert len(exp) >= 30
    opts = {} if remap == "auto" else {"key_remap": 1 if remap == "on" else 0}
    ranges = cuts_inside_pairs(exp, len(ts))
    assert straddling(exp, ranges) >= 3
    got, _, paths, _ = run(t, sid, cols, ts, ranges, **opts)
    assert set(paths) == {9}
    np.testing.assert_array_equal(got, exp)


def test_negative_int_keys():
    sid, cols, ts = events(K=50)
    cols = (cols[0] - 25, cols[1], cols[2], cols[3])
    t = text(keys=BY_SYMBOL)
    exp = tuples_of(oracle_out(t, sid, cols, ts), 2)
    assert len(exp) >= 30 and (cols[0][exp[:, 0]] < 0).any()
    got, _, paths, _ = run(t, sid, cols, ts, cuts_inside_pairs(exp, len(ts)))
    assert set(paths) == {9}
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("keyed", [True, False])
def test_given_ordinals_with_gaps(keyed):
    """Events carrying the global ordinals 3 i + 1, each piece's first ordinal as its base."""
    sid, cols, ts = events(K=50 if keyed else 1)
    ords = 3 * np.arange(len(ts), dtype=np.int64) + 1
    t = text(keys=BY_SYMBOL if keyed else None, within=T_KEYED if keyed else T_FLAT)
    exp = tuples_of(oracle_out(t, sid, cols, ts, ords), 2)
    assert len(exp) >= 30 and (exp % 3 == 1).all()
    ranges = cuts_inside_pairs((exp - 1) // 3, len(ts))
    got, _, paths, _ = run(t, sid, cols, ts, ranges, ords=ords)
    assert set(paths) == {9}
    np.testing.assert_array_equal(got, exp)


# ---- 4. a hot key and long scans

def hot_key_stream():
    """3440 A rows of key 7 (C rows and heartbeats between them), then one B row of key 7 that completes them all."""
    n = 4400
    sid = np.zeros(n, np.int32)
    sid[5::10] = 2
    sid[8::10] = -1
    sym = np.full(n, 7, np.int32)
    price = np.full(n, 30.0)
    vol = np.arange(n, dtype=np.int64)
    ts = np.arange(n, dtype=np.int64) // 50
    sid[4300] = 1
    price[4300] = 50.0
    sid[4390] = 1
    price[4390] = 25.0  # fails c2 for the partials behind row 4300
    sym[4350:4380] = 3  # another key's partials
    return sid, (sym, price, vol, np.arange(n, dtype=np.int64)), ts


@pytest.mark.parametrize("keyed", [True, False])
def test_one_e2_completes_3000_carried_and_batch_partials(keyed):
    sid, cols, ts = hot_key_stream()
    t = text(keys=BY_SYMBOL if keyed else None)
    exp = tuples_of(oracle_out(t, sid, cols, ts), 2)
    ranges = [(0, 2000), (2000, len(ts))]
    one = exp[exp[:, 1] == 4300]
    assert len(one) >= 3000 and (one[:, 0] < 2000).sum() >= 1000 and (one[:, 0] >= 2000).sum() >= 1000
    got, _, paths, _ = run(t, sid, cols, ts, ranges)
    assert paths == [9, 9]
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("keyed", [True, False])
def test_scans_longer_than_the_private_budget_and_a_wave_step(keyed):
    """Partials whose e2 lies 97 .. 1500 sorted positions ahead (the lane's own budget is 16 positions, a wave step 64),
    among B rows that fail c2."""
    n = 4100
    rng = np.random.default_rng(17)
    sid = np.ones(n, np.int32)
    sym = np.full(n, 3, np.int32)
    price = np.full(n, 10.0)
    sid[rng.random(n) < 0.1] = -1
    starts = [0, 100, 1200, 1300, 2500]
    dist = [97, 98, 161, 1090, 1500]
    for k, (s, d) in enumerate(zip(starts, dist)):  # the k-th partial's e2 passes c2 for it and fails for the later ones
        sid[s], price[s] = 0, 50.0 + k
        sid[s + d], price[s + d] = 1, 50.5 + k
    vol = np.arange(n, dtype=np.int64)
    ts = np.arange(n, dtype=np.int64) // 100
    cols = (sym, price, vol, np.arange(n, dtype=np.int64))
    t = text(keys=BY_SYMBOL if keyed else None, c1="[price>35]")
    exp = tuples_of(oracle_out(t, sid, cols, ts), 2)
    assert sorted((exp[:, 1] - exp[:, 0]).tolist())[-3:] == [161, 1090, 1500] and len(exp) == 5
    got, _, paths, _ = run(t, sid, cols, ts, [(0, n)])
    assert paths == [9]
    np.testing.assert_array_equal(got, exp)
    got, _, paths, _ = run(t, sid, cols, ts, [(0, 1250), (1250, 2000), (2000, n)])  # carried partials scan far too
    assert paths == [9, 9, 9]
    np.testing.assert_array_equal(got, exp)


# ---- 5. hand-over to the NFA kernel

RANGES3 = [(0, 8000), (8000, 14000), (14000, 20000)]


@pytest.mark.parametrize("case_", ["inside", "before_carry"])
@pytest.mark.parametrize("keyed", [True, False])
def test_decreasing_time_hands_over(case_, keyed):
    """Event time decreases inside the second piece, or from the first piece to the second: FAST_NON_MONOTONE, the NFA
    kernel takes the query over for good with the carried partials. The window is longer than the stream, so that no
    partial was dropped as expired before the hand-over (with a shorter window the reference's outputs on decreasing
    time are not the rule's: tests/test_mpat_plan.py)."""
    sid, cols, ts = events(K=50 if keyed else 1)
    ts = ts.copy()
    if case_ == "inside":
        ts[9000:9400] = ts[9000:9400][::-1]
    else:
        ts[8000:] -= 50
    assert (np.diff(ts) < 0).any()
    # (unkeyed, the NFA kernel's one lane walks every open partial at every B event: a c2 that leaves few of them open)
    t = text(keys=BY_SYMBOL if keyed else None, within=30000, c2="price > e1.price + 25.0" if keyed else C2)
    exp_out = oracle_out(t, sid, cols, ts)
    exp = tuples_of(exp_out, 2)
    assert len(exp) >= 30 and straddling(exp, RANGES3) >= (20 if keyed else 2)
    got, out, paths, state = run(t, sid, cols, ts, RANGES3)
    assert paths == [9, 5, 5] and state == 1
    np.testing.assert_array_equal(got, exp)
    assert out == exp_out


@pytest.mark.parametrize("keyed", [True, False])
def test_staged_sends_before_and_after_device_events(keyed):
    sid, cols, ts = events(n=6000, K=10 if keyed else 1, heartbeats=0.0)
    t = text(keys=BY_SYMBOL if keyed else None, within=40 if keyed else T_FLAT)
    exp_out = oracle_out(t, sid, cols, ts)
    exp = tuples_of(exp_out, 2)
    n = len(ts)
    assert len(exp) >= 30
    # staged, then device: the NFA kernel holds the state
    r = Run(t)
    send_rows(r.app, sid, cols, ts, 0, 40)
    tail = r.piece(sid, cols, ts, 40, n)
    assert r.paths == [5] and r.app.get_stat("match_arity:q") == 2
    _, out, state = r.finish()
    assert state == 1 and out == exp_out
    np.testing.assert_array_equal(tail, exp[exp[:, 1] >= 40])
    # device, staged, device: the flush replays the carried e1 rows into the NFA, which keeps the query
    a = next(int(e2) for e1, e2 in exp[len(exp) // 2:] if e2 - e1 > 1)  # in front of a pair's e2
    b = a + 40
    assert ((exp[:, 0] < a) & (exp[:, 1] >= a) & (exp[:, 1] < b)).any()  # a handed-over partial completes
    r = Run(t)
    first = r.piece(sid, cols, ts, 0, a)
    assert r.paths == [9] and r.app.get_stat("nfa_state:q") == 0
    send_rows(r.app, sid, cols, ts, a, b)
    r.app.flush()
    assert r.app.get_stat("nfa_state:q") == 1
    last = r.piece(sid, cols, ts, b, n)
    assert r.paths == [9, 5]
    _, out, state = r.finish()
    assert state == 1 and out == exp_out
    np.testing.assert_array_equal(first, exp[exp[:, 1] < a])
    np.testing.assert_array_equal(last, exp[exp[:, 1] >= b])


def feed_pieces(app_text, sid, cols, ts, ranges, **options):
    """process_device_events over the pieces; (collected outputs, fast_path after each piece)."""
    r = Run(app_text, **options)
    paths = []
    for lo, hi in ranges:
        up = lambda a: r.torch.from_numpy(np.ascontiguousarray(a[lo:hi])).to(r.dev)
        r.app.process_device_events(up(sid), up(ts), [up(c) for c in cols], ordinal_base=lo)
        paths.append(int(r.app.get_stat("fast_path:q")))
    out = r.app.outputs()
    r.app.close()
    return out, paths


def test_keep_outputs_a_second_query_and_no_within_stay_on_the_nfa_route():
    """What ran on the NFA kernel before runs there as before: option keep_outputs, an app with a second query, and the
    same query without a `within` (outside the envelope)."""
    sid, cols, ts = events(n=6000, K=10)
    ranges = [(0, 2500), (2500, 6000)]
    t = text(keys=BY_SYMBOL, within=40)
    exp_out = oracle_out(t, sid, cols, ts)
    assert len(exp_out["streams"]["OutputStream"]) >= 30
    out, paths = feed_pieces(t, sid, cols, ts, ranges, keep_outputs=1)
    assert 9 not in paths and out == exp_out
    two = t.replace(" end;", " @info(name='q2') from every e1=B[price>30] -> e2=A[price>e1.price] within 40 milliseconds "
                             "select e1.timestamp as i1, e2.timestamp as i2 insert into Out2; end;")
    exp_two = oracle_out(two, sid, cols, ts)
    assert len(exp_two["streams"]["Out2"]) >= 30
    out, paths = feed_pieces(two, sid, cols, ts, ranges)
    assert 9 not in paths and out == exp_two
    nw = text(keys=BY_SYMBOL, within=None)
    exp_nw = oracle_out(nw, sid, cols, ts)
    assert len(exp_nw["streams"]["OutputStream"]) >= 30
    out, paths = feed_pieces(nw, sid, cols, ts, ranges)
    assert 9 not in paths and paths[0] == paths[1] and out == exp_nw


# ---- 6. snapshot

@pytest.mark.parametrize("keyed", [True, False])
def test_snapshot_restore_between_e1_and_e2(keyed):
    sid, cols, ts = events(K=50 if keyed else 1)
    t = text(keys=BY_SYMBOL if keyed else None, within=T_KEYED if keyed else T_FLAT)
    exp = tuples_of(oracle_out(t, sid, cols, ts), 2)
    cut = int(exp[exp[:, 1] - exp[:, 0] > 1][len(exp) // 4, 1])
    assert ((exp[:, 0] < cut) & (exp[:, 1] >= cut)).sum() >= (3 if keyed else 1) and len(exp) >= 30
    a = Run(t)
    first = a.piece(sid, cols, ts, 0, cut)
    snap = a.app.snapshot()
    a.app.close()
    b = Run(t)
    b.app.restore(snap)
    second = b.piece(sid, cols, ts, cut, len(ts))
    b.app.close()
    assert a.paths == [9] and b.paths == [9]
    np.testing.assert_array_equal(np.concatenate([first, second]), exp)


# ---- 7. outputs and stats

PSELECT = ("select e1.symbol as k, e1.price as p1, e2.price as p2, e2.volume - e1.volume as dv, "
           "e1.timestamp as i1, e2.timestamp as i2")
PKINDS = ["i", "d", "d", "i", "i", "i"]


def words(row):
    return [struct.unpack("<q", struct.pack("<d", v))[0] if k == "d" else int(v) for v, k in zip(row, PKINDS)]


@pytest.mark.parametrize("keyed", [True, False])
def test_device_project_equals_oracle(keyed):
    sid, cols, ts = events(K=50 if keyed else 1)
    t = text(keys=BY_SYMBOL if keyed else None, within=T_KEYED if keyed else T_FLAT, select=PSELECT)
    rows = oracle_out(t, sid, cols, ts)["streams"]["OutputStream"]
    pairs = np.array([r[1][4:6] for r in rows], dtype=np.int64)
    assert len(pairs) >= 30
    ranges = cuts_inside_pairs(pairs, len(ts))
    assert straddling(pairs, ranges) >= 1  # an e1 read from the carry
    r = Run(t)
    got = []
    for lo, hi in ranges:
        r.piece(sid, cols, ts, lo, hi)
        assert r.app.get_stat("match_arity:q") == 2
        vals, nulls, ots = r.app.device_project("q")
        r.torch.cuda.synchronize()
        assert not nulls.any()
        got += [[t_, v] for t_, v in zip(ots.cpu().tolist(), vals.cpu().tolist())]
    assert set(r.paths) == {9}
    r.app.close()
    assert got == [[row[0], words(row[1])] for row in rows]


def test_callbacks_receive_the_oracles_events():
    """A StreamCallback and a columns callback through SiddhiAppRuntime.sendDeviceEvents: one call per e2, in order of
    it, before the call returns."""
    import torch
    import siddhi_amd
    from siddhi_amd import ColumnsStreamCallback, SiddhiManager, StreamCallback
    sid, cols, ts = events(K=50)
    t = text(keys=BY_SYMBOL, select=PSELECT, c2="price > 45")
    rows = oracle_out(t, sid, cols, ts)["streams"]["OutputStream"]
    assert len(rows) >= 100
    pairs = np.array([r[1][4:6] for r in rows], dtype=np.int64)
    ranges = cuts_inside_pairs(pairs, len(ts))
    assert straddling(pairs, ranges) >= 1
    evs, columns, seen = [], [], []

    class SC(StreamCallback):
        def receive(self, e):
            evs.append([[x.timestamp, x.data] for x in e])

    class CC(ColumnsStreamCallback):
        def receive_columns(self, timestamps, values, null_bits):
            columns.append([timestamps, values, null_bits])

    dev = torch.device("cuda", 0)
    for cb in (SC(), CC()):
        rt = SiddhiManager().createSiddhiAppRuntime(t)
        rt.addCallback("OutputStream", cb)
        rt.start()
        for lo, hi in ranges:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a[lo:hi])).to(dev)
            rt.sendDeviceEvents(up(sid), up(ts), [up(c) for c in cols], ordinal_base=lo)
            v = ctypes.c_double()
            siddhi_amd.check(siddhi_amd.lib().sm_app_get_stat(rt._h, b"fast_path:q", ctypes.byref(v)))
            assert v.value == 9
            seen.append(sum(len(c) for c in evs) + sum(len(c[0]) for c in columns))
        rt.shutdown()
    # one chunk per e2: the outputs one e2 completes arrive together, oldest e1 first
    flat_evs = [e for chunk in evs for e in chunk]
    assert flat_evs == [[r[0], r[1]] for r in rows]
    assert [len(c) for c in evs] == np.unique(pairs[:, 1], return_counts=True)[1].tolist()
    assert max(len(c) for c in evs) >= 2
    assert [w for c in columns for w in c[1]] == [words(r[1]) for r in rows]
    assert [x for c in columns for x in c[0]] == [r[0] for r in rows]
    assert seen[0] == int((pairs[:, 1] < ranges[0][1]).sum())  # delivered before the call returned


def test_match_arity_and_timing_labels():
    sid, cols, ts = events(K=50)
    n = len(ts)
    r = Run(text(keys=BY_SYMBOL), fast_timing=1)
    assert r.app.get_stat("match_arity:q") == 2
    r.piece(sid, cols, ts, 0, n // 2)
    labels = ["mpat_facts", "mpat_pack", "mpat_sort", "mpat_link", "mpat_count", "mpat_scan", "mpat_emit", "mpat_order",
              "mpat_carry"]
    for label in labels:
        assert r.app.get_stat(f"kernel_calls:{label}") == 1
        assert r.app.get_stat(f"kernel_ms:{label}") >= 0
    assert r.app.get_stat("kernel_calls:mseq_link") == 0
    r.piece(sid, cols, ts, n // 2, n)
    assert r.paths == [9, 9]
    r.app.close()
    u = Run(text(within=T_FLAT), fast_timing=1)  # unkeyed, every row read: no pack, no sort
    sid2 = np.where(sid == 0, 0, 1).astype(np.int32)
    u.piece(sid2, cols, ts, 0, n)
    assert u.paths == [9]
    assert u.app.get_stat("kernel_calls:mpat_pack") == 0 and u.app.get_stat("kernel_calls:mpat_sort") == 0
    assert u.app.get_stat("kernel_calls:mpat_link") == 1
    np.testing.assert_array_equal(u.tuples[0], tuples_of(oracle_out(text(within=T_FLAT), sid2, cols, ts), 2))
    u.app.close()
