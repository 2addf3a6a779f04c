"""The plan of the timeout `every e1=A[c1] -> not B[c2] for W` once the compiler marks it for the closed form of
interleaved device batches (compiler.cpp fast_absent, one hidden ordinal ref, e1's, for the NFA hand-over), and the rule
the device kernels (kernels/absent_dev.h) implement, tied to the oracle on the CPU:

    @app:playback. R = {A, B} (B may be A). Positions are rows of the feed, heartbeat rows (-1) and rows of unread streams
    included; clock[q] = the running maximum of ts over all rows up to q. A row of R belongs to the instance of its own
    stream's key attribute. Every A row i with c1(i) opens a partial with deadline d = ts[i] + W. It is cancelled iff a
    row j > i of B exists in the same instance with c2(j) and ts[j] < d; otherwise it is emitted at p(i) = the first
    position q > i with clock[q] >= d, as e1's select values with timestamp d. Outputs in order of (p, creation ordinal
    of the instance, i); an instance is created by the first row of a stream in R with its key.

The numpy statement of that rule equals the oracle's (output timestamp, e1) lists, in order, flat, partitioned by one
attribute and by an attribute per stream, for five waiting times, on three seeds, with heartbeat rows, for `A -> not A`,
without filters, with a compound c2 and with a partition that also keys the unread stream. Two cases stay outside: a c2
that reads e1, and read rows below the clock; there the oracle differs from the rule. Also the compiler's envelope for the
mark. Test infrastructure: no GPU; `-m "not gpu"`."""
import numpy as np
import pytest

from test_mseq_plan import NAMES, SCHEMA, KEYCOL, decreasing_ts, per_stream_cols, stream
from oracle_lib import OracleApp

C1 = {"gt20": ("[price>20]", lambda p, v: p > 20), "none": ("", lambda p, v: np.ones(len(p), bool))}
C2 = {
    "gt45": ("[price>45]", lambda p, v: p > 45),
    "gt59_5": ("[price>59.5]", lambda p, v: p > 59.5),  # rare: partials survive a second
    "gt70": ("[price>70]", lambda p, v: p > 70),
    "compound": ("[price > 30.0 and volume != 1000 or price < 3.0]", lambda p, v: ((p > 30.0) & (v != 1000)) | (p < 3.0)),
    "none": ("", lambda p, v: np.ones(len(p), bool)),
}
WAITS = {"1": 1, "2": 2, "5": 5, "40": 40, "1sec": 1000}


def wait_text(w):
    return "1 sec" if w == "1sec" else f"{w} milliseconds"


def absent_text(a, b, keys=None, wait="5", c1="gt20", c2="gt45", select="e1.timestamp as i", playback=True):
    """keys: {stream: key attribute} (None: unpartitioned)."""
    q = (f"@info(name='q') from every e1={a}{C1[c1][0]} -> not {b}{C2[c2][0]} for {wait_text(wait)} select {select} "
         "insert into OutputStream;")
    head = ("@app:playback " if playback else "") + SCHEMA
    if keys is None:
        return head + q
    return head + "partition with (" + ", ".join(f"{x} of {s}" for s, x in keys.items()) + f") begin {q} end;"


def row_keys(sid, cols, keys, streams):
    key = np.zeros(len(sid), np.int64)
    if keys is not None:
        for s in streams:
            mine = sid == NAMES.index(s)
            key[mine] = cols[KEYCOL[keys[s]]][mine]
    return key


def rule_outputs(a, b, sid, cols, ts, keys=None, wait="5", c1="gt20", c2="gt45", clock0=None):
    """The rule above: (m, 2) rows (output timestamp, e1 position) in order of (p, creation ordinal, i)."""
    W = WAITS[wait]
    sa, sb = NAMES.index(a), NAMES.index(b)
    price, vol = cols[1], cols[2]
    n = len(sid)
    clock = np.maximum.accumulate(ts if clock0 is None else np.maximum(ts, clock0))
    key = row_keys(sid, cols, keys, {a, b})
    read = np.isin(sid, [sa, sb])
    created = {}
    for i in np.nonzero(read)[0]:
        created.setdefault(int(key[i]), int(i))
    cancels = (sid == sb) & C2[c2][1](price, vol)
    opens = (sid == sa) & C1[c1][1](price, vol)
    out = []
    for k in np.unique(key[read]):
        bj = np.nonzero(cancels & (key == k))[0]
        for i in np.nonzero(opens & (key == k))[0]:
            d = ts[i] + W
            later = bj[np.searchsorted(bj, i, side="right"):]
            if (ts[later] < d).any():
                continue
            q = i + 1 + int(np.searchsorted(clock[i + 1:], d, side="left"))
            if q < n:
                out.append((q, created[int(k)], int(i), int(d)))
    out.sort()
    return np.array([(d, i) for _, _, i, d in out], dtype=np.int64).reshape(-1, 2)


def oracle_outputs(text, sid, cols, ts):
    """(output timestamp, e1 position): the timestamp attribute is the row's position in the feed."""
    a = OracleApp(text)
    a.start()
    a.send_interleaved_ord(sid, ts, np.arange(len(ts), dtype=np.int64), list(cols))
    out = a.outputs()["streams"].get("OutputStream", [])
    a.close()
    return np.array([(r[0], r[1][0]) for r in out], dtype=np.int64).reshape(-1, 2)


def keys_of(kind, a, b, also=None):
    if kind == "flat":
        return None
    k = {a: "symbol", b: "symbol" if kind == "symbol" or a == b else "volume"}
    if also:
        k[also] = "symbol"
    return k


def case(kind, seed=11, heartbeats=0.0):
    sid, cols, ts = stream(seed=seed)
    if kind == "per_stream":
        cols = per_stream_cols(cols)
    if heartbeats:
        sid = sid.copy()
        sid[np.random.default_rng(seed + 100).random(len(sid)) < heartbeats] = -1
    return sid, cols, ts


def floor(kind, wait):
    """Of the oracle's outputs alone: 300 keyed; flat, 500 up to 5 ms (40 ms and 1 sec flat leave few: no floor)."""
    if kind != "flat":
        return 300
    return 500 if WAITS[wait] <= 5 else 0


@pytest.mark.parametrize("heartbeats", [0.0, 0.18])
@pytest.mark.parametrize("wait", list(WAITS))
@pytest.mark.parametrize("kind", ["flat", "symbol", "per_stream"])
def test_rule_equals_the_oracle(kind, wait, heartbeats):
    keys = keys_of(kind, "A", "B")
    c2 = "gt59_5" if wait == "1sec" else "gt45"  # (`price>45` cancels every partial that waits a second)
    for seed in (11, 3, 5):
        sid, cols, ts = case(kind, seed, heartbeats)
        exp = oracle_outputs(absent_text("A", "B", keys, wait, c2=c2), sid, cols, ts)
        assert len(exp) >= floor(kind, wait), (seed, len(exp))
        np.testing.assert_array_equal(exp, rule_outputs("A", "B", sid, cols, ts, keys, wait, c2=c2))


@pytest.mark.parametrize("wait", ["1", "2", "5", "40"])
@pytest.mark.parametrize("kind", ["flat", "symbol"])
def test_the_same_stream_cancels(kind, wait):
    """`A -> not A`: a row is an e1 and a cancelling row of the earlier partials at once; with and without filters
    (without, flat, every partial is cancelled by the next row unless the clock jumps first)."""
    keys = keys_of(kind, "A", "A")
    sid, cols, ts = case(kind, 11, 0.15)
    exp = oracle_outputs(absent_text("A", "A", keys, wait), sid, cols, ts)
    assert len(exp) >= floor(kind, wait)
    np.testing.assert_array_equal(exp, rule_outputs("A", "A", sid, cols, ts, keys, wait))
    exp = oracle_outputs(absent_text("A", "A", keys, wait, "none", "none"), sid, cols, ts)
    np.testing.assert_array_equal(exp, rule_outputs("A", "A", sid, cols, ts, keys, wait, "none", "none"))


@pytest.mark.parametrize("c1,c2", [("none", "none"), ("gt20", "compound"), ("none", "gt70")])
@pytest.mark.parametrize("kind", ["flat", "symbol", "per_stream"])
def test_no_filters_and_a_compound_c2(kind, c1, c2):
    keys = keys_of(kind, "A", "B")
    for wait in ("1", "2") if kind == "flat" else ("2", "5"):  # (flat at 5 ms these leave 326 and 388 outputs)
        sid, cols, ts = case(kind, 3, 0.2)
        exp = oracle_outputs(absent_text("A", "B", keys, wait, c1, c2), sid, cols, ts)
        assert len(exp) >= floor(kind, wait)
        np.testing.assert_array_equal(exp, rule_outputs("A", "B", sid, cols, ts, keys, wait, c1, c2))


@pytest.mark.parametrize("wait", ["2", "40"])
def test_a_partition_that_also_keys_the_unread_stream(wait):
    """Rows of C create no instance of the query: the creation ordinals, and with them the order of the outputs of
    different instances due at one position, are those of the rows of A and B."""
    keys = keys_of("symbol", "A", "B", also="C")
    sid, cols, ts = case("symbol", 5)
    exp = oracle_outputs(absent_text("A", "B", keys, wait), sid, cols, ts)
    assert len(exp) >= 300
    np.testing.assert_array_equal(exp, rule_outputs("A", "B", sid, cols, ts, keys, wait))
    first_c = {int(k): int(np.nonzero((sid == 2) & (cols[0] == k))[0][0]) for k in np.unique(cols[0])}
    first_r = {int(k): int(np.nonzero((sid != 2) & (cols[0] == k))[0][0]) for k in np.unique(cols[0])}
    assert sorted(first_c, key=first_c.get) != sorted(first_r, key=first_r.get)  # counting C rows would reorder them


def test_unread_rows_whose_time_goes_back():
    """Rows of C and heartbeats below the clock are no advance points and break nothing."""
    sid, cols, ts = case("symbol", 11, 0.15)
    ts = ts.copy()
    back = (sid == 2) | (sid == -1)
    ts[back] -= np.random.default_rng(1).integers(0, 30, int(back.sum()))
    assert ((ts < np.maximum.accumulate(ts)) & back).sum() > 500
    for keys in (None, keys_of("symbol", "A", "B")):
        exp = oracle_outputs(absent_text("A", "B", keys, "5"), sid, cols, ts)
        assert len(exp) >= 300
        np.testing.assert_array_equal(exp, rule_outputs("A", "B", sid, cols, ts, keys, "5"))


def test_rule_does_not_hold_when_c2_reads_e1():
    """`not B[price > e1.price]`: a B that cancels one partial postpones the timers of its key's other partials (the
    processor-wide lastArrivalTime), so the oracle emits fewer or in another order than "no B with c2(i, j) before d".
    Such a query is not marked and stays on the NFA kernel."""
    sid, cols, ts = case("symbol", 11)
    price = cols[1]
    for keys in (None, keys_of("symbol", "A", "B")):
        t = absent_text("A", "B", keys, "5").replace("B[price>45]", "B[price>e1.price]")
        exp = oracle_outputs(t, sid, cols, ts)
        key = row_keys(sid, cols, keys, {"A", "B"})
        clock = np.maximum.accumulate(ts)
        created, out = {}, []
        for i in np.nonzero(np.isin(sid, [0, 1]))[0]:
            created.setdefault(int(key[i]), int(i))
        for i in np.nonzero((sid == 0) & (price > 20))[0]:
            d = ts[i] + 5
            j = np.arange(i + 1, len(sid))
            if ((sid[j] == 1) & (key[j] == key[i]) & (price[j] > price[i]) & (ts[j] < d)).any():
                continue
            q = i + 1 + int(np.searchsorted(clock[i + 1:], d, side="left"))
            if q < len(sid):
                out.append((q, created[int(key[i])], int(i), int(d)))
        out.sort()
        got = np.array([(d, i) for _, _, i, d in out], dtype=np.int64).reshape(-1, 2)
        assert len(exp) >= 300 and not np.array_equal(exp, got)


def test_rule_does_not_hold_when_read_rows_lie_below_the_clock():
    """Flat and keyed on decreasing event time: the oracle's outputs are not the rule's. This stays outside the device
    envelope (FAST_NON_MONOTONE: the NFA kernel takes the query over)."""
    sid, cols, ts = case("symbol")
    ts = decreasing_ts(ts)
    differ = 0
    for keys in (None, keys_of("symbol", "A", "B")):
        exp = oracle_outputs(absent_text("A", "B", keys, "5"), sid, cols, ts)
        got = rule_outputs("A", "B", sid, cols, ts, keys, "5")
        assert len(exp) >= 300
        differ += not np.array_equal(exp, got)
    assert differ >= 1


def test_the_compilers_envelope():
    """(fast_absent, fast_pat_ms, fast_every_within, fast_seq_adjacent, fast_seq_k, fast_seq_ms) of the plan the
    compiler makes; every text but the timeout's keeps the marks it has on the parent commit."""
    from test_absent_emu import marks_of
    head = "@app:playback " + SCHEMA
    q = lambda body, sel="e1.timestamp as i": head + f"@info(name='q') from {body} select {sel} insert into Out;"
    part = lambda with_, body: head + f"partition with ({with_}) begin @info(name='q') from {body} " \
                                      "select e1.timestamp as i insert into Out; end;"
    yes, no = (1, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0)
    for kind in ("flat", "symbol", "per_stream"):
        for wait in WAITS:
            for c2 in C2:
                assert marks_of(absent_text("A", "B", keys_of(kind, "A", "B"), wait, "gt20", c2)) == yes
    assert marks_of(absent_text("A", "A", None)) == yes and marks_of(absent_text("A", "A", keys_of("symbol", "A", "A"))) == yes
    assert marks_of(absent_text("C", "A", keys_of("per_stream", "C", "A"), c1="none")) == yes
    assert marks_of(q("every e1=A[price>20] -> not B[price>70] for 1 sec", "e1.price as p, e1.volume as v, 7 as c")) == yes
    assert marks_of(part("symbol of A, symbol of B, symbol of C", "every e1=A -> not B for 1 sec")) == yes
    # c2 reads e1; a having; a within on an element or on the root; no playback clock: an error, as before
    assert marks_of(q("every e1=A[price>20] -> not B[price>e1.price] for 1 sec")) == no
    assert marks_of(q("every e1=A -> not B[price>70] for 1 sec", "e1.timestamp as i having i > 3")) == no
    assert marks_of(q("every e1=A within 5 milliseconds -> not B for 1 sec")) == no
    assert marks_of(q("every (e1=A -> not B for 1 sec) within 2 sec")) == no
    with pytest.raises(AssertionError, match="playback"):
        marks_of(absent_text("A", "B", None, playback=False))
    # the absent element elsewhere, a logical absent, three elements, no leading every, a sequence
    assert marks_of(q("every not A for 1 sec -> e1=B")) == no
    assert marks_of(q("every e1=A -> (not B and e2=C)", "e1.timestamp as i")) == no
    assert marks_of(q("every e1=A -> not B for 1 sec -> e3=C")) == no
    assert marks_of(q("e1=A -> not B for 1 sec")) == no
    assert marks_of(q("every e1=A, not B for 1 sec")) == no
    # partition keys: one INT / LONG attribute per read stream, else no mark
    assert marks_of(part("symbol of A, volume of B", "every e1=A -> not B for 1 sec")) == yes
    assert marks_of(part("symbol + 1 of A, symbol of B", "every e1=A -> not B for 1 sec")) == no
    named = "@app:playback " + "".join(f"define stream {s} (name string, price double, volume long, timestamp long); "
                                      for s in "AB")
    assert marks_of(named + "partition with (name of A, name of B) begin @info(name='q') from every e1=A -> not B "
                    "for 1 sec select e1.timestamp as i insert into Out; end;") == no
    # streams of different schemas
    other = "@app:playback define stream A (symbol int, price double); define stream B (symbol int, price float); "
    assert marks_of(other + "@info(name='q') from every e1=A -> not B for 1 sec select e1.price as p insert into Out;") == no
    # the forms of paths 6-10 keep their marks
    assert marks_of(q("every e1=A[price>20] -> e2=B[price>e1.price] within 1 sec")) == (0, 1, 0, 0, 0, 0)
    assert marks_of(q("every e1=A[price>20] -> e2=A[price>e1.price] within 1 sec")) == (0, 0, 1, 0, 0, 0)
    assert marks_of(q("every e1=A[price>20], e2=A[price>e1.price]")) == (0, 0, 0, 1, 0, 0)
    assert marks_of(q("every e1=A, e2=A, e3=A")) == (0, 0, 0, 0, 3, 0)
    assert marks_of(q("every e1=A, e2=B")) == (0, 0, 0, 0, 0, 2)
