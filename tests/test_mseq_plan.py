"""The plan of `every e1=S1[c1], e2=S2[c2], ..., ek=Sk[ck]` (2 <= k <= 8) over several streams of one schema once the
compiler marks it for the closed form of interleaved device batches (compiler.cpp fast_seq_ms, k hidden ordinal refs for
the NFA hand-over), and the rule the device kernels (kernels/mseq_dev.h) implement, tied to the oracle on the CPU:

    R = the streams the query reads. Take the events of a partition instance whose stream is in R, in arrival order (an
    event's instance key is the key attribute of its own stream; unpartitioned: all such events). Events of other
    streams and heartbeats do not exist for the query. For every such event j with k - 1 predecessors
    i1 < ... < i(k-1) in that list, emit (i1, ..., i(k-1), j) iff the event at position m is on stream Sm for every
    m, c1 .. ck hold and, for every element m >= 2 written with `within Tm`, ts[e_m] - ts[e_(m-1)] <= Tm; outputs in
    order of j, at most one per j.

The numpy statement of that rule equals the oracle's outputs tuple for tuple for `A, B`, `A, B, A`, `A, A, B`, `A, B, C`,
a 6-state and an 8-state chain, flat and partitioned, with one key attribute and with a key attribute per stream, with
`within` on the last, on a middle and on two elements, with a stream in the feed that the query does not read (running
the rule over all three streams' events gives other outputs), and on a stream whose event time decreases when no element
has a `within`. With one the partitioned oracle differs from the rule, so the device path hands that to the NFA kernel.
The query tree sm_compile_dump reports is unchanged, and the plan still runs on the NFA built for the host
(tests/native) with the oracle's values and visible refs and the tuple in its hidden refs. Test infrastructure: no GPU;
`-m "not gpu"`."""
import os
import subprocess

import numpy as np
import pytest

import siddhi_amd
from oracle_lib import OracleApp

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["A", "B", "C"]
TYPES = ["INT", "DOUBLE", "LONG", "LONG"]
SCHEMA = "".join(f"define stream {s} (symbol int, price double, volume long, timestamp long); " for s in NAMES)
KEYCOL = {"symbol": 0, "volume": 2}


def mseq_text(pattern, keys=None, withins=None, select=None, c1="[price>20]",
              cm="price > {p}.price - 25.0 and volume != e1.volume"):
    """pattern: stream names in element order; keys: {stream: key attribute} (None: unpartitioned); withins: {m: T} on
    element m (1-based, m >= 2); cm: the condition of elements 2 .. k, {p} = the previous element."""
    withins = withins or {}
    k = len(pattern)
    els = [f"every e1={pattern[0]}{c1}"]
    for m in range(2, k + 1):
        w = f" within {withins[m]} milliseconds" if m in withins else ""
        els.append(f"e{m}={pattern[m - 1]}[{cm.format(p=f'e{m - 1}')}]{w}")
    sel = select or ", ".join(f"e{m}.timestamp as i{m}" for m in range(1, k + 1))
    q = f"@info(name='q') from {', '.join(els)} select {sel} insert into OutputStream;"
    if keys is None:
        return SCHEMA + q
    part = ", ".join(f"{a} of {s}" for s, a in keys.items())
    return SCHEMA + f"partition with ({part}) begin {q} end;"


def rule_tuples(pattern, sid, cols, ts, keys=None, withins=None, read=None):
    """The rule above. cols = [symbol, price, volume, timestamp]; read: stream indices taken as the query's (default:
    the pattern's). (m, k) rows of batch positions, in order of j."""
    withins = withins or {}
    k = len(pattern)
    want = [NAMES.index(s) for s in pattern]
    read = sorted(set(want)) if read is None else read
    rows = np.nonzero(np.isin(sid, read))[0]
    price, vol = cols[1], cols[2]
    if keys is None:
        key = np.zeros(len(rows), np.int64)
    else:
        key = np.zeros(len(rows), np.int64)
        for s, a in keys.items():
            mine = sid[rows] == NAMES.index(s)
            key[mine] = cols[KEYCOL[a]][rows][mine]
    order = rows[np.argsort(key, kind="stable")]
    ks = np.sort(key, kind="stable")
    n = len(rows)
    u = np.arange(k - 1, n)
    u = u[ks[u] == ks[u - (k - 1)]] if n >= k else u[:0]
    M = [order[u - (k - 1) + m] for m in range(k)]
    ok = price[M[0]] > 20
    for m in range(k):
        ok &= sid[M[m]] == want[m]
    for m in range(1, k):
        ok &= (price[M[m]] > price[M[m - 1]] - 25.0) & (vol[M[m]] != vol[M[0]])
        if m + 1 in withins:
            ok &= ts[M[m]] - ts[M[m - 1]] <= withins[m + 1]
    t = np.stack([x[ok] for x in M], axis=1).reshape(-1, k)
    return t[np.argsort(t[:, k - 1], kind="stable")]


def stream(n=4000, K=5, seed=11, pattern=None, noise=0.15):
    """Random events over the three streams and K keys (symbol and volume % K both serve as key attributes). With a
    pattern: an instance's events mostly follow it in turn, so that long chains complete."""
    rng = np.random.default_rng(seed)
    sym = rng.integers(0, K, n).astype(np.int32)
    price = np.round(rng.random(n) * 60.0, 1)
    vol = rng.integers(0, 2000, n).astype(np.int64)
    ts = np.cumsum(rng.integers(0, 3, n)).astype(np.int64)
    sid = rng.integers(0, 3, n).astype(np.int32)
    if pattern is not None:
        want = np.array([NAMES.index(s) for s in pattern], np.int32)
        seen = np.zeros(K, np.int64)
        for i in range(n):
            if rng.random() >= noise:
                sid[i] = want[seen[sym[i]] % len(want)]
            seen[sym[i]] += 1
        price = 30.0 + np.round(rng.random(n) * 20.0, 1)
    return sid, [sym, price, vol, np.arange(n, dtype=np.int64)], ts


def oracle_rows(text, sid, cols, ts):
    a = OracleApp(text)
    a.start()
    a.send_interleaved(sid, ts, cols)
    out = a.outputs()["streams"].get("OutputStream", [])
    a.close()
    return out


def oracle_tuples(text, sid, cols, ts, k):
    return np.array([r[2] for r in oracle_rows(text, sid, cols, ts)], dtype=np.int64).reshape(-1, k)


BY_SYMBOL = {"A": "symbol", "B": "symbol", "C": "symbol"}
PER_STREAM = {"A": "symbol", "B": "volume", "C": "symbol"}  # B's instances are keyed by its volume


def keys_of(kind, pattern):
    if kind == "flat":
        return None
    src = BY_SYMBOL if kind == "symbol" else PER_STREAM
    return {s: src[s] for s in sorted(set(pattern))}


def per_stream_cols(cols, K=5):
    cols = list(cols)
    cols[2] = cols[2] % K  # volume as a key attribute: the same K instances
    return cols


SHAPES = {
    "AB": (["A", "B"], {}),
    "AB_within2": (["A", "B"], {2: 2}),
    "ABA": (["A", "B", "A"], {}),
    "AAB_within3_on_e3": (["A", "A", "B"], {3: 3}),
    "ABC": (["A", "B", "C"], {}),
}


@pytest.mark.parametrize("kind", ["flat", "symbol", "per_stream"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_rule_equals_the_oracle(shape, kind):
    pattern, withins = SHAPES[shape]
    sid, cols, ts = stream()
    if kind == "per_stream":
        cols = per_stream_cols(cols)
    keys = keys_of(kind, pattern)
    exp = oracle_tuples(mseq_text(pattern, keys, withins), sid, cols, ts, len(pattern))
    got = rule_tuples(pattern, sid, cols, ts, keys, withins)
    assert len(exp) >= 10
    np.testing.assert_array_equal(exp, got)
    if len(set(pattern)) == 2:  # the third stream is in the feed and not read: it neither breaks nor extends a run
        over_all = rule_tuples(pattern, sid, cols, ts, keys_of(kind, NAMES), withins, read=[0, 1, 2])
        assert not np.array_equal(over_all, got)


@pytest.mark.parametrize("kind", ["flat", "symbol", "per_stream"])
def test_six_states_on_30000_events(kind):
    pattern, withins = ["A", "B", "B", "A", "C", "A"], {3: 4}
    sid, cols, ts = stream(30000, seed=5)
    if kind == "per_stream":
        cols = per_stream_cols(cols)
    keys = keys_of(kind, pattern)
    exp = oracle_tuples(mseq_text(pattern, keys, withins), sid, cols, ts, 6)
    assert len(exp) > 0
    np.testing.assert_array_equal(exp, rule_tuples(pattern, sid, cols, ts, keys, withins))


WITHINS = {"none": lambda k: {}, "last0": lambda k: {k: 0}, "last5": lambda k: {k: 5}, "middle": lambda k: {2: 2},
           "two": lambda k: {2: 3, k: 2}}
CHAINS = {2: ["A", "B"], 3: ["A", "B", "A"], 8: ["A", "B", "A", "A", "B", "C", "A", "B"]}


# (a two-state chain has one element that takes a within: no "middle", no "two")
K_WITHINS = [(k, w) for k in (2, 3, 8) for w in WITHINS if k > 2 or w not in ("middle", "two")]


@pytest.mark.parametrize("partitioned", [True, False])
@pytest.mark.parametrize("k,wname", K_WITHINS)
def test_withins_k2_to_k8(k, wname, partitioned):
    """k = 2 and k = 8 included; the streams mostly follow the chain, so that 8-state runs complete."""
    pattern = CHAINS[k]
    withins = WITHINS[wname](k)
    sid, cols, ts = stream(4000, seed=7 + k, pattern=pattern)
    keys = keys_of("symbol" if partitioned else "flat", pattern)
    exp = oracle_tuples(mseq_text(pattern, keys, withins), sid, cols, ts, k)
    assert len(exp) > 0
    np.testing.assert_array_equal(exp, rule_tuples(pattern, sid, cols, ts, keys, withins))


BY_SYMBOL_AB = {"A": "symbol", "B": "symbol"}


def decreasing_ts(ts):
    ts = ts.copy()
    ts[1000:1400] = ts[1000:1400][::-1]  # event time runs backwards for 400 events
    ts[2000:] -= 7                       # and steps back once more
    assert (np.diff(ts) < 0).sum() > 100
    return ts


@pytest.mark.parametrize("partitioned", [True, False])
@pytest.mark.parametrize("shape", ["AB", "ABA"])
def test_rule_equals_the_oracle_when_event_time_decreases_without_within(shape, partitioned):
    pattern, _ = SHAPES[shape]
    sid, cols, ts = stream()
    ts = decreasing_ts(ts)
    keys = keys_of("symbol" if partitioned else "flat", pattern)
    exp = oracle_tuples(mseq_text(pattern, keys), sid, cols, ts, len(pattern))
    assert len(exp) > 0
    np.testing.assert_array_equal(exp, rule_tuples(pattern, sid, cols, ts, keys))


def test_rule_does_not_hold_with_a_within_when_event_time_decreases():
    """`A, B within 2 ms`, partitioned, on decreasing event time: the oracle's outputs are not the rule's. This stays
    outside the device envelope (FAST_NON_MONOTONE: the NFA kernel takes the query over)."""
    pattern, withins = SHAPES["AB_within2"]
    sid, cols, ts = stream()
    ts = decreasing_ts(ts)
    exp = oracle_tuples(mseq_text(pattern, BY_SYMBOL_AB, withins), sid, cols, ts, 2)
    got = rule_tuples(pattern, sid, cols, ts, BY_SYMBOL_AB, withins)
    assert len(exp) > 0 and len(exp) != len(got)


def test_compile_dump_unchanged():
    """The hidden refs do not show: the query tree is what the parser made of the text."""
    d = siddhi_amd.compile_dump(mseq_text(["A", "B", "A"], {"A": "symbol", "B": "volume"}, {3: 1000},
                                          select="e1.timestamp as i, e3.timestamp as j", cm="price > {p}.price"))
    assert d["queries"] == [] and len(d["partitions"]) == 1
    assert d["partitions"][0]["with"] == [{"key": {"var": "symbol"}, "stream": "A"},
                                          {"key": {"var": "volume"}, "stream": "B"}]
    q = d["partitions"][0]["queries"][0]
    assert q["input"] == "sequence" and q["select"] == [
        {"as": "i", "expr": {"ref": "e1", "var": "timestamp"}}, {"as": "j", "expr": {"ref": "e3", "var": "timestamp"}}]
    nxt = q["state"]["next"]
    assert nxt[0] == {"every": {"filters": [{"cmp": ">", "l": {"var": "price"}, "r": {"const": 20, "type": "INT"}}],
                                "ref": "e1", "stream": "A"}}
    inner = nxt[1]["next"]
    assert [e["ref"] for e in inner] == ["e2", "e3"] and "within" not in inner[0] and inner[1]["within"] == 1000
    assert [e["stream"] for e in inner] == ["B", "A"]
    assert inner[0]["filters"] == [{"cmp": ">", "l": {"var": "price"}, "r": {"ref": "e1", "var": "price"}}]


@pytest.fixture(scope="module")
def harness():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "native")])
    from host_harness_lib import HostHarnessApp
    return HostHarnessApp


def feed(factory, text, sid, cols, ts, flush_every=0):
    a = factory(text)
    a.start()
    for i in range(len(ts)):
        a.send(NAMES[sid[i]], int(ts[i]), [int(cols[0][i]), float(cols[1][i]), int(cols[2][i]), int(cols[3][i])], TYPES)
        if flush_every and (i + 1) % flush_every == 0:
            a.flush()
    a.flush()
    out = a.outputs()["streams"].get("OutputStream", [])
    a.close()
    return out


@pytest.mark.parametrize("kind", ["flat", "per_stream"])
@pytest.mark.parametrize("shape", ["AB_within2", "ABA", "AAB_within3_on_e3"])
def test_plan_runs_on_the_host_nfa_with_the_tuple_in_its_hidden_refs(harness, shape, kind):
    """The select reads e1 and ek only: two visible refs, then the k hidden ones (slot m, index 0) = the rule's tuple,
    also when the lanes' state is carried across batches."""
    pattern, withins = SHAPES[shape]
    k = len(pattern)
    sid, cols, ts = stream(3000, seed=21)
    if kind == "per_stream":
        cols = per_stream_cols(cols)
    keys = keys_of(kind, pattern)
    t = mseq_text(pattern, keys, withins, select=f"e1.timestamp as i, e{k}.timestamp as j")
    exp = feed(OracleApp, t, sid, cols, ts)
    tuples = rule_tuples(pattern, sid, cols, ts, keys, withins)
    assert len(exp) == len(tuples) > 0
    for flush_every in (0, 997):
        got = feed(harness, t, sid, cols, ts, flush_every=flush_every)
        assert [[r[0], r[1], r[2][:2]] for r in got] == exp
        np.testing.assert_array_equal(np.array([r[2][2:] for r in got], dtype=np.int64), tuples)
