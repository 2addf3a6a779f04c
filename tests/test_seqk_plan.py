"""The plan of `every e1=S[c1], e2=S[c2], ..., ek=S[ck]` (3 <= k <= 8, one stream) once the compiler marks it for the
adjacent-run closed form (compiler.cpp fast_seq_k, k hidden ordinal refs for the NFA hand-over of device batches),
and the rule the device kernels (kernels/seq_dev.h) implement, tied to the oracle on the CPU:

    for every event j of a partition instance with k - 1 predecessors i1 < ... < i(k-1) (the previous k - 1 events of
    the instance), emit (i1, ..., i(k-1), j) iff c1(i1), c2(i1, i2), ..., ck(i1 .. j) hold and, for every element
    m >= 2 written with `within Tm`, ts[e_m] - ts[e_(m-1)] <= Tm; outputs in order of j.

The numpy statement of that rule equals the oracle's outputs tuple for tuple for k = 3, 4, 5 and 8, keyed and unkeyed,
with `within` on the last, on a middle and on two elements, and on a stream whose event time decreases when no
element has a `within` (with one the partitioned oracle differs from the rule, so the device path hands decreasing
time with a `within` to the NFA kernel, as the pair path does). The query tree
sm_compile_dump reports is unchanged, and the plan still runs on the NFA built for the host (tests/native), with the
oracle's values and visible refs and the tuple in its hidden refs. Test infrastructure: no GPU; `-m "not gpu"`."""
import os
import subprocess

import numpy as np
import pytest

import siddhi_amd
from oracle_lib import OracleApp
from test_seq_plan import PART, SCHEMA, TYPES, feed, stream

HERE = os.path.dirname(os.path.abspath(__file__))


def seqk_text(k, partitioned, withins=None, select=None):
    """c1 = price > 20; cm = price > e(m-1).price - 25.0 and volume != e1.volume (reads e1 and e(m-1)); withins: {m: T}
    on element m (1-based, m >= 2)."""
    withins = withins or {}
    els = ["every e1=StockStream[price>20]"]
    for m in range(2, k + 1):
        w = f" within {withins[m]} milliseconds" if m in withins else ""
        els.append(f"e{m}=StockStream[price > e{m - 1}.price - 25.0 and volume != e1.volume]{w}")
    sel = select or ", ".join(f"e{m}.timestamp as i{m}" for m in range(1, k + 1))
    q = f"@info(name='q') from {', '.join(els)} select {sel} insert into OutputStream;"
    return SCHEMA + (PART.format(q=q) if partitioned else q)


def rule_tuples(k, sym, price, vol, ts, partitioned, withins=None):
    """The adjacent-run rule: each event with the previous k - 1 events of its instance. (m, k) rows, in order of j."""
    withins = withins or {}
    n = len(ts)
    key = sym if partitioned else np.zeros(n, np.int64)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    u = np.arange(k - 1, n)
    u = u[ks[u] == ks[u - (k - 1)]] if n >= k else u[:0]  # the run holds k - 1 predecessors
    M = [order[u - (k - 1) + m] for m in range(k)]       # M[m]: rows of element m + 1
    ok = price[M[0]] > 20
    for m in range(1, k):
        ok &= (price[M[m]] > price[M[m - 1]] - 25.0) & (vol[M[m]] != vol[M[0]])
        if m + 1 in withins:
            ok &= ts[M[m]] - ts[M[m - 1]] <= withins[m + 1]
    t = np.stack([x[ok] for x in M], axis=1).reshape(-1, k)
    return t[np.argsort(t[:, k - 1], kind="stable")]


def rows_of(sym, price, vol, ts):
    return [(int(ts[i]), [int(sym[i]), float(price[i]), int(vol[i]), i]) for i in range(len(ts))]


WITHINS = {"none": lambda k: {}, "last0": lambda k: {k: 0}, "last5": lambda k: {k: 5}, "middle": lambda k: {2: 2},
           "two": lambda k: {2: 3, k: 2}}


_oracle_cache = {}


def oracle_tuples(k, partitioned, wname, decreasing=False):
    key = (k, partitioned, wname, decreasing)
    if key not in _oracle_cache:
        sym, price, vol, ts = stream()
        if decreasing:
            ts = decreasing_ts(ts)
        exp = feed(OracleApp, seqk_text(k, partitioned, WITHINS[wname](k)), rows_of(sym, price, vol, ts))
        _oracle_cache[key] = exp
    return _oracle_cache[key]


def decreasing_ts(ts):
    ts = ts.copy()
    ts[1000:1400] = ts[1000:1400][::-1]  # event time runs backwards for 400 events
    ts[2000:] -= 7                       # and steps back once more
    assert (np.diff(ts) < 0).sum() > 100
    return ts


@pytest.mark.parametrize("wname", list(WITHINS))
@pytest.mark.parametrize("partitioned", [True, False])
@pytest.mark.parametrize("k", [3, 4, 5, 8])
def test_rule_equals_the_oracle(k, partitioned, wname):
    sym, price, vol, ts = stream()
    exp = oracle_tuples(k, partitioned, wname)
    got = rule_tuples(k, sym, price, vol, ts, partitioned, WITHINS[wname](k))
    assert len(exp) > 0
    np.testing.assert_array_equal(np.array([r[1] for r in exp], dtype=np.int64).reshape(-1, k), got)
    # the oracle's refs are the select's k ordinals: the same tuple
    np.testing.assert_array_equal(np.array([r[2] for r in exp], dtype=np.int64).reshape(-1, k), got)


@pytest.mark.parametrize("partitioned", [True, False])
@pytest.mark.parametrize("k", [3, 4])
def test_rule_equals_the_oracle_when_event_time_decreases_without_within(k, partitioned):
    """Without a `within` the rule holds whatever the time order: no condition reads event time."""
    sym, price, vol, ts = stream()
    ts = decreasing_ts(ts)
    exp = oracle_tuples(k, partitioned, "none", decreasing=True)
    got = rule_tuples(k, sym, price, vol, ts, partitioned)
    assert len(exp) > 0
    np.testing.assert_array_equal(np.array([r[1] for r in exp], dtype=np.int64).reshape(-1, k), got)


def test_rule_does_not_hold_with_a_within_when_event_time_decreases():
    """With a `within` and decreasing event time the partitioned oracle's outputs are not the rule's (566 against 634
    here): this stays outside the device envelope (FAST_NON_MONOTONE: the NFA kernel takes the query over, as for the
    pair path), keyed and unkeyed alike."""
    sym, price, vol, ts = stream()
    ts = decreasing_ts(ts)
    exp = oracle_tuples(3, True, "last5", decreasing=True)
    got = rule_tuples(3, sym, price, vol, ts, True, {3: 5})
    assert len(exp) > 0 and len(exp) != len(got)


def test_compile_dump_unchanged():
    """The hidden refs do not show: the query tree is what the parser made of the text."""
    d = siddhi_amd.compile_dump(seqk_text(3, True, {3: 1000}, select="e1.timestamp as i, e3.timestamp as j"))
    assert d["queries"] == [] and len(d["partitions"]) == 1
    q = d["partitions"][0]["queries"][0]
    assert q["input"] == "sequence" and q["select"] == [
        {"as": "i", "expr": {"ref": "e1", "var": "timestamp"}}, {"as": "j", "expr": {"ref": "e3", "var": "timestamp"}}]
    nxt = q["state"]["next"]
    assert nxt[0] == {"every": {"filters": [{"cmp": ">", "l": {"var": "price"}, "r": {"const": 20, "type": "INT"}}],
                                "ref": "e1", "stream": "StockStream"}}
    inner = nxt[1]["next"]
    assert [e["ref"] for e in inner] == ["e2", "e3"] and "within" not in inner[0] and inner[1]["within"] == 1000
    assert inner[0]["stream"] == inner[1]["stream"] == "StockStream"


@pytest.fixture(scope="module")
def harness():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "native")])
    from host_harness_lib import HostHarnessApp
    return HostHarnessApp


@pytest.mark.parametrize("wname", ["none", "two"])
@pytest.mark.parametrize("partitioned", [True, False])
@pytest.mark.parametrize("k", [3, 5])
def test_plan_runs_on_the_host_nfa_with_the_tuple_in_its_hidden_refs(harness, k, partitioned, wname):
    """The select reads e1 and ek only: two visible refs, then the k hidden ones (slot m, index 0) = the rule's tuple,
    also when the lanes' state is carried across batches."""
    sym, price, vol, ts = stream()
    w = WITHINS[wname](k)
    t = seqk_text(k, partitioned, w, select=f"e1.timestamp as i, e{k}.timestamp as j")
    rows = rows_of(sym, price, vol, ts)
    exp = feed(OracleApp, t, rows)
    tuples = rule_tuples(k, sym, price, vol, ts, partitioned, w)
    assert len(exp) == len(tuples) > 0
    for flush_every in (0, 997):
        got = feed(harness, t, rows, flush_every=flush_every)
        assert [[r[0], r[1], r[2][:2]] for r in got] == exp
        np.testing.assert_array_equal(np.array([r[2][2:] for r in got], dtype=np.int64), tuples)
