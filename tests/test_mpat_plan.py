"""The plan of `every e1=A[c1] -> e2=B[c2] within T` over two streams of one schema once the compiler marks it for the
closed form of interleaved device batches (compiler.cpp fast_pat_ms, the hidden (e1, e2) ordinal refs for the NFA
hand-over), and the rule the device kernels (kernels/mpat_dev.h) implement, tied to the oracle on the CPU:

    R = {A, B}. Take the events of a partition instance whose stream is in R, in arrival order (an event's instance key
    is the key attribute of its own stream; unpartitioned: all such events). Events of other streams do not exist for
    the query. For every event i on stream A with c1(i), let j*(i) = min {j > i : stream[j] = B, key[j] = key[i],
    c2(i, j)}. The query emits (i, j*(i)) iff j* exists and ts[j*] - ts[i] <= T; outputs in order of (j*, i).

The numpy statement of that rule equals the oracle's outputs pair for pair, flat, partitioned by one attribute and by an
attribute per stream, for four windows and three forms of c2 (one compound and not monotone, one that does not read e1,
so that one e2 completes many partials), for the directions `B -> A` and `C -> A`, with a third stream in the feed that
the query does not read. With event time that decreases the oracle differs from the rule, so the device path hands that
to the NFA kernel. Also the compiler's envelope for the mark, and the plan on the NFA built for the host
(tests/native) with the oracle's values and the pair in its hidden refs. Test infrastructure: no GPU; `-m "not gpu"`."""
import os
import subprocess

import numpy as np
import pytest

from test_mseq_plan import NAMES, SCHEMA, KEYCOL, decreasing_ts, feed, oracle_tuples, per_stream_cols, stream
from oracle_lib import OracleApp

HERE = os.path.dirname(os.path.abspath(__file__))

C2 = {
    "gt": ("price > e1.price", lambda p1, v1, p2, v2: p2 > p1),
    "compound": ("price > e1.price - 25.0 and volume != e1.volume", lambda p1, v1, p2, v2: (p2 > p1 - 25.0) & (v2 != v1)),
    "const": ("price > 45", lambda p1, v1, p2, v2: p2 > 45),
}


def mpat_text(a, b, keys=None, within=5, c2="gt", select="e1.timestamp as i, e2.timestamp as j", c1="[price>20]"):
    """keys: {stream: key attribute} (None: unpartitioned); within: T in ms (None: no within)."""
    w = "" if within is None else f" within {within} milliseconds"
    q = (f"@info(name='q') from every e1={a}{c1} -> e2={b}[{C2[c2][0]}]{w} select {select} "
         "insert into OutputStream;")
    if keys is None:
        return SCHEMA + q
    return SCHEMA + "partition with (" + ", ".join(f"{x} of {s}" for s, x in keys.items()) + f") begin {q} end;"


def rule_pairs(a, b, sid, cols, ts, keys=None, within=5, c2="gt"):
    """The rule above; (m, 2) batch positions in order of (j*, i)."""
    sa, sb = NAMES.index(a), NAMES.index(b)
    rows = np.nonzero(np.isin(sid, [sa, sb]))[0]
    price, vol = cols[1], cols[2]
    key = np.zeros(len(rows), np.int64)
    if keys is not None:
        for s, x in keys.items():
            mine = sid[rows] == NAMES.index(s)
            key[mine] = cols[KEYCOL[x]][rows][mine]
    f = C2[c2][1]
    out = []
    for k in np.unique(key):
        r = rows[key == k]
        isb = sid[r] == sb
        for u in np.nonzero((sid[r] == sa) & (price[r] > 20))[0]:
            i = r[u]
            later = r[u + 1:]
            ok = isb[u + 1:] & f(price[i], vol[i], price[later], vol[later])
            if ok.any():
                j = later[np.argmax(ok)]
                if within is None or ts[j] - ts[i] <= within:
                    out.append((j, i))
    out.sort()
    return np.array([(i, j) for j, i in out], dtype=np.int64).reshape(-1, 2)


def keys_of(kind, a, b):
    if kind == "flat":
        return None
    return {a: "symbol", b: "symbol" if kind == "symbol" else "volume"}


def case(kind, seed=11):
    sid, cols, ts = stream(seed=seed)
    if kind == "per_stream":
        cols = per_stream_cols(cols)
    return sid, cols, ts


@pytest.mark.parametrize("c2", list(C2))
@pytest.mark.parametrize("within", [0, 2, 5, 40])
@pytest.mark.parametrize("kind", ["flat", "symbol", "per_stream"])
def test_rule_equals_the_oracle(kind, within, c2):
    """On the streams of seeds 11, 3 and 5. The floor of expected outputs (30; 3 for `within 0`) is asserted on seed 3,
    which reaches it in all 36 cases; seed 11 reaches it for `price > e1.price` (below) and the compound c2, and gives
    1 and 23 outputs for `price > 45` keyed by symbol within 0 and 2 ms."""
    keys = keys_of(kind, "A", "B")
    for seed in (3, 11, 5):
        sid, cols, ts = case(kind, seed)
        exp = oracle_tuples(mpat_text("A", "B", keys, within, c2), sid, cols, ts, 2)
        got = rule_pairs("A", "B", sid, cols, ts, keys, within, c2)
        if seed == 3:
            assert len(exp) >= (3 if within == 0 else 30)
        np.testing.assert_array_equal(exp, got)
        if c2 == "const" and within == 40:  # one e2 completes many partials, oldest e1 first
            _, cnt = np.unique(exp[:, 1], return_counts=True)
            assert cnt.max() >= 5


def test_output_counts_on_seed_11():
    """`price > e1.price` keyed by symbol: the counts the device tests' floors start from."""
    sid, cols, ts = case("symbol", 11)
    keys = keys_of("symbol", "A", "B")
    n = {w: len(oracle_tuples(mpat_text("A", "B", keys, w), sid, cols, ts, 2)) for w in (None, 5, 2, 0)}
    assert n[None] >= 376 and n[5] >= 62 and n[2] >= 32 and 3 <= n[0] <= 85


@pytest.mark.parametrize("kind", ["flat", "symbol"])
@pytest.mark.parametrize("a,b", [("B", "A"), ("C", "A")])
def test_other_directions(a, b, kind):
    sid, cols, ts = case(kind)
    keys = keys_of(kind, a, b)
    exp = oracle_tuples(mpat_text(a, b, keys, 5), sid, cols, ts, 2)
    assert len(exp) >= 30
    np.testing.assert_array_equal(exp, rule_pairs(a, b, sid, cols, ts, keys, 5))


@pytest.mark.parametrize("seed", [3, 5])
def test_other_seeds_and_no_within(seed):
    sid, cols, ts = case("symbol", seed)
    keys = keys_of("symbol", "A", "B")
    for within in (None, 5):
        exp = oracle_tuples(mpat_text("A", "B", keys, within), sid, cols, ts, 2)
        assert len(exp) >= 30
        np.testing.assert_array_equal(exp, rule_pairs("A", "B", sid, cols, ts, keys, within))


def test_rule_does_not_hold_with_a_within_when_event_time_decreases():
    """Flat and keyed, `within 5 ms` on decreasing event time: the oracle's outputs are not the rule's. This stays outside
    the device envelope (FAST_NON_MONOTONE: the NFA kernel takes the query over). Without a `within` the rule holds."""
    sid, cols, ts = case("symbol")
    ts = decreasing_ts(ts)
    for keys in (None, keys_of("symbol", "A", "B")):
        exp = oracle_tuples(mpat_text("A", "B", keys, 5), sid, cols, ts, 2)
        got = rule_pairs("A", "B", sid, cols, ts, keys, 5)
        assert len(exp) >= 30 and not np.array_equal(exp, got)
        exp = oracle_tuples(mpat_text("A", "B", keys, None), sid, cols, ts, 2)
        np.testing.assert_array_equal(exp, rule_pairs("A", "B", sid, cols, ts, keys, None))


def test_the_compilers_envelope():
    """(fast_pat_ms, fast_every_within, fast_seq_adjacent, fast_seq_k, fast_seq_ms) of the plan the compiler makes."""
    from test_mpat_emu import marks_of
    q = lambda body, sel="e1.timestamp as i": SCHEMA + f"@info(name='q') from {body} select {sel} insert into Out;"
    part = lambda with_, body: SCHEMA + f"partition with ({with_}) begin @info(name='q') from {body} " \
                                        "select e1.timestamp as i insert into Out; end;"
    yes = (1, 0, 0, 0, 0)
    for kind in ("flat", "symbol", "per_stream"):
        for c2 in C2:
            assert marks_of(mpat_text("A", "B", keys_of(kind, "A", "B"), 5, c2)) == yes
    assert marks_of(mpat_text("B", "A", None, 0)) == yes and marks_of(mpat_text("C", "A", keys_of("symbol", "C", "A"))) == yes
    assert marks_of(q("every e1=A[price>20] -> e2=B[price>e1.price] within 1 sec", "e1.price as p, e2.price as r")) == yes
    assert marks_of(q("every e1=A -> e2=B within 1 sec")) == yes
    # no within; a within on e1, on the root
    assert marks_of(mpat_text("A", "B", None, None)) == (0, 0, 0, 0, 0)
    assert marks_of(mpat_text("A", "B", keys_of("symbol", "A", "B"), None)) == (0, 0, 0, 0, 0)
    assert marks_of(q("every e1=A[price>20] within 5 milliseconds -> e2=B[price>e1.price] within 1 sec")) == (0, 0, 0, 0, 0)
    assert marks_of(q("every (e1=A[price>20] -> e2=B[price>e1.price]) within 1 sec")) == (0, 0, 0, 0, 0)
    # the same stream stays fast_every_within, the sequence forms stay what they are
    assert marks_of(q("every e1=A[price>20] -> e2=A[price>e1.price] within 1 sec")) == (0, 1, 0, 0, 0)
    assert marks_of(q("every e1=A[price>20], e2=B[price>e1.price] within 1 sec")) == (0, 0, 0, 0, 2)
    assert marks_of(q("every e1=A[price>20], e2=A[price>e1.price] within 1 sec")) == (0, 0, 1, 0, 0)
    # three states, a count, a logical element, a having, no leading every
    assert marks_of(q("every e1=A -> e2=B -> e3=A within 1 sec")) == (0, 0, 0, 0, 0)
    assert marks_of(q("every e1=A -> e2=B<2:3> within 1 sec")) == (0, 0, 0, 0, 0)
    assert marks_of(q("every e1=A -> (e2=B and e3=C) within 1 sec")) == (0, 0, 0, 0, 0)
    assert marks_of(q("every e1=A -> e2=B within 1 sec", "e1.timestamp as i having i > 3")) == (0, 0, 0, 0, 0)
    assert marks_of(q("e1=A[price>20] -> e2=B[price>e1.price] within 1 sec")) == (0, 0, 0, 0, 0)
    # partition keys: one INT / LONG attribute per read stream, else no mark
    assert marks_of(part("symbol of A, volume of B", "every e1=A -> e2=B within 1 sec")) == yes
    assert marks_of(part("symbol + 1 of A, symbol of B", "every e1=A -> e2=B within 1 sec")) == (0, 0, 0, 0, 0)
    named = "".join(f"define stream {s} (name string, price double, volume long, timestamp long); " for s in "AB")
    assert marks_of(named + "partition with (name of A, name of B) begin @info(name='q') from every e1=A -> e2=B "
                    "within 1 sec select e1.timestamp as i insert into Out; end;") == (0, 0, 0, 0, 0)
    # streams of different schemas
    other = "define stream A (symbol int, price double); define stream B (symbol int, price float); "
    assert marks_of(other + "@info(name='q') from every e1=A -> e2=B within 1 sec select e1.price as p "
                    "insert into Out;") == (0, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def harness():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "native")])
    from host_harness_lib import HostHarnessApp
    return HostHarnessApp


@pytest.mark.parametrize("kind", ["flat", "per_stream"])
@pytest.mark.parametrize("c2", ["gt", "const"])
def test_plan_runs_on_the_host_nfa_with_the_pair_in_its_hidden_refs(harness, kind, c2):
    """The select reads e1.price and e2.volume: two visible refs, then the hidden (e1, e2) = the rule's pair, also when
    the lanes' state is carried across batches."""
    sid, cols, ts = stream(3000, seed=21)
    if kind == "per_stream":
        cols = per_stream_cols(cols)
    keys = keys_of(kind, "A", "B")
    t = mpat_text("A", "B", keys, 5, c2, select="e1.timestamp as i, e2.timestamp as j, e1.price as p, e2.volume as v")
    exp = feed(OracleApp, t, sid, cols, ts)
    pairs = rule_pairs("A", "B", sid, cols, ts, keys, 5, c2)
    assert len(exp) == len(pairs) >= 30
    for flush_every in (0, 997):
        got = feed(harness, t, sid, cols, ts, flush_every=flush_every)
        nvis = len(exp[0][2])
        assert [[r[0], r[1], r[2][:nvis]] for r in got] == exp
        np.testing.assert_array_equal(np.array([r[2][nvis:] for r in got], dtype=np.int64), pairs)
