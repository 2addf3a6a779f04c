"""The plan of `every e1=S1[c1] -> e2=S2[c2] within T2 -> ... -> ek=Sk[ck] within Tk` (3 <= k <= 8) over several streams
of one schema once the compiler marks it for the closed form of interleaved device batches (compiler.cpp fast_pat_k, k
hidden ordinal refs for the NFA hand-over), and the rule the device kernels (kernels/mpatk_dev.h) implement, tied to the
oracle on the CPU:

    R = {S1 .. Sk}. Take the events of a partition instance whose stream is in R, in arrival order (an event's instance
    key is the key attribute of its own stream; unpartitioned: all such events). Events of other streams do not exist
    for the query. For every event i on S1 with c1(i), put o1 = i and, for m = 2 .. k,
        om = min {j > o(m-1) : stream[j] = Sm, key[j] = key[i], cm(o1, ..., o(m-1), j)}.
    The chain stops without an output if om does not exist or ts[om] - ts[o(m-1)] > Tm (inclusive window, measured from
    the event bound before). The query emits (o1, ..., ok) in lexicographic order of (ok, o(k-1), ..., o1).

The numpy statement of that rule equals the oracle's outputs tuple for tuple for `ABC`, `ABA`, `ABB`, `AAB`, `AAA` and
`BCAB`, flat, partitioned by one attribute and by an attribute per stream, for four sets of windows and three forms of
cm, and on a 4-state and an 8-state chain. With event time that decreases the oracle differs from the rule, so the
device path hands that to the NFA kernel. Also the compiler's envelope for the mark, and the plan on the NFA built for
the host (tests/native) with the oracle's values and the tuple in its hidden refs. Test infrastructure: no GPU;
`-m "not gpu"`."""
import os
import subprocess

import numpy as np
import pytest

from test_mseq_plan import NAMES, SCHEMA, KEYCOL, decreasing_ts, feed, keys_of, oracle_tuples, per_stream_cols, stream
from oracle_lib import OracleApp

HERE = os.path.dirname(os.path.abspath(__file__))

CM = {
    "gt": ("price > {p}.price", lambda P, V, p, v: p > P[-1]),
    "compound": ("price > {p}.price - 25.0 and volume != e1.volume", lambda P, V, p, v: (p > P[-1] - 25.0) & (v != V[0])),
    "const": ("price > 45", lambda P, V, p, v: p > 45),
}
CHAIN4 = ["B", "C", "A", "B"]
CHAIN8 = ["A", "B", "A", "A", "B", "C", "A", "B"]  # (S1 among S2 .. S7: the rule holds, the compiler's mark does not)
CHAIN8_IN = ["A", "B", "C", "B", "B", "C", "B", "A"]


def withins_of(k, w):
    return {m: w for m in range(2, k + 1)} if isinstance(w, int) else dict(w)


def mpatk_text(pattern, keys=None, withins=40, cm="gt", select=None, c1="[price>20]"):
    """pattern: stream names in element order; keys: {stream: key attribute} (None: unpartitioned); withins: T in ms on
    every hop, or {m: T} on element m (1-based, m >= 2; an element left out has none); cm: the condition of elements
    2 .. k, {p} = the previous element."""
    k = len(pattern)
    w = withins_of(k, withins)
    els = [f"every e1={pattern[0]}{c1}"]
    for m in range(2, k + 1):
        wt = f" within {w[m]} milliseconds" if m in w else ""
        els.append(f"e{m}={pattern[m - 1]}[{CM[cm][0].format(p=f'e{m - 1}')}]{wt}")
    sel = select or ", ".join(f"e{m}.timestamp as i{m}" for m in range(1, k + 1))
    q = f"@info(name='q') from {' -> '.join(els)} select {sel} insert into OutputStream;"
    if keys is None:
        return SCHEMA + q
    return SCHEMA + "partition with (" + ", ".join(f"{x} of {s}" for s, x in keys.items()) + f") begin {q} end;"


def rule_tuples(pattern, sid, cols, ts, keys=None, withins=40, cm="gt"):
    """The rule above; (m, k) batch positions in order of (ok, ..., o1)."""
    k = len(pattern)
    w = withins_of(k, withins)
    want = [NAMES.index(s) for s in pattern]
    rows = np.nonzero(np.isin(sid, sorted(set(want))))[0]
    price, vol = cols[1], cols[2]
    key = np.zeros(len(rows), np.int64)
    if keys is not None:
        for s, x in keys.items():
            mine = sid[rows] == NAMES.index(s)
            key[mine] = cols[KEYCOL[x]][rows][mine]
    f = CM[cm][1]
    out = []
    for kv in np.unique(key):
        r = rows[key == kv]
        sr, pr, vr, tr = sid[r], price[r], vol[r], ts[r]
        on = [np.nonzero(sr == want[m])[0] for m in range(k)]
        for u in on[0][pr[on[0]] > 20]:
            o = [u]
            for m in range(1, k):
                c = on[m][np.searchsorted(on[m], o[-1], side="right"):]
                ok = f(pr[o], vr[o], pr[c], vr[c])
                if not ok.any():
                    break
                j = c[np.argmax(ok)]
                if tr[j] - tr[o[-1]] > w[m + 1]:
                    break
                o.append(j)
            if len(o) == k:
                out.append(tuple(r[o][::-1]))
    out.sort()
    return np.array([t[::-1] for t in out], dtype=np.int64).reshape(-1, k)


def case(kind, seed=11):
    sid, cols, ts = stream(seed=seed)
    if kind == "per_stream":
        cols = per_stream_cols(cols)
    return sid, cols, ts


SHAPES = {"ABC": list("ABC"), "ABA": list("ABA"), "ABB": list("ABB"), "AAB": list("AAB"), "AAA": list("AAA"),
          "BCAB": CHAIN4}
WITHINS = {"0": 0, "2": 2, "40": 40, "5_9": {2: 5, 3: 9}}
# (kind, withins, cm) with at least 30 outputs for `ABC` on both seeds
FLOOR_30 = {("symbol", "40", "gt"), ("symbol", "40", "compound"), ("symbol", "40", "const"),
            ("symbol", "5_9", "compound"), ("flat", "2", "gt"), ("flat", "2", "compound")}


@pytest.mark.parametrize("cm", list(CM))
@pytest.mark.parametrize("wname", list(WITHINS))
@pytest.mark.parametrize("kind", ["flat", "symbol", "per_stream"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_rule_equals_the_oracle(shape, kind, wname, cm):
    pattern = SHAPES[shape]
    k = len(pattern)
    w = WITHINS[wname]
    if isinstance(w, dict):
        w = {m: (5 if m == 2 else 9) for m in range(2, k + 1)}
    keys = keys_of(kind, pattern)
    for seed in (3, 11):
        sid, cols, ts = case(kind, seed)
        exp = oracle_tuples(mpatk_text(pattern, keys, w, cm), sid, cols, ts, k)
        got = rule_tuples(pattern, sid, cols, ts, keys, w, cm)
        if shape == "ABC" and (kind, wname, cm) in FLOOR_30:
            assert len(exp) >= 30
        np.testing.assert_array_equal(exp, got)
        if shape == "ABC" and kind == "symbol" and wname == "40" and cm == "const" and seed == 3:
            _, cnt = np.unique(exp[:, 2], return_counts=True)  # one ek completes many partials
            _, c2 = np.unique(exp[:, 1], return_counts=True)   # one e2 is shared by many tuples
            assert cnt.max() >= 5 and c2.max() >= 5


@pytest.mark.parametrize("within", [5, 40])
@pytest.mark.parametrize("partitioned", [True, False])
@pytest.mark.parametrize("k", [4, 8])
def test_chains_k4_and_k8(k, partitioned, within):
    pattern = CHAIN4 if k == 4 else CHAIN8
    sid, cols, ts = stream(4000, seed=7 + k, pattern=pattern)
    keys = keys_of("symbol" if partitioned else "flat", pattern)
    exp = oracle_tuples(mpatk_text(pattern, keys, within, "compound"), sid, cols, ts, k)
    if within == 40:
        assert len(exp) >= 1000
    np.testing.assert_array_equal(exp, rule_tuples(pattern, sid, cols, ts, keys, within, "compound"))


def test_rule_does_not_hold_when_event_time_decreases():
    """Flat and keyed, `within 5 ms` on decreasing event time: the oracle's outputs are not the rule's. This stays
    outside the device envelope (FAST_NON_MONOTONE: the NFA kernel takes the query over)."""
    sid, cols, ts = case("symbol")
    ts = decreasing_ts(ts)
    for keys in (None, keys_of("symbol", list("ABC"))):
        exp = oracle_tuples(mpatk_text(list("ABC"), keys, 5), sid, cols, ts, 3)
        got = rule_tuples(list("ABC"), sid, cols, ts, keys, 5)
        assert len(exp) > 0 and not np.array_equal(exp, got)


def test_the_compilers_envelope():
    """(fast_pat_k, fast_pat_ms, fast_every_within, fast_seq_adjacent, fast_seq_k, fast_seq_ms) of the compiler's plan."""
    from test_mpatk_emu import marks_of
    from test_mpat_plan import mpat_text, keys_of as keys2, C2
    none = (0, 0, 0, 0, 0, 0)
    q = lambda body, sel="e1.timestamp as i": SCHEMA + f"@info(name='q') from {body} select {sel} insert into Out;"
    part = lambda with_, body: SCHEMA + f"partition with ({with_}) begin @info(name='q') from {body} " \
                                        "select e1.timestamp as i insert into Out; end;"
    for pattern in (list("ABC"), list("ABA"), CHAIN4, CHAIN8_IN):
        k = len(pattern)
        for kind in ("flat", "symbol", "per_stream"):
            for cm in CM:
                assert marks_of(mpatk_text(pattern, keys_of(kind, pattern), 40, cm)) == (k, 0, 0, 0, 0, 0)
        # a hop without a within
        for miss in range(2, k + 1):
            w = {m: 40 for m in range(2, k + 1) if m != miss}
            assert marks_of(mpatk_text(pattern, None, w)) == none
    abc = "every e1=A[price>20] -> e2=B[price>e1.price] within 1 sec -> e3=C[price>e2.price] within 1 sec"
    assert marks_of(q(abc, "e1.price as p, e3.price as r")) == (3, 0, 0, 0, 0, 0)
    assert marks_of(part("symbol of A, volume of B, symbol of C", abc)) == (3, 0, 0, 0, 0, 0)
    # S1 among S2 .. S(k-1); a parenthesised every; a having; a STRING key; an expression key; refs at another index
    assert marks_of(mpatk_text(list("AAB"))) == none and marks_of(mpatk_text(CHAIN8)) == none
    assert marks_of(q("every (e1=A -> e2=B within 1 sec) -> e3=C within 1 sec")) == none
    assert marks_of(q(abc, "e1.timestamp as i having i > 3")) == none
    named = "".join(f"define stream {s} (name string, price double, volume long, timestamp long); " for s in "ABC")
    assert marks_of(named + "partition with (name of A, name of B, name of C) begin @info(name='q') from " + abc +
                    " select e1.timestamp as i insert into Out; end;") == none
    assert marks_of(part("symbol + 1 of A, symbol of B, symbol of C", abc)) == none
    assert marks_of(q("every e1=A -> e2=B<2:3> within 1 sec -> e3=C[price>e2[1].price] within 1 sec")) == none
    # a within on e1, on the root; one stream only; a count, a logical element; the sequence form; other schemas
    assert marks_of(q("every e1=A within 5 milliseconds -> e2=B within 1 sec -> e3=C within 1 sec")) == none
    assert marks_of(q("every e1=A -> e2=A within 1 sec -> e3=A within 1 sec")) == none
    assert marks_of(q("every e1=A -> e2=B within 1 sec -> (e3=C and e4=A) within 1 sec")) == none
    assert marks_of(q("every e1=A, e2=B within 1 sec, e3=C within 1 sec")) == (0, 0, 0, 0, 0, 3)
    other = "define stream A (symbol int, price double); define stream B (symbol int, price float); "
    assert marks_of(other + "@info(name='q') from every e1=A -> e2=B within 1 sec -> e3=A within 1 sec select e1.price "
                    "as p insert into Out;") == none
    # every text of tests/test_mpat_plan.py::test_the_compilers_envelope keeps its marks
    yes = (0, 1, 0, 0, 0, 0)
    for kind in ("flat", "symbol", "per_stream"):
        for c2 in C2:
            assert marks_of(mpat_text("A", "B", keys2(kind, "A", "B"), 5, c2)) == yes
    assert marks_of(mpat_text("B", "A", None, 0)) == yes and marks_of(mpat_text("C", "A", keys2("symbol", "C", "A"))) == yes
    assert marks_of(q("every e1=A[price>20] -> e2=B[price>e1.price] within 1 sec", "e1.price as p, e2.price as r")) == yes
    assert marks_of(q("every e1=A -> e2=B within 1 sec")) == yes
    assert marks_of(mpat_text("A", "B", None, None)) == none
    assert marks_of(mpat_text("A", "B", keys2("symbol", "A", "B"), None)) == none
    assert marks_of(q("every e1=A[price>20] within 5 milliseconds -> e2=B[price>e1.price] within 1 sec")) == none
    assert marks_of(q("every (e1=A[price>20] -> e2=B[price>e1.price]) within 1 sec")) == none
    assert marks_of(q("every e1=A[price>20] -> e2=A[price>e1.price] within 1 sec")) == (0, 0, 1, 0, 0, 0)
    assert marks_of(q("every e1=A[price>20], e2=B[price>e1.price] within 1 sec")) == (0, 0, 0, 0, 0, 2)
    assert marks_of(q("every e1=A[price>20], e2=A[price>e1.price] within 1 sec")) == (0, 0, 0, 1, 0, 0)
    assert marks_of(q("every e1=A -> e2=B -> e3=A within 1 sec")) == none
    assert marks_of(q("every e1=A -> e2=B<2:3> within 1 sec")) == none
    assert marks_of(q("every e1=A -> (e2=B and e3=C) within 1 sec")) == none
    assert marks_of(q("every e1=A -> e2=B within 1 sec", "e1.timestamp as i having i > 3")) == none
    assert marks_of(q("e1=A[price>20] -> e2=B[price>e1.price] within 1 sec")) == none
    assert marks_of(part("symbol of A, volume of B", "every e1=A -> e2=B within 1 sec")) == yes
    assert marks_of(part("symbol + 1 of A, symbol of B", "every e1=A -> e2=B within 1 sec")) == none
    named2 = "".join(f"define stream {s} (name string, price double, volume long, timestamp long); " for s in "AB")
    assert marks_of(named2 + "partition with (name of A, name of B) begin @info(name='q') from every e1=A -> e2=B "
                    "within 1 sec select e1.timestamp as i insert into Out; end;") == none
    assert marks_of(other + "@info(name='q') from every e1=A -> e2=B within 1 sec select e1.price as p "
                    "insert into Out;") == none


@pytest.fixture(scope="module")
def harness():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "native")])
    from host_harness_lib import HostHarnessApp
    return HostHarnessApp


@pytest.mark.parametrize("kind", ["flat", "per_stream"])
@pytest.mark.parametrize("shape,cm", [("ABC", "compound"), ("ABA", "const"), ("BCAB", "gt")])
def test_plan_runs_on_the_host_nfa_with_the_tuple_in_its_hidden_refs(harness, shape, cm, kind):
    """The select reads e1 and ek only: two visible refs, then the k hidden ones (slot m, index 0) = the rule's tuple,
    also when the lanes' state is carried across batches."""
    pattern = SHAPES[shape]
    k = len(pattern)
    sid, cols, ts = stream(3000, seed=21)
    if kind == "per_stream":
        cols = per_stream_cols(cols)
    keys = keys_of(kind, pattern)
    t = mpatk_text(pattern, keys, 40, cm, select=f"e1.timestamp as i, e{k}.timestamp as j")
    exp = feed(OracleApp, t, sid, cols, ts)
    tuples = rule_tuples(pattern, sid, cols, ts, keys, 40, cm)
    assert len(exp) == len(tuples) >= 10
    for flush_every in (0, 997):
        got = feed(harness, t, sid, cols, ts, flush_every=flush_every)
        assert [[r[0], r[1], r[2][:2]] for r in got] == exp
        np.testing.assert_array_equal(np.array([r[2][2:] for r in got], dtype=np.int64), tuples)
