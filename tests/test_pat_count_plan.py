"""The plan of the count pattern `every e1=A[c1] -> e2=B[c2]<m:n> -> e3=C[c3] within T` once the compiler marks it for
the closed form of interleaved device batches (compiler.cpp fast_pat_count, the hidden (e1, e2[0] .. e2[n-1], e3) ordinal
refs for the NFA hand-over), and the rule the device kernels (kernels/mpat_count_dev.h) implement, tied to the oracle on
the CPU:

    R = {A, B, C}. Take the rows of a partition instance whose stream is in R, in arrival order (a row's instance is the
    key attribute of its own stream; unpartitioned: all such rows). Heartbeat rows (-1) and rows of other streams do not
    exist for the query. For every A row i with c1(i):
        hits     the later B rows j of the instance with c2(i, j), in order; the partial binds the first n of them
        p(i)     the row of the m-th hit (i itself if m = 0): from there on the partial also waits for e3
        tlast(j) the time of the last hit bound before row j, or ts[i] if none
    Walk the C rows j > p(i) of the instance in order, whether or not they pass c3: if ts[j] - tlast(j) > T the partial
    is dead (no output, no more hits, no revival); otherwise, if c3(i, j), it emits (i, hits bound before j, j) with j's
    timestamp and ends. If B = C a row is tried as C first and then as B. Nothing else ends a partial. Outputs come in
    order of (j, p(i), i).

The numpy statement of that rule equals the oracle's outputs tuple for tuple and in order, for the stream assignments
(A, B, C), (C, A, B), (A, B, A), (A, A, C) and (A, B, B), flat, keyed by one attribute and with the count's stream keyed
by another, for ten counts, without a `within` and with two, on two seeds; with heartbeat rows, with a partition that also
keys an unread stream, for three pairs of conditions. Measuring the window from e1, or letting a partial that failed the
window live on (which, event time not decreasing, is also what a later hit re-admitting it would give), gives other
outputs, and so does decreasing event time (outside the device envelope). Also the compiler's envelope for the mark. Test
infrastructure: no GPU; `-m "not gpu"`."""
import numpy as np
import pytest

from test_mseq_plan import NAMES, SCHEMA, KEYCOL, decreasing_ts, per_stream_cols, stream
from test_pat_logic_plan import CONDS, case
from oracle_lib import OracleApp

ASSIGN = {"ABC": ("A", "B", "C"), "CAB": ("C", "A", "B"), "ABA": ("A", "B", "A"), "AAC": ("A", "A", "C"),
          "ABB": ("A", "B", "B")}
# (text, m, n); n = None: unbounded
COUNTS = {"2_4": ("<2:4>", 2, 4), "1_": ("<1:>", 1, None), "0_3": ("<0:3>", 0, 3), "3_": ("<3:>", 3, None),
          "2_2": ("<2:2>", 2, 2), "1_1": ("<1:1>", 1, 1), "opt": ("<0:1>", 0, 1), "3_3": ("<3:3>", 3, 3),
          "2_6": ("<2:6>", 2, 6), "6_6": ("<6:6>", 6, 6)}
WITHINS = [None, 5, 40]
NULL = -1  # an unbound slot's position: its timestamp attribute is null
WIDTH = 6  # hit slots selected by the texts of this file


def count_text(count, a, b, c, keys=None, within=5, conds="gt_lt", select=None, c1="[price>20]", tail="", width=WIDTH):
    """keys: {stream: key attribute} (None: unpartitioned); within: T in ms on the last element (None: no within)."""
    w = "" if within is None else f" within {within} milliseconds"
    c2, c3 = COUNT_CONDS[conds]
    if select is None:
        select = "e1.timestamp as i, " + ", ".join(f"e2[{k}].timestamp as j{k}" for k in range(width)) + \
                 ", e2[last].timestamp as jl, e3.timestamp as k"
    q = (f"@info(name='q') from every e1={a}{c1} -> e2={b}[{c2[0]}]{COUNTS[count][0]} -> e3={c}[{c3[0]}]{w} "
         f"select {select}{tail} insert into OutputStream;")
    if keys is None:
        return SCHEMA + q
    return SCHEMA + "partition with (" + ", ".join(f"{x} of {s}" for s, x in keys.items()) + f") begin {q} end;"


LT = ("price < e1.price", lambda p1, v1, p2, v2: p2 < p1)
# the issue's pair (c2 `price > e1.price`, c3 `price < e1.price`), and the pairs of the logical pair's test
COUNT_CONDS = dict(CONDS, gt_lt=(CONDS["gt_gt"][0], LT))


def rule_tuples(count, a, b, c, sid, cols, ts, keys=None, within=5, conds="gt_lt", model="rule", with_p=False):
    """The rule above; (outputs, WIDTH + 3) batch positions (i, the first WIDTH hit slots, the last hit, j), NULL for an
    unbound slot, in order of (j, p, i). model: "from_e1" measures the window from e1; "no_death" lets a partial that
    failed the window live on."""
    _, m, n = COUNTS[count]
    sa, sb, sc = (NAMES.index(x) for x in (a, b, c))
    price, vol = cols[1], cols[2]
    key = np.zeros(len(sid), np.int64)
    if keys is not None:
        for s in {a, b, c}:
            mine = sid == NAMES.index(s)
            key[mine] = cols[KEYCOL[keys[s]]][mine]
    read = np.isin(sid, [sa, sb, sc])
    f2, f3 = COUNT_CONDS[conds][0][1], COUNT_CONDS[conds][1][1]
    out = []
    for k in np.unique(key[read]):
        r = np.nonzero(read & (key == k))[0]
        isb, isc = sid[r] == sb, sid[r] == sc
        for u in np.nonzero((sid[r] == sa) & (price[r] > 20))[0]:
            i = r[u]
            later = r[u + 1:]
            hits = later[isb[u + 1:] & f2(price[i], vol[i], price[later], vol[later])]
            if n is not None:
                hits = hits[:n]
            if len(hits) < m:
                continue
            p = i if m == 0 else hits[m - 1]
            cs = later[isc[u + 1:]]
            cs = cs[cs > p]  # (B = C: a row is tried as C first, with the hits in front of it, so the m-th hit is no e3)
            if not len(cs):
                continue
            before = np.searchsorted(hits, cs, side="left")  # hits bound before each C row
            hts = np.concatenate(([ts[i]], ts[hits]))  # tlast by the number of hits in front
            tlast = hts[before]
            if within is None:
                late = np.zeros(len(cs), bool)
            else:
                late = ts[cs] - (ts[i] if model == "from_e1" else tlast) > within
            ok = f3(price[i], vol[i], price[cs], vol[cs]) & ~late
            stop = ok if model == "no_death" else ok | late
            if not stop.any():
                continue
            x = int(np.argmax(stop))
            if not ok[x]:
                continue  # dead
            h = [int(v) for v in hits[:before[x]]]
            out.append((int(cs[x]), int(p), int(i), h))
    out.sort(key=lambda o: o[:3])
    tup = np.array([[i] + (h + [NULL] * WIDTH)[:WIDTH] + [h[-1] if h else NULL, j] for j, _, i, h in out],
                   dtype=np.int64).reshape(-1, WIDTH + 3)
    return (tup, np.array([o[1] for o in out], dtype=np.int64)) if with_p else tup


def oracle_tuples(text, sid, cols, ts, with_ts=False):
    """The selected positions: the timestamp attribute is the row's position in the feed; a null one is NULL."""
    a = OracleApp(text)
    a.start()
    a.send_interleaved_ord(sid, ts, np.arange(len(ts), dtype=np.int64), list(cols))
    out = a.outputs()["streams"].get("OutputStream", [])
    a.close()
    w = len(out[0][1]) if out else WIDTH + 3
    tup = np.array([[NULL if x is None else x for x in r[1]] for r in out], dtype=np.int64).reshape(-1, w)
    return (tup, np.array([r[0] for r in out], dtype=np.int64)) if with_ts else tup


def keys_of(kind, a, b, c, also=None):
    """symbol: every read stream by symbol; per_stream: the count's stream by volume (e3's when B is A)."""
    if kind == "flat":
        return None
    k = {s: "symbol" for s in (a, b, c)}
    if kind == "per_stream":
        k[b if b != a else c] = "volume"
    if also:
        k[also] = "symbol"
    return k


# the oracle's own outputs (seed 3, streams (A, B, C), c2 `price > e1.price`, c3 `price < e1.price`); asserted at 80 %
FLOORS = {("2_4", "flat", 5): 696, ("2_4", "symbol", 5): 205, ("2_2", "flat", 5): 604, ("2_2", "symbol", 5): 163,
          ("1_1", "flat", 5): 612, ("0_3", "flat", 5): 730, ("2_4", "flat", 40): 904}


@pytest.mark.parametrize("kind", ["flat", "symbol", "per_stream"])
@pytest.mark.parametrize("count", list(COUNTS))
@pytest.mark.parametrize("assign", list(ASSIGN))
def test_rule_equals_the_oracle(assign, count, kind):
    """Seeds 3 and 11, no within, 5 ms and 40 ms. The shared-stream assignments and the unbounded counts are outside the
    device envelope (no mark, test_the_compilers_envelope); the rule is compared there all the same."""
    a, b, c = ASSIGN[assign]
    keys = keys_of(kind, a, b, c)
    for seed in (3, 11):
        sid, cols, ts = case(kind, seed)
        for within in WITHINS:
            got = rule_tuples(count, a, b, c, sid, cols, ts, keys, within)
            exp = oracle_tuples(count_text(count, a, b, c, keys, within), sid, cols, ts)
            if seed == 3 and assign == "ABC" and (count, kind, within) in FLOORS:
                assert len(exp) >= 0.8 * FLOORS[(count, kind, within)], len(exp)
            assert len(exp) >= 3, (seed, within)
            np.testing.assert_array_equal(exp, got, err_msg=f"seed {seed} within {within}")


@pytest.mark.parametrize("conds", ["const_compound", "compound_gt"])
@pytest.mark.parametrize("count", ["2_4", "0_3", "opt"])
def test_other_conditions(count, conds):
    for kind in ("flat", "symbol"):
        keys = keys_of(kind, "A", "B", "C")
        sid, cols, ts = case(kind, 3)
        for within in (5, 40):
            exp = oracle_tuples(count_text(count, "A", "B", "C", keys, within, conds), sid, cols, ts)
            assert len(exp) >= 20
            np.testing.assert_array_equal(exp, rule_tuples(count, "A", "B", "C", sid, cols, ts, keys, within, conds))


@pytest.mark.parametrize("kind", ["flat", "symbol", "per_stream"])
@pytest.mark.parametrize("count", ["2_4", "0_3"])
def test_heartbeats_and_the_output_timestamp(count, kind):
    """The output timestamp is e3's."""
    keys = keys_of(kind, "A", "B", "C")
    sid, cols, ts = case(kind, 3, 0.18)
    assert (sid == -1).sum() > 600
    for within in (5, 40):
        exp, ets = oracle_tuples(count_text(count, "A", "B", "C", keys, within), sid, cols, ts, with_ts=True)
        assert len(exp) >= 30
        np.testing.assert_array_equal(exp, rule_tuples(count, "A", "B", "C", sid, cols, ts, keys, within))
        np.testing.assert_array_equal(ets, ts[exp[:, -1]])


@pytest.mark.parametrize("within", [5, 40])
def test_a_partition_that_also_keys_an_unread_stream(within):
    """`A -> e2=B<2:4> -> e3=A`: rows of C are keyed by the partition and not read by the query."""
    keys = keys_of("symbol", "A", "B", "A", also="C")
    sid, cols, ts = case("symbol", 3)
    exp = oracle_tuples(count_text("2_4", "A", "B", "A", keys, within), sid, cols, ts)
    assert len(exp) >= 30
    np.testing.assert_array_equal(exp, rule_tuples("2_4", "A", "B", "A", sid, cols, ts, keys, within))


@pytest.mark.parametrize("seed", [3, 11])
@pytest.mark.parametrize("model", ["from_e1", "no_death"])
def test_other_models_of_the_window_differ(model, seed):
    """The window measured from e1 loses most outputs; a partial that survives a failed window check (equally: one a
    later hit re-admits, event time not decreasing) gains some."""
    for kind, within in (("flat", 5), ("symbol", 5)):
        keys = keys_of(kind, "A", "B", "C")
        sid, cols, ts = case(kind, seed)
        exp = oracle_tuples(count_text("2_4", "A", "B", "C", keys, within), sid, cols, ts)
        got = rule_tuples("2_4", "A", "B", "C", sid, cols, ts, keys, within, model=model)
        assert len(exp) >= 100 and not np.array_equal(exp, got)
        assert len(got) < len(exp) if model == "from_e1" else len(got) > len(exp)
        if seed == 3 and kind == "flat":
            # the issue's figures: the oracle 696; from e1 30; a later hit re-admitting an expired partial 816. With
            # event time not decreasing, every C row between a failed check and the next hit fails too, so letting the
            # partial live on is that third model: the count ties the two
            assert len(exp) == 696 and len(got) == (30 if model == "from_e1" else 816)


def test_a_full_partial_past_its_window_is_never_completed():
    """The carry drops a partial with n hits whose last hit is older than T at the batch's last row: under the rule its
    next C row kills it, and event time does not decrease. Counted here: no output's e3 lies more than T after its last
    hit, and none more than T after e1 when nothing is bound."""
    sid, cols, ts = case("flat", 3)
    for count in ("2_4", "0_3", "2_2"):
        exp = oracle_tuples(count_text(count, "A", "B", "C", None, 5), sid, cols, ts)
        last = np.where(exp[:, -2] >= 0, exp[:, -2], exp[:, 0])
        assert len(exp) > 100 and (ts[exp[:, -1]] - ts[last] <= 5).all()


def test_rule_does_not_hold_when_event_time_decreases():
    """Flat and keyed on decreasing event time: the oracle's outputs are not the rule's (outside the device envelope:
    FAST_NON_MONOTONE, the NFA kernel takes the query over)."""
    sid, cols, ts = case("symbol", 3)
    ts = decreasing_ts(ts)
    for keys in (None, keys_of("symbol", "A", "B", "C")):
        exp = oracle_tuples(count_text("2_4", "A", "B", "C", keys, 5), sid, cols, ts)
        got = rule_tuples("2_4", "A", "B", "C", sid, cols, ts, keys, 5)
        assert len(exp) >= 30 and not np.array_equal(exp, got)


def test_a_within_on_the_count_element_stays_unmarked_and_changes_nothing_here():
    sid, cols, ts = case("flat", 3)
    base = oracle_tuples(count_text("2_4", "A", "B", "C", None, None), sid, cols, ts)
    text = count_text("2_4", "A", "B", "C", None, None).replace("<2:4> ->", "<2:4> within 5 milliseconds ->")
    assert "within 5" in text
    assert len(oracle_tuples(text, sid, cols, ts)) == len(base)


def test_the_compilers_envelope():
    """fast_pat_count (n, or 0) of the plan the compiler makes, with m, match_arity and the hidden refs
    (e1, e2[0] .. e2[n-1], e3); every other mark stays 0 for the count texts, and the forms of paths 6-13 keep theirs."""
    from test_pat_count_emu import count_mark_of, plan_of
    from test_pat_logic_emu import marks_of
    q = lambda body, sel="e1.timestamp as i": SCHEMA + f"@info(name='q') from {body} select {sel} insert into Out;"
    part = lambda with_, body: SCHEMA + f"partition with ({with_}) begin @info(name='q') from {body} " \
                                        "select e1.timestamp as i insert into Out; end;"
    no = (0, 0)
    old_none = (0,) * 9
    for name, (txt, m, n) in COUNTS.items():
        inside = n is not None and n <= 6
        for assign, abc in ASSIGN.items():
            for kind in ("flat", "symbol", "per_stream"):
                text = count_text(name, *abc, keys_of(kind, *abc), 5, width=min(n or 1, 6))
                want = (m, n) if inside and assign in ("ABC", "CAB") else no
                assert count_mark_of(text) == want, (name, assign, kind)
                assert marks_of(text) == old_none
        if inside:
            arity, hidden = plan_of(count_text(name, "A", "B", "C", None, 5, width=n))
            assert arity == n + 2 and hidden == [(0, 0)] + [(1, k) for k in range(n)] + [(2, 0)]
    for conds in COUNT_CONDS:
        assert count_mark_of(count_text("2_4", "A", "B", "C", None, 5, conds, width=4)) == (2, 4)
    assert count_mark_of(q("every e1=A -> e2=B<2:4> -> e3=C within 1 sec")) == (2, 4)
    assert count_mark_of(q("every e1=A -> e2=B<0:1> -> e3=C within 1 sec")) == (0, 1)
    assert count_mark_of(q("every e1=A[price>20] -> e2=B[price>e1.price]<2:4> -> e3=C[price<e1.price] within 1 sec",
                           "e1.price as p, e2[0].volume as v, e2[3].price as w, e2[last].price as l, e3.price as r, "
                           "7 as c")) == (2, 4)
    assert count_mark_of(part("symbol of A, volume of B, symbol of C", "every e1=A -> e2=B<2:4> -> e3=C within 1 sec")) \
        == (2, 4)
    # out of scope: unbounded counts and n > 6, a slot past n or counted from the end in a select, e2[k] / e2[last] in a
    # condition, c3 reading e2, no within, a within elsewhere, a having, a longer chain, a count elsewhere, a sequence,
    # expression and STRING keys, a stream of the pattern without a key, different schemas
    # (`+`, `*` and `?` are written in sequences only; a pattern writes them `<1:>`, `<0:>` and `<0:1>`)
    for body in ("every e1=A, e2=B+, e3=C within 1 sec", "every e1=A, e2=B*, e3=C within 1 sec",
                 "every e1=A, e2=B?, e3=C within 1 sec", "every e1=A -> e2=B<1:> -> e3=C within 1 sec",
                 "every e1=A -> e2=B<0:> -> e3=C within 1 sec", "every e1=A -> e2=B<2:> -> e3=C within 1 sec", "every e1=A -> e2=B<2:7> -> e3=C within 1 sec",
                 "every e1=A -> e2=B<2:4> -> e3=C[price>e2[0].price] within 1 sec",
                 "every e1=A -> e2=B<2:4> -> e3=C[price>e2[last].price] within 1 sec",
                 "every e1=A -> e2=B[price>e2[last].price]<2:4> -> e3=C within 1 sec",
                 "every e1=A -> e2=B<2:4> -> e3=C",
                 "every e1=A -> e2=B<2:4> within 5 milliseconds -> e3=C",
                 "every e1=A -> e2=B<2:4> within 5 milliseconds -> e3=C within 1 sec",
                 "every e1=A within 5 milliseconds -> e2=B<2:4> -> e3=C within 1 sec",
                 "every (e1=A -> e2=B<2:4> -> e3=C within 1 sec) within 2 sec",
                 "every e1=A -> e2=B<2:4> -> e3=C within 1 sec -> e4=A",
                 "every e1=A<2:4> -> e2=B -> e3=C within 1 sec",
                 "every e1=A -> e2=B -> e3=C<2:4> within 1 sec",
                 "e1=A -> e2=B<2:4> -> e3=C within 1 sec",
                 "every e1=A, e2=B<2:4>, e3=C within 1 sec"):
        assert count_mark_of(q(body)) == no, body
    assert count_mark_of(q("every e1=A -> e2=B<2:4> -> e3=C within 1 sec", "e2[4].price as p")) == no
    assert count_mark_of(q("every e1=A -> e2=B<2:4> -> e3=C within 1 sec", "e2[last - 1].price as p")) == no
    assert count_mark_of(q("every e1=A -> e2=B<2:4> -> e3=C within 1 sec", "e1.timestamp as i having i > 3")) == no
    assert count_mark_of(part("symbol + 1 of A, symbol of B, symbol of C", "every e1=A -> e2=B<2:4> -> e3=C within 1 sec")) == no
    assert count_mark_of(part("symbol of A, symbol of C", "every e1=A -> e2=B<2:4> -> e3=C within 1 sec")) == no
    named = "".join(f"define stream {s} (name string, price double, volume long, timestamp long); " for s in "ABC")
    assert count_mark_of(named + "partition with (name of A, name of B, name of C) begin @info(name='q') from every e1=A -> "
                         "e2=B<2:4> -> e3=C within 1 sec select e1.timestamp as i insert into Out; end;") == no
    other = ("define stream A (symbol int, price double); define stream B (symbol int, price float); "
             "define stream C (symbol int, price double); ")
    assert count_mark_of(other + "@info(name='q') from every e1=A -> e2=B<2:4> -> e3=C within 1 sec select e1.price as p "
                         "insert into Out;") == no
    # the forms of paths 6-13 keep their marks, and have none of the new one
    pb = "@app:playback "
    for text, marks in ((q("every e1=A -> e2=B and e3=C within 1 sec"), (1, 0, 0, 0, 0, 0, 0, 0, 0)),
                        (pb + q("every e1=A[price>20] -> not B[price>70] and e3=C[price>e1.price] within 1 sec"),
                         (0, 1, 0, 0, 0, 0, 0, 0, 0)),
                        (pb + q("every e1=A[price>20] -> not B[price>70] for 1 sec"), (0, 0, 1, 0, 0, 0, 0, 0, 0)),
                        (q("every e1=A[price>20] -> e2=B[price>e1.price] within 1 sec"), (0, 0, 0, 1, 0, 0, 0, 0, 0)),
                        (q("every e1=A[price>20] -> e2=A[price>e1.price] within 1 sec"), (0, 0, 0, 0, 1, 0, 0, 0, 0)),
                        (q("every e1=A, e2=B"), (0, 0, 0, 0, 0, 0, 0, 2, 0)),
                        (q("every e1=A -> e2=B within 1 sec -> e3=A within 1 sec"), (0, 0, 0, 0, 0, 0, 0, 0, 3))):
        assert marks_of(text) == marks and count_mark_of(text) == no
