"""The plan of the logical pair `every e1=A[c1] -> e2=B[c2] and|or e3=C[c3] within T` once the compiler marks it for the
closed form of interleaved device batches (compiler.cpp fast_pat_logic, the hidden (e1, e2, e3) ordinal refs for the NFA
hand-over), and the rule the device kernels (kernels/mpat_logic_dev.h) implement, tied to the oracle on the CPU:

    R = {A, B, C}. Take the rows of a partition instance whose stream is in R, in arrival order (a row's instance is the
    key attribute of its own stream; unpartitioned: all such rows). Heartbeat rows (-1) and rows of other streams do not
    exist for the query. For every A row i with c1(i), let
        j2(i) = min {j > i : stream[j] = B, same instance, c2(i, j)}
        j3(i) = min {j > i : stream[j] = C, same instance, c3(i, j)}
    and: emits (i, j2, j3) iff both exist and ts[max(j2, j3)] - ts[i] <= T; in order of (max(j2, j3), i), with the
         timestamp of max(j2, j3).
    or:  with jm the smaller of those that exist, emits (i, j2 or null, j3 or null), only the side at jm bound, iff jm
         exists and ts[jm] - ts[i] <= T; in order of (jm, i), with the timestamp of jm.
    The window is measured from e1.

The numpy statement of that rule equals the oracle's outputs tuple for tuple and in order, for both operators, the stream
assignments (A, B, C), (C, A, B), (A, B, A) and (A, A, C), flat, keyed by one attribute and with one operand's stream
keyed by another, without a `within` and with four, for three pairs of conditions, on two seeds: 720 runs; with heartbeat
rows, with a partition that also keys an unread stream. Measuring the window from the event bound last gives other
outputs, and so does decreasing event time under a `within` (outside the device envelope). Also the compiler's envelope
for the mark. Test infrastructure: no GPU; `-m "not gpu"`."""
import numpy as np
import pytest

from test_mseq_plan import NAMES, SCHEMA, KEYCOL, decreasing_ts, per_stream_cols, stream
from oracle_lib import OracleApp

GT = ("price > e1.price", lambda p1, v1, p2, v2: p2 > p1)
CONST = ("price > 45", lambda p1, v1, p2, v2: p2 > 45)
COMPOUND = ("price > e1.price - 25.0 and volume != e1.volume", lambda p1, v1, p2, v2: (p2 > p1 - 25.0) & (v2 != v1))
CONDS = {"gt_gt": (GT, GT), "const_compound": (CONST, COMPOUND), "compound_gt": (COMPOUND, GT)}
ASSIGN = {"ABC": ("A", "B", "C"), "CAB": ("C", "A", "B"), "ABA": ("A", "B", "A"), "AAC": ("A", "A", "C")}
WITHINS = [None, 0, 2, 5, 40]
NULL = -1  # an absent member's position: its timestamp attribute is null


def logic_text(op, a, b, c, keys=None, within=5, conds="gt_gt",
               select="e1.timestamp as i, e2.timestamp as j, e3.timestamp as k", c1="[price>20]", tail=""):
    """keys: {stream: key attribute} (None: unpartitioned); within: T in ms (None: no within)."""
    w = "" if within is None else f" within {within} milliseconds"
    c2, c3 = CONDS[conds]
    q = (f"@info(name='q') from every e1={a}{c1} -> e2={b}[{c2[0]}] {op} e3={c}[{c3[0]}]{w} select {select}{tail} "
         "insert into OutputStream;")
    if keys is None:
        return SCHEMA + q
    return SCHEMA + "partition with (" + ", ".join(f"{x} of {s}" for s, x in keys.items()) + f") begin {q} end;"


def rule_tuples(op, a, b, c, sid, cols, ts, keys=None, within=5, conds="gt_gt", from_last=False):
    """The rule above; (m, 3) batch positions (NULL: absent) in order of (completing member, i). from_last=True measures
    the `and` window from the member bound first instead of from e1 (path 10's per-hop windows)."""
    sa, sb, sc = (NAMES.index(x) for x in (a, b, c))
    price, vol = cols[1], cols[2]
    key = np.zeros(len(sid), np.int64)
    if keys is not None:
        for s in {a, b, c}:
            mine = sid == NAMES.index(s)
            key[mine] = cols[KEYCOL[keys[s]]][mine]
    read = np.isin(sid, [sa, sb, sc])
    f2, f3 = CONDS[conds][0][1], CONDS[conds][1][1]
    out = []
    for k in np.unique(key[read]):
        r = np.nonzero(read & (key == k))[0]
        isb, isc = sid[r] == sb, sid[r] == sc
        for u in np.nonzero((sid[r] == sa) & (price[r] > 20))[0]:
            i = r[u]
            later = r[u + 1:]
            ok2 = isb[u + 1:] & f2(price[i], vol[i], price[later], vol[later])
            ok3 = isc[u + 1:] & f3(price[i], vol[i], price[later], vol[later])
            j2 = int(later[np.argmax(ok2)]) if ok2.any() else None
            j3 = int(later[np.argmax(ok3)]) if ok3.any() else None
            if op == "and":
                if j2 is None or j3 is None:
                    continue
                jm = max(j2, j3)
                t0 = ts[min(j2, j3)] if from_last else ts[i]
                if within is not None and (ts[jm] - t0 > within or (from_last and ts[min(j2, j3)] - ts[i] > within)):
                    continue
                out.append((jm, i, j2, j3))
            else:
                if j2 is None and j3 is None:
                    continue
                jm = min(x for x in (j2, j3) if x is not None)
                if within is not None and ts[jm] - ts[i] > within:
                    continue
                out.append((jm, i, j2 if j2 == jm else NULL, j3 if j3 == jm else NULL))
    out.sort()
    return np.array([(i, j2, j3) for _, i, j2, j3 in out], dtype=np.int64).reshape(-1, 3)


def oracle_tuples(text, sid, cols, ts, with_ts=False):
    """(e1, e2, e3) positions: the timestamp attribute is the row's position in the feed; a null one is NULL."""
    a = OracleApp(text)
    a.start()
    a.send_interleaved_ord(sid, ts, np.arange(len(ts), dtype=np.int64), list(cols))
    out = a.outputs()["streams"].get("OutputStream", [])
    a.close()
    tup = np.array([[NULL if x is None else x for x in r[1][:3]] for r in out], dtype=np.int64).reshape(-1, 3)
    return (tup, np.array([r[0] for r in out], dtype=np.int64)) if with_ts else tup


def keys_of(kind, a, b, c, also=None):
    """symbol: every read stream by symbol; per_stream: e2's stream by volume (e3's when B is A)."""
    if kind == "flat":
        return None
    k = {s: "symbol" for s in (a, b, c)}
    if kind == "per_stream":
        k[b if b != a else c] = "volume"
    if also:
        k[also] = "symbol"
    return k


def case(kind, seed=3, heartbeats=0.0):
    sid, cols, ts = stream(seed=seed)
    if kind == "per_stream":
        cols = per_stream_cols(cols)
    if heartbeats:
        sid = sid.copy()
        sid[np.random.default_rng(seed + 100).random(len(sid)) < heartbeats] = -1
    return sid, cols, ts


def some(op, keyed, within):
    """A floor for the cases without a tabulated count: keyed `and` within 5 ms has about ten outputs here."""
    return 5 if op == "and" and keyed and within < 40 else 30


# the oracle's own outputs (seed 3, streams (A, B, C), both conditions `price > e1.price`); asserted at 80 %
FLOORS = {("and", "flat", 5): 191, ("and", "flat", 40): 767, ("and", "symbol", 40): 300,
          ("or", "flat", 0): 77, ("or", "symbol", 5): 183, ("or", "symbol", 40): 650}


@pytest.mark.parametrize("conds", list(CONDS))
@pytest.mark.parametrize("within", WITHINS)
@pytest.mark.parametrize("kind", ["flat", "symbol", "per_stream"])
@pytest.mark.parametrize("assign", list(ASSIGN))
@pytest.mark.parametrize("op", ["and", "or"])
def test_rule_equals_the_oracle(op, assign, kind, within, conds):
    """Seeds 3 and 11. `and` with A among B, C is outside the device envelope (no mark, test_the_compilers_envelope); the
    rule is compared there all the same."""
    a, b, c = ASSIGN[assign]
    keys = keys_of(kind, a, b, c)
    for seed in (3, 11):
        sid, cols, ts = case(kind, seed)
        got = rule_tuples(op, a, b, c, sid, cols, ts, keys, within, conds)
        exp = oracle_tuples(logic_text(op, a, b, c, keys, within, conds), sid, cols, ts)
        if seed == 3 and conds == "gt_gt" and assign == "ABC" and (op, kind, within) in FLOORS:
            assert len(exp) >= 0.8 * FLOORS[(op, kind, within)], len(exp)
        np.testing.assert_array_equal(exp, got)


@pytest.mark.parametrize("kind", ["flat", "symbol", "per_stream"])
@pytest.mark.parametrize("op", ["and", "or"])
def test_heartbeats_and_the_output_timestamp(op, kind):
    """The output timestamp is the completing event's: the later member of `and`, the bound member of `or`."""
    a, b, c = ASSIGN["ABC"]
    keys = keys_of(kind, a, b, c)
    sid, cols, ts = case(kind, 3, 0.18)
    assert (sid == -1).sum() > 600
    for within in (5, 40):
        exp, ets = oracle_tuples(logic_text(op, a, b, c, keys, within), sid, cols, ts, with_ts=True)
        assert len(exp) >= some(op, keys is not None, within)
        np.testing.assert_array_equal(exp, rule_tuples(op, a, b, c, sid, cols, ts, keys, within))
        np.testing.assert_array_equal(ets, ts[exp[:, 1:].max(axis=1)])


@pytest.mark.parametrize("within", [5, 40])
@pytest.mark.parametrize("op", ["and", "or"])
def test_a_partition_that_also_keys_an_unread_stream(op, within):
    """`A -> e2=B and|or e3=A`: rows of C are keyed by the partition and not read by the query."""
    keys = keys_of("symbol", "A", "B", "A", also="C")
    sid, cols, ts = case("symbol", 3)
    exp = oracle_tuples(logic_text(op, "A", "B", "A", keys, within), sid, cols, ts)
    assert len(exp) >= some(op, True, within)
    np.testing.assert_array_equal(exp, rule_tuples(op, "A", "B", "A", sid, cols, ts, keys, within))


@pytest.mark.parametrize("seed", [3, 11])
def test_the_window_is_measured_from_e1_not_from_the_event_bound_last(seed):
    """Path 10 measures each hop from the event bound before; applied to `and` that gives other outputs."""
    for kind, within in (("flat", 5), ("symbol", 40)):
        keys = keys_of(kind, "A", "B", "C")
        sid, cols, ts = case(kind, seed)
        exp = oracle_tuples(logic_text("and", "A", "B", "C", keys, within), sid, cols, ts)
        got = rule_tuples("and", "A", "B", "C", sid, cols, ts, keys, within, from_last=True)
        assert len(exp) >= 30 and len(got) > len(exp) and not np.array_equal(exp, got)


@pytest.mark.parametrize("op", ["and", "or"])
def test_rule_does_not_hold_with_a_within_when_event_time_decreases(op):
    """Flat and keyed on decreasing event time: with a `within` the oracle's outputs are not the rule's (outside the
    device envelope: FAST_NON_MONOTONE, the NFA kernel takes the query over)."""
    sid, cols, ts = case("symbol", 3)
    ts = decreasing_ts(ts)
    for keys in (None, keys_of("symbol", "A", "B", "C")):
        exp = oracle_tuples(logic_text(op, "A", "B", "C", keys, 5), sid, cols, ts)
        got = rule_tuples(op, "A", "B", "C", sid, cols, ts, keys, 5)
        assert len(exp) >= some(op, keys is not None, 5) and not np.array_equal(exp, got)


def test_the_compilers_envelope():
    """(fast_pat_logic, fast_pat_nand, fast_absent, fast_pat_ms, fast_every_within, fast_seq_adjacent, fast_seq_k,
    fast_seq_ms, fast_pat_k) of the plan the compiler makes, match_arity and the hidden (e1, e2, e3) refs in the order of
    the query text; every text outside the new form keeps the marks of the parent commit."""
    from test_pat_logic_emu import marks_of, plan_of
    q = lambda body, sel="e1.timestamp as i": SCHEMA + f"@info(name='q') from {body} select {sel} insert into Out;"
    part = lambda with_, body: SCHEMA + f"partition with ({with_}) begin @info(name='q') from {body} " \
                                        "select e1.timestamp as i insert into Out; end;"
    mark = lambda v: (v, 0, 0, 0, 0, 0, 0, 0, 0)
    no = mark(0)
    for op, v in (("and", 1), ("or", 2)):
        for name, assign in ASSIGN.items():
            inside = op == "or" or name in ("ABC", "CAB")  # `and`: A is neither B nor C
            for kind in ("flat", "symbol", "per_stream"):
                for conds in CONDS:
                    assert marks_of(logic_text(op, *assign, keys_of(kind, *assign), 5, conds)) == (mark(v) if inside else no)
        assert marks_of(logic_text(op, "A", "B", "C", None, 0)) == mark(v)
        assert marks_of(q(f"every e1=A -> e2=B {op} e3=C within 1 sec")) == mark(v)
        assert marks_of(q(f"every e1=A[price>20] -> e2=B[price>e1.price] {op} e3=C[price<e1.price] within 1 sec",
                          "e1.price as p, e2.volume as v, e3.price as r, 7 as c")) == mark(v)
        assert marks_of(part("symbol of A, volume of B, symbol of C", f"every e1=A -> e2=B {op} e3=C within 1 sec")) == mark(v)
        # three words per match; three hidden refs (slot, index 0) in the order of the query text: e1 is slot 0, and the
        # lowering numbers the second operand's slot before the first one's
        arity, hidden = plan_of(logic_text(op, "A", "B", "C", None, 5))
        assert arity == 3 and len(hidden) == 3 and hidden[0] == (0, 0)
        assert sorted(s for s, _ in hidden[1:]) == [1, 2] and all(i == 0 for _, i in hidden)
        assert hidden[1][0] == 2 and hidden[2][0] == 1
        # out of scope: B = C, an operand reading the other, no within, a having, different schemas, a within elsewhere,
        # STRING and expression keys, a stream of the pattern without a key
        assert marks_of(q(f"every e1=A -> e2=B[price>45] {op} e3=B[price<=45] within 1 sec")) == no
        # (c3 reading e2 does not compile: the second operand is lowered first and cannot see the first; the other
        # direction compiles and stays unmarked)
        with pytest.raises(AssertionError, match="e2 not found"):
            marks_of(q(f"every e1=A -> e2=B[price>e1.price] {op} e3=C[price>e2.price] within 1 sec"))
        assert marks_of(q(f"every e1=A -> e2=B[price>e3.price] {op} e3=C[price>e1.price] within 1 sec")) == no
        assert marks_of(logic_text(op, "A", "B", "C", None, None)) == no
        assert marks_of(logic_text(op, "A", "B", "C", keys_of("symbol", "A", "B", "C"), None)) == no
        assert marks_of(q(f"every e1=A -> e2=B {op} e3=C within 1 sec", "e1.timestamp as i having i > 3")) == no
        assert marks_of(q(f"every e1=A within 5 milliseconds -> e2=B {op} e3=C within 1 sec")) == no
        assert marks_of(q(f"every (e1=A -> e2=B {op} e3=C within 1 sec) within 2 sec")) == no
        assert marks_of(q(f"every e1=A -> e2=B {op} e3=C within 1 sec -> e4=A")) == no
        assert marks_of(part("symbol + 1 of A, symbol of B, symbol of C", f"every e1=A -> e2=B {op} e3=C within 1 sec")) == no
        assert marks_of(part("symbol of A, symbol of C", f"every e1=A -> e2=B {op} e3=C within 1 sec")) == no
        named = "".join(f"define stream {s} (name string, price double, volume long, timestamp long); " for s in "ABC")
        assert marks_of(named + "partition with (name of A, name of B, name of C) begin @info(name='q') from every e1=A -> "
                        f"e2=B {op} e3=C within 1 sec select e1.timestamp as i insert into Out; end;") == no
        other = ("define stream A (symbol int, price double); define stream B (symbol int, price float); "
                 "define stream C (symbol int, price double); ")
        assert marks_of(other + f"@info(name='q') from every e1=A -> e2=B {op} e3=C within 1 sec select e1.price as p "
                        "insert into Out;") == no
    assert marks_of(q("every e1=A -> e2=A and e3=C within 1 sec")) == no   # `and` with A = B
    assert marks_of(q("every e1=A -> e2=B and e3=A within 1 sec")) == no   # `and` with A = C
    assert marks_of(q("every e1=A -> e2=A or e3=C within 1 sec")) == mark(2)
    assert marks_of(q("every e1=A -> e2=B or e3=A within 1 sec")) == mark(2)
    # the forms of paths 6-12 keep their marks
    pb = "@app:playback "
    assert marks_of(pb + q("every e1=A[price>20] -> not B[price>70] and e3=C[price>e1.price] within 1 sec")) == \
        (0, 1, 0, 0, 0, 0, 0, 0, 0)
    assert marks_of(pb + q("every e1=A[price>20] -> not B[price>70] for 1 sec")) == (0, 0, 1, 0, 0, 0, 0, 0, 0)
    assert marks_of(q("every e1=A[price>20] -> e2=B[price>e1.price] within 1 sec")) == (0, 0, 0, 1, 0, 0, 0, 0, 0)
    assert marks_of(q("every e1=A[price>20] -> e2=A[price>e1.price] within 1 sec")) == (0, 0, 0, 0, 1, 0, 0, 0, 0)
    assert marks_of(q("every e1=A[price>20], e2=A[price>e1.price]")) == (0, 0, 0, 0, 0, 1, 0, 0, 0)
    assert marks_of(q("every e1=A, e2=A, e3=A")) == (0, 0, 0, 0, 0, 0, 3, 0, 0)
    assert marks_of(q("every e1=A, e2=B")) == (0, 0, 0, 0, 0, 0, 0, 2, 0)
    assert marks_of(q("every e1=A -> e2=B within 1 sec -> e3=A within 1 sec")) == (0, 0, 0, 0, 0, 0, 0, 0, 3)
