"""The closed form of the k-state pattern over several streams, `every e1=S1[c1] -> e2=S2[c2] within T2 -> ... ->
ek=Sk[ck] within Tk` (3 <= k <= 8, streams of one schema, S1 none of S2 .. S(k-1)), on interleaved device batches
(sm_app_process_device_events, fast_path 10: kernels/seqpath.hip fast_pat_k, mpatk_dev.h) against the CPU oracle fed the
same events. Every S1 event passing c1 binds, state by state, the first later Sm event of its partition instance that
passes cm, inside Tm of the event bound before; one ek may complete many partials and one e2 may be shared by many; the
product carries the open partials and the events they hold across batches. Every case compares the (e1, ..., ek)
ordinals of the whole stream, tuple for tuple and in order, and the delivered events with the oracle's, checks the path
taken, and asserts a floor of expected outputs that the oracle alone reaches (tests/test_mpatk_plan.py has the counts).
Inputs: 20 000 events or fewer."""
import ctypes
import struct

import numpy as np
import pytest

from test_device_mseq import (NAMES, Run, events, oracle_on_read_rows, oracle_out, run, send_rows, straddling, tuples_of,
                              unread_rows_going_back)
from test_mseq_plan import per_stream_cols, stream

pytestmark = pytest.mark.gpu

CMS = {"gt": "price > {p}.price", "compound": "price > {p}.price - 25.0 and volume != e1.volume", "const": "price > 45"}
ABC, ABA, BCAB = list("ABC"), list("ABA"), list("BCAB")
CHAIN8 = list("ABCBBCBA")
SRC = {"symbol": {"A": "symbol", "B": "symbol", "C": "symbol"}, "per_stream": {"A": "symbol", "B": "volume", "C": "symbol"}}


def text(pattern, kind="flat", withins=40, cm="compound", select=None, kt="int", c1="[price>20]"):
    """withins: T in ms on every hop, or {m: T} (an element left out has none: outside the envelope)."""
    k = len(pattern)
    w = {m: withins for m in range(2, k + 1)} if isinstance(withins, int) else withins
    schema = "".join(f"define stream {s} (symbol {kt}, price double, volume long, timestamp long); " for s in NAMES)
    els = [f"every e1={pattern[0]}{c1}"]
    for m in range(2, k + 1):
        wt = f" within {w[m]} milliseconds" if m in w else ""
        els.append(f"e{m}={pattern[m - 1]}[{CMS[cm].format(p=f'e{m - 1}')}]{wt}")
    sel = select or "select " + ", ".join(f"e{m}.timestamp as i{m}" for m in range(1, k + 1))
    q = f"@info(name='q') from {' -> '.join(els)} {sel} insert into OutputStream;"
    if kind == "flat":
        return schema + q
    keys = {s: SRC[kind][s] for s in sorted(set(pattern))}
    return schema + "partition with (" + ", ".join(f"{x} of {s}" for s, x in keys.items()) + f") begin {q} end;"


def check(t, sid, cols, ts, ranges, k, floor=1, ords=None, exp_out=None, **options):
    """The product over the pieces against the oracle: tuples, delivered events, path 10 and no NFA state."""
    exp_out = exp_out or oracle_out(t, sid, cols, ts, ords)
    exp = tuples_of(exp_out, k)
    assert len(exp) >= floor
    got, out, paths, state = run(t, sid, cols, ts, ranges, ords=ords, **options)
    assert set(paths) == {10} and state == 0
    np.testing.assert_array_equal(got, exp)
    assert out == exp_out  # values, timestamps, visible refs and order of the delivered events
    return exp


def pieces(n, cuts):
    cuts = sorted(c for c in set(cuts) if 0 < c < n)
    return list(zip([0] + cuts, cuts + [n]))


RAGGED = (1, 1023, 1025, 2049, 3333)


# ---- 1. the grid of tests/test_mpatk_plan.py

def grid():
    out = []
    for shape in (ABC, ABA, BCAB):
        k = len(shape)
        w59 = {m: (5 if m == 2 else 9) for m in range(2, k + 1)}
        for kind in ("flat", "symbol", "per_stream"):
            cm = "gt" if kind == "per_stream" else "compound"
            for wname, w in (("40", 40), ("5_9", w59)) + ((("2", 2),) if kind == "flat" else ()):
                out.append(pytest.param(shape, kind, w, cm, id=f"{''.join(shape)}-{kind}-{wname}-{cm}"))
    out += [pytest.param(ABC, "symbol", 40, "gt", id="ABC-symbol-40-gt"),
            pytest.param(ABC, "symbol", 40, "const", id="ABC-symbol-40-const"),
            pytest.param(ABC, "flat", 2, "gt", id="ABC-flat-2-gt"),
            pytest.param(BCAB, "flat", 5, "compound", id="BCAB-flat-5-compound"),
            pytest.param(BCAB, "flat", 40, "gt", id="BCAB-flat-40-gt")]
    return out


# the smaller of the two seeds' counts (tests/test_mpatk_plan.py asserts them on the CPU)
FLOORS = {("ABC", "symbol", 40, "gt"): 141, ("ABC", "symbol", 40, "compound"): 643, ("ABC", "symbol", 40, "const"): 169,
          ("ABC", "symbol", "5_9", "compound"): 72, ("ABC", "flat", 2, "gt"): 31, ("ABC", "flat", 2, "compound"): 176,
          ("BCAB", "flat", 5, "compound"): 308, ("BCAB", "flat", 40, "gt"): 310}


@pytest.mark.parametrize("shape,kind,w,cm", grid())
def test_one_batch_and_ragged_pieces(shape, kind, w, cm):
    k = len(shape)
    t = text(shape, kind, w, cm)
    floor = FLOORS.get(("".join(shape), kind, w if isinstance(w, int) else "5_9", cm), 1)
    for seed in (3, 11):
        sid, cols, ts = stream(4000, seed=seed)
        if kind == "per_stream":
            cols = per_stream_cols(cols)
        n = len(ts)
        exp_out = oracle_out(t, sid, cols, ts)
        exp = check(t, sid, cols, ts, [(0, n)], k, floor, exp_out=exp_out)
        extra = []
        if floor >= 141 and kind == "symbol":  # also a cut between e2 and e3 of an expected tuple, and of several with one e2
            far = exp[exp[:, 2] - exp[:, 1] > 1]
            extra.append(int(far[len(far) // 2, 2]))
            if cm == "const":
                e2s, cnt = np.unique(far[:, 1], return_counts=True)
                extra.append(int(far[far[:, 1] == e2s[np.argmax(cnt)]][:, 2].min()))
        ranges = pieces(n, RAGGED + tuple(extra))
        check(t, sid, cols, ts, ranges, k, floor, exp_out=exp_out)
        if extra:  # partials carried with one and with two bound events, and a carried e2 that several share
            los = np.array([lo for lo, _ in ranges[1:]])
            piece = np.searchsorted(los, exp, side="right")
            assert (piece[:, 0] != piece[:, 1]).any() and (piece[:, 1] != piece[:, -1]).any()
            if cm == "const":
                late = exp[piece[:, 1] != piece[:, -1]]
                assert np.unique(late[:, 1], return_counts=True)[1].max() >= 2


@pytest.mark.parametrize("kind", ["symbol", "flat"])
def test_eight_states_in_pieces_of_257(kind):
    sid, cols, ts = stream(6000, seed=15, pattern=CHAIN8)
    n = len(ts)
    exp = check(text(CHAIN8, kind), sid, cols, ts, pieces(n, range(257, n, 257)), 8, 1000)
    assert straddling(exp, pieces(n, range(257, n, 257))) >= 100


# ---- 2. rows that must be ignored

@pytest.mark.parametrize("kind", ["symbol", "flat"])
def test_heartbeats_and_unread_rows_between_members(kind):
    sid, cols, ts = events(K=50 if kind == "symbol" else 1, heartbeats=0.3)
    t = text(ABA, kind, 150 if kind == "symbol" else 10, "gt")
    n = len(ts)
    exp = check(t, sid, cols, ts, pieces(n, (5000, 5001, 11111)), 3, 30)
    gaps = [sid[a + 1:b] for a, b, _ in exp] + [sid[b + 1:c] for _, b, c in exp]
    assert any((x == -1).any() for x in gaps) and any((x == 2).any() for x in gaps)


@pytest.mark.parametrize("kind", ["symbol", "flat"])
def test_unread_rows_going_back_in_time_between_e1_and_e2(kind):
    """Three batches: 1025 rows of A that leave open partials, 65 rows of C and heartbeats whose event times decrease and
    lie before the first batch's, and 1025 rows of B and A in time order. The batch without a read row neither reports
    decreasing time nor moves the carried time: every batch stays on the closed form."""
    n1 = 1025
    rng = np.random.default_rng(23)
    a_sid = np.zeros(n1, np.int32)
    a_sid[::16] = -1
    step = np.arange(n1, dtype=np.int64) // 16
    sid = np.concatenate([a_sid, rng.integers(0, 2, n1).astype(np.int32)])
    sym = rng.integers(0, 5 if kind == "symbol" else 1, 2 * n1).astype(np.int32)
    price = np.concatenate([21.0 + np.round(rng.random(n1) * 19.0, 1), 30.0 + np.round(rng.random(n1) * 60.0, 1)])
    vol = rng.integers(0, 2000, 2 * n1).astype(np.int64)
    ts = 1000 + np.concatenate([step, step[-1] + step])
    sid, cols, ts = unread_rows_going_back(sid, (sym, price, vol), ts, n1)
    ranges = [(0, n1), (n1, n1 + 65), (n1 + 65, len(ts))]
    assert (np.diff(ts[n1:n1 + 65]) < 0).all() and ts[n1] < ts[0] and not np.isin(sid[n1:n1 + 65], [0, 1]).any()
    t = text(ABA, kind, 150, "gt")
    exp_out = oracle_on_read_rows(t, sid, cols, ts, [0, 1])
    exp = check(t, sid, cols, ts, ranges, 3, 100, exp_out=exp_out)
    assert straddling(exp, ranges) >= 100


# ---- 3. long scans, a hot key

def scan_stream():
    """One key per scan: its e2 lies L1 sorted positions behind its e1 and its e3 L2 positions behind that, for L1 and
    L2 at, below and above the lane's own budget (16 positions), a wave step (64) behind it, and 200."""
    ends = (15, 16, 17, 79, 80, 81, 200)
    parts = []
    for L1 in ends:
        for L2 in ends:
            n = 1 + L1 + L2 + 3
            sid = np.ones(n, np.int32)
            sid[2:L1:5] = 0
            sid[0] = 0
            price = np.full(n, 10.0)
            price[0] = 30.0
            sid[L1], price[L1] = 1, 40.0
            sid[L1 + 1:L1 + L2] = 0
            sid[L1 + 3:L1 + L2:7] = 1
            sid[L1 + L2], price[L1 + L2] = 0, 50.0
            price[L1 + L2 + 1:] = 55.0
            parts.append((sid, np.full(n, len(parts), np.int32), price))
    sid, sym, price = (np.concatenate([p[i] for p in parts]) for i in range(3))
    n = len(sid)
    return sid, (sym, price, np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)), np.arange(n, dtype=np.int64) // 500


def test_state_changes_inside_the_budget_at_its_edge_and_inside_a_wave_step():
    sid, cols, ts = scan_stream()
    n = len(ts)
    t = text(ABA, "symbol", 150, "gt")
    exp = check(t, sid, cols, ts, [(0, n)], 3, 49)
    d1, d2 = exp[:, 1] - exp[:, 0], exp[:, 2] - exp[:, 1]
    assert {(a, b) for a, b in zip(d1.tolist(), d2.tolist())} >= {(a, b) for a in (15, 16, 17, 79, 80, 81, 200)
                                                                  for b in (15, 16, 17, 79, 80, 81, 200)}
    check(t, sid, cols, ts, pieces(n, (n // 3, n // 2, n // 2 + 100)), 3, 49)
    # unkeyed: one scan at a time
    for lo in (0, n // 2):
        one = slice(lo, lo + 700)
        c = tuple(x[one] for x in cols[:3]) + (np.arange(700, dtype=np.int64),)
        check(text(ABA, "flat", 150, "gt"), sid[one], c, ts[one], [(0, 300), (300, 700)], 3, 1)


@pytest.mark.parametrize("kind", ["symbol", "flat"])
def test_one_e3_completes_3000_carried_and_batch_partials_through_two_e2s(kind):
    n = 4400
    sid = np.zeros(n, np.int32)
    sid[5::10] = 2
    sid[8::10] = -1
    sym = np.full(n, 7, np.int32)
    price = np.full(n, 30.0)
    sid[1500], price[1500] = 1, 40.0   # e2 of the partials before it
    sid[4200], price[4200] = 1, 41.0   # e2 of those behind row 1500
    sid[4300], price[4300] = 0, 50.0   # e3 of them all
    sym[4350:4380] = 3
    cols = (sym, price, np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64))
    ts = np.arange(n, dtype=np.int64) // 50
    t = text(ABA, kind, 150, "gt")
    exp = check(t, sid, cols, ts, [(0, 2000), (2000, n)], 3, 3000)
    one = exp[exp[:, 2] == 4300]
    assert len(one) >= 3000 and (one[:, 1] == 1500).sum() >= 1000 and (one[:, 1] == 4200).sum() >= 1000
    assert (one[:, 0] < 2000).sum() >= 1000 and (one[:, 0] >= 2000).sum() >= 1000


# ---- 4. keys and ordinals

@pytest.mark.parametrize("remap", ["auto", "off", "on"])
def test_long_keys_negative_and_wide(remap):
    sid, cols, ts = stream(4000, seed=3, K=40)
    sym = (cols[0].astype(np.int64) - 20) * 3_000_011
    assert sym.min() < 0 and sym.max() - sym.min() > 1 << 20
    cols = [sym, cols[1], cols[2], cols[3]]
    opts = {} if remap == "auto" else {"key_remap": 1 if remap == "on" else 0}
    check(text(ABC, "symbol", 400, "compound", kt="long"), sid, cols, ts, pieces(len(ts), (1000, 2500)), 3, 30, **opts)


@pytest.mark.parametrize("kind", ["symbol", "flat"])
def test_given_ordinals_with_gaps(kind):
    sid, cols, ts = stream(4000, seed=3)
    ords = 3 * np.arange(len(ts), dtype=np.int64) + 1
    exp = check(text(ABC, kind, 40 if kind == "symbol" else 2), sid, cols, ts, pieces(len(ts), (1000, 2500)), 3, 30,
                ords=ords)
    assert (exp % 3 == 1).all()


# ---- 5. snapshot

@pytest.mark.parametrize("kind", ["symbol", "flat"])
def test_snapshot_restore_between_e2_and_e3(kind):
    sid, cols, ts = stream(4000, seed=3)
    t = text(ABC, kind, 40 if kind == "symbol" else 2)
    exp_out = oracle_out(t, sid, cols, ts)
    exp = tuples_of(exp_out, 3)
    far = exp[exp[:, 2] - exp[:, 1] > 1]
    cut = int(far[len(far) // 2, 2])
    assert ((exp[:, 1] < cut) & (exp[:, 2] >= cut)).sum() >= 1 and len(exp) >= 30
    a = Run(t)
    first = a.piece(sid, cols, ts, 0, cut)
    snap = a.app.snapshot()
    out_a = a.app.outputs()
    a.app.close()
    b = Run(t)
    b.app.restore(snap)
    second = b.piece(sid, cols, ts, cut, len(ts))
    out_b = b.app.outputs()
    b.app.close()
    assert a.paths == [10] and b.paths == [10]
    np.testing.assert_array_equal(np.concatenate([first, second]), exp)
    rows = lambda o: o["streams"].get("OutputStream", [])
    assert rows(out_a) + rows(out_b) == rows(exp_out)  # the delivered events, e1 and e2 projected from the restored carry


# ---- 6. hand-over to the NFA kernel

@pytest.mark.parametrize("case_", ["inside", "before_carry"])
@pytest.mark.parametrize("kind", ["symbol", "flat"])
def test_decreasing_time_hands_over(case_, kind):
    """Event time decreases inside the second piece, or from the first piece to the second: FAST_NON_MONOTONE, the NFA
    kernel takes the query over for good with the carried partials' events. The windows are longer than the stream, so
    that no partial was dropped as expired before the hand-over."""
    sid, cols, ts = stream(4000, seed=3, K=5 if kind == "symbol" else 1)
    ts = ts.copy()
    if case_ == "inside":
        ts[1800:1900] = ts[1800:1900][::-1]
    else:
        ts[1600:] -= 50
    assert (np.diff(ts) < 0).any()
    ranges = [(0, 1600), (1600, 2800), (2800, 4000)]
    t = text(ABC, kind, 30000, "gt")
    exp_out = oracle_out(t, sid, cols, ts)
    exp = tuples_of(exp_out, 3)
    assert len(exp) >= 30 and straddling(exp, ranges) >= 2
    got, out, paths, state = run(t, sid, cols, ts, ranges)
    assert paths == [10, 5, 5] and state == 1
    np.testing.assert_array_equal(got, exp)
    assert out == exp_out


@pytest.mark.parametrize("kind", ["symbol", "flat"])
def test_staged_sends_before_and_after_device_events(kind):
    sid, cols, ts = stream(4000, seed=3)
    t = text(ABC, kind, 40 if kind == "symbol" else 5)
    exp_out = oracle_out(t, sid, cols, ts)
    exp = tuples_of(exp_out, 3)
    n = len(ts)
    assert len(exp) >= 30
    # staged, then device: the NFA kernel holds the state
    r = Run(t)
    send_rows(r.app, sid, cols, ts, 0, 40)
    tail = r.piece(sid, cols, ts, 40, n)
    assert r.paths == [5] and r.app.get_stat("match_arity:q") == 3
    _, out, state = r.finish()
    assert state == 1 and out == exp_out
    np.testing.assert_array_equal(tail, exp[exp[:, 2] >= 40])
    # device, staged, device: the flush replays the carried events into the NFA, which keeps the query
    a = next(int(e3) for e1, e2, e3 in exp[len(exp) // 2:] if e3 - e2 > 1)  # between a tuple's e2 and e3
    b = a + 40
    assert ((exp[:, 1] < a) & (exp[:, 2] >= a)).any()  # a handed-over partial with two bound events completes
    r = Run(t)
    first = r.piece(sid, cols, ts, 0, a)
    assert r.paths == [10] and r.app.get_stat("nfa_state:q") == 0
    send_rows(r.app, sid, cols, ts, a, b)
    r.app.flush()
    assert r.app.get_stat("nfa_state:q") == 1
    last = r.piece(sid, cols, ts, b, n)
    assert r.paths == [10, 5]
    _, out, state = r.finish()
    assert state == 1 and out == exp_out
    np.testing.assert_array_equal(first, exp[exp[:, 2] < a])
    np.testing.assert_array_equal(last, exp[exp[:, 2] >= b])


def feed_pieces(app_text, sid, cols, ts, ranges, **options):
    r = Run(app_text, **options)
    paths = []
    for lo, hi in ranges:
        up = lambda a: r.torch.from_numpy(np.ascontiguousarray(a[lo:hi])).to(r.dev)
        r.app.process_device_events(up(sid), up(ts), [up(c) for c in cols], ordinal_base=lo)
        paths.append(int(r.app.get_stat("fast_path:q")))
    out = r.app.outputs()
    # the NFA route's heap statistics, as the parent commit gives them for these inputs: the first pool, nothing in it
    pool = [r.app.get_stat(f"{k}:q") for k in ("pool_words", "pool_used", "pool_compactions", "pool_refused")]
    assert pool == [1124096, 0, 0, 0], pool
    r.app.close()
    return out, paths


def test_keep_outputs_a_second_query_and_a_missing_within_stay_on_the_nfa_route():
    sid, cols, ts = stream(4000, seed=3)
    ranges = [(0, 1500), (1500, 4000)]
    t = text(ABC, "symbol", 40)
    exp_out = oracle_out(t, sid, cols, ts)
    assert len(exp_out["streams"]["OutputStream"]) >= 30
    out, paths = feed_pieces(t, sid, cols, ts, ranges, keep_outputs=1)
    assert 10 not in paths and out == exp_out
    two = t.replace(" end;", " @info(name='q2') from every e1=B[price>30] -> e2=A[price>e1.price] within 40 milliseconds "
                             "select e1.timestamp as i1, e2.timestamp as i2 insert into Out2; end;")
    exp_two = oracle_out(two, sid, cols, ts)
    assert len(exp_two["streams"]["Out2"]) >= 30
    out, paths = feed_pieces(two, sid, cols, ts, ranges)
    assert 10 not in paths and out == exp_two
    nw = text(ABC, "symbol", {3: 40})
    exp_nw = oracle_out(nw, sid, cols, ts)
    assert len(exp_nw["streams"]["OutputStream"]) >= 30
    out, paths = feed_pieces(nw, sid, cols, ts, ranges)
    assert 10 not in paths and paths[0] == paths[1] and out == exp_nw


# ---- 7. outputs and stats

PSELECT = ("select e1.symbol as k, e1.price as p1, e2.price as p2, e3.volume - e1.volume as dv, "
           "e1.timestamp as i1, e2.timestamp as i2, e3.timestamp as i3")
PKINDS = ["i", "d", "d", "i", "i", "i", "i"]


def words(row):
    return [struct.unpack("<q", struct.pack("<d", v))[0] if k == "d" else int(v) for v, k in zip(row, PKINDS)]


@pytest.mark.parametrize("kind", ["symbol", "flat"])
def test_device_project_equals_oracle(kind):
    sid, cols, ts = stream(4000, seed=3)
    t = text(ABC, kind, 40 if kind == "symbol" else 2, select=PSELECT)
    rows = oracle_out(t, sid, cols, ts)["streams"]["OutputStream"]
    tup = np.array([r[1][4:7] for r in rows], dtype=np.int64)
    assert len(tup) >= 30
    ranges = pieces(len(ts), RAGGED)
    los = np.array([lo for lo, _ in ranges[1:]])
    piece = np.searchsorted(los, tup, side="right")
    assert (piece[:, 1] != piece[:, 2]).any()  # e1 and e2 read from the carry
    r = Run(t)
    got = []
    for lo, hi in ranges:
        r.piece(sid, cols, ts, lo, hi)
        assert r.app.get_stat("match_arity:q") == 3
        vals, nulls, ots = r.app.device_project("q")
        r.torch.cuda.synchronize()
        assert not nulls.any()
        got += [[t_, v] for t_, v in zip(ots.cpu().tolist(), vals.cpu().tolist())]
    assert set(r.paths) == {10}
    r.app.close()
    assert got == [[row[0], words(row[1])] for row in rows]


def test_callbacks_receive_the_oracles_events():
    """A StreamCallback and a columns callback through SiddhiAppRuntime.sendDeviceEvents: one call per ek, in order of
    it, before the call returns."""
    import torch
    import siddhi_amd
    from siddhi_amd import ColumnsStreamCallback, SiddhiManager, StreamCallback
    sid, cols, ts = stream(4000, seed=3)
    t = text(ABC, "symbol", 40, "const", select=PSELECT)
    rows = oracle_out(t, sid, cols, ts)["streams"]["OutputStream"]
    assert len(rows) >= 100
    tup = np.array([r[1][4:7] for r in rows], dtype=np.int64)
    ranges = pieces(len(ts), RAGGED)
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
            assert v.value == 10
            seen.append(sum(len(c) for c in evs) + sum(len(c[0]) for c in columns))
        rt.shutdown()
    flat_evs = [e for chunk in evs for e in chunk]
    assert flat_evs == [[r[0], r[1]] for r in rows]
    assert [len(c) for c in evs] == np.unique(tup[:, 2], return_counts=True)[1].tolist()  # one chunk per ek
    assert max(len(c) for c in evs) >= 2
    assert [w for c in columns for w in c[1]] == [words(r[1]) for r in rows]
    assert [x for c in columns for x in c[0]] == [r[0] for r in rows]
    assert seen[0] == int((tup[:, 2] < ranges[0][1]).sum())  # delivered before the call returned


def test_match_arity_and_timing_labels():
    sid, cols, ts = stream(4000, seed=3)
    n = len(ts)
    for pattern in (ABC, BCAB):
        r = Run(text(pattern, "symbol"), fast_timing=1)
        assert r.app.get_stat("match_arity:q") == len(pattern)
        r.piece(sid, cols, ts, 0, n // 2)
        for label in ["mpatk_facts", "mpatk_pack", "mpatk_sort", "mpatk_link", "mpatk_count", "mpatk_scan", "mpatk_cand",
                      "mpatk_emit", "mpatk_order", "mpatk_parts", "mpatk_carry"]:
            assert r.app.get_stat(f"kernel_calls:{label}") == 1, label
            assert r.app.get_stat(f"kernel_ms:{label}") >= 0
        assert r.app.get_stat("kernel_calls:mpat_link") == 0
        r.piece(sid, cols, ts, n // 2, n)
        assert r.paths == [10, 10]
        r.app.close()
