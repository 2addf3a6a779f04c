"""The closed form of the logical absent `every e1=A[c1] -> not B[c2] and e3=C[c3] within T` (either operand order,
streams of one schema) on interleaved device batches (sm_app_process_device_events, fast_path 12: kernels/seqpath.hip
fast_pat_nand, mpat_nand_dev.h) against the CPU oracle fed the same events. Every A row passing c1 waits for the first
later C row of its partition instance that passes c3; the pair comes out iff that row lies inside T and no B row of the
instance passing c2 came in between; the product carries the open partials' e1 rows across batches. Every case compares
the (e1, e3) ordinals of the whole stream, pair for pair and in order, with the oracle's, checks the path taken, and
asserts a floor of expected outputs that the oracle alone reaches. Inputs: 4000 rows (4400 for the hot key), 3 streams
and heartbeat rows, 20 keys or fewer."""
import ctypes
import struct

import numpy as np
import pytest

from test_device_mseq import NAMES, Run, events, oracle_out, run, send_rows, straddling, tuples_of

pytestmark = pytest.mark.gpu

C3 = "price > e1.price"
T_KEYED, T_FLAT = 60, 10  # ms: a few rows of a key out of 20, about ten rows of the flat stream
N = 4000


def text(a="A", b="B", c="C", keys=None, within=T_KEYED, c3=C3, select=None, kt="int", c1="[price>20]", c2="[price>45]",
         mirrored=False):
    schema = "".join(f"define stream {s} (symbol {kt}, price double, volume long, timestamp long); " for s in NAMES)
    w = "" if within is None else f" within {within} milliseconds"
    sel = select or "select e1.timestamp as i1, e3.timestamp as i3"
    nb, ec = f"not {b}{c2}", f"e3={c}[{c3}]"
    logical = f"{ec} and {nb}" if mirrored else f"{nb} and {ec}"
    q = f"@info(name='q') from every e1={a}{c1} -> {logical}{w} {sel} insert into OutputStream;"
    head = "@app:playback " + schema
    if keys is None:
        return head + q
    return head + "partition with (" + ", ".join(f"{x} of {s}" for s, x in keys.items()) + f") begin {q} end;"


BY_SYMBOL = {"A": "symbol", "B": "symbol", "C": "symbol"}
PER_STREAM = {"A": "symbol", "B": "volume", "C": "symbol"}


def case(kind, K=20, n=N, **kw):
    """(text, sid, cols, ts) of a form: flat, keyed by symbol, or B keyed by its volume."""
    if kind == "flat":
        sid, cols, ts = events(n=n, K=1)
        return text(keys=None, **dict({"within": T_FLAT}, **kw)), sid, cols, ts
    sid, cols, ts = events(n=n, K=K)
    if kind == "per_stream":
        cols = (cols[0], cols[1], cols[2] % K, cols[3])
        return text(keys=PER_STREAM, **kw), sid, cols, ts
    return text(keys=BY_SYMBOL, **kw), sid, cols, ts


def cuts_inside_pairs(exp, n, extra=()):
    """Pieces cut between e1 and e3 of expected pairs (one in each quarter of the stream), plus `extra` cuts."""
    far = exp[exp[:, 1] - exp[:, 0] > 1]
    cuts = {int(far[len(far) // 4, 1]), int(far[len(far) // 2, 1]), int(far[3 * len(far) // 4, 1])} | set(extra)
    cuts = sorted(c for c in cuts if 0 < c < n)
    return list(zip([0] + cuts, cuts + [n]))


def check(t, sid, cols, ts, ranges, floor=30, ords=None, **options):
    exp_out = oracle_out(t, sid, cols, ts, ords)
    exp = tuples_of(exp_out, 2)
    assert len(exp) >= floor, len(exp)
    got, out, paths, state = run(t, sid, cols, ts, ranges, ords=ords, **options)
    assert set(paths) == {12} and state == 0
    np.testing.assert_array_equal(got, exp)
    assert out == exp_out  # values, timestamps, visible refs and order of the delivered events
    return exp


# ---- 1. batches

@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("kind", ["flat", "symbol", "per_stream"])
def test_one_batch_and_ragged_pieces(kind, mirrored):
    """`fast_path:q` is 12 with `nfa_state` 0. One batch; then pieces of 1, 1023 and 1025 rows and cuts between an
    expected pair's e1 and e3."""
    t, sid, cols, ts = case(kind, mirrored=mirrored)
    n = len(ts)
    exp = check(t, sid, cols, ts, [(0, n)])
    inside = [lo for lo, _ in cuts_inside_pairs(exp[exp[:, 1] > 2049], n)[1:]]
    cuts = [1, 1024, 2049] + inside
    ranges = list(zip([0] + cuts, cuts + [n]))
    assert {hi - lo for lo, hi in ranges} >= {1, 1023, 1025} and len(inside) >= 2 and straddling(exp, ranges) >= 3
    check(t, sid, cols, ts, ranges)


@pytest.mark.parametrize("keyed", [True, False])
def test_pieces_of_1_and_37_rows(keyed):
    t, sid, cols, ts = case("symbol" if keyed else "flat", K=5)
    n = len(ts)
    ranges = [(lo, min(lo + 37, 1850)) for lo in range(0, 1850, 37)] + [(lo, lo + 1) for lo in range(1850, 2050)] + [(2050, n)]
    exp = check(t, sid, cols, ts, ranges)
    assert straddling(exp, ranges) >= 20


def cancelled_triples(sid, cols, ts, keyed, within):
    """(i, b, j) of partials that a cancelling row b kills in front of the C row j that would have matched inside T."""
    sym, price = cols[0], cols[1]
    out = []
    for i in np.nonzero((sid == 0) & (price > 20))[0]:
        mine = (np.arange(len(sid)) > i) & ((sym == sym[i]) if keyed else True)
        js = np.nonzero(mine & (sid == 2) & (price > price[i]))[0]
        bs = np.nonzero(mine & (sid == 1) & (price > 45))[0]
        if len(js) and len(bs) and bs[0] < js[0] and ts[js[0]] - ts[i] <= within:
            out.append((int(i), int(bs[0]), int(js[0])))
    return out


@pytest.mark.parametrize("keyed", [True, False])
def test_cuts_between_an_e1_its_cancelling_row_and_the_c_row_that_would_have_matched(keyed):
    """A piece starts at the cancelling row (the carried partial meets it first; keyed it is the head of its key's run)
    and another at the C row behind it: the dead partial is not carried there."""
    t, sid, cols, ts = case("symbol" if keyed else "flat")
    tr = cancelled_triples(sid, cols, ts, keyed, T_KEYED if keyed else T_FLAT)
    assert len(tr) >= 10
    cuts = set()
    for i, b, j in (tr[len(tr) // 4], tr[len(tr) // 2], tr[3 * len(tr) // 4]):
        cuts |= {b, j}
    cuts = sorted(cuts)
    exp = check(t, sid, cols, ts, list(zip([0] + cuts, cuts + [len(ts)])))
    assert not {(i, j) for i, _, j in tr} & {tuple(p) for p in exp.tolist()}


# ---- 2. long scans and a hot key

@pytest.mark.parametrize("keyed", [True, False])
def test_scans_longer_than_the_private_budget_and_a_wave_step_with_the_bound_inside(keyed):
    """Partials whose e3 lies 97 .. 1500 sorted positions ahead (the lane's own budget is 16 positions, a wave step 64)
    among C rows that fail c3 and B rows that fail c2; three of them have their cancelling row inside the scan, one of
    these one position in front of the e3."""
    n = 4000
    rng = np.random.default_rng(17)
    sid = np.where(rng.random(n) < 0.5, 2, 1).astype(np.int32)
    sym = np.full(n, 3, np.int32)
    price = np.full(n, 10.0)
    sid[rng.random(n) < 0.1] = -1
    starts = [0, 100, 300, 1200, 1400, 2400]
    dist = [97, 98, 161, 130, 1090, 1500]
    bound = [None, 40, None, 129, 700, None]  # positions past the e1
    for k, (s, d, b) in enumerate(zip(starts, dist, bound)):  # the k-th e3 passes c3 for its e1 and fails for the later ones
        sid[s], price[s] = 0, 50.0 + k
        sid[s + d], price[s + d] = 2, 50.5 + k
        if b is not None:
            sid[s + b], price[s + b] = 1, 46.0
    cols = (sym, price, np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64))
    ts = np.arange(n, dtype=np.int64) // 100
    t = text(keys=BY_SYMBOL if keyed else None, c1="[price>35]", within=100)
    exp = check(t, sid, cols, ts, [(0, n)], floor=3)
    assert sorted((exp[:, 1] - exp[:, 0]).tolist()) == [97, 161, 1500]
    check(t, sid, cols, ts, [(0, 1250), (1250, 2000), (2000, n)], floor=3)  # carried partials scan far too


def hot_key_stream():
    """3440 A rows of key 7 (heartbeats and rows of another key between them), a cancelling B row of key 7 behind the
    first third of them, then one C row of key 7 that completes all the others."""
    n = 4400
    sid = np.zeros(n, np.int32)
    sid[5::10] = -1
    sym = np.full(n, 7, np.int32)
    sym[8::10] = 3
    price = np.full(n, 30.0)
    sid[1433], price[1433] = 1, 50.0
    sid[4300], price[4300] = 2, 50.0
    sid[4390], price[4390] = 2, 25.0  # fails c3 for the partials behind row 4300
    return sid, (sym, price, np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)), np.arange(n, dtype=np.int64) // 50


@pytest.mark.parametrize("keyed", [True, False])
def test_one_e3_completes_3000_carried_and_batch_partials_a_third_of_them_cancelled(keyed):
    sid, cols, ts = hot_key_stream()
    t = text(keys=BY_SYMBOL if keyed else None, within=200)
    ranges = [(0, 2500), (2500, len(ts))]
    exp = check(t, sid, cols, ts, ranges, floor=2000)
    one = exp[exp[:, 1] == 4300]
    a_rows = int(((sid[:4300] == 0) & ((cols[0][:4300] == 7) | (not keyed))).sum())
    assert len(one) >= 2000 and a_rows - len(one) >= 1000  # the cancelled third
    assert (one[:, 0] < 2500).sum() >= 500 and (one[:, 0] >= 2500).sum() >= 1000 and one[:, 0].min() > 1433


# ---- 3. keys, ordinals, shared streams

@pytest.mark.parametrize("remap", ["auto", "off", "on"])
def test_long_keys_negative_and_wide(remap):
    sid, cols, ts = events(n=N, K=20)
    sym = (cols[0].astype(np.int64) - 10) * 3_000_011
    assert sym.min() < 0 and sym.max() - sym.min() > 1 << 20
    cols = (sym, cols[1], cols[2], cols[3])
    t = text(keys=BY_SYMBOL, kt="long")
    exp = tuples_of(oracle_out(t, sid, cols, ts), 2)
    opts = {} if remap == "auto" else {"key_remap": 1 if remap == "on" else 0}
    check(t, sid, cols, ts, cuts_inside_pairs(exp, len(ts)), **opts)


def test_negative_int_keys():
    sid, cols, ts = events(n=N, K=20)
    cols = (cols[0] - 10, cols[1], cols[2], cols[3])
    t = text(keys=BY_SYMBOL)
    exp = tuples_of(oracle_out(t, sid, cols, ts), 2)
    assert (cols[0][exp[:, 0]] < 0).any()
    check(t, sid, cols, ts, cuts_inside_pairs(exp, len(ts)))


@pytest.mark.parametrize("keyed", [True, False])
def test_given_ordinals_with_gaps(keyed):
    """Rows carrying the global ordinals 3 i + 1, each piece's first ordinal as its base."""
    t, sid, cols, ts = case("symbol" if keyed else "flat")
    ords = 3 * np.arange(len(ts), dtype=np.int64) + 1
    exp = tuples_of(oracle_out(t, sid, cols, ts, ords), 2)
    assert (exp % 3 == 1).all()
    check(t, sid, cols, ts, cuts_inside_pairs((exp - 1) // 3, len(ts)), ords=ords)


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("abc", [("A", "A", "C"), ("A", "B", "A"), ("C", "A", "B")])
def test_shared_streams_and_another_assignment(abc, keyed):
    """A = B: an e1 passing c2 cancels the earlier partials of its key. A = C: a row is an e3 and an e1 at once."""
    sid, cols, ts = events(n=N, K=20 if keyed else 1)
    t = text(*abc, keys={s: "symbol" for s in abc} if keyed else None, within=T_KEYED if keyed else T_FLAT)
    exp = tuples_of(oracle_out(t, sid, cols, ts), 2)
    check(t, sid, cols, ts, cuts_inside_pairs(exp, len(ts)))


# ---- 4. hand-over to the NFA kernel

def small(keyed):
    """3000 rows whose c1 leaves few partials open: unkeyed, the NFA kernel's one lane walks every one of them."""
    sid, cols, ts = events(n=3000, K=10 if keyed else 1, heartbeats=0.0)
    return sid, cols, ts, dict(keys=BY_SYMBOL if keyed else None, c1="[price>20]" if keyed else "[price>48]")


@pytest.mark.parametrize("case_", ["inside", "before_carry"])
@pytest.mark.parametrize("keyed", [True, False])
def test_decreasing_time_hands_over(case_, keyed):
    """Event time decreases inside the second piece, or from the first piece to the second: FAST_NON_MONOTONE, the NFA
    kernel takes the query over for good with the carried partials. The window is longer than the stream, so that no
    partial was dropped as expired before the hand-over (and the expected pairs do not depend on the event times). The
    pieces are cut in front of the e3 of two expected pairs."""
    sid, cols, ts, kw = small(keyed)
    t = text(within=30000, **kw)
    far = tuples_of(oracle_out(t, sid, cols, ts), 2)
    far = far[far[:, 1] - far[:, 0] > 1]
    c1 = int(far[len(far) // 3, 1])
    c2 = int(far[far[:, 1] > c1 + 300][0, 1])
    ranges = [(0, c1), (c1, c2), (c2, len(ts))]
    ts = ts.copy()
    if case_ == "inside":
        ts[c1 + 50:c1 + 250] = ts[c1 + 50:c1 + 250][::-1]
    else:
        ts[c1:] -= 50
    assert (np.diff(ts) < 0).any()
    exp_out = oracle_out(t, sid, cols, ts)
    exp = tuples_of(exp_out, 2)
    assert len(exp) >= 30 and straddling(exp, ranges) >= 2
    got, out, paths, state = run(t, sid, cols, ts, ranges)
    assert paths == [12, 5, 5] and state == 1
    np.testing.assert_array_equal(got, exp)
    assert out == exp_out


@pytest.mark.parametrize("keyed", [True, False])
def test_staged_sends_before_and_after_device_events(keyed):
    sid, cols, ts, kw = small(keyed)
    t = text(within=40 if keyed else T_FLAT, **kw)
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
    a = next(int(e3) for e1, e3 in exp[len(exp) // 2:] if e3 - e1 > 1)  # in front of a pair's e3
    b = a + 40
    assert ((exp[:, 0] < a) & (exp[:, 1] >= a) & (exp[:, 1] < b)).any()  # a handed-over partial completes
    r = Run(t)
    first = r.piece(sid, cols, ts, 0, a)
    assert r.paths == [12] and r.app.get_stat("nfa_state:q") == 0
    send_rows(r.app, sid, cols, ts, a, b)
    r.app.flush()
    assert r.app.get_stat("nfa_state:q") == 1
    last = r.piece(sid, cols, ts, b, n)
    assert r.paths == [12, 5]
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


STAY = {
    "keep_outputs": (dict(within=40), dict(keep_outputs=1)),
    "no_within": (dict(within=None), {}),
    "c2_reads_e1": (dict(within=40, c2="[price>e1.price + 20.0]"), {}),
    "b_is_c": (dict(within=40, b="B", c="B", c2="[price>45]", c3="price <= 45 and price > e1.price"), {}),
}


@pytest.mark.parametrize("which", list(STAY) + ["second_query"])
def test_texts_that_stay_on_the_nfa_route(which):
    """What ran on the NFA kernel before runs there as before, with the oracle's outputs. `fast_path:q` stays 0, as it
    does on the parent commit for each of these: an unmarked text and a second query never reach the closed-form branch
    of sm_app_process_device_events, and keep_outputs turns it off; the stat becomes 5 only where the NFA route leaves
    the only, marked query's matches in dev_pairs (the hand-over tests above)."""
    sid, cols, ts = events(n=3000, K=10, heartbeats=0.0)
    ranges = [(0, 1300), (1300, 3000)]
    if which == "second_query":
        t = text(keys=BY_SYMBOL, within=40).replace(
            " end;", " @info(name='q2') from every e1=B[price>30] -> e2=A[price>e1.price] within 40 milliseconds "
                     "select e1.timestamp as i1, e2.timestamp as i2 insert into Out2; end;")
        opts, stream = {}, "Out2"
    else:
        kw, opts = STAY[which]
        t, stream = text(keys={"A": "symbol", "B": "symbol"} if which == "b_is_c" else BY_SYMBOL, **kw), "OutputStream"
    exp_out = oracle_out(t, sid, cols, ts)
    assert len(exp_out["streams"][stream]) >= 30
    out, paths = feed_pieces(t, sid, cols, ts, ranges, **opts)
    assert paths == [0, 0] and out == exp_out


# ---- 5. snapshot

@pytest.mark.parametrize("keyed", [True, False])
def test_snapshot_restore_between_e1_and_e3(keyed):
    t, sid, cols, ts = case("symbol" if keyed else "flat")
    exp = tuples_of(oracle_out(t, sid, cols, ts), 2)
    cut = int(exp[exp[:, 1] - exp[:, 0] > 1][len(exp) // 4, 1])
    assert ((exp[:, 0] < cut) & (exp[:, 1] >= cut)).sum() >= 1 and len(exp) >= 30
    a = Run(t)
    first = a.piece(sid, cols, ts, 0, cut)
    snap = a.app.snapshot()
    a.app.close()
    b = Run(t)
    b.app.restore(snap)
    second = b.piece(sid, cols, ts, cut, len(ts))
    b.app.close()
    assert a.paths == [12] and b.paths == [12]
    np.testing.assert_array_equal(np.concatenate([first, second]), exp)


# ---- 6. outputs and stats

PSELECT = ("select e1.symbol as k, e1.price as p1, e3.price as p3, e3.volume - e1.volume as dv, "
           "e1.timestamp as i1, e3.timestamp as i3")
PKINDS = ["i", "d", "d", "i", "i", "i"]


def words(row):
    return [struct.unpack("<q", struct.pack("<d", v))[0] if k == "d" else int(v) for v, k in zip(row, PKINDS)]


@pytest.mark.parametrize("mirrored", [False, True])
@pytest.mark.parametrize("keyed", [True, False])
def test_device_project_equals_oracle(keyed, mirrored):
    t, sid, cols, ts = case("symbol" if keyed else "flat", select=PSELECT, mirrored=mirrored)
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
    assert set(r.paths) == {12}
    r.app.close()
    assert got == [[row[0], words(row[1])] for row in rows]


def test_callbacks_receive_the_oracles_events():
    """A StreamCallback and a columns callback through SiddhiAppRuntime.sendDeviceEvents: one call per e3, in order of
    it, before the call returns."""
    import torch
    import siddhi_amd
    from siddhi_amd import ColumnsStreamCallback, SiddhiManager, StreamCallback
    sid, cols, ts = events(n=N, K=20)
    t = text(keys=BY_SYMBOL, select=PSELECT, c3="price > 40", within=200, c2="[price>55]")
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
            assert v.value == 12
            seen.append(sum(len(c) for c in evs) + sum(len(c[0]) for c in columns))
        rt.shutdown()
    # one chunk per e3: the outputs one e3 completes arrive together, oldest e1 first
    flat_evs = [e for chunk in evs for e in chunk]
    assert flat_evs == [[r[0], r[1]] for r in rows]
    assert [len(c) for c in evs] == np.unique(pairs[:, 1], return_counts=True)[1].tolist()
    assert max(len(c) for c in evs) >= 2
    assert [w for c in columns for w in c[1]] == [words(r[1]) for r in rows]
    assert [x for c in columns for x in c[0]] == [r[0] for r in rows]
    assert seen[0] == int((pairs[:, 1] < ranges[0][1]).sum())  # delivered before the call returned


def test_match_arity_and_timing_labels():
    sid, cols, ts = events(n=N, K=20)
    n = len(ts)
    r = Run(text(keys=BY_SYMBOL), fast_timing=1)
    assert r.app.get_stat("match_arity:q") == 2
    r.piece(sid, cols, ts, 0, n // 2)
    labels = ["pnand_facts", "pnand_pack", "pnand_sort", "pnand_next", "pnand_link", "pnand_count", "pnand_scan",
              "pnand_emit", "pnand_order", "pnand_carry"]
    for label in labels:
        assert r.app.get_stat(f"kernel_calls:{label}") == 1
        assert r.app.get_stat(f"kernel_ms:{label}") >= 0
    assert r.app.get_stat("kernel_calls:mpat_link") == 0 and r.app.get_stat("kernel_calls:absent_next") == 0
    r.piece(sid, cols, ts, n // 2, n)
    assert r.paths == [12, 12] and r.app.get_stat("nfa_state:q") == 0
    r.app.close()
