"""The adjacent-run closed form of the k-state sequence `every e1=S[c1], e2=S[c2], ..., ek=S[ck]` (3 <= k <= 8, one
stream) on device batches (sm_app_process_device_batch, fast_path 7: kernels/seqpath.hip fast_seq_k, seq_dev.h)
against the CPU oracle. A sequence's partial lives for one event of its partition instance at every state, so the
outputs are runs of k adjacent events of an instance, at most one per last event; the product carries each instance's
last k - 1 events across device batches. Every case compares the (e1, ..., ek) ordinals of the whole stream, tuple for
tuple and in order, with the oracle's, and checks the path taken."""
import ctypes
import functools
import struct

import numpy as np
import pytest

from test_device_batch import PART, SCHEMA, stock, value_column
from test_device_seq import RANGES5, decreasing_streams, oracle_rows
from test_device_stream import SPLITS, pieces, run_stream

pytestmark = pytest.mark.gpu


def seqk_text(k=3, partitioned=True, c1="[price>20]", cm="price > {p}.price - 10.0 and volume != e1.volume",
              withins=None, kt="int", vt="double", select=None):
    """cm: the condition of elements 2 .. k, {p} = the previous element; withins: {m: text} on element m (1-based)."""
    withins = withins or {}
    els = [f"every e1=StockStream{c1}"]
    for m in range(2, k + 1):
        els.append(f"e{m}=StockStream[{cm.format(p=f'e{m - 1}')}]{withins.get(m, '')}")
    sel = select or "select " + ", ".join(f"e{m}.timestamp as i{m}" for m in range(1, k + 1))
    q = f"@info(name='q') from {', '.join(els)} {sel} insert into OutputStream;"
    return SCHEMA.format(kt=kt).replace("price double", f"price {vt}") + (PART.format(q=q) if partitioned else q)


def oracle_tuples(text, cols, ts, k):
    """(m, k) ordinals of the oracle's outputs (the select reads every slot once: its refs are the tuple)."""
    return np.array([r[2] for r in oracle_rows(text, cols, ts)], dtype=np.int64).reshape(-1, k)


@functools.lru_cache(maxsize=None)
def keyed_case(k, n, K, div=3):
    cols, ts = stock(n, K, div)
    return cols, ts, oracle_tuples(seqk_text(k), cols, ts, k)


# unkeyed streams: a condition most events pass, so that tuples lie across every batch boundary
UNKEYED_CM = "price > {p}.price - 60.0 and volume != e1.volume"


def unkeyed_text(k, **kw):
    return seqk_text(k, partitioned=False, cm=UNKEYED_CM, **kw)


@functools.lru_cache(maxsize=None)
def unkeyed_case(k, n):
    cols, _ = stock(n, 10, 1, config=1)
    ts = np.arange(n, dtype=np.int64)
    return cols, ts, oracle_tuples(unkeyed_text(k), cols, ts, k)


# ---- 1. shapes

SIZES = [1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 8191, 8193, 200000]


@pytest.mark.parametrize("K", [1, 50, 3000])
@pytest.mark.parametrize("k", [3, 4])
def test_keyed_shapes(k, K):
    seen = 0
    for n in SIZES:
        cols, ts, exp = keyed_case(k, n, K)
        got = run_stream(seqk_text(k), cols, ts, [(0, n)], expect_path=7)
        assert got.shape[1] == k
        np.testing.assert_array_equal(got, exp)
        seen += len(exp)
    assert seen > 0


@pytest.mark.parametrize("k", [3, 4])
def test_unkeyed_shapes(k):
    for n in SIZES:
        cols, ts, exp = unkeyed_case(k, n)
        got = run_stream(unkeyed_text(k), cols, ts, [(0, n)], expect_path=7)
        if n >= 63:
            assert len(exp) > 0
        np.testing.assert_array_equal(got, exp)


def test_more_keys_than_events():
    """Most keys have one or two events: runs shorter than k, nothing to emit, every event carried."""
    n, K = 3000, 1_000_000
    cols, ts, exp = keyed_case(3, n, K)
    got = run_stream(seqk_text(3), cols, ts, [(0, n)], expect_path=7)
    np.testing.assert_array_equal(got, exp)
    got = run_stream(seqk_text(3), cols, ts, pieces(n, [1000, 1000]), expect_path=7)
    np.testing.assert_array_equal(got, exp)


# ---- 2. split batches

def straddles(exp, ranges):
    """(tuples whose members lie in two pieces: one boundary; tuples whose members lie in three or more)"""
    los = np.array([lo for lo, _ in ranges[1:]], dtype=np.int64)
    piece = np.searchsorted(los, exp, side="right")
    distinct = np.array([len(set(r)) for r in piece], dtype=np.int64)
    return int((distinct == 2).sum()), int((distinct >= 3).sum())


@pytest.mark.parametrize("splits", [[1] * 50 + [999], SPLITS, [5000] * 10], ids=["ones", "ragged", "5000s"])
@pytest.mark.parametrize("k", [3, 4])
def test_unkeyed_split_batches(k, splits):
    n = 60000
    cols, ts, exp = unkeyed_case(k, n)
    ranges = pieces(n, splits)
    one, two = straddles(exp, ranges)
    assert len(exp) > 0 and one > 0
    if len(splits) > 10 and splits[0] == 1:
        assert two > 0  # among the one-event pieces a tuple's members lie in k pieces
    got = run_stream(unkeyed_text(k), cols, ts, ranges, expect_path=7)
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("splits", [[1] * 50 + [999], SPLITS, [5000] * 10], ids=["ones", "ragged", "5000s"])
@pytest.mark.parametrize("k", [3, 4])
def test_keyed_split_batches(k, splits):
    n, K = 60000, 50
    cols, ts, exp = keyed_case(k, n, K, 3)
    ranges = pieces(n, splits)
    one, two = straddles(exp, ranges)
    assert len(exp) > 0 and one > 0
    got = run_stream(seqk_text(k), cols, ts, ranges, expect_path=7)
    np.testing.assert_array_equal(got, exp)


def test_tuples_straddle_two_boundaries_keyed():
    """Pieces shorter than the gap between a key's events: a key's tuple takes members from three pieces, the oldest
    of them from rows that were carried twice."""
    n, K = 6000, 40
    cols, ts, exp = keyed_case(3, n, K, 3)
    ranges = pieces(n, [30] * 100)
    _, two = straddles(exp, ranges)
    assert two > 0
    got = run_stream(seqk_text(3), cols, ts, ranges, expect_path=7)
    np.testing.assert_array_equal(got, exp)


def test_keyed_silent_keys_keep_their_carried_rows():
    """Keys below 60 are silent for two whole pieces while they hold carried rows; their next events complete tuples
    with them (no `within`) across the gap, as in the oracle."""
    n, K = 24000, 120
    cols, ts = stock(n, K, 5)
    cols = [c.copy() for c in cols]
    sym = cols[0]
    sym[8000:16000] = np.where(sym[8000:16000] < 60, sym[8000:16000] + 60, sym[8000:16000])
    text = seqk_text(3)
    exp = oracle_tuples(text, cols, ts, 3)
    ranges = [(0, 4000), (4000, 8000), (8000, 12000), (12000, 16000), (16000, n)]
    span = exp[(exp[:, 0] < 8000) & (exp[:, 2] >= 16000)]
    assert len(span) > 0 and (sym[span[:, 0]] < 60).all()
    assert ((span[:, 1] < 8000).any() and (span[:, 1] >= 16000).any())  # two carried members, and one
    got = run_stream(text, cols, ts, ranges, expect_path=7)
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("partitioned", [True, False])
def test_zero_length_batch_between_pieces(partitioned):
    n = 20000
    cols, ts, exp = keyed_case(3, n, 50, 3) if partitioned else unkeyed_case(3, n)
    ranges = [(0, 7000), (7000, 7000), (7000, n)]
    assert straddles(exp, [(0, 7000), (7000, n)])[0] > 0
    got = run_stream(seqk_text(3) if partitioned else unkeyed_text(3), cols, ts, ranges, expect_path=7)
    np.testing.assert_array_equal(got, exp)


# ---- 3. within

@pytest.mark.parametrize("k", [3, 4])
def test_within_boundary_is_inclusive(k):
    """Same-key gaps of exactly T - 1, T and T + 1 between e(k-1) and ek: the oracle keeps the first two."""
    T, K, reps = 7, 5, 40
    gaps = np.tile(np.array([T - 1, T, T + 1]), reps)
    per_key_ts = np.concatenate([[0], np.cumsum(gaps)])
    m = len(per_key_ts)
    tsk = np.repeat(per_key_ts, K)
    key = np.tile(np.arange(K, dtype=np.int32), m)
    n = len(tsk)
    price = 21.0 + np.arange(n, dtype=np.float64)  # rising: every condition holds, the last gap decides
    tsa = np.arange(n, dtype=np.int64)
    cols = [key, price, tsa.copy(), tsa]
    text = seqk_text(k, withins={k: f" within {T} milliseconds"})
    exp = oracle_tuples(text, cols, tsk, k)
    gap = tsk[exp[:, k - 1]] - tsk[exp[:, k - 2]]
    assert (gap == T).any() and (gap == T - 1).any() and not (gap == T + 1).any()
    assert (tsk[exp[:, k - 1]] - tsk[exp[:, 0]] > T).any()  # measured against the previous element, not e1
    got = run_stream(text, cols, tsk, pieces(n, [K * 3 + 2, 1, 77]), expect_path=7)
    np.testing.assert_array_equal(got, exp)


def test_within_on_a_middle_and_on_two_elements():
    n, K = 20000, 40
    cols, ts = stock(n, K, 2)
    for w in ({2: " within 30 milliseconds"}, {2: " within 40 milliseconds", 4: " within 25 milliseconds"}):
        text = seqk_text(4, withins=w)
        exp = oracle_tuples(text, cols, ts, 4)
        full = oracle_tuples(seqk_text(4), cols, ts, 4)
        assert 0 < len(exp) < len(full)
        got = run_stream(text, cols, ts, pieces(n, [1, 8191]), expect_path=7)
        np.testing.assert_array_equal(got, exp)


# ---- 4. decreasing event time

def paths_and_tuples(text, cols, ts, ranges, **options):
    import torch
    from siddhi_amd.testing import ProductApp
    app = ProductApp(text, **options)
    dev = torch.device("cuda", 0)
    got, paths = [], []
    for lo, hi in ranges:
        tcols = [torch.from_numpy(np.ascontiguousarray(c[lo:hi])).to(dev) for c in cols]
        tts = torch.from_numpy(np.ascontiguousarray(ts[lo:hi], dtype=np.int64)).to(dev)
        torch.cuda.synchronize()
        app.process_device_batch("StockStream", tts, tcols, ordinal_base=lo)
        got.append(app.device_matches_host("q").view(np.int32).astype(np.int64) + lo)
        paths.append(int(app.get_stat("fast_path:q")))
    state = int(app.get_stat("nfa_state:q"))
    app.close()
    return np.concatenate(got), paths, state


@pytest.mark.parametrize("case", ["inside", "before_carry"])
@pytest.mark.parametrize("partitioned", [True, False])
def test_decreasing_time_with_within_hands_over(case, partitioned):
    cols, tss = decreasing_streams()
    ts = tss[case]
    text = seqk_text(3, partitioned=partitioned, withins={3: " within 30 milliseconds"})
    exp = oracle_tuples(text, cols, ts, 3)
    assert len(exp) > 0
    got, paths, state = paths_and_tuples(text, cols, ts, RANGES5)
    assert paths == [7, 7, 5, 5, 5] and state == 1  # handed over at the first such batch, for good
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("case", ["inside", "before_carry"])
@pytest.mark.parametrize("partitioned", [True, False])
def test_decreasing_time_without_within_stays(case, partitioned):
    """No condition reads event time (tests/test_seqk_plan.py checks the rule on such a stream)."""
    cols, tss = decreasing_streams()
    ts = tss[case]
    text = seqk_text(3, partitioned=partitioned)
    exp = oracle_tuples(text, cols, ts, 3)
    assert len(exp) > 0
    got, paths, state = paths_and_tuples(text, cols, ts, RANGES5)
    assert paths == [7] * 5 and state == 0
    np.testing.assert_array_equal(got, exp)


# ---- 5. conditions, key kinds, special values

@pytest.mark.parametrize("variant", ["no_c1", "k8", "long_keys", "negative_keys", "key_remap", "long_keys_remap_auto",
                                     "long_keys_wide_later"])
def test_variants(variant):
    n, K, div = 30000, 300, 20
    k, kw, kd, ko, opts = 3, {}, np.int32, 0, {}
    if variant == "no_c1":
        kw["c1"] = ""
    elif variant == "k8":
        k, K = 8, 30
        kw["cm"] = "price > {p}.price - 30.0 and volume != e1.volume"
    elif variant in ("long_keys", "long_keys_remap_auto", "long_keys_wide_later"):
        kw["kt"] = "long"
        kd, ko = np.int64, 1 << 40
    elif variant == "negative_keys":
        ko = -150
    elif variant == "key_remap":
        opts["key_remap"] = 1
    cols, ts = stock(n, K, div, key_dtype=kd, key_offset=ko)
    splits = [1, 8191, 9000]
    if variant == "long_keys_remap_auto":
        cols[0] = cols[0] * 5_000_011  # the first batch spans more than 2^30 keys: dense ids by themselves
        splits = [8191, 9000]
    if variant == "long_keys_wide_later":
        cols[0] = cols[0] * 50_000_011  # one key in the first batch, then a span above 2^32: 64-bit sort keys
    text = seqk_text(k, **kw)
    exp = oracle_tuples(text, cols, ts, k)
    assert len(exp) > 0
    got, paths, _ = paths_and_tuples(text, cols, ts, pieces(n, splits), **opts)
    assert paths == [7] * len(paths)
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("cm", ["price > {p}.price or price == e1.price", "price != {p}.price", "e1.price <= price"])
@pytest.mark.parametrize("partitioned", [True, False])
def test_double_special_values(cm, partitioned):
    """NaN, -0.0 / 0.0 and the infinities: the interpreter compares as Java does (NaN: only != holds)."""
    n, K = 20000, 30
    rng = np.random.default_rng(len(cm) * 2 + partitioned)
    vt, price = value_column("double_special", n, rng)
    sym = rng.integers(0, K, n).astype(np.int32)
    vol = rng.integers(0, 2000, n).astype(np.int64)
    tsa = np.arange(n, dtype=np.int64)
    cols = [sym, price, vol, tsa]
    text = seqk_text(3, partitioned=partitioned, c1="", cm=cm, vt=vt)
    exp = oracle_tuples(text, cols, tsa // 4, 3)
    assert len(exp) > 0
    got = run_stream(text, cols, tsa // 4, pieces(n, [1, 8191, 3333]), expect_path=7)
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("partitioned", [True, False])
def test_given_ordinals_sharded_style(partitioned):
    """Events carrying the global ordinals 3 i + 1 with ordinal_base = 0: one batch takes path 7; in pieces the tuples
    still equal the oracle's (carried members must precede ordinal_base, so with base 0 later pieces run on the NFA)."""
    n = 30000
    cols, ts, exp = keyed_case(3, n, 50, 3) if partitioned else unkeyed_case(3, n)
    text = seqk_text(3) if partitioned else unkeyed_text(3)
    ordinals = 3 * np.arange(n, dtype=np.int64) + 1
    assert len(exp) > 0
    got = run_stream(text, cols, ts, [(0, n)], ordinals=ordinals, expect_path=7)
    np.testing.assert_array_equal(got, 3 * exp + 1)
    got = run_stream(text, cols, ts, pieces(n, [1, 8191]), ordinals=ordinals)
    np.testing.assert_array_equal(got, 3 * exp + 1)


# ---- 6. projection and callbacks

PSELECT = ("select e1.symbol as k, e1.price as p1, e2.price as p2, e3.price as p3, e3.volume - e1.volume as dv, "
           "e1.timestamp as i1, e2.timestamp as i2, e3.timestamp as i3")
PKINDS = ["i", "d", "d", "d", "i", "i", "i", "i"]


def proj_text(partitioned):
    return seqk_text(3, partitioned=partitioned, select=PSELECT, **({} if partitioned else {"cm": UNKEYED_CM}))


def words(row):
    return [struct.unpack("<q", struct.pack("<d", v))[0] if k == "d" else int(v) for v, k in zip(row, PKINDS)]


@pytest.mark.parametrize("partitioned", [True, False])
def test_device_project_equals_oracle(partitioned):
    import torch
    from siddhi_amd.testing import ProductApp
    n = 30000
    cols, ts = stock(n, 80, 5)
    text = proj_text(partitioned)
    exp = oracle_rows(text, cols, ts)
    ranges = pieces(n, [1, 8191] + [700] * 12)
    tuples = np.array([r[1][5:8] for r in exp], dtype=np.int64)
    los = [lo for lo, _ in ranges[1:]]
    # outputs whose first member, and whose first two members, are read from the carry
    assert len(exp) > 100
    assert any(((tuples[:, 0] < lo) & (tuples[:, 1] >= lo)).any() for lo in los)
    assert any(((tuples[:, 1] < lo) & (tuples[:, 2] >= lo)).any() for lo in los)
    app = ProductApp(text)
    dev = torch.device("cuda", 0)
    got = []
    for lo, hi in ranges:
        tcols = [torch.from_numpy(np.ascontiguousarray(c[lo:hi])).to(dev) for c in cols]
        tts = torch.from_numpy(np.ascontiguousarray(ts[lo:hi], dtype=np.int64)).to(dev)
        torch.cuda.synchronize()
        app.process_device_batch("StockStream", tts, tcols, ordinal_base=lo)
        assert app.get_stat("fast_path:q") == 7
        vals, nulls, ots = app.device_project("q")
        torch.cuda.synchronize()
        assert not nulls.any()
        got += [[t, r] for t, r in zip(ots.cpu().tolist(), vals.cpu().tolist())]
    app.close()
    assert got == [[r[0], words(r[1])] for r in exp]


def test_callbacks_receive_the_oracles_events():
    """A StreamCallback and a columns callback through SiddhiAppRuntime.sendDeviceBatch: one call per last event."""
    import torch
    import siddhi_amd
    from siddhi_amd import ColumnsStreamCallback, SiddhiManager, StreamCallback
    n = 20000
    cols, ts = stock(n, 80, 5)
    text = proj_text(True)
    exp = oracle_rows(text, cols, ts)
    assert len(exp) > 100
    events, columns = [], []

    class SC(StreamCallback):
        def receive(self, evs):
            events.append([[e.timestamp, e.data] for e in evs])

    class CC(ColumnsStreamCallback):
        def receive_columns(self, timestamps, values, null_bits):
            columns.append([timestamps, values, null_bits])

    dev = torch.device("cuda", 0)
    for cb in (SC(), CC()):
        rt = SiddhiManager().createSiddhiAppRuntime(text)
        rt.addCallback("OutputStream", cb)
        rt.start()
        for lo, hi in pieces(n, [1, 8191]):
            tcols = [torch.from_numpy(np.ascontiguousarray(c[lo:hi])).to(dev) for c in cols]
            tts = torch.from_numpy(np.ascontiguousarray(ts[lo:hi], dtype=np.int64)).to(dev)
            rt.sendDeviceBatch("StockStream", tts, tcols, ordinal_base=lo)
            v = ctypes.c_double()
            siddhi_amd.check(siddhi_amd.lib().sm_app_get_stat(rt._h, b"fast_path:q", ctypes.byref(v)))
            assert v.value == 7
        rt.shutdown()
    assert events == [[[r[0], r[1]]] for r in exp]
    assert columns == [[[r[0]], [words(r[1])], [0]] for r in exp]


# ---- 7. bulk send, host send, snapshot, stats

def test_bulk_send_then_staged_then_device_batch():
    """sm_input_send_columns over bulk_min events goes to the adjacent-run kernels; a later staged send runs on the NFA
    kernel, which takes the carried rows over and keeps the query (nfa_state 1); a device batch after that runs on the
    NFA too (path 5), writing k-tuples from the hidden refs. The whole stream's outputs equal the oracle's."""
    import torch
    from siddhi_amd.testing import ProductApp
    n1, n2, n3 = 70000, 10, 5000
    n = n1 + n2 + n3
    cols, ts = stock(n, 200, 5)
    text = seqk_text(3)
    exp = oracle_tuples(text, cols, ts, 3)
    assert len(exp) > 0
    app = ProductApp(text)
    app.start()
    sl = lambda lo, hi: [np.ascontiguousarray(c[lo:hi]) for c in cols]
    app.send_columns("StockStream", np.ascontiguousarray(ts[:n1]), sl(0, n1))
    assert app.get_stat("fast_path:q") == 7 and app.get_stat("nfa_state:q") == 0
    app.send_columns("StockStream", np.ascontiguousarray(ts[n1:n1 + n2]), sl(n1, n1 + n2))
    app.flush()
    assert app.get_stat("nfa_state:q") == 1
    host = np.array([r[2] for r in app.outputs()["streams"].get("OutputStream", [])], dtype=np.int64).reshape(-1, 3)
    np.testing.assert_array_equal(host, exp[exp[:, 2] < n1 + n2])
    handed = exp[(exp[:, 2] >= n1) & (exp[:, 2] < n1 + n2)]
    assert (handed[:, 0] < n1).any()  # a handed-over row completed
    dev = torch.device("cuda", 0)
    lo = n1 + n2
    tcols = [torch.from_numpy(c).to(dev) for c in sl(lo, n)]
    tts = torch.from_numpy(np.ascontiguousarray(ts[lo:n])).to(dev)
    app.process_device_batch("StockStream", tts, tcols, ordinal_base=lo)
    assert app.get_stat("fast_path:q") == 5 and app.get_stat("match_arity:q") == 3
    tail = app.device_matches_host("q").view(np.int32).astype(np.int64) + lo
    app.close()
    np.testing.assert_array_equal(np.concatenate([host, tail]), exp)


@pytest.mark.parametrize("partitioned", [True, False])
def test_snapshot_restore_keeps_carried_rows(partitioned):
    import torch
    from siddhi_amd.testing import ProductApp
    n = 20000
    cols, ts, exp = keyed_case(3, n, 50, 3) if partitioned else unkeyed_case(3, n)
    text = seqk_text(3) if partitioned else unkeyed_text(3)
    dev = torch.device("cuda", 0)
    cut = int(exp[len(exp) // 2, 1])  # the snapshot is taken between e1 and e2 of an expected tuple
    assert ((exp[:, 0] < cut) & (exp[:, 1] >= cut)).any() and ((exp[:, 1] < cut) & (exp[:, 2] >= cut)).any()

    def batch(app, lo, hi):
        tcols = [torch.from_numpy(np.ascontiguousarray(c[lo:hi])).to(dev) for c in cols]
        tts = torch.from_numpy(np.ascontiguousarray(ts[lo:hi])).to(dev)
        app.process_device_batch("StockStream", tts, tcols, ordinal_base=lo)
        assert app.get_stat("fast_path:q") == 7
        return app.device_matches_host("q").view(np.int32).astype(np.int64) + lo

    a = ProductApp(text)
    first = batch(a, 0, cut)
    snap = a.snapshot()
    a.close()
    b = ProductApp(text)
    b.restore(snap)
    second = batch(b, cut, n)
    b.close()
    np.testing.assert_array_equal(np.concatenate([first, second]), exp)


def test_match_arity_and_timing_labels():
    """match_arity is k here and 2 for a pair query; the adjacent-run launches have labels of their own."""
    import torch
    from siddhi_amd.testing import ProductApp
    from test_device_seq import seq_text
    n = 20000
    cols, ts, _ = keyed_case(3, n, 50, 3)
    dev = torch.device("cuda", 0)
    tcols = [torch.from_numpy(np.ascontiguousarray(c)).to(dev) for c in cols]
    app = ProductApp(seqk_text(3), fast_timing=1)
    assert app.get_stat("match_arity:q") == 3
    app.process_device_batch("StockStream", torch.from_numpy(ts).to(dev), tcols, ordinal_base=0)
    for label in ("seqk_facts", "seqk_sort", "seqk_link", "seqk_count", "seqk_scan", "seqk_emit", "seqk_carry"):
        assert app.get_stat(f"kernel_calls:{label}") == 1
        assert app.get_stat(f"kernel_ms:{label}") >= 0
    assert app.get_stat("kernel_calls:seq_link") == 0
    app.close()
    pair = ProductApp(seq_text())
    assert pair.get_stat("match_arity:q") == 2
    pair.close()
    four = ProductApp(seqk_text(4))
    assert four.get_stat("match_arity:q") == 4
    four.close()
