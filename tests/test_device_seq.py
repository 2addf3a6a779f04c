"""The adjacent-pair closed form of the sequence `every e1=S[c1], e2=S[c2] [within T]` on device batches
(sm_app_process_device_batch, fast_path 6: kernels/seqpath.hip, seq_dev.h) against the CPU oracle. In the reference a
sequence's partial lives for one event of its partition instance (SequenceMultiProcessStreamReceiver.stabilizeStates
:59-61 → StateStreamRuntime.resetAndUpdate after every event), so the outputs are adjacent pairs of each instance;
the product carries each key's last event (if it passes c1) across device batches. Every case compares the (e1, e2)
ordinals of the whole stream, tuple for tuple and in order, with the oracle's, and checks the path taken."""
import functools
import struct

import numpy as np
import pytest

from test_device_batch import PART, SCHEMA, oracle_pairs, stock, value_column
from test_device_stream import SPLITS, pieces, run_stream

pytestmark = pytest.mark.gpu

SEQ = ("@info(name='q') from every e1=StockStream{c1}, e2=StockStream[{c2}]{within} "
       "select e1.timestamp as i, e2.timestamp as j insert into OutputStream;")


def seq_text(partitioned=True, c1="[price>20]", c2="price>e1.price", within=" within 1 sec", kt="int", vt="double"):
    q = SEQ.format(c1=c1, c2=c2, within=within)
    return SCHEMA.format(kt=kt).replace("price double", f"price {vt}") + (PART.format(q=q) if partitioned else q)


@functools.lru_cache(maxsize=None)
def keyed_case(n, K, div=3):
    cols, ts = stock(n, K, div)
    return cols, ts, oracle_pairs(seq_text(), cols, ts)


@functools.lru_cache(maxsize=None)
def unkeyed_case(n):
    cols, _ = stock(n, 10, 1, config=1)
    ts = np.arange(n, dtype=np.int64)
    return cols, ts, oracle_pairs(seq_text(partitioned=False), cols, ts)


# ---- 1. shapes

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 8191, 8193, 200000]


@pytest.mark.parametrize("K", [1, 50, 3000])
@pytest.mark.parametrize("n", SIZES)
def test_keyed_shapes(n, K):
    cols, ts, exp = keyed_case(n, K)
    got = run_stream(seq_text(), cols, ts, [(0, n)], expect_path=6)
    if n > 1:
        assert len(exp) > 0 or K > n
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("n", SIZES)
def test_unkeyed_shapes(n):
    cols, ts, exp = unkeyed_case(n)
    got = run_stream(seq_text(partitioned=False), cols, ts, [(0, n)], expect_path=6)
    if n > 2:
        assert len(exp) > 0
    np.testing.assert_array_equal(got, exp)


def test_more_keys_than_events():
    """Most keys have a single event: runs of one, nothing to pair, a carry row per key."""
    n, K = 3000, 1_000_000
    cols, ts, exp = keyed_case(n, K)
    got = run_stream(seq_text(), cols, ts, [(0, n)], expect_path=6)
    np.testing.assert_array_equal(got, exp)
    got = run_stream(seq_text(), cols, ts, pieces(n, [1000, 1000]), expect_path=6)
    np.testing.assert_array_equal(got, exp)


# ---- 2. / 3. split batches

def straddles(exp, ranges):
    """expected pairs whose e1 lies in an earlier piece than their e2"""
    los = np.array([lo for lo, _ in ranges[1:]], dtype=np.int64)
    return int(sum(((exp[:, 0] < lo) & (exp[:, 1] >= lo)).sum() for lo in los))


@pytest.mark.parametrize("splits", [[1] * 50 + [999], SPLITS, [5000] * 10], ids=["ones", "ragged", "5000s"])
def test_unkeyed_split_batches(splits):
    n = 60000
    cols, ts, exp = unkeyed_case(n)
    ranges = pieces(n, splits)
    assert len(exp) > 0 and straddles(exp, ranges) > 0
    if splits[0] == 1 and len(splits) > 10:  # every pair whose e2 is among the first 50 events straddles a boundary
        early = exp[exp[:, 1] < 50]
        assert len(early) > 0 and straddles(early, ranges) == len(early)
    got = run_stream(seq_text(partitioned=False), cols, ts, ranges, expect_path=6)
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("splits", [[1] * 50 + [999], SPLITS, [5000] * 10], ids=["ones", "ragged", "5000s"])
def test_keyed_split_batches(splits):
    n, K = 60000, 50
    cols, ts, exp = keyed_case(n, K, 3)
    ranges = pieces(n, splits)
    assert len(exp) > 0 and straddles(exp, ranges) > 0
    got = run_stream(seq_text(), cols, ts, ranges, expect_path=6)
    np.testing.assert_array_equal(got, exp)


def test_keyed_silent_keys_keep_their_carried_row():
    """Keys below 60 are silent for two whole pieces while they hold a carried row; their next event pairs with it
    (no `within`) across the gap, as in the oracle."""
    n, K = 24000, 120
    cols, ts = stock(n, K, 5)
    cols = [c.copy() for c in cols]
    sym = cols[0]
    sym[8000:16000] = np.where(sym[8000:16000] < 60, sym[8000:16000] + 60, sym[8000:16000])
    text = seq_text(within="")
    exp = oracle_pairs(text, cols, ts)
    ranges = [(0, 4000), (4000, 8000), (8000, 12000), (12000, 16000), (16000, n)]
    # a key silent in [8000, 16000) whose last event before passes c1 (a carried row) and whose pair spans the gap
    span = exp[(exp[:, 0] < 8000) & (exp[:, 1] >= 16000)]
    assert len(span) > 0 and (sym[span[:, 0]] < 60).all()
    got = run_stream(text, cols, ts, ranges, expect_path=6)
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("partitioned", [True, False])
def test_zero_length_batch_between_pieces(partitioned):
    n = 20000
    cols, ts, exp = keyed_case(n, 50, 3) if partitioned else unkeyed_case(n)
    ranges = [(0, 7000), (7000, 7000), (7000, n)]
    assert straddles(exp, [(0, 7000), (7000, n)]) > 0
    got = run_stream(seq_text(partitioned=partitioned), cols, ts, ranges, expect_path=6)
    np.testing.assert_array_equal(got, exp)


# ---- 4. within boundary

def test_within_boundary_is_inclusive():
    """Same-key gaps of exactly T - 1, T and T + 1: the oracle keeps the first two (ts[j] - ts[i] <= T)."""
    T, K, reps = 7, 5, 40
    gaps = np.tile(np.array([T - 1, T, T + 1]), reps)
    per_key_ts = np.concatenate([[0], np.cumsum(gaps)])
    m = len(per_key_ts)
    # events of all keys interleaved in time order (stable by key)
    tsk = np.repeat(per_key_ts, K)
    key = np.tile(np.arange(K, dtype=np.int32), m)
    n = len(tsk)
    price = 21.0 + np.arange(n, dtype=np.float64)  # rising: c1 and c2 always hold, the gap decides
    tsa = np.arange(n, dtype=np.int64)
    cols = [key, price, np.zeros(n, np.int64), tsa]
    text = seq_text(within=f" within {T} milliseconds")
    exp = oracle_pairs(text, cols, tsk)
    gap = tsk[exp[:, 1]] - tsk[exp[:, 0]]
    assert (gap == T).any() and (gap == T - 1).any() and not (gap == T + 1).any()
    assert len(exp) == 2 * reps * K
    got = run_stream(text, cols, tsk, pieces(n, [K * 3 + 2, 1, 77]), expect_path=6)
    np.testing.assert_array_equal(got, exp)


# ---- 5. decreasing event time

def paths_and_pairs(text, cols, ts, ranges, **options):
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


def decreasing_streams():
    n, K = 20000, 40
    cols, ts = stock(n, K, 2)
    inside = ts.copy()
    inside[9000:9500] = inside[9000:9500][::-1]  # time decreases inside the third piece
    assert (np.diff(inside[8000:12000]) < 0).any()
    before = ts.copy()
    before[8000:] -= 5  # the third piece starts before the last carried event time, monotone inside
    assert before[8000] < before[7999] and (np.diff(before[8000:]) >= 0).all()
    return cols, {"inside": inside, "before_carry": before}


RANGES5 = [(0, 4000), (4000, 8000), (8000, 12000), (12000, 16000), (16000, 20000)]


@pytest.mark.parametrize("case", ["inside", "before_carry"])
@pytest.mark.parametrize("partitioned", [True, False])
def test_decreasing_time_with_within_hands_over(case, partitioned):
    cols, tss = decreasing_streams()
    ts = tss[case]
    text = seq_text(partitioned=partitioned, within=" within 3 milliseconds")
    exp = oracle_pairs(text, cols, ts)
    assert len(exp) > 0
    got, paths, state = paths_and_pairs(text, cols, ts, RANGES5)
    assert paths == [6, 6, 5, 5, 5] and state == 1  # handed over at the first such batch, for good
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("case", ["inside", "before_carry"])
@pytest.mark.parametrize("partitioned", [True, False])
def test_decreasing_time_without_within_stays(case, partitioned):
    cols, tss = decreasing_streams()
    ts = tss[case]
    text = seq_text(partitioned=partitioned, within="")
    exp = oracle_pairs(text, cols, ts)
    assert len(exp) > 0
    got, paths, state = paths_and_pairs(text, cols, ts, RANGES5)
    assert paths == [6] * 5 and state == 0
    np.testing.assert_array_equal(got, exp)


# ---- 6. conditions, key kinds, special values

@pytest.mark.parametrize("variant", ["no_c1", "c1_and", "c2_plus_and", "c2_const_only", "c2_eq_ties", "long_keys",
                                     "negative_keys", "key_remap", "long_keys_remap_auto",
                                     "long_keys_wide_later"])
def test_variants(variant):
    n, K, div = 30000, 300, 20
    kw, kd, ko, opts = {}, np.int32, 0, {}
    if variant == "no_c1":
        kw["c1"] = ""
    elif variant == "c1_and":
        kw["c1"] = "[price > 30 and volume < 1500]"
    elif variant == "c2_plus_and":
        kw["c2"] = "price > e1.price + 5.0 and volume < e1.volume"
    elif variant == "c2_const_only":
        kw["c2"] = "price > 30"
    elif variant == "c2_eq_ties":
        kw["c2"] = "price == e1.price"
    elif variant in ("long_keys", "long_keys_remap_auto", "long_keys_wide_later"):
        kw["kt"] = "long"
        kd, ko = np.int64, 1 << 40
    elif variant == "negative_keys":
        ko = -150
    elif variant == "key_remap":
        opts["key_remap"] = 1
    cols, ts = stock(n, K, div, key_dtype=kd, key_offset=ko)
    if variant == "c2_eq_ties":
        cols[1] = 21.0 + (np.arange(n) * 7 % 3).astype(np.float64)  # three prices: ties everywhere
    splits = [1, 8191, 9000]
    if variant == "long_keys_remap_auto":
        cols[0] = cols[0] * 5_000_011  # the first batch spans more than 2^30 keys: dense ids by themselves
        splits = [8191, 9000]
    if variant == "long_keys_wide_later":
        cols[0] = cols[0] * 50_000_011  # one key in the first batch, then a span above 2^32: 64-bit sort keys
    text = seq_text(**kw)
    exp = oracle_pairs(text, cols, ts)
    assert len(exp) > 0
    got, paths, _ = paths_and_pairs(text, cols, ts, pieces(n, splits), **opts)
    assert paths == [6] * len(paths)
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("c2", ["price > e1.price", "price == e1.price", "price != e1.price", "e1.price <= price"])
@pytest.mark.parametrize("partitioned", [True, False])
def test_double_special_values(c2, partitioned):
    """NaN, -0.0 / 0.0 and the infinities: the interpreter compares as Java does (NaN: only != holds)."""
    n, K = 20000, 30
    rng = np.random.default_rng(abs(hash((c2, partitioned))) % (1 << 32))
    vt, price = value_column("double_special", n, rng)
    sym = rng.integers(0, K, n).astype(np.int32)
    vol = rng.integers(0, 2000, n).astype(np.int64)
    tsa = np.arange(n, dtype=np.int64)
    cols = [sym, price, vol, tsa]
    text = seq_text(partitioned=partitioned, c1="", c2=c2, vt=vt)
    exp = oracle_pairs(text, cols, tsa // 4)
    assert len(exp) > 0
    got = run_stream(text, cols, tsa // 4, pieces(n, [1, 8191, 3333]), expect_path=6)
    np.testing.assert_array_equal(got, exp)


# ---- 7. given ordinals

@pytest.mark.parametrize("partitioned", [True, False])
def test_given_ordinals_sharded_style(partitioned):
    """Events carrying the global ordinals 3 k + 1 with ordinal_base = 0: one batch takes path 6; in pieces the pairs
    still equal the oracle's (a carried e1 must precede ordinal_base for the on-device projection to tell it from a
    batch row, so with base 0 the later pieces run on the NFA kernel)."""
    n = 30000
    cols, ts, exp = keyed_case(n, 50, 3) if partitioned else unkeyed_case(n)
    text = seq_text(partitioned=partitioned)
    ordinals = 3 * np.arange(n, dtype=np.int64) + 1
    assert len(exp) > 0
    got = run_stream(text, cols, ts, [(0, n)], ordinals=ordinals, expect_path=6)
    np.testing.assert_array_equal(got, 3 * exp + 1)
    got = run_stream(text, cols, ts, pieces(n, [1, 8191]), ordinals=ordinals)
    np.testing.assert_array_equal(got, 3 * exp + 1)


# ---- 8. projection and callbacks

PSELECT = ("select e1.symbol as k, e1.price as p1, e2.price as p2, e2.volume - e1.volume as dv, "
           "e1.timestamp as i, e2.timestamp as j")
PKINDS = ["i", "d", "d", "i", "i", "i"]  # k; p1, p2 doubles (compared by their bits); dv, i, j


def proj_text(partitioned):
    q = ("@info(name='q') from every e1=StockStream[price>20], e2=StockStream[price>e1.price] within 1 sec "
         + PSELECT + " insert into OutputStream;")
    return SCHEMA.format(kt="int") + (PART.format(q=q) if partitioned else q)


def oracle_rows(text, cols, ts):
    import ctypes
    from oracle_lib import OracleApp, lib as olib
    a = OracleApp(text)
    a.start()
    cs = [np.ascontiguousarray(c) for c in cols]
    ptrs = (ctypes.c_void_p * len(cs))(*[c.ctypes.data for c in cs])
    err = ctypes.create_string_buffer(512)
    t = np.ascontiguousarray(ts, dtype=np.int64)
    assert olib().cr_send_columns(a.h, a.stream_index("StockStream"), len(t), t.ctypes.data, ptrs, err, 512) == 0
    out = a.outputs()["streams"].get("OutputStream", [])
    a.close()
    return out


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
    ranges = pieces(n, [1, 8191, 5000])
    pairs = np.array([[r[1][4], r[1][5]] for r in exp], dtype=np.int64)
    assert len(exp) > 100 and straddles(pairs, ranges) > 0  # outputs whose e1 is read from the carry
    app = ProductApp(text)
    dev = torch.device("cuda", 0)
    got = []
    for lo, hi in ranges:
        tcols = [torch.from_numpy(np.ascontiguousarray(c[lo:hi])).to(dev) for c in cols]
        tts = torch.from_numpy(np.ascontiguousarray(ts[lo:hi], dtype=np.int64)).to(dev)
        torch.cuda.synchronize()
        app.process_device_batch("StockStream", tts, tcols, ordinal_base=lo)
        assert app.get_stat("fast_path:q") == 6
        vals, nulls, ots = app.device_project("q")
        torch.cuda.synchronize()
        assert not nulls.any()
        got += [[t, r] for t, r in zip(ots.cpu().tolist(), vals.cpu().tolist())]
    app.close()
    assert got == [[r[0], words(r[1])] for r in exp]


def test_callbacks_receive_the_oracles_events():
    """A StreamCallback and a columns callback through SiddhiAppRuntime.sendDeviceBatch: one call per e2 event."""
    import ctypes

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
    for cb, sink in ((SC(), events), (CC(), columns)):
        rt = SiddhiManager().createSiddhiAppRuntime(text)
        rt.addCallback("OutputStream", cb)
        rt.start()
        for lo, hi in pieces(n, [1, 8191]):
            tcols = [torch.from_numpy(np.ascontiguousarray(c[lo:hi])).to(dev) for c in cols]
            tts = torch.from_numpy(np.ascontiguousarray(ts[lo:hi], dtype=np.int64)).to(dev)
            rt.sendDeviceBatch("StockStream", tts, tcols, ordinal_base=lo)
            v = ctypes.c_double()
            siddhi_amd.check(siddhi_amd.lib().sm_app_get_stat(rt._h, b"fast_path:q", ctypes.byref(v)))
            assert v.value == 6
        rt.shutdown()
    # each e2 has at most one output: one call per output, in the oracle's order
    assert events == [[[r[0], r[1]]] for r in exp]
    assert columns == [[[r[0]], [words(r[1])], [0]] for r in exp]


# ---- 9. bulk send

def test_bulk_send_then_staged_then_device_batch():
    """sm_input_send_columns over bulk_min events goes to the adjacent-pair kernels; a later staged send runs on the
    NFA kernel, which takes the carried rows over and keeps the query (nfa_state 1); a device batch after that runs on
    the NFA too (path 5). The whole stream's outputs equal the oracle's."""
    import torch
    from siddhi_amd.testing import ProductApp
    n1, n2, n3 = 70000, 10, 5000
    n = n1 + n2 + n3
    cols, ts = stock(n, 200, 5)
    text = seq_text()
    exp = oracle_pairs(text, cols, ts)
    assert len(exp) > 0
    app = ProductApp(text)
    app.start()
    sl = lambda lo, hi: [np.ascontiguousarray(c[lo:hi]) for c in cols]
    app.send_columns("StockStream", np.ascontiguousarray(ts[:n1]), sl(0, n1))
    assert app.get_stat("fast_path:q") == 6 and app.get_stat("nfa_state:q") == 0
    app.send_columns("StockStream", np.ascontiguousarray(ts[n1:n1 + n2]), sl(n1, n1 + n2))
    app.flush()
    assert app.get_stat("nfa_state:q") == 1
    host = np.array([r[2] for r in app.outputs()["streams"].get("OutputStream", [])], dtype=np.int64).reshape(-1, 2)
    np.testing.assert_array_equal(host, exp[exp[:, 1] < n1 + n2])
    assert ((exp[:, 0] < n1) & (exp[:, 1] >= n1) & (exp[:, 1] < n1 + n2)).any()  # a handed-over row completed
    dev = torch.device("cuda", 0)
    lo = n1 + n2
    tcols = [torch.from_numpy(c).to(dev) for c in sl(lo, n)]
    tts = torch.from_numpy(np.ascontiguousarray(ts[lo:n])).to(dev)
    app.process_device_batch("StockStream", tts, tcols, ordinal_base=lo)
    assert app.get_stat("fast_path:q") == 5
    tail = app.device_matches_host("q").view(np.int32).astype(np.int64) + lo
    app.close()
    np.testing.assert_array_equal(np.concatenate([host, tail]), exp)


# ---- 10. snapshot

@pytest.mark.parametrize("partitioned", [True, False])
def test_snapshot_restore_keeps_carried_rows(partitioned):
    import torch
    from siddhi_amd.testing import ProductApp
    n = 20000
    cols, ts, exp = keyed_case(n, 50, 3) if partitioned else unkeyed_case(n)
    text = seq_text(partitioned=partitioned)
    dev = torch.device("cuda", 0)
    cut = int(exp[len(exp) // 2, 1])  # the snapshot is taken between the two events of an expected pair
    assert straddles(exp, [(0, cut), (cut, n)]) > 0

    def batch(app, lo, hi):
        tcols = [torch.from_numpy(np.ascontiguousarray(c[lo:hi])).to(dev) for c in cols]
        tts = torch.from_numpy(np.ascontiguousarray(ts[lo:hi])).to(dev)
        app.process_device_batch("StockStream", tts, tcols, ordinal_base=lo)
        assert app.get_stat("fast_path:q") == 6
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


def test_fast_timing_labels():
    """kernel_ms / kernel_calls labels of the adjacent-pair launches (option fast_timing)."""
    import torch
    from siddhi_amd.testing import ProductApp
    n = 20000
    cols, ts, _ = keyed_case(n, 50, 3)
    app = ProductApp(seq_text(), fast_timing=1)
    dev = torch.device("cuda", 0)
    tcols = [torch.from_numpy(np.ascontiguousarray(c)).to(dev) for c in cols]
    app.process_device_batch("StockStream", torch.from_numpy(ts).to(dev), tcols, ordinal_base=0)
    for label in ("seq_facts", "seq_sort", "seq_link", "seq_count", "seq_scan", "seq_emit", "seq_carry"):
        assert app.get_stat(f"kernel_calls:{label}") == 1
        assert app.get_stat(f"kernel_ms:{label}") >= 0
    app.close()
