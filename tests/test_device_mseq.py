"""The adjacent-run closed form of sequences over several streams, `every e1=S1[c1], e2=S2[c2], ..., ek=Sk[ck]`
(2 <= k <= 8, streams of one schema), on interleaved device batches (sm_app_process_device_events, fast_path 8:
kernels/seqpath.hip fast_seq_ms, mseq_dev.h) against the CPU oracle fed the same events. The outputs are runs of k
adjacent events of a partition instance among the events of the streams the query reads, at most one per last event;
the product carries each instance's last k - 1 read events (with their streams) across batches. Every case compares the
(e1, ..., ek) ordinals of the whole stream, tuple for tuple and in order, with the oracle's, and checks the path taken.
Inputs: 20 000 events or fewer, 3 streams, 50 keys or fewer."""
import ctypes
import functools
import struct

import numpy as np
import pytest

from oracle_lib import OracleApp

pytestmark = pytest.mark.gpu

NAMES = ["A", "B", "C"]
TYPES = ["INT", "DOUBLE", "LONG", "LONG"]
CM = "price > {p}.price - 25.0 and volume != e1.volume"


def text(pattern, keys=None, withins=None, select=None, kt="int", c1="[price>20]", cm=CM):
    """pattern: stream names in element order; keys {stream: key attribute} (None: unpartitioned); withins {m: T ms}
    on element m (1-based); cm: the condition of elements 2 .. k, {p} = the previous element."""
    withins = withins or {}
    k = len(pattern)
    schema = "".join(f"define stream {s} (symbol {kt}, price double, volume long, timestamp long); " for s in NAMES)
    els = [f"every e1={pattern[0]}{c1}"]
    for m in range(2, k + 1):
        w = f" within {withins[m]} milliseconds" if m in withins else ""
        els.append(f"e{m}={pattern[m - 1]}[{cm.format(p=f'e{m - 1}')}]{w}")
    sel = select or "select " + ", ".join(f"e{m}.timestamp as i{m}" for m in range(1, k + 1))
    q = f"@info(name='q') from {', '.join(els)} {sel} insert into OutputStream;"
    if keys is None:
        return schema + q
    return schema + "partition with (" + ", ".join(f"{a} of {s}" for s, a in keys.items()) + f") begin {q} end;"


def by_symbol(pattern):
    return {s: "symbol" for s in sorted(set(pattern))}


@functools.lru_cache(maxsize=None)
def events(n=20000, K=50, seed=1, pattern=None, heartbeats=0.1, noise=0.15):
    """Rows over A, B, C and heartbeat rows (-1). With a pattern: a key's rows mostly follow it in turn, so that long
    chains complete. The timestamp attribute is the row's position."""
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
    sid[rng.random(n) < heartbeats] = -1
    return sid, (sym, price, vol, np.arange(n, dtype=np.int64)), ts


def oracle_out(app_text, sid, cols, ts, ords=None):
    """ords None: an event's ordinal is its position in the feed, heartbeat rows counted, as on the device."""
    a = OracleApp(app_text)
    a.start()
    a.send_interleaved_ord(sid, ts, np.arange(len(ts), dtype=np.int64) if ords is None else ords, list(cols))
    out = a.outputs()
    a.close()
    return out


def tuples_of(out, k):
    return np.array([r[2] for r in out["streams"].get("OutputStream", [])], dtype=np.int64).reshape(-1, k)


class Run:
    """The product over the pieces `ranges` of an interleaved stream: the device tuples (global ordinals), the collected
    outputs, fast_path and nfa_state after every piece."""

    def __init__(self, app_text, **options):
        import torch
        from siddhi_amd.testing import ProductApp
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.app = ProductApp(app_text, **options)
        self.app.start()
        self.tuples, self.paths = [], []

    def piece(self, sid, cols, ts, lo, hi, ords=None):
        t = self.torch
        up = lambda a: t.from_numpy(np.ascontiguousarray(a[lo:hi])).to(self.dev)
        tsid, tts, tcols = up(sid), up(ts), [up(c) for c in cols]
        tord = None if ords is None else up(ords)
        base = lo if ords is None else int(ords[lo]) if hi > lo else 0
        t.cuda.synchronize()
        self.app.process_device_events(tsid, tts, tcols, ordinals=tord, ordinal_base=base)
        self.keep = (tsid, tts, tcols, tord)  # the batch stays resident for device_project
        self.paths.append(int(self.app.get_stat("fast_path:q")))
        got = self.app.device_matches_host("q").view(np.int32).astype(np.int64) + base
        self.tuples.append(got)
        return got

    def finish(self):
        state = int(self.app.get_stat("nfa_state:q"))
        out = self.app.outputs()
        self.app.close()
        return np.concatenate(self.tuples), out, state


def run(app_text, sid, cols, ts, ranges, ords=None, **options):
    r = Run(app_text, **options)
    for lo, hi in ranges:
        r.piece(sid, cols, ts, lo, hi, ords)
    tuples, out, state = r.finish()
    return tuples, out, r.paths, state


def cuts_inside_tuples(exp, n):
    """Three pieces, cut in front of the last member of one expected tuple and of the second member of another."""
    a = int(exp[len(exp) // 3, -1])
    b = int(exp[2 * len(exp) // 3, 1])
    assert 0 < a < b < n
    return [(0, a), (a, b), (b, n)]


def straddling(exp, ranges):
    los = np.array([lo for lo, _ in ranges[1:]], dtype=np.int64)
    piece = np.searchsorted(los, exp, side="right")
    return int((piece.min(axis=1) != piece.max(axis=1)).sum())


CHAINS = {2: ["A", "B"], 3: ["A", "B", "A"], 8: ["A", "B", "A", "A", "B", "C", "A", "B"]}


# ---- 1. batches

@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("k", [2, 3, 8])
def test_three_batches_cut_inside_tuples(k, keyed):
    pattern = CHAINS[k]
    sid, cols, ts = events(pattern=tuple(pattern) if k > 2 else None, K=50 if keyed else 1)
    t = text(pattern, by_symbol(pattern) if keyed else None, {k: 40})
    exp_out = oracle_out(t, sid, cols, ts)
    exp = tuples_of(exp_out, k)
    assert len(exp) > 20
    ranges = cuts_inside_tuples(exp, len(ts))
    assert straddling(exp, ranges) > 0
    got, out, paths, state = run(t, sid, cols, ts, ranges)
    assert paths == [8, 8, 8] and state == 0
    assert got.shape[1] == k
    np.testing.assert_array_equal(got, exp)
    assert out == exp_out  # values, timestamps, visible refs and order of the delivered events


def test_one_batch_and_many_small_ones():
    pattern = CHAINS[3]
    sid, cols, ts = events(pattern=tuple(pattern))
    t = text(pattern, by_symbol(pattern))
    exp = tuples_of(oracle_out(t, sid, cols, ts), 3)
    n = len(ts)
    got, _, paths, _ = run(t, sid, cols, ts, [(0, n)])
    assert paths == [8]
    np.testing.assert_array_equal(got, exp)
    ranges = [(lo, min(lo + 37, 3000)) for lo in range(0, 3000, 37)] + [(3000, n)]
    assert straddling(exp, ranges) > 50
    got, _, paths, _ = run(t, sid, cols, ts, ranges)
    assert set(paths) == {8}
    np.testing.assert_array_equal(got, exp)


# ---- 2. rows that must be ignored

@pytest.mark.parametrize("keyed", [True, False])
def test_heartbeats_and_unread_rows_between_members(keyed):
    """`A, B` with C rows and heartbeat rows in the feed: tuples whose members have such rows between them."""
    pattern = CHAINS[2]
    sid, cols, ts = events(K=50 if keyed else 1, heartbeats=0.3)
    t = text(pattern, by_symbol(pattern) if keyed else None)
    exp = tuples_of(oracle_out(t, sid, cols, ts), 2)
    between = [sid[a + 1:b] for a, b in exp]
    assert any((x == -1).any() for x in between) and any((x == 2).any() for x in between)
    if not keyed:
        assert all(((x == -1) | (x == 2)).all() for x in between)
    got, _, paths, _ = run(t, sid, cols, ts, cuts_inside_tuples(exp, len(ts)))
    assert paths == [8, 8, 8]
    np.testing.assert_array_equal(got, exp)


# ---- 3. degenerate batches

@pytest.mark.parametrize("keyed", [True, False])
def test_batches_without_and_with_few_read_rows(keyed):
    """A batch of C rows and heartbeats only, and batches with one read row (fewer than k), between two members of
    expected tuples: the carried rows wait."""
    pattern = CHAINS[3]
    sid, cols, ts = events(n=6000, K=5 if keyed else 1, pattern=tuple(pattern))
    sid, sym, vol = sid.copy(), cols[0].copy(), cols[2].copy()
    sid[2000:2600] = np.where(sid[2000:2600] == 2, 2, -1)   # no read row
    sid[2600:3200] = -1                                     # one read row in each of the next two pieces
    at = [1998, 1999, 2700, 3000]
    sid[at] = [0, 1, 0, 1]
    sym[at] = sym[1998]
    vol[at] = [5001, 5002, 5003, 5004]
    cols = (sym, cols[1], vol, cols[3])
    t = text(pattern, by_symbol(pattern) if keyed else None)
    exp = tuples_of(oracle_out(t, sid, cols, ts), 3)
    ranges = [(0, 2000), (2000, 2600), (2600, 2900), (2900, 3200), (3200, 6000)]
    assert [1998, 1999, 2700] in exp.tolist()  # two carried members wait through the batch without a read row
    got, _, paths, _ = run(t, sid, cols, ts, ranges)
    assert paths == [8] * 5
    np.testing.assert_array_equal(got, exp)


def unread_rows_going_back(sid, cols, ts, at, m=65):
    """The stream with m rows of stream C (which the callers' queries do not read) and heartbeats in front of row `at`:
    their event times decrease and lie before the stream's first. The timestamp attribute stays the row's position."""
    assert ts.min() > m
    usid = np.full(m, 2, np.int32)
    usid[::4] = -1
    uts = ts.min() - 1 - np.arange(m, dtype=np.int64)
    ins = lambda a, b: np.concatenate([a[:at], b.astype(a.dtype), a[at:]])
    sid = ins(sid, usid)
    cols = tuple(ins(c, c[:m]) for c in cols[:3]) + (np.arange(len(sid), dtype=np.int64),)
    return sid, cols, ins(ts, uts)


def oracle_on_read_rows(app_text, sid, cols, ts, read):
    """The oracle fed the rows of the streams `read` alone, each with its position in the whole stream as its ordinal."""
    rows = np.nonzero(np.isin(sid, read))[0]
    return oracle_out(app_text, sid[rows], [c[rows] for c in cols], ts[rows], rows.astype(np.int64))


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("k", [2, 3])
def test_unread_rows_going_back_in_time_between_members(k, keyed):
    """Three batches under a `within`: 1025 rows (one more than a tile), 65 rows that the query does not read, whose
    event times decrease and lie before the first batch's, and 1025 rows. The batch without a read row neither reports
    decreasing time nor moves the carried time: the third batch stays on the closed form, and tuples whose members lie
    on both sides of the middle batch come out as the oracle's on the read rows."""
    pattern = CHAINS[k]
    sid, cols, ts = events(n=2050, K=5 if keyed else 1, pattern=tuple(pattern), heartbeats=0.05)
    sid, sym, price, vol = sid.copy(), cols[0].copy(), cols[1].copy(), cols[2].copy()
    at = np.arange(1026 - k, 1026)  # one key's run of k rows on the pattern's streams, its last row behind the cut
    sid[at], sym[at], price[at], vol[at] = [NAMES.index(s) for s in pattern], sym[1025], 30.0, 5001 + np.arange(k)
    sid, cols, ts = unread_rows_going_back(sid, (sym, price, vol), ts + 1000, 1025)
    ranges = [(0, 1025), (1025, 1090), (1090, len(ts))]
    assert (np.diff(ts[1025:1090]) < 0).all() and ts[1025] < ts[0] and ts[1090] >= ts[1024]
    assert not np.isin(sid[1025:1090], [0, 1]).any()
    t = text(pattern, by_symbol(pattern) if keyed else None, {k: 40})
    exp = tuples_of(oracle_on_read_rows(t, sid, cols, ts, [0, 1]), k)
    across = straddling(exp, ranges)
    assert at[:-1].tolist() + [1090] in exp.tolist()
    assert across >= 1 and ((exp[:, 0] < 1025) & (exp[:, -1] >= 1090)).sum() == across
    got, _, paths, state = run(t, sid, cols, ts, ranges)
    assert paths == [8, 8, 8] and state == 0
    np.testing.assert_array_equal(got, exp)
    assert straddling(got, ranges) >= across


# ---- 4. tile edges, silent keys

def test_runs_cross_tile_edges_and_a_key_skips_a_batch():
    """Four keys over 9000 rows: every key's run crosses the 1024-row tiles of the sorted order many times. Key 3 has no
    row in the second batch: its carried rows, streams included, complete tuples in the third."""
    pattern = CHAINS[3]
    sid, cols, ts = events(n=9000, K=4, pattern=tuple(pattern), heartbeats=0.05)
    sid, vol = sid.copy(), cols[2].copy()
    sid[3000:6000][cols[0][3000:6000] == 3] = -1
    mine = np.nonzero((cols[0] == 3) & np.isin(sid, [0, 1]))[0]
    i1, i2 = mine[mine < 3000][-2:]
    i3 = mine[mine >= 6000][0]
    sid[[i1, i2, i3]] = [0, 1, 0]
    vol[[i1, i2, i3]] = [5001, 5002, 5003]
    cols = (cols[0], cols[1], vol, cols[3])
    t = text(pattern, by_symbol(pattern))
    exp = tuples_of(oracle_out(t, sid, cols, ts), 3)
    ranges = [(0, 3000), (3000, 6000), (6000, 9000)]
    assert [i1, i2, i3] in exp.tolist()
    order = np.argsort(np.where(np.isin(sid[:3000], [0, 1]), cols[0][:3000], 99), kind="stable")
    assert len({int(cols[0][order[1023]]), int(cols[0][order[1024]])}) == 1  # one key on both sides of a tile edge
    got, _, paths, _ = run(t, sid, cols, ts, ranges)
    assert paths == [8, 8, 8]
    np.testing.assert_array_equal(got, exp)


# ---- 5. keys and ordinals

def test_per_stream_key_attributes():
    """B's instances are keyed by its volume, A's by its symbol."""
    pattern = CHAINS[3]
    sid, cols, ts = events(K=20)
    cols = (cols[0], cols[1], cols[2] % 20, cols[3])
    t = text(pattern, {"A": "symbol", "B": "volume"}, cm="price > {p}.price - 25.0")
    exp = tuples_of(oracle_out(t, sid, cols, ts), 3)
    assert len(exp) > 20
    assert (cols[0][exp[:, 0]] == cols[2][exp[:, 1]]).all() and (cols[0][exp[:, 1]] != cols[2][exp[:, 1]]).any()
    got, _, paths, _ = run(t, sid, cols, ts, cuts_inside_tuples(exp, len(ts)))
    assert paths == [8, 8, 8]
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("remap", ["auto", "off", "on"])
def test_long_keys_negative_and_wide(remap):
    """LONG keys, negative values, a span above 2^20: dense ids by themselves (the first batch's span), the key values
    (option key_remap = 0: more sort passes), or dense ids from the start."""
    pattern = CHAINS[2]
    sid, cols, ts = events(K=40)
    sym = (cols[0].astype(np.int64) - 20) * 3_000_011
    assert sym.min() < 0 and sym.max() - sym.min() > 1 << 20
    cols = (sym, cols[1], cols[2], cols[3])
    t = text(pattern, by_symbol(pattern), kt="long")
    exp = tuples_of(oracle_out(t, sid, cols, ts), 2)
    assert len(exp) > 20
    opts = {} if remap == "auto" else {"key_remap": 1 if remap == "on" else 0}
    got, _, paths, _ = run(t, sid, cols, ts, cuts_inside_tuples(exp, len(ts)), **opts)
    assert paths == [8, 8, 8]
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("keyed", [True, False])
def test_given_ordinals(keyed):
    """Events carrying the global ordinals 3 i + 1, each piece's first ordinal as its base."""
    pattern = CHAINS[3]
    sid, cols, ts = events(pattern=tuple(pattern), K=50 if keyed else 1)
    ords = 3 * np.arange(len(ts), dtype=np.int64) + 1
    t = text(pattern, by_symbol(pattern) if keyed else None)
    exp = tuples_of(oracle_out(t, sid, cols, ts, ords), 3)
    assert len(exp) > 20 and (exp % 3 == 1).all()
    ranges = cuts_inside_tuples((exp - 1) // 3, len(ts))
    got, _, paths, _ = run(t, sid, cols, ts, ranges, ords=ords)
    assert paths == [8, 8, 8]
    np.testing.assert_array_equal(got, exp)


# ---- 6. hand-over to the NFA kernel

def decreasing(ts, case):
    ts = ts.copy()
    if case == "inside":
        ts[9000:9400] = ts[9000:9400][::-1]   # event time runs backwards inside the second piece
    else:
        ts[8000:] -= 50                       # the second piece starts before the first one's last event
    assert (np.diff(ts) < 0).any()
    return ts


RANGES3 = [(0, 8000), (8000, 14000), (14000, 20000)]


@pytest.mark.parametrize("case", ["inside", "before_carry"])
@pytest.mark.parametrize("keyed", [True, False])
def test_decreasing_time_with_within_hands_over(case, keyed):
    pattern = CHAINS[3]
    sid, cols, ts = events(pattern=tuple(pattern), K=50 if keyed else 1)
    ts = decreasing(ts, case)
    t = text(pattern, by_symbol(pattern) if keyed else None, {3: 30})
    exp_out = oracle_out(t, sid, cols, ts)
    exp = tuples_of(exp_out, 3)
    assert len(exp) > 20 and straddling(exp, RANGES3) > 0
    got, out, paths, state = run(t, sid, cols, ts, RANGES3)
    assert paths == [8, 5, 5] and state == 1  # handed over at the first such batch, for good
    np.testing.assert_array_equal(got, exp)
    assert out == exp_out


@pytest.mark.parametrize("case", ["inside", "before_carry"])
@pytest.mark.parametrize("keyed", [True, False])
def test_decreasing_time_without_within_stays(case, keyed):
    pattern = CHAINS[3]
    sid, cols, ts = events(pattern=tuple(pattern), K=50 if keyed else 1)
    ts = decreasing(ts, case)
    t = text(pattern, by_symbol(pattern) if keyed else None)
    exp = tuples_of(oracle_out(t, sid, cols, ts), 3)
    assert len(exp) > 20
    got, _, paths, state = run(t, sid, cols, ts, RANGES3)
    assert paths == [8, 8, 8] and state == 0
    np.testing.assert_array_equal(got, exp)


def send_rows(app, sid, cols, ts, lo, hi):
    for i in range(lo, hi):
        if sid[i] >= 0:
            app.send(NAMES[sid[i]], int(ts[i]), [int(cols[0][i]), float(cols[1][i]), int(cols[2][i]), int(cols[3][i])],
                     TYPES)


@pytest.mark.parametrize("keyed", [True, False])
def test_staged_sends_before_and_after_device_events(keyed):
    """Staged host events first: the NFA kernel holds the state and the device events run on it (path 5, nfa_state 1).
    Device events first (path 8), then staged events: the flush replays the carried rows on their own streams into the
    NFA, which keeps the query. Both ways the whole stream's outputs are the oracle's."""
    pattern = CHAINS[3]
    sid, cols, ts = events(n=6000, pattern=tuple(pattern), K=10 if keyed else 1, heartbeats=0.0)
    t = text(pattern, by_symbol(pattern) if keyed else None)
    exp_out = oracle_out(t, sid, cols, ts)
    exp = tuples_of(exp_out, 3)
    n = len(ts)
    # staged, then device
    r = Run(t)
    send_rows(r.app, sid, cols, ts, 0, 40)
    tail = r.piece(sid, cols, ts, 40, n)
    assert r.paths == [5] and r.app.get_stat("match_arity:q") == 3
    _, out, state = r.finish()
    assert state == 1 and out == exp_out
    np.testing.assert_array_equal(tail, exp[exp[:, 2] >= 40])
    assert ((exp[:, 0] < 40) & (exp[:, 2] >= 40)).any()
    # device, staged, device
    a = next(int(e2) for _, e2, e3 in exp[len(exp) // 2:] if e3 < e2 + 40)  # in front of a tuple's second member
    b = a + 40
    assert ((exp[:, 0] < a) & (exp[:, 2] >= a) & (exp[:, 2] < b)).any()  # a handed-over row completes
    r = Run(t)
    first = r.piece(sid, cols, ts, 0, a)
    assert r.paths == [8] and r.app.get_stat("nfa_state:q") == 0
    send_rows(r.app, sid, cols, ts, a, b)
    r.app.flush()
    assert r.app.get_stat("nfa_state:q") == 1
    last = r.piece(sid, cols, ts, b, n)
    assert r.paths == [8, 5]
    _, out, state = r.finish()
    assert state == 1 and out == exp_out
    np.testing.assert_array_equal(first, exp[exp[:, 2] < a])
    np.testing.assert_array_equal(last, exp[exp[:, 2] >= b])


# ---- 7. snapshot

@pytest.mark.parametrize("keyed", [True, False])
def test_snapshot_restore_between_two_members(keyed):
    pattern = CHAINS[3]
    sid, cols, ts = events(pattern=tuple(pattern), K=50 if keyed else 1)
    t = text(pattern, by_symbol(pattern) if keyed else None)
    exp = tuples_of(oracle_out(t, sid, cols, ts), 3)
    # between e1 and e2 of an expected tuple and, keyed, between e2 and e3 of another key's (unkeyed, two tuples that
    # overlap share one row, `A, B, A`: no cut lies inside both in that way)
    cut = next(int(c) for c in exp[len(exp) // 2:, 1]
               if ((exp[:, 0] < c) & (exp[:, 1] >= c)).any() and
               (not keyed or ((exp[:, 1] < c) & (exp[:, 2] >= c)).any()))
    a = Run(t)
    first = a.piece(sid, cols, ts, 0, cut)
    snap = a.app.snapshot()
    a.app.close()
    b = Run(t)
    b.app.restore(snap)
    second = b.piece(sid, cols, ts, cut, len(ts))
    b.app.close()
    assert a.paths == [8] and b.paths == [8]
    np.testing.assert_array_equal(np.concatenate([first, second]), exp)


# ---- 8. outputs and stats

PSELECT = ("select e1.symbol as k, e1.price as p1, e2.price as p2, e3.price as p3, e3.volume - e1.volume as dv, "
           "e1.timestamp as i1, e2.timestamp as i2, e3.timestamp as i3")
PKINDS = ["i", "d", "d", "d", "i", "i", "i", "i"]


def words(row):
    return [struct.unpack("<q", struct.pack("<d", v))[0] if k == "d" else int(v) for v, k in zip(row, PKINDS)]


@pytest.mark.parametrize("keyed", [True, False])
def test_device_project_equals_oracle(keyed):
    pattern = CHAINS[3]
    sid, cols, ts = events(pattern=tuple(pattern), K=50 if keyed else 1)
    t = text(pattern, by_symbol(pattern) if keyed else None, select=PSELECT)
    rows = oracle_out(t, sid, cols, ts)["streams"]["OutputStream"]
    tuples = np.array([r[1][5:8] for r in rows], dtype=np.int64)
    ranges = cuts_inside_tuples(tuples, len(ts))
    los = [lo for lo, _ in ranges[1:]]
    # outputs whose first member, and whose first two members, are read from the carry
    assert any(((tuples[:, 0] < lo) & (tuples[:, 1] >= lo)).any() for lo in los)
    assert any(((tuples[:, 1] < lo) & (tuples[:, 2] >= lo)).any() for lo in los)
    r = Run(t)
    got = []
    for lo, hi in ranges:
        r.piece(sid, cols, ts, lo, hi)
        assert r.app.get_stat("match_arity:q") == 3
        vals, nulls, ots = r.app.device_project("q")
        r.torch.cuda.synchronize()
        assert not nulls.any()
        got += [[t_, v] for t_, v in zip(ots.cpu().tolist(), vals.cpu().tolist())]
    assert r.paths == [8, 8, 8]
    r.app.close()
    assert got == [[row[0], words(row[1])] for row in rows]


def test_callbacks_receive_the_oracles_events():
    """A StreamCallback and a columns callback through SiddhiAppRuntime.sendDeviceEvents: one call per last event, in
    order of it, before the call returns."""
    import torch
    import siddhi_amd
    from siddhi_amd import ColumnsStreamCallback, SiddhiManager, StreamCallback
    pattern = CHAINS[3]
    sid, cols, ts = events(pattern=tuple(pattern), K=50)
    t = text(pattern, by_symbol(pattern), select=PSELECT)
    rows = oracle_out(t, sid, cols, ts)["streams"]["OutputStream"]
    assert len(rows) > 100
    tuples = np.array([r[1][5:8] for r in rows], dtype=np.int64)
    ranges = cuts_inside_tuples(tuples, len(ts))
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
            assert v.value == 8
            seen.append(len(evs) + len(columns))
        rt.shutdown()
    assert evs == [[[r[0], r[1]]] for r in rows]
    assert columns == [[[r[0]], [words(r[1])], [0]] for r in rows]
    assert seen[0] == int((tuples[:, 2] < ranges[0][1]).sum())  # delivered before the call returned


def test_match_arity_and_timing_labels():
    pattern = CHAINS[3]
    sid, cols, ts = events(pattern=tuple(pattern), K=50)
    n = len(ts)
    r = Run(text(pattern, by_symbol(pattern)), fast_timing=1)
    assert r.app.get_stat("match_arity:q") == 3
    r.piece(sid, cols, ts, 0, n // 2)
    labels = ["mseq_facts", "mseq_pack", "mseq_sort", "mseq_link", "mseq_count", "mseq_scan", "mseq_emit", "mseq_carry"]
    for label in labels:
        assert r.app.get_stat(f"kernel_calls:{label}") == 1
        assert r.app.get_stat(f"kernel_ms:{label}") >= 0
    assert r.app.get_stat("kernel_calls:mseq_keep") == 0 and r.app.get_stat("kernel_calls:seqk_link") == 0
    r.piece(sid, cols, ts, n // 2, n)
    for label in labels + ["mseq_keep"]:
        assert r.app.get_stat(f"kernel_calls:{label}") == 1
    assert r.paths == [8, 8]
    r.app.close()
    for k in (2, 8):
        q = Run(text(CHAINS[k]))
        assert q.app.get_stat("match_arity:q") == k
        q.app.close()
    u = Run(text(CHAINS[2]), fast_timing=1)  # unkeyed, every row read: no pack, no sort
    sid2 = np.where(sid == 0, 0, 1).astype(np.int32)
    u.piece(sid2, cols, ts, 0, n)
    assert u.paths == [8]
    assert u.app.get_stat("kernel_calls:mseq_pack") == 0 and u.app.get_stat("kernel_calls:mseq_sort") == 0
    assert u.app.get_stat("kernel_calls:mseq_link") == 1
    np.testing.assert_array_equal(u.tuples[0], tuples_of(oracle_out(text(CHAINS[2]), sid2, cols, ts), 2))
    u.app.close()


# ---- 9. unchanged routing

@pytest.mark.parametrize("k", [2, 3])
def test_same_stream_sequences_keep_their_route(k):
    """`every e1=A, e2=A [, e3=A]` through sm_app_process_device_events runs on the NFA kernel as before: fast_path is
    what it was (0: no closed form ran), the outputs are the oracle's."""
    pattern = ["A"] * k
    sid, cols, ts = events(n=6000, K=10)
    t = text(pattern, by_symbol(pattern))
    exp_out = oracle_out(t, sid, cols, ts)
    assert len(exp_out["streams"]["OutputStream"]) > 20
    r = Run(t)
    r.app.process_device_events(*[r.torch.from_numpy(np.ascontiguousarray(a)).to(r.dev) for a in (sid, ts)],
                                [r.torch.from_numpy(np.ascontiguousarray(c)).to(r.dev) for c in cols])
    assert r.app.get_stat("fast_path:q") == 0 and r.app.get_stat("nfa_state:q") == 0
    out = r.app.outputs()
    r.app.close()
    assert out == exp_out
