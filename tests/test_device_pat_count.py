"""The closed form of the count pattern `every e1=A[c1] -> e2=B[c2]<m:n> -> e3=C[c3] within T` (three different streams of
one schema) on interleaved device batches (sm_app_process_device_events, fast_path 14: kernels/seqpath.hip fast_pat_count,
mpat_count_dev.h) against the CPU oracle fed the same events. Every A row passing c1 binds the first n later B rows of its
partition instance passing c2; once it holds m, the first C row beyond T of the hit bound last kills it and the first one
inside T passing c3 completes it; the product carries the open partials and the events they hold across batches. Every
case compares the (e1, e2[0] .. e2[n-1], e3) ordinals of the whole stream (-1: a hit slot that is not bound), tuple for
tuple and in order, with the oracle's, and the delivered events (values, nulls, timestamps, order), checks the path taken,
and asserts a floor of expected outputs that the oracle alone reaches. Inputs: 4000 rows, 3 streams and heartbeat rows, 20
keys or fewer; hand-built single-key streams of a few hundred rows."""
import ctypes
import struct

import numpy as np
import pytest

from test_device_mseq import NAMES, Run, events, oracle_out, send_rows, straddling, tuples_of
from test_pat_count_emu import EDGES, FAIL, FILL, HIT, PASS, feed, single

pytestmark = pytest.mark.gpu

T_KEYED, T_FLAT = 150, 10  # ms: about eight rows of a key out of 20, about ten rows of the flat stream
N = 4000
COUNTS = {"2_4": ("<2:4>", 2, 4), "2_2": ("<2:2>", 2, 2), "0_3": ("<0:3>", 0, 3), "1_1": ("<1:1>", 1, 1),
          "opt": ("<0:1>", 0, 1), "2_6": ("<2:6>", 2, 6)}
BY_SYMBOL = {"A": "symbol", "B": "symbol", "C": "symbol"}
PER_STREAM = {"A": "symbol", "B": "volume", "C": "symbol"}


def text(count, a="A", b="B", c="C", keys=None, within=T_KEYED, c2="price > e1.price", c3="price < e1.price", select=None,
         kt="int", c1="[price>20]", names=NAMES):
    n = COUNTS[count][2]
    schema = "".join(f"define stream {s} (symbol {kt}, price double, volume long, timestamp long); " for s in names)
    w = "" if within is None else f" within {within} milliseconds"
    sel = select or ("select e1.timestamp as i1, " + ", ".join(f"e2[{k}].timestamp as h{k}" for k in range(n)) +
                     ", e3.timestamp as i3")
    q = (f"@info(name='q') from every e1={a}{c1} -> e2={b}[{c2}]{COUNTS[count][0]} -> e3={c}[{c3}]{w} {sel} "
         "insert into OutputStream;")
    if keys is None:
        return schema + q
    return schema + "partition with (" + ", ".join(f"{x} of {s}" for s, x in keys.items()) + f") begin {q} end;"


def case(count, kind, K=20, n=N, **kw):
    """(text, sid, cols, ts) of a form: flat, keyed by symbol, or B keyed by its volume."""
    if kind == "flat":
        sid, cols, ts = events(n=n, K=1)
        return text(count, keys=None, **dict({"within": T_FLAT}, **kw)), sid, cols, ts
    sid, cols, ts = events(n=n, K=K)
    if kind == "per_stream":
        cols = (cols[0], cols[1], cols[2] % K, cols[3])
        return text(count, keys=PER_STREAM, **kw), sid, cols, ts
    return text(count, keys=BY_SYMBOL, **kw), sid, cols, ts


def nulls_out(got):
    """Run.piece() adds the piece's base to every word: the null word (-2^31) stays far below 0, a global ordinal never."""
    return np.where(got < 0, -1, got)


def run(app_text, sid, cols, ts, ranges, ords=None, **options):
    r = Run(app_text, **options)
    for lo, hi in ranges:
        r.piece(sid, cols, ts, lo, hi, ords)
    tuples, out, state = r.finish()
    return nulls_out(tuples), out, r.paths, state


def check(t, sid, cols, ts, ranges, w, floor=30, ords=None, **options):
    exp_out = oracle_out(t, sid, cols, ts, ords)
    exp = tuples_of(exp_out, w)
    assert len(exp) >= floor, len(exp)
    got, out, paths, state = run(t, sid, cols, ts, ranges, ords=ords, **options)
    assert set(paths) == {14} and state == 0
    assert got.shape[1] == w
    np.testing.assert_array_equal(got, exp)
    assert out == exp_out  # values (null ones too), timestamps, visible refs and order of the delivered events
    return exp


def cuts_for(exp, m, n, total):
    """Three cuts at arbitrary-looking rows that are chosen from expected tuples: between two hits of a partial (it is
    carried below m hits when m >= 2), between the m-th hit and e3 (carried in e3), and in front of the e3 of a tuple that
    holds n hits (carried full). Returns (ranges, the kinds of carried partial the cuts make)."""
    cuts, kinds = set(), set()
    hits = (exp[:, 1:-1] >= 0).sum(axis=1)
    if n >= 2:
        two = exp[(hits >= 2) & (exp[:, 2] - exp[:, 1] > 1)]
        if len(two):
            x = two[len(two) // 4]
            cuts.add(int(x[2]))
            kinds.add("below" if m >= 2 else "between_hits")
    if m >= 1:
        far = exp[(hits >= m) & (exp[:, -1] - exp[:, m] > 1)]
        if len(far):
            x = far[len(far) // 2]
            cuts.add(int(x[-1]))
            kinds.add("in_e3")
    full = exp[(hits == n) & (exp[:, -1] - exp[:, n] > 1)]
    if len(full):
        x = full[3 * len(full) // 4]
        cuts.add(int(x[-1]))
        kinds.add("full")
    if len(cuts) < 2:  # (m = 0 or n = 1 leave fewer kinds) a tile's edge plus one
        cuts |= {1025, 2049}
    cuts = sorted(c for c in cuts if 0 < c < total)
    return list(zip([0] + cuts, cuts + [total])), kinds


# ---- 1. batches

@pytest.mark.parametrize("within", ["short", "long"])
@pytest.mark.parametrize("kind", ["flat", "symbol", "per_stream"])
@pytest.mark.parametrize("count", ["2_4", "2_2", "0_3", "1_1", "opt"])
def test_one_batch_and_three_pieces(count, kind, within):
    """`fast_path:q` is 14 with `nfa_state` 0 (0 and 1 on the parent commit: the NFA kernel). One batch; then pieces cut
    between a partial's hits, between its m-th hit and its e3, and in front of the e3 of a full one."""
    _, m, n = COUNTS[count]
    kw = {} if within == "short" else {"within": 4 * (T_FLAT if kind == "flat" else T_KEYED)}
    t, sid, cols, ts = case(count, kind, **kw)
    total = len(ts)
    exp = check(t, sid, cols, ts, [(0, total)], n + 2)
    ranges, kinds = cuts_for(exp, m, n, total)
    assert len(ranges) >= 3 and kinds >= {"full"} | ({"in_e3"} if m else set()) | ({"below"} if m >= 2 else set()), kinds
    assert straddling(exp[:, [0, -1]], ranges) >= 2
    check(t, sid, cols, ts, ranges, n + 2)


@pytest.mark.parametrize("keyed", [True, False])
def test_pieces_of_1_and_37_rows(keyed):
    t, sid, cols, ts = case("2_4", "symbol" if keyed else "flat", K=5)
    n = len(ts)
    ranges = [(lo, min(lo + 37, 1850)) for lo in range(0, 1850, 37)] + [(lo, lo + 1) for lo in range(1850, 2050)] + [(2050, n)]
    exp = check(t, sid, cols, ts, ranges, 6)
    assert straddling(exp[:, [0, -1]], ranges) >= 20


@pytest.mark.parametrize("keyed", [True, False])
def test_six_hit_slots(keyed):
    """n = 6: tuples of eight words."""
    t, sid, cols, ts = case("2_6", "symbol" if keyed else "flat", **({} if keyed else {"within": 40}))
    exp = check(t, sid, cols, ts, [(0, len(ts))], 8)
    assert ((exp[:, 1:-1] >= 0).sum(axis=1) == 6).sum() >= 3
    ranges, kinds = cuts_for(exp, 2, 6, len(ts))
    assert len(ranges) >= 3
    check(t, sid, cols, ts, ranges, 8)


# ---- 2. the private budget and the wave step, on one key

def hand(rows, keyed, cuts=(), count="2_4", within=40, floor=0):
    """A hand-built stream of one key through the oracle and the product: its expected tuples."""
    sid, sym, price, vol, ts = feed(rows, 1)
    cols = (sym, price, vol, np.arange(len(sid), dtype=np.int64))
    t = text(count, keys=BY_SYMBOL if keyed else None, within=within)
    cuts = sorted(c for c in cuts if 0 < c < len(sid))
    return check(t, sid, cols, ts, list(zip([0] + cuts, cuts + [len(sid)])), COUNTS[count][2] + 2, floor=floor)


@pytest.mark.parametrize("keyed", [True, False])
def test_hits_at_the_budgets_and_the_wave_steps_edges(keyed):
    """Hits at 15, 16, 17 and 63, 64, 65 positions past the e1 (the lane's own budget is 16 positions, a wave step 64), the
    passing C row right behind: n hits and the deciding row inside one step. One stream holds the cases one after
    another, each e1 done before the next begins; then the same with cuts between the hits."""
    rows = []
    starts = []
    for d in EDGES:
        starts.append(len(rows))
        ev = {d + q: HIT for q in range(4)}
        ev[d + 4] = PASS
        rows += single(ev, d + 6)
    exp = hand(rows, keyed, floor=len(EDGES))
    assert exp[:, 0].tolist() == starts
    assert ((exp[:, 1:5] - exp[:, :1]) == [[d, d + 1, d + 2, d + 3] for d in EDGES]).all()
    hand(rows, keyed, cuts=[starts[1] + 17, starts[3] + 2, starts[4] + 66, starts[5] + 69], floor=len(EDGES))


@pytest.mark.parametrize("keyed", [True, False])
def test_death_and_revival_cases(keyed):
    """A dying C row and a passing C row in one step, in both orders; a hit behind a death (no revival); a C row passing
    c3 in front of the m-th hit (ignored). Event time only grows along the stream: every case starts later."""
    rows, want = [], []
    t0 = 100

    def add(ev, last, emits):
        nonlocal t0
        base = len(rows)
        ev = {g: (e[0], e[1], t0 + (e[2] if len(e) > 2 else 0)) for g, e in ev.items()}
        rows.extend(single(ev, last, t=t0))
        if emits is not None:
            want.append(base + emits)
        t0 = rows[-1][2] + 5000

    for d in (16, 64, 100):
        add({1: HIT, 2: HIT, d + 3: FAIL + (1000,), d + 4: PASS + (1000,)}, d + 6, None)   # dies, then would pass
        add({1: HIT, 2: HIT, d + 3: PASS, d + 4: FAIL + (1000,)}, d + 6, d + 3)            # passes, then would die
        add({1: HIT, 2: HIT, d + 3: FAIL + (1000,), d + 4: HIT + (1000,), d + 5: PASS + (1000,)}, d + 6, None)
        add({1: HIT, 2: PASS + (1000,), d + 3: HIT + (1000,), d + 4: PASS + (1000,)}, d + 6, d + 4)
    exp = hand(rows, keyed, floor=6)
    assert exp[:, -1].tolist() == want


@pytest.mark.parametrize("keyed", [True, False])
def test_one_row_completes_two_partials_in_order_of_p(keyed):
    """`<1:1>`: the first e1 (price 50) takes its hit late (a B row of 55), the second (price 30) early (40): one C row
    completes both, and the second comes out first. In one batch, and with both carried."""
    rows = [(0, 50.0, 100), (0, 30.0, 100), (1, 40.0, 100), (1, 55.0, 100), (2, 25.0, 100)]
    exp = hand(rows, keyed, count="1_1", floor=2)
    assert exp.tolist() == [[1, 2, 4], [0, 3, 4]]
    hand(rows, keyed, cuts=[4], count="1_1", floor=2)
    hand(rows, keyed, cuts=[3], count="1_1", floor=2)


# ---- 3. keys, ordinals, other streams

def test_an_unread_keyed_stream_and_another_assignment():
    """Four streams: the query reads (C, A, B); rows of D are keyed by the partition and not read."""
    names = ["A", "B", "C", "D"]
    sid, cols, ts = events(n=N, K=20)
    sid = sid.copy()
    sid[(np.arange(N) % 7 == 3) & (sid >= 0)] = 3
    keys = {s: "symbol" for s in names}
    t = text("2_4", "C", "A", "B", keys=keys, names=names)
    exp = tuples_of(oracle_out(t, sid, cols, ts), 6)
    ranges, _ = cuts_for(exp, 2, 4, len(ts))
    check(t, sid, cols, ts, ranges, 6)


@pytest.mark.parametrize("remap", ["auto", "off", "on"])
def test_long_keys_negative_and_wide(remap):
    sid, cols, ts = events(n=N, K=20)
    sym = (cols[0].astype(np.int64) - 10) * 3_000_011
    assert sym.min() < 0 and sym.max() - sym.min() > 1 << 20
    cols = (sym, cols[1], cols[2], cols[3])
    t = text("2_4", keys=BY_SYMBOL, kt="long")
    exp = tuples_of(oracle_out(t, sid, cols, ts), 6)
    opts = {} if remap == "auto" else {"key_remap": 1 if remap == "on" else 0}
    check(t, sid, cols, ts, cuts_for(exp, 2, 4, len(ts))[0], 6, **opts)


@pytest.mark.parametrize("keyed", [True, False])
def test_given_ordinals_with_gaps(keyed):
    """Rows carrying the global ordinals 3 i + 1, each piece's first ordinal as its base."""
    t, sid, cols, ts = case("2_4", "symbol" if keyed else "flat")
    ords = 3 * np.arange(len(ts), dtype=np.int64) + 1
    exp = tuples_of(oracle_out(t, sid, cols, ts, ords), 6)
    assert ((exp % 3 == 1) | (exp < 0)).all()
    check(t, sid, cols, ts, cuts_for(np.where(exp < 0, -1, (exp - 1) // 3), 2, 4, len(ts))[0], 6, ords=ords)


# ---- 4. hand-over to the NFA kernel

def small(keyed):
    """3000 rows whose c1 leaves few partials open: unkeyed, the NFA kernel's one lane walks every one of them."""
    sid, cols, ts = events(n=3000, K=10 if keyed else 1, heartbeats=0.0)
    return sid, cols, ts, dict(keys=BY_SYMBOL if keyed else None, c1="[price>20]" if keyed else "[price>48]")


@pytest.mark.parametrize("case_", ["inside", "before_carry"])
@pytest.mark.parametrize("keyed", [True, False])
def test_decreasing_time_hands_over(case_, keyed):
    """Event time decreases inside the second piece, or from the first piece to the second: FAST_NON_MONOTONE, the NFA
    kernel takes the query over for good with the carried partials, ones holding hits among them."""
    sid, cols, ts, kw = small(keyed)
    t = text("2_4", within=30000, **kw)
    exp0 = tuples_of(oracle_out(t, sid, cols, ts), 6)
    far = exp0[exp0[:, -1] - exp0[:, 2] > 1]
    c1 = int(far[len(far) // 3, -1])
    c2 = int(far[far[:, -1] > c1 + 300][0, -1])
    ranges = [(0, c1), (c1, c2), (c2, len(ts))]
    ts = ts.copy()
    if case_ == "inside":
        ts[c1 + 50:c1 + 250] = ts[c1 + 50:c1 + 250][::-1]
    else:
        ts[c1:] -= 50
    assert (np.diff(ts) < 0).any()
    exp_out = oracle_out(t, sid, cols, ts)
    exp = tuples_of(exp_out, 6)
    assert len(exp) >= 30 and straddling(exp[:, [0, -1]], ranges) >= 2
    assert ((exp[:, 2] >= 0) & (exp[:, 2] < c1) & (exp[:, -1] >= c1)).sum() >= 1  # carried with two hits at the hand-over
    got, out, paths, state = run(t, sid, cols, ts, ranges)
    assert paths == [14, 5, 5] and state == 1
    np.testing.assert_array_equal(got, exp)
    assert out == exp_out


@pytest.mark.parametrize("keyed", [True, False])
def test_staged_sends_before_and_after_device_events(keyed):
    sid, cols, ts, kw = small(keyed)
    t = text("2_4", within=40, **kw)
    exp_out = oracle_out(t, sid, cols, ts)
    exp = tuples_of(exp_out, 6)
    n = len(ts)
    assert len(exp) >= 30
    # staged, then device: the NFA kernel holds the state
    r = Run(t)
    send_rows(r.app, sid, cols, ts, 0, 40)
    tail = nulls_out(r.piece(sid, cols, ts, 40, n))
    assert r.paths == [5] and r.app.get_stat("match_arity:q") == 6
    _, out, state = r.finish()
    assert state == 1 and out == exp_out
    np.testing.assert_array_equal(tail, exp[exp[:, -1] >= 40])
    # device, staged, device: the flush replays the carried events into the NFA, which keeps the query
    x = next(x for x in exp[len(exp) // 2:] if x[2] >= 0 and x[-1] - x[2] > 1)  # in front of the e3 of a tuple with hits
    a = int(x[-1])
    b = a + 40
    assert ((exp[:, 0] < a) & (exp[:, -1] >= a) & (exp[:, -1] < b)).any()  # a handed-over partial completes
    r = Run(t)
    first = nulls_out(r.piece(sid, cols, ts, 0, a))
    assert r.paths == [14] and r.app.get_stat("nfa_state:q") == 0
    send_rows(r.app, sid, cols, ts, a, b)
    r.app.flush()
    assert r.app.get_stat("nfa_state:q") == 1
    last = nulls_out(r.piece(sid, cols, ts, b, n))
    assert r.paths == [14, 5]
    _, out, state = r.finish()
    assert state == 1 and out == exp_out
    np.testing.assert_array_equal(first, exp[exp[:, -1] < a])
    np.testing.assert_array_equal(last, exp[exp[:, -1] >= b])


def test_the_carry_cap_hands_over():
    """`<2:6>` keyed: a batch of n rows may leave n + slack / bytes-per-partial open partials (fastpath.h pcnt_carry_cap:
    the scratch's constant 64 MiB at (n + 1) events of 8 cw + 44 bytes and a row of n + 5 words per partial, cw = 8 for
    four attributes). 90,000 A rows of as many keys and no B row leave as many partials below m hits, which no window
    ends: their own batch may leave them, the next batch of 3150 rows may not: FAST_OUTSIDE once the partials are
    counted and before anything changes, and the NFA kernel takes the query over with the carried partials and events,
    some of which then complete."""
    n, big = 6, 90_000
    extra = (64 << 20) // ((n + 1) * (8 * 8 + 44) + 8 * (n + 5))
    sid0, cols0, ts0 = events(n=N, K=20)
    done = 50  # of the big keys, completed in the last piece: two hits and a drop each
    tail_sid = np.tile(np.array([1, 1, 2], np.int32), done)
    tail_sym = 1000 + np.repeat(np.arange(done, dtype=np.int32), 3)
    tail_price = np.tile(np.array([40.0, 41.0, 25.0]), done)
    sid = np.concatenate([sid0[:1000], np.zeros(big, np.int32), sid0[1000:], tail_sid])
    sym = np.concatenate([cols0[0][:1000], 1000 + np.arange(big, dtype=np.int32), cols0[0][1000:], tail_sym])
    price = np.concatenate([cols0[1][:1000], np.full(big, 30.0), cols0[1][1000:], tail_price])
    vol = np.concatenate([cols0[2][:1000], np.zeros(big, np.int64), cols0[2][1000:], np.zeros(3 * done, np.int64)])
    ts = np.concatenate([ts0[:1000], np.full(big, ts0[999]), ts0[1000:], np.full(3 * done, ts0[-1])])
    total = len(sid)
    cols = (sym, price, vol, np.arange(total, dtype=np.int64))
    ranges = [(0, 1000), (1000, 1000 + big), (1000 + big, total)]
    assert big <= big + extra and big > (total - 1000 - big) + extra  # the second piece fits its cap, the third does not
    t = text("2_6", keys=BY_SYMBOL)
    exp_out = oracle_out(t, sid, cols, ts)
    exp = tuples_of(exp_out, 8)
    assert ((exp[:, 0] >= 1000) & (exp[:, 0] < 1000 + done) & (exp[:, -1] >= total - 3 * done)).sum() == done
    assert ((exp[:, 0] < 1000) & (exp[:, -1] >= 1000 + big)).sum() >= 1 and len(exp) >= 100
    got, out, paths, state = run(t, sid, cols, ts, ranges)
    assert paths == [14, 14, 5] and state == 1
    np.testing.assert_array_equal(got, exp)
    assert out == exp_out


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
    "keep_outputs": (dict(within=40), dict(keep_outputs=1), BY_SYMBOL),
    "no_within": (dict(within=None, c1="[price>55]"), {}, BY_SYMBOL),
    "b_is_c": (dict(within=80, c="B"), {}, {"A": "symbol", "B": "symbol"}),
    "a_is_b": (dict(within=40, b="A"), {}, {"A": "symbol", "C": "symbol"}),
    "unbounded": (dict(within=40), {}, BY_SYMBOL),
}


@pytest.mark.parametrize("which", list(STAY))
def test_texts_that_stay_on_the_nfa_route(which):
    """What ran on the NFA kernel before runs there as before, with the oracle's outputs, and `fast_path:q` stays 0."""
    sid, cols, ts = events(n=3000, K=10, heartbeats=0.0)
    ranges = [(0, 1300), (1300, 3000)]
    kw, opts, keys = STAY[which]
    t = text("2_4", keys=keys, **kw)
    if which == "unbounded":
        t = t.replace("<2:4>", "<2:>")
    exp_out = oracle_out(t, sid, cols, ts)
    assert len(exp_out["streams"]["OutputStream"]) >= 30
    out, paths = feed_pieces(t, sid, cols, ts, ranges, **opts)
    assert paths == [0, 0] and out == exp_out


# ---- 5. snapshot

@pytest.mark.parametrize("keyed", [True, False])
def test_snapshot_restore_mid_stream(keyed):
    """Between the second hit of a partial and its e3."""
    t, sid, cols, ts = case("2_4", "symbol" if keyed else "flat", **({} if keyed else {"within": 40}))
    exp = tuples_of(oracle_out(t, sid, cols, ts), 6)
    far = exp[exp[:, -1] - exp[:, 2] > 1]
    cut = int(far[len(far) // 4, -1])
    assert ((exp[:, 2] >= 0) & (exp[:, 2] < cut) & (exp[:, -1] >= cut)).sum() >= 1 and len(exp) >= 30
    a = Run(t)
    first = nulls_out(a.piece(sid, cols, ts, 0, cut))
    snap = a.app.snapshot()
    a.app.close()
    b = Run(t)
    b.app.restore(snap)
    second = nulls_out(b.piece(sid, cols, ts, cut, len(ts)))
    b.app.close()
    assert a.paths == [14] and b.paths == [14]
    np.testing.assert_array_equal(np.concatenate([first, second]), exp)


# ---- 6. outputs and stats

PSELECT = ("select e1.symbol as k, e1.price as p1, e2[0].price as p20, e2[1].price as p21, e2[last].price as p2l, "
           "e3.price as p3, e3.volume - e1.volume as dv, e1.timestamp as i1")
PKINDS = ["i", "d", "d", "d", "d", "d", "i", "i"]
# the positions of e1, e2[0], e2[1], e2[2] and e3: the second select of the projection tests, for the cuts
ISELECT = "select e1.timestamp as i1, e2[0].timestamp as h0, e2[1].timestamp as h1, e2[2].timestamp as h2, e3.timestamp as i3"


def words(row):
    """(values with 0 for a null one, null flags)."""
    vals = [0 if v is None else struct.unpack("<q", struct.pack("<d", v))[0] if k == "d" else int(v)
            for v, k in zip(row, PKINDS)]
    return vals, [v is None for v in row]


@pytest.mark.parametrize("keyed", [True, False])
def test_device_project_equals_oracle(keyed):
    """`<0:3>`: the select list on the device, members read from the batch and from the carry; e2[1] of a tuple with fewer
    than two hits comes out with its null flag set, and e2[last] is the last bound slot (null without a hit); the
    timestamp is e3's."""
    kind = "symbol" if keyed else "flat"
    t, sid, cols, ts = case("0_3", kind, select=PSELECT)
    rows = oracle_out(t, sid, cols, ts)["streams"]["OutputStream"]
    tup = tuples_of(oracle_out(case("0_3", kind, select=ISELECT)[0], sid, cols, ts), 5)
    assert len(tup) == len(rows) >= 30
    ranges, _ = cuts_for(tup, 0, 3, len(ts))
    assert straddling(tup[:, [0, -1]], ranges) >= 1  # a member read from the carry
    r = Run(t)
    got = []
    for lo, hi in ranges:
        r.piece(sid, cols, ts, lo, hi)
        assert r.app.get_stat("match_arity:q") == 5
        vals, nulls, ots = r.app.device_project("q")
        r.torch.cuda.synchronize()
        nl = nulls.cpu().tolist()
        got += [[t_, [0 if z else x for x, z in zip(v, zs)], [bool(z) for z in zs]]
                for t_, v, zs in zip(ots.cpu().tolist(), vals.cpu().tolist(), nl)]
    assert set(r.paths) == {14}
    r.app.close()
    assert got == [[row[0], *words(row[1])] for row in rows]
    assert any(g[2][3] and not g[2][2] for g in got)  # one hit: e2[1] null, e2[0] and e2[last] not
    assert any(g[2][2] and g[2][4] for g in got)      # no hit: e2[0] and e2[last] null
    one = [g for g in got if g[2][3] and not g[2][2]]
    assert all(g[1][2] == g[1][4] for g in one)       # e2[last] is e2[0] then
    assert [g[0] for g in got] == ts[tup[:, -1]].tolist()


def test_callbacks_receive_the_oracles_events():
    """A StreamCallback and a columns callback through SiddhiAppRuntime.sendDeviceEvents: one call per completing event,
    in order of it, before the call returns."""
    import torch
    import siddhi_amd
    from siddhi_amd import ColumnsStreamCallback, SiddhiManager, StreamCallback
    sid, cols, ts = events(n=N, K=20)
    t = text("0_3", keys=BY_SYMBOL, select=PSELECT, within=400)
    rows = oracle_out(t, sid, cols, ts)["streams"]["OutputStream"]
    assert len(rows) >= 100
    tup = tuples_of(oracle_out(text("0_3", keys=BY_SYMBOL, select=ISELECT, within=400), sid, cols, ts), 5)
    ranges, _ = cuts_for(tup, 0, 3, len(ts))
    assert straddling(tup[:, [0, -1]], ranges) >= 1
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
            assert v.value == 14
            seen.append(sum(len(c) for c in evs) + sum(len(c[0]) for c in columns))
        rt.shutdown()
    # one chunk per completing event: the outputs it completes arrive together
    flat_evs = [e for chunk in evs for e in chunk]
    assert flat_evs == [[r[0], r[1]] for r in rows]
    assert [len(c) for c in evs] == np.unique(tup[:, -1], return_counts=True)[1].tolist()
    assert max(len(c) for c in evs) >= 2
    exp_words = [words(r[1]) for r in rows]
    got_words = [[0 if (nb >> a) & 1 else w[a] for a in range(len(w))] for c in columns for w, nb in zip(c[1], c[2])]
    assert got_words == [w for w, _ in exp_words]
    assert [[bool((nb >> a) & 1) for a in range(len(PKINDS))] for c in columns for nb in c[2]] == [z for _, z in exp_words]
    assert [x for c in columns for x in c[0]] == [r[0] for r in rows]
    assert seen[0] == int((tup[:, -1] < ranges[0][1]).sum())  # delivered before the call returned


def test_match_arity_and_timing_labels():
    sid, cols, ts = events(n=N, K=20)
    n = len(ts)
    r = Run(text("2_4", keys=BY_SYMBOL), fast_timing=1)
    assert r.app.get_stat("match_arity:q") == 6
    r.piece(sid, cols, ts, 0, n // 2)
    labels = ["pcnt_facts", "pcnt_pack", "pcnt_sort", "pcnt_link", "pcnt_count", "pcnt_scan", "pcnt_cand", "pcnt_emit",
              "pcnt_order", "pcnt_parts", "pcnt_carry"]
    for label in labels:
        assert r.app.get_stat(f"kernel_calls:{label}") == 1
        assert r.app.get_stat(f"kernel_ms:{label}") >= 0
    assert r.app.get_stat("kernel_calls:plog_link") == 0 and r.app.get_stat("kernel_calls:mpatk_link") == 0
    r.piece(sid, cols, ts, n // 2, n)
    assert r.paths == [14, 14] and r.app.get_stat("nfa_state:q") == 0
    r.app.close()
