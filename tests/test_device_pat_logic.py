"""The closed form of the logical pair `every e1=A[c1] -> e2=B[c2] and|or e3=C[c3] within T` (streams of one schema) on
interleaved device batches (sm_app_process_device_events, fast_path 13: kernels/seqpath.hip fast_pat_logic,
mpat_logic_dev.h) against the CPU oracle fed the same events. Every A row passing c1 takes the first later B row of its
partition instance passing c2 and the first later C row passing c3; `and` emits at the later of the two, `or` at the
earlier with the other side null, inside T of e1; the product carries the open partials, an `and` partial possibly with
one member bound, and the events they hold across batches. Every case compares the (e1, e2, e3) ordinals of the whole
stream (-1: the null side of `or`), tuple for tuple and in order, with the oracle's, checks the path taken, and asserts a
floor of expected outputs that the oracle alone reaches. Inputs: 4000 rows (4400 for the hot key), 3 streams and
heartbeat rows, 20 keys or fewer."""
import ctypes
import struct

import numpy as np
import pytest

from test_device_mseq import NAMES, Run, events, oracle_out, send_rows, straddling, tuples_of

pytestmark = pytest.mark.gpu

GT = "price > e1.price"
T_KEYED, T_FLAT = 150, 10  # ms: about eight rows of a key out of 20, about ten rows of the flat stream
N = 4000
OPS = ["and", "or"]


def text(op, a="A", b="B", c="C", keys=None, within=T_KEYED, c2=GT, c3=GT, select=None, kt="int", c1="[price>20]"):
    schema = "".join(f"define stream {s} (symbol {kt}, price double, volume long, timestamp long); " for s in NAMES)
    w = "" if within is None else f" within {within} milliseconds"
    sel = select or "select e1.timestamp as i1, e2.timestamp as i2, e3.timestamp as i3"
    q = f"@info(name='q') from every e1={a}{c1} -> e2={b}[{c2}] {op} e3={c}[{c3}]{w} {sel} insert into OutputStream;"
    if keys is None:
        return schema + q
    return schema + "partition with (" + ", ".join(f"{x} of {s}" for s, x in keys.items()) + f") begin {q} end;"


BY_SYMBOL = {"A": "symbol", "B": "symbol", "C": "symbol"}
PER_STREAM = {"A": "symbol", "B": "volume", "C": "symbol"}


def case(op, kind, K=20, n=N, **kw):
    """(text, sid, cols, ts) of a form: flat, keyed by symbol, or B keyed by its volume."""
    if kind == "flat":
        sid, cols, ts = events(n=n, K=1)
        return text(op, keys=None, **dict({"within": T_FLAT}, **kw)), sid, cols, ts
    sid, cols, ts = events(n=n, K=K)
    if kind == "per_stream":
        cols = (cols[0], cols[1], cols[2] % K, cols[3])
        return text(op, keys=PER_STREAM, **kw), sid, cols, ts
    return text(op, keys=BY_SYMBOL, **kw), sid, cols, ts


def done_of(exp):
    """The completing member of every tuple: the later of e2 / e3 (the null side is -1)."""
    return exp[:, 1:].max(axis=1)


def first_of(exp):
    """The member bound first (`or`: the only one)."""
    m = np.where(exp[:, 1:] < 0, np.iinfo(np.int64).max, exp[:, 1:])
    return m.min(axis=1)


def spans(exp):
    """(e1, completing member) of every tuple: what a cut must fall between for the partial to be carried."""
    return np.stack([exp[:, 0], done_of(exp)], axis=1)


def nulls_out(got):
    """Run.piece() adds the piece's base to every word: the null word (-2^31) stays far below 0, a global ordinal never."""
    return np.where(got < 0, -1, got)


def run(app_text, sid, cols, ts, ranges, ords=None, **options):
    r = Run(app_text, **options)
    for lo, hi in ranges:
        r.piece(sid, cols, ts, lo, hi, ords)
    tuples, out, state = r.finish()
    return nulls_out(tuples), out, r.paths, state


def cuts_inside(exp, n, extra=()):
    """Pieces cut in front of the completing member of expected tuples (one in each quarter), plus `extra` cuts."""
    sp = spans(exp)
    far = sp[sp[:, 1] - sp[:, 0] > 1]
    cuts = {int(far[len(far) // 4, 1]), int(far[len(far) // 2, 1]), int(far[3 * len(far) // 4, 1])} | set(extra)
    cuts = sorted(c for c in cuts if 0 < c < n)
    return list(zip([0] + cuts, cuts + [n]))


def check(t, sid, cols, ts, ranges, floor=30, ords=None, **options):
    exp_out = oracle_out(t, sid, cols, ts, ords)
    exp = tuples_of(exp_out, 3)
    assert len(exp) >= floor, len(exp)
    got, out, paths, state = run(t, sid, cols, ts, ranges, ords=ords, **options)
    assert set(paths) == {13} and state == 0
    assert got.shape[1] == 3
    np.testing.assert_array_equal(got, exp)
    assert out == exp_out  # values (null ones too), timestamps, visible refs and order of the delivered events
    return exp


# ---- 1. batches

@pytest.mark.parametrize("kind", ["flat", "symbol", "per_stream"])
@pytest.mark.parametrize("op", OPS)
def test_one_batch_and_ragged_pieces(op, kind):
    """`fast_path:q` is 13 with `nfa_state` 0 (0 and 1 on the parent commit: the NFA kernel). One batch; then pieces of 1,
    1023 and 1025 rows and cuts in front of expected tuples' completing members."""
    t, sid, cols, ts = case(op, kind)
    n = len(ts)
    exp = check(t, sid, cols, ts, [(0, n)])
    if op == "or":
        assert (exp[:, 1] < 0).sum() >= 10 and (exp[:, 2] < 0).sum() >= 10  # both sides complete tuples
    inside = [lo for lo, _ in cuts_inside(exp[done_of(exp) > 2049], n)[1:]]
    cuts = [1, 1024, 2049] + inside
    ranges = list(zip([0] + cuts, cuts + [n]))
    assert {hi - lo for lo, hi in ranges} >= {1, 1023, 1025} and len(inside) >= 2 and straddling(spans(exp), ranges) >= 3
    check(t, sid, cols, ts, ranges)


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("op", OPS)
def test_pieces_of_1_and_37_rows(op, keyed):
    t, sid, cols, ts = case(op, "symbol" if keyed else "flat", K=5)
    n = len(ts)
    ranges = [(lo, min(lo + 37, 1850)) for lo in range(0, 1850, 37)] + [(lo, lo + 1) for lo in range(1850, 2050)] + [(2050, n)]
    exp = check(t, sid, cols, ts, ranges)
    assert straddling(spans(exp), ranges) >= 20


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("first", ["e2", "e3"])
def test_and_cuts_between_e1_its_first_member_and_the_second(first, keyed):
    """`and`: for three expected tuples whose `first` member comes first, a piece starts at that member (the carried
    partial binds it at the head of its run), the next piece one row later and another at the completing member: the
    partial crosses two cuts holding one member."""
    t, sid, cols, ts = case("and", "symbol" if keyed else "flat", **({} if keyed else {"within": 40}))
    exp = tuples_of(oracle_out(t, sid, cols, ts), 3)
    f, l = first_of(exp), done_of(exp)
    sel = exp[(exp[:, 1 if first == "e2" else 2] == f) & (l - f >= 3) & (f - exp[:, 0] >= 1)]
    assert len(sel) >= 12, len(sel)
    cuts = set()
    for x in (sel[len(sel) // 4], sel[len(sel) // 2], sel[3 * len(sel) // 4]):
        fx, lx = int(min(x[1], x[2])), int(max(x[1], x[2]))
        cuts |= {fx, fx + 1, lx}
    cuts = sorted(cuts)
    ranges = list(zip([0] + cuts, cuts + [len(ts)]))
    los = np.array(cuts)
    half_crossings = ((los[None, :] > f[:, None]) & (los[None, :] <= l[:, None])).sum(axis=1)
    assert (half_crossings >= 2).sum() >= 3  # half bound across at least two cuts
    check(t, sid, cols, ts, ranges)


# ---- 2. long scans and a hot key

def long_scan_stream():
    """One key. Every e1 has its e2 (a B row) and e3 (a C row) at the given distances, both half a unit above its price;
    every other row fails c1, c2 and c3. The first e1 has the highest price and the longest scan (e3 at 17, e2 at 1500);
    the next five lie inside that scan, each done before the next begins, with lower prices, so that no member passes
    for another e1. The lane's own budget is 16 positions and a wave step 64. The last e1 has its e2 at 30, then, 199
    positions on, a C row that fails c3 with an event time beyond the window, one position in front of the C row that
    would have passed."""
    n = 4000
    rng = np.random.default_rng(17)
    sid = np.where(rng.random(n) < 0.5, 2, 1).astype(np.int32)
    sid[rng.random(n) < 0.1] = -1
    sym = np.full(n, 3, np.int32)
    price = np.full(n, 10.0)
    starts = [0, 100, 400, 700, 1000, 1300, 3000]
    d2 = [1500, 40, 5, 17, 200, 64, 30]
    d3 = [17, 50, 250, 90, 100, 65, 200]
    p1 = [59.0, 50.0, 51.0, 52.0, 53.0, 54.0, 55.0]
    for s, a, b, p in zip(starts, d2, d3, p1):
        sid[s], price[s] = 0, p
        sid[s + a], price[s + a] = 1, p + 0.5
        sid[s + b], price[s + b] = 2, p + 0.5
    ts = np.arange(n, dtype=np.int64) // 100
    sid[3199], price[3199] = 2, 10.0
    ts[3199:] += 1000
    cols = (sym, price, np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64))
    return sid, cols, ts, starts, d2, d3


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("op", OPS)
def test_members_far_ahead_among_rows_that_fail(op, keyed):
    """Members 17 .. 1500 sorted positions ahead: both inside one wave step ((40, 50), (64, 65)), one inside the private
    budget and the other in the wave finish ((5, 250)), e3 first ((1500, 17), (200, 100): `or` binds the C side; `and`
    holds its e3 over a scan of 1500 positions), and the
    window stop one position in front of a would-be hit (no output for the last e1 of `and`)."""
    sid, cols, ts, starts, d2, d3 = long_scan_stream()
    n = len(ts)
    t = text(op, keys=BY_SYMBOL if keyed else None, c1="[price>35]", within=100)
    exp = check(t, sid, cols, ts, [(0, n)], floor=6)
    want = []
    for s, a, b in zip(starts, d2, d3):
        if op == "and":
            want.append([s, s + a, s + b])
        else:
            want.append([s, s + a, -1] if a < b else [s, -1, s + b])
    if op == "and":
        want = want[:-1]  # the window stops the last one
    assert sorted(exp.tolist()) == sorted(want)
    check(t, sid, cols, ts, [(0, 450), (450, 1250), (1250, 3100), (3100, n)], floor=6)  # carried partials scan far too


def hot_key_stream(op):
    """3400 A rows of key 7 (heartbeats and rows of another key between them) and one B row of key 7 at 4300 that
    completes them all. `and`: a C row at 2400 gives the A rows in front of it their e3 (they are carried half bound),
    and one at 4290 gives it to the others."""
    n = 4400
    sid = np.zeros(n, np.int32)
    sid[5::10] = -1
    sym = np.full(n, 7, np.int32)
    sym[8::10] = 3
    price = np.full(n, 30.0)
    if op == "and":
        sid[2400], price[2400] = 2, 42.0
        sid[4290], price[4290] = 2, 42.0
    sid[4300], price[4300] = 1, 50.0
    sid[4390], price[4390] = 1, 50.0  # nobody is left for it but the A rows behind 4300
    return sid, (sym, price, np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)), np.arange(n, dtype=np.int64) // 50


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("op", OPS)
def test_one_event_completes_3000_carried_and_batch_partials(op, keyed):
    sid, cols, ts = hot_key_stream(op)
    t = text(op, keys=BY_SYMBOL if keyed else None, within=200, c2="price > 45", c3="price > 40")
    ranges = [(0, 2500), (2500, len(ts))]
    exp = check(t, sid, cols, ts, ranges, floor=3000)
    one = exp[done_of(exp) == 4300]
    assert len(one) >= 3000 and (one[:, 0] < 2500).sum() >= 1000 and (one[:, 0] >= 2500).sum() >= 1000
    assert (np.diff(one[:, 0]) > 0).all()  # oldest first
    if op == "and":
        assert (one[:, 2] == 2400).sum() >= 1000 and (one[:, 2] == 4290).sum() >= 1000


# ---- 3. keys, ordinals, shared streams

@pytest.mark.parametrize("remap", ["auto", "off", "on"])
@pytest.mark.parametrize("op", OPS)
def test_long_keys_negative_and_wide(op, remap):
    sid, cols, ts = events(n=N, K=20)
    sym = (cols[0].astype(np.int64) - 10) * 3_000_011
    assert sym.min() < 0 and sym.max() - sym.min() > 1 << 20
    cols = (sym, cols[1], cols[2], cols[3])
    t = text(op, keys=BY_SYMBOL, kt="long")
    exp = tuples_of(oracle_out(t, sid, cols, ts), 3)
    opts = {} if remap == "auto" else {"key_remap": 1 if remap == "on" else 0}
    check(t, sid, cols, ts, cuts_inside(exp, len(ts)), **opts)


@pytest.mark.parametrize("op", OPS)
def test_negative_int_keys(op):
    sid, cols, ts = events(n=N, K=20)
    cols = (cols[0] - 10, cols[1], cols[2], cols[3])
    t = text(op, keys=BY_SYMBOL)
    exp = tuples_of(oracle_out(t, sid, cols, ts), 3)
    assert (cols[0][exp[:, 0]] < 0).any()
    check(t, sid, cols, ts, cuts_inside(exp, len(ts)))


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("op", OPS)
def test_given_ordinals_with_gaps(op, keyed):
    """Rows carrying the global ordinals 3 i + 1, each piece's first ordinal as its base."""
    t, sid, cols, ts = case(op, "symbol" if keyed else "flat")
    ords = 3 * np.arange(len(ts), dtype=np.int64) + 1
    exp = tuples_of(oracle_out(t, sid, cols, ts, ords), 3)
    assert ((exp % 3 == 1) | (exp < 0)).all()
    check(t, sid, cols, ts, cuts_inside(np.where(exp < 0, -1, (exp - 1) // 3), len(ts)), ords=ords)


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("abc", [("A", "A", "C"), ("A", "B", "A"), ("C", "A", "B")])
def test_or_with_shared_streams_and_another_assignment(abc, keyed):
    """A = B: an e1 is a candidate e2 of the earlier partials of its key. A = C likewise with e3."""
    sid, cols, ts = events(n=N, K=20 if keyed else 1)
    t = text("or", *abc, keys={s: "symbol" for s in abc} if keyed else None, within=T_KEYED if keyed else T_FLAT)
    exp = tuples_of(oracle_out(t, sid, cols, ts), 3)
    check(t, sid, cols, ts, cuts_inside(exp, len(ts)))


def test_and_with_another_assignment():
    sid, cols, ts = events(n=N, K=20)
    abc = ("C", "A", "B")
    t = text("and", *abc, keys={s: "symbol" for s in abc})
    exp = tuples_of(oracle_out(t, sid, cols, ts), 3)
    check(t, sid, cols, ts, cuts_inside(exp, len(ts)))


# ---- 4. hand-over to the NFA kernel

def small(keyed):
    """3000 rows whose c1 leaves few partials open: unkeyed, the NFA kernel's one lane walks every one of them."""
    sid, cols, ts = events(n=3000, K=10 if keyed else 1, heartbeats=0.0)
    return sid, cols, ts, dict(keys=BY_SYMBOL if keyed else None, c1="[price>20]" if keyed else "[price>48]")


@pytest.mark.parametrize("case_", ["inside", "before_carry"])
@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("op", OPS)
def test_decreasing_time_hands_over(op, case_, keyed):
    """Event time decreases inside the second piece, or from the first piece to the second: FAST_NON_MONOTONE, the NFA
    kernel takes the query over for good with the carried partials, `and` ones holding one member among them. The window
    is longer than the stream, so that no partial was dropped as expired before the hand-over (and the expected tuples do
    not depend on the event times). The pieces are cut in front of the completing member of two expected tuples."""
    sid, cols, ts, kw = small(keyed)
    t = text(op, within=30000, **kw)
    exp0 = tuples_of(oracle_out(t, sid, cols, ts), 3)
    if op == "and":  # cut between the two members
        far = exp0[done_of(exp0) - first_of(exp0) > 1]
    else:
        far = exp0[done_of(exp0) - exp0[:, 0] > 1]
    c1 = int(done_of(far)[len(far) // 3])
    c2 = int(done_of(far)[done_of(far) > c1 + 300][0])
    ranges = [(0, c1), (c1, c2), (c2, len(ts))]
    ts = ts.copy()
    if case_ == "inside":
        ts[c1 + 50:c1 + 250] = ts[c1 + 50:c1 + 250][::-1]
    else:
        ts[c1:] -= 50
    assert (np.diff(ts) < 0).any()
    exp_out = oracle_out(t, sid, cols, ts)
    exp = tuples_of(exp_out, 3)
    assert len(exp) >= 30 and straddling(spans(exp), ranges) >= 2
    if op == "and":  # a half-bound partial is in the carry at the hand-over
        assert ((first_of(exp) < c1) & (done_of(exp) >= c1)).sum() >= 1
    got, out, paths, state = run(t, sid, cols, ts, ranges)
    assert paths == [13, 5, 5] and state == 1
    np.testing.assert_array_equal(got, exp)
    assert out == exp_out


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("op", OPS)
def test_staged_sends_before_and_after_device_events(op, keyed):
    sid, cols, ts, kw = small(keyed)
    t = text(op, within=40, **kw)
    exp_out = oracle_out(t, sid, cols, ts)
    exp = tuples_of(exp_out, 3)
    n = len(ts)
    assert len(exp) >= 30
    # staged, then device: the NFA kernel holds the state
    r = Run(t)
    send_rows(r.app, sid, cols, ts, 0, 40)
    tail = nulls_out(r.piece(sid, cols, ts, 40, n))
    assert r.paths == [5] and r.app.get_stat("match_arity:q") == 3
    _, out, state = r.finish()
    assert state == 1 and out == exp_out
    np.testing.assert_array_equal(tail, exp[done_of(exp) >= 40])
    # device, staged, device: the flush replays the carried events into the NFA, which keeps the query
    sp = spans(exp)
    a = next(int(d) for e1, d in sp[len(sp) // 2:] if d - e1 > 1)  # in front of a tuple's completing member
    b = a + 40
    assert ((sp[:, 0] < a) & (sp[:, 1] >= a) & (sp[:, 1] < b)).any()  # a handed-over partial completes
    r = Run(t)
    first = nulls_out(r.piece(sid, cols, ts, 0, a))
    assert r.paths == [13] and r.app.get_stat("nfa_state:q") == 0
    send_rows(r.app, sid, cols, ts, a, b)
    r.app.flush()
    assert r.app.get_stat("nfa_state:q") == 1
    last = nulls_out(r.piece(sid, cols, ts, b, n))
    assert r.paths == [13, 5]
    _, out, state = r.finish()
    assert state == 1 and out == exp_out
    np.testing.assert_array_equal(first, exp[done_of(exp) < a])
    np.testing.assert_array_equal(last, exp[done_of(exp) >= b])


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
    "no_within": (dict(within=None, c1="[price>55]"), {}),
    "b_is_c": (dict(within=80, b="B", c="B", c2="price > 45", c3="price <= 45 and price > e1.price"), {}),
    "and_a_is_b": (dict(within=40, b="A"), {}),
}


# (`or` with A = B is inside the envelope: test_or_with_shared_streams_and_another_assignment)
@pytest.mark.parametrize("op,which", [(op, w) for op in OPS for w in list(STAY) + ["second_query"]
                                      if (op, w) != ("or", "and_a_is_b")])
def test_texts_that_stay_on_the_nfa_route(op, which):
    """What ran on the NFA kernel before runs there as before, with the oracle's outputs, and `fast_path:q` stays 0: an
    unmarked text and a second query never reach the closed-form branch of sm_app_process_device_events, and
    keep_outputs turns it off."""
    sid, cols, ts = events(n=3000, K=10, heartbeats=0.0)
    ranges = [(0, 1300), (1300, 3000)]
    if which == "second_query":
        t = text(op, keys=BY_SYMBOL, within=40).replace(
            " end;", " @info(name='q2') from every e1=B[price>30] -> e2=A[price>e1.price] within 40 milliseconds "
                     "select e1.timestamp as i1, e2.timestamp as i2 insert into Out2; end;")
        opts, stream = {}, "Out2"
    else:
        kw, opts = STAY[which]
        keys = {"A": "symbol", "B": "symbol"} if which in ("b_is_c", "and_a_is_b") else BY_SYMBOL
        if which == "and_a_is_b":
            keys = {"A": "symbol", "C": "symbol"}
        t, stream = text(op, keys=keys, **kw), "OutputStream"
    exp_out = oracle_out(t, sid, cols, ts)
    assert len(exp_out["streams"][stream]) >= 30
    out, paths = feed_pieces(t, sid, cols, ts, ranges, **opts)
    assert paths == [0, 0] and out == exp_out


# ---- 5. snapshot

@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("op", OPS)
def test_snapshot_restore_inside_a_tuple(op, keyed):
    """`and`: between the partial's two members; `or`: between e1 and its member."""
    t, sid, cols, ts = case(op, "symbol" if keyed else "flat", **({} if keyed else {"within": 40}))
    exp = tuples_of(oracle_out(t, sid, cols, ts), 3)
    f, l = (first_of(exp), done_of(exp)) if op == "and" else (exp[:, 0], done_of(exp))
    far = np.nonzero(l - f > 1)[0]
    cut = int(l[far[len(far) // 4]])
    assert ((f < cut) & (l >= cut)).sum() >= 1 and len(exp) >= 30
    a = Run(t)
    first = nulls_out(a.piece(sid, cols, ts, 0, cut))
    snap = a.app.snapshot()
    a.app.close()
    b = Run(t)
    b.app.restore(snap)
    second = nulls_out(b.piece(sid, cols, ts, cut, len(ts)))
    b.app.close()
    assert a.paths == [13] and b.paths == [13]
    np.testing.assert_array_equal(np.concatenate([first, second]), exp)


# ---- 6. outputs and stats

PSELECT = ("select e1.symbol as k, e1.price as p1, e2.price as p2, e3.price as p3, e3.volume - e1.volume as dv, "
           "e1.timestamp as i1, e2.timestamp as i2, e3.timestamp as i3")
PKINDS = ["i", "d", "d", "d", "i", "i", "i", "i"]


def words(row):
    """(values with 0 for a null one, null flags)."""
    vals = [0 if v is None else struct.unpack("<q", struct.pack("<d", v))[0] if k == "d" else int(v)
            for v, k in zip(row, PKINDS)]
    return vals, [v is None for v in row]


@pytest.mark.parametrize("keyed", [True, False])
@pytest.mark.parametrize("op", OPS)
def test_device_project_equals_oracle(op, keyed):
    """The select list on the device, members read from the batch and from the carry; the null side of `or` comes out
    with its null flag set; the timestamp is the completing member's."""
    t, sid, cols, ts = case(op, "symbol" if keyed else "flat", select=PSELECT)
    rows = oracle_out(t, sid, cols, ts)["streams"]["OutputStream"]
    tup = np.array([[-1 if x is None else x for x in r[1][5:8]] for r in rows], dtype=np.int64)
    assert len(tup) >= 30
    ranges = cuts_inside(tup, len(ts))
    assert straddling(spans(tup), ranges) >= 1  # a member read from the carry
    r = Run(t)
    got = []
    for lo, hi in ranges:
        r.piece(sid, cols, ts, lo, hi)
        assert r.app.get_stat("match_arity:q") == 3
        vals, nulls, ots = r.app.device_project("q")
        r.torch.cuda.synchronize()
        nl = nulls.cpu().tolist()
        got += [[t_, [0 if z else x for x, z in zip(v, zs)], [bool(z) for z in zs]]
                for t_, v, zs in zip(ots.cpu().tolist(), vals.cpu().tolist(), nl)]
    assert set(r.paths) == {13}
    r.app.close()
    assert got == [[row[0], *words(row[1])] for row in rows]
    if op == "or":
        assert any(g[2][2] for g in got) and any(g[2][3] for g in got)
    assert [g[0] for g in got] == ts[done_of(tup)].tolist()


@pytest.mark.parametrize("op", OPS)
def test_callbacks_receive_the_oracles_events(op):
    """A StreamCallback and a columns callback through SiddhiAppRuntime.sendDeviceEvents: one call per completing event,
    in order of it, before the call returns."""
    import torch
    import siddhi_amd
    from siddhi_amd import ColumnsStreamCallback, SiddhiManager, StreamCallback
    sid, cols, ts = events(n=N, K=20)
    t = text(op, keys=BY_SYMBOL, select=PSELECT, c2="price > 40", c3="price > 40", within=400)
    rows = oracle_out(t, sid, cols, ts)["streams"]["OutputStream"]
    assert len(rows) >= 100
    tup = np.array([[-1 if x is None else x for x in r[1][5:8]] for r in rows], dtype=np.int64)
    ranges = cuts_inside(tup, len(ts))
    assert straddling(spans(tup), ranges) >= 1
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
            assert v.value == 13
            seen.append(sum(len(c) for c in evs) + sum(len(c[0]) for c in columns))
        rt.shutdown()
    # one chunk per completing event: the outputs it completes arrive together, oldest e1 first
    flat_evs = [e for chunk in evs for e in chunk]
    assert flat_evs == [[r[0], r[1]] for r in rows]
    assert [len(c) for c in evs] == np.unique(done_of(tup), return_counts=True)[1].tolist()
    assert max(len(c) for c in evs) >= 2
    exp_words = [words(r[1]) for r in rows]
    got_words = [[0 if (nb >> a) & 1 else w[a] for a in range(len(w))] for c in columns for w, nb in zip(c[1], c[2])]
    assert got_words == [w for w, _ in exp_words]
    assert [[bool((nb >> a) & 1) for a in range(len(PKINDS))] for c in columns for nb in c[2]] == [z for _, z in exp_words]
    assert [x for c in columns for x in c[0]] == [r[0] for r in rows]
    assert seen[0] == int((done_of(tup) < ranges[0][1]).sum())  # delivered before the call returned


@pytest.mark.parametrize("op", OPS)
def test_match_arity_and_timing_labels(op):
    sid, cols, ts = events(n=N, K=20)
    n = len(ts)
    r = Run(text(op, keys=BY_SYMBOL), fast_timing=1)
    assert r.app.get_stat("match_arity:q") == 3
    r.piece(sid, cols, ts, 0, n // 2)
    labels = ["plog_facts", "plog_pack", "plog_sort", "plog_link", "plog_count", "plog_scan", "plog_cand", "plog_emit",
              "plog_order", "plog_parts", "plog_carry"]
    for label in labels:
        assert r.app.get_stat(f"kernel_calls:{label}") == 1
        assert r.app.get_stat(f"kernel_ms:{label}") >= 0
    assert r.app.get_stat("kernel_calls:mpatk_link") == 0 and r.app.get_stat("kernel_calls:mpat_link") == 0
    r.piece(sid, cols, ts, n // 2, n)
    assert r.paths == [13, 13] and r.app.get_stat("nfa_state:q") == 0
    r.app.close()
