"""The closed form of the count pattern `every e1=A[c1] -> e2=B[c2]<m:n> -> e3=C[c3] within T`
(siddhi_amd/csrc/kernels/mpat_count_dev.h: pcnt_link_kernel, pcnt_parts_kernel and pcnt_emit_kernel, behind mseq_dev.h's
facts, pack and stream kernels, seq_dev.h's count kernel and mpatk_dev.h's candidate and tuple kernels) run on the CPU under
the host wave emulator (tests/native/pat_count_emu.cpp: the same device source, one fiber per GPU thread, on the plan the
product's compiler makes of the query text), against a brute-force statement of the rule tests/test_pat_count_plan.py ties
to the oracle, batch by batch with carried partials: every partial (a carried one, which may hold hits already, or an A row
of the batch passing c1) binds the first B rows of its instance passing c2 until it holds n; once it holds m, the first C
row that lies beyond T of the hit bound last kills it, and the first one inside T that passes c3 completes it; a partial
that neither emitted nor died is carried out with the events it holds, unless it holds n hits and its clock has run out at
the batch's last read row. Each case compares the tuples, in order of (e3, p, e1), the partials that stay and the sorted
carry-out candidates. The shapes are those at which the kernel can go wrong: hits at the private budget's edge and at a
wave step's edge, n hits and the deciding C row inside one wave step, a dying and a passing C row in one step in both
orders, a hit behind a death, a C row passing c3 in front of the m-th hit, two partials of one key completed by one C row
with p in the opposite order of e1. Test infrastructure: no GPU; `-m "not gpu"`."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_pat_count_plan import COUNTS, COUNT_CONDS, count_text

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
LIB = os.path.join(NATIVE, "build", "libpat_count_emu.so")
CSRC = os.path.join(HERE, "..", "siddhi_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
NAMES = ["A", "B", "C"]
CW = 8  # carried event: key, global ordinal, ts, the four attributes, stream
NULL = -(1 << 31)  # an unbound slot's word, as int32
BITS = lambda x: int(np.array([x], np.float64).view(np.int64)[0])
UNBITS = lambda x: float(np.array([x], np.int64).view(np.float64)[0])
ABC = ("A", "B", "C")


def lib():
    srcs = [os.path.join(NATIVE, "pat_count_emu.cpp"), os.path.join(CSRC, "compiler.cpp"),
            os.path.join(CSRC, "siddhiql", "parser.cpp")]
    deps = srcs + [os.path.join(NATIVE, "emu_fibers.h"), os.path.join(CSRC, "compiler.h"), os.path.join(CSRC, "plan.h")]
    deps += [os.path.join(CSRC, "kernels", f) for f in ("mpat_count_dev.h", "mpatk_dev.h", "mpat_dev.h", "mseq_dev.h",
                                                        "seq_dev.h", "fastpath_dev.h", "expr.h", "hd.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call([CXX if os.path.exists(CXX) else "g++", "-std=c++20", "-O2", "-g", "-fPIC", "-shared",
                               "-Wno-attributes", "-o", LIB] + srcs + ["-lpthread"])
    L = ctypes.CDLL(LIB)
    L.sm_pat_count_emu.restype = ctypes.c_int64
    return L


def call(app_text, sid, sym, price, vol, ts, ordinals=None, obase=0, evt=None, parts=None, cmax=6):
    """One batch: (m, tuples (m, n + 2) as int32 relative to obase (a carried member negative, an unbound slot NULL), the
    partials that stay (p, n + 5), sorted carry-out candidates, marks, (arity, hidden refs), facts, err)."""
    n = len(sid)
    pw, tw = cmax + 5, cmax + 2
    evt = np.zeros((0, CW), np.int64) if evt is None else np.ascontiguousarray(evt, dtype=np.int64)
    parts = np.zeros((0, pw), np.int64) if parts is None else np.ascontiguousarray(parts, dtype=np.int64)
    room = n + len(parts) + 2
    tuples = np.full(8 * room, 0xDEADBEEF, np.uint32)
    pout = np.zeros(11 * room, np.int64)
    cand = np.zeros(4 * (n + len(evt) + 2), np.int64)
    ncand, npart = ctypes.c_int64(), ctypes.c_int64()
    marks = np.zeros(4, np.int32)
    hidden = np.zeros(20, np.int32)
    facts = np.zeros(4, np.int64)
    err = ctypes.create_string_buffer(512)
    tcol = np.arange(n, dtype=np.int64)
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    I = ctypes.c_int64
    arrs = [np.ascontiguousarray(sid, dtype=np.int32), np.ascontiguousarray(sym, dtype=np.int32),
            np.ascontiguousarray(price, dtype=np.float64), np.ascontiguousarray(vol, dtype=np.int64), tcol,
            np.ascontiguousarray(ts, dtype=np.int64)]
    ordinals = None if ordinals is None else np.ascontiguousarray(ordinals, dtype=np.int64)
    m = lib().sm_pat_count_emu(app_text.encode(), I(n), *[P(a) for a in arrs], P(ordinals), I(obase), P(evt),
                               I(len(evt)), P(parts), I(len(parts)), P(tuples), P(pout), ctypes.byref(npart), P(cand),
                               ctypes.byref(ncand), P(marks), P(hidden), P(facts), err, ctypes.c_size_t(512))
    k = max(m, 0)
    tw = int(marks[0]) + 2 if marks[0] else tw
    pw = int(marks[0]) + 5 if marks[0] else pw
    assert tuples[tw * k] == 0xDEADBEEF  # nothing past the last tuple
    out = tuples[:tw * k].view(np.int32).astype(np.int64).reshape(-1, tw)
    cands = sorted(tuple(int(x) for x in cand[4 * c:4 * c + 4]) for c in range(ncand.value))
    plan = (int(hidden[0]), [(int(hidden[2 + 2 * r]), int(hidden[3 + 2 * r])) for r in range(min(int(hidden[1]), 8))])
    return m, out, pout[:pw * npart.value].reshape(-1, pw).copy(), cands, marks, plan, facts, err.value


def count_mark_of(app_text):
    """(m, n) of the plan's count mark, (0, 0) without one."""
    z = np.zeros(1, np.int64)
    r = call(app_text, z[:0].astype(np.int32), z[:0], z[:0], z[:0], z[:0])
    assert r[0] >= 0 or r[7].startswith(b"not marked"), r[7]  # the text compiles
    n = int(r[4][0])
    assert (int(r[4][3]) == n + 4 and int(r[4][2]) == n + 2) if n else int(r[4][1]) == 0
    return (int(r[4][1]), n)


def plan_of(app_text):
    z = np.zeros(1, np.int64)
    r = call(app_text, z[:0].astype(np.int32), z[:0], z[:0], z[:0], z[:0])
    assert r[0] >= 0, r[7]
    return r[5]


def rule(count, key, sid, price, vol, ts, gord, obase, within, conds, evt, parts):
    """One batch with its carry, partial by partial, by brute force: (tuples (m, n + 2) as call()'s, the partials that
    stay in order of place, the sorted carry-out candidates); None when no row is read (the carry waits)."""
    _, cmin, cmax = COUNTS[count]
    sa, sb, sc = 0, 1, 2
    n = len(sid)
    read = np.isin(sid, [sa, sb, sc])
    if not read.any():
        return None
    ts_last = int(ts[np.nonzero(read)[0][-1]])
    f2, f3 = COUNT_CONDS[conds][0][1], COUNT_CONDS[conds][1][1]
    erow = {(int(r[0]), int(r[1])): x for x, r in enumerate(evt)}
    ps = []  # key, o1, e1's source, scan after, price, volume, hit sources, tlast
    for r in parts:
        k, st, tl, _, o1 = (int(x) for x in r[:5])
        x1 = erow[(k, o1)]
        hits = [-erow[(k, int(o))] - 1 for o in r[5:5 + (st & 0xff)]]
        ps.append((k, o1, -x1 - 1, -1, UNBITS(evt[x1][4]), int(evt[x1][5]), hits, tl))
    for i in np.nonzero((sid == sa) & (price > 20))[0]:
        ps.append((int(key[i]), int(gord[i]), int(i), int(i), float(price[i]), int(vol[i]), [], int(ts[i])))
    pos = np.arange(n)
    ordinal = lambda src: int(evt[-src - 1][1]) if src < 0 else int(gord[src])
    time = lambda src: int(evt[-src - 1][2]) if src < 0 else int(ts[src])
    outs, stay, held = [], [], set()
    for place, (k, o1, src, after, p1, v1, hits, tl) in enumerate(ps):
        mine = read & (key == k) & (pos > after)
        new = np.nonzero(mine & (sid == sb) & f2(p1, v1, price, vol))[0][:cmax - len(hits)]
        cs = np.nonzero(mine & (sid == sc))[0]
        before = len(hits) + np.searchsorted(new, cs)
        hts = np.array([tl] * (len(hits) + 1) + [int(ts[j]) for j in new], np.int64)
        in3 = before >= cmin
        late = in3 & (ts[cs] - hts[before] > within)
        ok = in3 & ~late & f3(p1, v1, price[cs], vol[cs])
        stop = late | ok
        if stop.any():
            x = int(np.argmax(stop))
            if ok[x]:
                h = hits + [int(j) for j in new[:before[x] - len(hits)]]
                p = o1 if cmin == 0 else ordinal(h[cmin - 1])
                outs.append((int(cs[x]), p, place, [o1 - obase] + [ordinal(j) - obase for j in h] +
                             [NULL] * (cmax - len(h)) + [ordinal(int(cs[x])) - obase]))
            continue
        h = hits + [int(j) for j in new]
        tlast = time(h[-1]) if h else tl
        if len(h) == cmax and ts_last - tlast > within:
            continue
        stay.append([k, len(h) | (0x100 if len(h) >= cmin else 0), tlast,
                     (o1 if cmin == 0 else ordinal(h[cmin - 1])) if len(h) >= cmin else 0, o1] +
                    [ordinal(j) for j in h] + [0] * (cmax - len(h)))
        for x in [src] + h:
            held.add((k, ordinal(x), time(x), x))
    outs.sort(key=lambda o: o[:3])
    return (np.array([o[3] for o in outs], dtype=np.int64).reshape(-1, cmax + 2),
            np.array(stay, dtype=np.int64).reshape(-1, cmax + 5), sorted(held))


def next_carry(cands, evt, sid, sym, price, vol):
    """The event table build_carry makes of the candidates: rows sorted by (key, ordinal)."""
    rows = []
    for k, o, t, src in cands:
        if src < 0:
            r = [int(x) for x in evt[-src - 1]]
            r[0] = k
        else:
            r = [k, o, t, int(sym[src]), BITS(price[src]), int(vol[src]), src, int(sid[src])]
        rows.append(r)
    return np.array(sorted(rows), dtype=np.int64).reshape(-1, CW)


def keys_for(kind):
    if kind == "flat":
        return None
    keys = {s: "symbol" for s in ABC}
    if kind == "per_stream":
        keys["B"] = "volume"
    return keys


def check(count, kind, sid, sym, price, vol, ts, within=5, conds="gt_lt", evt=None, parts=None, obase=0, ordinals=None):
    _, cmin, cmax = COUNTS[count]
    keys = keys_for(kind)
    sid = np.asarray(sid, np.int32)
    sym, vol, price, ts = np.asarray(sym), np.asarray(vol, np.int64), np.asarray(price, float), np.asarray(ts, np.int64)
    key = np.zeros(len(sid), np.int64)
    if keys:
        for s in ABC:
            mine = sid == NAMES.index(s)
            key[mine] = (sym if keys[s] == "symbol" else vol)[mine]
    evt = np.zeros((0, CW), np.int64) if evt is None else evt
    parts = np.zeros((0, cmax + 5), np.int64) if parts is None else parts
    gord = obase + np.arange(len(sid), dtype=np.int64) if ordinals is None else np.asarray(ordinals, np.int64)
    text = count_text(count, *ABC, keys, within, conds, width=cmax)
    m, out, pout, cands, marks, _, facts, err = call(text, sid, sym, price, vol, ts, ordinals, obase, evt, parts, cmax)
    assert m >= 0 and marks[0] == cmax and marks[1] == cmin, err
    exp = rule(count, key, sid, price, vol, ts, gord, obase, within, conds, evt, parts)
    if exp is None:
        assert m == 0 and len(pout) == 0 and cands == []
        return out, parts, evt
    np.testing.assert_array_equal(out, exp[0])
    np.testing.assert_array_equal(pout, exp[1])
    assert cands == exp[2]
    return out, pout, next_carry(cands, evt, sid, sym, price, vol)


def random_batch(n, K, seed, heartbeats=0.1, step=3):
    rng = np.random.default_rng(seed)
    sid = rng.integers(0, 3, n).astype(np.int32)
    sid[rng.random(n) < heartbeats] = -1
    sym = rng.integers(0, K, n).astype(np.int32) - 2
    price = np.round(rng.random(n) * 60.0, 1)
    vol = (rng.integers(0, K, n) - 2).astype(np.int64)
    ts = 100 + np.cumsum(rng.integers(0, step, n)).astype(np.int64)
    return sid, sym, price, vol, ts


@pytest.mark.parametrize("kind", ["flat", "symbol", "per_stream"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2500])
@pytest.mark.parametrize("count", ["2_4", "0_3"])
def test_random_batches_in_three_pieces(count, n, kind):
    """Waves, blocks and tiles: one more and one fewer than each. Each piece takes the partials and events the piece
    before left; partials cross the cuts below m hits, in e3, and full."""
    sid, sym, price, vol, ts = random_batch(3 * n, 6, n)
    # B rows are mostly low and C rows mostly high, so that hits and e3 are rare and partials wait with hits bound
    price = np.where(sid == 1, price * 0.7, np.where(sid == 2, 20 + price * 0.7, price))
    evt = parts = None
    total, states = 0, set()
    cmin, cmax = COUNTS[count][1:]
    for piece in range(3):
        sl = slice(piece * n, (piece + 1) * n)
        out, parts, evt = check(count, kind, sid[sl], sym[sl], price[sl], vol[sl], ts[sl], 40, "gt_lt", evt, parts,
                                obase=1000 + piece * n)
        total += len(out)
        for st in parts[:, 1] if len(parts) else []:
            c = int(st) & 0xff
            states.add("below" if c < cmin else "full" if c == cmax else "in_e3")
    if n >= 1023:  # (a full partial crossing a cut: test_carried_partials_scan_far_and_the_carry_is_bounded_by_the_data)
        assert total >= 20 and states >= ({"in_e3"} | ({"below"} if cmin else set())), (total, states)
    sid, sym, price, vol, ts = random_batch(n, 6, n + 1)
    check(count, kind, sid, sym, price, vol, ts, 5, "compound_gt", obase=7)


@pytest.mark.parametrize("count", ["2_2", "1_1", "opt", "3_3", "2_6", "6_6"])
def test_other_counts(count):
    for kind in ("flat", "symbol"):
        sid, sym, price, vol, ts = random_batch(2400, 4, 5)
        evt = parts = None
        total = 0
        for piece in range(3):
            sl = slice(piece * 800, (piece + 1) * 800)
            out, parts, evt = check(count, kind, sid[sl], sym[sl], price[sl], vol[sl], ts[sl], 40, "gt_lt", evt, parts,
                                    obase=1000 + piece * 800)
            total += len(out)
        assert total >= 10, total


def feed(rows, K=1):
    """rows: (stream, price, ts) of one key's events, repeated for K keys."""
    sid = np.repeat(np.array([r[0] for r in rows], np.int32), K)
    price = np.repeat(np.array([r[1] for r in rows], float), K)
    ts = np.repeat(np.array([r[2] for r in rows], np.int64), K)
    sym = np.tile(np.arange(K, dtype=np.int32), len(rows))
    return sid, sym, price, np.zeros(len(rows) * K, np.int64), ts


FILL = [(2, 35.0), (1, 10.0), (0, 10.0)]  # rows that pass nothing for an e1 of price 30: C too high, B too low, A below c1


def single(events, last, t=100):
    """An e1 of price 30 at position 0; events: {distance: (stream, price[, ts])}; fillers elsewhere, up to `last`."""
    rows = [(0, 30.0, t)]
    for g in range(1, last + 1):
        if g in events:
            e = events[g]
            rows.append((e[0], e[1], e[2] if len(e) > 2 else t))
        else:
            rows.append(FILL[g % 3] + (t,))
    # event time never decreases: a row behind a late one is as late
    tt = np.maximum.accumulate([r[2] for r in rows])
    return [(r[0], r[1], int(x)) for r, x in zip(rows, tt)]


HIT, PASS, FAIL = (1, 40.0), (2, 25.0), (2, 35.0)
EDGES = [15, 16, 17, 63, 64, 65]


@pytest.mark.parametrize("kind", ["flat", "symbol"])
@pytest.mark.parametrize("d", EDGES + [1, 80, 200])
def test_hits_and_the_deciding_row_inside_one_step(d, kind):
    """`<2:4>`: four hits from distance d on and the passing C row right behind them: the private budget is 16 positions
    and a wave step 64, so the five rows fall inside the budget, across its edge, inside one step or across two."""
    assert lib().sm_pat_count_budget() == 16
    K = 1 if kind == "flat" else 3
    ev = {d + q: HIT for q in range(4)}
    ev[d + 4] = PASS
    out, pout, _ = check("2_4", kind, *feed(single(ev, d + 6), K), within=40)
    assert len(out) == K and len(pout) == 0
    assert (out[:, 1:5] == (np.arange(d, d + 4) * K)[None, :] + np.arange(K)[:, None]).all()
    # five hits: the fifth is not bound
    ev[d + 4], ev[d + 5] = HIT, PASS
    out, _, _ = check("2_4", kind, *feed(single(ev, d + 6), K), within=40)
    assert len(out) == K and (out[:, 4] == (d + 3) * K + np.arange(K)).all() and (out[:, 5] == (d + 5) * K + np.arange(K)).all()


@pytest.mark.parametrize("kind", ["flat", "symbol"])
@pytest.mark.parametrize("d", EDGES + [100])
@pytest.mark.parametrize("order", ["dies_then_passes", "passes_then_dies"])
def test_a_dying_and_a_passing_row_in_one_step(order, d, kind):
    """Two hits, then at d a C row beyond the window that fails c3 and a C row that passes, in both orders: the first of
    the two decides. The late row makes every row behind it late, so the passing row in front carries the earlier time."""
    K = 1 if kind == "flat" else 3
    ev = {1: HIT, 2: HIT}
    if order == "dies_then_passes":
        ev[d + 3] = FAIL + (1000,)
        ev[d + 4] = PASS + (1000,)
    else:
        ev[d + 3] = PASS
        ev[d + 4] = FAIL + (1000,)
    out, pout, _ = check("2_4", kind, *feed(single(ev, d + 6), K), within=40)
    assert len(out) == (0 if order == "dies_then_passes" else K) and len(pout) == 0


@pytest.mark.parametrize("kind", ["flat", "symbol"])
@pytest.mark.parametrize("d", EDGES)
def test_a_hit_behind_a_death_does_not_revive(d, kind):
    """Two hits, a late failing C row at d, then a hit (whose time would make the next C row fit) and a passing C row."""
    K = 1 if kind == "flat" else 3
    ev = {1: HIT, 2: HIT, d + 3: FAIL + (1000,), d + 4: HIT + (1000,), d + 5: PASS + (1000,)}
    out, pout, _ = check("2_4", kind, *feed(single(ev, d + 6), K), within=40)
    assert len(out) == 0 and len(pout) == 0
    # the same without the late row: the third hit refreshes the clock and the partial completes
    ev[d + 3] = FILL[1]
    out, _, _ = check("2_4", kind, *feed(single(ev, d + 6), K), within=40)
    assert len(out) == K


@pytest.mark.parametrize("kind", ["flat", "symbol"])
@pytest.mark.parametrize("d", EDGES)
def test_a_row_passing_c3_in_front_of_the_mth_hit_is_ignored(d, kind):
    """`<2:4>`: one hit, a passing C row (even a late one: a partial below m hits has no clock), the second hit at d, a
    passing C row behind it."""
    K = 1 if kind == "flat" else 3
    for t in (100, 1000):
        ev = {1: HIT, 2: PASS + (t,), d + 3: HIT + (t,), d + 4: PASS + (t,)}
        out, pout, _ = check("2_4", kind, *feed(single(ev, d + 6), K), within=40)
        assert len(out) == K and (out[:, -1] == (d + 4) * K + np.arange(K)).all()
        assert (out[:, 1] == K + np.arange(K)).all() and (out[:, 2] == (d + 3) * K + np.arange(K)).all()


@pytest.mark.parametrize("kind", ["flat", "symbol"])
def test_one_row_completes_two_partials_with_p_in_the_opposite_order_of_e1(kind):
    """`<1:1>`: the first e1 (price 50) takes its hit late (a B row of 55), the second (price 30) early (40): one C row
    completes both, and the second comes out first; with `<0:1>` p is e1 itself and the first comes out first."""
    K = 1 if kind == "flat" else 3
    rows = [(0, 50.0, 100), (0, 30.0, 100), (1, 40.0, 100), (1, 55.0, 100), (2, 25.0, 100)]
    out, _, _ = check("1_1", kind, *feed(rows, K), within=40)  # (a key's two outputs are adjacent: they share e3)
    assert len(out) == 2 * K and (out[0::2, 0] == K + np.arange(K)).all() and (out[1::2, 0] == np.arange(K)).all()
    out, _, _ = check("opt", kind, *feed(rows, K), within=40)
    assert len(out) == 2 * K and (out[0::2, 0] == np.arange(K)).all()
    # carried: the two partials cross a cut with their hits bound
    out, parts, evt = check("1_1", kind, *feed(rows[:4], K), within=40, obase=1000)
    assert len(out) == 0 and len(parts) == 2 * K and len(evt) == 4 * K
    out, parts, _ = check("1_1", kind, *feed(rows[4:], K), within=40, evt=evt, parts=parts, obase=1000 + 4 * K)
    assert len(out) == 2 * K and len(parts) == 0 and (out[0::2, 0] == -3 * K + np.arange(K)).all()


@pytest.mark.parametrize("kind", ["flat", "symbol"])
def test_carried_partials_scan_far_and_the_carry_is_bounded_by_the_data(kind):
    """A partial below m hits is carried whatever the time; a full one whose clock has run out is dropped; one in e3
    with room for hits is kept (a later hit refreshes its clock)."""
    K = 1 if kind == "flat" else 3
    rows = single({1: HIT}, 40) + [(0, 10.0, 5000)]
    out, parts, evt = check("2_4", kind, *feed(rows, K), within=40, obase=100)
    assert len(out) == 0 and len(parts) == K and (parts[:, 1] == 1).all() and len(evt) == 2 * K
    rows = single({1: HIT, 2: HIT}, 40) + [(0, 10.0, 5000)]
    out, parts, evt = check("2_4", kind, *feed(rows, K), within=40, obase=100)
    assert len(parts) == K and (parts[:, 1] == 0x102).all() and len(evt) == 3 * K
    rows2 = [FILL[1 + g % 2] + (5000,) for g in range(90)] + [HIT + (5000,), PASS + (5001,)]  # (no C row: it would kill)
    out, parts2, _ = check("2_4", kind, *feed(rows2, K), within=40, evt=evt, parts=parts, obase=100 + len(rows) * K)
    assert len(out) == K and len(parts2) == 0 and (out[:, :3] < 0).all() and (out[:, 3] >= 0).all()
    rows = single({1: HIT, 2: HIT}, 40) + [(0, 10.0, 5000)]
    out, parts, evt = check("2_2", kind, *feed(rows, K), within=40, obase=100)
    assert len(out) == 0 and len(parts) == 0 and len(evt) == 0
    # a full partial whose clock still runs is carried, and completes in the next batch
    rows = single({1: HIT, 2: HIT}, 40) + [(0, 10.0, 120)]
    out, parts, evt = check("2_2", kind, *feed(rows, K), within=40, obase=100)
    assert len(out) == 0 and len(parts) == K and (parts[:, 1] == 0x102).all() and len(evt) == 3 * K
    out, parts, _ = check("2_2", kind, *feed([FILL[1] + (130,), PASS + (140,)], K), within=40, evt=evt, parts=parts,
                          obase=100 + len(rows) * K)
    assert len(out) == K and len(parts) == 0


@pytest.mark.parametrize("kind", ["flat", "symbol", "per_stream"])
def test_given_ordinals_with_gaps(kind):
    sid, sym, price, vol, ts = random_batch(2400, 5, 21)
    ordinals = 5000 + 3 * np.arange(2400, dtype=np.int64) + 1
    evt = parts = None
    total = 0
    for piece in range(2):
        sl = slice(piece * 1200, (piece + 1) * 1200)
        out, parts, evt = check("2_4", kind, sid[sl], sym[sl], price[sl], vol[sl], ts[sl], 40, evt=evt, parts=parts,
                                obase=5000, ordinals=ordinals[sl])
        total += len(out)
    assert total > 10 and out[:, -1].max() > 1200


@pytest.mark.parametrize("kind", ["flat", "symbol"])
def test_no_read_row_and_only_a_rows(kind):
    n = 700
    sid = np.zeros(n, np.int32)
    sym = (np.arange(n) % 3).astype(np.int32)
    price = np.where(np.arange(n) % 5 == 0, 10.0, 30.0)
    ts = 100 + np.arange(n, dtype=np.int64) // 100
    out, parts, evt = check("2_4", kind, sid, sym, price, np.zeros(n, np.int64), ts, within=2, obase=1000)
    assert len(out) == 0 and len(parts) == n * 4 // 5 and len(evt) == len(parts)  # no clock below m hits: all stay
    hb = np.full(5, -1, np.int32)
    z = np.zeros(5, np.int64)
    out, p2, e2 = check("2_4", kind, hb, z, z.astype(float), z, 200 + z, 2, evt=evt, parts=parts, obase=2000)
    assert len(out) == 0 and p2 is parts and e2 is evt  # heartbeats only: the carried partials wait


def test_stand_alone_self_check_under_asan_and_ubsan():
    """tests/native/pat_count_emu.cpp's own main(), built with AddressSanitizer and UBSan as a stand-alone program and run
    once: four counts, keyed and unkeyed, random batches in three pieces at the wave and tile edges, and hits with their
    C row 1 .. 301 positions past the e1, against a plain loop."""
    exe = os.path.join(NATIVE, "build", "pat_count_emu_san")
    srcs = [os.path.join(NATIVE, "pat_count_emu.cpp"), os.path.join(CSRC, "compiler.cpp"),
            os.path.join(CSRC, "siddhiql", "parser.cpp")]
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    subprocess.check_call([CXX if os.path.exists(CXX) else "g++", "-std=c++20", "-O1", "-g", "-Wno-attributes",
                           "-DSM_PAT_COUNT_EMU_MAIN", "-o", exe] + san + srcs + ["-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "pat_count_emu self-check ok" in r.stdout, r.stdout + r.stderr
