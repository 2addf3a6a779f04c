"""The closed form of the logical pair `every e1=A[c1] -> e2=B[c2] and|or e3=C[c3] within T`
(siddhi_amd/csrc/kernels/mpat_logic_dev.h: plog_link_kernel, plog_parts_kernel and plog_emit_kernel, behind mseq_dev.h's
facts, pack and stream kernels, seq_dev.h's count kernel and mpatk_dev.h's candidate and tuple kernels) run on the CPU under
the host wave emulator (tests/native/pat_logic_emu.cpp: the same device source, one fiber per GPU thread, on the plan the
product's compiler makes of the query text), against a brute-force statement of the rule tests/test_pat_logic_plan.py ties
to the oracle, batch by batch with carried partials: every partial (a carried one, which may hold one member already, or an
A row of the batch passing c1) takes the first later B row of its instance passing c2 and the first later C row passing
c3, each only if still needed; `and` completes at the later of the two, `or` at the earlier, inside T of e1; a partial
that has not ended and is not older than T at the batch's last read row is carried out with the events it holds. Each
case compares the tuples, in order, the partials that stay and the sorted carry-out candidates. The shapes are those at
which the kernel can go wrong: the private budget's edge and a wave step's edge for either member, both members inside one
wave step, one in the budget and the other in the wave finish, the window stop one position in front of a would-be hit,
an `or` whose first hit is the C side. Test infrastructure: no GPU; `-m "not gpu"`."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_pat_logic_plan import CONDS, logic_text

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
LIB = os.path.join(NATIVE, "build", "libpat_logic_emu.so")
CSRC = os.path.join(HERE, "..", "siddhi_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
NAMES = ["A", "B", "C"]
CW = 8  # carried event: key, global ordinal, ts, the four attributes, stream
NULL = -(1 << 31)  # an absent member's word, as int32
BITS = lambda x: int(np.array([x], np.float64).view(np.int64)[0])
UNBITS = lambda x: float(np.array([x], np.int64).view(np.float64)[0])


def lib():
    srcs = [os.path.join(NATIVE, "pat_logic_emu.cpp"), os.path.join(CSRC, "compiler.cpp"),
            os.path.join(CSRC, "siddhiql", "parser.cpp")]
    deps = srcs + [os.path.join(NATIVE, "emu_fibers.h"), os.path.join(CSRC, "compiler.h"), os.path.join(CSRC, "plan.h")]
    deps += [os.path.join(CSRC, "kernels", f) for f in ("mpat_logic_dev.h", "mpatk_dev.h", "mpat_dev.h", "mseq_dev.h",
                                                        "seq_dev.h", "fastpath_dev.h", "expr.h", "hd.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call([CXX if os.path.exists(CXX) else "g++", "-std=c++20", "-O2", "-g", "-fPIC", "-shared",
                               "-Wno-attributes", "-o", LIB] + srcs + ["-lpthread"])
    L = ctypes.CDLL(LIB)
    L.sm_pat_logic_emu.restype = ctypes.c_int64
    return L


def call(app_text, sid, sym, price, vol, ts, ordinals=None, obase=0, evt=None, parts=None):
    """One batch: (m, tuples (m, 3) as int32 relative to obase (a carried member negative, an absent one NULL), the
    partials that stay (p, 4), sorted carry-out candidates, marks, (arity, hidden refs), facts, err)."""
    n = len(sid)
    evt = np.zeros((0, CW), np.int64) if evt is None else np.ascontiguousarray(evt, dtype=np.int64)
    parts = np.zeros((0, 4), np.int64) if parts is None else np.ascontiguousarray(parts, dtype=np.int64)
    room = n + len(parts) + 2
    tuples = np.full(3 * room, 0xDEADBEEF, np.uint32)
    pout = np.zeros(4 * room, np.int64)
    cand = np.zeros(4 * (n + len(evt) + 2), np.int64)
    ncand, npart = ctypes.c_int64(), ctypes.c_int64()
    marks = np.zeros(9, np.int32)
    hidden = np.zeros(8, np.int32)
    facts = np.zeros(4, np.int64)
    err = ctypes.create_string_buffer(512)
    tcol = np.arange(n, dtype=np.int64)
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    I = ctypes.c_int64
    arrs = [np.ascontiguousarray(sid, dtype=np.int32), np.ascontiguousarray(sym, dtype=np.int32),
            np.ascontiguousarray(price, dtype=np.float64), np.ascontiguousarray(vol, dtype=np.int64), tcol,
            np.ascontiguousarray(ts, dtype=np.int64)]
    ordinals = None if ordinals is None else np.ascontiguousarray(ordinals, dtype=np.int64)
    m = lib().sm_pat_logic_emu(app_text.encode(), I(n), *[P(a) for a in arrs], P(ordinals), I(obase), P(evt),
                               I(len(evt)), P(parts), I(len(parts)), P(tuples), P(pout), ctypes.byref(npart), P(cand),
                               ctypes.byref(ncand), P(marks), P(hidden), P(facts), err, ctypes.c_size_t(512))
    k = max(m, 0)
    assert tuples[3 * k] == 0xDEADBEEF  # nothing past the last tuple
    out = tuples[:3 * k].view(np.int32).astype(np.int64).reshape(-1, 3)
    cands = sorted(tuple(int(x) for x in cand[4 * c:4 * c + 4]) for c in range(ncand.value))
    plan = (int(hidden[0]), [(int(hidden[2 + 2 * r]), int(hidden[3 + 2 * r])) for r in range(min(int(hidden[1]), 3))])
    return m, out, pout[:4 * npart.value].reshape(-1, 4).copy(), cands, marks, plan, facts, err.value


def marks_of(app_text):
    z = np.zeros(1, np.int64)
    r = call(app_text, z[:0].astype(np.int32), z[:0], z[:0], z[:0], z[:0])
    assert r[0] >= 0 or r[7].startswith(b"not marked"), r[7]  # the text compiles
    return tuple(int(x) for x in r[4])


def plan_of(app_text):
    z = np.zeros(1, np.int64)
    r = call(app_text, z[:0].astype(np.int32), z[:0], z[:0], z[:0], z[:0])
    assert r[0] >= 0, r[7]
    return r[5]


def rule(op, abc, key, sid, price, vol, ts, gord, obase, within, conds, evt, parts):
    """One batch with its carry, partial by partial, by brute force: (tuples (m, 3) as call()'s, the partials that stay in
    order of place, the sorted carry-out candidates); None when no row is read (the carry waits)."""
    sa, sb, sc = (NAMES.index(x) for x in abc)
    n = len(sid)
    read = np.isin(sid, [sa, sb, sc])
    if not read.any():
        return None
    ts_last = int(ts[np.nonzero(read)[0][-1]])
    f2, f3 = CONDS[conds][0][1], CONDS[conds][1][1]
    erow = {(int(r[0]), int(r[1])): x for x, r in enumerate(evt)}
    ps = []  # key, o1, t1, e1's source, scan after, price, volume, [e2 source, e3 source] (None: needed)
    for r in parts:
        k, s, o1, o2 = (int(x) for x in r)
        x1 = erow[(k, o1)]
        mem = [None, None]
        if s >= 2:
            mem[s - 2] = -erow[(k, o2)] - 1
        ps.append((k, o1, int(evt[x1][2]), -x1 - 1, -1, UNBITS(evt[x1][4]), int(evt[x1][5]), mem))
    for i in np.nonzero((sid == sa) & (price > 20))[0]:
        ps.append((int(key[i]), int(gord[i]), int(ts[i]), int(i), int(i), float(price[i]), int(vol[i]), [None, None]))
    pos = np.arange(n)
    ordinal = lambda src: int(evt[-src - 1][1]) if src < 0 else int(gord[src])
    outs, stay, held = [], [], set()
    for place, (k, o1, t1, src, after, p1, v1, mem) in enumerate(ps):
        mine = read & (key == k) & (pos > after)
        found = []
        for side, (st, f) in enumerate(((sb, f2), (sc, f3))):
            if mem[side] is None:
                js = np.nonzero(mine & (sid == st) & f(p1, v1, price, vol))[0]
                if len(js):
                    found.append((int(js[0]), side))
        found.sort()
        done = None
        if op == "or":
            if found:
                done = found[0][0]
                mem[found[0][1]] = done
        else:
            for j, side in found:
                mem[side] = j
            if mem[0] is not None and mem[1] is not None:
                done = found[-1][0]
        if done is not None:
            if ts[done] - t1 <= within:
                outs.append((done, place, [o1 - obase] + [NULL if x is None else ordinal(x) - obase for x in mem]))
        elif ts_last - t1 <= within:
            s = 1 if mem[0] is None and mem[1] is None else 2 if mem[0] is not None else 3
            stay.append((k, s, o1, 0 if s == 1 else ordinal(mem[s - 2])))
            for x in [src] + [x for x in mem if x is not None]:
                held.add((k, ordinal(x), int(evt[-x - 1][2]) if x < 0 else int(ts[x]), x))
    outs.sort(key=lambda o: (o[0], o[1]))
    return (np.array([o[2] for o in outs], dtype=np.int64).reshape(-1, 3),
            np.array(stay, dtype=np.int64).reshape(-1, 4), sorted(held))


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


def keys_for(abc, kind):
    if kind == "flat":
        return None
    a, b, c = abc
    keys = {s: "symbol" for s in abc}
    if kind == "per_stream":
        keys[b if b != a else c] = "volume"
    return keys


def check(op, abc, kind, sid, sym, price, vol, ts, within=5, conds="gt_gt", evt=None, parts=None, obase=0, ordinals=None):
    keys = keys_for(abc, kind)
    sid = np.asarray(sid, np.int32)
    sym, vol, price, ts = np.asarray(sym), np.asarray(vol, np.int64), np.asarray(price, float), np.asarray(ts, np.int64)
    key = np.zeros(len(sid), np.int64)
    if keys:
        for s in set(abc):
            mine = sid == NAMES.index(s)
            key[mine] = (sym if keys[s] == "symbol" else vol)[mine]
    evt = np.zeros((0, CW), np.int64) if evt is None else evt
    parts = np.zeros((0, 4), np.int64) if parts is None else parts
    gord = obase + np.arange(len(sid), dtype=np.int64) if ordinals is None else np.asarray(ordinals, np.int64)
    text = logic_text(op, *abc, keys, within, conds)
    m, out, pout, cands, marks, _, facts, err = call(text, sid, sym, price, vol, ts, ordinals, obase, evt, parts)
    assert m >= 0 and marks[0] == (1 if op == "and" else 2), err
    exp = rule(op, abc, key, sid, price, vol, ts, gord, obase, within, conds, evt, parts)
    if exp is None:
        assert m == 0 and len(pout) == 0 and cands == []
        return out, parts, evt
    np.testing.assert_array_equal(out, exp[0])
    np.testing.assert_array_equal(pout, exp[1])
    assert cands == exp[2]
    return out, pout, next_carry(cands, evt, sid, sym, price, vol)


ABC = ("A", "B", "C")


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
@pytest.mark.parametrize("op", ["and", "or"])
def test_random_batches_in_three_pieces(op, n, kind):
    """Waves, blocks and tiles: one more and one fewer than each. Each piece takes the partials and events the piece before
    left; the `and` partials cross the cuts half bound."""
    sid, sym, price, vol, ts = random_batch(3 * n, 6, n)
    # C rows are mostly low, so that e3 (price > e1.price) is rare and partials wait for it with their e2 bound
    price = np.where(sid == 2, price * 0.5, price)
    evt = parts = None
    total, half = 0, 0
    for piece in range(3):
        sl = slice(piece * n, (piece + 1) * n)
        out, parts, evt = check(op, ABC, kind, sid[sl], sym[sl], price[sl], vol[sl], ts[sl], 40, "gt_gt", evt, parts,
                                obase=1000 + piece * n)
        total += len(out)
        half += int((parts[:, 1] >= 2).sum()) if len(parts) else 0
    if n >= 1023:
        assert total >= 20 and (op == "or" or half >= 1), (total, half)
    sid, sym, price, vol, ts = random_batch(n, 6, n + 1)
    check(op, ABC, kind, sid, sym, price, vol, ts, 5, "compound_gt", obase=7)


@pytest.mark.parametrize("kind", ["flat", "symbol"])
@pytest.mark.parametrize("first", ["e2", "e3"])
def test_a_half_bound_partial_crosses_two_cuts(first, kind):
    """`and`: e1 and its first member in piece 0, fillers that pass nothing in piece 1, the other member in piece 2: the
    partial is carried twice in state 2 (e2 first) or 3 (e3 first) and comes out with two carried members."""
    K = 1 if kind == "flat" else 3
    rep = lambda rows: (np.repeat(np.array([r[0] for r in rows], np.int32), K),
                        np.tile(np.arange(K, dtype=np.int32), len(rows)),
                        np.repeat(np.array([r[1] for r in rows]), K), np.zeros(len(rows) * K, np.int64),
                        100 + np.zeros(len(rows) * K, np.int64))
    b, c = (1, 40.0), (2, 45.0)
    fill = [((2, 10.0), (1, 10.0), (0, 10.0))[g % 3] for g in range(70)]
    pieces = [[(0, 30.0)] + fill[:20] + [b if first == "e2" else c], fill, fill[:5] + [c if first == "e2" else b]]
    evt = parts = None
    obase = 1000
    for x, rows in enumerate(pieces):
        out, parts, evt = check("and", ABC, kind, *rep(rows), within=40, evt=evt, parts=parts, obase=obase)
        obase += len(rows) * K
        if x < 2:
            assert len(out) == 0 and len(parts) == K and (parts[:, 1] == (2 if first == "e2" else 3)).all()
            assert len(evt) == 2 * K
    assert len(out) == K and len(parts) == 0 and len(evt) == 0
    assert (out[:, 0] < 0).all() and (out[:, 1 if first == "e2" else 2] < 0).all()
    assert (out[:, 2 if first == "e2" else 1] >= 0).all()


def member_feed(d2, d3, K=1, stop=None, p2=40.0, p3=40.0):
    """Per key: an e1, then fillers that pass nothing, e2 d2 positions and e3 d3 positions past the e1 (None: absent);
    stop: a B row at that distance whose event time lies beyond every window (it would pass c2)."""
    last = max(x for x in (d2, d3, stop) if x is not None)
    rows = [(0, 30.0, 100)]
    for g in range(1, last + 1):
        if g == stop:
            rows.append((1, 50.0, 1000))
        elif g == d2:
            rows.append((1, p2, 100 if stop is None or g < stop else 1000))
        elif g == d3:
            rows.append((2, p3, 100 if stop is None or g < stop else 1000))
        else:
            rows.append(((2, 10.0), (1, 10.0), (0, 10.0))[g % 3] + (100 if stop is None or g < stop else 1000,))
    n = len(rows) * K
    sid = np.repeat(np.array([r[0] for r in rows], np.int32), K)
    price = np.repeat(np.array([r[1] for r in rows]), K)
    ts = np.repeat(np.array([r[2] for r in rows], np.int64), K)
    sym = np.tile(np.arange(K, dtype=np.int32), len(rows))
    return sid, sym, price, np.zeros(n, np.int64), ts


EDGES = [(d2, d3) for d2 in (1, 15, 16, 17, 63, 64, 65, 80, 200, 1500) for d3 in (2, 16, 18, 66, 81, 129, 201, 1400)
         if d2 != d3]


@pytest.mark.parametrize("kind", ["flat", "symbol"])
@pytest.mark.parametrize("d2,d3", EDGES)
def test_members_at_the_budgets_and_the_wave_steps_edges(d2, d3, kind):
    """Both operators. The lane's own budget is 16 positions, a wave step 64: both members inside the budget, one in the
    budget and the other in the wave finish (first step, its edge, steps later), both inside one wave step ((17, 18),
    (65, 66), (80, 81), (17, 66) ...), e2 first and e3 first; `or` takes the earlier, which is the C side when d3 < d2."""
    assert lib().sm_pat_logic_budget() == 16
    K = 1 if kind == "flat" else 3
    fd = member_feed(d2, d3, K, p3=45.0)  # c3 of "gt_gt": price > e1.price
    out, pout, _ = check("and", ABC, kind, *fd, within=40)
    assert len(out) == K and len(pout) == 0
    assert (out[:, 1] == d2 * K + np.arange(K)).all() and (out[:, 2] == d3 * K + np.arange(K)).all()
    out, pout, _ = check("or", ABC, kind, *fd, within=40)
    assert len(out) == K and len(pout) == 0
    if d3 < d2:
        assert (out[:, 1] == NULL).all() and (out[:, 2] == d3 * K + np.arange(K)).all()
    else:
        assert (out[:, 2] == NULL).all() and (out[:, 1] == d2 * K + np.arange(K)).all()


@pytest.mark.parametrize("kind", ["flat", "symbol"])
@pytest.mark.parametrize("d", [2, 16, 17, 64, 65, 66, 130, 300])
def test_the_window_stop_one_position_in_front_of_a_would_be_hit(d, kind):
    """A B row beyond the window at d - 1, the passing row at d: nothing comes out and nothing stays (the batch's last
    read row lies beyond the window too). `and`: e2 found at 1 first, the stop then ends the search for e3."""
    K = 1 if kind == "flat" else 3
    out, pout, _ = check("or", ABC, kind, *member_feed(None, d, K, stop=d - 1, p3=45.0), within=40)
    assert len(out) == 0 and len(pout) == 0
    # the stop is a candidate only while its side is needed: with e2 bound at 1, a late B row is no stop, but a late C
    # row that fails c3 is
    fd = member_feed(1, d, K, p3=45.0)
    sid, sym, price, vol, ts = fd
    ts = ts.copy()
    late = np.arange(len(ts)) >= (d - 1) * K
    ts[late] = 1000
    sid = sid.copy()
    sid[(d - 1) * K:d * K] = 2
    price[(d - 1) * K:d * K] = 10.0
    if d - 1 > 1:
        out, pout, _ = check("and", ABC, kind, sid, sym, price, vol, ts, within=40)
        assert len(out) == 0 and len(pout) == 0


@pytest.mark.parametrize("kind", ["flat", "symbol"])
@pytest.mark.parametrize("op", ["and", "or"])
def test_one_event_completes_3000_carried_and_batch_partials(op, kind):
    """`price > 45`-style c2: 1500 carried partials (`and`: half bound with their e3) and 1500 batch partials of one key,
    then one B row: all of them come out at it, oldest first."""
    k = 1 if kind != "flat" else 0
    nc = 1500
    sid0 = np.zeros(nc + 1, np.int32)
    price0 = np.full(nc + 1, 30.0)
    if op == "and":
        sid0[-1], price0[-1] = 2, 50.0  # e3 of all of them (c3 compound: price > e1.price - 25 and volume differs)
    vol0 = np.where(sid0 == 2, 7, 0).astype(np.int64)
    sym = np.full(nc + 1, k, np.int32)
    out, parts, evt = check(op, ABC, kind, sid0, sym, price0, vol0, 100 + np.zeros(nc + 1, np.int64), 5, "const_compound",
                            obase=100)
    ncar = nc if op == "and" else nc + 1
    assert len(out) == 0 and len(parts) == ncar and (parts[:, 1] == (3 if op == "and" else 1)).all()
    n = 1502
    sid = np.zeros(n, np.int32)
    price = np.full(n, 30.0)
    sid[-1], price[-1] = 1, 50.0
    vol = np.zeros(n, np.int64)
    if op == "and":  # the batch partials need their e3 too
        sid[-2], price[-2], vol[-2] = 2, 50.0, 7
    out, pout, _ = check(op, ABC, kind, sid, np.full(n, k, np.int32), price, vol, 101 + np.zeros(n, np.int64), 5,
                         "const_compound", evt, parts, obase=5000)
    nb = int((sid == 0).sum())
    assert ncar + nb >= 3000 and len(out) == ncar + nb and len(pout) == 0
    assert (out[:, 1] == n - 1).all() and (np.diff(out[:, 0]) > 0).all() and (out[:ncar, 0] < 0).all()


@pytest.mark.parametrize("kind", ["flat", "symbol"])
@pytest.mark.parametrize("abc", [("A", "A", "C"), ("A", "B", "A"), ("C", "A", "B")])
def test_or_with_shared_streams(abc, kind):
    """A = B: an e1 is a candidate e2 of the earlier partials. A = C likewise."""
    sid, sym, price, vol, ts = random_batch(3000, 4, 5, step=2)
    evt = parts = None
    total = 0
    for piece in range(2):
        sl = slice(piece * 1500, (piece + 1) * 1500)
        out, parts, evt = check("or", abc, kind, sid[sl], sym[sl], price[sl], vol[sl], ts[sl], 5, "compound_gt", evt, parts,
                                obase=1000 + piece * 1500)
        total += len(out)
    assert total > 50


@pytest.mark.parametrize("kind", ["flat", "symbol"])
@pytest.mark.parametrize("op", ["and", "or"])
def test_no_read_row_and_only_a_rows(op, kind):
    n = 700
    sid = np.zeros(n, np.int32)
    sym = (np.arange(n) % 3).astype(np.int32)
    price = np.where(np.arange(n) % 5 == 0, 10.0, 30.0)
    ts = 100 + np.arange(n, dtype=np.int64) // 100
    out, parts, evt = check(op, ABC, kind, sid, sym, price, np.zeros(n, np.int64), ts, within=2, obase=1000)
    assert len(out) == 0 and 0 < len(parts) < n * 4 // 5 and len(evt) == len(parts)  # the open ones: c1, not older than 2 ms
    hb = np.full(5, -1, np.int32)
    z = np.zeros(5, np.int64)
    out, p2, e2 = check(op, ABC, kind, hb, z, z.astype(float), z, 200 + z, 2, evt=evt, parts=parts, obase=2000)
    assert len(out) == 0 and p2 is parts and e2 is evt  # heartbeats only: the carried partials wait


@pytest.mark.parametrize("kind", ["flat", "symbol", "per_stream"])
@pytest.mark.parametrize("op", ["and", "or"])
def test_given_ordinals_with_gaps(op, kind):
    sid, sym, price, vol, ts = random_batch(2400, 5, 21)
    ordinals = 5000 + 3 * np.arange(2400, dtype=np.int64) + 1
    evt = parts = None
    total = 0
    for piece in range(2):
        sl = slice(piece * 1200, (piece + 1) * 1200)
        out, parts, evt = check(op, ABC, kind, sid[sl], sym[sl], price[sl], vol[sl], ts[sl], 40, evt=evt, parts=parts,
                                obase=5000, ordinals=ordinals[sl])
        total += len(out)
    assert total > 10 and out[:, 1:].max() > 1200


@pytest.mark.parametrize("kind", ["flat", "symbol"])
@pytest.mark.parametrize("op", ["and", "or"])
def test_within_0(op, kind):
    sid, sym, price, vol, ts = random_batch(3000, 4, 8, step=2)
    out, _, _ = check(op, ABC, kind, sid, sym, price, vol, ts, 0)
    assert len(out) >= (3 if op == "or" or kind == "flat" else 1)  # (keyed `and` within 0 is rare)
    done = np.where(out[:, 1:] == NULL, -1, out[:, 1:]).max(axis=1)
    assert (ts[out[:, 0]] == ts[done]).all()


def test_stand_alone_self_check_under_asan_and_ubsan():
    """tests/native/pat_logic_emu.cpp's own main(), built with AddressSanitizer and UBSan as a stand-alone program and run
    once: both operators, keyed and unkeyed, random batches in three pieces at the wave and tile edges, and the two
    members 1 .. 301 positions past the e1, against a plain loop."""
    exe = os.path.join(NATIVE, "build", "pat_logic_emu_san")
    srcs = [os.path.join(NATIVE, "pat_logic_emu.cpp"), os.path.join(CSRC, "compiler.cpp"),
            os.path.join(CSRC, "siddhiql", "parser.cpp")]
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    subprocess.check_call([CXX if os.path.exists(CXX) else "g++", "-std=c++20", "-O1", "-g", "-Wno-attributes",
                           "-DSM_PAT_LOGIC_EMU_MAIN", "-o", exe] + san + srcs + ["-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "pat_logic_emu self-check ok" in r.stdout, r.stdout + r.stderr
