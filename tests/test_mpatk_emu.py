"""The closed form of `every e1=S1[c1] -> e2=S2[c2] within T2 -> ... -> ek=Sk[ck] within Tk` over several streams
(siddhi_amd/csrc/kernels/mpatk_dev.h: the link, candidate, partial, emit, key and tuple kernels, behind mseq_dev.h's
facts, pack and stream kernels and seq_dev.h's count kernel) run on the CPU under the host wave emulator
(tests/native/mpatk_emu.cpp: the same device source, one fiber per GPU thread, on the plan the product's compiler makes
of the query text), against a plain statement of the rule tests/test_mpatk_plan.py ties to the oracle: every partial (a
carried one with s bound events, or an S1 row of the batch passing c1) binds, state by state, the first later Sm row of
its instance that passes cm, if that row lies inside Tm of the event bound before; tuples in order of (ek, ..., e1); a
partial left open that the batch's last read event does not find expired is carried out, and so is every event it has
bound, once. The shapes are those at which the kernels can go wrong: waves, tiles, a state change inside the lane's
private budget, at its edge and inside a wave step, many partials on one ek. Test infrastructure: no GPU;
`-m "not gpu"`."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_mpatk_plan import CM, mpatk_text, rule_tuples, withins_of

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
LIB = os.path.join(NATIVE, "build", "libmpatk_emu.so")
CSRC = os.path.join(HERE, "..", "siddhi_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
NAMES = ["A", "B", "C"]
CW = 8  # carried event: key, global ordinal, ts, the four attributes, stream
BITS = lambda x: int(np.array([x], np.float64).view(np.int64)[0])
UNBITS = lambda b: float(np.array([b], np.int64).view(np.float64)[0])


def lib():
    srcs = [os.path.join(NATIVE, "mpatk_emu.cpp"), os.path.join(CSRC, "compiler.cpp"),
            os.path.join(CSRC, "siddhiql", "parser.cpp")]
    deps = srcs + [os.path.join(NATIVE, "emu_fibers.h"), os.path.join(CSRC, "compiler.h"), os.path.join(CSRC, "plan.h")]
    deps += [os.path.join(CSRC, "kernels", f) for f in ("mpatk_dev.h", "mpat_dev.h", "mseq_dev.h", "seq_dev.h",
                                                        "fastpath_dev.h", "expr.h", "hd.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call([CXX if os.path.exists(CXX) else "g++", "-std=c++20", "-O2", "-g", "-fPIC", "-shared",
                               "-Wno-attributes", "-o", LIB] + srcs + ["-lpthread"])
    L = ctypes.CDLL(LIB)
    L.sm_mpatk_emu.restype = ctypes.c_int64
    return L


def budget():
    return int(lib().sm_mpatk_budget())


def call(app_text, k, sid, sym, price, vol, ts, ordinals=None, obase=0, evt=None, parts=None):
    n = len(sid)
    evt = np.zeros((0, CW), np.int64) if evt is None else np.ascontiguousarray(evt, dtype=np.int64).reshape(-1, CW)
    parts = np.zeros((0, k + 1), np.int64) if parts is None else np.ascontiguousarray(parts, dtype=np.int64).reshape(-1, k + 1)
    tuples = np.full(k * (n + len(parts)) + 2, 0xDEADBEEF, np.uint32)
    pout = np.zeros((k + 1) * (n + len(parts)) + 2, np.int64)
    cand = np.zeros(4 * (n + len(evt)) + 4, np.int64)
    ncand, nparts = ctypes.c_int64(), ctypes.c_int64()
    marks = np.zeros(6, np.int32)
    facts = np.zeros(9, np.int64)
    err = ctypes.create_string_buffer(512)
    tcol = np.arange(n, dtype=np.int64)
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    arrs = [np.ascontiguousarray(sid, dtype=np.int32), np.ascontiguousarray(sym, dtype=np.int32),
            np.ascontiguousarray(price, dtype=np.float64), np.ascontiguousarray(vol, dtype=np.int64), tcol,
            np.ascontiguousarray(ts, dtype=np.int64)]
    m = lib().sm_mpatk_emu(app_text.encode(), ctypes.c_int64(n), *[P(a) for a in arrs], P(ordinals), ctypes.c_int64(obase),
                           P(evt), ctypes.c_int64(len(evt)), P(parts), ctypes.c_int64(len(parts)), P(tuples), P(pout),
                           ctypes.byref(nparts), P(cand), ctypes.byref(ncand), P(marks), P(facts), err,
                           ctypes.c_size_t(512))
    return m, tuples, pout[:(k + 1) * nparts.value].reshape(-1, k + 1), cand[:4 * ncand.value].reshape(-1, 4), marks, facts, err.value


def marks_of(app_text):
    z = np.zeros(1, np.int64)
    r = call(app_text, 3, z[:0].astype(np.int32), z[:0], z[:0], z[:0], z[:0])
    assert r[0] >= 0 or r[6].startswith(b"not marked"), r[6]  # the text compiles
    return tuple(int(x) for x in r[4])


def row_keys(pattern, keys, sid, sym, vol):
    key = np.zeros(len(sid), np.int64)
    if keys is not None:
        for s in set(pattern):
            mine = sid == NAMES.index(s)
            key[mine] = (sym if keys[s] == "symbol" else vol)[mine]
    return key


def rule(pattern, key, sid, price, vol, ts, gord, obase, withins, cm, evt, parts):
    """One batch with its carry, partial by partial: (tuples relative to obase in order of (ek, ..., e1), the partials
    that stay in order of place, the sorted carry-out candidates (key, global ordinal, ts, source), read rows)."""
    k = len(pattern)
    w = withins_of(k, withins)
    want = [NAMES.index(s) for s in pattern]
    f = CM[cm][1]
    read = np.nonzero(np.isin(sid, sorted(set(want))))[0]
    if len(read) == 0:
        return np.zeros((0, k), np.int64), np.zeros((0, k + 1), np.int64), [], 0
    ts_last = ts[read[-1]]
    where = {(int(r[0]), int(r[1])): c for c, r in enumerate(evt)}
    # a member: (global ordinal, price, volume, ts, source)
    todo = []
    for p in parts:
        mem = []
        for o in p[2:2 + p[1]]:
            c = where[(int(p[0]), int(o))]
            mem.append((int(o), UNBITS(evt[c][4]), int(evt[c][5]), int(evt[c][2]), -c - 1))
        todo.append((int(p[0]), mem, -1))
    for i in np.nonzero((sid == want[0]) & (price > 20))[0]:
        todo.append((int(key[i]), [(int(gord[i]), float(price[i]), int(vol[i]), int(ts[i]), int(i))], int(i)))
    on = {}
    tuples, stay, cand = [], [], set()
    for kv, mem, after in todo:
        mem = list(mem)
        done = dead = False
        while not done and not dead:
            m = len(mem)
            if (kv, m) not in on:
                on[(kv, m)] = np.nonzero((sid == want[m]) & (key == kv))[0]
            c = on[(kv, m)]
            c = c[np.searchsorted(c, after, side="right"):]
            P, V = np.array([x[1] for x in mem]), np.array([x[2] for x in mem])
            end = f(P, V, price[c], vol[c]) | (ts[c] - mem[-1][3] > w[m + 1])  # the scan ends at the first of either
            if not end.any():
                break
            j = c[np.argmax(end)]
            if ts[j] - mem[-1][3] > w[m + 1]:
                dead = True
            else:
                mem.append((int(gord[j]), float(price[j]), int(vol[j]), int(ts[j]), int(j)))
                after = j
                done = len(mem) == k
        if done:
            tuples.append(tuple(x[0] - obase for x in mem)[::-1])
        elif not dead and ts_last - mem[-1][3] <= w[len(mem) + 1]:
            stay.append([kv, len(mem)] + [x[0] for x in mem] + [0] * (k - 1 - len(mem)))
            for x in mem:
                cand.add((kv, x[0], x[3], x[4]))
    tuples.sort()
    return (np.array([t[::-1] for t in tuples], dtype=np.int64).reshape(-1, k),
            np.array(stay, dtype=np.int64).reshape(-1, k + 1), sorted(cand), len(read))


def run(pattern, keys, sid, sym, price, vol, ts, withins=5, cm="gt", ordinals=None, obase=0, evt=None, parts=None):
    k = len(pattern)
    n = len(sid)
    evt = np.zeros((0, CW), np.int64) if evt is None else np.asarray(evt, dtype=np.int64).reshape(-1, CW)
    parts = np.zeros((0, k + 1), np.int64) if parts is None else np.asarray(parts, dtype=np.int64).reshape(-1, k + 1)
    m, tuples, pout, cand, marks, facts, err = call(mpatk_text(pattern, keys, withins, cm), k, sid, sym, price, vol, ts,
                                                    ordinals, obase, evt, parts)
    assert m >= 0 and marks[0] == k, err
    gord = obase + np.arange(n, dtype=np.int64) if ordinals is None else ordinals
    sid, sym, vol = np.asarray(sid), np.asarray(sym, dtype=np.int64), np.asarray(vol, dtype=np.int64)
    key = row_keys(pattern, keys, sid, sym, vol)
    exp, exp_parts, exp_cand, nread = rule(pattern, key, sid, np.asarray(price, dtype=np.float64), vol,
                                           np.asarray(ts, dtype=np.int64), gord, obase, withins, cm, evt, parts)
    assert facts[0] == nread
    if nread == 0:
        assert m == 0  # the host entry returns before the carry is read: the carried partials wait
        return exp, parts, evt
    got = tuples[:k * m].view(np.int32).astype(np.int64).reshape(-1, k)
    np.testing.assert_array_equal(got, exp)
    assert tuples[k * m] == 0xDEADBEEF  # nothing written past the last tuple
    np.testing.assert_array_equal(pout, exp_parts)
    assert sorted(tuple(int(x) for x in c) for c in cand) == exp_cand
    # the new event table, as build_carry makes it: the candidates' rows sorted by (key, ordinal)
    rows = []
    for kv, o, t, src in exp_cand:
        rows.append(list(evt[-src - 1]) if src < 0 else
                    [kv, o, t, int(sym[src]), BITS(price[src]), int(vol[src]), src, int(sid[src])])
    rows.sort(key=lambda r: (r[0], r[1]))
    return exp, pout, np.array(rows, dtype=np.int64).reshape(-1, CW)


def batch(n, K, seed=0, streams=(0, 0, 1, 1, 2, -1), per=40):
    rng = np.random.default_rng(seed * 1000003 + n * 31 + K)
    sym = rng.integers(0, K, n).astype(np.int32) - 3  # negative keys too
    price = np.round(rng.random(n) * 60.0, 1)
    vol = rng.integers(0, 50, n).astype(np.int64)
    ts = np.arange(n, dtype=np.int64) // per
    sid = np.array(streams, np.int32)[rng.integers(0, len(streams), n)]
    return sid, sym, price, vol, ts


ABA, ABC = list("ABA"), list("ABC")
BY_SYMBOL = {"A": "symbol", "B": "symbol", "C": "symbol"}
SIZES = [1, 63, 64, 65, 600, 1023, 1024, 1025, 2049]


@pytest.mark.parametrize("K", [None, 1, 5, 60])
@pytest.mark.parametrize("cm", list(CM))
def test_link_order_and_carry_out_follow_the_rule(cm, K):
    """Below, at and above a wave, a tile (1024 rows) and two tiles; unkeyed, one key (a single run across tiles) and
    keyed; C rows and heartbeat rows in the feed. `price > 45` does not read the partial: one ek completes many."""
    total = 0
    for n in SIZES:
        sid, sym, price, vol, ts = batch(n, K or 1)
        total += len(run(ABA, None if K is None else BY_SYMBOL, sid, sym, price, vol, ts, withins=3, cm=cm)[0])
    assert total >= 30


def test_every_row_read_and_unkeyed_takes_no_pack():
    total = 0
    for n in SIZES:
        sid, sym, price, vol, ts = batch(n, 1, seed=3, streams=(0, 1))
        total += len(run(ABA, None, sid, sym, price, vol, ts, cm="compound")[0])
    assert total >= 30


@pytest.mark.parametrize("pattern", [ABA, ABC, list("BCAB"), list("ABCBBCBA")])
@pytest.mark.parametrize("K", [None, 1, 5])
def test_batches_chained_through_the_carry_equal_the_whole_stream(pattern, K):
    """600 events and more in ragged pieces, the partials and their events carried from piece to piece (at every s below
    k, an e2 shared by several partials): the pieces' tuples are the whole stream's."""
    k = len(pattern)
    keys = None if K is None else {s: BY_SYMBOL[s] for s in set(pattern)}
    seen, total = set(), 0
    for n, cuts in ((600, (1, 77, 300)), (2600, (1023, 1025, 2049, 2300))):
        sid, sym, price, vol, ts = batch(n, K or 1, seed=5, streams=(0, 1, 1, 2, 2, -1), per=8)
        cols = [sym.astype(np.int64), price, vol, np.arange(n)]
        whole = rule_tuples(pattern, sid, cols, ts, keys, 9, "compound")
        total += len(whole)
        got, evt, parts = [], None, None
        edges = [0, *cuts, n]
        for lo, hi in zip(edges[:-1], edges[1:]):
            exp, parts, evt = run(pattern, keys, sid[lo:hi], sym[lo:hi], price[lo:hi], vol[lo:hi], ts[lo:hi], 9,
                                  "compound", obase=lo, evt=evt, parts=parts)
            # (the attribute `timestamp` of a carried event is its row in its own piece: not read by these conditions)
            got.append(exp + lo)
            seen |= {int(p[1]) for p in parts}
            assert len(evt) <= sum(int(p[1]) for p in parts)
        np.testing.assert_array_equal(np.concatenate(got), whole)
    assert total >= 30 and seen >= {1, 2}  # partials carried with one and with two bound events


def scan_batch(L1, L2, keyed):
    """One partial (row 0) whose e2 lies L1 sorted positions behind it and whose e3 L2 positions behind that; other
    keys' rows (keyed) or unread rows lie around."""
    n = 1 + L1 + L2 + 70
    sid = np.ones(n, np.int32)           # B rows that fail c2 (price 10)
    sid[2:L1:5] = 0                      # A rows among them: looked at by no state, and failing c1
    sid[0] = 0
    sym = np.zeros(n, np.int32)
    price = np.full(n, 10.0)
    price[0] = 30.0
    sid[L1], price[L1] = 1, 40.0         # e2
    sid[L1 + 1:L1 + L2] = 0              # A rows that fail c3 (price 10); B rows among them
    sid[L1 + 3:L1 + L2:7] = 1
    sid[L1 + L2], price[L1 + L2] = 0, 50.0  # e3
    price[L1 + L2 + 1:] = 55.0           # later matches are not taken
    if keyed:
        sym[L1 + L2 + 1:] = 1
    vol = np.arange(n, dtype=np.int64)
    ts = np.zeros(n, np.int64)
    return sid, sym, price, vol, ts


@pytest.mark.parametrize("keyed", [False, True])
def test_state_changes_inside_the_budget_at_its_edge_and_inside_a_wave_step(keyed):
    B = budget()
    ends = (B - 1, B, B + 1, B + 63, B + 64, B + 65, 200)
    assert ends == (15, 16, 17, 79, 80, 81, 200)
    for L1 in ends:
        for L2 in (1, 2) + ends:
            sid, sym, price, vol, ts = scan_batch(L1, L2, keyed)
            exp, parts, _ = run(ABA, BY_SYMBOL if keyed else None, sid, sym, price, vol, ts)
            assert [0, L1, L1 + L2] in exp.tolist()
    # the same scans cut by the end of the batch: the partial waits with one and with two bound events
    for L1 in ends:
        sid, sym, price, vol, ts = scan_batch(L1, 40, keyed)
        for cut, s in ((L1, 1), (L1 + 1, 2), (L1 + 40, 2)):
            exp, parts, evt = run(ABA, BY_SYMBOL if keyed else None, sid[:cut], sym[:cut], price[:cut], vol[:cut], ts[:cut])
            assert len(exp) == 0 and parts.tolist()[0][:3] == [0, s, 0] and len(evt) >= s


@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("m", [1, 64, 65, 1100])
def test_one_ek_completes_many_partials_through_shared_and_distinct_e2s(m, keyed):
    """m partials (carried ones at s = 1 and s = 2 among them) completed by one e3: more than a wave and more than a
    tile of tuples with one ek, through two e2s of the batch and a carried one, in order of (e2, e1)."""
    nc = min(m // 2, 300)
    nb = m - nc
    h = nb // 2
    kv = 4 if keyed else 0
    # rows: h A rows, B (e2 of those), nb - h A rows, B (e2 of those and of the carried partials at s = 1), A = e3, A
    sid = np.array([0] * h + [1] + [0] * (nb - h) + [1, 0, 0], np.int32)
    n = len(sid)
    sym = np.full(n, 4, np.int32)
    price = np.array([30.0] * h + [40.0] + [30.0] * (nb - h) + [40.0, 50.0, 50.0])
    vol = np.arange(n, dtype=np.int64)
    ts = np.full(n, 7, np.int64)
    evt = [[kv, 500 + c, 5, 4, BITS(31.0), c, 0, 0] for c in range(nc)] + [[kv, 900, 6, 4, BITS(41.0), 0, 0, 1]]
    s2 = nc // 3  # carried partials that hold the carried e2 already
    parts = [[kv, 2, 500 + c, 900] if c < s2 else [kv, 1, 500 + c, 0] for c in range(nc)]
    exp, pout, _ = run(ABA, BY_SYMBOL if keyed else None, sid, sym, price, vol, ts, obase=1000, evt=evt, parts=parts)
    e3 = nb + 2
    assert len(exp) == m and (exp[:, 2] == e3).all()
    assert sorted(set(exp[:, 1].tolist())) == sorted({-100, h, nb + 1} if s2 else ({h, nb + 1} if h else {nb + 1}))
    assert len(pout) == 2  # the two A rows behind the last B row


def test_carried_partials_match_expire_and_stay():
    """Carried partials at s = 1 and s = 2: key 0's match, key 1's are found expired by a row of their state, key 2's
    fail their condition and stay, key 3 is idle inside the key range (stays), key 9 is seen only in the carry (stays),
    key 5's are older than the window of the batch's last event and idle (dropped)."""
    evt, parts = [], []
    o = 700
    for kv, t, p, s in ((0, 8, 31.0, 1), (0, 9, 32.0, 2), (1, 2, 31.0, 1), (1, 2, 31.0, 2), (2, 9, 58.0, 1), (2, 9, 59.0, 2),
                        (3, 9, 31.0, 2), (5, 1, 31.0, 1), (5, 1, 31.0, 2), (9, 9, 31.0, 1)):
        evt.append([kv, o, t, kv, BITS(p), 100 + o, 0, 0])
        if s == 2:
            evt.append([kv, o + 1, t, kv, BITS(p + 0.5), 100 + o, 0, 1])
        parts.append([kv, s, o, o + 1 if s == 2 else 0])
        o += 2
    evt, parts = np.array(evt, np.int64), np.array(parts, np.int64)
    n = 400
    sid, sym, price, vol, ts = batch(n, 3, seed=6, streams=(0, 1, 2, -1))
    sym = sym + 3  # keys 0 .. 2
    sym[sym == 2] = 4
    sym[n - 50:][sid[n - 50:] != 2] = 2  # key 2 has rows that fail every condition
    price[sym == 2] = 40.0
    ts = 10 + ts // 4
    for keyed in (True, False):
        if not keyed:
            evt[:, 0] = 0  # one instance: its carried rows are in ordinal order
            parts[:, 0] = 0
        exp, pout, _ = run(ABA, BY_SYMBOL if keyed else None, sid, sym, price, vol, ts, withins=4, obase=2000, evt=evt,
                           parts=parts)
        assert (exp[:, 0] < 0).any() and (exp[:, 1] < 0).any()
        if keyed:
            old = [(int(p[0]), int(p[1])) for p in pout if p[2] < 2000]
            assert old == [(2, 1), (2, 2), (3, 2), (9, 1)], old


def test_per_stream_key_attributes_and_four_states():
    """B's instances are keyed by its volume, A's and C's by their symbol."""
    total = 0
    for n in (65, 1025, 2049):
        sid, sym, price, vol, ts = batch(n, 6, seed=8, streams=(0, 1, 2))
        vol = vol % 6 - 3
        keys = {"A": "symbol", "B": "volume", "C": "symbol"}
        total += len(run(ABC, keys, sid, sym, price, vol, ts, cm="compound")[0])
        total += len(run(list("BCAB"), keys, sid, sym, price, vol, ts, withins={2: 3, 3: 1, 4: 6}, cm="compound")[0])
    assert total >= 30


def test_given_ordinals_with_gaps_and_within_0():
    n = 2049
    sid, sym, price, vol, ts = batch(n, 5, seed=9, per=12)
    ords = 3 * np.arange(n, dtype=np.int64) + 1
    assert len(run(ABA, BY_SYMBOL, sid, sym, price, vol, ts, ordinals=ords, withins=0, cm="compound")[0]) >= 3
    assert len(run(ABA, None, sid, sym, price, vol, ts, ordinals=ords, withins=1)[0]) >= 30
    evt = [[0, -40, 0, 0, BITS(30.0), 1, 0, 0], [0, -7, 0, 0, BITS(31.0), 2, 0, 1]]
    exp, _, _ = run(ABA, None, sid, sym, price, vol, ts, ordinals=ords, withins=0, cm="const", evt=evt,
                    parts=[[0, 2, -40, -7]])
    assert exp[0].tolist()[:2] == [-40, -7]
