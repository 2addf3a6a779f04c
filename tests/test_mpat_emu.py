"""The closed form of `every e1=A[c1] -> e2=B[c2] within T` over two streams (siddhi_amd/csrc/kernels/mpat_dev.h: the
link, emit and pairs kernels, behind mseq_dev.h's facts, pack and stream kernels and seq_dev.h's count kernel) run on the
CPU under the host wave emulator (tests/native/mpat_emu.cpp: the same device source, one fiber per GPU thread, on the
plan the product's compiler makes of the query text), against a numpy statement of the rule tests/test_mpat_plan.py ties
to the oracle: every partial (a carried e1 row, or an A row of the batch passing c1) takes the first later B row of its
instance that passes c2, if that row lies inside the window; pairs in order of (e2, e1); the unmatched partials that the
batch's last read event does not find expired are carried out. The shapes are those at which the kernels can go wrong:
waves, tiles, the hand-off from a lane's private budget to the wave, many partials on one e2. Test infrastructure: no
GPU; `-m "not gpu"`."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_mpat_plan import C2, mpat_text

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
LIB = os.path.join(NATIVE, "build", "libmpat_emu.so")
CSRC = os.path.join(HERE, "..", "siddhi_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
NAMES = ["A", "B", "C"]
CW = 7  # carried row: key, global ordinal, ts, the four attributes
BITS = lambda x: int(np.array([x], np.float64).view(np.int64)[0])


def lib():
    srcs = [os.path.join(NATIVE, "mpat_emu.cpp"), os.path.join(CSRC, "compiler.cpp"),
            os.path.join(CSRC, "siddhiql", "parser.cpp")]
    deps = srcs + [os.path.join(NATIVE, "emu_fibers.h"), os.path.join(CSRC, "compiler.h"), os.path.join(CSRC, "plan.h")]
    deps += [os.path.join(CSRC, "kernels", f) for f in ("mpat_dev.h", "mseq_dev.h", "seq_dev.h", "fastpath_dev.h",
                                                        "expr.h", "hd.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call([CXX if os.path.exists(CXX) else "g++", "-std=c++20", "-O2", "-g", "-fPIC", "-shared",
                               "-Wno-attributes", "-o", LIB] + srcs + ["-lpthread"])
    L = ctypes.CDLL(LIB)
    L.sm_mpat_emu.restype = ctypes.c_int64
    return L


def budget():
    return int(lib().sm_mpat_budget())


def call(app_text, sid, sym, price, vol, ts, ordinals=None, obase=0, carry=None):
    n = len(sid)
    carry = np.zeros((0, CW), np.int64) if carry is None else np.ascontiguousarray(carry, dtype=np.int64)
    pairs = np.full(2 * (n + len(carry)) + 2, 0xDEADBEEF, np.uint32)
    cand = np.zeros(4 * (n + len(carry)) + 4, np.int64)
    ncand = ctypes.c_int64()
    marks = np.zeros(5, np.int32)
    facts = np.zeros(9, np.int64)
    err = ctypes.create_string_buffer(512)
    tcol = np.arange(n, dtype=np.int64)
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    arrs = [np.ascontiguousarray(sid, dtype=np.int32), np.ascontiguousarray(sym, dtype=np.int32),
            np.ascontiguousarray(price, dtype=np.float64), np.ascontiguousarray(vol, dtype=np.int64), tcol,
            np.ascontiguousarray(ts, dtype=np.int64)]
    m = lib().sm_mpat_emu(app_text.encode(), ctypes.c_int64(n), *[P(a) for a in arrs], P(ordinals), ctypes.c_int64(obase),
                          P(carry), ctypes.c_int64(len(carry)), P(pairs), P(cand), ctypes.byref(ncand), P(marks),
                          P(facts), err, ctypes.c_size_t(512))
    return m, pairs, cand, ncand.value, marks, facts, err.value


def marks_of(app_text):
    z = np.zeros(1, np.int64)
    return tuple(int(x) for x in call(app_text, z[:0].astype(np.int32), z[:0], z[:0], z[:0], z[:0])[4])


def rule(a, b, key, sid, price, vol, ts, gord, obase, within, c2, carry):
    """(pairs relative to obase in order of (e2, e1), sorted carry-out rows (key, global ordinal, ts, source), read rows)"""
    sa, sb = NAMES.index(a), NAMES.index(b)
    f = C2[c2][1]
    read = np.nonzero(np.isin(sid, [sa, sb]))[0]
    if len(read) == 0:
        return np.zeros((0, 2), np.int64), [], 0
    ts_last = ts[read[-1]]
    parts = [(int(r[0]), int(r[1]), int(r[2]), float(np.array([r[4]], np.int64).view(np.float64)[0]), int(r[5]), -c - 1, -1)
             for c, r in enumerate(carry)]
    for i in np.nonzero((sid == sa) & (price > 20))[0]:
        parts.append((int(key[i]), int(gord[i]), int(ts[i]), float(price[i]), int(vol[i]), int(i), int(i)))
    brows = {}
    for k in np.unique(key[sid == sb]):
        brows[int(k)] = np.nonzero((sid == sb) & (key == k))[0]
    pairs, cand = [], []
    for k, o, t1, p1, v1, src, after in parts:
        bj = brows.get(k, np.zeros(0, np.int64))
        bj = bj[np.searchsorted(bj, after, side="right"):]
        ok = f(p1, v1, price[bj], vol[bj]) | (ts[bj] - t1 > within)  # the scan ends at the first of either
        hit = None
        if ok.any():
            j = bj[np.argmax(ok)]
            if ts[j] - t1 <= within:
                hit = j
        if hit is not None:
            pairs.append((int(gord[hit] - obase), o - obase))
        elif ts_last - t1 <= within:
            cand.append((k, o, t1, src))
    pairs.sort()
    return np.array([(i, j) for j, i in pairs], dtype=np.int64).reshape(-1, 2), sorted(cand), len(read)


def row_keys(a, b, keys, sid, sym, vol):
    key = np.zeros(len(sid), np.int64)
    if keys is not None:
        for s in (a, b):
            mine = sid == NAMES.index(s)
            key[mine] = (sym if keys[s] == "symbol" else vol)[mine]
    return key


def run(keys, sid, sym, price, vol, ts, within=5, c2="gt", ordinals=None, obase=0, carry=None, a="A", b="B"):
    n = len(sid)
    carry = np.zeros((0, CW), np.int64) if carry is None else np.ascontiguousarray(carry, dtype=np.int64)
    m, pairs, cand, ncand, marks, facts, err = call(mpat_text(a, b, keys, within, c2), sid, sym, price, vol, ts, ordinals,
                                                    obase, carry)
    assert m >= 0 and marks[0] == 1, err
    gord = obase + np.arange(n, dtype=np.int64) if ordinals is None else ordinals
    key = row_keys(a, b, keys, np.asarray(sid), np.asarray(sym, dtype=np.int64), np.asarray(vol, dtype=np.int64))
    exp, exp_cand, nread = rule(a, b, key, np.asarray(sid), np.asarray(price, dtype=np.float64),
                                np.asarray(vol, dtype=np.int64), np.asarray(ts, dtype=np.int64), gord, obase, within, c2,
                                carry)
    assert facts[0] == nread
    if nread == 0:
        assert m == 0  # the host entry returns before the carry is read: the carried rows wait
        return exp, []
    got = pairs[:2 * m].view(np.int32).astype(np.int64).reshape(-1, 2)
    np.testing.assert_array_equal(got, exp)
    assert pairs[2 * m] == 0xDEADBEEF  # nothing written past the last pair
    got_cand = sorted(tuple(int(x) for x in cand[4 * c:4 * c + 4]) for c in range(ncand))
    assert got_cand == exp_cand
    return exp, exp_cand


def batch(n, K, seed=0, streams=(0, 0, 1, 1, 2, -1), per=40):
    rng = np.random.default_rng(seed * 1000003 + n * 31 + K)
    sym = rng.integers(0, K, n).astype(np.int32) - 3  # negative keys too
    price = np.round(rng.random(n) * 60.0, 1)
    vol = rng.integers(0, 50, n).astype(np.int64)
    ts = np.arange(n, dtype=np.int64) // per
    sid = np.array(streams, np.int32)[rng.integers(0, len(streams), n)]
    return sid, sym, price, vol, ts


SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049]
BY_SYMBOL = {"A": "symbol", "B": "symbol"}


@pytest.mark.parametrize("K", [None, 1, 5, 60])
@pytest.mark.parametrize("c2", list(C2))
def test_link_order_and_carry_out_follow_the_rule(c2, K):
    """Below, at and above a wave, a tile (1024 rows) and two tiles; unkeyed, one key (a single run across tiles) and
    keyed; C rows and heartbeat rows in the feed. `price > 45` does not read e1: one e2 completes many partials."""
    total = 0
    for n in SIZES:
        sid, sym, price, vol, ts = batch(n, K or 1)
        exp, _ = run(None if K is None else BY_SYMBOL, sid, sym, price, vol, ts, within=3, c2=c2)
        total += len(exp)
    assert total >= 30


def test_every_row_read_and_unkeyed_takes_no_pack():
    total = 0
    for n in SIZES:
        sid, sym, price, vol, ts = batch(n, 1, seed=3, streams=(0, 1))
        total += len(run(None, sid, sym, price, vol, ts)[0])
    assert total >= 30


def test_no_read_row_only_a_rows_only_b_rows():
    n = 1300
    carry = np.array([[0, 90, 1, 0, BITS(30.0), 7, 90]], np.int64)
    for keys in (None, BY_SYMBOL):
        sid, sym, price, vol, ts = batch(n, 3, seed=4, streams=(2, -1))
        assert len(run(keys, sid, sym, price, vol, ts, obase=100, carry=carry)[0]) == 0
        sid, sym, price, vol, ts = batch(n, 3, seed=4, streams=(0, 2, -1))
        ts[:] = 2
        exp, cand = run(keys, sid, sym, price, vol, ts, obase=100, carry=carry)
        assert len(exp) == 0 and len(cand) == 1 + int(((sid == 0) & (price > 20)).sum())  # every partial waits
        sid, sym, price, vol, ts = batch(n, 3, seed=4, streams=(1, 2, -1))
        ts[:] = 2
        sym[:] = 0
        price[np.nonzero(sid == 1)[0][0]] = 29.0  # the first B row fails c2 for the carried partial
        exp, cand = run(keys, sid, sym, price, vol, ts, obase=100, carry=carry)
        assert exp[:, 0].tolist() == [-10] and cand == []


def scan_batch(L, end, keyed):
    """One partial (row 0) whose scan is L sorted positions long and ends in `end`: a match, the window, the end of its
    key's run (keyed: another key's rows follow) or the end of the batch."""
    tail = 70
    n = 1 + L + (tail if end in ("match", "window", "run") else 0)
    if end == "batch":
        n = L  # the partial and L - 1 positions: position L is past the last row
    sid = np.ones(n, np.int32)
    sid[0] = 0
    sid[2:n:5] = 0  # A rows among the candidates: looked at, never a match (price 10 fails c1 too)
    sym = np.zeros(n, np.int32)
    price = np.full(n, 10.0)
    price[0] = 30.0
    vol = np.arange(n, dtype=np.int64)
    ts = np.zeros(n, np.int64)
    if end in ("match", "window"):
        sid[L] = 1
        price[L] = 50.0
        price[L + 1:] = 55.0  # later matches are not taken
        sid[L + 1:] = 1
        if end == "window":
            ts[L:] = 9
    if end == "run":
        sym[L:] = 1 if keyed else 0
        price[L:] = 50.0
        sid[L:] = 1
    return sid, sym, price, vol, ts


@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("end", ["match", "window", "run", "batch"])
def test_private_budget_and_wave_finish(end, keyed):
    """A scan of exactly budget - 1, budget, budget + 1, budget + 64 and budget + 65 positions (and a few more around the
    second wave step): the hand-off from the lane's own budget to the wave-cooperative finish, 64 positions per step."""
    B = budget()
    for L in (1, 2, B - 1, B, B + 1, B + 63, B + 64, B + 65, B + 128, B + 129, 700, 1100):
        sid, sym, price, vol, ts = scan_batch(L, end, keyed)
        exp, cand = run(BY_SYMBOL if keyed else None, sid, sym, price, vol, ts)
        if end == "match" or (end == "run" and not keyed):
            assert exp.tolist() == [[0, L]]
        elif end == "window":
            assert len(exp) == 0 and cand == []  # expired: not carried either
        elif len(sid) > 1:
            assert len(exp) == 0 and cand[0][3] == 0  # the partial waits for the next batch


@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("m", [1, 64, 65, 1100])
def test_one_e2_completes_many_partials(m, keyed):
    """More than a wave and more than a tile of pairs with one e2, carried partials among them, oldest e1 first."""
    nc = min(m // 2, 300)
    nb = m - nc
    n = nb + 3
    sid = np.zeros(n, np.int32)
    sid[nb] = 1
    sid[nb + 1] = 1
    sym = np.full(n, 4, np.int32)
    price = np.full(n, 30.0)
    price[nb:] = 50.0
    vol = np.arange(n, dtype=np.int64)
    ts = np.full(n, 7, np.int64)
    carry = np.array([[4 if keyed else 0, 500 + c, 5, 4, BITS(31.0), c, 0] for c in range(nc)], np.int64).reshape(-1, CW)
    exp, cand = run(BY_SYMBOL if keyed else None, sid, sym, price, vol, ts, obase=1000, carry=carry)
    assert len(exp) == m and (exp[:, 1] == nb).all() and (np.diff(exp[:, 0]) > 0).all()
    assert len(cand) == 1  # the A row behind the two B rows


def test_carried_partials_match_expire_and_stay():
    """Keys 0 .. 5 hold carried partials: key 0's match, key 1's are found expired by a B row, key 2's fail c2 and stay,
    key 3 is idle and inside the key range (stays), key 9 is seen only in the carry and above the batch's key range
    (stays), key 5's are older than the window of the batch's last event and idle (dropped)."""
    rows = []
    for k, t, p in ((0, 8, 31.0), (0, 9, 32.0), (1, 2, 31.0), (2, 9, 58.0), (2, 9, 59.0), (3, 9, 31.0), (5, 1, 31.0),
                    (9, 9, 31.0)):
        rows.append([k, 700 + len(rows), t, k, BITS(p), 100 + len(rows), 0])
    carry = np.array(rows, np.int64)
    n = 400
    sid, sym, price, vol, ts = batch(n, 3, seed=6, streams=(0, 1, 2, -1))
    sym = sym + 3  # keys 0 .. 2
    sym[sym == 2] = 4
    sym[n - 50:][sid[n - 50:] == 1] = 2  # key 2 has B rows only, all of which fail c2
    price[sym == 2] = 40.0
    sid[sym == 2] = 1
    ts = 10 + ts // 4
    for keyed in (True, False):
        if not keyed:
            carry[:, 0] = 0  # one instance: its carried rows are in ordinal order
        exp, cand = run(BY_SYMBOL if keyed else None, sid, sym, price, vol, ts, within=4, obase=1000, carry=carry)
        assert (exp[:, 0] < 0).any()
        if keyed:
            kept = sorted(c[0] for c in cand if c[3] < 0)
            assert kept == [2, 2, 3, 9], kept


def test_per_stream_key_attributes_and_directions():
    """B's instances are keyed by its volume, A's by its symbol; `B -> A` and `C -> A`."""
    total = 0
    for n in (65, 1025, 2049):
        sid, sym, price, vol, ts = batch(n, 6, seed=8)
        vol = vol % 6 - 3
        total += len(run({"A": "symbol", "B": "volume"}, sid, sym, price, vol, ts)[0])
        total += len(run({"B": "symbol", "A": "symbol"}, sid, sym, price, vol, ts, a="B", b="A")[0])
        total += len(run(None, sid, sym, price, vol, ts, a="C", b="A")[0])
    assert total >= 30


def test_given_ordinals_and_within_0():
    n = 2049
    sid, sym, price, vol, ts = batch(n, 30, seed=9, per=3)
    ords = 3 * np.arange(n, dtype=np.int64) + 1
    assert len(run(BY_SYMBOL, sid, sym, price, vol, ts, ordinals=ords, within=0, c2="compound")[0]) >= 3
    assert len(run(None, sid, sym, price, vol, ts, ordinals=ords, within=1)[0]) >= 30


def test_facts_see_decreasing_time_of_read_rows_only():
    n = 3000
    sid, sym, price, vol, ts = batch(n, 4, seed=10)
    t = mpat_text("A", "B", BY_SYMBOL, 5)
    assert call(t, sid, sym, price, vol, ts)[5][1] == 0
    bad = ts.copy()
    at = np.nonzero(sid == 2)[0][5]
    bad[at] = -5  # a row that is not read: any time
    assert call(t, sid, sym, price, vol, bad)[5][1] == 0
    at = np.nonzero(sid == 1)[0][700]
    bad[at] = -5
    assert call(t, sid, sym, price, vol, bad)[5][1] == 1
