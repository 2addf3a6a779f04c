"""The timeout closed form `every e1=A[c1] -> not B[c2] for W` (siddhi_amd/csrc/kernels/absent_dev.h: the clock check,
the count scan over chunks that gives every sorted position its next cancelling row, the state kernel, emission, the
instance table and the projection, behind mseq_dev.h's facts, pack and stream kernels and seq_dev.h's count kernel) run
on the CPU under the host wave emulator (tests/native/absent_emu.cpp: the same device source, one fiber per GPU thread,
on the plan the product's compiler makes of the query text), against a numpy statement of the rule
tests/test_absent_plan.py ties to the oracle, batch by batch with carried partials: every partial (a carried e1 row, or
an A row of the batch passing c1) is cancelled by a later cancelling row of its instance before its deadline, or emitted
at the first position whose clock reaches the deadline, or stays open and is carried out; outputs in order of (p,
creation ordinal of the instance, e1). The shapes are those at which the kernels can go wrong: waves, tiles, chunks of
the scan, runs across chunks, cancelling rows at a run's ends, deadlines on and next to a cancelling row's time. Test
infrastructure: no GPU; `-m "not gpu"`."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_absent_plan import C1, C2, WAITS, absent_text

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
LIB = os.path.join(NATIVE, "build", "libabsent_emu.so")
CSRC = os.path.join(HERE, "..", "siddhi_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
NAMES = ["A", "B", "C"]
CW = 7  # carried row: key, global ordinal, ts, the four attributes
BITS = lambda x: int(np.array([x], np.float64).view(np.int64)[0])


def lib():
    srcs = [os.path.join(NATIVE, "absent_emu.cpp"), os.path.join(CSRC, "compiler.cpp"),
            os.path.join(CSRC, "siddhiql", "parser.cpp")]
    deps = srcs + [os.path.join(NATIVE, "emu_fibers.h"), os.path.join(CSRC, "compiler.h"), os.path.join(CSRC, "plan.h")]
    deps += [os.path.join(CSRC, "kernels", f) for f in ("absent_dev.h", "mseq_dev.h", "seq_dev.h", "fastpath_dev.h",
                                                        "expr.h", "hd.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call([CXX if os.path.exists(CXX) else "g++", "-std=c++20", "-O2", "-g", "-fPIC", "-shared",
                               "-Wno-attributes", "-o", LIB] + srcs + ["-lpthread"])
    L = ctypes.CDLL(LIB)
    L.sm_absent_emu.restype = ctypes.c_int64
    return L


def call(app_text, sid, sym, price, vol, ts, clock_in=0, ordinals=None, obase=0, carry=None, inst=None, per=256):
    """One batch: (m, outputs (m, 5) = e1 relative to obase, timestamp, position, creation ordinal, the select's first
    value; sorted carry-out candidates; the instance table afterwards; marks; facts; err)."""
    n = len(sid)
    carry = np.zeros((0, CW), np.int64) if carry is None else np.ascontiguousarray(carry, dtype=np.int64)
    inst = np.zeros((0, 2), np.int64) if inst is None else np.asarray(inst, dtype=np.int64).reshape(-1, 2)
    room = n + len(carry) + 2
    tab = np.zeros((len(inst) + n + 1, 2), np.int64)
    tab[:len(inst)] = inst
    e1 = np.full(room, 0xDEADBEEF, np.uint32)
    tso, pos, create, vals = (np.full(room, -99, np.int64) for _ in range(4))
    cand = np.zeros(4 * room, np.int64)
    ncand, ni = ctypes.c_int64(), ctypes.c_int64()
    marks = np.zeros(6, np.int32)
    facts = np.zeros(4, np.int64)
    err = ctypes.create_string_buffer(512)
    tcol = np.arange(n, dtype=np.int64)
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    I = ctypes.c_int64
    arrs = [np.ascontiguousarray(sid, dtype=np.int32), np.ascontiguousarray(sym, dtype=np.int32),
            np.ascontiguousarray(price, dtype=np.float64), np.ascontiguousarray(vol, dtype=np.int64), tcol,
            np.ascontiguousarray(ts, dtype=np.int64)]
    ordinals = None if ordinals is None else np.ascontiguousarray(ordinals, dtype=np.int64)
    m = lib().sm_absent_emu(app_text.encode(), I(n), *[P(a) for a in arrs], I(clock_in), P(ordinals), I(obase), P(carry),
                            I(len(carry)), P(tab), I(len(inst)), ctypes.byref(ni), I(per), P(e1), P(tso), P(pos),
                            P(create), P(vals), P(cand), ctypes.byref(ncand), P(marks), P(facts), err,
                            ctypes.c_size_t(512))
    k = max(m, 0)
    assert e1[k] == 0xDEADBEEF and tso[k] == -99 and pos[k] == -99 and create[k] == -99  # nothing past the last output
    outs = np.stack([e1[:k].view(np.int32).astype(np.int64), tso[:k], pos[:k], create[:k], vals[:k]], axis=1)
    cands = sorted(tuple(int(x) for x in cand[4 * c:4 * c + 4]) for c in range(ncand.value))
    return m, outs, cands, tab[:ni.value].copy(), marks, facts, err.value


def marks_of(app_text):
    z = np.zeros(1, np.int64)
    r = call(app_text, z[:0].astype(np.int32), z[:0], z[:0], z[:0], z[:0])
    assert r[0] >= 0 or r[6].startswith(b"not marked"), r[6]  # the text compiles
    return tuple(int(x) for x in r[4])


def rule(a, b, key, sid, price, vol, ts, clock_in, gord, obase, wait, c1, c2, carry, inst, keyed):
    """One batch with its carry, partial by partial: (outputs (m, 5) as call()'s, the sorted carry-out candidates, the
    instance table afterwards)."""
    W = WAITS[wait]
    sa, sb = NAMES.index(a), NAMES.index(b)
    n = len(sid)
    clock = np.maximum.accumulate(np.maximum(ts, clock_in)) if n else ts
    table = {int(k): int(o) for k, o in inst}
    if keyed:
        for i in np.nonzero(np.isin(sid, [sa, sb]))[0]:
            table.setdefault(int(key[i]), int(gord[i]))
    cancels = (sid == sb) & C2[c2][1](price, vol)
    parts = [(int(r[0]), int(r[1]), int(r[2]), -c - 1, -1, int(r[6])) for c, r in enumerate(carry)]
    for i in np.nonzero((sid == sa) & C1[c1][1](price, vol))[0]:
        parts.append((int(key[i]), int(gord[i]), int(ts[i]), int(i), int(i), int(i)))
    outs, cand = [], []
    for place, (k, o, t1, src, after, sel) in enumerate(parts):
        d = t1 + W
        later = np.nonzero(cancels & (key == k) & (np.arange(n) > after))[0]
        if (ts[later] < d).any():
            continue
        q = int(np.searchsorted(clock, d, side="left"))
        if q < n:
            assert q > after
            outs.append((q, table[k] if keyed else -1, place, o - obase, d, sel))
        else:
            cand.append((k, o, t1, src))
    outs.sort()
    res = np.array([(o, d, q, cr, sel) for q, cr, _, o, d, sel in outs], dtype=np.int64).reshape(-1, 5)
    return res, sorted(cand), np.array(sorted(table.items()), dtype=np.int64).reshape(-1, 2)


def carried(rows):
    """rows of (key, global ordinal, ts, price): carried e1 rows, their timestamp attribute = the ordinal; sorted."""
    return np.array(sorted((k, o, t, k, BITS(p), 100, o) for k, o, t, p in rows), dtype=np.int64).reshape(-1, CW)


def check(a, b, kind, sid, sym, price, vol, ts, wait="5", c1="gt20", c2="gt45", clock_in=0, carry=None, inst=None,
          obase=0, per=256):
    keyed = kind != "flat"
    keys = None if not keyed else {a: "symbol", b: "symbol" if kind == "symbol" or a == b else "volume"}
    sid = np.asarray(sid, np.int32)
    key = np.zeros(len(sid), np.int64)
    if keyed:
        for s in {a, b}:
            mine = sid == NAMES.index(s)
            key[mine] = (np.asarray(sym) if keys[s] == "symbol" else np.asarray(vol))[mine]
    carry = np.zeros((0, CW), np.int64) if carry is None else carry
    inst = np.zeros((0, 2), np.int64) if inst is None else np.asarray(inst, np.int64).reshape(-1, 2)
    gord = obase + np.arange(len(sid), dtype=np.int64)
    text = absent_text(a, b, keys, wait, c1, c2)
    m, outs, cands, tab, marks, facts, err = call(text, sid, sym, price, vol, ts, clock_in, None, obase, carry, inst, per)
    assert m >= 0 and marks[0] == 1 and facts[1] == 0, err
    exp, ecand, etab = rule(a, b, key, sid, np.asarray(price, float), np.asarray(vol, np.int64), np.asarray(ts, np.int64),
                            clock_in, gord, obase, wait, c1, c2, carry, inst, keyed)
    np.testing.assert_array_equal(outs, exp)
    assert cands == ecand
    np.testing.assert_array_equal(tab, etab)
    return outs, cands, facts


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
def test_random_batches_with_carried_partials(n, kind):
    """Waves, blocks, tiles and chunks of 256 positions: one more and one fewer than each; carried partials in front of
    their keys' runs, of a key without rows here, and one that is due at the batch's first row."""
    sid, sym, price, vol, ts = random_batch(n, 6, n)
    keyed = kind != "flat"
    ks = [-2, 0, 3, 9] if keyed else [0]  # (key 9 has no rows in the batch)
    carry = carried([(k, 50 + 3 * j + r, 96 + r, 30.0 + r) for j, k in enumerate(ks) for r in range(3)])
    inst = [(k, 10 + j) for j, k in enumerate(sorted(ks))] if keyed else None
    outs, cands, facts = check("A", "B", kind, sid, sym, price, vol, ts, "5", carry=carry, inst=inst, clock_in=99,
                               obase=1000)
    if n >= 255:
        assert len(outs) > 10 and facts[3] > 0
        assert not keyed or (outs[:, 0] < 0).any()  # key 9's carried partials fall due: no row of it cancels them


@pytest.mark.parametrize("kind", ["flat", "symbol"])
@pytest.mark.parametrize("run", [1, 63, 64, 65])
def test_runs_of_a_few_rows(run, kind):
    """Every key has `run` rows (flat: the batch has), the last or the first of them a cancelling row."""
    K = 1 if kind == "flat" else 5
    n = run * K
    for where in ("last", "first", "none"):
        sid = np.zeros(n, np.int32)
        sym = np.tile(np.arange(K, dtype=np.int32), run)
        price = np.full(n, 30.0)
        vol = np.zeros(n, np.int64)
        ts = 100 + np.arange(n, dtype=np.int64) // max(K, 2)
        at = {"last": np.arange(n - K, n), "first": np.arange(0, K), "none": np.arange(0)}[where]
        sid[at] = 1
        price[at] = 50.0
        outs, cands, _ = check("A", "B", kind, sid, sym, price, vol, ts, "2" if where == "last" else "5")
        if where == "none" and run > 1:
            assert len(outs) + len(cands) == n and len(cands) > 0


def test_one_run_across_every_chunk():
    """Unkeyed, 2000 read rows in chunks of 256: cancelling rows only in the last chunk, only in the first, and none."""
    n = 2000
    for lo, hi in ((1900, 1910), (3, 5), (0, 0)):
        sid = np.zeros(n, np.int32)
        price = np.full(n, 30.0)
        sid[lo:hi] = 1
        price[lo:hi] = 50.0
        ts = 100 + np.arange(n, dtype=np.int64) // 700  # nobody is due before the last rows without a cancelling row
        outs, cands, facts = check("A", "B", "flat", sid, np.zeros(n, np.int32), price, np.zeros(n, np.int64), ts, "5")
        assert facts[3] == hi - lo
        if hi == 0:
            assert len(cands) == n and len(outs) == 0
        if lo == 1900:
            assert len(outs) == 0 and len(cands) == n - hi  # every row before the cancelling ones is cancelled


@pytest.mark.parametrize("kind", ["flat", "symbol"])
def test_a_cancelling_row_at_and_next_to_the_deadline(kind):
    """W = 5, e1 at time 100: a B row at 104 cancels, a B row at 105 is too late (and is itself the due point)."""
    for tb, cancelled in ((104, True), (105, False)):
        sid = np.array([0, 2, 1, -1], np.int32)
        sym = np.array([1, 1, 1, 0], np.int32)
        price = np.array([30.0, 0.0, 50.0, 0.0])
        ts = np.array([100, 101, tb, 110], np.int64)
        outs, cands, _ = check("A", "B", kind, sid, sym, price, np.zeros(4, np.int64), ts, "5")
        assert len(outs) == (0 if cancelled else 1) and cands == []
        if not cancelled:
            assert outs[0].tolist()[:3] == [0, 105, 2]


@pytest.mark.parametrize("kind", ["flat", "symbol"])
def test_due_points(kind):
    """On the batch's last row; on a heartbeat; on a row of the unread stream; none yet (carried out); and a batch of
    heartbeats only, at which carried partials of several keys fall due at one position in creation order."""
    sid = np.array([0, 0, -1, 2, 0, 1], np.int32)
    sym = np.array([1, 2, 0, 0, 1, 3], np.int32)
    price = np.array([30.0, 31.0, 0.0, 0.0, 32.0, 10.0])
    ts = np.array([100, 101, 105, 106, 107, 112], np.int64)
    outs, cands, _ = check("A", "B", kind, sid, sym, price, np.zeros(6, np.int64), ts, "5")
    assert outs[:, :3].tolist() == [[0, 105, 2], [1, 106, 3], [4, 112, 5]] and cands == []
    outs, cands, _ = check("A", "B", kind, sid[:5], sym[:5], price[:5], np.zeros(5, np.int64), ts[:5], "5")
    assert len(outs) == 2 and len(cands) == 1
    keyed = kind != "flat"
    carry = carried([(k if keyed else 0, 10 + j, 90 + j, 30.0) for j, k in enumerate([7, 3, 5, 3])])
    inst = [(3, 2), (5, 0), (7, 1)] if keyed else None
    hb = np.full(4, -1, np.int32)
    z = np.zeros(4)
    outs, cands, _ = check("A", "B", kind, hb, z, z, z, np.array([91, 92, 99, 99], np.int64), "5", carry=carry, inst=inst,
                           clock_in=90, obase=100)
    assert len(outs) == 4 and cands == [] and set(outs[:, 2].tolist()) == {2}
    if keyed:  # key 5 was created first, then 7, then 3 (its two partials in order)
        assert outs[:, 0].tolist() == [12 - 100, 10 - 100, 11 - 100, 13 - 100]


@pytest.mark.parametrize("kind", ["flat", "symbol"])
def test_the_same_stream_and_no_filters(kind):
    sid, sym, price, vol, ts = random_batch(1500, 4, 5, step=4)
    outs, _, _ = check("A", "A", kind, sid, sym, price, vol, ts, "2")
    assert len(outs) > 10
    check("A", "A", kind, sid, sym, price, vol, ts, "2", "none", "none")
    check("A", "B", kind, sid, sym, price, vol, ts, "5", "none", "compound")


def test_a_read_row_below_the_clock_is_reported():
    sid, sym, price, vol, ts = random_batch(600, 4, 9)
    text = absent_text("A", "B", None, "5")
    assert call(text, sid, sym, price, vol, ts, clock_in=0)[5][1] == 0
    assert call(text, sid, sym, price, vol, ts, clock_in=int(ts[0]) + 1)[5][1] == 1  # against the app's clock
    back = ts.copy()
    i = int(np.nonzero(sid == 2)[0][5])
    back[i] -= 50  # an unread row: fine
    assert call(text, sid, sym, price, vol, back)[5][1] == 0
    i = int(np.nonzero(sid == 1)[0][5])
    back[i] = back[i - 1] - 1
    assert call(text, sid, sym, price, vol, back)[5][1] == 1
