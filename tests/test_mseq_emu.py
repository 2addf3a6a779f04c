"""The adjacent-run closed form over several streams (siddhi_amd/csrc/kernels/mseq_dev.h: facts, pack, stream gather and
link kernels, with seq_dev.h's seqk keep, count and emit kernels behind them) run on the CPU under the host wave emulator
(tests/native/mseq_emu.cpp: the same device source, one fiber per GPU thread, on the plan the product's compiler makes
of the query text), against a numpy statement of the rule tests/test_mseq_plan.py ties to the oracle: among the rows of
the streams the query reads (heartbeat rows and rows of other streams do not exist), a row j of an instance with k - 1
predecessors (the first of a batch taken from the tail of the instance's carried rows) emits the k-tuple iff every
member is on its element's stream and every condition and `within` holds; outputs in order of j; every instance carries
its last min(k - 1, read rows so far) rows. Also the compiler's envelope for the mark. Test infrastructure: no GPU;
`-m "not gpu"`."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
LIB = os.path.join(NATIVE, "build", "libmseq_emu.so")
CSRC = os.path.join(HERE, "..", "siddhi_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
NAMES = ["A", "B", "C"]
ATTRS = "(symbol int, price double, volume long, timestamp long)"
SCHEMA = "".join(f"define stream {s} {ATTRS}; " for s in NAMES)
CW = 8  # carried row: key, global ordinal, ts, the four attributes, the row's stream


def lib():
    srcs = [os.path.join(NATIVE, "mseq_emu.cpp"), os.path.join(CSRC, "compiler.cpp"),
            os.path.join(CSRC, "siddhiql", "parser.cpp")]
    deps = srcs + [os.path.join(NATIVE, "emu_fibers.h"), os.path.join(CSRC, "compiler.h"), os.path.join(CSRC, "plan.h")]
    deps += [os.path.join(CSRC, "kernels", f) for f in ("mseq_dev.h", "seq_dev.h", "fastpath_dev.h", "expr.h", "hd.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call([CXX if os.path.exists(CXX) else "g++", "-std=c++20", "-O2", "-g", "-fPIC", "-shared",
                               "-Wno-attributes", "-o", LIB] + srcs + ["-lpthread"])
    L = ctypes.CDLL(LIB)
    L.sm_mseq_emu.restype = ctypes.c_int64
    return L


def text(pattern, keys=None, withins=None):
    """c1 = price > 20; cm = price > e(m-1).price - 25.0 and volume != e1.volume; keys {stream: attribute} (None:
    unpartitioned); withins {m: T} (m 1-based)."""
    withins = withins or {}
    els = [f"every e1={pattern[0]}[price>20]"]
    for m in range(2, len(pattern) + 1):
        w = f" within {withins[m]} milliseconds" if m in withins else ""
        els.append(f"e{m}={pattern[m - 1]}[price > e{m - 1}.price - 25.0 and volume != e1.volume]{w}")
    q = f"@info(name='q') from {', '.join(els)} select e1.timestamp as i insert into Out;"
    if keys is None:
        return SCHEMA + q
    return SCHEMA + "partition with (" + ", ".join(f"{a} of {s}" for s, a in keys.items()) + f") begin {q} end;"


def row_keys(pattern, keys, sid, sym, vol):
    """The instance key of every row: the key attribute of its own stream (0 for a row that is not read)."""
    key = np.zeros(len(sid), np.int64)
    if keys is not None:
        for s in set(pattern):
            mine = sid == NAMES.index(s)
            key[mine] = (sym if keys[s] == "symbol" else vol)[mine]
    return key


def rule(pattern, key, sid, price, vol, ts, gord, obase, withins, carry):
    """(tuples relative to obase in order of j, sorted carry-out rows (key, global ordinal, ts, source))."""
    k = len(pattern)
    want = [NAMES.index(s) for s in pattern]
    rows = np.nonzero(np.isin(sid, sorted(set(want))))[0]
    nc = len(carry)
    akey = np.concatenate([carry[:, 0], key[rows]])
    aord = np.concatenate([carry[:, 1], gord[rows]])
    ats = np.concatenate([carry[:, 2], ts[rows]])
    aprice = np.concatenate([carry[:, 4].copy().view(np.float64), price[rows]])
    avol = np.concatenate([carry[:, 5], vol[rows]])
    asid = np.concatenate([carry[:, 7], sid[rows].astype(np.int64)])
    asrc = np.concatenate([-np.arange(nc, dtype=np.int64) - 1, rows.astype(np.int64)])
    order = np.lexsort((aord, akey))  # by (key, ordinal): the carried rows precede the batch's (older ordinals)
    ks = akey[order]
    N = len(rows) + nc
    u = np.arange(k - 1, N)
    u = u[(ks[u] == ks[u - (k - 1)]) & (asrc[order[u]] >= 0)] if N >= k else u[:0]
    M = [order[u - (k - 1) + m] for m in range(k)]
    ok = aprice[M[0]] > 20
    for m in range(k):
        ok &= asid[M[m]] == want[m]
    for m in range(1, k):
        ok &= (aprice[M[m]] > aprice[M[m - 1]] - 25.0) & (avol[M[m]] != avol[M[0]])
        if m + 1 in withins:
            ok &= ats[M[m]] - ats[M[m - 1]] <= withins[m + 1]
    t = np.stack([(aord[x] - obase)[ok] for x in M], axis=1).reshape(-1, k)
    t = t[np.argsort(t[:, k - 1], kind="stable")]
    last = np.ones(N, bool)  # carry-out: the last k - 1 rows of every (key, ordinal) run
    if N > k - 1:
        last[:N - (k - 1)] = ks[:N - (k - 1)] != ks[k - 1:]
    out = sorted((int(akey[i]), int(aord[i]), int(ats[i]), int(asrc[i])) for i in order[last])
    return t, out, len(rows)


def call(app_text, sid, sym, price, vol, ts, ordinals=None, obase=0, carry=None):
    n = len(sid)
    carry = np.zeros((0, CW), np.int64) if carry is None else np.ascontiguousarray(carry, dtype=np.int64)
    k_max = 8
    tuples = np.full(k_max * n + 2, 0xDEADBEEF, np.uint32)
    cand = np.zeros(4 * (n + len(carry)) + 4, np.int64)
    ncand = ctypes.c_int64()
    marks = np.zeros(3, np.int32)
    facts = np.zeros(9, np.int64)
    err = ctypes.create_string_buffer(512)
    tcol = np.arange(n, dtype=np.int64)
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    arrs = [np.ascontiguousarray(sid, dtype=np.int32), np.ascontiguousarray(sym, dtype=np.int32),
            np.ascontiguousarray(price, dtype=np.float64), np.ascontiguousarray(vol, dtype=np.int64), tcol,
            np.ascontiguousarray(ts, dtype=np.int64)]
    m = lib().sm_mseq_emu(app_text.encode(), ctypes.c_int64(n), *[P(a) for a in arrs], P(ordinals), ctypes.c_int64(obase),
                          P(carry), ctypes.c_int64(len(carry)), P(tuples), P(cand), ctypes.byref(ncand), P(marks),
                          P(facts), err, ctypes.c_size_t(512))
    return m, tuples, cand, ncand.value, marks, facts, err.value


def run(pattern, keys, sid, sym, price, vol, ts, ordinals=None, obase=0, withins=None, carry=None):
    n, k = len(sid), len(pattern)
    carry = np.zeros((0, CW), np.int64) if carry is None else np.ascontiguousarray(carry, dtype=np.int64)
    m, tuples, cand, ncand, marks, facts, err = call(text(pattern, keys, withins), sid, sym, price, vol, ts, ordinals,
                                                     obase, carry)
    assert m >= 0 and marks[0] == k, err
    gord = obase + np.arange(n, dtype=np.int64) if ordinals is None else ordinals
    key = row_keys(pattern, keys, sid, np.asarray(sym, dtype=np.int64), np.asarray(vol, dtype=np.int64))
    exp, exp_cand, nread = rule(pattern, key, np.asarray(sid), np.asarray(price, dtype=np.float64),
                                np.asarray(vol, dtype=np.int64), np.asarray(ts, dtype=np.int64), gord, obase,
                                withins or {}, carry)
    assert facts[0] == nread
    if nread == 0:
        assert m == 0  # the host entry returns before the carry is read: the carried rows wait
        return exp
    got = tuples[:k * m].view(np.int32).astype(np.int64).reshape(-1, k)
    np.testing.assert_array_equal(got, exp)
    assert tuples[k * m] == 0xDEADBEEF  # nothing written past the last tuple
    got_cand = sorted(tuple(int(x) for x in cand[4 * c:4 * c + 4]) for c in range(ncand))
    assert got_cand == exp_cand
    return exp


def batch(n, K, seed=0, streams=(0, 1, 2, -1), pattern=None, phase=lambda key: 0):
    """Random rows over the given streams (-1: heartbeat rows). With a pattern: a key's rows mostly follow it, from
    position phase(key) on."""
    rng = np.random.default_rng(seed * 1000003 + n * 31 + K)
    sym = rng.integers(0, K, n).astype(np.int32) - 3  # negative keys too
    price = np.round(20.0 + rng.random(n) * 40.0, 1)
    vol = rng.integers(0, 50, n).astype(np.int64)
    ts = np.arange(n, dtype=np.int64) // 40
    sid = np.array(streams, np.int32)[rng.integers(0, len(streams), n)]
    if pattern is not None:
        want = np.array([NAMES.index(s) for s in pattern], np.int32)
        seen = {}
        for i in range(n):
            c = seen.get(int(sym[i]), phase(int(sym[i])))
            if rng.random() >= 0.2:
                sid[i] = want[c % len(want)]
            if sid[i] in want:
                seen[int(sym[i])] = c + 1
    return sid, sym, price, vol, ts


SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 3100]
BY_SYMBOL = {"A": "symbol", "B": "symbol", "C": "symbol"}
PATTERNS = {"AB": ["A", "B"], "ABA": ["A", "B", "A"], "k8": ["A", "B", "A", "A", "B", "C", "A", "B"]}


@pytest.mark.parametrize("K", [None, 1, 5, 60])
@pytest.mark.parametrize("name", list(PATTERNS))
def test_link_and_compaction_follow_the_rule(name, K):
    """Below, at and above k, a wave, a tile (1024 rows) and three tiles; unkeyed and keyed; the third stream of the
    feed is not read by `A, B` and `A, B, A`, and one row in four is a heartbeat."""
    pattern = PATTERNS[name]
    total = 0
    for n in SIZES:
        sid, sym, price, vol, ts = batch(n, K or 1, pattern=pattern)
        keys = None if K is None else {s: "symbol" for s in set(pattern)}
        total += len(run(pattern, keys, sid, sym, price, vol, ts, withins={len(pattern): 2}))
    assert total > 0


def test_every_row_read_and_unkeyed_takes_no_pack():
    """Only A and B rows in the feed, unkeyed: the link reads the batch's stream column in row order."""
    total = 0
    for n in SIZES:
        sid, sym, price, vol, ts = batch(n, 1, seed=3, streams=(0, 1))
        total += len(run(["A", "B"], None, sid, sym, price, vol, ts))
        total += len(run(["A", "B", "A"], None, sid, sym, price, vol, ts, withins={2: 1}))
    assert total > 0


def test_no_read_row_and_fewer_than_k():
    n = 300
    sid, sym, price, vol, ts = batch(n, 5, seed=4, streams=(2, -1))
    carry = np.array([[0, 90, 1, 0, np.array([30.0]).view(np.int64)[0], 7, 90, 0]], np.int64)
    for keys in (None, {"A": "symbol", "B": "symbol"}):
        assert len(run(["A", "B"], keys, sid, sym, price, vol, ts, obase=100, carry=carry)) == 0
    sid[250] = 1  # one read row: it completes the carried A
    sym[250] = 0
    vol[250] = 8
    price[250] = 31.0
    for keys in (None, {"A": "symbol", "B": "symbol"}):
        exp = run(["A", "B"], keys, sid, sym, price, vol, ts, obase=100, carry=carry)
        np.testing.assert_array_equal(exp, [[-10, 250]])
        assert len(run(["A", "B", "A"], keys, sid, sym, price, vol, ts, obase=100, carry=carry)) == 0


def test_per_stream_key_attributes():
    """B's instances are keyed by its volume, A's by its symbol."""
    keys = {"A": "symbol", "B": "volume"}
    total = 0
    for n in (65, 1025, 3100):
        sid, sym, price, vol, ts = batch(n, 6, seed=8)
        vol = vol % 6 - 3
        total += len(run(["A", "B"], keys, sid, sym, price, vol, ts))
        total += len(run(["A", "B", "A"], keys, sid, sym, price, vol, ts))
    assert total > 0


@pytest.mark.parametrize("name", ["AB", "ABA", "k8"])
def test_runs_straddle_wave_and_tile_boundaries(name):
    """Keys in blocks of 1 .. k read rows, shifted so that runs of every length 2 .. k cross the packed positions 64 (a
    wave) and 1024 (a tile); unread rows lie between a run's members in arrival order."""
    pattern = PATTERNS[name]
    k = len(pattern)
    want = np.array([NAMES.index(s) for s in pattern], np.int32)
    seen = set()
    for shift in range(k * (k + 1) // 2):
        lens = ([1] * shift + list(range(1, k + 1)) * 400)
        keys = np.repeat(np.arange(len(lens), dtype=np.int32), lens)[:2100]
        pos = np.concatenate([np.arange(L) for L in lens])[:2100]
        nr = len(keys)
        rng = np.random.default_rng(shift + 10 * k)
        # arrival slots unrelated to the key order; a key's own rows keep their order, so that they follow the chain
        rank = rng.permutation(nr)
        arrive = rank[np.lexsort((rank, keys))]
        n = nr + nr // 3
        sid = np.full(n, -1, np.int32)
        sym = np.zeros(n, np.int32)
        place = np.sort(rng.choice(n, nr, replace=False))  # the other rows: heartbeats and (for two-stream chains) C rows
        sid[place[arrive]] = want[pos % k]
        sym[place[arrive]] = keys
        if "C" not in pattern:
            sid[(sid == -1) & (rng.random(n) < 0.5)] = 2
        price = 21.0 + rng.random(n)          # every condition holds: the run's length and streams decide
        vol = np.arange(n, dtype=np.int64)
        ts = np.arange(n, dtype=np.int64)
        exp = run(pattern, {s: "symbol" for s in set(pattern)}, sid, sym, price, vol, ts)
        assert len(exp) > 0
        ends = np.nonzero(np.diff(keys) != 0)[0] + 1
        seen |= {(b, int(e - s)) for s, e in zip(np.r_[0, ends], np.r_[ends, nr]) for b in (64, 1024) if s < b < e}
    assert seen >= {(b, L) for b in (64, 1024) for L in range(2, k + 1)}


@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("name", ["AB", "ABA", "k8"])
def test_run_heads_take_members_from_the_carry(name, keyed):
    """Keys hold 0 .. k - 1 carried rows whose streams continue the chain (and idle keys); the first read rows of a key's
    run take 1 .. k - 1 members from the carry's tail (negative relative ordinals), or have no tuple when the carry is
    too short or a carried row is on the wrong stream. Keys with e < k - 1 read rows keep their newest k - 1 - e rows."""
    pattern = PATTERNS[name]
    k = len(pattern)
    want = [NAMES.index(s) for s in pattern]
    n, K = 1500, 40 if keyed else 1
    # 0 .. k - 1 carried rows per key: the chain's first positions, which the key's rows of the batch continue
    have_of = lambda key: k - 1 if key in (7, 9) or not keyed else (key + 3) % k
    sid, sym, price, vol, ts = batch(n, K, seed=5, pattern=pattern, phase=have_of)
    price = 21.0 + price / 100.0  # conditions hold: membership and streams decide
    vol = np.arange(n, dtype=np.int64) + 1000
    ts = ts + 100
    if keyed:
        sym[sym == 7] = 8                    # key 7 is idle: its carried rows all stay
        few = np.nonzero(sym == 9)[0][1:]    # key 9 has one row: it keeps k - 2 carried rows
        sym[few] = 10
        ckeys = list(range(-3, K - 3))
        keys = {s: "symbol" for s in set(pattern)}
    else:
        sym[:] = 0
        ckeys = [0]
        keys = None
    rows, o = [], 5000 - 1000
    for key in ckeys:
        for r in range(have_of(key)):
            s = want[0] if keyed and key % 7 == 4 else want[r]  # (one key in seven: carried rows on a wrong stream)
            rows.append([key, o, 99, key, np.array([22.0 + r / 10.0]).view(np.int64)[0], r, o, s])
            o += 1
    carry = np.array(rows, np.int64).reshape(-1, CW)
    exp = run(pattern, keys, sid, sym, price, vol, ts, obase=5000, carry=carry)
    from_carry = (exp < 0).sum(axis=1)
    assert (from_carry > 0).any()
    if keyed:
        key = row_keys(pattern, keys, sid, sym.astype(np.int64), vol)
        _, cand, _ = rule(pattern, key, sid, price, vol, ts, 5000 + np.arange(n), 5000, {}, carry)
        assert sum(1 for c in cand if c[0] == 7 and c[3] < 0) == k - 1
        assert sum(1 for c in cand if c[0] == 9 and c[3] < 0) == max(k - 2, 0)
    run(pattern, keys, sid, sym, price, vol, ts, obase=5000, withins={2: 0, k: 1}, carry=carry)  # carried times count


def test_given_ordinals():
    n = 3000
    sid, sym, price, vol, ts = batch(n, 30, seed=9, pattern=["A", "B", "A"])
    ords = 3 * np.arange(n, dtype=np.int64) + 1
    assert len(run(["A", "B", "A"], BY_SYMBOL_AB, sid, sym, price, vol, ts, ordinals=ords, withins={3: 1})) > 0
    assert len(run(["A", "B"], None, sid, sym, price, vol, ts, ordinals=ords, withins={2: 1})) > 0


BY_SYMBOL_AB = {"A": "symbol", "B": "symbol"}


def test_facts_see_the_read_rows_only():
    """Event time and ordinals are compared between one read row and the previous read row, however many rows of other
    streams lie between them (the same wave, an earlier wave, an earlier tile); rows that are not read may hold
    anything. The ranges are those of the read rows."""
    n = 4000
    rng = np.random.default_rng(12)
    sid = np.where(rng.random(n) < 0.5, 2, -1).astype(np.int32)  # C rows and heartbeats
    read_at = np.array([5, 6, 70, 71, 900, 2100, 2101, 3999])
    sid[read_at] = [0, 1, 0, 1, 0, 1, 0, 1]
    sym = rng.integers(-9, 9, n).astype(np.int32)
    sym[read_at] = [3, -2, 3, 5, 5, -2, 3, 3]
    price = np.full(n, 30.0)
    vol = np.arange(n, dtype=np.int64)
    ts = rng.integers(0, 10 ** 6, n).astype(np.int64)  # rows that are not read: any time
    ords = rng.integers(0, 10 ** 6, n).astype(np.int64)
    ts[read_at] = [10, 10, 11, 20, 20, 25, 30, 31]
    ords[read_at] = [7, 9, 100, 101, 5000, 5001, 9000, 9001]
    t = text(["A", "B"], BY_SYMBOL_AB, {2: 50})

    def facts(ts_, ords_):
        m, _, _, _, marks, f, err = call(t, sid, sym, price, vol, ts_, ords_, obase=5)
        assert m >= 0 and marks[0] == 2, err
        return list(f)

    assert facts(ts, ords) == [8, 0, 0, -2, 5, 10, 31, 2, 8996]
    for at in (6, 70, 900, 2100, 3999):  # the previous read row: 1, 64, 829, 1200 and 1898 rows back
        bad = ts.copy()
        bad[at] = ts[read_at[list(read_at).index(at) - 1]] - 1
        assert facts(bad, ords)[1] == 1
        bad = ords.copy()
        bad[at] = ords[read_at[list(read_at).index(at) - 1]]
        assert facts(ts, bad)[2] == 1


def marks_of(app_text):
    """(fast_seq_ms, fast_seq_k, fast_seq_adjacent) of the plan the compiler makes."""
    z = np.zeros(1, np.int64)
    return tuple(int(x) for x in call(app_text, z[:0].astype(np.int32), z[:0], z[:0], z[:0], z[:0])[4])


def test_the_compilers_envelope():
    """The mark, and next to it what the same-stream marks are: on the parent commit every text below compiles to
    fast_seq_k = 0 and fast_seq_adjacent = false, except the all-one-stream chains (k = 3: fast_seq_k = 3; k = 2:
    fast_seq_adjacent)."""
    q = lambda body, sel="e1.timestamp as i": SCHEMA + f"@info(name='q') from {body} select {sel} insert into Out;"
    part = lambda with_, body: SCHEMA + f"partition with ({with_}) begin @info(name='q') from {body} " \
                                        "select e1.timestamp as i insert into Out; end;"
    assert marks_of(text(["A", "B"])) == (2, 0, 0)
    assert marks_of(text(["A", "B"], BY_SYMBOL_AB, {2: 3})) == (2, 0, 0)
    assert marks_of(text(["A", "B", "A"], {"A": "symbol", "B": "volume"}, {2: 1, 3: 3})) == (3, 0, 0)
    assert marks_of(text(PATTERNS["k8"], BY_SYMBOL)) == (8, 0, 0) and marks_of(text(PATTERNS["k8"])) == (8, 0, 0)
    assert marks_of(q("every e1=A[price>20], e2=B[price>e1.price] within 1 sec", "e1.price as p, e2.price as r")) == (2, 0, 0)
    # all on one stream: the same-stream paths keep their plans
    assert marks_of(text(["A", "A", "A"])) == (0, 3, 0)
    assert marks_of(text(["A", "A"])) == (0, 0, 1)
    assert marks_of(text(["A", "A"], {"A": "symbol"})) == (0, 0, 1)
    # outside: 9 states, a count, a logical element, no leading every, a within on e1, a having, a pattern
    assert marks_of(text(PATTERNS["k8"] + ["A"])) == (0, 0, 0)
    assert marks_of(q("every e1=A, e2=B+, e3=A")) == (0, 0, 0)
    assert marks_of(q("every e1=A, e2=B<1:3>")) == (0, 0, 0)
    assert marks_of(q("every e1=A, (e2=B and e3=C)")) == (0, 0, 0)
    assert marks_of(q("every e1=A, (e2=B or e3=C), e4=A")) == (0, 0, 0)
    assert marks_of(q("e1=A[price>20], e2=B[price>e1.price]")) == (0, 0, 0)
    assert marks_of(q("every e1=A[price>20] within 5 milliseconds, e2=B")) == (0, 0, 0)
    assert marks_of(q("every e1=A, e2=B", "e1.timestamp as i having i > 3")) == (0, 0, 0)
    assert marks_of(q("every e1=A[price>20] -> e2=B[price>e1.price]")) == (0, 0, 0)
    # partition keys: one INT / LONG attribute per read stream, else no mark
    assert marks_of(part("symbol of A, volume of B", "every e1=A, e2=B")) == (2, 0, 0)
    assert marks_of(part("symbol + 1 of A, symbol of B", "every e1=A, e2=B")) == (0, 0, 0)
    named = "".join(f"define stream {s} (name string, price double, volume long, timestamp long); " for s in "AB")
    assert marks_of(named + "partition with (name of A, name of B) begin @info(name='q') from every e1=A, e2=B "
                    "select e1.timestamp as i insert into Out; end;") == (0, 0, 0)
    # streams of different schemas
    other = "define stream A (symbol int, price double); define stream B (symbol int, price float); "
    assert marks_of(other + "@info(name='q') from every e1=A, e2=B select e1.price as p insert into Out;") == (0, 0, 0)
