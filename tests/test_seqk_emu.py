"""The adjacent-run closed form of `every e1=S[c1], ..., ek=S[ck]` (siddhi_amd/csrc/kernels/seq_dev.h: seqk link, keep,
count and emit kernels) run on the CPU under the host wave emulator (tests/native/seqk_emu.cpp: the same device
source, one fiber per GPU thread, on the plan the product's compiler makes of the query text), against a numpy
statement of the rule tests/test_seqk_plan.py ties to the oracle: an event j of an instance with k - 1 predecessors
(the previous k - 1 events of the instance, the first of a batch taken from the tail of the instance's carried rows)
emits the k-tuple iff every condition and every `within` (against the previous element) holds; outputs in order of j;
every instance carries its last min(k - 1, events so far) events. Test infrastructure: no GPU; `-m "not gpu"`."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
LIB = os.path.join(NATIVE, "build", "libseqk_emu.so")
CSRC = os.path.join(HERE, "..", "siddhi_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
SCHEMA = "define stream StockStream (symbol int, price double, volume long, timestamp long); "
CW = 7  # carried row: key, global ordinal, ts, then the four attributes


def lib():
    srcs = [os.path.join(NATIVE, "seqk_emu.cpp"), os.path.join(CSRC, "compiler.cpp"),
            os.path.join(CSRC, "siddhiql", "parser.cpp")]
    deps = srcs + [os.path.join(NATIVE, "emu_fibers.h"), os.path.join(CSRC, "compiler.h"), os.path.join(CSRC, "plan.h")]
    deps += [os.path.join(CSRC, "kernels", f) for f in ("seq_dev.h", "fastpath_dev.h", "expr.h", "hd.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call([CXX if os.path.exists(CXX) else "g++", "-std=c++20", "-O2", "-g", "-fPIC", "-shared",
                               "-Wno-attributes", "-o", LIB] + srcs + ["-lpthread"])
    L = ctypes.CDLL(LIB)
    L.sm_seqk_emu.restype = ctypes.c_int64
    return L


def text(k, keyed, withins=None):
    """c1 = price > 20; cm = price > e(m-1).price - 25.0 and volume != e1.volume; withins {m: T} (m 1-based)."""
    withins = withins or {}
    els = ["every e1=StockStream[price>20]"]
    for m in range(2, k + 1):
        w = f" within {withins[m]} milliseconds" if m in withins else ""
        els.append(f"e{m}=StockStream[price > e{m - 1}.price - 25.0 and volume != e1.volume]{w}")
    q = f"@info(name='q') from {', '.join(els)} select e1.timestamp as i insert into Out;"
    return SCHEMA + (f"partition with (symbol of StockStream) begin {q} end;" if keyed else q)


def rule(k, keys, price, vol, ts, gord, obase, withins, carry):
    """(tuples relative to obase in order of j, sorted carry-out rows (key, global ordinal, ts, source))."""
    n = len(price)
    key = np.zeros(n, np.int64) if keys is None else keys.astype(np.int64)
    # the carried rows in front of the batch, as events -nc .. -1 (source -(c) - 1 = index - nc ... mapped below)
    nc = len(carry)
    akey = np.concatenate([carry[:, 0], key])
    aord = np.concatenate([carry[:, 1], gord])
    ats = np.concatenate([carry[:, 2], ts])
    aprice = np.concatenate([carry[:, 4].copy().view(np.float64), price])
    avol = np.concatenate([carry[:, 5], vol])
    asrc = np.concatenate([-np.arange(nc, dtype=np.int64) - 1, np.arange(n, dtype=np.int64)])
    order = np.lexsort((aord, akey))  # by (key, ordinal): the carried rows precede the batch's (older ordinals)
    ks = akey[order]
    N = n + nc
    u = np.arange(k - 1, N)
    u = u[(ks[u] == ks[u - (k - 1)]) & (asrc[order[u]] >= 0)] if N >= k else u[:0]
    M = [order[u - (k - 1) + m] for m in range(k)]
    ok = aprice[M[0]] > 20
    for m in range(1, k):
        ok &= (aprice[M[m]] > aprice[M[m - 1]] - 25.0) & (avol[M[m]] != avol[M[0]])
        if m + 1 in withins:
            ok &= ats[M[m]] - ats[M[m - 1]] <= withins[m + 1]
    t = np.stack([(aord[x] - obase)[ok] for x in M], axis=1).reshape(-1, k)
    t = t[np.argsort(t[:, k - 1], kind="stable")]
    # carry-out: the last k - 1 rows of every (key, ordinal) run
    last = np.ones(N, bool)
    if N > k - 1:
        last[:N - (k - 1)] = ks[:N - (k - 1)] != ks[k - 1:]
    out = sorted((int(akey[i]), int(aord[i]), int(ats[i]), int(asrc[i])) for i in order[last])
    return t, out


def run(k, keys, price, vol, ts, ordinals=None, obase=0, withins=None, carry=None):
    n = len(price)
    carry = np.zeros((0, CW), np.int64) if carry is None else np.ascontiguousarray(carry, dtype=np.int64)
    nc = len(carry)
    tuples = np.full(k * n + 2, 0xDEADBEEF, np.uint32)
    cand = np.zeros(4 * (n + nc) + 4, np.int64)
    ncand, kout = ctypes.c_int64(), ctypes.c_int32()
    err = ctypes.create_string_buffer(512)
    price = np.ascontiguousarray(price, dtype=np.float64)
    vol = np.ascontiguousarray(vol, dtype=np.int64)
    ts = np.ascontiguousarray(ts, dtype=np.int64)
    tcol = np.arange(n, dtype=np.int64)
    sym = np.zeros(n, np.int32) if keys is None else np.ascontiguousarray(keys, dtype=np.int32)
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    m = lib().sm_seqk_emu(text(k, keys is not None, withins).encode(), ctypes.c_int64(n), ctypes.c_int(keys is not None),
                          P(sym), P(price), P(vol), P(tcol), P(ts), P(ordinals), ctypes.c_int64(obase), P(carry),
                          ctypes.c_int64(nc), P(tuples), P(cand), ctypes.byref(ncand), ctypes.byref(kout), err,
                          ctypes.c_size_t(512))
    assert m >= 0 and kout.value == k, err.value
    gord = obase + np.arange(n, dtype=np.int64) if ordinals is None else ordinals
    exp, exp_cand = rule(k, keys, price, vol, ts, gord, obase, withins or {}, carry)
    got = tuples[:k * m].view(np.int32).astype(np.int64).reshape(-1, k)
    np.testing.assert_array_equal(got, exp)
    assert tuples[k * m] == 0xDEADBEEF  # nothing written past the last tuple
    got_cand = sorted(tuple(int(x) for x in cand[4 * c:4 * c + 4]) for c in range(ncand.value))
    assert got_cand == exp_cand
    return exp


def batch(n, K, seed=0):
    rng = np.random.default_rng(seed * 1000003 + n * 31 + K)
    keys = rng.integers(0, K, n).astype(np.int32) - 3  # negative keys too
    price = np.round(rng.random(n) * 60.0, 1)
    vol = rng.integers(0, 50, n)
    ts = np.arange(n, dtype=np.int64) // 40
    return keys, price, vol, ts


def sizes(k):
    return sorted({1, 2, k - 1, k, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049})


@pytest.mark.parametrize("K", [None, 1, 5, 60])
@pytest.mark.parametrize("k", [3, 4, 8])
def test_link_and_compaction_follow_the_rule(k, K):
    """Below, at and above k, a wave, a tile (1024 rows) and two tiles; unkeyed and keyed."""
    total = 0
    for n in sizes(k):
        keys, price, vol, ts = batch(n, K or 1)
        total += len(run(k, None if K is None else keys, price, vol, ts, withins={k: 2}))
    assert total > 0


@pytest.mark.parametrize("k", [3, 5])
def test_more_keys_than_events(k):
    keys, price, vol, ts = batch(300, 100000)
    assert len(run(k, keys, price, vol, ts)) == 0


@pytest.mark.parametrize("k", [3, 4, 8])
def test_runs_straddle_wave_and_tile_boundaries(k):
    """Keys in blocks of 1 .. k events, shifted so that runs of every length 2 .. k cross the sorted positions 64 (a
    wave) and 1024 (a tile)."""
    seen = set()
    for shift in range(k * (k + 1) // 2):
        lens = ([1] * shift + list(range(1, k + 1)) * 400)
        keys = np.repeat(np.arange(len(lens), dtype=np.int32), lens)[:2100]
        n = len(keys)
        rng = np.random.default_rng(shift + 10 * k)
        perm = rng.permutation(n)  # arrival order unrelated to the key order
        keys = keys[perm]
        price = 21.0 + rng.random(n)          # every condition holds: the run length alone decides
        vol = np.arange(n, dtype=np.int64)
        ts = np.arange(n, dtype=np.int64)
        exp = run(k, keys, price, vol, ts)
        assert len(exp) > 0
        order = np.argsort(keys, kind="stable")
        ends = np.nonzero(np.diff(keys[order]) != 0)[0] + 1
        seen |= {(b, int(e - s)) for s, e in zip(np.r_[0, ends], np.r_[ends, n]) for b in (64, 1024) if s < b < e}
    assert seen >= {(b, L) for b in (64, 1024) for L in range(2, k + 1)}


@pytest.mark.parametrize("keyed", [False, True])
@pytest.mark.parametrize("k", [3, 4, 8])
def test_run_heads_take_members_from_the_carry(k, keyed):
    """Keys hold 0 .. k - 1 carried rows (fewer than k - 1 included, and idle keys); the first events of a key's run
    take 1 .. k - 1 members from the carry's tail, negative relative ordinals, or have no tuple when the carry is too
    short. Keys with e < k - 1 events keep their newest k - 1 - e carried rows."""
    n, K = 1500, 40 if keyed else 1
    keys, price, vol, ts = batch(n, K, seed=5)
    price = 21.0 + price / 10.0  # conditions hold: membership decides
    vol = np.arange(n, dtype=np.int64) + 1000
    ts = ts + 100
    if keyed:
        keys[keys == 7] = 8                    # key 7 is idle: its carried rows all stay
        few = np.nonzero(keys == 9)[0][1:]     # key 9 has one event: it keeps k - 2 carried rows
        keys[few] = 10
        ckeys = list(range(-3, K - 3))
    else:
        keys = None
        ckeys = [0]
    rows, o = [], 5000 - 1000
    for i, key in enumerate(ckeys):
        have = k - 1 if key in (7, 9) or not keyed else i % k  # 0 .. k - 1 carried rows
        for r in range(have):
            p = np.array([22.0 + r]).view(np.int64)[0]
            rows.append([key, o, 99, key, p, r, o])
            o += 1
    carry = np.array(rows, np.int64).reshape(-1, CW)
    exp = run(k, keys, price, vol, ts, obase=5000, carry=carry)
    from_carry = (exp < 0).sum(axis=1)
    for c in range(1, k):
        assert (from_carry == c).any()
    _, cand = rule(k, keys, price, vol, ts, 5000 + np.arange(n), 5000, {}, carry)
    if keyed:
        assert sum(1 for c in cand if c[0] == 7 and c[3] < 0) == k - 1
        assert sum(1 for c in cand if c[0] == 9 and c[3] < 0) == k - 2
    run(k, keys, price, vol, ts, obase=5000, withins={2: 0, k: 1}, carry=carry)  # the carried rows' times count


def test_given_ordinals():
    n = 3000
    keys, price, vol, ts = batch(n, 30, seed=9)
    assert len(run(3, keys, price, vol, ts, ordinals=3 * np.arange(n, dtype=np.int64) + 1, withins={3: 1})) > 0
    assert len(run(4, None, price, vol, ts, ordinals=3 * np.arange(n, dtype=np.int64) + 1, withins={2: 1})) > 0


def marked(app_text):
    """k if the compiler marks the query for the adjacent-run closed form, else 0."""
    z = np.zeros(1, np.int64)
    kout, ncand = ctypes.c_int32(), ctypes.c_int64()
    err = ctypes.create_string_buffer(512)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    lib().sm_seqk_emu(app_text.encode(), ctypes.c_int64(0), ctypes.c_int(0), P(z), P(z), P(z), P(z), P(z), None,
                      ctypes.c_int64(0), P(z), ctypes.c_int64(0), P(z), P(z), ctypes.byref(ncand), ctypes.byref(kout), err,
                      ctypes.c_size_t(512))
    return kout.value


def test_the_compilers_envelope():
    q = lambda body, sel="e1.timestamp as i": SCHEMA + f"@info(name='q') from {body} select {sel} insert into Out;"
    S = "StockStream"
    for k in range(3, 9):
        assert marked(text(k, True, {2: 1, k: 3})) == k and marked(text(k, False)) == k
    chain = lambda k: ", ".join([f"every e1={S}[price>20]"] + [f"e{m}={S}[price>e1.price]" for m in range(2, k + 1)])
    assert marked(q(chain(3))) == 3
    assert marked(q(chain(2))) == 0                                   # the pair form keeps its own path
    assert marked(q(chain(9))) == 0                                   # more than 8 states
    assert marked(q(chain(3).replace("every ", ""))) == 0             # no leading every
    assert marked(q(f"every e1={S}[price>20] within 5 milliseconds, e2={S}, e3={S}")) == 0  # within on e1
    assert marked(q(f"every e1={S}, e2={S}+, e3={S}")) == 0           # a count
    assert marked(q(f"every e1={S}, e2={S}, e3={S}", "e1.timestamp as i having i > 3")) == 0
    two = SCHEMA + "define stream Other (symbol int, price double, volume long, timestamp long); "
    assert marked(two + f"@info(name='q') from every e1={S}, e2=Other, e3={S} select e1.timestamp as i "
                  "insert into Out;") == 0                            # elements on different streams
    assert marked(SCHEMA + f"@info(name='q') from every e1={S}[price>20] -> e2={S} -> e3={S} select e1.timestamp as i "
                  "insert into Out;") == 0                            # a pattern, not a sequence
