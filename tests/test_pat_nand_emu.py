"""The closed form of the logical absent `every e1=A[c1] -> not B[c2] and e3=C[c3] within T`
(siddhi_amd/csrc/kernels/mpat_nand_dev.h: pnand_link_kernel, behind mseq_dev.h's facts, pack and stream kernels,
absent_dev.h's count scan, seq_dev.h's count kernel and mpat_dev.h's emit and pairs kernels) run on the CPU under the host
wave emulator (tests/native/pat_nand_emu.cpp: the same device source, one fiber per GPU thread, on the plan the product's
compiler makes of the query text), against a numpy statement of the rule tests/test_pat_nand_plan.py ties to the oracle,
batch by batch with carried partials: every partial (a carried e1 row, or an A row of the batch passing c1) takes the
first later C row of its instance that passes c3; the pair comes out iff that row lies inside T and no cancelling row of
the instance lies before it; a partial without either, not yet expired at the batch's last read row, is carried out.
Each case compares the pairs, in order, and the sorted carry-out candidates. The shapes are those at which the kernel can
go wrong: the private budget's edge and a wave step's edge for the cancel bound, the bound next to the e3, the bound and
the e3 in different chunks of the count scan, a run head that cancels. Test infrastructure: no GPU; `-m "not gpu"`."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_pat_nand_plan import C3, nand_text

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
LIB = os.path.join(NATIVE, "build", "libpat_nand_emu.so")
CSRC = os.path.join(HERE, "..", "siddhi_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
NAMES = ["A", "B", "C"]
CW = 7  # carried row: key, global ordinal, ts, the four attributes
BITS = lambda x: int(np.array([x], np.float64).view(np.int64)[0])
UNBITS = lambda x: float(np.array([x], np.int64).view(np.float64)[0])


def lib():
    srcs = [os.path.join(NATIVE, "pat_nand_emu.cpp"), os.path.join(CSRC, "compiler.cpp"),
            os.path.join(CSRC, "siddhiql", "parser.cpp")]
    deps = srcs + [os.path.join(NATIVE, "emu_fibers.h"), os.path.join(CSRC, "compiler.h"), os.path.join(CSRC, "plan.h")]
    deps += [os.path.join(CSRC, "kernels", f) for f in ("mpat_nand_dev.h", "mpat_dev.h", "absent_dev.h", "mseq_dev.h",
                                                        "seq_dev.h", "fastpath_dev.h", "expr.h", "hd.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call([CXX if os.path.exists(CXX) else "g++", "-std=c++20", "-O2", "-g", "-fPIC", "-shared",
                               "-Wno-attributes", "-o", LIB] + srcs + ["-lpthread"])
    L = ctypes.CDLL(LIB)
    L.sm_pat_nand_emu.restype = ctypes.c_int64
    return L


def call(app_text, sid, sym, price, vol, ts, ordinals=None, obase=0, carry=None, per=256):
    """One batch: (m, pairs (m, 2) relative to obase (a carried e1 negative), sorted carry-out candidates, marks, facts,
    err)."""
    n = len(sid)
    carry = np.zeros((0, CW), np.int64) if carry is None else np.ascontiguousarray(carry, dtype=np.int64)
    room = n + len(carry) + 2
    pairs = np.full(2 * room, 0xDEADBEEF, np.uint32)
    cand = np.zeros(4 * room, np.int64)
    ncand = ctypes.c_int64()
    marks = np.zeros(8, np.int32)
    facts = np.zeros(4, np.int64)
    err = ctypes.create_string_buffer(512)
    tcol = np.arange(n, dtype=np.int64)
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    I = ctypes.c_int64
    arrs = [np.ascontiguousarray(sid, dtype=np.int32), np.ascontiguousarray(sym, dtype=np.int32),
            np.ascontiguousarray(price, dtype=np.float64), np.ascontiguousarray(vol, dtype=np.int64), tcol,
            np.ascontiguousarray(ts, dtype=np.int64)]
    ordinals = None if ordinals is None else np.ascontiguousarray(ordinals, dtype=np.int64)
    m = lib().sm_pat_nand_emu(app_text.encode(), I(n), *[P(a) for a in arrs], P(ordinals), I(obase), P(carry),
                              I(len(carry)), I(per), P(pairs), P(cand), ctypes.byref(ncand), P(marks), P(facts), err,
                              ctypes.c_size_t(512))
    k = max(m, 0)
    assert pairs[2 * k] == 0xDEADBEEF  # nothing past the last pair
    out = pairs[:2 * k].view(np.int32).astype(np.int64).reshape(-1, 2)
    cands = sorted(tuple(int(x) for x in cand[4 * c:4 * c + 4]) for c in range(ncand.value))
    return m, out, cands, marks, facts, err.value


def marks_of(app_text):
    z = np.zeros(1, np.int64)
    r = call(app_text, z[:0].astype(np.int32), z[:0], z[:0], z[:0], z[:0])
    assert r[0] >= 0 or r[5].startswith(b"not marked"), r[5]  # the text compiles
    return tuple(int(x) for x in r[3])


def rule(a, b, c, key, sid, price, vol, ts, gord, obase, within, c3, carry):
    """One batch with its carry, partial by partial: (pairs (m, 2) as call()'s, the sorted carry-out candidates)."""
    sa, sb, sc = (NAMES.index(x) for x in (a, b, c))
    n = len(sid)
    read = np.isin(sid, [sa, sb, sc])
    if not read.any():
        return np.zeros((0, 2), np.int64), None  # the carried rows wait
    ts_last = int(ts[np.nonzero(read)[0][-1]])
    f = C3[c3][1]
    cancels = read & (sid == sb) & (price > 45)
    isc = read & (sid == sc)
    parts = [(int(r[0]), int(r[1]), int(r[2]), -x - 1, -1, UNBITS(r[4]), int(r[5])) for x, r in enumerate(carry)]
    for i in np.nonzero((sid == sa) & (price > 20))[0]:
        parts.append((int(key[i]), int(gord[i]), int(ts[i]), int(i), int(i), float(price[i]), int(vol[i])))
    outs, cand = [], []
    pos = np.arange(n)
    for place, (k, o, t1, src, after, p1, v1) in enumerate(parts):
        mine = (key == k) & (pos > after)
        js = np.nonzero(mine & isc & f(p1, v1, price, vol))[0]
        bs = np.nonzero(mine & cancels)[0]
        if len(js):
            j = int(js[0])
            if ts[j] - t1 <= within and not (len(bs) and bs[0] < j):
                outs.append((j, place, o - obase, int(gord[j]) - obase))
        elif not len(bs) and ts_last - t1 <= within:
            cand.append((k, o, t1, src))
    outs.sort()
    return np.array([(i, j) for _, _, i, j in outs], dtype=np.int64).reshape(-1, 2), sorted(cand)


def carried(rows):
    """rows of (key, global ordinal, ts, price): carried e1 rows, their timestamp attribute = the ordinal; sorted."""
    return np.array(sorted((k, o, t, k, BITS(p), 100, o) for k, o, t, p in rows), dtype=np.int64).reshape(-1, CW)


def check(abc, kind, sid, sym, price, vol, ts, within=5, c3="gt", carry=None, obase=0, ordinals=None, per=256,
          mirrored=False):
    a, b, c = abc
    keyed = kind != "flat"
    keys = None
    if keyed:
        keys = {s: "symbol" for s in abc}
        if kind == "per_stream":
            keys[b if b != a else c] = "volume"
    sid = np.asarray(sid, np.int32)
    sym, vol, price, ts = np.asarray(sym), np.asarray(vol, np.int64), np.asarray(price, float), np.asarray(ts, np.int64)
    key = np.zeros(len(sid), np.int64)
    if keyed:
        for s in set(abc):
            mine = sid == NAMES.index(s)
            key[mine] = (sym if keys[s] == "symbol" else vol)[mine]
    carry = np.zeros((0, CW), np.int64) if carry is None else carry
    gord = obase + np.arange(len(sid), dtype=np.int64) if ordinals is None else np.asarray(ordinals, np.int64)
    text = nand_text(a, b, c, keys, within, c3, mirrored)
    m, out, cands, marks, facts, err = call(text, sid, sym, price, vol, ts, ordinals, obase, carry, per)
    assert m >= 0 and marks[0] == 1, err
    exp, ecand = rule(a, b, c, key, sid, price, vol, ts, gord, obase, within, c3, carry)
    np.testing.assert_array_equal(out, exp)
    if ecand is not None:
        assert cands == ecand
    else:
        assert cands == []
    return out, cands, facts


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
def test_random_batches_with_carried_partials(n, kind):
    """Waves, blocks, tiles and chunks of 256 positions: one more and one fewer than each; carried partials in front of
    their keys' runs, of a key without rows here, one beyond the window already."""
    sid, sym, price, vol, ts = random_batch(n, 6, n)
    keyed = kind != "flat"
    ks = [-2, 0, 3, 9] if keyed else [0]  # (key 9 has no rows in the batch)
    carry = carried([(k, 50 + 3 * j + r, 93 + 3 * r, 20.5 + 9 * r) for j, k in enumerate(ks) for r in range(3)])
    out, cands, facts = check(ABC, kind, sid, sym, price, vol, ts, 5, carry=carry, obase=1000)
    if n >= 1023:
        assert len(out) >= 5 and facts[2] > 0
    check(ABC, kind, sid, sym, price, vol, ts, 40, "compound", carry=carry, obase=1000, mirrored=True)


def bound_feed(d, where, K=1):
    """Per key: an e1, d - 1 rows that neither cancel nor match, the bound d positions past the e1; the first passing C
    row one position before the bound ("before": it replaces the last filler), one after it, or absent; then a second
    e1 and a C row that completes it (and would have completed the first)."""
    rows = [(0, 30.0)]
    for g in range(d - 1):
        rows.append(((2, 10.0), (1, 10.0), (0, 10.0))[g % 3])  # no c3, no c2, no c1
    if where == "before":
        rows[-1] = (2, 40.0)
    rows.append((1, 50.0))  # the bound
    if where == "after":
        rows.append((2, 40.0))
    rows += [(0, 25.0), (2, 41.0)]
    n = len(rows) * K
    sid = np.repeat(np.array([r[0] for r in rows], np.int32), K)
    price = np.repeat(np.array([r[1] for r in rows]), K)
    sym = np.tile(np.arange(K, dtype=np.int32), len(rows))
    return sid, sym, price, np.zeros(n, np.int64), 100 + np.arange(n, dtype=np.int64) // (64 * K)


@pytest.mark.parametrize("kind", ["flat", "symbol"])
# (at d = 1 there is no position between the e1 and the bound)
@pytest.mark.parametrize("d,where", [(d, w) for d in (1, 15, 16, 17, 63, 64, 65, 200, 300)
                                     for w in ("before", "after", "absent") if d > 1 or w != "before"])
def test_the_cancel_bound_at_the_budgets_and_the_wave_steps_edges(d, where, kind):
    """The scan of the first e1 ends at the bound d positions on: inside the lane's own budget of 16, at its edge, in the
    wave's first step, at its edge, and steps later; at 300 the e1 and the bound lie in different chunks of 256."""
    fd = bound_feed(d, where, 1 if kind == "flat" else 3)
    K = 1 if kind == "flat" else 3
    out, cands, _ = check(ABC, kind, *fd, within=40)
    first = np.nonzero(out[:, 0] < K)[0]
    assert len(first) == (K if where == "before" else 0)  # the first e1s match only in front of the bound
    assert len(out) == (2 * K if where == "before" else K) and cands == []


def test_e3_and_the_bound_in_different_chunks():
    """Unkeyed, chunks of 256: the e1 in chunk 0, its C row in chunk 1 and the bound in chunk 3, and the other way."""
    for jpos, bpos in ((300, 800), (800, 300)):
        n = 1000
        sid = np.full(n, 2, np.int32)
        price = np.full(n, 10.0)
        sid[0], price[0] = 0, 30.0
        sid[jpos], price[jpos] = 2, 40.0
        sid[bpos], price[bpos] = 1, 50.0
        z = np.zeros(n, np.int64)
        out, cands, facts = check(ABC, "flat", sid, z, price, z, 100 + z, within=5)
        assert facts[2] == 1 and out.tolist() == ([[0, jpos]] if jpos < bpos else []) and cands == []


@pytest.mark.parametrize("kind", ["flat", "symbol"])
def test_a_run_head_that_cancels_meets_carried_partials(kind):
    """The first row of the key's run is a cancelling row: the carried partials of that key die there, also when the
    next row would have matched; the head of another key's run is the matching row itself."""
    keyed = kind != "flat"
    carry = carried([(1 if keyed else 0, 10, 98, 30.0), (1 if keyed else 0, 11, 99, 31.0)] +
                    ([(2, 12, 99, 30.0)] if keyed else []))
    sid = np.array([1, 2, 2, 0, 2], np.int32)
    sym = np.array([1, 1, 2, 1, 1], np.int32)
    price = np.array([50.0, 40.0, 40.0, 30.0, 45.0])
    out, cands, _ = check(ABC, kind, sid, sym, price, np.zeros(5, np.int64), np.array([100, 100, 101, 101, 102]),
                          carry=carry, obase=100)
    if keyed:
        assert out.tolist() == [[12 - 100, 2], [3, 4]] and cands == []
    else:
        assert out.tolist() == [[3, 4]]


@pytest.mark.parametrize("kind", ["flat", "symbol"])
def test_carried_partials_match_are_cancelled_expire_and_stay(kind):
    keyed = kind != "flat"
    k = (lambda x: x) if keyed else (lambda x: 0)
    # key 1 matches, key 2 is cancelled, key 3 expires (its C row comes late), key 4 has no rows and stays, key 5 has
    # rows that neither cancel nor match and stays; flat: one run, the first cancelling row ends them all
    carry = carried([(k(1), 10, 98, 30.0), (k(2), 11, 98, 30.0), (k(3), 12, 90, 30.0), (k(4), 13, 99, 30.0),
                     (k(5), 14, 99, 30.0)])
    sid = np.array([2, 1, 2, 2, 2], np.int32)
    sym = np.array([1, 2, 2, 3, 5], np.int32)
    price = np.array([40.0, 50.0, 40.0, 40.0, 10.0])
    out, cands, _ = check(ABC, kind, sid, sym, price, np.zeros(5, np.int64), np.array([100, 100, 101, 101, 102]),
                          carry=carry, obase=100)
    if keyed:
        assert out.tolist() == [[10 - 100, 0]]
        assert [c[0] for c in cands] == [4, 5] and [c[3] for c in cands] == [-4, -5]
    else:
        assert len(out) == 4 and cands == []  # every carried row inside the window takes row 0


@pytest.mark.parametrize("kind", ["flat", "symbol"])
@pytest.mark.parametrize("parts", [70, 900])
def test_one_e3_completes_many_partials_some_of_them_cancelled(parts, kind):
    """`price > 45`-style c3: carried and batch partials of one key, a cancelling row after the first third of the batch's,
    then one C row: the batch partials behind the cancelling row and nobody else come out, oldest first."""
    carry = carried([(1 if kind != "flat" else 0, 10 + r, 99, 30.0) for r in range(parts // 3)])
    n = parts + 2
    sid = np.zeros(n, np.int32)
    price = np.full(n, 30.0)
    cut = parts // 3
    sid[cut], price[cut] = 1, 50.0
    sid[-1], price[-1] = 2, 50.0
    out, cands, _ = check(ABC, kind, sid, np.ones(n, np.int32), price, np.zeros(n, np.int64),
                          100 + np.zeros(n, np.int64), within=5, c3="const", carry=carry, obase=2000)
    assert len(out) == n - 2 - cut and (out[:, 1] == n - 1).all() and (np.diff(out[:, 0]) > 0).all() and cands == []


@pytest.mark.parametrize("kind", ["flat", "symbol"])
@pytest.mark.parametrize("abc", [("A", "A", "C"), ("A", "B", "A"), ("C", "A", "B")])
def test_shared_streams(abc, kind):
    """A = B: an e1 passing c2 cancels the earlier partials and opens its own. A = C: a row is an e3 of the earlier
    partials and an e1 at once."""
    sid, sym, price, vol, ts = random_batch(1500, 4, 5, step=2)
    ks = [0, 1] if kind != "flat" else [0]
    carry = carried([(k, 50 + 2 * j + r, 97 + r, 22.0 + 20 * r) for j, k in enumerate(ks) for r in range(2)])
    out, cands, facts = check(abc, kind, sid, sym, price, vol, ts, 5, carry=carry, obase=1000)
    assert len(out) > 10 and facts[2] > 10
    check(abc, kind, sid, sym, price, vol, ts, 2, "compound", carry=carry, obase=1000, mirrored=True)


@pytest.mark.parametrize("kind", ["flat", "symbol"])
def test_no_read_row_and_only_a_rows(kind):
    carry = carried([(0, 10, 99, 30.0)])
    hb = np.full(5, -1, np.int32)
    z = np.zeros(5, np.int64)
    m, out, cands, _, facts, _ = call(nand_text("A", "B", "A", None if kind == "flat" else {"A": "symbol", "B": "symbol"}),
                                      np.array([-1, 2, 2, -1, 2], np.int32), z, z.astype(float), z, 100 + z, carry=carry,
                                      obase=100)
    assert m == 0 and cands == [] and facts[0] == 0  # rows of C and heartbeats only: the carried rows wait
    n = 700
    sid = np.zeros(n, np.int32)
    sym = (np.arange(n) % 3).astype(np.int32)
    price = np.where(np.arange(n) % 5 == 0, 10.0, 30.0)
    ts = 100 + np.arange(n, dtype=np.int64) // 100
    out, cands, _ = check(ABC, kind, sid, sym, price, np.zeros(n, np.int64), ts, within=2, carry=carry, obase=1000)
    assert len(out) == 0 and 0 < len(cands) < n * 4 // 5  # the open ones: c1 and not older than 2 ms at the last row


@pytest.mark.parametrize("kind", ["flat", "symbol", "per_stream"])
def test_given_ordinals_with_gaps(kind):
    sid, sym, price, vol, ts = random_batch(1200, 5, 21)
    ordinals = 5000 + np.cumsum(np.random.default_rng(2).integers(1, 9, 1200)).astype(np.int64)
    ks = [0, 1] if kind != "flat" else [0]
    carry = carried([(k, 4000 + j, 99, 25.0) for j, k in enumerate(ks)])
    out, _, _ = check(ABC, kind, sid, sym, price, vol, ts, 5, carry=carry, obase=5000, ordinals=ordinals)
    assert len(out) > 10 and out[:, 1].max() > 1200


@pytest.mark.parametrize("kind", ["flat", "symbol"])
def test_within_0(kind):
    sid, sym, price, vol, ts = random_batch(2000, 4, 8, step=2)
    out, cands, _ = check(ABC, kind, sid, sym, price, vol, ts, 0)
    assert len(out) >= 3 and (ts[out[:, 0]] == ts[out[:, 1]]).all()
    carry = carried([(0, 10, int(ts[0]), 25.0), (0, 11, int(ts[0]) - 1, 25.0)])
    check(ABC, kind, sid, sym, price, vol, ts, 0, carry=carry, obase=1000)


def test_stand_alone_self_check_under_asan_and_ubsan():
    """tests/native/pat_nand_emu.cpp's own main(), built with AddressSanitizer and UBSan as a stand-alone program and
    run once: random batches with carried partials at the wave, tile and chunk edges, and the bound shapes (the cancel
    bound 1 .. 301 positions past the e1, the first passing C row before it, behind it, absent) against a plain loop."""
    exe = os.path.join(NATIVE, "build", "pat_nand_emu_san")
    srcs = [os.path.join(NATIVE, "pat_nand_emu.cpp"), os.path.join(CSRC, "compiler.cpp"),
            os.path.join(CSRC, "siddhiql", "parser.cpp")]
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    subprocess.check_call([CXX if os.path.exists(CXX) else "g++", "-std=c++20", "-O1", "-g", "-Wno-attributes",
                           "-DSM_PAT_NAND_EMU_MAIN", "-o", exe] + san + srcs + ["-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "pat_nand_emu self-check ok" in r.stdout, r.stdout + r.stderr

