"""The adjacent-pair closed form of `every e1=S[c1], e2=S[c2] [within T]` (siddhi_amd/csrc/kernels/seq_dev.h: link,
keep, count and emit kernels) run on the CPU under the host wave emulator (tests/native/seq_emu.cpp: the same device
source, one fiber per GPU thread), against a numpy statement of the rule the oracle was checked to follow: for every
event j of a partition instance with a predecessor i (the previous event of the same instance, or the instance's
carried row at a batch start), emit (i, j) iff c1(i), c2(i, j) and ts[j] - ts[i] <= T; outputs in order of j; the
instance's last event is carried if it passes c1, and an instance without events keeps its carried row.
Test infrastructure: no GPU; `-m "not gpu"`."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
LIB = os.path.join(NATIVE, "build", "libseq_emu.so")
KERNELS = os.path.join(HERE, "..", "siddhi_amd", "csrc", "kernels")
CXX = "/opt/rocm/lib/llvm/bin/clang++"


def lib():
    deps = [os.path.join(NATIVE, "seq_emu.cpp"), os.path.join(NATIVE, "emu_fibers.h")] + [
        os.path.join(KERNELS, f) for f in ("seq_dev.h", "fastpath_dev.h", "expr.h", "hd.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call([CXX if os.path.exists(CXX) else "g++", "-std=c++20", "-O2", "-g", "-fPIC", "-shared",
                               "-Wno-attributes", "-o", LIB, os.path.join(NATIVE, "seq_emu.cpp"), "-lpthread"])
    L = ctypes.CDLL(LIB)
    L.sm_seq_emu.restype = ctypes.c_int64
    return L


def rule(keys, price, ts, ordinals, obase, within, thr, carry):
    """(pairs relative to obase, carry-out rows (key, global ordinal, ts, source), used marks), vectorised per
    instance: rows in (key, arrival) order, each compared with its left neighbour."""
    n = len(price)
    k = np.zeros(n, np.int64) if keys is None else keys.astype(np.int64)
    gord = obase + np.arange(n, dtype=np.int64) if ordinals is None else ordinals
    order = np.argsort(k, kind="stable")
    ks = k[order]
    head = np.ones(n, bool)
    head[1:] = ks[1:] != ks[:-1]
    tail = np.ones(n, bool)
    tail[:-1] = head[1:]
    c1 = np.ones(n, bool) if thr is None else price > thr
    # predecessor inside the batch
    e1 = np.full(n, np.iinfo(np.int64).min)
    j, i = order[1:][~head[1:]], order[:-1][~head[1:]]
    ok = c1[i] & (price[j] > price[i])
    if within >= 0:
        ok &= ts[j] - ts[i] <= within
    e1[j[ok]] = gord[i[ok]] - obase
    # run heads against the carry (one row per key)
    used = np.zeros(len(carry), np.uint8)
    ckeys = carry[:, 0] if len(carry) else np.zeros(0, np.int64)
    for u in np.nonzero(head)[0]:
        c = np.searchsorted(ckeys, ks[u])
        if c < len(ckeys) and ckeys[c] == ks[u]:
            used[c] = 1
            jj = order[u]
            cp = carry[c, 4:5].view(np.float64)[0]
            if price[jj] > cp and (within < 0 or ts[jj] - carry[c, 2] <= within):
                e1[jj] = carry[c, 1] - obase
    rows = np.nonzero(e1 != np.iinfo(np.int64).min)[0]
    pairs = np.stack([e1[rows], gord[rows] - obase], axis=1)
    out = [(int(ks[u]), int(gord[order[u]]), int(ts[order[u]]), int(order[u]))
           for u in np.nonzero(tail)[0] if c1[order[u]]]
    out += [(int(carry[c, 0]), int(carry[c, 1]), int(carry[c, 2]), -c - 1) for c in range(len(carry)) if not used[c]]
    return pairs, sorted(out), used


def run(keys, price, ts, ordinals=None, obase=0, within=-1, thr=None, carry=None):
    n = len(price)
    carry = np.zeros((0, 5), np.int64) if carry is None else np.ascontiguousarray(carry, dtype=np.int64)
    nc = len(carry)
    pairs = np.full(2 * n + 2, 0xDEADBEEF, np.uint32)
    cand = np.zeros(4 * (n + nc) + 4, np.int64)
    used = np.full(nc + 1, 7, np.uint8)
    ncand = ctypes.c_int64()
    price = np.ascontiguousarray(price, dtype=np.float64)
    ts = np.ascontiguousarray(ts, dtype=np.int64)
    k32 = None if keys is None else np.ascontiguousarray(keys, dtype=np.int32)
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    m = lib().sm_seq_emu(ctypes.c_int64(n), P(k32), P(price), P(ts), P(ordinals), ctypes.c_int64(obase),
                         ctypes.c_int64(within), ctypes.c_int(thr is not None),
                         ctypes.c_double(0.0 if thr is None else thr), P(carry), ctypes.c_int64(nc), P(pairs), P(cand),
                         ctypes.byref(ncand), P(used))
    exp_pairs, exp_cand, exp_used = rule(keys, price, ts, ordinals, obase, within, thr, carry)
    got = pairs[:2 * m].view(np.int32).astype(np.int64).reshape(-1, 2)
    np.testing.assert_array_equal(got, exp_pairs)
    assert pairs[2 * m] == 0xDEADBEEF  # nothing written past the last pair
    got_cand = sorted(tuple(int(x) for x in cand[4 * c:4 * c + 4]) for c in range(ncand.value))
    assert got_cand == exp_cand
    np.testing.assert_array_equal(used[:nc], exp_used)
    return len(exp_pairs)


def batch(n, K, seed=0):
    rng = np.random.default_rng(seed * 1000003 + n * 31 + K)
    keys = rng.integers(0, K, n).astype(np.int32) - 3  # negative keys too
    price = np.round(rng.random(n) * 100.0, 1)          # ties
    ts = np.arange(n, dtype=np.int64) // 3
    return keys, price, ts


SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 8191, 8193, 200000]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("K", [None, 1, 50, 3000])
def test_link_and_compaction_follow_the_rule(n, K):
    """Every size of the device tests: below, at and above a wave, a tile (1024 rows) and many tiles; unkeyed (K
    None: row order, the link pass counts its own tiles) and keyed (key order, seq_count_kernel)."""
    keys, price, ts = batch(n, K or 1)
    m = run(None if K is None else keys, price, ts, within=2, thr=20.0)
    if n >= 8191:
        assert m > 0


def test_more_keys_than_events():
    keys, price, ts = batch(300, 100000)
    run(keys, price, ts, thr=20.0)


@pytest.mark.parametrize("keyed", [False, True])
def test_run_heads_and_the_carry(keyed):
    """A run head whose key has a carried row pairs with it (negative relative ordinal) or drops it; a head whose key
    has none pairs with nothing; carried keys without events keep their rows; with a `within`, a carried row exactly
    T old still pairs and one T + 1 old does not."""
    n, K = 3000, 40
    keys, price, ts = batch(n, K, seed=5)
    ts = ts + 100
    if not keyed:
        keys = None
        ck = [0]
    else:
        present = np.unique(keys)
        ck = sorted(set(present[::2].tolist()) | {-50, 1000, 2000})  # every other present key, and three idle ones
    T = 4
    carry = np.zeros((len(ck), 5), np.int64)
    first_ts = {}
    for j in range(n - 1, -1, -1):
        first_ts[0 if keys is None else int(keys[j])] = int(ts[j])
    for r, k in enumerate(ck):
        age = T if r % 2 == 0 else T + 1
        carry[r] = [k, 5000 - 100 + r, first_ts.get(k, 0) - age, k, 0]
        carry[r, 4:5] = np.array([-1.0]).view(np.int64)  # below every price: c2 holds, the age decides
    m = run(keys, price, ts, obase=5000, within=T, thr=20.0, carry=carry)
    assert m > 0
    exp, cand, used = rule(keys, price, ts, None, 5000, T, 20.0, carry)
    carried_pairs = (exp[:, 0] < 0).sum()
    if keyed:
        assert 0 < carried_pairs < used.sum() and used.sum() == len(ck) - 3
        assert sum(1 for c in cand if c[3] < 0) == 3
    else:
        assert carried_pairs == 1 and used.sum() == 1
    run(keys, price, ts, obase=5000, within=-1, thr=None, carry=carry)


def test_given_ordinals():
    n = 5000
    keys, price, ts = batch(n, 30, seed=9)
    run(keys, price, ts, ordinals=3 * np.arange(n, dtype=np.int64) + 1, obase=0, within=1, thr=20.0)
    run(None, price, ts, ordinals=3 * np.arange(n, dtype=np.int64) + 1, obase=0, within=1, thr=20.0)
