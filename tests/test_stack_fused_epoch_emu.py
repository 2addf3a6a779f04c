"""The ring kernel's fused epoch (stack_dev.h, chain4: slice e's emission and slice e + kR's ranking run through one
chain of barriers, the ranking's counts lie on the slot's key-grouped records) under the host wave emulator, against
the pending-list model of tests/test_stack_emu.py (StreamPreStateProcessor.processAndReturn,
core/query/input/stream/state/StreamPreStateProcessor.java:274-327): staged pairs, tile offsets, totals, carry-out.

Streams: per key, prices in descending pairs followed by a peak, each triple above the one before. The peak pops the
pair (the older one through the slot's pool), the next triple's first price pops the peak: three pops per triple, one
of them through the pool, so that pool entries of slice e are read while slice e + kR is counted, and no stack grows.
The emulator build overwrites the slot's key-grouped records right after the event loop's barrier, so a read of them
by either half of the chain shows as a wrong pair. Test infrastructure: no GPU; `-m "not gpu"`."""
import ctypes

import numpy as np
import pytest

from test_stack_emu import consts, lib, model, ptr, vcode

SE_LOG = 2


def triple_prices(keys, desc=2):
    """Per key: `desc` falling prices then a peak above them, every group above the group before (all above 20)."""
    g = desc + 1
    occ = np.zeros(len(keys), np.int64)
    seen = {}
    for j, k in enumerate(keys.tolist()):
        occ[j] = seen.get(k, 0)
        seen[k] = occ[j] + 1
    t, ph = occ // g, occ % g
    step = 4.0 * g
    return 30.0 + step * t + np.where(ph == desc, step - 2.0, 2.0 * (desc - ph))


def run_batches(keys, price, ts, within, splits=(), grid=3):
    """The emulated kernel over the batches that `splits` cuts the stream into, each started from the carry-out of the
    one before; returns per batch what tests/test_stack_emu.py's check looks at, in global ordinals."""
    l = lib()
    c = consts(l)
    bins, tb = c["bins"], c["tb"]
    n = len(keys)
    c1 = price > 20.0
    H = (int(keys.max()) >> 10) + 1
    u32, i64, u64, f64 = ctypes.c_uint32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
    bounds = [0, *splits, n]
    carried = np.zeros((0, 4), np.int64)  # [key, ordinal, ts, value bits] by (key, ordinal)
    out = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        m = hi - lo
        kb, pb, tsb = keys[lo:hi], np.ascontiguousarray(price[lo:hi]), ts[lo:hi]
        d = kb & (bins - 1)
        order = np.argsort(d, kind="stable")
        counts = np.bincount(d, minlength=bins)
        dbase = np.zeros(bins, np.uint32)
        dbase[1:] = np.cumsum(counts)[:-1]
        rec = np.zeros((m, 4), np.uint32)
        rec[:, 0] = (kb | (c1[lo:hi].astype(np.int64) << 31)).astype(np.uint32)
        rec[:, 1] = np.arange(m, dtype=np.uint32)
        rec[:, 2] = vcode(pb)
        rec[:, 3] = (tsb - tsb[0]).astype(np.uint32)
        rec = np.ascontiguousarray(rec[order])
        ntiles = ((m - 1) >> tb) + 1
        # staging runs: a bucket's matches are at most its pops, at most its pushes plus its carried partials
        room = counts + np.bincount(carried[:, 0] & (bins - 1), minlength=bins)
        stage = np.full(int(room.sum()) + 16, 0xFFFFFFFFFFFFFFFF, np.uint64)
        sbase = np.zeros(bins, np.uint32)
        sbase[1:] = np.cumsum(room)[:-1]
        mstart = np.zeros(bins * (ntiles + 1), np.uint32)
        mtot = np.zeros(bins, np.uint32)
        cap = m + len(carried) + 1024
        cand = np.zeros(4 * cap, np.int64)
        cand_n = np.zeros(1, np.uint32)
        err = np.zeros(1, np.uint32)
        spill = np.zeros(grid * c["keys"] * c["q"] * 4, np.uint32)
        if len(carried):
            cin = np.zeros((len(carried), 4), np.uint32)
            cin[:, 0] = (carried[:, 1] - lo).astype(np.int32).view(np.uint32)
            cin[:, 1] = vcode(carried[:, 3].copy().view(np.float64))
            cin[:, 2] = (carried[:, 2] - tsb[0]).astype(np.int32).view(np.uint32)
            cstart = np.searchsorted(carried[:, 0], np.arange(H << 10), side="left").astype(np.uint32)
            cend = np.searchsorted(carried[:, 0], np.arange(H << 10), side="right").astype(np.uint32)
            crow = np.ascontiguousarray(carried)
            cargs = (ptr(cin, u32), ptr(cstart, u32), ptr(cend, u32), ptr(crow, i64))
        else:
            cargs = (None, None, None, None)
        rc = l.sm_stack4_emu(ptr(rec, u32), ptr(dbase, u32), u32(m), ctypes.c_int(H), ctypes.c_int32(within),
                             u32(ntiles), ctypes.c_int(grid), ptr(pb, f64), i64(0), i64(int(tsb[0])), i64(lo),
                             ctypes.c_int32(0), *cargs, ptr(sbase, u32), ptr(stage, u64), ptr(mstart, u32),
                             ptr(mtot, u32), ptr(cand, i64), u32(cap), ptr(cand_n, u32), ptr(err, u32),
                             ptr(spill, u32))
        assert rc == 0
        cd = cand[:4 * int(cand_n[0])].reshape(-1, 4)
        nxt = np.array(sorted((int(k), int(o), int(t), int(price[o:o + 1].view(np.int64)[0])) for k, o, t, _ in cd),
                       np.int64).reshape(-1, 4)
        out.append(dict(lo=lo, hi=hi, d=d, counts=counts, sbase=sbase, stage=stage, ntiles=ntiles,
                        mstart=mstart.reshape(bins, ntiles + 1), mtot=mtot, cand=cd, err=int(err[0]),
                        carried=carried))
        carried = nxt
    return out, c


def check_batches(keys, price, ts, within, splits=(), grid=3, least=None):
    res, c = run_batches(keys, price, ts, within, splits, grid)
    bins, tb = c["bins"], c["tb"]
    n = len(keys)
    c1 = price > 20.0
    for r in res:
        lo, hi = r["lo"], r["hi"]
        assert r["err"] & SE_LOG == 0, "a slice's pops overran its pool"
        assert r["err"] == 0, f"kernel error flags {r['err']:#x}"
        matches, exp_cand = model(keys[:hi], price[:hi], ts[:hi], within, c1[:hi])  # the whole stream up to here
        per = [[] for _ in range(bins)]
        for i, j in matches:  # in order of j, then pending order
            if j >= lo:
                per[int(keys[j]) & (bins - 1)].append(((j - lo) << 32) | ((i - lo) & 0xFFFFFFFF))
        for b in range(bins):
            exp = np.array(per[b], np.uint64)
            assert int(r["mtot"][b]) == len(exp), f"bucket {b}: {int(r['mtot'][b])} matches, expected {len(exp)}"
            got = r["stage"][r["sbase"][b]:r["sbase"][b] + len(exp)]
            assert np.array_equal(got, exp), f"bucket {b}: staged matches differ"
            t = np.arange(r["ntiles"] + 1, dtype=np.uint64) << np.uint64(tb)
            assert np.array_equal(r["mstart"][b], np.searchsorted(exp >> np.uint64(32), t).astype(np.uint32)), \
                f"bucket {b}: tile offsets differ"
        # carry-out: (key, ordinal, ts) of the partials still pending; the row is the batch row, or -1 - (row among the
        # carried partials) for one that came in carried
        crows = {int(o): q for q, o in enumerate(r["carried"][:, 1])}
        want = sorted((k, i, t, i - lo if i >= lo else -1 - crows[i]) for k, i, t, _ in exp_cand)
        assert sorted(tuple(int(x) for x in row) for row in r["cand"]) == want
    if least is not None:
        assert len(matches) > least, len(matches)
    return res


def bucket_lengths():
    c = consts(lib())
    ss, r = c["ss"], c["r"]
    return [ss - 1, ss, ss + 1, r * ss, r * ss + 1, (r + 2) * ss, 3 * ss + 1, 1]


def stream_of(lengths, hkeys, seed):
    """Buckets 0 .. len(lengths) - 1 of the given lengths in a random interleaving, in-bucket keys uniform below hkeys"""
    rng = np.random.default_rng(seed)
    digit = np.concatenate([np.full(n, b, np.int64) for b, n in enumerate(lengths)])
    rng.shuffle(digit)
    return (rng.integers(0, hkeys, len(digit)) << 10) | digit


@pytest.mark.parametrize("within", [1000, -1])
@pytest.mark.parametrize("hkeys", [1, 1024])
def test_bucket_lengths(hkeys, within):
    """one key per bucket: 64 * kI4 records of a wave land in one (key, wave) byte of the counts"""
    lengths = bucket_lengths()
    keys = stream_of(lengths, hkeys, 3 + hkeys)
    n = len(keys)
    ts = np.arange(n, dtype=np.int64) // 20
    res = check_batches(keys, triple_prices(keys), ts, within, least=n // 4)
    assert [int(x) for x in res[0]["counts"][:len(lengths)]] == lengths


@pytest.mark.parametrize("within", [1000, -1])
def test_edge_keys_at_slice_ends(within):
    """in-bucket keys 0 and 1023 only where a slice starts and ends: record 0 of every slice is key 0's and record
    sn - 1 is key 1023's (their key-grouped runs start at 0 and end at sn - 1), other keys between them"""
    c = consts(lib())
    ss, r = c["ss"], c["r"]
    m = (r + 1) * ss + 7  # the last slice holds seven records
    rng = np.random.default_rng(17)
    high = rng.integers(1, 1023, m)
    high[0::ss] = 0
    high[ss - 1::ss] = 1023
    high[m - 1] = 1023
    keys = (high << 10) | 5
    ts = np.arange(m, dtype=np.int64) // 20
    check_batches(keys, triple_prices(keys), ts, within, least=m // 8)
    both = (np.where(np.arange(m) % 2 == 0, 0, 1023) << 10) | 5  # and the two keys alone, alternating
    check_batches(both, triple_prices(both), ts, within, least=m // 2)


def test_pool_filled_exactly():
    """one key, three falling prices and a peak: two of four events' pops go to the pool, kPool = kSS / 2 in a slice"""
    c = consts(lib())
    ss, r = c["ss"], c["r"]
    assert ss % 4 == 0
    m = (r + 1) * ss
    keys = np.full(m, 9, np.int64)
    res = check_batches(keys, triple_prices(keys, desc=3), np.arange(m, dtype=np.int64) // 20, -1, least=m // 2)
    assert int(res[0]["mtot"][9]) == m - 1  # every event but the last peak is popped
    # four falling prices and a peak: three of five events' pops, more than the pool holds; the flag is raised
    out, _ = run_batches(keys, triple_prices(keys, desc=4), np.arange(m, dtype=np.int64) // 20, -1)
    assert out[0]["err"] & SE_LOG


@pytest.mark.parametrize("within", [1000, -1])
def test_two_batches_carry_partials(within):
    lengths = bucket_lengths()
    keys = stream_of(lengths, 1024, 29)
    n = len(keys)
    ts = np.arange(n, dtype=np.int64) // 20
    res = check_batches(keys, triple_prices(keys), ts, within, splits=(n // 2 + 1,), least=n // 4)
    assert len(res[1]["carried"]) > 1000
