"""The unkeyed walk's j order by output tiles (siddhi_amd/csrc/kernels/jtile_dev.h, jt_count_kernel and
jt_place_kernel) run on the CPU under the host wave emulator (tests/native/jtile_emu.cpp: the same device source, one
fiber per GPU thread), against numpy.

The walk leaves its (e1, e2) = (i, j) pairs chunk by chunk in ascending i; the output is those pairs under a stable
sort by j: the reference emits at e2's arrival, the partials it completes oldest first
(StreamPreStateProcessor.processAndReturn walks the pending list oldest first). The emulator entry fills P, which the
product takes from an uncleared scratch arena, with a poison word before the count kernel, so an entry of P the
kernel does not write is seen here as it may be on the GPU.

Checked: out against the stable sort, cnt against bincount(j >> 11), the largest j - i, and P by its meaning (P[u]
splits the populated staging slots into i < 2048 u before it and i >= 2048 u from it on), never against a second
implementation. Test infrastructure: no GPU; `-m "not gpu"`."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
LIB = os.path.join(NATIVE, "build", "libjtile_emu.so")

TB = 11
TILE = 1 << TB
CAP = 4096
DMAX = 4 * TILE
WALK_TILE = 1024  # the walk's chunks are whole tiles of this many events
SENTINEL = np.uint64(0xFFFFFFFFFFFFFFFF)  # out before the run: no pair has this value
SLACK = np.uint64(0xEEEEEEEEEEEEEEEE)     # staging slots past a chunk's pairs: never to be read as pairs
POISON = 0xA5A5A5A5
GUARD = 64  # sentinel entries past out[M]: nothing is placed there

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    kdir = os.path.join(HERE, "..", "siddhi_amd", "csrc", "kernels")
    deps = [os.path.join(NATIVE, f) for f in ("jtile_emu.cpp", "emu_fibers.h", "Makefile")]
    deps += [os.path.join(kdir, f) for f in ("jtile_dev.h", "fastpath_dev.h", "hd.h", "expr.h", "nfa.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["make", "-s", "-C", NATIVE, "jtileemu"])
    l = ctypes.CDLL(LIB)
    l.sm_jtile_emu.restype = ctypes.c_int
    c = (ctypes.c_int * 4)()
    l.sm_jtile_emu_consts(c)
    assert list(c) == [TILE, CAP, DMAX, 256]
    _lib = l
    return l


def walk_pairs(price, key, window=None):
    """Positions (i, j) of the matches of `every e1=[price > 20] -> e2=[price > e1.price]`: each event completes every
    pending e1 with a lower price (what stays pending never rises from oldest to newest, so those are the newest
    ones), then waits itself if its price is above 20. `window`: a pending e1 is dropped once key[j] - key[i] exceeds
    it."""
    pend, pi, pj = [], [], []
    head = 0
    price = price.tolist()
    key = key.tolist()
    for p, x in enumerate(price):
        if window is not None:
            while head < len(pend) and key[p] - key[pend[head]] > window:
                head += 1
        while len(pend) > head and price[pend[-1]] < x:
            pi.append(pend.pop())
            pj.append(p)
        if x > 20.0:
            pend.append(p)
    pi, pj = np.array(pi, dtype=np.int64), np.array(pj, dtype=np.int64)
    o = np.argsort(pi, kind="stable")
    return pi[o], pj[o]


def chunking(n, Gw=None, perw=None):
    """(Gw, perw) as the product derives them: perw = whole walk tiles covering n / Gw events."""
    if perw is None:
        if Gw is None:
            Gw = (n + WALK_TILE - 1) // WALK_TILE
        perw = -(-(-(-n // Gw)) // WALK_TILE) * WALK_TILE
    elif Gw is None:
        Gw = -(-n // perw)
    assert Gw * perw >= n
    return Gw, perw


def ptr(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def run(price, ordinals=None, window=None, Gw=None, perw=None, obase=0, poison=POISON):
    """Stage the model's pairs as the walk does, run both kernels, check cnt and dmax, and return the outcome."""
    n = len(price)
    rel = np.arange(n, dtype=np.int64) if ordinals is None else ordinals - obase
    assert rel[0] >= 0 and (np.diff(rel) > 0).all()
    pi, pj = walk_pairs(price, rel, window)
    M = len(pi)
    assert M > 0
    Gw, perw = chunking(n, Gw, perw)
    i, j = rel[pi], rel[pj]
    v = (j.astype(np.uint64) << np.uint64(32)) | i.astype(np.uint64)  # ascending position of i = chunk order
    g = pi // perw
    mcount = np.bincount(g, minlength=Gw).astype(np.uint32)
    assert (mcount <= perw).all()
    first = np.cumsum(mcount.astype(np.int64)) - mcount  # pairs before each chunk
    slot = g * perw + (np.arange(M) - first[g])  # ascending, as i
    stq = np.full(Gw * perw, SLACK, dtype=np.uint64)
    stq[slot] = v
    T = int(rel[-1] >> TB) + 1
    out = np.full(M + GUARD, SENTINEL, dtype=np.uint64)
    cnt = np.full(T + 1, 0x5A5A5A5A, dtype=np.uint32)
    P = np.zeros(T + 1, dtype=np.uint32)
    dmax = ctypes.c_uint32(0)
    err = ctypes.c_uint32(0)
    ordp = None if ordinals is None else ptr(np.ascontiguousarray(ordinals, dtype=np.int64), ctypes.c_int64)
    placed = lib().sm_jtile_emu(ptr(stq, ctypes.c_uint64), ptr(mcount, ctypes.c_uint32), ctypes.c_int64(perw), Gw, ordp,
                                ctypes.c_int64(obase), ctypes.c_int64(n), ctypes.c_uint32(T), ctypes.c_uint32(poison),
                                ptr(out, ctypes.c_uint64), ptr(cnt, ctypes.c_uint32), ptr(P, ctypes.c_uint32),
                                ctypes.byref(dmax), ctypes.byref(err))
    # the count kernel's results hold whatever the place kernel then makes of them
    np.testing.assert_array_equal(cnt, np.bincount(j >> TB, minlength=T + 1))
    assert dmax.value == int((j - i).max())
    assert (out[M:] == SENTINEL).all()
    exp = v[np.argsort(j, kind="stable")]
    return dict(placed=placed, err=err.value, out=out[:M], exp=exp, M=M, T=T, dmax=dmax.value, i=i, j=j, P=P,
                slot=slot, poison=poison, end=Gw * perw)


def check_P(r):
    """Every entry written, and each splitting the populated staging slots at its i-tile's first ordinal."""
    P, slot, i, M = r["P"], r["slot"], r["i"], r["M"]
    assert P[r["T"]] == r["end"]
    for u in range(r["T"]):
        assert P[u] != r["poison"], "P[%d] was never written" % u
        k = int(np.searchsorted(slot, P[u]))  # populated slots below P[u]
        assert k == 0 or i[k - 1] < TILE * u, (u, int(P[u]), "a pair of tile u or later lies before P[u]")
        assert k == M or i[k] >= TILE * u, (u, int(P[u]), "a pair of an earlier tile lies at or after P[u]")


def ok(r):
    """The tile path produced the output."""
    assert r["placed"] == 1
    assert r["err"] == 0, "placement error word %d" % r["err"]
    check_P(r)
    assert not (r["out"] == SENTINEL).any()
    np.testing.assert_array_equal(r["out"], r["exp"])
    return r


N = 20000


def spikes(n=N, seed=11):
    """Every event an e1; a price spike about every 300 events completes all that is pending: about a dozen partials
    (what is pending never rises from oldest to newest), 250 after a falling run (ties of j)."""
    rng = np.random.default_rng(seed)
    price = rng.uniform(21.0, 60.0, n)
    at = np.unique(rng.integers(0, n, n // 300))
    for s in at[at >= 250][::4]:  # a falling run before every fourth spike: 250 partials completed by one e2
        price[s - 250:s] = np.linspace(59.0, 21.5, 250)
    price[at] = 1000.0
    return price


def test_contiguous_ordinals():
    r = ok(run(spikes(), window=1000, perw=1024))
    assert r["T"] == 10 and r["M"] > N // 2
    assert np.bincount(r["j"]).max() > 100  # ties


OFFSETS = {"3k+1": lambda n: 3 * np.arange(n, dtype=np.int64) + 1,
           "from_1": lambda n: np.arange(n, dtype=np.int64) + 1,
           "from_2047": lambda n: np.arange(n, dtype=np.int64) + 2047,
           "from_2048": lambda n: np.arange(n, dtype=np.int64) + 2048,
           "from_2049": lambda n: np.arange(n, dtype=np.int64) + 2049,
           "from_5x2048+7": lambda n: np.arange(n, dtype=np.int64) + 5 * 2048 + 7}


@pytest.mark.parametrize("chunk0", ["full", "empty"])
@pytest.mark.parametrize("which", list(OFFSETS))
def test_first_ordinal_above_base(which, chunk0):
    """The first event's ordinal above the ordinal base: chunk 0 owns the i-tiles below it (their P is 0, the staging
    index of the first pair). `empty`: chunk 0 has no pair, and its m == 0 branch writes those entries."""
    price = spikes()
    if chunk0 == "empty":
        price[:1024] = 10.0
    ordv = OFFSETS[which](N)
    window = 3000 if which == "3k+1" else 1000
    r = ok(run(price, ordinals=ordv, window=window, perw=1024))
    assert (r["P"][:int(ordv[0] + TILE - 1) >> TB] == 0).all()


def test_first_ordinal_above_base_small_poison():
    """A stale entry that looks like a staging index (3) and not like garbage."""
    ok(run(spikes(), ordinals=np.arange(N, dtype=np.int64) + 2048, window=1000, perw=1024, poison=3))


def test_ordinal_base():
    """Absolute ordinals with their base: relative ordinals from 0 and from 5."""
    ok(run(spikes(), ordinals=np.arange(N, dtype=np.int64) + 70000, obase=70000, window=1000, perw=1024))
    ok(run(spikes(), ordinals=np.arange(N, dtype=np.int64) + 70005, obase=70000, window=1000, perw=1024))


def test_chunk_covers_two_tiles():
    ok(run(spikes(), window=1000, perw=4096))


def test_trailing_chunks_past_the_batch():
    """n = Gw 1024 + 1 with Gw given: chunks of 2048, one event in chunk 8, chunks 9 .. 15 start past the batch. The
    last event is a spike: the last tile holds the single ordinal 8 * 2048."""
    n = 16 * 1024 + 1
    price = spikes(n)
    price[-1] = 1000.0
    Gw, perw = chunking(n, Gw=16)
    assert perw == 2048 and 9 * perw >= n
    r = ok(run(price, window=1000, Gw=16, perw=perw))
    assert r["T"] == 9 and (r["j"] == 8 * TILE).sum() > 0


def test_last_tile_full():
    """The largest ordinal on a tile's last ordinal, a spike there."""
    n = 8 * TILE
    price = spikes(n)
    price[-1] = 1000.0
    r = ok(run(price, window=1000, perw=1024))
    assert r["T"] == 8 and (r["j"] == n - 1).sum() > 0


def test_ordinal_gaps():
    """Gaps in the ordinals: tiles that hold no ordinal at all, one chunk whose ordinal range spans more than ten tiles
    (five gaps inside chunk 4), a gap of exactly one tile and one that ends a chunk. The window is in ordinals, so no
    pair crosses a gap."""
    step = np.ones(N, dtype=np.int64)
    step[1500] += 5000
    step[[4200, 4400, 4600, 4800, 5000]] += 4500
    step[12000] += 2048
    step[15000] += 4097
    step[16384] += 3 * 2048  # the first event of chunk 16
    ordv = np.cumsum(step) - 1
    rel_tiles = set((ordv >> TB).tolist())
    assert len(rel_tiles) < int(ordv[-1] >> TB) + 1
    assert (ordv[5119] >> TB) - (ordv[4096] >> TB) >= 10
    ok(run(spikes(), ordinals=ordv, window=1000, perw=1024))
    ok(run(spikes(), ordinals=ordv + 2049, window=1000, perw=1024))


def test_chunk_reaches_past_its_local_counts():
    """The count kernel counts the 256 output tiles from a chunk's first one in LDS and any later one straight in
    memory: a gap of 260 tiles inside chunk 0 and inside chunk 1 puts half of each chunk's pairs past the 256."""
    n = 2048
    step = np.ones(n, dtype=np.int64)
    step[[512, 1536]] += 260 * TILE
    ordv = np.cumsum(step) - 1
    rng = np.random.default_rng(2)
    r = ok(run(rng.uniform(21.0, 60.0, n), ordinals=ordv, window=1000, perw=1024))
    assert r["T"] > 520 and ((r["j"] >> TB) >= 260).sum() > 100


@pytest.mark.parametrize("window", [1000, None])
def test_empty_chunks_in_the_middle(window):
    """Events 3000 .. 6999 are neither e1 nor e2 of anything pending (price 10): chunks 3, 4 and 5 hold no pair.
    Without a window the partials pending at 3000 complete after 7000 (j - i above 4000)."""
    price = spikes()
    price[3000:7000] = 10.0
    r = ok(run(price, window=window, perw=1024))
    if window is None:
        assert 4000 < r["dmax"] <= DMAX


def falling_run(n, start, L):
    price = np.full(n, 10.0)
    price[start:start + L] = np.linspace(59.0, 21.5, L)
    price[start + L] = 1000.0
    return price


def test_capacity_4096_pairs_on_one_j():
    r = ok(run(falling_run(12288, 3000, CAP), perw=1024))
    assert r["M"] == CAP and len(set(r["j"].tolist())) == 1


def test_capacity_4097_pairs_refused():
    r = run(falling_run(12288, 3000, CAP + 1), perw=1024)
    assert r["M"] == CAP + 1
    assert r["placed"] == 1 and r["err"] == 1
    check_P(r)
    assert (r["out"] == SENTINEL).all()  # the one tile that holds pairs placed none


def test_capacity_split_over_two_tiles():
    """More than 4096 pairs in the batch, at most 4096 per tile: 3000 on a j of tile 1, 3000 on a j of tile 3."""
    price = falling_run(12288, 1000, 3000)
    price[4001:4001 + 3000] = np.linspace(59.0, 21.5, 3000)
    price[7001] = 1000.0
    r = ok(run(price, perw=1024))
    assert r["M"] == 6000


@pytest.mark.parametrize("p", [1000, 2048, 4095])
def test_reach_8192(p):
    """One pair with j - i = 8192, the place kernel's reach; e1 on a tile's first and last ordinal."""
    price = np.full(14000, 10.0)
    price[p] = 50.0
    price[p + DMAX] = 1000.0
    r = ok(run(price, perw=1024))
    assert r["M"] == 1 and r["dmax"] == DMAX


def test_reach_8193_not_placed():
    price = np.full(14000, 10.0)
    price[1000] = 50.0
    price[1000 + DMAX + 1] = 1000.0
    r = run(price, perw=1024)
    assert r["dmax"] == DMAX + 1 and r["placed"] == 0 and r["err"] == 0
    check_P(r)
    assert (r["out"] == SENTINEL).all()


def test_reach_many_pairs():
    """Two thousand partials completed 6000 to 8000 ordinals later: the tile reads five i-tiles back."""
    price = np.full(14000, 10.0)
    price[500:2500] = np.linspace(59.0, 21.5, 2000)
    price[8500] = 1000.0
    r = ok(run(price, perw=1024))
    assert r["M"] == 2000 and r["dmax"] == 8000


def test_tile_edges_and_ties():
    """Spikes on a tile's first ordinal (4096, 10240) and on a tile's last (8191), each completing several hundred
    partials, from the tile before (3596 .. 4095), from across a tile boundary two tiles back (5900 .. 6399 over 6144)
    and one back (8000 .. 8399 over 8192). No window: a spike completes everything pending. Ties of j come out in
    ascending i."""
    n = 12288
    rng = np.random.default_rng(5)
    price = rng.uniform(21.0, 60.0, n)
    price[3596:4096] = np.linspace(59.0, 21.5, 500)
    price[4096] = 1000.0
    price[5900:6400] = np.linspace(59.0, 21.5, 500)
    price[6400:8191] = 10.0
    price[8191] = 1000.0
    price[8000 + 192:8400] = np.linspace(59.0, 21.5, 208)
    price[8400:10240] = 10.0
    price[9000:9002] = [21.0, 21.2]  # one pair inside tile 4, below everything pending
    price[10240] = 1000.0
    r = ok(run(price, perw=1024))
    oi, oj = (r["out"] & np.uint64(0xFFFFFFFF)).astype(np.int64), (r["out"] >> np.uint64(32)).astype(np.int64)
    for spike, least in ((4096, 500), (8191, 500), (10240, 208)):
        tie = oi[oj == spike]
        assert len(tie) >= least and (np.diff(tie) > 0).all()
    # the tiles before the first-ordinal spikes hold pairs themselves: their workgroups run, and must leave j = t1 alone
    assert ((oj >= TILE) & (oj < 2 * TILE)).any() and ((oj >= 4 * TILE) & (oj < 5 * TILE)).any()
