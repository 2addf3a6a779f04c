"""The ring kernel's straight-line event step (stack_dev.h, stack4_kernel: sentinel-padded register stack, pop run as
two counts, the shift as selects, general step for ties / refills / a push onto a full stack) under the host wave
emulator, on crafted streams at the smallest shapes where it can go wrong, against the pending-list model of
tests/test_stack_emu.py (StreamPreStateProcessor.processAndReturn,
core/query/input/stream/state/StreamPreStateProcessor.java:274-327). The emulator build also asserts the step's
invariants (padding, c2 on a prefix, expiry on a suffix) at every event that takes the straight-line step.

Streams are laid out in rounds: every case has its own key and one event per round (a filler with price 10, which
satisfies neither c1 nor c2 against any partial, where the case has none), with div = number of cases, so that a
case's events have the times 0, 1, 2, ... Layout "buckets": one key per bucket (one busy lane per workgroup);
layout "lanes": every key in bucket 0, so that the lanes of a wave diverge on the pop count, the expiry and the path
taken. Test infrastructure: no GPU; `-m "not gpu"`."""
import numpy as np
import pytest

from test_stack_emu import check, consts, lib, run_case

FILL = 10.0
SE_OVERFLOW = 1


def kc():
    return consts(lib())["c"]


def lay_out(cases, layout):
    """cases: per case the prices by round (None: filler). Returns run_case arguments."""
    C, R = len(cases), max(len(c) for c in cases) + 1
    price = np.full((R, C), FILL)
    for c, seq in enumerate(cases):
        for r, p in enumerate(seq):
            if p is not None:
                price[r, c] = p
    key = np.arange(C, dtype=np.int64)
    if layout == "lanes":
        assert C <= 1024
        key = key << 10
    else:
        assert C <= 1024
    keys = np.tile(key, R)
    assert len(keys) <= 20000
    return dict(n=len(keys), K=int(keys.max()) + 1, div=C, keys=keys, price=price.reshape(-1).copy())


def run_rounds(cases, layout, within):
    a = lay_out(cases, layout)
    r = run_case(a["n"], a["K"], a["div"], within=within, grid=2, price=a["price"], keys=a["keys"])
    r["price"] = a["price"]
    return r


def staircase(L, m, gap=0):
    """A falling run of L events (90, 88, ...), `gap` rounds without an event, one event that beats exactly the m
    youngest of them, then one that beats everything still pending."""
    run = [90.0 - 2.0 * i for i in range(L)]
    popper = 90.0 - 2.0 * (L - m) + 1.0
    return run + [None] * gap + [popper, 99.5]


@pytest.mark.parametrize("layout", ["buckets", "lanes"])
@pytest.mark.parametrize("within", [1000, -1])
def test_pop_run_lengths(layout, within):
    """every run length 1 .. kC + 3 (beyond kC: spills on the way down, refills on the way up) and every pop count"""
    cases = [staircase(L, m) for L in range(1, kc() + 4) for m in range(L + 1)]
    r = run_rounds(cases, layout, within)
    assert len(r["matches"]) >= sum(len(c) - 2 for c in cases)  # the last event pops whatever was left
    check(r)


@pytest.mark.parametrize("layout", ["buckets", "lanes"])
def test_expiry_inside_a_run(layout):
    """run at times 0 .. L-1, within = L + 2, the popping event at time within + e: the e oldest entries have expired.
    Over every (L, m, e): the run stops at the first expired entry and clears what is beneath it (m >= L - e), the
    expired entry is not the one the price would have stopped at (m > L - e), an expired entry is never reached
    (m < L - e), nothing has expired (e = 0), everything has (e = L)."""
    for L in range(1, kc() + 3):
        W = L + 2
        cases = [staircase(L, m, gap=W + e - L) for m in range(L + 1) for e in range(L + 1)]
        r = run_rounds(cases, layout, W)
        assert len(r["matches"]) > 0
        check(r)


A = 50.0
B = float(np.nextafter(50.0, 100.0))  # the same 32-bit code as A, a larger value


@pytest.mark.parametrize("layout", ["buckets", "lanes"])
def test_ties_of_inexact_codes(layout):
    """a partial with price A or B at depth k of a full register stack (top, middle, bottom register entry), k younger
    partials below 50 above it, older ones above 50 beneath; the event has price A or B: it pops the k younger ones and
    the exact compare decides the tied one each way (B > A pops; A > B, A > A, B > B do not)"""
    C = kc()
    cases = []
    for k in (0, C // 2, C - 1):
        for tied in (A, B):
            for ev in (A, B):
                run = [90.0 - 2.0 * i for i in range(C - 1 - k)] + [tied] + [48.0 - 2.0 * i for i in range(k)]
                cases.append(run + [ev, 99.5])
    r = run_rounds(cases, layout, 1000)
    popped = sum(1 for i, j in r["matches"] if r["price"][i] == A and r["price"][j] == B)
    assert popped >= 3
    check(r)


def test_tie_model_sees_exact_values():
    """the codes of A and B are equal, their values are not (else the tie test above checks nothing)"""
    from test_stack_emu import vcode
    assert vcode(np.array([A]))[0] == vcode(np.array([B]))[0] and B > A


@pytest.mark.parametrize("layout", ["buckets", "lanes"])
def test_push_on_a_full_stack_and_plain_steps(layout):
    C = kc()
    W = C + 4
    full = [90.0 - 2.0 * i for i in range(C)]
    cases = [
        full + [30.0, 29.0, 99.5],                                  # live bottom: spilled, twice; then all popped
        [90.0] + [None] * 5 + full[1:] + [30.0, 99.5],              # bottom older than `within` at the push: dropped
        [90.0] + [None] * 5 + full[1:] + [None, 30.0, 99.5],        # ... and when it expired a round earlier
        full + [15.0, 99.5],                                        # neither c1 nor c2 on a full stack: unchanged
        [60.0, 15.0, 59.0, 99.5],                                   # no c1 (price <= 20) between pushes
        [60.0, 50.0, 40.0, 99.5],                                   # push only
        [99.0],                                                     # a key's first event, nothing after it
        [None, None, 25.0, 26.0],                                   # first event late
    ]
    r = run_rounds(cases, layout, W)
    r2 = run_rounds(cases, layout, -1)
    assert len(r["matches"]) > 0 and len(r2["matches"]) > len(r["matches"])
    check(r)
    check(r2)


def test_lookahead_crosses_slots():
    """bucket 0 holds two and a bit slices: key `late` has its only events in the second held slice and beyond, key
    `both` in every slice, the other keys fill the slices; lanes go on into the second slot inside one epoch"""
    c = consts(lib())
    ss = c["ss"]
    n = 2 * ss + 200
    rng = np.random.default_rng(77)
    h = rng.integers(10, 400, n)
    late, both = 5, 6
    h[rng.choice(np.arange(ss, n), 60, replace=False)] = late
    h[np.arange(3, n, 97)] = both
    assert (h[:ss] != late).all() and (h[:ss] == both).any() and (h[ss:2 * ss] == both).any()
    keys = (h.astype(np.int64) << 10)
    r = run_case(n, int(keys.max()) + 1, 7, within=1000, seed=3, grid=1, keys=keys)
    assert len(r["matches"]) > n // 4
    assert any(r["keys"][j] == late << 10 for _, j in r["matches"])
    check(r)


def test_overflow_flag():
    """more than kC + kQ live partials on one key, no `within`: SE_OVERFLOW (the walk pipeline takes the batch)"""
    c = consts(lib())
    n = c["c"] + c["q"] + 3
    keys = np.zeros(n, np.int64)
    price = 99.0 - 0.5 * np.arange(n)
    assert price.min() > 20.0
    r = run_case(n, 1, 1, within=-1, grid=1, price=price, keys=keys)
    assert r["err"] & SE_OVERFLOW
    # one fewer than the capacity + 1 does not overflow, and everything is still there for the last event
    n = c["c"] + c["q"]
    price = np.concatenate([99.0 - 0.5 * np.arange(n), [99.5]])
    r = run_case(n + 1, 1, 1, within=-1, grid=1, price=price, keys=np.zeros(n + 1, np.int64))
    assert len(r["matches"]) == n
    check(r)
