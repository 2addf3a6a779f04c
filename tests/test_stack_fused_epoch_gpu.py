"""The ring kernel's fused epoch (stack_dev.h, chain4: slice e's emission and slice e + kR's ranking in one chain of
barriers, the ranking's counts on the slot's key-grouped records) on the GPU, pair for pair against the CPU oracle
(StreamPreStateProcessor.processAndReturn, core/query/input/stream/state/StreamPreStateProcessor.java:274-327), at
the bucket lengths where the ring's prologue, steady state and drain differ (kSS = 3072 records per slice, kR = 2
slices held): kSS - 1, kSS, kSS + 1, kR kSS, kR kSS + 1, (kR + 2) kSS, 3 kSS + 1 and 1, over buckets that include
0, 15, 64 and 1023, half of the records on the in-bucket keys 0, 63, 64 and 1023 (first and last lane of the first
two waves and of the workgroup). Per key the compared attribute comes in pairs moving away from the next event's
reach followed by one that beats both, each triple beyond the one before: three pops per triple, one of them through
the slot's pool, so that pool entries of slice e are read while slice e + kR is counted, and no stack grows."""
import numpy as np
import pytest

from test_stack_event_step_gpu import app_text, compare, device_pairs
from test_bench_shape import oracle_subsample

pytestmark = pytest.mark.gpu

SS, R = 3072, 2
LENGTHS = [SS - 1, SS, SS + 1, R * SS, R * SS + 1, (R + 2) * SS, 3 * SS + 1, 1]
BUCKETS = [0, 15, 64, 1023, 1, 16, 63, 512]
EDGE = np.array([0, 63, 64, 1023])


def stream(seed):
    rng = np.random.default_rng(seed)
    digit = np.concatenate([np.full(n, b, np.int64) for b, n in zip(BUCKETS, LENGTHS)])
    rng.shuffle(digit)
    n = len(digit)
    high = np.where(rng.random(n) < 0.5, EDGE[rng.integers(0, 4, n)], rng.integers(0, 1024, n))
    return ((high << 10) | digit).astype(np.int32)


def triples(sym):
    """Per key: two falling values and a peak above them, every triple above the one before (from 30 up)."""
    occ = np.zeros(len(sym), np.int64)
    seen = {}
    for j, k in enumerate(sym.tolist()):
        occ[j] = seen.get(k, 0)
        seen[k] = occ[j] + 1
    t, ph = occ // 3, occ % 3
    return 30 + 12 * t + np.where(ph == 2, 10, 2 * (2 - ph))


def column(sym, vt, op):
    v = triples(sym)
    if op == "<=":  # mirrored: two rising values and a trough below them, every triple below the one before
        v = 1_000_000 - v
    return v.astype(np.float64) if vt == "double" else v.astype(np.int32)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("within", [" within 1 sec", ""])
@pytest.mark.parametrize("vt,op", [("double", ">"), ("int", "<=")])
def test_bucket_lengths_equal_oracle(vt, op, within):
    sym = stream(0xF5ED)
    n = len(sym)
    assert 40_000 < n < 60_000
    ts = np.arange(n, dtype=np.int64) // 20  # 1 sec = 20 000 events: some partials of the rarer keys expire
    compare(app_text(vt, op, within=within), sym, column(sym, vt, op), ts, least=n // 4)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("within", [" within 1 sec", ""])
@pytest.mark.parametrize("vt,op", [("double", ">"), ("int", "<=")])
def test_two_batches_carry_partials(vt, op, within):
    """the split falls inside the triples of most keys: the second batch pops carried partials, the older of a pair
    through the pool"""
    sym = stream(0xCA77)
    n = len(sym)
    price = column(sym, vt, op)
    ts = np.arange(n, dtype=np.int64) // 20
    text = app_text(vt, op, within=within)
    exp = oracle_subsample(text, sym, price, ts, np.arange(n))
    cut = n // 2 + 1
    crossing = int(((exp[:, 0] < cut) & (exp[:, 1] >= cut)).sum())
    assert crossing > 1000 and len(exp) > n // 4, (crossing, len(exp))
    np.testing.assert_array_equal(device_pairs(text, sym, price, ts, ranges=[(0, cut), (cut, n)]), exp)
