"""The workgroup-wide exclusive scan (fastpath_dev.h: block_excl over wave_incl_scan, DPP adds) as the kernels of the
bucket-stack pipeline use it on the GPU: the ranking and emission scans of the ring kernel over in-bucket keys, key
pass 0's scan over digits, and the order kernel's segment and offset scans over buckets. The streams put their
events on the threads where a wrong row or wave carry shows: the first and last lane of every 16-lane row of wave 0
(0, 15, 16, 31, 32, 47, 48, 63), the first lane of wave 1 (64) and the last thread (1023). Config-4 query, pipeline
forced (fast_stack = 1), compared pair for pair with the CPU oracle."""
import numpy as np
import pytest

from test_bench_shape import oracle_subsample
from test_stack_event_step_gpu import app_text, compare, device_pairs

pytestmark = pytest.mark.gpu

EDGE_KEYS = np.array([0, 15, 16, 31, 32, 47, 48, 63, 64, 1023])  # in-bucket key h: thread h of the ring kernel
EDGE_BUCKETS = np.array([15, 16, 63, 64, 1023])                   # bucket = key's low digit: thread of pass 0 / order
N2 = 3072 + 1                                                     # two slices of the ring kernel: one full, one record
TEXT = app_text("double", ">")


def stream(n, h, b, seed):
    """keys (h << 10) | b (key 0's bucket decides the rebase: h = 0 is in every key set, so h and b are the
    kernels' thread indices as given), random prices, 100 events per ms"""
    rng = np.random.default_rng(seed)
    sym = ((rng.choice(h, n) << 10) | rng.choice(b, n)).astype(np.int32)
    sym[0] = b[0]  # h = 0 present
    return sym, rng.random(n) * 100.0, np.arange(n, dtype=np.int64) // 100


@pytest.mark.timeout(60)
def test_edge_keys_of_one_bucket():
    """ten keys of one bucket, two slices: the ranking scan's key starts and the emission scan's offsets cross
    every row and wave edge"""
    sym, price, ts = stream(N2, EDGE_KEYS, np.array([5]), 0xB5C1)
    compare(TEXT, sym, price, ts, least=N2 // 4)


@pytest.mark.timeout(60)
def test_edge_keys_over_edge_buckets():
    """the same keys over five buckets: pass 0's digit starts and the order kernel's segment starts and ordinal
    offsets cross the row and wave edges of the bucket index"""
    sym, price, ts = stream(N2, EDGE_KEYS, EDGE_BUCKETS, 0xB5C2)
    assert set((sym & 1023).tolist()) == set(EDGE_BUCKETS.tolist())
    compare(TEXT, sym, price, ts, least=N2 // 8)


@pytest.mark.timeout(60)
def test_one_record():
    compare(TEXT, np.array([7 << 10], np.int32), np.array([50.0]), np.zeros(1, np.int64), least=-1)


@pytest.mark.timeout(60)
def test_one_bucket_with_a_single_key():
    """every record on thread 1023's key: all other threads scan zeros"""
    n = 700
    rng = np.random.default_rng(0xB5C3)
    sym = np.full(n, (1023 << 10) | 1023, np.int32)
    compare(TEXT, sym, rng.random(n) * 100.0, np.arange(n, dtype=np.int64) // 100, least=n // 4)


@pytest.mark.timeout(60)
def test_two_batches_with_carried_partials():
    """the second batch starts from the first one's carry-out (a wave scan of the pending counts per key) on the
    edge keys and buckets: every key's pending partials at the split are the right-to-left minima of its prices, a
    handful per key, which stays inside the pipeline's per-slice pop pool"""
    n = 2 * N2
    sym, price, ts = stream(n, EDGE_KEYS, EDGE_BUCKETS, 0xB5C4)
    exp = oracle_subsample(TEXT, sym, price, ts, np.arange(n))
    crossing = int(((exp[:, 0] < n // 2) & (exp[:, 1] >= n // 2)).sum())
    assert crossing > len(EDGE_KEYS) * len(EDGE_BUCKETS) and len(exp) > n // 8, (crossing, len(exp))
    got = device_pairs(TEXT, sym, price, ts, ranges=[(0, n // 2), (n // 2, n)])
    np.testing.assert_array_equal(got, exp)
