"""The software-pipelined key pass 0 (pass0_dev.h: a tile's stores are issued after the wait for the next tile's
loads) and the ring kernel's pre-emission wait (stack_dev.h) on the GPU, at the shapes where the new order of work
can go wrong: chunks of several tiles in pass 0 (prologue, steady state and last tile of the pipeline), buckets of
many slices in the ring kernel (the prefetched slice is consumed before the emission's stores in every epoch), the
ordinal column of the sharded path (OrigSrc subtracts the ordinal base where the ordinal is used), and the smallest
batches (one record, exactly one tile, one tile and one record). Bucket-stack pipeline forced (fast_stack = 1), the
config-4 query, compared pair for pair with the brute-force closed form or the CPU oracle
(StreamPreStateProcessor.processAndReturn, core/query/input/stream/state/StreamPreStateProcessor.java:274-327)."""
import numpy as np
import pytest

import bench
from test_bench_shape import closed_form_torch, oracle_subsample, product_pairs

pytestmark = pytest.mark.gpu


def _dev():
    import torch
    return torch.device("cuda", 0)


def _pairs(sym, price, ts, ordinals=None):
    """(e1, e2) rows of the config-4 query on the bucket-stack pipeline, in output order; numpy columns in."""
    import torch
    from siddhi_amd.testing import ProductApp
    app = ProductApp(bench.APP, fast_stack=1)
    app.set_collect(False)
    d = _dev()
    tsym = torch.from_numpy(np.ascontiguousarray(sym, dtype=np.int32)).to(d)
    tprice = torch.from_numpy(np.ascontiguousarray(price, dtype=np.float64)).to(d)
    tts = torch.from_numpy(np.ascontiguousarray(ts, dtype=np.int64)).to(d)
    tord = torch.from_numpy(np.ascontiguousarray(ordinals, dtype=np.int64)).to(d) if ordinals is not None else None
    torch.cuda.synchronize()
    app.process_device_batch("StockStream", tts, [tsym, tprice, tprice, tprice], ordinals=tord, ordinal_base=0)
    path = int(app.get_stat("fast_path:q"))
    got = app.device_matches_host("q").astype(np.int64)
    app.close()
    assert path == 3, path
    return got


@pytest.fixture(scope="module")
def hot_buckets():
    """2^18 events on 8 hot buckets: keys (h << 10) | b, h < 1024, b < 8, so a bucket holds about 32768 records
    (10.7 slices of 3072) with about 3 events per key per slice, the bench's density. The oracle's pairs once."""
    n = 1 << 18
    rng = np.random.default_rng(0x51DD)
    sym = ((rng.integers(0, 1024, n) << 10) | rng.integers(0, 8, n)).astype(np.int32)
    price = rng.random(n) * 100.0
    ts = np.arange(n, dtype=np.int64) // 100
    return dict(n=n, sym=sym, price=price, ts=ts)


@pytest.mark.timeout(300)
def test_pass0_multi_tile_chunks_equal_brute_force():
    """3 * 2^21 + 17 events: 512 chunks of 4 tiles (3 full chunks' worth and a ragged end), 2000 keys, ts = i // 10."""
    import torch
    from siddhi_amd.testing import ProductApp
    n = 3 * (1 << 21) + 17
    sym, price, vol, tsa, ts = bench.gen_stock(0, n, 2000, 10, _dev(), bench.seed_for(4))
    del vol, tsa
    torch.cuda.synchronize()
    app = ProductApp(bench.APP, fast_stack=1, fast_timing=1)
    app.set_collect(False)
    app.process_device_batch("StockStream", ts, [sym, price, price, price])
    assert int(app.get_stat("fast_path:q")) == 3
    assert app.get_stat("kernel_calls:stack") > 0
    got = product_pairs(app, n).clone()
    app.close()
    ref = closed_form_torch(sym.to(torch.int64), price, ts, 1000)
    assert ref.numel() == got.numel() > n // 2, (ref.numel(), got.numel())
    assert torch.equal(ref, got)


@pytest.mark.timeout(300)
def test_stack_many_slice_buckets_equal_oracle(hot_buckets):
    c = hot_buckets
    exp = oracle_subsample(bench.APP, c["sym"], c["price"], c["ts"], np.arange(c["n"]))
    assert len(exp) > c["n"] // 4
    np.testing.assert_array_equal(_pairs(c["sym"], c["price"], c["ts"]), exp)


@pytest.mark.timeout(300)
def test_ordinal_column_equals_oracle_subset(hot_buckets):
    """The same stream as one rank's subset of a larger one: ordinals 3k + 1, strictly increasing with gaps."""
    c = hot_buckets
    ordn = 3 * np.arange(c["n"], dtype=np.int64) + 1
    exp = oracle_subsample(bench.APP, c["sym"], c["price"], c["ts"], ordn)
    assert len(exp) > c["n"] // 4
    np.testing.assert_array_equal(_pairs(c["sym"], c["price"], c["ts"], ordinals=ordn), exp)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", [1, 4096, 4097])
def test_edge_sizes_equal_oracle(n):
    """one record; exactly one pass-0 tile; one tile and a one-record last tile"""
    rng = np.random.default_rng(n)
    sym = rng.integers(0, 50, n).astype(np.int32)
    price = rng.random(n) * 100.0
    ts = np.arange(n, dtype=np.int64) // 3
    exp = oracle_subsample(bench.APP, sym, price, ts, np.arange(n))
    if n > 1:
        assert len(exp) > n // 4
    np.testing.assert_array_equal(_pairs(sym, price, ts).reshape(-1, 2), exp)
