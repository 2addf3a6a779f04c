"""Key pass 0's time-order check on the GPU (pass0_dev.h, pass0_kernel<OrigSrc<.., true>> behind the keys-only prep,
fastpath3.hip): the partitioned query of config 4 with int keys spread over more than 2^19 values, so that the batch
takes the bucket-stack route by itself and the flag is read with the pipeline's first read-back. n = 3 * 4096 + 17:
four chunks of one tile, the last one ragged. A batch whose event time decreases anywhere must reach the NFA kernel
(fast_path 5, as tests/test_device_stream.py expects of a non-monotone batch) with the reference's outputs; equal
neighbouring times are in order and stay on the closed form (fast_path 3). The reference keeps one pending list per
key across sends (StreamPreStateProcessor.java:274-327); the CPU oracle is compared pair for pair."""
import numpy as np
import pytest

from test_device_batch import app_text, oracle_pairs, stock
from test_device_stream import run_stream

pytestmark = pytest.mark.gpu

N = 3 * 4096 + 17
# lane, 16-lane row, wave-item, wave, tile / chunk boundaries of pass 0, and the ragged tile's first and last event
POSITIONS = [1, 16, 37, 48, 64, 192, 256, 3840, 4096, 8192, 3 * 4096, N - 1]


def batch():
    """300 keys spread over a span of about 9e5 (more than 2^19, less than 2^20), one event per ms."""
    cols, _ = stock(N, 300, 1)
    cols[0] = (cols[0].astype(np.int64) * 3001).astype(np.int32)
    assert int(cols[0].max()) - int(cols[0].min()) >= 1 << 19
    return cols, np.arange(N, dtype=np.int64) + 1_700_000_000_000


@pytest.mark.parametrize("p", POSITIONS)
def test_one_decrease_hands_over(p):
    cols, ts = batch()
    ts[p] = ts[p - 1] - 1
    text = app_text()
    exp = oracle_pairs(text, cols, ts)
    assert len(exp) > N // 8
    got = run_stream(text, cols, ts, [(0, N)], expect_path=5)
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("q", [2, 4097])
def test_time_2p32_later_between_small_ones_hands_over(q):
    """ts0 + 2^32 + 5 between ts0 + 3 and ts0 + 10: in order as far as the low words go"""
    cols, ts = batch()
    t0 = int(ts[0])
    ts[:] = t0 + 10
    ts[0], ts[1] = t0, t0 + 3
    ts[2:q] = t0 + 4
    ts[q] = t0 + (1 << 32) + 5
    text = app_text()
    exp = oracle_pairs(text, cols, ts)
    got = run_stream(text, cols, ts, [(0, N)], expect_path=5)
    np.testing.assert_array_equal(got, exp)


def test_equal_times_stay_on_the_closed_form():
    cols, ts = batch()
    for p in POSITIONS:
        ts[p] = ts[p - 1]
    assert (np.diff(ts) >= 0).all()
    text = app_text()
    exp = oracle_pairs(text, cols, ts)
    assert len(exp) > N // 8
    got = run_stream(text, cols, ts, [(0, N)], expect_path=3)
    np.testing.assert_array_equal(got, exp)


def test_monotone_batch_takes_the_stack_route():
    cols, ts = batch()
    text = app_text()
    exp = oracle_pairs(text, cols, ts)
    got = run_stream(text, cols, ts, [(0, N)], expect_path=3)
    np.testing.assert_array_equal(got, exp)


def _two_batches(ts_edit):
    """Two batches of N events on one app; returns (pairs, expected pairs, fast_path after each batch)."""
    import torch
    from siddhi_amd.testing import ProductApp
    n = 2 * N
    cols, _ = stock(n, 300, 1)
    cols[0] = (cols[0].astype(np.int64) * 3001).astype(np.int32)
    ts = np.arange(n, dtype=np.int64) + 1_700_000_000_000
    ts_edit(ts)
    text = app_text()
    exp = oracle_pairs(text, cols, ts)
    crossing = int(((exp[:, 0] < N) & (exp[:, 1] >= N)).sum())
    assert crossing > 50, crossing  # the first batch's carry is not empty and the second batch completes it
    app = ProductApp(text)
    dev = torch.device("cuda", 0)
    got, paths = [], []
    for lo, hi in [(0, N), (N, n)]:
        tcols = [torch.from_numpy(np.ascontiguousarray(c[lo:hi])).to(dev) for c in cols]
        tts = torch.from_numpy(np.ascontiguousarray(ts[lo:hi])).to(dev)
        torch.cuda.synchronize()
        app.process_device_batch("StockStream", tts, tcols, ordinal_base=lo)
        got.append(app.device_matches_host("q").view(np.int32).astype(np.int64) + lo)
        paths.append(int(app.get_stat("fast_path:q")))
    app.close()
    return np.concatenate(got), exp, paths


def test_second_batch_non_monotone_with_carried_partials():
    def edit(ts):
        ts[N + 4096] = ts[N + 4095] - 1
    got, exp, paths = _two_batches(edit)
    assert paths == [3, 5]
    np.testing.assert_array_equal(got, exp)


def test_two_batches_carry_out_equals_oracle():
    got, exp, paths = _two_batches(lambda ts: None)
    assert paths == [3, 3]
    np.testing.assert_array_equal(got, exp)
