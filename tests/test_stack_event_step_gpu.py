"""The ring kernel's straight-line event step (stack_dev.h, stack4_kernel) on the GPU, for what the host emulator
does not instantiate (it runs `>` on a double only): the four ordered compares on a double attribute (inexact codes,
padding code per compare) and on an int and a narrow long attribute (exact codes), a tie-heavy stream (the general
step's exact compare), a stream without `within` whose stacks go through the spill ring, and two batches on one app
(carried partials pushed at the bucket's start must leave a padded stack). Bucket-stack pipeline forced
(fast_stack = 1), compared pair for pair with the CPU oracle (StreamPreStateProcessor.processAndReturn,
core/query/input/stream/state/StreamPreStateProcessor.java:274-327)."""
import numpy as np
import pytest

from test_bench_shape import oracle_subsample

pytestmark = pytest.mark.gpu

N = 1 << 16


def app_text(vt, op, c1=20, within=" within 1 sec"):
    return (f"define stream StockStream (symbol int, price {vt}, volume long, timestamp long); "
            "partition with (symbol of StockStream) begin "
            f"@info(name='q') from every e1=StockStream[price>{c1}] -> e2=StockStream[price {op} e1.price]{within} "
            "select e1.timestamp as i, e2.timestamp as j insert into OutputStream; end;")


def hot_keys(n, rng):
    """keys (h << 10) | b, h < 1024, b < 8: 8 hot buckets of n / 8 records (2.7 slices of 3072 at n = 2^16)"""
    return ((rng.integers(0, 1024, n) << 10) | rng.integers(0, 8, n)).astype(np.int32)


def device_pairs(text, sym, price, ts, ranges=None):
    """Global (e1, e2) ordinals of the batches [lo, hi) fed to one app, in output order; asserts the ring kernel ran."""
    import torch
    from siddhi_amd.testing import ProductApp
    app = ProductApp(text, fast_stack=1, fast_timing=1)
    app.set_collect(False)
    dev = torch.device("cuda", 0)
    n = len(sym)
    tsa = np.arange(n, dtype=np.int64)
    vol = np.zeros(n, dtype=np.int64)
    got = []
    for lo, hi in ranges or [(0, n)]:
        tcols = [torch.from_numpy(np.ascontiguousarray(c[lo:hi])).to(dev) for c in (sym, price, vol, tsa)]
        tts = torch.from_numpy(np.ascontiguousarray(ts[lo:hi], dtype=np.int64)).to(dev)
        torch.cuda.synchronize()
        app.process_device_batch("StockStream", tts, tcols, ordinal_base=lo)
        assert int(app.get_stat("fast_path:q")) == 3
        assert app.get_stat("kernel_calls:stack") > 0
        got.append(app.device_matches_host("q").view(np.int32).astype(np.int64) + lo)  # carried e1: negative
    app.close()
    return np.concatenate(got)


def compare(text, sym, price, ts, ranges=None, least=None):
    n = len(sym)
    exp = oracle_subsample(text, sym, price, ts, np.arange(n))
    assert len(exp) > (n // 8 if least is None else least), len(exp)
    np.testing.assert_array_equal(device_pairs(text, sym, price, ts, ranges), exp)


def column(vt, n, rng):
    if vt == "double":
        return rng.random(n) * 100.0, 20
    if vt == "int":
        return rng.integers(0, 100, n).astype(np.int32), 20  # equal values are common: exact codes decide them
    return (rng.integers(0, 100, n) - 30).astype(np.int64), -10  # narrow range: exact codes (value - minimum)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("op", [">", ">=", "<", "<="])
@pytest.mark.parametrize("vt", ["double", "int", "long"])
def test_ordered_compares_and_types_equal_oracle(vt, op):
    rng = np.random.default_rng(0xE5 + 7 * len(op) + ord(op[0]) + len(vt))
    sym = hot_keys(N, rng)
    price, c1 = column(vt, N, rng)
    ts = np.arange(N, dtype=np.int64) // 100
    compare(app_text(vt, op, c1), sym, price, ts)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("op", [">", "<="])
def test_tie_heavy_stream_equals_oracle(op):
    """16 prices: 8 pairs of equal 32-bit code and different value, so that most compares are ties"""
    rng = np.random.default_rng(0x71E)
    base = 30.0 + 5.0 * np.arange(8)
    pool = np.concatenate([base, np.nextafter(base, 1000.0)])
    sym = hot_keys(N, rng)
    price = pool[rng.integers(0, 16, N)]
    ts = np.arange(N, dtype=np.int64) // 100
    compare(app_text("double", op), sym, price, ts)


@pytest.mark.timeout(120)
def test_no_within_spill_ring_equals_oracle():
    """falling runs of 30 events per key, rising after each run: the stacks grow past kC into the spill ring and the
    rise pops them whole, through the refills"""
    n = 6200
    i = np.arange(n)
    sym = (i % 50).astype(np.int32)
    price = 99.0 - ((i // 50) % 31) * 2.5
    ts = np.arange(n, dtype=np.int64)
    compare(app_text("double", ">", within=""), sym, price, ts, least=n // 2)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("within", [" within 1 sec", ""])
def test_two_batches_carry_partials(within):
    """the second batch starts from the first one's pending partials: prices fall towards the split and rise after
    it, a few deep keys per bucket carry up to 21 partials (the carried pushes overfill the register part and spill),
    the others fewer than kC; 16 buckets, so that a slice's pops stay inside its pop pool"""
    rng = np.random.default_rng(0xCA221)
    n = 1 << 15
    deep = rng.random(n) < 0.12
    h = np.where(deep, rng.integers(0, 6, n), rng.integers(6, 256, n))
    sym = ((h << 10) | rng.integers(0, 16, n)).astype(np.int32)
    ramp = 70.0 * np.arange(n) / (n // 2)
    price = np.where(np.arange(n) < n // 2, 95.0 - ramp, ramp - 45.0) + rng.random(n) * 8.0
    ts = np.arange(n, dtype=np.int64) // 100
    text = app_text("double", ">", within=within)
    exp = oracle_subsample(text, sym, price, ts, np.arange(n))
    got = device_pairs(text, sym, price, ts, ranges=[(0, n // 2), (n // 2, n)])
    crossing = int(((exp[:, 0] < n // 2) & (exp[:, 1] >= n // 2)).sum())
    assert crossing > n // 16 and len(exp) > n // 8, (crossing, len(exp))
    np.testing.assert_array_equal(got, exp)
