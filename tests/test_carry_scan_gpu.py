"""Carry-out of the bucket-stack pipeline without a sort (stack.hip, build_carry_runs): after the ring kernel the carry
rows are placed by a scan of the keys' run lengths in key order. 5120 keys (h << 10 | d, h < 5, every bucket d), three
batches on one app; at each split a key holds 1 to kC + 2 pending partials (a clearing event, then a falling ladder),
a third of the keys keep their carried partials over a batch (rows copied from the old carry), and every key's first
event of a later batch is a probe with price A, B (equal 32-bit codes, different values: the exact compare reads the
carry rows), 65 or 99.9. Checked pair for pair against the CPU oracle, and the carry rows (sm_app_snapshot after each
batch) byte for byte against the sort route (SM_CARRY_SORT=1, read per call) in the same process. In one case the
second batch leaves out the keys with h = 0 and h = 4: their carried partials are appended out of range, which takes
the sort route, and the third batch returns to the scan."""
import os

import numpy as np
import pytest

from test_bench_shape import oracle_subsample
from test_stack_event_step_gpu import app_text

pytestmark = pytest.mark.gpu

A = 50.0  # the tie prices of test_stack_event_step_emu.py
B = float(np.nextafter(50.0, 100.0))  # the same 32-bit code as A, a larger value

NH, NB = 5, 1024
LADDERS = ([85.0, 75.0, 65.0, 55.0, B, A], [85.0, 75.0, 65.0, 55.0, 52.0, B])
PROBES = (A, B, 65.0, 99.9)


def key_events(k, b):
    """prices of key k's events in batch b, in order"""
    hold = k % 3 == 0  # keeps its carried partials: no clearing event after batch 0
    m = 1 + (k * 7 + (k >> 10)) % 7
    if hold:
        m = min(m, 5)  # + one probe per later batch: kC + 2 at most
    ev = []
    if b > 0:
        ev.append(PROBES[(k // 3 + b) % 4])
    if b == 0 or not hold:
        ev.append(96.0 + b)
        ev += LADDERS[k & 1][len(LADDERS[0]) - (m - 1):] if m > 1 else []
    return ev


def stream(narrow_second):
    """sym, price and the batches' [lo, hi): round r of a batch holds event r of every key that has one"""
    sym, price, ranges = [], [], []
    for b in range(3):
        lo = len(sym)
        keys = [(h << 10) | d for h in range(NH) for d in range(NB)
                if not (narrow_second and b == 1 and h in (0, NH - 1))]
        evs = {k: key_events(k, b) for k in keys}
        for r in range(8):
            for k in keys:
                if r < len(evs[k]):
                    sym.append(k)
                    price.append(evs[k][r])
        ranges.append((lo, len(sym)))
    return np.array(sym, dtype=np.int32), np.array(price, dtype=np.float64), ranges


def run(text, sym, price, ts, ranges, sort_route):
    """pairs of every batch, the snapshot after each batch, and whether each batch's carry was placed by the scan"""
    import torch
    from siddhi_amd.testing import ProductApp
    app = ProductApp(text, fast_stack=1, fast_timing=1)
    app.set_collect(False)
    dev = torch.device("cuda", 0)
    n = len(sym)
    tsa = np.arange(n, dtype=np.int64)
    vol = np.zeros(n, dtype=np.int64)
    got, snaps, scans = [], [], []
    for lo, hi in ranges:
        tcols = [torch.from_numpy(np.ascontiguousarray(c[lo:hi])).to(dev) for c in (sym, price, vol, tsa)]
        tts = torch.from_numpy(np.ascontiguousarray(ts[lo:hi], dtype=np.int64)).to(dev)
        torch.cuda.synchronize()
        if sort_route:
            os.environ["SM_CARRY_SORT"] = "1"
        try:
            app.process_device_batch("StockStream", tts, tcols, ordinal_base=lo)
        finally:
            os.environ.pop("SM_CARRY_SORT", None)
        assert int(app.get_stat("fast_path:q")) == 3
        assert app.get_stat("kernel_calls:stack") > 0
        scans.append(int(app.get_stat("kernel_calls:carry_by_scan")))
        got.append(app.device_matches_host("q").view(np.int32).astype(np.int64) + lo)
        snaps.append(app.snapshot())
    app.close()
    return np.concatenate(got), snaps, scans


@pytest.mark.timeout(120)
@pytest.mark.parametrize("within,narrow_second", [("", False), (" within 1 sec", False), ("", True)])
def test_carry_by_scan_equals_oracle_and_sort_route(within, narrow_second):
    sym, price, ranges = stream(narrow_second)
    n = len(sym)
    ts = np.arange(n, dtype=np.int64) // 20  # about 2.3 s in all: with `within 1 sec` old partials expire
    text = app_text("double", ">", within=within)
    exp = oracle_subsample(text, sym, price, ts, np.arange(n))
    crossing = int(((exp[:, 0] < ranges[1][0]) & (exp[:, 1] >= ranges[1][0])).sum())
    assert crossing > 2000 and len(exp) > n // 8, (crossing, len(exp))
    got, snaps, scans = run(text, sym, price, ts, ranges, sort_route=False)
    assert scans == ([1, 0, 1] if narrow_second else [1, 1, 1]), scans
    np.testing.assert_array_equal(got, exp)
    got_s, snaps_s, scans_s = run(text, sym, price, ts, ranges, sort_route=True)
    assert scans_s == [0, 0, 0], scans_s
    np.testing.assert_array_equal(got_s, exp)
    for b in range(3):
        assert len(snaps[b]) > 8 * 4 * NB  # the carry rows are in it
        assert snaps[b] == snaps_s[b], f"carry rows differ after batch {b}"
