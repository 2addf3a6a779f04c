"""The ring kernel's epoch order (stack_dev.h, stack4_kernel: the prefetched slice e + kR is waited for before slice
e's staging stores, ranked after them, and slice e + kR + 1 is loaded after the ranking) under the host wave emulator,
at the bucket lengths where the ring's prologue, steady state and drain differ: exactly kR slices (no prefetch at
all), kR + 1 slices (one prefetch, consumed in the first epoch), an exact multiple of the slice with four slices,
three slices and one record (a one-record last slice), and a one-record bucket. Each with one key per bucket (every
record on one lane's stack) and with 1024 keys per bucket, with and without `within`, against the pending-list model
of tests/test_stack_emu.py (StreamPreStateProcessor.processAndReturn,
core/query/input/stream/state/StreamPreStateProcessor.java:274-327): staged pairs, tile offsets, totals and carry-out.
Test infrastructure: no GPU; `-m "not gpu"`."""
import numpy as np
import pytest

from test_stack_emu import check, consts, lib, run_case


def ring_keys(hkeys, seed):
    """Keys of five buckets (low digits 0..4) of kR, kR + 1, 4, 3 + one record and one record's worth of slices, in a
    random interleaving; the in-bucket key (high part) uniform below `hkeys`."""
    c = consts(lib())
    ss, r = c["ss"], c["r"]
    lengths = [r * ss, r * ss + 1, max(4, r + 2) * ss, 3 * ss + 1, 1]
    rng = np.random.default_rng(seed)
    digit = np.concatenate([np.full(n, b, np.int64) for b, n in enumerate(lengths)])
    rng.shuffle(digit)
    high = rng.integers(0, hkeys, len(digit))
    return (high << 10) | digit, lengths


@pytest.mark.parametrize("within", [1000, -1])
@pytest.mark.parametrize("hkeys", [1, 1024])
def test_ring_prologue_and_drain_lengths(hkeys, within):
    keys, lengths = ring_keys(hkeys, 5 + hkeys)
    n = len(keys)
    # random prices: a key's pending partials are its right-to-left price maxima, about ln(events of the key) of them,
    # so even one key per bucket stays inside the register stack and its spill ring without `within`
    r = run_case(n, hkeys << 10, 20, within=within, seed=11, grid=3, keys=keys)
    assert [int(x) for x in r["counts"][:5]] == lengths
    assert len(r["matches"]) > n // 4
    check(r)
