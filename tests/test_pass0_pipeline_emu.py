"""Key pass 0's software pipeline (pass0_dev.h: the records of tile t+1 are built after tile t's placement and
before tile t's stores; the carried records that leave with tile t are read into registers before the barrier that
frees their slots) under the host wave emulator, at the shapes that exercise its prologue (a chunk's first tile), its
epilogue (the chunk's last tile is stored by an iteration that builds no records), one-tile chunks and a one-record
last tile. The output must be the stable digit partition (tests/test_pass0_emu.py: run), which is what the
partitioned key lookup of the reference needs of the bucketing (core/partition/PartitionRuntime: a key's events stay
in arrival order). Test infrastructure: no GPU; `-m "not gpu"`."""
import numpy as np
import pytest

from test_pass0_emu import BINS, TILE, run


@pytest.mark.parametrize("n,G", [(TILE, 1), (2 * TILE, 1), (2 * TILE, 2), (6 * TILE, 3),  # exact multiples; the last
                                 # one has two full tiles per chunk
                                 (2 * TILE + 1, 1),    # a one-record last tile
                                 (4 * TILE + 63, 2)])  # chunks of 3 tiles: the second ends 63 records into its last
def test_pipeline_prologue_and_epilogue_shapes(n, G):
    keys = np.random.default_rng(n * 31 + G).integers(0, 1 << 20, n)
    run(keys, G)


def test_single_digit_keeps_the_carry_in_use():
    """every record in one digit: each tile's run ends inside a 64-byte segment or on its edge, and the carry slots
    are read and refilled at every tile boundary (4 tiles and 3 records, so the tile ends walk through the segment)"""
    n = 4 * TILE + 3
    keys = np.full(n, 5 + 7 * BINS, np.int64)
    keys[::3] += BINS  # the same digit from two keys
    run(keys, 1)
    run(keys[:3 * TILE + 1], 2)


def test_sparse_digits_store_only_from_the_carry_and_the_flush():
    """every digit gets 1-3 records per tile: no segment completes inside a tile, so a tile's own records all go to
    the carry, and records leave only as carried ones (when a later tile completes their segment) or in the last
    tile's flush. A full tile holds 4096 records, four per digit on average, so in the multi-tile run four filler
    digits take what the other 1020 (1-3 records each) leave of each tile; the one-tile run (a last tile of at most
    3072 records) has every digit at 1-3 records and stores nothing but the flush."""
    rng = np.random.default_rng(77)
    per = rng.integers(1, 4, BINS)
    one = np.repeat(np.arange(BINS), per)
    rng.shuffle(one)
    assert len(one) <= 3 * BINS
    run(one + BINS * rng.integers(0, 900, len(one)), 1)

    fill = np.arange(BINS - 4, BINS)
    parts = []
    for _ in range(4):
        per = rng.integers(1, 4, BINS - 4)
        d = np.repeat(np.arange(BINS - 4), per)
        d = np.concatenate([d, fill[rng.integers(0, 4, TILE - len(d))]])
        rng.shuffle(d)
        assert len(d) == TILE and np.bincount(d, minlength=BINS)[:BINS - 4].max() <= 3
        parts.append(d)
    digits = np.concatenate(parts + [parts[0][:1500]])  # and a ragged last tile
    keys = digits + BINS * rng.integers(0, 900, len(digits))
    run(keys, 1)
    run(keys[:4 * TILE], 2)
