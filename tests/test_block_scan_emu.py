"""The workgroup-wide exclusive scan of the hot kernels (siddhi_amd/csrc/kernels/fastpath_dev.h: block_excl over
wave_incl_scan, six DPP adds per wave and a 16-lane row scan of the wave totals) run on the CPU under the host wave
emulator (tests/native/block_scan_emu.cpp: the same device source; hd.h models the row_shr / row_bcast controls),
against a plain prefix sum mod 2^32, for the 1024-thread workgroup of the ring, order and pass-0 kernels and the
512-thread one of the v2 stack kernel.
Test infrastructure: no GPU; `-m "not gpu"`."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
LIB = os.path.join(NATIVE, "build", "libblock_scan_emu.so")
KERNELS = os.path.join(HERE, "..", "siddhi_amd", "csrc", "kernels")
CXX = "/opt/rocm/lib/llvm/bin/clang++"

EDGES = [0, 15, 16, 31, 32, 47, 48, 63]  # first and last lane of every 16-lane row


def lib():
    deps = [os.path.join(NATIVE, "block_scan_emu.cpp"), os.path.join(NATIVE, "emu_fibers.h")] + [
        os.path.join(KERNELS, f) for f in ("fastpath_dev.h", "expr.h", "nfa.h", "hd.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        subprocess.check_call([CXX if os.path.exists(CXX) else "g++", "-std=c++20", "-O2", "-g", "-fPIC", "-shared",
                               "-Wno-attributes", "-o", LIB, os.path.join(NATIVE, "block_scan_emu.cpp"), "-lpthread"])
    L = ctypes.CDLL(LIB)
    L.sm_block_scan_emu.restype = ctypes.c_int
    return L


def scan(nt, v, v2=None):
    """block_excl<nt> of v (then of v2 on the same lw, behind the caller's barrier), checked against the prefix sum."""
    P = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    ins = [np.ascontiguousarray(x, dtype=np.uint32) for x in ((v,) if v2 is None else (v, v2))]
    outs = [np.full(nt, 0xDEADBEEF, np.uint32) for _ in range(4)]
    rc = lib().sm_block_scan_emu(ctypes.c_int(nt), P(ins[0]), P(outs[0]), P(outs[1]),
                                 P(ins[1]) if v2 is not None else None, P(outs[2]), P(outs[3]))
    assert rc == 0
    for k, x in enumerate(ins):
        assert len(x) == nt
        incl = np.cumsum(x.astype(np.uint64)).astype(np.uint32)  # mod 2^32
        np.testing.assert_array_equal(outs[2 * k], incl - x)
        np.testing.assert_array_equal(outs[2 * k + 1], np.full(nt, incl[-1], np.uint32))  # every thread's total


NTS = [1024, 512]


@pytest.mark.parametrize("nt", NTS)
def test_zeros_and_ones(nt):
    scan(nt, np.zeros(nt, np.uint32))
    scan(nt, np.ones(nt, np.uint32))


@pytest.mark.parametrize("nt", NTS)
@pytest.mark.parametrize("wave", ["first", "last"])
@pytest.mark.parametrize("lane", EDGES)
def test_single_value_at_a_row_edge(nt, wave, lane):
    """One non-zero value: every later thread, in the row, the wave and the waves after it, sees it exactly once."""
    v = np.zeros(nt, np.uint32)
    v[(0 if wave == "first" else nt // 64 - 1) * 64 + lane] = 0x12345
    scan(nt, v)


@pytest.mark.parametrize("nt", NTS)
def test_random_values(nt):
    rng = np.random.default_rng(nt)
    for _ in range(4):
        scan(nt, rng.integers(0, 1 << 20, nt, dtype=np.uint32))


@pytest.mark.parametrize("nt", NTS)
def test_total_wraps(nt):
    """u32 adds throughout: prefixes and the total are equal mod 2^32."""
    rng = np.random.default_rng(nt + 1)
    v = rng.integers(0, 1 << 32, nt, dtype=np.uint64).astype(np.uint32)
    assert int(v.astype(np.uint64).sum()) >= 1 << 32
    scan(nt, v)
    scan(nt, np.full(nt, 0xFFFFFFFF, np.uint32))


@pytest.mark.parametrize("nt", NTS)
def test_two_scans_on_the_same_lw(nt):
    """The second scan reuses lw behind the caller's barrier and sees nothing of the first."""
    rng = np.random.default_rng(nt + 2)
    a = rng.integers(0, 1 << 20, nt, dtype=np.uint32)
    b = rng.integers(0, 1 << 20, nt, dtype=np.uint32)
    scan(nt, a, b)
    scan(nt, a, np.zeros(nt, np.uint32))
    scan(nt, np.zeros(nt, np.uint32), b)
