"""Key pass 0's time-order check (siddhi_amd/csrc/kernels/pass0_dev.h: pass0_kernel with a source that sets
kTimeOrder) run on the CPU under the host wave emulator (tests/native/pass0_ts_emu.cpp, a stand-alone program: the
same device source, one fiber per GPU thread, over a source with 64-bit timestamps). The flag must be raised exactly
when the 64-bit event time decreases from one event to the next, wherever the two events meet: two lanes of a
wave-item, two items of a wave, two waves, two tiles, two chunks, the ragged last tile; equal neighbouring times are
in order; a time 2^32 + 5 after the first between two small ones is not, although its low word is; a negative first
time and one near 2^40 change nothing. Every run also checks that the scatter is still the stable digit partition.
The closed form this guards assumes what the reference's `within` assumes of a stream: event time does not go back
(StreamPreStateProcessor.isExpired, core/query/input/stream/state/StreamPreStateProcessor.java:102-121).
Test infrastructure: no GPU; `-m "not gpu"`."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
KERNELS = os.path.join(HERE, "..", "siddhi_amd", "csrc", "kernels")
CXX = "/opt/rocm/lib/llvm/bin/clang++"

CASES = (["monotone", "all_equal", "monotone_ts0neg", "monotone_ts0big", "monotone_5tiles", "n1", "n100",
          "n100_decrease_last", "decrease_chunk2_first_16384", "decrease_chunk2_first_16384_G4",
          "equal_chunk2_first_16384", "wrap_2p32_at_2", "wrap_2p32_at_4097", "wrap_2p32_at_12303"] +
         [f"{kind}_{pos}" for kind in ("decrease", "equal") for pos in (
             "p1", "inside_item", "row16", "row48", "item_boundary_64", "item_boundary_192", "wave_boundary_256",
             "last_wave_3840", "tile_boundary_4096", "chunk1_first_8192", "ragged_tile_first", "ragged_tile_last")] +
         [f"{kind}_{pos}_{z}" for kind in ("decrease", "equal") for z in ("ts0neg", "ts0big") for pos in (
             "wave_boundary_256", "chunk1_first_8192", "ragged_tile_last")])


def program(sanitize):
    exe = os.path.join(NATIVE, "build", "pass0_ts_emu" + ("_san" if sanitize else ""))
    deps = [os.path.join(NATIVE, "pass0_ts_emu.cpp"), os.path.join(NATIVE, "emu_fibers.h")] + [
        os.path.join(KERNELS, f) for f in ("pass0_dev.h", "fastpath_dev.h", "expr.h", "nfa.h", "hd.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
        subprocess.check_call([CXX if os.path.exists(CXX) else "g++", "-std=c++20", "-O2", "-g", "-Wno-attributes"] +
                              (san if sanitize else []) +
                              ["-o", exe, os.path.join(NATIVE, "pass0_ts_emu.cpp"), "-lpthread"])
    return exe


def run(sanitize):
    # (the fibers switch stacks by hand: the leak checker's stack scan and the fake-stack of use-after-return
    # detection do not follow them)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:detect_stack_use_after_return=0")
    r = subprocess.run([program(sanitize)], capture_output=True, text=True, env=env)
    lines = r.stdout.splitlines()
    return r, {ln.split()[1] for ln in lines if ln.startswith("ok ")}, [ln for ln in lines if ln.startswith("FAIL")]


@pytest.fixture(scope="module")
def plain():
    return run(False)


@pytest.mark.parametrize("case", CASES)
def test_case(plain, case):
    r, ok, fails = plain
    assert case in ok, [f for f in fails if f" {case}:" in f] or r.stderr[-2000:]


def test_every_case_ran_and_passed(plain):
    r, ok, fails = plain
    assert r.returncode == 0 and not fails, (fails, r.stderr[-2000:])
    assert ok == set(CASES)


def test_sanitized_build_passes():
    """the same program under AddressSanitizer and UndefinedBehaviorSanitizer (a host build with its own main)"""
    r, ok, fails = run(True)
    assert r.returncode == 0 and not fails, (fails, r.stdout[-1000:], r.stderr[-3000:])
    assert ok == set(CASES)
