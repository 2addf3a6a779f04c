// Host wave emulator of the unkeyed walk's j order by output tiles (siddhi_amd/csrc/kernels/jtile_dev.h,
// jt_count_kernel and jt_place_kernel): the SAME device source, compiled for the host with SM_HOST_EMU (hd.h), driven
// as fastpath3.hip drives it: P filled with a poison word (the product takes it from an uncleared scratch arena), the
// counts cleared, the count kernel, an exclusive scan of the counts, and the place kernel unless the largest j - i is
// beyond its reach. Test infrastructure only (tests/test_jtile_emu.py: out must be the staged pairs under a stable
// sort by j).
#define SM_HOST_EMU 1
#include "../../siddhi_amd/csrc/kernels/jtile_dev.h"

#include "emu_fibers.h"

extern "C" void sm_jtile_emu_consts(int* out) {
  out[0] = (int)sm::kJtTile;
  out[1] = (int)sm::kJtCap;
  out[2] = (int)sm::kJtDMax;
  out[3] = sm::kJtThreads;
}

// stq: Gw chunks of perw slots, chunk g's mcount[g] pairs (j << 32) | i (ordinals relative to obase) in ascending i;
// ord: the events' ordinals (null: the batch positions); T: output tiles, (largest relative ordinal >> kJtB) + 1.
// Writes cnt[T + 1] (pairs per output tile), P[T + 1], *dmax (largest j - i), *err (the place kernel's error word)
// and out (the caller's sentinel stays wherever nothing is placed). Returns 1 when placement ran, 0 when the largest
// j - i is beyond the place kernel's reach and it was skipped.
extern "C" int sm_jtile_emu(const uint64_t* stq, const uint32_t* mcount, int64_t perw, int Gw, const int64_t* ord,
                            int64_t obase, int64_t n, uint32_t T, uint32_t poison, uint64_t* out, uint32_t* cnt,
                            uint32_t* P, uint32_t* dmax, uint32_t* err) {
  using namespace sm;
  for (uint32_t u = 0; u <= T; ++u) {
    P[u] = poison;
    cnt[u] = 0;
  }
  *dmax = 0;
  *err = 0;
  emu_launch(Gw, 1024, [&] { jt_count_kernel(stq, mcount, perw, Gw, ord, obase, n, T, cnt, dmax, P); });
  if (*dmax > kJtDMax) return 0;
  std::vector<uint32_t> off((size_t)T + 1);
  uint32_t run = 0;
  for (uint32_t t = 0; t <= T; ++t) {
    off[t] = run;
    run += cnt[t];
  }
  const uint32_t D = *dmax;
  emu_launch((int)T, kJtThreads, [&] { jt_place_kernel(stq, mcount, perw, P, off.data(), D, out, err); });
  return 1;
}
