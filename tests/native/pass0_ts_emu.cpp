// Host wave emulator of key pass 0's time-order check (siddhi_amd/csrc/kernels/pass0_dev.h, pass0_kernel with a
// source that sets kTimeOrder): the SAME device source, compiled for the host with SM_HOST_EMU (hd.h), over a source
// that supplies 64-bit timestamps. A stand-alone program: it runs every case below, prints one line per case
// ("ok <name>" / "FAIL <name>: ...") and exits with the number of failures. Test infrastructure only
// (tests/test_pass0_ts_emu.py); also built with -fsanitize=address,undefined there.
#define SM_HOST_EMU 1
#include "../../siddhi_amd/csrc/kernels/pass0_dev.h"

#include "emu_fibers.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace {

constexpr int64_t kTile = 4096;
constexpr int kDigits = 1024;

struct TsSrcEmu {  // key and 64-bit event time per event; the record keeps {key, row, 0, low word of ts - ts0}
  const uint32_t* key;
  const int64_t* ts;
  int64_t ts0;
  uint32_t* flag;
  struct Raw {
    uint32_t k;
    int64_t t;
  };
  static constexpr bool kTimeOrder = true;
  void init() {}
  void flush() {}
  Raw load(int64_t p) const { return Raw{key[p], ts[p]}; }
  uint4 record(const Raw& r, int64_t p) const {
    return make_uint4(r.k, (uint32_t)p, 0u, (uint32_t)r.t - (uint32_t)ts0);
  }
  int64_t time_of(const Raw& r) const { return r.t; }
  int64_t time0() const { return ts0; }
  int64_t time_at(int64_t p) const { return ts[p]; }
  void time_bad() const { __atomic_fetch_or(flag, 1u, __ATOMIC_SEQ_CST); }
};

int failures = 0;

// One launch over ts (keys: a fixed pseudo-random sequence); returns the flag, and checks that the output is the
// stable partition of the records by the key's low digit.
bool run(const std::string& name, const std::vector<int64_t>& ts, int G) {
  using namespace sm;
  const int64_t n = (int64_t)ts.size();
  std::vector<uint32_t> key(n);
  uint32_t x = 12345u + (uint32_t)n;
  for (int64_t i = 0; i < n; ++i) {
    x = x * 1664525u + 1013904223u;
    key[i] = (x >> 8) % 700000u;
  }
  const int64_t per = ((n + G - 1) / G + kTile - 1) / kTile * kTile;
  // cnt[d * G + g]: records of digit d in chunks before g; dbase[d]: records of digits before d
  std::vector<uint32_t> cnt((size_t)kDigits * G, 0u), tot(kDigits, 0u), dbase(kDigits, 0u);
  for (int g = 0; g < G; ++g) {
    std::vector<uint32_t> c(kDigits, 0u);
    for (int64_t p = (int64_t)g * per; p < std::min<int64_t>(n, (int64_t)(g + 1) * per); ++p) ++c[key[p] & (kDigits - 1)];
    for (int d = 0; d < kDigits; ++d) {
      if (g + 1 < G) cnt[(size_t)d * G + g + 1] = cnt[(size_t)d * G + g] + c[d];
      tot[d] += c[d];
    }
  }
  for (int d = 1; d < kDigits; ++d) dbase[d] = dbase[d - 1] + tot[d - 1];
  std::vector<uint4> out(n, make_uint4(0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu, 0xDEADBEEFu));
  uint32_t flag = 0;
  TsSrcEmu src{key.data(), ts.data(), ts[0], &flag};
  emu_launch(G, kP0Block, [&] { pass0_kernel<TsSrcEmu>(src, out.data(), n, per, G, cnt.data(), dbase.data()); });
  std::vector<uint32_t> next(dbase);
  for (int64_t p = 0; p < n; ++p) {
    const uint4 o = out[next[key[p] & (kDigits - 1)]++];
    if (o.x != key[p] || o.y != (uint32_t)p || o.z != 0u || o.w != (uint32_t)ts[p] - (uint32_t)ts[0]) {
      printf("FAIL %s: the output is not the stable digit partition (event %lld)\n", name.c_str(), (long long)p);
      ++failures;
      break;
    }
  }
  return flag != 0;
}

void expect(const std::string& name, const std::vector<int64_t>& ts, int G, bool want) {
  const int before = failures;
  const bool got = run(name, ts, G);
  if (got != want) {
    printf("FAIL %s: flag %d, expected %d\n", name.c_str(), (int)got, (int)want);
    ++failures;
  }
  if (failures == before) printf("ok %s\n", name.c_str());
}

std::vector<int64_t> rising(int64_t n, int64_t ts0) {  // 3 apart
  std::vector<int64_t> ts(n);
  for (int64_t i = 0; i < n; ++i) ts[i] = ts0 + 3 * i;
  return ts;
}

struct Pos {
  const char* what;
  int64_t p;
};

}  // namespace

int main() {
  // n = 3 tiles + 17 over G = 3 chunks of two tiles: chunk 1 = [8192, 12305) ends in a ragged tile, chunk 2 is empty
  const int64_t n = 3 * kTile + 17;
  const int G = 3;
  const Pos pos[] = {{"p1", 1},
                     {"inside_item", 37},
                     {"row16", 16},
                     {"row48", 48},
                     {"item_boundary_64", 64},
                     {"item_boundary_192", 192},
                     {"wave_boundary_256", 256},
                     {"last_wave_3840", 3840},
                     {"tile_boundary_4096", 4096},
                     {"chunk1_first_8192", 8192},
                     {"ragged_tile_first", 3 * kTile},
                     {"ragged_tile_last", n - 1}};
  const int64_t ts0s[] = {1000, -5000000000000ll, (1ll << 40) - 7};
  const char* ts0n[] = {"", "_ts0neg", "_ts0big"};
  for (int z = 0; z < 3; ++z) {
    expect(std::string("monotone") + ts0n[z], rising(n, ts0s[z]), G, false);
    for (const Pos& q : pos) {
      if (z > 0 && q.p != 256 && q.p != 8192 && q.p != n - 1) continue;  // other ts0: one position of each kind
      std::vector<int64_t> ts = rising(n, ts0s[z]);
      ts[q.p] = ts[q.p - 1] - 1;  // the one decrease; the events after it are later than both
      expect(std::string("decrease_") + q.what + ts0n[z], ts, G, true);
      ts[q.p] = ts[q.p - 1];
      expect(std::string("equal_") + q.what + ts0n[z], ts, G, false);
    }
  }
  {  // every event at the same time
    expect("all_equal", std::vector<int64_t>(n, 77), G, false);
  }
  // a timestamp 2^32 + 5 after the first between two small ones: monotone in the low words
  for (int64_t q : {(int64_t)2, (int64_t)4097, n - 2}) {
    std::vector<int64_t> ts(n, 1000 + 10);
    ts[0] = 1000;
    ts[1] = 1000 + 3;
    for (int64_t i = 2; i < q; ++i) ts[i] = 1000 + 4;
    ts[q] = 1000 + (1ll << 32) + 5;
    expect("wrap_2p32_at_" + std::to_string(q), ts, G, true);
  }
  // all three chunks of G = 3 hold events; first event of the last chunk, and G = 4 with an empty last chunk
  {
    const int64_t n2 = 5 * kTile + 17;
    expect("monotone_5tiles", rising(n2, -3), 3, false);
    std::vector<int64_t> ts = rising(n2, -3);
    ts[16384] = ts[16383] - 1;
    expect("decrease_chunk2_first_16384", ts, 3, true);
    expect("decrease_chunk2_first_16384_G4", ts, 4, true);
    ts[16384] = ts[16383];
    expect("equal_chunk2_first_16384", ts, 3, false);
  }
  {  // one event; one short tile
    expect("n1", rising(1, 5), 1, false);
    std::vector<int64_t> ts = rising(100, 5);
    expect("n100", ts, 1, false);
    ts[99] = ts[98] - 2;
    expect("n100_decrease_last", ts, 1, true);
  }
  printf("%d failure(s)\n", failures);
  return failures > 255 ? 255 : failures;
}
