// Host wave emulator of the workgroup-wide exclusive scan (siddhi_amd/csrc/kernels/fastpath_dev.h: block_excl,
// wave_incl_scan): the SAME device source, compiled for the host with SM_HOST_EMU, where the DPP steps run through
// hd.h's model of row_shr / row_bcast. One workgroup of nt threads scans in[] (and then, after the caller's barrier,
// in2[] on the same lw). Test infrastructure only (tests/test_block_scan_emu.py compares with a plain prefix sum).
// main(): a stand-alone self-check of the same entry, for sanitizer builds.
#define SM_HOST_EMU 1
#include "../../siddhi_amd/csrc/kernels/fastpath_dev.h"

#include "emu_fibers.h"

namespace {
template <int NT>
void scan_body(const uint32_t* in, uint32_t* out, uint32_t* tot, const uint32_t* in2, uint32_t* out2,
               uint32_t* tot2) {
  __shared__ uint32_t lw[NT / 64];
  const int tid = threadIdx.x;
  out[tid] = sm::block_excl<NT>(in[tid], lw, &tot[tid]);
  if (in2) {
    sm::lds_barrier();  // the caller's fence of lw's reuse
    out2[tid] = sm::block_excl<NT>(in2[tid], lw, &tot2[tid]);
  }
}
}  // namespace

// nt: 512 or 1024. out / tot (and out2 / tot2 when in2 is given): nt words each; tot holds every thread's total.
// Returns 0, or -1 for another nt.
extern "C" int sm_block_scan_emu(int nt, const uint32_t* in, uint32_t* out, uint32_t* tot, const uint32_t* in2,
                                 uint32_t* out2, uint32_t* tot2) {
  if (nt == 1024) emu_launch(1, 1024, [&] { scan_body<1024>(in, out, tot, in2, out2, tot2); });
  else if (nt == 512) emu_launch(1, 512, [&] { scan_body<512>(in, out, tot, in2, out2, tot2); });
  else return -1;
  return 0;
}

#ifdef SM_BLOCK_SCAN_EMU_MAIN
// Stand-alone self-check (sanitizer builds): ones, a single value at every row and wave edge, random values and a
// wrapping total, twice on the same lw, against a plain loop.
int main() {
  int bad = 0;
  uint64_t x = 88172645463325252ull;
  auto rnd = [&] {
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    return x;
  };
  for (int nt : {512, 1024}) {
    std::vector<std::vector<uint32_t>> cases;
    cases.push_back(std::vector<uint32_t>(nt, 0u));
    cases.push_back(std::vector<uint32_t>(nt, 1u));
    for (int w : {0, nt / 64 - 1})
      for (int l : {0, 15, 16, 31, 32, 47, 48, 63}) {
        std::vector<uint32_t> v(nt, 0u);
        v[w * 64 + l] = 7u + (uint32_t)l;
        cases.push_back(v);
      }
    std::vector<uint32_t> r(nt), big(nt);
    for (int i = 0; i < nt; ++i) {
      r[i] = (uint32_t)(rnd() & 0xfffffu);
      big[i] = (uint32_t)rnd();
    }
    cases.push_back(r);
    cases.push_back(big);
    for (size_t c = 0; c < cases.size(); ++c) {
      const std::vector<uint32_t>& a = cases[c];
      const std::vector<uint32_t>& b = cases[(c + 1) % cases.size()];
      std::vector<uint32_t> out(nt), tot(nt), out2(nt), tot2(nt);
      sm_block_scan_emu(nt, a.data(), out.data(), tot.data(), b.data(), out2.data(), tot2.data());
      uint32_t sa = 0, sb = 0;
      bool ok = true;
      for (int i = 0; i < nt; ++i) {
        ok = ok && out[i] == sa && out2[i] == sb;
        sa += a[i];
        sb += b[i];
      }
      for (int i = 0; i < nt; ++i) ok = ok && tot[i] == sa && tot2[i] == sb;
      if (!ok) {
        fprintf(stderr, "block_scan_emu: mismatch at nt=%d case=%zu\n", nt, c);
        ++bad;
      }
    }
  }
  if (!bad) printf("block_scan_emu self-check ok\n");
  return bad ? 1 : 0;
}
#endif
