// Host wave emulator of the adjacent-pair closed form (siddhi_amd/csrc/kernels/seq_dev.h: seq_link_kernel,
// seq_keep_kernel, seq_count_kernel, seq_emit_kernel): the SAME device source, compiled for the host with SM_HOST_EMU
// (hd.h), over a two-attribute stream (symbol int, price double) with
//     c1 = price > thr (or none)      c2 = price > e1.price
// What the product's host entry does around the kernels (seqpath.hip) is restated plainly here: a stable sort of the
// rows by key and an exclusive scan of the tile counts. Test infrastructure only (tests/test_seq_emu.py compares the
// pairs, the carry-out candidates and the used marks with a numpy statement of the adjacent-pair rule). main(): a
// stand-alone self-check of the same entry, for sanitizer builds.
#define SM_HOST_EMU 1
#include "../../siddhi_amd/csrc/kernels/seq_dev.h"

#include "emu_fibers.h"

#include <algorithm>
#include <numeric>

// keys: nullptr = one instance. carry: nc rows of 5 words [key, global ordinal, ts, symbol, price bits], sorted by
// key. pairs: room for 2 n words; cand: room for 4 (n + nc) words; used: nc bytes. Returns the number of pairs.
extern "C" int64_t sm_seq_emu(int64_t n, const int32_t* keys, const double* price, const int64_t* ts,
                              const int64_t* ordinals, int64_t obase, int64_t within, int has_c1, double thr,
                              const int64_t* carry, int64_t nc, uint32_t* pairs, int64_t* cand, int64_t* ncand,
                              uint8_t* used) {
  using namespace sm;
  std::vector<int32_t> sym(n);
  for (int64_t i = 0; i < n; ++i) sym[i] = keys ? keys[i] : 0;
  NfaStream st;
  memset(&st, 0, sizeof(st));
  st.nattr = 2;
  st.types[0] = T_INT;
  st.types[1] = T_DOUBLE;
  st.cols[0] = sym.data();
  st.cols[1] = price;
  // c1: e1.price > thr ; c2: e2.price > e1.price
  Instr code[6];
  memset(code, 0, sizeof(code));
  code[0] = Instr{OP_VAR, 0, T_DOUBLE, 0, 0, 0, 0, 1};
  code[1] = Instr{OP_CONST, 0, T_DOUBLE, 0, 0, 0, 0, 0};
  code[2] = Instr{OP_CMP, CMP_GT, CT_DOUBLE, T_DOUBLE, T_DOUBLE, 0, 0, 0};
  code[3] = Instr{OP_VAR, 0, T_DOUBLE, 0, 0, 1, -1, 1};
  code[4] = Instr{OP_VAR, 0, T_DOUBLE, 0, 0, 0, 0, 1};
  code[5] = Instr{OP_CMP, CMP_GT, CT_DOUBLE, T_DOUBLE, T_DOUBLE, 0, 0, 0};
  DVal k;
  memset(&k, 0, sizeof(k));
  k.d = thr;

  std::vector<uint32_t> perm, skey;
  int64_t kmin = 0;
  if (keys && n > 0) {
    perm.resize(n);
    std::iota(perm.begin(), perm.end(), 0u);
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return keys[x] < keys[y]; });
    kmin = keys[perm[0]];
    skey.resize(n);
    for (int64_t u = 0; u < n; ++u) skey[u] = (uint32_t)((int64_t)keys[perm[u]] - kmin);
  }
  const int64_t ntiles = (n + kSeqTile - 1) / kSeqTile;
  std::vector<int32_t> e1(n + 1, 12345);
  std::vector<uint32_t> counts(ntiles + 1, 0);
  uint32_t cand_n = 0;
  for (int64_t c = 0; c < nc; ++c) used[c] = 0;
  SeqArgs a{};
  a.n = n;
  a.ts = ts;
  a.st = &st;
  a.code = code;
  a.consts = &k;
  a.c1_off = 0;
  a.c1_len = has_c1 ? 3 : 0;
  a.c2_off = 3;
  a.c2_len = 3;
  a.within = within;
  a.ordinals = ordinals;
  a.obase = obase;
  a.perm = keys ? perm.data() : nullptr;
  a.skey = keys ? skey.data() : nullptr;
  a.kmin = kmin;
  a.carry = carry;
  a.nc = nc;
  a.cw = 5;
  a.e1 = e1.data();
  a.used = used;
  a.cand = cand;
  a.cand_n = &cand_n;
  a.counts = keys ? nullptr : counts.data();
  if (n > 0) emu_launch((int)ntiles, kSeqBlock, [&] { seq_link_kernel<uint32_t>(a); });
  if (nc > 0)
    emu_launch((int)((nc + kSeqBlock - 1) / kSeqBlock), kSeqBlock,
               [&] { seq_keep_kernel(carry, nc, 5, used, cand, &cand_n); });
  if (keys && n > 0) emu_launch((int)ntiles, kSeqBlock, [&] { seq_count_kernel(e1.data(), n, counts.data()); });
  uint32_t run = 0;
  for (int64_t t = 0; t < ntiles; ++t) {
    const uint32_t c = counts[t];
    counts[t] = run;
    run += c;
  }
  if (n > 0)
    emu_launch((int)ntiles, kSeqBlock, [&] { seq_emit_kernel(e1.data(), n, counts.data(), ordinals, obase, pairs); });
  *ncand = cand_n;
  return run;
}

#ifdef SM_SEQ_EMU_MAIN
// Stand-alone self-check (sanitizer builds): keyed and unkeyed batches with a carry, against a plain loop.
#include <map>
int main() {
  int bad = 0;
  for (int keyed = 0; keyed < 2; ++keyed)
    for (int64_t n : {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 8193}) {
      const int K = 37;
      std::vector<int32_t> keys(n);
      std::vector<double> price(n);
      std::vector<int64_t> ts(n);
      uint64_t x = 88172645463325252ull + (uint64_t)n * 2 + keyed;
      auto rnd = [&] {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
      };
      for (int64_t i = 0; i < n; ++i) {
        keys[i] = keyed ? (int32_t)(rnd() % K) - 5 : 0;
        price[i] = (double)(rnd() % 1000) / 10.0;
        ts[i] = i / 3;
      }
      // carried rows for the even keys (unkeyed: key 0), ordinals before the batch
      std::vector<int64_t> carry;
      for (int kk = keyed ? -5 : 0; kk < (keyed ? K - 5 : 1); ++kk)
        if (kk % 2 == 0) {
          const double p = 30.0 + kk;
          int64_t bits;
          memcpy(&bits, &p, 8);
          carry.insert(carry.end(), {kk, 1000 - 40 + kk, -2, kk, bits});
        }
      const int64_t nc = (int64_t)carry.size() / 5, obase = 1000, within = 2;
      std::vector<uint32_t> pairs(2 * n + 2);
      std::vector<int64_t> cand(4 * (n + nc) + 4);
      std::vector<uint8_t> used(nc + 1);
      int64_t ncand = 0;
      const int64_t m = sm_seq_emu(n, keyed ? keys.data() : nullptr, price.data(), ts.data(), nullptr, obase, within, 1,
                                   20.0, carry.data(), nc, pairs.data(), cand.data(), &ncand, used.data());
      // the rule, one event at a time
      struct Last {
        bool ok;
        int64_t rel, t;
        double p;
      };
      std::map<int32_t, Last> last;
      for (int64_t c = 0; c < nc; ++c) {
        double p;
        memcpy(&p, &carry[c * 5 + 4], 8);
        last[(int32_t)carry[c * 5]] = Last{true, carry[c * 5 + 1] - obase, carry[c * 5 + 2], p};
      }
      std::vector<uint32_t> exp;
      for (int64_t j = 0; j < n; ++j) {
        auto it = last.find(keys[j]);
        if (it != last.end() && it->second.ok && ts[j] - it->second.t <= within && price[j] > it->second.p) {
          exp.push_back((uint32_t)(int32_t)it->second.rel);
          exp.push_back((uint32_t)j);
        }
        last[keys[j]] = Last{price[j] > 20.0, j, ts[j], price[j]};
      }
      int64_t keep = 0;
      for (auto& kv : last) keep += kv.second.ok;
      if (m * 2 != (int64_t)exp.size() || !std::equal(exp.begin(), exp.end(), pairs.begin()) || ncand != keep) {
        fprintf(stderr, "seq_emu: mismatch at n=%lld keyed=%d (m=%lld exp=%zu cand=%lld keep=%lld)\n", (long long)n,
                keyed, (long long)m, exp.size() / 2, (long long)ncand, (long long)keep);
        ++bad;
      }
    }
  if (!bad) printf("seq_emu self-check ok\n");
  return bad ? 1 : 0;
}
#endif
