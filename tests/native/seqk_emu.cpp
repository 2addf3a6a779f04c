// Host wave emulator of the adjacent-run closed form of k-state sequences (siddhi_amd/csrc/kernels/seq_dev.h:
// seqk_link_kernel, seqk_keep_kernel, seqk_count_kernel, seqk_emit_kernel): the SAME device source, compiled for the
// host with SM_HOST_EMU (hd.h), driven by the plan the product's compiler makes of a query text over
//     define stream StockStream (symbol int, price double, volume long, timestamp long)
// (compiler.cpp fast_seq_k and its per-element programs and withins). What the product's host entry does around the
// kernels (seqpath.hip fast_seq_k) is restated plainly here: a stable sort of the rows by key and an exclusive scan of
// the tile counts. Test infrastructure only (tests/test_seqk_emu.py compares the tuples and the carry-out candidates
// with a numpy statement of the rule). main(): a stand-alone self-check of the same entry, for sanitizer builds.
#define SM_HOST_EMU 1
#include "../../siddhi_amd/csrc/kernels/seq_dev.h"

#include "emu_fibers.h"

#include <algorithm>
#include <numeric>

#include "../../siddhi_amd/csrc/compiler.h"

// keyed = 0: one instance. carry: nc rows of 7 words [key, global ordinal, ts, symbol, price bits, volume, timestamp],
// sorted by (key, ordinal). tuples: room for k n words; cand: room for 4 (n + nc) words. Returns the number of tuples,
// or -1 (err says why: the text does not parse, or the compiler does not mark it).
extern "C" int64_t sm_seqk_emu(const char* text, int64_t n, int keyed, const int32_t* sym, const double* price,
                               const int64_t* vol, const int64_t* tcol, const int64_t* ts, const int64_t* ordinals,
                               int64_t obase, const int64_t* carry, int64_t nc, uint32_t* tuples, int64_t* cand,
                               int64_t* ncand, int32_t* k_out, char* err, size_t errlen) {
  using namespace sm;
  CompiledQuery cq;
  try {
    sql::App app = sql::parse_app(text);
    Dict dict;
    auto [pi, qi] = app.order.at(0);
    const sql::Query& qd = pi < 0 ? app.queries[qi] : app.partitions[pi].queries[qi];
    cq = compile_query(app, qd, 0, pi, dict);
  } catch (const std::exception& e) {
    snprintf(err, errlen, "%s", e.what());
    return -1;
  }
  *k_out = cq.fast_seq_k;
  if (!cq.fast_seq_k) {
    snprintf(err, errlen, "not marked for the adjacent-run closed form");
    return -1;
  }
  const int k = cq.fast_seq_k;
  NfaStream st;
  memset(&st, 0, sizeof(st));
  st.nattr = 4;
  st.types[0] = T_INT;
  st.types[1] = T_DOUBLE;
  st.types[2] = T_LONG;
  st.types[3] = T_LONG;
  st.cols[0] = sym;
  st.cols[1] = price;
  st.cols[2] = vol;
  st.cols[3] = tcol;

  std::vector<uint32_t> perm, skey;
  int64_t kmin = 0, kmax = 0;
  if (keyed && n > 0) {
    perm.resize(n);
    std::iota(perm.begin(), perm.end(), 0u);
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return sym[x] < sym[y]; });
    kmin = sym[perm[0]];
    kmax = sym[perm[n - 1]];
    skey.resize(n);
    for (int64_t u = 0; u < n; ++u) skey[u] = (uint32_t)((int64_t)sym[perm[u]] - kmin);
  }
  const int64_t ntiles = (n + kSeqTile - 1) / kSeqTile;
  std::vector<int32_t> prev(n + 1, 12345);
  std::vector<uint8_t> hit(((size_t)n + 3 & ~(size_t)3) + 4, 0xEE);  // the padding holds garbage, as on the device
  std::vector<uint32_t> counts(ntiles + 1, 0);
  uint32_t cand_n = 0;
  SeqKArgs a{};
  a.n = n;
  a.ts = ts;
  a.st = &st;
  a.code = (const Instr*)(cq.blob.data() + cq.hdr.off_code);
  a.consts = (const DVal*)(cq.blob.data() + cq.hdr.off_const);
  a.k = k;
  for (int m = 0; m < kSeqKMax; ++m) {
    a.off[m] = m < k ? cq.fast_k_off[m] : 0;
    a.len[m] = m < k ? cq.fast_k_len[m] : 0;
    a.within[m] = m < k ? cq.fast_k_within[m] : -1;
  }
  a.ordinals = ordinals;
  a.obase = obase;
  a.perm = keyed ? perm.data() : nullptr;
  a.skey = keyed ? skey.data() : nullptr;
  a.kmin = kmin;
  a.kmax = kmax;
  a.carry = carry;
  a.nc = nc;
  a.cw = 7;
  a.prev = prev.data();
  a.hit = hit.data();
  a.cand = cand;
  a.cand_n = &cand_n;
  if (n > 0) emu_launch((int)ntiles, kSeqBlock, [&] { seqk_link_kernel<uint32_t>(a); });
  if (nc > 0) emu_launch((int)((nc + kSeqBlock - 1) / kSeqBlock), kSeqBlock, [&] { seqk_keep_kernel<uint32_t>(a); });
  if (n > 0) emu_launch((int)ntiles, kSeqBlock, [&] { seqk_count_kernel(hit.data(), n, counts.data()); });
  uint32_t run = 0;
  for (int64_t t = 0; t < ntiles; ++t) {
    const uint32_t c = counts[t];
    counts[t] = run;
    run += c;
  }
  if (n > 0)
    emu_launch((int)ntiles, kSeqBlock, [&] {
      seqk_emit_kernel(hit.data(), prev.data(), n, k, counts.data(), ordinals, obase, carry, 7, tuples);
    });
  *ncand = cand_n;
  return run;
}

#ifdef SM_SEQK_EMU_MAIN
// Stand-alone self-check (sanitizer builds): k = 3 and 4, keyed and unkeyed batches with a carry, against a plain loop
// that keeps each instance's last k - 1 events.
#include <deque>
#include <map>
int main() {
  int bad = 0;
  for (int k = 3; k <= 4; ++k)
    for (int keyed = 0; keyed < 2; ++keyed)
      for (int64_t n : {1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049}) {
        std::string q = "@info(name='q') from every e1=StockStream[price>20]";
        for (int m = 2; m <= k; ++m)
          q += ", e" + std::to_string(m) + "=StockStream[price > e" + std::to_string(m - 1) +
               ".price - 25.0 and volume != e1.volume]" + (m == k ? " within 2 milliseconds" : "");
        q += " select e1.timestamp as i insert into Out;";
        std::string text = "define stream StockStream (symbol int, price double, volume long, timestamp long); ";
        text += keyed ? "partition with (symbol of StockStream) begin " + q + " end;" : q;
        const int K = 37;
        std::vector<int32_t> sym(n);
        std::vector<double> price(n);
        std::vector<int64_t> vol(n), tcol(n), ts(n);
        uint64_t x = 88172645463325252ull + (uint64_t)n * 2 + keyed + 7 * k;
        auto rnd = [&] {
          x ^= x << 13;
          x ^= x >> 7;
          x ^= x << 17;
          return x;
        };
        for (int64_t i = 0; i < n; ++i) {
          sym[i] = keyed ? (int32_t)(rnd() % K) - 5 : 0;
          price[i] = (double)(rnd() % 600) / 10.0;
          vol[i] = (int64_t)(rnd() % 50);
          tcol[i] = i;
          ts[i] = i / 3;
        }
        struct Ev {
          int64_t rel, t, v;
          double p;
        };
        std::map<int32_t, std::deque<Ev>> last;
        // carried rows: the even keys hold 1 or 2 .. k - 1 rows (unkeyed: key 0)
        std::vector<int64_t> carry;
        const int64_t obase = 1000;
        int64_t co = obase - 500;
        for (int kk = keyed ? -5 : 0; kk < (keyed ? K - 5 : 1); ++kk)
          if (kk % 2 == 0)
            for (int r = 0; r < 1 + (kk / 2 + k) % (k - 1); ++r) {
              const double p = 25.0 + kk + r;
              int64_t bits;
              memcpy(&bits, &p, 8);
              carry.insert(carry.end(), {kk, co, -1, kk, bits, 100 + r, co});
              last[kk].push_back(Ev{co - obase, -1, 100 + r, p});
              ++co;
            }
        const int64_t nc = (int64_t)carry.size() / 7;
        std::vector<uint32_t> tuples((size_t)k * n + 4);
        std::vector<int64_t> cand(4 * (n + nc) + 4);
        int64_t ncand = 0;
        int32_t kout = 0;
        char err[256] = "";
        const int64_t m = sm_seqk_emu(text.c_str(), n, keyed, sym.data(), price.data(), vol.data(), tcol.data(),
                                      ts.data(), nullptr, obase, carry.data(), nc, tuples.data(), cand.data(), &ncand,
                                      &kout, err, sizeof(err));
        std::vector<uint32_t> exp;
        for (int64_t j = 0; j < n; ++j) {
          auto& d = last[sym[j]];
          d.push_back(Ev{j, ts[j], vol[j], price[j]});
          if ((int)d.size() > k) d.pop_front();
          if ((int)d.size() == k) {
            bool ok = d[0].p > 20.0 && d[k - 1].t - d[k - 2].t <= 2;
            for (int s = 1; ok && s < k; ++s) ok = d[s].p > d[s - 1].p - 25.0 && d[s].v != d[0].v;
            if (ok)
              for (int s = 0; s < k; ++s) exp.push_back((uint32_t)(int32_t)d[s].rel);
          }
        }
        int64_t keep = 0;
        for (auto& kv : last) keep += std::min<int64_t>((int64_t)kv.second.size(), k - 1);
        if (m < 0 || kout != k || m * k != (int64_t)exp.size() || !std::equal(exp.begin(), exp.end(), tuples.begin()) ||
            ncand != keep) {
          fprintf(stderr, "seqk_emu: mismatch at k=%d n=%lld keyed=%d (m=%lld exp=%zu cand=%lld keep=%lld) %s\n", k,
                  (long long)n, keyed, (long long)m, exp.size() / k, (long long)ncand, (long long)keep, err);
          ++bad;
        }
      }
  if (!bad) printf("seqk_emu self-check ok\n");
  return bad ? 1 : 0;
}
#endif
