// Host wave emulator of the closed form of the pattern over two streams (siddhi_amd/csrc/kernels/mpat_dev.h:
// mpat_link_kernel, mpat_emit_kernel, mpat_pairs_kernel, behind mseq_dev.h's facts, pack and stream kernels and
// seq_dev.h's count kernel): the SAME device source, compiled for the host with SM_HOST_EMU (hd.h), driven by the plan
// the product's compiler makes of a query text over streams of the schema
//     (symbol int, price double, volume long, timestamp long)
// (compiler.cpp fast_pat_ms: the two streams, programs, the within, per-stream key columns). What the product's host
// entry does around the kernels (seqpath.hip fast_pat_ms) is restated plainly here: the exclusive scans, a stable sort
// of the packed rows by key and a stable sort of the compacted pairs by e2. Test infrastructure only
// (tests/test_mpat_emu.py compares the pairs and the carry-out candidates with a numpy statement of the rule). main(): a
// stand-alone self-check of the same entry, for sanitizer builds.
#define SM_HOST_EMU 1
#include "../../siddhi_amd/csrc/kernels/mpat_dev.h"

#include "emu_fibers.h"

#include <algorithm>
#include <numeric>

#include "../../siddhi_amd/csrc/compiler.h"

extern "C" int sm_mpat_budget() { return sm::kMPatBudget; }

// sid: the app stream of every row (-1: a heartbeat). carry: nc rows of 7 words [key, global ordinal, ts, symbol, price
// bits, volume, timestamp], sorted by (key, ordinal). pairs: room for 2 (n + nc) words; cand: room for 4 (n + nc) words.
// marks[5]: the plan's fast_pat_ms, fast_every_within, fast_seq_adjacent, fast_seq_k, fast_seq_ms. facts[9]: read rows,
// decreasing time, bad ordinals, key min / max, first / last event time, first / last relative ordinal (of the read
// rows). Returns the number of pairs, or -1 (err says why: the text does not parse, or the compiler does not mark it).
extern "C" int64_t sm_mpat_emu(const char* text, int64_t n, const int32_t* sid, const int32_t* sym, const double* price,
                               const int64_t* vol, const int64_t* tcol, const int64_t* ts, const int64_t* ordinals,
                               int64_t obase, const int64_t* carry, int64_t nc, uint32_t* pairs, int64_t* cand,
                               int64_t* ncand, int32_t* marks, int64_t* facts, char* err, size_t errlen) {
  using namespace sm;
  CompiledQuery cq;
  bool keyed = false;
  try {
    sql::App app = sql::parse_app(text);
    Dict dict;
    auto [pi, qi] = app.order.at(0);
    const sql::Query& qd = pi < 0 ? app.queries[qi] : app.partitions[pi].queries[qi];
    cq = compile_query(app, qd, 0, pi, dict);
    keyed = pi >= 0;
  } catch (const std::exception& e) {
    snprintf(err, errlen, "%s", e.what());
    return -1;
  }
  marks[0] = cq.fast_pat_ms ? 1 : 0;
  marks[1] = cq.fast_every_within ? 1 : 0;
  marks[2] = cq.fast_seq_adjacent ? 1 : 0;
  marks[3] = cq.fast_seq_k;
  marks[4] = cq.fast_seq_ms;
  if (!cq.fast_pat_ms) {
    snprintf(err, errlen, "not marked for the closed form of the pattern over two streams");
    return -1;
  }
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
  const int cw = 7;

  MSeqSrc src{};
  src.n = n;
  src.sid = sid;
  for (int m = 0; m < 2; ++m) {
    const int s = cq.fast_pat_stream[m];
    src.read |= 1ull << s;
    if (keyed) {
      const int c = cq.fast_pat_keycol.at(s);
      src.kcol[s] = st.cols[c];
      if (st.types[c] == T_LONG) src.wide |= 1ull << s;
    }
  }
  src.ts = ts;
  src.ordinals = ordinals;
  src.obase = obase;

  const int64_t ntiles = (n + kSeqTile - 1) / kSeqTile;
  std::vector<uint32_t> tile_n(ntiles + 1, 0xDEADu);
  MSeqFacts f;
  memset(&f, 0, sizeof(f));
  if (n > 0) emu_launch((int)std::min<int64_t>(ntiles, 3), kSeqBlock, [&] { mseq_facts_kernel(src, ntiles, tile_n.data(), &f); });
  constexpr uint64_t kBias = 0x8000000000000000ull;
  const int64_t np = (int64_t)f.nread;
  facts[0] = np;
  facts[1] = f.bad_ts;
  facts[2] = f.bad_ord;
  facts[3] = (int64_t)(~f.kmin_c ^ kBias);
  facts[4] = (int64_t)(f.kmax ^ kBias);
  facts[5] = (int64_t)(~f.tmin_c ^ kBias);
  facts[6] = (int64_t)(f.tmax ^ kBias);
  facts[7] = (int64_t)(~f.omin_c ^ kBias);
  facts[8] = (int64_t)(f.omax ^ kBias);
  *ncand = 0;
  if (np == 0) return 0;  // the carried rows wait
  const int64_t kmin = keyed ? facts[3] : 0, kmax = keyed ? facts[4] : 0;

  // the read rows in row order, then (keyed) in (key, arrival) order
  uint32_t run = 0;
  for (int64_t t = 0; t < ntiles; ++t) {
    const uint32_t c = tile_n[t];
    tile_n[t] = run;
    run += c;
  }
  const bool packed = keyed || np < n;
  std::vector<uint32_t> prow(np + 1, 0xDEADBEEFu), pkey(np + 1, 0xDEADBEEFu), perm, skey;
  std::vector<uint8_t> pstr(np + 1, 0xEE), sstr(np + 1, 0xEE);
  if (packed) {
    MSeqPack pa{};
    pa.s = src;
    pa.tile_off = tile_n.data();
    pa.kmin = kmin;
    pa.pkey = keyed ? pkey.data() : nullptr;
    pa.prow = prow.data();
    pa.pstr = keyed ? nullptr : pstr.data();
    emu_launch((int)ntiles, kSeqBlock, [&] { mseq_pack_kernel<uint32_t>(pa); });
    if (keyed) {
      std::vector<uint32_t> o(np);
      std::iota(o.begin(), o.end(), 0u);
      std::stable_sort(o.begin(), o.end(), [&](uint32_t x, uint32_t y) { return pkey[x] < pkey[y]; });
      perm.resize(np);
      skey.resize(np);
      for (int64_t u = 0; u < np; ++u) {
        perm[u] = prow[o[u]];
        skey[u] = pkey[o[u]];
      }
      emu_launch((int)((np + kSeqBlock - 1) / kSeqBlock), kSeqBlock,
                 [&] { mseq_streams_kernel(perm.data(), sid, np, sstr.data()); });
    } else {
      perm.assign(prow.begin(), prow.begin() + np);
      sstr = pstr;
    }
  }

  const int64_t total = nc + n;
  const int64_t rtiles = (total + kSeqTile - 1) / kSeqTile;
  std::vector<int32_t> res(total + 4, 12345);  // every row has a lane or is filled below: garbage, as on the device
  if (np < n) std::fill(res.begin() + nc, res.begin() + nc + n, kSeqNone);
  std::vector<uint32_t> counts(rtiles + 1, 0);
  uint32_t cand_n = 0;
  MPatArgs a{};
  a.np = np;
  a.n = n;
  a.ts = ts;
  a.st = &st;
  a.code = (const Instr*)(cq.blob.data() + cq.hdr.off_code);
  a.consts = (const DVal*)(cq.blob.data() + cq.hdr.off_const);
  a.c1_off = cq.fast_pat_off[0];
  a.c1_len = cq.fast_pat_len[0];
  a.c2_off = cq.fast_pat_off[1];
  a.c2_len = cq.fast_pat_len[1];
  a.within = cq.fast_pat_within;
  a.ts_last = facts[6];
  a.ordinals = ordinals;
  a.obase = obase;
  a.perm = packed ? perm.data() : nullptr;
  a.skey = keyed ? skey.data() : nullptr;
  a.kmin = kmin;
  a.kmax = kmax;
  a.sstr = packed ? sstr.data() : nullptr;
  a.sid = sid;
  a.sa = cq.fast_pat_stream[0];
  a.sb = cq.fast_pat_stream[1];
  a.carry = carry;
  a.nc = nc;
  a.cw = cw;
  a.res = res.data();
  a.cand = cand;
  a.cand_n = &cand_n;
  emu_launch((int)((nc + np + kSeqTile - 1) / kSeqTile), kSeqBlock, [&] { mpat_link_kernel<uint32_t>(a); });
  res.resize(total);
  emu_launch((int)rtiles, kSeqBlock, [&] { seq_count_kernel(res.data(), total, counts.data()); });
  run = 0;
  for (int64_t t = 0; t < rtiles; ++t) {
    const uint32_t c = counts[t];
    counts[t] = run;
    run += c;
  }
  const int64_t m = run;
  *ncand = cand_n;
  std::vector<uint32_t> jk(m + 1, 0xDEADBEEFu), iv(m + 1, 0xDEADBEEFu);
  emu_launch((int)rtiles, kSeqBlock, [&] {
    mpat_emit_kernel(res.data(), total, nc, counts.data(), ordinals, obase, carry, cw, jk.data(), iv.data());
  });
  if (jk[m] != 0xDEADBEEFu || iv[m] != 0xDEADBEEFu) {
    snprintf(err, errlen, "emit wrote past its last pair");
    return -1;
  }
  std::vector<uint32_t> o(m), sj(m), si(m);
  std::iota(o.begin(), o.end(), 0u);
  std::stable_sort(o.begin(), o.end(), [&](uint32_t x, uint32_t y) { return jk[x] < jk[y]; });
  for (int64_t x = 0; x < m; ++x) {
    sj[x] = jk[o[x]];
    si[x] = iv[o[x]];
  }
  if (m > 0)
    emu_launch((int)((m + kSeqBlock - 1) / kSeqBlock), kSeqBlock, [&] { mpat_pairs_kernel(sj.data(), si.data(), m, pairs); });
  return m;
}

#ifdef SM_MPAT_EMU_MAIN
// Stand-alone self-check (sanitizer builds): `every e1=A[price>20] -> e2=B[price>e1.price] within 6 milliseconds` over
// three streams with heartbeat rows, keyed (the key of B rows is their volume) and unkeyed, with carried partials,
// against a plain loop that keeps every instance's open partials.
#include <map>
int main() {
  int bad = 0;
  const std::string defs =
      "define stream A (symbol int, price double, volume long, timestamp long); "
      "define stream B (symbol int, price double, volume long, timestamp long); "
      "define stream C (symbol int, price double, volume long, timestamp long); ";
  const std::string q = "@info(name='q') from every e1=A[price>20] -> e2=B[price>e1.price] within 6 milliseconds "
                        "select e1.timestamp as i insert into Out;";
  const int64_t T = 6;
  for (int keyed = 0; keyed < 2; ++keyed)
    for (int64_t n : {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 3100}) {
      const std::string text = defs + (keyed ? "partition with (symbol of A, volume of B) begin " + q + " end;" : q);
      const int K = 7;
      std::vector<int32_t> sid(n), sym(n);
      std::vector<double> price(n);
      std::vector<int64_t> vol(n), tcol(n), ts(n);
      uint64_t x = 88172645463325252ull + (uint64_t)n * 2 + keyed;
      auto rnd = [&] {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
      };
      for (int64_t i = 0; i < n; ++i) {
        const int r = (int)(rnd() % 10);
        sid[i] = r < 5 ? 0 : r < 8 ? 1 : r < 9 ? 2 : -1;  // C is not read; -1: a heartbeat
        sym[i] = (int32_t)(rnd() % K) - 3;
        price[i] = (double)(rnd() % 600) / 10.0;
        vol[i] = (int64_t)(rnd() % K) - 3;
        tcol[i] = i;
        ts[i] = 10 + i / 8;
      }
      struct P {
        int64_t rel, t;
        double p;
      };
      std::map<int64_t, std::vector<P>> open;
      std::vector<int64_t> carry;
      const int64_t obase = 1000;
      int64_t co = obase - 500;
      for (int kk = keyed ? -3 : 0; kk < (keyed ? K - 2 : 1); ++kk)  // (key K - 3 has no events here)
        for (int r = 0; r < 3; ++r) {
          const double p = 40.0 + 6.0 * r;
          int64_t bits;
          memcpy(&bits, &p, 8);
          const int64_t t = 3 + 3 * r;  // the oldest is beyond the window of the batch's first events
          carry.insert(carry.end(), {kk, co, t, kk, bits, 100 + r, co});
          open[kk].push_back(P{co - obase, t, p});
          ++co;
        }
      const int64_t nc = (int64_t)carry.size() / 7;
      std::vector<uint32_t> pairs(2 * (n + nc) + 4);
      std::vector<int64_t> cand(4 * (n + nc) + 4);
      int64_t ncand = 0, facts[9];
      int32_t marks[5] = {0, 0, 0, 0, 0};
      char err[256] = "";
      const int64_t m = sm_mpat_emu(text.c_str(), n, sid.data(), sym.data(), price.data(), vol.data(), tcol.data(),
                                    ts.data(), nullptr, obase, carry.data(), nc, pairs.data(), cand.data(), &ncand, marks,
                                    facts, err, sizeof(err));
      std::vector<uint32_t> exp;
      int64_t nread = 0, ts_last = 0;
      for (int64_t j = 0; j < n; ++j) {
        if (sid[j] != 0 && sid[j] != 1) continue;
        ++nread;
        ts_last = ts[j];
        auto& d = open[keyed ? (sid[j] == 0 ? (int64_t)sym[j] : vol[j]) : 0];
        if (sid[j] == 0) {
          if (price[j] > 20.0) d.push_back(P{j, ts[j], price[j]});
          continue;
        }
        std::vector<P> keep;
        for (const P& e : d) {
          if (ts[j] - e.t > T) continue;  // expired
          if (price[j] > e.p) {
            exp.push_back((uint32_t)(int32_t)e.rel);
            exp.push_back((uint32_t)j);
          } else {
            keep.push_back(e);
          }
        }
        d.swap(keep);
      }
      int64_t keep = 0;
      for (auto& kv : open)
        for (const P& e : kv.second) keep += ts_last - e.t <= T;
      if (nread == 0) keep = 0;  // the entry returns before the carry is read
      if (m < 0 || marks[0] != 1 || facts[0] != nread || 2 * m != (int64_t)exp.size() ||
          !std::equal(exp.begin(), exp.end(), pairs.begin()) || ncand != keep) {
        fprintf(stderr, "mpat_emu: mismatch at n=%lld keyed=%d (m=%lld exp=%zu cand=%lld keep=%lld) %s\n", (long long)n,
                keyed, (long long)m, exp.size() / 2, (long long)ncand, (long long)keep, err);
        ++bad;
      }
    }
  if (!bad) printf("mpat_emu self-check ok\n");
  return bad ? 1 : 0;
}
#endif
