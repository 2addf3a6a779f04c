// Host wave emulator of the closed form of the k-state pattern over several streams (siddhi_amd/csrc/kernels/
// mpatk_dev.h: the link, candidate, partial, emit, key and tuple kernels, behind mseq_dev.h's facts, pack and stream
// kernels and seq_dev.h's count kernel): the SAME device source, compiled for the host with SM_HOST_EMU (hd.h), driven
// by the plan the product's compiler makes of a query text over streams of the schema
//     (symbol int, price double, volume long, timestamp long)
// (compiler.cpp fast_pat_k: the streams, programs, withins, per-stream key columns). What the product's host entry does
// around the kernels (seqpath.hip fast_pat_k) is restated plainly here: the exclusive scans, a stable sort of the packed
// rows by key and the stable sorts of the compacted tuples by e2, ..., ek. Test infrastructure only
// (tests/test_mpatk_emu.py compares the tuples, the partials that stay and the events they hold with a numpy statement
// of the rule). main(): a stand-alone self-check of the same entry, for sanitizer builds.
#define SM_HOST_EMU 1
#include "../../siddhi_amd/csrc/kernels/mpatk_dev.h"

#include "emu_fibers.h"

#include <algorithm>
#include <numeric>

#include "../../siddhi_amd/csrc/compiler.h"

extern "C" int sm_mpatk_budget() { return sm::kMPatBudget; }

// sid: the app stream of every row (-1: a heartbeat). evt: ne carried events of 8 words [key, global ordinal, ts, symbol,
// price bits, volume, timestamp, stream], sorted by (key, ordinal). parts: ncp carried partials of k + 1 words
// [key, s, o1 .. o(k-1)]. tuples: room for k (n + ncp) words; parts_out: room for (k + 1) (n + ncp) words; cand: room for
// 4 (n + ne) words. marks[6]: the plan's fast_pat_k, fast_pat_ms, fast_every_within, fast_seq_adjacent, fast_seq_k,
// fast_seq_ms. facts[9] as sm_mpat_emu's. Returns the number of tuples, or -1 (err says why).
extern "C" int64_t sm_mpatk_emu(const char* text, int64_t n, const int32_t* sid, const int32_t* sym, const double* price,
                                const int64_t* vol, const int64_t* tcol, const int64_t* ts, const int64_t* ordinals,
                                int64_t obase, const int64_t* evt, int64_t ne, const int64_t* parts, int64_t ncp,
                                uint32_t* tuples, int64_t* parts_out, int64_t* nparts, int64_t* cand, int64_t* ncand,
                                int32_t* marks, int64_t* facts, char* err, size_t errlen) {
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
  marks[0] = cq.fast_pat_k;
  marks[1] = cq.fast_pat_ms ? 1 : 0;
  marks[2] = cq.fast_every_within ? 1 : 0;
  marks[3] = cq.fast_seq_adjacent ? 1 : 0;
  marks[4] = cq.fast_seq_k;
  marks[5] = cq.fast_seq_ms;
  *ncand = *nparts = 0;
  if (!cq.fast_pat_k) {
    snprintf(err, errlen, "not marked for the closed form of the k-state pattern over several streams");
    return -1;
  }
  const int k = cq.fast_pat_k, pw = k + 1;
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
  const int cw = 8;

  MSeqSrc src{};
  src.n = n;
  src.sid = sid;
  for (int m = 0; m < k; ++m) {
    const int s = cq.fast_patk_stream[m];
    src.read |= 1ull << s;
    if (keyed) {
      const int c = cq.fast_patk_keycol.at(s);
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
  if (np == 0) return 0;  // the carried partials wait
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

  const int64_t total = ncp + n;
  const int64_t rtiles = (total + kSeqTile - 1) / kSeqTile;
  // every row has a lane or is filled below: garbage, as on the device
  std::vector<int32_t> res(total + 4, 12345), kept(total + 4, 12345), mid((size_t)total * (k - 1) + 4, 0x5A5A5A5A);
  if (np < n) {
    std::fill(res.begin() + ncp, res.begin() + ncp + n, kSeqNone);
    std::fill(kept.begin() + ncp, kept.begin() + ncp + n, kSeqNone);
  }
  std::vector<uint8_t> eflag(ne + n + 1, 0);
  std::vector<uint32_t> counts(rtiles + 1, 0), kcounts(rtiles + 1, 0);
  MPatKArgs a{};
  a.np = np;
  a.n = n;
  a.ts = ts;
  a.st = &st;
  a.code = (const Instr*)(cq.blob.data() + cq.hdr.off_code);
  a.consts = (const DVal*)(cq.blob.data() + cq.hdr.off_const);
  a.k = k;
  for (int m = 0; m < kSeqKMax; ++m) {
    a.off[m] = m < k ? cq.fast_patk_off[m] : 0;
    a.len[m] = m < k ? cq.fast_patk_len[m] : 0;
    a.within[m] = m > 0 && m < k ? cq.fast_patk_within[m] : 0;
    a.want[m] = m < k ? cq.fast_patk_stream[m] : -2;
  }
  a.ts_last = facts[6];
  a.ordinals = ordinals;
  a.obase = obase;
  a.perm = packed ? perm.data() : nullptr;
  a.skey = keyed ? skey.data() : nullptr;
  a.kmin = kmin;
  a.kmax = kmax;
  a.sstr = packed ? sstr.data() : nullptr;
  a.sid = sid;
  a.evt = evt;
  a.ne = ne;
  a.cw = cw;
  a.parts = parts;
  a.ncp = ncp;
  a.res = res.data();
  a.kept = kept.data();
  a.mid = mid.data();
  a.eflag = eflag.data();
  emu_launch((int)((ncp + np + kSeqTile - 1) / kSeqTile), kSeqBlock, [&] { mpatk_link_kernel<uint32_t>(a); });
  if (eflag[ne + n] != 0) {
    snprintf(err, errlen, "link wrote past the last event flag");
    return -1;
  }
  res.resize(total);
  kept.resize(total);
  emu_launch((int)rtiles, kSeqBlock, [&] { seq_count_kernel(res.data(), total, counts.data()); });
  emu_launch((int)rtiles, kSeqBlock, [&] { seq_count_kernel(kept.data(), total, kcounts.data()); });
  uint32_t krun = 0;
  run = 0;
  for (int64_t t = 0; t < rtiles; ++t) {
    const uint32_t c = counts[t], kc = kcounts[t];
    counts[t] = run;
    kcounts[t] = krun;
    run += c;
    krun += kc;
  }
  const int64_t m = run, pk = krun;
  uint32_t cand_n = 0;
  MPatKCand ca{};
  ca.s = src;
  ca.evt = evt;
  ca.ne = ne;
  ca.cw = cw;
  ca.eflag = eflag.data();
  ca.cand = cand;
  ca.cand_n = &cand_n;
  emu_launch((int)((ne + n + kSeqBlock - 1) / kSeqBlock), kSeqBlock, [&] { mpatk_cand_kernel(ca); });
  *ncand = cand_n;

  MPatKOut oa{};
  oa.s = src;
  oa.total = total;
  oa.ncp = ncp;
  oa.mid = mid.data();
  oa.k = k;
  oa.evt = evt;
  oa.cw = cw;
  oa.parts = parts;
  std::vector<uint32_t> tup((size_t)m * k + 1, 0xDEADBEEFu);
  oa.flags = res.data();
  oa.offsets = counts.data();
  oa.tuples = tup.data();
  emu_launch((int)rtiles, kSeqBlock, [&] { mpatk_emit_kernel(oa); });
  if (tup[(size_t)m * k] != 0xDEADBEEFu) {
    snprintf(err, errlen, "emit wrote past its last tuple");
    return -1;
  }
  std::vector<int64_t> pout((size_t)pk * pw + 1, 0x7EADBEEF);
  oa.flags = kept.data();
  oa.offsets = kcounts.data();
  oa.parts_out = pout.data();
  emu_launch((int)rtiles, kSeqBlock, [&] { mpatk_parts_kernel(oa); });
  if (pout[(size_t)pk * pw] != 0x7EADBEEF) {
    snprintf(err, errlen, "parts wrote past the last partial");
    return -1;
  }
  std::copy(pout.begin(), pout.begin() + (size_t)pk * pw, parts_out);
  *nparts = pk;

  if (m > 0) {
    std::vector<uint32_t> idx(m), idx2(m), key(m);
    const int mg = (int)((m + kSeqBlock - 1) / kSeqBlock);
    for (int slot = 1; slot < k; ++slot) {
      const bool flip = slot < k - 1 && ne > 0;
      emu_launch(mg, kSeqBlock, [&] {
        mpatk_keys_kernel(tup.data(), k, slot, slot == 1 ? nullptr : idx.data(), m, flip ? 0x80000000u : 0u, key.data(),
                          idx.data());
      });
      std::vector<uint32_t> o(m);
      std::iota(o.begin(), o.end(), 0u);
      std::stable_sort(o.begin(), o.end(), [&](uint32_t x, uint32_t y) { return key[x] < key[y]; });
      for (int64_t x = 0; x < m; ++x) idx2[x] = idx[o[x]];
      idx.swap(idx2);
    }
    emu_launch(mg, kSeqBlock, [&] { mpatk_tuples_kernel(tup.data(), k, idx.data(), m, tuples); });
  }
  return m;
}

#ifdef SM_MPATK_EMU_MAIN
// Stand-alone self-check (sanitizer builds): `every e1=A[price>20] -> e2=B[price>e1.price] within 6 ms -> e3=A[price>
// e2.price] within 6 ms` over three streams with heartbeat rows, keyed (the key of B rows is their volume) and unkeyed,
// in two batches (the second takes the first one's partials and events), against a plain loop that keeps every
// instance's open partials.
#include <array>
#include <map>
#include <tuple>
int main() {
  int bad = 0;
  const std::string defs =
      "define stream A (symbol int, price double, volume long, timestamp long); "
      "define stream B (symbol int, price double, volume long, timestamp long); "
      "define stream C (symbol int, price double, volume long, timestamp long); ";
  const std::string q = "@info(name='q') from every e1=A[price>20] -> e2=B[price>e1.price] within 6 milliseconds -> "
                        "e3=A[price>e2.price] within 6 milliseconds select e1.timestamp as i insert into Out;";
  const int64_t T = 6;
  for (int keyed = 0; keyed < 2; ++keyed)
    for (int64_t n : {2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 3100}) {
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
        sid[i] = r < 4 ? 0 : r < 8 ? 1 : r < 9 ? 2 : -1;  // C is not read; -1: a heartbeat
        sym[i] = (int32_t)(rnd() % K) - 3;
        price[i] = (double)(rnd() % 600) / 10.0;
        vol[i] = (int64_t)(rnd() % K) - 3;
        tcol[i] = i;
        ts[i] = 10 + i / 8;
      }
      // the reference: every instance's open partials, in order of e1
      struct P {
        int s;
        int64_t o[2], t;
        double p;
      };
      std::map<int64_t, std::vector<P>> open;
      std::vector<std::array<int64_t, 3>> exp;
      for (int64_t j = 0; j < n; ++j) {
        if (sid[j] != 0 && sid[j] != 1) continue;
        auto& d = open[keyed ? (sid[j] == 0 ? (int64_t)sym[j] : vol[j]) : 0];
        std::vector<P> keep;
        for (const P& e : d) {
          const bool mine = (e.s == 1 && sid[j] == 1) || (e.s == 2 && sid[j] == 0);
          if (!mine) {
            keep.push_back(e);
            continue;
          }
          if (ts[j] - e.t > T) continue;  // expired
          if (!(price[j] > e.p)) {
            keep.push_back(e);
            continue;
          }
          if (e.s == 2) exp.push_back({e.o[0], e.o[1], j});
          else keep.push_back(P{2, {e.o[0], j}, ts[j], price[j]});
        }
        d.swap(keep);
        if (sid[j] == 0 && price[j] > 20.0) d.push_back(P{1, {j, 0}, ts[j], price[j]});
      }
      std::sort(exp.begin(), exp.end(), [](auto& a, auto& b) {
        return std::make_tuple(a[2], a[1], a[0]) < std::make_tuple(b[2], b[1], b[0]);
      });
      // the emulated entry, in two batches
      const int64_t cut = n / 2;
      std::vector<std::array<int64_t, 3>> got;
      std::vector<int64_t> evt, parts;
      int64_t ne = 0, ncp = 0;
      char err[256] = "";
      for (int part = 0; part < 2 && !bad; ++part) {
        const int64_t lo = part ? cut : 0, hi = part ? n : cut, nn = hi - lo;
        if (nn == 0) continue;
        std::vector<uint32_t> tuples(3 * (nn + ncp) + 4);
        std::vector<int64_t> pout(4 * (nn + ncp) + 4), cand(4 * (nn + ne) + 4);
        int64_t ncand = 0, np2 = 0, facts[9];
        int32_t marks[6] = {0, 0, 0, 0, 0, 0};
        const int64_t m = sm_mpatk_emu(text.c_str(), nn, sid.data() + lo, sym.data() + lo, price.data() + lo,
                                       vol.data() + lo, tcol.data() + lo, ts.data() + lo, nullptr, lo, evt.data(), ne,
                                       parts.data(), ncp, tuples.data(), pout.data(), &np2, cand.data(), &ncand, marks,
                                       facts, err, sizeof(err));
        if (m < 0 || marks[0] != 3) {
          fprintf(stderr, "mpatk_emu: n=%lld keyed=%d: %s\n", (long long)n, keyed, err);
          ++bad;
          break;
        }
        if (facts[0] == 0) continue;
        for (int64_t t = 0; t < m; ++t)
          got.push_back({lo + (int32_t)tuples[3 * t], lo + (int32_t)tuples[3 * t + 1], lo + (int32_t)tuples[3 * t + 2]});
        // the new carry: the candidates' rows sorted by (key, ordinal)
        std::vector<std::array<int64_t, 8>> rows;
        for (int64_t c = 0; c < ncand; ++c) {
          const int64_t* cc = cand.data() + 4 * c;
          std::array<int64_t, 8> r;
          if (cc[3] < 0) {
            std::copy(evt.begin() + (-cc[3] - 1) * 8, evt.begin() + (-cc[3] - 1) * 8 + 8, r.begin());
          } else {
            const int64_t j = lo + cc[3];
            int64_t bits;
            memcpy(&bits, &price[j], 8);
            r = {cc[0], cc[1], cc[2], sym[j], bits, vol[j], tcol[j], sid[j]};
          }
          rows.push_back(r);
        }
        std::sort(rows.begin(), rows.end(), [](auto& a, auto& b) { return std::make_pair(a[0], a[1]) < std::make_pair(b[0], b[1]); });
        evt.clear();
        for (auto& r : rows) evt.insert(evt.end(), r.begin(), r.end());
        ne = (int64_t)rows.size();
        parts.assign(pout.begin(), pout.begin() + 4 * np2);
        ncp = np2;
      }
      if (got != exp) {
        fprintf(stderr, "mpatk_emu: mismatch at n=%lld keyed=%d (got=%zu exp=%zu) %s\n", (long long)n, keyed, got.size(),
                exp.size(), err);
        ++bad;
      }
    }
  if (!bad) printf("mpatk_emu self-check ok\n");
  return bad ? 1 : 0;
}
#endif
