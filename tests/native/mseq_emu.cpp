// Host wave emulator of the adjacent-run closed form over several streams (siddhi_amd/csrc/kernels/mseq_dev.h:
// mseq_facts_kernel, mseq_pack_kernel, mseq_streams_kernel, mseq_link_kernel, and seq_dev.h's seqk keep, count and emit
// kernels behind them): the SAME device source, compiled for the host with SM_HOST_EMU (hd.h), driven by the plan the
// product's compiler makes of a query text over streams of the schema
//     (symbol int, price double, volume long, timestamp long)
// (compiler.cpp fast_seq_ms: per-element streams, programs and withins, per-stream key columns). What the product's host
// entry does around the kernels (seqpath.hip fast_seq_ms) is restated plainly here: the exclusive scans and a stable sort
// of the packed rows by key. Test infrastructure only (tests/test_mseq_emu.py compares the tuples and the carry-out
// candidates with a numpy statement of the rule). main(): a stand-alone self-check of the same entry, for sanitizer
// builds.
#define SM_HOST_EMU 1
#include "../../siddhi_amd/csrc/kernels/mseq_dev.h"

#include "emu_fibers.h"

#include <algorithm>
#include <numeric>

#include "../../siddhi_amd/csrc/compiler.h"

// sid: the app stream of every row (-1: a heartbeat). carry: nc rows of 8 words [key, global ordinal, ts, symbol, price
// bits, volume, timestamp, stream], sorted by (key, ordinal). tuples: room for k n words; cand: room for 4 (n + nc)
// words. marks[3]: the plan's fast_seq_ms, fast_seq_k, fast_seq_adjacent. facts[9]: read rows, decreasing time,
// bad ordinals, key min / max, first / last event time, first / last relative ordinal (of the read rows). Returns the
// number of tuples, or -1 (err says why: the text does not parse, or the compiler does not mark it).
extern "C" int64_t sm_mseq_emu(const char* text, int64_t n, const int32_t* sid, const int32_t* sym, const double* price,
                               const int64_t* vol, const int64_t* tcol, const int64_t* ts, const int64_t* ordinals,
                               int64_t obase, const int64_t* carry, int64_t nc, uint32_t* tuples, int64_t* cand,
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
  marks[0] = cq.fast_seq_ms;
  marks[1] = cq.fast_seq_k;
  marks[2] = cq.fast_seq_adjacent ? 1 : 0;
  if (!cq.fast_seq_ms) {
    snprintf(err, errlen, "not marked for the closed form over several streams");
    return -1;
  }
  const int k = cq.fast_seq_ms;
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
  for (int s : cq.streams) src.read |= 1ull << s;
  if (keyed)
    for (int s : cq.streams) {
      const int c = cq.fast_ms_keycol.at(s);
      src.kcol[s] = st.cols[c];
      if (st.types[c] == T_LONG) src.wide |= 1ull << s;
    }
  src.ts = ts;
  src.ordinals = ordinals;
  src.obase = obase;

  const int64_t ntiles = (n + kSeqTile - 1) / kSeqTile;
  std::vector<uint32_t> tile_n(ntiles + 1, 0xDEADu);
  MSeqFacts f;
  memset(&f, 0, sizeof(f));
  // (3 workgroups: with more tiles than that, a workgroup walks several)
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
  if (np == 0) return 0;
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
    if (prow[np] != 0xDEADBEEFu) {
      snprintf(err, errlen, "pack wrote past its last row");
      return -1;
    }
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

  const int64_t ptiles = (np + kSeqTile - 1) / kSeqTile;
  std::vector<int32_t> prev(n + 1, 12345);
  std::vector<uint8_t> hit((((size_t)n + 3) & ~(size_t)3) + 4, 0);
  if (!packed) std::fill(hit.begin(), hit.end(), 0xEE);  // every row has a lane: garbage, as on the device
  std::vector<uint32_t> counts(ntiles + 1, 0);
  uint32_t cand_n = 0;
  MSeqArgs ma{};
  SeqKArgs& a = ma.q;
  a.n = np;
  a.ts = ts;
  a.st = &st;
  a.code = (const Instr*)(cq.blob.data() + cq.hdr.off_code);
  a.consts = (const DVal*)(cq.blob.data() + cq.hdr.off_const);
  a.k = k;
  for (int m = 0; m < kSeqKMax; ++m) {
    a.off[m] = m < k ? cq.fast_ms_off[m] : 0;
    a.len[m] = m < k ? cq.fast_ms_len[m] : 0;
    a.within[m] = m < k ? cq.fast_ms_within[m] : -1;
    ma.want[m] = m < k ? (uint8_t)cq.fast_ms_stream[m] : 0;
  }
  a.ordinals = ordinals;
  a.obase = obase;
  a.perm = packed ? perm.data() : nullptr;
  a.skey = keyed ? skey.data() : nullptr;
  a.kmin = kmin;
  a.kmax = kmax;
  a.carry = carry;
  a.nc = nc;
  a.cw = cw;
  a.prev = prev.data();
  a.hit = hit.data();
  a.cand = cand;
  a.cand_n = &cand_n;
  ma.sstr = packed ? sstr.data() : nullptr;
  ma.sid = sid;
  emu_launch((int)ptiles, kSeqBlock, [&] { mseq_link_kernel<uint32_t>(ma); });
  if (nc > 0) emu_launch((int)((nc + kSeqBlock - 1) / kSeqBlock), kSeqBlock, [&] { seqk_keep_kernel<uint32_t>(a); });
  emu_launch((int)ntiles, kSeqBlock, [&] { seqk_count_kernel(hit.data(), n, counts.data()); });
  run = 0;
  for (int64_t t = 0; t < ntiles; ++t) {
    const uint32_t c = counts[t];
    counts[t] = run;
    run += c;
  }
  emu_launch((int)ntiles, kSeqBlock, [&] {
    seqk_emit_kernel(hit.data(), prev.data(), n, k, counts.data(), ordinals, obase, carry, cw, tuples);
  });
  *ncand = cand_n;
  return run;
}

#ifdef SM_MSEQ_EMU_MAIN
// Stand-alone self-check (sanitizer builds): `A, B` and `A, B, A` over three streams with heartbeat rows, keyed (the key
// of C rows is their volume) and unkeyed, with a carry, against a plain loop that keeps each instance's last k - 1 read
// events.
#include <deque>
#include <map>
int main() {
  int bad = 0;
  const std::string defs =
      "define stream A (symbol int, price double, volume long, timestamp long); "
      "define stream B (symbol int, price double, volume long, timestamp long); "
      "define stream C (symbol int, price double, volume long, timestamp long); ";
  for (int k = 2; k <= 3; ++k)
    for (int keyed = 0; keyed < 2; ++keyed)
      for (int64_t n : {1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 3100}) {
        std::string q = "@info(name='q') from every e1=A[price>20], e2=B[price > e1.price - 25.0]";
        if (k == 3) q += ", e3=A[volume != e1.volume] within 2 milliseconds";
        q += " select e1.timestamp as i insert into Out;";
        const std::string text =
            defs + (keyed ? "partition with (symbol of A, symbol of B, volume of C) begin " + q + " end;" : q);
        const int K = 11;
        std::vector<int32_t> sid(n), sym(n);
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
          const int r = (int)(rnd() % 10);
          sid[i] = r < 4 ? 0 : r < 8 ? 1 : r < 9 ? 2 : -1;  // C is not read; -1: a heartbeat
          sym[i] = (int32_t)(rnd() % K) - 5;
          price[i] = (double)(rnd() % 600) / 10.0;
          vol[i] = (int64_t)(rnd() % 50);
          tcol[i] = i;
          ts[i] = i / 3;
        }
        struct Ev {
          int64_t rel, t, v;
          double p;
          int s;
        };
        std::map<int32_t, std::deque<Ev>> last;
        std::vector<int64_t> carry;
        const int64_t obase = 1000;
        int64_t co = obase - 500;
        for (int kk = keyed ? -5 : 0; kk < (keyed ? K - 5 : 1); ++kk)
          if (kk % 2 == 0)
            for (int r = 0; r < k - 1; ++r) {
              const double p = 25.0 + kk + r;
              int64_t bits;
              memcpy(&bits, &p, 8);
              const int s = (r + k) % 2;  // k = 2: A; k = 3: B, then A
              carry.insert(carry.end(), {kk, co, -1, kk, bits, 100 + r, co, s});
              last[kk].push_back(Ev{co - obase, -1, 100 + r, p, s});
              ++co;
            }
        const int64_t nc = (int64_t)carry.size() / 8;
        std::vector<uint32_t> tuples((size_t)k * n + 4);
        std::vector<int64_t> cand(4 * (n + nc) + 4);
        int64_t ncand = 0, facts[9];
        int32_t marks[3] = {0, 0, 0};
        char err[256] = "";
        const int64_t m = sm_mseq_emu(text.c_str(), n, sid.data(), sym.data(), price.data(), vol.data(), tcol.data(),
                                      ts.data(), nullptr, obase, carry.data(), nc, tuples.data(), cand.data(), &ncand,
                                      marks, facts, err, sizeof(err));
        std::vector<uint32_t> exp;
        int64_t nread = 0;
        const int want[3] = {0, 1, 0};
        for (int64_t j = 0; j < n; ++j) {
          if (sid[j] != 0 && sid[j] != 1) continue;
          ++nread;
          auto& d = last[keyed ? sym[j] : 0];
          d.push_back(Ev{j, ts[j], vol[j], price[j], sid[j]});
          if ((int)d.size() > k) d.pop_front();
          if ((int)d.size() == k) {
            bool ok = d[0].p > 20.0 && d[1].p > d[0].p - 25.0;
            for (int s = 0; ok && s < k; ++s) ok = d[s].s == want[s];
            if (k == 3) ok = ok && d[2].v != d[0].v && d[2].t - d[1].t <= 2;
            if (ok)
              for (int s = 0; s < k; ++s) exp.push_back((uint32_t)(int32_t)d[s].rel);
          }
        }
        int64_t keep = 0;
        for (auto& kv : last) keep += std::min<int64_t>((int64_t)kv.second.size(), k - 1);
        if (nread == 0) keep = 0;  // the entry returns before the carry is read
        if (m < 0 || marks[0] != k || facts[0] != nread || m * k != (int64_t)exp.size() ||
            !std::equal(exp.begin(), exp.end(), tuples.begin()) || ncand != keep) {
          fprintf(stderr, "mseq_emu: mismatch at k=%d n=%lld keyed=%d (m=%lld exp=%zu cand=%lld keep=%lld) %s\n", k,
                  (long long)n, keyed, (long long)m, exp.size() / k, (long long)ncand, (long long)keep, err);
          ++bad;
        }
      }
  if (!bad) printf("mseq_emu self-check ok\n");
  return bad ? 1 : 0;
}
#endif
