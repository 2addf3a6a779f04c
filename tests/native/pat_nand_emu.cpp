// Host wave emulator of the closed form of the logical absent (siddhi_amd/csrc/kernels/mpat_nand_dev.h:
// pnand_link_kernel, behind mseq_dev.h's facts, pack and stream kernels, absent_dev.h's count scan (absent_flag_kernel,
// absent_chunk_kernel, absent_next_kernel), seq_dev.h's count kernel and mpat_dev.h's emit and pairs kernels): the SAME
// device source, compiled for the host with SM_HOST_EMU (hd.h), driven by the plan the product's compiler makes of a
// query text over streams of the schema
//     (symbol int, price double, volume long, timestamp long)
// (compiler.cpp fast_pat_nand: the three streams, programs, the within, per-stream key columns). What the product's host
// entry does around the kernels (seqpath.hip fast_pat_nand) is restated plainly here: the exclusive scans, a stable sort
// of the packed rows by key and a stable sort of the compacted pairs by e3. Test infrastructure only
// (tests/test_pat_nand_emu.py compares the pairs and the carry-out candidates with a numpy statement of the rule).
// main(): a stand-alone self-check of the same entry, for sanitizer builds.
#define SM_HOST_EMU 1
#include "../../siddhi_amd/csrc/kernels/mpat_nand_dev.h"

#include "emu_fibers.h"

#include <algorithm>
#include <numeric>

#include "../../siddhi_amd/csrc/compiler.h"

extern "C" int sm_pat_nand_budget() { return sm::kMPatBudget; }

// sid: the app stream of every row (-1: a heartbeat). carry: nc rows of 7 words [key, global ordinal, ts, symbol, price
// bits, volume, timestamp], sorted by (key, ordinal). per: sorted positions per chunk of the count scan (a multiple of
// 256). pairs: room for 2 (n + nc) words; cand: room for 4 (n + nc) words. marks[8]: the plan's fast_pat_nand,
// fast_absent, fast_pat_ms, fast_every_within, fast_seq_adjacent, fast_seq_k, fast_seq_ms, fast_pat_k. facts[4]: read
// rows, decreasing time among them, the number of cancelling rows, the event time of the last read row. Returns the
// number of pairs, or -1 (err says why: the text does not parse, or the compiler does not mark it).
extern "C" int64_t sm_pat_nand_emu(const char* text, int64_t n, const int32_t* sid, const int32_t* sym,
                                   const double* price, const int64_t* vol, const int64_t* tcol, const int64_t* ts,
                                   const int64_t* ordinals, int64_t obase, const int64_t* carry, int64_t nc, int64_t per,
                                   uint32_t* pairs, int64_t* cand, int64_t* ncand, int32_t* marks, int64_t* facts,
                                   char* err, size_t errlen) {
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
  marks[0] = cq.fast_pat_nand ? 1 : 0;
  marks[1] = cq.fast_absent ? 1 : 0;
  marks[2] = cq.fast_pat_ms ? 1 : 0;
  marks[3] = cq.fast_every_within ? 1 : 0;
  marks[4] = cq.fast_seq_adjacent ? 1 : 0;
  marks[5] = cq.fast_seq_k;
  marks[6] = cq.fast_seq_ms;
  marks[7] = cq.fast_pat_k;
  *ncand = 0;
  if (!cq.fast_pat_nand) {
    snprintf(err, errlen, "not marked for the closed form of the logical absent");
    return -1;
  }
  if (cq.match_arity() != 2 || cq.hdr.nrefs != cq.hdr.nrefs_vis + 2) {
    snprintf(err, errlen, "the plan does not carry two hidden refs");
    return -1;
  }
  if (n == 0) return 0;
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
  for (int m = 0; m < 3; ++m) {
    const int s = cq.fast_nand_stream[m];
    src.read |= 1ull << s;
    if (keyed) {
      const int c = cq.fast_nand_keycol.at(s);
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
  emu_launch((int)std::min<int64_t>(ntiles, 3), kSeqBlock, [&] { mseq_facts_kernel(src, ntiles, tile_n.data(), &f); });
  constexpr uint64_t kBias = 0x8000000000000000ull;
  const int64_t np = (int64_t)f.nread;
  facts[0] = np;
  facts[1] = f.bad_ts;
  facts[2] = 0;
  facts[3] = (int64_t)(f.tmax ^ kBias);
  if (np == 0) return 0;  // the carried rows wait
  const int64_t kmin = keyed ? (int64_t)(~f.kmin_c ^ kBias) : 0, kmax = keyed ? (int64_t)(f.kmax ^ kBias) : 0;

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

  // the count scan: every sorted position's next cancelling row
  const int nchunks = (int)((np + per - 1) / per);
  std::vector<uint8_t> fl(np + 1, 0xEE);
  std::vector<uint32_t> ccnt(nchunks + 2, 0xDEADu), rk(n + 1, 0xDEADBEEFu), F(np + 1, 0xDEADBEEFu);
  AbsArgs aa{};
  aa.np = np;
  aa.n = n;
  aa.ts = ts;
  aa.st = &st;
  aa.code = (const Instr*)(cq.blob.data() + cq.hdr.off_code);
  aa.consts = (const DVal*)(cq.blob.data() + cq.hdr.off_const);
  aa.c2_off = cq.fast_nand_off[1];
  aa.c2_len = cq.fast_nand_len[1];
  aa.perm = packed ? perm.data() : nullptr;
  aa.skey = keyed ? skey.data() : nullptr;
  aa.sstr = packed ? sstr.data() : nullptr;
  aa.sid = sid;
  aa.sb = cq.fast_nand_stream[1];
  aa.per = per;
  aa.nchunks = nchunks;
  aa.fl = fl.data();
  aa.ccnt = ccnt.data();
  aa.rk = rk.data();
  aa.F = F.data();
  emu_launch(nchunks, kSeqBlock, [&] { absent_flag_kernel(aa); });
  emu_launch(1, kSeqBlock, [&] { absent_chunk_kernel(ccnt.data(), nchunks); });
  emu_launch(nchunks, kSeqBlock, [&] { absent_next_kernel(aa); });
  facts[2] = ccnt[nchunks];
  if (fl[np] != 0xEE || ccnt[nchunks + 1] != 0xDEADu || F[ccnt[nchunks]] != 0xDEADBEEFu) {
    snprintf(err, errlen, "the count scan wrote past its arrays");
    return -1;
  }

  const int64_t total = nc + n;
  const int64_t rtiles = (total + kSeqTile - 1) / kSeqTile;
  std::vector<int32_t> res(total + 4, 12345);  // every row has a lane or is filled below: garbage, as on the device
  if (np < n) std::fill(res.begin() + nc, res.begin() + nc + n, kSeqNone);
  std::vector<uint32_t> counts(rtiles + 1, 0);
  uint32_t cand_n = 0;
  PNandArgs pa{};
  MPatArgs& a = pa.m;
  a.np = np;
  a.n = n;
  a.ts = ts;
  a.st = &st;
  a.code = aa.code;
  a.consts = aa.consts;
  a.c1_off = cq.fast_nand_off[0];
  a.c1_len = cq.fast_nand_len[0];
  a.c2_off = cq.fast_nand_off[2];
  a.c2_len = cq.fast_nand_len[2];
  a.within = cq.fast_nand_within;
  a.ts_last = facts[3];
  a.ordinals = ordinals;
  a.obase = obase;
  a.perm = aa.perm;
  a.skey = aa.skey;
  a.kmin = kmin;
  a.kmax = kmax;
  a.sstr = aa.sstr;
  a.sid = sid;
  a.sa = cq.fast_nand_stream[0];
  a.sb = cq.fast_nand_stream[2];
  a.carry = carry;
  a.nc = nc;
  a.cw = cw;
  a.res = res.data();
  a.cand = cand;
  a.cand_n = &cand_n;
  pa.fl = fl.data();
  pa.rk = rk.data();
  pa.F = F.data();
  pa.nf = ccnt.data() + nchunks;
  emu_launch((int)((nc + np + kSeqTile - 1) / kSeqTile), kSeqBlock, [&] { pnand_link_kernel<uint32_t>(pa); });
  if (res[total] != 12345) {
    snprintf(err, errlen, "the link kernel wrote past res");
    return -1;
  }
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

#ifdef SM_PAT_NAND_EMU_MAIN
// Stand-alone self-check (sanitizer builds): `every e1=A[price>20] -> not B[price>52] and e3=C[price>e1.price] within 6
// milliseconds` over three streams with heartbeat rows, keyed (the key of B rows is their volume) and unkeyed, with
// carried partials, in chunks of 256 positions, against a plain loop that keeps every instance's pending partials. Then
// the shapes of tests/test_pat_nand_emu.py's bound cases: one key, the cancel bound 1 .. 200 positions past the e1, the
// first passing C row one position before the bound, one after it, and absent.
#include <map>
namespace {
struct Feed {
  std::vector<int32_t> sid, sym;
  std::vector<double> price;
  std::vector<int64_t> vol, tcol, ts;
  void row(int s, int k, double p, int64_t v, int64_t t) {
    sid.push_back(s);
    sym.push_back(k);
    price.push_back(p);
    vol.push_back(v);
    tcol.push_back((int64_t)tcol.size());
    ts.push_back(t);
  }
};

// the plain loop; B rows keyed by volume when keyed. Returns the expected pairs and the number of open partials
struct P {
  int64_t rel, t;
  double p;
  bool dead;
};
int check(const char* what, const std::string& text, const Feed& fd, bool keyed, std::vector<int64_t> carry, int64_t obase,
          std::map<int64_t, std::vector<P>> open, double c2min, int64_t T) {
  const int64_t n = (int64_t)fd.sid.size(), nc = (int64_t)carry.size() / 7;
  std::vector<uint32_t> pairs(2 * (n + nc) + 4);
  std::vector<int64_t> cand(4 * (n + nc) + 4);
  int64_t ncand = 0, facts[4];
  int32_t marks[8] = {0};
  char err[256] = "";
  const int64_t m = sm_pat_nand_emu(text.c_str(), n, fd.sid.data(), fd.sym.data(), fd.price.data(), fd.vol.data(),
                                    fd.tcol.data(), fd.ts.data(), nullptr, obase, carry.data(), nc, 256, pairs.data(),
                                    cand.data(), &ncand, marks, facts, err, sizeof(err));
  std::vector<uint32_t> exp;
  int64_t nread = 0, ts_last = 0;
  for (int64_t j = 0; j < n; ++j) {
    const int s = fd.sid[j];
    if (s < 0 || s > 2) continue;
    ++nread;
    ts_last = fd.ts[j];
    auto& d = open[keyed ? (s == 1 ? fd.vol[j] : (int64_t)fd.sym[j]) : 0];
    if (s == 0) {
      if (fd.price[j] > 20.0) d.push_back(P{j, fd.ts[j], fd.price[j], false});
    } else if (s == 1) {
      if (fd.price[j] > c2min)
        for (P& e : d) e.dead = true;
    } else {
      std::vector<P> keep;
      for (const P& e : d) {
        if (!(fd.price[j] > e.p)) {
          keep.push_back(e);
        } else if (!e.dead && fd.ts[j] - e.t <= T) {
          exp.push_back((uint32_t)(int32_t)e.rel);
          exp.push_back((uint32_t)j);
        }
      }
      d.swap(keep);
    }
  }
  int64_t keep = 0;
  for (auto& kv : open)
    for (const P& e : kv.second) keep += !e.dead && ts_last - e.t <= T;
  if (nread == 0) keep = 0;  // the entry returns before the carry is read
  if (m < 0 || marks[0] != 1 || facts[0] != nread || 2 * m != (int64_t)exp.size() ||
      !std::equal(exp.begin(), exp.end(), pairs.begin()) || ncand != keep) {
    fprintf(stderr, "pat_nand_emu: mismatch at %s (m=%lld exp=%zu cand=%lld keep=%lld) %s\n", what, (long long)m,
            exp.size() / 2, (long long)ncand, (long long)keep, err);
    return 1;
  }
  return 0;
}
}  // namespace

int main() {
  int bad = 0;
  const std::string defs =
      "@app:playback define stream A (symbol int, price double, volume long, timestamp long); "
      "define stream B (symbol int, price double, volume long, timestamp long); "
      "define stream C (symbol int, price double, volume long, timestamp long); ";
  const std::string q = "@info(name='q') from every e1=A[price>20] -> not B[price>52] and e3=C[price>e1.price] within 6 "
                        "milliseconds select e1.timestamp as i, e3.timestamp as j insert into Out;";
  const int64_t T = 6;
  for (int keyed = 0; keyed < 2; ++keyed)
    for (int64_t n : {1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 3100}) {
      const std::string text =
          defs + (keyed ? "partition with (symbol of A, volume of B, symbol of C) begin " + q + " end;" : q);
      const int K = 7;
      Feed fd;
      uint64_t x = 88172645463325252ull + (uint64_t)n * 2 + keyed;
      auto rnd = [&] {
        x ^= x << 13;
        x ^= x >> 7;
        x ^= x << 17;
        return x;
      };
      for (int64_t i = 0; i < n; ++i) {
        const int r = (int)(rnd() % 10);
        const int s = r < 4 ? 0 : r < 6 ? 1 : r < 9 ? 2 : -1;  // -1: a heartbeat
        const int k = (int)(rnd() % K) - 3;
        const double p = (double)(rnd() % 600) / 10.0;
        fd.row(s, k, p, (int64_t)(rnd() % K) - 3, 10 + i / 8);
      }
      std::map<int64_t, std::vector<P>> open;
      std::vector<int64_t> carry;
      const int64_t obase = 1000;
      int64_t co = obase - 500;
      for (int kk = keyed ? -3 : 0; kk < (keyed ? K - 2 : 1); ++kk)  // (key K - 3 has no rows here)
        for (int r = 0; r < 3; ++r) {
          const double p = 30.0 + 6.0 * r;
          int64_t bits;
          memcpy(&bits, &p, 8);
          const int64_t t = 3 + 3 * r;  // the oldest is beyond the window of the batch's first rows
          carry.insert(carry.end(), {kk, co, t, kk, bits, 100 + r, co});
          open[kk].push_back(P{co - obase, t, p, false});
          ++co;
        }
      char what[64];
      snprintf(what, sizeof(what), "n=%lld keyed=%d", (long long)n, keyed);
      bad += check(what, text, fd, keyed != 0, carry, obase, open, 52.0, T);
    }
  // one key: an e1, `gap` rows that neither cancel nor match, then the bound; the first passing C row before the bound,
  // after it, or absent; a second e1 behind the bound that the same C row completes
  for (int keyed = 0; keyed < 2; ++keyed)
    for (int gap : {0, 14, 15, 16, 62, 63, 64, 199, 300})
      for (int where = 0; where < 3; ++where) {
        const std::string text =
            defs + (keyed ? "partition with (symbol of A, volume of B, symbol of C) begin " + q + " end;" : q);
        Feed fd;
        fd.row(0, 1, 30.0, 1, 10);
        for (int g = 0; g < gap; ++g) fd.row(g % 3 == 0 ? 2 : g % 3 == 1 ? 1 : 0, 1, 10.0, 1, 10);  // no c1, c2, c3
        if (where == 0) fd.row(2, 1, 40.0, 1, 11);
        fd.row(1, 1, 60.0, 1, 11);  // the bound
        fd.row(0, 1, 25.0, 1, 11);
        if (where == 1) fd.row(2, 1, 40.0, 1, 12);
        char what[64];
        snprintf(what, sizeof(what), "gap=%d where=%d keyed=%d", gap, where, keyed);
        bad += check(what, text, fd, keyed != 0, {}, 0, {}, 52.0, T);
      }
  if (!bad) printf("pat_nand_emu self-check ok\n");
  return bad ? 1 : 0;
}
#endif
