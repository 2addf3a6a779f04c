// Host wave emulator of the timeout closed form (siddhi_amd/csrc/kernels/absent_dev.h: the clock, flag, chunk, next,
// state, emit, instance, create and project kernels, behind mseq_dev.h's facts, pack and stream kernels and seq_dev.h's
// count kernel): the SAME device source, compiled for the host with SM_HOST_EMU (hd.h), driven by the plan the
// product's compiler makes of a query text over streams of the schema
//     (symbol int, price double, volume long, timestamp long)
// (compiler.cpp fast_absent: the two streams, programs, the waiting time, per-stream key columns). What the product's
// host entry does around the kernels (seqpath.hip fast_absent, and build_event_index for the clock) is restated plainly
// here: the running maximum of the event times, the exclusive scans, a stable sort of the packed rows by key, the sort
// of the instance table and the stable sort of the outputs by (p, creation ordinal). Test infrastructure only
// (tests/test_absent_emu.py compares the outputs, the carry-out candidates and the instance table with a numpy
// statement of the rule). main(): a stand-alone self-check of the same entry, for sanitizer builds.
#define SM_HOST_EMU 1
#include "../../siddhi_amd/csrc/kernels/absent_dev.h"

#include "emu_fibers.h"

#include <algorithm>
#include <numeric>

#include "../../siddhi_amd/csrc/compiler.h"

// sid: the app stream of every row (-1: a heartbeat). clock_in: the app's clock before the batch. carry: nc rows of 7
// words [key, global ordinal, ts, symbol, price bits, volume, timestamp], sorted by (key, ordinal). inst: ni rows [key,
// creation ordinal] sorted by key, with room for ni + n rows; *ni_out its rows afterwards. per: sorted positions per
// chunk of the count scan (a multiple of 256). Outputs, room for n + nc each: e1 (relative to obase), ts_out, pos,
// create, vals (nsel words each, the raw 64-bit value); cand: room for 4 (n + nc) words. marks[6]: the plan's
// fast_absent, fast_pat_ms, fast_every_within, fast_seq_adjacent, fast_seq_k, fast_seq_ms. facts[4]: read rows, a read
// row below the clock, decreasing time among the read rows, the number of cancelling rows. Returns the number of
// outputs, or -1 (err says why: the text does not parse, or the compiler does not mark it).
extern "C" int64_t sm_absent_emu(const char* text, int64_t n, const int32_t* sid, const int32_t* sym, const double* price,
                                 const int64_t* vol, const int64_t* tcol, const int64_t* ts, int64_t clock_in,
                                 const int64_t* ordinals, int64_t obase, const int64_t* carry, int64_t nc, int64_t* inst,
                                 int64_t ni, int64_t* ni_out, int64_t per, uint32_t* e1, int64_t* ts_out, int64_t* pos,
                                 int64_t* create, int64_t* vals, int64_t* cand, int64_t* ncand, int32_t* marks,
                                 int64_t* facts, char* err, size_t errlen) {
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
  marks[0] = cq.fast_absent ? 1 : 0;
  marks[1] = cq.fast_pat_ms ? 1 : 0;
  marks[2] = cq.fast_every_within ? 1 : 0;
  marks[3] = cq.fast_seq_adjacent ? 1 : 0;
  marks[4] = cq.fast_seq_k;
  marks[5] = cq.fast_seq_ms;
  *ncand = 0;
  *ni_out = ni;
  if (!cq.fast_absent) {
    snprintf(err, errlen, "not marked for the timeout closed form");
    return -1;
  }
  if (cq.match_arity() != 1 || cq.hdr.nrefs != cq.hdr.nrefs_vis + 1) {
    snprintf(err, errlen, "the plan does not carry one hidden ref");
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
  const int sa = cq.fast_abs_stream[0], sb = cq.fast_abs_stream[1];

  MSeqSrc src{};
  src.n = n;
  src.sid = sid;
  for (int s : {sa, sb}) {
    src.read |= 1ull << s;
    if (keyed) {
      const int c = cq.fast_abs_keycol.at(s);
      src.kcol[s] = st.cols[c];
      if (st.types[c] == T_LONG) src.wide |= 1ull << s;
    }
  }
  src.ts = ts;
  src.ordinals = ordinals;
  src.obase = obase;

  // the clock at every row, as build_event_index writes it
  std::vector<int64_t> clk(n);
  {
    int64_t c = clock_in;
    for (int64_t i = 0; i < n; ++i) clk[i] = c = std::max(c, ts[i]);
  }
  const int64_t ntiles = (n + kSeqTile - 1) / kSeqTile;
  uint32_t below = 0;
  emu_launch((int)std::min<int64_t>(ntiles, 3), kSeqBlock,
             [&] { absent_clock_kernel(sid, src.read, ts, clk.data(), n, &below); });
  std::vector<uint32_t> tile_n(ntiles + 1, 0xDEADu);
  MSeqFacts f;
  memset(&f, 0, sizeof(f));
  emu_launch((int)std::min<int64_t>(ntiles, 3), kSeqBlock, [&] { mseq_facts_kernel(src, ntiles, tile_n.data(), &f); });
  constexpr uint64_t kBias = 0x8000000000000000ull;
  const int64_t np = (int64_t)f.nread;
  facts[0] = np;
  facts[1] = below;
  facts[2] = f.bad_ts;
  facts[3] = 0;
  if (below) return 0;  // FAST_NON_MONOTONE: nothing is touched
  const int64_t kmin = keyed && np > 0 ? (int64_t)(~f.kmin_c ^ kBias) : 0;
  const int64_t kmax = keyed && np > 0 ? (int64_t)(f.kmax ^ kBias) : 0;

  // the read rows in row order, then (keyed) in (key, arrival) order
  const bool packed = np > 0 && (keyed || np < n);
  std::vector<uint32_t> perm, skey;
  std::vector<uint8_t> sstr(np + 1, 0xEE);
  if (packed) {
    uint32_t run = 0;
    for (int64_t t = 0; t < ntiles; ++t) {
      const uint32_t c = tile_n[t];
      tile_n[t] = run;
      run += c;
    }
    std::vector<uint32_t> prow(np + 1, 0xDEADBEEFu), pkey(np + 1, 0xDEADBEEFu);
    std::vector<uint8_t> pstr(np + 1, 0xEE);
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
  const int nchunks = (int)((np + per - 1) / per);
  std::vector<int32_t> res(total + 4, 12345);
  std::vector<uint8_t> fl(np + 1, 0xEE);
  std::vector<uint32_t> ccnt(nchunks + 2, 0xDEADu), rk(n + 1, 0xDEADBEEFu), F(np + 1, 0xDEADBEEFu);
  uint32_t cand_n = 0;
  AbsArgs a{};
  a.np = np;
  a.n = n;
  a.ts = ts;
  a.clk = clk.data();
  a.st = &st;
  a.code = (const Instr*)(cq.blob.data() + cq.hdr.off_code);
  a.consts = (const DVal*)(cq.blob.data() + cq.hdr.off_const);
  a.c1_off = cq.fast_abs_off[0];
  a.c1_len = cq.fast_abs_len[0];
  a.c2_off = cq.fast_abs_off[1];
  a.c2_len = cq.fast_abs_len[1];
  a.wait = cq.fast_abs_wait;
  a.ordinals = ordinals;
  a.obase = obase;
  a.perm = packed ? perm.data() : nullptr;
  a.skey = keyed && np > 0 ? skey.data() : nullptr;
  a.kmin = kmin;
  a.kmax = kmax;
  a.sstr = packed ? sstr.data() : nullptr;
  a.sid = sid;
  a.sa = sa;
  a.sb = sb;
  a.ka = keyed ? src.kcol[sa] : nullptr;
  a.ka_wide = (int)((src.wide >> sa) & 1ull);
  a.carry = carry;
  a.nc = nc;
  a.cw = cw;
  a.per = per;
  a.nchunks = nchunks;
  a.fl = fl.data();
  a.ccnt = ccnt.data();
  a.rk = rk.data();
  a.F = F.data();
  a.res = res.data();
  a.cand = cand;
  a.cand_n = &cand_n;
  if (np > 0) {
    emu_launch(nchunks, kSeqBlock, [&] { absent_flag_kernel(a); });
    emu_launch(1, kSeqBlock, [&] { absent_chunk_kernel(ccnt.data(), nchunks); });
    emu_launch(nchunks, kSeqBlock, [&] { absent_next_kernel(a); });
    facts[3] = ccnt[nchunks];
    if (fl[np] != 0xEE || ccnt[nchunks + 1] != 0xDEADu || F[ccnt[nchunks]] != 0xDEADBEEFu) {
      snprintf(err, errlen, "the count scan wrote past its arrays");
      return -1;
    }
  }
  emu_launch((int)rtiles, kSeqBlock, [&] { absent_state_kernel<uint32_t>(a); });
  if (res[total] != 12345) {
    snprintf(err, errlen, "the state kernel wrote past res");
    return -1;
  }
  res.resize(total);
  std::vector<uint32_t> counts(rtiles + 1, 0);
  emu_launch((int)rtiles, kSeqBlock, [&] { seq_count_kernel(res.data(), total, counts.data()); });
  uint32_t run = 0;
  for (int64_t t = 0; t < rtiles; ++t) {
    const uint32_t c = counts[t];
    counts[t] = run;
    run += c;
  }
  const int64_t m = run;
  *ncand = cand_n;

  // the instances this batch created
  if (keyed && np > 0) {
    std::vector<int64_t> fresh(2 * np + 2, -7);
    uint32_t nfresh = 0;
    emu_launch((int)((np + kSeqBlock - 1) / kSeqBlock), kSeqBlock,
               [&] { absent_inst_kernel<uint32_t>(a, inst, ni, fresh.data(), &nfresh); });
    if (nfresh > 0) {
      const int64_t tot = ni + nfresh;
      std::vector<int64_t> all(inst, inst + 2 * ni), sorted(2 * tot);
      all.insert(all.end(), fresh.begin(), fresh.begin() + 2 * (int64_t)nfresh);
      std::vector<uint64_t> tk(tot);
      std::vector<uint32_t> ti(tot);
      const int g = (int)((tot + kSeqBlock - 1) / kSeqBlock);
      emu_launch(g, kSeqBlock, [&] { absent_inst_keys_kernel(all.data(), tot, tk.data(), ti.data()); });
      std::stable_sort(ti.begin(), ti.end(), [&](uint32_t x, uint32_t y) { return tk[x] < tk[y]; });
      emu_launch(g, kSeqBlock, [&] { absent_inst_gather_kernel(all.data(), ti.data(), tot, sorted.data()); });
      std::copy(sorted.begin(), sorted.end(), inst);
      ni = tot;
    }
  }
  *ni_out = ni;

  if (m > 0) {
    std::vector<uint32_t> pv(m + 1, 0xDEADBEEFu), xv(m + 1, 0xDEADBEEFu);
    emu_launch((int)rtiles, kSeqBlock, [&] { absent_emit_kernel(res.data(), total, counts.data(), pv.data(), xv.data()); });
    if (pv[m] != 0xDEADBEEFu || xv[m] != 0xDEADBEEFu) {
      snprintf(err, errlen, "emit wrote past its last output");
      return -1;
    }
    AbsProj pa{};
    pa.pv = pv.data();
    pa.xv = xv.data();
    std::vector<int64_t> cr(m);
    std::vector<uint64_t> ck(m);
    std::vector<uint32_t> idx(m), pk(m);
    const int g = (int)((m + kSeqBlock - 1) / kSeqBlock);
    if (keyed) {
      emu_launch(g, kSeqBlock, [&] { absent_create_kernel(a, xv.data(), m, inst, ni, cr.data(), ck.data(), idx.data()); });
      std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return ck[x] < ck[y]; });
      emu_launch(g, kSeqBlock, [&] { absent_pkeys_kernel(pv.data(), idx.data(), m, pk.data()); });
      std::vector<uint32_t> o(m), idx2(m);
      std::iota(o.begin(), o.end(), 0u);
      std::stable_sort(o.begin(), o.end(), [&](uint32_t x, uint32_t y) { return pk[x] < pk[y]; });
      for (int64_t k = 0; k < m; ++k) idx2[k] = idx[o[k]];
      idx.swap(idx2);
      pa.order = idx.data();
      pa.cr = cr.data();
    }
    const int ns = cq.hdr.nsel;
    std::vector<DVal> dv((size_t)m * ns + 1);
    pa.m = m;
    pa.nc = nc;
    pa.carry = carry;
    pa.cw = cw;
    pa.st = &st;
    pa.ts = ts;
    pa.ordinals = ordinals;
    pa.obase = obase;
    pa.wait = cq.fast_abs_wait;
    pa.blob = cq.blob.data();
    pa.e1 = e1;
    pa.vals = dv.data();
    pa.ts_out = ts_out;
    pa.pos = pos;
    pa.create = create;
    emu_launch(g, kSeqBlock, [&] { absent_project_kernel(pa); });
    for (int64_t k = 0; k < m * ns; ++k) vals[k] = dv[k].i;
  }
  return m;
}

#ifdef SM_ABSENT_EMU_MAIN
// Stand-alone self-check (sanitizer builds): `every e1=A[price>20] -> not B[price>45] for 6 milliseconds` over three
// streams with heartbeat rows, keyed (the key of B rows is their volume) and unkeyed, with carried partials, against a
// plain loop that keeps every instance's pending partials.
#include <map>
int main() {
  int bad = 0;
  const std::string defs =
      "@app:playback define stream A (symbol int, price double, volume long, timestamp long); "
      "define stream B (symbol int, price double, volume long, timestamp long); "
      "define stream C (symbol int, price double, volume long, timestamp long); ";
  const std::string q = "@info(name='q') from every e1=A[price>20] -> not B[price>45] for 6 milliseconds "
                        "select e1.timestamp as i insert into Out;";
  const int64_t W = 6;
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
        ts[i] = 10 + i / 3;
      }
      struct P {
        int64_t rel, t;
      };
      std::map<int64_t, std::vector<P>> open;
      std::vector<int64_t> carry;
      const int64_t obase = 1000;
      int64_t co = obase - 500;
      for (int kk = keyed ? -3 : 0; kk < (keyed ? K - 2 : 1); ++kk)  // (key K - 3 has no rows here)
        for (int r = 0; r < 3; ++r) {
          const double p = 40.0 + 6.0 * r;
          int64_t bits;
          memcpy(&bits, &p, 8);
          const int64_t t = 5 + 2 * r;
          carry.insert(carry.end(), {kk, co, t, kk, bits, 100 + r, co});
          open[kk].push_back(P{co - obase, t});
          ++co;
        }
      const int64_t nc = (int64_t)carry.size() / 7;
      std::vector<uint32_t> e1(n + nc + 1);
      std::vector<int64_t> tso(n + nc + 1), pos(n + nc + 1), create(n + nc + 1), vals(n + nc + 1), cand(4 * (n + nc) + 4);
      std::vector<int64_t> inst(2 * (n + nc) + 2);
      int64_t ni = 0, ncand = 0, facts[4];
      int32_t marks[6] = {0, 0, 0, 0, 0, 0};
      char err[256] = "";
      const int64_t m = sm_absent_emu(text.c_str(), n, sid.data(), sym.data(), price.data(), vol.data(), tcol.data(),
                                      ts.data(), 9, nullptr, obase, carry.data(), nc, inst.data(), 0, &ni, 256, e1.data(),
                                      tso.data(), pos.data(), create.data(), vals.data(), cand.data(), &ncand, marks,
                                      facts, err, sizeof(err));
      // (p, e1) pairs of the plain loop; the emulator's are compared as sets per position (the order across instances is
      // test_absent_emu.py's business)
      std::vector<std::pair<int64_t, int64_t>> exp, got;
      int64_t clock = 9;
      for (int64_t j = 0; j < n; ++j) {
        clock = std::max(clock, ts[j]);
        for (auto& kv : open) {
          std::vector<P> keep;
          for (const P& e : kv.second) {
            if (e.t + W <= clock) exp.push_back({j, e.rel});
            else keep.push_back(e);
          }
          kv.second.swap(keep);
        }
        if (sid[j] == 0 && price[j] > 20.0) open[keyed ? (int64_t)sym[j] : 0].push_back(P{j, ts[j]});
        if (sid[j] == 1 && price[j] > 45.0) open[keyed ? vol[j] : 0].clear();
      }
      int64_t keep = 0;
      for (auto& kv : open) keep += (int64_t)kv.second.size();
      for (int64_t k = 0; k < std::max<int64_t>(m, 0); ++k) got.push_back({pos[k], (int64_t)(int32_t)e1[k]});
      std::sort(exp.begin(), exp.end());
      std::sort(got.begin(), got.end());
      if (m < 0 || marks[0] != 1 || exp != got || ncand != keep) {
        fprintf(stderr, "absent_emu: mismatch at n=%lld keyed=%d (m=%lld exp=%zu cand=%lld keep=%lld) %s\n", (long long)n,
                keyed, (long long)m, exp.size(), (long long)ncand, (long long)keep, err);
        ++bad;
      }
    }
  if (!bad) printf("absent_emu self-check ok\n");
  return bad ? 1 : 0;
}
#endif
