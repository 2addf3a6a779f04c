// Device side of the closed form of the count pattern over three different streams of one schema (seqpath.hip
// fast_pat_count):
//   [partition with (ka of A, kb of B, kc of C)]
//   from every e1=A[c1] -> e2=B[c2(e1, e2)]<m:n> -> e3=C[c3(e1, e3)] within T          0 <= m <= n, 1 <= n <= 6
// Fed as one interleaved batch with a stream index per row (sm_app_process_device_events). R = {A, B, C}. Take the rows
// of a partition instance whose stream is in R, in arrival order (a row's instance key is the key attribute of its own
// stream; unpartitioned: all such rows); rows of other streams and heartbeat rows (stream -1) do not exist for the query.
// For every A row i with c1(i):
//     hits      the later B rows j of the instance with c2(i, j), in order; the partial binds the first n of them
//     p(i)      the row of the m-th hit (i itself if m = 0): from there on the partial also waits for e3 ("in e3")
//     tlast(j)  the time of the last hit bound before row j, or ts[i] if none: a bind refreshes the partial's clock
// Walk the C rows j > p(i) of the instance in order, whether or not they pass c3: if ts[j] - tlast(j) > T the partial is
// dead (no output, no more hits, not carried; a later hit does not revive it); otherwise, if c3(i, j), it emits
// (i, hits bound before j, j) with j's timestamp and ends. Nothing else ends a partial: the window is not measured from
// e1, B and A rows expire nothing, and a partial with fewer than m hits has no clock at all. Outputs come in order of
// (j, p(i), i). tests/test_pat_count_plan.py ties this statement to the oracle.
//
// Facts, pack, the stable key sort and the stream byte of every sorted position are mseq_dev.h's, with R = {A, B, C}.
// The carry is mpatk_dev.h's two tables: the events held by the open partials, each once, as rows
// [key, global ordinal, ts, attributes, stream] sorted by (key, ordinal); and the partials
// [key, hits | in-e3 << 8, tlast, p, o1, n hit ordinals] (n + 5 words; p and unbound slots 0), every key's in order of o1.
// A partial is open at the end of a batch unless it emitted or died; one holding n hits whose clock has run out at the
// batch's last read row (ts_last - tlast > T) is dropped too: its next C row kills it, whatever comes before.
//   pcnt_link_kernel   one lane per carried partial and per sorted position, plog_link_kernel's shape. A lane holds its
//                      e1's source, its scan position, the hit count, tlast and the sources of the hits bound so far. It
//                      scans forward inside its key run: a B row while hits < n evaluates c2, and a hit binds and
//                      refreshes tlast; a C row while hits >= m checks the window against tlast (death), then c3 (emit).
//                      No window stops the scan at run distance: it ends at emit, death or the end of the run.
//                      kMPatBudget positions on the lane's own, then the whole wave finishes the open scans one at a
//                      time, 64 consecutive positions per step. Within a step every lane states its position's facts (a
//                      hit, a C row, c3, the time) and the facts meet as ballots: the first n - hits set bits of the hit
//                      ballot bind; a C lane counts the binding bits in front of it (in e3 or not) and takes the time of
//                      the last of them as its tlast (one shuffle); the first C bit in e3 that dies or passes decides, and
//                      only the hits in front of it bind. Several hits, the m-th among them, and the deciding C row may
//                      fall in one step. A scan is finished in one turn: no lane reads another lane's members. The
//                      result, e3's relative ordinal or kSeqNone, goes to the e1's own place (res[c] for carried partial
//                      c, res[ncp + row] for a batch row) with the n + 1 member sources (a batch row, -(carried event
//                      row) - 1, or kSeqNone) in mid. A partial that stays open leaves hits | in-e3 << 8 in kept[place]
//                      and a flag at each event it holds.
//   mpatk_cand_kernel  the flagged events as build_carry's candidates
//   pcnt_parts_kernel  after seq_count_kernel over `kept` and the scan: the new partial table, in order of place
//   pcnt_emit_kernel   after seq_count_kernel over `res` and the scan: the n + 2 words of every output, an unbound slot
//                      as kPCntNull, and (e3, p) as the 64-bit key of the one stable sort that follows (the placement is
//                      in order of e1 within a key; mpatk_tuples_kernel then writes the tuples in that order)
// Every wave operation is convergent, so the source also runs under the host wave emulator
// (tests/native/pat_count_emu.cpp).
#pragma once
#include "mpatk_dev.h"

namespace sm {
namespace {

constexpr int kPCntMax = 6;  // hit slots at most: a tuple is at most 8 words
// the word of a hit slot that is not bound. A carried member's word is its ordinal relative to the batch's base, which
// lies in (-2^31, 0) (the facts pass checks that), and a batch member's is >= 0
constexpr uint32_t kPCntNull = 0x80000000u;

struct PCntArgs {
  int64_t np;               // read rows = sorted positions
  int64_t n;                // rows of the batch
  const int64_t* ts;
  const NfaStream* st;
  const Instr* code;
  const DVal* consts;
  int off[3], len[3];       // c1, c2 (slot 0 and the current e2), c3 (slot 0 and e3)
  int cmin, cmax;           // m, n
  int64_t within;           // T >= 0, against tlast
  int64_t ts_last;          // event time of the batch's last read row
  const int64_t* ordinals;  // or nullptr: obase + row
  int64_t obase;
  const uint32_t* perm;     // row of each sorted position, or nullptr: every row is read, unkeyed
  const void* skey;         // key - kmin of each sorted position (K), or nullptr: unpartitioned
  int64_t kmin, kmax;
  const uint8_t* sstr;      // stream of each sorted position, or nullptr: sid[position]
  const int32_t* sid;
  int sa, sb, sc;           // app streams of e1, e2 and e3, pairwise different
  const int64_t* evt;       // carried events [key, global ordinal, ts, attributes, stream], sorted by (key, ordinal)
  int64_t ne;
  int cw;
  const int64_t* parts;     // carried partials [key, hits | in-e3 << 8, tlast, p, o1, cmax hit ordinals]
  int64_t ncp;
  int32_t* res;             // out: ncp + n entries (entries of rows that are not read are filled by the host)
  int32_t* kept;            // out: likewise: hits | in-e3 << 8 of a partial that stays, else kSeqNone
  int32_t* mid;             // out: (ncp + n) rows of cmax + 1 member sources
  uint8_t* eflag;           // out: ne + n bytes, zeroed by the host
};

__device__ __forceinline__ int32_t pcnt_stream(const PCntArgs& a, int64_t p) {
  return a.sstr ? (int32_t)a.sstr[p] : a.sid[p];
}
__device__ __forceinline__ int64_t pcnt_row(const PCntArgs& a, int64_t p) { return a.perm ? (int64_t)a.perm[p] : p; }
__device__ __forceinline__ int32_t pcnt_rel(const PCntArgs& a, int64_t j) {
  return a.ordinals ? (int32_t)(a.ordinals[j] - a.obase) : (int32_t)j;
}
// h[k] = v with k known at run time: six predicated moves, so that h stays in registers
__device__ __forceinline__ void pcnt_set(int32_t (&h)[kPCntMax], int k, int32_t v) {
#pragma unroll
  for (int q = 0; q < kPCntMax; ++q)
    if (q == k) h[q] = v;
}

template <typename K>
__global__ void __launch_bounds__(kSeqBlock) pcnt_link_kernel(PCntArgs a) {
  const K* skey = (const K*)a.skey;
  const int lane = threadIdx.x & 63;
  const Cond c1 = make_cond(a.code + a.off[0], a.len[0], a.consts);
  const Cond c2 = make_cond(a.code + a.off[1], a.len[1], a.consts);
  const Cond c3 = make_cond(a.code + a.off[2], a.len[2], a.consts);
  const int pw = a.cmax + 5, mw = a.cmax + 1;
  const uint64_t below = lane ? ~0ull >> (64 - lane) : 0ull;  // the lanes in front of this one
  for (int it = 0; it < kSeqItems; ++it) {
    const int64_t v = (int64_t)blockIdx.x * kSeqTile + it * kSeqBlock + threadIdx.x;
    bool part = false, open = false, dead = false;
    int64_t pos = 0, tlast = 0, x = 0, src = 0;  // x: the partial's place in res / kept / mid; src: e1's source
    int cnt = 0;
    int32_t h[kPCntMax];
#pragma unroll
    for (int q = 0; q < kPCntMax; ++q) h[q] = kSeqNone;
    K kk = (K)0;
    if (v < a.ncp) {
      const int64_t* r = a.parts + v * pw;
      const int64_t key = r[0];
      const int c = (int)(r[1] & 0xff);
      x = v;
      const int64_t e = mpatk_find_event(a.evt, a.ne, a.cw, key, r[4]);
      // (a row that fails here has no partial and is dropped; sm_app_restore checks the same conditions on a snapshot's
      // tables and the driver writes no other rows, so none does)
      part = e >= 0 && c <= a.cmax && (r[1] >> 8) == (c >= a.cmin ? 1 : 0);
      if (part) {
        src = -e - 1;
        tlast = r[2];
        for (int q = 0; q < c; ++q) {
          const int64_t eb = mpatk_find_event(a.evt, a.ne, a.cw, key, r[5 + q]);
          if (eb < 0) part = false;
          pcnt_set(h, q, (int32_t)(-eb - 1));
        }
        cnt = c;
      }
      if (part) {
        if (!skey) {
          open = true;
        } else if (key >= a.kmin && key <= a.kmax) {  // the head of the key's run, if it has rows here
          kk = (K)((uint64_t)key - (uint64_t)a.kmin);
          int64_t lo = 0, hi = a.np;
          while (lo < hi) {
            const int64_t md = (lo + hi) >> 1;
            if (skey[md] < kk) lo = md + 1;
            else hi = md;
          }
          pos = lo;
          open = lo < a.np && skey[lo] == kk;
        }
      }
    } else if (v < a.ncp + a.np) {
      const int64_t u = v - a.ncp;
      const int64_t j = pcnt_row(a, u);
      kk = skey ? skey[u] : (K)0;
      x = a.ncp + j;
      if (pcnt_stream(a, u) == a.sa && eval(c1, RowLoader{a.st, j})) {
        part = open = true;
        tlast = a.ts[j];
        pos = u + 1;
        src = j;
      }
    }
    int32_t found = kSeqNone;
    // ---- the lane's own budget
    const int64_t stop_at = pos + kMPatBudget;
    while (open && pos < stop_at) {
      if (pos >= a.np || (skey && skey[pos] != kk)) {
        open = false;  // the key's rows ran out
      } else {
        const int32_t sp = pcnt_stream(a, pos);
        if (sp == a.sb && cnt < a.cmax) {
          const int64_t j2 = pcnt_row(a, pos);
          if (eval(c2, SeqPairLoader{a.st, src, j2, src < 0 ? a.evt + (-src - 1) * a.cw : nullptr})) {
            pcnt_set(h, cnt, (int32_t)j2);
            ++cnt;
            tlast = a.ts[j2];
          }
        } else if (sp == a.sc && cnt >= a.cmin) {
          const int64_t j3 = pcnt_row(a, pos);
          if (a.ts[j3] - tlast > a.within) {
            dead = true;
            open = false;
          } else if (eval(c3, SeqPairLoader{a.st, src, j3, src < 0 ? a.evt + (-src - 1) * a.cw : nullptr})) {
            found = pcnt_rel(a, j3);
            open = false;
          }
        }
      }
      if (open) ++pos;
    }
    // ---- wave-cooperative finish of the open scans: one scan at a time, to its end, 64 consecutive sorted positions
    // per step
    uint64_t pend = __ballot(open);
    while (pend) {
      const int l = __builtin_ctzll(pend);
      int64_t p0 = __shfl(pos, l, 64);
      const int64_t s0 = __shfl(src, l, 64);
      int64_t tl0 = __shfl(tlast, l, 64);
      int n0 = __shfl(cnt, l, 64);
      const K k0 = (K)__shfl((unsigned long long)kk, l, 64);
      const int64_t* r0 = s0 < 0 ? a.evt + (-s0 - 1) * a.cw : nullptr;
      int32_t f0 = kSeqNone;
      bool d0 = false;
      for (;;) {
        const int64_t p = p0 + lane;
        const bool stop = p >= a.np || (skey && skey[p] != k0);
        bool hit = false, isc = false, cpass = false;
        int64_t t = 0;
        if (!stop) {
          const int32_t sp = pcnt_stream(a, p);
          if ((sp == a.sb && n0 < a.cmax) || sp == a.sc) {
            const int64_t j2 = pcnt_row(a, p);
            const SeqPairLoader ld{a.st, s0, j2, r0};
            t = a.ts[j2];
            if (sp == a.sb) {
              hit = eval(c2, ld);
            } else {
              isc = true;
              cpass = eval(c3, ld);
            }
          }
        }
        // (all wave-uniform from here unless said otherwise) facts count in front of the first stop only
        const uint64_t sm = __ballot(stop);
        const uint64_t front = sm ? (1ull << __builtin_ctzll(sm)) - 1 : ~0ull;
        uint64_t hb = 0, rest = __ballot(hit) & front;
        for (int q = n0; q < a.cmax && rest; ++q) {  // the first n - hits of them bind
          hb |= rest & (0 - rest);
          rest &= rest - 1;
        }
        // (per lane) a C row sees the hits in front of it
        const uint64_t mine = hb & below;
        const int lh = mine ? 63 - __builtin_clzll(mine) : 0;
        const int64_t th = __shfl(t, lh, 64);
        const bool in3 = isc && !stop && n0 + __popcll(mine) >= a.cmin;
        const bool late = in3 && t - (mine ? th : tl0) > a.within;
        const bool pass = in3 && !late && cpass;
        const uint64_t lb = __ballot(late) & front, pb = __ballot(pass) & front;
        const uint64_t db = lb | pb;
        const int d = db ? __builtin_ctzll(db) : 64;
        const uint64_t bound = d < 64 ? hb & ((1ull << d) - 1) : hb;  // the hits in front of the deciding row
        const int lastb = bound ? 63 - __builtin_clzll(bound) : 0;
        const int64_t tb = __shfl(t, lastb, 64);
        if (bound) tl0 = tb;
        if (lane == l) {
          uint64_t bm = bound;
          int q = n0;
          while (bm) {
            pcnt_set(h, q++, (int32_t)pcnt_row(a, p0 + __builtin_ctzll(bm)));
            bm &= bm - 1;
          }
        }
        n0 += __popcll(bound);
        if (d < 64) {
          if ((pb >> d) & 1) f0 = pcnt_rel(a, pcnt_row(a, p0 + d));
          else d0 = true;
          break;
        }
        if (sm) break;
        p0 += 64;
      }
      if (lane == l) {
        cnt = n0;
        tlast = tl0;
        found = f0;
        dead = d0;
        open = false;
      }
      pend = __ballot(open);
    }
    // ---- the result and the members at the e1's place; carry-out: not ended, and a later event can still complete it
    const bool keep = part && found == kSeqNone && !dead && !(cnt == a.cmax && a.ts_last - tlast > a.within);
    if (v < a.ncp + a.np) {
      a.res[x] = found;
      a.kept[x] = keep ? (cnt | (cnt >= a.cmin ? 0x100 : 0)) : kSeqNone;
      a.mid[mw * x] = (int32_t)src;
#pragma unroll
      for (int q = 0; q < kPCntMax; ++q)
        if (q < a.cmax) a.mid[mw * x + 1 + q] = h[q];
    }
    if (keep) {
      a.eflag[src < 0 ? -src - 1 : a.ne + src] = 1;
#pragma unroll
      for (int q = 0; q < kPCntMax; ++q)
        if (q < cnt) a.eflag[h[q] < 0 ? -(int64_t)h[q] - 1 : a.ne + h[q]] = 1;
    }
  }
}

struct PCntOut {
  MSeqSrc s;
  const int32_t* flags;     // kept (parts) or res (emit): ncp + s.n entries
  int64_t total, ncp;
  const uint32_t* offsets;  // exclusive scan of seq_count_kernel's tile counts over flags
  const int32_t* mid;
  int cmin, cmax;
  const int64_t* evt;
  int cw;
  const int64_t* parts;     // the carried partials (their keys)
  int64_t* parts_out;       // pcnt_parts_kernel: rows of cmax + 5 words
  uint32_t* tuples;         // pcnt_emit_kernel: rows of cmax + 2 words
  uint64_t* key;            // pcnt_emit_kernel: e3 << 32 | p with its sign flipped (a carried p sorts first)
  uint32_t* idx;            // pcnt_emit_kernel: 0 .. m - 1
};

__global__ void __launch_bounds__(kSeqBlock) pcnt_parts_kernel(PCntOut a) {
  __shared__ uint32_t wsum[kSeqBlock / 64];
  const int64_t r0 = (int64_t)blockIdx.x * kSeqTile + (int64_t)threadIdx.x * kSeqItems;
  int32_t v[kSeqItems];
  seq_load_items(a.flags, r0, a.total, v);
  uint32_t p = mpatk_rank(v, a.offsets, wsum);
  const int pw = a.cmax + 5, mw = a.cmax + 1;
  for (int q = 0; q < kSeqItems; ++q)
    if (v[q] != kSeqNone) {
      const int64_t x = r0 + q;
      int64_t* o = a.parts_out + (int64_t)p * pw;
      const int64_t j = x - a.ncp;
      const int32_t* m = a.mid + mw * x;
      const int cnt = v[q] & 0xff;
      const int64_t last = m[cnt];  // the event bound last: e1, or the last hit
      o[0] = x < a.ncp ? a.parts[x * pw] : mseq_key(a.s, a.s.sid[j], j);
      o[1] = v[q];
      o[2] = last < 0 ? a.evt[(-last - 1) * a.cw + 2] : a.s.ts[last];
      o[3] = cnt >= a.cmin ? mpatk_ordinal(m[a.cmin], a.s.ordinals, a.s.obase, a.evt, a.cw) : 0;
      o[4] = mpatk_ordinal(m[0], a.s.ordinals, a.s.obase, a.evt, a.cw);
      for (int i = 0; i < a.cmax; ++i)
        o[5 + i] = i < cnt ? mpatk_ordinal(m[1 + i], a.s.ordinals, a.s.obase, a.evt, a.cw) : 0;
      ++p;
    }
}

__global__ void __launch_bounds__(kSeqBlock) pcnt_emit_kernel(PCntOut a) {
  __shared__ uint32_t wsum[kSeqBlock / 64];
  const int64_t r0 = (int64_t)blockIdx.x * kSeqTile + (int64_t)threadIdx.x * kSeqItems;
  int32_t v[kSeqItems];
  seq_load_items(a.flags, r0, a.total, v);
  uint32_t p = mpatk_rank(v, a.offsets, wsum);
  const int mw = a.cmax + 1, tw = a.cmax + 2;
  for (int q = 0; q < kSeqItems; ++q)
    if (v[q] != kSeqNone) {
      const int64_t x = r0 + q;
      uint32_t* o = a.tuples + (int64_t)p * tw;
      for (int i = 0; i < mw; ++i) {
        const int32_t src = a.mid[mw * x + i];
        o[i] = src == kSeqNone
                   ? kPCntNull
                   : (uint32_t)(int32_t)(mpatk_ordinal(src, a.s.ordinals, a.s.obase, a.evt, a.cw) - a.s.obase);
      }
      o[mw] = (uint32_t)v[q];
      // p: the m-th hit, or e1 (an emitting partial holds at least m hits)
      a.key[p] = (uint64_t)(uint32_t)v[q] << 32 | (o[a.cmin] ^ 0x80000000u);
      a.idx[p] = p;
      ++p;
    }
}

}  // namespace
}  // namespace sm
