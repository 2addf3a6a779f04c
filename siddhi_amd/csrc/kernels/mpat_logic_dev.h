// Device side of the closed form of the logical pair of two present events over up to three streams of one schema
// (seqpath.hip fast_pat_logic):
//   [partition with (ka of A, kb of B, kc of C)]
//   from every e1=A[c1] -> e2=B[c2(e1, e2)] and e3=C[c3(e1, e3)] within T          (and likewise with `or`)
// B is not C; `and`: A is neither; `or`: A may be either. Fed as one interleaved batch with a stream index per row
// (sm_app_process_device_events). R = {A, B, C}. Take the rows of a partition instance whose stream is in R, in arrival
// order (a row's instance key is the key attribute of its own stream; unpartitioned: all such rows); rows of other
// streams and heartbeat rows (stream -1) do not exist for the query. For every A row i with c1(i), let
//     j2(i) = min { j > i : stream[j] = B, same instance, c2(i, j) }
//     j3(i) = min { j > i : stream[j] = C, same instance, c3(i, j) }
// Neither condition reads the other operand, so the two are independent of each other.
//   and: emits (i, j2, j3) iff both exist and ts[max(j2, j3)] - ts[i] <= T, in order of (max(j2, j3), i), with the
//        timestamp of max(j2, j3), where the partial ends.
//   or:  with jm the smaller of those that exist, emits (i, j2 or null, j3 or null), only the side at jm bound, iff jm
//        exists and ts[jm] - ts[i] <= T, in order of (jm, i), with the timestamp of jm, where the partial ends.
// The window is measured from e1, not from the event bound last (unlike the k-state pattern's per-hop windows). With
// event time non-decreasing over the read rows, a candidate row beyond the window ends the partial, and so would every
// later one. A partial is open at the end of a batch iff it has not ended and ts_last - ts[i] <= T; an open `and`
// partial may hold one of e2 / e3 already. tests/test_pat_logic_plan.py ties this statement to the oracle.
//
// Facts, pack, the stable key sort and the stream byte of every sorted position are mseq_dev.h's, with R = {A, B, C}.
// The carry is mpatk_dev.h's two tables: the events bound by the open partials, each once, as rows
// [key, global ordinal, ts, attributes, stream] sorted by (key, ordinal); and the partials [key, s, o1, o2] with
// s = 1 (e1 alone; the only state of `or`), 2 (e1 and e2: o2 is e2's ordinal) or 3 (e1 and e3: o2 is e3's), every key's
// in order of o1.
//   plog_link_kernel   one lane per carried partial and per sorted position, mpat_link_kernel's shape. A lane holds t1,
//                      its scan position, two need bits (e2, e3) and the sources of the members found so far; a carried
//                      `and` partial in state 2 or 3 starts with one need bit clear. It scans forward inside its key run:
//                      the stream byte against B and C (only a side still needed is a candidate), then the window on
//                      candidate rows, then c2 or c3. `or`: the first hit ends the scan. `and`: a hit clears its need bit
//                      and records the member; the scan ends when both are clear. kMPatBudget positions on the lane's
//                      own, then the whole wave finishes the open scans one at a time, 64 consecutive positions per step
//                      with two hit ballots and one stop ballot: the first set bit of each hit ballot in front of the
//                      first stop decides, so an `and` scan may bind both sides in one step, or one side and go on with
//                      the other need bit. A scan is finished in one turn: no lane reads another lane's members. The
//                      result, the completing member's relative ordinal or kSeqNone, goes to the e1's own place (res[c]
//                      for carried partial c, res[ncp + row] for a batch row) with the three member sources (a batch row,
//                      -(carried event row) - 1, or kSeqNone) in mid: the order of emission is e1 ascending within a
//                      key. A partial that stays open leaves its state in kept[place] and a flag at each event it holds.
//   mpatk_cand_kernel  the flagged events as build_carry's candidates, one atomic per wave (build_carry sorts them: no
//                      result depends on the order of atomics)
//   plog_parts_kernel  after seq_count_kernel over `kept` and the scan: the new partial table, in order of place
//   plog_emit_kernel   after seq_count_kernel over `res` and the scan: the three words of every output, an absent `or`
//                      member as kPLogNull, and the completing member as the key of the one stable sort that follows
//                      (mpatk_tuples_kernel then writes the tuples in that order)
// Every wave operation is convergent, so the source also runs under the host wave emulator
// (tests/native/pat_logic_emu.cpp).
#pragma once
#include "mpatk_dev.h"

namespace sm {
namespace {

// the word of a member that `or` left unbound. A carried member's word is its ordinal relative to the batch's base, which
// lies in (-2^31, 0) (the facts pass checks that), and a batch member's is >= 0
constexpr uint32_t kPLogNull = 0x80000000u;

struct PLogArgs {
  int64_t np;               // read rows = sorted positions
  int64_t n;                // rows of the batch
  const int64_t* ts;
  const NfaStream* st;
  const Instr* code;
  const DVal* consts;
  int off[3], len[3];       // c1, c2 (slot 0 and e2's slot), c3 (slot 0 and e3's slot)
  int64_t within;           // T >= 0, against e1
  int64_t ts_last;          // event time of the batch's last read row
  const int64_t* ordinals;  // or nullptr: obase + row
  int64_t obase;
  const uint32_t* perm;     // row of each sorted position, or nullptr: every row is read, unkeyed
  const void* skey;         // key - kmin of each sorted position (K), or nullptr: unpartitioned
  int64_t kmin, kmax;
  const uint8_t* sstr;      // stream of each sorted position, or nullptr: sid[position]
  const int32_t* sid;
  int sa, sb, sc;           // app streams of e1, e2 and e3
  const int64_t* evt;       // carried events [key, global ordinal, ts, attributes, stream], sorted by (key, ordinal)
  int64_t ne;
  int cw;
  const int64_t* parts;     // carried partials [key, s, o1, o2]
  int64_t ncp;
  int32_t* res;             // out: ncp + n entries (entries of rows that are not read are filled by the host)
  int32_t* kept;            // out: likewise: the state of a partial that stays, else kSeqNone
  int32_t* mid;             // out: (ncp + n) rows of three member sources
  uint8_t* eflag;           // out: ne + n bytes, zeroed by the host
};

__device__ __forceinline__ int32_t plog_stream(const PLogArgs& a, int64_t p) {
  return a.sstr ? (int32_t)a.sstr[p] : a.sid[p];
}
__device__ __forceinline__ int64_t plog_row(const PLogArgs& a, int64_t p) { return a.perm ? (int64_t)a.perm[p] : p; }
__device__ __forceinline__ int32_t plog_rel(const PLogArgs& a, int64_t j) {
  return a.ordinals ? (int32_t)(a.ordinals[j] - a.obase) : (int32_t)j;
}

template <typename K, bool kAnd>
__global__ void __launch_bounds__(kSeqBlock) plog_link_kernel(PLogArgs a) {
  const K* skey = (const K*)a.skey;
  const int lane = threadIdx.x & 63;
  const Cond c1 = make_cond(a.code + a.off[0], a.len[0], a.consts);
  const Cond c2 = make_cond(a.code + a.off[1], a.len[1], a.consts);
  const Cond c3 = make_cond(a.code + a.off[2], a.len[2], a.consts);
  for (int it = 0; it < kSeqItems; ++it) {
    const int64_t v = (int64_t)blockIdx.x * kSeqTile + it * kSeqBlock + threadIdx.x;
    bool part = false, open = false;
    int64_t pos = 0, t1 = 0, x = 0, src = 0;  // x: the partial's place in res / kept / mid; src: e1's source
    int need = 3;                             // bit 0: e2, bit 1: e3
    int32_t m2 = kSeqNone, m3 = kSeqNone;     // the members' sources
    K kk = (K)0;
    if (v < a.ncp) {
      const int64_t* r = a.parts + v * 4;
      const int64_t key = r[0];
      const int s = (int)r[1];
      x = v;
      const int64_t e = mpatk_find_event(a.evt, a.ne, a.cw, key, r[2]);
      part = e >= 0 && s >= 1 && s <= (kAnd ? 3 : 1);
      if (part) {
        src = -e - 1;
        t1 = a.evt[e * a.cw + 2];
      }
      if (part && s >= 2) {  // half bound: one need bit is clear already
        const int64_t eb = mpatk_find_event(a.evt, a.ne, a.cw, key, r[3]);
        part = eb >= 0;
        if (s == 2) {
          m2 = (int32_t)(-eb - 1);
          need = 2;
        } else {
          m3 = (int32_t)(-eb - 1);
          need = 1;
        }
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
      const int64_t j = plog_row(a, u);
      kk = skey ? skey[u] : (K)0;
      x = a.ncp + j;
      if (plog_stream(a, u) == a.sa && eval(c1, RowLoader{a.st, j})) {
        part = open = true;
        t1 = a.ts[j];
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
        const int32_t sp = plog_stream(a, pos);
        const bool is2 = (need & 1) && sp == a.sb, is3 = (need & 2) && sp == a.sc;  // (B is not C: at most one)
        if (is2 || is3) {
          const int64_t j2 = plog_row(a, pos);
          const SeqPairLoader ld{a.st, src, j2, src < 0 ? a.evt + (-src - 1) * a.cw : nullptr};
          if (a.ts[j2] - t1 > a.within) {
            open = false;  // expired
          } else if (is2 ? eval(c2, ld) : eval(c3, ld)) {
            if (is2) {
              m2 = (int32_t)j2;
              need &= ~1;
            } else {
              m3 = (int32_t)j2;
              need &= ~2;
            }
            if (!kAnd || need == 0) {
              found = plog_rel(a, j2);
              open = false;
            }
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
      const int64_t t0 = __shfl(t1, l, 64), s0 = __shfl(src, l, 64);
      int n0 = __shfl(need, l, 64);
      const K k0 = (K)__shfl((unsigned long long)kk, l, 64);
      const int64_t* r0 = s0 < 0 ? a.evt + (-s0 - 1) * a.cw : nullptr;
      int64_t at2 = -1, at3 = -1;
      for (;;) {
        const int64_t p = p0 + lane;
        bool stop = p >= a.np || (skey && skey[p] != k0), hit2 = false, hit3 = false;
        if (!stop) {
          const int32_t sp = plog_stream(a, p);
          const bool is2 = (n0 & 1) && sp == a.sb, is3 = (n0 & 2) && sp == a.sc;
          if (is2 || is3) {
            const int64_t j2 = plog_row(a, p);
            const SeqPairLoader ld{a.st, s0, j2, r0};
            if (a.ts[j2] - t0 > a.within) stop = true;
            else if (is2) hit2 = eval(c2, ld);
            else hit3 = eval(c3, ld);
          }
        }
        // (all wave-uniform from here) hits count in front of the first stop only
        const uint64_t sm = __ballot(stop);
        const uint64_t front = sm ? (1ull << __builtin_ctzll(sm)) - 1 : ~0ull;
        uint64_t h2 = __ballot(hit2) & front, h3 = __ballot(hit3) & front;
        if (!kAnd && h2 && h3) {  // `or`: the earlier side alone
          if (__builtin_ctzll(h2) < __builtin_ctzll(h3)) h3 = 0;
          else h2 = 0;
        }
        if (h2) {
          at2 = p0 + __builtin_ctzll(h2);
          n0 &= ~1;
        }
        if (h3) {
          at3 = p0 + __builtin_ctzll(h3);
          n0 &= ~2;
        }
        if (sm || n0 == 0 || (!kAnd && n0 != 3)) break;
        p0 += 64;
      }
      if (lane == l) {
        if (at2 >= 0) m2 = (int32_t)plog_row(a, at2);
        if (at3 >= 0) m3 = (int32_t)plog_row(a, at3);
        need = n0;
        // the completing member is the later of those found now: what was found before lies in front of them
        if (kAnd ? n0 == 0 : n0 != 3) found = plog_rel(a, plog_row(a, at2 > at3 ? at2 : at3));
        open = false;
      }
      pend = __ballot(open);
    }
    // ---- the result and the members at the e1's place; carry-out: not ended, and a later event can still complete it
    const bool keep = part && found == kSeqNone && a.ts_last - t1 <= a.within;
    if (v < a.ncp + a.np) {
      a.res[x] = found;
      a.kept[x] = keep ? (need == 3 ? 1 : need == 2 ? 2 : 3) : kSeqNone;
      a.mid[3 * x] = (int32_t)src;
      a.mid[3 * x + 1] = m2;
      a.mid[3 * x + 2] = m3;
    }
    if (keep) {
      a.eflag[src < 0 ? -src - 1 : a.ne + src] = 1;
      if (m2 != kSeqNone) a.eflag[m2 < 0 ? -(int64_t)m2 - 1 : a.ne + m2] = 1;
      if (m3 != kSeqNone) a.eflag[m3 < 0 ? -(int64_t)m3 - 1 : a.ne + m3] = 1;
    }
  }
}

struct PLogOut {
  MSeqSrc s;
  const int32_t* flags;     // kept (parts) or res (emit): ncp + s.n entries
  int64_t total, ncp;
  const uint32_t* offsets;  // exclusive scan of seq_count_kernel's tile counts over flags
  const int32_t* mid;
  const int64_t* evt;
  int cw;
  const int64_t* parts;     // the carried partials (their keys)
  int64_t* parts_out;       // plog_parts_kernel: rows of 4 words
  uint32_t* tuples;         // plog_emit_kernel: rows of 3 words
  uint32_t* key;            // plog_emit_kernel: the completing member
  uint32_t* idx;            // plog_emit_kernel: 0 .. m - 1
};

__global__ void __launch_bounds__(kSeqBlock) plog_parts_kernel(PLogOut a) {
  __shared__ uint32_t wsum[kSeqBlock / 64];
  const int64_t r0 = (int64_t)blockIdx.x * kSeqTile + (int64_t)threadIdx.x * kSeqItems;
  int32_t v[kSeqItems];
  seq_load_items(a.flags, r0, a.total, v);
  uint32_t p = mpatk_rank(v, a.offsets, wsum);
  for (int q = 0; q < kSeqItems; ++q)
    if (v[q] != kSeqNone) {
      const int64_t x = r0 + q;
      int64_t* o = a.parts_out + (int64_t)p * 4;
      const int64_t j = x - a.ncp;
      o[0] = x < a.ncp ? a.parts[x * 4] : mseq_key(a.s, a.s.sid[j], j);
      o[1] = v[q];
      o[2] = mpatk_ordinal(a.mid[3 * x], a.s.ordinals, a.s.obase, a.evt, a.cw);
      o[3] = v[q] == 1 ? 0 : mpatk_ordinal(a.mid[3 * x + v[q] - 1], a.s.ordinals, a.s.obase, a.evt, a.cw);
      ++p;
    }
}

__global__ void __launch_bounds__(kSeqBlock) plog_emit_kernel(PLogOut a) {
  __shared__ uint32_t wsum[kSeqBlock / 64];
  const int64_t r0 = (int64_t)blockIdx.x * kSeqTile + (int64_t)threadIdx.x * kSeqItems;
  int32_t v[kSeqItems];
  seq_load_items(a.flags, r0, a.total, v);
  uint32_t p = mpatk_rank(v, a.offsets, wsum);
  for (int q = 0; q < kSeqItems; ++q)
    if (v[q] != kSeqNone) {
      const int64_t x = r0 + q;
      uint32_t* o = a.tuples + (int64_t)p * 3;
      for (int i = 0; i < 3; ++i) {
        const int32_t src = a.mid[3 * x + i];
        o[i] = src == kSeqNone
                   ? kPLogNull
                   : (uint32_t)(int32_t)(mpatk_ordinal(src, a.s.ordinals, a.s.obase, a.evt, a.cw) - a.s.obase);
      }
      a.key[p] = (uint32_t)v[q];
      a.idx[p] = p;
      ++p;
    }
}

}  // namespace
}  // namespace sm
