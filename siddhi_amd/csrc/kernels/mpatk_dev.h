// Device side of the closed form of the k-state pattern over several streams of one schema (seqpath.hip fast_pat_k):
//   [partition with (ka of A, kb of B, ...)]
//   from every e1=S1[c1] -> e2=S2[c2] within T2 -> ... -> ek=Sk[ck] within Tk          3 <= k <= 8
// fed as one interleaved batch with a stream index per row (sm_app_process_device_events). R = {S1 .. Sk}. Take the
// events of a partition instance whose stream is in R, in arrival order (an event's instance key is the key attribute
// of its own stream; unpartitioned: all such events); rows of other streams and heartbeat rows (stream -1) do not exist
// for the query. For every event i on S1 with c1(i), put o1 = i and, for m = 2 .. k,
//     om = min { j > o(m-1) : stream[j] = Sm, key[j] = key[i], cm(o1, ..., o(m-1), j) }
// The chain stops, without an output, if om does not exist or ts[om] - ts[o(m-1)] > Tm: the window is inclusive and
// measured from the event bound before, not from e1. The query emits (o1, ..., ok) in lexicographic order of
// (ok, o(k-1), ..., o1). With event time non-decreasing over the read rows an Sm event beyond the window removes the
// partial, and so would every later one. tests/test_mpatk_plan.py ties this statement to the oracle.
//
// Facts, pack, the stable key sort and the stream byte of every sorted position are mseq_dev.h's, with R = {S1 .. Sk}.
// The carry is two tables: the events bound by the open partials, each once however many partials share it, as rows
// [key, global ordinal, ts, attributes, stream] sorted by (key, ordinal) (path 8's rows); and the partials,
// [key, s, o1 .. os] padded to k - 1 global ordinals, every key's in order of o1.
//   mpatk_link_kernel    one lane per carried partial and per sorted position, as mpat_link_kernel. A lane holds its
//                        partial's next state m, its scan position and the time of the event bound last. It scans
//                        forward inside its key run: the stream byte against Sm, then the window (an Sm event beyond it
//                        ends the chain), then cm. On a hit below the last state it writes the member's source (a batch
//                        row, or -(carried event row) - 1) into its own row of `mid`, which cm's slot loader reads
//                        back, takes the hit's time as the reference, moves to m + 1 and goes on from the next position:
//                        a state change may fall inside the lane's own budget (kMPatBudget positions) or inside the
//                        whole-wave finish (64 positions per step, one ballot), which carries m along. The result, ek's
//                        relative ordinal or kSeqNone, is written at the e1's own place: res[c] for carried partial c,
//                        res[ncp + row] for a batch row. A partial left open after s bound events stays iff
//                        ts_last - t_ref <= T(s+1): kept[place] = s, and a flag is set at each of its bound events.
//   mpatk_cand_kernel    the flagged events as build_carry's candidates, one atomic per wave (build_carry sorts them: no
//                        result depends on the order of atomics)
//   mpatk_parts_kernel   after seq_count_kernel over `kept` and the scan: the new partial table, in order of place
//                        (carried partials, then batch rows: within a key that is the order of o1)
//   mpatk_emit_kernel    after seq_count_kernel over `res` and the scan: the k relative ordinals of every output,
//                        compacted in order of place
//   mpatk_keys_kernel    member m of every tuple in the current order, as the key of the next stable sort (e2, e3, ...,
//                        ek in turn; a carried member sorts before every batch row)
//   mpatk_tuples_kernel  the tuples in their final order
// Every wave operation is convergent, so the source also runs under the host wave emulator (tests/native/mpatk_emu.cpp).
#pragma once
#include "mpat_dev.h"

namespace sm {
namespace {

struct MPatKArgs {
  int64_t np;               // read rows = sorted positions
  int64_t n;                // rows of the batch
  const int64_t* ts;
  const NfaStream* st;
  const Instr* code;
  const DVal* consts;
  int k;
  int off[kSeqKMax], len[kSeqKMax];
  int64_t within[kSeqKMax];  // of element m against element m - 1 (m >= 1)
  int32_t want[kSeqKMax];    // S1 .. Sk
  int64_t ts_last;          // event time of the batch's last read row
  const int64_t* ordinals;  // or nullptr: obase + row
  int64_t obase;
  const uint32_t* perm;     // row of each sorted position, or nullptr: every row is read, unkeyed
  const void* skey;         // key - kmin of each sorted position (K), or nullptr: unpartitioned
  int64_t kmin, kmax;
  const uint8_t* sstr;      // stream of each sorted position, or nullptr: sid[position]
  const int32_t* sid;
  const int64_t* evt;       // carried events [key, global ordinal, ts, attributes, stream], sorted by (key, ordinal)
  int64_t ne;
  int cw;
  const int64_t* parts;     // carried partials [key, s, o1 .. o(k-1)]
  int64_t ncp;
  int32_t* res;             // out: ncp + n entries (entries of rows that are not read are filled by the host)
  int32_t* kept;            // out: likewise: bound events of a partial that stays, else kSeqNone
  int32_t* mid;             // out: (ncp + n) rows of k - 1 member sources
  uint8_t* eflag;           // out: ne + n bytes, zeroed by the host
};

__device__ __forceinline__ void mpatk_fence() {
#ifndef SM_HOST_EMU
  __threadfence_block();  // a lane's `mid` row is read by the other lanes of its wave
#endif
}

__device__ __forceinline__ int32_t mpatk_stream(const MPatKArgs& a, int64_t p) {
  return a.sstr ? (int32_t)a.sstr[p] : a.sid[p];
}
__device__ __forceinline__ int64_t mpatk_row(const MPatKArgs& a, int64_t p) { return a.perm ? (int64_t)a.perm[p] : p; }

// row of (key, ordinal) in the carried events, or -1
__device__ __forceinline__ int64_t mpatk_find_event(const int64_t* evt, int64_t ne, int cw, int64_t key, int64_t ord) {
  int64_t lo = 0, hi = ne;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const int64_t* r = evt + mid * cw;
    if (r[0] < key || (r[0] == key && r[1] < ord)) lo = mid + 1;
    else hi = mid;
  }
  return lo < ne && evt[lo * cw] == key && evt[lo * cw + 1] == ord ? lo : -1;
}

// cm over slots 0 .. m: slot m is batch row j, an earlier slot the partial's bound member (a batch row, or a carried
// event's canonical words). Programs read slots at index 0 / CURRENT only (one event per slot).
struct MPatKLoader {
  const MPatKArgs* a;
  const int32_t* mid;  // the partial's row of member sources
  int m;
  int64_t j;
  __device__ StackVal var(const Instr& in) const {
    if (in.op == OP_COL) return col_value(a->st, in.a, j);  // (refused by the host entry)
    if (!(in.b == 0 || in.b == -1) || in.a < 0 || in.a > m) {
      StackVal v;
      v.i = 0;
      v.null = 1;
      return v;
    }
    if (in.a == m) return col_value(a->st, in.c, j);
    const int64_t src = mid[in.a];
    if (src < 0) {
      const int t = a->st->types[in.c];
      StackVal v = uncanon((uint64_t)a->evt[(-src - 1) * a->cw + 3 + in.c], t);
      if (t == T_STRING) v.null = v.i < 0;
      return v;
    }
    return col_value(a->st, in.c, src);
  }
};

__device__ __forceinline__ bool mpatk_cond(const MPatKArgs& a, int m, const MPatKLoader& ld) {
  return a.len[m] == 0 || truthy(eval_prog(a.code + a.off[m], a.len[m], a.consts, ld));
}

template <typename K>
__global__ void __launch_bounds__(kSeqBlock) mpatk_link_kernel(MPatKArgs a) {
  const K* skey = (const K*)a.skey;
  const int lane = threadIdx.x & 63;
  const int k = a.k, pw = k + 1;
  for (int it = 0; it < kSeqItems; ++it) {
    const int64_t v = (int64_t)blockIdx.x * kSeqTile + it * kSeqBlock + threadIdx.x;
    bool part = false, open = false;
    int64_t pos = 0, tref = 0, x = 0;  // x: the partial's place in res / kept / mid
    int m = 1;                        // the state the partial waits in = its bound events
    K kk = (K)0;
    if (v < a.ncp) {
      const int64_t* r = a.parts + v * pw;
      const int64_t key = r[0];
      x = v;
      m = (int)r[1];
      part = m >= 1 && m < k;
      int64_t last = -1;
      for (int i = 0; part && i < m; ++i) {
        last = mpatk_find_event(a.evt, a.ne, a.cw, key, r[2 + i]);
        part = last >= 0;
        a.mid[x * (k - 1) + i] = (int32_t)(-last - 1);
      }
      if (part) {
        tref = a.evt[last * a.cw + 2];
        if (!skey) {
          open = true;
        } else if (key >= a.kmin && key <= a.kmax) {  // the head of the key's run, if it has events here
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
      const int64_t j = mpatk_row(a, u);
      kk = skey ? skey[u] : (K)0;
      x = a.ncp + j;
      if (mpatk_stream(a, u) == a.want[0] && mpatk_cond(a, 0, MPatKLoader{&a, nullptr, 0, j})) {
        part = open = true;
        tref = a.ts[j];
        pos = u + 1;
        a.mid[x * (k - 1)] = (int32_t)j;
      }
    }
    int32_t* mine = a.mid + x * (k - 1);
    int32_t found = kSeqNone;
    // ---- the lane's own budget
    const int64_t stop_at = pos + kMPatBudget;
    while (open && pos < stop_at) {
      if (pos >= a.np || (skey && skey[pos] != kk)) {
        open = false;  // the key's events ran out
      } else if (mpatk_stream(a, pos) == a.want[m]) {
        const int64_t j2 = mpatk_row(a, pos);
        if (a.ts[j2] - tref > a.within[m]) {
          open = false;  // expired
        } else if (mpatk_cond(a, m, MPatKLoader{&a, mine, m, j2})) {
          if (m == k - 1) {
            found = a.ordinals ? (int32_t)(a.ordinals[j2] - a.obase) : (int32_t)j2;
            open = false;
          } else {
            mine[m] = (int32_t)j2;
            tref = a.ts[j2];
            ++m;
          }
        }
      }
      if (open) ++pos;
    }
    // ---- wave-cooperative finish of the open scans: one scan at a time, 64 consecutive sorted positions per step; a
    // scan that binds a member below the last state stays open and is taken up again in its next state
    mpatk_fence();
    uint64_t pend = __ballot(open);
    while (pend) {
      const int l = __builtin_ctzll(pend);
      int64_t p0 = __shfl(pos, l, 64);
      const int64_t t0 = __shfl(tref, l, 64), x0 = __shfl(x, l, 64);
      const int m0 = __shfl(m, l, 64);
      const K k0 = (K)__shfl((unsigned long long)kk, l, 64);
      const int32_t* mid0 = a.mid + x0 * (k - 1);
      const int32_t want0 = a.want[m0];
      const int64_t w0 = a.within[m0];
      int64_t at = -1;
      for (;;) {
        const int64_t p = p0 + lane;
        bool stop = p >= a.np || (skey && skey[p] != k0), hit = false;
        if (!stop && mpatk_stream(a, p) == want0) {
          const int64_t j2 = mpatk_row(a, p);
          if (a.ts[j2] - t0 > w0) stop = true;
          else hit = mpatk_cond(a, m0, MPatKLoader{&a, mid0, m0, j2});
        }
        const uint64_t hb = __ballot(hit), any = __ballot(stop) | hb;
        if (any) {  // (wave-uniform)
          const int f = __builtin_ctzll(any);
          if ((hb >> f) & 1ull) at = p0 + f;
          break;
        }
        p0 += 64;
      }
      if (lane == l) {
        if (at >= 0) {
          const int64_t j2 = mpatk_row(a, at);
          if (m == k - 1) {
            found = a.ordinals ? (int32_t)(a.ordinals[j2] - a.obase) : (int32_t)j2;
            open = false;
          } else {
            mine[m] = (int32_t)j2;
            tref = a.ts[j2];
            ++m;
            pos = at + 1;
          }
        } else {
          open = false;
        }
      }
      mpatk_fence();
      pend = __ballot(open);
    }
    // ---- the result at the e1's place; carry-out: unmatched, and a later event can still bind its next member
    const bool keep = part && found == kSeqNone && a.ts_last - tref <= a.within[m];
    if (v < a.ncp + a.np) {
      a.res[x] = found;
      a.kept[x] = keep ? m : kSeqNone;
    }
    if (keep)
      for (int i = 0; i < m; ++i) {
        const int64_t src = mine[i];
        a.eflag[src < 0 ? -src - 1 : a.ne + src] = 1;
      }
  }
}

struct MPatKCand {
  MSeqSrc s;                // the batch rows' keys
  const int64_t* evt;
  int64_t ne;
  int cw;
  const uint8_t* eflag;     // ne + s.n
  int64_t* cand;            // out: (key, global ordinal, ts, source: batch row or -(carried event row) - 1)
  uint32_t* cand_n;
};

__global__ void __launch_bounds__(kSeqBlock) mpatk_cand_kernel(MPatKCand a) {
  const int64_t e = (int64_t)blockIdx.x * kSeqBlock + threadIdx.x;
  const bool out = e < a.ne + a.s.n && a.eflag[e] != 0;
  const uint32_t slot = seq_wave_slot(out, a.cand_n);
  if (!out) return;
  int64_t* c = a.cand + 4 * (int64_t)slot;
  if (e < a.ne) {
    const int64_t* r = a.evt + e * a.cw;
    c[0] = r[0];
    c[1] = r[1];
    c[2] = r[2];
    c[3] = -e - 1;
  } else {
    const int64_t j = e - a.ne;
    c[0] = mseq_key(a.s, a.s.sid[j], j);
    c[1] = a.s.ordinals ? a.s.ordinals[j] : a.s.obase + j;
    c[2] = a.s.ts[j];
    c[3] = j;
  }
}

// the global ordinal of a member source
__device__ __forceinline__ int64_t mpatk_ordinal(int64_t src, const int64_t* ordinals, int64_t obase, const int64_t* evt,
                                                 int cw) {
  return src < 0 ? evt[(-src - 1) * cw + 1] : ordinals ? ordinals[src] : obase + src;
}

// this thread's kSeqItems consecutive entries of `flags`: the exclusive rank of its first entry that is not kSeqNone
// among the tile's, plus offsets[tile]
__device__ __forceinline__ uint32_t mpatk_rank(const int32_t (&v)[kSeqItems], const uint32_t* offsets, uint32_t* wsum) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t c = 0;
  for (int q = 0; q < kSeqItems; ++q) c += v[q] != kSeqNone;
  const uint32_t inc = wave_incl_scan(c);
  if (lane == 63) wsum[w] = inc;
  lds_barrier();
  uint32_t p = offsets[blockIdx.x] + inc - c;
  for (int q = 0; q < w; ++q) p += wsum[q];
  return p;
}

struct MPatKOut {
  MSeqSrc s;
  const int32_t* flags;     // kept (parts) or res (emit): ncp + s.n entries
  int64_t total, ncp;
  const uint32_t* offsets;  // exclusive scan of seq_count_kernel's tile counts over flags
  const int32_t* mid;
  int k;
  const int64_t* evt;
  int cw;
  const int64_t* parts;     // the carried partials (their keys)
  int64_t* parts_out;       // mpatk_parts_kernel: rows of k + 1 words
  uint32_t* tuples;         // mpatk_emit_kernel: rows of k relative ordinals
};

__global__ void __launch_bounds__(kSeqBlock) mpatk_parts_kernel(MPatKOut a) {
  __shared__ uint32_t wsum[kSeqBlock / 64];
  const int64_t r0 = (int64_t)blockIdx.x * kSeqTile + (int64_t)threadIdx.x * kSeqItems;
  int32_t v[kSeqItems];
  seq_load_items(a.flags, r0, a.total, v);
  uint32_t p = mpatk_rank(v, a.offsets, wsum);
  const int k = a.k, pw = k + 1;
  for (int q = 0; q < kSeqItems; ++q)
    if (v[q] != kSeqNone) {
      const int64_t x = r0 + q;
      int64_t* o = a.parts_out + (int64_t)p * pw;
      const int64_t j = x - a.ncp;
      o[0] = x < a.ncp ? a.parts[x * pw] : mseq_key(a.s, a.s.sid[j], j);
      o[1] = v[q];
      for (int i = 0; i < k - 1; ++i)
        o[2 + i] = i < v[q] ? mpatk_ordinal(a.mid[x * (k - 1) + i], a.s.ordinals, a.s.obase, a.evt, a.cw) : 0;
      ++p;
    }
}

__global__ void __launch_bounds__(kSeqBlock) mpatk_emit_kernel(MPatKOut a) {
  __shared__ uint32_t wsum[kSeqBlock / 64];
  const int64_t r0 = (int64_t)blockIdx.x * kSeqTile + (int64_t)threadIdx.x * kSeqItems;
  int32_t v[kSeqItems];
  seq_load_items(a.flags, r0, a.total, v);
  uint32_t p = mpatk_rank(v, a.offsets, wsum);
  const int k = a.k;
  for (int q = 0; q < kSeqItems; ++q)
    if (v[q] != kSeqNone) {
      const int64_t x = r0 + q;
      uint32_t* o = a.tuples + (int64_t)p * k;
      for (int i = 0; i < k - 1; ++i)
        o[i] = (uint32_t)(int32_t)(mpatk_ordinal(a.mid[x * (k - 1) + i], a.s.ordinals, a.s.obase, a.evt, a.cw) - a.s.obase);
      o[k - 1] = (uint32_t)v[q];
      ++p;
    }
}

// key[x] = member `slot` of tuple idx[x] (idx null: tuple x, and idx_out[x] = x); flip: sign-biased, so that a carried
// member (negative as int32) sorts before every batch row
__global__ void __launch_bounds__(kSeqBlock) mpatk_keys_kernel(const uint32_t* __restrict__ tuples, int k, int slot,
                                                               const uint32_t* __restrict__ idx, int64_t m,
                                                               uint32_t flip, uint32_t* __restrict__ key,
                                                               uint32_t* __restrict__ idx_out) {
  const int64_t x = (int64_t)blockIdx.x * kSeqBlock + threadIdx.x;
  if (x >= m) return;
  const uint32_t t = idx ? idx[x] : (uint32_t)x;
  key[x] = tuples[(int64_t)t * k + slot] ^ flip;
  if (!idx) idx_out[x] = t;
}

__global__ void __launch_bounds__(kSeqBlock) mpatk_tuples_kernel(const uint32_t* __restrict__ tuples, int k,
                                                                 const uint32_t* __restrict__ idx, int64_t m,
                                                                 uint32_t* __restrict__ out) {
  const int64_t x = (int64_t)blockIdx.x * kSeqBlock + threadIdx.x;
  if (x >= m) return;
  const uint32_t* t = tuples + (int64_t)idx[x] * k;
  for (int i = 0; i < k; ++i) out[x * k + i] = t[i];
}

}  // namespace
}  // namespace sm
