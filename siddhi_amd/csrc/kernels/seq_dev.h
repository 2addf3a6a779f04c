// Device side of the adjacent-pair closed form (seqpath.hip) of
//   [partition with (k of S)] from every e1=S[c1], e2=S[c2(e1, e2)] [within T]
// A sequence's partial lives for one event: StreamPreStateProcessor.processAndReturn (:274-327) of e2 either
// completes it or leaves it pending, and after each event the sequence receiver clears every state's pending list
// and keeps only what that event created (SequenceMultiProcessStreamReceiver.stabilizeStates :59-61 →
// StateStreamRuntime.resetAndUpdate), while the every back-edge re-arms e1 with the same event. So for every
// event j of a partition instance with a predecessor i (the previous event of the same instance):
//     emit (i, j)  iff  c1(i) and c2(i, j) and (no within, or ts[j] - ts[i] <= T)
// in order of j, and j starts the next partial whether or not it completed one. At most one output per e2.
//
// A header of its own so that the same source also builds on the host under the wave emulator of tests/native/
// (SM_HOST_EMU, hd.h; tests/test_seq_emu.py checks it against a numpy statement of the rule). Every wave operation
// here is convergent: no lane leaves a kernel before its last ballot.
//
//   seq_link_kernel   one lane per event in (key, arrival) order (perm / skey from the stable key sort; row order
//                     and one instance when perm is null): the predecessor is the lane to the left, or for the head
//                     of a key run that key's carried row (binary search in the carry, sorted by key). Writes e1's
//                     relative ordinal or kSeqNone at the e2's row, the carry-out candidate of each run's last event
//                     (if it passes c1) and marks the carried rows whose key had an event. In row order it also
//                     counts its tile's pairs.
//   seq_keep_kernel   carried rows whose key saw no event stay: candidates -(row) - 1.
//   seq_count_kernel  pairs per tile of kSeqTile rows (keyed path: the link ran in key order).
//   seq_emit_kernel   after the exclusive scan of the tile counts: (e1, e2) in row order = the reference's order.
#pragma once
#include "fastpath_dev.h"

namespace sm {
namespace {

constexpr int kSeqBlock = 256;
constexpr int kSeqItems = 4;                      // rows per thread
constexpr int kSeqTile = kSeqBlock * kSeqItems;   // rows per workgroup
constexpr int32_t kSeqNone = INT32_MIN;           // no pair at this e2 (carried e1 ordinals lie above it)

struct SeqArgs {
  int64_t n;
  const int64_t* ts;
  const NfaStream* st;
  const Instr* code;
  const DVal* consts;
  int c1_off, c1_len, c2_off, c2_len;
  int64_t within;           // -1 = none
  const int64_t* ordinals;  // or nullptr: obase + row
  int64_t obase;
  const uint32_t* perm;     // rows in (key, arrival) order, or nullptr: row order, one instance (key 0)
  const void* skey;         // key - kmin of each sorted position (K = uint32_t / uint64_t)
  int64_t kmin;
  const int64_t* carry;     // carried rows [key, global ordinal, ts, attributes], sorted by key; one per key
  int64_t nc;
  int cw;
  int32_t* e1;              // out, by row
  uint8_t* used;            // out, per carried row (zeroed by the host)
  int64_t* cand;            // out: carry-out candidates (key, global ordinal, ts, source row)
  uint32_t* cand_n;
  uint32_t* counts;         // out (row order only): pairs per tile
};

// c2 over (e1 = slot 0, e2 = slot 1); e1 is a batch row or a carried row (canonical attribute words)
struct SeqPairLoader {
  const NfaStream* st;
  int64_t r1, r2;
  const int64_t* c1;
  __device__ StackVal var(const Instr& in) const {
    if (in.op == OP_COL) return col_value(st, in.a, r2);
    if (!(in.b == 0 || in.b == -1)) {  // one-event slots: index 0 / CURRENT only
      StackVal v;
      v.i = 0;
      v.null = 1;
      return v;
    }
    if (in.a == 0 && c1) {
      const int t = st->types[in.c];
      StackVal v = uncanon((uint64_t)c1[3 + in.c], t);
      if (t == T_STRING) v.null = v.i < 0;
      return v;
    }
    return col_value(st, in.c, in.a == 0 ? r1 : r2);
  }
};

// row of `key` in the carry, or -1
__device__ __forceinline__ int64_t seq_carry_find(const int64_t* carry, int64_t nc, int cw, int64_t key) {
  int64_t lo = 0, hi = nc;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (carry[mid * cw] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < nc && carry[lo * cw] == key ? lo : -1;
}

// one slot per set lane of a convergent predicate: one atomic per wave
__device__ __forceinline__ uint32_t seq_wave_slot(bool want, uint32_t* counter) {
  const uint64_t m = __ballot(want);
  uint32_t base = 0;
  if ((threadIdx.x & 63) == 0 && m) base = atomicAdd(counter, (uint32_t)__popcll(m));
  base = __shfl(base, 0, 64);
  return base + lanes_below(m);
}

template <typename K>
__global__ void __launch_bounds__(kSeqBlock) seq_link_kernel(SeqArgs a) {
  __shared__ uint32_t wsum[kSeqBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const K* skey = (const K*)a.skey;
  const Cond c1 = make_cond(a.code + a.c1_off, a.c1_len, a.consts);
  const Cond c2 = make_cond(a.code + a.c2_off, a.c2_len, a.consts);
  uint32_t cnt = 0;
  for (int it = 0; it < kSeqItems; ++it) {
    const int64_t u = (int64_t)blockIdx.x * kSeqTile + it * kSeqBlock + threadIdx.x;
    const bool live = u < a.n;
    bool hit = false, out = false;
    int64_t j = 0, key = 0, tj = 0;
    if (live) {
      j = a.perm ? (int64_t)a.perm[u] : u;
      const K k = skey ? skey[u] : (K)0;
      key = a.kmin + (int64_t)k;
      tj = a.ts[j];
      const bool head = u == 0 || (skey && skey[u - 1] != k);
      const bool tail = u == a.n - 1 || (skey && skey[u + 1] != k);
      int32_t e1 = kSeqNone;
      if (!head) {
        const int64_t i = a.perm ? (int64_t)a.perm[u - 1] : u - 1;
        if (eval(c1, RowLoader{a.st, i}) && (a.within < 0 || tj - a.ts[i] <= a.within) &&
            eval(c2, SeqPairLoader{a.st, i, j, nullptr})) {
          e1 = a.ordinals ? (int32_t)(a.ordinals[i] - a.obase) : (int32_t)i;
          hit = true;
        }
      } else if (a.nc > 0) {
        const int64_t c = seq_carry_find(a.carry, a.nc, a.cw, key);
        if (c >= 0) {  // a carried row passed c1 when it was kept
          const int64_t* r = a.carry + c * a.cw;
          a.used[c] = 1;
          if ((a.within < 0 || tj - r[2] <= a.within) && eval(c2, SeqPairLoader{a.st, -1, j, r})) {
            e1 = (int32_t)(r[1] - a.obase);
            hit = true;
          }
        }
      }
      a.e1[j] = e1;
      out = tail && eval(c1, RowLoader{a.st, j});
    }
    const uint32_t slot = seq_wave_slot(out, a.cand_n);
    if (out) {
      int64_t* c = a.cand + 4 * (int64_t)slot;
      c[0] = key;
      c[1] = a.ordinals ? a.ordinals[j] : a.obase + j;
      c[2] = tj;
      c[3] = j;
    }
    cnt += (uint32_t)__popcll(__ballot(hit));
  }
  if (a.counts) {  // row order: this tile's rows are the emit kernel's tile
    if (lane == 0) wsum[w] = cnt;
    lds_barrier();
    if (threadIdx.x == 0) {
      uint32_t s = 0;
      for (int k = 0; k < kSeqBlock / 64; ++k) s += wsum[k];
      a.counts[blockIdx.x] = s;
    }
  }
}

__global__ void __launch_bounds__(kSeqBlock) seq_keep_kernel(const int64_t* __restrict__ carry, int64_t nc, int cw,
                                                             const uint8_t* __restrict__ used,
                                                             int64_t* __restrict__ cand, uint32_t* __restrict__ cand_n) {
  const int64_t c = (int64_t)blockIdx.x * kSeqBlock + threadIdx.x;
  const bool keep = c < nc && !used[c];
  const uint32_t slot = seq_wave_slot(keep, cand_n);
  if (keep) {
    const int64_t* r = carry + c * cw;
    int64_t* o = cand + 4 * (int64_t)slot;
    o[0] = r[0];
    o[1] = r[1];
    o[2] = r[2];
    o[3] = -c - 1;
  }
}

// the thread's kSeqItems consecutive rows of e1 (one 16-byte load inside the batch)
__device__ __forceinline__ void seq_load_items(const int32_t* __restrict__ e1, int64_t r0, int64_t n,
                                               int32_t (&v)[kSeqItems]) {
  static_assert(kSeqItems == 4, "one 16-byte load per thread");
  if (r0 + kSeqItems <= n) {
    const uint4 x = *(const uint4*)(e1 + r0);
    v[0] = (int32_t)x.x;
    v[1] = (int32_t)x.y;
    v[2] = (int32_t)x.z;
    v[3] = (int32_t)x.w;
  } else {
    for (int k = 0; k < kSeqItems; ++k) v[k] = r0 + k < n ? e1[r0 + k] : kSeqNone;
  }
}

__global__ void __launch_bounds__(kSeqBlock) seq_count_kernel(const int32_t* __restrict__ e1, int64_t n,
                                                              uint32_t* __restrict__ counts) {
  __shared__ uint32_t wsum[kSeqBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int32_t v[kSeqItems];
  seq_load_items(e1, (int64_t)blockIdx.x * kSeqTile + (int64_t)threadIdx.x * kSeqItems, n, v);
  uint32_t cnt = 0;
  for (int k = 0; k < kSeqItems; ++k) cnt += (uint32_t)__popcll(__ballot(v[k] != kSeqNone));
  if (lane == 0) wsum[w] = cnt;
  lds_barrier();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int k = 0; k < kSeqBlock / 64; ++k) s += wsum[k];
    counts[blockIdx.x] = s;
  }
}

// offsets = exclusive scan of the tile counts; pairs[2 m] = e1, pairs[2 m + 1] = e2, relative to obase
__global__ void __launch_bounds__(kSeqBlock) seq_emit_kernel(const int32_t* __restrict__ e1, int64_t n,
                                                             const uint32_t* __restrict__ offsets,
                                                             const int64_t* __restrict__ ordinals, int64_t obase,
                                                             uint32_t* __restrict__ pairs) {
  __shared__ uint32_t wsum[kSeqBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * kSeqTile + (int64_t)threadIdx.x * kSeqItems;
  int32_t v[kSeqItems];
  seq_load_items(e1, r0, n, v);
  uint32_t c = 0;
  for (int k = 0; k < kSeqItems; ++k) c += v[k] != kSeqNone;
  const uint32_t inc = wave_incl_scan(c);
  if (lane == 63) wsum[w] = inc;
  lds_barrier();
  uint32_t p = offsets[blockIdx.x] + inc - c;
  for (int k = 0; k < w; ++k) p += wsum[k];
  for (int k = 0; k < kSeqItems; ++k)
    if (v[k] != kSeqNone) {
      const int64_t j = r0 + k;
      pairs[2 * (int64_t)p] = (uint32_t)v[k];
      pairs[2 * (int64_t)p + 1] = ordinals ? (uint32_t)(ordinals[j] - obase) : (uint32_t)j;
      ++p;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The adjacent-run closed form of the k-state sibling (3 <= k <= 8, seqpath.hip fast_seq_k):
//   [partition with (key of S)] from every e1=S[c1], e2=S[c2(e1, e2)], ..., ek=S[ck(e1 .. ek)]   (within Tm on e_m)
// The same life of one event per partial holds at every state, so for every event j of an instance with k - 1
// predecessors i1 < ... < i(k-1) (the previous k - 1 events of the instance):
//     emit (i1, ..., i(k-1), j)  iff  c1(i1), c2(i1, i2), ..., ck(i1 .. j) and, for every e_m written with a within,
//                                     ts[e_m] - ts[e_(m-1)] <= Tm
// in order of j, at most one output per j. tests/test_seqk_plan.py ties this statement to the oracle.
//
//   seqk_link_kernel   one lane per event in (key, arrival) order. Its k - 1 predecessors are the lanes to its left
//                      while the key matches; the first k - 1 rows of a run take the missing ones from the tail of
//                      their key's carried rows (binary search of the key's run in the carry, sorted by (key,
//                      ordinal)). Writes, at the event's row, hit or none and its predecessor: a batch row, or the
//                      carried row c as -c - 1, or kSeqNone. The emit pass rebuilds a tuple by chasing the predecessor
//                      k - 1 times (a carried row's predecessor is the carried row before it). Also the carry-out
//                      candidates: the last min(k - 1, run length) rows of every run.
//   seqk_keep_kernel   carried rows that stay: all of a key without events, the newest k - 1 - e of a key with e < k - 1
//                      events (e from a binary search of the sorted batch keys). No marks, no order of atomics read.
//   seqk_count_kernel  hits per tile of kSeqTile rows.
//   seqk_emit_kernel   after the exclusive scan of the tile counts: k-tuples in row order of j.
constexpr int kSeqKMax = 8;

struct SeqKArgs {
  int64_t n;
  const int64_t* ts;
  const NfaStream* st;
  const Instr* code;
  const DVal* consts;
  int k;
  int off[kSeqKMax], len[kSeqKMax];  // condition program of element m (state context, slots 0 .. m)
  int64_t within[kSeqKMax];          // of element m against element m - 1, -1 = none
  const int64_t* ordinals;           // or nullptr: obase + row
  int64_t obase;
  const uint32_t* perm;              // rows in (key, arrival) order, or nullptr: row order, one instance (key 0)
  const void* skey;                  // key - kmin of each sorted position (K = uint32_t / uint64_t)
  int64_t kmin, kmax;
  const int64_t* carry;              // carried rows [key, global ordinal, ts, attributes], sorted by (key, ordinal)
  int64_t nc;
  int cw;
  int32_t* prev;                     // out, by row
  uint8_t* hit;                      // out, by row (n rounded up to 4 bytes)
  int64_t* cand;                     // out: carry-out candidates (key, global ordinal, ts, source row)
  uint32_t* cand_n;
};

// [first, end) of `key`'s rows in the carry
__device__ __forceinline__ void seqk_carry_run(const int64_t* carry, int64_t nc, int cw, int64_t key, int64_t* first,
                                               int64_t* end) {
  int64_t lo = 0, hi = nc;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (carry[mid * cw] < key) lo = mid + 1;
    else hi = mid;
  }
  *first = lo;
  hi = nc;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (carry[mid * cw] <= key) lo = mid + 1;
    else hi = mid;
  }
  *end = lo;
}

// The k events of one candidate tuple: slot m < nfc is the carried row c0 + m, slot m >= nfc the sorted position
// u - (k - 1 - m) of the batch. Programs read slots at index 0 / CURRENT only (one event per slot).
struct SeqKLoader {
  const SeqKArgs* a;
  int64_t u;   // sorted position of the last event (slot k - 1)
  int nfc;     // members from the carry
  int64_t c0;  // carried row of slot 0 (nfc > 0)
  __device__ __forceinline__ int64_t row(int m) const {
    const int64_t p = u - (a->k - 1 - m);
    return a->perm ? (int64_t)a->perm[p] : p;
  }
  __device__ __forceinline__ int64_t ts(int m) const {
    return m < nfc ? a->carry[(c0 + m) * a->cw + 2] : a->ts[row(m)];
  }
  __device__ StackVal var(const Instr& in) const {
    if (in.op == OP_COL) return col_value(a->st, in.a, row(a->k - 1));  // (refused by the host entry)
    if (!(in.b == 0 || in.b == -1) || in.a < 0 || in.a >= a->k) {
      StackVal v;
      v.i = 0;
      v.null = 1;
      return v;
    }
    if (in.a < nfc) {
      const int t = a->st->types[in.c];
      StackVal v = uncanon((uint64_t)a->carry[(c0 + in.a) * a->cw + 3 + in.c], t);
      if (t == T_STRING) v.null = v.i < 0;
      return v;
    }
    return col_value(a->st, in.c, row(in.a));
  }
};

template <typename K>
__global__ void __launch_bounds__(kSeqBlock) seqk_link_kernel(SeqKArgs a) {
  const K* skey = (const K*)a.skey;
  const int k = a.k;
  for (int it = 0; it < kSeqItems; ++it) {
    const int64_t u = (int64_t)blockIdx.x * kSeqTile + it * kSeqBlock + threadIdx.x;
    const bool live = u < a.n;
    bool out = false;
    int64_t j = 0, key = 0;
    if (live) {
      j = a.perm ? (int64_t)a.perm[u] : u;
      const K kk = skey ? skey[u] : (K)0;
      key = a.kmin + (int64_t)kk;
      int b = 0;  // predecessors inside the batch (at most k - 1)
      while (b < k - 1 && u - b - 1 >= 0 && (!skey || skey[u - b - 1] == kk)) ++b;
      SeqKLoader ld{&a, u, k - 1 - b, 0};
      int32_t prev = kSeqNone;
      bool have = b == k - 1;
      if (b > 0) prev = (int32_t)(a.perm ? a.perm[u - 1] : (uint32_t)(u - 1));
      if (!have && a.nc > 0) {
        int64_t c_first, c_end;
        seqk_carry_run(a.carry, a.nc, a.cw, key, &c_first, &c_end);
        if (b == 0 && c_end > c_first) prev = (int32_t)(-c_end);  // the key's newest carried row c_end - 1
        have = c_end - c_first >= ld.nfc;
        ld.c0 = c_end - ld.nfc;
      }
      bool hit = have;
      for (int m = 1; hit && m < k; ++m)
        if (a.within[m] >= 0) hit = ld.ts(m) - ld.ts(m - 1) <= a.within[m];
      for (int m = 0; hit && m < k; ++m)
        if (a.len[m] > 0) hit = truthy(eval_prog(a.code + a.off[m], a.len[m], a.consts, ld));
      a.prev[j] = prev;
      a.hit[j] = hit ? 1 : 0;
      // one of the last k - 1 rows of its run
      out = u + (k - 1) >= a.n || (skey && skey[u + (k - 1)] != kk);
    }
    const uint32_t slot = seq_wave_slot(out, a.cand_n);
    if (out) {
      int64_t* c = a.cand + 4 * (int64_t)slot;
      c[0] = key;
      c[1] = a.ordinals ? a.ordinals[j] : a.obase + j;
      c[2] = a.ts[j];
      c[3] = j;
    }
  }
}

template <typename K>
__global__ void __launch_bounds__(kSeqBlock) seqk_keep_kernel(SeqKArgs a) {
  const K* skey = (const K*)a.skey;
  const int64_t c = (int64_t)blockIdx.x * kSeqBlock + threadIdx.x;
  bool keep = false;
  if (c < a.nc) {
    const int64_t key = a.carry[c * a.cw];
    int newer = 0;  // carried rows of the key after this one (at most k - 2)
    while (newer < a.k && c + newer + 1 < a.nc && a.carry[(c + newer + 1) * a.cw] == key) ++newer;
    int64_t e = 0;  // the key's events in this batch, counted up to k - 1
    if (!skey) {
      e = a.n;
    } else if (a.n > 0 && key >= a.kmin && key <= a.kmax) {
      const K d = (K)((uint64_t)key - (uint64_t)a.kmin);
      int64_t lo = 0, hi = a.n;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (skey[mid] < d) lo = mid + 1;
        else hi = mid;
      }
      while (e < a.k - 1 && lo + e < a.n && skey[lo + e] == d) ++e;
    }
    keep = (int64_t)newer + e < a.k - 1;
  }
  const uint32_t slot = seq_wave_slot(keep, a.cand_n);
  if (keep) {
    const int64_t* r = a.carry + c * a.cw;
    int64_t* o = a.cand + 4 * (int64_t)slot;
    o[0] = r[0];
    o[1] = r[1];
    o[2] = r[2];
    o[3] = -c - 1;
  }
}

// the thread's kSeqItems consecutive hit bytes (one 4-byte load: the array is padded to a multiple of 4)
__device__ __forceinline__ uint32_t seqk_load_hits(const uint8_t* __restrict__ hit, int64_t r0, int64_t n) {
  static_assert(kSeqItems == 4, "one 4-byte load per thread");
  if (r0 >= n) return 0u;
  uint32_t x = *(const uint32_t*)(hit + r0);
  if (r0 + kSeqItems > n) x &= 0xffffffffu >> (8 * (int)(r0 + kSeqItems - n));
  return x & 0x01010101u;
}

__global__ void __launch_bounds__(kSeqBlock) seqk_count_kernel(const uint8_t* __restrict__ hit, int64_t n,
                                                               uint32_t* __restrict__ counts) {
  __shared__ uint32_t wsum[kSeqBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint32_t x = seqk_load_hits(hit, (int64_t)blockIdx.x * kSeqTile + (int64_t)threadIdx.x * kSeqItems, n);
  const uint32_t inc = wave_incl_scan((uint32_t)__popc(x));
  if (lane == 63) wsum[w] = inc;
  lds_barrier();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int q = 0; q < kSeqBlock / 64; ++q) s += wsum[q];
    counts[blockIdx.x] = s;
  }
}

// offsets = exclusive scan of the tile counts; tuples[k m + s] = relative ordinal of element s of the m-th output
__global__ void __launch_bounds__(kSeqBlock) seqk_emit_kernel(const uint8_t* __restrict__ hit,
                                                              const int32_t* __restrict__ prev, int64_t n, int k,
                                                              const uint32_t* __restrict__ offsets,
                                                              const int64_t* __restrict__ ordinals, int64_t obase,
                                                              const int64_t* __restrict__ carry, int cw,
                                                              uint32_t* __restrict__ tuples) {
  __shared__ uint32_t wsum[kSeqBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * kSeqTile + (int64_t)threadIdx.x * kSeqItems;
  const uint32_t x = seqk_load_hits(hit, r0, n);
  const uint32_t c = (uint32_t)__popc(x);
  const uint32_t inc = wave_incl_scan(c);
  if (lane == 63) wsum[w] = inc;
  lds_barrier();
  uint32_t p = offsets[blockIdx.x] + inc - c;
  for (int q = 0; q < w; ++q) p += wsum[q];
  for (int q = 0; q < kSeqItems; ++q)
    if ((x >> (8 * q)) & 1u) {
      uint32_t* t = tuples + (int64_t)p * k;
      int64_t cur = r0 + q;
      for (int m = k - 1; m >= 0; --m) {  // a hit has its k - 1 predecessors: no link is kSeqNone on the way
        if (cur >= 0) {
          t[m] = ordinals ? (uint32_t)(ordinals[cur] - obase) : (uint32_t)cur;
          if (m > 0) cur = prev[cur];
        } else {
          t[m] = (uint32_t)(int32_t)(carry[(-cur - 1) * cw + 1] - obase);
          cur += 1;  // the carried row before it
        }
      }
      ++p;
    }
}

}  // namespace
}  // namespace sm
