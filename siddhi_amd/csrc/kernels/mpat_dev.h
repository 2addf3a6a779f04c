// Device side of the closed form of the pattern over two streams of one schema (seqpath.hip fast_pat_ms):
//   [partition with (ka of A, kb of B)] from every e1=A[c1] -> e2=B[c2(e1, e2)] within T
// fed as one interleaved batch with a stream index per row (sm_app_process_device_events). R = {A, B}. Take the events
// of a partition instance whose stream is in R, in arrival order (an event's instance key is the key attribute of its
// own stream; unpartitioned: all such events); rows of other streams and heartbeat rows (stream -1) do not exist for
// the query. For every event i on stream A with c1(i), let
//     j*(i) = min { j > i : stream[j] = B, key[j] = key[i], c2(i, j) }
// The query emits (i, j*(i)) iff j* exists and ts[j*] - ts[i] <= T, in order of (j*, i): one e2 may complete many
// partials, oldest e1 first. With event time non-decreasing over the read rows this is "the first B event with c2 inside
// the window": a B event beyond the window removes the partial, and so does every later one.
// tests/test_mpat_plan.py ties this statement to the oracle.
//
// Facts, pack, the stable key sort and the stream byte of every sorted position are mseq_dev.h's, with R = {A, B}.
//   mpat_link_kernel   one lane per carried row and per sorted position. A sorted position on stream A whose row passes
//                      c1 is a partial; so is every carried row (it passed c1 when it was kept), which finds its key's
//                      run by binary search of the sorted batch keys and starts at the run's head. A partial scans
//                      forward inside its key run: the stream byte first (neighbouring bytes, no gather), then the
//                      window (a B event beyond it ends the scan), then c2. A lane scans kMPatBudget positions on its
//                      own; the scans still open are finished one at a time by the whole wave, 64 consecutive sorted
//                      positions per step and one ballot each (fastpath3.hip walk_kernel's unkeyed finish), so a window
//                      of W rows costs W / 64 steps. The result, e2's relative ordinal or kSeqNone, is written at the
//                      e1's own place: res[c] for carried row c, res[nc + row] for a batch row. Emitting `res` in that
//                      order gives the pairs in order of e1 for free (the carried rows of one key are in ordinal order
//                      and precede the batch's), which leaves a stable sort on e2 alone. Also the carry-out
//                      candidates: every unmatched partial that a later event can still complete
//                      (ts_last - ts[i] <= T). One atomic per wave; no result depends on the order of atomics.
//   mpat_emit_kernel   after seq_count_kernel over `res` and the exclusive scan of the tile counts: e2 as sort key and e1
//                      as its value, compacted in order of `res`
//   mpat_pairs_kernel  after the stable sort by e2: the (e1, e2) pairs
// Every wave operation is convergent, so the source also runs under the host wave emulator (tests/native/mpat_emu.cpp).
#pragma once
#include "mseq_dev.h"

namespace sm {
namespace {

// Sorted positions a lane scans before the wave takes the scan over. Measured at 16 / 32 / 64: keyed,
// runs of about a hundred rows, all three are equal; unkeyed with a 1000-row window 16 is the fastest.
#ifndef SM_MPAT_BUDGET
#define SM_MPAT_BUDGET 16
#endif
constexpr int kMPatBudget = SM_MPAT_BUDGET;

struct MPatArgs {
  int64_t np;               // read rows = sorted positions
  int64_t n;                // rows of the batch
  const int64_t* ts;
  const NfaStream* st;
  const Instr* code;
  const DVal* consts;
  int c1_off, c1_len, c2_off, c2_len;
  int64_t within;           // -1 = none
  int64_t ts_last;          // event time of the batch's last read row
  const int64_t* ordinals;  // or nullptr: obase + row
  int64_t obase;
  const uint32_t* perm;     // row of each sorted position, or nullptr: every row is read, unkeyed
  const void* skey;         // key - kmin of each sorted position (K), or nullptr: unpartitioned
  int64_t kmin, kmax;
  const uint8_t* sstr;      // stream of each sorted position, or nullptr: sid[position]
  const int32_t* sid;
  int sa, sb;               // app streams of e1 and e2
  const int64_t* carry;     // carried e1 rows [key, global ordinal, ts, attributes], sorted by (key, ordinal)
  int64_t nc;
  int cw;
  int32_t* res;             // out: nc + n entries (entries of rows that are not read are filled by the host)
  int64_t* cand;            // out: carry-out candidates (key, global ordinal, ts, source: batch row or -(carried row) - 1)
  uint32_t* cand_n;
};

__device__ __forceinline__ int32_t mpat_stream(const MPatArgs& a, int64_t p) {
  return a.sstr ? (int32_t)a.sstr[p] : a.sid[p];
}
__device__ __forceinline__ int64_t mpat_row(const MPatArgs& a, int64_t p) { return a.perm ? (int64_t)a.perm[p] : p; }

template <typename K>
__global__ void __launch_bounds__(kSeqBlock) mpat_link_kernel(MPatArgs a) {
  const K* skey = (const K*)a.skey;
  const int lane = threadIdx.x & 63;
  const Cond c1 = make_cond(a.code + a.c1_off, a.c1_len, a.consts);
  const Cond c2 = make_cond(a.code + a.c2_off, a.c2_len, a.consts);
  for (int it = 0; it < kSeqItems; ++it) {
    const int64_t v = (int64_t)blockIdx.x * kSeqTile + it * kSeqBlock + threadIdx.x;
    bool part = false, open = false;
    int64_t pos = 0, t1 = 0, src = 0, key = 0;
    K kk = (K)0;
    if (v < a.nc) {
      const int64_t* r = a.carry + v * a.cw;
      key = r[0];
      t1 = r[2];
      src = -v - 1;
      part = true;
      if (!skey) {
        open = true;
      } else if (key >= a.kmin && key <= a.kmax) {  // the head of the key's run, if it has events here
        kk = (K)((uint64_t)key - (uint64_t)a.kmin);
        int64_t lo = 0, hi = a.np;
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if (skey[mid] < kk) lo = mid + 1;
          else hi = mid;
        }
        pos = lo;
        open = lo < a.np && skey[lo] == kk;
      }
    } else if (v < a.nc + a.np) {
      const int64_t u = v - a.nc;
      const int64_t j = mpat_row(a, u);
      kk = skey ? skey[u] : (K)0;
      key = a.kmin + (int64_t)kk;
      src = j;
      if (mpat_stream(a, u) == a.sa && eval(c1, RowLoader{a.st, j})) {
        part = open = true;
        t1 = a.ts[j];
        pos = u + 1;
      }
    }
    int32_t found = kSeqNone;
    // ---- the lane's own budget
    const int64_t stop_at = pos + kMPatBudget;
    while (open && pos < stop_at) {
      if (pos >= a.np || (skey && skey[pos] != kk)) {
        open = false;  // the key's events ran out
      } else if (mpat_stream(a, pos) == a.sb) {
        const int64_t j2 = mpat_row(a, pos);
        if (a.within >= 0 && a.ts[j2] - t1 > a.within) {
          open = false;  // expired
        } else if (eval(c2, SeqPairLoader{a.st, src, j2, src < 0 ? a.carry + (-src - 1) * a.cw : nullptr})) {
          found = a.ordinals ? (int32_t)(a.ordinals[j2] - a.obase) : (int32_t)j2;
          open = false;
        }
      }
      if (open) ++pos;
    }
    // ---- wave-cooperative finish of the open scans: one scan at a time, 64 consecutive sorted positions per step
    uint64_t pend = __ballot(open);
    while (pend) {
      const int l = __builtin_ctzll(pend);
      int64_t p0 = __shfl(pos, l, 64);
      const int64_t t0 = __shfl(t1, l, 64), s0 = __shfl(src, l, 64);
      const K k0 = (K)__shfl((unsigned long long)kk, l, 64);
      const int64_t* r0 = s0 < 0 ? a.carry + (-s0 - 1) * a.cw : nullptr;
      int64_t at = -1;
      for (;;) {
        const int64_t p = p0 + lane;
        bool stop = p >= a.np || (skey && skey[p] != k0), hit = false;
        if (!stop && mpat_stream(a, p) == a.sb) {
          const int64_t j2 = mpat_row(a, p);
          if (a.within >= 0 && a.ts[j2] - t0 > a.within) stop = true;
          else hit = eval(c2, SeqPairLoader{a.st, s0, j2, r0});
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
          const int64_t j2 = mpat_row(a, at);
          found = a.ordinals ? (int32_t)(a.ordinals[j2] - a.obase) : (int32_t)j2;
        }
        open = false;
      }
      pend = __ballot(open);
    }
    if (v < a.nc) a.res[v] = found;
    else if (v < a.nc + a.np) a.res[a.nc + src] = found;
    // ---- carry-out: unmatched, and a later event can still complete it
    const bool out = part && found == kSeqNone && (a.within < 0 || a.ts_last - t1 <= a.within);
    const uint32_t slot = seq_wave_slot(out, a.cand_n);
    if (out) {
      int64_t* c = a.cand + 4 * (int64_t)slot;
      c[0] = key;
      c[1] = src < 0 ? a.carry[(-src - 1) * a.cw + 1] : (a.ordinals ? a.ordinals[src] : a.obase + src);
      c[2] = t1;
      c[3] = src;
    }
  }
}

// offsets = exclusive scan of seq_count_kernel's tile counts over res[0 .. total): jkey[m] = e2, ival[m] = e1 of the
// m-th entry that is not kSeqNone, both relative to obase (a carried e1 is negative as int32)
__global__ void __launch_bounds__(kSeqBlock) mpat_emit_kernel(const int32_t* __restrict__ res, int64_t total, int64_t nc,
                                                              const uint32_t* __restrict__ offsets,
                                                              const int64_t* __restrict__ ordinals, int64_t obase,
                                                              const int64_t* __restrict__ carry, int cw,
                                                              uint32_t* __restrict__ jkey, uint32_t* __restrict__ ival) {
  __shared__ uint32_t wsum[kSeqBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * kSeqTile + (int64_t)threadIdx.x * kSeqItems;
  int32_t v[kSeqItems];
  seq_load_items(res, r0, total, v);
  uint32_t c = 0;
  for (int k = 0; k < kSeqItems; ++k) c += v[k] != kSeqNone;
  const uint32_t inc = wave_incl_scan(c);
  if (lane == 63) wsum[w] = inc;
  lds_barrier();
  uint32_t p = offsets[blockIdx.x] + inc - c;
  for (int k = 0; k < w; ++k) p += wsum[k];
  for (int k = 0; k < kSeqItems; ++k)
    if (v[k] != kSeqNone) {
      const int64_t x = r0 + k;
      jkey[p] = (uint32_t)v[k];
      if (x < nc) ival[p] = (uint32_t)(int32_t)(carry[x * cw + 1] - obase);
      else ival[p] = ordinals ? (uint32_t)(ordinals[x - nc] - obase) : (uint32_t)(x - nc);
      ++p;
    }
}

__global__ void __launch_bounds__(kSeqBlock) mpat_pairs_kernel(const uint32_t* __restrict__ jkey,
                                                               const uint32_t* __restrict__ ival, int64_t m,
                                                               uint32_t* __restrict__ pairs) {
  const int64_t x = (int64_t)blockIdx.x * kSeqBlock + threadIdx.x;
  if (x < m) ((uint2*)pairs)[x] = make_uint2(ival[x], jkey[x]);
}

}  // namespace
}  // namespace sm
