// Device side of the closed form of the logical absent over up to three streams of one schema (seqpath.hip
// fast_pat_nand):
//   @app:playback [partition with (ka of A, kb of B, kc of C)]
//   from every e1=A[c1] -> not B[c2] and e3=C[c3(e1, e3)] within T      (or `e3=C[c3] and not B[c2]`)
// B is not C; A may be B, and A may be C; c2 reads the B event and constants only. Fed as one interleaved batch with a
// stream index per row (sm_app_process_device_events). R = {A, B, C}. Take the rows of a partition instance whose stream
// is in R, in arrival order (a row's instance key is the key attribute of its own stream; unpartitioned: all such rows);
// rows of other streams and heartbeat rows (stream -1) do not exist for the query. For every A row i with c1(i), let
//     j*(i) = min { j > i : stream[j] = C, same instance, c3(i, j) }
//     b(i)  = min { j > i : stream[j] = B, same instance, c2(j) }
// The query emits (i, j*(i)) iff j* exists, ts[j*] - ts[i] <= T, and b(i) does not exist or b(i) > j*(i); in order of
// (j*, i), with the timestamp of j*. Emitting or not, the partial ends at j*: after a cancelling B the first passing C
// removes it silently, so a dead partial is never carried. A partial is open at the end of a batch iff it has no j* yet,
// no b yet, and ts_last - ts[i] <= T. No timer, no due position, no creation order of instances: one C row fires one
// instance only. tests/test_pat_nand_plan.py ties this statement to the oracle.
//
// Facts, pack, the stable key sort and the stream byte of every sorted position are mseq_dev.h's, with R = {A, B, C};
// the next cancelling row of every sorted position is absent_dev.h's count scan (absent_flag_kernel, absent_chunk_kernel,
// absent_next_kernel, unchanged): with F the cancelling positions in sorted order and cnt(s) their number at or before
// s, the first one strictly after s is F[cnt(s)] iff that position has s's key.
//   pnand_link_kernel  mpat_link_kernel's shape: one lane per carried row and per sorted position, kMPatBudget positions
//                      on the lane's own, then the whole wave finishes the open scans one at a time, 64 consecutive
//                      sorted positions per ballot step. Each partial's scan has a third stop besides the end of the
//                      key run and the window: its cancel bound. Inside a key run sorted-position order is arrival
//                      order, so positions compare directly. A batch partial at sorted position s is bound by
//                      F[cnt(s)] (cnt counts s itself when A = B and the row passes c2: strictly after). A carried row
//                      is bound by the first cancelling position at or after the head h of its key's run:
//                      F[cnt(h) - flag(h)], which is h itself when the head is a cancelling row. A scan that reaches its
//                      bound ends dead: no output, no carry. B is not C, so the bound itself is never a candidate e3.
//                      The result, e3's relative ordinal or kSeqNone, is written at the e1's own place (res[c] for
//                      carried row c, res[nc + row] for a batch row), so the order of emission is the order of e1. The
//                      carry-out candidates are the open partials; one atomic per wave, no result depends on the order
//                      of atomics.
// Count, scan, emission and the (e3, e1) order are seq_count_kernel, mpat_emit_kernel and mpat_pairs_kernel.
// Every wave operation is convergent, so the source also runs under the host wave emulator
// (tests/native/pat_nand_emu.cpp).
#pragma once
#include "absent_dev.h"
#include "mpat_dev.h"

namespace sm {
namespace {

struct PNandArgs {
  MPatArgs m;               // sa = e1's stream, sb = e3's; c1 and c3 as mpat's c1 and c2; within >= 0
  const uint8_t* fl;        // by sorted position: a cancelling row (stream B and c2)
  const uint32_t* rk;       // by row: cancelling positions at or before the row's sorted position
  const uint32_t* F;        // the cancelling positions in sorted order
  const uint32_t* nf;       // their number (the count scan's total)
};

constexpr int64_t kPNandNoBound = INT64_MAX;

template <typename K>
__global__ void __launch_bounds__(kSeqBlock) pnand_link_kernel(PNandArgs pa) {
  const MPatArgs& a = pa.m;
  const K* skey = (const K*)a.skey;
  const int lane = threadIdx.x & 63;
  const Cond c1 = make_cond(a.code + a.c1_off, a.c1_len, a.consts);
  const Cond c3 = make_cond(a.code + a.c2_off, a.c2_len, a.consts);
  const uint32_t nf = *pa.nf;
  for (int it = 0; it < kSeqItems; ++it) {
    const int64_t v = (int64_t)blockIdx.x * kSeqTile + it * kSeqBlock + threadIdx.x;
    bool part = false, open = false, dead = false;
    int64_t pos = 0, t1 = 0, src = 0, key = 0;
    uint32_t r = nf;  // the bound's place in F
    K kk = (K)0;
    if (v < a.nc) {
      const int64_t* c = a.carry + v * a.cw;
      key = c[0];
      t1 = c[2];
      src = -v - 1;
      part = true;
      if (!skey) {
        open = true;
        r = 0;
      } else if (key >= a.kmin && key <= a.kmax) {  // the head of the key's run, if it has rows here
        kk = (K)((uint64_t)key - (uint64_t)a.kmin);
        int64_t lo = 0, hi = a.np;
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if (skey[mid] < kk) lo = mid + 1;
          else hi = mid;
        }
        pos = lo;
        open = lo < a.np && skey[lo] == kk;
        // the cancelling rows before the head: the head itself cancels a carried partial
        if (open) r = pa.rk[mpat_row(a, lo)] - (uint32_t)pa.fl[lo];
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
        r = pa.rk[j];
      }
    }
    int64_t bound = kPNandNoBound;
    if (open && r < nf) {
      const int64_t uf = (int64_t)pa.F[r];
      if (!skey || skey[uf] == kk) bound = uf;
    }
    int32_t found = kSeqNone;
    // ---- the lane's own budget
    const int64_t stop_at = pos + kMPatBudget;
    while (open && pos < stop_at) {
      if (pos >= bound) {
        open = false;  // cancelled before a C row passed c3
        dead = true;
      } else if (pos >= a.np || (skey && skey[pos] != kk)) {
        open = false;  // the key's rows ran out
      } else if (mpat_stream(a, pos) == a.sb) {
        const int64_t j2 = mpat_row(a, pos);
        if (a.within >= 0 && a.ts[j2] - t1 > a.within) {
          open = false;  // expired
        } else if (eval(c3, SeqPairLoader{a.st, src, j2, src < 0 ? a.carry + (-src - 1) * a.cw : nullptr})) {
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
      const int64_t t0 = __shfl(t1, l, 64), s0 = __shfl(src, l, 64), b0 = __shfl(bound, l, 64);
      const K k0 = (K)__shfl((unsigned long long)kk, l, 64);
      const int64_t* r0 = s0 < 0 ? a.carry + (-s0 - 1) * a.cw : nullptr;
      int64_t at = -1;
      bool cancelled = false;
      for (;;) {
        const int64_t p = p0 + lane;
        bool stop = p >= b0 || p >= a.np || (skey && skey[p] != k0), hit = false;
        if (!stop && mpat_stream(a, p) == a.sb) {
          const int64_t j2 = mpat_row(a, p);
          if (a.within >= 0 && a.ts[j2] - t0 > a.within) stop = true;
          else hit = eval(c3, SeqPairLoader{a.st, s0, j2, r0});
        }
        const uint64_t hb = __ballot(hit), any = __ballot(stop) | hb;
        if (any) {  // (wave-uniform)
          const int f = __builtin_ctzll(any);
          if ((hb >> f) & 1ull) at = p0 + f;
          else cancelled = p0 + f == b0;  // the first stop is the bound, not the window or the run's end
          break;
        }
        p0 += 64;
      }
      if (lane == l) {
        if (at >= 0) {
          const int64_t j2 = mpat_row(a, at);
          found = a.ordinals ? (int32_t)(a.ordinals[j2] - a.obase) : (int32_t)j2;
        }
        dead = cancelled;
        open = false;
      }
      pend = __ballot(open);
    }
    if (v < a.nc) a.res[v] = found;
    else if (v < a.nc + a.np) a.res[a.nc + src] = found;
    // ---- carry-out: no e3 yet, no cancelling row yet, and a later event can still complete it
    const bool out = part && found == kSeqNone && !dead && (a.within < 0 || a.ts_last - t1 <= a.within);
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

}  // namespace
}  // namespace sm
