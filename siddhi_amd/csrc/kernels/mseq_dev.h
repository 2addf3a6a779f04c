// Device side of the adjacent-run closed form over several streams (seqpath.hip fast_seq_ms):
//   [partition with (ka of A, kb of B, ...)] from every e1=S1[c1], e2=S2[c2(e1, e2)], ..., ek=Sk[ck(e1 .. ek)]
// with 2 <= k <= 8, S1 .. Sk streams of one schema, not all the same, fed as one interleaved batch with a stream index
// per row (sm_app_process_device_events). R = the streams the query reads. The rule of seq_dev.h carries over once
// "the instance's events" are its events on the streams of R: rows of other streams and heartbeat rows (stream -1)
// do not exist for the query, and for every read row j of an instance with k - 1 predecessors i1 < ... < i(k-1) (the
// previous k - 1 read rows of the instance)
//     emit (i1, ..., i(k-1), j)  iff  the row at position m is on stream Sm for every m, c1 .. ck hold and, for every
//                                     e_m written with a within, ts[e_m] - ts[e_(m-1)] <= Tm
// in order of j, at most one output per j. A read row at the wrong position ends the run as a failed condition does.
// A row's instance key is the key attribute of its own stream. tests/test_mseq_plan.py ties this statement to the
// oracle.
//
//   mseq_facts_kernel    one pass over the batch, in tiles of kSeqTile rows (a workgroup walks several): read rows per
//                        tile, and over the read rows the key range, the range of event times and of relative ordinals,
//                        event time or ordinals that do not increase from one read row to the next (the previous read
//                        row: the lanes to the left in the wave, else the wave looks back 64 rows at a time)
//   mseq_pack_kernel     after the exclusive scan of the tile counts: the read rows in row order as (key - kmin, row)
//                        sort pairs, and their stream as one byte per packed position
//   mseq_streams_kernel  keyed: the stream byte of every sorted position, gathered once after the key sort
//   mseq_link_kernel     one lane per packed row in (key, arrival) order, as seqk_link_kernel: the k stream bytes first
//                        (neighbouring bytes), then the withins, then c1 .. ck. Writes hit and predecessor link at the
//                        row (the hit bytes of rows that are not read are zeroed by the host) and the carry-out
//                        candidates: the last k - 1 read rows of every run
// Keep, count and emit are seq_dev.h's seqk kernels. A carried row has one word more than theirs, last: its stream.
// Every wave operation is convergent, so the source also runs under the host wave emulator (tests/native/mseq_emu.cpp).
#pragma once
#include "seq_dev.h"

namespace sm {
namespace {

constexpr int kMSeqStreams = 64;  // app streams a batch may name (one bit each)

struct MSeqSrc {
  int64_t n;                         // rows of the interleaved batch
  const int32_t* sid;                // stream of each row (-1: heartbeat)
  uint64_t read;                     // bit s: the query reads app stream s
  const void* kcol[kMSeqStreams];    // key column of stream s (all nullptr: unpartitioned)
  uint64_t wide;                     // bit s: that column is 64-bit
  const int64_t* ts;
  const int64_t* ordinals;           // or nullptr: obase + row
  int64_t obase;
};

// every range as a pair of maxima (sign-biased values; the minimum as the maximum of the complement), zero-initialised
struct MSeqFacts {
  unsigned long long kmin_c, kmax;
  unsigned long long tmin_c, tmax;
  unsigned long long omin_c, omax;   // ordinals relative to obase
  unsigned long long nread;
  unsigned int bad_ts, bad_ord, bad_carry, pad;
};

__device__ __forceinline__ bool mseq_read(const MSeqSrc& s, int32_t sid) {
  return sid >= 0 && sid < kMSeqStreams && ((s.read >> sid) & 1ull);
}

__device__ __forceinline__ int64_t mseq_key(const MSeqSrc& s, int32_t sid, int64_t row) {
  const void* c = s.kcol[sid];
  if (!c) return 0;
  return (s.wide >> sid) & 1ull ? ((const int64_t*)c)[row] : (int64_t)((const int32_t*)c)[row];
}

__device__ __forceinline__ unsigned long long mseq_wave_max(unsigned long long v) {
  const int lane = threadIdx.x & 63;
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long x = __shfl(v, lane ^ o, 64);
    v = x > v ? x : v;
  }
  return v;
}

// ntiles tiles of kSeqTile rows over gridDim.x workgroups (tile t to workgroup t % gridDim.x): the ranges stay in
// registers from tile to tile and reach memory once per workgroup, so the atomics on the seven words of `f` do not
// grow with the batch
__global__ void __launch_bounds__(kSeqBlock) mseq_facts_kernel(MSeqSrc s, int64_t ntiles, uint32_t* __restrict__ tile_n,
                                                               MSeqFacts* __restrict__ f) {
  constexpr int kWaves = kSeqBlock / 64;
  __shared__ uint32_t wsum[kWaves];
  __shared__ unsigned long long wmax[kWaves][6];
  __shared__ uint32_t wbad[kWaves][2];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  constexpr unsigned long long kBias = 0x8000000000000000ull;
  unsigned long long kmin_c = 0, kmax = 0, tmin_c = 0, tmax = 0, omin_c = 0, omax = 0;
  bool bts = false, bord = false;
  unsigned long long total = 0;  // (thread 0's: the workgroup's read rows)
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    uint32_t cnt = 0;
    for (int it = 0; it < kSeqItems; ++it) {
      const int64_t i = tile * kSeqTile + it * kSeqBlock + threadIdx.x;
      int32_t sd = -1;
      if (i < s.n) sd = s.sid[i];
      const bool rd = i < s.n && mseq_read(s, sd);
      const uint64_t m = __ballot(rd);
      // the previous read row: to the left in the wave, else the wave looks back 64 rows at a time (wave-uniform loop)
      const uint64_t below = m & ((1ull << lane) - 1ull);
      int64_t p = -1;
      if (below) p = i - lane + (63 - __builtin_clzll(below));
      if (m) {
        int64_t base = i - lane - 64, found = -1;
        while (found < 0 && base + 63 >= 0) {
          const int64_t r = base + lane;
          const uint64_t mm = __ballot(r >= 0 && mseq_read(s, s.sid[r]));
          if (mm) found = base + 63 - __builtin_clzll(mm);
          base -= 64;
        }
        if (!below) p = found;
      }
      if (rd) {
        const unsigned long long key = (unsigned long long)mseq_key(s, sd, i) ^ kBias;
        const int64_t t = s.ts[i];
        const int64_t o = s.ordinals ? s.ordinals[i] - s.obase : i;
        if (p >= 0) {
          bts |= t < s.ts[p];
          if (s.ordinals) bord |= s.ordinals[i] <= s.ordinals[p];
        }
        const unsigned long long tb = (unsigned long long)t ^ kBias, ob = (unsigned long long)o ^ kBias;
        kmin_c = ~key > kmin_c ? ~key : kmin_c;
        kmax = key > kmax ? key : kmax;
        tmin_c = ~tb > tmin_c ? ~tb : tmin_c;
        tmax = tb > tmax ? tb : tmax;
        omin_c = ~ob > omin_c ? ~ob : omin_c;
        omax = ob > omax ? ob : omax;
      }
      cnt += (uint32_t)__popcll(m);
    }
    if (lane == 0) wsum[w] = cnt;
    lds_barrier();
    if (threadIdx.x == 0) {
      uint32_t t = 0;
      for (int q = 0; q < kWaves; ++q) t += wsum[q];
      tile_n[tile] = t;
      total += t;
    }
    lds_barrier();  // wsum is read before the next tile writes it
  }
  kmin_c = mseq_wave_max(kmin_c);
  kmax = mseq_wave_max(kmax);
  tmin_c = mseq_wave_max(tmin_c);
  tmax = mseq_wave_max(tmax);
  omin_c = mseq_wave_max(omin_c);
  omax = mseq_wave_max(omax);
  const bool any_ts = __any(bts), any_ord = __any(bord);
  if (lane == 0) {
    wmax[w][0] = kmin_c;
    wmax[w][1] = kmax;
    wmax[w][2] = tmin_c;
    wmax[w][3] = tmax;
    wmax[w][4] = omin_c;
    wmax[w][5] = omax;
    wbad[w][0] = any_ts;
    wbad[w][1] = any_ord;
  }
  lds_barrier();
  if (threadIdx.x == 0 && total) {  // (a flag is only set next to a read row)
    unsigned long long v[6] = {0, 0, 0, 0, 0, 0};
    uint32_t bad_ts = 0, bad_ord = 0;
    for (int q = 0; q < kWaves; ++q) {
      for (int c = 0; c < 6; ++c) v[c] = wmax[q][c] > v[c] ? wmax[q][c] : v[c];
      bad_ts |= wbad[q][0];
      bad_ord |= wbad[q][1];
    }
    atomicMax(&f->kmin_c, v[0]);
    atomicMax(&f->kmax, v[1]);
    atomicMax(&f->tmin_c, v[2]);
    atomicMax(&f->tmax, v[3]);
    atomicMax(&f->omin_c, v[4]);
    atomicMax(&f->omax, v[5]);
    atomicAdd(&f->nread, total);
    if (bad_ts) atomicOr(&f->bad_ts, 1u);
    if (bad_ord) atomicOr(&f->bad_ord, 1u);
  }
}

struct MSeqPack {
  MSeqSrc s;
  const uint32_t* tile_off;  // exclusive scan of the tiles' read rows
  int64_t kmin;
  void* pkey;                // out: key - kmin of each packed position (K), or nullptr: unpartitioned
  uint32_t* prow;            // out: its row
  uint8_t* pstr;             // out: its stream, or nullptr (keyed: gathered after the sort)
};

template <typename K>
__global__ void __launch_bounds__(kSeqBlock) mseq_pack_kernel(MSeqPack a) {
  __shared__ uint32_t wcnt[kSeqItems][kSeqBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  bool rd[kSeqItems];
  int32_t sd[kSeqItems];
  uint32_t rank[kSeqItems];
  for (int it = 0; it < kSeqItems; ++it) {
    const int64_t i = (int64_t)blockIdx.x * kSeqTile + it * kSeqBlock + threadIdx.x;
    sd[it] = i < a.s.n ? a.s.sid[i] : -1;
    rd[it] = i < a.s.n && mseq_read(a.s, sd[it]);
    const uint64_t m = __ballot(rd[it]);
    rank[it] = lanes_below(m);
    if (lane == 0) wcnt[it][w] = (uint32_t)__popcll(m);
  }
  lds_barrier();
  uint32_t p = a.tile_off[blockIdx.x];
  for (int it = 0; it < kSeqItems; ++it) {
    uint32_t mine = p + rank[it];
    for (int q = 0; q < kSeqBlock / 64; ++q) {
      if (q < w) mine += wcnt[it][q];
      p += wcnt[it][q];
    }
    if (rd[it]) {
      const int64_t i = (int64_t)blockIdx.x * kSeqTile + it * kSeqBlock + threadIdx.x;
      a.prow[mine] = (uint32_t)i;
      if (a.pstr) a.pstr[mine] = (uint8_t)sd[it];
      if (a.pkey) ((K*)a.pkey)[mine] = (K)((uint64_t)mseq_key(a.s, sd[it], i) - (uint64_t)a.kmin);
    }
  }
}

__global__ void __launch_bounds__(kSeqBlock) mseq_streams_kernel(const uint32_t* __restrict__ perm,
                                                                 const int32_t* __restrict__ sid, int64_t np,
                                                                 uint8_t* __restrict__ sstr) {
  const int64_t u = (int64_t)blockIdx.x * kSeqBlock + threadIdx.x;
  if (u < np) sstr[u] = (uint8_t)sid[perm[u]];
}

struct MSeqArgs {
  SeqKArgs q;               // n = packed rows; perm / skey over packed positions (perm null: every row is read, unkeyed);
                            // carry rows of q.cw words, the last one the row's stream; prev / hit by batch row
  const uint8_t* sstr;      // stream of each packed position, or nullptr: sid[position]
  const int32_t* sid;
  uint8_t want[kSeqKMax];   // S1 .. Sk
};

template <typename K>
__global__ void __launch_bounds__(kSeqBlock) mseq_link_kernel(MSeqArgs a) {
  const SeqKArgs& q = a.q;
  const K* skey = (const K*)q.skey;
  const int k = q.k;
  for (int it = 0; it < kSeqItems; ++it) {
    const int64_t u = (int64_t)blockIdx.x * kSeqTile + it * kSeqBlock + threadIdx.x;
    const bool live = u < q.n;
    bool out = false;
    int64_t j = 0, key = 0;
    if (live) {
      j = q.perm ? (int64_t)q.perm[u] : u;
      const K kk = skey ? skey[u] : (K)0;
      key = q.kmin + (int64_t)kk;
      int b = 0;  // predecessors inside the batch (at most k - 1)
      while (b < k - 1 && u - b - 1 >= 0 && (!skey || skey[u - b - 1] == kk)) ++b;
      // the streams of the members inside the batch (slots k - 1 - b .. k - 1): most lanes leave here
      bool hit = true;
      for (int d = 0; hit && d <= b; ++d)
        hit = (a.sstr ? (int32_t)a.sstr[u - d] : a.sid[u - d]) == (int32_t)a.want[k - 1 - d];
      SeqKLoader ld{&q, u, k - 1 - b, 0};
      int32_t prev = kSeqNone;
      bool have = b == k - 1;
      if (b > 0) prev = (int32_t)(q.perm ? q.perm[u - 1] : (uint32_t)(u - 1));
      if (!have && q.nc > 0 && (hit || b == 0)) {  // a run's head links to the carry whether or not it hits
        int64_t c_first, c_end;
        seqk_carry_run(q.carry, q.nc, q.cw, key, &c_first, &c_end);
        if (b == 0 && c_end > c_first) prev = (int32_t)(-c_end);  // the key's newest carried row c_end - 1
        have = c_end - c_first >= ld.nfc;
        ld.c0 = c_end - ld.nfc;
        for (int m = 0; hit && have && m < ld.nfc; ++m)
          hit = q.carry[(ld.c0 + m) * q.cw + q.cw - 1] == (int64_t)a.want[m];
      }
      hit = hit && have;
      for (int m = 1; hit && m < k; ++m)
        if (q.within[m] >= 0) hit = ld.ts(m) - ld.ts(m - 1) <= q.within[m];
      for (int m = 0; hit && m < k; ++m)
        if (q.len[m] > 0) hit = truthy(eval_prog(q.code + q.off[m], q.len[m], q.consts, ld));
      q.prev[j] = prev;
      q.hit[j] = hit ? 1 : 0;
      // one of the last k - 1 rows of its run
      out = u + (k - 1) >= q.n || (skey && skey[u + (k - 1)] != kk);
    }
    const uint32_t slot = seq_wave_slot(out, q.cand_n);
    if (out) {
      int64_t* c = q.cand + 4 * (int64_t)slot;
      c[0] = key;
      c[1] = q.ordinals ? q.ordinals[j] : q.obase + j;
      c[2] = q.ts[j];
      c[3] = j;
    }
  }
}

}  // namespace
}  // namespace sm
