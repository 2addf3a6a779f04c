// Key pass 0 of the keyed fast path (round 3): the stable 1024-way scatter of 16-byte keyed records by the key's
// low digit, built from the original columns (Src: OrigSrc in fastpath3.hip). Same pass semantics and the same
// write-combining as downsweep_wc_kernel<0> (fastpath3.hip: a tile stores only records whose 64-byte segment of the
// output completes in this chunk; the < 4 records left of a digit's run are carried in LDS to the next tile and the
// chunk's last tile flushes them), with less LDS traffic per record:
//   * per (digit, wave) counts are one 32-byte row per digit ([digit][wave] u16): a digit's tile count and the
//     records of its earlier waves come from two 16-byte reads and packed 16-bit dot products, where the old layout
//     walked the 16 waves per digit with 32 LDS operations;
//   * the record moves through LDS once (16-byte slots, 64 KB per 4096-record tile) instead of as two 8-byte halves.
// A header of its own so the kernel also runs under the host wave emulator (tests/native/pass0_emu.cpp).
//
// Time-order check (optional, Src::kTimeOrder): the pass also answers "is the 64-bit event time non-decreasing over
// the whole batch", from the timestamps it loads for the records anyway, so that prep need not read the time column
// for it. A source that asks for it supplies time_of(raw) (the event's timestamp), time0() (the batch's first),
// time_at(p) (a global load, used for the one event before the chunk) and time_bad() (raises the device flag).
// With rel = ts - time0() in 64 bits, an event is out of order when rel >> 32 != 0 (before the batch's first event,
// or 2^32 or more after it: the caller has checked that the batch's last event is not, so some later event is
// earlier) or when its low word is below its predecessor's; with every high word zero the low words compare as the
// times do. The predecessor of an event is lane - 1 of the same wave-item (one DPP move), lane 63 of the wave's item
// before (v_readlane), the wave before's last event (one LDS word per wave) or the last event of the tile before
// (two more LDS words, by tile parity; seeded with the event before the chunk).
#pragma once
#include <type_traits>

#include "fastpath_dev.h"

namespace sm {
namespace {

constexpr int kP0Block = 1024;               // threads; thread d owns digit d in the per-digit steps
constexpr int kP0Waves = kP0Block / 64;      // 16: one u16 count per wave in a digit's 32-byte row
constexpr int kP0Items = 4;                  // records per thread per tile
constexpr int kP0Tile = kP0Block * kP0Items;  // 4096
constexpr int kP0Seg = 4;                    // records per 64-byte output segment
static_assert(kBins == kP0Block && kP0Waves == 16, "one digit per thread, 16 waves");

__device__ __forceinline__ uint32_t sm_udot2(uint32_t a, uint32_t b, uint32_t c) {  // sum of u16 products + c
#if defined(__HIP_DEVICE_COMPILE__)
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b), c, false);
#else
  return c + (a & 0xffffu) * (b & 0xffffu) + (a >> 16) * (b >> 16);
#endif
}

// sum of the u16 counts of waves [0, w) in a digit's row (8 words, two waves each)
__device__ __forceinline__ uint32_t p0_before(const uint4& r0, const uint4& r1, int w) {
  const uint32_t word[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
  uint32_t s = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t m = 2 * i + 1 < w ? 0xffffffffu : (2 * i < w ? 0x0000ffffu : 0u);
    s = sm_udot2(word[i] & m, 0x00010001u, s);
  }
  return s;
}

// Scheduling fence between the build of the next tile's records and the tile's global stores: the records (and so
// the wait for their loads) are complete before it, and no memory operation moves across it. No instruction.
__device__ __forceinline__ void p0_store_fence(uint4 (&rec)[kP0Items]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int k = 0; k < kP0Items; ++k)
    asm volatile("" : "+v"(rec[k].x), "+v"(rec[k].y), "+v"(rec[k].z), "+v"(rec[k].w) : : "memory");
#else
  (void)rec;
#endif
}

// A wave-uniform value the optimiser cannot see through (an SGPR pair). The tile base passes through it before the
// column addresses are formed: otherwise loop strength reduction keeps one 64-bit pointer per column and item alive
// across the whole loop (40 VGPRs), which the pipelined loop cannot afford. No instruction.
__device__ __forceinline__ int64_t p0_opaque(int64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+s"(v));
#endif
  return v;
}

// whether Src asks for the time-order check (a static member kTimeOrder that is true); sources without it build as
// before
template <typename S, typename = void>
struct p0_time_order : std::false_type {};
template <typename S>
struct p0_time_order<S, std::void_t<decltype(S::kTimeOrder)>> : std::integral_constant<bool, S::kTimeOrder> {};

// v of lane - 1 of the wave (lane 0: unspecified, replaced by the caller). Every lane of the wave must be active.
__device__ __forceinline__ uint32_t p0_lane_before(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
#else
  return __shfl_up(v, 1, 64);
#endif
}

// Chunk blockIdx.x = [blockIdx.x * per, + per) of the batch, tile by tile. cnt[d * G + g] = records of digit d in
// chunks before g (scan_chunks), dbase[d] = records of digits before d: chunk g's first position for digit d is
// dbase[d] + cnt[d * G + g].
template <typename Src>
__global__ void __launch_bounds__(kP0Block) pass0_kernel(Src src, uint4* __restrict__ drec, int64_t n, int64_t per,
                                                          int G, const uint32_t* __restrict__ cnt,
                                                          const uint32_t* __restrict__ dbase) {
  __shared__ __attribute__((aligned(16))) uint4 xb[kP0Tile];
  __shared__ __attribute__((aligned(16))) uint16_t wc[kBins][kP0Waves];
  __shared__ uint32_t tstart[kBins + 1];
  __shared__ uint32_t run[kBins];  // next output position of each digit for this chunk
  __shared__ uint32_t cst[kBins];  // first position of the digit's incomplete segment: carried = [cst, run)
  __shared__ __attribute__((aligned(16))) uint4 carry[kBins][kP0Seg - 1];
  __shared__ uint32_t lw[kP0Waves];
  // time-order check: relative time of wave w's last event of the tile in tlast[w] (w < 15); the tile's last event
  // (wave 15's) in tlast[15 + parity of the tile], so that the next tile's wave 0 still finds it after wave 15 has
  // written its own; tbad: some event of the chunk is out of order
  __shared__ uint32_t tlast[kP0Waves + 1];
  __shared__ uint32_t tbad;
  constexpr bool kTO = p0_time_order<Src>::value;

  const int tid = threadIdx.x, lane = tid & 63, w = wave_index();
  const int64_t lo = (int64_t)blockIdx.x * per;
  int64_t len = n - lo;
  if (len > per) len = per;
  if (len < 0) len = 0;
  src.init();
  uint4* row = (uint4*)&wc[tid][0];  // digit tid's count row, zeroed for the first tile here, then after each
                                     // tile's placement (its last reader), so no barrier opens a tile
  {
    const uint32_t r0 = dbase[tid] + cnt[(int64_t)tid * G + blockIdx.x];
    run[tid] = r0;
    cst[tid] = r0;
    row[0] = make_uint4(0, 0, 0, 0);
    row[1] = make_uint4(0, 0, 0, 0);
  }
  if constexpr (kTO) {
    if (tid == 0) {
      tbad = 0u;
      // the first tile's predecessor: the event before the chunk (whether its own high word is zero is its chunk's
      // business); none before the batch's first event, whose relative time 0 is below no other
      tlast[kP0Waves] = (lo > 0 && len > 0) ? (uint32_t)(src.time_at(lo - 1) - src.time0()) : 0u;
    }
  }
  lds_barrier();
  int tpar = 0;  // parity of the tile in the chunk
  typename Src::Raw raw[kP0Items];
  auto load_tile = [&](int64_t base) {
    const int64_t rem = lo + len - base;
    const int tn = rem < kP0Tile ? (int)rem : kP0Tile;
    base = p0_opaque(base);
#pragma unroll
    for (int k = 0; k < kP0Items; ++k) {
      const int e = w * 64 * kP0Items + k * 64 + lane;
      if (e < tn) raw[k] = src.load(base + e);
    }
  };
  // Software pipeline. gfx9 counts vector loads and stores in one in-order vmcnt, so a wait for a load that was
  // issued after a store also waits for that store's acknowledgement. Hence the order: tile t's column loads are
  // issued inside tile t-1 (after its ranking), and src.record consumes them after tile t-1's placement barrier and
  // BEFORE tile t-1's global stores. That wait is the loop's only one for vector memory, and the youngest stores it
  // has behind it are tile t-2's, a whole tile old; tile t-1's scattered stores drain during tile t's ranking and
  // scan. The loop is rotated so that each stage has one site: an iteration builds the records of the tile at
  // `base` (if there is one), stores the tile before it (if there is one), then ranks, scans and places its own.
  const int64_t end = lo + len;
  if (len > 0) load_tile(lo);
  // the placed, not yet stored tile: its size, whether it ends the chunk
  int ptile_n = 0;
  bool plast = false;
  uint4 cq0, cq1, cq2;  // digit tid's carried records that leave with that tile
  static_assert(kP0Seg == 4, "three carried records at most");

  for (int64_t base = lo;; base += kP0Tile) {
    const bool more = base < end;
    const int tile_n = (int)((end - base) < kP0Tile ? (end - base) : kP0Tile);
    const bool last = base + kP0Tile >= end;
    uint4 rec[kP0Items];
    // The loop's only wait for vector memory: vmcnt(0), stated once and under no condition. The waits the compiler
    // places itself sit under `more` and `e < tile_n` and leave it, on paths no tile takes, a load still in flight
    // into raw[]'s registers; it then guards every address it forms in one of them at load_tile with a wait of its
    // own, behind this tile's stores and between the tile's loads.
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_s_waitcnt(0x0F70);
#endif
    uint32_t tfirst = 0;  // relative time of the wave's first event of the tile (compared after the next barrier)
    if (more) {
      uint32_t tq[kP0Items];
      bool tb = false;
#pragma unroll
      for (int k = 0; k < kP0Items; ++k) {
        const int e = w * 64 * kP0Items + k * 64 + lane;
        if constexpr (kTO) tq[k] = 0u;
        if (e < tile_n) {
          rec[k] = src.record(raw[k], base + e);
          if constexpr (kTO) {
            const int64_t rel = src.time_of(raw[k]) - src.time0();
            tq[k] = (uint32_t)rel;
            tb |= ((uint64_t)rel >> 32) != 0;
          }
        }
      }
      if constexpr (kTO) {
#pragma unroll
        for (int k = 0; k < kP0Items; ++k) {
          const int e = w * 64 * kP0Items + k * 64 + lane;
          uint32_t pv = p0_lane_before(tq[k]);
          // lane 0: lane 63 of the item before (all of it is in the tile when this event is); item 0 waits for the
          // wave before's last event
          const uint32_t pl = wave_read_lane(tq[k > 0 ? k - 1 : 0], 63);
          if (lane == 0) pv = k > 0 ? pl : tq[0];
          tb |= e < tile_n && tq[k] < pv;
        }
        // (a wave the tile ends in writes a word no wave reads: the waves after it have no event)
        if (lane == 63) tlast[w < kP0Waves - 1 ? w : kP0Waves - 1 + tpar] = tq[kP0Items - 1];
        if (tb) tbad = 1u;
        tfirst = tq[0];
      }
    }
    p0_store_fence(rec);

    if (base != lo) {  // the tile before: its leaving carried records, then its own
      // digit tid's run / carry start / tile count, unchanged in LDS since that tile's scan (kept in no register
      // across the record build)
      const uint32_t rn = run[tid], c0 = cst[tid], ct = tstart[tid + 1] - tstart[tid];
      const uint32_t lim = plast ? 0xffffffffu : ((rn + ct) & ~(uint32_t)(kP0Seg - 1));
      const uint32_t nfl = (rn != c0 && (plast || lim > c0)) ? rn - c0 : 0u;  // as at the read of cq below
      if (nfl > 0) drec[c0] = cq0;
      if (nfl > 1) drec[c0 + 1] = cq1;
      if (nfl > 2) drec[c0 + 2] = cq2;
      // one 16-byte store per record, or into the carry when its segment is not complete in this chunk yet
#pragma unroll
      for (int r = 0; r < kP0Items; ++r) {
        const int s = r * kP0Block + tid;
        if (s < ptile_n) {
          const uint4 x = xb[s];
          const uint32_t d = x.x & (kBins - 1);
          const uint32_t rd = run[d], td = tstart[d];
          const uint32_t dest = rd + (uint32_t)s - td;
          const uint32_t ld = plast ? 0xffffffffu : ((rd + tstart[d + 1] - td) & ~(uint32_t)(kP0Seg - 1));
          if (dest < ld) {
            drec[dest] = x;
          } else {
            const uint32_t cd = cst[d];
            carry[d][dest - (cd > ld ? cd : ld)] = x;
          }
        }
      }
      lds_barrier();  // every destination computed from run / cst before they advance; xb / tstart free again
      run[tid] = rn + ct;
      if (lim != 0xffffffffu && lim > c0) cst[tid] = lim;
    }
    if (!more) break;

    // stable rank within (wave, digit): wave64 ballot peer masks, in arrival order
    uint32_t dg[kP0Items], lp = 0;  // lp: the four ranks, 8 bits each (< 256: a wave has 256 records of a tile)
    static_assert(kP0Items * 64 <= 256 && kP0Items <= 4, "a record's rank within (wave, digit) fits 8 bits");
#pragma unroll
    for (int k = 0; k < kP0Items; ++k) {
      const int e = w * 64 * kP0Items + k * 64 + lane;
      const bool valid = e < tile_n;
      dg[k] = valid ? rec[k].x & (kBins - 1) : 0u;
      const uint64_t peers = peer_mask(dg[k], valid);
      uint32_t old = 0;
      if (valid) old = wc[dg[k]][w];
      wave_lockstep();
      const uint32_t below = lanes_below(peers);
      if (valid && below == 0) wc[dg[k]][w] = (uint16_t)(old + (uint32_t)__popcll(peers));
      wave_lockstep();
      lp |= (old + below) << (8 * k);
    }
    // the next tile's loads: no global store between here and their wait at the top of the next iteration
    if (!last) load_tile(base + kP0Tile);
    lds_barrier();
    if constexpr (kTO) {
      // the wave's first event against the wave before's last, or the last event of the tile before (written one
      // tile ago; overwritten two barriers from here at the earliest)
      if (lane == 0 && w * 64 * kP0Items < tile_n && tfirst < tlast[w > 0 ? w - 1 : kP0Waves - 1 + (tpar ^ 1)])
        tbad = 1u;
      tpar ^= 1;
    }

    // digit tid: its tile count and the tile's digit starts (block scan)
    uint32_t ct = 0;
    {
      const uint4 r0 = row[0], r1 = row[1];
      const uint32_t word[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
      for (int i = 0; i < 8; ++i) ct = sm_udot2(word[i], 0x00010001u, ct);
      uint32_t tot;
      tstart[tid] = block_excl<kP0Block>(ct, lw, &tot);
      if (tid == 0) tstart[kBins] = tot;
    }
    const uint32_t rn = run[tid], c0 = cst[tid];
    const uint32_t lim = last ? 0xffffffffu : ((rn + ct) & ~(uint32_t)(kP0Seg - 1));
    lds_barrier();

    // the tile into LDS grouped by digit (arrival order within a digit)
#pragma unroll
    for (int k = 0; k < kP0Items; ++k) {
      const int e = w * 64 * kP0Items + k * 64 + lane;
      if (e < tile_n) {
        const uint32_t d = rec[k].x & (kBins - 1);  // (recomputed: dg[] is not kept across the scan)
        const uint4* rr = (const uint4*)&wc[d][0];
        xb[tstart[d] + p0_before(rr[0], rr[1], w) + ((lp >> (8 * k)) & 0xffu)] = rec[k];
      }
    }
    // carried records of digit tid whose segment completes now (or the chunk ends) leave first: read here, before
    // the barrier that lets their slots be refilled, stored after the wait for the next tile's loads
    const uint32_t nfl = (rn != c0 && (last || lim > c0)) ? rn - c0 : 0u;
    if (nfl > 0) cq0 = carry[tid][0];
    if (nfl > 1) cq1 = carry[tid][1];
    if (nfl > 2) cq2 = carry[tid][2];
    lds_barrier();  // xb complete; the carry slots read above may be refilled; the count rows are read no more
    row[0] = make_uint4(0, 0, 0, 0);
    row[1] = make_uint4(0, 0, 0, 0);
    ptile_n = tile_n;
    plast = last;
  }
  src.flush();
  if constexpr (kTO) {
    // every write of tbad lies before the last tile's placement barriers
    if (tid == 0 && tbad != 0u) src.time_bad();
  }
}

}  // namespace
}  // namespace sm
