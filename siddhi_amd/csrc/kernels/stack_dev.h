// Device side of the bucket-stack pipeline (stack.hip): the register stack, exact comparison of equal value codes,
// block scan, and the ring kernel (v4). A header of its own so that the same source also builds on the host under
// the wave emulator of tests/native/ (SM_HOST_EMU, hd.h), where tests/test_stack_emu.py checks the kernel against a
// plain per-key pending-list model on the CPU.
#pragma once
#include "fastpath_dev.h"
#ifdef SM_HOST_EMU
#include <cstdio>
#include <cstdlib>
#endif

namespace sm {
namespace {

constexpr int kKeys = 1024;  // in-bucket keys
#ifndef SM_STACK_KC
#define SM_STACK_KC 5         // A/B build flag (v2, config 4, slices of 4608: 3 -> 34.9 ms, 4 -> 32.1, 5 -> 31.7)
#endif
constexpr int kC = SM_STACK_KC;  // stack entries held in registers
constexpr int kQ = 32;           // spilled entries per thread (HBM ring)
constexpr int kOB = 1024;        // order workgroup: thread d owns bucket d
#ifndef SM_ORDER_TB
#define SM_ORDER_TB 13  // A/B build flag (config 4 order kernel: 13 -> 6.65 ms, 15 (direct writes) -> 9.8 ms; round 6:
#endif                  // 14 with two placement passes per tile (stack.hip kSplit) 9.6 against 6.7 ms, same box)
constexpr int kTB = SM_ORDER_TB;  // order tile: 2^kTB consecutive relative ordinals
constexpr int kOT = 1 << kTB;

enum : uint32_t { SE_OVERFLOW = 1, SE_LOG = 2, SE_NAN = 4, SE_CAND = 8, SE_ORD = 16 };

// Exact value of a compared attribute: a batch row's column, or a carried partial's stored value.
struct ExactSrc {
  bool exact_codes;
  int vtype, vattr, cwidth;
  const void* vcol;
  const int64_t* ord;
  int64_t obase, n;
  const int64_t* crow;
  int32_t o0;
  uint32_t cs, ce;  // this key's carried rows
  __device__ bool carried(uint32_t o) const { return (int32_t)o < o0; }
  __device__ int64_t row_of(uint32_t o) const {
    if (!ord) return o;
    const int64_t want = (int64_t)o + obase;
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (ord[mid] < want) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  }
  __device__ int64_t carry_row(uint32_t o) const {
    const int64_t want = (int64_t)(int32_t)o + obase;
    uint32_t lo = cs, hi = ce;
    while (lo + 1 < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (crow[(int64_t)mid * cwidth + 1] <= want) lo = mid;
      else hi = mid;
    }
    return lo;
  }
  __device__ double fval(uint32_t o) const {
    if (carried(o)) return __longlong_as_double((long long)crow[carry_row(o) * cwidth + 3 + vattr]);
    const int64_t r = row_of(o);
    return vtype == T_FLOAT ? (double)((const float*)vcol)[r] : ((const double*)vcol)[r];
  }
  __device__ int64_t ival(uint32_t o) const {
    if (carried(o)) return crow[carry_row(o) * cwidth + 3 + vattr];
    const int64_t r = row_of(o);
    return vtype == T_INT ? (int64_t)((const int32_t*)vcol)[r] : ((const int64_t*)vcol)[r];
  }
};

// equal inexact codes (or NaN): the exact values decide. Out of line: rare, and its binary searches must not
// hold registers in the event loop; the source is passed by value (a reference would put it in scratch).
#ifndef SM_EXACT_INLINE
#define SM_EXACT_INLINE __noinline__
#endif
template <int OP, bool FP>
__device__ SM_EXACT_INLINE bool c2_exact_v(bool exact_codes, int vtype, int vattr, int cwidth, const void* vcol,
                                        const int64_t* ord, int64_t obase, int64_t n, const int64_t* crow, int32_t o0,
                                        uint32_t cs, uint32_t ce, uint32_t oi, uint32_t oj) {
  const ExactSrc ex{exact_codes, vtype, vattr, cwidth, vcol, ord, obase, n, crow, o0, cs, ce};
  if constexpr (FP) return cmp_fixed<OP>(ex.fval(oj), ex.fval(oi));
  else return cmp_fixed<OP>(ex.ival(oj), ex.ival(oi));
}
template <int OP, bool FP>
__device__ __forceinline__ bool c2_exact(const ExactSrc& ex, uint32_t oi, uint32_t oj) {
  return c2_exact_v<OP, FP>(ex.exact_codes, ex.vtype, ex.vattr, ex.cwidth, ex.vcol, ex.ord, ex.obase, ex.n, ex.crow,
                            ex.o0, ex.cs, ex.ce, oi, oj);
}

// c2 = `e2.x OP e1.x` for partial i (code ci, ordinal oi) and event j
template <int OP, bool FP>
__device__ __forceinline__ bool c2_hit(const ExactSrc& ex, uint32_t ci, uint32_t oi, uint32_t cj, uint32_t oj) {
  const bool nan = FP & ((ci == kNanCode) | (cj == kNanCode));
  if (!nan & (ex.exact_codes | (ci != cj))) return cmp_fixed<OP>(cj, ci);
  return c2_exact<OP, FP>(ex, oi, oj);
}

struct Stack {
  uint32_t o[kC], c[kC];
  int32_t t[kC];
  int n;       // entries in registers
  int hb, hn;  // spill ring: head, count
};

__device__ __forceinline__ void st_pop(Stack& s) {
#pragma unroll
  for (int k = 0; k + 1 < kC; ++k) {
    s.o[k] = s.o[k + 1];
    s.c[k] = s.c[k + 1];
    s.t[k] = s.t[k + 1];
  }
  --s.n;
}

// the registers ran empty: bring back the youngest spilled entry (one at a time; spills are rare)
__device__ __forceinline__ void st_refill(Stack& s, const uint4* sp) {
  const uint4 e = sp[(s.hb + s.hn - 1) & (kQ - 1)];
  s.o[0] = e.x;
  s.c[0] = e.y;
  s.t[0] = (int32_t)e.z;
  s.hn -= 1;
  s.n = 1;
}

// push (o, c, t) on top; `now` = event time of the pushing event (entries older than now - within are dead)
__device__ __forceinline__ void st_push(Stack& s, uint4* sp, uint32_t o, uint32_t c, int32_t t, int32_t now,
                                        int64_t within, uint32_t* err) {
  if (s.n == kC) {
    if (within >= 0 && now - s.t[kC - 1] > (int32_t)within) {  // the register bottom and all spilled are dead
      s.hn = 0;
      s.n = kC - 1;
    } else {
      if (s.hn == kQ) {  // free the ring's dead head first
#pragma unroll 1
        while (s.hn > 0 && within >= 0 && now - (int32_t)sp[s.hb & (kQ - 1)].z > (int32_t)within) {
          s.hb = (s.hb + 1) & (kQ - 1);
          --s.hn;
        }
        if (s.hn == kQ) {  // more than kC + kQ live partials on one key: the walk pipeline takes the batch
          atomicOr(err, SE_OVERFLOW);
          s.hb = (s.hb + 1) & (kQ - 1);
          --s.hn;
        }
      }
      sp[(s.hb + s.hn) & (kQ - 1)] = make_uint4(s.o[kC - 1], s.c[kC - 1], (uint32_t)s.t[kC - 1], 0u);
      ++s.hn;
      s.n = kC - 1;
    }
  }
#pragma unroll
  for (int k = kC - 1; k > 0; --k) {
    s.o[k] = s.o[k - 1];
    s.c[k] = s.c[k - 1];
    s.t[k] = s.t[k - 1];
  }
  s.o[0] = o;
  s.c[0] = c;
  s.t[0] = t;
  ++s.n;
}

// Sentinel padding of the register stack (ring kernel v4; v2 does not pad): entries at index >= n hold a code no event
// beats unless it beats every live entry too (the largest code for > and >=, the smallest for < and <=), and a time
// no event of the batch finds expired (event times are below 2^30 relative to the batch), so that the event step's
// compares need no `u < n` test.
constexpr int32_t kPadT = 1 << 30;
template <int OP>
__device__ __forceinline__ constexpr uint32_t pad_code() {
  return (OP == CMP_LT || OP == CMP_LE) ? 0u : 0xffffffffu;
}
template <int OP>
__device__ __forceinline__ void st_pad(Stack& s) {
#pragma unroll
  for (int k = 0; k < kC; ++k)
    if (k >= s.n) {
      s.c[k] = pad_code<OP>();
      s.t[k] = kPadT;
    }
}

static_assert(kOB == 1024, "block_excl's default (fastpath_dev.h) is the order workgroup");

// ============================================================================================================
// v4 (default): the same closed form with a ring of ranked slices, so that no lane waits for the slowest key chain
// of one slice.
//   One workgroup per bucket (persistent), 1024 threads, thread h = in-bucket key h. The bucket is read once, in
//   slices of kSS records; kR consecutive slices are held in LDS, each ranked by key (wave64 ballot peer masks:
//   stable, arrival order within a key). In epoch e the slots hold slices e .. e+kR-1: every lane runs its key's
//   events against its register stack in one flat loop that must finish its events of slice e and may go on into
//   slices e+1 .. e+kR-1. A wave stops when all of its lanes have finished slice e, so a lane with many events in
//   slice e is mostly covered by lanes doing later slices' work instead of idling (simulated lane efficiency
//   0.58 against 0.35 for one slice at a time). Then slice e's matches are written (count per event, block scan,
//   placement at (offset of j) + (rank among j's pops counted from the oldest)) and slice e + kR is ranked into
//   the freed slot.
//   Per event the lane records its pops in the slot: the youngest popped e1 inline (pk, by arrival position), the
//   count (jc), and further pops in the slot's pool {i, position | k << 16}.
#ifndef SM_STACK_R
#define SM_STACK_R 2
#endif
#ifndef SM_STACK_SS
#define SM_STACK_SS 3072
#endif
constexpr int kR = SM_STACK_R;    // slices held in LDS
constexpr int kSS = SM_STACK_SS;  // records per slice
constexpr int kT4 = kKeys;        // threads: one in-bucket key each
constexpr int kW4 = kT4 / 64;     // waves (16): ranking counts per (key, wave) are 16 bytes per key
constexpr int kI4 = kSS / kT4;    // records per thread per slice
constexpr int kPool = kSS / 2;    // pops beyond the first per slice (more: the batch takes the sort / walk kernels)
static_assert(kSS % kT4 == 0 && kI4 * 64 <= 255 && kW4 == 16, "u8 per-(key, wave) counts, 16 waves");
static_assert(kSS <= 32768, "arrival positions | c1 fit 16 bits");

struct Slot4 {
  uint2 grp[kSS];       // key-grouped records {code, ts - ts0}; while the slot is ranked: u8 counts [key][wave]
  uint32_t ordt[kSS];   // ordinal by arrival position
  uint32_t pk[kSS];     // youngest pop (e1 ordinal) by arrival position
  uint2 pool[kPool];    // further pops {e1 ordinal, position | k << 16}
  uint32_t kst[kKeys];  // run of key h: start | count << 16
  uint16_t epos[kSS];   // key-grouped arrival position | c1 << 15; after the slice's epoch: output offset by position
  uint8_t jc[kSS];      // pops by arrival position
};
static_assert(sizeof(uint2) * kSS >= kKeys * kW4, "ranking counts fit grp");

// fields the event loop does not read (exact comparisons of equal codes, carried partials, carry-out): one struct in
// device memory, read where needed, so that they hold no registers across the loop
struct Stack4Cold {
  int64_t kmin, ts0, within, obase, n;
  int vtype, vattr, cwidth;
  int32_t o0;
  bool exact_codes;
  const void* vcol;
  const int64_t* ord;
  const uint4* cin;
  const uint32_t* cstart;
  const uint32_t* cend;
  const int64_t* crow;
  int64_t* cand;
  uint32_t* cand_n;
  uint32_t cand_cap;
  uint2* ktab;  // per key, bucket-major [d][h]: {its run's first candidate, its length}; or nullptr (stack.hip, carry-out)
};

#ifndef SM_EXACT4_INLINE
#define SM_EXACT4_INLINE __noinline__
#endif
struct Stack4Args {
  const uint4* rec;
  const uint32_t* dbase;
  uint32_t n;  // records (< 2^32: ordinals are u32)
  int H;
  int32_t within;  // < 0: no `within`
  bool exact_codes;
  uint32_t ntiles;
  const uint32_t* sbase;
  uint64_t* stage;
  uint32_t* mstart;
  uint32_t* mtot;
  uint4* spill;
  uint32_t* err;
  const Stack4Cold* cold;
  unsigned long long* stamps;  // SM_STACK4_STAMPS builds: shader clocks per phase, summed over waves
};

#ifndef SM_STACK4_SKIP
#define SM_STACK4_SKIP 0  // diagnostic build flag: 1 = no event loop (every pop count 0; wrong results, timing only)
#endif
#ifndef SM_STACK4_FLAT
#define SM_STACK4_FLAT 1  // A/B build flag: 0 = every event takes the general (cold) step of the event loop
#endif
#ifndef SM_STACK4_STAMPS
#define SM_STACK4_STAMPS 0  // diagnostic build flag: phase clock of stack4_kernel; the default build executes no stamp
#endif
// Slots of the phase clock: 0 ranking of the first kR slices, 1 event loop, 2 wait at the event loop's barrier (B0),
// 3 unused (it was the emission), 4 rest, 5 .. 9 the intervals F1 .. F5 of the epoch's chain (chain4), each read
// before the barrier that ends it, so that the wait at a barrier counts with the interval after it, 10 from before B5
// to the next event loop (B5's wait, the key runs, the next slice's loads).
constexpr int kStamps4 = 11;
#if SM_STACK4_STAMPS && defined(__HIP_DEVICE_COMPILE__)
#define SM4_CLOCK() __builtin_amdgcn_s_memtime()
#else
#define SM4_CLOCK() 0ull
#endif
#define SM4_PHASE(i)                              \
  do {                                            \
    if (SM_STACK4_STAMPS) {                       \
      const unsigned long long t_ = SM4_CLOCK();  \
      st_acc[i] += t_ - st_last;                  \
      st_last = t_;                               \
    }                                             \
  } while (0)

template <int OP, bool FP>
__device__ SM_EXACT4_INLINE bool c2_exact4(const Stack4Cold* c, uint32_t cs, uint32_t ce, uint32_t oi, uint32_t oj) {
  return c2_exact_v<OP, FP>(c->exact_codes, c->vtype, c->vattr, c->cwidth, c->vcol, c->ord, c->obase, c->n, c->crow,
                            c->o0, cs, ce, oi, oj);
}

// A per-lane value the optimiser cannot see through. What is computed from it is computed where it is used: without
// it, thread-invariant values of the epoch loop (a zero uint4, LDS addresses) are hoisted out of the loop, do not fit
// the 128 VGPRs and come back from scratch, and a scratch reload after the emission's stores waits for those stores.
// No instruction.
__device__ __forceinline__ uint32_t sm4_opaque(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(v));
#endif
  return v;
}

// The prefetched slice has arrived: the one wait of an epoch for vector memory. gfx9 counts vector loads and stores
// in one in-order vmcnt, so the first use of pre[] after the emission's staging stores would also wait for those
// stores; placed before them, it waits for loads issued an epoch ago and for nothing younger. No memory operation
// moves across it. No instruction beyond the s_waitcnt the compiler puts in front of it.
__device__ __forceinline__ void sm4_arrived(uint4 (&pre)[kI4]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int k = 0; k < kI4; ++k)
    asm volatile("" : "+v"(pre[k].x), "+v"(pre[k].y), "+v"(pre[k].z), "+v"(pre[k].w) : : "memory");
#else
  (void)pre;
#endif
}

#ifndef SM_RANK4_INLINE
#define SM_RANK4_INLINE __forceinline__
#endif
// what the emission half of an epoch works on besides the slot (chain4)
struct Emit4 {
  uint64_t* stb;      // the bucket's staged matches
  uint32_t* mst;      // the bucket's per-tile staging offsets
  uint32_t* s_pool;   // the slot's pool count
  uint32_t* s_lastj;  // ordinal of the previous slice's last record
  uint32_t* s_tot;
  uint32_t* lw;       // wave totals of the emission's scan
  int sn;             // records of the emitted slice
};

// One epoch's work between two event loops, on slot S, as one chain of five workgroup barriers B1 .. B5 after the
// caller's barrier B0 (every lane has left the events of the slice S holds). Two halves share every interval:
//   emission (EMIT): the matches of the slice S holds go to the bucket's staging run, in arrival order of j (count
//     per event, block scan, placement at (offset of j) + (rank among j's pops counted from the oldest)); it reads
//     the slot's jc / pk / pool / ordt and writes epos (output offsets by arrival position) and device memory;
//   ranking (rank): the slice in pre[] (rn records) is ranked by key into S (wave64 ballot peer masks: stable, arrival
//     order within a key): key runs (kst), key-grouped {code, ts} and arrival positions | c1, ordinals by arrival
//     position. Its u8 counts [key][wave] lie on S.grp, dead since B0, and it writes the slot's grp / epos / ordt only
//     in the last interval, so each thread takes what it needs from the counts (the records of earlier waves, `bef`)
//     one interval before any thread places.
// Both conditions are block-uniform, so every path executes the same barriers. Intervals:
//   F1  emission: jc sums, wave scan -> E.lw             ranking: zero the thread's count row
//   F2  emission: offsets, epos, mst, youngest pops      ranking: count loop
//   F3  emission: pool pops, mrun                        ranking: key totals, bef, wave scan -> lwR
//   F4  emission: s_lastj, pool count                    ranking: key starts -> kst
//   F5                                                   ranking: placement into grp / epos / ordt
// ordt and epos of the slot are read by F2 .. F4 and overwritten in F5; pk / pool are read in F2 / F3 and next written
// by the event loop; each lw has a barrier between its last read and its next write.
// Within an interval a thread's LDS reads are stated together and under no condition (a position past the slice's end
// reads inside the slot and its value is dropped): a read under `p < sn` or `if (v[k])` is an exec region with a wait
// of its own, one LDS round trip after the other per record, with four waves per SIMD to cover them.
// PH: first slot of the phase clock for the five intervals (SM_STACK4_STAMPS builds); < 0: the caller's own.
template <bool EMIT, int PH>
__device__ SM_RANK4_INLINE void chain4(Slot4& S, const uint4 (&pre)[kI4], bool rank, int rn, uint32_t* lwR, bool fp,
                                       uint32_t* err, const Emit4& E, uint32_t& mrun,
                                       unsigned long long (&st_acc)[kStamps4], unsigned long long& st_last) {
  const int tid = threadIdx.x, lane = tid & 63, w = wave_index();
  uint8_t* cnt = (uint8_t*)S.grp;  // [key][wave]
  // ---- F1
  uint32_t v[kI4], sum = 0, incE = 0;
  if (EMIT) {
#pragma unroll
    for (int k = 0; k < kI4; ++k) {
      const int p = tid * kI4 + k;
      const uint32_t c = S.jc[p];  // (read under no condition: inside the slot, and the reads go out together)
      v[k] = p < E.sn ? c : 0u;
      sum += v[k];
    }
    incE = block_excl_waves<kT4>(sum, E.lw);
  }
  if (rank) {
    const uint32_t z = sm4_opaque(0u);  // (a zero made here, not one kept in four registers across the kernel)
    *(uint4*)(cnt + 16 * tid) = make_uint4(z, z, z, z);
  }
  if (PH >= 0) SM4_PHASE(PH);
  lds_barrier();  // B1
  // ---- F2
  if (EMIT) {
    uint32_t tot;
    uint32_t r = block_excl_finish<kT4>(sum, incE, E.lw, &tot);
    // the thread's ordinals and youngest pops, and the ordinal of the record before its first (0xffffffff: the bucket
    // starts here), in one batch of LDS reads with one wait, not a read and a wait per record under its condition
    // (the positions at and after sn are inside the slot and never used)
    uint32_t jo[kI4], yo[kI4];
#pragma unroll
    for (int k = 0; k < kI4; ++k) {
      jo[k] = S.ordt[tid * kI4 + k];
      yo[k] = S.pk[tid * kI4 + k];
    }
    uint32_t jp = tid == 0 ? *E.s_lastj : S.ordt[tid * kI4 - 1];
#pragma unroll
    for (int k = 0; k < kI4; ++k) {
      const int p = tid * kI4 + k;
      if (p < E.sn) {
        S.epos[p] = (uint16_t)r;  // the key-grouped positions are dead: output offsets by arrival position
        const uint32_t j = jo[k];
        // ordinal tiles whose first ordinal falls in (previous record's ordinal, this record's]: their first
        // match in this bucket is this record's first. From tile (jp >> kTB) + 1, which (jp + kOT) >> kTB also
        // is where the bucket starts (ordinals are below 2^31; 0xffffffff + kOT wraps to kOT - 1: tile 0)
        const uint32_t t0 = (jp + (uint32_t)kOT) >> kTB;
#pragma unroll 1
        for (uint32_t t = t0; t <= (j >> kTB); ++t) E.mst[t] = mrun + r;
        jp = j;
        if (v[k]) E.stb[mrun + r + v[k] - 1u] = ((uint64_t)j << 32) | yo[k];
      }
      r += v[k];
    }
    if (tid == 0) *E.s_tot = tot;
  }
  uint32_t hk[kI4], bef[kI4];  // the record's key; its rank among the key's records of the slice
  if (rank) {
    bool nan = false;
#pragma unroll
    for (int k = 0; k < kI4; ++k) {
      const int e = w * 64 * kI4 + k * 64 + lane;
      const bool valid = e < rn;
      nan |= fp && valid && pre[k].z == kNanCode;  // a NaN sends the batch to the sort / walk kernels (SE_NAN)
      hk[k] = valid ? (pre[k].x & kKeyMask) >> kRB : 0u;
      const uint64_t peers = peer_mask(hk[k], valid);
      uint32_t old = 0;
      if (valid) old = cnt[16 * hk[k] + w];
      wave_lockstep();
      const uint32_t below = lanes_below(peers);
      if (valid && below == 0) cnt[16 * hk[k] + w] = (uint8_t)(old + (uint32_t)__popcll(peers));
      wave_lockstep();
      bef[k] = old + below;
    }
    if (__any(nan) && lane == 0) atomicOr(err, SE_NAN);
  }
  if (PH >= 0) SM4_PHASE(PH + 1);
  lds_barrier();  // B2
  // ---- F3
  if (EMIT) {
    // the thread's pool entries (kPI at most), then what each points at, then the stores: two batches of LDS reads and
    // not a chain per entry (an entry past the count reads position 0 and stores nothing)
    constexpr int kPI = (kPool + kT4 - 1) / kT4;
    const uint32_t np = *E.s_pool < (uint32_t)kPool ? *E.s_pool : (uint32_t)kPool;
    const uint32_t k0 = sm4_opaque((uint32_t)tid);
    uint2 pe[kPI];
#pragma unroll
    for (int u = 0; u < kPI; ++u) pe[u] = S.pool[k0 + u * kT4 < np ? k0 + u * kT4 : 0u];
    uint32_t po[kPI], pj[kPI];
#pragma unroll
    for (int u = 0; u < kPI; ++u) {
      const uint32_t p = k0 + u * kT4 < np ? pe[u].y & 0xffffu : 0u;
      po[u] = S.epos[p] + S.jc[p];
      pj[u] = S.ordt[p];
    }
#pragma unroll
    for (int u = 0; u < kPI; ++u) {
      const uint32_t kk = pe[u].y >> 16;
#ifdef SM_EMU_DEBUG
      if (k0 + u * kT4 < np && ((pe[u].y & 0xffffu) >= (uint32_t)E.sn || kk >= S.jc[pe[u].y & 0xffffu])) {
        printf("bad pool entry k=%u/%u p=%u kk=%u sn=%d\n", k0 + u * kT4, np, pe[u].y & 0xffffu, kk, E.sn);
        continue;
      }
#endif
      if (k0 + u * kT4 < np) E.stb[mrun + po[u] - 1u - kk] = ((uint64_t)pj[u] << 32) | pe[u].x;
    }
    mrun += *E.s_tot;
  }
  uint32_t tot = 0, incR = 0;
  if (rank) {
    {  // key h = tid: its count over the waves
      const uint4 c = *(const uint4*)(cnt + 16 * tid);
      const uint32_t ones = 0x01010101u;
      tot = sm_udot4(c.x, ones, 0u) + sm_udot4(c.y, ones, 0u) + sm_udot4(c.z, ones, 0u) + sm_udot4(c.w, ones, 0u);
    }
#pragma unroll
    for (int k = 0; k < kI4; ++k) {
      // same-key records of earlier waves: the bytes of waves 0 .. w-1 in the key's 16-byte row (a record past the
      // slice's end reads row 0 and is not placed: the reads go out together, under no condition)
      const uint4 c = *(const uint4*)(cnt + 16 * hk[k]);
      const uint32_t wb = (uint32_t)w * 8u;  // bits of the row below wave w
      auto part = [&](uint32_t word, uint32_t lo) {
        const uint32_t nb = wb > lo ? (wb - lo >= 32u ? 32u : wb - lo) : 0u;
        const uint32_t m = nb >= 32u ? 0xffffffffu : ((1u << nb) - 1u);
        return sm_udot4(word & m, 0x01010101u, 0u);
      };
      bef[k] += part(c.x, 0) + part(c.y, 32) + part(c.z, 64) + part(c.w, 96);
    }
    incR = block_excl_waves<kT4>(tot, lwR);  // block scan over keys
  }
  if (PH >= 0) SM4_PHASE(PH + 2);
  lds_barrier();  // B3
  // ---- F4
  if (rank) {
    uint32_t all;
    const uint32_t st = block_excl_finish<kT4>(tot, incR, lwR, &all);
    S.kst[tid] = st | (tot << 16);
  }
  if (EMIT && tid == 0) {
    *E.s_lastj = S.ordt[E.sn - 1];
    *E.s_pool = 0;
  }
  if (PH >= 0) SM4_PHASE(PH + 3);
  lds_barrier();  // B4
  // ---- F5
  if (rank) {
    uint32_t ks[kI4];
#pragma unroll
    for (int k = 0; k < kI4; ++k) ks[k] = S.kst[hk[k]];  // (key 0's for a record past the slice's end)
#pragma unroll
    for (int k = 0; k < kI4; ++k) {
      const int e = w * 64 * kI4 + k * 64 + lane;
      if (e < rn) {
        const uint32_t pos = (ks[k] & 0xffffu) + bef[k];
        S.grp[pos] = make_uint2(pre[k].z, pre[k].w);
        S.epos[pos] = (uint16_t)((uint32_t)e | ((pre[k].x >> 31) << 15));
        S.ordt[e] = pre[k].y;
        if (SM_STACK4_SKIP) S.jc[e] = 0;
      }
    }
  }
  if (PH >= 0) SM4_PHASE(PH + 4);
  lds_barrier();  // B5
}

#ifdef SM_HOST_EMU
// emulator build only: what the straight-line event step relies on, for an event (cj, jt) without a tie
template <int OP>
inline void sm4_check_step(const Stack& st, uint32_t cj, int32_t jt, int32_t weff, int nhit, int nexp) {
  bool ok = st.n >= 0 && st.n <= kC && nexp <= st.n;
  for (int u = 0; u < kC; ++u) {
    if (u >= st.n) ok = ok && st.c[u] == pad_code<OP>() && st.t[u] == kPadT;  // padded
    ok = ok && cmp_fixed<OP>(cj, st.c[u]) == (u < nhit);                       // c2 holds on a prefix
    ok = ok && (jt - st.t[u] > weff) == (u >= st.n - nexp && u < st.n);        // expired is a suffix of the live
    if (u > 0 && u < st.n) ok = ok && st.t[u] <= st.t[u - 1];                  // older towards the bottom
  }
  if (!ok) {
    fprintf(stderr, "stack4 event step: invariant broken (n %d, nhit %d, nexp %d, code %u, time %d)\n", st.n, nhit,
            nexp, cj, jt);
    abort();
  }
}
#endif

template <int OP, bool FP>
__global__ void __launch_bounds__(kT4) stack4_kernel(Stack4Args a) {
  __shared__ __attribute__((aligned(16))) Slot4 sl[kR];
  __shared__ uint32_t lw[kW4];
  __shared__ uint32_t s_pool[kR];
  __shared__ uint32_t s_lastj, s_tot;
  const int tid = threadIdx.x, lane = tid & 63;
  const int h = tid;
  const bool has = h < a.H;
  const int32_t within32 = a.within;
  const int32_t weff = within32 < 0 ? INT32_MAX : within32;  // no `within`: no difference of two times exceeds it
  uint4* sp = a.spill + ((int64_t)blockIdx.x * kKeys + h) * kQ;
  unsigned long long st_acc[kStamps4] = {}, st_last = SM4_CLOCK();

  for (int d = blockIdx.x; d < kBins; d += gridDim.x) {
    const uint32_t b0 = a.dbase[d];
    const uint32_t blen = (d + 1 < kBins ? a.dbase[d + 1] : a.n) - b0;
    const uint32_t nsl = (blen + kSS - 1) / kSS;
    const uint4* recb = a.rec + b0;
    uint64_t* stb = a.stage + a.sbase[d];
    uint32_t* mst = a.mstart + (int64_t)d * (a.ntiles + 1);
    const uint32_t kr = ((uint32_t)h << kRB) | (uint32_t)d;
    Stack st;
    st.n = st.hb = st.hn = 0;
#pragma unroll
    for (int k = 0; k < kC; ++k) st.o[k] = 0;  // (ordinals at index >= n are never used; defined all the same)
    uint32_t cs = 0, ce = 0;
    if (has && a.cold->cin) {  // carried partials first (oldest first)
      const Stack4Cold* c4 = a.cold;
      cs = c4->cstart[kr];
      ce = c4->cend[kr];
      for (uint32_t q = cs; q < ce; ++q) {
        const uint4 c = c4->cin[q];
        st_push(st, sp, c.x, c.y, (int32_t)c.z, (int32_t)c.z, within32, a.err);
      }
    }
    st_pad<OP>(st);
    int32_t tl = 0;
    bool seen = false;
    uint32_t mrun = 0;
    __syncthreads();  // the previous bucket's readers of the slots are done
    if (tid == 0) s_lastj = 0xffffffffu;
    if (tid < kR) s_pool[tid] = 0;

    uint4 pre[kI4];
    auto load = [&](uint32_t s) {
#pragma unroll
      for (int k = 0; k < kI4; ++k) {
        const uint32_t p = s * kSS + (uint32_t)wave_index() * 64 * kI4 + k * 64 + lane;
        if (p < blen) {
          typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
          const u32x4 v = __builtin_nontemporal_load((const u32x4*)recb + p);
          pre[k] = make_uint4(v.x, v.y, v.z, v.w);
        }
      }
    };
    auto slice_n = [&](uint32_t s) { return (int)(blen - s * kSS < (uint32_t)kSS ? blen - s * kSS : (uint32_t)kSS); };
    // the lane's runs in the held slices, relative to the epoch: k = 0 is slice e
    uint32_t off[kR], cnt[kR];
    SM4_PHASE(4);
    for (uint32_t s = 0; s < (uint32_t)kR; ++s) {
      off[s] = cnt[s] = 0;
      if (s < nsl) {
        load(s);
        chain4<false, -1>(sl[s], pre, true, slice_n(s), lw, FP, a.err, Emit4{}, mrun, st_acc, st_last);
        const uint32_t v = sl[s].kst[h];
        off[s] = v & 0xffffu;
        cnt[s] = v >> 16;
      }
    }
    if (kR < nsl) load(kR);

    SM4_PHASE(0);
    for (uint32_t e = 0; e < nsl; ++e) {
      const int q0 = (int)(e % kR);
      // ---- stack phase: finish this lane's events of slice e; go on into the later held slices meanwhile
      // (a loop with its test at the bottom: the compiler does not rotate a loop whose test is a wave vote, and with
      // the test at the top it copies the whole register stack at the loop's head in every iteration)
      if (!SM_STACK4_SKIP && __any(cnt[0] != 0)) do {
        // the lane's next event: its first held slice with events left
        int k = kR - 1;
        uint32_t o_ = off[kR - 1], c_ = cnt[kR - 1];
        if constexpr (kR == 2) {  // plain selects
          k = cnt[0] != 0 ? 0 : 1;
          o_ = k ? off[1] : off[0];
          c_ = k ? cnt[1] : cnt[0];
        } else {
#pragma unroll
          for (int u = kR - 2; u >= 0; --u)
            if (cnt[u]) k = u;
#pragma unroll
          for (int u = kR - 2; u >= 0; --u)
            if (u == k) {
              o_ = off[u];
              c_ = cnt[u];
            }
        }
        // act: the lane has an event; else nothing is held for it and it waits for the wave. Such a lane runs the
        // straight-line step too, on its slot's first record and with every effect masked: a step under `if (act)`
        // would leave the compiler two versions of the register stack to merge, which it does with a copy of all of
        // it per iteration.
        const bool act = c_ != 0;
        if constexpr (kR == 2) {
          const uint32_t a0 = k == 0 ? 1u : 0u, a1 = ((k != 0) & act) ? 1u : 0u;
          off[0] += a0;
          cnt[0] -= a0;
          off[1] += a1;
          cnt[1] -= a1;
        } else {
#pragma unroll
          for (int u = 0; u < kR; ++u)
            if ((u == k) & act) {
              off[u] = o_ + 1;
              cnt[u] = c_ - 1;
            }
        }
        const int q = q0 + k >= kR ? q0 + k - kR : q0 + k;
        Slot4& S = sl[q];
        const uint32_t oa = act ? o_ : 0u;
        const uint2 g = S.grp[oa];
        const uint32_t ep = S.epos[oa];
        const uint32_t p = act ? ep & 0x7fffu : 0u;
        const uint32_t oj = S.ordt[p];
        const bool push = (ep >> 15) != 0;
        const uint32_t cj = g.x;
        const int32_t jt = (int32_t)g.y;
        tl = act ? jt : tl;
        seen |= act;
        // a NaN anywhere sent the batch to the sort / walk kernels (chain4: SE_NAN), so the codes alone decide here.
        //
        // Straight-line step. The register stack is padded (st_pad) and, for the four ordered compares, monotone: from
        // the top the codes never get easier to beat and the times never get younger (events of a key arrive in time
        // order; a push follows the pops of everything the new entry beats). So without a tie of inexact codes "c2
        // holds" is a prefix of the entries and "expired" is a suffix of the live ones, and the run is two counts:
        //   nhit = entries the event's code beats (a padded entry only together with every live one),
        //   nexp = expired entries (never a padded one), nl = n - nexp,
        //   pops = min(nhit, nl); the run stopped at an expired entry, which clears the stack, iff nexp && nl <= nhit.
        // The new stack is the old one shifted by pops with padding coming in at the bottom (a barrel shift written as
        // selects), then shifted the other way by one under the event's entry if c1 holds: no branch, no exec region.
        // A tie of inexact codes and a spill onto a full ring take the general step below.
        int nhit = 0, nexp = 0;
        bool anytie = false;
        // expired: jt - t > weff, as one threshold for the kC compares (event times are in [0, 2^30), entry times at
        // least -2^30, padding 2^30 and weff at most 2^31 - 1: neither side wraps; a lane without an event may hold
        // any time, hence the unsigned difference)
        const int32_t tmin = (int32_t)((uint32_t)jt - (uint32_t)weff);
#pragma unroll
        for (int u = 0; u < kC; ++u) {
          nhit += cmp_fixed<OP>(cj, st.c[u]) ? 1 : 0;
          nexp += st.t[u] < tmin ? 1 : 0;
          anytie |= st.c[u] == cj;
        }
        const int nl = st.n - nexp;
        const int nmin = nhit < nl ? nhit : nl;
        const bool clr = (nexp != 0) & (nl <= nhit);
        const int nrem = clr ? 0 : st.n - nmin;
        // A push onto a full stack stays here: the push shift drops the bottom entry. If that entry has expired, so has
        // the spill ring, which is emptied (it is how expired entries leave a stack that no run reaches); if it is
        // live, it is stored to the ring first (no wait: the store is not read back before a refill, which waits).
        // A run through all of the registers with entries left in the ring is finished below, after the step.
        const bool full = push & (nrem == kC);
        const bool spill = full & (nexp == 0), refill = (nexp == 0) & (nhit >= st.n) & (st.hn > 0);
        const bool general = !SM_STACK4_FLAT | (anytie & !a.exact_codes) | (spill & (st.hn == kQ));
        const bool flat = act & !general;
#ifdef SM_HOST_EMU
        if (flat) sm4_check_step<OP>(st, cj, jt, weff, nhit, nexp);
#endif
        const uint32_t np = flat ? (uint32_t)nmin : 0u;
        const bool clear = flat & clr, pushf = flat & push, ring0 = flat & (clr | (full & !spill));
        if (flat & spill) {
          sp[(st.hb + st.hn) & (kQ - 1)] = make_uint4(st.o[kC - 1], st.c[kC - 1], (uint32_t)st.t[kC - 1], 0u);
          ++st.hn;
        }
        if (np) S.pk[p] = st.o[0];
        if (np > 1) {  // further pops go to the slot's pool
          const uint32_t base = atomicAdd(&s_pool[q], np - 1u);
          if (base + np - 1u > (uint32_t)kPool) atomicOr(a.err, SE_LOG);
#pragma unroll
          for (int u = 1; u < kC; ++u)
            if ((uint32_t)u < np && base + u - 1u < (uint32_t)kPool)
              S.pool[base + u - 1u] = make_uint2(st.o[u], p | ((uint32_t)u << 16));
        }
        if (flat) S.jc[p] = (uint8_t)np;
        {
          // the old entries move up by the pops (a cleared stack: by all of them), padding comes in at the bottom ...
          constexpr int top = kC >= 8 ? 8 : kC >= 4 ? 4 : 2;
          static_assert(kC < 2 * top, "the shift's bits cover kC");
          const uint32_t sh = clear ? (uint32_t)kC : np;
#pragma unroll
          for (int b = top; b >= 1; b >>= 1) {
            const bool on = (sh & (uint32_t)b) != 0;
#pragma unroll
            for (int u = 0; u < kC; ++u) {  // ascending: entry u + b is still the previous stage's
              if (u + b < kC) {
                st.o[u] = on ? st.o[u + b] : st.o[u];
                st.c[u] = on ? st.c[u + b] : st.c[u];
                st.t[u] = on ? st.t[u + b] : st.t[u];
              } else {  // (the ordinal of a padded entry is never used)
                st.c[u] = on ? pad_code<OP>() : st.c[u];
                st.t[u] = on ? kPadT : st.t[u];
              }
            }
          }
          // ... and this event's entry goes on top (the bottom entry it pushes out is padding, or expired)
#pragma unroll
          for (int u = kC - 1; u > 0; --u) {
            st.o[u] = pushf ? st.o[u - 1] : st.o[u];
            st.c[u] = pushf ? st.c[u - 1] : st.c[u];
            st.t[u] = pushf ? st.t[u - 1] : st.t[u];
          }
          st.o[0] = pushf ? oj : st.o[0];
          st.c[0] = pushf ? cj : st.c[0];
          st.t[0] = pushf ? jt : st.t[0];
          st.n = flat ? nrem + ((push & !full) ? 1 : 0) : st.n;
          st.hn = ring0 ? 0 : st.hn;
        }
        if (__builtin_expect(flat & refill, 0)) {
          // The run popped every register entry and the ring is not empty: it goes on there, youngest first, one
          // entry at a time (rare). An entry that stays comes back into the registers, beneath this event's own.
          uint32_t npop = np;
#pragma unroll 1
          for (;;) {
            const uint4 e = sp[(st.hb + st.hn - 1) & (kQ - 1)];
            if (jt - (int32_t)e.z > weff) {  // expired: so is everything older
              st.hn = 0;
              break;
            }
            const bool hh = (a.exact_codes | (e.y != cj)) ? cmp_fixed<OP>(cj, e.y)
                                                          : c2_exact4<OP, FP>(a.cold, cs, ce, e.x, oj);
            st.hn -= 1;
            if (!hh) {
              if (push) {
                st.o[1] = e.x;
                st.c[1] = e.y;
                st.t[1] = (int32_t)e.z;
              } else {
                st.o[0] = e.x;
                st.c[0] = e.y;
                st.t[0] = (int32_t)e.z;
              }
              st.n += 1;
              break;
            }
            if (npop == 0) {
              S.pk[p] = e.x;
            } else {  // each spilled pop reserves its own pool entry
              const uint32_t b1 = atomicAdd(&s_pool[q], 1u);
              if (b1 < (uint32_t)kPool) S.pool[b1] = make_uint2(e.x, p | (npop << 16));
              else atomicOr(a.err, SE_LOG);
            }
            ++npop;
            if (st.hn == 0) break;
          }
          S.jc[p] = (uint8_t)npop;
        }
        if (__builtin_expect(act & general, 0)) {
        // General step (rare: a tie of inexact codes, a spill onto a full ring): per-entry masks with the live test,
        // the exact compare of tied codes, refills from the spill ring, st_push; the padding is restored at its end.
        uint32_t hit = 0, exp = 0, tie = 0;
#pragma unroll
        for (int u = 0; u < kC; ++u) {
          const bool lv = u < st.n;
          hit |= (lv && cmp_fixed<OP>(cj, st.c[u])) ? (1u << u) : 0u;
          exp |= (lv && within32 >= 0 && jt - st.t[u] > within32) ? (1u << u) : 0u;
          tie |= (lv && !a.exact_codes && st.c[u] == cj) ? (1u << u) : 0u;
        }
        if (tie) {  // equal inexact codes: the exact values decide (out of line, one call site)
#pragma unroll 1
          for (uint32_t m = tie; m; m &= m - 1u) {
            const int u = __builtin_ctz(m);
            uint32_t oi = st.o[0];
#pragma unroll
            for (int v = 1; v < kC; ++v)
              if (v == u) oi = st.o[v];
            if (c2_exact4<OP, FP>(a.cold, cs, ce, oi, oj)) hit |= 1u << u;
            else hit &= ~(1u << u);
          }
        }
        const uint32_t ok = hit & ~exp;
        uint32_t npop = (uint32_t)__builtin_ctz(~ok);  // leading entries popped
        if (npop > (uint32_t)st.n) npop = st.n;
        const bool stop_expired = npop < (uint32_t)st.n && ((exp >> npop) & 1u);
        const bool cont = !stop_expired && npop == (uint32_t)st.n && st.hn > 0;
        if (npop) S.pk[p] = st.o[0];
        if (npop > 1) {  // further pops go to the slot's pool
          const uint32_t base = atomicAdd(&s_pool[q], npop - 1u);
          if (base + npop - 1u > (uint32_t)kPool) atomicOr(a.err, SE_LOG);
#pragma unroll
          for (int u = 1; u < kC; ++u)
            if ((uint32_t)u < npop && base + u - 1u < (uint32_t)kPool)
              S.pool[base + u - 1u] = make_uint2(st.o[u], p | ((uint32_t)u << 16));
        }
        // shift the register part down by npop
#pragma unroll
        for (int b = 1; b < kC; b <<= 1)
          if (npop & b) {
#pragma unroll
            for (int u = 0; u < kC; ++u)
              if (u + b < kC) {
                st.o[u] = st.o[u + b];
                st.c[u] = st.c[u + b];
                st.t[u] = st.t[u + b];
              }
          }
        st.n -= (int)npop;
        if (stop_expired) {  // the entry that stopped the run has expired: so has every older one
          st.n = 0;
          st.hn = 0;
        } else if (cont) {  // ran through the registers: continue into the spill ring (rare)
#pragma unroll 1
          for (;;) {
            st_refill(st, sp);
            if (within32 >= 0 && jt - st.t[0] > within32) {
              st.n = 0;
              st.hn = 0;
              break;
            }
            const bool hh = (a.exact_codes | (st.c[0] != cj)) ? cmp_fixed<OP>(cj, st.c[0])
                                                               : c2_exact4<OP, FP>(a.cold, cs, ce, st.o[0], oj);
            if (!hh) break;
            if (npop == 0) {
              S.pk[p] = st.o[0];
            } else {  // each spilled pop reserves its own pool entry
              const uint32_t b1 = atomicAdd(&s_pool[q], 1u);
              if (b1 < (uint32_t)kPool) S.pool[b1] = make_uint2(st.o[0], p | (npop << 16));
              else atomicOr(a.err, SE_LOG);
            }
            ++npop;
            st_pop(st);
            if (st.hn == 0) break;
          }
        }
        S.jc[p] = (uint8_t)npop;
        if (push) st_push(st, sp, oj, cj, jt, jt, within32, a.err);
        st_pad<OP>(st);
        }
      } while (__any(cnt[0] != 0));
      SM4_PHASE(1);
      lds_barrier();  // every lane is done with slice e
      SM4_PHASE(2);
      sm4_arrived(pre);  // slice e + kR, loaded during the epoch before (unconditional: a wait under a condition
                         // leaves the compiler its own wait at the ranking's first use, behind the stores)

#ifdef SM_HOST_EMU
      {  // emulator build only: nothing reads the slot's key-grouped records after this barrier
#pragma unroll
        for (int k = 0; k < kI4; ++k) sl[q0].grp[tid * kI4 + k] = make_uint2(0xdeadbeefu, 0xdeadbeefu);
        __syncthreads();
      }
#endif
      // ---- slice e's matches, in arrival order of j, and slice e + kR into the freed slot: one barrier chain
      off[0] = off[1];
      cnt[0] = cnt[1];
#pragma unroll
      for (int u = 1; u + 1 < kR; ++u) {
        off[u] = off[u + 1];
        cnt[u] = cnt[u + 1];
      }
      off[kR - 1] = cnt[kR - 1] = 0;
      {
        const bool more = e + kR < nsl;
        // the emission's wave totals lie on the slot's key runs, which are in off / cnt since the slot was ranked and
        // are written again in F4
        const Emit4 E{stb, mst, &s_pool[q0], &s_lastj, &s_tot, sl[q0].kst, slice_n(e)};
        chain4<true, 5>(sl[q0], pre, more, more ? slice_n(e + kR) : 0, lw, FP, a.err, E, mrun, st_acc, st_last);
        if (more) {
          const uint32_t vv = sl[q0].kst[h];
          off[kR - 1] = vv & 0xffffu;
          cnt[kR - 1] = vv >> 16;
          if (e + kR + 1 < nsl) load(e + kR + 1);  // lands during the next stack phase
        }
      }
      SM4_PHASE(10);
    }
    // tiles after the bucket's last record start at its end
    __syncthreads();
    {
      const uint32_t jl = s_lastj;
      const uint32_t t0 = jl == 0xffffffffu ? 0u : (jl >> kTB) + 1u;
      for (uint32_t t = t0 + tid; t <= (uint32_t)a.ntiles; t += kT4) mst[t] = mrun;
      if (tid == 0) a.mtot[d] = mrun;
    }

    // ---- carry out: the partials still pending in the reference (not matched, not found expired by the key's
    // last event; a key without events in this batch keeps all of its carried partials)
    auto pending = [&](int32_t t) { return !seen || within32 < 0 || (int64_t)tl - t <= within32; };
    uint32_t keep = 0;
    if (has) {
#pragma unroll
      for (int k = 0; k < kC; ++k)
        if (k < st.n && pending(st.t[k])) ++keep;
      for (int k = 0; k < st.hn; ++k)
        if (pending((int32_t)sp[(st.hb + k) & (kQ - 1)].z)) ++keep;
    }
    const uint32_t inc = wave_incl_scan(keep);
    uint32_t base = 0;
    const Stack4Cold* c4 = a.cold;
    if (lane == 63 && inc) base = atomicAdd(c4->cand_n, inc);
    base = __shfl(base, 63, 64) + inc - keep;
    // the key's run, for the carry-out that places rows by a scan of these counts instead of a sort (a wave's keys are
    // consecutive words of bucket d's row)
    if (has && c4->ktab) c4->ktab[(int64_t)d * kKeys + h] = make_uint2(base, keep);
    if (keep) {
      const ExactSrc ex{c4->exact_codes, c4->vtype, c4->vattr, c4->cwidth, c4->vcol, c4->ord, c4->obase, c4->n,
                        c4->crow, c4->o0, cs, ce};
      const int64_t key = c4->kmin + (int64_t)kr;
      auto put = [&](uint32_t o, int32_t t) {
        if (!pending(t)) return;
        if (base < c4->cand_cap) {
          int64_t* c = c4->cand + 4 * (int64_t)base;
          c[0] = key;
          c[1] = (int64_t)(int32_t)o + c4->obase;
          c[2] = (int64_t)t + c4->ts0;
          c[3] = ex.carried(o) ? -(int64_t)ex.carry_row(o) - 1 : ex.row_of(o);
        } else {
          atomicOr(a.err, SE_CAND);
        }
        ++base;
      };
      // one run per key, oldest first (build_carry's key_runs_ordered relies on it): spill ring, then registers
      for (int k = 0; k < st.hn; ++k) {
        const uint4 c = sp[(st.hb + k) & (kQ - 1)];
        put(c.x, (int32_t)c.z);
      }
#pragma unroll
      for (int k = kC - 1; k >= 0; --k)
        if (k < st.n) put(st.o[k], st.t[k]);
    }
  }
  SM4_PHASE(4);
  if (SM_STACK4_STAMPS && a.stamps && lane == 0)
    for (int i = 0; i < kStamps4; ++i) atomicAdd(&a.stamps[i], st_acc[i]);
}

}  // namespace
}  // namespace sm
