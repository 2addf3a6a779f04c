// Device helpers shared by the keyed fast-path kernels (fastpath3.hip: sort / walk pipeline; stack.hip:
// bucket-stack pipeline): record value codes, compare specialisation, wave64 ranking primitives.
#pragma once
#include <type_traits>

#include "expr.h"
#include "nfa.h"

namespace sm {
namespace {

#ifndef SM_RB
#define SM_RB 10
#endif
constexpr int kRB = SM_RB;  // radix bits per pass
constexpr int kBins = 1 << kRB;
constexpr uint32_t kKeyMask = 0x7fffffffu;

constexpr uint32_t kNanCode = 0xffffffffu;  // value code of a NaN (FLOAT / DOUBLE): always compared exactly

// value-code modes
enum : int { VC_I32 = 0, VC_F32 = 1, VC_F64 = 2, VC_I64R = 3, VC_I64H = 4 };

struct Ctrl {
  unsigned long long kmin, kmax;  // sign-biased key range
  unsigned long long omax;        // max relative ordinal
  unsigned long long vmin, vmax;  // sign-biased range of a LONG compared attribute
  unsigned int bad_ts, bad_ord;   // ts decreasing / ordinals not increasing
  long long ts0, ts_last;
  long long o0;  // relative ordinal of the batch's first event
};

// Workgroup barrier for LDS hand-offs only: waits for this wave's LDS operations, not for its global stores
// (__syncthreads() may also drain vmcnt, which exposes every round of scattered stores). No kernel here exchanges
// global data between the waves of a workgroup.
__device__ __forceinline__ void lds_barrier() {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
#else  // host wave emulator (hd.h SM_HOST_EMU): a workgroup barrier
  __syncthreads();
#endif
}

// Lockstep point of a wave: a no-op on the GPU (the lanes of a wave execute each instruction together), a wave
// barrier under the host wave emulator, where the lanes are threads: placed between an LDS read every lane makes
// and a write one lane makes to the same word (the rank-counting idiom), which SIMD order serialises on the GPU.
__device__ __forceinline__ void wave_lockstep() {
#if !defined(__HIP_DEVICE_COMPILE__) && defined(SM_HOST_EMU)
  (void)__ballot(1);
#endif
}

// gfx950 bit / dot instructions, with plain restatements for the host wave emulator
// (stated as the instruction: from the builtin the compiler makes a shift left and a shift right per bit)
template <int B>
__device__ __forceinline__ uint32_t sm_sbfe1(uint32_t d) {  // bit B of d as 0 or ~0
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t r;
  asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(r) : "v"(d), "n"(B));
  return r;
#else
  return ((d >> B) & 1u) ? 0xffffffffu : 0u;
#endif
}
__device__ __forceinline__ uint32_t sm_and_not_xor(uint32_t a, uint32_t b, uint32_t c) {  // a & ~(b ^ c)
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x90);  // a = 0xF0, b = 0xCC, c = 0xAA
#else
  return a & ~(b ^ c);
#endif
}
__device__ __forceinline__ uint32_t sm_udot4(uint32_t a, uint32_t b, uint32_t c) {  // sum of byte products + c
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_udot4(a, b, c, false);
#else
  uint32_t s = c;
  for (int k = 0; k < 4; ++k) s += ((a >> (8 * k)) & 255u) * ((b >> (8 * k)) & 255u);
  return s;
#endif
}

// Lanes of this wave whose kRB-bit digit equals this lane's (valid lanes only): one ballot per bit, and per
// bit one v_bitop3 per half, peers &= bit ? ballot : ~ballot  ==  peers & ~(ballot ^ sext(bit)).
template <int BB>
__device__ __forceinline__ void peer_mask_bit(uint32_t d, uint32_t& lo, uint32_t& hi) {
  const uint32_t m = sm_sbfe1<BB>(d);  // 0 or ~0
  const uint64_t bal = __ballot(m != 0u);
  lo = sm_and_not_xor(lo, (uint32_t)bal, m);
  hi = sm_and_not_xor(hi, (uint32_t)(bal >> 32), m);
  if constexpr (BB + 1 < kRB) peer_mask_bit<BB + 1>(d, lo, hi);
}
__device__ __forceinline__ uint64_t peer_mask(uint32_t d, bool valid) {
  const uint64_t v = __ballot(valid);
  uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
  peer_mask_bit<0>(d, lo, hi);
  return (uint64_t)lo | ((uint64_t)hi << 32);
}

__device__ __forceinline__ uint64_t lanemask_lt() {
  const int lane = threadIdx.x & 63;
  return lane == 0 ? 0ull : (~0ull >> (64 - lane));
}

// set bits of m below this lane (m & lanemask_lt(), counted): mbcnt needs no lane mask in registers
__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
#else
  return (uint32_t)__popcll(m & lanemask_lt());
#endif
}

// The wave's index in its workgroup as a scalar: what depends on it alone (masks over the waves before this one,
// the wave's first record of a tile) then lives in SGPRs and not in one VGPR per value per lane.
__device__ __forceinline__ int wave_index() {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
#else
  return (int)(threadIdx.x >> 6);
#endif
}

// One v_mov_b32_dpp, bank mask 0xf, bound_ctrl off: the lane takes v of the lane CTRL names, or keeps `old` where
// that lane does not exist or the lane's own 16-lane row is not in the row mask ROWS. Only the three controls of
// the scans below are used (and modelled by the host wave emulator, hd.h sm_emu_dpp).
constexpr int kDppRowShr = 0x110;      // row_shr:n = kDppRowShr + n: lane l - n of the same row
constexpr int kDppRowBcast15 = 0x142;  // row_bcast:15: lane 15 of the row before
constexpr int kDppRowBcast31 = 0x143;  // row_bcast:31: lane 31, into rows 2 and 3
template <int CTRL, int ROWS>
__device__ __forceinline__ uint32_t sm_dpp(uint32_t old, uint32_t v) {
#if !defined(__HIP_DEVICE_COMPILE__) && defined(SM_HOST_EMU)
  return sm_emu_dpp(old, v, CTRL, ROWS);
#else
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROWS, 0xf, false);
#endif
}

// v of lane l, l wave-uniform (v_readlane)
__device__ __forceinline__ uint32_t wave_read_lane(uint32_t v, int l) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
#else
  return __shfl(v, l, 64);
#endif
}

// Inclusive scan within each 16-lane row: four DPP adds, no LDS and no lane masks (with old = 0 the compiler folds
// each move into the add: v_add_u32_dpp). Every lane of the wave must be active: an inactive lane contributes 0
// and not its register, unlike a __shfl_up.
__device__ __forceinline__ uint32_t row_incl_scan(uint32_t v) {
  v += sm_dpp<kDppRowShr + 1, 0xf>(0u, v);
  v += sm_dpp<kDppRowShr + 2, 0xf>(0u, v);
  v += sm_dpp<kDppRowShr + 4, 0xf>(0u, v);
  v += sm_dpp<kDppRowShr + 8, 0xf>(0u, v);
  return v;
}

// Inclusive scan over the 64 lanes of the wave: the row scan, then lane 15 of rows 0 and 2 into rows 1 and 3, then
// lane 31 into rows 2 and 3. Precondition: every lane of the wave is active (all call sites are block-uniform).
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
  v = row_incl_scan(v);
  v += sm_dpp<kDppRowBcast15, 0xa>(0u, v);
  v += sm_dpp<kDppRowBcast31, 0xc>(0u, v);
  return v;
}

// Block-wide exclusive scan of one value per thread (NT threads, a multiple of 64, at most 1024; the default is the
// workgroup of the order kernels) in two halves, for a caller that has other work to put between them and owns the
// barrier: block_excl_waves scans within the wave and stores the wave's total to lw[wave] (NT / 64 words of LDS; it
// returns the lane's inclusive value, which the caller keeps); after a workgroup barrier block_excl_finish scans the
// wave totals, by every wave alike, in one 16-lane row (lane l holds wave l & 15), and returns the exclusive value and
// the total through *tot. The caller also fences lw's reuse (a barrier between the finish and the next scan on lw).
template <int NT = 1024>
__device__ __forceinline__ uint32_t block_excl_waves(uint32_t v, uint32_t* lw) {
  static_assert(NT % 64 == 0 && NT / 64 >= 1 && NT / 64 <= 16, "the wave totals fit one 16-lane row");
  const int lane = threadIdx.x & 63, w = wave_index();
  const uint32_t inc = wave_incl_scan(v);
  if (lane == 63) lw[w] = inc;
  return inc;
}
template <int NT = 1024>
__device__ __forceinline__ uint32_t block_excl_finish(uint32_t v, uint32_t inc, const uint32_t* lw, uint32_t* tot) {
  const int lane = threadIdx.x & 63, w = wave_index();
  const int q = lane & 15;
  const uint32_t ws = row_incl_scan(q < NT / 64 ? lw[q] : 0u);
  const uint32_t before = wave_read_lane(ws, w > 0 ? w - 1 : 0);
  *tot = wave_read_lane(ws, NT / 64 - 1);
  return inc - v + (w > 0 ? before : 0u);
}

// The two halves with their barrier between them: one barrier inside, between the write of lw and its reads.
template <int NT = 1024>
__device__ __forceinline__ uint32_t block_excl(uint32_t v, uint32_t* lw, uint32_t* tot) {
  const uint32_t inc = block_excl_waves<NT>(v, lw);
  lds_barrier();
  return block_excl_finish<NT>(v, inc, lw, tot);
}

__device__ __forceinline__ StackVal col_value(const NfaStream* st, int a, int64_t row) {
  StackVal v;
  v.i = 0;
  v.d = 0;
  v.null = 0;
  switch (st->types[a]) {
    case T_INT: v.i = ((const int32_t*)st->cols[a])[row]; break;
    case T_LONG: v.i = ((const int64_t*)st->cols[a])[row]; break;
    case T_FLOAT: v.d = (double)((const float*)st->cols[a])[row]; break;
    case T_DOUBLE: v.d = ((const double*)st->cols[a])[row]; break;
    case T_STRING: v.i = ((const int32_t*)st->cols[a])[row]; v.null = v.i < 0; break;
    default: v.i = ((const uint8_t*)st->cols[a])[row]; break;
  }
  return v;
}

// One attribute column resolved once per kernel (its pointer and type out of the NfaStream descriptor), so a loop
// of column reads does not reload the descriptor after every store (the compiler cannot prove the stores miss it)
struct ColRef {
  const void* p;
  int t;
  __device__ __forceinline__ StackVal at(int64_t row) const {
    StackVal v;
    v.i = 0;
    v.d = 0;
    v.null = 0;
    switch (t) {
      case T_INT: v.i = ((const int32_t*)p)[row]; break;
      case T_LONG: v.i = ((const int64_t*)p)[row]; break;
      case T_FLOAT: v.d = (double)((const float*)p)[row]; break;
      case T_DOUBLE: v.d = ((const double*)p)[row]; break;
      case T_STRING: v.i = ((const int32_t*)p)[row]; v.null = v.i < 0; break;
      default: v.i = ((const uint8_t*)p)[row]; break;
    }
    return v;
  }
};
__device__ __forceinline__ ColRef col_ref(const NfaStream* st, int a) { return ColRef{st->cols[a], st->types[a]}; }

// canonical 64-bit image of an attribute value (double bits for FLOAT/DOUBLE, integer otherwise)
__device__ __forceinline__ uint64_t canon(const StackVal& v, int type) {
  return (type == T_FLOAT || type == T_DOUBLE) ? (uint64_t)__double_as_longlong(v.d) : (uint64_t)v.i;
}
__device__ __forceinline__ StackVal uncanon(uint64_t bits, int type) {
  StackVal v;
  v.null = 0;
  if (type == T_FLOAT || type == T_DOUBLE) v.d = __longlong_as_double((long long)bits);
  else v.i = (int64_t)bits;
  return v;
}

// monotone 32-bit value code (see the header)
template <typename VT>
__device__ __forceinline__ uint32_t vcode(VT v, int mode, int64_t vmin) {
  if constexpr (std::is_same<VT, int32_t>::value) {
    return (uint32_t)v ^ 0x80000000u;
  } else if constexpr (std::is_same<VT, float>::value) {
    if (v != v) return kNanCode;
    const uint32_t b = v == 0.0f ? 0u : __float_as_uint(v);  // -0.0 == 0.0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  } else if constexpr (std::is_same<VT, double>::value) {
    if (v != v) return kNanCode;
    const uint64_t b = v == 0.0 ? 0ull : (uint64_t)__double_as_longlong(v);
    const uint64_t m = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    return (uint32_t)(m >> 32);
  } else {  // int64
    if (mode == VC_I64R) return (uint32_t)(v - vmin);
    return (uint32_t)(((uint64_t)v ^ 0x8000000000000000ull) >> 32);
  }
}

// A condition program decoded once per thread: its kernel-uniform instructions and constants stay in scalar
// registers across loops instead of being re-read every iteration.
struct Cond {
  const Instr* code;
  int len;
  const DVal* consts;
  bool simple;  // `x CMP y` with x, y variables or constants
  Instr a, b, op;
  StackVal ka, kb;
};

__device__ __forceinline__ StackVal const_val(const DVal* consts, int k) {
  const DVal c = consts[k];
  StackVal v;
  v.i = c.i;
  v.d = c.d;
  v.null = c.null;
  return v;
}

__device__ __forceinline__ Cond make_cond(const Instr* code, int len, const DVal* consts) {
  Cond c;
  c.code = code;
  c.len = len;
  c.consts = consts;
  c.simple = len == 3 && code[2].op == OP_CMP && code[0].op != OP_CMP && code[1].op != OP_CMP &&
             code[0].op != OP_MATH && code[1].op != OP_MATH && code[0].op != OP_NOT && code[1].op != OP_NOT;
  if (c.simple) {
    c.a = code[0];
    c.b = code[1];
    c.op = code[2];
    if (c.a.op == OP_CONST) c.ka = const_val(consts, c.a.a);
    if (c.b.op == OP_CONST) c.kb = const_val(consts, c.b.a);
  }
  return c;
}

template <typename Ld>
__device__ __forceinline__ bool eval(const Cond& c, const Ld& ld) {
  if (c.len == 0) return true;
  if (c.simple) {
    const StackVal l = c.a.op == OP_CONST ? c.ka : ld.var(c.a);
    const StackVal r = c.b.op == OP_CONST ? c.kb : ld.var(c.b);
    if (l.null || r.null) return c.op.sub == CMP_NE;
    return do_compare(c.op, l, r);
  }
  return truthy(eval_prog(c.code, c.len, c.consts, ld));
}

// c.simple (or empty) conditions only: no interpreter stack in the caller
template <typename Ld>
__device__ __forceinline__ bool eval_simple(const Cond& c, const Ld& ld) {
  if (c.len == 0) return true;
  const StackVal l = c.a.op == OP_CONST ? c.ka : ld.var(c.a);
  const StackVal r = c.b.op == OP_CONST ? c.kb : ld.var(c.b);
  if (l.null || r.null) return c.op.sub == CMP_NE;
  return do_compare(c.op, l, r);
}

template <int OP, typename T>
__device__ __forceinline__ bool cmp_fixed(T x, T y) {
  if constexpr (OP == CMP_EQ) return x == y;
  else if constexpr (OP == CMP_NE) return x != y;
  else if constexpr (OP == CMP_LT) return x < y;
  else if constexpr (OP == CMP_LE) return x <= y;
  else if constexpr (OP == CMP_GT) return x > y;
  else return x >= y;
}

// e1-only program on an original row (c1)
struct RowLoader {
  const NfaStream* st;
  int64_t row;
  __device__ StackVal var(const Instr& in) const {
    if (in.op == OP_COL) return col_value(st, in.a, row);
    return col_value(st, in.c, row);
  }
};

// c2 over the carried attribute: slot 0 = e1, slot 1 = e2 (host checked every variable reads `vattr`)
struct PairLoader {
  uint64_t v1, v2;
  int type;
  __device__ StackVal var(const Instr& in) const { return uncanon(in.a == 0 ? v1 : v2, type); }
};

// Unkeyed walk: c2 on canonical 64-bit values, as a fixed compare `e2.x OP e1.x` (OP >= 0; FP: compared as
// double, else as int64) or the generic condition program (OP < 0).
template <int OP, bool FP>
struct C2 {
  Cond c;
  int vtype;
  __device__ __forceinline__ bool operator()(uint64_t v1, uint64_t v2) const {
    if constexpr (OP < 0) {
      return eval(c, PairLoader{v1, v2, vtype});
    } else {
      if constexpr (FP) return cmp_fixed<OP>(__longlong_as_double((long long)v2), __longlong_as_double((long long)v1));
      else return cmp_fixed<OP>((int64_t)v2, (int64_t)v1);
    }
  }
};

// Keyed walk: c2 = `e2.x OP e1.x` on value codes; equal inexact codes and NaN go to the exact column values.
template <int OP, bool FP>
struct C2Code {
  bool exact_codes;  // the code mode is exact (INT, FLOAT, rebased LONG)
  int vtype;
  const void* vcol;
  const int64_t* ord;  // ordinals of the batch rows (nullptr: row = relative ordinal)
  int64_t obase, n;
  __device__ int64_t row_of(uint32_t o) const {  // rows are in ordinal order
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
  __device__ bool exact(uint32_t o1, uint32_t o2) const {
    const int64_t r1 = row_of(o1), r2 = row_of(o2);
    if constexpr (FP) {
      double x1, x2;
      if (vtype == T_FLOAT) {
        x1 = ((const float*)vcol)[r1];
        x2 = ((const float*)vcol)[r2];
      } else {
        x1 = ((const double*)vcol)[r1];
        x2 = ((const double*)vcol)[r2];
      }
      return cmp_fixed<OP>(x2, x1);
    } else {
      int64_t x1, x2;
      if (vtype == T_INT) {
        x1 = ((const int32_t*)vcol)[r1];
        x2 = ((const int32_t*)vcol)[r2];
      } else {
        x1 = ((const int64_t*)vcol)[r1];
        x2 = ((const int64_t*)vcol)[r2];
      }
      return cmp_fixed<OP>(x2, x1);
    }
  }
  __device__ __forceinline__ bool operator()(uint32_t c1, uint32_t o1, uint32_t c2, uint32_t o2) const {
    if (!needs_exact(c1, c2)) return cmp_fixed<OP>(c2, c1);
    return exact(o1, o2);
  }
  // the codes alone do not decide the comparison (equal inexact codes, or a NaN)
  __device__ __forceinline__ bool needs_exact(uint32_t c1, uint32_t c2) const {
    const bool nan = FP & ((c1 == kNanCode) | (c2 == kNanCode));
    return nan | (!exact_codes & (c1 == c2));
  }
};

// Chunk g of a pass: [g * per, g * per + len_g); len_g = seg_len[g] when given, else the uniform split of n.
__device__ __forceinline__ void chunk_range(int g, int64_t n, int64_t per, const uint32_t* seg_len, int64_t& lo,
                                            int64_t& len) {
  lo = (int64_t)g * per;
  if (seg_len) {
    len = seg_len[g];
  } else {
    len = n - lo;
    if (len > per) len = per;
    if (len < 0) len = 0;
  }
}

}  // namespace
}  // namespace sm
