// Host entry of the adjacent-pair closed form of `every e1=S[c1], e2=S[c2] [within T]` (seq_dev.h has the rule and
// the kernels). Per batch:
//   facts   one streaming pass over the key column, event times and ordinals: key range, decreasing event time,
//           ordinals that do not fit (the only host round trip before the carry is touched)
//   keyed   stable LSD sort of (key - kmin, row) (primitives.hip), so each event's predecessor is its left neighbour
//   link    seq_link_kernel: e1 (or none) at every e2's row, carry-out candidates, carried rows that saw an event
//   emit    tile counts (from the link pass in row order, seq_count_kernel after a key sort), their scan, then the
//           pairs in row order; each e2 has at most one pair, so this is the reference's order and nothing is sorted
//   carry   one row per key whose last event passes c1 (build_carry); keys without events keep their row
// Further down: the k-state sibling (fast_seq_k), the same form over several streams (fast_seq_ms, mseq_dev.h) and the
// pattern `every e1=A -> e2=B within T` over two streams (fast_pat_ms, mpat_dev.h).
#include "fastpath.h"
#include "mpat_dev.h"
#include "mseq_dev.h"
#include "seq_dev.h"

namespace sm {

namespace {

struct SeqFacts {
  unsigned long long kmin, kmax;  // sign-biased key range
  unsigned int bad_ts, bad_ord, bad_carry, pad;
  long long o0, omax;             // relative ordinals of the first and the last event
  long long ts0, ts_last;
};

constexpr int kFactsBlock = 256;

template <typename KT>
__global__ void __launch_bounds__(kFactsBlock) seq_facts_kernel(const KT* __restrict__ kcol,
                                                                const int64_t* __restrict__ ts,
                                                                const int64_t* __restrict__ ord, int64_t obase,
                                                                int64_t n, SeqFacts* __restrict__ f) {
  uint64_t lo = ~0ull, hi = 0;
  bool bts = false, bord = false;
  for (int64_t i = (int64_t)blockIdx.x * kFactsBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kFactsBlock) {
    if (kcol) {
      const uint64_t u = (uint64_t)(int64_t)kcol[i] ^ 0x8000000000000000ull;
      lo = u < lo ? u : lo;
      hi = u > hi ? u : hi;
    }
    const int64_t t = ts[i];
    if (i > 0) bts |= t < ts[i - 1];
    if (ord && i > 0) bord |= ord[i] <= ord[i - 1];
    if (i == 0) {
      f->ts0 = t;
      f->o0 = ord ? ord[0] - obase : 0;
    }
    if (i == n - 1) {
      f->ts_last = t;
      f->omax = ord ? ord[i] - obase : i;
    }
  }
  if (kcol) {
    for (int o = 32; o > 0; o >>= 1) {
      const uint64_t x = __shfl_down(lo, o, 64), y = __shfl_down(hi, o, 64);
      lo = x < lo ? x : lo;
      hi = y > hi ? y : hi;
    }
    if ((threadIdx.x & 63) == 0 && hi >= lo) {
      atomicMin(&f->kmin, (unsigned long long)lo);
      atomicMax(&f->kmax, (unsigned long long)hi);
    }
  }
  const bool any_ts = __any(bts), any_ord = __any(bord);
  if ((threadIdx.x & 63) == 0) {
    if (any_ts) atomicOr(&f->bad_ts, 1u);
    if (any_ord) atomicOr(&f->bad_ord, 1u);
  }
}

// carried e1 ordinals must lie in (base - 2^31, base): pair_project tells them from batch rows by their sign
__global__ void seq_carry_check_kernel(const int64_t* __restrict__ rows, int64_t nc, int cw, int64_t obase,
                                       SeqFacts* __restrict__ f) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int64_t o = rows[c * cw + 1] - obase;
  if (o >= 0 || o <= (int64_t)INT32_MIN) atomicOr(&f->bad_carry, 1u);
}

template <typename KT, typename K>
__global__ void seq_sort_keys_kernel(const KT* __restrict__ kcol, int64_t n, int64_t kmin, K* __restrict__ sk,
                                     uint32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  sk[i] = (K)((uint64_t)(int64_t)kcol[i] - (uint64_t)kmin);
  idx[i] = (uint32_t)i;
}

inline dim3 seq_grid(int64_t n, int t) { return dim3((unsigned)std::max<int64_t>(1, (n + t - 1) / t)); }

int bits_of(uint64_t x) {
  int b = 0;
  while (b < 64 && (x >> b) != 0) ++b;
  return b;
}

// rows in (key, arrival) order: a stable LSD sort of (key - kmin, row) over the key's significant bits
void seq_sort_rows(const void* kcol, bool key64, int64_t n, int64_t kmin, int kbits, Scratch& sc, hipStream_t s,
                   const uint32_t** perm, const void** skey) {
  const bool wide = kbits > 32;
  uint32_t* si = (uint32_t*)sc.take((size_t)n * 4);
  uint32_t* si2 = (uint32_t*)sc.take((size_t)n * 4);
  const dim3 g = seq_grid(n, 256);
  if (wide) {
    uint64_t* sk = (uint64_t*)sc.take((size_t)n * 8);
    uint64_t* sk2 = (uint64_t*)sc.take((size_t)n * 8);
    hipLaunchKernelGGL((seq_sort_keys_kernel<int64_t, uint64_t>), g, dim3(256), 0, s, (const int64_t*)kcol, n, kmin,
                       sk, si);
    const bool alt = radix_sort_pairs<uint64_t>(sk, sk2, si, si2, (size_t)n, 0, kbits, sc, s);
    *skey = alt ? sk2 : sk;
    *perm = alt ? si2 : si;
  } else {
    uint32_t* sk = (uint32_t*)sc.take((size_t)n * 4);
    uint32_t* sk2 = (uint32_t*)sc.take((size_t)n * 4);
    if (key64)
      hipLaunchKernelGGL((seq_sort_keys_kernel<int64_t, uint32_t>), g, dim3(256), 0, s, (const int64_t*)kcol, n, kmin,
                         sk, si);
    else
      hipLaunchKernelGGL((seq_sort_keys_kernel<int32_t, uint32_t>), g, dim3(256), 0, s, (const int32_t*)kcol, n, kmin,
                         sk, si);
    const bool alt = radix_sort_pairs<uint32_t>(sk, sk2, si, si2, (size_t)n, 0, kbits, sc, s);
    *skey = alt ? sk2 : sk;
    *perm = alt ? si2 : si;
  }
}

}  // namespace

int64_t fast_seq_adjacent(const FastArgs& a, const FastHostInfo& hi, FastState& fs, FastCarry& carry,
                          uint32_t* pairs_out, int64_t pairs_cap, Scratch& sc, hipStream_t s, FastTimings* tm) {
  const int64_t n = a.n;
  if (n == 0) return 0;
  if (n >= 0x7fffffffll) return FAST_OUTSIDE;
  const bool keyed = a.key != nullptr;
  if (keyed && (hi.key_col < 0 || !(hi.key_type == T_INT || hi.key_type == T_LONG))) return FAST_OUTSIDE;
  const size_t mark = sc.used;
  if (tm) {
    SM_HIP(hipEventRecord(tm->ev[0], s));
    tm->nmk = 0;
    tm->mark("start", s);
  }
  auto tmark = [&](const char* l) {
    if (tm) tm->mark(l, s);
  };
  const void* kcol = keyed ? (hi.dense_keys ? (const void*)hi.dense_keys : hi.cols[hi.key_col]) : nullptr;
  const bool key64 = keyed && !hi.dense_keys && hi.key_type == T_LONG;
  const int nattr = hi.nattr, cw = 3 + nattr;
  const int64_t nc = carry.n;

  // ---- facts: nothing is changed before they are read
  SeqFacts* f = (SeqFacts*)sc.take(sizeof(SeqFacts));
  {
    SeqFacts init{};
    init.kmin = ~0ull;
    SM_HIP(hipMemcpyAsync(f, &init, sizeof(SeqFacts), hipMemcpyHostToDevice, s));
  }
  const dim3 fgrid((unsigned)std::min<int64_t>(2048, (n + kFactsBlock - 1) / kFactsBlock));
  if (key64)
    hipLaunchKernelGGL(seq_facts_kernel<int64_t>, fgrid, dim3(kFactsBlock), 0, s, (const int64_t*)kcol, a.ts, a.ordinals,
                       a.ordinal_base, n, f);
  else
    hipLaunchKernelGGL(seq_facts_kernel<int32_t>, fgrid, dim3(kFactsBlock), 0, s, (const int32_t*)kcol, a.ts, a.ordinals,
                       a.ordinal_base, n, f);
  if (nc > 0)
    hipLaunchKernelGGL(seq_carry_check_kernel, seq_grid(nc, 256), dim3(256), 0, s, (const int64_t*)carry.rows, nc,
                       carry.width, a.ordinal_base, f);
  tmark("seq_facts");
  SeqFacts h;
  SM_HIP(hipMemcpyAsync(&h, f, sizeof(SeqFacts), hipMemcpyDeviceToHost, s));
  SM_HIP(hipStreamSynchronize(s));
  auto leave = [&](int64_t r) {
    sc.used = mark;
    return r;
  };
  // with a within, a partial older than T is dropped only because event time never goes back
  if (a.within >= 0 && (h.bad_ts || (carry.active && h.ts0 < carry.ts_last))) return leave(FAST_NON_MONOTONE);
  if (h.bad_ord || h.bad_carry || h.o0 < 0 || h.omax >= 0x7fffffffll) return leave(FAST_OUTSIDE);
  if (nc > 0 && carry.width != cw) return leave(FAST_OUTSIDE);
  int64_t kmin = 0;
  int kbits = 0;
  if (keyed) {
    kmin = (int64_t)(h.kmin ^ 0x8000000000000000ull);
    const uint64_t kspan = (uint64_t)((int64_t)(h.kmax ^ 0x8000000000000000ull) - kmin);
    kbits = std::max(1, bits_of(kspan));
    // a query's first batch decides between key values and dense ids when the caller offers them (remap_span: it
    // gives the ids and runs the batch again); once rows are carried their keys stay what they are: any span is sorted
    if (!carry.active && hi.remap_span > 0 && (kbits > 30 || kspan > (uint64_t)hi.remap_span))
      return leave(FAST_KEY_SPAN);
  }

  // what the carry-out reads lies first, so that the rest is free again when build_carry runs
  const int64_t cand_cap = n + nc;
  {  // scratch for the worst case, before anything changes: sort pairs + links, then the carry build per candidate
    const uint64_t kmax_runs = keyed ? (kbits >= 62 ? (uint64_t)n : std::min<uint64_t>((uint64_t)n, (1ull << kbits))) : 1;
    // sort pairs twice over (+ a histogram word per 4 events), links, tile counts
    const size_t link = (size_t)n * (keyed ? (kbits > 32 ? 29 : 21) : 4) + (size_t)(n / kSeqTile + 2) * 4 + (8 << 20);
    const size_t build = (size_t)(kmax_runs + (uint64_t)nc) * (size_t)(8 * cw + 44) + (8 << 20);
    if (sc.used + (size_t)cand_cap * 32 + (size_t)nc + std::max(link, build) + 4096 > sc.cap) return leave(FAST_OUTSIDE);
  }
  uint32_t* ctl = (uint32_t*)sc.take(8);  // [0] candidates, [1] pairs
  uint8_t* used = (uint8_t*)sc.take((size_t)std::max<int64_t>(nc, 1));
  int64_t* cand = (int64_t*)sc.take((size_t)cand_cap * 32);
  const size_t keep = sc.used;

  // ---- keyed: rows in (key, arrival) order
  const uint32_t* perm = nullptr;
  const void* skey = nullptr;
  const bool wide = kbits > 32;
  if (keyed) {
    seq_sort_rows(kcol, key64, n, kmin, kbits, sc, s, &perm, &skey);
    tmark("seq_sort");
  }
  if (tm) SM_HIP(hipEventRecord(tm->ev[1], s));

  // ---- link
  const int64_t ntiles = (n + kSeqTile - 1) / kSeqTile;
  SM_HIP(hipMemsetAsync(ctl, 0, 8, s));
  if (nc > 0) SM_HIP(hipMemsetAsync(used, 0, (size_t)nc, s));
  SeqArgs sa{};
  sa.n = n;
  sa.ts = a.ts;
  sa.st = a.st;
  sa.code = a.code;
  sa.consts = a.consts;
  sa.c1_off = a.c1_off;
  sa.c1_len = a.c1_len;
  sa.c2_off = a.c2_off;
  sa.c2_len = a.c2_len;
  sa.within = a.within;
  sa.ordinals = a.ordinals;
  sa.obase = a.ordinal_base;
  sa.perm = perm;
  sa.skey = skey;
  sa.kmin = kmin;
  sa.carry = (const int64_t*)carry.rows;
  sa.nc = nc;
  sa.cw = cw;
  sa.e1 = (int32_t*)sc.take((size_t)n * 4);
  sa.used = used;
  sa.cand = cand;
  sa.cand_n = ctl;
  uint32_t* counts = (uint32_t*)sc.take((size_t)(ntiles + 1) * 4);
  sa.counts = keyed ? nullptr : counts;
  if (wide) hipLaunchKernelGGL(seq_link_kernel<uint64_t>, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, sa);
  else hipLaunchKernelGGL(seq_link_kernel<uint32_t>, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, sa);
  tmark("seq_link");
  if (nc > 0) {
    hipLaunchKernelGGL(seq_keep_kernel, seq_grid(nc, kSeqBlock), dim3(kSeqBlock), 0, s, (const int64_t*)carry.rows, nc, cw,
                       (const uint8_t*)used, sa.cand, ctl);
    tmark("seq_keep");
  }
  if (tm) SM_HIP(hipEventRecord(tm->ev[2], s));

  // ---- pairs in row order
  if (keyed) {
    hipLaunchKernelGGL(seq_count_kernel, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, (const int32_t*)sa.e1, n, counts);
    tmark("seq_count");
  }
  exclusive_scan_u32(counts, (size_t)ntiles, sc, s, ctl + 1);
  tmark("seq_scan");
  hipLaunchKernelGGL(seq_emit_kernel, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, (const int32_t*)sa.e1, n,
                     (const uint32_t*)counts, a.ordinals, a.ordinal_base, pairs_out);
  tmark("seq_emit");
  uint32_t hc[2] = {0, 0};
  SM_HIP(hipMemcpyAsync(hc, ctl, 8, hipMemcpyDeviceToHost, s));
  SM_HIP(hipStreamSynchronize(s));
  const int64_t m = hc[1];
  if (m > pairs_cap || (int64_t)hc[0] > cand_cap) {  // cannot happen (m <= n <= pairs_cap): checked, not assumed
    sc.used = mark;
    throw std::runtime_error("adjacent-pair closed form: output larger than its buffer");
  }

  // ---- carry out (build_carry reads the old rows before it replaces them)
  sc.used = keep;
  build_carry(sa.cand, (int64_t)hc[0], a.st, nattr, carry, sc, s, 64, 0, true);
  tmark("seq_carry");
  carry.ts_last = carry.active ? std::max<int64_t>(carry.ts_last, h.ts_last) : (int64_t)h.ts_last;
  carry.active = true;
  fs.last_path = 6;
  if (tm) SM_HIP(hipEventRecord(tm->ev[3], s));
  sc.used = mark;
  return m;
}

// The k-state sibling (seq_dev.h, second half). Per batch: facts and key sort as above, then
//   seqk_link    predecessor link and hit at every row, carry-out candidates (the last k - 1 rows of every run)
//   seqk_keep    carried rows that stay
//   seqk_count / seqk_scan / seqk_emit   k-tuples in row order of the last event
//   seqk_carry   build_carry over the candidates, sorted by ordinal then key (several rows per key; the candidates'
//                order, which depends on the order of atomics, is not read)
int64_t fast_seq_k(const FastArgs& a, const SeqKPlan& p, const FastHostInfo& hi, FastState& fs, FastCarry& carry,
                   uint32_t* tuples_out, int64_t tuples_cap, Scratch& sc, hipStream_t s, FastTimings* tm) {
  const int64_t n = a.n;
  const int k = p.k;
  if (k < 3 || k > kSeqKMax) return FAST_OUTSIDE;
  if (n == 0) return 0;
  if (n >= 0x7fffffffll) return FAST_OUTSIDE;
  const bool keyed = a.key != nullptr;
  if (keyed && (hi.key_col < 0 || !(hi.key_type == T_INT || hi.key_type == T_LONG))) return FAST_OUTSIDE;
  const size_t mark = sc.used;
  if (tm) {
    SM_HIP(hipEventRecord(tm->ev[0], s));
    tm->nmk = 0;
    tm->mark("start", s);
  }
  auto tmark = [&](const char* l) {
    if (tm) tm->mark(l, s);
  };
  const void* kcol = keyed ? (hi.dense_keys ? (const void*)hi.dense_keys : hi.cols[hi.key_col]) : nullptr;
  const bool key64 = keyed && !hi.dense_keys && hi.key_type == T_LONG;
  const int nattr = hi.nattr, cw = 3 + nattr;
  const int64_t nc = carry.n;
  bool any_within = false;
  for (int m = 1; m < k; ++m) any_within |= p.within[m] >= 0;

  // ---- facts: nothing is changed before they are read
  SeqFacts* f = (SeqFacts*)sc.take(sizeof(SeqFacts));
  {
    SeqFacts init{};
    init.kmin = ~0ull;
    SM_HIP(hipMemcpyAsync(f, &init, sizeof(SeqFacts), hipMemcpyHostToDevice, s));
  }
  const dim3 fgrid((unsigned)std::min<int64_t>(2048, (n + kFactsBlock - 1) / kFactsBlock));
  if (key64)
    hipLaunchKernelGGL(seq_facts_kernel<int64_t>, fgrid, dim3(kFactsBlock), 0, s, (const int64_t*)kcol, a.ts, a.ordinals,
                       a.ordinal_base, n, f);
  else
    hipLaunchKernelGGL(seq_facts_kernel<int32_t>, fgrid, dim3(kFactsBlock), 0, s, (const int32_t*)kcol, a.ts, a.ordinals,
                       a.ordinal_base, n, f);
  if (nc > 0)
    hipLaunchKernelGGL(seq_carry_check_kernel, seq_grid(nc, 256), dim3(256), 0, s, (const int64_t*)carry.rows, nc,
                       carry.width, a.ordinal_base, f);
  tmark("seqk_facts");
  SeqFacts h;
  SM_HIP(hipMemcpyAsync(&h, f, sizeof(SeqFacts), hipMemcpyDeviceToHost, s));
  SM_HIP(hipStreamSynchronize(s));
  auto leave = [&](int64_t r) {
    sc.used = mark;
    return r;
  };
  if (any_within && (h.bad_ts || (carry.active && h.ts0 < carry.ts_last))) return leave(FAST_NON_MONOTONE);
  if (h.bad_ord || h.bad_carry || h.o0 < 0 || h.omax >= 0x7fffffffll) return leave(FAST_OUTSIDE);
  if (nc > 0 && carry.width != cw) return leave(FAST_OUTSIDE);
  if (n > tuples_cap) return leave(FAST_OUTSIDE);
  int64_t kmin = 0, kmax = 0;
  int kbits = 0;
  if (keyed) {
    kmin = (int64_t)(h.kmin ^ 0x8000000000000000ull);
    kmax = (int64_t)(h.kmax ^ 0x8000000000000000ull);
    const uint64_t kspan = (uint64_t)(kmax - kmin);
    kbits = std::max(1, bits_of(kspan));
    if (!carry.active && hi.remap_span > 0 && (kbits > 30 || kspan > (uint64_t)hi.remap_span))
      return leave(FAST_KEY_SPAN);
  }

  // what the carry-out reads lies first, so that the rest is free again when build_carry runs
  const int64_t cand_cap = n + nc;
  const int64_t ntiles = (n + kSeqTile - 1) / kSeqTile;
  {  // scratch for the worst case, before anything changes
    const uint64_t runs = keyed ? (kbits >= 62 ? (uint64_t)n : std::min<uint64_t>((uint64_t)n, (1ull << kbits))) : 1;
    const uint64_t ncand_max = std::min<uint64_t>((uint64_t)n, runs * (uint64_t)(k - 1)) + (uint64_t)nc;
    // sort pairs twice over (+ a histogram word per 4 events), links and hits, tile counts
    const size_t link = (size_t)n * (keyed ? (kbits > 32 ? 30 : 22) : 5) + (size_t)(ntiles + 2) * 4 + (8 << 20);
    const size_t build = (size_t)ncand_max * (size_t)(8 * cw + 44) + (8 << 20);
    if (sc.used + (size_t)cand_cap * 32 + std::max(link, build) + 4096 > sc.cap) return leave(FAST_OUTSIDE);
  }
  uint32_t* ctl = (uint32_t*)sc.take(8);  // [0] candidates, [1] tuples
  int64_t* cand = (int64_t*)sc.take((size_t)cand_cap * 32);
  const size_t keep = sc.used;

  const uint32_t* perm = nullptr;
  const void* skey = nullptr;
  const bool wide = kbits > 32;
  if (keyed) {
    seq_sort_rows(kcol, key64, n, kmin, kbits, sc, s, &perm, &skey);
    tmark("seqk_sort");
  }
  if (tm) SM_HIP(hipEventRecord(tm->ev[1], s));

  // ---- link
  SM_HIP(hipMemsetAsync(ctl, 0, 8, s));
  SeqKArgs sa{};
  sa.n = n;
  sa.ts = a.ts;
  sa.st = a.st;
  sa.code = a.code;
  sa.consts = a.consts;
  sa.k = k;
  for (int m = 0; m < kSeqKMax; ++m) {
    sa.off[m] = m < k ? p.off[m] : 0;
    sa.len[m] = m < k ? p.len[m] : 0;
    sa.within[m] = m > 0 && m < k ? p.within[m] : -1;
  }
  sa.ordinals = a.ordinals;
  sa.obase = a.ordinal_base;
  sa.perm = perm;
  sa.skey = skey;
  sa.kmin = kmin;
  sa.kmax = kmax;
  sa.carry = (const int64_t*)carry.rows;
  sa.nc = nc;
  sa.cw = cw;
  sa.prev = (int32_t*)sc.take((size_t)n * 4);
  sa.hit = (uint8_t*)sc.take(((size_t)n + 3) & ~(size_t)3);
  sa.cand = cand;
  sa.cand_n = ctl;
  uint32_t* counts = (uint32_t*)sc.take((size_t)(ntiles + 1) * 4);
  if (wide) hipLaunchKernelGGL(seqk_link_kernel<uint64_t>, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, sa);
  else hipLaunchKernelGGL(seqk_link_kernel<uint32_t>, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, sa);
  tmark("seqk_link");
  if (nc > 0) {
    if (wide) hipLaunchKernelGGL(seqk_keep_kernel<uint64_t>, seq_grid(nc, kSeqBlock), dim3(kSeqBlock), 0, s, sa);
    else hipLaunchKernelGGL(seqk_keep_kernel<uint32_t>, seq_grid(nc, kSeqBlock), dim3(kSeqBlock), 0, s, sa);
    tmark("seqk_keep");
  }
  if (tm) SM_HIP(hipEventRecord(tm->ev[2], s));

  // ---- tuples in row order
  hipLaunchKernelGGL(seqk_count_kernel, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, (const uint8_t*)sa.hit, n, counts);
  tmark("seqk_count");
  exclusive_scan_u32(counts, (size_t)ntiles, sc, s, ctl + 1);
  tmark("seqk_scan");
  hipLaunchKernelGGL(seqk_emit_kernel, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, (const uint8_t*)sa.hit,
                     (const int32_t*)sa.prev, n, k, (const uint32_t*)counts, a.ordinals, a.ordinal_base,
                     (const int64_t*)carry.rows, cw, tuples_out);
  tmark("seqk_emit");
  uint32_t hc[2] = {0, 0};
  SM_HIP(hipMemcpyAsync(hc, ctl, 8, hipMemcpyDeviceToHost, s));
  SM_HIP(hipStreamSynchronize(s));
  const int64_t m = hc[1];
  if (m > tuples_cap || (int64_t)hc[0] > cand_cap) {  // cannot happen (m <= n <= tuples_cap): checked, not assumed
    sc.used = mark;
    throw std::runtime_error("adjacent-run closed form: output larger than its buffer");
  }

  // ---- carry out (build_carry reads the old rows before it replaces them)
  sc.used = keep;
  build_carry(sa.cand, (int64_t)hc[0], a.st, nattr, carry, sc, s);
  tmark("seqk_carry");
  carry.ts_last = carry.active ? std::max<int64_t>(carry.ts_last, h.ts_last) : (int64_t)h.ts_last;
  carry.active = true;
  fs.last_path = 7;
  if (tm) SM_HIP(hipEventRecord(tm->ev[3], s));
  sc.used = mark;
  return m;
}

namespace {

__global__ void mseq_carry_check_kernel(const int64_t* __restrict__ rows, int64_t nc, int cw, int64_t obase,
                                        MSeqFacts* __restrict__ f) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int64_t o = rows[c * cw + 1] - obase;
  if (o >= 0 || o <= (int64_t)INT32_MIN) atomicOr(&f->bad_carry, 1u);
}

__global__ void mseq_keys_kernel(MSeqSrc s, int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.n) return;
  const int32_t sd = s.sid[i];
  keys[i] = mseq_read(s, sd) ? mseq_key(s, sd, i) : 0;
}

MSeqSrc mseq_src(int64_t n, const int32_t* sid, const MSeqPlan& p) {
  MSeqSrc src{};
  src.n = n;
  src.sid = sid;
  src.read = p.read;
  for (int q = 0; q < kMSeqStreams; ++q) src.kcol[q] = p.keyed ? p.kcol[q] : nullptr;
  src.wide = p.wide;
  return src;
}

}  // namespace

void mseq_gather_keys(int64_t n, const int32_t* sid, const MSeqPlan& p, int64_t* keys, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(mseq_keys_kernel, seq_grid(n, 256), dim3(256), 0, s, mseq_src(n, sid, p), keys);
}

// The same form over several streams of one schema on an interleaved batch (mseq_dev.h). Per batch:
//   mseq_facts   read rows per tile; over the read rows: key range, decreasing event time, ordinals (the only host round
//                trip before anything is changed)
//   mseq_pack    the read rows in row order as (key - kmin, row) sort pairs + a stream byte per packed position
//                (skipped when every row is read and the query is unkeyed)
//   mseq_sort    keyed: the stable LSD sort of the pairs, then the stream byte of every sorted position
//   mseq_link    stream bytes, withins, conditions: hit and predecessor link at every read row, carry-out candidates
//   mseq_keep / mseq_count / mseq_scan / mseq_emit / mseq_carry   as fast_seq_k, k = 2 included
int64_t fast_seq_ms(const FastArgs& a, const int32_t* sid, const MSeqPlan& p, int nattr, FastState& fs,
                    FastCarry& carry, uint32_t* tuples_out, int64_t tuples_cap, Scratch& sc, hipStream_t s,
                    FastTimings* tm) {
  const int64_t n = a.n;
  const int k = p.k;
  if (k < 2 || k > kSeqKMax) return FAST_OUTSIDE;
  if (n == 0) return 0;
  if (n >= 0x7fffffffll) return FAST_OUTSIDE;
  const bool keyed = p.keyed;
  const size_t mark = sc.used;
  if (tm) {  // (the entry point's own marks come first: the first label here times from the last of them)
    SM_HIP(hipEventRecord(tm->ev[0], s));
    if (tm->nmk == 0) tm->mark("start", s);
  }
  auto tmark = [&](const char* l) {
    if (tm) tm->mark(l, s);
  };
  const int cw = 4 + nattr;
  const int64_t nc = carry.n;
  bool any_within = false;
  for (int m = 1; m < k; ++m) any_within |= p.within[m] >= 0;
  const int64_t ntiles = (n + kSeqTile - 1) / kSeqTile;

  MSeqSrc src = mseq_src(n, sid, p);
  src.ts = a.ts;
  src.ordinals = a.ordinals;
  src.obase = a.ordinal_base;

  // ---- facts: nothing is changed before they are read
  MSeqFacts* f = (MSeqFacts*)sc.take(sizeof(MSeqFacts));
  uint32_t* tile_n = (uint32_t*)sc.take((size_t)(ntiles + 1) * 4);
  SM_HIP(hipMemsetAsync(f, 0, sizeof(MSeqFacts), s));
  hipLaunchKernelGGL(mseq_facts_kernel, dim3((unsigned)std::min<int64_t>(ntiles, 2048)), dim3(kSeqBlock), 0, s, src,
                     ntiles, tile_n, f);
  if (nc > 0)
    hipLaunchKernelGGL(mseq_carry_check_kernel, seq_grid(nc, 256), dim3(256), 0, s, (const int64_t*)carry.rows, nc,
                       carry.width, a.ordinal_base, f);
  tmark("mseq_facts");
  MSeqFacts h;
  SM_HIP(hipMemcpyAsync(&h, f, sizeof(MSeqFacts), hipMemcpyDeviceToHost, s));
  SM_HIP(hipStreamSynchronize(s));
  auto leave = [&](int64_t r) {
    sc.used = mark;
    return r;
  };
  constexpr uint64_t kBias = 0x8000000000000000ull;
  const int64_t np = (int64_t)h.nread;
  const int64_t ts0 = (int64_t)(~h.tmin_c ^ kBias), ts_last = (int64_t)(h.tmax ^ kBias);
  const int64_t o0 = (int64_t)(~h.omin_c ^ kBias), omax = (int64_t)(h.omax ^ kBias);
  if (any_within && np > 0 && (h.bad_ts || (carry.active && ts0 < carry.ts_last))) return leave(FAST_NON_MONOTONE);
  if (h.bad_ord || h.bad_carry || (np > 0 && (o0 < 0 || omax >= 0x7fffffffll))) return leave(FAST_OUTSIDE);
  if (nc > 0 && carry.width != cw) return leave(FAST_OUTSIDE);
  if (np > tuples_cap) return leave(FAST_OUTSIDE);
  if (np == 0) {  // no row of a stream the query reads: its carried rows wait
    fs.last_path = 8;
    return leave(0);
  }
  int64_t kmin = 0, kmax = 0;
  int kbits = 0;
  if (keyed) {
    kmin = (int64_t)(~h.kmin_c ^ kBias);
    kmax = (int64_t)(h.kmax ^ kBias);
    const uint64_t kspan = (uint64_t)(kmax - kmin);
    kbits = std::max(1, bits_of(kspan));
    if (!carry.active && p.remap_span > 0 && (kbits > 30 || kspan > (uint64_t)p.remap_span)) return leave(FAST_KEY_SPAN);
  }
  const bool wide = kbits > 32;
  const bool packed = keyed || np < n;

  // what the carry-out reads lies first, so that the rest is free again when build_carry runs
  const int64_t cand_cap = np + nc;
  const int64_t ptiles = (np + kSeqTile - 1) / kSeqTile;
  {  // scratch for the worst case, before anything changes
    const uint64_t runs = keyed ? (kbits >= 62 ? (uint64_t)np : std::min<uint64_t>((uint64_t)np, (1ull << kbits))) : 1;
    const uint64_t ncand_max = std::min<uint64_t>((uint64_t)np, runs * (uint64_t)(k - 1)) + (uint64_t)nc;
    // per read row: sort pairs twice over (+ a histogram word per 4 events) and a stream byte; per row: link and hit
    const size_t link = (size_t)np * (keyed ? (wide ? 26 : 18) : 5) + (size_t)n * 5 + (size_t)(ntiles + 2) * 8 + (8 << 20);
    const size_t build = (size_t)ncand_max * (size_t)(8 * cw + 44) + (8 << 20);
    if (sc.used + (size_t)cand_cap * 32 + std::max(link, build) + 4096 > sc.cap) return leave(FAST_OUTSIDE);
  }
  uint32_t* ctl = (uint32_t*)sc.take(8);  // [0] candidates, [1] tuples
  int64_t* cand = (int64_t*)sc.take((size_t)cand_cap * 32);
  const size_t keep = sc.used;

  // ---- the read rows, then (keyed) in (key, arrival) order
  const uint32_t* perm = nullptr;
  const void* skey = nullptr;
  const uint8_t* sstr = nullptr;
  if (packed) {
    exclusive_scan_u32(tile_n, (size_t)ntiles, sc, s);
    MSeqPack pa{};
    pa.s = src;
    pa.tile_off = tile_n;
    pa.kmin = kmin;
    uint32_t* prow = (uint32_t*)sc.take((size_t)np * 4);
    pa.prow = prow;
    if (keyed) {
      const size_t kb = wide ? 8 : 4;
      void* pkey = sc.take((size_t)np * kb);
      void* pkey2 = sc.take((size_t)np * kb);
      uint32_t* prow2 = (uint32_t*)sc.take((size_t)np * 4);
      uint8_t* ss = (uint8_t*)sc.take((size_t)np);
      pa.pkey = pkey;
      bool alt;
      if (wide) {
        hipLaunchKernelGGL(mseq_pack_kernel<uint64_t>, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, pa);
        tmark("mseq_pack");
        alt = radix_sort_pairs<uint64_t>((uint64_t*)pkey, (uint64_t*)pkey2, prow, prow2, (size_t)np, 0, kbits, sc, s);
      } else {
        hipLaunchKernelGGL(mseq_pack_kernel<uint32_t>, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, pa);
        tmark("mseq_pack");
        alt = radix_sort_pairs<uint32_t>((uint32_t*)pkey, (uint32_t*)pkey2, prow, prow2, (size_t)np, 0, kbits, sc, s);
      }
      skey = alt ? pkey2 : pkey;
      perm = alt ? prow2 : prow;
      hipLaunchKernelGGL(mseq_streams_kernel, seq_grid(np, kSeqBlock), dim3(kSeqBlock), 0, s, perm, sid, np, ss);
      sstr = ss;
      tmark("mseq_sort");
    } else {
      uint8_t* ss = (uint8_t*)sc.take((size_t)np);
      pa.pstr = ss;
      hipLaunchKernelGGL(mseq_pack_kernel<uint32_t>, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, pa);
      tmark("mseq_pack");
      perm = prow;
      sstr = ss;
    }
  }
  if (tm) SM_HIP(hipEventRecord(tm->ev[1], s));

  // ---- link
  SM_HIP(hipMemsetAsync(ctl, 0, 8, s));
  MSeqArgs ma{};
  SeqKArgs& sa = ma.q;
  sa.n = np;
  sa.ts = a.ts;
  sa.st = a.st;
  sa.code = a.code;
  sa.consts = a.consts;
  sa.k = k;
  for (int m = 0; m < kSeqKMax; ++m) {
    sa.off[m] = m < k ? p.off[m] : 0;
    sa.len[m] = m < k ? p.len[m] : 0;
    sa.within[m] = m > 0 && m < k ? p.within[m] : -1;
    ma.want[m] = m < k ? (uint8_t)p.stream[m] : 0;
  }
  sa.ordinals = a.ordinals;
  sa.obase = a.ordinal_base;
  sa.perm = perm;
  sa.skey = skey;
  sa.kmin = kmin;
  sa.kmax = kmax;
  sa.carry = (const int64_t*)carry.rows;
  sa.nc = nc;
  sa.cw = cw;
  sa.prev = (int32_t*)sc.take((size_t)n * 4);
  const size_t hit_bytes = ((size_t)n + 3) & ~(size_t)3;
  sa.hit = (uint8_t*)sc.take(hit_bytes);
  sa.cand = cand;
  sa.cand_n = ctl;
  ma.sstr = sstr;
  ma.sid = sid;
  uint32_t* counts = (uint32_t*)sc.take((size_t)(ntiles + 1) * 4);
  if (packed) SM_HIP(hipMemsetAsync(sa.hit, 0, hit_bytes, s));  // rows that are not read have no lane
  if (wide) hipLaunchKernelGGL(mseq_link_kernel<uint64_t>, dim3((unsigned)ptiles), dim3(kSeqBlock), 0, s, ma);
  else hipLaunchKernelGGL(mseq_link_kernel<uint32_t>, dim3((unsigned)ptiles), dim3(kSeqBlock), 0, s, ma);
  tmark("mseq_link");
  if (nc > 0) {
    if (wide) hipLaunchKernelGGL(seqk_keep_kernel<uint64_t>, seq_grid(nc, kSeqBlock), dim3(kSeqBlock), 0, s, sa);
    else hipLaunchKernelGGL(seqk_keep_kernel<uint32_t>, seq_grid(nc, kSeqBlock), dim3(kSeqBlock), 0, s, sa);
    tmark("mseq_keep");
  }
  if (tm) SM_HIP(hipEventRecord(tm->ev[2], s));

  // ---- tuples in row order
  hipLaunchKernelGGL(seqk_count_kernel, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, (const uint8_t*)sa.hit, n, counts);
  tmark("mseq_count");
  exclusive_scan_u32(counts, (size_t)ntiles, sc, s, ctl + 1);
  tmark("mseq_scan");
  hipLaunchKernelGGL(seqk_emit_kernel, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, (const uint8_t*)sa.hit,
                     (const int32_t*)sa.prev, n, k, (const uint32_t*)counts, a.ordinals, a.ordinal_base,
                     (const int64_t*)carry.rows, cw, tuples_out);
  tmark("mseq_emit");
  uint32_t hc[2] = {0, 0};
  SM_HIP(hipMemcpyAsync(hc, ctl, 8, hipMemcpyDeviceToHost, s));
  SM_HIP(hipStreamSynchronize(s));
  const int64_t m = hc[1];
  if (m > tuples_cap || (int64_t)hc[0] > cand_cap) {  // cannot happen (m <= np <= tuples_cap): checked, not assumed
    sc.used = mark;
    throw std::runtime_error("adjacent-run closed form over several streams: output larger than its buffer");
  }

  // ---- carry out (build_carry reads the old rows before it replaces them)
  sc.used = keep;
  build_carry(sa.cand, (int64_t)hc[0], a.st, nattr, carry, sc, s, 64, 0, false, sid);
  tmark("mseq_carry");
  carry.ts_last = carry.active ? std::max<int64_t>(carry.ts_last, ts_last) : ts_last;
  carry.active = true;
  fs.last_path = 8;
  if (tm) SM_HIP(hipEventRecord(tm->ev[3], s));
  sc.used = mark;
  return m;
}

// The pattern `every e1=A[c1] -> e2=B[c2] within T` over two streams of one schema on an interleaved batch
// (mpat_dev.h). Per batch:
//   mpat_facts / mpat_pack / mpat_sort   as fast_seq_ms with R = {A, B}: the read rows in (key, arrival) order with a
//                stream byte per sorted position (unkeyed: row order)
//   mpat_link    every partial (carried rows, then A rows passing c1) scans forward in its key run for its e2; the result
//                is written at the e1's own place; carry-out candidates
//   mpat_count / mpat_scan / mpat_emit   (e2, e1) compacted in order of e1: carried rows in carry order, then row order
//   mpat_order   a stable sort by e2 alone over the bits of the largest relative ordinal, then the (e1, e2) pairs: the
//                reference's (e2, e1) order
//   mpat_carry   build_carry in its general form (several rows per key, sorted by (key, ordinal))
// One host round trip for the facts and one for the two counts; nothing is changed before the second.
int64_t fast_pat_ms(const FastArgs& a, const int32_t* sid, const MPatPlan& p, int nattr, FastState& fs, FastCarry& carry,
                    uint32_t* pairs_out, int64_t pairs_cap, Scratch& sc, hipStream_t s, FastTimings* tm) {
  const int64_t n = a.n;
  if (n == 0) return 0;
  const int64_t nc = carry.n;
  if (n >= 0x7fffffffll || n + nc >= 0x7fffffffll) return FAST_OUTSIDE;
  if (p.stream[0] < 0 || p.stream[0] >= kMSeqStreams || p.stream[1] < 0 || p.stream[1] >= kMSeqStreams)
    return FAST_OUTSIDE;
  const bool keyed = p.keyed;
  const size_t mark = sc.used;
  if (tm) {  // (the entry point's own marks come first: the first label here times from the last of them)
    SM_HIP(hipEventRecord(tm->ev[0], s));
    if (tm->nmk == 0) tm->mark("start", s);
  }
  auto tmark = [&](const char* l) {
    if (tm) tm->mark(l, s);
  };
  const int cw = 3 + nattr;
  const int64_t ntiles = (n + kSeqTile - 1) / kSeqTile;

  MSeqSrc src{};
  src.n = n;
  src.sid = sid;
  src.read = p.read;
  for (int q = 0; q < kMSeqStreams; ++q) src.kcol[q] = keyed ? p.kcol[q] : nullptr;
  src.wide = p.wide;
  src.ts = a.ts;
  src.ordinals = a.ordinals;
  src.obase = a.ordinal_base;

  // ---- facts: nothing is changed before they are read
  MSeqFacts* f = (MSeqFacts*)sc.take(sizeof(MSeqFacts));
  uint32_t* tile_n = (uint32_t*)sc.take((size_t)(ntiles + 1) * 4);
  SM_HIP(hipMemsetAsync(f, 0, sizeof(MSeqFacts), s));
  hipLaunchKernelGGL(mseq_facts_kernel, dim3((unsigned)std::min<int64_t>(ntiles, 2048)), dim3(kSeqBlock), 0, s, src,
                     ntiles, tile_n, f);
  if (nc > 0)
    hipLaunchKernelGGL(mseq_carry_check_kernel, seq_grid(nc, 256), dim3(256), 0, s, (const int64_t*)carry.rows, nc,
                       carry.width, a.ordinal_base, f);
  tmark("mpat_facts");
  MSeqFacts h;
  SM_HIP(hipMemcpyAsync(&h, f, sizeof(MSeqFacts), hipMemcpyDeviceToHost, s));
  SM_HIP(hipStreamSynchronize(s));
  auto leave = [&](int64_t r) {
    sc.used = mark;
    return r;
  };
  constexpr uint64_t kBias = 0x8000000000000000ull;
  const int64_t np = (int64_t)h.nread;
  const int64_t ts0 = (int64_t)(~h.tmin_c ^ kBias), ts_last = (int64_t)(h.tmax ^ kBias);
  const int64_t o0 = (int64_t)(~h.omin_c ^ kBias), omax = (int64_t)(h.omax ^ kBias);
  // a partial older than T is dropped, and a scan ends at the window, only because event time never goes back
  if (p.within >= 0 && np > 0 && (h.bad_ts || (carry.active && ts0 < carry.ts_last))) return leave(FAST_NON_MONOTONE);
  if (h.bad_ord || h.bad_carry || (np > 0 && (o0 < 0 || omax >= 0x7fffffffll))) return leave(FAST_OUTSIDE);
  if (nc > 0 && carry.width != cw) return leave(FAST_OUTSIDE);
  if (np + nc > pairs_cap) return leave(FAST_OUTSIDE);
  if (np == 0) {  // no row of a stream the query reads: its carried rows wait
    fs.last_path = 9;
    return leave(0);
  }
  int64_t kmin = 0, kmax = 0;
  int kbits = 0;
  if (keyed) {
    kmin = (int64_t)(~h.kmin_c ^ kBias);
    kmax = (int64_t)(h.kmax ^ kBias);
    const uint64_t kspan = (uint64_t)(kmax - kmin);
    kbits = std::max(1, bits_of(kspan));
    if (!carry.active && p.remap_span > 0 && (kbits > 30 || kspan > (uint64_t)p.remap_span)) return leave(FAST_KEY_SPAN);
  }
  const bool wide = kbits > 32;
  const bool packed = keyed || np < n;

  // what the carry-out reads lies first, so that the rest is free again when build_carry runs
  const int64_t cand_cap = np + nc;
  const int64_t total = nc + n;  // entries of `res`
  const int64_t rtiles = (total + kSeqTile - 1) / kSeqTile;
  const size_t hist = (size_t)8 << 20;
  {  // scratch up to the counts, for the worst case, before anything changes. Per read row: sort pairs twice over (+ a
     // histogram word per 4 rows) and a stream byte, then the (e2, e1) sort pairs twice over; per entry of res: 4 bytes
    const size_t link = (size_t)np * (keyed ? (wide ? 43 : 35) : 22) + (size_t)nc * 17 + (size_t)total * 4 +
                        (size_t)(ntiles + rtiles + 4) * 8 + hist;
    if (sc.used + (size_t)cand_cap * 32 + link + 4096 > sc.cap) return leave(FAST_OUTSIDE);
  }
  uint32_t* ctl = (uint32_t*)sc.take(8);  // [0] candidates, [1] pairs
  int64_t* cand = (int64_t*)sc.take((size_t)cand_cap * 32);
  const size_t keep = sc.used;

  // ---- the read rows, then (keyed) in (key, arrival) order
  const uint32_t* perm = nullptr;
  const void* skey = nullptr;
  const uint8_t* sstr = nullptr;
  if (packed) {
    exclusive_scan_u32(tile_n, (size_t)ntiles, sc, s);
    MSeqPack pa{};
    pa.s = src;
    pa.tile_off = tile_n;
    pa.kmin = kmin;
    uint32_t* prow = (uint32_t*)sc.take((size_t)np * 4);
    pa.prow = prow;
    if (keyed) {
      const size_t kb = wide ? 8 : 4;
      void* pkey = sc.take((size_t)np * kb);
      void* pkey2 = sc.take((size_t)np * kb);
      uint32_t* prow2 = (uint32_t*)sc.take((size_t)np * 4);
      uint8_t* ss = (uint8_t*)sc.take((size_t)np);
      pa.pkey = pkey;
      bool alt;
      if (wide) {
        hipLaunchKernelGGL(mseq_pack_kernel<uint64_t>, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, pa);
        tmark("mpat_pack");
        alt = radix_sort_pairs<uint64_t>((uint64_t*)pkey, (uint64_t*)pkey2, prow, prow2, (size_t)np, 0, kbits, sc, s);
      } else {
        hipLaunchKernelGGL(mseq_pack_kernel<uint32_t>, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, pa);
        tmark("mpat_pack");
        alt = radix_sort_pairs<uint32_t>((uint32_t*)pkey, (uint32_t*)pkey2, prow, prow2, (size_t)np, 0, kbits, sc, s);
      }
      skey = alt ? pkey2 : pkey;
      perm = alt ? prow2 : prow;
      hipLaunchKernelGGL(mseq_streams_kernel, seq_grid(np, kSeqBlock), dim3(kSeqBlock), 0, s, perm, sid, np, ss);
      sstr = ss;
      tmark("mpat_sort");
    } else {
      uint8_t* ss = (uint8_t*)sc.take((size_t)np);
      pa.pstr = ss;
      hipLaunchKernelGGL(mseq_pack_kernel<uint32_t>, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, pa);
      tmark("mpat_pack");
      perm = prow;
      sstr = ss;
    }
  }
  if (tm) SM_HIP(hipEventRecord(tm->ev[1], s));

  // ---- link
  SM_HIP(hipMemsetAsync(ctl, 0, 8, s));
  MPatArgs ma{};
  ma.np = np;
  ma.n = n;
  ma.ts = a.ts;
  ma.st = a.st;
  ma.code = a.code;
  ma.consts = a.consts;
  ma.c1_off = p.off[0];
  ma.c1_len = p.len[0];
  ma.c2_off = p.off[1];
  ma.c2_len = p.len[1];
  ma.within = p.within;
  ma.ts_last = ts_last;
  ma.ordinals = a.ordinals;
  ma.obase = a.ordinal_base;
  ma.perm = perm;
  ma.skey = skey;
  ma.kmin = kmin;
  ma.kmax = kmax;
  ma.sstr = sstr;
  ma.sid = sid;
  ma.sa = p.stream[0];
  ma.sb = p.stream[1];
  ma.carry = (const int64_t*)carry.rows;
  ma.nc = nc;
  ma.cw = cw;
  ma.res = (int32_t*)sc.take((size_t)total * 4);
  ma.cand = cand;
  ma.cand_n = ctl;
  uint32_t* counts = (uint32_t*)sc.take((size_t)(rtiles + 1) * 4);
  // rows that are not read have no lane: their entries are "none"
  if (np < n) SM_HIP(hipMemsetD32Async((hipDeviceptr_t)(ma.res + nc), (int)kSeqNone, (size_t)n, s));
  const dim3 lgrid((unsigned)((nc + np + kSeqTile - 1) / kSeqTile));
  if (wide) hipLaunchKernelGGL(mpat_link_kernel<uint64_t>, lgrid, dim3(kSeqBlock), 0, s, ma);
  else hipLaunchKernelGGL(mpat_link_kernel<uint32_t>, lgrid, dim3(kSeqBlock), 0, s, ma);
  tmark("mpat_link");
  if (tm) SM_HIP(hipEventRecord(tm->ev[2], s));

  // ---- the two counts: pairs and carry-out candidates
  hipLaunchKernelGGL(seq_count_kernel, dim3((unsigned)rtiles), dim3(kSeqBlock), 0, s, (const int32_t*)ma.res, total, counts);
  tmark("mpat_count");
  exclusive_scan_u32(counts, (size_t)rtiles, sc, s, ctl + 1);
  tmark("mpat_scan");
  uint32_t hc[2] = {0, 0};
  SM_HIP(hipMemcpyAsync(hc, ctl, 8, hipMemcpyDeviceToHost, s));
  SM_HIP(hipStreamSynchronize(s));
  const int64_t m = hc[1], ncand = hc[0];
  if (m > pairs_cap || ncand > cand_cap) {  // cannot happen (one of each per partial at most): checked, not assumed
    sc.used = mark;
    throw std::runtime_error("pattern closed form over two streams: output larger than its buffer");
  }
  // room for the carry build, now that the number of candidates is known: still nothing is changed
  if (keep + (size_t)ncand * (size_t)(8 * cw + 44) + hist + 4096 > sc.cap) return leave(FAST_OUTSIDE);

  // ---- pairs in order of e1, then the stable sort by e2
  if (m > 0) {
    uint32_t* jk = (uint32_t*)sc.take((size_t)m * 4);
    uint32_t* jk2 = (uint32_t*)sc.take((size_t)m * 4);
    uint32_t* iv = (uint32_t*)sc.take((size_t)m * 4);
    uint32_t* iv2 = (uint32_t*)sc.take((size_t)m * 4);
    hipLaunchKernelGGL(mpat_emit_kernel, dim3((unsigned)rtiles), dim3(kSeqBlock), 0, s, (const int32_t*)ma.res, total, nc,
                       (const uint32_t*)counts, a.ordinals, a.ordinal_base, (const int64_t*)carry.rows, cw, jk, iv);
    tmark("mpat_emit");
    const bool alt = radix_sort_pairs<uint32_t>(jk, jk2, iv, iv2, (size_t)m, 0, std::max(1, bits_of((uint64_t)omax)), sc, s);
    hipLaunchKernelGGL(mpat_pairs_kernel, seq_grid(m, kSeqBlock), dim3(kSeqBlock), 0, s,
                       (const uint32_t*)(alt ? jk2 : jk), (const uint32_t*)(alt ? iv2 : iv), m, pairs_out);
    tmark("mpat_order");
  }

  // ---- carry out (build_carry reads the old rows before it replaces them)
  sc.used = keep;
  build_carry(cand, ncand, a.st, nattr, carry, sc, s);
  tmark("mpat_carry");
  carry.ts_last = carry.active ? std::max<int64_t>(carry.ts_last, ts_last) : ts_last;
  carry.active = true;
  fs.last_path = 9;
  if (tm) SM_HIP(hipEventRecord(tm->ev[3], s));
  sc.used = mark;
  return m;
}

}  // namespace sm
