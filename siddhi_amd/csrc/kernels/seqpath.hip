// Host entries of the nine sequence closed forms (fastpath.h has their contracts, seq_dev.h / mseq_dev.h / mpat_dev.h /
// mpatk_dev.h / absent_dev.h / mpat_nand_dev.h / mpat_logic_dev.h / mpat_count_dev.h the rules and the kernels). Every driver runs one batch through the same stages, each written once below:
//   begin      Batch: the timing start, the scratch mark, and leave(), which every return goes through
//   facts      one streaming pass over the keys, event times and ordinals, plus the carried ordinals; its read-back is
//              the only host round trip before anything is changed (Facts: the same fields for SeqFacts and MSeqFacts)
//   envelope   decreasing event time under a within, ordinals and carried ordinals that do not fit, carry width,
//              capacity, key span: 0 or the FAST_* result the batch leaves with, and the key's significant bits
//   budget     the scratch of the worst case (each driver's own formula), still before anything changes; then ctl
//              (candidates, outputs) and the carry-out candidates, which lie first so that the rest is free again when
//              build_carry runs (take_out)
//   sort       rows in (key, arrival) order: a stable LSD sort of (key - kmin, row) over the key's significant bits
//              (seq_sort_rows: every row of one stream; mseq_pack_sort: the read rows of an interleaved batch, with a
//              stream byte per position)
//   link       the driver's own kernel: what each row completes, and the carry-out candidates
//   out        tile counts, their scan, the outputs in row order, then the second and last round trip for the two
//              counts (read_counts); seqk_tuples_out is all of it for the adjacent-run forms
//   carry      carry_out: build_carry over the candidates (it reads the old rows before it replaces them), ts_last,
//              last_path
// The drivers:
//   fast_seq_adjacent  path 6: seq_link_kernel marks the carried rows an event saw (seq_keep keeps the others); unkeyed,
//                      the link pass counts as well; each e2 has at most one pair, so row order is the reference's order;
//                      one carried row per key, in key order already (build_carry's key_runs_ordered)
//   fast_seq_k         path 7: seqk_link_kernel, candidates = the last k - 1 rows of every run, several rows per key
//   fast_seq_ms        path 8: the read rows of an interleaved batch packed first (skipped when every row is read and the
//                      query is unkeyed); mseq_link_kernel; a carried row is one word wider, its stream
//   fast_pat_ms        path 9: packed as path 8; mpat_link_kernel writes each partial's e2 at the e1's own place; the pairs
//                      are compacted in order of e1 after the counts are known, then sorted by e2 alone (the reference's
//                      (e2, e1) order); the carry build's room is checked again once the candidates are counted
//   fast_pat_k         path 10: packed as path 8; mpatk_link_kernel walks each partial through its states and writes ek at
//                      the e1's own place; the k-tuples are compacted in order of e1, then sorted by e2, ..., ek in turn;
//                      the carry is two tables, the open partials and (path 8's rows, through build_carry) the events
//                      they hold, each once: the link pass flags them, mpatk_cand_kernel makes the candidates
//   fast_absent        path 11: packed as path 8 (no read row: nothing is packed, the carried partials may still fall due);
//                      no partial scans: the first cancelling row after every sorted position comes from one count scan
//                      over chunks (absent_next), then one lane per partial decides cancelled / due at p / open
//                      (absent_state_kernel); outputs compacted in arrival order, keyed sorted by (p, creation ordinal of
//                      the instance) and projected here, since their timestamp and trigger are no event's
//   fast_pat_nand      path 12: path 9 with path 11's count scan in front of the link pass: pnand_link_kernel ends a
//                      partial's scan at its next cancelling row as well; everything after the link pass is path 9's
//   fast_pat_logic     path 13: path 10 with plog_link_kernel in place of its link pass: two members found independently,
//                      both (and) or the earlier (or); three words per tuple and one stable sort by the completing member;
//                      the carry is path 10's two tables
//   fast_pat_count     path 14: path 13 with pcnt_link_kernel in place of its link pass: up to n hits, then the first C
//                      row in e3 that dies or passes; n + 2 words per tuple and one stable sort by (e3, p); the carry
//                      is path 10's two tables with rows of n + 5 words, bounded by the scratch and not by a window
#include <string>

#include "absent_dev.h"
#include "fastpath.h"
#include "mpat_count_dev.h"
#include "mpat_dev.h"
#include "mpat_logic_dev.h"
#include "mpat_nand_dev.h"
#include "mpatk_dev.h"
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
                                       unsigned int* __restrict__ bad_carry) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int64_t o = rows[c * cw + 1] - obase;
  if (o >= 0 || o <= (int64_t)INT32_MIN) atomicOr(bad_carry, 1u);
}

template <typename KT, typename K>
__global__ void seq_sort_keys_kernel(const KT* __restrict__ kcol, int64_t n, int64_t kmin, K* __restrict__ sk,
                                     uint32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  sk[i] = (K)((uint64_t)(int64_t)kcol[i] - (uint64_t)kmin);
  idx[i] = (uint32_t)i;
}

__global__ void mseq_keys_kernel(MSeqSrc s, int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= s.n) return;
  const int32_t sd = s.sid[i];
  keys[i] = mseq_read(s, sd) ? mseq_key(s, sd, i) : 0;
}

inline dim3 seq_grid(int64_t n, int t) { return dim3((unsigned)std::max<int64_t>(1, (n + t - 1) / t)); }

int bits_of(uint64_t x) {
  int b = 0;
  while (b < 64 && (x >> b) != 0) ++b;
  return b;
}

constexpr uint64_t kBias = 0x8000000000000000ull;

// FastTimings keeps labels by pointer: the marks of the shared stages, one table of literals per path
struct Labels {
  const char *facts, *pack, *sort, *keep, *count, *scan, *emit, *carry;
  const char* what;  // the form's name in the "output larger than its buffer" error
};
constexpr Labels kSeqLabels = {"seq_facts", nullptr,     "seq_sort", "seq_keep", "seq_count",
                               "seq_scan",  "seq_emit",  "seq_carry", "adjacent-pair closed form"};
constexpr Labels kSeqKLabels = {"seqk_facts", nullptr,     "seqk_sort", "seqk_keep", "seqk_count",
                                "seqk_scan",  "seqk_emit", "seqk_carry", "adjacent-run closed form"};
constexpr Labels kMSeqLabels = {"mseq_facts", "mseq_pack", "mseq_sort",  "mseq_keep",
                                "mseq_count", "mseq_scan", "mseq_emit",  "mseq_carry",
                                "adjacent-run closed form over several streams"};
constexpr Labels kMPatLabels = {"mpat_facts", "mpat_pack", "mpat_sort",  nullptr,
                                "mpat_count", "mpat_scan", "mpat_emit",  "mpat_carry",
                                "pattern closed form over two streams"};
constexpr Labels kMPatKLabels = {"mpatk_facts", "mpatk_pack", "mpatk_sort",  "mpatk_cand",
                                 "mpatk_count", "mpatk_scan", "mpatk_emit",  "mpatk_carry",
                                 "k-state pattern closed form over several streams"};

constexpr Labels kAbsLabels = {"absent_facts", "absent_pack", "absent_sort",  nullptr,
                               "absent_count", "absent_scan", "absent_emit",  "absent_carry",
                               "timeout closed form"};

constexpr Labels kPNandLabels = {"pnand_facts", "pnand_pack", "pnand_sort",  nullptr,
                                 "pnand_count", "pnand_scan", "pnand_emit",  "pnand_carry",
                                 "logical-absent pattern closed form"};

constexpr Labels kPCntLabels = {"pcnt_facts", "pcnt_pack", "pcnt_sort",  "pcnt_cand",
                                "pcnt_count", "pcnt_scan", "pcnt_emit",  "pcnt_carry",
                                "count pattern closed form"};

constexpr Labels kPLogLabels = {"plog_facts", "plog_pack", "plog_sort",  "plog_cand",
                                "plog_count", "plog_scan", "plog_emit",  "plog_carry",
                                "logical pattern closed form"};

// ---- begin / leave. own_marks: the driver's marks are the batch's only ones (same-stream); otherwise the entry
// point's own marks come first, and the first label here times from the last of them
struct Batch {
  Scratch& sc;
  hipStream_t s;
  FastTimings* tm;
  const size_t mark0;  // the scratch as the driver found it
  Batch(Scratch& sc_, hipStream_t s_, FastTimings* tm_, bool own_marks) : sc(sc_), s(s_), tm(tm_), mark0(sc_.used) {
    if (!tm) return;
    SM_HIP(hipEventRecord(tm->ev[0], s));
    if (own_marks) tm->nmk = 0;
    if (tm->nmk == 0) tm->mark("start", s);
  }
  void mark(const char* l) {
    if (tm) tm->mark(l, s);
  }
  void event(int i) {
    if (tm) SM_HIP(hipEventRecord(tm->ev[i], s));
  }
  int64_t leave(int64_t r) {
    sc.used = mark0;
    return r;
  }
};

// ---- facts: nothing is changed before they are read
struct Facts {
  int64_t np;          // rows the query reads (same-stream: all of them)
  int64_t kmin, kmax;  // their key range (0 when unkeyed); the rest is valid when np > 0
  int64_t ts0, ts_last;
  int64_t o0, omax;    // relative ordinals of the first and the last read row
  bool bad_ts, bad_ord, bad_carry;
};

// after the driver's facts kernel: the carried ordinals, the mark and the read-back
void read_facts(Batch& b, const FastArgs& a, const FastCarry& carry, unsigned int* bad_carry, const char* label,
                void* host, const void* dev, size_t bytes) {
  if (carry.n > 0)
    hipLaunchKernelGGL(seq_carry_check_kernel, seq_grid(carry.n, 256), dim3(256), 0, b.s, (const int64_t*)carry.rows,
                       carry.n, carry.width, a.ordinal_base, bad_carry);
  b.mark(label);
  SM_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, b.s));
  SM_HIP(hipStreamSynchronize(b.s));
}

Facts seq_facts(Batch& b, const FastArgs& a, const void* kcol, bool key64, const FastCarry& carry, const char* label) {
  const int64_t n = a.n;
  SeqFacts* f = (SeqFacts*)b.sc.take(sizeof(SeqFacts));
  {
    SeqFacts init{};
    init.kmin = ~0ull;
    SM_HIP(hipMemcpyAsync(f, &init, sizeof(SeqFacts), hipMemcpyHostToDevice, b.s));
  }
  const dim3 fgrid((unsigned)std::min<int64_t>(2048, (n + kFactsBlock - 1) / kFactsBlock));
  if (key64)
    hipLaunchKernelGGL(seq_facts_kernel<int64_t>, fgrid, dim3(kFactsBlock), 0, b.s, (const int64_t*)kcol, a.ts,
                       a.ordinals, a.ordinal_base, n, f);
  else
    hipLaunchKernelGGL(seq_facts_kernel<int32_t>, fgrid, dim3(kFactsBlock), 0, b.s, (const int32_t*)kcol, a.ts,
                       a.ordinals, a.ordinal_base, n, f);
  SeqFacts h;
  read_facts(b, a, carry, &f->bad_carry, label, &h, f, sizeof(SeqFacts));
  Facts r{};
  r.np = n;
  if (kcol) {
    r.kmin = (int64_t)(h.kmin ^ kBias);
    r.kmax = (int64_t)(h.kmax ^ kBias);
  }
  r.ts0 = h.ts0;
  r.ts_last = h.ts_last;
  r.o0 = h.o0;
  r.omax = h.omax;
  r.bad_ts = h.bad_ts != 0;
  r.bad_ord = h.bad_ord != 0;
  r.bad_carry = h.bad_carry != 0;
  return r;
}

MSeqSrc mseq_src(int64_t n, const int32_t* sid, const MSeqKeys& p) {
  MSeqSrc src{};
  src.n = n;
  src.sid = sid;
  src.read = p.read;
  for (int q = 0; q < kMSeqStreams; ++q) src.kcol[q] = p.keyed ? p.kcol[q] : nullptr;
  src.wide = p.wide;
  return src;
}

// over the read rows of an interleaved batch; *tile_n: the read rows of every tile (mseq_pack_sort scans them)
Facts mseq_facts(Batch& b, const FastArgs& a, const MSeqSrc& src, bool keyed, int64_t ntiles, const FastCarry& carry,
                 const char* label, uint32_t** tile_n) {
  MSeqFacts* f = (MSeqFacts*)b.sc.take(sizeof(MSeqFacts));
  *tile_n = (uint32_t*)b.sc.take((size_t)(ntiles + 1) * 4);
  SM_HIP(hipMemsetAsync(f, 0, sizeof(MSeqFacts), b.s));
  hipLaunchKernelGGL(mseq_facts_kernel, dim3((unsigned)std::min<int64_t>(ntiles, 2048)), dim3(kSeqBlock), 0, b.s, src,
                     ntiles, *tile_n, f);
  MSeqFacts h;
  read_facts(b, a, carry, &f->bad_carry, label, &h, f, sizeof(MSeqFacts));
  Facts r{};
  r.np = (int64_t)h.nread;
  if (keyed) {
    r.kmin = (int64_t)(~h.kmin_c ^ kBias);
    r.kmax = (int64_t)(h.kmax ^ kBias);
  }
  r.ts0 = (int64_t)(~h.tmin_c ^ kBias);
  r.ts_last = (int64_t)(h.tmax ^ kBias);
  r.o0 = (int64_t)(~h.omin_c ^ kBias);
  r.omax = (int64_t)(h.omax ^ kBias);
  r.bad_ts = h.bad_ts != 0;
  r.bad_ord = h.bad_ord != 0;
  r.bad_carry = h.bad_carry != 0;
  return r;
}

// ---- envelope: 0, or the result the batch leaves with before anything is changed; *kbits: the significant bits of
// key - kmin (0 when unkeyed). A batch without read rows (interleaved only: np = n > 0 on one stream) passes no time,
// ordinal or key check, since none of those facts exists: its driver returns 0 and leaves the carry as it is.
// fits: the driver's own capacity check.
int64_t envelope(const Facts& h, bool any_within, bool keyed, bool fits, const FastCarry& carry, int cw,
                 int64_t remap_span, int* kbits) {
  *kbits = 0;
  const bool rows = h.np > 0;
  // with a within, a partial older than T is dropped (and a scan ends at the window) only because event time never
  // goes back
  if (any_within && rows && (h.bad_ts || (carry.active && h.ts0 < carry.ts_last))) return FAST_NON_MONOTONE;
  if (h.bad_ord || h.bad_carry || (rows && (h.o0 < 0 || h.omax >= 0x7fffffffll))) return FAST_OUTSIDE;
  if (carry.n > 0 && carry.width != cw) return FAST_OUTSIDE;
  if (!fits) return FAST_OUTSIDE;
  if (keyed && rows) {
    const uint64_t kspan = (uint64_t)(h.kmax - h.kmin);
    *kbits = std::max(1, bits_of(kspan));
    // a query's first batch decides between key values and dense ids when the caller offers them (remap_span: it
    // gives the ids and runs the batch again); once rows are carried their keys stay what they are: any span is sorted
    if (!carry.active && remap_span > 0 && (*kbits > 30 || kspan > (uint64_t)remap_span)) return FAST_KEY_SPAN;
  }
  return 0;
}

// ---- what the carry-out reads lies first, so that the rest is free again when build_carry runs
struct Out {
  uint32_t* ctl;  // [0] candidates, [1] outputs
  uint8_t* used;  // adjacent pairs only: carried rows that saw an event
  int64_t* cand;
  int64_t cand_cap;
  size_t keep;
};

Out take_out(Scratch& sc, int64_t cand_cap, size_t used_bytes = 0) {
  Out o{};
  o.ctl = (uint32_t*)sc.take(8);
  if (used_bytes) o.used = (uint8_t*)sc.take(used_bytes);
  o.cand = (int64_t*)sc.take((size_t)cand_cap * 32);
  o.cand_cap = cand_cap;
  o.keep = sc.used;
  return o;
}

// ---- sort. true: the result lies in the second buffers
bool sort_pairs(bool wide, void* k, void* k2, uint32_t* v, uint32_t* v2, int64_t n, int bits, Batch& b) {
  return wide ? radix_sort_pairs<uint64_t>((uint64_t*)k, (uint64_t*)k2, v, v2, (size_t)n, 0, bits, b.sc, b.s)
              : radix_sort_pairs<uint32_t>((uint32_t*)k, (uint32_t*)k2, v, v2, (size_t)n, 0, bits, b.sc, b.s);
}

struct Rows {  // rows in (key, arrival) order; all null: row order
  const uint32_t* perm = nullptr;
  const void* skey = nullptr;    // key - kmin of each position (uint64_t when kbits > 32)
  const uint8_t* sstr = nullptr;  // interleaved: the stream of each position
};

// every row of one stream
Rows seq_sort_rows(Batch& b, const void* kcol, bool key64, int64_t n, int64_t kmin, int kbits) {
  const bool wide = kbits > 32;
  Scratch& sc = b.sc;
  uint32_t* si = (uint32_t*)sc.take((size_t)n * 4);
  uint32_t* si2 = (uint32_t*)sc.take((size_t)n * 4);
  void* sk = sc.take((size_t)n * (wide ? 8 : 4));
  void* sk2 = sc.take((size_t)n * (wide ? 8 : 4));
  const dim3 g = seq_grid(n, 256);
  if (wide)
    hipLaunchKernelGGL((seq_sort_keys_kernel<int64_t, uint64_t>), g, dim3(256), 0, b.s, (const int64_t*)kcol, n, kmin,
                       (uint64_t*)sk, si);
  else if (key64)
    hipLaunchKernelGGL((seq_sort_keys_kernel<int64_t, uint32_t>), g, dim3(256), 0, b.s, (const int64_t*)kcol, n, kmin,
                       (uint32_t*)sk, si);
  else
    hipLaunchKernelGGL((seq_sort_keys_kernel<int32_t, uint32_t>), g, dim3(256), 0, b.s, (const int32_t*)kcol, n, kmin,
                       (uint32_t*)sk, si);
  const bool alt = sort_pairs(wide, sk, sk2, si, si2, n, kbits, b);
  Rows r;
  r.skey = alt ? sk2 : sk;
  r.perm = alt ? si2 : si;
  return r;
}

// the np read rows of an interleaved batch: packed in row order as (key - kmin, row) + a stream byte per position
// (skipped when every row is read and the query is unkeyed), then, keyed, sorted, the stream bytes gathered after
Rows mseq_pack_sort(Batch& b, const MSeqSrc& src, uint32_t* tile_n, int64_t ntiles, int64_t np, bool keyed,
                    int64_t kmin, int kbits, const Labels& L) {
  Rows r;
  if (!keyed && np == src.n) return r;
  Scratch& sc = b.sc;
  exclusive_scan_u32(tile_n, (size_t)ntiles, sc, b.s);
  MSeqPack pa{};
  pa.s = src;
  pa.tile_off = tile_n;
  pa.kmin = kmin;
  uint32_t* prow = (uint32_t*)sc.take((size_t)np * 4);
  pa.prow = prow;
  const dim3 grid((unsigned)ntiles), block(kSeqBlock);
  if (!keyed) {
    uint8_t* ss = (uint8_t*)sc.take((size_t)np);
    pa.pstr = ss;
    hipLaunchKernelGGL(mseq_pack_kernel<uint32_t>, grid, block, 0, b.s, pa);
    b.mark(L.pack);
    r.perm = prow;
    r.sstr = ss;
    return r;
  }
  const bool wide = kbits > 32;
  const size_t kb = wide ? 8 : 4;
  void* pkey = sc.take((size_t)np * kb);
  void* pkey2 = sc.take((size_t)np * kb);
  uint32_t* prow2 = (uint32_t*)sc.take((size_t)np * 4);
  uint8_t* ss = (uint8_t*)sc.take((size_t)np);
  pa.pkey = pkey;
  if (wide) hipLaunchKernelGGL(mseq_pack_kernel<uint64_t>, grid, block, 0, b.s, pa);
  else hipLaunchKernelGGL(mseq_pack_kernel<uint32_t>, grid, block, 0, b.s, pa);
  b.mark(L.pack);
  const bool alt = sort_pairs(wide, pkey, pkey2, prow, prow2, np, kbits, b);
  r.skey = alt ? pkey2 : pkey;
  r.perm = alt ? prow2 : prow;
  hipLaunchKernelGGL(mseq_streams_kernel, seq_grid(np, kSeqBlock), block, 0, b.s, r.perm, src.sid, np, ss);
  r.sstr = ss;
  b.mark(L.sort);
  return r;
}

// ---- the adjacent-run kernels' arguments (paths 7 and 8): `rows` positions in `r` order; prev / hit by batch row
SeqKArgs seqk_args(const FastArgs& a, int k, const int* off, const int* len, const int64_t* within, int64_t rows,
                   const Rows& r, const Facts& h, const FastCarry& carry, int cw, const Out& o, Scratch& sc) {
  SeqKArgs sa{};
  sa.n = rows;
  sa.ts = a.ts;
  sa.st = a.st;
  sa.code = a.code;
  sa.consts = a.consts;
  sa.k = k;
  for (int m = 0; m < kSeqKMax; ++m) {
    sa.off[m] = m < k ? off[m] : 0;
    sa.len[m] = m < k ? len[m] : 0;
    sa.within[m] = m > 0 && m < k ? within[m] : -1;
  }
  sa.ordinals = a.ordinals;
  sa.obase = a.ordinal_base;
  sa.perm = r.perm;
  sa.skey = r.skey;
  sa.kmin = h.kmin;
  sa.kmax = h.kmax;
  sa.carry = (const int64_t*)carry.rows;
  sa.nc = carry.n;
  sa.cw = cw;
  sa.prev = (int32_t*)sc.take((size_t)a.n * 4);
  sa.hit = (uint8_t*)sc.take(((size_t)a.n + 3) & ~(size_t)3);
  sa.cand = o.cand;
  sa.cand_n = o.ctl;
  return sa;
}

// ---- out: the second and last round trip. Returns the outputs, *ncand the carry-out candidates
int64_t read_counts(Batch& b, const Out& o, int64_t out_cap, const Labels& L, int64_t* ncand) {
  uint32_t hc[2] = {0, 0};
  SM_HIP(hipMemcpyAsync(hc, o.ctl, 8, hipMemcpyDeviceToHost, b.s));
  SM_HIP(hipStreamSynchronize(b.s));
  // cannot happen (at most one output and one candidate per row or partial, and the capacity check): checked, not assumed
  if ((int64_t)hc[1] > out_cap || (int64_t)hc[0] > o.cand_cap) {
    b.leave(0);
    throw std::runtime_error(std::string(L.what) + ": output larger than its buffer");
  }
  *ncand = hc[0];
  return hc[1];
}

// after the link kernel of paths 7 and 8: the carried rows that stay, then the k-tuples in row order of the last event
// (counts: a word per tile of the batch's rows + 1, taken by the driver before its link kernel)
int64_t seqk_tuples_out(Batch& b, const FastArgs& a, const SeqKArgs& sa, bool wide, uint32_t* counts,
                        uint32_t* tuples_out, int64_t tuples_cap, const Out& o, const Labels& L, int64_t* ncand) {
  const int64_t n = a.n, ntiles = (n + kSeqTile - 1) / kSeqTile;
  const dim3 grid((unsigned)ntiles), block(kSeqBlock);
  if (sa.nc > 0) {
    if (wide) hipLaunchKernelGGL(seqk_keep_kernel<uint64_t>, seq_grid(sa.nc, kSeqBlock), block, 0, b.s, sa);
    else hipLaunchKernelGGL(seqk_keep_kernel<uint32_t>, seq_grid(sa.nc, kSeqBlock), block, 0, b.s, sa);
    b.mark(L.keep);
  }
  b.event(2);
  hipLaunchKernelGGL(seqk_count_kernel, grid, block, 0, b.s, (const uint8_t*)sa.hit, n, counts);
  b.mark(L.count);
  exclusive_scan_u32(counts, (size_t)ntiles, b.sc, b.s, o.ctl + 1);
  b.mark(L.scan);
  hipLaunchKernelGGL(seqk_emit_kernel, grid, block, 0, b.s, (const uint8_t*)sa.hit, (const int32_t*)sa.prev, n, sa.k,
                     (const uint32_t*)counts, a.ordinals, a.ordinal_base, sa.carry, sa.cw, tuples_out);
  b.mark(L.emit);
  return read_counts(b, o, tuples_cap, L, ncand);
}

// ---- carry out (build_carry reads the old rows before it replaces them); returns m
int64_t carry_out(Batch& b, const FastArgs& a, const Out& o, int64_t ncand, int nattr, int64_t ts_last, FastCarry& carry,
                  FastState& fs, int path, const Labels& L, int64_t m, bool key_runs_ordered = false,
                  const int32_t* row_stream = nullptr) {
  b.sc.used = o.keep;
  build_carry(o.cand, ncand, a.st, nattr, carry, b.sc, b.s, 64, 0, key_runs_ordered, row_stream);
  b.mark(L.carry);
  carry.ts_last = carry.active ? std::max<int64_t>(carry.ts_last, ts_last) : ts_last;
  carry.active = true;
  fs.last_path = path;
  b.event(3);
  return b.leave(m);
}

// the partition key of one stream's rows: a column, or the caller's dense ids
const void* seq_key_column(const FastHostInfo& hi, bool keyed, bool* key64) {
  *key64 = keyed && !hi.dense_keys && hi.key_type == T_LONG;
  return keyed ? (hi.dense_keys ? (const void*)hi.dense_keys : hi.cols[hi.key_col]) : nullptr;
}

}  // namespace

int64_t fast_seq_adjacent(const FastArgs& a, const FastHostInfo& hi, FastState& fs, FastCarry& carry,
                          uint32_t* pairs_out, int64_t pairs_cap, Scratch& sc, hipStream_t s, FastTimings* tm) {
  const Labels& L = kSeqLabels;
  const int64_t n = a.n;
  if (n == 0) return 0;
  if (n >= 0x7fffffffll) return FAST_OUTSIDE;
  const bool keyed = a.key != nullptr;
  if (keyed && (hi.key_col < 0 || !(hi.key_type == T_INT || hi.key_type == T_LONG))) return FAST_OUTSIDE;
  Batch b(sc, s, tm, true);
  bool key64;
  const void* kcol = seq_key_column(hi, keyed, &key64);
  const int nattr = hi.nattr, cw = 3 + nattr;
  const int64_t nc = carry.n;

  const Facts h = seq_facts(b, a, kcol, key64, carry, L.facts);
  int kbits;
  if (const int64_t r = envelope(h, a.within >= 0, keyed, true, carry, cw, hi.remap_span, &kbits)) return b.leave(r);

  const int64_t cand_cap = n + nc;
  {  // scratch for the worst case, before anything changes: sort pairs + links, then the carry build per candidate
    const uint64_t kmax_runs = keyed ? (kbits >= 62 ? (uint64_t)n : std::min<uint64_t>((uint64_t)n, (1ull << kbits))) : 1;
    // sort pairs twice over (+ a histogram word per 4 events), links, tile counts
    const size_t link = (size_t)n * (keyed ? (kbits > 32 ? 29 : 21) : 4) + (size_t)(n / kSeqTile + 2) * 4 + (8 << 20);
    const size_t build = (size_t)(kmax_runs + (uint64_t)nc) * (size_t)(8 * cw + 44) + (8 << 20);
    if (sc.used + (size_t)cand_cap * 32 + (size_t)nc + std::max(link, build) + 4096 > sc.cap) return b.leave(FAST_OUTSIDE);
  }
  const Out o = take_out(sc, cand_cap, (size_t)std::max<int64_t>(nc, 1));

  Rows rows;
  const bool wide = kbits > 32;
  if (keyed) {
    rows = seq_sort_rows(b, kcol, key64, n, h.kmin, kbits);
    b.mark(L.sort);
  }
  b.event(1);

  // ---- link
  const int64_t ntiles = (n + kSeqTile - 1) / kSeqTile;
  SM_HIP(hipMemsetAsync(o.ctl, 0, 8, s));
  if (nc > 0) SM_HIP(hipMemsetAsync(o.used, 0, (size_t)nc, s));
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
  sa.perm = rows.perm;
  sa.skey = rows.skey;
  sa.kmin = h.kmin;
  sa.carry = (const int64_t*)carry.rows;
  sa.nc = nc;
  sa.cw = cw;
  sa.e1 = (int32_t*)sc.take((size_t)n * 4);
  sa.used = o.used;
  sa.cand = o.cand;
  sa.cand_n = o.ctl;
  uint32_t* counts = (uint32_t*)sc.take((size_t)(ntiles + 1) * 4);
  sa.counts = keyed ? nullptr : counts;
  if (wide) hipLaunchKernelGGL(seq_link_kernel<uint64_t>, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, sa);
  else hipLaunchKernelGGL(seq_link_kernel<uint32_t>, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, sa);
  b.mark("seq_link");
  if (nc > 0) {
    hipLaunchKernelGGL(seq_keep_kernel, seq_grid(nc, kSeqBlock), dim3(kSeqBlock), 0, s, (const int64_t*)carry.rows, nc, cw,
                       (const uint8_t*)o.used, sa.cand, o.ctl);
    b.mark(L.keep);
  }
  b.event(2);

  // ---- pairs in row order: tile counts from the link pass, or (after a key sort) from seq_count_kernel
  if (keyed) {
    hipLaunchKernelGGL(seq_count_kernel, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, (const int32_t*)sa.e1, n, counts);
    b.mark(L.count);
  }
  exclusive_scan_u32(counts, (size_t)ntiles, sc, s, o.ctl + 1);
  b.mark(L.scan);
  hipLaunchKernelGGL(seq_emit_kernel, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, (const int32_t*)sa.e1, n,
                     (const uint32_t*)counts, a.ordinals, a.ordinal_base, pairs_out);
  b.mark(L.emit);
  int64_t ncand;
  const int64_t m = read_counts(b, o, pairs_cap, L, &ncand);
  return carry_out(b, a, o, ncand, nattr, h.ts_last, carry, fs, 6, L, m, true);
}

int64_t fast_seq_k(const FastArgs& a, const SeqKPlan& p, const FastHostInfo& hi, FastState& fs, FastCarry& carry,
                   uint32_t* tuples_out, int64_t tuples_cap, Scratch& sc, hipStream_t s, FastTimings* tm) {
  const Labels& L = kSeqKLabels;
  const int64_t n = a.n;
  const int k = p.k;
  if (k < 3 || k > kSeqKMax) return FAST_OUTSIDE;
  if (n == 0) return 0;
  if (n >= 0x7fffffffll) return FAST_OUTSIDE;
  const bool keyed = a.key != nullptr;
  if (keyed && (hi.key_col < 0 || !(hi.key_type == T_INT || hi.key_type == T_LONG))) return FAST_OUTSIDE;
  Batch b(sc, s, tm, true);
  bool key64;
  const void* kcol = seq_key_column(hi, keyed, &key64);
  const int nattr = hi.nattr, cw = 3 + nattr;
  const int64_t nc = carry.n;
  bool any_within = false;
  for (int m = 1; m < k; ++m) any_within |= p.within[m] >= 0;

  const Facts h = seq_facts(b, a, kcol, key64, carry, L.facts);
  int kbits;
  if (const int64_t r = envelope(h, any_within, keyed, n <= tuples_cap, carry, cw, hi.remap_span, &kbits))
    return b.leave(r);

  const int64_t cand_cap = n + nc;
  const int64_t ntiles = (n + kSeqTile - 1) / kSeqTile;
  {  // scratch for the worst case, before anything changes
    const uint64_t runs = keyed ? (kbits >= 62 ? (uint64_t)n : std::min<uint64_t>((uint64_t)n, (1ull << kbits))) : 1;
    const uint64_t ncand_max = std::min<uint64_t>((uint64_t)n, runs * (uint64_t)(k - 1)) + (uint64_t)nc;
    // sort pairs twice over (+ a histogram word per 4 events), links and hits, tile counts
    const size_t link = (size_t)n * (keyed ? (kbits > 32 ? 30 : 22) : 5) + (size_t)(ntiles + 2) * 4 + (8 << 20);
    const size_t build = (size_t)ncand_max * (size_t)(8 * cw + 44) + (8 << 20);
    if (sc.used + (size_t)cand_cap * 32 + std::max(link, build) + 4096 > sc.cap) return b.leave(FAST_OUTSIDE);
  }
  const Out o = take_out(sc, cand_cap);

  Rows rows;
  const bool wide = kbits > 32;
  if (keyed) {
    rows = seq_sort_rows(b, kcol, key64, n, h.kmin, kbits);
    b.mark(L.sort);
  }
  b.event(1);

  // ---- link: predecessor link and hit at every row, candidates = the last k - 1 rows of every run
  SM_HIP(hipMemsetAsync(o.ctl, 0, 8, s));
  const SeqKArgs sa = seqk_args(a, k, p.off, p.len, p.within, n, rows, h, carry, cw, o, sc);
  uint32_t* counts = (uint32_t*)sc.take((size_t)(ntiles + 1) * 4);
  if (wide) hipLaunchKernelGGL(seqk_link_kernel<uint64_t>, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, sa);
  else hipLaunchKernelGGL(seqk_link_kernel<uint32_t>, dim3((unsigned)ntiles), dim3(kSeqBlock), 0, s, sa);
  b.mark("seqk_link");

  int64_t ncand;
  const int64_t m = seqk_tuples_out(b, a, sa, wide, counts, tuples_out, tuples_cap, o, L, &ncand);
  // the candidates' order, which depends on the order of atomics, is not read: build_carry sorts by ordinal then key
  return carry_out(b, a, o, ncand, nattr, h.ts_last, carry, fs, 7, L, m);
}

void mseq_gather_keys(int64_t n, const int32_t* sid, const MSeqKeys& p, int64_t* keys, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(mseq_keys_kernel, seq_grid(n, 256), dim3(256), 0, s, mseq_src(n, sid, p), keys);
}

int64_t fast_seq_ms(const FastArgs& a, const int32_t* sid, const MSeqPlan& p, int nattr, FastState& fs,
                    FastCarry& carry, uint32_t* tuples_out, int64_t tuples_cap, Scratch& sc, hipStream_t s,
                    FastTimings* tm) {
  const Labels& L = kMSeqLabels;
  const int64_t n = a.n;
  const int k = p.k;
  if (k < 2 || k > kSeqKMax) return FAST_OUTSIDE;
  if (n == 0) return 0;
  if (n >= 0x7fffffffll) return FAST_OUTSIDE;
  const bool keyed = p.keyed;
  Batch b(sc, s, tm, false);
  const int cw = 4 + nattr;
  const int64_t nc = carry.n;
  bool any_within = false;
  for (int m = 1; m < k; ++m) any_within |= p.within[m] >= 0;
  const int64_t ntiles = (n + kSeqTile - 1) / kSeqTile;

  MSeqSrc src = mseq_src(n, sid, p);
  src.ts = a.ts;
  src.ordinals = a.ordinals;
  src.obase = a.ordinal_base;

  uint32_t* tile_n;
  const Facts h = mseq_facts(b, a, src, keyed, ntiles, carry, L.facts, &tile_n);
  const int64_t np = h.np;
  int kbits;
  if (const int64_t r = envelope(h, any_within, keyed, np <= tuples_cap, carry, cw, p.remap_span, &kbits))
    return b.leave(r);
  if (np == 0) {  // no row of a stream the query reads: its carried rows wait
    fs.last_path = 8;
    return b.leave(0);
  }
  const bool wide = kbits > 32;

  const int64_t cand_cap = np + nc;
  const int64_t ptiles = (np + kSeqTile - 1) / kSeqTile;
  {  // scratch for the worst case, before anything changes
    const uint64_t runs = keyed ? (kbits >= 62 ? (uint64_t)np : std::min<uint64_t>((uint64_t)np, (1ull << kbits))) : 1;
    const uint64_t ncand_max = std::min<uint64_t>((uint64_t)np, runs * (uint64_t)(k - 1)) + (uint64_t)nc;
    // per read row: sort pairs twice over (+ a histogram word per 4 events) and a stream byte; per row: link and hit
    const size_t link = (size_t)np * (keyed ? (wide ? 26 : 18) : 5) + (size_t)n * 5 + (size_t)(ntiles + 2) * 8 + (8 << 20);
    const size_t build = (size_t)ncand_max * (size_t)(8 * cw + 44) + (8 << 20);
    if (sc.used + (size_t)cand_cap * 32 + std::max(link, build) + 4096 > sc.cap) return b.leave(FAST_OUTSIDE);
  }
  const Out o = take_out(sc, cand_cap);

  const Rows rows = mseq_pack_sort(b, src, tile_n, ntiles, np, keyed, h.kmin, kbits, L);
  b.event(1);

  // ---- link: stream bytes, withins, conditions: hit and predecessor link at every read row
  SM_HIP(hipMemsetAsync(o.ctl, 0, 8, s));
  MSeqArgs ma{};
  ma.q = seqk_args(a, k, p.off, p.len, p.within, np, rows, h, carry, cw, o, sc);
  for (int m = 0; m < kSeqKMax; ++m) ma.want[m] = m < k ? (uint8_t)p.stream[m] : 0;
  ma.sstr = rows.sstr;
  ma.sid = sid;
  uint32_t* counts = (uint32_t*)sc.take((size_t)(ntiles + 1) * 4);
  // rows that are not read have no lane
  if (rows.perm) SM_HIP(hipMemsetAsync(ma.q.hit, 0, ((size_t)n + 3) & ~(size_t)3, s));
  if (wide) hipLaunchKernelGGL(mseq_link_kernel<uint64_t>, dim3((unsigned)ptiles), dim3(kSeqBlock), 0, s, ma);
  else hipLaunchKernelGGL(mseq_link_kernel<uint32_t>, dim3((unsigned)ptiles), dim3(kSeqBlock), 0, s, ma);
  b.mark("mseq_link");

  int64_t ncand;
  const int64_t m = seqk_tuples_out(b, a, ma.q, wide, counts, tuples_out, tuples_cap, o, L, &ncand);
  return carry_out(b, a, o, ncand, nattr, h.ts_last, carry, fs, 8, L, m, false, sid);
}

int64_t fast_pat_ms(const FastArgs& a, const int32_t* sid, const MPatPlan& p, int nattr, FastState& fs, FastCarry& carry,
                    uint32_t* pairs_out, int64_t pairs_cap, Scratch& sc, hipStream_t s, FastTimings* tm) {
  const Labels& L = kMPatLabels;
  const int64_t n = a.n;
  if (n == 0) return 0;
  const int64_t nc = carry.n;
  if (n >= 0x7fffffffll || n + nc >= 0x7fffffffll) return FAST_OUTSIDE;
  if (p.stream[0] < 0 || p.stream[0] >= kMSeqStreams || p.stream[1] < 0 || p.stream[1] >= kMSeqStreams)
    return FAST_OUTSIDE;
  const bool keyed = p.keyed;
  Batch b(sc, s, tm, false);
  const int cw = 3 + nattr;
  const int64_t ntiles = (n + kSeqTile - 1) / kSeqTile;

  MSeqSrc src = mseq_src(n, sid, p);
  src.ts = a.ts;
  src.ordinals = a.ordinals;
  src.obase = a.ordinal_base;

  uint32_t* tile_n;
  const Facts h = mseq_facts(b, a, src, keyed, ntiles, carry, L.facts, &tile_n);
  const int64_t np = h.np;
  int kbits;
  if (const int64_t r = envelope(h, p.within >= 0, keyed, np + nc <= pairs_cap, carry, cw, p.remap_span, &kbits))
    return b.leave(r);
  if (np == 0) {  // no row of a stream the query reads: its carried rows wait
    fs.last_path = 9;
    return b.leave(0);
  }
  const bool wide = kbits > 32;

  const int64_t cand_cap = np + nc;
  const int64_t total = nc + n;  // entries of `res`
  const int64_t rtiles = (total + kSeqTile - 1) / kSeqTile;
  const size_t hist = (size_t)8 << 20;
  {  // scratch up to the counts, for the worst case, before anything changes. Per read row: sort pairs twice over (+ a
     // histogram word per 4 rows) and a stream byte, then the (e2, e1) sort pairs twice over; per entry of res: 4 bytes
    const size_t link = (size_t)np * (keyed ? (wide ? 43 : 35) : 22) + (size_t)nc * 17 + (size_t)total * 4 +
                        (size_t)(ntiles + rtiles + 4) * 8 + hist;
    if (sc.used + (size_t)cand_cap * 32 + link + 4096 > sc.cap) return b.leave(FAST_OUTSIDE);
  }
  const Out o = take_out(sc, cand_cap);

  const Rows rows = mseq_pack_sort(b, src, tile_n, ntiles, np, keyed, h.kmin, kbits, L);
  b.event(1);

  // ---- link: every partial (carried rows, then A rows passing c1) scans forward in its key run for its e2
  SM_HIP(hipMemsetAsync(o.ctl, 0, 8, s));
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
  ma.ts_last = h.ts_last;
  ma.ordinals = a.ordinals;
  ma.obase = a.ordinal_base;
  ma.perm = rows.perm;
  ma.skey = rows.skey;
  ma.kmin = h.kmin;
  ma.kmax = h.kmax;
  ma.sstr = rows.sstr;
  ma.sid = sid;
  ma.sa = p.stream[0];
  ma.sb = p.stream[1];
  ma.carry = (const int64_t*)carry.rows;
  ma.nc = nc;
  ma.cw = cw;
  ma.res = (int32_t*)sc.take((size_t)total * 4);
  ma.cand = o.cand;
  ma.cand_n = o.ctl;
  uint32_t* counts = (uint32_t*)sc.take((size_t)(rtiles + 1) * 4);
  // rows that are not read have no lane: their entries are "none"
  if (np < n) SM_HIP(hipMemsetD32Async((hipDeviceptr_t)(ma.res + nc), (int)kSeqNone, (size_t)n, s));
  const dim3 lgrid((unsigned)((nc + np + kSeqTile - 1) / kSeqTile));
  if (wide) hipLaunchKernelGGL(mpat_link_kernel<uint64_t>, lgrid, dim3(kSeqBlock), 0, s, ma);
  else hipLaunchKernelGGL(mpat_link_kernel<uint32_t>, lgrid, dim3(kSeqBlock), 0, s, ma);
  b.mark("mpat_link");
  b.event(2);

  // ---- the two counts: pairs and carry-out candidates
  hipLaunchKernelGGL(seq_count_kernel, dim3((unsigned)rtiles), dim3(kSeqBlock), 0, s, (const int32_t*)ma.res, total, counts);
  b.mark(L.count);
  exclusive_scan_u32(counts, (size_t)rtiles, sc, s, o.ctl + 1);
  b.mark(L.scan);
  int64_t ncand;
  const int64_t m = read_counts(b, o, pairs_cap, L, &ncand);
  // room for the carry build, now that the number of candidates is known: still nothing is changed
  if (o.keep + (size_t)ncand * (size_t)(8 * cw + 44) + hist + 4096 > sc.cap) return b.leave(FAST_OUTSIDE);

  // ---- pairs in order of e1 (carried rows in carry order, then row order), then the stable sort by e2 alone over the
  // bits of the largest relative ordinal
  if (m > 0) {
    uint32_t* jk = (uint32_t*)sc.take((size_t)m * 4);
    uint32_t* jk2 = (uint32_t*)sc.take((size_t)m * 4);
    uint32_t* iv = (uint32_t*)sc.take((size_t)m * 4);
    uint32_t* iv2 = (uint32_t*)sc.take((size_t)m * 4);
    hipLaunchKernelGGL(mpat_emit_kernel, dim3((unsigned)rtiles), dim3(kSeqBlock), 0, s, (const int32_t*)ma.res, total, nc,
                       (const uint32_t*)counts, a.ordinals, a.ordinal_base, (const int64_t*)carry.rows, cw, jk, iv);
    b.mark(L.emit);
    const bool alt = sort_pairs(false, jk, jk2, iv, iv2, m, std::max(1, bits_of((uint64_t)h.omax)), b);
    hipLaunchKernelGGL(mpat_pairs_kernel, seq_grid(m, kSeqBlock), dim3(kSeqBlock), 0, s,
                       (const uint32_t*)(alt ? jk2 : jk), (const uint32_t*)(alt ? iv2 : iv), m, pairs_out);
    b.mark("mpat_order");
  }
  return carry_out(b, a, o, ncand, nattr, h.ts_last, carry, fs, 9, L, m);
}

int64_t fast_pat_k(const FastArgs& a, const int32_t* sid, const MPatKPlan& p, int nattr, FastState& fs, FastCarry& carry,
                   uint32_t* tuples_out, int64_t tuples_cap, Scratch& sc, hipStream_t s, FastTimings* tm) {
  const Labels& L = kMPatKLabels;
  const int64_t n = a.n;
  const int k = p.k, pw = k + 1;
  if (k < 3 || k > kSeqKMax) return FAST_OUTSIDE;
  if (n == 0) return 0;
  const int64_t ne = carry.n, ncp = carry.pn;
  if (n >= 0x7fffffffll || n + ncp >= 0x7fffffffll || n + ne >= 0x7fffffffll) return FAST_OUTSIDE;
  for (int m = 0; m < k; ++m)
    if (p.stream[m] < 0 || p.stream[m] >= kMSeqStreams || (m > 0 && p.within[m] < 0)) return FAST_OUTSIDE;
  if (ncp > 0 && carry.pw != pw) return FAST_OUTSIDE;
  const bool keyed = p.keyed;
  Batch b(sc, s, tm, false);
  const int cw = 4 + nattr;
  const int64_t ntiles = (n + kSeqTile - 1) / kSeqTile;

  MSeqSrc src = mseq_src(n, sid, p);
  src.ts = a.ts;
  src.ordinals = a.ordinals;
  src.obase = a.ordinal_base;

  uint32_t* tile_n;
  const Facts h = mseq_facts(b, a, src, keyed, ntiles, carry, L.facts, &tile_n);
  const int64_t np = h.np;
  int kbits;
  if (const int64_t r = envelope(h, true, keyed, np + ncp <= tuples_cap, carry, cw, p.remap_span, &kbits))
    return b.leave(r);
  if (np == 0) {  // no row of a stream the query reads: its carried partials wait
    fs.last_path = 10;
    return b.leave(0);
  }
  const bool wide = kbits > 32;

  const int64_t cand_cap = np + ne;  // every read row and every carried event at most once
  const int64_t total = ncp + n;     // entries of res / kept, rows of mid
  const int64_t rtiles = (total + kSeqTile - 1) / kSeqTile;
  const size_t hist = (size_t)8 << 20;
  {  // scratch up to the counts, for the worst case, before anything changes. Per read row: sort pairs twice over (+ a
     // histogram word per 4 rows) and a stream byte; per entry: result, kept and k - 1 members; a flag per event
    const size_t link = (size_t)np * (keyed ? (wide ? 27 : 19) : 6) + (size_t)total * 4 * (size_t)(k + 1) + (size_t)(ne + n) +
                        (size_t)(ntiles + 2 * rtiles + 8) * 8 + hist;
    if (sc.used + (size_t)cand_cap * 32 + link + 8192 > sc.cap) return b.leave(FAST_OUTSIDE);
  }
  uint32_t* npart = (uint32_t*)sc.take(8);  // the partials that stay
  const Out o = take_out(sc, cand_cap);

  const Rows rows = mseq_pack_sort(b, src, tile_n, ntiles, np, keyed, h.kmin, kbits, L);
  b.event(1);

  // ---- link: every partial (carried ones, then S1 rows passing c1) walks its key run through its states
  SM_HIP(hipMemsetAsync(o.ctl, 0, 8, s));
  MPatKArgs ma{};
  ma.np = np;
  ma.n = n;
  ma.ts = a.ts;
  ma.st = a.st;
  ma.code = a.code;
  ma.consts = a.consts;
  ma.k = k;
  for (int m = 0; m < kSeqKMax; ++m) {
    ma.off[m] = m < k ? p.off[m] : 0;
    ma.len[m] = m < k ? p.len[m] : 0;
    ma.within[m] = m > 0 && m < k ? p.within[m] : 0;
    ma.want[m] = m < k ? p.stream[m] : -2;
  }
  ma.ts_last = h.ts_last;
  ma.ordinals = a.ordinals;
  ma.obase = a.ordinal_base;
  ma.perm = rows.perm;
  ma.skey = rows.skey;
  ma.kmin = h.kmin;
  ma.kmax = h.kmax;
  ma.sstr = rows.sstr;
  ma.sid = sid;
  ma.evt = (const int64_t*)carry.rows;
  ma.ne = ne;
  ma.cw = cw;
  ma.parts = (const int64_t*)carry.parts;
  ma.ncp = ncp;
  ma.res = (int32_t*)sc.take((size_t)total * 4);
  ma.kept = (int32_t*)sc.take((size_t)total * 4);
  ma.mid = (int32_t*)sc.take((size_t)total * 4 * (size_t)(k - 1));
  ma.eflag = (uint8_t*)sc.take((size_t)(ne + n));
  uint32_t* counts = (uint32_t*)sc.take((size_t)(rtiles + 1) * 4);
  uint32_t* kcounts = (uint32_t*)sc.take((size_t)(rtiles + 1) * 4);
  SM_HIP(hipMemsetAsync(ma.eflag, 0, (size_t)(ne + n), s));
  // rows that are not read have no lane: their entries are "none"
  if (np < n) {
    SM_HIP(hipMemsetD32Async((hipDeviceptr_t)(ma.res + ncp), (int)kSeqNone, (size_t)n, s));
    SM_HIP(hipMemsetD32Async((hipDeviceptr_t)(ma.kept + ncp), (int)kSeqNone, (size_t)n, s));
  }
  const dim3 lgrid((unsigned)((ncp + np + kSeqTile - 1) / kSeqTile)), block(kSeqBlock);
  if (wide) hipLaunchKernelGGL(mpatk_link_kernel<uint64_t>, lgrid, block, 0, s, ma);
  else hipLaunchKernelGGL(mpatk_link_kernel<uint32_t>, lgrid, block, 0, s, ma);
  b.mark("mpatk_link");
  b.event(2);

  // ---- the three counts: tuples, partials that stay, and the events they hold
  const dim3 rgrid((unsigned)rtiles);
  hipLaunchKernelGGL(seq_count_kernel, rgrid, block, 0, s, (const int32_t*)ma.res, total, counts);
  hipLaunchKernelGGL(seq_count_kernel, rgrid, block, 0, s, (const int32_t*)ma.kept, total, kcounts);
  b.mark(L.count);
  exclusive_scan_u32(counts, (size_t)rtiles, sc, s, o.ctl + 1);
  exclusive_scan_u32(kcounts, (size_t)rtiles, sc, s, npart);
  b.mark(L.scan);
  MPatKCand ca{};
  ca.s = src;
  ca.evt = ma.evt;
  ca.ne = ne;
  ca.cw = cw;
  ca.eflag = ma.eflag;
  ca.cand = o.cand;
  ca.cand_n = o.ctl;
  hipLaunchKernelGGL(mpatk_cand_kernel, seq_grid(ne + n, kSeqBlock), block, 0, s, ca);
  b.mark(L.keep);
  uint32_t hpart = 0;
  SM_HIP(hipMemcpyAsync(&hpart, npart, 4, hipMemcpyDeviceToHost, s));
  int64_t ncand;
  const int64_t m = read_counts(b, o, tuples_cap, L, &ncand);
  const int64_t pk = hpart;
  // room for the tuples' sorts, the new partials and the carry build, now that the counts are known: still nothing is
  // changed
  // (per tuple: k words, two sort pairs and, as per read row above, a histogram word per 4 tuples for the sorts)
  if (sc.used + (size_t)m * (size_t)(4 * k + 17) + (size_t)pk * pw * 8 + hist + 8192 > sc.cap ||
      o.keep + (size_t)ncand * (size_t)(8 * cw + 44) + hist + 4096 > sc.cap)
    return b.leave(FAST_OUTSIDE);

  MPatKOut oa{};
  oa.s = src;
  oa.total = total;
  oa.ncp = ncp;
  oa.mid = ma.mid;
  oa.k = k;
  oa.evt = ma.evt;
  oa.cw = cw;
  oa.parts = ma.parts;
  // ---- the tuples in order of e1 (carried partials in their order, then row order), then stable sorts by e2, e3, ...,
  // ek in turn: the reference's (ek, ..., e1) order. ek is a batch row; an earlier member may be carried (negative)
  if (m > 0) {
    uint32_t* tup = (uint32_t*)sc.take((size_t)m * 4 * (size_t)k);
    uint32_t* key = (uint32_t*)sc.take((size_t)m * 4);
    uint32_t* key2 = (uint32_t*)sc.take((size_t)m * 4);
    uint32_t* idx = (uint32_t*)sc.take((size_t)m * 4);
    uint32_t* idx2 = (uint32_t*)sc.take((size_t)m * 4);
    oa.flags = ma.res;
    oa.offsets = counts;
    oa.tuples = tup;
    hipLaunchKernelGGL(mpatk_emit_kernel, rgrid, block, 0, s, oa);
    b.mark(L.emit);
    const int obits = std::max(1, bits_of((uint64_t)h.omax));
    for (int slot = 1; slot < k; ++slot) {  // idx: the tuples' order so far (the first pass writes 0 .. m - 1)
      const bool flip = slot < k - 1 && ne > 0;
      hipLaunchKernelGGL(mpatk_keys_kernel, seq_grid(m, kSeqBlock), block, 0, s, (const uint32_t*)tup, k, slot,
                         slot == 1 ? (const uint32_t*)nullptr : (const uint32_t*)idx, m, flip ? 0x80000000u : 0u, key, idx);
      if (sort_pairs(false, key, key2, idx, idx2, m, flip ? 32 : obits, b)) std::swap(idx, idx2);
    }
    hipLaunchKernelGGL(mpatk_tuples_kernel, seq_grid(m, kSeqBlock), block, 0, s, (const uint32_t*)tup, k,
                       (const uint32_t*)idx, m, tuples_out);
    b.mark("mpatk_order");
  }
  // ---- the partials that stay (the old ones are read until here), then their events
  if (pk > 0) {
    int64_t* pout = (int64_t*)sc.take((size_t)pk * pw * 8);
    oa.flags = ma.kept;
    oa.offsets = kcounts;
    oa.parts_out = pout;
    hipLaunchKernelGGL(mpatk_parts_kernel, rgrid, block, 0, s, oa);
    carry.reserve_parts(pk, pw, s);
    SM_HIP(hipMemcpyAsync(carry.parts, pout, (size_t)pk * pw * 8, hipMemcpyDeviceToDevice, s));
    b.mark("mpatk_parts");
  }
  carry.pn = pk;
  carry.pw = pw;
  return carry_out(b, a, o, ncand, nattr, h.ts_last, carry, fs, 10, L, m, false, sid);
}

namespace {
__global__ void absent_set_creation_kernel(int64_t* __restrict__ ks, int64_t state_slots, int word,
                                           const int64_t* __restrict__ create, int64_t n) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) ks[(int64_t)word * state_slots + k] = create[k];
}
}  // namespace

void absent_set_creation(int64_t* ks, int64_t state_slots, int word, const int64_t* create, int64_t n, hipStream_t s) {
  if (n <= 0) return;
  if (n > state_slots) throw std::runtime_error("timeout closed form: more instances than state slots");
  hipLaunchKernelGGL(absent_set_creation_kernel, seq_grid(n, 256), dim3(256), 0, s, ks, state_slots, word, create, n);
}

void AbsentInst::reserve(int64_t rows_needed) {
  if (rows_needed <= cap) return;
  int64_t* p = nullptr;
  const int64_t c = std::max<int64_t>(rows_needed, std::max<int64_t>(cap * 2, 1024));
  SM_HIP(hipMalloc(&p, (size_t)c * 16));
  if (rows) SM_HIP(hipFree(rows));
  rows = p;
  cap = c;
}

void AbsentInst::release() {
  if (rows) (void)hipFree(rows);
  rows = nullptr;
  n = cap = 0;
}

int64_t fast_absent(const FastArgs& a, const int32_t* sid, const int64_t* clk, const AbsentPlan& p, int nattr,
                    const char* blob_dev, FastState& fs, FastCarry& carry, AbsentInst& inst,
                    const std::function<AbsentOut(int64_t)>& out, Scratch& sc, hipStream_t s, FastTimings* tm) {
  const Labels& L = kAbsLabels;
  const int64_t n = a.n;
  if (n == 0) return 0;
  const int64_t nc = carry.n;
  if (n >= 0x7fffffffll || n + nc >= 0x7fffffffll || p.wait < 1) return FAST_OUTSIDE;
  if (p.stream[0] < 0 || p.stream[0] >= kMSeqStreams || p.stream[1] < 0 || p.stream[1] >= kMSeqStreams)
    return FAST_OUTSIDE;
  const bool keyed = p.keyed;
  Batch b(sc, s, tm, false);
  const int cw = 3 + nattr;
  const int64_t ntiles = (n + kSeqTile - 1) / kSeqTile;

  MSeqSrc src = mseq_src(n, sid, p);
  src.ts = a.ts;
  src.ordinals = a.ordinals;
  src.obase = a.ordinal_base;

  // ---- facts: a read row below the clock (read back with the facts), then path 8's
  uint32_t* below = (uint32_t*)sc.take(4);
  SM_HIP(hipMemsetAsync(below, 0, 4, s));
  hipLaunchKernelGGL(absent_clock_kernel, dim3((unsigned)std::min<int64_t>(ntiles, 2048)), dim3(kSeqBlock), 0, s, sid,
                     src.read, a.ts, clk, n, below);
  uint32_t hbelow = 0;
  SM_HIP(hipMemcpyAsync(&hbelow, below, 4, hipMemcpyDeviceToHost, s));
  uint32_t* tile_n;
  const Facts h = mseq_facts(b, a, src, keyed, ntiles, carry, L.facts, &tile_n);
  if (hbelow) return b.leave(FAST_NON_MONOTONE);
  const int64_t np = h.np;
  int kbits;
  if (const int64_t r = envelope(h, false, keyed, true, carry, cw, p.remap_span, &kbits)) return b.leave(r);
  const bool wide = kbits > 32;

  const int64_t cand_cap = np + nc;  // every partial at most once
  const int64_t total = nc + n;      // entries of res
  const int64_t rtiles = (total + kSeqTile - 1) / kSeqTile;
  const size_t hist = (size_t)8 << 20;
  // chunks of the count scan: persistent workgroups, eight per compute unit
  int cus = fs.cus;
  if (cus <= 0) {
    int dev = 0;
    SM_HIP(hipGetDevice(&dev));
    SM_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  }
  const int64_t want = std::max<int64_t>(1, (int64_t)cus * 8);
  const int64_t per = std::max<int64_t>(kSeqBlock, ((np + want - 1) / want + kSeqBlock - 1) / kSeqBlock * kSeqBlock);
  const int nchunks = (int)((np + per - 1) / per);
  const uint64_t runs = keyed ? (kbits >= 62 ? (uint64_t)np : std::min<uint64_t>((uint64_t)np, (1ull << kbits))) : 0;
  {  // scratch up to the counts, for the worst case, before anything changes. Per read row: sort pairs twice over (+ a
     // histogram word per 4 rows) and a stream byte, a flag and a cancelling position; per row a count; per entry of
     // res 4 bytes; per key run a new instance
    const size_t link = (size_t)np * ((keyed ? (wide ? 27 : 19) : 6) + 5) + (size_t)n * 4 + (size_t)total * 4 +
                        (size_t)runs * 16 + (size_t)(ntiles + rtiles + nchunks + 8) * 8 + hist;
    if (sc.used + (size_t)cand_cap * 32 + link + 8192 > sc.cap) return b.leave(FAST_OUTSIDE);
  }
  const Out o = take_out(sc, std::max<int64_t>(cand_cap, 1));

  Rows rows;
  if (np > 0) rows = mseq_pack_sort(b, src, tile_n, ntiles, np, keyed, h.kmin, kbits, L);
  b.event(1);

  SM_HIP(hipMemsetAsync(o.ctl, 0, 8, s));
  AbsArgs aa{};
  aa.np = np;
  aa.n = n;
  aa.ts = a.ts;
  aa.clk = clk;
  aa.st = a.st;
  aa.code = a.code;
  aa.consts = a.consts;
  aa.c1_off = p.off[0];
  aa.c1_len = p.len[0];
  aa.c2_off = p.off[1];
  aa.c2_len = p.len[1];
  aa.wait = p.wait;
  aa.ordinals = a.ordinals;
  aa.obase = a.ordinal_base;
  aa.perm = rows.perm;
  aa.skey = rows.skey;
  aa.kmin = h.kmin;
  aa.kmax = h.kmax;
  aa.sstr = rows.sstr;
  aa.sid = sid;
  aa.sa = p.stream[0];
  aa.sb = p.stream[1];
  aa.ka = keyed ? p.kcol[p.stream[0]] : nullptr;
  aa.ka_wide = (int)((p.wide >> p.stream[0]) & 1ull);
  aa.carry = (const int64_t*)carry.rows;
  aa.nc = nc;
  aa.cw = cw;
  aa.per = per;
  aa.nchunks = nchunks;
  aa.res = (int32_t*)sc.take((size_t)total * 4);
  aa.cand = o.cand;
  aa.cand_n = o.ctl;
  const dim3 block(kSeqBlock);
  // ---- next: the first cancelling row after every sorted position
  if (np > 0) {
    aa.fl = (uint8_t*)sc.take((size_t)np);
    aa.ccnt = (uint32_t*)sc.take((size_t)(nchunks + 1) * 4);
    aa.rk = (uint32_t*)sc.take((size_t)n * 4);
    aa.F = (uint32_t*)sc.take((size_t)np * 4);
    hipLaunchKernelGGL(absent_flag_kernel, dim3((unsigned)nchunks), block, 0, s, aa);
    hipLaunchKernelGGL(absent_chunk_kernel, dim3(1), block, 0, s, aa.ccnt, nchunks);
    hipLaunchKernelGGL(absent_next_kernel, dim3((unsigned)nchunks), block, 0, s, aa);
    b.mark("absent_next");
  }
  // ---- state: cancelled, due at p, or open
  if (wide) hipLaunchKernelGGL(absent_state_kernel<uint64_t>, dim3((unsigned)rtiles), block, 0, s, aa);
  else hipLaunchKernelGGL(absent_state_kernel<uint32_t>, dim3((unsigned)rtiles), block, 0, s, aa);
  b.mark("absent_state");
  b.event(2);

  // ---- the counts: outputs, carry-out candidates, new instances
  uint32_t* counts = (uint32_t*)sc.take((size_t)(rtiles + 1) * 4);
  hipLaunchKernelGGL(seq_count_kernel, dim3((unsigned)rtiles), block, 0, s, (const int32_t*)aa.res, total, counts);
  b.mark(L.count);
  exclusive_scan_u32(counts, (size_t)rtiles, sc, s, o.ctl + 1);
  b.mark(L.scan);
  int64_t* fresh = nullptr;
  uint32_t hfresh = 0;
  if (keyed && np > 0) {
    fresh = (int64_t*)sc.take((size_t)runs * 16);
    uint32_t* nfresh = (uint32_t*)sc.take(4);
    SM_HIP(hipMemsetAsync(nfresh, 0, 4, s));
    const dim3 g = seq_grid(np, kSeqBlock);
    if (wide)
      hipLaunchKernelGGL(absent_inst_kernel<uint64_t>, g, block, 0, s, aa, (const int64_t*)inst.rows, inst.n, fresh, nfresh);
    else
      hipLaunchKernelGGL(absent_inst_kernel<uint32_t>, g, block, 0, s, aa, (const int64_t*)inst.rows, inst.n, fresh, nfresh);
    SM_HIP(hipMemcpyAsync(&hfresh, nfresh, 4, hipMemcpyDeviceToHost, s));
  }
  int64_t ncand;
  const int64_t m = read_counts(b, o, total, L, &ncand);
  if ((uint64_t)hfresh > runs) {
    b.leave(0);
    throw std::runtime_error(std::string(L.what) + ": more new instances than key runs");
  }
  const int64_t ni = inst.n + (int64_t)hfresh;
  // room for the instance table's sort, the outputs' sorts and the carry build, now that the counts are known: still
  // nothing is changed
  if (sc.used + (hfresh ? (size_t)ni * 56 + hist : 0) + (size_t)m * (keyed ? 60 : 8) + 2 * hist + 8192 > sc.cap ||
      o.keep + (size_t)ncand * (size_t)(8 * cw + 44) + hist + 4096 > sc.cap)
    return b.leave(FAST_OUTSIDE);
  const AbsentOut ob = out(m);

  // ---- the instances this batch created join the table, which is sorted by key again
  if (hfresh > 0) {
    int64_t* all = (int64_t*)sc.take((size_t)ni * 16);
    int64_t* sorted = (int64_t*)sc.take((size_t)ni * 16);
    uint64_t* tk = (uint64_t*)sc.take((size_t)ni * 8);
    uint64_t* tk2 = (uint64_t*)sc.take((size_t)ni * 8);
    uint32_t* ti = (uint32_t*)sc.take((size_t)ni * 4);
    uint32_t* ti2 = (uint32_t*)sc.take((size_t)ni * 4);
    if (inst.n > 0) SM_HIP(hipMemcpyAsync(all, inst.rows, (size_t)inst.n * 16, hipMemcpyDeviceToDevice, s));
    SM_HIP(hipMemcpyAsync(all + 2 * inst.n, fresh, (size_t)hfresh * 16, hipMemcpyDeviceToDevice, s));
    const dim3 g = seq_grid(ni, kSeqBlock);
    hipLaunchKernelGGL(absent_inst_keys_kernel, g, block, 0, s, (const int64_t*)all, ni, tk, ti);
    const bool alt = radix_sort_pairs<uint64_t>(tk, tk2, ti, ti2, (size_t)ni, 0, 64, sc, s);
    hipLaunchKernelGGL(absent_inst_gather_kernel, g, block, 0, s, (const int64_t*)all, (const uint32_t*)(alt ? ti2 : ti), ni,
                       sorted);
    if (ni > inst.cap) {
      SM_HIP(hipStreamSynchronize(s));  // the kernels above read the old rows
      inst.reserve(ni);
    }
    SM_HIP(hipMemcpyAsync(inst.rows, sorted, (size_t)ni * 16, hipMemcpyDeviceToDevice, s));
    inst.n = ni;
    b.mark("absent_inst");
  }

  // ---- the outputs in order of res (carried rows in carry order, then row order): unkeyed that is the order of p;
  // keyed, stable sorts by the instance's creation ordinal, then by p
  if (m > 0) {
    uint32_t* pv = (uint32_t*)sc.take((size_t)m * 4);
    uint32_t* xv = (uint32_t*)sc.take((size_t)m * 4);
    hipLaunchKernelGGL(absent_emit_kernel, dim3((unsigned)rtiles), block, 0, s, (const int32_t*)aa.res, total,
                       (const uint32_t*)counts, pv, xv);
    b.mark(L.emit);
    AbsProj pa{};
    pa.pv = pv;
    pa.xv = xv;
    if (keyed) {
      int64_t* cr = (int64_t*)sc.take((size_t)m * 8);
      uint64_t* ck = (uint64_t*)sc.take((size_t)m * 8);
      uint64_t* ck2 = (uint64_t*)sc.take((size_t)m * 8);
      uint32_t* idx = (uint32_t*)sc.take((size_t)m * 4);
      uint32_t* idx2 = (uint32_t*)sc.take((size_t)m * 4);
      uint32_t* pk = (uint32_t*)sc.take((size_t)m * 4);
      uint32_t* pk2 = (uint32_t*)sc.take((size_t)m * 4);
      const dim3 g = seq_grid(m, kSeqBlock);
      hipLaunchKernelGGL(absent_create_kernel, g, block, 0, s, aa, (const uint32_t*)xv, m, (const int64_t*)inst.rows, inst.n,
                         cr, ck, idx);
      // creation ordinals are ordinals of rows up to this batch's last
      const int64_t omax = a.ordinal_base + (np > 0 ? h.omax : 0);
      const int cbits = omax < 0 ? 64 : std::min(64, std::max(1, bits_of((uint64_t)omax)));
      if (radix_sort_pairs<uint64_t>(ck, ck2, idx, idx2, (size_t)m, 0, cbits, sc, s)) std::swap(idx, idx2);
      hipLaunchKernelGGL(absent_pkeys_kernel, g, block, 0, s, (const uint32_t*)pv, (const uint32_t*)idx, m, pk);
      if (sort_pairs(false, pk, pk2, idx, idx2, m, std::max(1, bits_of((uint64_t)n)), b)) std::swap(idx, idx2);
      pa.order = idx;
      pa.cr = cr;
      b.mark("absent_order");
    }
    pa.m = m;
    pa.nc = nc;
    pa.carry = (const int64_t*)carry.rows;
    pa.cw = cw;
    pa.st = a.st;
    pa.ts = a.ts;
    pa.ordinals = a.ordinals;
    pa.obase = a.ordinal_base;
    pa.wait = p.wait;
    pa.blob = blob_dev;
    pa.e1 = ob.e1;
    pa.vals = ob.vals;
    pa.ts_out = ob.ts;
    pa.pos = ob.pos;
    pa.create = ob.create;
    hipLaunchKernelGGL(absent_project_kernel, seq_grid(m, kSeqBlock), block, 0, s, pa);
    b.mark("absent_project");
  }
  return carry_out(b, a, o, ncand, nattr, np > 0 ? h.ts_last : carry.ts_last, carry, fs, 11, L, m);
}

int64_t fast_pat_nand(const FastArgs& a, const int32_t* sid, const PNandPlan& p, int nattr, FastState& fs,
                      FastCarry& carry, uint32_t* pairs_out, int64_t pairs_cap, Scratch& sc, hipStream_t s,
                      FastTimings* tm) {
  const Labels& L = kPNandLabels;
  const int64_t n = a.n;
  if (n == 0) return 0;
  const int64_t nc = carry.n;
  if (n >= 0x7fffffffll || n + nc >= 0x7fffffffll || p.within < 0 || p.stream[1] == p.stream[2]) return FAST_OUTSIDE;
  for (int m = 0; m < 3; ++m)
    if (p.stream[m] < 0 || p.stream[m] >= kMSeqStreams) return FAST_OUTSIDE;
  const bool keyed = p.keyed;
  Batch b(sc, s, tm, false);
  const int cw = 3 + nattr;
  const int64_t ntiles = (n + kSeqTile - 1) / kSeqTile;

  MSeqSrc src = mseq_src(n, sid, p);
  src.ts = a.ts;
  src.ordinals = a.ordinals;
  src.obase = a.ordinal_base;

  uint32_t* tile_n;
  const Facts h = mseq_facts(b, a, src, keyed, ntiles, carry, L.facts, &tile_n);
  const int64_t np = h.np;
  int kbits;
  if (const int64_t r = envelope(h, true, keyed, np + nc <= pairs_cap, carry, cw, p.remap_span, &kbits))
    return b.leave(r);
  if (np == 0) {  // no row of a stream the query reads: its carried rows wait
    fs.last_path = 12;
    return b.leave(0);
  }
  const bool wide = kbits > 32;

  const int64_t cand_cap = np + nc;
  const int64_t total = nc + n;  // entries of `res`
  const int64_t rtiles = (total + kSeqTile - 1) / kSeqTile;
  const size_t hist = (size_t)8 << 20;
  // chunks of the count scan: persistent workgroups, eight per compute unit (as path 11)
  int cus = fs.cus;
  if (cus <= 0) {
    int dev = 0;
    SM_HIP(hipGetDevice(&dev));
    SM_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  }
  const int64_t want = std::max<int64_t>(1, (int64_t)cus * 8);
  const int64_t per = std::max<int64_t>(kSeqBlock, ((np + want - 1) / want + kSeqBlock - 1) / kSeqBlock * kSeqBlock);
  const int nchunks = (int)((np + per - 1) / per);
  {  // scratch up to the counts, for the worst case, before anything changes: path 9's, and per read row a flag and a
     // cancelling position, per row a count, per chunk a count
    const size_t link = (size_t)np * ((keyed ? (wide ? 43 : 35) : 22) + 5) + (size_t)n * 4 + (size_t)nc * 17 +
                        (size_t)total * 4 + (size_t)(ntiles + rtiles + nchunks + 8) * 8 + hist;
    if (sc.used + (size_t)cand_cap * 32 + link + 8192 > sc.cap) return b.leave(FAST_OUTSIDE);
  }
  const Out o = take_out(sc, cand_cap);

  const Rows rows = mseq_pack_sort(b, src, tile_n, ntiles, np, keyed, h.kmin, kbits, L);
  b.event(1);

  // ---- next: the first cancelling row (stream B and c2) after every sorted position
  const dim3 block(kSeqBlock);
  AbsArgs aa{};
  aa.np = np;
  aa.n = n;
  aa.ts = a.ts;
  aa.st = a.st;
  aa.code = a.code;
  aa.consts = a.consts;
  aa.c2_off = p.off[1];
  aa.c2_len = p.len[1];
  aa.perm = rows.perm;
  aa.skey = rows.skey;
  aa.sstr = rows.sstr;
  aa.sid = sid;
  aa.sb = p.stream[1];
  aa.per = per;
  aa.nchunks = nchunks;
  aa.fl = (uint8_t*)sc.take((size_t)np);
  aa.ccnt = (uint32_t*)sc.take((size_t)(nchunks + 1) * 4);
  aa.rk = (uint32_t*)sc.take((size_t)n * 4);
  aa.F = (uint32_t*)sc.take((size_t)np * 4);
  hipLaunchKernelGGL(absent_flag_kernel, dim3((unsigned)nchunks), block, 0, s, aa);
  hipLaunchKernelGGL(absent_chunk_kernel, dim3(1), block, 0, s, aa.ccnt, nchunks);
  hipLaunchKernelGGL(absent_next_kernel, dim3((unsigned)nchunks), block, 0, s, aa);
  b.mark("pnand_next");

  // ---- link: every partial (carried rows, then A rows passing c1) scans forward in its key run for its e3, up to its
  // cancel bound
  SM_HIP(hipMemsetAsync(o.ctl, 0, 8, s));
  PNandArgs pa{};
  MPatArgs& ma = pa.m;
  ma.np = np;
  ma.n = n;
  ma.ts = a.ts;
  ma.st = a.st;
  ma.code = a.code;
  ma.consts = a.consts;
  ma.c1_off = p.off[0];
  ma.c1_len = p.len[0];
  ma.c2_off = p.off[2];
  ma.c2_len = p.len[2];
  ma.within = p.within;
  ma.ts_last = h.ts_last;
  ma.ordinals = a.ordinals;
  ma.obase = a.ordinal_base;
  ma.perm = rows.perm;
  ma.skey = rows.skey;
  ma.kmin = h.kmin;
  ma.kmax = h.kmax;
  ma.sstr = rows.sstr;
  ma.sid = sid;
  ma.sa = p.stream[0];
  ma.sb = p.stream[2];
  ma.carry = (const int64_t*)carry.rows;
  ma.nc = nc;
  ma.cw = cw;
  ma.res = (int32_t*)sc.take((size_t)total * 4);
  ma.cand = o.cand;
  ma.cand_n = o.ctl;
  pa.fl = aa.fl;
  pa.rk = aa.rk;
  pa.F = aa.F;
  pa.nf = aa.ccnt + nchunks;
  uint32_t* counts = (uint32_t*)sc.take((size_t)(rtiles + 1) * 4);
  // rows that are not read have no lane: their entries are "none"
  if (np < n) SM_HIP(hipMemsetD32Async((hipDeviceptr_t)(ma.res + nc), (int)kSeqNone, (size_t)n, s));
  const dim3 lgrid((unsigned)((nc + np + kSeqTile - 1) / kSeqTile));
  if (wide) hipLaunchKernelGGL(pnand_link_kernel<uint64_t>, lgrid, block, 0, s, pa);
  else hipLaunchKernelGGL(pnand_link_kernel<uint32_t>, lgrid, block, 0, s, pa);
  b.mark("pnand_link");
  b.event(2);

  // ---- the two counts: pairs and carry-out candidates
  hipLaunchKernelGGL(seq_count_kernel, dim3((unsigned)rtiles), block, 0, s, (const int32_t*)ma.res, total, counts);
  b.mark(L.count);
  exclusive_scan_u32(counts, (size_t)rtiles, sc, s, o.ctl + 1);
  b.mark(L.scan);
  int64_t ncand;
  const int64_t m = read_counts(b, o, pairs_cap, L, &ncand);
  // room for the carry build, now that the number of candidates is known: still nothing is changed
  if (o.keep + (size_t)ncand * (size_t)(8 * cw + 44) + hist + 4096 > sc.cap) return b.leave(FAST_OUTSIDE);

  // ---- pairs in order of e1 (carried rows in carry order, then row order), then the stable sort by e3 alone over the
  // bits of the largest relative ordinal
  if (m > 0) {
    uint32_t* jk = (uint32_t*)sc.take((size_t)m * 4);
    uint32_t* jk2 = (uint32_t*)sc.take((size_t)m * 4);
    uint32_t* iv = (uint32_t*)sc.take((size_t)m * 4);
    uint32_t* iv2 = (uint32_t*)sc.take((size_t)m * 4);
    hipLaunchKernelGGL(mpat_emit_kernel, dim3((unsigned)rtiles), block, 0, s, (const int32_t*)ma.res, total, nc,
                       (const uint32_t*)counts, a.ordinals, a.ordinal_base, (const int64_t*)carry.rows, cw, jk, iv);
    b.mark(L.emit);
    const bool alt = sort_pairs(false, jk, jk2, iv, iv2, m, std::max(1, bits_of((uint64_t)h.omax)), b);
    hipLaunchKernelGGL(mpat_pairs_kernel, seq_grid(m, kSeqBlock), block, 0, s, (const uint32_t*)(alt ? jk2 : jk),
                       (const uint32_t*)(alt ? iv2 : iv), m, pairs_out);
    b.mark("pnand_order");
  }
  return carry_out(b, a, o, ncand, nattr, h.ts_last, carry, fs, 12, L, m);
}

int64_t fast_pat_logic(const FastArgs& a, const int32_t* sid, const PLogPlan& p, int nattr, FastState& fs,
                       FastCarry& carry, uint32_t* tuples_out, int64_t tuples_cap, Scratch& sc, hipStream_t s,
                       FastTimings* tm) {
  const Labels& L = kPLogLabels;
  const int64_t n = a.n;
  constexpr int pw = 4;
  if (n == 0) return 0;
  const int64_t ne = carry.n, ncp = carry.pn;
  if (n >= 0x7fffffffll || n + ncp >= 0x7fffffffll || n + ne >= 0x7fffffffll || p.within < 0 ||
      p.stream[1] == p.stream[2] || (p.land && (p.stream[0] == p.stream[1] || p.stream[0] == p.stream[2])))
    return FAST_OUTSIDE;
  for (int m = 0; m < 3; ++m)
    if (p.stream[m] < 0 || p.stream[m] >= kMSeqStreams) return FAST_OUTSIDE;
  if (ncp > 0 && carry.pw != pw) return FAST_OUTSIDE;
  const bool keyed = p.keyed;
  Batch b(sc, s, tm, false);
  const int cw = 4 + nattr;
  const int64_t ntiles = (n + kSeqTile - 1) / kSeqTile;

  MSeqSrc src = mseq_src(n, sid, p);
  src.ts = a.ts;
  src.ordinals = a.ordinals;
  src.obase = a.ordinal_base;

  uint32_t* tile_n;
  const Facts h = mseq_facts(b, a, src, keyed, ntiles, carry, L.facts, &tile_n);
  const int64_t np = h.np;
  int kbits;
  if (const int64_t r = envelope(h, true, keyed, np + ncp <= tuples_cap, carry, cw, p.remap_span, &kbits))
    return b.leave(r);
  if (np == 0) {  // no row of a stream the query reads: its carried partials wait
    fs.last_path = 13;
    return b.leave(0);
  }
  const bool wide = kbits > 32;

  const int64_t cand_cap = np + ne;  // every read row and every carried event at most once
  const int64_t total = ncp + n;     // entries of res / kept, rows of mid
  const int64_t rtiles = (total + kSeqTile - 1) / kSeqTile;
  const size_t hist = (size_t)8 << 20;
  {  // scratch up to the counts, for the worst case, before anything changes (as path 10 with k = 3, three members)
    const size_t link = (size_t)np * (keyed ? (wide ? 27 : 19) : 6) + (size_t)total * 20 + (size_t)(ne + n) +
                        (size_t)(ntiles + 2 * rtiles + 8) * 8 + hist;
    if (sc.used + (size_t)cand_cap * 32 + link + 8192 > sc.cap) return b.leave(FAST_OUTSIDE);
  }
  uint32_t* npart = (uint32_t*)sc.take(8);  // the partials that stay
  const Out o = take_out(sc, cand_cap);

  const Rows rows = mseq_pack_sort(b, src, tile_n, ntiles, np, keyed, h.kmin, kbits, L);
  b.event(1);

  // ---- link: every partial (carried ones, then A rows passing c1) scans its key run for its two members
  SM_HIP(hipMemsetAsync(o.ctl, 0, 8, s));
  PLogArgs ma{};
  ma.np = np;
  ma.n = n;
  ma.ts = a.ts;
  ma.st = a.st;
  ma.code = a.code;
  ma.consts = a.consts;
  for (int m = 0; m < 3; ++m) {
    ma.off[m] = p.off[m];
    ma.len[m] = p.len[m];
  }
  ma.within = p.within;
  ma.ts_last = h.ts_last;
  ma.ordinals = a.ordinals;
  ma.obase = a.ordinal_base;
  ma.perm = rows.perm;
  ma.skey = rows.skey;
  ma.kmin = h.kmin;
  ma.kmax = h.kmax;
  ma.sstr = rows.sstr;
  ma.sid = sid;
  ma.sa = p.stream[0];
  ma.sb = p.stream[1];
  ma.sc = p.stream[2];
  ma.evt = (const int64_t*)carry.rows;
  ma.ne = ne;
  ma.cw = cw;
  ma.parts = (const int64_t*)carry.parts;
  ma.ncp = ncp;
  ma.res = (int32_t*)sc.take((size_t)total * 4);
  ma.kept = (int32_t*)sc.take((size_t)total * 4);
  ma.mid = (int32_t*)sc.take((size_t)total * 12);
  ma.eflag = (uint8_t*)sc.take((size_t)(ne + n));
  uint32_t* counts = (uint32_t*)sc.take((size_t)(rtiles + 1) * 4);
  uint32_t* kcounts = (uint32_t*)sc.take((size_t)(rtiles + 1) * 4);
  SM_HIP(hipMemsetAsync(ma.eflag, 0, (size_t)(ne + n), s));
  // rows that are not read have no lane: their entries are "none"
  if (np < n) {
    SM_HIP(hipMemsetD32Async((hipDeviceptr_t)(ma.res + ncp), (int)kSeqNone, (size_t)n, s));
    SM_HIP(hipMemsetD32Async((hipDeviceptr_t)(ma.kept + ncp), (int)kSeqNone, (size_t)n, s));
  }
  const dim3 lgrid((unsigned)((ncp + np + kSeqTile - 1) / kSeqTile)), block(kSeqBlock);
  if (p.land) {
    if (wide) hipLaunchKernelGGL((plog_link_kernel<uint64_t, true>), lgrid, block, 0, s, ma);
    else hipLaunchKernelGGL((plog_link_kernel<uint32_t, true>), lgrid, block, 0, s, ma);
  } else {
    if (wide) hipLaunchKernelGGL((plog_link_kernel<uint64_t, false>), lgrid, block, 0, s, ma);
    else hipLaunchKernelGGL((plog_link_kernel<uint32_t, false>), lgrid, block, 0, s, ma);
  }
  b.mark("plog_link");
  b.event(2);

  // ---- the three counts: tuples, partials that stay, and the events they hold
  const dim3 rgrid((unsigned)rtiles);
  hipLaunchKernelGGL(seq_count_kernel, rgrid, block, 0, s, (const int32_t*)ma.res, total, counts);
  hipLaunchKernelGGL(seq_count_kernel, rgrid, block, 0, s, (const int32_t*)ma.kept, total, kcounts);
  b.mark(L.count);
  exclusive_scan_u32(counts, (size_t)rtiles, sc, s, o.ctl + 1);
  exclusive_scan_u32(kcounts, (size_t)rtiles, sc, s, npart);
  b.mark(L.scan);
  MPatKCand ca{};
  ca.s = src;
  ca.evt = ma.evt;
  ca.ne = ne;
  ca.cw = cw;
  ca.eflag = ma.eflag;
  ca.cand = o.cand;
  ca.cand_n = o.ctl;
  hipLaunchKernelGGL(mpatk_cand_kernel, seq_grid(ne + n, kSeqBlock), block, 0, s, ca);
  b.mark(L.keep);
  uint32_t hpart = 0;
  SM_HIP(hipMemcpyAsync(&hpart, npart, 4, hipMemcpyDeviceToHost, s));
  int64_t ncand;
  const int64_t m = read_counts(b, o, tuples_cap, L, &ncand);
  const int64_t pk = hpart;
  // room for the tuples' sort, the new partials and the carry build, now that the counts are known: still nothing is
  // changed (per tuple: three words, two sort pairs and a histogram word per 4 tuples)
  if (sc.used + (size_t)m * 29 + (size_t)pk * pw * 8 + hist + 8192 > sc.cap ||
      o.keep + (size_t)ncand * (size_t)(8 * cw + 44) + hist + 4096 > sc.cap)
    return b.leave(FAST_OUTSIDE);

  PLogOut oa{};
  oa.s = src;
  oa.total = total;
  oa.ncp = ncp;
  oa.mid = ma.mid;
  oa.evt = ma.evt;
  oa.cw = cw;
  oa.parts = ma.parts;
  // ---- the tuples in order of e1 (carried partials in their order, then row order), then one stable sort by the
  // completing member, which is always a batch row, over the bits of the largest relative ordinal
  if (m > 0) {
    uint32_t* tup = (uint32_t*)sc.take((size_t)m * 12);
    uint32_t* key = (uint32_t*)sc.take((size_t)m * 4);
    uint32_t* key2 = (uint32_t*)sc.take((size_t)m * 4);
    uint32_t* idx = (uint32_t*)sc.take((size_t)m * 4);
    uint32_t* idx2 = (uint32_t*)sc.take((size_t)m * 4);
    oa.flags = ma.res;
    oa.offsets = counts;
    oa.tuples = tup;
    oa.key = key;
    oa.idx = idx;
    hipLaunchKernelGGL(plog_emit_kernel, rgrid, block, 0, s, oa);
    b.mark(L.emit);
    if (sort_pairs(false, key, key2, idx, idx2, m, std::max(1, bits_of((uint64_t)h.omax)), b)) std::swap(idx, idx2);
    hipLaunchKernelGGL(mpatk_tuples_kernel, seq_grid(m, kSeqBlock), block, 0, s, (const uint32_t*)tup, 3,
                       (const uint32_t*)idx, m, tuples_out);
    b.mark("plog_order");
  }
  // ---- the partials that stay (the old ones are read until here), then their events
  if (pk > 0) {
    int64_t* pout = (int64_t*)sc.take((size_t)pk * pw * 8);
    oa.flags = ma.kept;
    oa.offsets = kcounts;
    oa.parts_out = pout;
    hipLaunchKernelGGL(plog_parts_kernel, rgrid, block, 0, s, oa);
    carry.reserve_parts(pk, pw, s);
    SM_HIP(hipMemcpyAsync(carry.parts, pout, (size_t)pk * pw * 8, hipMemcpyDeviceToDevice, s));
    b.mark("plog_parts");
  }
  carry.pn = pk;
  carry.pw = pw;
  return carry_out(b, a, o, ncand, nattr, h.ts_last, carry, fs, 13, L, m, false, sid);
}

int64_t fast_pat_count(const FastArgs& a, const int32_t* sid, const PCntPlan& p, int nattr, FastState& fs,
                       FastCarry& carry, uint32_t* tuples_out, int64_t tuples_cap, Scratch& sc, hipStream_t s,
                       FastTimings* tm) {
  const Labels& L = kPCntLabels;
  const int64_t n = a.n;
  const int pw = p.cmax + 5, mw = p.cmax + 1, tw = p.cmax + 2;
  if (n == 0) return 0;
  const int64_t ne = carry.n, ncp = carry.pn;
  if (n >= 0x7fffffffll || n + ncp >= 0x7fffffffll || n + ne >= 0x7fffffffll || p.within < 0 || p.cmin < 0 ||
      p.cmin > p.cmax || p.cmax < 1 || p.cmax > kPCntMax || p.stream[0] == p.stream[1] || p.stream[0] == p.stream[2] ||
      p.stream[1] == p.stream[2])
    return FAST_OUTSIDE;
  for (int m = 0; m < 3; ++m)
    if (p.stream[m] < 0 || p.stream[m] >= kMSeqStreams) return FAST_OUTSIDE;
  if (ncp > 0 && carry.pw != pw) return FAST_OUTSIDE;
  const bool keyed = p.keyed;
  Batch b(sc, s, tm, false);
  const int cw = 4 + nattr;
  const int64_t ntiles = (n + kSeqTile - 1) / kSeqTile;

  MSeqSrc src = mseq_src(n, sid, p);
  src.ts = a.ts;
  src.ordinals = a.ordinals;
  src.obase = a.ordinal_base;

  uint32_t* tile_n;
  const Facts h = mseq_facts(b, a, src, keyed, ntiles, carry, L.facts, &tile_n);
  const int64_t np = h.np;
  int kbits;
  if (const int64_t r = envelope(h, true, keyed, np + ncp <= tuples_cap, carry, cw, p.remap_span, &kbits))
    return b.leave(r);
  if (np == 0) {  // no row of a stream the query reads: its carried partials wait
    fs.last_path = 14;
    return b.leave(0);
  }
  const bool wide = kbits > 32;

  const int64_t cand_cap = np + ne;  // every read row and every carried event at most once
  const int64_t total = ncp + n;     // entries of res / kept, rows of mid
  const int64_t rtiles = (total + kSeqTile - 1) / kSeqTile;
  const size_t hist = (size_t)8 << 20;
  {  // scratch up to the counts, for the worst case, before anything changes
    const size_t link = (size_t)np * (keyed ? (wide ? 27 : 19) : 6) + (size_t)total * (8 + 4 * mw) + (size_t)(ne + n) +
                        (size_t)(ntiles + 2 * rtiles + 8) * 8 + hist;
    if (sc.used + (size_t)cand_cap * 32 + link + 8192 > sc.cap) return b.leave(FAST_OUTSIDE);
  }
  uint32_t* npart = (uint32_t*)sc.take(8);  // the partials that stay
  const Out o = take_out(sc, cand_cap);

  const Rows rows = mseq_pack_sort(b, src, tile_n, ntiles, np, keyed, h.kmin, kbits, L);
  b.event(1);

  // ---- link: every partial (carried ones, then A rows passing c1) scans its key run for its hits and its e3
  SM_HIP(hipMemsetAsync(o.ctl, 0, 8, s));
  PCntArgs ma{};
  ma.np = np;
  ma.n = n;
  ma.ts = a.ts;
  ma.st = a.st;
  ma.code = a.code;
  ma.consts = a.consts;
  for (int m = 0; m < 3; ++m) {
    ma.off[m] = p.off[m];
    ma.len[m] = p.len[m];
  }
  ma.cmin = p.cmin;
  ma.cmax = p.cmax;
  ma.within = p.within;
  ma.ts_last = h.ts_last;
  ma.ordinals = a.ordinals;
  ma.obase = a.ordinal_base;
  ma.perm = rows.perm;
  ma.skey = rows.skey;
  ma.kmin = h.kmin;
  ma.kmax = h.kmax;
  ma.sstr = rows.sstr;
  ma.sid = sid;
  ma.sa = p.stream[0];
  ma.sb = p.stream[1];
  ma.sc = p.stream[2];
  ma.evt = (const int64_t*)carry.rows;
  ma.ne = ne;
  ma.cw = cw;
  ma.parts = (const int64_t*)carry.parts;
  ma.ncp = ncp;
  ma.res = (int32_t*)sc.take((size_t)total * 4);
  ma.kept = (int32_t*)sc.take((size_t)total * 4);
  ma.mid = (int32_t*)sc.take((size_t)total * 4 * mw);
  ma.eflag = (uint8_t*)sc.take((size_t)(ne + n));
  uint32_t* counts = (uint32_t*)sc.take((size_t)(rtiles + 1) * 4);
  uint32_t* kcounts = (uint32_t*)sc.take((size_t)(rtiles + 1) * 4);
  SM_HIP(hipMemsetAsync(ma.eflag, 0, (size_t)(ne + n), s));
  // rows that are not read have no lane: their entries are "none"
  if (np < n) {
    SM_HIP(hipMemsetD32Async((hipDeviceptr_t)(ma.res + ncp), (int)kSeqNone, (size_t)n, s));
    SM_HIP(hipMemsetD32Async((hipDeviceptr_t)(ma.kept + ncp), (int)kSeqNone, (size_t)n, s));
  }
  const dim3 lgrid((unsigned)((ncp + np + kSeqTile - 1) / kSeqTile)), block(kSeqBlock);
  if (wide) hipLaunchKernelGGL(pcnt_link_kernel<uint64_t>, lgrid, block, 0, s, ma);
  else hipLaunchKernelGGL(pcnt_link_kernel<uint32_t>, lgrid, block, 0, s, ma);
  b.mark("pcnt_link");
  b.event(2);

  // ---- the three counts: tuples, partials that stay, and the events they hold
  const dim3 rgrid((unsigned)rtiles);
  hipLaunchKernelGGL(seq_count_kernel, rgrid, block, 0, s, (const int32_t*)ma.res, total, counts);
  hipLaunchKernelGGL(seq_count_kernel, rgrid, block, 0, s, (const int32_t*)ma.kept, total, kcounts);
  b.mark(L.count);
  exclusive_scan_u32(counts, (size_t)rtiles, sc, s, o.ctl + 1);
  exclusive_scan_u32(kcounts, (size_t)rtiles, sc, s, npart);
  b.mark(L.scan);
  MPatKCand ca{};
  ca.s = src;
  ca.evt = ma.evt;
  ca.ne = ne;
  ca.cw = cw;
  ca.eflag = ma.eflag;
  ca.cand = o.cand;
  ca.cand_n = o.ctl;
  hipLaunchKernelGGL(mpatk_cand_kernel, seq_grid(ne + n, kSeqBlock), block, 0, s, ca);
  b.mark(L.keep);
  uint32_t hpart = 0;
  SM_HIP(hipMemcpyAsync(&hpart, npart, 4, hipMemcpyDeviceToHost, s));
  int64_t ncand;
  const int64_t m = read_counts(b, o, tuples_cap, L, &ncand);
  const int64_t pk = hpart;
  // the cap on the open partials, which no window bounds: pcnt_carry_cap (fastpath.h), and the tuples' sort, the new partial table and the carry build
  // must fit the scratch, now that the counts are known: still nothing is changed (per tuple: n + 2 words, two 64-bit
  // sort keys, two indices and a histogram word per 4 tuples)
  if (pk > pcnt_carry_cap(n, p.cmax, cw) ||
      sc.used + (size_t)m * (4 * tw + 25) + (size_t)pk * pw * 8 + hist + 8192 > sc.cap ||
      o.keep + (size_t)ncand * (size_t)(8 * cw + 44) + hist + 4096 > sc.cap)
    return b.leave(FAST_OUTSIDE);

  PCntOut oa{};
  oa.s = src;
  oa.total = total;
  oa.ncp = ncp;
  oa.mid = ma.mid;
  oa.cmin = p.cmin;
  oa.cmax = p.cmax;
  oa.evt = ma.evt;
  oa.cw = cw;
  oa.parts = ma.parts;
  // ---- the tuples in order of e1 (carried partials in their order, then row order), then one stable sort by (e3, p):
  // e3 is always a batch row, over the bits of the largest relative ordinal; p may be a carried event, sign-flipped
  if (m > 0) {
    uint32_t* tup = (uint32_t*)sc.take((size_t)m * 4 * tw);
    uint64_t* key = (uint64_t*)sc.take((size_t)m * 8);
    uint64_t* key2 = (uint64_t*)sc.take((size_t)m * 8);
    uint32_t* idx = (uint32_t*)sc.take((size_t)m * 4);
    uint32_t* idx2 = (uint32_t*)sc.take((size_t)m * 4);
    oa.flags = ma.res;
    oa.offsets = counts;
    oa.tuples = tup;
    oa.key = key;
    oa.idx = idx;
    hipLaunchKernelGGL(pcnt_emit_kernel, rgrid, block, 0, s, oa);
    b.mark(L.emit);
    if (sort_pairs(true, key, key2, idx, idx2, m, 32 + std::max(1, bits_of((uint64_t)h.omax)), b)) std::swap(idx, idx2);
    hipLaunchKernelGGL(mpatk_tuples_kernel, seq_grid(m, kSeqBlock), block, 0, s, (const uint32_t*)tup, tw,
                       (const uint32_t*)idx, m, tuples_out);
    b.mark("pcnt_order");
  }
  // ---- the partials that stay (the old ones are read until here), then their events
  if (pk > 0) {
    int64_t* pout = (int64_t*)sc.take((size_t)pk * pw * 8);
    oa.flags = ma.kept;
    oa.offsets = kcounts;
    oa.parts_out = pout;
    hipLaunchKernelGGL(pcnt_parts_kernel, rgrid, block, 0, s, oa);
    carry.reserve_parts(pk, pw, s);
    SM_HIP(hipMemcpyAsync(carry.parts, pout, (size_t)pk * pw * 8, hipMemcpyDeviceToDevice, s));
    b.mark("pcnt_parts");
  }
  carry.pn = pk;
  carry.pw = pw;
  return carry_out(b, a, o, ncand, nattr, h.ts_last, carry, fs, 14, L, m, false, sid);
}

}  // namespace sm
