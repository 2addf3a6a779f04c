// Device side of the closed form of the timeout pattern over one or two streams of one schema (seqpath.hip fast_absent):
//   @app:playback [partition with (ka of A, kb of B)] from every e1=A[c1] -> not B[c2] for W select <e1, constants>
// B may be A itself; c2 reads the B event and constants only. Fed as one interleaved batch with a stream index per row
// (sm_app_process_device_events). R = {A, B}. Positions are rows of the feed, heartbeat rows (-1) and rows of unread
// streams included; clock[q] is the running maximum of ts over all rows up to q, starting at the app's clock
// (build_event_index's ev_clock). A row of R belongs to the instance of its own stream's key attribute. Every A row i
// with c1(i) opens a partial with deadline d = ts[i] + W. It is
//     cancelled  iff a row j > i of B exists in the same instance with c2(j) and ts[j] < d (a B row at d is too late:
//                the timer fires on the clock advance before that row is processed),
//     emitted    otherwise, at p(i) = the first position q > i with clock[q] >= d (any row), as e1's select values with
//                timestamp d, and
//     open       while no such position exists: carried to the next batch.
// Outputs in order of (p, creation ordinal of the instance, i); an instance is created by the first row of a stream in R
// with its key. The rule needs every read row at the clock (ts[i] = clock[i]): a batch with a read row below it leaves
// before anything changes (FAST_NON_MONOTONE). tests/test_absent_plan.py ties this statement to the oracle.
//
// Facts, pack, the stable key sort and the stream byte of every sorted position are mseq_dev.h's, with R = {A, B}.
//   absent_clock_kernel  read rows below the clock
//   absent_next          next[s] = the first cancelling row (stream B and c2, through the interpreter) strictly after
//                        sorted position s in its key run. Within a run that is the nearest cancelling position to the
//                        right, so the segmented reverse min-scan of the cancelling rows' times is stated as a count:
//                        with F the cancelling positions in sorted order and cnt(s) their number at or before s, the
//                        candidate is F[cnt(s)], and it is the answer iff it has s's key. Reduce-then-scan over
//                        persistent workgroups, each owning one contiguous chunk of the sorted positions:
//                          absent_flag_kernel   c2 at every B position: a flag byte, and the chunk's count
//                          absent_chunk_kernel  the exclusive scan of the chunk counts (one workgroup; the chunks' carries
//                                               pass between the two launches here: no workgroup waits on another)
//                          absent_next_kernel   the block scans of the flags (the DPP scans of fastpath_dev.h) on top of
//                                               the chunk's carry: cnt(s) written at s's own row, F compacted
//                        A run across many chunks (unkeyed: every chunk) needs nothing more: the key compare is all
//                        that is segmented.
//   absent_state_kernel  one lane per partial in arrival order, carried rows (which passed c1 when they were kept) in
//                        front: res[place] = p, or kSeqNone when the partial is cancelled or stays open; the open ones
//                        are the carry-out candidates. A carried row finds its key's run by binary search of the sorted
//                        batch keys and takes the run's first cancelling row. p is a binary search of the clock column;
//                        deadlines are monotone in arrival order, so neighbouring lanes probe the same lines.
//   absent_emit_kernel   after seq_count_kernel over `res` and the exclusive scan of the tile counts: (p, place) compacted
//                        in order of `res`: carried rows in (key, ordinal) order, then batch rows. Unkeyed that is the
//                        order of p already
//   absent_inst_*        the instances' creation ordinals, a table of [key, ordinal] rows sorted by key that lives with
//                        the carry: the heads of the batch's key runs that miss it are appended, then it is sorted again
//   absent_create_kernel keyed: each output's creation ordinal, for the stable sorts by (p, creation ordinal)
//   absent_project_kernel  the outputs in their final order: e1's relative ordinal, the select programs over e1 (a batch
//                        row, or a carried row's canonical words), timestamp d, trigger position and creation ordinal
// Every wave operation is convergent, so the source also runs under the host wave emulator (tests/native/absent_emu.cpp).
#pragma once
#include "mseq_dev.h"

namespace sm {
namespace {

struct AbsArgs {
  int64_t np;               // read rows = sorted positions
  int64_t n;                // rows of the batch
  const int64_t* ts;
  const int64_t* clk;       // clock[q] of every row
  const NfaStream* st;
  const Instr* code;
  const DVal* consts;
  int c1_off, c1_len, c2_off, c2_len;
  int64_t wait;             // W
  const int64_t* ordinals;  // or nullptr: obase + row
  int64_t obase;
  const uint32_t* perm;     // row of each sorted position, or nullptr: every row is read, unkeyed
  const void* skey;         // key - kmin of each sorted position (K), or nullptr: unpartitioned
  int64_t kmin, kmax;
  const uint8_t* sstr;      // stream of each sorted position, or nullptr: sid[position]
  const int32_t* sid;
  int sa, sb;               // app streams of A and B
  const void* ka;           // A's key column (int32, or int64 when ka_wide), or nullptr: unpartitioned
  int ka_wide;
  const int64_t* carry;     // carried e1 rows [key, global ordinal, ts, attributes], sorted by (key, ordinal)
  int64_t nc;
  int cw;
  int64_t per;              // sorted positions per chunk (a multiple of kSeqBlock)
  int nchunks;
  uint8_t* fl;              // np flags: the position is a cancelling row
  uint32_t* ccnt;           // nchunks + 1: chunk counts, then their exclusive scan and the total
  uint32_t* rk;             // by row: cancelling positions at or before the row's sorted position
  uint32_t* F;              // the cancelling positions in sorted order
  int32_t* res;             // out: nc + n entries (entries of rows that are not read are filled by the host)
  int64_t* cand;            // out: carry-out candidates (key, global ordinal, ts, source: batch row or -(carried row) - 1)
  uint32_t* cand_n;
};

__device__ __forceinline__ int32_t abs_stream(const AbsArgs& a, int64_t u) {
  return a.sstr ? (int32_t)a.sstr[u] : a.sid[u];
}
__device__ __forceinline__ int64_t abs_row(const AbsArgs& a, int64_t u) { return a.perm ? (int64_t)a.perm[u] : u; }

// flag[0] |= 1 when a row of a read stream lies below the clock
__global__ void __launch_bounds__(kSeqBlock) absent_clock_kernel(const int32_t* __restrict__ sid, uint64_t read,
                                                                 const int64_t* __restrict__ ts,
                                                                 const int64_t* __restrict__ clk, int64_t n,
                                                                 uint32_t* __restrict__ flag) {
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * kSeqBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kSeqBlock) {
    const int32_t sd = sid[i];
    if (sd >= 0 && sd < kMSeqStreams && ((read >> sd) & 1ull)) bad |= ts[i] < clk[i];
  }
  const bool any = __any(bad);
  if ((threadIdx.x & 63) == 0 && any) atomicOr(flag, 1u);
}

__global__ void __launch_bounds__(kSeqBlock) absent_flag_kernel(AbsArgs a) {
  __shared__ uint32_t wsum[kSeqBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const Cond c2 = make_cond(a.code + a.c2_off, a.c2_len, a.consts);
  const int64_t lo = (int64_t)blockIdx.x * a.per;
  const int64_t hi = lo + a.per < a.np ? lo + a.per : a.np;
  uint32_t cnt = 0;
  for (int64_t u0 = lo; u0 < hi; u0 += kSeqBlock) {
    const int64_t u = u0 + threadIdx.x;
    if (u < hi) {
      const bool f = abs_stream(a, u) == a.sb && eval(c2, RowLoader{a.st, abs_row(a, u)});
      a.fl[u] = f ? 1 : 0;
      cnt += f ? 1u : 0u;
    }
  }
  const uint32_t inc = wave_incl_scan(cnt);
  if (lane == 63) wsum[w] = inc;
  lds_barrier();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
    for (int k = 0; k < kSeqBlock / 64; ++k) s += wsum[k];
    a.ccnt[blockIdx.x] = s;
  }
}

// one workgroup: ccnt[0 .. g) becomes its exclusive scan, ccnt[g] the total
__global__ void __launch_bounds__(kSeqBlock) absent_chunk_kernel(uint32_t* __restrict__ ccnt, int g) {
  __shared__ uint32_t lw[kSeqBlock / 64];
  uint32_t base = 0;
  for (int g0 = 0; g0 < g; g0 += kSeqBlock) {
    const int c = g0 + (int)threadIdx.x;
    const uint32_t v = c < g ? ccnt[c] : 0u;
    uint32_t tot;
    const uint32_t ex = block_excl<kSeqBlock>(v, lw, &tot);
    if (c < g) ccnt[c] = base + ex;
    base += tot;
    lds_barrier();  // lw is read before the next round writes it
  }
  if (threadIdx.x == 0) ccnt[g] = base;
}

__global__ void __launch_bounds__(kSeqBlock) absent_next_kernel(AbsArgs a) {
  __shared__ uint32_t lw[kSeqBlock / 64];
  const int64_t lo = (int64_t)blockIdx.x * a.per;
  const int64_t hi = lo + a.per < a.np ? lo + a.per : a.np;
  uint32_t base = a.ccnt[blockIdx.x];
  for (int64_t u0 = lo; u0 < hi; u0 += kSeqBlock) {
    const int64_t u = u0 + threadIdx.x;
    const uint32_t f = u < hi ? (uint32_t)a.fl[u] : 0u;
    uint32_t tot;
    const uint32_t ex = block_excl<kSeqBlock>(f, lw, &tot);
    if (u < hi) {
      a.rk[abs_row(a, u)] = base + ex + f;
      if (f) a.F[base + ex] = (uint32_t)u;
    }
    base += tot;
    lds_barrier();
  }
}

template <typename K>
__global__ void __launch_bounds__(kSeqBlock) absent_state_kernel(AbsArgs a) {
  const K* skey = (const K*)a.skey;
  const Cond c1 = make_cond(a.code + a.c1_off, a.c1_len, a.consts);
  const uint32_t nf = a.np > 0 ? a.ccnt[a.nchunks] : 0u;
  for (int it = 0; it < kSeqItems; ++it) {
    const int64_t v = (int64_t)blockIdx.x * kSeqTile + it * kSeqBlock + threadIdx.x;
    bool part = false;
    int64_t t1 = 0, src = 0, key = 0;
    uint32_t r = nf;  // the candidate's place in F
    K kk = (K)0;
    if (v < a.nc) {
      const int64_t* c = a.carry + v * a.cw;
      key = c[0];
      t1 = c[2];
      src = -v - 1;
      part = true;
      if (a.np > 0) {
        if (!skey) {
          r = 0;
        } else if (key >= a.kmin && key <= a.kmax) {  // the head of the key's run, if it has rows here
          kk = (K)((uint64_t)key - (uint64_t)a.kmin);
          int64_t lo = 0, hi = a.np;
          while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (skey[mid] < kk) lo = mid + 1;
            else hi = mid;
          }
          if (lo < a.np && skey[lo] == kk) r = a.rk[abs_row(a, lo)] - (uint32_t)a.fl[lo];
        }
      }
    } else if (v < a.nc + a.n) {
      const int64_t i = v - a.nc;
      if (a.sid[i] == a.sa && eval(c1, RowLoader{a.st, i})) {
        part = true;
        t1 = a.ts[i];
        src = i;
        r = a.rk[i];
        if (a.ka) {
          key = a.ka_wide ? ((const int64_t*)a.ka)[i] : (int64_t)((const int32_t*)a.ka)[i];
          kk = (K)((uint64_t)key - (uint64_t)a.kmin);
        }
      }
    }
    int32_t found = kSeqNone;
    bool open = false;
    if (part) {
      const int64_t d = t1 + a.wait;
      bool cancelled = false;
      if (r < nf) {
        const int64_t uf = (int64_t)a.F[r];
        if (!skey || skey[uf] == kk) cancelled = a.ts[abs_row(a, uf)] < d;
      }
      if (!cancelled) {
        int64_t lo = 0, hi = a.n;
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if (a.clk[mid] < d) lo = mid + 1;
          else hi = mid;
        }
        if (lo < a.n) found = (int32_t)lo;
        else open = true;
      }
    }
    if (v < a.nc + a.n) a.res[v] = found;
    const uint32_t slot = seq_wave_slot(open, a.cand_n);
    if (open) {
      int64_t* c = a.cand + 4 * (int64_t)slot;
      c[0] = key;
      c[1] = src < 0 ? a.carry[(-src - 1) * a.cw + 1] : (a.ordinals ? a.ordinals[src] : a.obase + src);
      c[2] = t1;
      c[3] = src;
    }
  }
}

// offsets = exclusive scan of seq_count_kernel's tile counts over res[0 .. total): pv[m] = p and xv[m] = the place of
// the m-th entry that is not kSeqNone
__global__ void __launch_bounds__(kSeqBlock) absent_emit_kernel(const int32_t* __restrict__ res, int64_t total,
                                                                const uint32_t* __restrict__ offsets,
                                                                uint32_t* __restrict__ pv, uint32_t* __restrict__ xv) {
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
      pv[p] = (uint32_t)v[k];
      xv[p] = (uint32_t)(r0 + k);
      ++p;
    }
}

// row of `key` in the instance table ([key, creation ordinal] rows sorted by key), or -1
__device__ __forceinline__ int64_t abs_inst_find(const int64_t* tab, int64_t ni, int64_t key) {
  int64_t lo = 0, hi = ni;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (tab[2 * mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < ni && tab[2 * lo] == key ? lo : -1;
}

// the heads of the batch's key runs whose key the table does not hold: a run's head is the key's first read row
template <typename K>
__global__ void __launch_bounds__(kSeqBlock) absent_inst_kernel(AbsArgs a, const int64_t* __restrict__ tab, int64_t ni,
                                                                int64_t* __restrict__ fresh, uint32_t* __restrict__ nfresh) {
  const K* skey = (const K*)a.skey;
  const int64_t u = (int64_t)blockIdx.x * kSeqBlock + threadIdx.x;
  bool miss = false;
  int64_t key = 0;
  if (u < a.np && (u == 0 || skey[u - 1] != skey[u])) {
    key = a.kmin + (int64_t)skey[u];
    miss = abs_inst_find(tab, ni, key) < 0;
  }
  const uint32_t slot = seq_wave_slot(miss, nfresh);
  if (miss) {
    const int64_t j = abs_row(a, u);
    fresh[2 * (int64_t)slot] = key;
    fresh[2 * (int64_t)slot + 1] = a.ordinals ? a.ordinals[j] : a.obase + j;
  }
}

__global__ void __launch_bounds__(kSeqBlock) absent_inst_keys_kernel(const int64_t* __restrict__ rows, int64_t n,
                                                                     uint64_t* __restrict__ keys,
                                                                     uint32_t* __restrict__ idx) {
  const int64_t i = (int64_t)blockIdx.x * kSeqBlock + threadIdx.x;
  if (i >= n) return;
  keys[i] = (uint64_t)rows[2 * i] ^ 0x8000000000000000ull;
  idx[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(kSeqBlock) absent_inst_gather_kernel(const int64_t* __restrict__ rows,
                                                                       const uint32_t* __restrict__ idx, int64_t n,
                                                                       int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kSeqBlock + threadIdx.x;
  if (i >= n) return;
  out[2 * i] = rows[2 * (int64_t)idx[i]];
  out[2 * i + 1] = rows[2 * (int64_t)idx[i] + 1];
}

// keyed: cr[k] = the creation ordinal of output k's instance (compaction order), ckey[k] the same as a sort key
__global__ void __launch_bounds__(kSeqBlock) absent_create_kernel(AbsArgs a, const uint32_t* __restrict__ xv, int64_t m,
                                                                  const int64_t* __restrict__ tab, int64_t ni,
                                                                  int64_t* __restrict__ cr, uint64_t* __restrict__ ckey,
                                                                  uint32_t* __restrict__ idx) {
  const int64_t k = (int64_t)blockIdx.x * kSeqBlock + threadIdx.x;
  if (k >= m) return;
  const int64_t x = xv[k];
  int64_t key;
  if (x < a.nc) {
    key = a.carry[x * a.cw];
  } else {
    const int64_t i = x - a.nc;
    key = a.ka_wide ? ((const int64_t*)a.ka)[i] : (int64_t)((const int32_t*)a.ka)[i];
  }
  const int64_t at = abs_inst_find(tab, ni, key);
  const int64_t c = at >= 0 ? tab[2 * at + 1] : 0;
  cr[k] = c;
  ckey[k] = (uint64_t)c;
  idx[k] = (uint32_t)k;
}

__global__ void __launch_bounds__(kSeqBlock) absent_pkeys_kernel(const uint32_t* __restrict__ pv,
                                                                 const uint32_t* __restrict__ idx, int64_t m,
                                                                 uint32_t* __restrict__ keys) {
  const int64_t k = (int64_t)blockIdx.x * kSeqBlock + threadIdx.x;
  if (k < m) keys[k] = pv[idx[k]];
}

// e1 of an output: a batch row, or a carried row's canonical attribute words
struct AbsProjLoader {
  const NfaStream* st;
  int64_t r;
  const int64_t* c;
  __device__ StackVal var(const Instr& in) const {
    if (in.op == OP_COL) return col_value(st, in.a, r);
    if (c) {
      const int t = st->types[in.c];
      StackVal v = uncanon((uint64_t)c[3 + in.c], t);
      if (t == T_STRING) v.null = v.i < 0;
      return v;
    }
    return col_value(st, in.c, r);
  }
};

struct AbsProj {
  const uint32_t* pv;       // p of each compacted output
  const uint32_t* xv;       // its place in res
  const uint32_t* order;    // the outputs' final order over the compacted ones, or nullptr: as compacted
  const int64_t* cr;        // creation ordinals (compaction order), or nullptr: unpartitioned (-1)
  int64_t m, nc;
  const int64_t* carry;
  int cw;
  const NfaStream* st;
  const int64_t* ts;
  const int64_t* ordinals;
  int64_t obase, wait;
  const char* blob;         // the query's device plan
  uint32_t* e1;             // out: e1's ordinal relative to obase (a carried one negative as int32)
  DVal* vals;               // out: m x nsel
  int64_t* ts_out;          // out: d
  int64_t* pos;             // out: the trigger position p
  int64_t* create;          // out
};

__global__ void __launch_bounds__(kSeqBlock) absent_project_kernel(AbsProj a) {
  const int64_t k = (int64_t)blockIdx.x * kSeqBlock + threadIdx.x;
  if (k >= a.m) return;
  const DQuery* q = (const DQuery*)a.blob;
  const Instr* code = (const Instr*)(a.blob + q->off_code);
  const DVal* consts = (const DVal*)(a.blob + q->off_const);
  const int32_t* sel = (const int32_t*)(a.blob + q->off_sel);
  const int64_t s = a.order ? (int64_t)a.order[k] : k;
  const int64_t x = a.xv[s];
  AbsProjLoader ld{a.st, 0, nullptr};
  int64_t t1;
  if (x < a.nc) {
    ld.c = a.carry + x * a.cw;
    t1 = ld.c[2];
    a.e1[k] = (uint32_t)(int32_t)(ld.c[1] - a.obase);
  } else {
    ld.r = x - a.nc;
    t1 = a.ts[ld.r];
    a.e1[k] = a.ordinals ? (uint32_t)(a.ordinals[ld.r] - a.obase) : (uint32_t)ld.r;
  }
  DVal* o = a.vals + k * q->nsel;
  for (int c = 0; c < q->nsel; ++c) {
    const StackVal v = eval_prog(code + sel[3 * c], sel[3 * c + 1], consts, ld);
    DVal d;
    if (sel[3 * c + 2] == T_FLOAT || sel[3 * c + 2] == T_DOUBLE) d.d = v.d;
    else d.i = v.i;
    d.null = v.null;
    d.pad = 0;
    o[c] = d;
  }
  a.ts_out[k] = t1 + a.wait;
  a.pos[k] = (int64_t)a.pv[s];
  a.create[k] = a.cr ? a.cr[s] : -1;
}

}  // namespace
}  // namespace sm
