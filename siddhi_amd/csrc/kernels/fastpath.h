// Host entry of the closed-form `every e1 -> e2 within T` kernels (fastpath.hip: general form;
// fastpath3.hip: keyed bandwidth form for single-column keys and a single compared attribute).
#pragma once
#include <functional>

#include "nfa.h"
#include "primitives.h"
#include "stream_ops.h"

namespace sm {

struct FastArgs {
  int64_t n;
  const int64_t* ts;          // device, event timestamps
  const NfaStream* st;        // device stream descriptor (columns)
  const KeyProg* key;         // device key program or nullptr (non-partitioned)
  const Instr* code;          // device bytecode of the query
  const DVal* consts;
  int c1_off, c1_len, c2_off, c2_len;
  int64_t within;             // -1 = none
  const int64_t* ordinals;    // device or nullptr
  int64_t ordinal_base;
};

// Host-side facts about the plan and the batch used to pick the v2 kernels.
struct FastHostInfo {
  const void* const* cols;    // host array of device column pointers
  const int32_t* types;       // column types
  int key_col = -1;           // partition key is this column (-1: expression or none)
  int key_type = 0;
  int vattr = -1;             // the only attribute c2 reads (-1: not eligible)
  int vtype = 0;
  const Instr* c2_host = nullptr;  // host copy of the c2 program (specialisation of the walk's compare)
  int c2_len = 0;
  const Instr* c1_host = nullptr;  // host copy of the c1 program (c1 on the compared attribute: no bit mask)
  int c1_len = 0;
  int nattr = 0;              // attributes of the stream (carried partial rows)
  const int32_t* dense_keys = nullptr;  // device: the key column as dense ids (remap_keys), read instead of the column
  int64_t remap_span = 0;  // > 0: a key span above it returns FAST_KEY_SPAN (the caller gives the keys dense ids)
};

// Device facts cached across batches by the v2 kernels.
struct FastState {
  int cus = 0;              // compute units of the device
  int sort_wgs_per_cu = 0;  // resident down-sweep workgroups per CU (persistent-chunk grid)
  int walk_wgs_per_cu = 0;  // resident walk workgroups per CU
  // pipeline of the last batch: 2 = sort / walk, 3 = bucket stack; seqpath.hip: 6 = adjacent pairs, 7 = adjacent runs,
  // 8 = adjacent runs over several streams, 9 = the pattern over two streams, 10 = the k-state pattern over several
  // streams, 11 = the timeout `every A -> not B for W`, 12 = the logical absent `every A -> not B and C within T`,
  // 13 = the logical pair `every A -> B and|or C within T`, 14 = the count pattern `every A -> B<m:n> -> C within T`
  int last_path = 0;
};

struct FastTimings {          // optional HIP events: [0] start, [1] keyed sort done, [2] walk done, [3] end
  hipEvent_t ev[4];
  // per-launch marks of the v2 pipeline: mk[0] before the first kernel, mk[k] after the k-th, label[k] its kernel
  static constexpr int kMaxMarks = 32;
  hipEvent_t mk[kMaxMarks];
  const char* label[kMaxMarks];
  int nmk = 0;
  void mark(const char* l, hipStream_t s) {
    if (nmk < kMaxMarks) {
      label[nmk] = l;
      (void)hipEventRecord(mk[nmk++], s);
    }
  }
};

// Open partials carried across device batches of one query: the pending list of the e2 pre-processor, which the
// reference keeps between InputHandler.send calls (StreamPreStateProcessor.java:208-221 addState, :268-271
// updateState, :274-327 processAndReturn). One row per partial = its e1 event:
//   [key, global ordinal, event time, attribute 0 .. nattr-1 (canonical 64-bit: integers as int64, FLOAT /
//   DOUBLE as double bits)]
// sorted by (key, ordinal). As in the reference, a partial stays pending until an event of its own key either
// matches it or finds it expired (isExpired :102-121); keys that see no event keep their partials.
struct FastCarry {
  int64_t* rows = nullptr;  // device, n rows of `width` words
  int64_t n = 0, cap = 0;   // rows / allocated rows
  int width = 0;            // 3 + nattr
  bool active = false;      // a device batch has run for this query: ts_last is valid
  int64_t ts_last = 0;      // event time of the last event of the last batch
  // fast_pat_k and fast_pat_logic only: the open partials [key, bound events s, global ordinals o1 .. os padded to
  // k - 1], every key's in order of o1 (fast_pat_logic: [key, state, o1, o2], fastpath.h fast_pat_logic; fast_pat_count:
  // [key, hits | in-e3 << 8, tlast, p, o1, n hit ordinals], fastpath.h fast_pat_count); `rows` are then the events they
  // hold, each once, with the stream as the last word
  int64_t* parts = nullptr;  // device, pn rows of pw words
  int64_t pn = 0, pcap = 0;
  int pw = 0;               // k + 1 (fast_pat_count: n + 5)
  // second buffer of `rows` (spare_words words): the carry-out that writes each row once, in its place, writes there
  // while it reads the old rows, and the two change places (stack.hip build_carry_runs)
  int64_t* spare = nullptr;
  int64_t spare_words = 0;
  void reserve(int64_t rows_needed, int w);
  void reserve_parts(int64_t rows_needed, int w, hipStream_t s);  // the old rows are not kept
  void release();
  void reset() {
    n = 0;
    pn = 0;
    active = false;
    ts_last = 0;
  }
};

int64_t fast_every_within(const FastArgs& a, uint32_t* pairs_out, int64_t pairs_cap, Scratch& sc, hipStream_t s,
                          FastTimings* tm = nullptr);

// Results of fast_every_within_v2 besides M >= 0.
enum : int64_t { FAST_OUTSIDE = -1, FAST_NON_MONOTONE = -2, FAST_KEY_SPAN = -3 };

// FAST_OUTSIDE: outside the v2 envelope (caller falls back to fast_every_within); FAST_NON_MONOTONE: event time
// decreases inside the batch or against the carried state (the closed form does not apply: the caller takes the
// general NFA path); FAST_KEY_SPAN: the partition keys (carried ones included) span more than 2^30 values, or more
// than hi.remap_span when that is set (the caller may give them dense ids and run the batch again; nothing was
// changed). Match pairs are relative to a.ordinal_base; an e1 carried from an earlier batch has a
// negative (int32) relative ordinal. The carry is read and replaced.
int64_t fast_every_within_v2(const FastArgs& a, const FastHostInfo& hi, FastState& fs, FastCarry& carry,
                             uint32_t* pairs_out, int64_t pairs_cap, Scratch& sc, hipStream_t s,
                             FastTimings* tm = nullptr, int stack_mode = 0);

// The adjacent-pair closed form of `every e1=S[c1], e2=S[c2] [within T]` (seqpath.hip, seq_dev.h): a sequence's
// partial is completed or dropped by the next event of its partition instance, so the outputs are adjacent pairs, at
// most one per e2, in order of e2. Same results, pairs and carry conventions as fast_every_within_v2 (the carry holds at
// most one row per key: the key's last event if it passes c1; hi.vattr is not used: c1 and c2 are evaluated by the
// bytecode interpreter on the columns). FAST_NON_MONOTONE is returned only when a.within >= 0; FAST_KEY_SPAN only for a
// query's first batch with hi.remap_span set. Sets fs.last_path = 6.
int64_t fast_seq_adjacent(const FastArgs& a, const FastHostInfo& hi, FastState& fs, FastCarry& carry,
                          uint32_t* pairs_out, int64_t pairs_cap, Scratch& sc, hipStream_t s, FastTimings* tm = nullptr);

// The k-state sibling `every e1=S[c1], ..., ek=S[ck]`, 3 <= k <= 8 (seqpath.hip, seq_dev.h: the adjacent-run closed
// form). a.c1_* / a.c2_* / a.within are not read: the plan's programs and withins come in `p`.
struct SeqKPlan {
  int k = 0;
  int off[8] = {0}, len[8] = {0};  // condition program of element m (state context)
  int64_t within[8] = {-1, -1, -1, -1, -1, -1, -1, -1};  // element m against element m - 1; -1 = none
};

// Outputs are k-tuples (k uint32 words each, relative to a.ordinal_base; members carried from earlier batches are
// negative as int32), at most one per event, in order of the last event. The carry holds each instance's last
// min(k - 1, events so far) events, sorted by (key, ordinal). Results as fast_seq_adjacent; FAST_NON_MONOTONE only when
// some element has a within. tuples_cap counts tuples. Sets fs.last_path = 7.
int64_t fast_seq_k(const FastArgs& a, const SeqKPlan& p, const FastHostInfo& hi, FastState& fs, FastCarry& carry,
                   uint32_t* tuples_out, int64_t tuples_cap, Scratch& sc, hipStream_t s, FastTimings* tm = nullptr);

// The same form over several streams of one schema, 2 <= k <= 8, on an interleaved batch (seqpath.hip, mseq_dev.h):
// `sid` is the stream of every row (device); rows of streams outside p.read and heartbeat rows (-1) are ignored.
struct MSeqKeys {                  // the rows a query reads and their partition keys (fast_seq_ms and fast_pat_ms)
  uint64_t read = 0;               // bit s: the query reads app stream s
  bool keyed = false;
  const void* kcol[64] = {nullptr};  // keyed: the device key column of read stream s (INT, or LONG when bit s of wide)
  uint64_t wide = 0;
  int64_t remap_span = 0;          // as FastHostInfo::remap_span
};

struct MSeqPlan : MSeqKeys {
  int k = 0;
  int stream[8] = {0};             // app stream of element m
  int off[8] = {0}, len[8] = {0};  // condition program of element m (state context)
  int64_t within[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
};

// a.st: the device descriptor of a read stream (all share the columns); a.key / a.c1_* / a.c2_* / a.within are not
// read. Tuples, carry and results as fast_seq_k, except that a carried row has 4 + nattr words, the last one its
// stream. Sets fs.last_path = 8.
int64_t fast_seq_ms(const FastArgs& a, const int32_t* sid, const MSeqPlan& p, int nattr, FastState& fs,
                    FastCarry& carry, uint32_t* tuples_out, int64_t tuples_cap, Scratch& sc, hipStream_t s,
                    FastTimings* tm = nullptr);

// The pattern `every e1=A[c1] -> e2=B[c2] within T` over two streams of one schema on an interleaved batch
// (seqpath.hip, mpat_dev.h has the rule and the kernels).
struct MPatPlan : MSeqKeys {
  int stream[2] = {0, 0};          // app stream of e1 and of e2
  int off[2] = {0, 0}, len[2] = {0, 0};  // c1 and c2 (state context)
  int64_t within = -1;
};

// a.st, `sid`, key_remap and FAST_KEY_SPAN as fast_seq_ms; pairs and their conventions as fast_every_within_v2: (e1, e2)
// uint32 relative to a.ordinal_base, a carried e1 negative as int32, in order of (e2, e1); at most n + carry.n of them
// (pairs_cap). The carry holds the open partials' e1 rows [key, ordinal, ts, attributes] sorted by (key, ordinal): every
// unmatched e1 that the batch's last read event does not find expired. FAST_NON_MONOTONE: p.within >= 0 and the event
// time of the read rows decreases inside the batch or against carry.ts_last. Both error results are returned before the
// carry or pairs_out is touched. Sets fs.last_path = 9.
int64_t fast_pat_ms(const FastArgs& a, const int32_t* sid, const MPatPlan& p, int nattr, FastState& fs, FastCarry& carry,
                    uint32_t* pairs_out, int64_t pairs_cap, Scratch& sc, hipStream_t s, FastTimings* tm = nullptr);

// Its k-state sibling `every e1=S1[c1] -> e2=S2[c2] within T2 -> ... -> ek=Sk[ck] within Tk`, 3 <= k <= 8 (seqpath.hip,
// mpatk_dev.h has the rule and the kernels). within[m] >= 0 for every m >= 1, against the event bound before.
struct MPatKPlan : MSeqKeys {
  int k = 0;
  int stream[8] = {0};
  int off[8] = {0}, len[8] = {0};
  int64_t within[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
};

// a.st, `sid`, key_remap and FAST_KEY_SPAN as fast_seq_ms. Outputs are k-tuples as fast_seq_k's (members carried from
// earlier batches negative as int32), in lexicographic order of (ek, ..., e1), at most n + carry.pn of them (tuples_cap).
// The carry holds the open partials (FastCarry::parts) and the events they have bound, each once, as fast_seq_ms's rows
// of 4 + nattr words. FAST_NON_MONOTONE: the event time of the read rows decreases inside the batch or against
// carry.ts_last. Every error result is returned before the carry or tuples_out is touched. Sets fs.last_path = 10.
int64_t fast_pat_k(const FastArgs& a, const int32_t* sid, const MPatKPlan& p, int nattr, FastState& fs, FastCarry& carry,
                   uint32_t* tuples_out, int64_t tuples_cap, Scratch& sc, hipStream_t s, FastTimings* tm = nullptr);

// The timeout `every e1=A[c1] -> not B[c2] for W` over one or two streams of one schema on an interleaved batch
// (seqpath.hip, absent_dev.h has the rule and the kernels).
struct AbsentPlan : MSeqKeys {
  int stream[2] = {0, 0};          // app stream of A and of B (may be equal)
  int off[2] = {0, 0}, len[2] = {0, 0};  // c1 (over e1) and c2 (over the B event alone)
  int64_t wait = 0;                // W >= 1
};

// Every partition instance the query has created, with the global ordinal of the row that created it: [key, ordinal]
// rows sorted by key (device). It lives with the carry and orders the outputs of instances that are due at one position.
struct AbsentInst {
  int64_t* rows = nullptr;
  int64_t n = 0, cap = 0;
  void reserve(int64_t rows_needed);  // the old rows are not kept
  void release();
};

// The m outputs of a batch, in the reference's order (device): e1's ordinal relative to a.ordinal_base (a carried one
// negative as int32), the select values (m x nsel), the timestamp ts[e1] + W, the trigger position p in the batch and
// the instance's creation ordinal (-1: unpartitioned).
struct AbsentOut {
  uint32_t* e1;
  DVal* vals;
  int64_t* ts;
  int64_t* pos;
  int64_t* create;
};

// a.st, `sid`, key_remap and FAST_KEY_SPAN as fast_seq_ms. clk: the playback clock at every row of the batch
// (build_event_index's ev_clock). blob_dev: the query's device plan (its select programs). `out` is called once, with
// the number of outputs, when nothing has been changed yet, and returns where they go. The carry holds the open
// partials' e1 rows as fast_pat_ms's, `inst` the instances. FAST_NON_MONOTONE: a row of a read stream lies below the
// clock. Every error result is returned before the carry, `inst` or an output is touched. Sets fs.last_path = 11.
int64_t fast_absent(const FastArgs& a, const int32_t* sid, const int64_t* clk, const AbsentPlan& p, int nattr,
                    const char* blob_dev, FastState& fs, FastCarry& carry, AbsentInst& inst,
                    const std::function<AbsentOut(int64_t)>& out, Scratch& sc, hipStream_t s, FastTimings* tm = nullptr);

// The logical absent `every e1=A[c1] -> not B[c2] and e3=C[c3] within T` over up to three streams of one schema on an
// interleaved batch (seqpath.hip, mpat_nand_dev.h has the rule and the kernels).
struct PNandPlan : MSeqKeys {
  int stream[3] = {0, 0, 0};       // app streams of A, B and C (B is not C)
  int off[3] = {0, 0, 0}, len[3] = {0, 0, 0};  // c1 (over e1), c2 (over the B event alone), c3 (over e1 and e3)
  int64_t within = -1;             // T >= 0
};

// a.st, `sid`, key_remap and FAST_KEY_SPAN as fast_seq_ms; (e1, e3) pairs, their order (e3, e1), pairs_cap, the carry (the
// open partials' e1 rows: no e3 yet, no cancelling row yet, not expired at the batch's last read row) and both error
// results as fast_pat_ms. Sets fs.last_path = 12.
int64_t fast_pat_nand(const FastArgs& a, const int32_t* sid, const PNandPlan& p, int nattr, FastState& fs,
                      FastCarry& carry, uint32_t* pairs_out, int64_t pairs_cap, Scratch& sc, hipStream_t s,
                      FastTimings* tm = nullptr);

// The logical pair `every e1=A[c1] -> e2=B[c2] and|or e3=C[c3] within T` over up to three streams of one schema on an
// interleaved batch (seqpath.hip, mpat_logic_dev.h has the rule and the kernels).
struct PLogPlan : MSeqKeys {
  bool land = true;                // and / or
  int stream[3] = {0, 0, 0};       // app streams of A, B and C (B is not C; and: A is neither)
  int off[3] = {0, 0, 0}, len[3] = {0, 0, 0};  // c1 (over e1), c2 (over e1 and e2), c3 (over e1 and e3)
  int64_t within = -1;             // T >= 0, against e1
};

// a.st, `sid`, key_remap and FAST_KEY_SPAN as fast_seq_ms. Outputs are (e1, e2, e3) triples as fast_pat_k's (members
// carried from earlier batches negative as int32; a member `or` left unbound is the word 0x80000000, which no carried
// member is), in order of (completing member, e1), at most n + carry.pn of them (tuples_cap). The carry is fast_pat_k's:
// the open partials (FastCarry::parts, rows [key, s, o1, o2]: s = 1 e1 alone, 2 with e2, 3 with e3) and the events they
// hold. Both error results as fast_pat_k. Sets fs.last_path = 13.
int64_t fast_pat_logic(const FastArgs& a, const int32_t* sid, const PLogPlan& p, int nattr, FastState& fs,
                       FastCarry& carry, uint32_t* tuples_out, int64_t tuples_cap, Scratch& sc, hipStream_t s,
                       FastTimings* tm = nullptr);

// The count pattern `every e1=A[c1] -> e2=B[c2]<m:n> -> e3=C[c3] within T` over three different streams of one schema
// on an interleaved batch (seqpath.hip, mpat_count_dev.h has the rule and the kernels).
struct PCntPlan : MSeqKeys {
  int cmin = 0, cmax = 1;          // m, n: 0 <= m <= n, 1 <= n <= 6
  int stream[3] = {0, 0, 0};       // app streams of A, B and C, pairwise different
  int off[3] = {0, 0, 0}, len[3] = {0, 0, 0};  // c1 (over e1), c2 (over e1 and the current e2), c3 (over e1 and e3)
  int64_t within = -1;             // T >= 0, against the hit bound last (e1 if none)
};

// a.st, `sid`, key_remap and FAST_KEY_SPAN as fast_seq_ms. Outputs are tuples of n + 2 words (e1, e2[0] .. e2[n-1], e3) as
// fast_pat_k's (members carried from earlier batches negative as int32; a hit slot that is not bound is the word
// 0x80000000, which no carried member is), in order of (e3, the m-th hit or e1 if m = 0, e1), at most n + carry.pn of
// them (tuples_cap). The carry is fast_pat_k's two tables: the open partials (FastCarry::parts, rows
// [key, hits | in-e3 << 8, tlast, p, o1, n hit ordinals], n + 5 words) and the events they hold. No window bounds the open
// partials (one with fewer than m hits has no clock): they are bounded by the data, and by the scratch, which is checked
// once they are counted and before anything changes (FAST_OUTSIDE), and by pcnt_carry_cap, likewise. Both error results
// as fast_pat_k. Sets fs.last_path = 14.
// The cap on the open partials a batch of n rows may leave: every batch's scratch is its per-row terms plus the constant
// kBatchScratchSlack (runtime.cpp batch_scratch), and the carried state has to fit what the batch's own rows do not
// claim: one partial per row, plus as many as the slack holds at the bytes a partial costs the carry-out (its row of
// n + 5 words, and n + 1 held events at build_carry's 8 cw + 44 bytes each). It also bounds what the link pass spends on
// carried partials that never complete (each is scanned again from the head of its key's run in every batch).
constexpr size_t kBatchScratchSlack = (size_t)64 << 20;
inline int64_t pcnt_carry_cap(int64_t n, int cmax, int cw) {
  return n + (int64_t)(kBatchScratchSlack / ((size_t)(cmax + 1) * (size_t)(8 * cw + 44) + 8 * (size_t)(cmax + 5)));
}
int64_t fast_pat_count(const FastArgs& a, const int32_t* sid, const PCntPlan& p, int nattr, FastState& fs,
                       FastCarry& carry, uint32_t* tuples_out, int64_t tuples_cap, Scratch& sc, hipStream_t s,
                       FastTimings* tm = nullptr);

// The hand-over of the instances to the NFA kernel: word `word` of the per-key state of slots 0 .. n - 1 (ks: word-major,
// one column of state_slots per word) becomes create[slot], the instance's creation ordinal.
void absent_set_creation(int64_t* ks, int64_t state_slots, int word, const int64_t* create, int64_t n, hipStream_t s);

// keys[i] = the partition key of row i (the key column of its own stream, as int64), 0 for a row that is not read: the
// one key column remap_keys takes when an interleaved batch's keys become dense ids
void mseq_gather_keys(int64_t n, const int32_t* sid, const MSeqKeys& p, int64_t* keys, hipStream_t s);

// ---- internal: the bucket-stack pipeline (stack.hip), entered by fast_every_within_v2 after key pass 0 ----

// Facts about a batch once key pass 0 has scattered its 16-byte records {key - kmin | c1 << 31, ordinal - base,
// value code, ts - ts0} into kBins buckets by the low key digit (fastpath3.hip).
struct StackPlan {
  const void* rec;          // uint4 records, bucket order
  const uint32_t* dbase;    // bucket starts
  int64_t n;
  int64_t omax;             // largest relative ordinal of the batch
  int H;                    // in-bucket keys (key span >> kRB, rounded up)
  int64_t kmin;
  int op;                   // CMP_* of `e2.x OP e1.x`
  bool fp;                  // compared as floating point
  bool exact_codes;         // value codes decide every comparison
  int vtype, vattr, vmode;
  int64_t vmin;
  const void* vcol;
  int64_t within;
  int64_t ts0, ts_last;
  int32_t o0;               // relative ordinal of the batch's first event: carried partials lie before it
  // The pipeline's four status words, taken and zeroed by the caller before key pass 0 when that pass checks the
  // time order (keys-only prep): pass 0 sets word 3 if event time decreases somewhere in the batch, and the pipeline
  // reads it with its first read-back, before the stack kernel. nullptr: the pipeline takes its own.
  uint32_t* status = nullptr;
};

// M >= 0, or -1 when the batch must take the sort / walk pipeline instead (a key's open partials overflowed the
// stack, a slice's match log filled, a NaN compared value): neither pairs_out nor the carry was touched then.
// FAST_NON_MONOTONE when p.status is given and key pass 0 found event time decreasing: nothing was touched either.
int64_t stack_pipeline(const StackPlan& p, const FastArgs& a, const FastHostInfo& hi, FastState& fs, FastCarry& carry,
                       uint32_t* pairs_out, int64_t pairs_cap, Scratch& sc, hipStream_t s, FastTimings* tm);

// Carry-out candidates (4 words each: key, global ordinal, event time, source = batch row >= 0 or -(old carry
// row) - 1) → the new carry rows, sorted by (key, ordinal). `old` is read before carry.rows is replaced. row_stream
// (the stream of every batch row, fast_seq_ms only): the rows are one word wider, the last word the row's stream.
void build_carry(const int64_t* cand, int64_t ncand, const NfaStream* st, int nattr, FastCarry& carry, Scratch& sc,
                 hipStream_t s, int key_bits = 64, int64_t kmin = 0, bool key_runs_ordered = false,
                 const int32_t* row_stream = nullptr);

// On-device projection of m closed-form outputs (pairs = the device tuples of the last batch): the query's select
// programs (blob_dev = its device plan) → out[k * nsel + a], and e2's event time → ts_out[k] (may be null). An e1
// carried from an earlier batch reads its row of prev_carry (the carry as it was before the batch: nc rows of cw
// words). The batch's columns / ts / ordinals must still be resident. rows = true: `pairs` are a filter query's
// kept rows (m u32, ordinal - base), each output reading its own row.
void pair_project(const uint32_t* pairs, int64_t m, const NfaStream* st_dev, const int64_t* ord, int64_t n,
                  int64_t base, const int64_t* ts, const int64_t* prev_carry, int64_t nc, int cw, const char* blob_dev,
                  DVal* out, int64_t* ts_out, Scratch& sc, hipStream_t s, bool rows = false,
                  int64_t* words = nullptr, uint8_t* nulls = nullptr,  // words / nulls: compact form (nsel <= 8)
                  const uint32_t* carry_keys = nullptr, const uint32_t* carry_idx = nullptr, bool sync = true,
                  int arity = 2,  // arity k > 2: `pairs` are k-tuples (the adjacent-run closed form), slot s = word s
                  const int* logic_slot = nullptr,   // the logical pair's triples: word w holds slot logic_slot[w], a
                                                     // word 0x80000000 is an absent member (its attributes are null),
                                                     // and ts_out is the event time of the later of e2 / e3
                  bool count = false);  // the count pattern's tuples (e1, e2[0] .. e2[arity-3], e3): slot 1 is read at
                                        // an index or at CURRENT (the last bound hit); a word 0x80000000 is a hit slot
                                        // that is not bound (its attributes are null)
// The carried partials' e1 ordinals sorted for pair_project (carry_keys / carry_idx, nc each, in sc): a caller
// projecting one batch's outputs in several launches sorts them once (round 5: device_outputs' segments)
void pair_project_carry_order(const int64_t* prev_carry, int64_t nc, int cw, int64_t base, Scratch& sc, hipStream_t s,
                              const uint32_t** carry_keys, const uint32_t** carry_idx);

}  // namespace sm
