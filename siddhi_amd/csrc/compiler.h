// Host compiler: SiddhiQL AST → device plan (plan.h). Lowering mirrors
// core/util/parser/StateInputStreamParser.java:78-432 (state tables, within lists, every/next edges,
// receivers), SelectorParser.java:140-200 (projections) and ExpressionParser.java:231-1371 (bytecode).
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "plan.h"
#include "siddhiql/ast.h"

namespace sm {

struct Dict {  // string dictionary: device columns carry int32 ids
  std::unordered_map<std::string, int32_t> ids;
  std::vector<std::string> strs;
  int32_t intern(const std::string& s) {
    auto it = ids.find(s);
    if (it != ids.end()) return it->second;
    int32_t id = (int32_t)strs.size();
    strs.push_back(s);
    ids.emplace(s, id);
    return id;
  }
};

struct CompiledQuery {
  std::string name;
  std::string insert_into;
  int order = 0;          // position in app.order
  int partition = -1;     // partition index, -1 = none
  DQuery hdr{};
  std::vector<char> blob;               // header + tables, uploaded once
  std::vector<int32_t> sel_types;       // output attribute types
  std::vector<std::string> sel_names;
  std::vector<int> streams;             // app stream indices the query consumes
  bool has_absent = false;
  // fast path: every e1=S[c1] -> e2=S[c2] within T (closed form)
  bool fast_every_within = false;
  int64_t fast_within = -1;             // -1 = no within
  int fast_c1_off = 0, fast_c1_len = 0; // program over e1's stream columns (stream context)
  int fast_c2_off = 0, fast_c2_len = 0; // program over (e1 slot 0, e2 slot 1) state context
  // fast path: every e1=S[c1], e2=S[c2] [within T] (sequence: adjacent pairs of a partition instance, seqpath.hip);
  // shares fast_within / fast_c1_* / fast_c2_*
  bool fast_seq_adjacent = false;
  // fast path: every e1=S[c1], e2=S[c2], ..., ek=S[ck] with 3 <= k <= 8 (sequence: runs of k adjacent events of a
  // partition instance, seqpath.hip). fast_seq_k = k (0: not this form); per element m (0-based) its condition
  // program (state context, slots 0..m) and its `within` against the previous element's event (-1 = none; element 0
  // has none). The plan carries k hidden ordinal refs (slot m, index 0) after the visible ones.
  int fast_seq_k = 0;
  int fast_k_off[8] = {0}, fast_k_len[8] = {0};
  int64_t fast_k_within[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
  // fast path: every e1=S1[c1], e2=S2[c2], ..., ek=Sk[ck] with 2 <= k <= 8 over at least two streams of one schema
  // (sequence: runs of k adjacent events of a partition instance among the events of the streams the query reads,
  // seqpath.hip). fast_seq_ms = k (0: not this form); per element m its app stream index, its condition program
  // (state context, slots 0..m) and its `within` against the previous element's event (-1 = none; element 0 has
  // none). fast_ms_keycol[s] is the INT / LONG key attribute of app stream s when the query is partitioned (-1: the
  // query does not read s). The plan carries k hidden ordinal refs (slot m, index 0) after the visible ones. Such a
  // plan is not fast_seq_k / fast_seq_adjacent: it runs through sm_app_process_device_events only.
  int fast_seq_ms = 0;
  int fast_ms_stream[8] = {0};
  int fast_ms_off[8] = {0}, fast_ms_len[8] = {0};
  int64_t fast_ms_within[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
  std::vector<int> fast_ms_keycol;
  // fast path: every e1=A[c1] -> e2=B[c2] within T over two streams of one schema (pattern: every A event passing c1
  // waits for the first later B event of its partition instance that passes c2, inside T; kernels/mpat_dev.h). A mark of
  // its own: such a query runs through the interleaved entry point only. fast_pat_stream = the app streams of e1 and
  // e2, fast_pat_off / len their condition programs (state context), fast_pat_within = T (always >= 0),
  // fast_pat_keycol[s] as fast_ms_keycol. The plan carries the hidden (e1, e2) ordinal refs after the visible ones.
  bool fast_pat_ms = false;
  int fast_pat_stream[2] = {0, 0};
  int fast_pat_off[2] = {0, 0}, fast_pat_len[2] = {0, 0};
  int64_t fast_pat_within = -1;
  std::vector<int> fast_pat_keycol;
  // fast path: every e1=S1[c1] -> e2=S2[c2] within T2 -> ... -> ek=Sk[ck] within Tk with 3 <= k <= 8 over at least two
  // streams of one schema, S1 none of S2 .. S(k-1) (pattern: every S1 event passing c1 binds, state by state, the first
  // later Sm event of its partition instance that passes cm, each inside Tm of the event bound before it;
  // kernels/mpatk_dev.h). fast_pat_k = k (0: not this form), a mark of its own: such a query runs through the
  // interleaved entry point only. Per element m its app stream, its condition program (state context, slots 0..m) and
  // its within against the previous element's event (>= 0 for m >= 1; element 0 has none). fast_patk_keycol[s] as
  // fast_ms_keycol. The plan carries k hidden ordinal refs (slot m, index 0) after the visible ones.
  int fast_pat_k = 0;
  int fast_patk_stream[8] = {0};
  int fast_patk_off[8] = {0}, fast_patk_len[8] = {0};
  int64_t fast_patk_within[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
  std::vector<int> fast_patk_keycol;
  // fast path: every e1=A[c1] -> not B[c2] for W, B a stream of A's schema or A itself, c2 reading the B event and
  // constants only, the select reading e1 only, no within, no having, @app:playback (pattern: every A event passing c1
  // is emitted with timestamp ts + W once the playback clock reaches it, unless a B event of its partition instance
  // passing c2 arrives before; kernels/absent_dev.h). A mark of its own: such a query runs through the interleaved
  // entry point only. fast_abs_stream = the app streams of A and B, fast_abs_off / len = c1 and c2 (state context, c2
  // over slot 1 alone), fast_abs_wait = W >= 1 ms, fast_abs_keycol[s] as fast_ms_keycol. The plan carries one hidden
  // ordinal ref, e1's, after the visible ones.
  bool fast_absent = false;
  int fast_abs_stream[2] = {0, 0};
  int fast_abs_off[2] = {0, 0}, fast_abs_len[2] = {0, 0};
  int64_t fast_abs_wait = 0;
  std::vector<int> fast_abs_keycol;
  // fast path: every e1=A[c1] -> not B[c2] and e3=C[c3] within T (either operand order) over streams of one schema, B
  // not C, c2 reading the B event and constants only, c3 reading e1 and e3, the select reading e1 and e3, no having,
  // @app:playback (pattern: every A event passing c1 waits for the first later C event of its partition instance that
  // passes c3; the pair is emitted iff that event lies inside T and no B event of the instance passing c2 came in
  // between; kernels/mpat_nand_dev.h). A mark of its own: such a query runs through the interleaved entry point only.
  // fast_nand_stream = the app streams of A, B and C; fast_nand_off / len = c1, c2 (over B's slot alone) and c3 (state
  // context: slot 0 and e3's slot fast_nand_slot3, which is 1 or 2 with the operand order); fast_nand_within = T (always
  // >= 0); fast_nand_keycol[s] as fast_ms_keycol. The plan carries the hidden (e1, e3) ordinal refs after the visible
  // ones; match_arity() stays 2.
  bool fast_pat_nand = false;
  int fast_nand_stream[3] = {0, 0, 0};
  int fast_nand_off[3] = {0, 0, 0}, fast_nand_len[3] = {0, 0, 0};
  int fast_nand_slot3 = 0;
  int64_t fast_nand_within = -1;
  std::vector<int> fast_nand_keycol;
  // fast path: every e1=A[c1] -> e2=B[c2] and e3=C[c3] within T, or the same with `or`, over streams of one schema, B
  // not C, c2 reading e1 and e2, c3 reading e1 and e3, no having (pattern: every A event passing c1 takes the first later
  // B event of its partition instance passing c2 and the first later C event passing c3, independently; `and` emits at
  // the later of the two, `or` at the earlier with the other side null, iff that event lies inside T of e1;
  // kernels/mpat_logic_dev.h). fast_pat_logic = 1 (and: A is neither B nor C) or 2 (or); a mark of its own: such a query
  // runs through the interleaved entry point only. Index m = 0, 1, 2 is e1, e2, e3 in the order of the query text:
  // fast_logic_stream their app streams, fast_logic_off / len their condition programs (state context: slot 0 and the
  // member's own slot fast_logic_slot[m]; the lowering numbers the second operand's slot first), fast_logic_within = T
  // (always >= 0), fast_logic_keycol[s] as fast_ms_keycol. The plan carries the hidden (e1, e2, e3) ordinal refs after the
  // visible ones; a member that `or` left unbound has no ordinal there.
  int fast_pat_logic = 0;
  int fast_logic_stream[3] = {0, 0, 0};
  int fast_logic_off[3] = {0, 0, 0}, fast_logic_len[3] = {0, 0, 0};
  int fast_logic_slot[3] = {0, 0, 0};
  int64_t fast_logic_within = -1;
  std::vector<int> fast_logic_keycol;
  // fast path: every e1=A[c1] -> e2=B[c2]<m:n> -> e3=C[c3] within T over three different streams of one schema, 0 <= m
  // <= n, 1 <= n <= 6, c2 reading e1 and the current e2, c3 reading e1 and e3, the select reading e1, e2[k] (k < n),
  // e2[last] and e3, no having (pattern: every A event passing c1 binds the first n later B events of its partition
  // instance passing c2; from the m-th on, the first later C event ends it: beyond T of the hit bound last (of e1 if
  // none) the partial is dead, otherwise it emits if the event passes c3; kernels/mpat_count_dev.h). fast_pat_count = n
  // (0: not this form), a mark of its own, which none of the other marks accompanies: such a query runs through the
  // interleaved entry point only. fast_count_min = m; index 0, 1, 2 is e1, e2, e3: fast_count_stream their app streams (slot = index),
  // fast_count_off / len their condition programs (state context), fast_count_within = T (always >= 0),
  // fast_count_keycol[s] as fast_ms_keycol. The plan carries the hidden ordinal refs (e1, e2[0] .. e2[n-1], e3) after the
  // visible ones; a hit slot that is not bound has no ordinal there.
  int fast_pat_count = 0;
  int fast_count_min = 0;
  int fast_count_stream[3] = {0, 0, 0};
  int fast_count_off[3] = {0, 0, 0}, fast_count_len[3] = {0, 0, 0};
  int64_t fast_count_within = -1;
  std::vector<int> fast_count_keycol;
  // uint32 words per device match tuple: k, 3 for the logical pair, n + 2 for the count pattern, 2 for every other state
  // query, 1 for a filter (its kept row) and for the timeout (its e1)
  int match_arity() const {
    return hdr.kind == 0 || fast_absent ? 1
           : fast_seq_k ? fast_seq_k : fast_seq_ms ? fast_seq_ms : fast_pat_k ? fast_pat_k : fast_pat_logic ? 3
           : fast_pat_count ? fast_pat_count + 2 : 2;
  }
  // the closed forms that carry an event table and a partial table of k + 1 words per row (FastCarry::parts): k, or 0
  // (the count pattern: rows [key, hits | in-e3 << 8, tlast, p, o1, n hit ordinals], n + 5 words)
  int carry_parts_k() const { return fast_pat_k ? fast_pat_k : fast_pat_logic ? 3 : fast_pat_count ? fast_pat_count + 4 : 0; }
};

struct CompiledPartition {
  std::vector<int> streams;                    // partitioned stream indices
  std::vector<std::vector<Instr>> key_code;    // per partitioned stream: key expression program
  std::vector<std::vector<DVal>> key_consts;
  std::vector<int32_t> key_type;               // result type per stream
};

// Compile one query. `app_streams` gives stream index by id. Throws sql::*Error.
CompiledQuery compile_query(const sql::App& app, const sql::Query& q, int order, int partition, Dict& dict);
CompiledPartition compile_partition(const sql::App& app, const sql::Partition& p, Dict& dict);

int stream_index(const sql::App& app, const std::string& id);

}  // namespace sm
