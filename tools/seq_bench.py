"""Benchmark of the adjacent-pair closed form of `every e1=S[c1], e2=S[c2] within T` (fast_path 6, kernels/seqpath.hip)
on the config-4 data shape (bench.gen_stock: splitmix64 stream, f64 price, inputs resident on the device), keyed and
unkeyed, against the only device route such a query had before: sm_app_process_device_events (the general NFA kernel,
query-specialised JIT on). One JSON line per (route, form): ms per step (min / median / max over --steps timed steps
after --warmup), events/s of the median step, outputs, and for the closed form the per-kernel times of option
fast_timing. Each step starts from a fresh runtime state (option reset), as bench.py's steps do.

    python tools/seq_bench.py --route closed            # the new kernels
    python tools/seq_bench.py --route nfa               # the NFA route (run it with the parent commit's library too)
    python tools/seq_bench.py --precompile              # CPU only: the NFA route's JIT kernels into the code cache
    python tools/seq_bench.py --query three ...         # the three-state query `every e1, e2, e3 within T` (three rising
                                                        # ticks) on the same stream: fast_path 7, the adjacent-run kernels
    python tools/seq_bench.py --query streams ...       # `every e1=A[c1], e2=B[c2] within T` over two streams of the same
                                                        # rows (a row's stream: a hash bit of its number), and with
                                                        # --query streams3 the three-state `A, B, A`: fast_path 8. Both
                                                        # routes are sm_app_process_device_events here: --route closed
                                                        # with this library, --route nfa with the parent commit's
                                                        # (SM_LIB_VARIANT), which runs the NFA kernel
    python tools/seq_bench.py --query pattern_streams ...   # the pattern `every e1=A[c1] -> e2=B[c2] within T` on the same
                                                        # two-way stream index: fast_path 9 (kernels/mpat_dev.h); routes as
                                                        # for --query streams
    python tools/seq_bench.py --query pattern_chain ...     # the three-state pattern `every e1=A[c1] -> e2=B[c2] within T
                                                        # -> e3=A[c3] within T` on the same two-way stream index:
                                                        # fast_path 10 (kernels/mpatk_dev.h); routes as for --query streams
    python tools/seq_bench.py --query absent ...            # the timeout `every e1=A[c1] -> not B[c2] for 1 sec` on the same
                                                        # two-way stream index, @app:playback: fast_path 11
                                                        # (kernels/absent_dev.h); routes as for --query streams
    python tools/seq_bench.py --query absent_and ...        # the logical absent `every e1=A[c1] -> not B[c2] and e3=C[c3]
                                                        # within 1 sec` on a three-way stream index, @app:playback:
                                                        # fast_path 12 (kernels/mpat_nand_dev.h); routes as for --query
                                                        # streams
    python tools/seq_bench.py --query logic_and ...         # the logical pair `every e1=A[c1] -> e2=B[c2] and e3=C[c3]
                                                        # within 1 sec` on the same three-way stream index, and with
                                                        # --query logic_or its `or` form: fast_path 13
                                                        # (kernels/mpat_logic_dev.h); routes as for --query streams
    python tools/seq_bench.py --query pattern_count ...     # the count pattern `every e1=A[c1] -> e2=B[c2]<2:4> ->
                                                        # e3=C[c3] within 1 sec` on the same three-way stream index:
                                                        # fast_path 14 (kernels/mpat_count_dev.h); routes as for --query
                                                        # streams

Step time is a host clock around work that ends in a device synchronise; a run without a GPU fails."""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

SCHEMA = "define stream StockStream (symbol int, price double, volume long, timestamp long); "
QUERY = ("@info(name='q') from every e1=StockStream[price>20], e2=StockStream[price>e1.price] within 1 sec "
         "select e1.timestamp as i, e2.timestamp as j insert into OutputStream;")
QUERY3 = ("@info(name='q') from every e1=StockStream[price>20], e2=StockStream[price>e1.price], "
          "e3=StockStream[price>e2.price] within 1 sec "
          "select e1.timestamp as i, e2.timestamp as j, e3.timestamp as l insert into OutputStream;")
ATTRS = "(symbol int, price double, volume long, timestamp long); "
SCHEMA_AB = "define stream A " + ATTRS + "define stream B " + ATTRS
QUERY_AB = ("@info(name='q') from every e1=A[price>20], e2=B[price>e1.price] within 1 sec "
            "select e1.timestamp as i, e2.timestamp as j insert into OutputStream;")
QUERY_PAT_AB = ("@info(name='q') from every e1=A[price>20] -> e2=B[price>e1.price] within 1 sec "
                "select e1.timestamp as i, e2.timestamp as j insert into OutputStream;")
QUERY_ABA = ("@info(name='q') from every e1=A[price>20], e2=B[price>e1.price], e3=A[price>e2.price] within 1 sec "
             "select e1.timestamp as i, e2.timestamp as j, e3.timestamp as l insert into OutputStream;")
QUERY_PAT_ABA = ("@info(name='q') from every e1=A[price>20] -> e2=B[price>e1.price] within 1 sec -> "
                 "e3=A[price>e2.price] within 1 sec "
                 "select e1.timestamp as i, e2.timestamp as j, e3.timestamp as l insert into OutputStream;")
QUERY_ABSENT = ("@info(name='q') from every e1=A[price>20] -> not B[price>70] for 1 sec "
                "select e1.timestamp as i insert into OutputStream;")


SCHEMA_ABC = SCHEMA_AB + "define stream C " + ATTRS
QUERY_ABSENT_AND = ("@info(name='q') from every e1=A[price>20] -> not B[price>70] and e3=C[price>e1.price] within 1 sec "
                    "select e1.timestamp as i, e3.timestamp as j insert into OutputStream;")


QUERY_LOGIC = ("@info(name='q') from every e1=A[price>20] -> e2=B[price>e1.price] {op} e3=C[price<e1.price] within 1 sec "
               "select e1.timestamp as i, e2.timestamp as j, e3.timestamp as l insert into OutputStream;")


QUERY_COUNT = ("@info(name='q') from every e1=A[price>20] -> e2=B[price>e1.price]<2:4> -> e3=C[price<e1.price] within 1 sec "
               "select e1.timestamp as i, e2[0].timestamp as j, e2[last].timestamp as k, e3.timestamp as l "
               "insert into OutputStream;")


STREAM_QUERIES = ("streams", "streams3", "pattern_streams", "pattern_chain", "absent", "absent_and", "logic_and",
                  "logic_or", "pattern_count")
THREE_WAY = ("absent_and", "logic_and", "logic_or", "pattern_count")  # queries on the three-way stream index


def apps(query, cancel_above="70"):
    """cancel_above: c2's constant of --query absent_and (a large one cancels nothing)."""
    if query == "absent_and":
        head = "@app:playback " + SCHEMA_ABC
        q = QUERY_ABSENT_AND.replace("price>70", "price>" + cancel_above)
        return {"keyed": head + "partition with (symbol of A, symbol of B, symbol of C) begin " + q + " end;",
                "unkeyed": head + q}
    if query in ("logic_and", "logic_or"):
        q = QUERY_LOGIC.format(op=query[6:])
        return {"keyed": SCHEMA_ABC + "partition with (symbol of A, symbol of B, symbol of C) begin " + q + " end;",
                "unkeyed": SCHEMA_ABC + q}
    if query == "pattern_count":
        return {"keyed": SCHEMA_ABC + "partition with (symbol of A, symbol of B, symbol of C) begin " + QUERY_COUNT + " end;",
                "unkeyed": SCHEMA_ABC + QUERY_COUNT}
    if query in STREAM_QUERIES:
        q = {"streams": QUERY_AB, "streams3": QUERY_ABA, "pattern_streams": QUERY_PAT_AB,
             "pattern_chain": QUERY_PAT_ABA, "absent": QUERY_ABSENT}[query]
        head = ("@app:playback " if query == "absent" else "") + SCHEMA_AB  # timers run on the events' clock
        return {"keyed": head + "partition with (symbol of A, symbol of B) begin " + q + " end;", "unkeyed": head + q}
    q = QUERY3 if query == "three" else QUERY
    return {"keyed": SCHEMA + "partition with (symbol of StockStream) begin " + q + " end;", "unkeyed": SCHEMA + q}


APPS = apps("pair")
LABELS = ["seq_facts", "seq_sort", "seq_link", "seq_keep", "seq_count", "seq_scan", "seq_emit", "seq_carry"]
LABELS += ["seqk_" + l[4:] for l in LABELS]
LABELS += ["event_index", "mseq_facts", "mseq_pack", "mseq_sort", "mseq_link", "mseq_keep", "mseq_count", "mseq_scan",
           "mseq_emit", "mseq_carry"]
LABELS += ["mpat_facts", "mpat_pack", "mpat_sort", "mpat_link", "mpat_count", "mpat_scan", "mpat_emit", "mpat_order",
           "mpat_carry"]
LABELS += ["mpatk_facts", "mpatk_pack", "mpatk_sort", "mpatk_link", "mpatk_count", "mpatk_scan", "mpatk_cand", "mpatk_emit",
           "mpatk_order", "mpatk_parts", "mpatk_carry"]
LABELS += ["absent_facts", "absent_pack", "absent_sort", "absent_next", "absent_state", "absent_count", "absent_scan",
           "absent_inst", "absent_emit", "absent_order", "absent_project", "absent_carry"]
LABELS += ["pnand_facts", "pnand_pack", "pnand_sort", "pnand_next", "pnand_link", "pnand_count", "pnand_scan", "pnand_emit",
           "pnand_order", "pnand_carry", "pnand_clock"]
LABELS += ["plog_facts", "plog_pack", "plog_sort", "plog_link", "plog_count", "plog_scan", "plog_cand", "plog_emit",
           "plog_order", "plog_parts", "plog_carry"]
LABELS += ["pcnt_facts", "pcnt_pack", "pcnt_sort", "pcnt_link", "pcnt_count", "pcnt_scan", "pcnt_cand", "pcnt_emit",
           "pcnt_order", "pcnt_parts", "pcnt_carry"]


def precompile(query, cancel_above):
    """The NFA route's query-specialised kernels take minutes through hiprtc: compiled here, on a host without a GPU,
    into siddhi_amd/jit_cache (the compact lane-event form a 4-attribute stream takes), one process per plan."""
    import subprocess
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--query", query, "--cancel-above", cancel_above,
                               "--precompile-one", form],
                              env=dict(os.environ, SM_NFA_JIT_COMPACT="1")) for form in apps(query, cancel_above)]
    sys.exit(max(p.wait() for p in procs))


def precompile_one(form, query, cancel_above):
    import torch  # noqa: F401  (first, as in every run: the library then compiles with the hiprtc torch bundles)
    from siddhi_amd import _lib
    log = ctypes.create_string_buffer(8192)
    size = ctypes.c_size_t()
    t = time.time()
    rc = _lib.lib().sm_nfa_jit_compile(apps(query, cancel_above)[form].encode(), 0, log, 8192, ctypes.byref(size))
    print(f"{form}: rc {rc}, {size.value} bytes, {time.time() - t:.0f} s {log.value.decode()[:200]}", flush=True)
    sys.exit(rc)


def stats(ms):
    s = sorted(ms)
    return {"min": s[0], "median": s[len(s) // 2], "max": s[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=float, default=1e8)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--ts-div", type=int, default=10_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--route", choices=["closed", "nfa"], default="closed")
    ap.add_argument("--forms", default="keyed,unkeyed")
    ap.add_argument("--query", choices=["pair", "three", "streams", "streams3", "pattern_streams", "pattern_chain", "absent",
                                        "absent_and", "logic_and", "logic_or", "pattern_count"],
                    default="pair")
    ap.add_argument("--cancel-above", default="70",
                    help="--query absent_and: the constant of c2 `not B[price>X]`; the outputs a large X adds are the "
                         "partials that the default cancels")
    ap.add_argument("--heap-words", type=int, default=0,
                    help="--route nfa: the NFA kernel's per-key partial-match arena (option heap_words); a count pattern's "
                         "partials hold several events each and outgrow the default at 1e8 keyed events")
    ap.add_argument("--precompile", action="store_true")
    ap.add_argument("--precompile-one")
    a = ap.parse_args()
    if a.cancel_above != "70" and a.query != "absent_and":
        ap.error("--cancel-above belongs to --query absent_and")
    if a.precompile_one:
        precompile_one(a.precompile_one, a.query, a.cancel_above)
    if a.precompile:
        precompile(a.query, a.cancel_above)
    if a.steps < 10:
        print("note: fewer than 10 timed steps", file=sys.stderr)

    import torch
    from siddhi_amd import _lib
    from siddhi_amd.testing import ProductApp
    if not torch.cuda.is_available():
        sys.exit("seq_bench needs a GPU")
    dev = torch.device("cuda", 0)
    n = int(a.events)
    sym, price, _, _, ts = bench.gen_stock(0, n, a.keys, a.ts_div, dev, bench.seed_for(4))
    ordinals = torch.arange(n, dtype=torch.int64, device=dev)  # the timestamp attribute = the event's ordinal
    streams = a.query in STREAM_QUERIES
    sidx = torch.zeros(n, dtype=torch.int32, device=dev) if a.route == "nfa" or streams else None
    if streams:  # a deterministic two-way stream index from the row number
        x = ordinals * (0x9E3779B97F4A7C15 - (1 << 64))  # (wraps: a multiply-xorshift hash, one bit of it)
        x = (x ^ (x >> 29)) * (0xBF58476D1CE4E5B9 - (1 << 64))
        sidx = ((x >> 43) & 1).to(torch.int32)
        if a.query in THREE_WAY:  # three ways: two more bits of the hash, folded to 0 .. 2
            sidx = (((x >> 41) & 0xFFFF) % 3).to(torch.int32)
    hs = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    build_id = _lib.lib().sm_build_id().decode()
    torch.cuda.synchronize()
    for form in a.forms.split(","):
        opts = {"nfa_jit": 1} if a.route == "nfa" else {}
        if a.route == "nfa" and a.heap_words:
            opts["heap_words"] = a.heap_words
        app = ProductApp(apps(a.query, a.cancel_above)[form], **opts)
        app.set_collect(False)
        cols = [sym, price, price, ordinals]  # volume is not read: aliased

        def step():
            if a.route == "nfa" or streams:
                app.set_option("reset", 1)
                app.process_device_events(sidx, ts, cols, ordinals=ordinals, hip_stream=hs)
            else:
                app.set_option("reset", 0)
                app.process_device_batch("StockStream", ts, cols, hip_stream=hs)
            return int(app.get_stat("output_events:q"))

        for _ in range(a.warmup):
            step()
        if a.route == "closed":
            app.set_option("fast_timing", 1)
        ms, kern, m = [], {}, 0
        for _ in range(a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = step()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            print(f"{a.route} {form} step {len(ms)}: {ms[-1]:.3f} ms", file=sys.stderr, flush=True)
            if a.route == "closed":
                for lab in LABELS:
                    if app.get_stat("kernel_calls:" + lab):
                        kern.setdefault(lab, []).append(app.get_stat("kernel_ms:" + lab))
        st = stats(ms)
        line = {"route": a.route, "query": a.query, "form": form, "events": n, "keys": a.keys, "ts_div": a.ts_div, "steps": a.steps,
                "warmup": a.warmup, "ms": st, "events_per_s": n / (st["median"] * 1e-3), "outputs": m,
                "build_id": build_id}
        if a.route == "closed":
            line["fast_path"] = int(app.get_stat("fast_path:q"))
            if a.query == "pattern_count":  # the partials a step leaves open, and those below m hits (no window ends them)
                line["carry_partials"] = int(app.get_stat("carry_partials:q"))
                line["carry_unclocked"] = int(app.get_stat("carry_unclocked:q"))
            line["kernel_ms_median"] = {k: sorted(v)[len(v) // 2] for k, v in kern.items()}
        else:
            line["nfa_kernel"] = int(app.get_stat("nfa_kernel:q"))
        print(json.dumps(line), flush=True)
        app.close()


if __name__ == "__main__":
    main()
