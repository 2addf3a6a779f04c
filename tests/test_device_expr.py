"""Every device route of the bytecode evaluator (kernels/expr.h eval_prog / do_compare / do_math and its restatements)
against the numpy model of the reference's executors (tests/expr_model.py) and the CPU oracle, exactly: ints as ints,
floats and doubles by their bits, NaN as NaN. The values come from pools on the promotion, rounding, wrap-around,
zero-divisor and null edges; the shapes are the smallest at which each kernel can still go wrong. The CPU side of the
same cases (model == oracle == host build) is tests/test_expr_model.py."""
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest

import expr_model as M
from expr_model import BOOL, DOUBLE, FLOAT, INT, LONG, NUMERIC, STRING
from oracle_lib import OracleApp, lib as olib
from test_expr_model import (ATTRS, FMA_VALUES, NESTED, NESTED_NUMERIC, NUM_ATTRS, PAIRS, SCHEMA, TYPES, _assert_same,
                             _deep, dump_kept, dump_values, eval_rows, filter_app, model_kept, model_values, rows12,
                             run_rows, select_app, send_value)

pytestmark = pytest.mark.gpu

NP = {INT: np.int32, LONG: np.int64, FLOAT: np.float32, DOUBLE: np.float64}
SCHEMA8 = "define stream S (" + ", ".join(f"{a} {M.QL_TYPE[t]}" for a, t in NUM_ATTRS) + "); "
N_FILTER = 4096 + 64 + 1  # one full 4096-row tile, one full wave, one row: a tile boundary and a ragged last wave


# ---- device batches over the eight numeric attributes (no nulls: a device batch's columns carry none)

@functools.lru_cache(maxsize=None)
def batch8(n):
    rows = rows12(n, nulls=False)
    cols = [np.array([row[a] for row in rows], dtype=NP[t]) for a, t in NUM_ATTRS]
    return rows, cols


def oracle_batch(text, cols):
    a = OracleApp(text)
    a.start()
    ptrs = (ctypes.c_void_p * len(cols))(*[c.ctypes.data for c in cols])
    err = ctypes.create_string_buffer(512)
    ts = np.arange(len(cols[0]), dtype=np.int64)
    assert olib().cr_send_columns(a.h, a.stream_index("S"), len(ts), ts.ctypes.data, ptrs, err, 512) == 0, err.value
    out = a.outputs()
    a.close()
    return out


def device_batch(text, cols, collect=False):
    """One device batch of the whole stream (event time = row number); the app is returned open."""
    import torch
    from siddhi_amd.testing import ProductApp
    app = ProductApp(text)
    dev = torch.device("cuda", 0)
    app._keep = ([torch.from_numpy(c).to(dev) for c in cols], torch.arange(len(cols[0]), dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    app.process_device_batch("S", app._keep[1], app._keep[0], collect=collect)
    return app


def check_filters(conds, n, path):
    rows, cols = batch8(n)
    text = filter_app(conds, SCHEMA8)
    labels = [M.text(e) for e in conds]
    exp = model_kept(conds, rows)
    _assert_same(dump_kept(oracle_batch(text, cols), conds), exp, "oracle", labels)
    app = device_batch(text, cols)
    got = [app.device_rows_host(f"c{k}").astype(np.int64).tolist() for k in range(len(conds))]
    paths = [int(app.get_stat(f"fast_path:c{k}")) for k in range(len(conds))]
    app.close()
    assert paths == [path] * len(conds), [x for x, p in zip(labels, paths) if p != path]
    _assert_same(got, exp, f"device (fast_path {path})", labels)
    return exp


# constants of each type for `col cmp const`: one equal to a pool value, one between two, one extreme
LEAF_CONSTS = {INT: ["7", "5", "-2147483648"], LONG: ["16777217L", "5L", "9223372036854775807L"],
               FLOAT: ["0.1f", "16777217.0f", "3.4028235e38f"], DOUBLE: ["0.1", "16777216.5", "-1.7976931348623157e308"]}
COL_OF = {INT: "i", LONG: "l", FLOAT: "f", DOUBLE: "d"}


@pytest.mark.parametrize("ct", NUMERIC)
def test_typed_filter_leaves(ct):
    """filter.hip leaf_items (fast_path 4): col cmp const and its mirror, 4 constant types x 3 constants x 6 operators
    for one column type per case."""
    conds = []
    for kt in NUMERIC:
        for k in LEAF_CONSTS[kt]:
            for op in M.CMP_OPS:
                conds.append(M.parse(f"{COL_OF[ct]} {op} {k}", TYPES))
                conds.append(M.parse(f"{k} {op} {COL_OF[ct]}", TYPES))
    assert len(conds) == 144
    exp = check_filters(conds, N_FILTER, 4)
    # the extreme constant keeps all rows or none by design, and no value equals the in-between one; every other leaf
    # (2 constants x 6 operators less the in-between ==, != : 10 per constant type, and its mirror) must discriminate
    assert sum(1 for kept in exp if 0 < len(kept) < N_FILTER) >= 4 * 10 * 2


# of the nested numeric conditions, the ones that are one `col cmp const` leaf take the typed form, the others the interpreter
NESTED_LEAVES = [x for x in NESTED_NUMERIC if (lambda e: e[0] == "cmp" and {e[2][0], e[3][0]} == {"var", "const"})(M.parse(x, TYPES))]


def test_typed_filter_conjunctions():
    conds = [M.parse(x, TYPES) for x in NESTED_LEAVES] + [M.parse(x, TYPES) for x in (
        "i > 5 and d <= 0.1f", "16777217L != f and l2 < 2147483648L", "f2 >= 0.1 and i2 != 16777216.0f and d2 > -1",
        "(l >= 16777217.0f and f < 16777217) and d != 0.1f", "(i < 7L and 0.1f <= d) and (l != 5.0 and f2 == 2.5f)",
        "i2 >= -7 and (l2 > -2147483649L and (d2 < 1.7976931348623157e308 and f > -1.0f))")]
    exp = check_filters(conds, N_FILTER, 4)
    assert all(len(kept) < N_FILTER for kept in exp)
    assert [M.text(e) for e, kept in zip(conds, exp) if not kept] == ["(f == 0.1)"]  # (double)0.1f is not 0.1


def test_filter_interpreter():
    """filter.hip filter_count_prog_kernel (fast_path 3): column against column for every ordered pair and operator,
    and the nested numeric conditions."""
    conds = [M.c(op, M.var(a, ta), M.var(b, tb)) for op in M.CMP_OPS for (a, ta), (b, tb) in PAIRS]
    conds += [M.parse(x, TYPES) for x in NESTED_NUMERIC if x not in NESTED_LEAVES]
    assert len(NESTED_LEAVES) == 5 and len(conds) == 336 + len(NESTED_NUMERIC) - 5 and len(NESTED_NUMERIC) >= 15
    check_filters(conds, N_FILTER, 3)


N_PROJECT = 449  # two 256-thread blocks, the second ragged


@pytest.mark.parametrize("per_query", [8, 14], ids=["words8", "dval14"])
def test_projection_of_filter_rows(per_query):
    """select A op B for the five math ops over the 56 pairs on a filter query's kept rows: the JSON dump of a collected
    device batch (device_outputs: the compact word form for 8 values per query, the DVal form for more) and
    sm_app_device_project (DVal form), values and null bits."""
    rows, cols = batch8(N_PROJECT)
    exprs = [M.m(op, M.var(a, ta), M.var(b, tb)) for op in M.MATH_OPS for (a, ta), (b, tb) in PAIRS]
    cond = M.parse("i + l2 != 7L", TYPES)
    text, groups = select_app(exprs, per_query, SCHEMA8, cond=cond)
    kept = [r for r, v in enumerate(eval_rows(cond, rows)) if v is True]
    assert 256 < len(kept) < N_PROJECT
    exp = [[x for x in g if x[0] in set(kept)] for g in model_values(groups, rows)]
    assert any(v is None for g in exp for _, row in g for v in row) and any(v == "NaN" for g in exp for _, row in g for v in row)
    labels = [" | ".join(M.text(e) for e in g) for g in groups]
    _assert_same(dump_values(oracle_batch(text, cols), groups), exp, "oracle", labels)
    app = device_batch(text, cols, collect=True)
    got = dump_values(app.outputs(), groups)
    proj = []
    for k, g in enumerate(groups):
        assert app.get_stat(f"fast_path:v{k}") == 3
        vals, nulls, ts = app.device_project(f"v{k}")
        types = [M.type_of(e) for e in g]
        proj.append([(t, tuple(M.from_word(w, z, ty) for w, z, ty in zip(vr, nr, types)))
                     for t, vr, nr in zip(ts.cpu().tolist(), vals.cpu().tolist(), nulls.cpu().tolist())])
    app.close()
    _assert_same(got, exp, "device_outputs", labels)
    _assert_same(proj, exp, "device_project", labels)


# ---- host-staged single-stream route (stream_ops.hip): nulls, strings and bools through send

def _having_over_outputs(src, exprs):
    """A having condition written over output attributes c<j>: its tree, and the tree with each c<j> replaced by the
    select expression (the value the model evaluates)."""
    types = {f"c{j}": M.type_of(e) for j, e in enumerate(exprs)}
    tree = M.parse(src, types)

    def subst(e):
        if e[0] == "var":
            return exprs[int(e[1][1:])]
        return tuple(subst(x) if isinstance(x, tuple) else x for x in e)
    return tree, subst(tree)


@pytest.mark.parametrize("flush_every", [0, 9], ids=["one_flush", "flush_9"])
def test_host_staged_stream_ops(flush_every):
    from siddhi_amd.testing import ProductApp
    rows = rows12(300)
    exprs = [M.parse(x, TYPES) for x in NESTED + FMA_VALUES + ["s", "s2", "b", "f", "i % i2", "l / l2", "f % d2", "d / f2"]]
    exprs.append(_deep(8))
    cond = M.parse("s != s2 and not (i2 is null)", TYPES)
    having, having_model = _having_over_outputs("c6 and not c13", exprs)
    sel = ", ".join(f"{M.text(e)} as c{j}" for j, e in enumerate(exprs))
    text = SCHEMA + (f"@info(name='v0') from S[{M.text(cond)}] select {sel} insert into V0; "
                     f"@info(name='v1') from S select {sel} having {M.text(having)} insert into V1;")
    groups = [exprs, exprs]
    keep = [eval_rows(cond, rows), eval_rows(having_model, rows)]
    exp = [[x for x in g if keep[k][x[0]] is True] for k, g in enumerate(model_values(groups, rows))]
    assert all(30 < len(e) < 290 for e in exp)
    labels = ["filter + select", "select + having"]
    _assert_same(dump_values(run_rows(OracleApp, text, rows), groups), exp, "oracle", labels)
    _assert_same(dump_values(run_rows(ProductApp, text, rows, flush_every=flush_every), groups), exp, "stream_ops", labels)


# ---- NFA interpreter and query-specialised kernel: e1 read back from a stored partial, e2 the current event

KATTRS = [("k", INT)] + ATTRS
KSCHEMA = " ".join("define stream %s (%s);" % (s, ", ".join(f"{a} {M.QL_TYPE[t]}" for a, t in KATTRS)) for s in ("S", "S2"))
E_TYPES = {f"{e}.{a}": t for e in ("e1", "e2") for a, t in KATTRS}
BASE = {INT: "i", LONG: "l", FLOAT: "f", DOUBLE: "d"}
N_KEYS = 320


def _e(src):
    return M.parse(src, E_TYPES)


NFA_QUERIES = ["q0", "q1", "q2", "q3"]


@functools.lru_cache(maxsize=None)
def nfa_exprs():
    """The select lists of the four pattern queries (a stream, the output stream included, holds at most 48 attributes):
    the five math ops over the 16 (e1, e2) type pairs, the six compares over the 12 mixed ones, then nulls, strings,
    bools, the nested conditions, the depth-8 sum and a * b + c."""
    math = [M.m(op, M.var(f"e1.{BASE[ta]}", ta), M.var(f"e2.{BASE[tb]}", tb)) for op in M.MATH_OPS for ta in NUMERIC
            for tb in NUMERIC]
    cmps = [M.c(op, M.var(f"e1.{BASE[ta]}", ta), M.var(f"e2.{BASE[tb]}", tb)) for op in M.CMP_OPS for ta in NUMERIC
            for tb in NUMERIC if ta != tb]
    deep = M.right_sum([M.var(f"e{1 + j % 2}.{a}", TYPES[a]) for j, a in enumerate(["i", "i2", "l", "l2", "f", "f2", "d", "d2"])])
    rest = [_e(x) for x in (
        "e1.d * e2.d + e1.d2", "e1.f * e2.f + e1.f2", "e1.s", "e2.s", "e1.b", "e2.b", "e1.f", "e2.f", "e1.i", "e1.l", "e1.d",
        "e1.s == e2.s", "e1.s != 'a'", "e1.s is null", "e1.b == e2.b", "e1.b and e2.b", "e1.b or not e2.b", "e2.b != true",
        "e2.d > 0.1f", "e1.f == 0.1", "e1.f == 0.1f", "e1.l == 16777217.0f", "e1.i / 2 * 2 == e1.i",
        "(e1.i + e2.l) * e1.f > e2.d % 7", "not (e1.d / e2.d2 > 1)", "(e1.d / e2.d2) is null", "e1.d / e2.d2 != 1",
        "e1.l - e2.l2 >= e1.i * e2.i2", "e1.f % e2.f2 <= e1.l / e2.i", "e1.f + e2.i == e1.d + e2.i", "2147483647 < e1.i + 1",
        "e2.l * 3037000500L > 0", "(e1.i % e2.i2) is null")] + [deep]
    every = rest + math + cmps  # 34 + 80 + 72
    per = -(-len(every) // len(NFA_QUERIES))
    assert per <= 48
    return {name: every[k * per:(k + 1) * per] for k, name in enumerate(NFA_QUERIES)}


def nfa_text(name):
    exprs = nfa_exprs()[name]
    sel = ", ".join(f"{M.text(e)} as c{j}" for j, e in enumerate(exprs))
    cond = _e("not (e2.f > e1.d and e2.b)")
    # having over the outputs: a value that is null for some keys and a condition that is false for some
    nullable = [j for j, e in enumerate(exprs) if e[0] == "math" and e[1] in "/%"]
    bools = [j for j, e in enumerate(exprs) if M.type_of(e) == BOOL and e[0] == "cmp" and e[1] in ("<", ">=")]
    having = " or ".join([f"not (c{j} is null)" for j in nullable[:1]] + [f"c{j}" for j in bools[:1]])
    if name == NFA_QUERIES[0]:
        having += " or c12"  # e1.s != 'a': the a * b + c keys pass
    hv, hv_model = _having_over_outputs(having, exprs)
    text = (KSCHEMA + " partition with (k of S, k of S2) begin @info(name='q') from e1=S -> e2=S2[" + M.text(cond) + "] select "
            + sel + " having " + M.text(hv) + " insert into Out; end;")
    return text, exprs, cond, hv_model


def jit_plans():
    """The query plans the nfa_jit = 1 cases run (tools/jit_precompile.py compiles them at build time)."""
    return {f"device_expr_{name}": nfa_text(name)[0] for name in nfa_exprs()}


@functools.lru_cache(maxsize=None)
def nfa_events():
    """Per key j one S event (e1) and then one S2 event (e2). e1 takes row j; e2 takes row j with the suffixed and the
    unsuffixed attributes exchanged, so (e1.x, e2.y) runs over every pair of the two pools. The last keys hold the
    a * b + c values whose product rounds: (1 + 2^-30)(1 - 2^-30) + -1 and its float sibling with 2^-13."""
    rows = rows12(N_KEYS - 2)
    e1 = [dict(r) for r in rows]
    e2 = [{a: r[a[:-1] if a.endswith("2") else a + "2"] for a in r} for r in rows]
    one = {a: (1 if t in NUMERIC else "a" if t == STRING else True) for a, t in ATTRS}
    for sign in (1, -1):
        e1.append(dict(one, d=1 + sign * 2.0**-30, d2=-1.0, f=np.float32(1 + sign * 2.0**-13), f2=-1.0, s="b"))
        e2.append(dict(one, d=1 - sign * 2.0**-30, f=np.float32(1 - sign * 2.0**-13), b=False))
    joined = [dict({f"e1.{a}": v for a, v in x.items()}, **{f"e2.{a}": v for a, v in y.items()}) for x, y in zip(e1, e2)]
    return e1, e2, joined


def run_nfa(factory, text, **opts):
    e1, e2, _ = nfa_events()
    types = [t for _, t in KATTRS]
    a = factory(text, **opts)
    a.start()
    for j, (x, y) in enumerate(zip(e1, e2)):
        a.send("S", 2 * j, [j] + [send_value(x[n], t) for n, t in ATTRS], types)
        a.send("S2", 2 * j + 1, [j] + [send_value(y[n], t) for n, t in ATTRS], types)
    a.flush()
    out = a.outputs()
    kernel = a.get_stat("nfa_kernel:q") if opts else None
    a.close()
    return out, kernel


def test_fused_multiply_add_would_show():
    """The rows that separate two roundings from one: the model (Java) gives 0.0 where a fused multiply-add gives
    -2^-60 (double) and -2^-26 (float)."""
    _, _, joined = nfa_events()
    row = joined[-2]
    assert M.value(_e("e1.d * e2.d + e1.d2"), row) == 0.0 and M.value(_e("e1.f * e2.f + e1.f2"), row) == 0.0
    exact = lambda a, b, c: Fraction(float(row[a])) * Fraction(float(row[b])) + Fraction(float(row[c]))  # noqa: E731
    assert exact("e1.d", "e2.d", "e1.d2") == Fraction(-1, 2**60) and exact("e1.f", "e2.f", "e1.f2") == Fraction(-1, 2**26)


@pytest.mark.parametrize("name", NFA_QUERIES)
@pytest.mark.parametrize("jit", [0, 1], ids=["interpreter", "jit"])
def test_nfa_select_and_having(jit, name):
    import torch  # noqa: F401  before the library: it then loads torch's hiprtc, which the code-object cache is keyed by
    from siddhi_amd.testing import ProductApp
    text, exprs, cond, hv_model = nfa_text(name)
    _, _, joined = nfa_events()
    keep = [a is True and b is True for a, b in zip(eval_rows(cond, joined), eval_rows(hv_model, joined))]
    exp = [[(2 * j + 1, row) for (j, row) in model_values([exprs], joined)[0] if keep[j]]]
    assert 40 < len(exp[0]) < N_KEYS - 20
    if name == NFA_QUERIES[0]:  # the list with a * b + c: both keys whose product rounds are among the outputs
        assert M.text(exprs[0]) == "((e1.d * e2.d) + e1.d2)" and keep[-2] and keep[-1]
        assert [row[:2] for _, row in exp[0][-2:]] == [(0, 0), (0, 0)]  # +0.0, double and float
    label = [f"e1=S -> e2=S2, {name}"]

    def values(out):
        return [[(o[0], M.canon_row(o[1], [M.type_of(e) for e in exprs])) for o in out["streams"].get("Out", [])]]
    ora, _ = run_nfa(OracleApp, text)
    _assert_same(values(ora), exp, "oracle", label)
    got, kernel = run_nfa(ProductApp, text, nfa_jit=jit)
    assert kernel == (1 if jit else 2)
    _assert_same(values(got), exp, "query-specialised kernel" if jit else "NFA interpreter", label)


def test_operand_stack_limit_on_the_device():
    """The depth-8 sum runs on the device (select list above); depth 9 is the compiler's refusal, not a crash."""
    from siddhi_amd.testing import EngineError, ProductApp
    with pytest.raises(EngineError, match="operand stack"):
        ProductApp(select_app([_deep(9)])[0])


# ---- closed forms: attributes of a carried e1 (FLOAT, INT, LONG, BOOL) read back through the carry rows

ATTRS6 = [("symbol", INT), ("price", DOUBLE), ("qty", FLOAT), ("n", INT), ("v", LONG), ("flag", BOOL)]
COLS6 = ", ".join(f"{a} {M.QL_TYPE[t]}" for a, t in ATTRS6)
SELECT6 = [f"e{m}.{a}" for m in (1, 2) for a, _ in ATTRS6] + ["e1.qty * e2.v", "e2.n % e1.n"]
C1S = ["qty > 0.1f", "n / 2 * 2 == n", "v % 3 != 0 and qty <= 2.5", "flag == true"]


@functools.lru_cache(maxsize=None)
def stock6(n, K, div=10):
    """Deterministic columns: keys and prices that match often, the other attributes walking their pools (NaN, the
    infinities and -0.0 among the floats, the wrap-around values among the integers)."""
    r = np.arange(n, dtype=np.int64)
    P = M.POOLS
    cols = [((r * 7919 + (r >> 3)) % K).astype(np.int32), ((r * 2654435761) % 1009) / 10.0,
            np.array(P[FLOAT], np.float32)[(r * 5 + r // 17) % len(P[FLOAT])],
            np.array(P[INT], np.int32)[(r * 7 + r // 12) % len(P[INT])],
            np.array(P[LONG], np.int64)[(r * 3 + r // 16) % len(P[LONG])], ((r * 11 + r // 7) % 3 == 0).astype(np.uint8)]
    return cols, r // div


def _sel6(select, k=2):
    types = {f"e{m}.{a}": t for m in range(1, k + 1) for a, t in ATTRS6}
    exprs = [M.parse(x, types) for x in select]
    return exprs, ", ".join(f"{M.text(e)} as c{j}" for j, e in enumerate(exprs))


def _rows6(cols, ords, k=2):
    """The model's row of a tuple of event ordinals."""
    return {f"e{m + 1}.{a}": (bool(cols[c][o]) if t == BOOL else cols[c][o]) for m, o in enumerate(ords)
            for c, (a, t) in enumerate(ATTRS6)}


def _check_against_model(exprs, cols, outs, slots):
    """Every oracle output's values are the model's on the events behind it (refs: one ordinal per selected attribute;
    slots: which of them are e1, e2, ...)."""
    for o in outs:
        row = _rows6(cols, [o[2][s] for s in slots])
        want = M.canon_row([M.value(e, row) for e in exprs], [M.type_of(e) for e in exprs])
        assert M.canon_row(o[1], [M.type_of(e) for e in exprs]) == want, (o, want)


def _projected(app, exprs):
    import torch
    vals, nulls, ts = app.device_project("q")
    torch.cuda.synchronize()
    types = [M.type_of(e) for e in exprs]
    return [(t, tuple(M.from_word(w, z, ty) for w, z, ty in zip(vr, nr, types)))
            for t, vr, nr in zip(ts.cpu().tolist(), vals.cpu().tolist(), nulls.cpu().tolist())]


@functools.lru_cache(maxsize=None)
def closed_form_case(c1, partitioned):
    cols, ts = stock6(20000, 200)
    exprs, sel = _sel6(SELECT6)
    q = f"@info(name='q') from every e1=S[{c1}] -> e2=S[price > e1.price] within 1 sec select {sel} insert into Out;"
    text = f"define stream S ({COLS6}); " + (f"partition with (symbol of S) begin {q} end;" if partitioned else q)
    a = OracleApp(text)
    a.start()
    ptrs = (ctypes.c_void_p * len(cols))(*[c.ctypes.data for c in cols])
    err = ctypes.create_string_buffer(512)
    assert olib().cr_send_columns(a.h, a.stream_index("S"), len(ts), ts.ctypes.data, ptrs, err, 512) == 0, err.value
    outs = a.outputs()["streams"].get("Out", [])
    a.close()
    assert len(outs) > 1000
    _check_against_model(exprs, cols, outs[::7], (0, len(ATTRS6)))
    exp = [(o[0], M.canon_row(o[1], [M.type_of(e) for e in exprs])) for o in outs]
    assert any(row[-1] is None for _, row in exp) and any(row[-2] == "NaN" for _, row in exp)
    return text, exprs, exp


@pytest.mark.parametrize("c1", C1S)
@pytest.mark.parametrize("mode", ["stack", "walk", "unpartitioned"])
def test_closed_form_carried_partials(mode, c1):
    """every e1=S[c1] -> e2=S[price > e1.price] within 1 sec in ragged pieces: c1 through Cond.simple or the generic
    program, every attribute of a carried e1 and two mixed expressions projected on the device, bit-exact."""
    import torch
    from siddhi_amd.testing import ProductApp
    from test_device_stream import pieces
    cols, ts = stock6(20000, 200)
    text, exprs, exp = closed_form_case(c1, mode != "unpartitioned")
    app = ProductApp(text, fast_stack={"stack": 1, "walk": 2, "unpartitioned": 0}[mode])
    dev = torch.device("cuda", 0)
    got, carried = [], 0
    for lo, hi in pieces(20000, [1, 8191, 8193]):
        tcols = [torch.from_numpy(np.ascontiguousarray(c[lo:hi])).to(dev) for c in cols]
        tts = torch.from_numpy(np.ascontiguousarray(ts[lo:hi])).to(dev)
        torch.cuda.synchronize()
        app.process_device_batch("S", tts, tcols, ordinal_base=lo)
        assert app.get_stat("fast_path:q") == (3 if mode == "stack" else 2)
        carried += int((app.device_matches_host("q").view(np.int32)[:, 0] < 0).sum())
        got += _projected(app, exprs)
    app.close()
    assert carried > 0
    _assert_same([got], [exp], f"closed form ({mode})", [c1])


# ---- paths 6 to 9: the facts passes evaluate the members' conditions, the projection reads carried members

def _seq_text(path):
    streams = "define stream A (%s); define stream B (%s); " % (COLS6, COLS6)
    if path == 6:
        k, body = 2, "every e1=A[qty > 0.1f], e2=A[qty >= e1.qty and v != e1.v]"
    elif path == 7:
        k, body = 3, "every e1=A[n / 2 * 2 == n], e2=A[v >= e1.v], e3=A[qty != e2.qty and v < e1.v + 7]"
    elif path == 8:
        k, body = 2, "every e1=A[flag == true or qty <= 2.5], e2=B[v > e1.v and qty != e1.qty]"
    else:
        k, body = 2, "every e1=A[v % 3 != 0] -> e2=B[qty > e1.qty and v <= e1.v] within 40 milliseconds"
    select = [f"e{m}.{a}" for m in range(1, k + 1) for a, _ in ATTRS6[2:]] + [f"e1.qty * e{k}.v", f"e{k}.n % e1.n"]
    exprs, sel = _sel6(select, k)
    q = f"@info(name='q') from {body} select {sel} insert into Out;"
    with_ = "symbol of A" if path in (6, 7) else "symbol of A, symbol of B"
    return streams + f"partition with ({with_}) begin {q} end;", exprs, k


@pytest.mark.parametrize("path", [6, 7, 8, 9])
def test_sequence_closed_forms(path):
    """One query per closed form of paths 6 to 9 over (symbol, price, qty float, n int, v long, flag bool): float and
    long compares against the predecessor, float, int, long and bool attributes of carried members selected. Three
    ragged batches; tuples and projected values equal the oracle's, the values the model's."""
    from test_device_mseq import Run, oracle_out, straddling
    n, K = 6000, 20
    cols, ts = stock6(n, K, 3)
    r = np.arange(n)
    sid = (np.zeros(n) if path in (6, 7) else ((r * 13 + r // 5) % 5 < 2)).astype(np.int32)  # 0 = A, 1 = B
    text, exprs, k = _seq_text(path)
    outs = oracle_out(text, sid, cols, ts)["streams"].get("Out", [])
    assert len(outs) > 50
    per = len(ATTRS6) - 2
    _check_against_model(exprs, cols, outs, [m * per for m in range(k)])
    exp = [(o[0], M.canon_row(o[1], [M.type_of(e) for e in exprs])) for o in outs]
    tuples = np.array([[o[2][m * per] for m in range(k)] for o in outs], dtype=np.int64)
    ranges = [(0, 1), (1, 2049), (2049, n)]
    assert straddling(tuples, ranges) > 0  # a member read back from the carry
    got = []
    if path in (6, 7):  # one stream: sm_app_process_device_batch
        import torch
        from siddhi_amd.testing import ProductApp
        app, dev, dev_tuples, paths = ProductApp(text), torch.device("cuda", 0), [], []
        for lo, hi in ranges:
            tcols = [torch.from_numpy(np.ascontiguousarray(c[lo:hi])).to(dev) for c in cols]
            tts = torch.from_numpy(np.ascontiguousarray(ts[lo:hi])).to(dev)
            torch.cuda.synchronize()
            app.process_device_batch("A", tts, tcols, ordinal_base=lo)
            paths.append(int(app.get_stat("fast_path:q")))
            dev_tuples.append(app.device_matches_host("q").view(np.int32).astype(np.int64) + lo)
            got += _projected(app, exprs)
        app.close()
        dev_tuples = np.concatenate(dev_tuples)
    else:  # streams A and B interleaved: sm_app_process_device_events
        run = Run(text)
        for lo, hi in ranges:
            run.piece(sid, cols, ts, lo, hi)
            got += _projected(run.app, exprs)
        dev_tuples, _, _ = run.finish()
        paths = run.paths
    assert set(paths) == {path}
    np.testing.assert_array_equal(dev_tuples, tuples)
    _assert_same([got], [exp], f"fast_path {path}", [text])
