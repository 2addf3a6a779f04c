"""The expression model (tests/expr_model.py) against the CPU oracle and the host build of the device evaluator
(tests/native/nfa_host_harness.cpp over kernels/expr.h), exactly, on value pools that sit on the promotion, rounding,
wrap-around and null edges. CPU only. The GPU routes are compared with the same model in tests/test_device_expr.py,
which takes its schema, rows and case lists from here."""
import ctypes
import os
import subprocess

import pytest

import expr_model as M
from expr_model import BOOL, DOUBLE, FLOAT, INT, LONG, NUMERIC, POOLS, STRING
from oracle_lib import OracleApp

HERE = os.path.dirname(os.path.abspath(__file__))

ATTRS = [("i", INT), ("i2", INT), ("l", LONG), ("l2", LONG), ("f", FLOAT), ("f2", FLOAT), ("d", DOUBLE), ("d2", DOUBLE),
         ("s", STRING), ("s2", STRING), ("b", BOOL), ("b2", BOOL)]
TYPES = dict(ATTRS)
NAMES = [a for a, _ in ATTRS]
SEND_TYPES = [t for _, t in ATTRS]
NUM_ATTRS = [(a, t) for a, t in ATTRS if t in NUMERIC]
SCHEMA = "define stream S (" + ", ".join(f"{a} {M.QL_TYPE[t]}" for a, t in ATTRS) + "); "
PAIRS = M.numeric_pairs(NUM_ATTRS)  # the 56 ordered pairs of distinct numeric attributes

# conditions (BOOL) and values over the 12-attribute schema; the GPU routes reuse them
NESTED = ["d > 0.1f", "f == 0.1", "f == 0.1f", "l == 16777217.0f", "l < 9223372036854775807L", "i / 2 * 2 == i",
          "(i + l) * f > d % 7", "not (d / d2 > 1)", "(d / d2) is null", "d / d2 != 1", "s == s2", "s != 'a'",
          "s is null", "b == b2", "b", "not b", "b and b2", "b or not b2", "b != true", "l - l2 >= i * i2",
          "f % f2 <= l / i", "f + i == d + i", "2147483647 < i + 1", "l * 3037000500L > 0", "(i % i2) is null"]
FMA_VALUES = ["d * d2 + d", "f * f2 - f"]
DEPTH8 = ["i", "i2", "l", "l2", "f", "f2", "d", "d2"]


def _leaves(e):
    if e[0] in ("var", "const"):
        return [e]
    return [x for ch in e[1:] if isinstance(ch, tuple) for x in _leaves(ch)]


NESTED_NUMERIC = [x for x in NESTED if all(v[2] in NUMERIC for v in _leaves(M.parse(x, TYPES)))]


def rows12(n=400, nulls=True):
    """Deterministic rows over the pools: an unsuffixed attribute walks its pool with r, a suffixed one with r // 20.
    With nulls the pools have 13, 17, 19 and 20 entries (FLOAT takes two nulls), without them 13, 16, 17 and 19 (INT
    repeats its first value): pairwise coprime and at most 20, so every pair of values of (x, y) occurs within 380 rows
    and of (x, y2) within 400. With nulls, row 0 is all null."""
    if nulls:
        pools = {t: [None] * (2 if t == FLOAT else 1) + POOLS[t] for t in POOLS}
    else:
        pools = {t: POOLS[t][:1] * (t == INT) + POOLS[t] for t in POOLS}
    rows = []
    for r in range(n):
        row = {}
        for a, t in ATTRS:
            P = pools[t]
            step = 20 if t in NUMERIC else len(P)
            row[a] = P[(r // step) % len(P)] if a.endswith("2") else P[r % len(P)]
        rows.append(row)
    return rows


def variables(e):
    return sorted({(v[1], v[2]) for v in _leaves(e) if v[0] == "var"})


def eval_rows(e, rows):
    """value(e, row) of every row; rows that agree in the attributes e reads share one evaluation."""
    vs, memo, out = variables(e), {}, []
    for row in rows:
        key = tuple(M.canon(row[a], t) for a, t in vs)
        if key not in memo:
            memo[key] = M.value(e, row)
        out.append(memo[key])
    return out


def send_value(v, t):
    return None if v is None else float(v) if t in (FLOAT, DOUBLE) else v


def run_rows(factory, text, rows, flush_every=0, stream="S", names=NAMES, types=SEND_TYPES):
    """The app's dump after sending every row (timestamp = row number) through the host API."""
    a = factory(text)
    a.start()
    for r, row in enumerate(rows):
        a.send(stream, r, [send_value(row[k], t) for k, t in zip(names, types)], types)
        if flush_every and (r + 1) % flush_every == 0:
            a.flush()
    a.flush()
    out = a.outputs()
    a.close()
    return out


def select_app(exprs, per_query=28, schema=SCHEMA, cond=None, having=None):
    """`from S select e0 as c0, ...` queries of per_query expressions each, into streams V0, V1, ..."""
    qs, groups = [], []
    for k in range(0, len(exprs), per_query):
        g = exprs[k:k + per_query]
        groups.append(g)
        sel = ", ".join(f"{M.text(e)} as c{j}" for j, e in enumerate(g))
        qs.append(f"@info(name='v{len(qs)}') from S{'[' + M.text(cond) + ']' if cond else ''} select {sel}"
                  f"{' having ' + M.text(having) if having else ''} insert into V{len(qs)};")
    return schema + " ".join(qs), groups


def filter_app(conds, schema=SCHEMA):
    return schema + " ".join(f"@info(name='c{k}') from S[{M.text(e)}] select i insert into C{k};"
                             for k, e in enumerate(conds))


def model_values(groups, rows):
    """Per group: [(ts, canonical row)] for every row."""
    out = []
    for g in groups:
        cols = [[M.canon(v, M.type_of(e)) for v in eval_rows(e, rows)] for e in g]
        out.append([(r, tuple(c[r] for c in cols)) for r in range(len(rows))])
    return out


def dump_values(out, groups):
    return [[(o[0], M.canon_row(o[1], [M.type_of(e) for e in g])) for o in out["streams"].get(f"V{k}", [])]
            for k, g in enumerate(groups)]


def model_kept(conds, rows):
    return [[r for r, v in enumerate(eval_rows(e, rows)) if v is True] for e in conds]


def dump_kept(out, conds):
    return [[o[0] for o in out["streams"].get(f"C{k}", [])] for k in range(len(conds))]


@pytest.fixture(scope="module")
def harness():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "native")])
    from host_harness_lib import HostHarnessApp
    return HostHarnessApp


@pytest.fixture(scope="module")
def rows():
    return rows12()


def _assert_same(got, exp, what, labels):
    for k, (g, e) in enumerate(zip(got, exp)):
        if g != e:
            bad = next((x, y) for x, y in zip(g + [None], e + [None]) if x != y)
            raise AssertionError(f"{what}: {labels[k]}: first difference (got, model) = {bad}")


def test_math_all_pairs(harness, rows):
    """select A op B for the five math ops over the 56 ordered pairs: model == oracle == host build, bit-exact."""
    exprs = [M.m(op, M.var(a, ta), M.var(b, tb)) for op in M.MATH_OPS for (a, ta), (b, tb) in PAIRS]
    assert len(exprs) == 280
    text, groups = select_app(exprs)
    exp = model_values(groups, rows)
    flat = [v for g in exp for _, row in g for v in row]
    assert "NaN" in flat and M.canon(M.INF, DOUBLE) in flat and M.canon(-M.INF, DOUBLE) in flat and None in flat
    assert rows[0]["i"] is None and exp[0][0][1][0] is None  # the first staged row carries nulls
    labels = [" | ".join(M.text(e) for e in g) for g in groups]
    for name, factory in (("oracle", OracleApp), ("host build", harness)):
        _assert_same(dump_values(run_rows(factory, text, rows), groups), exp, name, labels)


def test_compare_all_pairs(harness, rows):
    """[A cmp B] for the six compares over the same pairs: the kept rows."""
    conds = [M.c(op, M.var(a, ta), M.var(b, tb)) for op in M.CMP_OPS for (a, ta), (b, tb) in PAIRS]
    assert len(conds) == 336
    text = filter_app(conds)
    exp = model_kept(conds, rows)
    labels = [M.text(e) for e in conds]
    for name, factory in (("oracle", OracleApp), ("host build", harness)):
        _assert_same(dump_kept(run_rows(factory, text, rows), conds), exp, name, labels)


def test_nested_constant_string_bool_null(harness, rows):
    conds = [M.parse(x, TYPES) for x in NESTED]
    vals = [M.parse(x, TYPES) for x in FMA_VALUES]
    ctext = filter_app(conds)
    vtext, groups = select_app(vals)
    exp_c, exp_v = model_kept(conds, rows), model_values(groups, rows)
    assert all(len(kept) < len(rows) for kept in exp_c)
    # (float)0.1 widened is not the double 0.1, and MAX + 1 wraps to MIN: these two hold for no row, the others for some
    assert [x for x, kept in zip(NESTED, exp_c) if not kept] == ["f == 0.1", "2147483647 < i + 1"]
    for name, factory in (("oracle", OracleApp), ("host build", harness)):
        _assert_same(dump_kept(run_rows(factory, ctext, rows), conds), exp_c, name, NESTED)
        _assert_same(dump_values(run_rows(factory, vtext, rows), groups), exp_v, name, FMA_VALUES)


def test_harness_keeps_a_null_in_the_first_staged_row(harness):
    """7 + null is null on row 0 as on every later row, also after a flush emptied the stage."""
    text = SCHEMA + "from S select 7 + i as x insert into V0;"
    a = harness(text)
    a.start()
    row = [None, 1, 1, 1, 1.0, 1.0, 1.0, 1.0, "a", "a", True, True]
    a.send("S", 0, row, SEND_TYPES)
    a.send("S", 1, [5] + row[1:], SEND_TYPES)
    a.flush()
    a.send("S", 2, row, SEND_TYPES)
    a.flush()
    a.send("S", 3, [5] + row[1:], SEND_TYPES)  # no null staged since the flush: the mask is gone again
    a.flush()
    assert [o[1] for o in a.outputs()["streams"]["V0"]] == [[None], [12], [None], [12]]
    a.close()


def test_harness_dump_is_json_for_non_finite_values(harness):
    text = SCHEMA + "from S select d * d2 as x, f * f2 as y, d - d as z insert into V0;"
    a = harness(text)
    a.start()
    big = [1, 1, 1, 1, 3e38, 10.0, 1e308, 10.0, "a", "a", True, True]
    a.send("S", 0, big, SEND_TYPES)
    a.send("S", 1, big[:6] + [-1e308, 10.0] + big[8:], SEND_TYPES)
    a.send("S", 2, big[:6] + [float("inf"), 1.0] + big[8:], SEND_TYPES)
    a.flush()
    got = [o[1] for o in a.outputs()["streams"]["V0"]]  # json.loads inside: "-nan.0" would not parse
    a.close()
    assert got == [["Infinity", "Infinity", 0.0], ["-Infinity", "Infinity", 0.0], ["Infinity", "Infinity", "NaN"]]


def test_pools_discriminate_every_compare_leaf():
    """A condition on the inputs, not on the code: on the cross product of the two pools, every (type, cmp, type) leaf
    keeps at least 5 pairs and drops at least 5 by the model alone, so a wrong promotion cannot hide in a leaf that
    keeps everything or nothing; and `/`, `%` yield null for 12 to 38 pairs of every type pair (the zero divisors)."""
    fractions = []
    for ta in NUMERIC:
        for tb in NUMERIC:
            rows = M.cross_rows(["x"], POOLS[ta], ["x2"], POOLS[tb])
            assert len(rows) == len(POOLS[ta]) * len(POOLS[tb])
            for op in M.CMP_OPS:
                e = M.c(op, M.var("x", ta), M.var("x2", tb))
                kept = sum(M.truthy(e, r) for r in rows)
                assert kept >= 5 and len(rows) - kept >= 5, (ta, op, tb, kept, len(rows))
                fractions.append(kept / len(rows))
            for op in "/%":
                e = M.m(op, M.var("x", ta), M.var("x2", tb))
                nulls = sum(M.value(e, r) is None for r in rows)
                # the zero divisors: every pool holds one (FLOAT and DOUBLE two, 0.0 and -0.0), and no dividend
                # pool has fewer than 12 values
                zeros = sum(1 for v in POOLS[tb] if v == 0)
                assert nulls == zeros * len(POOLS[ta]) >= 12, (ta, op, tb, nulls)
    assert len(fractions) == 96
    print(f"kept fraction per leaf: {min(fractions):.3f} .. {max(fractions):.3f}")


def _deep(n):
    terms = (DEPTH8 + ["i"])[:n]
    return M.right_sum([M.var(a, TYPES[a]) for a in terms])


def test_operand_stack_limit(harness, rows):
    """kMaxStack = 8: a right-nested sum of 8 operands needs all 8 entries, compiles and evaluates to the model's
    value; one of 9 is refused by the compiler with its "operand stack" message, by the product library
    (sm_compile_dump parses only, so the refusal is taken where the library compiles a query without a device:
    sm_nfa_jit_compile, which fails before any kernel is built) and by the host build. Nothing crashes."""
    import siddhi_amd
    from siddhi_amd import _lib
    from host_harness_lib import HarnessError
    text8, groups = select_app([_deep(8)])
    assert siddhi_amd.compile_dump(text8)["queries"]
    exp = model_values(groups, rows)
    assert len({v for _, row in exp[0] for v in row}) > 50
    for name, factory in (("oracle", OracleApp), ("host build", harness)):
        _assert_same(dump_values(run_rows(factory, text8, rows), groups), exp, name, [M.text(_deep(8))])
    text9, _ = select_app([_deep(9)])
    with pytest.raises(HarnessError, match="operand stack"):
        harness(text9)
    log = ctypes.create_string_buffer(4096)
    size = ctypes.c_size_t()
    rc = _lib.lib().sm_nfa_jit_compile(text9.encode(), 0, log, 4096, ctypes.byref(size))
    assert rc != 0 and "operand stack" in log.value.decode()
    # as a filter and inside a pattern's condition too
    with pytest.raises(HarnessError, match="operand stack"):
        harness(SCHEMA + f"from S[{M.text(_deep(9))} > 0] select i insert into O;")
    with pytest.raises(HarnessError, match="operand stack"):
        harness(SCHEMA + f"from every e1=S -> e2=S[{M.text(_deep(9))} > e1.d] select e1.i as a insert into O;")


def test_model_reads_its_own_text():
    """text() and parse() agree, so the SiddhiQL a test sends is the tree the model evaluates."""
    for x in NESTED + FMA_VALUES:
        e = M.parse(x, TYPES)
        assert M.parse(M.text(e), TYPES) == e


@pytest.mark.parametrize("name", ["q0", "q1", "q2", "q3"])
def test_nfa_select_lists_on_the_host_build(harness, name):
    """The pattern queries tests/test_device_expr.py runs on the GPU (e1 read back from a stored partial, e2 the current
    event; nulls, strings, bools, the depth-8 sum, a * b + c), here through the oracle and the host build of the NFA."""
    import test_device_expr as D
    text, exprs, cond, hv_model = D.nfa_text(name)
    joined = D.nfa_events()[2]
    keep = [a is True and b is True for a, b in zip(eval_rows(cond, joined), eval_rows(hv_model, joined))]
    exp = [[(2 * j + 1, row) for (j, row) in model_values([exprs], joined)[0] if keep[j]]]
    assert 40 < len(exp[0]) < D.N_KEYS - 20, len(exp[0])
    for what, factory in (("oracle", OracleApp), ("host build", harness)):
        out, _ = D.run_nfa(factory, text)
        got = [[(o[0], M.canon_row(o[1], [M.type_of(e) for e in exprs])) for o in out["streams"].get("Out", [])]]
        _assert_same(got, exp, what, [name])


def test_harness_refuses_an_output_stream_of_49_attributes(harness):
    """A stream descriptor holds 48 columns (kMaxAttrs) and the inferred output stream counts: the product refuses the
    app, and so does the host build (it used to write past its descriptors)."""
    from host_harness_lib import HarnessError
    text, _ = select_app([M.var("i", INT)] * 49, per_query=49)
    with pytest.raises(HarnessError, match="too many attributes"):
        harness(text)
    harness(select_app([M.var("i", INT)] * 48, per_query=48)[0]).close()
