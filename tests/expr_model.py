"""The reference's expression semantics stated once in numpy / Python, with no project code in it: the model every
device route's evaluator (siddhi_amd/csrc/kernels/expr.h and its restatements) is compared with, next to the oracle.

An expression is a small tuple tree; text(e) is its SiddhiQL and value(e, row) its value on a row (dict attribute
name -> Python value, None = null), so one object yields the query text and the expected result.

  ("var", name, TYPE)   ("const", v, TYPE)   ("math", op, l, r)   ("cmp", op, l, r)
  ("and", l, r)   ("or", l, r)   ("not", x)   ("isnull", x)

Values: INT / LONG are Python ints (wrapped to the type), FLOAT np.float32, DOUBLE np.float64, STRING str, BOOL bool.
Rules, each beside the reference file it restates (paths under siddhi-core/.../core/executor/):
  math result type      widest of INT < LONG < FLOAT < DOUBLE (ExpressionParser.parseArithmeticOperationResultType)
  math                  math/{add,subtract,multiply,divide,mod}/*ExpressionExecutor{Int,Long,Float,Double}.java:
                        null operand -> null; both operands through Number.xxxValue() of the result type; divide and
                        mod return null for a divisor == 0 (so -0.0 too); Java int / long wrap, `/` truncates, `%`
                        takes the dividend's sign; float and double `%` are fmod
  compare               condition/compare/**/*CompareConditionExpressionExecutor<L><R>.java: Java binary numeric
                        promotion of the two static types, except Equal / NotEqual FloatLong and LongFloat, which
                        compare doubleValue()s; null operand -> false (CompareConditionExpressionExecutor.java), true for
                        NotEqual (NotEqualCompareConditionExpressionExecutor.java)
  and / or              condition/{And,Or}ConditionExpressionExecutor.java: null counts as false
  not                   condition/NotConditionExpressionExecutor.java: not null -> true
  is null               condition/IsNullConditionExpressionExecutor.java
  string, bool          Equal / NotEqual only (StringString, BoolBool)
"""
import itertools
import math
import struct

import numpy as np

INT, LONG, FLOAT, DOUBLE, STRING, BOOL = "INT", "LONG", "FLOAT", "DOUBLE", "STRING", "BOOL"
NUMERIC = (INT, LONG, FLOAT, DOUBLE)
RANK = {INT: 0, LONG: 1, FLOAT: 2, DOUBLE: 3}
MATH_OPS = ("+", "-", "*", "/", "%")
CMP_OPS = ("==", "!=", "<", "<=", ">", ">=")
QL_TYPE = {INT: "int", LONG: "long", FLOAT: "float", DOUBLE: "double", STRING: "string", BOOL: "bool"}

f32, f64 = np.float32, np.float64
NAN, INF = float("nan"), float("inf")

# ---- value pools (None = null is added by the caller where the route can carry nulls)
POOLS = {
    INT: [0, 1, -1, 2, -2, 7, -7, 2**31 - 1, -2**31, 16777216, 16777217, 46341],
    LONG: [0, 1, -1, 3, -3, 7, -7, 2, 2**63 - 1, -2**63, 2**53 + 1, 2**31, -2**31 - 1, 16777216, 16777217, 3037000500],
    FLOAT: [f32(x) for x in (0.0, -0.0, 1, -1, 0.1, 2.5, -7.5, 7, 16777216, 16777218, 3.4028235e38, 1e-45, NAN, INF,
                             -INF, 1 + 2.0**-13, 1 - 2.0**-13)],
    DOUBLE: [f64(x) for x in (0.0, -0.0, 1, -1, 0.1, float(f32(0.1)), 2.5, -7.5, 7, 16777216, 16777217,
                              float(2**53 + 1), 1.7976931348623157e308, 5e-324, NAN, INF, -INF, 1 + 2.0**-30,
                              1 - 2.0**-30)],
    STRING: ["a", "b", ""],
    BOOL: [True, False],
}


def cross_rows(names_p, P, names_q, Q, n=None):
    """Rows r = 0 .. n-1 (default |P| * |Q|): attributes names_p take P[r % |P|], names_q take Q[(r // |P|) % |Q|]."""
    n = len(P) * len(Q) if n is None else n
    rows = []
    for r in range(n):
        row = {a: P[r % len(P)] for a in names_p}
        row.update({a: Q[(r // len(P)) % len(Q)] for a in names_q})
        rows.append(row)
    return rows


# ---- constructors
def var(name, t):
    return ("var", name, t)


def const(v, t):
    return ("const", coerce(v, t), t)


def m(op, l, r):
    return ("math", op, l, r)


def c(op, l, r):
    return ("cmp", op, l, r)


def coerce(v, t):
    """A Python / numpy value as the model's value of type t (what an InputHandler.send of it stores)."""
    if v is None:
        return None
    if t == INT:
        return _wrap(int(v), 32)
    if t == LONG:
        return _wrap(int(v), 64)
    if t == FLOAT:
        return f32(v)
    if t == DOUBLE:
        return f64(v)
    if t == BOOL:
        return bool(v)
    return str(v)


def type_of(e):
    k = e[0]
    if k in ("var", "const"):
        return e[2]
    if k == "math":
        a, b = type_of(e[2]), type_of(e[3])
        return max(a, b, key=RANK.__getitem__)
    return BOOL


def _lit(v, t):
    if t == INT:
        return str(v)
    if t == LONG:
        return f"{v}L"
    if t == FLOAT:
        return str(f32(v)) + "f"  # shortest text that reads back as this float
    if t == DOUBLE:
        return repr(float(v))
    if t == BOOL:
        return "true" if v else "false"
    return "'" + v + "'"


def text(e):
    """SiddhiQL of e, every binary node in parentheses (the grammar's own precedence is not relied on)."""
    k = e[0]
    if k == "var":
        return e[1]
    if k == "const":
        return e[3] if len(e) > 3 else _lit(e[1], e[2])  # a literal read by parse() keeps its spelling
    if k in ("math", "cmp"):
        return f"({text(e[2])} {e[1]} {text(e[3])})"
    if k in ("and", "or"):
        return f"({text(e[1])} {k} {text(e[2])})"
    if k == "not":
        return f"(not {text(e[1])})"
    return f"({text(e[1])} is null)"


# ---- evaluation
def _wrap(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def _to(v, t_from, t_to):
    """Number.intValue / longValue / floatValue / doubleValue of a value whose static type is t_from."""
    if t_to in (INT, LONG):
        return int(v)  # only widening INT -> LONG reaches here
    if t_from in (INT, LONG):
        x = np.array(v, dtype=np.int64)
        return x.astype(np.float32)[()] if t_to == FLOAT else x.astype(np.float64)[()]
    if t_to == FLOAT:
        return f32(v)
    return f64(f32(v)) if t_from == FLOAT else f64(v)


def _trunc_div(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _math(op, a, b, t):
    if t in (INT, LONG):
        bits = 32 if t == INT else 64
        if op in "/%" and b == 0:
            return None
        if op == "+":
            z = a + b
        elif op == "-":
            z = a - b
        elif op == "*":
            z = a * b
        elif op == "/":
            z = _trunc_div(a, b)
        else:
            z = a - b * _trunc_div(a, b)
        return _wrap(z, bits)
    if op in "/%" and b == 0:  # true for -0.0 as well
        return None
    with np.errstate(all="ignore"):
        if op == "+":
            z = a + b
        elif op == "-":
            z = a - b
        elif op == "*":
            z = a * b
        elif op == "/":
            z = a / b
        else:
            z = np.fmod(a, b)
    assert z.dtype == (np.float32 if t == FLOAT else np.float64)
    return z


def cmp_domain(op, a, b):
    """The type the two operands are compared in."""
    if a not in NUMERIC:
        return a
    if DOUBLE in (a, b):
        return DOUBLE
    if FLOAT in (a, b):
        return DOUBLE if (op in ("==", "!=") and LONG in (a, b)) else FLOAT
    return LONG if LONG in (a, b) else INT


def _cmp(op, x, y):
    if op == "==":
        return bool(x == y)
    if op == "!=":
        return bool(x != y)
    if op == "<":
        return bool(x < y)
    if op == "<=":
        return bool(x <= y)
    if op == ">":
        return bool(x > y)
    return bool(x >= y)


def value(e, row):
    k = e[0]
    if k == "var":
        return coerce(row[e[1]], e[2])
    if k == "const":
        return e[1]
    if k == "math":
        t = type_of(e)
        a, b = value(e[2], row), value(e[3], row)
        if a is None or b is None:
            return None
        return _math(e[1], _to(a, type_of(e[2]), t), _to(b, type_of(e[3]), t), t)
    if k == "cmp":
        a, b = value(e[2], row), value(e[3], row)
        if a is None or b is None:
            return e[1] == "!="
        ta, tb = type_of(e[2]), type_of(e[3])
        if ta not in NUMERIC:
            assert ta == tb and e[1] in ("==", "!=")
            return _cmp(e[1], a, b)
        d = cmp_domain(e[1], ta, tb)
        return _cmp(e[1], _to(a, ta, d), _to(b, tb, d))
    if k == "and":
        return bool(value(e[1], row)) and bool(value(e[2], row))
    if k == "or":
        return bool(value(e[1], row)) or bool(value(e[2], row))
    if k == "not":
        return not bool(value(e[1], row))
    return value(e[1], row) is None


def truthy(e, row):
    """A filter / having keeps the event when the condition is true (null counts as false)."""
    return value(e, row) is True


# ---- exact comparison: canonical images
def canon(v, t):
    """Hashable exact image: ints as ints, FLOAT / DOUBLE by the bits of their double image (-0.0 != 0.0), every NaN
    as "NaN" (Java fixes no payload). Accepts the JSON dumps' "NaN" / "Infinity" / "-Infinity" strings."""
    if v is None:
        return None
    if t in (FLOAT, DOUBLE):
        if isinstance(v, str):
            v = {"NaN": NAN, "Infinity": INF, "-Infinity": -INF}[v]
        d = float(f32(v)) if (t == FLOAT and not isinstance(v, float)) else float(v)
        return "NaN" if math.isnan(d) else struct.unpack("<q", struct.pack("<d", d))[0]
    if t == BOOL:
        assert isinstance(v, (bool, np.bool_)), v
        return bool(v)
    if t == STRING:
        return str(v)
    assert not isinstance(v, (bool, float)), v
    return int(v)


def canon_row(vals, types):
    return tuple(canon(v, t) for v, t in zip(vals, types))


def from_word(w, is_null, t):
    """A device_project word (raw 64-bit: integers, or double bits for FLOAT / DOUBLE) as a canonical image."""
    if is_null:
        return None
    if t in (FLOAT, DOUBLE):
        return canon(struct.unpack("<d", struct.pack("<q", int(w)))[0], DOUBLE)
    return bool(w) if t == BOOL else int(w)


def numeric_pairs(attrs):
    """Ordered pairs of distinct attributes, attrs = [(name, TYPE), ...]."""
    return [(a, b) for a, b in itertools.permutations(attrs, 2)]


def right_sum(terms):
    """t0 + (t1 + (t2 + ...)): needs len(terms) operand-stack entries."""
    e = terms[-1]
    for t in reversed(terms[:-1]):
        e = m("+", t, e)
    return e


# ---- the test lists are written as SiddhiQL; this reads them into the tree (SiddhiQL.g4 precedence: or < and <
# ==, != < relational < +, - < *, /, % < not < `is null`)
import re  # noqa: E402

_TOKEN = re.compile(r"\s*(?:(\d+\.\d*(?:[eE][-+]?\d+)?[fFdD]?|\d+(?:[eE][-+]?\d+)[fFdD]?|\d+[lLfFdD]?)|'([^']*)'"
                    r"|([A-Za-z_][A-Za-z_0-9]*(?:\.[A-Za-z_][A-Za-z_0-9]*)?)|(==|!=|<=|>=|[-+*/%<>()]))")


def parse(src, types):
    """SiddhiQL expression -> tree. types: attribute name (as written, e.g. "d" or "e1.d") -> TYPE."""
    toks, pos = [], 0
    src = src.rstrip()
    while pos < len(src):
        mt = _TOKEN.match(src, pos)
        assert mt, f"cannot read {src[pos:]!r}"
        pos = mt.end()
        num, st, ident, sym = mt.groups()
        toks.append(("num", num) if num is not None else ("str", st) if st is not None else
                    ("id", ident) if ident is not None else ("sym", sym))
    toks.append(("end", None))
    p = [0]

    def peek(k=0):
        return toks[min(p[0] + k, len(toks) - 1)]  # k = -1: the token just taken

    def take():
        p[0] += 1
        return toks[p[0] - 1]

    def number(neg):
        return number_value(neg) + (("-" if neg else "") + peek(-1)[1],)

    def number_value(neg):
        s = take()[1]
        sign = -1 if neg else 1
        if s[-1] in "lL":
            return const(sign * int(s[:-1]), LONG)
        if s[-1] in "fF":
            return const(f32(sign * float(f32(s[:-1]))), FLOAT)
        if s[-1] in "dD":
            return const(sign * float(s[:-1]), DOUBLE)
        if any(ch in s for ch in ".eE"):
            return const(sign * float(s), DOUBLE)
        return const(sign * int(s), INT)

    def primary():
        k, v = peek()
        if (k, v) == ("sym", "("):
            take()
            e = expr()
            assert take() == ("sym", ")")
            return e
        if k == "sym" and v in "-+" and peek(1)[0] == "num":
            take()
            return number(v == "-")
        if k == "num":
            return number(False)
        if k == "str":
            take()
            return const(v, STRING)
        assert k == "id", f"unexpected {v!r} in {src!r}"
        take()
        if v in ("true", "false"):
            return const(v == "true", BOOL)
        return var(v, types[v])

    def unary():
        if peek() == ("id", "not"):
            take()
            return ("not", unary())
        e = primary()
        if peek() == ("id", "is") and peek(1) == ("id", "null"):
            take(), take()
            return ("isnull", e)
        return e

    def level(ops, nxt, kind):
        def f():
            e = nxt()
            while peek()[0] in ("sym", "id") and peek()[1] in ops:
                op = take()[1]
                e = (op, e, nxt()) if kind is None else (kind, op, e, nxt())
            return e
        return f

    mul = level(("*", "/", "%"), unary, "math")
    add = level(("+", "-"), mul, "math")
    rel = level(("<", "<=", ">", ">="), add, "cmp")
    eq = level(("==", "!="), rel, "cmp")
    conj = level(("and",), eq, None)
    expr = level(("or",), conj, None)
    e = expr()
    assert peek()[0] == "end", f"trailing {peek()} in {src!r}"
    return e
