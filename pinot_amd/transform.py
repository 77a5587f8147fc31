"""Transform expressions (query.Expr) on the host: validation, type inference, lowering to the device program of
pa_query_set_expressions (include/pinot_amd.h "transform expressions"), and a numpy evaluator of that same program.

Semantics follow pinot-core's operator/transform/function/: AdditionTransformFunction (acc = the sum of the literal
arguments, then += every other argument in order), MultiplicationTransformFunction (the same with a product),
SubtractionTransformFunction / DivisionTransformFunction / ModuloTransformFunction (two arguments), the
SingleParamMathTransformFunctions abs / ceil / floor, and TimeConversionTransformFunction over
java.util.concurrent.TimeUnit (JavaTimeUnitTransformer). All arithmetic is in double (transformToDoubleValuesSV);
TIMECONVERT reads its argument as long and returns long.
"""
import struct

import numpy as np

from . import _lib as L
from .query import Expr

DOUBLE, LONG = "DOUBLE", "LONG"
LONG_MAX, LONG_MIN = 2**63 - 1, -2**63

# canonical function name -> (TransformFunctionType, device opcode of the n-ary / binary / unary arithmetic)
_NARY = {"add": ("ADD", L.PA_EXPR_ADD), "plus": ("ADD", L.PA_EXPR_ADD),
         "mult": ("MULT", L.PA_EXPR_MUL), "times": ("MULT", L.PA_EXPR_MUL)}
_BINARY = {"sub": ("SUB", L.PA_EXPR_SUB), "minus": ("SUB", L.PA_EXPR_SUB),
           "div": ("DIV", L.PA_EXPR_DIV), "divide": ("DIV", L.PA_EXPR_DIV), "mod": ("MOD", L.PA_EXPR_MOD)}
_UNARY = {"abs": ("ABS", L.PA_EXPR_ABS), "ceil": ("CEIL", L.PA_EXPR_CEIL), "ceiling": ("CEIL", L.PA_EXPR_CEIL),
          "floor": ("FLOOR", L.PA_EXPR_FLOOR)}
# java.util.concurrent.TimeUnit in nanoseconds
TIME_UNITS = {"NANOSECONDS": 1, "MICROSECONDS": 10**3, "MILLISECONDS": 10**6, "SECONDS": 10**9,
              "MINUTES": 60 * 10**9, "HOURS": 3600 * 10**9, "DAYS": 86400 * 10**9}
CUSTOM_TIME_UNITS = ("WEEKS", "MONTHS", "YEARS")  # CustomTimeUnitTransformer: not on this path
NUMERIC_TYPES = ("INT", "LONG", "FLOAT", "DOUBLE")


def _unsupported(msg):
    from .engine import UnsupportedQuery
    return UnsupportedQuery(msg)


class DoubleKey(float):
    """A DOUBLE group-key value compared the way the reference's Double2IntOpenHashMap compares keys, by
    Double.doubleToLongBits: every NaN is one key, and -0.0 and 0.0 are two."""
    __slots__ = ()

    def bits(self):
        return 0x7ff8000000000000 if float.__ne__(self, self) else struct.unpack("<Q", struct.pack("<d", self))[0]

    def __eq__(self, other):
        if not isinstance(other, (float, int)) or isinstance(other, bool):
            return NotImplemented
        try:
            return self.bits() == DoubleKey(other).bits()
        except OverflowError:
            return False

    def __ne__(self, other):
        r = self.__eq__(other)
        return r if r is NotImplemented else not r

    def __hash__(self):
        return 0x7ff8 if float.__ne__(self, self) else float.__hash__(self)

    def __repr__(self):
        return float.__repr__(self)


def _is_lit(a):
    return not isinstance(a, Expr) and a[0] == "lit"


def _lit_double(a):
    try:
        return float(a[1])  # (Double.parseDouble of the literal's string)
    except ValueError:
        raise _unsupported("the literal %r is not a number (a transform expression's operand)" % (a[1],)) from None


def infer_type(expr):
    """DOUBLE or LONG: the result type of a validated expression (every function returns DOUBLE but TIMECONVERT)."""
    return LONG if expr.fn == "timeconvert" else DOUBLE


def validate(expr, schema=None):
    """Raises UnsupportedQuery (ValueError for a wrong argument count or unit, with the reference's message where it has
    one) unless the engine runs `expr`. schema: {column: (data type, single value)} checks the operand columns too."""
    if not isinstance(expr, Expr):
        raise TypeError("not an expression: %r" % (expr,))
    fn, args = expr.fn, expr.args
    if fn in _NARY:
        if len(args) < 2:
            raise ValueError("At least 2 arguments are required for %s transform function" % _NARY[fn][0])
    elif fn in _BINARY:
        if len(args) != 2:
            raise ValueError("Exactly 2 arguments are required for %s transform function" % _BINARY[fn][0])
    elif fn in _UNARY:
        if len(args) != 1:
            raise ValueError("Exactly 1 argument is required for %s transform function" % _UNARY[fn][0])
    elif fn == "timeconvert":
        if len(args) != 3:
            raise ValueError("Exactly 3 arguments are required for TIME_CONVERT transform function")
        if _is_lit(args[0]):
            raise ValueError("The first argument of TIME_CONVERT transform function must be a single-valued column or a "
                             "transform function")
        for u in args[1:]:
            if not _is_lit(u):
                raise ValueError("the time units of TIME_CONVERT must be literals")
        if args[2][1].upper() in CUSTOM_TIME_UNITS:
            raise _unsupported("TIME_CONVERT to the custom time unit %s" % args[2][1].upper())
        for u in args[1:]:
            if u[1].upper() not in TIME_UNITS:  # (TimeUnit.valueOf)
                raise ValueError("No enum constant java.util.concurrent.TimeUnit.%s" % u[1].upper())
        args = args[:1]
    else:
        raise _unsupported("transform function %s" % fn)
    if all(_is_lit(a) for a in args):
        raise _unsupported("an expression made only of literals: %s" % expr)
    for a in args:
        if isinstance(a, Expr):
            validate(a, schema)
        elif a[0] == "lit":
            _lit_double(a)
        elif schema is not None:
            if a[1] not in schema:
                raise _unsupported("unknown column %s in %s" % (a[1], expr))
            dt, sv = schema[a[1]][0], schema[a[1]][-1]
            if not sv:
                raise _unsupported("multi-value column %s in the transform expression %s" % (a[1], expr))
            if dt not in NUMERIC_TYPES:
                raise _unsupported("%s column %s in the transform expression %s" % (dt, a[1], expr))


AGGREGATIONS = ("SUM", "MIN", "MAX", "AVG", "MINMAXRANGE")  # the functions that aggregate an expression's values


def query_expressions(query):
    """The distinct expressions of a query's group-by items and aggregation arguments, in that order."""
    out = []
    for item in list(query.group_by) + [a.column for a in query.aggregations]:
        if isinstance(item, Expr) and item not in out:
            out.append(item)
    return out


def check_query(query, schema=None):
    """Raises UnsupportedQuery for every use of transform expressions the engine refuses (and validate's errors);
    returns (expressions, programs over one shared operand-column table, that table) otherwise."""
    for c in list(query.select_columns) + [o.expr for o in query.order_by]:
        if isinstance(c, Expr) and (query.is_selection or query.is_distinct):
            raise _unsupported("transform expression %s in a %s" % (c, "selection" if query.is_selection else
                                                                    "DISTINCT list"))
    exprs = query_expressions(query)
    if not exprs:
        return [], [], []
    if str(query.options.get("enableNullHandling", "false")).lower() == "true":
        raise _unsupported("transform expressions with null handling")
    for a in query.aggregations:
        if a.filter is not None:
            raise _unsupported("transform expressions next to aggregation filters (FILTER (WHERE ...))")
        if isinstance(a.column, Expr) and a.function not in AGGREGATIONS:
            raise _unsupported("%s over the transform expression %s" % (a.function, a.column))
    if len(exprs) > L.PA_MAX_EXPRS:
        raise _unsupported("more than %d transform expressions in one query" % L.PA_MAX_EXPRS)
    columns, programs = [], []
    for e in exprs:
        validate(e, schema)
        programs.append(lower(e, columns))
    return exprs, programs, columns


class Program:
    """One lowered expression: result_type (DOUBLE / LONG), ops — tuples (opcode, dst, a_kind, a, b_kind, b) where an
    immediate operand's value (float for ARG_F64, int for ARG_I64) stands in a / b — and columns, the operand columns
    LOAD_COL's index refers to."""

    def __init__(self, result_type, ops, columns):
        self.result_type, self.ops, self.columns = result_type, ops, columns

    def infix(self):
        """The evaluation order as a parenthesised string, e.g. ((3.0 + a) + b): what the lowering tests pin."""
        sym = {L.PA_EXPR_ADD: "+", L.PA_EXPR_SUB: "-", L.PA_EXPR_MUL: "*", L.PA_EXPR_DIV: "/", L.PA_EXPR_MOD: "%"}
        name = {L.PA_EXPR_ABS: "abs", L.PA_EXPR_CEIL: "ceil", L.PA_EXPR_FLOOR: "floor", L.PA_EXPR_D2L: "d2l",
                L.PA_EXPR_L2D: "l2d", L.PA_EXPR_TCONV_DIV: "tdiv", L.PA_EXPR_TCONV_MUL: "tmul"}
        reg, last = {}, None

        def opnd(kind, v):
            return reg[v] if kind == L.PA_EXPR_ARG_REG else repr(v)
        for op, dst, ak, a, bk, b in self.ops:
            if op == L.PA_EXPR_LOAD_COL:
                s = self.columns[a] if b == L.PA_EXPR_DOUBLE else "long(%s)" % self.columns[a]
            elif op in sym:
                s = "(%s %s %s)" % (opnd(ak, a), sym[op], opnd(bk, b))
            elif op in (L.PA_EXPR_TCONV_DIV, L.PA_EXPR_TCONV_MUL):
                s = "%s(%s, %d)" % (name[op], opnd(ak, a), b)
            else:
                s = "%s(%s)" % (name[op], opnd(ak, a))
            reg[dst] = last = s
        return last


def lower(expr, columns=None):
    """The device program of a validated expression, in the reference's evaluation order. columns: the query's operand
    column table, extended in place with the columns this expression reads (default: a table of its own)."""
    columns = [] if columns is None else columns
    ops, free = [], list(range(L.PA_MAX_EXPR_REGS))
    REG, F64, I64 = L.PA_EXPR_ARG_REG, L.PA_EXPR_ARG_F64, L.PA_EXPR_ARG_I64

    def alloc():
        if not free:
            raise _unsupported("the expression %s needs more than %d value registers" % (expr, L.PA_MAX_EXPR_REGS))
        return free.pop(0)

    def release(r):
        free.insert(0, r)
        free.sort()

    def emit(*op):
        if len(ops) == L.PA_MAX_EXPR_OPS:
            raise _unsupported("the expression %s takes more than %d operations" % (expr, L.PA_MAX_EXPR_OPS))
        ops.append(op)

    def load(name, conv):
        if name not in columns:
            if len(columns) == L.PA_MAX_EXPR_COLUMNS:
                raise _unsupported("the query's expressions read more than %d distinct columns" % L.PA_MAX_EXPR_COLUMNS)
            columns.append(name)
        r = alloc()
        emit(L.PA_EXPR_LOAD_COL, r, L.PA_EXPR_ARG_COL, columns.index(name), 0, conv)
        return r

    def as_double(node):
        """(kind, value): a double immediate, or the register holding the node's value as a double."""
        if isinstance(node, Expr):
            r, t = gen(node)
            if t == LONG:
                emit(L.PA_EXPR_L2D, r, REG, r, 0, 0)
            return REG, r
        if node[0] == "lit":
            return F64, _lit_double(node)
        return REG, load(node[1], L.PA_EXPR_DOUBLE)

    def gen(e):
        """Emits e's operations; returns (register holding the value, its type)."""
        fn, args = e.fn, e.args
        if fn in _NARY:
            op = _NARY[fn][1]
            acc = 0.0 if op == L.PA_EXPR_ADD else 1.0  # literal terms folded first, as the reference's init() does
            for a in args:
                if _is_lit(a):
                    acc = acc + _lit_double(a) if op == L.PA_EXPR_ADD else acc * _lit_double(a)
            cur = None
            for a in args:
                if _is_lit(a):
                    continue
                _, r = as_double(a)
                if cur is None:
                    emit(op, r, F64, acc, REG, r)  # (0.0 + a: a -0.0 operand becomes +0.0 here, as in the reference)
                    cur = r
                else:
                    emit(op, cur, REG, cur, REG, r)
                    release(r)
            return cur, DOUBLE
        if fn in _BINARY:
            op = _BINARY[fn][1]
            (ak, a), (bk, b) = as_double(args[0]), as_double(args[1])
            dst = a if ak == REG else b
            emit(op, dst, ak, a, bk, b)
            if ak == REG and bk == REG:
                release(b)
            return dst, DOUBLE
        if fn in _UNARY:
            _, r = as_double(args[0])
            emit(_UNARY[fn][1], r, REG, r, 0, 0)
            return r, DOUBLE
        # timeconvert: the argument as long, then TimeUnit.convert
        x = args[0]
        if isinstance(x, Expr):
            r, t = gen(x)
            if t == DOUBLE:
                emit(L.PA_EXPR_D2L, r, REG, r, 0, 0)
        else:
            r = load(x[1], L.PA_EXPR_LONG)
        src, dst = TIME_UNITS[args[1][1].upper()], TIME_UNITS[args[2][1].upper()]
        if src < dst:
            emit(L.PA_EXPR_TCONV_DIV, r, REG, r, I64, dst // src)
        elif src > dst:
            emit(L.PA_EXPR_TCONV_MUL, r, REG, r, I64, src // dst)
        return r, LONG

    validate(expr)
    _, t = gen(expr)
    return Program(t, ops, columns)


def java_d2l(x):
    """Java's (long) cast of doubles: NaN -> 0, saturating at Long.MIN_VALUE / MAX_VALUE, else truncation."""
    x = np.asarray(x, dtype=np.float64)
    nan, hi, lo = np.isnan(x), x >= 2.0**63, x <= -2.0**63
    safe = np.where(nan | hi | lo, 0.0, x)
    out = np.trunc(safe).astype(np.int64)
    return np.where(hi, LONG_MAX, np.where(lo, LONG_MIN, out)).astype(np.int64)


def run_program(prog, column_values):
    """The program over numpy arrays, operation by operation as the device runs it. column_values: one array per
    prog.columns entry (INT / LONG as integers, FLOAT / DOUBLE as floats). float64 + - * /, np.fmod, np.floor,
    np.ceil and np.abs are the IEEE operations Java performs."""
    regs, last = {}, None

    def opnd(kind, v):
        return regs[v] if kind == L.PA_EXPR_ARG_REG else (np.float64(v) if kind == L.PA_EXPR_ARG_F64 else np.int64(v))
    with np.errstate(all="ignore"):
        for op, dst, ak, a, bk, b in prog.ops:
            if op == L.PA_EXPR_LOAD_COL:
                v = np.asarray(column_values[a])
                if b == L.PA_EXPR_DOUBLE:
                    out = v.astype(np.float64)  # ((double) of an int / long; a float widens)
                else:
                    out = java_d2l(v) if v.dtype.kind == "f" else v.astype(np.int64)
            elif op == L.PA_EXPR_ADD:
                out = opnd(ak, a) + opnd(bk, b)
            elif op == L.PA_EXPR_SUB:
                out = opnd(ak, a) - opnd(bk, b)
            elif op == L.PA_EXPR_MUL:
                out = opnd(ak, a) * opnd(bk, b)
            elif op == L.PA_EXPR_DIV:
                out = np.divide(opnd(ak, a), opnd(bk, b))
            elif op == L.PA_EXPR_MOD:
                out = np.fmod(opnd(ak, a), opnd(bk, b))
            elif op == L.PA_EXPR_ABS:
                out = np.abs(opnd(ak, a))
            elif op == L.PA_EXPR_CEIL:
                out = np.ceil(opnd(ak, a))
            elif op == L.PA_EXPR_FLOOR:
                out = np.floor(opnd(ak, a))
            elif op == L.PA_EXPR_D2L:
                out = java_d2l(opnd(ak, a))
            elif op == L.PA_EXPR_L2D:
                out = np.asarray(opnd(ak, a)).astype(np.float64)
            elif op == L.PA_EXPR_TCONV_DIV:
                x, m = np.asarray(opnd(ak, a), dtype=np.int64), np.int64(b)
                out = x // m + ((x % m != 0) & (x < 0))  # (floor -> truncation toward zero)
            elif op == L.PA_EXPR_TCONV_MUL:
                x, m = np.asarray(opnd(ak, a), dtype=np.int64), np.int64(b)
                over = np.int64(LONG_MAX // int(b))
                out = np.where(x > over, LONG_MAX, np.where(x < -over, LONG_MIN, x * m)).astype(np.int64)
            else:
                raise ValueError("unknown opcode %r" % (op,))
            regs[dst] = last = np.asarray(out, dtype=np.float64 if np.asarray(out).dtype.kind == "f" else np.int64)
    return last


def evaluate(expr, columns):
    """np.ndarray (float64 for a DOUBLE expression, int64 for a LONG one): the expression over `columns`, a mapping
    column name -> array of values. The restatement the tests compare the GPU with."""
    prog = lower(expr)
    return run_program(prog, [np.asarray(columns[c]) for c in prog.columns])


def fill_spec(programs, columns_ids, agg_expr, group_by_expr):
    """The pa_expr_spec of a query: programs (Program list over one shared column table), that table's column ids, and
    the expression index (or -1) of every GPU aggregation and group-by position."""
    spec = L.ExprSpec()
    spec.num_exprs, spec.num_columns = len(programs), len(columns_ids)
    for c, cid in enumerate(columns_ids):
        spec.columns[c] = cid
    for i in range(L.PA_MAX_AGGS):
        spec.agg_expr[i] = agg_expr[i] if i < len(agg_expr) else -1
    for j in range(L.PA_MAX_GROUP_BY):
        spec.group_by_expr[j] = group_by_expr[j] if j < len(group_by_expr) else -1

    def imm(kind, v):
        if kind == L.PA_EXPR_ARG_F64:
            return 0, struct.unpack("<q", struct.pack("<d", float(v)))[0]
        if kind == L.PA_EXPR_ARG_I64:
            return 0, int(v)
        return int(v), 0
    for x, prog in enumerate(programs):
        p = spec.exprs[x]
        p.result_type = L.PA_EXPR_DOUBLE if prog.result_type == DOUBLE else L.PA_EXPR_LONG
        p.num_ops = len(prog.ops)
        for o, (op, dst, ak, a, bk, b) in enumerate(prog.ops):
            d = p.ops[o]
            d.op, d.dst, d.a_kind, d.b_kind = op, dst, ak, bk
            d.a, d.a_imm = imm(ak, a)
            d.b, d.b_imm = imm(bk, b) if op != L.PA_EXPR_LOAD_COL else (int(b), 0)
    return spec
