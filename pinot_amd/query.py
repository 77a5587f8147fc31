"""Query model for the hot path (mirror of pinot-core's QueryContext / FilterContext / predicates) and a
parser for the SQL subset the reference's query tests use on this path:

  SELECT agg(col) [FILTER (WHERE filter)] [AS alias], ... FROM t [WHERE filter] [GROUP BY c1, ...]
  [ORDER BY x [ASC|DESC], ...] [LIMIT n] [OPTION(k=v, ...)]
  (agg(col) FILTER (WHERE f): the aggregation over the docs matching WHERE AND f; Aggregation.filter)
  SELECT col, ... | * FROM t [WHERE filter] [ORDER BY c1 [ASC|DESC], ...] [LIMIT [offset,] n | LIMIT n OFFSET m]
  (a selection: Query.is_selection; SelectionOnlyOperator / SelectionOrderByOperator on the server)
  SELECT DISTINCT c1, c2, ... | DISTINCT(c) FROM t [WHERE filter] [ORDER BY ci [ASC|DESC], ...] [LIMIT n]
  (Query.is_distinct; DistinctOperator on the server. ORDER BY columns must be among the DISTINCT columns)

filter: AND / OR / NOT / ( ) over  col = v | col != v | col <> v | col < v | col <= v | col > v | col >= v |
        col BETWEEN a AND b | col IN (...) | col NOT IN (...) | REGEXP_LIKE(col, 'regex') | col [NOT] LIKE 'pattern'
An aggregation argument (of SUM / MIN / MAX / AVG / MINMAXRANGE) and a GROUP BY item (also in the select list and in
ORDER BY) may be a transform expression (Expr): function calls fn(arg, ...), infix + - * / % (Calcite's plus / minus /
times / divide / mod; * / % bind over + -, left-associative), parentheses, columns and literals. A plain column stays a str.
REGEXP_LIKE / LIKE become RegexpLikePredicate as in RequestContextUtils.java:231-236 (LIKE through likeToRegexpLike).
Comparison predicates become RangePredicate exactly as the reference's RequestContextUtils does
(pinot-common/.../request/context/RequestContextUtils.java: >, >=, <, <=, BETWEEN -> RANGE).
Aggregations: COUNT(*), SUM, MIN, MAX, AVG, MINMAXRANGE, DISTINCTCOUNT, DISTINCTSUM, DISTINCTAVG, DISTINCTCOUNTHLL(col[, log2m]), DISTINCTCOUNTRAWHLL(col[, log2m]) and their *MV
forms; PERCENTILE<digits>(col), PERCENTILE<digits>MV(col), PERCENTILE(col, p), PERCENTILEMV(col, p);
FIRSTWITHTIME(dataCol, timeCol, 'dataType') and LASTWITHTIME(...) (any case, with or without underscores);
VAR_POP / VAR_SAMP / STDDEV_POP / STDDEV_SAMP (col) and COVAR_POP / COVAR_SAMP (col1, col2) (any case, with or without
underscores).
"""
import decimal
import re
from dataclasses import dataclass, field, replace as dataclasses_replace
from typing import List, Optional, Tuple

DEFAULT_HLL_LOG2M = 8          # CommonConstants.Helix.DEFAULT_HYPERLOGLOG_LOG2M
DEFAULT_NUM_GROUPS_LIMIT = 100_000   # InstancePlanMakerImplV2.DEFAULT_NUM_GROUPS_LIMIT
DEFAULT_MIN_SERVER_GROUP_TRIM_SIZE = 5000   # GroupByUtils.DEFAULT_MIN_NUM_GROUPS
UNBOUNDED = "*"                # RangePredicate.UNBOUNDED


# ------------------------------------------------------------------ predicates (pinot-common request/context)
@dataclass(frozen=True)
class EqPredicate:
    column: str
    value: object


@dataclass(frozen=True)
class NotEqPredicate:
    column: str
    value: object


@dataclass(frozen=True)
class InPredicate:
    column: str
    values: Tuple


@dataclass(frozen=True)
class NotInPredicate:
    column: str
    values: Tuple


@dataclass(frozen=True)
class RangePredicate:
    column: str
    lower: object = UNBOUNDED
    lower_inclusive: bool = False
    upper: object = UNBOUNDED
    upper_inclusive: bool = False


@dataclass(frozen=True)
class RegexpLikePredicate:
    """REGEXP_LIKE(col, pattern): a value matches when the pattern is found in it (Matcher.find(),
    RegexpLikePredicateEvaluatorFactory.java); LIKE arrives converted by like_to_regexp."""
    column: str
    pattern: str


def like_to_regexp(like):
    """RegexpPatternConverterUtils.likeToRegexpLike, restated from its test vectors (RegexpPatternConverterUtilsTest.java):
    leading / trailing '%' runs drop the '^' / '$' anchor, '%' -> '.*', '_' -> '.', a backslash escapes the next
    character (a trailing lone backslash is a literal one), regex metacharacters are escaped."""
    n = len(like)
    start, end = 0, n
    while start < end and like[start] == "%":
        start += 1
    while end > start and like[end - 1] == "%" and not (end - 2 >= start and like[end - 2] == "\\"):
        end -= 1
    out = ["^"] if start == 0 else []
    i = start
    while i < end:
        c = like[i]
        if c == "\\":
            if i + 1 < end:
                out.append("\\" + like[i + 1])
                i += 2
                continue
            out.append("\\\\")
        elif c == "%":
            out.append(".*")
        elif c == "_":
            out.append(".")
        elif c in ".^$*+?()[]{}|":
            out.append("\\" + c)
        else:
            out.append(c)
        i += 1
    if end == n:
        out.append("$")
    return "".join(out)


@dataclass(frozen=True)
class And:
    children: Tuple


@dataclass(frozen=True)
class Or:
    children: Tuple


@dataclass(frozen=True)
class Not:
    child: object


@dataclass(frozen=True)
class BoolFilter:
    """A constant filter (the boolean literal expression the reference's filter optimizers produce: TRUE becomes
    MatchAllFilterOperator, FALSE EmptyFilterOperator)."""
    value: bool


@dataclass(frozen=True)
class Comparison:
    """`a = b` / `a != b` where a side is not a plain column-vs-literal predicate (literal = literal, column = column):
    folded by IdenticalPredicateFilterOptimizer / constant evaluation (optimizer.py); each side ("id"|"lit", text)."""
    lhs: Tuple
    op: str
    rhs: Tuple


PREDICATES = (EqPredicate, NotEqPredicate, InPredicate, NotInPredicate, RangePredicate, RegexpLikePredicate)


# AggregationFunctionType names the hot path runs: single-value functions and their multi-value (*MV) forms, which
# aggregate every value of a multi-value column (SumMVAggregationFunction, CountMVAggregationFunction, ...)
SUPPORTED_FUNCTIONS = ("SUM", "MIN", "MAX", "AVG", "DISTINCTCOUNTHLL", "DISTINCTCOUNTRAWHLL", "MINMAXRANGE", "DISTINCTCOUNT",
                       "DISTINCTCOUNTBITMAP", "DISTINCTCOUNTBITMAPMV",
                       "DISTINCTSUM", "DISTINCTAVG",
                       "COUNTMV", "SUMMV", "MINMV", "MAXMV", "AVGMV", "DISTINCTCOUNTHLLMV", "DISTINCTCOUNTRAWHLLMV",
                       "MINMAXRANGEMV",
                       "DISTINCTCOUNTMV", "DISTINCTSUMMV", "DISTINCTAVGMV")
# BaseDistinctAggregateAggregationFunction subclasses: the intermediate result is the set of distinct values (one
# presence accumulator on the GPU); they differ only in extractFinalResult (size / sum / average)
DISTINCT_SET_FUNCTIONS = ("DISTINCTCOUNT", "DISTINCTSUM", "DISTINCTAVG", "DISTINCTCOUNTBITMAP", "DISTINCTCOUNTMV",
                          "DISTINCTCOUNTBITMAPMV", "DISTINCTSUMMV",
                          "DISTINCTAVGMV")


# DistinctCountBitmapAggregationFunction: the same value presence per group, reported as the set of the values' Java
# hash codes (its RoaringBitmap: java_hash.py), so equal hash codes count once
BITMAP_FUNCTIONS = ("DISTINCTCOUNTBITMAP", "DISTINCTCOUNTBITMAPMV")

# HyperLogLog functions: one register set per group (DistinctCountHLLAggregationFunction); the RAW forms differ only in
# the final result, the serialized registers (DistinctCountRawHLLAggregationFunction: SerializedHLL.toString, the hex
# of HyperLogLog.getBytes)
HLL_FUNCTIONS = ("DISTINCTCOUNTHLL", "DISTINCTCOUNTHLLMV", "DISTINCTCOUNTRAWHLL", "DISTINCTCOUNTRAWHLLMV")


# PercentileAggregationFunction / PercentileMVAggregationFunction: the intermediate result is every aggregated value (a
# DoubleArrayList; here a value histogram, engine.ValueHistogram), the final result the value at the percentile's rank
PERCENTILE_FUNCTIONS = ("PERCENTILE", "PERCENTILEMV")
_PERCENTILE_ONE_ARG = re.compile(r"(\d+)(MV)?$")


# FirstWithTimeAggregationFunction / LastWithTimeAggregationFunction: the intermediate result is the pair (value, time)
# of the group's winning doc (engine.ValueTimePair), the final result its value. The declared data types the factory
# takes (AggregationFunctionFactory.java:224-252, :324-350) and its names in messages
WITH_TIME_FUNCTIONS = ("FIRSTWITHTIME", "LASTWITHTIME")
WITH_TIME_TYPES = ("BOOLEAN", "INT", "LONG", "FLOAT", "DOUBLE", "STRING")
_WITH_TIME_LABEL = {"FIRSTWITHTIME": ("FIRST_WITH_TIME", "firstWithTime"), "LASTWITHTIME": ("LAST_WITH_TIME", "lastWithTime")}
_DATA_TYPES = ("INT", "LONG", "FLOAT", "DOUBLE", "BIG_DECIMAL", "BOOLEAN", "TIMESTAMP", "STRING", "JSON", "BYTES", "STRUCT",
               "MAP", "LIST", "UNKNOWN")


# VarianceAggregationFunction (VARPOP / VARSAMP / STDDEVPOP / STDDEVSAMP: the intermediate result is engine.VarianceTuple)
# and CovarianceAggregationFunction (COVARPOP / COVARSAMP: engine.CovarianceTuple), factory cases
# AggregationFunctionFactory.java:413-428; the functions of one family over the same argument(s) differ only in
# extractFinalResult
VARIANCE_FUNCTIONS = ("VARPOP", "VARSAMP", "STDDEVPOP", "STDDEVSAMP")
COVARIANCE_FUNCTIONS = ("COVARPOP", "COVARSAMP")
MOMENT_FUNCTIONS = VARIANCE_FUNCTIONS + COVARIANCE_FUNCTIONS
# the names in the constructors' messages (VarianceAggregationFunction.getFunctionName)
_VARIANCE_LABEL = {"VARPOP": "VAR_POP", "VARSAMP": "VAR_SAMP", "STDDEVPOP": "STD_DEV_POP", "STDDEVSAMP": "STD_DEV_SAMP"}


def java_double_string(x):
    """Double.toString of a finite double: the shortest digits that round-trip (Python's repr gives the same digits),
    plain notation from 1e-3 up to 1e7, computerized scientific notation (1.0E-5) outside."""
    x = float(x)
    if x == 0 or 1e-3 <= abs(x) < 1e7:
        return repr(x)  # (repr is plain from 1e-4 up to 1e16)
    sign, digits, exp = decimal.Decimal(repr(x)).as_tuple()
    digits = "".join(map(str, digits)).rstrip("0") or "0"
    exp10 = len(decimal.Decimal(repr(x)).as_tuple()[1]) + exp - 1
    return "%s%s.%sE%d" % ("-" if sign else "", digits[0], digits[1:] or "0", exp10)


def filter_string(f):
    """FilterContext.toString (FilterContext.java:136-167) over the predicates' toString: EqPredicate.java:64
    `c = 'v'`, NotEqPredicate.java:63 `c != 'v'`, InPredicate.java:58 / NotInPredicate.java:58 `c IN ('a','b')`,
    RangePredicate.java:130-142, RegexpLikePredicate.java:72; AND / OR in parentheses, `(NOT x)`, constants true /
    false. Values print as the query spelled them. Pinned by FilteredAggregationsTest.java:219 and :226."""
    if isinstance(f, (And, Or)):
        return "(" + (" AND " if isinstance(f, And) else " OR ").join(filter_string(c) for c in f.children) + ")"
    if isinstance(f, Not):
        return "(NOT %s)" % filter_string(f.child)
    if isinstance(f, BoolFilter):
        return "true" if f.value else "false"
    if isinstance(f, EqPredicate):
        return "%s = '%s'" % (f.column, f.value)
    if isinstance(f, NotEqPredicate):
        return "%s != '%s'" % (f.column, f.value)
    if isinstance(f, (InPredicate, NotInPredicate)):
        return "%s %s (%s)" % (f.column, "IN" if isinstance(f, InPredicate) else "NOT IN",
                               ",".join("'%s'" % v for v in f.values))
    if isinstance(f, RangePredicate):
        if f.lower == UNBOUNDED:
            return "%s %s '%s'" % (f.column, "<=" if f.upper_inclusive else "<", f.upper)
        if f.upper == UNBOUNDED:
            return "%s %s '%s'" % (f.column, ">=" if f.lower_inclusive else ">", f.lower)
        if f.lower_inclusive and f.upper_inclusive:
            return "%s BETWEEN '%s' AND '%s'" % (f.column, f.lower, f.upper)
        return "(%s %s '%s' AND %s %s '%s')" % (f.column, ">=" if f.lower_inclusive else ">", f.lower,
                                                f.column, "<=" if f.upper_inclusive else "<", f.upper)
    if isinstance(f, RegexpLikePredicate):
        return "regexp_like(%s,'%s')" % (f.column, f.pattern)
    raise ValueError("no FilterContext string for %r" % (f,))


def filter_columns(f, into):
    """Adds the columns a filter tree reads to the set or list `into`."""
    if f is None:
        return into
    for c in getattr(f, "children", ()) or ():
        filter_columns(c, into)
    if getattr(f, "child", None) is not None:
        filter_columns(f.child, into)
    col = getattr(f, "column", None)
    if col is not None and col not in into:
        into.add(col) if isinstance(into, set) else into.append(col)
    return into


@dataclass(frozen=True)
class Expr:
    """A transform function call (pinot-common FunctionContext inside an ExpressionContext): fn is the canonical
    function name (lower case, underscores removed: `add`, `plus` for infix +, `timeconvert`), args are Expr nodes and
    the leaves ("id", column name) / ("lit", text as written)."""
    fn: str
    args: Tuple

    def __str__(self):
        """ExpressionContext.toString: fn(arg,arg) without spaces, literals in single quotes (LiteralContext.toString)
        — the result column name of an aggregation over it (`max(add(column1,column9))`,
        ForwardIndexDisabledSingleValueQueriesTest.java:1604) and the group-key column name."""
        return "%s(%s)" % (self.fn, ",".join(
            str(a) if isinstance(a, Expr) else (a[1] if a[0] == "id" else "'%s'" % a[1]) for a in self.args))

    def columns(self, into=None):
        """The columns the expression reads, in first-use order."""
        into = [] if into is None else into
        for a in self.args:
            if isinstance(a, Expr):
                a.columns(into)
            elif a[0] == "id" and a[1] not in into:
                into.append(a[1])
        return into


def item_columns(item, into):
    """Adds the column(s) behind an aggregation argument or group-by item (a column name or an Expr) to `into`."""
    for c in (item.columns() if isinstance(item, Expr) else ([item] if item else [])):
        if c not in into:
            into.add(c) if isinstance(into, set) else into.append(c)
    return into


# names that start a transform expression in a select list or ORDER BY (every other call there is an aggregation):
# TransformFunctionType's arithmetic, math and date-time functions, whether the engine runs them or refuses them
TRANSFORM_NAMES = frozenset((
    "add plus sub minus mult times div divide mod abs ceil ceiling floor exp ln log log2 log10 sign sqrt power pow "
    "rounddecimal truncate least greatest timeconvert datetimeconvert datetrunc cast case year month day hour minute "
    "second tojsonmapstr jsonextractscalar arraylength valuein upper lower concat substr").split())
_INFIX = {"+": "plus", "-": "minus", "*": "times", "/": "divide", "%": "mod"}
# an identifier token spelled like one of these is never the left operand of a subtraction
_KEYWORDS = frozenset("AND OR NOT BETWEEN IN LIKE WHERE BY SELECT LIMIT OFFSET TOP DISTINCT AS WHEN THEN ELSE".split())


def base_function(fn):
    """Merge/extract semantics of a function: the *MV forms behave like their single-value form, COUNTMV like COUNT."""
    return fn[:-2] if fn.endswith("MV") else fn


@dataclass(frozen=True)
class Aggregation:
    function: str              # COUNT SUM MIN MAX AVG DISTINCTCOUNTHLL and the *MV forms
    column: object = None      # the column's name, or the transform expression (Expr) it aggregates
    log2m: int = DEFAULT_HLL_LOG2M
    percentile: float = -1.0   # PERCENTILE / PERCENTILEMV: 0..100
    version: int = 0           # PERCENTILE spelling: 0 = PERCENTILE<digits>(col), 1 = PERCENTILE(col, p)
    filter: object = None      # AGG(col) FILTER (WHERE filter): the filter tree, as written (no optimizer rewrite)
    time_column: object = None  # FIRSTWITHTIME / LASTWITHTIME: the time column's name (or the Expr written there)
    data_type: str = ""        # FIRSTWITHTIME / LASTWITHTIME: the declared type, upper case (WITH_TIME_TYPES)
    column2: object = None     # COVARPOP / COVARSAMP: the second argument (a column's name, or the Expr written there)

    @property
    def result_name(self):
        """AggregationFunctionUtils.getResultColumnName (:412-418): the function's name, plus
        " FILTER(WHERE " + FilterContext.toString + ")" for a filtered aggregation."""
        if self.filter is not None:
            return "%s FILTER(WHERE %s)" % (dataclasses_replace(self, filter=None).result_name,
                                            filter_string(self.filter))
        return self.function_name

    @property
    def function_name(self):
        """AggregationFunction.getResultColumnName: lower-case function name + (column)."""
        if self.function == "COUNT":
            return "count(*)"
        if self.function in PERCENTILE_FUNCTIONS:
            # Percentile(MV)AggregationFunction.getResultColumnName: percentile50(c) / percentile50mv(c) for the
            # one-argument spelling, percentile(c, 50.0) / percentilemv(c, 50.0) (Double.toString) for the other
            mv = "mv" if self.function.endswith("MV") else ""
            if self.version == 0:
                return "percentile%d%s(%s)" % (int(self.percentile), mv, self.column)
            return "percentile%s(%s, %s)" % (mv, self.column, java_double_string(self.percentile))
        if self.function in WITH_TIME_FUNCTIONS:
            # lastwithtime(intColumn,timestampColumn,'INT') (LastWithTimeQueriesTest.java:239-244): no spaces, the type
            # literal upper-cased in quotes
            return "%s(%s,%s,'%s')" % (self.function.lower(), self.column, self.time_column, self.data_type)
        if self.function in COVARIANCE_FUNCTIONS:
            # CovarianceAggregationFunction.getResultColumnName (:72-74): covarpop(x,y), no space
            return "%s(%s,%s)" % (self.function.lower(), self.column, self.column2)
        return "%s(%s)" % (self.function.lower(), self.column)


@dataclass(frozen=True)
class OrderBy:
    expr: object               # Aggregation or column name
    asc: bool = True


@dataclass
class Query:
    aggregations: List[Aggregation]
    aliases: List[Optional[str]] = field(default_factory=list)
    filter: object = None
    group_by: List[object] = field(default_factory=list)   # column names and transform expressions (Expr)
    order_by: List[OrderBy] = field(default_factory=list)
    limit: int = 10
    options: dict = field(default_factory=dict)
    select_columns: List[str] = field(default_factory=list)
    num_select_aggs: int = -1   # aggregations after this index are ORDER BY-only
    offset: int = 0             # LIMIT offset, n / LIMIT n OFFSET offset (selections: the broker drops these rows)
    select_star: bool = False   # SELECT *: every physical column of the schema
    distinct: bool = False      # SELECT DISTINCT select_columns (QueryContextUtils.isDistinctQuery)

    @property
    def is_selection(self):
        """No aggregation, no GROUP BY, no DISTINCT: SELECT columns / * [ORDER BY ...]
        (QueryContextUtils.isSelectionQuery)."""
        return not self.aggregations and not self.group_by and not self.distinct

    @property
    def is_distinct(self):
        """SELECT DISTINCT columns: neither a selection nor an aggregation."""
        return bool(self.distinct)

    @property
    def num_groups_limit(self):
        return int(self.options.get("numGroupsLimit", DEFAULT_NUM_GROUPS_LIMIT))

    @property
    def min_server_group_trim_size(self):
        return int(self.options.get("minServerGroupTrimSize", DEFAULT_MIN_SERVER_GROUP_TRIM_SIZE))

    def columns(self):
        cols = set()
        for g in self.group_by:
            item_columns(g, cols)
        for a in self.aggregations:
            item_columns(a.column, cols)
            item_columns(a.time_column, cols)
            item_columns(a.column2, cols)
            filter_columns(a.filter, cols)
        if self.is_selection or self.is_distinct:
            cols.update(self.select_columns)
            cols.update(o.expr for o in self.order_by if isinstance(o.expr, str))

        def walk(f):
            if f is None:
                return
            if isinstance(f, (And, Or)):
                for c in f.children:
                    walk(c)
            elif isinstance(f, Not):
                walk(f.child)
            elif hasattr(f, "column"):
                cols.add(f.column)
        walk(self.filter)
        return cols


# ------------------------------------------------------------------ SQL subset parser
_TOKEN = re.compile(r"\s*(?:(?P<num>-?\d+(?:\.\d+)?(?:[eE][-+]?\d+)?)|(?P<str>'(?:[^']|'')*')|"
                    r"(?P<qid>\"(?:[^\"]|\"\")*\")|"
                    r"(?P<op><>|!=|<=|>=|=|<|>|\(|\)|,|\*|\+|-|/|%)|(?P<id>[A-Za-z_][A-Za-z0-9_\.]*))")


def _tokenize(sql):
    pos, out = 0, []
    sql = sql.strip().rstrip(";")
    while pos < len(sql):
        m = _TOKEN.match(sql, pos)
        if not m or m.end() == pos:
            raise ValueError("cannot tokenize at: %r" % sql[pos:pos + 20])
        pos = m.end()
        if m.group("num") is not None:
            num = m.group("num")
            prev = out[-1] if out else (None, None)
            if num[0] == "-" and (prev[0] == "lit" or prev == ("op", ")") or
                                  (prev[0] == "id" and prev[1].upper() not in _KEYWORDS)):
                # `a -1`, `a-1`, `(a) -1`: a subtraction, not a negative literal after an operand
                out.append(("op", "-"))
                num = num[1:]
            out.append(("lit", num))
        elif m.group("str") is not None:
            out.append(("lit", m.group("str")[1:-1].replace("''", "'")))
        elif m.group("qid") is not None:  # "quoted identifier"
            out.append(("id", m.group("qid")[1:-1].replace('""', '"')))
        elif m.group("op") is not None:
            out.append(("op", m.group("op")))
        else:
            out.append(("id", m.group("id")))
    return out


class _Parser:
    def __init__(self, sql):
        self.t = _tokenize(sql)
        self.i = 0

    def peek(self, k=0):
        return self.t[self.i + k] if self.i + k < len(self.t) else (None, None)

    def kw(self, word):
        tok = self.peek()
        if tok[0] == "id" and tok[1].upper() == word:
            self.i += 1
            return True
        return False

    def expect_kw(self, word):
        if not self.kw(word):
            raise ValueError("expected %s at token %r" % (word, self.peek()))

    def op(self, sym):
        tok = self.peek()
        if tok[0] == "op" and tok[1] == sym:
            self.i += 1
            return True
        return False

    def expect_op(self, sym):
        if not self.op(sym):
            raise ValueError("expected %r at token %r" % (sym, self.peek()))

    def ident(self):
        tok = self.peek()
        if tok[0] != "id":
            raise ValueError("expected identifier at %r" % (tok,))
        self.i += 1
        return tok[1]

    def literal(self):
        tok = self.peek()
        if tok[0] != "lit":
            raise ValueError("expected literal at %r" % (tok,))
        self.i += 1
        return tok[1]

    # SELECT list item
    def aggregation(self):
        """One aggregation call, with its FILTER ( WHERE filter ) clause when one follows the closing parenthesis
        (every function form; the existing filter grammar)."""
        agg = self.aggregation_call()
        tok, nxt = self.peek(), self.peek(1)
        if tok[0] == "id" and tok[1].upper() == "FILTER":
            if nxt != ("op", "("):
                raise ValueError("FILTER clause: expected ( WHERE filter ) after FILTER, at token %r" % (nxt,))
            self.i += 2
            try:
                self.expect_kw("WHERE")
                f = self.filter_or()
                self.expect_op(")")
            except ValueError as e:
                raise ValueError("FILTER clause: %s" % e) from None
            agg = dataclasses_replace(agg, filter=f)
        return agg

    def aggregation_call(self):
        fn = self.ident().upper()
        self.expect_op("(")
        if self.kw("DISTINCT"):
            # CalciteSqlParser.java:761-772: COUNT / SUM / AVG (DISTINCT x) -> DISTINCTCOUNT / DISTINCTSUM / DISTINCTAVG,
            # any other aggregation on DISTINCT is refused
            if fn not in ("COUNT", "SUM", "AVG"):
                raise ValueError("Function '%s' on DISTINCT is not supported." % fn)
            fn = "DISTINCT" + fn
        elif fn == "COUNT":
            self.expect_op("*")
            self.expect_op(")")
            return Aggregation("COUNT")
        if fn.startswith("PERCENTILE"):
            return self.percentile(fn)
        if fn.replace("_", "") in WITH_TIME_FUNCTIONS:
            return self.with_time(fn.replace("_", ""))
        if fn.replace("_", "") in MOMENT_FUNCTIONS:
            return self.moments(fn.replace("_", ""))
        col = self.item()
        log2m = DEFAULT_HLL_LOG2M
        if self.op(","):
            log2m = int(self.literal())
        self.expect_op(")")
        if fn not in SUPPORTED_FUNCTIONS:
            raise ValueError("unsupported aggregation %s" % fn)
        return Aggregation(fn, col, log2m)

    # ---- transform expressions
    def item(self):
        """An aggregation argument or group-by item: a column name (str), or an Expr."""
        e = self.expr()
        if isinstance(e, Expr):
            return e
        if e[0] != "id":
            raise ValueError("expected a column or an expression, not the literal %r" % (e[1],))
        return e[1]

    def expr(self):
        left = self.term()
        while self.peek() in (("op", "+"), ("op", "-")):
            sym = self.peek()[1]
            self.i += 1
            left = Expr(_INFIX[sym], (left, self.term()))
        return left

    def term(self):
        left = self.primary()
        while self.peek() in (("op", "*"), ("op", "/"), ("op", "%")):
            sym = self.peek()[1]
            self.i += 1
            left = Expr(_INFIX[sym], (left, self.primary()))
        return left

    def primary(self):
        tok, nxt = self.peek(), self.peek(1)
        if self.op("("):
            e = self.expr()
            self.expect_op(")")
            return e
        if tok[0] == "lit":
            self.i += 1
            return tok
        if tok[0] != "id":
            raise ValueError("expected a column, literal or function call at %r" % (tok,))
        self.i += 1
        name = tok[1].replace("_", "").lower()
        if name == "case" and nxt != ("op", "("):
            # CASE ... END: kept opaque (the engine refuses it); nested CASEs balance
            depth = 1
            while depth:
                t = self.peek()
                if t[0] is None:
                    raise ValueError("CASE without END")
                self.i += 1
                if t[0] == "id":
                    depth += (t[1].upper() == "CASE") - (t[1].upper() == "END")
            return Expr("case", ())
        if nxt != ("op", "("):
            return tok
        self.i += 1
        args = []
        if not self.op(")"):
            while True:
                args.append(self.expr())
                if name == "cast" and self.kw("AS"):
                    args.append(("lit", self.ident()))
                if not self.op(","):
                    break
            self.expect_op(")")
        return Expr(name, tuple(args))

    def is_aggregation_call(self):
        """The next tokens start an aggregation: name( where the name is no transform function."""
        tok, nxt = self.peek(), self.peek(1)
        return tok[0] == "id" and nxt == ("op", "(") and tok[1].replace("_", "").lower() not in TRANSFORM_NAMES

    def moments(self, fn):
        """VARPOP / VARSAMP / STDDEVPOP / STDDEVSAMP take exactly one argument (verifySingleArgument,
        VarianceAggregationFunction.java:51), COVARPOP / COVARSAMP two (CovarianceAggregationFunction.java:57-61)."""
        args = []
        if not self.op(")"):
            while True:
                args.append(self.item())
                if not self.op(","):
                    break
            self.expect_op(")")
        if fn in VARIANCE_FUNCTIONS:
            if len(args) != 1:
                raise ValueError("%s expects 1 argument, got: %d" % (_VARIANCE_LABEL[fn], len(args)))
            return Aggregation(fn, args[0])
        if len(args) != 2:
            raise ValueError("%s expects 2 arguments, got: %d" % (fn, len(args)))
        return Aggregation(fn, args[0], column2=args[1])

    def with_time(self, fn):
        """AggregationFunctionFactory.java:224-252 (FIRSTWITHTIME) and :324-350 (LASTWITHTIME): exactly three arguments,
        the third a literal naming one of WITH_TIME_TYPES in any case; the factory's messages."""
        label, usage = _WITH_TIME_LABEL[fn]
        usage = "The function can be used as %s(dataColumn, timeColumn, 'dataType')" % usage
        args = []
        if not self.op(")"):
            while True:
                args.append(self.expr())
                if not self.op(","):
                    break
            self.expect_op(")")
        if len(args) != 3:
            raise ValueError("%s expects 3 arguments, got: %d. %s" % (label, len(args), usage))
        lit = args[2]
        if isinstance(lit, Expr) or lit[0] != "lit":
            raise ValueError("%s expects the 3rd argument to be literal, got: %s. %s"
                             % (label, "FUNCTION" if isinstance(lit, Expr) else "IDENTIFIER", usage))
        dtype = str(lit[1]).upper()
        if dtype not in _DATA_TYPES:  # (DataType.valueOf)
            raise ValueError("No enum constant org.apache.pinot.spi.data.FieldSpec.DataType.%s" % dtype)
        if dtype not in WITH_TIME_TYPES:
            raise ValueError("Unsupported data type for %s: %s" % (label, dtype))

        def operand(e):
            if isinstance(e, Expr):
                return e
            if e[0] != "id":
                raise ValueError("expected a column or an expression, not the literal %r" % (e[1],))
            return e[1]
        return Aggregation(fn, operand(args[0]), time_column=operand(args[1]), data_type=dtype)

    def percentile(self, fn):
        """AggregationFunctionFactory.java:66-175 for the exact percentile: PERCENTILE<digits>(col) and
        PERCENTILE<digits>MV(col) (version 0), PERCENTILE(col, p) and PERCENTILEMV(col, p) (version 1, p a number or a
        quoted number); every other PERCENTILE* name (EST, TDIGEST, KLL, RAW...) is not on this path."""
        rest = fn[len("PERCENTILE"):]
        col = self.item()
        args = []
        while self.op(","):
            args.append(self.literal())
        self.expect_op(")")
        one = _PERCENTILE_ONE_ARG.match(rest)
        if not args and one:
            p, version, mv = float(int(one.group(1))), 0, one.group(2)
        elif len(args) == 1 and rest in ("", "MV"):
            p, version, mv = float(args[0]), 1, rest
        else:
            raise ValueError("unsupported aggregation %s" % fn)
        if not 0 <= p <= 100:  # (Preconditions.checkArgument in the factory; NaN fails it too)
            raise ValueError("Invalid percentile: %s" % java_double_string(p))
        return Aggregation("PERCENTILEMV" if mv else "PERCENTILE", col, percentile=p, version=version)

    def filter_or(self):
        left = self.filter_and()
        items = [left]
        while self.kw("OR"):
            items.append(self.filter_and())
        return items[0] if len(items) == 1 else Or(tuple(items))

    def filter_and(self):
        items = [self.filter_not()]
        while self.kw("AND"):
            items.append(self.filter_not())
        return items[0] if len(items) == 1 else And(tuple(items))

    def filter_not(self):
        if self.kw("NOT"):
            return Not(self.filter_not())
        if self.op("("):
            f = self.filter_or()
            self.expect_op(")")
            return f
        return self.predicate()

    def predicate(self):
        tok, nxt = self.peek(), self.peek(1)
        if tok[0] == "id" and tok[1].upper() in ("TRUE", "FALSE") and not (nxt[0] == "op" and nxt[1] in
                                                                           ("=", "!=", "<>", "<", "<=", ">", ">=")):
            self.i += 1
            return BoolFilter(tok[1].upper() == "TRUE")
        if tok[0] == "lit" or (tok[0] == "id" and nxt[0] == "op" and nxt[1] in ("=", "!=", "<>") and
                               self.peek(2)[0] == "id" and self.peek(2)[1].upper() not in ("TRUE", "FALSE")):
            # literal = literal, column = column: a comparison the filter optimizers fold (optimizer.py)
            lhs = (tok[0], tok[1])
            self.i += 1
            op = self.peek()
            if op[0] != "op" or op[1] not in ("=", "!=", "<>"):
                raise ValueError("expected = or != after %r" % (tok,))
            self.i += 1
            rhs = self.peek()
            if rhs[0] not in ("id", "lit"):
                raise ValueError("expected a literal or column at %r" % (rhs,))
            self.i += 1
            return Comparison(lhs, "=" if op[1] == "=" else "!=", (rhs[0], rhs[1]))
        if tok[0] == "id" and tok[1].upper() == "REGEXP_LIKE" and nxt == ("op", "("):
            self.i += 2
            col = self.ident()
            self.expect_op(",")
            pat = self.literal()
            self.expect_op(")")
            return RegexpLikePredicate(col, str(pat))
        col = self.ident()
        if self.kw("BETWEEN"):
            lo = self.literal()
            self.expect_kw("AND")
            hi = self.literal()
            return RangePredicate(col, lo, True, hi, True)
        negate = self.kw("NOT")
        if self.kw("LIKE"):
            f = RegexpLikePredicate(col, like_to_regexp(str(self.literal())))
            return Not(f) if negate else f
        if self.kw("IN"):
            self.expect_op("(")
            vals = [self.literal()]
            while self.op(","):
                vals.append(self.literal())
            self.expect_op(")")
            return NotInPredicate(col, tuple(vals)) if negate else InPredicate(col, tuple(vals))
        if negate:
            raise ValueError("NOT must be followed by IN or LIKE here")
        tok = self.peek()
        if tok[0] != "op":
            raise ValueError("expected comparison at %r" % (tok,))
        self.i += 1
        v = self.literal()
        return {
            "=": lambda: EqPredicate(col, v),
            "!=": lambda: NotEqPredicate(col, v),
            "<>": lambda: NotEqPredicate(col, v),
            "<": lambda: RangePredicate(col, UNBOUNDED, False, v, False),
            "<=": lambda: RangePredicate(col, UNBOUNDED, False, v, True),
            ">": lambda: RangePredicate(col, v, False, UNBOUNDED, False),
            ">=": lambda: RangePredicate(col, v, True, UNBOUNDED, False),
        }[tok[1]]()

    def parse(self):
        self.expect_kw("SELECT")
        aggs, aliases, plain_cols = [], [], []
        star = False
        # SELECT DISTINCT c1, c2 / SELECT DISTINCT(c): the DISTINCT columns are the select list
        distinct = self.kw("DISTINCT")
        paren = distinct and self.op("(")
        while True:
            tok, nxt = self.peek(), self.peek(1)
            if distinct and (tok[0] != "id" or (nxt[0] == "op" and nxt[1] == "(")):
                raise ValueError("DISTINCT takes plain columns (no aggregations, no *): %r" % (tok,))
            if self.op("*"):
                star = True
            elif not self.is_aggregation_call():
                plain_cols.append(self.item())  # group-by column or expression in the select list
                if self.peek()[0] == "id" and self.peek()[1].upper() == "FILTER":
                    raise ValueError("FILTER clause: it follows an aggregation, not the column %r" % plain_cols[-1])
            else:
                aggs.append(self.aggregation())
                aliases.append(self.ident() if self.kw("AS") else None)
            if not self.op(","):
                break
        if paren:
            if len(plain_cols) != 1:
                raise ValueError("DISTINCT(c) takes one column; write several as SELECT DISTINCT c1, c2")
            self.expect_op(")")
            if self.op(","):
                raise ValueError("DISTINCT(...) is the whole select list: no aggregation or column may follow it")
        self.expect_kw("FROM")
        self.ident()
        q = Query(aggregations=aggs, aliases=aliases, distinct=distinct)
        q.select_columns = plain_cols
        q.num_select_aggs = len(aggs)
        q.select_star = star
        if star and aggs:
            raise ValueError("SELECT * next to aggregations")
        if self.kw("WHERE"):
            q.filter = self.filter_or()
        if self.kw("GROUP"):
            self.expect_kw("BY")
            q.group_by.append(self.item())
            while self.op(","):
                q.group_by.append(self.item())
        if self.kw("ORDER"):
            self.expect_kw("BY")
            while True:
                tok, nxt = self.peek(), self.peek(1)
                if self.is_aggregation_call():
                    expr = self.aggregation()
                    if expr not in aggs:  # ORDER BY aggregation absent from the select list: computed, not output
                        aggs.append(expr)
                        aliases.append(None)
                else:
                    name = self.item()
                    expr = name
                    for a, al in zip(aggs, aliases):
                        if al == name:
                            expr = a
                asc = True
                if self.kw("DESC"):
                    asc = False
                else:
                    self.kw("ASC")
                q.order_by.append(OrderBy(expr, asc))
                if not self.op(","):
                    break
        if self.kw("LIMIT"):
            q.limit = int(self.literal())
            if self.op(","):  # LIMIT offset, n
                q.offset, q.limit = q.limit, int(self.literal())
            elif self.kw("OFFSET"):
                q.offset = int(self.literal())
            if q.limit < 0 or q.offset < 0:
                raise ValueError("negative LIMIT / OFFSET")
        if self.kw("TOP"):
            q.limit = int(self.literal())
        if self.kw("OPTION"):
            self.expect_op("(")
            while True:
                k = self.ident()
                self.expect_op("=")
                tok = self.peek()
                self.i += 1
                q.options[k] = tok[1]
                if not self.op(","):
                    break
            self.expect_op(")")
        if self.peek()[0] is not None:
            raise ValueError("trailing tokens: %r" % (self.t[self.i:],))
        if distinct:
            # (the reference: "ORDER-BY columns should be included in the DISTINCT columns", and no aggregation or
            # GROUP BY next to DISTINCT; DistinctExecutorFactory looks ORDER BY expressions up in the DISTINCT list)
            if aggs or q.group_by:
                raise ValueError("DISTINCT next to aggregations or GROUP BY")
            for o in q.order_by:
                if o.expr not in plain_cols:
                    raise ValueError("ORDER BY column %r is not in the DISTINCT list" % (o.expr,))
        if aggs and (plain_cols or star) and not q.group_by:
            # (the reference: "... should appear in GROUP BY clause", CalciteSqlParser.validateGroupByClause)
            raise ValueError("plain columns next to aggregations without GROUP BY: %r" % (plain_cols or "*",))
        return q


def parse_sql(sql: str) -> Query:
    return _Parser(sql).parse()


def parse_filter(text: str):
    """A WHERE clause on its own (the filter tree parse_sql builds for it)."""
    p = _Parser(text)
    f = p.filter_or()
    if p.peek()[0] is not None:
        raise ValueError("trailing tokens: %r" % (p.t[p.i:],))
    return f


def query_columns(query):
    """Every column a query reads: filter leaves, group-by columns, aggregation columns."""
    names = []

    def walk(f):
        for c in getattr(f, "children", ()) or ():
            walk(c)
        if getattr(f, "child", None) is not None:
            walk(f.child)
        if getattr(f, "column", None) is not None and f.column not in names:
            names.append(f.column)
    if query.filter is not None:
        walk(query.filter)
    for n in list(query.group_by) + [c for a in query.aggregations for c in (a.column, a.time_column, a.column2) if c] + \
            (list(query.select_columns) if query.is_distinct else []):
        item_columns(n, names)
    for a in query.aggregations:
        filter_columns(a.filter, names)
    return names
