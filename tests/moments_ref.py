"""Doc-at-a-time restatement of the reference's statistical aggregations, and an exact evaluator.

VarianceAggregationFunction (VARPOP / VARSAMP / STDDEVPOP / STDDEVSAMP) and CovarianceAggregationFunction (COVARPOP /
COVARSAMP), in the reference's own order of floating-point operations:

  aggregation-only   per segment: count, sum and m2 updated per doc by computeIntermediateVariance
                     (VarianceAggregationFunction.java:80-121); covariance: the raw sums (CovarianceAggregationFunction
                     .java:95-110); the segments' tuples merged by VarianceTuple.apply / CovarianceTuple.apply
  group by           per doc VarianceTuple.apply(1, v, 0.0) into the group's tuple (:144-162); covariance apply(x, y, x*y, 1)
  final              extractFinalResult of both (:228-248, :186-203)

Values arrive as the doubles getDoubleValuesSV gives (float(v) of the stored value). Plain tuples: variance (count,
sum, m2), covariance (sum_x, sum_y, sum_xy, count), in the constructors' order.

The exact evaluator works on fractions.Fraction of the stored values: count, sum, m2 = sum (x - mean)^2 and the
covariance sums, without any rounding.
"""
import math
from fractions import Fraction


# ---------------------------------------------------------------- VarianceTuple / CovarianceTuple
def var_apply(t, count, s, m2):
    """VarianceTuple.apply(count, sum, m2) (:35-44) on the tuple t (or None: a new tuple)."""
    if t is None:
        return (count, s, m2)
    if count == 0:
        return t
    c0, s0, m0 = t
    curr_avg = 0.0 if c0 == 0 else s0 / c0
    delta = (s / count) - curr_avg
    return (c0 + count, s0 + s, m0 + (m2 + delta * delta * count * c0 / (count + c0)))


def var_merge(a, b):
    """VarianceTuple.apply(VarianceTuple) (:46-55)."""
    return var_apply(a, b[0], b[1], b[2])


def cov_apply(t, sx, sy, sxy, count):
    if t is None:
        return (sx, sy, sxy, count)
    return (t[0] + sx, t[1] + sy, t[2] + sxy, t[3] + count)


def cov_merge(a, b):
    return cov_apply(a, *b)


# ---------------------------------------------------------------- segments
def variance_segment(values):
    """aggregate (:80-115) over one segment's matching docs in docId order -> (count, sum, m2)."""
    count, s, m2 = 0, 0.0, 0.0
    for v in values:
        v = float(v)
        count += 1
        s += v
        if count > 1:
            t = count * v - s
            m2 += (t * t) / (count * (count - 1))
    return (count, s, m2)


def covariance_segment(xs, ys):
    sx = sy = sxy = 0.0
    n = 0
    for x, y in zip(xs, ys):
        x, y = float(x), float(y)
        sx += x
        sy += y
        sxy += x * y
        n += 1
    return (sx, sy, sxy, n)


def variance_table(segments):
    """Aggregation-only: segments = [values of the matching docs]; every segment with a holder contributes its tuple
    (a segment whose filter matches nothing still sets (0, 0.0, 0.0), which apply ignores)."""
    out = None
    for values in segments:
        t = variance_segment(values)
        out = t if out is None else var_merge(out, t)
    return out if out is not None else (0, 0.0, 0.0)


def covariance_table(segments):
    out = None
    for xs, ys in segments:
        t = covariance_segment(xs, ys)
        out = t if out is None else cov_merge(out, t)
    return out if out is not None else (0.0, 0.0, 0.0, 0)


def variance_groups(segments):
    """Group by: segments = [(keys, values)] of the matching docs -> {key: (count, sum, m2)} (per segment per doc
    apply(1, v, 0.0), then the segments' tuples merged in segment order)."""
    out = {}
    for keys, values in segments:
        seg = {}
        for k, v in zip(keys, values):
            seg[k] = var_apply(seg.get(k), 1, float(v), 0.0)
        for k, t in seg.items():
            out[k] = t if k not in out else var_merge(out[k], t)
    return out


def covariance_groups(segments):
    out = {}
    for keys, xs, ys in segments:
        seg = {}
        for k, x, y in zip(keys, xs, ys):
            x, y = float(x), float(y)
            seg[k] = cov_apply(seg.get(k), x, y, x * y, 1)
        for k, t in seg.items():
            out[k] = t if k not in out else cov_merge(out[k], t)
    return out


# ---------------------------------------------------------------- final results
def variance_final(fn, t):
    """VarianceAggregationFunction.extractFinalResult (:228-248); fn in VARPOP / VARSAMP / STDDEVPOP / STDDEVSAMP."""
    count, _, m2 = t
    sample, std = fn.endswith("SAMP"), fn.startswith("STDDEV")
    if count == 0 or (sample and count - 1 == 0):
        return -math.inf
    var = m2 / (count - 1) if sample else m2 / count
    if std:
        return math.sqrt(var) if var >= 0 else math.nan
    return var


def covariance_final(fn, t):
    """CovarianceAggregationFunction.extractFinalResult (:186-203); fn in COVARPOP / COVARSAMP."""
    sx, sy, sxy, count = t
    if count == 0:
        return -math.inf
    if fn == "COVARSAMP":
        if count - 1 == 0:
            return -math.inf
        return (sxy / (count - 1)) - (sx * sy) / (count * (count - 1))
    return (sxy / count) - (sx * sy) / (count * count)


# ---------------------------------------------------------------- exact
def frac(v):
    """The stored value exactly (a numpy float32 / float64 / integer scalar, or a Python number)."""
    if isinstance(v, float):
        return Fraction(v)
    try:
        import numpy as np
        if isinstance(v, np.floating):
            return Fraction(float(v))  # (float32 -> float64 is exact)
        if isinstance(v, np.integer):
            return Fraction(int(v))
    except ImportError:
        pass
    return Fraction(v)


def exact_variance(values):
    """(count, sum, m2) over Fractions: m2 = sum x^2 - (sum x)^2 / n (Python integers: plain integer arithmetic)."""
    if values and all(type(v) is int for v in values):
        n, s = len(values), sum(values)
        return (n, Fraction(s), Fraction(n * sum(v * v for v in values) - s * s, n))
    xs = [frac(v) for v in values]
    n = len(xs)
    s = sum(xs, Fraction(0))
    if n == 0:
        return (0, Fraction(0), Fraction(0))
    return (n, s, sum((x * x for x in xs), Fraction(0)) - s * s / n)


def exact_covariance(xs, ys):
    """(sum_x, sum_y, sum_xy, count) over Fractions."""
    if xs and all(type(v) is int for v in xs) and all(type(v) is int for v in ys):
        return (Fraction(sum(xs)), Fraction(sum(ys)), Fraction(sum(x * y for x, y in zip(xs, ys))), len(xs))
    xs, ys = [frac(v) for v in xs], [frac(v) for v in ys]
    return (sum(xs, Fraction(0)), sum(ys, Fraction(0)), sum((x * y for x, y in zip(xs, ys)), Fraction(0)), len(xs))


def nearest_double(fr):
    """The double nearest to a Fraction (ties to even): Python's int / int division is correctly rounded."""
    return fr.numerator / fr.denominator


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u), u = 2^-53, as a Fraction."""
    u = Fraction(1, 1 << 53)
    return k * u / (1 - k * u)


def double_form_bounds(values, pivot, with_sum=False):
    """A-priori bounds for the double form's variance over `values` (any summation order), from the group's own pivoted
    values in Fractions: (exact m2, bound on |m2_computed - m2|); with_sum: (count, exact m2, its bound, the exact sum of
    the values, the bound gamma_{n+3} sum |d| on the computed sum of the pivoted values). The values and the pivot are
    doubles or integers, so every d is an integer over one common power-of-two denominator: the sums run over integers.

    The device forms d = fl(x - c) (one rounding; the exact m2 of the d's is compared with the exact m2 of the x's
    through the same bound), S1 = sum d and S2 = sum fl(d^2) in some order and with some grouping: n terms, n - 1
    additions at most in a chain, plus the rounding of each term (the subtraction, the square), plus the adds of the
    partial sums across waves / workgroups: k = n + 3 roundings per term covers every such tree (Higham, Accuracy and
    Stability of Numerical Algorithms, section 4.2: |S - fl(S)| <= gamma_{n-1} sum |term| for any order; the roundings of
    the terms themselves add at most 2 more, one more of slack). So
        |S1 - S1'| <= g sum |d|,   |S2 - S2'| <= g sum d^2,   g = gamma_{n+3}
    and through m2 = S2 - S1^2 / n, evaluated as fma(-S1, fl(S1 / n), S2) (two more roundings, each relative 2^-53 of
    a quantity bounded by S2' + S1'^2 / n):
        |m2' - m2| <= g sum d^2 + (2 |S1| e1 + e1^2) / n + 3 u (sum d^2 (1 + g) + (|S1| + e1)^2 / n),   e1 = g sum |d|
    """
    c = Fraction(pivot)
    n = len(values)
    if n == 0:
        return (0, Fraction(0), Fraction(0), Fraction(0), Fraction(0)) if with_sum else (Fraction(0), Fraction(0))
    ratios = [v.as_integer_ratio() if isinstance(v, float) else (frac(v).numerator, frac(v).denominator) for v in values]
    den = max(max(q for _, q in ratios), c.denominator)  # (powers of two: the largest is a common denominator)
    assert den & (den - 1) == 0 and all(den % q == 0 for _, q in ratios)
    cn = c.numerator * (den // c.denominator)
    di = [p * (den // q) - cn for p, q in ratios]  # d = di / den
    s1 = Fraction(sum(di), den)
    s2 = Fraction(sum(d * d for d in di), den * den)
    sa = Fraction(sum(abs(d) for d in di), den)
    m2 = s2 - s1 * s1 / n
    g = gamma(n + 3)
    u = Fraction(1, 1 << 53)
    e1 = g * sa
    bound = g * s2 + (2 * abs(s1) * e1 + e1 * e1) / n + 3 * u * (s2 * (1 + g) + (abs(s1) + e1) ** 2 / n)
    if with_sum:
        return n, m2, bound, s1 + n * c, e1
    return m2, bound


def sum_bound(terms):
    """(exact sum, bound on |computed - exact|) of a double sum of `terms` (Fractions) in any order, each term itself
    rounded once when formed (a product): gamma_{n+3} sum |term|."""
    n = len(terms)
    if n == 0:
        return Fraction(0), Fraction(0)
    return sum(terms, Fraction(0)), gamma(n + 3) * sum((abs(t) for t in terms), Fraction(0))
