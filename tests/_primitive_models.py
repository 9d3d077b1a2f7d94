"""CPU models of the device primitives in littlemcmc_amd/csrc (lmc_wave.hpp, lmc_team.hpp, lmc_targets.hpp), each restated in
its documented operation order with exactly rounded IEEE operations, plus the high-precision references and the derived
error bounds that tests/test_primitive_models_cpu.py (here) and tests/test_gpu_primitives.py (on the device) hold them to.

The exponentials' table and constants are parsed out of the header text, so the model cannot drift from the source.
Needs numpy and mpmath only."""
import math
import os
import re
from fractions import Fraction

import numpy as np
from mpmath import mp, mpf

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "littlemcmc_amd", "csrc")
U = 2.0 ** -53            # unit roundoff of float64
TINY = 2.0 ** -1074       # spacing of the subnormals
PREC = 400                # bits of the mpmath references: 1e+-150 squared and summed is still exact to ~1e-100


def gamma(k):
    """k roundings compounded: |prod (1 + d_i) - 1| <= k u / (1 - k u) for |d_i| <= u (Higham, Lemma 3.1)."""
    return k * U / (1.0 - k * U)


# ---- exact IEEE steps ----------------------------------------------------------------------------------------------------
def fma(a, b, c):
    """round_to_nearest_even(a * b + c) with a single rounding (finite arguments)."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def ldexp(x, k):
    """round_to_nearest_even(x 2^k): one rounding when the result is subnormal, +-inf on overflow."""
    if x == 0.0 or k == 0:
        return x
    if k > 2200:
        return math.copysign(math.inf, x)
    if k < -2200:
        return math.copysign(0.0, x)
    try:
        return float(Fraction(x) * (Fraction(2) ** k))
    except OverflowError:
        return math.copysign(math.inf, x)


def rint(x):
    return float(np.rint(x))


# ---- the header's own numbers --------------------------------------------------------------------------------------------
def _header(name="lmc_wave.hpp", csrc=None):
    with open(os.path.join(csrc or CSRC, name)) as fh:
        return fh.read()


def _number(expr):
    """'1.0 / 720.0' or '92.33': the double the compiler folds the expression to (a correctly rounded quotient)."""
    parts = [p.strip() for p in expr.split("/")]
    assert 1 <= len(parts) <= 2, expr
    val = float(parts[0])
    return val / float(parts[1]) if len(parts) == 2 else val


def _function_constants(text, signature):
    i = text.index(signature)
    body = text[i:text.index("\n}\n", i)]
    return [_number(m) for m in re.findall(r"LMC_SC\(([^()]*)\)", body)], body


def exp2_table(csrc=None):
    """kExp2Table as the compiler reads it: 64 doubles."""
    m = re.search(r"kExp2Table\[64\]\s*=\s*\{(.*?)\};", _header(csrc=csrc), re.S)
    vals = [float(tok) for tok in m.group(1).replace("\n", " ").split(",")]
    assert len(vals) == 64
    return vals


class ExpUniformModel:
    """exp_uniform(): clamp to [-800, 800], k = rint(x log2 e), Cody-Waite r = (x - k ln2_hi) - k ln2_lo in two FMAs, degree-13
    Horner polynomial in FMAs (coefficients 1/13! ... 1/3!, then 1/2, 1, 1), ldexp(p, k)."""

    def __init__(self, csrc=None):
        self.c, body = _function_constants(_header(csrc=csrc), "double exp_uniform(double x) {")
        assert len(self.c) == 14 and body.count("__builtin_fma(p, r,") == 3, "exp_uniform no longer reads as modelled"
        self.lo, self.hi = (float(v) for v in re.search(r"fmin\(fmax\(x, (\S+)\), (\S+)\)", body).groups())

    def __call__(self, x):
        c = self.c
        xv = min(max(x, self.lo), self.hi)
        kf = rint(xv * c[0])
        r = fma(-kf, c[1], xv)
        r = fma(-kf, c[2], r)
        p = fma(r, c[3], c[4])
        for coef in c[5:]:
            p = fma(p, r, coef)
        for coef in (0.5, 1.0, 1.0):
            p = fma(p, r, coef)
        return ldexp(p, int(kf))


class ExpUniformFastModel:
    """exp_uniform_fast(): k = rint(x 64/ln2), r = (x - k hi) - k lo in two FMAs (ln2/64 in two pieces), t = table[k & 63],
    degree-5 Horner polynomial in FMAs (1/120, 1/24, 1/6, 1/2, 1, 1), ldexp(p t, k >> 6)."""

    def __init__(self, csrc=None):
        self.c, body = _function_constants(_header(csrc=csrc), "double exp_uniform_fast(double x) {")
        assert len(self.c) == 6 and body.count("__builtin_fma(p, r,") == 3, "exp_uniform_fast no longer reads as modelled"
        self.table = exp2_table(csrc)

    def __call__(self, x):
        c = self.c
        kf = rint(x * c[0])
        r = fma(-kf, c[1], x)
        r = fma(-kf, c[2], r)
        ki = int(kf)
        t = self.table[ki & 63]
        p = fma(r, c[3], c[4])
        p = fma(p, r, c[5])
        for coef in (0.5, 1.0, 1.0):
            p = fma(p, r, coef)
        return ldexp(p * t, ki >> 6)


# the bounds of the two exponentials in ulps of the exact value (tests/test_primitive_models_cpu.py derives the second)
EXP_UNIFORM_ULP = 1.5
EXP_FAST_ULP = 3.5
EXP_FAST_SUBNORMAL_ULP = 4.0     # + half a subnormal spacing: ldexp rounds a second time there


def ulp_of(exact):
    """Spacing of the float64 grid at the (mpmath) value ``exact`` (the subnormal spacing below 2^-1022)."""
    if exact == 0:
        return mpf(TINY)
    e = int(mp.floor(mp.log(abs(exact), 2)))
    return mpf(2) ** (max(e, -1022) - 52)


def ulp_errors(xs, got, fn=None):
    """|got - fn(x)| in ulps of fn(x), per argument (fn: mpmath function of the exactly converted x, default exp)."""
    fn = fn or mp.exp
    out = np.empty(len(xs))
    with mp.workprec(PREC):
        for i, (x, y) in enumerate(zip(xs, got)):
            exact = fn(mpf(float(x)))
            out[i] = float(abs(mpf(float(y)) - exact) / ulp_of(exact))
    return out


def exp_arguments(rs, lo, hi, n_bulk, per_ln2):
    """Named argument classes of an exponential on the callers' domain [lo, hi]: the bulk, results in the subnormal range,
    |x| < 1e-3 (both signs and zeros), and neighbourhoods of the reduction's breakpoints (k + 1/2) ln2 / per_ln2, where rint
    switches k and |r| is largest."""
    ln2 = math.log(2.0)
    classes = {"bulk": rs.uniform(lo, hi, n_bulk)}
    classes["subnormal"] = rs.uniform(-745.2, -708.3, max(n_bulk // 8, 16))
    small = np.concatenate([rs.uniform(-1e-3, 1e-3, max(n_bulk // 16, 16)), 10.0 ** rs.uniform(-300, -3, 16),
                            -(10.0 ** rs.uniform(-300, -3, 16)), [0.0, -0.0, 5e-324, -5e-324]])
    classes["small"] = small
    ks = np.concatenate([rs.randint(int(lo * per_ln2 / ln2), int(hi * per_ln2 / ln2), max(n_bulk // 16, 16)), np.arange(-4, 4)])
    bp = (ks + 0.5) * (ln2 / per_ln2)
    near = np.concatenate([bp, np.nextafter(bp, np.inf), np.nextafter(bp, -np.inf), bp * (1 + 4e-16), bp * (1 - 4e-16),
                           bp + rs.uniform(-1e-9, 1e-9, bp.size)])
    classes["breakpoints"] = near[(near >= lo) & (near <= hi)]
    return classes


EXP_FAST_REFUTATION = -540.68189113023186   # exp_uniform_fast is 2.22 ulp off here: the "< 1 ulp" of the header is false


# ---- reductions in the device's order -------------------------------------------------------------------------------------
def _tree(x):
    """Balanced adjacent-pair tree over the last axis (a power of two): ((x0 + x1) + (x2 + x3)) + ..."""
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def wave_sum(x):
    """wave_sum over x[..., 64]: Hillis-Steele rows (row_shr 1, 2, 4, 8: a balanced tree of adjacent pairs in lane 15 of each
    row), row_bcast:15 (R1 + R0, R3 + R2), row_bcast:31: (R3 + R2) + (R1 + R0) -- the balanced tree over all 64 lanes."""
    assert x.shape[-1] == 64
    with np.errstate(all="ignore"):
        return _tree(np.asarray(x, dtype=np.float64))


def wave_sum2(x):
    """One value of wave_sum2 / any_sum_nonpositive2 over x[..., 64]: c_l = x_l + x_{l+32} (the permlane32 swap add), then the
    balanced tree over the 32 c (row scan, row_bcast:15)."""
    assert x.shape[-1] == 64
    with np.errstate(all="ignore"):
        x = np.asarray(x, dtype=np.float64)
        return _tree(x[..., :32] + x[..., 32:])


def wave_sum6(x):
    """One value of wave_sum6_totals / any_sum_nonpositive6 over x[..., 64]: c_l = x_l + x_{l+32}, e_l = c_l + c_{l+16} (the
    permlane16 swap add), then the row scan's balanced tree over the 16 e."""
    assert x.shape[-1] == 64
    with np.errstate(all="ignore"):
        x = np.asarray(x, dtype=np.float64)
        c = x[..., :32] + x[..., 32:]
        return _tree(c[..., :16] + c[..., 16:])


def team_total(per_wave):
    """Team exchange over per_wave[..., W]: the wave totals added in wave order."""
    with np.errstate(all="ignore"):
        acc = per_wave[..., 0]
        for w in range(1, per_wave.shape[-1]):
            acc = acc + per_wave[..., w]
        return acc


def team_reduce(x, w, wave_fn):
    """x[..., 64 w] -> team total, the waves reduced by wave_fn (wave_sum / wave_sum2 / wave_sum6)."""
    x = np.asarray(x, dtype=np.float64)
    return team_total(wave_fn(x.reshape(x.shape[:-1] + (w, 64))))


def team_any_nonpositive(x, w, wave_fn):
    """x[..., K, 64 w] -> bool: any of the K sums (device order) <= 0; NaN compares false like the device's v_cmp_le."""
    with np.errstate(all="ignore"):
        return (team_reduce(x, w, wave_fn) <= 0.0).any(axis=-1)


def left_to_right(x):
    """The plain sequential sum over the last axis (what a reduction-order test must be able to tell from the device's)."""
    with np.errstate(all="ignore"):
        x = np.asarray(x, dtype=np.float64)
        acc = x[..., 0]
        for i in range(1, x.shape[-1]):
            acc = acc + x[..., i]
        return acc


def exact_sum(x):
    """(sum, sum of magnitudes) of a float64 vector in mpmath."""
    with mp.workprec(2200):
        vals = [mpf(float(v)) for v in np.ravel(x)]
        return mp.fsum(vals), mp.fsum(vals, absolute=True)


# ---- reduction inputs -----------------------------------------------------------------------------------------------------
def wide_range_vectors(rs, shape):
    """Magnitudes over 1e-150 ... 1e150, random signs."""
    return rs.randn(*shape) * 10.0 ** rs.uniform(-150, 150, shape)


def cancellation_vectors(rs, shape):
    """Every vector (last axis, even length) holds n/2 values spread over 2^0 ... 2^40 and their negatives, shuffled, plus
    noise at 1e-3: the exact sum is tiny against sum |x|, so every summation order rounds to a different result."""
    n = shape[-1]
    half = rs.randn(*(shape[:-1] + (n // 2,))) * 2.0 ** rs.uniform(0, 40, shape[:-1] + (n // 2,))
    x = np.concatenate([half, -half], axis=-1) + 1e-3 * rs.randn(*shape)
    flat = x.reshape(-1, n)
    for row in flat:
        rs.shuffle(row)
    return flat.reshape(shape)


def knife_edge_vectors(rs, shape):
    """Cancellation vectors whose EXACT sum is pushed to (almost) zero: the largest element absorbs the correctly rounded
    sum, so what any finite-precision order returns is its own rounding noise -- the sign depends on the order."""
    x = cancellation_vectors(rs, shape)
    flat = x.reshape(-1, shape[-1])
    for row in flat:
        j = int(np.argmax(np.abs(row)))
        row[j] -= math.fsum(row)
    return flat.reshape(shape)


# ---- densities: the formulas of oracle/targets.py in mpmath, with per-entry error bounds ----------------------------------
# A bound is the sum of what each rounding of the device's operation order can contribute, nothing else:
#   * a sum of n terms formed by FMAs and added in ANY order carries at most gamma(n) sum |terms|;
#   * every operation whose result can be subnormal adds half a subnormal spacing (n TINY covers a whole sum);
#   * e^{-v} from exp_uniform_fast is within EXP_FAST_ULP ulps = 2 EXP_FAST_ULP u relative (its results stay normal:
#     the argument is max(-v, -700) and |v| <= 708 in the tests);
#   * for v > 700 the functor uses e^{-700} by design: every term carrying e^{-v} may be off by e^{-700} times its factor.
E_FAST = 2.0 * EXP_FAST_ULP * U


def _mpl(a):
    return [mpf(float(v)) for v in a]


def _quadratic(q, g, delta, n):
    """logp = 1/2 sum q_e ghat_e (FMA chain and tree), ghat_e within delta_e of g_e: value and bound."""
    logp = mp.fdot(q, g) / 2
    mag = mp.fsum(abs(a) * (abs(b) + e) for a, b, e in zip(q, g, delta))
    carried = mp.fsum(abs(a) * e for a, e in zip(q, delta))
    return logp, (carried + gamma(n) * mag) / 2 + n * TINY


def density_reference(family, q, params=()):
    """(logp, logp_tol, g, g_tol) of a FINITE position q: mpmath values of oracle/targets.py's formulas and the bounds the
    device's operation order (lmc_targets.hpp) must meet, as mpf scalars and lists of mpf."""
    with mp.workprec(PREC):
        return _density_reference(family, q, params)


def _density_reference(family, q, params):
    n = len(q)
    x = _mpl(q)
    if family == "std_normal":          # fma(q, q, part); g = -q exactly
        s = mp.fdot(x, x)
        return -s / 2, gamma(n) * s / 2 + n * TINY, [-a for a in x], [mpf(0)] * n
    if family == "diag_gaussian":       # g = -(prec q): one rounding
        p = _mpl(params)
        g = [-(a * b) for a, b in zip(p, x)]
        delta = [U * abs(b) + TINY for b in g]
        logp, tol = _quadratic(x, g, delta, n)
        return logp, tol, g, delta
    if family == "ar1":                 # (diag q + off prev) + off next: two products, two sums; three roundings on any path
        c_end, c_mid, off = (mpf(float(v)) for v in params)
        g, delta = [], []
        for e in range(n):
            dg = c_end if e in (0, n - 1) else c_mid
            prev = x[e - 1] if e > 0 else mpf(0)
            nxt = x[e + 1] if e < n - 1 else mpf(0)
            g.append(-((dg * x[e] + off * prev) + off * nxt))
            delta.append(gamma(3) * (abs(dg * x[e]) + abs(off * prev) + abs(off * nxt)) + 4 * TINY)
        logp, tol = _quadratic(x, g, delta, n)
        return logp, tol, g, delta
    if family == "funnel":
        v, rest = x[0], x[1:]
        s = mp.fdot(rest, rest)
        ev = mp.exp(-v)                                  # the reference
        evm = mp.exp(max(-v, mpf(-700)))                 # what the device's exponential aims at
        clamp = mp.exp(-700) if v > 700 else mpf(0)      # the stated absolute effect of the clamp, per unit of the factor
        s_hat = s * (1 + gamma(max(n - 1, 1))) + n * TINY                # largest the device's sum of squares can be
        hes = ev * s / 2
        hes_hat = evm * (1 + E_FAST) * s_hat / 2 * (1 + U) + TINY        # 0.5 ev exact, one product
        d_hes = hes_hat - evm * s / 2 + clamp * s / 2
        a1, a2 = v * v / 18, abs((n - 1) * v / 2)
        logp = -v * v / 18 - (n - 1) * v / 2 - hes
        # lin = -(v v)(1/18) - (0.5 dm1) v: v v, the constant, the product | one product | the difference; then lin - hes
        tol = gamma(5) * a1 + gamma(3) * a2 + d_hes * (1 + U) + U * hes + 4 * TINY
        g0 = -v / 9 - mpf(n - 1) / 2 + hes
        # g0 = (-v (1/9) - 0.5 dm1) + hes: the constant, the product | exact | the difference, the sum
        tol0 = gamma(4) * abs(v) / 9 + gamma(2) * mpf(n - 1) / 2 + d_hes * (1 + U) + U * hes + 4 * TINY
        g = [g0] + [-(ev * a) for a in rest]
        g_tol = [tol0] + [evm * abs(a) * ((1 + E_FAST) * (1 + U) - 1) + clamp * abs(a) + TINY for a in rest]
        return logp, tol, g, g_tol
    if family == "normal1d":
        # z = (x - loc) / scale: two roundings; -0.5 z z: one more on z^2 / 2 (four carried, one own);
        # lognorm = log(scale sqrt(2 pi)): pi as a double (u/2), sqrt and log of the device library within 1 ulp = 2 u each
        # (AMD's documented accuracy of the double-precision sqrt and log), one product: the argument of the log is within
        # 3.5 u relative, which moves the log by as much in absolute terms; then the difference
        loc, scale = (mpf(float(v)) for v in params)
        z = (x[0] - loc) / scale
        lognorm = mp.log(scale * mp.sqrt(2 * mp.pi))
        logp = -z * z / 2 - lognorm
        tol = gamma(5) * z * z / 2 + (gamma(4) + 2 * U * abs(lognorm)) + U * (z * z / 2 + abs(lognorm)) * (1 + gamma(6)) + 4 * TINY
        g = [-(x[0] - loc) / scale] + [mpf(0)] * (n - 1)
        return logp, tol, g, [gamma(2) * abs(g[0]) + TINY] + [mpf(0)] * (n - 1)
    raise ValueError(family)



def ar1_params(rho):
    """{c_end, c_mid, off} of oracle/targets.py's AR1 for correlation rho."""
    c = 1.0 / (1.0 - rho * rho)
    return np.array([c, (1.0 + rho * rho) * c, -rho * c])


FUNNEL_V = (-700.5, -100.0, -1e-3, 0.0, 50.0, 699.0, 700.0, 701.0, 1000.0)


def _position_rows(rs, d, top=None):
    """Finite positions beyond randn: magnitudes 1e-150 ... 1e150 (exponents capped elementwise by ``top``), the same with
    signed zeros sprinkled in, and signed zeros alone."""
    def wide_row():
        ex = rs.uniform(-150, 150, d)
        if top is not None:
            ex = np.minimum(ex, top)
        return rs.choice([-1.0, 1.0], d) * rs.uniform(1, 10, d) * 10.0 ** (ex - 1)

    wide, mixed = wide_row(), wide_row()
    mixed[rs.rand(d) < 0.3] = 0.0
    mixed[rs.rand(d) < 0.15] = -0.0
    zeros = np.where(rs.rand(d) < 0.5, 0.0, -0.0)
    return np.stack([rs.randn(d), wide, mixed, zeros])


def density_inputs(family, d, rs):
    """[(label, params, q[rows, d])]: the finite input classes every density is held to its reference on. Magnitudes are
    capped only where the exact logp would leave the float64 range (the sum of up to 16384 terms of 1e300 fits)."""
    if family == "std_normal":
        return [("", np.zeros(0), _position_rows(rs, d))]
    if family == "diag_gaussian":     # precisions spanning 1e-12 ... 1e12; prec q^2 <= 1e300
        pe = rs.uniform(-12, 12, d)
        pe[rs.randint(d)] = 12.0
        pe[rs.randint(d)] = -12.0
        return [("prec 1e+-12", 10.0 ** pe, _position_rows(rs, d, top=(300 - pe) / 2))]
    if family == "ar1":               # |P| <= 4 c ~ 2000 at |rho| = 0.999: q P q <= 1e300
        return [("rho %g" % rho, ar1_params(rho), _position_rows(rs, d, top=148.0)) for rho in (0.999, -0.999, 0.0)]
    if family == "funnel":            # x at the funnel's own scale e^{v/2}, held where x^2 and e^{-v} x^2 stay finite
        rows = []
        for v in FUNNEL_V:
            q = rs.randn(d) * math.exp(min(max(v / 2, -345.0), 340.0))
            q[0] = v
            rows.append(q)
        out = [("v " + ", ".join("%g" % v for v in FUNNEL_V), np.zeros(0), np.stack(rows))]
        wide = _position_rows(rs, d)
        wide[:, 0] = [0.5, 0.0, -0.0, -0.0]
        return out + [("wide x", np.zeros(0), wide)]
    if family == "normal1d":
        assert d == 1
        out = [("loc 0 scale 1", np.array([0.0, 1.0]),
                np.array([[rs.randn()], [1e150], [-1e150], [1e-150], [-1e-150], [0.0], [-0.0]]))]
        for loc, scale in ((1.5, 0.3), (-2e3, 1e-12), (1e10, 1e12)):
            t = np.array([rs.randn(), 1e3, -1e-3, 0.0, 1e-14, -37.5])
            out.append(("loc %g scale %g" % (loc, scale), np.array([loc, scale]), (loc + scale * t)[:, None]))
        return out
    raise ValueError(family)


def density_check(ref, logp, g):
    """Largest error / bound ratio of a computed (logp, g[:d]) against density_reference()'s tuple; entries whose bound is 0
    must be equal (ratio inf otherwise)."""
    want, tol, g_ref, g_tol = ref
    with mp.workprec(PREC):
        pairs = [(abs(mpf(float(logp)) - want), tol)] + [(abs(mpf(float(a)) - b), t) for a, b, t in zip(g, g_ref, g_tol)]
        worst, where = 0.0, -1
        for k, (err, t) in enumerate(pairs):
            if not mp.isfinite(err):
                return math.inf, k - 1
            if err == 0:
                continue
            ratio = float(err / t) if t > 0 else math.inf
            if ratio > worst:
                worst, where = ratio, k - 1
        return worst, where
