"""-m gpu: the wave and team device primitives (csrc/lmc_wave.hpp, lmc_team.hpp, lmc_rng.hpp: log_unit, lmc_targets.hpp), each
on its own against an exact reference, through the test-only probe library (tests/probe/lmc_probe.hip, tests/_probe.py).

Two kinds of check, kept independent of each other:
  * device == CPU model (tests/_primitive_models.py) bit for bit, where every step is an IEEE operation whose order the
    header documents (the exponentials; the reductions and the U-turn predicates);
  * device within a derived bound of the mpmath value: the exponentials' ulp bounds (derivation:
    tests/test_primitive_models_cpu.py), (64 W - 1) 2^-53 sum |x| for a reduction, per-entry bounds for the densities
    (_primitive_models.density_reference). No bound is fitted to what the device returns; the observed maxima are printed."""
import math

import numpy as np
import pytest
from mpmath import mp, mpf

import littlemcmc_amd as lmc
from littlemcmc_amd import targets as T
from tests import _primitive_models as M
from tests import _probe as P          # importing it loads nothing: the library is opened by the first call

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    from tests import _probe

    _probe.load()   # a missing or stale probe is an error with instructions, not a skip
    return _probe


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_same_bits(got, want, what, args=None):
    bad = np.nonzero(_bits(got) != _bits(want))[0]
    if len(bad):
        i = int(bad[0])
        raise AssertionError("%s: %d of %d differ from the model; first at index %d%s: device %r (%s), model %r (%s)" % (
            what, len(bad), np.size(got), i, "" if args is None else " (argument %r)" % float(np.ravel(args)[i]),
            float(np.ravel(got)[i]), float(np.ravel(got)[i]).hex(), float(np.ravel(want)[i]), float(np.ravel(want)[i]).hex()))


# ---- exponentials ---------------------------------------------------------------------------------------------------------
def _exp_case(fast):
    if fast:   # tree weights x - coff <= 600 down to -(Emax + 600); the funnel passes max(-v, -700)
        return M.ExpUniformFastModel(), M.exp_arguments(np.random.RandomState(202), -1700.0, 709.78, 6000, 64)
    return M.ExpUniformModel(), M.exp_arguments(np.random.RandomState(201), -2000.0, 709.78, 4000, 1)


@pytest.mark.parametrize("fast", [False, True], ids=["exp_uniform", "exp_uniform_fast"])
def test_exponential_equals_model_bit_for_bit(probe, fast):
    """FMA, rint and ldexp are exactly rounded on both sides and the constants are the header's: no bit may differ."""
    model, classes = _exp_case(fast)
    classes["named"] = np.array([M.EXP_FAST_REFUTATION, 0.0, -0.0, 709.78, -745.13, -745.14, -700.0, 600.0, 1.0, -1.0])
    if not fast:   # the rest of exp_uniform's domain [-2000, 800]: overflow, the clamp's edge
        classes["above 709.78"] = np.concatenate([[709.79, 710.0, 750.0, 799.0, np.nextafter(800.0, 0.0), 800.0],
                                                  np.random.RandomState(205).uniform(709.78, 800.0, 100)])
    for name, xs in classes.items():
        got = probe.exp_uniform(xs, fast=fast)
        want = np.array([model(float(x)) for x in xs])
        _assert_same_bits(got, want, "%s, %s" % ("exp_uniform_fast" if fast else "exp_uniform", name), xs)


@pytest.mark.parametrize("fast", [False, True], ids=["exp_uniform", "exp_uniform_fast"])
def test_exponential_within_bound_of_mpmath(probe, fast):
    """exp_uniform: 1.5 ulp (the header's figure). exp_uniform_fast: 3.5 ulp, 4.0 where the result is subnormal (derived in
    tests/test_primitive_models_cpu.py; the "< 1 ulp" the header claimed is refuted by EXP_FAST_REFUTATION)."""
    _model, classes = _exp_case(fast)
    classes["named"] = np.array([M.EXP_FAST_REFUTATION, 0.0, -0.0, 709.78, -745.13])
    worst = 0.0
    for name, xs in classes.items():
        got = probe.exp_uniform(xs, fast=fast)
        err = M.ulp_errors(xs if fast else np.maximum(xs, -800.0), got)
        if fast:
            bound = np.where(np.exp(xs) < 2.0 ** -1022, M.EXP_FAST_SUBNORMAL_ULP, M.EXP_FAST_ULP)
        else:
            bound = np.full(len(xs), M.EXP_UNIFORM_ULP)
        i = int(np.argmax(err))
        worst = max(worst, err[i])
        print("%s device, %s: %d arguments, max %.3f ulp at x = %r" % ("exp_uniform_fast" if fast else "exp_uniform", name,
                                                                      len(xs), err[i], float(xs[i])))
        j = int(np.argmax(err / bound))
        assert err[j] <= bound[j], (name, float(xs[j]), err[j], bound[j])
    print("%s device: max %.3f ulp overall" % ("exp_uniform_fast" if fast else "exp_uniform", worst))


def test_exponentials_overflow_and_underflow_exactly(probe):
    rs = np.random.RandomState(203)
    over = np.concatenate([[709.79, 710.0, 750.0, 800.0, np.nextafter(800.0, np.inf), 801.0, 2000.0], rs.uniform(709.79, 2000.0, 200)])
    under = np.concatenate([[-745.14, -746.0, -800.0, -801.0, -2000.0], rs.uniform(-2000.0, -745.14, 200)])
    assert np.all(probe.exp_uniform(over) == np.inf)
    got = probe.exp_uniform(under)
    assert np.all(got == 0.0) and not np.signbit(got).any()
    over_fast = np.concatenate([[709.79, 710.0], rs.uniform(709.79, 712.0, 50)])
    under_fast = np.concatenate([[-745.14, -746.0, -1700.0], rs.uniform(-1700.0, -745.14, 200)])
    assert np.all(probe.exp_uniform(over_fast, fast=True) == np.inf)
    got = probe.exp_uniform(under_fast, fast=True)
    assert np.all(got == 0.0) and not np.signbit(got).any()
    for fast in (False, True):   # the last finite and the last non-zero side of each edge
        edge = probe.exp_uniform([709.78, -745.13], fast=fast)
        assert np.isfinite(edge[0]) and edge[0] > 1.79e308 and edge[1] == 5e-324


# ---- log_unit --------------------------------------------------------------------------------------------------------------
def test_log_unit_within_one_ulp_of_numpy(probe):
    """The argument classes its header names: the bulk of (0, 1), near 1, near 0 down to the smallest normals. The
    project's own claim: never more than 1 ulp from numpy's log."""
    rs = np.random.RandomState(204)
    tiny = np.finfo(np.float64).tiny
    one_minus = 1.0 - 2.0 ** -np.arange(1, 54, dtype=np.float64)
    below_one = [np.nextafter(1.0, 0.0)]
    for _ in range(63):
        below_one.append(np.nextafter(below_one[-1], 0.0))
    classes = {
        "bulk": rs.uniform(0.0, 1.0, 20000),
        "near 1": np.concatenate([one_minus, below_one, 1.0 - rs.uniform(0, 1e-3, 2000), 1.0 - 10.0 ** rs.uniform(-16, -3, 2000),
                                  np.sqrt(0.5) * (1 + rs.uniform(-1e-6, 1e-6, 2000))]),
        "near 0": np.concatenate([tiny * np.arange(1, 65), tiny * (1 + rs.uniform(0, 8, 500)), 10.0 ** rs.uniform(-307.6, -1, 4000),
                                  2.0 ** -np.arange(1, 1023, dtype=np.float64)]),
    }
    for name, xs in classes.items():
        xs = xs[(xs > 0.0) & (xs < 1.0)]
        got = probe.log_unit(xs)
        want = np.log(xs)
        apart = np.abs(got - want) / np.spacing(np.abs(want))
        i = int(np.argmax(apart))
        err = M.ulp_errors(xs, got, fn=mp.log)
        j = int(np.argmax(err))
        print("log_unit device, %s: %d arguments, at most %.0f ulp from numpy (x = %r), max %.3f ulp from mpmath (x = %r)" % (
            name, len(xs), apart[i], float(xs[i]), err[j], float(xs[j])))
        assert apart[i] <= 1.0, (name, float(xs[i]), float(got[i]), float(want[i]))


# ---- reductions, broadcast, neighbours --------------------------------------------------------------------------------------
ROUNDS = 5   # consecutive rounds in one kernel: both parities of the exchange buffer, back to back, fresh data each


def _randn(rs, shape):
    return rs.randn(*shape)


def _team_inputs(rs, w):
    """x[blocks, ROUNDS, 14, 64 w]: per input class a few blocks whose every row is of that class."""
    t = 64 * w
    parts = []
    for make in (_randn, M.wide_range_vectors, M.cancellation_vectors, M.knife_edge_vectors):
        parts.append(make(rs, (4, ROUNDS, P.TEAM_N_IN, t)))
    x = np.concatenate(parts)
    x[0, 1, 11, 0] = -0.0    # a team bcast0 turns -0.0 into +0.0 by design: compared with ==
    x[1, 2, 11, 0] = 0.0
    return x


@pytest.mark.parametrize("w", P.TEAM_WIDTHS)
def test_team_reductions_equal_the_order_model(probe, w):
    """sum / sum2 of Team<w>, ROUNDS times back to back: every wave's copy is the order model's bits (random data, a
    1e+-150 dynamic range, cancellation and knife-edge vectors), and, independently, within (64 w - 1) 2^-53 sum |x| of the
    exact sum. The U-turn predicates on the same data equal the model's sign tests."""
    rs = np.random.RandomState(300 + w)
    x = _team_inputs(rs, w)
    out = probe.team(w, x)
    rows = probe.TEAM_ROWS
    want = {"sum": M.team_reduce(x[:, :, rows["sum"]], w, M.wave_sum),
            "sum2a": M.team_reduce(x[:, :, rows["sum2"][0]], w, M.wave_sum2),
            "sum2b": M.team_reduce(x[:, :, rows["sum2"][1]], w, M.wave_sum2)}
    src = {"sum": rows["sum"], "sum2a": rows["sum2"][0], "sum2b": rows["sum2"][1]}
    worst = 0.0
    for name, val in want.items():
        for wave in range(w):
            _assert_same_bits(out[name][:, :, wave].ravel(), val.ravel(), "Team<%d>::%s, wave %d's copy" % (w, name, wave))
        for b in range(x.shape[0]):
            for r in range(ROUNDS):
                s, mag = M.exact_sum(x[b, r, src[name]])
                err = abs(mpf(float(out[name][b, r, 0])) - s)
                bound = (64 * w - 1) * M.U * mag
                assert err <= bound, (name, b, r, float(err), float(bound))
                worst = max(worst, float(err / bound))
    print("Team<%d> sums: at most %.3f of (64 W - 1) u sum |x| from the exact sum" % (w, worst))
    np2 = M.team_any_nonpositive(x[:, :, list(rows["np2"])], w, M.wave_sum2)
    np6 = M.team_any_nonpositive(x[:, :, list(rows["np6"])], w, M.wave_sum6)
    for wave in range(w):
        np.testing.assert_array_equal(out["np2"][:, :, wave], np2.astype(float), err_msg="any_nonpositive2, wave %d" % wave)
        np.testing.assert_array_equal(out["np6"][:, :, wave], np6.astype(float), err_msg="any_nonpositive6, wave %d" % wave)


@pytest.mark.parametrize("w", P.TEAM_WIDTHS)
def test_team_bcast0_and_neighbours_are_exact_copies(probe, w):
    """bcast0: thread 0's value in every thread. neighbours: thread t gets lo_src of t - 1 and hi_src of t + 1 -- across
    every wave edge of the team -- and exact zeros at the team's two edges. Compared with ==."""
    rs = np.random.RandomState(320 + w)
    x = _team_inputs(rs, w)
    out = probe.team(w, x)
    rows = probe.TEAM_ROWS
    t = 64 * w
    assert np.array_equal(out["bcast0"], np.broadcast_to(x[:, :, rows["bcast0"], :1], out["bcast0"].shape))
    if w == 1:
        assert np.signbit(out["bcast0"][0, 1]).all()      # one wave: a readlane, the sign of -0.0 survives
    lo, hi = x[:, :, rows["lo_src"]], x[:, :, rows["hi_src"]]
    below, above = out["below"], out["above"]
    assert np.array_equal(below[..., 1:], lo[..., :-1]) and np.all(below[..., 0] == 0.0)
    assert np.array_equal(above[..., :-1], hi[..., 1:]) and np.all(above[..., t - 1] == 0.0)
    for wave in range(1, w):    # the hand-over at every wave edge, spelled out
        assert np.array_equal(below[..., 64 * wave], lo[..., 64 * wave - 1]), wave
        assert np.array_equal(above[..., 64 * wave - 1], hi[..., 64 * wave]), wave


def test_wave_sum6_totals_equal_the_order_model(probe):
    rs = np.random.RandomState(340)
    x = np.concatenate([make(rs, (16, 6, 64)) for make in (_randn, M.wide_range_vectors, M.cancellation_vectors,
                                                           M.knife_edge_vectors)])
    got = probe.sum6(x)
    _assert_same_bits(got.ravel(), M.wave_sum6(x).ravel(), "wave_sum6_totals")
    worst = 0.0
    for b in range(x.shape[0]):
        for k in range(6):
            s, mag = M.exact_sum(x[b, k])
            err, bound = abs(mpf(float(got[b, k])) - s), 63 * M.U * mag
            assert err <= bound, (b, k)
            worst = max(worst, float(err / bound))
    print("wave_sum6_totals: at most %.3f of 63 u sum |x| from the exact sum" % worst)


# ---- U-turn predicates -----------------------------------------------------------------------------------------------------
def _uturn_cases(rs, w):
    """[(label, d2[2, T], d6[6, T], want2, want6)]: want None = ask the order model (knife edge)."""
    t = 64 * w

    def pos(k):
        return np.abs(rs.randn(k, t)) + 0.1

    cases = [("all positive", pos(2), pos(6), False, False)]
    for k in range(6):      # only slot k non-positive: a wrong ballot row or a dropped slot answers False
        d2, d6 = pos(2), pos(6)
        d6[k] = -d6[k]
        d2[k % 2] = -d2[k % 2]
        cases.append(("only slot %d negative" % k, d2, d6, True, True))
    for k in range(6):      # the same, decided by ONE lane of the last wave against small positive partials elsewhere
        d2, d6 = pos(2), pos(6)
        d6[k, t - 1] = -2.0 * d6[k].sum()
        d2[k % 2, t - 1] = -2.0 * d2[k % 2].sum()
        cases.append(("slot %d negative through its last thread" % k, d2, d6, True, True))
    for zero in (0.0, -0.0):
        for k in (0, 1, 5):
            d2, d6 = pos(2), pos(6)
            d6[k] = zero
            d2[k % 2] = zero
            cases.append(("slot %d sums to %r" % (k, zero), d2, d6, True, True))
    for k in range(6):      # NaN <= 0 is false, like numpy's <=
        d2, d6 = pos(2), pos(6)
        d6[k, rs.randint(t)] = np.nan
        d2[k % 2, rs.randint(t)] = np.nan
        cases.append(("NaN in slot %d" % k, d2, d6, False, False))
    for k in range(6):      # unambiguous sums of mixed signs: the exact sign decides
        d2, d6 = pos(2), pos(6)
        v = rs.randn(t)
        v -= v.mean() - (0.5 if k % 2 else -0.5)       # exact sum ~ +-0.5 t, far beyond the rounding of any order
        d6[k] = v
        d2[k % 2] = v
        neg = math.fsum(v) <= 0.0
        cases.append(("slot %d mixed signs, exact sum %s" % (k, "negative" if neg else "positive"), d2, d6, neg, neg))
    for rep in range(12):   # knife edge: the sign is the summation order's
        k = rep % 6
        d2, d6 = pos(2), pos(6)
        d6[k] = M.knife_edge_vectors(rs, (t,))
        d2[k % 2] = M.knife_edge_vectors(rs, (t,))
        cases.append(("knife edge in slot %d" % k, d2, d6, None, None))
    return cases


@pytest.mark.parametrize("w", P.TEAM_WIDTHS)
def test_uturn_predicates(probe, w):
    rs = np.random.RandomState(360 + w)
    cases = _uturn_cases(rs, w)
    rows = probe.TEAM_ROWS
    x = rs.randn(len(cases), 2, P.TEAM_N_IN, 64 * w)
    for b, (_label, d2, d6, _w2, _w6) in enumerate(cases):
        x[b, :, list(rows["np2"])] = d2[:, None]
        x[b, :, list(rows["np6"])] = d6[:, None]
    out = probe.team(w, x)
    model2 = M.team_any_nonpositive(x[:, :, list(rows["np2"])], w, M.wave_sum2)
    model6 = M.team_any_nonpositive(x[:, :, list(rows["np6"])], w, M.wave_sum6)
    flips = 0
    for b, (label, d2, d6, want2, want6) in enumerate(cases):
        if want2 is None:
            want2, want6 = bool(model2[b, 0]), bool(model6[b, 0])
            flips += want6 != bool((M.left_to_right(d6) <= 0.0).any())
        else:
            assert (bool(model2[b, 0]), bool(model6[b, 0])) == (want2, want6), ("the model disagrees with the case", label)
        for r in range(2):
            for wave in range(w):
                assert out["np2"][b, r, wave] == float(want2), ("any_nonpositive2", w, label, r, wave)
                assert out["np6"][b, r, wave] == float(want6), ("any_nonpositive6", w, label, r, wave)
    print("Team<%d> U-turn predicates: %d cases; %d of 12 knife-edge answers differ from a left-to-right sum's" % (w, len(cases), flips))


# ---- densities ---------------------------------------------------------------------------------------------------------------
FAMILY_LIST = ("std_normal", "diag_gaussian", "ar1", "funnel", "normal1d")


def _dims(ns, w):
    dpad = 64 * ns * w
    dims = {d for d in (1, 2, 63, 64, 65, dpad - 1, dpad) if 1 <= d <= dpad}
    for wave in range(1, w):          # one element past each wave edge: the last wave in use owns exactly one element
        dims.add(64 * ns * wave + 1)
    return sorted(dims)


def _rows_kept(family, q, d, dpad):
    """All rows of an input set up to 2048 elements, and beyond at d = dpad - 1 and dpad. At the wave-edge dimensions beyond
    2048: randn and the wide range with zeros, and of the funnel's v list the two ends that reach the exponential's edges
    and the middle (-700.5, 0, 701)."""
    if d <= 2048 or d in (dpad - 1, dpad):
        return q
    return q[[0, 3, 7]] if q.shape[0] == len(M.FUNNEL_V) else q[[0, 2]]


def _engine_target(family, d, params):
    if family == "std_normal":
        return T.StdNormal(d)
    if family == "diag_gaussian":
        return T.DiagGaussian(params)
    if family == "ar1":
        tgt = T.AR1(d)
        tgt.params = np.ascontiguousarray(params, dtype=np.float64)
        return tgt
    if family == "funnel":
        return T.Funnel(d)
    return T.Normal1D(*params)


def _engine_unit_ns(d):
    ns = 1
    while 64 * ns < d:
        ns *= 2
    return ns


def _nan_equal_bits(a, b):
    return np.array_equal(_bits(a), _bits(b)) or (np.isnan(a).all() and np.isnan(b).all())


@pytest.mark.parametrize("ns,w", P.LOGP_SHAPES)
def test_densities_against_mpmath(probe, ns, w):
    """logp_grad of every built-in functor as <NS = ns> on Team<w> -- every (NS, W) the product instantiates -- against the
    formulas of oracle/targets.py in mpmath, within the per-entry bounds of _primitive_models.density_reference, at
    d in {1, 2, 63, 64, 65, 64 NS W - 1, 64 NS W} and one element past each wave edge, on inputs beyond randn (magnitudes
    1e-150 ... 1e150, signed zeros, AR1 rho in {+-0.999, 0}, precisions spanning 1e+-12, the funnel's v list). Every wave
    holds the same logp; padding slots of g are exactly 0; with one wave the probe's bits are Engine.logp_dlogp's.
    The mpmath reference costs seconds per row of 16384 elements, so beyond 2048 elements fewer rows run (_rows_kept); every
    family, every parameter set and every d still does."""
    worst = {}
    for family in FAMILY_LIST:
        for d in ([1] if family == "normal1d" else _dims(ns, w)):
            for label, params, q in M.density_inputs(family, d, np.random.RandomState(7000 + 131 * d + ns + w)):
                q = _rows_kept(family, q, d, 64 * ns * w)
                logp, g = probe.logp_grad(family, ns, w, q, params)
                tag = "%s <%d,%d> d=%d %s" % (family, ns, w, d, label)
                for wave in range(1, w):
                    assert _nan_equal_bits(logp[:, wave], logp[:, 0]), (tag, "wave %d holds another logp" % wave)
                assert np.all(g[:, d:] == 0.0), (tag, "padding slots of g are not exactly 0")
                for c in range(q.shape[0]):
                    ref = M.density_reference(family, q[c], params)
                    ratio, where = M.density_check(ref, logp[c, 0], g[c, :d])
                    assert ratio <= 1.0, (tag, "row %d" % c, "logp" if where < 0 else "g[%d]" % where, ratio,
                                          float(logp[c, 0]), float(ref[0]))
                    worst[family] = max(worst.get(family, 0.0), ratio)
                if w == 1 and _engine_unit_ns(d) == ns:    # the unit kernel of this very shape: the same bits
                    with lmc.Engine(_engine_target(family, d, params), chains=q.shape[0]) as eng:
                        elogp, egrad = eng.logp_dlogp(q)
                    assert np.array_equal(_bits(elogp), _bits(logp[:, 0])), (tag, "Engine.logp_dlogp: other logp bits")
                    assert np.array_equal(_bits(egrad), _bits(g[:, :d])), (tag, "Engine.logp_dlogp: other gradient bits")
    for family in FAMILY_LIST:
        print("<%d,%d> %s: worst error / bound %.3f" % (ns, w, family, worst.get(family, 0.0)))


@pytest.mark.parametrize("ns,w", [(1, 1), (4, 1), (4, 2), (4, 4), (2, 16)])
def test_densities_nonfinite_positions(probe, ns, w):
    """A non-finite q: logp is non-finite exactly when the reference's is (numpy's statement of the formula: with an inf or
    a NaN anywhere in q it always is), and stays finite for the finite rows next to it. This is where exp_uniform_fast of
    +-inf / NaN and the clamp's handling of NaN matter."""
    from oracle import targets as OT

    dpad = 64 * ns * w
    d = dpad - 1 if dpad > 1 else 1
    rs = np.random.RandomState(7100 + ns + w)
    spots = sorted(e for e in {0, 1, d // 2, 64 * ns - 1, 64 * ns, d - 1} if e < d)
    for family in FAMILY_LIST:
        dd = 1 if family == "normal1d" else d
        params = {"diag_gaussian": 10.0 ** rs.uniform(-2, 2, dd), "ar1": M.ar1_params(0.9), "normal1d": np.array([0.5, 2.0])}.get(family, np.zeros(0))
        rows = [rs.randn(dd)]
        for e in ([0] if dd == 1 else spots):
            for bad in (np.inf, -np.inf, np.nan):
                q = rs.randn(dd)
                q[e] = bad
                rows.append(q)
        q = np.stack(rows)
        logp, _g = probe.logp_grad(family, ns, w, q, params)
        f = OT.DiagGaussian(params) if family == "diag_gaussian" else OT.make(family, dd, rho=0.9, loc=0.5, scale=2.0)
        for c in range(q.shape[0]):
            with np.errstate(all="ignore"):
                want = float(np.ravel(f(q[c])[0])[0])
            for wave in range(w):
                assert np.isfinite(logp[c, wave]) == np.isfinite(want), (family, ns, w, c, q[c][~np.isfinite(q[c])], logp[c], want)
        assert np.isfinite(logp[0]).all() and not np.isfinite(logp[1:]).any(), family
