"""The CPU models of the device primitives (tests/_primitive_models.py) against mpmath: what tests/test_gpu_primitives.py
compares the device with bit for bit must itself be right, and the comparison must have teeth.

The bound of exp_uniform_fast. The header claimed "< 1 ulp"; the model refutes that (2.22 ulp at EXP_FAST_REFUTATION), so the
bound is derived from the rounding steps instead, as relative errors in units of eps = 2^-53 (half an ulp at worst):
    table entry RN(2^(j/64))                          <= 1
    the polynomial's last FMA (p ~ 1)                 <= 1
    Taylor truncation r^6/720 at |r| <= ln2/128       <= 0.32   ((ln2/128)^6 / 720 = 3.5e-17)
    the product p t                                   <= 1
    reduction (two FMAs, |r| <= 5.5e-3 scales their error into p) and the inner Horner steps     < 0.05
which sum to < 3.4 eps. One ulp is at least 1 eps of the value (2 eps at the bottom of a binade), so the error is at most
3.4 ulp: the bound is 3.5 ulp. ldexp is exact for normal results; a subnormal result is rounded once more, which adds half a
subnormal spacing: 4.0 there. exp_uniform keeps the header's own figure, 1.5 ulp. Neither is tuned to what any
implementation returns; the maxima observed are printed."""
import math

import numpy as np
import pytest
from mpmath import mp, mpf

from tests import _primitive_models as M


@pytest.fixture(scope="module")
def fast():
    return M.ExpUniformFastModel()


@pytest.fixture(scope="module")
def slow():
    return M.ExpUniformModel()


def test_table_entries_are_correctly_rounded():
    table = M.exp2_table()
    with mp.workprec(200):
        for j, t in enumerate(table):
            assert t == float(mpf(2) ** (mpf(j) / 64)), (j, t)


def test_parsed_constants_are_the_documented_ones(fast, slow):
    ln2 = math.log(2.0)
    assert slow.c[0] == 1.0 / ln2 and fast.c[0] == 64.0 / ln2
    assert (slow.lo, slow.hi) == (-800.0, 800.0)
    with mp.workprec(200):
        assert abs(mpf(slow.c[1]) + mpf(slow.c[2]) - mp.log(2)) < mpf(2) ** -85       # hi + lo carry ln 2 to ~32 extra bits
        assert abs(mpf(fast.c[1]) + mpf(fast.c[2]) - mp.log(2) / 64) < mpf(2) ** -91
    assert slow.c[3:] == [1.0 / math.factorial(k) for k in range(13, 2, -1)]
    assert fast.c[3:] == [1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0]


def _bound_fast(exact):
    return M.EXP_FAST_SUBNORMAL_ULP if exact < 2.0 ** -1022 else M.EXP_FAST_ULP


def test_exp_uniform_model_within_bound(slow):
    rs = np.random.RandomState(101)
    for name, xs in M.exp_arguments(rs, -2000.0, 709.78, 4000, 1).items():   # (709.78, 800]: the overflow test below
        got = [slow(float(x)) for x in xs]
        err = M.ulp_errors(np.maximum(xs, -800.0), got)
        i = int(np.argmax(err))
        print("exp_uniform model, %s: %d arguments, max %.3f ulp at x = %r" % (name, len(xs), err[i], float(xs[i])))
        assert err[i] <= M.EXP_UNIFORM_ULP, (name, float(xs[i]), err[i])


def test_exp_uniform_fast_model_within_bound(fast):
    rs = np.random.RandomState(102)
    for name, xs in M.exp_arguments(rs, -1700.0, 709.78, 6000, 64).items():
        got = [fast(float(x)) for x in xs]
        err = M.ulp_errors(xs, got)
        bound = np.array([_bound_fast(math.exp(x)) for x in xs])
        i = int(np.argmax(err / bound))
        print("exp_uniform_fast model, %s: %d arguments, max %.3f ulp at x = %r" % (name, len(xs), err.max(), float(xs[int(np.argmax(err))])))
        assert err[i] <= bound[i], (name, float(xs[i]), err[i])


def test_exp_uniform_fast_refutes_the_one_ulp_claim(fast):
    """The named case: 2.22 ulp, where lmc_wave.hpp and lmc_targets.hpp said "< 1 ulp"."""
    x = M.EXP_FAST_REFUTATION
    err = M.ulp_errors([x], [fast(x)])[0]
    print("exp_uniform_fast model at %r: %.3f ulp" % (x, err))
    assert 2.2 < err < 2.25
    assert err <= M.EXP_FAST_ULP


def test_exp_models_overflow_and_underflow_exactly(fast, slow):
    for x in (709.79, 710.0, 750.0, 800.0, 801.0, 2000.0):
        assert slow(x) == math.inf, x
    for x in (709.79, 710.0):
        assert fast(x) == math.inf, x
    for x in (-745.14, -746.0, -800.0, -801.0, -2000.0):
        assert slow(x) == 0.0, x
    for x in (-745.14, -746.0, -800.0, -1700.0):
        assert fast(x) == 0.0, x
    for model in (fast, slow):
        assert model(709.78) < math.inf and model(-745.13) == 5e-324
        assert model(0.0) == 1.0 and model(-0.0) == 1.0


@pytest.mark.parametrize("name,fn", [("wave_sum", M.wave_sum), ("wave_sum2", M.wave_sum2), ("wave_sum6", M.wave_sum6)])
def test_reduction_order_models_have_teeth(name, fn):
    """On the cancellation inputs of the GPU test every order model returns other bits than a plain left-to-right sum (and
    than the other models): bit equality with the device can only come from the device's own order. All of them stay within
    the any-order bound of the exact sum."""
    rs = np.random.RandomState(7)
    x = M.cancellation_vectors(rs, (200, 64))
    got = fn(x)
    assert np.mean(got != M.left_to_right(x)) > 0.5          # most vectors tell the orders apart, each of them would do
    for other in (M.wave_sum, M.wave_sum2, M.wave_sum6):
        if other is not fn:
            assert np.mean(got != other(x)) > 0.5, other.__name__
    for row, val in zip(x[:20], got[:20]):
        s, mag = M.exact_sum(row)
        assert abs(mpf(float(val)) - s) <= 63 * M.U * mag


@pytest.mark.parametrize("w", [2, 4, 16])
def test_team_order_model_has_teeth(w):
    rs = np.random.RandomState(8)
    x = M.cancellation_vectors(rs, (200, 64 * w))
    got = M.team_reduce(x, w, M.wave_sum)
    assert np.mean(got != M.left_to_right(x)) > 0.5
    flat_tree = x
    while flat_tree.shape[-1] > 1:
        flat_tree = flat_tree[..., 0::2] + flat_tree[..., 1::2]
    if w == 2:    # two wave totals added ARE the balanced tree over 128 values
        assert np.array_equal(got, flat_tree[..., 0])
    else:         # wave totals added in wave order are not the balanced tree over all 64 w values
        assert np.mean(got != flat_tree[..., 0]) > 0.2


def test_knife_edge_sums_depend_on_the_order():
    rs = np.random.RandomState(9)
    x = M.knife_edge_vectors(rs, (400, 64))
    signs = [np.sign(fn(x)) for fn in (M.wave_sum, M.wave_sum2, M.wave_sum6, M.left_to_right)]
    for a in range(len(signs)):
        for b in range(a + 1, len(signs)):
            assert np.mean(signs[a] != signs[b]) > 0.2, (a, b)
    for row in x[:10]:
        s, mag = M.exact_sum(row)
        assert abs(s) < 1e-15 * mag


def _oracle(family, d, params):
    from oracle import targets as OT

    if family == "diag_gaussian":
        return OT.DiagGaussian(params)
    if family == "ar1":
        f = OT.AR1(d)
        f.c_end, f.c_mid, f.off = params
        return f
    if family == "normal1d":
        return OT.Normal1D(1, *params)
    return OT.make(family, d)


@pytest.mark.parametrize("family", ["std_normal", "diag_gaussian", "ar1", "funnel", "normal1d"])
def test_density_bounds_hold_for_the_numpy_oracle(family):
    """The derived per-entry bounds are any-order bounds: numpy's statement of the same formulas (oracle/targets.py: same
    roundings per term, another summation order, libm's exponential) must meet them too, on the GPU test's input classes."""
    worst = 0.0
    for d in ([1] if family == "normal1d" else [1, 2, 63, 65, 200]):
        for label, params, q in M.density_inputs(family, d, np.random.RandomState(1000 + d)):
            f = _oracle(family, d, params)
            for c in range(q.shape[0]):
                ref = M.density_reference(family, q[c], params)
                with np.errstate(all="ignore"):
                    logp, g = f(q[c])
                ratio, where = M.density_check(ref, float(np.ravel(logp)[0]), np.ravel(g))
                assert ratio <= 1.0, (family, d, label, c, ratio, where)
                worst = max(worst, ratio)
    print("%s: numpy oracle at most %.3f of the bound" % (family, worst))
