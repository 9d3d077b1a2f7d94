"""No-GPU checks of the pointwise predictive pass (littlemcmc_amd/predictive.py): the numpy model of the kernel's planes
against the 50-digit reference within the derived bound (tests/_predictive_model.py), the merge rule, the host logic
through ``stats_fn`` with the numpy model injected, and the definitions (constants, the n - 1) against a closed form."""
import ctypes
import math

import numpy as np
import pytest
import torch

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi, predictive
from littlemcmc_amd import targets as T

from . import _glm_model as G
from . import _predictive_model as P

SHAPES = ((1, 1), (63, 3), (65, 65))
DRAWS = 17


def _case(N, d, lik):
    X, y, _Q = G.case(N, d, lik)
    return X, y, P.draws_of(N, d, lik, DRAWS), G.SIGMA ** -2


@pytest.mark.parametrize("lik", G.LIKELIHOODS)
@pytest.mark.parametrize("N,d", SHAPES)
def test_numpy_model_within_bound_of_reference(N, d, lik):
    X, y, draws, isig2 = _case(N, d, lik)
    P.check_planes(P.planes(X, y, draws, lik, isig2), P.case_reference(N, d, lik, DRAWS), what="%s N=%d d=%d" % (lik, N, d))


@pytest.mark.parametrize("lik", G.LIKELIHOODS)
@pytest.mark.parametrize("N,d", SHAPES)
def test_merge_of_split_draws_within_bound(N, d, lik):
    X, y, draws, isig2 = _case(N, d, lik)
    ref = P.case_reference(N, d, lik, DRAWS)
    lo, mu = P.loglik_mu(X, y, draws, lik, isig2)
    rng = np.random.default_rng(5 + N + d)
    for parts in (2, 3, 5):
        for _rep in range(3):   # "any split": random cut points, and one with an empty part
            cuts = [0] + sorted(rng.integers(0, DRAWS + 1, parts - 1).tolist()) + [DRAWS]
            acc = P.planes_of(lo[:0], mu[:0])
            for a, b in zip(cuts[:-1], cuts[1:]):
                acc = P.merge(acc, P.planes_of(lo[a:b], mu[a:b]))
            assert acc[0, 0] == DRAWS
            P.check_planes(acc, ref, what="%s split %s" % (lik, cuts))
    # an empty part changes nothing, bit for bit -- on either side, whatever it holds
    whole, empty = P.planes_of(lo, mu), P.planes_of(lo[:0], mu[:0])
    junk = empty.copy()
    junk[1:] = np.nan
    for e in (empty, junk):
        assert np.array_equal(P.merge(whole, e), whole, equal_nan=True) and np.array_equal(P.merge(e, whole), whole, equal_nan=True)


def test_merge_guards_minus_infinity_and_carries_nan():
    """-inf draws do not turn a finite lppd into NaN (both sides -inf: m = -inf, S = 0), and a NaN stays."""
    inf = np.inf
    mk = lambda n, m, S, mean, M2, mu: np.array([[n], [m], [S], [mean], [M2], [mu]], dtype=np.float64)   # noqa: E731
    a, b = mk(2, -inf, 0.0, -inf, np.nan, inf), mk(3, -1.0, 2.5, -2.0, 1.0, 3.0)
    for got in (P.merge(a, b), P.merge(b, a)):
        assert got[0, 0] == 5 and got[1, 0] == -1.0 and got[2, 0] == 2.5
    both = P.merge(a, a)
    assert both[1, 0] == -inf and both[2, 0] == 0.0
    bad = mk(1, -1.0, np.nan, np.nan, np.nan, np.nan)
    assert np.isnan(P.merge(b, bad)[2, 0]) and np.isnan(P.merge(bad, b)[2, 0])
    lo = np.array([[-inf, -1.0], [-2.0, np.nan], [-3.0, -inf]])
    pl = P.planes_of(lo, np.ones_like(lo))
    assert pl[1, 0] == -2.0 and pl[2, 0] == 1.0 + math.exp(-1.0) and np.isnan(pl[1:, 1]).all()


def _batched(G_=3, N=5, d=3, lik="gaussian", seed=0):
    rng = np.random.default_rng(seed)
    ms = []
    for g in range(G_):
        X = rng.standard_normal((N, d))
        y = {"gaussian": rng.standard_normal(N), "poisson": rng.poisson(2.0, N).astype(float),
             "bernoulli": (rng.random(N) < 0.5).astype(float)}[lik]
        ms.append(T.GLM(X, y, lik, prior_scale=1.0 + g, sigma=0.5 + g))
    return T.Batched(ms)


def test_host_logic_shapes_blocks_and_held_out_data():
    tgt = _batched()
    rng = np.random.default_rng(1)
    x = torch.as_tensor(rng.standard_normal((3 * 4, 6, 3)))
    st = tgt.pointwise_stats(x, stats_fn=P.stats_fn)
    assert all(st[k].shape == (3, 5) and st[k].dtype == torch.float64 for k in predictive.PLANES)
    assert torch.equal(st["n"], torch.full((3, 5), 24.0, dtype=torch.float64))
    for g in range(3):   # each group: its own member's data, its own chains
        m = tgt[g]
        want = P.planes(m.X, m.y, x[4 * g:4 * g + 4].reshape(-1, 3).numpy(), "gaussian", m.isig2)
        assert all(np.array_equal(st[k][g].numpy(), want[i]) for i, k in enumerate(predictive.PLANES))
    # a list of two blocks cut inside group 1 == the single block, within the bound
    two = tgt.pointwise_stats([x[:6], x[6:]], stats_fn=P.stats_fn)
    for g in range(3):
        m = tgt[g]
        ref = P.reference_loglik(m.X, m.y, x[4 * g:4 * g + 4].reshape(-1, 3).numpy(), "gaussian", m.isig2)
        P.check_planes(np.stack([two[k][g].numpy() for k in predictive.PLANES]), ref, what="two blocks, group %d" % g)
    assert torch.equal(two["n"], st["n"]) and torch.equal(two["m"], st["m"])
    assert torch.equal(two["S"][0], st["S"][0]) and torch.equal(two["M2"][2], st["M2"][2])   # groups inside one block: untouched
    # a block that starts inside the job: groups 1 and 2 only, the first one partly
    part = tgt.pointwise_stats(x[6:], chains_per_group=4, first_chain=6, stats_fn=P.stats_fn)
    assert part["n"].shape == (2, 5) and part["first_group"] == 1 and float(part["n"][0, 0]) == 12.0 and float(part["n"][1, 0]) == 24.0
    # one GLM: a leading axis of 1, kept
    one = tgt[1].waic(x[:2], stats_fn=P.stats_fn)
    assert one["lppd"].shape == (1, 5) and one["elpd_waic"].shape == (1,) and one["n_high_variance"].shape == (1,)
    # held-out data with another N
    data = [(rng.standard_normal((7, 3)), rng.standard_normal(7)) for _ in range(3)]
    held = tgt.waic(x, data=data, stats_fn=P.stats_fn)
    assert held["lppd"].shape == (3, 7) and held["p_waic"].shape == (3, 7) and held["se"].shape == (3,)
    m = tgt[2]
    want = P.planes(data[2][0], data[2][1], x[8:].reshape(-1, 3).numpy(), "gaussian", m.isig2)
    lppd = want[1] + np.log(want[2]) - math.log(24.0) - math.log(m.sigma) - 0.5 * math.log(2 * math.pi)
    np.testing.assert_allclose(held["lppd"][2].numpy(), lppd, rtol=0, atol=1e-13)
    full = tgt.waic(x, stats_fn=P.stats_fn)
    np.testing.assert_array_equal(full["elpd_waic_i"].numpy(), (full["lppd"] - full["p_waic"]).numpy())
    np.testing.assert_allclose(full["p_waic"].numpy(), (st["M2"] / 23.0).numpy(), rtol=1e-15)
    np.testing.assert_allclose(full["elpd_waic"].numpy(), full["elpd_waic_i"].sum(dim=1).numpy(), rtol=1e-14)
    np.testing.assert_allclose(full["se"].numpy(), np.sqrt(5 * full["elpd_waic_i"].numpy().var(axis=1, ddof=1)), rtol=1e-13)
    assert torch.equal(full["waic"], -2.0 * full["elpd_waic"])
    assert torch.equal(full["n_high_variance"], (full["p_waic"] > 0.4).sum(dim=1))
    np.testing.assert_allclose(full["mu_mean"].numpy(), (st["sum_mu"] / 24.0).numpy(), rtol=1e-15)
    assert lmc.predictive is predictive


def test_loglik_constant_closed_forms():
    X = np.ones((4, 1))
    assert np.array_equal(T.GLM(X, [0, 1, 1, 0], "bernoulli").loglik_constant(), np.zeros(4))
    y = np.array([0.0, 1.0, 4.0, 11.0])
    np.testing.assert_array_equal(T.GLM(X, y, "poisson").loglik_constant(), [-math.lgamma(v + 1.0) for v in y])
    assert abs(T.GLM(X, y, "poisson").loglik_constant()[2] + math.log(24.0)) < 1e-15
    np.testing.assert_array_equal(T.GLM(X, y, "poisson").loglik_constant(y=[2.0, 3.0]), [-math.lgamma(3.0), -math.lgamma(4.0)])
    c = T.GLM(X, y, "gaussian", sigma=2.5).loglik_constant()
    assert c.shape == (4,) and np.all(c == -math.log(2.5) - 0.5 * math.log(2.0 * math.pi))
    # l + const is a normalised log density: the poisson masses sum to one, the gaussian density integrates to one
    t = T.GLM(np.ones((60, 1)), np.arange(60.0), "poisson")
    eta = 0.7
    assert abs(np.exp(t.y * eta - math.exp(eta) + t.loglik_constant()).sum() - 1.0) < 1e-12
    grid = np.linspace(-30, 30, 60001)
    dens = np.exp(-0.5 * (grid - 0.3) ** 2 / 2.5 ** 2 + c[0])
    assert abs(dens.sum() * (grid[1] - grid[0]) - 1.0) < 1e-9


def test_refusals():
    tgt = _batched()
    x = torch.zeros((12, 4, 3), dtype=torch.float64)
    with pytest.raises(TypeError, match="GLM"):
        predictive.pointwise_stats(x, T.StdNormal(3), stats_fn=P.stats_fn)
    with pytest.raises(TypeError, match="GLM"):
        predictive.waic(x, T.Batched([T.StdNormal(3), T.StdNormal(3)]), stats_fn=P.stats_fn)
    if not torch.cuda.is_available():
        with pytest.raises(_abi.HipLibraryError):      # CPU tensors: there is no host implementation
            tgt.pointwise_stats(x)
        with pytest.raises(_abi.HipLibraryError):
            tgt[0].waic(x[:4])
    with pytest.raises(ValueError, match="first_chain"):
        tgt.pointwise_stats([x[:6], x[6:]], first_chain=2, stats_fn=P.stats_fn)
    with pytest.raises(ValueError, match="group"):
        tgt.pointwise_stats(x, group=object(), stats_fn=P.stats_fn)
    with pytest.raises(ValueError, match="multiple"):
        tgt.pointwise_stats(x[:11], stats_fn=P.stats_fn)
    with pytest.raises(ValueError, match="d = "):
        tgt.pointwise_stats(torch.zeros((12, 4, 2), dtype=torch.float64), stats_fn=P.stats_fn)
    with pytest.raises(ValueError, match="reach group"):
        tgt.pointwise_stats(x, chains_per_group=2, stats_fn=P.stats_fn)
    with pytest.raises(ValueError, match="chains_per_group"):
        tgt.pointwise_stats(x, chains_per_group=0, stats_fn=P.stats_fn)
    rng = np.random.default_rng(0)
    ok = (rng.standard_normal((6, 3)), rng.standard_normal(6))
    with pytest.raises(ValueError, match="pairs"):
        tgt.waic(x, data=[ok, ok], stats_fn=P.stats_fn)
    with pytest.raises(ValueError, match="d = "):
        tgt.waic(x, data=[ok, ok, (rng.standard_normal((6, 2)), ok[1])], stats_fn=P.stats_fn)
    with pytest.raises(ValueError, match="common N"):
        tgt.waic(x, data=[ok, ok, (rng.standard_normal((5, 3)), ok[1][:5])], stats_fn=P.stats_fn)
    bern = _batched(lik="bernoulli")
    with pytest.raises(ValueError, match="0 or 1"):   # y validated as GLM.__init__ validates it
        bern.waic(x, data=[ok, ok, ok], stats_fn=P.stats_fn)
    with pytest.raises(ValueError, match="pair"):
        tgt[0].waic(x[:4], data=[ok, ok, ok], stats_fn=P.stats_fn)


def test_c_entry_refuses_before_any_hip_call():
    """The argument checks of lmc_glm_pointwise need no GPU: they come before the first HIP call."""
    lib = _abi.load()
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    d, N = 3, 5
    row_len = T.glm_row_layout(N, d)["size"]

    def call(x=p, chains=4, stride=10, dim=d, t0=0, n=10, rows=p, row_len=row_len, n_rows=2, first=0, per=2, out=p):
        return lib.lmc_glm_pointwise(x, chains, stride, dim, t0, n, rows, row_len, n_rows, first, per, out, None)

    for kw in (dict(x=None), dict(rows=None), dict(out=None), dict(chains=0), dict(chains=2 ** 31), dict(dim=0), dict(n=0),
               dict(t0=-1), dict(t0=1), dict(first=-1), dict(per=0), dict(first=2 ** 31), dict(dim=_abi.GLM_MAX_DIM + 1),
               dict(row_len=row_len + 2), dict(row_len=8), dict(row_len=T.glm_row_layout(N, 9)["size"]), dict(n_rows=1),
               dict(n_rows=0), dict(first=1), dict(per=1)):
        assert call(**kw) == 1, kw   # LMC_ERR_INVALID


def test_definitions_against_the_gaussian_closed_form():
    """lppd_n -> log N(y_n; x_n'm, sigma^2 + v_n) and p_waic_n -> (2 v_n^2 + 4 v_n delta_n^2) / (4 sigma^4) for iid draws of
    the exact gaussian posterior (v_n = x_n' Sigma x_n, delta_n = y_n - x_n'm): within 5 Monte-Carlo standard errors, the
    errors taken from the same draws (delta method for the log of a mean; the standard error of a variance from the fourth
    central moment). Pins the constants and the n - 1. The seed is fixed: the test is deterministic."""
    rng = np.random.default_rng(20261019)
    N, d, S, sigma = 8, 3, 20000, 0.7
    X = rng.standard_normal((N, d))
    y = X @ np.array([1.0, -0.5, 0.25]) + sigma * rng.standard_normal(N)
    tgt = T.GLM(X, y, "gaussian", prior_scale=2.0, sigma=sigma)
    mean, cov = tgt.posterior_gaussian()
    draws = rng.multivariate_normal(mean, cov, size=S)
    out = tgt.waic(torch.as_tensor(draws.reshape(4, S // 4, d)), stats_fn=P.stats_fn)
    v = np.einsum("ne,ef,nf->n", X, cov, X)
    delta = y - X @ mean
    lppd_exact = -0.5 * np.log(2 * np.pi * (sigma ** 2 + v)) - 0.5 * delta ** 2 / (sigma ** 2 + v)
    p_exact = (2 * v ** 2 + 4 * v * delta ** 2) / (4 * sigma ** 4)
    # Monte-Carlo standard errors from the same draws
    ll = -0.5 * (y - draws @ X.T) ** 2 / sigma ** 2 - math.log(sigma) - 0.5 * math.log(2 * math.pi)   # [S, N]
    dens = np.exp(ll)
    se_lppd = dens.std(axis=0, ddof=1) / math.sqrt(S) / dens.mean(axis=0)
    c = ll - ll.mean(axis=0)
    m2, m4 = (c ** 2).mean(axis=0), (c ** 4).mean(axis=0)
    se_p = np.sqrt((m4 - m2 ** 2) / S)
    got_l, got_p = out["lppd"][0].numpy(), out["p_waic"][0].numpy()
    assert float(out["n_draws"][0, 0]) == S
    assert np.all(np.abs(got_l - lppd_exact) <= 5 * se_lppd), (got_l - lppd_exact) / se_lppd
    assert np.all(np.abs(got_p - p_exact) <= 5 * se_p), (got_p - p_exact) / se_p
    # the n - 1: the reported p_waic is the unbiased variance of the same draws' l
    np.testing.assert_allclose(got_p, ll.var(axis=0, ddof=1), rtol=1e-9)
    assert abs(float(out["elpd_waic"][0]) - (got_l - got_p).sum()) < 1e-12


def test_the_closed_form_orders_the_prior_scale_ladder():
    """The fixture of the GPU end-to-end test: under the exact posteriors the 0.1 rung has the lowest elpd_waic, by several
    of the standard errors WAIC itself reports, so that test may rely on the ordering."""
    X, y, _Xn, _yn, sigma = P.ladder()
    elpd, se = [], []
    for s in P.LADDER_SCALES:
        lppd, p = P.gaussian_closed_form(T.GLM(X, y, "gaussian", prior_scale=s, sigma=sigma))
        e = lppd - p
        elpd.append(e.sum())
        se.append(math.sqrt(len(e) * e.var(ddof=1)))
    assert int(np.argmin(elpd)) == 0
    assert min(elpd[1:]) - elpd[0] > 3 * max(se), (elpd, se)
