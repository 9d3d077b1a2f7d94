"""No-GPU tests of littlemcmc_amd/sbc.py: the simulation pinned to its RNG order, the uniformity test against scipy, and
sbc_glm on EXACT posterior draws (the closed form of the gaussian GLM) with the numpy model of the count injected -- calibrated
when the fitted model is the simulating one, far from it for the negative control."""
import numpy as np
import pytest
import scipy.stats
import torch

import littlemcmc_amd as lmc
from littlemcmc_amd import sbc
from tests import _threshold_model as M


def design(N, d=3):
    X = np.random.RandomState(1000).standard_normal((N, d))
    X[:, 0] = 1
    return X


def test_simulate_glm_is_pinned_to_its_rng_order():
    X = design(20)
    for lik, kw in (("gaussian", dict(prior_scale=1.5, sigma=0.7)), ("bernoulli", dict(prior_scale=1.0)),
                    ("poisson", dict(prior_scale=0.5))):
        q, y = sbc.simulate_glm(X, lik, 11, random_seed=5, **kw)
        rs = np.random.RandomState(5)
        q_want = kw["prior_scale"] * rs.standard_normal((11, 3))
        eta = q_want @ X.T
        if lik == "gaussian":
            y_want = eta + kw["sigma"] * rs.standard_normal((11, 20))
        elif lik == "bernoulli":
            y_want = rs.random_sample((11, 20)) < 1 / (1 + np.exp(-eta))
        else:
            y_want = rs.poisson(np.exp(eta))
        np.testing.assert_array_equal(q, q_want)
        np.testing.assert_array_equal(y, y_want)
        assert y.dtype == np.float64 and q.shape == (11, 3) and y.shape == (11, 20)
    # a design per simulation: the same calls, eta per simulation
    Xg = np.random.RandomState(2).standard_normal((4, 20, 3))
    q, y = sbc.simulate_glm(Xg, "gaussian", 4, sigma=0.5, random_seed=9)
    rs = np.random.RandomState(9)
    q_want = rs.standard_normal((4, 3))
    np.testing.assert_array_equal(q, q_want)
    np.testing.assert_allclose(y, np.stack([Xg[g] @ q_want[g] for g in range(4)]) + 0.5 * rs.standard_normal((4, 20)), rtol=1e-13)
    for bad in (dict(likelihood="probit"), dict(X=np.zeros(3)), dict(X=np.zeros((3, 20, 3))), dict(sims=0)):
        with pytest.raises(ValueError):
            sbc.simulate_glm(**dict(dict(X=X, likelihood="gaussian", sims=4), **bad))
    assert lmc.sbc is sbc


def test_rank_uniformity_against_scipy():
    rs = np.random.RandomState(3)
    G, L = 256, 64
    ranks = np.stack([rs.randint(0, L, G),                               # uniform
                      np.minimum(rs.randint(0, L, G), rs.randint(0, L, G)),   # piled up at the low ranks
                      np.full(G, 63),                                     # all in the last bin: p underflows to 0
                      np.repeat(np.arange(L), G // L)], axis=1)           # exactly flat: chi2 = 0, p = 1
    out = sbc.rank_uniformity(ranks, L - 1, bins=8)
    counts = np.stack([np.bincount(ranks[:, j] // 8, minlength=8) for j in range(4)])
    np.testing.assert_array_equal(out["counts"].numpy(), counts)
    chi2 = ((counts - 32.0) ** 2 / 32.0).sum(axis=1)
    np.testing.assert_allclose(out["chi2"].numpy(), chi2, rtol=1e-14)
    np.testing.assert_allclose(out["p_value"].numpy(), scipy.stats.chi2.sf(chi2, 7), rtol=1e-12)
    assert out["p_value"].dtype == torch.float64 and out["p_value"][3] == 1.0 and 0 <= out["p_value"][2] < 1e-200
    for j in range(4):
        ecdf = np.array([(ranks[:, j] <= r).mean() for r in range(L)])
        np.testing.assert_allclose(out["ecdf_max_dev"][j].item(), np.abs(ecdf - (np.arange(L) + 1.0) / L).max(), rtol=0, atol=1e-15)
    assert out["ecdf_max_dev"][3] == 0.0
    # the p-value over its range, from 1 down to 1e-31: the regularised upper incomplete gamma function in float64
    x2 = torch.tensor([0.0, 1.0, 7.0, 30.0, 100.0, 160.0], dtype=torch.float64)
    p = torch.special.gammaincc(torch.full_like(x2, 3.5), x2 / 2)
    np.testing.assert_allclose(p.numpy(), scipy.stats.chi2.sf(x2.numpy(), 7), rtol=1e-12)
    assert p[-1] < 1e-30
    for n_draws, bins in ((63, 7), (62, 8), (63, 1), (0, 8)):
        with pytest.raises(ValueError, match="bins"):
            sbc.rank_uniformity(ranks, n_draws, bins=bins)
    with pytest.raises(ValueError, match="ranks"):
        sbc.rank_uniformity(ranks + 1, L - 1)
    with pytest.raises(ValueError, match="ranks"):
        sbc.rank_uniformity(ranks[:, 0], L - 1)
    with pytest.raises(ValueError, match="bins"):                          # refused before anything is simulated or sampled
        sbc.sbc_glm(design(20), "gaussian", sims=4, chains_per_sim=3, kept=20, draws_fn=lambda t: 1 / 0)


def exact_draws(seed, n=63):
    rs = np.random.RandomState(seed)

    def draws_fn(target):
        """3 chains x 21 exact, independent draws per simulation from the closed-form posterior of every member."""
        out = np.empty((3 * len(target.members), n // 3, target.d))
        for g, m in enumerate(target.members):
            mean, cov = m.posterior_gaussian()
            out[3 * g:3 * g + 3] = rs.multivariate_normal(mean, cov, size=n).reshape(3, n // 3, target.d)
        return torch.from_numpy(out)

    return draws_fn


def test_sbc_glm_on_exact_draws_is_calibrated_and_its_control_is_not():
    X = design(20)
    kw = dict(sims=256, chains_per_sim=3, kept=21, bins=8, prior_scale=1.5, sigma=0.7, random_seed=0, count_fn=M.count_fn)
    out = sbc.sbc_glm(X, "gaussian", draws_fn=exact_draws(1), **kw)
    assert out["n_draws"] == 63 and tuple(out["ranks"].shape) == (256, 3) == tuple(out["ties"].shape)
    assert int(out["ties"].sum()) == 0 and out["n_diverging"].tolist() == [0] * 256
    q_true, _y = sbc.simulate_glm(X, "gaussian", 256, prior_scale=1.5, sigma=0.7, random_seed=0)
    np.testing.assert_array_equal(out["q_true"], q_true)
    assert 0 <= int(out["ranks"].min()) and int(out["ranks"].max()) <= 63
    assert torch.equal(out["counts"], sbc.rank_uniformity(out["ranks"], 63, 8)["counts"])
    print("calibrated p:", out["p_value"].tolist(), "ecdf_max_dev:", out["ecdf_max_dev"].tolist())
    assert float(out["p_value"].min()) >= 1e-4
    ctl = sbc.sbc_glm(X, "gaussian", draws_fn=exact_draws(1), fit={"sigma": 1.4}, **kw)
    print("control p:", ctl["p_value"].tolist())
    assert float(ctl["p_value"].max()) <= 1e-6
    np.testing.assert_array_equal(ctl["q_true"], q_true)                   # the simulation is the same: only the fit differs
