"""-m gpu: simulation-based calibration of whole tuned jobs of the GLM kernels (littlemcmc_amd/sbc.py). 256 posteriors of
simulated data, 3 chains each, in ONE Batched job of 768 chains x 213 iterations at d = 3; the rank of every true coefficient
among its 63 kept draws is one pass of lmc_diag_threshold_counts over the trace in HBM.

The two bounds are conditions, not measurements. A correct sampler gives p-values that are uniform, so the smallest of three
lies below 1e-4 with probability 3e-4 per case; the negative control -- a fitted model that is not the simulating one -- is
what shows that the test can fail, and clears 1e-6 by many orders of magnitude. The same recipe through the numpy restatement
of the reference (3 chains per simulation) gave

    likelihood   calibrated p per coefficient   control p at most   divergences
    gaussian     0.80 / 0.70 / 0.44             7e-17               0
    bernoulli    0.24 / 0.46 / 0.85             1e-42               0
    poisson      0.55 / 0.37 / 0.28             2e-22               0

The device seeds every chain differently, so its p-values differ; the bounds do not depend on that."""
import numpy as np
import pytest

from littlemcmc_amd import sbc

pytestmark = pytest.mark.gpu

SETTINGS = dict(sims=256, chains_per_sim=3, kept=21, thin=3, tune=150, bins=8, random_seed=20260101)
CASES = {
    "gaussian": (20, dict(prior_scale=1.5, sigma=0.7), {"sigma": 1.4}),
    "bernoulli": (40, dict(prior_scale=1.0), {"prior_scale": 0.3}),
    "poisson": (40, dict(prior_scale=0.5), {"prior_scale": 0.15}),
}


def design(N):
    X = np.random.RandomState(1000).standard_normal((N, 3))
    X[:, 0] = 1
    return X


def report(name, out):
    print("%s: p = %s, chi2 = %s, ecdf_max_dev = %s, divergences = %d, ties = %d\n  rank histogram (coefficient x bin): %s"
          % (name, ["%.3g" % v for v in out["p_value"].tolist()], ["%.1f" % v for v in out["chi2"].tolist()],
             ["%.3f" % v for v in out["ecdf_max_dev"].tolist()], int(out["n_diverging"].sum()), int(out["ties"].sum()),
             out["counts"].tolist()))


@pytest.mark.parametrize("likelihood", sorted(CASES))
def test_the_sampler_is_calibrated(likelihood):
    N, sim, _fit = CASES[likelihood]
    out = sbc.sbc_glm(design(N), likelihood, **SETTINGS, **sim)
    report(likelihood + " calibrated", out)
    assert out["n_draws"] == 63 and tuple(out["ranks"].shape) == (256, 3) and int(out["counts"].sum()) == 3 * 256
    assert float(out["p_value"].min()) >= 1e-4
    assert int(out["n_diverging"].sum()) == 0


@pytest.mark.parametrize("likelihood", sorted(CASES))
def test_the_control_is_not(likelihood):
    N, sim, fit = CASES[likelihood]
    out = sbc.sbc_glm(design(N), likelihood, fit=fit, **SETTINGS, **sim)
    report(likelihood + " control", out)
    assert float(out["p_value"].max()) <= 1e-6
