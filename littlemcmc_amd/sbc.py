"""Simulation-based calibration (Talts, Betancourt, Simpson, Vehtari, Gelman 2018) of the GLM family: the end-to-end
statistical test of the sampler.

If ``q_true`` is drawn from the prior, ``y`` from the likelihood at ``q_true`` and L draws from the posterior of ``y``, then the
rank of ``q_true[e]`` among the L draws of coefficient e -- the number of draws below it -- is uniform on 0 .. L whenever the
draws come from the right posterior. One posterior per simulated data set, by the hundreds, is the workload of
``targets.Batched([GLM(X, y_g, ...)])``: one job samples them all, and the ranks are ONE pass over its trace in HBM,
``diagnostics.threshold_counts`` with every posterior's own threshold ``q_true[g]``.

The simulation is host numpy on purpose (``simulate_glm``: the order of its RNG calls is its definition) and shares nothing
with the device's replicated-response sampler: it is the independent side of the test. The chains of a posterior are
autocorrelated, so the kept draws are thinned (``thin``) and few (``kept`` per chain); uniformity is tested per coefficient
by a chi-square over ``bins`` equal bins of the L + 1 possible ranks (``rank_uniformity``)."""
import numpy as np
import torch

LIKELIHOODS = ("gaussian", "bernoulli", "poisson")


def simulate_glm(X, likelihood, sims, prior_scale=1.0, sigma=1.0, random_seed=0):
    """``(q_true[G, d], y[G, N])`` of G = ``sims`` simulated data sets (host numpy, float64). ``X`` is [N, d], shared by all
    simulations, or [G, N, d]. The order of the RNG calls is the definition:

        rs = np.random.RandomState(random_seed)
        q_true = prior_scale * rs.standard_normal((G, d))
        eta = q_true @ X.T                                  (per simulation for a [G, N, d] design)
        gaussian:   y = eta + sigma * rs.standard_normal((G, N))
        bernoulli:  y = rs.random_sample((G, N)) < 1 / (1 + exp(-eta))
        poisson:    y = rs.poisson(exp(eta))"""
    X = np.asarray(X, dtype=np.float64)
    G = int(sims)
    if likelihood not in LIKELIHOODS:
        raise ValueError("likelihood must be one of %s (got %r)" % (sorted(LIKELIHOODS), likelihood))
    if G < 1 or X.ndim not in (2, 3) or (X.ndim == 3 and X.shape[0] != G):
        raise ValueError("X must be [N, d] or [%d, N, d] with sims >= 1 (got shape %s, sims=%d)" % (G, X.shape, G))
    N, d = X.shape[-2:]
    rs = np.random.RandomState(random_seed)
    q_true = float(prior_scale) * rs.standard_normal((G, d))
    eta = q_true @ X.T if X.ndim == 2 else np.einsum("gnd,gd->gn", X, q_true)
    if likelihood == "gaussian":
        y = eta + float(sigma) * rs.standard_normal((G, N))
    elif likelihood == "bernoulli":
        y = (rs.random_sample((G, N)) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    else:
        y = rs.poisson(np.exp(eta)).astype(np.float64)
    return q_true, y


def _check_bins(n_draws, bins):
    n_draws, bins = int(n_draws), int(bins)
    if n_draws < 1 or bins < 2 or (n_draws + 1) % bins != 0:
        raise ValueError("the %d possible ranks 0 .. %d must fill %d bins evenly: (n_draws + 1) %% bins == 0, bins >= 2"
                         % (n_draws + 1, n_draws, bins))
    return n_draws, bins


def rank_uniformity(ranks, n_draws, bins=8):
    """Uniformity of SBC ranks per coefficient -> dict(counts[d, bins] int64, chi2[d], p_value[d], ecdf_max_dev[d]) (CPU tensors,
    float64 but for the counts). ``ranks[G, d]`` lie in 0 .. ``n_draws``; the ``n_draws + 1`` possible ranks are cut into
    ``bins`` equal bins, which needs ``(n_draws + 1) % bins == 0`` (ValueError otherwise: unequal bins are not uniform under the
    null). ``chi2 = sum_b (counts_b - G / bins)^2 / (G / bins)`` and ``p_value = Q((bins - 1) / 2, chi2 / 2)``, the upper tail of
    the chi-square distribution with ``bins - 1`` degrees of freedom (``torch.special.gammaincc`` in float64).
    ``ecdf_max_dev`` is ``max_r |ECDF(r) - (r + 1) / (n_draws + 1)|`` over the possible ranks r: the largest distance of the
    ranks' empirical distribution function from the uniform one."""
    n_draws, bins = _check_bins(n_draws, bins)
    r = torch.as_tensor(ranks).detach().cpu().to(torch.int64)
    if r.dim() != 2 or r.shape[0] < 1:
        raise ValueError("ranks must be [G, d] (got shape %s)" % (tuple(r.shape),))
    if int(r.min()) < 0 or int(r.max()) > n_draws:
        raise ValueError("ranks must lie in 0 .. %d (got %d .. %d)" % (n_draws, int(r.min()), int(r.max())))
    G, d = r.shape
    L = n_draws + 1
    hist = torch.zeros((d, L), dtype=torch.int64)
    hist.scatter_add_(1, r.t().contiguous(), torch.ones((d, G), dtype=torch.int64))
    counts = hist.reshape(d, bins, L // bins).sum(dim=2)
    expect = G / bins
    chi2 = ((counts.to(torch.float64) - expect) ** 2).sum(dim=1) / expect
    p_value = torch.special.gammaincc(torch.full_like(chi2, (bins - 1) / 2.0), chi2 / 2.0)
    uniform = torch.arange(1, L + 1, dtype=torch.float64) / L
    dev = (hist.cumsum(dim=1).to(torch.float64) / G - uniform).abs().max(dim=1).values
    return {"counts": counts, "chi2": chi2, "p_value": p_value, "ecdf_max_dev": dev}


def sbc_glm(X, likelihood, sims=256, chains_per_sim=3, kept=21, thin=3, tune=150, prior_scale=1.0, sigma=1.0, fit=None, bins=8,
            random_seed=0, draws_fn=None, count_fn=None, **sample_kw):
    """Simulation-based calibration of one GLM configuration in ONE job: simulate ``sims`` data sets (``simulate_glm``), build
    ``Batched([GLM(X_g, y_g, likelihood, **fitted)])``, run ``sample(..., chains=sims * chains_per_sim, draws=kept * thin,
    thin=thin, tune=tune, return_engine=True)``, take every ``q_true[g]``'s rank among the ``n_draws = chains_per_sim * kept``
    kept draws of its posterior with one pass over the trace in HBM (``diagnostics.threshold_counts`` with the thresholds
    ``q_true[:, None, :]``), and test the ranks (``rank_uniformity``, which needs ``(n_draws + 1) % bins == 0``: checked before
    anything runs). The engine is closed whatever happens.

    The fitted model uses the simulating ``prior_scale`` / ``sigma``, overridden by the dict ``fit``: a ``fit`` that differs
    from the simulation is the negative control, whose ranks must NOT be uniform. -> ``rank_uniformity``'s fields plus
    ``ranks[G, d]``, ``ties[G, d]`` (the draws equal to q_true: 0 for a continuous posterior), ``q_true[G, d]``, ``n_draws`` and
    ``n_diverging[G]`` (divergent kept iterations per simulation). ``**sample_kw`` goes to ``sample`` (``random_seed`` seeds
    both the simulation and the job). ``draws_fn(target) -> x[chains, kept, d]`` replaces sampling and ``count_fn`` the HIP
    count (``diagnostics.threshold_counts``), for tests of this logic without a GPU."""
    from . import diagnostics
    from .targets import GLM, Batched

    G, per, kept, thin = int(sims), int(chains_per_sim), int(kept), int(thin)
    if per < 1 or kept < 1:
        raise ValueError("chains_per_sim and kept must be >= 1 (got %d, %d)" % (per, kept))
    n_draws, bins = _check_bins(per * kept, bins)
    q_true, y = simulate_glm(X, likelihood, G, prior_scale=prior_scale, sigma=sigma, random_seed=random_seed)
    fitted = {"prior_scale": prior_scale, "sigma": sigma}
    fitted.update(fit or {})
    X = np.asarray(X, dtype=np.float64)
    target = Batched([GLM(X if X.ndim == 2 else X[g], y[g], likelihood, **fitted) for g in range(G)])
    n_diverging = np.zeros(G, dtype=np.int64)
    eng = None
    try:
        if draws_fn is not None:
            x = torch.as_tensor(draws_fn(target))
        else:
            from .sampling import sample

            _trace, stats, eng = sample(target, target.d, chains=G * per, draws=kept * thin, tune=int(tune), thin=thin,
                                        random_seed=random_seed, return_engine=True, progressbar=False, **sample_kw)
            n_diverging = np.asarray(stats["diverging"]).reshape(G, -1).sum(axis=1).astype(np.int64)
            x = diagnostics.trace_tensor(eng)
        tc = diagnostics.threshold_counts(x, q_true[:, None, :], chains_per_group=per, count_fn=count_fn)
        if tc["n"] != n_draws:
            raise ValueError("the job kept %d draws per simulation, not chains_per_sim x kept = %d" % (tc["n"], n_draws))
        ranks, ties = tc["less"][:, 0].cpu(), tc["equal"][:, 0].cpu()
    finally:
        if eng is not None:
            eng.close()
    out = rank_uniformity(ranks, n_draws, bins)
    out.update(ranks=ranks, ties=ties, q_true=q_true, n_draws=n_draws, n_diverging=n_diverging)
    return out
