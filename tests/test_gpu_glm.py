"""-m gpu: targets.GLM, the regression posterior that carries its data (csrc/lmc_targets.hpp: GLMTarget), through every
layer: the device value and gradient against a 50-digit reference within a derived bound, a leapfrog trajectory there and
back, the exact gaussian posterior, Batched, and the other kernels (dense per-chain, dense shared, general, HMC).

The bound (tests/_glm_model.py: reference) is a forward error bound for the functor's stated operation order, with
u = 2^-53, S_n = sum_e |X_ne q_e|, l' = dl/deta = r, r' = dr/deta, NS elements per lane:
    |d eta_n| <= (d + 2) u S_n                          a recursive sum of d fused multiply-adds
    |d l_n|   <= |r_n| |d eta_n| + 8 u |l_n|            the propagated argument error, and 8 ulp for the link: the device's exp
                                                        and log1p (csrc/lmc_targets.hpp: exp_lane < 1.5 ulp, log1p_unit < 2.5
                                                        ulp by their own error analyses) and the three operations around them
    |d logp|  <= sum_n |d l_n| + (ceil(N/64) + 8) u sum_n |l_n| + (NS + 8) u tau/2 sum_e q_e^2
                                                        a lane adds ceil(N/64) terms, the wave reduction is a tree of depth 6
    |d r_n|   <= |r'_n| |d eta_n| + 8 u w_n             w_n: the magnitude of the operands r_n is formed from
    |d g_e|   <= sum_n |X_ne| |d r_n| + (N + 2) u sum_n |X_ne r_n| + 3 u tau |q_e|
The tests allow TWICE the bound. tests/test_glm_cpu.py holds the numpy statement of the same order to ONCE the bound on the
same inputs: the reference arithmetic alone does not use the allowance up."""
import numpy as np
import pytest

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi
from littlemcmc_amd import targets as T
from tests import _glm_model as M

pytestmark = pytest.mark.gpu
INVALID = 1   # LMC_ERR_INVALID


def _target(N, d, lik):
    X, y, _ = M.case(N, d, lik)
    return T.GLM(X, y, lik, prior_scale=M.PRIOR_SCALE, sigma=M.SIGMA)


def _assert_within(got_logp, got_g, ref, what, factor=2.0):
    err = abs(got_logp - ref["logp"])
    print("%s: |dlogp| %.3e (bound %.3e)  max |dg|/bound %.3f" % (what, err, ref["logp_bound"],
                                                                 np.max(np.abs(got_g - ref["g"]) / ref["g_bound"])))
    assert np.isfinite(got_logp) and np.isfinite(got_g).all(), what
    assert err <= factor * ref["logp_bound"], (what, err, ref["logp_bound"])
    excess = np.abs(got_g - ref["g"]) - factor * ref["g_bound"]
    assert (excess <= 0.0).all(), (what, int(np.argmax(excess)), float(excess.max()))


# ---- 1. value and gradient ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, d", M.SHAPES)
@pytest.mark.parametrize("lik", M.LIKELIHOODS)
def test_value_and_gradient_against_mpmath(N, d, lik):
    """Engine.logp_dlogp at four points per cell (one all zeros; bernoulli: eta reaching 40 and 800 in magnitude, where logp
    and g must stay finite) against the 50-digit reference, within twice the bound of the module docstring."""
    _, _, Q = M.case(N, d, lik)
    tgt = _target(N, d, lik)
    with lmc.Engine(tgt, chains=M.N_POINTS) as eng:
        assert eng.wide == (d > 256) and eng.kernel_shape()[2] == 1          # one wavefront per chain, general kernels beyond 256
        logp, grad = eng.logp_dlogp(Q)
    for c, ref in enumerate(M.case_reference(N, d, lik)):
        _assert_within(logp[c], grad[c], ref, "%s N=%d d=%d point %d" % (lik, N, d, c))
    if (N, d) == (63, 3):   # the reference plug-in signature, inherited: one point on the GPU
        one_logp, one_g = tgt(Q[1])
        assert one_logp == logp[1] and np.array_equal(one_g, grad[1])


# ---- 2. trajectory -----------------------------------------------------------------------------------------------------------
def test_trajectory_there_and_back():
    N, d, lik, n, eps = 65, 65, "bernoulli", 4, 0.02
    X, y, Q = M.case(N, d, lik)
    tgt = _target(N, d, lik)
    rs = np.random.RandomState(11)
    q0, p0 = Q[:2], rs.randn(2, d)
    with lmc.Engine(tgt, chains=2, potential="diag") as eng:
        eng.set_potential(np.zeros(d), np.ones(d), 10.0)
        out = eng.trajectory(q0, p0, eps, n, n, p0_is_f32=False)
    tau, isig2 = M.PRIOR_SCALE ** -2, M.SIGMA ** -2
    Xm = M.mp_matrix(X)
    for c in range(2):
        # reversibility, as tests/test_gpu_units.py::test_leapfrog_golden asks it (reference tests/test_hmc.py:23-40)
        np.testing.assert_allclose(out["q"][c][-1], out["q"][c][0], rtol=1e-5, atol=1e-12)
        np.testing.assert_allclose(out["p"][c][-1], out["p"][c][0], rtol=1e-5, atol=1e-12)
        np.testing.assert_array_equal(out["q"][c][0], q0[c])
        assert np.abs(out["q"][c][n] - q0[c]).max() > 1e-3                   # it did go somewhere
        for k in range(2 * n + 1):
            qk = out["q"][c][k]
            ref = M.reference(X, y, qk, lik, tau, isig2, Xm)
            model_logp, model_g = M.logp_grad(X, y, qk, lik, tau, isig2)
            assert abs(out["logp"][c][k] - model_logp) <= 2.0 * ref["logp_bound"], (c, k)
            assert (np.abs(out["g"][c][k] - model_g) <= 2.0 * ref["g_bound"]).all(), (c, k)
            _assert_within(out["logp"][c][k], out["g"][c][k], ref, "chain %d state %d" % (c, k))


# ---- 3. exact posterior ----------------------------------------------------------------------------------------------------
def test_gaussian_likelihood_samples_the_exact_posterior():
    """N = 40, d = 5, 512 chains, tune 300, draws 200, fixed seed. Per coordinate the pooled mean is within
    6 sqrt(Sigma_ee / ESS_e) of the exact mean and the pooled variance within 6 sqrt(2 / ESS_e) relative of Sigma_ee: 6 sigma
    over 10 comparisons is a false-alarm probability below 1e-7, and the seed is fixed."""
    import torch

    from littlemcmc_amd import diagnostics as dg

    rs = np.random.RandomState(2024)
    N, d = 40, 5
    X = rs.randn(N, d)
    X[:, 0] = 1.0
    y = X @ rs.randn(d) + 0.7 * rs.randn(N)
    tgt = T.GLM(X, y, "gaussian", prior_scale=3.0, sigma=0.7)
    mean, cov = tgt.posterior_gaussian()
    trace, stats = lmc.sample(tgt, d, draws=200, tune=300, chains=512, random_seed=77, progressbar=False)
    assert trace.shape == (512, 200, d) and np.isfinite(trace).all()
    diag = dg.summarize(torch.from_numpy(np.ascontiguousarray(trace)).cuda())
    rhat, ess = diag["rhat"].cpu().numpy(), diag["ess"].cpu().numpy()
    pooled = trace.reshape(-1, d)
    got_mean, got_var = pooled.mean(axis=0), pooled.var(axis=0, ddof=1)
    sig = np.diag(cov)
    print("rhat", rhat, "ess", ess, "z mean", (got_mean - mean) / np.sqrt(sig / ess), "z var", (got_var / sig - 1) / np.sqrt(2 / ess))
    assert (rhat < 1.01).all(), rhat
    assert (np.abs(got_mean - mean) <= 6.0 * np.sqrt(sig / ess)).all()
    assert (np.abs(got_var / sig - 1.0) <= 6.0 * np.sqrt(2.0 / ess)).all()
    assert not stats["diverging"].any()


# ---- 4. Batched ----------------------------------------------------------------------------------------------------------------
def _bernoulli_sets(G=4, N=65, d=3):
    out = []
    for g in range(G):
        rs = np.random.RandomState(300 + g)
        X = rs.randn(N, d)
        X[:, 0] = 1.0
        out.append(T.GLM(X, (rs.rand(N) < 1.0 / (1.0 + np.exp(-(X @ rs.randn(d))))) * 1.0))
    return T.Batched(out)


@pytest.mark.parametrize("kw", [dict(), dict(rng="counter", thin=3)], ids=["plain", "counter_thin3"])
def test_batched_groups_are_their_members(kw):
    """The Batched contract (tests/test_gpu_target_groups.py): every chain of group g is, bit for bit, that chain of
    sample(batched[g], ...) on the same seeds -- trace and every statistic."""
    b, chains = _bernoulli_sets(), 32
    seeds = [500 + 13 * c for c in range(chains)]
    args = dict(draws=15, tune=30, chains=chains, random_seed=seeds, discard_tuned_samples=False, progressbar=False, **kw)
    trace, stats, eng = lmc.sample(b, b.d, return_engine=True, **args)
    try:
        assert eng.target.family == _abi.TARGET_GLM and not eng.wide and eng.rng == kw.get("rng", "numpy")
        assert eng.target_groups() == (4, b.params.shape[1], 0, 8)
    finally:
        eng.close()
    assert trace.shape == (chains, -(-45 // kw.get("thin", 1)), 3) and np.isfinite(trace).all()
    for g, sl in enumerate(b.chain_slices(chains)):
        wtrace, wstats = lmc.sample(b[g], b.d, **args)
        np.testing.assert_array_equal(trace[sl], wtrace[sl])
        assert set(stats) == set(wstats)
        for name in wstats:
            np.testing.assert_array_equal(stats[name][sl], wstats[name][sl], err_msg=name)
    assert not np.array_equal(trace[0:8], trace[8:16])       # the groups did not all see row 0


# ---- 5. the other paths run and agree ---------------------------------------------------------------------------------------
_cache = {}


def _paths_target():
    rs = np.random.RandomState(41)
    N, d = 70, 5
    X = rs.randn(N, d)
    X[:, 0] = 1.0
    X[:, 1] = 0.8 * X[:, 2] + 0.6 * X[:, 1]                  # correlated columns: a dense matrix has something to find
    return T.GLM(X, (rs.rand(N) < 1.0 / (1.0 + np.exp(-(X @ np.array([0.3, 1.0, -1.0, 0.5, 0.0]))))) * 1.0)


_PATH_ARGS = dict(draws=100, tune=200, chains=64, random_seed=5, progressbar=False)


def _diag_run():
    """The diagonal run every other path is compared with, computed once and never modified."""
    if "diag" not in _cache:
        tgt = _paths_target()
        trace, _ = lmc.sample(tgt, tgt.d, **_PATH_ARGS)
        trace.setflags(write=False)
        _cache["diag"] = trace
    return _cache["diag"]


def _rhat_with_the_diagonal_run(trace):
    import torch

    from littlemcmc_amd import diagnostics as dg

    both = np.ascontiguousarray(np.concatenate([_diag_run(), trace], axis=0))
    return dg.summarize(torch.from_numpy(both).cuda())["rhat"].cpu().numpy()


@pytest.mark.parametrize("path", ["adapt_full", "adapt_full_pooled", "float64_mass", "hmc"])
def test_other_paths_run_and_agree(path):
    tgt = _paths_target()
    d, kw, want = tgt.d, dict(_PATH_ARGS), {}
    if path == "adapt_full":
        kw["init"], want = "adapt_full", dict(dense="per_chain")
    elif path == "adapt_full_pooled":
        kw["init"], want = "jitter+adapt_full_pooled", dict(dense="shared")
    elif path == "float64_mass":
        kw["step"] = lmc.NUTS(tgt, d, potential=lmc.QuadPotentialDiagAdapt(d, np.zeros(d), np.ones(d), 10, dtype="float64"))
        want = dict(wide=True)
    else:
        kw["step"] = lmc.HamiltonianMC(tgt, d, path_length=1.0)
    trace, stats, eng = lmc.sample(tgt, d, return_engine=True, **kw)
    try:
        if "dense" in want:
            assert eng.last_run_dense_kernel() == want["dense"]
        assert eng.wide == want.get("wide", False) and eng.kind == ("hmc" if path == "hmc" else "nuts")
    finally:
        eng.close()
    assert trace.shape == (64, 100, d) and np.isfinite(trace).all()
    rhat = _rhat_with_the_diagonal_run(trace)
    print(path, "rhat with the diagonal run", rhat)
    if path != "hmc":            # (HMC "runs": a fixed path length is not asked to have mixed in 100 draws)
        assert (rhat < 1.05).all(), rhat


def test_poisson_overflow_is_a_divergence():
    """A start whose first leapfrog overflows exp(eta): the intercept starts at 700 (exp(700) is finite, its gradient is
    -1e304), so the start energy is finite and every trajectory from it has a non-finite energy -- which the sampler reports
    as a divergence and rejects. Nothing faults: a non-finite energy is ordinary arithmetic."""
    rs = np.random.RandomState(8)
    N, d = 20, 2
    X = np.column_stack([np.ones(N), rs.randn(N)])
    tgt = T.GLM(X, rs.poisson(3.0, N) * 1.0, "poisson")
    start = np.array([700.0, 0.0])
    assert np.isfinite(tgt(start)[0])
    trace, stats = lmc.sample(tgt, d, draws=5, tune=5, chains=8, random_seed=3, init="adapt_diag", start=start,
                              discard_tuned_samples=False, progressbar=False)
    assert np.isfinite(trace).all()
    assert stats["diverging"][:, 0].all()
    np.testing.assert_array_equal(trace[:, 0], np.broadcast_to(start, (8, d)))      # the diverged proposal was rejected


# ---- 6. refusal ------------------------------------------------------------------------------------------------------------------
def test_engine_refuses_dim_513_and_names_the_limit():
    import ctypes as C

    lib = _abi.load()
    cfg = _abi.Config()
    lib.lmc_config_defaults(C.byref(cfg), 4, 513)
    cfg.target_family = _abi.TARGET_GLM
    h = C.c_void_p()
    assert lib.lmc_engine_create(C.byref(cfg), C.byref(h)) == INVALID and not h.value
    assert b"512" in lib.lmc_last_error(None) and b"513" in lib.lmc_last_error(None)
    # a hand-built row for 513 coefficients (the Python constructor would not make one) is refused by the pure check too
    n = 8 + 64 * (1 + 520 + 1024)
    assert lib.lmc_target_groups_check(_abi.TARGET_GLM, 513, 4, 1, n, 0, 4) == INVALID and b"512" in lib.lmc_last_error(None)


def test_setters_refuse_a_bad_header():
    """What is written in a row is checked where there is a table: both setters, before any HIP call."""
    X, y, _ = M.case(63, 3, "bernoulli")
    tgt = T.GLM(X, y)
    with lmc.Engine(tgt, chains=4) as eng:
        lib, h = eng._lib, eng._h
        err = lambda: lib.lmc_last_error(h)   # noqa: E731

        def both(row):
            table = np.ascontiguousarray(np.stack([row, row]))
            return (lib.lmc_engine_set_target_params(h, _abi.ptr(row), row.size),
                    lib.lmc_engine_set_target_params_grouped(h, _abi.ptr(table), 2, row.size, 0, 2))

        good = tgt.params.copy()
        assert both(good) == (_abi.OK, _abi.OK)
        for field, value, word in ((0, 3.0, b"likelihood"), (0, 0.5, b"likelihood"), (0, np.nan, b"likelihood"),
                                   (1, 200.0, b"header"), (1, 0.0, b"N ="), (1, 62.5, b"N ="),
                                   (2, 128.0, b"header"), (5, 4.0, b"header"), (6, 128.0, b"header"),
                                   (3, 0.0, b"tau"), (4, -1.0, b"tau")):
            bad = good.copy()
            bad[field] = value
            assert both(bad) == (INVALID, INVALID), (field, value)
            assert word in err(), (field, value, err())
        assert both(good[:-2].copy()) == (INVALID, INVALID)                    # a length no N gives
        longer = T.GLM(*M.case(130, 3, "bernoulli")[:2]).params.copy()         # a well-formed row of another N ...
        assert both(longer) == (_abi.OK, _abi.OK)
        longer[1] = 63.0                                                       # ... whose header claims the first one's
        assert both(longer) == (INVALID, INVALID) and b"header" in err()
        assert both(good) == (_abi.OK, _abi.OK)
        logp, _ = eng.logp_dlogp(np.zeros(3))
        assert np.isfinite(logp).all()
