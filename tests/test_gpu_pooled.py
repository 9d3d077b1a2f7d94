"""-m gpu: one shared dense mass matrix adapted from ALL chains (QuadPotentialFullPooled, lmc_engine_pool_*).

The statistic (csrc/lmc_pool.hip) against numpy in extended precision with a DERIVED tolerance, its bit-reproducibility, the
installation of the shrunk covariance through the same tail as lmc_engine_set_dense_potential, the dual-averaging restart,
and the job end to end against two jobs of existing code on the same seeds: QuadPotentialFull(true covariance) -- the
ceiling -- and the default diagonal adaptation."""
import numpy as np
import pytest

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
SHAPES = [(2, 1), (1000, 7), (4097, 64), (3000, 100), (8192, 128), (2500, 200), (4096, 256)]


def _full_engine(chains, d):
    eng = lmc.Engine(lmc.targets.StdNormal(d), chains, potential="full")
    eng.set_dense_potential(np.eye(d))
    return eng


def _positions(chains, d, k):
    """Snapshot k of a shape: x = mu + A z with a mean of order 10 (so that the shift matters), seeded."""
    rng = np.random.RandomState(1000 * d + 10 * chains % 997 + k)
    mu = 10.0 + rng.standard_normal(d)
    a = rng.standard_normal((d, d)) / np.sqrt(d) + np.eye(d)
    return mu + rng.standard_normal((chains, d)) @ a.T + 0.1 * k


def _three_snapshots(eng, chains, d, count=3):
    xs = [_positions(chains, d, k) for k in range(count)]
    eng.pool_reset()
    for x in xs:
        eng.set_position(x)
        eng.pool_accumulate()
    return xs, eng.pool_get()


@pytest.mark.parametrize("chains,d", SHAPES)
def test_pooled_statistic_against_numpy(chains, d):
    """n exact, m2 exactly symmetric, and every entry within the worst-case bound of ANY summation order of the device's
    own operands: with N rows and a = |x - shift|, the sum S_ij of N products of rounded differences is off by at most
    N 2^-52 sum_c a_ci a_cj (2^-53 per factor for x - shift, (N - 1) 2^-53 for the sum), the column sums s_i by
    e_i = N 2^-52 sum_c a_ci, hence the correction s_i s_j / n by (|s_i| e_j + |s_j| e_i) / n. No free factor."""
    with _full_engine(chains, d) as eng:
        xs, (n, mean, m2) = _three_snapshots(eng, chains, d)
    rows = np.concatenate(xs).astype(np.longdouble)
    N = rows.shape[0]
    assert n == N == 3 * chains
    assert mean.shape == (d,) and m2.shape == (d, d)
    np.testing.assert_array_equal(m2, m2.T)
    ref_mean = rows.mean(axis=0)
    dev = rows - ref_mean
    ref_m2 = dev.T @ dev
    shift = xs[0].mean(axis=0)                       # what the first snapshot fixes (to rounding; only the bound uses it)
    a = np.abs(rows - shift.astype(np.longdouble))
    s = (rows - shift.astype(np.longdouble)).sum(axis=0)
    col = a.sum(axis=0)
    e_s = N * EPS * col
    tol_m2 = N * EPS * (a.T @ a) + (np.abs(s)[:, None] * e_s[None, :] + np.abs(s)[None, :] * e_s[:, None]) / N
    tol_mean = e_s / N + EPS * np.abs(ref_mean)
    err_m2 = np.abs(m2.astype(np.longdouble) - ref_m2)
    err_mean = np.abs(mean.astype(np.longdouble) - ref_mean)
    print("chains %d d %d: max |m2 - ref| / bound = %.3g, max |mean - ref| / bound = %.3g"
          % (chains, d, float((err_m2 / tol_m2).max()), float((err_mean / tol_mean).max())))
    assert (err_m2 <= tol_m2).all()
    assert (err_mean <= tol_mean).all()


@pytest.mark.parametrize("chains,d", SHAPES)
def test_pooled_statistic_is_bit_reproducible(chains, d):
    with _full_engine(chains, d) as one, _full_engine(chains, d) as two:
        _xs, (n1, mean1, m21) = _three_snapshots(one, chains, d)
        _xs, (n2, mean2, m22) = _three_snapshots(two, chains, d)
        assert n1 == n2
        np.testing.assert_array_equal(m21, m22)
        np.testing.assert_array_equal(mean1, mean2)
        # memoryless: reset, then one snapshot == a fresh engine's one snapshot
        _x, (n3, mean3, m23) = _three_snapshots(one, chains, d, count=1)
    with _full_engine(chains, d) as fresh:
        _x, (n4, mean4, m24) = _three_snapshots(fresh, chains, d, count=1)
    assert n3 == n4 == chains
    np.testing.assert_array_equal(m23, m24)
    np.testing.assert_array_equal(mean3, mean4)


def _shrunk(n, m2):
    """cov = m2 / (n - 1), then Stan's shrinkage, in the operation order of lmc_engine_pool_apply (include/lmc_hip.h)."""
    nn = float(n)
    cov = (nn / (nn + 5.0)) * (m2 / (nn - 1.0))
    cov[np.diag_indices_from(cov)] += 1e-3 * (5.0 / (nn + 5.0))
    return cov


@pytest.mark.parametrize("chains,d", [(3000, 100), (2500, 200), (64, 6)])
def test_pool_apply_installs_the_shrunk_covariance_through_the_shared_tail(chains, d):
    seeds = np.arange(chains) + 7
    with _full_engine(chains, d) as eng, _full_engine(chains, d) as other:
        _xs, (n, _mean, m2) = _three_snapshots(eng, chains, d, count=2)
        cov64 = _shrunk(n, m2)
        eng.pool_apply()
        cov, chol = eng.dense_chain(0)
        assert cov.dtype == np.float32
        np.testing.assert_array_equal(cov, cov64.astype(np.float32))
        # the factor: the tolerance tests/test_gpu_dense.py holds set_dense_potential's float32 factor to
        np.testing.assert_allclose(chol, np.linalg.cholesky(cov.astype("d")), rtol=1e-5, atol=1e-6)
        # one shared tail: set_dense_potential(the same matrix) on a second engine gives the same bits, momentum factor included
        other.set_dense_potential(cov64)
        cov_o, chol_o = other.dense_chain(0)
        np.testing.assert_array_equal(cov, cov_o)
        np.testing.assert_array_equal(chol, chol_o)
        eng.seed(seeds)
        other.seed(seeds)
        np.testing.assert_array_equal(eng.draw_momentum(), other.draw_momentum())


def test_pool_apply_refusals_leave_the_matrix():
    d = 5
    with _full_engine(16, d) as eng:
        before = eng.dense_chain(0)
        eng.pool_reset()
        with pytest.raises(_abi.HipLibraryError, match="error 1.*at least 2 samples"):
            eng.pool_apply()
        eng.set_position(np.full((16, d), np.inf))
        eng.pool_accumulate()
        with pytest.raises(_abi.HipLibraryError, match="error 1"):
            eng.pool_apply()
        after = eng.dense_chain(0)
        np.testing.assert_array_equal(before[0], after[0])
        np.testing.assert_array_equal(before[1], after[1])
    with lmc.Engine(lmc.targets.StdNormal(d), 16, potential="diag_adapt") as diag:
        for call in (diag.pool_reset, diag.pool_accumulate, diag.pool_get, diag.pool_apply, diag.restart_dual_average):
            with pytest.raises(_abi.HipLibraryError, match="error 3"):       # LMC_ERR_STATE
                call()
    with lmc.Engine(lmc.targets.StdNormal(300), 4, potential="full") as big:
        big.set_dense_potential(np.eye(300))
        with pytest.raises(_abi.HipLibraryError, match="error 1.*256"):      # LMC_ERR_INVALID
            big.pool_accumulate()


def test_restart_dual_average():
    """Stan's restart after a metric change: mu = log(10 step), hbar = 0, log_bar = 0, count = 1, log_step as it was. mu is
    two library calls on either side (exp, log: 1 ulp each) and a product: 8 x 2^-52 x max(1, |mu|) covers both."""
    chains, d = 500, 12
    with lmc.Engine(lmc.targets.AR1(d, 0.9), chains, potential="full") as eng:
        eng.set_dense_potential(np.eye(d))
        eng.seed(np.arange(chains) + 1)
        eng.set_position(np.zeros((chains, d)))
        eng.reset_tuning()
        eng.reserve(30, keep_trace=False)
        eng.run(30, 0, 30)
        before = eng.adapt_state()
        assert (before["count"] > 1).all() and (before["hbar"] != 0).any() and len(np.unique(before["log_step"])) > chains // 2
        eng.restart_dual_average()
        after = eng.adapt_state()
    np.testing.assert_array_equal(after["log_step"], before["log_step"])
    assert (after["hbar"] == 0).all() and (after["log_bar"] == 0).all() and (after["count"] == 1).all()
    want = np.log(10.0 * np.exp(before["log_step"]))
    assert (np.abs(after["mu"] - want) <= 8 * EPS * np.maximum(1.0, np.abs(want))).all()


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def _z_between(x, y):
    """Per dimension, (statistic of run x - statistic of run y) in Monte-Carlo standard errors taken from the spread of the
    per-chain values over the chains of each run (the method of tests/test_gpu_same_seed.py, with chains as the replicates):
    the mean, and the variance as the per-chain mean squared deviation from the RUN's mean (not the chain's: a chain's own
    mean would bias the two runs differently where their autocorrelations differ). x, y: [chains, draws, d]."""
    out = []
    for f in (lambda t: t.mean(axis=1), lambda t: ((t - t.mean(axis=(0, 1))) ** 2).mean(axis=1)):
        fx, fy = f(x), f(y)
        se = np.sqrt(fx.var(axis=0, ddof=1) / fx.shape[0] + fy.var(axis=0, ddof=1) / fy.shape[0])
        out.append((fx.mean(axis=0) - fy.mean(axis=0)) / se)
    return np.concatenate(out)


def test_pooled_adaptation_end_to_end():
    """AR(1) rho = 0.9, d = 128, 4 096 chains, tune 400 + draws 200 (the docstring of the module and the issue's item 7).
    The Frobenius bound is the expected sampling error of a covariance from `chains` independent draws,
    sqrt((tr(S)^2 + tr(S^2)) / chains); the last window holds 8 snapshots 25 iterations apart, so more than that."""
    d, chains, tune, draws, seed = 128, 4096, 400, 200, 20261016
    idx = np.arange(d)
    sigma = 0.9 ** np.abs(idx[:, None] - idx[None, :])
    tgt = lmc.targets.AR1(d, 0.9)
    kw = dict(draws=draws, tune=tune, chains=chains, random_seed=seed, progressbar=False)

    def pooled():
        trace, stats, eng = lmc.sample(tgt, d, init="jitter+adapt_full_pooled", return_engine=True, **kw)
        try:
            return np.array(trace), {k: np.array(v) for k, v in stats.items()}, eng.dense_chain(0)[0], eng.last_run_dense_kernel()
        finally:
            eng.close()

    trace, stats, cov, kernel = pooled()
    assert trace.shape == (chains, draws, d) and np.isfinite(trace).all()
    assert kernel == "shared"                # lmc_engine_last_run_dense_kernel() == 2: the draws ran in the shared-matrix MFMA kernel
    frob = float(np.linalg.norm(cov.astype("d") - sigma))
    bound = float(np.sqrt((np.trace(sigma) ** 2 + np.trace(sigma @ sigma)) / chains))
    print("||cov_adapted - Sigma||_F = %.4f, bound %.4f (||Sigma||_F = %.2f)" % (frob, bound, np.linalg.norm(sigma)))
    assert frob <= bound

    ceil_trace, ceil_stats = lmc.sample(tgt, d, step=lmc.NUTS(tgt, d, potential=lmc.QuadPotentialFull(sigma)), **kw)
    diag_trace, diag_stats = lmc.sample(tgt, d, **kw)
    size_pooled, size_diag, size_ceil = (float(s["tree_size"].mean()) for s in (stats, diag_stats, ceil_stats))
    print("mean tree_size of the draws: pooled %.2f, true covariance %.2f, diagonal %.2f; divergences %d"
          % (size_pooled, size_ceil, size_diag, int(stats["diverging"].sum())))
    assert size_pooled < 0.5 * size_diag
    assert not stats["diverging"].any()

    z = _z_between(trace, np.asarray(ceil_trace))
    print("pooled against QuadPotentialFull(Sigma): largest |z| over %d statistics %.2f (mean part %.2f, variance part %.2f)"
          % (z.size, np.abs(z).max(), np.abs(z[:d]).max(), np.abs(z[d:]).max()))
    assert z.size == 2 * d and np.abs(z).max() <= 4.5

    trace2, stats2, cov2, _k = pooled()      # the same job again: the same arrays bit for bit
    np.testing.assert_array_equal(trace, trace2)
    np.testing.assert_array_equal(cov, cov2)
    assert sorted(stats) == sorted(stats2)
    for name in stats:
        np.testing.assert_array_equal(stats[name], stats2[name], err_msg=name)


@pytest.mark.parametrize("init", ["adapt_full_pooled", "jitter+adapt_full_pooled"])
def test_sample_with_pooled_init_modes(init):
    """Result shapes and dtypes as test_sample_with_dense_init_modes asserts them for adapt_full."""
    d, chains, draws, tune = 6, 64, 60, 260
    tgt = lmc.targets.AR1(d, 0.9)
    trace, stats = lmc.sample(tgt, d, draws=draws, tune=tune, chains=chains, init=init, random_seed=3)
    assert trace.shape == (chains, draws, d)
    assert stats["depth"].shape == (chains, draws, 1) and stats["depth"].dtype == np.int64
    assert not stats["diverging"].any()
    start, step = lmc.init_nuts(tgt, d, init=init, random_seed=3)
    assert isinstance(step.potential, lmc.QuadPotentialFullPooled)


def test_pooled_in_the_per_wave_dense_kernel_and_write_back():
    """d = 200: beyond the shared-matrix kernel's 128 dimensions the draws run in run_dense_kernel; after sample() the
    step's potential holds the adapted matrix."""
    d, chains = 200, 2048
    idx = np.arange(d)
    sigma = 0.9 ** np.abs(idx[:, None] - idx[None, :])
    tgt = lmc.targets.AR1(d, 0.9)
    start, step = lmc.init_nuts(tgt, d, init="jitter+adapt_full_pooled", random_seed=5)
    trace, stats, eng = lmc.sample(tgt, d, draws=50, tune=200, chains=chains, step=step, start=start, random_seed=5,
                                   progressbar=False, return_engine=True)
    try:
        assert eng.last_run_dense_kernel() == "per_chain"      # lmc_engine_last_run_dense_kernel() == 1
        cov = eng.dense_chain(0)[0]
    finally:
        eng.close()
    assert trace.shape == (chains, 50, d) and np.isfinite(trace).all() and not stats["diverging"].any()
    np.testing.assert_array_equal(step.potential._cov, cov)
    assert step.potential._chol is not None and not np.array_equal(cov, np.eye(d, dtype=np.float32))
    bound = float(np.sqrt((np.trace(sigma) ** 2 + np.trace(sigma @ sigma)) / chains))
    assert np.linalg.norm(cov.astype("d") - sigma) <= bound


def test_pooled_with_hamiltonian_mc():
    d, chains = 32, 1024
    tgt = lmc.targets.AR1(d, 0.9)
    step = lmc.HamiltonianMC(tgt, d, potential=lmc.QuadPotentialFullPooled(d))
    trace, stats = lmc.sample(tgt, d, draws=100, tune=300, chains=chains, step=step, start=np.zeros(d), random_seed=9,
                              progressbar=False)
    assert trace.shape == (chains, 100, d) and np.isfinite(trace).all()
    assert stats["accept"].shape == (chains, 100, 1)
    var = trace.reshape(-1, d).var(axis=0)
    assert (np.abs(var - 1.0) < 0.1).all()           # unit marginal variances (1e5 draws per dimension)
    assert not np.array_equal(step.potential._cov, np.eye(d, dtype=np.float32))


def test_keyboard_interrupt_during_pooled_tuning():
    """A KeyboardInterrupt raised in ``callback`` inside an adaptation window returns the iterations every chain completed,
    as test_keyboard_interrupt_in_the_shared_matrix_kernel expects of the fixed matrix."""
    d, chains, tune = 32, 2048, 40000
    tgt = lmc.targets.AR1(d, 0.9)
    assert any(b <= 120 < e for b, e in lmc.sampling.pooled_windows(tune))
    fired = []

    def cb(trace, draw):
        if not fired and draw.iteration >= 120:
            fired.append(draw.iteration)
            raise KeyboardInterrupt

    total = tune + 100
    trace, stats = lmc.sample(tgt, d, draws=100, tune=tune, chains=chains, init="adapt_full_pooled", random_seed=3,
                              discard_tuned_samples=False, callback=cb, progressbar=False)
    n = trace.shape[1]
    print("interrupt at device iteration %s: %d of %d iterations" % (fired, n, total))
    assert fired and 0 < n < total and np.isfinite(trace).all()
    assert stats["tree_size"].shape == (chains, n, 1) and stats["tune"].all()
