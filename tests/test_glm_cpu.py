"""targets.GLM without a GPU: the constructor's refusals, the parameter row (include/lmc_hip.h: LMC_TARGET_GLM), Batched's
rules for GLM members, the library's pure row check, and the numpy statement of the density (tests/_glm_model.py) against
its 50-digit statement within the forward error bound that tests/test_gpu_glm.py holds the device to -- on that test's own
inputs, so that the bound is seen not to be violated by the reference arithmetic alone."""
import numpy as np
import pytest

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi
from littlemcmc_amd import targets as T
from tests import _glm_model as M

INVALID = 1   # LMC_ERR_INVALID


def _data(N, d, lik="bernoulli", seed=0):
    rs = np.random.RandomState(seed)
    X = rs.randn(N, d)
    y = {"bernoulli": (rs.rand(N) < 0.5) * 1.0, "poisson": rs.poisson(2.0, N) * 1.0, "gaussian": rs.randn(N)}[lik]
    return X, y


def test_constructor_validation():
    X, y = _data(10, 3)
    good = T.GLM(X, y)
    assert good.d == 3 and good.n_obs == 10 and good.family == _abi.TARGET_GLM == 8 and good.params.ndim == 1
    assert "dropped" in T.GLM.__doc__.lower()
    bad = [
        lambda: T.GLM(X[0], y),                                   # X not a matrix
        lambda: T.GLM(X, y[:9]),                                  # y of another length
        lambda: T.GLM(X, y.reshape(10, 1)),                       # y not a vector
        lambda: T.GLM(np.zeros((0, 3)), np.zeros(0)),             # no observations
        lambda: T.GLM(np.where(np.arange(30).reshape(10, 3) == 4, np.nan, X), y),
        lambda: T.GLM(X, np.where(np.arange(10) == 2, np.inf, y)),
        lambda: T.GLM(X, y + 0.5),                                # bernoulli y outside {0, 1}
        lambda: T.GLM(X, np.full(10, 2.0)),
        lambda: T.GLM(X, -np.ones(10), likelihood="poisson"),     # negative counts
        lambda: T.GLM(X, y, prior_scale=0.0),
        lambda: T.GLM(X, y, prior_scale=-1.0),
        lambda: T.GLM(X, y, prior_scale=np.inf),
        lambda: T.GLM(X, y, likelihood="gaussian", sigma=0.0),
        lambda: T.GLM(X, y, likelihood="gaussian", sigma=-2.0),
        lambda: T.GLM(X, y, likelihood="probit"),
        lambda: T.GLM(np.zeros((2, 513)), np.zeros(2)),           # d > 512
    ]
    for k, make in enumerate(bad):
        with pytest.raises(ValueError):
            make()
            pytest.fail("case %d was accepted" % k)
    with pytest.raises(ValueError, match="512"):
        T.GLM(np.zeros((2, 513)), np.zeros(2))
    T.GLM(np.zeros((2, 512)), np.zeros(2))                        # the limit itself is taken
    T.GLM(X, np.arange(10.0), likelihood="poisson")
    T.GLM(X, y - 3.5, likelihood="gaussian", sigma=0.1)
    with pytest.raises(TypeError, match="GLM"):
        T.require_device_target(3)


@pytest.mark.parametrize("N, d", [(1, 1), (63, 3), (65, 65), (130, 130)])
@pytest.mark.parametrize("lik", M.LIKELIHOODS)
def test_parameter_row(N, d, lik):
    X, y = _data(N, d, lik, seed=N + d)
    X[X == 0.0] = 1.0   # (so that "zero" below means padding)
    t = T.GLM(X, y, lik, prior_scale=2.0, sigma=0.5)
    row, lay = t.params, T.glm_row_layout(N, d)
    npad, d8, dpad = -(-N // 64) * 64, -(-d // 8) * 8, 64 * M.ns_for(d)
    assert (lay["npad"], lay["d8"], lay["dpad"]) == (npad, d8, dpad) and row.dtype == np.float64
    assert row.size == lay["size"] == 8 + npad * (1 + d8 + dpad)
    np.testing.assert_array_equal(row[:8], [T.GLM.LIKELIHOODS[lik], N, npad, 0.25, 4.0, d, dpad, 0.0])
    assert (lay["y"], lay["xt"], lay["xr"]) == (8, 8 + npad, 8 + npad * (1 + d8))
    assert all(lay[k] % 2 == 0 for k in ("y", "xt", "xr", "size"))          # 16-byte aligned sections, even row length
    ysec = row[lay["y"]:lay["xt"]]
    xt = row[lay["xt"]:lay["xr"]].reshape(d8, npad)
    xr = row[lay["xr"]:].reshape(npad, dpad)
    np.testing.assert_array_equal(ysec[:N], y)
    np.testing.assert_array_equal(xr[:N, :d], X)
    np.testing.assert_array_equal(xt[:d, :N], xr[:N, :d].T)                 # exact transposes of each other
    assert not ysec[N:].any() and not xt[:, N:].any() and not xt[d:].any() and not xr[N:].any() and not xr[:, d:].any()
    assert not np.signbit(row[row == 0.0]).any()                            # exactly +0.0
    # the row's shape is a function of (N, d) alone
    other = T.GLM(*_data(N, d, "gaussian", seed=99), likelihood="gaussian")
    assert other.params.shape == row.shape


def test_batched_takes_equal_glms_and_refuses_other_n_or_likelihood():
    sets = [_data(65, 3, seed=s) for s in range(4)]
    b = T.Batched([T.GLM(X, y) for X, y in sets])
    assert b.family == _abi.TARGET_GLM and b.groups == 4 and b.d == 3
    assert b.params.shape == (4, T.glm_row_layout(65, 3)["size"])
    for g, (X, y) in enumerate(sets):
        np.testing.assert_array_equal(b.params[g], T.GLM(X, y).params)
    assert T.glm_row_layout(65, 3)["size"] == T.glm_row_layout(70, 3)["size"]   # equal lengths, different headers:
    with pytest.raises(ValueError, match="N = 70"):
        T.Batched([T.GLM(*sets[0]), T.GLM(*_data(70, 3))])
    with pytest.raises(ValueError, match="poisson"):
        T.Batched([T.GLM(*sets[0]), T.GLM(*_data(65, 3, "poisson"), likelihood="poisson")])
    with pytest.raises(ValueError):
        T.Batched([T.GLM(*sets[0]), T.GLM(*_data(65, 4))])
    with pytest.raises(ValueError):
        T.Batched([T.GLM(*sets[0]), T.GLM(*_data(200, 3))])


def test_library_row_check():
    """lmc_target_groups_check is a pure function of (family, dim, chains, table shape): it takes the length every N gives at
    the engine's dim and refuses any other. It is handed no table, so what is written IN a row -- the likelihood code among
    it -- is checked by the setters, which are: tests/test_gpu_glm.py::test_setters_refuse_a_bad_header."""
    lib = _abi.load()
    assert lib.lmc_has_target(_abi.TARGET_GLM) == 1 and lib.lmc_has_target(7) == 0 and lib.lmc_has_target(9) == 0
    check, err = lib.lmc_target_groups_check, lambda: lib.lmc_last_error(None)   # noqa: E731
    glm = _abi.TARGET_GLM
    for N, d in ((1, 1), (63, 3), (65, 65), (130, 130), (70, 300), (5, 512)):
        n = T.GLM(*_data(N, d)).params.size
        assert check(glm, d, 8, 4, n, 0, 2) == _abi.OK, (N, d)
        for wrong in (n - 1, n + 1, n + 2, n + 64, 8, 0):
            assert check(glm, d, 8, 4, wrong, 0, 2) == INVALID and b"glm" in err(), (N, d, wrong)
        if d + 8 <= 512:
            assert check(glm, d + 8, 8, 4, n, 0, 2) == INVALID, (N, d)          # a row built for another dim
    assert check(glm, 513, 8, 4, 8 + 64 * (1 + 520 + 1024), 0, 2) == INVALID and b"512" in err()
    assert check(glm, 3, 9, 4, T.GLM(*_data(63, 3)).params.size, 0, 2) == INVALID and b"reads row 4" in err()


@pytest.mark.parametrize("lik", M.LIKELIHOODS)
def test_numpy_model_meets_the_bound_against_mpmath(lik):
    """The float64 statement against the 50-digit one, on the GPU test's inputs, within the bound (M.reference) -- not twice
    the bound: the slack is left to the device's own exp / log1p."""
    tau, isig2 = M.PRIOR_SCALE ** -2, M.SIGMA ** -2
    for N, d in M.SHAPES:
        X, y, Q = M.case(N, d, lik)
        if lik == "bernoulli":
            eta = Q @ X.T
            assert eta[0].max() == eta[0].min() == 0.0
            assert abs(np.abs(eta[2]).max() - 40.0) < 1e-9 and abs(np.abs(eta[3]).max() - 800.0) < 1e-9
        for c, ref in enumerate(M.case_reference(N, d, lik)):
            logp, g = M.logp_grad(X, y, Q[c], lik, tau, isig2)
            assert np.isfinite(logp) and np.isfinite(g).all() and np.isfinite(ref["logp"])
            assert abs(logp - ref["logp"]) <= ref["logp_bound"], (N, d, c, logp - ref["logp"], ref["logp_bound"])
            excess = np.abs(g - ref["g"]) - ref["g_bound"]
            assert (excess <= 0.0).all(), (N, d, c, excess.max())


@pytest.mark.parametrize("lik", M.LIKELIHOODS)
def test_numpy_gradient_is_the_derivative_of_numpy_logp(lik):
    N, d = 63, 3
    X, y, Q = M.case(N, d, lik)
    q, h = Q[1], 1e-5
    _, g = M.logp_grad(X, y, q, lik, 0.25, 4.0)
    for e in range(d):
        dq = np.zeros(d)
        dq[e] = h
        fd = (M.logp_grad(X, y, q + dq, lik, 0.25, 4.0)[0] - M.logp_grad(X, y, q - dq, lik, 0.25, 4.0)[0]) / (2 * h)
        np.testing.assert_allclose(g[e], fd, rtol=1e-6, atol=1e-6)


def test_posterior_gaussian():
    rs = np.random.RandomState(5)
    X, y = rs.randn(12, 3), rs.randn(12)
    t = T.GLM(X, y, "gaussian", prior_scale=2.0, sigma=0.5)
    mean, cov = t.posterior_gaussian()
    A = X.T @ X / 0.25 + np.eye(3) / 4.0
    np.testing.assert_allclose(mean, np.linalg.solve(A, X.T @ y / 0.25), rtol=1e-12)
    np.testing.assert_allclose(cov, np.linalg.solve(A, np.eye(3)), rtol=1e-12, atol=1e-15)
    # the mean is where the model's gradient vanishes
    _, g = M.logp_grad(X, y, mean, "gaussian", 0.25, 4.0)
    assert np.abs(g).max() < 1e-10
    with pytest.raises(ValueError, match="gaussian"):
        T.GLM(X, (y > 0) * 1.0).posterior_gaussian()
    assert lmc.targets.GLM is T.GLM
