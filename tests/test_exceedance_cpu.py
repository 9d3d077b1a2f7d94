"""No-GPU test of predictive.exceedance: the chunked write-then-count with the numpy models of the two HIP calls injected
(tests/_linpred_model.py, tests/_threshold_model.py), against direct counts over the model's own linear predictor."""
import numpy as np
import pytest
import torch

from littlemcmc_amd import _abi, predictive
from littlemcmc_amd import targets as T
from tests import _linpred_model as L
from tests import _threshold_model as M

KW = dict(linpred_fn=L.linpred_fn, count_fn=M.count_fn)


def _case(lik, y_of):
    rng = np.random.default_rng(40)
    N, d, per, n = 50, 4, 3, 11
    ms = [T.GLM(rng.standard_normal((N, d)) / 2.0, y_of(rng, N), lik) for _ in range(3)]
    tgt = T.Batched(ms)
    Xn = [rng.standard_normal((70, d)) for _ in range(3)]
    x = torch.from_numpy(rng.standard_normal((3 * per, n, d)))
    eta = predictive.linear_predictor(x, tgt, Xn, linpred_fn=L.linpred_fn)[0].numpy().reshape(3, per * n, 128)[:, :, :70]
    return tgt, ms, Xn, x, eta, per * n


def test_eta_and_mu_scales_chunks_blocks_and_forms_of_thresholds():
    tgt, ms, Xn, x, eta, S = _case("bernoulli", lambda rng, N: (rng.random(N) < 0.5).astype(np.float64))
    t_eta = np.array([-0.5, 0.0, 1.0])
    out = tgt.exceedance(x, Xn, thresholds=t_eta, **KW)
    assert tuple(out["p_less"].shape) == (3, 3, 70) and out["n"] == S and tuple(out["n_nan"].shape) == (3, 70)
    np.testing.assert_array_equal(out["p_less"].numpy(), (eta[:, :, None, :] < t_eta[:, None]).sum(axis=1) / S)
    np.testing.assert_array_equal(out["p_equal"].numpy(), np.zeros((3, 3, 70)))
    np.testing.assert_array_equal(out["p_greater"].numpy(), (eta[:, :, None, :] > t_eta[:, None]).sum(axis=1) / S)
    mu = 1 / (1 + np.exp(-eta))
    t_mu = np.array([0.25, 0.5])
    om = tgt.exceedance(x, Xn, thresholds=t_mu, scale="mu", **KW)
    np.testing.assert_array_equal(om["p_less"].numpy(), (mu[:, :, None, :] < t_mu[:, None]).sum(axis=1) / S)
    # the ends of mu's range: nothing lies below 0, everything below 1 and beyond
    ends = tgt.exceedance(x, Xn, thresholds=[-1.0, 0.0, 1.0, 2.0], scale="mu", **KW)
    np.testing.assert_array_equal(ends["p_less"].numpy(), np.broadcast_to(np.array([0.0, 0.0, 1.0, 1.0]).reshape(1, 4, 1), (3, 4, 70)))
    # one observation block per chunk, the list of blocks with a straddling group, a threshold per (group, point)
    calls = []
    chunked = tgt.exceedance(x, Xn, thresholds=t_mu, scale="mu", scratch_bytes=9 * 11 * 64 * 8, count_fn=M.count_fn,
                             linpred_fn=lambda *a: calls.append(a[4:6]) or L.linpred_fn(*a))
    assert calls == [(0, 1), (1, 2)]
    two = tgt.exceedance([x[:4], x[4:]], Xn, thresholds=t_mu, scale="mu", **KW)
    for k in ("p_less", "p_equal", "p_greater", "n_nan"):
        assert torch.equal(chunked[k], om[k]) and torch.equal(two[k], om[k]), k
    full = np.random.default_rng(1).standard_normal((3, 2, 70))
    per_point = tgt.exceedance(x, Xn, thresholds=full, **KW)
    np.testing.assert_array_equal(per_point["p_less"].numpy(), (eta[:, :, None, :] < full[:, None]).sum(axis=1) / S)
    own = ms[1].exceedance(x[3:6], thresholds=0.5, scale="mu", **KW)              # GLM.exceedance at the training design
    assert tuple(own["p_less"].shape) == (1, 1, 50)
    assert torch.equal(own["p_less"], tgt.exceedance(x, thresholds=0.5, scale="mu", **KW)["p_less"][1:2])


def test_log_link_nan_rule_and_refusals():
    tgt, _ms, Xn, x, eta, S = _case("poisson", lambda rng, N: rng.poisson(2.0, N).astype(np.float64))
    t_mu = np.array([0.5, 1.0, 3.0])
    om = tgt.exceedance(x, Xn, thresholds=t_mu, scale="mu", **KW)
    np.testing.assert_array_equal(om["p_less"].numpy(), (eta[:, :, None, :] < np.log(t_mu)[:, None]).sum(axis=1) / S)
    y = x.clone()
    y[4, 2, 1] = float("nan")                                                  # a NaN coefficient of group 1: every point of it
    bad = tgt.exceedance(y, Xn, thresholds=t_mu, scale="mu", **KW)
    assert bool(torch.isnan(bad["p_less"][1]).all()) and bool((bad["n_nan"][1] == 1).all())
    assert torch.equal(bad["p_less"][[0, 2]], om["p_less"][[0, 2]]) and not bool(bad["n_nan"][[0, 2]].any())
    with pytest.raises(ValueError, match="scratch_bytes"):
        tgt.exceedance(x, Xn, thresholds=0.0, scratch_bytes=1000, **KW)
    with pytest.raises(ValueError, match="scale"):
        tgt.exceedance(x, Xn, thresholds=0.0, scale="y", **KW)
    with pytest.raises(ValueError, match="thresholds"):
        tgt.exceedance(x, Xn, thresholds=np.zeros((2, 3, 70)), **KW)
    with pytest.raises(TypeError):
        predictive.exceedance(x, T.StdNormal(4), thresholds=0.0, **KW)
    with pytest.raises(_abi.HipLibraryError):
        tgt.exceedance(x, Xn, thresholds=0.0)                                  # a CPU tensor and no injected models
