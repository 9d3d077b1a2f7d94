"""No-GPU tests of PSIS-LOO: the numpy model of the row algorithm (tests/_psis_model.py) against the exact leave-one-out
density of the gaussian GLM and against itself at 50 digits, its edge rows, the host logic of littlemcmc_amd/predictive.py
(psis, pointwise_loglik, loo) with the model injected for the two HIP calls, and the C entry points' refusals.

Measured here (printed by the tests, asserted not to exceed the constants of _psis_model):
  closed form, 4 rungs x 20 seeds x S = 3200: worst |deviation| 3.12 seed-to-seed sd, largest per-point sd 0.0394, sd of the
  summed deviation 0.066 / 0.086 / 0.089 / 0.089 per rung (SD_TOTAL = 0.089), largest k on one draw set 0.769, n_tail 170;
  float64 model against the 50-digit model on the rows of the GPU test: eps_row = 4.10e-13 (the row of 1 860 000; every other
  row is below 5e-14) -> EPS_ROW = 4.2e-13."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from littlemcmc_amd import _abi, predictive
from littlemcmc_amd import targets as T
from tests import _predictive_model as P
from tests import _psis_model as M


def test_model_against_the_exact_closed_form():
    X, y, _Xn, _yn, sigma = P.ladder()
    S, seeds = M.SD_DRAWS, 20
    dev = np.zeros((4, seeds, X.shape[0]))
    k_max, nt_min = -np.inf, np.inf
    for g, scale in enumerate(P.LADDER_SCALES):
        tgt = T.GLM(X, y, "gaussian", prior_scale=scale, sigma=sigma)
        exact, const = M.exact_loo(tgt), tgt.loglik_constant()
        mean, cov = tgt.posterior_gaussian()
        for seed in range(seeds):
            q = np.random.default_rng(seed).multivariate_normal(mean, cov, size=S)
            ll = -0.5 * (y - q @ X.T) ** 2 / sigma ** 2
            for n in range(X.shape[0]):
                elpd, k, nt, _ess, _sg = M.psis_row(ll[:, n])
                dev[g, seed, n] = elpd + const[n] - exact[n]
                assert np.isfinite(k) and k < 1.0 and nt >= 170, (g, seed, n, k, nt)
                k_max, nt_min = max(k_max, k), min(nt_min, nt)
    sd = dev.std(axis=1, ddof=1)
    z = np.abs(dev) / sd[:, None, :]
    sd_total = dev.sum(axis=2).std(axis=1, ddof=1)
    print("worst z %.2f, largest per-point sd %.4f, sd of the summed deviation %s, largest k %.3f, smallest n_tail %d"
          % (z.max(), sd.max(), sd_total, k_max, nt_min))
    assert z.max() <= 5.0
    assert sd.max() <= M.SD_POINT and sd_total.max() <= M.SD_TOTAL   # the constants the GPU end-to-end test reads


def test_edge_rows():
    assert M.LOG_TINY == math.log(np.finfo(np.float64).tiny)
    elpd, k, nt, ess, sg = M.psis_row(np.full(100, -1.3))
    assert elpd == -1.3 and nt == 0 and k == np.inf and ess == 100.0 and np.isnan(sg)
    rng = np.random.default_rng(3)
    assert M.tail_len(10) == 2 and M.tail_len(25) == 5 and M.tail_len(200) == 40 and M.tail_len(250) == 48
    assert M.tail_len(M.BIG_S) == 4092 and M.tail_len(1) == 0 and M.tail_len(3200, 0.25) == 340
    _e, k, nt, _ess, sg = M.psis_row(-rng.standard_normal(10) ** 2)
    assert nt == 2 and k == np.inf and np.isnan(sg)                    # S = 10: M = 2, no fit
    _e, k, nt, _ess, sg = M.psis_row(-rng.standard_normal(25) ** 2)
    assert nt == 5 and np.isfinite(k) and np.isfinite(sg)              # S = 25: the smallest fit
    rows = dict(M.edge_rows())
    Mt = M.tail_len(4000)
    e, k, nt, ess, sg, cutoff, lmin = M.psis_row(rows["clamped"], M=Mt, full=True)
    assert cutoff == M.LOG_TINY and nt == 1 and k == np.inf and np.isfinite(e) and lmin == rows["clamped"].min()
    e, k, nt, ess, sg = M.psis_row(rows["tied"], M=Mt)
    assert 4 < nt < Mt and nt % 50 == 0 and np.isfinite(k)             # ties at the cutoff: n_tail < M
    for name, lmin_want in (("minus_inf", -np.inf), ("nan", np.nan)):
        e, k, nt, ess, sg, cutoff, lmin = M.psis_row(rows[name], M=Mt, full=True)
        assert all(np.isnan(v) for v in (e, k, ess, sg, cutoff)) and nt == 0
        assert np.isnan(lmin) if np.isnan(lmin_want) else lmin == lmin_want


def test_float64_model_against_the_50_digit_model():
    """eps_row: the rounding sensitivity the GPU test's tolerance (16 x EPS_ROW) is defined from."""
    worst, where = 0.0, None
    cases = [(kind, S, M.row(kind, S), None) for kind in M.KINDS for S in M.ROW_SIZES]
    cases += [(name, 4000, r, M.tail_len(4000)) for name, r in M.edge_rows() if np.isfinite(r).all()]
    cases.append(("gaussian", M.BIG_S, M.row("gaussian", M.BIG_S), None))
    for kind, S, r, Mt in cases:
        a, b = M.psis_row(r, M=Mt), M.psis_row_mp(r, M=Mt)
        assert a[2] == b[2], (kind, S, a, b)       # n_tail: the discrete part is exact
        dev = M.rel_dev(a, b)
        if dev > worst:
            worst, where = dev, (kind, S)
    print("eps_row = %.3e at %s" % (worst, where))
    assert worst <= M.EPS_ROW


def _batched(lik="poisson", N=70, d=3, groups=3):
    ms = []
    for g in range(groups):
        rng = np.random.default_rng(50 + g)
        X = rng.standard_normal((N, d)) / 2.0
        y = {"poisson": rng.poisson(2.0, N).astype(np.float64), "gaussian": rng.standard_normal(N),
             "bernoulli": (rng.random(N) < 0.5).astype(np.float64)}[lik]
        ms.append(T.GLM(X, y, lik))
    return T.Batched(ms)


KW = dict(psis_fn=M.psis_fn, loglik_fn=M.loglik_fn, stats_fn=P.stats_fn)
LOO_KEYS = ("elpd_loo_i", "pareto_k", "n_tail", "ess_w", "elpd_loo", "p_loo", "se_loo", "looic", "n_bad_k")


@pytest.fixture(scope="module")
def job():
    tgt = _batched()
    x = torch.as_tensor(np.random.default_rng(1).standard_normal((3 * 4, 30, 3)) * 0.3)
    return tgt, x, tgt.loo(x, **KW)


def _same(a, b):
    return all(torch.equal(a[k], b[k]) or (torch.isnan(a[k]) == torch.isnan(b[k])).all() and
               torch.equal(torch.nan_to_num(a[k]), torch.nan_to_num(b[k])) for k in a)


def test_loo_finalise_and_constants(job):
    tgt, x, out = job
    S, N = 4 * 30, 70
    w = tgt.waic(x, stats_fn=P.stats_fn)
    assert all(torch.equal(out[k], w[k]) for k in w) and set(out) == set(w) | set(LOO_KEYS)
    ll = M.loglik_fn(x, tgt.params, 0, 4, 0, 2).numpy()                       # [3, 128, S]
    for g in range(3):
        const = tgt[g].loglik_constant()
        np.testing.assert_array_equal(const, [-math.lgamma(v + 1.0) for v in tgt[g].y])   # poisson
        rows = M.model_rows(ll[g, :N], M.tail_len(S))
        np.testing.assert_array_equal(out["elpd_loo_i"][g].numpy(), rows[:, 0] + const)
        np.testing.assert_array_equal(out["pareto_k"][g].numpy(), rows[:, 1])
        np.testing.assert_array_equal(out["n_tail"][g].numpy(), rows[:, 2])
        np.testing.assert_array_equal(out["ess_w"][g].numpy(), rows[:, 3])
        e = rows[:, 0] + const
        assert abs(float(out["elpd_loo"][g]) - e.sum()) <= 1e-12 * abs(e.sum())
        assert abs(float(out["se_loo"][g]) - math.sqrt(N * e.var(ddof=1))) <= 1e-12
        assert float(out["p_loo"][g]) == float(out["lppd_total"][g] - out["elpd_loo"][g])
        assert float(out["looic"][g]) == -2.0 * float(out["elpd_loo"][g])
        assert int(out["n_bad_k"][g]) == int((rows[:, 1] > predictive.BAD_K).sum())
    assert predictive.BAD_K == 0.7 and out["elpd_loo_i"].shape == (3, N) and out["elpd_loo"].shape == (3,)
    assert bool((out["elpd_loo"] <= out["lppd_total"]).all())
    one = tgt[1].loo(x[4:8], **KW)                                              # a single GLM: leading axis 1
    assert one["elpd_loo_i"].shape == (1, N) and torch.equal(one["elpd_loo_i"][0], out["elpd_loo_i"][1])


def test_chunking_and_blocks_do_not_change_a_bit(job):
    tgt, x, out = job
    unit = 64 * 4 * 30 * 8
    calls = []

    def counting(xb, table, first, per, ob0, ob1):
        calls.append((int(xb.shape[0]) // per, ob1 - ob0))
        return M.loglik_fn(xb, table, first, per, ob0, ob1)

    kw = dict(KW, loglik_fn=counting)
    assert _same(tgt.loo(x, scratch_bytes=1 << 30, **kw), out) and calls == [(3, 2)]
    del calls[:]
    assert _same(tgt.loo(x, scratch_bytes=2 * unit, **kw), out) and calls == [(1, 2)] * 3      # cut between groups
    del calls[:]
    assert _same(tgt.loo(x, scratch_bytes=5 * unit, **kw), out) and calls == [(2, 2), (1, 2)]
    del calls[:]
    assert _same(tgt.loo(x, scratch_bytes=unit, **kw), out) and calls == [(1, 1)] * 6          # cut inside a group
    with pytest.raises(ValueError, match=str(unit)):
        tgt.loo(x, scratch_bytes=unit - 1, **KW)
    assert _same(tgt.loo([x[:4], x[4:]], **KW), out)                                           # a list cut on a group boundary
    assert _same(tgt.loo([x[:8], x[8:8], x[8:]], scratch_bytes=unit, **KW), out)
    with pytest.raises(ValueError, match="straddles"):
        tgt.loo([x[:6], x[6:]], **KW)
    with pytest.raises(ValueError, match="straddles"):
        predictive.pointwise_loglik([x[:6], x[6:]], tgt, loglik_fn=M.loglik_fn)
    full = predictive.pointwise_loglik(x, tgt, loglik_fn=M.loglik_fn)
    assert full.shape == (3, 128, 120)
    part = predictive.pointwise_loglik([x[:4], x[4:]], tgt, groups=(1, 3), obs_blocks=(1, 2), loglik_fn=M.loglik_fn)
    assert torch.equal(part, full[1:3, 64:128])


def test_psis_host_function():
    r = np.stack([M.row("gaussian", 257), M.row("heavy", 257), M.row("lattice", 257)])
    t = torch.as_tensor(r)
    out = predictive.psis(t, psis_fn=M.psis_fn)
    assert set(out) == {"elpd_i", "pareto_k", "n_tail", "ess_w", "sigma", "min_loglik"} and out["elpd_i"].shape == (3,)
    for i in range(3):
        e, k, nt, ess, sg = M.psis_row(r[i])
        assert (float(out["elpd_i"][i]), float(out["pareto_k"][i]), int(out["n_tail"][i]), float(out["ess_w"][i]),
                float(out["sigma"][i])) == (e, k, nt, ess, sg) and float(out["min_loglik"][i]) == r[i].min()
    assert predictive.psis(t.reshape(3, 1, 257), psis_fn=M.psis_fn)["pareto_k"].shape == (3, 1)
    assert predictive.psis(t[0], psis_fn=M.psis_fn)["elpd_i"].shape == ()
    wide = torch.full((3, 300), float("inf"), dtype=torch.float64)
    wide[:, :257] = t
    assert torch.equal(predictive.psis(wide[:, :257], psis_fn=M.psis_fn)["elpd_i"], out["elpd_i"])   # row stride > S
    seen = []
    predictive.psis(t, reff=0.25, psis_fn=lambda l2, Mt: seen.append(Mt) or M.psis_fn(l2, Mt))
    assert seen == [M.tail_len(257, 0.25)] and seen[0] == 51 == predictive.tail_len(257, 0.25)
    with pytest.raises(ValueError, match="reff"):
        predictive.psis(t, reff=0.0, psis_fn=M.psis_fn)
    with pytest.raises(ValueError, match="contiguous last axis"):
        predictive.psis(torch.zeros((4, 10, 2), dtype=torch.float64)[:, :, 0], psis_fn=M.psis_fn)
    if not torch.cuda.is_available():
        with pytest.raises(_abi.HipLibraryError):
            predictive.psis(t)


def test_refusals(job, monkeypatch):
    tgt, x, _out = job
    ok = (np.zeros((6, 3)), np.zeros(6))
    with pytest.raises(ValueError, match="in-sample"):
        tgt.loo(x, data=[ok, ok, ok], **KW)
    with pytest.raises(TypeError, match="GLM"):
        predictive.loo(x, T.StdNormal(3), **KW)
    with pytest.raises(ValueError, match="multiple"):
        tgt.loo(x[:11], **KW)
    # M > 4096: refused from the shapes alone, before anything is computed (x is never read)
    big = torch.zeros((1, 1), dtype=torch.float64).expand(1, 1870000)
    with pytest.raises(ValueError, match=r"4096.*fewer draws.*::k"):
        predictive.psis(big, psis_fn=M.psis_fn)
    assert predictive.tail_len(1860000) == 4092 and predictive.tail_len(1870000) > _abi.PSIS_MAX_TAIL
    huge = torch.zeros((1, 1, 1), dtype=torch.float64).expand(3, 1870000, 3)
    with pytest.raises(ValueError, match="4096"):
        tgt.loo(huge, **KW)
    import torch.distributed as dist

    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    with pytest.raises(ValueError, match="process group"):
        tgt.loo(x, **KW)
    with pytest.raises(ValueError, match="process group"):
        predictive.pointwise_loglik(x, tgt, loglik_fn=M.loglik_fn)


def test_abi_symbols_constant_and_refusals_before_any_hip_call():
    lib = _abi.load()
    for name in ("lmc_glm_pointwise_loglik", "lmc_psis_rows"):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lmc_hip.h")).read()
    assert "#define LMC_PSIS_MAX_TAIL 4096" in header and _abi.PSIS_MAX_TAIL == 4096 == M.MAX_TAIL
    assert lib.lmc_abi_version() == 9
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def psis(l=p, rows=1, S=100, stride=100, tail=20, out=p):
        return lib.lmc_psis_rows(l, rows, S, stride, tail, out, None)

    for kw in (dict(l=None), dict(out=None), dict(rows=0), dict(S=0), dict(stride=99), dict(tail=-1),
               dict(S=10 ** 8, stride=10 ** 8, tail=_abi.PSIS_MAX_TAIL + 1), dict(tail=100), dict(tail=101),
               dict(S=2, stride=2, tail=2)):
        assert psis(**kw) == 1, kw   # LMC_ERR_INVALID
    d, N = 3, 70
    row_len = T.glm_row_layout(N, d)["size"]

    def ll(x=p, chains=4, stride=10, dim=d, t0=0, n=10, rows=p, row_len=row_len, n_rows=2, first=0, per=2, ob0=0, ob1=2, out=p):
        return lib.lmc_glm_pointwise_loglik(x, chains, stride, dim, t0, n, rows, row_len, n_rows, first, per, ob0, ob1, out, None)

    for kw in (dict(x=None), dict(rows=None), dict(out=None), dict(chains=0), dict(chains=2 ** 31), dict(dim=0), dict(n=0),
               dict(t0=-1), dict(t0=1), dict(first=-1), dict(per=0), dict(dim=_abi.GLM_MAX_DIM + 1), dict(row_len=row_len + 2),
               dict(row_len=8), dict(n_rows=1), dict(n_rows=0),
               dict(first=1), dict(chains=3), dict(per=3), dict(first=2, n_rows=2),      # whole groups, inside the table
               dict(ob0=-1), dict(ob0=1, ob1=1), dict(ob0=2, ob1=1), dict(ob1=3)):
        assert ll(**kw) == 1, kw   # LMC_ERR_INVALID
