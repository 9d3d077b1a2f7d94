"""No-GPU checks of the replicated responses: the two C entry points' export, declaration and refusals; the Python model of the
sampler (tests/_yrep_model.py) by itself -- AS 241 against mpmath, the poisson samplers against the exact pmf, moments of the
other two, the cap on undecided elements on the GPU test's inputs -- and the host logic of littlemcmc_amd/predictive.py
(replicate, predict_response, ppc) with the numpy models injected for the HIP calls, against plain numpy."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from littlemcmc_amd import _abi, predictive
from littlemcmc_amd import targets as T
from tests import _counter_model as C
from tests import _linpred_model as LM
from tests import _select_model as SM
from tests import _yrep_model as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(yrep_fn=Y.yrep_fn, count_fn=SM.count_fn)


def test_symbols_are_exported_declared_and_bound():
    lib = _abi.load()
    header = open(os.path.join(ROOT, "include", "lmc_hip.h")).read()
    for name, n_args in (("lmc_glm_yrep", 16), ("lmc_glm_yrep_stats", 15)):
        assert name in _abi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert "int %s(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n," % name in header
        assert len(_abi._SIGNATURES[name][1]) == n_args
    assert "#define LMC_YREP_STATS 7" in header and _abi.YREP_STATS == Y.STATS == 7
    assert '0x6c6d6379 "lmcy"' in header and Y.C3_YREP == 0x6C6D6379 and Y.C3_YREP not in (C.C3_MOMENTUM, C.C3_UNIFORMS)
    assert lib.lmc_abi_version() == 9 and _abi.ABI_VERSION == 9
    for f in ("lmc_yrep.hip", "lmc_yrep.hpp"):
        assert os.path.exists(os.path.join(ROOT, "littlemcmc_amd", "csrc", f))


def test_refusals_before_any_hip_call():
    lib = _abi.load()
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    d, N = 3, 70                                   # npad = 128: two observation blocks
    row_len = T.glm_row_layout(N, d)["size"]

    def yrep(x=p, chains=4, stride=10, dim=d, t0=0, n=10, rows=p, row_len=row_len, n_rows=2, first=0, per=2, ob0=0, ob1=2, y=p):
        return lib.lmc_glm_yrep(x, chains, stride, dim, t0, n, rows, row_len, n_rows, first, per, ob0, ob1, 7, y, None)

    def stats(x=p, chains=4, stride=10, dim=d, t0=0, n=10, rows=p, row_len=row_len, n_rows=2, first=0, per=2, centre=p, T_=p):
        return lib.lmc_glm_yrep_stats(x, chains, stride, dim, t0, n, rows, row_len, n_rows, first, per, 7, centre, T_, None)

    common = (dict(x=None), dict(rows=None), dict(chains=0), dict(chains=2 ** 31), dict(dim=0), dict(n=0), dict(t0=-1), dict(t0=1),
              dict(first=-1), dict(first=2 ** 31), dict(per=0), dict(dim=_abi.GLM_MAX_DIM + 1), dict(row_len=row_len + 2),
              dict(row_len=8), dict(n_rows=1), dict(n_rows=0), dict(first=2))
    for kw in common + (dict(y=None), dict(ob0=-1), dict(ob0=1, ob1=1), dict(ob0=2, ob1=1), dict(ob1=3),
                        dict(chains=2 ** 20, per=2 ** 20, stride=2 ** 14, n=2 ** 14, ob1=1),     # chains n W = 2^40 elements
                        dict(chains=2 ** 30, per=2 ** 30, n=1)):                                  # 2^31 wavefronts
        assert yrep(**kw) == 1, kw   # LMC_ERR_INVALID
    for kw in common + (dict(centre=None), dict(T_=None),
                        dict(chains=2 ** 30, per=2 ** 30, stride=2 ** 8, n=2 ** 8),               # chains n 7 >= 2^40
                        dict(chains=2 ** 26, per=2 ** 26, stride=2 ** 10, n=2 ** 10)):            # 2^31 wavefronts
        assert stats(**kw) == 1, kw
    if lib.lmc_device_count() == 0:
        # accepted arguments pass every refusal and fail at the header copy, the first HIP call: LMC_ERR_HIP, not INVALID
        for kw in (dict(), dict(ob0=1, ob1=2), dict(chains=2 ** 20, per=2 ** 20, stride=2 ** 14, n=2 ** 14 - 1, ob1=1)):
            assert yrep(**kw) == 2, kw
        for kw in (dict(), dict(first=1, chains=3), dict(chains=2 ** 20, per=2 ** 20, stride=2 ** 10, n=2 ** 10)):
            assert stats(**kw) == 2, kw


def test_stream_is_the_counter_models_philox_and_its_own_space():
    w = Y.philox_vec(np.arange(6), 7, [0, 1, 2, 3, 4, 5], Y.C3_YREP, 123, 9)
    for r in range(6):
        assert tuple(int(v[r]) for v in w) == C.philox4x32_10((r, 7, r, Y.C3_YREP), (123, 9))
    for j in range(4):   # u_j: words (0, 1) of block j >> 1 for even j, words (2, 3) for odd j, the decision stream's 53 bits
        blk = C.philox4x32_10((5, 11, j >> 1, Y.C3_YREP), (99, 3))
        assert Y.integer(99, 3, 5, 11, j) / Y.TWO53 == C.words_to_unit(*(blk[2:] if j & 1 else blk[:2]))
        assert Y.integers_vec(99, 3, np.array([5]), 11, j)[0] == Y.integer(99, 3, 5, 11, j)
    s = Y.Stream(99, 3, 5, 11)
    assert [s.integer() for _ in range(4)] == [Y.integer(99, 3, 5, 11, j) for j in range(4)]
    assert Y.integer(99, 3, 5, 11, 0) != Y.integer(99, 4, 5, 11, 0) != Y.integer(98, 4, 5, 11, 0)


def test_as241_statement_against_mpmath():
    """Both tails down to p = 2^-54, the |q| = 0.425 and r = 5 seams, both ends, the centre: the worst error is E_Z."""
    worst = 0.0
    for m in Y.normal_grid():
        z = Y.normal(m)
        assert math.isfinite(z) and Y.normal(int(Y.TWO53) - 1 - m) == -z             # finite and antisymmetric
        worst = max(worst, abs(z - Y.normal_exact(m)))
    print("AS 241 in float64: worst |z - z_exact| = %.3g over %d values of m" % (worst, len(Y.normal_grid())))
    assert worst <= Y.E_Z
    assert Y.normal(0) == -Y.normal(int(Y.TWO53) - 1) and abs(Y.normal(0) + 8.29236107581) < 1e-9    # p = 2^-54
    assert 0.0 < Y.normal(2 ** 52) < 2e-16 and Y.normal(2 ** 52 - 1) == -Y.normal(2 ** 52)           # no m gives z = 0 ... or p = 1/2


@pytest.mark.parametrize("lam", [0.3, 9.99, 10.0, 37.0, 1e3, 1e6])
def test_poisson_goodness_of_fit(lam):
    """2e5 samples of the model at one lam against the exact pmf: chi-square on bins of expected count >= 20, p > 1e-6 (a
    wrong PTRS constant or an off-by-one of the multiplication method gives p = 0). The vectorised sampler is the scalar one."""
    y = Y.poisson_bulk(lam, 4242, 200000)
    stat, dof, p = Y.poisson_gof(y, lam)
    print("lam %g: mean %.5g var %.5g chi2 %.1f on %d dof, p = %.3g" % (lam, y.mean(), y.var(), stat, dof, p))
    assert p > 1e-6
    for r in range(200):
        assert Y.poisson(lam, Y.Stream(4242, 0, r, 0), exact=False)[0] == y[r]
    for r in range(25):   # ... and the float64 decisions are the 50-digit ones wherever the element is decided
        v, decided = Y.poisson(lam, Y.Stream(4242, 0, r, 0), exact=True)
        assert v == y[r] or not decided


def test_bernoulli_and_gaussian_moments():
    n = 200000
    r = np.arange(n)
    u = Y.integers_vec(7, 1, r, 3, 0) / Y.TWO53
    for mu in (0.03, 0.5, 0.9):
        yb = (u < mu).astype(np.float64)
        assert abs(yb.mean() - mu) <= 5.0 * math.sqrt(mu * (1.0 - mu) / n)
        assert all(Y.bernoulli(mu, Y.Stream(7, 1, k, 3))[0] == yb[k] for k in range(50))
    z = Y.normals_vec(Y.integers_vec(7, 1, r[:50000], 3, 0))
    m = len(z)
    assert abs(z.mean()) <= 5.0 / math.sqrt(m) and abs(z.var() - 1.0) <= 5.0 * math.sqrt(2.0 / m)
    assert abs((z ** 3).mean()) <= 5.0 * math.sqrt(15.0 / m) and abs((z ** 4).mean() - 3.0) <= 5.0 * math.sqrt(96.0 / m)
    v, decided = Y.element("gaussian", 1.5, 1.5, 0.25, 7, 1, 0, 3)
    assert decided and v == 0.25 * z[0] + 1.5


def test_non_finite_and_edge_elements():
    nan, inf = float("nan"), float("inf")
    for lik in Y.CODES:
        assert math.isnan(Y.element(lik, nan, 0.5, 1.0, 1, 0, 0, 0)[0]) and math.isnan(Y.element(lik, 0.0, nan, 1.0, 1, 0, 0, 0)[0])
        assert math.isnan(Y.element(lik, 710.0, inf, 1.0, 1, 0, 0, 0)[0])
    assert math.isnan(Y.element("poisson", 37.0, 2.0 ** 52 * 1.5, 1.0, 1, 0, 0, 0)[0])
    assert Y.element("poisson", -800.0, 0.0, 1.0, 1, 0, 0, 0) == (0.0, True)
    assert Y.element("bernoulli", -800.0, 0.0, 1.0, 1, 0, 0, 0)[0] == 0.0 and Y.element("bernoulli", 40.0, 1.0, 1.0, 1, 0, 0, 0)[0] == 1.0
    assert not Y.poisson(10.0 * (1.0 + 1e-13), Y.Stream(1, 0, 0, 0))[1]            # lam at the threshold between the two methods


@pytest.mark.parametrize("name", Y.CELLS)
def test_cells_of_the_gpu_test_meet_the_cap(name):
    """The model alone on the GPU test's inputs, with numpy's eta (the device's differs by ulps): at most MAX_UNDECIDED
    undecided elements a cell; the poisson cell holds mu on both sides of 10, up to 1e6, a certain 0 and a certain NaN."""
    c = Y.cell(name)
    table = Y.table_of(c)
    eta, _st = LM.linpred(c["x"], table, 0, c["per"], 0, int(table[0][2]) // 64)
    y, decided = Y.yrep(eta, table, 0, c["per"], 0, Y.SEED)
    N = c["N"]
    print("%s: %d elements, %d undecided" % (name, y[:, :, :N].size, int((~decided).sum())))
    assert int((~decided).sum()) <= Y.MAX_UNDECIDED
    assert not y[:, :, N:].any()
    if name == "poisson":
        with np.errstate(over="ignore"):
            mu = np.exp(eta[:, :, :68])
        assert mu.min() < 1.0 and (mu < 10.0).sum() > 100 and (mu > 10.0).sum() > 100 and 5e5 < mu.max() < 2e6
        assert (eta[:, :, 68] == -800.0).all() and (y[:, :, 68] == 0.0).all()
        assert (eta[:, :, 69] == 710.0).all() and np.isnan(y[:, :, 69]).all() and not np.isnan(y[:, :, :69]).any()
    else:
        assert not np.isnan(y).any()


def test_end_to_end_verdict_of_the_model_on_the_cpu():
    """The data seed of the GPU test's end-to-end case (E2E_DATA_SEED) was CHOSEN, among the first eight, so that the five
    non-degenerate p-values of data generated by the model lie well inside (0.05, 0.95): a p-value of well-specified data is
    uniform, so some seeds put one outside by chance. Here is the model's own verdict at that seed, in numpy on numpy's eta:
    what the GPU test then asks of the device."""
    good, bad = Y.e2e_verdict(1.0), Y.e2e_verdict(3.0)
    print("noise x1: %s\nnoise x3: %s" % (np.round(good, 3), np.round(bad, 3)))
    assert np.allclose(good, [0.496, 0.506, 0.209, 0.637, 1.0, 0.331], atol=0.002)
    assert ((good[[0, 1, 2, 3, 5]] > 0.1) & (good[[0, 1, 2, 3, 5]] < 0.9)).all() and good[4] == 1.0
    assert bad[5] == 0.0 and bad[1] == 0.0 and bad[4] == 1.0


# ---- the host logic, with the models injected ------------------------------------------------------------------------------------
def _batched(lik="poisson", G_=3, N=70, d=3):
    rng = np.random.default_rng(60)
    ms = []
    for g in range(G_):
        X = rng.standard_normal((N, d)) / 2.0
        y = {"poisson": rng.poisson(2.0, N).astype(float), "gaussian": rng.standard_normal(N),
             "bernoulli": (rng.random(N) < 0.5).astype(float)}[lik]
        ms.append(T.GLM(X, y, lik, prior_scale=1.0 + g, sigma=0.5 + g))
    return T.Batched(ms), [rng.standard_normal((N + 1, d)) / 2.0 for _ in range(G_)]


def _quantile_plan(S, probs):
    h = [p * (S - 1) for p in probs]
    lo = [int(math.floor(v)) for v in h]
    return np.array(lo), np.array([min(k + 1, S - 1) for k in lo]), np.array([a - b for a, b in zip(h, lo)]).reshape(-1, 1)


def test_predict_response_against_plain_numpy_groups_blocks_and_chunks():
    tgt, Xn = _batched()
    rng = np.random.default_rng(61)
    per, draws, n_new, probs = 2, 9, 71, (0.05, 0.5, 0.95, 0.0, 1.0)
    x = torch.from_numpy(0.5 * rng.standard_normal((3 * per, draws, 3)))
    one = tgt.predict_response(x, Xn, probs=probs, random_seed=5, **KW)
    S = per * draws
    assert one["n"] == S and one["probs"] == list(probs) and one["y_quantiles"].shape == (3, 5, n_new)
    y_all = tgt.replicate(x, Xn, random_seed=5, yrep_fn=Y.yrep_fn).numpy()            # [6, 9, 128]: the model's own array
    table = np.stack([T.GLM(Xn[g], np.zeros(n_new), "poisson", prior_scale=tgt[g].prior_scale, sigma=tgt[g].sigma).params
                      for g in range(3)])
    eta = LM.linpred(x.numpy(), table, 0, per, 0, 2)[0]
    assert np.array_equal(y_all, Y.yrep(eta, table, 0, per, 0, 5, exact=False)[0]) and not y_all[:, :, n_new:].any()
    lo, hi, frac = _quantile_plan(S, probs)
    for g in range(3):
        pool = np.sort(y_all[per * g:per * g + per].reshape(S, 128)[:, :n_new], axis=0)
        got = one["y_quantiles"][g].numpy()
        assert np.array_equal(got, pool[lo] + (pool[hi] - pool[lo]) * frac)            # order statistics: bit for bit
        assert np.array_equal(one["y_min"][g].numpy(), pool[0]) and np.array_equal(one["y_max"][g].numpy(), pool[-1])
        assert np.array_equal(got[3], pool[0]) and np.array_equal(got[4], pool[-1])
        npq = np.quantile(pool, probs, axis=0)                                         # numpy's own interpolation: a few ulps
        assert (np.abs(got - npq) <= 4 * LM.U * np.maximum(np.abs(pool[lo]), np.abs(pool[hi]))).all()
    # another seed is another array; a sub-range of observation blocks is the same bits
    assert not np.array_equal(tgt.replicate(x, Xn, random_seed=6, yrep_fn=Y.yrep_fn).numpy(), y_all)
    assert np.array_equal(tgt.replicate(x, Xn, random_seed=5, obs_blocks=(1, 2), yrep_fn=Y.yrep_fn).numpy(), y_all[:, :, 64:])
    # a list of two blocks that cuts group 1: the select is exact, so every output keeps its bits
    two = tgt.predict_response([x[:3], x[3:]], Xn, probs=probs, random_seed=5, **KW)
    # scratch_bytes that forces one observation block per chunk: the same bits; one byte less: refused, the unit named
    unit = 3 * per * draws * 64 * 8
    counts = 256 * 64 * 8 * len({0, S - 1} | set(lo.tolist()) | set(hi.tolist()))
    calls = []

    def counting(*a):
        calls.append(a[4:6])
        return Y.yrep_fn(*a)

    chunked = tgt.predict_response(x, Xn, probs=probs, random_seed=5, scratch_bytes=unit + counts, yrep_fn=counting,
                                   count_fn=SM.count_fn)
    assert calls == [(0, 1), (1, 2)]
    for other in (two, chunked):
        for k in ("y_quantiles", "y_min", "y_max"):
            assert torch.equal(one[k], other[k]), k
    with pytest.raises(ValueError, match="64 x 8 = %d bytes" % unit):
        tgt.predict_response(x, Xn, scratch_bytes=unit + counts - 1, **KW)
    # X_new=None: the training design; one GLM: a leading axis of 1
    tr = tgt.predict_response(x, random_seed=5, **KW)
    assert tr["y_quantiles"].shape == (3, 3, 70)
    solo = tgt[0].predict_response(x[:2], Xn[0], random_seed=5, **KW)
    assert torch.equal(solo["y_quantiles"][0], tgt.predict_response(x, Xn, random_seed=5, **KW)["y_quantiles"][0])


@pytest.mark.parametrize("lik", Y.CODES)
def test_ppc_against_plain_numpy(lik):
    tgt, _Xn = _batched(lik, N=9)
    rng = np.random.default_rng(62 + Y.CODES.index(lik))
    per, draws, N, probs = 2, 11, 9, (0.05, 0.5, 0.95)
    xs = 0.5 * rng.standard_normal((3 * per, draws, 3))
    x = torch.from_numpy(xs)
    seen = []                                      # the planes the injected model handed to ppc, call by call

    def recording(*a):
        seen.append(Y.stats_fn(*a))
        return seen[-1]

    out = tgt.ppc(x, random_seed=9, probs=probs, stats_fn=recording, count_fn=SM.count_fn)
    S = per * draws
    assert out["names"] == ("mean", "sd", "min", "max", "zeros", "chisq") and out["n"] == S
    assert out["T_obs"].shape == (3, 5) and out["T_rep_mean"].shape == (3, 5) and out["T_rep_quantiles"].shape == (3, 3, 5)
    assert out["p_value"].shape == (3, 6) and len(seen) == 1 and seen[0].shape == (6, draws, 7)
    assert set(out) == {"T_obs", "T_rep_mean", "T_rep_quantiles", "p_value", "names", "n", "probs"}
    table = tgt.params.reshape(3, -1)
    centre = np.array([m.y.sum() / N for m in tgt.members])
    Tm = Y.stats(xs, table, 0, per, 9, centre)
    assert np.array_equal(seen[0].numpy(), Tm)
    lo, hi, frac = _quantile_plan(S, probs)
    for g, m in enumerate(tgt.members):
        t = Tm[per * g:per * g + per].reshape(S, 7)
        c = centre[g]
        dev = t[:, 0] - N * c
        var = (t[:, 1] - dev * dev / N) / (N - 1.0)                                   # the variance formula of the issue
        tr = np.stack([t[:, 0] / N, np.sqrt(np.where(var < 0.0, 0.0, var)), t[:, 2], t[:, 3], t[:, 4]], axis=1)
        # the replicated data set itself: sd and mean of y_rep as numpy has them
        eta = LM.linpred(xs[per * g:per * g + per], table, per * g, per, 0, 1)[0]
        yr = Y.yrep(eta, table, per * g, per, 0, 9, exact=False)[0].reshape(S, 64)[:, :N]
        assert np.allclose(tr[:, 0], yr.mean(axis=1), rtol=1e-13, atol=0) and np.allclose(tr[:, 1], yr.std(axis=1, ddof=1), rtol=1e-9, atol=1e-12)
        assert np.array_equal(tr[:, 2], yr.min(axis=1)) and np.array_equal(tr[:, 4], (yr == 0).sum(axis=1))
        dev_o = m.y.sum() - N * c
        var_o = (((m.y - c) ** 2).sum() - dev_o * dev_o / N) / (N - 1.0)
        t_obs = np.array([m.y.sum() / N, math.sqrt(max(var_o, 0.0)), m.y.min(), m.y.max(), float((m.y == 0).sum())])
        assert np.array_equal(out["T_obs"][g].numpy(), t_obs)
        assert np.allclose(t_obs[:2], [m.y.mean(), m.y.std(ddof=1)], rtol=1e-12, atol=0)
        p = np.concatenate([(tr >= t_obs).sum(axis=0), [(t[:, 5] >= t[:, 6]).sum()]]) / float(S)
        assert np.array_equal(out["p_value"][g].numpy(), p)                            # counts: bit for bit
        srt = np.sort(tr, axis=0)
        assert np.array_equal(out["T_rep_quantiles"][g].numpy(), srt[lo] + (srt[hi] - srt[lo]) * frac)
        assert np.allclose(out["T_rep_mean"][g].numpy(), tr.mean(axis=0), rtol=1e-13, atol=0)
    # a list that cuts group 1: the counts and the select are exact, the mean a sum of parts
    two = tgt.ppc([x[:3], x[3:]], random_seed=9, probs=probs, stats_fn=recording, count_fn=SM.count_fn)
    assert torch.equal(out["p_value"], two["p_value"]) and torch.equal(out["T_rep_quantiles"], two["T_rep_quantiles"])
    assert torch.allclose(out["T_rep_mean"], two["T_rep_mean"], rtol=1e-13, atol=0) and torch.equal(out["T_obs"], two["T_obs"])
    assert torch.equal(torch.cat(seen[1:]), seen[0])                                # the two parts are the rows of the whole
    # one GLM: a leading axis of 1 (its chains are job chains 0, 1: another stream than group 1 of the Batched);
    # another seed is another answer
    solo = tgt[1].ppc(x[per:2 * per], random_seed=9, probs=probs, stats_fn=Y.stats_fn, count_fn=SM.count_fn)
    assert solo["p_value"].shape == (1, 6) and torch.equal(solo["T_obs"][0], out["T_obs"][1])
    assert not torch.equal(tgt.ppc(x, random_seed=10, stats_fn=Y.stats_fn, count_fn=SM.count_fn)["T_rep_mean"], out["T_rep_mean"])


def test_refusals_of_the_host_functions(monkeypatch):
    tgt, Xn = _batched()
    x = torch.zeros((6, 4, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="list of 3 arrays"):
        tgt.predict_response(x, Xn[:2], **KW)
    with pytest.raises(ValueError, match="probs"):
        tgt.predict_response(x, Xn, probs=(1.5,), **KW)
    with pytest.raises(ValueError, match="probs"):
        tgt.ppc(x, probs=(), stats_fn=Y.stats_fn, count_fn=SM.count_fn)
    with pytest.raises(ValueError, match="multiple of 3 chains"):
        tgt.ppc(x[:5], stats_fn=Y.stats_fn, count_fn=SM.count_fn)
    with pytest.raises(TypeError):
        predictive.ppc(x, T.StdNormal(3), stats_fn=Y.stats_fn)
    with pytest.raises(ValueError, match="one tensor"):
        predictive.replicate([x], tgt, yrep_fn=Y.yrep_fn)
    with pytest.raises(ValueError, match="obs_blocks"):
        predictive.replicate(x, tgt, Xn, obs_blocks=(1, 3), yrep_fn=Y.yrep_fn)
    for call in (lambda: tgt.ppc(x), lambda: tgt.predict_response(x, Xn), lambda: tgt.replicate(x)):
        with pytest.raises(_abi.HipLibraryError):                     # no host implementation
            call()
    import torch.distributed as dist

    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    with pytest.raises(ValueError, match="process group"):
        tgt.ppc(x, stats_fn=Y.stats_fn, count_fn=SM.count_fn)
