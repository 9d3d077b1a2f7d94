"""-m gpu: lmc_glm_linpred (csrc/lmc_linpred.hip) -- the linear predictor of every draw at the points to predict at, written
for the radix select, and the moments of it and of the mean response -- against the 50-digit reference within the bounds
derived in tests/_linpred_model.py, and littlemcmc_amd/predictive.py (linear_predictor, predict) on top of it. Tensors are made
with torch; only the last test but one runs a sampler."""
import ctypes

import numpy as np
import pytest
import torch

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi, predictive
from littlemcmc_amd import diagnostics as dg
from littlemcmc_amd import targets as T
from tests import _glm_model as G
from tests import _linpred_model as M
from tests import _predictive_model as P
from tests.test_gpu_predictive import DRAW_COUNTS, SHAPES, _three_groups

pytestmark = pytest.mark.gpu

GUARD = -7.25   # what the guard elements around an output hold


def _glm(N, d, lik):
    X, y, _Q = G.case(N, d, lik)
    return T.GLM(X, y, lik, prior_scale=G.PRIOR_SCALE, sigma=G.SIGMA)


def _raw(x, table, first, per, ob0, ob1, want_eta=True, want_stats=True, guard=0):
    """One call of lmc_glm_linpred with guard elements around both outputs: (eta[c, n, W], stats[groups, 5, W], the two guarded
    buffers)."""
    c, n, d = x.shape
    W = 64 * (ob1 - ob0)
    groups = dg._touched(first, c, per)[1]
    e_flat = torch.full((guard + c * n * W + guard,), GUARD, dtype=torch.float64, device="cuda")
    s_flat = torch.full((guard + groups * 5 * W + guard,), GUARD, dtype=torch.float64, device="cuda")
    eta, st = e_flat[guard:guard + c * n * W].view(c, n, W), s_flat[guard:guard + groups * 5 * W].view(groups, 5, W)
    torch.cuda.synchronize()
    rc = _abi.load().lmc_glm_linpred(ctypes.c_void_p(x.data_ptr()), c, x.stride(0) // d if c > 1 else n, d, 0, n,
                                     ctypes.c_void_p(table.data_ptr()), table.shape[1], table.shape[0], first, per, ob0, ob1,
                                     ctypes.c_void_p(eta.data_ptr()) if want_eta else None,
                                     ctypes.c_void_p(st.data_ptr()) if want_stats else None, None)
    torch.cuda.synchronize()
    assert rc == _abi.OK, rc
    return eta, st, e_flat, s_flat


def _table(tgt):
    return torch.from_numpy(np.ascontiguousarray(tgt.params, dtype=np.float64).reshape(getattr(tgt, "groups", 1), -1)).cuda()


def _planes(st, g=0):
    return np.stack([st[k][g].cpu().numpy() for k in predictive.MOMENT_PLANES])


@pytest.mark.parametrize("lik", G.LIKELIHOODS)
@pytest.mark.parametrize("N,d", SHAPES)
def test_kernel_within_bound_of_reference(N, d, lik):
    """3 chains of 1, 7, 8, 9 and 17 draws (the leading draws of one [3, 17, d] tensor: chains lie 17 rows apart): every eta
    element and all five planes."""
    tgt = _glm(N, d, lik)
    count = P.CHAINS * P.MAX_DRAWS
    ref = M.case_reference(N, d, lik, count)
    full = torch.from_numpy(np.array(P.draws_of(N, d, lik, count)).reshape(P.CHAINS, P.MAX_DRAWS, d)).cuda()
    W = (N + 63) // 64 * 64
    for n in DRAW_COUNTS:
        eta, st = predictive.linear_predictor(full[:, :n], tgt)
        assert eta.shape == (P.CHAINS, n, W) and eta.is_cuda and st["n"].shape == (1, W) and bool((st["n"] == 3 * n).all())
        eta = eta.cpu().numpy()
        idx = [c * P.MAX_DRAWS + t for c in range(P.CHAINS) for t in range(n)]
        what = "%s N=%d d=%d n=%d" % (lik, N, d, n)
        assert not eta[:, :, N:].any(), what                                     # padding observations: eta = 0
        M.check_eta(eta[:, :, :N].reshape(-1, N), ref, idx, what)
        M.check_planes(_planes(st)[:, :N], ref, idx, what)


def test_more_draws_than_one_segment_within_bound():
    """2 chains x 300 draws: a chain is two wavefronts (256 + 44 draws, the last tile of 4), merged by the reduce kernel."""
    rng = np.random.default_rng(21)
    N, d, chains, n = 5, 3, 2, 300
    X = rng.standard_normal((N, d)) / 2.0
    tgt = T.GLM(X, rng.poisson(2.0, N).astype(np.float64), "poisson")
    job = 0.5 * rng.standard_normal((chains, n, d))
    ref = M.reference(X, job.reshape(-1, d), "poisson", P.reference_loglik(X, tgt.y, job.reshape(-1, d), "poisson"))
    eta, st = predictive.linear_predictor(torch.from_numpy(job).cuda(), tgt)
    M.check_eta(eta.cpu().numpy()[:, :, :N].reshape(-1, N), ref, what="two segments")
    M.check_planes(_planes(st)[:, :N], ref, what="two segments")
    half, _st = predictive.linear_predictor(torch.from_numpy(job[:, :256]).cuda(), tgt)   # one segment: the same eta bits
    assert torch.equal(half, eta[:, :256])


@pytest.mark.parametrize("d", [3, 65])
def test_eta_is_the_eta_of_the_likelihood_kernels_exactly(d):
    """Gaussian, N = 130 (three observation blocks): -0.5 * ((y - eta)**2 * isig2) formed in numpy float64 -- one rounding per
    operation, as the device forms it -- from the written eta is lmc_glm_pointwise_loglik's output, bit for bit."""
    N, chains, n = 130, 3, 9
    tgt = _glm(N, d, "gaussian")
    x = torch.from_numpy(np.array(P.draws_of(N, d, "gaussian", chains * n)).reshape(chains, n, d)).cuda()
    eta, _st = predictive.linear_predictor(x, tgt)
    ll = predictive.pointwise_loglik(x, tgt)                                      # [1, 192, S], s = chain * n + t
    assert ll.shape == (1, 192, chains * n) and eta.shape == (chains, n, 192)
    y = np.zeros(192)
    y[:N] = tgt.y
    res = y - eta.cpu().numpy().reshape(chains * n, 192)
    want = -0.5 * ((res * res) * tgt.isig2)
    assert np.array_equal(ll[0].cpu().numpy().T, want)


def test_observation_subranges_and_null_outputs_give_the_same_bits():
    N, d, chains, n = 130, 7, 3, 9
    tgt = _glm(N, d, "poisson")
    x = torch.from_numpy(np.array(P.draws_of(N, d, "poisson", chains * n)).reshape(chains, n, d)).cuda()
    eta, st = predictive.linear_predictor(x, tgt)
    for ob0, ob1 in ((1, 3), (0, 1)):
        e, s = predictive.linear_predictor(x, tgt, obs_blocks=(ob0, ob1))
        assert torch.equal(e, eta[:, :, 64 * ob0:64 * ob1])
        for k in predictive.MOMENT_PLANES:
            assert torch.equal(s[k], st[k][:, 64 * ob0:64 * ob1]), (k, ob0, ob1)
    table = _table(tgt)
    e_both, s_both, _ef, _sf = _raw(x, table, 0, chains, 0, 3)
    assert torch.equal(e_both, eta) and all(torch.equal(s_both[:, i], st[k]) for i, k in enumerate(predictive.MOMENT_PLANES))
    e_none, s_only, _ef, _sf = _raw(x, table, 0, chains, 0, 3, want_eta=False)
    assert torch.equal(s_only, s_both) and bool((e_none == GUARD).all())           # eta = NULL: the same stats bits
    e_only, s_none, _ef, _sf = _raw(x, table, 0, chains, 0, 3, want_stats=False)
    assert torch.equal(e_only, e_both) and bool((s_none == GUARD).all())           # stats = NULL: the same eta bits


def test_groups_partial_first_group_and_blocks_cut_inside_a_group():
    tgt = _three_groups()
    rng = np.random.default_rng(12)
    job = rng.standard_normal((9, 11, 5))           # the job: 3 groups of 3 chains
    xd = torch.from_numpy(job).cuda()
    table = _table(tgt)
    refs = []
    for g in range(3):
        q = job[3 * g:3 * g + 3].reshape(-1, 5)
        refs.append(M.reference(tgt[g].X, q, "bernoulli", P.reference_loglik(tgt[g].X, tgt[g].y, q, "bernoulli")))
    # 7 chains from chain 2 of the job: group 0 holds one chain of its three, groups 1 and 2 are whole
    eta, st, _ef, _sf = _raw(xd[2:], table, 2, 3, 0, 2)
    st = st.cpu().numpy()
    assert st.shape == (3, 5, 128) and [float(v) for v in st[:, 0, 0]] == [11.0, 33.0, 33.0]
    M.check_planes(st[0][:, :65], refs[0], range(22, 33), what="partial group 0")
    M.check_eta(eta[0].cpu().numpy()[:, :65], refs[0], range(22, 33), what="partial group 0")
    for g in (1, 2):
        M.check_planes(st[g][:, :65], refs[g], what="group %d" % g)
    # two blocks cut inside group 1, merged on the host
    a, b = _raw(xd[:4], table, 0, 3, 0, 2)[1], _raw(xd[4:], table, 4, 3, 0, 2)[1]
    assert [float(v) for v in a[:, 0, 0]] == [33.0, 11.0] and [float(v) for v in b[:, 0, 0]] == [22.0, 33.0]
    merged = predictive.merge_moments(a[1], b[0]).cpu().numpy()
    M.check_planes(merged[:, :65], refs[1], what="group 1 merged from two blocks")
    # predict: the whole job as one block and as the two blocks
    one, two = tgt.predict(xd), tgt.predict([xd[:4], xd[4:]])
    for out in (one, two):
        for g in range(3):
            val, bnd = M.reference_planes(refs[g])
            assert P.within(out["eta_mean"][g].cpu().numpy(), val[1], bnd[1] + M.U * np.abs(val[1])).all(), g
            assert P.within(out["mu_mean"][g].cpu().numpy(), val[3], bnd[3] + M.U * np.abs(val[3])).all(), g
    assert torch.equal(one["eta_quantiles"], two["eta_quantiles"]) and torch.equal(one["mu_quantiles"], two["mu_quantiles"])
    for k in ("eta_mean", "eta_sd", "mu_mean", "mu_sd", "y_mean", "y_var"):   # groups 0 and 2 lie inside one block either way
        assert one[k].shape == (3, 65) and torch.equal(one[k][0], two[k][0]) and torch.equal(one[k][2], two[k][2]), k


def test_the_select_on_the_devices_own_output():
    """The order statistics predict() returns are np.sort of the eta read back from the device, bit for bit; the band of the
    mean response is torch's inverse link of the same two neighbours; one observation block per chunk changes nothing."""
    rng = np.random.default_rng(40)
    N, d, per, n = 70, 4, 3, 41
    ms = [T.GLM(rng.standard_normal((N, d)) / 2.0, rng.poisson(2.0, N).astype(np.float64), "poisson") for _ in range(3)]
    tgt = T.Batched(ms)
    Xn = [rng.standard_normal((N + 3, d)) / 2.0 for _ in range(3)]
    x = torch.from_numpy(0.5 * rng.standard_normal((3 * per, n, d))).cuda()
    probs = [0.05, 0.5, 0.95, 0.0, 1.0]
    out = tgt.predict(x, Xn, probs=probs)
    eta, st = predictive.linear_predictor(x, tgt, Xn)
    S, n_new = per * n, N + 3
    srt = np.sort(eta.cpu().numpy().reshape(3, S, 128)[:, :, :n_new], axis=1)
    h = [p * (S - 1) for p in probs]
    lo = [int(np.floor(v)) for v in h]
    hi = [min(k + 1, S - 1) for k in lo]
    frac = np.array([a - b for a, b in zip(h, lo)]).reshape(-1, 1)
    assert out["eta_quantiles"].shape == (3, 5, n_new) and out["n"] == S
    assert np.array_equal(out["eta_quantiles"].cpu().numpy(), srt[:, lo] + (srt[:, hi] - srt[:, lo]) * frac)
    mlo, mhi = torch.exp(torch.from_numpy(srt[:, lo]).cuda()), torch.exp(torch.from_numpy(srt[:, hi]).cuda())
    assert torch.equal(out["mu_quantiles"], mlo + (mhi - mlo) * torch.from_numpy(frac).cuda())
    assert torch.equal(out["eta_mean"], st["eta_mean"][:, :n_new]) and torch.equal(out["y_mean"], st["mu_mean"][:, :n_new])
    var = st["mu_M2"][:, :n_new] / (st["n"][:, :n_new] - 1.0)   # (a tensor divisor: a division, as in predict())
    assert torch.equal(out["y_var"], st["mu_mean"][:, :n_new] + var) and torch.equal(out["mu_sd"], torch.sqrt(var))
    unit, ranks = 3 * per * n * 64 * 8, len(set([0, S - 1] + lo + hi))
    chunked = tgt.predict(x, Xn, probs=probs, scratch_bytes=unit + 256 * 64 * 8 * ranks)   # room for one observation block
    for k, v in out.items():
        if torch.is_tensor(v):
            assert torch.equal(v, chunked[k]), k


@pytest.mark.parametrize("N,d", [(63, 3), (65, 65)])
def test_addressing_reads_and_writes_nothing_too_many(N, d):
    """x = big[:, :n] with big[:, n:] = inf and the chain stride larger than n d, inside a larger buffer whose slack is inf
    too, and the one-row table inside a buffer of inf: a kernel that reads a padded coefficient (inf x 0 = NaN), a row of
    the trace or of the table too many differs from the call on clean copies. Both outputs lie between guard elements."""
    tgt = _glm(N, d, "bernoulli")
    chains, n, slack = 3, P.T + 1, 1024
    draws = torch.from_numpy(np.array(P.draws_of(N, d, "bernoulli", chains * n)).reshape(chains, n, d))
    flat = torch.full((slack + chains * (n + 3) * d + slack,), float("inf"), dtype=torch.float64, device="cuda")
    big = flat[slack:slack + chains * (n + 3) * d].view(chains, n + 3, d)
    big[:, :n] = draws.cuda()
    x = big[:, :n]
    assert not x.is_contiguous() and dg._row_major(x) and x.stride(0) == (n + 3) * d
    clean = _table(tgt)
    row_len = clean.shape[1]
    tflat = torch.full((slack + row_len + slack,), float("inf"), dtype=torch.float64, device="cuda")
    tflat[slack:slack + row_len] = clean[0]
    nob = (N + 63) // 64
    eta, st, e_flat, s_flat = _raw(x, tflat[slack:slack + row_len].view(1, row_len), 0, chains, 0, nob, guard=slack)
    want_eta, want_st, _ef, _sf = _raw(x.contiguous(), clean, 0, chains, 0, nob)
    assert bool(torch.isfinite(eta).all()) and bool(torch.isfinite(st).all())
    assert torch.equal(eta, want_eta) and torch.equal(st, want_st)
    for buf in (e_flat, s_flat):   # nothing written before or beyond [chains][n][W] and [groups][5][W]
        assert bool((buf[:slack] == GUARD).all()) and bool((buf[-slack:] == GUARD).all())
    assert bool((eta != GUARD).all()) and bool((st != GUARD).all())                # and every element inside was written


def test_a_nan_coefficient_stays_in_its_group():
    tgt = _three_groups()
    rng = np.random.default_rng(13)
    job = rng.standard_normal((9, 11, 5))
    clean = tgt.predict(torch.from_numpy(job).cuda())
    job[4, 6, 2] = np.nan                          # one coefficient of one draw of group 1
    bad = tgt.predict(torch.from_numpy(job).cuda())
    for k, v in bad.items():
        if torch.is_tensor(v):
            assert bool(torch.isnan(v[1]).all()), k                               # planes and quantiles, at every observation
            assert torch.equal(v[0], clean[k][0]) and torch.equal(v[2], clean[k][2]), k
            assert bool(torch.isfinite(clean[k]).all()), k


def test_two_calls_give_the_same_bits():
    rng = np.random.default_rng(8)
    N, d, G_, per, n = 130, 33, 4, 8, 300           # two segments a chain
    ms = [T.GLM(rng.standard_normal((N, d)) / 6.0, rng.poisson(2.0, N).astype(np.float64), "poisson") for _ in range(G_)]
    tgt = T.Batched(ms)
    x = torch.from_numpy(rng.standard_normal((G_ * per, n, d))).cuda()
    (ea, sa), (eb, sb) = predictive.linear_predictor(x, tgt), predictive.linear_predictor(x, tgt)
    assert torch.equal(ea, eb) and bool(torch.isfinite(ea).all())
    for k in predictive.MOMENT_PLANES:
        assert sa[k].shape == (G_, 192) and bool(torch.isfinite(sa[k]).all()) and torch.equal(sa[k], sb[k]), k


def test_end_to_end_prior_scale_ladder():
    """Batched of 4 gaussian GLMs (N = 32, d = 4) along prior scales 0.1, 1, 10, 100, sampled once: y_mean and y_var at the 16
    fresh points within 5 Monte-Carlo standard errors (inflated by sqrt(draws / ess_min), the multiple and the inflation of
    test_gpu_predictive.py's ladder test) of the closed form x'm and sigma^2 + x' Sigma x; the standard errors come from the
    draws themselves."""
    X, y, Xn, _yn, sigma = P.ladder()
    tgt = T.Batched([T.GLM(X, y, "gaussian", prior_scale=s, sigma=sigma) for s in P.LADDER_SCALES])
    trace, stats, eng = lmc.sample(tgt, tgt.d, chains=4 * 16, draws=200, tune=200, random_seed=11, progressbar=False,
                                   return_engine=True)
    try:
        x = dg.trace_tensor(eng)
        out = tgt.predict(x, [Xn] * 4)
        ess_min = tgt.summarize(x)["ess_min"].cpu().numpy()
        y_mean, y_var = out["y_mean"].cpu().numpy(), out["y_var"].cpu().numpy()
        band = out["mu_quantiles"].cpu().numpy()
    finally:
        eng.close()
    assert y_mean.shape == y_var.shape == (4, 16) and band.shape == (4, 3, 16) and not stats["diverging"].any()
    per_group = 16 * 200
    assert out["n"] == per_group
    for g, sl in enumerate(tgt.chain_slices(64)):
        mean, cov = tgt[g].posterior_gaussian()
        v = np.einsum("ne,ef,nf->n", Xn, cov, Xn)
        e = trace[sl].reshape(-1, 4) @ Xn.T                       # the draws of eta themselves
        c = e - e.mean(axis=0)
        m2, m4 = (c ** 2).mean(axis=0), (c ** 4).mean(axis=0)
        se_mean, se_var = np.sqrt(m2 / per_group), np.sqrt((m4 - m2 ** 2) / per_group)
        infl = np.sqrt(per_group / ess_min[g])
        print("group %d: ess_min %.0f, z mean %s, z var %s" % (
            g, ess_min[g], np.abs(y_mean[g] - Xn @ mean) / (se_mean * infl), np.abs(y_var[g] - (sigma ** 2 + v)) / (se_var * infl)))
        assert (np.abs(y_mean[g] - Xn @ mean) <= 5 * se_mean * infl).all(), g
        assert (np.abs(y_var[g] - (sigma ** 2 + v)) <= 5 * se_var * infl).all(), g
        np.testing.assert_allclose(y_mean[g], e.mean(axis=0), rtol=1e-10, atol=1e-12)   # the draws themselves
        np.testing.assert_allclose(y_var[g], sigma ** 2 + e.var(axis=0, ddof=1), rtol=1e-10, atol=1e-12)
        assert (band[g, 0] < band[g, 1]).all() and (band[g, 1] < band[g, 2]).all()
        np.testing.assert_allclose(band[g], np.quantile(e, [0.05, 0.5, 0.95], axis=0), rtol=1e-10, atol=1e-12)


def test_two_blocks_on_two_devices_equal_the_one_device_result():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    tgt = _three_groups()
    rng = np.random.default_rng(14)
    job = rng.standard_normal((9, 11, 5))
    xd = torch.from_numpy(job).cuda()
    one = tgt.predict(xd)
    two = tgt.predict([xd[:4].contiguous(), xd[4:].to("cuda:1")])
    assert torch.equal(one["eta_quantiles"], two["eta_quantiles"]) and torch.equal(one["mu_quantiles"], two["mu_quantiles"])
    for g in range(3):
        q = job[3 * g:3 * g + 3].reshape(-1, 5)
        ref = M.reference(tgt[g].X, q, "bernoulli", P.reference_loglik(tgt[g].X, tgt[g].y, q, "bernoulli"))
        val, bnd = M.reference_planes(ref)
        assert two["eta_mean"].device == one["eta_mean"].device
        assert P.within(two["eta_mean"][g].cpu().numpy(), val[1], bnd[1] + M.U * np.abs(val[1])).all(), g
        assert P.within(two["mu_mean"][g].cpu().numpy(), val[3], bnd[3] + M.U * np.abs(val[3])).all(), g
