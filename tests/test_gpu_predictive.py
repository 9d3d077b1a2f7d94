"""-m gpu: lmc_glm_pointwise (csrc/lmc_predict.hip) -- the per-observation statistics of the pointwise log-likelihood from
one pass over the draws in HBM -- against the 50-digit reference within the bound derived in tests/_predictive_model.py, and
littlemcmc_amd/predictive.py on top of it. Tensors are made with torch; only the last test but one runs a sampler."""
import ctypes

import numpy as np
import pytest
import torch

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi, predictive
from littlemcmc_amd import diagnostics as dg
from littlemcmc_amd import targets as T
from tests import _glm_model as G
from tests import _predictive_model as P

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (63, 3), (64, 64), (65, 65), (130, 130), (70, 300))
# draws per chain: 1, 7, 17 are below, across and no multiple of the kernel's tile of T = 8 draws (P.T: kPredT); 7 is T - 1,
# and T, T + 1 are added
DRAW_COUNTS = (1, 7, P.T, P.T + 1, 17)
assert P.T == 8 and {P.T - 1, P.T, P.T + 1} <= set(DRAW_COUNTS) and max(DRAW_COUNTS) == P.MAX_DRAWS


def _glm(N, d, lik):
    X, y, _Q = G.case(N, d, lik)
    return T.GLM(X, y, lik, prior_scale=G.PRIOR_SCALE, sigma=G.SIGMA)


def _block(st, g=0):
    return np.stack([st[k][g].cpu().numpy() for k in predictive.PLANES])


@pytest.mark.parametrize("lik", G.LIKELIHOODS)
@pytest.mark.parametrize("N,d", SHAPES)
def test_kernel_within_bound_of_reference(N, d, lik):
    """3 chains of 1, 7, 8, 9 and 17 draws (the leading draws of one [3, 17, d] tensor: chains lie 17 rows apart)."""
    tgt = _glm(N, d, lik)
    count = P.CHAINS * P.MAX_DRAWS
    ref = P.case_reference(N, d, lik, count)
    full = torch.from_numpy(np.array(P.draws_of(N, d, lik, count)).reshape(P.CHAINS, P.MAX_DRAWS, d)).cuda()
    for n in DRAW_COUNTS:
        st = tgt.pointwise_stats(full[:, :n])
        assert st["n"].shape == (1, N) and st["n"].is_cuda and bool((st["n"] == 3 * n).all())
        idx = [c * P.MAX_DRAWS + t for c in range(P.CHAINS) for t in range(n)]
        P.check_planes(_block(st), ref, idx, what="%s N=%d d=%d n=%d" % (lik, N, d, n))


def _three_groups(N=65, d=5, lik="bernoulli"):
    ms = []
    for g in range(3):
        rng = np.random.default_rng(900 + g)
        X = rng.standard_normal((N, d)) / np.sqrt(d)
        y = (rng.random(N) < 0.5).astype(np.float64)
        ms.append(T.GLM(X, y, lik, prior_scale=1.0 + g))
    return T.Batched(ms)


def test_groups_partial_first_group_and_blocks_cut_inside_a_group():
    tgt = _three_groups()
    rng = np.random.default_rng(12)
    job = rng.standard_normal((9, 11, 5))           # the job: 3 groups of 3 chains
    xd = torch.from_numpy(job).cuda()
    refs = [P.reference_loglik(tgt[g].X, tgt[g].y, job[3 * g:3 * g + 3].reshape(-1, 5), "bernoulli") for g in range(3)]
    # 7 chains from chain 2 of the job: group 0 holds one chain of its three, groups 1 and 2 are whole
    st = tgt.pointwise_stats(xd[2:], chains_per_group=3, first_chain=2)
    assert st["n"].shape == (3, 65) and [float(v) for v in st["n"][:, 0]] == [11.0, 33.0, 33.0]
    P.check_planes(_block(st, 0), refs[0], range(22, 33), what="partial group 0")
    for g in (1, 2):
        P.check_planes(_block(st, g), refs[g], what="group %d" % g)
    # the whole job as one block and as two blocks cut inside group 1
    one, two = tgt.pointwise_stats(xd), tgt.pointwise_stats([xd[:4], xd[4:]])
    for g in range(3):
        P.check_planes(_block(one, g), refs[g], what="one block, group %d" % g)
        P.check_planes(_block(two, g), refs[g], what="two blocks, group %d" % g)
    assert torch.equal(one["n"], two["n"])
    for k in predictive.PLANES:   # groups 0 and 2 lie inside one block either way: the same bits
        assert torch.equal(one[k][0], two[k][0]) and torch.equal(one[k][2], two[k][2]), k


def test_many_groups_share_the_wave_budget():
    """512 groups of 9 chains at one observation block: 4096 / 512 = 8 chain blocks per group, so a wavefront walks more
    than one chain and the last chain block of a group gets one chain only."""
    rng = np.random.default_rng(3)
    N, d, G_, per, n = 5, 3, 512, 9, 3
    ms = [T.GLM(rng.standard_normal((N, d)), rng.standard_normal(N), "gaussian", sigma=0.5 + (g % 3)) for g in range(G_)]
    tgt = T.Batched(ms)
    job = rng.standard_normal((G_ * per, n, d))
    st = tgt.pointwise_stats(torch.from_numpy(job).cuda())
    assert st["n"].shape == (G_, N) and bool((st["n"] == per * n).all())
    for g in (0, 1, 255, 511):
        ref = P.reference_loglik(ms[g].X, ms[g].y, job[g * per:(g + 1) * per].reshape(-1, d), "gaussian", ms[g].isig2)
        P.check_planes(_block(st, g), ref, what="group %d of 512" % g)
    got = np.stack([st[k].cpu().numpy() for k in predictive.PLANES], axis=1)   # every group against the numpy model, loosely
    want = P.stats_fn(torch.from_numpy(job), tgt.params, 0, per).numpy()
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("N,d", [(63, 3), (65, 65)])
def test_addressing_reads_no_coefficient_and_no_row_too_many(N, d):
    """x = big[:, :n] with big[:, n:] = inf and the chain stride larger than n d, inside a larger buffer whose slack is inf
    too: a kernel that reads a padded coefficient (inf x 0 = NaN) or a row too many differs from the contiguous copy."""
    tgt = _glm(N, d, "bernoulli")
    chains, n, slack = 3, P.T + 1, 1024
    draws = torch.from_numpy(np.array(P.draws_of(N, d, "bernoulli", chains * n)).reshape(chains, n, d))
    flat = torch.full((slack + chains * (n + 3) * d + slack,), float("inf"), dtype=torch.float64, device="cuda")
    big = flat[slack:slack + chains * (n + 3) * d].view(chains, n + 3, d)
    big[:, :n] = draws.cuda()
    x = big[:, :n]
    assert not x.is_contiguous() and dg._row_major(x) and x.stride(0) == (n + 3) * d
    got, want = tgt.pointwise_stats(x), tgt.pointwise_stats(x.contiguous())
    for k in predictive.PLANES:
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(got[k], want[k]), k


def test_poisson_overflow_keeps_lppd_finite():
    """One draw of 9 is scaled so that exp(eta) overflows at some observations (l = -inf there): m, S and so lppd are those
    of the other eight draws, within the bound; the count is 9; mean and M2 are non-finite and sum mu is +inf, as
    include/lmc_hip.h documents (P.check_planes asks exactly that of a reference with a dead draw)."""
    N, d = 63, 3
    tgt = _glm(N, d, "poisson")
    X, y, Q = G.case(N, d, "poisson")
    draws = np.array(P.draws_of(N, d, "poisson", 9))
    slope = np.array([0.0, Q[1][1], Q[1][2]])            # no intercept: the linear predictors spread around zero
    draws[4] = slope * (2768.0 / (X @ slope).max())
    eta4 = X @ draws[4]
    over = eta4 > 709.79
    # the fixture: exp(eta) clearly overflows or clearly does not (exp(660) ~ 1e286: no l between -1e290 and -inf)
    assert over.any() and not over.all() and not ((eta4 > 660.0) & ~over).any()
    ref = P.reference_loglik(X, y, draws, "poisson")
    xd = torch.from_numpy(draws.reshape(1, 9, d)).cuda()
    st = tgt.waic(xd)
    blk = _block(tgt.pointwise_stats(xd))
    P.check_planes(blk, ref, what="poisson overflow")
    assert (blk[0] == 9).all() and np.isfinite(blk[1:3]).all()
    assert not np.isfinite(blk[3][over]).any() and np.isnan(blk[4][over]).all() and np.isposinf(blk[5][over]).all()
    # where nothing overflowed the mean and sum mu are finite; M2 is too where the squared deviations are representable --
    # a finite l = -exp(400) has a square beyond the float64 range, an ordinary overflow that the reference rounds to the
    # same +inf (check_planes above)
    assert np.isfinite(blk[3][~over]).all() and np.isfinite(blk[5][~over]).all()
    assert np.isfinite(blk[4][eta4 < 345.0]).all() and (eta4 < 345.0).any()   # exp(345) ~ 1e150
    lppd = st["lppd"][0].cpu().numpy()
    assert np.isfinite(lppd).all()
    _val, _bnd, lse, lse_b = P.reference_planes(ref)
    want = lse - np.log(9.0) + tgt.loglik_constant()
    assert (np.abs(lppd - want) <= lse_b + 4 * P.U * (np.abs(lse) + np.abs(want) + 3.0)).all()
    # a NaN draw: every plane of every observation it touches but the count
    draws[2, 0] = np.nan
    bad = tgt.pointwise_stats(torch.from_numpy(draws.reshape(1, 9, d)).cuda())
    assert bool((bad["n"] == 9).all()) and all(bool(torch.isnan(bad[k]).all()) for k in predictive.PLANES[1:])


def test_entry_refuses_a_bad_header():
    tgt = _glm(63, 3, "gaussian")
    x = torch.zeros((2, 4, 3), dtype=torch.float64, device="cuda")
    out = torch.zeros((1, 6, 64), dtype=torch.float64, device="cuda")
    lib = _abi.load()

    def call(row, dim=3):
        table = torch.from_numpy(np.ascontiguousarray(row)).cuda().reshape(1, -1)
        torch.cuda.synchronize()
        return lib.lmc_glm_pointwise(ctypes.c_void_p(x.data_ptr()), 2, 4, dim, 0, 4, ctypes.c_void_p(table.data_ptr()),
                                     table.shape[1], 1, 0, 2, ctypes.c_void_p(out.data_ptr()), None)

    assert call(tgt.params) == _abi.OK
    for slot, val in ((0, 3.0), (0, 0.5), (1, 0.0), (1, 65.0), (2, 128.0), (5, 4.0), (6, 128.0)):
        row = tgt.params.copy()
        row[slot] = val
        assert call(row) == 1, (slot, val)   # LMC_ERR_INVALID
    torch.cuda.synchronize()


def test_end_to_end_prior_scale_ladder():
    """Batched of 4 gaussian GLMs (N = 32, d = 4) along prior scales 0.1, 1, 10, 100: lppd_n and p_waic_n of every rung within
    5 Monte-Carlo standard errors (inflated by sqrt(draws / ess_min)) of the closed form, the 0.1 rung the worst, held-out
    points scored [4, 16]. test_predictive_cpu.py checks that the closed form orders the rungs so by several se."""
    X, y, Xn, yn, sigma = P.ladder()
    tgt = T.Batched([T.GLM(X, y, "gaussian", prior_scale=s, sigma=sigma) for s in P.LADDER_SCALES])
    trace, stats, eng = lmc.sample(tgt, tgt.d, chains=4 * 16, draws=200, tune=200, random_seed=11, progressbar=False,
                                   return_engine=True)
    try:
        x = dg.trace_tensor(eng)
        out = tgt.waic(x)
        diag = tgt.summarize(x)
        held = tgt.waic(x, data=[(Xn, yn)] * 4)
        assert held["lppd"].shape == (4, 16) and bool(torch.isfinite(held["lppd"]).all())
        lppd, p_waic, elpd = out["lppd"].cpu().numpy(), out["p_waic"].cpu().numpy(), out["elpd_waic"].cpu().numpy()
        ess_min, held_lppd = diag["ess_min"].cpu().numpy(), held["lppd"].cpu().numpy()
    finally:
        eng.close()
    assert lppd.shape == p_waic.shape == (4, 32) and elpd.shape == (4,) and not stats["diverging"].any()
    per_group = 16 * 200
    for g, sl in enumerate(tgt.chain_slices(64)):
        m = tgt[g]
        lppd_exact, p_exact = P.gaussian_closed_form(m)
        q = trace[sl].reshape(-1, 4)
        ll = -0.5 * (y - q @ X.T) ** 2 / sigma ** 2 + m.loglik_constant()
        se_l, se_p = P.monte_carlo_errors(ll)
        infl = np.sqrt(per_group / ess_min[g])
        print("group %d: ess_min %.0f, z lppd %s, z p_waic %s" % (
            g, ess_min[g], np.abs(lppd[g] - lppd_exact) / (se_l * infl), np.abs(p_waic[g] - p_exact) / (se_p * infl)))
        assert (np.abs(lppd[g] - lppd_exact) <= 5 * se_l * infl).all(), g
        assert (np.abs(p_waic[g] - p_exact) <= 5 * se_p * infl).all(), g
        np.testing.assert_allclose(lppd[g], np.log(np.exp(ll).mean(axis=0)), rtol=1e-10, atol=1e-12)   # the draws themselves
    assert np.argmin(elpd) == 0 and elpd[0] < elpd[1:].min(), elpd
    for g, sl in enumerate(tgt.chain_slices(64)):   # the held-out fold: the same closed form at the new points
        hl, _hp = P.gaussian_closed_form(tgt[g], Xn, yn)
        ll = -0.5 * (yn - trace[sl].reshape(-1, 4) @ Xn.T) ** 2 / sigma ** 2 + tgt[g].loglik_constant(yn)
        se_l, _se_p = P.monte_carlo_errors(ll)
        assert (np.abs(held_lppd[g] - hl) <= 5 * se_l * np.sqrt(per_group / ess_min[g])).all(), g


def test_two_calls_give_the_same_bits():
    rng = np.random.default_rng(8)
    N, d, G_, per, n = 130, 33, 4, 8, 50
    ms = [T.GLM(rng.standard_normal((N, d)) / 6.0, rng.poisson(2.0, N).astype(np.float64), "poisson") for _ in range(G_)]
    tgt = T.Batched(ms)
    x = torch.from_numpy(rng.standard_normal((G_ * per, n, d))).cuda()
    a, b = tgt.pointwise_stats(x), tgt.pointwise_stats(x)
    for k in predictive.PLANES:
        assert a[k].shape == (G_, N) and bool(torch.isfinite(a[k]).all()) and torch.equal(a[k], b[k]), k
