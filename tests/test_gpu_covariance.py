"""-m gpu: lmc_diag_cross_moments (csrc/lmc_cross.hip) against the longdouble model of one call and its derived tolerance
(tests/_cross_model.py), its bits (symmetry, reproducibility, hostile draws), and covariance / contrasts above it. Each shape
is the smallest that reaches one way the kernel can go wrong. The kernel's plan constants the shapes are taken from:
geometry classes NTL 1 / 2 / 4 / 8 first used at d = 1 / 17 / 33 / 65, items of KC = 128 / 128 / 64 / 32 draws of one chain,
panels of 8 x 8 tiles at NTL 8 (a second panel row from d = 129), a budget of kCrossBudget = 1024 workgroups."""
import ctypes

import numpy as np
import pytest
import torch

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi
from littlemcmc_amd import diagnostics as dg
from littlemcmc_amd import targets as T
from tests import _cross_model as M

pytestmark = pytest.mark.gpu


def _job(groups, per, n, d, seed=41):
    """Correlated draws with a mean of order 10 (so that the shift matters) and a chain effect, seeded."""
    rng = np.random.default_rng(seed + 1000 * d)
    mix = rng.standard_normal((d, d)) / np.sqrt(d) + np.eye(d)
    x = rng.standard_normal((groups * per, n, d)) @ mix.T
    return np.ascontiguousarray(x + 10.0 + rng.standard_normal(d) + 0.5 * rng.standard_normal((groups * per, 1, d)))


@pytest.fixture(scope="module")
def ragged():
    """(G, per, n, d) = (3, 5, 61, 70): n no multiple of 4 or 32; the last tile row has 6 live columns."""
    x = _job(3, 5, 61, 70)
    return x, torch.from_numpy(x).cuda()


def _raw(xd, t0, n, first_chain, per, stride=None):
    """The C entry itself on a contiguous device tensor xd[chains, stride, d] -> numpy n[touched], mean, m2."""
    c, rows, d = xd.shape
    touched = M.touched(first_chain, c, per)[1]
    outs = [torch.full(s, -7.0, dtype=torch.float64, device=xd.device) for s in ((touched,), (touched, d), (touched, d, d))]
    stream = torch.cuda.current_stream(xd.device).cuda_stream
    rc = _abi.load().lmc_diag_cross_moments(ctypes.c_void_p(xd.data_ptr()), c, rows if stride is None else stride, d, t0, n,
                                            first_chain, per, *[ctypes.c_void_p(o.data_ptr()) for o in outs],
                                            ctypes.c_void_p(stream))
    assert rc == _abi.OK
    return [o.cpu().numpy() for o in outs]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_raw_entry_against_the_model_ragged_shape(ragged):
    x, xd = ragged
    n, mean, m2 = _raw(xd, 0, 61, 0, 5)
    assert n.tolist() == [305.0] * 3
    M.check(n, mean, m2, M.moments(x, 0, 5), "ragged (3, 5, 61, 70)")
    np.testing.assert_array_equal(_bits(m2), _bits(m2.transpose(0, 2, 1)))       # symmetric bit for bit
    n2, mean2, m22 = _raw(xd, 0, 61, 0, 5)                                        # and the same bits from a second call
    np.testing.assert_array_equal(_bits(m2), _bits(m22))
    np.testing.assert_array_equal(_bits(mean), _bits(mean2))
    one = _raw(xd, 0, 61, 0, 15)                                                  # one group of all chains
    M.check(*one, M.moments(x, 0, 15), "ragged, one group")


@pytest.mark.parametrize("d", [1, 15, 16, 17, 33, 65, 129, 512])
def test_dimensions_around_the_tile_and_panel_widths(d):
    """per = 2, n = 9, two groups. d = 1, 17, 33 and 65 are the first of the classes NTL 1, 2, 4 and 8; 15 / 16 / 17 lie around a
    tile, 129 is the first with a second panel row (one live tile row in it), 512 is the limit (10 panels)."""
    x = _job(2, 2, 9, d, seed=5)
    n, mean, m2 = _raw(torch.from_numpy(x).cuda(), 0, 9, 0, 2)
    M.check(n, mean, m2, M.moments(x, 0, 2), "d = %d" % d)
    np.testing.assert_array_equal(_bits(m2), _bits(m2.transpose(0, 2, 1)))


def test_a_view_into_longer_chains(ragged):
    """t0 = 3, n = 37 of draws_stride = 61."""
    x, xd = ragged
    M.check(*_raw(xd, 3, 37, 0, 5), M.moments(x, 0, 5, 3, 37), "t0 3, n 37 of 61")


def test_a_block_that_touches_three_groups_two_of_them_partly(ragged):
    """Chains 3 .. 11 of the job (first_chain = 3, per = 5, chains = 9): groups 0 and 2 partly, group 1 whole -- whose bits are
    those of the whole job's call (the split of a group's rows depends on the shapes of the call, and both calls have
    three touched groups of at most 5 chains). With the complementary blocks merged, the whole job's moments within the
    merged bound."""
    x, xd = ragged
    n, mean, m2 = _raw(xd[3:12].contiguous(), 0, 61, 3, 5)
    assert n.tolist() == [122.0, 305.0, 122.0]
    M.check(n, mean, m2, M.moments(x[3:12], 3, 5), "chains 3 .. 11")
    whole = _raw(xd, 0, 61, 0, 5)
    np.testing.assert_array_equal(_bits(m2[1]), _bits(whole[2][1]))
    merged = dg.cross_moments([xd[:3].contiguous(), xd[3:12].contiguous(), xd[12:].contiguous()], chains_per_group=5)
    want = []
    for g in range(3):
        acc = M.zero_part(70)
        for lo, hi in ((0, 3), (3, 12), (12, 15)):
            a, b = max(lo, 5 * g), min(hi, 5 * g + 5)
            if a < b:
                acc = M.merge_tolerance(acc, M.part(x[a:b].reshape(-1, 70).astype(M.LD)))
        want.append(acc)
    M.check(merged["n"].cpu().numpy(), merged["mean"].cpu().numpy(), merged["m2"].cpu().numpy(), want, "three blocks merged")


@pytest.mark.parametrize("groups,per,n,d", [(1, 2, 1, 3), (1, 1, 129, 3), (1, 1, 33, 70), (2, 700, 5, 3), (1025, 1, 2, 3)])
def test_groups_split_over_workgroups_and_more_groups_than_the_budget(groups, per, n, d):
    """(1, 2, 1, 3): two items (two chains of one chunk), two workgroups of one item each -- the smallest shape at which one
    group's rows are split and the reduction adds more than one partial. (1, 1, 129, 3) and (1, 1, 33, 70): the same with one
    chain of two chunks, the second of one draw (KC = 128 at d <= 32, 32 above 64). (2, 700, 5, 3): 512 workgroups per group
    are cut to 350 of two items. (1025, 1, 2, 3): more groups than the budget of 1024, one workgroup per group -- the smallest
    such shape."""
    x = _job(groups, per, n, d, seed=9)
    got = _raw(torch.from_numpy(x).cuda(), 0, n, 0, per)
    M.check(*got, M.moments(x, 0, per), "(%d, %d, %d, %d)" % (groups, per, n, d))
    np.testing.assert_array_equal(_bits(got[2]), _bits(got[2].transpose(0, 2, 1)))


def test_one_chain_with_one_draw():
    x = np.array([[[-3.5, 0.0, 2.0]]])
    n, mean, m2 = _raw(torch.from_numpy(x).cuda(), 0, 1, 0, 1)
    assert n.tolist() == [1.0]
    np.testing.assert_array_equal(mean, x[0])
    np.testing.assert_array_equal(_bits(m2), _bits(np.zeros((1, 3, 3))))
    c = dg.covariance(torch.from_numpy(x).cuda())
    assert torch.isnan(c["cov"]).all() and torch.isnan(c["corr"]).all()


def test_offset_data_stays_within_the_bound():
    """A column 1e8 + N(0, 1) next to a column N(0, 1e-6): the bound is in |x - shift|, an uncentred sum fails it."""
    rng = np.random.default_rng(17)
    x = np.stack([1e8 + rng.standard_normal((4, 300)), 1e-6 * rng.standard_normal((4, 300)), rng.standard_normal((4, 300))], axis=2)
    x = np.ascontiguousarray(x)
    M.check(*_raw(torch.from_numpy(x).cuda(), 0, 300, 0, 2), M.moments(x, 0, 2), "offset columns")


def test_hostile_draws_poison_their_coordinate_only():
    """(G, per, n, d) = (2, 3, 45, 37), a NaN and a +inf planted in coordinate j = 20 of two draws of group 1: mean[j] and row and
    column j of that group are non-finite; every other entry of the result has the bits of the unpoisoned run."""
    x = _job(2, 3, 45, 37, seed=23)
    clean = _raw(torch.from_numpy(x).cuda(), 0, 45, 0, 3)
    bad = x.copy()
    j = 20
    bad[3, 7, j], bad[5, 44, j] = np.nan, np.inf
    n, mean, m2 = _raw(torch.from_numpy(bad).cuda(), 0, 45, 0, 3)
    assert n.tolist() == [135.0, 135.0]
    assert not np.isfinite(mean[1, j]) and not np.isfinite(m2[1, j, :]).any() and not np.isfinite(m2[1, :, j]).any()
    keep = np.ones(37, dtype=bool)
    keep[j] = False
    np.testing.assert_array_equal(_bits(mean[1, keep]), _bits(clean[1][1, keep]))
    np.testing.assert_array_equal(_bits(m2[1][np.ix_(keep, keep)]), _bits(clean[2][1][np.ix_(keep, keep)]))
    np.testing.assert_array_equal(_bits(mean[0]), _bits(clean[1][0]))
    np.testing.assert_array_equal(_bits(m2[0]), _bits(clean[2][0]))
    corr = dg.covariance(torch.from_numpy(bad).cuda(), chains_per_group=3)["corr"][1].cpu().numpy()
    assert np.isnan(corr[j]).all() and np.isnan(corr[:, j]).all() and np.isfinite(corr[np.ix_(keep, keep)]).all()


def test_public_functions_on_the_device_equal_the_injected_model():
    """(G, per, n, d) = (3, 5, 200, 6): every entry of cov within the m2 bound / (n - 1), mean within its bound; corr, sd and
    the contrasts are a few rounded operations on those (rtol 1e-12 against the same functions of the model's moments)."""
    x = _job(3, 5, 200, 6)
    xt, xd = torch.from_numpy(x), torch.from_numpy(x).cuda()
    got, want = dg.covariance(xd, chains_per_group=5), dg.covariance(xt, chains_per_group=5, moments_fn=M.moments_fn)
    assert got["cov"].is_cuda and tuple(got["cov"].shape) == (3, 6, 6)
    M.check(got["n"].cpu().numpy(), got["mean"].cpu().numpy(), got["cov"].cpu().numpy() * 999.0,
            [dict(p, tol_m2=p["tol_m2"] + 2 * M.EPS * np.abs(p["m2"])) for p in M.moments(x, 0, 5)], "covariance() x (n - 1)")
    for k in ("cov", "corr", "sd", "mean"):
        np.testing.assert_allclose(got[k].cpu().numpy(), want[k].numpy(), rtol=1e-12, atol=1e-15, err_msg=k)
    b = T.Batched([T.AR1(6, rho=r) for r in (0.2, 0.97, -0.5)])
    for k in ("cov", "corr", "mean"):
        np.testing.assert_array_equal(b.covariance(xd)[k].cpu().numpy(), got[k].cpu().numpy())
    L = np.array([[0, 0, 0, 1.0, 0, -1.0], [1.0, 1.0, 0, 0, 0, 0]])
    kc, kw = b.contrasts(xd, L), dg.contrasts(want, L)
    for k in ("mean", "sd", "cov"):
        np.testing.assert_allclose(kc[k].cpu().numpy(), kw[k].numpy(), rtol=1e-12, atol=1e-15, err_msg=k)
    rows = x[:5].reshape(-1, 6)
    np.testing.assert_allclose(kc["sd"][0, 0].item(), np.std(rows[:, 3] - rows[:, 5], ddof=1), rtol=1e-10)
    ung = dg.covariance(xd[:5])
    np.testing.assert_array_equal(ung["cov"].cpu().numpy(), got["cov"][0].cpu().numpy())
    # a two-block list on one device (group 1 straddles): the merged bound
    two = dg.cross_moments([xd[:7], xd[7:]], chains_per_group=5)
    parts = [M.part(x[:5].reshape(-1, 6).astype(M.LD)),
             M.merge_tolerance(M.part(x[5:7].reshape(-1, 6).astype(M.LD)), M.part(x[7:10].reshape(-1, 6).astype(M.LD))),
             M.part(x[10:].reshape(-1, 6).astype(M.LD))]
    M.check(two["n"].cpu().numpy(), two["mean"].cpu().numpy(), two["m2"].cpu().numpy(), parts, "two blocks, one device")


@pytest.mark.parametrize("thin", [1, 2])
def test_batched_glm_job_end_to_end(thin):
    """G = 3 gaussian GLMs, d = 4, N = 40, 64 chains each: tgt.covariance of the draws in HBM equals numpy.cov of the returned
    host trace within the bound, and both lie within the sampling-error Frobenius bound of tests/test_gpu_pooled.py around
    the exact posterior covariance, sqrt((tr(S)^2 + tr(S^2)) / n_eff) with n_eff = summarize's ess_min of the group.
    That bound is the RMS error of a covariance from n_eff independent draws, and ess_min is the ESS of the MEANS: it is the
    right n_eff for second moments only where the draws are positively autocorrelated (lag-k correlation rho_k of x, about
    rho_k^2 of its squares, so the squares mix faster). Full NUTS trees on a gaussian give antithetic draws whose means have
    ESS ~ n while the squares have about half of it -- measured over 120 seeds the ratio error / bound then centres on 1.3
    for the device result and numpy.cov of the same trace alike. So the job runs one-doubling trees (max_treedepth=1, a
    positively autocorrelated chain, ESS of the means ~ n / 6), where over 40 seeds the ratio lay in 0.35 .. 1.0; seed 19
    gives 0.38 .. 0.56. It is a sanity check on the statistic, with seed and inputs fixed."""
    ms = []
    for g in range(3):
        rng = np.random.default_rng(300 + g)
        X = rng.standard_normal((40, 4))
        ms.append(T.GLM(X, X @ np.array([0.5, -1.0, 0.25 * g, 2.0]) + 0.3 * rng.standard_normal(40), "gaussian"))
    tgt = T.Batched(ms)
    kw = {} if thin == 1 else {"thin": thin}
    trace, _stats, eng = lmc.sample(tgt, tgt.d, chains=192, draws=300, tune=300, random_seed=19, progressbar=False,
                                    return_engine=True, max_treedepth=1, **kw)
    try:
        x = dg.trace_tensor(eng)
        assert tuple(x.shape) == trace.shape
        trace = np.asarray(trace)
        out = tgt.covariance(x)
        ess_min = tgt.summarize(x)["ess_min"].cpu().numpy()
        S = 64 * trace.shape[1]
        assert out["n"].tolist() == [float(S)] * 3
        parts = M.moments(trace, 0, 64)
        M.check(out["n"].cpu().numpy(), out["mean"].cpu().numpy(), out["cov"].cpu().numpy() * (S - 1.0),
                [dict(p, tol_m2=p["tol_m2"] + 2 * M.EPS * np.abs(p["m2"])) for p in parts], "GLM job, thin %d" % thin)
        for g in range(3):
            host = np.cov(trace[64 * g:64 * g + 64].reshape(S, 4), rowvar=False)
            np.testing.assert_allclose(out["cov"][g].cpu().numpy(), host, rtol=1e-10, atol=1e-13)
            sigma = ms[g].posterior_gaussian()[1]
            bound = float(np.sqrt((np.trace(sigma) ** 2 + np.trace(sigma @ sigma)) / ess_min[g]))
            f_dev, f_host = (float(np.linalg.norm(c - sigma)) for c in (out["cov"][g].cpu().numpy(), host))
            print("group %d thin %d: ||cov - Sigma||_F = %.3g (host %.3g), bound %.3g at ess_min %.0f"
                  % (g, thin, f_dev, f_host, bound, ess_min[g]))
            assert f_dev <= bound and f_host <= bound
        k = tgt.contrasts(x, [[1.0, -1.0, 0, 0]])
        d01 = trace[:64, :, 0] - trace[:64, :, 1]
        np.testing.assert_allclose(k["sd"][0, 0].item(), d01.std(ddof=1), rtol=1e-10)
        one = ms[0].covariance(x[:64])                     # GLM.covariance: the ungrouped form
        np.testing.assert_allclose(one["cov"].cpu().numpy(), out["cov"][0].cpu().numpy(), rtol=1e-12, atol=1e-15)
    finally:
        eng.close()


def test_two_blocks_on_two_devices_equal_the_one_device_result():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    x = _job(3, 5, 61, 70)
    xd = torch.from_numpy(x).cuda()
    two = dg.cross_moments([xd[:7].contiguous(), xd[7:].to("cuda:1")], chains_per_group=5)
    assert two["m2"].device == xd.device
    p = lambda a, b: M.part(x[a:b].reshape(-1, 70).astype(M.LD))
    parts = [p(0, 5), M.merge_tolerance(p(5, 7), p(7, 10)), p(10, 15)]
    M.check(two["n"].cpu().numpy(), two["mean"].cpu().numpy(), two["m2"].cpu().numpy(), parts, "two devices")
    one = dg.cross_moments(xd, chains_per_group=5)
    for g in (0, 2):      # the groups inside one block come through bit for bit
        np.testing.assert_array_equal(two["m2"][g].cpu().numpy(), one["m2"][g].cpu().numpy())
