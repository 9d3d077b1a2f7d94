"""-m gpu: lmc_diag_threshold_counts (csrc/lmc_threshold.hip) against the numpy model of one count call
(tests/_threshold_model.py), every count exactly, and prob / rope / direction / exceedance above it against the same calls with
the model injected. Each shape is the smallest that reaches one way the kernel can go wrong."""
import ctypes

import numpy as np
import pytest
import torch

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi, predictive
from littlemcmc_amd import diagnostics as dg
from littlemcmc_amd import targets as T
from oracle import diagnostics_oracle as odg
from tests import _threshold_model as M
from tests.test_diagnostics_cpu import ar1_chains

pytestmark = pytest.mark.gpu

RHOS = (0.2, 0.97, -0.5)
FFT = odg.torch_chain_stats
SENTINEL = -7


def _job(groups, per, n, d, seed=41):
    return np.concatenate([ar1_chains(per, n, d, RHOS[g % 3], seed + g) for g in range(groups)])


def _thresholds(x, per, K, seed=9):
    """[G, K, d]: half of them draws of the group itself (ties), half values between the draws."""
    G, d = x.shape[0] // per, x.shape[2]
    rng = np.random.default_rng(seed)
    pool = x.reshape(G, -1, d)
    pick = rng.integers(0, pool.shape[1], (G, K, d))
    thr = np.take_along_axis(pool, pick, axis=1)
    thr[:, 1::2] += 0.01 * rng.standard_normal(thr[:, 1::2].shape)
    return np.ascontiguousarray(thr)


@pytest.fixture(scope="module")
def ragged():
    """(G, per, n, d) = (3, 5, 61, 70): ragged n; the second 64-lane slab has 6 live lanes."""
    x = _job(3, 5, 61, 70)
    return x, torch.from_numpy(x).cuda()


def _raw(xd, t0, n, first_chain, per, thr, stride=None):
    """The C entry itself on a contiguous device tensor xd[chains, stride, d]; thr: numpy [touched, K, d]; the output is
    pre-filled with a sentinel (the entry zeroes its result)."""
    c, rows, d = xd.shape
    touched = M.touched(first_chain, c, per)[1]
    K = thr.shape[1]
    assert thr.shape == (touched, K, d)
    td = torch.from_numpy(np.ascontiguousarray(thr)).to(xd.device)
    out = torch.full((touched, 2 * K + 1, d), SENTINEL, dtype=torch.int64, device=xd.device)
    stream = torch.cuda.current_stream(xd.device).cuda_stream
    rc = _abi.load().lmc_diag_threshold_counts(ctypes.c_void_p(xd.data_ptr()), c, rows if stride is None else stride, d, t0, n,
                                               first_chain, per, K, ctypes.c_void_p(td.data_ptr()),
                                               ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream))
    assert rc == _abi.OK
    return out.cpu().numpy()


@pytest.mark.parametrize("K", [1, 3, 16])
def test_raw_counts_equal_the_model(ragged, K):
    x, xd = ragged
    thr = _thresholds(x, 5, K)
    got = _raw(xd, 0, 61, 0, 5, thr)
    np.testing.assert_array_equal(got, M.counts(x, 0, 61, 0, 5, thr))
    assert got[:, 0::2].sum() > 0 and got[:, 1:2 * K:2].sum() > 0 and not got[:, 2 * K].any()


def test_a_view_into_longer_chains(ragged):
    """t0 = 3, n = 37 of draws_stride = 61."""
    x, xd = ragged
    thr = _thresholds(x[:, 3:40], 5, 3)
    np.testing.assert_array_equal(_raw(xd, 3, 37, 0, 5, thr), M.counts(x, 3, 37, 0, 5, thr))


def test_a_block_that_touches_three_groups_two_of_them_partly(ragged):
    """Chains 3 .. 11 of the job (first_chain = 3, per = 5, chains = 9): groups 0 and 2 partly, group 1 whole. With the
    complementary blocks the counts add up to the whole job's."""
    x, xd = ragged
    thr = _thresholds(x, 5, 3)
    whole = _raw(xd, 0, 61, 0, 5, thr)
    mid = _raw(xd[3:12].contiguous(), 0, 61, 3, 5, thr)
    assert mid.shape[0] == 3
    np.testing.assert_array_equal(mid, M.counts(x[3:12], 0, 61, 3, 5, thr))
    total = mid.copy()
    total[:1] += _raw(xd[:3].contiguous(), 0, 61, 0, 5, thr[:1])
    total[2:] += _raw(xd[12:].contiguous(), 0, 61, 12, 5, thr[2:])
    np.testing.assert_array_equal(total, whole)


@pytest.mark.parametrize("d", [1, 16, 17, 32, 33, 64, 65, 130])
def test_dimension_counts_around_the_slab_widths(d):
    """d <= 16, <= 32 and above use slabs of 16, 32 and 64 columns; 65 and 130 need a second and third slab."""
    x = _job(2, 3, 45, d, seed=5)
    thr = _thresholds(x, 3, 6)
    np.testing.assert_array_equal(_raw(torch.from_numpy(x).cuda(), 0, 45, 0, 3, thr), M.counts(x, 0, 45, 0, 3, thr))


def test_more_groups_and_more_chains_than_the_workgroup_budget():
    """600 groups of 3 chains: one workgroup per group loops over the group's chains; 2 groups of 700 chains: 512 chain blocks
    per group, each looping over one or two chains."""
    for groups, per, n, d in ((600, 3, 9, 2), (2, 700, 5, 3)):
        x = _job(groups, per, n, d, seed=2)
        thr = _thresholds(x, per, 2)
        got = _raw(torch.from_numpy(x).cuda(), 0, n, 0, per, thr)
        np.testing.assert_array_equal(got, M.counts(x, 0, n, 0, per, thr))


def test_one_chain_with_one_draw():
    x = np.array([[[0.5, -1.0, 2.0]]])
    thr = np.array([[[0.5, 0.0, 1.0], [1.0, -1.0, 2.5]]])
    got = _raw(torch.from_numpy(x).cuda(), 0, 1, 0, 1, thr)
    np.testing.assert_array_equal(got, M.counts(x, 0, 1, 0, 1, thr))
    assert got[0].tolist() == [[0, 1, 0], [1, 0, 0], [1, 0, 1], [0, 1, 0], [0, 0, 0]]


def test_a_count_above_65535():
    """2 x 40 000 draws of one constant, d = 1, thresholds below, at and above it."""
    x = np.full((2, 40000, 1), 1.25)
    thr = np.array([1.0, 1.25, 1.5]).reshape(1, 3, 1)
    got = _raw(torch.from_numpy(x).cuda(), 0, 40000, 0, 2, thr)
    assert got[0, :, 0].tolist() == [0, 0, 0, 80000, 80000, 0, 0]


def test_hostile_values():
    """(2, 40, 3): +-0, +-inf, +-denormal, +-max, +-NaN among ordinary draws; a constant column; a two-valued column."""
    tiny, big = 5e-324, np.finfo(np.float64).max
    rng = np.random.default_rng(8)
    x = rng.standard_normal((2, 40, 3))
    special = [0.0, -0.0, np.inf, -np.inf, tiny, -tiny, big, -big, np.nan, -np.nan]
    x[0, 5:15, 0] = special
    x[1, 20:30, 0] = special[::-1]
    x[:, :, 1] = 1.25
    x[:, :, 2] = np.where(rng.random((2, 40)) < 0.4, 1.0, 2.0)
    thr = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, tiny, 1.25, 1.5])
    thr = np.ascontiguousarray(np.broadcast_to(thr.reshape(1, 8, 1), (1, 8, 3)))
    got = _raw(torch.from_numpy(x).cuda(), 0, 40, 0, 2, thr)
    np.testing.assert_array_equal(got, M.counts(x, 0, 40, 0, 2, thr))
    assert got[0, 16].tolist() == [4, 0, 0]                                 # the NaN draws, either sign
    assert got[0, 0, 0] == got[0, 2, 0] and got[0, 1, 0] == got[0, 3, 0] == 4   # -0.0 == +0.0: as thresholds and as draws
    assert got[0, 8:10].tolist() == [[0, 0, 0], [0, 0, 0]]                  # a NaN threshold counts 0 and 0
    assert got[0, 4].tolist() == [74, 80, 80] and got[0, 5].tolist() == [2, 0, 0]   # below +inf: all but +inf and NaN
    assert got[0, 6].tolist() == [0, 0, 0] and got[0, 7].tolist() == [2, 0, 0]      # nothing lies below -inf
    assert got[0, 12:14, 1].tolist() == [0, 80] and got[0, 14, 2] == (x[:, :, 2] == 1.0).sum()


def test_thresholds_at_exact_order_statistics(ragged):
    """For v = the r-th smallest draw: less <= r < less + equal -- the count inverts the select."""
    x, xd = ragged
    S = 5 * 61
    ranks = [0, 1, S // 3, S // 2, S - 2, S - 1]
    v = dg.order_statistics(xd, ranks, chains_per_group=5)
    tc = dg.threshold_counts(xd, v, chains_per_group=5)
    r = torch.tensor(ranks, device=xd.device).reshape(1, -1, 1)
    assert bool(((tc["less"] <= r) & (r < tc["less"] + tc["equal"])).all()) and tc["n"] == S
    np.testing.assert_array_equal(v.cpu().numpy(), np.sort(x.reshape(3, S, 70), axis=1)[:, ranks])


def test_host_functions_equal_the_injected_model():
    """(3, 5, 200, 6), rounded to a quarter so that ties occur."""
    x = np.round(_job(3, 5, 200, 6) * 4.0) / 4.0
    xt, xd = torch.from_numpy(x), torch.from_numpy(x).cuda()
    kd, kc = dict(chains_per_group=5), dict(chains_per_group=5, count_fn=M.count_fn)
    thr = np.round(np.random.default_rng(1).standard_normal((17, 6)) * 4.0) / 4.0
    dev, cpu = dg.prob(xd, thr, mcse=True, **kd), dg.prob(xt, thr, mcse=True, stats_fn=FFT, **kc)
    for k in ("p_less", "p_equal", "p_greater", "n_nan"):
        assert dev[k].is_cuda
        np.testing.assert_array_equal(dev[k].cpu().numpy(), cpu[k].numpy(), err_msg=k)
    assert dev["n"] == cpu["n"] == 1000 and float(cpu["p_equal"].sum()) > 0
    np.testing.assert_allclose(dev["ess"].cpu().numpy(), cpu["ess"].numpy(), rtol=1e-7)
    for name, args in (("rope", (-0.5, 0.75)), ("direction", ())):
        a, b = getattr(dg, name)(xd, *args, **kd), getattr(dg, name)(xt, *args, **kc)
        for k, v in b.items():
            if torch.is_tensor(v):
                np.testing.assert_array_equal(a[k].cpu().numpy(), v.numpy(), err_msg=name + " " + k)
    b = T.Batched([T.AR1(6, rho=r) for r in RHOS])
    two = b.prob([xd[:7], xd[7:]], thr)                                     # group 1 straddles the two blocks
    for k in ("p_less", "p_equal", "p_greater"):
        np.testing.assert_array_equal(two[k].cpu().numpy(), cpu[k].numpy(), err_msg=k)
    one = dg.prob(xd[5:10], thr[:2])                                        # ungrouped: no leading axis
    assert tuple(one["p_less"].shape) == (2, 6) and torch.equal(one["p_less"], dev["p_less"][1, :2])


def test_exceedance_counts_the_devices_own_linear_predictor():
    """A bernoulli Batched of 3 members at N_new = 70 (two observation blocks, 58 padding columns)."""
    rng = np.random.default_rng(40)
    N, d, per, n = 50, 4, 3, 41
    ms = [T.GLM(rng.standard_normal((N, d)) / 2.0, (rng.random(N) < 0.5).astype(np.float64), "bernoulli") for _ in range(3)]
    tgt = T.Batched(ms)
    Xn = [rng.standard_normal((70, d)) for _ in range(3)]
    x = torch.from_numpy(rng.standard_normal((3 * per, n, d))).cuda()
    eta = predictive.linear_predictor(x, tgt, Xn)[0].cpu().numpy().reshape(3, per * n, 128)[:, :, :70]
    S = per * n
    t_eta = np.array([-0.5, 0.0, 1.0])
    out = tgt.exceedance(x, Xn, thresholds=t_eta)
    assert tuple(out["p_less"].shape) == (3, 3, 70) and out["n"] == S and not bool(out["n_nan"].any())
    np.testing.assert_array_equal(out["p_less"].cpu().numpy(), (eta[:, :, None, :] < t_eta[:, None]).sum(axis=1) / S)
    np.testing.assert_array_equal(out["p_greater"].cpu().numpy(), (eta[:, :, None, :] > t_eta[:, None]).sum(axis=1) / S)
    mu = 1 / (1 + np.exp(-eta))
    t_mu = np.array([0.25, 0.5])
    om = tgt.exceedance(x, Xn, thresholds=t_mu, scale="mu")
    np.testing.assert_array_equal(om["p_less"].cpu().numpy(), (mu[:, :, None, :] < t_mu[:, None]).sum(axis=1) / S)
    np.testing.assert_array_equal(om["p_greater"].cpu().numpy(), (mu[:, :, None, :] > t_mu[:, None]).sum(axis=1) / S)
    chunked = tgt.exceedance(x, Xn, thresholds=t_mu, scale="mu", scratch_bytes=3 * per * n * 64 * 8)   # one block per chunk
    for k, v in om.items():
        if torch.is_tensor(v):
            assert torch.equal(v, chunked[k]), k
    own = ms[0].exceedance(x[:per], thresholds=0.5, scale="mu")             # GLM.exceedance at the training design
    assert tuple(own["p_less"].shape) == (1, 1, N)
    with pytest.raises(ValueError, match="scratch_bytes"):
        tgt.exceedance(x, Xn, thresholds=0.0, scratch_bytes=1000)
    with pytest.raises(ValueError, match="scale"):
        tgt.exceedance(x, Xn, thresholds=0.0, scale="y")


@pytest.mark.parametrize("thin", [1, 2])
def test_batched_glm_job_end_to_end(thin):
    ms = []
    for g in range(3):
        rng = np.random.default_rng(300 + g)
        X = rng.standard_normal((40, 3))
        ms.append(T.GLM(X, X @ np.array([0.5, -1.0, 0.25 * g]) + 0.3 * rng.standard_normal(40), "gaussian"))
    tgt = T.Batched(ms)
    kw = {} if thin == 1 else {"thin": thin}
    trace, _stats, eng = lmc.sample(tgt, tgt.d, chains=12, draws=60, tune=60, random_seed=5, progressbar=False,
                                    return_engine=True, **kw)
    try:
        x = dg.trace_tensor(eng)
        assert tuple(x.shape) == trace.shape
        trace = np.asarray(trace)
        S = 4 * trace.shape[1]
        pool = trace.reshape(3, S, 1, 3)
        c = np.stack([np.median(trace.reshape(3, S, 3), axis=1), np.zeros((3, 3)), pool[:, 7, 0]], axis=1)   # [G, K = 3, d]
        out = tgt.prob(x, c)
        assert out["n"] == S
        np.testing.assert_array_equal(out["p_less"].cpu().numpy(), (pool < c[:, None]).sum(axis=1) / S)
        np.testing.assert_array_equal(out["p_equal"].cpu().numpy(), (pool == c[:, None]).sum(axis=1) / S)
        np.testing.assert_array_equal(out["p_greater"].cpu().numpy(), (pool > c[:, None]).sum(axis=1) / S)
        assert float(out["p_equal"][:, 2].min()) > 0
        r = tgt.rope(x, -0.1, 0.1)
        np.testing.assert_array_equal(r["inside"].cpu().numpy(), (np.abs(pool[:, :, 0]) <= 0.1).sum(axis=1) / S)
        one = ms[0].direction(x[:4])                                        # GLM.direction: the ungrouped form
        assert torch.equal(one["pd"], tgt.direction(x)["pd"][0])
    finally:
        eng.close()


def test_two_blocks_on_two_devices_equal_the_one_device_result():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    x = _job(3, 5, 61, 70)
    xd = torch.from_numpy(x).cuda()
    thr = _thresholds(x, 5, 5)
    one = dg.threshold_counts(xd, thr, chains_per_group=5)
    two = dg.threshold_counts([xd[:7].contiguous(), xd[7:].to("cuda:1")], thr, chains_per_group=5)
    for k in ("less", "equal", "nan"):
        assert two[k].device == one[k].device
        np.testing.assert_array_equal(two[k].cpu().numpy(), one[k].cpu().numpy(), err_msg=k)


def test_the_library_exports_the_entry_and_refuses_bad_arguments():
    lib = _abi.load()
    assert hasattr(lib, "lmc_diag_threshold_counts")
    xd = torch.zeros((2, 5, 3), dtype=torch.float64, device="cuda")
    td = torch.zeros((1, 17, 3), dtype=torch.float64, device="cuda")
    out = torch.full((1, 35, 3), SENTINEL, dtype=torch.int64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    for k, counts in ((0, p(out)), (17, p(out)), (2, None)):
        assert lib.lmc_diag_threshold_counts(p(xd), 2, 5, 3, 0, 5, 0, 2, k, p(td), counts, None) == 1   # LMC_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())                                    # refused before anything was enqueued
    assert lib.lmc_diag_threshold_counts(p(xd), 2, 5, 3, 0, 5, 0, 2, 16, p(td), p(out), None) == _abi.OK
    torch.cuda.synchronize()
    assert out[0, :33].cpu().numpy().reshape(-1, 3)[1:32:2].tolist() == [[10, 10, 10]] * 16 and int(out[0, 32].sum()) == 0
