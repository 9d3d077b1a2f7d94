"""-m gpu: lmc_select_digit_counts (csrc/lmc_select.hip) against the numpy model of one count call (tests/_select_model.py),
exactly, and the quantiles / intervals / tail-ESS above it against the same calls with the model injected. Each shape is the
smallest that reaches one way the kernel can go wrong."""
import ctypes

import numpy as np
import pytest
import torch

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi
from littlemcmc_amd import diagnostics as dg
from littlemcmc_amd import targets as T
from oracle import diagnostics_oracle as odg
from tests import _select_model as M
from tests.test_diagnostics_cpu import ar1_chains

pytestmark = pytest.mark.gpu

RHOS = (0.2, 0.97, -0.5)
FFT = odg.torch_chain_stats


def _job(groups, per, n, d, seed=41):
    return np.concatenate([ar1_chains(per, n, d, RHOS[g % 3], seed + g) for g in range(groups)])


@pytest.fixture(scope="module")
def ragged():
    """(G, per, n, d) = (3, 5, 61, 70): ragged n; the second 64-lane slab has 6 live lanes."""
    x = _job(3, 5, 61, 70)
    return x, torch.from_numpy(x).cuda()


def _raw(xd, t0, n, first_chain, per, shift, prefix=None, stride=None):
    """The C entry itself on a contiguous device tensor xd[chains, stride, d]; prefix: numpy uint64 [touched, n_ranks, d]."""
    c, rows, d = xd.shape
    touched = M.touched(first_chain, c, per)[1]
    n_ranks = 1 if prefix is None else prefix.shape[1]
    pd = None if prefix is None else torch.from_numpy(np.ascontiguousarray(prefix).view(np.int64)).to(xd.device)
    out = torch.full((touched, n_ranks, 256, d), -7, dtype=torch.int64, device=xd.device)
    stream = torch.cuda.current_stream(xd.device).cuda_stream
    rc = _abi.load().lmc_select_digit_counts(ctypes.c_void_p(xd.data_ptr()), c, rows if stride is None else stride, d, t0, n,
                                             first_chain, per, shift, n_ranks,
                                             None if pd is None else ctypes.c_void_p(pd.data_ptr()),
                                             ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream))
    assert rc == _abi.OK
    return out.cpu().numpy()


def _prefixes(x, per, ranks):
    """[G, len(ranks), d] uint64: the keys of the ``ranks``-th smallest draws of every (group, dimension) -- a prefix at every
    shift (the digits below the shift are not compared)."""
    G, d = x.shape[0] // per, x.shape[2]
    keys = np.sort(M.key(x).reshape(G, -1, d), axis=1)
    return np.ascontiguousarray(keys[:, ranks, :])


def test_raw_counts_at_every_kind_of_shift(ragged):
    x, xd = ragged
    n, S = 61, 5 * 61
    np.testing.assert_array_equal(_raw(xd, 0, n, 0, 5, 56), M.digit_counts(x, 0, n, 0, 5, 56))
    pf = _prefixes(x, 5, [0, S // 2, S - 1])
    for shift in (40, 0):
        got = _raw(xd, 0, n, 0, 5, shift, pf)
        np.testing.assert_array_equal(got, M.digit_counts(x, 0, n, 0, 5, shift, pf))
        assert got.sum() > 0
    # a slot whose prefix matches no draw: all-zero counts, the other slots unchanged
    none = pf.copy()
    none[:, 1, :] = M.key(np.array([1e300]))[0]
    got = _raw(xd, 0, n, 0, 5, 0, none)
    np.testing.assert_array_equal(got, M.digit_counts(x, 0, n, 0, 5, 0, none))
    assert not got[:, 1].any() and got[:, 0].any() and got[:, 2].any()
    # 16 rank slots: every slot tile of both slab widths' blocks
    pf16 = _prefixes(x, 5, list(range(0, S, S // 16))[:16])
    for shift in (48, 8):
        np.testing.assert_array_equal(_raw(xd, 0, n, 0, 5, shift, pf16), M.digit_counts(x, 0, n, 0, 5, shift, pf16))


def test_a_view_into_longer_chains(ragged):
    """t0 = 3, n = 37 of draws_stride = 61."""
    x, xd = ragged
    pf = _prefixes(x[:, 3:40], 5, [0, 90, 184])
    np.testing.assert_array_equal(_raw(xd, 3, 37, 0, 5, 56), M.digit_counts(x, 3, 37, 0, 5, 56))
    np.testing.assert_array_equal(_raw(xd, 3, 37, 0, 5, 16, pf), M.digit_counts(x, 3, 37, 0, 5, 16, pf))


def test_a_block_that_touches_three_groups_two_of_them_partly(ragged):
    """Chains 3 .. 11 of the job (first_chain = 3, per = 5, chains = 9): groups 0 and 2 partly, group 1 whole. With the
    complementary blocks the counts add up to the whole job's."""
    x, xd = ragged
    pf = _prefixes(x, 5, [7, 150])
    for shift, p in ((56, None), (32, pf)):
        whole = _raw(xd, 0, 61, 0, 5, shift, p)
        mid = _raw(xd[3:12].contiguous(), 0, 61, 3, 5, shift, p)
        assert mid.shape[0] == 3
        np.testing.assert_array_equal(mid, M.digit_counts(x[3:12], 0, 61, 3, 5, shift, p))
        head = _raw(xd[:3].contiguous(), 0, 61, 0, 5, shift, None if p is None else p[:1])
        tail = _raw(xd[12:].contiguous(), 0, 61, 12, 5, shift, None if p is None else p[2:])
        total = mid.copy()
        total[:1] += head
        total[2:] += tail
        np.testing.assert_array_equal(total, whole)


@pytest.mark.parametrize("d", [1, 16, 17, 32, 33, 64, 65, 130])
def test_dimension_counts_around_the_table_widths(d):
    """d <= 16, <= 32 and above use tables of 16, 32 and 64 columns; 65 and 130 need a second and third slab."""
    x = _job(2, 3, 45, d, seed=5)
    xd = torch.from_numpy(x).cuda()
    S = 3 * 45
    pf = _prefixes(x, 3, [0, 1, S // 3, S // 2, S - 2, S - 1])
    np.testing.assert_array_equal(_raw(xd, 0, 45, 0, 3, 56), M.digit_counts(x, 0, 45, 0, 3, 56))
    np.testing.assert_array_equal(_raw(xd, 0, 45, 0, 3, 24, pf), M.digit_counts(x, 0, 45, 0, 3, 24, pf))


def test_more_groups_than_the_workgroup_budget():
    """600 groups of 3 chains: one workgroup per group loops over the group's chains, and the grid exceeds the budget of 512;
    2 groups of 700 chains: 256 chain blocks per group, each looping over two or three chains."""
    for groups, per, n, d in ((600, 3, 9, 2), (2, 700, 5, 3)):
        x = ar1_chains(groups * per, n, d, 0.3, 9)
        xd = torch.from_numpy(x).cuda()
        pf = _prefixes(x, per, [0, per * n // 2, per * n - 1])
        np.testing.assert_array_equal(_raw(xd, 0, n, 0, per, 56), M.digit_counts(x, 0, n, 0, per, 56))
        np.testing.assert_array_equal(_raw(xd, 0, n, 0, per, 8, pf), M.digit_counts(x, 0, n, 0, per, 8, pf))


def test_one_chain_with_one_draw():
    x = np.array([[[-3.5, 0.0, 2.0]]])
    xd = torch.from_numpy(x).cuda()
    np.testing.assert_array_equal(_raw(xd, 0, 1, 0, 1, 56), M.digit_counts(x, 0, 1, 0, 1, 56))
    got = dg.order_statistics(xd, [0, 0])
    np.testing.assert_array_equal(got.cpu().numpy(), np.array([[-3.5, 0.0, 2.0]] * 2))


def test_hostile_draws_every_rank():
    """(2, 40, 3): +-0, +-inf, +-denormal, +-max and +-NaN; a constant column; a column of two distinct values."""
    rng = np.random.default_rng(2)
    tiny, big = 5e-324, np.finfo(np.float64).max
    col0 = rng.standard_normal(80)
    col0[:12] = [0.0, -0.0, np.inf, -np.inf, tiny, -tiny, big, -big, np.nan, -np.nan, 0.0, -0.0]
    x = np.stack([rng.permutation(col0), np.full(80, 1.25), rng.permutation(np.repeat([-2.0, 3.0], [33, 47]))], axis=1)
    x = np.ascontiguousarray(x.reshape(2, 40, 3))
    got = dg.order_statistics(torch.from_numpy(x).cuda(), list(range(80))).cpu().numpy()
    want = np.stack([M.key_sorted(x[:, :, j]) for j in range(3)], axis=1)
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))   # the bits: NaN signs and zero signs included
    q = dg.quantiles(torch.from_numpy(x).cuda(), [0.5])
    assert np.isnan(q["quantiles"][0, 0].item()) and q["quantiles"][0, 1].item() == 1.25 and q["quantiles"][0, 2].item() == 3.0


def test_a_bin_of_more_than_65535_draws():
    """2 chains x 40 000 draws of one constant, d = 1: one bin holds 80 000."""
    xd = torch.full((2, 40000, 1), 0.75, dtype=torch.float64, device="cuda")
    k = int(M.key(np.array([0.75]))[0])
    got = _raw(xd, 0, 40000, 0, 2, 56)
    assert got.sum() == 80000 and got[0, 0, k >> 56, 0] == 80000
    pf = np.full((1, 2, 1), k, dtype=np.uint64)
    got = _raw(xd, 0, 40000, 0, 2, 0, pf)
    assert got[0, 0, k & 255, 0] == 80000 and got[0, 1, k & 255, 0] == 80000 and got.sum() == 160000
    assert dg.order_statistics(xd, [0, 65536, 79999]).cpu().numpy().tolist() == [[0.75]] * 3


def test_host_functions_on_the_device_equal_the_injected_model():
    """(G, per, n, d) = (3, 5, 200, 6): order statistics exact, ess_tail to the project's rtol for ESS."""
    x = _job(3, 5, 200, 6)
    xt, xd = torch.from_numpy(x), torch.from_numpy(x).cuda()
    probs = [0.05, 0.5, 0.95]
    got, want = dg.quantiles(xd, probs, chains_per_group=5), dg.quantiles(xt, probs, chains_per_group=5, count_fn=M.count_fn)
    for k in ("quantiles", "min", "max"):
        np.testing.assert_array_equal(got[k].cpu().numpy(), want[k].numpy(), err_msg=k)
    srt = np.sort(x.reshape(3, 1000, 6), axis=1)
    ranks = [0, 49, 50, 499, 500, 949, 950, 999]
    np.testing.assert_array_equal(dg.order_statistics(xd, ranks, chains_per_group=5).cpu().numpy(), srt[:, ranks])
    iv, ivw = dg.intervals(xd, 0.9, chains_per_group=5), dg.intervals(xt, 0.9, chains_per_group=5, count_fn=M.count_fn)
    for k in ("lower", "median", "upper"):
        np.testing.assert_array_equal(iv[k].cpu().numpy(), ivw[k].numpy(), err_msg=k)
    b = T.Batched([T.AR1(6, rho=r) for r in RHOS])
    np.testing.assert_array_equal(b.quantiles(xd, probs)["quantiles"].cpu().numpy(), want["quantiles"].numpy())
    # a two-block list on one device (group 1 straddles) and a scratch that forces one group per chunk: the same bits
    np.testing.assert_array_equal(b.quantiles([xd[:7], xd[7:]], probs)["quantiles"].cpu().numpy(), want["quantiles"].numpy())
    np.testing.assert_array_equal(dg.quantiles(xd, probs, chains_per_group=5, scratch_bytes=256 * 6 * 8 * 8)["quantiles"].cpu().numpy(),
                                  want["quantiles"].numpy())
    te, tew = b.tail_ess(xd), dg.tail_ess(xt, chains_per_group=5, count_fn=M.count_fn, stats_fn=FFT)
    np.testing.assert_allclose(te["ess_tail"].cpu().numpy(), tew["ess_tail"].numpy(), rtol=1e-7)
    np.testing.assert_allclose(te["ess_tail_min"].cpu().numpy(), tew["ess_tail_min"].numpy(), rtol=1e-7)
    ung, ungw = dg.tail_ess(xd[:5]), dg.tail_ess(xt[:5], count_fn=M.count_fn, stats_fn=FFT)
    np.testing.assert_allclose(ung["ess_tail"].cpu().numpy(), ungw["ess_tail"].numpy(), rtol=1e-7)


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
        probs = [0.05, 0.5, 0.95]
        out = tgt.quantiles(x, probs)
        S = 4 * trace.shape[1]
        assert out["n"] == S
        srt = np.sort(trace.reshape(3, S, 3), axis=1)
        ranks = [0, S // 2, S - 1]
        np.testing.assert_array_equal(dg.order_statistics(x, ranks, chains_per_group=4).cpu().numpy(), srt[:, ranks])
        for k, p in enumerate(probs):
            want = np.stack([[M.quantile_formula(srt[g, :, j], p) for j in range(3)] for g in range(3)])
            np.testing.assert_array_equal(out["quantiles"][:, k].cpu().numpy(), want)
        iv = tgt.intervals(x, 0.9)
        np.testing.assert_array_equal(iv["median"].cpu().numpy(), out["quantiles"][:, 1].cpu().numpy())
    finally:
        eng.close()


def test_two_blocks_on_two_devices_equal_the_one_device_result():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    x = _job(3, 5, 61, 70)
    xd = torch.from_numpy(x).cuda()
    probs = [0.05, 0.5, 0.95]
    one = dg.quantiles(xd, probs, chains_per_group=5)
    two = dg.quantiles([xd[:7].contiguous(), xd[7:].to("cuda:1")], probs, chains_per_group=5)
    for k in ("quantiles", "min", "max"):
        assert two[k].device == one[k].device
        np.testing.assert_array_equal(two[k].cpu().numpy(), one[k].cpu().numpy(), err_msg=k)
    np.testing.assert_array_equal(dg.quantiles([xd[:7].contiguous(), xd[7:].to("cuda:1")], probs)["quantiles"].cpu().numpy(),
                                  dg.quantiles(xd, probs)["quantiles"].cpu().numpy())
