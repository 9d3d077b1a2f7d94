"""-m gpu: lmc_diag_chain_stats_grouped (csrc/lmc_diag.hip) -- R-hat / ESS of every posterior of a targets.Batched job from
one pass over the draws in HBM -- against the numpy restatement applied to each group's chains. Each shape is the smallest
that reaches one way the group decomposition can go wrong."""
import ctypes

import numpy as np
import pytest
import torch

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi
from littlemcmc_amd import diagnostics as dg
from oracle import diagnostics_oracle as odg
from tests.test_diagnostics_cpu import ar1_chains

pytestmark = pytest.mark.gpu

RHOS = (0.2, 0.97, -0.5)


def _job(groups, per, n, d, seed=41):
    """``groups`` posteriors of ``per`` AR(1) chains; the rho cycles through RHOS so that groups need different lag passes
    (thousands of groups: one rho, generated in one go)."""
    if groups > 8:
        return ar1_chains(groups * per, n, d, RHOS[0], seed)
    return np.concatenate([ar1_chains(per, n, d, RHOS[g % 3], seed + g) for g in range(groups)])


@pytest.fixture(scope="module")
def ragged():
    """(G, per, n, d) = (3, 5, 61, 70): ragged n, two 64-lane slabs, one rho per group."""
    x = _job(3, 5, 61, 70)
    return x, torch.from_numpy(x).cuda()


def _raw(xd, t0, n, lag0, first_chain, per, entry="lmc_diag_chain_stats_grouped"):
    """The C entry itself on a contiguous device tensor."""
    c, rows, d = xd.shape
    grouped = entry.endswith("grouped")
    touched = (first_chain + c - 1) // per - first_chain // per + 1 if grouped else 1
    out = torch.full((touched, 19, d), float("nan"), dtype=torch.float64, device=xd.device)
    args = (ctypes.c_void_p(xd.data_ptr()), c, rows, d, t0, n, lag0) + ((first_chain, per) if grouped else ())
    stream = torch.cuda.current_stream(xd.device).cuda_stream
    assert getattr(_abi.load(), entry)(*args, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream)) == _abi.OK
    return out


def _direct_block(sub, lag0):
    """[19, d] by direct sums over the chains of sub[chains, m, d] (the statement in include/lmc_hip.h)."""
    m = sub.shape[1]
    mean = sub.mean(axis=1)
    cen = sub - mean[:, None, :]
    out = np.zeros((19, sub.shape[2]))
    out[0], out[1] = mean.sum(axis=0), (mean ** 2).sum(axis=0)
    if lag0 == 0:
        out[2] = (cen ** 2).sum(axis=(0, 1)) / (m - 1)
    for k in range(16):
        lag = lag0 + k
        if lag < m:
            out[3 + k] = (cen[:, :m - lag] * cen[:, lag:]).sum(axis=(0, 1)) / m
    return out


def _assert_groups_equal_oracle(x, got, per, split=True, rank_normalized=False):
    rtol_rhat, rtol_ess = (1e-8, 1e-6) if rank_normalized else (1e-9, 1e-7)
    rhat, ess = got["rhat"].cpu().numpy(), got["ess"].cpu().numpy()
    groups = x.shape[0] // per
    assert got["groups"] == groups and rhat.shape == ess.shape == (groups, x.shape[2])
    for g in range(groups):
        want_rhat, want_ess = odg.rhat_ess(x[g * per:(g + 1) * per], do_split=split, rank_normalized=rank_normalized)
        np.testing.assert_allclose(rhat[g], want_rhat, rtol=rtol_rhat, err_msg="group %d" % g)
        np.testing.assert_allclose(ess[g], want_ess, rtol=rtol_ess, err_msg="group %d" % g)
    np.testing.assert_array_equal(got["rhat_max"].cpu().numpy(), rhat.max(axis=1))
    np.testing.assert_array_equal(got["ess_min"].cpu().numpy(), ess.min(axis=1))


@pytest.mark.parametrize("split", [True, False])
def test_ragged_groups_with_different_lag_passes(ragged, split):
    x, xd = ragged
    got = dg.summarize(xd, split=split, chains_per_group=5)
    _assert_groups_equal_oracle(x, got, 5, split=split)
    alone = [dg.summarize(xd[g * 5:(g + 1) * 5], split=split)["lag_passes"] for g in range(3)]
    assert got["lag_passes"] == max(alone) > min(alone)


def test_ragged_groups_rank_normalised(ragged):
    x, xd = ragged
    _assert_groups_equal_oracle(x, dg.summarize(xd, chains_per_group=5, rank_normalized=True), 5, rank_normalized=True)


@pytest.mark.parametrize("split", [True, False])
def test_one_chain_per_group(split):
    x = _job(4, 1, 40, 3)
    _assert_groups_equal_oracle(x, dg.summarize(torch.from_numpy(x).cuda(), split=split, chains_per_group=1), 1, split=split)


def test_more_chains_than_chain_blocks_per_group():
    """2 groups share the ~4096 wavefronts: 2048 chain blocks each for 2051 chains, so the strided chain loop runs."""
    x = _job(2, 2051, 20, 3)
    _assert_groups_equal_oracle(x, dg.summarize(torch.from_numpy(x).cuda(), chains_per_group=2051), 2051)


def test_more_groups_than_the_wavefront_budget():
    """5000 groups: one chain block per group, and the grid is larger than the budget."""
    x = _job(5000, 2, 16, 2)
    _assert_groups_equal_oracle(x, dg.summarize(torch.from_numpy(x).cuda(), chains_per_group=2), 2)


def test_a_block_that_starts_inside_a_group(ragged):
    """x[7:] with first_chain = 7 touches groups 1 and 2; the first row holds the sums over chains 7-9 only. The list
    [x[:7], x[7:]] adds the two parts of group 1."""
    x, xd = ragged
    n = x.shape[1]
    blk = _raw(xd[7:].contiguous(), 0, n, 0, 7, 5).cpu().numpy()
    assert blk.shape == (2, 19, 70)
    np.testing.assert_allclose(blk[0], _direct_block(x[7:10], 0), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(blk[1], _direct_block(x[10:15], 0), rtol=1e-10, atol=1e-12)
    head = _raw(xd[:7].contiguous(), 0, n, 0, 0, 5).cpu().numpy()          # and a block that ENDS inside one: chains 5, 6
    np.testing.assert_allclose(head[1], _direct_block(x[5:7], 0), rtol=1e-10, atol=1e-12)
    whole = dg.summarize(xd, chains_per_group=5)
    parts = dg.summarize([xd[:7], xd[7:]], chains_per_group=5)
    assert parts["lag_passes"] == whole["lag_passes"]
    for k in ("rhat", "ess", "mean", "var"):
        np.testing.assert_allclose(parts[k].cpu().numpy(), whole[k].cpu().numpy(), rtol=1e-12, err_msg=k)


def test_one_raw_pass_against_direct_sums_per_group(ragged):
    x, xd = ragged
    n = x.shape[1]
    blk = dg.chain_stats_pass(xd, [(3, n - 5)], 16, chains_per_group=5).cpu().numpy()
    assert blk.shape == (3, 19, 70)
    for g in range(3):
        sub = x[g * 5:(g + 1) * 5, 3:3 + n - 5]
        want = _direct_block(sub, 16)
        for k in (0, 5, 15):
            np.testing.assert_allclose(blk[g, 3 + k], want[3 + k], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(blk[g, 0], want[0], rtol=1e-12)
        assert not blk[g, 2].any()                                          # the variance row belongs to lag0 == 0


def test_one_group_is_the_ungrouped_call_bit_for_bit():
    xd = torch.from_numpy(ar1_chains(5000, 64, 70, 0.4, 2)).cuda()          # more chains than chain blocks, two slabs
    for t0, n, lag0 in ((0, 32, 0), (32, 32, 16)):
        one = _raw(xd, t0, n, lag0, 0, 5000)
        assert tuple(one.shape) == (1, 19, 70)
        assert torch.equal(one[0], _raw(xd, t0, n, lag0, 0, 0, entry="lmc_diag_chain_stats")[0])


def test_grouped_statistics_are_bit_reproducible():
    xd = torch.from_numpy(_job(7, 300, 64, 70)).cuda()                      # 7 groups x 292 chain blocks x 2 slabs
    a = dg.chain_stats_pass(xd, [(0, 32), (32, 32)], 0, chains_per_group=300)
    b = dg.chain_stats_pass(xd, [(0, 32), (32, 32)], 0, chains_per_group=300)
    assert tuple(a.shape) == (7, 19, 70) and torch.equal(a, b)


def test_batched_job_end_to_end():
    d, chains, tune, draws = 6, 32, 150, 120
    b = lmc.targets.Batched([lmc.targets.AR1(d, 0.0), lmc.targets.AR1(d, 0.9)])
    trace, stats, eng = lmc.sample(b, d, draws=draws, tune=tune, chains=chains, random_seed=8, return_engine=True,
                                   progressbar=False)
    try:
        got = b.summarize(dg.trace_tensor(eng))
        assert got["groups"] == 2 and got["n_chains"] == 32.0
        for g, sl in enumerate(b.chain_slices(chains)):
            rhat, ess = odg.rhat_ess(trace[sl])
            np.testing.assert_allclose(got["rhat"][g].cpu().numpy(), rhat, rtol=1e-9)
            np.testing.assert_allclose(got["ess"][g].cpu().numpy(), ess, rtol=1e-7)
        assert float(got["ess_min"][1]) < float(got["ess_min"][0])          # rho = 0.9 is the harder posterior
    finally:
        eng.close()
