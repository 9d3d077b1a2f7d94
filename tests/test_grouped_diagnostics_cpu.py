"""Per-posterior diagnostics without a GPU: ``summarize(..., chains_per_group=)`` gives every group of a targets.Batched job
what ``summarize`` of that group's chains alone gives -- the reduction / finalisation logic with the oracle's FFT restatement
of the kernel's block injected through ``stats_fn`` -- and the new C entry is declared, bound, exported and refuses nonsense
before any HIP call."""
import ctypes
import os

import numpy as np
import pytest
import torch

from littlemcmc_amd import _abi
from littlemcmc_amd import diagnostics as dg
from littlemcmc_amd import targets as T
from oracle import diagnostics_oracle as odg
from tests.test_diagnostics_cpu import ar1_chains

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1   # LMC_ERR_INVALID
FFT = odg.torch_chain_stats
RHOS = (0.2, 0.97, -0.5)


def grouped_chains(per, n, d, rhos=RHOS, seed=31):
    """len(rhos) groups of ``per`` AR(1) chains each, one rho per group: the groups need different numbers of lag passes."""
    return np.concatenate([ar1_chains(per, n, d, rho, seed + g) for g, rho in enumerate(rhos)])


@pytest.fixture(scope="module")
def job():
    x = grouped_chains(5, 301, 70)
    return x, torch.from_numpy(x), [slice(5 * g, 5 * g + 5) for g in range(3)]


def test_new_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "lmc_hip.h")).read()
    lib = _abi.load()
    assert "lmc_diag_chain_stats_grouped(" in header
    assert "lmc_diag_chain_stats_grouped" in _abi.EXPORTED_SYMBOLS and hasattr(lib, "lmc_diag_chain_stats_grouped")
    assert lib.lmc_abi_version() == 9 == _abi.ABI_VERSION     # additive: the ABI number stays


def test_grouped_entry_refuses_before_any_hip_call():
    """No device is needed to see a refusal: with NULL pointers, and with pointers that are there (host memory the entry
    never gets to touch) so that the refusal is the argument's and not the NULL's."""
    lib = _abi.load()
    fn = lib.lmc_diag_chain_stats_grouped
    buf = np.zeros(64)
    for x, out in ((None, None), (_abi.ptr(buf), _abi.ptr(buf))):
        # (chains, draws_stride, dim, t0, n, lag0, first_chain, chains_per_group)
        assert fn(x, 4, 16, 2, 0, 16, 0, 0, 0, out, None) == INVALID               # chains_per_group = 0
        assert fn(x, 4, 16, 2, 0, 16, 0, -1, 2, out, None) == INVALID              # a negative first_chain
        assert fn(x, 4, 16, 2, 0, 16, 0, 2 ** 31 - 4, 2, out, None) == INVALID     # first_chain + chains = 2^31
        assert fn(x, 4, 16, 2, 0, 16, 0, 2 ** 62, 2, out, None) == INVALID
        assert fn(x, 0, 16, 2, 0, 16, 0, 0, 2, out, None) == INVALID               # the existing conditions
        assert fn(x, 4, 16, 2, 1, 16, 0, 0, 2, out, None) == INVALID
        assert fn(x, 4, 16, 2, 0, 16, -1, 0, 2, out, None) == INVALID


@pytest.mark.parametrize("split", [True, False])
def test_grouped_summary_equals_every_group_summarised_alone(job, split):
    x, xt, slices = job
    got = dg.summarize(xt, split=split, chains_per_group=5, stats_fn=FFT)
    assert got["groups"] == 3 and got["n_chains"] == (10.0 if split else 5.0)
    for k in ("rhat", "ess", "mean", "var"):
        assert tuple(got[k].shape) == (3, 70), k
    alone = [dg.summarize(xt[sl], split=split, stats_fn=FFT) for sl in slices]
    assert [a["lag_passes"] for a in alone][0] < alone[1]["lag_passes"]          # the groups do need different numbers
    assert got["lag_passes"] == max(a["lag_passes"] for a in alone)
    for g, (sl, a) in enumerate(zip(slices, alone)):
        # extra lag passes forced by the slow group do not change a fast one: finalize cuts at the initial positive sequence
        for k in ("rhat", "mean", "var"):
            np.testing.assert_array_equal(got[k][g].numpy(), a[k].numpy(), err_msg=k)
        np.testing.assert_allclose(got["ess"][g].numpy(), a["ess"].numpy(), rtol=1e-12)
        rhat, ess = odg.rhat_ess(x[sl], do_split=split)
        np.testing.assert_allclose(got["rhat"][g].numpy(), rhat, rtol=1e-9)
        np.testing.assert_allclose(got["ess"][g].numpy(), ess, rtol=1e-7)
    np.testing.assert_array_equal(got["rhat_max"].numpy(), got["rhat"].numpy().max(axis=1))
    np.testing.assert_array_equal(got["ess_min"].numpy(), got["ess"].numpy().min(axis=1))
    assert int(got["ess_min"].argmin()) == 1                                     # rho = 0.97 is the slow posterior


@pytest.mark.parametrize("split", [True, False])
def test_one_chain_per_group(split):
    """m = 1 unsplit: the between-chain term is zero."""
    x = grouped_chains(1, 301, 70)
    got = dg.summarize(torch.from_numpy(x), split=split, chains_per_group=1, stats_fn=FFT)
    assert got["groups"] == 3
    for g in range(3):
        a = dg.summarize(torch.from_numpy(x[g:g + 1]), split=split, stats_fn=FFT)
        for k in ("rhat", "mean", "var"):
            np.testing.assert_array_equal(got[k][g].numpy(), a[k].numpy(), err_msg=k)
        np.testing.assert_allclose(got["ess"][g].numpy(), a["ess"].numpy(), rtol=1e-12)
        rhat, ess = odg.rhat_ess(x[g:g + 1], do_split=split)
        np.testing.assert_allclose(got["rhat"][g].numpy(), rhat, rtol=1e-9)
        np.testing.assert_allclose(got["ess"][g].numpy(), ess, rtol=1e-7)


def test_rank_normalised_within_groups(job):
    x, xt, slices = job
    xr = np.round(x[:, :, :6], 1)                                  # rounding makes exact ties
    xr[5:10] += 3.0                                                # pooled ranks over all groups would see this shift
    xt = torch.from_numpy(xr)
    z = dg.rank_normalize(xt, chains_per_group=5)
    got = dg.summarize(xt, rank_normalized=True, chains_per_group=5, stats_fn=FFT)
    for g, sl in enumerate(slices):
        np.testing.assert_allclose(z[sl].numpy(), odg.rank_normalize(xr[sl]), rtol=1e-12, atol=1e-14)
        np.testing.assert_array_equal(z[sl].numpy(), dg.rank_normalize(xt[sl]).numpy())
        a = dg.summarize(xt[sl], rank_normalized=True, stats_fn=FFT)
        for k in ("rhat", "mean", "var"):
            np.testing.assert_array_equal(got[k][g].numpy(), a[k].numpy(), err_msg=k)
        np.testing.assert_allclose(got["ess"][g].numpy(), a["ess"].numpy(), rtol=1e-12)
        rhat, ess = odg.rhat_ess(xr[sl], rank_normalized=True)
        np.testing.assert_allclose(got["rhat"][g].numpy(), rhat, rtol=1e-8)
        np.testing.assert_allclose(got["ess"][g].numpy(), ess, rtol=1e-6)


def test_blocks_with_a_straddling_group(job):
    """[x[:7], x[7:]]: group 1 has two chains in the first block and three in the second; its statistics are the sum of the parts."""
    x, xt, slices = job
    whole = dg.summarize(xt, chains_per_group=5, stats_fn=FFT)
    parts = dg.summarize([xt[:7], xt[7:]], chains_per_group=5, stats_fn=FFT)
    assert parts["lag_passes"] == whole["lag_passes"] and parts["groups"] == 3
    for k in ("rhat", "ess", "mean", "var"):
        np.testing.assert_allclose(parts[k].numpy(), whole[k].numpy(), rtol=1e-12, err_msg=k)
    # a block of the job on its own: chains 7..14 touch groups 1 and 2, group 1 with its chains 7, 8, 9 only
    blk = dg.chain_stats_pass(xt[7:], [(0, 301)], 0, stats_fn=FFT, chains_per_group=5, first_chain=7)
    assert tuple(blk.shape) == (2, 19, 70)
    np.testing.assert_array_equal(blk[0].numpy(), FFT(xt[7:10], 0, 301, 0).numpy())
    np.testing.assert_array_equal(blk[1].numpy(), FFT(xt[10:], 0, 301, 0).numpy())
    with pytest.raises(ValueError, match="straddles"):
        dg.summarize([xt[:7], xt[7:]], chains_per_group=5, rank_normalized=True, stats_fn=FFT)
    # no group straddles [x[:5], x[5:]] (an empty block in between changes nothing): ranks within groups, block by block
    ok = dg.summarize([xt[:5], xt[:0], xt[5:]], chains_per_group=5, rank_normalized=True, stats_fn=FFT)
    ref = dg.summarize(xt, chains_per_group=5, rank_normalized=True, stats_fn=FFT)
    for k in ("rhat", "ess"):
        np.testing.assert_allclose(ok[k].numpy(), ref[k].numpy(), rtol=1e-12, err_msg=k)


def test_chain_total_must_be_a_multiple_of_the_group_size(job):
    x, xt, slices = job
    for per in (4, 16, 0):
        with pytest.raises(ValueError, match="needs a multiple of"):
            dg.summarize(xt, chains_per_group=per, stats_fn=FFT)
    with pytest.raises(ValueError, match="needs a multiple of"):
        dg.rank_normalize(xt, chains_per_group=4)
    with pytest.raises(ValueError, match="needs a multiple of"):
        dg.rhat_from_moments(np.zeros((15, 3)), np.ones((15, 3)), np.full(15, 10), chains_per_group=4)


def test_chains_per_group_is_refused_with_an_active_process_group(job, tmp_path):
    import torch.distributed as dist

    x, xt, slices = job
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "rendezvous"), rank=0, world_size=1)
    try:
        with pytest.raises(ValueError, match="Batched does not run under sample_distributed"):
            dg.summarize(xt, chains_per_group=5, stats_fn=FFT)
        with pytest.raises(ValueError, match="Batched does not run under sample_distributed"):
            dg.rank_normalize(xt, chains_per_group=5)
        with pytest.raises(ValueError, match="Batched does not run under sample_distributed"):
            dg.rhat_from_moments(np.zeros((15, 3)), np.ones((15, 3)), np.full(15, 10), chains_per_group=5)
        assert tuple(dg.summarize(xt, stats_fn=FFT)["rhat"].shape) == (70,)      # the ungrouped call is what it was
    finally:
        dist.destroy_process_group()


def test_rhat_from_moments_per_group(job):
    x, xt, slices = job
    mean = x.mean(axis=1)
    m2 = ((x - mean[:, None, :]) ** 2).sum(axis=1)
    n = np.full(15, x.shape[1])
    got = dg.rhat_from_moments(mean, m2, n, chains_per_group=5)
    assert tuple(got.shape) == (3, 70)
    for g, sl in enumerate(slices):
        # the same formula on sums over 5 chains that torch may associate differently: a few ulp
        np.testing.assert_allclose(got[g].numpy(), dg.rhat_from_moments(mean[sl], m2[sl], n[sl]).numpy(), rtol=1e-12)
        np.testing.assert_allclose(got[g].numpy(), odg.rhat_ess(x[sl], do_split=False)[0], rtol=1e-9)
    one = dg.rhat_from_moments(mean[:3], m2[:3], n[:3], chains_per_group=1)       # one chain per group: no between-chain term
    for g in range(3):
        np.testing.assert_allclose(one[g].numpy(), dg.rhat_from_moments(mean[g:g + 1], m2[g:g + 1], n[g:g + 1]).numpy(), rtol=1e-12)


def test_batched_summarize_passes_its_group_size(job, monkeypatch):
    x, xt, slices = job
    b = T.Batched([T.AR1(70, rho=r) for r in RHOS])
    got = b.summarize(xt, stats_fn=FFT)
    want = dg.summarize(xt, chains_per_group=5, stats_fn=FFT)
    for k in ("rhat", "ess", "rhat_max", "ess_min"):
        np.testing.assert_array_equal(got[k].numpy(), want[k].numpy())
    seen = []
    monkeypatch.setattr(dg, "summarize", lambda x, **kw: seen.append(kw) or "result")
    assert b.summarize(xt, split=False) == "result"
    assert b.summarize([xt[:7], xt[7:]]) == "result"                 # the per-GPU list: the chain total counts
    assert b.summarize(torch.cat([xt, xt])) == "result"
    assert seen == [{"chains_per_group": 5, "split": False}, {"chains_per_group": 5}, {"chains_per_group": 10}]
    with pytest.raises(ValueError, match="needs a multiple of 3 chains"):
        b.summarize(xt[:14])


def test_without_the_keyword_nothing_changes(job):
    x, xt, slices = job
    sub = xt[:5, :, :6]
    for kw in ({}, {"split": False}, {"rank_normalized": True}):
        got = dg.summarize(sub, stats_fn=FFT, **kw)
        assert sorted(got) == ["definition", "ess", "lag_passes", "mean", "n_chains", "n_draws", "rhat", "var"]
        for k in ("rhat", "ess", "mean", "var"):
            assert tuple(got[k].shape) == (6,), k
        split = kw.get("split", True)
        y = dg.rank_normalize(sub) if kw.get("rank_normalized") else sub
        want = dg.finalize(dg.sufficient_stats(y, split=split, stats_fn=FFT))
        for k in ("rhat", "ess", "mean", "var"):
            np.testing.assert_array_equal(got[k].numpy(), want[k].numpy(), err_msg=k)
        assert got["n_chains"] == (10.0 if split else 5.0) and got["n_draws"] == (150.0 if split else 301.0)
        rhat, ess = odg.rhat_ess(sub.numpy(), do_split=split, rank_normalized=bool(kw.get("rank_normalized")))
        rtol_rhat, rtol_ess = (1e-8, 1e-6) if kw.get("rank_normalized") else (1e-9, 1e-7)
        np.testing.assert_allclose(got["rhat"].numpy(), rhat, rtol=rtol_rhat)
        np.testing.assert_allclose(got["ess"].numpy(), ess, rtol=rtol_ess)
        halves = dg.split_chains(y) if split else y
        np.testing.assert_allclose(got["mean"].numpy(), halves.mean(dim=(0, 1)).numpy(), rtol=1e-12, atol=1e-14)
    blk = dg.chain_stats_pass(sub, [(0, 301)], 0, stats_fn=FFT)
    assert tuple(blk.shape) == (19, 6)
    np.testing.assert_array_equal(blk.numpy(), FFT(sub, 0, 301, 0).numpy())
