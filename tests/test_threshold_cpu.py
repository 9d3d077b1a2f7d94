"""No-GPU tests of the threshold counts: the C entry's declaration and refusals, and the host logic of
littlemcmc_amd/diagnostics.py (threshold_counts, prob, direction, rope) with the numpy model of one count call
(tests/_threshold_model.py) injected for the HIP call."""
import ctypes
import os

import numpy as np
import pytest
import torch

from littlemcmc_amd import _abi
from littlemcmc_amd import diagnostics as dg
from littlemcmc_amd import targets as T
from oracle import diagnostics_oracle as odg
from tests import _threshold_model as M
from tests.test_diagnostics_cpu import ar1_chains

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FFT = odg.torch_chain_stats
RHOS = (0.2, 0.97, -0.5)
KW = dict(chains_per_group=5, count_fn=M.count_fn)


def grouped_chains(per, n, d, seed=31):
    return np.concatenate([ar1_chains(per, n, d, rho, seed + g) for g, rho in enumerate(RHOS)])


@pytest.fixture(scope="module")
def job():
    """(G, per, n, d) = (3, 5, 61, 7), with ties: every value rounded to a quarter."""
    x = np.round(grouped_chains(5, 61, 7) * 4.0) / 4.0
    return x, torch.from_numpy(x)


def direct(x, per, thr):
    """(less, equal) [G, K, d] of thresholds [G, K, d] by plain numpy."""
    G = x.shape[0] // per
    pool = x.reshape(G, -1, 1, x.shape[2])
    return (pool < thr[:, None]).sum(axis=1), (pool == thr[:, None]).sum(axis=1)


def test_abi_symbol_constant_and_refusals_before_any_hip_call():
    lib = _abi.load()
    assert "lmc_diag_threshold_counts" in _abi.EXPORTED_SYMBOLS and hasattr(lib, "lmc_diag_threshold_counts")
    header = open(os.path.join(ROOT, "include", "lmc_hip.h")).read()
    assert "#define LMC_THRESHOLD_MAX 16" in header and _abi.THRESHOLD_MAX == 16 == M.MAX_THRESHOLDS
    assert "lmc_diag_threshold_counts(" in header
    assert len(_abi._SIGNATURES["lmc_diag_threshold_counts"][1]) == 12
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(x=p, chains=4, stride=10, dim=3, t0=0, n=10, first=0, per=2, k=3, thr=p, counts=p):
        return lib.lmc_diag_threshold_counts(x, chains, stride, dim, t0, n, first, per, k, thr, counts, None)

    for kw in (dict(x=None), dict(counts=None), dict(thr=None), dict(chains=0), dict(dim=0), dict(n=0), dict(t0=-1), dict(t0=1),
               dict(n=11), dict(first=-1), dict(per=0), dict(k=0), dict(k=-1), dict(k=_abi.THRESHOLD_MAX + 1),
               dict(chains=2 ** 31), dict(first=2 ** 31 - 4), dict(first=2 ** 62), dict(n=2 ** 31, stride=2 ** 31)):
        assert call(**kw) == 1, kw   # LMC_ERR_INVALID


def test_the_model_states_the_definition():
    x = np.array([[[0.0], [-0.0], [1.0], [np.nan], [np.inf], [-np.inf], [1.0]]])            # one chain, 7 draws, d = 1
    thr = np.array([0.0, -0.0, 1.0, np.nan, np.inf, -np.inf, 0.5]).reshape(1, 7, 1)
    got = M.counts(x, 0, 7, 0, 1, thr)[0, :, 0]
    #                 <0 ==0  <-0 ==-0  <1 ==1  nan     <inf ==inf  <-inf ==-inf  <.5 ==.5  NaN draws
    assert got.tolist() == [1, 2, 1, 2, 3, 2, 0, 0, 5, 1, 0, 1, 3, 0, 1]
    # a view and a partial group: rows [2, 5) of chains that are chains 3, 4 of a job of 3 chains a group
    y = np.arange(2 * 6 * 2, dtype=np.float64).reshape(2, 6, 2)
    c = M.counts(y, 2, 3, 3, 3, np.full((1, 1, 2), 17.0))
    assert c.shape == (1, 3, 2) and c[0, :, 0].tolist() == [4, 0, 0] and c[0, :, 1].tolist() == [3, 1, 0]
    assert M.touched(3, 9, 5) == (0, 3)


def test_every_form_of_thresholds(job):
    x, xt = job
    d = 7
    rng = np.random.default_rng(3)
    full = np.round(rng.standard_normal((3, 4, d)) * 4.0) / 4.0
    less, equal = direct(x, 5, full)
    out = dg.threshold_counts(xt, full, **KW)
    assert out["n"] == 5 * 61 and out["less"].dtype == torch.int64 and tuple(out["less"].shape) == (3, 4, d)
    np.testing.assert_array_equal(out["less"].numpy(), less)
    np.testing.assert_array_equal(out["equal"].numpy(), equal)
    assert equal.sum() > 0 and tuple(out["nan"].shape) == (3, d) and int(out["nan"].sum()) == 0
    # [K, d], [d], a scalar, 1-D of length K (a torch tensor, a list): shared by the groups
    for thr, as_kd in ((full[0], full[0]), (full[0, 0], full[0, :1]), (0.25, np.full((1, d), 0.25)),
                       (torch.tensor([0.5, -0.25, 1.0]), np.repeat([[0.5], [-0.25], [1.0]], d, axis=1)),
                       ([0.0, 1.0], np.repeat([[0.0], [1.0]], d, axis=1))):
        want = direct(x, 5, np.broadcast_to(as_kd, (3,) + as_kd.shape))
        got = dg.threshold_counts(xt, thr, **KW)
        np.testing.assert_array_equal(got["less"].numpy(), want[0])
        np.testing.assert_array_equal(got["equal"].numpy(), want[1])
    # ungrouped: one pool of all 15 chains, no leading axis
    one = dg.threshold_counts(xt, full[0], count_fn=M.count_fn)
    want = direct(x, 15, full[:1])
    assert tuple(one["less"].shape) == (4, d) and tuple(one["nan"].shape) == (d,) and one["n"] == 15 * 61
    np.testing.assert_array_equal(one["less"].numpy(), want[0][0])
    np.testing.assert_array_equal(one["equal"].numpy(), want[1][0])


def test_rounds_of_sixteen_and_blocks_with_a_straddling_group(job):
    x, xt = job
    thr = np.round(np.random.default_rng(4).standard_normal((3, 17, 7)) * 4.0) / 4.0
    less, equal = direct(x, 5, thr)
    calls = []

    def counting(xb, first, per, th):
        calls.append((int(xb.shape[0]), int(first), tuple(th.shape)))
        return M.count_fn(xb, first, per, th)

    out = dg.threshold_counts(xt, thr, chains_per_group=5, count_fn=counting)
    assert calls == [(15, 0, (3, 16, 7)), (15, 0, (3, 1, 7))]
    np.testing.assert_array_equal(out["less"].numpy(), less)
    np.testing.assert_array_equal(out["equal"].numpy(), equal)
    del calls[:]
    two = dg.threshold_counts([xt[:7], xt[7:7], xt[7:]], thr, chains_per_group=5, count_fn=counting)   # group 1 straddles
    assert calls == [(7, 0, (2, 16, 7)), (8, 7, (2, 16, 7)), (7, 0, (2, 1, 7)), (8, 7, (2, 1, 7))]
    for k in ("less", "equal", "nan"):
        assert torch.equal(two[k], out[k]), k
    b = T.Batched([T.AR1(7, rho=r) for r in RHOS])
    p = b.prob([xt[:7], xt[7:]], thr, count_fn=M.count_fn)
    np.testing.assert_array_equal(p["p_less"].numpy(), less / (5 * 61))
    np.testing.assert_array_equal(p["p_greater"].numpy(), (5 * 61 - less - equal) / (5 * 61))
    assert p["n"] == 5 * 61 and torch.equal(b.prob(xt, thr, count_fn=M.count_fn)["p_equal"], p["p_equal"])


@pytest.mark.parametrize("nan", [np.nan, -np.nan], ids=["+nan", "-nan"])
def test_a_nan_draw_poisons_its_cell_only(job, nan):
    x, xt = job
    y = x.copy()
    y[7, 11, 3] = nan                                                      # group 1, dimension 3
    thr = [-0.5, 0.0, 0.75]
    out = dg.prob(torch.from_numpy(y), thr, **KW)
    clean = dg.prob(xt, thr, **KW)
    cell = np.zeros((3, 3, 7), dtype=bool)
    cell[1, :, 3] = True
    for k in ("p_less", "p_equal", "p_greater"):
        v = out[k].numpy()
        assert np.isnan(v[cell]).all() and not np.isnan(v[~cell]).any(), k
        np.testing.assert_array_equal(v[~cell], clean[k].numpy()[~cell])
    want = np.zeros((3, 7), dtype=np.int64)
    want[1, 3] = 1
    np.testing.assert_array_equal(out["n_nan"].numpy(), want)
    np.testing.assert_allclose((clean["p_less"] + clean["p_equal"] + clean["p_greater"]).numpy(), 1.0, rtol=0, atol=4.5e-16)
    for fn, keys in ((lambda t: dg.direction(t, **KW), ("pd", "sign")), (lambda t: dg.rope(t, -0.5, 0.5, **KW), ("inside", "below", "above"))):
        bad, good = fn(torch.from_numpy(y)), fn(xt)
        for k in keys:
            v = bad[k].numpy()
            assert np.isnan(v[1, 3]) and np.isnan(v).sum() == 1, k
            np.testing.assert_array_equal(np.delete(v.ravel(), 10), np.delete(good[k].numpy().ravel(), 10))


def test_rope_and_direction_against_direct_counts(job):
    x, xt = job
    S = 5 * 61
    pool = x.reshape(3, S, 7)
    low = -0.5 + 0.25 * np.arange(7)
    r = dg.rope(xt, low, 1.0, **KW)
    np.testing.assert_array_equal(r["inside"].numpy(), ((pool >= low) & (pool <= 1.0)).sum(axis=1) / S)
    np.testing.assert_array_equal(r["below"].numpy(), (pool < low).sum(axis=1) / S)
    np.testing.assert_array_equal(r["above"].numpy(), (pool > 1.0).sum(axis=1) / S)
    assert r["n"] == S and ((pool == 1.0).sum() > 0) and ((pool == low).sum() > 0)       # the closed ends are exercised
    per_group = np.array([0.25, 0.5, 1.5]).reshape(3, 1) * np.ones((3, 7))
    g = dg.rope(xt, -per_group, per_group, **KW)
    np.testing.assert_array_equal(g["inside"].numpy(), (np.abs(pool) <= per_group[:, None]).sum(axis=1) / S)
    one = dg.rope(xt[:5], -0.25, 0.25, count_fn=M.count_fn)
    assert tuple(one["inside"].shape) == (7,) and torch.equal(one["inside"], g["inside"][0])
    calls = []
    dg.rope(xt, -1.0, 1.0, chains_per_group=5, count_fn=lambda *a: calls.append(tuple(a[3].shape)) or M.count_fn(*a))
    assert calls == [(3, 2, 7)]                                            # two thresholds, one pass
    shifted = x + np.array([0.0, 0.4, -0.4, 3.0, -3.0, 0.1, -0.1])
    pool = shifted.reshape(3, S, 7)
    dr = dg.direction(torch.from_numpy(shifted), **KW)
    pos, neg = (pool > 0).sum(axis=1) / S, (pool < 0).sum(axis=1) / S
    np.testing.assert_array_equal(dr["pd"].numpy(), np.maximum(pos, neg))
    np.testing.assert_array_equal(dr["sign"].numpy(), np.where(pos >= neg, 1.0, -1.0))
    assert set(np.unique(dr["sign"].numpy())) == {-1.0, 1.0} and (pool == 0).sum() > 0
    b = T.Batched([T.AR1(7, rho=rho) for rho in RHOS])
    assert torch.equal(b.rope(xt, low, 1.0, count_fn=M.count_fn)["inside"], r["inside"])
    assert torch.equal(b.direction(torch.from_numpy(shifted), count_fn=M.count_fn)["pd"], dr["pd"])


def test_mcse_against_the_oracle():
    """(G, per, n, d) = (3, 5, 200, 6): ess is the split ESS of the indicator x < c through the same statistics."""
    x = grouped_chains(5, 200, 6)
    xt = torch.from_numpy(x)
    thr = np.array([[-0.5] * 6, [0.3] * 6])
    out = dg.prob(xt, thr, mcse=True, chunk_dims=4, stats_fn=FFT, **KW)
    assert tuple(out["ess"].shape) == (3, 2, 6) == tuple(out["mcse"].shape)
    for k in range(2):
        ind = torch.from_numpy((x < thr[k]).astype(np.float64))
        want = dg.finalize(dg.sufficient_stats(ind, stats_fn=FFT, chains_per_group=5))["ess"]
        np.testing.assert_allclose(out["ess"][:, k].numpy(), want.numpy(), rtol=1e-12)
        for g in range(3):
            ref = odg.rhat_ess((x[5 * g:5 * g + 5] < thr[k]).astype(np.float64), do_split=True)[1]
            np.testing.assert_allclose(out["ess"][g, k].numpy(), ref, rtol=1e-7)
    p = out["p_less"]
    np.testing.assert_array_equal(out["mcse"].numpy(), torch.sqrt(p * (1.0 - p) / out["ess"]).numpy())
    parts = dg.prob([xt[:7], xt[7:]], thr, mcse=True, stats_fn=FFT, **KW)
    np.testing.assert_allclose(parts["ess"].numpy(), out["ess"].numpy(), rtol=1e-12)
    alone = dg.prob(xt[5:10], 0.3, mcse=True, stats_fn=FFT, count_fn=M.count_fn)
    assert tuple(alone["ess"].shape) == (1, 6)
    np.testing.assert_allclose(alone["ess"][0].numpy(), out["ess"][1, 1].numpy(), rtol=1e-12)
    assert "ess" not in dg.prob(xt, thr, **KW)


def test_refusals(job, monkeypatch):
    x, xt = job
    for bad in (np.zeros((2, 6)), np.zeros((4, 2, 7)), np.zeros((3, 0, 7)), np.zeros((0, 7)), np.zeros((1, 3, 2, 7))):
        with pytest.raises(ValueError, match="thresholds"):
            dg.threshold_counts(xt, bad, **KW)
    with pytest.raises(ValueError, match="thresholds"):
        dg.threshold_counts(xt, np.zeros((3, 2, 7)), count_fn=M.count_fn)     # [G, K, d] needs chains_per_group
    for empty in (xt[:0], xt[:, :0], xt[:, :, :0], []):
        with pytest.raises(ValueError):
            dg.threshold_counts(empty, 0.0, count_fn=M.count_fn)
    with pytest.raises(ValueError, match="needs a multiple of"):
        dg.threshold_counts(xt, 0.0, chains_per_group=4, count_fn=M.count_fn)
    with pytest.raises(ValueError, match="low <= high"):
        dg.rope(xt, 0.5, -0.5, **KW)
    with pytest.raises(ValueError, match="broadcast"):
        dg.rope(xt, np.zeros(3), 1.0, **KW)
    with pytest.raises(_abi.HipLibraryError):
        dg.threshold_counts(xt, 0.0, chains_per_group=5)                    # a CPU tensor and no count_fn
    with pytest.raises(_abi.HipLibraryError):
        dg.prob(xt, 0.0)
    import torch.distributed as dist

    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    with pytest.raises(ValueError, match="process group"):
        dg.threshold_counts(xt, 0.0, count_fn=M.count_fn)
    with pytest.raises(ValueError, match="process group"):
        dg.rope(xt, -1.0, 1.0, **KW)
