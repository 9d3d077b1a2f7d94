"""No-GPU tests of the posterior quantiles: the numpy model of the radix select (tests/_select_model.py) against np.sort, the
C entry's declaration and refusals, and the host logic of littlemcmc_amd/diagnostics.py (order_statistics, quantiles,
intervals, tail_ess) with the model injected for the HIP call."""
import ctypes
import os

import numpy as np
import pytest
import torch

from littlemcmc_amd import _abi
from littlemcmc_amd import diagnostics as dg
from littlemcmc_amd import targets as T
from oracle import diagnostics_oracle as odg
from tests import _select_model as M
from tests.test_diagnostics_cpu import ar1_chains

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FFT = odg.torch_chain_stats
RHOS = (0.2, 0.97, -0.5)
EPS = np.finfo(np.float64).eps


def grouped_chains(per, n, d, seed=31):
    return np.concatenate([ar1_chains(per, n, d, rho, seed + g) for g, rho in enumerate(RHOS)])


@pytest.fixture(scope="module")
def job():
    """(G, per, n, d) = (3, 5, 61, 70)."""
    x = grouped_chains(5, 61, 70)
    return x, torch.from_numpy(x)


def _sorted_groups(x, per):
    """[G, S, d]: every group's pooled draws, sorted per dimension."""
    G = x.shape[0] // per
    return np.sort(x.reshape(G, per * x.shape[1], x.shape[2]), axis=1)


def test_model_select_equals_np_sort():
    col = M.hostile_column()
    S = len(col)
    ranks = [0, 1, S // 20, S // 4, S // 2, S // 2 + 1, S - 18, S - 2, S - 1] + list(range(100, 140, 3))
    assert len(ranks) > M.MAX_RANKS                                       # two rounds of the model, too
    want = np.sort(col)[ranks]
    got = M.select(col, ranks)
    np.testing.assert_array_equal(got, want)
    # np.sort leaves the order of -0 / +0 open; the key does not: every sign bit is the key-sorted pool's
    np.testing.assert_array_equal(np.signbit(M.select(col, range(S))), np.signbit(M.key_sorted(col)))
    np.testing.assert_array_equal(M.select(col, range(S)), M.key_sorted(col))
    const = np.full(50, -2.75)
    np.testing.assert_array_equal(M.select(const, [0, 7, 49]), np.sort(const)[[0, 7, 49]])
    # with +-NaN the extreme keys decode to -NaN and +NaN
    nan = np.concatenate([col, [np.nan, -np.nan]])
    lo, hi = M.select(nan, [0, len(nan) - 1])
    assert np.isnan(lo) and np.signbit(lo) and np.isnan(hi) and not np.signbit(hi)
    np.testing.assert_array_equal(M.unkey(M.key(col)), col)
    assert (np.diff(M.key(np.sort(col)).astype(object)) >= 0).all()


def test_abi_symbol_constant_and_refusals_before_any_hip_call():
    lib = _abi.load()
    assert "lmc_select_digit_counts" in _abi.EXPORTED_SYMBOLS and hasattr(lib, "lmc_select_digit_counts")
    header = open(os.path.join(ROOT, "include", "lmc_hip.h")).read()
    assert "#define LMC_SELECT_MAX_RANKS 16" in header and _abi.SELECT_MAX_RANKS == 16 == M.MAX_RANKS
    assert "lmc_select_digit_counts(" in header
    assert lib.lmc_abi_version() == 9 == _abi.ABI_VERSION                 # additive: the ABI number stays
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(x=p, chains=4, stride=10, dim=3, t0=0, n=10, first=0, per=2, shift=48, n_ranks=3, prefix=p, counts=p):
        return lib.lmc_select_digit_counts(x, chains, stride, dim, t0, n, first, per, shift, n_ranks, prefix, counts, None)

    for kw in (dict(x=None), dict(counts=None), dict(prefix=None), dict(chains=0), dict(dim=0), dict(n=0), dict(t0=-1),
               dict(t0=1), dict(n=11), dict(first=-1), dict(per=0), dict(shift=-8), dict(shift=4), dict(shift=64),
               dict(shift=60), dict(n_ranks=0), dict(n_ranks=_abi.SELECT_MAX_RANKS + 1), dict(shift=56, n_ranks=2),
               dict(shift=56, n_ranks=2, prefix=None), dict(chains=2 ** 31), dict(first=2 ** 31 - 4), dict(first=2 ** 62),
               dict(n=2 ** 31, stride=2 ** 31)):
        assert call(**kw) == 1, kw   # LMC_ERR_INVALID


def test_order_statistics_equal_np_sort(job):
    x, xt = job
    S = 5 * 61
    ranks = [0, 1, S // 20, S // 2, S - 2, S - 1]
    srt = _sorted_groups(x, 5)
    got = dg.order_statistics(xt, ranks, chains_per_group=5, count_fn=M.count_fn)
    assert tuple(got.shape) == (3, 6, 70) and got.dtype == torch.float64
    np.testing.assert_array_equal(got.numpy(), srt[:, ranks, :])
    # blocks of 4 + 11 chains: group 0 straddles the two blocks
    parts = dg.order_statistics([xt[:4], xt[4:]], ranks, chains_per_group=5, count_fn=M.count_fn)
    assert torch.equal(parts, got)
    assert torch.equal(dg.order_statistics([xt[:4], xt[4:4], xt[4:]], ranks, chains_per_group=5, count_fn=M.count_fn), got)
    # ungrouped: one pool of all 15 chains, as one tensor and as two blocks
    one = dg.order_statistics(xt, [0, 100, 15 * 61 - 1], count_fn=M.count_fn)
    assert tuple(one.shape) == (3, 70)
    np.testing.assert_array_equal(one.numpy(), np.sort(x.reshape(-1, 70), axis=0)[[0, 100, 15 * 61 - 1]])
    assert torch.equal(dg.order_statistics([xt[:7], xt[7:]], [0, 100, 15 * 61 - 1], count_fn=M.count_fn), one)


def test_scratch_chunks_rounds_and_duplicates(job):
    x, xt = job
    S = 5 * 61
    srt = _sorted_groups(x, 5)
    ranks = [0, 1, S // 20, S // 2, S - 2, S - 1]
    got = dg.order_statistics(xt, ranks, chains_per_group=5, count_fn=M.count_fn)
    calls = []

    def counting(xb, first, per, shift, prefix):
        calls.append((int(xb.shape[0]), first, shift))
        return M.count_fn(xb, first, per, shift, prefix)

    unit = 256 * 70 * 8 * len(ranks)
    assert torch.equal(dg.order_statistics(xt, ranks, chains_per_group=5, scratch_bytes=unit, count_fn=counting), got)
    assert len(calls) == 3 * 8 and {c[:2] for c in calls} == {(5, 0), (5, 5), (5, 10)}     # one group per chunk
    del calls[:]
    assert torch.equal(dg.order_statistics(xt, ranks, chains_per_group=5, scratch_bytes=2 * unit, count_fn=counting), got)
    assert {c[:2] for c in calls} == {(10, 0), (5, 10)}
    with pytest.raises(ValueError, match=str(unit)):
        dg.order_statistics(xt, ranks, chains_per_group=5, scratch_bytes=unit - 1, count_fn=M.count_fn)
    # 20 distinct ranks: two rounds that share the shift-56 pass
    many = list(range(3, 3 + 20 * 15, 15))
    del calls[:]
    two = dg.order_statistics(xt, many, chains_per_group=5, count_fn=counting)
    np.testing.assert_array_equal(two.numpy(), srt[:, many, :])
    assert [c[2] for c in calls].count(56) == 1 and len(calls) == 1 + 2 * 7
    # duplicated and unordered ranks
    dup = [S - 1, 0, 17, 17, 0, S // 2, 17]
    np.testing.assert_array_equal(dg.order_statistics(xt, dup, chains_per_group=5, count_fn=M.count_fn).numpy(), srt[:, dup, :])
    for bad in ([], [-1], [S]):
        with pytest.raises(ValueError):
            dg.order_statistics(xt, bad, chains_per_group=5, count_fn=M.count_fn)


def test_quantiles_formula_and_numpy(job):
    x, xt = job
    S = 5 * 61
    probs = [0.0, 0.05, 0.25, 0.5, 0.731, 0.95, 1.0]
    out = dg.quantiles(xt, probs, chains_per_group=5, count_fn=M.count_fn)
    assert set(out) == {"quantiles", "min", "max", "n", "probs"} and out["n"] == S
    assert tuple(out["quantiles"].shape) == (3, len(probs), 70) and tuple(out["min"].shape) == (3, 70)
    srt = _sorted_groups(x, 5)
    np.testing.assert_array_equal(out["min"].numpy(), srt[:, 0]), np.testing.assert_array_equal(out["max"].numpy(), srt[:, -1])
    worst = 0.0
    for k, p in enumerate(probs):
        h = p * (S - 1)
        lo = int(np.floor(h))
        hi = min(lo + 1, S - 1)
        want = srt[:, lo] + (srt[:, hi] - srt[:, lo]) * (h - lo)            # the documented formula
        np.testing.assert_array_equal(out["quantiles"][:, k].numpy(), want)
        ref = np.quantile(srt, p, axis=1)
        tol = 8 * EPS * np.maximum(np.abs(srt[:, lo]), np.abs(srt[:, hi]))
        dev = np.abs(out["quantiles"][:, k].numpy() - ref)
        worst = max(worst, float((dev / np.maximum(tol / 8, 1e-300)).max()))
        assert (dev <= tol).all(), (p, dev.max())
    print("largest deviation from np.quantile: %.2f eps x max(|v_lo|, |v_hi|)" % worst)
    one = dg.quantiles(xt[:5], np.array([0.05, 0.5]), count_fn=M.count_fn)      # ungrouped: no leading axis
    assert tuple(one["quantiles"].shape) == (2, 70) and torch.equal(one["quantiles"], out["quantiles"][0, [1, 3]])
    iv = dg.intervals(xt, 0.9, chains_per_group=5, count_fn=M.count_fn)
    q3 = dg.quantiles(xt, [(1.0 - 0.9) / 2.0, 0.5, 1.0 - (1.0 - 0.9) / 2.0], chains_per_group=5, count_fn=M.count_fn)["quantiles"]
    assert iv["level"] == 0.9 and all(torch.equal(iv[k], q3[:, i]) for i, k in enumerate(("lower", "median", "upper")))
    b = T.Batched([T.AR1(70, rho=r) for r in RHOS])
    assert torch.equal(b.quantiles(xt, probs, count_fn=M.count_fn)["quantiles"], out["quantiles"])
    assert torch.equal(b.quantiles([xt[:4], xt[4:]], probs, count_fn=M.count_fn)["quantiles"], out["quantiles"])
    assert torch.equal(b.intervals(xt, count_fn=M.count_fn)["upper"], iv["upper"])


@pytest.mark.parametrize("nan", [np.nan, -np.nan], ids=["+nan", "-nan"])
def test_a_nan_draw_poisons_its_cell_only(job, nan):
    x, _xt = job
    y = x[:, :, :5].copy()
    y[7, 11, 3] = nan                                                      # group 1, dimension 3
    probs = [0.0, 0.3, 0.5, 1.0]
    out = dg.quantiles(torch.from_numpy(y), probs, chains_per_group=5, count_fn=M.count_fn)
    clean = dg.quantiles(torch.from_numpy(x[:, :, :5].copy()), probs, chains_per_group=5, count_fn=M.count_fn)
    q = out["quantiles"].numpy()
    cell = np.zeros(q.shape, dtype=bool)
    cell[1, :, 3] = True
    assert np.isnan(q[cell]).all() and not np.isnan(q[~cell]).any()
    np.testing.assert_array_equal(q[~cell], clean["quantiles"].numpy()[~cell])
    assert bool(torch.isnan(out["min" if np.signbit(nan) else "max"][1, 3]))


def test_refusals(job, monkeypatch):
    x, xt = job
    kw = dict(chains_per_group=5, count_fn=M.count_fn)
    for bad in ([], [-0.1], [0.5, 1.5], [float("nan")]):
        with pytest.raises(ValueError, match="probs"):
            dg.quantiles(xt, bad, **kw)
    for empty in (xt[:0], xt[:, :0], xt[:, :, :0], []):
        with pytest.raises(ValueError):
            dg.quantiles(empty, [0.5], count_fn=M.count_fn)
    with pytest.raises(ValueError, match="differ in d"):
        dg.quantiles([xt[:5], xt[5:, :, :3]], [0.5], **kw)
    with pytest.raises(ValueError, match="needs a multiple of"):
        dg.quantiles(xt, [0.5], chains_per_group=4, count_fn=M.count_fn)
    with pytest.raises(ValueError, match="level"):
        dg.intervals(xt, 1.0, **kw)
    with pytest.raises(_abi.HipLibraryError):
        dg.quantiles(xt, [0.5], chains_per_group=5)                         # a CPU tensor and no count_fn
    with pytest.raises(_abi.HipLibraryError):
        dg.order_statistics(xt, [0])
    import torch.distributed as dist

    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    with pytest.raises(ValueError, match="process group"):
        dg.quantiles(xt, [0.5], count_fn=M.count_fn)
    with pytest.raises(ValueError, match="process group"):
        dg.order_statistics(xt, [0], **kw)


def test_tail_ess_against_the_oracle():
    """(G, per, n, d) = (3, 5, 200, 6): the ESS of the indicators x <= np.quantile(pool, p), the minimum over p."""
    x = grouped_chains(5, 200, 6)
    xt = torch.from_numpy(x)
    probs = (0.05, 0.95)
    out = dg.tail_ess(xt, chains_per_group=5, chunk_dims=4, count_fn=M.count_fn, stats_fn=FFT)
    assert tuple(out["ess_tail"].shape) == (3, 6) and tuple(out["ess_tail_min"].shape) == (3,) and out["groups"] == 3
    want = np.empty((3, 6))
    for g in range(3):
        sub = x[5 * g:5 * g + 5]
        q = np.quantile(sub.reshape(-1, 6), probs, axis=0)
        ess = [odg.rhat_ess((sub <= q[k]).astype(np.float64), do_split=True)[1] for k in range(len(probs))]
        want[g] = np.minimum(ess[0], ess[1])
    np.testing.assert_allclose(out["ess_tail"].numpy(), want, rtol=1e-7)
    np.testing.assert_array_equal(out["ess_tail_min"].numpy(), out["ess_tail"].numpy().min(axis=1))
    assert int(out["ess_tail_min"].argmin()) == 1                          # rho = 0.97 is the slow posterior
    # blocks with a straddling group, the chunk size, the Batched method and the ungrouped form
    parts = dg.tail_ess([xt[:7], xt[7:]], chains_per_group=5, count_fn=M.count_fn, stats_fn=FFT)
    np.testing.assert_allclose(parts["ess_tail"].numpy(), out["ess_tail"].numpy(), rtol=1e-12)
    b = T.Batched([T.AR1(6, rho=r) for r in RHOS])
    assert torch.equal(b.tail_ess(xt, chunk_dims=4, count_fn=M.count_fn, stats_fn=FFT)["ess_tail"], out["ess_tail"])
    alone = dg.tail_ess(xt[5:10], count_fn=M.count_fn, stats_fn=FFT)
    assert tuple(alone["ess_tail"].shape) == (6,) and "ess_tail_min" not in alone
    np.testing.assert_allclose(alone["ess_tail"].numpy(), want[1], rtol=1e-7)
