"""-m "not gpu": the host side of the covariance pass -- the ABI of lmc_diag_cross_moments and its refusals before any HIP
call, merge_cross_moments and the fan-out against the longdouble model (tests/_cross_model.py), covariance / contrasts
against numpy.cov / numpy.corrcoef, and the refusals of the job."""
import ctypes
import os

import numpy as np
import pytest
import torch

from littlemcmc_amd import _abi
from littlemcmc_amd import diagnostics as dg
from littlemcmc_amd import targets as T
from tests import _cross_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER = 2
CUTS = ([6], [2, 4], [3, 3], [1, 0, 5])   # [3, 3] cuts inside group 1; 6 chains, 3 groups of 2 (tests/test_trace_job_cpu.py)


def _draws(chains=6, n=23, d=5, seed=3):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((d, d)) / np.sqrt(d) + np.eye(d)
    return 3.0 + rng.standard_normal((chains, n, d)) @ a.T + rng.standard_normal((chains, 1, 1))


def _cut(x, sizes):
    out, lo = [], 0
    for s in sizes:
        out.append(x[lo:lo + s])
        lo += s
    return out


def test_abi_symbol_constant_and_refusals_before_any_hip_call():
    lib = _abi.load()
    assert "lmc_diag_cross_moments" in _abi.EXPORTED_SYMBOLS and hasattr(lib, "lmc_diag_cross_moments")
    header = open(os.path.join(ROOT, "include", "lmc_hip.h")).read()
    assert "#define LMC_CROSS_MAX_DIM 512" in header and _abi.CROSS_MAX_DIM == 512
    assert "lmc_diag_cross_moments(" in header
    assert lib.lmc_abi_version() == 9 == _abi.ABI_VERSION                 # additive: the ABI number stays
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(x=p, chains=4, stride=10, dim=3, t0=0, n=10, first=0, per=2, n_out=p, mean=p, m2=p):
        return lib.lmc_diag_cross_moments(x, chains, stride, dim, t0, n, first, per, n_out, mean, m2, None)

    for kw in (dict(x=None), dict(n_out=None), dict(mean=None), dict(m2=None), dict(chains=0), dict(dim=0), dict(n=0),
               dict(t0=-1), dict(t0=1), dict(n=11), dict(first=-1), dict(per=0), dict(dim=_abi.CROSS_MAX_DIM + 1),
               dict(chains=2 ** 31), dict(first=2 ** 31 - 4), dict(first=2 ** 62)):
        assert call(**kw) == 1, kw   # LMC_ERR_INVALID


@pytest.mark.parametrize("sizes", CUTS)
def test_merge_over_blocks_against_the_model(sizes):
    """The 6-chain, 3-group job cut four ways with the model as the kernel: every group within the merged bound of its parts,
    folded in job order; the uncut job gives the model's own bits."""
    x = _draws()
    got = dg.cross_moments(_cut(torch.from_numpy(x), sizes), chains_per_group=PER, moments_fn=M.moments_fn)
    assert tuple(got["n"].shape) == (3,) and tuple(got["mean"].shape) == (3, 5) and tuple(got["m2"].shape) == (3, 5, 5)
    want = [M.zero_part(5) for _ in range(3)]
    lo = 0
    for s in sizes:
        if s:
            g0, _k = M.touched(lo, s, PER)
            for i, p in enumerate(M.moments(x[lo:lo + s], lo, PER)):
                want[g0 + i] = M.merge_tolerance(want[g0 + i], p)
        lo += s
    M.check(got["n"].numpy(), got["mean"].numpy(), got["m2"].numpy(), want, "cut %s" % (sizes,))
    whole = M.moments(x, 0, PER)
    for g in range(3):   # the merged exact moments are the whole group's
        np.testing.assert_allclose(want[g]["m2"].astype("d"), whole[g]["m2"].astype("d"), rtol=1e-13)
        np.testing.assert_array_equal(got["m2"][g].numpy(), got["m2"][g].numpy().T)
    if sizes == [6]:
        ref = M.moments_fn(torch.from_numpy(x), 0, PER)
        for k in ("n", "mean", "m2"):
            np.testing.assert_array_equal(got[k].numpy(), ref[k].numpy())


def test_a_block_that_starts_inside_a_group_and_the_ungrouped_form():
    x = _draws()
    got = dg.cross_moments(torch.from_numpy(x[1:6]), chains_per_group=PER, first_chain=1, moments_fn=M.moments_fn)
    M.check(got["n"].numpy(), got["mean"].numpy(), got["m2"].numpy(), M.moments(x[1:6], 1, PER), "first_chain 1")
    assert got["n"].tolist() == [23.0, 46.0, 46.0]
    one = dg.cross_moments(torch.from_numpy(x), moments_fn=M.moments_fn)
    assert tuple(one["mean"].shape) == (5,) and tuple(one["m2"].shape) == (5, 5) and one["n"].dim() == 0
    b = T.Batched([T.AR1(5, rho=r) for r in (0.1, 0.2, 0.3)])
    grouped = dg.cross_moments(torch.from_numpy(x), target=b, moments_fn=M.moments_fn)
    assert tuple(grouped["m2"].shape) == (3, 5, 5)
    bc = b.covariance(torch.from_numpy(x), moments_fn=M.moments_fn)
    np.testing.assert_array_equal(bc["m2"].numpy(), grouped["m2"].numpy())


def test_zeros_are_the_identity_of_the_merge_bit_for_bit():
    x = _draws()
    a = M.moments_fn(torch.from_numpy(x), 0, PER)
    a["mean"][1, 2] = -0.0                              # a negative zero survives
    junk = {"n": torch.zeros(3, dtype=torch.float64), "mean": torch.full((3, 5), float("nan"), dtype=torch.float64),
            "m2": torch.full((3, 5, 5), float("inf"), dtype=torch.float64)}
    zero = {"n": torch.zeros(3, dtype=torch.float64), "mean": torch.zeros((3, 5), dtype=torch.float64),
            "m2": torch.zeros((3, 5, 5), dtype=torch.float64)}
    for empty in (zero, junk):   # skipped by its count, whatever it holds
        for got in (dg.merge_cross_moments(a, empty), dg.merge_cross_moments(empty, a)):
            for k in ("n", "mean", "m2"):
                np.testing.assert_array_equal(got[k].numpy().view(np.uint64), a[k].numpy().view(np.uint64), err_msg=k)
    both = dg.merge_cross_moments(zero, zero)
    assert not both["n"].any() and not both["mean"].any() and not both["m2"].any()
    # one side empty in one group only
    part = {k: v.clone() for k, v in a.items()}
    part["n"][0] = 0.0
    got = dg.merge_cross_moments(part, a)
    np.testing.assert_array_equal(got["m2"][0].numpy(), a["m2"][0].numpy())
    assert got["n"].tolist() == [46.0, 92.0, 92.0]


@pytest.mark.parametrize("ddof", [0, 1])
def test_covariance_and_contrasts_against_numpy(ddof):
    x = _draws(seed=11)
    xt = torch.from_numpy(x)
    c = dg.covariance(xt, chains_per_group=PER, ddof=ddof, moments_fn=M.moments_fn)
    L = np.array([[1.0, 0, -1, 0, 0], [0.5, 0.5, 0, 0, -1.0]])
    k = dg.contrasts(c, L, ddof=ddof)
    km = dg.contrasts(dg.cross_moments(xt, chains_per_group=PER, moments_fn=M.moments_fn), torch.from_numpy(L).expand(3, 2, 5),
                      ddof=ddof)
    for g in range(3):
        rows = x[2 * g:2 * g + 2].reshape(-1, 5)
        cov = np.cov(rows, rowvar=False, ddof=ddof)
        np.testing.assert_allclose(c["cov"][g].numpy(), cov, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(c["corr"][g].numpy(), np.corrcoef(rows, rowvar=False), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(c["sd"][g].numpy(), rows.std(axis=0, ddof=ddof), rtol=1e-12)
        np.testing.assert_allclose(c["mean"][g].numpy(), rows.mean(axis=0), rtol=1e-12)
        assert (np.diag(c["corr"][g].numpy()) == 1.0).all()
        for got in (k, km):
            np.testing.assert_allclose(got["cov"][g].numpy(), L @ cov @ L.T, rtol=1e-12, atol=1e-14)
            np.testing.assert_allclose(got["sd"][g].numpy(), np.sqrt(np.diag(L @ cov @ L.T)), rtol=1e-12)
            np.testing.assert_allclose(got["mean"][g].numpy(), L @ rows.mean(axis=0), rtol=1e-12)
    assert c["n"].tolist() == [46.0] * 3
    one = dg.covariance(xt, ddof=ddof, moments_fn=M.moments_fn)       # ungrouped: no leading axis, and the contrasts follow
    np.testing.assert_allclose(one["cov"].numpy(), np.cov(x.reshape(-1, 5), rowvar=False, ddof=ddof), rtol=1e-12)
    k1 = dg.contrasts(one, L)
    assert tuple(k1["mean"].shape) == (2,) and tuple(k1["cov"].shape) == (2, 2)
    with pytest.raises(ValueError, match="L must be"):
        dg.contrasts(c, np.ones((2, 4)))


def test_one_draw_and_a_constant_column():
    xt = torch.from_numpy(_draws(chains=1, n=1))
    c = dg.covariance(xt, moments_fn=M.moments_fn)
    assert float(c["n"]) == 1.0 and torch.isnan(c["cov"]).all() and torch.isnan(c["corr"]).all() and torch.isnan(c["sd"]).all()
    np.testing.assert_array_equal(c["mean"].numpy(), xt[0, 0].numpy())
    assert not c["m2"].any()
    c0 = dg.covariance(xt, ddof=0, moments_fn=M.moments_fn)
    assert not c0["cov"].any() and torch.isnan(c0["corr"]).all()
    x = _draws(seed=5)
    x[:, :, 3] = 1.25
    c = dg.covariance(torch.from_numpy(x), moments_fn=M.moments_fn)
    corr = c["corr"].numpy()
    assert np.isnan(corr[3]).all() and np.isnan(corr[:, 3]).all()
    keep = [0, 1, 2, 4]
    assert np.isfinite(corr[np.ix_(keep, keep)]).all() and (np.diag(corr)[keep] == 1.0).all()
    assert (np.abs(corr[np.ix_(keep, keep)]) <= 1.0).all() and c["cov"][3, 3] == 0.0


def test_refusals_of_the_job():
    xt = torch.from_numpy(_draws())
    with pytest.raises(_abi.HipLibraryError, match="CPU tensor"):
        dg.cross_moments(xt)
    with pytest.raises(ValueError, match="chains_per_group must be >= 1"):
        dg.cross_moments(xt, chains_per_group=0, moments_fn=M.moments_fn)
    with pytest.raises(ValueError, match="first_chain >= 0"):
        dg.cross_moments(xt, chains_per_group=2, first_chain=-1, moments_fn=M.moments_fn)
    with pytest.raises(ValueError, match=r"\[chains, draws, d\]"):
        dg.cross_moments(xt[0], moments_fn=M.moments_fn)
    with pytest.raises(ValueError, match="differ in d"):
        dg.cross_moments([xt[:2], xt[2:, :, :3]], moments_fn=M.moments_fn)
    with pytest.raises(ValueError, match="different numbers of draws"):
        dg.cross_moments([xt[:2], xt[2:, :5]], moments_fn=M.moments_fn)
    with pytest.raises(ValueError, match="holds no chain"):
        dg.cross_moments(xt[:0], moments_fn=M.moments_fn)
    b = T.Batched([T.AR1(5, rho=r) for r in (0.1, 0.2, 0.3)])
    with pytest.raises(ValueError, match="needs chains_per_group"):
        dg.cross_moments(xt, first_chain=2, target=b, moments_fn=M.moments_fn)
    with pytest.raises(ValueError, match="reach group 3; the target has 3"):
        dg.cross_moments(xt, chains_per_group=2, first_chain=2, target=b, moments_fn=M.moments_fn)
    with pytest.raises(ValueError, match="multiple of 3 chains"):
        b.covariance(xt[:5], moments_fn=M.moments_fn)
    wide = torch.zeros((1, 2, _abi.CROSS_MAX_DIM + 1), dtype=torch.float64)
    with pytest.raises(ValueError, match="beyond the 512 dimensions"):
        dg._hip_cross_moments(wide, 0, 1)
