"""No-GPU checks of the posterior predictions at new X: the C entry point's export, declaration and refusals, the numpy model
of one lmc_glm_linpred call (tests/_linpred_model.py) against the 50-digit reference within the derived bounds -- on the
inputs of the GPU test -- and the host logic of littlemcmc_amd/predictive.py (linear_predictor, predict, merge_moments) with
the numpy models injected for the two HIP calls, against plain numpy."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from littlemcmc_amd import _abi, predictive
from littlemcmc_amd import targets as T
from tests import _glm_model as G
from tests import _linpred_model as M
from tests import _predictive_model as P
from tests import _select_model as SM
from tests.test_gpu_predictive import DRAW_COUNTS, SHAPES

KW = dict(linpred_fn=M.linpred_fn, count_fn=SM.count_fn)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_declared_and_bound():
    lib = _abi.load()
    assert "lmc_glm_linpred" in _abi.EXPORTED_SYMBOLS and hasattr(lib, "lmc_glm_linpred")
    header = open(os.path.join(ROOT, "include", "lmc_hip.h")).read()
    assert "int lmc_glm_linpred(const double* x, int64_t chains, int64_t draws_stride, int32_t dim, int64_t t0, int64_t n," in header
    assert lib.lmc_abi_version() == 9 and len(_abi._SIGNATURES["lmc_glm_linpred"][1]) == 16
    assert os.path.exists(os.path.join(ROOT, "littlemcmc_amd", "csrc", "lmc_linpred.hip"))


def test_refusals_before_any_hip_call():
    lib = _abi.load()
    buf = (ctypes.c_double * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    d, N = 3, 70                                   # npad = 128: two observation blocks
    row_len = T.glm_row_layout(N, d)["size"]

    def call(x=p, chains=4, stride=10, dim=d, t0=0, n=10, rows=p, row_len=row_len, n_rows=2, first=0, per=2, ob0=0, ob1=2,
             eta=p, stats=p):
        return lib.lmc_glm_linpred(x, chains, stride, dim, t0, n, rows, row_len, n_rows, first, per, ob0, ob1, eta, stats, None)

    refused = (
        dict(x=None), dict(rows=None), dict(eta=None, stats=None),                       # both outputs NULL
        dict(chains=0), dict(chains=2 ** 31), dict(dim=0), dict(n=0), dict(t0=-1), dict(t0=1), dict(first=-1),
        dict(first=2 ** 31), dict(per=0), dict(dim=_abi.GLM_MAX_DIM + 1), dict(row_len=row_len + 2), dict(row_len=8),
        dict(n_rows=1), dict(n_rows=0), dict(first=2),                                   # a touched group beyond the table
        dict(ob0=-1), dict(ob0=1, ob1=1), dict(ob0=2, ob1=1), dict(ob1=3),
        dict(chains=2 ** 20, per=2 ** 20, stride=2 ** 14, n=2 ** 14, ob1=1),             # chains n W = 2^40 elements
        dict(chains=2 ** 30, per=2 ** 30, n=1),                                          # 2^31 wavefronts
    )
    for kw in refused:
        assert call(**kw) == 1, kw   # LMC_ERR_INVALID
    if lib.lmc_device_count() == 0:
        # accepted arguments pass every refusal and fail at the header copy, the first HIP call: LMC_ERR_HIP, not INVALID.
        # (With a device the pointers would have to be real: test_gpu_linpred.py makes these calls there.)
        for kw in (dict(), dict(ob0=1, ob1=2), dict(eta=None), dict(stats=None),         # ob1 == npad / 64
                   dict(chains=2 ** 20, per=2 ** 20, stride=2 ** 14, n=2 ** 14 - 1, ob1=1)):
            assert call(**kw) == 2, kw


def _glm(N, d, lik):
    X, y, _Q = G.case(N, d, lik)
    return T.GLM(X, y, lik, prior_scale=G.PRIOR_SCALE, sigma=G.SIGMA)


@pytest.mark.parametrize("lik", G.LIKELIHOODS)
@pytest.mark.parametrize("N,d", SHAPES)
def test_numpy_model_within_bound_of_reference(N, d, lik):
    """The inputs of test_gpu_linpred.py: 3 chains, 17 rows apart, of 1, 7, 8, 9 and 17 draws."""
    count = P.CHAINS * P.MAX_DRAWS
    ref = M.case_reference(N, d, lik, count)
    full = torch.from_numpy(np.array(P.draws_of(N, d, lik, count)).reshape(P.CHAINS, P.MAX_DRAWS, d))
    tgt = _glm(N, d, lik)
    nob = (N + 63) // 64
    for n in DRAW_COUNTS:   # the model as the host wrapper hands it on: what the GPU test asks of the kernel
        eta, st = predictive.linear_predictor(full[:, :n], tgt, linpred_fn=M.linpred_fn)
        eta, stats = eta.numpy(), np.stack([st[k][0].numpy() for k in predictive.MOMENT_PLANES])
        idx = [c * P.MAX_DRAWS + t for c in range(P.CHAINS) for t in range(n)]
        what = "%s N=%d d=%d n=%d" % (lik, N, d, n)
        assert eta.shape == (P.CHAINS, n, 64 * nob) and not eta[:, :, N:].any()     # padding observations: eta = 0
        M.check_eta(eta[:, :, :N].reshape(-1, N), ref, idx, what)
        M.check_planes(stats[:, :N], ref, idx, what)


def _quantile_plan(S, probs):
    h = [p * (S - 1) for p in probs]
    lo = [int(math.floor(v)) for v in h]
    return np.array(lo), np.array([min(k + 1, S - 1) for k in lo]), np.array([a - b for a, b in zip(h, lo)]).reshape(-1, 1)


@pytest.mark.parametrize("lik", G.LIKELIHOODS)
def test_predict_against_plain_numpy(lik):
    rng = np.random.default_rng(31 + G.LIKELIHOODS.index(lik))
    N, d, n_new, chains, draws = 9, 3, 7, 4, 25
    X = rng.standard_normal((N, d))
    y = {"gaussian": rng.standard_normal(N), "poisson": rng.poisson(2.0, N).astype(float),
         "bernoulli": (rng.random(N) < 0.5).astype(float)}[lik]
    tgt = T.GLM(X, y, lik, prior_scale=1.5, sigma=0.7)
    Xn = rng.standard_normal((n_new, d))
    x = torch.from_numpy(0.5 * rng.standard_normal((chains, draws, d)))
    probs = (0.05, 0.5, 0.95, 0.0, 1.0, 0.3333)
    out = tgt.predict(x, Xn, probs=probs, **KW)
    S = chains * draws
    assert out["n"] == S and out["probs"] == list(probs)
    # the model's eta columns, sorted by numpy
    table = T.GLM(Xn, np.zeros(n_new), lik, prior_scale=1.5, sigma=0.7).params.reshape(1, -1)
    eta, stats = M.linpred(x.numpy(), table, 0, chains, 0, 1)
    pool = np.sort(eta.reshape(S, 64)[:, :n_new], axis=0)
    lo, hi, frac = _quantile_plan(S, probs)
    vlo, vhi = pool[lo], pool[hi]                                     # the order statistics: bit-equal
    got = out["eta_quantiles"].numpy()
    assert got.shape == (1, len(probs), n_new) and out["eta_quantiles"].dtype == torch.float64
    assert np.array_equal(got[0], vlo + (vhi - vlo) * frac)            # the same expression on the same bits
    assert np.array_equal(got[0][3], pool[0]) and np.array_equal(got[0][4], pool[-1])
    # numpy's own interpolation rounds differently by a few ulps of the two neighbours
    npq = np.quantile(eta.reshape(S, 64)[:, :n_new], probs, axis=0)
    assert (np.abs(got[0] - npq) <= 4 * M.U * np.maximum(np.abs(vlo), np.abs(vhi))).all()
    # mu_quantiles: the host's inverse link of the two neighbours, interpolated on the mu scale
    mlo, mhi = M.inverse_link(vlo, lik), M.inverse_link(vhi, lik)
    assert np.array_equal(out["mu_quantiles"].numpy()[0], mlo + (mhi - mlo) * frac)
    # the moments and the law of total variance
    st = stats[0][:, :n_new]
    evar, mvar = st[2] / (S - 1.0), st[4] / (S - 1.0)
    for key, want in (("eta_mean", st[1]), ("eta_sd", np.sqrt(evar)), ("mu_mean", st[3]), ("mu_sd", np.sqrt(mvar))):
        assert out[key].shape == (1, n_new) and np.array_equal(out[key].numpy()[0], want), key
    y_mean, y_var = {"bernoulli": (st[3], st[3] * (1.0 - st[3])), "poisson": (st[3], st[3] + mvar),
                     "gaussian": (st[1], 0.7 ** 2 + evar)}[lik]
    assert np.array_equal(out["y_mean"].numpy()[0], y_mean) and np.array_equal(out["y_var"].numpy()[0], y_var)
    assert (out["y_var"] > 0).all()
    # X_new=None: the training design; linear_predictor returns the model's own arrays
    e2, s2 = predictive.linear_predictor(x, tgt, linpred_fn=M.linpred_fn)
    e_tr, st_tr = M.linpred(x.numpy(), tgt.params.reshape(1, -1), 0, chains, 0, 1)
    assert np.array_equal(e2.numpy(), e_tr) and all(np.array_equal(s2[k][0].numpy(), st_tr[0][i])
                                                    for i, k in enumerate(predictive.MOMENT_PLANES))
    assert np.array_equal(tgt.predict(x, **KW)["eta_mean"].numpy()[0], st_tr[0][1][:N])
    # one draw per posterior: the sd is NaN, the quantiles are the draw
    one = tgt.predict(x[:1, :1], Xn, **KW)
    assert one["n"] == 1 and bool(torch.isnan(one["eta_sd"]).all()) and bool(torch.isnan(one["y_var"]).all()) == (lik != "bernoulli")
    assert torch.equal(one["eta_quantiles"][0, 0], one["eta_mean"][0])


def _batched(lik="poisson", G_=3, N=70, d=3):
    rng = np.random.default_rng(50)
    ms = []
    for g in range(G_):
        X = rng.standard_normal((N, d)) / 2.0
        y = rng.poisson(2.0, N).astype(float)
        ms.append(T.GLM(X, y, lik, prior_scale=1.0 + g, sigma=0.5 + g))
    return T.Batched(ms), [rng.standard_normal((N + 1, d)) / 2.0 for _ in range(G_)]


def _same(a, b, keys=None):
    for k in keys or [k for k in a if torch.is_tensor(a[k])]:
        assert torch.equal(a[k], b[k]), k


def test_groups_split_blocks_and_chunks():
    tgt, Xn = _batched()
    rng = np.random.default_rng(51)
    per, draws, n_new = 2, 9, 71
    job = 0.5 * rng.standard_normal((3 * per, draws, 3))
    x = torch.from_numpy(job)
    one = tgt.predict(x, Xn, **KW)
    assert one["eta_quantiles"].shape == (3, 3, n_new) and one["y_var"].shape == (3, n_new) and one["n"] == per * draws
    table = np.stack([T.GLM(Xn[g], np.zeros(n_new), "poisson", prior_scale=tgt[g].prior_scale, sigma=tgt[g].sigma).params
                      for g in range(3)])
    eta_all = M.linpred(job, table, 0, per, 0, 2)[0]
    refs = []
    for g in range(3):   # every group: its own X_new, its own chains
        q = job[per * g:per * g + per].reshape(-1, 3)
        pool = np.sort(eta_all[per * g:per * g + per].reshape(-1, 128)[:, :n_new], axis=0)
        lo, hi, frac = _quantile_plan(per * draws, (0.05, 0.5, 0.95))
        assert np.array_equal(one["eta_quantiles"][g].numpy(), pool[lo] + (pool[hi] - pool[lo]) * frac)
        refs.append(M.reference(Xn[g], q, "poisson", P.reference_loglik(Xn[g], np.zeros(n_new), q, "poisson")))
        val, bnd = M.reference_planes(refs[g])
        assert P.within(one["eta_mean"][g].numpy(), val[1], bnd[1] + M.U * np.abs(val[1])).all()
        assert P.within(one["mu_mean"][g].numpy(), val[3], bnd[3] + M.U * np.abs(val[3])).all()
    # a list of two blocks that cuts group 1: the select is exact (the same bits), the moments of group 1 are a merge of its
    # parts (within the bound), groups 0 and 2 lie inside one block either way (the same bits)
    two = tgt.predict([x[:3], x[3:]], Xn, **KW)
    _same(one, two, ("eta_quantiles", "mu_quantiles"))
    for k in ("eta_mean", "eta_sd", "mu_mean", "mu_sd", "y_mean", "y_var"):
        assert torch.equal(one[k][0], two[k][0]) and torch.equal(one[k][2], two[k][2]), k
    val, bnd = M.reference_planes(refs[1])
    assert P.within(two["eta_mean"][1].numpy(), val[1], bnd[1] + M.U * np.abs(val[1])).all()
    assert P.within(two["mu_mean"][1].numpy(), val[3], bnd[3] + M.U * np.abs(val[3])).all()
    # the merge itself, on the kernel's planes of the two parts of group 1 (job chains 2 and 3)
    a = M.linpred(job[2:3], table, 2, per, 0, 2)[1]
    b = M.linpred(job[3:4], table, 3, per, 0, 2)[1]
    merged = predictive.merge_moments(torch.from_numpy(a), torch.from_numpy(b)).numpy()
    M.check_planes(merged[0][:, :n_new], refs[1], what="merge of the parts of group 1")
    empty = np.zeros_like(a)
    junk = empty.copy()
    junk[:, 1:] = np.nan
    for e in (empty, junk):   # a side of count 0 is skipped by its count, whatever it holds
        for got in (predictive.merge_moments(torch.from_numpy(a), torch.from_numpy(e)),
                    predictive.merge_moments(torch.from_numpy(e), torch.from_numpy(a))):
            assert np.array_equal(got.numpy(), a)
    # scratch_bytes that forces one observation block per chunk: the same bits; one byte less: refused, the unit named
    unit = 3 * per * draws * 64 * 8
    lo, hi, _frac = _quantile_plan(per * draws, (0.05, 0.5, 0.95))
    counts = 256 * 64 * 8 * len({0, per * draws - 1} | set(lo.tolist()) | set(hi.tolist()))
    calls = []

    def counting(*a, **k):
        calls.append(a[4:6])
        return M.linpred_fn(*a, **k)

    chunked = tgt.predict(x, Xn, scratch_bytes=unit + counts, linpred_fn=counting, count_fn=SM.count_fn)
    assert calls == [(0, 1), (1, 2)]
    _same(one, chunked)
    with pytest.raises(ValueError, match="64 x 8 = %d bytes" % unit):
        tgt.predict(x, Xn, scratch_bytes=unit + counts - 1, **KW)


def test_x_new_is_validated_and_other_refusals(monkeypatch):
    tgt, Xn = _batched()
    x = torch.zeros((6, 4, 3), dtype=torch.float64)
    with pytest.raises(ValueError, match="list of 3 arrays"):
        tgt.predict(x, Xn[:2], **KW)
    with pytest.raises(ValueError, match="d = 4, the posterior d = 3"):
        tgt.predict(x, [Xn[0], np.zeros((71, 4)), Xn[2]], **KW)
    with pytest.raises(ValueError, match="one common N_new"):
        tgt.predict(x, [Xn[0], Xn[1][:70], Xn[2]], **KW)
    with pytest.raises(ValueError, match=r"\[N_new, d\]"):
        tgt[0].predict(x[:2], np.zeros(3), **KW)
    with pytest.raises(ValueError):                                   # GLM validates the design: no NaN
        tgt[0].predict(x[:2], np.full((4, 3), np.nan), **KW)
    with pytest.raises(ValueError, match="probs"):
        tgt.predict(x, Xn, probs=(1.5,), **KW)
    with pytest.raises(ValueError, match="x has d = 2"):
        tgt.predict(torch.zeros((6, 4, 2), dtype=torch.float64), Xn, **KW)
    with pytest.raises(ValueError, match="multiple of 3 chains"):
        tgt.predict(x[:5], Xn, **KW)
    with pytest.raises(TypeError):
        predictive.predict(x, T.StdNormal(3), **KW)
    with pytest.raises(ValueError, match="one tensor"):
        predictive.linear_predictor([x], tgt, linpred_fn=M.linpred_fn)
    with pytest.raises(ValueError, match="obs_blocks"):
        predictive.linear_predictor(x, tgt, Xn, obs_blocks=(1, 3), linpred_fn=M.linpred_fn)
    with pytest.raises(_abi.HipLibraryError):                         # no host implementation
        tgt.predict(x, Xn)
    with pytest.raises(_abi.HipLibraryError):
        predictive.linear_predictor(x, tgt, Xn)
    import torch.distributed as dist

    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    with pytest.raises(ValueError, match="process group"):
        tgt.predict(x, Xn, **KW)
    with pytest.raises(ValueError, match="process group"):
        predictive.linear_predictor(x, tgt, Xn, linpred_fn=M.linpred_fn)
