"""-m gpu: PSIS-LOO on the device. lmc_psis_rows (csrc/lmc_psis.hip) against the numpy model of tests/_psis_model.py on
identical rows -- the discrete outputs (n_tail, the cutoff's bits, min l) equal, elpd / k / sigma / ess_w within 16 x EPS_ROW
(EPS_ROW: the model's own rounding sensitivity against its 50-digit form, measured by test_psis_cpu.py; the device's math
functions are 1-2 ulp off numpy's and its sums run in another, equally good order) -- lmc_glm_pointwise_loglik against the
50-digit reference of tests/_predictive_model.py and against the planes of lmc_glm_pointwise, and predictive.loo() on top."""
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
from tests import _psis_model as M

pytestmark = pytest.mark.gpu

TOL = 16 * M.EPS_ROW
NAMES = ("elpd", "k", "n_tail", "ess_w", "sigma", "cutoff", "min_l")


def _device_rows(mat, Mt):
    """[rows, 7] in the model's order (elpd, k, n_tail, ess_w, sigma, cutoff, min l) from one call of lmc_psis_rows."""
    t = mat if torch.is_tensor(mat) else torch.from_numpy(np.array(mat)).cuda()   # (a copy: the shared rows are read-only)
    out = predictive._hip_psis(t, Mt).cpu().numpy()
    assert (out[:, 7] == 0.0).all()
    return out[:, [0, 1, 2, 4, 3, 5, 6]]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _check(got, want, what):
    """One row: got (device) against want (model), both in the model's order."""
    print("%s: device %r\n%s  model %r" % (what, tuple(got), " " * len(what), tuple(want)))
    assert got[2] == want[2], "%s: n_tail %r, model %r" % (what, got[2], want[2])
    for i in (5, 6):   # the cutoff and min l: the same bits (NaN for a non-finite row)
        assert (np.isnan(got[i]) and np.isnan(want[i])) or _bits(got[i]) == _bits(want[i]), (what, NAMES[i], got[i], want[i])
    for i in (0, 1, 3, 4):
        g, w = got[i], want[i]
        if not np.isfinite(w):
            assert (np.isnan(g) and np.isnan(w)) or g == w, (what, NAMES[i], g, w)
            continue
        bound = TOL * (abs(w) + 1.0) if i == 0 else TOL * abs(w)
        assert abs(g - w) <= bound, "%s: %s device %r, model %r: off by %.3e, bound %.3e" % (what, NAMES[i], g, w, abs(g - w), bound)


@pytest.mark.parametrize("kind", M.KINDS)
def test_rows_against_the_model(kind):
    for S in M.ROW_SIZES:
        r = M.row(kind, S)
        Mt = M.tail_len(S)
        _check(_device_rows(r.reshape(1, S), Mt)[0], M.psis_row(r, M=Mt, full=True), "%s S=%d" % (kind, S))


def test_the_longest_row_just_under_the_lds_limit():
    r = M.row("gaussian", M.BIG_S)
    Mt = M.tail_len(M.BIG_S)
    assert Mt == 4092 <= _abi.PSIS_MAX_TAIL
    got = _device_rows(r.reshape(1, -1), Mt)[0]
    _check(got, M.psis_row(r, M=Mt, full=True), "gaussian S=%d" % M.BIG_S)
    assert got[2] == 4092


def test_row_stride_and_nothing_read_past_a_row():
    """Three rows of 257 and of 1000 values inside a wider buffer whose slack is +inf: a read past a row would make it
    non-finite (NaN outputs); the strided call equals the contiguous one bit for bit."""
    for S in (257, 1000):
        rows = np.stack([M.row(kind, S) for kind in M.KINDS])
        wide = torch.full((3, S + 37), float("inf"), dtype=torch.float64, device="cuda")
        wide[:, :S] = torch.from_numpy(rows).cuda()
        view = wide[:, :S]
        assert not view.is_contiguous() and view.stride(0) == S + 37
        got, want = _device_rows(view, M.tail_len(S)), _device_rows(rows, M.tail_len(S))
        assert np.isfinite(got[:, 0]).all() and np.array_equal(_bits(got), _bits(want))
        out = predictive.psis(view)
        assert np.array_equal(_bits(out["elpd_i"].cpu().numpy()), _bits(want[:, 0]))
        assert np.array_equal(_bits(out["pareto_k"].cpu().numpy()), _bits(want[:, 1]))


def test_edge_rows_in_one_call_and_their_neighbours():
    named = M.edge_rows()
    mat = np.stack([r for _n, r in named])
    Mt = M.tail_len(mat.shape[1])
    got = _device_rows(mat, Mt)
    for (name, r), g in zip(named, got):
        _check(g, M.psis_row(r, M=Mt, full=True), name)
    by = {name: g for (name, _r), g in zip(named, got)}
    assert by["constant"][0] == -1.3 and by["constant"][2] == 0 and by["constant"][3] == mat.shape[1]
    assert by["clamped"][5] == M.LOG_TINY and by["clamped"][2] == 1
    assert 4 < by["tied"][2] < Mt
    assert np.isnan(by["nan"][[0, 1, 3, 4, 5, 6]]).all() and np.isnan(by["minus_inf"][[0, 1, 3, 4, 5]]).all()
    assert by["minus_inf"][6] == -np.inf and by["nan"][2] == 0 and by["minus_inf"][2] == 0
    # the neighbours of the bad rows: the bits they have in a call without them
    plain = [i for i, (name, _r) in enumerate(named) if name.startswith("plain")]
    alone = _device_rows(mat[plain], Mt)
    assert np.array_equal(_bits(got[plain]), _bits(alone))
    assert np.array_equal(_bits(_device_rows(mat, Mt)), _bits(got))   # two calls: the same bits (NaN payloads included)


# ---- lmc_glm_pointwise_loglik ------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (63, 3), (65, 65), (70, 300))
CHAINS, DRAWS = P.CHAINS, 9   # 9 draws: one whole tile of T = 8 and a tail of one
assert DRAWS % P.T != 0 and DRAWS > P.T


def _glm(N, d, lik):
    X, y, _Q = G.case(N, d, lik)
    return T.GLM(X, y, lik, prior_scale=G.PRIOR_SCALE, sigma=G.SIGMA)


@pytest.mark.parametrize("lik", G.LIKELIHOODS)
@pytest.mark.parametrize("N,d", SHAPES)
def test_loglik_within_bound_of_reference_and_the_bits_of_the_planes(N, d, lik):
    """3 chains x 9 draws, the leading draws of a [3, 17, d] tensor: chains lie 17 rows apart in x and 9 apart in a row."""
    tgt = _glm(N, d, lik)
    count = P.CHAINS * P.MAX_DRAWS
    ref = P.case_reference(N, d, lik, count)
    full = torch.from_numpy(np.array(P.draws_of(N, d, lik, count)).reshape(P.CHAINS, P.MAX_DRAWS, d)).cuda()
    x = full[:, :DRAWS]
    ll = predictive.pointwise_loglik(x, tgt)
    npad = (N + 63) // 64 * 64
    assert ll.shape == (1, npad, CHAINS * DRAWS) and ll.is_cuda and bool(torch.isfinite(ll[0, N:]).all())
    got = ll[0, :N].cpu().numpy()
    for c in range(CHAINS):
        for t in range(DRAWS):
            s_ref, s = c * P.MAX_DRAWS + t, c * DRAWS + t
            val = np.array([float(v) for v in ref["l"][s_ref]])
            # the bound of _predictive_model is relative (u |l|): a subnormal l (-1e-318 at |eta| = 800) is rounded to the
            # subnormal spacing 2^-1074 instead, once per operation of the link, and once more in the reference's float()
            ok = P.within(got[:, s], val, ref["dl"][s_ref] + 2 * P.U * np.abs(np.where(np.isfinite(val), val, 0.0)) + 8 * 2.0 ** -1074)
            assert ok.all(), "%s N=%d d=%d chain %d draw %d: got %r, reference %r, bound %r" % (
                lik, N, d, c, t, got[~ok, s][:4], val[~ok][:4], ref["dl"][s_ref][~ok][:4])
    st = tgt.pointwise_stats(x)
    assert torch.equal(ll[:, :N].max(dim=-1).values, st["m"])   # one tile function: the bits the planes were reduced from


def test_loglik_observation_block_range_strided_x_and_refusals():
    N, d = 130, 3
    tgt = _glm(N, d, "bernoulli")
    chains, n = 4, P.T + 1
    draws = torch.from_numpy(np.array(P.draws_of(N, d, "bernoulli", chains * n)).reshape(chains, n, d))
    # x embedded in an inf-filled buffer, chain stride larger than n d: a read of a padded coefficient or of a row too many shows
    slack = 1024
    flat = torch.full((slack + chains * (n + 3) * d + slack,), float("inf"), dtype=torch.float64, device="cuda")
    big = flat[slack:slack + chains * (n + 3) * d].view(chains, n + 3, d)
    big[:, :n] = draws.cuda()
    x = big[:, :n]
    assert not x.is_contiguous() and dg._row_major(x)
    full = predictive.pointwise_loglik(x, tgt)
    assert full.shape == (1, 192, chains * n) and bool(torch.isfinite(full).all())
    assert torch.equal(full, predictive.pointwise_loglik(x.contiguous(), tgt))
    part = predictive.pointwise_loglik(x, tgt, obs_blocks=(1, 2))
    assert part.shape == (1, 64, chains * n) and torch.equal(part, full[:, 64:128])
    # two groups of two chains (a Batched of the same model twice): group g holds chains 2 g, 2 g + 1
    two = T.Batched([tgt, tgt])
    both = predictive.pointwise_loglik(x, two)
    assert both.shape == (2, 192, 2 * n)
    assert torch.equal(both[0], full[0, :, :2 * n]) and torch.equal(both[1], full[0, :, 2 * n:])
    assert torch.equal(predictive.pointwise_loglik(x, two, groups=(1, 2)), both[1:])
    # the whole-group refusals, with real device pointers
    lib = _abi.load()
    xc = x.contiguous()
    table = torch.from_numpy(np.ascontiguousarray(two.params).reshape(2, -1)).cuda()
    out = torch.zeros((2, 192, 2 * n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def call(c, first, per):
        return lib.lmc_glm_pointwise_loglik(ctypes.c_void_p(xc.data_ptr()), c, n, d, 0, n, ctypes.c_void_p(table.data_ptr()),
                                            table.shape[1], 2, first, per, 0, 3, ctypes.c_void_p(out.data_ptr()), None)

    assert call(4, 0, 2) == _abi.OK
    assert call(3, 0, 2) == 1 and call(2, 1, 2) == 1 and call(4, 0, 3) == 1 and call(4, 2, 2) == 1   # LMC_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(out, both)


# ---- predictive.loo ------------------------------------------------------------------------------------------------------------
def _three_groups(N=65, d=5, lik="bernoulli"):
    ms = []
    for g in range(3):
        rng = np.random.default_rng(900 + g)
        X = rng.standard_normal((N, d)) / np.sqrt(d)
        y = (rng.random(N) < 0.5).astype(np.float64)
        ms.append(T.GLM(X, y, lik, prior_scale=1.0 + g))
    return T.Batched(ms)


def _equal_bits(a, b):
    return all(np.array_equal(_bits(a[k].cpu().numpy().astype(np.float64)), _bits(b[k].cpu().numpy().astype(np.float64))) for k in a)


def test_loo_of_three_groups_model_chunks_and_bits():
    tgt = _three_groups()
    N, S = 65, 3 * 11
    x = torch.from_numpy(np.random.default_rng(12).standard_normal((9, 11, 5))).cuda()
    out = tgt.loo(x)
    ll = predictive.pointwise_loglik(x, tgt).cpu().numpy()
    assert ll.shape == (3, 128, S)
    Mt = M.tail_len(S)
    for g in range(3):
        want = M.model_rows(ll[g, :N], Mt)
        got = np.stack([(out["elpd_loo_i"][g].cpu().numpy() - tgt[g].loglik_constant()), out["pareto_k"][g].cpu().numpy(),
                        out["n_tail"][g].cpu().numpy(), out["ess_w"][g].cpu().numpy()], axis=1)
        assert np.array_equal(got[:, 2], want[:, 2])
        for i in (0, 1, 3):
            bound = TOL * (np.abs(want[:, i]) + (1.0 if i == 0 else 0.0))
            fin = np.isfinite(want[:, i])
            assert (np.abs(got[fin, i] - want[fin, i]) <= bound[fin]).all(), (g, NAMES[i])
            assert np.array_equal(got[~fin, i], want[~fin, i])
    unit = 64 * S * 8
    assert _equal_bits(tgt.loo(x, scratch_bytes=unit), out)       # one group and one observation block per chunk
    assert _equal_bits(tgt.loo(x, scratch_bytes=5 * unit), out)   # two groups, then one
    assert _equal_bits(tgt.loo(x), out)                           # two calls
    w = tgt.waic(x)
    assert all(torch.equal(out[k], w[k]) for k in w)
    assert out["elpd_loo"].shape == (3,) and out["n_bad_k"].shape == (3,) and out["pareto_k"].is_cuda


def test_end_to_end_prior_scale_ladder():
    """The job of test_gpu_predictive.py's ladder (4 gaussian GLMs along the prior scales, 64 chains, 200 + 200 draws):
    elpd_loo_i equals the model applied to the returned host trace, elpd_loo lies within 5 sd (inflated by sqrt(S / ess_min))
    of the exact leave-one-out sum and not above elpd_waic by more than that band, every k is finite, the 0.1 rung is the
    worst."""
    X, y, _Xn, _yn, sigma = P.ladder()
    tgt = T.Batched([T.GLM(X, y, "gaussian", prior_scale=s, sigma=sigma) for s in P.LADDER_SCALES])
    trace, stats, eng = lmc.sample(tgt, tgt.d, chains=4 * 16, draws=200, tune=200, random_seed=11, progressbar=False,
                                   return_engine=True)
    try:
        x = dg.trace_tensor(eng)
        out = {k: v.cpu().numpy() for k, v in tgt.loo(x).items() if torch.is_tensor(v)}
        ess_min = tgt.summarize(x)["ess_min"].cpu().numpy()
    finally:
        eng.close()
    S = 16 * 200
    assert out["elpd_loo_i"].shape == (4, 32) and np.isfinite(out["pareto_k"]).all() and not stats["diverging"].any()
    for g, sl in enumerate(tgt.chain_slices(64)):
        const = tgt[g].loglik_constant()
        ll = -0.5 * (y - trace[sl].reshape(-1, 4) @ X.T) ** 2 / sigma ** 2
        want = np.array([M.psis_row(ll[:, n])[0] for n in range(32)]) + const
        print("group %d: ess_min %.0f, largest k %.3f, max |elpd_loo_i - model| %.3e, elpd_loo %.4f, exact %.4f, elpd_waic %.4f"
              % (g, ess_min[g], out["pareto_k"][g].max(), np.abs(out["elpd_loo_i"][g] - want).max(), out["elpd_loo"][g],
                 M.exact_loo(tgt[g]).sum(), out["elpd_waic"][g]))
        assert (np.abs(out["elpd_loo_i"][g] - want) <= 1e-9).all(), g
        band = 5 * M.SD_TOTAL * np.sqrt(S / ess_min[g])
        assert S == M.SD_DRAWS and abs(out["elpd_loo"][g] - M.exact_loo(tgt[g]).sum()) <= band, g
        assert out["elpd_loo"][g] <= out["elpd_waic"][g] + band, g
    assert np.argmin(out["elpd_loo"]) == 0, out["elpd_loo"]
