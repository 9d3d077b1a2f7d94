"""-m gpu: lmc_glm_yrep and lmc_glm_yrep_stats (csrc/lmc_yrep.hip, csrc/lmc_yrep.hpp) -- the replicated responses of every draw
as an array, and their test statistics per draw without the array -- against the Python model of the stream and the samplers
(tests/_yrep_model.py) evaluated on the device's own eta, and littlemcmc_amd/predictive.py (replicate, predict_response, ppc)
on top of them. Tensors are made with torch; no test runs a sampler. The model's values of a cell are computed once."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from littlemcmc_amd import _abi, predictive
from littlemcmc_amd import diagnostics as dg
from littlemcmc_amd import targets as T
from tests import _yrep_model as Y
from tests.test_gpu_predictive import _three_groups

pytestmark = pytest.mark.gpu

GUARD = -7.25   # what the guard elements around an output hold
U = Y.U


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _guarded(shape, guard):
    size = int(np.prod(shape))
    flat = torch.full((guard + size + guard,), GUARD, dtype=torch.float64, device="cuda")
    return flat[guard:guard + size].view(*shape), flat


def _raw_yrep(x, table, first, per, ob0, ob1, seed, guard=0, t0=0, n=None):
    """One call of lmc_glm_yrep between guard elements: (y[c, n, W], the guarded buffer)."""
    c, rows, d = x.shape
    n = rows if n is None else n
    y, flat = _guarded((c, n, 64 * (ob1 - ob0)), guard)
    torch.cuda.synchronize()
    rc = _abi.load().lmc_glm_yrep(_ptr(x), c, x.stride(0) // d if c > 1 else rows, d, t0, n, _ptr(table), table.shape[1],
                                  table.shape[0], first, per, ob0, ob1, seed, _ptr(y), None)
    torch.cuda.synchronize()
    assert rc == _abi.OK, rc
    return y, flat


def _raw_stats(x, table, first, per, seed, centre, guard=0, t0=0, n=None):
    """One call of lmc_glm_yrep_stats between guard elements: (T[c, n, 7], the guarded buffer)."""
    c, rows, d = x.shape
    n = rows if n is None else n
    Tt, flat = _guarded((c, n, Y.STATS), guard)
    torch.cuda.synchronize()
    rc = _abi.load().lmc_glm_yrep_stats(_ptr(x), c, x.stride(0) // d if c > 1 else rows, d, t0, n, _ptr(table), table.shape[1],
                                        table.shape[0], first, per, seed, _ptr(centre), _ptr(Tt), None)
    torch.cuda.synchronize()
    assert rc == _abi.OK, rc
    return Tt, flat


def _same(a, b):
    """Bit for bit, a NaN equal to a NaN."""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@functools.lru_cache(maxsize=None)
def _on_device(name):
    """The cell on the device, once: target, draws, table, the device's eta and mu of every (chain, draw, observation), the
    array kernel's y_rep, and the model's (value, decided) on that eta."""
    c = Y.cell(name)
    tgt = Y.target_of(c)
    x = torch.from_numpy(c["x"]).cuda()
    table_np = Y.table_of(c)
    table = torch.from_numpy(table_np).cuda()
    chains, n, d = x.shape
    nob = (c["N"] + 63) // 64
    eta, _st = predictive.linear_predictor(x, tgt)
    # the device's own mu, bit for bit: every draw as a chain and a group of its own (its row repeated) -- the mean of one mu
    rows = table[(torch.arange(chains * n, device="cuda") // n) // c["per"]].contiguous()
    _e, st = predictive._hip_linpred(x.reshape(chains * n, 1, d), rows, 0, 1, 0, nob, want_eta=False)
    mu = st[:, 3].reshape(chains, n, 64 * nob)
    y = tgt.replicate(x, random_seed=Y.SEED)
    centre = np.array([m[1].sum() / c["N"] for m in c["members"]])
    eta_np = eta.cpu().numpy()
    model, decided = Y.yrep(eta_np, table_np, 0, c["per"], 0, Y.SEED)
    return dict(c=c, tgt=tgt, x=x, table=table, table_np=table_np, eta=eta_np, mu=mu.cpu().numpy(), y=y, y_np=y.cpu().numpy(),
                centre=centre, model=model, decided=decided, nob=nob)


@pytest.mark.parametrize("name", Y.CELLS)
def test_array_kernel_equals_the_model_on_the_devices_eta(name):
    """Every decided element: counts exactly, gaussian within 8 E_z sigma + 2 u |y|; at most MAX_UNDECIDED are undecided."""
    D = _on_device(name)
    c, y, model, decided = D["c"], D["y_np"], D["model"], D["decided"]
    N = c["N"]
    assert D["y"].shape == (c["G"] * c["per"], c["n"], 64 * D["nob"]) and D["y"].is_cuda
    assert not y[:, :, N:].any()                                                    # padding observations hold 0
    undecided = int((~decided).sum())
    print("%s: %d elements, %d undecided" % (name, y[:, :, :N].size, undecided))
    assert undecided <= Y.MAX_UNDECIDED
    if c["lik"] == "gaussian":
        sigma = np.array([m[3] for m in c["members"]]).repeat(c["per"]).reshape(-1, 1, 1)
        err = np.abs(y - model)[:, :, :N]
        tol = (8.0 * Y.E_Z * sigma + 2.0 * U * np.abs(model))[:, :, :N]
        print("gaussian: worst error / tolerance = %.3g" % (err / tol).max())
        assert (err <= tol).all()
    else:
        ok = np.where(decided, (y == model) | (np.isnan(y) & np.isnan(model)), True)
        assert ok.all(), (np.argwhere(~ok)[:4], y[~ok][:4], model[~ok][:4])
        assert (np.isnan(y) | (y == np.floor(y))).all() and not (y < 0).any()
    if name == "poisson":
        assert (y[:, :, 68] == 0.0).all() and np.isnan(y[:, :, 69]).all() and not np.isnan(y[:, :, :69]).any()
        assert np.nanmax(y) > 5e5 and (D["mu"][:, :, :68] < 10.0).sum() > 100 and (D["mu"][:, :, :68] > 10.0).sum() > 100


def _reduce(y, mu, yobs, lik, isig2, centre):
    """(T_ref[..., 7], tol[..., 7]) from the array kernel's own y[..., N] and the device's mu: the terms are formed in numpy as
    the device forms them (one rounding an operation), so only the order of the sums differs: (N + 2) u sum |terms|."""
    N = y.shape[-1]
    ref = Y.stats_of(y, mu, yobs, lik, isig2, centre)
    with np.errstate(all="ignore"):
        mag = np.stack([np.abs(y).sum(axis=-1), ref[..., 1], 0 * ref[..., 2], 0 * ref[..., 3], 0 * ref[..., 4], ref[..., 5],
                        ref[..., 6]], axis=-1)
    return ref, (N + 2) * U * mag


def _check_stats(Tt, ref, tol, counts, what):
    for p in (2, 3, 4) + ((0,) if counts else ()):
        assert _same(Tt[..., p], ref[..., p]), "%s plane %d" % (what, p)
    for p in (0, 1, 5, 6):
        nan = np.isnan(ref[..., p])
        assert np.array_equal(np.isnan(Tt[..., p]), nan), "%s plane %d: NaN pattern" % (what, p)
        with np.errstate(invalid="ignore"):
            ok = nan | (np.abs(Tt[..., p] - ref[..., p]) <= tol[..., p]) | (Tt[..., p] == ref[..., p])
        assert ok.all(), "%s plane %d: %r vs %r, tolerance %r" % (what, p, Tt[..., p][~ok][:3], ref[..., p][~ok][:3], tol[..., p][~ok][:3])


@pytest.mark.parametrize("name", Y.CELLS)
def test_stats_kernel_equals_reductions_of_the_array_kernels_output(name):
    D = _on_device(name)
    c = D["c"]
    N, per = c["N"], c["per"]
    Tt, _flat = _raw_stats(D["x"], D["table"], 0, per, Y.SEED, torch.from_numpy(D["centre"]).cuda())
    Tt = Tt.cpu().numpy()
    for g, (X, yobs, _ps, sg) in enumerate(c["members"]):
        sl = slice(per * g, per * g + per)
        ref, tol = _reduce(D["y_np"][sl][:, :, :N], D["mu"][sl][:, :, :N], yobs, c["lik"], sg ** -2, D["centre"][g])
        _check_stats(Tt[sl], ref, tol, c["lik"] != "gaussian", "%s group %d" % (name, g))
    if name == "poisson":
        # observation 69 (mu = +inf, y_rep = NaN) makes the planes it enters NaN in every draw and leaves the zeros alone ...
        assert np.isnan(Tt[..., [0, 1, 2, 3, 5, 6]]).all() and np.isfinite(Tt[..., 4]).all()
        # ... so the numbers are held on the rows of the first 69 and 68 observations: the same y_rep (a value depends on its
        # observation's index, not on N). With 69 the eta = -800 observation is in: mu = 0 = V, both Pearson terms are 0 / 0
        # and planes 5 and 6 alone are NaN; with 68 every plane is finite
        for M in (69, 68):
            ms = [T.GLM(X[:M], yobs[:M], "poisson", prior_scale=ps, sigma=sg) for X, yobs, ps, sg in c["members"]]
            centre = np.array([m.y.sum() / M for m in ms])
            TM, _flat = _raw_stats(D["x"], torch.from_numpy(T.Batched(ms).params.reshape(3, -1)).cuda(), 0, per, Y.SEED,
                                   torch.from_numpy(centre).cuda())
            TM = TM.cpu().numpy()
            assert np.isfinite(TM[..., :5]).all() and np.isnan(TM[..., 5:]).all() == (M == 69) == (not np.isfinite(TM[..., 5:]).any())
            for g, m in enumerate(ms):
                sl = slice(per * g, per * g + per)
                ref, tol = _reduce(D["y_np"][sl][:, :, :M], D["mu"][sl][:, :, :M], m.y, "poisson", m.isig2, centre[g])
                _check_stats(TM[sl], ref, tol, True, "poisson, %d observations, group %d" % (M, g))


@pytest.mark.parametrize("name", ["bernoulli", "poisson"])
def test_values_do_not_depend_on_the_shape_of_the_call(name):
    D = _on_device(name)
    c, x, table, tgt, y = D["c"], D["x"], D["table"], D["tgt"], D["y"]
    per, nob, n = c["per"], D["nob"], c["n"]
    centre = torch.from_numpy(D["centre"]).cuda()
    Tt, _f = _raw_stats(x, table, 0, per, Y.SEED, centre)
    # a sub-range of observation blocks
    for ob0, ob1 in ((nob - 1, nob), (0, 1), (1, nob)):
        if ob0 < ob1:
            assert _same(tgt.replicate(x, random_seed=Y.SEED, obs_blocks=(ob0, ob1)).cpu(), y[:, :, 64 * ob0:64 * ob1].cpu())
    # a block of chains at its first_chain (cut inside groups), a sub-series of draws at its t0
    lo, hi = 1, x.shape[0] - 1
    part, _f = _raw_yrep(x[lo:hi], table, lo, per, 0, nob, Y.SEED)
    assert _same(part.cpu(), y[lo:hi].cpu())
    part, _f = _raw_stats(x[lo:hi], table, lo, per, Y.SEED, centre)
    assert _same(part.cpu(), Tt[lo:hi].cpu())
    t0, m = 3, n - 4
    part, _f = _raw_yrep(x, table, 0, per, 0, nob, Y.SEED, t0=t0, n=m)
    assert _same(part.cpu(), y[:, t0:t0 + m].cpu())
    part, _f = _raw_stats(x, table, 0, per, Y.SEED, centre, t0=t0, n=m)
    assert _same(part.cpu(), Tt[:, t0:t0 + m].cpu())
    # two calls on one seed: the same bits; another seed: other values
    again, _f = _raw_yrep(x, table, 0, per, 0, nob, Y.SEED)
    T2, _f = _raw_stats(x, table, 0, per, Y.SEED, centre)
    assert _same(again.cpu(), y.cpu()) and _same(T2.cpu(), Tt.cpu())
    other, _f = _raw_yrep(x, table, 0, per, 0, nob, Y.SEED + 1)
    assert not _same(other.cpu(), y.cpu())
    frac = float((other[:, :, :c["N"]] != y[:, :, :c["N"]]).double().mean())
    print("%s: another seed changes %.0f %% of the elements" % (name, 100 * frac))
    assert frac > 0.1


@pytest.mark.parametrize("lik,N,d", [("bernoulli", 63, 3), ("poisson", 65, 65)])
def test_addressing_reads_and_writes_nothing_too_many(lik, N, d):
    """x = big[:, :n] with big[:, n:] = inf and the chain stride larger than n d, inside a buffer whose slack is inf; the
    one-row table and the centre inside buffers of inf: a kernel that reads a padded coefficient, a row of the trace or of the
    table too many differs from the call on clean copies. The outputs lie between guard elements."""
    rng = np.random.default_rng(3 + d)
    X = rng.standard_normal((N, d)) / np.sqrt(d)
    yobs = (rng.random(N) < 0.5).astype(np.float64) if lik == "bernoulli" else rng.poisson(2.0, N).astype(np.float64)
    tgt = T.GLM(X, yobs, lik)
    chains, n, slack = 3, 35, 1024                                       # 35 draws: two segments of the statistics kernel
    draws = torch.from_numpy(0.5 * rng.standard_normal((chains, n, d)))
    flat = torch.full((slack + chains * (n + 3) * d + slack,), float("inf"), dtype=torch.float64, device="cuda")
    big = flat[slack:slack + chains * (n + 3) * d].view(chains, n + 3, d)
    big[:, :n] = draws.cuda()
    x = big[:, :n]
    assert not x.is_contiguous() and dg._row_major(x) and x.stride(0) == (n + 3) * d
    clean = torch.from_numpy(tgt.params.reshape(1, -1)).cuda()
    row_len = clean.shape[1]
    tflat = torch.full((slack + row_len + slack,), float("inf"), dtype=torch.float64, device="cuda")
    tflat[slack:slack + row_len] = clean[0]
    cflat = torch.full((slack + 1 + slack,), float("inf"), dtype=torch.float64, device="cuda")
    cflat[slack] = float(yobs.mean())
    nob = (N + 63) // 64
    table = tflat[slack:slack + row_len].view(1, row_len)
    y, y_flat = _raw_yrep(x, table, 0, chains, 0, nob, 11, guard=slack)
    Tt, t_flat = _raw_stats(x, table, 0, chains, 11, cflat[slack:slack + 1], guard=slack)
    want_y, _f = _raw_yrep(x.contiguous(), clean, 0, chains, 0, nob, 11)
    want_T, _f = _raw_stats(x.contiguous(), clean, 0, chains, 11, cflat[slack:slack + 1].clone())
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(Tt).all())
    assert torch.equal(y, want_y) and torch.equal(Tt, want_T)
    for buf in (y_flat, t_flat):   # nothing written before or beyond the output
        assert bool((buf[:slack] == GUARD).all()) and bool((buf[-slack:] == GUARD).all())
    assert bool((y != GUARD).all()) and bool((Tt != GUARD).all())                   # and every element inside was written
    assert bool((Tt[..., 2] <= Tt[..., 3]).all()) and bool((Tt[..., 4] <= N).all())


def test_a_nan_coefficient_stays_in_its_draw_and_group():
    tgt = _three_groups()
    rng = np.random.default_rng(13)
    job = rng.standard_normal((9, 11, 5))
    x = torch.from_numpy(job).cuda()
    y, clean = tgt.replicate(x, random_seed=4), tgt.ppc(x, random_seed=4)
    job[4, 6, 2] = np.nan                          # one coefficient of one draw of group 1
    xb = torch.from_numpy(job).cuda()
    yb, bad = tgt.replicate(xb, random_seed=4), tgt.ppc(xb, random_seed=4)
    assert bool(torch.isnan(yb[4, 6, :65]).all()) and not bool(yb[4, 6, 65:].any())
    yb[4, 6] = y[4, 6]
    assert torch.equal(yb, y) and bool(torch.isfinite(y).all())
    table = torch.from_numpy(tgt.params.reshape(3, -1)).cuda()
    centre = torch.from_numpy(np.array([m.y.sum() / 65 for m in tgt.members])).cuda()
    Tc, Tb = _raw_stats(x, table, 0, 3, 4, centre)[0], _raw_stats(xb, table, 0, 3, 4, centre)[0]
    assert bool(torch.isnan(Tb[4, 6, [0, 1, 2, 3, 5, 6]]).all()) and float(Tb[4, 6, 4]) == 0.0    # min and max keep the NaN
    Tb[4, 6] = Tc[4, 6]
    assert torch.equal(Tb, Tc) and bool(torch.isfinite(Tc).all())
    for k in ("T_obs", "T_rep_mean", "T_rep_quantiles", "p_value"):
        assert torch.equal(bad[k][0], clean[k][0]) and torch.equal(bad[k][2], clean[k][2]), k
        assert bool(torch.isfinite(clean[k]).all()), k
    assert bool(torch.isnan(bad["T_rep_quantiles"][1][:, :4]).all()) and bool(torch.isnan(bad["T_rep_mean"][1][:4]).all())
    assert bool(torch.isfinite(bad["p_value"]).all())                              # the NaN draw counts as "not >="


def test_predict_response_is_numpys_quantile_of_the_devices_own_array():
    rng = np.random.default_rng(40)
    N, d, per, n = 70, 4, 3, 41
    ms = [T.GLM(rng.standard_normal((N, d)) / 2.0, rng.poisson(2.0, N).astype(np.float64), "poisson") for _ in range(3)]
    tgt = T.Batched(ms)
    Xn = [np.concatenate([rng.standard_normal((N + 3, d - 1)) / 2.0, np.linspace(0.0, 5.0, N + 3)[:, None]], axis=1) for _ in range(3)]
    x = torch.from_numpy(0.5 * rng.standard_normal((3 * per, n, d)) + np.array([0.0, 0.0, 0.0, 1.0])).cuda()
    probs = [0.05, 0.5, 0.95, 0.0, 1.0]
    out = tgt.predict_response(x, Xn, probs=probs, random_seed=8)
    y = tgt.replicate(x, Xn, random_seed=8)
    S, n_new = per * n, N + 3
    pool = y.cpu().numpy().reshape(3, S, 128)[:, :, :n_new]
    srt = np.sort(pool, axis=1)
    h = [p * (S - 1) for p in probs]
    lo = [int(np.floor(v)) for v in h]
    hi = [min(k + 1, S - 1) for k in lo]
    frac = np.array([a - b for a, b in zip(h, lo)]).reshape(-1, 1)
    got = out["y_quantiles"].cpu().numpy()
    assert got.shape == (3, 5, n_new) and out["n"] == S
    assert np.array_equal(got, srt[:, lo] + (srt[:, hi] - srt[:, lo]) * frac)
    npq = np.quantile(pool, probs, axis=1).transpose(1, 0, 2)
    assert (np.abs(got - npq) <= 4 * U * np.maximum(np.abs(srt[:, lo]), np.abs(srt[:, hi]))).all()
    assert np.array_equal(out["y_min"].cpu().numpy(), srt[:, 0]) and np.array_equal(out["y_max"].cpu().numpy(), srt[:, -1])
    assert srt[:, -1].max() > 50 and (got[:, 0] <= got[:, 1]).all() and (got[:, 1] <= got[:, 2]).all()
    unit, ranks = 3 * per * n * 64 * 8, len(set([0, S - 1] + lo + hi))
    chunked = tgt.predict_response(x, Xn, probs=probs, random_seed=8, scratch_bytes=unit + 256 * 64 * 8 * ranks)
    halves = tgt.predict_response([x[:4], x[4:]], Xn, probs=probs, random_seed=8)
    for other in (chunked, halves):
        for k in ("y_quantiles", "y_min", "y_max"):
            assert torch.equal(out[k], other[k]), k


def test_ppc_end_to_end_on_exact_gaussian_posterior_draws():
    """N = 50, d = 4, known sigma; 8 x 125 draws from GLM.posterior_gaussian(), drawn in numpy (tests/_yrep_model.e2e_case: the
    model gave this verdict on the CPU first). Data from the model: every p-value inside (0.05, 0.95) -- but `zeros`, which is
    1 by identity for a continuous response (no replicate and no observation is 0: 0 >= 0 in every draw). Data with three
    times the noise: the Pearson statistic of the data is beyond every replicate's."""
    names = predictive.PPC_NAMES
    verdicts = {}
    for noise in (1.0, 3.0):
        c = Y.e2e_case(noise)
        tgt = T.GLM(c["X"], c["y"], "gaussian", prior_scale=c["prior_scale"], sigma=c["sigma"])
        out = tgt.ppc(torch.from_numpy(c["x"]).cuda(), random_seed=Y.SEED)
        p = out["p_value"][0].cpu().numpy()
        verdicts[noise] = p
        print("noise x%g: p = %s" % (noise, dict(zip(names, np.round(p, 3)))))
        assert out["n"] == 1000 and out["T_rep_quantiles"].shape == (1, 3, 5)
        q = out["T_rep_quantiles"][0].cpu().numpy()
        assert (q[0] <= q[1]).all() and (q[1] <= q[2]).all()
        # the replicated mean and sd centre on the model's: mean of y_rep ~ mean of X beta, sd ~ sqrt(sigma^2 + var(X beta))
        assert abs(float(out["T_rep_mean"][0, 0]) - float(out["T_obs"][0, 0])) < 0.2
    good, bad = verdicts[1.0], verdicts[3.0]
    for k, name in enumerate(names):
        if name == "zeros":
            assert good[k] == 1.0
        else:
            assert 0.05 < good[k] < 0.95, name
    assert bad[names.index("chisq")] < 0.01 and bad[names.index("sd")] < 0.01


def test_two_blocks_on_two_devices_equal_the_one_device_result():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible devices")
    D = _on_device("poisson")
    tgt, x = D["tgt"], D["x"]
    one = tgt.ppc(x, random_seed=3)
    two = tgt.ppc([x[:3].contiguous(), x[3:].to("cuda:1")], random_seed=3)          # cuts group 1
    for k in ("T_obs", "T_rep_quantiles", "p_value"):
        assert _same(one[k].cpu(), two[k].cpu()) and two[k].device == one[k].device, k
    a = tgt.predict_response(x, random_seed=3)
    b = tgt.predict_response([x[:3].contiguous(), x[3:].to("cuda:1")], random_seed=3)
    for k in ("y_quantiles", "y_min", "y_max"):
        assert _same(a[k].cpu(), b[k].cpu()), k
