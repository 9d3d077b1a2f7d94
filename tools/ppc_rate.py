"""Replicated data from a trace in HBM: Batched.ppc (lmc_glm_yrep_stats reduces every draw's replicated data set to seven test
statistics, y_rep is never written) and Batched.predict_response (lmc_glm_yrep writes y_rep in chunks of observation blocks,
the radix select takes its order statistics), each next to the torch statement of the same result on
the same tensor -- eta by a batched matmul, the inverse link, torch.poisson, then reductions (ppc) or a chunked torch.sort and
the same interpolation (predict_response). Synthetic float64 draws of the README's GLM shape by default (256 posteriors x 64
chains x 500 draws, d = 32, N = 256, poisson), probs = (0.05, 0.5, 0.95).

All four paths are warmed up, then timed alternately (--repeats times each, a device synchronise inside every timing); the
line reports the median, the minimum and the maximum of each and the peak extra device memory of each (max_memory_allocated
above what was allocated before the call). The two generators differ, so the results agree in distribution only: the line
carries the largest difference of the posterior means of the replicated mean and sd, and of the median band, for the eye.
One JSON line.

    python tools/ppc_rate.py [--groups G --per P --draws N --dim D --n-obs M --scratch-gib S --torch-groups K --repeats R --warmup W]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from littlemcmc_amd import _abi  # noqa: E402
from littlemcmc_amd import targets as T  # noqa: E402


def torch_yrep(x, X, per, g0, g1):
    """y_rep[g, N, S] and mu of the groups [g0, g1) in torch: bmm, exp, torch.poisson."""
    c, n, d = x.shape
    S = per * n
    xt = x[g0 * per:g1 * per].reshape(g1 - g0, S, d).transpose(1, 2)                  # [g, d, S], a view
    mu = torch.exp(torch.bmm(X[g0:g1], xt))                                        # [g, N, S]
    return torch.poisson(mu), mu


def torch_ppc(x, X, y, per, step):
    """The torch baseline of ppc: T_rep_mean[G, 5] and p_value[G, 6], ``step`` groups at a time."""
    G, N = y.shape
    S = per * x.shape[1]
    mean, p = torch.empty((G, 5), dtype=torch.float64, device=x.device), torch.empty((G, 6), dtype=torch.float64, device=x.device)
    obs = torch.stack([y.mean(dim=1), y.std(dim=1), y.amin(dim=1), y.amax(dim=1), (y == 0).sum(dim=1).double()], dim=1)
    for g0 in range(0, G, step):
        g1 = min(g0 + step, G)
        yr, mu = torch_yrep(x, X, per, g0, g1)
        sd, mn = torch.std_mean(yr, dim=1)
        tr = torch.stack([mn, sd, yr.amin(dim=1), yr.amax(dim=1), (yr == 0).sum(dim=1).double()], dim=2)     # [g, S, 5]
        chi_rep = ((yr - mu) ** 2 / mu).sum(dim=1)
        chi_obs = ((y[g0:g1].unsqueeze(2) - mu) ** 2 / mu).sum(dim=1)
        mean[g0:g1] = tr.mean(dim=1)
        p[g0:g1, :5] = (tr >= obs[g0:g1].unsqueeze(1)).double().mean(dim=1)
        p[g0:g1, 5] = (chi_rep >= chi_obs).double().mean(dim=1)
    return mean, p


def torch_band(x, X, per, probs, step):
    """The torch baseline of predict_response: y_quantiles[G, Q, N] by a sort of y_rep, ``step`` groups at a time."""
    G, N = X.shape[0], X.shape[1]
    S = per * x.shape[1]
    h = [p * (S - 1) for p in probs]
    lo = [int(math.floor(v)) for v in h]
    hi = [min(k + 1, S - 1) for k in lo]
    frac = torch.tensor([a - b for a, b in zip(h, lo)], dtype=torch.float64, device=x.device).reshape(1, 1, -1)
    lo_t, hi_t = torch.tensor(lo, device=x.device), torch.tensor(hi, device=x.device)
    q = torch.empty((G, len(probs), N), dtype=torch.float64, device=x.device)
    for g0 in range(0, G, step):
        g1 = min(g0 + step, G)
        srt = torch.sort(torch_yrep(x, X, per, g0, g1)[0], dim=2).values
        vlo, vhi = srt.index_select(2, lo_t), srt.index_select(2, hi_t)
        q[g0:g1] = (vlo + (vhi - vlo) * frac).transpose(1, 2)
    return q


def timed(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    return out, dt, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--groups", type=int, default=256)
    ap.add_argument("--per", type=int, default=64)
    ap.add_argument("--draws", type=int, default=500)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--n-obs", type=int, default=256)
    ap.add_argument("--scratch-gib", type=float, default=8.0)
    ap.add_argument("--torch-groups", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise _abi.HipLibraryError("ppc_rate.py measures on a GPU; there is none")
    probs = (0.05, 0.5, 0.95)
    rng = np.random.default_rng(1)
    members = []
    for _ in range(a.groups):   # an intercept near log 7 and small slopes: the means lie on both sides of 10 (both samplers run)
        X = rng.standard_normal((a.n_obs, a.dim)) / math.sqrt(a.dim)
        X[:, 0] = 1.0
        members.append(T.GLM(X, rng.poisson(7.0, a.n_obs).astype(np.float64), "poisson"))
    tgt = T.Batched(members)
    Xd = torch.from_numpy(np.stack([m.X for m in members])).cuda()
    yd = torch.from_numpy(np.stack([m.y for m in members])).cuda()
    chains = a.groups * a.per
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = 0.5 * torch.randn((chains, a.draws, a.dim), dtype=torch.float64, device="cuda", generator=gen)
    x[:, :, 0] = 2.0 + 0.2 * x[:, :, 0]
    scratch = int(a.scratch_gib * (1 << 30))
    paths = {"ppc": lambda: tgt.ppc(x, probs=probs, random_seed=1),
             "torch_ppc": lambda: torch_ppc(x, Xd, yd, a.per, a.torch_groups),
             "predict_response": lambda: tgt.predict_response(x, probs=probs, random_seed=1, scratch_bytes=scratch),
             "torch_band": lambda: torch_band(x, Xd, a.per, probs, a.torch_groups)}
    for _ in range(a.warmup):
        for fn in paths.values():
            fn()
    times, peaks, outs = {k: [] for k in paths}, {k: 0 for k in paths}, {}
    for _ in range(a.repeats):
        for name, fn in paths.items():                                             # alternated
            outs[name], dt, peak = timed(fn)
            times[name].append(dt)
            peaks[name] = max(peaks[name], peak)
    got, (t_mean, t_p) = outs["ppc"], outs["torch_ppc"]
    band, t_band = outs["predict_response"]["y_quantiles"], outs["torch_band"]
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    elements = chains * a.draws * a.n_obs
    line = {"tool": "ppc_rate", "build": _abi.load().lmc_build_hash().decode(), "groups": a.groups, "per": a.per, "draws": a.draws,
            "dim": a.dim, "n_obs": a.n_obs, "likelihood": "poisson", "probs": probs, "scratch_bytes": scratch,
            "torch_groups": a.torch_groups, "repeats": a.repeats, "warmup": a.warmup, "trace_bytes": 8 * chains * a.draws * a.dim,
            "y_rep_bytes": 8 * elements, "mean_mu": float(torch.exp(torch.bmm(Xd[:1], x[:a.per].reshape(1, -1, a.dim).transpose(1, 2))).mean()),
            "rep_mean_max_abs_diff": float((got["T_rep_mean"][:, 0] - t_mean[:, 0]).abs().max()),
            "rep_sd_max_abs_diff": float((got["T_rep_mean"][:, 1] - t_mean[:, 1]).abs().max()),
            "p_value_max_abs_diff": float((got["p_value"] - t_p).abs().max()),
            "median_band_max_abs_diff": float((band[:, 1] - t_band[:, 1]).abs().max())}
    for k in paths:
        line[k + "_s"] = {"median": med[k], "min": min(times[k]), "max": max(times[k])}
        line[k + "_peak_extra_bytes"] = peaks[k]
    line["ppc_draw_observations_per_s"] = elements / med["ppc"]
    line["predict_response_draw_observations_per_s"] = elements / med["predict_response"]
    line["torch_over_ppc"] = med["torch_ppc"] / med["ppc"]
    line["torch_over_predict_response"] = med["torch_band"] / med["predict_response"]
    print(json.dumps(line))


if __name__ == "__main__":
    main()
