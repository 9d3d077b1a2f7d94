"""Posterior predictions at new X from a trace in HBM: Batched.predict (lmc_glm_linpred writes the linear predictor in chunks
of observation blocks, the radix select of csrc/lmc_select.hip takes its order statistics) next to the
torch statement of the same result on the same tensor -- eta by a batched matmul, a chunked torch.sort, indexing and the same
interpolation, moments by torch.var_mean. Synthetic float64 draws of the README's GLM shape by default (256 posteriors x 64
chains x 500 draws, d = 32) and N_new = 256 points per posterior, gaussian likelihood, probs = (0.05, 0.5, 0.95).

Both paths are warmed up, then timed alternately (--repeats times each, a device synchronise inside every timing); the line
reports the median, the minimum and the maximum of each, the peak extra device memory of each (max_memory_allocated above what
was allocated before the call), and the largest difference of the two eta_quantiles over the forward bound of the two
contractions, 2 (d + 2) u max_s sum_e |X_e q_se| + 4 u max |eta| (tests/_linpred_model.py; must be <= 1). One JSON line.

    python tools/predict_rate.py [--groups G --per P --draws N --dim D --n-new M --scratch-gib S --sort-cols K --repeats R --warmup W]"""
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


def torch_predict(x, Xn, probs, per, cols):
    """The torch baseline: eta_quantiles [G, Q, M], eta_mean [G, M], eta_sd [G, M] from ``cols`` columns of eta at a time."""
    c, n, d = x.shape
    G, S, M = c // per, per * n, Xn.shape[1]
    h = [p * (S - 1) for p in probs]
    lo = [int(math.floor(v)) for v in h]
    hi = [min(k + 1, S - 1) for k in lo]
    frac = torch.tensor([a - b for a, b in zip(h, lo)], dtype=torch.float64, device=x.device).reshape(1, 1, -1)
    lo_t, hi_t = torch.tensor(lo, device=x.device), torch.tensor(hi, device=x.device)
    q = torch.empty((G, len(probs), M), dtype=torch.float64, device=x.device)
    mean, sd = torch.empty((G, M), dtype=torch.float64, device=x.device), torch.empty((G, M), dtype=torch.float64, device=x.device)
    xt = x.reshape(G, S, d).transpose(1, 2)                                       # [G, d, S], a view
    for a in range(0, M, cols):
        b = min(a + cols, M)
        eta = torch.bmm(Xn[:, a:b], xt)                                           # [G, k, S]
        var, mu = torch.var_mean(eta, dim=2)
        mean[:, a:b], sd[:, a:b] = mu, torch.sqrt(var)
        srt = torch.sort(eta, dim=2).values
        vlo, vhi = srt.index_select(2, lo_t), srt.index_select(2, hi_t)           # [G, k, Q]
        q[:, :, a:b] = (vlo + (vhi - vlo) * frac).transpose(1, 2)
    return q, mean, sd


def eta_bound(x, Xn, per, cols):
    """[G, M]: 2 (d + 2) u max_s sum_e |X_e q_se|, the two contractions' forward errors, an order statistic being 1-Lipschitz
    in the sup norm of its column; the caller adds the interpolation's roundings."""
    c, n, d = x.shape
    G, S, M = c // per, per * n, Xn.shape[1]
    at = x.abs().reshape(G, S, d).transpose(1, 2)
    out = torch.empty((G, M), dtype=torch.float64, device=x.device)
    for a in range(0, M, cols):
        b = min(a + cols, M)
        out[:, a:b] = torch.bmm(Xn[:, a:b].abs(), at).amax(dim=2)
    return 2 * (d + 2) * 2.0 ** -53 * out


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
    ap.add_argument("--n-new", type=int, default=256)
    ap.add_argument("--scratch-gib", type=float, default=8.0)
    ap.add_argument("--sort-cols", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise _abi.HipLibraryError("predict_rate.py measures on a GPU; there is none")
    probs = (0.05, 0.5, 0.95)
    rng = np.random.default_rng(1)
    members = []
    for _ in range(a.groups):   # the training data only shape the target; the draws below are synthetic
        X = rng.standard_normal((8, a.dim))
        members.append(T.GLM(X, rng.standard_normal(8), "gaussian"))
    tgt = T.Batched(members)
    Xn_host = [rng.standard_normal((a.n_new, a.dim)) / math.sqrt(a.dim) for _ in range(a.groups)]
    Xn = torch.from_numpy(np.stack(Xn_host)).cuda()
    chains = a.groups * a.per
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((chains, a.draws, a.dim), dtype=torch.float64, device="cuda", generator=gen)
    x += torch.arange(a.dim, dtype=torch.float64, device="cuda") / a.dim           # one scale, a location per coordinate
    scratch = int(a.scratch_gib * (1 << 30))
    paths = {"predict": lambda: tgt.predict(x, Xn_host, probs=probs, scratch_bytes=scratch),
             "torch": lambda: torch_predict(x, Xn, probs, a.per, a.sort_cols)}
    for _ in range(a.warmup):
        for fn in paths.values():
            fn()
    times, peaks, outs = {k: [] for k in paths}, {k: 0 for k in paths}, {}
    for _ in range(a.repeats):
        for name, fn in paths.items():                                             # alternated
            outs[name], dt, peak = timed(fn)
            times[name].append(dt)
            peaks[name] = max(peaks[name], peak)
    got, (want, mean, sd) = outs["predict"], outs["torch"]
    bound = eta_bound(x, Xn, a.per, a.sort_cols).unsqueeze(1) + 4 * 2.0 ** -53 * torch.maximum(got["eta_quantiles"].abs(), want.abs())
    ratio = float(((got["eta_quantiles"] - want).abs() / bound).max())
    eta_bytes = 8 * chains * a.draws * a.n_new
    unit = 8 * chains * a.draws * 64
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    line = {"tool": "predict_rate", "build": _abi.load().lmc_build_hash().decode(), "groups": a.groups, "per": a.per,
            "draws": a.draws, "dim": a.dim, "n_new": a.n_new, "probs": probs, "scratch_bytes": scratch, "sort_cols": a.sort_cols,
            "repeats": a.repeats, "warmup": a.warmup, "trace_bytes": 8 * chains * a.draws * a.dim, "eta_bytes": eta_bytes,
            "obs_block_bytes": unit, "obs_blocks_per_chunk": min(scratch // unit, (a.n_new + 63) // 64),
            "eta_quantiles_max_error_over_bound": ratio, "within_bound": ratio <= 1.0,
            "eta_mean_max_abs_diff": float((got["eta_mean"] - mean).abs().max()),
            "eta_sd_max_abs_diff": float((got["eta_sd"] - sd).abs().max())}
    for k in paths:
        line[k + "_s"] = {"median": med[k], "min": min(times[k]), "max": max(times[k])}
        line[k + "_peak_extra_bytes"] = peaks[k]
    line["predict_draw_observations_per_s"] = chains * a.draws * a.n_new / med["predict"]
    line["torch_over_predict"] = med["torch"] / med["predict"]
    print(json.dumps(line))
    if not line["within_bound"]:
        raise SystemExit("eta_quantiles of the two paths differ by %.3g times the bound" % ratio)


if __name__ == "__main__":
    main()
