#!/usr/bin/env python3
"""The pointwise predictive pass (lmc_glm_pointwise, littlemcmc_amd/predictive.py) timed on one GPU against the torch
formulation a user would otherwise write, on synthetic draws in HBM:

    python tools/bench_predictive.py                       # 256 groups x 64 chains x 500 draws, N = 256, d = 32, bernoulli
    python tools/bench_predictive.py --groups 1 --per 16384    # one posterior with the same number of draws

Three variants: ``waic`` (predictive.waic: the kernel, the merge and the finalisation), ``kernel`` (the C entry alone on a
table already in HBM) and ``torch`` (per group ``x_g.reshape(-1, d) @ X_g.T``, the link, then logsumexp / var / mean over
draws, chunked over groups so that the [draws, N] intermediates fit). Every variant is warmed up, then the variants are timed
alternately (A B C A B C ...), one JSON line per (variant, repeat): a host clock around a call that ends in a device
synchronise. Read the spread between repeats before the difference between variants. The results of the two ways are
compared as well.

flop count of the kernel per (draw, observation), an FMA counted as two, from csrc/lmc_predict.hip and lmc_targets.hpp
(exp_lane 36: clamp 2, reduction 6, 13 FMAs, ldexp + convert 2; log1p_unit 37: quotient 2, square 1, 15 FMAs, tail 4; a
division counted as one): contraction 2 d; link: bernoulli 79 (exp_lane, 1 + ex, quotient, y eta, max, log1p_unit, add, sub),
poisson 38, gaussian 4; running statistics 44 (max, two sums, deviation and square 3, l - m, exp_lane, add). At d = 32 the
elementwise part (123 for bernoulli) is twice the contraction (64)."""
import argparse
import ctypes
import json
import os
import sys
import time

LINK_FLOP = {"bernoulli": 79, "poisson": 38, "gaussian": 4}
STATS_FLOP = 44
FP64_VALU_PEAK = 78.6e12   # flop/s: 256 CUs x 4 SIMDs x 16 lanes x 2 (FMA) x 2.4 GHz


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--groups", type=int, default=256)
    ap.add_argument("--per", type=int, default=64, help="chains per group")
    ap.add_argument("--draws", type=int, default=500)
    ap.add_argument("--obs", type=int, default=256, help="N, observations per group")
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--likelihood", default="bernoulli", choices=sorted(LINK_FLOP))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--torch-chunk", type=int, default=8, help="groups per chunk of the torch formulation")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch

    from littlemcmc_amd import _abi, _build, predictive
    from littlemcmc_amd import targets as T

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures, and a measurement does not fall back")

    def emit(rec):
        rec["build_hash"] = _build.binary_hash()
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(line + "\n")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    G, per, n, N, d, lik = args.groups, args.per, args.draws, args.obs, args.dim, args.likelihood
    rng = np.random.default_rng(20261019)
    members = []
    for g in range(G):
        X = rng.standard_normal((N, d)) / np.sqrt(d)
        eta = X @ rng.standard_normal(d)
        y = {"bernoulli": (rng.random(N) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64),
             "poisson": rng.poisson(np.exp(np.clip(eta, -3, 3))).astype(np.float64),
             "gaussian": eta + rng.standard_normal(N)}[lik]
        members.append(T.GLM(X, y, lik))
    tgt = T.Batched(members) if G > 1 else members[0]
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.randn((G * per, n, d), dtype=torch.float64, device="cuda", generator=gen)
    table = torch.from_numpy(np.ascontiguousarray(tgt.params).reshape(G, -1)).cuda()
    npad = (N + 63) // 64 * 64
    Xd = torch.from_numpy(np.stack([m.X for m in members])).cuda()          # [G, N, d]
    yd = torch.from_numpy(np.stack([m.y for m in members])).cuda()          # [G, N]
    lib = _abi.load()
    stream = torch.cuda.current_stream().cuda_stream

    def kernel():
        out = torch.empty((G, 6, npad), dtype=torch.float64, device="cuda")
        rc = lib.lmc_glm_pointwise(ctypes.c_void_p(x.data_ptr()), G * per, n, d, 0, n, ctypes.c_void_p(table.data_ptr()),
                                   table.shape[1], G, 0, per, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream))
        assert rc == 0, rc
        return out

    def waic():
        return predictive.waic(x, tgt)

    peak = {"bytes": 0}

    def torch_way():
        lppd, p_waic = [], []
        S = per * n
        ch = max(1, min(args.torch_chunk, G))
        for lo in range(0, G, ch):
            hi = min(lo + ch, G)
            xg = x[lo * per:hi * per].reshape(hi - lo, S, d)
            eta = torch.bmm(xg, Xd[lo:hi].transpose(1, 2))                 # [g, S, N]: the array the kernel never writes
            yy = yd[lo:hi].unsqueeze(1)
            if lik == "bernoulli":
                ll = yy * eta - torch.nn.functional.softplus(eta)
            elif lik == "poisson":
                ll = yy * eta - torch.exp(eta)
            else:
                ll = -0.5 * (yy - eta) ** 2
            lppd.append(torch.logsumexp(ll, dim=1) - float(np.log(S)))
            p_waic.append(ll.var(dim=1))
            peak["bytes"] = max(peak["bytes"], 2 * eta.numel() * 8)        # eta and ll alive together (temporaries come on top)
        return torch.cat(lppd), torch.cat(p_waic)

    variants = {"waic": waic, "kernel": kernel, "torch": torch_way}
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    warm = {}
    for name, fn in variants.items():
        torch.cuda.reset_peak_memory_stats()
        warm[name] = timed(fn)
        warm[name] += (torch.cuda.max_memory_allocated() - base,)
    w, (t_lppd, t_p) = warm["waic"][1], warm["torch"][1]
    # the torch way drops the constants, as the kernel's planes do
    k_lppd = w["lppd"] - torch.as_tensor(np.stack([m.loglik_constant() for m in members])).cuda()
    draws_total = G * per * n
    flop = draws_total * npad * (2 * d + LINK_FLOP[lik] + STATS_FLOP)
    shape = {"groups": G, "chains_per_group": per, "draws": n, "obs": N, "dim": d, "likelihood": lik}
    emit(dict(shape, what="agreement", lppd_max_abs_diff=float((k_lppd - t_lppd).abs().max()),
              p_waic_max_rel_diff=float(((w["p_waic"] - t_p).abs() / t_p).max()),
              first_call_seconds={k: v[0] for k, v in warm.items()},
              peak_extra_bytes={k: int(v[2]) for k, v in warm.items()},
              torch_intermediate_bytes=int(peak["bytes"]), kernel_output_bytes=G * 6 * npad * 8,
              trace_bytes=draws_total * d * 8, flop_per_call=flop))
    for rep in range(args.repeats):
        for name, fn in variants.items():
            sec = timed(fn)[0]
            rec = dict(shape, what="time", variant=name, repeat=rep, seconds=sec)
            if name == "kernel":
                rec.update(tflops=flop / sec / 1e12, frac_fp64_vector_peak=flop / sec / FP64_VALU_PEAK,
                           trace_gb_per_s=draws_total * d * 8 / sec / 1e9)
            emit(rec)


if __name__ == "__main__":
    main()
