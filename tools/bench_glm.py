#!/usr/bin/env python3
"""leapfrog-steps/s of a regression posterior three ways: the fused targets.GLM, the same posterior as
a TorchTarget (X q as one GEMM over all chains per tick), and a targets.Batched of GLMs over many data sets.
Usage (GPU box): python tools/bench_glm.py [N] [d] [chains] [groups] [tune] [draws] [likelihood]
Every figure is the whole job (tune + draws NUTS iterations from a cold start, fixed seeds) in the engine's own loop, run twice
on fresh engines; the second run is reported and both are printed. Design-matrix traffic is derived: 2 N d 8 bytes per gradient, one gradient per leapfrog step."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import littlemcmc_amd as lmc  # noqa: E402
from littlemcmc_amd import _abi  # noqa: E402
from littlemcmc_amd.targets import GLM, Batched, TorchTarget  # noqa: E402

arg = lambda i, default: type(default)(sys.argv[i]) if len(sys.argv) > i else default   # noqa: E731
N, d, chains, groups, tune, draws, lik = arg(1, 256), arg(2, 32), arg(3, 16384), arg(4, 256), arg(5, 500), arg(6, 500), arg(7, "bernoulli")
only = os.environ.get("LMC_GLM_BENCH_ONLY")   # substring filter


def data(seed):
    rs = np.random.RandomState(seed)
    X = rs.randn(N, d) / np.sqrt(d)
    X[:, 0] = 1.0
    eta = X @ rs.randn(d)
    y = {"bernoulli": (rs.rand(N) < 1.0 / (1.0 + np.exp(-eta))) * 1.0, "poisson": rs.poisson(np.exp(np.clip(eta, -3, 3))) * 1.0,
         "gaussian": eta + rs.randn(N)}[lik]
    return X, y


X, y = data(0)
Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()


def torch_posterior(q):   # the same bernoulli / poisson / gaussian posterior, prior_scale = sigma = 1, constants dropped
    eta = q @ Xd.T
    if lik == "bernoulli":
        ll = yd * eta - torch.nn.functional.softplus(eta)
        r = yd - torch.sigmoid(eta)
    elif lik == "poisson":
        mu = torch.exp(eta)
        ll, r = yd * eta - mu, yd - mu
    else:
        r = yd - eta
        ll = -0.5 * r * r
    return ll.sum(dim=1) - 0.5 * (q * q).sum(dim=1), r @ Xd - q


def run(name, target, n_chains):
    """The method of tools/bench_torch_target.py: the engine's own iteration loop, no trace kept, leapfrogs from the device
    counters; the whole job (tune + draws iterations from a cold start) is timed, twice on fresh engines."""
    if only and only not in name:
        return
    out = []
    for _ in range(2):
        eng = lmc.NUTS(target, d)._make_engine(n_chains)
        eng.seed(np.arange(n_chains, dtype=np.uint32) + 1)
        eng.set_position(np.zeros(d))
        eng.reset_tuning()
        eng.reserve(tune + draws, keep_trace=False)
        eng.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.run(tune, 0, tune + draws)
        eng.synchronize()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        leaps = float(eng.counters()[:, _abi.CT_LEAPFROGS].sum())
        divs = float(eng.counters()[:, _abi.CT_DIVS_AFTER_TUNE].sum())
        eng.close()
        out.append((leaps / dt, dt, leaps, divs))
    rate, dt, leaps, divs = out[1]
    print("%-44s %9.3e leapfrog-steps/s  (first run %9.3e; %.2f s, %d chains, N=%d d=%d, %d+%d iterations, %.1f leapfrogs per "
          "iteration, %d divergences after tuning)  design-matrix traffic %.3e B/s"
          % (name, rate, out[0][0], dt, n_chains, N, d, tune, draws, leaps / n_chains / (tune + draws), divs, rate * 2 * N * d * 8), flush=True)


print("build %s, likelihood %s" % (_abi.load().lmc_build_hash().decode(), lik), flush=True)
run("fused GLM", GLM(X, y, lik), chains)
run("TorchTarget (same posterior, GEMM form)", TorchTarget(d, torch_posterior), chains)
run("Batched of %d GLMs, %d chains each" % (groups, chains // groups), Batched([GLM(*data(g), lik) for g in range(groups)]), chains)
