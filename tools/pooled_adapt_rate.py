#!/usr/bin/env python3
"""What a dense mass matrix pooled across chains is worth (GPU box): AR(1) rho = 0.9, tune + draws, at chains x d, for
    diag      init="jitter+adapt_diag"                     the diagonal headline
    full      QuadPotentialFull(true covariance)           existing code and the CEILING: nobody has that matrix
    pooled    init="jitter+adapt_full_pooled"              QuadPotentialFullPooled
    adapt     init="jitter+adapt_full" (per chain)         only where asked for (--per-chain; 37 s at d = 128)
everything in one process, warmed up, the variants alternating. Every job is driven as sample() drives it (same engine
set-up, same launch schedule, same job loops) with the draws left in HBM, in two timed segments -- tuning, then draws --
on the synchronised host clock; ESS through diagnostics.summarize on the trace where it lies.

    python tools/pooled_adapt_rate.py [--chains 65536] [--dims 128,32] [--tune 1000] [--draws 1000] [--reps 2]
                                      [--per-chain 32] [--out profiles/pooled_adapt_rate.txt]
    python tools/pooled_adapt_rate.py --snapshots 20 [--chains 65536] [--dims 128]
        only snapshots of random positions: the run to put under `rocprofv3 --kernel-trace --stats`
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import littlemcmc_amd as lmc  # noqa: E402
from littlemcmc_amd import _abi, sampling  # noqa: E402
from littlemcmc_amd import diagnostics as dg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--chains", type=int, default=65536)
ap.add_argument("--dims", default="128,32")
ap.add_argument("--tune", type=int, default=1000)
ap.add_argument("--draws", type=int, default=1000)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--per-chain", default="32", help="dims at which per-chain adapt_full runs too")
ap.add_argument("--out", default=None)
ap.add_argument("--snapshots", type=int, default=0)
args = ap.parse_args()
SEED = 20260928
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def snapshots_only(chains, d, count):
    """`count` snapshots of fixed random positions (mean 10) and one pool_get: the accumulate kernels alone."""
    rng = np.random.RandomState(1)
    eng = lmc.Engine(lmc.targets.StdNormal(d), chains, potential="full")
    try:
        eng.set_dense_potential(np.eye(d))
        eng.set_position(10.0 + rng.standard_normal((chains, d)))
        eng.pool_reset()
        eng.pool_accumulate()
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            eng.pool_accumulate()
        eng.synchronize()
        dt = (time.perf_counter() - t0) / count
        n, _mean, m2 = eng.pool_get()
        say("snapshot of %d chains x d = %d: %.1f us each on the host clock (%d back to back, column sums + product + "
            "reduction); n = %d, trace(m2) / n = %.4f" % (chains, d, 1e6 * dt, count, n, float(np.trace(m2)) / n))
    finally:
        eng.close()


def job(variant, chains, d):
    tgt = lmc.targets.AR1(d, 0.9)
    seeds = sampling._derive_seeds(SEED, chains)
    tune, n_total = args.tune, args.tune + args.draws
    if variant == "full":
        idx = np.arange(d)
        start, _step = lmc.init_nuts(tgt, d, init="jitter+adapt_diag", random_seed=seeds)
        step = lmc.NUTS(tgt, d, potential=lmc.QuadPotentialFull(0.9 ** np.abs(idx[:, None] - idx[None, :])))
    else:
        init = {"diag": "jitter+adapt_diag", "pooled": "jitter+adapt_full_pooled", "adapt": "jitter+adapt_full"}[variant]
        start, step = lmc.init_nuts(tgt, d, init=init, random_seed=seeds)
    eng = step._make_engine(chains)
    try:
        eng.seed(seeds)
        eng.set_position(np.ascontiguousarray(sampling._start_points(start, chains, d)))
        eng.reset_tuning()
        eng.reserve(n_total, keep_trace=True, trace_begin=tune)
        per = sampling._launch_schedule(n_total, None, eng.resident_chains(), chains, eng.wide, False)
        eng.synchronize()
        t0 = time.perf_counter()
        if variant == "pooled":
            sampling._run_job_pooled(eng, tune, tune, per, False)
        else:
            sampling._run_job(eng, tune, tune, per, False)
        t1 = time.perf_counter()
        sampling._run_job(eng, tune, n_total, per, False, first_iter=tune)
        t2 = time.perf_counter()
        leaps = int(eng.counters()[:, _abi.CT_LEAPFROGS].sum())
        depth = float(eng.stat_i32(_abi.STAT_DEPTH, tune, args.draws).mean())
        draw_leaps = int(eng.stat_i32(_abi.STAT_TREE_SIZE, tune, args.draws).astype(np.int64).sum())
        diag = dg.summarize(dg.trace_tensor(eng))
        ess, rhat = float(diag["ess"].min()), float(diag["rhat"].max())
        var = float(diag["var"].mean())
        return dict(job=t2 - t0, tune=t1 - t0, draw=t2 - t1, rate=leaps / (t2 - t0), draw_rate=draw_leaps / (t2 - t1), depth=depth,
                    tune_leaps=leaps - draw_leaps,
                    ess=ess, rhat=rhat, var=var, kernel=eng.last_run_dense_kernel())
    finally:
        eng.close()


dims = [int(x) for x in args.dims.split(",") if x]
if args.snapshots:
    for d in dims:
        snapshots_only(args.chains, d, args.snapshots)
else:
    per_chain = [int(x) for x in args.per_chain.split(",") if x]
    say("build %s; AR(1) rho = 0.9, %d chains, tune %d + draws %d, seed %d; best of %d alternating runs after a warm-up"
        % (_abi.load().lmc_build_hash().decode(), args.chains, args.tune, args.draws, SEED, args.reps))
    for d in dims:
        variants = ["diag", "full", "pooled"] + (["adapt"] if d in per_chain else [])
        job("pooled", min(args.chains, 4096), d)       # warm-up: code objects, allocator, the statistics kernels
        best = {}
        for r in range(args.reps):
            for v in variants:
                res = job(v, args.chains, d)
                say("d = %d run %d %-6s: job %.3f s (tuning %.3f s with %.3e leapfrog steps, draws %.3f s), %.3e leapfrog-steps/s (draws %.3e), mean depth %.2f, "
                    "ESS min %.3e, R-hat max %.4f, mean marginal variance %.3f, dense kernel %s"
                    % (d, r, v, res["job"], res["tune"], res["tune_leaps"], res["draw"], res["rate"], res["draw_rate"], res["depth"], res["ess"],
                       res["rhat"], res["var"], res["kernel"]))
                if v not in best or res["job"] < best[v]["job"]:
                    best[v] = res
        say("")
        say("d = %d, %d chains: | mass | job s | tuning s | leapfrog-steps/s | mean depth | ESS/s (min, per job second) | ESS/s (min, per draw second) |"
            % (d, args.chains))
        for v in variants:
            b = best[v]
            say("| %s | %.2f | %.2f | %.2e | %.2f | %.2e | %.2e |" % (v, b["job"], b["tune"], b["rate"], b["depth"], b["ess"] / b["job"], b["ess"] / b["draw"]))
        p, c, g = best["pooled"], best["full"], best["diag"]
        # the ceiling has its matrix from iteration 0; the pooled job tunes under the identity until its first window ends, with
        # the deep trees of the diagonal job in the dense kernel. What the cuts (8 per window) and drains (one per window) cost
        # shows in the leapfrog rate of the tuning phase, not in its length
        say("pooled / ceiling (true covariance): job time %.3f, ESS/s %.3f; tuning phase %.3f s against %.3f s (+%.3f s) with %.3e "
            "against %.3e leapfrog steps (+%.3e), i.e. at %.3e against %.3e leapfrog-steps/s; pooled / diagonal: ESS/s %.2f"
            % (p["job"] / c["job"], (p["ess"] / p["job"]) / (c["ess"] / c["job"]), p["tune"], c["tune"], p["tune"] - c["tune"],
               p["tune_leaps"], c["tune_leaps"], p["tune_leaps"] - c["tune_leaps"], p["tune_leaps"] / p["tune"],
               c["tune_leaps"] / c["tune"], (p["ess"] / p["job"]) / (g["ess"] / g["job"])))
        say("")
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
