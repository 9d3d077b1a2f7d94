#!/usr/bin/env python3
"""A/B of the three random streams of the fused sampling kernels -- rng = numpy | philox | counter (include/lmc_hip.h:
LMC_RNG_*) -- on the BASELINE shapes, timed the way bench.py's run_job times the headline job: HIP events on the streams
the engine launches on, a throw-away warm-up copy of the job first, two launches kept in flight, K timed launches of
`--iters-per-step` iterations (first half tuning). bench.py itself only knows numpy | philox.

    python tools/ab_rng_modes.py                                  # C3, north_star shape, C2, C4, C5 x the three modes
    python tools/ab_rng_modes.py --shapes C3 north_star --modes counter --lib build_variants/liblmc_plan0.so --tag plan0
    python tools/ab_rng_modes.py --tree ../parent-checkout --modes numpy philox --tag parent

One line per (shape, mode, repeat): leapfrog-steps/s over the kernel-busy span, the dynamic LDS bytes per workgroup of the
launch that ran (lmc_engine_run_lds_bytes), mean tree depth of the last launch. `--repeats` alternates the modes (A B C A B C),
so that drift of the box shows up as disagreement between repeats instead of as a difference between modes. `--lib` measures
another build of the library (tools/variant_build.py: e.g. -DLMC_COUNTER_LDS_PLAN=0, the LDS-layout A/B of the counter mode);
`--tree` measures another checkout with ITS package and library (a parent commit)."""
import argparse
import json
import os
import sys
import time

SHAPES = {   # BASELINE.json's configurations: (target, dim, chains, max_treedepth)
    "C3": ("ar1", 128, 65536, 10),
    "north_star": ("std_normal", 128, 65536, 10),
    "C2": ("std_normal", 64, 4096, 10),
    "C4": ("diag", 1000, 8192, 10),
    "C5": ("funnel", 256, 16384, 12),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument("--modes", nargs="+", default=["numpy", "philox", "counter"])
    ap.add_argument("--steps", type=int, default=10, help="timed launches")
    ap.add_argument("--warmup", type=int, default=2, help="warm-up launches of a throw-away copy of the job")
    ap.add_argument("--iters-per-step", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--lib", default=None, help="another build of liblmc_hip.so to measure")
    ap.add_argument("--tree", default=None, help="another checkout to measure (its package, its library)")
    ap.add_argument("--tag", default="", help="label of this build in the output lines")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()

    root = os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import numpy as np
    import torch

    import littlemcmc_amd as lmc
    from littlemcmc_amd import _abi, _build

    lib_path = os.path.abspath(args.lib) if args.lib else None
    build_hash = _build.binary_hash(lib_path) if lib_path else _build.binary_hash()
    K, ips, W = args.steps, args.iters_per_step, args.warmup
    n_total, n_tune = K * ips, (K * ips) // 2

    def target_of(name, dim):
        return {"ar1": lambda: lmc.targets.AR1(dim, 0.9), "std_normal": lambda: lmc.targets.StdNormal(dim),
                "funnel": lambda: lmc.targets.Funnel(dim), "diag": lambda: lmc.targets.DiagGaussian.ill_conditioned(dim, 1e4)}[name]()

    def one(shape, mode):
        tname, dim, chains, md = SHAPES[shape]
        target = target_of(tname, dim)
        seeds = lmc.distributed.global_seeds(20260928, chains)
        np.random.seed(int(seeds[0]))
        start = 2 * np.random.rand(dim) - 1
        step = lmc.NUTS(target, dim, potential=lmc.QuadPotentialDiagAdapt(dim, start, np.ones(dim), 10), max_treedepth=md)
        kw = step._engine_kwargs()
        kw["rng"] = mode
        if lib_path:
            kw["lib_path"] = lib_path

        def new_job(capacity):
            eng = lmc.Engine(target, chains=chains, **kw)
            step.potential._push_initial(eng)
            eng.seed(seeds)
            eng.set_position(start)
            eng.reset_tuning()
            eng.reserve(capacity, keep_trace=False)
            return eng

        if W > 0:
            w_ips = min(ips, 100)
            warm = new_job(W * w_ips)
            for s in range(W):
                warm.run((W * w_ips) // 2, s * w_ips, w_ips)
            warm.synchronize()
            warm.close()
        eng = new_job(n_total)
        try:
            streams = [torch.cuda.ExternalStream(h, device=torch.device("cuda", 0)) for h in eng.run_streams()]
            ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in streams] for _ in range(K)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for s in range(K):          # two launches in flight: the engine picks the LDS plan of a launch when it is enqueued
                if s >= 2:
                    for b in range(len(streams)):
                        ev[s - 2][b][1].synchronize()
                for b, st in enumerate(streams):
                    ev[s][b][0].record(st)
                eng.run(n_tune, s * ips, ips)
                for b, st in enumerate(streams):
                    ev[s][b][1].record(st)
            eng.synchronize()
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
            nb = len(streams)
            kernel_ms = max(ev[0][b0][0].elapsed_time(ev[K - 1][b1][1]) for b0 in range(nb) for b1 in range(nb))
            assert not eng.status().any(), "chains reported failure status bits"
            leaps = float(eng.counters()[:, _abi.CT_LEAPFROGS].sum())
            depth = float(eng.stat_i32(_abi.STAT_DEPTH, n_total - ips, ips).mean())
            return {"shape": shape, "rng": mode, "build": args.tag or "this", "build_hash": build_hash,
                    "leapfrog_steps_per_s": leaps / (kernel_ms / 1e3), "kernel_ms": kernel_ms, "wall_s": wall, "leapfrogs": leaps,
                    "lds_bytes_per_workgroup": eng.run_lds_bytes(), "kernel_shape": list(eng.kernel_shape()),
                    "mean_depth_last_launch": depth, "steps": K, "iters_per_step": ips, "chains": chains, "dim": dim}
        finally:
            eng.close()

    for rep in range(args.repeats):
        for shape in args.shapes:
            for mode in args.modes:
                rec = one(shape, mode)
                rec["repeat"] = rep
                line = json.dumps(rec)
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as fh:
                        fh.write(line + "\n")


if __name__ == "__main__":
    main()
