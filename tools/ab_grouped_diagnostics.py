#!/usr/bin/env python3
"""A/B of per-posterior diagnostics on one GPU: the per-slice loop -- ``summarize(x[sl])`` for every group of a
targets.Batched job, the only way before ``chains_per_group`` -- against ONE ``summarize(x, chains_per_group=per)``
(lmc_diag_chain_stats_grouped), plain and rank-normalised, on synthetic AR(1) draws in HBM.

    python tools/ab_grouped_diagnostics.py                          # 256 groups x 64 chains x 500 draws x d = 32
    python tools/ab_grouped_diagnostics.py --c3 --parent-lib build_variants/liblmc_diag_parent.so

Every variant is warmed up first (the first call of a process loads code objects), then the variants are timed alternately
(A B A B ...), one JSON line per (variant, repeat): a host clock around the call, which ends in a device synchronise. Drift of
the box shows up as disagreement between repeats, so read the spread before the difference. The results of the two ways
are compared as well (faster and different is not faster).

``--c3``: the ungrouped call at the size of BASELINE's C3 trace (65536 chains x 1000 draws x d = 128, 67 GB), two halves of
lag block 0 as ``summarize`` issues them, through the C entry. ``--parent-lib`` names a library that exports
lmc_diag_chain_stats built from csrc/lmc_diag.hip of a commit before lmc_diag_chain_stats_grouped, where that file is
self-contained (``hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared -mllvm -disable-machine-licm``;
since then it calls lmc_target_param_row of lmc_engine.hip and is measured as part of the library); the two
libraries alternate on the same tensor and their outputs are compared bit for bit."""
import argparse
import ctypes
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--groups", type=int, default=256)
    ap.add_argument("--per", type=int, default=64, help="chains per group")
    ap.add_argument("--draws", type=int, default=500)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--rho", type=float, default=0.5, help="AR(1) coefficient of the synthetic draws")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-groups", action="store_true", help="only the --c3 measurement")
    ap.add_argument("--c3", action="store_true", help="also time the ungrouped call at the size of the C3 trace")
    ap.add_argument("--c3-shape", type=int, nargs=3, default=[65536, 1000, 128], metavar=("CHAINS", "DRAWS", "DIM"))
    ap.add_argument("--parent-lib", default=None, help="a library with another commit's lmc_diag_chain_stats")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    from littlemcmc_amd import _abi, _build
    from littlemcmc_amd import diagnostics as dg

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

    def ar1(chains, n, d, rho, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        x = torch.empty((chains, n, d), dtype=torch.float64, device="cuda")
        x[:, 0] = torch.randn((chains, d), dtype=torch.float64, device="cuda", generator=g)
        for t in range(1, n):
            x[:, t] = rho * x[:, t - 1] + (1 - rho ** 2) ** 0.5 * torch.randn((chains, d), dtype=torch.float64, device="cuda",
                                                                                generator=g)
        return x

    if not args.skip_groups:
        G, per = args.groups, args.per
        x = ar1(G * per, args.draws, args.dim, args.rho, 20260928)
        slices = [slice(g * per, (g + 1) * per) for g in range(G)]
        shape = {"groups": G, "chains_per_group": per, "draws": args.draws, "dim": args.dim}
        for rn in (False, True):
            variants = {
                "per_slice_loop": lambda: [dg.summarize(x[sl], rank_normalized=rn) for sl in slices],
                "grouped": lambda: dg.summarize(x, chains_per_group=per, rank_normalized=rn),
            }
            warm = {name: timed(fn) for name, fn in variants.items()}
            loop, grouped = warm["per_slice_loop"][1], warm["grouped"][1]
            rhat = torch.stack([r["rhat"] for r in loop])
            ess = torch.stack([r["ess"] for r in loop])
            emit(dict(shape, what="agreement", rank_normalized=rn, rhat_max_rel_diff=float(((rhat - grouped["rhat"]).abs() / rhat).max()),
                      ess_max_rel_diff=float(((ess - grouped["ess"]).abs() / ess).max()),
                      lag_passes_grouped=grouped["lag_passes"], lag_passes_loop_max=max(r["lag_passes"] for r in loop),
                      first_call_seconds={k: v[0] for k, v in warm.items()}))
            for rep in range(args.repeats):
                for name, fn in variants.items():
                    emit(dict(shape, what="time", variant=name, rank_normalized=rn, repeat=rep, seconds=timed(fn)[0]))
        del x

    if args.c3:
        chains, n, d = args.c3_shape
        x = torch.empty((chains, n, d), dtype=torch.float64, device="cuda")
        step = max(1, (1 << 28) // (n * d))
        for lo in range(0, chains, step):                       # filled in slabs: no second tensor of this size
            x[lo:lo + step].normal_()
        h = n // 2
        libs = {"this": _abi.load()}
        if args.parent_lib:
            parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
            parent.lmc_diag_chain_stats.restype = ctypes.c_int
            parent.lmc_diag_chain_stats.argtypes = libs["this"].lmc_diag_chain_stats.argtypes
            libs["parent"] = parent
        stream = torch.cuda.current_stream().cuda_stream

        def call(lib):
            outs = []
            for t0 in (0, n - h):
                out = torch.empty((19, d), dtype=torch.float64, device="cuda")
                rc = lib.lmc_diag_chain_stats(ctypes.c_void_p(x.data_ptr()), chains, n, d, t0, h, 0, ctypes.c_void_p(out.data_ptr()),
                                              ctypes.c_void_p(stream))
                assert rc == 0, rc
                outs.append(out)
            return torch.stack(outs)

        warm = {name: timed(lambda lib=lib: call(lib)) for name, lib in libs.items()}
        shape = {"chains": chains, "draws": n, "dim": d, "trace_gb": chains * n * d * 8 / 1e9}
        emit(dict(shape, what="c3_agreement", first_call_seconds={k: v[0] for k, v in warm.items()},
                  bit_equal_to_parent=bool(torch.equal(warm["this"][1], warm["parent"][1])) if "parent" in warm else None))
        for rep in range(args.repeats):
            for name, lib in libs.items():
                emit(dict(shape, what="c3_time", variant=name, repeat=rep, seconds=timed(lambda: call(lib))[0]))


if __name__ == "__main__":
    main()
