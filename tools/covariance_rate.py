"""Posterior covariance per posterior of a trace in HBM: diagnostics.covariance (the FP64 MFMA pass of csrc/lmc_cross.hip, the
trace read in place) next to the torch statement of the same result on the same tensor -- x.reshape(G, per * n, d), subtract
the mean, torch.baddbmm, in float64. Synthetic float64 draws at two shapes by default: the README's GLM shape (256 posteriors
x 64 chains x 500 draws x d = 32) and 64 x 64 x 500 x d = 128.

Both paths are warmed up, then timed alternately (--repeats times each, a device synchronise inside every timing); a line
reports the median, the minimum and the maximum of each, the peak extra device memory of each -- torch's max_memory_allocated
above what was allocated before the call, which for the kernel holds its outputs, plus the stream-ordered scratch of the call
(partials, column sums and shifts, restated from the plan of csrc/lmc_cross.hip) -- the largest entry-wise difference of the
two covariances in units of the bound of tests/_cross_model.py (N 2^-52 (a^T a) / (N - 1), a = |x - mean|, evaluated on the
device in float64), and the achieved bytes/s against two reads of the trace. One JSON line per shape.

    python tools/covariance_rate.py [--shapes G,per,n,d ... --repeats R --warmup W]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from littlemcmc_amd import _abi  # noqa: E402
from littlemcmc_amd import diagnostics as dg  # noqa: E402

EPS = 2.0 ** -52


def torch_covariance(x, per):
    """The torch baseline: cov[G, d, d] from a centred copy of the trace and one batched matmul."""
    c, n, d = x.shape
    rows = x.reshape(c // per, per * n, d)
    dev = rows - rows.mean(dim=1, keepdim=True)
    out = torch.zeros((c // per, d, d), dtype=torch.float64, device=x.device)
    return torch.baddbmm(out, dev.transpose(1, 2), dev) / (per * n - 1.0)


def bound(x, per):
    """tol_m2 / (N - 1) of tests/_cross_model.py per entry, [G, d, d], on the device (its s term is zero to rounding)."""
    c, n, d = x.shape
    rows = x.reshape(c // per, per * n, d)
    a = (rows - rows.mean(dim=1, keepdim=True)).abs_()
    N = per * n
    return torch.bmm(a.transpose(1, 2), a) * (N * EPS / (N - 1.0))


def kernel_scratch_bytes(groups, per, n, d):
    """The hipMallocAsync scratch of one lmc_diag_cross_moments call (csrc/lmc_cross.hip: cross_plan)."""
    ntl = 1 if d <= 16 else (2 if d <= 32 else (4 if d <= 64 else 8))
    kc = 128 if ntl <= 2 else (64 if ntl == 4 else 32)
    nt = (d + 15) // 16
    mb = (nt + 7) // 8 if ntl == 8 else 1
    items = per * ((n + kc - 1) // kc)
    w = max(1, min(items, 1024 // (groups * (mb * (mb + 1) // 2))))
    ipw = (items + w - 1) // w
    wpg = (items + ipw - 1) // ipw
    return 8 * (groups * wpg * (nt * (nt + 1) // 2 * 256 + 16 * nt) + groups * 16 * nt)


def timed(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    return out, dt, torch.cuda.max_memory_allocated() - base


def measure(G, per, n, d, repeats, warmup):
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((G * per, n, d), dtype=torch.float64, device="cuda", generator=gen)
    x += torch.arange(d, dtype=torch.float64, device="cuda")                      # one scale, a location per coordinate
    paths = {"kernel": lambda: dg.covariance(x, chains_per_group=per)["cov"], "torch": lambda: torch_covariance(x, per)}
    for _ in range(warmup):
        for fn in paths.values():
            fn()
    times, peaks, outs = {k: [] for k in paths}, {k: 0 for k in paths}, {}
    for _ in range(repeats):
        for name, fn in paths.items():                                             # alternated
            outs[name], dt, peak = timed(fn)
            times[name].append(dt)
            peaks[name] = max(peaks[name], peak)
    peaks["kernel"] += kernel_scratch_bytes(G, per, n, d)
    diff = float(((outs["kernel"] - outs["torch"]).abs() / bound(x, per)).max())
    trace_bytes = 8 * G * per * n * d
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    line = {"tool": "covariance_rate", "build": _abi.load().lmc_build_hash().decode(), "groups": G, "per": per, "draws": n, "dim": d,
            "repeats": repeats, "warmup": warmup, "trace_bytes": trace_bytes, "max_diff_over_bound": diff}
    for k in paths:
        line[k + "_s"] = {"median": med[k], "min": min(times[k]), "max": max(times[k])}
        line[k + "_peak_extra_bytes"] = peaks[k]
    line["kernel_algorithmic_bytes_per_s"] = 2 * trace_bytes / med["kernel"]
    line["kernel_fma_per_s"] = G * per * n * (16 * ((d + 15) // 16)) ** 2 / 2 / med["kernel"]
    line["torch_over_kernel"] = med["torch"] / med["kernel"]
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=["256,64,500,32", "64,64,500,128"], help="G,per,n,d")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise _abi.HipLibraryError("covariance_rate.py measures on a GPU; there is none")
    for s in a.shapes:
        G, per, n, d = (int(v) for v in s.split(","))
        measure(G, per, n, d, a.repeats, a.warmup)


if __name__ == "__main__":
    main()
