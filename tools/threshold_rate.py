"""Threshold counts of a trace in HBM: diagnostics.threshold_counts (csrc/lmc_threshold.hip, the trace read in place, once for
all thresholds) next to what a user would write in torch on the same tensor -- a loop over the thresholds of

    (x.view(G, per, n, d) < c[:, None, None, :]).sum((1, 2))      and the same with ==

in float64, which makes a boolean temporary an eighth the size of the trace per comparison. Synthetic float64 draws at the
README's GLM shape (256 posteriors x 64 chains x 500 draws x d = 32) with K = 1 and K = 8 thresholds, and at 64 x 64 x 500 x d =
128, by default.

Both paths are warmed up, then timed alternately (--repeats times each, a host clock around work that ends in a device
synchronise); a line reports the median, the minimum and the maximum of each, the peak extra device memory of each (torch's
max_memory_allocated above what was allocated before the call; the kernel's holds its thresholds and counts), whether the two
results are equal (they are integers), and the kernel path's achieved bytes/s against ONE read of the trace, as a share of
the HBM peak (bench.HBM_PEAK) and of the rate a plain device copy of the same trace reaches in this run (2 x trace bytes over
its time: the streaming rate this machine gives torch). The kernel figure is a whole-call rate -- host logic, memset and
launch included -- not a kernel's share of peak. One JSON line per shape. No number is a pass / fail criterion.

    python tools/threshold_rate.py [--shapes G,per,n,d,K ... --repeats R --warmup W]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from littlemcmc_amd import _abi  # noqa: E402
from littlemcmc_amd import diagnostics as dg  # noqa: E402

HBM_PEAK = 8.0e12   # bench.HBM_PEAK


def torch_counts(x, per, thr):
    """The torch baseline: (less, equal) [G, K, d] int64, one threshold at a time."""
    c, n, d = x.shape
    v = x.view(c // per, per, n, d)
    less = torch.stack([(v < thr[:, k, None, None, :]).sum((1, 2)) for k in range(thr.shape[1])], dim=1)
    equal = torch.stack([(v == thr[:, k, None, None, :]).sum((1, 2)) for k in range(thr.shape[1])], dim=1)
    return less, equal


def timed(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    return out, dt, torch.cuda.max_memory_allocated() - base


def measure(G, per, n, d, K, repeats, warmup):
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((G * per, n, d), dtype=torch.float64, device="cuda", generator=gen)
    thr = torch.randn((G, K, d), dtype=torch.float64, device="cuda", generator=gen)
    thr[:, 0] = x[::per, 0]                                                        # a threshold that ties with a draw

    def kernel():
        tc = dg.threshold_counts(x, thr, chains_per_group=per)
        return tc["less"], tc["equal"]

    paths = {"kernel": kernel, "torch": lambda: torch_counts(x, per, thr), "copy": lambda: x.clone()}
    for _ in range(warmup):
        for fn in paths.values():
            fn()
    times, peaks, outs = {k: [] for k in paths}, {k: 0 for k in paths}, {}
    for _ in range(repeats):
        for name, fn in paths.items():                                             # alternated
            outs[name], dt, peak = timed(fn)
            times[name].append(dt)
            peaks[name] = max(peaks[name], peak)
    same = all(torch.equal(a, b) for a, b in zip(outs["kernel"], outs["torch"]))
    del outs
    trace_bytes = 8 * G * per * n * d
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    line = {"tool": "threshold_rate", "build": _abi.load().lmc_build_hash().decode(), "groups": G, "per": per, "draws": n, "dim": d,
            "thresholds": K, "repeats": repeats, "warmup": warmup, "trace_bytes": trace_bytes, "results_equal": same}
    for k in paths:
        line[k + "_s"] = {"median": med[k], "min": min(times[k]), "max": max(times[k])}
        line[k + "_peak_extra_bytes"] = peaks[k]
    line["copy_bytes_per_s"] = 2 * trace_bytes / med["copy"]
    line["kernel_algorithmic_bytes_per_s"] = trace_bytes / med["kernel"]
    line["kernel_share_of_hbm_peak"] = line["kernel_algorithmic_bytes_per_s"] / HBM_PEAK
    line["kernel_share_of_copy_rate"] = line["kernel_algorithmic_bytes_per_s"] / line["copy_bytes_per_s"]
    line["torch_over_kernel"] = med["torch"] / med["kernel"]
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", nargs="+", default=["256,64,500,32,1", "256,64,500,32,8", "64,64,500,128,1", "64,64,500,128,8"],
                    help="G,per,n,d,K")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise _abi.HipLibraryError("threshold_rate.py measures on a GPU; there is none")
    for s in a.shapes:
        G, per, n, d, K = (int(v) for v in s.split(","))
        measure(G, per, n, d, K, a.repeats, a.warmup)


if __name__ == "__main__":
    main()
