"""Posterior quantiles of a trace in HBM: diagnostics.quantiles (the radix select of csrc/lmc_select.hip, the trace read in
place) next to a torch baseline on the same tensor -- a chunked transposed copy and torch.sort, the way
_rank_normalize_grouped does it, then indexing and the same interpolation. Synthetic float64 draws of the README's GLM shape
by default (16 384 chains x 500 draws x d = 32, 64 chains per posterior), probs = (0.05, 0.5, 0.95).

Both paths are warmed up, then timed alternately (--repeats times each, a device synchronise inside every timing); the line
reports the median, the minimum and the maximum of each, the peak extra device memory of each (max_memory_allocated above what
was allocated before the call), whether the two agree bit for bit, and the achieved bytes/s of the select against the trace
volume x the reads of its passes. One JSON line.

    python tools/quantile_rate.py [--chains C --draws N --dim D --per P --chunk-dims K --repeats R --warmup W]"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from littlemcmc_amd import _abi  # noqa: E402
from littlemcmc_amd import diagnostics as dg  # noqa: E402


def sort_quantiles(x, probs, per, chunk_dims):
    """The torch baseline: [G, Q, d] by sorting a transposed copy of ``chunk_dims`` dimensions at a time."""
    c, n, d = x.shape
    G, S = c // per, per * n
    h = [p * (S - 1) for p in probs]
    lo = [int(math.floor(v)) for v in h]
    hi = [min(k + 1, S - 1) for k in lo]
    frac = torch.tensor([a - b for a, b in zip(h, lo)], dtype=torch.float64, device=x.device).reshape(1, 1, -1)
    lo_t, hi_t = torch.tensor(lo, device=x.device), torch.tensor(hi, device=x.device)
    out = torch.empty((G, len(probs), d), dtype=torch.float64, device=x.device)
    for a in range(0, d, chunk_dims):
        b = min(a + chunk_dims, d)
        blk = x[:, :, a:b].reshape(G, S, b - a).transpose(1, 2).contiguous()      # [G, k, S]
        srt = torch.sort(blk, dim=2).values
        vlo, vhi = srt.index_select(2, lo_t), srt.index_select(2, hi_t)
        out[:, :, a:b] = (vlo + (vhi - vlo) * frac).transpose(1, 2)
    return out


def select_reads(d, n_ranks):
    """How many times the eight passes of one round read the trace: once at shift 56, ceil(ranks / slots of a block) times at
    each of the other seven (csrc/lmc_select.hip: 8, 4 or 2 slots at table widths 16, 32, 64)."""
    slots = 8 if d <= 16 else (4 if d <= 32 else 2)
    return 1 + 7 * -(-n_ranks // slots)


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
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--draws", type=int, default=500)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--per", type=int, default=64)
    ap.add_argument("--chunk-dims", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise _abi.HipLibraryError("quantile_rate.py measures on a GPU; there is none")
    probs = (0.05, 0.5, 0.95)
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((a.chains, a.draws, a.dim), dtype=torch.float64, device="cuda", generator=gen)
    x += torch.arange(a.dim, dtype=torch.float64, device="cuda")                  # one scale, a location per coordinate
    paths = {"select": lambda: dg.quantiles(x, probs, chains_per_group=a.per)["quantiles"],
             "sort": lambda: sort_quantiles(x, probs, a.per, a.chunk_dims)}
    for _ in range(a.warmup):
        for fn in paths.values():
            fn()
    times, peaks, outs = {k: [] for k in paths}, {k: 0 for k in paths}, {}
    for _ in range(a.repeats):
        for name, fn in paths.items():                                             # alternated
            outs[name], dt, peak = timed(fn)
            times[name].append(dt)
            peaks[name] = max(peaks[name], peak)
    S = a.per * a.draws
    ranks = {0, S - 1}
    for p in probs:
        lo = int(math.floor(p * (S - 1)))
        ranks |= {lo, min(lo + 1, S - 1)}
    reads = select_reads(a.dim, len(ranks))
    trace_bytes = 8 * a.chains * a.draws * a.dim
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    line = {"tool": "quantile_rate", "build": _abi.load().lmc_build_hash().decode(), "chains": a.chains, "draws": a.draws,
            "dim": a.dim, "per": a.per, "probs": probs, "chunk_dims": a.chunk_dims, "repeats": a.repeats, "warmup": a.warmup,
            "trace_bytes": trace_bytes, "distinct_ranks": len(ranks), "select_trace_reads": reads,
            "equal_bits": bool(torch.equal(outs["select"], outs["sort"]))}
    for k in paths:
        line[k + "_s"] = {"median": med[k], "min": min(times[k]), "max": max(times[k])}
        line[k + "_peak_extra_bytes"] = peaks[k]
    line["select_algorithmic_bytes_per_s"] = trace_bytes * reads / med["select"]
    line["sort_over_select"] = med["sort"] / med["select"]
    print(json.dumps(line))


if __name__ == "__main__":
    main()
