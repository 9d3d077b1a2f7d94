"""Numpy restatement of ONE call of lmc_diag_threshold_counts (include/lmc_hip.h; littlemcmc_amd/diagnostics.py:
threshold_counts): its group / first_chain / t0 conventions and the definition in three lines. The GPU tests compare the
kernel's counts with ``counts`` exactly; the CPU tests inject ``count_fn`` for the HIP call."""
import numpy as np
import torch

MAX_THRESHOLDS = 16


def touched(first_chain, chains, per):
    g0 = first_chain // per
    return g0, (first_chain + chains - 1) // per - g0 + 1


def counts(x, t0, n, first_chain, per, thresholds):
    """One call: x[chains, draws_stride, d] float64 whose chain 0 is chain ``first_chain`` of the job, rows [t0, t0 + n),
    ``per`` chains a group (a first or last group that lies only partly in x is counted over its chains that are present);
    thresholds [groups touched, K, d] -> counts [groups touched, 2 K + 1, d] int64. IEEE numeric comparisons."""
    c, _stride, d = x.shape
    g0, groups = touched(first_chain, c, per)
    thresholds = np.asarray(thresholds, dtype=np.float64)
    K = thresholds.shape[1]
    assert thresholds.shape == (groups, K, d) and 1 <= K <= MAX_THRESHOLDS
    out = np.zeros((groups, 2 * K + 1, d), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for g in range(groups):
            lo, hi = max((g0 + g) * per - first_chain, 0), min((g0 + g + 1) * per - first_chain, c)
            v = x[lo:hi, t0:t0 + n].reshape(-1, 1, d)
            out[g, 0:2 * K:2] = (v < thresholds[g][None]).sum(axis=0)
            out[g, 1:2 * K:2] = (v == thresholds[g][None]).sum(axis=0)
            out[g, 2 * K] = (v != v).sum(axis=0)[0]
    return out


def count_fn(x, first_chain, per, thresholds):
    """``count_fn`` of diagnostics.threshold_counts: the model in place of the HIP call (torch in, torch out)."""
    xn = x.detach().cpu().numpy().astype(np.float64, copy=False)
    th = thresholds.detach().cpu().numpy()
    return torch.from_numpy(counts(xn, 0, xn.shape[1], int(first_chain), int(per), th)).to(x.device)
