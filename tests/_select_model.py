"""Numpy restatement of the radix select behind the posterior quantiles (include/lmc_hip.h: lmc_select_digit_counts;
littlemcmc_amd/diagnostics.py: order_statistics): the key, ONE count call with its group / first_chain / t0 conventions, and
the eight-pass select of one column. The GPU tests compare the kernel's counts with ``digit_counts`` exactly; the CPU tests
inject ``count_fn`` for the HIP call and compare the host logic with np.sort."""
import numpy as np
import torch

MAX_RANKS = 16
SHIFTS = (56, 48, 40, 32, 24, 16, 8, 0)
TOP = np.uint64(1) << np.uint64(63)


def key(v):
    """K(v): the IEEE total order on the bits as an unsigned integer (-NaN < -inf < .. < -0 < +0 < .. < +inf < +NaN)."""
    u = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | TOP)


def unkey(k):
    """The draw whose key is k."""
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k >> np.uint64(63) != 0, k & ~TOP, ~k).view(np.float64)


def touched(first_chain, chains, per):
    g0 = first_chain // per
    return g0, (first_chain + chains - 1) // per - g0 + 1


def digit_counts(x, t0, n, first_chain, per, shift, prefix=None, n_ranks=1):
    """One call: x[chains, draws_stride, d] float64 whose chain 0 is chain ``first_chain`` of the job, rows [t0, t0 + n),
    ``per`` chains a group; prefix [groups touched, n_ranks, d] uint64 (not read at shift 56)
    -> counts [groups touched, n_ranks, 256, d] int64."""
    c, _stride, d = x.shape
    g0, groups = touched(first_chain, c, per)
    if shift == 56:
        assert n_ranks == 1
    else:
        prefix = np.asarray(prefix, dtype=np.uint64)
        n_ranks = prefix.shape[1]
        assert prefix.shape == (groups, n_ranks, d)
    out = np.zeros((groups, n_ranks, 256, d), dtype=np.int64)
    cols = np.arange(d)
    for g in range(groups):
        lo, hi = max((g0 + g) * per - first_chain, 0), min((g0 + g + 1) * per - first_chain, c)
        k = key(x[lo:hi, t0:t0 + n]).reshape(-1, d)
        digit = ((k >> np.uint64(shift)) & np.uint64(255)).astype(np.int64)
        for r in range(n_ranks):
            if shift == 56:
                match = np.ones(k.shape, dtype=bool)
            else:
                hs = np.uint64(shift + 8)
                match = (k >> hs) == (prefix[g, r][None, :] >> hs)
            np.add.at(out[g, r], (digit[match], np.broadcast_to(cols, k.shape)[match]), 1)
    return out


def select(col, ranks):
    """The eight-pass select of one column: the ``ranks``-th smallest values (0-based) in the order of ``key``."""
    x = np.asarray(col, dtype=np.float64).reshape(1, -1, 1)
    ranks = [int(r) for r in ranks]
    out = []
    for q0 in range(0, len(ranks), MAX_RANKS):
        rem = np.array(ranks[q0:q0 + MAX_RANKS], dtype=np.int64)
        prefix = np.zeros((1, len(rem), 1), dtype=np.uint64)
        for shift in SHIFTS:
            cnt = digit_counts(x, 0, x.shape[1], 0, 1, shift, prefix, 1)[0, :, :, 0]
            if shift == 56:
                cnt = np.broadcast_to(cnt, (len(rem), 256))
            cum = np.cumsum(cnt, axis=1)
            bucket = (cum <= rem[:, None]).sum(axis=1)
            assert bucket.max() < 256, "a rank beyond the column"
            below = np.where(bucket > 0, cum[np.arange(len(rem)), np.maximum(bucket - 1, 0)], 0)
            rem = rem - below
            prefix[0, :, 0] |= bucket.astype(np.uint64) << np.uint64(shift)
        out.append(unkey(prefix[0, :, 0]))
    return np.concatenate(out)


def count_fn(x, first_chain, per, shift, prefix):
    """``count_fn`` of diagnostics.order_statistics: the model in place of the HIP call (torch in, torch out; the prefix
    travels as int64 bits)."""
    pf = None if prefix is None else prefix.detach().cpu().numpy().view(np.uint64)
    xn = x.detach().cpu().numpy().astype(np.float64, copy=False)
    return torch.from_numpy(digit_counts(xn, 0, xn.shape[1], int(first_chain), int(per), int(shift), pf)).to(x.device)


def key_sorted(pool):
    """The pool in the order of the key (np.sort would put -NaN last and leaves the order of -0 / +0 open)."""
    pool = np.asarray(pool, dtype=np.float64).ravel()
    return pool[np.argsort(key(pool), kind="stable")]


def hostile_column():
    """365 values: +-0, +-inf, +-denormal, +-max-double, a run of 40 ties, a run of 17 ties, and ordinary draws."""
    rng = np.random.default_rng(7)
    tiny, big = 5e-324, np.finfo(np.float64).max
    special = [0.0, -0.0, np.inf, -np.inf, tiny, -tiny, 3 * tiny, -3 * tiny, big, -big]
    col = np.concatenate([special, np.full(40, 0.25), np.full(17, -1.5), rng.standard_normal(365 - 67) * 3.0])
    assert col.shape == (365,)
    return rng.permutation(col)


def quantile_formula(pool_sorted, p):
    """The documented interpolation: h = p (S - 1), lo = floor(h), q = v[lo] + (v[min(lo + 1, S - 1)] - v[lo]) (h - lo)."""
    S = len(pool_sorted)
    h = float(p) * (S - 1)
    lo = int(np.floor(h))
    hi = min(lo + 1, S - 1)
    return pool_sorted[lo] + (pool_sorted[hi] - pool_sorted[lo]) * (h - lo)
