"""Pointwise predictive statistics of a GLM posterior from the draws where they lie (HBM): lppd, WAIC, held-out scoring.

Everything WAIC and a held-out score need from the pointwise log-likelihood ``l[s, n]`` (draw s, observation n) is a
handful of statistics per observation that MERGE over blocks of draws -- chains, chain blocks, GPUs:

    n (draws), m = max_s l, S = sum_s exp(l - m), mean_s l, M2 = sum_s (l - mean)^2, sum_s mu

They come from one streaming pass of the HIP kernel ``lmc_glm_pointwise`` (csrc/lmc_predict.hip) over the trace; the array
``l`` itself -- N / d times the size of the trace -- is never written. ``l`` is the device functor's ``l_n`` (``targets.GLM``:
constants that do not depend on the coefficients dropped); :func:`finalize` adds ``GLM.loglik_constant()`` back. There is
one backend, the HIP kernel; the merge / finalise logic above it is plain tensor code, and its CPU tests inject a numpy
restatement of the kernel's block through ``stats_fn`` (as ``diagnostics.summarize`` does)."""
import ctypes
import weakref

import numpy as np
import torch

from . import diagnostics

PLANES = ("n", "m", "S", "mean", "M2", "sum_mu")
HIGH_VARIANCE = 0.4   # p_waic_i beyond which WAIC is unreliable for that observation (Vehtari, Gelman, Gabry 2017)

_device_rows = weakref.WeakKeyDictionary()   # target -> {device: its parameter table in HBM}


def merge(a, b):
    """Two blocks ``[..., 6, N]`` of the six planes, over disjoint sets of draws -> the block over their union:
    m = max(ma, mb), S = Sa exp(ma - m) + Sb exp(mb - m), Chan's update of (mean, M2), sums for the count and sum mu.
    A side of count 0 is skipped BY ITS COUNT: the other side comes through bit for bit, whatever the empty side holds."""
    na, ma, Sa, mea, M2a, mua = a.unbind(-2)
    nb, mb, Sb, meb, M2b, mub = b.unbind(-2)
    n = na + nb
    hi, lo = torch.maximum(ma, mb), torch.minimum(ma, mb)
    e = torch.where(torch.isneginf(lo), torch.zeros_like(lo), torch.exp(lo - hi))   # (-inf) - (-inf) is never used
    S = torch.where(ma >= mb, Sa + Sb * e, Sa * e + Sb)
    safe = torch.where(n > 0, n, torch.ones_like(n))
    delta = meb - mea
    mean = mea + delta * (nb / safe)
    M2 = (M2a + M2b) + (delta * delta) * (na * nb / safe)
    both = torch.stack([n, hi, S, mean, M2, mua + mub], dim=-2)
    only_a, only_b = (nb == 0).unsqueeze(-2), (na == 0).unsqueeze(-2)
    return torch.where(only_a, a, torch.where(only_b, b, both))


def _members(target):
    from .targets import GLM, Batched

    if isinstance(target, GLM):
        return [target]
    if isinstance(target, Batched) and isinstance(target.members[0], GLM):
        return list(target.members)
    raise TypeError("pointwise predictive statistics are those of a targets.GLM or a targets.Batched of GLM members "
                    "(the family that carries its data); got %r" % (target,))


def _scored(target, members, data):
    """(table[G, row_len] (host), the GLMs whose y and constants apply) for the training data or for held-out ``data``."""
    from .targets import GLM, Batched

    if data is None:
        return np.ascontiguousarray(target.params, dtype=np.float64).reshape(len(members), -1), members
    if isinstance(target, Batched):
        pairs = list(data)
        if len(pairs) != len(members) or any(not isinstance(p, (tuple, list)) or len(p) != 2 for p in pairs):
            raise ValueError("data= for a Batched of %d groups is a list of %d pairs (X_new, y_new)" % (len(members), len(members)))
    else:
        if not isinstance(data, (tuple, list)) or len(data) != 2:
            raise ValueError("data= is a pair (X_new, y_new)")
        pairs = [data]
    held = [GLM(X, y, likelihood=m.likelihood, prior_scale=m.prior_scale, sigma=m.sigma) for m, (X, y) in zip(members, pairs)]
    for g, (h, m) in enumerate(zip(held, members)):
        if h.d != m.d:
            raise ValueError("data= of group %d has d = %d, the posterior d = %d" % (g, h.d, m.d))
        if h.n_obs != held[0].n_obs:
            raise ValueError("data= of group %d has N = %d, group 0 N = %d: one common N" % (g, h.n_obs, held[0].n_obs))
    return np.stack([h.params for h in held]), held


def _hip_pointwise(x, table, first_chain, per):
    """One call of lmc_glm_pointwise: x[chains, draws, d] (float64, _row_major, on a ROCm device), table[n_rows, row_len] on
    the same device -> [groups touched, 6, npad]."""
    from . import _abi
    from .targets import glm_row_layout

    lib = _abi.load()
    c, n, d = x.shape
    stride = x.stride(0) // d if c > 1 else n
    n_rows, row_len = table.shape
    npad = (row_len - _abi.GLM_HEADER) // (glm_row_layout(1, d)["size"] - _abi.GLM_HEADER) * 64
    out = torch.empty((diagnostics._touched(first_chain, c, per)[1], len(PLANES), npad), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        rc = lib.lmc_glm_pointwise(ctypes.c_void_p(x.data_ptr()), c, stride, d, 0, n, ctypes.c_void_p(table.data_ptr()),
                                   row_len, n_rows, int(first_chain), int(per), ctypes.c_void_p(out.data_ptr()),
                                   ctypes.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("lmc_glm_pointwise failed (status %d)" % rc)
    return out


def _table_on(target, table, device, cache):
    if not cache:
        return torch.as_tensor(table).to(device)
    held = _device_rows.setdefault(target, {})
    key = str(device)
    if key not in held:
        held[key] = torch.as_tensor(table).to(device)
    return held[key]


def pointwise_stats(x, target, data=None, chains_per_group=None, first_chain=0, stats_fn=None, group=None):
    """The six planes ``n, m, S, mean, M2, sum_mu`` of the pointwise log-likelihood, a dict of float64 tensors ``[G, N]`` on
    x's device (one group: a leading axis of 1).

    ``x``: the draws, a float64 ROCm tensor ``[chains, draws, d]`` (``diagnostics.trace_tensor(engine)``), or the list of
    per-GPU blocks of one job (``trace_tensor(engine_group)``): each block is passed on its own device at its running
    ``first_chain`` and the partial blocks are merged on the first block's device -- a group that straddles two devices is
    the merge of its parts. ``target``: the ``GLM``, or the ``Batched`` of ``GLM`` members, whose chains these are;
    ``chains_per_group`` defaults to all chains for a ``GLM`` and to ``target.group_size(chains)`` for a ``Batched``.
    ``first_chain``: x's chain 0 is that chain of the job (one tensor only). ``data=(X_new, y_new)`` -- for a ``Batched`` a
    list of G such pairs with one common N -- scores held-out data under the posterior draws: the same ``d``, ``y`` validated
    as ``GLM`` validates it, any N. ``stats_fn(x, table, first_chain, per) -> [groups touched, 6, >= N]`` replaces the HIP
    call (tests of the merge and finalise logic only; ``table`` is then the host table of parameter rows)."""
    from .targets import Batched

    members = _members(target)
    if group is not None or diagnostics._group_active(group):
        raise ValueError("pointwise predictive statistics are a one-process matter: group= / an active process group "
                         "(sample_distributed) is not supported")
    is_list = isinstance(x, (list, tuple))
    blocks = list(x) if is_list else [x]
    first_chain = int(first_chain)
    if is_list and first_chain != 0:
        raise ValueError("first_chain=%d with a list of blocks: the list is the whole job, its first block starts at chain 0"
                         % first_chain)
    if not blocks or any(b.dim() != 3 for b in blocks):
        raise ValueError("x must be [chains, draws, d] or a list of such blocks")
    held = [b for b in blocks if b.shape[0] > 0]
    if not held:
        raise ValueError("x holds no chain")
    if len({(int(b.shape[1]), int(b.shape[2])) for b in held}) > 1:
        raise ValueError("the chain blocks differ in draws per chain or in d: %s" % [tuple(b.shape[1:]) for b in held])
    n_draws, d = int(held[0].shape[1]), int(held[0].shape[2])
    if d != members[0].d:
        raise ValueError("x has d = %d, the target d = %d" % (d, members[0].d))
    if n_draws < 1:
        raise ValueError("x holds no draw")
    chains = sum(int(b.shape[0]) for b in blocks)
    if chains_per_group is None:
        per = target.group_size(chains) if isinstance(target, Batched) and first_chain == 0 else None
        if per is None:
            if isinstance(target, Batched):
                raise ValueError("a block of a Batched job that starts at first_chain=%d needs chains_per_group" % first_chain)
            per = first_chain + chains
    else:
        per = int(chains_per_group)
    if per < 1 or first_chain < 0:
        raise ValueError("chains_per_group must be >= 1 and first_chain >= 0 (got %d, %d)" % (per, first_chain))
    g0, touched = diagnostics._touched(first_chain, chains, per)
    if g0 + touched > len(members):
        raise ValueError("chains %d .. %d at %d chains per group reach group %d; the target has %d"
                         % (first_chain, first_chain + chains - 1, per, g0 + touched - 1, len(members)))
    table, scored = _scored(target, members, data)
    n_obs = scored[0].n_obs
    dev = blocks[0].device
    parts, f = [], first_chain
    for b in blocks:   # one kernel per device, all enqueued before the first result is moved
        c = int(b.shape[0])
        if c > 0:
            if stats_fn is not None:
                blk = stats_fn(b, table, f, per)
            else:
                b = diagnostics._device_block(b)
                blk = _hip_pointwise(b, _table_on(target, table, b.device, data is None), f, per)
            parts.append((f // per - g0, blk[..., :n_obs]))
        f += c
    tot = torch.zeros((touched, len(PLANES), n_obs), dtype=torch.float64, device=dev)
    for off, blk in parts:
        blk = blk.to(dev)
        tot[off:off + blk.shape[0]] = merge(tot[off:off + blk.shape[0]], blk)
    out = {name: tot[:, i] for i, name in enumerate(PLANES)}
    out["first_group"] = g0
    return out


def _const(target, data, stats):
    members = _members(target)
    _table, scored = _scored(target, members, data)
    g0, G = int(stats.get("first_group", 0)), int(stats["n"].shape[0])
    c = np.stack([m.loglik_constant() for m in scored[g0:g0 + G]])
    return torch.as_tensor(c, dtype=torch.float64).to(stats["n"].device)


def finalize(stats, const):
    """The planes of :func:`pointwise_stats` and the dropped constant ``const`` (``[N]`` or ``[G, N]``:
    ``GLM.loglik_constant()``) -> ``lppd[G, N] = m + log S - log n + const`` (the log of the posterior-mean predictive
    density of the point), ``p_waic[G, N] = M2 / (n - 1)`` (the posterior variance of its log-likelihood),
    ``elpd_waic_i = lppd - p_waic``, ``mean_loglik = mean + const``, ``mu_mean = sum_mu / n`` (the posterior mean response)."""
    n = stats["n"]
    const = torch.as_tensor(const, dtype=torch.float64).to(n.device)
    lppd = stats["m"] + torch.log(stats["S"]) - torch.log(n) + const
    p_waic = stats["M2"] / (n - 1.0)
    return dict(lppd=lppd, p_waic=p_waic, elpd_waic_i=lppd - p_waic, mean_loglik=stats["mean"] + const,
                mu_mean=stats["sum_mu"] / n, n_draws=n)


def waic(x, target, data=None, **kw):
    """WAIC of a ``GLM`` (leading axis 1) or of every posterior of a ``Batched`` of GLMs (leading axis G), from the draws in
    HBM: :func:`finalize` of :func:`pointwise_stats` plus ``elpd_waic[G] = sum_n elpd_waic_i``, ``p_waic_total[G]``,
    ``se[G] = sqrt(N var_n(elpd_waic_i))``, ``waic[G] = -2 elpd_waic`` and ``n_high_variance[G]``, the number of observations
    with ``p_waic_i > 0.4`` (where WAIC is unreliable: Vehtari, Gelman, Gabry 2017). Higher ``elpd_waic`` is better.

    ``data=(X_new, y_new)`` (a ``Batched``: a list of G pairs) scores held-out points instead. Their ``lppd`` -- the log
    predictive density of each point under the posterior -- IS then the quantity of interest (its sum over the fold is the
    fold's score); ``p_waic`` corrects an in-sample lppd and has no meaning for held-out data."""
    stats = pointwise_stats(x, target, data=data, **kw)
    out = finalize(stats, _const(target, data, stats))
    e = out["elpd_waic_i"]
    N = e.shape[-1]
    out["elpd_waic"] = e.sum(dim=-1)
    out["p_waic_total"] = out["p_waic"].sum(dim=-1)
    out["se"] = torch.sqrt(N * e.var(dim=-1)) if N > 1 else torch.full_like(out["elpd_waic"], float("nan"))
    out["waic"] = -2.0 * out["elpd_waic"]
    out["n_high_variance"] = (out["p_waic"] > HIGH_VARIANCE).sum(dim=-1)
    out["lppd_total"] = out["lppd"].sum(dim=-1)
    return out
