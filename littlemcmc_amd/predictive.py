"""Pointwise predictive statistics of a GLM posterior from the draws where they lie (HBM): lppd, WAIC, held-out scoring.

Everything WAIC and a held-out score need from the pointwise log-likelihood ``l[s, n]`` (draw s, observation n) is a
handful of statistics per observation that MERGE over blocks of draws -- chains, chain blocks, GPUs:

    n (draws), m = max_s l, S = sum_s exp(l - m), mean_s l, M2 = sum_s (l - mean)^2, sum_s mu

They come from one streaming pass of the HIP kernel ``lmc_glm_pointwise`` (csrc/lmc_predict.hip) over the trace; the array
``l`` itself -- N / d times the size of the trace -- is never written. ``l`` is the device functor's ``l_n`` (``targets.GLM``:
constants that do not depend on the coefficients dropped); :func:`finalize` adds ``GLM.loglik_constant()`` back. There is
one backend, the HIP kernel; the merge / finalise logic above it is plain tensor code, and its CPU tests inject a numpy
restatement of the kernel's block through ``stats_fn`` (as ``diagnostics.summarize`` does).

Further down: PSIS-LOO (``psis``, ``loo``; csrc/lmc_psis.hip smooths the array that ``lmc_glm_pointwise_loglik`` of
csrc/lmc_predict.hip writes) and posterior predictions at new X (``linear_predictor``, ``predict``; csrc/lmc_linpred.hip) and
replicated responses (``replicate``, ``predict_response``, ``ppc``; csrc/lmc_yrep.hip),
each with its own kernel and its own injected model in the CPU tests; ``exceedance`` (P(prediction < t) at new points) counts
the written linear predictor with ``diagnostics.threshold_counts`` (csrc/lmc_threshold.hip).

What the passes over the trace share is stated once, in ``diagnostics``: ``_trace_job`` answers "what is x?" (one tensor or
the per-GPU blocks of a job, chains per group, the groups touched) with every refusal, each pass naming the rule it wants in
one line; ``_fan_out`` runs a kernel on every block's device and folds the parts with :func:`merge` / :func:`merge_moments`;
``_call_trace_kernel`` is the ctypes call; ``_quantile_plan`` / ``_interpolate`` are the quantiles of a select's result. Here
remain the kernels' outputs (``_hip_*``), the one way to call them or their injected models (:func:`_run`, with the parameter
table on the devices: :func:`_table_on`), the chunked write-then-select of ``predict`` and ``predict_response``
(:func:`_select_by_obs_blocks`) and the statistics."""
import ctypes
import weakref

import numpy as np
import torch

from . import diagnostics

PLANES = ("n", "m", "S", "mean", "M2", "sum_mu")
HIGH_VARIANCE = 0.4   # p_waic_i beyond which WAIC is unreliable for that observation (Vehtari, Gelman, Gabry 2017)
BAD_K = 0.7           # Pareto shape beyond which the PSIS-LOO estimate of that observation is unreliable (the same paper)
PSIS_COLUMNS = ("elpd", "pareto_k", "n_tail", "sigma", "ess_w", "cutoff", "min_loglik", "reserved")   # lmc_psis_rows: out[.][8]

_device_rows = weakref.WeakKeyDictionary()   # target -> {device: its parameter table in HBM}


def merge(a, b):
    """Two blocks ``[..., 6, N]`` of the six planes, over disjoint sets of draws -> the block over their union:
    m = max(ma, mb), S = Sa exp(ma - m) + Sb exp(mb - m), Chan's update of (mean, M2), sums for the count and sum mu.
    A side of count 0 is skipped BY ITS COUNT: the other side comes through bit for bit, whatever the empty side holds."""
    na, ma, Sa, mea, M2a, mua = a.unbind(-2)
    nb, mb, Sb, meb, M2b, mub = b.unbind(-2)
    hi, lo = torch.maximum(ma, mb), torch.minimum(ma, mb)
    e = torch.where(torch.isneginf(lo), torch.zeros_like(lo), torch.exp(lo - hi))   # (-inf) - (-inf) is never used
    S = torch.where(ma >= mb, Sa + Sb * e, Sa * e + Sb)
    both = torch.stack([na + nb, hi, S, *_chan(na, mea, M2a, nb, meb, M2b), mua + mub], dim=-2)
    only_a, only_b = (nb == 0).unsqueeze(-2), (na == 0).unsqueeze(-2)
    return torch.where(only_a, a, torch.where(only_b, b, both))


def _chan(na, mean_a, M2_a, nb, mean_b, M2_b):
    """Chan's update of a (mean, M2) pair over disjoint sets of na and nb draws (na + nb = 0: finite junk, never selected)."""
    n = na + nb
    safe = torch.where(n > 0, n, torch.ones_like(n))
    delta = mean_b - mean_a
    return mean_a + delta * (nb / safe), (M2_a + M2_b) + (delta * delta) * (na * nb / safe)


def _members(target):
    from .targets import GLM, Batched

    if isinstance(target, GLM):
        return [target]
    if isinstance(target, Batched) and isinstance(target.members[0], GLM):
        return list(target.members)
    raise TypeError("pointwise predictive statistics are those of a targets.GLM or a targets.Batched of GLM members "
                    "(the family that carries its data); got %r" % (target,))


def _own_table(target, members):
    """The target's own parameter rows, table[G, row_len] on the host."""
    return np.ascontiguousarray(target.params, dtype=np.float64).reshape(len(members), -1)


def _scored(target, members, data):
    """(table[G, row_len] (host), the GLMs whose y and constants apply) for the training data or for held-out ``data``."""
    from .targets import GLM, Batched

    if data is None:
        return _own_table(target, members), members
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

    c, _n, d = x.shape
    n_rows, row_len = table.shape
    npad = (row_len - _abi.GLM_HEADER) // (glm_row_layout(1, d)["size"] - _abi.GLM_HEADER) * 64
    out = torch.empty((diagnostics._touched(first_chain, c, per)[1], len(PLANES), npad), dtype=torch.float64, device=x.device)
    diagnostics._call_trace_kernel("lmc_glm_pointwise", x, table, row_len, n_rows, int(first_chain), int(per), out)
    return out


def _table_on(target, table, device, cache=None):
    """The host table of parameter rows on ``device``, copied there once per ``cache``: a dict device -> table of this call, or
    (None: the table is the target's own) the dict that lives and dies with the target."""
    held = _device_rows.setdefault(target, {}) if cache is None else cache
    key = str(device)
    if key not in held:
        held[key] = torch.as_tensor(table).to(device)
    return held[key]


def _run(fn, hip, b, target, table, cache, *args):
    """One kernel call on the block ``b`` of draws: the injected ``fn(b, table, *args)`` (tests of the host logic; ``table`` is
    then the host table of parameter rows), or else the HIP call ``hip`` on the block as the kernel reads it, with the table on
    the block's device (``cache``: as for :func:`_table_on`)."""
    if fn is not None:
        return fn(b, table, *args)
    b = diagnostics._device_block(b)
    return hip(b, _table_on(target, table, b.device, cache), *args)


def _block_range(rng, n, refusal=None):
    """(lo, hi) of the half-open, non-empty range ``rng`` of [0, n) (None: all of it), or ValueError: ``refusal``, by default
    that of an ``obs_blocks=`` of n blocks of 64 observations."""
    lo, hi = (0, n) if rng is None else (int(rng[0]), int(rng[1]))
    if not (0 <= lo < hi <= n):
        raise ValueError(refusal or "obs_blocks=%r of %d: a half-open, non-empty range" % (rng, n))
    return lo, hi


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
    members = _members(target)
    if group is not None:
        raise ValueError("pointwise predictive statistics are a one-process matter: group= / an active process group "
                         "(sample_distributed) is not supported")
    # one tensor may start inside the job, a list is the whole job; a group may straddle blocks
    job = diagnostics._trace_job(x, chains_per_group, first_chain, target, allow_first_chain=not isinstance(x, (list, tuple)))
    table, scored = _scored(target, members, data)
    n_obs = scored[0].n_obs
    cache = None if data is None else {}   # where the table of parameter rows lives on the devices

    def call(b, first):
        return _run(stats_fn, _hip_pointwise, b, target, table, cache, first, job.per)[..., :n_obs]

    tot = diagnostics._fan_out(job, job.g0, job.g0 + job.groups, call, merge)
    out = {name: tot[:, i] for i, name in enumerate(PLANES)}
    out["first_group"] = job.g0
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


# ---- PSIS-LOO (csrc/lmc_psis.hip: the rows; csrc/lmc_predict.hip: the array; include/lmc_hip.h states the row algorithm) -------
def tail_len(S, reff=1.0):
    """M of a row of S draws at relative efficiency ``reff``: ``min(S // 5, ceil(3 sqrt(S / reff)))`` (Vehtari et al.)."""
    import math

    S, reff = int(S), float(reff)
    if not (reff > 0.0) or math.isinf(reff):
        raise ValueError("reff is one positive number, the relative efficiency ESS / S of the draws (got %r)" % (reff,))
    return min(S // 5, int(math.ceil(3.0 * math.sqrt(S / reff))))


def _checked_tail_len(S, reff):
    from . import _abi

    M = tail_len(S, reff)
    if M > _abi.PSIS_MAX_TAIL:
        raise ValueError("PSIS of %d draws per posterior at reff=%g needs a tail of M = %d values; the kernel sorts at most %d "
                         "in LDS (LMC_PSIS_MAX_TAIL: about 1.86 million draws at reff=1). Pass fewer draws, e.g. x[:, ::k]"
                         % (S, reff, M, _abi.PSIS_MAX_TAIL))
    return M


def _hip_psis(l2, M):
    """One call of lmc_psis_rows: l2[rows, S] (float64, last axis contiguous, on a ROCm device) -> [rows, 8]."""
    from . import _abi

    lib = _abi.load()
    rows, S = l2.shape
    stride = l2.stride(0) if rows > 1 else S
    out = torch.empty((rows, len(PSIS_COLUMNS)), dtype=torch.float64, device=l2.device)
    with torch.cuda.device(l2.device):
        stream = torch.cuda.current_stream(l2.device).cuda_stream
        rc = lib.lmc_psis_rows(ctypes.c_void_p(l2.data_ptr()), rows, S, stride, int(M), ctypes.c_void_p(out.data_ptr()),
                               ctypes.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("lmc_psis_rows failed (status %d)" % rc)
    return out


def psis(loglik, reff=1.0, psis_fn=None):
    """Pareto-smoothed importance sampling of every row of ``loglik[..., S]`` (a float64 ROCm tensor with a contiguous last
    axis: S log-likelihood values of one observation under S posterior draws) by the HIP kernel ``lmc_psis_rows``
    (include/lmc_hip.h states the algorithm). It knows nothing of GLMs: any log-likelihood tensor on the device will do.
    Returns a dict of tensors shaped ``[...]``: ``elpd_i`` (the leave-one-out log predictive density of the observation,
    additive constants as in ``loglik``), ``pareto_k`` (the Pareto shape: above ``BAD_K`` = 0.7 the estimate is unreliable;
    ``inf`` when the tail has fewer than 5 values), ``n_tail``, ``ess_w`` (the effective sample size of the final weights),
    ``sigma`` (the Pareto scale) and ``min_loglik``.

    ``reff``: ONE positive number, the relative efficiency ``ESS / S`` of the draws; it sets the tail length
    ``M = min(S // 5, ceil(3 sqrt(S / reff)))``. The default 1.0 is that of independent draws: pass ``ess / S`` of an MCMC
    run. ``M`` above 4096 -- S above about 1.86 million -- is refused with a ValueError. ``psis_fn(l2[rows, S], M) ->
    [rows, 8]`` replaces the HIP call (tests of the host logic only)."""
    if loglik.dim() < 1 or int(loglik.shape[-1]) < 1:
        raise ValueError("loglik must be [..., S] with S >= 1")
    S = int(loglik.shape[-1])
    M = _checked_tail_len(S, reff)
    if psis_fn is None:
        if not loglik.is_cuda:
            from ._abi import HipLibraryError

            raise HipLibraryError("psis() runs on a log-likelihood tensor in HBM (a ROCm tensor); got a CPU tensor and there "
                                  "is no host implementation")
        if loglik.dtype != torch.float64:
            raise ValueError("loglik must be float64 (got %s)" % loglik.dtype)
    lead = tuple(loglik.shape[:-1])
    if loglik.dim() == 2 and (S == 1 or loglik.stride(1) == 1) and loglik.stride(0) >= S:
        l2 = loglik
    else:
        if S > 1 and loglik.stride(-1) != 1:
            raise ValueError("loglik must have a contiguous last axis (stride %d)" % loglik.stride(-1))
        l2 = loglik.reshape(-1, S)
        if not l2.is_contiguous():
            l2 = l2.contiguous()
    if l2.shape[0] == 0:
        raise ValueError("loglik holds no row")
    out = (psis_fn or _hip_psis)(l2, M)
    names = {"elpd_i": 0, "pareto_k": 1, "n_tail": 2, "sigma": 3, "ess_w": 4, "min_loglik": 6}
    return {k: out[:, i].reshape(lead) for k, i in names.items()}


def _hip_loglik(x, table, first_chain, per, ob0, ob1):
    """One call of lmc_glm_pointwise_loglik: x[chains, draws, d] holding whole groups -> [groups, 64 (ob1 - ob0), per * draws]."""
    c, n, _d = x.shape
    n_rows, row_len = table.shape
    out = torch.empty((c // per, 64 * (ob1 - ob0), per * n), dtype=torch.float64, device=x.device)
    diagnostics._call_trace_kernel("lmc_glm_pointwise_loglik", x, table, row_len, n_rows, int(first_chain), int(per), int(ob0),
                                   int(ob1), out)
    return out


def pointwise_loglik(x, target, groups=None, obs_blocks=None, loglik_fn=None):
    """The pointwise log-likelihood array itself, ``[G', 64 * blocks, S]`` on the device: ``out[g, i, s]`` is ``l`` of
    observation ``64 * ob0 + i`` of group ``g`` under draw ``s = (chain within the group) * draws + t`` -- the bits that
    :func:`pointwise_stats` reduces (additive constants dropped; observations beyond N are padding). It is N / d times the
    trace: meant for tests and small jobs, :func:`loo` walks it in chunks. ``groups=(g0, g1)`` and ``obs_blocks=(ob0, ob1)``
    select half-open ranges of groups and of blocks of 64 observations (default: all). ``x`` as for :func:`waic`; with a
    list of per-GPU blocks every group must lie in one block, and the result is gathered on the first block's device."""
    members = _members(target)
    job = diagnostics._trace_job(x, None, 0, target, whole_job=True, whole_groups=True)   # a posterior's draws form one row
    table, per = _own_table(target, members), job.per
    nob = (members[0].n_obs + 63) // 64
    refusal = "groups=%r of %d, obs_blocks=%r of %d: half-open, non-empty ranges" % (groups, len(members), obs_blocks, nob)
    g_lo, g_hi = _block_range(groups, len(members), refusal)
    ob0, ob1 = _block_range(obs_blocks, nob, refusal)
    parts = []
    for b, f in zip(job.held, job.firsts):   # (a gather of whole groups, not a fan-out: nothing is combined)
        lo, hi = max(g_lo, f // per), min(g_hi, (f + int(b.shape[0])) // per)
        if lo < hi:
            parts.append(_run(loglik_fn, _hip_loglik, b[lo * per - f:hi * per - f], target, table, None, lo * per, per, ob0, ob1))
    return parts[0] if len(parts) == 1 else torch.cat([p.to(parts[0].device) for p in parts], dim=0)


def loo(x, target, reff=1.0, scratch_bytes=1 << 30, psis_fn=None, loglik_fn=None, data=None, **kw):
    """PSIS-LOO of a ``GLM`` (leading axis 1) or of every posterior of a ``Batched`` of GLMs (leading axis G) from the draws in
    HBM, without a refit: everything :func:`waic` returns (the existing pass; ``**kw`` goes to it), plus per observation
    ``elpd_loo_i[G, N]`` (the leave-one-out log predictive density, ``GLM.loglik_constant()`` added), ``pareto_k[G, N]``
    (above ``BAD_K`` = 0.7 the estimate of that observation cannot be trusted -- the per-point answer to ``n_high_variance``),
    ``n_tail[G, N]``, ``ess_w[G, N]``, and per posterior ``elpd_loo[G]``, ``p_loo[G] = lppd_total - elpd_loo``,
    ``se_loo[G] = sqrt(N var_n(elpd_loo_i))``, ``looic[G] = -2 elpd_loo`` and ``n_bad_k[G]``. ``reff`` as for :func:`psis`.

    The pointwise log-likelihood (``lmc_glm_pointwise_loglik``) is written to a scratch array of at most ``scratch_bytes`` and
    smoothed row by row (``lmc_psis_rows``), in chunks of whole groups or, where one group exceeds the scratch, of blocks of
    64 observations of one group; one such block is ``64 * S * 8`` bytes and must fit. Rows are independent, so the chunking
    does not change a bit of the result. ``x`` is one tensor or the list of per-GPU blocks of the job (every group within one
    block): each block runs on its own device and the ``[G, N]`` results are gathered on the first block's device. LOO is
    in-sample: ``data=`` is refused (score held-out data with :func:`waic`). ``psis_fn`` / ``loglik_fn(x, table, first_chain,
    per, ob0, ob1)`` replace the two HIP calls (tests of the chunking and finalise logic)."""
    if data is not None:
        raise ValueError("loo() is in-sample: leave-one-out of the training data has no data= (waic(x, data=...) scores "
                         "held-out points)")
    members = _members(target)
    job = diagnostics._trace_job(x, None, 0, target, whole_job=True, whole_groups=True)   # a posterior's draws form one row
    table, per = _own_table(target, members), job.per
    S = per * job.n_draws
    M = _checked_tail_len(S, reff)
    n_obs = members[0].n_obs
    nob = (n_obs + 63) // 64
    unit = 64 * S * 8
    if unit > int(scratch_bytes):
        raise ValueError("scratch_bytes=%d is below one block of 64 observations of one posterior: 64 x %d draws x 8 = %d "
                         "bytes needed" % (int(scratch_bytes), S, unit))
    cap = int(scratch_bytes) // unit
    out = waic(x, target, **kw)
    dev = out["lppd"].device
    rows = torch.empty((len(members), nob * 64, len(PSIS_COLUMNS)), dtype=torch.float64, device=dev)
    for b, f in zip(job.held, job.firsts):   # each block on its own device; the small results move to the first one
        g_b, n_g = f // per, int(b.shape[0]) // per
        if cap >= nob:
            chunks = [(g, min(g + cap // nob, n_g), 0, nob) for g in range(0, n_g, cap // nob)]
        else:
            chunks = [(g, g + 1, ob, min(ob + cap, nob)) for g in range(n_g) for ob in range(0, nob, cap)]
        for lo, hi, ob0, ob1 in chunks:
            ll = _run(loglik_fn, _hip_loglik, b[lo * per:hi * per], target, table, None, f + lo * per, per, ob0, ob1)
            res = (psis_fn or _hip_psis)(ll.reshape(-1, S), M).reshape(hi - lo, (ob1 - ob0) * 64, len(PSIS_COLUMNS))
            rows[g_b + lo:g_b + hi, ob0 * 64:ob1 * 64] = res.to(dev)
            del ll
    rows = rows[:, :n_obs]
    const = torch.as_tensor(np.stack([m.loglik_constant() for m in members]), dtype=torch.float64).to(dev)
    e = rows[..., 0] + const
    out["elpd_loo_i"], out["pareto_k"], out["n_tail"], out["ess_w"] = e, rows[..., 1], rows[..., 2], rows[..., 4]
    out["elpd_loo"] = e.sum(dim=-1)
    out["p_loo"] = out["lppd_total"] - out["elpd_loo"]
    out["se_loo"] = torch.sqrt(n_obs * e.var(dim=-1)) if n_obs > 1 else torch.full_like(out["elpd_loo"], float("nan"))
    out["looic"] = -2.0 * out["elpd_loo"]
    out["n_bad_k"] = (out["pareto_k"] > BAD_K).sum(dim=-1)
    return out


# ---- posterior predictions at new X (csrc/lmc_linpred.hip; include/lmc_hip.h: lmc_glm_linpred) ------------------------------
MOMENT_PLANES = ("n", "eta_mean", "eta_M2", "mu_mean", "mu_M2")


def merge_moments(a, b):
    """Two blocks ``[..., 5, W]`` of the planes ``n, mean eta, M2 eta, mean mu, M2 mu`` over disjoint sets of draws -> the
    block over their union: Chan's update of both (mean, M2) pairs, the rule of :func:`merge`. A side of count 0 is skipped
    BY ITS COUNT: the other side comes through bit for bit, whatever the empty side holds."""
    na, mea, M2a, mma, N2a = a.unbind(-2)
    nb, meb, M2b, mmb, N2b = b.unbind(-2)
    both = torch.stack([na + nb, *_chan(na, mea, M2a, nb, meb, M2b), *_chan(na, mma, N2a, nb, mmb, N2b)], dim=-2)
    only_a, only_b = (nb == 0).unsqueeze(-2), (na == 0).unsqueeze(-2)
    return torch.where(only_a, a, torch.where(only_b, b, both))


def _predicted(target, members, X_new):
    """(table[G, row_len] (host), N_new) of the points to predict at: the training design, or ``X_new`` validated as
    :func:`_scored` validates ``data=`` -- through ``GLM(X_new, zeros, ...)`` of the member's likelihood and scales (the y
    section of such a row is never read)."""
    from .targets import GLM, Batched

    if X_new is None:
        return _own_table(target, members), members[0].n_obs
    if isinstance(target, Batched):
        designs = list(X_new)
        if len(designs) != len(members):
            raise ValueError("X_new for a Batched of %d groups is a list of %d arrays [N_new, d] (got %d)"
                             % (len(members), len(members), len(designs)))
    else:
        designs = [X_new]
    held = []
    for g, (m, X) in enumerate(zip(members, designs)):
        X = np.asarray(X, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("X_new of group %d must be [N_new, d] (got shape %r)" % (g, tuple(X.shape)))
        if X.shape[1] != m.d:
            raise ValueError("X_new of group %d has d = %d, the posterior d = %d" % (g, X.shape[1], m.d))
        if held and X.shape[0] != held[0].n_obs:
            raise ValueError("X_new of group %d has N_new = %d, group 0 N_new = %d: one common N_new" % (g, X.shape[0], held[0].n_obs))
        held.append(GLM(X, np.zeros(X.shape[0]), likelihood=m.likelihood, prior_scale=m.prior_scale, sigma=m.sigma))
    return np.stack([h.params for h in held]), held[0].n_obs


def _hip_linpred(x, table, first_chain, per, ob0, ob1, want_eta=True, want_stats=True):
    """One call of lmc_glm_linpred: x[chains, draws, d] (float64, _row_major, on a ROCm device), table[n_rows, row_len] on the
    same device -> (eta[chains, draws, W] or None, stats[groups touched, 5, W] or None), W = 64 (ob1 - ob0)."""
    c, n, _d = x.shape
    n_rows, row_len = table.shape
    W = 64 * (int(ob1) - int(ob0))
    eta = torch.empty((c, n, W), dtype=torch.float64, device=x.device) if want_eta else None
    stats = (torch.empty((diagnostics._touched(first_chain, c, per)[1], len(MOMENT_PLANES), W), dtype=torch.float64, device=x.device)
             if want_stats else None)
    diagnostics._call_trace_kernel("lmc_glm_linpred", x, table, row_len, n_rows, int(first_chain), int(per), int(ob0), int(ob1),
                                   eta, stats)
    return eta, stats


def linear_predictor(x, target, X_new=None, obs_blocks=None, linpred_fn=None):
    """The linear predictor itself and its moments, from ONE tensor of draws ``x[chains, draws, d]`` (the whole job of
    ``target``) -> ``(eta[chains, draws, W], stats)``: ``eta[c, t, i]`` is ``X_new[64 * ob0 + i] @ x[c, t]`` on the row of
    chain c's group -- the sampler's own contraction, bit for bit; observations beyond N_new are padding (0) -- and ``stats``
    is a dict of ``[G, W]`` tensors ``n, eta_mean, eta_M2, mu_mean, mu_M2`` (``MOMENT_PLANES``). It is N_new / d times the
    trace: meant for tests and small jobs, :func:`predict` walks it in chunks. ``X_new=None`` means the training design;
    ``obs_blocks=(ob0, ob1)`` selects a half-open range of blocks of 64 observations (default: all). ``linpred_fn(x, table,
    first_chain, per, ob0, ob1, want_eta, want_stats) -> (eta, stats[groups touched, 5, W])`` replaces the HIP call."""
    if isinstance(x, (list, tuple)):
        raise ValueError("linear_predictor takes one tensor; predict() takes the list of per-GPU blocks of a job")
    members = _members(target)
    job = diagnostics._trace_job(x, None, 0, target, whole_job=True)
    table, n_new = _predicted(target, members, X_new)
    ob0, ob1 = _block_range(obs_blocks, (n_new + 63) // 64)
    eta, st = _run(linpred_fn, _hip_linpred, job.held[0], target, table, None if X_new is None else {}, 0, job.per, ob0, ob1,
                   True, True)
    return eta, {name: st[:, i] for i, name in enumerate(MOMENT_PLANES)}


def _select_by_obs_blocks(job, n_new, ranks, scratch_bytes, what, write, count_fn):
    """Write an array ``[chains, draws, 64 k]`` of ``what`` by blocks of 64 of the ``n_new`` observations, then select from it:
    yields ``diagnostics.order_statistics`` at ``ranks`` of every chunk, ``[G, len(ranks), 64 k]``, the chunks in order.
    ``write(ob0, ob1)`` returns the written arrays of the job's blocks, each on its device. A chunk holds as many observation
    blocks as fit into ``scratch_bytes`` with the select's counts of them -- ``chains x draws x 64 x 8`` bytes an observation
    block over all devices, and 256 buckets x 64 columns x 8 bytes a rank and group -- and the select gets the rest through its
    own ``scratch_bytes=``; ValueError if one observation block does not fit. Columns are independent, so the chunking does not
    change a bit."""
    from . import _abi

    unit = job.chains * job.n_draws * 64 * 8
    count_unit = 256 * 64 * 8 * min(len(set(ranks)), _abi.SELECT_MAX_RANKS)
    nob = (n_new + 63) // 64
    step = min(int(scratch_bytes) // (unit + count_unit), nob)
    if step < 1:
        raise ValueError("scratch_bytes=%d is below one block of 64 observations of %s, %d chains x %d draws x 64 x 8 = %d bytes, "
                         "plus %d bytes of the select's counts of it" % (int(scratch_bytes), what, job.chains, job.n_draws, unit,
                                                                        count_unit))
    for ob0 in range(0, nob, step):
        ob1 = min(ob0 + step, nob)
        written = write(ob0, ob1)
        os_ = diagnostics.order_statistics(written if len(written) > 1 else written[0], ranks, chains_per_group=job.per,
                                           scratch_bytes=int(scratch_bytes) - (ob1 - ob0) * unit, count_fn=count_fn)
        del written
        yield os_


def _inverse_link(likelihood, eta):
    return {"bernoulli": torch.sigmoid, "poisson": torch.exp, "gaussian": lambda v: v}[likelihood](eta)


def predict(x, target, X_new=None, probs=(0.05, 0.5, 0.95), chains_per_group=None, scratch_bytes=1 << 30, linpred_fn=None,
            count_fn=None):
    """Posterior predictions of a ``GLM`` (leading axis 1) or of every posterior of a ``Batched`` of GLMs (leading axis G) at
    the points ``X_new`` -- ``[N_new, d]``, for a ``Batched`` a list of G such arrays with one common N_new; ``None``: the
    training design -- from the draws in HBM. A dict of float64 tensors on x's device:

    ``eta_mean, eta_sd, mu_mean, mu_sd`` ``[G, N_new]``: the posterior mean and standard deviation ``sqrt(M2 / (n - 1))`` (NaN
    for one draw) of the linear predictor ``eta = x'q`` and of the mean response ``mu = sigmoid(eta) | exp(eta) | eta``
    (bernoulli | poisson | gaussian), from the kernel's merged moments;
    ``eta_quantiles`` ``[G, Q, N_new]``: the quantiles at ``probs`` of eta, as ``diagnostics.quantiles`` gives them for a trace:
    EXACT order statistics of the written eta (the radix select) and numpy's linear interpolation;
    ``mu_quantiles`` ``[G, Q, N_new]``: the credible band of the mean response. The inverse link is monotone, so THE SORTED mu
    ARE DEFINED AS the inverse link (``torch.sigmoid``, ``torch.exp``, the identity; on the host) of the sorted eta: the link
    is applied to the two neighbouring eta order statistics of each probability and the interpolation is done on the mu
    scale -- no second select;
    ``y_mean, y_var`` ``[G, N_new]``: the posterior-predictive mean and variance of a NEW response by the law of total
    variance, without simulation -- bernoulli: ``mu_mean``, ``mu_mean (1 - mu_mean)``; poisson: ``mu_mean``,
    ``mu_mean + var mu``; gaussian: ``eta_mean``, ``sigma^2 + var eta`` (var = M2 / (n - 1));
    ``n``: S = chains of a group x draws, the draws per posterior; ``probs``.

    ``x`` is one tensor ``[chains, draws, d]`` or the list of per-GPU blocks of the job: each block runs on its own device at
    its running first chain (a group may straddle blocks), the moments merge on the first block's device
    (:func:`merge_moments`) and the select adds its integer counts across blocks. The linear predictor is written
    (``lmc_glm_linpred``) in chunks of blocks of 64 observations: the chunks of a pass (``chains x draws x 64 x 8`` bytes an
    observation block, over all devices) plus the select's counts stay within ``scratch_bytes`` -- the select gets the rest
    through its own ``scratch_bytes=`` -- and ValueError if one observation block does not fit. Columns are independent, so the
    chunking does not change a bit. ``linpred_fn`` (see :func:`linear_predictor`) and ``count_fn`` (see
    ``diagnostics.order_statistics``) replace the two HIP calls (tests of this logic); without ``linpred_fn`` a CPU tensor
    raises HipLibraryError. Not with an active process group."""
    members = _members(target)
    job = diagnostics._trace_job(x, chains_per_group, 0, target, whole_job=True)   # a group may straddle blocks
    per, dev, S = job.per, job.device, job.per * job.n_draws
    probs, ranks, frac = diagnostics._quantile_plan(S, probs)
    table, n_new = _predicted(target, members, X_new)
    G = len(members)
    liks = [m.likelihood for m in members]
    cache = None if X_new is None else {}   # where the table of parameter rows lives on the devices
    moments, eta_q, mu_q = [], [], []

    def write(ob0, ob1):   # the eta of a block stays on its device for the select; its moments are the part to merge
        etas = []

        def call(b, first):
            eta, st = _run(linpred_fn, _hip_linpred, b, target, table, cache, first, per, ob0, ob1, True, True)
            etas.append(eta)
            return st

        moments.append(diagnostics._fan_out(job, 0, G, call, merge_moments))
        return etas

    def mu_of(v):   # the member's inverse link, group by group
        return torch.stack([_inverse_link(liks[g], v[g]) for g in range(G)])

    for os_ in _select_by_obs_blocks(job, n_new, ranks, scratch_bytes, "the linear predictor", write, count_fn):
        _vmin, _vmax, q, q_mu = diagnostics._interpolate(os_, frac, link=mu_of)
        eta_q.append(q)
        mu_q.append(q_mu)
    tot = torch.cat(moments, dim=-1)[..., :n_new]
    n = tot[:, 0]
    eta_mean, mu_mean = tot[:, 1], tot[:, 3]
    eta_var, mu_var = tot[:, 2] / (n - 1.0), tot[:, 4] / (n - 1.0)
    sig2 = torch.tensor([float(m.sigma) ** 2 for m in members], dtype=torch.float64, device=dev).reshape(G, 1)
    is_b = torch.tensor([k == "bernoulli" for k in liks], device=dev).reshape(G, 1)
    is_p = torch.tensor([k == "poisson" for k in liks], device=dev).reshape(G, 1)
    y_mean = torch.where(is_b | is_p, mu_mean, eta_mean)
    y_var = torch.where(is_b, mu_mean * (1.0 - mu_mean), torch.where(is_p, mu_mean + mu_var, sig2 + eta_var))
    return dict(eta_mean=eta_mean, eta_sd=torch.sqrt(eta_var), mu_mean=mu_mean, mu_sd=torch.sqrt(mu_var),
                eta_quantiles=torch.cat(eta_q, dim=-1)[..., :n_new], mu_quantiles=torch.cat(mu_q, dim=-1)[..., :n_new],
                y_mean=y_mean, y_var=y_var, n=S, probs=probs)


def _link(likelihood, t):
    """The link of a threshold ``t`` on the mean response: logit | log | identity, monotone, so mu < t exactly where eta <
    link(t) up to the rounding of the inverse link. A threshold at or beyond the end of mu's range maps to -inf / +inf (no
    mu lies below 0; every bernoulli mu lies below 1 and beyond); NaN stays NaN."""
    if likelihood == "gaussian":
        return t
    low = torch.full_like(t, float("-inf"))
    if likelihood == "poisson":
        return torch.where(t <= 0, low, torch.log(t.clamp(min=0.0)))
    inner = t.clamp(min=0.0, max=1.0)
    return torch.where(t <= 0, low, torch.where(t >= 1, -low, torch.log(inner) - torch.log1p(-inner)))


def exceedance(x, target, X_new=None, thresholds=0.0, scale="eta", chains_per_group=None, scratch_bytes=1 << 30,
               linpred_fn=None, count_fn=None):
    """P(prediction < t) at new points, counted over the draws in HBM -> dict(p_less, p_equal, p_greater [G, K, N_new] float64,
    n = S, n_nan [G, N_new]) for a ``GLM`` (G = 1) or every posterior of a ``Batched`` of GLMs; ``1 - p_less - p_equal`` is
    ``p_greater``, e.g. P(p_new > 0.5) of a bernoulli fit is ``exceedance(x, tgt, X_new, thresholds=0.5, scale="mu")["p_greater"]``.
    ``thresholds`` is what ``diagnostics.threshold_counts`` takes with N_new in place of d: a scalar, 1-D of length K, [K, N_new]
    or [G, K, N_new]. ``scale="eta"`` compares the linear predictor; ``scale="mu"`` the mean response, whose thresholds are
    mapped through the member's monotone link on the host (logit | log | identity) and compared on the eta scale -- the
    definition ``predict`` uses for its mu quantiles. A (posterior, point) with a NaN prediction is NaN.

    The linear predictor is written (``lmc_glm_linpred``, the kernel of ``predict``) in chunks of blocks of 64 observations that
    stay within ``scratch_bytes`` -- ``chains x draws x 64 x 8`` bytes an observation block over all devices; ValueError if one
    does not fit -- and each chunk, which is trace-shaped, is counted with ``threshold_counts``. Columns are independent, so the
    chunking does not change a count. ``x`` is one tensor or the list of per-GPU blocks of the job. ``linpred_fn`` (see
    :func:`linear_predictor`) and ``count_fn`` (see ``diagnostics.threshold_counts``) replace the two HIP calls."""
    if scale not in ("eta", "mu"):
        raise ValueError("scale must be 'eta' or 'mu' (got %r)" % (scale,))
    members = _members(target)
    job = diagnostics._trace_job(x, chains_per_group, 0, target, whole_job=True)
    per, dev, G = job.per, job.device, len(members)
    table, n_new = _predicted(target, members, X_new)
    thr = diagnostics._threshold_block(thresholds, G, n_new, True)
    if scale == "mu":
        thr = torch.stack([_link(m.likelihood, thr[g]) for g, m in enumerate(members)])
    K, nob = int(thr.shape[1]), (n_new + 63) // 64
    padded = torch.full((G, K, 64 * nob), float("nan"), dtype=torch.float64)   # a padding column counts nothing
    padded[..., :n_new] = thr
    unit = job.chains * job.n_draws * 64 * 8
    step = min(int(scratch_bytes) // unit, nob)
    if step < 1:
        raise ValueError("scratch_bytes=%d is below one block of 64 observations of the linear predictor, %d chains x %d draws x "
                         "64 x 8 = %d bytes" % (int(scratch_bytes), job.chains, job.n_draws, unit))
    cache = None if X_new is None else {}
    less, equal, nan = [], [], []
    for ob0 in range(0, nob, step):
        ob1 = min(ob0 + step, nob)
        etas = [_run(linpred_fn, _hip_linpred, b, target, table, cache, f, per, ob0, ob1, True, False)[0]
                for b, f in zip(job.held, job.firsts)]
        tc = diagnostics.threshold_counts(etas if len(etas) > 1 else etas[0], padded[..., 64 * ob0:64 * ob1],
                                          chains_per_group=per, count_fn=count_fn)
        del etas
        less.append(tc["less"].to(dev))
        equal.append(tc["equal"].to(dev))
        nan.append(tc["nan"].to(dev))
    less, equal = (torch.cat(v, dim=-1)[..., :n_new].to(torch.float64) for v in (less, equal))
    n_nan = torch.cat(nan, dim=-1)[..., :n_new]
    bad = (n_nan > 0).unsqueeze(-2)
    S = diagnostics._divisor(job.per * job.n_draws, less)   # (a tensor divisor: a division)
    nanned = lambda t: torch.where(bad, torch.full_like(t, float("nan")), t)   # noqa: E731
    return {"p_less": nanned(less / S), "p_equal": nanned(equal / S), "p_greater": nanned((S - less - equal) / S),
            "n": job.per * job.n_draws, "n_nan": n_nan}


# ---- replicated responses (csrc/lmc_yrep.hpp, csrc/lmc_yrep.hip; include/lmc_hip.h: lmc_glm_yrep, lmc_glm_yrep_stats) --------
PPC_NAMES = ("mean", "sd", "min", "max", "zeros", "chisq")


def _seed32(random_seed):
    return int(random_seed) & 0xFFFFFFFF


def _hip_yrep(x, table, first_chain, per, ob0, ob1, seed):
    """One call of lmc_glm_yrep: x[chains, draws, d] (a ROCm tensor), table[n_rows, row_len] on the same device ->
    y[chains, draws, W], W = 64 (ob1 - ob0)."""
    c, n, _d = x.shape
    n_rows, row_len = table.shape
    y = torch.empty((c, n, 64 * (int(ob1) - int(ob0))), dtype=torch.float64, device=x.device)
    diagnostics._call_trace_kernel("lmc_glm_yrep", x, table, row_len, n_rows, int(first_chain), int(per), int(ob0), int(ob1),
                                   int(seed), y)
    return y


def replicate(x, target, X_new=None, obs_blocks=None, random_seed=0, yrep_fn=None):
    """Replicated responses ``y_rep ~ p(y | q_s)`` of every draw, from ONE tensor of draws ``x[chains, draws, d]`` (the whole
    job of ``target``) -> ``y[chains, draws, W]`` on the device: ``y[c, t, i]`` is a bernoulli / poisson / gaussian response at
    ``X_new[64 * ob0 + i]`` under draw t of chain c -- a pure function of ``(random_seed, c, t, observation)``
    (include/lmc_hip.h states the stream), whatever the chunking or the device; counts are doubles, observations beyond N_new
    are padding (0), and a draw whose mean response is NaN, infinite or (poisson) above 2^52 gives NaN. It is N_new / d times
    the trace: meant for tests and small jobs, :func:`predict_response` walks it in chunks and :func:`ppc` never writes it.
    ``X_new``, ``obs_blocks`` as for :func:`linear_predictor`; ``yrep_fn(x, table, first_chain, per, ob0, ob1, seed) -> y``
    replaces the HIP call."""
    if isinstance(x, (list, tuple)):
        raise ValueError("replicate takes one tensor; predict_response() and ppc() take the list of per-GPU blocks of a job")
    members = _members(target)
    job = diagnostics._trace_job(x, None, 0, target, whole_job=True)
    table, n_new = _predicted(target, members, X_new)
    ob0, ob1 = _block_range(obs_blocks, (n_new + 63) // 64)
    return _run(yrep_fn, _hip_yrep, job.held[0], target, table, None if X_new is None else {}, 0, job.per, ob0, ob1,
                _seed32(random_seed))


def predict_response(x, target, X_new=None, probs=(0.05, 0.5, 0.95), chains_per_group=None, scratch_bytes=1 << 30,
                     random_seed=0, yrep_fn=None, count_fn=None):
    """The prediction band of a NEW response of a ``GLM`` (leading axis 1) or of every posterior of a ``Batched`` of GLMs
    (leading axis G) at the points ``X_new`` (as for :func:`predict`; ``None``: the training design), from the draws in HBM:
    a dict with ``y_quantiles[G, P, N_new]``, the quantiles at ``probs`` of the S = chains of a group x draws replicated
    responses of each point (one per draw: :func:`replicate`), ``y_min`` and ``y_max`` ``[G, N_new]``, ``n`` = S and ``probs``.

    The order statistics are EXACT (the radix select on the written ``y_rep``) and the quantiles are interpolated between
    them as numpy's default does -- also for counts: the 0.05 quantile of a poisson response may be 2.35. Take ``floor`` /
    ``ceil`` of the two ends for an integer interval that covers at least the nominal mass. A point with a NaN replicate has
    NaN quantiles, as numpy's are. The result is a pure function of ``random_seed`` and the draws: ``scratch_bytes`` (the
    chunking over blocks of 64 observations, as in :func:`predict`), the list of per-GPU blocks and the devices do not change
    a bit. ``yrep_fn`` (see :func:`replicate`) and ``count_fn`` (``diagnostics.order_statistics``) replace the two HIP calls."""
    members = _members(target)
    job = diagnostics._trace_job(x, chains_per_group, 0, target, whole_job=True)   # a group may straddle blocks
    per, S = job.per, job.per * job.n_draws
    probs, ranks, frac = diagnostics._quantile_plan(S, probs)
    table, n_new = _predicted(target, members, X_new)
    cache = None if X_new is None else {}
    seed = _seed32(random_seed)
    y_q, y_min, y_max = [], [], []

    def write(ob0, ob1):
        return [_run(yrep_fn, _hip_yrep, b, target, table, cache, f, per, ob0, ob1, seed) for b, f in zip(job.held, job.firsts)]

    for os_ in _select_by_obs_blocks(job, n_new, ranks, scratch_bytes, "the replicated responses", write, count_fn):
        vmin, vmax, q = diagnostics._interpolate(os_, frac)
        y_min.append(vmin)
        y_max.append(vmax)
        y_q.append(q)
    return dict(y_quantiles=torch.cat(y_q, dim=-1)[..., :n_new], y_min=torch.cat(y_min, dim=-1)[..., :n_new],
                y_max=torch.cat(y_max, dim=-1)[..., :n_new], n=S, probs=probs)


def _hip_yrep_stats(x, table, first_chain, per, seed, centre):
    """One call of lmc_glm_yrep_stats: x[chains, draws, d] (a ROCm tensor), table[n_rows, row_len] on the same device and
    centre[n_rows] (a host array; it goes there) -> T[chains, draws, 7]."""
    from . import _abi

    c, n, _d = x.shape
    n_rows, row_len = table.shape
    centre = torch.from_numpy(centre).to(x.device)
    T = torch.empty((c, n, _abi.YREP_STATS), dtype=torch.float64, device=x.device)
    diagnostics._call_trace_kernel("lmc_glm_yrep_stats", x, table, row_len, n_rows, int(first_chain), int(per), int(seed), centre, T)
    return T


def ppc_scales(T, n_obs, centre):
    """The five statistics of a data set on their own scales from the planes ``T[..., 0:5]`` (sum, sum of squares about
    ``centre``, min, max, zeros) of its N = ``n_obs`` values: ``[..., 5]`` = mean ``P0 / N``, sd ``sqrt(var)`` with
    ``var = (P1 - (P0 - N c)^2 / N) / (N - 1)`` (clamped at 0; NaN for N = 1), min, max, zeros. ``centre`` broadcasts
    against ``T[..., 0]``. The observed data go through the same expression, so ties compare equal."""
    N = float(n_obs)
    P0, P1 = T[..., 0], T[..., 1]
    dev = P0 - N * centre
    var = (P1 - dev * dev / N) / (N - 1.0) if n_obs > 1 else torch.full_like(P0, float("nan"))
    sd = torch.sqrt(torch.where(var < 0.0, torch.zeros_like(var), var))
    return torch.stack([P0 / N, sd, T[..., 2], T[..., 3], T[..., 4]], dim=-1)


def _sum_by_group(v, first, per):
    """v[c, k] of a block whose chain 0 is job chain ``first`` -> [groups touched, k]: the rows of every group's chains added."""
    c = int(v.shape[0])
    g0, touched = diagnostics._touched(first, c, per)
    if first % per == 0 and c % per == 0:
        return v.reshape(touched, per, -1).sum(dim=1)
    cuts = [min(max((g0 + i) * per - first, 0), c) for i in range(touched + 1)]
    return torch.stack([v[a:b].sum(dim=0) for a, b in zip(cuts[:-1], cuts[1:])])


def ppc(x, target, random_seed=0, probs=(0.05, 0.5, 0.95), chains_per_group=None, stats_fn=None, count_fn=None, **kw):
    """Posterior predictive checks of a ``GLM`` (leading axis 1) or of every posterior of a ``Batched`` of GLMs (leading axis
    G) from the draws in HBM: does the fitted model reproduce the data? Every draw s gives one replicated data set
    ``y_rep ~ p(y | q_s)`` at the training design (the values of :func:`replicate` on the same ``random_seed``, never
    written), reduced on the device to test statistics (``lmc_glm_yrep_stats``); a dict of float64 tensors on x's device:

    ``T_obs[G, 5]``: mean, sd, min, max and number of zeros of the observed ``y`` (``names[:5]``);
    ``T_rep_mean[G, 5]``, ``T_rep_quantiles[G, P, 5]``: the mean over the S draws, and the quantiles at ``probs``
    (``diagnostics.quantiles``: exact order statistics, numpy's interpolation), of the same five statistics of the
    replicated data sets, each on its own scale (:func:`ppc_scales`);
    ``p_value[G, 6]``: the posterior predictive p-value (Gelman, Meng, Stern 1996) -- the share of draws with
    ``T(y_rep) >= T(y)`` for the five statistics, and with ``X^2(y_rep, q_s) >= X^2(y, q_s)`` for ``chisq``, Pearson's
    ``sum_i (y_i - mu_i)^2 / V_i``, whose realised value depends on the draw. A value near 0 or 1 says the data are extreme
    under the model: ``chisq`` near 0 is overdispersion, ``zeros`` near 0 excess zeros. A draw with a NaN statistic counts as
    "not >=";
    ``names`` = ``PPC_NAMES``, ``n`` = S, ``probs``.

    ``x`` is one tensor ``[chains, draws, d]`` or the list of per-GPU blocks of the job; the counts of the p-values are integers
    added over blocks and the select is exact, so a posterior may straddle devices (``T_rep_mean`` is then a sum of parts).
    The kernel's planes ``T[chains, draws, 7]`` of a block live on its device until its counts are taken; only the five scaled
    statistics (``5 / N`` of what ``y_rep`` would be) are kept for the select.
    ``**kw`` goes to the select (``scratch_bytes``). ``stats_fn(x, table, first_chain, per, seed, centre) -> T[chains, draws,
    7]`` and ``count_fn`` replace the two HIP calls (tests of this logic)."""
    members = _members(target)
    job = diagnostics._trace_job(x, chains_per_group, 0, target, whole_job=True)   # a group may straddle blocks
    per, dev, S = job.per, job.device, job.per * job.n_draws
    probs = diagnostics._probs(probs)
    G, n_obs = len(members), members[0].n_obs
    table = _own_table(target, members)
    seed = _seed32(random_seed)
    centre = np.array([float(m.y.sum()) / n_obs for m in members], dtype=np.float64)
    planes_obs = np.array([[m.y.sum(), ((m.y - c) ** 2).sum(), m.y.min(), m.y.max(), float((m.y == 0.0).sum())]
                           for m, c in zip(members, centre)], dtype=np.float64)
    T_obs = ppc_scales(torch.from_numpy(planes_obs), n_obs, torch.from_numpy(centre)).to(dev)
    scaled = []

    def call(b, first):   # the five scales stay on the block's device; what is merged are sums and counts per group
        T = _run(stats_fn, _hip_yrep_stats, b, target, table, None, first, per, seed, centre)
        g = (first + torch.arange(int(b.shape[0]), device=T.device)) // per
        tr = ppc_scales(T, n_obs, torch.from_numpy(centre).to(T.device)[g].unsqueeze(1))
        scaled.append(tr)
        ge = torch.cat([tr >= T_obs.to(T.device)[g].unsqueeze(1), (T[..., 5] >= T[..., 6]).unsqueeze(-1)], dim=-1)
        per_chain = torch.cat([tr.sum(dim=1), ge.sum(dim=1).to(torch.float64)], dim=-1)   # [c, 5 + 6]; counts are exact
        return _sum_by_group(per_chain, first, per)

    tot = diagnostics._fan_out(job, 0, G, call, torch.add)
    q = diagnostics.quantiles(scaled if len(scaled) > 1 else scaled[0], probs, chains_per_group=per, count_fn=count_fn, **kw)
    return dict(T_obs=T_obs, T_rep_mean=tot[:, :5] / float(S), T_rep_quantiles=q["quantiles"], p_value=tot[:, 5:] / float(S),
                names=PPC_NAMES, n=S, probs=probs)
