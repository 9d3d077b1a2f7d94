"""Cross-chain convergence diagnostics: split R-hat and multi-chain effective sample size.

The reference has none (ArviZ appears only in a docs recipe, docs/tutorials/framework_cookbook.rst:201-213;
SURVEY.md section 0.9): the definitions below are this build's own -- split R-hat and the Geyer
initial-monotone-sequence ESS of the Stan reference manual, optionally on rank-normalised draws (Vehtari et al.
2021: z = Phi^-1((rank - 3/8) / (S + 1/4)) over the pooled draws of a dimension) -- and are pinned against a
plain-numpy restatement (oracle/diagnostics_oracle.py).

Everything reduces to per-dimension *sufficient statistics that add over chains* (and chain halves, and ranks):

    n_chains, sum_c mean_c, sum_c mean_c^2, sum_c var_c, sum_c acov_c[t]

For draws in HBM (``Engine.trace_device_ptr()`` through ``trace_tensor``) they come from the HIP kernel
``lmc_diag_chain_stats`` (csrc/lmc_diag.hip), 16 lags per pass over the trace; passes continue until Geyer's initial
positive sequence has ended in every dimension (one pass for well-mixing NUTS chains), each pass followed by ONE
small all-reduce (RCCL on GPUs) of its (3 + 16) x d block. ``chains_per_group=per`` (a ``targets.Batched`` job: many
posteriors, ``per`` consecutive chains each) gives every statistic and every result a leading group axis from the same
passes -- ``lmc_diag_chain_stats_grouped``, one launch for all groups and still one host look per pass. There is one
backend: the HIP kernel. The reduction /
finalisation logic above it is backend-agnostic tensor code, and the CPU tests of that logic (gloo, world_size 2) inject
the test oracle's restatement of the kernel's block (oracle/diagnostics_oracle.py: torch_chain_stats) through the
``stats_fn`` argument; nothing in this package computes the statistics on the host.

Posterior quantiles, equal-tailed credible intervals and tail-ESS (``order_statistics``, ``quantiles``, ``intervals``,
``tail_ess``, at the end of this module) follow the same rule with an integer statistic: a radix select whose passes are
histograms of key digits from ``lmc_select_digit_counts`` (csrc/lmc_select.hip), exact and additive over chains and GPUs.

Posterior covariance and correlation per posterior (``cross_moments``, ``covariance``, ``contrasts``, after them) are one
contraction over the (chain, draw) rows of every group on the FP64 matrix cores, ``lmc_diag_cross_moments``
(csrc/lmc_cross.hip); blocks merge by Chan's rule for matrices (``merge_cross_moments``).

Posterior probabilities (``threshold_counts``, ``prob``, ``direction``, ``rope``, after ``tail_ess``) are the inverse question
of the select, which rank a value has: per (posterior, coefficient, threshold) the draws below and equal to the threshold
from ``lmc_diag_threshold_counts`` (csrc/lmc_threshold.hip), one read of the trace for up to 16 thresholds, integers that add
over chains and GPUs. ``sbc`` takes the ranks of simulation-based calibration from it."""
import collections
import ctypes
import math

import torch

LAGS_PER_PASS = 16


def split_chains(x):
    """[chains, draws, d] -> [2*chains, draws//2, d] (second half of every chain becomes its own chain)."""
    c, n, d = x.shape
    h = n // 2
    return torch.cat([x[:, :h], x[:, n - h:]], dim=0)


def _hip_chain_stats(x, t0, n, lag0, first_chain=None, per=None):
    """One pass of lmc_diag_chain_stats over x[chains, draws, d] (float64, contiguous, on a ROCm device):
    -> [3 + 16, d] float64 tensor on the same device. With ``per`` chains per group, x's chain 0 being chain ``first_chain`` of
    the job, one pass of lmc_diag_chain_stats_grouped: -> [groups touched, 3 + 16, d]."""
    name, grouping, lead = "lmc_diag_chain_stats", (), ()
    if per is not None:
        name, grouping = "lmc_diag_chain_stats_grouped", (int(first_chain), int(per))
        lead = (_touched(first_chain, int(x.shape[0]), per)[1],)
    out = torch.empty(lead + (3 + LAGS_PER_PASS, int(x.shape[2])), dtype=torch.float64, device=x.device)
    _call_trace_kernel(name, x, int(lag0), *grouping, out, t0=t0, n=n)
    return out


def _call_trace_kernel(name, x, *args, t0=0, n=None):
    """The one call of an entry point that makes a pass over the trace (include/lmc_hip.h): ``name(x, chains, draws_stride, d,
    t0, n, *args, stream)`` on x's device and current stream, over the sub-series [t0, t0 + n) of every chain (default: all
    draws). x[chains, draws, d] goes as the kernel reads it (_device_block: HipLibraryError for a CPU tensor); a tensor among
    ``args`` goes as its device pointer, None as NULL. RuntimeError unless the call returns LMC_OK."""
    from . import _abi

    x = _device_block(x)
    c, rows, d = x.shape
    stride = x.stride(0) // d if c > 1 else rows     # rows of a chain lie d apart; chains `stride` rows apart (_row_major)
    with torch.cuda.device(x.device):
        stream = torch.cuda.current_stream(x.device).cuda_stream
        rc = getattr(_abi.load(), name)(ctypes.c_void_p(x.data_ptr()), c, stride, d, int(t0), int(rows if n is None else n),
                                        *[ctypes.c_void_p(a.data_ptr()) if torch.is_tensor(a) else a for a in args],
                                        ctypes.c_void_p(stream))
    if rc != 0:
        raise RuntimeError("%s failed (status %d)" % (name, rc))


def _row_major(x):
    """x[chains, draws, d] as the kernel reads it: a draw is d contiguous doubles, a chain's draws follow each other, and
    chains are a whole number of rows apart -- a contiguous tensor, or the leading draws of one (trace_tensor(e, n))."""
    c, n, d = x.shape
    return x.stride(2) == 1 and x.stride(1) == d and (c <= 1 or (x.stride(0) % d == 0 and x.stride(0) >= n * d))


def _touched(first_chain, chains, per):
    """(g0, number of groups) that the job's chains [first_chain, first_chain + chains) touch, ``per`` chains a group."""
    g0 = first_chain // per
    return g0, (first_chain + chains - 1) // per - g0 + 1


# ---- a pass over the trace: the job (what is x?) and the fan-out (one kernel per device, the parts combined) --------------
# held: the blocks that hold chains, in job order; firsts: the job chain of each one's chain 0; chains: their total; per:
# chains per group; the chains touch the groups [g0, g0 + groups); n_draws, d: of every block; device: of the first block.
TraceJob = collections.namedtuple("TraceJob", "held firsts chains per g0 groups n_draws d device")


def _trace_job(x, chains_per_group=None, first_chain=0, target=None, whole_job=False, whole_groups=False,
               allow_first_chain=False):
    """The TraceJob of x: one tensor [chains, draws, d], or the list of the chain blocks of ONE job that this process holds on
    several GPUs (sample(..., devices=[...]) -> trace_tensor(group)), in job order -- and every refusal of such an x. Blocks
    without chains are dropped first; the others agree in draws and in d (``target.d``, with a target). ``chains_per_group``
    defaults to ``target.group_size(chains)`` (a ``targets.Batched``) or to one group of all chains. The rules a pass chooses:
    ``allow_first_chain``: x's first chain may be chain ``first_chain`` > 0 of the job (without: x is the whole job);
    ``whole_job``: the chains are all the chains of every posterior -- ``per`` times the target's groups, a multiple of ``per``
    without a target; ``whole_groups``: no group straddles two blocks. Not with an active process group."""
    blocks, first_chain = list(x) if isinstance(x, (list, tuple)) else [x], int(first_chain)
    if not blocks or any(b.dim() != 3 for b in blocks):
        raise ValueError("x must be [chains, draws, d] or a non-empty list of such blocks")
    if _group_active():
        raise ValueError("a pass over the trace with an active process group (sample_distributed) is not supported: it is "
                         "taken within one process (pass the list of its per-GPU blocks), not reduced across ranks")
    if first_chain != 0 and not allow_first_chain:
        raise ValueError("first_chain=%d: this x is the whole job (for this pass a list of blocks is), its first block starts at "
                         "chain 0" % first_chain)
    held = [b for b in blocks if b.shape[0] > 0]
    firsts = [first_chain + sum(int(a.shape[0]) for a in held[:i]) for i in range(len(held))]
    if not held:
        raise ValueError("x holds no chain")
    if len({int(b.shape[2]) for b in held}) > 1:
        raise ValueError("the chain blocks differ in d: %s" % [int(b.shape[2]) for b in held])
    if len({int(b.shape[1]) for b in held}) > 1:
        raise ValueError("the chain blocks hold different numbers of draws per chain: %s" % [int(b.shape[1]) for b in held])
    chains, n_draws, d = firsts[-1] + int(held[-1].shape[0]) - first_chain, int(held[0].shape[1]), int(held[0].shape[2])
    if n_draws < 1 or d < 1:
        raise ValueError("x holds no draw")
    if target is not None and d != target.d:
        raise ValueError("x has d = %d, the target d = %d" % (d, target.d))
    if chains_per_group is not None:
        per = int(chains_per_group)
    elif hasattr(target, "group_size"):
        if first_chain != 0:
            raise ValueError("a block of a Batched job that starts at first_chain=%d needs chains_per_group" % first_chain)
        per = target.group_size(chains)
    else:
        per = first_chain + chains
    if per < 1 or first_chain < 0:
        raise ValueError("chains_per_group must be >= 1 and first_chain >= 0 (got %d, %d)" % (per, first_chain))
    g0, groups = _touched(first_chain, chains, per)
    if target is not None:
        rows = getattr(target, "groups", 1)
        if whole_job and per * rows != chains:
            raise ValueError("%d chains at %d chains per group are not the %d posteriors of the target" % (chains, per, rows))
        if g0 + groups > rows:
            raise ValueError("chains %d .. %d at %d chains per group reach group %d; the target has %d"
                             % (first_chain, first_chain + chains - 1, per, g0 + groups - 1, rows))
    elif whole_job and chains % per != 0:
        raise ValueError("chains_per_group=%d needs a multiple of %d chains (got chains=%d)" % (per, per, chains))
    if whole_groups and any(f % per != 0 for f in firsts):
        raise ValueError("at %d chains per group a group straddles two chain blocks (blocks of %s chains); the draws of one "
                         "posterior form one row and need to lie on one device" % (per, [int(b.shape[0]) for b in held]))
    return TraceJob(held, firsts, chains, per, g0, groups, n_draws, d, held[0].device)


def _fan_out(job, ga, gb, call, combine):
    """One pass over the groups [ga, gb) of a job -> [gb - ga, ...] on ``job.device``. ``call(block, first_chain)`` runs the
    kernel on the part of those groups' chains that a block holds, on the block's own device, and returns [groups the part
    touches, ...]; every block's call is enqueued before the first result moves. The parts are then folded, in job order,
    into a block of zeros at their group offsets: ``combine(so far, part)`` is ``torch.add`` for sums and counts, or a merge
    that skips a side of count 0 by its count (predictive.merge, merge_moments) -- so zeros are the identity of each, and a
    group that straddles two blocks is the combination of its parts."""
    parts = []
    for b, f in zip(job.held, job.firsts):
        lo, hi = max(ga * job.per, f), min(gb * job.per, f + int(b.shape[0]))
        if lo < hi:
            parts.append((lo // job.per - ga, call(b[lo - f:hi - f], lo)))
    tot = None
    for off, part in parts:
        part = part.to(job.device)
        if tot is None:
            tot = torch.zeros((gb - ga,) + tuple(part.shape[1:]), dtype=part.dtype, device=job.device)
        tot[off:off + part.shape[0]] = combine(tot[off:off + part.shape[0]], part)
    return tot


def chain_stats_pass(x, ranges, lag0, stats_fn=None, chains_per_group=None, first_chain=0):
    """Statistics block of one pass: [3 + 16, d], or with ``chains_per_group`` [groups touched, 3 + 16, d] -- x's chain 0 is
    chain ``first_chain`` of the job, and a first or last group that lies only partly in x holds the sums over its chains
    that are present. A list of blocks (in job order) is added up: a group that straddles two blocks is the sum of its parts."""
    if isinstance(x, (list, tuple)):   # one kernel per device, all enqueued before the first result is moved
        if chains_per_group is not None:
            job = _trace_job(x, chains_per_group, first_chain, allow_first_chain=True)
            return _fan_out(job, job.g0, job.g0 + job.groups,
                            lambda b, f: _chain_stats_pass_grouped(b, ranges, lag0, stats_fn, job.per, f), torch.add)
        parts = [chain_stats_pass(b, ranges, lag0, stats_fn) for b in x]
        tot = parts[0]
        for p_ in parts[1:]:
            tot = tot + p_.to(tot.device)
        return tot
    if chains_per_group is not None:
        return _chain_stats_pass_grouped(x, ranges, lag0, stats_fn, int(chains_per_group), int(first_chain))
    return _chain_stats_pass_one(x, ranges, lag0, stats_fn)


def _device_block(x):
    """x as the HIP kernel reads it (float64, _row_major), or HipLibraryError for a CPU tensor."""
    if not x.is_cuda:
        from ._abi import HipLibraryError

        raise HipLibraryError("diagnostics run on draws in HBM (a ROCm tensor, e.g. diagnostics.trace_tensor(engine)); "
                              "got a CPU tensor and there is no host implementation")
    if x.dtype != torch.float64 or not _row_major(x):
        x = x.to(torch.float64).contiguous()
    return x


def _chain_stats_pass_grouped(x, ranges, lag0, stats_fn, per, first_chain):
    """[groups touched, 3 + 16, d] of one block. With ``stats_fn`` (tests of the logic) every touched group's chains are
    handed to it as one slice; without, the HIP kernel does all groups in one launch per range."""
    if per < 1 or first_chain < 0:
        raise ValueError("chains_per_group must be >= 1 and first_chain >= 0 (got %d, %d)" % (per, first_chain))
    c = int(x.shape[0])
    if c == 0:
        return torch.zeros((0, 3 + LAGS_PER_PASS, x.shape[2]), dtype=torch.float64, device=x.device)
    g0, touched = _touched(first_chain, c, per)
    if stats_fn is not None:
        cuts = [min(max((g0 + i) * per - first_chain, 0), c) for i in range(touched + 1)]
        return torch.stack([_chain_stats_pass_one(x[lo:hi], ranges, lag0, stats_fn) for lo, hi in zip(cuts[:-1], cuts[1:])])
    x = _device_block(x)
    tot = None
    for t0, n in ranges:
        blk = _hip_chain_stats(x, t0, n, lag0, first_chain, per)
        tot = blk if tot is None else tot + blk
    return tot


def _chain_stats_pass_one(x, ranges, lag0, stats_fn=None):
    """Statistics block [3 + 16, d] of one pass, summed over the sub-series ``ranges`` = [(t0, n), ...] of every
    chain of x (the two halves for split diagnostics). ``stats_fn(x, t0, n, lag0)`` replaces the HIP kernel (tests of
    the reduction logic only)."""
    if x.shape[0] == 0:
        return torch.zeros((3 + LAGS_PER_PASS, x.shape[2]), dtype=torch.float64, device=x.device)
    fn = stats_fn
    if fn is None:
        x = _device_block(x)
        fn = _hip_chain_stats
    tot = None
    for t0, n in ranges:
        blk = fn(x, t0, n, lag0)
        tot = blk if tot is None else tot + blk
    return tot


def _group_active(group=None):
    import torch.distributed as dist

    return dist.is_available() and dist.is_initialized()


def _all_reduce(t, group=None, reduce_device=None, op="sum"):
    """All-reduce over the ranks of ``group`` (a no-op without a process group). The collective runs even in a group
    of one rank: a single-GPU job under RCCL executes the very calls the 8-GPU job does."""
    import torch.distributed as dist

    if not _group_active(group):
        return t
    home = t.device
    r = t.clone() if reduce_device is None else t.to(reduce_device)
    dist.all_reduce(r, op={"sum": dist.ReduceOp.SUM, "max": dist.ReduceOp.MAX, "min": dist.ReduceOp.MIN}[op], group=group)
    return r.to(home)


def _geyer_ended(stats):
    """True when the initial positive sequence has ended within the available lags in every dimension (of every group:
    the lag axis is the last but one, whatever leads)."""
    m, n = float(stats["n_chains"]), float(stats["n_draws"])
    w = stats["sum_var"] / m
    gmean = stats["sum_mean"] / m
    b_over_n = (stats["sum_mean_sq"] - m * gmean ** 2) / (m - 1.0) if m > 1 else torch.zeros_like(w)
    var_plus = w * (n - 1.0) / n + b_over_n
    acov = stats["sum_acov"] / m
    rho = 1.0 - (w.unsqueeze(-2) - acov * (n / (n - 1.0))) / var_plus.unsqueeze(-2)
    rho[..., 0, :] = 1.0
    T = rho.shape[-2] - (rho.shape[-2] % 2)
    pairs = rho[..., 0:T:2, :] + rho[..., 1:T:2, :]
    return bool(((pairs <= 0).any(dim=-2) | ~torch.isfinite(pairs).all(dim=-2)).all())


def _chains_per_group(chains, chains_per_group, group=None):
    """``chains_per_group`` as an int, checked against the job's chain total; grouped diagnostics are a one-process matter."""
    per = int(chains_per_group)
    if _group_active(group):
        raise ValueError("chains_per_group with an active process group: targets.Batched does not run under "
                         "sample_distributed, and grouped diagnostics are not reduced across ranks")
    if per < 1 or chains < per or chains % per != 0:
        raise ValueError("chains_per_group=%d needs a multiple of %d chains (got chains=%d)" % (per, max(per, 1), chains))
    return per


def sufficient_stats(x, split=True, max_lag=None, group=None, reduce_device=None, stats_fn=None, chains_per_group=None):
    """Reduced (over chains, halves and ranks) sufficient statistics of x[chains, draws, d] (this rank's block, or the
    list of this process's per-GPU blocks). Every quantity that steers the pass loop -- the draw count, the lag limit,
    "Geyer's sequence has ended" -- is a REDUCED one, so all ranks issue the same collectives whatever their blocks hold
    (a rank may own no chain at all).

    ``chains_per_group=per``: the job's chains (the blocks, in job order) are G = chains / per posteriors of ``per``
    consecutive chains; every statistic gets a leading [G] axis, ``n_chains`` is the chains (times halves) of ONE group, and
    the passes continue until Geyer's sequence has ended in every dimension of every group -- still one host look per pass."""
    blocks = list(x) if isinstance(x, (list, tuple)) else [x]   # (no TraceJob: a rank of a process group may hold no chain)
    held = [b for b in blocks if b.shape[0] > 0]
    if len({int(b.shape[1]) for b in held}) > 1:
        raise ValueError("the chain blocks hold different numbers of draws per chain: %s" % [int(b.shape[1]) for b in held])
    c = sum(int(b.shape[0]) for b in blocks)
    per = None if chains_per_group is None else _chains_per_group(c, chains_per_group, group)
    n_all, d = (held[0].shape[1], held[0].shape[2]) if held else (blocks[0].shape[1], blocks[0].shape[2])
    dev = blocks[0].device
    if len(blocks) > 1:
        x = held if held else blocks[:1]
    else:
        x = blocks[0]
    # the draw count is agreed first: ranks that own chains must have the same, ranks that own none adopt it
    big = float(2 ** 52)
    mine = torch.tensor([float(n_all), -float(n_all)] if c > 0 else [0.0, -big], dtype=torch.float64, device=dev)
    agreed = _all_reduce(mine, group, reduce_device, op="max")
    n_max, n_min = int(agreed[0]), int(-agreed[1])
    if n_max == 0 and n_min >= int(big):
        raise ValueError("no rank holds any chain")
    if n_max != n_min:
        raise ValueError("ranks hold different numbers of draws per chain (%d .. %d)" % (n_min, n_max))
    n_all = n_max
    if split:
        h = n_all // 2
        ranges, n, halves = [(0, h), (n_all - h, h)], h, 2
    else:
        ranges, n, halves = [(0, n_all)], n_all, 1
    if n < 4:
        raise ValueError("need at least %d draws per chain" % (4 * halves))
    limit = n if max_lag is None else min(int(max_lag), n)
    nch = _all_reduce(torch.tensor([float((c if per is None else per) * halves)], dtype=torch.float64, device=dev), group,
                      reduce_device)
    stats = {"n_chains": nch[0], "n_draws": torch.tensor(float(n), dtype=torch.float64, device=dev)}
    if per is not None:
        stats["groups"] = c // per
    acov_blocks = []
    lag0 = 0
    while True:
        blk = _all_reduce(chain_stats_pass(x, ranges, lag0, stats_fn, per), group, reduce_device)   # the pass's one collective
        if lag0 == 0:
            stats["sum_mean"], stats["sum_mean_sq"], stats["sum_var"] = blk[..., 0, :], blk[..., 1, :], blk[..., 2, :]
        acov_blocks.append(blk[..., 3:, :])
        lag0 += LAGS_PER_PASS
        stats["sum_acov"] = torch.cat(acov_blocks, dim=-2)[..., :limit, :]
        if lag0 >= limit:
            break
        ended = torch.tensor([1.0 if _geyer_ended(stats) else 0.0], dtype=torch.float64, device=dev)
        if _group_active(group):   # the verdict is a function of reduced data, but ranks must not differ by a rounding
            ended = _all_reduce(ended, group, reduce_device, op="min")
        if float(ended[0]) > 0.5:
            break
    stats["lag_passes"] = len(acov_blocks)
    return stats


def finalize(stats):
    """R-hat[d] and ESS[d] from (reduced) sufficient statistics; [G, d] each, plus rhat_max[G], ess_min[G] and ``groups``,
    from grouped ones (sufficient_stats(..., chains_per_group=)): the lag axis is the last but one, whatever leads."""
    m = float(stats["n_chains"])
    n = float(stats["n_draws"])
    w = stats["sum_var"] / m                                              # mean within-chain variance
    gmean = stats["sum_mean"] / m
    if m > 1:
        b_over_n = (stats["sum_mean_sq"] - m * gmean ** 2) / (m - 1.0)    # variance of chain means
    else:
        b_over_n = torch.zeros_like(w)
    var_plus = w * (n - 1.0) / n + b_over_n
    rhat = torch.sqrt(var_plus / w)
    acov = stats["sum_acov"] / m                                          # [T, d]
    rho = 1.0 - (w.unsqueeze(-2) - acov * (n / (n - 1.0))) / var_plus.unsqueeze(-2)
    rho[..., 0, :] = 1.0
    T = rho.shape[-2]
    if T % 2:
        rho = rho[..., :-1, :]
        T -= 1
    pairs = rho[..., 0::2, :] + rho[..., 1::2, :]                         # Geyer P_t, [T/2, d]
    positive = torch.cumprod((pairs > 0).to(pairs.dtype), dim=-2)         # initial positive sequence
    pairs = torch.nan_to_num(pairs, nan=0.0) * positive
    pairs = torch.cummin(pairs, dim=-2).values                            # initial monotone sequence
    tau = -1.0 + 2.0 * pairs.sum(dim=-2)
    tau = torch.clamp(tau, min=1.0 / math.log10(max(m * n, 10.0)))
    ess = m * n / tau
    out = {"rhat": rhat, "ess": ess, "mean": gmean, "var": var_plus, "n_chains": m, "n_draws": n,
           "lag_passes": stats.get("lag_passes", 0)}
    if "groups" in stats:   # "which of my posteriors has not converged" is one comparison
        out.update(groups=stats["groups"], rhat_max=rhat.max(dim=-1).values, ess_min=ess.min(dim=-1).values)
    return out


def rank_normalize(x, chunk_dims=8, group=None, reduce_device=None, chains_per_group=None):
    """z-scores of the pooled ranks of every dimension (Vehtari et al. 2021, eq. 14): z = Phi^-1((r - 3/8) / (S + 1/4)),
    S = ALL chains x draws of ALL ranks, r = the average rank of the draw among them (ties -- a rejected HMC proposal, a
    NUTS tree that returns its start point -- share the mean of their positions, scipy's rankdata(method="average")).

    Multi-GPU: the ranks are global. Every rank sorts its own pooled draws of a block of dimensions, the sorted blocks
    are all-gathered (padded to the largest block with +inf), and a draw's global rank is the sum over ranks of its
    insertion points: r = #less + (#equal + 1) / 2. Normalising each rank's block on its own would map every block to
    N(0, 1) separately and erase exactly the between-rank differences R-hat is there to detect.

    ``chains_per_group=per``: the ranks are taken within each group of ``per`` consecutive chains (S = per x draws), all
    groups sorted in one call per chunk of dimensions. A list of blocks is taken block by block, which needs every group
    to lie inside one block."""
    import torch.distributed as dist

    if chains_per_group is not None:
        return _rank_normalize_grouped(x, chunk_dims, group, chains_per_group)
    if isinstance(x, (list, tuple)):
        return _rank_normalize_blocks(list(x), chunk_dims, group)
    c, n, d = x.shape
    S_local = c * n
    active = _group_active(group)
    S = S_local
    sizes = None
    if active:
        world = dist.get_world_size(group)
        cnt = torch.zeros((world,), dtype=torch.float64, device=x.device)
        cnt[dist.get_rank(group)] = float(S_local)
        sizes = [int(v) for v in _all_reduce(cnt, group, reduce_device)]
        S = sum(sizes)
    out = torch.empty((c, n, d), dtype=torch.float64, device=x.device)
    if active:   # the gathered pools of a chunk are world x chunk x (largest block) doubles on every rank: keep them <= ~1 GiB
        chunk_dims = max(1, min(int(chunk_dims), (1 << 30) // max(1, 8 * len(sizes) * max(sizes))))
    for lo in range(0, d, chunk_dims):
        hi = min(lo + chunk_dims, d)
        blk = x[:, :, lo:hi].reshape(S_local, hi - lo).to(torch.float64).t().contiguous()      # [k, S_local]
        srt = torch.sort(blk, dim=1).values
        if active:
            pad = max(sizes)
            mine = torch.full((hi - lo, pad), float("inf"), dtype=torch.float64, device=x.device)
            mine[:, :S_local] = srt
            send = mine if reduce_device is None else mine.to(reduce_device)
            gathered = [torch.empty_like(send) for _ in sizes]
            dist.all_gather(gathered, send, group=group)
            pools = [g.to(x.device)[:, :sz] for g, sz in zip(gathered, sizes)]
        else:
            pools = [srt]
        less = torch.zeros_like(blk)
        leq = torch.zeros_like(blk)
        for pool in pools:
            if pool.shape[1] == 0:
                continue
            less += torch.searchsorted(pool, blk, right=False).to(torch.float64)
            leq += torch.searchsorted(pool, blk, right=True).to(torch.float64)
        ranks = less + 0.5 * (leq - less + 1.0)
        p = (ranks - 0.375) / (S + 0.25)
        z = math.sqrt(2.0) * torch.erfinv(2.0 * p - 1.0)
        out[:, :, lo:hi] = z.t().reshape(c, n, hi - lo)
    return out


def _rank_normalize_grouped(x, chunk_dims, group, chains_per_group):
    """rank_normalize within groups of ``chains_per_group`` consecutive chains: one batched sort [G, k, per * n] per chunk of k
    dimensions, ties averaged as in the ungrouped form. Like that form it holds about six temporaries of chains x draws x k
    values (8 bytes each: float64 and the int64 insertion points) per chunk on the device -- 0.5 GB each at 16 384 chains x
    500 draws and k = 8; ``chunk_dims`` is the knob (call rank_normalize(x, chunk_dims=1, chains_per_group=per) and summarize
    its result when HBM is nearly full)."""
    if isinstance(x, (list, tuple)):
        per = _chains_per_group(sum(int(b.shape[0]) for b in x), chains_per_group, group)
        if any(int(b.shape[0]) % per for b in x):
            raise ValueError("rank_normalize(chains_per_group=%d): a group straddles two chain blocks (blocks of %s chains); "
                             "ranks within a group need the group's draws on one device"
                             % (per, [int(b.shape[0]) for b in x]))
        return [_rank_normalize_grouped(b, chunk_dims, group, per) if b.shape[0] else b.to(torch.float64) for b in x]
    c, n, d = x.shape
    per = _chains_per_group(c, chains_per_group, group)
    groups, S = c // per, per * n
    out = torch.empty((c, n, d), dtype=torch.float64, device=x.device)
    for lo in range(0, d, chunk_dims):
        hi = min(lo + chunk_dims, d)
        blk = x[:, :, lo:hi].reshape(groups, S, hi - lo).to(torch.float64).transpose(1, 2).contiguous()   # [G, k, S]
        srt = torch.sort(blk, dim=2).values
        less = torch.searchsorted(srt, blk, right=False).to(torch.float64)
        leq = torch.searchsorted(srt, blk, right=True).to(torch.float64)
        ranks = less + 0.5 * (leq - less + 1.0)
        p = (ranks - 0.375) / (S + 0.25)
        z = math.sqrt(2.0) * torch.erfinv(2.0 * p - 1.0)
        out[:, :, lo:hi] = z.transpose(1, 2).reshape(c, n, hi - lo)
    return out


def _rank_normalize_blocks(blocks, chunk_dims, group):
    """rank_normalize for the per-GPU chain blocks of one process: global ranks over ALL blocks. Every device sorts its
    own block of a chunk of dimensions; every device then counts its draws' insertion points in every sorted pool
    (copied device to device), exactly as the multi-process form does with all-gathered pools."""
    if _group_active(group):
        raise ValueError("per-GPU blocks inside one rank of a process group are not supported: use one device per rank")
    S = sum(int(b.shape[0]) * int(b.shape[1]) for b in blocks)
    d = int(blocks[0].shape[2])
    outs = [torch.empty(tuple(b.shape), dtype=torch.float64, device=b.device) for b in blocks]
    largest = max(int(b.shape[0]) * int(b.shape[1]) for b in blocks)
    chunk_dims = max(1, min(int(chunk_dims), (1 << 30) // max(1, 8 * len(blocks) * max(largest, 1))))
    for lo in range(0, d, chunk_dims):
        hi = min(lo + chunk_dims, d)
        flat = [b[:, :, lo:hi].reshape(-1, hi - lo).to(torch.float64).t().contiguous() for b in blocks]   # [k, S_b]
        pools = [torch.sort(f, dim=1).values for f in flat]
        for b, f, out in zip(blocks, flat, outs):
            if f.shape[1] == 0:
                continue
            less = torch.zeros_like(f)
            leq = torch.zeros_like(f)
            for pool in pools:
                if pool.shape[1] == 0:
                    continue
                pl = pool.to(f.device)
                less += torch.searchsorted(pl, f, right=False).to(torch.float64)
                leq += torch.searchsorted(pl, f, right=True).to(torch.float64)
            ranks = less + 0.5 * (leq - less + 1.0)
            p = (ranks - 0.375) / (S + 0.25)
            z = math.sqrt(2.0) * torch.erfinv(2.0 * p - 1.0)
            out[:, :, lo:hi] = z.t().reshape(b.shape[0], b.shape[1], hi - lo)
    return outs


def summarize(x, split=True, max_lag=None, group=None, reduce_device=None, rank_normalized=False, chunk=None,
              stats_fn=None, chains_per_group=None):
    """x[chains, draws, d] (this rank's chain block; or the list of this process's per-GPU blocks, trace_tensor(group))
    -> dict(rhat[d], ess[d], mean[d], var[d]) over ALL chains of ALL ranks.
    ``rank_normalized=True``: the rank-normalised split-R-hat / bulk ESS (diagnostics of the z-scores of the GLOBAL
    ranks). ``stats_fn`` replaces the HIP kernel (tests of the reduction logic only).
    ``chains_per_group=per`` (a ``targets.Batched`` job; ``Batched.summarize`` fills it in): one posterior per ``per``
    consecutive chains, all of them in the same passes -> rhat[G, d], ess[G, d], mean[G, d], var[G, d], rhat_max[G],
    ess_min[G], groups; n_chains counts the chains (halves) of one group. Not with a process group."""
    if rank_normalized:
        x = rank_normalize(x, group=group, reduce_device=reduce_device, chains_per_group=chains_per_group)
    out = finalize(sufficient_stats(x, split=split, max_lag=max_lag, group=group, reduce_device=reduce_device,
                                    stats_fn=stats_fn, chains_per_group=chains_per_group))
    out["definition"] = ("rank-normalised " if rank_normalized else "") + (
        "split-R-hat / Geyer initial-monotone-sequence ESS" if split else "R-hat / Geyer initial-monotone-sequence ESS")
    return out


def rhat_from_moments(mean, m2, n, group=None, reduce_device=None, chains_per_group=None):
    """(Non-split) R-hat[d] from per-chain running moments -- mean[chains, d], m2[chains, d] (sum of squared
    deviations), n[chains] equal draws per chain -- reduced over ranks with one all-reduce of
    {chains, draws, sum mean, sum mean^2, sum var}. This is the trace-free diagnostic of SURVEY.md section 8e.
    ``chains_per_group=per``: R-hat[G, d], one row per ``per`` consecutive chains (not with a process group)."""
    mean = torch.as_tensor(mean, dtype=torch.float64)
    m2 = torch.as_tensor(m2, dtype=torch.float64)
    nt = torch.as_tensor(n).to(torch.float64)
    d = mean.shape[1]
    if chains_per_group is not None:
        per = _chains_per_group(int(mean.shape[0]), chains_per_group, group)
        nd, m = float(nt.mean()), float(per)
        mean, m2 = mean.reshape(-1, per, d), m2.reshape(-1, per, d)
        w = (m2 / (nd - 1.0)).sum(dim=1) / m
        gmean = mean.sum(dim=1) / m
        b_over_n = ((mean ** 2).sum(dim=1) - m * gmean ** 2) / (m - 1.0) if per > 1 else torch.zeros_like(w)
        return torch.sqrt((w * (nd - 1.0) / nd + b_over_n) / w)
    nd_local = float(nt.mean()) if nt.numel() else 2.0
    blk = torch.zeros((3, d), dtype=torch.float64, device=mean.device)
    head = torch.zeros((2,), dtype=torch.float64, device=mean.device)
    if mean.shape[0]:
        blk[0], blk[1], blk[2] = mean.sum(dim=0), (mean ** 2).sum(dim=0), (m2 / (nd_local - 1.0)).sum(dim=0)
        head[0], head[1] = float(mean.shape[0]), float(nt.sum())
    blk = _all_reduce(blk, group, reduce_device)
    head = _all_reduce(head, group, reduce_device)
    m = float(head[0])
    nd = float(head[1]) / m
    w = blk[2] / m
    gmean = blk[0] / m
    b_over_n = (blk[1] - m * gmean ** 2) / (m - 1.0) if m > 1 else torch.zeros_like(w)
    return torch.sqrt((w * (nd - 1.0) / nd + b_over_n) / w)


class _DevicePtr:
    """__cuda_array_interface__ shim: view engine-owned HBM as a torch tensor without copying."""

    def __init__(self, ptr, shape, typestr="<f8"):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2}


def trace_tensor(engine, n_draws=None):
    """Zero-copy torch view [chains, trace_rows, dim] of the engine's draws in HBM (an EngineGroup: the list
    of its engines' views, one per GPU -- summarize() takes it as it is): capacity - trace_begin rows, or, on a thinned
    engine (reserve(thin=k)), the ceil((capacity - trace_begin) / k) kept draws. ``n_draws`` keeps the first n_draws rows of
    every chain only: the rows an interrupted run has actually written."""
    if hasattr(engine, "engines"):
        return [trace_tensor(e, n_draws) for e in engine.engines]
    if n_draws is not None:
        return trace_tensor(engine)[:, :max(int(n_draws), 0)]
    ptr = engine.trace_device_ptr()
    if not ptr:
        raise RuntimeError("the engine keeps no trace (reserve(keep_trace=False))")
    engine.synchronize()
    shape = (engine.chains, engine.trace_rows(), engine.dim)
    return torch.as_tensor(_DevicePtr(ptr, shape), device="cuda:%d" % engine.cfg.device)


# ---- exact order statistics of the trace in place: posterior quantiles, credible intervals, tail-ESS ---------------------
# A radix select over the order-preserving 64-bit keys of the draws (include/lmc_hip.h: lmc_select_digit_counts). A pass is
# an INTEGER HISTOGRAM of one key digit, which adds over chains, chain blocks and GPUs exactly, so a posterior spread over
# several devices is no special case; eight passes leave the key of the wanted draw, bit for bit. Keys and prefixes travel
# as int64 tensors holding the unsigned bits.
SELECT_SHIFTS = (56, 48, 40, 32, 24, 16, 8, 0)
_INT64_MIN = -(1 << 63)


def _hip_select_counts(x, first_chain, per, shift, prefix):
    """One call of lmc_select_digit_counts over x[chains, draws, d] (a ROCm tensor): -> [groups touched, n_ranks, 256, d] int64
    on x's device. ``prefix`` is [groups touched, n_ranks, d] int64 on that device (None at shift 56: one rank slot)."""
    c, _n, d = x.shape
    touched = _touched(first_chain, c, per)[1]
    n_ranks = 1 if prefix is None else int(prefix.shape[1])
    if prefix is not None:
        prefix = prefix.contiguous()
        if tuple(prefix.shape) != (touched, n_ranks, d) or prefix.dtype != torch.int64 or prefix.device != x.device:
            raise ValueError("prefix must be int64 [%d, n_ranks, %d] on %s" % (touched, d, x.device))
    out = torch.empty((touched, n_ranks, 256, d), dtype=torch.int64, device=x.device)
    _call_trace_kernel("lmc_select_digit_counts", x, int(first_chain), int(per), int(shift), n_ranks, prefix, out)
    return out


def _select_job(x, chains_per_group):
    """The TraceJob of an order-statistics job: the whole job, all chains of every group; a group may straddle blocks."""
    return _trace_job(x, chains_per_group, whole_job=True)


def _select_counts(job, ga, gb, shift, prefix, count_fn):
    """Digit counts [gb - ga, n_ranks, 256, d] of the groups [ga, gb) of the job, on ``job.device``: every block counts the
    part of those groups' chains it holds, on its own device, and the parts are added (_fan_out)."""
    fn = _hip_select_counts if count_fn is None else count_fn

    def call(b, first):
        off, touched = _touched(first, int(b.shape[0]), job.per)
        return fn(b, first, job.per, shift, None if prefix is None else prefix[off - ga:off - ga + touched].to(b.device))

    for b, f in zip(job.held, job.firsts):   # one block holds all these chains: its counts are the sum -- moved, not added to
        if f <= ga * job.per and gb * job.per <= f + int(b.shape[0]):   # zeros (exact for integers, and half the memory)
            return call(b[ga * job.per - f:gb * job.per - f], ga * job.per).to(job.device)
    return _fan_out(job, ga, gb, call, torch.add)


def order_statistics(x, ranks, chains_per_group=None, scratch_bytes=1 << 30, count_fn=None):
    """Exact order statistics of the draws in HBM: entry k of the result [Q', d] float64 (with ``chains_per_group=per``:
    [G, Q', d], one posterior per ``per`` consecutive chains) is the ``ranks[k]``-th smallest (0-based) of the S = chains of a
    group x draws values of that dimension -- the draw itself, bit for bit. The order is the IEEE total order on the bits
    (-NaN < -inf < .. < -0 < +0 < .. < +inf < +NaN).

    x is one tensor [chains, draws, d], or the list of per-GPU blocks of one job (``trace_tensor(engine_group)``): every block
    is counted on its own device at its running first chain, the integer counts are added on the first block's device, and a
    group -- or the whole ungrouped job -- may straddle blocks. Eight passes over the trace (lmc_select_digit_counts, 8 key
    bits each, most significant first): after each, per (group, rank, dimension), the bucket where the cumulative count passes
    the remaining rank extends the prefix and the count below it is subtracted. Duplicated ranks are selected once; more than
    16 distinct ranks take several rounds of passes that share the first (shift 56) pass. The groups are taken in chunks so
    that the counts of a pass ([groups, ranks of the round, 256, d] int64) stay within ``scratch_bytes``; ValueError if one
    group alone does not fit. Nothing in the pass loop looks at the host. ``count_fn(x, first_chain, per, shift, prefix) ->
    counts`` replaces the HIP call (tests of this logic only); without it a CPU tensor raises HipLibraryError. Not with an
    active process group."""
    from . import _abi

    job = _select_job(x, chains_per_group)
    G, d, dev, S = job.groups, job.d, job.device, job.per * job.n_draws
    want = [int(r) for r in ranks]
    if not want:
        raise ValueError("no ranks")
    if min(want) < 0 or max(want) >= S:
        raise ValueError("ranks must lie in [0, %d) (got %d .. %d)" % (S, min(want), max(want)))
    uniq = sorted(set(want))
    rounds = [uniq[i:i + _abi.SELECT_MAX_RANKS] for i in range(0, len(uniq), _abi.SELECT_MAX_RANKS)]
    unit = 256 * d * 8 * max(len(r) for r in rounds)
    chunk = int(scratch_bytes) // unit
    if chunk < 1:
        raise ValueError("scratch_bytes=%d is below the %d bytes of one group's counts (%d ranks x 256 x %d dimensions x 8)"
                         % (scratch_bytes, unit, max(len(r) for r in rounds), d))
    out = torch.empty((G, len(uniq), d), dtype=torch.float64, device=dev)
    for ga in range(0, G, chunk):
        gb = min(ga + chunk, G)
        # the shift-56 pass is shared by the rounds; the cumulative counts overwrite the counts (no second table)
        first = _select_counts(job, ga, gb, SELECT_SHIFTS[0], None, count_fn).cumsum_(2)
        q0 = 0
        for rks in rounds:
            rem = torch.tensor(rks, dtype=torch.int64, device=dev).reshape(1, -1, 1).expand(gb - ga, len(rks), d).contiguous()
            prefix = torch.zeros((gb - ga, len(rks), d), dtype=torch.int64, device=dev)
            for shift in SELECT_SHIFTS:
                if shift == SELECT_SHIFTS[0]:
                    cum = first.expand(-1, len(rks), -1, -1)                      # [g, ranks, 256, d]
                else:
                    cum = _select_counts(job, ga, gb, shift, prefix, count_fn).cumsum_(2)
                bucket = (cum <= rem.unsqueeze(2)).sum(dim=2).clamp_(max=255)     # the first bucket whose cumulative count passes
                below = torch.gather(cum, 2, (bucket - 1).clamp_(min=0).unsqueeze(2)).squeeze(2)
                rem = rem - torch.where(bucket > 0, below, torch.zeros_like(below))
                prefix = prefix | (bucket << shift)
            bits = torch.where(prefix < 0, prefix ^ _INT64_MIN, ~prefix)          # the key back to the draw's bits
            out[ga:gb, q0:q0 + len(rks)] = bits.view(torch.float64)
            q0 += len(rks)
    pick = torch.tensor([uniq.index(r) for r in want], dtype=torch.int64, device=dev)
    out = out.index_select(1, pick)
    return out if chains_per_group is not None else out[0]


def _probs(probs):
    """``probs`` as a list of floats, validated: the one refusal of every ``probs=`` of this package."""
    probs = [float(p) for p in (probs.tolist() if hasattr(probs, "tolist") else probs)]
    if not probs or any(not (0.0 <= p <= 1.0) for p in probs):
        raise ValueError("probs must be a non-empty sequence of numbers in [0, 1] (got %r)" % (probs,))
    return probs


def _quantile_plan(S, probs):
    """What the quantiles at ``probs`` of S sorted values v need, by numpy's default interpolation

        h = p (S - 1),  lo = floor(h),  q = v[lo] + (v[min(lo + 1, S - 1)] - v[lo]) (h - lo)

    -> (the validated probs, ranks = [0, S - 1] + lo + hi to hand to :func:`order_statistics`, frac = h - lo)."""
    probs = _probs(probs)
    h = [p * (S - 1) for p in probs]
    lo = [int(math.floor(v)) for v in h]
    hi = [min(k + 1, S - 1) for k in lo]
    return probs, [0, S - 1] + lo + hi, [a - b for a, b in zip(h, lo)]


def _interpolate(os_, frac, link=None):
    """The select's result ``os_[..., 2 + 2 Q, d]`` at the ranks of :func:`_quantile_plan` -> (min[..., d], max[..., d],
    quantiles[..., Q, d] = vlo + (vhi - vlo) frac). A column whose min or max is NaN holds a NaN value and all its quantiles
    are NaN, as numpy's are. With ``link``, a monotone map, a fourth entry: the quantiles of link(v) -- the sorted link(v) ARE
    the link of the sorted v, so the map is applied to vlo and vhi and the interpolation is done on its scale, no second select."""
    Q = len(frac)
    vmin, vmax = os_[..., 0, :], os_[..., 1, :]
    vlo, vhi = os_[..., 2:2 + Q, :], os_[..., 2 + Q:, :]
    frac = torch.tensor(frac, dtype=torch.float64, device=os_.device).reshape(Q, 1)
    bad = (torch.isnan(vmin) | torch.isnan(vmax)).unsqueeze(-2)

    def band(lo, hi):
        q = lo + (hi - lo) * frac
        return torch.where(bad, torch.full_like(q, float("nan")), q)

    out = (vmin, vmax, band(vlo, vhi))
    return out if link is None else out + (band(link(vlo), link(vhi)),)


def quantiles(x, probs, chains_per_group=None, **kw):
    """Posterior quantiles from the trace in place -> dict(quantiles[Q, d], min[d], max[d], n, probs); with
    ``chains_per_group=per`` quantiles[G, Q, d], min[G, d], max[G, d]. With v the sorted S = chains x draws values of a
    (group, dimension), by linear interpolation between order statistics (numpy's default):

        h = p (S - 1),  lo = floor(h),  q = v[lo] + (v[min(lo + 1, S - 1)] - v[lo]) (h - lo)

    v[lo] and v[lo + 1] are exact (``order_statistics``; ``**kw`` goes there); ``min`` and ``max`` are ranks 0 and S - 1,
    always selected; ``n`` is S. A (group, dimension) whose min or max is NaN holds a NaN draw and all its quantiles are
    NaN, as numpy's are. ``probs`` must lie in [0, 1] and must not be empty."""
    job = _select_job(x, chains_per_group)
    S = job.per * job.n_draws
    probs, ranks, frac = _quantile_plan(S, probs)
    vmin, vmax, q = _interpolate(order_statistics(x, ranks, chains_per_group=chains_per_group, **kw), frac)
    return {"quantiles": q, "min": vmin, "max": vmax, "n": S, "probs": probs}


def intervals(x, level=0.9, chains_per_group=None, **kw):
    """Equal-tailed credible intervals -> dict(lower, median, upper, level): the quantiles at (1 - level) / 2, 1 / 2 and
    1 - (1 - level) / 2 of ``quantiles`` ([d] each, [G, d] with ``chains_per_group``). Highest-density intervals are not
    computed."""
    level = float(level)
    if not (0.0 < level < 1.0):
        raise ValueError("level must lie in (0, 1) (got %r)" % (level,))
    tail = (1.0 - level) / 2.0
    q = quantiles(x, [tail, 0.5, 1.0 - tail], chains_per_group=chains_per_group, **kw)["quantiles"]
    return {"lower": q[..., 0, :], "median": q[..., 1, :], "upper": q[..., 2, :], "level": level}


def tail_ess(x, probs=(0.05, 0.95), split=True, chains_per_group=None, chunk_dims=8, stats_fn=None, **kw):
    """Tail effective sample size (Vehtari et al. 2021): the minimum over ``probs`` of the (split) ESS of the indicator
    x <= q_p, q_p the posterior quantile of ``quantiles`` -> dict(ess_tail[d]); ess_tail[G, d] and ess_tail_min[G] with
    ``chains_per_group``. The indicator is built for ``chunk_dims`` dimensions at a time -- the temporary is chains x draws x
    chunk_dims doubles, the bound rank_normalize keeps -- and goes through ``sufficient_stats`` / ``finalize`` like any draws.
    ``**kw`` goes to ``order_statistics``; ``stats_fn`` to ``sufficient_stats``."""
    q = quantiles(x, probs, chains_per_group=chains_per_group, **kw)["quantiles"]
    job = _select_job(x, chains_per_group)
    best = None
    for k in range(q.shape[-2]):
        ess = _indicator_ess(job, q[..., k, :], torch.le, split, chunk_dims, stats_fn, chains_per_group)
        best = ess if best is None else torch.minimum(best, ess)
    out = {"ess_tail": best, "probs": [float(p) for p in probs]}
    if chains_per_group is not None:
        out.update(groups=job.groups, ess_tail_min=best.min(dim=-1).values)
    return out


def _indicator_ess(job, q, below, split, chunk_dims, stats_fn, chains_per_group):
    """The (split) ESS of the indicator ``below(x, q)`` of the job's draws -> [d] on q's device, [G, d] with ``chains_per_group``
    (q is then [G, d]: every chain is compared with the value of its own group). ``below`` is ``torch.le`` (tail_ess) or
    ``torch.lt`` (prob). The indicator is built for ``chunk_dims`` dimensions at a time -- the temporary is chains x draws x
    chunk_dims doubles -- and goes through ``sufficient_stats`` / ``finalize`` like any draws."""
    parts = []
    for lo in range(0, job.d, int(chunk_dims)):
        hi = min(lo + int(chunk_dims), job.d)
        ind = []
        for b, f in zip(job.held, job.firsts):
            qk = q[..., lo:hi].to(b.device)
            if chains_per_group is not None:   # the value of every chain's own group
                rows = (torch.arange(int(b.shape[0]), device=b.device) + f) // job.per
                qk = qk.index_select(0, rows)
                ind.append(below(b[:, :, lo:hi], qk.unsqueeze(1)).to(torch.float64))
            else:
                ind.append(below(b[:, :, lo:hi], qk).to(torch.float64))
        st = sufficient_stats(ind if len(ind) > 1 else ind[0], split=split, stats_fn=stats_fn, chains_per_group=chains_per_group)
        parts.append(finalize(st)["ess"].to(q.device))
    return torch.cat(parts, dim=-1)


# ---- threshold counts of the trace in place: P(q < c), probability of direction, ROPE, ranks for calibration --------------
# The inverse question of the select: which rank a value has. Per (posterior, coefficient, threshold) the draws below and
# equal to the threshold, and per (posterior, coefficient) the NaN draws (include/lmc_hip.h: lmc_diag_threshold_counts,
# csrc/lmc_threshold.hip): integers that add over chains, chain blocks and GPUs exactly. IEEE numeric comparisons.
def _hip_threshold_counts(x, first_chain, per, thresholds):
    """One call of lmc_diag_threshold_counts over x[chains, draws, d] (a ROCm tensor): thresholds [groups touched, K, d] float64
    on x's device, K <= 16 -> counts [groups touched, 2 K + 1, d] int64 there (2k: below, 2k + 1: equal, 2K: NaN draws)."""
    x = _device_block(x)
    c, _n, d = x.shape
    touched = _touched(first_chain, c, per)[1]
    thresholds = thresholds.contiguous()
    K = int(thresholds.shape[1]) if thresholds.dim() == 3 else 0
    if tuple(thresholds.shape) != (touched, K, d) or thresholds.dtype != torch.float64 or thresholds.device != x.device:
        raise ValueError("thresholds must be float64 [%d, K, %d] on %s" % (touched, d, x.device))
    out = torch.empty((touched, 2 * K + 1, d), dtype=torch.int64, device=x.device)
    _call_trace_kernel("lmc_diag_threshold_counts", x, int(first_chain), int(per), K, thresholds, out)
    return out


def _threshold_block(thresholds, G, d, grouped):
    """``thresholds`` as a float64 tensor [G, K, d]: [K, d]; a scalar, [d] or 1-D of length K (a length of d is a [d]), all
    broadcast to [K, d] and shared by the groups; with ``grouped`` also [G, K, d]. ValueError for any other shape."""
    t = torch.as_tensor(thresholds, dtype=torch.float64)
    if t.dim() == 0:
        t = t.reshape(1, 1)
    elif t.dim() == 1:
        t = t.reshape(1, d) if t.shape[0] == d else t.reshape(-1, 1)
    if t.dim() == 2 and t.shape[0] >= 1 and t.shape[1] in (1, d):
        return t.expand(t.shape[0], d).unsqueeze(0).expand(G, -1, -1)
    if t.dim() == 3 and grouped and t.shape[0] == G and t.shape[1] >= 1 and t.shape[2] == d:
        return t
    raise ValueError("thresholds must be a scalar, [%d], [K] or [K, %d]%s (got shape %s)"
                     % (d, d, ", or [%d, K, %d]" % (G, d) if grouped else "", tuple(t.shape)))


def threshold_counts(x, thresholds, chains_per_group=None, count_fn=None):
    """How many draws in HBM lie below and at each threshold -> dict(less[K, d], equal[K, d] int64, nan[d] int64, n = S): per
    coefficient j and threshold k, over the S = chains of a group x draws values v of the coefficient, ``less`` counts v < c,
    ``equal`` v == c and ``nan`` the NaN draws, so S - less - equal - nan lie above. With ``chains_per_group=per`` (one posterior
    per ``per`` consecutive chains) less, equal [G, K, d] and nan [G, d]. The comparisons are IEEE numeric ones: -0.0 == +0.0, a
    NaN draw is neither below nor equal to anything, a NaN threshold counts 0 and 0. ``less`` is the RANK of the threshold
    among the draws: the inverse of ``order_statistics``.

    x is one tensor [chains, draws, d], or the list of per-GPU blocks of one job (``trace_tensor(engine_group)``): every block
    is counted on its own device at its running first chain, the integer counts are added on the first block's device, and a
    group may straddle blocks. ``thresholds`` is array-like: [K, d]; a scalar, [d] or 1-D of length K, broadcast to [K, d] (a
    1-D length of d is read as [d]); with ``chains_per_group`` also [G, K, d], each posterior its own. One pass over the trace
    (lmc_diag_threshold_counts) serves up to 16 thresholds; more run in rounds of 16. ``count_fn(x, first_chain, per,
    thresholds[groups touched, K, d]) -> counts[groups touched, 2 K + 1, d]`` replaces the HIP call (tests of this logic only);
    without it a CPU tensor raises HipLibraryError. Not with an active process group."""
    from . import _abi

    job = _trace_job(x, chains_per_group, whole_job=True)
    G, d, dev = job.groups, job.d, job.device
    thr = _threshold_block(thresholds, G, d, chains_per_group is not None).to(dev)
    K = int(thr.shape[1])
    fn = _hip_threshold_counts if count_fn is None else count_fn

    def call(b, first):
        off, touched = _touched(first, int(b.shape[0]), job.per)
        return fn(b, first, job.per, part[off:off + touched].to(b.device).contiguous())

    less = torch.empty((G, K, d), dtype=torch.int64, device=dev)
    equal = torch.empty((G, K, d), dtype=torch.int64, device=dev)
    nan = None
    for k0 in range(0, K, _abi.THRESHOLD_MAX):
        k1 = min(k0 + _abi.THRESHOLD_MAX, K)
        part = thr[:, k0:k1]
        if len(job.held) == 1:   # one block holds all chains: its counts are the sum -- moved, not added to zeros
            cnt = call(job.held[0], 0).to(dev)
        else:
            cnt = _fan_out(job, 0, G, call, torch.add)
        less[:, k0:k1], equal[:, k0:k1], nan = cnt[:, 0:2 * (k1 - k0):2], cnt[:, 1:2 * (k1 - k0):2], cnt[:, 2 * (k1 - k0)]
    out = {"less": less, "equal": equal, "nan": nan, "n": job.per * job.n_draws}
    if chains_per_group is None:
        out.update(less=less[0], equal=equal[0], nan=nan[0])
    return out


def _divisor(S, like):
    """S as a tensor divisor next to ``like``: count / S is then ONE correctly rounded division on every device (a Python
    scalar divisor may be turned into a multiplication by its reciprocal, which differs in the last bit)."""
    return torch.tensor(float(S), dtype=torch.float64, device=like.device)


def _nan_where(bad, t):
    return torch.where(bad, torch.full_like(t, float("nan")), t)


def prob(x, thresholds, chains_per_group=None, mcse=False, split=True, chunk_dims=8, stats_fn=None, **kw):
    """Posterior probabilities from the trace in place -> dict(p_less, p_equal, p_greater [K, d] float64, n = S, n_nan[d]):
    the counts of ``threshold_counts`` (``thresholds``, ``**kw`` go there) over S, and p_greater = (S - less - equal) / S;
    [G, K, d] and n_nan[G, d] with ``chains_per_group``. P(q_e > 0) is ``prob(x, 0.0)["p_greater"]``. A (posterior,
    coefficient) that holds a NaN draw is NaN at every threshold and no other is -- the rule ``quantiles`` keeps.

    ``mcse=True`` adds ``ess`` and ``mcse = sqrt(p (1 - p) / ess)`` of p_less: ``ess`` is the (split) ESS of the indicator
    x < c, built ``chunk_dims`` dimensions at a time as ``tail_ess`` builds its indicator (``stats_fn`` goes to
    ``sufficient_stats``). An indicator that is constant (p_less of 0 or 1) has no autocorrelation to estimate: its ess and
    mcse are NaN."""
    tc = threshold_counts(x, thresholds, chains_per_group=chains_per_group, **kw)
    bad = (tc["nan"] > 0).unsqueeze(-2)
    less, equal = tc["less"].to(torch.float64), tc["equal"].to(torch.float64)
    S = _divisor(tc["n"], less)
    out = {"p_less": _nan_where(bad, less / S), "p_equal": _nan_where(bad, equal / S),
           "p_greater": _nan_where(bad, (S - less - equal) / S), "n": tc["n"], "n_nan": tc["nan"]}
    if mcse:
        job = _trace_job(x, chains_per_group, whole_job=True)
        thr = _threshold_block(thresholds, job.groups, job.d, chains_per_group is not None).to(job.device)
        if chains_per_group is None:
            thr = thr[0]
        ess = torch.stack([_indicator_ess(job, thr[..., k, :], torch.lt, split, chunk_dims, stats_fn, chains_per_group)
                           for k in range(thr.shape[-2])], dim=-2)
        p = out["p_less"]
        out.update(ess=ess, mcse=torch.sqrt(p * (1.0 - p) / ess))
    return out


def direction(x, chains_per_group=None, **kw):
    """Probability of direction -> dict(pd[d], sign[d], n): ``pd = max(P(q > 0), P(q < 0))`` and ``sign`` = +1 where P(q > 0) >=
    P(q < 0), else -1 (float64); [G, d] with ``chains_per_group``. One threshold, 0, of ``prob`` (``**kw`` goes there); NaN where
    the coefficient holds a NaN draw."""
    p = prob(x, 0.0, chains_per_group=chains_per_group, **kw)
    pos, neg = p["p_greater"][..., 0, :], p["p_less"][..., 0, :]
    sign = torch.where(pos >= neg, torch.ones_like(pos), -torch.ones_like(pos))
    return {"pd": torch.maximum(pos, neg), "sign": _nan_where(torch.isnan(pos), sign), "n": p["n"]}


def rope(x, low, high, chains_per_group=None, **kw):
    """Region of practical equivalence -> dict(inside, below, above [d], n): ``inside = P(low <= q <= high)``, ``below = P(q <
    low)``, ``above = P(q > high)``; [G, d] with ``chains_per_group``. ``low`` and ``high`` are scalars or [d] (with
    ``chains_per_group`` also [G, d]), low <= high. The two thresholds go through ONE pass of ``threshold_counts`` (``**kw``
    goes there): ``inside = (less_high + equal_high - less_low) / S``. NaN where the coefficient holds a NaN draw."""
    job = _trace_job(x, chains_per_group, whole_job=True)
    lead = (job.groups, job.d) if chains_per_group is not None else (job.d,)
    try:
        lo = torch.as_tensor(low, dtype=torch.float64).to(job.device).expand(lead)
        hi = torch.as_tensor(high, dtype=torch.float64).to(job.device).expand(lead)
    except RuntimeError:
        raise ValueError("low and high must be scalars or broadcast to %s" % (lead,))
    if bool((lo > hi).any()):
        raise ValueError("rope needs low <= high")
    tc = threshold_counts(x, torch.stack([lo, hi], dim=-2), chains_per_group=chains_per_group, **kw)
    bad = tc["nan"] > 0
    less, equal = tc["less"].to(torch.float64), tc["equal"].to(torch.float64)
    S = _divisor(tc["n"], less)
    less_lo, less_hi, equal_hi = less[..., 0, :], less[..., 1, :], equal[..., 1, :]
    return {"inside": _nan_where(bad, (less_hi + equal_hi - less_lo) / S), "below": _nan_where(bad, less_lo / S),
            "above": _nan_where(bad, (S - less_hi - equal_hi) / S), "n": tc["n"]}


# ---- posterior covariance and correlation per posterior: the co-moment matrix of the draws in place ------------------------
# One contraction over the (chain, draw) rows of every group on the FP64 matrix cores (include/lmc_hip.h:
# lmc_diag_cross_moments, csrc/lmc_cross.hip) -> n[G], mean[G, d], m2[G, d, d]; blocks merge by Chan's rule for matrices.
def _hip_cross_moments(x, first_chain, per):
    """One call of lmc_diag_cross_moments over x[chains, draws, d] (a ROCm tensor), x's chain 0 being chain ``first_chain`` of
    the job: -> dict(n[groups touched], mean[.., d], m2[.., d, d]) float64 on x's device."""
    from . import _abi

    c, _n, d = x.shape
    if d > _abi.CROSS_MAX_DIM:
        raise ValueError("cross_moments: d = %d is beyond the %d dimensions of lmc_diag_cross_moments" % (d, _abi.CROSS_MAX_DIM))
    touched = _touched(first_chain, c, per)[1]
    out = {"n": torch.empty((touched,), dtype=torch.float64, device=x.device),
           "mean": torch.empty((touched, d), dtype=torch.float64, device=x.device),
           "m2": torch.empty((touched, d, d), dtype=torch.float64, device=x.device)}
    _call_trace_kernel("lmc_diag_cross_moments", x, int(first_chain), int(per), out["n"], out["mean"], out["m2"])
    return out


def merge_cross_moments(a, b):
    """Two results dict(n[G], mean[G, d], m2[G, d, d]) over disjoint sets of draws of the same groups -> the result over their
    union, by Chan's rule for matrices:

        n = na + nb,  mean = ma + (mb - ma) nb / n,  m2 = m2a + m2b + (mb - ma)(mb - ma)^T na nb / n

    A side of count 0 is skipped BY ITS COUNT: the other side comes through bit for bit, whatever the empty side holds, so
    zeros are the identity. The outer product of one vector with itself is symmetric bit for bit, so symmetric sides merge to
    a symmetric matrix."""
    na, nb = a["n"], b["n"]
    n = na + nb
    delta = b["mean"] - a["mean"]
    mean = a["mean"] + delta * (nb / n).unsqueeze(-1)
    m2 = a["m2"] + b["m2"] + delta.unsqueeze(-1) * delta.unsqueeze(-2) * (na * nb / n).unsqueeze(-1).unsqueeze(-1)
    only_a, only_b = nb == 0, na == 0
    pick = lambda ta, tb, both, k: torch.where(only_a.reshape(only_a.shape + (1,) * k), ta,
                                               torch.where(only_b.reshape(only_b.shape + (1,) * k), tb, both))
    return {"n": pick(na, nb, n, 0), "mean": pick(a["mean"], b["mean"], mean, 1), "m2": pick(a["m2"], b["m2"], m2, 2)}


def _pack_cross(m):
    """dict(n[g], mean[g, d], m2[g, d, d]) as one tensor [g, 1 + d + d d] (what _fan_out folds), and back."""
    g = m["n"].shape[0]
    return torch.cat([m["n"].reshape(g, 1), m["mean"], m["m2"].reshape(g, -1)], dim=1)


def _unpack_cross(t, d):
    return {"n": t[:, 0], "mean": t[:, 1:1 + d], "m2": t[:, 1 + d:].reshape(t.shape[0], d, d)}


def cross_moments(x, chains_per_group=None, first_chain=0, moments_fn=None, target=None):
    """Count, mean and co-moment matrix of the draws in HBM per posterior -> dict(n[G], mean[G, d], m2[G, d, d]) on the first
    block's device, ``m2 = sum over the group's (chain, draw) rows of (x - mean)(x - mean)^T``, exactly symmetric. One
    posterior per ``chains_per_group`` consecutive chains of the job (default: ``target.group_size`` of a ``targets.Batched``,
    else one group of all chains -- and then, without a Batched target, the leading axis is dropped, as ``summarize`` does).
    x is one tensor [chains, draws, d] whose chain 0 is chain ``first_chain`` of the job -- a first or last group that lies only
    partly in x gets the moments of its chains that are present -- or the list of per-GPU blocks of one job in job order: every
    block is taken on its own device and the parts are merged in job order (``merge_cross_moments``), so a group may straddle
    blocks. d <= 512. ``moments_fn(x, first_chain, per) -> dict`` replaces the HIP call (tests of this logic only); without it
    a CPU tensor raises HipLibraryError. Not with an active process group."""
    job = _trace_job(x, chains_per_group, first_chain, target=target, allow_first_chain=True)
    fn = _hip_cross_moments if moments_fn is None else moments_fn
    d = job.d
    if len(job.held) == 1:
        out = fn(job.held[0], job.firsts[0], job.per)
        out = {k: out[k].to(job.device) for k in ("n", "mean", "m2")}
    else:
        out = _unpack_cross(_fan_out(job, job.g0, job.g0 + job.groups, lambda b, f: _pack_cross(fn(b, f, job.per)),
                                     lambda a, b: _pack_cross(merge_cross_moments(_unpack_cross(a, d), _unpack_cross(b, d)))), d)
    if chains_per_group is None and not hasattr(target, "group_size"):
        out = {k: v[0] for k, v in out.items()}
    return out


def _cov_of(moments, ddof):
    """cov = m2 / (n - ddof), NaN where n - ddof <= 0 (numpy.cov warns and divides by zero there; here it is NaN throughout)."""
    dof = moments["n"] - float(ddof)
    dof = torch.where(dof > 0, dof, torch.full_like(dof, float("nan")))
    return moments["m2"] / dof.unsqueeze(-1).unsqueeze(-1)


def covariance(x, chains_per_group=None, ddof=1, **kw):
    """Posterior covariance and correlation per posterior from the draws in HBM -> dict(n, mean, cov, sd, corr, m2):
    ``cov = m2 / (n - ddof)`` ([G, d, d]; NaN where n - ddof <= 0, like numpy.cov), ``sd = sqrt(diag cov)``, ``corr_ij = m2_ij /
    sqrt(m2_ii m2_jj)`` clipped to [-1, 1] as numpy.corrcoef does, exactly 1 on the diagonal, and NaN in the row and column of
    a coordinate whose variance is 0 or not finite. ``**kw`` goes to ``cross_moments`` (``first_chain``, ``target``,
    ``moments_fn``); the leading axis is dropped as there.

    This is the SAMPLE covariance of autocorrelated draws, all chains of a posterior pooled. It estimates the posterior
    covariance; it says nothing about the Monte Carlo error of that estimate (see ``summarize`` for the ESS of the means)."""
    mo = cross_moments(x, chains_per_group=chains_per_group, **kw)
    cov = _cov_of(mo, ddof)
    var = torch.diagonal(mo["m2"], dim1=-2, dim2=-1)
    root = torch.sqrt(torch.where(torch.isfinite(var) & (var > 0), var, torch.full_like(var, float("nan"))))
    corr = (mo["m2"] / root.unsqueeze(-1) / root.unsqueeze(-2)).clamp(-1.0, 1.0)
    eye = torch.eye(corr.shape[-1], dtype=torch.bool, device=corr.device)
    corr = torch.where(eye & ~torch.isnan(corr), torch.ones_like(corr), corr)
    return {"n": mo["n"], "mean": mo["mean"], "cov": cov, "sd": torch.sqrt(torch.diagonal(cov, dim1=-2, dim2=-1)), "corr": corr,
            "m2": mo["m2"]}


def contrasts(moments, L, ddof=1):
    """Posterior mean, sd and covariance of the linear combinations ``L q`` from a ``cross_moments`` / ``covariance`` result ->
    dict(mean[G, k], sd[G, k], cov[G, k, k]); ``L`` is [k, d] (the same contrasts for every posterior) or [G, k, d]. The
    covariance is the result's own ``cov`` if it has one, else ``m2 / (n - ddof)``. An ungrouped result ([d], [d, d]) gives
    [k], [k], [k, k]. Small torch matmuls on the result's device; works on CPU tensors too."""
    mean = moments["mean"]
    cov = moments["cov"] if "cov" in moments else _cov_of(moments, ddof)
    L = torch.as_tensor(L, dtype=torch.float64, device=mean.device)
    single = mean.dim() == 1
    if single:
        mean, cov = mean.unsqueeze(0), cov.unsqueeze(0)
    if L.dim() == 2:
        L = L.unsqueeze(0).expand(mean.shape[0], -1, -1)
    if L.dim() != 3 or L.shape[0] != mean.shape[0] or L.shape[2] != mean.shape[1]:
        raise ValueError("L must be [k, %d] or [%d, k, %d] (got %s)" % (mean.shape[1], mean.shape[0], mean.shape[1], tuple(L.shape)))
    cm = torch.matmul(L, mean.unsqueeze(-1)).squeeze(-1)
    cc = torch.matmul(torch.matmul(L, cov), L.transpose(1, 2))
    cc = 0.5 * (cc + cc.transpose(1, 2))
    out = {"mean": cm, "sd": torch.sqrt(torch.diagonal(cc, dim1=-2, dim2=-1)), "cov": cc}
    return {k: v[0] for k, v in out.items()} if single else out
