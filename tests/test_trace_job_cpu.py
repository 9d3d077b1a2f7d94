"""No-GPU checks of what every pass over the trace shares (littlemcmc_amd/diagnostics.py): the job constructor ``_trace_job``
against a brute-force enumeration of chains and groups, its switches and refusals on the inputs the five passes' own CPU tests
refuse, and the fan-out ``_fan_out`` with its three combiners against a per-group fold of the same parts."""
import numpy as np
import pytest
import torch

from littlemcmc_amd import diagnostics as dg
from littlemcmc_amd import predictive
from littlemcmc_amd import targets as T

from . import _predictive_model as P


def _cut(x, sizes):
    edges = np.cumsum([0] + list(sizes))
    return [x[a:b] for a, b in zip(edges[:-1], edges[1:])]


# ---- (a) blocks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 3])
@pytest.mark.parametrize("per", [1, 2, 4, None])
@pytest.mark.parametrize("sizes", [[4], [3, 0, 5], [0, 2, 2]])
def test_job_equals_brute_force_enumeration(sizes, per, first):
    x = torch.zeros((sum(sizes), 5, 2), dtype=torch.float64)
    job = dg._trace_job(_cut(x, sizes), per, first, allow_first_chain=True)
    # brute force: every chain's job index and group, block by block
    p = per if per is not None else first + sum(sizes)
    chain, firsts, groups = first, [], []
    for s in sizes:
        if s:
            firsts.append(chain)
        for _ in range(s):
            groups.append(chain // p)
            chain += 1
    assert job.firsts == firsts and [int(b.shape[0]) for b in job.held] == [s for s in sizes if s]
    assert (job.chains, job.per, job.n_draws, job.d, job.device) == (sum(sizes), p, 5, 2, x.device)
    assert (job.g0, job.groups) == (min(groups), len(set(groups))) == dg._touched(first, sum(sizes), p)
    if len(sizes) == 1:   # one tensor is the list of one block
        assert dg._trace_job(x, per, first, allow_first_chain=True)[1:] == job[1:]


# ---- (b) switches and refusals ----------------------------------------------------------------------------------------------
def _batched(G_=3, N=5, d=3):
    rng = np.random.default_rng(0)
    return T.Batched([T.GLM(rng.standard_normal((N, d)), rng.standard_normal(N), "gaussian", prior_scale=1.0 + g, sigma=0.5 + g)
                      for g in range(G_)])


X12 = torch.zeros((12, 4, 3), dtype=torch.float64)     # 3 groups of 4: the job of test_predictive_cpu / test_psis_cpu
X6 = torch.zeros((6, 4, 3), dtype=torch.float64)       # 3 groups of 2: test_linpred_cpu
X15 = torch.zeros((15, 61, 70), dtype=torch.float64)   # 3 groups of 5: test_quantiles_cpu


def test_whole_groups_refuses_a_group_that_straddles_blocks():
    tgt = _batched()
    for blocks in ([X12[:6], X12[6:]],):                                  # test_psis_cpu: loo, pointwise_loglik
        with pytest.raises(ValueError, match="straddles"):
            dg._trace_job(blocks, None, 0, tgt, whole_job=True, whole_groups=True)
        assert dg._trace_job(blocks, None, 0, tgt, whole_job=True).firsts == [0, 6]     # predict, the select: a group may straddle
    for blocks in ([X12[:4], X12[4:]], [X12[:8], X12[8:8], X12[8:]], X12):
        assert dg._trace_job(blocks, None, 0, tgt, whole_job=True, whole_groups=True).per == 4


def test_whole_job_refuses_chains_that_are_not_all_posteriors():
    tgt = _batched()
    with pytest.raises(ValueError, match="needs a multiple of"):          # test_quantiles_cpu: no target
        dg._trace_job(X15, 4, whole_job=True)
    assert dg._trace_job(X15, 4).groups == 4                               # a block of a job: the last group partly
    with pytest.raises(ValueError, match="multiple of 3 chains"):         # test_linpred_cpu (Batched.group_size)
        dg._trace_job(X6[:5], None, 0, tgt, whole_job=True)
    with pytest.raises(ValueError, match="multiple"):                     # test_psis_cpu, test_predictive_cpu
        dg._trace_job(X12[:11], None, 0, tgt, whole_job=True, whole_groups=True)
    with pytest.raises(ValueError, match="posteriors of the target"):     # predict(chains_per_group=) that is not chains / G
        dg._trace_job(X12[:8], 4, 0, tgt, whole_job=True)
    assert dg._trace_job(X12[:8], 4, 0, tgt).groups == 2                   # pointwise_stats: the first two groups
    assert dg._trace_job(X6[:2], None, 0, tgt[0], whole_job=True).per == 2  # one GLM: one group of all chains


def test_allow_first_chain():
    tgt = _batched()
    with pytest.raises(ValueError, match="first_chain"):                  # test_predictive_cpu: a list is the whole job
        dg._trace_job([X12[:6], X12[6:]], None, 2, tgt, allow_first_chain=False)
    with pytest.raises(ValueError, match="first_chain"):
        dg._trace_job(X12, None, 2, tgt)
    job = dg._trace_job(X12[6:], 4, 6, tgt, allow_first_chain=True)
    assert (job.g0, job.groups, job.firsts) == (1, 2, [6])
    with pytest.raises(ValueError, match="needs chains_per_group"):       # a Batched block inside the job
        dg._trace_job(X12[6:], None, 6, tgt, allow_first_chain=True)
    assert dg._trace_job(X12[:2], None, 3, tgt[0], allow_first_chain=True).per == 5   # one GLM: one group, whatever starts
    assert dg._trace_job([X12[:6], X12[6:]], 5, 7, allow_first_chain=True).firsts == [7, 13]   # chain_stats_pass


def test_shape_and_target_refusals(monkeypatch):
    tgt = _batched()
    with pytest.raises(ValueError, match="x has d = 2"):
        dg._trace_job(torch.zeros((12, 4, 2), dtype=torch.float64), None, 0, tgt)
    with pytest.raises(ValueError, match="reach group"):
        dg._trace_job(X12, 2, 0, tgt)
    for cpg, first in ((0, 0), (4, -1)):
        with pytest.raises(ValueError, match="chains_per_group"):
            dg._trace_job(X12, cpg, first, tgt, allow_first_chain=True)
    with pytest.raises(ValueError, match="differ in d"):                  # test_quantiles_cpu
        dg._trace_job([X15[:5], X15[5:, :, :3]], 5, whole_job=True)
    with pytest.raises(ValueError, match="different numbers of draws"):
        dg._trace_job([X15[:5], X15[5:, :7]], 5)
    for empty in (X15[:0], X15[:, :0], X15[:, :, :0], [], [X15[:0], X15[:0]], X15[0]):
        with pytest.raises(ValueError):
            dg._trace_job(empty)
    import torch.distributed as dist

    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    with pytest.raises(ValueError, match="process group"):
        dg._trace_job(X15, 5)


# ---- (c) the fan-out --------------------------------------------------------------------------------------------------------
CUTS = ([6], [2, 4], [3, 3], [1, 0, 5])   # [3, 3] cuts inside group 1; 6 chains, 3 groups of 2
PER, N_OBS = 2, 7


@pytest.fixture(scope="module")
def draws():
    return torch.as_tensor(np.random.default_rng(3).standard_normal((6, 9, N_OBS)))


def _per_group(b, first, fn):
    """[groups the part touches, ...]: fn of the draws [S, N] of every group's chains present in the part."""
    g0, touched = dg._touched(first, int(b.shape[0]), PER)
    cuts = [min(max((g0 + i) * PER - first, 0), int(b.shape[0])) for i in range(touched + 1)]
    return torch.stack([fn(b[lo:hi].reshape(-1, N_OBS).numpy()) for lo, hi in zip(cuts[:-1], cuts[1:])])


def _counts(v):
    return torch.as_tensor(np.stack([(v > 0).sum(axis=0), (v <= 0).sum(axis=0)]).astype(np.int64))


def _planes(v):
    return torch.as_tensor(P.planes_of(v, np.exp(v)))


def _moments(v):
    mu = 1.0 / (1.0 + np.exp(-v))
    return torch.as_tensor(np.stack([np.full(N_OBS, float(len(v))), v.mean(axis=0), ((v - v.mean(axis=0)) ** 2).sum(axis=0),
                                     mu.mean(axis=0), ((mu - mu.mean(axis=0)) ** 2).sum(axis=0)]))


def _fold_by_group(x, sizes, fn, combine):
    """What the passes did before they shared a fan-out, stated per group: the parts of the blocks that hold chains of the
    group, in job order, folded into zeros."""
    out, first = [], 0
    parts = []
    for b in _cut(x, sizes):
        if b.shape[0]:
            parts.append((first // PER, _per_group(b, first, fn)))
        first += int(b.shape[0])
    for g in range(3):
        acc = torch.zeros_like(parts[0][1][0])
        for g0, p in parts:
            if g0 <= g < g0 + p.shape[0]:
                acc = combine(acc, p[g - g0])
        out.append(acc)
    return torch.stack(out)


@pytest.mark.parametrize("sizes", CUTS)
@pytest.mark.parametrize("fn,combine", [(_counts, torch.add), (_planes, predictive.merge), (_moments, predictive.merge_moments)],
                         ids=["add", "merge", "merge_moments"])
def test_fan_out_folds_the_parts_in_job_order(draws, sizes, fn, combine):
    job = dg._trace_job(_cut(draws, sizes), PER)
    seen = []

    def call(b, first):
        seen.append((first, int(b.shape[0])))
        return _per_group(b, first, fn)

    got = dg._fan_out(job, 0, 3, call, combine)
    want = _fold_by_group(draws, sizes, fn, combine)
    assert got.dtype == want.dtype and torch.equal(got, want)
    assert seen == [(f, int(b.shape[0])) for b, f in zip(job.held, job.firsts)]      # every block once, whole, in job order
    whole = _per_group(draws, 0, fn)
    if combine is torch.add:    # integer counts: every cut gives the bits of the uncut job
        assert torch.equal(got, whole)
    else:                       # a Chan merge: groups that lie inside one block come through bit for bit
        first = np.cumsum([0] + list(sizes))
        for g in range(3):
            if any(a <= g * PER and (g + 1) * PER <= b for a, b in zip(first[:-1], first[1:])):
                assert torch.equal(got[g], whole[g]), g
        assert torch.equal(got[:, 0], whole[:, 0])                                   # the counts always
    # a sub-range of groups: only the chains of those groups are handed out, and the result is that slice
    del seen[:]
    sub = dg._fan_out(job, 1, 3, call, combine)
    assert torch.equal(sub, got[1:]) and sum(c for _f, c in seen) == 4 and min(f for f, _c in seen) == 2


def test_the_passes_fold_as_before_through_their_injected_models():
    """pointwise_stats on a list == the per-group fold of its stats_fn parts with merge (the loop it had of its own)."""
    tgt = _batched()
    x = torch.as_tensor(np.random.default_rng(1).standard_normal((12, 6, 3)))
    table = np.ascontiguousarray(tgt.params, dtype=np.float64).reshape(3, -1)
    for sizes in ([12], [6, 6], [5, 0, 7], [1, 11]):
        st = tgt.pointwise_stats(_cut(x, sizes), stats_fn=P.stats_fn)
        tot, first = torch.zeros((3, 6, 5), dtype=torch.float64), 0
        for b in _cut(x, sizes):
            if b.shape[0]:
                blk = P.stats_fn(b, table, first, 4)[..., :5]
                off = first // 4
                tot[off:off + blk.shape[0]] = predictive.merge(tot[off:off + blk.shape[0]], blk)
            first += int(b.shape[0])
        assert all(torch.equal(st[k], tot[:, i]) for i, k in enumerate(predictive.PLANES)), sizes
