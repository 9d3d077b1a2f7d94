"""Leaf quads (lmc_sampler.hpp: nuts_transition2<.., G = 4>) against leaf pairs (G = 2) on the same seeds: the quad form
applies the decisions of four leaves in the pair form's order, keeps every sum's summation tree and every uniform's place in
the stream, so draws, sampler statistics and generator positions are equal bit for bit."""
import numpy as np
import pytest

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi
from littlemcmc_amd import targets as T

pytestmark = pytest.mark.gpu


def _job(monkeypatch, group, tgt, d, chains, n, lds_plan, kw):
    monkeypatch.setenv("LMC_LEAF_GROUP", group)   # struct lmc_tuning.leaf_group, read by the host (engine.tuning_from_env)
    seeds = lmc.distributed.global_seeds(11, chains)
    start, step = lmc.init_nuts(tgt, d, random_seed=seeds, lds_plan=lds_plan, **kw)
    eng = step._make_engine(chains)
    try:
        eng.seed(seeds)
        eng.set_position(start)
        eng.reset_tuning()
        eng.reserve(n, keep_trace=True)
        for first in range(0, n, 60):
            eng.run(n // 2, first, min(60, n - first))
            eng.synchronize()
        assert not eng.status().any()
        assert eng.last_run_leaf_group() == int(group)   # the launches really ran the pinned form
        out = {"trace": eng.trace().copy()}
        for name in ("STEP_SIZE", "STEP_SIZE_BAR", "ACCEPT", "ENERGY_ERROR", "ENERGY", "MAX_ENERGY_ERROR", "MODEL_LOGP"):
            out[name] = eng.stat_f64(getattr(_abi, "STAT_" + name), 0, n).copy()
        for name in ("DEPTH", "TREE_SIZE"):
            out[name] = eng.stat_i32(getattr(_abi, "STAT_" + name), 0, n).copy()
        for name in ("DIVERGING", "TUNE", "ACCEPTED"):
            out[name] = eng.stat_u8(getattr(_abi, "STAT_" + name), 0, n).copy()
        out["rng"] = [(st[1].tobytes(),) + tuple(st[2:]) for st in (eng.get_rng_state(c) for c in range(chains))]
        out["counters"] = np.delete(eng.counters(), _abi.CT_WAVE_TICKS, axis=1)   # (residence time: not a result)
        return out, eng.run_lds_bytes()
    finally:
        eng.close()


@pytest.mark.parametrize("family,d,plan,kw", [
    ("ar1", 128, "shallow", {}), ("ar1", 128, "deep", {}),                  # C3's target: depth 6-7 trees
    ("std_normal", 128, "shallow", {}), ("std_normal", 128, "deep", {}),
    ("std_normal", 64, "shallow", {}), ("std_normal", 64, "deep", {}),
    ("funnel", 100, "shallow", {}), ("funnel", 60, "deep", {}),             # divergences: the quads' sequential path
])
def test_leaf_quads_are_bit_identical_to_leaf_pairs(monkeypatch, family, d, plan, kw):
    tgt = {"ar1": lambda: T.AR1(d, 0.9), "funnel": lambda: T.Funnel(d), "std_normal": lambda: T.StdNormal(d)}[family]()
    chains, n = 64, 240   # the first 200 iterations run under early_max_treedepth
    pair, lds2 = _job(monkeypatch, "2", tgt, d, chains, n, plan, kw)
    quad, lds4 = _job(monkeypatch, "4", tgt, d, chains, n, plan, kw)
    if d <= 64 and plan == "shallow":
        assert lds2 != lds4   # the pinned form really is the other kernel (one element per lane: the layouts differ in size)
    if family == "ar1":
        assert pair["TREE_SIZE"].max() >= 64   # depth >= 6 trees happened
    if family == "funnel":
        # a diverging transition stops in its last subtree (depth - 1) after tree_size - (2^(depth-1) - 1) of its leaves: some
        # must stop at leaf 1, 2 or 3 of a quad -- the sequential path with the speculative leaves after the diverging one
        div = pair["DIVERGING"].astype(bool)
        sub = pair["DEPTH"][div].astype(np.int64) - 1
        at = pair["TREE_SIZE"][div].astype(np.int64) - ((1 << sub) - 1) - 1   # index of the diverging leaf in its subtree
        assert ((sub >= 2) & (at % 4 != 0)).any() and ((sub >= 2) & (at % 4 == 0)).any()
    for key in pair:
        if isinstance(pair[key], np.ndarray):
            np.testing.assert_array_equal(pair[key], quad[key], err_msg=key)
        else:
            assert pair[key] == quad[key], key
    # CT_LEAPFROGS counts accepted leaves only: the sum of the recorded tree sizes (tests/test_gpu_scale.py), in either form
    assert quad["counters"][:, _abi.CT_LEAPFROGS].sum() == quad["TREE_SIZE"].astype(np.int64).sum()
