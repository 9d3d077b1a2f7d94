"""Where a subtree-stack level lives is decided once per NODE (lmc_sampler.hpp: level_node_load / level_node_store /
level_vec_load): levels 1..nlds in LDS, the others in the chain's scratch row, addressed as a wave-uniform base + the lane
offset + an immediate. The same job under every placement the engine accepts must give the same bits: trace, every sampler
statistic, the counters and the generator state.

Per case 8 chains, tune 30 + draws 30, and a start step size small enough that trees of depth >= 7 are built (asserted from
the depth statistic): a subtree of depth D parks nodes at the levels up to D - 1, so the deepest level that is certainly
parked in a run whose deepest tree has depth K is K - 3 (the last doubling, a subtree of depth K - 1, may stop before it
parks anything; the one before it completed) and no level above K - 2 is ever parked. A placement with nlds below K - 3
copies a proposal position from an LDS level into a scratch-row level when it parks, and reads it back from the row at
acceptance; a placement with nlds >= K - 1 keeps the whole stack in LDS.

Placements: lds_levels = 1, the default count n0, n0 + 1, n0 + 2 and the largest count that fits the 160 KB of LDS a
workgroup may use (max_treedepth, the whole stack, where that fits), the engine's own choice (lds_plan "auto"), and both
pinned LDS plans where the shape has them (one-wave kernels).

The four-wave team (d = 1000) holds 32 KB per level after a 67 KB head: 160 KB end at nlds = 3, so NO placement can have nlds
above the deepest parked level of a depth-7 tree there. Whether the stack fits decides what is asserted, not the shape: where
it cannot fit, the largest count that does (1, 2, 3 for that team) must have run, each with parked levels on both sides of nlds.

Equality among placements that share one bug proves nothing by itself: this stands next to the oracle replay
(tests/test_gpu_round6.py, tests/test_gpu_reference_suite.py), it does not replace it."""
import numpy as np
import pytest

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi
from littlemcmc_amd import targets as T

pytestmark = pytest.mark.gpu

CHAINS, TUNE, DRAWS = 8, 30, 30
LDS_LIMIT = 160 * 1024   # per workgroup, the generator / team-exchange tail behind the stack included


def _job(tgt, d, kw, lds_levels=0, lds_plan="auto"):
    n = TUNE + DRAWS
    seeds = lmc.distributed.global_seeds(23, CHAINS)
    start = 2.0 * np.random.RandomState(5).rand(d) - 1.0
    eng = lmc.Engine(tgt, chains=CHAINS, lds_levels=lds_levels, lds_plan=lds_plan, **kw)   # (an explicit lds_levels pins plan 0)
    eng.set_potential(start, np.ones(d), 10.0)
    try:
        eng.seed(seeds)
        eng.set_position(start)
        eng.reset_tuning()
        eng.reserve(n, keep_trace=True)
        eng.run(TUNE, 0, n)
        eng.synchronize()
        assert not eng.status().any()
        out = {"trace": eng.trace().copy()}
        for name in ("STEP_SIZE", "STEP_SIZE_BAR", "ACCEPT", "ENERGY_ERROR", "ENERGY", "MAX_ENERGY_ERROR", "MODEL_LOGP"):
            out[name] = eng.stat_f64(getattr(_abi, "STAT_" + name), 0, n).copy()
        for name in ("DEPTH", "TREE_SIZE"):
            out[name] = eng.stat_i32(getattr(_abi, "STAT_" + name), 0, n).copy()
        for name in ("DIVERGING", "TUNE", "ACCEPTED"):
            out[name] = eng.stat_u8(getattr(_abi, "STAT_" + name), 0, n).copy()
        out["rng"] = [(st[1].tobytes(),) + tuple(st[2:]) for st in (eng.get_rng_state(c) for c in range(CHAINS))]
        out["counters"] = np.delete(eng.counters(), _abi.CT_WAVE_TICKS, axis=1)   # (residence time: not a result)
        return out, eng.run_lds_bytes(), eng.kernel_shape(), eng.last_run_plan()
    finally:
        eng.close()


def _assert_same(ref, out, what):
    for key in ref:
        if isinstance(ref[key], np.ndarray):
            np.testing.assert_array_equal(ref[key], out[key], err_msg="%s: %s" % (what, key))
        else:
            assert ref[key] == out[key], (what, key)


# step_scale: the start step size is step_scale / d^0.25 (base_hmc.py); a twentieth of the default builds depth >= 7 trees from
# the first iterations on, before the dual averaging has brought the step size up
@pytest.mark.parametrize("family,d,kw,waves", [
    ("ar1", 128, {}, 1),                            # NS 2: quads, and the pinned pair form below
    ("std_normal", 64, {}, 1),                      # NS 1
    ("funnel", 256, {"max_treedepth": 8}, 1),       # NS 4, pair form
    ("diag", 300, {}, 2),                           # two-wave team
    ("diag", 1000, {}, 4),                          # four-wave team
])
def test_results_do_not_depend_on_the_placement_of_any_stack_level(monkeypatch, family, d, kw, waves):
    tgt = {"ar1": lambda: T.AR1(d, 0.9), "std_normal": lambda: T.StdNormal(d), "funnel": lambda: T.Funnel(d),
           "diag": lambda: T.DiagGaussian(np.linspace(0.5, 2.0, d))}[family]()
    kw = dict(kw, step_scale=0.25 / 20.0)
    max_depth = kw.get("max_treedepth", 10)

    ref, lds1, shape, _plan = _job(tgt, d, kw, lds_levels=1)   # (run_lds_bytes: what the launch asked for, tail included)
    assert shape[2] == waves
    per_level = 4 * 64 * shape[1] * shape[2] * 8            # {lp, rp, psum, q} of 64 * NS * W doubles
    deepest_tree = int(ref["DEPTH"].max())
    print("%s d=%d: kernel shape %s, lds_levels=1 -> %d B, %d B per level, deepest tree %d, tree sizes up to %d"
          % (family, d, shape, lds1, per_level, deepest_tree, ref["TREE_SIZE"].max()))
    assert deepest_tree >= 7
    parked_for_sure, parked_at_most = deepest_tree - 3, deepest_tree - 2

    default = _job(tgt, d, kw, lds_plan="shallow" if waves == 1 else "auto")
    n0 = 1 + (default[1] - lds1) // per_level
    assert default[1] == lds1 + (n0 - 1) * per_level and 1 <= n0 <= max_depth
    _assert_same(ref, default[0], "default count (%d)" % n0)
    ran = {1, n0}
    most = min(max_depth, 1 + (LDS_LIMIT - lds1) // per_level)   # the largest count a workgroup's LDS holds: the whole stack where it fits
    for levels in (n0 + 1, n0 + 2, most):
        if levels in ran or levels > most:
            continue
        got = _job(tgt, d, kw, lds_levels=levels)
        assert got[1] == lds1 + (levels - 1) * per_level   # the levels really moved
        _assert_same(ref, got[0], "lds_levels=%d" % levels)
        ran.add(levels)
    _assert_same(ref, _job(tgt, d, kw)[0], "the engine's own choice (lds_plan auto)")   # what a caller gets
    if waves == 1:
        plans = set()
        for plan in ("shallow", "deep"):
            got = _job(tgt, d, kw, lds_plan=plan)
            _assert_same(ref, got[0], "plan " + plan)
            plans.add(got[3])
        assert plans == {"shallow", "deep"}   # every one-wave shape here has both plans, and each launch ran the pinned one
        if shape[1] <= 2:   # leaf quads by default: the pair form runs through the same accessors
            monkeypatch.setenv("LMC_LEAF_GROUP", "2")
            for levels in (1, n0 + 1):
                _assert_same(ref, _job(tgt, d, kw, lds_levels=levels)[0], "leaf pairs, lds_levels=%d" % levels)
            monkeypatch.delenv("LMC_LEAF_GROUP")

    print("  placements run: nlds in %s; parked levels: certainly up to %d, at most %d" % (sorted(ran), parked_for_sure, parked_at_most))
    assert min(ran) < parked_for_sure        # LDS level -> scratch-row level copies of q, and the read back at acceptance
    if lds1 + parked_at_most * per_level <= LDS_LIMIT:   # levels 2 .. parked_at_most + 1 fit behind lds_levels = 1's bytes
        assert max(ran) > parked_at_most     # the whole stack in LDS
    else:
        # no placement can hold the stack (the four-wave team): the largest count that fits ran, below the deepest parked level
        assert max(ran) == most == 1 + (LDS_LIMIT - lds1) // per_level and 2 <= most <= parked_at_most
