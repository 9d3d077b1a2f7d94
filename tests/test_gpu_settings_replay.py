"""-m gpu: the eleven sampler settings OFF their defaults, replayed iteration by iteration against the oracle in every kernel
family that reads them -- the pair / quad forms (lmc_sampler.hpp), the leaf form of the general and dense kernels
(lmc_tree_leaf.hpp), the tick machine (lmc_tick.hpp) -- and through the host plumbing step -> Engine -> lmc_config ->
SamplerParams (tests/test_settings_config_cpu.py holds the host half without a device).

The cases are tests/_settings_cases.py: CASES; the first seven are chains of the reference (tests/golden/e2e_set_<case>.npz, the
oracle held to them bit for bit by tests/test_oracle_golden.py). Every replay is the harness's (tests/_replay.py) under its own
rule tables, at most 2 iterations skipped by the rules' margins, and every replay first asserts on the ORACLE's chain that the
case still does what it is for. A replay with one of the case's keywords left at its default on the device must fail
(test_a_case_fails_without_its_keyword): a kernel or a launch that ignored the setting would pass everything else."""
import functools
import os

import numpy as np
import pytest

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi
from oracle import lmc_oracle as orc
from oracle import targets as OT
from tests._gpu_util import device_target, kwargs_from
from tests._replay import Rules, assert_replay, dense_rules, record_chain, run_snapshots
from tests._settings_cases import ABOUT, CASES, GOLDEN, NUTS_CASES, SEED, assert_the_case_does_what_it_is_for, dense_matrix, stats_of

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAX_SKIPPED = 2            # iterations a replay may leave to the rules' margins: a condition on the cases, not a knob
SEEDS = orc.derive_seeds(SEED, 2)
# The fixed dense matrices: dense_matrix(d, seed). The seed is the dimension (as tests/test_gpu_dense.py seeds its own) except
# for emax_funnel, whose first trajectories from the jittered start leave the funnel with |energy error| > 1000 under most
# matrices: 4 is the first seed under which the oracle's chain keeps every divergence below 1000 with both potentials
# (oracle only; the oracle skips 0 iterations under dense_rules with each of these).
MATRIX_SEED = {"emax_funnel": 4, "depth_caps": 10, "low_accept": 16, "hmc_caps": 10, "hmc_emax": 8}
DENSE_CASES = list(MATRIX_SEED)
TICK_CASES = ["da_params", "emax_funnel", "depth_caps", "fixed_step", "hmc_caps", "hmc_emax"]


@pytest.fixture(autouse=True)
def _golden_sdot(monkeypatch):
    """The float32 start energy in the capture host's summation order (tests/test_gpu_parity.py)."""
    from littlemcmc_amd import engine

    monkeypatch.setattr(engine, "DEFAULT_SDOT", "skylakex")


def _oracle_step(name, potential):
    """(oracle step, start) of a case; ``potential``: None (the default diagonal adaptation), "full" or "inv"."""
    case = CASES[name]
    f = OT.make(case.family, case.d)
    start = orc.jitter_start(SEEDS[0], case.d)
    if potential is not None:
        pot = orc.quad_potential(dense_matrix(case.d, MATRIX_SEED[name]), potential == "full")
        return orc.Step(f, case.d, kind=case.kind, potential=pot, **case.kw), start
    if case.kind == "hmc":
        return orc.Step(f, case.d, kind="hmc", **case.kw), start
    start_, ostep = orc.init_nuts(f, case.d, seeds=SEEDS, **case.kw)
    np.testing.assert_array_equal(start_, start)
    return ostep, start


@functools.lru_cache(maxsize=None)
def oracle_chain(name, potential=None):
    """(snaps, outs) of the oracle's chain on SEEDS[0], recorded once per (case, potential) and shared by every replay of it;
    asserted to do what the case is for and, for a captured case on its own potential, to be the reference's chain."""
    case = CASES[name]
    ostep, start = _oracle_step(name, potential)
    snaps, outs = record_chain(ostep, start, np.random.RandomState(SEEDS[0]), case.tune, case.draws)
    assert_the_case_does_what_it_is_for(name, stats_of(outs), case.tune)
    if potential is None and name in GOLDEN:
        g = np.load(os.path.join(GOLDEN_DIR, "e2e_set_%s.npz" % name))
        assert (str(g["family"]), int(g["d"]), str(g["kind"]), int(g["tune"]), int(g["draws"])) == case[:3] + case[4:]
        assert kwargs_from(g) == {k: (v if isinstance(v, int) and not isinstance(v, bool) else float(v)) for k, v in case.kw.items()}
        np.testing.assert_array_equal(g["seeds"], SEEDS)
        np.testing.assert_allclose(np.array([o["q"] for o in outs]), g["trace"][0], rtol=1e-9, atol=1e-300)
        np.testing.assert_array_equal(np.array([o["stats"]["diverging"] for o in outs]), g["stat_diverging"][0, :, 0])
    return snaps, outs


def device_step(name, tgt=None, potential=None, drop=(), **extra):
    """The device step of a case on ``tgt`` (default: the built-in density), with the keywords ``drop`` left at their defaults."""
    case = CASES[name]
    tgt = device_target(case.family, case.d, OT.make(case.family, case.d).params()) if tgt is None else tgt
    kw = {k: v for k, v in case.kw.items() if k not in drop}
    kw.update(extra)
    cls = lmc.HamiltonianMC if case.kind == "hmc" else lmc.NUTS
    if potential is not None:
        mat = dense_matrix(case.d, MATRIX_SEED[name])
        return cls(tgt, case.d, potential=lmc.QuadPotentialFull(mat) if potential == "full" else lmc.QuadPotentialFullInv(mat), **kw)
    if case.kind == "hmc":
        return cls(tgt, case.d, **kw)
    start, step = lmc.init_nuts(tgt, case.d, random_seed=SEEDS, **kw)
    np.testing.assert_array_equal(start, orc.jitter_start(SEEDS[0], case.d))
    return step


def replay(name, step, rules, label, potential=None, expect=None):
    """One replay of the case's oracle chain on ``step``; ``expect``: what DeviceIterations.kernels must report."""
    snaps, outs = oracle_chain(name, potential)
    ran = run_snapshots(step, snaps, rules.dense_fields)
    for key, want in (expect or {}).items():
        assert ran.kernels(key) == {want}, (label, key, ran.engines)
    res = assert_replay(ran, snaps, outs, rules, "%s (%s)" % (name, label))
    print("%s (%s): checked %d skipped %d; worst position %.3g / statistic %.3g of the tolerance; %s" % (
        name, label, res.checked, res.skipped, res.worst_q, res.worst_stat, ran.engines[0]))
    assert res.skipped <= MAX_SKIPPED and res.checked == len(outs) - res.skipped, res
    return ran


@pytest.mark.parametrize("name", list(CASES))
def test_fused_kernels_on_the_default_plan(name):
    ran = replay(name, device_step(name), Rules.diag(), "fused", expect={"wide": False})
    if name == "depth_caps_team":
        assert {shape[2] for shape in ran.kernels("shape")} == {4}, ran.engines     # four wavefronts per chain


@pytest.mark.parametrize("group,plan", [("2", "shallow"), ("2", "deep"), ("4", "shallow"), ("4", "deep")])
@pytest.mark.parametrize("name", NUTS_CASES)
def test_fused_kernels_in_both_leaf_groups_and_lds_plans(name, group, plan, monkeypatch):
    """Leaf pairs and leaf quads (LMC_LEAF_GROUP, as tests/test_gpu_leaf_quads.py pins them) under both LDS plans: whichever
    the default plan of a shape is, the other one runs here."""
    monkeypatch.setenv("LMC_LEAF_GROUP", group)
    replay(name, device_step(name, lds_plan=plan), Rules.diag(), "leaf group %s, plan %s" % (group, plan),
           expect={"wide": False, "leaf": int(group), "plan": plan})


@pytest.mark.parametrize("name", GOLDEN)
def test_general_kernels(name, monkeypatch):
    """LMC_FORCE_WIDE=1 (tests/test_gpu_wide.py): the leaf form of the tree, HMC and dual averaging of the general kernels."""
    monkeypatch.setenv("LMC_FORCE_WIDE", "1")
    replay(name, device_step(name), Rules.diag(), "general", expect={"wide": True})


@pytest.mark.parametrize("potential,coop,expect", [("full", "1", "shared"), ("full", "0", "per_chain"), ("inv", "1", "per_chain")])
@pytest.mark.parametrize("name", DENSE_CASES)
def test_dense_kernels_with_a_fixed_matrix(name, potential, coop, expect, monkeypatch):
    """Both dense kernels are reachable at these sizes with the selection the suite already has: QuadPotentialFull runs the
    shared-matrix kernel, LMC_DENSE_COOP=0 sends it to the per-chain kernel (tests/test_gpu_dense_shapes.py), and
    QuadPotentialFullInv always runs the per-chain kernel. The momentum of QuadPotentialFull is float32-born:
    dense_rules(True); QuadPotentialFullInv: dense_rules(False)."""
    monkeypatch.setenv("LMC_DENSE_COOP", coop)
    rules = dense_rules(potential == "full")
    snaps, outs = oracle_chain(name, potential)
    assert sum(rules.skips(o) for o in outs) <= MAX_SKIPPED     # the oracle's own count, before anything runs
    replay(name, device_step(name, potential=potential), rules, "dense %s -> %s" % (potential, expect), potential=potential,
           expect={"dense": expect, "wide": False})


def _torch_target(name):
    from tests.test_gpu_torch_target import torch_funnel, torch_std_normal

    case = CASES[name]
    return {"std_normal": torch_std_normal, "funnel": torch_funnel}[case.family](case.d)


@pytest.mark.parametrize("name", TICK_CASES)
def test_tick_machine(name):
    """A torch callable (the funnel through autograd): the tick machine restates the Emax test, the depth choice and the
    max_steps clamp itself (lmc_tick.hpp)."""
    step = device_step(name, tgt=_torch_target(name))
    assert step._logp_dlogp_func.family == _abi.TARGET_EXTERNAL
    replay(name, step, Rules.diag(), "ticks", expect={"wide": False})


@pytest.mark.parametrize("name,drop", [(n, d) for n in ABOUT for d in ABOUT[n]], ids=lambda v: v if isinstance(v, str) else "+".join(v))
def test_a_case_fails_without_its_keyword(name, drop):
    """The oracle's chain has the keywords; the device step is built without the one(s) the case is about. The same
    assert_replay must fail -- otherwise the case would not notice a kernel that ignored the setting."""
    snaps, outs = oracle_chain(name)
    ran = run_snapshots(device_step(name, drop=drop), snaps)
    with pytest.raises(AssertionError) as failure:
        assert_replay(ran, snaps, outs, Rules.diag(), "%s without %s" % (name, "+".join(drop)))
    print("%s without %s: %s" % (name, "+".join(drop), str(failure.value)[:300]))


# ---- dual averaging beyond the host tables ----------------------------------------------------------------------------------
def _late_dual_averaging_chain():
    """Ten tuning iterations of std_normal d = 10 with k = 0.6 whose dual-averaging count starts at 16 380: the snapshots carry
    da_count 16 380 .. 16 389 and cross the 16 384 entries of the host-built sqrt(count) / count ** -k tables
    (lmc_engine.hip: da_table_len), after which the device's own sqrt and pow serve (lmc_sampler.hpp: dual_average_update)."""
    d, kw, seed = 10, dict(k=0.6), SEEDS[1]
    f = OT.make("std_normal", d)
    start, ostep = orc.init_nuts(f, d, seeds=[seed], **kw)

    def late(step):
        step.adapt.count = 16380

    snaps, outs = record_chain(ostep, start, np.random.RandomState(seed), 10, 0, after_reset=late)
    assert [s["da_count"] for s in snaps] == list(range(16380, 16390))
    return d, kw, seed, start, snaps, outs


@pytest.mark.parametrize("path", ["fused", "ticks"])
def test_dual_averaging_beyond_the_host_tables(path):
    from tests.test_gpu_torch_target import torch_std_normal

    d, kw, seed, start, snaps, outs = _late_dual_averaging_chain()
    tgt = torch_std_normal(d) if path == "ticks" else lmc.targets.StdNormal(d)
    start_d, step = lmc.init_nuts(tgt, d, random_seed=[seed], **kw)
    np.testing.assert_array_equal(start, start_d)
    ran = run_snapshots(step, snaps)
    res = assert_replay(ran, snaps, outs, Rules.diag(), "late dual averaging (%s)" % path)
    print("late dual averaging (%s): checked %d skipped %d" % (path, res.checked, res.skipped))
    assert res.skipped == 0 and res.checked == 10, res
