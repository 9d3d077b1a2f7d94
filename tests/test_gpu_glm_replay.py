"""-m gpu: a targets.GLM transition in every kernel that runs one, against the oracle.

tests/test_gpu_glm.py holds the functor alone (Engine.logp_dlogp, Engine.trajectory) to a 50-digit reference. A job evaluates
GLMTarget<NS>::logp_grad inside other instantiations: the fused one-wave samplers run_kernel<1|2|4, 1, GLMTarget, ...> (both
LDS plans, leaf pairs and quads, the transition inlined by kInlineTransition), the general one-wave kernels
run_wide_kernel<1|2|4|8, 1> (256 < d <= 512, and every float64 mass diagonal), the dense kernels run_dense_kernel /
run_dense_coop_kernel, and the HMC transition. Here every iteration of an oracle chain on the float64 statement of the
posterior (tests/_glm_oracle.py over tests/_glm_model.logp_grad) is replayed on the device from the oracle's exact
pre-iteration state, with the harness and the rules every other family is replayed with (tests/_replay.py: Rules.diag() for
the diagonal masses, dense_rules for the dense ones; _glm_oracle.rules).

tests/test_glm_replay_cpu.py shows, without a device, that two independent statements of the posterior stay 500 times below
these tolerances, that three small errors fail them, and that no chain has more than two iterations under the skip floor.

Every case asserts the kernel that ran (LDS plan, leaf group, general / fused, dense kernel) and prints what it checked and its
worst position error in units of the tolerance. One oracle chain per cell, shared by the variants (_glm_oracle.oracle_chain)."""
import numpy as np
import pytest

from tests import _glm_model as M
from tests import _glm_oracle as GO
from tests._replay import assert_replay, run_snapshots

pytestmark = pytest.mark.gpu


def _diag_replay(c, label, **step_kw):
    """The memoised oracle chain of ``c`` on the device under Rules.diag(); prints checked / skipped, the worst position error
    in units of the tolerance (rtol 1e-11, atol 1e-12) and the kernels that ran. Returns (the device's iterations, outs)."""
    snaps, outs = GO.oracle_chain(c)
    step, _start = GO.device_step(c, **step_kw)
    ran = run_snapshots(step, snaps)
    res = assert_replay(ran, snaps, outs, GO.rules(c), label)
    total = c.tune + c.draws
    print("%s: checked %s skipped %s of %d; worst position error %.4g of the tolerance; plan %s leaf group %s general %s "
          "shape %s" % (label, res.checked, res.skipped, total, res.worst_q, sorted(map(str, ran.kernels("plan"))),
                        sorted(map(str, ran.kernels("leaf"))), sorted(ran.kernels("wide")), sorted(ran.kernels("shape"))))
    assert res.checked + res.skipped == total
    assert res.checked >= total - (2 if total >= 30 else 1), (label, res)
    assert len(ran.engines) == 2      # the tuning iterations and the draws
    return ran, outs


# ---- a. fused one-wave kernels, numpy rng: LDS plan x leaf group ----------------------------------------------------------------
def _fused_variants():
    for c in GO.FUSED:
        for plan in ("shallow", "deep"):
            for leaf in (("2", "4") if M.ns_for(c.d) <= 2 else (None,)):   # NS = 4 is built for pairs only: nothing to pin
                yield pytest.param(c, plan, leaf, id="%s-%s-%s" % (GO.case_id(c), plan, "pairs" if leaf == "2" else
                                                                   "quads" if leaf == "4" else "as_built"))


@pytest.mark.parametrize("c, plan, leaf", list(_fused_variants()))
def test_fused_kernels_replay_the_oracle(monkeypatch, c, plan, leaf):
    """run_kernel<NS, 1, GLMTarget, ..>: NS = 1, 2, 4, full and partial last blocks on both axes, under both LDS plans and
    both leaf groups. (65, 65, poisson) additionally holds the divergence path to the oracle: at least three diverging
    iterations, each with ``diverging``, ``tree_size`` and ``depth`` equal and -- where the oracle's transition stayed at its
    start, the proposal of the diverged tree rejected -- the position equal bit for bit."""
    if leaf is None:
        monkeypatch.delenv("LMC_LEAF_GROUP", raising=False)
    else:
        monkeypatch.setenv("LMC_LEAF_GROUP", leaf)   # struct lmc_tuning.leaf_group, read by the host (engine.tuning_from_env)
    label = "fused %s plan %s leaf %s" % (GO.case_id(c), plan, leaf)
    ran, outs = _diag_replay(c, label, lds_plan=plan)
    ns = M.ns_for(c.d)
    assert ran.kernels("wide") == {False} and ran.kernels("kind") == {"nuts"}, ran.kernels("wide")
    assert {s[1:] for s in ran.kernels("shape")} == {(ns, 1)}, ran.kernels("shape")
    assert ran.kernels("plan") == {plan}
    assert ran.kernels("leaf") == {2 if leaf is None else int(leaf)}, ran.kernels("leaf")
    if (c.N, c.d, c.lik) == (65, 65, "poisson"):
        snaps, _ = GO.oracle_chain(c)
        div = [i for i, o in enumerate(outs) if o["stats"]["diverging"]]
        assert len(div) >= 3, div
        stayed = 0
        for i in div:
            assert not GO.rules(c).skips(outs[i]), i      # none of them is among the skipped
            for name in ("diverging", "tree_size", "depth"):
                assert ran[i]["stats"][name] == outs[i]["stats"][name], (label, i, name)
            if np.array_equal(outs[i]["q"], snaps[i]["q"]):
                stayed += 1
                np.testing.assert_array_equal(ran.q[i], snaps[i]["q"], err_msg="%s iter %d" % (label, i))
        print("%s: %d diverging iterations replayed, %d of them stayed at their start" % (label, len(div), stayed))


def test_a_prior_scale_off_by_five_parts_in_ten_million_fails_the_replay():
    """The control on the device: the same replay with a targets.GLM whose prior precision is off by 1e-6 relative (the
    CPU test's third mutant, on every coefficient) is refused by assert_replay, and at least half of the tuning iterations miss
    the position tolerance -- the comparison really is between this device run and that oracle chain."""
    from littlemcmc_amd import targets as T

    c = next(k for k in GO.FUSED if (k.N, k.d, k.lik) == (63, 3, "bernoulli"))
    X, y, _ = M.case(c.N, c.d, c.lik)
    wrong = T.GLM(X, y, c.lik, prior_scale=M.PRIOR_SCALE * (1.0 + 5e-7), sigma=M.SIGMA)
    assert abs(wrong.tau / GO.TAU - 1.0) < 1.1e-6
    snaps, outs = GO.oracle_chain(c)
    step, _start = GO.device_step(c, target=wrong)
    ran = run_snapshots(step, snaps)
    with pytest.raises(AssertionError):
        assert_replay(ran, snaps, outs, GO.rules(c), "wrong prior scale")
    got = ran.q[:c.tune]                          # the tuning iterations
    missing = sum(not np.allclose(got[i], outs[i]["q"], rtol=1e-11, atol=1e-12) for i in range(c.tune))
    print("wrong prior scale: %d of %d tuning iterations miss the position tolerance" % (missing, c.tune))
    assert 2 * missing >= c.tune, missing


# ---- c. general one-wave kernels -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GO.WIDE, ids=GO.case_id)
def test_general_kernels_replay_the_oracle(c):
    """run_wide_kernel<8, 1>: d = 300 (two likelihoods), d = 512 (the last supported dimension: every slot of every lane
    live) and d = 257 (255 dead slots)."""
    ran, _outs = _diag_replay(c, "general %s" % GO.case_id(c))
    assert ran.kernels("wide") == {True} and M.ns_for(c.d) == 8
    assert {s[2] for s in ran.kernels("shape")} == {1}, ran.kernels("shape")      # one wavefront per chain


@pytest.mark.parametrize("c", GO.DIAG64, ids=GO.case_id)
def test_general_kernels_with_a_float64_diagonal_replay_the_oracle(c):
    """QuadPotentialDiagAdapt(dtype="float64") runs the general kernels at every dimension: run_wide_kernel<1|2|4, 1>."""
    ran, _outs = _diag_replay(c, "general float64 diagonal %s" % GO.case_id(c))
    assert ran.kernels("wide") == {True} and ran.kernels("mass_f64") == {True}
    assert {s[2] for s in ran.kernels("shape")} == {1}, ran.kernels("shape")


# ---- e. HMC -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", GO.HMC, ids=GO.case_id)
def test_hmc_replays_the_oracle(c):
    ran, outs = _diag_replay(c, "hmc %s" % GO.case_id(c))
    assert ran.kernels("kind") == {"hmc"} and ran.kernels("wide") == {False}
    assert {s[2] for s in ran.kernels("shape")} == {1}, ran.kernels("shape")      # one wavefront per chain
    assert max(o["stats"]["n_steps"] for o in outs) > 1


# ---- d. dense mass matrices -----------------------------------------------------------------------------------------------------
def _dense_replay(c, expect, label):
    snaps, outs = GO.oracle_chain(c)
    dstep, _start = GO.device_step(c)
    ran = run_snapshots(dstep, snaps)
    assert ran.kernels("dense") == {expect}, (label, ran.engines)
    res = assert_replay(ran, snaps, outs, GO.rules(c), label)
    total = c.tune + c.draws
    print("%s: kernel %s; checked %d skipped %d of %d; worst position %.3g / stat %.3g of the tolerance" % (
        label, expect, res.checked, res.skipped, total, res.worst_q, res.worst_stat))
    assert res.checked >= total - 1, res      # TUNE + DRAWS = 19 < 30


@pytest.mark.parametrize("c", GO.SHARED, ids=GO.case_id)
def test_shared_matrix_kernel_replays_the_oracle(c):
    """run_dense_coop_kernel<1|2> under QuadPotentialFull(inverse Hessian at 0): d = 3, 65 and 128 (the kernel's last)."""
    _dense_replay(c, "shared", "shared %s" % GO.case_id(c))


@pytest.mark.parametrize("c", GO.PER_CHAIN, ids=GO.case_id)
def test_per_chain_kernel_replays_the_oracle(c, monkeypatch):
    """run_dense_kernel<2|4, float|double>: QuadPotentialFull sent to it by LMC_DENSE_COOP=0, its float64 form, and
    QuadPotentialFullInv (the Hessian itself)."""
    if c.kind == "full":
        monkeypatch.setenv("LMC_DENSE_COOP", "0")
    _dense_replay(c, "per_chain", "per-chain %s" % GO.case_id(c))


@pytest.mark.parametrize("c", GO.ADAPT, ids=GO.case_id)
def test_adapted_dense_matrix_replays_the_oracle(c):
    """init="adapt_full": the estimators, the matrix and its factor go in through set_dense_state per iteration, and the
    matrix after the iteration is compared with the oracle's next snapshot (Rules.dense)."""
    _dense_replay(c, "per_chain", "adapt_full %s" % GO.case_id(c))
