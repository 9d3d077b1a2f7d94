"""-m gpu: per-group target parameters (targets.Batched) -- many posteriors in one job. One yardstick for every sample()
comparison: the chains of group g of the grouped job equal, bit for bit (trace and every statistic), the chains of the same
indices of ``sample(batched[g], ...)`` run with the same per-chain seeds and the same chain count -- the ungrouped runs are
what the parity tests pin to the oracle. Tiny jobs: at most 24 chains, explicit seed lists, nothing discarded."""
import numpy as np
import pytest

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi
from littlemcmc_amd import targets as T

pytestmark = pytest.mark.gpu
SEEDS = [1000 + 37 * c for c in range(24)]
TUNE, DRAWS = 30, 15


def _sample(target, chains, step=None, **kw):
    """One seeded job; ``step``: None or a factory target -> step object (a fresh one per job)."""
    args = dict(draws=DRAWS, tune=TUNE, chains=chains, random_seed=SEEDS[:chains], discard_tuned_samples=False,
                progressbar=False)
    args.update(kw)
    return lmc.sample(target, target.d, step=None if step is None else step(target), **args)


def _assert_chains_equal(got, want, sl=slice(None), rows=slice(None)):
    """got[sl] == want[sl, rows]: trace and every statistic, bit for bit."""
    (trace, stats), (wtrace, wstats) = got[:2], want[:2]
    np.testing.assert_array_equal(trace[sl], wtrace[sl, rows])
    assert set(stats) == set(wstats)
    for name in wstats:
        assert stats[name].dtype == wstats[name].dtype, name
        np.testing.assert_array_equal(stats[name][sl], wstats[name][sl, rows], err_msg=name)


def _assert_groups_are_their_members(batched, chains, grouped, step=None, **kw):
    """THE yardstick: group g's chains of ``grouped`` are those chain indices of sample(batched[g], same seeds, same chains).
    Also: the groups did not all see row 0 (members differ, so their chains must)."""
    assert grouped[0].shape[0] == chains
    for g, sl in enumerate(batched.chain_slices(chains)):
        _assert_chains_equal(grouped, _sample(batched[g], chains, step, **kw), sl)


def _ar1_ladder(d=16, rhos=(0.0, 0.5, 0.9, -0.7)):
    return T.Batched([T.AR1(d, rho=r) for r in rhos])


def _diag_pair(d):
    return T.Batched([T.DiagGaussian(np.linspace(0.5, 2.0, d)), T.DiagGaussian(np.linspace(3.0, 0.25, d))])


# ---- 1. unit kernels ---------------------------------------------------------------------------------------------------
def test_unit_kernels_evaluate_every_chain_on_its_own_row():
    from oracle import targets as OT

    d, chains = 5, 6
    precs = [np.linspace(0.5, 2.0, d), np.linspace(4.0, 1.0, d), np.full(d, 0.125)]
    b = T.Batched([T.DiagGaussian(p) for p in precs])
    rs = np.random.RandomState(4)
    q, p = rs.randn(chains, d), rs.randn(chains, d)
    var = np.linspace(0.5, 1.5, d)
    with lmc.Engine(b, chains=chains) as eng:
        assert eng.target_groups() == (3, d, 0, 2)
        eng.set_potential(np.zeros(d), var, 10.0)
        logp, grad = eng.logp_dlogp(q)
        traj = eng.trajectory(q, p, 0.1, 3, 0, p0_is_f32=False)
        same, _ = eng.logp_dlogp(q[0])          # ONE point for all chains: one value per group, three different values
        assert same[0] == same[1] and same[2] == same[3] and same[4] == same[5] and len(set(same.tolist())) == 3
    for g, sl in enumerate(b.chain_slices(chains)):
        with lmc.Engine(b[g], chains=chains) as one:
            assert one.target_groups() == (1, d, 0, chains)
            one.set_potential(np.zeros(d), var, 10.0)
            wl, wg = one.logp_dlogp(q)
            wt = one.trajectory(q, p, 0.1, 3, 0, p0_is_f32=False)
        np.testing.assert_array_equal(logp[sl], wl[sl])
        np.testing.assert_array_equal(grad[sl], wg[sl])
        for name in wt:
            np.testing.assert_array_equal(traj[name][sl], wt[name][sl], err_msg=name)
        f = OT.DiagGaussian(precs[g])     # (tests/test_gpu_units.py::test_logp_dlogp_matches_oracle_targets: same tolerances)
        for c in range(chains)[sl]:
            ol, og = f(q[c])
            np.testing.assert_allclose(logp[c], ol, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(grad[c], og, rtol=1e-13, atol=1e-13)
    with lmc.Engine(b, chains=3, first_chain=3, chains_per_group=2) as part:      # chains 3, 4, 5 of the job: rows 1, 2, 2
        lp, _ = part.logp_dlogp(q[3:])
        np.testing.assert_array_equal(lp, logp[3:])


# ---- 2. fused one-wave NUTS ---------------------------------------------------------------------------------------------
_cache = {}


def _ar1_grouped():
    """Test 2's plain grouped job, computed once and shared (never modified)."""
    if "ar1" not in _cache:
        trace, stats = _sample(_ar1_ladder(), 8)
        trace.setflags(write=False)
        _cache["ar1"] = (trace, stats)
    return _cache["ar1"]


@pytest.mark.parametrize("kw", [dict(lds_plan=0), dict(lds_plan=1), dict(rng="counter")], ids=["plan0", "plan1", "counter"])
def test_fused_one_wave_nuts(kw):
    b = _ar1_ladder()
    trace, stats, eng = _sample(b, 8, return_engine=True, **kw)
    try:
        assert not eng.wide and eng.kernel_shape()[1:] == (1, 1) and eng.rng == kw.get("rng", "numpy")
        if kw.get("lds_plan") == 0:
            assert eng.last_run_plan() == "shallow"
    finally:
        eng.close()
    _assert_groups_are_their_members(b, 8, (trace, stats), **kw)
    assert not np.array_equal(trace[0:2], trace[2:4])
    if "lds_plan" in kw:     # the plans are bit-identical: the shared plain job is the same job
        _assert_chains_equal((trace, stats), _ar1_grouped())


# ---- 3. fused teams -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, waves", [(257, 2), (513, 4)])
def test_fused_teams(d, waves):
    b, kw = _diag_pair(d), dict(tune=20, draws=10, max_treedepth=5)
    trace, stats, eng = _sample(b, 4, return_engine=True, **kw)
    try:
        assert not eng.wide and eng.kernel_shape()[2] == waves
    finally:
        eng.close()
    _assert_groups_are_their_members(b, 4, (trace, stats), **kw)


# ---- 4. general kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d, waves", [(5, 1), (513, 16)])
def test_general_kernels(d, waves):
    def step(target):
        return lmc.NUTS(target, d, potential=lmc.QuadPotentialDiagAdapt(d, np.zeros(d), np.ones(d), 10, dtype="float64"),
                        max_treedepth=5)

    b, kw = _diag_pair(d), dict(tune=20, draws=10)
    trace, stats, eng = _sample(b, 4, step, return_engine=True, **kw)
    try:
        assert eng.wide and eng.kernel_shape()[2] == waves
    finally:
        eng.close()
    _assert_groups_are_their_members(b, 4, (trace, stats), step, **kw)


# ---- 5. dense, per-chain adaptive -----------------------------------------------------------------------------------------
def test_dense_per_chain_adaptive():
    d = 8
    b = T.Batched([T.DiagGaussian(np.linspace(0.5, 2.0, d) * s) for s in (1.0, 3.0, 0.2)])
    trace, stats, eng = _sample(b, 6, init="adapt_full", return_engine=True)
    try:
        assert eng.last_run_dense_kernel() == "per_chain"
    finally:
        eng.close()
    _assert_groups_are_their_members(b, 6, (trace, stats), init="adapt_full")


# ---- 6. dense shared matrix: the eight-chains-per-workgroup kernel ------------------------------------------------------------
def test_dense_shared_matrix_workgroups_hold_chains_of_different_groups():
    d = 8
    idx = np.arange(d)
    cov = 0.5 ** np.abs(idx[:, None] - idx[None, :])

    def step(target):
        return lmc.NUTS(target, d, potential=lmc.QuadPotentialFull(cov))

    b = _ar1_ladder(d)          # 4 groups of 3 chains: workgroup 0 holds chains 0-7 (groups 0, 1, 2), workgroup 1 chains 8-11
    trace, stats, eng = _sample(b, 12, step, return_engine=True)
    try:
        assert eng.last_run_dense_kernel() == "shared"
    finally:
        eng.close()
    _assert_groups_are_their_members(b, 12, (trace, stats), step)


# ---- 7. HMC -----------------------------------------------------------------------------------------------------------------
def test_hmc():
    def step(target):
        return lmc.HamiltonianMC(target, 1, path_length=1.0)

    b = T.Batched([T.Normal1D(0.0, 1.0), T.Normal1D(3.0, 0.5), T.Normal1D(-2.0, 4.0)])
    trace, stats, eng = _sample(b, 6, step, return_engine=True)
    try:
        assert eng.kind == "hmc"
    finally:
        eng.close()
    _assert_groups_are_their_members(b, 6, (trace, stats), step)


# ---- 8. run-time compiled density -------------------------------------------------------------------------------------------
def test_run_time_compiled_density_with_a_padded_stride():
    """One parameter per group (nu in P[0]): rows of one double, two doubles apart on the device."""
    d = 7
    b = T.Batched([T.UserTarget.separable(d, logp="-0.5*(P[0]+1.0)*log1p(q*q/P[0])", grad="-(P[0]+1.0)*q/(P[0]+q*q)",
                                          params=[nu]) for nu in (3.0, 8.0, 30.0)])
    trace, stats, eng = _sample(b, 6, return_engine=True)
    try:
        assert eng.target.family == _abi.TARGET_USER and not eng.wide and eng.target_groups() == (3, 1, 0, 2)
    finally:
        eng.close()
    _assert_groups_are_their_members(b, 6, (trace, stats))


# ---- 9. device blocks that cut a group --------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices, per", [([0, 0], 2), ([0, 0, 0], 7)], ids=["blocks_3_3", "blocks_7_7_7"])
def test_device_blocks_that_cut_a_group(devices, per):
    """devices=[0, 0] with 6 chains in 3 groups: blocks 3 + 3, group 1 = chains 2, 3 spans both engines. Three engines of
    7 chains with 7 per group: every block is one group, found by its offset alone."""
    b = T.Batched([T.AR1(16, rho=r) for r in (0.0, 0.6, 0.9)])
    chains = 3 * per
    one = _sample(b, chains, device=0)
    trace, stats, eng = _sample(b, chains, devices=devices, return_engine=True)
    try:
        per_engine = [e.target_groups() for e in eng.engines]
        assert [t[2] for t in per_engine] == [lo for lo, _hi in eng.blocks] and all(t[3] == per for t in per_engine)
    finally:
        eng.close()
    _assert_chains_equal((trace, stats), one)
    if per == 2:
        _assert_groups_are_their_members(b, chains, one)


# ---- 10. launch splitting and outputs ---------------------------------------------------------------------------------------
def test_launch_splitting_and_thinned_streamed_outputs():
    b, plain = _ar1_ladder(), _ar1_grouped()
    _assert_chains_equal(_sample(b, 8, launch_iters=7), plain)
    _assert_chains_equal(_sample(b, 8, thin=3, stream_results="windows"), plain, rows=slice(None, None, 3))
    _assert_chains_equal(_sample(b, 8, thin=3, stream_results="windows", launch_iters=7), plain, rows=slice(None, None, 3))


# ---- 11. guard: grouping does not change arithmetic -----------------------------------------------------------------------
def test_identical_members_equal_the_ungrouped_job():
    member = T.AR1(16, rho=0.9)
    grouped = _sample(T.Batched([T.AR1(16, rho=0.9) for _ in range(4)]), 8)
    _assert_chains_equal(grouped, _sample(member, 8))


def test_step_methods_refuse_one_point_calls():
    b = _ar1_ladder()
    with pytest.raises(TypeError, match=r"batched\[g\]"):
        b(np.zeros(16))
    with pytest.raises(ValueError, match=r"batched\[g\]"):
        lmc.NUTS(b, 16)._astep(np.zeros(16))
    logp, grad = b[1](np.ones(16))
    assert np.isfinite(logp) and grad.shape == (16,)
