"""rng="counter" on the device (include/lmc_hip.h: LMC_RNG_COUNTER): every random number of a transition is a pure function
of (chain seed, iteration, index). The device's streams are held to the host model (tests/_counter_model.py), every
iteration is replayed against the unchanged oracle driven by that model, and the mode is held to what a pure function
promises: independence of launch slicing and chain blocks, an untouched MT19937 state, the target's moments."""
import numpy as np
import pytest

import littlemcmc_amd as lmc
from littlemcmc_amd import _abi
from littlemcmc_amd import targets as T
from oracle import lmc_oracle as orc
from oracle import targets as OT
from tests import _counter_model as cm
from tests import _glm_oracle as GO
from tests._gpu_util import device_target
from tests._replay import Rules, assert_replay, record_chain, run_keyed_iterations

pytestmark = pytest.mark.gpu

SEED = 20260928

# Largest |device normal - float64 Box-Muller of the same words| measured on an MI355X over the draws of
# test_device_streams_are_the_models (8 chains x 5 iterations x d in {1, 64, 65, 200, 600}): the error of v_log_f32 /
# v_sin_f32 / v_cos_f32 / v_sqrt_f32 and of the float32 products behind one normal.
NORMALS_MEASURED_MAX_ABS = 4.774e-07


def test_device_streams_are_the_models():
    """Engine.counter_draws against the model: the decision uniforms bit for bit (300 = five refills of the 64-wide window),
    the normals against the float64 Box-Muller of the same Philox words within 4x the largest difference measured
    (NORMALS_MEASURED_MAX_ABS = 4.774e-07 on an MI355X, i.e. a bound of 1.91e-06), at iterations on both sides of 2^32 and at every kernel shape (d = 1: one live lane;
    64 / 65: one and two elements per lane; 200: four; 600: a team of four wavefronts). Elements of a lane beyond d are
    never handed out (the kernels hold 0 there): the result has exactly d columns, float32-valued and finite."""
    chains = 8
    seeds = lmc.distributed.global_seeds(SEED, chains)
    worst = 0.0
    for d in (1, 64, 65, 200, 600):
        eng = lmc.NUTS(T.StdNormal(d), d, rng="counter")._make_engine(chains)
        try:
            eng.seed(seeds)
            for git in (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5):
                normals, uniforms = eng.counter_draws(git, n_uniforms=300)
                assert normals.shape == (chains, d) and uniforms.shape == (chains, 300)
                for c in range(chains):
                    np.testing.assert_array_equal(uniforms[c], cm.uniforms(seeds[c], git, 300), err_msg="d=%d git=%d chain %d" % (d, git, c))
                    want = cm.normals(seeds[c], git, d)
                    worst_here = float(np.abs(normals[c] - want).max())
                    worst = max(worst, worst_here)
                    assert np.all(normals[c] == normals[c].astype(np.float32)) and np.all(np.isfinite(normals[c]))
                only_normals, none = eng.counter_draws(git)
                np.testing.assert_array_equal(only_normals, normals)
                assert none.shape == (chains, 0)
        finally:
            eng.close()
    print("counter_draws normals: max |device - float64 model| = %.3e" % worst)
    assert worst <= 4.0 * NORMALS_MEASURED_MAX_ABS, worst
    # the momentum-only mode has the same momentum stream; the numpy stream has none to show
    eng = lmc.NUTS(T.StdNormal(65), 65, momentum_rng="philox")._make_engine(chains)
    try:
        eng.seed(seeds)
        np.testing.assert_allclose(eng.counter_draws(3)[0][1], cm.normals(seeds[1], 3, 65), rtol=0, atol=4.0 * NORMALS_MEASURED_MAX_ABS)
    finally:
        eng.close()
    eng = lmc.NUTS(T.StdNormal(65), 65)._make_engine(chains)
    try:
        with pytest.raises(_abi.HipLibraryError, match="error 1: .*LMC_RNG_NUMPY"):
            eng.counter_draws(0, n_uniforms=4)
    finally:
        eng.close()


# ---- every iteration against the oracle ----------------------------------------------------------------------------------
_USER_STD_NORMAL = dict(logp="-0.5*q*q", grad="-q")
# name -> (family, d, chains K, iterations T, iterations that tune, kind, extra)
CASES = {
    "ar1_16": ("ar1", 16, 24, 40, 40, "nuts", {}),
    "std_normal_1": ("std_normal", 1, 8, 40, 20, "nuts", {}),                 # one live lane
    "ar1_65": ("ar1", 65, 8, 30, 30, "nuts", {}),                              # NS = 2, just past one element per lane
    "funnel_8": ("funnel", 8, 8, 40, 20, "nuts", {}),
    "ar1_200": ("ar1", 200, 4, 24, 24, "nuts", {}),                            # NS = 4
    "ar1_300": ("ar1", 300, 2, 16, 8, "nuts", {}),                             # W = 2
    "diag_gaussian_600": ("diag_gaussian", 600, 2, 16, 16, "nuts", {}),        # W = 4, sigma^2 spanning 1e4
    "hmc_std_normal_10": ("std_normal", 10, 8, 40, 20, "hmc", {}),
    "ar1_16_jitter": ("ar1", 16, 8, 40, 40, "nuts", {"jitter": (0.8, 1.2)}),   # k = 0 is drawn before the tree
    "std_normal_70_scaling": ("std_normal", 70, 8, 40, 20, "nuts", {"scaling": 1.3}),   # float64 momentum
    "user_std_normal_16": ("std_normal", 16, 8, 40, 40, "nuts", {"user": True}),        # run-time compiled density
    # targets.GLM: family "glm" names a cell (N, d, likelihood) of tests/_glm_model.py instead of an oracle family
    "glm_63_3_bernoulli": ("glm", 3, 8, 30, 30, "nuts", {"glm": (63, 3, "bernoulli")}),
    "glm_130_130_poisson": ("glm", 130, 4, 20, 10, "nuts", {"glm": (130, 130, "poisson")}),   # NS = 4, divergences
}
_REPLAYED = {}


def _steps(family, d, kind, extra, seeds, mode=(("rng", "counter"),)):
    """(device step, factory of oracle steps, start). ``mode``: the keyword that selects the stream (this file's is
    rng="counter"; tests/test_gpu_philox_replay.py builds the same cases with momentum_rng="philox")."""
    mode = dict(mode)
    if "glm" in extra:   # the float64 statement of the posterior in the device's order, and the targets.GLM of the same cell
        assert family == "glm" and extra["glm"][1] == d
        f, make_target, _info = GO.oracle_glm(*extra["glm"])
        tgt = make_target()
    else:
        f = OT.make(family, d)
        tgt = T.UserTarget.separable(d, **_USER_STD_NORMAL) if extra.get("user") else device_target(family, d, f.params())
    jit = extra.get("jitter")
    start = orc.jitter_start(seeds[0], d)
    if kind == "hmc":
        step = lmc.HamiltonianMC(tgt, d, **mode)
        ostep = lambda: orc.Step(f, d, kind="hmc", potential=orc.DiagAdaptPotential(d, np.zeros(d), np.ones(d), 10))   # noqa: E731
    elif "scaling" in extra:
        var = np.full(d, extra["scaling"])
        step = lmc.NUTS(tgt, d, scaling=var, is_cov=True, **mode)
        ostep = lambda: orc.Step(f, d, kind="nuts", scaling=var, is_cov=True)   # noqa: E731
    else:
        kw = {} if jit is None else {"step_rand": lmc.base_hmc.StepRandUniform(*jit)}
        start_dev, step = lmc.init_nuts(tgt, d, random_seed=seeds, **mode, **kw)
        np.testing.assert_array_equal(start_dev, start)
        ostep = lambda: orc.init_nuts(f, d, seeds=seeds, **({} if jit is None else {"step_rand": jit}))[1]   # noqa: E731
    return step, ostep, start


def _replay(name):
    """Replay every iteration of K oracle chains of case ``name`` on the device; memoised. Returns a dict of counts."""
    if name in _REPLAYED:
        return _REPLAYED[name]
    family, d, K, n_it, n_tune, kind, extra = CASES[name]
    seeds = lmc.distributed.global_seeds(SEED, K)
    step, make_ostep, start = _steps(family, d, kind, extra, seeds)
    eng = step._make_engine(K)
    try:
        eng.seed(seeds)                      # once: the streams are keyed by these seeds and nothing else
        rng_before = [eng.get_rng_state(c) for c in range(K)]
        normals = np.stack([eng.counter_draws(t)[0] for t in range(n_it)])      # [T, K, d]: the device's own normals
        chains, used = [], []
        for c in range(K):
            rng = cm.CounterRng(seeds[c], normals[:, c])
            chains.append(record_chain(make_ostep(), start, rng, n_tune, n_it - n_tune))
            used.append(rng.finish())
        used = np.array(used)                # [K, T] uniforms the oracle consumed
        ran = run_keyed_iterations(step, eng, [snaps for snaps, _outs in chains], n_tune)
        # the chains' MT19937 state was never touched
        for c in range(K):
            now = eng.get_rng_state(c)
            np.testing.assert_array_equal(now[1], rng_before[c][1])
            assert now[2:] == rng_before[c][2:]
        shape, lds = eng.kernel_shape(), eng.run_lds_bytes()
    finally:
        eng.close()
    done = [assert_replay(ran[c], snaps, outs, Rules.diag(), "%s chain %d" % (name, c))
            for c, (snaps, outs) in enumerate(chains)]
    res = dict(checked=sum(r.checked for r in done), fragile=sum(r.skipped for r in done), total=K * n_it, max_used=int(used.max()), over128=int((used > 128).sum()),
               over256=int((used > 256).sum()), shape=shape, lds=lds)
    print("%s: %s" % (name, res))
    _REPLAYED[name] = res
    return res


@pytest.mark.parametrize("name", list(CASES))
def test_every_iteration_replays_against_the_oracle(name):
    """For every iteration t of K chains: the oracle's pre-iteration state goes into ONE engine of K chains, seeded once,
    eng.run(n_tune, t, 1) runs iteration t, and positions (rtol 1e-11), float statistics (1e-10), integer statistics (exact)
    and the adaptation state (against the oracle's next snapshot) equal the oracle's, which runs UNCHANGED on
    CounterRng(seed, the device's normals). An iteration whose oracle margin is below 1e-9 is skipped."""
    res = _replay(name)
    assert res["checked"] + res["fragile"] == res["total"]
    assert res["fragile"] <= max(1, res["total"] // 100), res
    want_shape = {"ar1_200": (4, 1), "ar1_300": (4, 2), "diag_gaussian_600": (4, 4), "ar1_65": (2, 1), "std_normal_1": (1, 1),
                  "glm_63_3_bernoulli": (1, 1), "glm_130_130_poisson": (4, 1)}.get(name)
    if want_shape is not None:
        assert res["shape"][1:] == want_shape, res


def test_replay_covers_window_refills_and_skips_next_to_nothing():
    """Over all cases: at most 1 % of the iterations were skipped for a margin below 1e-9, and the replayed iterations
    include one that consumed more than 128 uniforms and one that consumed more than 256 (several refills of the
    device's 64-wide window inside one transition)."""
    res = [_replay(name) for name in CASES]
    total, fragile = sum(r["total"] for r in res), sum(r["fragile"] for r in res)
    print("replayed %d iterations, %d skipped; most uniforms in one iteration %d; %d over 128, %d over 256" % (
        total, fragile, max(r["max_used"] for r in res), sum(r["over128"] for r in res), sum(r["over256"] for r in res)))
    assert fragile * 100 <= total, (fragile, total)
    assert sum(r["over128"] for r in res) >= 1 and sum(r["over256"] for r in res) >= 1


# ---- what a pure function promises -----------------------------------------------------------------------------------
def test_slicing_chain_blocks_and_the_generator_state_do_not_matter():
    d, chains, tune, draws = 200, 96, 40, 15
    tgt = T.AR1(d, 0.9)
    seeds = lmc.distributed.global_seeds(7, chains)
    start, step = lmc.init_nuts(tgt, d, random_seed=seeds, rng="counter")
    full, sfull, eng = lmc.sample(tgt, d, draws=draws, tune=tune, chains=chains, random_seed=seeds, start=start, step=step,
                                  launch_iters=1000, return_engine=True)
    try:
        # the job left every chain's MT19937 state as lmc_engine_seed made it
        fresh = lmc.NUTS(tgt, d)._make_engine(chains)
        try:
            fresh.seed(seeds)
            for c in range(chains):
                a, b = eng.get_rng_state(c), fresh.get_rng_state(c)
                np.testing.assert_array_equal(a[1], b[1])
                assert a[2:] == b[2:], c
        finally:
            fresh.close()
    finally:
        eng.close()
    _s, step2 = lmc.init_nuts(tgt, d, random_seed=seeds, rng="counter")
    cut, scut = lmc.sample(tgt, d, draws=draws, tune=tune, chains=chains, random_seed=seeds, start=start, step=step2, launch_iters=7)
    np.testing.assert_array_equal(cut, full)
    np.testing.assert_array_equal(scut["tree_size"], sfull["tree_size"])
    lo, hi = lmc.distributed.chain_block(chains, 1, 3)
    _s, step3 = lmc.init_nuts(tgt, d, random_seed=seeds, rng="counter")
    part, spart = lmc.sample(tgt, d, draws=draws, tune=tune, chains=hi - lo, random_seed=seeds[lo:hi], start=start, step=step3,
                             launch_iters=7)
    np.testing.assert_array_equal(part, full[lo:hi])
    np.testing.assert_array_equal(spart["tree_size"], sfull["tree_size"][lo:hi])
    # its own draws: neither the reference's stream nor the momentum-only mode's
    for kw in ({}, {"momentum_rng": "philox"}):
        _s, other = lmc.init_nuts(tgt, d, random_seed=seeds, **kw)
        ref, _ = lmc.sample(tgt, d, draws=draws, tune=tune, chains=8, random_seed=seeds[:8], start=start, step=other)
        assert not np.allclose(ref, full[:8]), kw
    assert np.isfinite(full).all() and abs(full.var() - 1.0) < 0.5


# ---- it samples the target -------------------------------------------------------------------------------------------
def _pooled_moments(mean, m2, n):
    n = np.asarray(n, dtype="d")[:, None]
    tot = n.sum()
    grand = (mean * n).sum(axis=0) / tot
    ss = m2.sum(axis=0) + (n * (mean - grand) ** 2).sum(axis=0)
    return grand, ss / (tot - 1.0)


def test_counter_mode_samples_the_target_at_scale():
    """Shape and bounds of tests/test_gpu_scale.py's momentum-only test: 65 536 chains x d = 128 standard normal, every pooled
    mean and variance within 2e-3 after 600 draws per chain, median depth 3, no status bit."""
    d, chains, tune, draws = 128, 65536, 300, 600
    tgt = T.StdNormal(d)
    seeds = lmc.distributed.global_seeds(SEED, chains)
    start, step = lmc.init_nuts(tgt, d, random_seed=seeds, rng="counter")
    eng = step._make_engine(chains)
    try:
        eng.seed(seeds); eng.set_position(start); eng.reset_tuning(); eng.keep_moments(True)
        eng.reserve(tune + draws, keep_trace=False)
        eng.run(tune, 0, tune + draws)
        eng.synchronize()
        assert not eng.status().any()
        mean, m2, n = eng.moments()
        gmean, gvar = _pooled_moments(np.asarray(mean), np.asarray(m2), n)
        depth = eng.stat_i32(_abi.STAT_DEPTH, tune, draws)
    finally:
        eng.close()
    print("counter mode: max |mean| %.2e, max |var - 1| %.2e, median depth %g" % (
        np.abs(gmean).max(), np.abs(gvar - 1.0).max(), np.median(depth)))
    assert np.abs(gmean).max() < 2e-3 and np.abs(gvar - 1.0).max() < 2e-3
    assert np.median(depth) == 3


@pytest.mark.parametrize("kind,d", [("hmc", 10), ("nuts_fixed_diag", 70), ("nuts_team", 600)])
def test_counter_mode_other_paths(kind, d):
    """The three other paths of test_counter_based_momentum_stream_other_paths, with that test's tolerances."""
    chains = 2048 if d < 100 else 512
    tgt = T.StdNormal(d)
    if kind == "hmc":
        step = lmc.HamiltonianMC(tgt, d, path_length=2.0, rng="counter")
    elif kind == "nuts_fixed_diag":
        step = lmc.NUTS(tgt, d, scaling=np.full(d, 1.3), is_cov=True, rng="counter")
    else:
        step = lmc.NUTS(tgt, d, rng="counter")
    trace, stats = lmc.sample(tgt, d, draws=300, tune=300, step=step, chains=chains, random_seed=5)
    assert np.isfinite(trace).all() and not stats["diverging"].any()
    n = chains * 300
    assert np.abs(trace.mean(axis=(0, 1))).max() < 6.0 / np.sqrt(n) + 5e-3
    assert np.abs(trace.var(axis=(0, 1)) - 1.0).max() < 0.03


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_refusals_name_the_mode():
    d = 16
    with pytest.raises(_abi.HipLibraryError, match="LMC_RNG_COUNTER"):
        lmc.NUTS(T.StdNormal(d), d, potential=lmc.QuadPotentialFull(np.eye(d)), rng="counter")._make_engine(4)
    with pytest.raises(_abi.HipLibraryError, match="LMC_RNG_COUNTER"):
        lmc.NUTS(T.StdNormal(2000), 2000, rng="counter")._make_engine(4)
    import torch

    fn = lambda q: (-0.5 * (q * q).sum(dim=1), -q)   # noqa: E731
    with pytest.raises(_abi.HipLibraryError, match="LMC_RNG_COUNTER"):
        lmc.NUTS(T.TorchTarget(d, fn), d, rng="counter")._make_engine(4)
    assert torch.cuda.is_available()
